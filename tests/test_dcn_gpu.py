"""Modulated deformable conv (DCNv2) on the GPU: scd_dcn_cols / scd_dcn_cols_bwd against the float64 restatement
(tests/dcn_ref.py), the DCN module and one DCN + BN + ReLU stage against torch, and the ResNet-DCN CenterNet.

Kernel bounds (derived by counting roundings before the first GPU run; u = 2^-24, u_T = 0 / 2^-8 / 2^-11 for
fp32 / bf16 / fp16; the restatement gets the same rounded inputs; S = its sum of absolute terms):
  cols with masks    8 u S + u_T |ref|
  cols with logits  12 u S + u_T |ref|        (expf 1 ulp = 2u, the sum u, the correctly rounded divide u)
  dom               (4 C/G + 8) u S + u_T |ref|,  bit-equal from call to call, pad channels 0
  dx32              (n_e + 8) u S,  n_e the restatement's count of contributions to the element

A finding of the first GPU run, kept as input design and not as a wider bound: below 2^-14 fp16 is subnormal, its
spacing is 2^-24 whatever the value, and u_T |ref| no longer covers the rounding to the storage type -- the float64
reference rounded to fp16 on the CPU misses the `cols` bound by the same factor (11.8 at ref = -4.4e-6) as the kernel
did with signed normal inputs.  The kernel tests therefore draw |x| in [0.5, 1.5] (signed in fp32 and bf16, positive
in fp16), masks in [0.125, 1) and logits in [-3, 3]: a non-zero fp16 column is then at least 0.5 * (1/8)^2 * 0.047,
far above 2^-14, and the forward test asserts that no reference column lies in fp16's subnormal range.
"""
import functools
import importlib
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dcn_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
UT = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
# (N,H,W,C,G) in the 16-bit types; the fp32 cases halve the channel counts (chunks of 4 instead of 8)
SHAPES = [(2, 5, 7, 8, 1), (2, 5, 7, 16, 2), (2, 5, 7, 64, 1), (2, 5, 7, 192, 1), (2, 5, 7, 512, 1), (1, 1, 1, 8, 1),
          (3, 33, 65, 64, 1)]
TOL_RMS, TOL_MEAN = 2.0 ** -3, 2.0 ** -6     # 16-bit groups against fp32 torch (tests/test_hourglass_gpu.py)


def _shape(shape, dtype):
    N, H, W, C, G = shape
    return (N, H, W, C // 2 if dtype == torch.float32 else C, G)


@functools.lru_cache(maxsize=None)
def _inputs(shape, dtype, sigmoid, grad, P=None):
    """Inputs rounded to `dtype`, as float64 CPU tensors: x, om (pad channels NaN: never read), dcols."""
    from scdhip import ops
    N, H, W, C, G = shape
    # the first seed of the case's sequence whose draw has the coverage every kernel test asserts (_classified)
    for seed in range(100 + H * W + C + G + int(sigmoid), 10 ** 6, 1000):
        g = torch.Generator().manual_seed(seed)
        off = R.draw_offsets(g, N, H, W, G, grad)
        none, part, full = R.classify(off, H, W, G)
        if (H, W) == (5, 7):
            if none >= 0.12 and part >= 0.12 and full >= 0.42:
                break
        elif R.cols_gather(torch.ones(N, H, W, G, dtype=torch.float64), off, torch.ones(N, H, W, 9 * G,
                                                                                       dtype=torch.float64), G).any():
            break                       # (a one-pixel image: some sample draws on the pixel)
    P = P or ops.dcn_om_channels(G, dtype)
    om = torch.full((N, H, W, P), float("nan"), dtype=torch.float64)
    om[..., :18 * G] = off
    m = torch.rand(N, H, W, 9 * G, dtype=torch.float64, generator=g)
    om[..., 18 * G:27 * G] = (m * 6 - 3) if sigmoid else 0.125 + 0.875 * m
    # magnitudes in [0.5, 1.5]; signed, except in fp16 (the module docstring's note on its subnormal range)
    x = 0.5 + torch.rand(N, H, W, C, dtype=torch.float64, generator=g)
    sign = torch.randint(0, 2, (N, H, W, C), generator=g).double() * 2 - 1
    if dtype != torch.float16:
        x = x * sign
    dcols = torch.randn(N, H, W, 9 * C, dtype=torch.float64, generator=g)
    rnd = lambda t: t.to(dtype).double()
    return rnd(x), rnd(om), rnd(dcols)


@functools.lru_cache(maxsize=None)
def _forward_ref(shape, dtype, sigmoid, P=None):
    x, om, _ = _inputs(shape, dtype, sigmoid, False, P)
    G = shape[4]
    off, m = R.split_om(om, G, sigmoid)
    ref = R.cols_gather(x, off, m, G)
    return ref, R.cols_gather(x.abs(), off, m.abs(), G)


def _classified(shape, off):
    N, H, W, C, G = shape
    none, part, full = R.classify(off, H, W, G)
    if (N, H, W) == (2, 5, 7):
        assert none >= 0.10 and part >= 0.10 and full >= 0.40, (none, part, full)
    elif (N, H, W) == (3, 33, 65):
        assert full >= 0.50, full


@pytest.mark.parametrize("sigmoid", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_dcn_cols_forward(dtype, shape, sigmoid):
    from scdhip import ops
    shape = _shape(shape, dtype)
    N, H, W, C, G = shape
    x, om, _ = _inputs(shape, dtype, sigmoid, False)
    _classified(shape, om[..., :18 * G])
    ref, s = _forward_ref(shape, dtype, sigmoid)
    got = ops.dcn_cols(x.to(dtype).to(DEV), om.to(dtype).to(DEV), G, sigmoid).cpu().double().view(N, H, W, 9, C)
    bound = (12 if sigmoid else 8) * U * s + UT[dtype] * ref.abs()
    err = (got - ref).abs()
    print("cols %s %s sigmoid=%d: worst err/bound %.3g" % (dtype, shape, sigmoid,
                                                           (err / bound.clamp_min(1e-300)).max().item()))
    assert torch.isfinite(got).all() and (err <= bound).all()
    assert ref.abs().max() > 0
    if dtype == torch.float16:
        assert not ((ref != 0) & (ref.abs() < 2.0 ** -14)).any()


def test_dcn_cols_wide_om():
    """P = 64: the pad channels [27G, P) are never read (they hold NaN)."""
    from scdhip import ops
    dtype, shape = torch.bfloat16, (2, 5, 7, 16, 2)
    x, om, _ = _inputs(shape, dtype, True, False, 64)
    assert om.shape[-1] == 64 and torch.isnan(om[..., 54:]).all()
    ref, s = _forward_ref(shape, dtype, True, 64)
    got = ops.dcn_cols(x.to(dtype).to(DEV), om.to(dtype).to(DEV), 2, True).cpu().double().view(ref.shape)
    assert ((got - ref).abs() <= 12 * U * s + UT[dtype] * ref.abs()).all()


@functools.lru_cache(maxsize=None)
def _backward_ref(shape, dtype, sigmoid, P=None):
    x, om, dcols = _inputs(shape, dtype, sigmoid, True, P)
    N, H, W, C, G = shape
    xr = x.clone().requires_grad_()
    omr = om[..., :27 * G].clone().requires_grad_()
    off, m = R.split_om(omr, G, sigmoid)
    d5 = dcols.view(N, H, W, 9, C)
    dx, dom = torch.autograd.grad(R.cols_gather(xr, off, m, G), (xr, omr), d5)
    # absolute sums.  dx: the same backward on |dcol| (masks and corner weights are >= 0)
    xa = x.clone().requires_grad_()
    (sx,) = torch.autograd.grad(R.cols_gather(xa, off.detach(), m.detach().abs(), G), xa, d5.abs())
    sdom = R.abs_terms_dom(d5, x, off.detach(), m.detach(), G)
    if sigmoid:
        sdom[..., 18 * G:] *= (m * (1 - m)).detach()
    return dx, dom, sx, sdom, R.dx_counts(off.detach(), x.shape, G)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_dcn_cols_backward(dtype, shape):
    from scdhip import ops
    shape = _shape(shape, dtype)
    N, H, W, C, G = shape
    sigmoid = True
    x, om, dcols = _inputs(shape, dtype, sigmoid, True)
    _classified(shape, om[..., :18 * G])
    dx, dom, sx, sdom, ne = _backward_ref(shape, dtype, sigmoid)
    args = [t.to(dtype).to(DEV) for t in (dcols.view(N, H, W, 9 * C), x, om)]
    dx32, gdom = ops.dcn_cols_bwd(*args, G, sigmoid)
    _, gdom2 = ops.dcn_cols_bwd(*args, G, sigmoid)
    assert dx32.dtype == torch.float32 and gdom.dtype == dtype and gdom.shape == om.shape
    assert torch.equal(gdom.view(torch.uint8), gdom2.view(torch.uint8)), "dom differs between two calls"
    assert not gdom[..., 27 * G:].any(), "pad channels of dom"
    gd = gdom[..., :27 * G].cpu().double()
    bd = (4 * C // G + 8) * U * sdom + UT[dtype] * dom.abs()
    ed = (gd - dom).abs()
    bx = (ne + 8) * U * sx
    ex = (dx32.cpu().double() - dx).abs()
    print("bwd %s %s: dom worst err/bound %.3g, dx32 worst err/bound %.3g" % (
        dtype, shape, (ed / bd.clamp_min(1e-300)).max().item(), (ex / bx.clamp_min(1e-300)).max().item()))
    assert torch.isfinite(gd).all() and (ed <= bd).all()
    assert torch.isfinite(dx32).all() and (ex <= bx).all()
    assert dom.abs().max() > 0 and dx.abs().max() > 0


def test_dcn_cols_backward_with_masks_and_wide_om():
    """sigmoid = 0 (DCNv2's case) and P = 64."""
    from scdhip import ops
    dtype, shape = torch.bfloat16, (2, 5, 7, 16, 2)
    N, H, W, C, G = shape
    x, om, dcols = _inputs(shape, dtype, False, True, 64)
    dx, dom, sx, sdom, ne = _backward_ref(shape, dtype, False, 64)
    dx32, gdom = ops.dcn_cols_bwd(*[t.to(dtype).to(DEV) for t in (dcols.view(N, H, W, 9 * C), x, om)], G, False)
    assert gdom.shape[-1] == 64 and not gdom[..., 54:].any()
    assert ((gdom[..., :54].cpu().double() - dom).abs() <= (4 * C // G + 8) * U * sdom + UT[dtype] * dom.abs()).all()
    assert ((dx32.cpu().double() - dx).abs() <= (ne + 8) * U * sx).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_invalid_arguments_return_before_any_launch(dtype):
    """Every SCD_ERR_ARG case: status 9001, and the output buffers keep their bytes."""
    import scdhip.lib as L
    from scdhip import ops
    lib = L.lib()
    e = ops.dcn_chunk(dtype)
    N, H, W, G = 1, 3, 4, 1
    C, P = 2 * e, ops.dcn_om_channels(1, dtype)
    big = max(P, 64) * 4
    x = torch.ones(N * H * W * big, dtype=dtype, device=DEV)
    om = torch.zeros(N * H * W * big, dtype=dtype, device=DEV)
    cols = torch.full((N * H * W * 9 * big,), 7.0, dtype=dtype, device=DEV)
    dcols = torch.ones_like(cols)
    dom = torch.full_like(om, 7.0)
    dx32 = torch.full((N * H * W * big,), 7.0, dtype=torch.float32, device=DEV)
    d, s = ops._DT[dtype], ops.stream()
    p = lambda t: t.data_ptr()

    def fwd(x_=x, om_=om, cols_=cols, N=N, H=H, W=W, C=C, G=G, P=P, sg=1):
        return lib.scd_dcn_cols(d, p(x_), p(om_), p(cols_), N, H, W, C, G, P, sg, s)

    def bwd(dc_=dcols, x_=x, om_=om, dx_=dx32, dom_=dom, N=N, H=H, W=W, C=C, G=G, P=P, sg=1):
        return lib.scd_dcn_cols_bwd(d, p(dc_), p(x_), p(om_), p(dx_), p(dom_), N, H, W, C, G, P, sg, s)

    bad = [dict(C=C + e // 2), dict(C=3 * e, G=2), dict(P=27 - 27 % e), dict(P=P + e // 2), dict(G=2), dict(N=0),
           dict(H=0), dict(W=-1), dict(C=0), dict(G=0), dict(P=0), dict(sg=2)]
    for kw in bad:
        assert fwd(**kw) == 9001, ("fwd", kw)
        assert bwd(**kw) == 9001, ("bwd", kw)
    assert fwd(cols_=x) == 9001 and fwd(cols_=om) == 9001
    assert bwd(dom_=dcols) == 9001 and bwd(dom_=x) == 9001 and bwd(dom_=om) == 9001
    assert bwd(dx_=x) == 9001 and bwd(dx_=dom) == 9001
    # partial overlaps: an output that starts inside an input's range
    assert fwd(cols_=x[e:]) == 9001 and fwd(cols_=om[N * H * W * P - e:]) == 9001
    assert bwd(dom_=dcols[e:]) == 9001 and bwd(dom_=om[e:]) == 9001 and bwd(dx_=dom[e:].view(torch.float32)) == 9001
    assert lib.scd_dcn_cols(7, p(x), p(om), p(cols), N, H, W, C, G, P, 1, s) == 9001
    torch.cuda.synchronize()
    assert (cols == 7).all() and (dom == 7).all() and (dx32 == 7).all() and (x == 1).all() and not om.any()
    assert fwd() == 0 and bwd() == 0          # and the arguments they vary are good ones
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- module

def _dcn_module(C, Co, G, seed, off_std):
    from models.backbones.deformable import DCN
    torch.manual_seed(seed)
    d = DCN(C, Co, 3, 1, 1, deformable_groups=G)
    with torch.no_grad():
        d.conv_offset_mask.weight.normal_(0, off_std / math.sqrt(9 * C))
        d.conv_offset_mask.bias.normal_(0, 0.1)
        d.bias.normal_(0, 0.1)
    return d


def _restated_dcn(d, x, dy, dtype):
    """DCN.forward restated (NHWC x, torch's conv for the offsets) in `dtype` on the CPU: output and the gradients of
    (x, weight, bias, conv_offset_mask.weight, conv_offset_mask.bias)."""
    G = d.deformable_groups
    leaves = [t.detach().to(dtype).clone().requires_grad_() for t in
              (x, d.weight, d.bias, d.conv_offset_mask.weight, d.conv_offset_mask.bias)]
    xr, w, b, wo, bo = leaves
    om = F.conv2d(xr.permute(0, 3, 1, 2), wo, bo, padding=1).permute(0, 2, 3, 1)
    off, m = R.split_om(om, G, True)
    y = R.dcn(xr, off, m, w, b, G)
    return y.detach(), torch.autograd.grad(y, leaves, dy.to(dtype)), off.detach()


@functools.lru_cache(maxsize=None)
def _fp32_case(G):
    """The first input seed whose float32 run of the restatement stays within 1e-5 of max|g| of its float64 gradients
    (another seed may put a sample on a kink of the bilinear map in one precision only, and bounds nothing)."""
    d = _dcn_module(64, 32, G, 5, 1.0)
    for seed in range(32):
        g = torch.Generator().manual_seed(seed)
        x = torch.randn(2, 12, 10, 64, generator=g)
        dy = torch.randn(2, 12, 10, 32, generator=g)
        y64, g64, off = _restated_dcn(d, x, dy, torch.float64)
        y32, g32, _ = _restated_dcn(d, x, dy, torch.float32)
        floor = max(((a.double() - b).abs().max() / b.abs().max()).item() for a, b in zip(g32, g64))
        if floor <= 1e-5 and (y32.double() - y64).abs().max() <= 1e-5:
            assert off.abs().max() > 1.5, "offsets of about +-2 px"
            return d, x, dy, y64, g64, seed, floor
    raise AssertionError("no seed in 0..31 with a float32 floor <= 1e-5")


@pytest.mark.parametrize("G", [1, 2])
def test_dcn_module_fp32_matches_the_restatement(G):
    """Outputs rtol = atol = 1e-3, gradient norms 1e-3, gradient elements 3e-3 of max|g| (1e-2 for 1-D tensors): the
    project's fp32 step bounds."""
    d, x, dy, y64, g64, seed, floor = _fp32_case(G)
    print("G=%d seed %d, float32 floor of the restatement %.2e" % (G, seed, floor))
    d = d.to(DEV)
    d.zero_grad()
    xg = x.to(DEV).requires_grad_()
    y = d(xg)
    y.backward(dy.to(DEV))
    torch.cuda.synchronize()
    from scdhip import ops
    ops.join_side_streams()
    np.testing.assert_allclose(y.detach().cpu().numpy(), y64.numpy(), rtol=1e-3, atol=1e-3)
    got = [xg.grad, d.weight.grad, d.bias.grad, d.conv_offset_mask.weight.grad, d.conv_offset_mask.bias.grad]
    for name, a, b in zip(("input", "weight", "bias", "conv_offset_mask.weight", "conv_offset_mask.bias"), got, g64):
        a = a.detach().cpu().double()
        nrm = abs(a.norm().item() - b.norm().item()) / b.norm().item()
        el = ((a - b).abs().max() / b.abs().max()).item()
        print("%-26s norm rel %.2e  max element err / max|g| %.2e" % (name, nrm, el))
        assert nrm < 1e-3 and el <= (1e-2 if b.dim() == 1 else 3e-3), name


def test_dcn_v2_with_given_offsets_and_masks():
    """DCNv2.forward(input, offset, mask) (sigmoid = 0) in fp32: every input's gradient against the restatement."""
    from models.backbones.deformable import DCNv2
    torch.manual_seed(9)
    N, H, W, C, Co, G = 2, 6, 9, 64, 32, 2
    d = DCNv2(C, Co, 3, 1, 1, deformable_groups=G)
    with torch.no_grad():
        d.bias.normal_(0, 0.1)
    g = torch.Generator().manual_seed(4)
    x = torch.randn(N, H, W, C, generator=g)
    off = R.draw_offsets(g, N, H, W, G, True).float()
    m = torch.rand(N, H, W, 9 * G, generator=g)
    dy = torch.randn(N, H, W, Co, generator=g)
    leaves = [t.detach().double().requires_grad_() for t in (x, off, m, d.weight, d.bias)]
    yr = R.dcn(*leaves, G)
    gr = torch.autograd.grad(yr, leaves, dy.double())
    d = d.to(DEV)
    ins = [t.to(DEV).requires_grad_() for t in (x, off, m)]
    y = d(*ins)
    y.backward(dy.to(DEV))
    np.testing.assert_allclose(y.detach().cpu().numpy(), yr.detach().numpy(), rtol=1e-3, atol=1e-3)
    for name, a, b in zip(("input", "offset", "mask", "weight", "bias"),
                          [t.grad for t in ins] + [d.weight.grad, d.bias.grad], gr):
        el = ((a.cpu().double() - b).abs().max() / b.abs().max()).item()
        print("%-8s max element err / max|g| %.2e" % (name, el))
        assert el <= (1e-2 if b.dim() == 1 else 3e-3), name


def _check(name, got, ref, scale):
    got, ref = got.float().cpu(), ref.float().cpu()
    assert got.shape == ref.shape and torch.isfinite(got).all(), name
    rms = ref.square().mean().sqrt().item()
    err = (got - ref).abs()
    mx, me = err.max().item() / rms, err.square().mean().sqrt().item() / rms
    print("%-28s max|err|/rms %.5f  rms(err)/rms %.6f  (bounds %.5f, %.6f)" % (name, mx, me, TOL_RMS * scale,
                                                                                 TOL_MEAN * scale))
    assert mx <= TOL_RMS * scale and me <= TOL_MEAN * scale, (name, mx, me)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_dcn_bn_relu_stage_16bit(dtype):
    """One DCN + BatchNorm2d + ReLU stage (blocks.DeformConvFn, training mode) against fp32 torch from the same 16-bit
    input.  Output: 2^-3 max and 2^-6 rms of the reference's rms, a quarter for fp16 (the hourglass groups' bounds,
    which that file holds forward outputs to).

    Gradients cannot be held to those: where the post-BN value lies within the forward error of 0 the 16-bit run and
    the fp32 reference take different sides of the ReLU, and such an element's gradient differs by all of itself
    (first seen on the GPU: input gradient 0.060 rms, 0.68 max in bf16, with every fp32 gradient of the same code
    within 3e-3 of max|g| in test_dcn_module_fp32_matches_the_restatement).  Bound, from the forward bound and not from
    that figure: the post-BN values have unit-variance normal density at most phi(0) = 0.399 per unit (gamma >= 0.5
    only narrows it relative to the output's rms), so a forward error of e = 2^-6 * scale rms flips at most a
    fraction f = 2 * phi(0) * e of the masks; a flipped element contributes its whole gradient, so the rms error of a
    gradient is at most sqrt(f) of its rms, plus the 2^-6 * scale of the roundings: 0.127 in bf16, 0.060 in fp16.  No
    max bound: one flipped element moves a gradient element by any amount."""
    from scdhip import blocks
    scale = 0.25 if dtype == torch.float16 else 1.0
    d = _dcn_module(64, 64, 1, 11, 0.5)
    bn = torch.nn.BatchNorm2d(64)
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.normal_(0, 0.2)
    g = torch.Generator().manual_seed(12)
    x = torch.randn(2, 12, 10, 64, generator=g).to(dtype)
    dy = torch.randn(2, 12, 10, 64, generator=g).to(dtype)
    # fp32 torch: the restatement in float32, torch's conv for the offsets, F.batch_norm on batch statistics
    leaves = [t.detach().float().clone().requires_grad_() for t in
              (x, d.weight, d.bias, d.conv_offset_mask.weight, d.conv_offset_mask.bias, bn.weight, bn.bias)]
    xr, w, b, wo, bo, gam, bet = leaves
    om = F.conv2d(xr.permute(0, 3, 1, 2), wo, bo, padding=1).permute(0, 2, 3, 1)
    off, m = R.split_om(om, 1, True)
    yr = R.dcn(xr, off, m, w, b, 1).permute(0, 3, 1, 2)
    yr = F.relu(F.batch_norm(yr, None, None, gam, bet, True, 0.1, bn.eps)).permute(0, 2, 3, 1)
    gr = torch.autograd.grad(yr, leaves, dy.float())
    d, bn = d.to(DEV), bn.to(DEV).train()
    xg = x.to(DEV).requires_grad_()
    y = blocks.DeformConvFn.apply(xg, d.weight, d, bn, True)
    y.backward(dy.to(DEV))
    from scdhip import ops
    ops.join_side_streams()
    torch.cuda.synchronize()
    _check("stage %s output" % dtype, y.detach(), yr.detach(), scale)
    got = [xg.grad, d.weight.grad, d.bias.grad, d.conv_offset_mask.weight.grad, d.conv_offset_mask.bias.grad,
           bn.weight.grad, bn.bias.grad]
    names = ("input", "weight", "bias", "conv_offset_mask.weight", "conv_offset_mask.bias", "bn.weight", "bn.bias")
    for name, a, r in zip(names, got, gr):
        if name == "bias":
            # batch statistics remove a per-channel constant: the true gradient is 0 and both sides hold rounding only
            # (each of the 240 gradients a channel sums carries one 16-bit rounding: far inside this)
            assert a.abs().max().item() <= TOL_RMS * scale * gr[6].square().mean().sqrt().item()
            continue
        a, r = a.detach().float().cpu(), r.float()
        assert a.shape == r.shape and torch.isfinite(a).all() and a.abs().max() > 0, name
        me = ((a - r).square().mean().sqrt() / r.square().mean().sqrt()).item()
        gb = math.sqrt(2 * 0.399 * TOL_MEAN * scale) + TOL_MEAN * scale
        print("stage %s d %-24s rms(err)/rms %.6f  (bound %.6f)" % (dtype, name, me, gb))
        assert me <= gb, (name, me, gb)


# ---------------------------------------------------------------------------------------------- model

def _dcn_model(dtype, offsets=False):
    plugin = importlib.import_module("trainer.model.centerOffsetRes18dcn")
    torch.manual_seed(42)
    m = plugin.model(**plugin.modelParams)
    if offsets:
        with torch.no_grad():
            for stage in m.deformLayers:
                com = stage[0].conv_offset_mask
                com.weight.normal_(0, 0.5 / math.sqrt(9 * com.in_channels))
                com.bias.normal_(0, 0.1)
                stage[1].running_mean.normal_(0, 0.1)
                stage[1].running_var.uniform_(0.5, 1.5)
    return m.to(DEV).set_compute_dtype(dtype), plugin


def test_model_heads_and_training_reduces_the_loss():
    from oracle import targets as T
    from scdhip.flat import FlatAdam
    m, plugin = _dcn_model(torch.bfloat16)
    m.train()
    x = T.batch_inputs(31, 2, 128).to(DEV)
    ys = [y.to(DEV) for y in T.batch_targets(32, 2, 32)]
    out = m(x, decode=False)[0]
    assert {k: tuple(v.shape) for k, v in out.items()} == {"heatmap": (2, 1, 32, 32), "regr": (2, 4, 32, 32),
                                                           "offset": (2, 2, 32, 32)}
    opt = FlatAdam(filter(lambda p: p.requires_grad, m.parameters()), lr=1e-3)
    losses = []
    for _ in range(20):
        opt.zero_grad()
        loss, _ = plugin.loss(m(x, decode=False), ys)
        loss.mean().backward()
        opt.step()
        losses.append(loss.item())
    print("loss", ["%.4f" % v for v in losses])
    assert np.isfinite(losses).all() and np.mean(losses[-5:]) < np.mean(losses[:5]), losses
    for stage in m.deformLayers:        # the zero-initialised offset conv has moved: its gradients arrive
        assert stage[0].conv_offset_mask.weight.abs().max() > 0 and stage[0].conv_offset_mask.bias.abs().max() > 0
        assert torch.isfinite(stage[0].weight).all()


def test_folded_model_matches_the_eval_forward_fp32():
    """fold(model) against the HIP eval forward, max |diff| <= 5e-5 (tests/test_infer_gpu.py's bound)."""
    from oracle import targets as T
    from scdhip import infer
    m, _ = _dcn_model(torch.float32, offsets=True)
    m.eval()
    x = T.batch_inputs(21, 2, 128).to(DEV)
    fm = infer.fold(m)
    assert len(fm.deforms) == 3
    with torch.no_grad():
        got = fm(x, decode=False)[0]
        hip = m(x, decode=False)[0]
    for k in ("heatmap", "regr", "offset"):
        dlt = (got[k] - hip[k]).abs().max().item()
        print("%s fold vs HIP eval: max |diff| %.3e (max |value| %.3e)" % (k, dlt, hip[k].abs().max().item()))
        assert torch.isfinite(got[k]).all() and dlt <= 5e-5, (k, dlt)


def test_slide_run_in_eval_mode_returns_detections(tmp_path):
    import slide
    from oracle import slide_case
    m, _ = _dcn_model(torch.bfloat16, offsets=True)
    with torch.no_grad():
        m.heatmap[2].bias.fill_(0.5)         # an untrained heatmap sits at sigmoid(-2.19), under slide.py's threshold
    ckpt = str(tmp_path / "res18dcn.pth")
    torch.save({k: v.cpu() for k, v in m.state_dict().items()}, ckpt)
    wrapper = slide.load_wrapper("centerOffsetRes18dcn", ckpt, True, False)
    assert wrapper.model.deformable and not wrapper.model.training
    det = slide.analyseArray(wrapper, slide_case.slide())
    print("%d detections" % len(det))
    assert len(det) > 0 and all(len(r) == 3 and all(math.isfinite(v) for v in r) for r in det)
