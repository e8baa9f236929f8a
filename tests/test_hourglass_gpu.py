"""The stacked-hourglass CenterNet on the GPU: the upsample-merge kernels against torch bit for bit, their argument
checks, the model in fp32 parity mode against the reference's float64 vectors (tests/golden/hourglass.npz, written by
make_golden_hourglass.py from the real reference), the 16-bit module groups against a plain-torch fp32 recomputation
(the method and bounds of test_bf16_parity_gpu.py), eval / decode, the full-depth net, the step graph and the training
loop.

Merge bounds.  Forward: torch forms up + low in fp32 and rounds once to the dtype, as the kernel does, so equality is
exact.  Backward: (d00 + d01) + (d10 + d11) in fp32 is three additions, each within 2^-24 relative of its exact
value, so within 3 * 2^-24 * sum|d| of the float64 sum, and one rounding to the dtype adds u * |ref| (u = 0 for fp32
beyond the three, 2^-8 bf16, 2^-11 fp16); integer-valued d in [-8, 8] sum exactly (|sum| <= 32 has at most 6 bits).
"""
import math
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import centernet as O
from oracle import targets as T

pytestmark = pytest.mark.gpu
DEV = "cuda"
ERR_ARG = 9001
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
U_OUT = {F32: 0.0, BF16: 2.0 ** -8, F16: 2.0 ** -11}
TOL_RMS = 2.0 ** -3          # test_bf16_parity_gpu.py: max |err| / rms(ref)
TOL_MEAN = 2.0 ** -6         # rms(err) / rms(ref)
HEADS = ("heatmap", "regr", "offset")
CASES = {"A": (dict(hourglassIters=2, dimensions=[64, 64, 128], modules=[1, 1, 2], predictionConvDim=128), (2, 1, 64, 64)),
         "B": (dict(hourglassIters=2, dimensions=[64, 128, 192], modules=[2, 1, 2], predictionConvDim=256), (3, 1, 64, 96))}

SHAPES = [(3, 3, 5, 8), (3, 3, 5, 24), (1, 1, 1, 8), (2, 4, 4, 136)]
MERGE = [(d, s) for d in (F32, BF16, F16) for s in SHAPES] + [(F32, (3, 3, 5, 4)), (F32, (3, 3, 5, 12))]
MERGE_IDS = ["%s-%s" % (str(d).split(".")[1], "x".join(map(str, s))) for d, s in MERGE]


def _ops():
    from scdhip import ops
    return ops


def gen(seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return g


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


# ------------------------------------------------------------------ 1-4: the merge kernels

def _merge_inputs(dtype, shape, seed):
    N, h, w, C = shape
    g = gen(seed)
    up = torch.randn(N, 2 * h, 2 * w, C, device=DEV, generator=g).to(dtype)
    low = (torch.randn(N, h, w, C, device=DEV, generator=g) * 1.5 + 0.25).to(dtype)
    return up, low


def _merge_ref(up, low):
    """up + nearest_2x(low) by torch in the same dtype, on NCHW views."""
    return _nhwc(_nchw(up) + F.interpolate(_nchw(low), scale_factor=2, mode="nearest"))


@pytest.mark.parametrize("dtype,shape", MERGE, ids=MERGE_IDS)
def test_merge_forward_bit_for_bit(dtype, shape):
    ops = _ops()
    up, low = _merge_inputs(dtype, shape, 11 + shape[3])
    up0, low0 = up.clone(), low.clone()
    out = ops.upsample_add(up, low)
    torch.cuda.synchronize()
    assert out.shape == up.shape and out.dtype == dtype
    assert torch.equal(out, _merge_ref(up, low))
    assert torch.equal(up, up0) and torch.equal(low, low0)
    into = torch.full_like(up, float("nan"))
    assert ops.upsample_add(up, low, out=into) is into
    assert torch.equal(into, out)


def test_merge_forward_grid_stride_loop():
    """786,432 chunks: more than any resident grid holds threads for, so every thread takes several chunks."""
    ops = _ops()
    p = torch.cuda.get_device_properties(0)
    shape = (4, 96, 64, 256)
    assert 4 * 96 * 64 * 256 // 8 == 786432 > p.multi_processor_count * p.max_threads_per_multi_processor
    up, low = _merge_inputs(BF16, shape, 5)
    out = ops.upsample_add(up, low)
    assert torch.equal(out, _merge_ref(up, low))
    dlow = ops.upsample_add_bwd(up)
    ref, mag = _block_sum64(up), _block_sum64(up.abs())
    assert ((dlow.double() - ref).abs() <= 3 * 2.0 ** -24 * mag + U_OUT[BF16] * ref.abs()).all()


def _block_sum64(d):
    """float64 2x2 block sums of an NHWC tensor -> NHWC."""
    x = d.double()
    return x[:, 0::2, 0::2] + x[:, 0::2, 1::2] + x[:, 1::2, 0::2] + x[:, 1::2, 1::2]


@pytest.mark.parametrize("dtype,shape", MERGE, ids=MERGE_IDS)
def test_merge_backward(dtype, shape):
    ops = _ops()
    N, h, w, C = shape
    g = gen(23 + C)
    d_int = torch.randint(-8, 9, (N, 2 * h, 2 * w, C), device=DEV, generator=g).to(dtype)
    keep = d_int.clone()
    got = ops.upsample_add_bwd(d_int)
    torch.cuda.synchronize()
    assert got.shape == (N, h, w, C) and got.dtype == dtype
    assert torch.equal(got.double(), _block_sum64(d_int))
    assert torch.equal(d_int, keep)
    d = torch.randn(N, 2 * h, 2 * w, C, device=DEV, generator=g).to(dtype)
    got = ops.upsample_add_bwd(d)
    ref, mag = _block_sum64(d), _block_sum64(d.abs())
    err = (got.double() - ref).abs()
    bound = 3 * 2.0 ** -24 * mag + U_OUT[dtype] * ref.abs()
    print("merge backward %s %s: worst err/bound %.3g" % (dtype, shape, (err / bound.clamp_min(1e-300)).max().item()))
    assert (err <= bound).all()


def test_merge_argument_errors():
    ops = _ops()
    lib = ops.L.lib()
    for dtype, C in ((BF16, 6), (F16, 6), (F32, 6), (BF16, 12), (F32, 2)):
        up = torch.zeros(1, 4, 4, C, device=DEV, dtype=dtype)
        low = torch.zeros(1, 2, 2, C, device=DEV, dtype=dtype)
        out = torch.full_like(up, 7.0)
        assert lib.scd_upsample2x_add(ops.dt(up), ops.ptr(up), ops.ptr(low), ops.ptr(out), 1, 2, 2, C, ops.stream()) == ERR_ARG
        assert lib.scd_upsample2x_add_bwd(ops.dt(up), ops.ptr(up), ops.ptr(low), 1, 2, 2, C, ops.stream()) == ERR_ARG
        torch.cuda.synchronize()
        assert torch.equal(out, torch.full_like(up, 7.0))
    up = torch.ones(1, 4, 4, 8, device=DEV, dtype=BF16)
    low = torch.ones(1, 2, 2, 8, device=DEV, dtype=BF16)
    out = torch.empty_like(up)
    args = lambda u, l, o, n=1, h=2, w=2: (ops.dt(up), ops.ptr(u), ops.ptr(l), ops.ptr(o), n, h, w, 8, ops.stream())  # noqa: E731
    assert lib.scd_upsample2x_add(*args(up, low, up)) == ERR_ARG           # out == up
    assert lib.scd_upsample2x_add(*args(up, low, low)) == ERR_ARG          # out == low
    for n, h, w in ((0, 2, 2), (1, 0, 2), (1, 2, -1)):
        assert lib.scd_upsample2x_add(*args(up, low, out, n, h, w)) == ERR_ARG
        assert lib.scd_upsample2x_add_bwd(ops.dt(up), ops.ptr(up), ops.ptr(low), n, h, w, 8, ops.stream()) == ERR_ARG
    assert lib.scd_upsample2x_add(7, ops.ptr(up), ops.ptr(low), ops.ptr(out), 1, 2, 2, 8, ops.stream()) == ERR_ARG
    torch.cuda.synchronize()
    assert torch.equal(up, torch.ones_like(up)) and torch.equal(low, torch.ones_like(low))
    with pytest.raises(RuntimeError):                                     # the ops wrapper raises on the status
        ops.upsample_add(up, low, out=up)
    assert lib.scd_upsample2x_add(*args(up, low, out)) == 0


@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=["float32", "bfloat16", "float16"])
def test_upsample_add_fn_autograd(dtype):
    from scdhip import blocks
    up, low = _merge_inputs(dtype, (2, 3, 5, 16), 3)
    up.requires_grad_(True)
    low.requires_grad_(True)
    up0 = up.detach().clone()
    out = blocks.UpsampleAddFn.apply(up, low)
    assert torch.equal(out.detach(), _merge_ref(up.detach(), low.detach()))
    dout = torch.randint(-8, 9, out.shape, device=DEV, generator=gen(4)).to(dtype)
    out.backward(dout)
    torch.cuda.synchronize()
    assert torch.equal(up.grad, dout)
    assert torch.equal(low.grad.double(), _block_sum64(dout))
    assert torch.equal(up.detach(), up0)


# ------------------------------------------------------------------ the BatchNorm kernels at the hourglass's widths
#
# 192 channels are 24 bf16 / 48 fp32 chunks of 16 B: neither a divisor nor a multiple of 256, the two row widths the
# elementwise BN kernels took before.  Rows of whole 128-byte lines (a multiple of 8 chunks, below 256) now run with a
# grid that is a multiple of cpr / gcd(cpr, 256), and in the reduction the last 256 % cpr threads of a block own no
# row lane.  Checked with the helpers, references and bounds of tests/test_bn_gpu.py at 24 / 48 chunks, at 40 chunks
# (grid unit 5) and at 248 (one row lane, 8 idle threads, grid unit 31).

BN_WIDE = [(F32, 192), (BF16, 192), (F16, 192), (BF16, 320), (BF16, 1984), (F32, 992)]
BN_WIDE_IDS = ["%s-%d" % (str(d).split(".")[1], C) for d, C in BN_WIDE]


def _bn_rows(C, dtype):
    import test_bn_gpu as B
    rpi = 256 // (C // B.EPC[dtype])
    return rpi, [1, 3, 8 * rpi + 1, 40 * rpi + 3]


@pytest.mark.parametrize("dtype,C", BN_WIDE, ids=BN_WIDE_IDS)
def test_bn_elementwise_kernels_at_line_multiple_rows(dtype, C):
    import test_bn_gpu as B
    ops = _ops()
    _, rows = _bn_rows(C, dtype)
    for r in rows[:3]:
        B.check_apply(ops, dtype, C, r, 31 * C + r, (0, 1, 2))
        B.check_bwd_apply(ops, dtype, C, r, 37 * C + r, (0, 1, 2))
        B.check_bwd_apply2(ops, dtype, C, r)


@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=["float32", "bfloat16", "float16"])
def test_bn_elementwise_kernels_at_192_long_runs(dtype):
    """More than four grid strides of vectors and an odd row count: the unrolled main loops and their ragged tails on
    a grid rounded to a multiple of 3."""
    import test_bn_gpu as B
    ops = _ops()
    rows = B.long_rows(192, dtype)
    B.check_apply(ops, dtype, 192, rows, 5, (2,), (1,))
    B.check_bwd_apply(ops, dtype, 192, rows, 9, (1,), (True,))
    B.check_bwd_apply2(ops, dtype, 192, rows)


@pytest.mark.parametrize("dtype,C", BN_WIDE, ids=BN_WIDE_IDS)
def test_bn_bwd_reduce_exact_at_line_multiple_rows(dtype, C):
    """Integer-valued inputs (test_bn_gpu.py's exact construction): the sums of both reduce kernels equal float64 bit
    for bit on a pre-filled buffer, so a row lane taken by an idle thread, or a dropped or doubled row, cannot hide."""
    import test_bn_gpu as B
    ops = _ops()
    mean, invstd, rsc, rsh = B.exact_params(C)
    mean_b, is_b = B.exact_params_b(C)
    for rows in _bn_rows(C, dtype)[1]:
        g = B.gen(17 * C + rows)
        dout = B.ints(g, -4, 4, (rows, C), dtype)
        y = B.ints(g, -8, 8, (rows, C), dtype)
        yb = B.ints(g, -8, 8, (rows, C), dtype)
        mask = B.ints(g, -2, 2, (rows, C), dtype)
        for kind in (0, 1, 2):
            stats = B.prefilled_stats(ops, C)
            want = stats.sum(0) + B.reduce_ref(dout, y, kind, mask, rsc, rsh, mean, invstd)[0]
            B.run_reduce(ops, dout, y, kind, mask, rsc, rsh, mean, invstd, stats)
            torch.cuda.synchronize()
            assert torch.equal(stats.sum(0), want), (dtype, C, rows, kind)
        sa, sb = B.prefilled_stats(ops, C), B.prefilled_stats(ops, C) * 3.0
        want_a = sa.sum(0) + B.reduce_ref(dout, y, 1, mask, None, None, mean, invstd)[0]
        want_b = sb.sum(0) + B.reduce_ref(dout, yb, 1, mask, None, None, mean_b, is_b)[0]
        ops.L.call("scd_bn_bwd_reduce2", ops.dt(y), ops.ptr(dout), ops.ptr(mask), ops.ptr(y), ops.ptr(yb), ops.ptr(mean),
                   ops.ptr(invstd), ops.ptr(mean_b), ops.ptr(is_b), C, y.numel(), ops.ptr(sa), ops.ptr(sb), ops.stream())
        torch.cuda.synchronize()
        assert torch.equal(sa.sum(0), want_a) and torch.equal(sb.sum(0), want_b), (dtype, C, rows)


def test_bn_rows_of_partial_lines_stay_refused():
    """12 chunks (bf16 C = 96): not a divisor of 256, not whole 128-byte lines."""
    import test_bn_gpu as B
    ops = _ops()
    y = torch.ones(7, 96, device=DEV, dtype=BF16)
    out = torch.full_like(y, 7.0)
    sc = torch.ones(96, device=DEV)
    assert B.status("scd_bn_apply", ops.dt(y), ops.ptr(y), ops.ptr(out), 96, y.numel(), ops.ptr(sc), ops.ptr(sc), 0, 0, 0, 1,
                    ops.stream()) == ERR_ARG
    torch.cuda.synchronize()
    assert torch.equal(out, torch.full_like(y, 7.0))


# ------------------------------------------------------------------ 5: fp32 parity with the reference

def _entries(g, case):
    keys = [str(k) for k in g[case + "|keys"]]
    shapes = [tuple(int(v) for v in str(s).split(",")) if str(s) else () for s in g[case + "|shapes"]]
    return list(zip(keys, shapes))


def _build(g, case, dtype):
    from models.centerNetOffseth import CenterNetHourglass
    m = CenterNetHourglass(**CASES[case][0])
    m.load_state_dict(O.hash_weights(_entries(g, case)))
    return m.to(DEV).train().set_compute_dtype(dtype)


def _loss_weight(shape):
    return torch.from_numpy(0.25 + 0.75 * np.random.RandomState(7).random_sample(shape)).float().to(DEV)


@pytest.mark.parametrize("case", ["A", "B"])
def test_fp32_parity_with_the_reference(case, golden):
    """Outputs rtol = atol = 1e-3, gradient norms 1e-3, sampled gradient elements 3e-3 of max|g| (1e-2 for 1-D
    tensors): the bounds tests/test_model_gpu.py holds the ResNet's fp32 step to, for the same cause (another summation
    order).  The fixture's own float32-against-float64 floor is asserted to lie 100 times below each."""
    g = golden("hourglass")
    assert float(g[case + "|floor"]) <= 1e-5 and float(g[case + "|out_floor"]) <= 1e-5
    m = _build(g, case, F32)
    x = torch.from_numpy(np.random.RandomState(int(g[case + "|seed"])).standard_normal(CASES[case][1])).float().to(DEV)
    out = m(x, decode=False)[0]
    loss = sum((out[h] * _loss_weight(tuple(out[h].shape))).sum() for h in HEADS)
    loss.backward()
    torch.cuda.synchronize()
    worst_out = {h: float(np.abs(out[h].detach().cpu().double().numpy() - g["%s|out|%s" % (case, h)]).max()) for h in HEADS}
    print("case %s worst absolute output errors:" % case, worst_out)
    names = [str(n) for n in g[case + "|pnames"]]
    params = dict(m.named_parameters())
    assert list(params) == names
    rel, samp = {}, {1: {}, 2: {}}
    for i, k in enumerate(names):
        gr = params[k].grad.detach().double().cpu()
        ref = float(g[case + "|gnorm"][i])
        d = abs(gr.norm().item() - ref)
        rel[k] = d / max(ref, 1e-6) if d > 1e-6 else 0.0
        pos = np.random.RandomState(zlib.crc32(k.encode()) & 0xFFFFFFFF).randint(0, gr.numel(), 16)
        assert np.array_equal(pos, g[case + "|gpos"][i])
        scale = max(gr.abs().max().item(), 1e-30)
        samp[1 if gr.dim() == 1 else 2][k] = float(np.abs(gr.reshape(-1)[pos].numpy() - g[case + "|gsamp"][i]).max() / scale)
    top = sorted(rel.items(), key=lambda kv: -kv[1])[:4]
    print("case %s worst gradient-norm relative errors:" % case, top)
    tops = {}
    for kind in (2, 1):
        tops[kind] = sorted(samp[kind].items(), key=lambda kv: -kv[1])[:4]
        print("case %s worst sampled-gradient errors (/ max|g|) of the %s:" % (case, "weights" if kind == 2 else "1-D tensors"),
              tops[kind])
    for h in HEADS:
        np.testing.assert_allclose(out[h].detach().cpu().numpy(), g["%s|out|%s" % (case, h)], rtol=1e-3, atol=1e-3, err_msg=h)
    assert top[0][1] < 1e-3, top
    assert tops[2][0][1] <= 3e-3, tops[2]
    assert tops[1][0][1] <= 1e-2, tops[1]


# ------------------------------------------------------------------ 6: 16-bit groups against fp32 torch

def _bn(h, m):
    return F.batch_norm(h, m.running_mean.clone(), m.running_var.clone(), m.weight, m.bias, True, 0.1, m.eps)


def ref_residual(blk, x):
    """Residual.forward of the reference (residuals.py:69-79) in fp32, NCHW."""
    o = F.relu(_bn(F.conv2d(x, blk.conv1.weight, stride=blk.conv1.stride, padding=1), blk.bn1))
    o = _bn(F.conv2d(o, blk.conv2.weight, padding=1), blk.bn2)
    skip = _bn(F.conv2d(x, blk.skip[0].weight, stride=blk.skip[0].stride), blk.skip[1]) if len(blk.skip) else x
    return F.relu(o + skip)


def ref_level(hg, x):
    """Hourglass.forward of the reference (hourglass.py:107-114) in fp32, NCHW; no pooling layer."""
    def seq(s, h):
        for blk in s:
            h = ref_residual(blk, h)
        return h
    up1 = seq(hg.preserveCurrentDimension, x)
    low1 = seq(hg.changeDimension, x)
    low2 = ref_level(hg.embeddedHourglass, low1) if hasattr(hg.embeddedHourglass, "merge") else seq(hg.embeddedHourglass, low1)
    low3 = seq(hg.changeDimensionBack, low2)
    return up1 + F.interpolate(low3, scale_factor=2, mode="nearest")


def check(name, got, ref, scale):
    got, ref = got.float(), ref.float()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert torch.isfinite(got).all(), name
    rms = ref.square().mean().sqrt().item()
    err = (got - ref).abs()
    mx, me = err.max().item() / rms, err.square().mean().sqrt().item() / rms
    print("%-28s max|err|/rms %.5f  rms(err)/rms %.6f  (bounds %.5f, %.6f)" % (name, mx, me, TOL_RMS * scale, TOL_MEAN * scale))
    assert mx <= TOL_RMS * scale and me <= TOL_MEAN * scale, (name, mx, me)


def _hashed(module, prefix):
    """Hash-initialised (oracle.centernet.hash_weights over the module's own entries, keys under `prefix`)."""
    state = O.hash_weights([(prefix + k, tuple(v.shape)) for k, v in module.state_dict().items()])
    module.load_state_dict({k[len(prefix):]: v for k, v in state.items()})
    return module.to(DEV).train()


@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bfloat16", "float16"])
def test_16bit_groups_match_fp32(dtype, golden):
    """StemConvFn at (2,1,64,64) -> 128, Residual in its three forms at 16^2 with 64 / 128 channels and the innermost
    Hourglass level of case A, each against plain torch fp32 from the same 16-bit input.  fp16 rounds at 2^-11: a
    quarter of the bf16 bound, as in test_bf16_parity_gpu.py."""
    from models.backbones.convolutions import Convolution
    from models.backbones.residuals import Residual
    from scdhip import blocks
    scale = 0.25 if dtype == F16 else 1.0
    g = gen(17)
    with torch.no_grad():
        stem = _hashed(Convolution(7, 1, 128, stride=2), "stem.")
        x = torch.randn(2, 1, 64, 64, device=DEV, generator=g)
        got = blocks.StemConvFn.apply(x, stem.conv.weight, stem.conv, stem.bn, dtype)
        assert got.shape == (2, 32, 32, 128) and got.dtype == dtype
        ref = F.relu(_bn(F.conv2d(x.to(dtype).float(), stem.conv.weight, stride=2, padding=3), stem.bn))
        check("stem 7x7 s2 -> 128", _nchw(got), ref, scale)
        for name, blk in (("residual 64 -> 64", Residual(3, 64, 64)), ("residual 64 -> 128", Residual(3, 64, 128)),
                          ("residual 64 -> 64 stride 2", Residual(3, 64, 64, stride=2))):
            blk = _hashed(blk, name + ".")
            xh = torch.randn(2, 16, 16, 64, device=DEV, generator=g).to(dtype)
            check(name, _nchw(blk(xh)), ref_residual(blk, _nchw(xh).float()), scale)
        m = _build(golden("hourglass"), "A", dtype)
        level = m.hourglassStack[0].embeddedHourglass
        assert level.iteration == 1
        xh = torch.randn(2, 8, 8, 64, device=DEV, generator=g).to(dtype)
        check("hourglass level 64 | 128", _nchw(level(xh)), ref_level(level, _nchw(xh).float()), scale)


# ------------------------------------------------------------------ 7: eval and decode

def test_eval_decode_structure_and_repeatability(golden):
    import trainer.model.centerOffsetRes10 as res10
    g = golden("hourglass")
    m = _build(g, "A", F32).eval()
    x = T.batch_inputs(5, 2, 64).to(DEV)
    with torch.no_grad():
        a = m(x, decode=True)
        b = m(x, decode=True)
        r = res10.model(**res10.modelParams).to(DEV).eval().set_compute_dtype(F32)(x, decode=True)
    torch.cuda.synchronize()
    assert len(a) == len(r) == 7
    for u, v in zip(a[:6], r[:6]):
        assert type(u) is type(v) and u.dtype == v.dtype and u.shape == v.shape
    assert sorted(a[6]) == sorted(r[6]) == sorted(HEADS)
    for h in HEADS:
        assert a[6][h].shape == r[6][h].shape and a[6][h].dtype == r[6][h].dtype
        assert torch.equal(a[6][h], b[6][h])
    for u, v in zip(a[:6], b[:6]):
        assert torch.equal(u, v)
    assert torch.isfinite(a[0]).all()
    sd = m.state_dict()
    assert int(sd["preprocess.0.bn.num_batches_tracked"]) == 0      # eval mode: the running statistics were only read


# ------------------------------------------------------------------ 8: full depth

def test_full_depth_bf16_step():
    """CenterNetHourglass() at (2,1,128,128), the smallest input its five levels take (the deepest map is 1x1): one
    loss forward / backward and one FlatAdam step."""
    import trainer.model.centerOffsetHourglass as plugin
    from scdhip.flat import FlatAdam
    torch.random.manual_seed(42)
    m = plugin.model(**plugin.modelParams).to(DEV).train().set_compute_dtype(BF16)
    with pytest.raises(ValueError, match="multiples of 32"):
        m(torch.zeros(2, 1, 96, 96, device=DEV), decode=False)
    opt = FlatAdam(filter(lambda p: p.requires_grad, m.parameters()))
    x = T.batch_inputs(51, 2, 128).to(DEV)
    ys = [y.to(DEV) for y in T.batch_targets(52, 2, 32)]
    opt.zero_grad()
    loss, _ = plugin.loss(m(x, decode=False), ys)
    loss.mean().backward()
    grads = {k: p.grad.detach().clone() for k, p in m.named_parameters()}
    opt.step()
    torch.cuda.synchronize()
    assert math.isfinite(loss.item())
    bad = [k for k, v in grads.items() if not torch.isfinite(v).all()]
    zero = [k for k, v in grads.items() if not v.any()]
    print("full depth: loss %.5f, %d parameters, non-finite %s, identically zero %s" % (loss.item(), len(grads), bad, zero))
    assert not bad and not zero
    assert all(torch.isfinite(p).all() for p in m.parameters())


# ------------------------------------------------------------------ 9: step graph

def test_step_graph_matches_eager(golden):
    """The eager-against-graph check of tests/test_graph_gpu.py on case A's net, three steps (the third is captured):
    losses within 1e-5 relative, the bound that file holds the ResNet to."""
    import trainer.model.centerOffsetHourglass as plugin
    from scdhip.flat import FlatAdam
    from scdhip.graph import StepGraph
    g = golden("hourglass")
    batches = [(T.batch_inputs(100 + i, 2, 64).to(DEV), [y.to(DEV) for y in T.batch_targets(200 + i, 2, 16)])
               for i in range(3)]

    def run(graph):
        m = _build(g, "A", F32)
        opt = FlatAdam(filter(lambda p: p.requires_grad, m.parameters()))

        def step(x, ys):
            opt.zero_grad()
            loss, _ = plugin.loss(m(x, decode=False), ys)
            loss = loss.mean()
            loss.backward()
            opt.step()
            return loss

        runner = StepGraph(step, optimizer=opt, warmup=2) if graph else step
        losses = [runner(x, ys).item() for x, ys in batches]
        return losses, torch.cat([p.detach().reshape(-1) for p in m.parameters()]).cpu(), runner

    le, pe, _ = run(False)
    lg, pg, runner = run(True)
    print("eager losses", le, "graph losses", lg)
    assert len(runner.graphs) == 1 and runner.calls == 3
    np.testing.assert_allclose(lg, le, rtol=1e-5)
    np.testing.assert_allclose(pg.numpy(), pe.numpy(), rtol=1e-5, atol=1e-6)


# ------------------------------------------------------------------ 10: the training loop

def test_train_through_network_factory(tmp_path):
    """"modelName": "centerOffsetHourglass" through NetworkFactory (what train.py builds and runs) on the synthetic
    dataset: two iterations at batch 2 in bf16, the way the existing end-to-end tests drive it."""
    from configuration import defaultConfig
    from models.centerNetOffseth import CenterNetHourglass
    from models.networkFactory import NetworkFactory
    old = dict(defaultConfig.config)
    try:
        defaultConfig.updateConfig({"modelName": "centerOffsetHourglass", "datasetName": "syntheticSCD",
                                    "trainName": "hgtest", "computeDtype": "bf16", "iterations": 2, "validation": 1000,
                                    "snapshot": 2, "batchSize": 2, "dirTemp": str(tmp_path / "t") + "/",
                                    "dirResult": str(tmp_path / "r") + "/", "currentIter": 0})
        f = NetworkFactory(True)
        assert isinstance(f.model, CenterNetHourglass)
        f.beginTraining(0)
        assert f.optimizer.state_dict()["step"] == 2
        losses = np.loadtxt(str(tmp_path / "r" / "losses.hgtest.2.txt"), delimiter=",", ndmin=2)
        assert (tmp_path / "r" / "evals.hgtest.txt").exists()
    finally:
        defaultConfig.config.clear()
        defaultConfig.config.update(old)
    assert losses.shape == (2, 5) and np.isfinite(losses).all() and (losses[:, 1] > 0).all()
