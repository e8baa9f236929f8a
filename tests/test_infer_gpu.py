"""Folded-BatchNorm inference on the GPU: the scd_conv_gemm_res epilogue (y = act(acc + bias + res), summed in fp32
from the unrounded accumulator, rounded once at the store), the folded blocks of scdhip/infer.py, the folded model
against the CPU oracle and the HIP eval forward, and the "fold" mode of the TorchScript export.

16-bit group bound (restated from tests/test_bf16_parity_gpu.py): in units of the reference's rms, a group that rounds
c <= 6 weights / intermediates / outputs to bf16 (2^-9 each) has rms(err) <= 2^-6 and max|err| <= 2^-3; fp16 rounds
at 2^-11, a quarter of both.  A folded group rounds fewer values (no pre-BN intermediate is stored), so the bound
holds a fortiori.
"""
import functools
import importlib

import pytest
import torch
import torch.nn.functional as F

from oracle import centernet as O
from oracle import targets as T

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
TOL = {torch.float32: 1e-4, torch.bfloat16: 3e-2, torch.float16: 1e-2}      # tests/test_kernels_gpu.py
TOL_RMS, TOL_MEAN = 2.0 ** -3, 2.0 ** -6

CASES = [  # N, Ci, H, W, Co, k, stride, pad
    (1, 64, 8, 8, 128, 3, 1, 1),          # a partial 128-row tile
    (2, 64, 16, 16, 64, 3, 2, 1),         # the narrow 256 x 64 kernel
    (2, 64, 15, 13, 128, 1, 2, 0),        # ragged, a 1x1 stride-2 downsample
    (4, 128, 32, 32, 256, 3, 1, 1),       # 32 tiles of 128 x 128 rows, 18 K stages
    (4, 64, 128, 128, 256, 3, 1, 1),      # the ping-pong kernel, >= 256 tiles (16-bit types)
    (4, 64, 128, 128, 128, 3, 1, 1),      # the LDS-DMA ring kernel: 256 tiles of 256 x 128 (16-bit types)
]
DECONV = (2, 64, 8, 8, 128)               # (N, Ci, H, W) -> (N, Co, 2H, 2W): k 4, stride 2, pad 1, four phases


def nhwc(t, dtype):
    return t.permute(0, 2, 3, 1).contiguous().to(DEV, dtype)


def nchw(t):
    return t.float().permute(0, 3, 1, 2).cpu()


def rel_err(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return (a - b).abs().max().item() / max(1e-6, b.abs().max().item())


def _conv_ref(x, w, case):
    if len(case) == 5:
        return F.conv_transpose2d(x, w, stride=2, padding=1)
    return F.conv2d(x, w, stride=case[6], padding=case[7])


def _out_shape(case):
    if len(case) == 5:
        return (case[0], case[4], 2 * case[2], 2 * case[3])
    N, Ci, H, W, Co, k, s, p = case
    return (N, Co, (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1)


def _weight(rows, case):
    """(Co, Ci * taps) rows -> the layer's weight: Conv2d (Co, Ci, k, k) or ConvTranspose2d (Ci, Co, 4, 4)."""
    Ci, Co = case[1], case[4]
    if len(case) == 5:
        return rows.view(Co, Ci, 4, 4).transpose(0, 1).contiguous()
    return rows.view(Co, Ci, case[5], case[5]).contiguous()


@functools.lru_cache(maxsize=None)
def _exact_operands(case):
    """Integer-valued operands (exact in fp32, bf16 and fp16: |v| <= 48) and the CPU reference, computed once."""
    g = torch.Generator().manual_seed(1234)
    N, Ci, H, W, Co = case[:5]
    x = torch.randint(-3, 4, (N, Ci, H, W), generator=g).float()
    taps = 16 if len(case) == 5 else case[5] ** 2
    # at most 8 non-zeros (+-1) per output channel
    idx = torch.randint(0, Ci * taps, (Co, 8), generator=g)
    val = (torch.randint(0, 2, (Co, 8), generator=g) * 2 - 1).float()
    rows = torch.zeros(Co, Ci * taps).scatter_(1, idx, val)
    assert (rows != 0).sum(1).max().item() <= 8
    w = _weight(rows, case)
    bias = torch.randint(-8, 9, (Co,), generator=g).float()
    acc = _conv_ref(x, w, case)
    res = torch.randint(-16, 17, acc.shape, generator=g).float()
    a = acc + bias.view(1, -1, 1, 1)
    assert a.abs().max().item() <= 32 and (a + res).abs().max().item() <= 48
    return x, w, bias, res, a


def _launch(case, dtype, x, w, bias, res, relu):
    """The new entry point on NCHW fp32 host operands -> NCHW fp32 host result."""
    from scdhip import ops
    xg = nhwc(x, dtype)
    bg = bias.to(DEV) if bias is not None else None
    rg = nhwc(res, dtype) if res is not None else None
    if len(case) == 5:
        y = ops.deconv_fwd_res(xg, ops.pack_weight(w.to(DEV), dtype, 1), case[4], 4, 2, 1, bg, rg, relu)
    else:
        N, Ci, H, W, Co, k, s, p = case
        y = ops.conv_fwd_res(xg, ops.pack_weight(w.to(DEV), dtype, 0), Co, k, k, s, p, bg, rg, relu)
    return nchw(y)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", CASES + [DECONV])
def test_exact_epilogue(case, dtype):
    """Integer operands: the result equals the reference bit for bit in all three dtypes, ReLU on and off, residual
    present and NULL.  The residual flips the sign of >= 5 % of the outputs in each direction, so an epilogue that
    applies the ReLU before the add cannot pass."""
    x, w, bias, res, a = _exact_operands(case)
    up = ((a < 0) & (a + res > 0)).float().mean().item()
    down = ((a > 0) & (a + res < 0)).float().mean().item()
    assert up >= 0.05 and down >= 0.05, (up, down)
    for relu in (False, True):
        for r in (res, None):
            ref = a + r if r is not None else a
            ref = F.relu(ref) if relu else ref
            got = _launch(case, dtype, x, w, bias, r, relu)
            assert torch.equal(got, ref), (relu, r is not None, (got - ref).abs().max().item())
    # bias NULL as well
    got = _launch(case, dtype, x, w, None, res, True)
    assert torch.equal(got, F.relu(a - bias.view(1, -1, 1, 1) + res))


@functools.lru_cache(maxsize=None)
def _random_operands(case):
    g = torch.Generator().manual_seed(4321)
    N, Ci, H, W, Co = case[:5]
    taps = 16 if len(case) == 5 else case[5] ** 2
    x = torch.randn(N, Ci, H, W, generator=g)
    w = _weight(torch.randn(Co, Ci * taps, generator=g) / (Ci * taps) ** 0.5, case)
    bias = torch.randn(Co, generator=g)
    res = torch.randn(_out_shape(case), generator=g)
    return x, w, bias, res


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", CASES + [DECONV])
def test_random_values_match_torch_fp32(case, dtype):
    x, w, bias, res = _random_operands(case)
    if dtype != torch.float32:            # compare on operands representable in the 16-bit type
        x, w, res = x.to(dtype).float(), w.to(dtype).float(), res.to(dtype).float()
    ref = F.relu(_conv_ref(x, w, case) + bias.view(1, -1, 1, 1) + res)
    got = _launch(case, dtype, x, w, bias, res, True)
    e = rel_err(got, ref)
    print("rel_err %.3e" % e)
    assert e < TOL[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", [CASES[1], CASES[3]])
def test_null_residual_is_scd_conv_gemm(case, dtype):
    from scdhip import ops
    N, Ci, H, W, Co, k, s, p = case
    x, w, bias, _ = _random_operands(case)
    xg, bg = nhwc(x, dtype), bias.to(DEV)
    wp = ops.pack_weight(w.to(DEV), dtype, 0)
    want = ops.conv_fwd(xg, wp, Co, k, k, s, p, bias=bg, relu=True)
    got = ops.conv_fwd_res(xg, wp, Co, k, k, s, p, bg, None, True)
    assert torch.equal(got, want)


def test_residual_aliasing_the_output_is_refused():
    from scdhip import ops
    N, Ci, H, W, Co, k, s, p = (1, 64, 8, 8, 64, 3, 1, 1)
    x = torch.zeros(N, H, W, Ci, device=DEV)
    wp = ops.pack_weight(torch.zeros(Co, Ci, k, k, device=DEV), torch.float32, 0)
    y = torch.zeros(N, H, W, Co, device=DEV)
    with pytest.raises(RuntimeError, match="9001"):
        ops.conv_fwd_res(x, wp, Co, k, k, s, p, None, y, False, out=y)


def _fast_operands(N, Ci, H, W, Co, k, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    x = nhwc(torch.randn(N, Ci, H, W, generator=g), dtype)
    w = (torch.randn(Co, Ci, k, k, generator=g) / (Ci * k * k) ** 0.5).to(DEV)
    bias = torch.randn(Co, generator=g).to(DEV)
    res = nhwc(torch.randn(N, Co, H, W, generator=g), dtype)
    return x, w, bias, res


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("N,H,W", [(3, 64, 64), (2, 32, 128)])
def test_row_ring_kernel_is_the_tiled_kernel(N, H, W, dtype, monkeypatch):
    """conv_gemm_l1p_kernel with the bias / residual / ReLU epilogue (3x3, 64 -> 64, whole rows of 64 / 128 pixels)
    against the register-staged 256 x 64 kernel (SCD_GEMM_HALO64=0): the same bits, with and without the residual."""
    from scdhip import ops
    x, w, bias, res = _fast_operands(N, 64, H, W, 64, 3, dtype, 71)
    wp = ops.pack_weight(w, dtype, 0)
    outs = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("SCD_GEMM_HALO64", mode)
        outs[mode] = (ops.conv_fwd_res(x, wp, 64, 3, 3, 1, 1, bias, res, True),
                      ops.conv_fwd_res(x, wp, 64, 3, 3, 1, 1, bias, None, True),
                      ops.conv_fwd_res(x, wp, 64, 3, 3, 1, 1, None, res, False))
        torch.cuda.synchronize()
    for a, b in zip(outs["1"], outs["0"]):
        assert torch.equal(a, b)
    ref = F.relu(F.conv2d(nchw(x), w.cpu().to(dtype).float(), bias.cpu(), padding=1) + nchw(res))
    assert rel_err(nchw(outs["1"][0]), ref) < TOL[dtype]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("K,C", [(64, 256), (256, 64), (128, 128)])
def test_stream_kernel_is_the_tiled_kernel(K, C, dtype, monkeypatch):
    """conv1x1_stream_kernel's bias / residual / ReLU mode at its lower limit (N = 4 at 128^2: 65,536 pixels) against
    the tiled kernels: the same bits.  SCD_GEMM_STREAM1X1=2 fails every GEMM the stream kernel does not take, so the
    "2" results are its own."""
    from scdhip import ops
    x, w, bias, res = _fast_operands(4, K, 128, 128, C, 1, dtype, 113)
    wp = ops.pack_weight(w, dtype, 0)
    outs = {}
    for mode in ("2", "0"):
        monkeypatch.setenv("SCD_GEMM_STREAM1X1", mode)
        outs[mode] = (ops.conv_fwd_res(x, wp, C, 1, 1, 1, 0, bias, res, True),
                      ops.conv_fwd_res(x, wp, C, 1, 1, 1, 0, bias, None, True),
                      ops.conv_fwd_res(x, wp, C, 1, 1, 1, 0, None, res, False))
        torch.cuda.synchronize()
    for a, b in zip(outs["2"], outs["0"]):
        assert torch.equal(a, b)
    ref = F.relu(F.conv2d(nchw(x), w.cpu().to(dtype).float(), bias.cpu()) + nchw(res))
    assert rel_err(nchw(outs["2"][0]), ref) < TOL[dtype]


def test_stream_only_mode_fails_shapes_the_stream_kernel_does_not_take(monkeypatch):
    """SCD_GEMM_STREAM1X1=2 fails every GEMM the 1x1 stream kernel does not take, on the new entry point as on
    scd_conv_gemm."""
    from scdhip import ops
    N, Ci, H, W, Co, k, s, p = CASES[0]
    x, w, bias, res = _random_operands(CASES[0])
    xg, bg, rg = nhwc(x, torch.bfloat16), bias.to(DEV), nhwc(res, torch.bfloat16)
    wp = ops.pack_weight(w.to(DEV), torch.bfloat16, 0)
    monkeypatch.setenv("SCD_GEMM_STREAM1X1", "2")
    with pytest.raises(RuntimeError, match="9001"):
        ops.conv_fwd(xg, wp, Co, k, k, s, p, bias=bg, relu=True)
    with pytest.raises(RuntimeError, match="9001"):
        ops.conv_fwd_res(xg, wp, Co, k, k, s, p, bg, rg, True)
    monkeypatch.setenv("SCD_GEMM_STREAM1X1", "1")
    ops.conv_fwd_res(xg, wp, Co, k, k, s, p, bg, rg, True)
    torch.cuda.synchronize()


# ------------------------------------------------------------------ folded groups in 16-bit

def _seed_bn(bn, g):
    with torch.no_grad():
        C = bn.num_features
        bn.weight.copy_(torch.rand(C, generator=g) + 0.5)
        bn.weight[::7] *= -1.0
        bn.bias.copy_(torch.randn(C, generator=g) * 0.3)
        bn.running_mean.copy_(torch.randn(C, generator=g) * 0.3)
        bn.running_var.copy_(torch.rand(C, generator=g) + 0.5)


def _seed(mod, g):
    for m in mod.modules():
        if isinstance(m, (torch.nn.Conv2d, torch.nn.ConvTranspose2d)):
            fan = m.weight[0].numel() if isinstance(m, torch.nn.Conv2d) else m.weight.shape[0] * 4
            with torch.no_grad():
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) / fan ** 0.5)
        elif isinstance(m, torch.nn.BatchNorm2d):
            _seed_bn(m, g)
    return mod.eval()


def _bn_eval(h, m):
    return F.batch_norm(h, m.running_mean, m.running_var, m.weight, m.bias, False, 0.0, m.eps)


def _ref_block(blk, x):
    s = blk.stride
    if hasattr(blk, "conv3"):
        o = F.relu(_bn_eval(F.conv2d(x, blk.conv1.weight), blk.bn1))
        o = F.relu(_bn_eval(F.conv2d(o, blk.conv2.weight, stride=s, padding=1), blk.bn2))
        o = _bn_eval(F.conv2d(o, blk.conv3.weight), blk.bn3)
    else:
        o = F.relu(_bn_eval(F.conv2d(x, blk.conv1.weight, stride=s, padding=1), blk.bn1))
        o = _bn_eval(F.conv2d(o, blk.conv2.weight, padding=1), blk.bn2)
    idn = x
    if blk.downsample is not None:
        idn = _bn_eval(F.conv2d(x, blk.downsample[0].weight, stride=s), blk.downsample[1])
    return F.relu(o + idn)


def _down(ci, co, s):
    return torch.nn.Sequential(torch.nn.Conv2d(ci, co, kernel_size=1, stride=s, bias=False), torch.nn.BatchNorm2d(co))


def _group(name):
    from models.backbones.residuals import BasicBlock, Bottleneck
    if name == "basic64":
        return BasicBlock(64, 64), 64, 16
    if name == "basic64-128s2":
        return BasicBlock(64, 128, 2, _down(64, 128, 2)), 64, 16
    if name == "bottleneck256":
        return Bottleneck(256, 64), 256, 16
    if name == "bottleneck256-512s2":
        return Bottleneck(256, 128, 2, _down(256, 512, 2)), 256, 16
    return torch.nn.Sequential(torch.nn.ConvTranspose2d(512, 256, 4, stride=2, padding=1, bias=False),
                               torch.nn.BatchNorm2d(256)), 512, 8


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("name", ["basic64", "basic64-128s2", "bottleneck256", "bottleneck256-512s2", "deconv512-256"])
def test_folded_groups_match_fp32_eval(name, dtype):
    from scdhip import infer
    g = torch.Generator().manual_seed(97)
    mod, Ci, S = _group(name)
    _seed(mod, g)
    x = torch.randn(2, Ci, S, S, generator=g).to(dtype)            # the 16-bit input both sides see
    with torch.no_grad():
        if name.startswith("deconv"):
            ref = F.relu(_bn_eval(F.conv_transpose2d(x.float(), mod[0].weight, stride=2, padding=1), mod[1]))
        else:
            ref = _ref_block(mod, x.float())
    mod = mod.to(DEV)
    fn = infer.fold_deconv(mod[0], mod[1], dtype) if name.startswith("deconv") else infer.fold_block(mod, dtype)
    got = nchw(fn(nhwc(x, dtype)))
    assert got.shape == ref.shape and torch.isfinite(got).all()
    scale = 0.25 if dtype == torch.float16 else 1.0
    rms = ref.square().mean().sqrt().item()
    err = (got - ref).abs()
    mx, me = err.max().item() / rms, err.square().mean().sqrt().item() / rms
    print("%-20s max|err|/rms %.5f  rms(err)/rms %.6f" % (name, mx, me))
    assert mx <= TOL_RMS * scale and me <= TOL_MEAN * scale, (name, mx, me)


# ------------------------------------------------------------------ the folded model

def _plugin_model(name):
    plugin = importlib.import_module("trainer.model." + name)
    entries, topo = O.model_spec(plugin.modelParams["numLayers"], plugin.modelParams["dims"])
    state = O.hash_weights(entries)
    m = plugin.model(**plugin.modelParams)
    m.load_state_dict(state)
    return m, state, topo


@pytest.mark.parametrize("name,S", [("centerOffsetRes10", 512), ("centerOffsetRes50", 256)])
def test_folded_model_fp32(name, S):
    """fold(model) in fp32 against the CPU oracle's eval forward (rtol = atol = 1e-3, the project's F1 tolerance) and
    against the HIP eval forward (atol 5e-5: folding moves the fp32 oracle by <= 1.43e-6 against itself and 2.1e-6
    against float64; the rest is the GPU's summation order).  Measured on MI355X, fold vs HIP eval, max |diff|:
    Res10 512^2 heatmap 4.8e-7, regr 4.2e-7, offset 4.4e-7; Res50 256^2 heatmap 1.2e-6, regr 1.1e-6, offset 1.2e-6."""
    from scdhip import infer
    m, state, topo = _plugin_model(name)
    m = m.to(DEV).eval().set_compute_dtype(torch.float32)
    x = T.batch_inputs(21, 2, S)
    fm = infer.fold(m)
    with torch.no_grad():
        got = fm(x.to(DEV), decode=False)[0]
        hip = m(x.to(DEV), decode=False)[0]
        P, Bf = O.split_state({k: v.clone() for k, v in state.items()})
        ref = O.forward(P, Bf, x, topo, train=False)
    for k in ("heatmap", "regr", "offset"):
        d = (got[k] - hip[k]).abs().max().item()
        print("%s %s fold vs HIP eval: max |diff| %.3e" % (name, k, d))
        torch.testing.assert_close(got[k].cpu(), ref[k], rtol=1e-3, atol=1e-3)
        assert d <= 5e-5, (k, d)


def test_folded_forward_makes_no_bn_and_no_pack_call(monkeypatch):
    from scdhip import infer
    from scdhip import lib as L
    m, _, _ = _plugin_model("centerOffsetRes10")
    fm = infer.fold(m.to(DEV).eval())
    x = T.batch_inputs(22, 1, 256).to(DEV)
    fm(x, decode=True)
    names = []
    real = L.call

    def call(name, *args):
        names.append(name)
        return real(name, *args)

    monkeypatch.setattr(L, "call", call)
    fm(x, decode=True)
    torch.cuda.synchronize()
    assert names and not [n for n in names if n.startswith("scd_bn_") or n.startswith("scd_pack_")], names
    # one per folded conv: 8 block convs, the 3 downsample convs of layer2-4 and 3 deconvs
    assert names.count("scd_conv_gemm_res") == 14
    assert not any(p.requires_grad for p in fm.parameters())


def test_wrapper_around_folded_model_and_refold():
    from scdhip import infer
    from trainer.wrappers.centerOffsetResidual import Wrapper
    m, _, _ = _plugin_model("centerOffsetRes10")
    m = m.to(DEV).eval()
    fm = infer.fold(m)
    x = T.batch_inputs(23, 2, 256).to(DEV)
    a = Wrapper(fm)(x)
    assert a.shape == (10, 2, 100)
    with torch.no_grad():
        m.layer1[0].bn1.weight.mul_(0.5)
    assert torch.equal(Wrapper(fm)(x), a)                  # a snapshot
    fm.refold()
    b = Wrapper(fm)(x)
    assert not torch.equal(b, a)
    assert torch.equal(b, Wrapper(infer.fold(m))(x))


# ------------------------------------------------------------------ export

def test_export_fold_mode(tmp_path):
    from scdhip import export, infer
    from trainer.wrappers.centerOffsetResidual import Wrapper
    x = T.batch_inputs(5, 2, 256).to(DEV)
    m, _, _ = _plugin_model("centerOffsetRes10")
    m = m.to(DEV)
    path = str(tmp_path / "res10_fold.pt")
    export.trace("centerOffsetRes10", m, x, path, mode="fold", dtype="fp32")
    loaded = export.load(path)
    assert isinstance(loaded, torch.jit.ScriptModule)
    got = loaded(x)
    m2, _, _ = _plugin_model("centerOffsetRes10")
    m2 = m2.to(DEV).eval().set_compute_dtype(torch.float32)
    want = Wrapper(infer.fold(m2))(x)
    assert got.shape == (10, 2, 100) and torch.equal(got, want)
    # against the eval mode of the same archive format: scores within 1e-4, integer rows equal wherever the eval
    # scores are strictly ordered (near-tied scores may swap; the rule of test_f4_decode)
    pe = str(tmp_path / "res10_eval.pt")
    export.trace("centerOffsetRes10", m, x, pe, mode="eval", dtype="fp32")
    ev = export.load(pe)(x)
    assert torch.allclose(got[0], ev[0], rtol=0, atol=1e-4)
    s = ev[0]
    # (two scores that each move by <= 1e-4 keep their order where they are more than 2e-4 apart)
    gap = torch.ones_like(s, dtype=torch.bool)
    gap[:, 1:] &= (s[:, :-1] - s[:, 1:]) > 2e-4
    gap[:, :-1] &= (s[:, :-1] - s[:, 1:]) > 2e-4
    print("strictly ordered slots: %.3f" % gap.float().mean().item())
    for r in (1, 2, 3):
        assert torch.equal(got[r][gap], ev[r][gap]), r
    # changing a parameter tensor of the loaded module refolds
    with torch.no_grad():
        for n, p in loaded.named_parameters():
            if n.endswith("layer1.0.bn1.weight"):
                p.mul_(0.5)
                m2.layer1[0].bn1.weight.mul_(0.5)
                break
        else:
            raise AssertionError("parameter not found")
    got2 = loaded(x)
    assert not torch.equal(got2, got)
    assert torch.equal(got2, Wrapper(infer.fold(m2))(x))
