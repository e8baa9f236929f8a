"""conv_gemm_ring128_kernel (the LDS-DMA ring on the 128 x 128 tile) against conv_gemm_kernel<T,128,128> on the same
inputs, through scd_conv_gemm_sel: the outputs and the fp64 statistics must be equal bit for bit (the ring keeps the
register-staged kernel's MFMA order per output, its split-K halves included, and its epilogue), and the output is
held to a float64 torch convolution at test_kernels_gpu.py's 16-bit GEMM tolerance.

The shapes are the smallest that reach every path: more K stages than ring slots and fewer, one tile and a ragged
second one, a halo on all four sides, both K splits (1: fewer than 16 stages; 2: from 16 up, odd and even halves),
four sub-pixel phases of 1 / 2 / 2 / 4 taps in one launch, phases without taps, += into a filled output, the
statistics of the forward and of the BN-backward epilogue.

The stride-2 input gradient runs here as the four-phase launch on both kernels: the merged 2x2-tap form
(scd_conv_dgrad_s2) was not moved onto the new kernel and still belongs to the ping-pong kernel alone."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOL = {torch.bfloat16: 3e-2, torch.float16: 1e-2}      # tests/test_kernels_gpu.py TOL


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return (a - b).abs().max().item() / max(1e-6, b.abs().max().item())


def nhwc(t, dtype):
    return t.permute(0, 2, 3, 1).contiguous().to(DEV, dtype)


def nchw(t):
    return t.double().permute(0, 3, 1, 2).cpu()


def gemm_sel(kernel, x, wpack, y, Co, in_stride, out_stride, phases, stats=None, accumulate=False, bn_bwd=None):
    from scdhip import ops
    L = ops.L
    N, Hi, Wi, Ci = x.shape
    _, Ho, Wo, _ = y.shape
    bn = (None,) * 5
    if bn_bwd is not None:
        st, ybn = bn_bwd
        bn = (ops.ptr(ybn), ops.ptr(st["mean"]), ops.ptr(st["invstd"]), ops.ptr(st["scale"]), ops.ptr(st["shift"]))
    L.call("scd_conv_gemm_sel", ops.dt(x), kernel, ops.ptr(x), ops.ptr(wpack), ops.ptr(y), None, ops.ptr(stats), N, Hi,
           Wi, Ci, Ho, Wo, Co, in_stride, out_stride, wpack.shape[1], 0, int(accumulate), phases.n, phases.arr, *bn,
           ops.stream())
    return y


def both_kernels(x, wpack, shape, Co, in_stride, out_stride, phases, dtype, with_stats=False, fill=None, bn_bwd=None):
    """The launch on kernel 0 and on kernel 1 -> [(y, stats)] after asserting the two equal bit for bit."""
    from scdhip import ops
    res = []
    for kernel in (0, 1):
        y = torch.full(shape, float("nan"), device=DEV, dtype=dtype) if fill is None else fill.clone()
        stats = ops.new_stats(Co, DEV) if with_stats or bn_bwd is not None else None
        gemm_sel(kernel, x, wpack, y, Co, in_stride, out_stride, phases, stats=stats, accumulate=fill is not None,
                 bn_bwd=bn_bwd)
        torch.cuda.synchronize()
        res.append((y, stats))
    (y0, s0), (y1, s1) = res
    assert torch.isfinite(y1.float()).all()
    assert torch.equal(y0, y1), "outputs differ: max |d| %g" % (y0.float() - y1.float()).abs().max().item()
    if s0 is not None:
        assert s0.abs().sum().item() > 0
        assert torch.equal(s0, s1), "statistics differ"
    return res


def operands(seed, N, Cin, H, W, Cout, k, dtype):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, Cin, H, W, generator=g).to(dtype).double()
    w = (torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5).to(dtype).double()
    return g, x, w


FWD_CASES = [  # N, Cin, H, W, Cout, k, stride, pad, dtype
    (2, 64, 8, 8, 128, 3, 1, 1, torch.bfloat16),      # one tile, halo on all four sides, 9 stages: K split 1
    (2, 64, 8, 8, 128, 3, 1, 1, torch.float16),
    (1, 128, 24, 24, 256, 3, 2, 1, torch.bfloat16),   # 12 x 12 output: a ragged second tile; 18 stages: K split 2
    (2, 64, 16, 16, 128, 1, 2, 0, torch.bfloat16),    # one stage, shorter than the ring
    (1, 192, 9, 11, 128, 3, 1, 1, torch.bfloat16),    # 27 stages: K split 2 with a shorter second half
]


@pytest.mark.parametrize("case", FWD_CASES, ids=lambda c: "x".join(str(v).replace("torch.", "") for v in c))
def test_forward_with_statistics_and_plain(case):
    from scdhip import ops
    N, Cin, H, W, Cout, k, s, p, dtype = case
    _, x, w = operands(11, N, Cin, H, W, Cout, k, dtype)
    ref = F.conv2d(x, w, stride=s, padding=p)
    Ho, Wo = ref.shape[2], ref.shape[3]
    xg, wp = nhwc(x, dtype), ops.pack_weight(w.float().to(DEV), dtype, 0)
    ph = ops._fwd_phase(k, k, p, Ho, Wo)
    (_, _), (y, stats) = both_kernels(xg, wp, (N, Ho, Wo, Cout), Cout, s, 1, ph, dtype, with_stats=True)
    assert rel_err(nchw(y), ref) < TOL[dtype]
    st = stats.view(-1, 2, Cout).sum(0).cpu()
    scale = ref.abs().sum((0, 2, 3)).max().item()
    assert (st[0] - ref.sum((0, 2, 3))).abs().max().item() <= 1e-3 * scale      # fp32 partial sums of <= 288 terms
    (_, _), (yp, _) = both_kernels(xg, wp, (N, Ho, Wo, Cout), Cout, s, 1, ph, dtype)
    assert torch.equal(yp, y)                           # the plain store is the statistics variant's


@pytest.mark.parametrize("Cg,Cin", [(128, 128), (256, 256)])
def test_stride2_input_gradient_phases_and_accumulate(Cg, Cin):
    """The 3x3 / stride 2 / pad 1 input gradient as four sub-pixel phases of 1, 2, 2 and 4 taps in one launch (Cg =
    128: at most 8 stages, K split 1; Cg = 256: 16 stages in the four-tap phase, K split 2 in every phase), plain and
    += on a filled output."""
    from scdhip import ops
    dtype = torch.bfloat16
    N, Hq, Wq = 2, 8, 8
    g, dy, w = operands(12, N, Cg, Hq, Wq, Cg, 1, dtype)
    w = (torch.randn(Cg, Cin, 3, 3, generator=g) / (Cg * 9) ** 0.5).to(dtype).double()
    ref = F.conv_transpose2d(dy, w, stride=2, padding=1, output_padding=1)          # (N, Cin, 16, 16)
    dyg, wt = nhwc(dy, dtype), ops.pack_weight(w.float().to(DEV), dtype, 1)
    ph = ops._dgrad_phases(3, 3, 2, 1, 2 * Hq, 2 * Wq)
    assert sorted(p.ntaps for p in ph) == [1, 2, 2, 4]
    shape = (N, 2 * Hq, 2 * Wq, Cin)
    (_, _), (dx, _) = both_kernels(dyg, wt, shape, Cin, 1, 2, ph, dtype)
    assert rel_err(nchw(dx), ref) < TOL[dtype]
    base = torch.randn(shape, generator=g).to(dtype)
    (_, _), (dxa, _) = both_kernels(dyg, wt, shape, Cin, 1, 2, ph, dtype, fill=base.to(DEV))
    # += adds the rounded product to the stored value and rounds again: two roundings of the 16-bit type
    want = ref + nchw(base)
    assert rel_err(nchw(dxa), want) < TOL[dtype]


def test_phases_without_taps_store_zeros():
    """A 1x1 / stride 2 input gradient without accumulate: three of its four phases have no tap and no K stage, and
    their pixels must come out as zeros."""
    from scdhip import ops
    dtype = torch.bfloat16
    N, Hq, Wq, Cg, Cin = 2, 8, 8, 128, 128
    _, dy, w = operands(13, N, Cg, Hq, Wq, Cg, 1, dtype)
    w = w[:, :Cin]
    ref = F.conv_transpose2d(dy, w, stride=2, padding=0, output_padding=1)
    ph = ops._dgrad_phases(1, 1, 2, 0, 2 * Hq, 2 * Wq)
    assert sorted(p.ntaps for p in ph) == [0, 0, 0, 1]
    (_, _), (dx, _) = both_kernels(nhwc(dy, dtype), ops.pack_weight(w.float().to(DEV), dtype, 1),
                                   (N, 2 * Hq, 2 * Wq, Cin), Cin, 1, 2, ph, dtype)
    assert rel_err(nchw(dx), ref) < TOL[dtype]
    assert (dx[:, 1::2].float() == 0).all() and (dx[:, :, 1::2].float() == 0).all()


def test_bn_backward_sums_epilogue():
    """The input gradient of a 3x3 conv with the preceding BN+ReLU layer's backward sums in the epilogue (layer4's
    conv2): 18 stages, K split 2; output and both sums equal bit for bit."""
    from scdhip import ops
    dtype = torch.bfloat16
    N, H, W, C = 2, 9, 7, 128                             # 126 pixels: one ragged tile
    g, dy, w = operands(14, N, C, H, W, C, 3, dtype)
    ref = F.conv_transpose2d(dy, w, stride=1, padding=1)
    st = {"mean": torch.randn(C, generator=g) * 0.1, "invstd": torch.rand(C, generator=g) + 0.5,
          "scale": torch.rand(C, generator=g) + 0.5, "shift": torch.randn(C, generator=g) * 0.1}
    st = {k: v.to(DEV) for k, v in st.items()}
    ybn = torch.randn(N, H, W, C, generator=g).to(DEV, dtype)
    ph = ops._dgrad_phases(3, 3, 1, 1, H, W)
    (_, _), (dx, sums) = both_kernels(nhwc(dy, dtype), ops.pack_weight(w.float().to(DEV), dtype, 1), (N, H, W, C), C,
                                      1, 1, ph, dtype, bn_bwd=(st, ybn))
    assert rel_err(nchw(dx), ref) < TOL[dtype]
    # the sums are over the gradient as stored: float64 sums of the same 16-bit values, to the fp32 partial sums'
    # rounding (<= 126 terms of one sign pattern: 1e-4 of the sum of magnitudes)
    act = ybn.double() * st["scale"].double() + st["shift"].double() > 0
    dz = torch.where(act, dx.double(), torch.zeros((), dtype=torch.float64, device=DEV))
    xh = (ybn.double() - st["mean"].double()) * st["invstd"].double()
    got = sums.view(-1, 2, C).sum(0)
    for i, term in enumerate((dz, dz * xh)):
        want, mag = term.sum((0, 1, 2)), term.abs().sum((0, 1, 2))
        assert ((got[i] - want).abs() <= 1e-4 * mag + 1e-12).all(), i
