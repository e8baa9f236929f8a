"""The BatchNorm kernel family of libscdhip (csrc/bn.hip) against plain torch float64, at every loop and row width.

Every reference is built in float64 from the inputs as stored (16-bit or fp32), never from another scd kernel's output.
Channel classes per dtype (E = channels per 16 B): the smallest row, a row whose chunks divide 256, a row of exactly
256 chunks, and a row of more than 256 chunks (channel windows in the elementwise kernels, channel slices in the
reductions).  "Ragged" row counts are {1, 3, 8 * rpi + 1} with rpi = 256 / min(C / E, 256) row lanes per block.  The
long cases are sized from the device so that the unrolled main loops of bn_apply_kernel (U = 4) and
bn_bwd_apply_kernel (U = 2) run and end in a ragged tail whatever grid the occupancy query gives.

Bounds: one rounding to the output type (2^-8 bf16, 2^-11 fp16 relative) plus 4 * 2^-24 of the sum of the absolute
terms of the fp32 expression; the reductions are exact on integer-valued inputs and within the first-order bound
n * 2^-24 * sum|term| on random ones.  Per-channel shifts / constant coefficients are kept >= 0.25 in magnitude so
that no fp16 result lands in the subnormal range, where a rounding is absolute (2^-25) rather than relative."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
ERR_ARG = 9001                      # SCD_ERR_ARG
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DTYPES = [F32, BF16, F16]
EPC = {F32: 4, BF16: 8, F16: 8}     # channels per 16-B chunk
ULP_OUT = {F32: 0.0, BF16: 2.0 ** -8, F16: 2.0 ** -11}
C_CLASSES = {F32: [4, 64, 1024, 2048], BF16: [8, 16, 64, 2048, 4096], F16: [8, 16, 64, 2048, 4096]}
DC = [(d, C) for d in DTYPES for C in C_CLASSES[d]]
DC_IDS = ["%s-%d" % (str(d).split(".")[1], C) for d, C in DC]
U24 = 2.0 ** -24
U23 = 2.0 ** -23


def _ops():
    from scdhip import ops
    return ops


def gen(seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return g


def normal(g, shape, dtype=F32, mean=0.25, std=1.5):
    return (torch.randn(shape, device=DEV, generator=g) * std + mean).to(dtype)


def ints(g, lo, hi, shape, dtype):
    return torch.randint(lo, hi + 1, shape, device=DEV, generator=g).to(dtype)


def away_from_zero(g, C, std=0.5, floor=0.25):
    """Per-channel N(0, std^2) values pushed to magnitude >= floor (see the module docstring)."""
    v = torch.randn(C, device=DEV, generator=g) * std
    return torch.where(v < 0, v - floor, v + floor)


def ragged_rows(C, dtype):
    rpi = 256 // min(C // EPC[dtype], 256)
    return [1, 3, 8 * rpi + 1]


def long_rows(C, dtype):
    """An odd row count with rows * C / E > 4 * T + 256 vectors, T the most threads the device can hold: more than four
    grid strides of any launch, so the U = 4 and U = 2 main loops run and a ragged tail follows."""
    p = torch.cuda.get_device_properties(0)
    T = p.multi_processor_count * p.max_threads_per_multi_processor
    cpr = C // EPC[dtype]
    rows = ((4 * T + 256) // cpr + 1) | 1
    assert rows % 2 == 1 and rows * cpr > 4 * T + 256
    return rows


def state(ops, **kw):
    st = ops.BNState()
    for k, v in kw.items():
        setattr(st, k, v)
    return st


def status(name, *args):
    """The C-ABI status of a call (ops.L.call raises on a non-zero one)."""
    ops = _ops()
    return getattr(ops.L.lib(), name)(*args)


def assert_elementwise(got, ref, bound, what):
    err = (got.double() - ref).abs()
    bad = ~(err <= bound)
    if bad.any():
        i = torch.nonzero(bad.reshape(-1))[0].item()
        raise AssertionError("%s: %d of %d elements over the bound; first at %d: got %r ref %r bound %r, worst err/bound %g"
                             % (what, int(bad.sum()), bad.numel(), i, got.reshape(-1)[i].item(),
                                ref.reshape(-1)[i].item(), bound.reshape(-1)[i].item(),
                                (err / bound.clamp_min(1e-300)).max().item()))


# ------------------------------------------------------------------ 1. statistics -> per-channel state

def spread(g, total, nrep):
    """[nrep][...] float64 parts of `total` (random positive shares)."""
    w = torch.rand((nrep,) + tuple(total.shape), device=DEV, generator=g, dtype=torch.float64) + 0.05
    return (w / w.sum(0)) * total


def f32_as_f64(v):
    return torch.tensor(v, dtype=F32).double().item()


def finalize_ref(S, Q, count, gamma, beta, rm, rv, momentum, eps):
    """float64 training-mode BatchNorm state from the sums; no Bessel correction at count == 1 (the kernel's rule)."""
    mom, eps = f32_as_f64(momentum), f32_as_f64(eps)
    mean = S / count
    var = (Q / count - mean * mean).clamp_min(0.0)
    invstd = 1.0 / torch.sqrt(var + eps)
    g64, b64 = gamma.double(), beta.double()
    scale = g64 * invstd
    unb = var * count / (count - 1.0) if count > 1 else var
    r = dict(mean=mean, invstd=invstd, scale=scale, shift=b64 - mean * scale,
             rm=(1.0 - mom) * rm.double() + mom * mean, rv=(1.0 - mom) * rv.double() + mom * unb)
    r["shift_mag"] = b64.abs() + (mean * scale).abs()
    r["rm_mag"] = ((1.0 - mom) * rm.double()).abs() + (mom * mean).abs()
    r["rv_mag"] = ((1.0 - mom) * rv.double()).abs() + (mom * unb).abs()
    return r


def check_finalize(out, r, what):
    mean, invstd, scale, shift, rm, rv = out
    assert_elementwise(mean, r["mean"], U23 * r["mean"].abs(), what + " mean")
    assert_elementwise(invstd, r["invstd"], U23 * r["invstd"].abs(), what + " invstd")
    assert_elementwise(scale, r["scale"], U23 * r["scale"].abs(), what + " scale")
    assert_elementwise(shift, r["shift"], 2 * U23 * r["shift_mag"], what + " shift")
    assert_elementwise(rm, r["rm"], 2 * U23 * r["rm_mag"], what + " running_mean")
    assert_elementwise(rv, r["rv"], 2 * U23 * r["rv_mag"], what + " running_var")
    for t in out:
        assert torch.isfinite(t).all(), what


def run_finalize(ops, stats, nrep, C, count, gamma, beta, rm, rv, nbt, momentum=0.1, eps=1e-5):
    o = torch.full((4, C), float("nan"), device=DEV)
    ops.L.call("scd_bn_finalize", ops.ptr(stats), nrep, C, float(count), ops.ptr(gamma), ops.ptr(beta), ops.ptr(rm),
               ops.ptr(rv), ops.ptr(nbt), momentum, eps, ops.ptr(o[0]), ops.ptr(o[1]), ops.ptr(o[2]), ops.ptr(o[3]),
               ops.stream())
    return o[0], o[1], o[2], o[3]


def bn_params(g, C):
    gamma = torch.rand(C, device=DEV, generator=g) + 0.5
    beta = torch.randn(C, device=DEV, generator=g) * 0.3
    rm = torch.randn(C, device=DEV, generator=g) * 0.5
    rv = torch.rand(C, device=DEV, generator=g) + 0.5
    return gamma, beta, rm, rv


def random_sums(g, C, count):
    m = torch.randn(C, device=DEV, generator=g, dtype=torch.float64) * 2.0
    v = torch.rand(C, device=DEV, generator=g, dtype=torch.float64) * 3.0 + 0.1
    return count * m, count * (v + m * m)


@pytest.mark.parametrize("nrep", [1, 64, 100])
@pytest.mark.parametrize("C", [1, 5, 64, 2048])
def test_bn_finalize_training_matches_float64(C, nrep):
    """mean, invstd, scale, shift within one fp32 rounding of float64 (2^-23 relative; two for shift and the running
    statistics, relative to the sum of their absolute terms), num_batches_tracked counted, every replica read re-zeroed,
    and a second call on the same buffer with new sums gives the new result."""
    ops = _ops()
    g = gen(1000 * C + nrep)
    gamma, beta, rm, rv = bn_params(g, C)
    nbt = torch.zeros(1, dtype=torch.int64, device=DEV)
    stats = torch.zeros(nrep, 2, C, dtype=torch.float64, device=DEV)
    for call, count in enumerate((70, 333)):
        S, Q = random_sums(g, C, count)
        stats.copy_(spread(g, torch.stack([S, Q]), nrep))
        tot = stats.sum(0)
        r = finalize_ref(tot[0], tot[1], count, gamma, beta, rm, rv, 0.1, 1e-5)
        mean, invstd, scale, shift = run_finalize(ops, stats, nrep, C, count, gamma, beta, rm, rv, nbt)
        torch.cuda.synchronize()
        check_finalize((mean, invstd, scale, shift, rm, rv), r, "call %d" % call)
        assert nbt.item() == call + 1
        assert torch.equal(stats, torch.zeros_like(stats))


def test_bn_finalize_eval_mode_uses_running_statistics():
    """stats == NULL: the state comes from the running statistics, which (and num_batches_tracked) stay as they were."""
    ops = _ops()
    C = 69
    g = gen(7)
    gamma, beta, rm, rv = bn_params(g, C)
    rm0, rv0 = rm.clone(), rv.clone()
    nbt = torch.full((1,), 5, dtype=torch.int64, device=DEV)
    mean, invstd, scale, shift = run_finalize(ops, None, 0, C, 1.0, gamma, beta, rm, rv, nbt, momentum=0.0)
    torch.cuda.synchronize()
    assert torch.equal(rm, rm0) and torch.equal(rv, rv0) and nbt.item() == 5
    is64 = 1.0 / torch.sqrt(rv0.double() + f32_as_f64(1e-5))
    sc64 = gamma.double() * is64
    assert torch.equal(mean, rm0)
    assert_elementwise(invstd, is64, U23 * is64, "invstd")
    assert_elementwise(scale, sc64, U23 * sc64.abs(), "scale")
    assert_elementwise(shift, beta.double() - rm0.double() * sc64, 2 * U23 * (beta.double().abs() + (rm0.double() * sc64).abs()),
                       "shift")


def test_bn_finalize_edge_inputs():
    """A constant channel (variance exactly 0 and slightly negative), count = 1, and a channel with mean / sigma = 100
    whose invstd must survive the fp64 subtraction to 1e-6."""
    ops = _ops()
    eps = f32_as_f64(1e-5)
    # channels 0, 1: constant 3.0 over 70 samples (the second with sum x^2 a little short: negative variance);
    # channel 2: mean 100, sigma 1 over 1000 samples is fed on its own below (another count)
    for count, S, Q, want_is in ((70.0, [210.0, 210.0], [630.0, 630.0 * (1 - 1e-12)], [eps ** -0.5] * 2),
                                 (1.0, [2.5, -7.0], [6.25, 49.0], [eps ** -0.5] * 2),
                                 (1000.0, [100000.0, -100000.0], [1000.0 * 10001.0] * 2, [(1.0 + eps) ** -0.5] * 2)):
        C = 2
        g = gen(int(count))
        gamma, beta, rm, rv = bn_params(g, C)
        nbt = torch.zeros(1, dtype=torch.int64, device=DEV)
        stats = torch.zeros(64, 2, C, dtype=torch.float64, device=DEV)
        stats[0, 0] = torch.tensor(S, dtype=torch.float64)
        stats[0, 1] = torch.tensor(Q, dtype=torch.float64)
        r = finalize_ref(stats[0, 0].clone(), stats[0, 1].clone(), count, gamma, beta, rm, rv, 0.1, 1e-5)
        mean, invstd, scale, shift = run_finalize(ops, stats, 64, C, count, gamma, beta, rm, rv, nbt)
        torch.cuda.synchronize()
        want = torch.tensor(want_is, dtype=torch.float64, device=DEV)
        assert ((invstd.double() - want).abs() <= 1e-6 * want).all(), (count, invstd, want)
        check_finalize((mean, invstd, scale, shift, rm, rv), r, "count %g" % count)
        assert nbt.item() == 1


FIN_LAYERS = [(5, 70.0, True), (64, 333.0, True), (2048, 9.0, False), (16, 1.0, True)]   # C, count, training


def _fin_layer_inputs(i, C, count, training):
    g = gen(100 + i)
    gamma, beta, rm, rv = bn_params(g, C)
    S, Q = random_sums(g, C, count)
    stats = spread(g, torch.stack([S, Q]), 64) if training else None
    nbt = torch.full((1,), i, dtype=torch.int64, device=DEV)
    return dict(stats=stats, C=C, count=count, gamma=gamma, beta=beta, rm=rm, rv=rv, nbt=nbt,
                out=torch.full((4, C), float("nan"), device=DEV))


def _clone_layer(d):
    return {k: (v.clone() if torch.is_tensor(v) else v) for k, v in d.items()}


def _fin_args(ops, d):
    o = d["out"]
    return ops.L.BnFinArgs(ops.ptr(d["stats"]), 64 if d["stats"] is not None else 0, d["C"], float(d["count"]),
                           ops.ptr(d["gamma"]), ops.ptr(d["beta"]), ops.ptr(d["rm"]), ops.ptr(d["rv"]), ops.ptr(d["nbt"]),
                           0.1, 1e-5, ops.ptr(o[0]), ops.ptr(o[1]), ops.ptr(o[2]), ops.ptr(o[3]))


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_bn_finalize_n_is_bit_identical_to_single_calls(n):
    ops = _ops()
    base = [_fin_layer_inputs(i, *FIN_LAYERS[i]) for i in range(n)]
    one, many = [_clone_layer(d) for d in base], [_clone_layer(d) for d in base]
    for d in one:
        o = d["out"]
        ops.L.call("scd_bn_finalize", ops.ptr(d["stats"]), 64 if d["stats"] is not None else 0, d["C"], float(d["count"]),
                   ops.ptr(d["gamma"]), ops.ptr(d["beta"]), ops.ptr(d["rm"]), ops.ptr(d["rv"]), ops.ptr(d["nbt"]), 0.1, 1e-5,
                   ops.ptr(o[0]), ops.ptr(o[1]), ops.ptr(o[2]), ops.ptr(o[3]), ops.stream())
    args = (ops.L.BnFinArgs * n)(*[_fin_args(ops, d) for d in many])
    ops.L.call("scd_bn_finalize_n", args, n, ops.stream())
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(one, many)):
        assert torch.isfinite(b["out"]).all(), i
        for k in ("out", "rm", "rv", "nbt"):
            assert torch.equal(a[k], b[k]), (i, k)
        if a["stats"] is not None:
            assert torch.equal(b["stats"], torch.zeros_like(b["stats"])), i
        else:                                     # the eval-mode layer: running statistics and the count untouched
            assert torch.equal(b["rm"], base[i]["rm"]) and torch.equal(b["rv"], base[i]["rv"])
            assert b["nbt"].item() == i


def test_bn_finalize_n_rejects_bad_arguments():
    ops = _ops()
    layers = [_fin_layer_inputs(i, 8, 4.0, True) for i in range(5)]
    keep = [_clone_layer(d) for d in layers]
    args = (ops.L.BnFinArgs * 5)(*[_fin_args(ops, d) for d in layers])
    assert status("scd_bn_finalize_n", args, 0, ops.stream()) == ERR_ARG
    assert status("scd_bn_finalize_n", args, 5, ops.stream()) == ERR_ARG
    args[1].C = 0
    assert status("scd_bn_finalize_n", args, 2, ops.stream()) == ERR_ARG
    torch.cuda.synchronize()
    for a, b in zip(keep, layers):
        assert torch.equal(a["stats"], b["stats"]) and torch.equal(a["rm"], b["rm"]) and torch.equal(a["nbt"], b["nbt"])
        assert torch.isnan(b["out"]).all()


@pytest.mark.parametrize("C", [5, 300])
def test_stats_collapse_exact(C):
    """Integer-valued sums: replica 0 (scd_stats_collapse) / `out` (scd_stats_collapse_to) equal the float64 sum
    exactly; collapse zeroes replicas 1.., collapse_to zeroes all."""
    ops = _ops()
    R = ops.L.STAT_REPLICAS
    g = gen(C)
    src = ints(g, -1000, 1000, (R, 2 * C), torch.float64)
    want = src.sum(0)
    s = src.clone()
    ops.L.call("scd_stats_collapse", ops.ptr(s), R, C, ops.stream())
    torch.cuda.synchronize()
    assert torch.equal(s[0], want)
    assert torch.equal(s[1:], torch.zeros_like(s[1:]))
    s = src.clone()
    out = torch.full((2 * C,), float("nan"), dtype=torch.float64, device=DEV)
    ops.L.call("scd_stats_collapse_to", ops.ptr(s), R, C, ops.ptr(out), ops.stream())
    torch.cuda.synchronize()
    assert torch.equal(out, want)
    assert torch.equal(s, torch.zeros_like(s))


# ------------------------------------------------------------------ 2. scd_bn_apply

def apply_state(ops, g, C):
    return state(ops, scale=torch.rand(C, device=DEV, generator=g) + 0.5, shift=away_from_zero(g, C))


def check_apply(ops, dtype, C, rows, seed, forms, relus=(0, 1)):
    g = gen(seed)
    y = normal(g, (rows, C), dtype)
    res = normal(g, (rows, C), dtype)
    st, rst = apply_state(ops, g, C), apply_state(ops, g, C)
    y64, r64 = y.double(), res.double()
    base = y64 * st.scale.double() + st.shift.double()
    base_mag = (y64 * st.scale.double()).abs() + st.shift.double().abs()
    for form in forms:
        if form == 0:
            pre, mag = base, base_mag
        elif form == 1:
            pre, mag = base + r64, base_mag + r64.abs()
        else:
            t = r64 * rst.scale.double()
            pre, mag = base + (t + rst.shift.double()), base_mag + t.abs() + rst.shift.double().abs()
        for relu in relus:
            ref = pre.clamp_min(0.0) if relu else pre
            out = torch.full_like(y, float("nan"))
            ops.bn_apply(y, st, relu, res=res if form else None, rst=rst if form == 2 else None, out=out)
            torch.cuda.synchronize()
            assert_elementwise(out, ref, ULP_OUT[dtype] * ref.abs() + 4 * U24 * mag,
                               "bn_apply %s C %d rows %d form %d relu %d" % (dtype, C, rows, form, relu))


@pytest.mark.parametrize("dtype,C", DC, ids=DC_IDS)
def test_bn_apply_matches_float64(dtype, C):
    """out = [relu](y * sc + sh [+ res | + res * rs + rh]) on every element, all forms, the ragged row counts."""
    ops = _ops()
    for rows in ragged_rows(C, dtype):
        check_apply(ops, dtype, C, rows, 31 * C + rows, (0, 1, 2))


@pytest.mark.parametrize("dtype", DTYPES, ids=["float32", "bfloat16", "float16"])
def test_bn_apply_long_runs_unrolled_loop(dtype):
    """More than four grid strides of vectors and an odd row count: the U = 4 main loop and a ragged tail."""
    check_apply(_ops(), dtype, 64, long_rows(64, dtype), 5, (2,), (1,))


@pytest.mark.parametrize("dtype", DTYPES, ids=["float32", "bfloat16", "float16"])
def test_bn_apply_rejects_three_chunk_rows(dtype):
    ops = _ops()
    C = 3 * EPC[dtype]
    g = gen(3)
    y = normal(g, (7, C), dtype)
    st = apply_state(ops, g, C)
    out = torch.full_like(y, 7.0)
    rc = status("scd_bn_apply", ops.dt(y), ops.ptr(y), ops.ptr(out), C, y.numel(), ops.ptr(st.scale), ops.ptr(st.shift),
                0, 0, 0, 1, ops.stream())
    torch.cuda.synchronize()
    assert rc == ERR_ARG
    assert torch.equal(out, torch.full_like(y, 7.0))


# ------------------------------------------------------------------ 3. scd_bn_bwd_reduce, scd_bn_bwd_reduce2

def exact_params(C):
    c = torch.arange(C, device=DEV)
    mean = ((c % 7) - 3).float()
    invstd = torch.pow(2.0, ((c % 5) - 2).float())
    rsc = torch.ones(C, device=DEV)
    rsh = ((c % 5) - 2).float() + 0.5
    return mean, invstd, rsc, rsh


def exact_params_b(C):
    c = torch.arange(C, device=DEV)
    return ((c % 3) - 1).float(), torch.pow(2.0, ((c % 3) - 1).float())


def masked(dout, y, kind, mask, rsc, rsh):
    """float64 dz = dout where the ReLU is on, and the on-pattern."""
    if kind == 0:
        return dout.double(), None
    on = (mask.double() > 0) if kind == 1 else (y.double() * rsc.double() + rsh.double() > 0)
    return torch.where(on, dout.double(), torch.zeros((), dtype=torch.float64, device=DEV)), on


def reduce_ref(dout, y, kind, mask, rsc, rsh, mean, invstd):
    dz, _ = masked(dout, y, kind, mask, rsc, rsh)
    term = dz * (y.double() - mean.double()) * invstd.double()
    return torch.stack([dz.sum(0), term.sum(0)]), torch.stack([dz.abs().sum(0), term.abs().sum(0)])


def prefilled_stats(ops, C):
    R = ops.L.STAT_REPLICAS
    return ((torch.arange(R * 2 * C, device=DEV) % 17) - 8).double().view(R, 2, C)


def run_reduce(ops, dout, y, kind, mask, rsc, rsh, mean, invstd, stats):
    C = y.shape[-1]
    ops.L.call("scd_bn_bwd_reduce", ops.dt(y), ops.ptr(dout), ops.ptr(mask) if kind == 1 else 0, ops.ptr(y),
               ops.ptr(rsc) if kind == 2 else 0, ops.ptr(rsh) if kind == 2 else 0, ops.ptr(mean), ops.ptr(invstd), C,
               y.numel(), ops.ptr(stats), ops.stream())


@pytest.mark.parametrize("dtype,C", DC, ids=DC_IDS)
def test_bn_bwd_reduce_exact(dtype, C):
    """Integer-valued dout / y / mask, integer means and power-of-two invstd: every fp32 product and partial sum is an
    exact multiple of a power of two below 2^24 (|term| <= 44 invstd, rows <= 65,536), so the replica sum on top of a
    pre-filled buffer equals the float64 reference bit for bit -- a dropped, duplicated or mis-sliced row or channel
    chunk cannot hide.  In the > 256-chunk class channel c of slice s must land at stats[c0 + c] with row stride C."""
    ops = _ops()
    rpi = 256 // min(C // EPC[dtype], 256)
    mean, invstd, rsc, rsh = exact_params(C)
    for rows in ragged_rows(C, dtype) + [40 * rpi + 3]:
        assert rows <= 65536
        g = gen(17 * C + rows)
        dout = ints(g, -4, 4, (rows, C), dtype)
        y = ints(g, -8, 8, (rows, C), dtype)
        mask = ints(g, -2, 2, (rows, C), dtype)
        for kind in (0, 1, 2):
            stats = prefilled_stats(ops, C)
            want = stats.sum(0) + reduce_ref(dout, y, kind, mask, rsc, rsh, mean, invstd)[0]
            run_reduce(ops, dout, y, kind, mask, rsc, rsh, mean, invstd, stats)
            torch.cuda.synchronize()
            got = stats.sum(0)
            assert torch.equal(got, want), (dtype, C, rows, kind, int((got != want).sum()),
                                            torch.nonzero(got != want)[:4].tolist())


def test_bn_bwd_reduce_exact_more_rows_than_one_round():
    """More than 8 rows per row lane for every resident block (at most T / 256 blocks are resident, T the device's
    thread capacity): the host then sizes rows_per_block from the row count instead of its floor of 8 per lane.  bf16,
    C = 2048 (256 chunks, one row lane), an odd row count; both reduce kernels, exact."""
    ops = _ops()
    p = torch.cuda.get_device_properties(0)
    C, dtype = 2048, BF16
    rows = (8 * (p.multi_processor_count * p.max_threads_per_multi_processor // 256) + 5) | 1
    assert rows <= 65536
    mean, invstd, rsc, rsh = exact_params(C)
    mean_b, is_b = exact_params_b(C)
    g = gen(rows)
    dout = ints(g, -4, 4, (rows, C), dtype)
    y = ints(g, -8, 8, (rows, C), dtype)
    yb = ints(g, -8, 8, (rows, C), dtype)
    mask = ints(g, -2, 2, (rows, C), dtype)
    stats = prefilled_stats(ops, C)
    want = stats.sum(0) + reduce_ref(dout, y, 2, None, rsc, rsh, mean, invstd)[0]
    run_reduce(ops, dout, y, 2, None, rsc, rsh, mean, invstd, stats)
    sa, sb = prefilled_stats(ops, C), prefilled_stats(ops, C) * 3.0
    want_a = sa.sum(0) + reduce_ref(dout, y, 1, mask, None, None, mean, invstd)[0]
    want_b = sb.sum(0) + reduce_ref(dout, yb, 1, mask, None, None, mean_b, is_b)[0]
    ops.L.call("scd_bn_bwd_reduce2", ops.dt(y), ops.ptr(dout), ops.ptr(mask), ops.ptr(y), ops.ptr(yb), ops.ptr(mean),
               ops.ptr(invstd), ops.ptr(mean_b), ops.ptr(is_b), C, y.numel(), ops.ptr(sa), ops.ptr(sb), ops.stream())
    torch.cuda.synchronize()
    assert torch.equal(stats.sum(0), want)
    assert torch.equal(sa.sum(0), want_a) and torch.equal(sb.sum(0), want_b)


@pytest.mark.parametrize("dtype,C", DC, ids=DC_IDS)
def test_bn_bwd_reduce2_exact(dtype, C):
    """Both layers' sums of the pair kernel equal the single-layer float64 reference exactly."""
    ops = _ops()
    rpi = 256 // min(C // EPC[dtype], 256)
    mean_a, is_a, _, _ = exact_params(C)
    mean_b, is_b = exact_params_b(C)
    for rows in ragged_rows(C, dtype) + [40 * rpi + 3]:
        g = gen(19 * C + rows)
        dout = ints(g, -4, 4, (rows, C), dtype)
        ya = ints(g, -8, 8, (rows, C), dtype)
        yb = ints(g, -8, 8, (rows, C), dtype)
        mask = ints(g, -2, 2, (rows, C), dtype)
        sa, sb = prefilled_stats(ops, C), prefilled_stats(ops, C) * 3.0
        want_a = sa.sum(0) + reduce_ref(dout, ya, 1, mask, None, None, mean_a, is_a)[0]
        want_b = sb.sum(0) + reduce_ref(dout, yb, 1, mask, None, None, mean_b, is_b)[0]
        ops.L.call("scd_bn_bwd_reduce2", ops.dt(ya), ops.ptr(dout), ops.ptr(mask), ops.ptr(ya), ops.ptr(yb), ops.ptr(mean_a),
                   ops.ptr(is_a), ops.ptr(mean_b), ops.ptr(is_b), C, ya.numel(), ops.ptr(sa), ops.ptr(sb), ops.stream())
        torch.cuda.synchronize()
        assert torch.equal(sa.sum(0), want_a), (dtype, C, rows, "a")
        assert torch.equal(sb.sum(0), want_b), (dtype, C, rows, "b")


def test_bn_bwd_reduce2_rejects_null_operands():
    ops = _ops()
    C, rows = 64, 9
    g = gen(2)
    t = [ints(g, -2, 2, (rows, C), BF16) for _ in range(4)]
    mean, invstd, _, _ = exact_params(C)
    for null in (1, 2, 3):          # mask, ya, yb
        p = [ops.ptr(x) for x in t]
        p[null] = 0
        sa, sb = prefilled_stats(ops, C), prefilled_stats(ops, C)
        rc = status("scd_bn_bwd_reduce2", ops.dt(t[0]), p[0], p[1], p[2], p[3], ops.ptr(mean), ops.ptr(invstd), ops.ptr(mean),
                    ops.ptr(invstd), C, rows * C, ops.ptr(sa), ops.ptr(sb), ops.stream())
        torch.cuda.synchronize()
        assert rc == ERR_ARG, null
        assert torch.equal(sa, prefilled_stats(ops, C)) and torch.equal(sb, prefilled_stats(ops, C))


def relu_threshold_guard(dout, y, sc, sh, what, factor=4.0):
    """Elements whose recomputed BN+ReLU pre-activation lies within factor * 2^-23 * (|y sc| + |sh|) of zero may switch
    either way in fp32: their share is asserted <= 1e-5 and their gradient is zeroed in the input, so they add nothing
    to either side."""
    t = y.double() * sc.double()
    near = (t + sh.double()).abs() <= factor * U23 * (t.abs() + sh.double().abs())
    share = near.double().mean().item()
    print("relu-threshold share %s: %.3g (%d of %d)" % (what, share, int(near.sum()), near.numel()))
    assert share <= 1e-5, (what, share)
    dout[near] = 0
    return share


def random_channel_params(g, C):
    mean = torch.randn(C, device=DEV, generator=g) * 0.5 + 0.25
    invstd = torch.rand(C, device=DEV, generator=g) + 0.5
    rsc = torch.rand(C, device=DEV, generator=g) + 0.5
    rsh = torch.randn(C, device=DEV, generator=g) * 0.5
    return mean, invstd, rsc, rsh


@pytest.mark.parametrize("dtype,C", DC, ids=DC_IDS)
def test_bn_bwd_reduce_random(dtype, C):
    """N(0.25, 1.5^2) inputs, the three mask kinds, scd_bn_bwd_reduce and both layers of scd_bn_bwd_reduce2: per channel
    within n * 2^-24 * sum|term| of float64 (the order-independent first-order bound of an fp32 sum of n rows; n >= 9
    covers the three roundings inside a term too, n <= 2048 keeps the bound below one row's contribution)."""
    ops = _ops()
    rpi = 256 // min(C // EPC[dtype], 256)
    for rows in (min(8 * rpi + 1, 2047), 67):
        g = gen(23 * C + rows)
        dout = normal(g, (rows, C), dtype)
        y = normal(g, (rows, C), dtype)
        yb = normal(g, (rows, C), dtype)
        mask = normal(g, (rows, C), dtype)
        mean, invstd, rsc, rsh = random_channel_params(g, C)
        mean_b, is_b, _, _ = random_channel_params(g, C)
        relu_threshold_guard(dout, y, rsc, rsh, "reduce %s C %d rows %d" % (dtype, C, rows))
        for kind in (0, 1, 2):
            stats = ops.new_stats(C, DEV).view(-1, 2, C)
            ref, mag = reduce_ref(dout, y, kind, mask, rsc, rsh, mean, invstd)
            run_reduce(ops, dout, y, kind, mask, rsc, rsh, mean, invstd, stats)
            torch.cuda.synchronize()
            assert_elementwise(stats.sum(0), ref, rows * U24 * mag, "reduce %s C %d rows %d kind %d" % (dtype, C, rows, kind))
        sa, sb = ops.new_stats(C, DEV).view(-1, 2, C), ops.new_stats(C, DEV).view(-1, 2, C)
        ref_a, mag_a = reduce_ref(dout, y, 1, mask, None, None, mean, invstd)
        ref_b, mag_b = reduce_ref(dout, yb, 1, mask, None, None, mean_b, is_b)
        ops.L.call("scd_bn_bwd_reduce2", ops.dt(y), ops.ptr(dout), ops.ptr(mask), ops.ptr(y), ops.ptr(yb), ops.ptr(mean),
                   ops.ptr(invstd), ops.ptr(mean_b), ops.ptr(is_b), C, y.numel(), ops.ptr(sa), ops.ptr(sb), ops.stream())
        torch.cuda.synchronize()
        assert_elementwise(sa.sum(0), ref_a, rows * U24 * mag_a, "reduce2 a %s C %d rows %d" % (dtype, C, rows))
        assert_elementwise(sb.sum(0), ref_b, rows * U24 * mag_b, "reduce2 b %s C %d rows %d" % (dtype, C, rows))


# ------------------------------------------------------------------ 4. scd_bn_bwd_finalize, scd_bn_bwd_finalize_n

def bwd_fin_inputs(seed, C, count, gscale, with_gamma=True, nrep=64):
    g = gen(seed)
    tot = torch.randn(2, C, device=DEV, generator=g, dtype=torch.float64) * 50.0
    return dict(stats=spread(g, tot, nrep), nrep=nrep, C=C, count=count, gscale=gscale,
                gamma=(torch.rand(C, device=DEV, generator=g) + 0.5) if with_gamma else None,
                mean=torch.randn(C, device=DEV, generator=g) * 2.0, invstd=torch.rand(C, device=DEV, generator=g) + 0.5,
                dgamma=torch.randn(C, device=DEV, generator=g), dbeta=torch.randn(C, device=DEV, generator=g),
                coef=torch.full((3, C), float("nan"), device=DEV))


def bwd_fin_ref(d):
    tot = d["stats"].sum(0)
    s, q = tot[0], tot[1]
    gs = f32_as_f64(d["gscale"])
    g64 = d["gamma"].double() if d["gamma"] is not None else torch.ones(d["C"], dtype=torch.float64, device=DEV)
    is64, mu = d["invstd"].double(), d["mean"].double()
    sc = g64 * is64
    k1, k2 = s / d["count"], q / d["count"]
    t1, t2 = -sc * k1, sc * is64 * k2 * mu
    return dict(dgamma=(d["dgamma"].double() + gs * q, d["dgamma"].double().abs() + (gs * q).abs()),
                dbeta=(d["dbeta"].double() + gs * s, d["dbeta"].double().abs() + (gs * s).abs()),
                c0=(sc, sc.abs()), c1=(-sc * is64 * k2, (sc * is64 * k2).abs()), c2=(t1 + t2, t1.abs() + t2.abs()))


def run_bwd_finalize(ops, d):
    ops.L.call("scd_bn_bwd_finalize", ops.ptr(d["stats"]), d["nrep"], d["C"], float(d["count"]), ops.ptr(d["gamma"]),
               ops.ptr(d["mean"]), ops.ptr(d["invstd"]), ops.ptr(d["dgamma"]), ops.ptr(d["dbeta"]), d["gscale"],
               ops.ptr(d["coef"]), ops.stream())


def bwd_fin_args(ops, d):
    return ops.L.BnBwdFinArgs(ops.ptr(d["stats"]), d["nrep"], d["C"], float(d["count"]), ops.ptr(d["gamma"]),
                              ops.ptr(d["mean"]), ops.ptr(d["invstd"]), ops.ptr(d["dgamma"]), ops.ptr(d["dbeta"]),
                              d["gscale"], ops.ptr(d["coef"]))


@pytest.mark.parametrize("with_gamma", [True, False], ids=["gamma", "nogamma"])
@pytest.mark.parametrize("gscale", [1.0, 1.0 / 8, 1.0 / 1024])
@pytest.mark.parametrize("C", [5, 64, 2048])
def test_bn_bwd_finalize_matches_float64(C, gscale, with_gamma):
    """dgamma / dbeta accumulated onto pre-filled gradients and coef[3][C] within 4 * 2^-24 of the sum of the absolute
    terms of each expression; gamma NULL is gamma = 1; the replicas read are re-zeroed and a second call adds again."""
    ops = _ops()
    d = bwd_fin_inputs(1000 * C + int(1 / gscale), C, 70.0, gscale, with_gamma, nrep=64 if C != 5 else 100)
    for call in range(2):
        if call:
            d["stats"].copy_(bwd_fin_inputs(77 + C, C, 70.0, gscale, nrep=d["nrep"])["stats"])
        r = bwd_fin_ref(d)
        run_bwd_finalize(ops, d)
        torch.cuda.synchronize()
        for got, key in ((d["dgamma"], "dgamma"), (d["dbeta"], "dbeta"), (d["coef"][0], "c0"), (d["coef"][1], "c1"),
                         (d["coef"][2], "c2")):
            assert_elementwise(got, r[key][0], 4 * U24 * r[key][1], "%s call %d" % (key, call))
        assert torch.equal(d["stats"], torch.zeros_like(d["stats"]))


BWD_FIN_LAYERS = [(5, 70.0, 1.0, True), (64, 333.0, 1.0 / 8, False), (2048, 9.0, 1.0 / 1024, True), (16, 1.0, 1.0, True)]


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_bn_bwd_finalize_n_is_bit_identical_to_single_calls(n):
    ops = _ops()
    base = [bwd_fin_inputs(200 + i, C, count, gs, wg) for i, (C, count, gs, wg) in enumerate(BWD_FIN_LAYERS[:n])]
    one, many = [_clone_layer(d) for d in base], [_clone_layer(d) for d in base]
    for d in one:
        run_bwd_finalize(ops, d)
    args = (ops.L.BnBwdFinArgs * n)(*[bwd_fin_args(ops, d) for d in many])
    ops.L.call("scd_bn_bwd_finalize_n", args, n, ops.stream())
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(one, many)):
        assert torch.isfinite(b["coef"]).all(), i
        for k in ("coef", "dgamma", "dbeta", "stats"):
            assert torch.equal(a[k], b[k]), (i, k)
        assert torch.equal(b["stats"], torch.zeros_like(b["stats"])), i


def test_bn_bwd_finalize_n_rejects_bad_arguments():
    ops = _ops()
    layers = [bwd_fin_inputs(300 + i, 8, 4.0, 1.0) for i in range(5)]
    keep = [_clone_layer(d) for d in layers]

    def rc(n, **null):
        args = (ops.L.BnBwdFinArgs * 5)(*[bwd_fin_args(ops, d) for d in layers])
        for k, v in null.items():
            setattr(args[1], k, v)
        return status("scd_bn_bwd_finalize_n", args, n, ops.stream())
    assert rc(0) == ERR_ARG
    assert rc(5) == ERR_ARG
    assert rc(2, C=0) == ERR_ARG
    for field in ("stats", "invstd", "mean", "coef"):
        assert rc(2, **{field: None}) == ERR_ARG, field
    torch.cuda.synchronize()
    for a, b in zip(keep, layers):
        for k in ("stats", "dgamma", "dbeta"):
            assert torch.equal(a[k], b[k]), k
        assert torch.isnan(b["coef"]).all()


# ------------------------------------------------------------------ 5. scd_bn_bwd_apply, scd_bn_bwd_apply2

def random_coef(g, C):
    """[3][C]: a distinct per channel (1 + c / C), b random, c random with |c| >= 0.25."""
    a = 1.0 + torch.arange(C, device=DEV).float() / C
    return torch.stack([a, torch.randn(C, device=DEV, generator=g) * 0.5, away_from_zero(g, C)]).contiguous()


def bwd_apply_ref(dz, y, coef):
    c = coef.double()
    t0, t1 = c[0] * dz, c[1] * y.double()
    return t0 + t1 + c[2], t0.abs() + t1.abs() + c[2].abs()


def check_bwd_apply(ops, dtype, C, rows, seed, kinds, want_dz=(False, True)):
    g = gen(seed)
    dout = normal(g, (rows, C), dtype)
    y = normal(g, (rows, C), dtype)
    mask = normal(g, (rows, C), dtype)
    _, _, rsc, rsh = random_channel_params(g, C)
    coef = random_coef(g, C)
    if 2 in kinds:
        relu_threshold_guard(dout, y, rsc, rsh, "bwd_apply %s C %d rows %d" % (dtype, C, rows))
    for kind in kinds:
        dz64, on = masked(dout, y, kind, mask, rsc, rsh)
        ref, mag = bwd_apply_ref(dz64, y, coef)
        for with_dz in want_dz:
            dy = torch.full_like(y, float("nan"))
            dz = torch.full_like(y, float("nan")) if with_dz else None
            ops.L.call("scd_bn_bwd_apply", ops.dt(y), ops.ptr(dout), ops.ptr(mask) if kind == 1 else 0, ops.ptr(y),
                       ops.ptr(rsc) if kind == 2 else 0, ops.ptr(rsh) if kind == 2 else 0, ops.ptr(coef), C, y.numel(),
                       ops.ptr(dy), ops.ptr(dz), ops.stream())
            torch.cuda.synchronize()
            what = "bwd_apply %s C %d rows %d kind %d dz %d" % (dtype, C, rows, kind, with_dz)
            assert_elementwise(dy, ref, ULP_OUT[dtype] * ref.abs() + 4 * U24 * mag, what)
            if with_dz:
                assert torch.equal(dz.double(), dz64), what


@pytest.mark.parametrize("dtype,C", DC, ids=DC_IDS)
def test_bn_bwd_apply_matches_float64(dtype, C):
    """dy = a dz + b y + c per element (and dz = the masked dout exactly) for the three mask kinds at the ragged rows."""
    ops = _ops()
    for rows in ragged_rows(C, dtype):
        check_bwd_apply(ops, dtype, C, rows, 37 * C + rows, (0, 1, 2))


@pytest.mark.parametrize("dtype,kind", [(F32, 0), (BF16, 1), (F16, 2)], ids=["float32-nomask", "bfloat16-mask", "float16-recompute"])
def test_bn_bwd_apply_long_runs_unrolled_loop(dtype, kind):
    """More than four grid strides of vectors and an odd row count: the U = 2 main loop (one per mask kind) and a tail."""
    check_bwd_apply(_ops(), dtype, 64, long_rows(64, dtype), 9, (kind,), (True,))


def check_bwd_apply2(ops, dtype, C, rows):
    g = gen(41 * C + rows)
    dout = normal(g, (rows, C), dtype)
    ya = normal(g, (rows, C), dtype)
    yb = normal(g, (rows, C), dtype, mean=-0.5, std=2.0)
    mask = normal(g, (rows, C), dtype)
    ca, cb = random_coef(g, C), random_coef(g, C) * 0.75
    dz64, _ = masked(dout, ya, 1, mask, None, None)
    dya, dyb = torch.full_like(ya, float("nan")), torch.full_like(ya, float("nan"))
    ops.L.call("scd_bn_bwd_apply2", ops.dt(ya), ops.ptr(dout), ops.ptr(mask), ops.ptr(ya), ops.ptr(yb), ops.ptr(ca),
               ops.ptr(cb), C, ya.numel(), ops.ptr(dya), ops.ptr(dyb), ops.stream())
    torch.cuda.synchronize()
    for got, yv, coef, name in ((dya, ya, ca, "a"), (dyb, yb, cb, "b")):
        ref, mag = bwd_apply_ref(dz64, yv, coef)
        assert_elementwise(got, ref, ULP_OUT[dtype] * ref.abs() + 4 * U24 * mag,
                           "bwd_apply2 %s %s C %d rows %d" % (name, dtype, C, rows))


@pytest.mark.parametrize("dtype,C", DC, ids=DC_IDS)
def test_bn_bwd_apply2_matches_float64(dtype, C):
    """Both layers of the pair kernel: dy_a = a_a dz + b_a y_a + c_a, dy_b likewise, dz masked by the stored activation."""
    ops = _ops()
    for rows in ragged_rows(C, dtype):
        check_bwd_apply2(ops, dtype, C, rows)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["float32", "bfloat16"])
def test_bn_bwd_apply2_long_runs(dtype):
    """More than four grid strides of vectors and an odd row count: the pair kernel's main loop over several strides
    and a ragged last one."""
    check_bwd_apply2(_ops(), dtype, 64, long_rows(64, dtype))


# ------------------------------------------------------------------ 6. one composite against autograd

def _bn_module(C):
    bn = torch.nn.BatchNorm2d(C).to(DEV)
    with torch.no_grad():
        bn.weight.copy_(torch.linspace(0.5, 1.5, C))
        bn.bias.copy_(torch.linspace(-0.3, 0.3, C))
        bn.running_mean.copy_(torch.linspace(-0.5, 0.5, C))
        bn.running_var.copy_(torch.linspace(0.5, 2.0, C))
    return bn


def _exact_forward_stats(ops, y, C):
    stats = ops.new_stats(C, DEV)
    yd = y.double().reshape(-1, C)
    stats[:C] = yd.sum(0)
    stats[C:2 * C] = (yd * yd).sum(0)
    return stats, yd.shape[0]


class _Ref:
    """float64 torch.nn.functional.batch_norm(training=True) of an NHWC tensor with autograd leaves."""

    def __init__(self, bn, y):
        self.y = y.double().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
        self.w = bn.weight.detach().double().clone().requires_grad_(True)
        self.b = bn.bias.detach().double().clone().requires_grad_(True)
        self.rm, self.rv = bn.running_mean.double().clone(), bn.running_var.double().clone()
        self.rm0, self.rv0 = self.rm.clone(), self.rv.clone()
        self.z = F.batch_norm(self.y, self.rm, self.rv, self.w, self.b, training=True, momentum=f32_as_f64(bn.momentum),
                              eps=f32_as_f64(bn.eps))

    def terms(self, eps):
        """|y sc| + |sh| of z = y sc + sh, x-hat, and the batch mean / unbiased variance, in float64."""
        yd = self.y.detach()
        mean = yd.mean((0, 2, 3))
        var = yd.var((0, 2, 3), unbiased=False)
        invstd = 1.0 / torch.sqrt(var + f32_as_f64(eps))
        sc = self.w.detach() * invstd
        sh = self.b.detach() - mean * sc
        v = lambda t: t.view(1, -1, 1, 1)
        mag = (yd * v(sc)).abs() + v(sh).abs()
        xhat = (yd - v(mean)) * v(invstd)
        n = yd.numel() // yd.shape[1]
        return mag, xhat, mean, var * n / (n - 1)


def _nhwc(t):
    return t.permute(0, 2, 3, 1)


def _check_running(bn, ref, mean, unb, what):
    mom = f32_as_f64(bn.momentum)
    for got, r, r0, new in ((bn.running_mean, ref.rm, ref.rm0, mean), (bn.running_var, ref.rv, ref.rv0, unb)):
        assert_elementwise(got, r, 2 * U23 * (((1 - mom) * r0).abs() + (mom * new).abs()), what)
    assert bn.num_batches_tracked.item() == 1


def _check_param_grads(bn, ref, dz, xhat, what):
    """1e-5 relative to the sum of the absolute terms of each per-channel sum (<= 70 terms: summation error ~1e-6)."""
    assert_elementwise(bn.bias.grad, ref.b.grad, 1e-5 * dz.abs().sum((0, 2, 3)), what + " dbeta")
    assert_elementwise(bn.weight.grad, ref.w.grad, 1e-5 * (dz * xhat).abs().sum((0, 2, 3)), what + " dgamma")


COMPOSITE = [(F32, 64), (BF16, 64), (F16, 64), (F32, 2048)]
COMPOSITE_IDS = ["float32-64", "bfloat16-64", "float16-64", "float32-2048"]


@pytest.mark.parametrize("dtype,C", COMPOSITE, ids=COMPOSITE_IDS)
def test_bn_relu_forward_backward_matches_autograd(dtype, C):
    """ops.bn_finalize -> ops.bn_apply(relu) -> ops.bn_backward(relu) against float64 batch_norm + ReLU with autograd:
    out, dx, dgamma, dbeta and the running statistics."""
    ops = _ops()
    N, H, W = 2, 5, 7
    g = gen(C + 1)
    y = normal(g, (N, H, W, C), dtype)
    dout = normal(g, (N, H, W, C), dtype, mean=0.0, std=1.0)
    bn = _bn_module(C)
    ref = _Ref(bn, y)
    mag, xhat, mean, unb = ref.terms(bn.eps)
    near = _nhwc(ref.z.detach().abs() <= 8 * U23 * mag)
    print("relu-threshold share composite %s C %d: %d of %d" % (dtype, C, int(near.sum()), near.numel()))
    assert near.double().mean().item() <= 1e-5
    dout[near] = 0
    out_ref = torch.relu(ref.z)
    out_ref.backward(dout.double().permute(0, 3, 1, 2))
    stats, count = _exact_forward_stats(ops, y, C)
    st = ops.bn_finalize(bn, stats, C, count)
    out = ops.bn_apply(y, st, True)
    dx = ops.bn_backward(bn, st, dout, y, relu=True)
    torch.cuda.synchronize()
    o64, dx64 = _nhwc(out_ref.detach()), _nhwc(ref.y.grad)
    assert_elementwise(out, o64, 1e-5 * o64.abs().max() + ULP_OUT[dtype] * o64.abs(), "out")
    assert_elementwise(dx, dx64, 1e-5 * dx64.abs().max() + ULP_OUT[dtype] * dx64.abs(), "dx")
    dz = dout.double().permute(0, 3, 1, 2) * (ref.z.detach() > 0)
    _check_param_grads(bn, ref, dz, xhat, "bn")
    _check_running(bn, ref, mean, unb, "running")


@pytest.mark.parametrize("pair", [True, False], ids=["pair", "two-passes"])
@pytest.mark.parametrize("dtype,C", COMPOSITE, ids=COMPOSITE_IDS)
def test_bn_residual_join_matches_autograd(dtype, C, pair):
    """out = relu(bn_a(y_a) + bn_b(y_b)) through ops.bn_apply with a normalised residual and ops.bn_backward_pair
    (scd_bn_bwd_reduce2 / apply2 with BNPair on, two single passes with it off) against float64 autograd."""
    ops = _ops()
    N, H, W = 2, 5, 7
    g = gen(C + 2)
    ya = normal(g, (N, H, W, C), dtype)
    yb = normal(g, (N, H, W, C), dtype, mean=-0.5, std=2.0)
    dout = normal(g, (N, H, W, C), dtype, mean=0.0, std=1.0)
    bns = [_bn_module(C), _bn_module(C)]
    with torch.no_grad():
        bns[1].weight.mul_(0.75)
        bns[1].bias.add_(0.2)
    refs = [_Ref(bns[0], ya), _Ref(bns[1], yb)]
    ta, tb = refs[0].terms(bns[0].eps), refs[1].terms(bns[1].eps)
    z = refs[0].z + refs[1].z
    near = _nhwc(z.detach().abs() <= 8 * U23 * (ta[0] + tb[0]))
    print("relu-threshold share join %s C %d: %d of %d" % (dtype, C, int(near.sum()), near.numel()))
    assert near.double().mean().item() <= 1e-5
    dout[near] = 0
    out_ref = torch.relu(z)
    out_ref.backward(dout.double().permute(0, 3, 1, 2))
    sts = []
    for bn, y in zip(bns, (ya, yb)):
        stats, count = _exact_forward_stats(ops, y, C)
        sts.append(ops.bn_finalize(bn, stats, C, count))
    out = ops.bn_apply(ya, sts[0], True, res=yb, rst=sts[1])
    old = ops.BNPair.enabled
    ops.BNPair.enabled = pair
    try:
        dya, dyb = ops.bn_backward_pair(bns[0], sts[0], ya, bns[1], sts[1], yb, dout, out)
    finally:
        ops.BNPair.enabled = old
    torch.cuda.synchronize()
    o64 = _nhwc(out_ref.detach())
    assert_elementwise(out, o64, 1e-5 * o64.abs().max() + ULP_OUT[dtype] * o64.abs(), "out")
    dz = dout.double().permute(0, 3, 1, 2) * (z.detach() > 0)
    for name, bn, ref, t, dy in (("a", bns[0], refs[0], ta, dya), ("b", bns[1], refs[1], tb, dyb)):
        d64 = _nhwc(ref.y.grad)
        assert_elementwise(dy, d64, 1e-5 * d64.abs().max() + ULP_OUT[dtype] * d64.abs(), "dy_" + name)
        _check_param_grads(bn, ref, dz, t[1], name)
        _check_running(bn, ref, t[2], t[3], "running " + name)
