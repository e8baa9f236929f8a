"""Dynamic fp16 loss scaling on the GPU: the gradient guard kernel (scd_grad_guard), the optimizers' skipped step, the
lag rule through the pinned ring, grad_norm, a Res10 fp16 step end to end and the config path."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
ERR_ARG = 9001


@pytest.fixture(autouse=True)
def _process_wide_state():
    """ops.LossScale.f16 and defaultConfig.config are process-wide: put both back."""
    from configuration import defaultConfig
    from scdhip import ops
    scale, config = ops.LossScale.f16, dict(defaultConfig.config)
    yield
    ops.set_loss_scale(scale)
    defaultConfig.config.clear()
    defaultConfig.config.update(config)


# ------------------------------------------------------------------ the guard kernel

SIZES = [0, 1, 3, 4, 5, 255, 256, 257, 1023, 65537, 2 ** 22 + 5]      # the last: more than one pass of the grid


def _values(n, seed, huge=True):
    """Seeded normal values times 2^U(-30, 30), a few denormals and (huge) +-3e38 among them."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(n, generator=g, dtype=torch.float64)
         * torch.exp2(torch.rand(n, generator=g, dtype=torch.float64) * 60 - 30)).float()
    special = [1e-45, -3e-39, 3e38, -3e38, 1.1e-38] if huge else [1e-45, -3e-39, 1.1e-38]
    for k, v in enumerate(special):
        i = (k * 7 + 2) % max(n, 1)
        if i < n and n > len(special):
            x[i] = v
    return x


_CASES = {}


def _case(n):
    """(values, their exact float64 squares as a Python list) -- computed once per size and left unchanged."""
    if n not in _CASES:
        x = _values(n, 100 + n % 97)
        _CASES[n] = (x, (x.double() * x.double()).tolist())
    return _CASES[n]


class _Guard:
    def __init__(self):
        from scdhip import ops
        self.ws = torch.zeros(ops.grad_guard_workspace(0), dtype=torch.uint8, device=DEV)
        self.out = torch.full((3,), -7, dtype=torch.int64, device=DEV)      # stale non-zero contents

    def __call__(self, g, also=None):
        from scdhip import ops
        ops.grad_guard(g, self.ws, self.out[:2], self.out[2:], also=also)
        host = self.out.cpu()
        assert not self.ws.any(), "the workspace is left zero"
        return int(host[0]), int(host[1]), host[2:].view(torch.float64).item(), host[2].item()


def _close(got, ref, n):
    # the squares are exact in float64, so the error is the summation's alone: at most n - 1 roundings of 2^-53 each
    return abs(got - ref) <= n * 2.0 ** -52 * ref


@pytest.mark.parametrize("huge", [True, False], ids=["huge", "nohuge"])
@pytest.mark.parametrize("n", SIZES)
def test_guard_clean_values(n, huge):
    """The two +-3e38 elements' squares outweigh every other term of the sum by 2^50 and more, so the sizes run a second
    time without them: there the rounding of the whole summation shows."""
    if huge:
        x, sq = _case(n)
    else:
        x = _values(n, 300 + n % 89, huge=False)
        sq = (x.double() * x.double()).tolist()
    guard = _Guard()
    g = x.to(DEV)
    skip, count, sumsq, bits = guard(g)
    assert (skip, count) == (0, 0)
    ref = math.fsum(sq)
    print("n %d sumsq %.17g fsum %.17g rel %.3g" % (n, sumsq, ref, abs(sumsq - ref) / ref if ref else 0.0))
    assert _close(sumsq, ref, n), (sumsq, ref)
    if n == 0:
        assert sumsq == 0.0
    guard.out.fill_(-7)
    assert guard(g) == (0, 0, sumsq, bits), "two calls, identical bits"


_BAD = {"+inf": 0x7f800000, "-inf": 0xff800000 - (1 << 32), "qnan": 0x7fc00000, "snan": 0x7f800001}


@pytest.mark.parametrize("n", [1, 5, 257, 65537])
def test_guard_nonfinite(n):
    """+inf, -inf, a quiet NaN and the pattern 0x7f800001 at the first element, the last (a tail element when n % 4 != 0)
    and the middle one, singly and all together: exact count, skip word set, the clean elements' sum; a clean call
    on the same verdict buffer then writes [0, 0]; `also` alone sets the skip word and not the count."""
    x, sq = _case(n)
    guard = _Guard()
    clean = x.to(DEV)
    places = sorted({0, n - 1, n // 2})
    cases = [[(i, b)] for i in places for b in _BAD.values()]
    cases.append([(i, list(_BAD.values())[k % 4]) for k, i in enumerate(places)])
    if n > 4:
        cases.append([(i, b) for i, b in zip(range(n - 4, n), _BAD.values())])      # all four patterns at once
    for case in cases:
        g = clean.clone()
        gi = g.view(torch.int32)
        for i, b in case:
            gi[i] = b
        hit = {i for i, _ in case}
        assert int((~torch.isfinite(g)).sum()) == len(hit)
        skip, count, sumsq, _ = guard(g)
        assert count == len(hit) and skip != 0, (case, skip, count)
        ref = math.fsum(v for i, v in enumerate(sq) if i not in hit)
        assert _close(sumsq, ref, n) and math.isfinite(sumsq), (case, sumsq, ref)
        skip, count, sumsq, _ = guard(clean)
        assert (skip, count) == (0, 0) and _close(sumsq, math.fsum(sq), n), (case, skip, count)
    also = torch.tensor([1 << 40], dtype=torch.int64, device=DEV)
    skip, count, sumsq, _ = guard(clean, also=also)
    assert skip != 0 and count == 0 and _close(sumsq, math.fsum(sq), n)
    also.zero_()
    assert guard(clean, also=also)[:2] == (0, 0)
    empty = torch.empty(0, device=DEV)
    assert guard(empty, also=also)[:3] == (0, 0, 0.0)
    also.fill_(3)
    skip, count, sumsq, _ = guard(empty, also=also)
    assert skip != 0 and count == 0 and sumsq == 0.0


def test_guard_arguments():
    from scdhip import lib as L
    from scdhip import ops
    fn = L.lib().scd_grad_guard
    g = torch.zeros(64, device=DEV)
    ws = torch.zeros(ops.grad_guard_workspace(64), dtype=torch.uint8, device=DEV)
    out = torch.zeros(3, dtype=torch.int64, device=DEV)
    v, s, st = out.data_ptr(), out[2:].data_ptr(), ops.stream()
    assert fn(g.data_ptr(), -1, None, ws.data_ptr(), v, s, st) == ERR_ARG
    assert fn(None, 64, None, ws.data_ptr(), v, s, st) == ERR_ARG
    assert fn(g.data_ptr(), 64, None, None, v, s, st) == ERR_ARG
    assert fn(g.data_ptr(), 64, None, ws.data_ptr(), None, s, st) == ERR_ARG
    assert fn(g.data_ptr(), 64, None, ws.data_ptr(), v, None, st) == ERR_ARG
    assert fn(g[1:].data_ptr(), 63, None, ws.data_ptr(), v, s, st) == ERR_ARG      # a 4-byte-aligned view
    assert fn(g.data_ptr(), 64, None, ws.data_ptr(), v, s, st) == 0
    torch.cuda.synchronize()
    assert out.tolist() == [0, 0, 0]
    with pytest.raises(RuntimeError):
        ops.grad_guard(g[1:], ws, out[:2], out[2:])


# ------------------------------------------------------------------ the optimizers

_SHAPES = [(25, 40), (2,), (1,)]            # 1,003 elements


def _pair(kind, seed):
    from scdhip.flat import FlatAdam, FlatSGD
    g = torch.Generator().manual_seed(seed)
    p0 = [torch.randn(*s, generator=g) for s in _SHAPES]
    pt = [x.clone().requires_grad_(True) for x in p0]
    pd = [torch.nn.Parameter(x.clone().to(DEV)) for x in p0]
    if kind == "adam":
        return g, pt, pd, torch.optim.Adam(pt, lr=1e-3), FlatAdam(pd, lr=1e-3)
    kw = dict(lr=2.5e-4, momentum=0.9, weight_decay=1e-4)
    return g, pt, pd, torch.optim.SGD(pt, **kw), FlatSGD(pd, **kw)


def _set_grads(g, pt, pd, opt, poison=None):
    opt.zero_grad()
    for k, (a, b) in enumerate(zip(pt, pd)):
        gr = torch.randn(a.shape, generator=g)
        a.grad = gr.clone()
        if poison is not None and k == poison[0]:
            gr.view(-1)[poison[1]] = float("inf")
        b.grad.copy_(gr.to(DEV))


def _state(opt):
    bufs = [opt._m, opt._v] if hasattr(opt, "_m") else [opt._buf]
    return [opt.flat().data.clone()] + [b.clone() for b in bufs] + [opt._hyper.clone()]


@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_overflowed_step_is_skipped(kind):
    """One inf among 1,003 gradient elements: parameters, state buffers and the device step state stay bitwise
    unchanged, update() takes the step off the host mirror and halves S; the next clean step equals torch's from the
    same state (bound of test_adam_device_state_matches_torch / test_flat_sgd_matches_torch)."""
    from scdhip.amp import DynamicLossScale
    g, pt, pd, opt_t, opt = _pair(kind, 21)
    scaler = DynamicLossScale(init_scale=2.0 ** 16).attach(opt)
    try:
        _set_grads(g, pt, pd, opt)              # a clean step first: moments / momentum buffer are in use
        opt_t.step()
        opt.step()
        assert scaler.update(block=True) == 2.0 ** 16 and (scaler.steps, scaler.skipped) == (1, 0)
        before = _state(opt)
        _set_grads(g, pt, pd, opt, poison=(0, 517))
        opt.step()
        torch.cuda.synchronize()
        for a, b in zip(before, _state(opt)):
            assert torch.equal(a, b)
        assert opt._hyper[1].item() == 1.0 and opt._step == 2       # the mirror runs ahead until update()
        scaler.update(block=True)
        assert opt._step == 1 == int(opt._hyper[1].item())
        assert (scaler.steps, scaler.skipped, scaler.scale, scaler.last_nonfinite) == (2, 1, 2.0 ** 15, 1)
        assert opt.state_dict()["step"] == 1 and opt.state_dict()["loss_scale"]["scale"] == 2.0 ** 15
        _set_grads(g, pt, pd, opt)
        opt_t.step()                            # torch never saw the overflowed step
        opt.step()
        scaler.update(block=True)
        assert (scaler.steps, scaler.skipped, opt._step) == (3, 1, 2) and opt._hyper[1].item() == 2.0
        for a, b in zip(pt, pd):
            np.testing.assert_allclose(b.detach().cpu().numpy(), a.detach().numpy(), rtol=1e-6, atol=1e-7)
    finally:
        scaler.detach()


def test_lag_two_overflows_halve_once():
    """Two overflowing steps issued with no update() between them ran at the same S: one halving, two skipped; a
    third overflow, issued after the host heard, halves again.  A ring of depth 2 blocks on its oldest slot when a
    third step is issued before any update()."""
    from scdhip.amp import DynamicLossScale
    g, pt, pd, _, opt = _pair("adam", 22)
    scaler = DynamicLossScale(init_scale=2.0 ** 16, depth=2).attach(opt)
    try:
        p0 = opt.flat().data.clone()
        for _ in range(2):
            _set_grads(g, pt, pd, opt, poison=(1, 1))
            opt.step()
        assert scaler.steps == 0 and scaler.scale == 2.0 ** 16
        scaler.update(block=True)
        assert (scaler.scale, scaler.skipped, scaler.steps, opt._step) == (2.0 ** 15, 2, 2, 0)
        _set_grads(g, pt, pd, opt, poison=(2, 0))
        opt.step()
        scaler.update(block=True)
        assert (scaler.scale, scaler.skipped, opt._step) == (2.0 ** 14, 3, 0)
        for _ in range(3):                      # the third finds the ring of two full
            _set_grads(g, pt, pd, opt, poison=(0, 3))
            opt.step()
        assert scaler.steps == 4 and scaler.scale == 2.0 ** 13
        scaler.update(block=True)
        assert (scaler.scale, scaler.skipped, scaler.steps, opt._step) == (2.0 ** 13, 6, 6, 0)
        assert torch.equal(opt.flat().data, p0) and opt._hyper[1].item() == 0.0
    finally:
        scaler.detach()


def test_grad_norm():
    from scdhip.amp import DynamicLossScale
    g, pt, pd, _, opt = _pair("sgd", 23)
    scaler = DynamicLossScale().attach(opt)
    try:
        assert scaler.grad_norm is None
        _set_grads(g, pt, pd, opt)
        ref = torch.linalg.vector_norm(opt.flat().grad.double()).item()
        opt.step()
        scaler.update(block=True)
        assert abs(scaler.grad_norm - ref) <= 1e-12 * ref, (scaler.grad_norm, ref)
        _set_grads(g, pt, pd, opt, poison=(0, 0))          # the norm of a skipped step is still a number
        opt.step()
        scaler.update(block=True)
        assert math.isfinite(scaler.grad_norm) and scaler.grad_norm > 0 and scaler.skipped == 1
    finally:
        scaler.detach()


# ------------------------------------------------------------------ end to end

def test_res10_fp16_end_to_end():
    """centerOffsetRes10 in fp16 at B = 2, 128^2 (the oracle's hashed weights and batches): from S = 2^24 every
    overflowed step leaves the parameters bitwise unchanged, a step is applied within 15 (2^24 -> 2^10 is 14 halvings)
    at a power-of-two S >= 1024, and that step's flat gradient is the one a fresh model gives statically at that S,
    within the spread of two such static runs (0 when they agree, else four times it)."""
    import trainer.model.centerOffsetRes10 as plugin
    from oracle import centernet as O
    from oracle import targets as T
    from scdhip import ops
    from scdhip.amp import DynamicLossScale
    from scdhip.flat import FlatAdam

    entries, _ = O.model_spec(10)
    state = O.hash_weights(entries)
    x = T.batch_inputs(8, 2, 128).to(DEV)
    ys = [y.to(DEV) for y in T.batch_targets(9, 2, 32)]

    def make():
        m = plugin.model(**plugin.modelParams)
        m.load_state_dict(state)
        m = m.to(DEV).train().set_compute_dtype(torch.float16)
        return m, FlatAdam(filter(lambda p: p.requires_grad, m.parameters()))

    def backward(m, opt):
        opt.zero_grad()
        loss, _ = plugin.loss(m(x, decode=False), ys)
        loss.mean().backward()
        return opt.flat().grad

    def static_grad(S):
        ops.set_loss_scale(S)
        m, opt = make()
        return backward(m, opt).clone()

    # the premise: at the static default the gradient of this step is finite
    assert torch.isfinite(static_grad(1024.0)).all(), "one static step at S = 1024 overflows at this shape"

    m, opt = make()
    scaler = DynamicLossScale(init_scale=2.0 ** 24).attach(opt)
    try:
        applied = None
        for it in range(15):
            S = scaler.scale
            before = opt.flat().data.clone()
            grad = backward(m, opt).clone()
            opt.step()
            skipped = scaler.skipped
            scaler.update(block=True)
            if scaler.skipped == skipped:
                applied = S
                break
            assert torch.equal(opt.flat().data, before), "a skipped step moved the parameters (step %d)" % it
            assert scaler.scale == S / 2
        print("applied at step %d, S = 2^%d, %d skipped" % (it, int(math.log2(applied or 1)), scaler.skipped))
        assert applied is not None, "no step applied within 15"
        assert applied >= 1024.0 and math.frexp(applied)[0] == 0.5
        assert not torch.equal(opt.flat().data, before) and opt._step == 1 == int(opt._hyper[1].item())
        assert torch.isfinite(opt.flat().data).all() and torch.isfinite(grad).all()
        for k, b in m.named_buffers():
            assert torch.isfinite(b).all(), k
    finally:
        scaler.detach()
    a, b = static_grad(applied), static_grad(applied)
    spread = (a - b).abs().max().item()
    diff = (grad - a).abs().max().item()
    print("flat gradient, max abs: dynamic vs static %.3e, static vs static %.3e (max |g| %.3e)"
          % (diff, spread, a.abs().max().item()))
    assert diff <= 4 * spread, (diff, spread)


def test_network_factory_dynamic(tmp_path):
    """"lossScale": "dynamic" through NetworkFactory on the synthetic dataset: three iterations in fp16."""
    from configuration import defaultConfig
    from models.networkFactory import NetworkFactory
    from scdhip import ops
    from scdhip.amp import DynamicLossScale
    defaultConfig.updateConfig({"modelName": "centerOffsetRes10", "datasetName": "syntheticSCD", "trainName": "amptest",
                                "computeDtype": "fp16", "lossScale": "dynamic", "iterations": 3, "validation": 1000,
                                "snapshot": 3, "batchSize": 2, "dirTemp": str(tmp_path / "t") + "/",
                                "dirResult": str(tmp_path / "r") + "/", "currentIter": 0})
    f = NetworkFactory(True)
    try:
        assert isinstance(f.lossScaler, DynamicLossScale) and f.optimizer._scaler is f.lossScaler
        assert ops.LossScale.f16 == f.lossScaler.scale
        f.beginTraining(0)
        s = f.lossScaler
        assert s.steps == 3 and not s._pending and ops.LossScale.f16 == s.scale
        assert f.optimizer._step == 3 - s.skipped == int(f.optimizer._hyper[1].item())
        losses = np.loadtxt(str(tmp_path / "r" / "losses.amptest.3.txt"), delimiter=",", ndmin=2)
        assert losses.shape == (3, 5) and np.isfinite(losses).all()
        for p in f.model.parameters():
            assert torch.isfinite(p).all()
    finally:
        f.lossScaler.detach()
