"""Dynamic fp16 loss scaling, host side (scdhip/amp.py): the scale rule against torch.amp.GradScaler, its bounds and
its lag rule, the construction and configuration checks, the checkpoint keys and the declarations of the guard kernel's
entry points.  No GPU."""
import os
import random

import pytest
import torch

from conftest import REPO


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


def _found_sequence(seed, n, p):
    rng = random.Random(seed)
    return [rng.random() < p for _ in range(n)]


@pytest.mark.parametrize("seed,p", [(1, 0.2), (2, 0.05), (3, 0.5)])
def test_rule_matches_torch_gradscaler(seed, p):
    """200 steps of a seeded found / clean sequence through torch.amp.GradScaler (a one-element parameter whose
    gradient is inf on the found steps) and through amp.scale_rule, every step run at the current scale: equal scales
    after every step.  torch has no bounds, so they are set out of reach here."""
    from scdhip.amp import scale_rule
    w = torch.nn.Parameter(torch.ones(1))
    opt = torch.optim.SGD([w], lr=0.0)
    scaler = torch.amp.GradScaler("cpu", init_scale=2.0 ** 10, growth_interval=3)
    S, tracker = 2.0 ** 10, 0
    for step, found in enumerate(_found_sequence(seed, 200, p)):
        opt.zero_grad()
        scaler.scale((w * 1.0).sum()).backward()
        if found:
            w.grad.fill_(float("inf"))
        scaler.step(opt)
        scaler.update()
        S, tracker = scale_rule(S, tracker, found, S, growth_interval=3, min_scale=2.0 ** -300, max_scale=2.0 ** 300)
        assert S == scaler.get_scale(), (step, S, scaler.get_scale())
        assert tracker == scaler._get_growth_tracker(), step


def test_rule_bounds():
    """min_scale and max_scale by hand: the scale stops at either and the tracker still resets."""
    from scdhip.amp import scale_rule
    S, tracker, seen = 4.0, 0, []
    for _ in range(4):
        S, tracker = scale_rule(S, tracker, True, S, min_scale=1.0)
        seen.append(S)
    assert seen == [2.0, 1.0, 1.0, 1.0] and tracker == 0
    S, tracker, seen = 2.0 ** 22, 0, []
    for _ in range(8):
        S, tracker = scale_rule(S, tracker, False, S, growth_interval=2, max_scale=2.0 ** 24)
        seen.append((S, tracker))
    assert seen == [(2.0 ** 22, 1), (2.0 ** 23, 0), (2.0 ** 23, 1), (2.0 ** 24, 0), (2.0 ** 24, 1), (2.0 ** 24, 0),
                    (2.0 ** 24, 1), (2.0 ** 24, 0)]
    # a found step in between takes the growth run back to its start
    S, tracker = scale_rule(8.0, 1, True, 8.0, growth_interval=2)
    assert (S, tracker) == (4.0, 0)
    assert scale_rule(S, tracker, False, S, growth_interval=2) == (4.0, 1)


def test_rule_lag():
    """Two found verdicts tagged with the same scale halve it once (the second was issued before the host heard of the
    first); a third tagged with the new scale halves it again.  Either way the tracker restarts."""
    from scdhip.amp import scale_rule
    S, tracker = scale_rule(1024.0, 5, True, 1024.0)
    assert (S, tracker) == (512.0, 0)
    S, tracker = scale_rule(S, 3, True, 1024.0)
    assert (S, tracker) == (512.0, 0)
    S, tracker = scale_rule(S, tracker, True, 512.0)
    assert (S, tracker) == (256.0, 0)


@pytest.mark.parametrize("kw", [dict(growth_factor=3.0), dict(backoff_factor=0.3), dict(init_scale=1000),
                                dict(min_scale=3.0, init_scale=4.0), dict(max_scale=1e6), dict(growth_interval=0),
                                dict(min_scale=8.0, init_scale=4.0), dict(init_scale=2.0 ** 25)])
def test_construction_value_errors(kw):
    from scdhip.amp import DynamicLossScale
    with pytest.raises(ValueError):
        DynamicLossScale(**kw)


def test_construction_defaults():
    from scdhip.amp import DynamicLossScale
    s = DynamicLossScale()
    assert s.scale == 65536.0 and s.grad_norm is None and s.skipped == 0 and s.steps == 0
    assert (s.growth_factor, s.backoff_factor, s.growth_interval, s.min_scale, s.max_scale, s.depth) == \
        (2.0, 0.5, 2000, 1.0, 2.0 ** 24, 8)


@pytest.mark.parametrize("update", [{"lossScale": "dynamic", "computeDtype": "bf16"},
                                    {"lossScale": "dynamic", "computeDtype": "fp32"},
                                    {"lossScale": "dynamic", "computeDtype": "fp16", "stepGraph": True},
                                    {"lossScale": "adaptive", "computeDtype": "fp16"}])
def test_network_factory_value_errors(update):
    from configuration import defaultConfig
    from models.networkFactory import NetworkFactory
    defaultConfig.updateConfig(dict({"modelName": "centerOffsetRes10", "datasetName": "syntheticSCD"}, **update))
    with pytest.raises(ValueError, match="lossScale"):
        NetworkFactory(True)


def test_config_key():
    from configuration import Configuration
    c = Configuration()
    assert c.lossScale == "static"
    c.updateConfig({"lossScale": "dynamic"})
    assert c.lossScale == "dynamic"


def test_set_loss_scale_wants_a_power_of_two():
    from scdhip import ops
    old = ops.LossScale.f16
    assert ops.set_loss_scale(4096.0) == old and ops.LossScale.f16 == 4096.0
    assert ops.loss_scale(torch.float16) == 4096.0 and ops.loss_scale(torch.bfloat16) == 1.0
    for bad in (1000.0, 0.0, -2.0, float("inf")):
        with pytest.raises(ValueError):
            ops.set_loss_scale(bad)
    assert ops.LossScale.f16 == 4096.0


@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_checkpoint_keys(kind):
    """With a scaler attached the optimizer's state_dict carries "loss_scale" and load_state_dict restores it; without
    one the state dict is what it was.  attach moves the process-wide scale, detach puts the static one back."""
    from scdhip import ops
    from scdhip.amp import DynamicLossScale
    from scdhip.flat import FlatAdam, FlatSGD

    def make():
        p = [torch.nn.Parameter(torch.ones(3))]
        return FlatAdam(p) if kind == "adam" else FlatSGD(p, lr=0.1, momentum=0.9)

    static = ops.LossScale.f16
    plain = make().state_dict()
    assert "loss_scale" not in plain
    assert sorted(plain) == (["exp_avg", "exp_avg_sq", "param_groups", "step"] if kind == "adam"
                             else ["momentum_buffer", "param_groups", "step"])
    opt = make()
    scaler = DynamicLossScale(init_scale=2.0 ** 12).attach(opt)
    assert ops.LossScale.f16 == 2.0 ** 12
    with pytest.raises(RuntimeError):
        DynamicLossScale().attach(opt)
    scaler._scale, scaler._tracker, scaler.skipped, scaler.steps = 2.0 ** 9, 7, 3, 40
    sd = opt.state_dict()
    assert sd["loss_scale"] == {"scale": 512.0, "tracker": 7, "skipped": 3, "steps": 40}
    assert sorted(k for k in sd if k != "loss_scale") == sorted(plain)
    scaler.detach()
    assert ops.LossScale.f16 == static and opt._scaler is None
    opt2 = make()
    s2 = DynamicLossScale().attach(opt2)
    opt2.load_state_dict(sd)
    assert s2.state_dict() == sd["loss_scale"] and s2.scale == 512.0 and ops.LossScale.f16 == 512.0
    opt2.load_state_dict(plain)                 # a state saved without a scaler leaves the scaler as it is
    assert s2.scale == 512.0
    with pytest.raises(ValueError):
        s2.load_state_dict({"scale": 1000.0, "tracker": 0, "skipped": 0, "steps": 0})
    s2.detach()
    assert ops.LossScale.f16 == static
    with pytest.raises(TypeError):
        DynamicLossScale().attach(torch.optim.SGD([torch.nn.Parameter(torch.ones(1))], lr=0.1))


def test_guard_entry_points_declared_everywhere():
    from scdhip import lib as L
    header = open(os.path.join(REPO, "include", "scdhip.h")).read()
    dll = L.lib().dll
    for name in ("scd_grad_guard_workspace", "scd_grad_guard"):
        assert name + "(" in header, name
        assert name in L.SIGNATURES, name
        assert hasattr(dll, name), name
    # the workspace query is host code: one fp64 partial and one count per workgroup, whatever the length
    nbytes = L.lib().scd_grad_guard_workspace(10 ** 7)
    assert nbytes > 0 and nbytes % 16 == 0 and nbytes == L.lib().scd_grad_guard_workspace(0)
