"""CPU tests of the stacked-hourglass CenterNet: the module tree against the reference's state-dict layout
(tests/golden/hourglass.npz, written by make_golden_hourglass.py from the real reference), the Residual block's
`skip` / `downsample`, the terminal initialiser, the plugin surface, and the argument checks that run before the GPU
is needed."""
import importlib

import pytest
import torch


def _entries(g, prefix=""):
    keys = [str(k) for k in g[prefix + "keys"]]
    shapes = [tuple(int(v) for v in str(s).split(",")) if str(s) else () for s in g[prefix + "shapes"]]
    return keys, shapes


def test_default_model_has_the_reference_state_dict(golden):
    from models.centerNetOffseth import CenterNetHourglass
    keys, shapes = _entries(golden("hourglass"))
    sd = CenterNetHourglass().state_dict()
    assert list(sd.keys()) == keys
    assert [tuple(v.shape) for v in sd.values()] == shapes
    assert len(keys) > 400


@pytest.mark.parametrize("case,kw", [
    ("A", dict(hourglassIters=2, dimensions=[64, 64, 128], modules=[1, 1, 2], predictionConvDim=128)),
    ("B", dict(hourglassIters=2, dimensions=[64, 128, 192], modules=[2, 1, 2], predictionConvDim=256))])
def test_two_level_nets_have_the_fixture_layout(golden, case, kw):
    from models.centerNetOffseth import CenterNetHourglass
    keys, shapes = _entries(golden("hourglass"), case + "|")
    sd = CenterNetHourglass(**kw).state_dict()
    assert list(sd.keys()) == keys
    assert [tuple(v.shape) for v in sd.values()] == shapes


def test_heatmap_tail_bias_is_initialised():
    from models.centerNetOffseth import CenterNetHourglass
    m = CenterNetHourglass(hourglassIters=1, dimensions=[64, 64], modules=[1, 1], predictionConvDim=64)
    assert torch.equal(m.heatmap[0][1].bias.data, torch.full((1,), -2.19))
    assert not torch.equal(m.regr[0][1].bias.data, torch.full((4,), -2.19))


def test_residual_skip_and_downsample():
    from models.backbones.residuals import Residual, residual3x3
    same = Residual(3, 64, 64)
    assert [n for n, _ in same.named_children()] == ["conv1", "bn1", "relu1", "conv2", "bn2", "skip", "relu"]
    assert not [k for k in same.state_dict() if k.startswith("skip")]
    assert same.downsample is None
    assert residual3x3(64).downsample is None
    for blk in (Residual(3, 64, 128), Residual(3, 64, 64, stride=2)):
        keys = list(blk.state_dict())
        assert "skip.0.weight" in keys and "skip.1.weight" in keys and "skip.1.running_mean" in keys
        assert not [k for k in keys if k.startswith("downsample")]
        conv, bn = blk.downsample
        assert conv is blk.skip[0] and bn is blk.skip[1]
    assert Residual(3, 64, 64, stride=2).conv1.stride == (2, 2)


def test_more_than_one_stack_is_refused():
    from models.backbones.stackHourglass import StackHourglass
    with pytest.raises(NotImplementedError):
        StackHourglass(2, 2, [64, 64, 128], [1, 1, 2], 1)


def test_other_layer_kinds_are_refused_before_any_launch():
    from models.backbones.hourglass import Hourglass
    from models.backbones.pooling import UpsampleType, unpoolingLayer
    x = torch.zeros(1, 4, 4, 64)
    with pytest.raises(NotImplementedError):            # the default MaxPool2d down-sampling layer
        Hourglass(1, [64, 64], [1, 1])(x)
    no_pool = lambda s: torch.nn.Sequential()   # noqa: E731
    with pytest.raises(NotImplementedError):
        Hourglass(1, [64, 64], [1, 1], layersDownsampling=no_pool,
                  layersUpsampling=lambda s: unpoolingLayer(s, UpsampleType.Bilinear))(x)
    with pytest.raises(NotImplementedError):
        Hourglass(1, [64, 64], [1, 1], layersDownsampling=no_pool, layersMerge=lambda d: torch.nn.Identity())(x)


def test_cpu_input_and_geometry_are_refused():
    from models.centerNetOffseth import CenterNetHourglass
    m = CenterNetHourglass(hourglassIters=2, dimensions=[64, 64, 128], modules=[1, 1, 2], predictionConvDim=128)
    with pytest.raises(RuntimeError, match="MI355X only"):
        m(torch.zeros(1, 1, 64, 64))


def test_plugin_surface():
    plugin = importlib.import_module("trainer.model.centerOffsetHourglass")
    for attr in ("model", "loss", "modelParams", "evaluation", "expression"):
        assert hasattr(plugin, attr)
    from models.centerNetOffseth import CenterNetHourglass
    res10 = importlib.import_module("trainer.model.centerOffsetRes10")
    assert plugin.model is CenterNetHourglass and plugin.modelParams == {}
    assert plugin.evaluation is res10.evaluation and plugin.expression is res10.expression
    assert type(plugin.loss) is type(res10.loss)
    assert (plugin.loss.regressionWeight, plugin.loss.offsetWeight) == (res10.loss.regressionWeight,
                                                                        res10.loss.offsetWeight)


def test_trace_and_slide_refuse_the_hourglass_with_a_message(tmp_path):
    """TorchScript export and slide analysis are not built for this model: both tools say so and exit before they
    load anything, and fold refuses it as every non-ResNet model."""
    import importlib.util
    import os
    import slide
    from models.centerNetOffseth import CenterNetHourglass
    # (by path: `trace` is also a standard-library module)
    spec = importlib.util.spec_from_file_location("scd_trace_tool", os.path.join(os.path.dirname(slide.__file__), "trace.py"))
    trace = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(trace)
    from scdhip import export, infer
    args = trace.parseArguments([str(tmp_path / "o.pt"), "-a", "centerOffsetHourglass", "-m", str(tmp_path / "none.pth"),
                                 "-s", "1 1 128 128"])
    with pytest.raises(SystemExit) as e:
        trace.begin(args)
    assert e.value.code == 1
    with pytest.raises(SystemExit) as e:
        slide.load_wrapper("centerOffsetHourglass", str(tmp_path / "none.pth"), True, False)
    assert "not a CenterNet ResNet" in str(e.value.code)
    with pytest.raises(NotImplementedError, match="not a CenterNet ResNet"):
        export._plugin_model("centerOffsetHourglass")
    assert export.unsupported("centerOffsetRes10", export._plugin_model("centerOffsetRes10")) is None
    with pytest.raises(NotImplementedError):
        infer.fold(CenterNetHourglass(hourglassIters=1, dimensions=[64, 64], modules=[1, 1], predictionConvDim=64))


def test_upsample_add_checks_shapes_before_the_gpu():
    from scdhip import ops
    up, low = torch.zeros(2, 6, 10, 8), torch.zeros(2, 3, 5, 8)
    for bad_up, bad_low in ((torch.zeros(2, 6, 10, 16), low), (torch.zeros(2, 6, 9, 8), low),
                            (up, torch.zeros(2, 3, 5, 8, dtype=torch.bfloat16)),
                            (up.permute(0, 2, 1, 3), torch.zeros(2, 5, 3, 8)), (torch.zeros(6, 10, 8), low)):
        with pytest.raises(ValueError) as e:
            ops.upsample_add(bad_up, bad_low)
        assert str(tuple(bad_up.shape)) in str(e.value) and str(tuple(bad_low.shape)) in str(e.value)
    with pytest.raises(ValueError):
        ops.upsample_add_bwd(torch.zeros(2, 5, 10, 8))
    with pytest.raises(RuntimeError, match="MI355X only"):     # well-formed CPU tensors: the usual no-fallback error
        ops.upsample_add(up, low)


def test_new_entry_points_are_declared_everywhere():
    """Header, ctypes table and the fp16 build's list name both merge entry points (test_host_cpu.py holds the three
    lists to each other; this pins that the new names are on them)."""
    import os
    import re
    import scdhip.lib as L
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(repo, "include", "scdhip.h")).read()
    common = open(os.path.join(repo, "scd-resnet_amd", "csrc", "scd_common.h")).read()
    for name in ("scd_upsample2x_add", "scd_upsample2x_add_bwd"):
        assert re.search(r"^int %s\(" % name, header, re.M)
        assert name in L.SIGNATURES
        assert "X(%s)" % name in common
        assert hasattr(L.lib().dll, name) and hasattr(L.lib().dll, name + "__f16")
