"""Modulated deformable conv (DCNv2), the parts that need no GPU: the float64 restatement (tests/dcn_ref.py) held to
itself -- two independent formulations, the plain-conv identity, integer offsets against shifted copies -- and the
module, plugin and entry-point surfaces.

Bound of the restatement checks: 2^-40 x the sum of absolute terms.  A result is a sum of at most 9C <= 2^13 float64
terms, each a product of a few factors, summed in some order: 2^13 roundings of 2^-53 each on the absolute sum.
"""
import importlib
import math
import os
import re

import pytest
import torch
import torch.nn.functional as F

import dcn_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "scd-resnet_amd", "csrc")
EPS = 2.0 ** -40


def _case(seed, N, H, W, C, G, Co, grad):
    g = torch.Generator().manual_seed(seed)
    off = R.draw_offsets(g, N, H, W, G, grad)
    x = torch.randn(N, H, W, C, dtype=torch.float64, generator=g)
    m = torch.rand(N, H, W, 9 * G, dtype=torch.float64, generator=g)
    w = torch.randn(Co, C, 3, 3, dtype=torch.float64, generator=g) / math.sqrt(9 * C)
    b = torch.randn(Co, dtype=torch.float64, generator=g)
    dy = torch.randn(N, H, W, Co, dtype=torch.float64, generator=g)
    return x, off, m, w, b, dy


@pytest.mark.parametrize("shape", [(2, 5, 7, 16, 2), (3, 33, 65, 64, 1)])
def test_offset_draw_covers_outside_partial_and_inside_samples(shape):
    N, H, W, C, G = shape
    for seed in (1, 2, 3):
        off = R.draw_offsets(torch.Generator().manual_seed(seed), N, H, W, G, False)
        assert (off * 8 == torch.round(off * 8)).all() and (off.bfloat16().double() == off).all()
        none, part, full = R.classify(off, H, W, G)
        print(shape, seed, "none %.3f partial %.3f all %.3f" % (none, part, full))
        if (H, W) == (5, 7):
            assert none >= 0.10 and part >= 0.10 and full >= 0.40
        else:
            assert full >= 0.50
    # the gradient draw has no sample on a kink of the bilinear map
    off = R.draw_offsets(torch.Generator().manual_seed(1), N, H, W, G, True)
    assert ((off != torch.floor(off)) | (off.abs() > 3)).all()


@pytest.mark.parametrize("shape", [(2, 5, 7, 16, 2), (3, 33, 65, 64, 1)])
def test_the_two_restatements_agree(shape):
    """Index gather + einsum against grid_sample + nine 1x1 convs: outputs and all five gradients."""
    N, H, W, C, G = shape
    x, off, m, w, b, dy = _case(5, N, H, W, C, G, 24, True)
    res = {}
    for form in ("gather", "grid"):
        leaves = [t.clone().requires_grad_() for t in (x, off, m, w, b)]
        y = R.dcn(*leaves, G, form)
        res[form] = [y.detach()] + list(torch.autograd.grad(y, leaves, dy))
    # sums of absolute terms: the same computation on absolute values (corner weights are >= 0); the offset
    # gradient's terms carry the signed weight derivatives, written out in dcn_ref.abs_terms_dom
    la = [t.abs().requires_grad_() for t in (x, m, w, b)]
    ya = R.dcn(la[0], off, la[1], la[2], la[3], G, "gather")
    ga = torch.autograd.grad(ya, la, dy.abs())
    dcols_abs = torch.einsum("nhwo,ock->nhwkc", dy.abs(), w.abs().reshape(24, C, 9))
    aoff = R.abs_terms_dom(dcols_abs, x, off, m, G)[..., :18 * G]
    bounds = [ya.detach(), ga[0], aoff, ga[1], ga[2], ga[3]]
    for name, a, c, s in zip(("y", "dx", "doff", "dmask", "dweight", "dbias"), res["gather"], res["grid"], bounds):
        err = (a - c).abs()
        print("%-8s max |diff| %.3e  max ratio to the absolute sum %.3e" % (
            name, err.max().item(), (err / s.clamp_min(1e-300)).max().item()))
        assert (err <= EPS * s).all(), name
        assert a.abs().max() > 0


def test_zero_offsets_and_unit_masks_are_a_plain_conv():
    x, off, m, w, b, _ = _case(6, 2, 5, 7, 16, 2, 24, False)
    y = R.dcn(x, torch.zeros_like(off), torch.ones_like(m), w, b, 2)
    ref = F.conv2d(x.permute(0, 3, 1, 2), w, b, padding=1).permute(0, 2, 3, 1)
    s = F.conv2d(x.abs().permute(0, 3, 1, 2), w.abs(), b.abs(), padding=1).permute(0, 2, 3, 1)
    assert ((y - ref).abs() <= EPS * s).all()


def test_integer_offsets_are_shifted_zero_padded_copies():
    """Per-tap integer offsets, the same at every pixel: column k is x shifted by (i - 1 + dh_k, j - 1 + dw_k) into a
    zero frame, so the conv is a sum of nine 1x1 convs over explicitly shifted copies."""
    N, H, W, C, G, Co = 2, 5, 7, 8, 1, 12
    x, _, m, w, b, _ = _case(7, N, H, W, C, G, Co, False)
    g = torch.Generator().manual_seed(8)
    d = torch.randint(-3, 4, (9, 2), generator=g)
    off = d.double().view(1, 1, 1, 18).expand(N, H, W, 18).contiguous()
    y = R.dcn(x, off, m, w, b, G)
    big = F.pad(x, (0, 0, 8, 8, 8, 8))                 # zero frame of 8 pixels: every shift stays inside it
    ref = b.view(1, 1, 1, Co).expand(N, H, W, Co).clone()
    s = b.abs().view(1, 1, 1, Co).expand(N, H, W, Co).clone()
    for k in range(9):
        i, j = divmod(k, 3)
        sh, sw = i - 1 + int(d[k, 0]), j - 1 + int(d[k, 1])
        col = big[:, 8 + sh:8 + sh + H, 8 + sw:8 + sw + W] * m[..., k:k + 1]
        ref += torch.einsum("nhwc,oc->nhwo", col, w[:, :, i, j])
        s += torch.einsum("nhwc,oc->nhwo", col.abs(), w[:, :, i, j].abs())
    assert ((y - ref).abs() <= EPS * s).all()


# ---------------------------------------------------------------------------------------------- surfaces

def test_module_surface():
    from models.backbones.deformable import DCN, DCNv2, dcn_v2_conv
    torch.manual_seed(3)
    d = DCN(64, 32, 3, 1, 1, deformable_groups=2)
    sd = d.state_dict()
    assert list(sd) == ["weight", "bias", "conv_offset_mask.weight", "conv_offset_mask.bias"]
    assert sd["weight"].shape == (32, 64, 3, 3) and sd["bias"].shape == (32,)
    assert sd["conv_offset_mask.weight"].shape == (54, 64, 3, 3) and sd["conv_offset_mask.bias"].shape == (54,)
    bound = 1 / math.sqrt(9 * 64)
    assert sd["weight"].abs().max() <= bound and sd["weight"].abs().max() > 0.9 * bound
    assert abs(sd["weight"].mean().item()) < 0.05 * bound
    assert not sd["bias"].any() and not sd["conv_offset_mask.weight"].any() and not sd["conv_offset_mask.bias"].any()
    v2 = DCNv2(16, 8, (3, 3), (1, 1), (1, 1), dilation=1, deformable_groups=1)
    assert list(v2.state_dict()) == ["weight", "bias"] and v2.kernel_size == (3, 3) and v2.deformable_groups == 1
    for args in ((16, 8, 1, 1, 0), (16, 8, 3, 2, 1), (16, 8, 3, 1, 0), (16, 8, 5, 1, 2)):
        with pytest.raises(NotImplementedError):
            DCN(*args)
    with pytest.raises(NotImplementedError):
        DCNv2(16, 8, 3, 1, 1, dilation=2)
    with pytest.raises(RuntimeError, match="MI355X only"):
        d(torch.zeros(1, 4, 4, 64))
    with pytest.raises(RuntimeError, match="MI355X only"):
        v2(torch.zeros(1, 4, 4, 16), torch.zeros(1, 4, 4, 18), torch.ones(1, 4, 4, 9))
    with pytest.raises(NotImplementedError):
        dcn_v2_conv(torch.zeros(1, 4, 4, 16), torch.zeros(1, 4, 4, 18), torch.ones(1, 4, 4, 9), v2.weight, v2.bias,
                    2, 1, 1, 1)


def test_ops_check_arguments_before_the_library_is_called():
    from scdhip import ops
    x, om = torch.zeros(1, 4, 4, 16), torch.zeros(1, 4, 4, 32)
    with pytest.raises(RuntimeError, match="MI355X only"):
        ops.dcn_cols(x.bfloat16(), om.bfloat16())
    with pytest.raises(RuntimeError, match="MI355X only"):
        ops.dcn_cols_bwd(torch.zeros(1, 4, 4, 144), x, torch.zeros(1, 4, 4, 28))
    for bad in (lambda: ops.dcn_cols(x, om.bfloat16()),                      # dtypes differ
                lambda: ops.dcn_cols(x, torch.zeros(1, 4, 5, 32)),           # other pixels
                lambda: ops.dcn_cols(x, torch.zeros(1, 4, 4, 24)),           # P < 27G
                lambda: ops.dcn_cols(x, torch.zeros(1, 4, 4, 30)),           # P not in whole chunks
                lambda: ops.dcn_cols(x, torch.zeros(1, 4, 4, 56), G=8),      # 2 channels per group
                lambda: ops.dcn_cols(x.double(), om.double()),
                lambda: ops.dcn_cols_bwd(torch.zeros(1, 4, 4, 16), x, om)):  # dcols is not (N,H,W,9C)
        with pytest.raises(ValueError):
            bad()


def test_entry_points_are_on_all_three_lists():
    import scdhip.lib as L
    header = open(os.path.join(REPO, "include", "scdhip.h")).read()
    common = open(os.path.join(CSRC, "scd_common.h")).read()
    src = open(os.path.join(CSRC, "deform.hip")).read()
    mk = open(os.path.join(CSRC, "Makefile")).read()
    for name in ("scd_dcn_cols", "scd_dcn_cols_bwd"):
        assert re.search(r"^int %s\(" % name, header, re.M)
        assert name in L.SIGNATURES and hasattr(L.lib().dll, name) and hasattr(L.lib().dll, name + "__f16")
        assert "X(%s)" % name in common
        assert len(re.findall(r"SCD_F16_FWD\(%s," % name, src)) == 1
    assert len(L.SIGNATURES["scd_dcn_cols"][1]) == 12 and len(L.SIGNATURES["scd_dcn_cols_bwd"][1]) == 14
    assert re.search(r"^SRCS :=.*\bdeform\.hip\b", mk, re.M) and re.search(r"^F16SRCS :=.*\bdeform\.hip\b", mk, re.M)


def test_plugin_surface():
    from models.backbones.deformable import DCN
    plugin = importlib.import_module("trainer.model.centerOffsetRes18dcn")
    base = importlib.import_module("trainer.model.centerOffsetRes18")
    for name in ("model", "loss", "modelParams", "evaluation", "expression"):
        assert hasattr(plugin, name)
    assert plugin.model is base.model and plugin.evaluation is base.evaluation
    assert plugin.expression is base.expression
    assert plugin.modelParams == dict(base.modelParams, deformable=True)
    assert (plugin.loss.regressionWeight, plugin.loss.offsetWeight) == (base.loss.regressionWeight,
                                                                        base.loss.offsetWeight)
    m = plugin.model(**plugin.modelParams)
    assert m.deformable and len(m.deformLayers) == 3 and len(m.deconvolutionLayers) == 9
    cin = 512
    for i, stage in enumerate(m.deformLayers):
        assert isinstance(stage[0], DCN) and isinstance(stage[1], torch.nn.BatchNorm2d)
        assert isinstance(stage[2], torch.nn.ReLU) and len(stage) == 3
        assert (stage[0].in_channels, stage[0].out_channels) == (cin, 256)
        dc = m.deconvolutionLayers[3 * i]
        assert isinstance(dc, torch.nn.ConvTranspose2d) and (dc.in_channels, dc.out_channels) == (256, 256)
        cin = 256
    keys = [k for k in m.state_dict() if k.startswith("deformLayers.")]
    assert len(keys) == 3 * 9 and "deformLayers.2.0.conv_offset_mask.bias" in keys


def test_plain_model_is_unchanged():
    from models.centerNetOffset import CenterNetResidual
    from oracle import centernet as O
    entries, _ = O.model_spec(18)
    want = O.hash_weights(entries)
    m = CenterNetResidual(18)
    sd = m.state_dict()
    assert sorted(sd) == sorted(want) and all(sd[k].shape == want[k].shape for k in want)
    assert not any(k.startswith("deformLayers") for k in sd) and not hasattr(m, "deformLayers")
    assert m.deformable is False and m.deconvolutionLayers[0].in_channels == 512
    m.load_state_dict(want)
