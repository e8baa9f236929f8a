"""Folded-BatchNorm inference, host side (scdhip/infer.py): the fold arithmetic against PyTorch's eval-mode BatchNorm in
float64, and the refusal of models the folded path does not cover."""
import pytest
import torch
import torch.nn.functional as F


def _bn(C, g):
    """BatchNorm2d with random fp32 tensors: negative gammas, variances down to 1e-3."""
    bn = torch.nn.BatchNorm2d(C)
    with torch.no_grad():
        bn.weight.copy_(torch.randn(C, generator=g))
        bn.bias.copy_(torch.randn(C, generator=g))
        bn.running_mean.copy_(torch.randn(C, generator=g))
        bn.running_var.copy_(torch.rand(C, generator=g) * 2.0 + 1e-3)
        bn.running_var[::5] = 1e-3
    assert (bn.weight < 0).any() and bn.running_var.min().item() == pytest.approx(1e-3)
    return bn.eval()


def _bn64(h, bn):
    return F.batch_norm(h, bn.running_mean.double(), bn.running_var.double(), bn.weight.double(), bn.bias.double(),
                        False, 0.0, bn.eps)


def _check(got, ref):
    # the only error is the fp32 rounding of w' and b'
    assert (got - ref).abs().max().item() <= 1e-5 * ref.abs().max().item()


@pytest.mark.parametrize("bias", [False, True])
def test_fold_conv_bn_matches_eval_batchnorm(bias):
    from scdhip.infer import fold_conv_bn
    g = torch.Generator().manual_seed(7)
    Ci, Co = 12, 20
    x = torch.randn(2, Ci, 9, 11, generator=g, dtype=torch.float64)
    w = torch.randn(Co, Ci, 3, 3, generator=g) / (Ci * 9) ** 0.5
    b = torch.randn(Co, generator=g) if bias else None
    bn = _bn(Co, g)
    wf, bf = fold_conv_bn(w, bn, conv_bias=b)
    assert wf.dtype == torch.float32 and bf.dtype == torch.float32 and wf.shape == w.shape and bf.shape == (Co,)
    ref = _bn64(F.conv2d(x, w.double(), None if b is None else b.double(), stride=2, padding=1), bn)
    got = F.conv2d(x, wf.double(), bf.double(), stride=2, padding=1)
    _check(got, ref)


def test_fold_conv_bn_transposed():
    from scdhip.infer import fold_conv_bn
    g = torch.Generator().manual_seed(8)
    Ci, Co = 16, 10
    x = torch.randn(2, Ci, 5, 6, generator=g, dtype=torch.float64)
    w = torch.randn(Ci, Co, 4, 4, generator=g) / (Ci * 4) ** 0.5       # ConvTranspose2d: (in, out, kh, kw)
    bn = _bn(Co, g)
    wf, bf = fold_conv_bn(w, bn, transposed=True)
    assert wf.dtype == torch.float32 and wf.shape == w.shape and bf.shape == (Co,)
    ref = _bn64(F.conv_transpose2d(x, w.double(), stride=2, padding=1), bn)
    got = F.conv_transpose2d(x, wf.double(), bf.double(), stride=2, padding=1)
    _check(got, ref)


def test_fold_refuses_the_corner_pool_model():
    """Construction only: the refusal comes before any operand is packed, so no GPU is needed."""
    import trainer.model.cornerNetCPool as plugin
    from scdhip.infer import fold
    model = plugin.model(**plugin.modelParams)
    with pytest.raises(NotImplementedError, match="Pool"):
        fold(model)
