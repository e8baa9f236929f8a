"""One residual block's training forward and backward (and eval forward) through the model's own modules, in the fp32
compute dtype, against float64 torch autograd on the CPU.

This sits between the per-kernel tests (exact / float64, tests/test_kernels_gpu.py, tests/test_bn_gpu.py) and the
whole-model goldens, whose bf16 tolerances (5e-2 .. 0.15 on backbone gradients) cannot see one reordered launch or one
dropped fused sum inside a block.

Bound: the same float64 graph is evaluated once more in torch fp32 on the CPU; per tensor the library may be 8 times as
far from float64 as that run (error = max |difference| / max |float64 value|).  Two fp32 evaluations with different
summation orders sit at the same order of distance from float64, not the same distance: that is the factor 8.  No
element is left out: the generator seed of each group is chosen so that in the float64 run every pre-ReLU value (inner
BN outputs and the join sum) has magnitude >= 1e-5, far above fp32 rounding at these magnitudes, so no ReLU flips.

Measured on MI355X over the 46 compared tensors: torch fp32's own error 5e-8 .. 7e-7, the library's 1e-7 .. 1e-6, the
largest ratio 3.09 (basic64-128s2, output), the eval forwards 2.60 and 1.19.
"""
import copy
import functools

import pytest
import torch
import torch.nn.functional as F

from test_infer_gpu import _group, _ref_block, _seed

pytestmark = pytest.mark.gpu
DEV = "cuda"
FACTOR = 8.0
RELU_MARGIN = 1e-5
# group -> generator seed under which the float64 run keeps every pre-ReLU value at least RELU_MARGIN from zero
SEEDS = {"basic64": 0, "basic64-128s2": 0, "bottleneck256": 0, "bottleneck256-512s2": 0}


def _train_ref(blk, x, dout, dtype):
    """The block in batch-statistics mode as plain torch autograd in `dtype` on the CPU: ({name: tensor} of the output,
    dx and every parameter gradient, [pre-ReLU tensors])."""
    P = {n: p.detach().to(dtype).requires_grad_() for n, p in blk.named_parameters()}
    x = x.detach().to(dtype).requires_grad_()         # (detach: a new leaf, also where .to() is the identity)

    def bn(h, mod, name):
        return F.batch_norm(h, None, None, P[name + ".weight"], P[name + ".bias"], True, 0.0, mod.eps)

    names = [n for n in ("1", "2", "3") if hasattr(blk, "conv" + n)]
    pre, h = [], x
    for n in names:
        conv = getattr(blk, "conv" + n)
        h = bn(F.conv2d(h, P["conv%s.weight" % n], stride=conv.stride, padding=conv.padding), getattr(blk, "bn" + n),
               "bn" + n)
        if n != names[-1]:
            pre.append(h)
            h = F.relu(h)
    idn = x
    if blk.downsample is not None:
        idn = bn(F.conv2d(x, P["downsample.0.weight"], stride=blk.downsample[0].stride), blk.downsample[1],
                 "downsample.1")
    pre.append(h + idn)
    out = F.relu(pre[-1])
    out.backward(dout.to(dtype))
    res = {"out": out.detach(), "dx": x.grad}
    res.update({n: p.grad for n, p in P.items()})
    return res, [t.detach() for t in pre]


@functools.lru_cache(maxsize=None)
def _case(name):
    """(block, x, dout) of a group, NCHW fp32 on the CPU, from the group's seed."""
    g = torch.Generator().manual_seed(SEEDS[name])
    blk, Ci, S = _group(name)
    _seed(blk, g)
    x = torch.randn(2, Ci, S, S, generator=g)
    with torch.no_grad():
        shape = _ref_block(blk, x).shape
    return blk, x, torch.randn(shape, generator=g)


def _err(a, ref):
    return (a.double().cpu() - ref).abs().max().item() / ref.abs().max().item()


def _check(name, got, ref64, ref32):
    """Every tensor of ref64 within FACTOR times torch fp32's own distance from float64; prints the ratios."""
    assert got.keys() == ref64.keys()
    bad = []
    for k, r in ref64.items():
        assert got[k].shape == r.shape and torch.isfinite(got[k]).all(), k
        e, e32 = _err(got[k], r), _err(ref32[k], r)
        assert e32 > 0.0, k
        print("%-20s %-22s library %.3e  torch fp32 %.3e  ratio %.2f" % (name, k, e, e32, e / e32))
        if e > FACTOR * e32:
            bad.append((k, e, e32))
    assert not bad, bad


@pytest.mark.parametrize("name", list(SEEDS))
def test_block_training_forward_backward_fp32(name):
    blk, x, dout = _case(name)
    ref64, pre = _train_ref(blk, x, dout, torch.float64)
    margin = min(t.abs().min().item() for t in pre)
    assert margin >= RELU_MARGIN, (name, margin)
    ref32, _ = _train_ref(blk, x, dout, torch.float32)
    mod = copy.deepcopy(blk).to(DEV).train()
    xg = x.permute(0, 2, 3, 1).contiguous().to(DEV).detach().requires_grad_()
    out = mod(xg)
    out.backward(dout.permute(0, 2, 3, 1).contiguous().to(DEV))
    torch.cuda.synchronize()
    got = {"out": out.detach().permute(0, 3, 1, 2), "dx": xg.grad.permute(0, 3, 1, 2)}
    for n, p in mod.named_parameters():
        assert p.grad is not None, n
        got[n] = p.grad
    _check(name, got, ref64, ref32)


@pytest.mark.parametrize("name", ["basic64-128s2", "bottleneck256-512s2"])
def test_block_eval_forward_fp32(name):
    """blk.eval(): running statistics, the downsample conv after the main branch; forward only."""
    blk, x, _ = _case(name)
    with torch.no_grad():
        ref64 = {"out": _ref_block(copy.deepcopy(blk).double(), x.double())}
        ref32 = {"out": _ref_block(blk, x)}
        mod = copy.deepcopy(blk).to(DEV).eval()
        out = mod(x.permute(0, 2, 3, 1).contiguous().to(DEV))
    torch.cuda.synchronize()
    _check(name + " eval", {"out": out.permute(0, 3, 1, 2)}, ref64, ref32)
