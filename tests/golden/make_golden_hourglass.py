"""Golden vectors for the stacked-hourglass CenterNet, from the REAL reference (build container only; needs
/root/reference, as make_golden_ae.py).

  hourglass.npz
    keys, shapes            the ordered state-dict entries of the reference's default CenterNetHourglass()
    <case>|keys, |shapes    the entries of the case's two-level net (what both sides feed oracle.centernet.hash_weights)
    <case>|seed             the input seed (below), <case>|floor the float32-against-float64 gradient floor it achieved,
                            <case>|out_floor the largest absolute float32-against-float64 output difference
    <case>|out|<head>       float64 outputs
    <case>|gnorm            float64 gradient norm per parameter, in named_parameters() order (<case>|pnames)
    <case>|gsamp, |gpos     16 sampled gradient elements per parameter and their flat positions
                            (RandomState(crc32(name)).randint(0, numel, 16), the rule of make_golden.py)
    <case>|gmax             max |g| per parameter

Case A: StackHourglass(2, 1, [64, 64, 128], [1, 1, 2], 1, predictionConvDim=128, ...) in the wiring of the reference's
CenterNetHourglass (no pool layer, stride-2 makeHourglassLayer, Residual, beforeBackbone = Convolution(7, 1, 128, 2) +
Residual(3, 128, 64, 2), the three convolutionConv1x1 terminals), input (2, 1, 64, 64).
Case B: dimensions [64, 128, 192], modules [2, 1, 2], predictionConvDim=256, input (3, 1, 64, 96): an odd batch, a
non-square map, a 192-wide level.

No weights are stored: both sides load hash_weights over the reference model's own entries.  The model runs in train
mode.  Input RandomState(seed).standard_normal; loss = sum over the three outputs of (out * w).sum() with
w = 0.25 + 0.75 * RandomState(7).random_sample(out.shape) (a fresh RandomState(7) per output; positive weights, so no
bias gradient cancels to zero).

The seed is the first, counting from 0, for which every parameter's float32 gradient is within 1e-5 of that tensor's
max |g| of its float64 gradient: on other seeds a near-zero pre-activation flips a ReLU between the two precisions and
the reference alone differs by 1e-2 .. 2e-1, which bounds nothing.  The script asserts the condition and stores the
floor.
"""
import os
import sys
import types
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
for _n in ["torchvision", "torchvision.transforms", "torchvision.transforms.functional"]:
    sys.modules[_n] = types.ModuleType(_n)
sys.modules["torchvision"].transforms = sys.modules["torchvision.transforms"]
sys.modules["torchvision.transforms"].functional = sys.modules["torchvision.transforms.functional"]
sys.path.insert(0, "/root/reference")
sys.path.insert(1, REPO)

import torch  # noqa: E402

import models.centerNetOffseth as ref  # noqa: E402  (the reference's)
from models.backbones.convolutions import Convolution  # noqa: E402
from models.backbones.residuals import Residual  # noqa: E402
from models.backbones.stackHourglass import StackHourglass  # noqa: E402

from oracle import centernet as O  # noqa: E402

HEADS = ("heatmap", "regr", "offset")
CASES = {"A": dict(dims=[64, 64, 128], mods=[1, 1, 2], pred=128, shape=(2, 1, 64, 64)),
         "B": dict(dims=[64, 128, 192], mods=[2, 1, 2], pred=256, shape=(3, 1, 64, 96))}
FLOOR = 1e-5


def sample_positions(name, numel, k):
    rs = np.random.RandomState(zlib.crc32(name.encode()) & 0xFFFFFFFF)
    return rs.randint(0, numel, k)


def loss_weight(shape):
    return 0.25 + 0.75 * np.random.RandomState(7).random_sample(shape)


def build(case):
    return StackHourglass(
        2, 1, case["dims"], case["mods"], 1, predictionConvDim=case["pred"], hourglassPool=ref.makePoolLayer,
        hourglassBefore=ref.makeHourglassLayer, hourglassLayer=Residual,
        beforeBackbone=torch.nn.Sequential(Convolution(7, 1, 128, stride=2), Residual(3, 128, case["dims"][0], stride=2)),
        terminals=[ref.heatmapTerminalHg, ref.sizeRegressionTerminalHg, ref.offsetRegressionTerminalHg],
        decoder=ref.decodeCenterNet)


def entries_of(model):
    return [(k, tuple(v.shape)) for k, v in model.state_dict().items()]


def run(case, entries, seed, dtype):
    model = build(case)
    model.load_state_dict(O.hash_weights(entries))
    model = model.to(dtype).train()
    x = torch.from_numpy(np.random.RandomState(seed).standard_normal(case["shape"])).to(dtype)
    out = model(x)[0]
    loss = sum((out[h] * torch.from_numpy(loss_weight(tuple(out[h].shape))).to(dtype)).sum() for h in HEADS)
    loss.backward()
    grads = [(n, p.grad.detach().double().numpy()) for n, p in model.named_parameters()]
    return {h: out[h].detach().double().numpy() for h in HEADS}, grads


def main():
    out = {}
    default = ref.CenterNetHourglass()
    ent = entries_of(default)
    out["keys"] = np.array([k for k, _ in ent])
    out["shapes"] = np.array([",".join(map(str, s)) for _, s in ent])
    for name, case in CASES.items():
        entries = entries_of(build(case))
        seed = 0
        while True:
            o64, g64 = run(case, entries, seed, torch.float64)
            o32, g32 = run(case, entries, seed, torch.float32)
            floor = max(np.abs(a - b).max() / np.abs(a).max() for (_, a), (_, b) in zip(g64, g32))
            print("case %s seed %d: float32 gradient floor %.3g" % (name, seed, floor))
            if floor <= FLOOR:
                break
            seed += 1
        assert floor <= FLOOR
        assert all(np.abs(g).max() > 0 for _, g in g64)
        out_floor = max(np.abs(o64[h] - o32[h]).max() for h in HEADS)
        print("case %s: seed %d, gradient floor %.3g, output floor %.3g" % (name, seed, floor, out_floor))
        out[name + "|keys"] = np.array([k for k, _ in entries])
        out[name + "|shapes"] = np.array([",".join(map(str, s)) for _, s in entries])
        out[name + "|seed"] = np.int64(seed)
        out[name + "|floor"] = np.float64(floor)
        out[name + "|out_floor"] = np.float64(out_floor)
        for h in HEADS:
            out["%s|out|%s" % (name, h)] = o64[h]
        out[name + "|pnames"] = np.array([n for n, _ in g64])
        out[name + "|gnorm"] = np.array([np.sqrt((g * g).sum()) for _, g in g64])
        out[name + "|gmax"] = np.array([np.abs(g).max() for _, g in g64])
        pos = np.stack([sample_positions(n, g.size, 16) for n, g in g64])
        out[name + "|gpos"] = pos.astype(np.int64)
        out[name + "|gsamp"] = np.stack([g.reshape(-1)[p] for (_, g), p in zip(g64, pos)])
    np.savez_compressed(os.path.join(HERE, "hourglass.npz"), **out)
    print("hourglass fixtures written: %d arrays" % len(out))


if __name__ == "__main__":
    main()
