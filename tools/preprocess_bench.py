"""Time preprocess.py's slide rotation for one 2048 x 3072 slide and R = 16 angles: scd_slide_rotate_clips against
PyTorch-ROCm's F.pad + grid_sample on the same device (HIP events on the launch stream, one warm-up, the median of
10 runs each).  The PyTorch side is given the cheaper schedule: grayscale and both reflect pads once, then per angle
affine_grid + grid_sample + crop (the reference pads again for every repeat, on the CPU).

Usage: python tools/preprocess_bench.py [--out profiles/preprocess_rotate.txt]
"""
import argparse
import math
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "scd-resnet_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from scdhip import lib as L  # noqa: E402
from scdhip import ops  # noqa: E402

H, W, TILE, R, RUNS = 2048, 3072, 512, 16, 10


def torch_rotations(rgb, angles):
    c = rgb.double()
    g = ((0.30 * c[:, :, 0] + 0.59 * c[:, :, 1]) + 0.11 * c[:, :, 2]).float()[None, None]
    radius = math.sqrt(W ** 2 + H ** 2) / 2
    lp, tp = math.ceil(radius - 0.5 * W), math.ceil(radius - 0.5 * H)
    q = F.pad(g, (lp, lp, tp, tp), "reflect")
    hq, wq = q.shape[2:]
    out = []
    for angle in angles:
        a = math.radians(angle)
        theta = torch.tensor([[[math.cos(a), -math.sin(a) * hq / wq, 0.0], [math.sin(a) * wq / hq, math.cos(a), 0.0]]],
                             device=rgb.device)
        grid = F.affine_grid(theta, (1, 1, hq, wq), align_corners=False)
        rot = F.grid_sample(q, grid, mode="bilinear", padding_mode="zeros", align_corners=False)
        out.append(rot[0, 0, tp:tp + H, lp:lp + W].contiguous())
    return out


def timed(fn):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(RUNS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "preprocess_rotate.txt"))
    args = ap.parse_args()
    rs = np.random.RandomState(1)
    rgb = torch.from_numpy(rs.randint(0, 256, (H, W, 3)).astype(np.uint8)).cuda()
    angles = (rs.uniform(size=R) * 30 - 15).tolist()
    hip = timed(lambda: ops.slide_rotate_clips(rgb, (0, 0, 0, 0), TILE, angles))
    ref = timed(lambda: torch_rotations(rgb, angles))
    got = ops.slide_rotate_clips(rgb, (0, 0, 0, 0), TILE, angles)
    want = torch_rotations(rgb, angles)
    diff = max(float((got[r].view(W // TILE, H // TILE, TILE, TILE).permute(1, 2, 0, 3).reshape(H, W) - want[r])
                     .abs().max()) for r in range(R))
    out_bytes = R * H * W * 4
    lines = [
        "%s on %s" % (L.lib().dll.scd_version().decode(), torch.cuda.get_device_name(0)),
        "slide %d x %d x 3 u8, tile %d, R = %d angles in [-15, 15), output %.1f MB fp32; HIP events, 1 warm-up, "
        "median of %d (min .. max)" % (H, W, TILE, R, out_bytes / 1e6, RUNS),
        "scd_slide_rotate_clips (grey pass + one rotation launch, incl. output allocation): %.3f ms (%.3f .. %.3f), "
        "%.0f GB/s of output" % (hip + (out_bytes / hip[0] / 1e6,)),
        "PyTorch-ROCm grayscale + F.pad once, then 16 x (affine_grid + grid_sample + crop): %.3f ms (%.3f .. %.3f), "
        "%.0f GB/s of output" % (ref + (out_bytes / ref[0] / 1e6,)),
        "max |kernel - PyTorch fp32| over the 16 rotations: %.3g (0-255 data; PyTorch's grid is float32)" % diff,
    ]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
