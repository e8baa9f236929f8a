"""Time CornerNet target rendering for one B=32 batch at H=128 (the synthetic set's 5-20 objects per tile) and write
profiles/corner_targets.txt:
  * scd_render_corner_targets, one launch, at each split of the pixel work over the three maps (ops.CORNER_SPLITS);
  * the only device route without it: the corner rows derived with torch ops, three scd_render_center_targets launches;
  * CornerSCD's per-sample host rendering of the same batch's targets (numpy, one thread).
The device routes alternate in one process; each figure is the median of 50 rounds of the host clock around the calls
and a device synchronise."""
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "scd-resnet_amd"))
import torch  # noqa: E402

import scdhip.lib as L  # noqa: E402
from scdhip import ops  # noqa: E402
from trainer.dataset.syntheticCorner import CornerSCD, corner_locs  # noqa: E402
from trainer.dataset.syntheticSCD import encode_targets  # noqa: E402

B, H, ROUNDS = 32, 128, 50


def three_launches(locs, counts):
    """[heat, mask, regr, tl, br]: corner_locs in torch on the device, then the centre renderer per map."""
    dx, dy = locs[:, :, 4].abs().round(), locs[:, :, 6].round()
    heat, mask, regr, _ = ops.render_center_targets(locs, counts, H)
    maps = []
    for sign in (-1.0, 1.0):
        c = locs.clone()
        c[:, :, 0] = (locs[:, :, 0] + sign * dx).clamp(0, H - 1)
        c[:, :, 1] = (locs[:, :, 1] + sign * dy).clamp(0, H - 1)
        maps.append(ops.render_center_targets(c, counts, H)[0])
    return [heat, mask, regr] + maps


def main():
    ds = CornerSCD(None, True, seed=500)
    _, locs, counts = ds.batch_rows(range(B))
    locs, counts = locs.cuda(), counts.cuda()
    routes = [("scd_render_corner_targets, split %s" % s,
               lambda s=s: ops.render_corner_targets(locs, counts, H, split=s))
              for s in sorted(ops.CORNER_SPLITS, key=ops.CORNER_SPLITS.get)]
    routes.append(("torch corner rows + 3 x scd_render_center_targets", lambda: three_launches(locs, counts)))
    want = routes[0][1]()
    for name, fn in routes:                       # warm up, and the routes agree bit for bit
        got = fn()
        assert all(torch.equal(a, b) for a, b in zip(got[:5], want[:5])), name
    times = {name: [] for name, _ in routes}
    for _ in range(ROUNDS):
        for name, fn in routes:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e6)
    rows = [r[:n] for r, n in zip(locs.cpu().numpy(), counts.tolist())]
    t0 = time.perf_counter()
    for _ in range(5):
        for r in rows:                            # what CornerSCD.item renders per sample
            for c in (r,) + corner_locs(r, H):
                encode_targets(c, H)
    host_ms = (time.perf_counter() - t0) / 5 * 1e3
    lines = ["device: %s; torch %s; libscdhip %s; %s" % (
        torch.cuda.get_device_name(0), torch.__version__, L.lib().scd_version().decode(), time.strftime("%Y-%m-%d")),
        "CornerNet targets of one batch: B=%d, H=%d, %d objects (5-20 per tile)" % (B, H, int(counts.sum())),
        "host clock around the calls and a synchronise, median of %d alternating rounds (min .. max), microseconds"
        % ROUNDS]
    for name, _ in routes:
        t = times[name]
        lines.append("  %-52s %8.1f  (%.1f .. %.1f)" % (name, statistics.median(t), min(t), max(t)))
    lines.append("  %-52s %8.2f ms (CornerSCD.item's three encode_targets per sample, numpy, one thread)" % (
        "per-sample host rendering of the batch", host_ms))
    lines.append("scd_render_corner_targets without a split named uses SCD_CORNER_SPLIT_DEFAULT (include/scdhip.h); "
                 "every route gave the same bits.")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    out = os.environ.get("CORNER_TARGETS_OUT", os.path.join(REPO, "profiles", "corner_targets.txt"))
    with open(out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
