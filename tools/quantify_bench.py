"""Times the per-slide reduction of quantify.py on the recorded fixture slide (tests/golden/slide.npz: T = 48,
K = 100, 3,388 detections): the device path (ops.slide_samples, then one read of the histogram) against the host
path it replaces (ops.slide_detections, the detections read back, then box filter, greedy de-duplication and
binning restated in numpy).  The model is left out of both: it is the same work either way.

    python tools/quantify_bench.py [-o profiles/quantify.txt]

Prints the median and the range of `rounds` timings per leg, host wall clock around a device synchronisation.  A
record, not a claim: no threshold or ratio is asserted.
"""
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "scd-resnet_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from scdhip import ops, rhr  # noqa: E402
import slide  # noqa: E402

BOX = (0, 0, 3072, 2056)


def host_path(dec, score_np, K, g, radius):
    """slide_detections + numpy: what a caller without scd_slide_samples would run per slide."""
    xy, ratio = ops.slide_detections(dec, 384, g["padLR"], g["padTB"], g["clipV"], slide.THRESHOLD)
    xy, ratio = xy.cpu().numpy().astype(np.int64), ratio.cpu().numpy()
    flat = np.flatnonzero(score_np > np.float32(slide.THRESHOLD))
    ok = (xy[:, 0] >= BOX[0]) & (xy[:, 0] < BOX[2]) & (xy[:, 1] >= BOX[1]) & (xy[:, 1] < BOX[3])
    xy, ratio, flat = xy[ok], ratio[ok], flat[ok]
    keep = np.ones(flat.size, bool)
    if radius >= 0:
        sc, clip = score_np[flat], flat // K
        order = np.lexsort((flat, -sc.astype(np.float64)))
        keep[:] = False
        kept = np.zeros(flat.size, np.int64)
        m = 0
        for q in order:
            k = kept[:m]
            d2 = (xy[k, 0] - xy[q, 0]) ** 2 + (xy[k, 1] - xy[q, 1]) ** 2
            if np.any((clip[k] != clip[q]) & (d2 <= radius * radius)):
                continue
            keep[q] = True
            kept[m] = q
            m += 1
    b = rhr.bin_index(ratio[keep])
    return np.bincount(b[b >= 0], minlength=rhr.BINS)


def device_path(dec, g, radius, hist, counters):
    hist.zero_()
    counters.zero_()
    ops.slide_samples(dec, 384, g["padLR"], g["padTB"], g["clipV"], slide.THRESHOLD, BOX, radius, hist, counters)
    return hist.cpu().numpy()


def timed(fn, rounds):
    ts = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def main(argv):
    out = argv[argv.index("-o") + 1] if "-o" in argv else None
    gold = np.load(os.path.join(REPO, "tests", "golden", "slide.npz"))
    dec_np = gold["decoded"]
    _, T, K = dec_np.shape
    dec = torch.from_numpy(dec_np).cuda()
    score_np = dec_np[0].reshape(-1)
    g = slide.geometry(2056, 3092)
    hist = torch.zeros(rhr.BINS, dtype=torch.int64, device="cuda")
    counters = torch.zeros(5, dtype=torch.int64, device="cuda")
    lines = ["quantify_bench: %s, decoded (10, %d, %d), box %s, torch %s" % (
        torch.cuda.get_device_name(0), T, K, " ".join(map(str, BOX)), torch.__version__)]
    for radius in (-1, 8, 16):
        a, b = host_path(dec, score_np, K, g, radius), device_path(dec, g, radius, hist, counters)
        same = bool(np.array_equal(a, b))
        for _ in range(3):
            device_path(dec, g, radius, hist, counters)
        dm, dlo, dhi = timed(lambda: device_path(dec, g, radius, hist, counters), 50)
        hm, hlo, hhi = timed(lambda: host_path(dec, score_np, K, g, radius), 10)
        lines.append("radius %3d  kept %5d  histograms equal %s  device %.3f ms (%.3f .. %.3f, 50 rounds)  "
                     "host %.3f ms (%.3f .. %.3f, 10 rounds)" % (radius, int(counters[2]), same, dm, dlo, dhi, hm, hlo,
                                                                 hhi))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if out:
        with open(out, "w") as fh:
            fh.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
