"""Time the random-angle rotation augmentation for one B=32 batch of 512 x 512 tiles already in HBM.

1. scd_augment_tiles alone against scd_augment_tiles + scd_rotate_tiles, for every thread-to-pixel mapping of the
   rotation kernel (ops.ROTATE_MAPS), at angles uniform in +-2 degrees (the reference's range) and in +-180 degrees.
2. SCD.gpu_batch of a `.d` archive of 512 x 512 tiles with rotateAugmentation at 0 and at 30, which adds the
   host-side SCD.rotateLocs per sample; that host part is also timed alone.
Host clock around a device synchronise, median of 50 rounds after 5 warm-up rounds; at most 16 host threads.
Run under a time limit:  timeout 300 python tools/rotate_bench.py > profiles/rotate_aug.txt
"""
import os
import statistics
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "scd-resnet_amd"))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402
import torch  # noqa: E402

torch.set_num_threads(min(16, torch.get_num_threads()))

from configuration import defaultConfig  # noqa: E402
from scdhip import ops  # noqa: E402
from trainer.dataset import scdx16p100 as D  # noqa: E402

B, S, ROUNDS, WARMUP = 32, 512, 50, 5


def median_ms(fn, sync=True):
    times = []
    for r in range(WARMUP + ROUNDS):
        if sync:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        if sync:
            torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    t = times[WARMUP:]
    return statistics.median(t), min(t), max(t)


def kernels():
    tiles = torch.randn(B, 1, S, S, device="cuda") * 30 + 100
    flips = torch.randint(0, 2, (B, 2), dtype=torch.uint8, device="cuda")
    jit = 1 + 0.05 * torch.randn(B, device="cuda")
    aug, rot = torch.empty_like(tiles), torch.empty_like(tiles)

    def augment():
        ops.augment_tiles(tiles, flips, jit, None, 0.05, 1, out=aug)
    base = median_ms(augment)
    nbytes = B * S * S * 4
    print("B=%d %dx%d tiles in HBM; host clock around a synchronise, median (min .. max) of %d rounds" % (
        B, S, S, ROUNDS))
    print("augment_tiles alone:                          %.4f ms (%.4f .. %.4f)" % base)
    rs = np.random.RandomState(3)
    for label, span in (("+-2 deg", 2.0), ("+-180 deg", 180.0)):
        angles = (rs.uniform(size=B) * 2 * span - span).tolist()
        for mapping in sorted(ops.ROTATE_MAPS, key=ops.ROTATE_MAPS.get):
            def both():
                augment()
                ops.rotate_tiles(aug, angles, out=rot, mapping=mapping)

            def alone():
                ops.rotate_tiles(aug, angles, out=rot, mapping=mapping)
            t, a = median_ms(both), median_ms(alone)
            print("augment_tiles + rotate_tiles %-9s %-6s  %.4f ms (%.4f .. %.4f), +%.4f ms; rotate_tiles alone "
                  "%.4f ms (%.4f .. %.4f) = %.0f GB/s over %d read + %d written bytes" % (
                      label, mapping, t[0], t[1], t[2], t[0] - base[0], a[0], a[1], a[2],
                      2 * nbytes / a[0] / 1e6, nbytes, nbytes))
    print("(rotate_tiles alone includes its host side: %d cosines and sines and their one copy to the device)" % B)


def batches():
    from oracle import scd_archive
    with tempfile.TemporaryDirectory() as d:
        names, samples, locs = scd_archive.archive_content(seed=5, count=72, size=S)
        path = os.path.join(d, "bench.d")
        D.writeArchive(path, names, samples, locs)
        old = dict(defaultConfig.config)
        defaultConfig.config["dirTemp"] = os.path.join(d, "temp") + "/"
        defaultConfig.config["dirDataSplitProfile"] = os.path.join(d, "split.json")
        try:
            ds = D.SCD(path, True, {"validation": list(range(8))})
            idx = list(range(1, B + 1))
            nobj = [len(ds.bounds[ds.order[i]]) for i in idx]
            print("gpu_batch of %d tiles of a %d-tile archive (%d .. %d objects per tile, %d in the batch):" % (
                B, len(names), min(nobj), max(nobj), sum(nobj)))
            res = {}
            for key in (0, 30):
                defaultConfig.config["rotateAugmentation"] = key
                res[key] = median_ms(lambda: ds.gpu_batch(idx))
                print("  rotateAugmentation = %-2d  %.3f ms (%.3f .. %.3f)" % ((key,) + res[key]))
            rows = [D.SCD.flipLocs(ds.bounds[ds.order[i]], True, False) for i in idx]
            host = median_ms(lambda: [D.SCD.rotateLocs(r, 17.0) for r in rows], sync=False)
            print("  host-side rotateLocs for the batch alone (%d calls): %.3f ms (%.3f .. %.3f)" % ((B,) + host))
            print("  the switch costs %.3f ms per batch" % (res[30][0] - res[0][0]))
        finally:
            defaultConfig.config.clear()
            defaultConfig.config.update(old)


if __name__ == "__main__":
    print("device: %s; torch %s; libscdhip %s; %s" % (
        torch.cuda.get_device_name(0), torch.__version__, ops.L.lib().dll.scd_version().decode(),
        time.strftime("%Y-%m-%d")))
    kernels()
    batches()
