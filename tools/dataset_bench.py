"""Time a training batch from a `.d` archive: the host path of SCD.gpu_batch against the device-resident archive
(configuration key residentDataset), one B=32 batch of 512 x 512 tiles.

1. The two kernels the resident path adds, alone, on data already in HBM: scd_augment_tiles_indexed (against
   scd_augment_tiles on the stacked tiles) and scd_pack_locs without and with rotation.
2. SCD.gpu_batch of one archive with residentDataset off and on, alternated round by round in one process, with
   rotateAugmentation at 0 and at 30.
3. The CenterNet-Res10 bf16 B=32 training step fed by gpu_batch: wall time per iteration of `batch, step` loops (one
   synchronise at the end, as the training loop runs), both paths, the step alone on a fixed batch, and the host-side
   time of the gpu_batch calls inside those loops.
tools/rotate_bench.py's clock: host time around a device synchronise, median of 50 rounds after 5 warm-up rounds; at
most 16 host threads.
Run under a time limit:  timeout 420 python tools/dataset_bench.py > profiles/resident_dataset.txt
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

B, S, ROUNDS, WARMUP, TILES = 32, 512, 50, 5, 72


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def summary(times):
    t = times[WARMUP:]
    return statistics.median(t), min(t), max(t)


def median_ms(fn):
    return summary([timed(fn) for _ in range(WARMUP + ROUNDS)])


def alternated(fns):
    """Every function once per round, in turn: drift of the machine falls on all of them alike."""
    times = [[] for _ in fns]
    for _ in range(WARMUP + ROUNDS):
        for t, fn in zip(times, fns):
            t.append(timed(fn))
    return [summary(t) for t in times]


def kernels(ds):
    res = ds.resident
    store, rows, offsets = res["store"], res["rows"], res["offsets"]
    rs = np.random.RandomState(3)
    ids = rs.randint(0, store.shape[0], B).tolist()
    dids = torch.tensor(ids, dtype=torch.int32, device="cuda")
    flips = torch.randint(0, 2, (B, 2), dtype=torch.uint8, device="cuda")
    jit = 1 + 0.05 * torch.randn(B, device="cuda")
    stacked = store[ids].contiguous()[:, None]
    out = torch.empty_like(stacked)
    cs = ops.pack_locs_cs((rs.uniform(size=B) * 60 - 30).tolist()).to("cuda")
    nobj = (offsets[1:] - offsets[:-1])[ids]
    print("kernels alone, B=%d of a %d-tile store of %dx%d in HBM (%d .. %d objects per tile, %d in the batch):" % (
        B, store.shape[0], S, S, int(nobj.min()), int(nobj.max()), int(nobj.sum())))
    a, b = alternated([lambda: ops.augment_tiles(stacked, flips, jit, None, 0.05, 1, out=out),
                       lambda: ops.augment_tiles_indexed(store, dids, flips, jit, None, 0.05, 1, out=out)])
    print("  augment_tiles on the stacked tiles:   %.4f ms (%.4f .. %.4f)" % a)
    print("  augment_tiles_indexed from the store: %.4f ms (%.4f .. %.4f)" % b)
    a, b = alternated([lambda: ops.pack_locs(rows, offsets, dids, flips),
                       lambda: ops.pack_locs(rows, offsets, dids, flips, cs=cs)])
    print("  pack_locs, flips only:                %.4f ms (%.4f .. %.4f)" % a)
    print("  pack_locs, flips and rotation:        %.4f ms (%.4f .. %.4f)" % b)
    print("  (each includes its host side: the output allocations and one launch, two for the augmentation)")


def batches(ds):
    idx = list(range(1, B + 1))
    nobj = [len(ds.bounds[ds.order[i]]) for i in idx]
    print("gpu_batch of %d tiles of a %d-tile archive (%d .. %d objects per tile, %d in the batch), the two paths "
          "alternated:" % (B, TILES, min(nobj), max(nobj), sum(nobj)))

    def batch(resident):
        def run():
            defaultConfig.config["residentDataset"] = resident
            return ds.gpu_batch(idx)
        return run
    res = {}
    for key in (0, 30):
        defaultConfig.config["rotateAugmentation"] = key
        res[key] = alternated([batch(False), batch(True)])
        for name, r in zip(("host path    ", "resident path"), res[key]):
            print("  rotateAugmentation = %-2d  %s  %.3f ms (%.3f .. %.3f)" % ((key, name) + r))
    for key in (0, 30):
        h, r = res[key][0][0], res[key][1][0]
        print("  rotateAugmentation = %-2d  resident / host = %.3f (%s)" % (
            key, r / h, "faster" if r < h else "NOT faster"))
    return res


def steps(ds, iters=30):
    import trainer.model.centerOffsetRes10 as plugin
    from scdhip.flat import FlatAdam
    from scdhip.loss import mean_backward
    dev = torch.device("cuda", torch.cuda.current_device())
    model = plugin.model(**plugin.modelParams).to(dev).set_compute_dtype(torch.bfloat16).train()
    opt = FlatAdam(filter(lambda p: p.requires_grad, model.parameters()))
    idx = list(range(1, B + 1))

    def step(b):
        opt.zero_grad()
        loss, _ = plugin.loss(model(b["xs"][0], decode=False), b["ys"])
        mean_backward(loss)
        opt.step()

    host = []       # host-side time of every gpu_batch call inside a loop (no synchronise around it)

    def loop(resident, load=True):
        defaultConfig.config["residentDataset"] = resident
        fixed = ds.gpu_batch(idx)

        def run():
            for _ in range(iters):
                if load:
                    t0 = time.perf_counter()
                    b = ds.gpu_batch(idx)
                    host.append((time.perf_counter() - t0) * 1e3)
                step(b if load else fixed)
        return run
    defaultConfig.config["rotateAugmentation"] = 0
    for _ in range(5):
        loop(True)()
    print("CenterNet-Res10 bf16 B=%d training on %dx%d tiles, wall time per iteration over loops of %d iterations "
          "(median of 5 loops, one synchronise per loop):" % (B, S, S, iters))
    alone = statistics.median(timed(loop(True, load=False)) for _ in range(5)) / iters
    print("  the step alone, on a fixed batch:                         %.3f ms" % alone)
    for key in (0, 30):
        defaultConfig.config["rotateAugmentation"] = key
        for name, resident in (("host path    ", False), ("resident path", True)):
            del host[:]
            t = statistics.median(timed(loop(resident)) for _ in range(5)) / iters
            print("  rotateAugmentation = %-2d  %s  batch + step  %.3f ms  (+%.3f ms on the step alone); gpu_batch's "
                  "host side inside the loop: median %.3f ms (%.3f .. %.3f)" % (
                      key, name, t, t - alone, statistics.median(host), min(host), max(host)))


if __name__ == "__main__":
    print("device: %s; torch %s; libscdhip %s; %s" % (
        torch.cuda.get_device_name(0), torch.__version__, ops.L.lib().dll.scd_version().decode(),
        time.strftime("%Y-%m-%d")))
    print("host clock around a synchronise, median (min .. max) of %d rounds after %d warm-up rounds" % (
        ROUNDS, WARMUP))
    from oracle import scd_archive
    with tempfile.TemporaryDirectory() as d:
        names, samples, locs = scd_archive.archive_content(seed=5, count=TILES, size=S)
        path = os.path.join(d, "bench.d")
        D.writeArchive(path, names, samples, locs)
        old = dict(defaultConfig.config)
        defaultConfig.config["dirTemp"] = os.path.join(d, "temp") + "/"
        defaultConfig.config["dirDataSplitProfile"] = os.path.join(d, "split.json")
        try:
            ds = D.SCD(path, True, {"validation": list(range(8))})
            defaultConfig.config["residentDataset"] = True
            ds.gpu_batch(list(range(1, B + 1)))          # builds the store
            mb = ds.resident["store"].numel() * 4 / 2.0 ** 20
            print("resident store: %d tiles, %.0f MiB (the canonical archive: 49,920 tiles, 48.8 GiB)" % (TILES, mb))
            batches(ds)
            kernels(ds)
            if "--no-step" not in sys.argv:
                steps(ds)
        finally:
            defaultConfig.config.clear()
            defaultConfig.config.update(old)
