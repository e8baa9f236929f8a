"""Record of the hourglass up path and the hourglass training step (profiles/hourglass.txt), one process.

python tools/hourglass_bench.py [--rounds 50] [--inner 20]

1. The merge forward / backward at (32, 64 -> 128, 64 -> 128, 128) bf16: scd_upsample2x_add / _bwd against the torch
   route on the device, `up + F.interpolate(low, scale_factor=2)` and `4 * F.avg_pool2d(dout, 2)` on channels-last
   tensors (NCHW views of the same NHWC memory).  A round is `inner` back-to-back launches between two host clock
   reads, each after a synchronise; the routes alternate round by round; the figure is the median of the rounds per
   launch, with the bytes moved (forward 9, backward 5 units of N*h*w*C elements) over that time.
2. scd_bn_apply without a residual on the merge's output shape, for scale: a 2-unit stream of the same library
   (what tools/hbm_bench.py reads as "bn_apply relu").
3. One bf16 training step (forward, CenterNetLoss, backward, FlatAdam) of CenterNetHourglass() at B = 8, 512^2 and
   of centerOffsetRes10 at the same batch, alternated, median of `rounds` steps each.
"""
import argparse
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "scd-resnet_amd"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from oracle import targets as T  # noqa: E402
from scdhip import lib as L  # noqa: E402
from scdhip import ops  # noqa: E402


def clocked(fn, inner):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / inner * 1e6


def alternate(routes, rounds, inner):
    """{name: fn} -> {name: median us per call}, the routes taking turns round by round."""
    for fn in routes.values():
        clocked(fn, 3)
    times = {k: [] for k in routes}
    for _ in range(rounds):
        for k, fn in routes.items():
            times[k].append(clocked(fn, inner))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in times.items()}


def merge_rows(rounds, inner):
    N, h, w, C = 32, 64, 64, 128
    bf = torch.bfloat16
    up = torch.randn(N, 2 * h, 2 * w, C, device="cuda").to(bf)
    low = torch.randn(N, h, w, C, device="cuda").to(bf)
    dout = torch.randn(N, 2 * h, 2 * w, C, device="cuda").to(bf)
    out = torch.empty_like(up)
    up_cl, low_cl, dout_cl = up.permute(0, 3, 1, 2), low.permute(0, 3, 1, 2), dout.permute(0, 3, 1, 2)
    assert up_cl.is_contiguous(memory_format=torch.channels_last)
    unit = N * h * w * C * 2
    y = torch.empty_like(up)
    sc, sh = torch.rand(C, device="cuda") + 0.5, torch.randn(C, device="cuda") * 0.1
    fwd = alternate({"scd_upsample2x_add": lambda: ops.upsample_add(up, low, out=out),
                     "torch up + interpolate(low)": lambda: up_cl + F.interpolate(low_cl, scale_factor=2)},
                    rounds, inner)
    bwd = alternate({"scd_upsample2x_add_bwd": lambda: ops.upsample_add_bwd(dout),
                     "torch 4 * avg_pool2d(dout, 2)": lambda: 4 * F.avg_pool2d(dout_cl, 2)}, rounds, inner)
    bn = alternate({"scd_bn_apply relu (2 units x 4)": lambda: L.call(
        "scd_bn_apply", L.DT_BF16, up.data_ptr(), y.data_ptr(), C, up.numel(), sc.data_ptr(), sh.data_ptr(), 0, 0, 0, 1,
        ops.stream())}, rounds, inner)
    print("merge at (%d, %d -> %d, %d -> %d, %d) bf16; one unit = %.1f MB" % (N, h, 2 * h, w, 2 * w, C, unit / 1e6))
    for rows, units in ((fwd, 9), (bwd, 5), (bn, 8)):
        for k, (med, lo, hi) in rows.items():
            print("  %-34s %8.1f us (min %.1f max %.1f)  %5.0f GB/s over %d units" % (k, med, lo, hi,
                                                                                  units * unit / med / 1e3, units))


def step_rows(rounds):
    import trainer.model.centerOffsetHourglass as hg
    import trainer.model.centerOffsetRes10 as r10
    from scdhip.flat import FlatAdam
    B = 8
    x = T.batch_inputs(61, B, 512).cuda()
    ys = [t.cuda() for t in T.batch_targets(62, B, 128)]
    steps = {}
    for name, plugin in (("centerOffsetHourglass", hg), ("centerOffsetRes10", r10)):
        torch.random.manual_seed(42)
        m = plugin.model(**plugin.modelParams).cuda().train().set_compute_dtype(torch.bfloat16)
        opt = FlatAdam(filter(lambda p: p.requires_grad, m.parameters()))
        nparam = sum(p.numel() for p in m.parameters())

        def step(m=m, opt=opt, plugin=plugin):
            opt.zero_grad()
            plugin.loss.prepare(ys)
            loss, _ = plugin.loss(m(x, decode=False), ys)
            loss.mean().backward()
            opt.step()
        steps["%s (%.1f M parameters)" % (name, nparam / 1e6)] = step
    res = alternate(steps, rounds, 1)
    print("one bf16 training step at B = %d, 512^2 (eager, no step graph)" % B)
    for k, (med, lo, hi) in res.items():
        print("  %-44s %9.2f ms (min %.2f max %.2f)  %7.1f images/s" % (k, med / 1e3, lo / 1e3, hi / 1e3, B / med * 1e6))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=50)
    ap.add_argument("--inner", type=int, default=20)
    a = ap.parse_args()
    p = torch.cuda.get_device_properties(0)
    print("%s, %d CUs, torch %s, %s, %s" % (p.name, p.multi_processor_count, torch.__version__,
                                        L.lib().dll.scd_version().decode(), time.strftime("%Y-%m-%d")))
    merge_rows(a.rounds, a.inner)
    step_rows(a.rounds)


if __name__ == "__main__":
    main()
