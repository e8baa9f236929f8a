"""Record of the deformable-conv kernels and the ResNet-DCN training step (profiles/dcn.txt), one process.

python tools/dcn_bench.py [--rounds 50] [--inner 20] [--batch 32]

The three deformable stages of centerOffsetRes18dcn at 512^2 (B = 32, bf16): (16, 16, 512), (32, 32, 256), (64, 64, 256).
A round is `inner` back-to-back launches between two host clock reads, each after a synchronise; the routes alternate
round by round; the figure is the median of the rounds per launch.
1. scd_dcn_cols (reads x through four corners, writes the 9C columns) beside scd_bn_apply on a tensor of the columns'
   size, read as rows of C channels: the same bytes written, a 2-unit stream of the same library.
2. scd_dcn_cols_bwd beside its cost model's floor, 144 * C * N*H*W bytes of float atomics at 1.3 TB/s, at
   zero-initialised offsets (one corner in four has a weight) and at offsets of +-2 px (all four).
3. One bf16 training step (forward, CenterNetLoss, backward, FlatAdam) of centerOffsetRes18dcn against centerOffsetRes18,
   alternated, median of `rounds` steps each.
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

from oracle import targets as T  # noqa: E402
from scdhip import lib as L  # noqa: E402
from scdhip import ops  # noqa: E402

ATOMIC_RATE = 1.3e12        # chip-wide float-atomic rate, bytes added per second


def clocked(fn, inner):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / inner * 1e6


def alternate(routes, rounds, inner):
    """{name: fn} -> {name: (median, min, max) us per call}, the routes taking turns round by round."""
    for fn in routes.values():
        clocked(fn, 3)
    times = {k: [] for k in routes}
    for _ in range(rounds):
        for k, fn in routes.items():
            times[k].append(clocked(fn, inner))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in times.items()}


def kernel_rows(B, rounds, inner):
    bf = torch.bfloat16
    for H, W, C in ((16, 16, 512), (32, 32, 256), (64, 64, 256)):
        x = torch.randn(B, H, W, C, device="cuda").to(bf)
        om0 = torch.zeros(B, H, W, 32, device="cuda", dtype=bf)
        om2 = torch.zeros(B, H, W, 32, device="cuda")
        om2[..., :18] = torch.rand(B, H, W, 18, device="cuda") * 4 - 2
        om2[..., 18:27] = torch.randn(B, H, W, 9, device="cuda")
        om2 = om2.to(bf)
        dcols = torch.randn(B, H, W, 9 * C, device="cuda").to(bf)
        cols = torch.empty_like(dcols)
        y = torch.empty_like(dcols)
        dx32 = torch.zeros(B, H, W, C, device="cuda")
        dom = torch.empty_like(om0)
        sc, sh = torch.rand(C, device="cuda") + 0.5, torch.randn(C, device="cuda") * 0.1
        s = ops.stream()

        def fwd(om):
            L.call("scd_dcn_cols", L.DT_BF16, x.data_ptr(), om.data_ptr(), cols.data_ptr(), B, H, W, C, 1, 32, 1, s)

        def bwd(om):
            # (dx32 keeps accumulating: the figure is the kernel's, the values are not read)
            L.call("scd_dcn_cols_bwd", L.DT_BF16, dcols.data_ptr(), x.data_ptr(), om.data_ptr(), dx32.data_ptr(),
                   dom.data_ptr(), B, H, W, C, 1, 32, 1, s)

        res = alternate({
            "scd_dcn_cols, zero offsets": lambda: fwd(om0),
            "scd_dcn_cols, +-2 px offsets": lambda: fwd(om2),
            "scd_bn_apply relu, columns' size": lambda: L.call(
                "scd_bn_apply", L.DT_BF16, dcols.data_ptr(), y.data_ptr(), C, dcols.numel(), sc.data_ptr(),
                sh.data_ptr(), 0, 0, 0, 1, s),
            "scd_dcn_cols_bwd, zero offsets": lambda: bwd(om0),
            "scd_dcn_cols_bwd, +-2 px offsets": lambda: bwd(om2)}, rounds, inner)
        colbytes = dcols.numel() * 2
        floor = 144.0 * C * B * H * W / ATOMIC_RATE * 1e6
        print("stage (%d, %d, %d, %d) bf16: columns %.1f MB, atomic floor %.1f us at four corners, %.1f us at one"
              % (B, H, W, C, colbytes / 1e6, floor, floor / 4))
        for k, (med, lo, hi) in res.items():
            print("  %-36s %8.1f us (min %.1f max %.1f)  %6.0f GB/s of column bytes" % (k, med, lo, hi,
                                                                                     colbytes / med / 1e3))


def step_rows(B, rounds):
    import trainer.model.centerOffsetRes18 as r18
    import trainer.model.centerOffsetRes18dcn as r18dcn
    from scdhip.flat import FlatAdam
    x = T.batch_inputs(61, B, 512).cuda()
    ys = [t.cuda() for t in T.batch_targets(62, B, 128)]
    steps = {}
    for name, plugin in (("centerOffsetRes18dcn", r18dcn), ("centerOffsetRes18", r18)):
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
    ap.add_argument("--batch", type=int, default=32)
    a = ap.parse_args()
    p = torch.cuda.get_device_properties(0)
    print("%s, %d CUs, torch %s, %s, %s" % (p.name, p.multi_processor_count, torch.__version__,
                                        L.lib().dll.scd_version().decode(), time.strftime("%Y-%m-%d")))
    kernel_rows(a.batch, a.rounds, a.inner)
    step_rows(a.batch, a.rounds)


if __name__ == "__main__":
    main()
