"""Record of the dynamic fp16 loss scale's cost (profiles/loss_scale.txt), one process.

python tools/loss_scale_bench.py [--rounds 50] [--inner 20] [--only kernels|steps|static-step] [--tree DIR]

1. scd_grad_guard over a flat fp32 gradient of centerOffsetRes10's and of centerOffsetRes50's parameter count (taken
   from the models), and scd_adam_step_dev on the same buffers for scale: Adam moves seven words per element (reads
   p, g, m, v; writes p, m, v) to the guard's one.  A round is `inner` back-to-back calls between two host clock reads,
   each read after a synchronise; all shapes are warmed first; the routes take turns round by round; the figure is the
   median round per call.
2. The fp16 centerOffsetRes10 training step (forward, CenterNetLoss, backward, FlatAdam) at B = 32, 512^2 with the
   loss scale static against dynamic (a DynamicLossScale attached at the same S = 1024, growth_interval out of reach,
   update() after every step), the two alternated round by round in this process, `inner` steps per round.
3. --only static-step: the static step alone; with --tree DIR the package (and its libscdhip.so) is imported from
   another checkout, so the parent commit's static step can be run by this file in a process of its own.
"""
import argparse
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def clocked(fn, inner):
    import torch
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


def kernel_rows(rounds, inner):
    import importlib

    import torch

    from scdhip import ops
    routes, size = {}, {}
    for name in ("centerOffsetRes10", "centerOffsetRes50"):
        plugin = importlib.import_module("trainer.model." + name)
        n = sum(p.numel() for p in plugin.model(**plugin.modelParams).parameters() if p.requires_grad)
        g = torch.randn(n, device="cuda") * 1e-3
        p, m, v = torch.randn(n, device="cuda"), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
        hyper = torch.tensor([1e-3, 0.0], dtype=torch.float64, device="cuda")
        ws = torch.zeros(ops.grad_guard_workspace(n), dtype=torch.uint8, device="cuda")
        out = torch.zeros(3, dtype=torch.int64, device="cuda")
        routes["scd_grad_guard     " + name] = lambda g=g, ws=ws, out=out: ops.grad_guard(g, ws, out[:2], out[2:])
        routes["scd_adam_step_dev  " + name] = lambda p=p, g=g, m=m, v=v, hyper=hyper: ops.adam_step_dev(
            p, g, m, v, hyper, 0.9, 0.999, 1e-8)
        size["scd_grad_guard     " + name] = (n, 1)
        size["scd_adam_step_dev  " + name] = (n, 7)
    res = alternate(routes, rounds, inner)
    print("flat fp32 buffers of the models' trainable parameter counts; bytes = words moved per element x 4 x n")
    for k, (med, lo, hi) in res.items():
        n, words = size[k]
        nbytes = 4 * n * words
        print("  %-38s n %9d  %7.1f MB  %8.1f us (min %.1f max %.1f)  %6.0f GB/s" % (k, n, nbytes / 1e6, med, lo, hi,
                                                                                nbytes / med / 1e3))


def step_rows(rounds, inner, dynamic):
    import torch

    import trainer.model.centerOffsetRes10 as plugin
    from oracle import targets as T
    from scdhip import ops
    from scdhip.flat import FlatAdam
    B = 32
    x = T.batch_inputs(61, B, 512).cuda()
    ys = [t.cuda() for t in T.batch_targets(62, B, 128)]
    steps, scaler = {}, None
    for name in ("static", "dynamic") if dynamic else ("static",):
        torch.random.manual_seed(42)
        m = plugin.model(**plugin.modelParams).cuda().train().set_compute_dtype(torch.float16)
        opt = FlatAdam(filter(lambda p: p.requires_grad, m.parameters()))
        if name == "dynamic":
            from scdhip.amp import DynamicLossScale
            scaler = DynamicLossScale(init_scale=ops.LossScale.f16, growth_interval=10 ** 9).attach(opt)

        def step(m=m, opt=opt, update=scaler.update if name == "dynamic" else None):
            opt.zero_grad()
            plugin.loss.prepare(ys)
            loss, _ = plugin.loss(m(x, decode=False), ys)
            loss.mean().backward()
            opt.step()
            if update is not None:
                update()
        steps[name] = step
    res = alternate(steps, rounds, inner)
    print("one fp16 centerOffsetRes10 training step at B = %d, 512^2, S = %g (eager, no step graph), %d steps per round"
          % (B, ops.LossScale.f16, inner))
    for k, (med, lo, hi) in res.items():
        print("  loss scale %-8s %9.3f ms (min %.3f max %.3f)  %7.1f images/s" % (k, med / 1e3, lo / 1e3, hi / 1e3,
                                                                               B / med * 1e6))
    if scaler is not None:
        scaler.update(block=True)
        print("  dynamic: %d steps processed, %d skipped, S = %g at the end (no scale change in the window: %s)"
              % (scaler.steps, scaler.skipped, scaler.scale, scaler.skipped == 0))
        scaler.detach()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=50)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--only", choices=["kernels", "steps", "static-step"], default=None)
    ap.add_argument("--tree", default=REPO, help="the checkout to import the package and its library from")
    a = ap.parse_args()
    tree = os.path.abspath(a.tree)
    sys.path.insert(0, tree)
    sys.path.insert(0, os.path.join(tree, "scd-resnet_amd"))
    import torch

    from scdhip import lib as L
    p = torch.cuda.get_device_properties(0)
    print("%s, %d CUs, torch %s, %s, %s" % (p.name, p.multi_processor_count, torch.__version__,
                                        L.lib().dll.scd_version().decode(), time.strftime("%Y-%m-%d")))
    if a.only in (None, "kernels"):
        kernel_rows(a.rounds, a.inner)
    if a.only in (None, "steps"):
        step_rows(a.rounds, a.inner, True)
    if a.only == "static-step":
        step_rows(a.rounds, a.inner, False)


if __name__ == "__main__":
    main()
