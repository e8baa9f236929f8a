"""Decoded-forward throughput of the eval path against the folded path (scdhip/infer.py): Wrapper(model.eval()) and
Wrapper(fold(model)) on the same model, input and process, for centerOffsetRes10 and centerOffsetRes50 in bf16 at
slide.py's batch (24 clips of 512 x 512).

Both paths are warmed up, then timed alternately over ROUNDS rounds of ITERS forwards each (device events around the
round, so the window ends in a synchronise); reported: images/s at the median round time, the (min .. max) spread over
the rounds, and the speed-up of the medians.  The eval path is the training forward with BatchNorm on running
statistics (a GEMM that writes the pre-BN output, scd_bn_finalize, scd_bn_apply).

Usage: python tools/infer_bench.py [--out profiles/infer_fold.txt] [--rounds 5] [--iters 100] [--batch 24] [--size 512]
"""
import argparse
import importlib
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "scd-resnet_amd"))
import torch  # noqa: E402

from oracle import centernet as O  # noqa: E402
from oracle import targets as T  # noqa: E402
from scdhip import infer  # noqa: E402
from scdhip import lib as L  # noqa: E402
from trainer.wrappers.centerOffsetResidual import Wrapper  # noqa: E402

MODELS = ("centerOffsetRes10", "centerOffsetRes50")


def build(name, dev):
    plugin = importlib.import_module("trainer.model." + name)
    entries, _ = O.model_spec(plugin.modelParams["numLayers"], plugin.modelParams["dims"])
    m = plugin.model(**plugin.modelParams)
    m.load_state_dict(O.hash_weights(entries))
    return m.to(dev).eval().set_compute_dtype(torch.bfloat16)


def round_ms(fn, x, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn(x)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "infer_fold.txt"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=24)
    ap.add_argument("--size", type=int, default=512)
    args = ap.parse_args()
    if args.rounds < 3:
        ap.error("at least three rounds")
    dev = torch.device("cuda", 0)
    lines = ["%s on %s" % (L.lib().dll.scd_version().decode(), torch.cuda.get_device_name(0)),
             "decoded forward (10, B, K), bf16, B = %d at %d x %d; %d warm-up forwards, then eval / fold alternately: "
             "%d rounds of %d forwards each (device events); images/s at the median round (min .. max over rounds)"
             % (args.batch, args.size, args.size, args.warmup, args.rounds, args.iters)]
    x = T.batch_inputs(41, args.batch, args.size).to(dev)
    for name in MODELS:
        m = build(name, dev)
        paths = {"eval": Wrapper(m), "fold": Wrapper(infer.fold(m))}
        with torch.no_grad():
            outs = {k: w(x) for k, w in paths.items()}
            torch.cuda.synchronize()
            for _ in range(args.warmup):
                for w in paths.values():
                    w(x)
            torch.cuda.synchronize()
            ms = {k: [] for k in paths}
            for _ in range(args.rounds):
                for k, w in paths.items():
                    ms[k].append(round_ms(w, x, args.iters))
        dscore = (outs["eval"][0] - outs["fold"][0]).abs().max().item()
        rate = {}
        for k in paths:
            med = statistics.median(ms[k])
            rate[k] = args.batch / med * 1e3
            lines.append("%-18s %-4s %8.3f ms  %9.1f images/s  (%.1f .. %.1f)"
                         % (name, k, med, rate[k], args.batch / max(ms[k]) * 1e3, args.batch / min(ms[k]) * 1e3))
        lines.append("%-18s fold / eval = %.3f x; max |score(eval) - score(fold)| = %.2e (bf16: the folded path rounds "
                     "fewer intermediates)" % (name, rate["fold"] / rate["eval"], dscore))
        del m, paths
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
