"""Time the Res10 B=32 512^2 GEMM launches with 8,192 GEMM rows (layer4.0, its downsample and the deconv1 input
gradient) alone, as the block Functions launch them: HIP events around `--reps` back-to-back launches after a warm-up.

python tools/small_m_bench.py [--reps 200] [--dtype bf16]

  conv1 fwd      3x3 s2 256 -> 512 + BN statistics        (128 x 128 tile, split K: the ring kernel on that tile)
  down fwd       1x1 s2 256 -> 512 + BN statistics        (register-staged 128 x 128, 4 K stages)
  conv2 fwd      3x3 512 -> 512 + BN statistics           (128 x 128, split K)
  deconv1 dgrad  4x4 s2 gather, 256 -> 512                (128 x 128, split K)
  conv2 dgrad    3x3 512 -> 512 + the bn1 backward sums   (128 x 128, split K)
  conv1 dgrad    3x3 s2, 4 sub-pixel phases of 1/2/2/4 taps, 32,768 rows in all (the 256 x 128 ring kernel)
  down dgrad     1x1 s2, += into the block's input gradient (register-staged 128 x 128, 128 tiles)
"""
import argparse
import os
import sys
import types

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "scd-resnet_amd"))
import torch  # noqa: E402

from scdhip import ops  # noqa: E402

B = 32


def timed(fn, reps):
    for _ in range(5):
        fn()
    s = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    for _ in range(reps):
        fn()
    e1.record(s)
    e1.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--dtype", default="bf16", choices=("bf16", "fp16"))
    a = ap.parse_args()
    dt = torch.bfloat16 if a.dtype == "bf16" else torch.float16
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(5)

    def rnd(*shape, scale=1.0):
        return torch.randn(*shape, device=dev, generator=g) * scale

    x = rnd(B, 32, 32, 256).to(dt)                 # the block input
    a1 = rnd(B, 16, 16, 512).to(dt)                # conv2's input
    dy = rnd(B, 16, 16, 512).to(dt)
    w1, w2, wd = rnd(512, 256, 3, 3, scale=1 / 48), rnd(512, 512, 3, 3, scale=1 / 68), rnd(512, 256, 1, 1, scale=1 / 16)
    w1p, w2p, wdp = (ops.pack_weight(w, dt, 0) for w in (w1, w2, wd))
    w1t, w2t, wdt = (ops.pack_weight(w, dt, 1) for w in (w1, w2, wd))
    w13 = ops.pack_weight(w1, dt, 3)
    stats = ops.new_stats(512, dev)
    bst = ops.new_stats(512, dev)
    st = types.SimpleNamespace(mean=rnd(512, scale=0.1), invstd=torch.rand(512, device=dev, generator=g) + 0.5,
                               scale=torch.rand(512, device=dev, generator=g) + 0.5, shift=rnd(512, scale=0.1))
    y1 = rnd(B, 16, 16, 512).to(dt)                # conv1's pre-BN output
    o512 = torch.empty(B, 16, 16, 512, device=dev, dtype=dt)
    dx = torch.zeros(B, 32, 32, 256, device=dev, dtype=dt)
    wu = ops.pack_weight(rnd(512, 256, 4, 4, scale=1 / 64), dt, 0)      # deconv1: ConvTranspose2d(512, 256, 4, 2, 1)

    def conv1_dgrad():
        # ops.conv_dgrad_w's choice, with the operands packed once outside the timed launches
        rc = ops.L.lib().scd_conv_dgrad_s2(ops.dt(dy), ops.ptr(dy), ops.ptr(w13), ops.ptr(dx), B, 16, 16, 512, 256, 0,
                                           ops.stream())
        if rc == 9001:
            ops.conv_dgrad(dy, w1t, 256, 32, 32, 3, 3, 2, 1, out=dx)
        elif rc:
            ops.L.check(rc, "scd_conv_dgrad_s2")

    gf = lambda K, N: 2.0 * B * 256 * K * N / 1e9  # noqa: E731  (8,192 output rows)
    runs = [
        ("layer4.0.conv1 fwd", gf(2304, 512), lambda: ops.conv_fwd(x, w1p, 512, 3, 3, 2, 1, stats=stats, out=o512)),
        ("layer4.0.downsample fwd", gf(256, 512), lambda: ops.conv_fwd(x, wdp, 512, 1, 1, 2, 0, stats=stats, out=o512)),
        ("layer4.0.conv2 fwd", gf(4608, 512), lambda: ops.conv_fwd(a1, w2p, 512, 3, 3, 1, 1, stats=stats, out=o512)),
        ("deconv1 dgrad", gf(4096, 512), lambda: ops.deconv_dgrad(x, wu, 512, out=o512)),
        ("layer4.0.conv2 dgrad", gf(4608, 512),
         lambda: ops.conv_dgrad(dy, w2t, 512, 16, 16, 3, 3, 1, 1, out=o512, bn_bwd=(st, y1, bst))),
        ("layer4.0.conv1 dgrad", gf(2304, 512), conv1_dgrad),
        ("layer4.0.downsample dgrad", gf(256, 512),
         lambda: ops.conv_dgrad(dy, wdt, 256, 32, 32, 1, 1, 2, 0, out=dx, accumulate=True)),
    ]
    print("library %s, %s, %d launches each" % (os.path.basename(ops.L.LIB_PATH), a.dtype, a.reps))
    print("%-28s %8s %9s %7s" % ("launch", "GFLOP", "us alone", "PF/s"))
    tot = 0.0
    for name, gflop, fn in runs:
        us = timed(fn, a.reps)
        tot += us
        print("%-28s %8.1f %9.1f %7.2f" % (name, gflop, us, gflop / us))     # GFLOP per us = PFLOP/s
    print("%-28s %8s %9.1f" % ("sum", "", tot))


if __name__ == "__main__":
    main()
