"""Time cornerNetAE's new device work at B=32, 128^2 maps, K=100, D=1000 and write profiles/corner_pairs.txt
(DESIGN §8f):
  * scd_corner_pairs (one launch) against the reference's formulation of the pairing in torch ops on the device (the
    N x K x K score, box and mask tensors, topk and gathers of cornerNetLegacy.py:332-446, restated), on the same
    top-K corners; the two alternate in one process and must give the same surviving rows;
  * CornerNetAELossFn forward + backward (three focal maps and the embedding terms, 5-20 objects per tile);
  * one training step (forward, loss, backward, FlatAdam) of cornerNetAE against cornerNetCPool, whose model and loss
    this feature leaves untouched, on the same syntheticCorner batch in bf16, alternating.
Each figure is the median of 50 rounds of the host clock around the calls and a device synchronise.  A record, not a
target."""
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "scd-resnet_amd"))
import torch  # noqa: E402

import scdhip.lib as L  # noqa: E402
from scdhip import ops  # noqa: E402
from scdhip.loss import CornerNetAELossFn  # noqa: E402

B, S, K, D, ROUNDS = 32, 128, 100, 1000, 50


def pairs_torch(tl, br, tl_tag, br_tag, threshold, count):
    """The pairing as the reference states it: every K x K candidate materialised, rejected ones set to -1, topk."""
    (s_tl, i_tl, y_tl, x_tl), (s_br, i_br, y_br, x_br) = tl, br
    N, k = s_tl.shape
    e = lambda t, d: t.view(N, k, 1).expand(N, k, k) if d == 0 else t.view(N, 1, k).expand(N, k, k)     # noqa: E731
    boxes = torch.stack((e(x_tl, 0), e(y_tl, 0), e(x_br, 1), e(y_br, 1)), 3)
    t_tl = tl_tag.view(N, -1).gather(1, i_tl).view(N, k, 1)
    t_br = br_tag.view(N, -1).gather(1, i_br).view(N, 1, k)
    scores = (e(s_tl, 0) + e(s_br, 1)) / 2
    scores[(t_tl - t_br).abs() > threshold] = -1
    scores[e(x_br, 1) < e(x_tl, 0)] = -1
    scores[e(y_br, 1) < e(y_tl, 0)] = -1
    scores, inds = torch.topk(scores.view(N, -1), count)

    def take(t):                        # (N, k, k[, c]) -> (N, count, c) at the kept candidates
        t = t.reshape(N, k * k, -1)
        return t.gather(1, inds[..., None].expand(N, count, t.shape[2]))
    return torch.cat([take(boxes).float(), scores[..., None], take(e(s_tl, 0)), take(e(s_br, 1)),
                      torch.zeros(N, count, 1, device=scores.device)], 2)


def timed(routes, rounds=ROUNDS):
    times = {name: [] for name, _ in routes}
    for _ in range(rounds):
        for name, fn in routes:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e6)
    return times


def main():
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(1)
    lines = ["device: %s; torch %s; libscdhip %s; %s" % (
        torch.cuda.get_device_name(0), torch.__version__, L.lib().scd_version().decode(), time.strftime("%Y-%m-%d")),
        "host clock around the calls and a synchronise, median of %d alternating rounds (min .. max), microseconds"
        % ROUNDS]

    # ---- pairing
    maps = [(torch.randn(B, 1, S, S, generator=g) * 3).to(dev) for _ in range(2)]
    tags = [(torch.randn(B, 1, S, S, generator=g) * 0.7).to(dev) for _ in range(2)]
    tl, br = (ops.decode_topk(m, None, None, K)[:4] for m in maps)
    routes = [("scd_corner_pairs (one launch)", lambda: ops.corner_pairs(tl, br, tags[0], tags[1], 1.0, D)),
              ("the reference's formulation in torch ops", lambda: pairs_torch(tl, br, tags[0], tags[1], 1.0, D))]
    (det, nvalid), want = routes[0][1](), routes[1][1]()
    same = 0
    for b in range(B):                  # the same survivors (torch.topk orders equal scores as it likes: compared sorted)
        n = int(nvalid[b])
        assert n == int((want[b, :, 4] >= 0).sum())
        assert torch.equal(det[b, :n, 4], want[b, :n, 4])
        same += int(torch.equal(det[b, :n], want[b, :n]))
    t = timed(routes)
    lines.append("corner pairing: B=%d, %d^2 maps, K=%d, D=%d; surviving pairs per image %d .. %d; %d of %d images "
                 "row for row the same as the torch route (the others differ only in the order of equal scores)"
                 % (B, S, K, D, int(nvalid.min()), int(nvalid.max()), same, B))
    for name, _ in routes:
        lines.append("  %-52s %8.1f  (%.1f .. %.1f)" % (name, statistics.median(t[name]), min(t[name]), max(t[name])))

    # ---- embedding loss
    from trainer.dataset.syntheticCorner import CornerSCD
    ds = CornerSCD(None, True, seed=500)
    tiles, locs, counts = ds.batch_rows(range(B))
    locs, counts = locs.to(dev), counts.to(dev)
    ys = ops.render_corner_targets(locs, counts, S)[:5] + list(ops.corner_tag_inds(locs, counts, S))
    outs = [torch.randn(B, 1, S, S, generator=g).to(dev).requires_grad_(True) for _ in range(5)]

    def loss_step():
        loss, _ = CornerNetAELossFn.apply(*outs, ys[0], ys[3], ys[4], ys[5], ys[6], ys[7], 1, 1)
        torch.autograd.grad(loss, outs, torch.ones_like(loss))
    loss_step()
    t = timed([("loss", loss_step)])["loss"]
    lines.append("embedding loss: B=%d, %d^2 maps, %d objects (5-20 per tile)" % (B, S, int(ys[7].sum())))
    lines.append("  %-52s %8.1f  (%.1f .. %.1f)" % ("CornerNetAELossFn forward + backward (9 launches)",
                                                   statistics.median(t), min(t), max(t)))

    # ---- training step
    import importlib

    from scdhip.flat import FlatAdam
    x = tiles.to(dev)
    steps = []
    for name, nys in (("cornerNetCPool", 5), ("cornerNetAE", 8)):
        plugin = importlib.import_module("trainer.model." + name)
        torch.manual_seed(0)
        m = plugin.model(**plugin.modelParams).to(dev).train().set_compute_dtype(torch.bfloat16)
        opt = FlatAdam(m.parameters(), lr=2.5e-4)

        def step(m=m, opt=opt, plugin=plugin, t=ys[:nys]):
            opt.zero_grad()
            loss, _ = plugin.loss(m(x, decode=False), t)
            loss.sum().backward()
            opt.step()
        for _ in range(5):
            step()
        steps.append((name, step))
    t = timed(steps)
    lines.append("training step (forward, loss, backward, FlatAdam): bf16, B=%d, %d^2 tiles, ResNet-10" % (B, x.shape[-1]))
    for name, _ in steps:
        lines.append("  %-52s %8.1f  (%.1f .. %.1f)" % (name, statistics.median(t[name]), min(t[name]), max(t[name])))
    a, c = statistics.median(t["cornerNetAE"]), statistics.median(t["cornerNetCPool"])
    lines.append("  cornerNetAE / cornerNetCPool = %.3f" % (a / c))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    out = os.environ.get("CORNER_PAIRS_OUT", os.path.join(REPO, "profiles", "corner_pairs.txt"))
    with open(out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
