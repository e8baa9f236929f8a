"""Golden vectors for CornerNet's embedding loss and corner pairing decode, from the REAL reference (build container
only; needs /root/reference and oracle/build_ref_cpool.py's modules, as make_golden_corner.py).

  ae.npz   loss|<case>|...   embeddingLoss (models/losses/embeddings.py) on tags ~ 0.6 N(0,1), called with a uint8
                             mask: with the project's bool masks its `mask + mask` stays bool, `.eq(2)` is false
                             everywhere and push is identically 0.  pull, push and the gradients of
                             pull + push on both tag tensors, from a float32 run and a float64 run of the same tags.
           pair|<case>|...   decodeCornerNet (models/cornerNetLegacy.py:332-446) without regression heads, 3x3 NMS,
                             threshold 1: the maps, the reference's own top-K of both corner maps, and its detections.

Loss cases: `mixed` N = 4, K = 8 with 5, 1, 0 and 8 objects (n = 1: push cancels to ~0; n = 0: the empty image);
`equal` the same counts, two slots of image 0 with identical tags on both corners (|m_i - m_j| = 0 off the diagonal);
`single` one image.  embeddingLoss itself cannot take N = 1 (its squeeze() drops the batch axis and unsqueeze(2) then
raises), so `single` is computed on two images of which the second is empty; the script asserts on `mixed` that an
empty image adds exactly nothing to pull, push and the other images' gradients.

Pairing cases: `small` (N = 2, 16^2, K = 8, count 64) whose image 1 has no surviving pair (every br peak lies left of
every tl peak), `large` (N = 2, 32^2, K = 100, count 1000) whose image 0 has more survivors than count.  Peaks sit on
a stride-3 lattice over a low background, so each is its 3x3 maximum and the top-K are K distinct positive scores.
torch.topk leaves ties unordered, so the script asserts that each image's surviving scores are pairwise distinct and
draws the next seed otherwise.
"""
import os
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
for _n in ["torchvision", "torchvision.transforms", "torchvision.transforms.functional"]:
    sys.modules[_n] = types.ModuleType(_n)
sys.modules["torchvision"].transforms = sys.modules["torchvision.transforms"]
sys.modules["torchvision.transforms"].functional = sys.modules["torchvision.transforms.functional"]
sys.path.insert(0, "/root/reference")
sys.path.insert(1, REPO)

import torch  # noqa: E402

from oracle import build_ref_cpool  # noqa: E402

sys.modules.update(build_ref_cpool.build())
import models.cornerNetLegacy as ref  # noqa: E402
from models.backbones.utility import extractTopK, nonMaximumSuppression  # noqa: E402
from models.losses.embeddings import embeddingLoss  # noqa: E402


def run_loss(tl, br, mask, dtype):
    a = torch.from_numpy(tl).to(dtype).unsqueeze(2).requires_grad_(True)
    b = torch.from_numpy(br).to(dtype).unsqueeze(2).requires_grad_(True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")             # indexing with a uint8 mask is deprecated, and what is wanted here
        pull, push = embeddingLoss(a, b, torch.from_numpy(mask))
        (pull + push).backward()
    return [pull.detach().numpy(), push.detach().numpy(), a.grad[..., 0].numpy(), b.grad[..., 0].numpy()]


def loss_case(rs, counts, K, equal=False):
    N = len(counts)
    tl = (0.6 * rs.standard_normal((N, K))).astype(np.float32)
    br = (0.6 * rs.standard_normal((N, K))).astype(np.float32)
    if equal:
        tl[0, 3], br[0, 3] = tl[0, 1], br[0, 1]
    mask = (np.arange(K)[None, :] < np.asarray(counts)[:, None]).astype(np.uint8)
    return tl, br, mask


def loss_cases():
    out = {}
    rs = np.random.RandomState(7)
    cases = {"mixed": loss_case(rs, [5, 1, 0, 8], 8), "equal": loss_case(rs, [5, 1, 0, 8], 8, equal=True),
             "single": loss_case(rs, [6, 0], 8)}
    for name, (tl, br, mask) in cases.items():
        r32, r64 = run_loss(tl, br, mask, torch.float32), run_loss(tl, br, mask, torch.float64)
        assert r64[1] > 0, (name, r64[1])                           # some image has n >= 2: the tags are pushed apart
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            _, push_bool = embeddingLoss(torch.from_numpy(tl).unsqueeze(2), torch.from_numpy(br).unsqueeze(2),
                                         torch.from_numpy(mask).bool())
        assert push_bool.item() == 0.0                              # the bool-mask result this project does not build
        if name == "single":
            assert not r64[2][1].any() and not r64[3][1].any()
            tl, br, mask = tl[:1], br[:1], mask[:1]
            r32, r64 = [r[:1] if r.ndim else r for r in r32], [r[:1] if r.ndim else r for r in r64]
        for k, v in zip(("tl", "br", "mask"), (tl, br, mask)):
            out["loss|%s|%s" % (name, k)] = v
        for tag, r in (("32", r32), ("64", r64)):
            for k, v in zip(("pull", "push", "gtl", "gbr"), r):
                out["loss|%s|%s%s" % (name, k, tag)] = v
    # an empty image adds exactly nothing: `mixed` without its image 2 gives the same sums and gradients
    tl, br, mask = cases["mixed"]
    keep = [0, 1, 3]
    full, part = run_loss(tl, br, mask, torch.float64), run_loss(tl[keep], br[keep], mask[keep], torch.float64)
    assert full[0] == part[0] and full[1] == part[1]
    assert np.array_equal(full[2][keep], part[2]) and np.array_equal(full[3][keep], part[3])
    # n = 1: the one diagonal term relu(1 - 0) - 1 / (1 + 1e-4) over 1e-4 is all of that image's push
    one = run_loss(tl[1:2].repeat(2, 0), br[1:2].repeat(2, 0), np.stack([mask[1], 0 * mask[1]]), torch.float64)
    assert 0 < one[1] < 1.1
    return out


def lattice_map(rs, N, S, regions):
    """Logits (N,1,S,S): background -8 + noise, a spike ~ 1.5 N(0,1) on every stride-3 lattice point whose x passes
    regions[n] (None: all)."""
    m = (-8 + 0.1 * rs.standard_normal((N, 1, S, S))).astype(np.float32)
    for n in range(N):
        for y in range(0, S, 3):
            for x in range(0, S, 3):
                if regions[n] is None or regions[n](x):
                    m[n, 0, y, x] = 1.5 * rs.standard_normal()
    return m


def pair_case(seed, S, K, count, tag_sd, regions_tl, regions_br):
    rs = np.random.RandomState(seed)
    N = 2
    tl, br = lattice_map(rs, N, S, regions_tl), lattice_map(rs, N, S, regions_br)
    tl_tag = np.stack([(sd * rs.standard_normal((1, S, S))).astype(np.float32) for sd in tag_sd])
    br_tag = np.stack([(sd * rs.standard_normal((1, S, S))).astype(np.float32) for sd in tag_sd])
    t = [torch.from_numpy(a) for a in (tl, br, tl_tag, br_tag)]
    det = ref.decodeCornerNet(t[0], t[1], t[2], t[3], None, None, K=K, nmsKernelSize=3, avgEmbeddingThreshold=1,
                              detectionCount=count).numpy()
    out = {"tl": tl, "br": br, "tl_tag": tl_tag, "br_tag": br_tag, "det": det.astype(np.float32)}
    for name, m in (("tl", t[0]), ("br", t[1])):
        s, i, _, y, x = extractTopK(nonMaximumSuppression(torch.sigmoid(m), kernelSize=3), K=K)
        assert (s > 0).all()
        out[name + "_scores"], out[name + "_inds"] = s.numpy(), i.numpy().astype(np.int64)
        out[name + "_ys"], out[name + "_xs"] = y.numpy().astype(np.int64), x.numpy().astype(np.int64)
    # every survivor, not only the first `count`: a tie across the cut would be as unordered as one inside it
    every = ref.decodeCornerNet(t[0], t[1], t[2], t[3], None, None, K=K, nmsKernelSize=3, avgEmbeddingThreshold=1,
                                detectionCount=K * K).numpy()
    nvalid, nall = [], []
    for n in range(N):
        v = every[n, :, 4][every[n, :, 4] >= 0]
        if len(np.unique(v)) != len(v):
            return None                                             # a tie among the survivors: draw again
        nall.append(len(v))
        nvalid.append(int((det[n, :, 4] >= 0).sum()))
        assert nvalid[-1] == min(len(v), count)
    out["nvalid"], out["nall"] = np.asarray(nvalid, np.int32), np.asarray(nall, np.int32)
    return out


def pair_cases():
    out = {}
    specs = {"small": (16, 8, 64, (0.5, 0.5), (None, lambda x: x >= 9), (None, lambda x: x <= 6)),
             "large": (32, 100, 1000, (0.5, 3.0), (None, None), (None, None))}
    for name, (S, K, count, sd, rtl, rbr) in specs.items():
        seed = 100
        while True:
            c = pair_case(seed, S, K, count, sd, rtl, rbr)
            if c is not None:
                break
            seed += 1
        print("pair case %s: seed %d, surviving pairs %s (rows %s of %d)" % (name, seed, c["nall"].tolist(),
                                                                          c["nvalid"].tolist(), count))
        for k, v in c.items():
            out["pair|%s|%s" % (name, k)] = v
        out["pair|%s|K" % name] = np.int32(K)
        out["pair|%s|count" % name] = np.int32(count)
    assert out["pair|small|nvalid"][0] > 0 and out["pair|small|nvalid"][1] == 0
    assert out["pair|large|nall"][0] > 1000 and 0 < out["pair|large|nall"][1] < 1000
    return out


def main():
    out = loss_cases()
    out.update(pair_cases())
    np.savez_compressed(os.path.join(HERE, "ae.npz"), **out)
    print("ae fixtures written: %d arrays" % len(out))


if __name__ == "__main__":
    main()
