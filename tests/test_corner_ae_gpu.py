"""cornerNetAE on the GPU: the embedding loss and the corner pairing against the reference's own results
(tests/golden/ae.npz, written by tests/golden/make_golden_ae.py from models/losses/embeddings.py and
models/cornerNetLegacy.py:332-446), the corner cell indices against the dataset's host rule, the two-head HeadsFn with
a sparse tag gradient against torch autograd in float64, the model against cornerNetCPool, and the dataset routes.

Tolerances.  Loss: per quantity 4 x the fixture's own |float32 run - float64 run| + 8 float32 ulps of the quantity's
largest magnitude, against the float64 run (the kernel sums in float64, so it may not be further away than the
reference's float32 arithmetic; the ulp floor covers quantities on which the two reference runs agree).  Pairing: exact.
Sparse against dense heads backward and HeadsFn against float64 autograd: 1e-5 of each gradient's scale, the fp32
bound of tests/test_sparse_heads_gpu.py."""
import random

import numpy as np
import pytest
import torch

from oracle import scd_archive

pytestmark = pytest.mark.gpu
DEV = "cuda"
H = 16          # the loss tests' map side


def _tol(r32, r64):
    r32, r64 = np.asarray(r32, np.float64), np.asarray(r64, np.float64)
    return 4 * np.abs(r32 - r64) + 8 * np.spacing(np.float32(np.abs(r64).max()))


def _focal_inputs(N, g):
    maps = [torch.randn(N, 1, H, H, generator=g).to(DEV).requires_grad_(True) for _ in range(3)]
    gts = [torch.rand(N, 1, H, H, generator=g).to(DEV) for _ in range(3)]
    return maps, gts


def _tag_maps(tags, inds, g):
    """(N,1,H,H) maps of noise with tags[b][k] at pixel inds[b][k]."""
    m = torch.randn(tags.shape[0], H * H, generator=g)
    m.scatter_(1, inds, tags)
    return m.view(-1, 1, H, H).to(DEV).requires_grad_(True)


def _distinct_inds(N, K, g):
    return torch.stack([torch.randperm(H * H, generator=g)[:K] for _ in range(N)])


def _ae(tl_map, br_map, tl_inds, br_inds, valid, seed=0):
    """CornerNetAELossFn on the tag maps -> (stats, tl_map.grad, br_map.grad)."""
    from scdhip.loss import CornerNetAELossFn
    g = torch.Generator().manual_seed(seed)
    maps, gts = _focal_inputs(tl_map.shape[0], g)
    loss, stats = CornerNetAELossFn.apply(*maps, tl_map, br_map, *gts, tl_inds.to(DEV), br_inds.to(DEV), valid.to(DEV),
                                          1, 1)
    assert loss.shape == (1,)
    loss.backward()
    torch.cuda.synchronize()
    assert abs(loss.item() - stats.sum().item()) <= 1e-5 * max(1.0, abs(loss.item()))
    return stats.cpu(), tl_map.grad.cpu(), br_map.grad.cpu()


# ------------------------------------------------------------------------------------------- 1: loss vs the reference

@pytest.mark.parametrize("case", ["mixed", "equal", "single"])
def test_embedding_loss_matches_reference(golden, case):
    f = golden("ae")
    get = lambda k: f["loss|%s|%s" % (case, k)]         # noqa: E731
    tl, br, valid = torch.from_numpy(get("tl")), torch.from_numpy(get("br")), torch.from_numpy(get("mask")).bool()
    N, K = tl.shape
    g = torch.Generator().manual_seed(3)
    tl_inds, br_inds = _distinct_inds(N, K, g), _distinct_inds(N, K, g)
    stats, g_tl, g_br = _ae(_tag_maps(tl, tl_inds, g), _tag_maps(br, br_inds, g), tl_inds, br_inds, valid)
    for name, got in (("pull", stats[3].item()), ("push", stats[4].item())):
        err, tol = abs(got - float(get(name + "64"))), _tol(get(name + "32"), get(name + "64"))
        print("%s %s: kernel %.9g reference64 %.17g |diff| %.3g tolerance %.3g" % (case, name, got,
                                                                                    float(get(name + "64")), err, tol))
        assert err <= tol, (name, got, err, tol)
    for name, gmap, inds in (("gtl", g_tl, tl_inds), ("gbr", g_br, br_inds)):
        got = gmap.view(N, -1).gather(1, inds).double().numpy()
        err, tol = np.abs(got - get(name + "64")), _tol(get(name + "32"), get(name + "64"))
        print("%s %s: worst |diff| %.3g, tolerance there %.3g" % (case, name, err.max(), tol.flat[err.argmax()]))
        assert (err <= tol).all(), (name, err.max())
        on = torch.zeros(N, H * H, dtype=torch.bool).scatter_(1, inds, valid)
        assert (gmap.view(N, -1)[~on] == 0).all(), name + ": nonzero off the gathered pixels"


# ------------------------------------------------------------------------------------------- 2: a shared corner cell

def _ae_torch(e_tl, e_br, valid):
    """The issue's formulas in plain torch on gathered tags (N,K) (float64 leaves) -> pull + push."""
    total = 0
    for b in range(e_tl.shape[0]):
        v = valid[b]
        n = int(v.sum())
        if n == 0:
            continue
        a, c = e_tl[b][v], e_br[b][v]
        m = (a + c) / 2
        nf = float(np.float32(n) + np.float32(1e-4))
        pull = (((a - m) ** 2).sum() + ((c - m) ** 2).sum()) / nf
        d = torch.relu(1 - (m[None, :] - m[:, None]).abs())
        push = ((d - float(np.float32(1) / np.float32(nf))) / float(np.float32((n - 1) * n) + np.float32(1e-4))).sum()
        total = total + pull + push
    return total


def test_shared_corner_cell_sums_and_is_deterministic():
    g = torch.Generator().manual_seed(9)
    K = 6
    tl_inds = torch.tensor([[5, 40, 5, 77, 130, 0]])            # slots 0 and 2 share cell 5; slot 5 is invalid
    br_inds = torch.tensor([[90, 200, 91, 255, 17, 0]])
    valid = torch.tensor([[True, True, True, True, True, False]])
    tl_host, br_host = 0.6 * torch.randn(1, H * H, generator=g), 0.6 * torch.randn(1, H * H, generator=g)
    runs = []
    for _ in range(2):
        tl_map = tl_host.view(1, 1, H, H).to(DEV).requires_grad_(True)
        br_map = br_host.view(1, 1, H, H).to(DEV).requires_grad_(True)
        runs.append(_ae(tl_map, br_map, tl_inds, br_inds, valid))
    assert torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][2], runs[1][2])
    e_tl = tl_host.double().gather(1, tl_inds).requires_grad_(True)
    e_br = br_host.double().gather(1, br_inds).requires_grad_(True)
    _ae_torch(e_tl, e_br, valid).backward()
    got = runs[0][1].view(-1)
    want = (e_tl.grad[0, 0] + e_tl.grad[0, 2]).item()
    tol = 8 * np.spacing(np.float32(e_tl.grad.abs().max().item()))
    print("shared cell: map %.9g, slot gradients %.9g + %.9g" % (got[5].item(), e_tl.grad[0, 0], e_tl.grad[0, 2]))
    assert abs(got[5].item() - want) <= tol
    for k in (1, 3, 4):
        assert abs(got[tl_inds[0, k]].item() - e_tl.grad[0, k].item()) <= tol
    assert got[0] == 0          # the invalid slot's pixel


# ------------------------------------------------------------------------------------------- 3: certificate

def _ae_model(dtype=torch.float32, seed=0):
    import trainer.model.cornerNetAE as plugin
    torch.manual_seed(seed)
    m = plugin.model(**plugin.modelParams)
    return m.to(DEV).train().set_compute_dtype(dtype), plugin


def _ae_targets(B, S, K, seed):
    """[heat, mask, regr, tl, br, tl_inds, br_inds, valid] on an S x S map: a repeated cell, an image corner, border
    cells with overlapping 3x3 reach, and invalid slots (index 0)."""
    g = torch.Generator().manual_seed(seed)
    maps = [(torch.rand(B, 1, S, S, generator=g) > 0.99).float() for _ in range(3)]
    valid = torch.arange(K)[None, :] < torch.randint(K // 2, K, (B, 1), generator=g)
    inds = []
    for _ in range(2):
        i = torch.randint(0, S * S, (B, K), generator=g)
        i[:, 1] = i[:, 0]
        i[:, 2] = S * S - 1
        i[:, 3] = S - 1
        i[:, 4] = i[:, 3] + S
        inds.append(i * valid)
    return [t.to(DEV) for t in (maps[0], valid, torch.zeros(B, K, 6), maps[1], maps[2], inds[0], inds[1], valid)]


def _rel(a, b):
    a, b = a.double(), b.double()
    return (a - b).abs().max().item() / max(1e-12, b.abs().max().item())


def test_tag_gradient_certificates_and_sparse_matches_dense():
    from scdhip import blocks, ops
    m, plugin = _ae_model()
    state = {k: v.clone() for k, v in m.state_dict().items()}
    x = torch.randn(2, 1, 128, 128, generator=torch.Generator().manual_seed(1)).to(DEV)
    ys = _ae_targets(2, 32, 8, 4)
    taken, orig = [], blocks.HeadsFn._backward_sparse

    def spy(*a, **k):
        taken.append(a[4])
        return orig(*a, **k)

    def run(sparse):
        seen = {}
        prev = ops.SparseHeads.enabled
        ops.SparseHeads.enabled = sparse
        blocks.HeadsFn._backward_sparse = staticmethod(spy)
        try:
            m.load_state_dict(state)
            m.zero_grad(set_to_none=False)
            feat = m.backbone_forward(x)
            feat.retain_grad()
            outs = m.heads_forward(feat)
            for name in ("tlTag", "brTag"):
                outs[name].register_hook(lambda g, name=name: seen.__setitem__(name, ops.sparse_grad_inds(g)))
            loss, _ = plugin.loss([outs], ys)
            loss.backward()
            torch.cuda.synchronize()
        finally:
            ops.SparseHeads.enabled = prev
            blocks.HeadsFn._backward_sparse = staticmethod(orig)
        grads = {n: p.grad.detach().clone() for n, p in m.named_parameters()}
        grads["dfeat"] = feat.grad.detach().clone()
        return grads, seen, loss.item()

    gs, seen, ls = run(True)
    assert torch.equal(seen["tlTag"], ys[5]) and torch.equal(seen["brTag"], ys[6])
    assert taken == [1, 1]                          # both corners: heat tail dense, tag tail over the gathered cells
    slotmap, ownermap = ops.sparse_maps(torch.device(DEV, torch.cuda.current_device()), 2 * 32 * 32)
    assert (slotmap == -1).all() and (ownermap == 0x7fffffff).all()
    gd, seen_d, ld = run(False)
    assert seen_d["tlTag"] is None and seen_d["brTag"] is None and taken == [1, 1]
    assert abs(ls - ld) <= 1e-6 * max(1.0, abs(ld))
    assert all(g.abs().max() > 0 for n, g in gd.items() if "Tag" in n)
    worst = max((_rel(gs[n], gd[n]), n) for n in gd)
    print("fp32: worst relative gradient difference sparse vs dense %.2e (%s)" % worst)
    assert worst[0] < 1e-5, worst


# ------------------------------------------------------------------------------------------- 4: two-head HeadsFn

def test_two_head_headsfn_sparse_tag_gradient_matches_float64_autograd():
    from models.cornerNetCPool import makeResnetTerminal
    from scdhip import blocks, ops
    g = torch.Generator().manual_seed(21)
    N, S, C, K = 2, 32, 256, 8
    heads = [makeResnetTerminal(C, 128, 1).to(DEV), makeResnetTerminal(C, 128, 1).to(DEV)]
    feat = torch.randn(N, S, S, C, generator=g).to(DEV).requires_grad_(True)
    inds = torch.stack([torch.randperm(S * S, generator=g)[:K] for _ in range(N)])
    inds[:, 1] = inds[:, 0]                                     # a duplicate pixel
    inds[:, 2] = S - 1                                          # a border pixel
    slot_g = torch.randn(N, K, generator=g)
    slot_g[:, 7] = 0                                            # an invalid slot: index 0, no gradient
    inds[:, 7] = 0
    d0 = torch.randn(N, 1, S, S, generator=g)
    d1 = torch.zeros(N, S * S).scatter_add_(1, inds, slot_g).view(N, 1, S, S)
    taken, orig = [], blocks.HeadsFn._backward_sparse

    def spy(*a, **k):
        taken.append(a[4])
        return orig(*a, **k)
    blocks.HeadsFn._backward_sparse = staticmethod(spy)
    try:
        outs = blocks.HeadsFn.apply(feat, heads[0][0].weight, heads)
        d1_dev = d1.to(DEV)
        ops.clear_sparse_grads()
        ops.certify_sparse_grad(d1_dev, inds.to(DEV))
        torch.autograd.backward(outs, [d0.to(DEV), d1_dev])
        torch.cuda.synchronize()
    finally:
        blocks.HeadsFn._backward_sparse = staticmethod(orig)
        ops.clear_sparse_grads()
    assert taken == [1]
    x64 = feat.detach().cpu().double().permute(0, 3, 1, 2).requires_grad_(True)
    want = {}
    for i, (h, d) in enumerate(zip(heads, (d0, d1))):
        p = [t.detach().cpu().double().requires_grad_(True) for t in (h[0].weight, h[0].bias, h[2].weight, h[2].bias)]
        hid = torch.relu(torch.nn.functional.conv2d(x64, p[0], p[1], padding=1))
        out = torch.nn.functional.conv2d(hid, p[2], p[3])
        np.testing.assert_allclose(outs[i].detach().cpu().numpy(), out.detach().numpy(), rtol=1e-4, atol=1e-4)
        out.backward(d.double())
        for name, t in zip(("w0", "b0", "w1", "b1"), p):
            want["%d.%s" % (i, name)] = t.grad
    got = {"%d.%s" % (i, name): t.grad.cpu()
           for i, h in enumerate(heads)
           for name, t in zip(("w0", "b0", "w1", "b1"), (h[0].weight, h[0].bias, h[2].weight, h[2].bias))}
    got["dfeat"], want["dfeat"] = feat.grad.cpu().permute(0, 3, 1, 2), x64.grad
    rows = sorted(((_rel(got[n], want[n]), n) for n in want), reverse=True)
    for r in rows:
        print("HeadsFn vs float64 autograd: %.2e  %s" % r)
    assert rows[0][0] < 1e-5, rows[0]


# ------------------------------------------------------------------------------------------- 5, 6: pairing

def _pairs_from_fixture(f, case):
    from scdhip import ops
    get = lambda k: torch.from_numpy(f["pair|%s|%s" % (case, k)]).to(DEV)       # noqa: E731
    tl = tuple(get("tl_" + k) for k in ("scores", "inds", "ys", "xs"))
    br = tuple(get("br_" + k) for k in ("scores", "inds", "ys", "xs"))
    return ops.corner_pairs(tl, br, get("tl_tag"), get("br_tag"), threshold=1.0, count=int(f["pair|%s|count" % case]))


@pytest.mark.parametrize("case", ["small", "large"])
def test_corner_pairs_match_reference(golden, case):
    f = golden("ae")
    det, nvalid = _pairs_from_fixture(f, case)
    want = torch.from_numpy(f["pair|%s|det" % case])
    assert det.shape == want.shape and det.dtype == torch.float32
    det, nvalid = det.cpu(), nvalid.cpu()
    assert nvalid.tolist() == f["pair|%s|nvalid" % case].tolist()
    for b in range(det.shape[0]):
        n = int((want[b, :, 4] >= 0).sum())
        assert nvalid[b] == n
        assert torch.equal(det[b, :n], want[b, :n]), b
        assert (det[b, n:, 4] == -1).all() and (det[b, n:, :4] == 0).all() and (det[b, n:, 5:] == 0).all()
    if case == "small":
        assert nvalid[1] == 0       # the image whose br peaks all lie left of its tl peaks


@pytest.mark.parametrize("K,count", [(8, 64), (100, 1000), (128, 1024)])
def test_corner_pairs_tie_rule(K, count):
    """Scores from {0.25, 0.5, 0.75}: many equal pair scores, inside the kept rows and across the cut.  The order is
    score descending, then flat index i*K + j ascending: a stable sort of the survivors in flat order."""
    from scdhip import ops
    g = torch.Generator().manual_seed(K)
    N, S = 2, 32
    lv = torch.tensor([0.25, 0.5, 0.75])
    mk = lambda: (lv[torch.randint(0, 3, (N, K), generator=g)], torch.randint(0, S * S, (N, K), generator=g))   # noqa
    (s_tl, i_tl), (s_br, i_br) = mk(), mk()
    tags = [torch.randn(N, 1, S, S, generator=g) for _ in range(2)]
    tl = (s_tl, i_tl, i_tl // S, i_tl % S)
    br = (s_br, i_br, i_br // S, i_br % S)
    det, nvalid = ops.corner_pairs(tuple(t.to(DEV) for t in tl), tuple(t.to(DEV) for t in br), tags[0].to(DEV),
                                   tags[1].to(DEV), threshold=1.0, count=count)
    det, nvalid = det.cpu(), nvalid.cpu()
    D = min(count, K * K)
    assert det.shape == (N, D, 8)
    for b in range(N):
        t_tl, t_br = tags[0][b].view(-1)[i_tl[b]], tags[1][b].view(-1)[i_br[b]]
        score = ((s_tl[b][:, None] + s_br[b][None, :]) * 0.5).reshape(-1)
        bad = (((t_tl[:, None] - t_br[None, :]).abs() > 1.0) | (br[3][b][None, :] < tl[3][b][:, None])
               | (br[2][b][None, :] < tl[2][b][:, None])).reshape(-1)
        flat = torch.nonzero(~bad).view(-1)
        flat = flat[torch.sort(-score[flat], stable=True)[1]][:D]
        i, j = flat // K, flat % K
        want = torch.stack([tl[3][b][i].float(), tl[2][b][i].float(), br[3][b][j].float(), br[2][b][j].float(),
                            score[flat], s_tl[b][i], s_br[b][j], torch.zeros(len(flat))], 1)
        assert nvalid[b] == len(flat) and len(flat) > 0
        assert torch.equal(det[b, :len(flat)], want), b
        assert (det[b, len(flat):, 4] == -1).all()


def test_corner_pairs_limits():
    from scdhip import ops
    z = torch.zeros(1, 130, device=DEV)
    zi = z.long()
    tag = torch.zeros(1, 1, 16, 16, device=DEV)
    with pytest.raises(ValueError):
        ops.corner_pairs((z, zi, zi, zi), (z, zi, zi, zi), tag, tag)
    with pytest.raises(ValueError):
        ops.corner_pairs((z[:, :64], zi[:, :64], zi[:, :64], zi[:, :64]), (z[:, :64], zi[:, :64], zi[:, :64], zi[:, :64]),
                         tag, tag, count=1025)


# ------------------------------------------------------------------------------------------- 7: corner_tag_inds

def test_corner_tag_inds_match_dataset_rule_and_renderer():
    from scdhip import ops
    from trainer.dataset import syntheticCorner as SC
    from trainer.dataset.syntheticSCD import THRESHOLDIOU
    ds = SC.dataset(None, True)
    _, locs, counts = ds.batch_rows(list(range(8)))
    locs = locs.clone()
    counts = counts.clone()
    counts[0] = max(int(counts[0]), 3)
    locs[0, 0] = torch.tensor([200.0, 40.0, 0, 0, 3.0, 1.0, 2.0, 4.0])     # a centre off the map
    locs[0, 1] = torch.tensor([40.5, -3.0, 0, 0, 3.0, 1.0, 2.0, 4.0])      # ... above it
    locs[0, 2] = torch.tensor([60.2, 70.9, 0, 0, float("nan"), 1.0, 2.0, 4.0])      # a NaN row
    dl, dc = locs.to(DEV), counts.to(DEV)
    before = ops.render_corner_targets(dl, dc, ds.heat, THRESHOLDIOU)
    tl_inds, br_inds, valid = ops.corner_tag_inds(dl, dc, ds.heat)
    after = ops.render_corner_targets(dl, dc, ds.heat, THRESHOLDIOU)
    for a, b in zip(before, after):         # (a NaN row renders NaNs: compared as a value of their own)
        if a.is_floating_point():
            a, b = a.nan_to_num(nan=-7.0), b.nan_to_num(nan=-7.0)
        assert torch.equal(a, b)
    assert tl_inds.dtype == torch.int64 and valid.dtype == torch.bool and tl_inds.shape == (8, locs.shape[1])
    tl_inds, br_inds, valid = tl_inds.cpu(), br_inds.cpu(), valid.cpu()
    assert not valid[0, :3].any()
    for b in range(8):
        n = int(counts[b])
        assert not valid[b, n:].any()
        assert (tl_inds[b][~valid[b]] == 0).all() and (br_inds[b][~valid[b]] == 0).all()
        tl, br = SC.corner_locs(locs[b, :n].numpy(), ds.heat)
        for k in range(n):
            if b == 0 and k < 3:
                continue
            assert valid[b, k]
            assert tl_inds[b, k] == int(tl[k, 1]) * ds.heat + int(tl[k, 0])
            assert br_inds[b, k] == int(br[k, 1]) * ds.heat + int(br[k, 0])
        h_tl, h_br, h_v = SC.corner_tag_inds(locs[b, :n].numpy(), ds.heat)
        assert np.array_equal(h_tl, tl_inds[b].numpy()) and np.array_equal(h_br, br_inds[b].numpy())
        assert np.array_equal(h_v, valid[b].numpy())
    # the rendered corner maps peak at exactly those cells (a batch with no zero major axis and no NaN row)
    _, locs, counts = ds.batch_rows(list(range(8, 16)))
    dl, dc = locs.to(DEV), counts.to(DEV)
    ys = ops.render_corner_targets(dl, dc, ds.heat, THRESHOLDIOU)
    tl_inds, br_inds, valid = ops.corner_tag_inds(dl, dc, ds.heat)
    assert valid.sum() == counts.sum()
    assert (ys[3].flatten(1).gather(1, tl_inds)[valid] == 1).all()
    assert (ys[4].flatten(1).gather(1, br_inds)[valid] == 1).all()


# ------------------------------------------------------------------------------------------- 8: model

def test_model_shares_cornernetcpool_parameters_and_outputs():
    from models.cornerNetAE import CornerNetAEResidual
    from models.cornerNetCPool import CornerNetResidual
    torch.manual_seed(3)
    base = CornerNetResidual(10)
    torch.manual_seed(3)
    ae = CornerNetAEResidual(10)
    sb, sa = base.state_dict(), ae.state_dict()
    assert list(sa.keys())[:len(sb)] == list(sb.keys())
    assert sorted(set(sa) - set(sb)) == sorted("%s.%d.%s" % (t, i, p) for t in ("tlTag", "brTag") for i in (0, 2)
                                               for p in ("weight", "bias"))
    for k, v in sb.items():
        assert torch.equal(v, sa[k]), k
    assert not (sa["tlTag.2.bias"] == -2.19).any()
    base, ae = base.to(DEV).train(), ae.to(DEV).train()
    x = torch.randn(2, 1, 128, 128, generator=torch.Generator().manual_seed(8)).to(DEV)
    with torch.no_grad():
        ob, oa = base(x, decode=False)[0], ae(x, decode=False)[0]
    assert list(oa.keys()) == ["heatmap", "tl", "br", "tlTag", "brTag"]
    for k, v in oa.items():
        assert v.shape == (2, 1, 32, 32) and v.dtype == torch.float32, k
    for k in ("heatmap", "tl", "br"):
        assert torch.equal(ob[k], oa[k]), k
    assert oa["tlTag"].abs().max() > 0 and not torch.equal(oa["tlTag"], oa["brTag"])


# ------------------------------------------------------------------------------------------- 9: training

def _embeddings_on():
    from configuration import defaultConfig
    old = dict(defaultConfig.config)
    defaultConfig.config.update({"cornerTargets": True, "cornerEmbeddings": True})
    return old


def _restore(old):
    from configuration import defaultConfig
    defaultConfig.config.clear()
    defaultConfig.config.update(old)


def test_bf16_training_reduces_loss_and_validation_line_prints():
    from models.cornerNetAE import cornerNetAEEvaluation, expression
    from scdhip.flat import FlatAdam
    from trainer.dataset import syntheticCorner as SC
    m, plugin = _ae_model(torch.bfloat16)
    old = _embeddings_on()
    try:
        batch = SC.dataset(None, True).gpu_batch([0, 1, 2, 3], DEV)
    finally:
        _restore(old)
    xs, ys = batch["xs"], batch["ys"]
    assert len(ys) == 8
    opt = FlatAdam(m.parameters(), lr=1e-3)
    losses, emb = [], []
    for _ in range(20):
        opt.zero_grad()
        loss, stats = plugin.loss(m(*xs, decode=False), ys)
        assert stats == {}
        loss.sum().backward()
        opt.step()
        losses.append(loss.item())
        emb.append(plugin.loss.last_stats[3:5].sum().item())
    print("loss", ["%.4f" % v for v in losses])
    print("pull + push", ["%.4f" % v for v in emb])
    assert np.isfinite(losses).all() and np.isfinite(emb).all()
    assert np.mean(losses[-5:]) < np.mean(losses[:5]), losses
    assert np.mean(emb[-5:]) < np.mean(emb[:5]), emb
    with torch.no_grad():
        dec = m(*xs, decode=True)
    det, nvalid = dec[0], dec[1]
    assert det.shape == (4, 1000, 8) and nvalid.shape == (4,) and len(dec) == 7 and dec[-1]["tlTag"].shape[1] == 1
    ev, od = cornerNetAEEvaluation(xs, ys, *dec)
    assert od is dec[-1] and ev["counts"].shape == (6,) and ev["counts"].is_cuda
    line = expression([ev, ev])
    print(line)
    for field in ("[Obj]", "[Det]", "[mIoU]", "[Rec50]", "[Rec75]", "[Prec50]"):
        assert field in line
    assert int(line.split("[Obj]")[1].split()[0]) == 2 * int(ys[7].sum())
    # detections that are the ground-truth boxes themselves score full marks
    W = ys[0].shape[-1]
    gt = torch.stack([ys[5] % W, ys[5] // W, ys[6] % W, ys[6] // W], -1).float()
    perfect = torch.cat([gt, ys[7].float()[..., None] * 2 - 1, torch.zeros(*gt.shape[:2], 3, device=DEV)], -1)
    c = cornerNetAEEvaluation(xs, ys, perfect, None, None)[0]["counts"].tolist()
    assert c[0] == c[1] == c[2] == c[3] == c[4] == c[5] == float(ys[7].sum())


# ------------------------------------------------------------------------------------------- 10: datasets

COUNT = 7680      # tests/test_corner_targets_gpu.py's archive: 20 synthetic slides of 8 x 8 tiles


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    from configuration import defaultConfig
    from trainer.dataset import scdx16p100 as D
    d = tmp_path_factory.mktemp("scdae")
    path = str(d / "synthetic.d")
    scd_archive.write(path, count=COUNT, size=8)
    old = dict(defaultConfig.config)
    defaultConfig.config.update({"dirTemp": str(d / "temp") + "/", "dirDataSplitProfile": str(d / "split.json"),
                                 "cornerTargets": True, "cornerEmbeddings": True})
    try:
        random.seed(77)
        ds = D.SCD(path, True, None)
    finally:
        _restore(old)
    return ds


def _d_batch(ds, embeddings, resident=False):
    from configuration import defaultConfig
    old = dict(defaultConfig.config)
    defaultConfig.config.update({"cornerTargets": True, "cornerEmbeddings": embeddings, "rotateAugmentation": 0.0,
                                 "residentDataset": resident})
    ds.order.sort()
    random.seed(5)
    np.random.seed(6)
    torch.manual_seed(7)
    try:
        return ds.gpu_batch(list(range(32)))["ys"]
    finally:
        _restore(old)


def test_synthetic_corner_layouts():
    from configuration import defaultConfig
    from trainer.dataset import syntheticCorner as SC
    assert not defaultConfig.cornerEmbeddings
    ds = SC.dataset(None, True)
    off = ds.gpu_batch([0, 1, 2, 3], DEV)["ys"]
    assert len(off) == 5 and len(ds[0]["ys"]) == 5 and len(ds.getValidationSet(batch=32)[0]["ys"]) == 5
    old = _embeddings_on()
    try:
        on = ds.gpu_batch([0, 1, 2, 3], DEV)["ys"]
        item = ds[1]["ys"]
        vs = ds.getValidationSet(batch=32)
    finally:
        _restore(old)
    assert len(on) == 8 and len(item) == 8
    for a, b in zip(off, on):
        assert torch.equal(a, b)
    for k in (5, 6, 7):         # the host item states the same cells and slots
        assert torch.equal(on[k][1].cpu(), item[k]), k
    assert len(vs) == 2 and [tuple(t.shape) for t in vs[0]["ys"][5:]] == [(32, 30)] * 3
    assert vs[0]["ys"][7].dtype == torch.bool and vs[0]["ys"][5].dtype == torch.int64


def test_d_archive_layouts_host_and_resident(built):
    off = _d_batch(built, False)
    on = _d_batch(built, True)
    res = _d_batch(built, True, resident=True)
    assert len(off) == 5 and len(on) == 8 and len(res) == 8
    for a, b in zip(off, on):
        assert torch.equal(a, b)
    for k, (a, b) in enumerate(zip(on, res)):
        assert torch.equal(a, b), k
    assert on[7].any() and (on[3].flatten(1).gather(1, on[5])[on[7]] == 1).all()
    from configuration import defaultConfig
    old = _embeddings_on()
    try:
        vs = built.getValidationSet()
    finally:
        _restore(old)
    assert len(vs[0]["ys"]) == 8 and vs[0]["ys"][5].shape == vs[0]["ys"][1].shape
    old = dict(defaultConfig.config)
    defaultConfig.config.update({"cornerTargets": False, "cornerEmbeddings": True})
    try:
        with pytest.raises(RuntimeError, match="cornerTargets"):
            built.gpu_batch([1, 2])
    finally:
        _restore(old)


def test_d_validation_set_built_without_the_key_raises(tmp_path):
    from configuration import defaultConfig
    from trainer.dataset import scdx16p100 as D
    path = str(tmp_path / "synthetic.d")
    scd_archive.write(path, count=COUNT, size=8)
    old = dict(defaultConfig.config)
    defaultConfig.config.update({"dirTemp": str(tmp_path / "temp") + "/",
                                 "dirDataSplitProfile": str(tmp_path / "split.json"), "cornerTargets": True})
    try:
        random.seed(77)
        ds = D.SCD(path, True, None)
        defaultConfig.config["cornerEmbeddings"] = True
        with pytest.raises(RuntimeError, match="cornerEmbeddings"):
            ds.getValidationSet()
    finally:
        _restore(old)
