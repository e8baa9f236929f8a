"""Slide cohort quantification on the GPU (scd_slide_samples, slide.analyseSamples, quantify.main).

The checker is a numpy restatement of the rule written here: candidates = score > thr with the projected pixel in
the box; greedy de-duplication by descending score (ties by ascending flat index) against already-kept candidates
of a different clip, dx^2 + dy^2 <= radius^2 in integers; samples in flat order; bin floor((ratio - lo) * scale)
in float64.  Every comparison is exact (indices, xy, score, hist, counters), the ratio bit for bit: it is the same
float64 expression on both sides."""
import json

import numpy as np
import pytest
import torch

from oracle import slide_case

pytestmark = pytest.mark.gpu
DEV = "cuda"
LO, SCALE, NBINS = -0.25, 100.0, 150
REF_BOX = (0, 0, 3072, 2056)


def check_samples(dec, stride, pad_lr, pad_tb, clip_v, thr, box, radius, lo=LO, scale=SCALE, nbins=NBINS):
    dec = np.asarray(dec, np.float32)
    _, T, K = dec.shape
    flat = np.arange(T * K)
    t = flat // K
    i, j = t // clip_v, t % clip_v
    f = [dec[r].reshape(-1).astype(np.float64) for r in range(10)]
    score = dec[0].reshape(-1)
    px = np.trunc((i * stride - pad_lr).astype(np.float64) + f[3] * 4.0 + f[8]).astype(np.int64)
    py = np.trunc((j * stride - pad_tb).astype(np.float64) + f[2] * 4.0 + f[9]).astype(np.int64)
    with np.errstate(all="ignore"):
        minl, halo = f[6] * 4.0, f[7] * 4.0
        ratio = (halo - minl) / (2.0 * minl)
    above = score > np.float32(thr)
    x0, y0, x1, y1 = box
    valid = above & (px >= x0) & (px < x1) & (py >= y0) & (py < y1)
    cand = flat[valid]
    kept = np.zeros(T * K, bool)
    if radius < 0:
        kept[cand] = True
    else:
        order = cand[np.lexsort((cand, -score[cand].astype(np.float64)))]
        kx, ky, kt, m = np.zeros(cand.size, np.int64), np.zeros(cand.size, np.int64), np.zeros(cand.size, np.int64), 0
        for q in order:
            d2 = (kx[:m] - px[q]) ** 2 + (ky[:m] - py[q]) ** 2
            if np.any((kt[:m] != t[q]) & (d2 <= radius * radius)):
                continue
            kept[q] = True
            kx[m], ky[m], kt[m] = px[q], py[q], t[q]
            m += 1
    idx = flat[kept]
    r = ratio[idx]
    with np.errstate(all="ignore"):
        b = np.floor((r - lo) * scale)
        binned = np.isfinite(r) & (b >= 0) & (b < nbins)
    hist = np.bincount(b[binned].astype(np.int64), minlength=nbins).astype(np.int64)
    counters = np.array([above.sum(), valid.sum(), idx.size, binned.sum(), idx.size - binned.sum()], np.int64)
    return dict(index=idx.astype(np.int32), xy=np.stack([px[idx], py[idx]], 1).astype(np.int32), ratio=r,
                score=score[idx], hist=hist, counters=counters)


def run_samples(dec, stride, pad_lr, pad_tb, clip_v, thr, box, radius, hist=None, counters=None, lo=LO, scale=SCALE,
                nbins=NBINS):
    from scdhip import ops
    if hist is None:
        hist = torch.zeros(nbins, dtype=torch.int64, device=DEV)
    if counters is None:
        counters = torch.zeros(5, dtype=torch.int64, device=DEV)
    d = torch.from_numpy(np.asarray(dec, np.float32)).to(DEV)
    xy, ratio, score, index, count = ops.slide_samples(d, stride, pad_lr, pad_tb, clip_v, thr, box, radius, hist,
                                                       counters, lo=lo, scale=scale)
    n = int(count.item())
    return dict(index=index[:n].cpu().numpy(), xy=xy[:n].cpu().numpy(), ratio=ratio[:n].cpu().numpy(),
                score=score[:n].cpu().numpy(), hist=hist.cpu().numpy(), counters=counters.cpu().numpy())


def assert_same(got, ref):
    np.testing.assert_array_equal(got["index"], ref["index"])
    np.testing.assert_array_equal(got["xy"], ref["xy"])
    np.testing.assert_array_equal(got["score"], ref["score"])
    assert got["ratio"].dtype == np.float64
    np.testing.assert_array_equal(got["ratio"].view(np.int64), ref["ratio"].view(np.int64))
    np.testing.assert_array_equal(got["hist"], ref["hist"])
    np.testing.assert_array_equal(got["counters"], ref["counters"])


def both(dec, *args, **kw):
    got, ref = run_samples(dec, *args, **kw), check_samples(dec, *args, **kw)
    assert_same(got, ref)
    return got


# ---------------------------------------------------------------- the recorded fixture

@pytest.fixture(scope="module")
def gold_dec(golden):
    return golden("slide")["decoded"]


@pytest.fixture(scope="module")
def geom():
    import slide
    return slide.geometry(slide_case.SLIDE_H, slide_case.SLIDE_W)


@pytest.mark.parametrize("radius", [-1, 0, 8, 16])
def test_recorded_fixture(gold_dec, geom, radius):
    assert gold_dec.shape == (10, 48, 100)
    got = both(gold_dec, 384, geom["padLR"], geom["padTB"], geom["clipV"], 0.3, REF_BOX, radius)
    c = got["counters"]
    assert c[0] >= c[1] >= c[2] == c[3] + c[4] and got["hist"].sum() == c[3]
    if radius >= 8:
        assert c[2] < c[1]          # the overlap bands do hold cross-clip pairs (100 within 8 px, 368 within 16)


def test_no_dedup_full_box_equals_slide_detections(gold_dec, geom):
    from scdhip import ops
    big = (-(1 << 30), -(1 << 30), 1 << 30, 1 << 30)
    got = run_samples(gold_dec, 384, geom["padLR"], geom["padTB"], geom["clipV"], 0.3, big, -1)
    xy, ratio = ops.slide_detections(torch.from_numpy(gold_dec).to(DEV), 384, geom["padLR"], geom["padTB"],
                                     geom["clipV"], 0.3)
    np.testing.assert_array_equal(got["xy"], xy.cpu().numpy())
    np.testing.assert_array_equal(got["ratio"].view(np.int64), ratio.cpu().numpy().view(np.int64))
    assert got["counters"][0] == got["counters"][1] == got["counters"][2] == xy.shape[0]


# ---------------------------------------------------------------- built stacks

def dense_stack(T, K, seed, lo_score, hi_score):
    """Clips 8 px apart with centres on a 16 x 16 map: many cross-clip neighbours within a few pixels."""
    rs = np.random.RandomState(seed)
    ys, xs = rs.randint(0, 16, (T, K)), rs.randint(0, 16, (T, K))
    minl = rs.uniform(0.5, 3, (T, K))
    rows = [rs.uniform(lo_score, hi_score, (T, K)), ys * 128 + xs, ys, xs, rs.uniform(-6, 6, (T, K)),
            rs.uniform(-6, 6, (T, K)), minl, minl + rs.uniform(0, 4, (T, K)), rs.uniform(0, 4, (T, K)),
            rs.uniform(0, 4, (T, K))]
    return np.stack(rows).astype(np.float32)


SHAPES = [(1, 1), (7, 9), (8, 8), (5, 13), (3, 43), (25, 41), (2, 64)]     # 1, 63, 64, 65, 129, 1025, 128 slots


@pytest.mark.parametrize("T,K", SHAPES)
@pytest.mark.parametrize("radius", [-1, 3])
def test_built_all_above(T, K, radius):
    dec = dense_stack(T, K, 100 + T * K, 0.31, 1.0)
    clip_v = 2 if T % 2 == 0 else 1
    box = (4, 4, 8 * T + 40, 60)
    got = both(dec, 8, 3, 2, clip_v, 0.3, box, radius)
    assert got["counters"][0] == T * K
    got = both(dec, 8, 3, 2, clip_v, 0.3, (-1000, -1000, 100000, 100000), radius)
    assert got["counters"][1] == T * K


@pytest.mark.parametrize("T,K", SHAPES)
def test_built_none_above(T, K):
    dec = dense_stack(T, K, 200 + T * K, 0.0, 0.3)
    hist = torch.arange(NBINS, dtype=torch.int64, device=DEV)
    counters = torch.arange(5, dtype=torch.int64, device=DEV) + 7
    got = run_samples(dec, 8, 3, 2, 1, 0.3, (-1000, -1000, 100000, 100000), 3, hist=hist, counters=counters)
    assert got["index"].size == 0
    np.testing.assert_array_equal(got["hist"], np.arange(NBINS))
    np.testing.assert_array_equal(got["counters"], np.arange(5) + 7)


def test_built_mixed_scores_with_ties():
    """Scores quantised to 8 levels: many equal scores, so the rank's tie rule decides most suppressions."""
    dec = dense_stack(25, 41, 5, 0.0, 1.0)
    dec[0] = np.floor(dec[0] * 8) / 8
    both(dec, 8, 3, 2, 5, 0.3, (0, 0, 200, 70), 2)
    both(dec, 8, 3, 2, 5, 0.3, (0, 0, 200, 70), 0)


# ---------------------------------------------------------------- hand-made cases

STRIDE = 1000


def hand_stack(T, K, items):
    """items: (clip, slot, score, x, y[, minl, halo]) at absolute pixels; clip t starts at x = 1000 t (clipV = 1)."""
    dec = np.zeros((10, T, K), np.float32)
    dec[6], dec[7] = 1.0, 1.5
    for it in items:
        t, k, s, x, y = it[:5]
        dec[0, t, k] = s
        dec[8, t, k] = x - STRIDE * t
        dec[9, t, k] = y
        if len(it) > 5:
            dec[6, t, k], dec[7, t, k] = it[5], it[6]
    return dec


def hand(T, K, items, radius, box=(0, 0, 10000, 10000)):
    return both(hand_stack(T, K, items), STRIDE, 0, 0, 1, 0.3, box, radius)


def test_tie_lower_flat_index_survives():
    got = hand(3, 4, [(2, 1, 0.5, 100, 100), (0, 3, 0.5, 100, 100), (1, 0, 0.5, 100, 100)], 0)
    assert got["index"].tolist() == [3]


def test_radius_edge():
    # (3, 4, 5): d^2 = 25 = r^2 is suppressed; d^2 = 26 = r^2 + 1 is kept
    got = hand(2, 2, [(0, 0, 0.9, 100, 100), (1, 0, 0.8, 103, 104)], 5)
    assert got["index"].tolist() == [0]
    got = hand(2, 2, [(0, 0, 0.9, 100, 100), (1, 0, 0.8, 101, 105)], 5)
    assert got["index"].tolist() == [0, 2]


@pytest.mark.parametrize("scores,kept", [((0.9, 0.8, 0.7), [0, 2]), ((0.8, 0.9, 0.7), [1]), ((0.7, 0.8, 0.9), [0, 2])])
def test_chain(scores, kept):
    # A (100), B (106), C (112) in three clips, radius 6: B is within r of both, A-C are 12 apart
    items = [(0, 0, scores[0], 100, 50), (1, 0, scores[1], 106, 50), (2, 0, scores[2], 112, 50)]
    got = hand(3, 1, items, 6)
    assert got["index"].tolist() == kept


def test_same_clip_neighbours_both_kept():
    got = hand(2, 3, [(1, 0, 0.9, 1100, 50), (1, 2, 0.8, 1101, 50)], 8)
    assert got["index"].tolist() == [3, 5]


def test_invalid_top_score_suppresses_nothing():
    # the best score lies outside the box, one pixel from a valid candidate of another clip
    got = hand(2, 1, [(0, 0, 0.99, 99, 50), (1, 0, 0.5, 100, 50)], 8, box=(100, 0, 10000, 10000))
    assert got["index"].tolist() == [1]
    np.testing.assert_array_equal(got["counters"], [2, 1, 1, 1, 0])


def test_non_finite_ratios_kept_not_binned():
    items = [(0, 0, 0.9, 10, 10, 0.0, 2.0), (0, 1, 0.8, 500, 10, 0.0, 0.0), (0, 2, 0.7, 900, 10, 1.0, 1.5),
             (0, 3, 0.6, 950, 10, 1.0, 9.0)]
    got = hand(1, 4, items, 8)
    assert got["index"].tolist() == [0, 1, 2, 3]
    assert np.isposinf(got["ratio"][0]) and np.isnan(got["ratio"][1])
    assert got["ratio"][2] == 0.25 and got["ratio"][3] == 4.0
    np.testing.assert_array_equal(got["counters"], [4, 4, 4, 1, 3])
    assert got["hist"].sum() == 1 and got["hist"][50] == 1


def test_accumulation(gold_dec, geom):
    args = (384, geom["padLR"], geom["padTB"], geom["clipV"], 0.3, REF_BOX)
    a = check_samples(gold_dec, *args, 8)
    b = check_samples(gold_dec[:, :20], *args, -1)
    hist = torch.zeros(NBINS, dtype=torch.int64, device=DEV)
    counters = torch.zeros(5, dtype=torch.int64, device=DEV)
    run_samples(gold_dec, *args, 8, hist=hist, counters=counters)
    got = run_samples(gold_dec[:, :20], *args, -1, hist=hist, counters=counters)
    np.testing.assert_array_equal(got["hist"], a["hist"] + b["hist"])
    np.testing.assert_array_equal(got["counters"], a["counters"] + b["counters"])
    np.testing.assert_array_equal(got["index"], b["index"])


def test_refusals():
    """Argument checks only: each call returns before any launch."""
    from scdhip import ops
    dec = torch.zeros(10, 2, 3, device=DEV)
    hist = torch.zeros(NBINS, dtype=torch.int64, device=DEV)
    counters = torch.zeros(5, dtype=torch.int64, device=DEV)
    for box in [(5, 0, 5, 10), (6, 0, 5, 10), (0, 3, 10, 3)]:
        with pytest.raises(RuntimeError, match="9001"):
            ops.slide_samples(dec, 384, 0, 0, 1, 0.3, box, -1, hist, counters)
    with pytest.raises(RuntimeError, match="9001"):
        ops.slide_samples(dec, 384, 0, 0, 1, 0.3, (0, 0, 10, 10), -1, hist[:0], counters)
    with pytest.raises(RuntimeError, match="9001"):
        ops.slide_samples(dec, 384, 0, 0, 1, 0.3, (0, 0, 10, 10), -1, torch.zeros(1025, dtype=torch.int64, device=DEV),
                          counters)
    with pytest.raises(RuntimeError, match="9001"):
        ops.slide_samples(dec, 384, 0, 0, 1, 0.3, (0, 0, 10, 10), -2, hist, counters)
    big = torch.zeros(10, 1, ops.SLIDE_SAMPLES_MAX + 1, device=DEV)
    with pytest.raises(RuntimeError, match="9001"):
        ops.slide_samples(big, 384, 0, 0, 1, 0.3, (0, 0, 10, 10), -1, hist, counters)
    assert int(hist.sum()) == 0 and int(counters.sum()) == 0


def test_cap_is_accepted():
    """T*K = 16384, every slot a candidate on a 40 x 40 px patch: the largest matrix the kernel builds."""
    from scdhip import ops
    assert ops.SLIDE_SAMPLES_MAX >= 16384
    dec = dense_stack(128, 128, 9, 0.31, 1.0)
    dec[[2, 3]] = np.random.RandomState(4).randint(0, 10, (2, 128, 128))
    got = both(dec, 1, 0, 0, 128, 0.3, (0, 0, 4000, 4000), 1)
    assert got["counters"][1] == 16384 and got["counters"][2] < 16384


# ---------------------------------------------------------------- end to end

def test_analyse_samples_end_to_end(gold_dec, geom):
    """slide.analyseSamples with the replaying stub model of test_analyse_array_end_to_end; the fit of its
    histogram is the fit of the checker's histogram, bit for bit."""
    import slide
    from scdhip import rhr
    dec = torch.from_numpy(gold_dec).to(DEV)
    state = {"at": 0, "shapes": []}

    def model(inp):
        state["shapes"].append(tuple(inp.shape))
        b = inp.shape[0]
        out = dec[:, state["at"]:state["at"] + b]
        state["at"] += b
        return out

    hist = torch.zeros(rhr.BINS, dtype=torch.int64, device=DEV)
    counters = torch.zeros(5, dtype=torch.int64, device=DEV)
    xy, ratio, score, index, count = slide.analyseSamples(model, slide_case.slide(), REF_BOX, 8, hist, counters)
    assert state["shapes"] == [(24, 1, 512, 512), (24, 1, 512, 512)]
    ref = check_samples(gold_dec, 384, geom["padLR"], geom["padTB"], geom["clipV"], 0.3, REF_BOX, 8)
    n = int(count.item())
    got = dict(index=index[:n].cpu().numpy(), xy=xy[:n].cpu().numpy(), ratio=ratio[:n].cpu().numpy(),
               score=score[:n].cpu().numpy(), hist=hist.cpu().numpy(), counters=counters.cpu().numpy())
    assert_same(got, ref)
    fa = rhr.fit_gauss2(rhr.frequencies(got["hist"]))
    fb = rhr.fit_gauss2(rhr.frequencies(ref["hist"]))
    np.testing.assert_array_equal(fa.params, fb.params)
    assert fa.sse == fb.sse and np.isfinite(fa.sse)


def test_quantify_main(tmp_path, capsys):
    import quantify
    import trainer.model.centerOffsetRes10 as plugin
    from PIL import Image
    torch.manual_seed(0)
    ckpt = tmp_path / "model.pth"
    torch.save(plugin.model(**plugin.modelParams).state_dict(), str(ckpt))
    img = tmp_path / "slide.png"
    Image.fromarray(np.random.RandomState(3).randint(0, 256, (700, 900, 3)).astype(np.uint8)).save(str(img))
    out = tmp_path / "report.json"
    rc = quantify.main(["centerOffsetRes10", str(ckpt), str(img), "-radius", "4", "-samples", "-o", str(out)])
    assert rc == 0
    rep = json.loads(out.read_text())
    c = rep["counters"]
    assert c["above"] >= c["valid"] >= c["kept"] == c["binned"] + c["unbinned"]
    assert len(rep["histogram"]) == 150 and sum(rep["histogram"]) == c["binned"]
    assert rep["box"] is None and rep["radius"] == 4
    assert rep["slides"][0]["box"] == [0, 0, 900, 700]
    assert len(rep["slides"][0]["samples"]) == rep["slides"][0]["counters"]["kept"] == c["kept"]
    if c["binned"] == 0:
        assert rep["fit"] is None and "skipped" in rep["fit_status"]
    else:
        assert len(rep["fit"]["params"]) == 6 and 0.0 <= rep["fit"]["dfi"] <= 1.0
    assert "DFI" in capsys.readouterr().out or c["binned"] == 0
