"""CornerNet training end to end: scd_render_corner_targets against the centre renderer (same device
functions: bit for bit), against the host rule (trainer/dataset/syntheticCorner.corner_locs + the host renderer) and
fixture F8, the dataset plugins' corner layout, and cornerNetCPool trained through NetworkFactory.

Bounds.  Device against device is exact.  Device against host is tests/test_targets_gpu.py's: both sides add the
float64 Gaussian to the float32 map and round back per splat, only the device's double exp can differ from libm's in
its last bit, so NaN positions are equal, the largest difference is one float32 ulp below 1 (6e-8) and more than
99.99 % of the pixels are identical."""
import json
import random

import numpy as np
import pytest
import torch

import resident_case as C
from oracle import scd_archive
from oracle import targets as T

pytestmark = pytest.mark.gpu
DEV = "cuda"
ERR_ARG = 9001


def _pack(locs_list, K=30, counts=None):
    B = len(locs_list)
    locs = np.zeros((B, K, 8), dtype=np.float32)
    n = np.zeros(B, dtype=np.int32)
    for b, l in enumerate(locs_list):
        l = np.asarray(l, dtype=np.float32).reshape(-1, 8)
        n[b] = len(l)
        locs[b, :min(len(l), K)] = l[:K]
    if counts is None:
        n = np.minimum(n, K)
    return torch.from_numpy(locs).to(DEV), torch.from_numpy(n).to(DEV)


def _rows(locs_list):
    return [np.asarray(l, dtype=np.float32).reshape(-1, 8) for l in locs_list]


def _host_corner_maps(locs_list, size, K=30):
    """(tl, br) (B,1,size,size) by the host rule: corner_locs on the first K rows, then the reference's renderer."""
    from trainer.dataset.syntheticCorner import corner_locs
    tl, br = [], []
    for l in _rows(locs_list):
        a, b = corner_locs(l[:K], size)
        with np.errstate(invalid="ignore", divide="ignore"):
            tl.append(T.render(a, size)[0])
            br.append(T.render(b, size)[0])
    return np.stack(tl), np.stack(br)


def _same(a, b):
    """Bit for bit, a NaN equal to a NaN."""
    return a.dtype == b.dtype and a.shape == b.shape and bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


def _close(got, want, what=""):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    assert got.shape == want.shape, what
    nan = np.isnan(want)
    np.testing.assert_array_equal(np.isnan(got), nan, err_msg=what)
    diff = np.abs(got - want)[~nan]
    print("%s: max difference %.3g, identical %.6f" % (what, diff.max(initial=0.0), (diff == 0).mean()))
    assert diff.max(initial=0.0) <= 6e-8, what
    assert (diff == 0).mean() > 0.9999, what


def _center_outputs_equal(ys, locs, counts, size):
    from scdhip import ops
    heat, mask, regr, inds = ops.render_center_targets(locs, counts, size)
    assert _same(ys[0], heat)
    assert torch.equal(ys[1], mask) and _same(ys[2], regr) and torch.equal(ys[5], inds)


# --------------------------------------------------------------------------------------------- 1: device against device

@pytest.mark.parametrize("H,B", [(32, 2), (128, 32)])
def test_corner_maps_equal_the_centre_renderer_on_corner_rows(H, B):
    from scdhip import ops
    from trainer.dataset.syntheticCorner import corner_locs
    from trainer.dataset.syntheticSCD import sample_objects
    rows = [sample_objects(np.random.RandomState(300 + H + i), size=H) for i in range(B)]
    locs, counts = _pack(rows)
    ys = ops.render_corner_targets(locs, counts, H)
    assert [tuple(y.shape) for y in ys] == [(B, 1, H, H), (B, 30), (B, 30, 6), (B, 1, H, H), (B, 1, H, H), (B, 30)]
    assert ys[1].dtype == torch.bool and ys[5].dtype == torch.int64
    heat, mask, regr, inds = ops.render_center_targets(locs, counts, H)
    assert torch.equal(ys[0], heat) and torch.equal(ys[1], mask)
    assert torch.equal(ys[2], regr) and torch.equal(ys[5], inds)
    corners = [corner_locs(r, H) for r in rows]
    for k, which in ((3, 0), (4, 1)):
        cl, cn = _pack([c[which] for c in corners])
        assert torch.equal(ys[k], ops.render_center_targets(cl, cn, H)[0])
        assert int((ys[k] == 1.0).sum()) >= B and not torch.equal(ys[k], heat)
    for split in sorted(ops.CORNER_SPLITS):                        # every split of the pixel work gives the same bits
        again = ops.render_corner_targets(locs, counts, H, split=split)
        assert all(torch.equal(a, b) for a, b in zip(again, ys)), split


# --------------------------------------------------------------------------------------------- 2: the host rule and F8

def test_corner_maps_against_the_host_rule_and_f8(golden):
    from scdhip import ops
    from trainer.dataset.syntheticCorner import corner_locs
    from trainer.dataset.syntheticSCD import encode_targets
    rs = np.random.RandomState(32)
    rows = [T.random_locs(rs, size=32) for _ in range(2)]
    locs, counts = _pack(rows)
    ys = ops.render_corner_targets(locs, counts, 32)
    g = golden("corner")
    _close(ys[0], g["ys|heat"], "F8 heat")
    _close(ys[3], g["ys|tl"], "F8 tl")
    _close(ys[4], g["ys|br"], "F8 br")
    np.testing.assert_array_equal(ys[2].cpu().numpy(), g["ys|regr"])
    corners = [corner_locs(r, 32) for r in rows]
    for k, which in ((3, 0), (4, 1)):
        _close(ys[k], np.stack([encode_targets(c[which], 32)[0] for c in corners]), "encode_targets %d" % k)


# ------------------------------------------------------------------------------------------------------- 3: edge rows

def row(x, y, mx=3.0, my=1.0, mn=1.5):
    return [x, y, 0.5, 0.25, mx, my, mn, mn + 1.0]


def test_corner_edge_rows():
    from scdhip import ops
    H = 32
    rs = np.random.RandomState(9)

    def many(n):
        return [row(rs.randint(0, H), rs.randint(0, H), rs.uniform(-5, 5), rs.uniform(0, 3), rs.uniform(1, 3))
                for _ in range(n)]

    cases = [
        [row(16, 16, 0.5, 2.0, 0.5), row(6, 24, 1.5, 2.0, 1.5), row(24, 6, -2.5, 2.0, 2.5)],     # ties: 0, 2, 2
        [row(16, 16, -3.2, 1.0, 1.4), row(8, 8, -0.4, -2.0, 2.6)],                               # negative major x
        [row(0, 0), row(31, 31)],                                                                # clipped onto borders
        [row(16, 16)] * 5 + [row(17, 16, 4.0, 0.0, 1.5)],                                        # one shared tl cell
        [],                                                                                      # count 0
        many(40),                                                                                # count above K
    ]
    locs, counts = _pack(cases, counts="as given")
    assert counts.tolist() == [3, 2, 2, 6, 0, 40]
    ys = ops.render_corner_targets(locs, counts, H)
    tl, br = _host_corner_maps(cases, H)
    _close(ys[3], tl, "edge tl")
    _close(ys[4], br, "edge br")
    _center_outputs_equal(ys, locs, counts, H)
    g = ys[3][:, 0].cpu().numpy(), ys[4][:, 0].cpu().numpy()
    # the ties round half to even: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2 (maps are [y, x])
    for (x, y, d) in ((16, 16, 0), (6, 24, 2), (24, 6, 2)):
        assert g[0][0, y - d, x - d] == 1.0 and g[1][0, y + d, x + d] == 1.0
    assert sorted(zip(*np.nonzero(g[0][0] == 1.0))) == [(4, 22), (16, 16), (22, 4)]
    assert g[0][1, 15, 13] == 1.0 and g[1][1, 17, 19] == 1.0                 # |-3.2| -> 3, 1.4 -> 1
    assert g[0][2, 0, 0] == 1.0 and g[1][2, 31, 31] == 1.0 and g[0][2, 29, 28] == 1.0 and g[1][2, 2, 3] == 1.0
    assert g[0][3, 14, 13] == 1.0 and (g[0][3] == 1.0).sum() >= 1
    assert not g[0][4].any() and not g[1][4].any()
    assert not np.array_equal(tl[5], _host_corner_maps([cases[5]], H, K=40)[0][0])        # the 10 cut rows matter

    # K = 64, every slot used
    full = [many(64), many(50)]
    locs, counts = _pack(full, K=64)
    assert counts.tolist() == [64, 50]
    ys = ops.render_corner_targets(locs, counts, H)
    tl, br = _host_corner_maps(full, H, K=64)
    _close(ys[3], tl, "K=64 tl")
    _close(ys[4], br, "K=64 br")
    _center_outputs_equal(ys, locs, counts, H)

    # a zero major axis: radius 0, NaN at the corner cell and nowhere else
    zero = [[row(10, 10, 0.0, 0.0, 1.0), row(20, 20)]]
    locs, counts = _pack(zero)
    ys = ops.render_corner_targets(locs, counts, H)
    tl, br = _host_corner_maps(zero, H)
    _close(ys[3], tl, "zero axis tl")
    _close(ys[4], br, "zero axis br")
    assert torch.isnan(ys[3][0, 0]).nonzero().tolist() == [[9, 10]]
    assert torch.isnan(ys[4][0, 0]).nonzero().tolist() == [[11, 10]]
    _center_outputs_equal(ys, locs, counts, H)


def test_corner_not_drawn_for_outside_centre_or_nan_axis():
    """The two cases the host rule leaves undefined, against the rule as DESIGN §8e completes it."""
    from scdhip import ops
    H = 32
    nan = float("nan")
    cases = [
        [row(-1, 5), row(32, 5), row(5, -1), row(5, 40)],            # every centre outside the map
        [row(10, 10, nan, 1.0, 1.5)],                                # majx NaN: what pack_locs turns a zero axis into
        [row(10, 10, nan, nan, 1.5), row(20, 12), row(40, 12)],      # ... beside an object that is drawn
        [row(20, 12)],
    ]
    locs, counts = _pack(cases)
    ys = ops.render_corner_targets(locs, counts, H)
    for k in (3, 4):
        assert not ys[k][0].any() and not ys[k][1].any()
        assert torch.equal(ys[k][2], ys[k][3]) and int((ys[k][3] == 1.0).sum()) == 1
    _center_outputs_equal(ys, locs, counts, H)
    assert ys[1].tolist()[0][:4] == [False] * 4 and ys[1].tolist()[2][:3] == [True, True, False]


# ------------------------------------------------------------------------------------------------ 4: another map size

def test_corner_other_map_size():
    from scdhip import ops
    from trainer.dataset.syntheticSCD import sample_objects
    rows = [sample_objects(np.random.RandomState(7 + i), size=256) for i in range(4)]
    locs, counts = _pack(rows)
    ys = ops.render_corner_targets(locs, counts, 256)
    tl, br = _host_corner_maps(rows, 256)
    _close(ys[3], tl, "256 tl")
    _close(ys[4], br, "256 br")
    _center_outputs_equal(ys, locs, counts, 256)


# ------------------------------------------------------------------------------------------------- 5: argument errors

@pytest.mark.parametrize("case", ["65-slots", "no-tile", "null-tl", "null-br", "null-heat", "no-size", "bad-split"])
def test_corner_argument_errors_launch_nothing(case):
    import scdhip.lib as L
    locs = torch.zeros(65 * 8, device=DEV)
    counts = torch.ones(1, dtype=torch.int32, device=DEV)
    maps = [torch.full((32 * 32,), -7.0, device=DEV) for _ in range(3)]
    mask = torch.full((65,), 7, dtype=torch.uint8, device=DEV)
    regr = torch.full((65 * 6,), -7.0, device=DEV)
    inds = torch.full((65,), -7, dtype=torch.int64, device=DEV)
    p = {"heat": maps[0].data_ptr(), "tl": maps[1].data_ptr(), "br": maps[2].data_ptr()}
    B, K, H, split = 1, 30, 32, 0
    if case.startswith("null-"):
        p[case[5:]] = 0
    elif case == "65-slots":
        K = 65
    elif case == "no-tile":
        B = 0
    elif case == "no-size":
        H = 0
    args = (locs.data_ptr(), counts.data_ptr(), B, K, H, 0.5, p["heat"], p["tl"], p["br"], mask.data_ptr(),
            regr.data_ptr(), inds.data_ptr())
    if case == "bad-split":
        assert L.lib().scd_render_corner_targets_split(*args, 2, 0) == ERR_ARG
    else:
        assert L.lib().scd_render_corner_targets(*args, 0) == ERR_ARG
        with pytest.raises(RuntimeError, match="scd_render_corner_targets"):
            L.call("scd_render_corner_targets", *args, 0)
    torch.cuda.synchronize()
    assert all(bool((m == -7.0).all()) for m in maps) and bool((mask == 7).all())
    assert bool((regr == -7.0).all()) and bool((inds == -7).all())


def test_corner_binding_refuses_65_slots_and_cpu_rows():
    from scdhip import ops
    with pytest.raises(RuntimeError):
        ops.render_corner_targets(torch.zeros(1, 65, 8, device=DEV), torch.ones(1, dtype=torch.int32, device=DEV), 32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.render_corner_targets(torch.zeros(1, 30, 8), torch.ones(1, dtype=torch.int32), 32)


# ------------------------------------------------------------------------------------------- 6: the synthetic dataset

def test_corner_dataset_gpu_batch_equals_per_sample_items():
    from trainer.dataset.syntheticCorner import CornerSCD
    ds = CornerSCD(None, True, seed=77)
    gb = ds.gpu_batch(range(8), DEV)
    items = [ds[i] for i in range(8)]
    assert len(gb["ys"]) == 5 and all(len(it["ys"]) == 5 for it in items)
    assert torch.equal(gb["xs"][0].cpu(), torch.stack([it["xs"][0] for it in items]))
    ref = [torch.stack([it["ys"][k] for it in items]) for k in range(5)]
    for k in (1, 2):
        assert torch.equal(gb["ys"][k].cpu(), ref[k]), k
    for k in (0, 3, 4):
        assert gb["ys"][k].shape == ref[k].shape
        assert (gb["ys"][k].cpu() - ref[k]).abs().max().item() <= 6e-8, k


# --------------------------------------------------------------------------------------------------- 7: `.d` archive

COUNT = 7680      # 20 synthetic slides: the 5760 validation positions and 1920 training tiles


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    """tests/test_dataset_gpu.py's `built` at tests/test_resident_gpu.py's size (8 x 8 tiles), constructed with
    cornerTargets on: the validation set keeps its corner maps."""
    from configuration import defaultConfig
    from trainer.dataset import scdx16p100 as D
    d = tmp_path_factory.mktemp("scdcorner")
    path = str(d / "synthetic.d")
    scd_archive.write(path, count=COUNT, size=8)
    old = dict(defaultConfig.config)
    defaultConfig.config["dirTemp"] = str(d / "temp") + "/"
    defaultConfig.config["dirDataSplitProfile"] = str(d / "split.json")
    defaultConfig.config["cornerTargets"] = True
    try:
        random.seed(77)
        ds = D.SCD(path, True, None)
    finally:
        defaultConfig.config.clear()
        defaultConfig.config.update(old)
    return ds


def batch_with_keys(ds, corner, rotate=0, resident=False):
    """gpu_batch(range(32)) from fixed seeds of the three generators it draws from (tests/test_resident_gpu.py) ->
    (batch, the numpy and torch generator states afterwards)."""
    from configuration import defaultConfig
    old = dict(defaultConfig.config)
    defaultConfig.config.update({"cornerTargets": corner, "rotateAugmentation": rotate, "residentDataset": resident})
    ds.order.sort()
    random.seed(5)
    np.random.seed(6)
    torch.manual_seed(7)
    try:
        return ds.gpu_batch(list(range(32))), C.host_states()
    finally:
        defaultConfig.config.clear()
        defaultConfig.config.update(old)


def host_rows(ds, R):
    """The packed rows of the host path's batch, from its draws (tests/resident_case.py replay)."""
    from trainer.dataset import scdx16p100 as D
    ids = [ds.order[i] for i in range(32)]
    flips, _, angles, _ = C.draws(R)
    rows = [D.SCD.flipLocs(ds.bounds[i], flips[b, 0], flips[b, 1]) for b, i in enumerate(ids)]
    if R > 0:
        rows = [D.SCD.rotateLocs(r, a) for r, a in zip(rows, angles)]
    l, n = D._pack_locs(rows, trunc=True)
    return torch.from_numpy(l).to(DEV), torch.from_numpy(n).to(DEV), ids, flips, angles


def test_d_archive_key_off_is_the_centre_layout(built):
    off, _ = batch_with_keys(built, False)
    assert [tuple(y.shape) for y in off["ys"]] == [(32, 1, 128, 128), (32, 30), (32, 30, 6), (32, 30)]
    assert off["ys"][3].dtype == torch.int64
    xs, ys = C.replay(built, 0)                                       # the parent's path written out
    assert torch.equal(off["xs"][0], xs) and all(_same(a, b) for a, b in zip(off["ys"], ys))
    vs = built.getValidationSet()
    assert all(len(v["ys"]) == 6 and v["ys"][5].dtype == torch.int64 for v in vs)


def test_d_archive_corner_batches(built):
    from scdhip import ops
    from trainer.dataset import scdx16p100 as D
    off, off_after = batch_with_keys(built, False)
    on, on_after = batch_with_keys(built, True)
    assert C.same_states(on_after, off_after)                         # the draws and their order do not change
    assert len(on["ys"]) == 5 and torch.equal(on["xs"][0], off["xs"][0])
    for k in range(3):
        assert _same(on["ys"][k], off["ys"][k]), k
    locs, counts, _, _, _ = host_rows(built, 0)
    want = ops.render_corner_targets(locs, counts, D.HEATMAPSIZE, D.THRESHOLDIOU)
    for k in (0, 3, 4):
        assert on["ys"][k].shape == (32, 1, 128, 128) and _same(on["ys"][k], want[k]), k
    assert int(counts.sum()) > 0 and not torch.equal(on["ys"][3], on["ys"][0])

    # the resident path, without rotation: bit for bit the host path, and the same draws
    res, res_after = batch_with_keys(built, True, resident=True)
    assert C.same_states(res_after, on_after) and len(res["ys"]) == 5
    assert torch.equal(res["xs"][0], on["xs"][0])
    for k in range(5):
        assert _same(res["ys"][k], on["ys"][k]), k


def test_d_archive_corner_batches_with_rotation(built):
    """At rotateAugmentation 30 the two paths turn the labels with different float32 roundings, so the
    maps are compared on the tiles whose packed rows came out equal; the corner rule sees the turned major axis."""
    from scdhip import ops
    from trainer.dataset import scdx16p100 as D
    host, host_after = batch_with_keys(built, True, rotate=30)
    res, res_after = batch_with_keys(built, True, rotate=30, resident=True)
    assert C.same_states(res_after, host_after)
    assert torch.equal(res["xs"][0], host["xs"][0]) and len(res["ys"]) == len(host["ys"]) == 5
    hl, hn, ids, flips, angles = host_rows(built, 30)
    want = ops.render_corner_targets(hl, hn, D.HEATMAPSIZE, D.THRESHOLDIOU)
    for k in range(5):
        assert _same(host["ys"][k], want[k]), k                      # the host batch renders its own packed rows
    rows, offsets = C.csr(built.bounds)
    dl, dn = ops.pack_locs(rows.to(DEV), offsets.to(DEV), ids, torch.from_numpy(flips).to(DEV), angles,
                           D.HEATMAPSIZE, D.MAXTAGLEN, True)
    want = ops.render_corner_targets(dl, dn, D.HEATMAPSIZE, D.THRESHOLDIOU)
    for k in range(5):
        assert _same(res["ys"][k], want[k]), k                       # ... and the resident batch the device's rows
    eq = ((hl == dl) | (torch.isnan(hl) & torch.isnan(dl))).flatten(1).all(1) & (hn == dn)
    print("rotation 30: %d of 32 tiles with bit-equal packed rows on the two paths" % int(eq.sum()))
    assert bool(eq.any())
    for k in range(5):
        assert _same(res["ys"][k][eq], host["ys"][k][eq]), k
    plain, _ = batch_with_keys(built, True)
    assert not torch.equal(plain["ys"][3], host["ys"][3])


def test_d_archive_corner_validation_set(built):
    from configuration import defaultConfig
    from scdhip import ops
    from trainer.dataset import scdx16p100 as D
    old = dict(defaultConfig.config)
    defaultConfig.config["cornerTargets"] = True
    try:
        vs = built.getValidationSet()
    finally:
        defaultConfig.config.clear()
        defaultConfig.config.update(old)
    size = defaultConfig.validationBatchSize
    assert len(vs) == 5760 // size
    for v in vs:
        heat, mask, regr, tl, br = v["ys"]
        assert v["xs"][0].shape == (size, 1, 8, 8) and heat.shape == (size, 1, 128, 128)
        assert tl.shape == heat.shape and br.shape == heat.shape and tl.dtype == torch.float32
        assert mask.dtype == torch.bool and mask.shape == (size, 30) and regr.shape == (size, 30, 6)
    # the first slice is the renderer on the stored validation rows, the mask every stored object
    v = built.validation
    n = torch.tensor(v["ys"][4][:size], dtype=torch.int32, device=DEV)
    want = ops.render_corner_targets(v["ys"][3][:size], n, D.HEATMAPSIZE, D.THRESHOLDIOU)
    for got, k in zip(vs[0]["ys"], range(5)):
        if k != 1:
            assert _same(got, want[k]), k
    assert torch.equal(vs[0]["ys"][1], torch.arange(30, device=DEV)[None, :] < n[:, None])
    assert int(n.sum()) > 0 and int((vs[0]["ys"][3] == 1.0).sum()) > 0


# ----------------------------------------------------------------------------------------------------- 8: end to end

@pytest.mark.parametrize("data", ["syntheticCorner", "archive", "resident-archive"])
def test_train_cornernet_through_network_factory(tmp_path, data):
    """NetworkFactory end to end with cornerNetCPool (tests/test_dataset_gpu.py test_train_loop_on_d_archive): batches
    through gpu_batch, bf16 steps, validation through cornerNetEvaluation / expression, evals file written."""
    from configuration import defaultConfig
    from models.networkFactory import NetworkFactory
    from trainer.dataset.scdx16p100 import writeArchive
    old = dict(defaultConfig.config)
    cfg = {"modelName": "cornerNetCPool", "trainName": "ctest", "computeDtype": "bf16", "iterations": 2,
           "validation": 2, "snapshot": 2, "batchSize": 4, "dirTemp": str(tmp_path / "t") + "/",
           "dirResult": str(tmp_path / "r") + "/", "currentIter": 0,
           "dirDataSplitProfile": str(tmp_path / "tiny.split.json")}
    if data == "syntheticCorner":
        cfg.update({"datasetName": "syntheticCorner"})
    else:
        names, samples, locs = scd_archive.archive_content(seed=5, count=48, size=512)
        path = str(tmp_path / "tiny.d")
        writeArchive(path, names, samples, locs)
        (tmp_path / "tiny.split.json").write_text(json.dumps({"validation": list(range(8))}))
        cfg.update({"datasetName": "tiny", "dirData": "trainer.dataset.scdx16p100", "dirDatafile": path,
                    "cornerTargets": True, "residentDataset": data == "resident-archive"})
    try:
        defaultConfig.updateConfig(cfg)
        f = NetworkFactory(True)
        f.beginTraining(0)
        if data == "resident-archive":
            assert f.dataset.resident["store"].shape == (48, 512, 512)
        text = open(str(tmp_path / "r" / "evals.ctest.txt")).read()
        losses = np.loadtxt(str(tmp_path / "r" / "losses.ctest.2.txt"), delimiter=",", ndmin=2)
    finally:
        defaultConfig.config.clear()
        defaultConfig.config.update(old)
    assert losses.shape == (2, 2) and np.isfinite(losses).all() and (losses[:, 1] > 0).all()
    assert "[Ct]" in text and "[TL]" in text and "[BR]" in text and "[Tr]" in text and "[It]" in text
