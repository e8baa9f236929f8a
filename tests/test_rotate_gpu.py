"""Random-angle rotation augmentation on the GPU: scd_rotate_tiles (ops.rotate_tiles) against a float64
CPU oracle and the reference's own rotated tiles (tests/golden/rotaug.npz, tests/golden/make_golden_rotaug.py), the
agreement of its direction with SCD.rotateLocs, its argument errors, and the dataset plugin's switch end to end.

The oracle is argumentations.rotate(tile, angle, MirrorPadding, Bilinear) restated in float64 with torch only, as
tests/test_preprocess_gpu.py's: F.pad('reflect') to the diagonal, torchvision's tensor rotate as affine_grid /
grid_sample (align_corners=False, zeros padding), the centre crop.  That this restatement equals real torchvision bit
for bit has not been measured.

Tolerance against the oracle: atol = 16 * 2^-24 * max|x| -- the derivation of tests/test_preprocess_gpu.py scaled to
the data: the kernel's coordinates are float64 like the oracle's, so what differs is the float32 rounding of the two
weights and of the three lerps of values below max|x| (each at most half an ulp of max|x| per operation, 16 ulps
bound them all).  Against the reference's float32 tiles the fixture's ref32_err (the reference's own distance from
the float64 evaluation) is added.  At angle 0 the source coordinates are whole and the output is the input bit for bit.
"""
import json
import math
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import scd_archive

pytestmark = pytest.mark.gpu
DEV = "cuda"
ERR_ARG = 9001


def atol_for(x):
    return 16 * 2.0 ** -24 * float(np.abs(x).max())


def oracle(x, angles):
    """(B,H,W) float32 array, B angles in degrees -> (B,H,W) float64."""
    B, H, W = x.shape
    radius = math.sqrt(W ** 2 + H ** 2) / 2
    lp, tp = math.ceil(radius - 0.5 * W), math.ceil(radius - 0.5 * H)
    q = F.pad(torch.from_numpy(x).double()[:, None], (lp, lp, tp, tp), "reflect")
    hq, wq = q.shape[2:]
    theta = torch.tensor([[[math.cos(a), -math.sin(a) * hq / wq, 0.0], [math.sin(a) * wq / hq, math.cos(a), 0.0]]
                          for a in (math.radians(d) for d in angles)], dtype=torch.float64)
    grid = F.affine_grid(theta, (B, 1, hq, wq), align_corners=False)
    rot = F.grid_sample(q, grid, mode="bilinear", padding_mode="zeros", align_corners=False)
    return rot[:, 0, tp:tp + H, lp:lp + W].numpy()


SHAPES = {
    # B, H, W, one angle per tile
    "3x6x8": (3, 6, 8, (0.0, 33.3, -120.0)),
    "2x16x16": (2, 16, 16, (2.0, 179.0)),
    "1x24x32": (1, 24, 32, (-41.5,)),
    "2x512x512": (2, 512, 512, (-2.0, 45.0)),
}


@pytest.mark.parametrize("case", sorted(SHAPES))
def test_rotate_tiles_vs_float64_oracle(case):
    from scdhip import ops
    B, H, W, angles = SHAPES[case]
    x = (np.random.RandomState(B + H + W).standard_normal((B, H, W)) * 30 + 100).astype(np.float32)
    xd = torch.from_numpy(x).to(DEV)
    got = ops.rotate_tiles(xd, angles).cpu().numpy()
    want = oracle(x, angles)
    atol = atol_for(x)
    assert got.shape == want.shape and got.dtype == np.float32
    err = np.abs(got - want).reshape(B, -1).max(1)
    print("%s: max |kernel - float64 oracle| per tile %s (atol %.3g)" % (case, err, atol))
    np.testing.assert_allclose(got, want, rtol=0, atol=atol)
    # every thread-to-pixel mapping computes the same bits, and (B,1,H,W) is taken like (B,H,W)
    for mapping in sorted(ops.ROTATE_MAPS):
        np.testing.assert_array_equal(ops.rotate_tiles(xd, angles, mapping=mapping).cpu().numpy(), got, err_msg=mapping)
    four = ops.rotate_tiles(xd[:, None], angles)
    assert four.shape == (B, 1, H, W) and torch.equal(four[:, 0].cpu(), torch.from_numpy(got))
    # angle 0: the input itself
    out = torch.full_like(xd, -7.0)
    assert ops.rotate_tiles(xd, [0.0] * B, out=out).data_ptr() == out.data_ptr()
    np.testing.assert_array_equal(out.cpu().numpy(), x)


@pytest.mark.parametrize("shape", ["16x16", "24x32", "64x64"])
def test_rotate_tiles_vs_reference_tiles(golden, shape):
    from scdhip import ops
    g = golden("rotaug")
    img, ref, angles = g["img_" + shape], g["rot_" + shape], g["angles"].tolist()
    tiles = torch.from_numpy(np.repeat(img[None], len(angles), 0)).to(DEV)
    got = ops.rotate_tiles(tiles, angles).cpu().numpy()
    bound = g["ref32_err_" + shape] + atol_for(img)
    err = np.abs(got.astype(np.float64) - ref).reshape(len(angles), -1).max(1)
    print("%s: max |kernel - reference tile| per angle %s (bound %s)" % (shape, err, bound))
    assert got.shape == ref.shape
    assert (err <= bound).all(), (err, bound)


def blob_case():
    """A 512 x 512 tile of zeros with Gaussian blobs (sigma 3 px) at image pixels 4 c + 1.5 for four label centres c
    about 25 heatmap cells (100 px) from the centre, and their label rows."""
    centres = np.array([[88.0, 66.0], [63.0, 39.0], [46.0, 81.0], [75.0, 84.0]], np.float32)
    rows = np.zeros((len(centres), 8), np.float32)
    rows[:, 0:2] = centres
    rows[:, 4:8] = [2.0, 1.0, 1.0, 3.0]
    yy, xx = np.mgrid[0:512, 0:512].astype(np.float64)
    tile = np.zeros((512, 512))
    for cx, cy in centres:
        tile += np.exp(-((xx - (4 * cx + 1.5)) ** 2 + (yy - (4 * cy + 1.5)) ** 2) / (2 * 3.0 ** 2))
    return tile.astype(np.float32), rows


def centroid_near(img, px, py, half=16):
    """Intensity centroid (x, y) of the window of +-half pixels about (px, py)."""
    x0, y0 = int(round(px)) - half, int(round(py)) - half
    win = np.asarray(img, np.float64)[y0:y0 + 2 * half + 1, x0:x0 + 2 * half + 1]
    yy, xx = np.mgrid[y0:y0 + 2 * half + 1, x0:x0 + 2 * half + 1]
    assert win.sum() > 10, "no blob near (%s, %s): mass %s" % (px, py, win.sum())       # a whole blob is 2 pi 9 = 56
    return float((win * xx).sum() / win.sum()), float((win * yy).sum() / win.sum())


@pytest.mark.parametrize("angle", [20.0, -35.0])
def test_pixels_and_labels_turn_the_same_way(angle):
    """The reference never ran its rotation block, so nothing else certifies that rotate() and rotateCoordinates turn
    the same way: each blob's centroid in the rotated tile lies within 1 image pixel of 4 x its rotateLocs centre +
    1.5 (a wrong sign misses by 2 * 100 * sin(20 deg) = 68 px).  The float64 oracle is held to the same first."""
    from scdhip import ops
    from trainer.dataset.scdx16p100 import SCD
    tile, rows = blob_case()
    turned = SCD.rotateLocs(rows, angle)
    assert len(turned) == len(rows)         # interior centres: every object stays, no replica enters
    assert np.abs(turned[:, 0:2] - rows[:, 0:2]).max() > 5
    got = ops.rotate_tiles(torch.from_numpy(tile[None]).to(DEV), [angle])[0].cpu().numpy()
    for name, img in (("oracle", oracle(tile[None], [angle])[0]), ("kernel", got)):
        for cx, cy in turned[:, 0:2]:
            px, py = 4 * float(cx) + 1.5, 4 * float(cy) + 1.5
            mx, my = centroid_near(img, px, py)
            dist = math.hypot(mx - px, my - py)
            print("%s %+.0f deg: label (%.2f, %.2f) px, blob centroid (%.2f, %.2f), %.3f px apart" % (
                name, angle, px, py, mx, my, dist))
            assert dist < 1.0, (name, angle, dist)


def _raw_call(inp, out, B, H, W, cs, mapping=None):
    import scdhip.lib as L
    if mapping is None:
        return L.lib().scd_rotate_tiles(inp, out, B, H, W, cs, 0)
    return L.lib().scd_rotate_tiles_mapped(inp, out, B, H, W, cs, mapping, 0)


BAD = {
    # B, H, W, which pointer is NULL or aliased, mapping
    "null-in": (1, 16, 16, "in", None),
    "null-out": (1, 16, 16, "out", None),
    "null-cs": (1, 16, 16, "cs", None),
    "in-is-out": (1, 16, 16, "alias", None),
    "no-tile": (0, 16, 16, None, None),
    "one-row": (1, 1, 16, None, None),
    "two-columns": (1, 16, 2, None, None),
    "no-column": (1, 16, 0, None, None),
    "width-6": (1, 16, 6, None, None),
    "diagonal-padding-ge-height": (1, 4, 252, None, None),
    "diagonal-padding-ge-width": (1, 252, 4, None, None),
    "tile-of-2^31-pixels": (1, 46340, 46344, None, None),
    "unknown-mapping": (1, 16, 16, None, 4),
    "negative-mapping": (1, 16, 16, None, -1),
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_argument_errors_launch_nothing(case):
    """SCD_ERR_ARG from the C entry points with the output untouched.  The library returns before it reads a tile, so
    token buffers stand in for the tiles of the large cases."""
    B, H, W, special, mapping = BAD[case]
    inp = torch.zeros(1 << 16, device=DEV)
    out = torch.full((1 << 16,), -7.0, device=DEV)
    cs = torch.tensor([[1.0, 0.0]], dtype=torch.float64, device=DEV)
    pi, po, pc = inp.data_ptr(), out.data_ptr(), cs.data_ptr()
    if special == "in":
        pi = 0
    elif special == "out":
        po = 0
    elif special == "cs":
        pc = 0
    elif special == "alias":
        pi = po
    assert _raw_call(pi, po, B, H, W, pc, mapping) == ERR_ARG
    if mapping is None:       # the named-mapping entry point refuses the same arguments
        assert _raw_call(pi, po, B, H, W, pc, 0) == ERR_ARG
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())


def test_wrapper_refusals():
    from scdhip import ops
    x = torch.zeros(2, 16, 16, device=DEV)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.rotate_tiles(torch.zeros(2, 16, 16), [1.0, 2.0])
    with pytest.raises(RuntimeError, match="fp32 tiles expected"):
        ops.rotate_tiles(x.double(), [1.0, 2.0])
    with pytest.raises(RuntimeError, match="fp32 tiles expected"):
        ops.rotate_tiles(x.to(torch.bfloat16), [1.0, 2.0])
    with pytest.raises(RuntimeError, match="one channel per tile"):
        ops.rotate_tiles(torch.zeros(2, 2, 16, 16, device=DEV), [1.0, 2.0])
    with pytest.raises(RuntimeError, match="3 angles for 2 tiles"):
        ops.rotate_tiles(x, [1.0, 2.0, 3.0])
    with pytest.raises(RuntimeError, match="out must be"):
        ops.rotate_tiles(x, [1.0, 2.0], out=torch.zeros(2, 16, 8, device=DEV))
    with pytest.raises(RuntimeError, match="scd_rotate_tiles"):
        ops.rotate_tiles(x, [1.0, 2.0], out=x)                                   # in == out
    with pytest.raises(RuntimeError, match="scd_rotate_tiles"):
        ops.rotate_tiles(torch.zeros(1, 16, 6, device=DEV), [1.0])               # W % 4 != 0
    with pytest.raises(RuntimeError, match="scd_rotate_tiles"):
        ops.rotate_tiles(torch.zeros(1, 4, 252, device=DEV), [1.0])              # the diagonal padding >= H
    assert bool((x == 0).all())


# ---------------------------------------------------------------------------------------------- the dataset's switch

COUNT = 7680      # 20 synthetic slides: the 5760 validation positions and 1920 training tiles


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    """tests/test_dataset_gpu.py's `built` on a shorter archive, constructed with the key ON: the validation set must
    not care."""
    from configuration import defaultConfig
    from trainer.dataset import scdx16p100 as D
    d = tmp_path_factory.mktemp("scdrot")
    path = str(d / "synthetic.d")
    scd_archive.write(path, count=COUNT)
    old = dict(defaultConfig.config)
    defaultConfig.config["dirTemp"] = str(d / "temp") + "/"
    defaultConfig.config["dirDataSplitProfile"] = str(d / "split.json")
    defaultConfig.config["rotateAugmentation"] = 30
    try:
        random.seed(77)
        ds = D.SCD(path, True, None)
    finally:
        defaultConfig.config.clear()
        defaultConfig.config.update(old)
    return ds


def batch_with_key(ds, value):
    """gpu_batch(range(32)) from fixed seeds of the three generators it draws from, with the key at `value`."""
    from configuration import defaultConfig
    old = dict(defaultConfig.config)
    defaultConfig.config["rotateAugmentation"] = value
    ds.order.sort()
    random.seed(5)
    np.random.seed(6)
    torch.manual_seed(7)
    try:
        return ds.gpu_batch(list(range(32)))
    finally:
        defaultConfig.config.clear()
        defaultConfig.config.update(old)


def replay(ds, R):
    """The batch batch_with_key(ds, R) must give, from the same draws, written out: per sample two numpy uniforms
    for the flips, a third for the angle when R > 0, one torch normal for the jitter; then one torch seed.  With
    R = 0 this is the path as it was before the rotation existed."""
    from scdhip import ops
    from trainer.dataset import scdx16p100 as D
    ids = [ds.order[i] for i in range(32)]         # gpu_batch has shuffled the order already
    np.random.seed(6)
    torch.manual_seed(7)
    flips, jit, angles = np.zeros((32, 2), np.uint8), np.zeros(32, np.float32), []
    for b in range(32):
        flips[b, 0] = np.random.uniform() > 0.5
        flips[b, 1] = np.random.uniform() > 0.5
        if R > 0:
            angles.append(np.random.uniform() * (2 * R) - R)
        jit[b] = np.float32(1) + np.float32(D.JITTERSV) * torch.randn(1).numpy()[0]
    seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    tiles = torch.stack([ds.samples[i] for i in ids]).to(DEV)
    xs = ops.augment_tiles(tiles, torch.from_numpy(flips).to(DEV), torch.from_numpy(jit).to(DEV), None, D.NOISESV,
                           seed)
    rows = [D.SCD.flipLocs(ds.bounds[i], flips[b, 0], flips[b, 1]) for b, i in enumerate(ids)]
    if R > 0:
        xs = ops.rotate_tiles(xs, angles)
        rows = [D.SCD.rotateLocs(r, a) for r, a in zip(rows, angles)]
    l, n = D._pack_locs(rows, trunc=True)
    ys = ops.render_center_targets(torch.from_numpy(l).to(DEV), torch.from_numpy(n).to(DEV), D.HEATMAPSIZE,
                                   D.THRESHOLDIOU)
    return xs, ys, angles, n


def test_gpu_batch_with_rotation_on(built):
    b = batch_with_key(built, 30)
    x = b["xs"][0]
    assert x.shape == (32, 1, 8, 8) and x.is_cuda and x.dtype == torch.float32 and bool(torch.isfinite(x).all())
    assert [tuple(y.shape) for y in b["ys"]] == [(32, 1, 128, 128), (32, 30), (32, 30, 6), (32, 30)]
    xs, ys, angles, counts = replay(built, 30)
    assert len(angles) == 32 and max(abs(a) for a in angles) <= 30 and len({round(a, 6) for a in angles}) == 32
    assert torch.equal(x, xs)
    for got, want in zip(b["ys"], ys):
        assert got.dtype == want.dtype and torch.equal(got, want)
    assert counts.sum() > 0 and int(b["ys"][1].sum()) > 0         # there are objects, and the targets hold some
    # and the rotation did something: the same draws without it give another batch
    plain = batch_with_key(built, 0)
    assert not torch.equal(plain["xs"][0], x) and not torch.equal(plain["ys"][0], b["ys"][0])


def test_gpu_batch_with_the_key_at_zero_is_the_unmodified_path(built, monkeypatch):
    from scdhip import ops

    def refuse(*a, **k):
        raise AssertionError("rotate_tiles with rotateAugmentation = 0")
    monkeypatch.setattr(ops, "rotate_tiles", refuse)
    b = batch_with_key(built, 0)
    after = np.random.get_state()[1].copy(), torch.get_rng_state()
    xs, ys, angles, _ = replay(built, 0)
    assert angles == []
    assert torch.equal(b["xs"][0], xs)
    for got, want in zip(b["ys"], ys):
        assert got.dtype == want.dtype and torch.equal(got, want)
    # the generators stand where the unmodified path leaves them
    assert np.array_equal(after[0], np.random.get_state()[1]) and torch.equal(after[1], torch.get_rng_state())


def test_validation_set_is_never_rotated(built):
    """Built with the key at 30: the validation tiles are normalize alone, the labels the stored ones."""
    from scdhip import ops
    from trainer.dataset import scdx16p100 as D
    ids = built.dataProfile["validation"][:64]
    tiles = torch.stack([built.samples[i] for i in ids]).to(DEV)
    assert torch.equal(built.validation["xs"][0][:64], ops.augment_tiles(tiles))
    l, _ = D._pack_locs([built.bounds[i] for i in ids], trunc=True)
    assert torch.equal(built.validation["ys"][3][:64].cpu(), torch.from_numpy(l))


def test_train_loop_with_rotation_on(tmp_path, monkeypatch):
    """tests/test_dataset_gpu.py's test_train_loop_on_d_archive at its smallest setting (eager, two iterations) with
    rotateAugmentation = 30: every training batch goes through rotate_tiles, and the losses are finite."""
    from configuration import defaultConfig
    from models.networkFactory import NetworkFactory
    from scdhip import ops
    from trainer.dataset.scdx16p100 import writeArchive
    names, samples, locs = scd_archive.archive_content(seed=5, count=48, size=512)
    path = str(tmp_path / "tiny.d")
    writeArchive(path, names, samples, locs)
    split = tmp_path / "tiny.split.json"
    split.write_text(json.dumps({"validation": list(range(8))}))
    rotated, losses = [], []
    real_rotate = ops.rotate_tiles

    def spy_rotate(tiles, angles, *a, **k):
        rotated.append((tuple(tiles.shape), [float(v) for v in angles]))
        return real_rotate(tiles, angles, *a, **k)
    monkeypatch.setattr(ops, "rotate_tiles", spy_rotate)
    old = dict(defaultConfig.config)
    try:
        defaultConfig.updateConfig({"modelName": "centerOffsetRes10", "datasetName": "tiny", "trainName": "rtest",
                                    "iterations": 2, "validation": 2, "snapshot": 1000, "batchSize": 16,
                                    "stepGraph": False, "rotateAugmentation": 30,
                                    "dirData": "trainer.dataset.scdx16p100", "dirDatafile": path,
                                    "dirDataSplitProfile": str(split), "dirTemp": str(tmp_path / "t") + "/",
                                    "dirResult": str(tmp_path / "r") + "/", "currentIter": 0})
        f = NetworkFactory(True)
        real_train = f.train

        def spy_train(**data):
            loss, stats = real_train(**data)
            losses.append([loss.item()] + [s.item() for s in stats])
            return loss, stats
        f.train = spy_train
        f.beginTraining(0)
        text = open(str(tmp_path / "r" / "evals.rtest.txt")).read()
    finally:
        defaultConfig.config.clear()
        defaultConfig.config.update(old)
    assert len(losses) == 2 and np.isfinite(np.array(losses)).all(), losses
    assert len(rotated) >= 2 and all(shape == (16, 1, 512, 512) for shape, _ in rotated)
    assert all(len(a) == 16 and max(abs(v) for v in a) <= 30 and len(set(a)) == 16 for _, a in rotated)
    assert "[mIoU]" in text and "[Tr]" in text
