"""preprocess.py on the GPU: scd_slide_rotate_clips (ops.slide_rotate_clips) against a float64 CPU oracle and against
the reference's own tiles (tests/golden/preproc.npz, tests/golden/make_golden_preproc.py), its argument errors, and
preprocess.main end to end into an archive the scdx{N}p{M} plugins read.

The oracle is argumentations.rotate(pad_reflect(grey, margins), angle, MirrorPadding, Bilinear) restated in float64
with torch only: F.pad('reflect') twice and torchvision's tensor rotate as affine_grid / grid_sample
(align_corners=False, zeros padding).  That this restatement equals real torchvision bit for bit has not been
measured.

Tolerance against the oracle: atol = 16 * 2^-24 * 256 = 2.4e-4 on 0-255 data -- the kernel's coordinates are float64
like the oracle's, so what differs is the float32 rounding of the grey value, of the two weights and of the three
lerps of values below 256 (each at most half an ulp of 256 per operation, 16 ulps bound them all).  Against the
reference's float32 tiles the fixture's rot_ref32_err (the reference's own distance from the float64 evaluation) is
added.  At angle 0 the source coordinates are exact integers and the output equals the padded grey slide bit for bit.
"""
import ctypes
import json
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
ATOL = 16 * 2.0 ** -24 * 256


def grey32(rgb):
    c = rgb.astype(np.float64)
    return torch.from_numpy((0.30 * c[:, :, 0] + 0.59 * c[:, :, 1]) + 0.11 * c[:, :, 2]).float()


def padded(rgb, margins):
    l, t, r, b = margins
    return F.pad(grey32(rgb)[None, None], (l, r, t, b), "reflect")


def oracle(rgb, margins, tile, angles):
    """(R, nx*ny, tile, tile) float64."""
    g = padded(rgb, margins).double()
    hp, wp = g.shape[2:]
    radius = math.sqrt(wp ** 2 + hp ** 2) / 2
    lp, tp = math.ceil(radius - 0.5 * wp), math.ceil(radius - 0.5 * hp)
    q = F.pad(g, (lp, lp, tp, tp), "reflect")
    hq, wq = q.shape[2:]
    out = []
    for angle in angles:
        a = math.radians(angle)
        theta = torch.tensor([[[math.cos(a), -math.sin(a) * hq / wq, 0.0], [math.sin(a) * wq / hq, math.cos(a), 0.0]]],
                             dtype=torch.float64)
        grid = F.affine_grid(theta, (1, 1, hq, wq), align_corners=False)
        rot = F.grid_sample(q, grid, mode="bilinear", padding_mode="zeros", align_corners=False)
        rot = rot[0, 0, tp:tp + hp, lp:lp + wp]
        out.append(torch.stack([rot[y * tile:(y + 1) * tile, x * tile:(x + 1) * tile]
                                for x in range(wp // tile) for y in range(hp // tile)]))
    return torch.stack(out).numpy()


def tiles_of(plane, tile):
    hp, wp = plane.shape
    return np.stack([plane[y * tile:(y + 1) * tile, x * tile:(x + 1) * tile]
                     for x in range(wp // tile) for y in range(hp // tile)])


CASES = {
    # H, W, C, margins (l, t, r, b), tile, angles
    "a-88x120": (88, 120, 3, (4, 4, 4, 4), 32, (0.0, -15.0, 12.3, 14.999, 7.0)),
    "b-4ch-asymmetric": (40, 56, 4, (8, 0, 0, 8), 16, (0.0, -7.5, 3.0, 15.0)),
    "c-500x1000-tile512": (500, 1000, 3, (12, 6, 12, 6), 512, (0.0, -11.0)),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_rotate_clips_vs_float64_oracle(case):
    from scdhip import ops
    H, W, C, margins, tile, angles = CASES[case]
    rgb = np.random.RandomState(H + W).randint(0, 256, (H, W, C)).astype(np.uint8)
    got = ops.slide_rotate_clips(torch.from_numpy(rgb).to(DEV), margins, tile, angles).cpu().numpy()
    want = oracle(rgb, margins, tile, angles)
    assert got.shape == want.shape and got.dtype == np.float32
    err = np.abs(got - want).reshape(len(angles), -1).max(1)
    print("%s: max |kernel - float64 oracle| per angle %s (atol %.3g)" % (case, err, ATOL))
    np.testing.assert_allclose(got, want, rtol=0, atol=ATOL)
    # angle 0: the reflect-padded grey slide itself
    np.testing.assert_array_equal(got[0], tiles_of(padded(rgb, margins)[0, 0].numpy(), tile))


def test_rotate_clips_vs_reference_tiles(golden):
    from scdhip import ops
    g = golden("preproc")
    got = ops.slide_rotate_clips(torch.from_numpy(g["slide"]).to(DEV), g["margin"].tolist(), int(g["tile"]),
                                 g["angles"].tolist()).cpu().numpy()
    ref = g["samples"].reshape(16, 12, 16, 16)
    bound = float(g["rot_ref32_err"]) + ATOL
    err = np.abs(got.astype(np.float64) - ref).reshape(16, -1).max(1)
    print("max |kernel - reference tile| per repeat %s (bound %.3g)" % (err, bound))
    assert got.shape == ref.shape
    assert (err <= bound).all(), err


def _raw_call(rgb, H, W, C, margins, tile, angles, out, ws):
    import scdhip.lib as L
    ang = (ctypes.c_double * max(1, len(angles)))(*angles)
    return L.lib().scd_slide_rotate_clips(rgb.data_ptr(), H, W, C, *margins, tile, ang, len(angles), out.data_ptr(),
                                          ws.data_ptr(), 0)


BAD = {
    # H, W, C, margins, tile, R
    "padded-width-no-multiple": (40, 56, 3, (4, 4, 5, 4), 16, 2),
    "padded-height-no-multiple": (40, 56, 3, (4, 4, 4, 5), 16, 2),
    "left-margin-ge-width": (40, 56, 3, (56, 4, 16, 4), 16, 2),
    "right-margin-ge-width": (40, 56, 3, (16, 4, 56, 4), 16, 2),
    "top-margin-ge-height": (40, 56, 3, (4, 40, 4, 16), 16, 2),
    "bottom-margin-ge-height": (40, 56, 3, (4, 16, 4, 40), 16, 2),
    "diagonal-padding-ge-width": (252, 4, 3, (0, 0, 0, 0), 4, 2),
    "diagonal-padding-ge-height": (4, 252, 3, (0, 0, 0, 0), 4, 2),
    "two-channels": (40, 56, 2, (4, 4, 4, 4), 16, 2),
    "no-angle": (40, 56, 3, (4, 4, 4, 4), 16, 0),
    "seventeen-angles": (40, 56, 3, (4, 4, 4, 4), 16, 17),
    "tile-no-multiple-of-4": (40, 56, 3, (4, 4, 4, 4), 2, 2),
    "output-of-2^31-elements": (16384, 16384, 3, (0, 0, 0, 0), 16384, 8),
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_argument_errors_launch_nothing(case):
    """SCD_ERR_ARG from the C entry point with the output and the workspace untouched (the grey pass would overwrite
    the workspace, the rotation the output), and a RuntimeError from the wrapper."""
    from scdhip import ops
    H, W, C, margins, tile, R = BAD[case]
    angles = [3.0] * R
    # the library returns before it reads the slide, so a token buffer stands in for the 2^31 case's slide
    small = H * W * C <= 1 << 20
    rgb = torch.zeros((H, W, C) if small else (4, 4, C), dtype=torch.uint8, device=DEV)
    out = torch.full((1 << 20,), -7.0, device=DEV)
    ws = torch.full((1 << 20,), -7.0, device=DEV)
    assert _raw_call(rgb, H, W, C, margins, tile, angles, out, ws) == 9001
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((ws == -7.0).all())
    if small:
        with pytest.raises(RuntimeError, match="scd_slide_rotate_clips"):
            ops.slide_rotate_clips(rgb, margins, tile, angles)


def test_wrapper_refuses_2_31_elements_cpu_tensors_and_other_resampling():
    from scdhip import ops
    huge = torch.empty(16384, 16384, 3, dtype=torch.uint8, device=DEV)      # refused before the 8 GiB output exists
    with pytest.raises(RuntimeError, match="scd_slide_rotate_clips"):
        ops.slide_rotate_clips(huge, (0, 0, 0, 0), 16384, [1.0] * 8)
    del huge
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.slide_rotate_clips(torch.zeros(40, 56, 3, dtype=torch.uint8), (4, 4, 4, 4), 16, [1.0])
    with pytest.raises(RuntimeError, match="only bilinear"):
        ops.slide_rotate_clips(torch.zeros(40, 56, 3, dtype=torch.uint8, device=DEV), (4, 4, 4, 4), 16, [1.0],
                               resample="nearest")


def test_preprocess_main_end_to_end(tmp_path, golden):
    """Two slides, the second without annotation: the archive holds the first one's 16 x 12 tiles under the
    fixture's names, readArchive loads it, the counts are the reference's, and a scdx1p100 batch comes out of it."""
    from PIL import Image

    import preprocess as P
    from configuration import defaultConfig
    from trainer.dataset import scdx1p100 as D
    g = golden("preproc")
    (tmp_path / "img").mkdir()
    (tmp_path / "ann").mkdir()
    Image.fromarray(g["slide"]).save(str(tmp_path / "img" / "1.png"))
    Image.fromarray(g["slide"][::-1].copy()).save(str(tmp_path / "img" / "2.png"))
    (tmp_path / "ann" / "1.txt").write_text(bytes(g["annotation"]).decode())
    path = str(tmp_path / "out.d")
    np.random.seed(42)
    P.main(P.parseArguments([path, "-i", str(tmp_path / "img") + "/", "-a", str(tmp_path / "ann") + "/", "-s", "16",
                             "-m", "4 4 4 4", "-v", "-p", "datasets.preprocessor.scdManual"]))
    names, counts, samples, bounds = D.readArchive(path, str(tmp_path / "none") + "/")
    ref_names = [n[:-len(".npy")] for n in json.loads(bytes(g["names_json"]).decode())["names"]]
    assert names == ref_names == ["1.%d.%d" % (r, r * 12 + k + 1) for r in range(16) for k in range(12)]
    assert counts == {"count": {n: int(c) for n, c in zip(names, g["locs_count"])}}
    assert [len(b) for b in bounds] == g["locs_count"].tolist()
    assert all(tuple(s.shape) == (1, 16, 16) and s.dtype == torch.float32 for s in samples)
    assert all(tuple(b.shape) == (int(c), 8) and b.dtype == torch.float32 for b, c in zip(bounds, g["locs_count"]))
    bound = float(g["rot_ref32_err"]) + ATOL
    assert np.abs(torch.cat(samples).numpy().astype(np.float64) - g["samples"]).max() <= bound
    np.testing.assert_allclose(torch.cat(bounds).numpy(), g["locs"], rtol=0, atol=1e-4)

    old = dict(defaultConfig.config)
    defaultConfig.config["dirTemp"] = str(tmp_path / "temp") + "/"
    defaultConfig.config["dirDataSplitProfile"] = str(tmp_path / "split.json")
    try:
        ds = D.SCD(path, True, {"validation": [0, 1]})
    finally:
        defaultConfig.config.clear()
        defaultConfig.config.update(old)
    assert len(ds) == 22 and sorted(ds.order) == list(range(2, 24))      # repeat 0 of a 24-clip slide, less two
    assert json.loads(open(str(tmp_path / "split.json")).read())["train1p100"] == ds.order
    b = ds.gpu_batch([0, 1])
    assert b["xs"][0].shape == (2, 1, 16, 16) and b["xs"][0].is_cuda and torch.isfinite(b["xs"][0]).all()
    assert [tuple(y.shape) for y in b["ys"]] == [(2, 1, 128, 128), (2, 30), (2, 30, 6), (2, 30)]


def test_slide_that_does_not_fit_the_tile_raises_before_any_draw(tmp_path, golden):
    import zipfile

    from PIL import Image

    from datasets.preprocessor import scdManual as M
    g = golden("preproc")
    Image.fromarray(g["slide"]).save(str(tmp_path / "3.png"))
    (tmp_path / "3.txt").write_text(bytes(g["annotation"]).decode())
    settings = {"inputImage": str(tmp_path), "annotation": str(tmp_path), "destinationSize": 16, "margin": [4, 4, 5, 4],
                "iouThreshold": 0.7, "verbal": False}
    np.random.seed(42)
    with zipfile.ZipFile(str(tmp_path / "o.d"), "w") as z:
        with pytest.raises(RuntimeError, match=r"3\.png.*multiple of 16"):
            M.generateArchieve(settings, ["3.png"], z)
    assert np.random.uniform() * 30 - 15 == g["angles"][0]       # no draw was consumed
