"""Golden fixture for preprocess.py / the scdx{N}p{M} dataset family, from the REAL reference (build container only).

Run:  python tests/golden/make_golden_preproc.py      (needs /root/reference; never runs on the GPU box; ~5 min)

torchvision is not installed where this runs, so its three module names are stubbed and
torchvision.transforms.functional.rotate is restated with torch's affine_grid / grid_sample exactly as torchvision's
tensor path builds it (rotation about the image centre by the inverse matrix [cosA, -sinA; sinA, cosA] on pixel
centres, bilinear, zeros outside, align_corners=False).  That the restatement equals real torchvision bit for bit has
not been measured; on the CPU it matched the reference's own pure-torch rotateNearestNeighbour at 90/180/270 degrees
and a linear ramp at 12.3 / -14.9 degrees within the half-pixel bound.

1. Runs the reference's datasets.preprocessor.scdManual.generateArchieve itself on a synthetic 40 x 56 x 3 uint8
   slide (margins 4 4 4 4, destinationSize 16, two annotation lines) after numpy.random.seed(42): 12 tiles x 16
   repeats.  Its hard-coded writes under /hy-tmp are captured by replacing numpy.save and the module-level `open` of
   that module; the angles by wrapping the module's `rotate`.
2. Re-evaluates the same 16 rotations with the same stub in float64: rot_ref32_err = the largest absolute
   difference to the reference's float32 samples, i.e. the reference's own noise floor.
3. Asserts that no object centre (4 cx + ox, 4 cy + oy) lies within 1e-3 px of a tile boundary, so the tile
   assignment is exact.
4. Splits: the reference's datasets.scds.scdx8p50.SCD without a profile and datasets.scds.scdx1p5.SCD with
   {"validation": <valid_ids of scd.npz>}, each after random.seed(77), on the canonical synthetic archive of
   oracle/scd_archive.py.
Writes tests/golden/preproc.npz:
  slide (40,56,3) u8, annotation (text bytes), margin, tile, angles (16) f64, names_json / count_json (the
  reference's dataset.json / object-count.json, bytes), samples (192,16,16) f32 and locs (sum n, 8) f64 with
  locs_count (192) in the order of names_json, rot_ref32_err,
  x8p50_valid / x8p50_train / x8p50_profile_json, x1p5_valid / x1p5_train / x1p5_profile_json (ids int32).
"""
import importlib.util
import io
import json
import math
import os
import random
import shutil
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
WORK = "/tmp/preproc_golden"

sys.dont_write_bytecode = True
for _n in ["torchvision", "torchvision.transforms", "torchvision.transforms.functional"]:
    sys.modules[_n] = types.ModuleType(_n)
sys.modules["torchvision"].transforms = sys.modules["torchvision.transforms"]
sys.modules["torchvision.transforms"].functional = sys.modules["torchvision.transforms.functional"]
sys.path.insert(0, REF)
sys.path.insert(1, REPO)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402


def tv_rotate(img, angle, interpolation=None, expand=False, center=None, fill=None):
    """torchvision.transforms.functional.rotate, tensor path, restated (see the module docstring)."""
    n, c, h, w = img.shape
    a = math.radians(angle)
    theta = torch.tensor([[math.cos(a), -math.sin(a) * h / w, 0.0], [math.sin(a) * w / h, math.cos(a), 0.0]],
                         dtype=img.dtype)
    grid = F.affine_grid(theta[None].expand(n, 2, 3), (n, c, h, w), align_corners=False)
    return F.grid_sample(img, grid, mode="bilinear", padding_mode="zeros", align_corners=False)


sys.modules["torchvision.transforms.functional"].rotate = tv_rotate

from PIL import Image  # noqa: E402

from configuration import defaultConfig  # noqa: E402  (reference)
from datasets.preprocessor import scdManual  # noqa: E402  (reference)
from datasets.scds import scdx1p5, scdx8p50  # noqa: E402  (reference)

from oracle import scd_archive  # noqa: E402

H, W, MARGIN, TILE = 40, 56, [4, 4, 4, 4], 16
ANNOTATION = "9.5;7.25;19.0;12.5;3.0;6.0\n41.0;30.5;33.5;23.0;2.5;5.0\n"


def slide():
    return np.random.RandomState(11).randint(0, 256, (H, W, 3)).astype(np.uint8)


def run_reference_preprocess():
    shutil.rmtree(WORK, ignore_errors=True)
    os.makedirs(os.path.join(WORK, "img"))
    os.makedirs(os.path.join(WORK, "ann"))
    img = slide()
    Image.fromarray(img).save(os.path.join(WORK, "img", "1.png"))
    with open(os.path.join(WORK, "ann", "1.txt"), "w") as f:
        f.write(ANNOTATION)
    saved, texts, angles = {}, {}, []

    class Capture(io.StringIO):
        def __init__(self, path):
            super().__init__()
            self.path = path

        def close(self):
            texts[self.path] = self.getvalue()
            super().close()

    real_open, real_save, real_rotate = open, np.save, scdManual.rotate

    def fake_open(path, *a, **k):
        return Capture(path) if str(path).startswith("/hy-tmp/") else real_open(path, *a, **k)

    def fake_save(path, arr, *a, **k):
        saved[path] = np.array(arr)

    def spy_rotate(tensor, angle, *a, **k):
        angles.append(angle)
        return real_rotate(tensor, angle, *a, **k)

    settings = {"inputImage": os.path.join(WORK, "img") + "/", "annotation": os.path.join(WORK, "ann") + "/",
                "destinationSize": TILE, "margin": MARGIN, "iouThreshold": 0.7, "verbal": False}
    scdManual.open, np.save, scdManual.rotate = fake_open, fake_save, spy_rotate
    try:
        np.random.seed(42)
        scdManual.generateArchieve(settings, ["1.png"], None)
    finally:
        del scdManual.open
        np.save, scdManual.rotate = real_save, real_rotate
    names = json.loads(texts["/hy-tmp/temp/confocalCenter/dataset.json"])["names"]
    assert len(names) == 12 * 16 and len(angles) == 16, (len(names), len(angles))
    samples = np.stack([saved["/hy-tmp/temp/confocalCenter/samples/" + n] for n in names]).astype(np.float32)
    locs = [saved["/hy-tmp/temp/confocalCenter/locs/" + n].reshape(-1, 8) for n in names]
    assert samples.shape == (192, TILE, TILE)

    # (3) exact tile assignment: no centre near a tile boundary (and every object in exactly the tiles it was given)
    for l in locs:
        for cx, cy in zip(l[:, 0] * 4 + l[:, 2], l[:, 1] * 4 + l[:, 3]):
            for v in (cx, cy):
                assert abs(v - TILE * round(v / TILE)) > 1e-3, ("object centre on a tile boundary", v)

    # (2) the same rotations in float64
    grey = 0.30 * img[:, :, 0] + 0.59 * img[:, :, 1] + 0.11 * img[:, :, 2]
    g = torch.from_numpy(grey).float().double().reshape(1, 1, H, W)
    g = F.pad(g, (MARGIN[0], MARGIN[2], MARGIN[1], MARGIN[3]), "reflect")
    hp, wp = g.shape[2:]
    radius = math.sqrt(wp ** 2 + hp ** 2) / 2
    lp, tp = math.ceil(radius - 0.5 * wp), math.ceil(radius - 0.5 * hp)
    q = F.pad(g, (lp, lp, tp, tp), "reflect")
    err = 0.0
    for r, a in enumerate(angles):
        rot = tv_rotate(q, a)[0, 0, tp:tp + hp, lp:lp + wp].numpy()
        k = 0
        for x in range(wp // TILE):
            for y in range(hp // TILE):
                ref = samples[r * 12 + k].astype(np.float64)
                err = max(err, float(np.abs(rot[y * TILE:(y + 1) * TILE, x * TILE:(x + 1) * TILE] - ref).max()))
                k += 1
    return {
        "slide": img, "annotation": np.frombuffer(ANNOTATION.encode(), np.uint8), "margin": np.array(MARGIN, np.int32),
        "tile": np.array(TILE, np.int32), "angles": np.array(angles, np.float64),
        "names_json": np.frombuffer(texts["/hy-tmp/temp/confocalCenter/dataset.json"].encode(), np.uint8),
        "count_json": np.frombuffer(texts["/hy-tmp/temp/confocalCenter/object-count.json"].encode(), np.uint8),
        "samples": samples, "locs": np.concatenate(locs).astype(np.float64),
        "locs_count": np.array([len(l) for l in locs], np.int32), "rot_ref32_err": np.array(err, np.float64),
    }


def product_writer():
    pkg = os.path.join(REPO, "scd-resnet_amd")
    spec = importlib.util.spec_from_file_location("_scd_plugin", os.path.join(pkg, "trainer", "dataset",
                                                                             "scdx16p100.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.writeArchive


def run_reference_splits():
    path = os.path.join(WORK, "synthetic.d")
    names, samples, locs = scd_archive.archive_content()
    product_writer()(path, names, samples, locs)
    defaultConfig.config["dirTemp"] = os.path.join(WORK, "temp") + "/"
    defaultConfig.config["dirDataSplitProfile"] = os.path.join(WORK, "split.json")
    valid16 = np.load(os.path.join(HERE, "scd.npz"), allow_pickle=False)["valid_ids"].tolist()
    out = {}
    for key, mod, profile in (("x8p50", scdx8p50, None), ("x1p5", scdx1p5, {"validation": valid16})):
        random.seed(77)
        ds = mod.SCD(path, False, profile)
        text = open(defaultConfig.config["dirDataSplitProfile"], "rb").read()
        out[key + "_valid"] = np.array(ds.dataProfile["validation"], np.int32)
        out[key + "_train"] = np.array(ds.order, np.int32)
        out[key + "_profile_json"] = np.frombuffer(text, np.uint8)
        print(key, "validation", len(out[key + "_valid"]), "train", len(out[key + "_train"]), sorted(json.loads(text)))
    return out


def main():
    out = run_reference_preprocess()
    print("preprocess: %d samples, %d objects, angles %.3f .. %.3f, rot_ref32_err %.3g" % (
        len(out["samples"]), int(out["locs_count"].sum()), out["angles"].min(), out["angles"].max(),
        float(out["rot_ref32_err"])))
    out.update(run_reference_splits())
    np.savez_compressed(os.path.join(HERE, "preproc.npz"), **out)
    print("preproc.npz: %d bytes" % os.path.getsize(os.path.join(HERE, "preproc.npz")))
    shutil.rmtree(WORK, ignore_errors=True)


if __name__ == "__main__":
    main()
