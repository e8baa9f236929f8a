"""Golden fixture for the random-angle rotation augmentation (scd_rotate_tiles, SCD.rotateLocs), from the REAL
reference (build container only).

Run:  python tests/golden/make_golden_rotaug.py      (needs /root/reference; never runs on the GPU box; seconds)

torchvision is not installed where this runs, so, as in make_golden_preproc.py, its three module names are stubbed and
torchvision.transforms.functional.rotate is restated with torch's affine_grid / grid_sample exactly as torchvision's
tensor path builds it (rotation about the image centre by the inverse matrix [cosA, -sinA; sinA, cosA] on pixel
centres, with the h / w factors of a non-square image, bilinear, zeros outside, align_corners=False).  That the
restatement equals real torchvision bit for bit has not been measured.

The reference holds the rotation step of SCD.argumentation inside a string literal (datasets/scds/scdx16p100.py:
445-486), so nothing there can be called as a whole.  What this script calls is the reference's own
datasets.argumentations.rotate (pixels) and datasets.scds.scdx16p100.SCD.rotateCoordinates (labels); the glue between
them -- the nine-fold replication of :457-473 and the int() filter of :478-483 -- is carried out HERE,
in the literal's order and arithmetic, with torch as there.  (The literal names ConfocalCenter.rotateCoordinates; the
class of that module is SCD and its rotateCoordinates takes (locs, targetSize, angle).)

1. Image cases: seeded normal float32 tiles of 16 x 16, 24 x 32 and 64 x 64, each rotated by 0, 2, -2, 33.3, 90,
   179 and -120 degrees with rotate(tile, angle, MirrorPadding, Bilinear): the reference's float32 output, and
   ref32_err = its largest distance from the same evaluation (same stub) in float64 -- the reference's own noise floor.
2. Label cases: 40 seeded object rows on the 128 heatmap -- rows within 2 cells of every edge and corner, so that
   mirror replicas enter the map, and rows with a zero offset vector -- through the replication, rotateCoordinates
   and the filter at the same angles.
3. Asserted: no rotated centre coordinate of any replica lies within 1e-3 of an integer and no replica sits at
   distance 0 from the rotation centre, so the kept set and the int() filter are the same for any float32-faithful
   implementation.  The row seed is advanced until that holds; the seed found is stored.
Writes tests/golden/rotaug.npz:
  angles (7) f64; img_{H}x{W} (H,W) f32, rot_{H}x{W} (7,H,W) f32, ref32_err_{H}x{W} (7) f64 for the three shapes;
  loc_rows (40,8) f32, loc_seed, loc_out (sum n, 8) f32 with loc_count (7) in the order of angles.
"""
import math
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"

sys.dont_write_bytecode = True
for _n in ["torchvision", "torchvision.transforms", "torchvision.transforms.functional"]:
    sys.modules[_n] = types.ModuleType(_n)
sys.modules["torchvision"].transforms = sys.modules["torchvision.transforms"]
sys.modules["torchvision.transforms"].functional = sys.modules["torchvision.transforms.functional"]
sys.path.insert(0, REF)

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

from datasets import argumentations as A  # noqa: E402  (reference)
from datasets.scds import scdx16p100 as R  # noqa: E402  (reference)

ANGLES = [0.0, 2.0, -2.0, 33.3, 90.0, 179.0, -120.0]
SHAPES = [(16, 16), (24, 32), (64, 64)]
HEATMAPSIZE = R.HEATMAPSIZE
NROWS = 40


def image_cases():
    out = {}
    for h, w in SHAPES:
        tile = torch.from_numpy(np.random.RandomState(1000 + h + w).standard_normal((h, w)).astype(np.float32))
        radius = math.sqrt(w ** 2 + h ** 2) / 2
        lp, tp = math.ceil(radius - 0.5 * w), math.ceil(radius - 0.5 * h)
        q = F.pad(tile.double()[None, None], (lp, lp, tp, tp), "reflect")
        rots, errs = [], []
        for angle in ANGLES:
            rot = A.rotate(tile[None, None], angle, A.PaddingMode.MirrorPadding, A.ResampleMode.Bilinear)[0, 0]
            assert rot.dtype == torch.float32 and tuple(rot.shape) == (h, w)
            rot64 = tv_rotate(q, angle)[0, 0, tp:tp + h, lp:lp + w]
            rots.append(rot.numpy())
            errs.append(float((rot.double() - rot64).abs().max()))
        key = "%dx%d" % (h, w)
        out["img_" + key] = tile.numpy()
        out["rot_" + key] = np.stack(rots)
        out["ref32_err_" + key] = np.array(errs, np.float64)
        print("%s: ref32_err per angle %s" % (key, ["%.2g" % e for e in errs]))
    return out


def rows_of(seed):
    """40 object rows [ctx, cty, offx, offy, majx, majy, minl, halo]: 12 near the edges and corners, 28 anywhere;
    every fifth one with a zero offset vector."""
    rs = np.random.RandomState(seed)
    rows = np.zeros((NROWS, 8), np.float32)
    rows[:, 0:2] = rs.uniform(0, HEATMAPSIZE, (NROWS, 2))
    lo, hi = (lambda n: rs.uniform(0, 2, n)), (lambda n: rs.uniform(HEATMAPSIZE - 2, HEATMAPSIZE, n))
    rows[0:2, 0], rows[2:4, 0], rows[4:6, 1], rows[6:8, 1] = lo(2), hi(2), lo(2), hi(2)
    rows[8, 0:2], rows[9, 0:2] = lo(2), hi(2)
    rows[10, 0:2], rows[11, 0:2] = (lo(1)[0], hi(1)[0]), (hi(1)[0], lo(1)[0])
    rows[:, 2:4] = rs.uniform(0, 4, (NROWS, 2))
    rows[::5, 2:4] = 0
    rows[:, 4:6] = rs.uniform(-6, 6, (NROWS, 2))
    rows[:, 6] = rs.uniform(1, 4, NROWS)
    rows[:, 7] = rs.uniform(2, 8, NROWS)
    return rows


def replicate(rows):
    """The nine-fold replication (scdx16p100.py:457-473): per row, in the reference's order, the x variants
    (ctx, 2 S - 1 - ctx, -1 - ctx) outermost and the y variants (cty, -1 - cty, 2 S - 1 - cty) innermost; a mirrored
    axis negates that axis' offset and major-axis components.  Python arithmetic on 0-d float32 tensors, then one
    torch.tensor() of the nested list, as there."""
    far = 2 * HEATMAPSIZE - 1
    out = []
    for row in rows:
        cx, cy, ox, oy, mx, my, minor, halo = row
        for kx, x in enumerate((cx, far - cx, -1 - cx)):
            for ky, y in enumerate((cy, -1 - cy, far - cy)):
                out.append([x, y, -ox if kx else ox, -oy if ky else oy, -mx if kx else mx, -my if ky else my,
                            minor, halo])
    return torch.tensor(out)


def keep(rotated):
    """The filter (scdx16p100.py:478-483): the rows whose int() centre lies in [0, S) on both axes, in order."""
    rows = [list(r) for r in rotated if 0 <= int(r[0]) < HEATMAPSIZE and 0 <= int(r[1]) < HEATMAPSIZE]
    return torch.tensor(rows).reshape(-1, 8)


def label_cases():
    centre = HEATMAPSIZE // 2 - 0.5
    seed = 2000
    while True:
        rows = rows_of(seed)
        rep = replicate(torch.from_numpy(rows))
        assert rep.dtype == torch.float32 and tuple(rep.shape) == (9 * NROWS, 8)
        ok = not bool(((rep[:, 0] == centre) & (rep[:, 1] == centre)).any())
        rotated = []
        for angle in ANGLES:
            rot = R.SCD.rotateCoordinates(rep.clone(), HEATMAPSIZE // 2, angle)
            c = rot[:, 0:2].double()
            ok = ok and bool(torch.isfinite(rot).all()) and float((c - c.round()).abs().min()) > 1e-3
            if not ok:
                break
            rotated.append(rot)
        if ok:
            break
        seed += 1
        assert seed < 2000 + 500000, "no seed meets the condition"
    kept = [keep(rot) for rot in rotated]
    print("labels: seed %d, kept per angle %s of %d rows" % (seed, [len(k) for k in kept], NROWS))
    # (angle 0 keeps more than the originals: 2 S - 1 - c of a centre c in (S - 1, S) lies in (S - 1, S) too)
    assert all(len(k) > NROWS // 2 for k in kept) and len(kept[0]) >= NROWS
    return {"loc_rows": rows, "loc_seed": np.array(seed, np.int64),
            "loc_out": torch.cat(kept).numpy().astype(np.float32),
            "loc_count": np.array([len(k) for k in kept], np.int32)}


def main():
    out = {"angles": np.array(ANGLES, np.float64)}
    out.update(image_cases())
    out.update(label_cases())
    path = os.path.join(HERE, "rotaug.npz")
    np.savez_compressed(path, **out)
    print("rotaug.npz: %d bytes" % os.path.getsize(path))


if __name__ == "__main__":
    main()
