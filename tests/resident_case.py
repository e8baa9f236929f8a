"""Shared by tests/test_resident_cpu.py and tests/test_resident_gpu.py: the seeded label tiles the batched
label rotation (scd_pack_locs) is checked on, SCD.rotateLocs' formulas evaluated in float64, and the host batch path
written out from its draws.  No test lives here.

The float64 evaluation is the yardstick of the rotation test.  The host (torch float32, whose sqrt and pow are not
correctly rounded everywhere) and the device (correctly rounded float32) differ from it by rounding only, so wherever a
coordinate is not within UNSAFE of an integer all three truncate alike and keep the same candidates.  A tile with such
a coordinate among its 9 n candidates is `unsafe` and only counted."""
import math

import numpy as np
import torch

ANGLES = (0.0, 2.0, -2.0, 20.0, -35.0, 90.0, 180.0)
UNSAFE = 5e-4
SEED = 12          # 3 of the 238 slots unsafe, every special tile safe at five angles or more (settled on the CPU)
K = 30
SIZE = 128
# special tiles, by position from the end of rotation_tiles()
CENTRE, NAN, WIDE, FULL = -4, -3, -2, -1


def random_rows(rs, n, lo=0.25, hi=127.75):
    l = np.zeros((n, 8), np.float32)
    l[:, 0:2] = rs.uniform(lo, hi, (n, 2))
    l[:, 2:4] = rs.uniform(-4, 4, (n, 2))
    length, ang = rs.uniform(2, 6, n), rs.uniform(0, 2 * np.pi, n)
    l[:, 4], l[:, 5] = length * np.cos(ang), length * np.sin(ang)
    l[:, 6] = rs.uniform(1, 3, n)
    l[:, 7] = l[:, 6] + rs.uniform(0, 4, n)
    return l


def rotation_tiles(seed=SEED):
    """30 tiles of 0 .. 3 objects anywhere on the map, then four special ones: CENTRE (a row on the rotation centre
    (63.5, 63.5) and a row with a zero offset), NAN (a row with a zero major axis), WIDE (40 rows: 360 candidates, more
    than one workgroup's 256) and FULL (45 rows within 44 cells of the centre on each axis: all of them stay on the map
    at any angle, more than K are kept)."""
    rs = np.random.RandomState(seed)
    tiles = [random_rows(rs, rs.randint(0, 4)) for _ in range(30)]
    centre = random_rows(rs, 3)
    centre[1, 0:2] = 63.5
    centre[2, 0:4] = [80.3, 50.7, 0, 0]         # (both special rows well inside the map: they stay at every angle)
    nan = random_rows(rs, 2)
    nan[0, 0:2] = [40.3, 90.7]
    nan[0, 4:6] = 0
    return tiles + [centre, nan, random_rows(rs, 40), random_rows(rs, 45, 20.0, 107.0)]


def rotation_slots(seed=SEED):
    """Every tile at every angle of ANGLES, with seeded flips: (tile ids, flips (B,2) u8, angles), B = 7 x 34."""
    tiles = rotation_tiles(seed)
    rs = np.random.RandomState(seed + 1)
    ids = [i for _ in ANGLES for i in range(len(tiles))]
    angles = [a for a in ANGLES for _ in range(len(tiles))]
    flips = (rs.uniform(size=(len(ids), 2)) > 0.5).astype(np.uint8)
    flips[:len(tiles)] = 0          # the angle-0 slots unflipped: compared with the stored rows themselves
    return tiles, ids, flips, angles


def csr(tiles):
    rows = np.concatenate([np.asarray(t, np.float32).reshape(-1, 8) for t in tiles] + [np.zeros((0, 8), np.float32)])
    offsets = np.zeros(len(tiles) + 1, np.int64)
    offsets[1:] = np.cumsum([len(t) for t in tiles])
    return torch.from_numpy(rows), torch.from_numpy(offsets)


def rotate_f64(rows, angle, size=SIZE):
    """SCD.rotateLocs' formulas on float32 rows (already flipped) in float64 -> (kept rows (m,8) f64 in candidate
    order, kept candidates' (row, replica) (m,2), safe)."""
    L = np.asarray(rows, np.float32).reshape(-1, 8).astype(np.float64)
    n = len(L)
    if n == 0:
        return np.zeros((0, 8)), np.zeros((0, 2), np.int64), True
    far = 2 * size - 1
    rep = np.repeat(L[:, None, :], 9, axis=1)
    xs = (L[:, 0], far - L[:, 0], -1 - L[:, 0])
    ys = (L[:, 1], -1 - L[:, 1], far - L[:, 1])
    for k in range(9):
        kx, ky = divmod(k, 3)
        rep[:, k, 0], rep[:, k, 1] = xs[kx], ys[ky]
        if kx:
            rep[:, k, 2], rep[:, k, 4] = -L[:, 2], -L[:, 4]
        if ky:
            rep[:, k, 3], rep[:, k, 5] = -L[:, 3], -L[:, 5]
    rep = rep.reshape(-1, 8)
    turn = -angle * math.pi / 180
    ca, sa = math.cos(turn), math.sin(turn)

    def turned(x, y):
        with np.errstate(invalid="ignore", divide="ignore"):
            m = np.sqrt(x * x + y * y)
            s, c = y / m, x / m
            return m * (c * ca - s * sa), m * (s * ca + c * sa), m
    h = size // 2 - 0.5
    out = rep.copy()
    x, y, m = turned(rep[:, 0] - h, rep[:, 1] - h)
    out[:, 0] = np.where(m == 0, rep[:, 0], x + h)
    out[:, 1] = np.where(m == 0, rep[:, 1], y + h)
    x, y, m = turned(rep[:, 2], rep[:, 3])
    out[:, 2], out[:, 3] = np.where(m == 0, 0.0, x), np.where(m == 0, 0.0, y)
    out[:, 4], out[:, 5], _ = turned(rep[:, 4], rep[:, 5])
    safe = bool((np.abs(out[:, 0:2] - np.round(out[:, 0:2])) >= UNSAFE).all())
    cx, cy = np.trunc(out[:, 0]), np.trunc(out[:, 1])
    keep = (cx >= 0) & (cx < size) & (cy >= 0) & (cy < size)
    which = np.stack(np.divmod(np.arange(9 * n), 9), axis=1)
    return out[keep], which[keep], safe


def rotate_f32(rows, angle, size=SIZE):
    """scd_pack_locs' arithmetic restated in numpy float32 -> the kept rows (m,8) f32 in candidate order, not truncated.
    numpy's float32 multiply, add, subtract, divide and sqrt round correctly and are never contracted, which is what
    the kernel promises, so the device must give these bits (torch's CPU sqrt / pow do not everywhere, hence
    SCD.rotateLocs is no bit reference).  (cos, sin) are ops.pack_locs_cs': float64, rounded to float32."""
    f = np.float32
    L = np.asarray(rows, f).reshape(-1, 8)
    n = len(L)
    if n == 0:
        return np.zeros((0, 8), f)
    far = f(2 * size - 1)
    rep = np.repeat(L[:, None, :], 9, axis=1)
    xs = (L[:, 0], far - L[:, 0], f(-1) - L[:, 0])
    ys = (L[:, 1], f(-1) - L[:, 1], far - L[:, 1])
    for k in range(9):
        kx, ky = divmod(k, 3)
        rep[:, k, 0], rep[:, k, 1] = xs[kx], ys[ky]
        if kx:
            rep[:, k, 2], rep[:, k, 4] = -L[:, 2], -L[:, 4]
        if ky:
            rep[:, k, 3], rep[:, k, 5] = -L[:, 3], -L[:, 5]
    rep = rep.reshape(-1, 8)
    turn = -angle * math.pi / 180
    ca, sa = f(math.cos(turn)), f(math.sin(turn))

    def turned(x, y):
        with np.errstate(invalid="ignore", divide="ignore"):
            m = np.sqrt(x * x + y * y)
            s, c = y / m, x / m
            out = m * (c * ca - s * sa), m * (s * ca + c * sa), m
        assert all(o.dtype == f for o in out)
        return out
    shift = f(0.5 - size // 2)
    out = rep.copy()
    sx, sy = rep[:, 0] + shift, rep[:, 1] + shift
    still = (sx == 0) & (sy == 0)
    x, y, _ = turned(sx, sy)
    out[:, 0] = np.where(still, rep[:, 0], x - shift)
    out[:, 1] = np.where(still, rep[:, 1], y - shift)
    x, y, m = turned(rep[:, 2], rep[:, 3])
    out[:, 2], out[:, 3] = np.where(m == 0, f(0), x), np.where(m == 0, f(0), y)
    out[:, 4], out[:, 5], _ = turned(rep[:, 4], rep[:, 5])
    cx, cy = np.trunc(out[:, 0]), np.trunc(out[:, 1])
    return out[(cx >= 0) & (cx < size) & (cy >= 0) & (cy < size)]


def host_states():
    return np.random.get_state(), torch.get_rng_state()


def same_states(a, b):
    return a[0][0] == b[0][0] and np.array_equal(a[0][1], b[0][1]) and a[0][2:] == b[0][2:] and torch.equal(a[1], b[1])


def draws(R, B=32):
    """SCD._draws written out, from numpy seed 6 and torch seed 7: (flips, jitter, angles, seed)."""
    from trainer.dataset import scdx16p100 as D
    np.random.seed(6)
    torch.manual_seed(7)
    flips, jit, angles = np.zeros((B, 2), np.uint8), np.zeros(B, np.float32), []
    for b in range(B):
        flips[b, 0] = np.random.uniform() > 0.5
        flips[b, 1] = np.random.uniform() > 0.5
        if R > 0:
            angles.append(np.random.uniform() * (2 * R) - R)
        jit[b] = np.float32(1) + np.float32(D.JITTERSV) * torch.randn(1).numpy()[0]
    seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    return flips, jit, angles, seed


def replay(ds, R, dev="cuda"):
    """The batch gpu_batch(range(32)) gave through the host path, from the same draws, as the path stood before the
    resident archive existed (tests/test_rotate_gpu.py's replay): ds.order is the order gpu_batch left."""
    from scdhip import ops
    from trainer.dataset import scdx16p100 as D
    ids = [ds.order[i] for i in range(32)]
    flips, jit, angles, seed = draws(R)
    tiles = torch.stack([ds.samples[i] for i in ids]).to(dev)
    xs = ops.augment_tiles(tiles, torch.from_numpy(flips).to(dev), torch.from_numpy(jit).to(dev), None, D.NOISESV,
                           seed)
    rows = [D.SCD.flipLocs(ds.bounds[i], flips[b, 0], flips[b, 1]) for b, i in enumerate(ids)]
    if R > 0:
        xs = ops.rotate_tiles(xs, angles)
        rows = [D.SCD.rotateLocs(r, a) for r, a in zip(rows, angles)]
    l, n = D._pack_locs(rows, trunc=True)
    ys = ops.render_center_targets(torch.from_numpy(l).to(dev), torch.from_numpy(n).to(dev), D.HEATMAPSIZE,
                                   D.THRESHOLDIOU)
    return xs, ys
