"""Device-resident `.d` archive: scd_augment_tiles_indexed against the stacked scd_augment_tiles,
scd_pack_locs against the host's flipLocs / rotateLocs / _pack_locs, and the dataset plugin's residentDataset key
against its host path.

Without rotation everything is asked for bit for bit: the indexed augmentation runs the stacked one's arithmetic on the
same values, and a flip is one exact float32 subtraction and negations on either side.

With rotation the host's bits cannot be asked for: it turns the labels with torch's float32 sqrt / pow / divide, which
are not correctly rounded on every CPU, the device with correctly rounded ones.  The device's own promise, one
correctly rounded uncontracted operation per operation of the formulas, is held bit for bit to numpy float32, which
keeps it.  Against the host, both are held to the same formulas
evaluated in float64 (tests/resident_case.py), on the slots where no candidate coordinate lies within 5e-4 of an integer
(elsewhere the truncation and the keep rule may legitimately differ): equal counts, equal truncated centres, columns 6
and 7 bit-equal, and columns 2..5 within 4 x E_host of float64, E_host = the host's own largest error there but not
below one float32 ulp of 256 (2^-15).  The factor: the two sides differ in rounding only, so their errors are of one
order, while a wrong sign or operand order misses by the size of the value (2 .. 6 here).
Recorded on an MI355X (profiles/resident_dataset.txt): 3 of 238 slots unsafe; E_host 3.05e-05 (the floor; the host's
own error is 6.59e-07), device error 6.59e-07, angle 0 against the stored rows 2.38e-07.
"""
import copy
import random

import numpy as np
import pytest
import torch

import resident_case as C
from oracle import scd_archive

pytestmark = pytest.mark.gpu
DEV = "cuda"
ERR_ARG = 9001


# ------------------------------------------------------------------------------------------- 1, 2: indexed augment

@pytest.mark.parametrize("shape", [(8, 8), (12, 16)])
def test_indexed_augment_equals_stacked(shape):
    from scdhip import ops
    H, W = shape
    g = torch.Generator().manual_seed(H * W)
    store = (torch.randn(12, H, W, generator=g) * 30 + 100).to(DEV)
    ids = [11, 0, 3, 3, 7]                                      # out of order, a repeat, B no multiple of anything
    flips = torch.tensor([[1, 0], [0, 1], [1, 1], [0, 0], [1, 1]], dtype=torch.uint8, device=DEV)
    jitter = (1 + 0.05 * torch.randn(5, generator=g)).to(DEV)
    noise = torch.randn(5, H, W, generator=g).to(DEV)
    stacked = store[ids].contiguous()
    for args in ((flips, jitter, None, 0.05, 1234567), (flips, jitter, noise, 0.05, 0), ()):      # () = validation form
        want = ops.augment_tiles(stacked, *args)
        got = ops.augment_tiles_indexed(store, ids, *args)
        assert got.shape == (5, 1, H, W) and got.dtype == torch.float32
        assert torch.equal(got[:, 0], want)
        assert not torch.equal(got[2], got[3]) or not args      # the repeat is augmented per slot (its own flips)
        # a device id tensor, a (N,1,H,W) store and a caller's output buffer are taken alike
        out = torch.full((5, H, W), -7.0, device=DEV)
        again = ops.augment_tiles_indexed(store[:, None], torch.tensor(ids, device=DEV), *args, out=out)
        assert again.data_ptr() == out.data_ptr() and torch.equal(again[:, 0], want)
    assert torch.equal(store[ids], stacked)                     # the store is only read


def test_indexed_augment_tile_offset_is_64_bit():
    """A store of 2^25 + 1 tiles of 8 x 8 is just over 2^31 elements (8 GiB, never filled): the last tile's offset
    does not fit 32 bits."""
    from scdhip import ops
    free = torch.cuda.mem_get_info()[0]
    if free < 12 * 2 ** 30:
        pytest.skip("%.1f GiB free on the device, the 8 GiB store needs 12 GiB of headroom" % (free / 2.0 ** 30))
    N = 2 ** 25 + 1
    store = torch.empty(N, 8, 8, device=DEV)
    g = torch.Generator().manual_seed(3)
    first, last = torch.randn(8, 8, generator=g) * 30 + 100, torch.randn(8, 8, generator=g) * 5 - 40
    store[0], store[N - 1] = first.to(DEV), last.to(DEV)
    flips = torch.tensor([[1, 0], [0, 1]], dtype=torch.uint8, device=DEV)
    jitter = torch.tensor([1.03, 0.97], device=DEV)
    got = ops.augment_tiles_indexed(store, [N - 1, 0], flips, jitter, None, 0.05, 99)
    want = ops.augment_tiles(torch.stack([last, first]).to(DEV), flips, jitter, None, 0.05, 99)
    assert torch.equal(got[:, 0], want)
    del store


# ------------------------------------------------------------------------------------------------- 3, 4: pack_locs

def plain_tiles():
    """Tiles of 0, 1, 30, 31 and 45 rows (K = 30: below, at, one above and well above), fractional and negative
    centres."""
    rs = np.random.RandomState(8)
    tiles = [C.random_rows(rs, n, -20.0, 150.0) for n in (0, 1, 30, 31, 45)]
    tiles[2][3, 0:2] = [-0.5, 127.5]
    tiles[3][30, 0:2] = [-3.75, 0.25]
    return tiles


@pytest.mark.parametrize("trunc", [True, False])
def test_pack_locs_without_rotation_equals_the_host(trunc):
    from scdhip import ops
    from trainer.dataset import scdx16p100 as D
    tiles = plain_tiles()
    rows, offsets = C.csr(tiles)
    ids = [i for i in (4, 0, 1, 2, 3) for _ in range(4)] + [2, 2, 4]
    flips = np.array([[k & 1, k >> 1] for k in range(4)] * 5 + [[1, 0], [1, 0], [0, 1]], np.uint8)
    locs, counts = ops.pack_locs(rows.to(DEV), offsets.to(DEV), ids, torch.from_numpy(flips).to(DEV), None, C.SIZE,
                                 C.K, trunc)
    want_l, want_n = D._pack_locs([D.SCD.flipLocs(tiles[i], fx, fy) for i, (fx, fy) in zip(ids, flips)], trunc=trunc)
    assert locs.dtype == torch.float32 and counts.dtype == torch.int32 and locs.shape == (len(ids), C.K, 8)
    assert torch.equal(counts.cpu(), torch.from_numpy(want_n))
    assert torch.equal(locs.cpu(), torch.from_numpy(want_l))
    assert sorted(set(want_n.tolist())) == [0, 1, 30]
    # without flips, from a device id tensor
    locs, counts = ops.pack_locs(rows.to(DEV), offsets.to(DEV), torch.tensor(ids, device=DEV), K=C.K, trunc=trunc)
    want_l, want_n = D._pack_locs([tiles[i] for i in ids], trunc=trunc)
    assert torch.equal(counts.cpu(), torch.from_numpy(want_n)) and torch.equal(locs.cpu(), torch.from_numpy(want_l))


def test_pack_locs_with_rotation_is_numpy_float32_bit_for_bit():
    """The kernel's float32 rotation is one correctly rounded, uncontracted operation per operation of the host's
    formulas.  numpy's float32 arithmetic is exactly that (tests/resident_case.py rotate_f32), so on every slot, safe or
    not, the un-truncated rows, their order and the counts must be its bits: a fused multiply-add or a 1-ulp sqrt in
    the kernel shows here, which the float64 bound of the next test is too wide to see."""
    from scdhip import ops
    from trainer.dataset import scdx16p100 as D
    tiles, ids, flips, angles = C.rotation_slots()
    rows, offsets = C.csr(tiles)
    rows, offsets, dflips = rows.to(DEV), offsets.to(DEV), torch.from_numpy(flips).to(DEV)
    raw, counts = ops.pack_locs(rows, offsets, ids, dflips, angles, C.SIZE, C.K, False)
    cut, cut_counts = ops.pack_locs(rows, offsets, ids, dflips, angles, C.SIZE, C.K, True)
    raw, counts, cut = raw.cpu().numpy(), counts.cpu().numpy(), cut.cpu().numpy()
    assert np.array_equal(counts, cut_counts.cpu().numpy())
    rows_checked = 0
    for b, (i, (fx, fy), angle) in enumerate(zip(ids, flips, angles)):
        want = C.rotate_f32(D.SCD.flipLocs(tiles[i], fx, fy), angle)[:C.K]
        assert counts[b] == len(want), (b, i, angle)
        np.testing.assert_array_equal(raw[b, :len(want)], want, err_msg="slot %d tile %d angle %s" % (b, i, angle))
        assert not raw[b, len(want):].any()
        want[:, 0:2] = np.trunc(want[:, 0:2])
        np.testing.assert_array_equal(cut[b, :len(want)], want)
        rows_checked += len(want)
    assert rows_checked == 853 and np.isnan(raw).any()      # the seeded case's kept rows, all of them compared


def test_pack_locs_with_rotation_against_rotate_locs():
    from scdhip import ops
    from trainer.dataset import scdx16p100 as D
    tiles, ids, flips, angles = C.rotation_slots()
    rows, offsets = C.csr(tiles)
    rows, offsets, dflips = rows.to(DEV), offsets.to(DEV), torch.from_numpy(flips).to(DEV)
    locs, counts = ops.pack_locs(rows, offsets, ids, dflips, angles, C.SIZE, C.K, True)
    raw, raw_counts = ops.pack_locs(rows, offsets, ids, dflips, angles, C.SIZE, C.K, False)
    assert torch.equal(counts, raw_counts)
    locs, counts, raw = locs.cpu().numpy(), counts.cpu().numpy(), raw.cpu().numpy()
    np.testing.assert_array_equal(locs[:, :, 2:], raw[:, :, 2:])
    np.testing.assert_array_equal(locs[:, :, :2], np.trunc(raw[:, :, :2]))
    unsafe, e_host, e_dev, stored_err, checked, seen = 0, 0.0, 0.0, 0.0, {}, {}
    for b, (i, (fx, fy), angle) in enumerate(zip(ids, flips, angles)):
        flipped = D.SCD.flipLocs(tiles[i], fx, fy)
        want, which, safe = C.rotate_f64(flipped, angle)
        if not safe:
            unsafe += 1
            continue
        host = D.SCD.rotateLocs(flipped, angle)
        assert len(host) == len(want)
        n = min(len(want), C.K)
        assert counts[b] == n, (b, i, angle)
        host, want, which, got = host[:n], want[:n], which[:n], locs[b, :n]
        assert not locs[b, n:].any() and not raw[b, n:].any()                    # zero beyond the count
        np.testing.assert_array_equal(got[:, 0:2], np.trunc(want[:, 0:2]))
        np.testing.assert_array_equal(got[:, 0:2], np.trunc(host[:, 0:2]))
        np.testing.assert_array_equal(got[:, 6:8], host[:, 6:8])
        np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
        np.testing.assert_array_equal(np.isnan(host), np.isnan(want))
        if n:
            e_host = max(e_host, float(np.nanmax(np.abs(host[:, 2:6] - want[:, 2:6]), initial=0.0)))
            e_dev = max(e_dev, float(np.nanmax(np.abs(got[:, 2:6] - want[:, 2:6]), initial=0.0)))
        special = i - len(tiles)
        checked.setdefault(special, []).append(angle)
        if special == C.FULL:
            assert counts[b] == C.K and len(C.rotate_f64(flipped, angle)[0]) > C.K
        if special == C.WIDE:
            assert 9 * len(tiles[i]) > 256
        if special == C.CENTRE:
            at = [j for j in range(n) if tuple(which[j]) == (1, 0)]              # the row on the rotation centre
            assert len(at) == 1 and raw[b, at[0], 0] == 63.5 and raw[b, at[0], 1] == 63.5
            zero = [j for j in range(n) if which[j][0] == 2]                     # the zero offset, and its replicas
            assert not got[zero, 2:4].any()
            seen["zero offset"] = seen.get("zero offset", 0) + len(zero)
        if special == C.NAN:
            nan = [j for j in range(n) if which[j][0] == 0]
            assert np.isnan(got[nan, 4:6]).all() and np.isfinite(got[nan, 0:4]).all()
            seen["zero major axis"] = seen.get("zero major axis", 0) + len(nan)
        if angle == 0.0:
            # angle 0 with cs given: the originals (replica 0) come back as the stored rows (unflipped slots)
            assert not fx and not fy
            own = which[:, 1] == 0
            stored = np.asarray(tiles[i], np.float32)[which[own, 0]]
            np.testing.assert_array_equal(got[own, 0:2], np.trunc(stored[:, 0:2]))
            np.testing.assert_array_equal(got[own, 6:8], stored[:, 6:8])
            ok = (stored[:, 4] != 0) | (stored[:, 5] != 0)                        # a zero major axis is NaN, as above
            stored_err = max(stored_err, float(np.abs(got[own, 2:6][ok] - stored[ok, 2:6]).max(initial=0.0)))
    floor = 2.0 ** -15                                                             # one float32 ulp of 256
    E_host = max(e_host, floor)
    print("pack_locs with rotation: %d of %d slots unsafe; E_host %.3g (the host's own error %.3g, floor %.3g); device "
          "error %.3g; angle 0 against the stored rows %.3g" % (unsafe, len(ids), E_host, e_host, floor, e_dev,
                                                                stored_err))
    assert unsafe <= 0.10 * len(ids)
    assert e_dev <= 4 * E_host and stored_err <= 4 * E_host
    for special in (C.CENTRE, C.NAN, C.WIDE, C.FULL):
        assert {20.0, -35.0} & set(checked[special]), (special, checked[special])
    assert 0.0 in checked[C.CENTRE] and 0.0 in checked[C.NAN]
    assert seen["zero offset"] >= 7 and seen["zero major axis"] >= 7, seen


# ----------------------------------------------------------------------------------------- 5, 8: the dataset's switch

COUNT = 7680      # 20 synthetic slides: the 5760 validation positions and 1920 training tiles


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    """tests/test_rotate_gpu.py's `built`: a 7,680-tile archive of 8 x 8 tiles, constructed with both keys off."""
    from configuration import defaultConfig
    from trainer.dataset import scdx16p100 as D
    d = tmp_path_factory.mktemp("scdres")
    path = str(d / "synthetic.d")
    scd_archive.write(path, count=COUNT, size=8)
    old = dict(defaultConfig.config)
    defaultConfig.config["dirTemp"] = str(d / "temp") + "/"
    defaultConfig.config["dirDataSplitProfile"] = str(d / "split.json")
    try:
        random.seed(77)
        ds = D.SCD(path, True, None)
    finally:
        defaultConfig.config.clear()
        defaultConfig.config.update(old)
    return ds


def batch_with_keys(ds, rotate, resident, indices=None, item=None):
    """gpu_batch(range(32)) (or ds[item]) from fixed seeds of the three generators it draws from -> (batch, the numpy
    and torch generator states afterwards)."""
    from configuration import defaultConfig
    old = dict(defaultConfig.config)
    defaultConfig.config["rotateAugmentation"] = rotate
    defaultConfig.config["residentDataset"] = resident
    ds.order.sort()
    random.seed(5)
    np.random.seed(6)
    torch.manual_seed(7)
    try:
        b = ds[item] if item is not None else ds.gpu_batch(list(range(32)) if indices is None else indices)
        return b, C.host_states()
    finally:
        defaultConfig.config.clear()
        defaultConfig.config.update(old)


def same_batch(a, b):
    assert torch.equal(a["xs"][0], b["xs"][0])
    assert len(a["ys"]) == len(b["ys"]) == 4
    for got, want in zip(a["ys"], b["ys"]):
        assert got.dtype == want.dtype and got.shape == want.shape and torch.equal(got, want)


def test_resident_batch_equals_host_batch(built):
    host, host_after = batch_with_keys(built, 0, False)
    assert not hasattr(built, "resident")
    res, res_after = batch_with_keys(built, 0, True)
    assert built.resident["store"].shape == (COUNT, 8, 8) and built.resident["store"].is_cuda
    assert built.resident["offsets"].shape == (COUNT + 1,) and built.resident["rows"].shape[1] == 8
    x = res["xs"][0]
    assert x.shape == (32, 1, 8, 8) and x.dtype == torch.float32 and bool(torch.isfinite(x).all())
    assert [tuple(y.shape) for y in res["ys"]] == [(32, 1, 128, 128), (32, 30), (32, 30, 6), (32, 30)]
    same_batch(res, host)
    assert int(res["ys"][1].sum()) > 0
    assert C.same_states(res_after, host_after)
    assert len(built.samples) == COUNT and len(built.bounds) == COUNT          # the host copy stays


def test_resident_batch_with_rotation(built):
    from scdhip import ops
    from trainer.dataset import scdx16p100 as D
    host, host_after = batch_with_keys(built, 30, False)
    res, res_after = batch_with_keys(built, 30, True)
    assert torch.equal(res["xs"][0], host["xs"][0])                              # pixels do not depend on labels
    assert C.same_states(res_after, host_after)
    # the labels, composed by hand from the same draws
    ids = [built.order[i] for i in range(32)]
    flips, _, angles, _ = C.draws(30)
    assert len(angles) == 32 and len({round(a, 6) for a in angles}) == 32
    rows, offsets = C.csr(built.bounds)
    locs, counts = ops.pack_locs(rows.to(DEV), offsets.to(DEV), ids, torch.from_numpy(flips).to(DEV), angles,
                                 D.HEATMAPSIZE, D.MAXTAGLEN, True)
    want = ops.render_center_targets(locs, counts, D.HEATMAPSIZE, D.THRESHOLDIOU)
    for got, w in zip(res["ys"], want):
        assert got.dtype == w.dtype and torch.equal(got, w)
    assert int(counts.sum()) > 0 and int(res["ys"][1].sum()) > 0
    plain, _ = batch_with_keys(built, 0, True)
    assert not torch.equal(plain["ys"][0], res["ys"][0])                         # and the rotation did something


class Untouchable:
    """Stands in for the host tiles and labels: any use raises."""

    def _refuse(self, *a, **k):
        raise AssertionError("the resident batch read the host copy")
    __getitem__ = __len__ = __iter__ = __contains__ = _refuse

    def __getattr__(self, name):
        self._refuse()


def test_resident_batch_reads_no_host_tile_or_label(built):
    want0, _ = batch_with_keys(built, 0, True)
    want30, _ = batch_with_keys(built, 30, True)
    bare = copy.copy(built)
    bare.order = list(built.order)
    bare.samples, bare.bounds = Untouchable(), Untouchable()
    assert bare.resident is built.resident
    same_batch(batch_with_keys(bare, 0, True)[0], want0)
    same_batch(batch_with_keys(bare, 30, True)[0], want30)


def test_getitem_in_resident_mode(built):
    item, _ = batch_with_keys(built, 30, True, item=5)
    one, _ = batch_with_keys(built, 30, True, indices=[5])
    assert item["xs"][0].shape == (1, 8, 8) and torch.equal(item["xs"][0], one["xs"][0][0])
    for got, want in zip(item["ys"], one["ys"]):
        assert torch.equal(got, want[0])
    host, _ = batch_with_keys(built, 0, False, item=5)
    res, _ = batch_with_keys(built, 0, True, item=5)
    assert torch.equal(host["xs"][0], res["xs"][0]) and all(torch.equal(a, b) for a, b in zip(host["ys"], res["ys"]))


def test_defaults_unchanged(built, monkeypatch):
    """With the key off neither new op runs, and the batch is the parent's path written out."""
    from scdhip import ops

    def refuse(*a, **k):
        raise AssertionError("a resident-archive op with residentDataset off")
    monkeypatch.setattr(ops, "augment_tiles_indexed", refuse)
    monkeypatch.setattr(ops, "pack_locs", refuse)
    b, after = batch_with_keys(built, 0, False)
    xs, ys = C.replay(built, 0)
    assert C.same_states(after, C.host_states())         # replay's draws are gpu_batch's
    assert torch.equal(b["xs"][0], xs)
    for got, want in zip(b["ys"], ys):
        assert got.dtype == want.dtype and torch.equal(got, want)


# ------------------------------------------------------------------------------------------------------- 6: guards

def test_out_of_range_id_raises_before_any_launch(monkeypatch):
    from scdhip import ops
    store = torch.zeros(12, 8, 8, device=DEV)
    rows, offsets = C.csr(plain_tiles())
    rows, offsets = rows.to(DEV), offsets.to(DEV)

    def refuse(*a, **k):
        raise AssertionError("a launch after an id out of range")
    monkeypatch.setattr(ops.L, "call", refuse)
    for bad in ([0, 12], [-1], [3, 2 ** 31]):
        with pytest.raises(IndexError, match="outside the store's 12 tiles"):
            ops.augment_tiles_indexed(store, bad)
    for bad in ([0, 5], [-1]):
        with pytest.raises(IndexError, match="outside the store's 5 tiles"):
            ops.pack_locs(rows, offsets, bad)


def test_store_that_does_not_fit_raises_and_allocates_nothing(built, monkeypatch):
    fresh = copy.copy(built)
    fresh.order = list(built.order)
    fresh.__dict__.pop("resident", None)
    T = sum(len(b) for b in built.bounds)
    need = COUNT * 8 * 8 * 4 + T * 32 + (COUNT + 1) * 8
    assert need > 2 ** 20
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a, **k: (2 ** 20, 2 ** 38))
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    with pytest.raises(RuntimeError, match="needs %d bytes .* %d bytes are free" % (need, 2 ** 20)):
        batch_with_keys(fresh, 0, True)
    assert not hasattr(fresh, "resident") and torch.cuda.memory_allocated() == before


def test_two_tile_shapes_raise_at_build_time(tmp_path):
    from configuration import defaultConfig
    from trainer.dataset import scdx16p100 as D
    names, samples, locs = scd_archive.archive_content(seed=5, count=48, size=8)
    samples[40] = np.zeros((8, 12), np.float32)
    path = str(tmp_path / "mixed.d")
    D.writeArchive(path, names, samples, locs)
    old = dict(defaultConfig.config)
    defaultConfig.config["dirTemp"] = str(tmp_path / "temp") + "/"
    defaultConfig.config["dirDataSplitProfile"] = str(tmp_path / "split.json")
    try:
        ds = D.SCD(path, True, {"validation": list(range(8))})
    finally:
        defaultConfig.config.clear()
        defaultConfig.config.update(old)
    with pytest.raises(RuntimeError, match="tiles of one shape"):
        batch_with_keys(ds, 0, True, indices=[1, 2])
    assert not hasattr(ds, "resident")


def test_second_device_raises(built):
    batch_with_keys(built, 0, True)
    assert built.resident["device"] == torch.device("cuda", torch.cuda.current_device())
    other = torch.device("cuda", torch.cuda.current_device() + 1)
    from configuration import defaultConfig
    old = dict(defaultConfig.config)
    defaultConfig.config["residentDataset"] = True
    try:
        with pytest.raises(RuntimeError, match="lives on cuda:%d" % torch.cuda.current_device()):
            built.gpu_batch([1, 2], other)
        built.gpu_batch([1, 2], torch.device("cuda"))          # the current device without an index is the same one
    finally:
        defaultConfig.config.clear()
        defaultConfig.config.update(old)


def test_cpu_tensors_are_refused():
    from scdhip import ops
    rows, offsets = C.csr(plain_tiles())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.augment_tiles_indexed(torch.zeros(4, 8, 8), [0])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.augment_tiles_indexed(torch.zeros(4, 8, 8, device=DEV), torch.tensor([0]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.pack_locs(rows, offsets.to(DEV), [0])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.pack_locs(rows.to(DEV), offsets, [0])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.pack_locs(rows.to(DEV), offsets.to(DEV), [0], flips=torch.zeros(1, 2, dtype=torch.uint8))


BAD_AUGMENT = {
    # which pointer is NULL or aliased, nstore, B, H, W
    "null-store": ("store", 4, 1, 8, 8),
    "null-ids": ("ids", 4, 1, 8, 8),
    "null-out": ("out", 4, 1, 8, 8),
    "store-is-out": ("alias", 4, 1, 8, 8),
    "empty-store": (None, 0, 1, 8, 8),
    "no-tile": (None, 4, 0, 8, 8),
    "no-row": (None, 4, 1, 0, 8),
    "two-columns": (None, 4, 1, 8, 2),
    "width-6": (None, 4, 1, 8, 6),
    "tile-of-2^31-pixels": (None, 4, 1, 46340, 46344),
}


@pytest.mark.parametrize("case", sorted(BAD_AUGMENT))
def test_indexed_augment_argument_errors_launch_nothing(case):
    import scdhip.lib as L
    special, nstore, B, H, W = BAD_AUGMENT[case]
    store = torch.zeros(4 * 64, device=DEV)
    out = torch.full((64,), -7.0, device=DEV)
    ids = torch.zeros(1, dtype=torch.int32, device=DEV)
    ws = torch.zeros(L.lib().scd_augment_workspace(1), dtype=torch.uint8, device=DEV)
    ps, pi, po = store.data_ptr(), ids.data_ptr(), out.data_ptr()
    if special == "store":
        ps = 0
    elif special == "ids":
        pi = 0
    elif special == "out":
        po = 0
    elif special == "alias":
        ps = po
    assert L.lib().scd_augment_tiles_indexed(ps, nstore, pi, po, B, H, W, 0, 0, 0, 0.0, 0, ws.data_ptr(), 0) == ERR_ARG
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())


@pytest.mark.parametrize("case", ["null-rows", "null-offsets", "null-ids", "null-locs", "null-counts", "no-tile",
                                  "no-size", "no-slot", "65-slots"])
def test_pack_locs_argument_errors_launch_nothing(case):
    import scdhip.lib as L
    rows, offsets = C.csr(plain_tiles())
    rows, offsets = rows.to(DEV), offsets.to(DEV)
    ids = torch.zeros(1, dtype=torch.int32, device=DEV)
    locs = torch.full((65 * 8,), -7.0, device=DEV)
    counts = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    p = {"rows": rows.data_ptr(), "offsets": offsets.data_ptr(), "ids": ids.data_ptr(), "locs": locs.data_ptr(),
         "counts": counts.data_ptr()}
    B, size, K = 1, 128, 30
    if case.startswith("null-"):
        p[case[5:]] = 0
    elif case == "no-tile":
        B = 0
    elif case == "no-size":
        size = 0
    elif case == "no-slot":
        K = 0
    elif case == "65-slots":
        K = 65
    assert L.lib().scd_pack_locs(p["rows"], p["offsets"], p["ids"], B, 0, 0, size, K, 1, p["locs"], p["counts"],
                                 0) == ERR_ARG
    torch.cuda.synchronize()
    assert bool((locs == -7.0).all()) and int(counts[0]) == -7
