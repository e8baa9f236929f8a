"""Device-resident `.d` archive, host side, CPU only: the configuration key and that every scdx{N}p{M}
plugin serves its batches through the one gpu_batch that reads it."""
import importlib

from trainer.dataset import scdx16p100 as D


def test_config_key_defaults_to_false():
    from configuration import Configuration, defaultConfig
    assert Configuration().config["residentDataset"] is False
    assert Configuration().residentDataset is False and defaultConfig.residentDataset is False


def test_overlay_accepts_the_key():
    from configuration import Configuration
    c = Configuration()
    c.updateConfig({"residentDataset": True, "residentDatasets": True})
    assert c.residentDataset is True and "residentDatasets" not in c.config
    c.updateConfig({"residentDataset": 0})
    assert c.residentDataset is False


def test_rotation_case_is_settled_by_the_host_alone():
    """A check of the fixture, not of the feature (it runs none of its code and passes without it): the seed of the
    rotation case is settled here, on the CPU, before any device run.
    The seeded tiles tests/test_resident_gpu.py rotates on the device (tests/resident_case.py): at most 10 % of the
    (tile, angle) slots are unsafe, every special tile is safe at two angles or more, and on the safe slots the host's
    SCD.rotateLocs keeps the candidates the float64 evaluation keeps, with equal truncated centres and the NaN of the
    zero major axis in the same place."""
    import numpy as np
    import resident_case as C
    tiles, ids, flips, angles = C.rotation_slots()
    assert len(ids) == len(C.ANGLES) * len(tiles) == 238
    assert [len(tiles[i]) for i in (C.CENTRE, C.NAN, C.WIDE, C.FULL)] == [3, 2, 40, 45]
    assert 0 in {len(t) for t in tiles[:30]}
    unsafe, safe_at = 0, {}
    for i, (fx, fy), angle in zip(ids, flips, angles):
        rows = D.SCD.flipLocs(tiles[i], fx, fy)
        want, which, safe = C.rotate_f64(rows, angle)
        if not safe:
            unsafe += 1
            continue
        safe_at.setdefault(i - len(tiles), []).append(angle)
        got = D.SCD.rotateLocs(rows, angle)
        assert got.shape == want.shape, (i, angle)
        np.testing.assert_array_equal(np.trunc(got[:, 0:2]), np.trunc(want[:, 0:2]))
        np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
        np.testing.assert_array_equal(got[:, 6:8], want[:, 6:8].astype(np.float32))
        if i == len(tiles) + C.FULL:
            assert len(want) > C.K
    print("unsafe slots: %d of %d" % (unsafe, len(ids)))
    assert unsafe <= 0.10 * len(ids)
    for special in (C.CENTRE, C.NAN, C.WIDE, C.FULL):
        assert len(safe_at.get(special, [])) >= 2, (special, safe_at.get(special))
        assert {20.0, -35.0} & set(safe_at[special]), (special, safe_at[special])       # a turn that is no mirror
    assert 0.0 in safe_at[C.CENTRE] and 0.0 in safe_at[C.NAN]


def test_all_25_plugins_share_the_one_gpu_batch():
    mods = [importlib.import_module("trainer.dataset.scdx%dp%d" % (n, m))
            for n in (1, 4, 8, 12, 16) for m in (5, 10, 25, 50, 100)]
    assert len(mods) == 25
    for mod in mods:
        assert issubclass(mod.SCD, D.SCD) and mod.dataset is mod.SCD
        assert mod.SCD.gpu_batch is D.SCD.gpu_batch and mod.SCD._draws is D.SCD._draws
        assert mod.SCD._resident_batch is D.SCD._resident_batch and mod.SCD._buildResident is D.SCD._buildResident
        assert mod.SCD.__getitem__ is D.SCD.__getitem__
