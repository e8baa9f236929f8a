"""Random-angle rotation augmentation, host side, CPU only: SCD.rotateLocs against the reference's own
rotateCoordinates on the replicated rows (tests/golden/rotaug.npz, tests/golden/make_golden_rotaug.py), the
configuration key, and the random draws of SCD._draws.

rotateLocs goes through datasets.preprocessor.scdManual.rotateCoordinates, the reference's float32 torch arithmetic in
the reference's order.  Counts and order must equal the reference's; values within atol 1e-4 in heatmap units, the
float32 agreement tests/test_preprocess_gpu.py asks of rotated labels.  Where the fixture was made the rows are equal
bit for bit, but that is no property to assert: torch's vectorised float32 sqrt / divide differ in the last bit between
CPUs (8 of 312 values by one ulp of 64, 7.6e-6, on another host).  The fixture's generator asserts that no rotated
centre lies within 1e-3 of an integer, so the kept set does not hang on such a bit."""
import contextlib

import numpy as np
import torch

from trainer.dataset import scdx16p100 as D


@contextlib.contextmanager
def rotate_key(value):
    from configuration import defaultConfig
    old = dict(defaultConfig.config)
    defaultConfig.config["rotateAugmentation"] = value
    try:
        yield
    finally:
        defaultConfig.config.clear()
        defaultConfig.config.update(old)


def test_rotate_locs_vs_reference_rows(golden):
    g = golden("rotaug")
    rows = g["loc_rows"]
    before = rows.copy()
    start = 0
    for angle, n in zip(g["angles"].tolist(), g["loc_count"].tolist()):
        want = g["loc_out"][start:start + n]
        start += n
        for given in (rows, torch.from_numpy(rows.copy())):
            got = D.SCD.rotateLocs(given, angle)
            assert got.dtype == np.float32 and got.shape == want.shape, (angle, got.shape, want.shape)
            np.testing.assert_allclose(got, want, rtol=0, atol=1e-4, err_msg="angle %s" % angle)
            np.testing.assert_array_equal(np.trunc(got[:, 0:2]), np.trunc(want[:, 0:2]))      # the cells drawn into
    np.testing.assert_array_equal(rows, before)        # the caller's rows are not mutated
    assert start == len(g["loc_out"])
    # replicas did enter the map: more rows than objects at 0 and 90 degrees, and other counts elsewhere
    assert g["loc_count"][0] > len(rows) and len(set(g["loc_count"].tolist())) > 3


def test_angle_zero_returns_in_range_originals_unchanged():
    rs = np.random.RandomState(5)
    rows = rs.uniform(-6, 6, (12, 8)).astype(np.float32)
    rows[:, 0:2] = rs.uniform(0.25, 126.75, (12, 2))          # centres below 127: no replica lands in the map
    rows[3, 2:4] = 0
    rows[7, 0], rows[9, 1] = 300.0, -200.0                    # far outside the map: dropped, replicas too
    got = D.SCD.rotateLocs(rows, 0.0)
    keep = [i for i in range(12) if i not in (7, 9)]
    assert got.shape == (10, 8)
    # the centre goes through distance * (x / distance) in float32: a few ulps of 64, everything else is exact
    np.testing.assert_allclose(got[:, 0:2], rows[keep, 0:2], rtol=0, atol=4 * 2.0 ** -17)
    np.testing.assert_allclose(got[:, 2:6], rows[keep, 2:6], rtol=0, atol=4 * 2.0 ** -21)
    np.testing.assert_array_equal(got[:, 6:8], rows[keep, 6:8])
    np.testing.assert_array_equal(got[3, 2:4], [0, 0])        # row 3's zero offset stays zero
    assert D.SCD.rotateLocs(np.zeros((0, 8), np.float32), 12.0).shape == (0, 8)
    # other map sizes: the centre of a size-64 map is 31.5
    small = D.SCD.rotateLocs(np.array([[40.0, 31.5, 1, 0, 2, 0, 1, 1]], np.float32), 90.0, size=64)
    np.testing.assert_allclose(small[0, :6], [31.5, 23.0, 0, -1, 0, -2], rtol=0, atol=1e-5)


def test_centre_at_distance_zero_stays_finite():
    rows = np.array([[63.5, 63.5, 1.0, 2.0, 3.0, -1.0, 2.0, 4.0], [10.0, 20.0, 0.0, 0.0, 1.0, 1.0, 1.0, 2.0]],
                    np.float32)
    for angle in (0.0, 30.0, -77.0):
        got = D.SCD.rotateLocs(rows, angle)
        assert np.isfinite(got).all()
        np.testing.assert_array_equal(got[0, 0:2], [63.5, 63.5])
        a = np.deg2rad(-angle)
        np.testing.assert_allclose(got[0, 2:6], [np.cos(a) - 2 * np.sin(a), 2 * np.cos(a) + np.sin(a),
                                                 3 * np.cos(a) + np.sin(a), -np.cos(a) + 3 * np.sin(a)],
                                   rtol=0, atol=1e-5)
        np.testing.assert_array_equal(got[0, 6:8], [2.0, 4.0])


def test_config_key_defaults_to_zero():
    from configuration import Configuration, defaultConfig
    assert Configuration().config["rotateAugmentation"] == 0.0
    assert Configuration().rotateAugmentation == 0.0 and defaultConfig.rotateAugmentation == 0.0
    c = Configuration()
    c.updateConfig({"rotateAugmentation": 30})
    assert c.rotateAugmentation == 30.0 and isinstance(c.rotateAugmentation, float)


def parent_draws(B):
    """SCD._draws as it was before the rotation existed."""
    flips = np.zeros((B, 2), np.uint8)
    jit = np.zeros(B, np.float32)
    for b in range(B):
        flips[b, 0] = np.random.uniform() > 0.5
        flips[b, 1] = np.random.uniform() > 0.5
        jit[b] = np.float32(1) + np.float32(D.JITTERSV) * torch.randn(1).numpy()[0]
    seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    return flips, jit, seed


def states():
    return np.random.get_state(), torch.get_rng_state()


def same_states(a, b):
    return a[0][0] == b[0][0] and np.array_equal(a[0][1], b[0][1]) and a[0][2:] == b[0][2:] and torch.equal(a[1], b[1])


def test_draws_with_the_key_at_zero_leave_the_generators_where_the_parent_did():
    ds = D.SCD.__new__(D.SCD)          # _draws needs no archive (and the constructor needs a GPU)
    np.random.seed(123)
    torch.manual_seed(456)
    want = parent_draws(7)
    after_parent = states()
    np.random.seed(123)
    torch.manual_seed(456)
    with rotate_key(0.0):
        flips, jit, seed, angles = ds._draws(7)
    assert angles is None and seed == want[2]
    np.testing.assert_array_equal(flips, want[0])
    np.testing.assert_array_equal(jit, want[1])
    assert same_states(states(), after_parent)


def test_draws_with_the_key_on_take_one_more_numpy_uniform_per_sample():
    ds = D.SCD.__new__(D.SCD)
    np.random.seed(123)
    u = np.random.uniform(size=(7, 3))
    after_numpy = np.random.get_state()
    np.random.seed(123)
    torch.manual_seed(456)
    want = parent_draws(7)              # torch draws are the same with the key on or off
    after_torch = torch.get_rng_state()
    np.random.seed(123)
    torch.manual_seed(456)
    with rotate_key(2):
        flips, jit, seed, angles = ds._draws(7)
    np.testing.assert_array_equal(flips, u[:, 0:2] > 0.5)
    np.testing.assert_array_equal(angles, u[:, 2] * 4 - 2)        # the reference's uniform() * 4 - 2 at R = 2
    np.testing.assert_array_equal(jit, want[1])
    assert seed == want[2] and angles.dtype == np.float64 and (np.abs(angles) <= 2).all()
    assert same_states((np.random.get_state(), torch.get_rng_state()), (after_numpy, after_torch))


def test_family_plugins_carry_rotate_locs():
    from trainer.dataset import scdx1p5, scdx8p50
    for mod in (scdx1p5, scdx8p50):
        assert issubclass(mod.SCD, D.SCD) and mod.SCD.rotateLocs is D.SCD.rotateLocs
        assert mod.SCD._draws is D.SCD._draws and mod.SCD.gpu_batch is D.SCD.gpu_batch
