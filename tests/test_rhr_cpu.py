"""scdhip.rhr against the reference's recipe recorded in tests/golden/rhr.npz
(tests/golden/make_golden_rhr.py: curve_fit(gauss2, xs, ys, bounds=pbounds2, maxfev=5000) at its default and at
1e-15 tolerances).  No scipy here: the npz is the reference.

Bounds of the comparisons:
  * SSE: fit.sse <= sse_ref * (1 + 1e-9) on every fixture: at least as good as the reference's recipe; 1e-9 is
    rounding slack only.
  * parameters, where the reference pins them down (`checked`: its two tolerances agree within 1e-5) and the fit
    reached the same minimum (|sse - sse_tight| <= 1e-9 sse_tight): max |p - p_tight| <= ptol, ptol = 10 x the
    largest checked spread, recorded in the npz.
  * DFI: first-order bound derived in test_dfi_on_checked_fixtures.
"""
import numpy as np
import pytest

from scdhip import rhr


def test_no_scipy_in_the_product():
    assert "import scipy" not in open(rhr.__file__).read() and "from scipy" not in open(rhr.__file__).read()


@pytest.fixture(scope="module")
def gold(golden):
    return golden("rhr")


@pytest.fixture(scope="module")
def fits(gold):
    return [rhr.fit_gauss2(rhr.frequencies(h)) for h in gold["hist"]]


def compared(gold, fits):
    """Indices where the parameter comparison applies."""
    return [i for i, f in enumerate(fits)
            if gold["checked"][i] and abs(f.sse - gold["sse_tight"][i]) <= 1e-9 * gold["sse_tight"][i]]


def test_fixture_shape(gold):
    n = gold["hist"].shape[0]
    assert n >= 36 and gold["hist"].shape == (n, rhr.BINS) and gold["hist"].dtype == np.int64
    assert 3 * int(gold["checked"].sum()) >= 2 * n
    np.testing.assert_array_equal(gold["checked"], gold["spread"] <= 1e-5)
    assert float(gold["ptol"]) == 10.0 * gold["spread"][gold["checked"]].max() <= 1e-4
    shares = gold["cases"][:, 1]
    assert (shares == 0).any() and (shares == 1).any()
    assert set(gold["cases"][:, 0].astype(int)) == {60, 100, 500, 3000, 20000}


def test_sse_not_worse_than_reference_on_every_fixture(gold, fits):
    for i, f in enumerate(fits):
        print("case %2d  sse %.9e  sse_ref %.9e  sse/sse_ref - 1 = %+.3e" % (i, f.sse, gold["sse_ref"][i],
                                                                             f.sse / gold["sse_ref"][i] - 1))
    for i, f in enumerate(fits):
        assert f.converged, i
        assert f.sse == float(np.sum((rhr.gauss2(rhr.xs(), f.params) - rhr.frequencies(gold["hist"][i])) ** 2)), i
        assert f.sse <= gold["sse_ref"][i] * (1 + 1e-9), (i, f.sse, gold["sse_ref"][i])


def test_parameters_on_checked_fixtures(gold, fits):
    ptol = float(gold["ptol"])
    idx = compared(gold, fits)
    for i in idx:
        print("case %2d  max|p - p_tight| = %.3e  (ptol %.3e)" % (i, np.max(np.abs(fits[i].params - gold["p_tight"][i])),
                                                                 ptol))
    assert 3 * len(idx) >= 2 * len(fits), (len(idx), len(fits))
    for i in idx:
        assert np.max(np.abs(fits[i].params - gold["p_tight"][i])) <= ptol, i


def test_dfi_on_checked_fixtures(gold, fits):
    """d = u / (u + w), u = a1 s1, w = a2 s2.  With every parameter within ptol of the reference's:
    |du| <= ptol (a1 + s1) + ptol^2, |dw| <= ptol (a2 + s2) + ptol^2, and since dd/du = w / (u+w)^2,
    dd/dw = -u / (u+w)^2, to first order |dd| <= (w |du| + u |dw|) / (u+w)^2.  The second-order remainder is
    bounded by taking the derivative's denominator at its smallest over the box, (u + w - |du| - |dw|)^2."""
    ptol = float(gold["ptol"])
    idx = compared(gold, fits)
    assert 3 * len(idx) >= 2 * len(fits)
    for i in idx:
        a1, _, s1, a2, _, s2 = gold["p_tight"][i]
        u, w = a1 * s1, a2 * s2
        du, dw = ptol * (a1 + s1) + ptol * ptol, ptol * (a2 + s2) + ptol * ptol
        den = u + w - du - dw
        assert den > 0, i
        bound = ((w + dw) * du + (u + du) * dw) / (den * den)
        got, ref = rhr.dfi(fits[i].params), rhr.dfi(gold["p_tight"][i])
        print("case %2d  dfi %.9f  ref %.9f  |d| %.3e  bound %.3e" % (i, got, ref, abs(got - ref), bound))
        assert abs(got - ref) <= bound, (i, got, ref, bound)


def test_parameters_inside_bounds(fits):
    for i, f in enumerate(fits):
        assert f.params.shape == (6,) and np.all(np.isfinite(f.params)), i
        assert np.all(f.params >= rhr.LOWER) and np.all(f.params <= rhr.UPPER), (i, f.params)


def test_bounds_and_start_are_the_references():
    np.testing.assert_array_equal(rhr.LOWER, [0, -0.25, 0, 0, 0, 0])
    np.testing.assert_array_equal(rhr.UPPER, [1, 0.33, 0.2, 1, 1.25, 1])
    np.testing.assert_array_equal(rhr._starts()[0], 0.5 * (rhr.LOWER + rhr.UPPER))


def test_deterministic(gold):
    for i in (0, 3, 27):
        ys = rhr.frequencies(gold["hist"][i])
        a, b = rhr.fit_gauss2(ys), rhr.fit_gauss2(ys.copy())
        assert a.params.tobytes() == b.params.tobytes()
        assert a.sse == b.sse and a.iterations == b.iterations and a.converged == b.converged


def test_xs_are_the_left_bin_edges():
    x = rhr.xs()
    assert x.shape == (150,) and x.dtype == np.float64
    assert x.tolist() == [(i - 25) / 100 for i in range(150)]
    assert (rhr.BINS, rhr.LO, rhr.SCALE) == (150, -0.25, 100.0)


def test_frequencies():
    h = np.zeros(150, np.int64)
    with pytest.raises(ValueError):
        rhr.frequencies(h)
    with pytest.raises(ValueError):
        rhr.frequencies(np.zeros(0, np.int64))
    h[[3, 7]] = [1, 3]
    f = rhr.frequencies(h)
    assert f.dtype == np.float64 and f[3] == 0.25 and f[7] == 0.75 and f.sum() == 1.0


def test_binning_expression_at_the_edges():
    """b = floor((r - LO) * SCALE) in float64; -1 = not counted.  0.01 k: (0.01 k + 0.25) * 100 is 26, 27 and 28
    to rounding, and the expected bins below are that float64 expression evaluated by hand: 0.01 + 0.25 = 0.26
    and 0.26 * 100 = 26.000000000000004 -> 26; 0.02 + 0.25 = 0.27, * 100 = 27.0 -> 27; 0.03 + 0.25 = 0.28,
    * 100 = 28.000000000000004 -> 28."""
    r = np.array([-0.25, 1.25, -0.2500001, 0.01, 0.02, 0.03, np.inf, -np.inf, np.nan, 1.2499999, 0.0])
    want = [0, -1, -1, 26, 27, 28, -1, -1, -1, 149, 25]
    assert rhr.bin_index(r).tolist() == want
    for v, b in zip(r, want):
        e = (float(v) - (-0.25)) * 100.0
        ok = np.isfinite(v) and 0 <= np.floor(e) < 150
        assert (int(np.floor(e)) if ok else -1) == b


def test_dfi_by_hand():
    assert rhr.dfi([0.5, 0.0, 0.1, 0.5, 0.5, 0.1]) == 0.5
    assert rhr.dfi([0.2, 0.1, 0.1, 0.1, 0.6, 0.6]) == pytest.approx(0.02 / 0.08, abs=1e-15)
    assert rhr.dfi([0.0, 0.1, 0.1, 0.3, 0.5, 0.2]) == 0.0
    assert rhr.dfi([0.3, 0.1, 0.1, 0.0, 0.5, 0.2]) == 1.0
    with pytest.raises(ValueError):
        rhr.dfi([0.0, 0.1, 0.1, 0.0, 0.5, 0.2])
    assert "project" in rhr.dfi.__doc__ and "paper" in rhr.dfi.__doc__
    # area: a s sqrt(pi), checked by quadrature on a wide grid
    x = np.linspace(-5, 5, 200001)
    area = np.sum(0.3 * np.exp(-((x - 0.2) / 0.4) ** 2)) * (x[1] - x[0])
    assert area == pytest.approx(0.3 * 0.4 * np.sqrt(np.pi), rel=1e-9)
