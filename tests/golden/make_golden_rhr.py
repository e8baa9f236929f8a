"""Golden fixture for the two-Gaussian Rhr fit, from the REAL reference recipe (build container only).

Run:  python tests/golden/make_golden_rhr.py      (needs /root/reference and scipy; the tests read only the npz)

Imports the reference's test.py the way make_golden_slide.py does (torch.jit.load stubbed for the import only) and
takes its gauss2.  A fixed, seeded list of histograms is drawn from two normal populations (sizes 60 .. 20000;
shares, means and widths spread over the fit's bounds, shares 0 and 1 and overlapping components among them) and
binned with b = floor((r - LO) * SCALE), 0 <= b < 150.  Per case, with ys = hist / hist.sum() and the reference's
xs = (i - 25) / 100 and bounds (test.py:174-178):
  hist        (N, 150) int64
  p_ref       (N, 6)   curve_fit(gauss2, xs, ys, bounds=pbounds2, maxfev=5000)          -- the reference's call
  sse_ref     (N,)     its residual sum of squares
  p_tight, sse_tight   the same call with ftol = xtol = gtol = 1e-15
  spread      (N,)     max |p_ref - p_tight|
  checked     (N,)     spread <= 1e-5: the reference recipe itself pins the parameters down
and once: ptol = 10 * max(spread over checked cases) (the factor 10: another solver stops on another criterion),
cases (N, 7) the generating [n, share, m1, s1, m2, s2, seed].
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"

sys.dont_write_bytecode = True
for _n in ["torchvision", "torchvision.transforms", "torchvision.transforms.functional"]:
    sys.modules[_n] = types.ModuleType(_n)
sys.modules["torchvision"].transforms = sys.modules["torchvision.transforms"]
sys.modules["torchvision.transforms"].functional = sys.modules["torchvision.transforms.functional"]
sys.path.insert(0, REF)
sys.path.insert(1, REPO)

import torch  # noqa: E402
import torch.jit  # noqa: E402
from scipy.optimize import curve_fit  # noqa: E402


class _Dummy:
    def eval(self):
        return self


_load = torch.jit.load
torch.jit.load = lambda *a, **k: _Dummy()
try:
    import test as ref_test  # noqa: E402  (reference test.py)
finally:
    torch.jit.load = _load

BINS, LO, SCALE = 150, -0.25, 100.0
PBOUNDS2 = ([0, -0.25, 0, 0, 0, 0], [1, 0.33, 0.2, 1, 1.25, 1])   # test.py:177

# (n, share of population 1, m1, sd1, m2, sd2): population sd; the model's s is sd * sqrt(2)
CASES = [
    (60, 0.5, 0.05, 0.03, 0.60, 0.10), (60, 0.2, 0.10, 0.05, 0.45, 0.08), (60, 0.8, 0.00, 0.04, 0.70, 0.15),
    (60, 0.0, 0.05, 0.03, 0.50, 0.10), (60, 1.0, 0.10, 0.04, 0.50, 0.10), (60, 0.5, 0.20, 0.06, 0.35, 0.08),
    (100, 0.3, 0.05, 0.03, 0.55, 0.12), (100, 0.6, 0.12, 0.05, 0.50, 0.10), (100, 0.1, 0.02, 0.02, 0.40, 0.09),
    (100, 0.9, 0.15, 0.06, 0.80, 0.10), (100, 0.0, 0.10, 0.03, 0.30, 0.06), (100, 1.0, 0.05, 0.05, 0.60, 0.10),
    (100, 0.5, 0.25, 0.08, 0.40, 0.10), (100, 0.4, -0.05, 0.05, 0.90, 0.12),
    (500, 0.5, 0.05, 0.03, 0.60, 0.10), (500, 0.25, 0.10, 0.04, 0.45, 0.08), (500, 0.75, 0.08, 0.05, 0.75, 0.20),
    (500, 0.0, 0.05, 0.03, 0.55, 0.12), (500, 1.0, 0.12, 0.05, 0.50, 0.10), (500, 0.5, 0.22, 0.07, 0.38, 0.09),
    (500, 0.15, 0.00, 0.03, 0.30, 0.15), (500, 0.6, 0.30, 0.10, 1.00, 0.10),
    (3000, 0.5, 0.05, 0.03, 0.60, 0.10), (3000, 0.3, 0.10, 0.05, 0.50, 0.12), (3000, 0.7, 0.15, 0.06, 0.65, 0.08),
    (3000, 0.0, 0.05, 0.03, 0.45, 0.10), (3000, 1.0, 0.08, 0.04, 0.50, 0.10), (3000, 0.5, 0.20, 0.08, 0.35, 0.12),
    (3000, 0.05, 0.05, 0.02, 0.70, 0.25), (3000, 0.95, 0.10, 0.08, 0.90, 0.05),
    (20000, 0.5, 0.05, 0.03, 0.60, 0.10), (20000, 0.2, 0.12, 0.05, 0.50, 0.15), (20000, 0.8, 0.10, 0.06, 0.55, 0.10),
    (20000, 0.0, 0.05, 0.03, 0.60, 0.20), (20000, 1.0, 0.15, 0.10, 0.50, 0.10), (20000, 0.5, 0.18, 0.07, 0.32, 0.10),
    (20000, 0.35, 0.00, 0.04, 0.25, 0.05), (20000, 0.6, 0.28, 0.12, 1.10, 0.08),
    (100, 0.5, 0.08, 0.04, 0.65, 0.10), (100, 0.7, 0.03, 0.03, 0.50, 0.14), (500, 0.4, 0.02, 0.04, 0.50, 0.10),
    (500, 0.65, 0.14, 0.05, 0.85, 0.12), (500, 0.1, 0.06, 0.02, 0.60, 0.18), (500, 0.85, 0.18, 0.07, 0.70, 0.06),
    (3000, 0.4, -0.02, 0.05, 0.40, 0.08), (3000, 0.6, 0.12, 0.04, 0.95, 0.10), (3000, 0.15, 0.20, 0.05, 0.60, 0.15),
    (3000, 0.85, 0.06, 0.06, 0.45, 0.05), (20000, 0.45, 0.10, 0.03, 0.70, 0.18), (20000, 0.1, 0.16, 0.04, 0.80, 0.12),
    (100, 0.35, 0.10, 0.03, 0.75, 0.12), (500, 0.55, 0.00, 0.05, 0.60, 0.09), (500, 0.3, 0.15, 0.04, 1.00, 0.14),
    (3000, 0.25, 0.04, 0.03, 0.55, 0.20), (3000, 0.75, 0.16, 0.05, 0.60, 0.10), (20000, 0.65, 0.02, 0.05, 0.48, 0.07),
]


def histogram(n, share, m1, sd1, m2, sd2, seed):
    rs = np.random.RandomState(seed)
    n1 = int(round(n * share))
    r = np.concatenate([rs.normal(m1, sd1, n1), rs.normal(m2, sd2, n - n1)])
    b = np.floor((r - LO) * SCALE)
    ok = np.isfinite(r) & (b >= 0) & (b < BINS)
    return np.bincount(b[ok].astype(np.int64), minlength=BINS).astype(np.int64)


def main():
    gauss2 = ref_test.gauss2
    xs = [(x - 25) / 100 for x in range(150)]                       # test.py:174
    out = {k: [] for k in ("hist", "p_ref", "sse_ref", "p_tight", "sse_tight", "spread", "checked", "cases")}
    for i, c in enumerate(CASES):
        seed = 1000 + i
        h = histogram(*c, seed)
        ys = h / h.sum()
        p_ref, _ = curve_fit(gauss2, xs, ys, bounds=PBOUNDS2, maxfev=5000)
        p_tight, _ = curve_fit(gauss2, xs, ys, bounds=PBOUNDS2, maxfev=5000, ftol=1e-15, xtol=1e-15, gtol=1e-15)
        sse = [float(np.sum((gauss2(np.array(xs), *p) - ys) ** 2)) for p in (p_ref, p_tight)]
        spread = float(np.max(np.abs(p_ref - p_tight)))
        for k, v in zip(out, (h, p_ref, sse[0], p_tight, sse[1], spread, spread <= 1e-5, list(c) + [seed])):
            out[k].append(v)
        print("%2d n=%5d share=%.2f  sse_ref %.6e  tight/ref-1 %+.2e  spread %.2e  %s" % (
            i, c[0], c[1], sse[0], sse[1] / sse[0] - 1, spread, "checked" if spread <= 1e-5 else "-"))
    arr = {k: np.array(v) for k, v in out.items()}
    arr["hist"] = arr["hist"].astype(np.int64)
    nchk = int(arr["checked"].sum())
    assert len(CASES) >= 36 and 3 * nchk >= 2 * len(CASES), (nchk, len(CASES))
    arr["ptol"] = np.float64(10.0 * arr["spread"][arr["checked"]].max())
    np.savez_compressed(os.path.join(HERE, "rhr.npz"), **arr)
    print("cases %d  checked %d  ptol %.3e" % (len(CASES), nchk, float(arr["ptol"])))


if __name__ == "__main__":
    main()
