"""Cases and bar for the reverse mode of `approx` (approx_vjp_kernel: Context.approx_vjp, Dataset.logpdf_theta_grad(approx_on="device")), shared by
the CPU tests (the numpy twin and its seeded mistakes, tests/test_theta_grad_host.py) and the GPU tests (tests/test_gpu_theta_grad.py).  A plain
module, no fixtures.

combos()   J in {2, 3, 20, 33} (2: the least the setup accepts; 33: odd, a multiple of nothing) x both models x both bases x both normalisations,
           six draws each, and the smallest grids whose LU factorisation interchanges rows at F_MIN, F_MAX (SHO J = 48: 21 interchanges,
           DRWCelerite J = 72: 34; condition numbers 2e5 and 5e5), both models, two draws each: the only cases that reach the row interchanges of
           the transposed solve.
draws()    theta as bench.py's prior draws it (alpha1 ~ U(-0.25, 2), f1 log-uniform in [f_min, f_max], alpha2 ~ U(1.5, 4), variance log-normal;
           the second bend f2 = f1 10^U(0.2, 1.5), alpha3 ~ U(2, 6)), with alpha1 < 0 in draw 1, f1 = f_min in draw 2, f1 = f_max in draw 3 and, for
           the double bend, f2 = 1.05 f1 in draw 0.
truth()    tests/golden/approx_vjp_truth.npz (tools/make_approx_vjp_truth.py: approx restated in mpmath at 50 digits, differentiated by a complex
           step of 1e-30): the draws and every da_j/dtheta_k, db_j/dtheta_k, da_j/dnorm, db_j/dnorm.
batch()    B rows for a launch: the combo's draws in turn, each row with a cotangent (ga, gb) of its own — the truth is the Jacobian, so any
           cotangent and any B has its truth.

The bar, in the natural scale of each output: for output k of a row, S_k = sum_j |ga_j| |da_j/dtheta_k| + |gb_j| |db_j/dtheta_k| (the sum of the
absolute terms of the sum that defines it), and |got_k - truth_k| <= max(MARGIN x dev, FLOOR) x S_k.  dev (ref_dev()) is the largest deviation in
the same scale of the fp64 reference that is not the code under test — approx_batch_vjp, the host complex step through numpy's solve — from the
same truth over the same cases (the six-draw batch of every combo with the cotangent of batch(combo, 6)).  MARGIN = 20 and FLOOR = 256 eps are
those of tests/grad_cases.py, for the reason given there: the kernel forms the same sums in another order."""
import functools
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tools"))

MARGIN, FLOOR = 20.0, 256 * np.finfo(float).eps
F_MIN, F_MAX = 1e-3, 1.0
S_LOW = S_HIGH = 20.0
SIZES = (2, 3, 20, 33)
PIVOTING = ((48, 0), (72, 1))            # (J, basis) of the smallest grids with row interchanges
LAUNCH_B = (1, 63, 64, 65, 130)          # around the 64-thread block of the kernel, and more than two blocks
BASIS_NAME = ("SHO", "DRWCelerite")


def combos():
    """(model, basis, integrated, J, number of draws)"""
    out = [(m, b, i, J, 6) for J in SIZES for m in (0, 1) for b in (0, 1) for i in (1, 0)]
    return out + [(m, b, 1, J, 2) for J, b in PIVOTING for m in (0, 1)]


def name(combo):
    m, b, i, J, _ = combo
    return f"m{m}_b{b}_i{i}_J{J}"


def draws(combo):
    """(theta [n][P], norm [n]) of a combo (what the truth file was made from)"""
    m, b, i, J, n = combo
    rng = np.random.default_rng([20260, m, b, i, J])
    a1 = rng.uniform(-0.25, 2.0, n)
    f1 = np.exp(rng.uniform(np.log(F_MIN), np.log(F_MAX), n))
    a2 = rng.uniform(1.5, 4.0, n)
    norm = np.exp(np.log(0.5) + 1.25 * rng.standard_normal(n))
    ratio = 10.0 ** rng.uniform(0.2, 1.5, n)
    a3 = rng.uniform(2.0, 6.0, n)
    a1[1] = -0.2
    if n > 3:
        f1[2], f1[3] = F_MIN, F_MAX
    ratio[0] = 1.05
    th = np.column_stack([a1, f1, a2] if m == 0 else [a1, f1, a2, f1 * ratio, a3])
    return np.ascontiguousarray(th), norm


@functools.lru_cache(maxsize=None)
def _file():
    with np.load(ROOT / "tests" / "golden" / "approx_vjp_truth.npz") as z:
        return {k: z[k] for k in z.files}


def truth(combo):
    """theta [n][P], norm [n], dA, dB [n][Jt][P + 1] (the last: d/dnorm) of a combo"""
    z, k = _file(), name(combo)
    return z[k + "/theta"], z[k + "/norm"], z[k + "/dA"], z[k + "/dB"]


def batch(combo, B, zero=False):
    """(theta [B][P], norm [B], ga, gb [B][Jt], truth [B][P + 1], S [B][P + 1]) — the combo's draws in turn, a normal cotangent per row (zero: 0)"""
    th, nm, dA, dB = truth(combo)
    idx = np.arange(B) % len(th)
    rng = np.random.default_rng([777, B, *combo[:4]])
    ga, gb = rng.standard_normal((2, B, dA.shape[1]))
    if zero:
        ga, gb = np.zeros_like(ga), np.zeros_like(gb)
    t = np.einsum("bj,bjk->bk", ga, dA[idx]) + np.einsum("bj,bjk->bk", gb, dB[idx])
    S = np.einsum("bj,bjk->bk", np.abs(ga), np.abs(dA[idx])) + np.einsum("bj,bjk->bk", np.abs(gb), np.abs(dB[idx]))
    return np.ascontiguousarray(th[idx]), np.ascontiguousarray(nm[idx]), ga, gb, t, S


def deviation(got_theta, got_norm, t, S):
    """largest |got - truth| / S over the rows and outputs"""
    got = np.column_stack([got_theta, got_norm])
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.max(np.where(S > 0, np.abs(got - t) / S, np.where(got == t, 0.0, np.inf))))


@functools.lru_cache(maxsize=None)
def ref_dev():
    """dev of the bar: approx_batch_vjp against the truth, over the six-draw (two-draw) batch of every combo"""
    import pioran_jl_amd as pj
    cls = (pj.SingleBendingPowerLaw, pj.DoubleBendingPowerLaw)
    dev = 0.0
    for c in combos():
        m, b, i, J, n = c
        th, nm, ga, gb, t, S = batch(c, n)
        g, gn = pj.approx_batch_vjp(cls[m], th, F_MIN, F_MAX, J, nm, ga, gb, S_LOW, S_HIGH, is_integrated_power=bool(i), basis_function=BASIS_NAME[b])
        dev = max(dev, deviation(g, gn, t, S))
    return dev


def bar():
    return max(MARGIN * ref_dev(), FLOOR)
