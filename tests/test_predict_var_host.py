"""CPU tests (-m "not gpu") of the posterior variance through the celerite factorisation: the numpy prototype of the recurrences
(tools/predict_var_proto.py — what the HIP kernels of celerite_predict.hip restate) against the dense oracle
diag(oracle.predict_cov_numpy), and the new C entry's presence and argument checks.

Bound: 1e-11 k(0), k(0) = sum(a).  The error of var = k(0) - q1 - q2 is absolute on the scale of k(0) (a difference of numbers of that
size; the dense formula shares this); the prototype measured 5e-13 k(0) against an 80-bit dense evaluation on the inputs of the first
test, the bound is 20 x that."""
import ctypes
import importlib.util
import json
import re
import sys
from pathlib import Path

import numpy as np
import pytest

import pioran_jl_amd as pj
from oracle import oracle as O

ROOT = Path(__file__).resolve().parents[1]
BOUND = 1e-11
sys.path.insert(0, str(Path(__file__).resolve().parent))
import predict_var_cases as PV  # noqa: E402


def _proto():
    spec = importlib.util.spec_from_file_location("predict_var_proto", ROOT / "tools" / "predict_var_proto.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _check(a, b, c, d, t, s2, tau):
    ref = np.diag(O.predict_cov_numpy(a, b, c, d, tau, t, s2))
    got = _proto().predict_var(a, b, c, d, t, s2, tau)
    k0 = np.sum(a)
    err = np.max(np.abs(got - ref)) / k0
    print(f"max |delta| / k(0) = {err:.2e}   min var / k(0) = {ref.min() / k0:.2e}")
    assert err <= BOUND, err
    return err


def _tau(t, n_in, n_out, step, seed):
    """evaluation times: inside the span, outside it on both sides, exact data times, in no particular order"""
    rng = np.random.default_rng(seed)
    span = t[-1] - t[0]
    return np.concatenate([rng.uniform(t[0], t[-1], n_in), t[0] - rng.uniform(0, 0.05 * span, n_out // 2),
                           t[-1] + rng.uniform(0, 0.05 * span, n_out - n_out // 2), t[::step]])


@pytest.mark.parametrize("basis", ["SHO", "DRWCelerite"])
def test_prototype_against_dense_oracle_synthetic(basis):
    """N = 400 of the synthetic series, 160 evaluation times, six prior draws, SHO-20 (40 rows) and DRWCelerite-20 (60 rows)."""
    t, y, yerr = O.synthetic_series(400)
    A, Bc, C, Dd, mu, nu = O.theta_to_coefs(O.synthetic_theta(6, t, y), t, 20, basis)
    tau = _tau(t, 120, 20, 20, 0)
    assert len(tau) == 160
    for k in range(6):
        _check(A[k], Bc[k], C, Dd, t, nu[k] * yerr ** 2, tau)


def test_prototype_against_dense_oracle_simu(golden_dir):
    """The reference's test series (test/data/simu.txt, N = 489): a Celerite sum with mixed-sign b, and a CARMA(3,2) set (one real term:
    a single row, and a complex term with negative d)."""
    S = np.loadtxt(golden_dir / "simu.txt")
    t, yerr = S[:, 0], S[:, 2]
    tau = _tau(t, 150, 30, 25, 1)
    a = np.array([1.3, 0.6, 0.25]); c = np.array([0.02, 0.11, 0.6]); d = np.array([0.05, 0.4, 2.1])
    b = np.array([0.4, -0.5, 0.3]) * a * c / d          # |b d| <= a c keeps every term a valid covariance
    _check(a, b, c, d, t, yerr ** 2, tau)
    g = json.loads((golden_dir / "reference_literals.json").read_text())["carma32"]
    a, b, c, d = O.carma_celerite_coefs(g["p"], np.array([complex(*z) for z in g["r_alpha"]]), g["beta"], g["norm"])
    _check(a, b, c, d, t, yerr ** 2, tau)


def test_prototype_order_and_edges():
    """Unsorted tau gives the permuted result; a point equal to a data time has a variance below that point's noise variance."""
    t, y, yerr = O.synthetic_series(200)
    A, Bc, C, Dd, mu, nu = O.theta_to_coefs(O.synthetic_theta(1, t, y), t)
    P = _proto()
    tau = _tau(t, 40, 10, 10, 2)
    v = P.predict_var(A[0], Bc[0], C, Dd, t, yerr ** 2, tau)
    o = np.argsort(tau, kind="stable")
    assert np.array_equal(P.predict_var(A[0], Bc[0], C, Dd, t, yerr ** 2, tau[o]), v[o])
    vd = P.predict_var(A[0], Bc[0], C, Dd, t, yerr ** 2, t)
    assert (vd >= 0).all() and (vd <= yerr ** 2).all()


def test_entry_declared_everywhere():
    name = "pioran_celerite_predict_var"
    hdr = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "pioran_hip.h").read_text(), flags=re.S)
    assert re.search(r"\bint\s+" + name + r"\s*\(", hdr)
    assert name in pj._lib.SIGNATURES and len(pj._lib.SIGNATURES[name][1]) == 13
    jl = (ROOT / "pioran.jl_amd" / "julia" / "PioranHIP.jl").read_text()
    assert re.search(r"ccall\(\(:" + name + r", LIB\)", jl)
    assert hasattr(pj._lib.lib(), name)
    for f in ("predict_var", "var", "std"):
        assert callable(getattr(pj, f))
    assert callable(pj.Dataset.predict_var)
    assert pj._lib.lib().pioran_abi_version() == 7


def test_argument_validation_without_gpu():
    L = pj._lib.lib()
    one = (ctypes.c_double * 1)(1.0)
    p = ctypes.cast(one, ctypes.c_void_p)
    # no data set
    assert L.pioran_celerite_predict_var(None, 1, 1, p, p, p, p, 1, None, 1, p, p, None) == -1
    fake = ctypes.c_void_p(8)   # never dereferenced: the checks below come first
    assert L.pioran_celerite_predict_var(fake, 1, 1, p, p, p, p, 1, None, 1, None, p, None) == -1    # tau
    assert L.pioran_celerite_predict_var(fake, 1, 1, p, p, p, p, 1, None, 1, p, None, None) == -1    # var_out
    assert L.pioran_celerite_predict_var(fake, 0, 1, p, p, p, p, 1, None, 1, p, p, None) == -1       # B
    assert L.pioran_celerite_predict_var(fake, 1, 1, p, p, p, p, 1, None, -1, p, p, None) == -1      # M
    assert L.pioran_celerite_predict_var(fake, 1, 1, None, p, p, p, 1, None, 1, p, p, None) == -1    # A
    nan = (ctypes.c_double * 1)(float("nan"))
    assert L.pioran_celerite_predict_var(fake, 1, 1, p, p, p, p, 1, None, 1, ctypes.cast(nan, ctypes.c_void_p), p, None) == -1
    with pytest.raises(ValueError):
        pj.std(None, None, solver="dense")


# ---- the truth, the prototype against it, and the cases the kernels are held to -----------------------------------------------------
def test_long_double_truth_against_50_digits(golden_dir):
    """oracle.predict_var_truth in long double on the six N = 150 fixture draws against the stored mpmath values: within 4 x the deviation
    recorded when the fixture was made (another libm), and that deviation at most 1/100 of the prototype's on the same draw, which is what
    lets long double stand in as the truth everywhere else."""
    F = np.load(golden_dir / "predict_var_truth.npz")
    P = _proto()
    draws = [d for d in PV.fixture_draws(golden_dir) if d[0].startswith("n150")]
    assert len(draws) == 6 == len(F["ld_dev"])
    for (label, a, b, c, d, t, s2, tau, truth, ratio), stored in zip(draws, F["ld_dev"]):
        k0 = a.sum()
        ld = float(np.max(np.abs(O.predict_var_truth(a, b, c, d, tau, t, s2) - truth))) / k0
        pdev = float(np.max(np.abs(P.predict_var(a, b, c, d, t, s2, tau) - truth))) / k0
        print(f"{label}: ratio {ratio:.1e}   long double {ld:.2e} k(0) (stored {stored:.2e})   prototype {pdev:.2e} k(0)")
        assert ld <= 4 * stored, (label, ld, stored)
        assert stored <= pdev / 100, (label, stored, pdev)


def test_prototype_on_the_fixture(golden_dir):
    """The prototype and the fp64 dense oracle on the nine ill-conditioned fixture draws (N = 150, N = 1000); the figures are printed (the
    table of docs/EXPERIMENTS.md).  N = 150: the prototype within 20 x the 3.7e-14 k(0) measured on the worst of these draws.  N = 1000 is a
    measurement (7e-12 k(0) on the lowest ratio: the recurrences' error grows with N on such a draw, the dense formula's does not); the GPU test
    takes its bound from the figure computed on the same draw."""
    P = _proto()
    for label, a, b, c, d, t, s2, tau, truth, ratio in PV.fixture_draws(golden_dir):
        k0 = a.sum()
        pdev = float(np.max(np.abs(P.predict_var(a, b, c, d, t, s2, tau) - truth))) / k0
        ddev = float(np.max(np.abs(np.diag(O.predict_cov_numpy(a, b, c, d, tau, t, s2)) - truth))) / k0
        print(f"{label}: ratio {ratio:.1e}   prototype {pdev:.2e} k(0)   fp64 dense oracle {ddev:.2e} k(0)   min var / k(0) {float(truth.min()) / k0:.2e}")
        assert np.isfinite(pdev) and (len(t) > 150 or pdev <= 20 * 3.7e-14), (label, pdev)


@pytest.mark.parametrize("which", ["edge", "fuzz"])
def test_prototype_on_the_cases(which):
    """check(prototype) on every edge and fuzz case: every draw positive definite in the truth's own Cholesky (reference() raises otherwise),
    the prototype within the floor of the bound where 20 x its own deviation is below it."""
    cases = list(PV.edge_cases()) if which == "edge" else list(PV.fuzz_cases(40))
    assert len(cases) == (2 * len(PV.edge_combinations()) if which == "edge" else 40)
    worst = 0.0
    for case in cases:
        worst = max(worst, PV.check(PV.proto_impl(), case).max())
    print(f"{which}: {len(cases)} cases, worst prototype deviation {worst:.2e} k(0)")


def test_case_list_covers_what_it_promises():
    combos = PV.edge_combinations()
    assert len(set(combos)) == len(combos)
    for R in PV.ROWS:
        assert {(R, 3, "mixed"), (R, 9, "mixed")} <= set(combos)
    for N in PV.LENGTHS:
        assert {(3, N, "mixed"), (33, N, "mixed")} <= set(combos)
    for pat in PV.PATTERNS:
        assert {(17, 5, pat), (64, 33, pat)} <= set(combos)
    for label, t, s2, A, Bc, C, Dd, nu, tau in PV.edge_cases():
        R, N = int(label.split("-")[0][1:]), int(label.split("-")[1][1:])
        assert len(t) == N and A.shape[0] == 3 and 2 * A.shape[1] - int(np.sum(Dd == 0.0)) == R, label
    seen = {(c[0].split("-")[-2], c[0].split("-")[-1]) for c in PV.fuzz_cases(40)}
    assert {k for _, k in seen} == {"shared", "perdraw"}


@pytest.mark.parametrize("mistake", ["mask_last_row", "reuse_alpha", "phi_of_step", "n0_le_forward"])
def test_the_cases_can_fail(mistake):
    """Each seeded mistake of the prototype (tools/predict_var_proto.py, MISTAKES) fails check() on at least one edge case."""
    caught = []
    for case in PV.edge_cases():
        try:
            PV.check(PV.proto_impl(mistake=mistake), case)
        except AssertionError:
            caught.append(case[0])
    print(f"{mistake}: caught by {len(caught)} edge cases, e.g. {caught[:4]}")
    assert caught, mistake
