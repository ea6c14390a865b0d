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
from pathlib import Path

import numpy as np
import pytest

import pioran_jl_amd as pj
from oracle import oracle as O

ROOT = Path(__file__).resolve().parents[1]
BOUND = 1e-11


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
