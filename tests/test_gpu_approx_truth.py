"""GPU tests (-m gpu) of the forward `approx` on the device (approx_kernel, csrc/approx.hip): the coefficients every theta-level entry starts from,
held to the 50-digit truth of tests/approx_cases.py within its bar max(20 x ref_dev, 256 eps) per combo and array — the CPU suite,
tests/test_approx_host.py, shows that the bar catches seeded mistakes and holds the host mirrors and a numpy restatement of the kernel to it.

1. the continuum's (a, b) through Dataset.logpdf_theta(return_coefs=True) for every continuum combo at every launch size around the 64-thread
   block; the value path takes every size, the 216 rows of DRWCelerite J = 72 on its any-size kernel, so no combo is left out of the value call;
2. with features, coef_a .. coef_d of Dataset.logpdf_theta_grad(qpo=..., approx_on="device", return_coef_grads=True), the continuum columns of
   coef_c, coef_d against the truth's grid, and the same (a, b) bit for bit from Dataset.logpdf_theta(qpo=...) where the forward entry takes the
   rows (it refuses the 98 rows of SHO J = 48 with a feature); n_qpo up to the limit of 8 in both normalisations;
3. a draw's coefficients do not depend on its place in the batch or on the batch size;
4. end to end: log L of logpdf_theta against -oracle.dense_nll_truth (dense, long double) on the truth coefficients, plain, with mu / nu and with
   a shift, within max(20 x ref_dev, 256 eps) |truth|, ref_dev that of the fp64 oracle on the host mirror's coefficients;
5. pioran_celerite_config_name(-1) names what ran after every call of 1 and 2.
The series is the first 48 points of tests/golden/simu.txt (the approx kernel does not read it).  Every figure is printed before it is asserted."""
import importlib.util
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import pioran_jl_amd as pj  # noqa: E402
from oracle import oracle as O  # noqa: E402

sys.path.insert(0, str(Path(__file__).resolve().parent))
import approx_cases as AC  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]
CLS = (pj.SingleBendingPowerLaw, pj.DoubleBendingPowerLaw)
COEF_KEYS = ("coef_a", "coef_b", "coef_c", "coef_d")
QPO_VJP_NAME = "approx with features (reverse mode of the coefficients)"
UNSUPPORTED = -4


def _route_grid():
    spec = importlib.util.spec_from_file_location("route_grid", ROOT / "tools" / "route_grid.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _route_grid()


@pytest.fixture(scope="module")
def ctx():
    return pj.Context(0)


@pytest.fixture(scope="module")
def ds(ctx, golden_dir):
    A = np.loadtxt(golden_dir / "simu.txt")
    return pj.Dataset(A[:AC.E2E_N, 0], A[:AC.E2E_N, 1], A[:AC.E2E_N, 2] ** 2, ctx)


def _ran():
    return pj._lib.lib().pioran_celerite_config_name(-1).decode()


def _args(combo):
    m, b, i, J, nq, n, lo, hi = combo
    return (AC.F_MIN, AC.F_MAX, J, lo, hi), dict(is_integrated_power=bool(i), basis_function=AC.BASIS_NAME[b])


def _forward(ds, combo, th, nm, qp, **kw):
    pos, named = _args(combo)
    return ds.logpdf_theta(CLS[combo[0]], th, nm, *pos, **named, qpo=qp, return_status=True, **kw)


def _grad_entry(ds, combo, th, nm, qp):
    pos, named = _args(combo)
    g = ds.logpdf_theta_grad(CLS[combo[0]], th, nm, *pos, **named, qpo=qp, approx_on="device", return_coef_grads=True)
    return dict(zip("abcd", (g[k] for k in COEF_KEYS)))


def _terms(combo):
    """(two-row terms, one-row terms) of the continuum"""
    J, b = combo[3], combo[1]
    return J, (J if b else 0)


# ---- 1. the continuum's coefficients against the truth ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("combo", AC.continuum_combos(), ids=AC.name)
def test_continuum_coefficients_against_truth(ds, combo):
    Jc, Jt = AC.widths(combo)
    n_two, n_one = _terms(combo)
    for B in AC.LAUNCH_B:
        th, nm, _, idx = AC.batch(combo, B)
        out, st, A, Bc = _forward(ds, combo, th, nm, None, return_coefs=True)
        ran, want = _ran(), G.value_route(AC.state_rows(combo), Jc, n_one, B, ds.N)[0]
        print(f"{AC.name(combo)} B = {B}: value path on '{ran}' (the rule: '{want}'), status {np.bincount(st, minlength=3)}")
        assert A.shape == Bc.shape == (B, Jt) and out.shape == st.shape == (B,)
        AC.check(combo, {"a": A, "b": Bc}, idx, leg=f"device B={B}")        # (coefficients are returned whatever the draw's status)
        assert ran == want


# ---- 2. coefficients with features ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("combo", AC.qpo_combos(), ids=AC.name)
def test_feature_coefficients_against_truth(ds, combo):
    Jc, Jt = AC.widths(combo)
    n_two, n_one = _terms(combo)
    for B in AC.LAUNCH_B:
        th, nm, qp, idx = AC.batch(combo, B)
        got = _grad_entry(ds, combo, th, nm, qp)
        ran = _ran()
        assert all(v.shape == (B, Jt) for v in got.values())
        AC.check(combo, got, idx, leg=f"device B={B}")
        assert ran == QPO_VJP_NAME
        # the continuum's (c, d) are the grid's: the same bits in every row
        assert (got["c"][:, :Jc] == got["c"][0, :Jc]).all() and (got["d"][:, :Jc] == got["d"][0, :Jc]).all()
        if AC.forward_entry_takes(combo):                                   # the same kernel behind the forward entry: the same bits
            out, st, A, Bc = _forward(ds, combo, th, nm, qp, return_coefs=True)
            ran, want = _ran(), G.value_route_cd(n_two, n_one, combo[4], B, ds.N, must_run=True)[0]
            print(f"{AC.name(combo)} B = {B}: forward entry on '{ran}' (the rule: '{want}'), status {np.bincount(st, minlength=3)}")
            assert np.array_equal(A, got["a"]) and np.array_equal(Bc, got["b"])
            assert ran == want
        else:
            with pytest.raises(pj._lib.PioranHipError, match=f"error {UNSUPPORTED}:"):
                _forward(ds, combo, th, nm, qp, return_coefs=True)


# ---- 3. place independence ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("combo", AC.PLACE_COMBOS, ids=AC.name)
def test_a_draw_does_not_depend_on_its_place_or_the_batch_size(ds, combo):
    th, nm, qp, idx = AC.batch(combo, 130)
    full = _grad_entry(ds, combo, th, nm, qp)
    for k in (0, 63, 64, 129):
        one = _grad_entry(ds, combo, th[k:k + 1], nm[k:k + 1], qp[k:k + 1])
        for key in "abcd":
            assert np.array_equal(one[key][0], full[key][k]), (key, k)
    # the last 70 rows as a batch of their own: every draw at another position of another block
    tail = _grad_entry(ds, combo, th[60:], nm[60:], qp[60:])
    for key in "abcd":
        assert np.array_equal(tail[key], full[key][60:]), key
    if AC.forward_entry_takes(combo):
        A, Bc = _forward(ds, combo, th[60:], nm[60:], qp[60:], return_coefs=True)[2:]
        assert np.array_equal(A, full["a"][60:]) and np.array_equal(Bc, full["b"][60:])


# ---- 4. end to end ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", AC.E2E_VARIANTS)
@pytest.mark.parametrize("combo", AC.END_TO_END, ids=AC.name)
def test_end_to_end_against_dense_truth_on_truth_coefficients(ctx, golden_dir, combo, variant):
    t, y, s2 = AC.e2e_series(golden_dir, combo)
    tr = AC.truth(combo)
    n = combo[5]
    mu, nu, shift = AC.e2e_extras(combo, variant)
    host = AC.host_mirror(combo)
    dse = pj.Dataset(t, y, s2, ctx)
    out, st = _forward(dse, combo, tr["theta"], tr["norm"], tr["qpo"], mu=mu, nu=nu, shift=shift)
    ran = _ran()
    dev, bound = np.empty(n), np.empty(n)
    for k in range(n):
        yk, sk = AC.e2e_draw_series(y, s2, mu, nu, shift, k)
        truth = -float(O.dense_nll_truth(tr["A"][k], tr["B"][k], tr["C"][k], tr["D"][k], t, yk, sk)[0])
        ref = O.logl(host["a"][k], host["b"][k], host["c"][k], host["d"][k], t, yk, sk)
        ref_dev = abs(ref - truth) / abs(truth)
        dev[k], bound[k] = abs(out[k] - truth) / abs(truth), max(AC.MARGIN * ref_dev, AC.FLOOR)
        print(f"{AC.name(combo)} {variant} draw {k} ('{ran}'): log L {out[k]:.12g}, truth {truth:.12g}, status {st[k]}, deviation {dev[k]:.3e} "
              f"({dev[k] / AC.EPS:.1f} eps)   ref_dev {ref_dev:.3e}   bound {bound[k]:.3e}")
    assert (st == 0).all()
    assert (dev <= bound).all(), (AC.name(combo), variant, dev, bound)         # no draw is left out
