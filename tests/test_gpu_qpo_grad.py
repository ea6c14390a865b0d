"""GPU tests (-m gpu) of the gradient of log L with respect to the sampled parameters of continuum + QPO models (pioran_approx_qpo_vjp_batch,
pioran_logpdf_batch_theta_qpo_grad: Context.approx_qpo_vjp, Dataset.logpdf_theta_grad(qpo=..., approx_on="device")).

The reverse mode of approx with features against a 50-digit truth within the bar of tests/qpo_grad_cases.py (whose CPU suite,
tests/test_qpo_grad_host.py, shows that the bar catches seeded mistakes) at launch sizes around the 64-thread block; its structural properties;
the entry, exactly, against the chain it is made of (Dataset.logl_grad on the returned coefficients, Context.approx_qpo_vjp on its gradients); end
to end against the oracle's gradient contracted with the truth Jacobian; the routing edges at 64 and 144 rows; the shifted models; rejected draws.
Series are the first 120 points of tests/golden/simu.txt.  Every figure is printed before it is asserted."""
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import pioran_jl_amd as pj  # noqa: E402
from oracle import oracle as O  # noqa: E402

sys.path.insert(0, str(Path(__file__).resolve().parent))
import qpo_grad_cases as QC  # noqa: E402

CLS = (pj.SingleBendingPowerLaw, pj.DoubleBendingPowerLaw)
COEF_KEYS = ("coef_a", "coef_b", "coef_c", "coef_d")
GRAD_KEYS = ("grad_a", "grad_b", "grad_c", "grad_d")
OUT_KEYS = ("grad_theta", "grad_norm", "grad_qpo", "grad_nu", "grad_mu", "grad_shift")
UNSUPPORTED = -4


@pytest.fixture(scope="module")
def ctx():
    return pj.Context(0)


@pytest.fixture(scope="module")
def ds(ctx, golden_dir):
    A = np.loadtxt(golden_dir / "simu.txt")
    return pj.Dataset(A[:120, 0], A[:120, 1], A[:120, 2] ** 2, ctx)


@pytest.fixture(scope="module")
def series(golden_dir):
    A = np.loadtxt(golden_dir / "simu.txt")
    return A[:120, 0], A[:120, 1], A[:120, 2]


def _ran():
    return pj._lib.lib().pioran_celerite_config_name(-1).decode()


def _vjp(ctx, combo, th, nm, qp, g):
    m, b, i, J, nq, _ = combo
    return ctx.approx_qpo_vjp(CLS[m], th, nm, qp, *g, QC.F_MIN, QC.F_MAX, J, QC.S_LOW, QC.S_HIGH, is_integrated_power=bool(i),
                              basis_function=QC.BASIS_NAME[b])


def _entry(ds, combo, th, nm, qp, approx_on="device", **kw):
    m, b, i, J, nq, _ = combo
    return ds.logpdf_theta_grad(CLS[m], th, nm, QC.F_MIN, QC.F_MAX, J, QC.S_LOW, QC.S_HIGH, is_integrated_power=bool(i),
                                basis_function=QC.BASIS_NAME[b], qpo=qp, approx_on=approx_on, **kw)


def _draws(rng, B, nq):
    """B prior draws of the single bend with nq features: theta, norm, qpo, mu, nu"""
    th = np.column_stack([rng.uniform(0.0, 1.2, B), np.exp(rng.uniform(np.log(4 * QC.F_MIN), np.log(QC.F_MAX / 4), B)), rng.uniform(2.0, 3.8, B)])
    qp = np.stack([rng.uniform(0.05, 2.0, (B, nq)), np.exp(rng.uniform(np.log(20 * QC.F_MIN), np.log(QC.F_MAX / 5), (B, nq))),
                   rng.uniform(2.0, 20.0, (B, nq))], axis=2)
    return th, np.exp(np.log(0.5) + 0.5 * rng.standard_normal(B)), qp, 4.8 + 0.1 * rng.standard_normal(B), rng.uniform(0.8, 1.5, B)


# ---- 1. the kernel against the truth ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("combo", QC.combos(), ids=QC.name)
def test_approx_qpo_vjp_against_truth(ctx, combo):
    P = 3 if combo[0] == 0 else 5
    for B in QC.LAUNCH_B:
        th, nm, qp, g, want, S = QC.batch(combo, B)
        gth, gn, gq = _vjp(ctx, combo, th, nm, qp, g)
        d = QC.deviation(QC.flatten(gth, gn, gq), want, S)
        print(f"{QC.name(combo)}, B = {B}: device deviates by {d:.3e} S_k (bar {QC.bar():.3e}, dev {QC.ref_dev():.3e})")
        assert gth.shape == (B, P) and gn.shape == (B,) and gq.shape == (B, combo[4], 3)
        assert d <= QC.bar()
    assert _ran() == "approx with features (reverse mode of the coefficients)"


# ---- 2. structural properties -------------------------------------------------------------------------------------------------------------------

def test_zero_cotangent_is_exactly_zero(ctx):
    for combo in QC.combos():
        th, nm, qp, g, want, S = QC.batch(combo, combo[5], zero=True)
        assert not QC.flatten(*_vjp(ctx, combo, th, nm, qp, g)).any(), QC.name(combo)


@pytest.mark.parametrize("combo", [(0, 0, 1, 3, 1, 4), (1, 1, 1, 20, 2, 4), (1, 0, 0, 20, 2, 4), (0, 0, 1, 48, 1, 2)], ids=QC.name)
def test_a_draw_does_not_depend_on_its_place_or_the_batch_size(ctx, combo):
    th, nm, qp, g, want, S = QC.batch(combo, 130)
    full = QC.flatten(*_vjp(ctx, combo, th, nm, qp, g))
    for k in (0, 63, 64, 129):
        one = QC.flatten(*_vjp(ctx, combo, th[k:k + 1], nm[k:k + 1], qp[k:k + 1], g[:, k:k + 1]))
        assert np.array_equal(one[0], full[k]), k
    # the last 70 rows as a batch of their own: every draw at another position of another block
    tail = QC.flatten(*_vjp(ctx, combo, th[60:], nm[60:], qp[60:], g[:, 60:]))
    assert np.array_equal(tail, full[60:])


@pytest.mark.parametrize("combo", [c for c in QC.combos() if c[2] == 0 and c[3] in (3, 20)], ids=QC.name)
def test_variance_form_with_zero_feature_cotangents_is_the_continuum_reverse_mode(ctx, combo):
    m, b, i, J, nq, n = combo
    th, nm, qp, g, want, S = QC.batch(combo, 65)
    Jc = J * (1 + b)
    g = g.copy()
    g[:, :, Jc:] = 0.0
    t = QC.truth(combo)
    idx = np.arange(65) % n
    jac = np.stack([t[k][idx] for k in ("dA", "dB", "dC", "dD")])
    want, S = np.einsum("abj,abjk->bk", g, jac), np.einsum("abj,abjk->bk", np.abs(g), np.abs(jac))
    gth, gn, gq = _vjp(ctx, combo, th, nm, qp, g)
    assert not gq.any()                                       # the features enter neither I nor any continuum coefficient
    old_th, old_n = ctx.approx_vjp(CLS[m], th, nm, g[0][:, :Jc], g[1][:, :Jc], QC.F_MIN, QC.F_MAX, J, QC.S_LOW, QC.S_HIGH, is_integrated_power=False,
                                   basis_function=QC.BASIS_NAME[b])
    P = th.shape[1]
    d_new = QC.deviation(np.column_stack([gth, gn]), want[:, :P + 1], S[:, :P + 1])
    d_old = QC.deviation(np.column_stack([old_th, old_n]), want[:, :P + 1], S[:, :P + 1])
    print(f"{QC.name(combo)}: against the truth, new kernel {d_new:.3e} S_k, approx_vjp_kernel {d_old:.3e} S_k (bar {QC.bar():.3e})")
    assert d_new <= QC.bar() and d_old <= QC.bar()
    assert np.max(np.abs(np.column_stack([gth - old_th, gn - old_n])) / S[:, :P + 1]) <= QC.bar()


# ---- 3. the same kernels on the same numbers ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("extras", ["none", "mu_nu"])
@pytest.mark.parametrize("combo,B", [((0, 0, 1, 20, 1, 4), 6), ((1, 1, 1, 3, 2, 4), 5), ((0, 1, 0, 20, 2, 4), 1), ((0, 0, 1, 3, 1, 4), 70)],
                         ids=lambda v: QC.name(v) if isinstance(v, tuple) else f"B{v}")
def test_entry_is_the_chain_of_its_parts(ctx, ds, combo, B, extras):
    th, nm, qp, _, _, _ = QC.batch(combo, B)
    rng = np.random.default_rng([31, B])
    mu, nu = (None, None) if extras == "none" else (4.8 + 0.1 * rng.standard_normal(B), rng.uniform(0.8, 1.5, B))
    got = _entry(ds, combo, th, nm, qp, mu=mu, nu=nu, return_coef_grads=True)
    ref = ds.logl_grad(*(got[k] for k in COEF_KEYS), mu=mu, nu=nu, cd_grad=True)
    fam = _ran()
    print(f"\n{QC.name(combo)} B = {B}, {extras}: reverse mode on '{fam}', status {np.bincount(got['status'])}")
    for k in ("logl", "status") + GRAD_KEYS:
        np.testing.assert_array_equal(got[k], ref[k], err_msg=k)
    for k, v in (("grad_nu", nu), ("grad_mu", mu)):
        if v is None:
            assert got[k] is None
        else:
            np.testing.assert_array_equal(got[k], ref[k], err_msg=k)
    assert got["grad_shift"] is None
    chain = _vjp(ctx, combo, th, nm, qp, [got[k] for k in GRAD_KEYS])
    for k, v in zip(OUT_KEYS[:3], chain):
        np.testing.assert_array_equal(got[k], v, err_msg=k)
    lean = _entry(ds, combo, th, nm, qp, mu=mu, nu=nu)
    assert "grad_a" not in lean and "coef_a" not in lean
    for k in ("logl", "status") + OUT_KEYS:
        if got[k] is None:
            assert lean[k] is None
        else:
            np.testing.assert_array_equal(lean[k], got[k], err_msg=k)


# ---- 4. end to end against the oracle ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("integ", (1, 0))
@pytest.mark.parametrize("case", QC.END_TO_END, ids=lambda c: "m%d_b%d_J%d_q%d" % c)
def test_end_to_end_against_oracle_and_truth_jacobian(ds, series, case, integ):
    """d log L / d(theta, norm, qpo) = the oracle's gradient w.r.t. (a, b, c, d) (complex step) contracted with the 50-digit Jacobian of the
    coefficients.  Bar per output, as test_logpdf_carma_grad_end_to_end_against_oracle_and_truth_jacobian states it: the vjp's bar on its scale S plus
    the oracle gradient's own tolerance, 1e-8 (1 + max |grad_x|) per array, carried through the Jacobian."""
    t, y, yerr = series
    m, b, J, nq = case
    combo = (m, b, integ, J, nq, 4)
    tr = QC.truth(combo)
    n = len(tr["theta"])
    mu, nu = np.full(n, QC.E2E_MU), np.full(n, QC.E2E_NU)
    got = _entry(ds, combo, tr["theta"], tr["norm"], tr["qpo"], mu=mu, nu=nu)
    print(f"\n{QC.name(combo)}: status {got['status']}, logl {got['logl']}")
    assert (got["status"] == 0).all()
    got_all = QC.flatten(got["grad_theta"], got["grad_norm"], got["grad_qpo"])
    worst = 0.0
    for r in range(n):
        ref = O.logl_grad(tr["A"][r], tr["B"][r], tr["C"][r], tr["D"][r], t, y - mu[r], nu[r] * yerr ** 2, cd=True)
        g = np.stack([ref[k] for k in GRAD_KEYS])                                  # [4][Jt]
        jac = np.stack([tr[k][r] for k in ("dA", "dB", "dC", "dD")])               # [4][Jt][K]
        want = np.einsum("kj,kjp->p", g, jac)
        S = np.einsum("kj,kjp->p", np.abs(g), np.abs(jac))
        tol = QC.bar() * S + 1e-8 * np.einsum("k,kp->p", 1 + np.abs(g).max(axis=1), np.abs(jac).sum(axis=1))
        ratio = np.max(np.abs(got_all[r] - want) / tol)
        worst = max(worst, ratio)
        assert ratio <= 1.0, (combo, r, got_all[r], want, tol)
    print(f"{QC.name(combo)}: largest |got - want| / bar = {worst:.3e}")


# ---- 5. routing edges ---------------------------------------------------------------------------------------------------------------------------------

def test_64_rows_run_step_by_step(ctx, ds):
    """SHO with 31 components and one feature: 64 rows, one more than the windowed reverse mode takes"""
    th, nm, qp, mu, nu = _draws(np.random.default_rng(51), 2, 1)
    combo = (0, 0, 1, 31, 1, 2)
    got = _entry(ds, combo, th, nm, qp, mu=mu, nu=nu, return_coef_grads=True)
    ref = ds.logl_grad(*(got[k] for k in COEF_KEYS), mu=mu, nu=nu, cd_grad=True)
    fam = _ran()
    print(f"\n64 rows, B = 2: reverse mode on '{fam}', status {got['status']}")
    assert fam == "wide (step-by-step gradient)" and (got["status"] == 0).all()
    for k in ("logl", "status") + GRAD_KEYS:
        np.testing.assert_array_equal(got[k], ref[k], err_msg=k)
    host = _entry(ds, combo, th, nm, qp, approx_on="host", mu=mu, nu=nu)
    for k in ("logl",) + OUT_KEYS[:5]:
        err = np.max(np.abs(got[k] - host[k])) / (1 + np.max(np.abs(host[k])))
        print(f"  {k}: device against host {err:.3e}")
        assert err <= 1e-8, k


def test_144_rows_are_unsupported_on_both_paths(ds):
    th, nm, qp, mu, nu = _draws(np.random.default_rng(52), 2, 1)
    combo = (0, 0, 1, 71, 1, 2)
    for where in ("device", "host"):
        with pytest.raises(pj._lib.PioranHipError, match=f"error {UNSUPPORTED}:"):
            _entry(ds, combo, th, nm, qp, approx_on=where, mu=mu, nu=nu)


# ---- 6. the shifted models ------------------------------------------------------------------------------------------------------------------------------

def test_shifted_model_against_the_host_chain(ds):
    B = 3
    th, nm, qp, mu, nu = _draws(np.random.default_rng(53), B, 2)
    shift = np.linspace(0.0, 0.3, B)
    combo = (0, 0, 1, 20, 2, B)
    got = _entry(ds, combo, th, nm, qp, mu=np.log(mu), nu=nu, shift=shift)
    host = _entry(ds, combo, th, nm, qp, approx_on="host", mu=np.log(mu), nu=nu, shift=shift)
    print(f"\nshifted, B = {B}: status {got['status']}, logl {got['logl']}")
    assert (got["status"] == 0).all() and np.array_equal(got["status"], host["status"])
    for k in ("logl",) + OUT_KEYS:
        err = np.max(np.abs(got[k] - host[k])) / (1 + np.max(np.abs(host[k])))
        print(f"  {k}: device against host {err:.3e}")
        assert err <= 1e-8, k


# ---- 7. rejected draws ----------------------------------------------------------------------------------------------------------------------------------

def test_rejected_draws_one_for_each_reason(ds):
    B = 9
    th, nm, qp, mu, nu = _draws(np.random.default_rng(54), B, 2)
    good = (th.copy(), nm.copy(), qp.copy())
    th[1, 2] = np.nan                  # NaN in theta
    nm[2] = np.inf                     # the norm
    qp[4, 0, 1] = 0.0                  # f0 = 0
    qp[5, 1, 2] = 0.5                  # Q = 1/2: Delta = 0, a DomainError of convert_feature below it
    qp[7, 1, 0] = np.nan               # NaN in a feature
    rej = np.zeros(B, bool)
    rej[[1, 2, 4, 5, 7]] = True
    combo = (0, 0, 1, 20, 2, B)
    g = _entry(ds, combo, th, nm, qp, mu=mu, nu=nu, return_coef_grads=True)
    # the same batch with good draws in the rejected rows: the same size, so the same kernels
    g0 = _entry(ds, combo, *good, mu=mu, nu=nu, return_coef_grads=True)
    print(f"\nstatus {g['status']} (all good: {g0['status']})")
    np.testing.assert_array_equal(g["status"], np.where(rej, 3, g0["status"]))
    assert (g0["status"] == 0).all() and np.all(g["logl"][rej] == -np.inf)
    np.testing.assert_array_equal(g["logl"][~rej], g0["logl"][~rej])
    for k in OUT_KEYS[:5] + GRAD_KEYS:
        assert not np.any(g[k][rej]), k                       # exactly 0.0 in every gradient row
        np.testing.assert_array_equal(g[k][~rej], g0[k][~rej], err_msg=k)
    for k in COEF_KEYS:
        assert np.isfinite(g[k]).all()                        # the rejected draws ran on benign coefficients
        np.testing.assert_array_equal(g[k][~rej], g0[k][~rej], err_msg=k)
