"""GPU tests (-m gpu) of the posterior draws at new times by Matheron's rule (pioran_celerite_rand_posterior: Dataset.rand_posterior behind
pj.rand_posterior(solver="celerite") and pj.ppc_timeseries) against a truth that is neither the kernels nor a restatement of their
recurrences: oracle.sim_truth on the merged grid and oracle.predict_mean_truth on the residual series, dense in long double.

Cases, checkers and the bound max(20 x ref_dev, 256 eps) live in tests/rand_posterior_cases.py; the CPU suite
(tests/test_rand_posterior_host.py) shows that the case list holds what it promises and that the checks catch seeded mistakes.  Every case
runs on three legs, and the family that ran is asserted:
    default routing, (c, d) shared         block (windowed posterior draw) up to 63 rows, wide (step-by-step posterior draw) above
    no_block, up to 63 rows                wide (step-by-step posterior draw) at the same shapes
    (c, d) per draw                        draw by draw on the shared route
each with tau ascending and with the same tau permuted.  Every figure is printed before it is asserted; test_zz_worst_deviation_per_family
prints the table of docs/EXPERIMENTS.md."""
import functools
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import pioran_jl_amd as pj  # noqa: E402

sys.path.insert(0, str(Path(__file__).resolve().parent))
import rand_posterior_cases as RP  # noqa: E402

CASES = RP.cases()
WORST = {}          # family -> (deviation, bound, label)
WINDOWED, STEPWISE = "block (windowed posterior draw)", "wide (step-by-step posterior draw)"


@pytest.fixture(scope="module")
def ctx():
    return pj.Context(0)


def _ran():
    return pj._lib.lib().pioran_celerite_config_name(-1).decode()


def _family(case, no_block=False):
    return STEPWISE if no_block or RP.rows(case) > 63 else WINDOWED


def _note(family, dev, bound, label):
    if family not in WORST or dev > WORST[family][0]:
        WORST[family] = (float(dev), float(bound), label)


def device_impl(ctx, family):
    def impl(case, tau, q_new):
        label, t, y, s2, A, Bc, C, Dd, mu, nu = case[:10]
        ds = pj.Dataset(t, y, s2, ctx)
        try:
            got, st = ds.rand_posterior(A, Bc, C, Dd, tau, case[11], q_new, case[13], mu=mu, nu=nu, shift=case[14], return_status=True)
        finally:
            ds.close()
        assert _ran() == family, (_ran(), family)
        return got, st
    return impl


class no_block:
    def __init__(self, ctx, on=True):
        self.ctx, self.on = ctx, on

    def __enter__(self):
        if self.on:
            self.ctx.set_option("no_block", "1")

    def __exit__(self, *exc):
        if self.on:
            self.ctx.set_option("no_block", None)


# ---- 1 --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_cases_against_truth(ctx, case):
    legs = [("shared", case, False), ("per-draw", RP.per_draw(case), False)]
    if RP.rows(case) <= 63:
        legs.append(("no_block", case, True))
    for leg, c, nb in legs:
        family = _family(c, nb)
        with no_block(ctx, nb):
            dev = RP.check(device_impl(ctx, family), c, leg=f"[{leg}: {family}]")
        ref_dev = RP.reference(c)[2]
        k = int(np.argmax(dev.max(axis=0)))
        name = family + {"shared": "", "per-draw": ", (c, d) per draw", "no_block": " (no_block)"}[leg] + (", shift" if c[14] is not None else "")
        _note(name, dev.max(axis=0)[k], max(RP.MARGIN * ref_dev[k], RP.FLOOR), c[0])


# ---- 2 --------------------------------------------------------------------------------------------------------------------------------
def _device_draws(ctx, shape):
    label, t, y, s2, a, b, c, d, mu, nu, tau = shape
    qd, qn, ep = RP.affine_inputs(shape)
    n = len(qd)
    assert n <= 44
    ds = pj.Dataset(t, y, s2, ctx)
    try:
        got, st = ds.rand_posterior(np.tile(a, (n, 1)), np.tile(b, (n, 1)), c, d, tau, qd, qn, ep, mu=np.full(n, mu), nu=np.full(n, nu), return_status=True)
    finally:
        ds.close()
    assert (st == 0).all()
    return got - mu


@pytest.mark.parametrize("R,N,M,on_data,nb", [(5, 9, 7, 0, False), (5, 9, 7, 0, True), (33, 17, 9, 2, False), (33, 17, 9, 2, True), (65, 9, 5, 0, False)])
def test_distribution_from_the_affine_map(ctx, R, N, M, on_data, nb):
    """out = m + G (q_data | q_new | eps) read off 2 N + M + 1 draws: m is the posterior mean, G G' the dense posterior covariance on tau"""
    shape = RP.affine_shape(R, N, M, on_data)
    family = STEPWISE if nb or R > 63 else WINDOWED
    with no_block(ctx, nb):
        draws = _device_draws(ctx, shape)
    assert _ran() == family
    dev_m, dev_c, bound_m, bound_c = RP.check_affine(draws, shape, leg=f"[{family}{' (no_block)' if nb else ''}]")
    _note("affine map, covariance / k(0), " + family + (" (no_block)" if nb else ""), dev_c, bound_c, shape[0])


# ---- 3 --------------------------------------------------------------------------------------------------------------------------------
def _call(ctx, case, **kw):
    label, t, y, s2, A, Bc, C, Dd, mu, nu, tau, q_data, q_new, eps, shift = case
    args = dict(A=A, Bc=Bc, mu=mu, nu=nu, shift=shift)
    args.update(kw)
    ds = pj.Dataset(t, y, s2, ctx)
    try:
        return ds.rand_posterior(args["A"], args["Bc"], C, Dd, tau, q_data, q_new, eps, mu=args["mu"], nu=args["nu"], shift=args["shift"], return_status=True)
    finally:
        ds.close()


@pytest.mark.parametrize("label", [s + "-shift" for s in RP.SHIFT_SHAPES])
def test_shift_not_below_the_data_is_status_2(ctx, label):
    """a draw with shift >= min y: status 2 and a NaN row; the other draws equal the call without it"""
    case = next(c for c in CASES if c[0] == label)
    good, st = _call(ctx, case)
    assert (st == 0).all()
    for bad_shift in (float(np.min(case[2])), float(np.min(case[2])) + 0.5):
        shift = case[14].copy()
        shift[1] = bad_shift
        got, st = _call(ctx, case, shift=shift)
        print(f"{label}: shift {bad_shift:.3f} >= min y: status {st}")
        assert list(st) == [0, 2] + [0] * (len(shift) - 2)
        assert np.isnan(got[1]).all()
        keep = [k for k in range(len(shift)) if k != 1]
        assert np.array_equal(got[keep], good[keep])


# ---- 4 --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", ["R33-N33-mixed-s2x1", "R65-N9-mixed-s2x1"])
def test_not_positive_definite_is_status_2(ctx, label):
    """a draw whose kernel is not positive definite (negative amplitudes): status 2 and a NaN row; the others are unaffected"""
    case = next(c for c in CASES if c[0] == label)
    good, st = _call(ctx, case)
    assert (st == 0).all()
    A, Bc = case[4].copy(), case[5].copy()
    A[0], Bc[0] = -A[0], -Bc[0]
    got, st = _call(ctx, case, A=A, Bc=Bc)
    print(f"{label}: draw 0 with -a, -b: status {st}")
    assert list(st) == [2] + [0] * (len(A) - 1)
    assert np.isnan(got[0]).all()
    assert np.array_equal(got[1:], good[1:])


# ---- 5 --------------------------------------------------------------------------------------------------------------------------------
def _kernel(a, b, C, Dd):
    k = functools.reduce(lambda k, j: k + pj.Celerite(a[j], b[j], C[j], Dd[j]), range(1, len(C)), pj.Celerite(a[0], b[0], C[0], Dd[0]))
    assert all(np.array_equal(np.real(np.atleast_1d(v)), w) for v, w in zip(k.celerite_coefs(), (a, b, C, Dd)))
    return k


def test_pj_rand_posterior_celerite_against_truth(ctx):
    """pj.rand_posterior(rng, fp, tau, n=3, solver="celerite") on the generator's own normals — standard_normal((n, N)), ((n, M)), ((n, N)) in
    this order — against the truth; N = 257"""
    case = next(c for c in CASES if c[0] == "R33-N257-mixed-s2x1")
    label, t, y, s2, A, Bc, C, Dd, mu, nu, tau = case[:11]
    n, N, M, m0 = 3, len(t), len(tau), 0.7
    fp = pj.posterior(pj.ScalableGP(m0, _kernel(A[0], Bc[0], C, Dd))(t, s2), y)
    seed = 20261018
    rng = np.random.default_rng(seed)
    q_data, q_new, eps = rng.standard_normal((n, N)), rng.standard_normal((n, M)), rng.standard_normal((n, N))
    got = pj.rand_posterior(np.random.default_rng(seed), fp, tau, n=n, ctx=ctx, solver="celerite")
    assert _ran() == WINDOWED and got.shape == (M, n)
    twin = (label + "/pj", t, y, s2, np.tile(A[0], (n, 1)), np.tile(Bc[0], (n, 1)), C, Dd, np.full(n, m0), np.ones(n), tau, q_data, q_new, eps, None)
    truth, scale, ref_dev = RP.truth_for(twin, tau, q_new)
    bound = np.maximum(RP.MARGIN * ref_dev, RP.FLOOR)
    dev = np.array([float(np.max(np.abs(got[:, k] - m0 - truth[k]))) / scale[k] for k in range(n)])
    for k in range(n):
        print(f"pj.rand_posterior(solver='celerite') R33-N257 draw {k}: deviation {dev[k]:.2e}   ref_dev {ref_dev[k]:.2e}   bound {bound[k]:.2e}")
    assert (dev <= bound).all(), (dev, bound)
    _note("pj.rand_posterior(solver='celerite')", dev.max(), bound[int(np.argmax(dev))], label)


def test_pj_rand_posterior_dense_route_unchanged(ctx):
    """solver=None: mean + chol(cov + jitter) q from pj.mean and pj.cov, as before"""
    case = next(c for c in CASES if c[0] == "R5-N17-mixed-s2x1")
    label, t, y, s2, A, Bc, C, Dd = case[:8]
    fp = pj.posterior(pj.ScalableGP(0.3, _kernel(A[0], Bc[0], C, Dd))(t, s2), y)
    tau = np.linspace(t[0] - 1.0, t[-1] + 1.0, 12)
    got = pj.rand_posterior(np.random.default_rng(5), fp, tau, 4, ctx=ctx)
    m, K = pj.mean(fp, tau, ctx=ctx), pj.cov(fp, tau, ctx=ctx)
    L = np.linalg.cholesky(K + 1e-14 * np.trace(K) / len(tau) * np.eye(len(tau)))
    want = m[:, None] + L @ np.random.default_rng(5).standard_normal((len(tau), 4))
    assert got.shape == (12, 4) and np.array_equal(got, want)


# ---- 6 --------------------------------------------------------------------------------------------------------------------------------
def test_ppc_timeseries(ctx):
    case = next(c for c in CASES if c[0] == "R33-N33-mixed-s2x1-shift")
    label, t, y, s2, A, Bc, C, Dd, mu, nu, tau, q_data, q_new, eps, shift = case
    B, N = len(A), len(t)
    yerr = np.sqrt(s2)
    ts, t_pred = pj.ppc_timeseries(np.random.default_rng(9), t, y, yerr, A, Bc, C, Dd, mu=mu, nu=nu, ctx=ctx)
    M = len(t_pred)
    assert ts.shape == (M, B) and np.isin(t, t_pred).all() and (np.diff(t_pred) > 0).all() and np.isfinite(ts).all()
    assert np.array_equal(t_pred, np.unique(np.concatenate([t, np.linspace(t[0], t[-1], 2 * N)])))
    rng = np.random.default_rng(9)
    qd, qn, ep = rng.standard_normal((B, N)), rng.standard_normal((B, M)), rng.standard_normal((B, N))
    ds = pj.Dataset(t, y, yerr ** 2, ctx)
    try:
        want = ds.rand_posterior(A, Bc, C, Dd, t_pred, qd, qn, ep, mu=mu, nu=nu)
        assert np.array_equal(ts, want.T)
        # with the shift: exp(realisation + c), as the reference writes it
        ts2, tp2 = pj.ppc_timeseries(np.random.default_rng(9), t, y, yerr, A, Bc, C, Dd, mu=mu, nu=nu, shift=shift, t_pred=tau, ctx=ctx)
        assert np.array_equal(tp2, np.unique(np.concatenate([t, tau]))) and ts2.shape == (len(tp2), B)
        rng = np.random.default_rng(9)
        qd, qn, ep = rng.standard_normal((B, N)), rng.standard_normal((B, len(tp2))), rng.standard_normal((B, N))
        want2 = ds.rand_posterior(A, Bc, C, Dd, tp2, qd, qn, ep, mu=mu, nu=nu, shift=shift)
    finally:
        ds.close()
    back = np.log(ts2) - shift[None, :]
    err = float(np.max(np.abs(back - want2.T)))
    print(f"ppc_timeseries with shift: max |log(ts) - c - draw| = {err:.2e}")
    assert err <= 64 * np.finfo(float).eps * max(1.0, float(np.max(np.abs(want2))) + float(np.max(shift)))     # exp, log and the sum round


# ---- 7 --------------------------------------------------------------------------------------------------------------------------------
def test_zz_worst_deviation_per_family():
    """The table: per family and leg the largest deviation met, with its bound and case (runs last in this module; empty when the tests above
    were deselected)."""
    for name in sorted(WORST):
        dev, bound, label = WORST[name]
        print(f"WORST {name:72s} deviation {dev:.2e}   bound {bound:.2e}   {label}")
    assert all(d <= b for d, b, _ in WORST.values())
