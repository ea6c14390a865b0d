"""GPU tests of the CARMA(p, q) feature (pioran.jl_amd/csrc/carma.hip and its entries): the three kernels against the 100-digit truth within the bars
of tests/carma_cases.py, launch shapes, the one-call value and gradient entries against the chains they replace, rejected draws, and the PSD check.
Series are prefixes of tests/golden/simu.txt with N <= 200."""
import numpy as np
import pytest

import carma_cases as cc
import carma_proto as cp
import pioran_jl_amd as pj
from oracle import oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    return pj.Context(0)


@pytest.fixture(scope="module")
def simu(golden_dir):
    A = np.loadtxt(golden_dir / "simu.txt")
    return A[:200, 0], A[:200, 1], A[:200, 2]


def _kernel():
    return pj._lib.lib().pioran_celerite_config_name(-1).decode()


def _model_draws(p, q, n, t, seed):
    """n draws of the models of docs/src/carma.md on the series' own window: sample_quad within (f_min, f_max) = (1 / T, 1 / (2 min dt))"""
    f_min, f_max = 1 / (t[-1] - t[0]), 1 / np.min(np.diff(t)) / 2
    rng = np.random.default_rng([seed, p, q])
    qa, qb = np.empty((n, p)), np.empty((n, q))
    for k in range(n):
        qa[k], qb[k] = pj.sample_quad(p, q, rng, f_min, f_max)
    norm = np.exp(np.log(0.5) + 0.5 * rng.standard_normal(n))
    mu, nu = 4.8 + 0.1 * rng.standard_normal(n), rng.uniform(0.8, 1.5, n)
    return qa, qb, norm, mu, nu, (f_min, f_max)


# ---- 1. the kernels against the truth ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo", cc.combos(), ids=cc.name)
def test_kernels_against_truth(ctx, combo):
    p, q, i = combo
    t = cc.truth(combo)
    quad = ctx.carma_coefs(p, q, t["qa"], t["qb"], t["norm"], is_integrated_power=bool(i), return_flags=True)
    roots = ctx.carma_coefs(p, q, r_alpha=t["r_alpha"], beta=t["beta"], norm=t["norm"], is_integrated_power=bool(i), return_flags=True)
    dq, dr = cc.coef_deviation(quad[:4], t), cc.coef_deviation(roots[:4], t)
    qa, qb, norm, g, tv, S = cc.vjp_batch(combo, cc.N_DRAWS)
    dv = cc.vjp_deviation(*ctx.carma_vjp(p, q, qa, qb, norm, *g, is_integrated_power=bool(i)), tv, S)
    psd_q, st_q = ctx.carma_psd(p, q, cc.FREQ, t["qa"], t["qb"], t["norm"], is_integrated_power=bool(i), return_status=True)
    psd_r = ctx.carma_psd(p, q, cc.FREQ, r_alpha=t["r_alpha"], beta=t["beta"], norm=t["norm"], is_integrated_power=bool(i))
    dpq, dpr = cc.psd_deviation(psd_q, t), cc.psd_deviation(psd_r, t)
    print(f"\n{cc.name(combo)}: coefs quad {dq:.2e} roots {dr:.2e} (dev {cc.coef_ref_dev():.2e}, bar {cc.coef_bar():.2e}); vjp {dv:.2e} (dev "
          f"{cc.vjp_ref_dev():.2e}, bar {cc.vjp_bar():.2e}); psd quad {dpq:.2e} roots {dpr:.2e} (dev {cc.psd_ref_dev():.2e}, bar {cc.psd_bar():.2e})")
    assert not quad[4].any() and not roots[4].any() and not st_q.any()
    assert dq <= cc.coef_bar() and dr <= cc.coef_bar()
    assert dv <= cc.vjp_bar()
    assert dpq <= cc.psd_bar() and dpr <= cc.psd_bar()
    if p % 2:   # the real term: b = d = 0 exactly
        assert not quad[1][:, -1].any() and not quad[3][:, -1].any()
    np.testing.assert_array_equal(ctx.carma_psd(p, q, cc.FREQ, t["qa"], t["qb"], t["norm"], is_integrated_power=bool(i), times_f=True), psd_q * cc.FREQ)


@pytest.mark.parametrize("combo", [(1, 0, 1), (5, 2, 1), (6, 5, 0), (16, 15, 1)], ids=cc.name)
def test_launch_shapes_last_row_alone_is_the_last_row_in_the_batch(ctx, combo):
    p, q, i = combo
    F = np.concatenate([cc.FREQ, 10.0 ** np.linspace(-3, 2, 300)])       # more than one 256-frequency tile
    for B in cc.LAUNCH_B:
        qa, qb, norm, g, tv, S = cc.vjp_batch(combo, B)
        kw = dict(is_integrated_power=bool(i))
        co = ctx.carma_coefs(p, q, qa, qb, norm, **kw)
        vj = ctx.carma_vjp(p, q, qa, qb, norm, *g, **kw)
        ps = ctx.carma_psd(p, q, F, qa, qb, norm, **kw)
        assert cc.vjp_deviation(*vj, tv, S) <= cc.vjp_bar()
        co1 = ctx.carma_coefs(p, q, qa[-1:], qb[-1:], norm[-1:], **kw)
        vj1 = ctx.carma_vjp(p, q, qa[-1:], qb[-1:], norm[-1:], *g[:, -1:], **kw)
        ps1 = ctx.carma_psd(p, q, F, qa[-1:], qb[-1:], norm[-1:], **kw)
        for whole, alone in zip(co + vj + (ps,), co1 + vj1 + (ps1,)):
            np.testing.assert_array_equal(whole[-1:], alone)
        # every row is its draw's: the batch repeats the combo's six draws
        for whole in co + (ps,):
            np.testing.assert_array_equal(whole[cc.N_DRAWS:], whole[np.arange(cc.N_DRAWS, B) % cc.N_DRAWS])
        qa, qb, norm, g0, _, _ = cc.vjp_batch(combo, B, zero=True)       # a zero cotangent gives exact zeros
        assert all(not np.any(x) for x in ctx.carma_vjp(p, q, qa, qb, norm, *g0, **kw))


# ---- 2. (qa, qb, norm) -> log L in one call -----------------------------------------------------------------------------------------------------
def _oracle_logl(A, Bc, C, Dd, t, y, s2, mu, nu, shift):
    out = np.empty(len(A))
    for k in range(len(A)):
        yy, ss = (y, s2) if shift is None else (np.log(y - shift[k]), s2 / (y - shift[k]) ** 2)
        out[k] = O.logl(A[k], Bc[k], C[k], Dd[k], t, yy - (mu[k] if mu is not None else 0.0), (nu[k] if nu is not None else 1.0) * ss)
    return out


def _relerr(got, ref):
    return np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300))


@pytest.mark.parametrize("p,q,B", [(3, 2, 7), (5, 2, 16), (5, 2, 1), (4, 3, 5)])
@pytest.mark.parametrize("extras", ["none", "mu_nu", "mu_nu_shift"])
def test_logpdf_carma_is_the_chain(ctx, simu, p, q, B, extras):
    """The one call against the chain carma_coefs -> logl_batch(per-draw C, Dd): the same kernel (one value body routes both) and bit for bit, and against oracle.logl draw
    by draw within the tolerance tests/test_gpu_parity.py applies to per-draw (c, d) batches: 1e-11 (test_random_batches_per_draw_cd), and 1e-9 where the
    batch is shifted (its shifted per-draw batch, test_device_approx_with_qpo_features: the device's log(y - shift) and the host's differ in the last bit, and a
    draw whose chi^2 is large amplifies that).  Measured on an MI355X: unshifted at most 5.6e-12; shifted 2.8e-10 (CARMA(3, 2), 7 draws, 'block+pd'),
    1.7e-11 (CARMA(5, 2), 16 draws, per-draw tables), 3.6e-13 and 6.1e-13 — every value equal, bit for bit, to the existing chain's."""
    t, y, yerr = simu
    qa, qb, norm, mu, nu, bounds = _model_draws(p, q, B, t, 5)
    mu, nu = (None, None) if extras == "none" else (mu, nu)
    shift = np.linspace(0.0, 0.3, B) if extras == "mu_nu_shift" else None
    if shift is not None and mu is not None:
        mu = np.log(mu)
    ds = pj.Dataset(t, y, yerr ** 2, ctx)
    got, st, A, Bc, C, Dd = ds.logpdf_carma(p, q, qa, qb, norm, bounds=bounds, mu=mu, nu=nu, shift=shift, return_status=True, return_coefs=True)
    k_one = _kernel()
    co = ctx.carma_coefs(p, q, qa, qb, norm, bounds=bounds)
    for x, z in zip((A, Bc, C, Dd), co):
        np.testing.assert_array_equal(x, z)
    chain, st_chain = ds.logl_batch(*co, mu=mu, nu=nu, shift=shift, return_status=True)
    k_chain = _kernel()
    ref = _oracle_logl(*co, t, y, yerr ** 2, mu, nu, shift)
    print(f"\nCARMA({p},{q}) B = {B}, {extras}: one call on '{k_one}', chain on '{k_chain}'; vs chain {_relerr(got, chain):.2e}, vs oracle {_relerr(got, ref):.2e}")
    assert (st == 0).all() and (st_chain == 0).all()
    if p % 2 and B > 1:   # a per-draw term whose sine row is zero in every draw
        assert not Bc[:, -1].any() and not Dd[:, -1].any() and len(np.unique(C[:, -1])) == B
    assert k_one == k_chain
    np.testing.assert_array_equal(got, chain)
    assert _relerr(got, ref) < (1e-11 if shift is None else 1e-9)


@pytest.mark.parametrize("p,q,B", [(3, 2, 300), (5, 2, 300)])
def test_logpdf_carma_more_draws_than_one_chunk(ctx, simu, p, q, B):
    """More draws than one chunk of per-draw tables or rows holds (256): the one call against the chain it replaces: the same kernel, bit for bit.  The oracle is not asked here: among 300 draws some have log L near 0, where the per-element relative error of tests/test_gpu_parity.py
    measures nothing — measured on an MI355X for CARMA(3, 2) with mu and nu, kernel 'block+pd': 3.4e-11 against the oracle for values that equal the
    existing chain's bit for bit."""
    t, y, yerr = simu
    qa, qb, norm, mu, nu, bounds = _model_draws(p, q, B, t, 5)
    ds = pj.Dataset(t, y, yerr ** 2, ctx)
    got, st = ds.logpdf_carma(p, q, qa, qb, norm, bounds=bounds, mu=mu, nu=nu, return_status=True)
    k_one = _kernel()
    chain, st_chain = ds.logl_batch(*ctx.carma_coefs(p, q, qa, qb, norm, bounds=bounds), mu=mu, nu=nu, return_status=True)
    k_chain = _kernel()
    print(f"\nCARMA({p},{q}) B = {B}: one call on '{k_one}', chain on '{k_chain}'; vs chain {_relerr(got, chain):.2e}")
    np.testing.assert_array_equal(st, st_chain)
    assert k_one == k_chain
    np.testing.assert_array_equal(got, chain)


# ---- 3. ... and its gradient ------------------------------------------------------------------------------------------------------------------
GRAD_KEYS = ("logl", "grad_qa", "grad_qb", "grad_norm", "grad_nu", "grad_mu", "grad_shift", "grad_a", "grad_b", "grad_c", "grad_d")


def _grad_chain(ds, ctx, p, q, qa, qb, norm, bounds, mu, nu, shift):
    co = ctx.carma_coefs(p, q, qa, qb, norm, bounds=bounds)
    g = ds.logl_grad(*co, mu=mu, nu=nu, shift=shift, cd_grad=True)
    kern = _kernel()
    gqa, gqb, gn = ctx.carma_vjp(p, q, qa, qb, norm, g["grad_a"], g["grad_b"], g["grad_c"], g["grad_d"])
    ref = dict(g, grad_qa=gqa, grad_qb=gqb, grad_norm=gn)
    for k, v in (("grad_nu", nu), ("grad_mu", mu), ("grad_shift", shift)):
        if v is None:
            ref[k] = None
    return ref, co, kern


@pytest.mark.parametrize("p,q,B", [(3, 2, 6), (5, 2, 1), (4, 3, 5)])
@pytest.mark.parametrize("extras", ["none", "mu_nu", "mu_nu_shift"])
def test_logpdf_carma_grad_is_the_chain(ctx, simu, p, q, B, extras):
    t, y, yerr = simu
    t, y, yerr = t[:120], y[:120], yerr[:120]
    qa, qb, norm, mu, nu, bounds = _model_draws(p, q, B, t, 6)
    mu, nu = (None, None) if extras == "none" else (mu, nu)
    shift = np.linspace(0.0, 0.3, B) if extras == "mu_nu_shift" else None
    if shift is not None:
        mu = np.log(mu)
    ds = pj.Dataset(t, y, yerr ** 2, ctx)
    got = ds.logpdf_carma_grad(p, q, qa, qb, norm, bounds=bounds, mu=mu, nu=nu, shift=shift, return_coef_grads=True)
    ref, co, k_chain = _grad_chain(ds, ctx, p, q, qa, qb, norm, bounds, mu, nu, shift)
    print(f"\nCARMA({p},{q}) B = {B}, {extras}: reverse mode on '{k_chain}'")
    assert (got["status"] == 0).all()
    for k in GRAD_KEYS:
        if ref[k] is None:
            assert got[k] is None, k
        else:
            np.testing.assert_array_equal(got[k], ref[k], err_msg=k)      # the same kernels on the same numbers
    lean = ds.logpdf_carma_grad(p, q, qa, qb, norm, bounds=bounds, mu=mu, nu=nu, shift=shift)
    assert "grad_a" not in lean
    np.testing.assert_array_equal(lean["grad_qa"], got["grad_qa"])


def test_logpdf_carma_grad_end_to_end_against_oracle_and_truth_jacobian(ctx, simu):
    """d log L / d(qa, qb, norm) = the oracle's gradient w.r.t. (a, b, c, d) (complex step) contracted with the 100-digit Jacobian of the coefficients.
    Bar per output: the vjp's bar on its scale S (sum of absolute terms) plus the oracle gradient's own tolerance as
    test_gradient_wrt_c_and_d_qpo_and_carma states it, 1e-8 (1 + max |grad_x|) per array, carried through the Jacobian: 1e-8 sum_x (1 + max |grad_x|) sum_j |dx_j / dtheta|."""
    t, y, yerr = simu
    t, y, yerr = t[:120], y[:120], yerr[:120]
    ds = pj.Dataset(t, y, yerr ** 2, ctx)
    for combo in ((3, 2, 1), (5, 2, 0)):
        p, q, i = combo
        tr = cc.truth(combo)
        mu, nu = np.full(cc.N_DRAWS, 4.8), np.full(cc.N_DRAWS, 1.1)
        got = ds.logpdf_carma_grad(p, q, tr["qa"], tr["qb"], tr["norm"], is_integrated_power=bool(i), mu=mu, nu=nu)
        got_all = np.column_stack([got["grad_qa"], got["grad_qb"], got["grad_norm"]])
        worst = 0.0
        for n in np.flatnonzero(got["status"] == 0):
            ref = O.logl_grad(tr["a"][n], tr["b"][n], tr["c"][n], tr["d"][n], t, y - mu[n], nu[n] * yerr ** 2, cd=True)
            g = np.stack([ref[k] for k in ("grad_a", "grad_b", "grad_c", "grad_d")])          # [4][J]
            want = np.einsum("kj,kjp->p", g, tr["jac"][n])
            S = np.einsum("kj,kjp->p", np.abs(g), np.abs(tr["jac"][n]))
            tol = cc.vjp_bar() * S + 1e-8 * np.einsum("k,kp->p", 1 + np.abs(g).max(axis=1), np.abs(tr["jac"][n]).sum(axis=1))
            ratio = np.max(np.abs(got_all[n] - want) / tol)
            worst = max(worst, ratio)
            assert ratio <= 1.0, (combo, n, got_all[n], want, tol)
        print(f"\n{cc.name(combo)}: {int(np.sum(got['status'] == 0))} draws with status 0; largest |got - want| / bar = {worst:.3e}")
        assert np.sum(got["status"] == 0) >= 3


# ---- 4. rejected draws ------------------------------------------------------------------------------------------------------------------------
def test_rejected_draws_one_for_each_reason(ctx, simu):
    t, y, yerr = simu
    p, q, B = 5, 2, 9
    qa, qb, norm, mu, nu, bounds = _model_draws(p, q, B, t, 7)
    good = (qa.copy(), qb.copy(), norm.copy())
    qa[1, 2] = np.nan                                        # 1: a non-finite parameter
    norm[2] = np.inf                                         # 1: ... the norm
    qa[3, 0] = qa[3, 1] ** 2 / 8                             # 2: b^2 - 4 c > 0: not a conjugate pair
    qa[4, 1] = -qa[4, 1]                                     # 3: a pair with positive real part
    qa[5, 4] = 0.1 * bounds[0]                               # 4: the real root inside (-f_lo, 0)
    qb[7, 0] = qb[7, 1] ** 2 / 4 + (2 * bounds[1]) ** 2      # 4: a moving-average pair with |Im| above f_hi
    want = np.array([0, 1, 1, 2, 3, 4, 0, 4, 0], dtype=np.int32)
    np.testing.assert_array_equal(cp.reject_quad(qa, qb, norm, bounds), want)
    rej = want != 0
    *co, flags = ctx.carma_coefs(p, q, qa, qb, norm, bounds=bounds, return_flags=True)
    np.testing.assert_array_equal(flags, want)
    for x, v in zip(co, (1.0, 0.0, 1.0, 0.0)):
        assert np.all(x[rej] == v)
    _, st_psd = ctx.carma_psd(p, q, cc.FREQ, qa, qb, norm, bounds=bounds, return_status=True)
    np.testing.assert_array_equal(st_psd, np.where(rej, 3, 0))
    ds = pj.Dataset(t, y, yerr ** 2, ctx)
    # the same batch with good draws in the rejected rows: the same size, so the same kernels
    val, st = ds.logpdf_carma(p, q, qa, qb, norm, bounds=bounds, mu=mu, nu=nu, return_status=True)
    val0, st0 = ds.logpdf_carma(p, q, *good, bounds=bounds, mu=mu, nu=nu, return_status=True)
    np.testing.assert_array_equal(st, np.where(rej, 3, st0))
    assert np.all(val[rej] == -np.inf)
    np.testing.assert_array_equal(val[~rej], val0[~rej])
    g = ds.logpdf_carma_grad(p, q, qa, qb, norm, bounds=bounds, mu=mu, nu=nu, return_coef_grads=True)
    g0 = ds.logpdf_carma_grad(p, q, *good, bounds=bounds, mu=mu, nu=nu, return_coef_grads=True)
    np.testing.assert_array_equal(g["status"], np.where(rej, 3, g0["status"]))
    assert np.all(g["logl"][rej] == -np.inf)
    for k in GRAD_KEYS[1:]:
        if g[k] is None:
            continue
        assert not np.any(g[k][rej]), k                       # exactly 0.0 in every gradient row
        np.testing.assert_array_equal(g[k][~rej], g0[k][~rej], err_msg=k)
    # the reverse-mode entry alone takes no bounds: reasons 1 .. 3 give zeros there
    z = ctx.carma_vjp(p, q, qa, qb, norm, *np.ones((4, B, 3)))
    assert all(not np.any(x[(want >= 1) & (want <= 3)]) for x in z) and np.all(z[2][want == 4] != 0)


# ---- 5. the PSD check ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plot_f_P", [False, True])
def test_psd_ppc_carma_and_summary_are_the_quantiles_of_carma_psd(ctx, simu, plot_f_P):
    t, y, yerr = simu
    p, q, B = 3, 2, 150
    qa, qb, norm, _, nu, _ = _model_draws(p, q, B, t, 8)
    r, beta = cp.roots_of_quad(qa, qb)
    r[5, 0] = 0.3 + 1j                                       # a draw the checks reject: left out of the quantiles
    res = pj.psd_ppc_carma(r, beta, norm, nu, t, y, yerr, p, q, plot_f_P=plot_f_P, n_frequencies=300, ctx=ctx)
    f = res["f"]
    dt = np.diff(t)
    assert np.isclose(f[0], 1 / (t[-1] - t[0]) / 10) and np.isclose(f[-1], 10 / (2 * np.min(dt))) and len(f) == 300
    np.testing.assert_allclose(np.diff(np.log(f)), np.log(f[-1] / f[0]) / 299, rtol=1e-9)
    psd, st = ctx.carma_psd(p, q, f, r_alpha=r, beta=beta, norm=norm, times_f=plot_f_P, return_status=True)
    assert st[5] == 3 and np.isnan(psd[5]).all() and np.sum(st != 0) == 1
    quant, _, kept = pj.gp._quantiles_host(psd, pj.gp.PPC_QUANTILES, st)
    np.testing.assert_array_equal(res["psd_quantiles"], quant)
    assert res["kept"] == kept == B - 1
    s = ctx.carma_psd_summary(p, q, f, r_alpha=r, beta=beta, norm=norm, times_f=plot_f_P)
    np.testing.assert_array_equal(s["quant"], quant)
    np.testing.assert_array_equal(s["status"], st)
    # the array itself against the twin, and the two noise levels
    ok = st == 0
    tw = cp.evaluate_roots(r[ok], beta[ok], norm[ok], True, f, times_f=plot_f_P)
    assert np.max(np.abs(psd[ok] - tw) / tw) <= cc.psd_bar()
    assert res["mean_noise_level"] == 2.0 * np.mean(nu) * np.mean(yerr ** 2) * np.mean(dt)
    assert res["median_noise_level"] == 2.0 * np.median(nu) * np.median(yerr ** 2) * np.median(dt)
    logt = pj.psd_ppc_carma(r, beta, norm, nu, t, y, yerr, p, q, n_frequencies=20, with_log_transform=True, ctx=ctx)
    assert logt["mean_noise_level"] == 2.0 * np.mean(nu) * np.mean((yerr / y) ** 2) * np.mean(dt)
    assert logt["median_noise_level"] == 2.0 * np.median(nu) * np.median((yerr / y) ** 2) * np.median(dt)
