"""GPU tests (-m gpu) of the gradient of log L with respect to the sampled PSD parameters in one device call (pioran_logpdf_batch_theta_grad,
pioran_approx_vjp_batch: Dataset.logpdf_theta_grad(approx_on="device"), Context.approx_vjp).

The reverse mode of approx against a 50-digit truth within the bar of tests/theta_grad_cases.py (whose CPU suite, tests/test_theta_grad_host.py,
shows that the bar catches seeded mistakes); the plumbing of the entry, exactly, against the chain it replaces (the value entry's coefficients,
Dataset.logl_grad, Context.approx_vjp); chunk edges; the shifted models; an independent finite difference of the oracle for the double bend; a draw
that is not positive definite.  Every figure is printed before it is asserted."""
import math
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import pioran_jl_amd as pj  # noqa: E402
from oracle import oracle as O  # noqa: E402

sys.path.insert(0, str(Path(__file__).resolve().parent))
import theta_grad_cases as TC  # noqa: E402

CLS = (pj.SingleBendingPowerLaw, pj.DoubleBendingPowerLaw)
KEYS = ("logl", "status", "grad_theta", "grad_norm", "grad_nu", "grad_mu", "grad_a", "grad_b")


@pytest.fixture(scope="module")
def ctx():
    return pj.Context(0)


@pytest.fixture(scope="module")
def simu_log(golden_dir):
    A = np.loadtxt(golden_dir / "simu_log.txt")
    t, y, yerr = A[:, 0], A[:, 1], A[:, 2]
    return t, y, yerr, 1 / (t[-1] - t[0]), 1 / np.min(np.diff(t)) / 2


def _ran():
    return pj._lib.lib().pioran_celerite_config_name(-1).decode()


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _differing(got, ref, keys):
    """prints, per key, how many entries differ and by how much; returns the keys that differ"""
    bad = []
    for k in keys:
        g, r = np.asarray(got[k]), np.asarray(ref[k])
        if not _same(g, r):
            bad.append(k)
            with np.errstate(invalid="ignore", divide="ignore"):
                print(f"  {k}: {int(np.sum(g != r))} of {g.size} entries differ, largest |got - ref| / max|ref| = {np.nanmax(np.abs(g - r)) / np.nanmax(np.abs(r)):.3e}")
    return bad


def _vjp(ctx, combo, th, nm, ga, gb):
    m, b, i, J, _ = combo
    return ctx.approx_vjp(CLS[m], th, nm, ga, gb, TC.F_MIN, TC.F_MAX, J, TC.S_LOW, TC.S_HIGH, is_integrated_power=bool(i), basis_function=TC.BASIS_NAME[b])


def _grid_cd(J, basis, f_min, f_max):
    """the shared (c, d) of approx's celerite terms, formed as the library forms them (src/psd.jl:250, 266-273)"""
    f0, fM = f_min / 20.0, f_max * 20.0
    sp = [f0 * math.pow(fM / f0, j / (J - 1)) for j in range(J)]
    if basis == "SHO":
        c = np.array([math.sqrt(2.0) * math.pi * f for f in sp])
        return c, c.copy()
    c = np.array([math.pi * f for f in sp])
    return np.concatenate([c, 2.0 * c]), np.concatenate([math.sqrt(3.0) * c, np.zeros(J)])


def _prior(rng, B, model, f_min, f_max):
    """theta as bench.py's prior draws it (tests/theta_grad_cases.py for the second bend), norm, mu, nu"""
    cols = [rng.uniform(-0.25, 2.0, B), np.exp(rng.uniform(np.log(f_min), np.log(f_max), B)), rng.uniform(1.5, 4.0, B)]
    if model == 1:
        cols += [cols[1] * 10.0 ** rng.uniform(0.2, 1.5, B), rng.uniform(2.0, 6.0, B)]
    return (np.column_stack(cols), np.exp(np.log(0.5) + 1.25 * rng.standard_normal(B)), 0.1 * rng.standard_normal(B), rng.gamma(2.0, 0.5, B) + 0.1)


# ---- 1. the kernel against the truth --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("combo", TC.combos(), ids=TC.name)
def test_approx_vjp_against_truth(ctx, combo):
    th, nm, ga, gb, t, S = TC.batch(combo, combo[4])
    g, gn = _vjp(ctx, combo, th, nm, ga, gb)
    d = TC.deviation(g, gn, t, S)
    print(f"{TC.name(combo)}: device deviates by {d:.3e} S_k (bar {TC.bar():.3e}, dev {TC.ref_dev():.3e})")
    assert d <= TC.bar()


@pytest.mark.parametrize("B", TC.LAUNCH_B)
@pytest.mark.parametrize("combo", [(0, 0, 1, 3, 6), (1, 1, 1, 20, 6), (1, 0, 0, 33, 6)], ids=TC.name)
def test_approx_vjp_launch_edges(ctx, combo, B):
    th, nm, ga, gb, t, S = TC.batch(combo, B)
    g, gn = _vjp(ctx, combo, th, nm, ga, gb)
    d = TC.deviation(g, gn, t, S)
    print(f"{TC.name(combo)}, B = {B}: device deviates by {d:.3e} S_k (bar {TC.bar():.3e})")
    assert g.shape == (B, th.shape[1]) and gn.shape == (B,) and d <= TC.bar()
    # a row does not depend on its place in the batch
    k = B - 1
    g1, gn1 = _vjp(ctx, combo, th[k:k + 1], nm[k:k + 1], ga[k:k + 1], gb[k:k + 1])
    assert np.array_equal(g1[0], g[k]) and gn1[0] == gn[k]


def test_approx_vjp_zero_cotangent_is_exactly_zero(ctx):
    for combo in TC.combos():
        th, nm, ga, gb, t, S = TC.batch(combo, combo[4], zero=True)
        g, gn = _vjp(ctx, combo, th, nm, ga, gb)
        assert np.all(g == 0.0) and np.all(gn == 0.0), TC.name(combo)


# ---- 2. plumbing, exactly ----------------------------------------------------------------------------------------------------------------

def _chain(ds, ctx, model, th, nm, f_min, f_max, J, basis, mu, nu, shift=None):
    """what the entry replaces: the value entry's coefficients, the gradient entry on them, the reverse mode of approx on its (grad_a, grad_b)"""
    res = ds.logpdf_theta(CLS[model], th, nm, f_min, f_max, J, basis_function=basis, mu=mu, nu=nu, shift=shift, return_coefs=True)
    A, Bc = res[-2], res[-1]
    C, Dd = _grid_cd(J, basis, f_min, f_max)
    g = ds.logl_grad(A, Bc, C, Dd, mu=mu, nu=nu, shift=shift, cd_grad=False)
    fam = _ran()
    g["grad_theta"], g["grad_norm"] = ctx.approx_vjp(CLS[model], th, nm, g["grad_a"], g["grad_b"], f_min, f_max, J, basis_function=basis)
    return g, fam


@pytest.mark.parametrize("basis", TC.BASIS_NAME)
@pytest.mark.parametrize("model", (0, 1))
def test_entry_equals_the_chain_it_replaces(ctx, simu_log, model, basis):
    t, y, yerr, f_min, f_max = simu_log
    th, nm, mu, nu = _prior(np.random.default_rng(100 + model), 5, model, f_min, f_max)
    ds = pj.Dataset(t, y, yerr ** 2, ctx)
    got = ds.logpdf_theta_grad(CLS[model], th, nm, f_min, f_max, 20, basis_function=basis, mu=mu, nu=nu, approx_on="device", return_coef_grads=True)
    fam = _ran()
    ref, ref_fam = _chain(ds, ctx, model, th, nm, f_min, f_max, 20, basis, mu, nu)
    # mu, nu left out: no gradient asked for, none returned; the intermediate gradients only on request
    g0 = ds.logpdf_theta_grad(CLS[model], th, nm, f_min, f_max, 20, basis_function=basis, approx_on="device")
    r0, _ = _chain(ds, ctx, model, th, nm, f_min, f_max, 20, basis, None, None)
    ds.close()
    assert fam == ref_fam, (fam, ref_fam)
    print(f"model {model}, {basis}: {fam}; status 0 in {int(np.sum(got['status'] == 0))} of {len(th)} draws")
    assert np.any(got["status"] == 0) and got["grad_shift"] is None
    assert not _differing(got, ref, KEYS)
    assert g0["grad_mu"] is None and g0["grad_nu"] is None and "grad_a" not in g0
    for k in ("logl", "status", "grad_theta", "grad_norm"):
        assert _same(g0[k], r0[k]), k


# ---- 3. chunk edges ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("J, option", [(3, None), (20, ("scan_config", "tile")), (20, ("no_tile", True))], ids=["J3", "J20-tile", "J20-no_tile"])
def test_chunk_edge_every_draw_as_a_call_of_its_own(J, option):
    """515 chains cross the 512-chain chunk of the windowed reverse mode; every draw equals the same draw in a call of its own"""
    ctx = pj.Context(0)
    if option:
        ctx.set_option(*option)
    rng = np.random.default_rng(515 + J)
    N, B = 24, 515
    t = np.cumsum(rng.uniform(0.5, 1.5, N)); y = rng.standard_normal(N); s2 = rng.uniform(0.01, 0.1, N)
    f_min, f_max = 1 / (t[-1] - t[0]), 1 / np.min(np.diff(t)) / 2
    th, nm, mu, nu = _prior(rng, B, 0, f_min, f_max)
    ds = pj.Dataset(t, y, s2, ctx)
    kw = dict(basis_function="SHO", approx_on="device", return_coef_grads=True)
    g = ds.logpdf_theta_grad(CLS[0], th, nm, f_min, f_max, J, mu=mu, nu=nu, **kw)
    fam = _ran()
    bad = []
    for i in range(B):
        one = ds.logpdf_theta_grad(CLS[0], th[i:i + 1], nm[i:i + 1], f_min, f_max, J, mu=mu[i:i + 1], nu=nu[i:i + 1], **kw)
        bad += [(i, k) for k in KEYS if not _same(one[k][0], g[k][i])]
    ds.close(); ctx.close()
    print(f"J = {J}, {option}: {fam}; status 0 in {int(np.sum(g['status'] == 0))} of {B} draws; draws that differ: {bad[:8]}")
    assert not bad


# ---- 4. shift --------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("basis", TC.BASIS_NAME)
def test_shifted_models(ctx, simu_log, basis):
    t, ylog, yerr, f_min, f_max = simu_log
    flux = np.exp(ylog) + 0.3                                   # raw flux; draw b conditions on log(flux - shift_b)
    th, nm, mu, nu = _prior(np.random.default_rng(41), 4, 1, f_min, f_max)
    shift = np.array([0.3, 0.25, 0.1, 0.0])
    ds = pj.Dataset(t, flux, (yerr * flux) ** 2, ctx)
    got = ds.logpdf_theta_grad(CLS[1], th, nm, f_min, f_max, 20, basis_function=basis, mu=mu, nu=nu, shift=shift, approx_on="device",
                               return_coef_grads=True)
    fam = _ran()
    ref, ref_fam = _chain(ds, ctx, 1, th, nm, f_min, f_max, 20, basis, mu, nu, shift=shift)
    ds.close()
    print(f"shift, {basis}: {fam}; status 0 in {int(np.sum(got['status'] == 0))} of {len(th)} draws; grad_shift {got['grad_shift']}")
    assert fam == ref_fam and np.any(got["status"] == 0)
    assert not _differing(got, ref, KEYS + ("grad_shift",))


# ---- 5. end to end against an independent path ----------------------------------------------------------------------------------------------

def test_double_bend_against_finite_differences_of_the_oracle(ctx, simu_log):
    """as tests/test_gpu_parity.py::test_gradient_wrt_sampled_parameters, for DoubleBendingPowerLaw: the five-point difference of the oracle's value
    through the oracle's own approx, bar 1e-5 (1 + |fd|)"""
    t, y, yerr, f_min, f_max = simu_log
    th = np.array([[0.82, 0.01, 2.1, 0.08, 3.6], [0.3, 0.05, 2.5, 0.06, 4.5], [0.6, 0.02, 1.8, 0.2, 3.0]])
    var = np.array([np.var(y, ddof=1), 0.5, 2.0]); nu = np.array([1.0, 1.4, 0.8]); mu = np.array([0.0, 0.1, -0.2])
    ds = pj.Dataset(t, y, yerr ** 2, ctx)
    worst = 0.0
    for basis in TC.BASIS_NAME:
        g = ds.logpdf_theta_grad(pj.DoubleBendingPowerLaw, th, var, f_min, f_max, 20, basis_function=basis, mu=mu, nu=nu, approx_on="device")

        def val(p):
            a, b, c, d = O.approx(lambda f: O.double_bending_power_law(f, *p[:5]), f_min, f_max, 20, p[5], basis_function=basis)
            return O.logl(a, b, c, d, t, y - p[7], p[6] * yerr ** 2)
        for i in range(3):
            p0 = np.array([*th[i], var[i], nu[i], mu[i]])
            assert abs(g["logl"][i] - val(p0)) <= 1e-10 * abs(val(p0))
            got = np.array([*g["grad_theta"][i], g["grad_norm"][i], g["grad_nu"][i], g["grad_mu"][i]])
            for k in range(8):
                h = 1e-4 * p0[k] if k in (1, 3) else 1e-4 * max(1.0, abs(p0[k]))
                e = np.zeros(8); e[k] = h
                fd = (8 * (val(p0 + e) - val(p0 - e)) - (val(p0 + 2 * e) - val(p0 - 2 * e))) / (12 * h)
                worst = max(worst, abs(got[k] - fd) / (1 + abs(fd)))
                assert abs(got[k] - fd) <= 1e-5 * (1 + abs(fd)), (basis, i, k, got[k], fd)
    ds.close()
    print(f"double bend: worst |device - finite difference| / (1 + |fd|) = {worst:.2e}")


# ---- 6. a draw that is not positive definite ----------------------------------------------------------------------------------------------------

def test_not_positive_definite_draw(ctx):
    """the recipe of tests/test_gpu_parity.py::test_status_not_positive_definite (a negative amplitude on a series with sigma2 = 1e-8), here through
    a negative variance: status and out are the gradient entry's, the other draws are what they are without it"""
    rng = np.random.default_rng(5)
    t = np.cumsum(rng.uniform(0.1, 2, 50)); y = rng.standard_normal(50); s2 = np.full(50, 1e-8)
    f_min, f_max = 1 / (t[-1] - t[0]), 1 / np.min(np.diff(t)) / 2
    th, nm, mu, nu = _prior(rng, 3, 0, f_min, f_max)
    nm = np.array([1.0, -5.0, 0.7])
    ds = pj.Dataset(t, y, s2, ctx)
    kw = dict(basis_function="SHO", mu=mu, nu=nu, approx_on="device", return_coef_grads=True)
    got = ds.logpdf_theta_grad(CLS[0], th, nm, f_min, f_max, 6, **kw)
    ref, _ = _chain(ds, ctx, 0, th, nm, f_min, f_max, 6, "SHO", mu, nu)
    keep = np.array([0, 2])
    rest = ds.logpdf_theta_grad(CLS[0], th[keep], nm[keep], f_min, f_max, 6, **{**kw, "mu": mu[keep], "nu": nu[keep]})
    ds.close()
    print("status", got["status"], "logl", got["logl"])
    assert got["status"][1] != 0 and got["status"][0] == 0 and got["status"][2] == 0
    assert _same(got["status"], ref["status"]) and _same(got["logl"], ref["logl"])
    for k in KEYS:
        assert _same(got[k][keep], rest[k]), k
        assert _same(got[k], ref[k]), k
