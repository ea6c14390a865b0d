"""GPU tests (-m gpu) of the posterior variance through the celerite factorisation (pioran_celerite_predict_var: Dataset.predict_var,
pj.predict_var, pj.var, pj.std(solver="celerite")).

The result is var = k(0) - q1 - q2, a difference of numbers of the size of k(0) = sum(a): every bound is absolute on that scale.
  1e-10 k(0)  against diag(oracle.predict_cov_numpy): 200 x the 5e-13 k(0) the numpy prototype of the same recurrences measured on the CPU at
              N = 400 (room for N five times longer and another summation order), a hundred times tighter than the project's 1e-8 bar.
  N = 1e4     against the prototype on the same inputs: 10 x the prototype's own deviation from the dense oracle at N = 4000 (computed here),
              never looser than 1e-8 k(0).
Every figure is printed before it is asserted.

Below those (tests 7 - 10): the kernels against a truth that is neither them nor their prototype — oracle.predict_var_truth, dense in long
double, and the 50-digit values of tests/golden/predict_var_truth.npz — at the shapes where predict_var_fwd_kernel<H> / predict_var_bwd_kernel<H>
take another path and on ill-conditioned draws, with the bound max(20 x the prototype's deviation on the same draw, 256 eps) k(0) of
tests/predict_var_cases.py (cases, checker and the reasoning behind the bound live there; the CPU suite shows that the cases catch seeded
mistakes)."""
import importlib.util
import json
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import pioran_jl_amd as pj  # noqa: E402
from oracle import oracle as O  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]
BOUND = 1e-10
sys.path.insert(0, str(Path(__file__).resolve().parent))
import predict_var_cases as PV  # noqa: E402


@pytest.fixture(scope="module")
def ctx():
    return pj.Context(0)


@pytest.fixture(scope="module")
def proto():
    spec = importlib.util.spec_from_file_location("predict_var_proto", ROOT / "tools" / "predict_var_proto.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def full_size():
    return O.synthetic_series(10_000)


def make_tau(t, M, seed):
    """M evaluation times in no particular order: inside the span, outside it on both sides, exact data times, duplicates."""
    rng = np.random.default_rng(seed)
    span = t[-1] - t[0]
    n_out, n_data, n_dup = M // 10, M // 5, M // 20
    inner = rng.uniform(t[0], t[-1], M - n_out - n_data - n_dup)
    out = np.concatenate([t[0] - rng.uniform(0, 0.05 * span, n_out // 2), t[-1] + rng.uniform(0, 0.05 * span, n_out - n_out // 2)])
    data = rng.choice(t, n_data, replace=False)
    dup = np.concatenate([inner[:n_dup // 2], data[:n_dup - n_dup // 2]])
    tau = np.concatenate([inner, out, data, dup])
    assert len(tau) == M
    return rng.permutation(tau)


def celerite_sum():
    a = np.array([1.3, 0.6, 0.25]); c = np.array([0.02, 0.11, 0.6]); d = np.array([0.05, 0.4, 2.1])
    b = np.array([0.4, -0.5, 0.3]) * a * c / d          # mixed signs; |b d| <= a c keeps every term a valid covariance
    return a, b, c, d


def carma32(golden_dir):
    g = json.loads((golden_dir / "reference_literals.json").read_text())["carma32"]
    return O.carma_celerite_coefs(g["p"], np.array([complex(*z) for z in g["r_alpha"]]), g["beta"], g["norm"])


def against_oracle(ctx, label, t, s2, A, Bc, C, Dd, nu, tau):
    ds = pj.Dataset(t, np.zeros(len(t)), s2, ctx)
    got, st = ds.predict_var(A, Bc, C, Dd, tau, nu=nu, return_status=True)
    assert pj._lib.lib().pioran_celerite_config_name(-1) == b"wide (step-by-step variance)"
    ds.close()
    assert (st == 0).all(), st
    for k in range(len(A)):
        ref = np.diag(O.predict_cov_numpy(A[k], Bc[k], C, Dd, tau, t, (1.0 if nu is None else nu[k]) * s2))
        k0 = A[k].sum()
        err = np.max(np.abs(got[k] - ref)) / k0
        print(f"{label} draw {k}: max |delta| / k(0) = {err:.2e}   min var / k(0) = {ref.min() / k0:.2e}")
        assert err <= BOUND, (label, k, err)


# ---- 1 --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("basis,N", [("SHO", 2000), ("DRWCelerite", 1500)])
def test_against_dense_oracle_synthetic(ctx, basis, N):
    """SHO-20 (40 rows) and DRWCelerite-20 (60 rows) on the synthetic series, M = 1000, two prior draws with their own nu."""
    t, y, yerr = O.synthetic_series(N)
    A, Bc, C, Dd, mu, nu = O.theta_to_coefs(O.synthetic_theta(2, t, y), t, 20, basis)
    against_oracle(ctx, f"{basis}-20 N={N}", t, yerr ** 2, A, Bc, C, Dd, nu, make_tau(t, 1000, 11))


def test_against_dense_oracle_simu(ctx, golden_dir):
    """The reference's test series (N = 489), M = 1000: a Celerite sum with mixed-sign b (6 rows), CARMA(3,2) (3 rows, one of a real term)."""
    S = np.loadtxt(golden_dir / "simu.txt")
    t, yerr = S[:, 0], S[:, 2]
    tau = make_tau(t, 1000, 12)
    a, b, c, d = celerite_sum()
    against_oracle(ctx, "Celerite sum", t, yerr ** 2, a[None], b[None], c, d, None, tau)
    a, b, c, d = carma32(golden_dir)
    against_oracle(ctx, "CARMA(3,2)", t, yerr ** 2, a[None], b[None], c, d, None, tau)


# ---- 2 --------------------------------------------------------------------------------------------------------------------------------
def test_full_size_against_prototype(ctx, proto, full_size):
    """N = 1e4, M = 2000, SHO-20: the kernels against the numpy prototype of the same recurrences.  Bound: 10 x the prototype's deviation
    from the dense oracle at N = 4000, at most 1e-8 k(0)."""
    t, y, yerr = full_size
    A, Bc, C, Dd, mu, nu = O.theta_to_coefs(O.synthetic_theta(1, t, y), t, 20, "SHO")
    a, b, k0 = A[0], Bc[0], A[0].sum()
    t4, s4 = t[:4000], nu[0] * yerr[:4000] ** 2
    tau4 = make_tau(t4, 400, 21)
    dev = np.max(np.abs(proto.predict_var(a, b, C, Dd, t4, s4, tau4) - np.diag(O.predict_cov_numpy(a, b, C, Dd, tau4, t4, s4)))) / k0
    bound = min(10 * dev, 1e-8)
    tau = make_tau(t, 2000, 22)
    ref = proto.predict_var(a, b, C, Dd, t, nu[0] * yerr ** 2, tau)
    ds = pj.Dataset(t, y, yerr ** 2, ctx)
    got, st = ds.predict_var(A, Bc, C, Dd, tau, nu=nu, return_status=True)
    ds.close()
    err = np.max(np.abs(got[0] - ref)) / k0
    print(f"prototype vs dense oracle at N = 4000: {dev:.2e} k(0);  GPU vs prototype at N = 1e4: {err:.2e} k(0)  (bound {bound:.2e})")
    assert st[0] == 0
    assert err <= bound, (err, bound)


# ---- 3 --------------------------------------------------------------------------------------------------------------------------------
def test_against_the_dense_std(ctx):
    """pj.std(fp, tau, solver="celerite") against the product's own dense pj.std (N = 2000, M = 500); the default stays the dense route."""
    t, y, yerr = O.synthetic_series(2000)
    f_min, f_max = 1 / (t[-1] - t[0]), 1 / np.min(np.diff(t)) / 2
    R = pj.approx(pj.SingleBendingPowerLaw(0.82, 0.01, 3.3), f_min, f_max, 20, np.var(y, ddof=1))
    fp = pj.posterior(pj.ScalableGP(0.1, R)(t, yerr ** 2), y)
    tau = make_tau(t, 500, 31)
    dense = pj.std(fp, tau, ctx=ctx)
    assert np.array_equal(dense, np.sqrt(np.diag(pj.cov(fp, tau, ctx=ctx))))
    cel = pj.std(fp, tau, ctx=ctx, solver="celerite")
    v = pj.var(fp, tau, ctx=ctx)
    assert np.array_equal(cel, np.sqrt(np.maximum(v, 0.0)))
    k0 = np.sum(np.real(R.celerite_coefs()[0]))
    err = np.max(np.abs(v - dense ** 2)) / k0
    print(f"celerite variance vs dense std**2: max |delta| / k(0) = {err:.2e}")
    assert err <= BOUND, err
    assert np.array_equal(pj.predict_var(R, tau, t, yerr ** 2, ctx=ctx), v)
    assert np.array_equal(pj.var(fp, ctx=ctx), pj.predict_var(R, t, t, yerr ** 2, ctx=ctx))      # tau defaults to the data times


# ---- 4 --------------------------------------------------------------------------------------------------------------------------------
def test_order_batching_and_per_draw_tables(ctx):
    t, y, yerr = O.synthetic_series(1500)
    A, Bc, C, Dd, mu, nu = O.theta_to_coefs(O.synthetic_theta(64, t, y), t, 20, "SHO")
    tau = make_tau(t, 700, 41)
    ds = pj.Dataset(t, y, yerr ** 2, ctx)
    # unsorted tau = the permuted result of sorted tau
    o = np.argsort(tau, kind="stable")
    v = ds.predict_var(A[:3], Bc[:3], C, Dd, tau, nu=nu[:3])
    vs = ds.predict_var(A[:3], Bc[:3], C, Dd, tau[o], nu=nu[:3])
    assert np.array_equal(v[:, o], vs)
    # 64 draws with per-draw nu in one call = the 64 single calls
    vb, st = ds.predict_var(A, Bc, C, Dd, tau, nu=nu, return_status=True)
    assert (st == 0).all()
    for k in range(64):
        assert np.array_equal(ds.predict_var(A[k:k + 1], Bc[k:k + 1], C, Dd, tau, nu=nu[k:k + 1])[0], vb[k]), k
    # more draws than one chunk of the entry holds (256): 300 draws = the 64 repeated
    rep = np.arange(300) % 64
    assert np.array_equal(ds.predict_var(A[rep], Bc[rep], C, Dd, tau, nu=nu[rep]), vb[rep])
    # per-draw (c, d) arrays whose rows are all equal = the shared call
    vp = ds.predict_var(A[:5], Bc[:5], np.tile(C, (5, 1)), np.tile(Dd, (5, 1)), tau, nu=nu[:5])
    assert np.array_equal(vp, vb[:5])
    # ... and rows that differ: every draw against its own shared call
    C2 = np.tile(C, (2, 1)); C2[1] *= 1.1
    vq = ds.predict_var(A[:2], Bc[:2], C2, np.tile(Dd, (2, 1)), tau)
    assert np.array_equal(vq[0], ds.predict_var(A[:1], Bc[:1], C2[0], Dd, tau)[0])
    assert np.array_equal(vq[1], ds.predict_var(A[1:2], Bc[1:2], C2[1], Dd, tau)[0])
    ds.close()


# ---- 5 --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 32])
def test_full_size_properties(ctx, full_size, B):
    """N = M = 1e4: range, the noise bound at data times, and 64 spot times through the existing posterior mean:
    k*' K^-1 k* is the posterior mean at tau_m of the 'series' y = k*_m."""
    t, y, yerr = full_size
    N = len(t)
    A, Bc, C, Dd, mu, nu = O.theta_to_coefs(O.synthetic_theta(B, t, y), t, 20, "SHO")
    rng = np.random.default_rng(50 + B)
    span = t[-1] - t[0]
    tau = np.concatenate([t[::2], rng.uniform(t[0], t[-1], N // 2 - 200), t[0] - rng.uniform(0, 0.02 * span, 100), t[-1] + rng.uniform(0, 0.02 * span, 100)])
    assert len(tau) == N
    perm = rng.permutation(N)
    tau = tau[perm]
    is_data = np.argsort(perm)[:N // 2]                 # positions of t[::2] in tau
    assert np.array_equal(tau[is_data], t[::2])
    ds = pj.Dataset(t, y, yerr ** 2, ctx)
    v, st = ds.predict_var(A, Bc, C, Dd, tau, nu=nu, return_status=True)
    ds.close()
    assert (st == 0).all()
    k0 = A.sum(axis=1)[:, None]
    print(f"B = {B}: min var / k(0) = {np.min(v / k0):.3e}   max var / k(0) = {np.max(v / k0):.15f}")
    assert (v >= 0).all() and (v <= k0 * (1 + 1e-12)).all()
    assert (v[:, is_data] <= nu[:, None] * (yerr[::2] ** 2)[None, :]).all()
    spots = rng.choice(N, 64, replace=False)
    worst = 0.0
    for i, m in enumerate(spots):
        k = i % B
        lag = np.abs(tau[m] - t)[:, None]
        ks = (np.exp(-C * lag) * (A[k] * np.cos(Dd * lag) + Bc[k] * np.sin(Dd * lag))).sum(axis=1)      # k*_n = k(|tau_m - t_n|)
        dm = pj.Dataset(t, ks, yerr ** 2, ctx)
        q = dm.predict(A[k:k + 1], Bc[k:k + 1], C, Dd, tau[m:m + 1], nu=nu[k:k + 1])[0, 0]
        dm.close()
        worst = max(worst, abs(v[k, m] - (k0[k, 0] - q)) / k0[k, 0])
    print(f"B = {B}: 64 spot times against k(0) - predict(k*): max |delta| / k(0) = {worst:.2e}")
    assert worst <= 1e-8


# ---- 6 --------------------------------------------------------------------------------------------------------------------------------
def test_limits_and_status(ctx):
    t, y, yerr = O.synthetic_series(600)
    ds = pj.Dataset(t, y, yerr ** 2, ctx)
    tau = make_tau(t, 100, 61)
    # 33 two-row terms = 66 rows: unsupported
    J = 33
    c = np.linspace(0.01, 1.0, J); d = np.linspace(0.05, 3.0, J)
    with pytest.raises(pj._lib.PioranHipError, match="unsupported"):
        ds.predict_var(np.full((1, J), 0.1), np.zeros((1, J)), c, d, tau)
    A, Bc, C, Dd, mu, nu = O.theta_to_coefs(O.synthetic_theta(5, t, y), t, 20, "SHO")
    # M = 0
    e, st = ds.predict_var(A, Bc, C, Dd, np.empty(0), return_status=True)
    assert e.shape == (5, 0) and (st == 0).all()
    # a draw that is not positive definite: status 2 and NaN, its neighbours untouched
    good = ds.predict_var(A, Bc, C, Dd, tau, nu=nu)
    Ab = A.copy(); Ab[2] = -A[2]
    v, st = ds.predict_var(Ab, Bc, C, Dd, tau, nu=nu, return_status=True)
    assert list(st) == [0, 0, 2, 0, 0]
    assert np.isnan(v[2]).all()
    assert np.array_equal(v[[0, 1, 3, 4]], good[[0, 1, 3, 4]])
    with pytest.raises(np.linalg.LinAlgError):
        pj.predict_var(pj.Celerite(-1.0, 0.0, 0.5, 0.0), tau[:5], t[:70], np.zeros(70), ctx=ctx)
    with pytest.raises(ValueError):
        ds.predict_var(A, Bc, C, Dd, np.array([0.0, np.nan]))
    ds.close()


# ---- 7 --------------------------------------------------------------------------------------------------------------------------------
def gpu_impl(ctx):
    """Dataset.predict_var as an `impl` of predict_var_cases.check; (c, d) per draw goes draw by draw inside the entry"""
    def impl(A, Bc, C, Dd, t, s2, nu, tau):
        ds = pj.Dataset(t, np.zeros(len(t)), s2, ctx)
        try:
            v, st = ds.predict_var(A, Bc, C, Dd, tau, nu=nu, return_status=True)
        finally:
            ds.close()
        assert pj._lib.lib().pioran_celerite_config_name(-1) == b"wide (step-by-step variance)"
        return v, st
    return impl


@pytest.mark.parametrize("case", list(PV.edge_cases()), ids=lambda c: c[0])
def test_edge_shapes_against_truth(ctx, case):
    """Rows on both sides of every H = 16, 32, 48, 64, series around the VD = 4 prefetch depth, evaluation times all before / all after / on the
    data / alone / forty in one gap; each with sigma2 as drawn and x 1e-6.  Three draws with their own nu, against the long-double truth."""
    PV.check(gpu_impl(ctx), case)


# ---- 8 --------------------------------------------------------------------------------------------------------------------------------
def test_fuzz_slice_against_truth(ctx):
    """40 seeded random shapes (R 1..64, N 1..120 with long gaps, M 1..60, 1..4 draws, sigma2 x 10^U(-7, 0)); shared (c, d): one launch,
    (c, d) per draw: the entry's draw-by-draw route."""
    worst, n = 0.0, 0
    for case in PV.fuzz_cases(40):
        worst = max(worst, PV.check(gpu_impl(ctx), case).max())
        n += 1
    print(f"fuzz: {n} cases, worst deviation {worst:.2e} k(0)")
    assert n == 40


# ---- 9 --------------------------------------------------------------------------------------------------------------------------------
def test_ill_conditioned_draws_against_truth(ctx, proto, golden_dir):
    """The nine draws of tests/golden/predict_var_truth.npz (SHO-20; ratio = nu min sigma2 / k(0) from 5.7e-11): N = 150 against the 50-digit
    truth, N = 1000 against the long-double one.  Bound per draw: 20 x the prototype's deviation from the same truth, computed here, with the
    floor of predict_var_cases.  Sorted and permuted evaluation times give the permuted result bit for bit."""
    Q = np.load(golden_dir / "quad_truth.npz")
    draws = PV.fixture_draws(golden_dir)
    assert len(draws) == 9
    F = np.load(golden_dir / "predict_var_truth.npz")
    rng = np.random.default_rng(91)
    for tag in ("n150", "n1000"):
        idx, tau, t, yerr = F[f"{tag}_idx"], F[f"{tag}_tau"], Q[f"{tag}_t"], Q[f"{tag}_yerr"]
        A, Bc, C, Dd, nu = Q[f"{tag}_A"][idx], Q[f"{tag}_Bc"][idx], Q[f"{tag}_C"], Q[f"{tag}_Dd"], Q[f"{tag}_nu"][idx]
        ds = pj.Dataset(t, np.zeros(len(t)), yerr ** 2, ctx)
        got, st = ds.predict_var(A, Bc, C, Dd, tau, nu=nu, return_status=True)
        o = np.argsort(tau, kind="stable")
        perm = rng.permutation(len(tau))
        got_sorted = ds.predict_var(A, Bc, C, Dd, tau[o], nu=nu)
        got_perm = ds.predict_var(A, Bc, C, Dd, tau[perm], nu=nu)
        ds.close()
        assert (st == 0).all(), st
        fails = []
        for k, (label, a, b, c, d, t_, s2, tau_, truth, ratio) in enumerate(x for x in draws if x[0].startswith(tag + " ")):
            k0 = a.sum()
            assert np.array_equal(a, A[k]) and np.array_equal(tau_, tau)
            pdev = float(np.max(np.abs(proto.predict_var(a, b, c, d, t_, s2, tau_) - truth))) / k0
            dev = float(np.max(np.abs(got[k] - truth))) / k0
            bound = max(PV.MARGIN * pdev, PV.FLOOR)
            print(f"{label}: ratio {ratio:.1e}   deviation {dev:.2e} k(0)   prototype {pdev:.2e}   bound {bound:.2e}   min var / k(0) {float(truth.min()) / k0:.2e}")
            if not dev <= bound:
                fails.append((label, dev, bound))
        assert not fails, fails
        assert np.array_equal(got[:, o], got_sorted)
        assert np.array_equal(got[:, perm], got_perm)


# ---- 10 -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [(16, 32, 48, 64), (1, 17, 33, 49)], ids=["H_full", "H_one_live_lane_more"])
def test_every_instantiation_runs(ctx, rows):
    """Each of the four instantiations with every lane of H live and with one row (R = 1) or one row past the smaller H, on 70 draws: more
    workgroups than one per SIMD of a CU, a multiple of nothing.  A draw that is not positive definite, first, in the middle and last:
    status 2 and NaN for it, every other row bit-identical to the call without it; three of the good rows against the long-double truth."""
    B, N = 70, 37
    for R in rows:
        rng = np.random.default_rng([20261020, R])
        nreal = R % 2
        t, s2, A, Bc, C, Dd, nu = PV._draws(rng, N, (R + nreal) // 2, B, np.arange(nreal))
        tau = PV.make_tau("mixed", t, rng)
        ds = pj.Dataset(t, np.zeros(N), s2, ctx)
        good, st = ds.predict_var(A, Bc, C, Dd, tau, nu=nu, return_status=True)
        assert pj._lib.lib().pioran_celerite_config_name(-1) == b"wide (step-by-step variance)"
        assert (st == 0).all(), (R, st)
        for bad in (0, B // 2, B - 1):
            Ab = A.copy(); Ab[bad] = -A[bad]
            v, st = ds.predict_var(Ab, Bc, C, Dd, tau, nu=nu, return_status=True)
            want = np.zeros(B, dtype=st.dtype); want[bad] = 2
            assert np.array_equal(st, want), (R, bad, st)
            assert np.isnan(v[bad]).all(), (R, bad)
            others = np.arange(B) != bad
            assert np.array_equal(v[others], good[others]), (R, bad)
        ds.close()
        keep = [0, B // 2, B - 1]
        PV.check(lambda *a: (good[keep], np.zeros(3, dtype=np.int32)), (f"R{R}-N{N}-B{B}-draws{keep}", t, s2, A[keep], Bc[keep], C, Dd, nu[keep], tau))
