"""GPU tests of the posterior predictive summaries (pioran_celerite_rand_posterior_summary through Dataset.rand_posterior_summary and
pj.ppc_timeseries_summary): the draws stay on the device and come back as quantiles and means over the draws.

Reference: Dataset.rand_posterior on the same normals — the same kernels, so the same bits — followed by the numpy twin of the reduction
(tools/quantiles_proto.py).  Series: prefixes N = 37 and N = 130 of tests/golden/simu.txt on the reference's default grid (pj.ppc_t_pred);
kernel: SHO with 4 (N = 37) or 3 (N = 130) components from pj.approx_batch on seeded bending-power-law parameters.

Bounds.  Without shift the quantiles of the series and of the residuals must be the twin's numbers, and a mean must lie within
K eps mean_b|v| of the long-double mean (any summation order).  With shift and backtransform the values are e_b = exp(draw_b + shift_b), formed
by ocml's exp on the device and numpy's in the twin: they differ by at most (3 + 1) eps e_b (assumed of the two libraries, not measured), order
statistics and their convex combinations are 1-Lipschitz in the sup norm, the interpolation adds 3 eps: 16 eps max_b|v| for a column of the
series, and the same 16 eps max_b|v| is asserted for a residual column.  (The Lipschitz argument alone does not give that for a residual
v = (y - e) / yerr, whose perturbation is that of e divided by yerr; the bound is held as set, and the tests print the deviation in that unit.)
The shifted means get 4 eps mean_b(e_b [/ yerr]) for the two exp on top of K eps mean_b|v|.  Every test prints what it measured."""
import importlib.util
from pathlib import Path

import numpy as np
import pytest

import pioran_jl_amd as pj

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
EPS = np.finfo(np.float64).eps
FIVE = (0.025, 0.16, 0.5, 0.84, 0.975)
NAME = "quantiles (sort over draws)"


def _proto():
    spec = importlib.util.spec_from_file_location("quantiles_proto", ROOT / "tools" / "quantiles_proto.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


P = _proto()
_CASES = {}


@pytest.fixture(scope="module")
def ctx():
    c = pj.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def simu(golden_dir):
    A = np.loadtxt(golden_dir / "simu.txt")
    return tuple(np.ascontiguousarray(A[:, k]) for k in range(3))


def _case(simu, N, B, shifted):
    """series, grid, coefficient sets and normals of a case; with `shifted` the series is raw flux (positive) and every sample has a shift below it"""
    key = (N, B, shifted)
    if key in _CASES:
        return _CASES[key]
    t, y, yerr = (a[:N].copy() for a in simu)
    J = 4 if N == 37 else 3
    rng = np.random.default_rng(100000 + 1000 * N + B + (7 if shifted else 0))
    f_min, f_max = 1.0 / (t[-1] - t[0]), 1.0 / (2.0 * np.min(np.diff(t)))
    theta = np.column_stack([rng.uniform(0.0, 1.25, B), np.exp(rng.uniform(np.log(f_min), np.log(f_max), B)), rng.uniform(2.0, 4.0, B)])
    shift = None
    if shifted:
        y = y - y.min() + 2.0
        shift = rng.uniform(0.0, 1.5, B)
        z = np.log(y[None, :] - shift[:, None])
        var, mu = np.var(z, axis=1) * np.exp(0.3 * rng.standard_normal(B)), np.mean(z, axis=1) + 0.1 * rng.standard_normal(B)
    else:
        var, mu = np.var(y) * np.exp(0.3 * rng.standard_normal(B)), np.mean(y) + 0.3 * np.std(y) * rng.standard_normal(B)
    A, Bc, C, Dd = pj.approx_batch(pj.SingleBendingPowerLaw, theta, f_min, f_max, J, norm=var)
    nu = rng.gamma(2.0, 0.5, B) + 0.2
    tau = pj.ppc_t_pred(t)
    M = len(tau)
    c = dict(t=t, y=y, yerr=yerr, tau=tau, A=A, Bc=Bc, C=C, Dd=Dd, mu=mu, nu=nu, shift=shift, q_data=rng.standard_normal((B, N)),
             q_new=rng.standard_normal((B, M)), eps=rng.standard_normal((B, N)), idx=np.searchsorted(tau, t).astype(np.int32))
    assert np.array_equal(tau[c["idx"]], t)
    _CASES[key] = c
    return c


def _same(a, b):
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])


def _expect(draws, st, shift, cols=None, ref=None, scale=None, probs=FIVE):
    """twin quantiles, long-double mean, and the bounds on both (zero for the quantiles without shift: equal as numbers)"""
    q, _, K = P.quantiles(draws, probs, status=st, shift=shift, cols=cols, ref=ref, scale=scale)
    V = P.load(draws, st, shift, cols, ref, scale)
    mean, absmean = P.mean_longdouble(draws, status=st, shift=shift, cols=cols, ref=ref, scale=scale)
    qb, mb = np.zeros(V.shape[1]), K * EPS * absmean
    if shift is not None and K:
        E = np.abs(P.load(draws, st, shift, cols)) / (1.0 if scale is None else np.abs(scale)[None, :])
        qb = 16.0 * EPS * np.max(np.abs(V), axis=0)
        mb = mb + 4.0 * EPS * np.mean(E, axis=0)
    return q, mean, qb, mb, K


def _hold(label, q, mean, want):
    wq, wmean, qb, mb, K = want
    if not np.any(qb):
        print(f"{label}: quantiles that differ from the twin: {int(np.sum(~((q == wq) | (np.isnan(q) & np.isnan(wq)))))} of {q.size}", end="; ")
        assert _same(q, wq)
    else:
        assert np.array_equal(np.isnan(q), np.isnan(wq))
        ratio = float(np.nanmax(np.abs(q - wq) / qb[None, :]))
        print(f"{label}: max |device - twin| = {16 * ratio:.2f} eps max_b|v| of the column (bound 16)", end="; ")
        assert ratio <= 1.0
    if mean is not None and K:
        fin = np.isfinite(wmean.astype(np.float64))
        mr = float(np.max(np.abs(mean[fin] - wmean[fin]) / mb[fin])) if fin.any() else 0.0
        print(f"|mean - long double| = {mr:.3f} x bound")
        assert np.array_equal(mean[~fin], wmean.astype(np.float64)[~fin], equal_nan=True) and mr <= 1.0
    else:
        print()


def _both(ctx, c, per_draw_cd=False, shift="case", probs=FIVE):
    """(draws, status) of Dataset.rand_posterior and the summary of the same call"""
    shift = c["shift"] if isinstance(shift, str) else shift
    C, Dd = c["C"], c["Dd"]
    if per_draw_cd:
        B = len(c["A"])
        scale = 1.0 + 0.01 * np.arange(B)[:, None]
        C, Dd = C[None, :] * scale, Dd[None, :] * scale
    ds = pj.Dataset(c["t"], c["y"], c["yerr"] ** 2, ctx)
    try:
        draws, st = ds.rand_posterior(c["A"], c["Bc"], C, Dd, c["tau"], c["q_data"], c["q_new"], c["eps"], mu=c["mu"], nu=c["nu"], shift=shift,
                                      return_status=True)
        r = ds.rand_posterior_summary(c["A"], c["Bc"], C, Dd, c["tau"], c["q_data"], c["q_new"], c["eps"], probs=probs, mu=c["mu"], nu=c["nu"],
                                      shift=shift, backtransform=shift is not None, res_cols=c["idx"], res_ref=c["y"], res_scale=c["yerr"])
        name = pj._lib.lib().pioran_celerite_config_name(-1).decode()
    finally:
        ds.close()
    assert name == NAME
    return draws, st, r, shift


def _hold_summary(label, c, draws, st, r, shift, probs=FIVE):
    B = len(st)
    assert np.array_equal(r["status"], st) and r["kept"] == B - int(np.sum(st == 2)) == int(np.sum(st == 0))
    assert np.all(np.isnan(draws[st != 0])) and np.all(np.isfinite(draws[st == 0]))
    _hold(f"{label}, series", r["ts_quantiles"], r["ts_mean"], _expect(draws, st, shift, probs=probs))
    _hold(f"{label}, residuals", r["res_quantiles"], r["res_mean"], _expect(draws, st, shift, c["idx"], c["y"], c["yerr"], probs=probs))


@pytest.mark.parametrize("shifted", [False, True])
@pytest.mark.parametrize("B", [5, 70, 300])
@pytest.mark.parametrize("N", [37, 130])
def test_summary_equals_draws_then_twin(ctx, simu, N, B, shifted):
    c = _case(simu, N, B, shifted)
    draws, st, r, shift = _both(ctx, c)
    M = len(c["tau"])
    assert r["ts_quantiles"].shape == (5, M) and r["res_quantiles"].shape == (5, N) and r["res_mean"].shape == (N,)
    print(f"N = {N}, M = {M}, B = {B}, shift {shifted}: {int(np.sum(st != 0))} draws with status 2")
    assert np.sum(st == 0) >= B // 2
    _hold_summary(f"(N, B) = ({N}, {B}){', shift' if shifted else ''}", c, draws, st, r, shift)


def test_a_draw_whose_shift_reaches_the_data_is_left_out(ctx, simu):
    c = dict(_case(simu, 37, 5, True))
    shift = c["shift"].copy()
    shift[1] = float(np.min(c["y"]))            # y - shift <= 0 at one time stamp: status 2
    draws, st, r, _ = _both(ctx, c, shift=shift)
    clean = _case(simu, 37, 5, True)
    _, st0, _, _ = _both(ctx, clean)
    assert st[1] == 2 and np.array_equal(np.delete(st, 1), np.delete(st0, 1))
    assert r["kept"] == int(np.sum(st0 == 0)) - (1 if st0[1] == 0 else 0)
    _hold_summary("one shift at min y", c, draws, st, r, shift)
    # ... and the summaries are those of the other draws alone
    others = np.delete(np.arange(5), 1)
    want = _expect(draws[others], st[others], shift[others])
    _hold("the other four draws", r["ts_quantiles"], r["ts_mean"], want)


@pytest.mark.parametrize("shifted", [False, True])
def test_cd_per_draw(ctx, simu, shifted):
    c = _case(simu, 37, 3, shifted)
    draws, st, r, shift = _both(ctx, c, per_draw_cd=True)
    _hold_summary(f"(c, d) per draw, B = 3{', shift' if shifted else ''}", c, draws, st, r, shift)


def test_chunked_call_and_trim_give_the_same_bits(simu):
    """N = 130, B = 300 under workspace_limit_mb = 1: the per-draw inputs and outputs of a chunk alone (3 P + 4 N + 3 M doubles, 22.8 KB at
    M = P = 388) put the 256-draw chunk at 5.8 MB, so the sizer halves to at most 32 draws a chunk, while the resident draws (300 x 388 doubles,
    0.93 MB) still fit.  A grid that makes them 4.8 MB is refused with the out-of-memory code before any draw is computed."""
    c = _case(simu, 130, 300, False)
    probs = [0.5, 0.0, 1.0, 0.975, 0.025]
    whole_ctx = pj.Context(0)
    try:
        _, _, whole, _ = _both(whole_ctx, c, probs=probs)
        whole_ctx.trim()
        _, _, again, _ = _both(whole_ctx, c, probs=probs)
    finally:
        whole_ctx.close()
    small = pj.Context(0)
    try:
        small.set_option("workspace_limit_mb", 1)
        draws, st, parts, shift = _both(small, c, probs=probs)
        _hold_summary("300 draws in chunks of at most 32", c, draws, st, parts, shift, probs=probs)
        big = dict(c)
        big["tau"] = np.linspace(c["t"][0], c["t"][-1], 2000)
        big["q_new"] = np.zeros((300, 2000))
        ds = pj.Dataset(c["t"], c["y"], c["yerr"] ** 2, small)
        try:
            with pytest.raises(pj._lib.PioranHipError, match="error -3"):
                ds.rand_posterior_summary(c["A"], c["Bc"], c["C"], c["Dd"], big["tau"], c["q_data"], big["q_new"], c["eps"], mu=c["mu"], nu=c["nu"])
        finally:
            ds.close()
    finally:
        small.close()
    keys = ("ts_quantiles", "ts_mean", "res_quantiles", "res_mean", "status")
    same = all(np.array_equal(parts[k], whole[k], equal_nan=True) for k in keys) and parts["kept"] == whole["kept"]
    same_trim = all(np.array_equal(again[k], whole[k], equal_nan=True) for k in keys) and again["kept"] == whole["kept"]
    print(f"chunked against unchunked bit-identical: {same}; after trim(): {same_trim}")
    assert same and same_trim


@pytest.mark.parametrize("shifted", [False, True])
def test_ppc_timeseries_summary_against_ppc_timeseries(ctx, simu, shifted):
    """pj.ppc_timeseries_summary against pj.ppc_timeseries with an equally seeded generator followed by the reference's recipe on the host
    (src/plots_diagnostics.jl:805-816): indices by equality, (y - ts[idx]) / yerr, quantiles of the rows, mean"""
    c = _case(simu, 37, 70, shifted)
    args = (c["t"], c["y"], c["yerr"], c["A"], c["Bc"], c["C"], c["Dd"])
    kw = dict(mu=c["mu"], nu=c["nu"], shift=c["shift"], ctx=ctx)
    s = pj.ppc_timeseries_summary(np.random.default_rng(31), *args, **kw)
    ts, t_pred = pj.ppc_timeseries(np.random.default_rng(31), *args, **kw)
    N, B = len(c["t"]), len(c["A"])
    assert np.array_equal(s["t_pred"], t_pred) and s["ts_quantiles"].shape == (5, len(t_pred)) and s["res_quantiles"].shape == (5, N)
    st = np.where(np.isnan(ts).any(axis=0), 2, 0).astype(np.int32)          # ppc_timeseries marks a failed sample by a NaN column
    assert np.array_equal(s["status"], st) and s["kept"] == int(np.sum(st == 0))
    indexes = np.array([int(np.flatnonzero(t_pred == ti)[0]) for ti in c["t"]])
    res = (c["y"][:, None] - ts[indexes, :]) / c["yerr"][:, None]
    ok = st == 0
    K = int(ok.sum())
    for label, got, arr in (("series", s["ts_quantiles"], ts), ("residuals", s["res_quantiles"], res)):
        want = P.quantiles(arr.T, FIVE, status=st)[0]
        if not shifted:
            print(f"ppc summary, {label}: quantiles that differ: {int(np.sum(got != want))} of {got.size}")
            assert np.array_equal(got, want)
        else:
            bound = 16.0 * EPS * np.max(np.abs(arr[:, ok]), axis=1)
            ratio = float(np.max(np.abs(got - want) / bound[None, :]))
            print(f"ppc summary with shift, {label}: max |device - host recipe| = {16 * ratio:.2f} eps max_b|v| of the column (bound 16)")
            assert ratio <= 1.0
    mean_res = np.sum(res[:, ok].astype(np.longdouble), axis=1) / K
    mb = K * EPS * np.mean(np.abs(res[:, ok]), axis=1) + (4.0 * EPS * np.mean(np.abs(ts[indexes][:, ok]), axis=1) / c["yerr"] if shifted else 0.0)
    mr = float(np.max(np.abs(s["mean_res"] - mean_res) / mb))
    print(f"ppc summary{' with shift' if shifted else ''}: |mean_res - long double| = {mr:.3f} x bound")
    assert mr <= 1.0
