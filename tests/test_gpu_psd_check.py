"""GPU tests of the PSD check (psd_check.hip through pioran_psd_check_batch[_dev] and pioran_psd_check_summary, and the Python layer above them)
against the 50-digit truth tests/golden/psd_check_truth.npz and the numpy twins (tools/psd_check_proto.py, tools/quantiles_proto.py).
Cases, deviation scales and the bar — max(20 x the fp64 twin's own deviation from the truth on that case and array, 256 eps) — are
tests/psd_check_cases.py's.  Every test prints what it measured; profiles/psd_check_gpu_test_deviations.txt keeps one run's output."""
import numpy as np
import pytest

import pioran_jl_amd as pj
import psd_check_cases as PC

pytestmark = pytest.mark.gpu
P = PC.PROTO
NAME = "psd check (model against approximation)"
MODELS = (pj.SingleBendingPowerLaw, pj.DoubleBendingPowerLaw)
PROBS = [0.025, 0.16, 0.5, 0.84, 0.975, 0.0, 1.0]


@pytest.fixture(scope="module")
def ctx():
    c = pj.Context(0)
    yield c
    c.close()


def _config_name():
    return pj._lib.lib().pioran_celerite_config_name(-1).decode()


def _same(a, b):
    """equal as numbers, NaN exactly where the other has NaN"""
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def _call(ctx, case, theta=None, norm=None, freq=None, summary=False, **kw):
    m, b, J, B, F, i, n, tf = case
    th, nm = PC.draws(case)
    fn = ctx.psd_check_summary if summary else ctx.psd_check
    return fn(MODELS[m], th if theta is None else theta, nm if norm is None else norm, PC.freqs(case) if freq is None else freq, PC.F_MIN, PC.F_MAX,
              J, PC.S_LOW, PC.S_HIGH, basis_function=PC.BASIS_NAME[b], is_integrated_power=bool(i), normalise=bool(n), times_f=bool(tf), **kw)


def _big_case():
    """257 draws x 1000 frequencies (16 frequency tiles, 9 draw tiles, the last with one draw), J = 20, normalised: no truth, only identities"""
    case = (1, 0, 20, 257, 1000, 1, 1, 0)
    th, nm = PC.draws(case)
    f = 10.0 ** np.linspace(np.log10(PC.F_MIN / PC.S_LOW), np.log10(PC.F_MAX * PC.S_HIGH), 1000)
    return case, th, nm, f


@pytest.mark.parametrize("case", PC.cases(), ids=PC.name)
def test_arrays_against_the_truth(ctx, case):
    r = _call(ctx, case, amplitudes=True, integ=True)
    assert _config_name() == NAME
    assert (r["status"] == 0).all()
    dev, bars, tdev = PC.deviations(r, PC.truth(case)), PC.bars(case), PC.twin_dev(case)
    print(PC.name(case) + ": " + "; ".join(f"{k} {dev[k]:.2e} (twin {tdev[k]:.2e}, bar {bars[k]:.2e})" for k in dev))
    for k in dev:
        assert dev[k] <= bars[k], (k, dev[k], bars[k])


def test_null_outputs_in_every_combination(ctx):
    """What is returned does not change by a bit with what else is requested."""
    case = PC.cases()[1]                       # 65 x 65: three draw tiles, two frequency tiles, normalised
    full = _call(ctx, case, amplitudes=True, integ=True)
    for mask in range(16):
        outs = tuple(n for k, n in enumerate(PC.ARRAYS) if mask >> k & 1)
        for extra in ({}, dict(amplitudes=True), dict(integ=True)) if mask else (dict(amplitudes=True), dict(integ=True), {}):
            r = _call(ctx, case, outputs=outs, **extra)
            assert set(r) == set(outs) | set(extra) | {"status"}
            for k in r:
                assert _same(r[k], full[k]), (outs, extra, k)


def test_chunked_equals_unchunked(ctx):
    case, th, nm, f = _big_case()
    whole = _call(ctx, case, th, nm, f, amplitudes=True, integ=True)
    ctx.trim()                                 # (buffers the context already holds do not count against the limit)
    ctx.set_option("workspace_limit_mb", 1)    # 257 draws x 4 arrays x 8 kB: chunks of 32 draws
    try:
        parts = _call(ctx, case, th, nm, f, amplitudes=True, integ=True)
        two = _call(ctx, case, th, nm, f, outputs=("residuals", "psd"))
    finally:
        ctx.set_option("workspace_limit_mb", None)
        ctx.trim()
    for k in whole:
        assert _same(parts[k], whole[k]), k
    assert _same(two["residuals"], whole["residuals"]) and _same(two["psd"], whole["psd"])


def _bad_draws(case, th, nm, f):
    """draws 1, 40 and 64 replaced by a NaN in theta, an infinite norm and a model that underflows to 0 at freq[0]"""
    th, nm = th.copy(), nm.copy()
    th[1, 2] = np.nan
    nm[40] = np.inf
    th[64, 0], th[64, 1] = 400.0, 1e-6
    f = f.copy()
    f[0] = 10.0
    return th, nm, f, [1, 40, 64]


def test_status_two_and_its_neighbours(ctx):
    case = PC.cases()[1]
    th, nm = PC.draws(case)
    thb, nmb, f, bad = _bad_draws(case, th, nm, PC.freqs(case))
    good = np.setdiff1d(np.arange(len(th)), bad)
    clean = _call(ctx, case, th, nm, f, amplitudes=True, integ=True)
    r = _call(ctx, case, thb, nmb, f, amplitudes=True, integ=True)
    tw = P.psd_check(case[0], thb, nmb, f, PC.F_MIN, PC.F_MAX, PC.S_LOW, PC.S_HIGH, case[2], case[1], integrated=case[5], normalise=case[6], times_f=case[7])
    assert np.array_equal(r["status"], tw["status"]) and r["status"][bad].tolist() == [2, 2, 2] and (r["status"][good] == 0).all()
    for k in PC.ARRAYS + ("amplitudes", "integ"):
        assert np.isnan(r[k][bad]).all(), k
        assert _same(r[k][good], clean[k][good]), k      # the neighbours: the bits of a call without the bad draws' values
    s = _call(ctx, case, thb, nmb, f, summary=True, probs=PROBS)
    assert s["kept"] == len(good) and np.array_equal(s["status"], r["status"])
    assert np.isnan(s["meta"][bad]).all() and np.isfinite(s["meta"][good]).all()
    for a, k in enumerate(PC.ARRAYS):                      # the bad draws are left out of the per-frequency reductions
        q, mean, kept = pj.quantiles(r[k][good], PROBS, ctx=ctx)
        assert kept == len(good) and _same(s["quant"][a], q)
    # all draws bad: NaN everywhere, kept 0
    allbad = _call(ctx, case, np.full_like(th, np.nan), nm, f, summary=True, probs=PROBS)
    assert allbad["kept"] == 0 and np.isnan(allbad["quant"]).all() and np.isnan(allbad["meta"]).all() and (allbad["status"] == 2).all()


def _check_summary(ctx, case, th, nm, f, label):
    r = _call(ctx, case, th, nm, f)
    s = _call(ctx, case, th, nm, f, summary=True, probs=PROBS)
    assert _config_name() == NAME
    B, F = len(th), len(f)
    assert s["quant"].shape == (4, len(PROBS), F) and s["mean"].shape == (4, F) and s["meta"].shape == (B, 8) and s["kept"] == B
    for a, k in enumerate(PC.ARRAYS):
        q, mean, kept = pj.quantiles(r[k], PROBS, status=r["status"], ctx=ctx)
        assert _same(s["quant"][a], q) and _same(s["mean"][a], mean), k
    for j, k in enumerate(("residuals", "ratios")):
        med, mean, _ = pj.quantiles(np.ascontiguousarray(r[k].T), [0.5], ctx=ctx)
        assert _same(s["meta"][:, 4 * j], mean) and _same(s["meta"][:, 4 * j + 1], med[0]), k
        assert _same(s["meta"][:, 4 * j + 2], np.min(np.abs(r[k]), axis=1)) and _same(s["meta"][:, 4 * j + 3], np.max(np.abs(r[k]), axis=1)), k
    # the twin's reductions of the same arrays: quantiles to the bit, means within K eps mean|v| of the long-double mean
    tq, tmean, tmeta, tkept = P.summary(r, r["status"], PROBS)
    assert tkept == s["kept"] and _same(s["quant"], tq) and _same(s["meta"][:, [1, 2, 3, 5, 6, 7]], tmeta[:, [1, 2, 3, 5, 6, 7]])
    eps = np.finfo(float).eps
    for a, k in enumerate(PC.ARRAYS):
        assert np.all(np.abs(s["mean"][a] - tmean[a]) <= B * eps * np.mean(np.abs(r[k]), axis=0)), k
    for j, k in enumerate(("residuals", "ratios")):
        assert np.all(np.abs(s["meta"][:, 4 * j] - tmeta[:, 4 * j]) <= F * eps * np.mean(np.abs(r[k]), axis=1)), k
    print(f"summary {label}: quant, mean and meta are pj.quantiles' bits on the array form's output; min / max are numpy's")
    # without mean and meta
    s2 = _call(ctx, case, th, nm, f, summary=True, probs=PROBS, mean=False, meta=False)
    assert set(s2) == {"quant", "status", "kept"} and _same(s2["quant"], s["quant"])


def test_summary_equals_the_reductions_of_the_arrays(ctx):
    case = PC.cases()[1]
    th, nm = PC.draws(case)
    _check_summary(ctx, case, th, nm, PC.freqs(case), "65 x 65")
    case, th, nm, f = _big_case()
    _check_summary(ctx, case, th, nm, f, "257 x 1000")
    case = PC.cases()[0]
    th, nm = PC.draws(case)
    _check_summary(ctx, case, th[:1], nm[:1], PC.freqs(case)[:1], "1 x 1")


@pytest.mark.parametrize("B,F", [(4096, 8), (8, 4096)])
def test_summary_at_the_limit(ctx, B, F):
    case = (0, 0, 20, B, F, 1, 0, 0)
    th, nm = PC.draws(case)
    _check_summary(ctx, case, th, nm, PC.freqs(case), f"{B} x {F}")


def test_summary_beyond_the_limit_is_unsupported(ctx):
    for B, F in ((4097, 8), (8, 4097)):
        case = (0, 0, 20, B, F, 1, 0, 0)
        th, nm = PC.draws(case)
        with pytest.raises(pj._lib.PioranHipError, match="error -4"):
            _call(ctx, case, th, nm, PC.freqs(case), summary=True)
        r = _call(ctx, case, th, nm, PC.freqs(case), outputs=("ratios",))       # the array form has no such limit
        assert r["ratios"].shape == (B, F) and np.isfinite(r["ratios"]).all()


def test_device_pointer_form_equals_host_form(ctx):
    import torch
    case = PC.cases()[6]                       # 65 x 63, DRWCelerite, normalised
    m, b, J, B, F, i, n, tf = case
    th, nm = PC.draws(case)
    f = PC.freqs(case)
    host = _call(ctx, case, amplitudes=True, integ=True)
    dev = torch.device("cuda:0")
    dth, dnm, df = (torch.from_numpy(a).to(dev) for a in (th, nm, f))
    out = {k: torch.full((B, F), -1.0, dtype=torch.float64, device=dev) for k in PC.ARRAYS}
    damp = torch.full((B, J), -1.0, dtype=torch.float64, device=dev)
    dint = torch.full((B,), -1.0, dtype=torch.float64, device=dev)
    dst = torch.full((B,), -1, dtype=torch.int32, device=dev)
    kw = dict(basis_function=PC.BASIS_NAME[b], is_integrated_power=bool(i), normalise=bool(n), times_f=bool(tf))
    torch.cuda.synchronize()
    ctx.psd_check_dev(B, F, MODELS[m], dth.data_ptr(), dnm.data_ptr(), df.data_ptr(), PC.F_MIN, PC.F_MAX, J, PC.S_LOW, PC.S_HIGH,
                      dpsd=out["psd"].data_ptr(), dpsd_approx=out["psd_approx"].data_ptr(), dresiduals=out["residuals"].data_ptr(),
                      dratios=out["ratios"].data_ptr(), damplitudes=damp.data_ptr(), dinteg=dint.data_ptr(), dstatus=dst.data_ptr(), **kw)
    ctx.synchronize()
    for k in PC.ARRAYS:
        assert _same(out[k].cpu().numpy(), host[k]), k
    assert _same(damp.cpu().numpy(), host["amplitudes"]) and _same(dint.cpu().numpy(), host["integ"]) and np.array_equal(dst.cpu().numpy(), host["status"])
    # one output only, a second call on the same grid
    only = torch.full((B, F), -1.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    ctx.psd_check_dev(B, F, MODELS[m], dth.data_ptr(), dnm.data_ptr(), df.data_ptr(), PC.F_MIN, PC.F_MAX, J, PC.S_LOW, PC.S_HIGH, dratios=only.data_ptr(), **kw)
    ctx.synchronize()
    assert _same(only.cpu().numpy(), host["ratios"])


# ---- the Python layer ---------------------------------------------------------------------------------------------------------------------
def _prior(n, seed):
    """the prior of the reference's modelling guide (docs/src/modelling.md:90-101): alpha1 ~ U(0, 1.25), f1 ~ LogU(1e-3, 1e3), alpha2 ~ U(alpha1, 4),
    norm ~ LogNormal(-1, 2); samples (3, n) as the reference passes them"""
    rng = np.random.default_rng(seed)
    a1 = rng.uniform(0.0, 1.25, n)
    f1 = 10.0 ** rng.uniform(-3, 3, n)
    a2 = a1 + (4.0 - a1) * rng.uniform(size=n)
    return np.vstack([a1, f1, a2]), np.exp(-1.0 + 2.0 * rng.standard_normal(n))


F_MIN_DOC, F_MAX_DOC = 5e-3, 200.0      # docs/src/modelling.md:118


def test_sample_approx_model_layout_and_grid(ctx):
    samples, norm = _prior(7, 1)
    f0, fM = F_MIN_DOC / 20, F_MAX_DOC * 20
    psd, approx, res, rat, f = pj.sample_approx_model(samples, norm, f0, fM, pj.SingleBendingPowerLaw, n_frequencies=50, n_components=20, ctx=ctx)
    assert np.array_equal(f, 10.0 ** np.linspace(np.log10(f0), np.log10(fM), 50))
    for a in (psd, approx, res, rat):
        assert a.shape == (50, 7) and a.base is not None and a.T.flags["C_CONTIGUOUS"]      # (F, B) views of the (B, F) device layout
    tw = P.psd_check(0, samples.T, norm, f, f0, fM, 1.0, 1.0, 20, 0)
    assert np.max(np.abs(psd.T - tw["psd"]) / tw["psd"]) < 1e-13 and np.max(np.abs(approx.T - tw["psd_approx"]) / np.abs(tw["psd_approx"])) < 1e-9
    assert np.array_equal(psd[0], norm)                                                     # normalised at the first frequency, times norm
    assert np.array_equal(res, psd - approx) and np.array_equal(rat, approx / psd)


def _diagnostics_of_arrays(arr, status):
    q, mean, meta, kept = P.summary(arr, status, pj.gp.PPC_QUANTILES)
    return q, mean, meta, kept


@pytest.mark.parametrize("n", [300, 4100])
def test_run_diagnostics_equals_the_twins_reductions(ctx, n):
    """300 draws: the device summary; 4100 draws: the array form chunk by chunk and the host reduction"""
    samples, norm = _prior(n, 7)
    d = pj.run_diagnostics(samples, norm, F_MIN_DOC, F_MAX_DOC, pj.SingleBendingPowerLaw, n_frequencies=200 if n > 4096 else 1000, ctx=ctx)
    f0, fM = F_MIN_DOC / 20.0, F_MAX_DOC * 20.0
    assert np.array_equal(d["f"], 10.0 ** np.linspace(np.log10(f0), np.log10(fM), len(d["f"])))
    arr = ctx.psd_check(pj.SingleBendingPowerLaw, samples.T, norm, d["f"], f0, fM, 20, 1.0, 1.0)
    q, mean, meta, kept = P.summary(arr, arr["status"], pj.gp.PPC_QUANTILES)
    assert d["kept"] == kept == n
    assert _same(d["res_quantiles"], q[2]) and _same(d["rat_quantiles"], q[3])
    names = pj.gp._META_NAMES
    for k in (1, 2, 3, 5, 6, 7):
        assert _same(d[names[k]], meta[:, k]), names[k]
    eps = np.finfo(float).eps
    assert np.all(np.abs(d["mean_res"] - mean[2]) <= n * eps * np.mean(np.abs(arr["residuals"]), axis=0))
    assert np.all(np.abs(d["mean_rat"] - mean[3]) <= n * eps * np.mean(np.abs(arr["ratios"]), axis=0))
    for j, k in ((0, "residuals"), (4, "ratios")):
        assert np.all(np.abs(d[names[j]] - meta[:, j]) <= len(d["f"]) * eps * np.mean(np.abs(arr[k]), axis=1))
    print(f"run_diagnostics, {n} draws: median ratio at the ends of the observed window "
          f"{d['rat_quantiles'][2][np.searchsorted(d['f'], F_MIN_DOC)]:.4f}, {d['rat_quantiles'][2][np.searchsorted(d['f'], F_MAX_DOC) - 1]:.4f}")


def _series(N, seed):
    rng = np.random.default_rng(seed)
    t = np.cumsum(rng.uniform(0.5, 1.5, N))
    return t, 2.0 + 0.3 * rng.standard_normal(N), rng.uniform(0.02, 0.06, N)


def test_psd_ppc_noise_levels_and_quantiles(ctx):
    t, y, yerr = _series(50, 3)
    samples, norm = _prior(12, 4)
    nu = np.random.default_rng(5).uniform(0.5, 1.5, 12)
    for log_tr, fP in ((False, False), (True, True)):
        r = pj.psd_ppc(samples.T, norm, nu, t, y, yerr, pj.SingleBendingPowerLaw, n_frequencies=40, plot_f_P=fP, with_log_transform=log_tr, ctx=ctx)
        dt = np.diff(t)
        sq = (yerr / y) ** 2 if log_tr else yerr ** 2
        assert r["mean_noise_level"] == 2 * np.mean(nu) * np.mean(sq) * np.mean(dt)
        assert r["median_noise_level"] == 2 * np.median(nu) * np.median(sq) * np.median(dt)
        assert r["f_min"] == 1 / (t[-1] - t[0]) and r["f_max"] == 1 / np.min(dt) / 2 and r["kept"] == 12
        arr = ctx.psd_check(pj.SingleBendingPowerLaw, samples.T, norm, r["f"], r["f_min"], r["f_max"], 20, 20.0, 20.0, normalise=True, times_f=fP)
        q, _, _, _ = P.summary(arr, arr["status"], pj.gp.PPC_QUANTILES)
        assert _same(r["psd_quantiles"], q[0]) and _same(r["psd_approx_quantiles"], q[1])


def test_psd_ppc_beyond_4096_samples_reduces_on_the_host(ctx):
    t, y, yerr = _series(50, 3)
    samples, norm = _prior(4100, 6)
    r = pj.psd_ppc(samples.T, norm, np.ones(4100), t, y, yerr, pj.SingleBendingPowerLaw, n_frequencies=12, basis_function="DRWCelerite",
                   is_integrated_power=False, ctx=ctx)
    arr = ctx.psd_check(pj.SingleBendingPowerLaw, samples.T, norm, r["f"], r["f_min"], r["f_max"], 20, 20.0, 20.0, basis_function="DRWCelerite",
                        is_integrated_power=False, normalise=True)
    q, _, _, kept = P.summary(arr, arr["status"], pj.gp.PPC_QUANTILES)
    assert r["kept"] == kept == 4100 and _same(r["psd_quantiles"], q[0]) and _same(r["psd_approx_quantiles"], q[1])


def test_posterior_predict_checks_is_the_three_calls(ctx):
    N, B = 50, 8
    t, y, yerr = _series(N, 11)
    samples, norm = _prior(B, 12)
    rng0 = np.random.default_rng(13)
    nu, mu = rng0.uniform(0.8, 1.2, B), 2.0 + 0.01 * rng0.standard_normal(B)
    model = pj.SingleBendingPowerLaw
    kw = dict(n_frequencies=16, n_components=20)
    both = pj.posterior_predict_checks(np.random.default_rng(99), samples.T, norm, nu, mu, None, t, y, yerr, model, ctx=ctx, **kw)
    assert set(both) == {"psd", "lsp", "timeseries"}
    one = pj.psd_ppc(samples.T, norm, nu, t, y, yerr, model, ctx=ctx, **kw)
    for k in one:
        assert np.array_equal(np.asarray(both["psd"][k]), np.asarray(one[k]), equal_nan=True), k
    f_min, f_max = 1 / (t[-1] - t[0]), 1 / np.min(np.diff(t)) / 2
    A, Bc, C, Dd = pj.approx_batch(model, samples.T, f_min, f_max, 20, norm, 20.0, 20.0)
    rng = np.random.default_rng(99)
    lsp = pj.lsp_ppc(rng, t, yerr, A, Bc, C, Dd, mu=mu, nu=nu, n_frequencies=16, ctx=ctx)
    ts = pj.ppc_timeseries_summary(rng, t, y, yerr, A, Bc, C, Dd, mu=mu, nu=nu, ctx=ctx)
    for got, want in zip(both["lsp"], lsp):
        assert np.array_equal(got, want, equal_nan=True)
    for k in ts:
        assert np.array_equal(np.asarray(both["timeseries"][k]), np.asarray(ts[k]), equal_nan=True), k
    only = pj.posterior_predict_checks(np.random.default_rng(99), samples.T, norm, nu, mu, None, t, y, yerr, model, plots=["psd"], ctx=ctx, **kw)
    assert set(only) == {"psd"} and np.array_equal(only["psd"]["psd_quantiles"], one["psd_quantiles"])
    ts_only = pj.posterior_predict_checks(np.random.default_rng(99), samples.T, norm, nu, mu, None, t, y, yerr, model, plots=["timeseries"], ctx=ctx, **kw)
    assert set(ts_only) == {"timeseries"}
