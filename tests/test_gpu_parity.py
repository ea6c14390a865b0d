"""GPU parity tests (-m gpu): the HIP path, called through the C ABI, against
  (1) log-likelihood values the REFERENCE itself produced (tests/golden/ultranest_points.npz),
  (2) the pinned CPU oracle (oracle/) on the reference's literal test inputs and on seeded inputs,
  (3) size-independent properties at BASELINE.json's full size (N = 1e4, J = 20).
Tolerances are relative errors on log L, written next to each assert; north-star bar is 1e-8.
"""
import ctypes
import json
import os

import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import pioran_jl_amd as pj  # noqa: E402
from oracle import oracle as O  # noqa: E402


@pytest.fixture(scope="module")
def ctx():
    return pj.Context(0)


def relerr(got, ref):
    got = np.asarray(got, float); ref = np.asarray(ref, float)
    return np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300))


# ---------------------------------------------------------------------------------------------
def test_reference_outputs_ultranest(ctx, golden_dir):
    """5791 draws, N=242, SHO-20 (J=20): per-draw series (sampled shift c), mu, nu — vs Julia's values."""
    un = np.load(golden_dir / "ultranest_points.npz")
    t, y, yerr, P, ref = un["t"], un["y"], un["yerr"], un["params"], un["logl"]
    f_min, f_max = 1 / (t[-1] - t[0]), 1 / np.min(np.diff(t)) / 2
    A, Bc, C, Dd = pj.approx_batch(pj.SingleBendingPowerLaw, P[:, :3], f_min, f_max, 20, P[:, 3],
                                   is_integrated_power=False)
    cs = P[:, 6:7]
    Y = np.log(y[None, :] - cs)
    S2 = yerr[None, :] ** 2 / (y[None, :] - cs) ** 2
    ds = pj.Dataset(t, y, yerr ** 2, ctx)
    got, st = ds.logl_batch(A, Bc, C, Dd, mu=P[:, 5], nu=P[:, 4], Y=Y, S2=S2, return_status=True)
    assert (st == 0).all()
    assert relerr(got, ref) < 1e-10


def test_reference_outputs_ultranest_device_transform(ctx, golden_dir):
    """Same 5791 reference values, but the data set holds the RAW flux and yerr**2 and the per-draw transform
    log(y - c_b), yerr**2 / (y - c_b)**2 runs on the device (pioran_celerite_logl_batch_shift): the reference's
    production model end to end (docs/src/ultranest.md:197-219), only theta-derived arrays cross the boundary."""
    un = np.load(golden_dir / "ultranest_points.npz")
    t, y, yerr, P, ref = un["t"], un["y"], un["yerr"], un["params"], un["logl"]
    f_min, f_max = 1 / (t[-1] - t[0]), 1 / np.min(np.diff(t)) / 2
    A, Bc, C, Dd = pj.approx_batch(pj.SingleBendingPowerLaw, P[:, :3], f_min, f_max, 20, P[:, 3],
                                   is_integrated_power=False)
    ds = pj.Dataset(t, y, yerr ** 2, ctx)
    got, st = ds.logl_batch(A, Bc, C, Dd, mu=P[:, 5], nu=P[:, 4], shift=P[:, 6], return_status=True)
    assert (st == 0).all()
    assert relerr(got, ref) < 1e-10
    # a shift above min(y) makes log(y - c) undefined: status 2 / NaN where the reference throws DomainError
    bad, st = ds.logl_batch(A[:2], Bc[:2], C, Dd, mu=P[:2, 5], nu=P[:2, 4], shift=[y.min() + 1.0, P[1, 6]],
                            return_status=True)
    assert st[0] == 2 and np.isnan(bad[0]) and st[1] == 0 and abs(bad[1] - ref[1]) <= 1e-10 * abs(ref[1])


def test_reference_outputs_turing_chain(ctx, golden_dir):
    """8183 log-likelihoods out of the reference's stored NUTS chains (docs/src/data/subset_simu_single.h5: `log_density` minus
    the closed-form prior and Jacobian, tests/golden/turing_chain.npz) — the high-likelihood region — through three entries:
    coefficients + caller-side transform, coefficients + device-side shift transform, and theta only."""
    tc = np.load(golden_dir / "turing_chain.npz")
    t, y, yerr, P, ref = tc["t"], tc["y"], tc["yerr"], tc["params"], tc["logl"]
    f_min, f_max = 1 / (t[-1] - t[0]), 1 / np.min(np.diff(t)) / 2
    A, Bc, C, Dd = pj.approx_batch(pj.SingleBendingPowerLaw, P[:, :3], f_min, f_max, 20, P[:, 3], is_integrated_power=False)
    ds = pj.Dataset(t, y, yerr ** 2, ctx)
    cs = P[:, 6:7]
    bar = lambda got: np.max(np.abs(got - ref) / np.maximum(1.0, np.abs(ref)))   # noqa: E731
    got1, st = ds.logl_batch(A, Bc, C, Dd, mu=P[:, 5], nu=P[:, 4], Y=np.log(y[None, :] - cs), S2=yerr[None, :] ** 2 / (y[None, :] - cs) ** 2,
                             return_status=True)
    assert (st == 0).all() and bar(got1) < 1e-10
    got2, st = ds.logl_batch(A, Bc, C, Dd, mu=P[:, 5], nu=P[:, 4], shift=P[:, 6], return_status=True)
    assert (st == 0).all() and bar(got2) < 1e-10
    got3, st = ds.logpdf_theta(pj.SingleBendingPowerLaw, P[:, :3], P[:, 3], f_min, f_max, 20, is_integrated_power=False,
                               mu=P[:, 5], nu=P[:, 4], shift=P[:, 6], return_status=True)
    assert (st == 0).all() and bar(got3) < 1e-10
    # a sampler-sized batch of the same draws takes the windowed kernel: same bar
    got4 = ds.logl_batch(A[:200], Bc[:200], C, Dd, mu=P[:200, 5], nu=P[:200, 4], shift=P[:200, 6])
    assert np.max(np.abs(got4 - ref[:200]) / np.maximum(1.0, np.abs(ref[:200]))) < 1e-10


def test_reference_literal_cases(ctx, golden_dir):
    lit = json.loads((golden_dir / "reference_literals.json").read_text())
    rel = {c["name"]: c for c in json.loads((golden_dir / "relation_cases.json").read_text())["cases"]}
    g = lit["scalablegp_n6"]
    t = np.array(g["t"]); y = np.array(g["y"]); yerr = np.array(g["yerr"])
    for i in range(10):  # test/test_scalablegp.jl:109-132 through the reference-shaped API
        P = pj.SingleBendingPowerLaw(g["alpha1"][i], g["f1"][i], g["alpha2"][i])
        R = pj.approx(P, g["f_min"], g["f_max"], g["n_components"], g["variance"][i], basis_function="SHO")
        f = pj.ScalableGP(g["mu"][i], R)
        val = pj.logpdf(f(t, yerr ** 2), y, ctx=ctx)
        assert np.isfinite(val)
        assert abs(val - rel[f"scalablegp_n6[{i}]"]["logl_mpmath50"]) <= 1e-10 * abs(val)
    A = np.loadtxt(golden_dir / "simu_log.txt")
    t, y, yerr = A[:, 0], A[:, 1], A[:, 2]
    f0 = 1 / (t[-1] - t[0]) / 100
    fM = 1 / np.min(np.diff(t)) / 2 * 20
    for basis in ("SHO", "DRWCelerite"):  # test/test_likelihood.jl:7-59 (J=20 -> R=40; J=40 -> 60 active rows)
        R = pj.approx(pj.SingleBendingPowerLaw(0.82, 0.01, 3.3), f0, fM, 20, np.var(y, ddof=1), basis_function=basis)
        v1 = pj.log_likelihood(R, t, y - 0.0, yerr ** 2, ctx=ctx)
        v2 = pj.logpdf(pj.ScalableGP(0.0, R)(t, yerr ** 2), y, ctx=ctx)
        assert v1 == v2
        assert abs(v1 - rel[f"simu_log[{basis}]"]["logl_celerite"]) <= 1e-10 * abs(v1)
    with pytest.raises(ValueError, match="not recognised"):
        pj.log_likelihood(R, t, y, yerr ** 2, solver="foo", ctx=ctx)


def _random_case(rng, N, J, B, per_draw_cd=False):
    t = np.cumsum(rng.uniform(0.05, 2.0, N))
    y = rng.standard_normal(N)
    s2 = rng.uniform(0.01, 0.1, N)
    A = rng.uniform(0.1, 2.0, (B, J))
    Bc = rng.uniform(-0.05, 0.05, (B, J)) * A
    shape = (B, J) if per_draw_cd else (J,)
    C = rng.uniform(0.05, 2.0, shape)
    Dd = rng.uniform(0.0, 3.0, shape)
    mu = rng.standard_normal(B) * 0.1
    nu = rng.uniform(0.5, 2.0, B)
    return t, y, s2, A, Bc, C, Dd, mu, nu


@pytest.fixture(params=["throughput", "throughput_steps", "throughput_pairs", "throughput_triples", "latency", "latency_lean", "block", "tile"])
def layout(request, ctx):
    """Small batches (B <= 512) with 6 <= R <= 63 rows take the windowed kernel (celerite_block.hip) by default; "no_block" sends
    them to the one-draw-per-workgroup latency layout (celerite_wide.hip), "no_wide" as well to the throughput layouts (the ones
    large batches use).  The throughput layouts run the two-step form up to four rows per lane (R <= 63) and the step-by-step recurrence
    above ("no_win2" / "win2" force either everywhere).  All are checked on the same inputs."""
    if request.param == "tile":             # celerite_tile.hip (windowed form, one draw per wavefront; default for large batches from 49 rows
        ctx.set_option("scan_config", "tile")   # on) forced for every launch it can take, whatever the batch size
    elif request.param != "block":
        ctx.set_option("no_block", True)
    if request.param.startswith("throughput"):
        ctx.set_option("no_wide", True)
    if request.param == "latency_lean":     # celerite_wide2_kernel (default from 64 rows on) forced for every row count
        ctx.set_option("wide2", True)
        ctx.set_option("scan_config", "wide")   # ... and for every batch size
    if request.param == "throughput_steps":
        ctx.set_option("no_win2", True)
    if request.param == "throughput_pairs":
        ctx.set_option("win2", True)
    if request.param == "throughput_triples":   # the three-step form wherever it exists (two / three rows per lane, shared table)
        ctx.set_option("win3", True)
    yield request.param
    for k in ("no_wide", "no_block", "no_win2", "win2", "win3", "wide2"):
        ctx.set_option(k, False)
    ctx.set_option("scan_config", None)


@pytest.mark.parametrize("J", [1, 2, 3, 5, 8, 10, 13, 16, 20, 21, 24, 27, 32, 40])
def test_random_batches_shared_cd(ctx, J, layout):
    """Every register-resident kernel configuration (R = 2J = 2..80) + ragged batch sizes."""
    rng = np.random.default_rng(100 + J)
    N, B = 257, 37
    t, y, s2, A, Bc, C, Dd, mu, nu = _random_case(rng, N, J, B)
    ds = pj.Dataset(t, y, s2, ctx)
    got, st = ds.logl_batch(A, Bc, C, Dd, mu=mu, nu=nu, return_status=True)
    ref = O.logl_batch(A, Bc, C, Dd, t, y, s2, mu, nu, nthreads=8)
    assert relerr(got, ref) < 1e-11, pj._lib.lib().pioran_celerite_config_name(2 * J)
    assert (st == 0).all()
    if layout == "tile":
        assert pj._lib.lib().pioran_celerite_config_name(-1).decode() == "tile"


@pytest.mark.parametrize("J", [2, 7, 20, 30])
def test_random_batches_per_draw_cd(ctx, J, layout):
    rng = np.random.default_rng(200 + J)
    N, B = 130, 19
    t, y, s2, A, Bc, C, Dd, mu, nu = _random_case(rng, N, J, B, per_draw_cd=True)
    ds = pj.Dataset(t, y, s2, ctx)
    got = ds.logl_batch(A, Bc, C, Dd, mu=mu, nu=nu)
    ref = O.logl_batch(A, Bc, C, Dd, t, y, s2, mu, nu, nthreads=8)
    assert relerr(got, ref) < 1e-11
    kern = pj._lib.lib().pioran_celerite_config_name(-1).decode()
    if layout in ("block", "tile"):   # small batches, 6 .. 63 rows: every draw its own table of the windowed kernel (round 3); "tile" takes no per-draw (c, d): automatic choice
        assert kern == ("block (per-draw tables)" if J >= 3 else "block+pd"), kern   # (one or two terms: per-draw ROWS, late round 4)
    else:
        assert kern in ("scan", "wide"), kern
    # one draw, or the same (c, d) in every draw, handed over as per-draw arrays: that is the shared case
    same, st = ds.logl_batch(A, Bc, np.tile(C[:1], (B, 1)), np.tile(Dd[:1], (B, 1)), mu=mu, nu=nu, return_status=True)
    ref_same = O.logl_batch(A, Bc, C[0], Dd[0], t, y, s2, mu, nu, nthreads=8)
    assert relerr(same, ref_same) < 1e-11
    one = ds.logl_batch(A[:1], Bc[:1], C[:1], Dd[:1], mu=mu[:1], nu=nu[:1])
    assert relerr(one, ref[:1]) < 1e-11
    if layout == "block":
        assert pj._lib.lib().pioran_celerite_config_name(-1).decode() == ("block" if J >= 3 else "scan")
    if layout == "tile":    # ... and the one-draw shared case is a launch it can take
        assert pj._lib.lib().pioran_celerite_config_name(-1).decode() == "tile"


@pytest.mark.parametrize("J,N,B", [(20, 100, 300), (16, 49, 700), (23, 33, 1000), (9, 80, 400), (20, 260, 513)])
def test_windowed_kernel_pair_table_modes_agree(ctx, J, N, B):
    """Above 256 draws the windowed kernel reads its pair table from global memory where that lets two workgroups share a CU (round 3);
    one LDS buffer, two, or none: the same numbers to the last bit, and the oracle's."""
    rng = np.random.default_rng(5100 + J + N)
    t, y, s2, A, Bc, C, Dd, mu, nu = _random_case(rng, N, J, B)
    ds = pj.Dataset(t, y, s2, ctx)
    outs = {}
    try:
        ctx.set_option("scan_config", "block")
        for em in (None, 0, 1, 2):
            ctx.set_option("block_emode", em)
            outs[em] = ds.logl_batch(A, Bc, C, Dd, mu=mu, nu=nu)
            assert pj._lib.lib().pioran_celerite_config_name(-1).decode() == "block"
    finally:
        ctx.set_option("block_emode", None); ctx.set_option("scan_config", None)
    for em in (0, 1, 2):
        assert np.array_equal(outs[em], outs[None]), em
    assert relerr(outs[None], O.logl_batch(A, Bc, C, Dd, t, y, s2, mu, nu, nthreads=8)) < 1e-11


def test_windowed_table_kernels_agree(ctx):
    """The windowed kernel's table is built by one workgroup per window (transcendentals once per (term, step) / (term, pair));
    the entry-per-thread kernel of round 2 is kept as its cross-check: same expressions on the same arguments, so log L comes out
    bit-identical — shared table, ragged last window, one-row terms, R + 1 = 16 NB exactly."""
    rng = np.random.default_rng(4242)
    for J, N, nreal in ((20, 333, 0), (5, 48, 2), (31, 100, 1), (8, 17, 1), (24, 1000, 0)):
        B = 9
        t, y, s2, A, Bc, C, Dd, mu, nu = _random_case(rng, N, J, B)
        Bc[:, :nreal] = 0.0; Dd[:nreal] = 0.0
        outs = []
        for ref_tab in (False, True):
            try:
                ctx.set_option("btab_reference", ref_tab)
                ds = pj.Dataset(t, y, s2, ctx)          # a fresh data set: the table is built on its first small batch
                outs.append(ds.logl_batch(A, Bc, C, Dd, mu=mu, nu=nu))
                assert pj._lib.lib().pioran_celerite_config_name(-1).decode() == "block"
                ds.close()
            finally:
                ctx.set_option("btab_reference", False)
        assert np.array_equal(outs[0], outs[1]), (J, N)
        assert relerr(outs[0], O.logl_batch(A, Bc, C, Dd, t, y, s2, mu, nu, nthreads=8)) < 1e-11


@pytest.mark.parametrize("J,B", [(40, 5), (44, 5), (47, 300), (40, 300)])
def test_rows_80_to_95_stay_register_resident(ctx, J, B):
    """R = 80 .. 95 rows (SHO-40, the dense configuration's model, is R = 80): past the throughput layouts' 79 rows the
    latency layout still holds S in registers, for any batch size; same values as the oracle and as the HBM fallback."""
    rng = np.random.default_rng(350 + J)
    t, y, s2, A, Bc, C, Dd, mu, nu = _random_case(rng, 90, J, B)
    ds = pj.Dataset(t, y, s2, ctx)
    got = ds.logl_batch(A, Bc, C, Dd, mu=mu, nu=nu)
    ref = O.logl_batch(A, Bc, C, Dd, t, y, s2, mu, nu, nthreads=8)
    assert relerr(got, ref) < 1e-11
    try:
        ctx.set_option("force_fallback", True)
        fb = ds.logl_batch(A[:7], Bc[:7], C, Dd, mu=mu[:7], nu=nu[:7])
    finally:
        ctx.set_option("force_fallback", False)
    assert relerr(fb, ref[:7]) < 1e-11
    tau = np.linspace(t[0] - 1, t[-1] + 1, 33)
    pm = ds.predict(A[:2], Bc[:2], C, Dd, tau, mu=mu[:2], nu=nu[:2])
    np.testing.assert_allclose(pm[0], O.predict(A[0], Bc[0], C, Dd, tau, t, y - mu[0], nu[0] * s2) + mu[0], rtol=1e-10, atol=1e-11)


@pytest.mark.parametrize("basis,B", [("SHO", 4096 + 104), ("SHO", 8192 + 500), ("DRWCelerite", 2048 + 77), ("DRWCelerite", 4096 + 200)])
def test_remainder_of_a_multi_pass_batch_on_the_second_stream(ctx, basis, B):
    """A batch that is not a whole number of passes of the throughput kernel (SHO-20: 4096 draws per pass, DRWCelerite-20: 2048): the
    remainder — or what exceeds half a pass — runs on the windowed kernel on the context's second stream, concurrently (capi.hip
    split_dispatch).  Same values as the single launch (another kernel family: to rounding) and as the oracle; option no_split."""
    rng = np.random.default_rng(B)
    N, J = 150, 20
    t = np.cumsum(rng.uniform(0.05, 2.0, N)); y = rng.standard_normal(N); yerr = rng.uniform(0.01, 0.05, N)
    th = O.synthetic_theta(B, t, y, seed=B)
    A, Bc, C, Dd, mu, nu = O.theta_to_coefs(th, t, J, basis)
    ds = pj.Dataset(t, y, yerr ** 2, ctx)
    # (round 5: from 49 rows on a shared series is celerite_tile.hip's by default, which has no passes to split; the step-by-step layouts
    #  and this split still serve per-draw series and "no_tile")
    ctx.set_option("no_tile", True)
    try:
        got, st = ds.logl_batch(A, Bc, C, Dd, mu=mu, nu=nu, return_status=True)
        assert pj._lib.lib().pioran_celerite_config_name(-1).decode() == "scan + block (remainder)"
        ctx.set_option("no_split", True)
        one, st1 = ds.logl_batch(A, Bc, C, Dd, mu=mu, nu=nu, return_status=True)
        assert pj._lib.lib().pioran_celerite_config_name(-1).decode() == "scan"
    finally:
        ctx.set_option("no_split", False)
        ctx.set_option("no_tile", False)
    ok = (st == 0) & (st1 == 0)
    assert np.array_equal(st == 0, st1 == 0) and ok.sum() > B // 2
    # Two kernel families on PRIOR draws.  Where a sampler lives (here: within 1e3 of the best draw) they agree to 1e-10.  In the far tail both
    # follow eps / ratio, ratio = nu min(sigma2) / sum(a) ~ 1 / cond(K) (profiles/r04_accuracy_vs_conditioning.txt), and on draws where D_n
    # crosses zero within rounding (the oracle calls them not positive definite, a GPU path may not) they differ by up to 1.4e-7.
    kept = ok & (one > one[ok].max() - 1e3)
    assert kept.sum() > B // 3 and relerr(got[kept], one[kept]) < 5e-10
    assert relerr(got[ok], one[ok]) < 1e-6
    idx = np.concatenate([np.arange(0, B, 97), np.arange(B - 20, B)])          # incl. the tail that went to the second stream
    ref, rst = O.logl_batch(A[idx], Bc[idx], C, Dd, t, y, yerr ** 2, mu[idx], nu[idx], nthreads=8, return_status=True)
    k = (rst == 0) & ok[idx]
    assert relerr(got[idx][k & kept[idx]], ref[k & kept[idx]]) < 1e-9 and relerr(got[idx][k], ref[k]) < 1e-6
    # per-draw series ride along (the windowed kernel stages them through LDS)
    Bs = 2048 + 64 if basis == "DRWCelerite" else 4096 + 64
    Y = rng.standard_normal((Bs, N)); S2 = rng.uniform(0.01, 0.1, (Bs, N))
    sl = slice(0, Bs)
    if Bs <= B:
        g2 = ds.logl_batch(A[sl], Bc[sl], C, Dd, mu=mu[sl], nu=nu[sl], Y=Y, S2=S2)
        tail = np.arange(Bs - 8, Bs)
        r2 = np.array([O.logl(A[i], Bc[i], C, Dd, t, Y[i] - mu[i], nu[i] * S2[i]) for i in tail])
        fin = np.isfinite(r2) & np.isfinite(g2[tail])
        assert relerr(g2[tail][fin], r2[fin]) < 1e-10


@pytest.mark.parametrize("J,B", [(40, 1024 + 70), (32, 2048 + 100), (39, 1024 + 256)])
def test_remainder_of_a_multi_pass_batch_64_to_95_rows(ctx, J, B):
    """64 .. 95 rows (a pass of the throughput kernel is 1024 .. 2048 draws there): the remainder, up to 256 draws, runs on the windowed
    kernel's five / six block columns on the second stream (round 4; SHO-40, 1100 draws at N = 1e4: 25 instead of 37 ms)."""
    rng = np.random.default_rng(B + J)
    N = 120
    t = np.cumsum(rng.uniform(0.05, 2.0, N)); y = rng.standard_normal(N); yerr = rng.uniform(0.01, 0.05, N)
    th = O.synthetic_theta(B, t, y, seed=B)
    A, Bc, C, Dd, mu, nu = O.theta_to_coefs(th, t, J, "SHO")
    ds = pj.Dataset(t, y, yerr ** 2, ctx)
    # (round 5: from 49 rows on a shared series is celerite_tile.hip's by default, which has no passes to split; the step-by-step layouts
    #  and this split still serve per-draw series and "no_tile")
    ctx.set_option("no_tile", True)
    try:
        got, st = ds.logl_batch(A, Bc, C, Dd, mu=mu, nu=nu, return_status=True)
        assert pj._lib.lib().pioran_celerite_config_name(-1).decode() == "scan + block (remainder)"
        ctx.set_option("no_split", True)
        one, st1 = ds.logl_batch(A, Bc, C, Dd, mu=mu, nu=nu, return_status=True)
        assert pj._lib.lib().pioran_celerite_config_name(-1).decode() == "scan"
    finally:
        ctx.set_option("no_split", False)
        ctx.set_option("no_tile", False)
    ok = (st == 0) & (st1 == 0)
    kept = ok & (one > one[ok].max() - 1e3)
    assert np.array_equal(st == 0, st1 == 0) and kept.sum() > B // 4 and relerr(got[kept], one[kept]) < 5e-10
    idx = np.concatenate([np.arange(0, B, 211), np.arange(B - 12, B)])
    ref, rst = O.logl_batch(A[idx], Bc[idx], C, Dd, t, y, yerr ** 2, mu[idx], nu[idx], nthreads=8, return_status=True)
    k = (rst == 0) & kept[idx]
    assert k.sum() >= 4 and relerr(got[idx][k], ref[k]) < 1e-9


@pytest.mark.parametrize("J,N,B,series", [(2, 40, 1, True), (20, 300, 8, False), (20, 300, 8, True), (5, 1000, 37, False), (31, 77, 3, True), (40, 64, 2, False)])
def test_small_host_calls_without_copy_commands(ctx, J, N, B, series):
    """Host-pointer calls whose coefficients and results fit 16 KB (the scalar drop-in, a few walkers): the kernels read a, b, mu, nu from and
    write log L / status to pinned host memory, (y | sigma2) go up in one copy (late round 4).  Bit for bit what the path with copy commands
    (context option exp = 64) returns, status included, and the oracle's values."""
    rng = np.random.default_rng(7300 + J + N + B)
    t, y, s2, A, Bc, C, Dd, mu, nu = _random_case(rng, N, J, B)
    A[B - 1] *= 1e3                                   # one draw the solver may flag
    Y = rng.standard_normal((B, N)) if series else None
    S2 = rng.uniform(0.01, 0.1, (B, N)) if series else None
    ds = pj.Dataset(t, y, s2, ctx)
    res = []
    try:
        for e in (64, 0, 0):
            ctx.set_option("exp", e)
            res.append(ds.logl_batch(A, Bc, C, Dd, mu=mu, nu=nu, Y=Y, S2=S2, return_status=True))
    finally:
        ctx.set_option("exp", 0)
    for got, st in res[1:]:
        assert np.array_equal(got, res[0][0], equal_nan=True) and np.array_equal(st, res[0][1])
    ref = np.array([O.logl(A[i], Bc[i], C, Dd, t, (Y[i] if series else y) - mu[i], nu[i] * (S2[i] if series else s2)) for i in range(B)])
    ok = (res[1][1] == 0) & np.isfinite(ref)
    assert ok[: B - 1].all() and relerr(res[1][0][ok], ref[ok]) < 1e-10
    if B == 1:
        one, st1 = ctx.logl(A[0], Bc[0], C, Dd, t, Y[0] - mu[0], nu[0] * S2[0], return_status=True)
        assert st1 == 0 and abs(one - ref[0]) <= 1e-10 * abs(ref[0])


@pytest.mark.parametrize("J,N,B", [(1, 300, 16), (2, 129, 70), (2, 1000, 300), (1, 77, 700), (2, 40, 2)])
def test_fewer_than_six_rows_per_draw_cd_on_the_windowed_kernel(ctx, J, N, B):
    """One or two terms with (c, d) per draw (a free Celerite / Exp term under a sampler): up to 768 draws run on the windowed kernel with per-draw
    rows since late round 4 (N = 1e4, 16 draws of one term: 7.5 -> 1.7 ms) — against the oracle and against the generic per-draw path."""
    rng = np.random.default_rng(6900 + 10 * J + N)
    t, y, s2, A, Bc, C, Dd, mu, nu = _random_case(rng, N, J, B, per_draw_cd=True)
    name = lambda: pj._lib.lib().pioran_celerite_config_name(-1).decode()
    ds = pj.Dataset(t, y, s2, ctx)
    got, st = ds.logl_batch(A, Bc, C, Dd, mu=mu, nu=nu, return_status=True)
    assert name() == "block+pd", name()
    try:
        ctx.set_option("no_block", True)
        gen, st2 = ds.logl_batch(A, Bc, C, Dd, mu=mu, nu=nu, return_status=True)
        assert "block" not in name()
    finally:
        ctx.set_option("no_block", False)
    assert np.array_equal(st, st2) and (st == 0).all()
    idx = np.unique(np.concatenate([np.arange(0, B, max(1, B // 24)), [B - 1]]))
    ref = np.array([O.logl(A[i], Bc[i], C[i], Dd[i], t, y - mu[i], nu[i] * s2) for i in idx])
    assert relerr(got[idx], ref) < 1e-10 and relerr(got, gen) < 1e-9


@pytest.mark.parametrize("J,nreal", [(1, 1), (1, 0), (2, 1), (2, 0), (3, 3), (4, 4), (3, 1)])
def test_fewer_than_six_rows_long_series_and_scalar_call(ctx, J, nreal):
    """1 .. 5 rows (the reference grid's j = 2 is four, benchmark/benchmarks.jl:16-18): five rows, long series (N >= 16384, up to 512 draws) and
    the scalar call from N = 2048 on run on the windowed kernel since late round 4 (N = 65536: 14.3 -> 9.5 ms); everything else on the
    throughput layout as before.  Both against the oracle, and which kernel ran."""
    rng = np.random.default_rng(7000 + 10 * J + nreal)
    name = lambda: pj._lib.lib().pioran_celerite_config_name(-1).decode()
    R = 2 * J - nreal
    for N, B in ((16384 + 77, 3), (2500, 1), (900, 1), (2500, 4)):
        t, y, s2, A, Bc, C, Dd, mu, nu = _random_case(rng, N, J, B)
        if nreal:
            Bc[:, -nreal:] = 0.0; Dd[-nreal:] = 0.0
        ds = pj.Dataset(t, y, s2, ctx)
        ref = np.array([O.logl(A[i], Bc[i], C, Dd, t, y - mu[i], nu[i] * s2) for i in range(B)])
        # round 5: up to 8 draws of a long series take the time-parallel family (celerite_tp.hip) — from 1024 steps on at up to 4 state rows, from
        # 2048 at up to 8; the serial-chain kernels this test is about are what "no_tp" leaves
        tp_takes = N >= (1024 if R <= 4 else 2048)
        got = ds.logl_batch(A, Bc, C, Dd, mu=mu, nu=nu)
        assert (name() == "tp") == tp_takes, (name(), R, N)
        assert relerr(got, ref) < 1e-10
        try:
            ctx.set_option("no_tp", True)
            got = ds.logl_batch(A, Bc, C, Dd, mu=mu, nu=nu)
            assert name() == ("block" if (R == 5 or N >= 16384) else "scan"), (name(), R, N)
            assert relerr(got, ref) < 1e-10
            if B == 1:
                one = ctx.logl(A[0], Bc[0], C, Dd, t, y - mu[0], nu[0] * s2)
                assert name() == ("block" if (R == 5 or N >= 2048) else "scan"), (name(), R, N)
                assert abs(one - ref[0]) <= 1e-10 * max(1.0, abs(ref[0]))
        finally:
            ctx.set_option("no_tp", False)
        if B == 1:
            one = ctx.logl(A[0], Bc[0], C, Dd, t, y - mu[0], nu[0] * s2)
            assert (name() == "tp") == tp_takes, (name(), R, N)
            assert abs(one - ref[0]) <= 1e-10 * max(1.0, abs(ref[0]))
        ds.close()


@pytest.mark.parametrize("J,nreal,N,B", [(40, 0, 61, 300), (40, 0, 90, 5), (33, 0, 130, 290), (36, 0, 47, 301), (39, 0, 1, 280), (39, 0, 2, 280),
                                          (40, 0, 3, 7), (40, 0, 4, 7), (40, 0, 5, 7), (40, 0, 6, 7), (40, 0, 7, 7), (40, 0, 8, 7), (40, 0, 9, 7),
                                          (45, 20, 75, 300), (50, 22, 64, 258), (42, 4, 333, 259), (44, 12, 51, 3)])
def test_rows_65_to_80_throughput_shapes(ctx, J, nreal, N, B):
    """65 .. 80 active rows, shared table (SHO-33 .. 40 — the dense configuration's model is SHO-40 —, DRWCelerite-22 .. 26 and other mixes
    of two-row and one-row terms): the throughput shapes with five rows per lane (rpl5_cbr4_nsrc4 and its paired / y-as-a-vector forms).
    Against the oracle and the lean latency kernel; series of odd and even length, N = 1 and 2, per-draw series."""
    rng = np.random.default_rng(8000 + J + N)
    t, y, s2, A, Bc, C, Dd, mu, nu = _random_case(rng, N, J, B)
    if nreal:      # one-row terms (b = d = 0: Exp / DRW): rows = 2 J - nreal
        Bc[:, -nreal:] = 0.0; Dd[-nreal:] = 0.0
    R = 2 * J - nreal
    assert 65 <= R <= 80
    ds = pj.Dataset(t, y, s2, ctx)
    ref, rst = O.logl_batch(A, Bc, C, Dd, t, y, s2, mu, nu, nthreads=8, return_status=True)
    try:
        ctx.set_option("no_wide", True); ctx.set_option("no_block", True)   # (batches up to 256 draws would take the windowed / the latency kernel)
        got, st = ds.logl_batch(A, Bc, C, Dd, mu=mu, nu=nu, return_status=True)
        cfg = pj._lib.lib().pioran_celerite_config_name(0).decode()
        assert pj._lib.lib().pioran_celerite_config_name(-1).decode() == "scan" and cfg.startswith("rpl5_cbr4_nsrc4"), cfg
        Y = rng.standard_normal((B, N)); S2 = rng.uniform(0.01, 0.1, (B, N))
        got2 = ds.logl_batch(A, Bc, C, Dd, mu=mu, nu=nu, Y=Y, S2=S2)
    finally:
        ctx.set_option("no_wide", False); ctx.set_option("no_block", False)
    assert np.array_equal(st, rst)
    assert relerr(got, ref) < 1e-11
    ref2 = np.array([O.logl(A[i], Bc[i], C, Dd, t, Y[i] - mu[i], nu[i] * S2[i]) for i in range(min(B, 40))])
    assert relerr(got2[:len(ref2)], ref2) < 1e-11
    try:
        ctx.set_option("no_block", True)
        lat = ds.logl_batch(A[:5], Bc[:5], C, Dd, mu=mu[:5], nu=nu[:5])     # five draws: the lean latency kernel
        assert pj._lib.lib().pioran_celerite_config_name(-1).decode() == "wide"
    finally:
        ctx.set_option("no_block", False)
    assert relerr(lat, ref[:5]) < 1e-11


@pytest.mark.parametrize("J,nreal,N,B", [(32, 0, 300, 4), (33, 0, 61, 3), (36, 0, 1, 2), (36, 0, 2, 2), (36, 0, 15, 2), (36, 0, 16, 2), (36, 0, 17, 2),
                                          (39, 0, 129, 5), (40, 0, 33, 3), (40, 0, 500, 2), (44, 0, 48, 2), (47, 0, 77, 7), (45, 20, 75, 6),
                                          (50, 22, 64, 3), (60, 30, 90, 2), (47, 0, 40, 256)])
def test_rows_64_to_95_windowed_kernel_with_five_and_six_block_columns(ctx, J, nreal, N, B):
    """64 .. 95 rows, up to 256 draws (round 4): the windowed kernel with five / six block columns (value only; the reference benchmark
    grid's j = 32 is 64 rows + y).  Against the oracle and the lean latency kernel (`no_block`), ragged windows, N = 1 and 2, one-row
    terms, per-draw series; more than 256 draws stay on the other kernels."""
    rng = np.random.default_rng(6400 + J + N)
    t, y, s2, A, Bc, C, Dd, mu, nu = _random_case(rng, N, J, B)
    if nreal:
        Bc[:, -nreal:] = 0.0; Dd[-nreal:] = 0.0
    R = 2 * J - nreal
    assert 64 <= R <= 95
    ds = pj.Dataset(t, y, s2, ctx)
    ref, rst = O.logl_batch(A, Bc, C, Dd, t, y, s2, mu, nu, nthreads=8, return_status=True)
    got, st = ds.logl_batch(A, Bc, C, Dd, mu=mu, nu=nu, return_status=True)
    assert pj._lib.lib().pioran_celerite_config_name(-1).decode() == "block"
    assert np.array_equal(st, rst) and relerr(got, ref) < 1e-11
    Y = rng.standard_normal((B, N)); S2 = rng.uniform(0.01, 0.1, (B, N))
    got2 = ds.logl_batch(A, Bc, C, Dd, mu=mu, nu=nu, Y=Y, S2=S2)
    assert pj._lib.lib().pioran_celerite_config_name(-1).decode() == "block"
    ref2 = np.array([O.logl(A[i], Bc[i], C, Dd, t, Y[i] - mu[i], nu[i] * S2[i]) for i in range(min(B, 6))])
    assert relerr(got2[:len(ref2)], ref2) < 1e-11
    try:
        ctx.set_option("no_block", True)
        lat = ds.logl_batch(A, Bc, C, Dd, mu=mu, nu=nu)
        assert pj._lib.lib().pioran_celerite_config_name(-1).decode() == "wide"
    finally:
        ctx.set_option("no_block", False)
    assert relerr(got, lat) < 1e-10
    if B == 256:     # one more draw: not the windowed kernel's any more
        ds.logl_batch(np.vstack([A, A[:1]]), np.vstack([Bc, Bc[:1]]), C, Dd, mu=np.append(mu, mu[0]), nu=np.append(nu, nu[0]))
        assert pj._lib.lib().pioran_celerite_config_name(-1).decode() != "block"


@pytest.mark.parametrize("J,N,B", [(48, 60, 5), (52, 33, 2), (56, 130, 3), (60, 61, 1), (64, 60, 5), (64, 700, 2), (71, 45, 3), (32, 300, 4), (40, 77, 2)])
def test_rows_64_to_143_lean_latency_layout(ctx, J, N, B):
    """R = 64 .. 143 rows stay register-resident (round 3): celerite_wide2_kernel, 5 .. 9 rows per lane.  The reference's own
    benchmark grid goes up to j = 64 terms = 128 rows (benchmark/benchmarks.jl:16-18), which used to run on the HBM-resident
    any-rank kernel.  Against the oracle, and against that kernel (still the path for more than 143 rows)."""
    rng = np.random.default_rng(300 + J)
    t, y, s2, A, Bc, C, Dd, mu, nu = _random_case(rng, N, J, B)
    ds = pj.Dataset(t, y, s2, ctx)
    got, st = ds.logl_batch(A, Bc, C, Dd, mu=mu, nu=nu, return_status=True)
    ref = O.logl_batch(A, Bc, C, Dd, t, y, s2, mu, nu, nthreads=8)
    assert relerr(got, ref) < 1e-11 and (st == 0).all()
    Y = rng.standard_normal((B, N)); S2 = rng.uniform(0.01, 0.1, (B, N))       # per-draw series through the y slot's thread
    got2 = ds.logl_batch(A, Bc, C, Dd, mu=mu, nu=nu, Y=Y, S2=S2)
    ref2 = np.array([O.logl(A[i], Bc[i], C, Dd, t, Y[i] - mu[i], nu[i] * S2[i]) for i in range(B)])
    assert relerr(got2, ref2) < 1e-11
    try:
        ctx.set_option("force_fallback", True)
        fb = ds.logl_batch(A, Bc, C, Dd, mu=mu, nu=nu)
    finally:
        ctx.set_option("force_fallback", False)
    assert relerr(fb, ref) < 1e-11
    plain = ds.logl_batch(A, Bc, C, Dd)                                          # no mu, no nu
    assert relerr(plain, O.logl_batch(A, Bc, C, Dd, t, y, s2, np.zeros(B), np.ones(B), nthreads=8)) < 1e-11
    if 2 * J > 79:
        # per-draw (c, d) past the throughput layouts' 79 rows: every draw gets its own table, the same kernel walks it
        C2 = np.tile(C, (B, 1)) * rng.uniform(0.8, 1.2, (B, J)); D2 = np.tile(Dd, (B, 1)) * rng.uniform(0.8, 1.2, (B, J))
        got3, st3 = ds.logl_batch(A, Bc, C2, D2, mu=mu, nu=nu, Y=Y, S2=S2, return_status=True)
        ref3 = np.array([O.logl(A[i], Bc[i], C2[i], D2[i], t, Y[i] - mu[i], nu[i] * S2[i]) for i in range(B)])
        assert relerr(got3, ref3) < 1e-11 and (st3 == 0).all()


def test_per_draw_tables_in_chunks(ctx):
    """Per-draw (c, d) with 80 rows and more draws than one chunk of per-draw tables holds (256): two chunks, ragged tail."""
    rng = np.random.default_rng(77)
    N, B, J = 24, 300, 40
    t, y, s2, A, Bc, C, Dd, mu, nu = _random_case(rng, N, J, B, per_draw_cd=True)
    got, st = pj.Dataset(t, y, s2, ctx).logl_batch(A, Bc, C, Dd, mu=mu, nu=nu, return_status=True)
    ref = O.logl_batch(A, Bc, C, Dd, t, y, s2, mu, nu, nthreads=8)
    assert relerr(got, ref) < 1e-11 and (st == 0).all()


def test_lean_latency_layout_mixed_rows_and_nonpd(ctx):
    """celerite_wide2_kernel with per-draw rows (a QPO-like term with per-draw (c, d) on 33 shared terms: 68 rows) and with a
    draw whose D_n goes negative (status 1, log|D_n| as the reference, src/celerite_solver.jl:140)."""
    rng = np.random.default_rng(9)
    N, B, J = 150, 6, 34
    t, y, s2, A, Bc, C, Dd, mu, nu = _random_case(rng, N, J, B, per_draw_cd=True)
    C[:, :33] = C[0, :33]; Dd[:, :33] = Dd[0, :33]
    ds = pj.Dataset(t, y, s2, ctx)
    try:
        ctx.set_option("no_block", True)
        got, st = ds.logl_batch(A, Bc, C, Dd, mu=mu, nu=nu, return_status=True)
    finally:
        ctx.set_option("no_block", False)
    ref = O.logl_batch(A, Bc, C, Dd, t, y, s2, mu, nu, nthreads=8)
    assert relerr(got, ref) < 1e-11 and (st == 0).all()
    A2 = A.copy(); A2[2, :] *= -1.0      # indefinite "covariance": D_1 < 0 -> NaN like the reference's log(D[1]) DomainError
    A2[4, 5] = -30.0
    got3, st3 = ds.logl_batch(A2, Bc, C[0], Dd[0], mu=mu, nu=nu, return_status=True)
    ref3, rst3 = O.logl_batch(A2, Bc, C[0], Dd[0], t, y, s2, mu, nu, nthreads=8, return_status=True)
    assert (np.isnan(got3) == np.isnan(ref3)).all()
    fin = np.isfinite(ref3)
    assert relerr(got3[fin], ref3[fin]) < 1e-9 and ((st3 != 0) == (rst3 != 0)).all()


def test_three_step_form_is_the_default_for_24_to_31_rows_in_large_batches(ctx):
    """R = 30 rows (SHO-15 / DRWCelerite-10), more than 2048 draws: the throughput scan takes its three-step form on its own
    (two rows per lane, 16 source lanes: tools/sweep_win3.py); series lengths of every remainder mod 3."""
    rng = np.random.default_rng(33)
    for N in (60, 61, 62):
        B, J = 2100, 15
        t, y, s2, A, Bc, C, Dd, mu, nu = _random_case(rng, N, J, B)
        got, st = pj.Dataset(t, y, s2, ctx).logl_batch(A, Bc, C, Dd, mu=mu, nu=nu, return_status=True)
        assert pj._lib.lib().pioran_celerite_config_name(0).decode() == "rpl2_cbr1_nsrc16_p+win3"
        assert relerr(got, O.logl_batch(A, Bc, C, Dd, t, y, s2, mu, nu, nthreads=8)) < 1e-11 and (st == 0).all()


@pytest.mark.parametrize("J,cfg", [(8, "rpl1_cbr1_nsrc16_yp"), (16, "rpl2_cbr1_nsrc16_yp"), (24, "rpl3_cbr2_nsrc8_yp")])
@pytest.mark.parametrize("N", [1, 2, 5, 130])
def test_one_more_row_with_y_as_a_vector(ctx, J, cfg, N):
    """R = 16, 32, 48 rows (the reference benchmark's j = 8, 16 and SHO-24) in the 16-, 32- and 48-slot shapes: y as a separate
    vector (kernel template YC) frees the slot it used to take; several draws per wavefront here (four, four, two)."""
    rng = np.random.default_rng(900 + J + N)
    B = 45
    t, y, s2, A, Bc, C, Dd, mu, nu = _random_case(rng, N, J, B)
    ds = pj.Dataset(t, y, s2, ctx)
    try:
        ctx.set_option("no_block", True); ctx.set_option("no_wide", True)
        got, st = ds.logl_batch(A, Bc, C, Dd, mu=mu, nu=nu, return_status=True)
        assert pj._lib.lib().pioran_celerite_config_name(0).decode() == cfg
        assert relerr(got, O.logl_batch(A, Bc, C, Dd, t, y, s2, mu, nu, nthreads=8)) < 1e-11 and (st == 0).all()
        Y = rng.standard_normal((B, N)); S2 = rng.uniform(0.01, 0.1, (B, N))
        got2 = ds.logl_batch(A, Bc, C, Dd, mu=mu, nu=nu, Y=Y, S2=S2)
        ref2 = np.array([O.logl(A[i], Bc[i], C, Dd, t, Y[i] - mu[i], nu[i] * S2[i]) for i in range(B)])
        assert relerr(got2, ref2) < 1e-11
        A2 = A.copy(); A2[3, 0] = -40.0                          # a draw that is not positive definite: status and log|D| semantics
        got3, st3 = ds.logl_batch(A2, Bc, C, Dd, mu=mu, nu=nu, return_status=True)
        ref3, rst3 = O.logl_batch(A2, Bc, C, Dd, t, y, s2, mu, nu, nthreads=8, return_status=True)
        fin = np.isfinite(ref3)
        assert (np.isnan(got3) == np.isnan(ref3)).all() and ((st3 != 0) == (rst3 != 0)).all() and relerr(got3[fin], ref3[fin]) < 1e-9
    finally:
        ctx.set_option("no_block", False); ctx.set_option("no_wide", False)


@pytest.mark.parametrize("N", [1, 2, 3, 4, 5, 64, 257])
def test_64_rows_in_the_64_row_shape(ctx, N):
    """R = 64 rows (the reference benchmark's j = 32, benchmark/benchmarks.jl:16-18) in the 64-row throughput shape: y rides as a
    separate vector instead of a row slot (kernel template YC, configurations rpl4_cbr4_nsrc4_y / _yp), odd and even series
    lengths (the two-step form pairs the steps), shared and per-draw (c, d), per-draw series, a row map that is not all pairs."""
    rng = np.random.default_rng(640 + N)
    B, J = 70, 32
    t, y, s2, A, Bc, C, Dd, mu, nu = _random_case(rng, N, J, B)
    ds = pj.Dataset(t, y, s2, ctx)
    try:
        ctx.set_option("no_block", True); ctx.set_option("no_wide", True)
        got, st = ds.logl_batch(A, Bc, C, Dd, mu=mu, nu=nu, return_status=True)
        cfg = pj._lib.lib().pioran_celerite_config_name(0).decode()
        ref = O.logl_batch(A, Bc, C, Dd, t, y, s2, mu, nu, nthreads=8)
        assert cfg == "rpl4_cbr4_nsrc4_yp", cfg
        assert relerr(got, ref) < 1e-11 and (st == 0).all()
        Y = rng.standard_normal((B, N)); S2 = rng.uniform(0.01, 0.1, (B, N))
        got2 = ds.logl_batch(A, Bc, C, Dd, mu=mu, nu=nu, Y=Y, S2=S2)
        ref2 = np.array([O.logl(A[i], Bc[i], C, Dd, t, Y[i] - mu[i], nu[i] * S2[i]) for i in range(B)])
        assert relerr(got2, ref2) < 1e-11
        # per-draw (c, d): no table, transcendentals in the kernel
        C2 = np.tile(C, (B, 1)) * rng.uniform(0.8, 1.2, (B, J)); D2 = np.tile(Dd, (B, 1)) * rng.uniform(0.8, 1.2, (B, J))
        got3 = ds.logl_batch(A, Bc, C2, D2, mu=mu, nu=nu)
        ref3 = O.logl_batch(A, Bc, C2, D2, t, y, s2, mu, nu, nthreads=8)
        assert relerr(got3, ref3) < 1e-11
        # 30 two-row terms + 4 one-row terms = 64 rows, not all pairs: the unpaired y-vector shape
        J4 = 34
        t4, y4, s4, A4, B4, C4, D4, mu4, nu4 = _random_case(rng, max(N, 2), J4, 9)
        B4[:, 30:] = 0.0; D4[30:] = 0.0
        ds4 = pj.Dataset(t4, y4, s4, ctx)
        got4 = ds4.logl_batch(A4, B4, C4, D4, mu=mu4, nu=nu4)
        assert pj._lib.lib().pioran_celerite_config_name(0).decode() == "rpl4_cbr4_nsrc4_y"
        assert relerr(got4, O.logl_batch(A4, B4, C4, D4, t4, y4, s4, mu4, nu4, nthreads=8)) < 1e-11
    finally:
        ctx.set_option("no_block", False); ctx.set_option("no_wide", False)


@pytest.mark.parametrize("J", [80, 100])
def test_fallback_any_rank(ctx, J):
    """More than 143 rows run on the HBM-resident any-rank kernel (celerite_fallback.hip)."""
    rng = np.random.default_rng(300 + J)
    N, B = 40, 3
    t, y, s2, A, Bc, C, Dd, mu, nu = _random_case(rng, N, J, B)
    ds = pj.Dataset(t, y, s2, ctx)
    got = ds.logl_batch(A, Bc, C, Dd, mu=mu, nu=nu)
    ref = O.logl_batch(A, Bc, C, Dd, t, y, s2, mu, nu, nthreads=8)
    assert relerr(got, ref) < 1e-11


def test_real_terms_row_compaction(ctx, layout):
    """Exp / DRW terms (b = d = 0): their zero sin rows are dropped; result must equal the full-rank oracle."""
    rng = np.random.default_rng(7)
    N, B, J = 200, 9, 12
    t, y, s2, A, Bc, C, Dd, mu, nu = _random_case(rng, N, J, B)
    Bc[:, 5:] = 0.0
    Dd[5:] = 0.0
    ds = pj.Dataset(t, y, s2, ctx)
    got = ds.logl_batch(A, Bc, C, Dd, mu=mu, nu=nu)
    ref = O.logl_batch(A, Bc, C, Dd, t, y, s2, mu, nu, nthreads=8)
    assert relerr(got, ref) < 1e-11


def test_edge_sizes(ctx, layout):
    rng = np.random.default_rng(11)
    for N in (1, 2, 3):
        t, y, s2, A, Bc, C, Dd, mu, nu = _random_case(rng, N, 4, 3)
        ds = pj.Dataset(t, y, s2, ctx)
        got = ds.logl_batch(A, Bc, C, Dd, mu=mu, nu=nu)
        ref = O.logl_batch(A, Bc, C, Dd, t, y, s2, mu, nu)
        assert relerr(got, ref) < 1e-12
    # B = 1 scalar drop-in, sigma2 = 0 (test/test_mean.jl:64-74 uses zero measurement variance)
    t, y, s2, A, Bc, C, Dd, mu, nu = _random_case(rng, 100, 6, 1)
    v = ctx.logl(A[0], Bc[0], C, Dd, t, y, np.zeros_like(s2))
    assert abs(v - O.logl(A[0], Bc[0], C, Dd, t, y, np.zeros_like(s2))) <= 1e-10 * abs(v)


def test_block_kernel_edges(ctx):
    """Windowed kernel (celerite_block.hip): series shorter than, equal to and just past a window / two windows, every block
    count NB = 1..4, batches above the automatic limit, per-draw series, the y row in the last lane of a block (R = 15, 31, 47)
    and in the first lane of the next one (R = 16, 32, 48)."""
    rng = np.random.default_rng(77)
    ctx.set_option("scan_config", "block")
    try:
        for J, N, B in [(1, 1, 3), (2, 15, 4), (8, 16, 5), (8, 17, 5), (12, 31, 2), (16, 32, 3), (16, 33, 300), (20, 100, 7),
                        (24, 64, 3), (30, 49, 2), (31, 130, 3)]:
            t, y, s2, A, Bc, C, Dd, mu, nu = _random_case(rng, N, J, B)
            ds = pj.Dataset(t, y, s2, ctx)
            got, st = ds.logl_batch(A, Bc, C, Dd, mu=mu, nu=nu, return_status=True)
            ref = O.logl_batch(A, Bc, C, Dd, t, y, s2, mu, nu, nthreads=8)
            assert relerr(got, ref) < 1e-11, (J, N, B)
            assert (st == 0).all()
        # odd row counts through real (one-row) terms: R = 15, 16, 31, 47
        for J, nreal in [(8, 1), (9, 2), (16, 1), (24, 1)]:
            t, y, s2, A, Bc, C, Dd, mu, nu = _random_case(rng, 70, J, 5)
            Bc[:, :nreal] = 0.0
            Dd[:nreal] = 0.0
            ds = pj.Dataset(t, y, s2, ctx)
            got = ds.logl_batch(A, Bc, C, Dd, mu=mu, nu=nu)
            ref = O.logl_batch(A, Bc, C, Dd, t, y, s2, mu, nu, nthreads=8)
            assert relerr(got, ref) < 1e-11, (J, nreal)
        # per-draw series
        t, y, s2, A, Bc, C, Dd, mu, nu = _random_case(rng, 90, 20, 6)
        Y = rng.standard_normal((6, 90)); S2 = rng.uniform(0.01, 0.1, (6, 90))
        ds = pj.Dataset(t, y, s2, ctx)
        got = ds.logl_batch(A, Bc, C, Dd, mu=mu, nu=nu, Y=Y, S2=S2)
        ref = np.array([O.logl(A[i], Bc[i], C, Dd, t, Y[i] - mu[i], nu[i] * S2[i]) for i in range(6)])
        assert relerr(got, ref) < 1e-11
        # non-positive-definite draws follow the reference's log(abs(D_n)) (src/celerite_solver.jl:140) and are flagged
        t, y, s2, A, Bc, C, Dd, mu, nu = _random_case(rng, 60, 20, 4)
        A[1] *= -1.0
        got, st = pj.Dataset(t, y, s2, ctx).logl_batch(A, Bc, C, Dd, mu=mu, nu=nu, return_status=True)
        ref, rst = O.logl_batch(A, Bc, C, Dd, t, y, s2, mu, nu, nthreads=4, return_status=True)
        assert (st == rst).all() and st[1] != 0
        ok = np.isfinite(ref)
        assert relerr(got[ok], ref[ok]) < 1e-9 and (np.isnan(got) == np.isnan(ref)).all()
    finally:
        ctx.set_option("scan_config", None)


def test_latency_layout_edges(ctx):
    """celerite_wide.hip on its own: every prologue / tail length of the 4-deep record pipeline (N = 1..9), every
    RPL (R = 2J = 2..78), with and without mu / nu, per-draw series, and the not-positive-definite status."""
    rng = np.random.default_rng(12)
    ctx.set_option("scan_config", "wide")
    try:
        for N in range(1, 10):
            t, y, s2, A, Bc, C, Dd, mu, nu = _random_case(rng, N, 9, 3)
            ds = pj.Dataset(t, y, s2, ctx)
            assert relerr(ds.logl_batch(A, Bc, C, Dd, mu=mu, nu=nu), O.logl_batch(A, Bc, C, Dd, t, y, s2, mu, nu)) < 1e-12
        for J in (1, 7, 8, 15, 16, 23, 24, 31, 32, 39):
            t, y, s2, A, Bc, C, Dd, mu, nu = _random_case(rng, 203, J, 5)
            ds = pj.Dataset(t, y, s2, ctx)
            ref = O.logl_batch(A, Bc, C, Dd, t, y, s2, mu, nu, nthreads=8)
            assert relerr(ds.logl_batch(A, Bc, C, Dd, mu=mu, nu=nu), ref) < 1e-11, J
        t, y, s2, A, Bc, C, Dd, mu, nu = _random_case(rng, 150, 12, 4)
        ds = pj.Dataset(t, y, s2, ctx)
        zero, one = np.zeros(4), np.ones(4)
        assert relerr(ds.logl_batch(A, Bc, C, Dd), O.logl_batch(A, Bc, C, Dd, t, y, s2, zero, one)) < 1e-11
        Y = y[None, :] + 0.01 * rng.standard_normal((4, 150)); S2 = np.broadcast_to(s2, (4, 150)) * rng.uniform(0.5, 2, (4, 1))
        got = ds.logl_batch(A, Bc, C, Dd, mu=mu, nu=nu, Y=Y, S2=S2)
        ref = np.array([O.logl(A[i], Bc[i], C, Dd, t, Y[i] - mu[i], nu[i] * S2[i]) for i in range(4)])
        assert relerr(got, ref) < 1e-11
        # not positive definite: same status and |D| semantics as the throughput layouts
        A2 = A.copy(); A2[1] = -5.0
        out, st = ds.logl_batch(A2, Bc, C, Dd, mu=mu, nu=nu, return_status=True)
        ctx.set_option("scan_config", "rpl2_cbr1_nsrc13")
        out_t, st_t = ds.logl_batch(A2, Bc, C, Dd, mu=mu, nu=nu, return_status=True)
        assert (st == st_t).all() and st[1] != 0 and st[0] == 0
        ok = np.isfinite(out_t)
        assert (np.isfinite(out) == ok).all() and relerr(out[ok], out_t[ok]) < 1e-9
    finally:
        ctx.set_option("scan_config", None)


def test_drwcelerite_block_layout(ctx):
    """DRWCelerite with 20 components (20 two-row + 20 one-row terms) runs on the block-layout configuration; same
    values as the plain configuration and as the oracle; 12 components (no matching block layout) stay on the plain one."""
    rng = np.random.default_rng(41)
    t = np.cumsum(rng.uniform(0.05, 2.0, 300)); y = rng.standard_normal(300); yerr = rng.uniform(0.01, 0.05, 300)
    th = O.synthetic_theta(300, t, y)
    ds = pj.Dataset(t, y, yerr ** 2, ctx)
    name = lambda: pj._lib.lib().pioran_celerite_config_name(0).decode()
    for ncomp, expect in ((20, "rpl4_cbr4_nsrc4_b5a"), (12, "rpl3_cbr2_nsrc7")):
        A, Bc, C, Dd, mu, nu = O.theta_to_coefs(th, t, ncomp, "DRWCelerite")
        ctx.set_option("no_block", True)   # 300 draws would take the windowed kernel: this test is about the throughput layouts
        got = ds.logl_batch(A, Bc, C, Dd, mu=mu, nu=nu)
        assert name() == expect, name()
        ref, rst = O.logl_batch(A, Bc, C, Dd, t, y, yerr ** 2, mu, nu, nthreads=8, return_status=True)
        ok = rst == 0
        assert ok.sum() > 100 and relerr(got[ok], ref[ok]) < 1e-9
        try:
            ctx.set_option("no_paired", True)
            plain = ds.logl_batch(A, Bc, C, Dd, mu=mu, nu=nu)
            assert not name().startswith("rpl4_cbr4_nsrc4_b5")
        finally:
            ctx.set_option("no_paired", False)
            ctx.set_option("no_block", False)
        assert relerr(got[ok], plain[ok]) < 1e-9   # different row order => different summation order of q


def test_status_not_positive_definite(ctx):
    rng = np.random.default_rng(5)
    t = np.cumsum(rng.uniform(0.1, 2, 50)); y = rng.standard_normal(50); s2 = np.full(50, 1e-8)
    ds = pj.Dataset(t, y, s2, ctx)
    A = np.array([[1.0], [-5.0]]); Bc = np.zeros((2, 1))
    out, st = ds.logl_batch(A, Bc, np.array([0.1]), np.array([0.0]), return_status=True)
    ref, rst = O.logl_batch(A, Bc, np.array([0.1]), np.array([0.0]), t, y, s2, return_status=True)
    assert st[0] == 0 and st[1] != 0 and rst[1] != 0
    assert abs(out[0] - ref[0]) <= 1e-11 * abs(ref[0])
    with pytest.raises(ValueError):
        pj.logl([-5.0], [0.0], [0.1], [0.0], t, y, s2, ctx=ctx)


def test_all_kernel_configs_agree(ctx):
    """Tuning alternatives (context option "scan_config") compute the same thing."""
    rng = np.random.default_rng(21)
    t, y, s2, A, Bc, C, Dd, mu, nu = _random_case(rng, 300, 20, 21)
    ref = O.logl_batch(A, Bc, C, Dd, t, y, s2, mu, nu, nthreads=8)
    ds = pj.Dataset(t, y, s2, ctx)
    try:
        for name in ("rpl3_cbr2_nsrc7_p", "rpl3_cbr2_nsrc8_p", "rpl3_cbr2_nsrc7", "rpl3_cbr2_nsrc8", "rpl3_cbr4_nsrc4", "rpl4_cbr4_nsrc4",
                     "rpl5_cbr4_nsrc4", "rpl4_cbr4_nsrc4_p", "rpl5_cbr4_nsrc4_p", "wide", "block"):
            ctx.set_option("scan_config", name)
            got = ds.logl_batch(A, Bc, C, Dd, mu=mu, nu=nu)
            if name not in ("wide", "block"):   # (the small-batch kernels of celerite_wide.hip / celerite_block.hip are not entries of the scan table)
                assert pj._lib.lib().pioran_celerite_config_name(0).decode() == name   # what the launch actually ran on
            assert relerr(got, ref) < 1e-11, name
        ctx.set_option("force_fallback", True)
        assert relerr(ds.logl_batch(A, Bc, C, Dd, mu=mu, nu=nu), ref) < 1e-11
    finally:
        ctx.set_option("scan_config", None)
        ctx.set_option("force_fallback", False)

def test_ill_conditioned_draws_vs_quad_truth(ctx, golden_dir):
    """Every kernel family against log L evaluated in __float128 (tests/golden/quad_truth.npz, oracle/celerite_oracle_q.c) on the
    ill-conditioned prior draws of the bench model: ratio = nu min(sigma2) / sum(a) ~ 1 / cond(K) from 1e-5 down to 3e-10, series of 150,
    1000 and 1e4 time stamps.  What the truth settles (profiles/r05_quad_truth.txt, tools/window_precision_study.py): the fp64 ORACLE itself
    is up to 8e-9 from the exact value below ratio 1e-8 — rounding sum(a), nu sigma2 and the phases alone costs 7e-9 there — and every family,
    step-by-step or windowed, has the same error distribution (median 1e-13 .. 1e-10, 90th percentile ~1e-10); single draws whose pivots
    come close to zero reach 2 .. 3e-8 on the windowed kernels (one or two of ~40 draws per series).  From ratio 1e-8 on — and every stored
    chain of the reference sits above 1e-5 — all families hold the north-star bar against the TRUTH."""
    q = np.load(golden_dir / "quad_truth.npz")
    name = lambda: pj._lib.lib().pioran_celerite_config_name(-1).decode()   # noqa: E731
    for N in (150, 1000, 10000):
        tag = f"n{N}"
        t, y, yerr = O.synthetic_series(N, seed=1234) if N == 10000 else (q[f"{tag}_t"], q[f"{tag}_y"], q[f"{tag}_yerr"])
        A, Bc, C, Dd, mu, nu = (q[f"{tag}_{k}"] for k in ("A", "Bc", "C", "Dd", "mu", "nu"))
        truth, ratio = q[f"{tag}_truth"], q[f"{tag}_ratio"]
        ds = pj.Dataset(t, y, yerr ** 2, ctx)
        res = {}
        try:
            ctx.set_option("no_block", True); ctx.set_option("no_wide", True)
            res["scan"], st = ds.logl_batch(A, Bc, C, Dd, mu=mu, nu=nu, return_status=True)
            assert name() == "scan" and (st == 0).all()
            ctx.set_option("no_block", False); ctx.set_option("no_wide", False)
            for fam in ("block", "tile"):
                ctx.set_option("scan_config", fam)
                res[fam], st = ds.logl_batch(A, Bc, C, Dd, mu=mu, nu=nu, return_status=True)
                assert name() == fam and (st == 0).all()
            # the time-parallel family (celerite_tp.hip; 64 draws per call): it filters in P = P_inf - S with the process noise in closed form and is
            # 30 .. 300 times CLOSER to the truth than the reference's recurrence in any evaluation order (max 1e-10 over all bins)
            # (tp_scan = 0: the sequential boundary walk.  With the boundary phase as a scan — round 6 — a draw whose scan fails the check is evaluated again by the
            #  windowed small-batch kernel and comes back with THAT family's accuracy: second leg below)
            ctx.set_option("scan_config", "tp")
            tpv, tpa = np.empty(len(truth)), np.empty(len(truth))
            for mode, dst in ((0, tpv), (-1, tpa)):
                ctx.set_option("tp_scan", mode); ctx.set_option("tp_unchecked", mode == 0)         # (the family's own arithmetic | the product: checked, repaired)
                for b0 in range(0, len(truth), 16):
                    sl = slice(b0, min(len(truth), b0 + 16))
                    dst[sl], st = ds.logl_batch(A[sl], Bc[sl], C, Dd, mu=mu[sl], nu=nu[sl], return_status=True)
                    assert name() == "tp" and (st == 0).all()
        finally:
            ctx.set_option("scan_config", None); ctx.set_option("no_block", False); ctx.set_option("no_wide", False); ctx.set_option("tp_scan", -1); ctx.set_option("tp_unchecked", False)
        etp = np.abs(tpv - truth) / np.abs(truth)
        assert etp.max() < 5e-10 and np.median(etp) < 5e-12, (N, "tp", etp.max(), np.median(etp))
        eta = np.abs(tpa - truth) / np.abs(truth)
        assert eta[ratio >= 1e-8].max() < 1e-8 and eta.max() < 5e-8 and np.median(eta) < 5e-12, (N, "tp, scan + check + repair", eta.max(), np.median(eta))
        hi, lo = ratio >= 1e-8, ratio < 1e-8
        for fam, v in res.items():
            err = np.abs(v - truth) / np.abs(truth)
            assert err[hi].max() < 1e-8, (N, fam, err[hi].max())                      # the bar, against the exact value
            assert np.median(err[lo]) < 1e-9 and np.percentile(err[lo], 80) < 8e-9 and np.median(err) < 2e-10, (N, fam)   # below 1e-8: the same distribution for every family ...
            assert err[lo].max() < (1e-8 if fam == "scan" else 5e-8), (N, fam, err[lo].max())   # ... and its tail (fp64 oracle: 8e-9)
        ds.close()


def test_tile_kernel_edges(ctx):
    """Windowed form with one draw per wavefront (celerite_tile.hip; default for large batches from 49 rows on): series shorter than,
    equal to and just past a window / two windows, every block count NB = 1..6, batches that do not fill their last workgroup, the y row
    in the last lane of a block and in the first lane of the next one, one-row terms, no mu / nu, non-positive-definite draws; a draw's
    value does not depend on its position in the batch nor on how the batch is cut into workspace chunks."""
    rng = np.random.default_rng(771)
    name = lambda: pj._lib.lib().pioran_celerite_config_name(-1).decode()   # noqa: E731
    ctx.set_option("scan_config", "tile")
    try:
        for J, N, B in [(1, 1, 3), (2, 15, 4), (8, 16, 5), (8, 17, 5), (12, 31, 2), (16, 32, 3), (16, 33, 301), (20, 100, 7),
                        (24, 64, 3), (30, 49, 2), (31, 130, 3), (32, 47, 9), (39, 81, 6), (40, 160, 5), (47, 35, 6)]:
            t, y, s2, A, Bc, C, Dd, mu, nu = _random_case(rng, N, J, B)
            ds = pj.Dataset(t, y, s2, ctx)
            got, st = ds.logl_batch(A, Bc, C, Dd, mu=mu, nu=nu, return_status=True)
            assert name() == "tile"
            ref = O.logl_batch(A, Bc, C, Dd, t, y, s2, mu, nu, nthreads=8)
            assert relerr(got, ref) < 1e-11, (J, N, B)
            assert (st == 0).all()
        # odd row counts through real (one-row) terms: R = 15, 16, 31, 47, 63, 64, 79, 95
        for J, nreal in [(8, 1), (9, 2), (16, 1), (24, 1), (32, 1), (33, 2), (40, 1), (48, 1)]:
            t, y, s2, A, Bc, C, Dd, mu, nu = _random_case(rng, 70, J, 5)
            Bc[:, :nreal] = 0.0
            Dd[:nreal] = 0.0
            ds = pj.Dataset(t, y, s2, ctx)
            got = ds.logl_batch(A, Bc, C, Dd, mu=mu, nu=nu)
            assert name() == "tile"
            ref = O.logl_batch(A, Bc, C, Dd, t, y, s2, mu, nu, nthreads=8)
            assert relerr(got, ref) < 1e-11, (J, nreal)
        # 96 rows and more: launches it does not take (the automatic choice runs)
        t, y, s2, A, Bc, C, Dd, mu, nu = _random_case(rng, 40, 48, 3)
        got = pj.Dataset(t, y, s2, ctx).logl_batch(A, Bc, C, Dd, mu=mu, nu=nu)
        assert name() != "tile" and relerr(got, O.logl_batch(A, Bc, C, Dd, t, y, s2, mu, nu, nthreads=4)) < 1e-11
        # per-draw series (the shifted log-flux models hand every draw its own y and sigma2): ragged last window, every block count
        for J, N, B in [(20, 90, 6), (7, 16, 5), (27, 33, 7), (40, 50, 5)]:
            t, y, s2, A, Bc, C, Dd, mu, nu = _random_case(rng, N, J, B)
            Y = rng.standard_normal((B, N)); S2 = rng.uniform(0.01, 0.1, (B, N))
            ds = pj.Dataset(t, y, s2, ctx)
            got = ds.logl_batch(A, Bc, C, Dd, mu=mu, nu=nu, Y=Y, S2=S2)
            assert name() == "tile"
            ref = np.array([O.logl(A[i], Bc[i], C, Dd, t, Y[i] - mu[i], nu[i] * S2[i]) for i in range(B)])
            assert relerr(got, ref) < 1e-11, (J, N, B)
        t, y, s2, A, Bc, C, Dd, mu, nu = _random_case(rng, 90, 20, 6)
        ds = pj.Dataset(t, y, s2, ctx)
        # neither mu nor nu
        got = ds.logl_batch(A, Bc, C, Dd)
        assert name() == "tile" and relerr(got, O.logl_batch(A, Bc, C, Dd, t, y, s2, np.zeros(6), np.ones(6), nthreads=4)) < 1e-11
        # non-positive-definite draws follow the reference's log(abs(D_n)) (src/celerite_solver.jl:140) and are flagged
        t, y, s2, A, Bc, C, Dd, mu, nu = _random_case(rng, 60, 20, 4)
        A[1] *= -1.0
        got, st = pj.Dataset(t, y, s2, ctx).logl_batch(A, Bc, C, Dd, mu=mu, nu=nu, return_status=True)
        ref, rst = O.logl_batch(A, Bc, C, Dd, t, y, s2, mu, nu, nthreads=4, return_status=True)
        assert name() == "tile" and (st == rst).all() and st[1] != 0
        ok = np.isfinite(ref)
        assert relerr(got[ok], ref[ok]) < 1e-9 and (np.isnan(got) == np.isnan(ref)).all()
        # position in the batch and workspace chunks: same bits
        t, y, s2, A, Bc, C, Dd, mu, nu = _random_case(rng, 200, 26, 2600)     # 52 rows: four block columns, a pass is 2048 draws
        ds = pj.Dataset(t, y, s2, ctx)
        whole = ds.logl_batch(A, Bc, C, Dd, mu=mu, nu=nu)
        assert name() == "tile"
        perm = rng.permutation(2600)
        shuffled = ds.logl_batch(A[perm], Bc[perm], C, Dd, mu=mu[perm], nu=nu[perm])
        assert np.array_equal(shuffled, whole[perm])
        ctx.trim()                                        # (the limit is on NEW workspace: drop the 34 MB the call above left)
        ctx.set_option("workspace_limit_mb", 32)          # 13 windows x 1 KB x 2600 draws = 34 MB: two chunks
        try:
            chunked = ds.logl_batch(A, Bc, C, Dd, mu=mu, nu=nu)
        finally:
            ctx.set_option("workspace_limit_mb", None)
        assert name() == "tile" and np.array_equal(chunked, whole)
        assert relerr(whole, O.logl_batch(A, Bc, C, Dd, t, y, s2, mu, nu, nthreads=8)) < 1e-11
    finally:
        ctx.set_option("scan_config", None)


def test_tile_kernel_is_the_default_for_large_batches_from_49_rows(ctx):
    """capi.hip tile_dispatch: shared (c, d), no per-draw rows or series; 49 rows and more: every batch above the small-batch windowed kernel's
    range; 39 .. 47 rows (SHO-20 is 40): the same; 33 .. 38 and 48 rows: what falls between the passes of the throughput layouts (up to three
    quarters of a pass past the last whole one, unless the small-batch kernel takes the remainder beside the scan); 17 .. 32 rows: 513 .. 2048
    draws (round 6: the committed sweep had SHO-12 at 1536 / 2048 draws 20 % ahead on this kernel, tools/retune_thresholds.py); "no_tile" switches it off."""
    rng = np.random.default_rng(772)
    name = lambda: pj._lib.lib().pioran_celerite_config_name(-1).decode()   # noqa: E731
    for J, B, want in [(25, 513, "tile"), (25, 512, "block"), (24, 600, "tile"), (24, 2048, "scan"), (24, 2500, "tile"), (24, 4000, "scan"), (20, 4096, "tile"), (19, 4096, "scan"),
                       (16, 1024, "tile"), (16, 2048, "tile"), (16, 2049, "scan"), (8, 700, "scan"), (32, 257, "tile"), (40, 300, "tile"), (40, 256, "block")]:
        t, y, s2, A, Bc, C, Dd, mu, nu = _random_case(rng, 50, J, B)
        ds = pj.Dataset(t, y, s2, ctx)
        got = ds.logl_batch(A, Bc, C, Dd, mu=mu, nu=nu)
        assert name().startswith(want), (J, B, name())
        assert relerr(got, O.logl_batch(A, Bc, C, Dd, t, y, s2, mu, nu, nthreads=8)) < 1e-11
        if want == "tile":
            ctx.set_option("no_tile", True)
            try:
                other = ds.logl_batch(A, Bc, C, Dd, mu=mu, nu=nu)
            finally:
                ctx.set_option("no_tile", False)
            assert name() != "tile" and relerr(other, got) < 1e-11


# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def full_size():
    t, y, yerr = O.synthetic_series(10_000, seed=1234)
    return t, y, yerr


def test_full_size_vs_oracle(ctx, full_size, layout):
    """BASELINE config 2/3 shape: N = 1e4, J = 20 (SHO-20) and J = 40 (DRWCelerite-20); bar 1e-8 (north star)."""
    t, y, yerr = full_size
    th = O.synthetic_theta(48, t, y)
    ds = pj.Dataset(t, y, yerr ** 2, ctx)
    for basis in ("SHO", "DRWCelerite"):
        A, Bc, C, Dd, mu, nu = O.theta_to_coefs(th, t, 20, basis)
        ref, rst = O.logl_batch(A, Bc, C, Dd, t, y, yerr ** 2, mu, nu, nthreads=8, return_status=True)
        got, st = ds.logl_batch(A, Bc, C, Dd, mu=mu, nu=nu, return_status=True)
        ok = rst == 0
        assert ok.sum() >= 24
        assert relerr(got[ok], ref[ok]) < 1e-8, basis
        assert (st[ok] == 0).all()


def test_full_size_properties(ctx, full_size):
    """Size-independent identities of a Gaussian log-density at N = 1e4, J = 20, B = 512."""
    t, y, yerr = full_size
    N = len(t)
    th = O.synthetic_theta(512, t, y, seed=99)
    A, Bc, C, Dd, mu, nu = O.theta_to_coefs(th, t, 20, "SHO")
    ds = pj.Dataset(t, y, yerr ** 2, ctx)
    base, st = ds.logl_batch(A, Bc, C, Dd, mu=mu, nu=nu, return_status=True)
    ok = st == 0
    assert ok.mean() > 0.9
    # (1) scale covariance: y -> s y, K -> s^2 K  =>  logL -> logL - N log s
    s = 3.0
    ds2 = pj.Dataset(t, s * y, s * s * yerr ** 2, ctx)
    sc = ds2.logl_batch(s * s * A, s * s * Bc, C, Dd, mu=s * mu, nu=nu)
    assert relerr(sc[ok], (base - N * np.log(s))[ok]) < 1e-8   # s = 3 changes every rounding; north-star bar
    ds4 = pj.Dataset(t, 2.0 * y, 4.0 * yerr ** 2, ctx)   # power-of-two scaling is exact in fp64
    sc4 = ds4.logl_batch(4.0 * A, 4.0 * Bc, C, Dd, mu=2.0 * mu, nu=nu)
    assert relerr(sc4[ok], (base - N * np.log(2.0))[ok]) < 1e-13
    # (2) permutation of terms leaves the kernel unchanged
    perm = np.random.default_rng(0).permutation(20)
    pm = ds.logl_batch(A[:, perm], Bc[:, perm], C[perm], Dd[perm], mu=mu, nu=nu)
    assert relerr(pm[ok], base[ok]) < 1e-8
    # (3) splitting a term in two halves (J = 21) leaves the kernel unchanged
    A2 = np.concatenate([A, A[:, :1] / 2], axis=1); A2[:, 0] /= 2
    B2 = np.concatenate([Bc, Bc[:, :1] / 2], axis=1); B2[:, 0] /= 2
    sp = ds.logl_batch(A2, B2, np.append(C, C[0]), np.append(Dd, Dd[0]), mu=mu, nu=nu)
    assert relerr(sp[ok], base[ok]) < 1e-8
    # (4) batch consistency: the same draw evaluated in a different batch position / batch size is bit-identical
    sub = ds.logl_batch(A[100:103], Bc[100:103], C, Dd, mu=mu[100:103], nu=nu[100:103])
    assert (sub == base[100:103]).all() or np.array_equal(np.isnan(sub), np.isnan(base[100:103]))


# ---------------------------------------------------------------------------------------------
# dense solver: log_likelihood_direct (src/direct_solver.jl:6-21)
# ---------------------------------------------------------------------------------------------
def test_dense_covariance_build(ctx):
    rng = np.random.default_rng(31)
    for N, J in ((5, 1), (70, 3), (130, 6)):
        t = rng.uniform(0, 50, N)          # unsorted on purpose: tau = |t_i - t_k|
        a = rng.uniform(0.1, 2, J); b = rng.uniform(-0.2, 0.2, J); c = rng.uniform(0.05, 1, J); d = rng.uniform(0, 3, J)
        s2 = rng.uniform(0.01, 0.1, N)
        K = ctx.dense_covariance(a, b, c, d, t, s2)
        ref = np.array([[O.kappa(a, b, c, d, abs(ti - tk)) for tk in t] for ti in t]) + np.diag(s2)
        np.testing.assert_allclose(K, ref, rtol=1e-13, atol=1e-15)
        assert (K == K.T).all()


def test_dense_covariance_build_sorted_fast_path(ctx):
    """Ascending t takes the factorised build (exp split at the tile corner + angle addition) for off-diagonal
    64 x 64 tiles; entries must agree with the closed form to ~1e-15 of the kernel amplitude."""
    rng = np.random.default_rng(32)
    for N, J in ((130, 3), (300, 20), (513, 7)):
        t = np.cumsum(rng.uniform(0.05, 3.0, N)) + 1000.0     # large absolute phases d * t
        a = rng.uniform(0.1, 2, J); b = rng.uniform(-0.2, 0.2, J); c = rng.uniform(0.01, 3, J); d = rng.uniform(0, 30, J)
        s2 = rng.uniform(0.01, 0.1, N)
        K = ctx.dense_covariance(a, b, c, d, t, s2)
        tau = np.abs(t[:, None] - t[None, :])
        ref = sum(np.exp(-c[j] * tau) * (a[j] * np.cos(d[j] * tau) + b[j] * np.sin(d[j] * tau)) for j in range(J)) + np.diag(s2)
        assert np.max(np.abs(K - ref)) <= 2e-12 * np.abs(a).sum()   # phase rounding |d t| 2^-53 ~ 1e-11 rad at most
        assert (K == K.T).all()


@pytest.mark.parametrize("N,J", [(1, 1), (6, 2), (63, 3), (64, 3), (65, 3), (200, 5), (257, 20), (1000, 8)])
def test_dense_nll_vs_oracle(ctx, N, J):
    rng = np.random.default_rng(400 + N)
    t = np.cumsum(rng.uniform(0.05, 2.0, N)); y = rng.standard_normal(N); s2 = rng.uniform(0.01, 0.1, N)
    a = rng.uniform(0.1, 2, J); b = rng.uniform(-0.05, 0.05, J) * a; c = rng.uniform(0.05, 2, J); d = rng.uniform(0, 3, J)
    got, info = ctx.dense_nll(a, b, c, d, t, y, s2, return_info=True)
    ref = O.dense_nll(a, b, c, d, t, y, s2)
    assert info == 0
    assert abs(got - ref) <= 1e-11 * abs(ref)


@pytest.mark.parametrize("N", [129, 191, 192, 193, 257, 320, 1000, 1472, 1536, 1700, 2760, 2881, 3100])
def test_dense_one_launch_per_block_column_equals_the_panel_update_chain(ctx, N):
    """log_likelihood_direct (src/direct_solver.jl:6-21) for one matrix: the one-launch-per-block-column factorisation of round 4
    (dense_step_kernel: critical workgroup + strips + lagging bulk, paired / single-panel phases, half tiles) against the panel / update
    chain of rounds 1-3 (option dense_old_chain) and the oracle, at sizes on both sides of every schedule switch (3 .. 49 block columns)."""
    rng = np.random.default_rng(9000 + N)
    J = 5
    t = np.cumsum(rng.uniform(0.05, 2.0, N)); y = rng.standard_normal(N); s2 = rng.uniform(0.01, 0.1, N)
    a = rng.uniform(0.1, 2, J); b = rng.uniform(-0.05, 0.05, J) * a; c = rng.uniform(0.05, 2, J); d = rng.uniform(0, 3, J)
    new, i1 = ctx.dense_nll(a, b, c, d, t, y, s2, return_info=True)
    try:
        ctx.set_option("dense_old_chain", 1)
        old, i0 = ctx.dense_nll(a, b, c, d, t, y, s2, return_info=True)
        ctx.set_option("dense_old_chain", 0); ctx.set_option("dense_no_pairs", True)
        single, i2 = ctx.dense_nll(a, b, c, d, t, y, s2, return_info=True)
        ctx.set_option("dense_no_pairs", False); ctx.set_option("dense_no_halves", True)
        whole, i3 = ctx.dense_nll(a, b, c, d, t, y, s2, return_info=True)
        ctx.set_option("dense_no_halves", False)
        # the option has two values: anything else (the numbers once taken by the timing experiments of round 4 among them) is refused
        for v in (2, 5, 8):
            with pytest.raises(pj._lib.PioranHipError):
                ctx.set_option("dense_old_chain", v)
    finally:
        ctx.set_option("dense_old_chain", 0); ctx.set_option("dense_no_pairs", False); ctx.set_option("dense_no_halves", False)
    assert i0 == i1 == i2 == i3 == 0
    assert abs(new - old) <= 1e-12 * abs(old) and abs(single - old) <= 1e-12 * abs(old) and whole == new
    if N <= 1000:
        ref = O.dense_nll(a, b, c, d, t, y, s2)
        assert abs(new - ref) <= 1e-11 * abs(ref)
    # a matrix that stops being positive definite in the middle: both chains report the same first bad pivot (LAPACK's info)
    bad = int(0.6 * N)
    s2b = s2.copy(); s2b[bad] = -50.0
    try:
        v1, j1 = ctx.dense_nll(a, b, c, d, t, y, s2b, return_info=True)
        ctx.set_option("dense_old_chain", 1)
        v0, j0 = ctx.dense_nll(a, b, c, d, t, y, s2b, return_info=True)
    finally:
        ctx.set_option("dense_old_chain", 0)
    assert np.isnan(v1) and np.isnan(v0) and j1 == j0 == bad + 1


def test_dense_reference_relation(ctx, golden_dir):
    """The reference's own test relation: logpdf (celerite) == -log_likelihood_direct, isapprox rtol 1.49e-8
    (test/test_likelihood.jl:58-59, test/test_scalablegp.jl:128) — here both sides on the GPU, bar 1e-10."""
    lit = json.loads((golden_dir / "reference_literals.json").read_text())
    g = lit["scalablegp_n6"]
    t = np.array(g["t"]); y = np.array(g["y"]); yerr = np.array(g["yerr"])
    for i in range(10):
        R = pj.approx(pj.SingleBendingPowerLaw(g["alpha1"][i], g["f1"][i], g["alpha2"][i]), g["f_min"], g["f_max"],
                      g["n_components"], g["variance"][i], basis_function="SHO")
        f = pj.ScalableGP(g["mu"][i], R)
        cel = pj.logpdf(f(t, yerr ** 2), y, ctx=ctx)
        den = -pj.log_likelihood_direct(f.kernel, t, y - g["mu"][i], yerr ** 2, ctx=ctx)
        assert abs(cel - den) <= 1e-10 * abs(den)
    A = np.loadtxt(golden_dir / "simu_log.txt")
    t, y, yerr = A[:, 0], A[:, 1], A[:, 2]
    f0 = 1 / (t[-1] - t[0]) / 100
    fM = 1 / np.min(np.diff(t)) / 2 * 20
    rel = {c["name"]: c for c in json.loads((golden_dir / "relation_cases.json").read_text())["cases"]}
    for basis in ("SHO", "DRWCelerite"):
        R = pj.approx(pj.SingleBendingPowerLaw(0.82, 0.01, 3.3), f0, fM, 20, np.var(y, ddof=1), basis_function=basis)
        cel = pj.log_likelihood(R, t, y, yerr ** 2, ctx=ctx)
        den = -pj.log_likelihood_direct(R, t, y, yerr ** 2, ctx=ctx)
        assert abs(cel - den) <= 1e-10 * abs(den)
        assert abs(den - rel[f"simu_log[{basis}]"]["logl_dense"]) <= 1e-10 * abs(den)


def test_dense_batch(ctx, golden_dir):
    """pioran_dense_nll_batch: B factorisations in batched launches == B single calls == -celerite path; per-draw mu / nu;
    shared and per-draw (c, d); one non-PD draw in the middle only flags itself."""
    rng = np.random.default_rng(17)
    A_ = np.loadtxt(golden_dir / "simu.txt")
    t, y, yerr = A_[:300, 0], A_[:300, 1], A_[:300, 2]
    B, J = 19, 6
    _, _, _, A, Bc, C, Dd, mu, nu = _random_case(rng, 300, J, B)
    one = np.array([ctx.dense_nll(A[i], Bc[i], C, Dd, t, y - mu[i], nu[i] * yerr ** 2) for i in range(B)])
    got, info = ctx.dense_nll_batch(A, Bc, C, Dd, t, y, yerr ** 2, mu=mu, nu=nu, return_info=True)
    assert (info == 0).all() and relerr(got, one) < 1e-13
    cel = pj.Dataset(t, y, yerr ** 2, ctx).logl_batch(A, Bc, C, Dd, mu=mu, nu=nu)
    assert relerr(-got, cel) < 1e-9
    C2 = np.tile(C, (B, 1)) * rng.uniform(0.8, 1.2, (B, J)); D2 = np.tile(Dd, (B, 1)) * rng.uniform(0.8, 1.2, (B, J))
    got2 = ctx.dense_nll_batch(A, Bc, C2, D2, t, y, yerr ** 2, mu=mu, nu=nu)
    ref2 = np.array([O.dense_nll(A[i], Bc[i], C2[i], D2[i], t, y - mu[i], nu[i] * yerr ** 2) for i in range(B)])
    assert relerr(got2, ref2) < 1e-10
    Abad = A.copy(); Abad[7] = -3.0
    got3, info3 = ctx.dense_nll_batch(Abad, Bc, C, Dd, t, y, yerr ** 2, mu=mu, nu=nu, return_info=True)
    assert info3[7] != 0 and np.isnan(got3[7]) and (np.delete(info3, 7) == 0).all() and relerr(np.delete(got3, 7), np.delete(one, 7)) < 1e-13


def test_dense_batch_long_series_grouped_steps(ctx):
    """Batched launches take the steps of the factorisation in fours and pairs (256- / 128-deep trailing updates) where one matrix takes
    them in pairs and singles: N = 2100 (33 tiles per side), 5 matrices per launch, per-draw mu / nu, shared and per-draw (c, d) —
    against single calls, the oracle's dense path and the celerite path."""
    rng = np.random.default_rng(23)
    N, J, B = 2100, 5, 5
    t, y, s2, A, Bc, C, Dd, mu, nu = _random_case(rng, N, J, B)
    one = np.array([ctx.dense_nll(A[i], Bc[i], C, Dd, t, y - mu[i], nu[i] * s2) for i in range(B)])
    got, info = ctx.dense_nll_batch(A, Bc, C, Dd, t, y, s2, mu=mu, nu=nu, return_info=True)
    assert (info == 0).all() and relerr(got, one) < 1e-11
    ref = np.array([O.dense_nll_numpy(A[i], Bc[i], C, Dd, t, y - mu[i], nu[i] * s2) for i in (0, B - 1)])   # (LAPACK: the C restatement is O(N^3) scalar code)
    assert relerr(got[[0, B - 1]], ref) < 1e-10
    cel = pj.Dataset(t, y, s2, ctx).logl_batch(A, Bc, C, Dd, mu=mu, nu=nu)
    assert relerr(-got, cel) < 1e-9
    C2 = np.tile(C, (B, 1)) * rng.uniform(0.8, 1.2, (B, J)); D2 = np.tile(Dd, (B, 1)) * rng.uniform(0.8, 1.2, (B, J))
    got2 = ctx.dense_nll_batch(A, Bc, C2, D2, t, y, s2, mu=mu, nu=nu)
    one2 = np.array([ctx.dense_nll(A[i], Bc[i], C2[i], D2[i], t, y - mu[i], nu[i] * s2) for i in range(B)])
    assert relerr(got2, one2) < 1e-11
    # fewer matrices per launch than draws: several batched launches per call
    ctx.set_option("dense_streams", 2)
    try:
        got3 = ctx.dense_nll_batch(A, Bc, C, Dd, t, y, s2, mu=mu, nu=nu)
    finally:
        ctx.set_option("dense_streams", None)
    assert relerr(got3, got) < 1e-11


def test_dense_not_positive_definite(ctx):
    t = np.linspace(0, 10, 40); y = np.ones(40); s2 = np.full(40, 1e-9)
    val, info = ctx.dense_nll([-1.0], [0.0], [0.3], [0.0], t, y, s2, return_info=True)
    assert info == 1 and np.isnan(val)          # first pivot K_11 = -1 + 1e-9 <= 0
    with pytest.raises(np.linalg.LinAlgError):
        pj.log_likelihood_direct(pj.Celerite(-1.0, 0.0, 0.3, 0.0), t, y, s2, ctx=ctx)


def test_dense_full_size_relation(ctx, full_size):
    """BASELINE config 5: N = 4096 prefix, SHO-40 (J = 40): dense (MFMA Cholesky) vs celerite scan, bar 1e-8."""
    t, y, yerr = (v[:4096] for v in full_size)
    f_min, f_max = 1 / (t[-1] - t[0]), 1 / np.min(np.diff(t)) / 2
    R = pj.approx(pj.SingleBendingPowerLaw(0.82, 0.01, 3.3), f_min, f_max, 40, 1.0, basis_function="SHO")
    mu = float(np.mean(y))
    den, info = ctx.dense_nll(R.a, R.b, R.c, R.d, t, y - mu, yerr ** 2, return_info=True)
    cel = pj.log_likelihood(R, t, y - mu, yerr ** 2, ctx=ctx)
    assert info == 0
    assert abs(cel + den) <= 1e-8 * abs(den)
    # ... and BOTH against the CPU oracle at this size (one evaluation, ~30 ms): anchors the 80-row celerite_wide_kernel<6> and
    # the MFMA Cholesky at length, not only against each other
    ref = O.logl(R.a, R.b, R.c, R.d, t, y - mu, yerr ** 2)
    assert abs(cel - ref) <= 1e-8 * abs(ref), (cel, ref)
    assert abs(-den - ref) <= 1e-8 * abs(ref), (den, ref)
    # the throughput shape for 80 rows would be the any-rank kernel; the batch entry at B = 3 takes the same latency layout
    got3 = pj.Dataset(t, y, yerr ** 2, ctx).logl_batch(np.tile(R.a, (3, 1)), np.tile(R.b, (3, 1)), R.c, R.d, mu=np.full(3, mu))
    assert np.max(np.abs(got3 - ref)) <= 1e-8 * abs(ref)


# ---------------------------------------------------------------------------------------------
# C-ABI behaviour: caching, re-preparation, several handles, argument errors
# ---------------------------------------------------------------------------------------------
def test_scalar_entry_caches_series_and_table(ctx):
    """Repeated logl calls with the same t (sampler pattern) reuse the resident series; changing y, sigma2,
    (a, b), (c, d), J or t between calls must still give the right answer every time."""
    rng = np.random.default_rng(77)
    t, y, s2, A, Bc, C, Dd, mu, nu = _random_case(rng, 300, 5, 4)
    for k in range(4):   # same t, same (c, d); fresh y - mu, nu * s2, (a, b)
        v = ctx.logl(A[k], Bc[k], C, Dd, t, y - mu[k], nu[k] * s2)
        assert abs(v - O.logl(A[k], Bc[k], C, Dd, t, y - mu[k], nu[k] * s2)) <= 1e-11 * abs(v)
    C2 = C * 1.3
    assert abs(ctx.logl(A[0], Bc[0], C2, Dd, t, y, s2) - O.logl(A[0], Bc[0], C2, Dd, t, y, s2)) <= 1e-9   # new (c, d)
    assert abs(ctx.logl(A[0, :3], Bc[0, :3], C[:3], Dd[:3], t, y, s2) - O.logl(A[0, :3], Bc[0, :3], C[:3], Dd[:3], t, y, s2)) <= 1e-9
    t2 = t * 1.01                                                                                              # new t
    assert abs(ctx.logl(A[0], Bc[0], C, Dd, t2, y, s2) - O.logl(A[0], Bc[0], C, Dd, t2, y, s2)) <= 1e-9
    t3 = t[:200]                                                                                               # new N
    assert abs(ctx.logl(A[0], Bc[0], C, Dd, t3, y[:200], s2[:200]) - O.logl(A[0], Bc[0], C, Dd, t3, y[:200], s2[:200])) <= 1e-9


def test_two_datasets_and_two_contexts(ctx):
    rng = np.random.default_rng(78)
    c1 = _random_case(rng, 150, 6, 9)
    c2 = _random_case(rng, 90, 11, 5)
    ctx2 = pj.Context(0)
    ds1 = pj.Dataset(c1[0], c1[1], c1[2], ctx)
    ds2 = pj.Dataset(c2[0], c2[1], c2[2], ctx2)
    ds3 = pj.Dataset(c2[0], c2[1], c2[2], ctx)      # second data set on the first context
    for _ in range(2):                               # interleaved use must not cross-contaminate cached tables
        for ds, cs in ((ds1, c1), (ds2, c2), (ds3, c2)):
            t, y, s2, A, Bc, C, Dd, mu, nu = cs
            got = ds.logl_batch(A, Bc, C, Dd, mu=mu, nu=nu)
            assert relerr(got, O.logl_batch(A, Bc, C, Dd, t, y, s2, mu, nu)) < 1e-11
    ds2.close(); ctx2.close()


def test_prepared_state_survives_host_pointer_calls(ctx):
    """The (c, d) declared by pioran_dataset_prepare belong to the *_dev entries and nothing else touches them: a mixed-mode
    host call (per-draw rows), a theta-only call with another n_components / f-range, a plain host batch with other (c, d)
    and a gradient call in between must leave a following *_dev launch on the caller's [B][J] arrays correct."""
    import torch
    rng = np.random.default_rng(81)
    t, y, s2, A, Bc, C, Dd, mu, nu = _random_case(rng, 200, 20, 300)
    ds = pj.Dataset(t, y, s2, ctx)
    ds.prepare(C, Dd)
    dev = torch.device("cuda", 0)
    d = [torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in (A, Bc, mu, nu)]
    dout = torch.empty(300, dtype=torch.float64, device=dev); dst = torch.zeros(300, dtype=torch.int32, device=dev)
    ref = O.logl_batch(A, Bc, C, Dd, t, y, s2, mu, nu, nthreads=8)

    def dev_call(B):
        dout.fill_(float("nan")); torch.cuda.synchronize()
        ds.logl_batch_dev(B, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), 0, 0, dout.data_ptr(), dst.data_ptr())
        ctx.synchronize()
        assert relerr(dout[:B].cpu().numpy(), ref[:B]) < 1e-11 and (dst[:B].cpu().numpy() == 0).all()

    dev_call(300)
    # (1) mixed mode: 21 terms, one of them with per-draw (c, d)
    C2 = np.tile(np.append(C, 0.3), (40, 1)); D2 = np.tile(np.append(Dd, 1.0), (40, 1))
    C2[:, 20] = rng.uniform(0.1, 1.0, 40); D2[:, 20] = rng.uniform(0.5, 2.0, 40)
    A2 = np.concatenate([A[:40], rng.uniform(0.1, 1, (40, 1))], axis=1); B2 = np.concatenate([Bc[:40], np.zeros((40, 1))], axis=1)
    mixed = ds.logl_batch(A2, B2, C2, D2, mu=mu[:40], nu=nu[:40])
    assert relerr(mixed, O.logl_batch(A2, B2, C2, D2, t, y, s2, mu[:40], nu[:40], nthreads=8)) < 1e-11
    dev_call(300); dev_call(7)          # both layouts
    # (2) theta-only entry: J = 12 DRWCelerite terms (24 celerite terms, another row map), another frequency range
    th = np.column_stack([rng.uniform(0, 1.5, 16), np.exp(rng.uniform(-4, 0, 16)), rng.uniform(2, 4, 16)])
    ds.logpdf_theta(pj.SingleBendingPowerLaw, th, 1.0, 1e-3, 3.0, 12, basis_function="DRWCelerite")
    dev_call(300)
    # (3) host batch with other shared (c, d) and (4) a gradient call
    ds.logl_batch(A[:5, :7], Bc[:5, :7], C[:7] * 1.5, Dd[:7])
    ds.logl_grad(A[:2, :9], Bc[:2, :9], C[:9] * 0.7, Dd[:9], mu=mu[:2], nu=nu[:2])
    assert ds.J == 20
    dev_call(300); dev_call(1)
    # a per-draw term declared through prepare() is refused by the *_dev entry instead of reading a (0, 0, 1) table row
    ds.prepare(C, Dd, real_term=[2] + [0] * 19)
    L = pj._lib.lib()
    v = ctypes.c_void_p
    assert L.pioran_celerite_logl_batch_dev(ds._h, 4, v(d[0].data_ptr()), v(d[1].data_ptr()), None, None, None, None,
                                            v(dout.data_ptr()), None) == -1


def test_abi_argument_errors_on_gpu(ctx):
    L = pj._lib.lib()
    rng = np.random.default_rng(79)
    t, y, s2, A, Bc, C, Dd, mu, nu = _random_case(rng, 50, 3, 2)
    ds = pj.Dataset(t, y, s2, ctx)
    # device-pointer batch before pioran_dataset_prepare -> invalid argument, not a crash
    assert L.pioran_celerite_logl_batch_dev(ds._h, 2, 1, 1, None, None, None, None, 1, None) == -1
    with pytest.raises(ValueError):
        ds.logl_batch(A, Bc[:, :2], C, Dd)
    with pytest.raises(ValueError):
        ds.logl_batch(A, Bc, C, Dd, Y=np.zeros((2, 50)))
    with pytest.raises(pj._lib.PioranHipError):     # a "real" term must have d = 0
        ds.prepare(C, np.ones(3), real_term=[1, 0, 0])
    with pytest.raises(ValueError):
        pj.Dataset(t, y[:10], s2, ctx)
    assert L.pioran_ctx_event_record(ctx._h, 99) == -1
    ctx.event_record(0); ctx.event_record(1)
    assert ctx.event_elapsed_ms(0, 1) >= 0.0


def test_large_batch_and_long_series(ctx):
    """B = 20000 draws (ragged vs workgroup size) at small N, and N = 65536 (the reference benchmark's longest
    series, benchmark/benchmarks.jl:16) at small B, J = 16 terms."""
    rng = np.random.default_rng(80)
    t, y, s2, A, Bc, C, Dd, mu, nu = _random_case(rng, 40, 4, 20001)
    got = pj.Dataset(t, y, s2, ctx).logl_batch(A, Bc, C, Dd, mu=mu, nu=nu)
    sel = rng.choice(20001, 300, replace=False)
    assert relerr(got[sel], O.logl_batch(A[sel], Bc[sel], C, Dd, t, y, s2, mu[sel], nu[sel], nthreads=8)) < 1e-11
    t, y, s2, A, Bc, C, Dd, mu, nu = _random_case(rng, 65536, 16, 3)
    got = pj.Dataset(t, y, s2, ctx).logl_batch(A, Bc, C, Dd, mu=mu, nu=nu)
    assert relerr(got, O.logl_batch(A, Bc, C, Dd, t, y, s2, mu, nu, nthreads=3)) < 1e-9


def test_nonpd_value_follows_reference_abs_semantics(ctx):
    """D_n <= 0 for some n >= 2 but D_1 > 0: the reference silently uses log(abs(D[n])) (celerite_solver.jl:140);
    the value must match the oracle's (which restates that), with status 1."""
    rng = np.random.default_rng(91)
    t = np.cumsum(rng.uniform(0.2, 1.0, 60)); y = rng.standard_normal(60); s2 = np.full(60, 1e-3)
    # two terms, the second with a negative amplitude: sum(a) + s2 > 0 but K is indefinite
    a = np.array([1.0, -0.9]); b = np.zeros(2); c = np.array([0.05, 2.0]); d = np.array([0.0, 0.0])
    ref, rst = O.logl(a, b, c, d, t, y, s2, return_status=True)
    got, st = ctx.logl(a, b, c, d, t, y, s2, return_status=True)
    assert rst == 1 and st == 1 and np.isfinite(ref)
    assert abs(got - ref) <= 1e-9 * abs(ref)


def test_custom_mean_logpdf(ctx):
    """test/test_mean.jl:64-74: CustomMean, zero measurement variance, N = 100 on a regular grid: finite logpdf,
    equal to the oracle with the mean subtracted."""
    t = np.linspace(0, 1000, 100)
    mfun = lambda x: 1.3 * np.sin(2 * np.pi * x / 53.4) + 0.84
    R = pj.approx(pj.SingleBendingPowerLaw(0.4, 1e-2, 3.1), 1e-3, 1e3, 20, 0.3, basis_function="SHO")
    fx = pj.ScalableGP(pj.CustomMean(mfun), R)(t, np.zeros(100))
    y = np.random.default_rng(12).standard_normal(100)
    val = pj.logpdf(fx, y, ctx=ctx)
    assert np.isfinite(val)
    assert abs(val - O.logl(R.a, R.b, R.c, R.d, t, y - mfun(t), np.zeros(100))) <= 1e-9 * abs(val)


# ---------------------------------------------------------------------------------------------
# approx on the device: theta -> log L in one call
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("basis", ["SHO", "DRWCelerite"])
@pytest.mark.parametrize("integ", [True, False])
def test_device_approx_matches_host_approx(ctx, basis, integ):
    """Coefficients produced by the device approx kernel vs the host approx_batch (itself pinned to the reference's
    amplitude golden, test/test_psd.jl:38) — same 1e-9 bar as the host tests (cond of the spectral matrix ~1e3-1e4)."""
    rng = np.random.default_rng(55)
    B = 200
    t = np.cumsum(rng.uniform(0.05, 2.0, 120)); y = rng.standard_normal(120); s2 = rng.uniform(0.01, 0.1, 120)
    th = np.column_stack([rng.uniform(-0.25, 2, B), np.exp(rng.uniform(np.log(1e-3), np.log(5), B)), rng.uniform(1.5, 4, B)])
    var = np.exp(rng.standard_normal(B))
    ds = pj.Dataset(t, y, s2, ctx)
    out, st, A, Bc = ds.logpdf_theta(pj.SingleBendingPowerLaw, th, var, 1e-3, 5.0, 20, is_integrated_power=integ,
                                     basis_function=basis, return_status=True, return_coefs=True)
    Ah, Bh, C, Dd = pj.approx_batch(pj.SingleBendingPowerLaw, th, 1e-3, 5.0, 20, var, is_integrated_power=integ,
                                    basis_function=basis)
    scale = np.abs(Ah).max(axis=1, keepdims=True)
    assert np.max(np.abs(A - Ah) / scale) < 1e-9 and np.max(np.abs(Bc - Bh) / scale) < 1e-9
    ref = ds.logl_batch(Ah, Bh, C, Dd)
    ok = st == 0
    assert ok.mean() > 0.8
    assert relerr(out[ok], ref[ok]) < 1e-8        # log L through either coefficient source
    # double-bending model
    th5 = np.column_stack([th[:, 0], th[:, 1], th[:, 2] * 0.6 + 0.4, th[:, 1] * 30, th[:, 2] + 0.5])
    out5, A5, B5 = ds.logpdf_theta(pj.DoubleBendingPowerLaw, th5, var, 1e-3, 5.0, 20, is_integrated_power=integ,
                                   basis_function=basis, return_coefs=True)
    A5h, _, _, _ = pj.approx_batch(pj.DoubleBendingPowerLaw, th5, 1e-3, 5.0, 20, var, is_integrated_power=integ,
                                   basis_function=basis)
    assert np.max(np.abs(A5 - A5h) / np.abs(A5h).max(axis=1, keepdims=True)) < 1e-9


@pytest.mark.parametrize("basis,integ,nq", [("SHO", True, 1), ("SHO", False, 2), ("DRWCelerite", True, 1)])
def test_device_approx_with_qpo_features(ctx, golden_dir, basis, integ, nq):
    """approx(continuum + QPO features) on the device (src/psd.jl:228-241, 254-261): only (theta, norm, S0, f0, Q, mu, nu)
    cross the boundary; the feature terms have per-draw (c, d) and run in the mixed mode.  Against the oracle's approx +
    logl per draw, and against the host mirror's approx through the coefficient-level entry."""
    rng = np.random.default_rng(60 + nq)
    A_ = np.loadtxt(golden_dir / "simu.txt")
    t, y, yerr = A_[:, 0], A_[:, 1], A_[:, 2]
    f_min, f_max = 1 / (t[-1] - t[0]), 1 / np.min(np.diff(t)) / 2
    B = 37
    th = np.column_stack([rng.uniform(0.0, 1.2, B), np.exp(rng.uniform(np.log(f_min * 4), np.log(f_max / 4), B)), rng.uniform(2.0, 3.8, B)])
    var = np.exp(rng.normal(np.log(np.var(y)), 0.5, B)); nu = rng.uniform(0.7, 1.5, B); mu = np.mean(y) + 0.1 * rng.standard_normal(B)
    qpo = np.stack([np.column_stack([rng.uniform(0.05, 2.0, B), np.exp(rng.uniform(np.log(f_min * 20), np.log(f_max / 5), B)),
                                     rng.uniform(2.0, 30.0, B)]) for _ in range(nq)], axis=1)      # (B, nq, 3): S0, f0, Q
    ds = pj.Dataset(t, y, yerr ** 2, ctx)
    got, st, Ao, Bo = ds.logpdf_theta(pj.SingleBendingPowerLaw, th, var, f_min, f_max, 20, is_integrated_power=integ,
                                      basis_function=basis, mu=mu, nu=nu, qpo=qpo, return_status=True, return_coefs=True)
    J = (20 if basis == "SHO" else 40) + nq
    assert Ao.shape == (B, J) and (st == 0).all()
    ref = np.empty(B); C = np.empty((B, J)); D = np.empty((B, J)); Ah = np.empty((B, J)); Bh = np.empty((B, J))
    for i in range(B):
        a, b, c, d = O.approx(lambda f: O.single_bending_power_law(f, *th[i]), f_min, f_max, 20, var[i], is_integrated_power=integ,
                              basis_function=basis, qpo_features=[tuple(q) for q in qpo[i]])
        ref[i] = O.logl(a, b, c, d, t, y - mu[i], nu[i] * yerr ** 2)
        Ah[i], Bh[i], C[i], D[i] = a, b, c, d
        # the host mirror of approx (the reference-shaped API) gives the same kernel
        psd = pj.SingleBendingPowerLaw(*th[i])
        for q in qpo[i]:
            psd = psd + pj.QPO(*q)
        R = pj.approx(psd, f_min, f_max, 20, var[i], is_integrated_power=integ, basis_function=basis)
        np.testing.assert_allclose(R.a, a, rtol=1e-11); np.testing.assert_allclose(R.d, d, rtol=1e-12)
    assert np.max(np.abs(Ao - Ah) / np.abs(Ah).max(axis=1, keepdims=True)) < 1e-9
    assert np.max(np.abs(Bo - Bh) / np.abs(Ah).max(axis=1, keepdims=True)) < 1e-9
    assert relerr(got, ref) < 1e-9
    host = ds.logl_batch(Ah, Bh, C, D, mu=mu, nu=nu)       # coefficient-level entry, mixed mode on its own detection
    assert relerr(host, ref) < 1e-10
    # a single evaluation and a handful of walkers: the theta entry has no generic per-draw path to fall back to, so the mixed
    # core must run for ANY batch size (the reference evaluates such models one draw at a time; round 2 returned UNSUPPORTED
    # below 16 draws)
    for nb in (1, 8):
        small, sst = ds.logpdf_theta(pj.SingleBendingPowerLaw, th[:nb], var[:nb], f_min, f_max, 20, is_integrated_power=integ,
                                     basis_function=basis, mu=mu[:nb], nu=nu[:nb], qpo=qpo[:nb], return_status=True)
        assert (sst == 0).all() and relerr(small, ref[:nb]) < 1e-9
    # shifted log-flux series on top
    ys = y - y.min() + 1.0
    ds2 = pj.Dataset(t, ys, yerr ** 2, ctx)
    shift = rng.uniform(0.0, 0.5, B)
    got2 = ds2.logpdf_theta(pj.SingleBendingPowerLaw, th, var, f_min, f_max, 20, is_integrated_power=integ, basis_function=basis,
                            mu=mu, nu=nu, shift=shift, qpo=qpo)
    ref2 = np.array([O.logl(Ah[i], Bh[i], C[i], D[i], t, np.log(ys - shift[i]) - mu[i], nu[i] * yerr ** 2 / (ys - shift[i]) ** 2)
                     for i in range(B)])
    assert relerr(got2, ref2) < 1e-9


def test_reference_outputs_ultranest_theta_only(ctx, golden_dir):
    """The reference's stored run once more, now with NOTHING but the sampled parameters crossing the boundary:
    approx, the shift transform and the scan all on the device; 5791 reference log-likelihoods, bar 1e-10."""
    un = np.load(golden_dir / "ultranest_points.npz")
    t, y, yerr, P, ref = un["t"], un["y"], un["yerr"], un["params"], un["logl"]
    f_min, f_max = 1 / (t[-1] - t[0]), 1 / np.min(np.diff(t)) / 2
    ds = pj.Dataset(t, y, yerr ** 2, ctx)
    got, st = ds.logpdf_theta(pj.SingleBendingPowerLaw, P[:, :3], P[:, 3], f_min, f_max, 20, is_integrated_power=False,
                              mu=P[:, 5], nu=P[:, 4], shift=P[:, 6], return_status=True)
    assert (st == 0).all()
    assert relerr(got, ref) < 1e-10


# ---------------------------------------------------------------------------------------------
# mixed mode: a few per-draw terms (QPO features) on top of shared terms
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("J,npd,with_real", [(21, 1, False), (12, 2, False), (9, 1, True), (5, 2, True)])
def test_mixed_shared_and_per_draw_terms(ctx, J, npd, with_real, layout):
    """C, Dd given per draw, but only `npd` columns actually differ between draws (src/psd.jl:254-261: QPO terms
    appended to an approx continuum).  The host entry detects that, keeps the shared table for the common terms and
    builds a per-draw table for the rest; result must equal the oracle and the generic per-draw path."""
    rng = np.random.default_rng(600 + J)
    N, B = 140, 37
    t, y, s2, A, Bc, C, Dd, mu, nu = _random_case(rng, N, J, B)
    C2 = np.broadcast_to(C, (B, J)).copy(); D2 = np.broadcast_to(Dd, (B, J)).copy()
    cols = rng.choice(J, npd, replace=False)
    C2[:, cols] = rng.uniform(0.05, 2.0, (B, npd)); D2[:, cols] = rng.uniform(0.1, 3.0, (B, npd))
    if with_real:   # some shared Exp-like terms (b = d = 0): their sin rows are dropped
        real_cols = [j for j in range(J) if j not in cols][:2]
        Bc[:, real_cols] = 0.0; D2[:, real_cols] = 0.0
    ds = pj.Dataset(t, y, s2, ctx)
    ref = O.logl_batch(A, Bc, C2, D2, t, y, s2, mu, nu, nthreads=8)
    got = ds.logl_batch(A, Bc, C2, D2, mu=mu, nu=nu)
    assert relerr(got, ref) < 1e-11
    if layout == "block":   # small batches with one or two per-draw terms: the windowed kernel with per-draw rows (round 3)
        assert pj._lib.lib().pioran_celerite_config_name(-1).decode() == "block+pd"
    try:
        ctx.set_option("no_mixed", True)
        gen = ds.logl_batch(A, Bc, C2, D2, mu=mu, nu=nu)
    finally:
        ctx.set_option("no_mixed", False)
    assert relerr(gen, ref) < 1e-11
    # per-draw series on top (Y, S2) and the shift transform go through the same path
    Y = y[None, :] + 0.01 * rng.standard_normal((B, N)); S2 = np.broadcast_to(s2, (B, N)) * rng.uniform(0.5, 2, (B, 1))
    got2 = ds.logl_batch(A, Bc, C2, D2, mu=mu, nu=nu, Y=Y, S2=S2)
    ref2 = np.array([O.logl(A[i], Bc[i], C2[i], D2[i], t, Y[i] - mu[i], nu[i] * S2[i]) for i in range(B)])
    assert relerr(got2, ref2) < 1e-11


@pytest.mark.parametrize("J,npd,nreal", [(3, 1, 0), (7, 2, 1), (15, 1, 0), (16, 2, 3), (23, 1, 0), (24, 2, 0), (30, 2, 0), (31, 1, 0), (33, 2, 8)])
def test_block_kernel_per_draw_rows_edges(ctx, J, npd, nreal):
    """The windowed kernel with per-draw rows (celerite_block.hip, BlockPd): every block count NB = 1 .. 4, the per-draw rows inside one
    16-row block and across a block boundary, series of 1 .. 3 windows and a ragged tail, batches on both sides of 256 draws (one /
    two E buffers), per-draw series; against the oracle and against the throughput layouts' mixed mode."""
    rng = np.random.default_rng(7700 + 10 * J + npd)
    for N, B in ((1, 3), (2, 5), (15, 4), (16, 9), (17, 9), (33, 37), (48, 6), (100, 300)):
        t, y, s2, A, Bc, C, Dd, mu, nu = _random_case(rng, N, J, B)
        C2 = np.broadcast_to(C, (B, J)).copy(); D2 = np.broadcast_to(Dd, (B, J)).copy()
        cols = rng.choice(J, npd, replace=False)
        C2[:, cols] = rng.uniform(0.05, 2.0, (B, npd)); D2[:, cols] = rng.uniform(0.1, 3.0, (B, npd))
        real_cols = [j for j in range(J) if j not in cols][:nreal]
        Bc[:, real_cols] = 0.0; D2[:, real_cols] = 0.0
        if B == 1:
            continue
        ds = pj.Dataset(t, y, s2, ctx)
        ref = O.logl_batch(A, Bc, C2, D2, t, y, s2, mu, nu, nthreads=8)
        got, st = ds.logl_batch(A, Bc, C2, D2, mu=mu, nu=nu, return_status=True)
        name = pj._lib.lib().pioran_celerite_config_name(-1).decode()
        if J < 32:   # (beyond, the kernel's LDS record does not fit beside the per-draw block: the latency layout takes it)
            assert name == "block+pd", name
        assert (st == 0).all() and relerr(got, ref) < 1e-11, (N, B)
        if N in (17, 100):
            Y = y[None, :] + 0.01 * rng.standard_normal((B, N)); S2 = np.broadcast_to(s2, (B, N)) * rng.uniform(0.5, 2, (B, 1))
            got2 = ds.logl_batch(A, Bc, C2, D2, mu=mu, nu=nu, Y=Y, S2=S2)
            ref2 = np.array([O.logl(A[i], Bc[i], C2[i], D2[i], t, Y[i] - mu[i], nu[i] * S2[i]) for i in range(B)])
            assert relerr(got2, ref2) < 1e-11
            try:
                ctx.set_option("no_block", True)
                alt = ds.logl_batch(A, Bc, C2, D2, mu=mu, nu=nu)
                assert pj._lib.lib().pioran_celerite_config_name(-1).decode() in ("wide", "scan")
            finally:
                ctx.set_option("no_block", False)
            assert relerr(alt, got) < 1e-11
        ds.close()


def test_mixed_mode_qpo_model_full_size(ctx, full_size):
    """approx(SingleBendingPowerLaw + QPO) at N = 1e4: 20 shared SHO terms + 1 sampled QPO term (J = 21)."""
    t, y, yerr = full_size
    rng = np.random.default_rng(9)
    B = 24
    th = O.synthetic_theta(B, t, y, seed=3)
    f_min, f_max = 1 / (t[-1] - t[0]), 1 / np.min(np.diff(t)) / 2
    rows = []
    for i in range(B):
        PS = pj.SingleBendingPowerLaw(*th[i, :3]) + pj.QPO(rng.uniform(0.01, 0.1), np.exp(rng.uniform(np.log(1e-2), 0.0)), rng.uniform(2, 20))
        R = pj.approx(PS, f_min, f_max, 20, th[i, 3])
        rows.append((R.a, R.b, R.c, R.d))
    A, Bc, C2, D2 = (np.array([r[k] for r in rows]) for k in range(4))
    assert A.shape == (B, 21) and (C2[:, :20] == C2[0, :20]).all() and not (C2[:, 20] == C2[0, 20]).all()
    ds = pj.Dataset(t, y, yerr ** 2, ctx)
    got, st = ds.logl_batch(A, Bc, C2, D2, mu=th[:, 5], nu=th[:, 4], return_status=True)
    assert pj._lib.lib().pioran_celerite_config_name(-1).decode() == "block+pd"   # 24 draws: the windowed kernel with per-draw rows
    ref, rst = O.logl_batch(A, Bc, C2, D2, t, y, yerr ** 2, th[:, 5].copy(), th[:, 4].copy(), nthreads=8, return_status=True)
    ok = rst == 0
    assert ok.sum() >= B // 2 and (st[ok] == 0).all()
    assert relerr(got[ok], ref[ok]) < 1e-8
    try:   # ... and the latency layout's mixed mode on the same inputs
        ctx.set_option("no_block", True)
        alt = ds.logl_batch(A, Bc, C2, D2, mu=th[:, 5], nu=th[:, 4])
    finally:
        ctx.set_option("no_block", False)
    assert relerr(alt[ok], ref[ok]) < 1e-8 and relerr(alt[ok], got[ok]) < 1e-8


def test_in_process_farm_sharding(golden_dir):
    """pioran_farm: several contexts in one process, one thread per device, contiguous ragged shards.  The 1-GPU box
    lists device 0 three times — same code path as three GPUs; checked against reference-computed values."""
    un = np.load(golden_dir / "ultranest_points.npz")
    t, y, yerr, P, ref = un["t"], un["y"], un["yerr"], un["params"][:1000], un["logl"][:1000]
    f_min, f_max = 1 / (t[-1] - t[0]), 1 / np.min(np.diff(t)) / 2
    A, Bc, C, Dd = pj.approx_batch(pj.SingleBendingPowerLaw, P[:, :3], f_min, f_max, 20, P[:, 3], is_integrated_power=False)
    farm = pj.Farm([0, 0, 0], t, y, yerr ** 2)
    assert len(farm) == 3
    got, st = farm.logl_batch(A, Bc, C, Dd, mu=P[:, 5], nu=P[:, 4], shift=P[:, 6], return_status=True)
    assert (st == 0).all() and relerr(got, ref) < 1e-10
    got2 = farm.logl_batch(A[:2], Bc[:2], C, Dd, mu=P[:2, 5], nu=P[:2, 4], shift=P[:2, 6])    # fewer draws than devices
    assert relerr(got2, ref[:2]) < 1e-10
    # per-draw series through the farm (pioran_farm_logl_batch_series; round 3): the same reference values with the shifted
    # log-flux transform done by the caller — what a CustomMean model hands over (examples/ultranest/single_pl_periodicity.jl:115)
    cs = P[:, 6:7]
    Y = np.log(y[None, :] - cs); S2 = yerr[None, :] ** 2 / (y[None, :] - cs) ** 2
    got3, st3 = farm.logl_batch(A, Bc, C, Dd, mu=P[:, 5], nu=P[:, 4], Y=Y, S2=S2, return_status=True)
    assert (st3 == 0).all() and relerr(got3, ref) < 1e-10
    with pytest.raises(ValueError):
        farm.logl_batch(A, Bc, C, Dd, Y=Y, S2=S2, shift=P[:, 6])
    farm.close()


# ---------------------------------------------------------------------------------------------
# posterior mean and simulation (the callers either side of the likelihood)
# ---------------------------------------------------------------------------------------------
def test_predict_reference_cases(ctx, golden_dir):
    """mean(posterior(f(t, s2), y)[, tau]) on the inputs of test/test_scalablegp.jl:134-157 and
    test/test_prediction.jl:49-58 / test_predict_celerite.jl: equal to the oracle's `pred` (1e-10) and, like the
    reference asserts, to the dense prediction."""
    t = np.array([0.0, 3.0, 3.2, 3.4, 45.5, 101.2])
    tx = np.array([0.0, 1.4, 2.3, 3.0, 3.1, 3.2, 3.3, 3.4, 45.5, 101.2, 202.32])
    y = np.array([1.3, 2.2, 4.21, 2.5, 3.3, 5.2]); yerr = np.array([0.1, 0.2, 0.1, 0.1, 0.2, 0.1])
    R = pj.approx(pj.SingleBendingPowerLaw(0.2, 0.02, 3.1), 1e-4, 1e1, 30, 2.31, basis_function="SHO")
    fp = pj.posterior(pj.ScalableGP(1.2, R)(t, yerr ** 2), y)
    for tau in (None, tx):
        tt = t if tau is None else tau
        m = pj.mean(fp, tau, ctx=ctx)
        assert np.isfinite(m).all()
        np.testing.assert_allclose(m, O.predict(R.a, R.b, R.c, R.d, tt, t, y - 1.2, yerr ** 2) + 1.2, rtol=1e-10, atol=1e-12)
        np.testing.assert_allclose(m, O.predict_direct_numpy(R.a, R.b, R.c, R.d, tt, t, y - 1.2, yerr ** 2) + 1.2, rtol=1e-9)
    A = np.loadtxt(golden_dir / "simu.txt")
    t, y, yerr = A[:, 0], A[:, 1], A[:, 2]
    f0, fM = 1 / (t[-1] - t[0]) / 100, 1 / np.min(np.diff(t)) / 2 * 20
    rng = np.random.default_rng(0)
    grids = (t, np.linspace(t.min(), t.max(), 1000), np.linspace(t.min() - 30, t.max() + 30, 1000),
             np.sort(rng.random(1000)) * (t[-1] - t[0]) * 2 + (t[0] - t[-1] / 2))
    kernels = [pj.approx(pj.SingleBendingPowerLaw(0.82, 0.01, 3.3), f0, fM, 20, np.var(y, ddof=1)),
               pj.approx(pj.SingleBendingPowerLaw(0.82, 0.01, 3.3), f0, fM, 20, np.var(y, ddof=1), basis_function="DRWCelerite"),
               pj.Exp(1.0, 2.4), pj.Celerite(3.2, 0.2, 3.0, 0.2)]
    for k in kernels:
        a, b, c, d = (np.real(np.atleast_1d(v)) for v in k.celerite_coefs())
        for tau in grids:
            m = pj.predict(k, tau, t, y, yerr ** 2, ctx=ctx)
            np.testing.assert_allclose(m, O.predict(a, b, c, d, tau, t, y, yerr ** 2), rtol=1e-10, atol=1e-11)
    # unsorted tau: every evaluation time is independent here (the reference requires ascending tau)
    tau = grids[3]; perm = rng.permutation(len(tau))
    k = kernels[0]
    np.testing.assert_allclose(pj.predict(k, tau[perm], t, y, yerr ** 2, ctx=ctx), pj.predict(k, tau, t, y, yerr ** 2, ctx=ctx)[perm],
                               rtol=1e-13, atol=1e-14)


@pytest.mark.parametrize("J,N,B", [(3, 50, 4), (10, 257, 7), (20, 1000, 300), (39, 300, 3)])
def test_predict_random_batches(ctx, J, N, B):
    """B draws at once (more than one 256-draw chunk), mu / nu per draw, every RPL of the factor-storing scan."""
    rng = np.random.default_rng(700 + J)
    t, y, s2, A, Bc, C, Dd, mu, nu = _random_case(rng, N, J, B)
    tau = np.sort(rng.uniform(t[0] - 5, t[-1] + 5, 123))
    tau[:3] = t[[0, N // 2, N - 1]]          # exactly on data points
    tau = np.sort(tau)
    ds = pj.Dataset(t, y, s2, ctx)
    got, st = ds.predict(A, Bc, C, Dd, tau, mu=mu, nu=nu, return_status=True)
    assert (st == 0).all()
    for i in list(range(min(B, 5))) + [B - 1]:
        ref = O.predict(A[i], Bc[i], C, Dd, tau, t, y - mu[i], nu[i] * s2) + mu[i]
        np.testing.assert_allclose(got[i], ref, rtol=1e-10, atol=1e-11)
    # the log-likelihood the same launch computes is still the batch log-likelihood
    ll = ds.logl_batch(A, Bc, C, Dd, mu=mu, nu=nu)
    assert np.isfinite(ll).all()


@pytest.mark.parametrize("J,N,B,basis", [(20, 1000, 40, "SHO"), (3, 333, 5, "SHO"), (12, 4097, 3, "DRWCelerite"), (31, 160, 2, "SHO")])
def test_predict_windowed_path_matches_step_by_step(ctx, J, N, B, basis):
    """6 .. 63 rows: the prediction runs on the windowed kernels (z = -dL/dy of the windowed reverse mode, Q recurrences in
    segments); with `no_block` the same call takes the step-by-step kernels — both against the oracle, and against each other."""
    rng = np.random.default_rng(4100 + J)
    t = np.cumsum(rng.uniform(0.2, 1.5, N)); y = rng.standard_normal(N); s2 = rng.uniform(0.01, 0.1, N)
    th = O.synthetic_theta(B, t, y)
    A, Bc, C, Dd, mu, nu = O.theta_to_coefs(th, t, J, basis)
    tau = np.sort(np.concatenate([rng.uniform(t[0] - 3, t[-1] + 3, 500), t[[0, 127, 128, N - 1]]]))
    ds = pj.Dataset(t, y, s2, ctx)
    lib = pj._lib.lib()
    got, st = ds.predict(A, Bc, C, Dd, tau, mu=mu, nu=nu, return_status=True)
    fam = lib.pioran_celerite_config_name(-1).decode()
    assert (st == 0).all()
    ctx.set_option("no_block", "1")
    try:
        ref_dev = ds.predict(A, Bc, C, Dd, tau, mu=mu, nu=nu)
        fam2 = lib.pioran_celerite_config_name(-1).decode()
    finally:
        ctx.set_option("no_block", "0")
    assert "windowed prediction" in fam and "step-by-step" in fam2, (fam, fam2)
    scale = np.max(np.abs(ref_dev), axis=1, keepdims=True)
    assert np.max(np.abs(got - ref_dev) / scale) < 1e-9
    for i in (0, B - 1):
        ref = O.predict(A[i], Bc[i], C, Dd, tau, t, y - mu[i], nu[i] * s2) + mu[i]
        assert np.max(np.abs(got[i] - ref)) <= 1e-9 * max(1.0, np.max(np.abs(ref)))


@pytest.mark.parametrize("J,N,B", [(12, 1000, 9), (3, 130, 3), (20, 517, 20)])
def test_predict_and_simulate_per_draw_cd_all_draws_in_one_launch(ctx, J, N, B):
    """(c, d) per draw in every term, several draws: one launch of every kernel with per-draw windowed tables — against the draw-by-draw
    path (`no_block`: step-by-step kernels) and the oracle."""
    rng = np.random.default_rng(6100 + J)
    t, y, s2, A, Bc, C, Dd, mu, nu = _random_case(rng, N, J, B, per_draw_cd=True)
    tau = np.sort(np.concatenate([rng.uniform(t[0] - 2, t[-1] + 2, 300), t[[0, N // 2, N - 1]]]))
    ds = pj.Dataset(t, y, s2, ctx)
    lib = pj._lib.lib()
    got, st = ds.predict(A, Bc, C, Dd, tau, mu=mu, nu=nu, return_status=True)
    assert lib.pioran_celerite_config_name(-1).decode() == "block (windowed prediction, per-draw tables)"
    assert (st == 0).all()
    ctx.set_option("no_block", "1")
    try:
        ref_dev = ds.predict(A, Bc, C, Dd, tau, mu=mu, nu=nu)
    finally:
        ctx.set_option("no_block", "0")
    scale = np.max(np.abs(ref_dev), axis=1, keepdims=True)
    assert np.max(np.abs(got - ref_dev) / scale) < 1e-9
    for i in (0, B - 1):
        ref = O.predict(A[i], Bc[i], C[i], Dd[i], tau, t, y - mu[i], nu[i] * s2) + mu[i]
        assert np.max(np.abs(got[i] - ref)) <= 1e-9 * max(1.0, np.max(np.abs(ref)))
    # the simulation likewise
    q = rng.standard_normal((B, N))
    ys = ctx.simulate(A, Bc, C, Dd, t, s2, q)
    assert lib.pioran_celerite_config_name(-1).decode() == "block (windowed simulation, per-draw tables)"
    ctx.set_option("no_block", "1")
    try:
        ys2 = ctx.simulate(A, Bc, C, Dd, t, s2, q)
    finally:
        ctx.set_option("no_block", "0")
    assert np.max(np.abs(ys - ys2) / np.max(np.abs(ys2), axis=1, keepdims=True)) < 1e-9
    for i in (0, B - 1):
        ref = O.sim(A[i], Bc[i], C[i], Dd[i], t, s2, q[i])
        assert np.max(np.abs(ys[i] - ref)) <= 1e-9 * np.max(np.abs(ref))


def test_predict_and_simulate_per_draw_cd(ctx):
    """predict / simulate with (c, d) given per draw [B][J] (QPO / CARMA posterior samples): every draw against the oracle."""
    rng = np.random.default_rng(91)
    t, y, s2, A, Bc, C, Dd, mu, nu = _random_case(rng, 180, 5, 4, per_draw_cd=True)
    ds = pj.Dataset(t, y, s2, ctx)
    tau = np.sort(rng.uniform(t[0] - 2, t[-1] + 2, 41))
    pm = ds.predict(A, Bc, C, Dd, tau, mu=mu, nu=nu)
    for i in range(4):
        ref = O.predict(A[i], Bc[i], C[i], Dd[i], tau, t, y - mu[i], nu[i] * s2) + mu[i]
        np.testing.assert_allclose(pm[i], ref, rtol=1e-9, atol=1e-10)
    q = rng.standard_normal((4, 180))
    ys = ctx.simulate(A, Bc, C, Dd, t, s2, q)
    for i in range(4):
        np.testing.assert_allclose(ys[i], O.sim(A[i], Bc[i], C[i], Dd[i], t, s2, q[i]), rtol=1e-9, atol=1e-10)


def test_predict_full_size(ctx, full_size):
    """N = 1e4 (BASELINE config shape), M = 2000: against the oracle to 1e-8 and self-consistency at the data."""
    t, y, yerr = full_size
    th = O.synthetic_theta(6, t, y)
    A, Bc, C, Dd, mu, nu = O.theta_to_coefs(th, t, 20, "SHO")
    tau = np.sort(np.random.default_rng(1).uniform(t[0], t[-1], 2000))
    ds = pj.Dataset(t, y, yerr ** 2, ctx)
    got = ds.predict(A, Bc, C, Dd, tau, mu=mu, nu=nu)
    for i in range(2):
        ref = O.predict(A[i], Bc[i], C, Dd, tau, t, y - mu[i], nu[i] * yerr ** 2) + mu[i]
        assert np.max(np.abs(got[i] - ref)) <= 1e-8 * max(1.0, np.max(np.abs(ref)))


@pytest.mark.parametrize("J,N,B", [(32, 90, 3), (40, 130, 2), (47, 61, 2), (48, 77, 3), (56, 40, 2), (64, 100, 2), (71, 50, 2)])
def test_predict_and_simulate_64_to_143_rows(ctx, J, N, B):
    """64 .. 143 rows (past the windowed kernels): posterior mean and simulation from the factor the LEAN latency kernel stores
    (celerite_wide2_kernel<RPL, false, 1 | 2>, round 4).  Before: 95 rows at most, on the round-1 kernel, which stays behind `no_wide2`.
    The reference benchmark grid's largest model (j = 64: 128 rows) is in; past 128 rows the prediction's sweeps hold three rows per lane."""
    rng = np.random.default_rng(4200 + J)
    t, y, s2, A, Bc, C, Dd, mu, nu = _random_case(rng, N, J, B)
    tau = np.sort(np.concatenate([rng.uniform(t[0] - 5, t[-1] + 5, 60), t[[0, N // 2, N - 1]]]))
    ds = pj.Dataset(t, y, s2, ctx)
    q = rng.standard_normal((B, N))
    ys = ctx.simulate(A, Bc, C, Dd, t, s2, q)
    assert pj._lib.lib().pioran_celerite_config_name(-1).decode() == "wide (step-by-step simulation)"
    for i in range(B):
        ref = O.sim(A[i], Bc[i], C, Dd, t, s2, q[i])
        assert np.max(np.abs(ys[i] - ref)) <= 1e-10 * np.max(np.abs(ref))
    got, st = ds.predict(A, Bc, C, Dd, tau, mu=mu, nu=nu, return_status=True)
    assert (st == 0).all() and pj._lib.lib().pioran_celerite_config_name(-1).decode() == "wide (step-by-step prediction)"
    for i in range(B):
        ref = O.predict(A[i], Bc[i], C, Dd, tau, t, y - mu[i], nu[i] * s2) + mu[i]
        np.testing.assert_allclose(got[i], ref, rtol=1e-9, atol=1e-10)
    if 2 * J <= 95:
        try:
            ctx.set_option("no_wide2", True)
            old = ds.predict(A, Bc, C, Dd, tau, mu=mu, nu=nu)
            ys_old = ctx.simulate(A, Bc, C, Dd, t, s2, q)
        finally:
            ctx.set_option("no_wide2", False)
        np.testing.assert_allclose(got, old, rtol=1e-11, atol=1e-12)
        assert np.max(np.abs(ys - ys_old)) <= 1e-12 * np.max(np.abs(ys_old))


def test_simulate_matches_oracle(ctx, golden_dir):
    """simulate / rand: y = L D^(1/2) q for the same normals q as the oracle's `sim` (src/celerite_solver.jl:515-549)."""
    A = np.loadtxt(golden_dir / "simu.txt")
    t, yerr = A[:, 0], A[:, 2]
    f0, fM = 1 / (t[-1] - t[0]) / 100, 1 / np.min(np.diff(t)) / 2 * 20
    rng = np.random.default_rng(3)
    for basis in ("SHO", "DRWCelerite"):
        R = pj.approx(pj.SingleBendingPowerLaw(0.82, 0.01, 3.3), f0, fM, 20, 1.0, basis_function=basis)
        q = rng.standard_normal((5, len(t)))
        scale = np.array([1.0, 2.0, 0.5, 1.5, 0.1])[:, None]
        ys = ctx.simulate(scale * R.a, scale * R.b, R.c, R.d, t, yerr ** 2, q)
        for i in range(5):
            ref = O.sim(scale[i] * R.a, scale[i] * R.b, R.c, R.d, t, yerr ** 2, q[i])
            assert np.max(np.abs(ys[i] - ref)) <= 1e-10 * np.max(np.abs(ref)), basis
    # reference-shaped entry: rand(rng, f(t, s2)) adds the mean; same generator state -> same normals
    R = pj.approx(pj.SingleBendingPowerLaw(0.82, 0.01, 3.3), f0, fM, 20, 1.0)
    y1 = pj.rand(np.random.default_rng(9), pj.ScalableGP(0.7, R)(t, yerr ** 2), ctx=ctx)
    ref = O.sim(R.a, R.b, R.c, R.d, t, yerr ** 2, np.random.default_rng(9).standard_normal(len(t))) + 0.7
    assert np.max(np.abs(y1 - ref)) <= 1e-10 * np.max(np.abs(ref))
    # more draws than one chunk, and the sample covariance of many draws approaches K
    tt = np.cumsum(np.random.default_rng(4).uniform(0.2, 1.0, 24)); s2 = np.full(24, 0.05)
    a, b, c, d = np.array([1.0, 0.4]), np.array([0.2, 0.0]), np.array([0.3, 1.0]), np.array([1.1, 0.0])
    B = 4000
    q = np.random.default_rng(5).standard_normal((B, 24))
    ys = ctx.simulate(np.tile(a, (B, 1)), np.tile(b, (B, 1)), c, d, tt, s2, q)
    K = np.array([[O.kappa(a, b, c, d, abs(ti - tj)) for tj in tt] for ti in tt]) + np.diag(s2)
    assert np.max(np.abs(ys.T @ ys / B - K)) < 0.15 * np.max(np.abs(K))
    assert np.max(np.abs(ys[7] - O.sim(a, b, c, d, tt, s2, q[7]))) < 1e-12


@pytest.mark.parametrize("J,nreal,N,B,per_draw_cd", [(1, 0, 300, 3, False), (1, 1, 77, 2, False), (2, 0, 1000, 5, False), (2, 1, 129, 3, False), (2, 2, 40, 2, False),
                                                     (1, 0, 90, 3, True), (2, 0, 150, 4, True)])
def test_predict_and_simulate_fewer_than_six_rows_on_the_windowed_kernels(ctx, J, nreal, N, B, per_draw_cd):
    """1 .. 4 rows (the reference grid's j = 2): prediction and simulation run on the windowed factorisation since late round 4 (N = 1e4, four
    draws: 11.3 -> 2.4 ms and 4.7 -> 2.5 ms) — against the step-by-step kernels (`no_block`) and the oracle; shared and per-draw (c, d)."""
    rng = np.random.default_rng(6600 + 10 * J + nreal + N)
    t, y, s2, A, Bc, C, Dd, mu, nu = _random_case(rng, N, J, B, per_draw_cd=per_draw_cd)
    if nreal:
        Bc[:, :nreal] = 0.0; Dd[..., :nreal] = 0.0
    tau = np.sort(np.concatenate([rng.uniform(t[0] - 2, t[-1] + 2, 200), t[[0, N // 2, N - 1]]]))
    q = rng.standard_normal((B, N))
    ds = pj.Dataset(t, y, s2, ctx)
    name = lambda: pj._lib.lib().pioran_celerite_config_name(-1).decode()
    got, st = ds.predict(A, Bc, C, Dd, tau, mu=mu, nu=nu, return_status=True); fam_p = name()
    ys = ctx.simulate(A, Bc, C, Dd, t, s2, q); fam_s = name()
    assert "windowed prediction" in fam_p and "windowed simulation" in fam_s and (st == 0).all(), (fam_p, fam_s)
    ctx.set_option("no_block", "1")
    try:
        got2 = ds.predict(A, Bc, C, Dd, tau, mu=mu, nu=nu); fam_p2 = name()
        ys2 = ctx.simulate(A, Bc, C, Dd, t, s2, q); fam_s2 = name()
    finally:
        ctx.set_option("no_block", "0")
    assert "step-by-step" in fam_p2 and "step-by-step" in fam_s2
    assert np.max(np.abs(got - got2) / np.max(np.abs(got2), axis=1, keepdims=True)) < 1e-9
    assert np.max(np.abs(ys - ys2) / np.max(np.abs(ys2), axis=1, keepdims=True)) < 1e-9
    for i in range(B):
        c_i, d_i = (C[i], Dd[i]) if per_draw_cd else (C, Dd)
        ref = O.predict(A[i], Bc[i], c_i, d_i, tau, t, y - mu[i], nu[i] * s2) + mu[i]
        assert np.max(np.abs(got[i] - ref)) <= 1e-9 * max(1.0, np.max(np.abs(ref)))
        refs = O.sim(A[i], Bc[i], c_i, d_i, t, s2, q[i])
        assert np.max(np.abs(ys[i] - refs)) <= 1e-9 * np.max(np.abs(refs))


@pytest.mark.parametrize("J,N,B,basis", [(20, 1000, 40, "SHO"), (3, 333, 5, "SHO"), (12, 4097, 3, "DRWCelerite"), (31, 160, 2, "SHO")])
def test_simulate_windowed_path_matches_step_by_step(ctx, J, N, B, basis):
    """6 .. 63 rows: the simulation runs on the windowed factorisation (L applied window by window); with `no_block` the same call
    takes the step-by-step kernel — both against the oracle's `sim` on the same normals, and against each other."""
    rng = np.random.default_rng(5200 + J)
    t = np.cumsum(rng.uniform(0.2, 1.5, N)); y = rng.standard_normal(N); s2 = rng.uniform(0.01, 0.1, N)
    th = O.synthetic_theta(B, t, y)
    A, Bc, C, Dd, mu, nu = O.theta_to_coefs(th, t, J, basis)
    q = rng.standard_normal((B, N))
    lib = pj._lib.lib()
    ys = ctx.simulate(A, Bc, C, Dd, t, s2, q)
    fam = lib.pioran_celerite_config_name(-1).decode()
    ctx.set_option("no_block", "1")
    try:
        ys2 = ctx.simulate(A, Bc, C, Dd, t, s2, q)
        fam2 = lib.pioran_celerite_config_name(-1).decode()
    finally:
        ctx.set_option("no_block", "0")
    assert "windowed simulation" in fam and "step-by-step" in fam2, (fam, fam2)
    scale = np.max(np.abs(ys2), axis=1, keepdims=True)
    assert np.isfinite(ys).all() and np.max(np.abs(ys - ys2) / scale) < 1e-9
    for i in (0, B - 1):
        ref = O.sim(A[i], Bc[i], C, Dd, t, s2, q[i])
        assert np.max(np.abs(ys[i] - ref)) <= 1e-9 * np.max(np.abs(ref))


def test_predict_cov_reference_cases(ctx, golden_dir):
    """cov / std of the posterior (src/direct_solver.jl:28-69 through src/scalable_GP.jl:73-104) on the inputs of
    test/test_scalablegp.jl:134-175: finite, positive definite, equal to the numpy restatement of predict_cov."""
    t = np.array([0.0, 3.0, 3.2, 3.4, 45.5, 101.2])
    tx = np.array([0.0, 1.4, 2.3, 3.0, 3.1, 3.2, 3.3, 3.4, 45.5, 101.2, 202.32])
    y = np.array([1.3, 2.2, 4.21, 2.5, 3.3, 5.2]); yerr = np.array([0.1, 0.2, 0.1, 0.1, 0.2, 0.1])
    R = pj.approx(pj.SingleBendingPowerLaw(0.2, 0.02, 3.1), 1e-4, 1e1, 30, 2.31, basis_function="SHO")
    fp = pj.posterior(pj.ScalableGP(1.2, R)(t, yerr ** 2), y)
    for tau in (None, tx):
        tt = t if tau is None else tau
        K = pj.cov(fp, tau, ctx=ctx)
        ref = O.predict_cov_numpy(R.a, R.b, R.c, R.d, tt, t, yerr ** 2)
        assert np.isfinite(K).all() and np.allclose(K, K.T, rtol=0, atol=0)
        scale = np.max(np.abs(ref))
        assert np.max(np.abs(K - ref)) <= 1e-9 * scale
        assert np.linalg.eigvalsh(K).min() > -1e-9 * scale                      # isposdef up to rounding, like the reference's checks
        np.testing.assert_allclose(pj.std(fp, tau, ctx=ctx), np.sqrt(np.diag(ref)), rtol=1e-6, atol=1e-7)
    # a larger case crossing several 64-blocks on both sides: N = 489 data points, M = 300 new times
    A = np.loadtxt(golden_dir / "simu.txt")
    t, y, yerr = A[:, 0], A[:, 1], A[:, 2]
    f0, fM = 1 / (t[-1] - t[0]) / 100, 1 / np.min(np.diff(t)) / 2 * 20
    R = pj.approx(pj.SingleBendingPowerLaw(0.82, 0.01, 3.3), f0, fM, 20, np.var(y, ddof=1))
    tau = np.linspace(t.min() - 30, t.max() + 30, 300)
    K = pj.predict_cov(R, tau, t, yerr ** 2, ctx=ctx)
    ref = O.predict_cov_numpy(R.a, R.b, R.c, R.d, tau, t, yerr ** 2)
    assert np.max(np.abs(K - ref)) <= 1e-9 * np.max(np.abs(ref))
    # posterior draws: right shape, centred on the posterior mean
    fp = pj.posterior(pj.ScalableGP(0.0, R)(t, yerr ** 2), y)
    draws = pj.rand_posterior(np.random.default_rng(2), fp, tau, 200, ctx=ctx)
    assert draws.shape == (300, 200)
    m = pj.mean(fp, tau, ctx=ctx)
    assert np.max(np.abs(draws.mean(axis=1) - m)) < 6 * np.sqrt(np.max(np.diag(K)) / 200) + 1e-6
    # K(t,t) + diag(sigma2) not positive definite -> LinAlgError like the reference's PosDefException
    with pytest.raises(np.linalg.LinAlgError):
        pj.predict_cov(pj.Celerite(-1.0, 0.0, 0.5, 0.0), tau[:5], t[:70], np.zeros(70), ctx=ctx)


# ---------------------------------------------------------------------------------------------
# gradient of log L by reverse mode through the recurrence
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("J,N,B", [(3, 40, 2), (7, 64, 3), (10, 257, 3), (20, 500, 2), (30, 129, 2), (39, 100, 2), (4, 1, 1), (9, 2, 2),
                                   (9, 3, 2), (9, 6, 2), (32, 45, 2), (40, 70, 2), (47, 37, 1),    # 40, 47: 80 / 94 rows (SHO-40 is the dense configuration's model)
                                   (48, 50, 2), (55, 33, 1), (56, 20, 2), (64, 40, 2), (71, 37, 1)])   # 96 .. 142 rows (round 4; j = 64: the reference grid's largest)
def test_gradient_matches_complex_step(ctx, J, N, B):
    """dlogL/d(a_j, b_j, c_j, d_j, mu, nu, y_n, sigma2_n) against the complex-step derivatives of the oracle (exact to
    rounding): every RPL of the adjoint kernel, every prologue / tail length of its pipelines, series shorter and longer
    than one checkpoint segment (16 steps at these N)."""
    rng = np.random.default_rng(800 + J + N)
    t, y, s2, A, Bc, C, Dd, mu, nu = _random_case(rng, N, J, B)
    ds = pj.Dataset(t, y, s2, ctx)
    g = ds.logl_grad(A, Bc, C, Dd, mu=mu, nu=nu, series_grad=True)
    if 32 <= J <= 47:      # 64 .. 95 rows: the lean reverse pass (round 4) is the default; the round-1 kernels stay behind `no_wide2`
        try:
            ctx.set_option("no_wide2", True)
            g1 = ds.logl_grad(A, Bc, C, Dd, mu=mu, nu=nu, series_grad=True)
        finally:
            ctx.set_option("no_wide2", False)
        for k in ("grad_a", "grad_b", "grad_c", "grad_d", "grad_mu", "grad_nu", "grad_y", "grad_sigma2"):
            assert np.max(np.abs(g[k] - g1[k])) <= 1e-10 * (1 + np.max(np.abs(g1[k]))), k
    ref_l = O.logl_batch(A, Bc, C, Dd, t, y, s2, mu, nu)
    assert relerr(g["logl"], ref_l) < 1e-11 and (g["status"] == 0).all()
    assert (g["logl"] == ds.logl_batch(A, Bc, C, Dd, mu=mu, nu=nu)).all() or relerr(g["logl"], ds.logl_batch(A, Bc, C, Dd, mu=mu, nu=nu)) < 1e-12
    for i in range(B):
        ref = O.logl_grad(A[i], Bc[i], C, Dd, t, y - mu[i], nu[i] * s2, series=N <= 129, cd=True)
        sa = 1e-9 * (1 + np.max(np.abs(ref["grad_a"]))); sb = 1e-9 * (1 + np.max(np.abs(ref["grad_b"])))
        assert np.max(np.abs(g["grad_a"][i] - ref["grad_a"])) <= sa
        assert np.max(np.abs(g["grad_b"][i] - ref["grad_b"])) <= sb
        assert np.max(np.abs(g["grad_c"][i] - ref["grad_c"])) <= 1e-9 * (1 + np.max(np.abs(ref["grad_c"])))
        assert np.max(np.abs(g["grad_d"][i] - ref["grad_d"])) <= 1e-9 * (1 + np.max(np.abs(ref["grad_d"])))
        gm = O.logl_dir(A[i], Bc[i], C, Dd, t, y - mu[i], nu[i] * s2, dy=-np.ones(N))
        gn = O.logl_dir(A[i], Bc[i], C, Dd, t, y - mu[i], nu[i] * s2, ds2=s2)
        assert abs(g["grad_mu"][i] - gm) <= 1e-9 * (1 + abs(gm)) and abs(g["grad_nu"][i] - gn) <= 1e-9 * (1 + abs(gn))
        if N <= 129:
            # the data set holds (y, s2): dL/dy_n is the oracle's derivative w.r.t. (y - mu)_n, dL/ds2_n carries nu
            assert np.max(np.abs(g["grad_y"][i] - ref["grad_y"])) <= 1e-9 * (1 + np.max(np.abs(ref["grad_y"])))
            assert np.max(np.abs(g["grad_sigma2"][i] - nu[i] * ref["grad_sigma2"])) <= 1e-9 * (1 + np.max(np.abs(ref["grad_sigma2"])))


@pytest.mark.parametrize("J,N,B,nreal", [(1, 40, 3, 0), (1, 33, 2, 1), (2, 50, 3, 0), (2, 17, 2, 2), (2, 100, 2, 1), (3, 40, 3, 0), (5, 16, 2, 0), (7, 33, 4, 2), (8, 100, 3, 1), (12, 17, 2, 0), (15, 130, 5, 0), (20, 257, 3, 0),
                                         (23, 48, 2, 0), (24, 70, 2, 0), (30, 95, 2, 5), (31, 64, 3, 0)])
def test_windowed_gradient_matches_complex_step(ctx, J, N, B, nreal):
    """d log L / d(a_j, b_j, mu, nu) by the windowed reverse mode (celerite_block_adjoint_kernel; what a sampler of an approx-based
    model asks for: (c, d) fixed by the spectral grid): against the complex-step derivatives of the oracle and against the
    step-by-step adjoint kernels; every block count NB = 1 .. 4, ragged last windows, one-row terms; the value is bit-identical to the
    windowed forward kernel's."""
    rng = np.random.default_rng(8800 + J + N)
    t, y, s2, A, Bc, C, Dd, mu, nu = _random_case(rng, N, J, B)
    Bc[:, :nreal] = 0.0; Dd[:nreal] = 0.0
    ds = pj.Dataset(t, y, s2, ctx)
    g = ds.logl_grad(A, Bc, C, Dd, mu=mu, nu=nu)
    assert pj._lib.lib().pioran_celerite_config_name(-1).decode() == "block (windowed gradient)"
    g0 = ds.logl_grad(A, Bc, C, Dd, mu=mu, nu=nu, cd_grad=False)          # the variant without d/d(c, d)
    assert g0["grad_c"] is None and np.array_equal(g0["logl"], g["logl"])
    for key in ("grad_a", "grad_b", "grad_mu", "grad_nu"):
        assert np.max(np.abs(g0[key] - g[key])) <= 1e-12 * (1 + np.max(np.abs(g[key])))
    if 2 * J - nreal < 5:      # (the VALUE of so few rows runs on the throughput layout unless asked: short series)
        ctx.set_option("scan_config", "block")
    try:
        val = ds.logl_batch(A, Bc, C, Dd, mu=mu, nu=nu)
    finally:
        ctx.set_option("scan_config", None)
    assert pj._lib.lib().pioran_celerite_config_name(-1).decode() == "block"
    assert (g["logl"] == val).all() and (g["status"] == 0).all()
    assert relerr(g["logl"], O.logl_batch(A, Bc, C, Dd, t, y, s2, mu, nu)) < 1e-11
    try:
        ctx.set_option("no_block", True)
        old = ds.logl_grad(A, Bc, C, Dd, mu=mu, nu=nu)
        assert pj._lib.lib().pioran_celerite_config_name(-1).decode() == "wide (step-by-step gradient)"
    finally:
        ctx.set_option("no_block", False)
    for i in range(B):
        ref = O.logl_grad(A[i], Bc[i], C, Dd, t, y - mu[i], nu[i] * s2, cd=True)
        for key in ("grad_a", "grad_b", "grad_c", "grad_d"):
            tol = 1e-9 * (1 + np.max(np.abs(ref[key])))
            assert np.max(np.abs(g[key][i] - ref[key])) <= tol, (key, i)
            assert np.max(np.abs(g[key][i] - old[key][i])) <= tol, (key, i)
        gm = O.logl_dir(A[i], Bc[i], C, Dd, t, y - mu[i], nu[i] * s2, dy=-np.ones(N))
        gn = O.logl_dir(A[i], Bc[i], C, Dd, t, y - mu[i], nu[i] * s2, ds2=s2)
        assert abs(g["grad_mu"][i] - gm) <= 1e-9 * (1 + abs(gm)) and abs(g["grad_nu"][i] - gn) <= 1e-9 * (1 + abs(gn))
    # series gradients (what a per-draw data transform chains through) from the same kernels
    gs = ds.logl_grad(A, Bc, C, Dd, mu=mu, nu=nu, cd_grad=False, series_grad=True)
    assert pj._lib.lib().pioran_celerite_config_name(-1).decode() == "block (windowed gradient)"
    # (another instantiation of the reverse kernel; its per-term sums are LDS atomics, whose order is not fixed: equal to rounding)
    assert (gs["logl"] == val).all()
    for key in ("grad_a", "grad_mu"):
        assert np.max(np.abs(gs[key] - g[key])) <= 1e-13 * (1 + np.max(np.abs(g[key]))), key
    for i in range(min(B, 2)):
        ref = O.logl_grad(A[i], Bc[i], C, Dd, t, y - mu[i], nu[i] * s2, series=True)
        assert np.max(np.abs(gs["grad_y"][i] - ref["grad_y"])) <= 1e-9 * (1 + np.max(np.abs(ref["grad_y"])))
        assert np.max(np.abs(gs["grad_sigma2"][i] - nu[i] * ref["grad_sigma2"])) <= 1e-9 * (1 + np.max(np.abs(ref["grad_sigma2"])))


# ---- time-parallel evaluation of a handful of draws (celerite_tp.hip, round 5) -----------------------------------------------------------------
@pytest.mark.parametrize("J,N,B,nreal,nseg", [(1, 100, 1, 0, 2), (1, 100, 1, 1, 2), (2, 200, 1, 0, 4), (3, 500, 2, 1, 5), (6, 300, 3, 0, 0), (8, 640, 2, 0, 7),
                                              (9, 400, 4, 4, 6), (12, 2000, 8, 3, 0), (20, 1000, 2, 0, 8), (20, 777, 1, 0, 3), (21, 500, 1, 20, 5),
                                              (24, 640, 2, 0, 4), (5, 64, 1, 0, 4), (4, 333, 64, 0, 3), (32, 700, 2, 0, 5), (30, 300, 1, 0, 3), (40, 450, 2, 20, 4),
                                              (36, 260, 1, 9, 2)])
def test_time_parallel_family_vs_oracle(ctx, J, N, B, nreal, nseg):
    """The state-space / associative-element form (segments of the series on different CUs), forced at every shape it takes: one wavefront per
    segment (up to 16 state rows) and four (up to 64: DRWCelerite-20 is 20 two-row and 20 one-row terms), one-row terms packed in pairs, padded row counts, segment counts that do not divide N, the
    shortest segments (16 steps), 64 draws.  Against the oracle at 1e-11 (the prototype's study: profiles/r05_time_parallel_proto.txt)."""
    rng = np.random.default_rng(3300 + J + N)
    t, y, s2, A, Bc, C, Dd, mu, nu = _random_case(rng, N, J, B)
    Dd = np.maximum(Dd, 0.05)
    Bc[:, :nreal] = 0.0; Dd[:nreal] = 0.0
    ds = pj.Dataset(t, y, s2, ctx)
    ref = O.logl_batch(A, Bc, C, Dd, t, y, s2, mu, nu, nthreads=8)
    try:
        ctx.set_option("scan_config", "tp"); ctx.set_option("tp_segments", nseg)
        got, st = ds.logl_batch(A, Bc, C, Dd, mu=mu, nu=nu, return_status=True)
        assert pj._lib.lib().pioran_celerite_config_name(-1).decode() == "tp"
        one = ds.logl_batch(A[:1], Bc[:1], C, Dd)                 # no mu, no nu
    finally:
        ctx.set_option("scan_config", None); ctx.set_option("tp_segments", 0)
    assert relerr(got, ref) < 1e-11 and (st == 0).all()
    assert relerr(one, O.logl_batch(A[:1], Bc[:1], C, Dd, t, y, s2, None, None)) < 1e-11


def test_time_parallel_dispatch_reference_values_and_flagged_draws(ctx, golden_dir):
    """(i) The automatic choice: up to 8 draws (64 at up to four state rows), up to 16 state rows, long series; "no_tp" and everything else stay on
    the serial-chain kernels.
    (ii) Values the REFERENCE computed (stored ultranest run, N = 242, SHO-20: 40 rows, four wavefronts per segment), forced.
    (iii) A draw that is not positive definite: the status and the log |D_n| semantics of the other families (src/celerite_solver.jl:126, 140).
    (iv) Per-draw series (Y, S2)."""
    name = lambda: pj._lib.lib().pioran_celerite_config_name(-1).decode()
    rng = np.random.default_rng(515)
    N, J, B = 8192, 2, 3
    t, y, s2, A, Bc, C, Dd, mu, nu = _random_case(rng, N, J, B)
    ds = pj.Dataset(t, y, s2, ctx)
    ref = O.logl_batch(A, Bc, C, Dd, t, y, s2, mu, nu, nthreads=8)
    got = ds.logl_batch(A, Bc, C, Dd, mu=mu, nu=nu)
    assert name() == "tp" and relerr(got, ref) < 1e-11
    try:
        ctx.set_option("no_tp", True)
        chain = ds.logl_batch(A, Bc, C, Dd, mu=mu, nu=nu)
        assert name() != "tp" and relerr(chain, ref) < 1e-11
    finally:
        ctx.set_option("no_tp", False)
    A9 = np.tile(A, (3, 1)); B9 = np.tile(Bc, (3, 1))
    g9 = ds.logl_batch(A9, B9, C, Dd, mu=np.tile(mu, 3), nu=np.tile(nu, 3))
    assert name() == "tp" and np.array_equal(g9[:3], got)            # up to 64 draws at up to four state rows from 4096 steps on
    ds.logl_batch(np.tile(A, (22, 1)), np.tile(Bc, (22, 1)), C, Dd)
    assert name() != "tp"                                           # 66 draws
    ds2 = pj.Dataset(t[:900], y[:900], s2[:900], ctx)
    ds2.logl_batch(A, Bc, C, Dd)
    assert name() != "tp"                                           # a short series
    rng2 = np.random.default_rng(516)
    t8, y8, s8, A8, B8, C8, D8, mu8, nu8 = _random_case(rng2, 5000, 7, 2)      # fourteen state rows: from 6144 steps on
    ds3 = pj.Dataset(t8, y8, s8, ctx)
    g14 = ds3.logl_batch(A8, B8, C8, D8)
    assert name() == "tp"                                           # (up to two draws: the boundary phase as a scan, from 1024 steps on)
    assert relerr(g14, O.logl_batch(A8, B8, C8, D8, t8, y8, s8, None, None)) < 1e-11
    g14b = ds3.logl_batch(np.tile(A8, (2, 1)), np.tile(B8, (2, 1)), C8, D8)
    assert name() == "tp" and relerr(g14b[:2], g14) < 1e-11         # four draws: the scan at 64 segments (3 .. 32 draws: by the model of tp_dispatch)
    ds3.logl_batch(np.tile(A8, (17, 1)), np.tile(B8, (17, 1)), C8, D8)
    assert name() != "tp"                                           # 34 draws
    g6 = ds3.logl_batch(np.tile(A8[:, :6], (2, 1)), np.tile(B8[:, :6], (2, 1)), C8[:6], D8[:6])[:2]
    assert name() == "tp"                                           # twelve state rows: from 4096
    assert relerr(g6, O.logl_batch(A8[:, :6], B8[:, :6], C8[:6], D8[:6], t8, y8, s8, None, None)) < 1e-11
    # 17 .. 64 state rows: long series only (the boundary solves are R^3 each)
    t9, y9, s9, A9_, B9_, C9, D9, mu9, nu9 = _random_case(np.random.default_rng(517), 7000, 20, 4)
    ds9 = pj.Dataset(t9, y9, s9, ctx)
    g9_ = ds9.logl_batch(A9_[:2, :12], B9_[:2, :12], C9[:12], D9[:12], mu=mu9[:2], nu=nu9[:2])       # 24 state rows: from 4096 steps on
    assert name() == "tp" and relerr(g9_, O.logl_batch(A9_[:2, :12], B9_[:2, :12], C9[:12], D9[:12], t9, y9, s9, mu9[:2], nu9[:2], nthreads=8)) < 1e-10
    g40 = ds9.logl_batch(A9_, B9_, C9, D9)
    assert name() == "tp" and relerr(g40, O.logl_batch(A9_, B9_, C9, D9, t9, y9, s9, None, None, nthreads=8)) < 1e-10   # 40 state rows, four draws: the scan
    ds9.logl_batch(np.tile(A9_, (3, 1)), np.tile(B9_, (3, 1)), C9, D9)
    assert name() != "tp"                                           # twelve draws of 40 rows: the serial chains
    ds9.logl_batch(A9_[:, :16], B9_[:, :16], C9[:16], D9[:16])
    assert name() == "tp"                                           # 32 state rows, four draws: from 6144
    ds9.close()
    # (iv) per-draw series
    Y = y[None, :] + 0.01 * rng.standard_normal((B, N)); S2 = s2[None, :] * rng.uniform(0.8, 1.2, (B, 1))
    gy = ds.logl_batch(A, Bc, C, Dd, mu=mu, nu=nu, Y=Y, S2=S2)
    assert name() == "tp"
    ry = np.array([O.logl(A[i], Bc[i], C, Dd, t, Y[i] - mu[i], nu[i] * S2[i]) for i in range(B)])
    assert relerr(gy, ry) < 1e-11
    # (iii)
    A2 = A.copy(); A2[1, 0] = -40.0
    gb, sb = ds.logl_batch(A2, Bc, C, Dd, mu=mu, nu=nu, return_status=True)
    assert name() == "tp"
    rb, rs = O.logl_batch(A2, Bc, C, Dd, t, y, s2, mu, nu, return_status=True)
    assert sb[1] != 0 and rs[1] != 0 and sb[0] == 0 and sb[2] == 0
    assert relerr(gb[[0, 2]], rb[[0, 2]]) < 1e-11
    assert (np.isnan(gb[1]) and np.isnan(rb[1])) or abs(gb[1] - rb[1]) <= 1e-6 * abs(rb[1])
    # (ii)
    un = np.load(golden_dir / "ultranest_points.npz")
    sys.path.insert(0, str(Path(__file__).resolve().parent))
    from test_oracle import _un_inputs
    try:
        ctx.set_option("scan_config", "tp")
        worst = 0.0
        for i in np.linspace(0, len(un["logl"]) - 1, 40).astype(int):
            a, b, c, d, tt, yy, ss = _un_inputs(un, i)
            dsu = pj.Dataset(tt, yy, ss, ctx)
            g = dsu.logl_batch(a[None, :], b[None, :], c, d)[0]
            assert name() == "tp"
            worst = max(worst, abs(g - un["logl"][i]) / abs(un["logl"][i]))
            dsu.close()
    finally:
        ctx.set_option("scan_config", None)
    assert worst < 1e-10, worst


@pytest.mark.parametrize("J,N,B,nreal,nseg", [(3, 500, 1, 1, 2), (4, 640, 2, 0, 3), (8, 2000, 1, 0, 17), (8, 4096, 2, 0, 128), (12, 3000, 2, 3, 0), (11, 1500, 1, 1, 33),
                                              (20, 10000, 1, 0, 0), (20, 4096, 2, 0, 256), (24, 3100, 1, 0, 64), (25, 1800, 2, 22, 9), (9, 1111, 4, 0, 16),
                                              (28, 900, 1, 0, 5), (30, 1500, 2, 0, 33), (32, 4200, 1, 0, 0), (40, 2000, 1, 20, 64), (36, 700, 2, 9, 2),
                                              (2, 3000, 1, 0, 0), (2, 2500, 2, 1, 16)])
def test_time_parallel_boundary_scan_vs_walk_and_oracle(ctx, J, N, B, nreal, nseg):
    """Round 6: the boundary phase as a Kogge-Stone scan over the segments' elements (tp_combine_kernel), 5 .. 48 state rows padded to a multiple of 8,
    (three and four rows — the reference grid's j = 2 — from 2048 steps on) against the boundary walk (tp_scan = 0) and the oracle: segment counts that are not powers of two, 2 segments (one level), the cap of 256, one and
    two draws, four when forced (tp_scan = 1), one-row terms, padded rows; 49 .. 64 rows (DRWCelerite-20 is 60) on tp_combine_lean_kernel (operands from global
    memory: the form that fits the LDS there), which tp_scan_lean = 1 also puts under the smaller shapes.  With tp_scan_tol negative every draw counts as
    having failed the verification launch and is repaired: by the serial-chain windowed kernel (bit-identical to "no_tp") or, with tp_walk_repair, by the
    family's boundary walk (bit-identical to the walk alone)."""
    name = lambda: pj._lib.lib().pioran_celerite_config_name(-1).decode()
    rng = np.random.default_rng(6600 + J + N)
    t, y, s2, A, Bc, C, Dd, mu, nu = _random_case(rng, N, J, B)
    Dd = np.maximum(Dd, 0.05)
    Bc[:, :nreal] = 0.0; Dd[:nreal] = 0.0
    ds = pj.Dataset(t, y, s2, ctx)
    ref = O.logl_batch(A, Bc, C, Dd, t, y, s2, mu, nu, nthreads=8)
    try:
        ctx.set_option("scan_config", "tp"); ctx.set_option("tp_segments", nseg)
        ctx.set_option("tp_scan", 1)
        scan, st = ds.logl_batch(A, Bc, C, Dd, mu=mu, nu=nu, return_status=True)
        assert name() == "tp"
        ctx.set_option("tp_scan_lean", 1)
        lean = ds.logl_batch(A, Bc, C, Dd, mu=mu, nu=nu)
        ctx.set_option("tp_scan_lean", 0)
        ctx.set_option("tp_scan", 0)
        walk = ds.logl_batch(A, Bc, C, Dd, mu=mu, nu=nu)
        ctx.set_option("tp_scan", 1); ctx.set_option("tp_scan_tol", -1.0)    # (negative: every draw counts as failed — well-conditioned draws pass with discrepancy 0)
        repaired = ds.logl_batch(A, Bc, C, Dd, mu=mu, nu=nu)
        assert name() == "tp"
        ctx.set_option("tp_walk_repair", True)
        both = ds.logl_batch(A, Bc, C, Dd, mu=mu, nu=nu)
        ctx.set_option("scan_config", "block" if 2 * J - nreal < 5 else None); ctx.set_option("no_tp", True)       # (fewer than five rows: the windowed kernel only when asked)
        chain = ds.logl_batch(A, Bc, C, Dd, mu=mu, nu=nu)
        assert name() == "block"
    finally:
        ctx.set_option("scan_config", None); ctx.set_option("tp_segments", 0); ctx.set_option("tp_scan", -1); ctx.set_option("tp_scan_tol", 0); ctx.set_option("tp_scan_lean", 0)
        ctx.set_option("tp_walk_repair", False); ctx.set_option("no_tp", False)
    assert np.array_equal(repaired, chain)                 # (every draw through the repair pass: the serial-chain windowed kernel's own values)
    assert (st == 0).all()
    assert relerr(scan, ref) < 1e-11 and relerr(walk, ref) < 1e-11 and relerr(scan, walk) < 1e-11 and relerr(lean, scan) < 1e-12
    rows = 2 * J - nreal
    if 0 < nseg <= 128 and (rows + 7) & ~7 == ((rows + 1) & ~1 if rows <= 12 else (rows + 7) & ~7):
        assert np.array_equal(both, walk)                  # (same segments, same padded layout: the walk after a failed verification is the walk)
    else:
        assert relerr(both, walk) < 1e-12


def test_time_parallel_scan_flagged_draw_and_ill_conditioned_reference_points(ctx, golden_dir):
    """(i) A draw that is not positive definite next to one that is, through the scan: status and value semantics of the other families.
    (ii) Stored reference values at N = 242 (SHO-20, 40 rows) through the scan at 8 segments: 1e-10 against Julia's numbers."""
    name = lambda: pj._lib.lib().pioran_celerite_config_name(-1).decode()
    rng = np.random.default_rng(6715)
    N, J, B = 3000, 6, 2
    t, y, s2, A, Bc, C, Dd, mu, nu = _random_case(rng, N, J, B)
    A[1, 0] = -40.0
    ds = pj.Dataset(t, y, s2, ctx)
    gb, sb = ds.logl_batch(A, Bc, C, Dd, mu=mu, nu=nu, return_status=True)
    assert name() == "tp"
    rb, rs = O.logl_batch(A, Bc, C, Dd, t, y, s2, mu, nu, return_status=True)
    assert sb[1] != 0 and rs[1] != 0 and sb[0] == 0
    assert abs(gb[0] - rb[0]) <= 1e-11 * abs(rb[0])
    assert (np.isnan(gb[1]) and np.isnan(rb[1])) or abs(gb[1] - rb[1]) <= 1e-6 * abs(rb[1])
    # per-draw series (Y, S2) through the scan, and through its repair pass (every draw repaired: the serial-chain kernel's values)
    A[1, 0] = 1.3
    Y = y[None, :] + 0.01 * rng.standard_normal((B, N)); S2 = s2[None, :] * rng.uniform(0.8, 1.2, (B, 1))
    gy = ds.logl_batch(A, Bc, C, Dd, mu=mu, nu=nu, Y=Y, S2=S2)
    assert name() == "tp"
    ry = np.array([O.logl(A[i], Bc[i], C, Dd, t, Y[i] - mu[i], nu[i] * S2[i]) for i in range(B)])
    assert relerr(gy, ry) < 1e-11
    try:
        ctx.set_option("tp_scan_tol", -1.0)
        gr = ds.logl_batch(A, Bc, C, Dd, mu=mu, nu=nu, Y=Y, S2=S2)
        assert name() == "tp"
        ctx.set_option("no_tp", True)
        gc_ = ds.logl_batch(A, Bc, C, Dd, mu=mu, nu=nu, Y=Y, S2=S2)
    finally:
        ctx.set_option("tp_scan_tol", 0); ctx.set_option("no_tp", False)
    assert np.array_equal(gr, gc_) and relerr(gr, ry) < 1e-11
    un = np.load(golden_dir / "ultranest_points.npz")
    sys.path.insert(0, str(Path(__file__).resolve().parent))
    from test_oracle import _un_inputs
    try:
        ctx.set_option("scan_config", "tp"); ctx.set_option("tp_scan", 1); ctx.set_option("tp_segments", 8)
        worst = 0.0
        for i in np.linspace(0, len(un["logl"]) - 1, 40).astype(int):
            a, b, c, d, tt, yy, ss = _un_inputs(un, i)
            dsu = pj.Dataset(tt, yy, ss, ctx)
            g = dsu.logl_batch(a[None, :], b[None, :], c, d)[0]
            assert name() == "tp"
            worst = max(worst, abs(g - un["logl"][i]) / abs(un["logl"][i]))
            dsu.close()
    finally:
        ctx.set_option("scan_config", None); ctx.set_option("tp_scan", -1); ctx.set_option("tp_segments", 0)
    assert worst < 1e-10, worst


def test_time_parallel_scan_check_and_repair_on_prior_draws(ctx, full_size):
    """BASELINE configs[1] as the product runs it (one draw, N = 1e4, automatic choice: the scan, its check by the filter, the repair pass on the serial chain) on 160 prior
    draws of DRWCelerite-20 (60 rows: tp_combine_lean_kernel) and DRWCelerite-10 — the models on which the scan ALONE is wrong for a few per cent of the prior
    (profiles/r06_time_parallel_scan.txt sections 10, 11): every positive definite draw within the north star's 1e-8 of the oracle, statuses the oracle's.  With the check
    switched off (tp_scan_tol huge) the same draws are evaluated again: where that result is off by more than 1e-8 the product path must have repaired it — the check is
    what stands between the scan and the bar."""
    t, y, yerr = full_size
    th = O.synthetic_theta(160, t, y, seed=909)
    ds = pj.Dataset(t, y, yerr ** 2, ctx)
    name = lambda: pj._lib.lib().pioran_celerite_config_name(-1).decode()
    caught = 0
    for ncomp in (20, 10):
        A, Bc, C, Dd, mu, nu = O.theta_to_coefs(th, t, ncomp, "DRWCelerite")
        ref, rst = O.logl_batch(A, Bc, C, Dd, t, y, yerr ** 2, mu, nu, nthreads=8, return_status=True)
        got = np.empty(len(th)); st = np.empty(len(th), int); alone = np.empty(len(th))
        for i in range(len(th)):
            g, s_ = ds.logl_batch(A[i:i + 1], Bc[i:i + 1], C, Dd, mu=mu[i:i + 1], nu=nu[i:i + 1], return_status=True)
            assert name() == "tp"
            got[i], st[i] = g[0], s_[0]
        try:
            ctx.set_option("tp_scan_tol", 1e30)
            for i in range(len(th)):
                alone[i] = ds.logl_batch(A[i:i + 1], Bc[i:i + 1], C, Dd, mu=mu[i:i + 1], nu=nu[i:i + 1])[0]
        finally:
            ctx.set_option("tp_scan_tol", 0)
        ok = rst == 0
        assert np.array_equal(st != 0, rst != 0)
        assert relerr(got[ok], ref[ok]) < 1e-8, (ncomp, relerr(got[ok], ref[ok]))
        caught += int((np.abs(alone[ok] - ref[ok]) / np.abs(ref[ok]) > 1e-8).sum())
    print(f"draws the scan alone gets wrong by more than 1e-8 (all repaired): {caught}")


TILE_GRAD = "tile (windowed gradient, one draw per wavefront)"


@pytest.mark.parametrize("J,N,B,nreal", [(1, 40, 3, 0), (3, 50, 5, 0), (5, 16, 2, 0), (8, 37, 6, 0), (8, 100, 3, 1), (10, 17, 4, 0), (12, 64, 4, 2), (15, 130, 5, 0),
                                         (16, 33, 70, 0), (20, 257, 9, 0), (23, 48, 2, 0), (23, 95, 3, 5), (24, 50, 5, 0), (28, 40, 7, 2), (30, 97, 5, 3),
                                         (31, 130, 4, 0), (40, 65, 4, 20)])
def test_tile_gradient_matches_complex_step(ctx, J, N, B, nreal):
    """d log L / d(a_j, b_j, mu, nu) by the one-draw-per-wavefront reverse mode (celerite_tile_adjoint_kernel, round 5; what many chains of an
    approx-based model ask for), forced here at every batch size: against the complex-step derivatives of the oracle and the small-batch windowed
    reverse mode; block columns NB = 1 .. 4 (up to 63 rows; at four — DRWCelerite-20's 60 rows — three draws per workgroup and T_k loaded at the head of
    its own window), ragged last windows, N = 16 and 17 (one window / one step in the second), one-row terms, more draws than one workgroup
    holds; the value is bit-identical to the tile forward kernel's."""
    rng = np.random.default_rng(7700 + J + N)
    t, y, s2, A, Bc, C, Dd, mu, nu = _random_case(rng, N, J, B)
    Bc[:, :nreal] = 0.0; Dd[:nreal] = 0.0
    ds = pj.Dataset(t, y, s2, ctx)
    name = lambda: pj._lib.lib().pioran_celerite_config_name(-1).decode()
    try:
        ctx.set_option("scan_config", "tile")
        g = ds.logl_grad(A, Bc, C, Dd, mu=mu, nu=nu, cd_grad=False)
        assert name() == TILE_GRAD
        val = ds.logl_batch(A, Bc, C, Dd, mu=mu, nu=nu)
        assert name() == "tile"
        gt = ds.logl_grad(A, Bc, C, Dd, mu=mu, nu=nu)               # with d/d(c, d) of the shared (c, d): round 6, the same kernels (CD instantiation)
        assert name() == TILE_GRAD
    finally:
        ctx.set_option("scan_config", None)
    gc = ds.logl_grad(A, Bc, C, Dd, mu=mu, nu=nu)                   # the small-batch windowed reverse mode (the automatic choice at these chain counts)
    assert name() == "block (windowed gradient)"
    assert (g["logl"] == val).all() and (g["status"] == 0).all() and (gt["logl"] == val).all()
    assert relerr(g["logl"], O.logl_batch(A, Bc, C, Dd, t, y, s2, mu, nu)) < 1e-11
    for key in ("grad_a", "grad_b", "grad_mu", "grad_nu"):
        assert np.max(np.abs(g[key] - gc[key])) <= 1e-11 * (1 + np.max(np.abs(gc[key]))), key
    for key in ("grad_a", "grad_b", "grad_c", "grad_d", "grad_mu", "grad_nu"):
        assert np.max(np.abs(gt[key] - gc[key])) <= 1e-11 * (1 + np.max(np.abs(gc[key]))), key
    ref = O.logl_grad(A[0], Bc[0], C, Dd, t, y - mu[0], nu[0] * s2, cd=True)       # d/d(c, d) against complex steps of the oracle
    assert np.max(np.abs(gt["grad_c"][0] - ref["grad_c"])) <= 1e-9 * (1 + np.max(np.abs(ref["grad_c"])))
    assert np.max(np.abs(gt["grad_d"][0] - ref["grad_d"])) <= 1e-9 * (1 + np.max(np.abs(ref["grad_d"])))
    one_row = Dd == 0.0                                             # (one-row terms: structurally zero, exactly 0.0 by the contract of pioran_hip.h)
    assert (gt["grad_b"][:, one_row] == 0.0).all() and (gt["grad_d"][:, one_row] == 0.0).all() and (g["grad_b"][:, one_row] == 0.0).all()
    for i in range(min(B, 4)):
        ref = O.logl_grad(A[i], Bc[i], C, Dd, t, y - mu[i], nu[i] * s2)
        for key in ("grad_a", "grad_b"):
            assert np.max(np.abs(g[key][i] - ref[key])) <= 1e-9 * (1 + np.max(np.abs(ref[key]))), (key, i)
        gm = O.logl_dir(A[i], Bc[i], C, Dd, t, y - mu[i], nu[i] * s2, dy=-np.ones(N))
        gn = O.logl_dir(A[i], Bc[i], C, Dd, t, y - mu[i], nu[i] * s2, ds2=s2)
        assert abs(g["grad_mu"][i] - gm) <= 1e-9 * (1 + abs(gm)) and abs(g["grad_nu"][i] - gn) <= 1e-9 * (1 + abs(gn))


def test_tile_gradient_dispatch_chunks_and_flagged_draws(ctx):
    """The automatic choice (more than 512 chains, 17 .. 63 rows, with or without d/d(c, d) of shared (c, d)), "no_tile", a workspace limit that forces several
    launches (the chunk is cut by 1024 chains, then halved), optional outputs left out, and a draw that is not positive definite: its status
    is the forward kernel's and the other chains are untouched."""
    rng = np.random.default_rng(4242)
    J, N, B = 10, 300, 700
    t, y, s2, A, Bc, C, Dd, mu, nu = _random_case(rng, N, J, B)
    ds = pj.Dataset(t, y, s2, ctx)
    name = lambda: pj._lib.lib().pioran_celerite_config_name(-1).decode()
    g = ds.logl_grad(A, Bc, C, Dd, mu=mu, nu=nu, cd_grad=False)
    assert name() == TILE_GRAD and (g["status"] == 0).all()
    assert ds.logl_grad(A[:512], Bc[:512], C, Dd, mu=mu[:512], nu=nu[:512], cd_grad=False)["logl"].shape == (512,) and name() == "block (windowed gradient)"
    gcd = ds.logl_grad(A, Bc, C, Dd, mu=mu, nu=nu)               # with d/d(c, d) (round 6): the same kernels
    assert gcd["grad_c"] is not None and name() == TILE_GRAD
    assert ds.logl_grad(A[:, :8], Bc[:, :8], C[:8], Dd[:8], mu=mu, nu=nu, cd_grad=False)["logl"].shape == (B,) and name() == "block (windowed gradient)"   # 16 rows
    try:
        ctx.set_option("no_tile", True)
        h = ds.logl_grad(A, Bc, C, Dd, mu=mu, nu=nu, cd_grad=False)
        assert name() == "block (windowed gradient)"
    finally:
        ctx.set_option("no_tile", False)
    assert relerr(g["logl"], h["logl"]) < 1e-12
    for key in ("grad_a", "grad_b", "grad_mu", "grad_nu"):
        assert np.max(np.abs(g[key] - h[key])) <= 1e-11 * (1 + np.max(np.abs(h[key]))), key
    try:
        ctx.set_option("no_tile", True)
        hcd = ds.logl_grad(A, Bc, C, Dd, mu=mu, nu=nu)
        assert name() == "block (windowed gradient)"
    finally:
        ctx.set_option("no_tile", False)
    for key in ("grad_a", "grad_b", "grad_c", "grad_d", "grad_mu", "grad_nu"):
        assert np.max(np.abs(gcd[key] - hcd[key])) <= 1e-11 * (1 + np.max(np.abs(hcd[key]))), key
    try:       # 19 windows x 3 tiles x 2 KB = 114 KB of T per chain: 1 MB holds nine chains -> 700 -> 350 -> ... -> 5 per launch
        ctx.set_option("workspace_limit_mb", 1)
        gs = ds.logl_grad(A, Bc, C, Dd, mu=mu, nu=nu, cd_grad=False)
        assert name() == TILE_GRAD
    finally:
        ctx.set_option("workspace_limit_mb", 0)
    assert np.array_equal(gs["logl"], g["logl"])
    for key in ("grad_a", "grad_b", "grad_mu", "grad_nu"):       # (sums over lanes by LDS atomics: equal to rounding)
        assert np.max(np.abs(gs[key] - g[key])) <= 1e-13 * (1 + np.max(np.abs(g[key]))), key
    g2 = ds.logl_grad(A, Bc, C, Dd, cd_grad=False)               # no mu, no nu
    assert name() == TILE_GRAD and relerr(g2["logl"], O.logl_batch(A, Bc, C, Dd, t, y, s2, None, None, nthreads=8)) < 1e-11
    A2 = A.copy(); A2[3, 0] = -40.0; A2[699, 1] = -60.0
    gb = ds.logl_grad(A2, Bc, C, Dd, mu=mu, nu=nu, cd_grad=False)
    assert name() == TILE_GRAD
    try:
        ctx.set_option("no_tile", True)
        hb = ds.logl_grad(A2, Bc, C, Dd, mu=mu, nu=nu, cd_grad=False)
    finally:
        ctx.set_option("no_tile", False)
    assert np.array_equal(gb["status"], hb["status"]) and gb["status"][3] != 0 and gb["status"][699] != 0 and (np.delete(gb["status"], [3, 699]) == 0).all()
    ok = gb["status"] == 0
    assert np.array_equal(gb["logl"][ok], g["logl"][ok])
    for key in ("grad_a", "grad_b", "grad_mu", "grad_nu"):
        assert np.max(np.abs(gb[key][ok] - g[key][ok])) <= 1e-13 * (1 + np.max(np.abs(g[key]))), key


def test_tile_gradient_full_size(ctx, full_size):
    """N = 1e4 (BASELINE shape), 1024 prior draws of SHO-20 (40 rows) and DRWCelerite-15 (45 rows, 15 of the 30 terms with one row): the
    one-draw-per-wavefront reverse mode against the small-batch windowed reverse mode on every chain both call positive definite, and against
    complex steps of the oracle; DRWCelerite-20 (60 rows: four block columns, three draws per workgroup — automatic since the reverse kernel stopped
    spilling there, round 6) likewise.  Up to 512 chains: the small-batch kernels."""
    t, y, yerr = full_size
    th = O.synthetic_theta(1024, t, y, seed=77)
    ds = pj.Dataset(t, y, yerr ** 2, ctx)
    rng = np.random.default_rng(6)
    name = lambda: pj._lib.lib().pioran_celerite_config_name(-1).decode()
    A, Bc, C, Dd, mu, nu = O.theta_to_coefs(th[:300], t, 20, "DRWCelerite")
    ds.logl_grad(A, Bc, C, Dd, mu=mu, nu=nu, cd_grad=False)
    assert name() == "block (windowed gradient)"
    for basis, ncomp in (("SHO", 20), ("DRWCelerite", 15), ("DRWCelerite", 20)):
        A, Bc, C, Dd, mu, nu = O.theta_to_coefs(th, t, ncomp, basis)
        g = ds.logl_grad(A, Bc, C, Dd, mu=mu, nu=nu, cd_grad=False)
        assert name() == TILE_GRAD
        try:
            ctx.set_option("no_tile", True)
            h = ds.logl_grad(A, Bc, C, Dd, mu=mu, nu=nu, cd_grad=False)
            assert name() == "block (windowed gradient)"
        finally:
            ctx.set_option("no_tile", False)
        assert np.array_equal(g["status"] != 0, h["status"] != 0)
        ok = g["status"] == 0
        assert ok.mean() > 0.9
        # (prior draws include ill-conditioned ones, where every fp64 evaluation is up to 8e-9 from the __float128 truth: profiles/r05_quad_truth.txt)
        el = np.abs(g["logl"][ok] - h["logl"][ok]) / np.abs(h["logl"][ok])
        assert np.median(el) < 1e-12 and el.max() < 2e-8, (float(np.median(el)), float(el.max()))
        # per chain, relative to the chain's gradient scale.  Both are fp64 evaluations of an ill-conditioned sum at the worst draws:
        # the bulk agrees to 1e-10, the worst chain of 1024 to 1e-6
        for key in ("grad_a", "grad_b", "grad_mu", "grad_nu"):
            a_, b_ = g[key][ok].reshape(ok.sum(), -1), h[key][ok].reshape(ok.sum(), -1)
            sc = np.max(np.abs(h["grad_a"][ok]), axis=1) + 1.0 if key in ("grad_a", "grad_b") else np.abs(b_[:, 0]) + 1.0
            d = np.max(np.abs(a_ - b_), axis=1) / sc
            assert np.median(d) < 1e-10 and d.max() < 1e-6, (basis, key, float(np.median(d)), float(d.max()))
        for i in np.flatnonzero(ok)[:2]:
            J = A.shape[1]
            scale = 1 + max(np.max(np.abs(g["grad_a"][i])), np.max(np.abs(g["grad_b"][i])))
            for _ in range(2):
                da, db = rng.standard_normal(J), rng.standard_normal(J)
                if basis == "DRWCelerite":
                    db[Dd == 0.0] = 0.0
                ref = O.logl_dir(A[i], Bc[i], C, Dd, t, y - mu[i], nu[i] * yerr ** 2, da=da, db=db)
                assert abs(g["grad_a"][i] @ da + g["grad_b"][i] @ db - ref) <= 1e-7 * scale * np.sqrt(J), basis
            gm = O.logl_dir(A[i], Bc[i], C, Dd, t, y - mu[i], nu[i] * yerr ** 2, dy=-np.ones(len(t)))
            assert abs(g["grad_mu"][i] - gm) <= 1e-7 * (1 + abs(gm))


@pytest.mark.parametrize("J,N,B", [(1, 45, 3), (2, 60, 4), (3, 50, 4), (7, 33, 3), (12, 100, 5), (20, 130, 3), (31, 40, 2)])
def test_windowed_gradient_per_draw_cd_all_chains_in_one_launch(ctx, J, N, B):
    """(c, d) per draw in every term (CARMA kernels, QPO features, free Celerite sums under NUTS): all chains in one launch of the
    windowed reverse mode, one pair of tables per draw — against the complex-step oracle draw by draw, series gradients included."""
    rng = np.random.default_rng(9900 + J + N)
    t, y, s2, A, Bc, C, Dd, mu, nu = _random_case(rng, N, J, B, per_draw_cd=True)
    ds = pj.Dataset(t, y, s2, ctx)
    g = ds.logl_grad(A, Bc, C, Dd, mu=mu, nu=nu, series_grad=True)
    assert pj._lib.lib().pioran_celerite_config_name(-1).decode() == "block (windowed gradient, per-draw tables)"
    assert relerr(g["logl"], O.logl_batch(A, Bc, C, Dd, t, y, s2, mu, nu)) < 1e-11 and (g["status"] == 0).all()
    for i in range(B):
        ref = O.logl_grad(A[i], Bc[i], C[i], Dd[i], t, y - mu[i], nu[i] * s2, cd=True, series=True)
        for key in ("grad_a", "grad_b", "grad_c", "grad_d", "grad_y"):
            assert np.max(np.abs(g[key][i] - ref[key])) <= 1e-9 * (1 + np.max(np.abs(ref[key]))), (key, i)
        assert np.max(np.abs(g["grad_sigma2"][i] - nu[i] * ref["grad_sigma2"])) <= 1e-9 * (1 + np.max(np.abs(ref["grad_sigma2"])))
        gm = O.logl_dir(A[i], Bc[i], C[i], Dd[i], t, y - mu[i], nu[i] * s2, dy=-np.ones(N))
        gn = O.logl_dir(A[i], Bc[i], C[i], Dd[i], t, y - mu[i], nu[i] * s2, ds2=s2)
        assert abs(g["grad_mu"][i] - gm) <= 1e-9 * (1 + abs(gm)) and abs(g["grad_nu"][i] - gn) <= 1e-9 * (1 + abs(gn))


def test_windowed_gradient_shifted_log_flux_model(ctx, golden_dir):
    """The shifted log-flux models (docs/src/turing.md:205-230) through the windowed reverse mode: per-draw transformed series in,
    series gradients chained to d/dshift — equal to the step-by-step adjoint path on the reference's own nested-sampling points."""
    un = np.load(golden_dir / "ultranest_points.npz")
    t, y, yerr, P = un["t"], un["y"], un["yerr"], un["params"][:6]
    f_min, f_max = 1 / (t[-1] - t[0]), 1 / np.min(np.diff(t)) / 2
    A, Bc, C, Dd = pj.approx_batch(pj.SingleBendingPowerLaw, P[:, :3], f_min, f_max, 20, P[:, 3], is_integrated_power=False)
    ds = pj.Dataset(t, y, yerr ** 2, ctx)
    gw = ds.logl_grad(A, Bc, C, Dd, mu=P[:, 5], nu=P[:, 4], shift=P[:, 6])
    assert pj._lib.lib().pioran_celerite_config_name(-1).decode() == "block (windowed gradient)"
    try:
        ctx.set_option("no_block", True)
        go = ds.logl_grad(A, Bc, C, Dd, mu=P[:, 5], nu=P[:, 4], shift=P[:, 6])
    finally:
        ctx.set_option("no_block", False)
    assert pj._lib.lib().pioran_celerite_config_name(-1).decode() == "wide (step-by-step gradient)"
    assert relerr(gw["logl"], un["logl"][:6]) < 1e-10
    for k in ("grad_a", "grad_b", "grad_c", "grad_d", "grad_mu", "grad_nu", "grad_shift"):
        assert np.max(np.abs(gw[k] - go[k])) <= 1e-8 * (1 + np.max(np.abs(go[k]))), k


def test_gradient_full_size_and_real_terms(ctx, full_size):
    """N = 1e4 (BASELINE shape), SHO-20 and DRWCelerite-20 (terms with b = d = 0: one row each), against one complex
    step per direction for a few directions, bar 1e-7 relative to the gradient scale."""
    t, y, yerr = full_size
    th = O.synthetic_theta(3, t, y)
    ds = pj.Dataset(t, y, yerr ** 2, ctx)
    rng = np.random.default_rng(5)
    for basis, windowed in (("SHO", False), ("DRWCelerite", False), ("SHO", True), ("DRWCelerite", True)):
        A, Bc, C, Dd, mu, nu = O.theta_to_coefs(th, t, 20, basis)
        try:   # both reverse modes: the windowed one (round 3; the default up to 63 rows) and the step-by-step adjoint kernels
            ctx.set_option("no_block", not windowed)
            g = ds.logl_grad(A, Bc, C, Dd, mu=mu, nu=nu)
        finally:
            ctx.set_option("no_block", False)
        assert pj._lib.lib().pioran_celerite_config_name(-1).decode() == ("block (windowed gradient)" if windowed else "wide (step-by-step gradient)")
        ref_l, rst = O.logl_batch(A, Bc, C, Dd, t, y, yerr ** 2, mu, nu, nthreads=4, return_status=True)
        for i in np.flatnonzero(rst == 0)[:2]:
            assert abs(g["logl"][i] - ref_l[i]) <= 1e-8 * abs(ref_l[i])
            J = A.shape[1]
            scale = 1 + max(np.max(np.abs(g["grad_a"][i])), np.max(np.abs(g["grad_b"][i])))
            for _ in range(3):
                da, db = rng.standard_normal(J), rng.standard_normal(J)
                if basis == "DRWCelerite":
                    db[Dd == 0.0] = 0.0        # b of a real term is structurally zero (its sin row is dropped)
                ref = O.logl_dir(A[i], Bc[i], C, Dd, t, y - mu[i], nu[i] * yerr ** 2, da=da, db=db)
                got = g["grad_a"][i] @ da + g["grad_b"][i] @ db
                assert abs(got - ref) <= 1e-7 * scale * np.sqrt(J), basis
            gm = O.logl_dir(A[i], Bc[i], C, Dd, t, y - mu[i], nu[i] * yerr ** 2, dy=-np.ones(len(t)))
            assert abs(g["grad_mu"][i] - gm) <= 1e-7 * (1 + abs(gm))


def test_gradient_wrt_c_and_d_qpo_and_carma(ctx, golden_dir, full_size):
    """dlogL/d(c_j, d_j) — what ForwardDiff gets through the generic logl for kernels whose decay rates and frequencies are
    sampled: a QPO feature on top of an approx continuum (src/psd.jl:15-27, 254-261), a CARMA(3,2) kernel
    (src/CARMA.jl:98-143, coefficients of test/test_carma.jl:55-69), per-draw (c, d) [B][J], and N = 1e4 with 78 checkpoint
    segments.  Against the complex step of the oracle, 1e-8 of the gradient scale (1e-6 at N = 1e4: the gradient of a
    10^4-step recurrence carries ~1e-9 relative rounding per component of a vector whose entries span 6 decades)."""
    def check(ds, t, y, s2, A, Bc, C, Dd, mu, nu, tol, dirs=None):
        g = ds.logl_grad(A, Bc, C, Dd, mu=mu, nu=nu)
        shared = np.ndim(C) == 1
        for i in range(len(A)):
            c_i, d_i = (C, Dd) if shared else (C[i], Dd[i])
            yy, ss = y - (mu[i] if mu is not None else 0.0), (nu[i] if nu is not None else 1.0) * s2
            assert abs(g["logl"][i] - O.logl(A[i], Bc[i], c_i, d_i, t, yy, ss)) <= 1e-8 * abs(g["logl"][i])
            if dirs is None:
                ref = O.logl_grad(A[i], Bc[i], c_i, d_i, t, yy, ss, cd=True)
                for k in ("grad_a", "grad_b", "grad_c", "grad_d"):
                    assert np.max(np.abs(g[k][i] - ref[k])) <= tol * (1 + np.max(np.abs(ref[k]))), (k, i)
            else:   # a few random directions in (c, d) space: one complex step each
                J = A.shape[1]
                im = ctypes.c_double()
                P = lambda v: np.ascontiguousarray(v, dtype=np.float64).ctypes.data_as(ctypes.POINTER(ctypes.c_double))
                for dc, dd in dirs:
                    h = 1e-30
                    O.lib().oracle_logl_complex_cd(len(t), J, P(A[i]), None, P(Bc[i]), None, P(c_i), P(h * dc), P(d_i), P(h * dd), P(t),
                                                   P(yy), None, P(ss), None, ctypes.byref(im))
                    got = g["grad_c"][i] @ dc + g["grad_d"][i] @ dd
                    scale = np.abs(g["grad_c"][i]) @ np.abs(dc) + np.abs(g["grad_d"][i]) @ np.abs(dd)
                    assert abs(got - im.value / h) <= tol * (1 + scale), (got, im.value / h)
        return g

    rng = np.random.default_rng(4)
    A_ = np.loadtxt(golden_dir / "simu.txt")
    t, y, yerr = A_[:300, 0], A_[:300, 1], A_[:300, 2]
    ds = pj.Dataset(t, y, yerr ** 2, ctx)
    # (1) continuum (SHO-10) + one QPO term (a, b = a / (2Q) ... : Celerite term with d >> c), shared by 3 draws
    f_min, f_max = 1 / (t[-1] - t[0]), 1 / np.min(np.diff(t)) / 2
    th = np.array([[0.5, 0.02, 3.0], [0.8, 0.05, 2.5], [0.2, 0.01, 3.5]])
    A, Bc, C, Dd = pj.approx_batch(pj.SingleBendingPowerLaw, th, f_min, f_max, 10, np.array([1.0, 0.5, 2.0]))
    qa = rng.uniform(0.1, 0.5, (3, 1))
    C2 = np.append(C, 0.02); D2 = np.append(Dd, 2 * np.pi * 0.1)
    # (a celerite term is a valid covariance only for |b d| <= a c: half of that bound)
    A2 = np.concatenate([A, qa], axis=1); B2 = np.concatenate([Bc, 0.5 * qa * C2[-1] / D2[-1]], axis=1)
    check(ds, t, y, yerr ** 2, A2, B2, C2, D2, np.array([0.1, 0.0, -0.1]), np.array([1.0, 1.2, 0.9]), 1e-8)
    # (2) the same with per-draw (c, d) of the QPO term: [B][J] arrays, every draw its own table
    C3 = np.tile(C2, (3, 1)); D3 = np.tile(D2, (3, 1))
    C3[:, -1] = [0.02, 0.05, 0.01]; D3[:, -1] = 2 * np.pi * np.array([0.1, 0.13, 0.07])
    B3 = B2.copy(); B3[:, -1] = 0.5 * A2[:, -1] * C3[:, -1] / D3[:, -1]
    g3 = check(ds, t, y, yerr ** 2, A2, B3, C3, D3, np.array([0.1, 0.0, -0.1]), np.array([1.0, 1.2, 0.9]), 1e-8)
    assert g3["grad_c"].shape == (3, 11)
    # (3) CARMA(3,2): one real term (b = d = 0: single row) and one complex term with NEGATIVE d
    lit = json.loads((golden_dir / "reference_literals.json").read_text())["carma32"]
    k = pj.CARMA(lit["p"], lit["q"], np.array([complex(*z) for z in lit["r_alpha"]]), lit["beta"], lit["norm"])
    a, b, c, d = (np.atleast_2d(v) for v in k.celerite_coefs())
    gk = ds.logl_grad(a, b, c[0], d[0], mu=[0.3], nu=[1.1])
    ref = O.logl_grad(a[0], b[0], c[0], d[0], t, y - 0.3, 1.1 * yerr ** 2, cd=True)
    real = d[0] == 0.0
    for key in ("grad_a", "grad_c"):
        assert np.max(np.abs(gk[key][0] - ref[key])) <= 1e-8 * (1 + np.max(np.abs(ref[key]))), key
    # a real term keeps only its cos row: b and d are structurally absent there, their derivatives are reported as 0
    for key in ("grad_b", "grad_d"):
        assert np.max(np.abs(gk[key][0][~real] - ref[key][~real])) <= 1e-8 * (1 + np.max(np.abs(ref[key]))), key
        assert (gk[key][0][real] == 0.0).all()
    # (4) N = 1e4, SHO-20: 78 segments of 128 steps (+ the tail); random directions in (c, d)
    tL, yL, eL = full_size
    thL = O.synthetic_theta(2, tL, yL)
    AL, BL, CL, DL, muL, nuL = O.theta_to_coefs(thL, tL, 20, "SHO")
    dsL = pj.Dataset(tL, yL, eL ** 2, ctx)
    dirs = [(rng.standard_normal(20) * CL, rng.standard_normal(20) * DL) for _ in range(3)]
    check(dsL, tL, yL, eL ** 2, AL, BL, CL, DL, muL, nuL, 1e-6, dirs=dirs)


def test_gradient_workspace_is_small(ctx, full_size):
    """64 chains at N = 1e4, J = 20.  Step-by-step reverse mode: checkpoints + one replayed segment, not every S_n (180 MB per draw
    in round 1): ~10 MB per draw, the context grows by well under 1 GB.  Windowed reverse mode (round 3): what the forward pass leaves
    per 16-step window (T, M', Q' twice, Sigma^-1: 38 KB) = 24 MB per draw, under 2 GB.  pioran_ctx_trim gives either back."""
    import torch
    t, y, yerr = full_size
    th = O.synthetic_theta(64, t, y, seed=3)
    A, Bc, C, Dd, mu, nu = O.theta_to_coefs(th, t, 20, "SHO")
    for mode, bound in (("windowed", 2.0e9), ("step-by-step", 1.0e9)):
        c2 = pj.Context(0)
        c2.set_option("no_block", mode != "windowed")
        ds = pj.Dataset(t, y, yerr ** 2, c2)
        val = ds.logl_batch(A, Bc, C, Dd, mu=mu, nu=nu)
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        g = ds.logl_grad(A, Bc, C, Dd, mu=mu, nu=nu)
        used = free0 - torch.cuda.mem_get_info()[0]
        assert used < bound, (mode, used)
        ok = g["status"] == 0
        assert ok.sum() > 32 and relerr(g["logl"][ok], val[ok]) < 1e-10
        c2.trim()
        assert torch.cuda.mem_get_info()[0] >= free0 - (64 << 20)
        ds.close(); c2.close()


def test_gradient_wrt_sampled_parameters(ctx, golden_dir):
    """d log L / d(alpha1, f1, alpha2, variance, nu, mu) — the parameters a sampler moves (README.md:38-71) — on the
    reference's simu_log series: device gradient chained through approx vs central differences of the oracle's value
    through the oracle's own approx (a fully independent path), bar 1e-5 (finite-difference accuracy)."""
    A_ = np.loadtxt(golden_dir / "simu_log.txt")
    t, y, yerr = A_[:, 0], A_[:, 1], A_[:, 2]
    f_min, f_max = 1 / (t[-1] - t[0]), 1 / np.min(np.diff(t)) / 2
    th = np.array([[0.82, 0.01, 3.3], [0.3, 0.05, 2.5], [0.6, 0.02, 3.0]])
    var = np.array([np.var(y, ddof=1), 0.5, 2.0]); nu = np.array([1.0, 1.4, 0.8]); mu = np.array([0.0, 0.1, -0.2])
    ds = pj.Dataset(t, y, yerr ** 2, ctx)
    for basis in ("SHO", "DRWCelerite"):
        g = ds.logpdf_theta_grad(pj.SingleBendingPowerLaw, th, var, f_min, f_max, 20, basis_function=basis, mu=mu, nu=nu)
        def val(i, p):
            a, b, c, d = O.approx(lambda f: O.single_bending_power_law(f, p[0], p[1], p[2]), f_min, f_max, 20, p[3],
                                  basis_function=basis)
            return O.logl(a, b, c, d, t, y - p[5], p[4] * yerr ** 2)
        for i in range(3):
            p0 = np.array([th[i, 0], th[i, 1], th[i, 2], var[i], nu[i], mu[i]])
            assert abs(g["logl"][i] - val(i, p0)) <= 1e-10 * abs(val(i, p0))
            got = np.array([*g["grad_theta"][i], g["grad_norm"][i], g["grad_nu"][i], g["grad_mu"][i]])
            for k in range(6):
                # five-point stencil with a step large enough to keep the rounding of the ill-conditioned spectral
                # solve inside approx (amplified by 1/h) below the bar
                h = 1e-4 * max(1.0, abs(p0[k])) if k != 1 else 1e-4 * p0[1]
                e = np.zeros(6); e[k] = h
                fd = (8 * (val(i, p0 + e) - val(i, p0 - e)) - (val(i, p0 + 2 * e) - val(i, p0 - 2 * e))) / (12 * h)
                assert abs(got[k] - fd) <= 1e-5 * (1 + abs(fd)), (basis, i, k, got[k], fd)


def test_gradient_chunking_and_optional_arguments(ctx):
    """More draws than one 1024-draw chunk; mu / nu omitted; gradient rows of every draw consistent with a one-draw call."""
    rng = np.random.default_rng(31)
    N, J, B = 60, 6, 1030
    t, y, s2, A, Bc, C, Dd, mu, nu = _random_case(rng, N, J, B)
    ds = pj.Dataset(t, y, s2, ctx)
    g = ds.logl_grad(A, Bc, C, Dd)
    assert relerr(g["logl"], O.logl_batch(A, Bc, C, Dd, t, y, s2, np.zeros(B), np.ones(B), nthreads=8)) < 1e-11
    for i in (0, 255, 1023, 1024, 1029):
        one = ds.logl_grad(A[i:i + 1], Bc[i:i + 1], C, Dd)
        assert np.array_equal(one["grad_a"][0], g["grad_a"][i]) and np.array_equal(one["grad_b"][0], g["grad_b"][i])
        ref = O.logl_grad(A[i], Bc[i], C, Dd, t, y, s2)
        assert np.max(np.abs(g["grad_a"][i] - ref["grad_a"])) <= 1e-9 * (1 + np.max(np.abs(ref["grad_a"])))


def test_carma_kernel_on_the_likelihood_path(ctx, golden_dir):
    """log_likelihood(::CARMA, ...) (src/celerite_solver.jl:272-282): the kernel enters as its celerite coefficients;
    celerite path == oracle == -dense path, as the reference's relation tests do for the other kernels."""
    g = json.loads((golden_dir / "reference_literals.json").read_text())["carma32"]
    k = pj.CARMA(g["p"], g["q"], np.array([complex(*z) for z in g["r_alpha"]]), g["beta"], g["norm"])
    A = np.loadtxt(golden_dir / "simu.txt")
    t, y, yerr = A[:200, 0], A[:200, 1], A[:200, 2]
    v = pj.log_likelihood(k, t, y, yerr ** 2, ctx=ctx)
    a, b, c, d = k.celerite_coefs()
    assert abs(v - O.logl(a, b, c, d, t, y, yerr ** 2)) <= 1e-10 * abs(v)
    assert abs(v + pj.log_likelihood_direct(k, t, y, yerr ** 2, ctx=ctx)) <= 1e-9 * abs(v)
    assert abs(pj.logpdf(pj.ScalableGP(0.3, k)(t, yerr ** 2), y, ctx=ctx) - O.logl(a, b, c, d, t, y - 0.3, yerr ** 2)) <= 1e-10 * abs(v)


def test_dense_predict_direct(ctx, golden_dir):
    """predict_direct (src/direct_solver.jl:75-119) on the device's dense solver: equal to the numpy restatement and — the
    relation the reference's prediction tests assert (test/test_prediction.jl:49-58) — to the celerite `predict`."""
    A = np.loadtxt(golden_dir / "simu.txt")
    t, y, yerr = A[:, 0], A[:, 1], A[:, 2]
    f0, fM = 1 / (t[-1] - t[0]) / 100, 1 / np.min(np.diff(t)) / 2 * 20
    R = pj.approx(pj.SingleBendingPowerLaw(0.82, 0.01, 3.3), f0, fM, 20, np.var(y, ddof=1))
    for tau in (t, np.linspace(t.min() - 30, t.max() + 30, 333)):
        m, K = pj.predict_direct(R, tau, t, y, yerr ** 2, with_covariance=True, ctx=ctx)
        ref = O.predict_direct_numpy(R.a, R.b, R.c, R.d, tau, t, y, yerr ** 2)
        assert np.max(np.abs(m - ref)) <= 1e-9 * max(1.0, np.max(np.abs(ref)))
        assert np.max(np.abs(m - pj.predict(R, tau, t, y, yerr ** 2, ctx=ctx))) <= 1e-8 * max(1.0, np.max(np.abs(ref)))
        Kref = O.predict_cov_numpy(R.a, R.b, R.c, R.d, tau, t, yerr ** 2)
        assert np.max(np.abs(K - Kref)) <= 1e-9 * np.max(np.abs(Kref))
        assert np.array_equal(pj.predict_direct(R, tau, t, y, yerr ** 2, ctx=ctx), m)


def test_reference_sample_tests(ctx):
    """test/test_scalablegp.jl:179-237: rand of the posterior (shapes, finiteness) and of the prior GP, same literals."""
    t = np.array([0.0, 3.0, 3.2, 3.4, 45.5, 101.2])
    tx = np.array([0.0, 1.4, 2.3, 3.0, 3.1, 3.2, 3.3, 3.4, 45.5, 101.2, 202.32])
    y = np.array([1.3, 2.2, 4.21, 2.5, 3.3, 5.2]); yerr = np.array([0.1, 0.2, 0.1, 0.1, 0.2, 0.1])
    R = pj.approx(pj.SingleBendingPowerLaw(0.2, 0.02, 3.1), 1e-4, 1e1, 30, 2.31, basis_function="SHO")
    fx = pj.ScalableGP(1.2, R)(t, yerr ** 2)
    fp = pj.posterior(fx, y)
    rng = np.random.default_rng(1234)
    s, s10 = pj.rand_posterior(rng, fp, ctx=ctx), pj.rand_posterior(rng, fp, None, 10, ctx=ctx)
    sx, sx10 = pj.rand_posterior(rng, fp, tx, ctx=ctx), pj.rand_posterior(rng, fp, tx, 10, ctx=ctx)
    assert np.isfinite(s).all() and np.isfinite(s10).all()
    assert s10.shape == (len(t), 10) and sx.shape == (len(tx), 1) and sx10.shape == (len(tx), 10)
    assert np.isfinite(pj.rand(rng, fx, ctx=ctx)).all() and np.isfinite(pj.rand(rng, fx, tx, ctx=ctx)).all()
    assert len(pj.rand(rng, fx, tx, ctx=ctx)) == len(tx)


def test_gradient_shifted_log_flux_model(ctx, golden_dir):
    """The documented Turing model with a sampled shift (docs/src/turing.md:205-230): d log L / dc through the device
    transform, against the complex step of the oracle along the induced direction in (y, sigma2) space; the other
    gradients equal those of a data set that holds the transformed series."""
    un = np.load(golden_dir / "ultranest_points.npz")
    t, y, yerr = un["t"], un["y"], un["yerr"]
    P = un["params"][:5]
    f_min, f_max = 1 / (t[-1] - t[0]), 1 / np.min(np.diff(t)) / 2
    A, Bc, C, Dd = pj.approx_batch(pj.SingleBendingPowerLaw, P[:, :3], f_min, f_max, 20, P[:, 3], is_integrated_power=False)
    nu, mu, cs = P[:, 4].copy(), P[:, 5].copy(), P[:, 6].copy()
    ds = pj.Dataset(t, y, yerr ** 2, ctx)
    g = ds.logl_grad(A, Bc, C, Dd, mu=mu, nu=nu, shift=cs)
    assert relerr(g["logl"], ds.logl_batch(A, Bc, C, Dd, mu=mu, nu=nu, shift=cs)) < 1e-12
    assert relerr(g["logl"], un["logl"][:5]) < 1e-9          # the reference's own values for these points
    for i in range(5):
        v = y - cs[i]
        Yt, St = np.log(v), yerr ** 2 / v ** 2
        ref = O.logl_dir(A[i], Bc[i], C, Dd, t, Yt - mu[i], nu[i] * St, dy=-1 / v, ds2=nu[i] * 2 * yerr ** 2 / v ** 3)
        assert abs(g["grad_shift"][i] - ref) <= 1e-8 * (1 + abs(ref)), (g["grad_shift"][i], ref)
        gi = pj.Dataset(t, Yt, St, ctx).logl_grad(A[i:i + 1], Bc[i:i + 1], C, Dd, mu=mu[i:i + 1], nu=nu[i:i + 1])
        for k in ("grad_a", "grad_b", "grad_mu", "grad_nu"):
            assert np.max(np.abs(g[k][i] - gi[k][0])) <= 1e-9 * (1 + np.max(np.abs(gi[k][0]))), k
    # y - c <= 0: status 2, as in the value-only entry
    bad = ds.logl_grad(A[:1], Bc[:1], C, Dd, mu=mu[:1], nu=nu[:1], shift=[y.min() + 1.0])
    assert bad["status"][0] == 2 and np.isnan(bad["logl"][0])
    # the same model with 36 and 52 components (72 / 104 rows): the step-by-step reverse mode with per-draw series (lean kernels, round 4)
    for Jw in (36, 52):
        A, Bc, C, Dd = pj.approx_batch(pj.SingleBendingPowerLaw, P[:2, :3], f_min, f_max, Jw, P[:2, 3], is_integrated_power=False)
        g = ds.logl_grad(A, Bc, C, Dd, mu=mu[:2], nu=nu[:2], shift=cs[:2])
        assert pj._lib.lib().pioran_celerite_config_name(-1).decode() == "wide (step-by-step gradient)" and (g["status"] == 0).all()
        assert relerr(g["logl"], ds.logl_batch(A, Bc, C, Dd, mu=mu[:2], nu=nu[:2], shift=cs[:2])) < 1e-11
        for i in range(2):
            v = y - cs[i]
            Yt, St = np.log(v), yerr ** 2 / v ** 2
            ref = O.logl_dir(A[i], Bc[i], C, Dd, t, Yt - mu[i], nu[i] * St, dy=-1 / v, ds2=nu[i] * 2 * yerr ** 2 / v ** 3)
            assert abs(g["grad_shift"][i] - ref) <= 1e-8 * (1 + abs(ref)), (Jw, g["grad_shift"][i], ref)
            gn = O.logl_dir(A[i], Bc[i], C, Dd, t, Yt - mu[i], nu[i] * St, ds2=St)
            assert abs(g["grad_nu"][i] - gn) <= 1e-8 * (1 + abs(gn))


def test_fp64_probe_leaves_the_callers_event_slots_alone(ctx):
    """pioran_ctx_fp64_probe (ABI 7): a plausible FP64 FMA rate, argument checks, and the caller's timing slots 0 .. 11 are not touched by it
    (it records into the context's internal slots)."""
    ctx.event_record(0)
    r = ctx.fp64_probe(2, 5.0)
    ctx.event_record(1)
    assert 20.0 < r < 90.0, r
    ms = ctx.event_elapsed_ms(0, 1)
    assert ms >= 1.0                      # the probe ran between the two records: had it re-recorded slot 0 or 1, this would be ~0 or an error
    L = pj._lib.lib()
    out = ctypes.c_double(0.0)
    assert L.pioran_ctx_fp64_probe(ctx._h, 0, 5.0, ctypes.byref(out)) != 0 and L.pioran_ctx_fp64_probe(ctx._h, 2, -1.0, ctypes.byref(out)) != 0
    assert L.pioran_ctx_fp64_probe(ctx._h, 2, 5.0, None) != 0
