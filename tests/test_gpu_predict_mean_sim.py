"""GPU tests (-m gpu) of the posterior mean (pioran_celerite_predict: Dataset.predict behind pj.mean, pj.predict and every posterior predictive
check) and of the simulation (pioran_celerite_simulate: Context.simulate behind pj.rand, pj.simulate, pj.lsp_ppc) against truths that are
neither the kernels nor a restatement of their recurrences: oracle.predict_mean_truth and oracle.sim_truth, dense in long double.

Cases, checkers and the reasoning behind the bound max(20 x ref_dev, 256 eps) live in tests/predict_mean_cases.py; the CPU suite
(tests/test_predict_mean_sim_host.py) shows that the case list holds the edges it promises and catches seeded mistakes.  Every case runs on
every family of kernels that takes it, and the family that ran is asserted:
    default routing, (c, d) shared         block (windowed ...) up to 63 rows, wide (step-by-step ...) above
    default routing, (c, d) per draw       block (windowed ..., per-draw tables) where 2 J <= 63, else draw by draw on the shared route
    no_block, up to 63 rows                wide (step-by-step ...) at the same shapes
The mean is asked for with tau ascending (windowed: the fused evaluation while M <= N R) and with the same tau permuted (two passes).
Every figure is printed before it is asserted; test_zz_worst_deviation_per_path prints the table of docs/EXPERIMENTS.md."""
import functools
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import pioran_jl_amd as pj  # noqa: E402
from oracle import oracle as O  # noqa: E402

sys.path.insert(0, str(Path(__file__).resolve().parent))
import predict_mean_cases as PM  # noqa: E402

EDGE = list(PM.edge_cases())
WORST = {}          # path -> (deviation, bound, label)


@pytest.fixture(scope="module")
def ctx():
    return pj.Context(0)


def _rows(case):
    A, Dd = case[4], case[7]
    return 2 * A.shape[1] - int(np.sum(np.atleast_2d(Dd)[0] == 0.0)), A.shape[1]


def _family(case, what, no_block):
    """the family name the entry must report for this case"""
    R, J = _rows(case)
    if no_block or R > 63:
        return f"wide (step-by-step {what})"
    if np.ndim(case[6]) == 2 and len(case[4]) > 1 and 2 * J <= 63:
        return f"block (windowed {what}, per-draw tables)"
    return f"block (windowed {what})"


def _ran():
    return pj._lib.lib().pioran_celerite_config_name(-1).decode()


def _note(path, dev, case, what):
    """keeps, per path, the largest deviation met (with its bound and case)"""
    ref_dev = PM.reference(case, what)[1]
    k = int(np.argmax(dev))
    if path not in WORST or dev[k] > WORST[path][0]:
        WORST[path] = (float(dev[k]), float(max(PM.MARGIN * ref_dev[k], PM.FLOOR)), case[0])


def mean_impl(ctx, family):
    def impl(A, Bc, C, Dd, t, y, s2, mu, nu, tau):
        ds = pj.Dataset(t, y, s2, ctx)
        try:
            got, st = ds.predict(A, Bc, C, Dd, tau, mu=mu, nu=nu, return_status=True)
        finally:
            ds.close()
        assert _ran() == family, (_ran(), family)
        return got, st
    return impl


def sim_impl(ctx, family):
    def impl(A, Bc, C, Dd, t, s2, q):
        got = ctx.simulate(A, Bc, C, Dd, t, s2, q)          # (raises unless the entry returns 0: there is no status per draw)
        assert _ran() == family, (_ran(), family)
        return got, np.zeros(len(A), dtype=np.int32)
    return impl


def _legs(case, what):
    """(leg, the case as that leg sees it, no_block)"""
    R, _ = _rows(case)
    legs = [("shared", case, False)] if np.ndim(case[6]) == 1 else []
    legs.append(("per-draw", PM.per_draw_variant(case), False))
    if R <= 63:
        legs.append(("no_block", case, True))
    return legs


def run_mean(ctx, case):
    N, M = len(case[1]), len(case[10])
    R, _ = _rows(case)
    for leg, c, no_block in _legs(case, "prediction"):
        family = _family(c, "prediction", no_block)
        if no_block:
            ctx.set_option("no_block", "1")
        try:
            dev = PM.check_mean(mean_impl(ctx, family), c, leg=f"[{leg}: {family}]")
        finally:
            if no_block:
                ctx.set_option("no_block", None)
        if family.startswith("wide"):
            _note("mean, step by step" + (" (no_block)" if no_block else ""), dev.max(axis=0), c, "mean")
        else:
            pd = ", per-draw tables" if "per-draw" in family else ""
            fused = M <= N * R
            _note("mean, windowed, " + ("fused" if fused else "two passes (ascending tau, M > N R)") + pd, dev[0], c, "mean")
            if M > 1:
                _note("mean, windowed, two passes" + pd, dev[1], c, "mean")


def run_sim(ctx, case):
    for leg, c, no_block in _legs(case, "simulation"):
        family = _family(c, "simulation", no_block)
        if no_block:
            ctx.set_option("no_block", "1")
        try:
            dev = PM.check_sim(sim_impl(ctx, family), c, leg=f"[{leg}: {family}]")
        finally:
            if no_block:
                ctx.set_option("no_block", None)
        zero = ", sigma2 = 0" if not c[3].any() else ""
        if family.startswith("wide"):
            _note("simulation, step by step" + (" (no_block)" if no_block else "") + zero, dev, c, "sim")
        else:
            _note("simulation, windowed" + (", per-draw tables" if "per-draw" in family else "") + zero, dev, c, "sim")


# ---- 1 --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", EDGE, ids=lambda c: c[0])
def test_mean_edge_shapes_against_truth(ctx, case):
    """Dataset.predict at every edge shape of predict_mean_cases: (c, d) shared and per draw on the default route, and step by step under
    no_block where the rows fit the windowed kernels; each with tau ascending and permuted, sigma2 as drawn and x 1e-6."""
    run_mean(ctx, case)


# ---- 2 --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [sc for c in EDGE for sc in PM.sim_variants(c)], ids=lambda c: c[0])
def test_simulation_edge_shapes_against_truth(ctx, case):
    """Context.simulate at the same shapes and on the same families, with sigma2 as drawn, x 1e-6 and exactly zero (what pj.rand passes for new
    times)."""
    run_sim(ctx, case)


# ---- 3 --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(PM.fuzz_cases(40)), ids=lambda c: c[0])
def test_fuzz_against_truth(ctx, case):
    """40 seeded random shapes (R 1..64, N 1..300 with long gaps, M 1..60, 1..4 draws, sigma2 x 10^U(-7, 0)); (c, d) shared or per draw as the
    case says, each also per draw where it is shared, and step by step."""
    run_mean(ctx, case)
    run_sim(ctx, case)


# ---- 4 --------------------------------------------------------------------------------------------------------------------------------
def test_rand_at_new_times_against_truth(ctx):
    """pj.rand(rng, f(t, s2), t_new): a realisation at new times with zero variance added, on the generator's own normals, against sim_truth
    with s2 = 0 (+ the mean); N = 257: sixteen full windows and one step."""
    case = next(c for c in EDGE if c[0] == "R33-N257-mixed-s2x1")
    label, t, y, s2, A, Bc, C, Dd, mu, nu, tau, q = case
    zero = next(sc for sc in PM.sim_variants(case) if not sc[3].any())
    kernel = functools.reduce(lambda k, j: k + pj.Celerite(A[0][j], Bc[0][j], C[j], Dd[j]), range(1, len(C)), pj.Celerite(A[0][0], Bc[0][0], C[0], Dd[0]))
    assert all(np.array_equal(np.real(np.atleast_1d(v)), w) for v, w in zip(kernel.celerite_coefs(), (A[0], Bc[0], C, Dd)))
    fx = pj.ScalableGP(0.7, kernel)(np.linspace(0.0, 1.0, 5), np.full(5, 0.1))      # (the data of f do not enter a draw at new times)
    seed = 20261018
    assert np.array_equal(np.random.default_rng(seed).standard_normal(len(t)), np.random.default_rng(seed).standard_normal(len(t)))
    qq = np.random.default_rng(seed).standard_normal(len(t))
    got = pj.rand(np.random.default_rng(seed), fx, t, ctx=ctx)
    assert _ran() == "block (windowed simulation)"
    z = np.zeros(len(t))
    want = O.sim_truth(A[0], Bc[0], C, Dd, t, z, qq)
    scale = float(np.max(np.abs(want)))
    ref_dev = max(float(np.max(np.abs(r - want))) for r in (O.sim(A[0], Bc[0], C, Dd, t, z, qq), np.linalg.cholesky(PM._dense(A[0], Bc[0], C, Dd, t, z)) @ qq)) / scale
    dev = float(np.max(np.abs(got - 0.7 - want))) / scale
    bound = max(PM.MARGIN * ref_dev, PM.FLOOR)
    print(f"pj.rand at new times (R33-N257, sigma2 = 0): deviation {dev:.2e}   ref_dev {ref_dev:.2e}   bound {bound:.2e}")
    assert got.shape == (len(t),)
    assert dev <= bound, (dev, bound)
    WORST["simulation, pj.rand at new times"] = (dev, bound, zero[0])


# ---- 5 --------------------------------------------------------------------------------------------------------------------------------
def test_zz_worst_deviation_per_path():
    """The table: per path the largest deviation met, with its bound and case (runs last in this module; empty when the tests above were
    deselected)."""
    for path in sorted(WORST):
        dev, bound, label = WORST[path]
        print(f"WORST {path:58s} deviation {dev:.2e}   bound {bound:.2e}   {label}")
    assert all(d <= b for d, b, _ in WORST.values())
