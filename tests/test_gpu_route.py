"""GPU tests (-m gpu): capi.hip's launch() takes the family the routing rules name (csrc/route.hip, pioran_value_route) at every point of
tools/route_grid.py — the smallest shapes that cross every batch rule (N = 256) and every time-parallel threshold (N up to 4416) — and
the launch gives finite values with status 0; likewise the calls whose draws bring (c, d) of their own, against pioran_value_route_cd.  That the
plans are the ones the code made before the rules were separated is not a test here: docs/EXPERIMENTS.md sections 22 and 27 have the listings
against the parent's library."""
import importlib.util
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import pioran_jl_amd as pj  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]
_spec = importlib.util.spec_from_file_location("route_grid", ROOT / "tools" / "route_grid.py")
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)


@pytest.fixture(scope="module")
def ctx():
    return pj.Context(0)


def check(ctx, pts):
    seen = set()
    for pt in pts:
        want, plan = G.value_route(G.rows_of(pt), pt.J, pt.n_one, pt.B, pt.N, options=pt.options)
        got, out, st = G.run_point(ctx, pt)
        assert got == want, (pt, got, want, plan)
        assert np.isfinite(out).all() and (st == 0).all(), (pt, got)
        seen.add(got)
    return seen


def test_batch_rules(ctx):
    seen = check(ctx, G.batch_points())
    assert seen == {"tile", "block", "wide", "scan", "fallback"}


def test_time_parallel_thresholds(ctx):
    pts = G.tp_points()
    seen = check(ctx, pts)
    assert "tp" in seen and len(seen) > 1
    for pt in pts:     # the table's side of the threshold is the rule's (tests/test_route.py) — and so the launch's
        thr = G.TP_THRESHOLD[G.rows_of(pt)][G.TP_B.index(pt.B)]
        assert (G.value_route(G.rows_of(pt), pt.J, pt.n_one, pt.B, pt.N)[0] == "tp") == (pt.N >= thr)


def test_draws_with_their_own_cd(ctx):
    """Dataset.logl_batch with C, Dd per draw — all terms or a few of them differing (mixed mode) — Dataset.logpdf_theta with QPO features, whose
    mixed mode must run, and Dataset.logpdf_carma, whose coefficients are made on the device: the family pioran_value_route_cd names (route.hip
    mixed_plan, perdraw_form), at N = 130 (nine windows, the last ragged)."""
    seen = set()
    for pt in G.carma_points():
        got, out, st, (_, Bc, C, Dd) = G.run_carma_point(ctx, pt)
        want = G.carma_expected(pt, Bc, C, Dd)
        assert got == want, (pt, got, want)
        assert np.isfinite(out).all() and (st == 0).all(), (pt, got)
        seen.add(got)
    for pt in G.cd_points() + G.theta_points():
        want = G.expected(pt)
        got, out, st = G.run_point(ctx, pt)
        assert got == want, (pt, got, want)
        assert np.isfinite(out).all() and (st == 0).all(), (pt, got)
        seen.add(got)
    assert seen == {"block+pd", "block (per-draw tables)", "wide (per-draw tables)", "wide", "scan", "fallback"}

