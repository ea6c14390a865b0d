"""GPU tests (-m gpu) of log L and its gradient (pioran_celerite_logl_grad, pioran_celerite_logl_grad_shift: Dataset.logl_grad, what the HMC / NUTS
users call at every leapfrog step) against a truth that is neither the kernels nor a restatement of their recurrence: oracle.logl_grad_truth, dense in
long double, pinned to a 50-digit evaluation (tests/golden/grad_truth.npz).

Cases, checker and the reasoning behind the bound max(20 x ref_dev, 256 eps) live in tests/grad_cases.py; the CPU suite (tests/test_grad_host.py)
shows that the case list holds the edges it promises and that the checker catches seeded mistakes.  Every case runs on every reverse-mode family
that takes it, and the family that ran is asserted:
    default routing, (c, d) shared, with d/d(c, d) and the series gradients     block (windowed gradient) up to 63 rows, wide (step-by-step gradient) above
    the same with neither (the kernels' other instantiation)                    the same
    (c, d) per draw                                                             block (windowed gradient, per-draw tables) where 2 J <= 63, else draw by
                                                                                draw on the shared route
    no_block, up to 63 rows                                                     wide (step-by-step gradient): RPL 1 .. 4 (4: the lean adjoint kernel)
    no_wide2 (with no_block below 64 rows), 48 .. 95 rows                       wide (step-by-step gradient): the round-1 adjoint kernel
    scan_config = "tile", up to 63 rows, without and with d/d(c, d)             tile (windowed gradient, one draw per wavefront)
    shift per draw (four shapes)                                                block / wide by rows, grad_shift through the chain rule of table.hip
The bound is the common one but for grad_d of the step-by-step family, whose form has a deviation of its own (grad_cases.wide_bounds, set from
tools/wide_adjoint_dd_proto.py on the CPU).  The value log L of every leg goes through the same check.  grad_b_j and grad_d_j of a one-row term (b_j = d_j = 0) must be exactly 0.0 on every leg
(grad_cases.check asserts it with ==).  Every figure is printed before it is asserted; test_zz_worst_deviation_per_family prints the table of
docs/EXPERIMENTS.md."""
import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import pioran_jl_amd as pj  # noqa: E402

sys.path.insert(0, str(Path(__file__).resolve().parent))
import grad_cases as GC  # noqa: E402

EDGE = list(GC.edge_cases())
WORST = {}          # (path, key) -> (deviation, bound, label)
BLOCK, WIDE, TILE = "block (windowed gradient)", "wide (step-by-step gradient)", "tile (windowed gradient, one draw per wavefront)"
PER_DRAW = "block (windowed gradient, per-draw tables)"
PLAIN_KEYS = ("logl", "grad_a", "grad_b", "grad_mu", "grad_nu")


@pytest.fixture(scope="module")
def ctx():
    return pj.Context(0)


def _ran():
    return pj._lib.lib().pioran_celerite_config_name(-1).decode()


def _note(path, dev, case, bounds):
    """keeps, per path and key, the largest deviation met (with its bound and case)"""
    for key, v in dev.items():
        k = int(np.argmax(v))
        if (path, key) not in WORST or v[k] > WORST[path, key][0]:
            WORST[path, key] = (float(v[k]), float(GC.bound_of(case, key, bounds)[k]), case[0])


def grad_impl(ctx, family, **kw):
    def impl(case):
        label, t, y, s2, A, Bc, C, Dd, mu, nu, shift = case
        ds = pj.Dataset(t, y, s2, ctx)
        try:
            g = ds.logl_grad(A, Bc, C, Dd, mu=mu, nu=nu, shift=shift, **kw)
        finally:
            ds.close()
        assert _ran() == (family() if callable(family) else family), (label, _ran(), family)
        return g
    return impl


def legs(case):
    """(path of the table, the case as the leg sees it, context options, arguments of logl_grad, keys, the family that must run)"""
    R, J, B = GC.rows(case), case[4].shape[1], len(case[4])
    by_rows = BLOCK if R <= 63 else WIDE
    full, none = dict(cd_grad=True, series_grad=True), dict(cd_grad=False, series_grad=False)
    if case[10] is not None:
        return [(f"shift per draw, {by_rows}", case, {}, dict(cd_grad=True), GC.keys_of(case), by_rows)]
    out = [(by_rows, case, {}, full, GC.keys_of(case), by_rows),
           (f"{by_rows}, neither d/d(c, d) nor series", case, {}, none, PLAIN_KEYS, by_rows)]
    pd = GC.per_draw_variant(case)
    if B > 1 and 2 * J <= 63:
        out.append((PER_DRAW, pd, {}, full, GC.keys_of(pd), PER_DRAW))
    else:
        out.append((f"(c, d) per draw, draw by draw: {by_rows}", pd, {}, full, GC.keys_of(pd), by_rows))
    if R <= 63:
        out.append((f"no_block: {WIDE}, RPL {GC.rpl_of(R)}", case, {"no_block": "1"}, full, GC.keys_of(case), WIDE))
    if 48 <= R <= 95:
        opts = {"no_wide2": "1", **({"no_block": "1"} if R <= 63 else {})}
        out.append((f"no_wide2: {WIDE}, round-1 adjoint kernel", case, opts, full, GC.keys_of(case), WIDE))
    if R <= 63:
        out.append((TILE, case, {"scan_config": "tile"}, none, PLAIN_KEYS, TILE))
        out.append((f"{TILE}, with d/d(c, d)", case, {"scan_config": "tile"}, dict(cd_grad=True), PLAIN_KEYS + ("grad_c", "grad_d"), TILE))
    return out


def default_family(ctx, case):
    """What the default routing must take.  Up to 63 rows the windowed kernels, above the step-by-step ones; a model of mostly one-row terms can
    have up to 63 rows and more terms than the 32 of a full two-row model, and the windowed kernels keep 2 KB of LDS per term beside their tiles
    (pioran_block_fits): with more than 32 terms either family may run, and the one that does is what the leg is held to."""
    R, J = GC.rows(case), case[4].shape[1]
    if R > 63 or J <= 32:
        return BLOCK if R <= 63 else WIDE
    grad_impl(ctx, _ran, cd_grad=False)(GC.one_draw(case, 0))
    assert _ran() in (BLOCK, WIDE), _ran()
    return _ran()


def run(ctx, case, only_default=False):
    """every leg of the case; a leg that fails does not keep the others from running (all failures are raised together at the end)"""
    failed = []
    for path, c, opts, kw, keys, family in legs(case)[:1 if only_default else None]:
        if only_default:
            path = family = default_family(ctx, case)
        try:
            for key, value in opts.items():
                ctx.set_option(key, value)
            bounds = GC.wide_bounds(c) if family == WIDE and "grad_d" in keys else None      # (the form's own deviation: grad_cases)
            _note(path, GC.check(grad_impl(ctx, family, **kw), c, keys=keys, leg=f"[{path}]", bounds=bounds), c, bounds)
        except AssertionError as e:
            print(f"FAILED {c[0]} [{path}]: {e}")
            failed.append((path, str(e)))
        finally:
            for key in opts:
                ctx.set_option(key, None)
    assert not failed, failed


# ---- 1 --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", EDGE, ids=lambda c: c[0])
def test_edge_shapes_against_truth(ctx, case):
    """Dataset.logl_grad at every edge shape of grad_cases on every family that takes it (legs()), sigma2 as drawn and x 1e-6: the value and every
    gradient within max(20 x ref_dev, 256 eps) of the long-double truth in the output's natural scale; exact zeros at the one-row terms."""
    run(ctx, case)


# ---- 2 --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(GC.fuzz_cases(40)), ids=lambda c: c[0])
def test_fuzz_against_truth(ctx, case):
    """40 seeded random shapes (R 1 .. 143, N 1 .. 200, one-row terms at random places, sigma2 x 10^U(-6, 0)) through the default routing, with
    d/d(c, d) and the series gradients; every one of them has a truth and references (tests/test_grad_host.py: none is left out)."""
    run(ctx, case, only_default=True)


# ---- 3 --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("leg", ["block", "per-draw tables", "tile", "wide", "no_block", "no_wide2"])
def test_every_entry_of_the_outputs_is_written(ctx, leg):
    """pioran_celerite_logl_grad called with every output array filled with NaN beforehand (Dataset.logl_grad hands over np.empty): no family leaves
    an entry of the caller's memory as it was — the one-row terms' grad_b and grad_d included, which come back as 0.0."""
    label = {"wide": "R65-N18-s2x1", "no_wide2": "R49-N17-s2x1"}.get(leg, "R33-N17-s2x1")
    case = next(c for c in EDGE if c[0] == label)
    if leg == "per-draw tables":
        case = GC.per_draw_variant(case)
    label, t, y, s2, A, Bc, C, Dd, mu, nu, shift = case
    opts = {"tile": {"scan_config": "tile"}, "no_block": {"no_block": "1"}, "no_wide2": {"no_wide2": "1", "no_block": "1"}}.get(leg, {})
    family = {"block": BLOCK, "per-draw tables": PER_DRAW, "tile": TILE}.get(leg, WIDE)
    B, J, N = len(A), A.shape[1], len(t)
    assert (Dd == 0.0).any()
    f = lambda *shape: np.full(shape, np.nan)
    out, st = f(B), np.full(B, -1, dtype=np.int32)
    ga, gb, gc, gd, gnu, gmu = f(B, J), f(B, J), f(B, J), f(B, J), f(B), f(B)
    gy, gs = (None, None) if leg == "tile" else (f(B, N), f(B, N))          # (the tile family takes no series gradients)
    P = lambda v: None if v is None else ctypes.c_void_p(np.ascontiguousarray(v).ctypes.data)   # noqa: E731
    arrays = [np.ascontiguousarray(v, dtype=np.float64) for v in (A, Bc, C, Dd, mu, nu)]
    ds = pj.Dataset(t, y, s2, ctx)
    try:
        for key, value in opts.items():
            ctx.set_option(key, value)
        rc = pj._lib.lib().pioran_celerite_logl_grad(ds._h, B, J, *map(P, arrays[:4]), int(np.ndim(C) == 1), P(arrays[4]), P(arrays[5]), P(out), P(st),
                                                     P(ga), P(gb), P(gc), P(gd), P(gnu), P(gmu), P(gy), P(gs))
    finally:
        for key in opts:
            ctx.set_option(key, None)
        ds.close()
    assert rc == 0 and _ran() == family, (rc, _ran())
    assert (st == 0).all()
    for name, v in (("logl", out), ("grad_a", ga), ("grad_b", gb), ("grad_c", gc), ("grad_d", gd), ("grad_nu", gnu), ("grad_mu", gmu), ("grad_y", gy), ("grad_sigma2", gs)):
        assert v is None or np.isfinite(v).all(), (leg, name)
    zero = GC.structural_zeros(case)
    assert (gb[zero] == 0.0).all() and (gd[zero] == 0.0).all()
    got = {"logl": out, "status": st, "grad_a": ga, "grad_b": gb, "grad_c": gc, "grad_d": gd, "grad_nu": gnu, "grad_mu": gmu, "grad_y": gy, "grad_sigma2": gs}
    GC.check(lambda c: got, case, keys=[k for k in GC.keys_of(case) if got[k] is not None], leg=f"[NaN-filled outputs, {leg}]",
             bounds=GC.wide_bounds(case) if family == WIDE else None)


# ---- 4 --------------------------------------------------------------------------------------------------------------------------------
def test_zz_worst_deviation_per_family():
    """The table: per family and output the largest deviation met, with its bound and case (runs last in this module; empty when the tests above
    were deselected)."""
    for path, key in sorted(WORST):
        dev, bound, label = WORST[path, key]
        print(f"WORST {path:84s} {key:12s} deviation {dev:.2e}   bound {bound:.2e}   {label}")
    assert all(d <= b for d, b, _ in WORST.values())
