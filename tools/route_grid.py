#!/usr/bin/env python3
"""The launches that cross every routing rule of the value path (csrc/route.hip), at the smallest shapes that still do.

Importable: `points()` is the grid of tests/test_gpu_route.py, `run_point` makes one launch through the Python API, `value_route` asks
pioran_value_route; `cd_points()` / `theta_points()` / `carma_points()` are the launches whose draws bring (c, d) of their own, `value_route_cd`
asks pioran_value_route_cd.  As a program it runs the grid and prints, per point, the kernel family that ran and a hash of the log L and status
arrays — a different segment count, mode or chunking changes bits, so two libraries with equal listings made equal plans:

    PIORAN_HIP_LIB=/path/to/other/libpioran_hip.so python tools/route_grid.py [--before-value-route] [--before-value-route-cd] > listing.txt

(--before-value-route[-cd]: the library is from before pioran_value_route[_cd] existed; the binding does not ask for the symbol.)

`step_route` asks pioran_step_route, one level below the families: the kernel instantiation a throughput- or latency-layout launch runs;
`step_points()` / `run_step_point` are the launches of tests/test_gpu_step_route.py, listed with `--steps`.

`entry_points()` is the grid of tests/test_gpu_entry_route.py — posterior mean and variance, value and gradient, simulation, posterior draws —
`run_entry_point` makes one call, `entry_route` asks pioran_entry_route.  `--entries [--save FILE.npz] [--against FILE.npz]` lists that grid
instead: name, return code and a hash of the outputs per point; the gradient arrays are saved / compared with the saved ones
(--before-entry-route: the library is from before pioran_entry_route existed).  `--steps` lists step_points() the same way
(--before-step-route: the library is from before pioran_step_route existed).

`window_route` asks pioran_window_route: the instantiations of the windowed kernels, their one-draw-per-wavefront form and the time-parallel family;
`window_points()` / `run_window_point` are the launches of tests/test_gpu_window_route.py, listed behind the others by `--steps`
(--before-window-route: the library is from before pioran_window_route existed; the name that ran, pioran_celerite_config_name(-2), is then not listed).
"""
import ctypes
import hashlib
import itertools
import sys
from collections import namedtuple
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

# rows = 2 J - n_one active rows; options: "key=value;key=value" as pioran_value_route takes them
Point = namedtuple("Point", "J n_one B N options")
# (c, d) per draw: the LAST npd of the J terms differ between the draws (npd = J: all of them), no one-row terms
CdPoint = namedtuple("CdPoint", "J npd B N options")
# pioran_logpdf_batch_theta: n_qpo QPO features on a continuum of n_components SHO terms (mixed mode that must run)
ThetaPoint = namedtuple("ThetaPoint", "n_components n_qpo B N")
# pioran_logpdf_batch_carma: CARMA(p, q) from sampled parameters; which terms are per draw is read off the coefficients the call returns
CarmaPoint = namedtuple("CarmaPoint", "p q B N options shift")


def rows_of(pt):
    return 2 * pt.J - pt.n_one


def _terms(rows):
    """All terms with both rows, except 60 rows: 20 two-row and 20 one-row terms (DRWCelerite-20)."""
    return (40, 20) if rows == 60 else (rows // 2, 0)


# ---- N = 256: below every time-parallel threshold, only the batch rules decide.  No point needs the occupancy figure `pass`: rows 33 .. 38 and 48
# stay at one pass's draws, and no batch exceeds a pass ------------------------------------------------------------------------------------------
BATCH_N = 256
BATCH_ROWS = (2, 4, 6, 16, 32, 40, 48, 60, 64, 80, 96, 128)
BATCH_B = (1, 8, 256, 512, 513, 768, 1024)
# (rows, B) repeated under options that take a family out of the ladder or force one
BATCH_VARIANTS = (("no_block=1", ((6, 8), (40, 256), (60, 513), (80, 8), (32, 768))),
                  ("no_tile=1", ((40, 1024), (60, 513), (80, 1024), (32, 768))),
                  ("no_wide=1;no_block=1", ((16, 8), (40, 256), (80, 256), (80, 1024))),
                  ("scan_config=block", ((4, 8), (40, 1024), (60, 768), (80, 513))))

# ---- the time-parallel family: per (state rows, draws) the shortest series, in steps of 64, that it takes by default — every term with both
# rows, shared series.  tests/test_route.py holds this table to the rules; the grid runs N = threshold and threshold - 64 ------------------------
TP_B = (1, 2, 4, 8)
TP_THRESHOLD = {2: (1024, 1024, 1024, 1024), 4: (1024, 1024, 1024, 1024), 8: (1024, 1024, 2048, 2048), 16: (1024, 1024, 2048, 1600),
                24: (1536, 1536, 2048, 2112), 40: (3072, 3072, 2880, 4416), 64: (2048, 2048, 2176, 2560)}


def batch_points():
    pts = []
    for rows in BATCH_ROWS:
        for B in BATCH_B + ((2048,) if rows >= 39 and rows != 48 else ()):
            pts.append(Point(*_terms(rows), B, BATCH_N, ""))
    pts += [Point(72, 0, B, BATCH_N, "") for B in (1, 8, 64)]      # 144 rows: past every register-resident kernel
    for options, cases in BATCH_VARIANTS:
        pts += [Point(*_terms(rows), B, BATCH_N, options) for rows, B in cases]
    return pts


def tp_points():
    return [Point(rows // 2, 0, B, N, "") for rows, thr in TP_THRESHOLD.items() for B, n in zip(TP_B, thr) for N in (n - 64, n)]


def points():
    return batch_points() + tp_points()


# ---- (c, d) per draw.  N = 130: nine 16-step windows, the last ragged.  All terms per draw: the ends of the windowed kernel with per-draw rows
# (J <= 2), of the per-draw windowed tables (6 .. 63 rows, up to 768 draws), of the table-less scan (up to 79 rows), the latency kernel's tables
# from 80 rows on, 144 rows; mixed: both sides of the windowed kernel's batch limits (512 from six rows on, 768 below), three per-draw terms on the
# combined table (from 16 draws on), more per-draw terms than half (generic path), nine (past mixed mode's eight); force_fallback leaves the combined table on the scan -------------------------------
CD_N = 130
CD_ALL = ((1, (8, 768, 769)), (2, (8,)), (3, (8, 768, 769)), (31, (8,)), (32, (8,)), (39, (8,)), (40, (8,)), (71, (8,)), (72, (8,)))
CD_MIXED = ((5, 1, (8, 512, 513)), (2, 1, (768, 769)), (8, 3, (8, 16, 37)), (8, 5, (37,)), (12, 9, (37,)))
CD_VARIANTS = ((5, 1, 8, "no_block=1"), (5, 1, 8, "no_mixed=1"), (5, 1, 8, "scan_config=block"), (3, 3, 8, "no_block=1"),
               (3, 3, 1000, "scan_config=block"), (8, 3, 37, "force_fallback=1"))


def cd_points():
    pts = [CdPoint(J, J, B, CD_N, "") for J, Bs in CD_ALL for B in Bs]
    pts.append(CdPoint(40, 40, 300, 24, ""))        # two chunks of per-draw tables (256 + 44)
    pts += [CdPoint(J, npd, B, CD_N, "") for J, npd, Bs in CD_MIXED for B in Bs]
    pts += [CdPoint(J, npd, B, CD_N, options) for J, npd, B, options in CD_VARIANTS]
    return pts


def theta_points():
    return [ThetaPoint(5, n_qpo, 8, CD_N) for n_qpo in (1, 3)]


def carma_points():
    """One draw (the shared case); a few draws, also with mixed mode switched off and on per-draw series; more than one chunk; five roots; an even p
    (no term with one row)."""
    return [CarmaPoint(3, 2, 1, CD_N, "", False), CarmaPoint(3, 2, 7, CD_N, "", False), CarmaPoint(3, 2, 7, CD_N, "no_mixed=1", False),
            CarmaPoint(3, 2, 7, CD_N, "", True), CarmaPoint(3, 2, 300, CD_N, "", False), CarmaPoint(5, 2, 16, CD_N, "", False),
            CarmaPoint(4, 3, 5, CD_N, "", False)]


# ---- the other batched entries (route.hip entry_plan).  N = 130: nine 16-step windows, the last ragged; M = 7 evaluation times, one on a data time.
# Rows at the smallest values where a rule flips: 4; 16 / 18 either side of the tile reverse mode's 17; 40; 60 as DRWCelerite-20 (three draws per
# workgroup there); 62 / 64 either side of the windowed kernels; 80: step by step only; 144: refused.  Batches either side of the gradient's 512 and of
# the 256-draw chunk.  The base grid asks the gradient without d/d(c, d) -----------------------------------------------------------------------------
EntryPoint = namedtuple("EntryPoint", "entry J n_one B per_draw shift cd_grad series options")
ENTRIES = ("predict", "predict_var", "grad", "simulate", "rand_posterior")
ENTRY_N, ENTRY_M = 130, 7
# what pioran_celerite_config_name(-1) reports after these entries, per entry: step by step, windowed, windowed with per-draw tables, tile
ENTRY_NAME_TABLE = {
    "predict": ("wide (step-by-step prediction)", "block (windowed prediction)", "block (windowed prediction, per-draw tables)"),
    "predict_var": ("wide (step-by-step variance)",),
    "grad": ("wide (step-by-step gradient)", "block (windowed gradient)", "block (windowed gradient, per-draw tables)",
             "tile (windowed gradient, one draw per wavefront)"),
    "simulate": ("wide (step-by-step simulation)", "block (windowed simulation)", "block (windowed simulation, per-draw tables)"),
    "rand_posterior": ("wide (step-by-step posterior draw)", "block (windowed posterior draw)"),
}
ENTRY_ROWS = (4, 16, 18, 40, 60, 62, 64, 80, 144)
ENTRY_B = {"grad": (1, 8, 512, 513)}
ENTRY_OPTION_VARIANTS = ("no_block=1", "no_tile=1", "scan_config=tile", "scan_config=block")


def entry_points():
    def pt(entry, rows, B, per_draw=False, shift=False, cd_grad=False, series=False, options=""):
        return EntryPoint(entry, *_terms(rows), B, per_draw, shift, cd_grad, series, options)
    pts = [pt(e, rows, B) for rows in ENTRY_ROWS for e in ENTRIES for B in ENTRY_B.get(e, (1, 8, 257))]
    pts.append(pt("grad", 4, 1025, options="no_block=1"))        # two chunks of the step-by-step reverse mode
    pts.append(pt("grad", 16, 257, per_draw=True))               # two chunks of per-draw tables
    # 40 rows under the options: every entry at 8 draws, the gradient also past 512 (but scan_config=tile: it forces the family at any size)
    for options in ENTRY_OPTION_VARIANTS:
        pts += [pt(e, 40, 8, options=options) for e in ENTRIES]
        if options != "scan_config=tile":
            pts.append(pt("grad", 40, 513, options=options))
    for B in (8, 513):
        pts += [pt("grad", 40, B, shift=True), pt("grad", 40, B, cd_grad=True), pt("grad", 40, B, series=True)]
    # (c, d) per draw: 8 terms on per-draw tables; 40 terms are 80 rows, refused, so draw by draw
    pts += [pt(e, rows, 8, per_draw=True) for rows in (16, 80) for e in ENTRIES]
    return pts


def entry_expected(pt):
    """(name, chunk cap, shrink) of pioran_entry_route for an EntryPoint."""
    return entry_route(pt.entry, rows_of(pt), pt.J, pt.n_one, pt.B, pt.per_draw, pt.shift, pt.cd_grad, pt.cd_grad, pt.series, pt.options)


def run_entry_point(ctx, pt):
    """One call of the entry through the Python API under the point's options: (name that ran, return code, dict of outputs)."""
    import pioran_jl_amd as pj
    shape = Point(pt.J, pt.n_one, pt.B, ENTRY_N, "")
    t, y, s2, A, Bc, C, Dd, mu, nu = inputs_cd(CdPoint(pt.J, pt.J, pt.B, ENTRY_N, "")) if pt.per_draw else inputs(shape)
    rng = np.random.default_rng([pt.J, pt.n_one, pt.B, ENTRY_N, 3])
    tau = np.concatenate([rng.uniform(t[0] - 1, t[-1] + 1, ENTRY_M - 1), t[[ENTRY_N // 2]]])
    q_data, q_new, eps = rng.standard_normal((pt.B, ENTRY_N)), rng.standard_normal((pt.B, ENTRY_M)), rng.standard_normal((pt.B, ENTRY_N))
    if pt.shift:        # the shifted log-flux form: the data set holds a positive series, every shift lies below its minimum
        y = np.exp(0.5 * y)
    opts = [kv.split("=") for kv in pt.options.split(";") if kv]
    ds = pj.Dataset(t, y, s2, ctx)
    try:
        for k, v in opts:
            ctx.set_option(k, v)
        if pt.entry == "predict":
            mean, st = ds.predict(A, Bc, C, Dd, tau, mu=mu, nu=nu, return_status=True)
            out = dict(mean=mean, status=st)
        elif pt.entry == "predict_var":
            var, st = ds.predict_var(A, Bc, C, Dd, tau, nu=nu, return_status=True)
            out = dict(var=var, status=st)
        elif pt.entry == "simulate":
            out = dict(y=ctx.simulate(A, Bc, C, Dd, t, s2, q_data))
        elif pt.entry == "rand_posterior":
            draws, st = ds.rand_posterior(A, Bc, C, Dd, tau, q_data, q_new, eps, mu=mu, nu=nu, return_status=True)
            out = dict(draws=draws, status=st)
        else:
            shift = y.min() * np.linspace(0.1, 0.9, pt.B) if pt.shift else None
            out = ds.logl_grad(A, Bc, C, Dd, mu=mu, nu=nu, series_grad=pt.series, shift=shift, cd_grad=pt.cd_grad)
            out = {k: v for k, v in out.items() if v is not None}
        return pj._lib.lib().pioran_celerite_config_name(-1).decode(), 0, out
    except pj._lib.PioranHipError as e:
        return None, int(str(e).split()[2].rstrip(":")), {}
    finally:
        for k, _ in opts:
            ctx.set_option(k, None)
        ds.close()


def value_route(rows, J, n_one, B, N, per_draw_series=False, pass_draws=0, options=""):
    """(family, (scan, RP, nseg, L)) of pioran_value_route."""
    import pioran_jl_amd as pj
    name = ctypes.create_string_buffer(64)
    tp = (ctypes.c_int32 * 4)()
    rc = pj._lib.lib().pioran_value_route(rows, J, n_one, B, N, int(per_draw_series), pass_draws, options.encode(), name, len(name), tp)
    if rc:
        raise ValueError(f"pioran_value_route: error {rc}")
    return name.value.decode(), tuple(tp)


def value_route_cd(n_two, n_one, npd, B, N, per_draw_series=False, must_run=False, options=""):
    """(family, mixed chunk) of pioran_value_route_cd; family None: must_run and mixed mode refuses."""
    import pioran_jl_amd as pj
    name = ctypes.create_string_buffer(64)
    chunk = ctypes.c_int64(0)
    rc = pj._lib.lib().pioran_value_route_cd(n_two, n_one, npd, B, N, int(per_draw_series), int(must_run), options.encode(), name, len(name),
                                             ctypes.byref(chunk))
    if rc not in (0, -4):
        raise ValueError(f"pioran_value_route_cd: error {rc}")
    return (name.value.decode() if rc == 0 else None), chunk.value


def entry_route(entry, rows, J, n_one, B, per_draw=False, shift=False, want_c=True, want_d=True, series_grads=False, options=""):
    """(name, chunk cap, shrink) of pioran_entry_route; name None: the entry refuses the rows."""
    import pioran_jl_amd as pj
    name = ctypes.create_string_buffer(64)
    cap, shrink = ctypes.c_int64(0), ctypes.c_int(0)
    rc = pj._lib.lib().pioran_entry_route(entry.encode(), rows, J, n_one, B, int(per_draw), int(shift), int(want_c), int(want_d), int(series_grads),
                                          options.encode(), name, len(name), ctypes.byref(cap), ctypes.byref(shrink))
    if rc not in (0, -4):
        raise ValueError(f"pioran_entry_route: error {rc}")
    return (name.value.decode() if rc == 0 else None), cap.value, bool(shrink.value)


def step_route(family, R, standard_rows=0, n_complex=0, B=1, shared=True, npd_rows=0, per_draw_tables=False, options=""):
    """(name, plan) of pioran_step_route — the kernel instantiation of a step-by-step launch: family "scan" (throughput layout) or the latency
    layout's "value", "store", "simulate", "gradient".  name: what pioran_celerite_config_name(0) reports after the launch, None where the family
    refuses.  plan, scan: (configuration's index, steps per pass, shared table, per-draw rows, y as a vector, pairs per block, a kernel exists,
    rows the configuration holds); latency: (rows per lane, lean forward kernel, y as a vector, lean reverse pass, 0 ...)."""
    import pioran_jl_amd as pj
    name = ctypes.create_string_buffer(64)
    plan = (ctypes.c_int32 * 8)()
    rc = pj._lib.lib().pioran_step_route(family.encode(), R, standard_rows, n_complex, B, int(shared), npd_rows, int(per_draw_tables), options.encode(),
                                         name, len(name), plan)
    if rc not in (0, -4):
        raise ValueError(f"pioran_step_route: error {rc}")
    return (name.value.decode() if rc == 0 else None), tuple(plan)


# ---- one level below the families: the grid tests/golden/step_route_listing.json was recorded over, from the commit before scan_plan / wide_plan
# existed (tools/experiments/step_route_listing.py), and tests/test_route.py holds pioran_step_route to ---------------------------------------------
_SCAN_SHAPES = ((1, 1, 5), (1, 1, 9), (1, 1, 13), (1, 1, 16), (2, 1, 9), (2, 1, 11), (2, 1, 13), (2, 1, 15), (2, 1, 16), (3, 2, 6), (3, 2, 7), (3, 2, 8),
                (4, 4, 4), (5, 4, 4))
_SCAN_Y_SHAPES = ((1, 1, 16), (2, 1, 16), (3, 2, 8), (4, 4, 4), (5, 4, 4))
SCAN_CONFIG_NAMES = tuple(f"rpl{r}_cbr{c}_nsrc{n}{sfx}" for shapes, sfxs in ((_SCAN_SHAPES, ("", "_p")), (_SCAN_Y_SHAPES, ("_y", "_yp")))
                          for r, c, n in shapes for sfx in sfxs) + ("rpl4_cbr4_nsrc4_b5a", "rpl3_cbr4_nsrc4", "rpl2_cbr2_nsrc8")
STEP_SCAN_ROWS = range(1, 81)
STEP_SCAN_OPTIONS = ("", "no_win2=1", "win2=1", "win3=1", "no_win3=1", "no_paired=1") + tuple(f"scan_config={n}" for n in SCAN_CONFIG_NAMES)
STEP_WIDE_ROWS = range(1, 145)
STEP_WIDE_MODES = ("value", "store", "simulate", "gradient")


def step_n_complex(kind, R):
    """Two-row terms of the row map 'n_complex two-row terms, then one-row terms' (kind 2) of R rows: a third — 60 rows are DRWCelerite-20."""
    return R // 3 if kind == 2 else 0


def step_scan_keys():
    """(row-map kind, B, shared table, per-draw rows, options): every R of STEP_SCAN_ROWS is asked under each."""
    return list(itertools.product((0, 1, 2), (1, 2048, 2049), (1, 0), (0, 2), STEP_SCAN_OPTIONS))


def step_wide_keys():
    """(mode, per-draw rows, per-draw tables, options): every R of STEP_WIDE_ROWS is asked under each."""
    return list(itertools.product(STEP_WIDE_MODES, (0, 2), (0, 1), ("", "wide2=1", "no_wide2=1")))


def step_runs(answers):
    """Runs of equal answers over consecutive rows: [[first row, last row, answer], ...] of a list of (row, answer)."""
    runs = []
    for R, a in answers:
        if runs and runs[-1][2] == a and runs[-1][1] == R - 1:
            runs[-1][1] = R
        else:
            runs.append([R, R, a])
    return runs


def step_scan_answer(key, R):
    """What the listing holds per scan query: [name, steps per pass, shared table, per-draw rows, y as a vector, pairs per block], None: refused."""
    kind, B, shared, npd, options = key
    name, plan = step_route("scan", R, kind, step_n_complex(kind, R), B, shared, npd, False, options)
    return None if name is None else [name, *plan[1:6]]


def step_wide_answer(key, R):
    """... per latency query: the kernels in launch order as [template, rows per lane, y as a vector, mode], None: refused."""
    mode, npd, per_draw_tables, options = key
    name, (rpl, lean, ycol, lean_adjoint, *_) = step_route(mode, R, 0, 0, 1, True, npd, per_draw_tables, options)
    if name is None:
        return None
    m = STEP_WIDE_MODES.index(mode)
    kernels = [["celerite_wide2_kernel" if lean else "celerite_wide_kernel", rpl, ycol, m]]
    if mode == "gradient":
        kernels.append(["celerite_adjoint2_kernel" if lean_adjoint else "celerite_adjoint_kernel", rpl, 0, 0])
    return [name, kernels]


# ---- the launches of tests/test_gpu_step_route.py: one on each side of every rule of scan_plan / wide_plan.  N = 37; the one-row terms are the LAST
# ones (the row map "two-row terms, then one-row terms": an odd row count has one, the 60-row shape is DRWCelerite-20) ---------------------------------
StepPoint = namedtuple("StepPoint", "family J n_one B options")
STEP_N, STEP_M = 37, 5
STEP_TO_SCAN = "no_tile=1;no_block=1;no_wide=1"
STEP_SCAN_POINT_ROWS = (15, 16, 23, 24, 31, 32, 47, 48, 63, 64, 79, 80)


def step_points():
    def pt(family, rows, B, options):
        return StepPoint(family, (rows + 1) // 2, rows % 2, B, options)
    # the throughput layout: the batch classes where the rule reads B (the mid-batch shape and the three-step form: 24 .. 31 rows) and beside them
    pts = [pt("scan", rows, B, STEP_TO_SCAN) for rows in STEP_SCAN_POINT_ROWS for B in ((5, 2048, 2049) if 23 <= rows <= 32 else (5,))]
    pts.append(StepPoint("scan", 40, 20, 5, STEP_TO_SCAN))
    # the latency layout at three draws: value, store (the prediction's factor), simulate, gradient, rows either side of 48, 64 and 96 ...
    pts += [pt(mode, rows, 3, "no_tile=1;no_block=1") for mode in STEP_WIDE_MODES for rows in (47, 48, 63, 64, 95, 96)]
    # ... and where only an option tells the sides apart
    pts += [pt("value", 47, 3, "no_block=1;wide2=1"), pt("value", 48, 3, "no_block=1;no_wide2=1"), pt("simulate", 64, 3, "no_wide2=1"),
            pt("gradient", 47, 3, "no_block=1;wide2=1"), pt("gradient", 95, 3, "no_wide2=1"), pt("gradient", 96, 3, "no_wide2=1")]
    return pts


def step_expected(pt):
    """The name pioran_step_route gives the point's launch."""
    rows = 2 * pt.J - pt.n_one
    if pt.family == "scan":
        return step_route("scan", rows, 2 if pt.n_one else 1, pt.J - pt.n_one, pt.B, True, 0, False, pt.options)[0]
    return step_route(pt.family, rows, options=pt.options)[0]


def run_step_point(ctx, pt):
    """One call that reaches the point's launch: (family that ran, pioran_celerite_config_name(0) after it, the outputs that are one workgroup's
    or one wavefront's sums — the gradient arrays are left out)."""
    import pioran_jl_amd as pj
    t, y, s2, A, Bc, C, Dd, mu, nu = inputs(Point(pt.J, 0, pt.B, STEP_N, ""))
    if pt.n_one:
        Bc[:, -pt.n_one:] = 0.0
        Dd[-pt.n_one:] = 0.0
    rng = np.random.default_rng([pt.J, pt.n_one, pt.B, STEP_N, 4])
    opts = [kv.split("=") for kv in pt.options.split(";") if kv]
    ds = pj.Dataset(t, y, s2, ctx)
    try:
        for k, v in opts:
            ctx.set_option(k, v)
        if pt.family in ("scan", "value"):
            out, st = ds.logl_batch(A, Bc, C, Dd, mu=mu, nu=nu, return_status=True)
            out = dict(logl=out, status=st)
        elif pt.family == "store":
            mean, st = ds.predict(A, Bc, C, Dd, rng.uniform(t[0] - 1, t[-1] + 1, STEP_M), mu=mu, nu=nu, return_status=True)
            out = dict(mean=mean, status=st)
        elif pt.family == "simulate":
            out = dict(y=ctx.simulate(A, Bc, C, Dd, t, s2, rng.standard_normal((pt.B, STEP_N))))
        else:
            g = ds.logl_grad(A, Bc, C, Dd, mu=mu, nu=nu)
            out = dict(logl=g["logl"], status=g["status"])
        L = pj._lib.lib()
        return L.pioran_celerite_config_name(-1).decode(), L.pioran_celerite_config_name(0).decode(), out
    finally:
        for k, _ in opts:
            ctx.set_option(k, None)
        ds.close()


# ---- the windowed, tile and time-parallel kernels' instantiations (route.hip block_plan, tile_plan, tp_step_plan): the grid
# tests/golden/window_route_listing.json was recorded over, from the commit before those rules (tools/experiments/window_route_listing.py) --------------
WINDOW_MAX_TERMS = 64
WINDOW_EMODES = ("", "block_emode=0", "block_emode=1", "block_emode=2")


def window_route(family, R=0, J=0, B=1, npd_rows=0, per_draw_series=False, want_cd=False, tp_rows=0, tp_segments=0, tp_mode=0, options=""):
    """(rc, name, plan) of pioran_window_route — family "block", "block_grad", "block_solve", "block_sim", "tile", "tile_grad" or "tp"; name: what
    pioran_celerite_config_name(-2) reports after the launch, "none" where it is refused (rc -4); plan: the 12 integers include/pioran_hip.h documents."""
    import pioran_jl_amd as pj
    name = ctypes.create_string_buffer(96)
    plan = (ctypes.c_int32 * 12)()
    rc = pj._lib.lib().pioran_window_route(family.encode(), R, J, B, npd_rows, int(per_draw_series), int(want_cd), tp_rows, tp_segments, tp_mode,
                                           options.encode(), name, len(name), plan)
    if rc not in (0, -4):
        raise ValueError(f"pioran_window_route: error {rc}")
    return rc, name.value.decode(), tuple(plan)


def window_keys():
    """family -> (keys, the values of the variable every key is asked over): the terms J for the windowed families (key[0] is R: J from ceil(R / 2)
    on), the rows R for the tile family (J = ceil(R / 2)), the padded state rows for the time-parallel one, valid or not."""
    value = [(R, B, npd, em) for R in range(1, 97) for B in (1, 256, 257, 512, 513) for npd in (0, 2, 4) for em in WINDOW_EMODES]
    grad = [(R, B, cd, ex) for R in range(1, 65) for B in (256, 257) for cd in (0, 1) for ex in ("", "exp=16")]
    terms = lambda key: range((key[0] + 1) // 2, WINDOW_MAX_TERMS + 1)
    return {"block": (value, terms), "block_grad": (grad, terms), "block_solve": ([(R,) for R in range(1, 65)], terms),
            "block_sim": ([(R,) for R in range(1, 65)], terms),
            "tile": ([(0,), (1,)], lambda key: range(1, 97)), "tile_grad": ([(0,), (1,)], lambda key: range(1, 65)),
            "tp": ([(nseg, mode, lean, waves) for nseg in (1, 2, 3, 9) for mode in (0, 1, 2, 4) for lean in ("", "tp_scan_lean=1")
                    for waves in ("", "tp_scan_waves=4")], lambda key: range(1, 67))}


def window_query(family, key, x):
    """The arguments of window_route for one entry of the grid."""
    if family == "block":
        return dict(R=key[0], J=x, B=key[1], npd_rows=key[2], options=key[3])
    if family == "block_grad":
        return dict(R=key[0], J=x, B=key[1], want_cd=bool(key[2]), options=key[3])
    if family in ("block_solve", "block_sim"):
        return dict(R=key[0], J=x, B=3)
    if family == "tile":
        return dict(R=x, J=(x + 1) // 2, B=5, per_draw_series=bool(key[0]))
    if family == "tile_grad":
        return dict(R=x, J=(x + 1) // 2, B=7, want_cd=bool(key[0]))
    return dict(tp_rows=x, tp_segments=key[0], tp_mode=key[1], options=";".join(o for o in key[2:] if o))


def window_kernels(family, plan, tp_segments=2):
    """The launches a plan of pioran_window_route stands for, as the listing holds them: [[kernel<template arguments>, threads per workgroup, dynamic
    LDS bytes], ...] in launch order.  The forward kernel's threads and LDS bytes, and every kernel's template arguments, are the plan's; the threads of the
    kernels behind it are written out here as the launch code has them (the launches themselves are held by the GPU tests).  Not listed, because no rule chooses them: the tile family's pair pre-pass, tp_records_kernel, tp_finish_kernel."""
    tf = ("false", "true")
    if family.startswith("block"):
        NB, e, pd, st, threads, lds, cd, tpt = plan[:8]
        out = [[f"celerite_block_kernel<{NB},{e},{pd},{st}>", threads, lds]]
        if family == "block_grad":
            out.append([f"celerite_block_adjoint_kernel<{NB},{tf[cd]},{tpt}>", 256, 0])
        elif family == "block_solve":
            out.append([f"celerite_block_backsolve_kernel<{NB}>", 64, 0])
        elif family == "block_sim":
            out += [[f"block_sim_xi_kernel<{NB}>", 256, 0], [f"celerite_block_sim_kernel<{NB}>", 64, 0]]
        return out
    if family == "tile":
        NB, KL, ser, _, _, threads, lds = plan[:7]
        return [[f"celerite_tile_kernel<{NB},{KL},false,{tf[ser]}>", threads, lds]]
    if family == "tile_grad":
        NB, KL, _, cd, waves, threads, lds, adj_lds = plan[:8]
        return [[f"celerite_tile_kernel<{NB},{KL},true,false>", threads, lds], [f"celerite_tile_adjoint_kernel<{NB},{tf[cd]}>", 64 * waves, adj_lds],
                [f"tile_pairs_grad_kernel<{tf[cd]}>", 512, 0]]
    NP, NWV, boundary, arg, lean, tw, lds, verify, varg, vlds, _, _ = plan
    walk = {1: lambda a, l: [f"tp_boundary_small_kernel<{a}>", 64, 0], 2: lambda a, l: [f"tp_boundary_wave_kernel<{a}>", 64, 0],
            3: lambda a, l: [f"tp_boundary_kernel<4,{a}>", 256, l]}
    out = [[f"tp_element_kernel<{NP},{NWV}>", 64 * NWV, 0]] if tp_segments > 1 else []
    out.append([f"tp_combine{'_lean' if lean else ''}_kernel<{arg},{tw}>", 64 * tw, lds] if boundary == 4 else walk[boundary](arg, lds))
    if verify:
        out.append(walk[verify](varg, vlds))
    return out + [[f"tp_filter_kernel<{NP},{NWV}>", 64 * NWV, 0]]


def window_answer(family, key, x):
    """What the listing holds per entry: the kernels of the plan, or the return code where the launch is refused."""
    q = window_query(family, key, x)
    rc, _, plan = window_route(family, **q)
    return rc if rc else window_kernels(family, plan, q.get("tp_segments", 2))


def window_runs(answers):
    """[(x, answer), ...] over consecutive x as runs [last x, answer] (the first run starts at the first x).  Within a run the kernels keep their names
    and threads and every dynamic LDS size is affine in x: a kernel of a run is [name, threads, LDS bytes at x = 0, LDS bytes per unit of x]."""
    runs = []        # [last x, answer, entries]
    for x, a in answers:
        r = runs[-1] if runs else None
        if r is not None and isinstance(a, int) and a == r[1]:
            r[0] = x
            continue
        if r is not None and not isinstance(a, int) and not isinstance(r[1], int) and [k[:2] for k in a] == [k[:2] for k in r[1]]:
            if r[2] == 1:        # the run's second entry sets the slopes
                for k, held in zip(a, r[1]):
                    held[3] = k[2] - held[2]
                    held[2] = k[2] - held[3] * x
            if all(held[2] + held[3] * x == k[2] for k, held in zip(a, r[1])):
                r[0], r[2] = x, r[2] + 1
                continue
        runs.append([x, a if isinstance(a, int) else [[k[0], k[1], k[2], 0] for k in a], 1])
    return [r[:2] for r in runs]


def window_expand(runs, xs):
    """The inverse of window_runs: [(x, answer), ...]."""
    out, i = [], 0
    for x in xs:
        while runs[i][0] < x:
            i += 1
        a = runs[i][1]
        out.append((x, a if isinstance(a, int) else [[k[0], k[1], k[2] + k[3] * x] for k in a]))
    return out


# ---- the launches of tests/test_gpu_window_route.py: one on each side of every rule of block_plan / tile_plan / tp_step_plan -----------------------------
WindowPoint = namedtuple("WindowPoint", "family rows J B npd_rows series cd options")
WINDOW_N, WINDOW_TP_N, WINDOW_M = 37, 64, 5
WINDOW_TO_BLOCK = "scan_config=block"
WINDOW_TO_TILE = "scan_config=tile"


def window_points():
    def pt(family, rows, B, npd_rows=0, series=False, cd=False, options="", J=None):
        return WindowPoint(family, rows, J or (rows + 1) // 2, B, npd_rows, series, cd, options)
    pts = []
    # the windowed value kernel: a point per block-column count, three draws and 257 (where the rule reads B > 256; five and six block columns have no such rule)
    pts += [pt("block", rows, B, options=WINDOW_TO_BLOCK) for rows in (5, 20, 40, 60, 70, 90) for B in ((3, 257) if rows < 64 else (3,))]
    # ... the forced E modes, where the kernel has them (three block columns) and where it does not (four: two LDS buffers do not fit, none is no option)
    pts += [pt("block", 40, 3, options=WINDOW_TO_BLOCK + f";block_emode={e}") for e in (0, 1, 2)]
    pts += [pt("block", 60, 3, options=WINDOW_TO_BLOCK + ";block_emode=1"), pt("block", 60, 3, options=WINDOW_TO_BLOCK + ";block_emode=2")]
    # ... per-draw rows (the last one or two terms per draw) at two and four block columns, either side of 256 draws
    pts += [pt("block", rows, B, npd_rows=npd) for rows in (20, 60) for npd in (2, 4) for B in (3, 257)]
    # gradient, solve (the prediction), simulate
    pts += [pt("block_grad", rows, B, cd=cd, options="no_tile=1") for rows in (5, 20, 40, 60) for B in (3, 257) for cd in (False, True)]
    pts.append(pt("block_grad", 40, 3, J=36, options="no_tile=1"))        # more than 32 terms: four contraction threads per term (32 of them with one row)
    pts += [pt(f, rows, 3) for f in ("block_solve", "block_sim") for rows in (5, 20, 40, 60)]
    # the tile family, five draws (the second workgroup ragged): a point per block-column count, the K-step edges of three block columns, a series per draw
    pts += [pt("tile", rows, 5, options=WINDOW_TO_TILE) for rows in (5, 20, 40, 60, 70, 90, 32, 33, 36, 37, 44, 47)]
    pts.append(pt("tile", 40, 5, series=True, options=WINDOW_TO_TILE))
    # its gradient, seven draws (ragged for two, three and four adjoint wavefronts)
    pts += [pt("tile_grad", rows, 7, cd=cd, options=WINDOW_TO_TILE) for rows in (5, 20, 40, 60) for cd in (False, True)]
    # the time-parallel family, one draw of 64 steps in four segments (two scan levels): the walk unchecked, the scan with its verification launch, and the
    # default repair pass (the scan or, below eight rows, the walk checked by the filter) — after that one the last launch is the windowed kernel's
    for rows in (2, 4, 8, 12, 16, 24, 64):
        base = "scan_config=tp;tp_segments=4"
        pts += [pt("tp", rows, 1, options=base + ";tp_scan=0;tp_unchecked=1"), pt("tp", rows, 1, options=base + ";tp_walk_repair=1"), pt("tp", rows, 1, options=base)]
    pts.append(pt("tp", 24, 1, options="scan_config=tp;tp_segments=4;tp_walk_repair=1;tp_scan_lean=1"))
    return pts


def _option(pt, key):
    return dict(kv.split("=") for kv in pt.options.split(";") if kv).get(key)


def window_expected(pt):
    """The name pioran_window_route gives the point's LAST launch of the three families — pioran_celerite_config_name(-2) after the call."""
    terms_options = ";".join(kv for kv in pt.options.split(";") if kv.split("=")[0] in ("block_emode", "exp", "tp_scan_lean", "tp_scan_waves"))
    if pt.family != "tp":
        # (the gradient of the Python API asks for d/dc and d/dd together; per-draw rows: the draws' own kernel has them, npd_rows of them)
        return window_route(pt.family, R=pt.rows, J=pt.J, B=pt.B, npd_rows=pt.npd_rows, per_draw_series=pt.series, want_cd=pt.cd, options=terms_options)[1]
    _, (scan, RP, nseg, _) = value_route(pt.rows, pt.J, 0, pt.B, WINDOW_TP_N, options=pt.options)
    repair = not _option(pt, "tp_walk_repair") and not _option(pt, "tp_unchecked")
    if repair:      # the serial-chain kernel runs last, over the draws that failed the check
        return window_route("block", R=pt.rows, J=pt.J, B=pt.B)[1]
    return window_route("tp", tp_rows=RP, tp_segments=nseg, tp_mode=1 if scan and _option(pt, "tp_walk_repair") else 0, options=terms_options)[1]


def run_window_point(ctx, pt):
    """One call that reaches the point's launch: (family that ran, pioran_celerite_config_name(-2) after it, the outputs that are one workgroup's or
    one wavefront's sums — the gradient arrays are left out)."""
    import pioran_jl_amd as pj
    N = WINDOW_TP_N if pt.family == "tp" else WINDOW_N
    npd = pt.npd_rows // 2
    n_one = 2 * pt.J - pt.rows
    t, y, s2, A, Bc, C, Dd, mu, nu = inputs_cd(CdPoint(pt.J, npd, pt.B, N, "")) if npd else inputs(Point(pt.J, 0, pt.B, N, ""))
    if n_one:          # the one-row terms are the LAST ones
        Bc[:, -n_one:] = 0.0
        Dd[-n_one:] = 0.0
    rng = np.random.default_rng([pt.J, pt.rows, pt.B, N, 6])
    opts = [kv.split("=") for kv in pt.options.split(";") if kv]
    ds = pj.Dataset(t, y, s2, ctx)
    try:
        for k, v in opts:
            ctx.set_option(k, v)
        if pt.family in ("block", "tile", "tp"):
            if pt.series:      # a series per draw: the shifted log-flux form on a positive series
                ds.close()
                ds = pj.Dataset(t, np.exp(0.5 * y), s2, ctx)
                out, st = ds.logl_batch(A, Bc, C, Dd, mu=mu, nu=nu, shift=np.exp(0.5 * y).min() * np.linspace(0.1, 0.9, pt.B), return_status=True)
            else:
                out, st = ds.logl_batch(A, Bc, C, Dd, mu=mu, nu=nu, return_status=True)
            out = dict(logl=out, status=st)
        elif pt.family == "block_solve":
            mean, st = ds.predict(A, Bc, C, Dd, rng.uniform(t[0] - 1, t[-1] + 1, WINDOW_M), mu=mu, nu=nu, return_status=True)
            out = dict(mean=mean, status=st)
        elif pt.family == "block_sim":
            out = dict(y=ctx.simulate(A, Bc, C, Dd, t, s2, rng.standard_normal((pt.B, N))))
        else:
            g = ds.logl_grad(A, Bc, C, Dd, mu=mu, nu=nu, cd_grad=pt.cd)
            out = dict(logl=g["logl"], status=g["status"])
        L = pj._lib.lib()
        ran = L.pioran_celerite_config_name(-2).decode() if "pioran_window_route" in pj._lib.SIGNATURES else ""
        return L.pioran_celerite_config_name(-1).decode(), ran, out
    finally:
        for k, _ in opts:
            ctx.set_option(k, None)
        ds.close()


def expected(pt):
    """The family the rules name for a point of any of the three kinds."""
    if isinstance(pt, CdPoint):
        return value_route_cd(pt.J - pt.npd, 0, pt.npd, pt.B, pt.N, options=pt.options)[0]
    if isinstance(pt, ThetaPoint):
        return value_route_cd(pt.n_components, 0, pt.n_qpo, pt.B, pt.N, must_run=True)[0]
    return value_route(rows_of(pt), pt.J, pt.n_one, pt.B, pt.N, options=pt.options)[0]


def inputs(pt):
    """Well-conditioned draws on an irregular grid; the first n_one terms have b = d = 0 (one row each)."""
    rng = np.random.default_rng([pt.J, pt.n_one, pt.B, pt.N])
    t = np.cumsum(rng.uniform(0.05, 2.0, pt.N))
    y = rng.standard_normal(pt.N)
    s2 = rng.uniform(0.01, 0.1, pt.N)
    A = rng.uniform(0.1, 2.0, (pt.B, pt.J))
    Bc = rng.uniform(-0.05, 0.05, (pt.B, pt.J)) * A
    C = rng.uniform(0.05, 2.0, pt.J)
    Dd = rng.uniform(0.05, 3.0, pt.J)
    Bc[:, :pt.n_one] = 0.0
    Dd[:pt.n_one] = 0.0
    return t, y, s2, A, Bc, C, Dd, rng.standard_normal(pt.B) * 0.1, rng.uniform(0.5, 2.0, pt.B)


def inputs_cd(pt):
    """The inputs of the shared point of these sizes, with C, Dd [B][J]: the last npd columns differ between the draws."""
    t, y, s2, A, Bc, C, Dd, mu, nu = inputs(Point(pt.J, 0, pt.B, pt.N, ""))
    rng = np.random.default_rng([pt.J, pt.npd, pt.B, pt.N, 1])
    C2 = np.broadcast_to(C, (pt.B, pt.J)).copy()
    D2 = np.broadcast_to(Dd, (pt.B, pt.J)).copy()
    C2[:, pt.J - pt.npd:] = rng.uniform(0.05, 2.0, (pt.B, pt.npd))
    D2[:, pt.J - pt.npd:] = rng.uniform(0.05, 3.0, (pt.B, pt.npd))
    return t, y, s2, A, Bc, C2, D2, mu, nu


def run_theta_point(ctx, pt):
    """One call of Dataset.logpdf_theta with QPO features: (family that ran, log L, status)."""
    import pioran_jl_amd as pj
    rng = np.random.default_rng([pt.n_components, pt.n_qpo, pt.B, pt.N, 2])
    t = np.cumsum(rng.uniform(0.05, 2.0, pt.N))
    y = rng.standard_normal(pt.N)
    s2 = rng.uniform(0.01, 0.1, pt.N)
    f_min, f_max = 1 / (t[-1] - t[0]), 1 / np.min(np.diff(t)) / 2
    theta = np.column_stack([rng.uniform(0.0, 1.2, pt.B), np.exp(rng.uniform(np.log(f_min * 4), np.log(f_max / 4), pt.B)), rng.uniform(2.0, 3.8, pt.B)])
    qpo = np.stack([rng.uniform(0.05, 2.0, (pt.B, pt.n_qpo)), np.exp(rng.uniform(np.log(f_min * 20), np.log(f_max / 5), (pt.B, pt.n_qpo))),
                    rng.uniform(2.0, 30.0, (pt.B, pt.n_qpo))], axis=2)      # (B, n_qpo, 3): S0, f0, Q
    ds = pj.Dataset(t, y, s2, ctx)
    try:
        out, st = ds.logpdf_theta(pj.SingleBendingPowerLaw, theta, rng.uniform(0.5, 2.0, pt.B), f_min, f_max, pt.n_components, qpo=qpo, return_status=True)
        return pj._lib.lib().pioran_celerite_config_name(-1).decode(), out, st
    finally:
        ds.close()


def run_carma_point(ctx, pt):
    """One call of Dataset.logpdf_carma under the point's options: (family that ran, log L, status, the coefficients A, Bc, C, Dd (B, J))."""
    import pioran_jl_amd as pj
    rng = np.random.default_rng([pt.p, pt.q, pt.B, pt.N, 5])
    t = np.cumsum(rng.uniform(0.05, 2.0, pt.N))
    y = np.exp(0.5 * rng.standard_normal(pt.N)) if pt.shift else rng.standard_normal(pt.N)     # a shifted call holds a positive series
    s2 = rng.uniform(0.01, 0.1, pt.N)
    bounds = 1 / (t[-1] - t[0]), 1 / np.min(np.diff(t)) / 2
    quads = [pj.sample_quad(pt.p, pt.q, rng, *bounds) for _ in range(pt.B)]
    qa, qb = np.array([x[0] for x in quads]), np.array([x[1] for x in quads])
    shift = y.min() * np.linspace(0.1, 0.9, pt.B) if pt.shift else None
    opts = [kv.split("=") for kv in pt.options.split(";") if kv]
    ds = pj.Dataset(t, y, s2, ctx)
    try:
        for k, v in opts:
            ctx.set_option(k, v)
        out, st, *co = ds.logpdf_carma(pt.p, pt.q, qa, qb, rng.uniform(0.5, 2.0, pt.B), bounds=bounds, mu=rng.standard_normal(pt.B) * 0.1,
                                       nu=rng.uniform(0.5, 2.0, pt.B), shift=shift, return_status=True, return_coefs=True)
        return pj._lib.lib().pioran_celerite_config_name(-1).decode(), out, st, co
    finally:
        for k, _ in opts:
            ctx.set_option(k, None)
        ds.close()


def carma_expected(pt, Bc, C, Dd):
    """The family the rules name for a CarmaPoint whose call returned these coefficients: a term is per draw where its (c, d) differ between the
    draws, and keeps one row where it is not and d = 0 and b = 0 in every draw.  No per-draw term is the shared case, pioran_value_route's."""
    per_draw = (C != C[0]).any(axis=0) | (Dd != Dd[0]).any(axis=0)
    one_row = ~per_draw & (Dd[0] == 0) & ~Bc.any(axis=0)
    J, npd, n_one = len(per_draw), int(per_draw.sum()), int(one_row.sum())
    if npd == 0:
        return value_route(2 * J - n_one, J, n_one, pt.B, pt.N, per_draw_series=pt.shift, options=pt.options)[0]
    return value_route_cd(J - npd - n_one, n_one, npd, pt.B, pt.N, per_draw_series=pt.shift, options=pt.options)[0]


def run_point(ctx, pt):
    """One launch through Dataset.logl_batch under the point's options: (family that ran, log L, status)."""
    import pioran_jl_amd as pj
    if isinstance(pt, ThetaPoint):
        return run_theta_point(ctx, pt)
    t, y, s2, A, Bc, C, Dd, mu, nu = inputs_cd(pt) if isinstance(pt, CdPoint) else inputs(pt)
    opts = [kv.split("=") for kv in pt.options.split(";") if kv]
    ds = pj.Dataset(t, y, s2, ctx)
    try:
        for k, v in opts:
            ctx.set_option(k, v)
        out, st = ds.logl_batch(A, Bc, C, Dd, mu=mu, nu=nu, return_status=True)
        return pj._lib.lib().pioran_celerite_config_name(-1).decode(), out, st
    finally:
        for k, _ in opts:
            ctx.set_option(k, None)
        ds.close()


GRAD_ARRAYS = ("grad_a", "grad_b", "grad_c", "grad_d", "grad_mu", "grad_nu", "grad_y", "grad_sigma2", "grad_shift")


def run_entries(ctx, save=None, against=None):
    """The listing of entry_points(): per point the name that ran, the return code and a hash of every output that is one workgroup per draw.  The
    gradient arrays' lane sums go through LDS atomics whose order is not fixed: with `against` (an .npz of `save`) their largest deviation from it,
    max |delta| / (1 + max |ref|), is printed instead, and its maximum over the grid last."""
    ref = np.load(against) if against else None
    kept, worst = {}, 0.0
    for i, pt in enumerate(entry_points()):
        name, rc, out = run_entry_point(ctx, pt)
        h = hashlib.sha256(b"".join(np.ascontiguousarray(v).tobytes() for k, v in sorted(out.items()) if k not in GRAD_ARRAYS)).hexdigest()[:16]
        line = (f"{pt.entry:14s} rows {rows_of(pt):3d} J {pt.J:2d} B {pt.B:4d} per-draw {int(pt.per_draw)} shift {int(pt.shift)} cd {int(pt.cd_grad)} "
                f"series {int(pt.series)} [{pt.options}] rc {rc} {name} {h if out else '-'}")
        for k in GRAD_ARRAYS:
            if k in out:
                kept[f"{i}:{k}"] = out[k]
                if ref is not None:
                    r = ref[f"{i}:{k}"]
                    ok = np.isfinite(r)
                    assert np.array_equal(ok, np.isfinite(out[k])), (pt, k)
                    dev = float(np.max(np.abs(out[k][ok] - r[ok])) / (1 + np.max(np.abs(r[ok])))) if ok.any() else 0.0
                    worst = max(worst, dev)
                    line += f" {k} {dev:.1e}"
        print(line, flush=True)
    if save:
        np.savez(save, **kept)
    if ref is not None:
        print(f"largest gradient deviation max |delta| / (1 + max |ref|): {worst:.2e}")


def main():
    import pioran_jl_amd as pj
    if "--before-value-route" in sys.argv:
        pj._lib.SIGNATURES.pop("pioran_value_route", None)
    if "--before-value-route-cd" in sys.argv:
        pj._lib.SIGNATURES.pop("pioran_value_route_cd", None)
    if "--before-entry-route" in sys.argv:
        pj._lib.SIGNATURES.pop("pioran_entry_route", None)
    if "--before-step-route" in sys.argv:
        pj._lib.SIGNATURES.pop("pioran_step_route", None)
    if "--before-window-route" in sys.argv:
        pj._lib.SIGNATURES.pop("pioran_window_route", None)
    ctx = pj.Context(0)
    if "--entries" in sys.argv:
        arg = lambda flag: sys.argv[sys.argv.index(flag) + 1] if flag in sys.argv else None
        return run_entries(ctx, arg("--save"), arg("--against"))
    if "--steps" in sys.argv:      # (the name of the instantiation is not listed: a library from before pioran_step_route names the scan's only)
        for pt in step_points():
            fam, _, out = run_step_point(ctx, pt)
            digest = hashlib.sha256(b"".join(np.ascontiguousarray(v).tobytes() for _, v in sorted(out.items()))).hexdigest()[:16]
            print(f"step {pt.family:8s} rows {2 * pt.J - pt.n_one:3d} J {pt.J:2d} B {pt.B:4d} N {STEP_N} [{pt.options}] {fam} {digest}", flush=True)
        for pt in window_points():     # (the instantiation's name last: empty from a library before pioran_window_route)
            fam, ran, out = run_window_point(ctx, pt)
            digest = hashlib.sha256(b"".join(np.ascontiguousarray(v).tobytes() for _, v in sorted(out.items()))).hexdigest()[:16]
            print(f"window {pt.family:11s} rows {pt.rows:3d} J {pt.J:2d} B {pt.B:4d} per-draw rows {pt.npd_rows} series {int(pt.series)} cd {int(pt.cd)} "
                  f"[{pt.options}] {fam} {digest} {ran}", flush=True)
        return
    for pt in carma_points():
        fam, out, st, _ = run_carma_point(ctx, pt)
        digest = hashlib.sha256(out.tobytes() + st.tobytes()).hexdigest()[:16]
        print(f"carma ({pt.p}, {pt.q}) B {pt.B:4d} N {pt.N:5d} shift {int(pt.shift)} [{pt.options}] {fam} {digest}", flush=True)
    for pt in points() + cd_points() + theta_points():
        fam, out, st = run_point(ctx, pt)
        digest = hashlib.sha256(out.tobytes() + st.tobytes()).hexdigest()[:16]
        if isinstance(pt, CdPoint):
            print(f"cd J {pt.J:2d} per draw {pt.npd:2d} B {pt.B:4d} N {pt.N:5d} [{pt.options}] {fam} {digest}", flush=True)
        elif isinstance(pt, ThetaPoint):
            print(f"theta SHO-{pt.n_components} qpo {pt.n_qpo} B {pt.B:4d} N {pt.N:5d} {fam} {digest}", flush=True)
        else:
            print(f"rows {rows_of(pt):3d} J {pt.J:2d} B {pt.B:4d} N {pt.N:5d} [{pt.options}] {fam} {digest}", flush=True)


if __name__ == "__main__":
    main()
