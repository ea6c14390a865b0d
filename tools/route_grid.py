#!/usr/bin/env python3
"""The launches that cross every routing rule of the value path (csrc/route.hip), at the smallest shapes that still do.

Importable: `points()` is the grid of tests/test_gpu_route.py, `run_point` makes one launch through the Python API, `value_route` asks
pioran_value_route; `cd_points()` / `theta_points()` are the launches whose draws bring (c, d) of their own, `value_route_cd` asks
pioran_value_route_cd.  As a program it runs the grid and prints, per point, the kernel family that ran and a hash of the log L and status
arrays — a different segment count, mode or chunking changes bits, so two libraries with equal listings made equal plans:

    PIORAN_HIP_LIB=/path/to/other/libpioran_hip.so python tools/route_grid.py [--before-value-route] [--before-value-route-cd] > listing.txt

(--before-value-route[-cd]: the library is from before pioran_value_route[_cd] existed; the binding does not ask for the symbol.)
"""
import ctypes
import hashlib
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


def main():
    import pioran_jl_amd as pj
    if "--before-value-route" in sys.argv:
        pj._lib.SIGNATURES.pop("pioran_value_route", None)
    if "--before-value-route-cd" in sys.argv:
        pj._lib.SIGNATURES.pop("pioran_value_route_cd", None)
    ctx = pj.Context(0)
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
