#!/usr/bin/env python3
"""The launches that cross every routing rule of the value path (csrc/route.hip), at the smallest shapes that still do.

Importable: `points()` is the grid of tests/test_gpu_route.py, `run_point` makes one launch through the Python API, `value_route` asks
pioran_value_route.  As a program it runs the grid and prints, per point, the kernel family that ran and a hash of the log L and status
arrays — a different segment count, mode or chunking changes bits, so two libraries with equal listings made equal plans:

    PIORAN_HIP_LIB=/path/to/other/libpioran_hip.so python tools/route_grid.py [--before-value-route] > listing.txt

(--before-value-route: the library is from before pioran_value_route existed; the binding does not ask for the symbol.)
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


def value_route(rows, J, n_one, B, N, per_draw_series=False, pass_draws=0, options=""):
    """(family, (scan, RP, nseg, L)) of pioran_value_route."""
    import pioran_jl_amd as pj
    name = ctypes.create_string_buffer(64)
    tp = (ctypes.c_int32 * 4)()
    rc = pj._lib.lib().pioran_value_route(rows, J, n_one, B, N, int(per_draw_series), pass_draws, options.encode(), name, len(name), tp)
    if rc:
        raise ValueError(f"pioran_value_route: error {rc}")
    return name.value.decode(), tuple(tp)


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


def run_point(ctx, pt):
    """One launch through Dataset.logl_batch under the point's options: (family that ran, log L, status)."""
    import pioran_jl_amd as pj
    t, y, s2, A, Bc, C, Dd, mu, nu = inputs(pt)
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
    ctx = pj.Context(0)
    for pt in points():
        fam, out, st = run_point(ctx, pt)
        digest = hashlib.sha256(out.tobytes() + st.tobytes()).hexdigest()[:16]
        print(f"rows {rows_of(pt):3d} J {pt.J:2d} B {pt.B:4d} N {pt.N:5d} [{pt.options}] {fam} {digest}", flush=True)


if __name__ == "__main__":
    main()
