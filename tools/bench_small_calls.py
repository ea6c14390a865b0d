#!/usr/bin/env python3
"""Host time of the small-call path, where the kernels take next to nothing: us per call (median of 15 batches of 300 calls) of the scalar call at
N = 32, SHO-20, and of four walkers on the default family, on the latency layout (no_block) and on the throughput layout (no_block, no_wide,
no_tile), on the tile family (scan_config=tile), and of the scalar call of two terms at N = 64 on the time-parallel family (scan_config=tp, with its
repair pass).  One JSON line.  PIORAN_HIP_LIB chooses the library: for an A/B run fresh processes alternately on the two (profiles/step_route_ab.txt,
profiles/window_route_ab.txt); --before-step-route / --before-window-route: the library is from before pioran_step_route / pioran_window_route existed."""
import json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pioran_jl_amd as pj
if "--before-step-route" in sys.argv:
    pj._lib.SIGNATURES.pop("pioran_step_route", None)
if "--before-window-route" in sys.argv:
    pj._lib.SIGNATURES.pop("pioran_window_route", None)
rng = np.random.default_rng(1)
N, J, B = 32, 20, 4
t = np.cumsum(rng.uniform(0.05, 2.0, N)); y = rng.standard_normal(N); s2 = rng.uniform(0.01, 0.1, N)
A = rng.uniform(0.1, 2.0, (B, J)); Bc = rng.uniform(-0.05, 0.05, (B, J)) * A; C = rng.uniform(0.05, 2.0, J); Dd = rng.uniform(0.05, 3.0, J)
mu = rng.standard_normal(B) * 0.1; nu = rng.uniform(0.5, 2.0, B)
ctx = pj.Context(0)
ds = pj.Dataset(t, y, s2, ctx)

def timed(f, reps=300, batches=15):
    for _ in range(50):
        f()
    out = []
    for _ in range(batches):
        t0 = time.perf_counter()
        for _ in range(reps):
            f()
        out.append((time.perf_counter() - t0) / reps * 1e6)
    return float(np.median(out))

res = {}
res["scalar_logl_us"] = timed(lambda: pj.logl(A[0], Bc[0], C, Dd, t, y, s2, ctx=ctx))
res["scalar_family"] = pj._lib.lib().pioran_celerite_config_name(-1).decode()
for key, opts in (("walkers4_default_us", ()), ("walkers4_wide_us", ("no_block",)), ("walkers4_scan_us", ("no_block", "no_wide", "no_tile"))):
    for o in opts:
        ctx.set_option(o, True)
    res[key] = timed(lambda: ds.logl_batch(A, Bc, C, Dd, mu=mu, nu=nu))
    res[key.replace("_us", "_family")] = pj._lib.lib().pioran_celerite_config_name(-1).decode()
    for o in opts:
        ctx.set_option(o, False)
ctx.set_option("scan_config", "tile")
res["walkers4_tile_us"] = timed(lambda: ds.logl_batch(A, Bc, C, Dd, mu=mu, nu=nu))
res["walkers4_tile_family"] = pj._lib.lib().pioran_celerite_config_name(-1).decode()
ctx.set_option("scan_config", "tp")
t2 = np.cumsum(rng.uniform(0.05, 2.0, 64)); ds2 = pj.Dataset(t2, rng.standard_normal(64), rng.uniform(0.01, 0.1, 64), ctx)
res["scalar_tp_us"] = timed(lambda: ds2.logl_batch(A[:1, :2], Bc[:1, :2], C[:2], Dd[:2]))
res["scalar_tp_family"] = pj._lib.lib().pioran_celerite_config_name(-1).decode()
ctx.set_option("scan_config", None)
print(json.dumps(res))
