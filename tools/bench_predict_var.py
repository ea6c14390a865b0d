#!/usr/bin/env python3
"""Posterior variance at new times through the celerite factorisation (Dataset.predict_var) against the dense route (pj.std):
N = M = 1e4, SHO-20 at 1 / 16 / 256 draws, N = M = 65 536 at one draw; the dense pj.std at the largest (N, M) of DENSE_SIZES that fits.
Host-pointer entries (PCIe and host staging included).  One JSON line; kernel times: run under `rocprofv3 --kernel-trace --stats`."""
import json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pioran_jl_amd as pj
from oracle import oracle as O

J = 20
DENSE_SIZES = [int(x) for x in os.environ.get("DENSE_SIZES", "10000,8192,4096").split(",") if x]
ctx = pj.Context(0)


def timed(f, reps=3):
    f(); ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); r = f(); ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), r


def case(N, M, B):
    t, y, yerr = O.synthetic_series(N)
    A, Bc, C, Dd, mu, nu = O.theta_to_coefs(O.synthetic_theta(min(B, 8), t, y), t, J, "SHO")
    reps = -(-B // len(A))
    A, Bc, nu = (np.tile(v, (reps,) + (1,) * (v.ndim - 1))[:B] for v in (A, Bc, nu))
    tau = np.linspace(t[0] - 10, t[-1] + 10, M)
    ds = pj.Dataset(t, y, yerr ** 2, ctx)
    sec, (v, st) = timed(lambda: ds.predict_var(A, Bc, C, Dd, tau, nu=nu, return_status=True))
    ds.close()
    return {"N": N, "M": M, "draws": B, "ms_per_call": sec * 1e3, "ms_per_draw": sec * 1e3 / B, "status_ok": bool((st == 0).all()),
            "min_var_over_k0": float(np.min(v / A.sum(axis=1)[:, None]))}


res = {"workload": f"SHO-{J}, synthetic series", "fp64_fma_ceiling_tflops": ctx.fp64_probe(), "celerite": [], "dense": None}
for N, M, B in ((10_000, 10_000, 1), (10_000, 10_000, 16), (10_000, 10_000, 256), (65_536, 65_536, 1)):
    if os.environ.get("ONLY_B") and int(os.environ["ONLY_B"]) != B:
        continue
    res["celerite"].append(case(N, M, B))
for n in DENSE_SIZES:
    t, y, yerr = O.synthetic_series(n)
    A, Bc, C, Dd, mu, nu = O.theta_to_coefs(O.synthetic_theta(1, t, y), t, J, "SHO")
    R = pj.SumOfCelerite(A[0], Bc[0], C, Dd)
    fp = pj.posterior(pj.ScalableGP(0.0, R)(t, yerr ** 2), y)
    tau = np.linspace(t[0] - 10, t[-1] + 10, n)
    try:
        sd, dense = timed(lambda: pj.std(fp, tau, ctx=ctx), reps=1)
    except (pj._lib.PioranHipError, MemoryError) as e:
        print(f"dense N = M = {n}: {e}", file=sys.stderr)
        continue
    sc, cel = timed(lambda: pj.std(fp, tau, ctx=ctx, solver="celerite"))
    res["dense"] = {"N": n, "M": n, "dense_std_ms": sd * 1e3, "celerite_std_ms": sc * 1e3, "ratio": sd / sc,
                    "max_abs_var_diff_over_k0": float(np.max(np.abs(cel ** 2 - dense ** 2)) / A[0].sum())}
    break
print(json.dumps(res))
