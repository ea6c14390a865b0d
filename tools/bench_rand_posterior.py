#!/usr/bin/env python3
"""Posterior draws at new times by Matheron's rule (Dataset.rand_posterior, pioran_celerite_rand_posterior) at the shape of the reference's
posterior predictive check get_ppc_timeseries (src/plots_diagnostics.jl:640-671): N = 1e4 (oracle.synthetic_series), t_pred =
sort(unique(t | range(t[1], t[end], 2 N))) (M about 3e4), B = 100 draws of SHO-20 —
    the entry as it is called (host clock: uploads, the chain, download), without and with a shift per draw;
    the steps of the chain's first chunk from the context's event slots (context option "rp_events": gather | simulation | residual |
    prediction | combination) and the share of the three streaming kernels in it;
    at N = 500, M = 1000, one draw: the same entry against the dense route of pj.rand_posterior (pj.mean, the dense pj.cov, a Cholesky on
    the host), the one comparison with the earlier code there is.
One JSON line; `--out FILE` also writes it there."""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pioran_jl_amd as pj
from oracle import oracle as O

ap = argparse.ArgumentParser()
ap.add_argument("--N", type=int, default=10_000)
ap.add_argument("--B", type=int, default=100)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--small-N", type=int, default=500)
ap.add_argument("--small-M", type=int, default=1000)
ap.add_argument("--no-dense", action="store_true")
ap.add_argument("--out", default=None)
args = ap.parse_args()

STEPS = ("gather", "simulation", "residual", "prediction", "combination")     # between the event slots 4 .. 9
ctx = pj.Context(0)
res = {"fp64_fma_ceiling_tflops_now": ctx.fp64_probe(), "ppc": []}


def timed(ds, call, reps):
    """(host ms median / min / max of the whole call, per-step device ms medians of the first chunk, config name)"""
    call()
    ctx.set_option("rp_events", 1)
    host, steps = [], []
    for _ in range(reps):
        ctx.synchronize()
        t0 = time.perf_counter()
        call()
        host.append((time.perf_counter() - t0) * 1e3)
        steps.append([ctx.event_elapsed_ms(4 + i, 5 + i) for i in range(5)])
    ctx.set_option("rp_events", None)
    steps = np.median(np.array(steps), axis=0)
    name = pj._lib.lib().pioran_celerite_config_name(-1).decode()
    return {"host_ms_median": float(np.median(host)), "host_ms_min": float(np.min(host)), "host_ms_max": float(np.max(host)),
            "device_ms": dict(zip(STEPS, map(float, steps))), "device_ms_chain": float(steps.sum()),
            "share_of_the_three_new_kernels": float((steps[0] + steps[2] + steps[4]) / steps.sum()), "config": name}


# ---- the PPC shape -----------------------------------------------------------------------------------------------------------------
N, B = args.N, args.B
t, y, yerr = O.synthetic_series(N)
A, Bc, C, Dd, mu, nu = O.theta_to_coefs(O.synthetic_theta(B, t, y), t, 20, "SHO")
t_pred = pj.ppc_t_pred(t)
M = len(t_pred)
rng = np.random.default_rng(0)
qd, qn, ep = rng.standard_normal((B, N)), rng.standard_normal((B, M)), rng.standard_normal((B, N))
for with_shift in (False, True):
    if with_shift:      # raw flux whose logarithm is the series above
        yy, s2 = np.exp(y) + 1.0, (yerr * np.exp(y)) ** 2
        shift = np.random.default_rng(1).uniform(0.1, 0.9, B)
    else:
        yy, s2, shift = y, yerr ** 2, None
    ds = pj.Dataset(t, yy, s2, ctx)
    out = {}
    def call():
        out["draws"], out["status"] = ds.rand_posterior(A, Bc, C, Dd, t_pred, qd, qn, ep, mu=mu, nu=nu, shift=shift, return_status=True)
    r = timed(ds, call, args.reps)
    ds.close()
    r.update({"N": N, "M": M, "B": B, "J": int(A.shape[1]), "shift": with_shift, "status_nonzero": int((out["status"] != 0).sum()),
              "bytes_moved_by_the_three_kernels": int(8 * B * (2 * (N + M) + 5 * N + 3 * M))})
    res["ppc"].append(r)

# ---- the dense route, one draw -----------------------------------------------------------------------------------------------------
Ns, Ms = args.small_N, args.small_M
ts, ys, es = O.synthetic_series(Ns)
As, Bs, Cs, Ds, mus, nus = O.theta_to_coefs(O.synthetic_theta(1, ts, ys), ts, 20, "SHO")
taus = np.linspace(ts[0], ts[-1], Ms)
kernel = pj.Celerite(As[0][0], Bs[0][0], Cs[0], Ds[0])
for j in range(1, len(Cs)):
    kernel = kernel + pj.Celerite(As[0][j], Bs[0][j], Cs[j], Ds[j])
fp = pj.posterior(pj.ScalableGP(float(mus[0]), kernel)(ts, nus[0] * es ** 2), ys)
small = {"N": Ns, "M": Ms, "draws": 1}
for name, solver in (("celerite_ms", "celerite"),) + (() if args.no_dense else (("dense_ms", None),)):
    try:
        pj.rand_posterior(np.random.default_rng(2), fp, taus, 1, ctx=ctx, solver=solver)
        ts_ = []
        for _ in range(3):
            t0 = time.perf_counter()
            pj.rand_posterior(np.random.default_rng(2), fp, taus, 1, ctx=ctx, solver=solver)
            ts_.append((time.perf_counter() - t0) * 1e3)
        small[name] = float(np.median(ts_))
    except np.linalg.LinAlgError as e:
        small[name] = None
        small[name + "_error"] = str(e)
res["small"] = small
line = json.dumps(res)
print(line)
if args.out:
    with open(args.out, "w") as f:
        f.write(line + "\n")
