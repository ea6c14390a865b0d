#!/usr/bin/env python3
"""Quantiles over the draw axis (Context.quantiles_dev) and the posterior predictive summary (pj.ppc_timeseries_summary) at the sizes of the
reference's predictive check, one box, one process:

(a) the kernel alone through the device-pointer entry at (B, M) = (100, 29998), (1000, 29998), (1000, 999), five quantiles and the mean, timed
    with the context's event slots;
(b) the floor it is read against: B M 8 bytes read once at the rate this box copies device memory (a 1 GiB torch copy, bytes read + written
    over its time, measured here);
(c) pj.ppc_timeseries_summary against the path it replaces — pj.ppc_timeseries, then np.quantile of the series and of the residuals and the
    residuals' mean on the host, over the samples whose draw did not fail (NaN columns dropped first: the same draws the summary keeps) — by the
    host clock (both calls block), N = 1e4, SHO with 20 components, B = 100 and 1000, the two alternating.
    Both draw the same 5 N B normals on the host first; that time is part of both figures and is also given on its own.

Every figure: one untimed run, then `--reps` timed ones (at least 10), median with minimum and maximum.  The one condition: the summary call is
not slower than the path it replaces at either B (exit status 1 otherwise).  One JSON line; `--out FILE` also writes it there."""
import argparse, json, os, socket, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pioran_jl_amd as pj

FIVE = (0.025, 0.16, 0.5, 0.84, 0.975)
ap = argparse.ArgumentParser()
ap.add_argument("--N", type=int, default=10_000)
ap.add_argument("--J", type=int, default=20)
ap.add_argument("--B", type=int, nargs="+", default=[100, 1000])
ap.add_argument("--shapes", type=int, nargs="+", default=[100, 29998, 1000, 29998, 1000, 999], help="B M pairs of part (a)")
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--out", default=None)
args = ap.parse_args()
reps = max(10, args.reps)

import torch
ctx = pj.Context(0)
dev = torch.device("cuda:0")
rng = np.random.default_rng(0)


def stats(ts):
    return {"median": float(np.median(ts)), "min": float(np.min(ts)), "max": float(np.max(ts)), "reps": len(ts)}


res = {"box": socket.gethostname(), "device": torch.cuda.get_device_name(0), "kernel": [], "ppc": []}

# (b) the box's copy rate
src = torch.empty(1 << 27, dtype=torch.float64, device=dev).normal_()
dst = torch.empty_like(src)
dst.copy_(src); torch.cuda.synchronize()
ts = []
for _ in range(reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); dst.copy_(src); e1.record(); torch.cuda.synchronize()
    ts.append(e0.elapsed_time(e1))
rate = 2.0 * src.numel() * 8 / (np.median(ts) * 1e-3)          # bytes per second, read + written
res["copy_rate_TBps"] = rate / 1e12
del src, dst

# (a) the kernel alone
for B, M in zip(args.shapes[::2], args.shapes[1::2]):
    dX = torch.empty((B, M), dtype=torch.float64, device=dev).normal_()
    dq = torch.empty((len(FIVE), M), dtype=torch.float64, device=dev)
    dm = torch.empty((M,), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    run = lambda: ctx.quantiles_dev(B, M, M, dX.data_ptr(), FIVE, dquant=dq.data_ptr(), dmean=dm.data_ptr())
    run(); ctx.synchronize()
    ts = []
    for _ in range(reps):
        ctx.event_record(0); run(); ctx.event_record(1); ctx.synchronize()
        ts.append(ctx.event_elapsed_ms(0, 1))
    floor_ms = B * M * 8 / rate * 1e3
    ref = np.quantile(dX[:, :64].cpu().numpy(), FIVE, axis=0)
    err = float(np.max(np.abs(dq[:, :64].cpu().numpy() - ref) / np.max(np.abs(ref))))
    res["kernel"].append({"B": B, "M": M, "ms": stats(ts), "read_once_floor_ms": floor_ms, "floor_over_median": floor_ms / float(np.median(ts)),
                          "max_rel_dev_from_numpy_first_64_columns": err})
    del dX, dq, dm

# (c) the predictive check
N, J = args.N, args.J
t = np.cumsum(0.05 + rng.exponential(0.95, N))
yerr = rng.uniform(0.05, 0.2, N)
y = np.sin(0.01 * t) + 0.3 * rng.standard_normal(N)
f_min, f_max = 1.0 / (t[-1] - t[0]), 1.0 / (2.0 * np.min(np.diff(t)))
ok = True
for B in args.B:
    theta = np.column_stack([rng.uniform(0.0, 1.25, B), np.exp(rng.uniform(np.log(f_min), np.log(f_max), B)), rng.uniform(2.0, 4.0, B)])
    A, Bc, C, Dd = pj.approx_batch(pj.SingleBendingPowerLaw, theta, f_min, f_max, J, norm=np.var(y) * np.exp(0.3 * rng.standard_normal(B)))
    mu, nu = np.mean(y) + 0.1 * rng.standard_normal(B), rng.gamma(2.0, 0.5, B) + 0.2
    M = len(pj.ppc_t_pred(t))

    def summary():
        return pj.ppc_timeseries_summary(np.random.default_rng(1), t, y, yerr, A, Bc, C, Dd, mu=mu, nu=nu, ctx=ctx)

    def replaced():
        ts_array, t_pred = pj.ppc_timeseries(np.random.default_rng(1), t, y, yerr, A, Bc, C, Dd, mu=mu, nu=nu, ctx=ctx)
        ts_array = ts_array[:, ~np.isnan(ts_array[0])]      # a failed sample is a NaN column: dropped, so both paths reduce the same draws
        q = np.quantile(ts_array, FIVE, axis=1)
        idx = np.searchsorted(t_pred, t)
        r = (y[:, None] - ts_array[idx, :]) / yerr[:, None]
        return q, np.quantile(r, FIVE, axis=1), np.mean(r, axis=1)

    def normals():
        g = np.random.default_rng(1)
        return g.standard_normal((B, N)), g.standard_normal((B, M)), g.standard_normal((B, N))

    s = summary(); replaced()
    good = s["status"] == 0
    # outside the timing: np.quantile over the draws that entered the summary (the replaced path leaves a failed draw as a NaN column)
    ts_array, _ = pj.ppc_timeseries(np.random.default_rng(1), t, y, yerr, A, Bc, C, Dd, mu=mu, nu=nu, ctx=ctx)
    q = np.quantile(ts_array[:, good], FIVE, axis=1)
    dev_q = float(np.max(np.abs(s["ts_quantiles"] - q) / np.max(np.abs(ts_array[:, good]), axis=1)[None, :]))
    del ts_array
    tt = {"summary": [], "replaced": [], "normals": []}
    for _ in range(reps):
        for name, fn in (("summary", summary), ("replaced", replaced), ("normals", normals)):
            t0 = time.perf_counter(); fn(); tt[name].append((time.perf_counter() - t0) * 1e3)
    case = {"B": B, "N": N, "M": M, "J": J, "draws_with_status_0": int(good.sum()), "summary_ms": stats(tt["summary"]), "replaced_path_ms": stats(tt["replaced"]),
            "host_normals_ms": stats(tt["normals"]), "max_dev_of_series_quantiles_from_np_quantile_in_units_of_max_abs": dev_q,
            "bytes_back_summary": int(8 * (len(FIVE) * (M + N) + N) + 4 * B), "bytes_back_replaced": int(8 * B * M)}
    case["not_slower"] = case["summary_ms"]["median"] <= case["replaced_path_ms"]["median"]
    ok = ok and case["not_slower"]
    res["ppc"].append(case)

line = json.dumps(res)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
sys.exit(0 if ok else 1)
