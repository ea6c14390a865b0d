#!/usr/bin/env python3
"""Value and gradient of log L with respect to the sampled PSD parameters (Dataset.logpdf_theta_grad): the host chain (approx_on="host": approx on
the host, the reverse mode on the device, approx_batch_vjp on the host) against the single device call (approx_on="device":
pioran_logpdf_batch_theta_grad), one box, one process, the two alternating.

Workloads at N = 1e4, 20 components, mu and nu given: 1, 64 and 4096 chains of SHO, 4096 chains of DRWCelerite.  Per workload:
  wall time per call of each path by the host clock (both block): one untimed call of each, then `--reps` timed pairs (at least 10), median
    with minimum and maximum;
  approx_kernel and approx_vjp_kernel alone, from the context's event slots (context option "theta_events": slots 4 | 5 around the staging of
    a chunk's draws — the upload of its mu, nu and approx_kernel —, 6 | 7 around approx_vjp_kernel and the download of its results), taken in
    five more calls with "workspace_limit_mb" raised so that the whole batch is ONE chunk, and their share of that call;
  the bytes each path moves each way (counted, not measured).
The one condition: the device call is not slower than the host chain at any workload (exit status 1 otherwise).  The share of the two small
kernels is reported with `small_kernels_under_1_percent` for the 4096-chain workloads.  One JSON line; `--out FILE` also writes it there."""
import argparse, json, os, socket, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pioran_jl_amd as pj

ap = argparse.ArgumentParser()
ap.add_argument("--N", type=int, default=10_000)
ap.add_argument("--J", type=int, default=20)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--workloads", nargs="+", default=["SHO:1", "SHO:64", "SHO:4096", "DRWCelerite:4096"])
ap.add_argument("--out", default=None)
args = ap.parse_args()
reps = max(10, args.reps)

import torch
ctx = pj.Context(0)
rng = np.random.default_rng(0)
N, J = args.N, args.J
t = np.cumsum(0.05 + rng.exponential(0.95, N))
yerr = rng.uniform(0.05, 0.2, N)
y = np.sin(0.01 * t) + 0.3 * rng.standard_normal(N)
f_min, f_max = 1.0 / (t[-1] - t[0]), 1.0 / (2.0 * np.min(np.diff(t)))
ds = pj.Dataset(t, y, yerr ** 2, ctx)


def stats(ts):
    return {"median": float(np.median(ts)), "min": float(np.min(ts)), "max": float(np.max(ts)), "reps": len(ts)}


res = {"box": socket.gethostname(), "device": torch.cuda.get_device_name(0), "N": N, "n_components": J, "workloads": []}
ok = True
for w in args.workloads:
    basis, B = w.split(":")[0], int(w.split(":")[1])
    theta = np.column_stack([rng.uniform(-0.25, 2.0, B), np.exp(rng.uniform(np.log(f_min), np.log(f_max), B)), rng.uniform(1.5, 4.0, B)])
    norm = np.var(y) * np.exp(0.3 * rng.standard_normal(B))
    mu, nu = np.mean(y) + 0.1 * rng.standard_normal(B), rng.gamma(2.0, 0.5, B) + 0.2
    call = lambda where: ds.logpdf_theta_grad(pj.SingleBendingPowerLaw, theta, norm, f_min, f_max, J, basis_function=basis, mu=mu, nu=nu, approx_on=where)
    gh, gd = call("host"), call("device")
    family = pj._lib.lib().pioran_celerite_config_name(-1).decode()
    good = (gh["status"] == 0) & (gd["status"] == 0)
    scale = np.max(np.abs(gh["grad_theta"][good]), axis=0)
    dev = float(np.max(np.abs(gd["grad_theta"][good] - gh["grad_theta"][good]) / scale))
    tt = {"host": [], "device": []}
    for _ in range(reps):
        for where in ("host", "device"):
            t0 = time.perf_counter(); call(where); tt[where].append((time.perf_counter() - t0) * 1e3)
    # the two small kernels alone, the whole batch one chunk
    ctx.set_option("workspace_limit_mb", 131072)
    ctx.set_option("theta_events", 1)
    call("device")
    one, ka, kv = [], [], []
    for _ in range(5):
        t0 = time.perf_counter(); call("device"); one.append((time.perf_counter() - t0) * 1e3)
        ka.append(ctx.event_elapsed_ms(4, 5)); kv.append(ctx.event_elapsed_ms(6, 7))
    ctx.set_option("theta_events", None)
    ctx.set_option("workspace_limit_mb", None)
    ctx.trim()
    Jt, P = J * (1 if basis == "SHO" else 2), 3
    share = (float(np.median(ka)) + float(np.median(kv))) / float(np.median(one))
    case = {"basis": basis, "chains": B, "kernel_family": family, "draws_with_status_0": int(good.sum()),
            "host_chain_ms": stats(tt["host"]), "device_call_ms": stats(tt["device"]),
            "host_over_device": float(np.median(tt["host"]) / np.median(tt["device"])),
            "one_chunk_device_call_ms": stats(one), "approx_stage_ms": stats(ka), "approx_vjp_stage_ms": stats(kv), "small_kernels_share_of_call": share,
            "max_dev_grad_theta_device_from_host_in_units_of_max_abs": dev,
            "bytes_up_host_chain": int(8 * B * (2 * Jt + 2)), "bytes_down_host_chain": int(8 * B * (2 * Jt + 3) + 4 * B),
            "bytes_up_device_call": int(8 * B * (P + 3) + 8 * (2 * J + J * J) + 4 * J), "bytes_down_device_call": int(8 * B * (P + 4) + 4 * B)}
    case["not_slower"] = case["device_call_ms"]["median"] <= case["host_chain_ms"]["median"]
    if B >= 4096:
        case["small_kernels_under_1_percent"] = share < 0.01
    ok = ok and case["not_slower"]
    res["workloads"].append(case)
    print(json.dumps(case), file=sys.stderr, flush=True)

line = json.dumps(res)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
sys.exit(0 if ok else 1)
