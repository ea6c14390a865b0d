#!/usr/bin/env python3
"""Value and gradient of log L with respect to the sampled parameters of a continuum + QPO model (Dataset.logpdf_theta_grad(qpo=...)): the host
chain (approx_on="host": approx_batch_qpo on the host, the reverse mode with (c, d) per draw on the device, approx_batch_qpo_vjp on the host)
against the single call (approx_on="device": pioran_logpdf_batch_theta_qpo_grad), one box, one process, the two alternating.

Workloads at N = 1e4, SHO with 20 components + 1 QPO (42 rows), mu and nu given: 1, 16, 64 and 256 chains.  Per workload:
  wall time per call of each path by the host clock (both block): one untimed call of each, then `--reps` timed pairs (at least 10), median
    with minimum and maximum;
  approx_qpo_vjp_kernel alone, from the context's event slots (context option "theta_events": slots 6 | 7 around the kernel), in five more calls.
The one condition: the device call is not slower than the host chain at any workload (exit status 1 otherwise).  One JSON line; `--out FILE`
also writes it there."""
import argparse, json, os, socket, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pioran_jl_amd as pj

ap = argparse.ArgumentParser()
ap.add_argument("--N", type=int, default=10_000)
ap.add_argument("--J", type=int, default=20)
ap.add_argument("--n-qpo", type=int, default=1)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--chains", type=int, nargs="+", default=[1, 16, 64, 256])
ap.add_argument("--out", default=None)
args = ap.parse_args()
reps = max(10, args.reps)

import torch
ctx = pj.Context(0)
rng = np.random.default_rng(0)
N, J, nq = args.N, args.J, args.n_qpo
t = np.cumsum(0.05 + rng.exponential(0.95, N))
yerr = rng.uniform(0.05, 0.2, N)
y = np.sin(0.01 * t) + 0.3 * rng.standard_normal(N)
f_min, f_max = 1.0 / (t[-1] - t[0]), 1.0 / (2.0 * np.min(np.diff(t)))
ds = pj.Dataset(t, y, yerr ** 2, ctx)


def stats(ts):
    return {"median": float(np.median(ts)), "min": float(np.min(ts)), "max": float(np.max(ts)), "reps": len(ts)}


res = {"box": socket.gethostname(), "device": torch.cuda.get_device_name(0), "N": N, "n_components": J, "n_qpo": nq, "workloads": []}
ok = True
for B in args.chains:
    theta = np.column_stack([rng.uniform(-0.25, 2.0, B), np.exp(rng.uniform(np.log(f_min), np.log(f_max), B)), rng.uniform(1.5, 4.0, B)])
    qpo = np.stack([rng.uniform(0.05, 2.0, (B, nq)), np.exp(rng.uniform(np.log(20 * f_min), np.log(f_max / 5), (B, nq))),
                    rng.uniform(2.0, 20.0, (B, nq))], axis=2)
    norm = np.var(y) * np.exp(0.3 * rng.standard_normal(B))
    mu, nu = np.mean(y) + 0.1 * rng.standard_normal(B), rng.gamma(2.0, 0.5, B) + 0.2
    call = lambda where: ds.logpdf_theta_grad(pj.SingleBendingPowerLaw, theta, norm, f_min, f_max, J, mu=mu, nu=nu, qpo=qpo, approx_on=where)
    gh = call("host")
    family = pj._lib.lib().pioran_celerite_config_name(-1).decode()      # the host chain ends with the reverse mode of the likelihood
    gd = call("device")
    good = (gh["status"] == 0) & (gd["status"] == 0)
    both = lambda g: np.column_stack([g["grad_theta"], g["grad_norm"], g["grad_qpo"].reshape(B, -1)])[good]
    scale = np.max(np.abs(both(gh)), axis=0)
    dev = float(np.max(np.abs(both(gd) - both(gh)) / scale)) if good.any() else float("nan")
    tt = {"host": [], "device": []}
    for _ in range(reps):
        for where in ("host", "device"):
            t0 = time.perf_counter(); call(where); tt[where].append((time.perf_counter() - t0) * 1e3)
    ctx.set_option("theta_events", 1)
    call("device")
    kv = []
    for _ in range(5):
        call("device")
        kv.append(ctx.event_elapsed_ms(6, 7))
    ctx.set_option("theta_events", None)
    Jt, P = J + nq, 3
    case = {"basis": "SHO", "chains": B, "kernel_family": family, "draws_with_status_0": int(good.sum()),
            "host_chain_ms": stats(tt["host"]), "device_call_ms": stats(tt["device"]),
            "host_over_device": float(np.median(tt["host"]) / np.median(tt["device"])),
            "approx_qpo_vjp_kernel_ms": stats(kv), "vjp_kernel_share_of_call": float(np.median(kv) / np.median(tt["device"])),
            "max_dev_grad_device_from_host_in_units_of_max_abs": dev,
            "bytes_up_host_chain": int(8 * B * (4 * Jt + 2)), "bytes_down_host_chain": int(8 * B * (4 * Jt + 3) + 4 * B),
            "bytes_up_device_call": int(8 * B * (P + 3 + 3 * nq + 8 * Jt) + 8 * (2 * J + J * J) + 4 * J),
            "bytes_down_device_call": int(8 * B * (P + 4 + 3 * nq + 8 * Jt) + 4 * B)}
    case["not_slower"] = case["device_call_ms"]["median"] <= case["host_chain_ms"]["median"]
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
