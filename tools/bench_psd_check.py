#!/usr/bin/env python3
"""The PSD check (psd_check.hip) at the size of the reference's prior check, B = 2000 draws x F = 1000 frequencies x J = 20 components, for the
SHO and the DRWCelerite basis, one box, one process:

(a) the summary call (Context.psd_check_summary: five quantiles, mean and meta), by the host clock (the call blocks);
(b) the array call (Context.psd_check, all four arrays) with the download, by the host clock, and without it: the device-pointer entry
    (Context.psd_check_dev) timed with the context's event slots 0 / 1;
(c) the two new kernels alone, from the event slots 4 .. 6 the context records with option "pc_events";
(d) the host chain it replaces: psd._eval_model_batch on the frequencies and on the spectral grid, np.linalg.solve for the amplitudes, the sum
    over the basis functions, and np.quantile / np.mean of residuals and ratios;
(e) what the figures are read against: the box's FP64 FMA rate (Context.fp64_probe) and its device copy rate (a 1 GiB torch copy), as the other
    bench tools record them; the evaluation kernel's arithmetic is B F J (2 divisions + 5 multiply/adds) + B F (2 or 3 pow), its stores 6 B F 8 bytes
    with the transposed copies.

No rate is promised: nobody had measured this path.  Every figure: one untimed run, then `--reps` timed ones (at least 10), median with minimum
and maximum.  One JSON line; `--out FILE` also writes it there."""
import argparse, json, os, socket, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pioran_jl_amd as pj
from pioran_jl_amd import psd as PSD

FIVE = (0.025, 0.16, 0.5, 0.84, 0.975)
ap = argparse.ArgumentParser()
ap.add_argument("--B", type=int, default=2000)
ap.add_argument("--F", type=int, default=1000)
ap.add_argument("--J", type=int, default=20)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--out", default=None)
args = ap.parse_args()
reps = max(10, args.reps)
B, F, J = args.B, args.F, args.J

import torch
ctx = pj.Context(0)
dev = torch.device("cuda:0")
rng = np.random.default_rng(0)


def stats(ts):
    return {"median": float(np.median(ts)), "min": float(np.min(ts)), "max": float(np.max(ts)), "reps": len(ts)}


def clock(fn):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); ts.append((time.perf_counter() - t0) * 1e3)
    return stats(ts)


res = {"box": socket.gethostname(), "device": torch.cuda.get_device_name(0), "B": B, "F": F, "J": J, "cases": []}
res["fp64_fma_TFLOPs"] = ctx.fp64_probe()
src = torch.empty(1 << 27, dtype=torch.float64, device=dev).normal_()
dst = torch.empty_like(src)
dst.copy_(src); torch.cuda.synchronize()
ts = []
for _ in range(reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); dst.copy_(src); e1.record(); torch.cuda.synchronize()
    ts.append(e0.elapsed_time(e1))
res["copy_rate_TBps"] = 2.0 * src.numel() * 8 / (np.median(ts) * 1e-3) / 1e12
del src, dst

# the prior of the reference's modelling guide, the observed window of its example
f_min, f_max, S = 5e-3, 200.0, 20.0
f0, fM = f_min / S, f_max * S
a1 = rng.uniform(0.0, 1.25, B)
theta = np.column_stack([a1, 10.0 ** rng.uniform(-3, 3, B), a1 + (4.0 - a1) * rng.uniform(size=B)])
norm = np.exp(-1.0 + 2.0 * rng.standard_normal(B))
freq = 10.0 ** np.linspace(np.log10(f0), np.log10(fM), F)
model = pj.SingleBendingPowerLaw

for basis in ("SHO", "DRWCelerite"):
    kw = dict(basis_function=basis)
    case = {"basis": basis}
    case["summary_ms"] = clock(lambda: ctx.psd_check_summary(model, theta, norm, freq, f0, fM, J, 1.0, 1.0, probs=FIVE, **kw))
    case["arrays_with_download_ms"] = clock(lambda: ctx.psd_check(model, theta, norm, freq, f0, fM, J, 1.0, 1.0, **kw))
    dth, dnm, dfr = (torch.from_numpy(a).to(dev) for a in (theta, norm, freq))
    outs = [torch.empty((B, F), dtype=torch.float64, device=dev) for _ in range(4)]
    torch.cuda.synchronize()

    def on_device():
        ctx.psd_check_dev(B, F, model, dth.data_ptr(), dnm.data_ptr(), dfr.data_ptr(), f0, fM, J, 1.0, 1.0, dpsd=outs[0].data_ptr(),
                          dpsd_approx=outs[1].data_ptr(), dresiduals=outs[2].data_ptr(), dratios=outs[3].data_ptr(), **kw)

    on_device(); ctx.synchronize()
    ctx.set_option("pc_events", True)
    t_all, t_draw, t_eval = [], [], []
    for _ in range(reps):
        ctx.event_record(0); on_device(); ctx.event_record(1); ctx.synchronize()
        t_all.append(ctx.event_elapsed_ms(0, 1)); t_draw.append(ctx.event_elapsed_ms(4, 5)); t_eval.append(ctx.event_elapsed_ms(5, 6))
    ctx.set_option("pc_events", False)
    case["arrays_on_device_ms"] = stats(t_all)
    case["draw_kernel_ms"] = stats(t_draw)
    case["eval_kernel_ms"] = stats(t_eval)
    pw = 4 if basis == "SHO" else 6
    sp, Bm = PSD.build_approx(J, f0, fM, basis)

    def host_chain():
        p = PSD._eval_model_batch(model, theta, sp)
        amp = np.linalg.solve(Bm, (p / p[:, :1]).T).T
        psd = PSD._eval_model_batch(model, theta, freq)
        psd = psd / psd[:, :1] * norm[:, None]
        approx = np.zeros((B, F))
        for j in range(J):
            approx += (amp[:, j] * norm)[:, None] / (1.0 + (freq / sp[j]) ** pw)[None, :]
        r, q = psd - approx, approx / psd
        return (np.quantile(r, FIVE, axis=0), np.quantile(q, FIVE, axis=0), r.mean(axis=0), q.mean(axis=0), np.median(r, axis=1), np.median(q, axis=1),
                r.mean(axis=1), q.mean(axis=1), np.abs(r).min(axis=1), np.abs(r).max(axis=1), np.abs(q).min(axis=1), np.abs(q).max(axis=1))

    case["host_chain_ms"] = clock(host_chain)
    s = ctx.psd_check_summary(model, theta, norm, freq, f0, fM, J, 1.0, 1.0, probs=FIVE, **kw)
    h = host_chain()
    case["kept"] = int(s["kept"])
    case["max_rel_dev_of_ratio_quantiles_from_host_chain"] = float(np.nanmax(np.abs(s["quant"][3] - h[1]) / np.abs(h[1])))
    ev = np.median(t_eval) * 1e-3
    case["eval_kernel_terms_per_s"] = B * F * J / ev
    case["eval_kernel_store_TBps"] = 4 * B * F * 8 / ev / 1e12
    res["cases"].append(case)

line = json.dumps(res)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
