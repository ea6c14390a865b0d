#!/usr/bin/env python3
"""Batched Lomb-Scargle periodogram (Context.lombscargle[_dev]) at the size of the reference's posterior predictive check:
N = 1e4 irregular times, F = 1000 frequencies of its grid, B = 1000 and 256 series.

Per phase (weights + table, series scalars, product) with the context's event slots around the device-pointer entry restricted to that phase
(context option "ls_only"), for both output tiles of the product ("ls_tile" 64 / 128); the product's share of the fp64 matrix peak on
2 B N 2F flop; the host-pointer entry (upload, run, download) by the host clock; and scipy.signal.lombscargle on ONE series of the same size
on the host, times B — an extrapolation.  One JSON line; `--out FILE` also writes it there."""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pioran_jl_amd as pj

FP64_PEAK_TFLOPS = 78.6   # MI355X fp64 matrix peak (vendor), as in bench.py

ap = argparse.ArgumentParser()
ap.add_argument("--N", type=int, default=10_000)
ap.add_argument("--F", type=int, default=1000)
ap.add_argument("--B", type=int, nargs="+", default=[1000, 256])
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--no-scipy", action="store_true")
ap.add_argument("--out", default=None)
args = ap.parse_args()

import torch
N, F = args.N, args.F
rng = np.random.default_rng(0)
t = np.cumsum(0.05 + rng.exponential(0.95, N))
yerr = rng.uniform(0.05, 0.2, N)
f_min, f_max = 1 / (t[-1] - t[0]), 1 / np.min(np.diff(t)) / 2
freq = np.exp(np.linspace(np.log(f_min / 20), np.log(f_max * 20), F + 1))[:-1]
ctx = pj.Context(0)
dev = torch.device("cuda:0")


def phase_ms(run, only, reps):
    """median of `reps` event-timed runs of the phases `only` (0 = all); one untimed run first"""
    ctx.set_option("ls_only", only or None)
    run(); ctx.synchronize()
    ts = []
    for _ in range(reps):
        ctx.event_record(0); run(); ctx.event_record(1)
        ts.append(ctx.event_elapsed_ms(0, 1))
    ctx.set_option("ls_only", None)
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


res = {"N": N, "F": F, "fp64_peak_tflops": FP64_PEAK_TFLOPS, "fp64_fma_ceiling_tflops_now": ctx.fp64_probe(), "cases": []}
for B in args.B:
    Y = rng.standard_normal((B, N)) + np.sin(0.3 * t)[None, :]
    dt, dY, de, df = (torch.from_numpy(a).to(dev) for a in (t, Y, yerr, freq))
    dP = torch.empty((B, F), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    run = lambda: ctx.lombscargle_dev(N, B, F, dt.data_ptr(), dY.data_ptr(), de.data_ptr(), df.data_ptr(), dpower=dP.data_ptr())
    case = {"B": B, "tiles": {}}
    flop = 2.0 * B * N * 2 * F
    first = None
    for tile in (64, 128):
        ctx.set_option("ls_tile", tile)
        run(); ctx.synchronize()      # all phases once: the workspace the single phases run on
        got = dP.cpu().numpy()
        first = got if first is None else first
        all_ms = phase_ms(run, 0, args.reps)
        tab, ser, prod = (phase_ms(run, k, args.reps) for k in (1, 2, 4))
        case["tiles"][str(tile)] = {"all_ms": all_ms[0], "table_ms": tab[0], "series_ms": ser[0], "product_ms": prod[0], "product_ms_min_max": prod[1:],
                                    "product_tflops": flop / prod[0] / 1e9, "product_share_of_fp64_matrix_peak": flop / prod[0] / 1e9 / FP64_PEAK_TFLOPS,
                                    "bit_identical_to_tile_64": bool(np.array_equal(got, first))}
    ctx.set_option("ls_tile", None)
    ctx.lombscargle(t, Y, yerr, freq)
    hs = []
    for _ in range(3):
        t0 = time.perf_counter(); host = ctx.lombscargle(t, Y, yerr, freq); hs.append(time.perf_counter() - t0)
    case["host_form_ms_pcie_inclusive"] = float(np.median(hs)) * 1e3
    case["host_form_bytes_each_way"] = [int(Y.nbytes), int(host.nbytes)]
    res["cases"].append(case)

if not args.no_scipy:
    from scipy import signal
    w = yerr ** -2.0 / np.sum(yerr ** -2.0)
    y1 = rng.standard_normal(N)
    f = lambda: signal.lombscargle(t, y1 - np.sum(w * y1), 2 * np.pi * freq, weights=w, floating_mean=True, normalize=True)
    f()
    t0 = time.perf_counter(); f(); one = time.perf_counter() - t0
    res["scipy_one_series_s"] = one
    res["scipy_threads"] = 1   # scipy.signal.lombscargle runs on the calling thread
    res["scipy_extrapolated_s"] = {str(B): one * B for B in args.B}
line = json.dumps(res)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
