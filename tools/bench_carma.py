#!/usr/bin/env python3
"""The CARMA(p, q) entries (carma.hip) at the reference's own order, CARMA(5, 2), N = 1e4, for B in {1, 64, 4096} draws, one box, one process:

(a) value: the host chain — a Python loop of pj.CARMA(...).celerite_coefs() over the draws + Dataset.logl_batch with per-draw (C, Dd) — against
    Dataset.logpdf_carma, by the host clock (both block);
(b) gradient: Dataset.logl_grad + the twin's reverse mode on the host (tools/carma_proto.py vjp_quad, which recomputes the forward map as the
    kernel does; the coefficient loop of (a) in front) against Dataset.logpdf_carma_grad, without and with `shift` (B <= --grad-B-max draws: the
    shifted per-draw reverse mode goes draw by draw);
(c) the three small kernels alone, from the event slots 4 | 5 the context records with option "carma_events": carma_coefs_kernel,
    carma_vjp_kernel, and the two PSD kernels together at B = 2000, F = 1000;
(d) the PSD summary at B = 2000, F = 1000 (Context.carma_psd_summary) against the host twin (carma_proto.evaluate_roots + np.quantile);
(e) what the figures are read against: the box's FP64 FMA rate (Context.fp64_probe), as the other bench tools record it.

No time is promised: nobody had measured this path.  Every figure: one untimed run, then `--reps` timed ones, median with minimum and maximum.
One JSON line; `--out FILE` also writes it there.  Exit status 1 if a device call is slower than the chain it replaces at the largest B."""
import argparse, json, os, socket, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import carma_proto as cp
import pioran_jl_amd as pj

ap = argparse.ArgumentParser()
ap.add_argument("--N", type=int, default=10_000)
ap.add_argument("--B", type=int, nargs="+", default=[1, 64, 4096])
ap.add_argument("--grad-B-max", type=int, default=4096)
ap.add_argument("--shift-B-max", type=int, default=64)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=None)
args = ap.parse_args()
p, q = 5, 2


def stats(ts):
    ts = np.asarray(ts) * 1e3
    return dict(median_ms=float(np.median(ts)), min_ms=float(ts.min()), max_ms=float(ts.max()))


def timed(fn, reps=args.reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
    return stats(ts)


def kernel_ms(fn, reps=args.reps):
    fn()
    ts = []
    for _ in range(reps):
        fn(); ts.append(ctx.event_elapsed_ms(4, 5) * 1e-3)
    return stats(ts)


rng = np.random.default_rng(0)
t = np.cumsum(rng.uniform(0.05, 2.0, args.N))
y = 5.0 + 0.3 * rng.standard_normal(args.N)
yerr = rng.uniform(0.01, 0.05, args.N)
f_min, f_max = 1 / (t[-1] - t[0]), 1 / np.min(np.diff(t)) / 2
ctx = pj.Context(0)
ds = pj.Dataset(t, y, yerr ** 2, ctx)
res = dict(host=socket.gethostname(), N=args.N, p=p, q=q, reps=args.reps, fp64_fma_TFLOPs=ctx.fp64_probe(), value={}, grad={}, grad_shift={}, kernels={})


def draws(B):
    qa, qb = np.empty((B, p)), np.empty((B, q))
    for k in range(B):
        qa[k], qb[k] = pj.sample_quad(p, q, rng, f_min, f_max)
    return qa, qb, np.exp(np.log(0.5) + 0.5 * rng.standard_normal(B)), 5.0 + 0.05 * rng.standard_normal(B), rng.uniform(0.8, 1.5, B)


def host_coefs(qa, qb, norm):
    co = [pj.CARMA(p, q, pj.quad2roots(qa[k]), pj.roots2coeffs(pj.quad2roots(qb[k])).real, norm[k]).celerite_coefs() for k in range(len(qa))]
    return [np.ascontiguousarray(np.array([c[i] for c in co])) for i in range(4)]


slower = []
for B in args.B:
    qa, qb, norm, mu, nu = draws(B)
    shift = np.full(B, 0.2)
    chain = lambda: ds.logl_batch(*host_coefs(qa, qb, norm), mu=mu, nu=nu)
    one = lambda: ds.logpdf_carma(p, q, qa, qb, norm, mu=mu, nu=nu)
    v = dict(chain=timed(chain), device=timed(one), kernel=pj._lib.lib().pioran_celerite_config_name(-1).decode())
    v["max_rel_dev"] = float(np.max(np.abs(one() - chain()) / np.abs(chain())))
    res["value"][str(B)] = v
    if B == max(args.B) and v["device"]["median_ms"] > v["chain"]["median_ms"]:
        slower.append(f"value B={B}")
    if B <= args.grad_B_max:
        for key, sh, lim in (("grad", None, args.grad_B_max), ("grad_shift", shift, args.shift_B_max)):
            if B > lim:
                continue
            m = None if sh is None else np.log(mu)

            def gchain():
                g = ds.logl_grad(*host_coefs(qa, qb, norm), mu=m if sh is not None else mu, nu=nu, shift=sh, cd_grad=True)
                return cp.vjp_quad(qa, qb, norm, True, g["grad_a"], g["grad_b"], g["grad_c"], g["grad_d"])
            gone = lambda: ds.logpdf_carma_grad(p, q, qa, qb, norm, mu=m if sh is not None else mu, nu=nu, shift=sh)
            r = dict(chain=timed(gchain), device=timed(gone), kernel=pj._lib.lib().pioran_celerite_config_name(-1).decode())
            res[key][str(B)] = r
            if B == min(max(args.B), lim) and r["device"]["median_ms"] > r["chain"]["median_ms"]:
                slower.append(f"{key} B={B}")
    ctx.set_option("carma_events", True)
    g4 = rng.standard_normal((4, B, (p + 1) // 2))
    res["kernels"][str(B)] = dict(coefs=kernel_ms(lambda: ctx.carma_coefs(p, q, qa, qb, norm)), vjp=kernel_ms(lambda: ctx.carma_vjp(p, q, qa, qb, norm, *g4)))
    ctx.set_option("carma_events", False)

Bp, F = 2000, 1000
qa, qb, norm, _, _ = draws(Bp)
r_alpha, beta = cp.roots_of_quad(qa, qb)
f = np.exp(np.linspace(np.log(f_min / 10), np.log(10 * f_max), F))
dev_sum = lambda: ctx.carma_psd_summary(p, q, f, r_alpha=r_alpha, beta=beta, norm=norm)
host_sum = lambda: np.quantile(cp.evaluate_roots(r_alpha, beta, norm, True, f), pj.gp.PPC_QUANTILES, axis=0)
res["psd_summary"] = dict(B=Bp, F=F, device=timed(dev_sum), host_twin=timed(host_sum),
                          max_rel_dev=float(np.max(np.abs(dev_sum()["quant"] - host_sum()) / host_sum())))
ctx.set_option("carma_events", True)
res["kernels"]["psd_B2000_F1000"] = kernel_ms(dev_sum)
ctx.set_option("carma_events", False)
if res["psd_summary"]["device"]["median_ms"] > res["psd_summary"]["host_twin"]["median_ms"]:
    slower.append("psd summary")
res["slower_than_chain"] = slower
line = json.dumps(res)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
sys.exit(1 if slower else 0)
