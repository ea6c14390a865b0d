#!/usr/bin/env python3
"""TEST INFRASTRUCTURE: generates tests/golden/predict_var_truth.npz — the posterior variance k(0) - k*' K^-1 k* on ill-conditioned draws of
tests/golden/quad_truth.npz (SHO-20, 40 rows), the truth against which the numpy prototype of the variance recurrences
(tools/predict_var_proto.py) and the HIP kernels (predict_var_fwd_kernel / predict_var_bwd_kernel) are held
(tests/test_predict_var_host.py, tests/test_gpu_predict_var.py::test_ill_conditioned_draws_against_truth).

  N = 150   six draws of n150_* by ratio = nu min(sigma2) / sum(a): the two lowest, the median, the highest and the two quartiles; 24 evaluation
            times (14 inside the span, two before, two after, t[[0, 1, 74, 75, 148, 149]]); truth: a dense evaluation with mpmath at 50 digits
            (its own kernel function, Cholesky and substitutions; nothing of numpy's arithmetic).
  N = 1000  three draws of n1000_*: lowest ratio, median, highest; 40 evaluation times of the same mix; truth: oracle.predict_var_truth in long
            double (mpmath is O(N^3) in software arithmetic: hours at this size).
  ld_dev    what entitles the second to be called a truth: the long-double function's deviation from the 50-digit values on the six N = 150
            draws, in units of k(0).

The draws are stored as indices into quad_truth.npz.  Every truth is stored as a pair of doubles (hi + lo): one double rounds a variance of the
size of k(0) by 1e-16 k(0), more than the long-double error to be recorded.  CPU only; needs mpmath (here alone); about 20 s per N = 150 draw (the draws
in parallel) and 15 s per N = 1000 draw.

usage: python oracle/make_predict_var_truth.py [processes]"""
import sys
import time
from multiprocessing import Pool
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from oracle import oracle as O  # noqa: E402

SEED = 20261018
DIGITS = 50


def pick(ratio, which):
    o = np.argsort(ratio, kind="stable")
    n = len(o)
    pos = {"six": [0, 1, n // 4, n // 2, (3 * n) // 4, n - 1], "three": [0, n // 2, n - 1]}[which]
    return o[pos]


def make_tau(t, n_in, rng):
    """n_in times inside the span, two before it, two after it, and six data times (both ends and the middle), in this order"""
    N = len(t)
    span = t[-1] - t[0]
    return np.concatenate([rng.uniform(t[0], t[-1], n_in), t[0] - rng.uniform(0, 0.05 * span, 2), t[-1] + rng.uniform(0, 0.05 * span, 2),
                           t[[0, 1, N // 2 - 1, N // 2, N - 2, N - 1]]])


def truth_mpmath(args):
    """the variance at every tau as (hi, lo) doubles: dense, 50 digits, the fp64 inputs taken exactly"""
    import mpmath as mp
    a, b, c, d, tau, t, s2 = args
    mp.mp.dps = DIGITS
    J, N, M = len(a), len(t), len(tau)
    a, b, c, d = ([mp.mpf(float(x)) for x in v] for v in (a, b, c, d))
    t = [mp.mpf(float(x)) for x in t]; tau = [mp.mpf(float(x)) for x in tau]; s2 = [mp.mpf(float(x)) for x in s2]
    def kern(dt):
        dt = abs(dt)
        return mp.fsum(mp.exp(-c[j] * dt) * (a[j] * mp.cos(d[j] * dt) + b[j] * mp.sin(d[j] * dt)) for j in range(J))
    k0 = mp.fsum(a)
    L = [[mp.mpf(0)] * N for _ in range(N)]
    for n in range(N):
        for j in range(n):
            L[n][j] = (kern(t[n] - t[j]) - mp.fdot(L[n][:j], L[j][:j])) / L[j][j]
        piv = k0 + s2[n] - mp.fdot(L[n][:n], L[n][:n])
        assert piv > 0, n
        L[n][n] = mp.sqrt(piv)
    hi, lo = np.empty(M), np.empty(M)
    for m in range(M):
        w = [mp.mpf(0)] * N
        for n in range(N):
            w[n] = (kern(tau[m] - t[n]) - mp.fdot(L[n][:n], w[:n])) / L[n][n]
        v = k0 - mp.fdot(w, w)
        hi[m] = float(v); lo[m] = float(v - mp.mpf(hi[m]))
    return hi, lo


if __name__ == "__main__":
    nproc = int(sys.argv[1]) if len(sys.argv) > 1 else 6
    Q = np.load(ROOT / "tests" / "golden" / "quad_truth.npz")
    out = {"seed": np.int64(SEED), "digits": np.int64(DIGITS)}
    rng = np.random.default_rng(SEED)

    t, yerr = Q["n150_t"], Q["n150_yerr"]
    idx = pick(Q["n150_ratio"], "six")
    tau = make_tau(t, 14, rng)
    assert len(tau) == 24
    jobs = [(Q["n150_A"][i], Q["n150_Bc"][i], Q["n150_C"], Q["n150_Dd"], tau, t, Q["n150_nu"][i] * yerr ** 2) for i in idx]
    t0 = time.time()
    with Pool(min(nproc, len(jobs))) as pool:
        res = pool.map(truth_mpmath, jobs)
    hi = np.array([r[0] for r in res]); lo = np.array([r[1] for r in res])
    ld_dev = np.empty(len(idx))
    for k, job in enumerate(jobs):
        ld = O.predict_var_truth(*job)
        ld_dev[k] = float(np.max(np.abs((ld - hi[k].astype(np.longdouble)) - lo[k].astype(np.longdouble))) / np.sum(job[0]))
        print(f"N = 150 draw {idx[k]}: ratio {Q['n150_ratio'][idx[k]]:.2e}  min var / k(0) {hi[k].min() / np.sum(job[0]):.2e}  long double vs {DIGITS} digits "
              f"{ld_dev[k]:.2e} k(0)", flush=True)
    print(f"N = 150: {len(idx)} draws in {time.time() - t0:.0f} s")
    out.update(n150_idx=idx.astype(np.int64), n150_tau=tau, n150_truth_hi=hi, n150_truth_lo=lo, ld_dev=ld_dev)

    t, yerr = Q["n1000_t"], Q["n1000_yerr"]
    idx = pick(Q["n1000_ratio"], "three")
    tau = make_tau(t, 30, rng)
    assert len(tau) == 40
    hi = np.empty((len(idx), len(tau))); lo = np.empty_like(hi)
    for k, i in enumerate(idx):
        t0 = time.time()
        ld = O.predict_var_truth(Q["n1000_A"][i], Q["n1000_Bc"][i], Q["n1000_C"], Q["n1000_Dd"], tau, t, Q["n1000_nu"][i] * yerr ** 2)
        hi[k] = ld.astype(np.float64); lo[k] = (ld - hi[k].astype(np.longdouble)).astype(np.float64)
        print(f"N = 1000 draw {i}: ratio {Q['n1000_ratio'][i]:.2e}  min var / k(0) {hi[k].min() / Q['n1000_A'][i].sum():.2e}  ({time.time() - t0:.0f} s)", flush=True)
    out.update(n1000_idx=idx.astype(np.int64), n1000_tau=tau, n1000_truth_hi=hi, n1000_truth_lo=lo)
    np.savez_compressed(ROOT / "tests" / "golden" / "predict_var_truth.npz", **out)
    print("wrote tests/golden/predict_var_truth.npz")
