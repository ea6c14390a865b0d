#!/usr/bin/env python3
"""TEST INFRASTRUCTURE: generates tests/golden/dense_truth.npz — the yardstick for the dense solver's likelihood (csrc/dense.hip,
pioran_dense_nll / pioran_dense_nll_batch) on the ill-conditioned draws of tests/golden/quad_truth.npz: for every stored draw the truth
(the positive NLL) and the deviation of four fp64 evaluations that are not the code under test from it, |ref - truth| / |truth|.  The
device is held to max(20 x the worst of the four, 256 eps) (tests/dense_cases.check_fixture, tests/test_gpu_dense_truth.py); the host test
(tests/test_dense_host.py) recomputes a slice and asserts the leave-one-out property below on every stored draw.

  n150   all 325 draws of n150_*; truth: minus the stored __float128 value.
  n1000  48 draws of n1000_*: the 24 of lowest ratio and 24 spread evenly over the rest (by rank); truth as above.
         References of both: oracle.dense_nll_numpy (LAPACK), oracle.dense_nll (the C restatement), and both on the time-reversed series
         (-t[::-1], y[::-1], s2[::-1]).
  long   N in LONG_N (both sides of dense_step_kernel's pair / single switch and of its half-tile limit), the prefix of
         oracle.synthetic_series(10_000, seed=1234), the 4 draws of lowest ratio among n10000_* at each size; truth: oracle.logl_quad on the
         prefix.  The C restatement is O(N^3) scalar code: the references are LAPACK forward, LAPACK reversed and LAPACK on two seeded random
         symmetric permutations of the series.

Leave-one-out: on every stored draw each reference is within 20 x the worst of the other three, after the floor of 256 eps — a condition on
the inputs, checked with the references alone; no draw is ever judged by a device result.  n150 and n1000 are stored whole and the host
test asserts it; for `long` this script checks it and replaces a failing draw by the draw of next-lowest ratio, printing which (at most one
per size: more stops the script — that size then needs a third permutation as a fifth reference, to be said here).

The draws are stored as indices into quad_truth.npz; the references' values are stored beside their deviations.  CPU only, a few minutes
on 8 cores.

usage: python oracle/make_dense_truth.py [processes]"""
import os
import sys
import time
from multiprocessing import Pool
from pathlib import Path

if __name__ == "__main__":
    for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):     # one thread per process: the processes are the parallelism
        os.environ.setdefault(_v, "1")

import numpy as np  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from oracle import oracle as O  # noqa: E402

SEED = 20261020
MARGIN = 20
FLOOR = 256 * np.finfo(float).eps
LONG_N = (1536, 1700, 2881, 3100)
N_LONG_DRAWS = 4
REFS = ("lapack", "c", "lapack_reversed", "c_reversed")
REFS_LONG = ("lapack", "lapack_reversed", "lapack_perm0", "lapack_perm1")


def pick_n1000(ratio):
    """the 24 of lowest ratio and 24 spread evenly (by rank) over the rest"""
    o = np.argsort(ratio, kind="stable")
    rest = o[24:]
    return np.concatenate([o[:24], rest[np.round(np.linspace(0, len(rest) - 1, 24)).astype(int)]])


def long_perms(N):
    """the two seeded permutations of the `long` set at size N"""
    return [np.random.default_rng([SEED, N, k]).permutation(N) for k in range(2)]


def reference(name, a, b, c, d, t, y, s2):
    """one fp64 reference by name on the draw (a, b, c, d) and the series (t, y, s2) (y centred, s2 scaled already)"""
    if name.endswith("_reversed"):
        t, y, s2 = -t[::-1], y[::-1], s2[::-1]
    elif "_perm" in name:
        p = long_perms(len(t))[int(name[-1])]
        t, y, s2 = t[p], y[p], s2[p]
    f = O.dense_nll if name.startswith("c") else O.dense_nll_numpy
    return float(f(a, b, c, d, np.ascontiguousarray(t), np.ascontiguousarray(y), np.ascontiguousarray(s2)))


def _job(args):
    return reference(*args)


def leave_one_out(dev):
    """dev (..., R): True where every reference is within MARGIN of the worst of the others, after the floor"""
    dev = np.asarray(dev)
    ok = np.ones(dev.shape[:-1], dtype=bool)
    for r in range(dev.shape[-1]):
        others = np.delete(dev, r, axis=-1).max(axis=-1)
        ok &= dev[..., r] <= np.maximum(MARGIN * others, FLOOR)
    return ok


def series(Q, tag):
    if tag == "n10000":
        return O.synthetic_series(10_000, seed=1234)
    return Q[f"{tag}_t"], Q[f"{tag}_y"], Q[f"{tag}_yerr"]


def draw_args(Q, tag, i, t, y, yerr):
    return (Q[f"{tag}_A"][i], Q[f"{tag}_Bc"][i], Q[f"{tag}_C"], Q[f"{tag}_Dd"], t, y - Q[f"{tag}_mu"][i], Q[f"{tag}_nu"][i] * yerr ** 2)


if __name__ == "__main__":
    nproc = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    Q = np.load(ROOT / "tests" / "golden" / "quad_truth.npz")
    out = {"seed": np.int64(SEED), "refs": np.array(REFS), "refs_long": np.array(REFS_LONG), "long_N": np.array(LONG_N, dtype=np.int64)}
    with Pool(nproc) as pool:
        for tag, idx in (("n150", np.arange(len(Q["n150_ratio"]))), ("n1000", pick_n1000(Q["n1000_ratio"]))):
            t0 = time.time()
            t, y, yerr = series(Q, tag)
            truth = -Q[f"{tag}_truth"][idx]
            jobs = [(r,) + draw_args(Q, tag, i, t, y, yerr) for i in idx for r in REFS]
            val = np.array(pool.map(_job, jobs, chunksize=1)).reshape(len(idx), len(REFS))
            dev = np.abs(val - truth[:, None]) / np.abs(truth[:, None])
            loo = leave_one_out(dev)
            w = dev.max(axis=1)
            print(f"{tag}: {len(idx)} draws in {time.time() - t0:.0f} s; worst reference deviation: median {np.median(w):.2e}, max {w.max():.2e}; LAPACK alone: median "
                  f"{np.median(dev[:, 0]):.2e}, max {dev[:, 0].max():.2e}; leave-one-out fails on {np.flatnonzero(~loo).tolist()}", flush=True)
            out.update({f"{tag}_idx": idx.astype(np.int64), f"{tag}_truth": truth, f"{tag}_ref": val, f"{tag}_ref_dev": dev})

        t, y, yerr = series(Q, "n10000")
        order = np.argsort(Q["n10000_ratio"], kind="stable")
        L_idx, L_truth, L_val, L_dev = [], [], [], []
        for N in LONG_N:
            t0 = time.time()
            tp, yp, ep = t[:N], y[:N], yerr[:N]
            def evaluate(cand):
                truth = np.array([-O.logl_quad(*draw_args(Q, "n10000", i, tp, yp, ep)) for i in cand])
                jobs = [(r,) + draw_args(Q, "n10000", i, tp, yp, ep) for i in cand for r in REFS_LONG]
                val = np.array(pool.map(_job, jobs, chunksize=1)).reshape(len(cand), len(REFS_LONG))
                return truth, val, np.abs(val - truth[:, None]) / np.abs(truth[:, None])
            cand = order[:N_LONG_DRAWS].copy()
            truth, val, dev = evaluate(cand)
            bad = np.flatnonzero(~leave_one_out(dev))
            if len(bad) > 1:
                sys.exit(f"long N = {N}: {len(bad)} draws fail leave-one-out ({cand[bad].tolist()}): this size needs a fifth reference")
            nxt = N_LONG_DRAWS
            while len(bad):
                k = bad[0]
                print(f"long N = {N}: draw {cand[k]} fails leave-one-out (deviations {dev[k]}), replaced by draw {order[nxt]}", flush=True)
                cand[k] = order[nxt]
                tr1, v1, d1 = evaluate(cand[k:k + 1])
                if not leave_one_out(d1)[0]:
                    sys.exit(f"long N = {N}: the replacement {cand[k]} fails too: this size needs a fifth reference")
                truth[k], val[k], dev[k] = tr1[0], v1[0], d1[0]
                bad = bad[1:]
            print(f"long N = {N}: draws {cand.tolist()} in {time.time() - t0:.0f} s; worst reference deviation per draw {dev.max(axis=1)}", flush=True)
            L_idx.append(cand); L_truth.append(truth); L_val.append(val); L_dev.append(dev)
        out.update(long_idx=np.array(L_idx, dtype=np.int64), long_truth=np.array(L_truth), long_ref=np.array(L_val), long_ref_dev=np.array(L_dev))
    np.savez_compressed(ROOT / "tests" / "golden" / "dense_truth.npz", **out)
    print("wrote tests/golden/dense_truth.npz")
