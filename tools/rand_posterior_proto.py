"""NumPy twin of the posterior-draw chain (pioran_celerite_rand_posterior, capi.hip rand_posterior_batch): Matheron's rule

    out(tau) = f~(tau) + k*(tau)' K^-1 (y - f~(t) - eta),   K = k(t, t) + diag(nu sigma2),   eta_n = sqrt(nu sigma2_n) eps_n

composed from the two fp64 oracles oracle.sim (the prior draw f~ on the merged grid, sigma2 = 0) and oracle.predict (the correction), with
what the host and the three streaming kernels add written out in the plainest way: the merged grid and its index maps (merged_grid), the
gather of the normals, the residual series, the combination.  Zero-mean: the caller subtracts mu from y and adds it to the result, as the
prediction kernels do.

`mistake` seeds one wrong turn each, for tests/test_rand_posterior_host.py to catch:
    "no_eta"          the noise eta left out of the residual series
    "nu_forgotten"    eta = sqrt(sigma2) eps: nu forgotten
    "noisy_at_data"   a tau on a data time gets the noisy value f~ + eta instead of the latent one
    "no_merge"        equal times not merged: every occurrence its own grid point and normal
    "qnew_sorted"     q_new indexed in the sorted order of tau instead of the caller's
"""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from oracle import oracle as O  # noqa: E402

MISTAKES = ("no_eta", "nu_forgotten", "noisy_at_data", "no_merge", "qnew_sorted")


def merged_grid(t, tau, merge=True):
    """T = sort(unique(t | tau)) (times merged only where they compare equal) and the maps
        origin [P]  index into (t | tau) of the first occurrence of T[p] (data times come before new times)
        it [N]      merged index of t[n]
        itau [M]    merged index of tau[m]"""
    t, tau = np.asarray(t, dtype=np.float64), np.asarray(tau, dtype=np.float64)
    both = np.concatenate([t, tau])
    order = np.argsort(both, kind="stable")
    T, origin, where = [], [], np.empty(len(both), dtype=np.int64)
    for i in order:
        if not merge or not T or both[i] != T[-1]:
            T.append(both[i])
            origin.append(i)
        where[i] = len(T) - 1
    return np.array(T), np.array(origin, dtype=np.int64), where[:len(t)], where[len(t):]


def gather(origin, N, q_data, q_new):
    """qT[p] = origin[p] < N ? q_data[origin[p]] : q_new[origin[p] - N]"""
    return np.array([q_data[o] if o < N else q_new[o - N] for o in origin])


def transformed(y, s2, shift):
    """the series a draw conditions on: (y, sigma2), or with a shift c (log(y - c), sigma2 / (y - c)^2)"""
    if shift is None:
        return np.asarray(y, dtype=np.float64), np.asarray(s2, dtype=np.float64)
    v = np.asarray(y, dtype=np.float64) - shift
    return np.log(v), np.asarray(s2, dtype=np.float64) / (v * v)


def predict_any_order(a, b, c, d, tau, t, y, s2):
    """oracle.predict wants tau ascending: sort, evaluate, undo"""
    o = np.argsort(tau, kind="stable")
    out = np.empty(len(tau))
    out[o] = O.predict(a, b, c, d, tau[o], t, y, s2)
    return out


def rand_posterior(a, b, c, d, t, y, s2, tau, q_data, q_new, eps, nu=1.0, shift=None, mistake=None, sim=None, predict=None):
    """One draw at the times tau (any order) of the zero-mean GP conditioned on y (mu already subtracted, or with `shift` the raw flux: then
    y -> log(y - shift), sigma2 -> sigma2 / (y - shift)^2 first).  q_data [N], q_new [M], eps [N]: standard normals.  sim / predict: the
    two compositions' ingredients (default oracle.sim, oracle.predict)."""
    assert mistake is None or mistake in MISTAKES, mistake
    sim = sim or O.sim
    predict = predict or predict_any_order
    t, tau = np.asarray(t, dtype=np.float64), np.asarray(tau, dtype=np.float64)
    N = len(t)
    T, origin, it, itau = merged_grid(t, tau, merge=mistake != "no_merge")
    if mistake == "qnew_sorted":
        rank = np.empty(len(tau), dtype=np.int64)
        rank[np.argsort(tau, kind="stable")] = np.arange(len(tau))
        origin = np.array([o if o < N else N + rank[o - N] for o in origin])
    qT = gather(origin, N, q_data, q_new)
    f = sim(a, b, c, d, T, np.zeros(len(T)), qT)
    yk, sk = transformed(y, s2, shift)
    eta = np.sqrt((1.0 if mistake == "nu_forgotten" else nu) * sk) * eps
    resid = yk - f[it] - (0.0 if mistake == "no_eta" else eta)
    out = predict(a, b, c, d, tau, t, resid, nu * sk) + f[itau]
    if mistake == "noisy_at_data":
        at = np.searchsorted(t, tau)
        at = np.where(at < N, at, 0)
        on = t[at] == tau
        out = out + np.where(on, eta[at], 0.0)
    return out
