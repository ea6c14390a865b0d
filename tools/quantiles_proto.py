"""numpy restatement of the column quantiles and means over the draw axis that pioran.jl_amd/csrc/quantiles.hip evaluates — the twin the
tests hold the device against, and the project's definition of the quantile.

Value of draw b in output column m, formed in this order (each operation rounded on its own):
    v = X[b][cols[m]]                      (cols absent: column m)
    v = exp(v + shift[b])                  (shift given: the back-transform of the log-flux models, src/plots_diagnostics.jl:663)
    v = (ref[m] - v) / scale[m]            (ref, scale given: the standardised residual, :812)
Rows with status != 0 are left out of every column.  For the K kept values of a column sorted ascending, v[1..K] (Statistics.quantile with
its defaults, type 7, alpha = beta = 1):
    aleph = K p + (1 - p),  j = clamp(trunc(aleph), 1, K - 1),  gamma = clamp(aleph - j, 0, 1)       clamp(x, lo, hi): hi if x > hi, lo if x < lo
    a = v[j], b = v[j + 1]  (K = 1: a = b = v[1])
    q = a + gamma (b - a) if a and b are finite and a ~ b, else (1 - gamma) a + gamma b
    a ~ b: |a - b| <= 2^-26 max(|a|, |b|)  (isapprox with its default tolerance sqrt(eps))
in fp64, every operation rounded on its own (numpy has no fused multiply-add; aleph is a product, a difference and a sum).  The condition
a ~ b is this project's definition, made for one reason: the project requires the minimum at p = 0 and the maximum at p = 1 exactly, and
a + gamma (b - a) for every finite pair misses the maximum (a + 1 (b - a) != b once b - a rounds: 917 of 9800 seeded columns).  Between two
close values the first form is monotone in gamma and exact at both ends (their difference is exact); everywhere else the second form gives a and
b exactly at gamma = 0 and 1.  Whether Statistics.jl makes the same distinction, or forms aleph with a fused multiply-add, could not be checked:
its source is not available to this project.  A NaN among the kept values of a column gives NaN in all its
quantiles; K = 0 gives NaN everywhere.  The mean is the long-double sum of the kept values over K, rounded to fp64.
"""
from __future__ import annotations

import numpy as np

RTOL = np.float64(2.0 ** -26)                     # sqrt(eps): isapprox's default relative tolerance
DEFAULT_PROBS = (0.025, 0.16, 0.5, 0.84, 0.975)   # the five of src/plots_diagnostics.jl:805-816


def load(X, status=None, shift=None, cols=None, ref=None, scale=None):
    """the [K][Mc] values the reduction sees: gather, back-transform, residual; kept rows only"""
    X = np.asarray(X, dtype=np.float64)
    V = X if cols is None else X[:, np.asarray(cols, dtype=np.int64)]
    if shift is not None:
        with np.errstate(over="ignore", invalid="ignore"):
            V = np.exp(V + np.asarray(shift, dtype=np.float64)[:, None])
    if ref is not None:
        with np.errstate(invalid="ignore", over="ignore"):
            V = (np.asarray(ref, dtype=np.float64)[None, :] - V) / np.asarray(scale, dtype=np.float64)[None, :]
    if status is not None:
        V = V[np.asarray(status) == 0]
    return np.ascontiguousarray(V)


def position(K, p):
    """(j, gamma) of the Julia form for K values and probability p"""
    p = np.float64(p)
    aleph = np.float64(K) * p + (np.float64(1.0) - p)
    j = int(np.trunc(aleph))
    j = K - 1 if j > K - 1 else (1 if j < 1 else j)
    g = aleph - np.float64(j)
    g = np.float64(1.0) if g > 1.0 else (np.float64(0.0) if g < 0.0 else g)
    return j, g


def quantile_sorted(S, p):
    """the quantile of ascending values without NaN along axis 0 of S (K,) or (K, Mc), the Julia form"""
    S = np.asarray(S, dtype=np.float64)
    K = S.shape[0]
    j, g = position(K, p)
    a, b = (S[0], S[0]) if K == 1 else (S[j - 1], S[j])
    with np.errstate(invalid="ignore", over="ignore"):
        close = np.isfinite(a) & np.isfinite(b) & (np.abs(a - b) <= RTOL * np.maximum(np.abs(a), np.abs(b)))
        return np.where(close, a + g * (b - a), (np.float64(1.0) - g) * a + g * b)[()]


def quantiles(X, probs=DEFAULT_PROBS, status=None, shift=None, cols=None, ref=None, scale=None):
    """(quant [Q][Mc], mean [Mc], kept) of the draws in the rows of X"""
    V = load(X, status, shift, cols, ref, scale)
    K, Mc = V.shape
    probs = np.asarray(probs, dtype=np.float64).reshape(-1)
    quant = np.full((len(probs), Mc), np.nan)
    if K == 0:
        return quant, np.full(Mc, np.nan), 0
    S = np.sort(V, axis=0)                      # NaN last
    with np.errstate(invalid="ignore", over="ignore"):
        mean = (np.sum(V.astype(np.longdouble), axis=0) / np.longdouble(K)).astype(np.float64)
    has_nan = np.isnan(S[-1])
    for q, p in enumerate(probs):
        quant[q] = np.where(has_nan, np.nan, quantile_sorted(S, p))
    return quant, mean, K


def mean_longdouble(X, **kw):
    """the long-double mean and the mean of |v| per column (the bound of the device's mean is K eps mean|v|)"""
    V = load(X, **kw).astype(np.longdouble)
    K, Mc = V.shape
    if K == 0:
        return np.full(Mc, np.nan, dtype=np.longdouble), np.full(Mc, np.nan, dtype=np.longdouble)
    with np.errstate(invalid="ignore"):
        return np.sum(V, axis=0) / np.longdouble(K), np.sum(np.abs(V), axis=0) / np.longdouble(K)
