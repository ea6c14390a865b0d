#!/usr/bin/env python3
"""numpy prototype of the dense solver's arithmetic (csrc/dense.hip and the dense entries of capi.hip), written for the tests of
tests/dense_cases.py: what the checkers there must accept, and — one switch per seeded mistake — what they must refuse
(tests/test_dense_host.py).  fp64 throughout; it restates the structure of the kernels, not their instruction order.

  * one column-major-style slab: the lower triangle of K padded to Mp = N rounded up to 64 with identity rows / columns, the y row
    (y - mu, zero in the padding) below it; factorising the augmented matrix leaves z' = (L^-1 y)' in that row;
  * 64-wide block columns; the diagonal block is factored in 16 x 16 sub-blocks whose inverses are formed explicitly (a pivot p enters as
    r = 1 / sqrt(p): L_jj = p r, the column times r), and every row below a sub-block — the rest of the diagonal block and the whole panel
    — is solved by multiplying with that inverse; then the trailing update A22 -= P P' by 64 x 64 tiles of the lower triangle;
  * info: 1 + the row of the first pivot that is not positive, as LAPACK's; the value is then NaN;
  * prediction (dense_predict_impl): times [t | NaN x (Mp - N) | tau | NaN x (Mq - M)], a NaN time an identity row / column; the
    factorisation stops after the Mp data columns, the Schur complement left in the lower triangle of the tau block is the posterior
    covariance (mirrored into the upper one), the mean the product of the tau rows of the panel with the y row.

MISTAKES  skip_tile     the last diagonal tile misses the update by the first panel
          rsqrt_fp32    r = 1 / sqrt(p) in fp32, no Newton step
          pad_as_data   the padding of the data block built as data (the last time stamp again, sigma2 = 1) and counted in the sums
          y_before_mu   the y row holds y, not y - mu
          mirror_upper  the covariance's lower triangle filled from the (never built) upper one
          info_minus_1  info = the 0-based row of the bad pivot"""
import numpy as np

NB, SB = 64, 16
MISTAKES = ("skip_tile", "rsqrt_fp32", "pad_as_data", "y_before_mu", "mirror_upper", "info_minus_1")


def _kern(a, b, c, d, dt):
    dt = np.abs(dt)[..., None]
    return (np.exp(-c * dt) * (a * np.cos(d * dt) + b * np.sin(d * dt))).sum(-1)


def build(a, b, c, d, te, s2e):
    """lower triangle of the covariance at the times te (NaN: identity row / column) plus diag(s2e)"""
    pad = np.isnan(te)
    tt = np.where(pad, 0.0, te)
    K = _kern(a, b, c, d, tt[:, None] - tt[None, :]) + np.diag(s2e)
    K[pad, :] = 0.0; K[:, pad] = 0.0
    K[pad, pad] = 1.0
    return np.tril(K)


def _inv16(L):
    """explicit inverse of a lower-triangular 16 x 16 block, row by row"""
    W = np.zeros_like(L)
    for n in range(len(L)):
        W[n, :n] = -(L[n, :n] @ W[:n, :n]) / L[n, n]
        W[n, n] = 1.0 / L[n, n]
    return W


def _solve16(L, B):
    """B L^-T by forward substitution, column by column (no inverse formed)"""
    X = np.zeros_like(B)
    for n in range(len(L)):
        X[:, n] = (B[:, n] - X[:, :n] @ L[n, :n]) / L[n, n]
    return X


def factor(A, ncols, mistake=None, explicit_inverse=True):
    """In place: the first `ncols` (a multiple of 64) columns of the square part of A (rows >= its width: the y row) become L, the rest
    the Schur complement (lower triangle).  Returns info.  explicit_inverse=False solves the rows below a sub-block by substitution instead."""
    C = A.shape[1]
    for kb in range(0, ncols, NB):
        for j0 in range(kb, kb + NB, SB):
            blk = A[j0:j0 + SB, j0:j0 + SB]
            for j in range(SB):
                p = blk[j, j] - blk[j, :j] @ blk[j, :j]
                if not p > 0:
                    return j0 + j + 1
                r = float(np.float32(1) / np.sqrt(np.float32(p))) if mistake == "rsqrt_fp32" else 1.0 / np.sqrt(p)
                blk[j, j] = p * r
                blk[j + 1:, j] = (blk[j + 1:, j] - blk[j + 1:, :j] @ blk[j, :j]) * r
            if explicit_inverse:                         # the rest of the diagonal block and the panel: times the explicit inverse
                X = A[j0 + SB:, j0:j0 + SB] @ _inv16(np.tril(blk)).T
            else:                                        # (the same elimination order by substitution: a yardstick for what the inverses cost)
                X = _solve16(np.tril(blk), A[j0 + SB:, j0:j0 + SB])
            A[j0 + SB:, j0:j0 + SB] = X
            for c0 in range(j0 + SB, kb + NB, SB):       # the later sub-blocks of this block column
                A[c0:, c0:c0 + SB] -= X[c0 - j0 - SB:] @ X[c0 - j0 - SB:c0 - j0].T
        P = A[kb + NB:, kb:kb + NB]
        for tj in range(kb + NB, C, NB):                 # trailing update, tile columns of the lower triangle
            if mistake == "skip_tile" and kb == 0 and tj == C - NB:
                continue
            A[tj:, tj:tj + NB] -= P[tj - kb - NB:] @ P[tj - kb - NB:tj - kb].T
    return 0


def nll(a, b, c, d, t, y, s2, mu=0.0, nu=1.0, mistake=None, explicit_inverse=True):
    """(value, info) of pioran_dense_nll / one draw of pioran_dense_nll_batch"""
    a, b, c, d, t, y, s2 = (np.asarray(v, dtype=np.float64).reshape(-1) for v in (a, b, c, d, t, y, s2))
    N = len(t)
    Mp = (N + NB - 1) // NB * NB
    te = np.full(Mp, np.nan); te[:N] = t
    s2e = np.zeros(Mp); s2e[:N] = nu * s2
    ye = np.zeros(Mp); ye[:N] = y if mistake == "y_before_mu" else y - mu
    nsum = N
    if mistake == "pad_as_data":
        te[N:] = t[-1]; s2e[N:] = 1.0; nsum = Mp
    A = np.vstack([build(a, b, c, d, te, s2e), ye[None, :]])
    info = factor(A, Mp, mistake, explicit_inverse)
    if info != 0:
        return np.nan, info - (mistake == "info_minus_1")
    z = A[Mp, :nsum]
    return float(np.log(np.diag(A[:Mp])[:nsum]).sum() + 0.5 * (z @ z) + 0.5 * N * np.log(2 * np.pi)), 0


def predict(a, b, c, d, tau, t, y, s2, mistake=None):
    """(mean (M,), cov (M, M), info) of pioran_dense_predict with the covariance; y None: mean None (pioran_dense_predict_cov)"""
    a, b, c, d, tau, t, s2 = (np.asarray(v, dtype=np.float64).reshape(-1) for v in (a, b, c, d, tau, t, s2))
    N, M = len(t), len(tau)
    Mp, Mq = (N + NB - 1) // NB * NB, (M + NB - 1) // NB * NB
    Mtot = Mp + Mq
    te = np.full(Mtot, np.nan); te[:N] = t; te[Mp:Mp + M] = tau
    s2e = np.zeros(Mtot); s2e[:N] = s2
    ye = np.zeros(Mtot)
    if y is not None:
        ye[:N] = np.asarray(y, dtype=np.float64).reshape(-1)
    if mistake == "pad_as_data":
        te[N:Mp] = t[-1]; s2e[N:Mp] = 1.0
    A = np.vstack([build(a, b, c, d, te, s2e), ye[None, :]])
    info = factor(A, Mp, mistake)
    if info != 0:
        return (None if y is None else np.full(M, np.nan)), np.full((M, M), np.nan), info - (mistake == "info_minus_1")
    S = A[Mp:Mp + M, Mp:Mp + M]
    cov = np.triu(S) + np.triu(S, 1).T if mistake == "mirror_upper" else np.tril(S) + np.tril(S, -1).T
    mean = None if y is None else A[Mp:Mp + M, :Mp] @ A[Mtot, :Mp]
    return mean, cov, info
