"""Posterior variance of a celerite GP at new times in O((N + M) R^2): numpy prototype of the recurrences behind
pioran_celerite_predict_var ("Posterior variance through the factorisation"; kernels in
pioran.jl_amd/csrc/celerite_predict.hip).

    var(tau) = k(0) - k*' K^-1 k*,   K = L D L' the celerite factorisation of the data covariance (+ diag sigma2)

Rows r: a cos and a sin row per term (the sin row dropped where d_j = 0).  U~_n, V_n the pre-conditioned generators,
phi_n = exp(-c (t_n - t_{n-1})), (D_n, W_n) the factor.  Forward S+_n = S_n + D_n W_n W_n', S_{n+1} = phi phi' o S+_n;
backward B_n = U~ U~'/D_n + A' B_{n+1} A, A = diag(phi_{n+1}) (I - W_n U~_n').  With n0 = #{t_n < tau},
alpha = e^{-c (tau - t_{n0-1})} U~(tau), beta = e^{-c (t_{n0} - tau)} V(tau):

    g = S+_{n0-1} alpha,  q1 = alpha'g;   e = beta - phi_{n0} o g,  q2 = e' B_{n0} e;   var = k(0) - q1 - q2.

Importable: predict_var(a, b, c, d, t, sigma2, tau) -> (M,) (tests/test_predict_var_host.py holds it against the dense oracle).

`mistake` seeds one of the slips a kernel of these recurrences can make (MISTAKES); tests/test_predict_var_host.py uses them to show that the
case list of tests/predict_var_cases.py catches each of them.
"""
from __future__ import annotations

import numpy as np


def _rows(a, b, c, d):
    """Row tables: (al, be, c_r, d_r, sin_row) with U~_r(t) = al v + be x, (v, x) = (cos, sin) or (sin, cos)(d t)."""
    al, be, cr, dr, ks = [], [], [], [], []
    for j in range(len(a)):
        al.append(a[j]); be.append(b[j]); cr.append(c[j]); dr.append(d[j]); ks.append(False)
        if d[j] != 0.0:
            al.append(a[j]); be.append(-b[j]); cr.append(c[j]); dr.append(d[j]); ks.append(True)
    return tuple(np.array(v) for v in (al, be, cr, dr, ks))


def _uv(al, be, dr, ks, x):
    co, si = np.cos(dr * x), np.sin(dr * x)
    v = np.where(ks, si, co)
    return al * v + be * np.where(ks, co, si), v


MISTAKES = {
    "mask_last_row": "row R - 1 left out of the two quadratic forms (a lane mask off by one)",
    "reuse_alpha": "the second and later evaluation times of a step use the first one's alpha",
    "phi_of_step": "e = beta - phi_{n0-1} o g: the phi of the step itself, not of the gap the evaluation time lies in",
    "n0_le_forward": "the forward pass counts t_n <= tau, the backward pass t_n < tau",
}


def predict_var(a, b, c, d, t, sigma2, tau, mistake=None):
    assert mistake is None or mistake in MISTAKES, mistake
    a, b, c, d, t, sigma2, tau = (np.asarray(v, dtype=np.float64).reshape(-1) for v in (a, b, c, d, t, sigma2, tau))
    N, M = len(t), len(tau)
    al, be, cr, dr, ks = _rows(a, b, c, d)
    R = len(al)
    k0 = a.sum()
    order = np.argsort(tau, kind="stable")
    ts = tau[order]
    n0 = np.searchsorted(t, ts, side="left")          # number of t_n < tau
    n0f = np.searchsorted(t, ts, side="right") if mistake == "n0_le_forward" else n0
    keep = np.ones(R)
    if mistake == "mask_last_row":
        keep[R - 1] = 0.0
    U = np.empty((N, R)); V = np.empty((N, R)); phi = np.zeros((N + 1, R))
    for n in range(N):
        U[n], V[n] = _uv(al, be, dr, ks, t[n])
        if n > 0:
            phi[n] = np.exp(-cr * (t[n] - t[n - 1]))
    # factor + forward pass
    W = np.empty((N, R)); D = np.empty(N)
    q1 = np.zeros(M); E = np.zeros((M, R))
    Sp = np.zeros((R, R))                              # S+_{n-1}
    mp = 0
    while mp < M and n0f[mp] == 0:                     # before the first data point: g = 0, e = beta
        _, vt = _uv(al, be, dr, ks, ts[mp])
        E[mp] = keep * np.exp(-cr * (t[0] - ts[mp])) * vt
        mp += 1
    for n in range(N):
        S = np.outer(phi[n], phi[n]) * Sp
        Su = S @ U[n]
        D[n] = k0 + sigma2[n] - U[n] @ Su
        W[n] = (V[n] - Su) / D[n]
        Sp = S + D[n] * np.outer(W[n], W[n])
        first = None
        while mp < M and n0f[mp] == n + 1:
            ut, vt = _uv(al, be, dr, ks, ts[mp])
            alpha = keep * np.exp(-cr * (ts[mp] - t[n])) * ut
            if mistake == "reuse_alpha":
                first = alpha if first is None else first
                alpha = first
            g = Sp @ alpha
            q1[mp] = alpha @ g
            if n + 1 < N:
                E[mp] = keep * (np.exp(-cr * (t[n + 1] - ts[mp])) * vt - phi[n if mistake == "phi_of_step" else n + 1] * g)
            mp += 1
    # backward pass
    out = np.empty(M)
    mq = M - 1
    while mq >= 0 and n0[mq] == N:
        out[mq] = k0 - q1[mq]
        mq -= 1
    Bm = np.zeros((R, R))
    for n in range(N - 1, -1, -1):
        Bp = np.outer(phi[n + 1], phi[n + 1]) * Bm
        h = Bp @ W[n]
        Bm = Bp - np.outer(U[n], h) - np.outer(h, U[n]) + (1.0 / D[n] + W[n] @ h) * np.outer(U[n], U[n])
        while mq >= 0 and n0[mq] == n:
            out[mq] = k0 - q1[mq] - E[mq] @ Bm @ E[mq]
            mq -= 1
    res = np.empty(M)
    res[order] = out
    return res


if __name__ == "__main__":
    import sys
    from pathlib import Path
    sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
    from oracle import oracle
    t, y, yerr = oracle.synthetic_series(400)
    A, Bc, C, Dd, mu, nu = oracle.theta_to_coefs(oracle.synthetic_theta(3, t, y), t)
    rng = np.random.default_rng(0)
    tau = np.concatenate([rng.uniform(t[0] - 5, t[-1] + 5, 150), t[::40]])
    for bb in range(3):
        ref = np.diag(oracle.predict_cov_numpy(A[bb], Bc[bb], C, Dd, tau, t, yerr ** 2))
        got = predict_var(A[bb], Bc[bb], C, Dd, t, yerr ** 2, tau)
        print(f"draw {bb}: max |delta| / k(0) = {np.abs(got - ref).max() / A[bb].sum():.2e}, min var / k(0) = {ref.min() / A[bb].sum():.2e}")
