#!/usr/bin/env python3
"""d log L / d d_j in the FORM of the step-by-step reverse mode (celerite_adjoint_kernel / celerite_adjoint2_kernel, celerite_wide.hip), restated
densely in numpy: what that form costs in accuracy, apart from any kernel.

The recurrence carries the phases as rows v_n = (cos, sin)(d_j t_n), u_n = (a cos + b sin, a sin - b cos)(d_j t_n) of ABSOLUTE times, and the
reverse pass adds, per row and step, t_n x (adjoint of the row's v and u entries x their derivative by the phase) to one accumulator per row
(do_step: sh_acc[2]); grad_finish_kernel adds the rows of a term.  With K_mn = sum_j E_mn (u_cos(m) v_cos(n) + u_sin(m) v_sin(n)) for m > n,
E_mn = exp(-c_j (t_m - t_n)) and G = dlogL/dK, the adjoints are sums over the other index, and the form is
    P_n  = sum_{m>n} 2 G_mn E_mn u_cos(m)      P'_n = sum_{m<n} 2 G_mn E_mn v_cos(m)          (Q, Q' likewise with the sin rows)
    cos row:  C = sum_n t_n (-sin(th_n) P_n + (-a sin(th_n) + b cos(th_n)) P'_n)
    sin row:  S = sum_n t_n ( cos(th_n) Q_n + ( a cos(th_n) + b sin(th_n)) Q'_n)                th_n = d_j t_n
    d log L / d d_j = C + S.
Every per-step term is a product of trigonometric values of absolute phases; only in the sum over rows and steps do they combine to the
(t_m - t_n) sin / cos(d_j (t_m - t_n)) of the dense formula (oracle.logl_grad_truth), so the two accumulators are larger than their sum by a
factor of the order of (series span) / (correlation time): roundings of the terms are amplified by it.  The windowed kernels (celerite_block.hip,
celerite_tile.hip) take differences within a window first and do not pay this.

wide_dd(a, b, c, d, t, y, s2, dtype)   the form in `dtype` (np.float64: what an fp64 evaluation of this form gives; np.longdouble: it is the
                                       dense formula to rounding), G from a dense solve in the same dtype.
usage: python tools/wide_adjoint_dd_proto.py      prints, on a few cases of tests/grad_cases.py, the form's fp64 and long-double deviations from the
truth beside the fp64 references' (ref_dev)."""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from oracle import oracle as O  # noqa: E402


def _G(a, b, c, d, t, y, s2, dtype):
    D = np.abs(t[:, None] - t[None, :])
    if dtype is np.float64:
        K = (np.exp(-c * D[..., None]) * (a * np.cos(d * D[..., None]) + b * np.sin(d * D[..., None]))).sum(-1) + np.diag(s2)
        L = np.linalg.cholesky(K)
        W = np.linalg.solve(L, np.eye(len(t)))
    else:
        L = O._truth_cholesky(a, b, c, d, t, s2, dtype)
        W = np.zeros_like(L)
        for n in range(len(t)):
            W[n, :n] = -(L[n, :n] @ W[:n, :n]) / L[n, n]
            W[n, n] = 1 / L[n, n]
    Kinv = W.T @ W
    z = Kinv @ y
    return (np.outer(z, z) - Kinv) / 2, D


def wide_dd(a, b, c, d, t, y, s2, dtype=np.float64):
    """(d log L / d d_j [J], the cos rows' and the sin rows' accumulators [2][J]) in the step-by-step form, steps taken last to first"""
    a, b, c, d, t, y, s2 = O._truth_inputs(dtype, a, b, c, d, t, y, s2)
    G, D = _G(a, b, c, d, t, y, s2, dtype)
    N, J = len(t), len(a)
    upper = np.triu(np.ones((N, N), dtype=dtype), 1)            # [n][m]: m > n
    acc = np.zeros((2, J), dtype=dtype)
    for j in range(J):
        co, si = np.cos(d[j] * t), np.sin(d[j] * t)
        GE = 2 * G * np.exp(-c[j] * D)
        ucos, usin = a[j] * co + b[j] * si, a[j] * si - b[j] * co
        P, Q = (GE * upper) @ ucos, (GE * upper) @ usin
        P_, Q_ = (GE * upper.T) @ co, (GE * upper.T) @ si
        cterm = t * (-si * P + (-a[j] * si + b[j] * co) * P_)
        sterm = t * (co * Q + (a[j] * co + b[j] * si) * Q_)
        for n in range(N - 1, -1, -1):
            acc[0, j] += cterm[n]
            acc[1, j] += sterm[n]
        if d[j] == 0:
            acc[:, j] = 0                                       # (a one-row term has no phase: the kernels add nothing for it)
    return acc[0] + acc[1], acc


if __name__ == "__main__":
    sys.path.insert(0, str(ROOT / "tests"))
    import grad_cases as GC
    cases = {c[0]: c for c in GC.edge_cases()}
    for label in sys.argv[1:] or ("R3-N48-s2x1e-6", "R3-N66-s2x1", "R3-N66-s2x1e-6", "R3-N97-s2x1", "R3-N256-s2x1e-6", "R33-N257-s2x1", "R80-N65-s2x1"):
        case = cases[label]
        truth, ref_dev, _ = GC.reference(case)
        for k in range(len(case[4])):
            yc, sk, S, v = GC._series(case, k)
            scale = float(np.max(np.abs(truth[k]["grad_d"])))
            f64, rows = wide_dd(case[4][k], case[5][k], case[6], case[7], case[1], yc, sk, np.float64)
            fld, _ = wide_dd(case[4][k], case[5][k], case[6], case[7], case[1], yc, sk, np.longdouble)
            print(f"{label} draw {k}: ref_dev {ref_dev['grad_d'][k]:.2e}   form in fp64 {float(np.max(np.abs(f64 - truth[k]['grad_d']))) / scale:.2e}   "
                  f"in long double {float(np.max(np.abs(fld - truth[k]['grad_d']))) / scale:.2e}   rows / sum {float(np.max(np.abs(rows))) / scale:.1e}")
