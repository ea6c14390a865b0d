"""numpy restatement of the reverse mode of `approx` that pioran.jl_amd/csrc/approx.hip (approx_vjp_kernel) evaluates — the twin the tests
hold the device against.

Forward (approx_kernel; src/psd.jl:214-289), per draw with parameters theta and variance `norm`, on the spectral grid f_0 .. f_{J-1}:
    p_j = P(f_j) / P(f_0)                  the normalised PSD
    x = B^-1 p                             B_jk = 1 / (1 + (f_j / f_k)^(4 | 6)), factorised once: P B = L U
    I = w' x                               w_j: the bracket of integral_sho / integral_drwcelerite between f_min and f_max per unit amplitude,
                                           or f_j pi / sqrt2 (SHO), 2 pi f_j / 3 (DRWCelerite) for the variance form
    a_j = kappa_j x_j norm / I             kappa_j = f_j pi / sqrt2, b_j = a_j (SHO);  kappa_j = f_j pi / 3, a_{J+j} = a_j, b_j = sqrt3 a_j,
                                           b_{J+j} = 0 (DRWCelerite)
Reverse, from ga = dL/da, gb = dL/db:
    h_j = kappa_j (ga_j + gb_j)            SHO
    h_j = kappa_j (ga_j + ga_{J+j} + sqrt3 gb_j)        DRWCelerite
    grad_norm = h'x / I
    xbar = (norm / I) h - (norm / I^2) (h'x) w
    pbar = B^-T xbar                       U' y = xbar, L' z = y, pbar = P' z
    grad_theta_k = sum_j pbar_j p_j (dlog P(f_j)/dtheta_k - dlog P(f_0)/dtheta_k)
with the logarithmic derivatives of the bending power laws in closed form (dlog_psd).

`mistake` seeds one error per reverse step, so that the tests can show that their bar catches each:
    "no_w"          the w term of xbar dropped (the normalisation taken as constant)
    "no_transpose"  B^-1 xbar instead of B^-T xbar
    "no_f0"         dlog P(f_0) not subtracted (the normalisation by P(f_0) taken as constant)
    "no_sqrt3"      the sqrt3 gb term of the DRWCelerite h dropped
"""
from __future__ import annotations

import math

import numpy as np

MISTAKES = ("no_w", "no_transpose", "no_f0", "no_sqrt3")
N_PARAMS = {0: 3, 1: 5}     # model 0 SingleBendingPowerLaw(alpha1, f1, alpha2), 1 DoubleBendingPowerLaw(alpha1, f1, alpha2, f2, alpha3)


def grid(J, basis, f_min, f_max, S_low=20.0, S_high=20.0):
    """(sp [J], B [J][J]) of build_approx; basis 0 SHO, 1 DRWCelerite"""
    f0, fM = f_min / S_low, f_max * S_high
    sp = f0 * (fM / f0) ** (np.arange(J) / (J - 1))
    return sp, 1.0 / (1.0 + (sp[:, None] / sp[None, :]) ** (4 if basis == 0 else 6))


def weights(sp, basis, integrated, f_min, f_max):
    """w_j: I = w'x"""
    c = sp
    if not integrated:
        return c * math.pi / math.sqrt(2) if basis == 0 else c * 2 * math.pi / 3
    if basis == 0:
        s2 = math.sqrt(2)

        def prim(f):
            ph = (f * f + s2 * c * f + c * c) / (f * f - s2 * c * f + c * c)
            return c / (4 * s2) * (np.log(ph) + 2 * np.arctan2(c * s2 * f, c * c - f * f))
    else:
        s3 = math.sqrt(3)

        def prim(f):
            ph = (f * f + s3 * c * f + c * c) / (f * f - s3 * c * f + c * c)
            return c / 3 * (np.arctan(f / c) + 0.5 * np.arctan2(f * f - c * c, c * f) + s3 / 4 * np.log(ph))
    w = prim(f_max) - prim(f_min)
    far = c <= 0.5 * f_min          # far below the band the two primitives cancel: the series of psd_device.h psd_band_tail (16 terms)
    p = 4 if basis == 0 else 6
    th, tl = c[far] / f_min, c[far] / f_max
    thp, tlp = th ** p, tl ** p
    uh, ul, total, sign = thp / th, tlp / tl, 0.0, 1.0
    for k in range(16):
        total = total + sign * (uh - ul) / (p * (k + 1) - 1)
        uh, ul, sign = uh * thp, ul * tlp, -sign
    w[far] = c[far] * total
    return w


def dlog_psd(model, theta, f):
    """(P(f) [B][F], dlog P / dtheta_k [B][F][P]) for theta [B][P] and frequencies f [F]"""
    th = np.asarray(theta, float)
    f = np.asarray(f, float)[None, :]
    a1, f1, a2 = (th[:, i:i + 1] for i in range(3))
    with np.errstate(over="ignore", invalid="ignore"):
        x = f / f1
        lx = np.log(x)
        u = x ** (a2 - a1)
        q = np.where(np.isinf(u), 1.0, u / (1.0 + u))
        val = x ** (-a1) / (1.0 + u)
        d = [-lx * (1.0 - q), (a1 + q * (a2 - a1)) / f1, -q * lx]
        if model == 1:
            f2, a3 = th[:, 3:4], th[:, 4:5]
            ly = np.log(f / f2)
            v = (f / f2) ** (a3 - a2)
            r = np.where(np.isinf(v), 1.0, v / (1.0 + v))
            val = val / (1.0 + v)
            d[2] = d[2] + r * ly
            d += [r * (a3 - a2) / f2 + 0.0 * ly, -r * ly]
    return val, np.stack(d, axis=-1)


def lu_factor(Bm):
    """(LU, piv) with P B = L U by partial pivoting, pioran_approx_setup_host's loop"""
    LU = Bm.copy()
    J = len(LU)
    piv = np.zeros(J, dtype=np.int64)
    for k in range(J):
        p = k + int(np.argmax(np.abs(LU[k:, k])))
        piv[k] = p
        if p != k:
            LU[[k, p]] = LU[[p, k]]
        LU[k + 1:, k] /= LU[k, k]
        LU[k + 1:, k + 1:] -= np.outer(LU[k + 1:, k], LU[k, k + 1:])
    return LU, piv


def lu_solve(LU, piv, rhs):
    """B^-1 rhs for rhs [B][J] through the factors, in the kernel's order (psd_lu_solve): interchanges, unit lower, upper"""
    x = np.array(rhs, float).T.copy()
    J = len(piv)
    for j in range(J):
        if piv[j] != j:
            x[[j, piv[j]]] = x[[piv[j], j]]
    for i in range(1, J):
        x[i] = x[i] - LU[i, :i] @ x[:i]
    for i in range(J - 1, -1, -1):
        x[i] = (x[i] - LU[i, i + 1:] @ x[i + 1:]) / LU[i, i]
    return x.T


def lu_solve_transposed(LU, piv, rhs):
    """B^-T rhs for rhs [B][J] through the same factors (psd_lu_solve_transposed): U' forward, L' backward, the interchanges undone in reverse
    order.  numpy's solve on B' factorises B' anew, with other pivots: on the sparse grids its result is as good in norm but loses the small
    components that the pullback multiplies with large p_j (draws with alpha1 < 0), 8e-11 S_k at DRWCelerite J = 3 where the kernel has 1e-15."""
    x = np.array(rhs, float).T.copy()
    J = len(piv)
    for i in range(J):
        x[i] = (x[i] - LU[:i, i] @ x[:i]) / LU[i, i]
    for i in range(J - 2, -1, -1):
        x[i] = x[i] - LU[i + 1:, i] @ x[i + 1:]
    for j in range(J - 1, -1, -1):
        if piv[j] != j:
            x[[j, piv[j]]] = x[[piv[j], j]]
    return x.T


def approx_vjp(model, theta, norm, grad_a, grad_b, f_min, f_max, n_components=20, S_low=20.0, S_high=20.0, *, is_integrated_power=True,
               basis=0, mistake=None):
    """(grad_theta [B][P], grad_norm [B]) from grad_a, grad_b [B][J] (J = n_components, or 2 n_components for basis 1)"""
    if mistake is not None and mistake not in MISTAKES:
        raise ValueError(mistake)
    theta = np.atleast_2d(np.asarray(theta, float))
    B = theta.shape[0]
    J = n_components
    norm = np.broadcast_to(np.asarray(norm, float), (B,))
    ga, gb = np.asarray(grad_a, float), np.asarray(grad_b, float)
    sp, Bm = grid(J, basis, f_min, f_max, S_low, S_high)
    w = weights(sp, basis, is_integrated_power, f_min, f_max)
    P, dl = dlog_psd(model, theta, sp)                 # [B][J], [B][J][P]
    p = P / P[:, :1]
    LU, piv = lu_factor(Bm)
    x = lu_solve(LU, piv, p)                           # [B][J]
    if basis == 0:
        h = sp * math.pi / math.sqrt(2) * (ga + gb)
    else:
        gb3 = 0.0 if mistake == "no_sqrt3" else math.sqrt(3) * gb[:, :J]
        h = sp * math.pi / 3 * (ga[:, :J] + ga[:, J:] + gb3)
    I = x @ w
    hx = np.sum(h * x, axis=1)
    xbar = (norm / I)[:, None] * h
    if mistake != "no_w":
        xbar = xbar - (norm / I ** 2 * hx)[:, None] * w[None, :]
    pbar = lu_solve(LU, piv, xbar) if mistake == "no_transpose" else lu_solve_transposed(LU, piv, xbar)
    dd = dl if mistake == "no_f0" else dl - dl[:, :1, :]
    return np.einsum("bj,bj,bjk->bk", pbar, p, dd), hx / I


def interchanges(J, basis, f_min=1e-3, f_max=1.0, S_low=20.0, S_high=20.0):
    """number of rows that partial pivoting interchanges when it factorises the spectral matrix (pioran_approx_setup_host's loop)"""
    _, A = grid(J, basis, f_min, f_max, S_low, S_high)
    A = A.copy()
    n = 0
    for k in range(J):
        p = k + int(np.argmax(np.abs(A[k:, k])))
        if p != k:
            A[[k, p]] = A[[p, k]]
            n += 1
        A[k + 1:, k] /= A[k, k]
        A[k + 1:, k + 1:] -= np.outer(A[k + 1:, k], A[k, k + 1:])
    return n


if __name__ == "__main__":
    # the transposed solve's interchange code is reached by no grid the setup accepts: 0 for every J = 2 .. 256 of both bases
    for basis in (0, 1):
        bad = [J for J in range(2, 257) if interchanges(J, basis)]
        print("basis", basis, "grids with a row interchange:", bad)
