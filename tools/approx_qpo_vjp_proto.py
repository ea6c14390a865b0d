"""numpy restatement of the reverse mode of `approx` with QPO features that pioran.jl_amd/csrc/approx.hip (approx_qpo_vjp_kernel) evaluates,
operation by operation — the twin the CPU tests hold against the 50-digit truth.  The grid, the weights and the power laws' logarithmic derivatives
are tools/approx_vjp_proto.py's.

Forward (approx_kernel; src/psd.jl:214-289), per draw, with p0 = P(f_0; theta), p_j = P(f_j) / p0, x = B^-1 p, and per feature (S0, f0, Q):
    w0 = 2 pi f0,  De = sqrt(4 Q^2 - 1),  al = S0 w0 Q / 4             convert_feature
    fa = al / p0,  fb = fa / De,  c = w0 / (2 Q),  d = c De
    I = w'x + [integrated] sum_q (fa_q Ia_q + fb_q Ib_q)                Ia, Ib: the brackets of integral_celerite between f_min and f_max
    a_j = kappa_j x_j norm / I (b_j as in approx_vjp_proto),  A_q = 2 fa_q norm / I,  B_q = 2 fb_q norm / I,  C_q = c_q,  D_q = d_q
Reverse, from ga, gb, gc, gd [B][Jt] (the feature columns are the last n_qpo; of gc, gd only they are read), with h as in approx_vjp_proto:
    s = norm / I,  T = h'x + sum_q 2 (ga_q fa_q + gb_q fb_q),  grad_norm = T / I,  Ibar = -s T / I
    xbar = s h + Ibar w,  pbar = B^-T xbar
    fabar = 2 s ga_q + [i] Ibar Ia,  fbbar = 2 s gb_q + [i] Ibar Ib
    cbar = gc_q + [i] Ibar (fa dIa/dc + fb dIb/dc),  dbar = gd_q + [i] Ibar (fa dIa/dd + fb dIb/dd)      dIb/dc = dIa/dd, dIb/dd = -dIa/dc
    fabar += fbbar / De,  Debar = dbar c - fbbar fb / De,  cbar += dbar De,  albar = fabar / p0
    grad_S0 = albar w0 Q / 4,  grad_f0 = 2 pi (albar S0 Q / 4 + cbar / (2 Q)),  grad_Q = albar S0 w0 / 4 - cbar c / Q + Debar 4 Q / De
    grad_theta_k = sum_j pbar_j p_j (dlog P(f_j)/dtheta_k - dlog P(f_0)/dtheta_k) - (sum_q fabar_q fa_q) dlog P(f_0)/dtheta_k

`mistake` seeds one error per reverse step, so that the tests can show that their bar catches each:
    "no_feature_T"     the features' terms of T dropped (grad_norm and Ibar from the continuum alone)
    "no_w"             the w term of xbar dropped
    "no_transpose"     B^-1 xbar instead of B^-T xbar
    "no_integral"      Ibar Ia, Ibar Ib dropped from fabar, fbbar (the features taken out of the normalisation)
    "no_integral_cd"   the integral's terms dropped from cbar, dbar
    "cr_sign"          dIb/dd = +dIa/dc (the sign of the Cauchy-Riemann pair)
    "no_fb_chain"      fabar += fbbar / De dropped
    "no_delta"         Debar dropped from grad_Q
    "no_d_chain"       cbar += dbar De dropped
    "no_p0"            the features' 1 / p0 dropped from grad_theta
    "no_f0"            dlog P(f_0) not subtracted in the continuum's sum
    "no_c_f0"          cbar / (2 Q) dropped from grad_f0
"""
from __future__ import annotations

import math

import numpy as np

from approx_vjp_proto import dlog_psd, grid, interchanges, weights  # noqa: F401  (interchanges: for the tests' case list)

MISTAKES = ("no_feature_T", "no_w", "no_transpose", "no_integral", "no_integral_cd", "cr_sign", "no_fb_chain", "no_delta", "no_d_chain", "no_p0",
            "no_f0", "no_c_f0")


def brackets(c, d, f):
    """(ia, ib, d ia / dc, d ia / dd) of integral_celerite at the frequency f per unit (a, b)"""
    up, um = d + 2 * math.pi * f, d - 2 * math.pi * f
    num, den = c * c + up * up, c * c + um * um
    return ((np.arctan2(c, um) - np.arctan2(c, up)) / math.pi, np.log(num / den) / (2 * math.pi), (um / den - up / num) / math.pi,
            c * (1 / num - 1 / den) / math.pi)


def approx_qpo_vjp(model, theta, norm, qpo, grad_a, grad_b, grad_c, grad_d, f_min, f_max, n_components=20, S_low=20.0, S_high=20.0, *,
                   is_integrated_power=True, basis=0, mistake=None):
    """(grad_theta [B][P], grad_norm [B], grad_qpo [B][n_qpo][3]) from grad_a .. grad_d [B][Jt], Jt = n_components (2 n_components for basis 1) + n_qpo"""
    if mistake is not None and mistake not in MISTAKES:
        raise ValueError(mistake)
    theta = np.atleast_2d(np.asarray(theta, float))
    B = theta.shape[0]
    J = n_components
    Jc = J * (1 + basis)
    norm = np.broadcast_to(np.asarray(norm, float), (B,))
    qpo = np.asarray(qpo, float).reshape(B, -1, 3)
    ga, gb, gc, gd = (np.asarray(v, float) for v in (grad_a, grad_b, grad_c, grad_d))
    sp, Bm = grid(J, basis, f_min, f_max, S_low, S_high)
    w = weights(sp, basis, is_integrated_power, f_min, f_max)
    P, dl = dlog_psd(model, theta, sp)                 # [B][J], [B][J][P]
    p0 = P[:, :1]
    p = P / p0
    x = np.linalg.solve(Bm, p.T).T                     # [B][J]
    if basis == 0:
        h = sp * math.pi / math.sqrt(2) * (ga[:, :J] + gb[:, :J])
    else:
        h = sp * math.pi / 3 * (ga[:, :J] + ga[:, J:Jc] + math.sqrt(3) * gb[:, :J])
    S0, f0, Q = qpo[:, :, 0], qpo[:, :, 1], qpo[:, :, 2]           # [B][n_qpo]
    De, w0 = np.sqrt(4 * Q * Q - 1), 2 * math.pi * f0
    fa = S0 * w0 * Q / 4 / p0
    fb, fc = fa / De, w0 / Q / 2
    fd = fc * De
    gaq, gbq, gcq, gdq = ga[:, Jc:], gb[:, Jc:], gc[:, Jc:], gd[:, Jc:]
    I = x @ w
    T = np.sum(h * x, axis=1)
    if mistake != "no_feature_T":
        T = T + 2 * np.sum(gaq * fa + gbq * fb, axis=1)
    if is_integrated_power:
        hi, lo = brackets(fc, fd, f_max), brackets(fc, fd, f_min)
        ia, ib, ia_c, ia_d = (u - v for u, v in zip(hi, lo))
        I = I + np.sum(fa * ia + fb * ib, axis=1)
    s = norm / I
    Ibar = -s * T / I
    xbar = s[:, None] * h
    if mistake != "no_w":
        xbar = xbar + Ibar[:, None] * w[None, :]
    fab, fbb, cb, db = 2 * s[:, None] * gaq, 2 * s[:, None] * gbq, gcq.copy(), gdq.copy()
    if is_integrated_power:
        ib_d = ia_c if mistake == "cr_sign" else -ia_c
        if mistake != "no_integral":
            fab, fbb = fab + Ibar[:, None] * ia, fbb + Ibar[:, None] * ib
        if mistake != "no_integral_cd":
            cb, db = cb + Ibar[:, None] * (fa * ia_c + fb * ia_d), db + Ibar[:, None] * (fa * ia_d + fb * ib_d)
    if mistake != "no_fb_chain":
        fab = fab + fbb / De
    Deb = db * fc - fbb * fb / De
    if mistake == "no_delta":
        Deb = 0 * Deb
    if mistake != "no_d_chain":
        cb = cb + db * De
    fsum = np.sum(fab * fa, axis=1)
    alb = fab / p0
    gq = np.stack([alb * w0 * Q / 4, 2 * math.pi * (alb * S0 * Q / 4 + (0 if mistake == "no_c_f0" else cb / (2 * Q))),
                   alb * S0 * w0 / 4 - cb * fc / Q + Deb * 4 * Q / De], axis=2)
    pbar = np.linalg.solve(Bm if mistake == "no_transpose" else Bm.T, xbar.T).T
    dd = dl if mistake == "no_f0" else dl - dl[:, :1, :]
    gth = np.einsum("bj,bj,bjk->bk", pbar, p, dd)
    if mistake != "no_p0":
        gth = gth - fsum[:, None] * dl[:, 0, :]
    return gth, T / I, gq
