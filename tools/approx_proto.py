"""numpy restatement of the forward `approx` in the order pioran.jl_amd/csrc/approx.hip evaluates it (pioran_approx_setup_host, approx_kernel and
the device functions of psd_device.h), operation by operation — the twin the CPU tests hold against the 50-digit truth of
tools/make_approx_truth.py, and the carrier of the seeded mistakes that show what the tests' bar catches.

Host side, once per grid (setup()):
    f_j = f_0 (f_M / f_0)^(j / (J - 1)),  f_0 = f_min / S_low,  f_M = f_max S_high
    B_jk = 1 / (1 + (f_j / f_k)^(4 | 6)),  P B = L U by partial pivoting (the first largest entry of the column; rows interchanged whole)
    (c, d) of the grid: SHO c = d = sqrt2 pi f_j;  DRWCelerite c = pi f_j, d = sqrt3 c, then c = 2 pi f_j, d = 0
Per draw (approx()), vectorised over the draws, every sum in the kernel's order:
    p_j = P(f_j) / P(f_0)
    x = B^-1 p: the row interchanges j = 0 .. J - 1 in turn, then L y = P p (unit lower; row i takes its k < i ascending), then U x = y
                (rows from the last; row i takes its k > i ascending, then the division)
    I = (hi - lo) + tail, hi and lo the sums over the terms with f_j > f_min / 2 of integral_sho / integral_drwcelerite at f_max and at f_min
        (two separate sums, not per-term differences), tail the terms far below the band, whose primitives cancel, as a series in f_j / f
        (psd_band_tail); or the variance form; with is_integrated_power the features add integral_celerite(f_max) - integral_celerite(f_min) each
    features: De = sqrt(4 Q^2 - 1), w0 = 2 pi f0, fa = S0 w0 Q / 4 / P(f_0), c = w0 / Q / 2, d = c De;  (2 fa s, 2 (fa s / De), c, d), s = norm / I
    continuum: a_j = x_j s f_j pi / sqrt2 = b_j (SHO);  a_j = x_j s f_j pi / 3 twice, b_j = sqrt3 a_j, then 0 (DRWCelerite)
(The kernel's fused multiply-adds in the two triangular solves are separate multiplications and subtractions here.)

`mistake` seeds one error, so that the tests can show that their bar catches each:
    "no_interchange"         the row interchanges skipped
    "reversed_interchange"   the interchanges applied from the last to the first
    "atan2_swapped"          the arguments of atan2 swapped in integral_sho
    "no_half"                the 0.5 dropped in integral_drwcelerite
    "variance_form"          the variance form used where is_integrated_power (continuum)
    "sqrt2_for_sqrt3"        sqrt2 instead of sqrt3 in DRWCelerite's b
    "a_not_doubled"          a feature's a not doubled
    "no_p0"                  a feature not divided by P(f_0)
    "delta_plus"             Delta = sqrt(4 Q^2 + 1)
    "no_feature_integral"    the features' integral left out of I
    "grid_from_f_min"        f_0 of the grid taken as f_min (no S_low)
    "no_last_row"            the last row of the back substitution (row 0) skipped
    "no_tail_series"         the terms far below the band through the difference of their primitives, as the reference writes them
"""
from __future__ import annotations

import math

import numpy as np

MISTAKES = ("no_interchange", "reversed_interchange", "atan2_swapped", "no_half", "variance_form", "sqrt2_for_sqrt3", "a_not_doubled", "no_p0",
            "delta_plus", "no_feature_integral", "grid_from_f_min", "no_last_row", "no_tail_series")
SQRT2, SQRT3 = 1.4142135623730951, 1.7320508075688772          # the kernel's literals


def setup(J, basis, f_min, f_max, S_low=20.0, S_high=20.0, mistake=None):
    """(sp [J], LU [J][J], piv [J], c, d [Jc]) as pioran_approx_setup_host builds them"""
    f0, fM = (f_min if mistake == "grid_from_f_min" else f_min / S_low), f_max * S_high
    sp = np.array([f0 * math.pow(fM / f0, j / (J - 1)) for j in range(J)])
    LU = 1.0 / (1.0 + (sp[:, None] / sp[None, :]) ** (4.0 if basis == 0 else 6.0))
    piv = np.zeros(J, dtype=np.int32)
    for k in range(J):
        p = k + int(np.argmax(np.abs(LU[k:, k])))          # (argmax: the first of equal entries, as the host's `>` keeps it)
        piv[k] = p
        if p != k:
            LU[[k, p]] = LU[[p, k]]
        LU[k + 1:, k] /= LU[k, k]
        LU[k + 1:, k + 1:] -= np.outer(LU[k + 1:, k], LU[k, k + 1:])
    if basis == 0:
        c = math.sqrt(2.0) * math.pi * sp
        return sp, LU, piv, c, c.copy()
    c = math.pi * sp
    return sp, LU, piv, np.concatenate([c, 2.0 * c]), np.concatenate([math.sqrt(3.0) * c, np.zeros(J)])


def interchanges(J, basis, f_min=1e-3, f_max=1.0, S_low=20.0, S_high=20.0):
    """number of rows the factorisation interchanges"""
    piv = setup(J, basis, f_min, f_max, S_low, S_high)[2]
    return int(np.sum(piv != np.arange(J)))


def psd_model(model, th, f):
    """psd_device.h psd_model for theta [B][P] at one frequency: [B]"""
    with np.errstate(over="ignore"):
        x = f / th[:, 1]
        v = x ** (-th[:, 0]) / (1.0 + x ** (th[:, 2] - th[:, 0]))
        if model == 1:
            v = v / (1.0 + (f / th[:, 3]) ** (th[:, 4] - th[:, 2]))
    return v


def lu_solve(LU, piv, x, mistake=None):
    """psd_lu_solve on x [J][B], in place"""
    J = len(piv)
    order = range(J - 1, -1, -1) if mistake == "reversed_interchange" else range(J)
    if mistake != "no_interchange":
        for j in order:
            pj = int(piv[j])
            if pj != j:
                x[[j, pj]] = x[[pj, j]]
    for i in range(1, J):
        acc = x[i].copy()
        for k in range(i):
            acc -= LU[i, k] * x[k]
        x[i] = acc
    for i in range(J - 1, 0 if mistake == "no_last_row" else -1, -1):
        acc = x[i].copy()
        for k in range(i + 1, J):
            acc -= LU[i, k] * x[k]
        x[i] = acc / LU[i, i]
    return x


def band_tail(c, f_min, f_max, p):
    """psd_band_tail: int_{f_min}^{f_max} df / (1 + (f / c)^p) for c <= f_min / 2 as the series in c / f, 16 terms"""
    th, tl = c / f_min, c / f_max
    thp, tlp = th * th, tl * tl
    thp = thp * thp if p == 4 else thp * thp * thp
    tlp = tlp * tlp if p == 4 else tlp * tlp * tlp
    uh, ul, total, sign = thp / th, tlp / tl, 0.0, 1.0
    for k in range(16):
        total += sign * (uh - ul) / float(p * (k + 1) - 1)
        uh, ul, sign = uh * thp, ul * tlp, -sign
    return c * total


def norm_integral(basis, integrated, f_min, f_max, sp, x, mistake=None):
    """psd_norm_integral on x [J][B]: [B]"""
    J = len(sp)
    if not integrated or mistake == "variance_form":
        acc = np.zeros(x.shape[1])
        for j in range(J):
            acc = acc + x[j] * sp[j]
        return acc * math.pi / SQRT2 if basis == 0 else acc * 2.0 * math.pi / 3.0
    hi, lo, tail = np.zeros(x.shape[1]), np.zeros(x.shape[1]), np.zeros(x.shape[1])
    for j in range(J):
        c = sp[j]
        if c <= 0.5 * f_min and mistake != "no_tail_series":
            tail = tail + x[j] * band_tail(c, f_min, f_max, 4 if basis == 0 else 6)
            continue
        if basis == 0:
            nrm = c * x[j] / (4.0 * SQRT2)
            ph = (f_max * f_max + SQRT2 * c * f_max + c * c) / (f_max * f_max - SQRT2 * c * f_max + c * c)
            pl = (f_min * f_min + SQRT2 * c * f_min + c * c) / (f_min * f_min - SQRT2 * c * f_min + c * c)
            at = (lambda u, v: math.atan2(v, u)) if mistake == "atan2_swapped" else math.atan2
            hi = hi + nrm * (math.log(ph) + 2.0 * at(c * SQRT2 * f_max, c * c - f_max * f_max))
            lo = lo + nrm * (math.log(pl) + 2.0 * at(c * SQRT2 * f_min, c * c - f_min * f_min))
        else:
            nrm = x[j] * c / 3.0
            half = 1.0 if mistake == "no_half" else 0.5
            ph = (f_max * f_max + SQRT3 * c * f_max + c * c) / (f_max * f_max - SQRT3 * c * f_max + c * c)
            pl = (f_min * f_min + SQRT3 * c * f_min + c * c) / (f_min * f_min - SQRT3 * c * f_min + c * c)
            hi = hi + nrm * (math.atan(f_max / c) + half * math.atan2(f_max * f_max - c * c, c * f_max) + SQRT3 / 4.0 * math.log(ph))
            lo = lo + nrm * (math.atan(f_min / c) + half * math.atan2(f_min * f_min - c * c, c * f_min) + SQRT3 / 4.0 * math.log(pl))
    return (hi - lo) + tail


def approx(model, theta, norm, qpo, f_min, f_max, n_components=20, S_low=20.0, S_high=20.0, *, is_integrated_power=True, basis=0, mistake=None):
    """dict a, b, c, d [B][Jt] (Jt = n_components (2 n_components for basis 1) + n_qpo; the continuum's (c, d) are the grid's in every row),
    x [B][J] the amplitudes, I [B] the normalising integral.  qpo: [B][n_qpo][3] or None."""
    if mistake is not None and mistake not in MISTAKES:
        raise ValueError(mistake)
    th = np.atleast_2d(np.asarray(theta, float))
    B, J = th.shape[0], n_components
    norm = np.broadcast_to(np.asarray(norm, float), (B,))
    qpo = np.zeros((B, 0, 3)) if qpo is None else np.asarray(qpo, float).reshape(B, -1, 3)
    nq = qpo.shape[1]
    sp, LU, piv, c, d = setup(J, basis, f_min, f_max, S_low, S_high, mistake)
    Jc = len(c)
    p0 = psd_model(model, th, sp[0])
    x = np.stack([psd_model(model, th, sp[j]) / p0 for j in range(J)])        # [J][B]
    x = lu_solve(LU, piv, x, mistake)
    amplitudes = x.T.copy()
    integ = norm_integral(basis, is_integrated_power, f_min, f_max, sp, x, mistake)
    S0, f0q, Q = qpo[:, :, 0], qpo[:, :, 1], qpo[:, :, 2]
    De = np.sqrt(4.0 * Q * Q + 1.0) if mistake == "delta_plus" else np.sqrt(4.0 * Q * Q - 1.0)
    w0 = 2.0 * math.pi * f0q
    fa = S0 * w0 * Q / 4.0
    if mistake != "no_p0":
        fa = fa / p0[:, None]
    fb, fc = fa / De, w0 / Q / 2.0
    fd = fc * De
    if is_integrated_power and mistake != "no_feature_integral":
        def icel(xx):
            num = fc * fc + (fd + 2.0 * math.pi * xx) * (fd + 2.0 * math.pi * xx)
            den = fc * fc + (fd - 2.0 * math.pi * xx) * (fd - 2.0 * math.pi * xx)
            return (2.0 * fa * (np.arctan2(fc, fd - 2.0 * math.pi * xx) - np.arctan2(fc, fd + 2.0 * math.pi * xx)) + fb * np.log(num / den)) / (2.0 * math.pi)
        for q in range(nq):
            integ = integ + (icel(f_max)[:, q] - icel(f_min)[:, q])
    scale = norm / integ
    fas = fa * scale[:, None]
    qa = fas if mistake == "a_not_doubled" else 2.0 * fas
    qb = 2.0 * (fas / De)
    if basis == 0:
        a = x.T * scale[:, None] * sp * math.pi / SQRT2
        aa, bb = a, a
    else:
        a = x.T * scale[:, None] * sp * math.pi / 3.0
        aa = np.concatenate([a, a], axis=1)
        bb = np.concatenate([(SQRT2 if mistake == "sqrt2_for_sqrt3" else SQRT3) * a, np.zeros_like(a)], axis=1)
    ones = np.ones((B, 1))
    return {"a": np.concatenate([aa, qa], axis=1), "b": np.concatenate([bb, qb], axis=1), "c": np.concatenate([ones * c, fc], axis=1),
            "d": np.concatenate([ones * d, fd], axis=1), "x": amplitudes, "I": integ}
