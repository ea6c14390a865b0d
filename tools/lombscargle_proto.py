"""numpy restatement of the batched generalised Lomb-Scargle periodogram (Zechmeister & Kuerster 2009, time-shift-free form) that
pioran.jl_amd/csrc/periodogram.hip evaluates — the twin the tests hold the device against.

    w = yerr^-2 / sum yerr^-2 (1/N without errors),  omega = 2 pi f
    C = sum w cos, S = sum w sin, C^ = sum w cos^2, CS^ = sum w cos sin;  CC = C^ - C^2, SS = (1 - C^) - S^2, CS = CS^ - C S, D = CC SS - CS^2
    y~ = y - sum w y (center_data),  Y = sum w y~, YY = sum w y~^2 - Y^2,  YC = sum w y~ cos - Y C, YS = sum w y~ sin - Y S
    P = (SS YC^2 + CC YS^2 - 2 CS YC YS) / (YY D)
fit_mean = False: C, S, Y taken as zero in CC, SS, CS, YC, YS, YY.

dtype = np.float64 or np.longdouble: every sum and product in that type; the series is centred first (also with center_data = False when the
mean is fitted: the power is then invariant under a constant offset, and projecting an offset series loses digits).  The phase is formed in cycles and
reduced before the trigonometric functions see it (two_prod splits f t into its rounded value and the rounding error), so it carries no
error that grows with |omega t| in either type.
"""
from __future__ import annotations

import numpy as np


def _split(a):
    c = a * 134217729.0   # 2^27 + 1 (Veltkamp)
    hi = c - (c - a)
    return hi, a - hi


def _cycles(f, t):
    """f t as (p, e) in float64 with p + e = f t exactly (Dekker's two_prod; numpy has no fma)"""
    f = np.asarray(f, dtype=np.float64)[None, :]
    t = np.asarray(t, dtype=np.float64)[:, None]
    p = t * f
    th, tl = _split(t)
    fh, fl = _split(f)
    e = ((th * fh - p) + th * fl + tl * fh) + tl * fl
    return p, e


def trig_table(t, freq, dtype=np.float64):
    """(cos, sin)(2 pi f t) as two [N][F] arrays of `dtype`"""
    p, e = _cycles(freq, t)
    r = p - np.rint(p)                                   # exact
    x = (r.astype(dtype) + e.astype(dtype)) * (dtype(2) * np.arccos(dtype(-1)))     # arccos(-1): pi in `dtype`
    return np.cos(x), np.sin(x)


def frequency_terms(t, yerr, freq, fit_mean=True, dtype=np.float64):
    """w [N], cos, sin [N][F] and the per-frequency C, S, CC, SS, CS, D [F]"""
    N = len(t)
    if yerr is None:
        w = np.full(N, dtype(1) / dtype(N), dtype=dtype)
    else:
        iv = dtype(1) / np.asarray(yerr, dtype=dtype) ** 2
        w = iv / iv.sum()
    c, s = trig_table(t, freq, dtype)
    wc = w[:, None] * c
    C, S = wc.sum(0), (w[:, None] * s).sum(0)
    Ch, CSh = (wc * c).sum(0), (wc * s).sum(0)
    if not fit_mean:
        C, S = np.zeros_like(C), np.zeros_like(S)
    CC, SS, CS = Ch - C * C, (dtype(1) - Ch) - S * S, CSh - C * S
    return w, c, s, C, S, CC, SS, CS, CC * SS - CS * CS


def lombscargle(t, y, yerr, freq, fit_mean=True, center_data=True, dtype=np.float64):
    """Standard-normalised power of y (N,) or (B, N) at freq (F,): (F,) or (B, F) in `dtype`.  A frequency with D <= 0 gives NaN."""
    y = np.asarray(y, dtype=dtype)
    Y2 = np.atleast_2d(y)
    w, c, s, C, S, CC, SS, CS, D = frequency_terms(t, yerr, freq, fit_mean, dtype)
    D = np.where(D > 0, D, dtype(np.nan))
    if center_data or fit_mean:     # with a fitted mean the power is invariant under a constant offset: take it off before projecting, as the kernel does
        Y2 = Y2 - (Y2 * w).sum(1)[:, None]
    wy = Y2 * w
    Yw = wy.sum(1) if fit_mean else np.zeros(len(Y2), dtype=dtype)
    YY = (wy * Y2).sum(1) - Yw * Yw
    YC = wy @ c - Yw[:, None] * C
    YS = wy @ s - Yw[:, None] * S
    P = (SS * YC * YC + CC * YS * YS - 2 * CS * YC * YS) / (YY[:, None] * D)
    return P[0] if y.ndim == 1 else P


def reference_grid(t, n_frequencies=1000, S_low=20, S_high=20):
    """plot_lsp_ppc's frequencies (src/plots_diagnostics.jl:522-528): log-spaced between f_min / S_low and f_max S_high of the sampling; the caller
    drops the last point as the reference does (:545)."""
    t = np.asarray(t, dtype=np.float64)
    f_min, f_max = 1.0 / (t[-1] - t[0]), 1.0 / np.min(np.diff(t)) / 2.0
    return np.exp(np.linspace(np.log(f_min / S_low), np.log(f_max * S_high), n_frequencies))
