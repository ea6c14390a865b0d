"""numpy restatement of the PSD check that pioran.jl_amd/csrc/psd_check.hip evaluates — the model PSD against its basis-function approximation
for a batch of draws (sample_approx_model, src/plots_diagnostics.jl:195-213; plot_psd_ppc's normalisation :404-409, :419-420) — and of the
reductions of its summary form.  This twin is the definition the tests hold the device against; it runs in fp64 and, dtype=np.longdouble, in
long double (the solve is then a hand-written elimination with partial pivoting: numpy's is fp64 only).

Per draw b, with theta [B][P], norm [B], freq [F], the grid f0 = f_min / S_low, fM = f_max S_high, sp_j = f0 (fM / f0)^(j / (J - 1)),
B_jk = 1 / (1 + (sp_j / sp_k)^p), p = 4 (basis 0, SHO) or 6 (basis 1, DRWCelerite):
  2. amp_b = B \\ (P_b(sp) / P_b(sp_0))                                                   src/psd.jl:129-135
  3. psd[b][f] = P_b(freq_f) / P_b(freq_0) * norm_b                                        :202-205 — normalised at the FIRST frequency passed
  4. psd_approx[b][f] = sum_j (amp_bj norm_b) / (1 + (freq_f / sp_j)^p)                    :207, src/psd.jl:171-179; j ascending, r2 = r r, r4 = r2 r2, r6 = r4 r2
  6. normalise: both divided by integ_b = get_norm_psd(amp_b, sp, f_min, f_max, basis, integrated)   :404-409;   times_f: both multiplied by freq_f after that   :419-420
  5. residuals = psd - psd_approx,  ratios = psd_approx / psd                              :210-211, of the arrays as divided and multiplied
  7. status[b] = 2 and NaN in every row of the draw when a theta or the norm is not finite, P_b(freq_0) or P_b(sp_0) is not positive and finite, or,
     with normalise, integ_b is zero or not finite; else 0.
`mistake` seeds one wrong turn per step, for tests/test_psd_check_host.py to catch against the 50-digit truth:
  amp_unnormalised   step 2: the right-hand side is P_b(sp), not divided by P_b(sp_0)
  normaliser_sp0     step 3: the model PSD is divided by P_b(sp_0) instead of P_b(freq_0)
  approx_no_norm     step 4: norm_b left out of the approximation
  wrong_power        step 4: the other basis's power in the sum
  ratio_inverted     step 5: ratios = psd / psd_approx
  integ_model_only   step 6: only the model PSD is divided by integ_b
  times_f_residuals  step 6: the residuals are formed before the multiplication by freq_f
"""
from __future__ import annotations

import importlib.util
from pathlib import Path

import numpy as np

MISTAKES = ("amp_unnormalised", "normaliser_sp0", "approx_no_norm", "wrong_power", "ratio_inverted", "integ_model_only", "times_f_residuals")
NAMES = ("psd", "psd_approx", "residuals", "ratios")


def _quantiles_proto():
    spec = importlib.util.spec_from_file_location("quantiles_proto", Path(__file__).resolve().parent / "quantiles_proto.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def model_psd(model, theta, f):
    """P_b(f) for theta [B][P] and f [F] -> [B][F], in the dtype of theta (Tonari's closed forms, test/test_psd.jl:3-13)"""
    f = f[None, :]
    a1, f1, a2 = (theta[:, k:k + 1] for k in range(3))
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        v = (f / f1) ** (-a1) / (1 + (f / f1) ** (a2 - a1))
        if model == 1:
            f2, a3 = theta[:, 3:4], theta[:, 4:5]
            v = v / (1 + (f / f2) ** (a3 - a2))
    return v


def grid(J, basis, f_min, f_max, S_low, S_high, dtype=np.float64):
    """(sp [J], B [J][J]) of build_approx (src/psd.jl:73-102)"""
    f0, fM = dtype(f_min) / dtype(S_low), dtype(f_max) * dtype(S_high)
    sp = f0 * (fM / f0) ** (np.arange(J).astype(dtype) / dtype(J - 1))
    return sp, 1 / (1 + (sp[:, None] / sp[None, :]) ** (4 if basis == 0 else 6))


def solve(Bm, rhs):
    """Bm \\ rhs for rhs [J][n]: numpy's solve in fp64, elimination with partial pivoting in any other dtype"""
    if Bm.dtype == np.float64:
        return np.linalg.solve(Bm, rhs)
    A, X = Bm.copy(), rhs.copy()
    J = len(A)
    for k in range(J):
        p = k + int(np.argmax(np.abs(A[k:, k])))
        if p != k:
            A[[k, p]], X[[k, p]] = A[[p, k]], X[[p, k]]
        for i in range(k + 1, J):
            l = A[i, k] / A[k, k]
            A[i, k:] -= l * A[k, k:]
            X[i] -= l * X[k]
    for i in range(J - 1, -1, -1):
        X[i] = (X[i] - A[i, i + 1:] @ X[i + 1:]) / A[i, i]
    return X


def norm_integral(amp, sp, f_min, f_max, basis, integrated):
    """get_norm_psd (src/psd.jl:375-395) for amp [B][J]"""
    dt = amp.dtype.type
    if not integrated:
        pi = dt(np.pi) if dt is np.float64 else np.arctan(dt(1)) * 4
        s = np.sum(amp * sp, axis=-1)
        return s * pi / np.sqrt(dt(2)) if basis == 0 else s * 2 * pi / 3

    def sho(x):                                   # integral_sho :301-305
        s2 = np.sqrt(dt(2))
        poly = (x ** 2 + s2 * sp * x + sp ** 2) / (x ** 2 - s2 * sp * x + sp ** 2)
        return np.sum(sp * amp / (4 * s2) * (np.log(poly) + 2 * np.arctan2(sp * s2 * x, sp ** 2 - x ** 2)), axis=-1)

    def drw(x):                                   # integral_drwcelerite :318-324
        s3 = np.sqrt(dt(3))
        poly = (x ** 2 + s3 * sp * x + sp ** 2) / (x ** 2 - s3 * sp * x + sp ** 2)
        return np.sum(amp * sp / 3 * (np.arctan(x / sp) + np.arctan2(x ** 2 - sp ** 2, sp * x) / 2 + s3 / 4 * np.log(poly)), axis=-1)

    fn = sho if basis == 0 else drw
    return fn(dt(f_max)) - fn(dt(f_min))


def psd_check(model, theta, norm, freq, f_min, f_max, S_low, S_high, J, basis, integrated=1, normalise=0, times_f=0, dtype=np.float64, mistake=None):
    """dict of psd, psd_approx, residuals, ratios [B][F], amplitudes [B][J], integ [B] (in `dtype`) and status [B]"""
    assert mistake is None or mistake in MISTAKES, mistake
    theta = np.atleast_2d(np.asarray(theta, dtype=np.float64)).astype(dtype)
    B = len(theta)
    norm = np.broadcast_to(np.asarray(norm, dtype=np.float64), (B,)).astype(dtype)
    freq = np.asarray(freq, dtype=np.float64).reshape(-1).astype(dtype)
    sp, Bm = grid(J, basis, f_min, f_max, S_low, S_high, dtype)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        p = model_psd(model, theta, sp)
        p_sp0 = p[:, 0].copy()
        rhs = p if mistake == "amp_unnormalised" else p / p_sp0[:, None]
        bad_in = ~(np.isfinite(rhs).all(axis=1))
        amp = solve(Bm, np.where(bad_in[:, None], 0, rhs).T).T.copy()
        amp[bad_in] = np.nan
        integ = norm_integral(amp, sp, f_min, f_max, basis, integrated)
        p_f0 = model_psd(model, theta, freq[:1])[:, 0]
        psd = model_psd(model, theta, freq) / (p_sp0 if mistake == "normaliser_sp0" else p_f0)[:, None] * norm[:, None]
        r = freq[None, :] / sp[:, None]                                    # [J][F]
        r2 = r * r
        r4 = r2 * r2
        pw = r4 if (basis == 0) != (mistake == "wrong_power") else r4 * r2
        approx = np.zeros_like(psd)
        for j in range(J):
            aj = amp[:, j] if mistake == "approx_no_norm" else amp[:, j] * norm
            approx = approx + aj[:, None] / (1 + pw[j])[None, :]
        early_res = psd - approx
        if normalise:
            psd = psd / integ[:, None]
            if mistake != "integ_model_only":
                approx = approx / integ[:, None]
            early_res = psd - approx
        if times_f:
            psd, approx = psd * freq[None, :], approx * freq[None, :]
        res = early_res if mistake == "times_f_residuals" else psd - approx
        rat = psd / approx if mistake == "ratio_inverted" else approx / psd
        ok = np.isfinite(theta).all(axis=1) & np.isfinite(norm) & np.isfinite(p_sp0) & (p_sp0 > 0) & np.isfinite(p_f0) & (p_f0 > 0)
        if normalise:
            ok &= np.isfinite(integ) & (integ != 0)
    out = dict(psd=psd, psd_approx=approx, residuals=res, ratios=rat, amplitudes=amp, integ=integ)
    for v in out.values():
        v[~ok] = np.nan
    out["status"] = np.where(ok, 0, 2).astype(np.int32)
    return out


def summary(arrays, status, probs):
    """(quant [4][Q][F], mean [4][F], meta [B][8], kept) of the summary form from the [B][F] arrays of psd_check: per frequency the quantiles and
    the mean over the draws with status 0 (tools/quantiles_proto.py), per draw mean, median, min |.|, max |.| over the frequencies of the
    residuals, then of the ratios (plot_boxplot_psd_approx :43-51); NaN in the meta row of a draw with status 2"""
    QP = _quantiles_proto()
    X = [np.asarray(arrays[n], dtype=np.float64) for n in NAMES]
    B, F = X[0].shape
    quant = np.empty((4, len(probs), F))
    mean = np.empty((4, F))
    kept = 0
    for a in range(4):
        quant[a], mean[a], kept = QP.quantiles(X[a], probs, status=status)
    meta = np.full((B, 8), np.nan)
    ok = np.asarray(status) == 0
    for k, Xa in enumerate(X[2:]):
        if ok.any():
            med, mn, _ = QP.quantiles(Xa[ok].T, [0.5])
            meta[ok, 4 * k], meta[ok, 4 * k + 1] = mn, med[0]
            meta[ok, 4 * k + 2], meta[ok, 4 * k + 3] = np.min(np.abs(Xa[ok]), axis=1), np.max(np.abs(Xa[ok]), axis=1)
    return quant, mean, meta, kept
