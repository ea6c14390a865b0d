"""Writes tests/golden/psd_check_truth.npz: the PSD check (sample_approx_model, src/plots_diagnostics.jl:195-213, with plot_psd_ppc's normalisation
:404-409 and plot_f_P :419-420) at the cases of tests/psd_check_cases.py.

Everything is restated here in mpmath at 50 digits from the fp64 inputs (theta, norm, freq, f_min, f_max, S_low, S_high taken as the exact values
of their doubles): the spectral grid, B inverted once per grid, the amplitudes x = B^-1 (P(sp) / P(sp_0)), the normalising integral of get_norm_psd
(integral_sho / integral_drwcelerite, or the variance form), the model PSD normalised at the first frequency, the approximation as a sum over the
basis functions, and the residuals as the difference of the two 50-digit values (rounded to fp64 only then: the difference cancels).  It shares no
code with pioran.jl_amd/psd.py, tools/psd_check_proto.py or the kernels.  The ratios are not stored: psd_approx / psd of the stored arrays is theirs
to 2^-52.

    python tools/make_psd_check_truth.py        (about a minute)
"""
import sys
from pathlib import Path

import numpy as np
from mpmath import mp, mpf

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))
import psd_check_cases as PC  # noqa: E402

mp.dps = 50


def grid(J, basis):
    f0, fM = mpf(PC.F_MIN) / mpf(PC.S_LOW), mpf(PC.F_MAX) * mpf(PC.S_HIGH)
    sp = [f0 * (fM / f0) ** (mpf(j) / (J - 1)) for j in range(J)]
    pw = 4 if basis == 0 else 6
    Bm = mp.matrix(J, J)
    for j in range(J):
        for k in range(J):
            Bm[j, k] = 1 / (1 + (sp[j] / sp[k]) ** pw)
    return sp, Bm ** -1


def weights(sp, basis, integrated):
    """w_j with get_norm_psd = sum_j w_j x_j"""
    fmin, fmax = mpf(PC.F_MIN), mpf(PC.F_MAX)
    if not integrated:
        return [c * mp.pi / mp.sqrt(2) if basis == 0 else 2 * mp.pi * c / 3 for c in sp]
    s2, s3 = mp.sqrt(2), mp.sqrt(3)

    def sho(c, x):
        poly = (x ** 2 + s2 * c * x + c ** 2) / (x ** 2 - s2 * c * x + c ** 2)
        return c / (4 * s2) * (mp.log(poly) + 2 * mp.atan2(c * s2 * x, c ** 2 - x ** 2))

    def drw(c, x):
        poly = (x ** 2 + s3 * c * x + c ** 2) / (x ** 2 - s3 * c * x + c ** 2)
        return c / 3 * (mp.atan(x / c) + mp.atan2(x ** 2 - c ** 2, c * x) / 2 + s3 / 4 * mp.log(poly))

    fn = sho if basis == 0 else drw
    return [fn(c, fmax) - fn(c, fmin) for c in sp]


def psd(model, th, f):
    x = f / th[1]
    v = x ** (-th[0]) / (1 + x ** (th[2] - th[0]))
    if model == 1:
        v = v / (1 + (f / th[3]) ** (th[4] - th[2]))
    return v


def main():
    out = {}
    for case in PC.cases():
        m, b, J, B, F, integrated, normalise, times_f = case
        sp, Binv = grid(J, b)
        w = weights(sp, b, integrated)
        theta, norm = PC.draws(case)
        freq = PC.freqs(case)
        fr = [mpf(float(v)) for v in freq]
        pw = 4 if b == 0 else 6
        basisf = [[1 / (1 + (f / c) ** pw) for f in fr] for c in sp]          # [J][F]
        t_psd, t_app, t_res = np.empty((B, F)), np.empty((B, F)), np.empty((B, F))
        t_amp, t_int = np.empty((B, J)), np.empty(B)
        for r in range(B):
            th = [mpf(float(v)) for v in theta[r]]
            nm = mpf(float(norm[r]))
            P = [psd(m, th, c) for c in sp]
            p = [v / P[0] for v in P]
            x = [sum(Binv[j, k] * p[k] for k in range(J)) for j in range(J)]
            integ = sum(wj * xj for wj, xj in zip(w, x))
            pf0 = psd(m, th, fr[0])
            for i, f in enumerate(fr):
                vp = psd(m, th, f) / pf0 * nm
                va = sum(x[j] * nm * basisf[j][i] for j in range(J))
                if normalise:
                    vp, va = vp / integ, va / integ
                if times_f:
                    vp, va = vp * f, va * f
                t_psd[r, i], t_app[r, i], t_res[r, i] = float(vp), float(va), float(vp - va)
            t_amp[r], t_int[r] = [float(v) for v in x], float(integ)
        k = PC.name(case)
        for n, v in (("psd", t_psd), ("psd_approx", t_app), ("residuals", t_res), ("amplitudes", t_amp), ("integ", t_int), ("theta", theta),
                     ("norm", norm), ("freq", freq)):
            out[f"{k}/{n}"] = v
        print(k, flush=True)
    np.savez_compressed(ROOT / "tests" / "golden" / "psd_check_truth.npz", **out)


if __name__ == "__main__":
    main()
