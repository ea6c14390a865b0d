"""Writes tests/golden/approx_qpo_vjp_truth.npz: `approx` with QPO features (src/psd.jl:214-289; features :15-27, 228-241, 254-261, 330-334,
356-358) and its Jacobian at the draws of tests/qpo_grad_cases.py.

approx is restated here in mpmath at 50 digits — the spectral grid, p = P(f_j) / P(f_0), x = B^-1 p with B inverted once per grid, convert_feature,
the normalising integral of get_norm_psd with integral_celerite of the features (or the variance form, which leaves them out), the SHO and
DRWCelerite coefficient maps and the appended (2a, 2b, c, d) — and differentiated by a complex step of 1e-30 in every parameter, in norm and in
(S0, f0, Q) of every feature (every operation is analytic: atan2(c, u) is written pi / 2 - atan(u / c), valid for c > 0).  It shares no code with
pioran.jl_amd/psd.py, tools/approx_qpo_vjp_proto.py or the kernels; the grid, the weights and the power laws are tools/make_approx_vjp_truth.py's.

It also checks what the end-to-end GPU test relies on: every draw of qpo_grad_cases.END_TO_END gives a finite oracle.logl on the first 120 points
of tests/golden/simu.txt.

    python tools/make_approx_qpo_vjp_truth.py        (a few minutes)
"""
import sys
from pathlib import Path

import numpy as np
from mpmath import mp, mpc, mpf

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT))
import qpo_grad_cases as QC  # noqa: E402
from make_approx_vjp_truth import H, grid, psd, weights  # noqa: E402

mp.dps = 50
FMIN, FMAX = mpf(QC.F_MIN), mpf(QC.F_MAX)


def celerite_primitive(a, b, c, d, x):
    """integral_celerite, src/psd.jl:330-334"""
    up, um = d + 2 * mp.pi * x, d - 2 * mp.pi * x
    return (2 * a * (mp.atan(up / c) - mp.atan(um / c)) + b * mp.log((c ** 2 + up ** 2) / (c ** 2 + um ** 2))) / (2 * mp.pi)


def approx(model, basis, integrated, th, norm, qpo, sp, Binv, w):
    """(a, b, c, d) lists of the celerite terms, complex arguments allowed"""
    J = len(sp)
    P = [psd(model, th, f) for f in sp]
    p = [v / P[0] for v in P]
    x = [sum(Binv[j, k] * p[k] for k in range(J)) for j in range(J)]
    feats = []
    for S0, f0, Q in qpo:                                    # convert_feature, then a and b over P(f_0)
        delta = mp.sqrt(4 * Q ** 2 - 1)
        w0 = 2 * mp.pi * f0
        fa = S0 * w0 * Q / 4
        fc = w0 / Q / 2
        feats.append((fa / P[0], fa / delta / P[0], fc, fc * delta))
    integ = sum(wj * xj for wj, xj in zip(w, x))
    if integrated:
        integ += sum(celerite_primitive(*f, FMAX) - celerite_primitive(*f, FMIN) for f in feats)
    s = norm / integ
    if basis == 0:
        a = [xj * s * f * mp.pi / mp.sqrt(2) for xj, f in zip(x, sp)]
        b = list(a)
        c = [mp.sqrt(2) * mp.pi * f for f in sp]
        d = list(c)
    else:
        a0 = [xj * s * f * mp.pi / 3 for xj, f in zip(x, sp)]
        a, b = a0 + a0, [mp.sqrt(3) * v for v in a0] + [mpf(0)] * J
        c = [mp.pi * f for f in sp] + [2 * mp.pi * f for f in sp]
        d = [mp.sqrt(3) * mp.pi * f for f in sp] + [mpf(0)] * J
    return (a + [2 * f[0] * s for f in feats], b + [2 * f[1] * s for f in feats], c + [f[2] for f in feats], d + [f[3] for f in feats])


def check_end_to_end(out):
    from oracle import oracle as O
    A = np.loadtxt(ROOT / "tests" / "golden" / "simu.txt")
    t, y, yerr = A[:120, 0], A[:120, 1], A[:120, 2]
    for c in QC.combos():
        if (c[0], c[1], c[3], c[4]) not in QC.END_TO_END:
            continue
        k0 = QC.name(c)
        for n in range(c[5]):
            v = O.logl(*(out[f"{k0}/{f}"][n] for f in "ABCD"), t, y - QC.E2E_MU, QC.E2E_NU * yerr ** 2)
            print(k0, "draw", n, "oracle.logl", v, flush=True)
            if not np.isfinite(v):
                raise SystemExit("a draw of the end-to-end cases is not positive definite: choose other draws")


def main():
    out = {}
    grids = {}
    for c in QC.combos():
        m, b, i, J, nq, n = c
        if (J, b) not in grids:
            grids[(J, b)] = grid(J, b)
        sp, Binv = grids[(J, b)]
        w = weights(sp, b, i)
        th, nm, qp = QC.draws(c)
        Pn = th.shape[1]
        K = Pn + 1 + 3 * nq
        Jt = J * (1 + b) + nq
        val = np.zeros((4, n, Jt))
        jac = np.zeros((4, n, Jt, K))
        for r in range(n):
            base = [mpf(float(v)) for v in th[r]] + [mpf(float(nm[r]))] + [mpf(float(v)) for v in qp[r].reshape(-1)]
            for k in range(-1, K):
                z = [mpc(v, H if q == k else 0) for q, v in enumerate(base)]
                res = approx(m, b, i, z[:Pn], z[Pn], [z[Pn + 1 + 3 * q:Pn + 4 + 3 * q] for q in range(nq)], sp, Binv, w)
                for e in range(4):
                    if k < 0:
                        val[e, r] = [float(mp.re(v)) for v in res[e]]
                    else:
                        jac[e, r, :, k] = [float(mp.im(v) / H) for v in res[e]]
        k0 = QC.name(c)
        out[k0 + "/theta"], out[k0 + "/norm"], out[k0 + "/qpo"] = th, nm, qp
        for e, f in enumerate("ABCD"):
            out[f"{k0}/{f}"], out[f"{k0}/d{f}"] = val[e], jac[e]
        print(k0, flush=True)
    check_end_to_end(out)
    np.savez_compressed(ROOT / "tests" / "golden" / "approx_qpo_vjp_truth.npz", **out)


if __name__ == "__main__":
    main()
