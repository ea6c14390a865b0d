"""Writes tests/golden/carma_truth.npz: the CARMA map of tests/carma_cases.py's draws restated in mpmath at 100 digits.

It shares no code with the twin (tools/carma_proto.py), pioran.jl_amd/kernels.py or the kernels: the roots are formed in complex arithmetic as
quad2roots does (src/CARMA.jl:201-223), beta as roots2coeffs(quad2roots(qb)) — the product of (x - r) over the complex roots, real part taken —,
the coefficients as CARMA_celerite_coefs writes them (powers of the root, src/CARMA.jl:98-143), the PSD as evaluate does (alpha from the roots'
product, both polynomials summed in powers of i w, CARMA_normalisation over all roots; :150-172, :279-300).

The Jacobian w.r.t. (qa, qb, norm) is by central differences with h = 1e-40 |x| in the same 100-digit arithmetic.  For a well-separated pair
h = 1e-20 |x| in 60 digits would do; for the nearly degenerate pair of each combo it would not: a relative step h in c moves c - b^2 / 4 (down to 1e-9
here, with c up to 1e4) by h c / (c - b^2 / 4) <= 1e13 h in relative terms, and the truncation error is the square of that — 1e-14 at h = 1e-20,
1e-54 at h = 1e-40, where the rounding error 1e-100 / 1e-40 is still far below 25 digits.  check_step() compares two step sizes on the (16, 15)
degenerate draw.

    python tools/make_carma_truth.py          # ~ 1 minute
"""
import sys
from pathlib import Path

import mpmath as mp
import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

mp.mp.dps = 100
H_REL = mp.mpf(10) ** -40


def quad_roots(quad):
    n = len(quad)
    r = []
    for k in range(0, n - n % 2, 2):
        c, b = quad[k], quad[k + 1]
        delta = b * b - 4 * c
        assert delta < 0
        s = mp.sqrt(-delta)
        r += [mp.mpc(-b, s) / 2, mp.mpc(-b, -s) / 2]
    if n % 2:
        r.append(mp.mpc(-quad[-1], 0))
    return r


def from_roots(r):
    c = [mp.mpc(1)]
    for root in r:
        c = [(c[i - 1] if i >= 1 else 0) - (root * c[i] if i < len(c) else 0) for i in range(len(c) + 1)]
    return c


def poly_at(coef, x):
    s, xp = mp.mpc(0), mp.mpc(1)
    for cl in coef:
        s += cl * xp
        xp *= x
    return s


def variance_term(r, beta, k):
    """num / den of root k as CARMA_normalisation writes it, without the -2 Re r (the callers divide)"""
    rk = r[k]
    num = poly_at(beta, rk) * poly_at(beta, -rk)
    den = mp.mpc(1)
    for j, rj in enumerate(r):
        if j != k:
            den *= (rj - rk) * (mp.conj(rj) + rk)
    return num / den


def forward(qa, qb, norm, integrated, freq=None):
    """(a, b, c, d) lists of J mpf, and with freq the PSD there"""
    p = len(qa)
    r = quad_roots(qa)
    beta = [mp.re(x) for x in from_roots(quad_roots(qb))]
    J = (p + 1) // 2
    a, b, c, d = [], [], [], []
    for k in range(J):
        rk = r[2 * k]
        fr = -variance_term(r, beta, 2 * k) / mp.re(rk)
        if p % 2 == 1 and k == J - 1:
            a.append(mp.re(fr)); b.append(mp.mpf(0)); c.append(-mp.re(rk)); d.append(mp.mpf(0))
        else:
            a.append(2 * mp.re(fr)); b.append(2 * mp.im(fr)); c.append(-mp.re(rk)); d.append(-mp.im(rk))
    va = norm / mp.fsum(a) if integrated else norm
    out = ([x * va for x in a], [x * va for x in b], c, d)
    if freq is None:
        return out
    alpha = from_roots(r)
    normalisation = mp.re(mp.fsum(variance_term(r, beta, k) / (-2 * mp.re(r[k])) for k in range(p)))
    psd = []
    for f in freq:
        wi = mp.mpc(0, 2 * mp.pi * f)
        ratio = abs(poly_at(beta, wi) / poly_at(alpha, wi)) ** 2
        psd.append(2 * ratio * norm / normalisation if integrated else 4 * ratio * norm)
    return out, r, beta, psd


def jacobian(qa, qb, norm, integrated, h_rel=H_REL):
    """[4][J][p + q + 1] of mpf"""
    x = list(qa) + list(qb) + [norm]
    p, q = len(qa), len(qb)
    cols = []
    for i in range(len(x)):
        h = abs(x[i]) * h_rel
        xp, xm = list(x), list(x)
        xp[i] += h
        xm[i] -= h
        fp = forward(xp[:p], xp[p:p + q], xp[-1], integrated)
        fm = forward(xm[:p], xm[p:p + q], xm[-1], integrated)
        cols.append([[(u - v) / (2 * h) for u, v in zip(fp[k], fm[k])] for k in range(4)])
    J = len(cols[0][0])
    return [[[cols[i][k][j] for i in range(len(x))] for j in range(J)] for k in range(4)]


def check_step(cases):
    """largest relative change of the Jacobian of the (16, 15) degenerate draw between h = 1e-40 |x| and 1e-45 |x|"""
    combo = (16, 15, 1)
    qa, qb, norm = cases.draws(combo)
    args = ([mp.mpf(float(v)) for v in qa[1]], [mp.mpf(float(v)) for v in qb[1]], mp.mpf(float(norm[1])), True)
    j1, j2 = jacobian(*args), jacobian(*args, h_rel=mp.mpf(10) ** -45)
    worst = mp.mpf(0)
    for k in range(4):
        for u, v in zip(j1[k], j2[k]):
            for s, t in zip(u, v):
                if t != 0:
                    worst = max(worst, abs(s - t) / abs(t))
    return worst


def main():
    import carma_cases as cases
    out = {}
    for combo in cases.combos():
        p, q, i = combo
        qa, qb, norm = cases.draws(combo)
        rows = {k: [] for k in ("r_re", "r_im", "beta", "a", "b", "c", "d", "jac", "psd")}
        for n in range(len(qa)):
            mqa, mqb, mn = [mp.mpf(float(v)) for v in qa[n]], [mp.mpf(float(v)) for v in qb[n]], mp.mpf(float(norm[n]))
            (a, b, c, d), r, beta, psd = forward(mqa, mqb, mn, bool(i), [mp.mpf(float(f)) for f in cases.FREQ])
            jac = jacobian(mqa, mqb, mn, bool(i))
            rows["r_re"].append([float(mp.re(x)) for x in r]); rows["r_im"].append([float(mp.im(x)) for x in r])
            rows["beta"].append([float(x) for x in beta])
            for key, v in zip("abcd", (a, b, c, d)):
                rows[key].append([float(x) for x in v])
            rows["jac"].append([[[float(x) for x in row] for row in arr] for arr in jac])
            rows["psd"].append([float(x) for x in psd])
        k = cases.name(combo) + "/"
        out[k + "qa"], out[k + "qb"], out[k + "norm"] = qa, qb, norm
        out[k + "r_alpha"] = np.array(rows["r_re"]) + 1j * np.array(rows["r_im"])
        for key in ("beta", "a", "b", "c", "d", "jac", "psd"):
            out[k + key] = np.array(rows[key], dtype=np.float64)
        print(k, out[k + "jac"].shape, flush=True)
    print("step check (relative change of the Jacobian, h 1e-40 -> 1e-45):", mp.nstr(check_step(cases), 5))
    np.savez_compressed(ROOT / "tests" / "golden" / "carma_truth.npz", **out)


if __name__ == "__main__":
    main()
