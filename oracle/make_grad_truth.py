#!/usr/bin/env python3
"""TEST INFRASTRUCTURE: generates tests/golden/grad_truth.npz — log L and its gradient on a handful of small draws, evaluated densely with mpmath
at 50 digits (its own kernel function, Cholesky, inverse and sums; nothing of numpy's arithmetic): what entitles oracle.logl_grad_truth, the
long-double evaluation of the same formulas, to be called the truth of the reverse-mode kernels (tests/grad_cases.py,
tests/test_grad_host.py::test_truth_against_50_digits, tests/test_gpu_grad_truth.py).

  draw 0   R = 3  (one one-row term), N = 9, mu = 0, nu = 1
  draw 1   R = 6,  N = 17, mu and nu of its own
  draw 2   R = 9  (one one-row term), N = 24, mu and nu of its own
  draw 3   draw 2 with sigma2 x 1e-6: ill-conditioned
  draw 4   R = 5  (one one-row term), N = 12, raw flux with a shift below the data minimum (the shifted log-flux models)
  draw 5   draw 4 with sigma2 x 1e-6

Inputs are stored as the fp64 values the entry would be given; every result as a pair of doubles (hi + lo), since one double rounds by 1e-16, more
than the long-double error to be recorded.  ld_dev [draw][key]: the long-double function's deviation from the 50-digit values in the scale
tests/grad_cases.py takes deviations in.  CPU only; needs mpmath (here alone); seconds.

usage: python oracle/make_grad_truth.py"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from oracle import oracle as O  # noqa: E402

SEED = 20261019
DIGITS = 50
KEYS = ("logl", "grad_a", "grad_b", "grad_c", "grad_d", "grad_y", "grad_sigma2", "grad_mu", "scale_mu", "grad_nu", "scale_nu", "grad_shift",
        "scale_shift")
SCALED_BY = {"grad_mu": "scale_mu", "grad_nu": "scale_nu", "grad_shift": "scale_shift"}


def draw(rng, J, nreal, N, own_mu_nu):
    """one draw in the style of the test cases: gaps U(0.05, 2), sigma2 U(0.01, 0.1), a U(0.1, 2), |b| <= 0.05 a and <= 0.9 a c / d, c U(0.05, 2),
    d U(0, 3) or zero for the first nreal terms; y a realisation of the draw plus 0.3"""
    t = np.cumsum(rng.uniform(0.05, 2.0, N))
    s2 = rng.uniform(0.01, 0.1, N)
    a = rng.uniform(0.1, 2.0, J)
    b = rng.uniform(-0.05, 0.05, J) * a
    c = rng.uniform(0.05, 2.0, J)
    d = rng.uniform(0.0, 3.0, J)
    d[:nreal] = 0.0
    b = np.sign(b) * np.minimum(np.abs(b), 0.9 * a * c / np.maximum(d, 1e-300))
    b[:nreal] = 0.0
    mu, nu = (float(rng.uniform(-1.0, 1.0)), float(rng.uniform(0.5, 2.0))) if own_mu_nu else (0.0, 1.0)
    y = O.sim(a, b, c, d, t, nu * s2, rng.standard_normal(N)) + 0.3
    return dict(a=a, b=b, c=c, d=d, t=t, y=y, s2=s2, mu=mu, nu=nu, shift=np.nan)


def draws():
    rng = np.random.default_rng(SEED)
    out = [draw(rng, 2, 1, 9, False), draw(rng, 3, 0, 17, True), draw(rng, 5, 1, 24, True)]
    out.append(dict(out[2], s2=out[2]["s2"] * 1e-6))
    sh = draw(rng, 3, 1, 12, True)
    sh.update(y=np.exp(sh["y"]) + 1.0, s2=sh["s2"] * np.exp(2.0 * sh["y"]), shift=float(rng.uniform(0.1, 0.9)))
    out.append(sh)
    out.append(dict(sh, s2=sh["s2"] * 1e-6))
    return out


def truth_mpmath(dr):
    """every key of oracle.logl_grad_truth as mpmath values (lists for the arrays); the fp64 inputs taken exactly, y - mu and nu s2 formed in
    fp64 without a shift as the entry's callers form them"""
    import mpmath as mp
    mp.mp.dps = DIGITS
    M = lambda v: [mp.mpf(float(x)) for x in v]
    a, b, c, d, t = (M(dr[k]) for k in "abcdt")
    J, N = len(a), len(t)
    mu, nu = mp.mpf(dr["mu"]), mp.mpf(dr["nu"])
    shifted = not np.isnan(dr["shift"])
    if shifted:
        v = [yn - mp.mpf(dr["shift"]) for yn in M(dr["y"])]
        yc = [mp.log(vn) - mu for vn in v]
        S = [sn / (vn * vn) for sn, vn in zip(M(dr["s2"]), v)]
        sk = [nu * sn for sn in S]
    else:
        yc, S, sk = M(dr["y"] - dr["mu"]), M(dr["s2"]), M(dr["nu"] * dr["s2"])
    def kern(dt):
        return mp.fsum(mp.exp(-c[j] * dt) * (a[j] * mp.cos(d[j] * dt) + b[j] * mp.sin(d[j] * dt)) for j in range(J))
    L = [[mp.mpf(0)] * N for _ in range(N)]
    for n in range(N):
        for j in range(n):
            L[n][j] = (kern(abs(t[n] - t[j])) - mp.fdot(L[n][:j], L[j][:j])) / L[j][j]
        piv = mp.fsum(a) + sk[n] - mp.fdot(L[n][:n], L[n][:n])
        assert piv > 0, n
        L[n][n] = mp.sqrt(piv)
    W = [[mp.mpf(0)] * N for _ in range(N)]                # L^-1, column by column
    for col in range(N):
        for n in range(col, N):
            W[n][col] = ((1 if n == col else 0) - mp.fsum(L[n][k] * W[k][col] for k in range(col, n))) / L[n][n]
    Kinv = [[mp.fsum(W[k][m] * W[k][n] for k in range(max(m, n), N)) for n in range(N)] for m in range(N)]
    z = [mp.fdot(Kinv[m], yc) for m in range(N)]
    G = [[(z[m] * z[n] - Kinv[m][n]) / 2 for n in range(N)] for m in range(N)]
    out = {"logl": -mp.fdot(yc, z) / 2 - mp.fsum(mp.log(L[n][n]) for n in range(N)) - N * mp.log(2 * mp.pi) / 2}
    ga, gb, gc, gd = [], [], [], []
    for j in range(J):
        sa = sb = sc = sd = mp.mpf(0)
        for m in range(N):
            for n in range(N):
                D = abs(t[m] - t[n])
                e = mp.exp(-c[j] * D); co = mp.cos(d[j] * D); si = mp.sin(d[j] * D)
                sa += G[m][n] * e * co
                sb += G[m][n] * e * si
                sc -= G[m][n] * D * e * (a[j] * co + b[j] * si)
                sd += G[m][n] * D * e * (b[j] * co - a[j] * si)
        ga.append(sa); gb.append(sb); gc.append(sc); gd.append(sd)
    g = [G[n][n] for n in range(N)]
    out.update(grad_a=ga, grad_b=gb, grad_c=gc, grad_d=gd, grad_y=[-x for x in z], grad_sigma2=[nu * x for x in g],
               grad_mu=mp.fsum(z), scale_mu=mp.fsum(abs(x) for x in z),
               grad_nu=mp.fsum(s * x for s, x in zip(S, g)), scale_nu=mp.fsum(abs(s * x) for s, x in zip(S, g)))
    if shifted:
        terms = [zn / vn for zn, vn in zip(z, v)] + [2 * nu * gn * sn / vn ** 3 for gn, sn, vn in zip(g, M(dr["s2"]), v)]
        out.update(grad_shift=mp.fsum(terms), scale_shift=mp.fsum(abs(x) for x in terms))
    return out


def hi_lo(v):
    import mpmath as mp
    v = v if isinstance(v, list) else [v]
    hi = np.array([float(x) for x in v])
    lo = np.array([float(x - mp.mpf(h)) for x, h in zip(v, hi)])
    return hi, lo


def deviations(ld, hi, lo):
    """per key the long-double result's deviation from hi + lo in the scale of tests/grad_cases.py (NaN: the draw has no such output)"""
    want = {k: hi[k].astype(np.longdouble) + lo[k].astype(np.longdouble) for k in hi}
    out = []
    for k in KEYS:
        if k not in want or ld.get(k) is None:
            out.append(np.nan)
            continue
        err = float(np.max(np.abs(np.atleast_1d(ld[k]) - want[k])))
        scale = float(want[SCALED_BY[k]][0]) if k in SCALED_BY else float(np.max(np.abs(want[k])))
        out.append(err / scale if scale > 0 else (0.0 if err == 0 else np.inf))
    return np.array(out)


def truth_of(dr):
    shift = None if np.isnan(dr["shift"]) else dr["shift"]
    return O.logl_grad_truth(dr["a"], dr["b"], dr["c"], dr["d"], dr["t"], dr["y"], dr["s2"], mu=dr["mu"], nu=dr["nu"], shift=shift)


if __name__ == "__main__":
    out = {"seed": np.int64(SEED), "digits": np.int64(DIGITS), "keys": np.array(KEYS)}
    ds = draws()
    out["ndraws"] = np.int64(len(ds))
    ld_dev = []
    for i, dr in enumerate(ds):
        res = truth_mpmath(dr)
        hi, lo = {}, {}
        for k, v in res.items():
            if k in ("grad_y", "grad_sigma2") and not np.isnan(dr["shift"]):
                continue
            hi[k], lo[k] = hi_lo(v)
            out[f"d{i}_{k}_hi"], out[f"d{i}_{k}_lo"] = hi[k], lo[k]
        for k, v in dr.items():
            out[f"d{i}_in_{k}"] = np.asarray(v, dtype=np.float64)
        ld_dev.append(deviations(truth_of(dr), hi, lo))
        print(f"draw {i}: J = {len(dr['a'])} N = {len(dr['t'])}  long double vs {DIGITS} digits: " +
              "  ".join(f"{k} {v:.1e}" for k, v in zip(KEYS, ld_dev[-1]) if not np.isnan(v)), flush=True)
    out["ld_dev"] = np.array(ld_dev)
    print(f"largest deviation {np.nanmax(out['ld_dev']):.2e}")
    np.savez_compressed(ROOT / "tests" / "golden" / "grad_truth.npz", **out)
    print("wrote tests/golden/grad_truth.npz")
