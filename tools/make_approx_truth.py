"""Writes tests/golden/approx_truth.npz: the values of `approx` (src/psd.jl:214-289) at the draws of tests/approx_cases.py — the coefficients the
forward kernel (approx_kernel, csrc/approx.hip) is held to.

approx is restated here in mpmath at 50 digits from the fp64 inputs: the spectral grid f_j = f_0 (f_M / f_0)^(j / (J - 1)) with f_0 = f_min / S_low,
f_M = f_max S_high, p = P(f_j) / P(f_0), the amplitudes x = B^-1 p with B inverted once per grid, convert_feature, the normalising integral I of
get_norm_psd (integral_sho / integral_drwcelerite between f_min and f_max plus integral_celerite of the features, or the variance form, which leaves
the features out), the SHO and DRWCelerite coefficient maps, the appended (2a, 2b, c, d) of the features and the grid's (c, d).  The power laws and
the weights are tools/make_approx_vjp_truth.py's, integral_celerite is tools/make_approx_qpo_vjp_truth.py's; nothing is shared with
pioran.jl_amd/psd.py, tools/approx_proto.py or the kernels.

Per combo it stores theta, norm, qpo (with features), x [n][J], I [n] and A, B, C, D [n][Jt] — except for the combos whose A .. D
tests/golden/approx_qpo_vjp_truth.npz already holds: those are asserted to be reproduced (reproduces_stored(), which the CPU suite calls as well) and
not stored again.  The continuum's (a, b) are also compared with tools/make_approx_vjp_truth.py's own restatement.

It then writes the host mirrors' deviation from the truth per combo and array (tests/approx_cases.py ref_dev) into the head of
profiles/approx_truth.txt; the device's figures below it, recorded from a run of tests/test_gpu_approx_truth.py, stay.

    python tools/make_approx_truth.py        (about a minute)
"""
import sys
from pathlib import Path

import numpy as np
from mpmath import mp, mpf

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT))
import approx_cases as AC  # noqa: E402
import make_approx_vjp_truth as V  # noqa: E402
from make_approx_qpo_vjp_truth import celerite_primitive  # noqa: E402

mp.dps = 50
FMIN, FMAX = mpf(AC.F_MIN), mpf(AC.F_MAX)
DEVICE_MARK = "==== device"
_grids = {}


def grid(J, basis, S_low, S_high):
    """(sp [J], B^-1) of build_approx on [f_min / S_low, f_max S_high]; once per grid"""
    key = (J, basis, S_low, S_high)
    if key not in _grids:
        f0, fM = FMIN / mpf(S_low), FMAX * mpf(S_high)
        sp = [f0 * (fM / f0) ** (mpf(j) / (J - 1)) for j in range(J)]
        pw = 4 if basis == 0 else 6
        Bm = mp.matrix(J, J)
        for j in range(J):
            for k in range(J):
                Bm[j, k] = 1 / (1 + (sp[j] / sp[k]) ** pw)
        _grids[key] = (sp, Bm ** -1)
    return _grids[key]


def approx(model, basis, integrated, th, norm, qpo, sp, Binv, w):
    """(a, b, c, d, x, I): the celerite terms in full rows, the amplitudes and the normalising integral"""
    J = len(sp)
    P = [V.psd(model, th, f) for f in sp]
    p = [v / P[0] for v in P]
    x = [mp.fsum(Binv[j, k] * p[k] for k in range(J)) for j in range(J)]
    feats = []
    for S0, f0, Q in qpo:                                    # convert_feature, then a and b over P(f_0)
        delta = mp.sqrt(4 * Q ** 2 - 1)
        w0 = 2 * mp.pi * f0
        fa = S0 * w0 * Q / 4
        fc = w0 / Q / 2
        feats.append((fa / P[0], fa / delta / P[0], fc, fc * delta))
    integ = mp.fsum(wj * xj for wj, xj in zip(w, x))
    if integrated:
        integ += mp.fsum(celerite_primitive(*f, FMAX) - celerite_primitive(*f, FMIN) for f in feats)
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
    return (a + [2 * f[0] * s for f in feats], b + [2 * f[1] * s for f in feats], c + [f[2] for f in feats], d + [f[3] for f in feats], x, integ)


def evaluate(combo):
    """dict of a combo at its draws, rounded to fp64: theta, norm, qpo, A, B, C, D [n][Jt], x [n][J], I [n]"""
    m, b, i, J, nq, n, lo, hi = combo
    sp, Binv = grid(J, b, lo, hi)
    w = V.weights(sp, b, i)
    th, nm, qp = AC.draws(combo)
    Jt = AC.widths(combo)[1]
    val = np.zeros((4, n, Jt))
    x, integ = np.zeros((n, J)), np.zeros(n)
    for r in range(n):
        theta = [mpf(float(v)) for v in th[r]]
        feats = [] if qp is None else [[mpf(float(v)) for v in f] for f in qp[r]]
        res = approx(m, b, i, theta, mpf(float(nm[r])), feats, sp, Binv, w)
        for e in range(4):
            val[e, r] = [float(v) for v in res[e]]
        x[r], integ[r] = [float(v) for v in res[4]], float(res[5])
        if nq == 0 and (lo, hi) == (AC.TC.S_LOW, AC.TC.S_HIGH):      # the other restatement of the continuum, its own grid and inverse
            a2, b2 = V.approx(m, b, theta, mpf(float(nm[r])), *V.grid(J, b), w)
            assert np.array_equal(val[0, r], [float(v) for v in a2]) and np.array_equal(val[1, r], [float(v) for v in b2]), AC.name(combo)
    out = {"theta": th, "norm": nm, "x": x, "I": integ, **dict(zip("ABCD", val))}
    if qp is not None:
        out["qpo"] = qp
    return out


def reproduces_stored(combo, res=None):
    """whether this restatement gives, bit for bit, the A .. D that approx_qpo_vjp_truth.npz stores for the combo"""
    res = evaluate(combo) if res is None else res
    t = AC.QC.truth(combo[:6])
    return all(np.array_equal(res[f], t[f]) for f in "ABCD") and np.array_equal(res["qpo"], t["qpo"])


def write_profile(path):
    lines = ["host mirrors (pioran_jl_amd.approx_batch / approx_batch_qpo) against tests/golden/approx_truth.npz: ref_dev of tests/approx_cases.py per",
             "combo and array, largest over the combo's draws, in eps = 2.22e-16 (a, b: of the draw's largest |a|; qc, qd, gc, gd: of their own size)", ""]
    worst = {}
    for c in AC.combos():
        dev = AC.ref_dev(c)
        lines.append(f"{AC.name(c):28s} " + "  ".join(f"{k} {v / AC.EPS:8.1f}" for k, v in dev.items()))
        for k, v in dev.items():
            worst[k] = max(worst.get(k, 0.0), v)
    lines += ["", "largest over the combos:  " + "  ".join(f"{k} {v / AC.EPS:.1f} eps" for k, v in worst.items())]
    old = path.read_text() if path.exists() else ""
    tail = old[old.index(DEVICE_MARK):] if DEVICE_MARK in old else ""           # the device's figures, recorded from a GPU run, stay
    path.write_text("\n".join(lines) + "\n\n" + tail)
    print("\n".join(lines))


def main():
    out = {}
    for c in AC.combos():
        res = evaluate(c)
        k0 = AC.name(c)
        if AC.stored(c):
            assert reproduces_stored(c, res), k0
            res = {k: v for k, v in res.items() if k not in "ABCD"}
        for k, v in res.items():
            out[f"{k0}/{k}"] = v
        print(k0, flush=True)
    np.savez_compressed(ROOT / "tests" / "golden" / "approx_truth.npz", **out)
    AC._file.cache_clear()
    write_profile(ROOT / "profiles" / "approx_truth.txt")


if __name__ == "__main__":
    main()
