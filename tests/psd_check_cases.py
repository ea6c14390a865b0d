"""Cases and bar of the PSD check (psd_check.hip: Context.psd_check and its summary form), shared by the CPU tests (the numpy twin and its
seeded mistakes, tests/test_psd_check_host.py) and the GPU tests (tests/test_gpu_psd_check.py).  A plain module, no fixtures.

cases()    (model, basis, J, B, F, integrated, normalise, times_f): B in {1, 3, 65, 257} (one draw; less than a tile of 32 draws; three tiles with one
           draw in the last; more than a block of the per-draw kernel and a draw count that is a multiple of nothing), F in {1, 63, 65, 1000} (around
           the 64-frequency tile), J in {2, 20, 35}, both models, both bases, normalise 0 / 1 with is_integrated_power 0 / 1, times_f 0 / 1.
draws()    theta as bench.py's prior draws it (as tests/theta_grad_cases.py: alpha1 ~ U(-0.25, 2), f1 log-uniform in [f_min, f_max], alpha2 ~ U(1.5, 4),
           norm log-normal; f2 = f1 10^U(0.2, 1.5), alpha3 ~ U(2, 6)).
freqs()    the reference's grid 10 .^ range(log10 f0, log10 fM, F) with freq[0] = 1.7 f0 (the normaliser of the model PSD is the model THERE, not at
           the first spectral point f0), freq[1] a spectral point of the approximation (to the bit), freq[2] below f0 and the last above fM; one
           frequency: 0.37.
truth()    tests/golden/psd_check_truth.npz (tools/make_psd_check_truth.py: everything restated in mpmath at 50 digits from the fp64 inputs).
deviations()  per array, in its natural scale: psd, psd_approx and ratios relative to the truth, residuals relative to max(|psd|, |psd_approx|) of the
           truth (the difference cancels), amplitudes relative to the largest amplitude of the draw, integ relative to the truth.
The bar for a case and an array: max(MARGIN x the fp64 twin's own deviation from the truth on that case and array, FLOOR), MARGIN = 20 and
FLOOR = 256 eps as tests/grad_cases.py and tests/theta_grad_cases.py have them, for the reason given there: the kernel forms the same sums in
another order (here: the LU solve with fused multiply-adds against LAPACK's, ocml's pow against numpy's)."""
import functools
import importlib.util
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
MARGIN, FLOOR = 20.0, 256 * np.finfo(float).eps
F_MIN, F_MAX = 1e-3, 1.0
S_LOW = S_HIGH = 20.0
BASIS_NAME = ("SHO", "DRWCelerite")
ARRAYS = ("psd", "psd_approx", "residuals", "ratios")


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


PROTO = _load("psd_check_proto", ROOT / "tools" / "psd_check_proto.py")


def cases():
    """(model, basis, J, B, F, integrated, normalise, times_f)"""
    return [(0, 0, 20, 3, 63, 1, 0, 0),
            (1, 0, 20, 65, 65, 1, 1, 0),
            (0, 1, 35, 3, 1000, 0, 1, 1),
            (1, 1, 2, 257, 1, 1, 0, 1),
            (0, 0, 2, 1, 1, 1, 0, 0),
            (1, 0, 35, 1, 65, 1, 1, 1),
            (0, 1, 20, 65, 63, 1, 1, 0),
            (1, 1, 20, 3, 65, 0, 1, 0)]


def name(case):
    m, b, J, B, F, i, n, tf = case
    return f"m{m}_b{b}_J{J}_B{B}_F{F}_i{i}_n{n}_tf{tf}"


def draws(case):
    """(theta [B][P], norm [B]) of a case"""
    m, b, J, B, F, i, n, tf = case
    rng = np.random.default_rng([20261, m, b, J, B, F])
    a1 = rng.uniform(-0.25, 2.0, B)
    f1 = np.exp(rng.uniform(np.log(F_MIN), np.log(F_MAX), B))
    a2 = rng.uniform(1.5, 4.0, B)
    norm = np.exp(np.log(0.5) + 1.25 * rng.standard_normal(B))
    ratio = 10.0 ** rng.uniform(0.2, 1.5, B)
    a3 = rng.uniform(2.0, 6.0, B)
    th = np.column_stack([a1, f1, a2] if m == 0 else [a1, f1, a2, f1 * ratio, a3])
    return np.ascontiguousarray(th), norm


def freqs(case):
    m, b, J, B, F, i, n, tf = case
    f0, fM = F_MIN / S_LOW, F_MAX * S_HIGH
    if F < 4:
        return np.full(F, 0.37)
    f = 10.0 ** np.linspace(np.log10(f0), np.log10(fM), F)
    sp, _ = PROTO.grid(J, b, F_MIN, F_MAX, S_LOW, S_HIGH)
    f[0], f[1], f[2], f[-1] = 1.7 * f0, sp[J // 2], f0 / 3.0, 3.0 * fM
    return f


def twin(case, dtype=np.float64, mistake=None):
    m, b, J, B, F, i, n, tf = case
    th, nm = draws(case)
    return PROTO.psd_check(m, th, nm, freqs(case), F_MIN, F_MAX, S_LOW, S_HIGH, J, b, integrated=i, normalise=n, times_f=tf, dtype=dtype, mistake=mistake)


@functools.lru_cache(maxsize=None)
def _file():
    with np.load(ROOT / "tests" / "golden" / "psd_check_truth.npz") as z:
        return {k: z[k] for k in z.files}


def truth(case):
    """dict of psd, psd_approx, residuals [B][F], amplitudes [B][J], integ [B] (fp64 roundings of the 50-digit values), theta, norm, freq; the ratios
    are formed from psd_approx and psd in long double (their own rounding, 2^-53 each, is far below every bar)"""
    z, k = _file(), name(case)
    out = {n: z[f"{k}/{n}"] for n in ("psd", "psd_approx", "residuals", "amplitudes", "integ", "theta", "norm", "freq")}
    out["ratios"] = (out["psd_approx"].astype(np.longdouble) / out["psd"].astype(np.longdouble))
    return out


def deviations(got, t):
    """{array: largest deviation in its natural scale} of the arrays present in `got` against the truth dict t"""
    dev = {}
    with np.errstate(invalid="ignore", divide="ignore"):
        for n in ("psd", "psd_approx", "ratios", "integ"):
            if n in got:
                dev[n] = float(np.max(np.abs((np.asarray(got[n]).astype(np.longdouble) - t[n]) / t[n])))
        if "residuals" in got:
            scale = np.maximum(np.abs(t["psd"]), np.abs(t["psd_approx"]))
            dev["residuals"] = float(np.max(np.abs(np.asarray(got["residuals"]).astype(np.longdouble) - t["residuals"]) / scale))
        if "amplitudes" in got:
            scale = np.max(np.abs(t["amplitudes"]), axis=1, keepdims=True)
            dev["amplitudes"] = float(np.max(np.abs(np.asarray(got["amplitudes"]).astype(np.longdouble) - t["amplitudes"]) / scale))
    return dev


@functools.lru_cache(maxsize=None)
def twin_dev(case):
    """the fp64 twin's own deviations from the truth on a case"""
    return deviations(twin(case), truth(case))


def bars(case):
    return {n: max(MARGIN * d, FLOOR) for n, d in twin_dev(case).items()}
