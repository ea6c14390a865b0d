"""Cases and checker for log L and its gradient (pioran_celerite_logl_grad / _shift: Dataset.logl_grad, what the HMC / NUTS users call at every
leapfrog step), shared by the CPU tests (the fp64 references and seeded mistakes, tests/test_grad_host.py) and the GPU tests (every reverse-mode
family, tests/test_gpu_grad_truth.py).  A plain module, no fixtures; draws, constants and the style follow tests/predict_var_cases.py and
tests/predict_mean_cases.py.

edge_cases()   the shapes at which the reverse-mode kernels take another branch (celerite_block.hip, celerite_tile.hip, celerite_wide.hip): rows R on
               both sides of every step of rpl_of (15 | 16 .. 127 | 128, 143) and of the block columns NB = (R + 16) / 16; series around the KW = 16
               windows and their ragged ends, with nseg = ceil((N - 1) / K) = 0 .. 4 checkpoint segments and on both sides of the K = 16 | 32 | 64 switches
               at N = 64 | 65 and 256 | 257; the wide shape R = 80 with one, two and three or more segments; 5 draws where N <= 34 (the last workgroup
               of the tile reverse kernel partly filled at 4, 3 and 2 draws per workgroup), 3 up to N = 129, 2 above, each with its own mu and nu.
               Each shape with sigma2 as drawn and x 1e-6; four shapes also on raw flux with a shift per draw.
fuzz_cases()   seeded random shapes: R 1 .. 143, N 1 .. 200, one-row terms at random places, sigma2 x 10^U(-6, 0).
reference()    the truth oracle.logl_grad_truth (dense, long double, shares nothing with the recurrences) and ref_dev.
check()        an implementation against the truth.

Deviations are taken in the natural scale of each output, per draw:
    grad_a, grad_b, grad_c, grad_d     max_j |got_j - truth_j| / max_j |truth_j|
    grad_y, grad_sigma2                the same over n
    grad_mu, grad_nu, grad_shift       |got - truth| / (the sum of the absolute terms of the sum that defines it)
    logl                               |got - truth| / |truth|
and the bound per case, draw and key is max(MARGIN x ref_dev, FLOOR).  ref_dev is the worst deviation, from the same truth on the same draw in
the same scale, of the fp64 evaluations that are not the code under test: the complex step through the C restatement of the recurrence
(oracle.logl_grad / oracle.logl_dir; the series gradients, 2 N evaluations, only where N <= 129, or 66 past 63 rows) and a dense fp64 evaluation of the same
G (.) dK sums with np.linalg.  MARGIN = 20 and FLOOR = 256 eps are those of tests/predict_var_cases.py and carry over for the reason given there
and in tests/predict_mean_cases.py: the kernels form the same sums as these fp64 evaluations in another order (window by window, MFMA tiles, LDS
atomics), which moves a result by a few of the reference's own roundings, not by orders of magnitude.

One family and key has a bound of its own, set from a CPU prototype and not from the kernels: grad_d of the step-by-step reverse mode
(celerite_wide.hip).  Its form adds t_n x (terms in the absolute phases d_j t_n) to one accumulator per row, and the accumulators exceed their
sum by up to 9e3 on these cases (series span / correlation time), which amplifies the roundings of the terms; tools/wide_adjoint_dd_proto.py
restates that form densely, is the dense formula to 2e-15 in long double and deviates by up to 8e-12 in fp64 where the fp64 references stay at
1e-12.  wide_bounds() therefore takes max(MARGIN x max(ref_dev, form_dev), FLOOR) for that key, form_dev being the prototype's own fp64
deviation on the same draw (docs/EXPERIMENTS.md section 28).  The windowed families take differences within a window first and keep the
common bound.

An entry that is structurally zero — grad_b_j, grad_d_j of a one-row term (b_j = d_j = 0) — is not masked: it counts in the deviation like any
other, and check() asserts that it is exactly 0.0, the contract of include/pioran_hip.h."""
import importlib.util
import sys
import zlib
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np

from oracle import oracle as O

sys.path.insert(0, str(Path(__file__).resolve().parent))
import predict_mean_cases as PM  # noqa: E402
from predict_var_cases import FLOOR, MARGIN, _draws, draw_cd  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]

ROWS = (1, 2, 5, 6, 15, 16, 17, 31, 32, 33, 47, 48, 49, 62, 63)              # at N in ROWS_N
ROWS_N = (3, 17)
WIDE_ROWS = (64, 65, 79, 80, 95, 96, 111, 112, 127, 128, 143)                # at N in WIDE_N
WIDE_N = (1, 2, 5, 9, 18)
LENGTHS = (1, 2, 3, 4, 5, 8, 9, 15, 16, 17, 18, 31, 32, 33, 34, 48, 49, 50, 64, 65, 66, 97, 98, 129, 256, 257)   # at R in LENGTHS_R
LENGTHS_R = (3, 33)
WIDE_LENGTHS = ((80, 17), (80, 18), (80, 49), (80, 65))                      # RPL 6: one, two, three or more segments of the step-by-step reverse mode
SHIFT_SHAPES = ((5, 17), (33, 33), (33, 129), (80, 9))
S2_VARIANTS = (("s2x1", 1.0), ("s2x1e-6", 1e-6))
SERIES_REF_MAX_N = 129                                                       # complex-step series gradients (2 N evaluations) up to here ...
SERIES_REF_MAX_N_WIDE = 66                                                   # ... and up to here past 63 rows (an evaluation costs N R^2)
TERM_KEYS = ("grad_a", "grad_b", "grad_c", "grad_d")
SERIES_KEYS = ("grad_y", "grad_sigma2")
SUM_KEYS = {"grad_mu": "scale_mu", "grad_nu": "scale_nu", "grad_shift": "scale_shift"}
ALL_KEYS = ("logl",) + TERM_KEYS + SERIES_KEYS + tuple(SUM_KEYS)
KW = 16


# ---- the routing constants of celerite_wide.hip / celerite_block.hip / celerite_tile.hip, restated --------------------------------------------
def rpl_of(R):
    return next(i + 1 for i, top in enumerate((15, 31, 47, 63, 79, 95, 111, 127, 10 ** 9)) if R <= top)


def ckpt_every(N):
    k = 16
    while k < 256 and k * k < 4 * N:
        k *= 2
    return k


def nseg_of(N):
    K = ckpt_every(N)
    return (N - 1 + K - 1) // K


def block_columns(R):
    return (R + 16) // 16


def tile_adj_waves(R, cd):
    return 4 if block_columns(R) <= 3 else (2 if cd else 3)


def series_ref(case):
    """whether the complex-step reference is asked for the series gradients of this case (the dense reference always is)"""
    return len(case[1]) <= (SERIES_REF_MAX_N if rows(case) <= 63 else SERIES_REF_MAX_N_WIDE)


def n_draws(N):
    return 5 if N <= 34 else 3 if N <= 129 else 2


def rows(case):
    A, Dd = case[4], case[7]
    return 2 * A.shape[1] - int(np.sum(np.atleast_2d(Dd)[0] == 0.0))


# ---- cases ---------------------------------------------------------------------------------------------------------------------------------
def _rng(label):
    return np.random.default_rng([20261019, zlib.crc32(label.encode())])


def edge_combinations():
    """(R, N), each once"""
    out = [(R, N) for R in ROWS for N in ROWS_N]
    out += [(R, N) for R in WIDE_ROWS for N in WIDE_N]
    out += [(R, N) for N in LENGTHS for R in LENGTHS_R]
    out += list(WIDE_LENGTHS)
    return list(dict.fromkeys(out))


def _shape(R, N):
    """(stem, t, s2, A, Bc, C, Dd, mu, nu, q) of one shape, seeded by its label; one-row terms mixed in as predict_mean_cases._shape does"""
    stem = f"R{R}-N{N}"
    rng = _rng(stem)
    B = n_draws(N)
    nreal = R % 2 + (2 * int(rng.integers(0, 2)) if 4 <= R <= 62 else 0)
    J = (R + nreal) // 2
    t, s2, A, Bc, C, Dd, nu = _draws(rng, N, J, B, np.arange(nreal))
    mu = rng.uniform(-1.0, 1.0, B)
    q = rng.standard_normal(N)
    return stem, t, s2, A, Bc, C, Dd, mu, nu, q


def _case(label, t, s2, A, Bc, C, Dd, mu, nu, q):
    y = PM.make_y(t, s2, A, Bc, C, Dd, nu, q)         # a realisation of draw 0 plus a constant: z = K^-1 (y - mu) stays of the size of y
    return (label, t, y, s2, A, Bc, C, Dd, mu, nu, None)


def shifted(case):
    """the case on raw flux: y_raw = exp(y) + 1 with variances sigma2 exp(2 y) and a shift c_b in (0.1, 0.9) per draw, below the data minimum —
    the transformed series log(y_raw - c_b) and its variances stay of the size of the case's own (as tests/rand_posterior_cases.py does)"""
    label, t, y, s2, A, Bc, C, Dd, mu, nu, _ = case
    label += "-shift"
    c = _rng(label).uniform(0.1, 0.9, len(A))
    return (label, t, np.exp(y) + 1.0, s2 * np.exp(2.0 * y), A, Bc, C, Dd, mu, nu, c)


def edge_cases():
    """yields (label, t, y, s2, A, Bc, C, Dd, mu, nu, shift): B draws with their own mu and nu, (c, d) shared; shift None or [B] (the data set
    then holds raw flux); R = 2 J - (terms with b = d = 0) rows"""
    for R, N in edge_combinations():
        stem, t, s2, A, Bc, C, Dd, mu, nu, q = _shape(R, N)
        for tag, scale in S2_VARIANTS:
            case = _case(f"{stem}-{tag}", t, s2 * scale, A, Bc, C, Dd, mu, nu, q)
            yield case
            if (R, N) in SHIFT_SHAPES:
                yield shifted(case)


def n_edge_cases():
    return 2 * (len(edge_combinations()) + len(SHIFT_SHAPES))


def fuzz_cases(n=40, seed=20261022):
    """yields n cases as edge_cases(): R in 1 .. 143 with a random number of one-row terms at random places, N in 1 .. 200, 1 .. 4 draws,
    sigma2 scaled by 10^U(-6, 0); (c, d) shared, no shift"""
    for i in range(n):
        rng = np.random.default_rng([seed, i])
        R = int(rng.integers(1, 144))
        nreal = R % 2 + 2 * int(rng.integers(0, min(R, 143 - R) // 2 + 1)) * int(rng.random() < 0.5)
        J = (R + nreal) // 2
        N = int(rng.integers(1, 201))
        B = int(rng.integers(1, 5))
        t, s2, A, Bc, C, Dd, nu = _draws(rng, N, J, B, rng.permutation(J)[:nreal])
        mu = rng.uniform(-1.0, 1.0, B)
        scale = 10.0 ** rng.uniform(-6, 0)
        yield _case(f"fuzz{i}-R{R}-N{N}-B{B}-J{J}", t, s2 * scale, A, Bc, C, Dd, mu, nu, rng.standard_normal(N))


def per_draw_variant(case):
    """the case with (c, d) of its own in every draw (predict_mean_cases.per_draw_variant)"""
    v = PM.per_draw_variant(case[:10] + (None, None))
    return v[:10] + case[10:]


def one_draw(case, k):
    """draw k of a case as a one-draw case with shared (c, d)"""
    label, t, y, s2, A, Bc, C, Dd, mu, nu, shift = case
    c, d = draw_cd(C, Dd, k)
    return (f"{label}/draw{k}", t, y, s2, A[k:k + 1], Bc[k:k + 1], c, d, mu[k:k + 1], nu[k:k + 1], None if shift is None else shift[k:k + 1])


# ---- the fp64 references ---------------------------------------------------------------------------------------------------------------------
def _series(case, k):
    """what draw k is evaluated on, in fp64: (y - mu, nu S, S, v) with S the data set's variances or the transformed ones, v = y - shift or None"""
    label, t, y, s2, A, Bc, C, Dd, mu, nu, shift = case
    if shift is None:
        return y - mu[k], nu[k] * s2, s2, None
    v = y - shift[k]
    return np.log(v) - mu[k], nu[k] * s2 / v ** 2, s2 / v ** 2, v


_ref_out = {}          # the references' outputs by (name, label, draw[, series]): check()'s legs and seeded mistakes ask for them again


def complex_step(case, k, series):
    """every output of draw k by complex steps through the C restatement of the recurrence (exact to rounding for that recurrence); read-only"""
    label, t, y, s2, A, Bc, C, Dd, mu, nu, shift = case
    series = bool(series and shift is None)
    if ("complex_step", label, k, series) in _ref_out:
        return _ref_out["complex_step", label, k, series]
    c, d = draw_cd(C, Dd, k)
    yc, sk, S, v = _series(case, k)
    N = len(t)
    out = O.logl_grad(A[k], Bc[k], c, d, t, yc, sk, series=series, cd=True)
    if "grad_sigma2" in out:
        out["grad_sigma2"] = nu[k] * out["grad_sigma2"]
    out["logl"] = O.logl(A[k], Bc[k], c, d, t, yc, sk)
    out["grad_mu"] = O.logl_dir(A[k], Bc[k], c, d, t, yc, sk, dy=-np.ones(N))
    out["grad_nu"] = O.logl_dir(A[k], Bc[k], c, d, t, yc, sk, ds2=S)
    if shift is not None:
        out["grad_shift"] = O.logl_dir(A[k], Bc[k], c, d, t, yc, sk, dy=-1 / v, ds2=nu[k] * 2 * s2 / v ** 3)
    _ref_out["complex_step", label, k, series] = out
    return out


def dense_fp64(case, k):
    """every output of draw k by the G (.) dK sums in fp64 with np.linalg: K = L L', K^-1 = L^-T L^-1, G = (z z' - K^-1) / 2; read-only"""
    label, t, y, s2, A, Bc, C, Dd, mu, nu, shift = case
    if ("dense_fp64", label, k) in _ref_out:
        return _ref_out["dense_fp64", label, k]
    a, b = A[k], Bc[k]
    c, d = draw_cd(C, Dd, k)
    yc, sk, S, v = _series(case, k)
    N = len(t)
    D = np.abs(t[:, None] - t[None, :])
    E = np.exp(-c * D[..., None])
    Co, Si = E * np.cos(d * D[..., None]), E * np.sin(d * D[..., None])
    L = np.linalg.cholesky((a * Co + b * Si).sum(-1) + np.diag(sk))
    W = np.linalg.solve(L, np.eye(N))
    Kinv = W.T @ W
    z = W.T @ (W @ yc)
    G = 0.5 * (np.outer(z, z) - Kinv)
    J = len(a)
    Co, Si, GD = Co.reshape(-1, J), Si.reshape(-1, J), (G * D).ravel()
    ga, gb = G.ravel() @ Co, G.ravel() @ Si
    gco, gsi = GD @ Co, GD @ Si
    g = np.diag(G)
    out = {"logl": -0.5 * yc @ z - np.log(np.diag(L)).sum() - 0.5 * N * np.log(2 * np.pi), "grad_a": ga, "grad_b": gb,
           "grad_c": -(a * gco + b * gsi), "grad_d": b * gco - a * gsi, "grad_mu": z.sum(), "grad_nu": (S * g).sum()}
    if shift is None:
        out.update(grad_y=-z, grad_sigma2=nu[k] * g)
    else:
        out["grad_shift"] = (z / v).sum() + (2 * nu[k] * g * s2 / v ** 3).sum()
    _ref_out["dense_fp64", label, k] = out
    return out


def deviation(got, truth, key):
    """the deviation of one draw's output from its truth (the dict of oracle.logl_grad_truth) in the natural scale of `key`"""
    want = truth[key]
    err = float(np.max(np.abs(np.asarray(got, dtype=np.longdouble) - want)))
    if key in SUM_KEYS:
        scale = float(truth[SUM_KEYS[key]])
    else:
        scale = float(np.max(np.abs(want)))
    if not np.isfinite(err):
        return np.inf
    return err / scale if scale > 0 else (0.0 if err == 0 else np.inf)          # (all of it structurally zero: only exact zeros agree)


def keys_of(case, series=True):
    """the output keys a case has: no series gradients with a shift (the entry does not return them), grad_shift only with one"""
    shift = case[10]
    return ("logl",) + TERM_KEYS + (SERIES_KEYS if shift is None and series else ()) + ("grad_mu", "grad_nu") + (("grad_shift",) if shift is not None else ())


_reference = {}


def reference(case):
    """(truth, ref_dev, parts): truth [B] dicts of oracle.logl_grad_truth (raises unless positive definite); ref_dev: key -> [B]; parts: the
    two references' own deviations, name -> key -> [B] (NaN where a reference was not asked for the key).  Computed once per label, never
    changed afterwards."""
    label, t, y, s2, A, Bc, C, Dd, mu, nu, shift = case
    if label in _reference:
        return _reference[label]
    B, N = len(A), len(t)
    keys = keys_of(case)
    truth = []
    parts = {name: {key: np.full(B, np.nan) for key in keys} for name in ("complex_step", "dense_fp64")}
    O.lib()
    with ThreadPoolExecutor(max_workers=B) as pool:      # (the complex steps are calls into C that hold no lock: the draws side by side)
        steps = list(pool.map(lambda k: complex_step(case, k, series=series_ref(case)), range(B)))
    for k in range(B):
        c, d = draw_cd(C, Dd, k)
        tr = O.logl_grad_truth(A[k], Bc[k], c, d, t, y, s2, mu=mu[k], nu=nu[k], shift=None if shift is None else shift[k])
        for v in tr.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        truth.append(tr)
        refs = {"complex_step": steps[k], "dense_fp64": dense_fp64(case, k)}
        for name, ref in refs.items():
            for key in keys:
                if key in ref:
                    parts[name][key][k] = deviation(ref[key], tr, key)
    ref_dev = {key: np.fmax(parts["complex_step"][key], parts["dense_fp64"][key]) for key in keys}
    _reference[label] = (truth, ref_dev, parts)
    return _reference[label]


def wide_proto():
    spec = importlib.util.spec_from_file_location("wide_adjoint_dd_proto", ROOT / "tools" / "wide_adjoint_dd_proto.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_form_dev = {}


def wide_form_dev(case):
    """[B]: the deviation from the truth, in grad_d's scale, of d log L / d d_j evaluated in fp64 in the form of the step-by-step reverse mode
    (tools/wide_adjoint_dd_proto.py); computed once per label"""
    label, A, Bc, C, Dd = case[0], case[4], case[5], case[6], case[7]
    if label not in _form_dev:
        truth = reference(case)[0]
        P = wide_proto()
        out = []
        for k in range(len(A)):
            yc, sk, S, v = _series(case, k)
            got = P.wide_dd(A[k], Bc[k], *draw_cd(C, Dd, k), case[1], yc, sk, np.float64)[0]
            out.append(deviation(got, truth[k], "grad_d"))
        _form_dev[label] = np.array(out)
    return _form_dev[label]


def wide_bounds(case):
    """the bounds of the step-by-step reverse mode that differ from the common one: grad_d, from the form's own fp64 deviation"""
    ref_dev = reference(case)[1]
    return {"grad_d": np.maximum(MARGIN * np.maximum(ref_dev["grad_d"], wide_form_dev(case)), FLOOR)}


def bound_of(case, key, bounds=None):
    """[B]: max(MARGIN x ref_dev, FLOOR), or what `bounds` (wide_bounds) holds for the key"""
    if bounds is not None and key in bounds:
        return np.asarray(bounds[key])
    return np.maximum(MARGIN * reference(case)[1][key], FLOOR)


def structural_zeros(case):
    """[B][J] bool: the entries of grad_b and grad_d whose derivative is exactly zero (one-row terms: b_j = d_j = 0)"""
    A, Bc, Dd = case[4], case[5], case[7]
    return (Bc == 0.0) & (np.broadcast_to(Dd, A.shape) == 0.0)


def check(impl, case, keys=None, leg="", bounds=None):
    """impl(case) -> a dict as Dataset.logl_grad returns it (logl [B], status [B], grad_a .. grad_d [B][J], grad_mu, grad_nu [B], grad_y,
    grad_sigma2 [B][N], grad_shift [B]).  keys: the outputs to hold to the truth (default: all the case has).  bounds: wide_bounds(case) for the
    step-by-step reverse mode, else None.
    Every figure is printed before anything is asserted.  Returns the deviations, key -> [B]."""
    label, t, y, s2, A, Bc, C, Dd, mu, nu, shift = case
    truth, ref_dev, _ = reference(case)
    keys = keys_of(case) if keys is None else tuple(keys)
    got = impl(case)
    B, J, N = len(A), A.shape[1], len(t)
    shapes = {"logl": (B,), "grad_mu": (B,), "grad_nu": (B,), "grad_shift": (B,), "grad_y": (B, N), "grad_sigma2": (B, N)}
    dev, bound = {}, {}
    for key in keys:
        g = np.asarray(got[key])
        assert g.shape == shapes.get(key, (B, J)), (label, leg, key, g.shape)
        dev[key] = np.array([deviation(g[k], truth[k], key) for k in range(B)])
        bound[key] = bound_of(case, key, bounds)
        for k in range(B):
            print(f"{label} {leg} {key} draw {k}: deviation {dev[key][k]:.2e}   ref_dev {ref_dev[key][k]:.2e}   bound {bound[key][k]:.2e}")
    zero = structural_zeros(case)
    stray = {key: np.asarray(got[key])[zero] for key in ("grad_b", "grad_d") if key in keys}
    for key, v in stray.items():
        if v.size and not (v == 0.0).all():
            print(f"{label} {leg} {key} at one-row terms: {v[v != 0.0][:4]} (must be exactly 0)")
    assert (np.asarray(got["status"]) == 0).all(), (label, leg, got["status"])
    for key in keys:
        for k in range(B):
            assert dev[key][k] <= bound[key][k], (label, leg, key, k, dev[key][k], bound[key][k])
    for key, v in stray.items():
        assert (v == 0.0).all(), (label, leg, key, "a structurally zero entry is not exactly 0")
    return dev


# ---- the fp64 references as `impl`s -------------------------------------------------------------------------------------------------------
def reference_impl(which, series=True):
    """complex_step or dense_fp64 as an `impl` of check()"""
    def impl(case):
        B = len(case[4])
        per = [complex_step(case, k, series) if which == "complex_step" else dense_fp64(case, k) for k in range(B)]
        out = {key: np.array([p[key] for p in per]) for key in per[0]}
        out["status"] = np.zeros(B, dtype=np.int32)
        return out
    return impl
