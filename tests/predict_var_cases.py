"""Cases and checker for the posterior variance through the celerite factorisation, shared by the CPU tests (the numpy prototype,
tests/test_predict_var_host.py) and the GPU tests (Dataset.predict_var, tests/test_gpu_predict_var.py).  A plain module, no fixtures.

edge_cases()   the shapes at which predict_var_fwd_kernel<H> / predict_var_bwd_kernel<H> take another path: rows R on both sides of every
               H = (R + 15) & ~15, series shorter than / equal to / just longer than the VD = 4 steps both kernels prefetch, and evaluation
               times that are all before, all after, exactly on, or crowded into one gap of the data.  Each shape with sigma2 as drawn and
               with sigma2 x 1e-6 (small posterior variances).
fuzz_cases()   seeded random shapes.
check()        an implementation against oracle.predict_var_truth in long double (dense, shares nothing with the recurrences).

The bound of check() is max(20 x proto_dev, 256 eps) k(0): proto_dev is the deviation of tools/predict_var_proto.py from the same truth on
the same draw (fp64 recurrences in the plainest summation order), 20 the margin tests/test_predict_var_host.py gives the prototype's
measured figure (the kernels sum in another order: four chains per dot product, a rotation tree, four row sums); the floor, 5.7e-14, is three
nested dot products of at most 64 terms of the size of k(0) and the final difference, and keeps a draw on which the prototype happens to land
on 1e-16 from failing on summation order alone."""
import importlib.util
from pathlib import Path

import numpy as np

from oracle import oracle as O

ROOT = Path(__file__).resolve().parents[1]
FLOOR = 256 * np.finfo(float).eps
MARGIN = 20

ROWS = (1, 2, 3, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64)
LENGTHS = (1, 2, 3, 4, 5, 7, 8, 9, 33)
PATTERNS = ("mixed", "before", "after", "data", "single_before", "single_first", "single_gap", "single_last", "single_after", "runs")


def proto():
    spec = importlib.util.spec_from_file_location("predict_var_proto", ROOT / "tools" / "predict_var_proto.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def make_tau(pattern, t, rng):
    N = len(t)
    span = max(t[-1] - t[0], 1.0)
    before = lambda k: t[0] - rng.uniform(0.01, 0.3, k) * span
    after = lambda k: t[-1] + rng.uniform(0.01, 0.3, k) * span
    gap = N // 2 - 1                                      # the gap (t[gap], t[gap + 1]) for the patterns that need one (N >= 2)
    if pattern == "mixed":                                # inside, outside on both sides, exact data times, duplicates; unsorted
        inner = rng.uniform(t[0], t[-1], 6)
        data = rng.choice(t, min(N, 4), replace=False)
        tau = np.concatenate([inner, before(2), after(2), data, inner[:1], data[:1]])
        return rng.permutation(tau)
    if pattern == "before":
        b = before(6)
        return np.concatenate([b, b[:1]])
    if pattern == "after":
        a = after(6)
        return np.concatenate([a, a[:1]])
    if pattern == "data":
        return t.copy()
    if pattern == "single_before":
        return before(1)
    if pattern == "single_first":
        return t[:1].copy()
    if pattern == "single_gap":
        return rng.uniform(t[gap], t[gap + 1], 1)
    if pattern == "single_last":
        return t[-1:].copy()
    if pattern == "single_after":
        return after(1)
    if pattern == "runs":                                 # 40 times inside one gap and none in the others
        return rng.permutation(rng.uniform(t[gap], t[gap + 1], 40))
    raise ValueError(pattern)


def _draws(rng, N, J, B, one_row, per_draw=False, long_gaps=False):
    """Inputs in the style of test_gpu_parity._random_case; one_row: the terms with b = d = 0 (one row each).  |b| is capped at 0.9 a c / d:
    every term is then a covariance of its own and K is positive definite whatever sigma2 > 0."""
    gaps = rng.uniform(0.05, 2.0, N)
    if long_gaps:
        gaps[rng.integers(0, N, max(1, N // 20))] *= rng.uniform(5, 400)
    t = np.cumsum(gaps)
    s2 = rng.uniform(0.01, 0.1, N)
    A = rng.uniform(0.1, 2.0, (B, J))
    Bc = rng.uniform(-0.05, 0.05, (B, J)) * A
    shape = (B, J) if per_draw else (J,)
    C = rng.uniform(0.05, 2.0, shape)
    Dd = rng.uniform(0.0, 3.0, shape)
    Dd[..., one_row] = 0.0
    Bc = np.sign(Bc) * np.minimum(np.abs(Bc), 0.9 * A * C / np.maximum(Dd, 1e-300))
    Bc[:, one_row] = 0.0
    nu = rng.uniform(0.5, 2.0, B)
    return t, s2, A, Bc, C, Dd, nu


def edge_combinations():
    """(R, N, pattern): every R with N = 3 and 9, every N with R = 3 and 33 (all `mixed`), every pattern at (17, 5) and (64, 33)"""
    out = [(R, N, "mixed") for R in ROWS for N in (3, 9)]
    out += [(R, N, "mixed") for N in LENGTHS for R in (3, 33) if N not in (3, 9)]
    out += [(R, N, pat) for (R, N) in ((17, 5), (64, 33)) for pat in PATTERNS]
    return out


def edge_cases():
    """yields (label, t, s2, A, Bc, C, Dd, nu, tau); B = 3 draws with their own nu, R = 2 J - nreal rows"""
    for i, (R, N, pat) in enumerate(edge_combinations()):
        rng = np.random.default_rng([20261018, i])
        nreal = R % 2 + (2 * int(rng.integers(0, 2)) if 4 <= R <= 62 else 0)
        J = (R + nreal) // 2
        t, s2, A, Bc, C, Dd, nu = _draws(rng, N, J, 3, np.arange(nreal))
        tau = make_tau(pat, t, rng)
        for scale, tag in ((1.0, "s2x1"), (1e-6, "s2x1e-6")):
            yield (f"R{R}-N{N}-{pat}-{tag}", t, s2 * scale, A, Bc, C, Dd, nu, tau)


def fuzz_cases(n=40, seed=20261019):
    """yields n cases as edge_cases(): R in 1..64 with one-row terms at random places, N in 1..120 with occasional long gaps, M in 1..60 of a
    random pattern, 1..4 draws, (c, d) shared or per draw (half each), sigma2 scaled by 10^U(-7, 0)"""
    for i in range(n):
        rng = np.random.default_rng([seed, i])
        R = int(rng.integers(1, 65))
        nreal = R % 2 + 2 * int(rng.integers(0, min(R, 64 - R) // 2 + 1)) * int(rng.random() < 0.5)
        J = (R + nreal) // 2
        N = int(rng.integers(1, 121))
        B = int(rng.integers(1, 5))
        per_draw = i % 2 == 1
        one_row = rng.permutation(J)[:nreal]
        t, s2, A, Bc, C, Dd, nu = _draws(rng, N, J, B, one_row, per_draw, long_gaps=rng.random() < 0.3)
        pats = [p for p in PATTERNS if N > 1 or p not in ("single_gap", "runs")]
        pat = pats[int(rng.integers(0, len(pats)))]
        tau = make_tau(pat, t, rng)
        M = int(rng.integers(1, 61))                      # (`data`: M = N, `single_*`: M = 1)
        if pat == "mixed":                                # cut, or filled up with times anywhere around the data
            tau = tau[:M] if M <= len(tau) else np.concatenate([tau, rng.uniform(t[0] - 2.0, t[-1] + 2.0, M - len(tau))])
        elif pat in ("before", "after", "runs"):          # cut, or repeated
            tau = np.resize(tau, M)
        scale = 10.0 ** rng.uniform(-7, 0)
        kind = "perdraw" if per_draw else "shared"
        yield (f"fuzz{i}-R{R}-N{N}-M{len(tau)}-B{B}-{pat}-{kind}", t, s2 * scale, A, Bc, C, Dd, nu, tau)


def fixture_draws(golden_dir):
    """The nine ill-conditioned draws of tests/golden/predict_var_truth.npz (oracle/make_predict_var_truth.py): a list of
    (label, a, b, c, d, t, s2, tau, truth in long double, ratio); N = 150: 50-digit truth, N = 1000: long-double truth."""
    Q = np.load(golden_dir / "quad_truth.npz")
    F = np.load(golden_dir / "predict_var_truth.npz")
    out = []
    for tag in ("n150", "n1000"):
        t, yerr, tau = Q[f"{tag}_t"], Q[f"{tag}_yerr"], F[f"{tag}_tau"]
        for k, i in enumerate(F[f"{tag}_idx"]):
            truth = F[f"{tag}_truth_hi"][k].astype(np.longdouble) + F[f"{tag}_truth_lo"][k].astype(np.longdouble)
            out.append((f"{tag} draw {i}", Q[f"{tag}_A"][i], Q[f"{tag}_Bc"][i], Q[f"{tag}_C"], Q[f"{tag}_Dd"], t, Q[f"{tag}_nu"][i] * yerr ** 2, tau, truth,
                        float(Q[f"{tag}_ratio"][i])))
    return out


def draw_cd(C, Dd, k):
    return (C[k], Dd[k]) if np.ndim(C) == 2 else (C, Dd)


_reference = {}


def reference(case):
    """(truth [B][M] in long double, proto_dev [B]) of a case: computed once per label, never changed afterwards"""
    label, t, s2, A, Bc, C, Dd, nu, tau = case
    if label not in _reference:
        P = proto()
        truth, dev = [], []
        for k in range(len(A)):
            c, d = draw_cd(C, Dd, k)
            truth.append(O.predict_var_truth(A[k], Bc[k], c, d, tau, t, nu[k] * s2))      # (raises unless positive definite)
            got = P.predict_var(A[k], Bc[k], c, d, t, nu[k] * s2, tau)
            dev.append(float(np.max(np.abs(got - truth[-1])) / A[k].sum()))
        truth = np.array(truth); truth.setflags(write=False)
        _reference[label] = (truth, np.array(dev))
    return _reference[label]


def proto_impl(**kw):
    """the prototype as an `impl` of check(); kw: its seeded mistakes"""
    P = proto()
    def impl(A, Bc, C, Dd, t, s2, nu, tau):
        out = np.array([P.predict_var(A[k], Bc[k], *draw_cd(C, Dd, k), t, nu[k] * s2, tau, **kw) for k in range(len(A))])
        return out, np.zeros(len(A), dtype=np.int32)
    return impl


def check(impl, case):
    """impl(A, Bc, C, Dd, t, s2, nu, tau) -> (var [B][M], status [B]).  Returns the deviations [B] in units of k(0)."""
    label, t, s2, A, Bc, C, Dd, nu, tau = case
    truth, proto_dev = reference(case)
    var, status = impl(A, Bc, C, Dd, t, s2, nu, tau)
    var = np.asarray(var)
    assert var.shape == (len(A), len(tau)), (label, var.shape)
    k0 = A.sum(axis=1)
    dev = np.array([float(np.max(np.abs(var[k] - truth[k]))) / k0[k] for k in range(len(A))])
    bound = np.maximum(MARGIN * proto_dev, FLOOR)
    for k in range(len(A)):
        print(f"{label} draw {k}: deviation {dev[k]:.2e} k(0)   prototype {proto_dev[k]:.2e}   bound {bound[k]:.2e}   "
              f"min var / k(0) {float(truth[k].min()) / k0[k]:.2e}")
    assert (np.asarray(status) == 0).all(), (label, status)
    at = np.searchsorted(t, tau)
    at = np.where(at < len(t), at, 0)
    on_data = t[at] == tau
    for k in range(len(A)):
        assert dev[k] <= bound[k], (label, k, dev[k], bound[k])
        slack = bound[k] * k0[k]
        v = var[k][on_data]
        assert (v >= -slack).all() and (v <= nu[k] * s2[at[on_data]] + slack).all(), (label, k, "variance at a data time")
        assert (var[k] <= k0[k] * (1 + 1e-12)).all(), (label, k, "variance above k(0)")
    return dev
