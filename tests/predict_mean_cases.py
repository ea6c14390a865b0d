"""Cases and checkers for the posterior mean and the simulation, shared by the CPU tests (the numpy twin and the fp64 oracles,
tests/test_predict_mean_sim_host.py) and the GPU tests (Dataset.predict, Context.simulate, pj.rand: tests/test_gpu_predict_mean_sim.py).
A plain module, no fixtures; the draws, tau patterns and the style follow tests/predict_var_cases.py.

edge_cases()   the shapes at which the kernels of the two paths take another branch (celerite_predict.hip, celerite_block.hip,
               celerite_wide.hip): rows R on both sides of every multiple of 16 (RP = (R + 15) & ~15 of the tau factors, NB = (R + 16) / 16 of the
               windowed kernels) and of 64 and 128 (two / three rows per lane step by step); series of 1 .. 5, 8, 9 steps (the one-step-ahead
               fetch and the FD = 4 prefetch), around the KW = 16 window and around QSEG = 128 and 256 (one, two, three segments: only the
               third has a non-zero carry to multiply); evaluation times all before / all after / on the data / alone / forty in one gap /
               crowded around the segment edges; M around EVT = 8, 128 and 256 per block and on both sides of the M <= N R switch.  Each
               shape with sigma2 as drawn, x 1e-6 and (simulation only) exactly zero.
fuzz_cases()   seeded random shapes.
check_mean()   an implementation against oracle.predict_mean_truth, with tau ascending and with the same tau permuted (the fused and the
               two-pass evaluation of the windowed path).
check_sim()    an implementation against oracle.sim_truth.

The truths are dense in long double and share nothing with the recurrences.  Deviations are taken in the natural scale,
    mean          max |got - truth| / max_n |y_n - mu|
    simulation    max |got - truth| / max |truth|,
and the bound per case and draw is max(MARGIN x ref_dev, FLOOR).  ref_dev is the worst deviation, from the same truth on the same draw, of the
fp64 evaluations that are not the code under test: oracle.predict (the C restatement of the reference's pred), oracle.predict_direct_numpy
(dense) and tools/predict_mean_proto.py fed with an fp64 dense solve for z; oracle.sim and np.linalg.cholesky(K) @ q for the simulation.
MARGIN = 20 and FLOOR = 256 eps are those of tests/predict_var_cases.py and carry over for the reason given there: the kernels sum the
same terms as these fp64 evaluations in another order (window by window instead of step by step, a rotation tree instead of a running sum,
fma where numpy rounds twice), which moves the result by a few of the reference's own roundings but not by orders of magnitude; the
floor, 5.7e-14, is a dot product of at most 143 rows of terms of the size of the result on top of N steps of a recurrence, and keeps a
draw on which every reference happens to land on 1e-16 from failing on summation order alone."""
import importlib.util
import zlib
from pathlib import Path

import numpy as np

from oracle import oracle as O
from predict_var_cases import FLOOR, MARGIN, PATTERNS, _draws, draw_cd, make_tau

ROOT = Path(__file__).resolve().parents[1]

ROWS = (1, 2, 5, 6, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63)
LENGTHS = (1, 2, 3, 4, 5, 8, 9, 15, 16, 17, 31, 32, 33, 127, 128, 129, 255, 256, 257)
PATTERN_SHAPES = ((17, 5), (40, 129), (63, 257))
M_EDGES = (1, 7, 8, 9, 127, 128, 129, 255, 256, 257)
SWITCH_SHAPES = ((2, 2), (5, 3))                             # sorted tau with M = N R and N R + 1
WIDE_ROWS = (64, 65, 127, 128, 129, 143)
WIDE_LENGTHS = (1, 2, 5, 9)
S2_VARIANTS = (("s2x1", 1.0), ("s2x1e-6", 1e-6))             # the simulation adds sigma2 = 0: sim_variants()


def proto():
    spec = importlib.util.spec_from_file_location("predict_mean_proto", ROOT / "tools" / "predict_mean_proto.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _rng(label):
    return np.random.default_rng([20261018, zlib.crc32(label.encode())])


def segment_edges_tau(t, rng):
    """N > 129: five times in each of the gaps around the steps 127 | 128 and 255 | 256 (as far as the series has them), those data times
    themselves, one duplicate; unsorted"""
    N = len(t)
    parts = []
    for e in (128, 256):
        for g in (e - 2, e - 1, e):                       # gaps (t[g], t[g + 1])
            if g + 1 < N:
                parts.append(rng.uniform(t[g], t[g + 1], 5))
        parts.append(t[[n for n in (e - 1, e) if n < N]])
    tau = np.concatenate(parts)
    return rng.permutation(np.concatenate([tau, tau[:1]]))


def _tau(pattern, t, rng):
    return segment_edges_tau(t, rng) if pattern == "segment_edges" else make_tau(pattern, t, rng)


def _fill(tau, M, t, rng):
    """tau cut to M, or filled up with times anywhere around the data"""
    return tau[:M] if M <= len(tau) else np.concatenate([tau, rng.uniform(t[0] - 2.0, t[-1] + 2.0, M - len(tau))])


def edge_combinations():
    """(R, N, pattern, M or None), each once"""
    out = [(R, N, "mixed", None) for R in ROWS for N in (3, 17)]
    out += [(R, N, "mixed", None) for N in LENGTHS for R in (3, 33)]
    for R, N in PATTERN_SHAPES:
        out += [(R, N, pat, None) for pat in PATTERNS + (("segment_edges",) if N > 129 else ())]
    out += [(20, 40, "mixed", M) for M in M_EDGES]
    out += [(R, N, "mixed", N * R + k) for R, N in SWITCH_SHAPES for k in (0, 1)]
    out += [(R, N, "mixed", None) for R in WIDE_ROWS for N in WIDE_LENGTHS]
    return list(dict.fromkeys(out))


def _shape(R, N, pat, M):
    """One shape: (stem, t, s2, A, Bc, C, Dd, mu, nu, tau, q).  The draws are seeded by (R, N), so the patterns of one (R, N) share them (and the
    factorisations of their truths); tau and what hangs on it by the whole label."""
    stem = f"R{R}-N{N}-{pat}" + ("" if M is None else f"-M{M}")
    rng = _rng(f"R{R}-N{N}")
    B = 3 if N <= 129 else 2
    nreal = R % 2 + (2 * int(rng.integers(0, 2)) if 4 <= R <= 62 else 0)
    J = (R + nreal) // 2
    t, s2, A, Bc, C, Dd, nu = _draws(rng, N, J, B, np.arange(nreal))
    mu = rng.uniform(-1.0, 1.0, B)
    q = rng.standard_normal((B, N))
    rt = _rng(stem)
    tau = _tau(pat, t, rt)
    if M is not None:
        tau = _fill(tau, M, t, rt)
    return stem, t, s2, A, Bc, C, Dd, mu, nu, tau, q


def make_y(t, s2, A, Bc, C, Dd, nu, q):
    """A series the model can explain at this sigma2 (so that z = K^-1 (y - mu) stays of the size of y): a realisation of draw 0 in fp64 plus
    a constant"""
    c, d = draw_cd(C, Dd, 0)
    return O.sim(A[0], Bc[0], c, d, t, nu[0] * s2, q) + 0.3


def _case(label, t, s2, A, Bc, C, Dd, mu, nu, tau, q):
    y = make_y(t, s2, A, Bc, C, Dd, nu, q[0])
    return (label, t, y, s2, A, Bc, C, Dd, mu, nu, tau, q)


def edge_cases():
    """yields (label, t, y, s2, A, Bc, C, Dd, mu, nu, tau, q): B draws (3, or 2 where N > 129) with their own mu and nu and normals q [B][N];
    R = 2 J - (terms with d = 0) rows"""
    for R, N, pat, M in edge_combinations():
        stem, t, s2, A, Bc, C, Dd, mu, nu, tau, q = _shape(R, N, pat, M)
        for tag, scale in S2_VARIANTS:
            yield _case(f"{stem}-{tag}", t, s2 * scale, A, Bc, C, Dd, mu, nu, tau, q)


def sim_variants(case):
    """the simulation's cases of a mean case: itself, and for the `s2x1` variant the same shape with sigma2 exactly zero"""
    yield case
    label = case[0]
    if label.endswith("-s2x1") or "-s2x1-" in label:
        yield (label.replace("-s2x1", "-s2zero"), case[1], case[2], np.zeros_like(case[3])) + tuple(case[4:])


def fuzz_cases(n=40, seed=20261021):
    """yields n cases as edge_cases(): R in 1..64 with one-row terms at random places, N in 1..300 with occasional long gaps, M in 1..60 of a
    random pattern, 1..4 draws, (c, d) shared or per draw (half each), sigma2 scaled by 10^U(-7, 0)"""
    for i in range(n):
        rng = np.random.default_rng([seed, i])
        R = int(rng.integers(1, 65))
        nreal = R % 2 + 2 * int(rng.integers(0, min(R, 64 - R) // 2 + 1)) * int(rng.random() < 0.5)
        J = (R + nreal) // 2
        N = int(rng.integers(1, 301))
        B = int(rng.integers(1, 5))
        per_draw = i % 2 == 1
        one_row = rng.permutation(J)[:nreal]
        t, s2, A, Bc, C, Dd, nu = _draws(rng, N, J, B, one_row, per_draw, long_gaps=rng.random() < 0.3)
        pats = [p for p in PATTERNS + ("segment_edges",) if (N > 1 or p not in ("single_gap", "runs")) and (N > 129 or p != "segment_edges")]
        pat = pats[int(rng.integers(0, len(pats)))]
        tau = _tau(pat, t, rng)
        M = int(rng.integers(1, 61))                      # (`data`: M = N, `single_*`: M = 1)
        if pat == "mixed":
            tau = _fill(tau, M, t, rng)
        elif pat in ("before", "after", "runs", "segment_edges"):
            tau = np.resize(tau, M)
        scale = 10.0 ** rng.uniform(-7, 0)
        mu = rng.uniform(-1.0, 1.0, B)
        q = rng.standard_normal((B, N))
        kind = "perdraw" if per_draw else "shared"
        yield _case(f"fuzz{i}-R{R}-N{N}-M{len(tau)}-B{B}-{pat}-{kind}", t, s2 * scale, A, Bc, C, Dd, mu, nu, tau, q)


def per_draw_variant(case):
    """The case with (c, d) of its own in every draw: C, Dd tiled to [B][J], draw k with c x (1 + 0.05 k) and d x (1 - 0.03 k) (a term with
    d = 0 keeps its single row; |b| <= 0.9 a c / d still holds)."""
    label, t, y, s2, A, Bc, C, Dd, mu, nu, tau, q = case
    if np.ndim(C) == 2:
        return case
    k = np.arange(len(A))[:, None]
    C2 = np.tile(C, (len(A), 1)) * (1 + 0.05 * k)
    D2 = np.tile(Dd, (len(A), 1)) * (1 - 0.03 * k)
    return (label + "-cd_per_draw", t, y, s2, A, Bc, C2, D2, mu, nu, tau, q)


def orders(case):
    """(ascending tau, the same times permuted and not ascending where M allows, the permutation)"""
    tau = case[10]
    asc = np.sort(tau)
    perm = _rng(case[0] + "/perm").permutation(len(tau))
    if np.all(np.diff(asc[perm]) >= 0):
        perm = perm[::-1].copy()
    return asc, asc[perm], perm


_dense_cache, _z_cache = {}, {}


def _memo(cache, limit, arrays, make):
    key = tuple(np.ascontiguousarray(v, dtype=np.float64).tobytes() for v in arrays)
    if key not in cache:
        while len(cache) >= limit:
            cache.pop(next(iter(cache)))
        cache[key] = make()
        cache[key].setflags(write=False)
    return cache[key]


def _dense(a, b, c, d, t, s2):
    """K = k(|t_i - t_j|) + diag(s2) in fp64 (the last few are kept: the legs and seeded mistakes of a case ask for the same matrix)"""
    def make():
        dt = np.abs(t[:, None] - t[None, :])[..., None]
        return (np.exp(-c * dt) * (a * np.cos(d * dt) + b * np.sin(d * dt))).sum(-1) + np.diag(s2)
    return _memo(_dense_cache, 16, (a, b, c, d, t, s2), make)


def twin_mean(a, b, c, d, tau, t, y, s2, **kw):
    """the twin fed with an fp64 dense solve for z; zero-mean"""
    z = _memo(_z_cache, 64, (a, b, c, d, t, s2, y), lambda: np.linalg.solve(_dense(a, b, c, d, t, s2), y))
    return proto().predict_mean(a, b, c, d, t, z, tau, **kw)


_reference = {}


def reference(case, what):
    """what = "mean": (truth [B][M] for ASCENDING tau, in long double, without mu; ref_dev [B]); what = "sim": (truth [B][N], ref_dev [B]).
    Computed once per label, never changed afterwards.  The simulation's sigma2 is the case's s2 itself (one series for all draws)."""
    label, t, y, s2, A, Bc, C, Dd, mu, nu, tau, q = case
    if (label, what) in _reference:
        return _reference[label, what]
    truths, devs = [], []
    for k in range(len(A)):
        c, d = draw_cd(C, Dd, k)
        a, b = A[k], Bc[k]
        if what == "mean":
            asc, unsorted, perm = orders(case)
            yk, sk = y - mu[k], nu[k] * s2
            truth = O.predict_mean_truth(a, b, c, d, asc, t, yk, sk)          # (raises unless positive definite)
            scale = float(np.max(np.abs(yk)))
            refs = [O.predict(a, b, c, d, asc, t, yk, sk), O.predict_direct_numpy(a, b, c, d, asc, t, yk, sk),
                    twin_mean(a, b, c, d, asc, t, yk, sk), twin_mean(a, b, c, d, unsorted, t, yk, sk)[np.argsort(perm)]]
        else:
            truth = O.sim_truth(a, b, c, d, t, s2, q[k])
            scale = float(np.max(np.abs(truth)))
            refs = [O.sim(a, b, c, d, t, s2, q[k]), np.linalg.cholesky(_dense(a, b, c, d, t, s2)) @ q[k]]
        truths.append(truth)
        devs.append(max(float(np.max(np.abs(r - truth))) for r in refs) / scale)
    truths = np.array(truths); truths.setflags(write=False)
    _reference[label, what] = (truths, np.array(devs))
    return _reference[label, what]


def check_mean(impl, case, leg=""):
    """impl(A, Bc, C, Dd, t, y, s2, mu, nu, tau) -> (mean [B][M], status [B]); called with tau ascending and with the same tau permuted.
    Returns the deviations [2][B] (ascending, permuted) in units of max |y - mu|."""
    label, t, y, s2, A, Bc, C, Dd, mu, nu, tau, q = case
    truth, ref_dev = reference(case, "mean")
    asc, unsorted, perm = orders(case)
    bound = np.maximum(MARGIN * ref_dev, FLOOR)
    B = len(A)
    dev = np.zeros((2, B))
    results = []
    for i, (name, tt, want) in enumerate((("ascending", asc, truth), ("permuted", unsorted, truth[:, perm]))):
        got, status = impl(A, Bc, C, Dd, t, y, s2, mu, nu, tt)
        got = np.asarray(got)
        assert got.shape == (B, len(tau)), (label, name, got.shape)
        for k in range(B):
            dev[i, k] = float(np.max(np.abs(got[k] - mu[k] - want[k]))) / np.max(np.abs(y - mu[k]))
            print(f"{label} {leg} mean {name} draw {k}: deviation {dev[i, k]:.2e}   ref_dev {ref_dev[k]:.2e}   bound {bound[k]:.2e}")
        results.append((name, status))
    for name, status in results:
        assert (np.asarray(status) == 0).all(), (label, name, status)
    for i, name in enumerate(("ascending", "permuted")):
        for k in range(B):
            assert dev[i, k] <= bound[k], (label, leg, name, k, dev[i, k], bound[k])
    return dev


def check_sim(impl, case, leg=""):
    """impl(A, Bc, C, Dd, t, s2, q) -> (y [B][N], status [B]).  Returns the deviations [B] in units of max |truth|."""
    label, t, y, s2, A, Bc, C, Dd, mu, nu, tau, q = case
    truth, ref_dev = reference(case, "sim")
    bound = np.maximum(MARGIN * ref_dev, FLOOR)
    got, status = impl(A, Bc, C, Dd, t, s2, q)
    got = np.asarray(got)
    B = len(A)
    assert got.shape == (B, len(t)), (label, got.shape)
    dev = np.array([float(np.max(np.abs(got[k] - truth[k])) / np.max(np.abs(truth[k]))) for k in range(B)])
    for k in range(B):
        print(f"{label} {leg} sim draw {k}: deviation {dev[k]:.2e}   ref_dev {ref_dev[k]:.2e}   bound {bound[k]:.2e}")
    assert (np.asarray(status) == 0).all(), (label, status)
    for k in range(B):
        assert dev[k] <= bound[k], (label, leg, k, dev[k], bound[k])
    return dev


# ---- the fp64 evaluations as `impl`s --------------------------------------------------------------------------------------------------
def _each_mean(f):
    def impl(A, Bc, C, Dd, t, y, s2, mu, nu, tau):
        out = np.array([f(A[k], Bc[k], *draw_cd(C, Dd, k), tau, t, y - mu[k], nu[k] * s2) + mu[k] for k in range(len(A))])
        return out, np.zeros(len(A), dtype=np.int32)
    return impl


def twin_impl(**kw):
    """the twin as an `impl` of check_mean(); kw: its seeded mistakes"""
    return _each_mean(lambda *a: twin_mean(*a, **kw))


def oracle_predict_impl():
    """oracle.predict wants tau ascending: sort, evaluate, undo"""
    def f(a, b, c, d, tau, t, y, s2):
        o = np.argsort(tau, kind="stable")
        out = np.empty(len(tau))
        out[o] = O.predict(a, b, c, d, tau[o], t, y, s2)
        return out
    return _each_mean(f)


def direct_impl():
    return _each_mean(O.predict_direct_numpy)


def _each_sim(f):
    def impl(A, Bc, C, Dd, t, s2, q):
        out = np.array([f(A[k], Bc[k], *draw_cd(C, Dd, k), t, s2, q[k]) for k in range(len(A))])
        return out, np.zeros(len(A), dtype=np.int32)
    return impl


def oracle_sim_impl():
    return _each_sim(O.sim)


def dense_sim_impl():
    return _each_sim(lambda a, b, c, d, t, s2, q: np.linalg.cholesky(_dense(a, b, c, d, t, s2)) @ q)
