"""Cases and checkers for the posterior draws at new times by Matheron's rule (pioran_celerite_rand_posterior: Dataset.rand_posterior behind
pj.rand_posterior(solver="celerite") and pj.ppc_timeseries), shared by the CPU tests (the numpy twin tools/rand_posterior_proto.py,
tests/test_rand_posterior_host.py) and the GPU tests (tests/test_gpu_rand_posterior.py).  A plain module, no fixtures.

cases()        shapes of predict_mean_cases.edge_cases() — every ROWS x N in {3, 17} and LENGTHS x R in {3, 33} with sigma2 as drawn, the
               PATTERN_SHAPES with every pattern of tau (before / after / on the data, tied, crowded at the 128- and 256-step edges) and both
               sigma2 variants, WIDE_ROWS x N in {2, 9} — with normals (q_data, q_new, eps) seeded per label; one shape whose merged grid crosses a
               16-step window while the data do not (N = 9, M = 9, no ties: P = 18); three shapes with a shift per draw (the data set then holds
               raw flux).  A shape enters only if the long-double Cholesky of its zero-noise kernel on the merged grid succeeds (EXCLUDED names
               the others, with the reason).
check()        an implementation against the truth, tau ascending and the same tau permuted.
affine_map()   the mean vector m and the matrix G of out = m + G (q_data | q_new | eps) of an implementation, from the zero vector and the
               2 N + M unit vectors; check_affine() holds m against predict_mean_truth and G G' against the dense long-double posterior
               covariance k** - k*' K^-1 k* on tau, singular blocks at tied times included.

The truth is dense in long double and shares nothing with the recurrences: f~ = oracle.sim_truth(.., T, 0, qT) on the merged grid (restated
here with numpy.unique), the correction oracle.predict_mean_truth on the residual series y - mu - f~(t) - sqrt(nu sigma2) eps.  Deviations
are taken in the scale of what is summed,
    max |got - truth| / max(max_n |y_n - mu|, max |f~|)         (affine map: m as the mean, G G' in units of k(0) = sum(a))
and the bound per case and draw is max(MARGIN x ref_dev, FLOOR) with MARGIN = 20 and FLOOR = 256 eps of tests/predict_var_cases.py, for the
reason given there and in tests/predict_mean_cases.py: the chain sums the same terms as the fp64 references in another order.  ref_dev is
the worst deviation, from the same truth on the same draw, of two fp64 compositions that are not the code under test:
    oracle.sim -> oracle.predict                                        (the C restatements of the reference's sim and pred)
    np.linalg.cholesky(dense) @ qT -> oracle.predict_direct_numpy       (dense; where LAPACK's fp64 Cholesky of the zero-noise kernel
                                                                         fails on a grid the long-double one factors, this reference is
                                                                         absent and the first stands alone)."""
import importlib.util
import sys
from pathlib import Path

import numpy as np

from oracle import oracle as O

sys.path.insert(0, str(Path(__file__).resolve().parent))
import predict_mean_cases as PM  # noqa: E402
from predict_var_cases import FLOOR, MARGIN, draw_cd  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]
CROSS16 = "R17-N9-cross16-s2x1"                              # N = 9, M = 9, no ties: P = 18
SHIFT_SHAPES = ("R5-N17-mixed-s2x1", "R33-N33-mixed-s2x1", "R65-N9-mixed-s2x1")
# candidate shapes the long-double Cholesky of the zero-noise kernel on the merged grid refuses: label -> reason (filled by cases())
EXCLUDED = {}


def proto():
    spec = importlib.util.spec_from_file_location("rand_posterior_proto", ROOT / "tools" / "rand_posterior_proto.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def merged(t, tau):
    """(T, origin, it, itau): sort(unique(t | tau)), the first occurrence of each merged time in (t | tau), the merged indices of t and tau"""
    T, origin, inverse = np.unique(np.concatenate([t, tau]), return_index=True, return_inverse=True)
    return T, origin, inverse[:len(t)], inverse[len(t):]


def candidate_labels():
    """the labels of predict_mean_cases.edge_cases() this module takes"""
    out = [f"R{R}-N{N}-mixed-s2x1" for R in PM.ROWS for N in (3, 17)]
    out += [f"R{R}-N{N}-mixed-s2x1" for N in PM.LENGTHS for R in (3, 33)]
    for R, N in PM.PATTERN_SHAPES:
        out += [f"R{R}-N{N}-{pat}-{tag}" for pat in PM.PATTERNS + (("segment_edges",) if N > 129 else ()) for tag, _ in PM.S2_VARIANTS]
    out += [f"R{R}-N{N}-mixed-s2x1" for R in PM.WIDE_ROWS for N in (2, 9)]
    return list(dict.fromkeys(out))


def _with_normals(case, shift=None, label=None):
    """(label, t, y, s2, A, Bc, C, Dd, mu, nu, tau, q_data, q_new, eps, shift) from a case of predict_mean_cases"""
    lab, t, y, s2, A, Bc, C, Dd, mu, nu, tau, _ = case
    label = label or lab
    rng = PM._rng(label + "/rand_posterior")
    B, N, M = len(A), len(t), len(tau)
    return (label, t, y, s2, A, Bc, C, Dd, mu, nu, tau, rng.standard_normal((B, N)), rng.standard_normal((B, M)), rng.standard_normal((B, N)), shift)


def _cross16():
    stem, t, s2, A, Bc, C, Dd, mu, nu, _, q = PM._shape(17, 9, "mixed", None)
    tau = PM._rng(CROSS16).uniform(t[0], t[-1], 9)
    assert len(np.unique(np.concatenate([t, tau]))) == 18
    return PM._case(CROSS16, t, s2, A, Bc, C, Dd, mu, nu, tau, q)


def _shifted(case):
    """the case on raw flux: y_raw = exp(y) + 1 with variances sigma2 exp(2 y), a shift c_b in (0.1, 0.9) per draw — the transformed series
    log(y_raw - c_b) and its variances stay of the size of the case's own"""
    lab, t, y, s2, A, Bc, C, Dd, mu, nu, tau, q = case
    label = lab + "-shift"
    c = PM._rng(label).uniform(0.1, 0.9, len(A))
    raw = (label, t, np.exp(y) + 1.0, s2 * np.exp(2.0 * y)) + tuple(case[4:])
    return _with_normals(raw, shift=c, label=label)


def _admit(case):
    """None, or why the zero-noise kernel of a draw has no long-double Cholesky factor on the merged grid"""
    label, t, y, s2, A, Bc, C, Dd, mu, nu, tau = case[:11]
    T = merged(t, tau)[0]
    for variant in (case, per_draw(case)):
        for k in range(len(A)):
            c, d = draw_cd(variant[6], variant[7], k)
            try:
                O.sim_truth(A[k], Bc[k], c, d, T, np.zeros(len(T)), np.zeros(len(T)))
            except np.linalg.LinAlgError as e:
                return f"draw {k}{' (per-draw (c, d))' if variant is not case else ''}: {e}"
    return None


_cases = []


def cases():
    """the admitted cases (built once)"""
    if not _cases:
        by_label = {c[0]: c for c in PM.edge_cases()}
        cand = [_with_normals(by_label[lab]) for lab in candidate_labels()]
        cand.append(_with_normals(_cross16()))
        cand += [_shifted(by_label[lab]) for lab in SHIFT_SHAPES]
        for c in cand:
            why = _admit(c)
            if why is None:
                _cases.append(c)
            else:
                EXCLUDED[c[0]] = why
    return list(_cases)


def n_candidates():
    return len(candidate_labels()) + 1 + len(SHIFT_SHAPES)


def per_draw(case):
    """the case with (c, d) of its own in every draw (predict_mean_cases.per_draw_variant)"""
    v = PM.per_draw_variant(case[:11] + (None,))
    return v[:11] + case[11:]


def orders(case):
    """(ascending tau, the same times permuted, the permutation): the normals q_new follow their times"""
    return PM.orders(case[:11] + (None,))


def rows(case):
    A, Dd = case[4], case[7]
    return 2 * A.shape[1] - int(np.sum(np.atleast_2d(Dd)[0] == 0.0))


def _series(case, k, dtype):
    """what draw k conditions on, in `dtype`: (y_k - mu_k, sigma2_k) — transformed first where the case has a shift"""
    label, t, y, s2, A, Bc, C, Dd, mu, nu = case[:10]
    shift = case[14]
    y, s2 = np.asarray(y, dtype=np.float64).astype(dtype), np.asarray(s2, dtype=np.float64).astype(dtype)
    if shift is not None:
        v = y - dtype(shift[k])
        y, s2 = np.log(v), s2 / (v * v)
    return y - dtype(mu[k]), s2


def _dense(a, b, c, d, x1, x2):
    dt = np.abs(x1[:, None] - x2[None, :])[..., None]
    return (np.exp(-c * dt) * (a * np.cos(d * dt) + b * np.sin(d * dt))).sum(-1)


_reference = {}


def _ordered(case):
    """the two askings of a case: (name, tau, q_new [B][M] in that order) with tau ascending and with the same times permuted.  Where times are
    tied the FIRST occurrence in the order asked gives the normal, so the two are different draws with truths of their own."""
    tau, q_new = case[10], case[12]
    asc, unsorted, perm = orders(case)
    o = np.argsort(tau, kind="stable")                       # asc = tau[o]
    return (("ascending", asc, np.ascontiguousarray(q_new[:, o])), ("permuted", unsorted, np.ascontiguousarray(q_new[:, o][:, perm])))


def truth_for(case, tt, qn):
    """(truth [B][M] in long double, without mu; scale [B]; ref_dev [B]) of the case's draws asked for at the times tt (any order) with the
    normals qn [B][M] of those times"""
    label, t, y, s2, A, Bc, C, Dd, mu, nu, tau, q_data, q_new, eps, shift = case
    LD = np.longdouble
    B = len(A)
    truths, scales, devs = [], np.zeros(B), np.zeros(B)
    T, origin, it, itau = merged(t, tt)
    o = np.argsort(tt, kind="stable")
    zero = np.zeros(len(T))
    for k in range(B):
        a, b = A[k], Bc[k]
        c, d = draw_cd(C, Dd, k)
        qT = np.concatenate([q_data[k], qn[k]])[origin]
        f = O.sim_truth(a, b, c, d, T, zero, qT)                                     # (raises unless positive definite)
        yk, sk = _series(case, k, LD)
        resid = yk - f[it] - np.sqrt(LD(nu[k]) * sk) * eps[k].astype(LD)
        hi = resid.astype(np.float64)
        lo = (resid - hi.astype(LD)).astype(np.float64)                             # predict_mean_truth takes fp64 values: two of them
        s2k = (LD(nu[k]) * sk).astype(np.float64)
        truth = f[itau] + O.predict_mean_truth(a, b, c, d, tt, t, hi, s2k) + O.predict_mean_truth(a, b, c, d, tt, t, lo, s2k)
        scales[k] = float(max(np.max(np.abs(yk)), np.max(np.abs(f))))
        # the two fp64 compositions
        y64, s64 = _series(case, k, np.float64)
        eta = np.sqrt(nu[k] * s64) * eps[k]
        f1 = O.sim(a, b, c, d, T, zero, qT)
        corr = np.empty(len(tt))
        corr[o] = O.predict(a, b, c, d, tt[o], t, y64 - f1[it] - eta, nu[k] * s64)
        refs = [f1[itau] + corr]
        try:
            f2 = np.linalg.cholesky(_dense(a, b, c, d, T, T)) @ qT
            refs.append(f2[itau] + O.predict_direct_numpy(a, b, c, d, tt, t, y64 - f2[it] - eta, nu[k] * s64))
        except np.linalg.LinAlgError:
            pass
        truths.append(truth)
        devs[k] = max(float(np.max(np.abs(r - truth))) for r in refs) / scales[k]
    return np.array(truths), scales, devs


def reference(case):
    """(truth [2][B][M] in long double, without mu, for tau ascending and permuted (_ordered); scale [B]; ref_dev [B], the worse of the two
    askings).  Computed once per label, never changed."""
    label = case[0]
    if label not in _reference:
        both = [truth_for(case, tt, qn) for name, tt, qn in _ordered(case)]
        truths = np.array([r[0] for r in both]); truths.setflags(write=False)
        _reference[label] = (truths, np.maximum(both[0][1], both[1][1]), np.maximum(both[0][2], both[1][2]))
    return _reference[label]


def check(impl, case, leg=""):
    """impl(case, tau, q_new) -> (out [B][M], status [B]) for the case's draws at the times tau with the normals q_new [B][M] of those times;
    called with tau ascending and with the same tau permuted.  Returns the deviations [2][B]."""
    label, t, y, s2, A, Bc, C, Dd, mu, nu, tau, q_data, q_new, eps, shift = case
    truth, scale, ref_dev = reference(case)
    bound = np.maximum(MARGIN * ref_dev, FLOOR)
    B = len(A)
    dev = np.full((2, B), np.inf)
    results = []
    for i, (name, tt, qn) in enumerate(_ordered(case)):
        got, status = impl(case, tt, qn)
        got = np.asarray(got)
        assert got.shape == (B, len(tau)), (label, name, got.shape)
        for k in range(B):
            if np.isfinite(got[k]).all():
                dev[i, k] = float(np.max(np.abs(got[k] - mu[k] - truth[i][k]))) / scale[k]
            print(f"{label} {leg} {name} draw {k}: deviation {dev[i, k]:.2e}   ref_dev {ref_dev[k]:.2e}   bound {bound[k]:.2e}")
        results.append((name, status))
    for name, status in results:
        assert (np.asarray(status) == 0).all(), (label, name, status)
    for i, name in enumerate(("ascending", "permuted")):
        for k in range(B):
            assert dev[i, k] <= bound[k], (label, leg, name, k, dev[i, k], bound[k])
    return dev


def proto_impl(**kw):
    """the prototype as an `impl` of check(); kw: its seeded mistakes"""
    P = proto()

    def impl(case, tau, q_new):
        label, t, y, s2, A, Bc, C, Dd, mu, nu = case[:10]
        shift = case[14]
        out = []
        for k in range(len(A)):
            if shift is None:
                r = P.rand_posterior(A[k], Bc[k], *draw_cd(C, Dd, k), t, y - mu[k], s2, tau, case[11][k], q_new[k], case[13][k], nu=nu[k], **kw)
            else:                                                   # (mu leaves the TRANSFORMED series)
                yt, st = P.transformed(y, s2, shift[k])
                r = P.rand_posterior(A[k], Bc[k], *draw_cd(C, Dd, k), t, yt - mu[k], st, tau, case[11][k], q_new[k], case[13][k], nu=nu[k], **kw)
            out.append(r + mu[k])
        return np.array(out), np.zeros(len(A), dtype=np.int32)
    return impl


# ---- the distribution, deterministically ----------------------------------------------------------------------------------------------
def affine_shape(R, N, M, on_data=0):
    """(label, t, y, s2, a, b, c, d, mu, nu, tau): ONE draw of a shape of predict_mean_cases with M evaluation times, `on_data` of them data
    times, the others distinct and off the data"""
    stem, t, s2, A, Bc, C, Dd, mu, nu, _, q = PM._shape(R, N, "mixed", None)
    label = f"affine-R{R}-N{N}-M{M}"
    rng = PM._rng(label)
    tau = np.concatenate([rng.choice(t, on_data, replace=False), rng.uniform(t[0] - 1.0, t[-1] + 1.0, M - on_data)])
    tau = rng.permutation(tau)
    y = PM.make_y(t, s2, A, Bc, C, Dd, nu, q[0])
    return (label, t, y, s2, A[0], Bc[0], C, Dd, float(mu[0]), float(nu[0]), tau)


def affine_inputs(shape):
    """the 2 N + M + 1 draws that read the affine map off: (q_data, q_new, eps) all zero, then each unit vector"""
    N, M = len(shape[1]), len(shape[10])
    Z = np.vstack([np.zeros((1, 2 * N + M)), np.eye(2 * N + M)])
    return np.ascontiguousarray(Z[:, :N]), np.ascontiguousarray(Z[:, N:N + M]), np.ascontiguousarray(Z[:, N + M:])


def affine_truth(shape):
    """(m [M] without mu, cov [M][M]) in long double: K* K^-1 (y - mu) and k** - k*' K^-1 k* with K = k(t, t) + diag(nu sigma2), dense"""
    label, t, y, s2, a, b, c, d, mu, nu, tau = shape
    LD = np.longdouble
    al, bl, cl, dl, tl, taul = (np.asarray(v, dtype=np.float64).astype(LD) for v in (a, b, c, d, t, tau))
    s2k = nu * s2
    L = O._truth_cholesky(al, bl, cl, dl, tl, s2k.astype(LD), LD)
    Ks = _dense(al, bl, cl, dl, taul, tl)
    w = np.zeros_like(Ks)
    for n in range(len(t)):                                 # rows: L^-1 k*(tau_m)
        w[:, n] = (Ks[:, n] - w[:, :n] @ L[n, :n]) / L[n, n]
    cov = _dense(al, bl, cl, dl, taul, taul) - w @ w.T
    return O.predict_mean_truth(a, b, c, d, tau, t, y - mu, s2k), cov


def affine_map(draws):
    """(m, G) from the 2 N + M + 1 draws of affine_inputs(), mu already subtracted"""
    draws = np.asarray(draws)
    return draws[0], (draws[1:] - draws[0]).T


def affine_references(shape):
    """the two fp64 compositions' draws [2 N + M + 1][M] on affine_inputs(), without mu"""
    label, t, y, s2, a, b, c, d, mu, nu, tau = shape
    P = proto()
    qd, qn, ep = affine_inputs(shape)
    dense_sim = lambda a, b, c, d, T, z, q: np.linalg.cholesky(_dense(a, b, c, d, T, T)) @ q
    direct = lambda a, b, c, d, tau, t, y, s2: O.predict_direct_numpy(a, b, c, d, tau, t, y, s2)
    out = []
    for sim, predict in ((None, None), (dense_sim, direct)):
        try:
            out.append(np.array([P.rand_posterior(a, b, c, d, t, y - mu, s2, tau, qd[i], qn[i], ep[i], nu=nu, sim=sim, predict=predict) for i in range(len(qd))]))
        except np.linalg.LinAlgError:
            pass
    return out


def check_affine(draws, shape, leg=""):
    """draws [2 N + M + 1][M] of an implementation on affine_inputs() (mu already subtracted) against affine_truth(): m in units of
    max |y - mu|, G G' in units of k(0); bound max(MARGIN x ref_dev, FLOOR) with ref_dev from affine_references().  Returns (dev_m, dev_cov)."""
    label, t, y, s2, a, b, c, d, mu, nu, tau = shape
    m_true, cov_true = affine_truth(shape)
    ys, k0 = float(np.max(np.abs(y - mu))), float(np.sum(a))

    def devs(dr):
        if not np.isfinite(dr).all():
            return np.inf, np.inf
        m, G = affine_map(dr)
        return float(np.max(np.abs(m - m_true))) / ys, float(np.max(np.abs(G @ G.T - cov_true))) / k0
    refs = [devs(r) for r in affine_references(shape)]
    bound_m = max(MARGIN * max(r[0] for r in refs), FLOOR)
    bound_c = max(MARGIN * max(r[1] for r in refs), FLOOR)
    dev_m, dev_c = devs(np.asarray(draws))
    print(f"{label} {leg} affine map: mean deviation {dev_m:.2e} (bound {bound_m:.2e})   covariance deviation {dev_c:.2e} k(0) (bound {bound_c:.2e})   "
          f"smallest eigenvalue of the true covariance / k(0) {float(np.linalg.eigvalsh(cov_true.astype(np.float64)).min()) / k0:.1e}")
    assert dev_m <= bound_m, (label, leg, "mean", dev_m, bound_m)
    assert dev_c <= bound_c, (label, leg, "covariance", dev_c, bound_c)
    return dev_m, dev_c, bound_m, bound_c
