"""CPU tests (-m "not gpu") of what the dense solver's GPU tests (tests/test_gpu_dense_truth.py) stand on: the long-double truths
oracle.dense_nll_truth and oracle.predict_cov_truth against the other truths of the oracle, the fixture tests/golden/dense_truth.npz
against its generator (oracle/make_dense_truth.py) and the leave-one-out condition on every stored draw, and the checkers of
tests/dense_cases.py on the numpy prototype of the device's arithmetic (tools/dense_proto.py): the prototype as it is must pass every case,
each of its seeded mistakes must fail at least one.

Measured here (the prototype, in units of ref_dev): sorted / unsorted `hard` cases at most 2.3; `repeat`-`hard` cases median 1.0 with a
heavy tail (two of the 26 first draws above 20 — with substitution in place of the explicit inverses 26.1 and 15.1 — and drawn again by
dense_cases._qualifies, which see)."""
import importlib.util
import sys
from pathlib import Path

import numpy as np
import pytest

from oracle import oracle as O

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(Path(__file__).resolve().parent))
import dense_cases as DC  # noqa: E402

LD_EPS = float(np.finfo(np.longdouble).eps)


def _generator():
    spec = importlib.util.spec_from_file_location("make_dense_truth", ROOT / "oracle" / "make_dense_truth.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _draw(N, J, seed):
    rng = np.random.default_rng([DC.SEED, 4000 + seed])
    t, s2, A, Bc, C, Dd, _ = DC._draws(rng, N, J, 1, np.arange(0))
    return A[0], Bc[0], C, Dd, t, rng.standard_normal(N), s2


# ---- the truths against each other ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 65, 193])
def test_nll_truth_against_the_gradient_truth(N):
    """dense_nll_truth == -logl_grad_truth()["logl"] (the same Cholesky, K^-1 formed another way) to long-double rounding of the scale; the
    scale is at least |nll|; an unsorted series gives the same value."""
    a, b, c, d, t, y, s2 = _draw(N, 5, N)
    nll, scale = O.dense_nll_truth(a, b, c, d, t, y, s2)
    assert nll.dtype == np.longdouble and scale >= abs(nll)
    other = -O.logl_grad_truth(a, b, c, d, t, y, s2)["logl"]
    assert abs(nll - other) <= 64 * N * LD_EPS * scale, (float(nll), float(other))
    p = np.random.default_rng(N).permutation(N)
    assert abs(O.dense_nll_truth(a, b, c, d, t[p], y[p], s2[p])[0] - nll) <= 64 * N * LD_EPS * scale


@pytest.mark.parametrize("N", [193, 321, 600])
def test_nll_truth_against_the_quad_precision_recurrence(N):
    """dense in long double against the celerite recurrence in __float128 (oracle.logl_quad, rounded to fp64): equal to the last bit of fp64
    on well-conditioned draws (one ulp allowed for the rounding of either)."""
    a, b, c, d, t, y, s2 = _draw(N, 5, N)
    nll, _ = O.dense_nll_truth(a, b, c, d, t, y, s2)
    quad = -O.logl_quad(a, b, c, d, t, y, s2)
    print(f"N = {N}: long double {float(nll)!r}   quad {quad!r}")
    assert abs(float(nll) - quad) <= np.spacing(abs(quad))


def test_nll_truth_names_the_first_bad_row():
    a, b, c, d, t, y, s2 = _draw(70, 5, 7)
    for bad in (0, 17, 69):
        s2b = s2.copy(); s2b[bad] = -50.0
        with pytest.raises(np.linalg.LinAlgError, match=f"at row {bad}$"):
            O.dense_nll_truth(a, b, c, d, t, y, s2b)


@pytest.mark.parametrize("N,M", [(1, 1), (65, 16), (130, 70)])
def test_cov_truth_against_the_variance_truth(N, M):
    a, b, c, d, t, y, s2 = _draw(N, 5, 10 + N)
    rng = np.random.default_rng(N)
    tau = DC.make_tau("mixed", t, rng)
    tau = tau[:M] if M <= len(tau) else np.concatenate([tau, rng.uniform(t[0] - 2.0, t[-1] + 2.0, M - len(tau))])
    cov = O.predict_cov_truth(a, b, c, d, tau, t, s2)
    assert cov.shape == (M, M) and cov.dtype == np.longdouble and np.array_equal(cov, cov.T)
    var = O.predict_var_truth(a, b, c, d, tau, t, s2)
    assert np.max(np.abs(np.diag(cov) - var)) <= 16 * max(N, 4) * LD_EPS * a.sum()
    ref = O.predict_cov_numpy(a, b, c, d, tau, t, s2)
    assert np.max(np.abs(ref - cov)) <= 1e-12 * a.sum()


# ---- the fixture ------------------------------------------------------------------------------------------------------------------------
def test_fixture_in_sync_with_its_generator(golden_dir):
    """The stored selection and truths are the generator's; the references of 8 draws of n150 and 2 of n1000 recomputed here lie within the
    bound their draw sets, max(MARGIN x the stored worst deviation, FLOOR), of the stored truth: LAPACK and the OpenMP sums of the C
    restatement round otherwise with another thread count (measured here: by as much as the stored deviation itself), so a recomputed
    reference is one more correct evaluation of the same draw, held as the device is; inputs that went out of step would miss by orders."""
    G = _generator()
    Q = np.load(golden_dir / "quad_truth.npz")
    F = np.load(golden_dir / "dense_truth.npz")
    assert tuple(F["refs"]) == G.REFS and tuple(F["refs_long"]) == G.REFS_LONG and tuple(F["long_N"]) == G.LONG_N
    assert np.array_equal(F["n150_idx"], np.arange(325)) and np.array_equal(F["n1000_idx"], G.pick_n1000(Q["n1000_ratio"]))
    assert len(F["n1000_idx"]) == 48 == len(set(F["n1000_idx"].tolist()))
    assert F["long_idx"].shape == (4, 4) and F["long_ref_dev"].shape == (4, 4, 4)
    for tag, picks in (("n150", (0, 47, 101, 150, 199, 250, 300, 324)), ("n1000", (0, 30))):
        t, y, yerr = G.series(Q, tag)
        assert np.array_equal(F[f"{tag}_truth"], -Q[f"{tag}_truth"][F[f"{tag}_idx"]])
        assert np.array_equal(F[f"{tag}_ref_dev"], np.abs(F[f"{tag}_ref"] - F[f"{tag}_truth"][:, None]) / np.abs(F[f"{tag}_truth"][:, None]))
        for k in picks:
            args = G.draw_args(Q, tag, F[f"{tag}_idx"][k], t, y, yerr)
            truth, tol = F[f"{tag}_truth"][k], max(DC.MARGIN * F[f"{tag}_ref_dev"][k].max(), DC.FLOOR)
            for r, name in enumerate(G.REFS):
                got = G.reference(name, *args)
                assert abs(got - truth) <= tol * abs(truth), (tag, k, name, got, F[f"{tag}_ref"][k, r])
    order = np.argsort(Q["n10000_ratio"], kind="stable")
    for k in range(4):                                   # `long`: the four lowest ratios, at most one replaced by the next
        assert len(set(F["long_idx"][k].tolist()) - set(order[:4].tolist())) <= 1 and set(F["long_idx"][k].tolist()) <= set(order[:5].tolist())
    assert np.array_equal(F["long_ref_dev"], np.abs(F["long_ref"] - F["long_truth"][..., None]) / np.abs(F["long_truth"][..., None]))


def test_fixture_long_truth_recomputed(golden_dir):
    """one draw of the `long` set: the truth (oracle.logl_quad on the prefix) exactly, the LAPACK references as above"""
    G = _generator()
    Q = np.load(golden_dir / "quad_truth.npz")
    F = np.load(golden_dir / "dense_truth.npz")
    t, y, yerr = G.series(Q, "n10000")
    N = int(F["long_N"][0])
    args = G.draw_args(Q, "n10000", F["long_idx"][0][1], t[:N], y[:N], yerr[:N])
    assert -O.logl_quad(*args) == F["long_truth"][0][1]
    tol = max(DC.MARGIN * F["long_ref_dev"][0][1].max(), DC.FLOOR) * abs(F["long_truth"][0][1])
    for r in (0, 2):
        assert abs(G.reference(G.REFS_LONG[r], *args) - F["long_truth"][0][1]) <= tol


def test_leave_one_out_on_every_stored_draw(golden_dir):
    """Each of the four references within MARGIN of the worst of the other three, after the floor: the stored draws are inputs on which fp64
    evaluations that are correct agree on the size of the error, so 20 x the worst of them is a bound a correct kernel can meet."""
    F = np.load(golden_dir / "dense_truth.npz")
    for tag in ("n150", "n1000", "long"):
        dev = F[f"{tag}_ref_dev"].reshape(-1, 4)
        worst = max(float(dev[k, r] / max(np.delete(dev[k], r).max(), DC.FLOOR / DC.MARGIN)) for k in range(len(dev)) for r in range(4))
        print(f"{tag}: {len(dev)} draws, worst reference deviation median {np.median(dev.max(axis=1)):.2e} max {dev.max():.2e}; a reference at most {worst:.1f} x the "
              f"worst of the other three")
        assert DC.leave_one_out(dev).all(), (tag, np.flatnonzero(~DC.leave_one_out(dev)))
    assert np.isfinite(F["n150_ref"]).all() and np.isfinite(F["n1000_ref"]).all() and np.isfinite(F["long_ref"]).all()


# ---- the cases and the checkers ---------------------------------------------------------------------------------------------------------
def test_case_lists_cover_what_they_promise():
    shapes = DC.nll_edge_shapes()
    assert len(set(shapes)) == len(shapes) == 27
    assert {(N, 5) for N in (1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 191, 192, 193, 256, 257, 320)} <= set(shapes)
    assert {(N, J) for N in (65, 193) for J in (1, 20, 61, 64, 65)} <= set(shapes)
    cases = list(DC.nll_edge_cases([(65, 5), (1, 5)]))
    assert len(cases) == 8
    for label, a, b, c, d, t, y, s2 in cases[:6]:
        order = label.split("-")[2]
        assert (np.diff(t) >= 0).all() == (order != "unsorted"), label
        assert ((t[6] == t[5]) and (t[64] == t[63])) == (order == "repeat"), label
    kinds = {(k, B, N, o) for k, B, N, o in DC.BATCH_SHAPES}
    assert {("shared", 3, 70, "sorted"), ("shared", 17, 70, "sorted"), ("shared", 33, 70, "sorted"), ("perdraw", 3, 70, "sorted"),
            ("perdraw", 3, 193, "sorted"), ("shared", 5, 193, "unsorted")} == kinds
    assert len(list(DC.nll_batch_cases())) == 12
    ps = DC.predict_shapes()
    assert {(N, 65) for N in DC.PREDICT_N} | {(65, M) for M in DC.PREDICT_M} | {(1, 1), (64, 64), (128, 64), (64, 129)} <= {(N, M) for N, M, _, _ in ps}
    assert {pat for N, M, pat, J in ps if N == 65} == set(DC.PATTERNS) and (65, 65, "mixed", 20) in ps
    for label, a, b, c, d, t, y, s2, tau in DC.predict_cases():
        N, M = int(label.split("-")[0][1:]), int(label.split("-")[1][1:])
        assert len(t) == N and len(tau) == M, label
    assert [c[-1] for c in DC.status_cases()] == [0, 63, 64, 100]


@pytest.mark.parametrize("N,J", DC.nll_edge_shapes())
def test_prototype_passes_edge_likelihood(N, J):
    for case in DC.nll_edge_cases([(N, J)]):
        DC.check_nll(DC.proto_nll(), case)


def test_prototype_passes_batch_likelihood():
    for case in DC.nll_batch_cases():
        DC.check_nll_batch(DC.proto_nll_batch(), case)


def test_prototype_passes_prediction_and_status():
    worst = np.zeros(2)
    for case in DC.predict_cases():
        worst = np.maximum(worst, DC.check_predict(DC.proto_predict(), case))
    print(f"worst prototype deviation: mean {worst[0]:.2e} max|mean|, covariance {worst[1]:.2e} k(0)")
    for case in DC.status_cases():
        DC.check_status(DC.proto_predict(), case)


def test_prototype_on_the_fixture(golden_dir):
    """the prototype on the eight n150 draws of lowest ratio and eight spread over the rest, through check_fixture"""
    (group,) = DC.fixture_groups(golden_dir, "n150")
    o = np.argsort(group[-1], kind="stable")
    pick = np.concatenate([o[:8], o[8::40]])
    sub = group[:4] + (group[4][pick], group[5][pick]) + group[6:8] + (group[8][pick], group[9][pick], group[10][pick], group[11][pick], group[12][pick])
    DC.check_fixture(DC.proto_nll_batch(), sub)


def _caught(check, impl, cases):
    out = []
    for case in cases:
        try:
            check(impl, case)
        except AssertionError:
            out.append(case[0])
    return out


@pytest.mark.parametrize("mistake", DC.proto().MISTAKES)
def test_the_cases_can_fail(mistake):
    """Each seeded mistake of the prototype fails a checker on at least one case.  (The edge likelihood cases here: the shapes up to N = 193
    with J = 5, whose references the tests above have computed already.)"""
    caught = _caught(DC.check_nll, DC.proto_nll(mistake=mistake), DC.nll_edge_cases([(N, 5) for N in DC.N_EDGE if N <= 193]))
    caught += _caught(DC.check_nll_batch, DC.proto_nll_batch(mistake=mistake), DC.nll_batch_cases())
    caught += _caught(DC.check_predict, DC.proto_predict(mistake=mistake), DC.predict_cases())
    caught += _caught(DC.check_status, DC.proto_predict(mistake=mistake), DC.status_cases())
    print(f"{mistake}: caught by {len(caught)} cases, e.g. {caught[:6]}")
    assert caught, mistake
