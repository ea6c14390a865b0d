"""CPU tests (-m "not gpu") of the cases and checkers the posterior mean and the simulation are held to on the GPU
(tests/predict_mean_cases.py): the long-double truths, the numpy twin of the windowed mean path (tools/predict_mean_proto.py) and the fp64
oracles on every case, that the case list holds every edge it promises, and that the cases catch seeded mistakes."""
import sys
from pathlib import Path

import numpy as np
import pytest

from oracle import oracle as O

sys.path.insert(0, str(Path(__file__).resolve().parent))
import predict_mean_cases as PM  # noqa: E402
import predict_var_cases as PV  # noqa: E402

QSEG, KW, EVT = 128, 16, 8


@pytest.fixture(scope="module")
def edge():
    return list(PM.edge_cases())


def _features(case):
    label, t, y, s2, A, Bc, C, Dd, mu, nu, tau, q = case
    N, M = len(t), len(tau)
    R = 2 * A.shape[1] - int(np.sum(np.atleast_2d(Dd)[0] == 0.0))
    asc = np.sort(tau)
    n0 = np.searchsorted(t, asc, side="left")
    return N, M, R, asc, n0


# ---- the truths ------------------------------------------------------------------------------------------------------------------------
def test_truths_agree_with_each_other_and_raise():
    """predict_mean_truth at the data times with nothing held back is y - s2 K^-1 y; sim_truth's factor reproduces K; the variance truth, the
    mean truth and the simulation truth see the same factor; a matrix that is not positive definite raises."""
    rng = np.random.default_rng(5)
    t, s2, A, Bc, C, Dd, nu = PV._draws(rng, 40, 4, 1, np.arange(1))
    a, b = A[0], Bc[0]
    y = rng.standard_normal(40)
    K = PM._dense(a, b, C, Dd, t, s2)
    m = O.predict_mean_truth(a, b, C, Dd, t, t, y, s2)
    assert m.dtype == np.longdouble
    assert np.max(np.abs(m - (y - s2 * np.linalg.solve(K, y)))) <= 1e-12 * np.max(np.abs(y))
    Cq = np.array([O.sim_truth(a, b, C, Dd, t, s2, e) for e in np.eye(40)]).T          # the factor, column by column
    assert (np.diag(Cq) > 0).all() and np.array_equal(Cq, np.tril(Cq))
    assert np.max(np.abs((Cq @ Cq.T).astype(float) - K)) <= 1e-14 * a.sum()
    # var(tau) = k(0) - k*' K^-1 k*: the mean truth of the 'series' k*(tau_m) at tau_m
    tau = rng.uniform(t[0], t[-1], 3)
    v = O.predict_var_truth(a, b, C, Dd, tau, t, s2)
    for i, tm in enumerate(tau):
        ks = np.array([O.kappa(a, b, C, Dd, abs(tm - tn)) for tn in t])
        assert abs(float(a.sum() - O.predict_mean_truth(a, b, C, Dd, tau[i:i + 1], t, ks, s2)[0] - v[i])) <= 1e-14 * a.sum()
    for f in (lambda: O.predict_mean_truth(-a, b, C, Dd, tau, t, y, s2), lambda: O.sim_truth(-a, b, C, Dd, t, s2, y),
              lambda: O.predict_var_truth(-a, b, C, Dd, tau, t, s2)):
        with pytest.raises(np.linalg.LinAlgError):
            f()


# ---- the twin and the fp64 oracles on the cases ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["edge", "fuzz"])
def test_twin_and_oracles_on_the_cases(which, edge):
    """check_mean / check_sim of the twin and of both fp64 oracles on every edge and fuzz case, sigma2 = 0 included for the simulation: every draw
    positive definite in the truth's own Cholesky (reference() raises otherwise), none skipped."""
    cases = edge if which == "edge" else list(PM.fuzz_cases(40))
    assert len(cases) == (2 * len(PM.edge_combinations()) if which == "edge" else 40)
    worst = {"mean": 0.0, "sim": 0.0, "mean_ref": 0.0, "sim_ref": 0.0}
    nsim = 0
    for case in cases:
        for impl in (PM.twin_impl(), PM.oracle_predict_impl(), PM.direct_impl()):
            worst["mean"] = max(worst["mean"], PM.check_mean(impl, case).max())
        worst["mean_ref"] = max(worst["mean_ref"], PM.reference(case, "mean")[1].max())
        for sc in PM.sim_variants(case):
            for impl in (PM.oracle_sim_impl(), PM.dense_sim_impl()):
                worst["sim"] = max(worst["sim"], PM.check_sim(impl, sc).max())
            worst["sim_ref"] = max(worst["sim_ref"], PM.reference(sc, "sim")[1].max())
            nsim += 1
    print(f"{which}: {len(cases)} mean cases, {nsim} simulation cases, worst deviations {worst}")
    assert nsim == (3 * len(cases) // 2 if which == "edge" else len(cases))


# ---- what the case list holds ----------------------------------------------------------------------------------------------------------
def test_case_list_covers_what_it_promises(edge):
    """Every edge named in the module docstring of predict_mean_cases, derived from the cases themselves."""
    combos = PM.edge_combinations()
    assert len(set(combos)) == len(combos) and len(edge) == 2 * len(combos)
    assert len({c[0] for c in edge}) == len(edge)
    feats = [(c, *_features(c)) for c in edge]
    windowed = [f for f in feats if f[3] <= 63]
    wide = [f for f in feats if f[3] > 63]
    for case, N, M, R, asc, n0 in feats:
        label = case[0]
        assert f"R{R}-N{N}-" in label and (f"-M{M}-" in label or "-M" not in label), label
        assert len(case[4]) == (3 if N <= 129 else 2), label
        assert len(set(case[8])) == len(case[8]) and len(set(case[9])) == len(case[9]), label        # mu, nu of their own
    have = lambda fs, i, vals: set(vals) <= {f[i] for f in fs}
    # q_segment / q_carry: one, two, three segments; only the third has a non-zero carry to multiply
    assert {1, 2, 3} <= {(N + QSEG - 1) // QSEG for _, N, *_ in windowed}
    # fused path (ascending tau, M <= N R)
    fused = [f for f in windowed if f[2] <= f[1] * f[3]]
    assert any((n0 == 0).any() for *_, n0 in fused) and any((n0 == N).any() for _, N, _, _, _, n0 in fused)
    assert any(np.max(np.bincount(n0[(n0 > 0) & (n0 < N)], minlength=1)) >= 5 for _, N, _, _, _, n0 in fused)          # many times in one gap
    assert any(((n0 % QSEG == 0) & (n0 > 0) & (n0 < N)).any() for _, N, _, _, _, n0 in fused)      # n0 - 1 the last step of a segment
    assert any(((n0 % QSEG == QSEG - 1) & (n0 + 1 < N)).any() for _, N, _, _, _, n0 in fused)      # n0 the last step of a segment
    assert any((np.diff(asc) == 0).any() for *_, asc, _ in fused)                                   # ties
    assert any(M == 1 for _, _, M, *_ in fused)
    for R, N in PM.SWITCH_SHAPES:                                                                   # both sides of the switch, tau ascending
        assert {N * R, N * R + 1} <= {f[2] for f in windowed if (f[3], f[1]) == (R, N)}
    # two-pass path (the permuted leg of every case; ascending where M > N R)
    assert have(windowed, 2, (EVT - 1, EVT, EVT + 1, 127, 128, 129))
    assert have(windowed, 3, (16, 17, 32, 33, 48, 49))
    assert any((n0 == 0).any() and M > 1 for _, _, M, _, _, n0 in windowed) and any((n0 == N).any() and M > 1 for _, N, M, _, _, n0 in windowed)
    # windowed z and the windowed simulation
    assert have(windowed, 1, (KW - 1, KW, KW + 1, 2 * KW - 1, 2 * KW, 2 * KW + 1))
    assert have(windowed, 3, (15, 16, 31, 32, 47, 48))
    assert {1, 2, 3, 4} == {(R + 16) // 16 for _, _, _, R, *_ in windowed}
    assert have(windowed, 1, (16 * KW, 16 * KW + 1))                                                # sixteen windows per block of the xi kernel
    assert any(N % KW for _, N, *_ in windowed) and any(N <= KW for _, N, *_ in windowed)
    assert any(N % KW == 1 and N > KW for _, N, *_ in windowed)                                     # a last window of one step
    # step by step: through no_block every windowed shape as well, so the lengths and M count over all cases
    assert have(feats, 1, (1, 2, 3, 4, 5, 8, 9))
    assert have(wide, 3, (64, 65, 128, 129, 143))
    assert have(feats, 2, (255, 256, 257))
    # sigma2: as drawn, x 1e-6, and zero for the simulation
    assert sum(c[0].endswith("-s2x1") for c in edge) == sum(c[0].endswith("-s2x1e-6") for c in edge) == len(combos)
    assert all(np.array_equal(a[3] * 1e-6, b[3]) for a, b in zip(edge[0::2], edge[1::2]))
    zero = [sc for c in edge for sc in PM.sim_variants(c) if not sc[3].any()]
    assert len(zero) == len(combos)
    # the fuzz: both kinds of (c, d), more than two segments
    fz = list(PM.fuzz_cases(40))
    assert {c[0].split("-")[-1] for c in fz} == {"shared", "perdraw"}
    assert max(len(c[1]) for c in fz) > 2 * QSEG and min(len(c[1]) for c in fz) < KW
    # the per-draw variant keeps the rows and differs between the draws
    v = PM.per_draw_variant(edge[0])
    assert v[6].shape == edge[0][4].shape and len({tuple(r) for r in v[6]}) == len(v[6]) and np.array_equal(v[7] == 0, np.tile(edge[0][7] == 0, (len(v[7]), 1)))


# ---- the cases can fail ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mistake", ["carry_drops_product", "no_backward_link", "fused_misses_segment_end", "clamped_row_weighted", "sin_row_sign"])
def test_the_cases_can_fail(mistake, edge):
    """Each seeded mistake of the twin (tools/predict_mean_proto.py, MISTAKES) fails check_mean() on at least one edge case;
    carry_drops_product on none with N <= 256 (two segments: the carry that is multiplied is zero), which is why the longer cases exist."""
    assert mistake in PM.proto().MISTAKES
    caught = []
    for case in edge:
        try:
            PM.check_mean(PM.twin_impl(mistake=mistake), case)
        except AssertionError:
            caught.append(case)
    print(f"{mistake}: caught by {len(caught)} edge cases, e.g. {[c[0] for c in caught[:4]]}")
    assert caught, mistake
    if mistake == "carry_drops_product":
        assert all(len(c[1]) > 2 * QSEG for c in caught), [c[0] for c in caught]
    if mistake == "no_backward_link":
        assert all(len(c[1]) > QSEG for c in caught), [c[0] for c in caught]


def test_the_simulation_checker_can_fail(edge):
    """An implementation that returns the truth with ONE element off by 1e3 x FLOOR x scale fails check_sim, wherever the element is: the first
    step, both sides of the first window edge, the first step of the last, partial window, the last step."""
    case = next(c for c in edge if c[0].startswith("R33-N257-mixed-s2x1"))
    for sc in PM.sim_variants(case):
        truth = PM.reference(sc, "sim")[0]
        N = truth.shape[1]
        exact = lambda *a: (truth.astype(float), np.zeros(len(truth), dtype=np.int32))
        PM.check_sim(exact, sc)
        assert N % KW
        for n in (0, KW - 1, KW, N - N % KW, N - 1):
            for k in range(len(truth)):
                off = truth.astype(float)
                off[k, n] += 1e3 * PM.FLOOR * float(np.max(np.abs(truth[k])))
                with pytest.raises(AssertionError):
                    PM.check_sim(lambda *a: (off, np.zeros(len(truth), dtype=np.int32)), sc)
    with pytest.raises(AssertionError):
        PM.check_sim(lambda *a: (truth.astype(float), np.array([0, 2], dtype=np.int32)), sc)
    with pytest.raises(AssertionError):
        PM.check_sim(lambda *a: (truth.astype(float)[:, :-1], np.zeros(2, dtype=np.int32)), sc)
