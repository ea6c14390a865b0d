"""GPU tests (-m gpu) of the dense solver (csrc/dense.hip; Context.dense_nll, dense_nll_batch, dense_predict, dense_predict_cov) against a
truth that is no fp64 code: oracle.dense_nll_truth, oracle.predict_mean_truth and oracle.predict_cov_truth, dense in long double, and the
__float128 values of tests/golden/quad_truth.npz through tests/golden/dense_truth.npz.

Every bound is max(20 x ref_dev, 256 eps) in the natural scale of the quantity, ref_dev the worst deviation from the same truth of fp64
evaluations that are not the device (LAPACK, the C restatement, the same on the reversed or permuted series; for the prediction
oracle.predict_*_numpy, the reversed series and the LU form).  Cases, checkers and the reasoning behind the bound live in tests/dense_cases.py;
tests/test_dense_host.py shows that the cases catch seeded mistakes.  Every figure is printed before it is asserted
(profiles/dense_truth.txt holds the measured ones)."""
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import pioran_jl_amd as pj  # noqa: E402

sys.path.insert(0, str(Path(__file__).resolve().parent))
import dense_cases as DC  # noqa: E402

VARIANTS = (("old chain", "dense_old_chain", 1, 0), ("no pairs", "dense_no_pairs", True, False), ("no halves", "dense_no_halves", True, False))


@pytest.fixture(scope="module")
def ctx():
    return pj.Context(0)


def single(ctx):
    return lambda a, b, c, d, t, y, s2: ctx.dense_nll(a, b, c, d, t, y, s2, return_info=True)


def batched(ctx):
    return lambda A, Bc, C, Dd, t, y, s2, mu, nu: ctx.dense_nll_batch(A, Bc, C, Dd, t, y, s2, mu=mu, nu=nu, return_info=True)


def one_by_one(ctx):
    """the single-matrix entry as an `impl` of the batch checkers: y - mu and nu sigma2 formed in fp64 by the caller"""
    def impl(A, Bc, C, Dd, t, y, s2, mu, nu):
        res = [ctx.dense_nll(A[k], Bc[k], C, Dd, t, y - mu[k], nu[k] * s2, return_info=True) for k in range(len(A))]
        return np.array([r[0] for r in res]), np.array([r[1] for r in res])
    return impl


class option:
    """a context option for the length of a `with` block"""
    def __init__(self, ctx, key, on, off):
        self.ctx, self.key, self.on, self.off = ctx, key, on, off

    def __enter__(self):
        self.ctx.set_option(self.key, self.on)

    def __exit__(self, *exc):
        self.ctx.set_option(self.key, self.off)


# ---- a: edge shapes, one matrix --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,J,order", [(N, J, o) for N, J in DC.nll_edge_shapes() for o in DC.ORDERS if N > 1 or o == "sorted"])
def test_edge_shapes_one_matrix(ctx, N, J, order):
    """dense_nll at every tile edge, sigma2 as drawn and `hard`; from N = 192 on (three block columns: dense_step_kernel) the same draw also
    on the panel / update chain, with one panel per launch and with whole tiles: each within the bound, info 0, whole tiles bit-equal to the
    default.  One case is held to its measured figure instead of 20 ref_dev: dense_cases.KNOWN_LIMITS says which and why."""
    for case in DC.nll_edge_cases([(N, J)], [order]):
        DC.check_nll(single(ctx), case, DC.KNOWN_LIMITS)
        if N >= 192:
            default = ctx.dense_nll(*case[1:])
            for name, key, on, off in VARIANTS:
                with option(ctx, key, on, off):
                    got, info = ctx.dense_nll(*case[1:], return_info=True)
                    print(f"({name})", end=" ")
                    DC.check_nll(lambda *args: (got, info), case, DC.KNOWN_LIMITS)
                if key == "dense_no_halves":
                    assert got == default, (case[0], got, default)


# ---- b: edge shapes, batched -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(2 * len(DC.BATCH_SHAPES)))
def test_edge_shapes_batched(ctx, k):
    """dense_nll_batch: every draw within its own bound, and bit-equal to the same draw one batch position further on (the last draw first)"""
    case = list(DC.nll_batch_cases())[k]
    label, t, y, s2, A, Bc, C, Dd, mu, nu = case
    DC.check_nll_batch(batched(ctx), case)
    got, info = batched(ctx)(A, Bc, C, Dd, t, y, s2, mu, nu)
    roll = lambda v: None if v is None else np.roll(v, 1, axis=0)
    again, info2 = batched(ctx)(roll(A), roll(Bc), roll(C) if C.ndim == 2 else C, roll(Dd) if Dd.ndim == 2 else Dd, t, y, s2, roll(mu), roll(nu))
    assert np.array_equal(np.roll(got, 1), again) and np.array_equal(np.roll(info, 1), info2), (label, got, again)


# ---- c: ill-conditioned draws ----------------------------------------------------------------------------------------------------------
def test_ill_conditioned_n150(ctx, golden_dir):
    """all 325 stored draws at N = 150 through dense_nll_batch (11 launches of at most 32)"""
    (group,) = DC.fixture_groups(golden_dir, "n150")
    assert len(group[4]) == 325
    DC.check_fixture(batched(ctx), group)


def test_ill_conditioned_n1000_batched(ctx, golden_dir):
    (group,) = DC.fixture_groups(golden_dir, "n1000")
    assert len(group[4]) == 48
    DC.check_fixture(batched(ctx), group)


def test_ill_conditioned_n1000_one_matrix_both_chains(ctx, golden_dir):
    """the 8 draws of lowest ratio through the single-matrix call: one launch per block column, then the panel / update chain"""
    (group,) = DC.fixture_groups(golden_dir, "n1000")
    assert (np.diff(group[-1][:8]) >= 0).all() and group[-1][:8].max() <= group[-1][8:].min()
    DC.check_fixture(one_by_one(ctx), group, slice(0, 8))
    with option(ctx, "dense_old_chain", 1, 0):
        print("(old chain)")
        DC.check_fixture(one_by_one(ctx), group, slice(0, 8))


@pytest.mark.parametrize("k", range(4))
def test_ill_conditioned_long(ctx, golden_dir, k):
    """N = 1536, 1700, 2881, 3100 (both sides of the pair / single switch and of the half-tile limit), the four draws of lowest ratio: the
    single-matrix call on both chains"""
    group = DC.fixture_groups(golden_dir, "long")[k]
    assert len(group[1]) == (1536, 1700, 2881, 3100)[k]
    DC.check_fixture(one_by_one(ctx), group)
    with option(ctx, "dense_old_chain", 1, 0):
        print("(old chain)")
        DC.check_fixture(one_by_one(ctx), group)


# ---- d: prediction ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", DC.predict_shapes(), ids=lambda s: f"N{s[0]}-M{s[1]}-{s[2]}-J{s[3]}")
def test_prediction(ctx, shape):
    """dense_predict with the covariance: mean and covariance within their bounds, the covariance exactly symmetric and its diagonal at a data
    time within [0, sigma2_n] (check_predict); the covariance-only entry and the mean-only call bit-equal to the combined call."""
    cases = list(DC.predict_cases([shape]))
    assert len(cases) == 2
    for case in cases:
        label, a, b, c, d, t, y, s2, tau = case
        (mean, cov), info = ctx.dense_predict(a, b, c, d, tau, t, y, s2, with_covariance=True, return_info=True)
        DC.check_predict(lambda *args: (mean, cov, info), case)
        cov_only, info_c = ctx.dense_predict_cov(a, b, c, d, tau, t, s2, return_info=True)
        mean_only, info_m = ctx.dense_predict(a, b, c, d, tau, t, y, s2, return_info=True)
        assert info_c == info_m == 0
        assert np.array_equal(cov_only, cov), (label, "covariance-only entry")
        assert np.array_equal(mean_only, mean), (label, "mean-only call")


# ---- e: status -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(DC.STATUS_BAD)))
def test_prediction_status_of_a_bad_pivot(ctx, k):
    """one sigma2 = -50 at row 0, 63, 64, 100 of N = 130: info is that row + 1 (LAPACK's numbering) on all three calls, mean and covariance
    all NaN; the truth raises at the same row"""
    case = list(DC.status_cases())[k]
    label, a, b, c, d, t, y, s2, tau, bad = case
    def impl(a, b, c, d, tau, t, y, s2):
        (mean, cov), info = ctx.dense_predict(a, b, c, d, tau, t, y, s2, with_covariance=True, return_info=True)
        return mean, cov, info
    DC.check_status(impl, case)
    cov_only, info_c = ctx.dense_predict_cov(a, b, c, d, tau, t, s2, return_info=True)
    mean_only, info_m = ctx.dense_predict(a, b, c, d, tau, t, y, s2, return_info=True)
    assert info_c == info_m == bad + 1 and np.isnan(cov_only).all() and np.isnan(mean_only).all()
