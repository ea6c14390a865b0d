"""CPU tests (-m "not gpu") of the cases and the checker the gradient of log L is held to on the GPU (tests/grad_cases.py): the long-double truth
against its 50-digit pin and against the quad-precision value, both fp64 references on every case, that the case list holds every edge it
promises, and that the checker catches seeded mistakes.  The references of the edge cases are computed once per session (grad_cases.reference
keeps them) and shared by the tests below."""
import sys
from pathlib import Path

import numpy as np
import pytest

from oracle import oracle as O

sys.path.insert(0, str(Path(__file__).resolve().parent))
import grad_cases as GC  # noqa: E402

# oracle.logl_grad_truth against the 50-digit values of tests/golden/grad_truth.npz: measured 1.7e-18 at the worst (grad_c of draw 0; the
# sigma2 x 1e-6 draws are no worse), 16 long-double eps; allowed 1e-17.  docs/EXPERIMENTS.md section 28.
PIN_BOUND = 1e-17
# largest ref_dev any edge case may show (the issue's figure; measured: see test_references_on_every_edge_case)
REF_DEV_MAX = 1e-11


@pytest.fixture(scope="module")
def edge():
    return list(GC.edge_cases())


# ---- the truth ---------------------------------------------------------------------------------------------------------------------------
def test_truth_against_50_digits(golden_dir):
    """oracle.logl_grad_truth on the six draws of oracle/make_grad_truth.py (one-row terms, own mu and nu, sigma2 x 1e-6, a shift) against the
    stored mpmath evaluation, every key in the scale grad_cases takes deviations in."""
    F = np.load(golden_dir / "grad_truth.npz")
    keys = [str(k) for k in F["keys"]]
    scaled_by = {"grad_mu": "scale_mu", "grad_nu": "scale_nu", "grad_shift": "scale_shift"}
    worst = 0.0
    for i in range(int(F["ndraws"])):
        dr = {k: F[f"d{i}_in_{k}"] for k in ("a", "b", "c", "d", "t", "y", "s2", "mu", "nu", "shift")}
        shift = None if np.isnan(dr["shift"]) else float(dr["shift"])
        ld = O.logl_grad_truth(dr["a"], dr["b"], dr["c"], dr["d"], dr["t"], dr["y"], dr["s2"], mu=float(dr["mu"]), nu=float(dr["nu"]), shift=shift)
        assert ld["logl"].dtype == np.longdouble
        seen = 0
        for k in keys:
            if f"d{i}_{k}_hi" not in F.files:
                assert ld.get(k) is None, (i, k)
                continue
            want = F[f"d{i}_{k}_hi"].astype(np.longdouble) + F[f"d{i}_{k}_lo"].astype(np.longdouble)
            scale = float(F[f"d{i}_{scaled_by[k]}_hi"][0]) if k in scaled_by else float(np.max(np.abs(want)))
            err = float(np.max(np.abs(np.atleast_1d(ld[k]) - want)))
            dev = err / scale if scale > 0 else err
            print(f"draw {i} {k}: {dev:.2e}")
            worst = max(worst, dev)
            seen += 1
            assert dev <= PIN_BOUND, (i, k, dev)
        assert seen == 11                                 # (a shifted draw has grad_shift and its scale in place of the two series gradients)
        one_row = (dr["b"] == 0) & (dr["d"] == 0)
        assert (ld["grad_b"][one_row] == 0).all() and (ld["grad_d"][one_row] == 0).all()
    print(f"worst deviation of the long-double truth from 50 digits: {worst:.2e}")


def test_truth_value_against_quad_and_the_entry_conventions(edge):
    """The truth's value is the likelihood the entry returns: against oracle.logl_quad (the recurrence in __float128) of y - mu and nu s2, and with a
    shift against the same of the transformed series — no Jacobian term; its grad_mu, grad_nu, grad_shift are the derivatives of that value
    (central differences in long double through the truth itself would share its code: complex steps of the oracle instead)."""
    picked = [c for c in edge if c[0].split("-s2")[0] in ("R5-N17", "R33-N33", "R33-N129", "R80-N9", "R63-N17", "R143-N18", "R3-N257")]
    assert len(picked) == 2 * 7 + 2 * 4
    worst = 0.0
    for case in picked:
        truth = GC.reference(case)[0]
        label, t, y, s2, A, Bc, C, Dd, mu, nu, shift = case
        for k in range(len(A)):
            yc, sk, S, v = GC._series(case, k)
            want = O.logl_quad(A[k], Bc[k], C, Dd, t, yc, sk)
            dev = abs(float(truth[k]["logl"]) - want) / abs(want)
            worst = max(worst, dev)
            # without a shift both see the same fp64 series: the quad value rounded to fp64 and the long-double one differ by roundings of the value;
            # with one, the fp64 transform's roundings move the value (1e-16 of each Y_n and S_n against z_n and G_nn)
            assert dev <= (4 * np.finfo(float).eps if shift is None else 1e-11), (label, k, dev)
    print(f"truth's value against the quad-precision recurrence: worst {worst:.2e}")


# ---- both fp64 references on every case -------------------------------------------------------------------------------------------------------
def test_references_on_every_edge_case(edge):
    """Every edge case has a truth (positive definite in long double: reference() raises otherwise, none is skipped); both fp64 references pass
    check() and lie within the bound of each other; ref_dev stays below 1e-11 on every case, draw and key."""
    assert len(edge) == GC.n_edge_cases() and len({c[0] for c in edge}) == len(edge)
    worst = {}
    for case in edge:
        truth, ref_dev, parts = GC.reference(case)
        keys = GC.keys_of(case)
        for key in keys:
            assert np.isfinite(ref_dev[key]).all(), (case[0], key)
            m = float(ref_dev[key].max())
            if key not in worst or m > worst[key][0]:
                worst[key] = (m, case[0])
            assert m < REF_DEV_MAX, (case[0], key, m)
        series = GC.series_ref(case)
        cs = GC.reference_impl("complex_step", series)(case)
        de = GC.reference_impl("dense_fp64")(case)
        for key in keys:
            if key not in cs:
                assert key in GC.SERIES_KEYS and not series
                continue
            bound = np.maximum(GC.MARGIN * ref_dev[key], GC.FLOOR)
            for k in range(len(case[4])):
                # the two references against each other, in the truth's scale (nothing to compare where all of it is structurally zero)
                scale = float(truth[k][GC.SUM_KEYS[key]]) if key in GC.SUM_KEYS else float(np.max(np.abs(truth[k][key])))
                if scale > 0:
                    between = float(np.max(np.abs(cs[key][k] - de[key][k]))) / scale
                    assert between <= bound[k], (case[0], key, k, between, bound[k])
    for key, (m, label) in worst.items():
        print(f"largest ref_dev {key:12s} {m:.2e}   {label}")


def test_step_by_step_form_of_grad_d(edge):
    """The bound of its own that grad_d of the step-by-step reverse mode has (grad_cases.wide_bounds) comes from tools/wide_adjoint_dd_proto.py:
    in long double that form IS the dense formula (measured: within 1.7e-15 of the truth; allowed 1e-13, the amplification times the long-double
    eps), in fp64 it deviates by more than the fp64 references do — its two accumulators exceed their sum by up to 9e3 —, and the bound is never
    below the common one."""
    P = GC.wide_proto()
    worst_ld = worst_ratio = 0.0
    for case in [c for c in edge if c[0].split("-s2")[0] in ("R3-N48", "R3-N66", "R3-N97", "R3-N256", "R33-N129", "R80-N65") and c[10] is None]:
        truth = GC.reference(case)[0]
        for k in range(len(case[4])):
            yc, sk, S, v = GC._series(case, k)
            ld, rows = P.wide_dd(case[4][k], case[5][k], case[6], case[7], case[1], yc, sk, np.longdouble)
            dev = GC.deviation(ld, truth[k], "grad_d")
            worst_ld = max(worst_ld, dev)
            worst_ratio = max(worst_ratio, float(np.max(np.abs(rows)) / np.max(np.abs(truth[k]["grad_d"]))))
            assert dev <= 1e-13, (case[0], k, dev)
            one_row = case[7] == 0.0
            assert (ld[one_row] == 0).all()
    worst = (0.0, "")
    for case in edge:
        form, common, own = GC.wide_form_dev(case), GC.bound_of(case, "grad_d"), GC.wide_bounds(case)["grad_d"]
        assert np.isfinite(form).all() and (own >= common).all() and (own <= np.maximum(GC.MARGIN * np.maximum(form, GC.reference(case)[1]["grad_d"]), GC.FLOOR)).all()
        worst = max(worst, (float(form.max()), case[0]))
    print(f"step-by-step form of grad_d: in long double {worst_ld:.2e} from the truth; accumulators / sum up to {worst_ratio:.1e}; largest fp64 deviation {worst[0]:.2e} ({worst[1]})")
    assert worst_ratio > 1e3 and worst[0] < 1e-10


def test_fuzz_cases_have_references():
    """The fuzz may leave out at most 5 % of its cases (truth or reference refusing the draw); measured: none."""
    left_out = []
    cases = list(GC.fuzz_cases(40))
    assert len(cases) == 40 and len({c[0] for c in cases}) == 40
    for case in cases:
        try:
            GC.check(GC.reference_impl("dense_fp64"), case)
        except np.linalg.LinAlgError as e:
            left_out.append((case[0], str(e)))
    print(f"fuzz: {len(left_out)} of {len(cases)} left out {left_out}")
    assert len(left_out) <= 0.05 * len(cases)
    Rs = [GC.rows(c) for c in cases]
    assert min(Rs) < 16 and max(Rs) > 127 and any(64 <= r <= 95 for r in Rs)
    assert any(np.sum(c[7] == 0.0) > 1 for c in cases) and min(c[3].max() for c in cases) < 1e-5


# ---- what the case list holds ------------------------------------------------------------------------------------------------------------------
def test_case_list_covers_what_it_promises(edge):
    """Every edge named in the module docstring of grad_cases, derived from the cases themselves with rpl_of, the block columns and the checkpoint
    segments restated from celerite_wide.hip / celerite_block.hip / celerite_tile.hip."""
    plain = [c for c in edge if c[10] is None]
    feats = [(GC.rows(c), len(c[1]), len(c[4]), c) for c in plain]
    for R, N, B, c in feats:
        assert c[0].startswith(f"R{R}-N{N}-"), c[0]
        assert B == GC.n_draws(N) and len(set(c[8])) == B and len(set(c[9])) == B, c[0]          # mu, nu of their own
        assert np.ndim(c[6]) == 1
    shapes = {(R, N) for R, N, _, _ in feats}
    Rs, Ns = {R for R, _ in shapes}, {N for _, N in shapes}
    # rpl_of: both sides of every step, and the last row count; the restatement itself
    assert [GC.rpl_of(R) for R in (1, 15, 16, 31, 32, 47, 48, 63, 64, 79, 80, 95, 96, 111, 112, 127, 128, 143)] == [1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9]
    for lo in (15, 31, 47, 63, 79, 95, 111, 127):
        assert {lo, lo + 1} <= Rs, lo
    assert 143 in Rs and {GC.rpl_of(R) for R in Rs} == set(range(1, 10))
    # block columns NB = (R + 16) / 16 of the windowed kernels: both sides of every step, up to 63 rows
    for lo in (15, 31, 47):
        assert {lo, lo + 1} <= Rs and GC.block_columns(lo) + 1 == GC.block_columns(lo + 1)
    assert {GC.block_columns(R) for R in Rs if R <= 63} == {1, 2, 3, 4} and {1, 2, 62, 63} <= Rs
    assert all(c[4].shape[1] <= 32 for R, _, _, c in feats if R <= 63)       # (terms within the windowed kernels' LDS: the family follows from the rows)
    # the windows: one step, full, one more, ragged ends
    assert {1, 2, KW_ - 1, KW_, KW_ + 1, 2 * KW_ - 1, 2 * KW_, 2 * KW_ + 1, 3 * KW_, 3 * KW_ + 1, 4 * KW_, 4 * KW_ + 1, 16 * KW_, 16 * KW_ + 1} <= Ns
    # checkpoint segments of the step-by-step reverse mode: K = 16 | 32 | 64, nseg = 0 .. 4 (two buffers and the second stream alternate from three on)
    assert [GC.ckpt_every(N) for N in (1, 64, 65, 256, 257)] == [16, 16, 32, 32, 64]
    assert {64, 65, 256, 257} <= Ns
    for R in GC.LENGTHS_R:
        assert {GC.nseg_of(N) for r, N in shapes if r == R} >= {0, 1, 2, 3, 4}, R
        assert {(GC.ckpt_every(N), GC.nseg_of(N)) for r, N in shapes if r == R} >= {(16, 4), (32, 3), (32, 8), (64, 4)}
    assert (17 - 1) // 16 == 1 and GC.nseg_of(17) == 1 and GC.nseg_of(18) == 2 and GC.nseg_of(33) == 2 and GC.nseg_of(34) == 3
    # the rows that default to the step-by-step reverse mode: one, two, three and more segments
    assert {GC.nseg_of(N) for R, N in shapes if R == 80} >= {1, 2, 3} and {17, 18, 49, 65} <= {N for R, N in shapes if R == 80}
    assert {GC.nseg_of(N) for R, N in shapes if R > 63} >= {0, 1, 2, 3}
    # the tile reverse kernel's last workgroup partly filled: 5 draws at 4, 3 and 2 draws per workgroup
    five = {R for R, N, B, _ in feats if B == 5 and R <= 63}
    assert {GC.tile_adj_waves(R, cd) for R in five for cd in (False, True)} == {4, 3, 2}
    assert all(5 % GC.tile_adj_waves(R, cd) for R in five for cd in (False, True))
    # one-row terms: alone, first among others, and shapes without any
    nreal = {R: int(np.sum(c[7] == 0.0)) for R, _, _, c in feats}
    assert nreal[1] == 1 and nreal[2] == 0 and set(nreal.values()) == {0, 1, 2, 3}
    assert any(n > 0 for R, n in nreal.items() if R > 63) and any(n > 0 for R, n in nreal.items() if 16 <= R <= 63)
    # sigma2: as drawn and x 1e-6, in pairs
    a, b = [c for c in plain if c[0].endswith("-s2x1")], [c for c in plain if c[0].endswith("-s2x1e-6")]
    assert len(a) == len(b) == len(GC.edge_combinations()) and all(np.array_equal(x[3] * 1e-6, y[3]) for x, y in zip(a, b))
    # shift: the four shapes, a shift per draw below the data minimum
    sh = [c for c in edge if c[10] is not None]
    assert {(GC.rows(c), len(c[1])) for c in sh} == set(GC.SHIFT_SHAPES) and len(sh) == 2 * len(GC.SHIFT_SHAPES)
    for c in sh:
        assert len(set(c[10])) == len(c[4]) and c[10].max() < c[2].min()
    # the per-draw variant keeps the rows and differs between the draws
    v = GC.per_draw_variant(edge[0])
    assert v[6].shape == edge[0][4].shape and len({tuple(r) for r in v[6]}) == len(v[6]) and GC.rows(v) == GC.rows(edge[0])


KW_ = GC.KW


# ---- the checker can fail ----------------------------------------------------------------------------------------------------------------------
def _dense_G(case, k):
    """(G, D) of draw k in fp64"""
    label, t, y, s2, A, Bc, C, Dd, mu, nu, shift = case
    yc, sk, S, v = GC._series(case, k)
    D = np.abs(t[:, None] - t[None, :])
    K = (np.exp(-C * D[..., None]) * (A[k] * np.cos(Dd * D[..., None]) + Bc[k] * np.sin(Dd * D[..., None]))).sum(-1) + np.diag(sk)
    Kinv = np.linalg.inv(K)
    z = Kinv @ yc
    return 0.5 * (np.outer(z, z) - Kinv), D


def _mistaken(mistake):
    """the complex-step reference's output with a seeded mistake, as an `impl` of check(); None from the impl: the mistake does not apply to the case"""
    def impl(case):
        label, t, y, s2, A, Bc, C, Dd, mu, nu, shift = case
        out = {k: np.array(v, copy=True) for k, v in GC.reference_impl("complex_step", True)(case).items()}
        B, N = len(A), len(t)
        if mistake == "one_grad_a_scaled":                   # the term with the median |grad_a| of draw 0
            j = int(np.argsort(np.abs(out["grad_a"][0]))[A.shape[1] // 2])
            out["grad_a"][0, j] *= 1 + 1e-10
        elif mistake == "grad_c_last_window_dropped":        # the entries of the last N mod 16 steps dropped from the sum
            tail = N % 16
            for k in range(B):
                G, D = _dense_G(case, k)
                G[:N - tail, :N - tail] = 0.0
                out["grad_c"][k] -= np.array([-(G * D * np.exp(-C[j] * D) * (A[k, j] * np.cos(Dd[j] * D) + Bc[k, j] * np.sin(Dd[j] * D))).sum() for j in range(len(C))])
        elif mistake == "grad_sigma2_without_nu":
            out["grad_sigma2"] = out["grad_sigma2"] / nu[:, None]
        elif mistake == "grad_mu_sign_one_draw":
            out["grad_mu"][3] = -out["grad_mu"][3]
        elif mistake == "grad_d_at_one_row_term":
            out["grad_d"][-1, int(np.flatnonzero(Dd == 0.0)[0])] = 1e-300
        elif mistake == "grad_y_shifted_one_step":
            out["grad_y"] = np.roll(out["grad_y"], 1, axis=1)
        else:
            raise ValueError(mistake)
        return out
    return impl


MISTAKES = {
    # mistake -> (the cases it applies to, the keys it touches)
    "one_grad_a_scaled": (lambda c: len(c[1]) <= 34, ("grad_a",)),
    "grad_c_last_window_dropped": (lambda c: len(c[1]) > 16 and len(c[1]) % 16 and len(c[1]) <= 66, ("grad_c",)),
    "grad_sigma2_without_nu": (lambda c: len(c[1]) <= 34, ("grad_sigma2",)),
    "grad_mu_sign_one_draw": (lambda c: len(c[4]) == 5, ("grad_mu",)),
    "grad_d_at_one_row_term": (lambda c: (c[7] == 0.0).any() and len(c[1]) <= 34, ("grad_d",)),
    "grad_y_shifted_one_step": (lambda c: 2 <= len(c[1]) <= 34, ("grad_y",)),
}


@pytest.mark.parametrize("mistake", sorted(MISTAKES))
def test_the_checker_can_fail(mistake, edge):
    """Each seeded mistake, applied to the complex-step reference's output and fed through check() as an implementation, fails on EVERY edge case
    it applies to (shapes of the N = 3 and 17 rows sweep and the short lengths; no shift) — except one_grad_a_scaled, a relative 1e-10 on one
    term of median size, which must fail wherever 1e-10 of that term exceeds the case's bound and on more than nine cases in ten — while the
    unaltered output passes."""
    applies, keys = MISTAKES[mistake]
    cases = [c for c in edge if c[10] is None and GC.rows(c) <= 63 and applies(c)]
    assert len(cases) >= 20, len(cases)
    caught = []
    for case in cases:
        GC.check(GC.reference_impl("complex_step", True), case, keys=keys)
        try:
            GC.check(_mistaken(mistake), case, keys=keys)
        except AssertionError:
            caught.append(case[0])
    print(f"{mistake}: caught by {len(caught)} of {len(cases)} cases")
    if mistake == "one_grad_a_scaled":
        assert len(caught) > 0.9 * len(cases), (len(caught), len(cases))
    else:
        assert len(caught) == len(cases), sorted(set(c[0] for c in cases) - set(caught))
