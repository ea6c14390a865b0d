"""CPU tests (-m "not gpu") of the forward `approx` behind the device coefficients: the case list and the 50-digit truth of tests/approx_cases.py,
the host mirrors approx_batch / approx_batch_qpo and the numpy restatement of the kernel's own order (tools/approx_proto.py) within the bar the
GPU tests hold the device to (tests/test_gpu_approx_truth.py), every seeded mistake of the restatement beyond that bar, the stored coefficients of
tests/golden/approx_qpo_vjp_truth.npz reproduced by the new restatement, and the conditioning of the end-to-end draws.  Every figure is printed
before it is asserted.

A finding of these tests, fixed with them: written as the reference writes it — the difference of two primitives of size c — the band integral of a
basis function far below the band cancels (c / f_min)^(p - 1) of its digits, seven at c = f_min / 20 for DRWCelerite, and on the J = 2 DRWCelerite
grid with the integrated normalisation, where that term is all of I for a steep spectrum, host mirror and kernel alike deviated by 5.0e6 eps =
1.1e-9 (a) and 8.7e6 eps = 1.9e-9 (b) of the draw's largest |a|; 1.8e4 eps on J = 2 SHO and on J = 3.  Terms with c <= f_min / 2 are now summed
as a series in c / f (psd_device.h psd_band_tail; psd.py _band_tail): 21 eps on those combos, and the seeded mistake "no_tail_series" puts the old
form back and is caught.  docs/EXPERIMENTS.md section 39."""
import importlib.util
import sys
from pathlib import Path

import numpy as np
import pytest

import pioran_jl_amd as pj  # noqa: F401  (the host mirrors, through approx_cases)
from oracle import oracle as O

sys.path.insert(0, str(Path(__file__).resolve().parent))
import approx_cases as AC  # noqa: E402
import qpo_grad_cases as QC  # noqa: E402
import theta_grad_cases as TC  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]
FAR_BELOW = 1e-11            # "far below the present 1e-9": two orders


def _tool(name):
    sys.path.insert(0, str(ROOT / "tools"))
    spec = importlib.util.spec_from_file_location(name, ROOT / "tools" / f"{name}.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


T = _tool("approx_proto")


def _proto(combo, mistake=None):
    m, b, i, J, nq, n, lo, hi = combo
    t = AC.truth(combo)
    return T.approx(m, t["theta"], t["norm"], t["qpo"], AC.F_MIN, AC.F_MAX, J, lo, hi, is_integrated_power=bool(i), basis=b, mistake=mistake)


def test_case_list_holds_what_it_promises():
    cs = AC.combos()
    assert len(set(cs)) == len(cs) and len({AC.name(c) for c in cs}) == len(cs)
    std = (TC.S_LOW, TC.S_HIGH)
    # continuum: theta_grad_cases' combos, all of them, and one more grid per basis
    assert [c[:4] + c[5:6] for c in AC.continuum_combos() if c[6:] == std and c not in AC.CHAINED] == TC.combos()
    assert {c[:4] for c in cs if c[4] == 0 and c[5] == 6 and c[6:] == std} == \
        {(m, b, i, J) for J in (2, 3, 20, 33) for m in (0, 1) for b in (0, 1) for i in (0, 1)}
    assert {c[:5] for c in cs if c[4] == 0 and c[5] == 2} == {(0, 0, 1, 48, 0), (1, 0, 1, 48, 0), (0, 1, 1, 72, 0), (1, 1, 1, 72, 0), (0, 0, 1, 60, 0)}
    other = [c for c in cs if c[6:] != std]
    assert sorted(c[1] for c in other) == [0, 1] and all(c[3] == 20 and c[4] == 0 for c in other)
    assert all(lo != hi and lo != 20.0 and hi != 20.0 for *_, lo, hi in other)
    # features: qpo_grad_cases' combos, all of them, and n_qpo = 8 in both normalisations
    assert [c[:6] for c in AC.qpo_combos() if AC.stored(c)] == QC.combos()
    assert [c[:5] for c in AC.qpo_combos() if not AC.stored(c)] == [(0, 0, 1, 20, 8), (0, 0, 0, 20, 8)]
    assert {c[4] for c in cs} == {0, 1, 2, 8} and {c[3] for c in cs} == {2, 3, 20, 33, 48, 60, 72}
    assert AC.LAUNCH_B == (1, 63, 64, 65, 130)
    # the grids that reach the row interchanges of the forward solve, and those that do not
    assert T.interchanges(48, 0) > 0 and T.interchanges(72, 1) > 0
    assert T.interchanges(47, 0) == 0 and T.interchanges(71, 1) == 0 and T.interchanges(33, 0) == 0 and T.interchanges(33, 1) == 0
    # ... in an order that matters: at J = 48 and 72 the interchanges are of disjoint pairs of rows, at J = 60 they share rows
    for J, b, matters in ((48, 0, False), (72, 1, False), (59, 0, False), (60, 0, True)):
        piv = T.setup(J, b, AC.F_MIN, AC.F_MAX)[2]
        fwd, rev = np.arange(J), np.arange(J)
        for j in range(J):
            fwd[[j, piv[j]]] = fwd[[piv[j], j]]
        for j in range(J - 1, -1, -1):
            rev[[j, piv[j]]] = rev[[piv[j], j]]
        assert (not np.array_equal(fwd, rev)) == matters, (J, b)
    assert AC.CHAINED == ((0, 0, 1, 60, 0, 2, *std),)
    vp = _tool("approx_vjp_proto")
    assert T.interchanges(48, 0) == vp.interchanges(48, 0) and T.interchanges(72, 1) == vp.interchanges(72, 1)
    # the subsets the GPU tests name
    assert all(c in cs for c in AC.PLACE_COMBOS + AC.END_TO_END)
    assert [(c[3], c[1], c[4], c[2]) for c in AC.PLACE_COMBOS] == [(3, 0, 1, 1), (20, 1, 2, 1), (20, 0, 2, 0), (48, 0, 1, 1)]
    assert [(c[0], c[1], c[3], c[4]) for c in AC.END_TO_END] == [(0, 0, 20, 0), (1, 1, 3, 0), (0, 0, 20, 1)]
    # what the forward entry takes with features: all but the 98 rows of SHO J = 48 with a feature
    assert [AC.name(c) for c in AC.qpo_combos() if not AC.forward_entry_takes(c)] == ["m0_b0_i1_J48_q1"]
    assert AC.state_rows((0, 1, 1, 72, 0, 2, *std)) == 216 and AC.state_rows(AC.N_QPO_MAX[0]) == 56


def test_truth_file_matches_the_draws():
    keys = set()
    for c in AC.combos():
        m, b, i, J, nq, n, lo, hi = c
        th, nm, qp = AC.draws(c)
        t = AC.truth(c)
        Jc, Jt = AC.widths(c)
        assert np.array_equal(th, t["theta"]) and np.array_equal(nm, t["norm"]), AC.name(c)
        assert th.shape == (n, 3 if m == 0 else 5)
        assert (qp is None and t["qpo"] is None) if nq == 0 else (qp.shape == (n, nq, 3) and np.array_equal(qp, t["qpo"]))
        for k in "ABCD":
            assert t[k].shape == (n, Jt) and np.isfinite(t[k]).all(), (AC.name(c), k)
        assert t["x"].shape == (n, J) and t["I"].shape == (n,) and np.isfinite(t["x"]).all() and (t["I"] > 0).all()
        # the draws' edges
        assert th[1, 0] < 0 and (n <= 3 or (th[2, 1] == AC.F_MIN and th[3, 1] == AC.F_MAX)) and (m == 0 or th[0, 3] == 1.05 * th[0, 1])
        # the continuum's (c, d) are the grid's, the same in every row; the structural zeros are zeros
        assert (t["C"][:, :Jc] == t["C"][0, :Jc]).all() and (t["D"][:, :Jc] == t["D"][0, :Jc]).all()
        if b == 1:
            assert not t["B"][:, J:Jc].any() and not t["D"][:, J:Jc].any() and np.array_equal(t["A"][:, :J], t["A"][:, J:Jc])
        else:
            assert np.array_equal(t["A"][:, :Jc], t["B"][:, :Jc]) and np.array_equal(t["C"][:, :Jc], t["D"][:, :Jc])
        # the coefficients are the amplitudes scaled: a_j = kappa_j x_j norm / I, to the rounding of the stored values
        kap = np.pi / np.sqrt(2) if b == 0 else np.pi / 3
        grid = t["C"][0, :J] / (np.sqrt(2) * np.pi if b == 0 else np.pi)
        np.testing.assert_allclose(t["A"][:, :J], kap * grid * t["x"] * (t["norm"] / t["I"])[:, None], rtol=16 * AC.EPS, atol=0)
        f0, fM = AC.F_MIN / lo, AC.F_MAX * hi
        np.testing.assert_allclose(grid[[0, -1]], [f0, fM], rtol=4 * AC.EPS)
        keys |= {f"{AC.name(c)}/{k}" for k in ("theta", "norm", "x", "I") + (("qpo",) if nq else ()) + (() if AC.stored(c) else tuple("ABCD"))}
    assert set(AC._file()) == keys                     # values only: no Jacobians, and no second copy of the stored coefficients
    assert (ROOT / "tests" / "golden" / "approx_truth.npz").stat().st_size < 512 * 1024


@pytest.mark.parametrize("combo", [c for c in AC.combos() if AC.stored(c)], ids=AC.name)
def test_stored_qpo_truth_is_reproduced(combo):
    """the new 50-digit restatement gives, bit for bit, the A .. D that tools/make_approx_qpo_vjp_truth.py stored"""
    M = _make_truth()
    assert M.reproduces_stored(combo)


_made = []


def _make_truth():
    if not _made:
        _made.append(_tool("make_approx_truth"))
    return _made[0]


@pytest.mark.parametrize("combo", AC.combos(), ids=AC.name)
def test_reference_deviation_is_positive_and_far_below_the_parity_bar(combo):
    """ref_dev of the bar: the host mirror against the truth: at most 90 eps up to J = 33 and with features, 2.2e3 eps = 5e-13 on the pivoting
    grids (through the amplitudes)"""
    dev = AC.ref_dev(combo)
    print(f"{AC.name(combo)}: host mirror against the 50-digit truth: " + "  ".join(f"{k} {v:.3e} ({v / AC.EPS:.1f} eps)" for k, v in dev.items()))
    assert set(dev) == ({"a", "b", "gc", "gd"} | ({"qc", "qd"} if combo[4] else set()))
    assert dev["a"] > 0.0 and dev["b"] > 0.0
    assert all(np.isfinite(v) for v in dev.values())
    assert max(dev.values()) <= FAR_BELOW


@pytest.mark.parametrize("combo", AC.combos(), ids=AC.name)
def test_host_mirror_and_proto_within_the_bar(combo):
    got = _proto(combo)
    AC.check(combo, AC.host_mirror(combo), leg="host mirror")
    AC.check(combo, got, leg="proto")
    t = AC.truth(combo)
    dx = np.max(np.abs(got["x"] - t["x"]).max(axis=1) / np.abs(t["x"]).max(axis=1))
    dI = np.max(np.abs(got["I"] - t["I"]) / t["I"])
    print(f"{AC.name(combo)} proto stages: amplitudes {dx / AC.EPS:.1f} eps of the largest, integral {dI / AC.EPS:.1f} eps")
    # the proto's grid is the one the entry hands on: (c, d) in every row, zeros where the term has one row
    Jc = AC.widths(combo)[0]
    assert (got["c"][:, :Jc] == got["c"][0, :Jc]).all() and (got["d"][:, :Jc] == got["d"][0, :Jc]).all()


@pytest.mark.parametrize("mistake", T.MISTAKES)
def test_seeded_mistake_exceeds_the_bar(mistake):
    worst, where, caught = 0.0, None, []
    for combo in AC.combos():
        dev = {k: float(v.max()) for k, v in AC.deviations(combo, _proto(combo, mistake)).items()}
        bars = AC.bar(combo)
        over = {k: v / bars[k] for k, v in dev.items() if v > bars[k]}
        if over:
            caught.append(AC.name(combo))
            k = max(over, key=over.get)
            if over[k] > worst:
                worst, where = over[k], (AC.name(combo), k, dev[k], bars[k])
    print(f"{mistake}: beyond the bar on {len(caught)} of {len(AC.combos())} combos; worst {where[1]} of {where[0]}: deviation {where[2]:.3e}, "
          f"bar {where[3]:.3e} ({worst:.3g} x)" if caught else f"{mistake}: not caught")
    assert caught


def test_difference_of_sums_costs_no_digits_against_per_term_differences():
    """psd_norm_integral forms hi - lo from two sums over the terms, not from per-term differences.  Measured here on the truth's amplitudes, in
    the kernel's arithmetic, with the terms far below the band through their series in both: 9.2 | 9.2 eps on the small grids, 11.3 | 3.8 eps from
    J = 20 on — the two sums cost nothing that shows beside the 100 .. 2e3 eps the amplitudes carry there."""
    worst = {(form, wide): 0.0 for form in ("sums", "per term") for wide in (False, True)}
    for combo in AC.continuum_combos():
        m, b, i, J, nq, n, lo, hi = combo
        if not i:
            continue
        t = AC.truth(combo)
        sp = T.setup(J, b, AC.F_MIN, AC.F_MAX, lo, hi)[0]
        x = np.ascontiguousarray(t["x"].T)
        got = {"sums": T.norm_integral(b, True, AC.F_MIN, AC.F_MAX, sp, x),
               "per term": sum(T.norm_integral(b, True, AC.F_MIN, AC.F_MAX, sp[j:j + 1], x[j:j + 1]) for j in range(J))}
        for form, v in got.items():
            worst[form, J >= 20] = max(worst[form, J >= 20], float(np.max(np.abs(v - t["I"]) / t["I"])))
    for wide in (False, True):
        print(f"normalising integral on the truth's amplitudes, J {'>= 20' if wide else '<= 3'}: hi - lo of two sums "
              f"{worst['sums', wide] / AC.EPS:.1f} eps, per-term differences {worst['per term', wide] / AC.EPS:.1f} eps")
        assert worst["sums", wide] <= max(AC.MARGIN * worst["per term", wide], AC.FLOOR)     # the same sums in another order


@pytest.mark.parametrize("variant", AC.E2E_VARIANTS)
@pytest.mark.parametrize("combo", AC.END_TO_END, ids=AC.name)
def test_end_to_end_draws_are_well_conditioned(golden_dir, combo, variant):
    """every draw of the end-to-end cases has status 0 in the fp64 oracle and ratio = nu min(sigma2) / sum(a) >= 1e-5, in every variant, and its
    log L (the truth, dense in long double) is at least 0.02 of the sum of its absolute terms: a bar relative to |log L| means something"""
    t, y, s2 = AC.e2e_series(golden_dir, combo)
    tr = AC.truth(combo)
    mu, nu, shift = AC.e2e_extras(combo, variant)
    for k in range(combo[5]):
        yk, sk = AC.e2e_draw_series(y, s2, mu, nu, shift, k)
        v, st = O.logl(tr["A"][k], tr["B"][k], tr["C"][k], tr["D"][k], t, yk, sk, return_status=True)
        ratio = sk.min() / tr["A"][k].sum()
        nll, scale = O.dense_nll_truth(tr["A"][k], tr["B"][k], tr["C"][k], tr["D"][k], t, yk, sk)
        print(f"{AC.name(combo)} {variant} draw {k}: oracle.logl {v:.6f} status {st} ratio {ratio:.2e}   |truth| / sum of |terms| {abs(nll) / scale:.3f}")
        assert st == 0 and np.isfinite(v) and ratio >= 1e-5
        assert abs(nll) >= 0.02 * scale and abs(v + float(nll)) <= 1e-9 * float(scale)
    if variant == "shift":                                 # the scale is the smallest power of ten that does it
        lowest = min(AC.e2e_draw_series(y, s2, mu, nu, shift, k)[1].min() / tr["A"][k].sum() for k in range(combo[5]))
        assert lowest < 1e-4
