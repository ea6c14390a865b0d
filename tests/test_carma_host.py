"""CPU tests (-m "not gpu") of the CARMA(p, q) feature: the new host functions and the numpy twin of the kernels (tools/carma_proto.py) against the
reference's literals (test/test_carma.jl) and against the 100-digit truth (tests/golden/carma_truth.npz), the bars of tests/carma_cases.py — which
must still catch every seeded mistake —, the rejection rules, and the argument checks of the new entries, which need no GPU."""
import ctypes

import numpy as np
import pytest

import carma_cases as cc
import carma_proto as cp
import pioran_jl_amd as pj


def _quad_of_roots(r):
    """the quadratic factors whose quad2roots is r (pairs first, a real root last)"""
    r = np.asarray(r, dtype=complex)
    quad = []
    for k in range(0, len(r) - len(r) % 2, 2):
        quad += [abs(r[k]) ** 2, -2 * r[k].real]
    if len(r) % 2:
        quad.append(-r[-1].real)
    return np.array(quad)


def test_reference_literals_host_functions_and_twin():
    q32 = cc.REF_QUAD2ROOTS32
    np.testing.assert_allclose(pj.quad2roots(q32["qa"]), q32["r"], rtol=1e-8)
    r, _ = cp.roots_of_quad([q32["qa"]], np.zeros((1, 0)))
    np.testing.assert_allclose(r[0], q32["r"], rtol=1e-8)
    c32 = cc.REF_ROOTS2COEFFS32
    alpha = pj.roots2coeffs(c32["r"])
    np.testing.assert_allclose(alpha.real, c32["alpha"], rtol=1e-8)
    assert np.max(np.abs(alpha.imag)) < 1e-15
    _, beta = cp.roots_of_quad(np.ones((1, 1)), [_quad_of_roots(c32["r"])])     # the twin forms the polynomial from the real factors
    np.testing.assert_allclose(beta[0], c32["alpha"], rtol=1e-8)
    m = cc.REF_CARMA32
    model = pj.CARMA(m["p"], m["q"], m["r_alpha"], m["beta"], m["norm"])
    twin = cp.coefs_roots([m["r_alpha"]], [m["beta"]], [m["norm"]], True)
    for got, tw, key in zip(model.celerite_coefs(), twin, "abcd"):
        np.testing.assert_allclose(got, m[key], rtol=1e-8)
        np.testing.assert_allclose(tw[0], m[key], rtol=1e-8)


def test_sample_quad_draws_pass_the_checks():
    """test_sampling_quad of test/test_carma.jl:164-191"""
    rng = np.random.default_rng(1234)
    f_min, f_max = 1e-3, 1e2
    for p in range(1, 6):
        for q in range(1, p):
            for _ in range(3):
                qa, qb = pj.sample_quad(p, q, rng, f_min, f_max)
                assert qa.shape == (p,) and qb.shape == (q,)
                for r in (pj.quad2roots(qa), pj.quad2roots(qb)):
                    assert pj.check_conjugate_pair(r)
                    assert pj.check_roots_bounds(r, f_min, f_max)
                    assert pj.check_order_imag_roots(r)
    assert not pj.check_conjugate_pair(np.array([1 + 1j, 1 - 1j])) and not pj.check_conjugate_pair(np.array([-1 + 1j, -1 - 2j]))
    assert not pj.check_roots_bounds(np.array([-1e-4 + 0j]), f_min, f_max) and not pj.check_roots_bounds(np.array([-1 + 200j]), f_min, f_max)
    assert not pj.check_order_imag_roots(np.array([-1 + 2j, -1 - 2j, -1 + 1j, -1 - 1j]))


def _celerite_psd(f, a, b, c, d):
    """Celerite_psd of src/Celerite.jl:46-51"""
    w = 2 * np.pi * f
    num = (a * c + b * d) * (c ** 2 + d ** 2) + (a * c - b * d) * w ** 2
    den = w ** 4 + 2 * (c ** 2 - d ** 2) * w ** 2 + (c ** 2 + d ** 2) ** 2
    return num / den * 4


@pytest.mark.parametrize("integrated", [False, True])
def test_sum_of_celerite_psds_is_evaluate(integrated):
    """test_CARMA_PSD of test/test_carma.jl:115-141, on the host functions and on the twin"""
    f = 10.0 ** np.linspace(-3, 3, 1000)
    m = cc.REF_CARMA32
    model = pj.CARMA(m["p"], m["q"], m["r_alpha"], m["beta"], 1.0, integrated)
    psd_cel = sum(_celerite_psd(f, *co) for co in zip(*model.celerite_coefs()))
    np.testing.assert_allclose(model.evaluate(f), psd_cel, rtol=1e-8)
    np.testing.assert_allclose(pj.evaluate(model, f), psd_cel, rtol=1e-8)
    assert np.isclose(pj.CARMA_normalisation(model), pj.CARMA_normalisation(model.r_alpha, model.beta))
    twin = cp.evaluate_roots([m["r_alpha"]], [m["beta"]], np.array([1.0]), integrated, f)[0]
    np.testing.assert_allclose(twin, psd_cel, rtol=1e-8)
    np.testing.assert_allclose(cp.evaluate_roots([m["r_alpha"]], [m["beta"]], np.array([1.0]), integrated, f, times_f=True)[0], psd_cel * f, rtol=1e-8)


def test_cases_are_what_the_truth_was_made_from():
    for combo in cc.combos():
        qa, qb, norm = cc.draws(combo)
        t = cc.truth(combo)
        assert np.array_equal(qa, t["qa"]) and np.array_equal(qb, t["qb"]) and np.array_equal(norm, t["norm"])
        assert t["jac"].shape == (cc.N_DRAWS, 4, (combo[0] + 1) // 2, combo[0] + combo[1] + 1) and t["psd"].shape == (cc.N_DRAWS, len(cc.FREQ))


def test_twin_against_truth_within_the_bars():
    print(f"\ndev: coefficients {cc.coef_ref_dev():.3e} (bar {cc.coef_bar():.3e}), vjp {cc.vjp_ref_dev():.3e} (bar {cc.vjp_bar():.3e}), "
          f"psd {cc.psd_ref_dev():.3e} (bar {cc.psd_bar():.3e})")
    for combo in cc.combos():
        t = cc.truth(combo)
        i = bool(combo[2])
        for dtype in (np.float64, np.longdouble):
            dc = cc.coef_deviation(cp.coefs_quad(t["qa"], t["qb"], t["norm"], i, dtype=dtype), t)
            dr = cc.coef_deviation(cp.coefs_roots(t["r_alpha"], t["beta"], t["norm"], i, dtype=dtype), t)
            dp = cc.psd_deviation(cp.evaluate_quad(t["qa"], t["qb"], t["norm"], i, cc.FREQ, dtype=dtype), t)
            qa, qb, norm, g, tv, S = cc.vjp_batch(combo, cc.N_DRAWS)
            dv = cc.vjp_deviation(*cp.vjp_quad(qa, qb, norm, i, *g, dtype=dtype), tv, S)
            print(f"{cc.name(combo):12s} {np.dtype(dtype).name:10s} coefs {dc:.2e} (roots form {dr:.2e})  vjp {dv:.2e}  psd {dp:.2e}")
            assert dc <= cc.coef_bar() and dr <= cc.coef_bar() and dv <= cc.vjp_bar() and dp <= cc.psd_bar()
        # the twin's roots and beta are the truth's
        r, be = cp.roots_of_quad(t["qa"], t["qb"])
        np.testing.assert_allclose(be, t["beta"], rtol=1e-12)
        np.testing.assert_allclose(r.real, t["r_alpha"].real, rtol=1e-14)
    # a zero cotangent gives exact zeros
    qa, qb, norm, g, tv, S = cc.vjp_batch((5, 2, 1), cc.N_DRAWS, zero=True)
    assert all(not np.any(x) for x in cp.vjp_quad(qa, qb, norm, True, *g))


@pytest.mark.parametrize("mistake", cp.MISTAKES)
def test_every_seeded_mistake_exceeds_its_bar(mistake):
    worst = 0.0
    bar = {"vjp_v_const": cc.vjp_bar(), "psd_factor": cc.psd_bar(), "psd_norm_half": cc.psd_bar()}.get(mistake, cc.coef_bar())
    for combo in cc.combos():
        t = cc.truth(combo)
        i = bool(combo[2])
        if mistake == "vjp_v_const":
            qa, qb, norm, g, tv, S = cc.vjp_batch(combo, cc.N_DRAWS)
            dev = cc.vjp_deviation(*cp.vjp_quad(qa, qb, norm, i, *g, mistake=mistake), tv, S)
        elif mistake.startswith("psd"):
            dev = cc.psd_deviation(cp.evaluate_quad(t["qa"], t["qb"], t["norm"], i, cc.FREQ, mistake=mistake), t)
        else:
            dev = cc.coef_deviation(cp.coefs_quad(t["qa"], t["qb"], t["norm"], i, mistake=mistake), t)
        worst = max(worst, dev)
    print(f"\n{mistake}: largest deviation {worst:.3e}, bar {bar:.3e}")
    assert worst > bar


def test_rejection_rules_one_case_each():
    ok_a, ok_b = [2.0, 1.0, 0.5], [3.0, 1.0]          # roots -0.5 +- 1.32i, -0.5 | -0.5 +- 1.66i
    bounds = (1e-3, 1e2)
    cases = [
        (ok_a, ok_b, 1.0, bounds, 0),
        ([np.nan, 1.0, 0.5], ok_b, 1.0, None, 1),      # a non-finite parameter
        (ok_a, ok_b, np.inf, None, 1),                 # ... the norm
        ([1.0, 2.0, 0.5], ok_b, 1.0, None, 2),         # b^2 - 4c = 0: not a conjugate pair
        (ok_a, [0.2, 1.0], 1.0, None, 2),              # ... of the moving-average polynomial, b^2 - 4c > 0
        ([2.0, -1.0, 0.5], ok_b, 1.0, None, 3),        # real part +0.5
        ([2.0, 1.0, -0.5], ok_b, 1.0, None, 3),        # the real root positive
        ([2.0, 1.0, 0.0], ok_b, 1.0, None, 3),         # ... zero
        ([2.0, 1.0, 1e-4], ok_b, 1.0, bounds, 4),      # |Re| below f_lo
        (ok_a, [4e4, 1.0], 1.0, bounds, 4),            # Im above f_hi (moving-average roots)
        ([2.0, 1.0, 1e-4], ok_b, 1.0, None, 0),        # no bounds given: accepted
        ([np.nan, -1.0, 1e-4], ok_b, 1.0, bounds, 1),  # several reasons: the first in the order is reported
    ]
    for qa, qb, norm, b, want in cases:
        assert cp.reject_quad([qa], [qb], norm, b)[0] == want, (qa, qb, norm, b)
    assert cp.reject_quad([[1.0, 2.0, 0.5]], [ok_b], 1.0, None, mistake="reject_ge")[0] == 0     # the seeded mistake of this step is seen by its case
    r = pj.quad2roots(ok_a)
    assert cp.reject_roots([r], [[1.0, 2.0, 1.0]], 1.0, bounds)[0] == 0
    assert cp.reject_roots([r], [[1.0, np.nan, 1.0]], 1.0, bounds)[0] == 1
    assert cp.reject_roots([-np.conj(r)], [[1.0, 2.0, 1.0]], 1.0, None)[0] == 3
    assert cp.reject_roots([r * 1e3], [[1.0, 2.0, 1.0]], 1.0, bounds)[0] == 4


def test_new_entries_refuse_bad_arguments_without_a_gpu():
    L = pj._lib.lib()
    ARG, UNSUPPORTED = -1, -4
    assert L.pioran_abi_version() == 7
    assert L.pioran_carma_coefs_batch(None, 1, 3, 2, 0, None, None, None, 1, 0.0, 0.0, None, None, None, None, None) == ARG
    assert L.pioran_carma_vjp_batch(None, 1, 3, 2, None, None, None, 1, None, None, None, None, None, None, None) == ARG
    assert L.pioran_carma_psd_batch(None, 1, 3, 2, 0, None, None, None, 1, 0.0, 0.0, 1, None, 0, None, None) == ARG
    assert L.pioran_carma_psd_summary(None, 1, 3, 2, 0, None, None, None, 1, 0.0, 0.0, 1, None, 0, 1, None, None, None, None) == ARG
    assert L.pioran_logpdf_batch_carma(None, 1, 3, 2, None, None, None, 1, 0.0, 0.0, *[None] * 9) == ARG
    assert L.pioran_logpdf_batch_carma_grad(None, 1, 3, 2, None, None, None, 1, 0.0, 0.0, *[None] * 15) == ARG
    # with every pointer given the checks go on before anything is dereferenced: the orders, then the bounds
    x = np.ones(64)
    h = v = ctypes.c_void_p(x.ctypes.data)
    for p, q in ((0, 0), (17, 0), (3, 4), (3, -1)):
        assert L.pioran_carma_coefs_batch(h, 1, p, q, 0, v, v, v, 1, 0.0, 0.0, v, v, v, v, v) == UNSUPPORTED
        assert L.pioran_logpdf_batch_carma(h, 1, p, q, v, v, v, 1, 0.0, 0.0, *[v] * 9) == UNSUPPORTED
    assert L.pioran_carma_coefs_batch(h, 0, 3, 2, 0, v, v, v, 1, 0.0, 0.0, v, v, v, v, v) == ARG            # B < 1
    assert L.pioran_carma_coefs_batch(h, 1, 3, 2, 2, v, v, v, 1, 0.0, 0.0, v, v, v, v, v) == ARG            # form
    assert L.pioran_carma_coefs_batch(h, 1, 3, 2, 0, v, v, v, 1, 1.0, 0.5, v, v, v, v, v) == ARG            # f_hi < f_lo
    assert L.pioran_carma_coefs_batch(h, 1, 3, 2, 0, v, None, v, 1, 0.0, 0.0, v, v, v, v, v) == ARG         # qb missing with q > 0
    assert L.pioran_carma_coefs_batch(h, 1, 3, 2, 0, v, v, v, 1, 0.0, 0.0, v, v, v, None, v) == ARG         # an output missing
    assert L.pioran_carma_psd_summary(h, 5000, 3, 2, 0, v, v, v, 1, 0.0, 0.0, 1, v, 0, 1, v, v, None, None) == UNSUPPORTED   # more than 4096 draws
    # the gradient entry: grad_nu without nu; some but not all of the four intermediates
    args = [h, 1, 3, 2, v, v, v, 1, 0.0, 0.0]
    assert L.pioran_logpdf_batch_carma_grad(*args, None, None, None, v, v, v, v, v, v, None, None, None, None, None, None) == ARG
    assert L.pioran_logpdf_batch_carma_grad(*args, None, None, None, v, v, v, v, v, None, None, None, v, None, None, None) == ARG


def test_psd_ppc_carma_size_errors():
    t = np.arange(10.0)
    y = yerr = np.ones(10)
    r = np.tile(pj.quad2roots([2.0, 1.0, 0.5]), (4, 1))
    beta = np.ones((4, 3))
    with pytest.raises(ValueError, match=r"p=2 is not equal to the number of columns in samples_rα=3"):
        pj.psd_ppc_carma(r, beta, np.ones(4), np.ones(4), t, y, yerr, 2, 2)
    with pytest.raises(ValueError, match=r"q\+1=2 is not equal to the number of columns in samples_β=3"):
        pj.psd_ppc_carma(r, beta, np.ones(4), np.ones(4), t, y, yerr, 3, 1)
