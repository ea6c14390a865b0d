"""CPU tests of the PSD check (psd_check.hip's definition): the host function pj.approximated_psd and the numpy twin tools/psd_check_proto.py against
the reference's own assertions on its literal inputs, against the oracle's amplitudes and normalising integral, and against the 50-digit truth
tests/golden/psd_check_truth.npz — which must also catch every mistake the twin can seed.  Argument validation of the three C entries without a
GPU.  Cases and bar: tests/psd_check_cases.py."""
import ctypes
import json

import numpy as np
import pytest

import pioran_jl_amd as pj
import psd_check_cases as PC
from oracle import oracle as O

P = PC.PROTO
REF = json.loads((PC.ROOT / "tests" / "golden" / "psd_check_reference_inputs.json").read_text())


def _reference_grid():
    return 10.0 ** np.linspace(np.log10(REF["f0"]), np.log10(REF["fM"]), REF["n_frequencies"])


@pytest.mark.parametrize("basis", ["SHO", "DRWCelerite"])
def test_reference_relation_on_its_literal_inputs(basis):
    """test/test_psd.jl:54-55, :93-94: max |P(f)/P(f_1) - approx/approx_1| < 1 and every point within atol = 1e-2, for the ten parameter sets of
    each basis — on the host function and on the twin (f_min = f0, f_max = fM, S_low = S_high = 1, norm = 1)."""
    r, f = REF[basis], _reference_grid()
    worst = 0.0
    for a1, f1, a2 in zip(r["alpha1"], r["f1"], r["alpha2"]):
        model = pj.SingleBendingPowerLaw(a1, f1, a2)
        want = model(f) / model(f[0])
        host = pj.approximated_psd(f, model, REF["f0"], REF["fM"], n_components=r["n_components"], basis_function=basis)
        tw = P.psd_check(0, [[a1, f1, a2]], 1.0, f, REF["f0"], REF["fM"], 1.0, 1.0, r["n_components"], PC.BASIS_NAME.index(basis))
        assert tw["status"][0] == 0
        for got in (host, tw["psd_approx"][0]):
            dev = np.abs(want - got / got[0])
            worst = max(worst, float(dev.max()))
            assert dev.max() < REF["max_bound"]
            assert np.all(dev <= REF["atol"])
        # the twin's model PSD is the reference's P(f) / P(f[1]) * norm
        assert np.max(np.abs(tw["psd"][0] - want) / want) < 8 * np.finfo(float).eps
    print(f"{basis}: worst |P/P_1 - approx/approx_1| over the ten sets = {worst:.2e} (bound {REF['atol']})")


def test_host_function_components_and_sum():
    f = _reference_grid()[::50]
    model = pj.DoubleBendingPowerLaw(0.3, 0.02, 1.4, 10.2, 2.93)
    comps = pj.approximated_psd(f, model, 2e-3, 352.0, n_components=12, norm=2.5, basis_function="DRWCelerite", individual=True)
    total = pj.approximated_psd(f, model, 2e-3, 352.0, n_components=12, norm=2.5, basis_function="DRWCelerite")
    assert comps.shape == (len(f), 12)
    acc = np.zeros(len(f))
    for j in range(12):
        acc = acc + comps[:, j]
    assert np.array_equal(acc, total)
    amp = pj.get_approx_coefficients(model, 2e-3, 352.0, 12, "DRWCelerite")
    sp, _ = pj.build_approx(12, 2e-3, 352.0, "DRWCelerite")
    assert np.allclose(comps, amp * 2.5 / (1 + (f[:, None] / sp) ** 6), rtol=1e-13, atol=0)
    with pytest.raises(ValueError):
        pj.approximated_psd(f, model, 2e-3, 352.0, basis_function="Matern")


def test_amplitudes_and_integral_equal_the_oracle():
    g = REF["get_coefs"]
    th = np.array([g["theta"]])
    golden = np.array(g["amplitudes"])
    model = pj.SingleBendingPowerLaw(*g["theta"])
    for basis in (0, 1):
        for integrated in (1, 0):
            tw = P.psd_check(0, th, 1.0, [g["f0"]], g["f0"], g["fM"], 1.0, 1.0, g["n_components"], basis, integrated=integrated, normalise=1)
            want = O.get_approx_coefficients(model, g["f0"], g["fM"], g["n_components"], PC.BASIS_NAME[basis])
            # (the same solve of the same matrix up to the last bit of the grid points: vectorised against scalar pow)
            assert np.max(np.abs(tw["amplitudes"][0] - want)) <= 1e-11 * np.max(np.abs(want))
            sp, _ = O.build_approx(g["n_components"], g["f0"], g["fM"], PC.BASIS_NAME[basis])
            integ = O.get_norm_psd(want, sp, g["f0"], g["fM"], PC.BASIS_NAME[basis], bool(integrated))
            assert abs(tw["integ"][0] - integ) <= 4 * np.finfo(float).eps * abs(integ)
    tw = P.psd_check(0, th, 1.0, [g["f0"]], g["f0"], g["fM"], 1.0, 1.0, g["n_components"], 0)
    # test/test_psd.jl:38 (isapprox of two vectors: the norm of the difference against sqrt(eps) times the larger norm)
    assert np.linalg.norm(tw["amplitudes"][0] - golden) <= np.sqrt(np.finfo(float).eps) * max(np.linalg.norm(golden), np.linalg.norm(tw["amplitudes"][0]))
    # the long-double twin (its own elimination) agrees with the fp64 one to the conditioning of the grid
    lw = P.psd_check(0, th, 1.0, [g["f0"]], g["f0"], g["fM"], 1.0, 1.0, g["n_components"], 0, dtype=np.longdouble)
    assert np.max(np.abs(lw["amplitudes"][0] - tw["amplitudes"][0])) <= 1e-10 * np.max(np.abs(golden))


@pytest.mark.parametrize("case", PC.cases(), ids=PC.name)
def test_twin_against_the_truth(case):
    """fp64 twin within a few thousand eps of the 50-digit truth in every array's natural scale (printed: these deviations set the bar of the GPU
    tests), the long-double twin far closer, and the inputs of the truth file are the case table's."""
    t = PC.truth(case)
    th, nm = PC.draws(case)
    assert np.array_equal(t["theta"], th) and np.array_equal(t["norm"], nm) and np.array_equal(t["freq"], PC.freqs(case))
    tw = PC.twin(case)
    assert (tw["status"] == 0).all()
    dev = PC.deviations(tw, t)
    ldev = PC.deviations(PC.twin(case, dtype=np.longdouble), t)
    print(PC.name(case), "fp64 twin:", {k: f"{v:.2e}" for k, v in dev.items()}, "long double:", {k: f"{v:.2e}" for k, v in ldev.items()})
    for n in PC.ARRAYS:
        assert dev[n] < 1e-9, (n, dev[n])         # cond(B) eps: 1e-11 at J = 35
        assert ldev[n] < 1e-12, (n, ldev[n])      # (the stored truth is rounded to fp64: 1.1e-16 is the least a deviation can be)


@pytest.mark.parametrize("mistake", P.MISTAKES)
def test_every_seeded_mistake_is_caught_by_the_truth(mistake):
    """In every case where the mistake changes the definition, it moves at least one array beyond the bar the GPU tests use."""
    applied = 0
    for case in PC.cases():
        m, b, J, B, F, i, n, tf = case
        if not {"integ_model_only": n == 1, "times_f_residuals": tf == 1}.get(mistake, True):
            continue
        applied += 1
        dev = PC.deviations(PC.twin(case, mistake=mistake), PC.truth(case))
        bars = PC.bars(case)
        over = [k for k in PC.ARRAYS + ("amplitudes",) if not dev[k] <= bars[k]]
        assert over, (PC.name(case), mistake, dev)
    assert applied >= 2


def test_status_and_nan_rows_of_the_twin():
    case = PC.cases()[1]
    m, b, J, B, F, i, n, tf = case
    th, nm = PC.draws(case)
    th, nm = th[:6].copy(), nm[:6].copy()
    th[1, 2] = np.nan
    nm[3] = np.inf
    th[4, 0], th[4, 1] = 400.0, 1e-3 * 1e-3    # P(freq_0) = (f / f1)^-400 / (...) underflows to 0
    f = PC.freqs(case)
    f[0] = 10.0
    r = P.psd_check(m, th, nm, f, PC.F_MIN, PC.F_MAX, PC.S_LOW, PC.S_HIGH, J, b, integrated=i, normalise=n)
    assert r["status"].tolist() == [0, 2, 0, 2, 2, 0]
    for k in PC.ARRAYS + ("amplitudes", "integ"):
        assert np.isnan(r[k][[1, 3, 4]]).all() and np.isfinite(r[k][[0, 2, 5]]).all(), k
    quant, mean, meta, kept = P.summary(r, r["status"], [0.5])
    assert kept == 3 and np.isnan(meta[[1, 3, 4]]).all() and np.isfinite(meta[[0, 2, 5]]).all() and np.isfinite(quant).all()


def test_argument_validation_without_gpu():
    """NULL ctx, and everything else that is refused before any GPU call, is PIORAN_ERR_ARG in the three entries."""
    L = pj._lib.lib()
    th, nm, fr = np.array([[0.3, 0.02, 2.9]]), np.ones(1), np.array([1e-3, 1e-2])
    out = np.empty((1, 2))
    pr = np.array([0.5])
    p = lambda a: ctypes.c_void_p(a.ctypes.data)   # noqa: E731
    fake = ctypes.c_void_p(8)                       # a context that is never dereferenced: every call below is refused first
    head = (1, 0, 20, 0, 1, 1e-3, 1.0, 20.0, 20.0)
    for fn, tail in ((L.pioran_psd_check_batch, (p(out), None, None, None, None, None, None)),
                     (L.pioran_psd_check_batch_dev, (p(out), None, None, None, None, None, None)),
                     (L.pioran_psd_check_summary, (1, p(pr), p(out), None, None, None, None))):
        assert fn(None, *head, p(th), p(nm), 2, p(fr), 0, 0, *tail) == -1
        assert fn(fake, *head, None, p(nm), 2, p(fr), 0, 0, *tail) == -1
        assert fn(fake, *head, p(th), None, 2, p(fr), 0, 0, *tail) == -1
        assert fn(fake, *head, p(th), p(nm), 2, None, 0, 0, *tail) == -1
        assert fn(fake, *head, p(th), p(nm), 0, p(fr), 0, 0, *tail) == -1
        assert fn(fake, 0, *head[1:], p(th), p(nm), 2, p(fr), 0, 0, *tail) == -1
        for bad in ((1, 2, 20, 0, 1, 1e-3, 1.0, 20.0, 20.0), (1, 0, 1, 0, 1, 1e-3, 1.0, 20.0, 20.0), (1, 0, 257, 0, 1, 1e-3, 1.0, 20.0, 20.0),
                    (1, 0, 20, 2, 1, 1e-3, 1.0, 20.0, 20.0), (1, 0, 20, 0, 1, 1.0, 1.0, 20.0, 20.0), (1, 0, 20, 0, 1, -1e-3, 1.0, 20.0, 20.0),
                    (1, 0, 20, 0, 1, 1e-3, np.inf, 20.0, 20.0), (1, 0, 20, 0, 1, 1e-3, 1.0, 0.0, 20.0), (1, 0, 20, 0, 1, 1e-3, 1.0, 20.0, np.nan)):
            assert fn(fake, *bad, p(th), p(nm), 2, p(fr), 0, 0, *tail) == -1, bad
    none7 = (None,) * 7
    assert L.pioran_psd_check_batch(fake, *head, p(th), p(nm), 2, p(fr), 0, 0, *none7) == -1          # all outputs NULL
    assert L.pioran_psd_check_batch_dev(fake, *head, p(th), p(nm), 2, p(fr), 0, 0, *none7) == -1
    assert L.pioran_psd_check_summary(fake, *head, p(th), p(nm), 2, p(fr), 0, 0, 1, p(pr), None, None, None, None, None) == -1
    for badf in (np.array([1e-3, 0.0]), np.array([1e-3, -1.0]), np.array([np.nan, 1.0]), np.array([1e-3, np.inf])):
        assert L.pioran_psd_check_batch(fake, *head, p(th), p(nm), 2, p(badf), 0, 0, p(out), None, None, None, None, None, None) == -1
        assert L.pioran_psd_check_summary(fake, *head, p(th), p(nm), 2, p(badf), 0, 0, 1, p(pr), p(out), None, None, None, None) == -1
    for badp in (np.array([1.5]), np.array([-0.1]), np.array([np.nan])):
        assert L.pioran_psd_check_summary(fake, *head, p(th), p(nm), 2, p(fr), 0, 0, 1, p(badp), p(out), None, None, None, None) == -1
    assert L.pioran_psd_check_summary(fake, *head, p(th), p(nm), 2, p(fr), 0, 0, 0, p(pr), p(out), None, None, None, None) == -1
    assert L.pioran_psd_check_summary(fake, *head, p(th), p(nm), 2, p(fr), 0, 0, 1, None, p(out), None, None, None, None) == -1
    # the summary form's limit comes after the argument checks and before any GPU call
    big = np.ones(4097)
    assert L.pioran_psd_check_summary(fake, 4097, *head[1:], p(np.ones((4097, 3))), p(big), 2, p(fr), 0, 0, 1, p(pr), p(out), None, None, None, None) == -4
    assert L.pioran_psd_check_summary(fake, *head, p(th), p(nm), 4097, p(big), 0, 0, 1, p(pr), p(out), None, None, None, None) == -4


def test_host_reduction_of_the_python_layer_is_the_quantile_twin():
    """pj.run_diagnostics and pj.psd_ppc reduce on the host above 4096 draws: that reduction is tools/quantiles_proto.py's, bit for bit."""
    gp = pj.gp
    QP = P._quantiles_proto()
    rng = np.random.default_rng(5)
    X = rng.standard_normal((37, 11)) * 10.0 ** rng.uniform(-3, 3, 11)
    X[:, 3] = X[0, 3]
    st = (rng.uniform(size=37) < 0.2).astype(np.int32) * 2
    for status in (None, st):
        q, mean, kept = gp._quantiles_host(X, [0.0, 0.025, 0.5, 0.84, 1.0], status)
        wq, wmean, wkept = QP.quantiles(X, [0.0, 0.025, 0.5, 0.84, 1.0], status=status)
        assert kept == wkept and np.array_equal(q, wq) and np.array_equal(mean, wmean)
    q, mean, kept = gp._quantiles_host(X[:1], [0.3], None)
    assert np.array_equal(q[0], X[0]) and kept == 1
