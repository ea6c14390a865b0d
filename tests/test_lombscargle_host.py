"""CPU tests (-m "not gpu") of the batched Lomb-Scargle periodogram: the numpy twin of periodogram.hip (tools/lombscargle_proto.py) in fp64
against itself in long double and against an independent implementation, the argument checks of the two C entries and the host-side API.

Inputs: (t, y, yerr) of tests/golden/simu.txt, as prefixes of 5, 37, 130 rows and the whole file; frequencies by the reference's recipe
(src/plots_diagnostics.jl:522-528, :545) applied to the series under test: log-spaced between f_min / 20 and 20 f_max, last point dropped.
Every case first asserts that the long-double determinant D is at least 1e-8 at every frequency (minimum over the four cases: 4.0e-8 at
(37, 70)) — the power divides by D, and the bound below presumes it is not small.

Bound: 1e-10 absolute (the power lies in [0, 1]) = 10 x the worst deviation of the fp64 twin from the long-double twin on these cases
(the twin measures 3.3e-14, 2.7e-11, 1.8e-11, 1.9e-12; an evaluation with another order of the sums 6.6e-13, 1.1e-11, 3.0e-12, 2.1e-12).

What pins the semantics: the reference's LombScargle.jl cannot be run here, so the published formulas (Zechmeister & Kuerster 2009, time-shift-free
form — LombScargle.jl's defaults fit_mean = true, center_data = true, normalization = :standard) and the relation to
scipy.signal.lombscargle(t, y - Ybar_w, 2 pi freq, weights = w, floating_mean = True, normalize = True), an implementation that shares no
code with the twin, are what the twin is held against (5e-12 on the full file)."""
import ctypes
import importlib.util
from pathlib import Path

import numpy as np
import pytest

import pioran_jl_amd as pj

ROOT = Path(__file__).resolve().parents[1]
BOUND = 1e-10
D_MIN = 1e-8
SHAPES = [(5, 3), (37, 70), (130, 33), (None, 199)]


def _proto():
    spec = importlib.util.spec_from_file_location("lombscargle_proto", ROOT / "tools" / "lombscargle_proto.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


P = _proto()
_CACHE = {}


def _case(golden_dir, N, F):
    """(t, y, yerr, freq, long-double power of y) of a shape, computed once; the determinant precondition is asserted here"""
    key = (N, F)
    if key not in _CACHE:
        A = np.loadtxt(golden_dir / "simu.txt")
        A = A if N is None else A[:N]
        t, y, yerr = (np.ascontiguousarray(A[:, k]) for k in range(3))
        freq = P.reference_grid(t, F + 1)[:-1]
        D = P.frequency_terms(t, yerr, freq, True, np.longdouble)[-1]
        assert len(D) == F and np.all(D >= D_MIN), float(D.min())
        _CACHE[key] = (t, y, yerr, freq, P.lombscargle(t, y, yerr, freq, dtype=np.longdouble))
    return _CACHE[key]


@pytest.mark.parametrize("N,F", SHAPES)
def test_fp64_twin_against_long_double(golden_dir, N, F):
    t, y, yerr, freq, ref = _case(golden_dir, N, F)
    got = P.lombscargle(t, y, yerr, freq)
    assert got.dtype == np.float64 and got.shape == (F,)
    err = float(np.max(np.abs(got - ref)))
    print(f"N = {len(t)}, F = {F}: max |fp64 - long double| = {err:.2e}")
    assert err <= BOUND, err
    assert np.all(ref >= 0) and np.all(ref <= 1)
    # batch form, without errors, and the other (fit_mean, center_data) combinations: the same twin in both types
    Y = np.stack([y, y[::-1], y * 2 + 1])
    for ye in (yerr, None):
        for fm in (True, False):
            for cd in (True, False):
                a = P.lombscargle(t, Y, ye, freq, fm, cd)
                b = P.lombscargle(t, Y, ye, freq, fm, cd, dtype=np.longdouble)
                assert a.shape == (3, F) and float(np.max(np.abs(a - b))) <= BOUND, (ye is None, fm, cd)


@pytest.mark.parametrize("N,F", SHAPES)
def test_fp64_twin_against_scipy(golden_dir, N, F):
    """The twin against scipy.signal.lombscargle with a floating mean and weights — an independent implementation of the generalised
    periodogram (the reference's LombScargle.jl is not available to the tests: this relation and the published formulas pin the semantics)."""
    from scipy import signal
    t, y, yerr, freq, ref = _case(golden_dir, N, F)
    w = yerr ** -2.0 / np.sum(yerr ** -2.0)
    sp = signal.lombscargle(t, y - np.sum(w * y), 2 * np.pi * freq, weights=w, floating_mean=True, normalize=True)
    got = P.lombscargle(t, y, yerr, freq)
    err = float(np.max(np.abs(got - sp)))
    print(f"N = {len(t)}, F = {F}: max |twin - scipy| = {err:.2e}")
    assert err <= BOUND, err


@pytest.mark.parametrize("N,F", SHAPES)
def test_offset_series_needs_centring(golden_dir, N, F):
    """y + 1000 has the periodogram of y; an evaluation that projects the raw series and subtracts Ybar C afterwards is off by 1.7e-9"""
    t, y, yerr, freq, ref = _case(golden_dir, N, F)
    got = P.lombscargle(t, y + 1000.0, yerr, freq)
    err = float(np.max(np.abs(got - ref)))
    print(f"N = {len(t)}, F = {F}: max |fp64(y + 1000) - long double(y)| = {err:.2e}")
    assert err <= BOUND, err
    # with a fitted mean the offset is taken off also when centring is not asked for (the power does not depend on it)
    assert float(np.max(np.abs(P.lombscargle(t, y + 1000.0, yerr, freq, True, False) - ref))) <= BOUND


def test_argument_checks_without_gpu():
    """Every PIORAN_ERR_ARG case of the two entries returns -1 before any GPU call (no context can exist here: a bad-argument call with a
    non-NULL context is made with a dummy handle that must never be dereferenced)."""
    L = pj._lib.lib()
    v = ctypes.c_void_p
    N, B, F = 4, 2, 3
    t = np.array([0.0, 1.0, 2.5, 4.0]); Y = np.ones((B, N)); yerr = np.full(N, 0.1); freq = np.array([0.1, 0.2, 0.3])
    power = np.empty((B, F)); st = np.zeros(B, dtype=np.int32)
    p = lambda a: None if a is None else v(a.ctypes.data)
    dummy = v(ctypes.addressof(ctypes.create_string_buffer(4096)))

    def host(ctx=dummy, N=N, B=B, F=F, t=t, Y=Y, yerr=yerr, freq=freq, power=power):
        return L.pioran_lombscargle_batch(ctx, N, B, F, p(t), p(Y), p(yerr), p(freq), 1, 1, p(power), p(st))

    def dev(ctx=dummy, N=N, B=B, F=F, t=t, Y=Y, yerr=yerr, freq=freq, power=power):
        return L.pioran_lombscargle_batch_dev(ctx, N, B, F, p(t), p(Y), p(yerr), p(freq), 1, 1, p(power), p(st))

    for f in (host, dev):
        assert f(ctx=None) == -1
        for name in ("t", "Y", "freq", "power"):
            assert f(**{name: None}) == -1, name
        assert f(N=2) == -1 and f(B=0) == -1 and f(F=0) == -1
    # what only the host form can look at
    for bad in (np.nan, np.inf):
        tb = t.copy(); tb[2] = bad
        assert host(t=tb) == -1
        fb = freq.copy(); fb[1] = bad
        assert host(freq=fb) == -1
        eb = yerr.copy(); eb[3] = bad
        assert host(yerr=eb) == -1
    for bad in (0.0, -1.0):
        fb = freq.copy(); fb[0] = bad
        assert host(freq=fb) == -1
        eb = yerr.copy(); eb[0] = bad
        assert host(yerr=eb) == -1
    assert L.pioran_abi_version() == 7


def test_public_api_on_the_host(golden_dir):
    A = np.loadtxt(golden_dir / "simu.txt")
    t, y, yerr = A[:, 0], A[:, 1], A[:, 2]
    with pytest.raises(ValueError, match="standard.*model.*log"):
        pj.lombscargle(t, y, yerr, frequencies=[0.1], normalization="psd")
    # lsp_ppc's default grid: the reference's recipe, src/plots_diagnostics.jl:522-528
    f_min, f_max = 1 / (t[-1] - t[0]), 1 / np.min(np.diff(t)) / 2
    want = np.exp(np.linspace(np.log(f_min / 20), np.log(f_max * 20), 1000))
    assert np.array_equal(pj.lsp_ppc_frequencies(t), want)
    assert np.array_equal(pj.lsp_ppc_frequencies(t, 50, 10, 5), np.exp(np.linspace(np.log(f_min / 10), np.log(f_max * 5), 50)))
    assert np.array_equal(P.reference_grid(t), want)
    import inspect
    sig = inspect.signature(pj.lsp_ppc)
    assert sig.parameters["n_frequencies"].default == 1000 and sig.parameters["S_low"].default == 20 and sig.parameters["S_high"].default == 20
    assert tuple(sig.parameters["quantiles"].default) == (0.025, 0.16, 0.5, 0.84, 0.975)
    assert "lombscargle_dev" in dir(pj.Context) and "lombscargle" in dir(pj.Context)
