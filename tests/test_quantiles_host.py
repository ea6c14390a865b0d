"""CPU tests (-m "not gpu") of the quantiles over the draw axis: the numpy twin of quantiles.hip (tools/quantiles_proto.py), which is the
project's definition of the quantile (Statistics.quantile's default, type 7), the argument checks of the three C entries and the host-side API.

Inputs: seeded standard normals, each column scaled by 10^U(-3, 3), K = 1, 2, 3, 5, 64, 65, 1000 values per column, 7 columns; probabilities
0, 1, 0.5, the reference's five and 1/3.

Bound: 16 eps max|v| of the column against np.quantile(method = "linear"), which rounds gamma differently: a fuzz over K <= 1000 measured
14 eps (not a proven bound), 16 adds a small margin.  Measured on these cases: 3.5 eps against numpy, 5.4 eps for the reflection
q_p(-x) = -q_{1-p}(x) (1 - p is rounded)."""
import ctypes
import importlib.util
import re
from pathlib import Path

import numpy as np
import pytest

import pioran_jl_amd as pj

ROOT = Path(__file__).resolve().parents[1]
EPS = np.finfo(np.float64).eps
KS = [1, 2, 3, 5, 64, 65, 1000]
PROBS = [0.0, 1.0, 0.5, 0.025, 0.16, 0.84, 0.975, 1.0 / 3.0]
FIVE = (0.025, 0.16, 0.5, 0.84, 0.975)


def _proto():
    spec = importlib.util.spec_from_file_location("quantiles_proto", ROOT / "tools" / "quantiles_proto.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


P = _proto()


def _columns(K):
    rng = np.random.default_rng(77000 + K)
    return rng.standard_normal((K, 7)) * 10.0 ** rng.uniform(-3, 3, 7)


@pytest.mark.parametrize("K", KS)
def test_twin_against_numpy(K):
    X = _columns(K)
    q, mean, kept = P.quantiles(X, PROBS)
    ref = np.quantile(X, PROBS, axis=0, method="linear")
    dev = float(np.max(np.abs(q - ref) / np.max(np.abs(X), axis=0))) / EPS
    print(f"K = {K}: max |twin - np.quantile| = {dev:.2f} eps max|v|")
    assert kept == K and q.shape == (len(PROBS), 7)
    assert dev <= 16.0
    assert np.max(np.abs(mean - X.mean(axis=0)) / np.mean(np.abs(X), axis=0)) <= K * EPS


@pytest.mark.parametrize("K", KS)
def test_twin_ends_are_exact(K):
    X = _columns(K)
    q, _, _ = P.quantiles(X, [0.0, 1.0, 0.3])
    assert np.array_equal(q[0], X.min(axis=0)) and np.array_equal(q[1], X.max(axis=0))
    if K == 1:
        assert np.array_equal(q[2], X[0])


@pytest.mark.parametrize("K", KS)
def test_twin_reflection(K):
    X = _columns(K)
    q, _, _ = P.quantiles(X, PROBS)
    r, _, _ = P.quantiles(-X, [1.0 - p for p in PROBS])
    dev = float(np.max(np.abs(q + r) / np.max(np.abs(X), axis=0))) / EPS
    print(f"K = {K}: max |q_p(x) + q_(1-p)(-x)| = {dev:.2f} eps max|v|")
    assert dev <= 16.0


def test_twin_infinite_values_take_the_second_branch():
    inf = np.inf
    X = np.array([[2.0, 1.0], [inf, inf], [-inf, 3.0], [1.0, 2.0]])     # column 0: -inf 1 2 inf; column 1: 1 2 3 inf
    q, mean, _ = P.quantiles(X, [0.0, 0.2, 0.5, 1.0, 0.9])
    # column 0: aleph = 1, 1.6, 2.5, 4: (1 - g) a + g b with an infinite a or b; a + g (b - a) between the finite pair
    assert q[0, 0] == -inf and q[1, 0] == -inf and q[2, 0] == 1.5 and q[3, 0] == inf
    assert np.isnan(mean[0]) and mean[1] == inf
    # column 1 at p = 0.9: aleph = 3.7, a = 3, b = inf, gamma = 0.7: 0.3 * 3 + 0.7 inf
    assert q[4, 1] == inf
    # gamma = 0 beside an infinite neighbour: the second form gives 1 * 1 + 0 * inf = NaN, as written
    q2, _, _ = P.quantiles(np.array([[1.0], [inf]]), [0.0, 1.0])
    assert np.isnan(q2[0, 0]) and q2[1, 0] == inf


def test_twin_nan_column_and_no_rows():
    X = _columns(5)
    X[3, 2] = np.nan
    q, mean, kept = P.quantiles(X, FIVE)
    clean, cmean, _ = P.quantiles(np.delete(X, 2, axis=1), FIVE)
    assert np.all(np.isnan(q[:, 2])) and np.isnan(mean[2])
    assert np.array_equal(np.delete(q, 2, axis=1), clean) and np.array_equal(np.delete(mean, 2), cmean)
    q0, m0, k0 = P.quantiles(X, FIVE, status=np.ones(5, dtype=np.int32))
    assert k0 == 0 and np.all(np.isnan(q0)) and np.all(np.isnan(m0))


def test_twin_load_stages_and_row_exclusion():
    rng = np.random.default_rng(5)
    X = rng.standard_normal((9, 6))
    status = np.array([0, 2, 0, 0, 1, 0, 0, 0, 2], dtype=np.int32)
    shift = rng.uniform(-1, 1, 9)
    cols = np.array([4, 0, 4, 5])
    ref, scale = rng.standard_normal(4), rng.uniform(0.5, 2, 4)
    V = P.load(X, status, shift, cols, ref, scale)
    keep = status == 0
    want = (ref[None, :] - np.exp(X[keep][:, cols] + shift[keep, None])) / scale[None, :]
    assert np.array_equal(V, want)
    q, mean, kept = P.quantiles(X, FIVE, status, shift, cols, ref, scale)
    q2, mean2, _ = P.quantiles(want, FIVE)
    assert kept == 6 and np.array_equal(q, q2) and np.array_equal(mean, mean2)
    q3, _, _ = P.quantiles(X, FIVE, status, shift, cols)          # a repeated column repeats its result
    assert np.array_equal(q3[:, 0], q3[:, 2]) and not np.array_equal(q3[:, 0], q3[:, 1])


def test_symbols_and_public_names():
    hdr = (ROOT / "include" / "pioran_hip.h").read_text()
    jl = (ROOT / "pioran.jl_amd" / "julia" / "PioranHIP.jl").read_text()
    L = pj._lib.lib()
    for name in ("pioran_quantiles_batch", "pioran_quantiles_batch_dev", "pioran_celerite_rand_posterior_summary"):
        assert re.search(r"\bint " + name + r"\(", hdr), name
        assert name in pj._lib.SIGNATURES and hasattr(L, name)
        assert f"(:{name}, LIB)" in jl, name
    for name in ("quantiles", "ppc_timeseries_summary", "ppc_timeseries", "lsp_ppc"):
        assert hasattr(pj, name), name
    for name in ("quantiles", "quantiles_dev"):
        assert hasattr(pj.Context, name), name
    assert hasattr(pj.Dataset, "rand_posterior_summary")
    import inspect
    assert tuple(inspect.signature(pj.quantiles).parameters["probs"].default) == FIVE
    assert tuple(inspect.signature(pj.ppc_timeseries_summary).parameters["quantiles"].default) == FIVE
    assert tuple(P.DEFAULT_PROBS) == FIVE
    assert L.pioran_abi_version() == 7


def test_argument_checks_without_gpu():
    """Every PIORAN_ERR_ARG / PIORAN_ERR_UNSUPPORTED case of the three entries comes back before any GPU call (no context can exist here: a
    refused call with a non-NULL handle is made with a dummy that must never be used)."""
    L = pj._lib.lib()
    v = ctypes.c_void_p
    p = lambda a: None if a is None else v(a.ctypes.data)
    dummy = v(ctypes.addressof(ctypes.create_string_buffer(4096)))
    B, M, Q, Mc = 3, 4, 2, 2
    X = np.ones((B, M)); probs = np.array([0.25, 0.5]); quant = np.empty((Q, M)); mean = np.empty(M); kept = np.zeros(1, dtype=np.int32)
    cols = np.array([3, 0], dtype=np.int32); ref = np.zeros(Mc); scale = np.ones(Mc)

    def call(fn, ctx=dummy, B=B, M=M, ldx=M, X=X, Mc=0, cols=None, ref=None, scale=None, Q=Q, probs=probs, quant=quant):
        return fn(ctx, B, M, ldx, p(X), None, None, Mc, p(cols), p(ref), p(scale), Q, p(probs), p(quant), p(mean), p(kept))

    for fn in (L.pioran_quantiles_batch, L.pioran_quantiles_batch_dev):
        f = lambda **kw: call(fn, **kw)
        assert f(ctx=None) == -1
        for name in ("X", "probs", "quant"):
            assert f(**{name: None}) == -1, name
        assert f(B=0) == -1 and f(M=0) == -1 and f(Q=0) == -1
        assert f(ldx=M - 1) == -1
        assert f(cols=cols, Mc=0) == -1
        assert f(cols=cols, Mc=Mc, ref=ref) == -1 and f(cols=cols, Mc=Mc, scale=scale) == -1
        for bad in (-1e-9, 1.0 + 1e-9, np.nan, np.inf):
            assert f(probs=np.array([0.5, bad])) == -1, bad
        big = np.ones((4097, 1))
        assert f(B=4097, M=1, ldx=1, X=big) == -4
    # what only the host form can look at
    host = lambda **kw: call(L.pioran_quantiles_batch, **kw)
    for bad in (-1, M):
        assert host(cols=np.array([0, bad], dtype=np.int32), Mc=Mc) == -1
    for bad in (0.0, np.nan, np.inf):
        assert host(cols=cols, Mc=Mc, ref=ref, scale=np.array([1.0, bad])) == -1

    # the summary entry: the checks of pioran_celerite_rand_posterior, of the reduction, and its own
    J, N = 2, 0        # (the dummy data set reads as N = 0; no call below gets past the checks)
    A = np.ones((B, J)); C = np.array([0.1, 0.2]); tau = np.arange(M, dtype=np.float64)
    qd = np.zeros((B, 1)); qn = np.zeros((B, M)); shift = np.zeros(B)
    tsq = np.empty((Q, M)); rq = np.empty((Q, Mc)); rm = np.empty(Mc); st = np.zeros(B, dtype=np.int32)

    def summ(ds=dummy, B=B, J=J, A=A, tau=tau, M=M, shift=None, back=0, Q=Q, probs=probs, tsq=tsq, Nres=Mc, cols=cols, ref=ref, scale=scale, rq=rq,
             qn=qn, Bc=A, C=C, Dd=C, qd=qd, eps=qd):
        return L.pioran_celerite_rand_posterior_summary(ds, B, J, p(A), p(Bc), p(C), p(Dd), 1, None, None, p(shift), M, p(tau), p(qd), p(qn), p(eps),
                                                        back, Q, p(probs), p(tsq), p(mean), Nres, p(cols), p(ref), p(scale), p(rq), p(rm), p(st),
                                                        p(kept))

    assert summ(ds=None) == -1 and summ(B=0) == -1 and summ(J=0) == -1 and summ(M=0) == -1 and summ(Q=0) == -1
    for name in ("A", "Bc", "C", "Dd", "tau", "qd", "qn", "eps", "probs", "tsq"):
        assert summ(**{name: None}) == -1, name
    assert summ(back=1) == -1                                   # backtransform without shift
    assert summ(Nres=-1) == -1
    assert summ(ref=None) == -1 and summ(scale=None) == -1 and summ(rq=None) == -1
    assert summ(cols=None) == -1                                # without columns Nres must be M
    assert summ(cols=np.array([0, M], dtype=np.int32)) == -1
    assert summ(scale=np.array([1.0, 0.0])) == -1
    assert summ(probs=np.array([0.5, 1.5])) == -1
    tb = tau.copy(); tb[1] = np.nan
    assert summ(tau=tb) == -1
    assert summ(B=4097, A=np.ones((4097, J)), Nres=0) == -4
