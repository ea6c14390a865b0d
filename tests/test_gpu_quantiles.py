"""GPU tests of the quantiles and means over the draw axis (quantiles.hip through pioran_quantiles_batch[_dev]) against the numpy twin
(tools/quantiles_proto.py), which is the definition.

Without `shift` the quantiles must be the twin's numbers (np.array_equal on the values, NaN where the twin has NaN): sorting only moves data,
gather, subtraction and division are correctly rounded on both sides, and the interpolation is specified operation by operation.  The mean
must lie within K eps mean_b|v| of the long-double mean, the worst case of any summation order.  With `shift` the bound is
16 eps max_b|v| of the column: order statistics and their convex combinations are 1-Lipschitz in the sup norm, the two exp differ by at most
(3 + 1) eps |v| (3 ulp: the OpenCL bound ocml's exp is held to; 1 ulp: numpy's — assumed of both libraries, not measured), the interpolation
adds 3 eps, the rest is margin.  Every test prints what it measured; docs/EXPERIMENTS.md (quantile section) records the figures.
Inputs: seeded standard normals, each column scaled by 10^U(-3, 3)."""
import importlib.util
from pathlib import Path

import numpy as np
import pytest

import pioran_jl_amd as pj

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
EPS = np.finfo(np.float64).eps
NAME = "quantiles (sort over draws)"
PROBS = [0.5, 0.0, 1.0, 0.975, 0.025, 0.16, 0.84, 0.5, 0.3]       # 0, 1, 0.5, the five defaults, unsorted, one repeated
SHAPES = [(1, 1), (2, 3), (5, 1), (63, 7), (64, 64), (65, 130), (100, 257), (129, 33), (1000, 70), (1024, 9), (1025, 5), (4096, 3)]


def _proto():
    spec = importlib.util.spec_from_file_location("quantiles_proto", ROOT / "tools" / "quantiles_proto.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


P = _proto()


@pytest.fixture(scope="module")
def ctx():
    c = pj.Context(0)
    yield c
    c.close()


def _data(B, M):
    rng = np.random.default_rng(1000 * B + M)
    return rng.standard_normal((B, M)) * 10.0 ** rng.uniform(-3, 3, M)


def _config_name():
    return pj._lib.lib().pioran_celerite_config_name(-1).decode()


def _same(a, b):
    """equal as numbers, NaN exactly where the other has NaN"""
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])


def _mean_excess(mean, X, **kw):
    """largest |mean - long-double mean| in units of the bound K eps mean|v| over the columns with a finite mean; the others must agree in kind"""
    ref, absmean = P.mean_longdouble(X, **kw)
    ref64 = ref.astype(np.float64)
    fin = np.isfinite(ref64)
    assert np.array_equal(mean[~fin], ref64[~fin], equal_nan=True)
    if not fin.any():
        return 0.0
    K = P.load(X, **kw).shape[0]
    return float(np.max(np.abs(mean[fin] - ref[fin]) / (K * EPS * absmean[fin] + np.finfo(np.float64).tiny)))


def _check_exact(ctx, X, label, **kw):
    want_q, _, want_k = P.quantiles(X, PROBS, **kw)
    q, mean, kept = ctx.quantiles(X, PROBS, **kw)
    excess = _mean_excess(mean, X, **kw)
    differ = int(np.sum(~((q == want_q) | (np.isnan(q) & np.isnan(want_q)))))
    print(f"{label}: kept {kept} (twin {want_k}); quantiles that differ from the twin: {differ} of {q.size}; "
          f"|mean - long double| = {excess:.3f} x K eps mean|v|")
    assert kept == want_k
    assert _same(q, want_q)
    assert excess <= 1.0
    return q, mean, kept


@pytest.mark.parametrize("B,M", SHAPES)
def test_shapes_equal_the_twin(ctx, B, M):
    X = _data(B, M)
    if (B, M) == (63, 7):                      # rows three doubles longer than the columns that are reduced
        wide = np.full((B, M + 3), np.nan)
        wide[:, :M] = X
        X = wide[:, :M]
        assert X.strides[0] == 8 * (M + 3)
    _check_exact(ctx, X, f"(B, M) = ({B}, {M})")
    assert _config_name() == NAME


@pytest.mark.parametrize("pattern", ["first", "last", "every second", "all but one", "all"])
def test_row_exclusion(ctx, pattern):
    B, M = 65, 130
    X = _data(B, M)
    status = np.zeros(B, dtype=np.int32)
    if pattern == "first":
        status[0] = 2
    elif pattern == "last":
        status[-1] = 2
    elif pattern == "every second":
        status[::2] = 2
    elif pattern == "all but one":
        status[:] = 2
        status[17] = 0
    else:
        status[:] = 1
    X[status != 0] = np.nan                    # what the entries that set a status leave in such rows
    q, mean, kept = _check_exact(ctx, X, f"rows left out: {pattern}", status=status)
    kept_rows = X[status == 0]
    assert kept == len(kept_rows)
    if len(kept_rows):
        assert _same(q, P.quantiles(kept_rows, PROBS)[0]) and np.all(np.isfinite(q))
    else:
        assert kept == 0 and np.all(np.isnan(q)) and np.all(np.isnan(mean))


def test_non_finite_values_in_kept_rows(ctx):
    B, M = 65, 130
    X = _data(B, M)
    clean_q, clean_mean, _ = ctx.quantiles(X, PROBS)
    Z = X.copy()
    Z[7, 3] = np.nan
    Z[64, 50] = np.inf
    Z[0, 129] = -np.inf
    Z[33, 129] = np.inf
    q, mean, kept = _check_exact(ctx, Z, "NaN in column 3, +inf in 50, -inf and +inf in 129")
    assert np.all(np.isnan(q[:, 3])) and np.isnan(mean[3])
    assert mean[50] == np.inf and q[PROBS.index(1.0), 50] == np.inf and np.isfinite(q[PROBS.index(0.0), 50])
    assert np.isnan(mean[129]) and q[PROBS.index(0.0), 129] == -np.inf and q[PROBS.index(1.0), 129] == np.inf
    others = np.setdiff1d(np.arange(M), [3, 50, 129])
    assert np.array_equal(q[:, others], clean_q[:, others]) and np.array_equal(mean[others], clean_mean[others])
    # a negative NaN sorts with the other NaN
    Z[9, 11] = np.copysign(np.nan, -1.0)
    assert np.all(np.isnan(ctx.quantiles(Z, PROBS)[0][:, 11]))


def test_cols_ref_scale(ctx):
    B, M = 100, 257
    X = _data(B, M)
    rng = np.random.default_rng(8)
    cols = rng.permutation(M)[:77].astype(np.int32)
    cols[5] = cols[60]                           # unsorted, one repeated
    ref = rng.standard_normal(77) * 10.0
    scale = rng.uniform(0.05, 3.0, 77) * rng.choice([-1.0, 1.0], 77)
    q, _, _ = _check_exact(ctx, X, "cols (77 of 257, unsorted, one repeated)", cols=cols)
    assert np.array_equal(q[:, 5], q[:, 60])
    _check_exact(ctx, X, "cols, ref, scale (the residual map)", cols=cols, ref=ref, scale=scale)
    _check_exact(ctx, X, "ref, scale on all columns", ref=np.resize(ref, M), scale=np.resize(scale, M))
    status = np.zeros(B, dtype=np.int32)
    status[[3, 64, 99]] = 2
    _check_exact(ctx, X, "cols, ref, scale, three rows left out", status=status, cols=cols, ref=ref, scale=scale)


@pytest.mark.parametrize("B,M", [(5, 1), (65, 130), (1000, 70)])
def test_shift_back_transform(ctx, B, M):
    rng = np.random.default_rng(B + M)
    X = rng.standard_normal((B, M)) * rng.uniform(0.1, 3.0, M)
    shift = rng.uniform(-2.0, 2.0, B)
    status = np.zeros(B, dtype=np.int32)
    status[B // 2] = 2
    want_q, _, want_k = P.quantiles(X, PROBS, status=status, shift=shift)
    q, mean, kept = ctx.quantiles(X, PROBS, status=status, shift=shift)
    vmax = np.max(np.abs(P.load(X, status, shift)), axis=0) if want_k else np.ones(M)
    dev = float(np.max(np.abs(q - want_q) / vmax[None, :])) / EPS if want_k else 0.0
    excess = _mean_excess(mean, X, status=status, shift=shift)
    print(f"shift, (B, M) = ({B}, {M}): max |device - twin| = {dev:.2f} eps max|v|; |mean - long double| = {excess:.3f} x (K + 4) eps mean|v|")
    assert kept == want_k
    assert dev <= 16.0
    assert excess <= (want_k + 4.0) / want_k          # the values themselves differ by up to 4 eps |v|


def test_device_form_equals_host_form(ctx):
    import torch
    B, M = 129, 33
    X = _data(B, M)
    rng = np.random.default_rng(2)
    status = np.zeros(B, dtype=np.int32)
    status[[0, 77]] = 2
    shift = rng.uniform(-1, 1, B)
    cols = rng.permutation(M)[:20].astype(np.int32)
    ref, scale = rng.standard_normal(20), rng.uniform(0.5, 2.0, 20)
    dev = torch.device("cuda:0")
    dX, dst, dsh, dc, dr, dsc = (torch.from_numpy(a).to(dev) for a in (X, status, shift, cols, ref, scale))
    Q = len(PROBS)
    for label, kw, dkw, Mc in (("plain", {}, {}, M),
                               ("status, cols, ref, scale", dict(status=status, cols=cols, ref=ref, scale=scale),
                                dict(dstatus=dst.data_ptr(), Mc=20, dcols=dc.data_ptr(), dref=dr.data_ptr(), dscale=dsc.data_ptr()), 20),
                               ("status, shift", dict(status=status, shift=shift), dict(dstatus=dst.data_ptr(), dshift=dsh.data_ptr()), M)):
        hq, hm, hk = ctx.quantiles(X, PROBS, **kw)
        dq = torch.full((Q, Mc), -1.0, dtype=torch.float64, device=dev)
        dm = torch.full((Mc,), -1.0, dtype=torch.float64, device=dev)
        dk = torch.full((1,), -1, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        ctx.quantiles_dev(B, M, M, dX.data_ptr(), PROBS, dquant=dq.data_ptr(), dmean=dm.data_ptr(), dkept=dk.data_ptr(), **dkw)
        ctx.synchronize()
        # (exp(v + shift) overflows in the columns with a large scale: inf and NaN have to agree as well)
        same = np.array_equal(dq.cpu().numpy(), hq, equal_nan=True) and np.array_equal(dm.cpu().numpy(), hm, equal_nan=True) and int(dk.cpu()[0]) == hk
        print(f"device form, {label}: bit-identical to the host form: {same}")
        assert same
    # without mean and kept
    dq = torch.full((Q, M), -1.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    ctx.quantiles_dev(B, M, M, dX.data_ptr(), PROBS, dquant=dq.data_ptr())
    ctx.synchronize()
    assert np.array_equal(dq.cpu().numpy(), ctx.quantiles(X, PROBS)[0])


@pytest.mark.parametrize("B,M", [(100, 257), (1000, 70)])
def test_result_does_not_depend_on_the_layout(ctx, B, M):
    """the same columns in one call and split over two calls (each with its own tiles), and picked through cols: identical bits, mean included"""
    X = _data(B, M)
    q, mean, _ = ctx.quantiles(X, PROBS)
    cut = M // 3 + 1
    q1, m1, _ = ctx.quantiles(np.ascontiguousarray(X[:, :cut]), PROBS)
    q2, m2, _ = ctx.quantiles(X, PROBS, cols=np.arange(cut, M))
    same = np.array_equal(np.hstack([q1, q2]), q) and np.array_equal(np.concatenate([m1, m2]), mean)
    rev = np.arange(M)[::-1].copy()
    q3, m3, _ = ctx.quantiles(X, PROBS, cols=rev)
    same_rev = np.array_equal(q3[:, ::-1], q) and np.array_equal(m3[::-1], mean)
    print(f"(B, M) = ({B}, {M}): split at column {cut} bit-identical: {same}; columns reversed through cols: {same_rev}")
    assert same and same_rev


def test_module_level_function_and_defaults(ctx):
    X = _data(100, 257)
    q, mean, kept = pj.quantiles(X, ctx=ctx)
    want, _, _ = P.quantiles(X)
    assert q.shape == (5, 257) and kept == 100 and np.array_equal(q, want)
    with pytest.raises(pj._lib.PioranHipError):
        ctx.quantiles(np.zeros((4097, 2)), [0.5])
