"""CPU tests (-m "not gpu") of the posterior draws at new times by Matheron's rule: that the case list of tests/rand_posterior_cases.py holds
what it promises and every case has a truth; the numpy twin of the composition (tools/rand_posterior_proto.py: merged grid, index maps,
gather, residual, combination on top of oracle.sim and oracle.predict — what capi.hip's rand_posterior_batch and the three streaming
kernels of celerite_predict.hip restate) against the long-double truth on every case; the distribution of the draws read off the affine
map; seeded mistakes that the checks must catch; and the C entry's presence and argument checks.

Bounds: max(20 x ref_dev, 256 eps) per case and draw, ref_dev from two fp64 compositions that are not the code under test — the rule and
its reasoning are in tests/rand_posterior_cases.py."""
import ctypes
import inspect
import re
import sys
from pathlib import Path

import numpy as np
import pytest

import pioran_jl_amd as pj

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(Path(__file__).resolve().parent))
import rand_posterior_cases as RP  # noqa: E402

AFFINE_SHAPES = ((5, 9, 7, 0), (33, 17, 9, 2))               # (R, N, M, tau on data times)


def test_case_list_holds_what_it_promises():
    cases = RP.cases()
    labels = [c[0] for c in cases]
    assert len(set(labels)) == len(labels)
    # admission: every candidate but at most 2 % has a long-double Cholesky factor of its zero-noise kernel on the merged grid; the others by name
    n = RP.n_candidates()
    assert len(cases) + len(RP.EXCLUDED) == n
    for label, why in RP.EXCLUDED.items():
        print(f"left out: {label}: {why}")
    assert len(RP.EXCLUDED) <= 0.02 * n, RP.EXCLUDED
    for c in cases:
        assert RP._admit(c) is None, c[0]
    P = {c[0]: len(RP.merged(c[1], c[10])[0]) for c in cases}
    assert min(P.values()) < 16 < max(P.values())                       # P on both sides of the 16-step window
    assert P[RP.CROSS16] == 18 and len(next(c for c in cases if c[0] == RP.CROSS16)[1]) == 9
    on_data = lambda c: np.isin(c[10], c[1]).any()
    tied = lambda c: len(np.unique(c[10])) < len(c[10])
    outside = lambda c: (c[10] < c[1][0]).any() and (c[10] > c[1][-1]).any()
    assert any(on_data(c) for c in cases) and any(tied(c) for c in cases) and any(outside(c) for c in cases)
    assert any(on_data(c) and tied(c) for c in cases)
    R = {RP.rows(c) for c in cases}
    assert min(R) == 1 and {63, 64, 65, 143} <= R                       # both routes' row counts, to their ends
    assert sum(c[14] is not None for c in cases) == 3
    assert any(RP.rows(c) > 63 for c in cases if c[14] is not None) and any(RP.rows(c) <= 63 for c in cases if c[14] is not None)
    # the patterns at the segment edges, both sigma2 variants
    assert {"R63-N257-segment_edges-s2x1", "R63-N257-segment_edges-s2x1e-6", "R40-N129-data-s2x1e-6", "R17-N5-runs-s2x1"} <= set(labels)
    # the normals of a case are its own
    a, b = cases[0], cases[1]
    assert not np.array_equal(a[11][0][:2], b[11][0][:2])


@pytest.mark.parametrize("case", RP.cases(), ids=lambda c: c[0])
def test_prototype_reproduces_the_truth(case):
    """the twin on every case, tau ascending and permuted; the truth exists (reference() raises unless every factorisation succeeds) and the
    fp64 references themselves stay far from garbage: within 1e-12 of it, so that 20 x ref_dev bounds a rounding error, not a mistake"""
    truth, scale, ref_dev = RP.reference(case)
    assert np.isfinite(np.asarray(truth, dtype=np.float64)).all() and (ref_dev < 1e-12).all(), ref_dev
    RP.check(RP.proto_impl(), case, leg="[prototype]")


def _proto_draws(shape, **kw):
    label, t, y, s2, a, b, c, d, mu, nu, tau = shape
    P = RP.proto()
    qd, qn, ep = RP.affine_inputs(shape)
    return np.array([P.rand_posterior(a, b, c, d, t, y - mu, s2, tau, qd[i], qn[i], ep[i], nu=nu, **kw) for i in range(len(qd))])


@pytest.mark.parametrize("R,N,M,on_data", AFFINE_SHAPES)
def test_distribution_from_the_affine_map(R, N, M, on_data):
    """out = m + G (q_data | q_new | eps): m is the posterior mean and G G' the posterior covariance on tau, singular blocks included"""
    shape = RP.affine_shape(R, N, M, on_data)
    assert np.isin(shape[10], shape[1]).sum() == on_data
    RP.check_affine(_proto_draws(shape), shape, leg="[prototype]")


SHOULD_FAIL = {
    "no_eta": ("covariance", "case"),
    "nu_forgotten": ("covariance", "case"),
    "noisy_at_data": ("covariance", "case"),
    "no_merge": ("case",),
    "qnew_sorted": ("case",),
}


@pytest.mark.parametrize("mistake", sorted(SHOULD_FAIL))
def test_seeded_mistakes_are_caught(mistake):
    """each of the prototype's switches fails the covariance check or the case check (a case with ties inside tau and on the data, tau
    permuted)"""
    assert set(SHOULD_FAIL) == set(RP.proto().MISTAKES)
    caught = []
    if "covariance" in SHOULD_FAIL[mistake]:
        shape = RP.affine_shape(33, 17, 9, 2)
        with pytest.raises(AssertionError):
            RP.check_affine(_proto_draws(shape, mistake=mistake), shape, leg=f"[{mistake}]")
        caught.append("covariance")
    if "case" in SHOULD_FAIL[mistake]:
        case = next(c for c in RP.cases() if c[0] == "R17-N5-mixed-s2x1")
        with pytest.raises(AssertionError):
            RP.check(RP.proto_impl(mistake=mistake), case, leg=f"[{mistake}]")
        caught.append("case")
    assert caught


def test_library_entry():
    name = "pioran_celerite_rand_posterior"
    hdr = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "pioran_hip.h").read_text(), flags=re.S)
    assert re.search(r"\bint\s+" + name + r"\s*\(", hdr)
    assert name in pj._lib.SIGNATURES and len(pj._lib.SIGNATURES[name][1]) == 18
    L = pj._lib.lib()
    assert hasattr(L, name)
    jl = (ROOT / "pioran.jl_amd" / "julia" / "PioranHIP.jl").read_text()
    assert re.search(r"ccall\(\(:" + name + r", LIB\)", jl)
    assert L.pioran_abi_version() == 7
    assert callable(pj.Dataset.rand_posterior) and callable(pj.ppc_timeseries)
    assert list(inspect.signature(pj.rand_posterior).parameters) == ["rng", "fp", "tau", "n", "ctx", "solver"]
    assert inspect.signature(pj.rand_posterior).parameters["solver"].default is None
    assert list(inspect.signature(pj.ppc_timeseries).parameters)[:12] == ["rng", "t", "y", "yerr", "A", "Bc", "C", "Dd", "mu", "nu", "shift", "t_pred"]
    # argument checks come before any GPU call
    one = (ctypes.c_double * 1)(1.0)
    p = ctypes.cast(one, ctypes.c_void_p)
    fake = ctypes.c_void_p(8)   # never dereferenced: the checks below come first
    f = L.pioran_celerite_rand_posterior
    assert f(None, 1, 1, p, p, p, p, 1, None, None, None, 1, p, p, p, p, p, None) == -1     # ds
    assert f(fake, 1, 1, p, p, p, p, 1, None, None, None, 1, None, p, p, p, p, None) == -1  # tau
    assert f(fake, 1, 1, p, p, p, p, 1, None, None, None, 1, p, p, p, p, None, None) == -1  # out
    assert f(fake, 1, 1, p, p, p, p, 1, None, None, None, 0, p, p, p, p, p, None) == -1     # M
    assert f(fake, 0, 1, p, p, p, p, 1, None, None, None, 1, p, p, p, p, p, None) == -1     # B
    assert f(fake, 1, 0, p, p, p, p, 1, None, None, None, 1, p, p, p, p, p, None) == -1     # J
    assert f(fake, 1, 1, None, p, p, p, 1, None, None, None, 1, p, p, p, p, p, None) == -1  # A
    assert f(fake, 1, 1, p, p, p, p, 1, None, None, None, 1, p, None, p, p, p, None) == -1  # q_data
    assert f(fake, 1, 1, p, p, p, p, 1, None, None, None, 1, p, p, None, p, p, None) == -1  # q_new
    assert f(fake, 1, 1, p, p, p, p, 1, None, None, None, 1, p, p, p, None, p, None) == -1  # eps
    nan = (ctypes.c_double * 1)(float("nan"))
    assert f(fake, 1, 1, p, p, p, p, 1, None, None, None, 1, ctypes.cast(nan, ctypes.c_void_p), p, p, p, p, None) == -1
    with pytest.raises(ValueError):
        pj.rand_posterior(None, pj.posterior(pj.ScalableGP(pj.Exp(1.0, 1.0))(np.arange(3.0), 0.1), np.zeros(3)), solver="dense")


def test_ppc_grid_is_the_reference_s():
    """t_pred of get_ppc_timeseries: range(t[1], t[end], 2 N) merged with t, sorted, unique"""
    t = np.cumsum(np.random.default_rng(3).uniform(0.1, 2.0, 50))
    g = pj.ppc_t_pred(t)
    assert np.isin(t, g).all() and (np.diff(g) > 0).all() and len(g) == len(np.unique(np.concatenate([t, np.linspace(t[0], t[-1], 100)])))
    g2 = pj.ppc_t_pred(t, [t[3], -1.0, t[3], 1e3])
    assert np.array_equal(g2, np.unique(np.concatenate([t, [-1.0, 1e3]])))


def test_merged_grid_of_the_prototype():
    """the twin's maps against numpy.unique's, with ties inside tau and on the data, tau in any order"""
    P = RP.proto()
    t = np.array([0.5, 1.0, 2.5, 4.0])
    tau = np.array([3.0, 1.0, -2.0, 3.0, 9.0, 2.5])
    T, origin, it, itau = P.merged_grid(t, tau)
    T2, o2, it2, itau2 = RP.merged(t, tau)
    assert np.array_equal(T, T2) and np.array_equal(origin, o2) and np.array_equal(it, it2) and np.array_equal(itau, itau2)
    assert list(origin) == [6, 0, 1, 2, 4, 3, 8]           # a tau on a data time: the data time's normal; tied taus: the first one's
    q = P.gather(origin, 4, np.arange(4.0), 10.0 + np.arange(6.0))
    assert list(q) == [12.0, 0.0, 1.0, 2.0, 10.0, 3.0, 14.0]
