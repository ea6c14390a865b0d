"""GPU tests (-m gpu) of the stores of the tile family's pair pre-pass (tile_pairs_mfma_kernel, celerite_tile.hip).  The pre-pass writes the workspace
[draw][window][128] that the main kernel reads; what a single store instruction writes, and so which lane writes which draw row, is the part under
test.  Through the public batch entry with the tile family forced, against the oracle (1e-11 relative on log L as the other tile tests; statuses the
oracle's):

* rows: B = 1, 15, 16, 17, 63, 64, 65, 130 — one live row in a wavefront, the live-row mask inside a group of rows that one instruction writes, a
  wavefront that returns early (its sixteen rows all past B), a second workgroup in y (64 draws per workgroup);
* windows: N = 16, 17, 80, 81, 96, 161 (1, 2, 5, 6, 6, 11 windows: a workgroup walks kPairWin = 5 of them — remainders 0 and 1 — and the ragged last one);
* terms: J = 1, 4, 5, 20, 21, 40, 41, 64 (the instantiations <5>, <10>, <16> and their boundaries JQ = ceil(J / 4) = 5 | 6, 10 | 11, 16); J = 64 on real
  terms, one row each, since the kernel takes 95 rows at the most;
* a guard: in a fresh context a B = 17 call comes first, so that its workspace holds seventeen rows and no more, then B = 130, then both again.  A
  store past row B lands in whatever the device allocator placed behind the workspace (the next call's buffers among them) or in the rows of the
  larger call; every call must agree with the oracle and the repeated calls bit for bit with the first ones.  (Where the allocator puts the buffers is
  not in the test's hands: the check is necessary, not sufficient.)

One draw of every case with J >= 2 has a negative leading amplitude (the oracle decides whether that makes it status 1); it sits in the last, partly live,
row group.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import pioran_jl_amd as pj  # noqa: E402
from oracle import oracle as O  # noqa: E402

ROWS = [1, 15, 16, 17, 63, 64, 65, 130]
SIZES = [16, 17, 80, 81, 96, 161]
TERMS = [1, 4, 5, 20, 21, 40, 41, 64]


@pytest.fixture(scope="module")
def ctx():
    c = pj.Context(0)
    c.set_option("scan_config", "tile")
    yield c
    c.set_option("scan_config", None)


def relerr(got, ref):
    got = np.asarray(got, float); ref = np.asarray(ref, float)
    return np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300))


def case(seed, B, N, J):
    rng = np.random.default_rng(seed)
    t = np.cumsum(rng.uniform(0.05, 2.0, N))
    y = rng.standard_normal(N)
    s2 = rng.uniform(0.01, 0.1, N)
    A = rng.uniform(0.1, 2.0, (B, J))
    Bc = rng.uniform(-0.05, 0.05, (B, J)) * A
    C = rng.uniform(0.05, 2.0, J)
    Dd = rng.uniform(0.0, 3.0, J)
    if 2 * J > 95:                      # real terms, one row each: the rows fit the kernel
        Bc[:] = 0.0
        Dd[:] = 0.0
    if J >= 2 and B >= 2:               # sum(a) stays positive, the first term's negative amplitude outweighs it one step on
        ratio = Bc[B - 1, 0] / A[B - 1, 0]
        A[B - 1, 0] = -0.98 * A[B - 1, 1:].sum()
        Bc[B - 1, 0] = ratio * A[B - 1, 0]
    mu = rng.standard_normal(B) * 0.1
    nu = rng.uniform(0.5, 2.0, B)
    return t, y, s2, A, Bc, C, Dd, mu, nu


def check(ctx, B, N, J, seed):
    t, y, s2, A, Bc, C, Dd, mu, nu = case(seed, B, N, J)
    got, st = pj.Dataset(t, y, s2, ctx).logl_batch(A, Bc, C, Dd, mu=mu, nu=nu, return_status=True)
    assert pj._lib.lib().pioran_celerite_config_name(-1).decode() == "tile"
    ref, rst = O.logl_batch(A, Bc, C, Dd, t, y, s2, mu, nu, nthreads=4, return_status=True)
    pd = rst == 0
    err = relerr(got[pd], ref[pd])
    print(f"B={B} N={N} J={J}: {int(pd.sum())} PD draws, oracle statuses {sorted(set(rst.tolist()))}, max rel err {err:.3e}")
    assert (st == rst).all()
    assert pd.sum() >= B - 1
    assert err < 1e-11
    return got, st


@pytest.mark.parametrize("B", ROWS)
def test_prepass_rows(ctx, B):
    check(ctx, B, 81, 5, 1000 + B)


@pytest.mark.parametrize("N", SIZES)
def test_prepass_windows(ctx, N):
    check(ctx, 17, N, 5, 2000 + N)


@pytest.mark.parametrize("J", TERMS)
def test_prepass_terms(ctx, J):
    check(ctx, 17, 33, J, 3000 + J)


def test_prepass_guard_rows():
    c = pj.Context(0)
    c.set_option("scan_config", "tile")
    try:
        first = [check(c, B, 81, 20, 4000 + B) for B in (17, 130)]
        again = [check(c, B, 81, 20, 4000 + B) for B in (17, 130)]
    finally:
        c.set_option("scan_config", None)
    for (g0, s0), (g1, s1) in zip(first, again):
        assert g0.tobytes() == g1.tobytes() and (s0 == s1).all()
