"""GPU tests (-m gpu) of the order of a window in the tile kernel (celerite_tile.hip, round 9): values now cross phases and windows in LDS and in registers —
1 / D_n goes from lane column n to its users through the padding column of the transposing scratch, the rescaling (C_K C_K') o T of the update stands in the
waits in front of and behind the window's LDL', the table reads of the next window's U~ are issued in front of that exchange.  The cases are the ones where such
a value can be read before it is written, or written over before it is read:

* N = 16 (one window: nothing fetched ahead is ever used), 17 (a second, ragged window with a single live step), 32 and 33, 49 (three full windows and one
  step more: every buffer is used again);
* B = 1, 5 and 9 draws: workgroups of four wavefronts that are not filled;
* R = 32 (KL = 0: the last block holds the y row alone), 33, 40 (the headline's <3, 2>), 47, 60 (four block columns), 80 (six: one wavefront per SIMD);
* the shared series everywhere, per-draw series at R = 40 and 60;
* one non-positive-definite draw among positive-definite ones at R = 40.

The kernel is forced by scan_config = "tile"; the reference is the CPU oracle, the tolerance 1e-11 relative on log L as in tests/test_gpu_tile_ksteps.py.
The oracle is evaluated once per (R, N) on the nine draws; the smaller batches are the leading draws of the same inputs."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import pioran_jl_amd as pj  # noqa: E402
from oracle import oracle as O  # noqa: E402

NS = (16, 17, 32, 33, 49)
BS = (1, 5, 9)
RS = (32, 33, 40, 47, 60, 80)
TOL = 1e-11


@pytest.fixture(scope="module")
def ctx():
    c = pj.Context(0)
    c.set_option("scan_config", "tile")
    yield c
    c.set_option("scan_config", None)


def relerr(got, ref):
    got = np.asarray(got, float); ref = np.asarray(ref, float)
    return np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300))


def kernel_name():
    return pj._lib.lib().pioran_celerite_config_name(-1).decode()


def rows_case(rng, R, N, B):
    """R rows: ceil(R / 2) terms, the first one real (one row) when R is odd — the ranges of tests/test_gpu_tile_ksteps.py."""
    J = (R + 1) // 2
    nreal = 2 * J - R
    t = np.cumsum(rng.uniform(0.05, 2.0, N))
    y = rng.standard_normal(N)
    s2 = rng.uniform(0.01, 0.1, N)
    A = rng.uniform(0.1, 2.0, (B, J))
    Bc = rng.uniform(-0.05, 0.05, (B, J)) * A
    C = rng.uniform(0.05, 2.0, J)
    Dd = rng.uniform(0.0, 3.0, J)
    Bc[:, :nreal] = 0.0
    Dd[:nreal] = 0.0
    mu = rng.standard_normal(B) * 0.1
    nu = rng.uniform(0.5, 2.0, B)
    return t, y, s2, A, Bc, C, Dd, mu, nu


_cases = {}


def case(R, N):
    """Inputs of (R, N) for max(BS) draws and the oracle's log L and status on them: made once, read-only."""
    if (R, N) not in _cases:
        rng = np.random.default_rng(19000 + 100 * R + N)
        c = rows_case(rng, R, N, max(BS))
        t, y, s2, A, Bc, C, Dd, mu, nu = c
        ref, rst = O.logl_batch(A, Bc, C, Dd, t, y, s2, mu, nu, nthreads=4, return_status=True)
        for a in (*c, ref, rst):
            a.setflags(write=False)
        _cases[(R, N)] = (c, ref, rst)
    return _cases[(R, N)]


@pytest.mark.parametrize("R", RS)
@pytest.mark.parametrize("N", NS)
def test_window_order_shared_series(ctx, R, N):
    (t, y, s2, A, Bc, C, Dd, mu, nu), ref, rst = case(R, N)
    assert (rst == 0).all() and np.isfinite(ref).all()
    ds = pj.Dataset(t, y, s2, ctx)
    for B in BS:
        got, st = ds.logl_batch(A[:B], Bc[:B], C, Dd, mu=mu[:B], nu=nu[:B], return_status=True)
        assert kernel_name() == "tile", (R, N, B)
        err = relerr(got, ref[:B])
        print(f"R = {R} N = {N} B = {B}: max relative error {err:.2e}")
        assert err < TOL, (R, N, B)
        assert (st == 0).all(), (R, N, B)
    ds.close()


@pytest.mark.parametrize("R", (40, 60))
@pytest.mark.parametrize("N", NS)
def test_window_order_per_draw_series(ctx, R, N):
    (t, y, s2, A, Bc, C, Dd, mu, nu), _, _ = case(R, N)
    rng = np.random.default_rng(29000 + 100 * R + N)
    Bm = max(BS)
    Y = rng.standard_normal((Bm, N)); S2 = rng.uniform(0.01, 0.1, (Bm, N))
    ref = np.array([O.logl(A[i], Bc[i], C, Dd, t, Y[i] - mu[i], nu[i] * S2[i]) for i in range(Bm)])
    ds = pj.Dataset(t, y, s2, ctx)
    for B in BS:
        got = ds.logl_batch(A[:B], Bc[:B], C, Dd, mu=mu[:B], nu=nu[:B], Y=Y[:B], S2=S2[:B])
        assert kernel_name() == "tile", (R, N, B)
        err = relerr(got, ref[:B])
        print(f"per-draw series R = {R} N = {N} B = {B}: max relative error {err:.2e}")
        assert err < TOL, (R, N, B)
    ds.close()


@pytest.mark.parametrize("N", NS)
def test_window_order_non_pd_draw(ctx, N):
    """R = 40: draw 1 is not positive definite; its status is the oracle's, the other draws keep 1e-11."""
    (t, y, s2, A, Bc, C, Dd, mu, nu), _, _ = case(40, N)
    A = A.copy()
    A[1] *= -1.0
    ref, rst = O.logl_batch(A, Bc, C, Dd, t, y, s2, mu, nu, nthreads=4, return_status=True)
    assert rst[1] != 0 and (np.delete(rst, 1) == 0).all()
    ds = pj.Dataset(t, y, s2, ctx)
    for B in (5, 9):
        got, st = ds.logl_batch(A[:B], Bc[:B], C, Dd, mu=mu[:B], nu=nu[:B], return_status=True)
        assert kernel_name() == "tile", (N, B)
        assert (st == rst[:B]).all(), (N, B)
        pd = rst[:B] == 0
        err = relerr(got[pd], ref[:B][pd])
        print(f"non-positive-definite draw, N = {N} B = {B}: max relative error of the others {err:.2e}")
        assert err < TOL, (N, B)
        assert (np.isnan(got) == np.isnan(ref[:B])).all(), (N, B)
    ds.close()
