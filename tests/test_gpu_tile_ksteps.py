"""GPU tests (-m gpu) of the tile kernel's row dispatch (celerite_tile.hip, round 7): the value kernel is instantiated per (NB, KL) — NB block
columns, KL = ceil((R - 16 (NB - 1)) / 4) K-steps of the last row block that hold a state row — and skips the K-steps past them.  Every row count
the kernel takes, R = 1 .. 95, so every (NB, KL) pair, against the oracle; odd R through one-row (real) terms.
Tolerance: 1e-11 relative on log L, as tests/test_gpu_parity.py::test_tile_kernel_edges.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import pioran_jl_amd as pj  # noqa: E402
from oracle import oracle as O  # noqa: E402


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
    """R rows: ceil(R / 2) terms, the first one real (one row) when R is odd."""
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


def nb_kl(R):
    nb = (R + 1 + 15) // 16
    return nb, (R - 16 * (nb - 1) + 3) // 4


def test_tile_every_row_count(ctx):
    """R = 1 .. 95 at N = 37 (two full windows and a ragged one), 5 draws (a workgroup not filled)."""
    rng = np.random.default_rng(9107)
    seen = set()
    for R in range(1, 96):
        t, y, s2, A, Bc, C, Dd, mu, nu = rows_case(rng, R, 37, 5)
        got, st = pj.Dataset(t, y, s2, ctx).logl_batch(A, Bc, C, Dd, mu=mu, nu=nu, return_status=True)
        assert kernel_name() == "tile", R
        ref = O.logl_batch(A, Bc, C, Dd, t, y, s2, mu, nu, nthreads=4)
        assert relerr(got, ref) < 1e-11, (R, nb_kl(R))
        assert (st == 0).all(), R
        seen.add(nb_kl(R))
    # every instantiation ran: NB = 1 has KL = 1 .. 4, NB = 2 .. 6 have KL = 0 .. 4
    assert seen == {(1, kl) for kl in range(1, 5)} | {(nb, kl) for nb in range(2, 7) for kl in range(5)}


def test_tile_row_counts_per_draw_series(ctx):
    """Per-draw series (Y, S2) with a ragged last window, the first row count of every (NB, KL) pair."""
    rng = np.random.default_rng(9108)
    first = {}
    for R in range(1, 96):
        first.setdefault(nb_kl(R), R)
    for R in sorted(first.values()):
        N, B = 29, 3
        t, y, s2, A, Bc, C, Dd, mu, nu = rows_case(rng, R, N, B)
        Y = rng.standard_normal((B, N)); S2 = rng.uniform(0.01, 0.1, (B, N))
        got = pj.Dataset(t, y, s2, ctx).logl_batch(A, Bc, C, Dd, mu=mu, nu=nu, Y=Y, S2=S2)
        assert kernel_name() == "tile", R
        ref = np.array([O.logl(A[i], Bc[i], C, Dd, t, Y[i] - mu[i], nu[i] * S2[i]) for i in range(B)])
        assert relerr(got, ref) < 1e-11, (R, nb_kl(R))


@pytest.mark.parametrize("R", [16, 40, 60, 80, 95])
def test_tile_row_counts_non_pd_draw(ctx, R):
    """A non-positive-definite draw among positive-definite ones: flagged as the oracle flags it, log(abs(D_n)) as the reference
    (src/celerite_solver.jl:140); the others unchanged."""
    rng = np.random.default_rng(9109 + R)
    t, y, s2, A, Bc, C, Dd, mu, nu = rows_case(rng, R, 45, 4)
    A[1] *= -1.0
    got, st = pj.Dataset(t, y, s2, ctx).logl_batch(A, Bc, C, Dd, mu=mu, nu=nu, return_status=True)
    assert kernel_name() == "tile"
    ref, rst = O.logl_batch(A, Bc, C, Dd, t, y, s2, mu, nu, nthreads=4, return_status=True)
    assert (st == rst).all() and st[1] != 0
    pd = rst == 0
    assert relerr(got[pd], ref[pd]) < 1e-11
    ok = np.isfinite(ref)
    assert relerr(got[ok], ref[ok]) < 1e-9 and (np.isnan(got) == np.isnan(ref)).all()
