"""GPU tests (-m gpu) of the tile kernel's padding (celerite_tile.hip, round 10).  The value kernel no longer rescales the registers of the last row
block's tiles that hold padding rows alone (register g > KL of row block NB - 1, KL = ceil((R - 16 (NB - 1)) / 4)), forms the diagonal of Sigma
without the padded-step test (the steps past N of the ragged window take D = 1 under the wave-uniform test of that window), and the last
elimination step of the window's LDL' no longer forms a multiplier.  Against the oracle:

* rows: R = 33, 36, 37, 40, 44, 47 (three block columns, KL = 1, 1, 2, 2, 3, 4; R a multiple of 4 — the y row in register KL — and not),
  R = 49, 52 (four block columns: the rescaling inside the update), R = 48 (KL = 0: the y row alone in the last block);
* sizes: N = 15 (one ragged window), 16 (one full window), 17 (a full window and a one-step ragged one), 47 (ragged by 15);
* 8 draws per case (two workgroups), one of them with a non-positive-definite Sigma (status 1) and one with a non-finite amplitude (status 2: its
  products with the zeros of the padding rows are NaN — they must stay in the padding); the statuses are the oracle's (0 ok, 1 some D_n <= 0,
  2 non-finite result).

Tolerance: 1e-11 relative on log L, as tests/test_gpu_tile_ksteps.py.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import pioran_jl_amd as pj  # noqa: E402
from oracle import oracle as O  # noqa: E402

ROWS = [33, 36, 37, 40, 44, 47, 49, 52, 48]
SIZES = [15, 16, 17, 47]
B = 8
NON_PD, NON_FINITE = 1, 6       # draw indices: one in each workgroup of four


@pytest.fixture(scope="module")
def ctx():
    c = pj.Context(0)
    c.set_option("scan_config", "tile")
    yield c
    c.set_option("scan_config", None)


def relerr(got, ref):
    got = np.asarray(got, float); ref = np.asarray(ref, float)
    return np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300))


def rows_case(rng, R, N):
    """R rows: ceil(R / 2) terms, the first one real (one row) when R is odd (as tests/test_gpu_tile_ksteps.py)."""
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


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("R", ROWS)
def test_tile_padding_rows(ctx, R, N):
    rng = np.random.default_rng(10_000 * R + N)
    t, y, s2, A, Bc, C, Dd, mu, nu = rows_case(rng, R, N)
    # sum(a) stays positive (D_1 > 0: the result is finite) while the first term's negative amplitude outweighs it one step on: D_2 < 0
    ratio = Bc[NON_PD, 0] / A[NON_PD, 0]
    A[NON_PD, 0] = -0.98 * A[NON_PD, 1:].sum()
    Bc[NON_PD, 0] = ratio * A[NON_PD, 0]
    A[NON_FINITE, -1] = np.inf         # the last term: its rows sit in the last row block, beside the padding
    got, st = pj.Dataset(t, y, s2, ctx).logl_batch(A, Bc, C, Dd, mu=mu, nu=nu, return_status=True)
    assert pj._lib.lib().pioran_celerite_config_name(-1).decode() == "tile"
    ref, rst = O.logl_batch(A, Bc, C, Dd, t, y, s2, mu, nu, nthreads=4, return_status=True)
    print(f"R={R} N={N}: status {st.tolist()} oracle {rst.tolist()} max rel err (PD draws) {relerr(got[rst == 0], ref[rst == 0]):.3e}")
    assert rst[NON_PD] == 1 and rst[NON_FINITE] == 2          # the case is what it says
    assert (st == rst).all()
    pd = rst == 0
    assert pd.sum() == B - 2
    assert relerr(got[pd], ref[pd]) < 1e-11
    assert relerr(got[NON_PD], ref[NON_PD]) < 1e-9           # log(abs(D_n)) as the reference: finite, the bar of tests/test_gpu_tile_ksteps.py
    assert not np.isfinite(got[NON_FINITE])
