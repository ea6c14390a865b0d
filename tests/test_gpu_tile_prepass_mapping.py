"""GPU tests (-m gpu) of the workgroup mapping of the tile family's pair pre-pass (tile_pairs_mfma_kernel, celerite_tile.hip; the decode is
tile_pairs_slot, common.h).  A workgroup covers one block of 64 draws and one chunk of kPairWin = 5 windows; which block and which chunk follows from its
place in the launch order, so that the workgroups that read one chunk of the pair table run side by side behind one L2 (groups of four draw blocks; whole
eights of chunks and the chunks left over decode differently), and draw block i of a group walks the eight tiles of a window from tile 2 i on.  A wrong
decode leaves a (draw block, chunk) of the workspace unwritten or written from another chunk's table, a wrong tile order puts pairs in each other's place,
and the main kernel then reads it: the test goes through the public
batch entry with the tile family forced, against the oracle (1e-11 relative on log L over the draws of status 0, as tests/test_gpu_tile_window_order.py;
statuses the oracle's).

* B = 1, 15, 17, 63, 65, 129: a ragged 16-draw wavefront, a ragged 64-draw workgroup, two and three draw blocks;
* N = 16, 17, 81, 160 (1, 2, 6, 10 windows): one chunk, a ragged second chunk, two whole chunks — with B = 129 six workgroups, no two on the same slot;
* 1, 5, 20, 21 and 41 terms of two rows each: the instantiations <5>, <10> (from 21 terms on) and <16>;
* N = 641 (nine chunks: the decode of a whole eight of chunks, which the sizes above never reach) with up to 321 draws (two groups of draw blocks);
* per-draw series at 20 terms;
* one gradient call at B = 17, N = 81 (the reverse mode's forward pass launches the same pre-pass), against the complex-step oracle as
  tests/test_gpu_parity.py::test_tile_gradient_matches_complex_step.

The oracle is evaluated once per (terms, N) on 129 draws; the smaller batches are the leading draws of the same inputs.  Every amplitude is positive:
the oracle accepts every draw (asserted)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import pioran_jl_amd as pj  # noqa: E402
from oracle import oracle as O  # noqa: E402

BS = (1, 15, 17, 63, 65, 129)
NS = (16, 17, 81, 160)
TERMS = (1, 5, 20, 21, 41)
TOL = 1e-11
TILE_GRAD = "tile (windowed gradient, one draw per wavefront)"


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


def inputs(J, N):
    """J terms of two rows each on N time stamps, max(BS) draws (the ranges of tests/test_gpu_tile_prepass_stores.py, every amplitude positive)"""
    rng = np.random.default_rng(13000 + 1000 * J + N)
    B = max(BS)
    t = np.cumsum(rng.uniform(0.05, 2.0, N))
    y = rng.standard_normal(N)
    s2 = rng.uniform(0.01, 0.1, N)
    A = rng.uniform(0.1, 2.0, (B, J))
    Bc = rng.uniform(-0.05, 0.05, (B, J)) * A
    C = rng.uniform(0.05, 2.0, J)
    Dd = rng.uniform(0.1, 3.0, J)
    mu = rng.standard_normal(B) * 0.1
    nu = rng.uniform(0.5, 2.0, B)
    return t, y, s2, A, Bc, C, Dd, mu, nu


_cases = {}


def case(J, N):
    """Inputs of (J, N) and the oracle's log L and status on them: made once, read-only."""
    if (J, N) not in _cases:
        c = inputs(J, N)
        t, y, s2, A, Bc, C, Dd, mu, nu = c
        ref, rst = O.logl_batch(A, Bc, C, Dd, t, y, s2, mu, nu, nthreads=4, return_status=True)
        for a in (*c, ref, rst):
            a.setflags(write=False)
        _cases[(J, N)] = (c, ref, rst)
    return _cases[(J, N)]


def check(ctx, J, N, B):
    (t, y, s2, A, Bc, C, Dd, mu, nu), ref, rst = case(J, N)
    ok = rst[:B] == 0
    assert 4 * ok.sum() >= 3 * B, (J, N, B)
    ds = pj.Dataset(t, y, s2, ctx)
    got, st = ds.logl_batch(A[:B], Bc[:B], C, Dd, mu=mu[:B], nu=nu[:B], return_status=True)
    assert kernel_name() == "tile", (J, N, B)
    ds.close()
    err = relerr(got[ok], ref[:B][ok])
    print(f"J = {J} N = {N} B = {B}: {int(ok.sum())} draws of status 0, max relative error {err:.2e}")
    assert (st == rst[:B]).all(), (J, N, B)
    assert err < TOL, (J, N, B)


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("B", BS)
def test_mapping_draw_blocks_and_chunks(ctx, B, N):
    check(ctx, 20, N, B)


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("J", TERMS)
def test_mapping_terms(ctx, J, N):
    for B in (17, 129):
        check(ctx, J, N, B)


def test_mapping_whole_eights_of_chunks(ctx):
    """N = 641 (41 windows, nine chunks: a whole eight of chunks, decoded by residue modulo 8, and one chunk left over) with B = 65, 129 (a short group
    of draw blocks), 257 (one whole group and one block more) and 321 draws (a whole group and a group of two); 20 terms."""
    J, N, Bm = 20, 641, 321
    rng = np.random.default_rng(33000)
    t = np.cumsum(rng.uniform(0.05, 2.0, N))
    y = rng.standard_normal(N)
    s2 = rng.uniform(0.01, 0.1, N)
    A = rng.uniform(0.1, 2.0, (Bm, J))
    Bc = rng.uniform(-0.05, 0.05, (Bm, J)) * A
    C = rng.uniform(0.05, 2.0, J)
    Dd = rng.uniform(0.1, 3.0, J)
    mu = rng.standard_normal(Bm) * 0.1
    nu = rng.uniform(0.5, 2.0, Bm)
    ref, rst = O.logl_batch(A, Bc, C, Dd, t, y, s2, mu, nu, nthreads=4, return_status=True)
    assert 4 * (rst == 0).sum() >= 3 * Bm
    ds = pj.Dataset(t, y, s2, ctx)
    for B in (65, 129, 257, 321):
        got, st = ds.logl_batch(A[:B], Bc[:B], C, Dd, mu=mu[:B], nu=nu[:B], return_status=True)
        assert kernel_name() == "tile", B
        ok = rst[:B] == 0
        err = relerr(got[ok], ref[:B][ok])
        print(f"N = {N} B = {B}: {int(ok.sum())} draws of status 0, max relative error {err:.2e}")
        assert (st == rst[:B]).all(), B
        assert err < TOL, B
    ds.close()


@pytest.mark.parametrize("N", NS)
def test_mapping_per_draw_series(ctx, N):
    (t, y, s2, A, Bc, C, Dd, mu, nu), _, _ = case(20, N)
    rng = np.random.default_rng(23000 + N)
    Bm = max(BS)
    Y = rng.standard_normal((Bm, N)); S2 = rng.uniform(0.01, 0.1, (Bm, N))
    ref = np.array([O.logl(A[i], Bc[i], C, Dd, t, Y[i] - mu[i], nu[i] * S2[i]) for i in range(Bm)])
    assert np.isfinite(ref).all()
    ds = pj.Dataset(t, y, s2, ctx)
    for B in (17, 65, 129):
        got, st = ds.logl_batch(A[:B], Bc[:B], C, Dd, mu=mu[:B], nu=nu[:B], Y=Y[:B], S2=S2[:B], return_status=True)
        assert kernel_name() == "tile", (N, B)
        err = relerr(got, ref[:B])
        print(f"per-draw series N = {N} B = {B}: max relative error {err:.2e}")
        assert (st == 0).all(), (N, B)
        assert err < TOL, (N, B)
    ds.close()


def test_mapping_gradient(ctx):
    """B = 17, N = 81, 20 terms: the reverse mode's forward pass reads the workspace of the same pre-pass (two draw blocks' worth of wavefronts, two chunks)."""
    J, N, B = 20, 81, 17
    (t, y, s2, A, Bc, C, Dd, mu, nu), ref, rst = case(J, N)
    A, Bc, mu, nu = A[:B], Bc[:B], mu[:B], nu[:B]
    assert (rst[:B] == 0).all()
    ds = pj.Dataset(t, y, s2, ctx)
    g = ds.logl_grad(A, Bc, C, Dd, mu=mu, nu=nu, cd_grad=False)
    assert kernel_name() == TILE_GRAD
    val = ds.logl_batch(A, Bc, C, Dd, mu=mu, nu=nu)
    assert kernel_name() == "tile"
    gt = ds.logl_grad(A, Bc, C, Dd, mu=mu, nu=nu)
    assert kernel_name() == TILE_GRAD
    ds.close()
    assert (g["logl"] == val).all() and (g["status"] == 0).all() and (gt["logl"] == val).all()
    assert relerr(g["logl"], ref[:B]) < TOL
    full = O.logl_grad(A[0], Bc[0], C, Dd, t, y - mu[0], nu[0] * s2, cd=True)
    for key in ("grad_c", "grad_d"):
        assert np.max(np.abs(gt[key][0] - full[key])) <= 1e-9 * (1 + np.max(np.abs(full[key]))), key
    for i in (0, 15, 16):              # the first wavefront's first and last draw, the second wavefront's only one
        r = O.logl_grad(A[i], Bc[i], C, Dd, t, y - mu[i], nu[i] * s2)
        for key in ("grad_a", "grad_b"):
            dev = np.max(np.abs(g[key][i] - r[key]))
            print(f"gradient draw {i} {key}: max deviation {dev:.2e} on a scale of {1 + np.max(np.abs(r[key])):.2e}")
            assert dev <= 1e-9 * (1 + np.max(np.abs(r[key]))), (key, i)
            assert np.max(np.abs(gt[key][i] - r[key])) <= 1e-9 * (1 + np.max(np.abs(r[key]))), (key, i)
        gm = O.logl_dir(A[i], Bc[i], C, Dd, t, y - mu[i], nu[i] * s2, dy=-np.ones(N))
        gn = O.logl_dir(A[i], Bc[i], C, Dd, t, y - mu[i], nu[i] * s2, ds2=s2)
        assert abs(g["grad_mu"][i] - gm) <= 1e-9 * (1 + abs(gm)) and abs(g["grad_nu"][i] - gn) <= 1e-9 * (1 + abs(gn)), i
