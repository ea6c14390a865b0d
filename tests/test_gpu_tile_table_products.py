"""Tests of the tile kernel's window loop after its LDS was re-addressed (celerite_tile.hip, round 12): the LDS copies of the strictly lower tiles of T
sit in a permuted order with base registers of their own, the scratch and the staged C_K are reached through lane bases formed once, and the diagonal
of Sigma takes nu sigma2_n without a select.  Every value is the parent's bit for bit (profiles/r12_ab_same_box.txt); here the same paths against the
oracle, at the 1e-11 relative on log L of tests/test_gpu_tile_padding_rows.py and with the oracle's statuses (0 ok, 1 some D_n <= 0, 2 non-finite):

* tile positions: R = 16, 17, 32, 33, 40, 47, 48, 49, 60, 63, 80 (one to six block columns, KL = 0 .. 4, the y row in register KL and KL - 1, the rescaling
  in the two waits — up to three block columns — and inside the update), N = 15, 16, 17, 33 (a ragged window, a full one, a full and a one-step ragged one,
  two full and a ragged one), B = 1 and 5 (a workgroup not filled; one and a second, partly filled workgroup);
* R = 40 with a non-positive-definite draw (D_2 < 0: status 1, finite) and one with an infinite amplitude in the last term (status 2);
* a term whose decay over a window underflows (c (t_16 - t_0) > 745): C_K and every product with it are exact zeros;
* per-draw series (Y, S2) at R = 40 (its staging array moved with the LDS layout);
* one context, B = 5, then another prepared (c, d) with B = 9, then the first again: the table is rebuilt each time.

The table's record (window_common.h: block_rec_doubles) has no host-side description and no entry hands a record out, and this round adds no section to
it (the products C_K C_K' as table data are not built: docs/EXPERIMENTS.md section 35), so there is no rounding rule to check on the CPU; the CPU test
here (not `gpu`) holds the headline's window loop at no literal address sum, counted by tools/tile_isa_stats.py on the listing built with build.py's flags.
"""
import importlib.util
import subprocess
from pathlib import Path

import numpy as np
import pytest

import pioran_jl_amd as pj
from oracle import oracle as O

ROOT = Path(__file__).resolve().parents[1]
ROWS = [16, 17, 32, 33, 40, 47, 48, 49, 60, 63, 80]
SIZES = [15, 16, 17, 33]
BATCHES = [1, 5]


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


@pytest.mark.gpu
@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("R", ROWS)
def test_tile_positions(ctx, R, N):
    for B in BATCHES:
        rng = np.random.default_rng(120_000 * R + 10 * N + B)
        t, y, s2, A, Bc, C, Dd, mu, nu = rows_case(rng, R, N, B)
        got, st = pj.Dataset(t, y, s2, ctx).logl_batch(A, Bc, C, Dd, mu=mu, nu=nu, return_status=True)
        assert kernel_name() == "tile"
        ref, rst = O.logl_batch(A, Bc, C, Dd, t, y, s2, mu, nu, nthreads=4, return_status=True)
        print(f"R={R} N={N} B={B}: max rel err {relerr(got, ref):.3e}")
        assert (rst == 0).all() and (st == rst).all()
        assert relerr(got, ref) < 1e-11


@pytest.mark.gpu
@pytest.mark.parametrize("N", [17, 33])
def test_tile_without_nu(ctx, N):
    """No nu: the diagonal takes sigma2_n itself (the factor 1 of the kernel multiplies exactly)."""
    rng = np.random.default_rng(121_000 + N)
    t, y, s2, A, Bc, C, Dd, mu, _ = rows_case(rng, 40, N, 5)
    got, st = pj.Dataset(t, y, s2, ctx).logl_batch(A, Bc, C, Dd, mu=mu, return_status=True)
    assert kernel_name() == "tile"
    ref, rst = O.logl_batch(A, Bc, C, Dd, t, y, s2, mu, np.ones(5), nthreads=4, return_status=True)
    print(f"N={N}: max rel err {relerr(got, ref):.3e}")
    assert (rst == 0).all() and (st == rst).all()
    assert relerr(got, ref) < 1e-11


@pytest.mark.gpu
@pytest.mark.parametrize("N", [17, 33])
def test_tile_special_draws(ctx, N):
    """R = 40, 8 draws: draw 1 with D_2 < 0 (status 1, finite), draw 6 with an infinite amplitude in the last term (status 2)."""
    B, NON_PD, NON_FINITE = 8, 1, 6
    rng = np.random.default_rng(122_000 + N)
    t, y, s2, A, Bc, C, Dd, mu, nu = rows_case(rng, 40, N, B)
    # sum(a) stays positive (D_1 > 0) while the first term's negative amplitude outweighs it one step on: D_2 < 0
    ratio = Bc[NON_PD, 0] / A[NON_PD, 0]
    A[NON_PD, 0] = -0.98 * A[NON_PD, 1:].sum()
    Bc[NON_PD, 0] = ratio * A[NON_PD, 0]
    A[NON_FINITE, -1] = np.inf
    got, st = pj.Dataset(t, y, s2, ctx).logl_batch(A, Bc, C, Dd, mu=mu, nu=nu, return_status=True)
    assert kernel_name() == "tile"
    ref, rst = O.logl_batch(A, Bc, C, Dd, t, y, s2, mu, nu, nthreads=4, return_status=True)
    print(f"N={N}: status {st.tolist()} oracle {rst.tolist()}")
    assert rst[NON_PD] == 1 and rst[NON_FINITE] == 2          # the case is what it says
    assert (st == rst).all()
    pd = rst == 0
    assert pd.sum() == B - 2
    assert relerr(got[pd], ref[pd]) < 1e-11
    assert np.isfinite(got[NON_PD]) and relerr(got[NON_PD], ref[NON_PD]) < 1e-9     # log(abs(D_n)) as the reference: the bar of tests/test_gpu_tile_ksteps.py
    assert not np.isfinite(got[NON_FINITE])


@pytest.mark.gpu
@pytest.mark.parametrize("R", [40, 49])
def test_tile_underflowing_decay(ctx, R):
    """The last term decays by more than e^-745 over a window: its rows' C_K, and every product C_K C_K' with them, are exact zeros."""
    N, B = 33, 5
    rng = np.random.default_rng(123_000 + R)
    t, y, s2, A, Bc, C, Dd, mu, nu = rows_case(rng, R, N, B)
    t = np.arange(N, dtype=np.float64) + rng.uniform(0.0, 0.2, N)
    C[-1] = 50.0
    assert C[-1] * (t[16] - t[0]) > 745.0 and np.exp(-C[-1] * (t[16] - t[0])) == 0.0
    got, st = pj.Dataset(t, y, s2, ctx).logl_batch(A, Bc, C, Dd, mu=mu, nu=nu, return_status=True)
    assert kernel_name() == "tile"
    ref, rst = O.logl_batch(A, Bc, C, Dd, t, y, s2, mu, nu, nthreads=4, return_status=True)
    print(f"R={R}: max rel err {relerr(got, ref):.3e}")
    assert (rst == 0).all() and (st == rst).all()
    assert relerr(got, ref) < 1e-11


@pytest.mark.gpu
@pytest.mark.parametrize("N", [17, 33])
def test_tile_per_draw_series(ctx, N):
    R, B = 40, 5
    rng = np.random.default_rng(124_000 + N)
    t, y, s2, A, Bc, C, Dd, mu, nu = rows_case(rng, R, N, B)
    Y = rng.standard_normal((B, N)); S2 = rng.uniform(0.01, 0.1, (B, N))
    got = pj.Dataset(t, y, s2, ctx).logl_batch(A, Bc, C, Dd, mu=mu, nu=nu, Y=Y, S2=S2)
    assert kernel_name() == "tile"
    ref = np.array([O.logl(A[i], Bc[i], C, Dd, t, Y[i] - mu[i], nu[i] * S2[i]) for i in range(B)])
    print(f"N={N}: max rel err {relerr(got, ref):.3e}")
    assert relerr(got, ref) < 1e-11


@pytest.mark.gpu
def test_tile_context_reuse():
    """A fresh context: B = 5 on one (c, d), B = 9 on another, the first again."""
    c = pj.Context(0)
    c.set_option("scan_config", "tile")
    try:
        R, N = 40, 33
        rng = np.random.default_rng(125_000)
        t, y, s2, A5, Bc5, C1, D1, mu5, nu5 = rows_case(rng, R, N, 5)
        _, _, _, A9, Bc9, C2, D2, mu9, nu9 = rows_case(rng, R, N, 9)
        assert not np.array_equal(C1, C2) and not np.array_equal(D1, D2)
        ds = pj.Dataset(t, y, s2, c)
        ref5 = O.logl_batch(A5, Bc5, C1, D1, t, y, s2, mu5, nu5, nthreads=4)
        ref9 = O.logl_batch(A9, Bc9, C2, D2, t, y, s2, mu9, nu9, nthreads=4)
        for A, Bc, C, Dd, mu, nu, ref in ((A5, Bc5, C1, D1, mu5, nu5, ref5), (A9, Bc9, C2, D2, mu9, nu9, ref9), (A5, Bc5, C1, D1, mu5, nu5, ref5)):
            got, st = ds.logl_batch(A, Bc, C, Dd, mu=mu, nu=nu, return_status=True)
            assert kernel_name() == "tile"
            print(f"B={len(mu)}: max rel err {relerr(got, ref):.3e}")
            assert (st == 0).all()
            assert relerr(got, ref) < 1e-11
    finally:
        c.set_option("scan_config", None)


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_headline_loop_has_no_literal_address_sums(tmp_path):
    """celerite_tile_kernel<3, 2, false, false>: no v_add_u32 of a literal and a loop-invariant register inside the window loop (ten before round 12),
    and what tests/test_tile_isa.py holds it to."""
    build = _load("_pioran_build_isa12", ROOT / "pioran.jl_amd" / "build.py")
    stats = _load("_pioran_tile_isa_stats12", ROOT / "tools" / "tile_isa_stats.py")
    try:
        cc = build.hipcc()
    except RuntimeError:
        pytest.skip("no hipcc")
    src = "celerite_tile.hip"
    path = tmp_path / "celerite_tile.s"
    subprocess.run([cc, *build.FLAGS, *build.EXTRA_FLAGS.get(src, []), "-S", "--cuda-device-only", str(build.CSRC / src), "-o", str(path)], check=True)
    head = stats.kernel_stats(path.read_text())[(3, 2, False, False)]
    print(stats.summary(head))
    assert head["literal_address_adds"] == 0
    assert head["loop"]["v_mfma_f64_16x16x4_f64"] == 76
    assert head["meta"]["vgpr_spill_count"] == 0 and head["meta"]["sgpr_spill_count"] == 0 and head["meta"]["vgpr_count"] <= 216
