"""GPU tests of the batched Lomb-Scargle periodogram (periodogram.hip through pioran_lombscargle_batch[_dev]) against the long-double twin
(tools/lombscargle_proto.py).

Bound: 1e-10 absolute (the power lies in [0, 1]): 10 x the worst deviation of the fp64 twin from the long-double twin on the same series and
frequency grids (tests/test_lombscargle_host.py) — the device differs from the fp64 twin in the order of its sums only.  Every test prints
the largest deviation it measured; docs/EXPERIMENTS.md (periodogram section) records them:
    shapes (N, B, F), with / without yerr: (5, 1, 3) 4.2e-14 / 4.1e-14; (37, 1, 70) 3.9e-11 / 1.1e-11; (37, 130, 1) 3.8e-11 / 6.8e-13;
    (130, 65, 33) 2.8e-11 / 5.3e-12; (490, 3, 199) 3.8e-11 / 2.9e-12.
    (fit_mean, center_data) at (130, 65, 33), with / without yerr: (1, 1) 2.8e-11 / 5.3e-12; (1, 0) 2.8e-11 / 5.3e-12; (0, 1) 4.0e-12 / 3.4e-12;
    (0, 0) 4.1e-12 / 3.3e-12.  (A loader that centres only on request gives 2.9e-9 at (1, 0) on the draw "series + 1000".)
    both output tiles: (130, 150, 70) 2.8e-11 each, (490, 260, 130) 8.2e-11 each; tiles and automatic choice bit-identical.
    chunking: unchunked against long double 5.0e-13; chunked against unchunked 0 (bit-identical), also after trim().
    900 draws in four chunks against two frequency chunks (limit 8 MB): bit-identical to the unchunked call.
    degenerate frequency: the Nyquist column NaN, the other three within the bound.
"""
import importlib.util
from pathlib import Path

import numpy as np
import pytest

import pioran_jl_amd as pj

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
BOUND = 1e-10
NAME = "periodogram (fp64 matrix product)"


def _proto():
    spec = importlib.util.spec_from_file_location("lombscargle_proto", ROOT / "tools" / "lombscargle_proto.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


P = _proto()


@pytest.fixture(scope="module")
def ctx():
    c = pj.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def simu(golden_dir):
    A = np.loadtxt(golden_dir / "simu.txt")
    return tuple(np.ascontiguousarray(A[:, k]) for k in range(3))


def _inputs(simu, N, B, F):
    """prefix of the file's series; draws: the series, the series + 1000, then seeded standard-normal series; the reference's grid of the prefix"""
    t, y, yerr = (a if N is None else a[:N] for a in simu)
    rng = np.random.default_rng(1000 * len(t) + B)
    Y = np.stack(([y, y + 1000.0] + [rng.standard_normal(len(t)) for _ in range(B)])[:B]) if B > 1 else y[None, :].copy()
    return t, Y, yerr, P.reference_grid(t, F + 1)[:-1]


def _config_name():
    return pj._lib.lib().pioran_celerite_config_name(-1).decode()


@pytest.mark.parametrize("with_err", [True, False])
@pytest.mark.parametrize("N,B,F", [(5, 1, 3), (37, 1, 70), (37, 130, 1), (130, 65, 33), (None, 3, 199)])
def test_shapes_against_long_double_twin(ctx, simu, N, B, F, with_err):
    t, Y, yerr, freq = _inputs(simu, N, B, F)
    ye = yerr if with_err else None
    ref = P.lombscargle(t, Y, ye, freq, dtype=np.longdouble)
    got, st = ctx.lombscargle(t, Y, ye, freq, return_status=True)
    assert got.shape == (B, F) and np.all(st == 0)
    err = float(np.max(np.abs(got - ref)))
    print(f"(N, B, F) = ({len(t)}, {B}, {F}), yerr {with_err}: max |device - long double| = {err:.2e}")
    assert err <= BOUND, err
    assert _config_name() == NAME


@pytest.mark.parametrize("with_err", [True, False])
@pytest.mark.parametrize("fit_mean,center_data", [(True, True), (True, False), (False, True), (False, False)])
def test_fit_mean_and_center_data(ctx, simu, fit_mean, center_data, with_err):
    t, Y, yerr, freq = _inputs(simu, 130, 65, 33)
    ye = yerr if with_err else None
    ref = P.lombscargle(t, Y, ye, freq, fit_mean, center_data, dtype=np.longdouble)
    got = ctx.lombscargle(t, Y, ye, freq, fit_mean=fit_mean, center_data=center_data)
    err = float(np.max(np.abs(got - ref)))
    print(f"fit_mean {fit_mean}, center_data {center_data}, yerr {with_err}: max |device - long double| = {err:.2e}")
    assert err <= BOUND, err


@pytest.mark.parametrize("N,B,F", [(130, 150, 70), (None, 260, 130)])
def test_both_output_tiles_of_the_product(simu, N, B, F):
    """The product kernel's two instantiations (64 x 64 and 128 x 128 columns per workgroup, context option "ls_tile") on shapes that leave a
    ragged tile beside a whole one in B, N and 2F for both, the second with more than 256 draws and 128 frequencies, and the automatic choice:
    each within the bound of the long-double twin, and all three bit-identical (one order of the sum per element)."""
    t, Y, yerr, freq = _inputs(simu, N, B, F)
    ref = P.lombscargle(t, Y, yerr, freq, dtype=np.longdouble)
    c = pj.Context(0)
    try:
        auto = c.lombscargle(t, Y, yerr, freq)
        c.set_option("ls_tile", 64)
        p64 = c.lombscargle(t, Y, yerr, freq)
        c.set_option("ls_tile", 128)
        p128 = c.lombscargle(t, Y, yerr, freq)
    finally:
        c.close()
    e64, e128 = float(np.max(np.abs(p64 - ref))), float(np.max(np.abs(p128 - ref)))
    print(f"(N, B, F) = ({len(t)}, {B}, {F}): max |device - long double| tile 64: {e64:.2e}, tile 128: {e128:.2e}; "
          f"bit-identical: {np.array_equal(p64, p128)}, automatic == both: {np.array_equal(auto, p64)}")
    assert e64 <= BOUND and e128 <= BOUND
    assert np.array_equal(p64, p128) and np.array_equal(auto, p64)


@pytest.fixture(scope="module")
def irregular():
    """N = 1000 irregular times (gaps 0.05 + Exponential(0.95)), 70 series, 300 frequencies of the reference's grid"""
    rng = np.random.default_rng(7)
    t = np.cumsum(0.05 + rng.exponential(0.95, 1000))
    yerr = rng.uniform(0.05, 0.2, 1000)
    Y = rng.standard_normal((70, 1000)) + np.sin(0.3 * t)[None, :] * rng.uniform(0, 2, 70)[:, None] + rng.uniform(-5, 5, 70)[:, None]
    return t, Y, yerr, P.reference_grid(t, 301)[:-1]


def test_chunking_does_not_change_the_result(irregular):
    t, Y, yerr, freq = irregular
    c = pj.Context(0)
    try:
        whole = c.lombscargle(t, Y, yerr, freq)
        ref = P.lombscargle(t, Y, yerr, freq, dtype=np.longdouble)
        err0 = float(np.max(np.abs(whole - ref)))
        c.trim()
        c.set_option("workspace_limit_mb", 1)     # staged series + powers may take 512 KB: 35 draws a chunk, two chunks; the table of the smallest frequency
        # chunk (64 frequencies: 1 MB) is over its half of this budget, so the sizer ends at that smallest chunk: five frequency chunks
        parts = c.lombscargle(t, Y, yerr, freq)
        err = float(np.max(np.abs(parts - whole)))
        same = bool(np.array_equal(parts, whole))
        print(f"unchunked against long double {err0:.2e}; chunked against unchunked {err:.2e}, bit-identical: {same}")
        assert err0 <= BOUND and err <= BOUND
        assert same
        c.trim()
        again = c.lombscargle(t, Y, yerr, freq)
        assert np.array_equal(again, parts)
        c.set_option("workspace_limit_mb", None)
        c.trim()
        assert np.array_equal(c.lombscargle(t, Y, yerr, freq), whole)
    finally:
        c.close()


def test_draw_chunks_share_one_frequency_chunking(irregular):
    """Several draw chunks, each against the same TWO frequency chunks: N = 1000, F = 300, B = 900 under workspace_limit_mb = 8.  Staged series
    and powers may take 4 MB: 900 -> 225 draws a chunk (2.3 MB), four chunks.  The table may take 4 MB: all 300 frequencies (320 padded) need
    5.4 MB, 150 (192 padded) 3.2 MB, so 192 + 108.  The frequency chunk is sized once per call: sized again per draw chunk it would grow to all
    300 once the first chunk's table is allocated (the allowance counts what the buffer holds), and a later draw chunk must then not take
    the table for built.  Bit-identical to the unchunked call."""
    t, Y70, yerr, freq = irregular
    rng = np.random.default_rng(70)
    Y = np.concatenate([Y70, rng.standard_normal((830, 1000)) * rng.uniform(0.5, 3, 830)[:, None] + rng.uniform(-50, 50, 830)[:, None]])
    c = pj.Context(0)
    try:
        whole, st0 = c.lombscargle(t, Y, yerr, freq, return_status=True)
        assert np.array_equal(whole[:70], c.lombscargle(t, Y70, yerr, freq))
        c.trim()
        c.set_option("workspace_limit_mb", 8)
        parts, st = c.lombscargle(t, Y, yerr, freq, return_status=True)
        again = c.lombscargle(t, Y, yerr, freq)          # buffers of the first chunked call still allocated
        c.set_option("workspace_limit_mb", None)
    finally:
        c.close()
    print(f"900 draws in four chunks against two frequency chunks: max |chunked - unchunked| = {float(np.max(np.abs(parts - whole))):.2e}, "
          f"bit-identical: {np.array_equal(parts, whole)}, repeated: {np.array_equal(again, whole)}")
    assert np.all(st0 == 0) and np.all(st == 0) and np.all(np.isfinite(whole))
    assert np.array_equal(parts, whole) and np.array_equal(again, whole)


def test_closing_a_context_frees_the_frequency_table():
    """N = F = 2048, B = 4: the table of the frequency chunk (blstab) is 2 * 2048 * 2048 doubles = 64 MiB before the growth slack.  Contexts that are
    closed without trim() must give it back: after a warm-up cycle (code object, the runtime's pools), three more cycles of Context, lombscargle,
    close() may not lower the device's free memory by more than 64 MiB (the margin test_gradient_workspace_is_small leaves for other tenants),
    where a context that kept its table would lose 192 MiB.  The free memory is device-wide: another process allocating meanwhile can fail this."""
    import torch
    N = F = 2048
    rng = np.random.default_rng(2048)
    t = np.cumsum(0.05 + rng.exponential(0.95, N))
    yerr = rng.uniform(0.05, 0.2, N)
    Y = rng.standard_normal((4, N)) + np.sin(0.3 * t)[None, :]
    freq = P.reference_grid(t, F + 1)[:-1]

    def cycle():
        c = pj.Context(0)
        try:
            return c.lombscargle(t, Y, yerr, freq)
        finally:
            c.close()

    first = cycle()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(3):
        last = cycle()
    free1 = torch.cuda.mem_get_info()[0]
    print(f"free memory before / after three cycles without trim(): {free0} / {free1} bytes, lost {(free0 - free1) / 2**20:.1f} MiB")
    assert free1 >= free0 - (64 << 20)
    assert np.all(np.isfinite(first)) and np.array_equal(last, first)


def test_device_form_equals_host_form(ctx, irregular):
    import torch
    t, Y, yerr, freq = irregular
    B, N = Y.shape
    F = len(freq)
    host, hst = ctx.lombscargle(t, Y, yerr, freq, return_status=True)
    dev = torch.device("cuda:0")
    dt, dY, de, df = (torch.from_numpy(a).to(dev) for a in (t, Y, yerr, freq))
    dP = torch.full((B, F), -1.0, dtype=torch.float64, device=dev)
    dS = torch.full((B,), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ctx.lombscargle_dev(N, B, F, dt.data_ptr(), dY.data_ptr(), de.data_ptr(), df.data_ptr(), dpower=dP.data_ptr(), dstatus=dS.data_ptr())
    ctx.synchronize()
    assert np.array_equal(dP.cpu().numpy(), host) and np.array_equal(dS.cpu().numpy(), hst)
    # without errors and without a status array
    ctx.lombscargle_dev(N, B, F, dt.data_ptr(), dY.data_ptr(), 0, df.data_ptr(), dpower=dP.data_ptr())
    ctx.synchronize()
    assert np.array_equal(dP.cpu().numpy(), ctx.lombscargle(t, Y, None, freq))


def test_status_of_constant_and_non_finite_draws(ctx, simu):
    t, Y, yerr, freq = _inputs(simu, 130, 65, 33)
    clean = ctx.lombscargle(t, Y, yerr, freq)
    Z = Y.copy()
    Z[3] = 4.25
    Z[40, 77] = np.nan
    Z[64, 0] = np.inf
    got, st = ctx.lombscargle(t, Z, yerr, freq, return_status=True)
    bad = np.array([3, 40, 64])
    want = np.zeros(65, dtype=np.int32); want[bad] = 2
    assert np.array_equal(st, want)
    assert np.all(np.isnan(got[bad]))
    keep = np.setdiff1d(np.arange(65), bad)
    assert np.array_equal(got[keep], clean[keep])
    # a constant that the weights do not reproduce exactly is constant all the same
    Z[3] = 1000.1
    assert ctx.lombscargle(t, Z, None, freq, return_status=True)[1][3] == 2


def test_degenerate_frequency_gives_a_nan_column(ctx):
    """regular sampling: sin(omega t) vanishes at the grid's Nyquist frequency, D = 0 there"""
    rng = np.random.default_rng(3)
    t = np.arange(64, dtype=np.float64) * 0.5
    Y = rng.standard_normal((5, 64))
    freq = np.array([0.11, 0.37, 1.0, 0.83])      # Nyquist: 1 / (2 * 0.5) = 1
    got, st = ctx.lombscargle(t, Y, None, freq, return_status=True)
    assert np.all(st == 0)
    assert np.all(np.isnan(got[:, 2])) and np.all(np.isfinite(got[:, [0, 1, 3]]))
    ref = P.lombscargle(t, Y, None, freq[[0, 1, 3]], dtype=np.longdouble)
    assert float(np.max(np.abs(got[:, [0, 1, 3]] - ref))) <= BOUND


def test_lsp_ppc_is_simulate_then_lombscargle(ctx, simu):
    from oracle import oracle as O
    t, y, yerr = (a[:37] for a in simu)
    B = 4
    A, Bc, C, Dd, mu, nu = O.theta_to_coefs(O.synthetic_theta(B, t, y), t, 4, "SHO")
    freq_in = P.reference_grid(t, 21)
    f, power, quant = pj.lsp_ppc(np.random.default_rng(11), t, yerr, A, Bc, C, Dd, mu=mu, nu=nu, frequencies=freq_in, ctx=ctx)
    assert _config_name() == NAME
    rng = np.random.default_rng(11)
    latent = ctx.simulate(A, Bc, C, Dd, t, np.zeros(len(t)), rng.standard_normal((B, len(t))))
    Y = latent + np.sqrt(nu)[:, None] * yerr[None, :] * rng.standard_normal((B, len(t))) + mu[:, None]
    assert np.array_equal(f, freq_in[:-1]) and power.shape == (B, 20) and quant.shape == (5, 20)
    assert np.array_equal(power, pj.lombscargle(t, Y, yerr, frequencies=freq_in[:-1], ctx=ctx))
    assert np.array_equal(quant, np.quantile(power, [0.025, 0.16, 0.5, 0.84, 0.975], axis=0))
    # default grid: the reference's 1000 points, last one dropped
    f2, p2, q2 = pj.lsp_ppc(np.random.default_rng(11), t, yerr, A, Bc, C, Dd, n_frequencies=30, ctx=ctx)
    assert np.array_equal(f2, pj.lsp_ppc_frequencies(t, 30)[:-1]) and p2.shape == (B, 29) and q2.shape == (5, 29)
    # the other normalisations are functions of the standard power
    one = pj.lombscargle(t, Y[0], yerr, frequencies=f, ctx=ctx)
    assert one.shape == (20,) and np.array_equal(one, power[0])
    assert np.array_equal(pj.lombscargle(t, Y[0], yerr, frequencies=f, normalization="model", ctx=ctx), one / (1 - one))
    assert np.array_equal(pj.lombscargle(t, Y[0], yerr, frequencies=f, normalization="log", ctx=ctx), -np.log(1 - one))
