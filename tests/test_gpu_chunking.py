"""GPU tests (-m gpu): the batched host-pointer entries cut their draws into chunks that fit the workspace budget; a call that runs in
several chunks must return what the same call returns in one.

Every case runs twice on the same inputs: whole, and again after ctx.trim() with "workspace_limit_mb" = 1 (the trim matters: capacity a
context already holds adds to what a call may take).  Compared between the two runs: the kernel family that ran, the status, and the values
— bit for bit where every draw is its own workgroup (log L, means, variances, realisations), to 1e-13 (1 + max |ref|) for the gradient
outputs (sums over lanes by LDS atomics, whose order is not fixed: the bound test_tile_gradient_dispatch_chunks_and_flagged_draws uses for
the same comparison).  One draw of every case is held to the CPU oracle at the tolerance of the entry's own test in test_gpu_parity.py /
test_gpu_predict_var.py.

Shapes: N = 300 irregular times, J = 10 (R = 20 rows: NB = 2 block columns, 19 windows of 16 steps), B = 23 draws (23 -> 11 -> 5 -> 2 -> 1
by halving: the last chunk is ragged whatever the entry settles on), M = 37 evaluation times, mu and nu per draw.  1 MB = 131072 doubles;
next to each case: the doubles per draw from the pioran_*_workspace_doubles formula of its workspace, which 23 draws exceed.

The last five cases cover the other way a call is cut up: (c, d) per draw on a route without per-draw-table kernels runs draw by draw, and must
return what the same draws return as one-draw calls."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import pioran_jl_amd as pj  # noqa: E402
from oracle import oracle as O  # noqa: E402

N, J, B, M = 300, 10, 23, 37
GRAD_KEYS = ("grad_a", "grad_b", "grad_c", "grad_d", "grad_mu", "grad_nu", "grad_y", "grad_sigma2", "grad_shift")


@pytest.fixture(scope="module")
def ctx():
    return pj.Context(0)


@pytest.fixture(scope="module")
def data():
    """One series, B prior draws of SHO-10 sharing (c, d), B draws with (c, d) of their own in every term, evaluation times, normals."""
    rng = np.random.default_rng(2323)
    t = np.cumsum(rng.uniform(0.05, 2.0, N)); y = rng.standard_normal(N); s2 = rng.uniform(0.01, 0.1, N)
    A, Bc, C, Dd, mu, nu = O.theta_to_coefs(O.synthetic_theta(B, t, y), t, J, "SHO")
    Ap = rng.uniform(0.1, 2.0, (B, J)); Bp = rng.uniform(-0.05, 0.05, (B, J)) * Ap
    Cp = rng.uniform(0.05, 2.0, (B, J)); Dp = rng.uniform(0.0, 3.0, (B, J))
    mup = rng.standard_normal(B) * 0.1; nup = rng.uniform(0.5, 2.0, B)
    tau = np.sort(np.concatenate([rng.uniform(t[0] - 2, t[-1] + 2, M - 3), t[[0, N // 2, N - 1]]]))
    d = dict(t=t, y=y, s2=s2, shared=(A, Bc, C, Dd, mu, nu), perdraw=(Ap, Bp, Cp, Dp, mup, nup), tau=tau, tau_any=rng.permutation(tau),
             q=rng.standard_normal((B, N)))
    for v in d.values():
        for a in (v if isinstance(v, tuple) else (v,)):
            a.setflags(write=False)
    return d


def name():
    return pj._lib.lib().pioran_celerite_config_name(-1).decode()


def whole_and_chunked(ctx, call, options=()):
    """call() once as it comes and once with nothing held and a 1 MB workspace budget: (result, kernel family) of each."""
    for k in options:
        ctx.set_option(k, True)
    try:
        whole = (call(), name())
        ctx.trim()
        ctx.set_option("workspace_limit_mb", 1)
        try:
            chunked = (call(), name())
        finally:
            ctx.set_option("workspace_limit_mb", 0)
    finally:
        for k in options:
            ctx.set_option(k, False)
    return whole, chunked


def same_values(label, whole, chunked, family):
    (w, fw), (c, fc) = whole, chunked
    print(f"{label}: whole on '{fw}', chunked on '{fc}'")
    assert fw == fc == family
    for key in w:
        if w[key] is None:
            assert c[key] is None, key
            continue
        equal = np.array_equal(w[key], c[key], equal_nan=True)
        print(f"{label}: {key} bit-identical: {equal}")
        if key in GRAD_KEYS:
            ok = np.isfinite(w[key])
            assert np.array_equal(ok, np.isfinite(c[key])), key
            dev = np.max(np.abs(w[key][ok] - c[key][ok])); scale = 1 + np.max(np.abs(w[key][ok]))
            print(f"{label}: {key} max |delta| = {dev:.2e}  (bound {1e-13 * scale:.2e})")
            assert dev <= 1e-13 * scale, key
        else:
            assert equal, key


def first_good(status):
    good = np.flatnonzero(status == 0)
    assert len(good) > 0
    return int(good[0])


# ---- posterior mean ---------------------------------------------------------------------------------------------------------------------
# windowed: pioran_block_store_workspace_doubles(., 2) = 19 windows x NB 256 = 9728, pioran_predict_q_workspace_doubles = N (2 R + 1) +
#           2 x 3 segments x R x 3 = 12660: 22388 doubles per draw, 23 draws = 4.1 MB
# no_block: pioran_predict_workspace_doubles = N (3 R + 3) = 18900 doubles per draw, 23 draws = 3.5 MB — the step-by-step path takes its 256-draw
#           chunk whatever the budget says: the two runs are the same launches, and stay so
@pytest.mark.parametrize("options,family", [((), "block (windowed prediction)"), (("no_block",), "wide (step-by-step prediction)")])
def test_predict_shared(ctx, data, options, family):
    t, y, s2, tau = data["t"], data["y"], data["s2"], data["tau"]
    A, Bc, C, Dd, mu, nu = data["shared"]
    ds = pj.Dataset(t, y, s2, ctx)

    def call():
        mean, st = ds.predict(A, Bc, C, Dd, tau, mu=mu, nu=nu, return_status=True)
        return dict(mean=mean, status=st)
    whole, chunked = whole_and_chunked(ctx, call, options)
    ds.close()
    same_values(f"predict {family}", whole, chunked, family)
    i = first_good(whole[0]["status"])
    ref = O.predict(A[i], Bc[i], C, Dd, tau, t, y - mu[i], nu[i] * s2) + mu[i]
    assert np.max(np.abs(whole[0]["mean"][i] - ref)) <= 1e-9 * max(1.0, np.max(np.abs(ref)))


# per-draw tables: pioran_block_table_doubles = 19 x (1664 + 256 J) = 80256, pioran_block_gtab_doubles = 19 x 2120 = 40280, the stores and the Q
# workspace as above 22388, pioran_predict_tau_workspace_doubles = M 3 x 32 = 3552 per draw, the means M: 146513 doubles per draw — ONE draw is
# over 1 MB, the entry goes draw by draw
def test_predict_per_draw(ctx, data):
    t, y, s2, tau = data["t"], data["y"], data["s2"], data["tau"]
    A, Bc, C, Dd, mu, nu = data["perdraw"]
    ds = pj.Dataset(t, y, s2, ctx)

    def call():
        mean, st = ds.predict(A, Bc, C, Dd, tau, mu=mu, nu=nu, return_status=True)
        return dict(mean=mean, status=st)
    whole, chunked = whole_and_chunked(ctx, call)
    ds.close()
    same_values("predict per-draw", whole, chunked, "block (windowed prediction, per-draw tables)")
    i = first_good(whole[0]["status"])
    ref = O.predict(A[i], Bc[i], C[i], Dd[i], tau, t, y - mu[i], nu[i] * s2) + mu[i]
    assert np.max(np.abs(whole[0]["mean"][i] - ref)) <= 1e-9 * max(1.0, np.max(np.abs(ref)))


# ---- posterior variance -----------------------------------------------------------------------------------------------------------------
# pioran_predict_var_workspace_doubles = N (R + 2) + M (32 + 1) = 7821 doubles per draw: 23 draws = 1.44 MB, 11 draws = 0.69 MB
def test_predict_var_shared(ctx, data):
    t, y, s2, tau = data["t"], data["y"], data["s2"], data["tau_any"]
    A, Bc, C, Dd, mu, nu = data["shared"]
    ds = pj.Dataset(t, y, s2, ctx)

    def call():
        var, st = ds.predict_var(A, Bc, C, Dd, tau, nu=nu, return_status=True)
        return dict(var=var, status=st)
    whole, chunked = whole_and_chunked(ctx, call)
    ds.close()
    same_values("predict_var", whole, chunked, "wide (step-by-step variance)")
    i = first_good(whole[0]["status"])
    ref = np.diag(O.predict_cov_numpy(A[i], Bc[i], C, Dd, tau, t, nu[i] * s2))
    assert np.max(np.abs(whole[0]["var"][i] - ref)) <= 1e-10 * A[i].sum()


# ---- value and gradient -----------------------------------------------------------------------------------------------------------------
# windowed (with and without the series gradients): pioran_block_grad_workspace_doubles = 19 x (NB^2 256 + 3 NB 256 + 256 + 320) = 59584 doubles
#           per draw: two draws are 0.95 MB, 23 are 11 MB
# no_block: pioran_grad_workspace_doubles (two rows per lane, checkpoints every 64 steps) = (2 x 64 + 5) x 256 x 4 + N x 33 + ... > 146000
#           doubles per draw: one draw is over 1 MB
@pytest.mark.parametrize("options,series,family", [((), False, "block (windowed gradient)"), (("no_block",), False, "wide (step-by-step gradient)"),
                                                   ((), True, "block (windowed gradient)")])
def test_logl_grad_shared(ctx, data, options, series, family):
    t, y, s2 = data["t"], data["y"], data["s2"]
    A, Bc, C, Dd, mu, nu = data["shared"]
    ds = pj.Dataset(t, y, s2, ctx)
    whole, chunked = whole_and_chunked(ctx, lambda: ds.logl_grad(A, Bc, C, Dd, mu=mu, nu=nu, series_grad=series), options)
    ds.close()
    same_values(f"logl_grad {family} series={series}", whole, chunked, family)
    g = whole[0]
    ok = g["status"] == 0
    i = first_good(g["status"])
    ref = O.logl_batch(A, Bc, C, Dd, t, y, s2, mu, nu)
    assert np.max(np.abs(g["logl"][ok] - ref[ok]) / np.abs(ref[ok])) < 1e-11
    rg = O.logl_grad(A[i], Bc[i], C, Dd, t, y - mu[i], nu[i] * s2, cd=True, series=series)
    for key in ("grad_a", "grad_b", "grad_c", "grad_d") + (("grad_y",) if series else ()):
        assert np.max(np.abs(g[key][i] - rg[key])) <= 1e-9 * (1 + np.max(np.abs(rg[key]))), key


# per-draw tables: block table 80256 + reverse table 40280 + pioran_block_grad_workspace_doubles 59584 = 180120 doubles per draw: one draw is 1.4 MB
def test_logl_grad_per_draw(ctx, data):
    t, y, s2 = data["t"], data["y"], data["s2"]
    A, Bc, C, Dd, mu, nu = data["perdraw"]
    ds = pj.Dataset(t, y, s2, ctx)
    whole, chunked = whole_and_chunked(ctx, lambda: ds.logl_grad(A, Bc, C, Dd, mu=mu, nu=nu))
    ds.close()
    same_values("logl_grad per-draw", whole, chunked, "block (windowed gradient, per-draw tables)")
    g = whole[0]
    ok = g["status"] == 0
    i = first_good(g["status"])
    ref = O.logl_batch(A, Bc, C, Dd, t, y, s2, mu, nu)
    assert np.max(np.abs(g["logl"][ok] - ref[ok]) / np.abs(ref[ok])) < 1e-11
    rg = O.logl_grad(A[i], Bc[i], C[i], Dd[i], t, y - mu[i], nu[i] * s2, cd=True)
    for key in ("grad_a", "grad_b", "grad_c", "grad_d"):
        assert np.max(np.abs(g[key][i] - rg[key])) <= 1e-9 * (1 + np.max(np.abs(rg[key]))), key


# ---- simulation -------------------------------------------------------------------------------------------------------------------------
# shared:   pioran_block_store_workspace_doubles(., 3) = 19 x (NB 256 + 320) = 15808 doubles per draw: 23 draws = 2.9 MB, 5 draws = 0.63 MB
# per draw: + the block table 80256 + 3 N = 96964 doubles per draw: two draws are 1.55 MB
@pytest.mark.parametrize("which,family", [("shared", "block (windowed simulation)"), ("perdraw", "block (windowed simulation, per-draw tables)")])
def test_simulate(ctx, data, which, family):
    t, s2, q = data["t"], data["s2"], data["q"]
    A, Bc, C, Dd, mu, nu = data[which]
    whole, chunked = whole_and_chunked(ctx, lambda: dict(y=ctx.simulate(A, Bc, C, Dd, t, s2, q)))
    same_values(f"simulate {which}", whole, chunked, family)
    ys = whole[0]["y"]
    assert np.isfinite(ys).all()
    c0, d0 = (C[0], Dd[0]) if which == "perdraw" else (C, Dd)
    ref = O.sim(A[0], Bc[0], c0, d0, t, s2, q[0])
    assert np.max(np.abs(ys[0] - ref)) <= 1e-9 * np.max(np.abs(ref))


# ---- log L with (c, d) per draw: per-draw tables of the windowed kernel -------------------------------------------------------------------
# pioran_block_table_doubles = 80256 doubles per draw: two draws are 1.3 MB
def test_logl_batch_per_draw_tables(ctx, data):
    t, y, s2 = data["t"], data["y"], data["s2"]
    A, Bc, C, Dd, mu, nu = data["perdraw"]
    ds = pj.Dataset(t, y, s2, ctx)

    def call():
        logl, st = ds.logl_batch(A, Bc, C, Dd, mu=mu, nu=nu, return_status=True)
        return dict(logl=logl, status=st)
    whole, chunked = whole_and_chunked(ctx, call)
    ds.close()
    same_values("logl_batch per-draw", whole, chunked, "block (per-draw tables)")
    ok = whole[0]["status"] == 0
    assert ok.any()
    ref = O.logl_batch(A, Bc, C, Dd, t, y, s2, mu, nu)
    assert np.max(np.abs(whole[0]["logl"][ok] - ref[ok]) / np.abs(ref[ok])) < 1e-11


# ---- (c, d) per draw where the windowed per-draw-table kernels do not take the call: draw by draw -------------------------------------------
# The entries then run every draw as a one-draw call of their own.  One call with three draws of the per-draw set (a first, a middle and a last
# one: a wrong offset into any of the arrays shows in at least one of them) against the same three draws as three one-draw calls, which take the
# shared-(c, d) body directly: same kernel family, same status, same values under the rules of same_values.
FALLBACK_DRAWS = 3


def batched_and_one_by_one(ctx, call, options=()):
    """call(sl) -> dict of arrays with the draws on axis 0: once for all FALLBACK_DRAWS draws, and once per draw, the results joined."""
    for k in options:
        ctx.set_option(k, True)
    try:
        batched = (call(slice(0, FALLBACK_DRAWS)), name())
        singles = [call(slice(b, b + 1)) for b in range(FALLBACK_DRAWS)]
        joined = {k: None if singles[0][k] is None else np.concatenate([r[k] for r in singles]) for k in singles[0]}
        one_by_one = (joined, name())
    finally:
        for k in options:
            ctx.set_option(k, False)
    assert set(batched[0]) == set(joined)
    for k, v in batched[0].items():
        assert v is None or v.shape == joined[k].shape, k
    return batched, one_by_one


def test_predict_draw_by_draw(ctx, data):
    t, y, s2, tau = data["t"], data["y"], data["s2"], data["tau"]
    A, Bc, C, Dd, mu, nu = data["perdraw"]
    ds = pj.Dataset(t, y, s2, ctx)

    def call(sl):
        mean, st = ds.predict(A[sl], Bc[sl], C[sl], Dd[sl], tau, mu=mu[sl], nu=nu[sl], return_status=True)
        return dict(mean=mean, status=st)
    batched, single = batched_and_one_by_one(ctx, call, ("no_block",))
    ds.close()
    same_values("predict draw by draw", batched, single, "wide (step-by-step prediction)")
    first_good(batched[0]["status"])


def test_predict_var_draw_by_draw(ctx, data):
    t, y, s2, tau = data["t"], data["y"], data["s2"], data["tau_any"]
    A, Bc, C, Dd, mu, nu = data["perdraw"]
    ds = pj.Dataset(t, y, s2, ctx)

    def call(sl):
        var, st = ds.predict_var(A[sl], Bc[sl], C[sl], Dd[sl], tau, nu=nu[sl], return_status=True)
        return dict(var=var, status=st)
    batched, single = batched_and_one_by_one(ctx, call)
    ds.close()
    same_values("predict_var draw by draw", batched, single, "wide (step-by-step variance)")
    first_good(batched[0]["status"])


def test_simulate_draw_by_draw(ctx, data):
    t, s2, q = data["t"], data["s2"], data["q"]
    A, Bc, C, Dd, mu, nu = data["perdraw"]
    batched, single = batched_and_one_by_one(ctx, lambda sl: dict(y=ctx.simulate(A[sl], Bc[sl], C[sl], Dd[sl], t, s2, q[sl])), ("no_block",))
    same_values("simulate draw by draw", batched, single, "wide (step-by-step simulation)")
    assert np.isfinite(batched[0]["y"]).all()


def test_logl_grad_draw_by_draw(ctx, data):
    t, y, s2 = data["t"], data["y"], data["s2"]
    A, Bc, C, Dd, mu, nu = data["perdraw"]
    ds = pj.Dataset(t, y, s2, ctx)
    batched, single = batched_and_one_by_one(ctx, lambda sl: ds.logl_grad(A[sl], Bc[sl], C[sl], Dd[sl], mu=mu[sl], nu=nu[sl], series_grad=True),
                                             ("no_block",))
    ds.close()
    same_values("logl_grad draw by draw", batched, single, "wide (step-by-step gradient)")
    first_good(batched[0]["status"])


# the shifted log-flux form has no per-draw-table kernel: with (c, d) per draw it goes draw by draw under every option.  The data set holds a
# positive series (raw flux), every shift lies below its minimum
def test_logl_grad_shift_draw_by_draw(ctx, data):
    t, s2 = data["t"], data["s2"]
    A, Bc, C, Dd, mu, nu = data["perdraw"]
    flux = np.exp(0.5 * data["y"])
    shift = flux.min() * np.linspace(0.1, 0.9, B)
    ds = pj.Dataset(t, flux, s2, ctx)
    batched, single = batched_and_one_by_one(ctx, lambda sl: ds.logl_grad(A[sl], Bc[sl], C[sl], Dd[sl], mu=mu[sl], nu=nu[sl], shift=shift[sl]))
    ds.close()
    assert batched[0]["grad_shift"] is not None
    same_values("logl_grad shift draw by draw", batched, single, "block (windowed gradient)")
    first_good(batched[0]["status"])
