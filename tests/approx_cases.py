"""Cases and bar for the forward `approx` on the device (approx_kernel, csrc/approx.hip: theta -> the celerite coefficients (a, b) and, for QPO
features, their (c, d); Dataset.logpdf_theta(return_coefs=True), Dataset.logpdf_theta_grad(qpo=..., approx_on="device", return_coef_grads=True)),
shared by the CPU tests (the host mirrors, the numpy restatement of the kernel's order and its seeded mistakes, tests/test_approx_host.py) and the
GPU tests (tests/test_gpu_approx_truth.py).  A plain module, no fixtures, in the style of tests/theta_grad_cases.py.

combos()   (model, basis, integrated, J, n_qpo, number of draws, S_low, S_high):
             continuum    every combo of theta_grad_cases.combos(): J in {2, 3, 20, 33} x both models x both bases x both normalisations, six draws
                          each, and the grids whose LU factorisation interchanges rows (SHO J = 48, DRWCelerite J = 72), both models, two draws;
             CHAINED      SHO J = 60, single bend, two draws: on the two grids above every interchange is of two neighbouring rows that no other
                          interchange touches, so their order does not matter; J = 60 is the smallest grid where interchanges share rows
                          (38 of them; DRWCelerite: J = 89) and a solve that applies them in another order is wrong;
             features     every combo of qpo_grad_cases.combos() (n_qpo 1 and 2; their coefficients are stored in approx_qpo_vjp_truth.npz: stored()),
                          and N_QPO_MAX: n_qpo = 8, the entries' limit, single bend, SHO, J = 20, in both normalisations;
             OTHER_GRID   one continuum combo per basis on a grid with S_low = 5, S_high = 40 (f_0 = f_min / 5, f_M = 40 f_max), J = 20.
draws()    theta_grad_cases.draws / qpo_grad_cases.draws with their edges (alpha1 < 0, f1 = f_min, f1 = f_max, f2 = 1.05 f1; Q = 0.51, Q = 50,
           f0 = f_min, f0 = 2 f_max in the first feature).
truth()    tests/golden/approx_truth.npz (tools/make_approx_truth.py: approx restated in mpmath at 50 digits from the fp64 inputs): theta, norm, qpo,
           the coefficients A, B, C, D in full rows [n][Jt] with the continuum's (c, d) from the grid, the amplitudes x = B^-1 p [n][J] and the
           normalising integral I [n].  For the stored() combos A .. D are approx_qpo_vjp_truth.npz's (the tool asserts that it reproduces them).
batch()    B rows for a launch: the combo's draws in turn.

Deviations (deviations()), per draw:
    a, b        max_j |got_j - truth_j| / max_j |a_truth_j|        (the scale of tests/test_gpu_parity.py's 1e-9 assertions)
    qc, qd      the features' (c, d): max_q |got_q - truth_q| / |truth_q|
    gc, gd      the grid's (c, d) of the continuum columns: max_j |got_j - truth_j| / |truth_j|; where the truth is 0 (d of the one-row terms of
                DRWCelerite) only an exact 0.0 agrees
and check() asserts, not masks, that b of the DRWCelerite second half and d of its one-row terms are exactly 0.0.

The bar, per combo and array: max(MARGIN x ref_dev, FLOOR).  ref_dev (ref_dev()) is the largest deviation over the combo's own draws, in the same
scale and from the same truth, of the fp64 evaluation that is not the code under test: pioran_jl_amd.approx_batch (continuum) or approx_batch_qpo
(features) — numpy's pow, log, arctan2 and LAPACK's solve — never device output.  MARGIN = 20 and FLOOR = 256 eps are those of tests/grad_cases.py,
for the reason given there: the kernel forms the same sums in another order (fused multiply-adds in the LU solve, ocml's pow, log, atan2), which
moves a result by a few of the reference's own roundings, not by orders of magnitude.  No figure is fixed in advance: tests/test_approx_host.py
prints ref_dev per combo and asserts only that it is positive for (a, b) and far below 1e-9; profiles/approx_truth.txt holds the figures measured
when the truth was written (a, b: at most 90 eps up to J = 33 and with features, 331 .. 2245 eps on the pivoting grids) and the device's beside
them.

END_TO_END  the combos whose log L is held to -oracle.dense_nll_truth on the truth coefficients: the series is the first E2E_N points of
            tests/golden/simu.txt with the variances yerr^2 x E2E_S2_SCALE (per combo), chosen so that every draw has status 0 and ratio = nu min(sigma2) /
            sum(a) >= 1e-5 in all three variants (plain; mu, nu; shift) — tests/test_approx_host.py checks that with the fp64 oracle, and that
            no draw's log L is a sum that cancels to less than 0.02 of its absolute terms (the bar is relative to |log L|; E2E_SEED, chosen on
            the truth alone)."""
import functools
from pathlib import Path

import numpy as np

import qpo_grad_cases as QC
import theta_grad_cases as TC

ROOT = Path(__file__).resolve().parents[1]
MARGIN, FLOOR = TC.MARGIN, TC.FLOOR
EPS = float(np.finfo(float).eps)
F_MIN, F_MAX = TC.F_MIN, TC.F_MAX
BASIS_NAME = TC.BASIS_NAME
LAUNCH_B = (1, 63, 64, 65, 130)          # around the 64-thread block of the kernel, and more than two blocks
N_QPO_MAX = ((0, 0, 1, 20, 8, 4, TC.S_LOW, TC.S_HIGH), (0, 0, 0, 20, 8, 4, TC.S_LOW, TC.S_HIGH))
OTHER_GRID = ((0, 0, 1, 20, 0, 6, 5.0, 40.0), (1, 1, 1, 20, 0, 6, 5.0, 40.0))
CHAINED = ((0, 0, 1, 60, 0, 2, TC.S_LOW, TC.S_HIGH),)
ARRAYS = ("a", "b", "qc", "qd", "gc", "gd")
PLACE_COMBOS = ((0, 0, 1, 3, 1, 4, TC.S_LOW, TC.S_HIGH), (1, 1, 1, 20, 2, 4, TC.S_LOW, TC.S_HIGH), (1, 0, 0, 20, 2, 4, TC.S_LOW, TC.S_HIGH),
                (0, 0, 1, 48, 1, 2, TC.S_LOW, TC.S_HIGH))
END_TO_END = ((0, 0, 1, 20, 0, 6, TC.S_LOW, TC.S_HIGH), (1, 1, 1, 3, 0, 6, TC.S_LOW, TC.S_HIGH), (0, 0, 1, 20, 1, 4, TC.S_LOW, TC.S_HIGH))
E2E_N = 48
E2E_S2_SCALE = (1e3, 1e5, 1e4)           # per combo of END_TO_END: the smallest power of ten that gives ratio >= 1e-5 in every draw and variant
E2E_VARIANTS = ("plain", "mu_nu", "shift")
E2E_SEED = 20263                         # of mu, nu, shift: chosen on the truth alone, |log L| >= 0.02 x the sum of its absolute terms in every draw
SCAN_ROWS = 79                           # pioran_logpdf_batch_theta with features takes at most these rows (celerite_scan.hip, mixed mode)


def continuum_combos():
    return [(m, b, i, J, 0, n, TC.S_LOW, TC.S_HIGH) for m, b, i, J, n in TC.combos()] + list(CHAINED + OTHER_GRID)


def qpo_combos():
    return [c + (TC.S_LOW, TC.S_HIGH) for c in QC.combos()] + list(N_QPO_MAX)


def combos():
    """(model, basis, integrated, J, n_qpo, number of draws, S_low, S_high)"""
    return continuum_combos() + qpo_combos()


def stored(combo):
    """whether approx_qpo_vjp_truth.npz already holds the combo's A .. D"""
    return combo[4] > 0 and combo[:6] in QC.combos() and combo[6:] == (TC.S_LOW, TC.S_HIGH)


def name(combo):
    m, b, i, J, nq, _, lo, hi = combo
    return f"m{m}_b{b}_i{i}_J{J}_q{nq}" + ("" if (lo, hi) == (TC.S_LOW, TC.S_HIGH) else f"_S{lo:g}-{hi:g}")


def widths(combo):
    """(Jc, Jt): celerite terms of the continuum, and with the features"""
    Jc = combo[3] * (1 + combo[1])
    return Jc, Jc + combo[4]


def state_rows(combo):
    """rows of the celerite state: two per SHO term and per feature, three per DRWCelerite pair"""
    return combo[3] * (2 if combo[1] == 0 else 3) + 2 * combo[4]


def forward_entry_takes(combo):
    """whether pioran_logpdf_batch_theta takes the combo's shape: any continuum; with features what the mixed mode's kernels hold"""
    return combo[4] == 0 or state_rows(combo) <= SCAN_ROWS


def draws(combo):
    """(theta [n][P], norm [n], qpo [n][n_qpo][3] or None) of a combo (what the truth file was made from)"""
    m, b, i, J, nq, n, _, _ = combo
    if nq == 0:
        return TC.draws((m, b, i, J, n)) + (None,)
    return QC.draws((m, b, i, J, nq, n))


@functools.lru_cache(maxsize=None)
def _file():
    with np.load(ROOT / "tests" / "golden" / "approx_truth.npz") as z:
        return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def truth(combo):
    """dict of a combo: theta [n][P], norm [n], qpo [n][n_qpo][3] (None without features), A, B, C, D [n][Jt], x [n][J], I [n]; read-only"""
    z, k = _file(), name(combo)
    out = {f: z[f"{k}/{f}"] for f in ("theta", "norm", "x", "I")}
    out["qpo"] = z[f"{k}/qpo"] if combo[4] else None
    src = QC.truth(combo[:6]) if stored(combo) else {f: z[f"{k}/{f}"] for f in "ABCD"}
    out.update({f: src[f] for f in "ABCD"})
    for v in out.values():
        if v is not None:
            v.setflags(write=False)
    return out


def batch(combo, B):
    """(theta [B][P], norm [B], qpo [B][n_qpo][3] or None, idx [B]): the combo's draws in turn; idx: the truth's row of every batch row"""
    t = truth(combo)
    idx = np.arange(B) % len(t["theta"])
    qp = None if t["qpo"] is None else np.ascontiguousarray(t["qpo"][idx])
    return np.ascontiguousarray(t["theta"][idx]), np.ascontiguousarray(t["norm"][idx]), qp, idx


def _rel(got, want):
    """max over the last axis of |got - want| / |want|; where want = 0 only an exact 0.0 agrees"""
    if want.shape[-1] == 0:
        return np.zeros(want.shape[:-1])
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(want != 0, np.abs(got - want) / np.abs(want), np.where(got == want, 0.0, np.inf))
    return np.where(np.isfinite(got), r, np.inf).max(axis=-1)


def deviations(combo, got, idx=None):
    """got: dict with a, b [B][Jt] and, optionally, c, d [B][Jt] (the grid's (c, d) may be given as gc, gd [Jc] instead).  Returns array -> [B]
    for the arrays `got` allows (ARRAYS)."""
    t = truth(combo)
    Jc, Jt = widths(combo)
    idx = np.arange(len(t["theta"])) if idx is None else idx
    A, Bt, C, D = (t[f][idx] for f in "ABCD")
    scale = np.abs(A).max(axis=1)
    out = {}
    for k, want in (("a", A), ("b", Bt)):
        if k in got:
            g = np.asarray(got[k])
            assert g.shape == want.shape, (name(combo), k, g.shape, want.shape)
            err = np.where(np.isfinite(g), np.abs(g - want), np.inf).max(axis=1)
            out[k] = err / scale
    for k, want in (("c", C), ("d", D)):
        if k in got:
            g = np.asarray(got[k])
            assert g.shape == want.shape, (name(combo), k, g.shape, want.shape)
            out["g" + k] = _rel(g[:, :Jc], want[:, :Jc])
            if combo[4]:
                out["q" + k] = _rel(g[:, Jc:], want[:, Jc:])
        elif "g" + k in got:
            g = np.broadcast_to(np.asarray(got["g" + k]), (len(idx), Jc))
            out["g" + k] = _rel(g, want[:, :Jc])
    return out


def structural_zeros(combo, got):
    """the entries of `got` that must be exactly 0.0: b of the DRWCelerite second half, d of its one-row terms; array -> values"""
    J, Jc = combo[3], widths(combo)[0]
    if combo[1] == 0:
        return {}
    out = {}
    if "b" in got:
        out["b"] = np.asarray(got["b"])[:, J:Jc]
    if "d" in got:
        out["d"] = np.asarray(got["d"])[:, J:Jc]
    elif "gd" in got:
        out["gd"] = np.asarray(got["gd"])[J:Jc]
    return out


def host_mirror(combo, th=None, nm=None, qp=None):
    """approx_batch / approx_batch_qpo on the combo's draws (or a batch of it): dict a, b [B][Jt], c, d [B][Jt]"""
    import pioran_jl_amd as pj
    m, b, i, J, nq, n, lo, hi = combo
    if th is None:
        t = truth(combo)
        th, nm, qp = t["theta"], t["norm"], t["qpo"]
    cls = (pj.SingleBendingPowerLaw, pj.DoubleBendingPowerLaw)[m]
    kw = dict(is_integrated_power=bool(i), basis_function=BASIS_NAME[b])
    if nq == 0:
        A, Bc, c, d = pj.approx_batch(cls, th, F_MIN, F_MAX, J, nm, lo, hi, **kw)
        ones = np.ones((len(th), 1))
        return {"a": A, "b": Bc, "c": ones * c, "d": ones * d}
    return dict(zip("abcd", pj.approx_batch_qpo(cls, th, qp, F_MIN, F_MAX, J, nm, lo, hi, **kw)))


@functools.lru_cache(maxsize=None)
def ref_dev(combo):
    """array -> the host mirror's largest deviation from the truth over the combo's own draws"""
    return {k: float(v.max()) for k, v in deviations(combo, host_mirror(combo)).items()}


def bar(combo):
    """array -> max(MARGIN x ref_dev, FLOOR)"""
    return {k: max(MARGIN * v, FLOOR) for k, v in ref_dev(combo).items()}


def check(combo, got, idx=None, leg=""):
    """`got` (as deviations() takes it) against the truth within the bar, the structural zeros exactly.  Every figure is printed before anything is
    asserted.  Returns array -> the largest deviation over the rows."""
    dev = {k: float(v.max()) for k, v in deviations(combo, got, idx).items()}
    bars, ref = bar(combo), ref_dev(combo)
    for k, v in dev.items():
        print(f"{name(combo)} {leg} {k}: deviation {v:.3e} ({v / EPS:.1f} eps)   ref_dev {ref[k]:.3e}   bar {bars[k]:.3e}   "
              f"margin {bars[k] / v if v else np.inf:.1f}x")
    zeros = structural_zeros(combo, got)
    for k, v in zeros.items():
        if v.size and not (v == 0.0).all():
            print(f"{name(combo)} {leg} {k} at structural zeros: {v[v != 0.0][:4]} (must be exactly 0.0)")
    for k, v in dev.items():
        assert v <= bars[k], (name(combo), leg, k, v, bars[k])
    for k, v in zeros.items():
        assert (v == 0.0).all(), (name(combo), leg, k, "a structurally zero entry is not exactly 0.0")
    return dev


# ---- end to end ------------------------------------------------------------------------------------------------------------------------------
def e2e_series(golden_dir, combo):
    """(t, y, sigma2) of a combo's end-to-end tests: the first E2E_N points of simu.txt, the variances scaled"""
    A = np.loadtxt(Path(golden_dir) / "simu.txt")
    return A[:E2E_N, 0], A[:E2E_N, 1], E2E_S2_SCALE[END_TO_END.index(combo)] * A[:E2E_N, 2] ** 2


def e2e_extras(combo, variant):
    """(mu, nu, shift) [n] or None each, seeded by the combo; with a shift the data set holds raw flux and mu is the mean of its logarithm"""
    n = combo[5]
    rng = np.random.default_rng([E2E_SEED, *combo[:5], E2E_VARIANTS.index(variant)])
    if variant == "plain":
        return None, None, None
    mu, nu = 4.8 + 0.1 * rng.standard_normal(n), rng.uniform(0.8, 1.5, n)
    if variant == "mu_nu":
        return mu, nu, None
    return np.log(mu), nu, rng.uniform(0.0, 0.3, n)


def e2e_draw_series(y, s2, mu, nu, shift, k):
    """what draw k is evaluated on, formed in fp64 as every fp64 reference forms it: (y - mu, nu sigma2), with a shift (log(y - shift) - mu,
    nu sigma2 / (y - shift)^2) — the likelihood of the transformed series, no Jacobian term (include/pioran_hip.h)"""
    m = 0.0 if mu is None else mu[k]
    v = 1.0 if nu is None else nu[k]
    if shift is None:
        return y - m, v * s2
    w = y - shift[k]
    return np.log(w) - m, v * s2 / w ** 2
