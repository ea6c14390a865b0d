"""Cases and bar for the reverse mode of `approx` with QPO features (approx_qpo_vjp_kernel: Context.approx_qpo_vjp,
Dataset.logpdf_theta_grad(qpo=..., approx_on="device")), shared by the CPU tests (the host twin, the numpy twin of the kernel and its seeded mistakes,
tests/test_qpo_grad_host.py) and the GPU tests (tests/test_gpu_qpo_grad.py).  A plain module, no fixtures, modelled on tests/theta_grad_cases.py.

combos()   J in {2, 3, 20} x both models x both bases x both normalisations x n_qpo in {1, 2}, four draws each, and one grid whose LU factorisation
           interchanges rows (SHO J = 48, n_qpo = 1, two draws).  F_MIN, F_MAX, S_LOW, S_HIGH are theta_grad_cases'.
draws()    theta and norm as theta_grad_cases.draws; per feature S0 ~ U(0.05, 2), f0 log-uniform in [20 f_min, f_max / 5], Q ~ U(2, 20) (as
           test_device_approx_with_qpo_features), and in the first feature Q = 0.51 in draw 0 (Delta small, b = a / Delta large), Q = 50 in draw 1,
           f0 = f_min in draw 2 (the atan2 arguments of the integral change sign at a limit), f0 = 2 f_max in draw 3 (feature outside the band).
truth()    tests/golden/approx_qpo_vjp_truth.npz (tools/make_approx_qpo_vjp_truth.py: approx with features restated in mpmath at 50 digits,
           differentiated by a complex step of 1e-30): the draws, the coefficients A, B, C, D [n][Jt] and their Jacobians dA, dB, dC, dD
           [n][Jt][P + 1 + 3 n_qpo] with the columns in the order theta, norm, then (S0, f0, Q) per feature.
batch()    B rows for a launch: the combo's draws in turn, each row with a normal cotangent (ga, gb, gc, gd) of its own.

The bar, in the natural scale of each output: S_k = sum over the four arrays and j of |cotangent_j| |Jacobian entry_jk|, and
|got_k - truth_k| <= max(MARGIN x dev, FLOOR) x S_k; where S_k = 0 the output must equal the truth exactly.  dev (ref_dev()) is the largest
deviation in the same scale of the fp64 reference that is not the code under test — approx_batch_qpo_vjp, the host complex step through numpy's
solve — from the same truth over the same cases (every combo's own draws with the cotangent of batch(combo, n)).  MARGIN = 20 and FLOOR = 256 eps
are those of tests/grad_cases.py, for the reason given there: the kernel forms the same sums in another order."""
import functools
from pathlib import Path

import numpy as np

import theta_grad_cases as TC

ROOT = Path(__file__).resolve().parents[1]
MARGIN, FLOOR = TC.MARGIN, TC.FLOOR
F_MIN, F_MAX, S_LOW, S_HIGH = TC.F_MIN, TC.F_MAX, TC.S_LOW, TC.S_HIGH
SIZES = (2, 3, 20)
LAUNCH_B = (1, 63, 64, 65, 130)          # around the 64-thread block of the kernel, and more than two blocks
BASIS_NAME = TC.BASIS_NAME
# (model, basis, J, n_qpo) of the end-to-end test against the oracle, both normalisations each: every draw of these must give a finite oracle.logl
# on the first 120 points of tests/golden/simu.txt (checked when the truth is written)
END_TO_END = ((0, 0, 3, 1), (0, 0, 20, 2), (0, 1, 3, 1))
E2E_MU, E2E_NU = 4.8, 1.1


def combos():
    """(model, basis, integrated, J, n_qpo, number of draws)"""
    out = [(m, b, i, J, nq, 4) for J in SIZES for m in (0, 1) for b in (0, 1) for i in (1, 0) for nq in (1, 2)]
    return out + [(0, 0, 1, 48, 1, 2)]


def name(combo):
    m, b, i, J, nq, _ = combo
    return f"m{m}_b{b}_i{i}_J{J}_q{nq}"


def draws(combo):
    """(theta [n][P], norm [n], qpo [n][n_qpo][3]) of a combo (what the truth file was made from)"""
    m, b, i, J, nq, n = combo
    th, norm = TC.draws((m, b, i, J, n))
    rng = np.random.default_rng([20261, m, b, i, J, nq])
    qpo = np.stack([rng.uniform(0.05, 2.0, (n, nq)), np.exp(rng.uniform(np.log(20 * F_MIN), np.log(F_MAX / 5), (n, nq))),
                    rng.uniform(2.0, 20.0, (n, nq))], axis=2)
    qpo[0, 0, 2] = 0.51
    qpo[1, 0, 2] = 50.0
    if n > 3:
        qpo[2, 0, 1] = F_MIN
        qpo[3, 0, 1] = 2 * F_MAX
    return th, norm, np.ascontiguousarray(qpo)


@functools.lru_cache(maxsize=None)
def _file():
    with np.load(ROOT / "tests" / "golden" / "approx_qpo_vjp_truth.npz") as z:
        return {k: z[k] for k in z.files}


def truth(combo):
    """dict of a combo: theta [n][P], norm [n], qpo [n][n_qpo][3], A, B, C, D [n][Jt], dA, dB, dC, dD [n][Jt][P + 1 + 3 n_qpo]"""
    z, k = _file(), name(combo)
    return {f: z[f"{k}/{f}"] for f in ("theta", "norm", "qpo", "A", "B", "C", "D", "dA", "dB", "dC", "dD")}


def batch(combo, B, zero=False):
    """(theta [B][P], norm [B], qpo [B][n_qpo][3], g = (ga, gb, gc, gd) [4][B][Jt], truth [B][K], S [B][K]), K = P + 1 + 3 n_qpo — the combo's draws
    in turn, a normal cotangent per row (zero: 0)"""
    t = truth(combo)
    idx = np.arange(B) % len(t["theta"])
    rng = np.random.default_rng([778, B, *combo[:5]])
    g = rng.standard_normal((4, B, t["dA"].shape[1]))
    if zero:
        g = np.zeros_like(g)
    jac = np.stack([t[k][idx] for k in ("dA", "dB", "dC", "dD")])            # [4][B][Jt][K]
    want = np.einsum("abj,abjk->bk", g, jac)
    S = np.einsum("abj,abjk->bk", np.abs(g), np.abs(jac))
    return (np.ascontiguousarray(t["theta"][idx]), np.ascontiguousarray(t["norm"][idx]), np.ascontiguousarray(t["qpo"][idx]), g, want, S)


def flatten(got_theta, got_norm, got_qpo):
    """the three outputs as [B][K], in the truth's column order"""
    return np.column_stack([got_theta, got_norm, np.asarray(got_qpo).reshape(len(got_norm), -1)])


def deviation(got, want, S):
    """largest |got - truth| / S over the rows and outputs (inf where S = 0 and got != truth)"""
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.max(np.where(S > 0, np.abs(got - want) / S, np.where(got == want, 0.0, np.inf))))


def host_twin(combo, th, nm, qp, g):
    """approx_batch_qpo_vjp on a batch of the combo, flattened"""
    import pioran_jl_amd as pj
    m, b, i, J, nq, _ = combo
    cls = (pj.SingleBendingPowerLaw, pj.DoubleBendingPowerLaw)[m]
    return flatten(*pj.approx_batch_qpo_vjp(cls, th, qp, F_MIN, F_MAX, J, nm, *g, S_LOW, S_HIGH, is_integrated_power=bool(i),
                                            basis_function=BASIS_NAME[b]))


@functools.lru_cache(maxsize=None)
def ref_dev():
    """dev of the bar: approx_batch_qpo_vjp against the truth, over every combo's own draws"""
    dev = 0.0
    for c in combos():
        th, nm, qp, g, want, S = batch(c, c[5])
        dev = max(dev, deviation(host_twin(c, th, nm, qp, g), want, S))
    return dev


def bar():
    return max(MARGIN * ref_dev(), FLOOR)
