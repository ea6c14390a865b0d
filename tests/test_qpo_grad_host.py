"""CPU tests (-m "not gpu") of the gradient with respect to the sampled parameters of continuum + QPO models: the host twin approx_batch_qpo[_vjp]
and the numpy twin of approx_qpo_vjp_kernel (tools/approx_qpo_vjp_proto.py) against the 50-digit truth within the bar of tests/qpo_grad_cases.py,
the proto's seeded mistakes caught by that bar, approx_batch_qpo against the oracle's and the host's approx on the reference's own cases, the argument
checks of the two C entries without a GPU, and the names of the new entries in the header, the ctypes table and the Julia wrapper."""
import ctypes
import importlib.util
import sys
from pathlib import Path

import numpy as np
import pytest

import pioran_jl_amd as pj
from oracle import oracle as O

sys.path.insert(0, str(Path(__file__).resolve().parent))
import qpo_grad_cases as QC  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]
CLS = (pj.SingleBendingPowerLaw, pj.DoubleBendingPowerLaw)


def _proto():
    sys.path.insert(0, str(ROOT / "tools"))          # the proto takes the grid, the weights and dlog_psd from tools/approx_vjp_proto.py
    spec = importlib.util.spec_from_file_location("approx_qpo_vjp_proto", ROOT / "tools" / "approx_qpo_vjp_proto.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


T = _proto()


def _twin(combo, th, nm, qp, g, mistake=None):
    m, b, i, J, nq, _ = combo
    return QC.flatten(*T.approx_qpo_vjp(m, th, nm, qp, *g, QC.F_MIN, QC.F_MAX, J, QC.S_LOW, QC.S_HIGH, is_integrated_power=bool(i), basis=b,
                                        mistake=mistake))


def test_case_list_holds_what_it_promises():
    cs = QC.combos()
    grid = {(m, b, i, J, nq) for J in (2, 3, 20) for m in (0, 1) for b in (0, 1) for i in (0, 1) for nq in (1, 2)}
    assert {c[:5] for c in cs if c[5] == 4} == grid and [c for c in cs if c[5] != 4] == [(0, 0, 1, 48, 1, 2)]
    assert all((m, b, i, J, nq, 4) in cs for m, b, J, nq in QC.END_TO_END for i in (0, 1))
    for c in cs:
        m, b, i, J, nq, n = c
        th, nm, qp = QC.draws(c)
        t = QC.truth(c)
        assert np.array_equal(th, t["theta"]) and np.array_equal(nm, t["norm"]) and np.array_equal(qp, t["qpo"]), QC.name(c)
        Jt, K = J * (1 + b) + nq, th.shape[1] + 1 + 3 * nq
        assert qp.shape == (n, nq, 3)
        for k in "ABCD":
            assert t[k].shape == (n, Jt) and t["d" + k].shape == (n, Jt, K) and np.isfinite(t[k]).all() and np.isfinite(t["d" + k]).all()
        assert qp[0, 0, 2] == 0.51 and qp[1, 0, 2] == 50.0
        if n > 3:
            assert qp[2, 0, 1] == QC.F_MIN and qp[3, 0, 1] == 2 * QC.F_MAX
        # the continuum's (c, d) are the grid's: they depend on no parameter
        assert not t["dC"][:, :Jt - nq].any() and not t["dD"][:, :Jt - nq].any()
    assert T.interchanges(48, 0, QC.F_MIN, QC.F_MAX, QC.S_LOW, QC.S_HIGH) > 0


def test_reference_deviation_and_bar():
    dev = QC.ref_dev()
    print(f"approx_batch_qpo_vjp against the 50-digit truth: dev = {dev:.3e} S_k; bar = {QC.bar():.3e} S_k")
    assert 0.0 < dev < 1e-8          # a complex step through an fp64 solve: far from exact, far from wrong


@pytest.mark.parametrize("combo", QC.combos(), ids=QC.name)
def test_twins_against_truth(combo):
    th, nm, qp, g, want, S = QC.batch(combo, combo[5])
    d_proto = QC.deviation(_twin(combo, th, nm, qp, g), want, S)
    d_host = QC.deviation(QC.host_twin(combo, th, nm, qp, g), want, S)
    print(f"{QC.name(combo)}: proto deviates by {d_proto:.3e} S_k, approx_batch_qpo_vjp by {d_host:.3e} S_k (bar {QC.bar():.3e})")
    assert d_proto <= QC.bar() and d_host <= QC.bar()


@pytest.mark.parametrize("combo", QC.combos(), ids=QC.name)
def test_host_forward_against_truth(combo):
    """approx_batch_qpo's coefficients against the 50-digit ones, relative to the largest |a| of the draw (c, d: to their own size)"""
    m, b, i, J, nq, n = combo
    t = QC.truth(combo)
    got = pj.approx_batch_qpo(CLS[m], t["theta"], t["qpo"], QC.F_MIN, QC.F_MAX, J, t["norm"], QC.S_LOW, QC.S_HIGH, is_integrated_power=bool(i),
                              basis_function=QC.BASIS_NAME[b])
    scale = np.abs(t["A"]).max(axis=1, keepdims=True)
    for k, v in zip("AB", got[:2]):
        assert np.max(np.abs(v - t[k]) / scale) < 1e-9, k
    for k, v in zip("CD", got[2:]):
        np.testing.assert_allclose(v, t[k], rtol=1e-14, atol=0, err_msg=k)


def test_proto_zero_cotangent_is_exactly_zero():
    for combo in QC.combos():
        th, nm, qp, g, want, S = QC.batch(combo, combo[5], zero=True)
        assert not _twin(combo, th, nm, qp, g).any()


@pytest.mark.parametrize("mistake", T.MISTAKES)
def test_seeded_mistake_fails_the_bar(mistake):
    worst = 0.0
    for combo in QC.combos():
        th, nm, qp, g, want, S = QC.batch(combo, combo[5])
        worst = max(worst, QC.deviation(_twin(combo, th, nm, qp, g, mistake=mistake), want, S))
    print(f"{mistake}: worst deviation {worst:.3e} S_k (bar {QC.bar():.3e})")
    assert worst > QC.bar()


# the reference's own cases, test/test_psd.jl:214-285: (alpha1, f1, alpha2), features, basis
REFERENCE_CASES = [((0.2, 1.3e-2, 3.2), [(2.0, 1.0e-2, 14.2)], "SHO"),
                   ((0.2, 1.3e-2, 3.2), [(2.0, 1.0e-2, 14.2), (4.0, 1.0e-1, 4.2)], "SHO"),
                   ((0.2, 1.3e-2, 4.2), [(1.4, 1.0e-2, 10.2)], "DRWCelerite"),
                   ((0.2, 1.3e-2, 4.2), [(1.4, 1.0e-2, 10.2), (2.4, 5.0e-2, 12.2)], "DRWCelerite")]


@pytest.mark.parametrize("integ", [False, True])
@pytest.mark.parametrize("theta,feats,basis", REFERENCE_CASES)
def test_approx_batch_qpo_on_the_reference_cases(theta, feats, basis, integ):
    f_min, f_max, J, va = 2.0e-3, 3.52e2, 25, 1.32
    got = pj.approx_batch_qpo(pj.SingleBendingPowerLaw, [theta], [feats], f_min, f_max, J, va, is_integrated_power=integ, basis_function=basis)
    assert all(v.shape == (1, J * (1 if basis == "SHO" else 2) + len(feats)) for v in got)
    ref = O.approx(lambda f: O.single_bending_power_law(f, *theta), f_min, f_max, J, va, is_integrated_power=integ, basis_function=basis,
                   qpo_features=feats)
    psd = pj.SingleBendingPowerLaw(*theta)
    for q in feats:
        psd = psd + pj.QPO(*q)
    R = pj.approx(psd, f_min, f_max, J, va, is_integrated_power=integ, basis_function=basis)
    for v, o, h in zip(got, ref, pj.celerite_coefs(R)):
        tol = 1e-14 * np.abs(o).max()
        np.testing.assert_allclose(v[0], o, rtol=1e-9, atol=tol)
        np.testing.assert_allclose(v[0], h, rtol=1e-9, atol=tol)


def test_new_entries_refuse_bad_arguments_without_a_gpu():
    L = pj._lib.lib()
    ARG, UNSUPPORTED = -1, -4
    assert L.pioran_abi_version() == 7
    x = np.ones(64)
    h = v = ctypes.c_void_p(x.ctypes.data)
    N = None
    head = lambda **k: [k.get("h", h), k.get("B", 1), k.get("model", 0), k.get("J", 20), k.get("basis", 0), 1, 1e-3, 1.0, 20.0, 20.0]  # noqa: E731
    # the stand-alone reverse mode: ctx, theta, norm, n_qpo, qpo, four cotangents, three outputs
    vjp = lambda n_qpo=1, ptrs=(v,) * 10, **k: L.pioran_approx_qpo_vjp_batch(*head(**k), ptrs[0], ptrs[1], n_qpo, *ptrs[2:])  # noqa: E731
    assert vjp(h=N) == ARG and vjp(B=0) == ARG and vjp(model=2) == ARG and vjp(basis=2) == ARG and vjp(J=1) == ARG and vjp(J=257) == ARG
    assert vjp(n_qpo=0) == ARG and vjp(n_qpo=9) == ARG
    for k in range(10):
        assert vjp(ptrs=tuple(N if j == k else v for j in range(10))) == ARG, k
    # the one-call entry: ds, theta, norm | mu, nu, shift | n_qpo | qpo, out, status | grad_theta, grad_norm, grad_qpo | grad_nu, grad_mu, grad_shift | 8
    def one(n_qpo=1, th=v, nm=v, extras=(N, N, N), qpo=v, out=v, st=v, g3=(v, v, v), gex=(N, N, N), inter=(N,) * 8, **k):
        return L.pioran_logpdf_batch_theta_qpo_grad(*head(**k), th, nm, *extras, n_qpo, qpo, out, st, *g3, *gex, *inter)
    assert one(h=N) == ARG and one(B=0) == ARG and one(model=-1) == ARG and one(basis=2) == ARG and one(J=1) == ARG
    assert one(n_qpo=0) == ARG and one(n_qpo=9) == ARG                     # n_qpo = 0 is pioran_logpdf_batch_theta_grad's
    assert one(th=N) == ARG and one(nm=N) == ARG and one(qpo=N) == ARG and one(out=N) == ARG
    for k in range(3):
        assert one(g3=tuple(N if j == k else v for j in range(3))) == ARG
        assert one(extras=tuple(v if j == k else N for j in range(3))) == ARG              # nu / mu / shift without its gradient
        assert one(gex=tuple(v if j == k else N for j in range(3))) == ARG                 # a gradient without its input
    assert one(inter=(v,) * 7 + (N,)) == ARG and one(inter=(N,) * 4 + (v,) * 4) == ARG     # the eight [B][Jt] arrays: all or none
    # more than 143 rows, before anything is dereferenced: 2 J + 2 n_qpo (SHO), 3 J + 2 n_qpo (DRWCelerite)
    assert one(J=71) == UNSUPPORTED and one(J=70, n_qpo=2) == UNSUPPORTED and one(J=48, basis=1) == UNSUPPORTED
    assert one(J=71, inter=(v,) * 8, extras=(v, v, v), gex=(v, v, v)) == UNSUPPORTED


def test_header_ctypes_table_and_julia_wrapper_name_the_new_entries():
    header = (ROOT / "include" / "pioran_hip.h").read_text()
    julia = (ROOT / "pioran.jl_amd" / "julia" / "PioranHIP.jl").read_text()
    for name in ("pioran_approx_qpo_vjp_batch", "pioran_logpdf_batch_theta_qpo_grad"):
        assert f"int {name}(" in header and name in pj._lib.SIGNATURES and f":{name}" in julia, name
        assert hasattr(pj._lib.lib(), name)
    assert "PSD features (QPO) are out of scope" not in header
    assert "ABI_VERSION = 7" in julia
    assert hasattr(pj.Context, "approx_qpo_vjp") and pj.approx_batch_qpo and pj.approx_batch_qpo_vjp


class _RecordedDataset(pj.Dataset):
    """logl_grad replaced by a recorded answer: the host path of logpdf_theta_grad(qpo=...) needs no GPU"""

    def __init__(self, N, answer):
        self.N, self.answer, self.calls = N, answer, []

    def logl_grad(self, A, Bc, C, Dd, **kw):
        self.calls.append((A, Bc, C, Dd, kw))
        return self.answer

    def close(self):
        pass

    def __del__(self):
        pass


def test_logpdf_theta_grad_host_path_with_qpo_chains_through_the_twin():
    combo = (1, 1, 1, 3, 2, 4)
    th, nm, qp, g, want, S = QC.batch(combo, 4)
    ans = {"logl": np.arange(4.0), "status": np.zeros(4, np.int32), "grad_a": g[0], "grad_b": g[1], "grad_c": g[2], "grad_d": g[3],
           "grad_nu": np.ones(4), "grad_mu": np.ones(4)}
    ds = _RecordedDataset(10, ans)
    kw = dict(basis_function="DRWCelerite", qpo=qp, return_coef_grads=True)
    res = ds.logpdf_theta_grad(CLS[1], th, nm, QC.F_MIN, QC.F_MAX, 3, QC.S_LOW, QC.S_HIGH, nu=np.ones(4), **kw)
    A, Bc, C, Dd, opts = ds.calls[0]
    assert A.shape == C.shape == (4, 8) and opts["cd_grad"] is True and opts["shift"] is None
    assert res["grad_mu"] is None and res["grad_shift"] is None and res["grad_nu"] is ans["grad_nu"] and res["grad_qpo"].shape == (4, 2, 3)
    assert QC.deviation(QC.flatten(res["grad_theta"], res["grad_norm"], res["grad_qpo"]), want, S) <= QC.bar()
    for k, v in zip(("coef_a", "coef_b", "coef_c", "coef_d"), (A, Bc, C, Dd)):
        assert res[k] is v
    # without qpo nothing changes, the keys included
    plain = _RecordedDataset(10, {**ans, "grad_a": g[0][:, :6], "grad_b": g[1][:, :6]})
    assert set(plain.logpdf_theta_grad(CLS[1], th, nm, QC.F_MIN, QC.F_MAX, 3, basis_function="DRWCelerite")) == \
        {"logl", "status", "grad_theta", "grad_norm", "grad_nu", "grad_mu", "grad_shift"}
    with pytest.raises(ValueError, match="approx_on"):
        ds.logpdf_theta_grad(CLS[1], th, nm, QC.F_MIN, QC.F_MAX, 3, approx_on="elsewhere", **kw)
