"""CPU tests (-m "not gpu") of the gradient with respect to the sampled parameters: the numpy twin of approx_vjp_kernel (tools/approx_vjp_proto.py)
against the 50-digit truth within the bar of tests/theta_grad_cases.py, its seeded mistakes caught by that bar, the twin against the host chain
approx_batch_vjp, the argument checks of the two C entries without a GPU, and Dataset.logpdf_theta_grad's unchanged host path."""
import importlib.util
import sys
from pathlib import Path

import numpy as np
import pytest

import pioran_jl_amd as pj

sys.path.insert(0, str(Path(__file__).resolve().parent))
import theta_grad_cases as TC  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]
CLS = (pj.SingleBendingPowerLaw, pj.DoubleBendingPowerLaw)


def _proto():
    spec = importlib.util.spec_from_file_location("approx_vjp_proto", ROOT / "tools" / "approx_vjp_proto.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


T = _proto()


def _twin(combo, th, nm, ga, gb, mistake=None):
    m, b, i, J, _ = combo
    return T.approx_vjp(m, th, nm, ga, gb, TC.F_MIN, TC.F_MAX, J, TC.S_LOW, TC.S_HIGH, is_integrated_power=bool(i), basis=b, mistake=mistake)


def test_case_list_holds_what_it_promises():
    cs = TC.combos()
    assert {c[3] for c in cs} >= {2, 3, 20, 33} and {c[:3] for c in cs if c[3] == 33} == {(m, b, i) for m in (0, 1) for b in (0, 1) for i in (0, 1)}
    for c in cs:
        th, nm = TC.draws(c)
        t_th, t_nm, dA, dB = TC.truth(c)
        assert np.array_equal(th, t_th) and np.array_equal(nm, t_nm), TC.name(c)          # the truth file is of these draws
        assert dA.shape == (c[4], c[3] * (1 + c[1]), th.shape[1] + 1) and np.isfinite(dA).all() and np.isfinite(dB).all()
        assert th[1, 0] < 0
        if c[4] > 3:
            assert th[2, 1] == TC.F_MIN and th[3, 1] == TC.F_MAX
        if c[0] == 1:
            assert 1.0 < th[0, 3] / th[0, 1] < 1.06
    # the pivoting grids interchange rows, the others do not
    for J, b in TC.PIVOTING:
        assert T.interchanges(J, b, TC.F_MIN, TC.F_MAX, TC.S_LOW, TC.S_HIGH) > 0
        assert T.interchanges(J - 1, b, TC.F_MIN, TC.F_MAX, TC.S_LOW, TC.S_HIGH) == 0
    assert all(T.interchanges(J, b, TC.F_MIN, TC.F_MAX, TC.S_LOW, TC.S_HIGH) == 0 for J in TC.SIZES for b in (0, 1))


def test_reference_deviation_and_bar():
    dev = TC.ref_dev()
    print(f"approx_batch_vjp against the 50-digit truth: dev = {dev:.3e} S_k; bar = {TC.bar():.3e} S_k")
    assert 0.0 < dev < 1e-8          # a complex step through an fp64 solve: far from exact, far from wrong


@pytest.mark.parametrize("combo", TC.combos(), ids=TC.name)
def test_twin_against_truth(combo):
    th, nm, ga, gb, t, S = TC.batch(combo, combo[4])
    g, gn = _twin(combo, th, nm, ga, gb)
    d = TC.deviation(g, gn, t, S)
    print(f"{TC.name(combo)}: twin deviates by {d:.3e} S_k (bar {TC.bar():.3e})")
    assert d <= TC.bar()


def test_twin_zero_cotangent_is_exactly_zero():
    for combo in TC.combos():
        th, nm, ga, gb, t, S = TC.batch(combo, combo[4], zero=True)
        g, gn = _twin(combo, th, nm, ga, gb)
        assert np.all(g == 0.0) and np.all(gn == 0.0)


@pytest.mark.parametrize("mistake", T.MISTAKES)
def test_seeded_mistake_fails_the_bar(mistake):
    worst = 0.0
    for combo in TC.combos():
        th, nm, ga, gb, t, S = TC.batch(combo, combo[4])
        g, gn = _twin(combo, th, nm, ga, gb, mistake=mistake)
        worst = max(worst, TC.deviation(g, gn, t, S))
    print(f"{mistake}: worst deviation {worst:.3e} S_k (bar {TC.bar():.3e})")
    assert worst > TC.bar()


def test_twin_agrees_with_the_host_chain():
    """relative to each gradient entry's scale S_k, within twice the host chain's own deviation from the truth plus the floor"""
    for combo in TC.combos():
        m, b, i, J, n = combo
        th, nm, ga, gb, t, S = TC.batch(combo, n)
        g, gn = _twin(combo, th, nm, ga, gb)
        h, hn = pj.approx_batch_vjp(CLS[m], th, TC.F_MIN, TC.F_MAX, J, nm, ga, gb, TC.S_LOW, TC.S_HIGH, is_integrated_power=bool(i),
                                    basis_function=TC.BASIS_NAME[b])
        d = float(np.max(np.abs(np.column_stack([g - h, gn - hn])) / S))
        assert d <= 2 * TC.ref_dev() + TC.FLOOR, (TC.name(combo), d)


def test_entries_reject_null_handles_without_a_gpu():
    L = pj._lib.lib()
    z = np.zeros(8)
    p = z.ctypes.data
    assert L.pioran_logpdf_batch_theta_grad(None, 1, 0, 20, 0, 1, 1e-3, 1.0, 20.0, 20.0, p, p, None, None, None, p, None, p, p, None, None, None,
                                            None, None) == -1
    assert L.pioran_approx_vjp_batch(None, 1, 0, 20, 0, 1, 1e-3, 1.0, 20.0, 20.0, p, p, p, p, p, p) == -1
    assert L.pioran_approx_vjp_batch(None, 1, 2, 20, 0, 1, 1e-3, 1.0, 20.0, 20.0, p, p, p, p, p, p) == -1


class _StubDataset(pj.Dataset):
    """logpdf_theta_grad's host path over a recorded logl_grad: no GPU"""

    def __init__(self):
        self.calls = []

    def logl_grad(self, A, Bc, C, Dd, mu=None, nu=None, series_grad=False, shift=None, cd_grad=True):
        self.calls.append(dict(A=A, Bc=Bc, C=C, Dd=Dd, mu=mu, nu=nu, shift=shift, cd_grad=cd_grad))
        rng = np.random.default_rng(5)
        B = len(A)
        return {"logl": rng.normal(size=B), "status": np.zeros(B, np.int32), "grad_a": rng.normal(size=A.shape), "grad_b": rng.normal(size=A.shape),
                "grad_nu": rng.normal(size=B), "grad_mu": rng.normal(size=B)}

    def close(self):
        pass

    def __del__(self):
        pass


def test_host_path_is_what_it_was():
    """approx_on="host" (the default): approx_batch, the device gradient with cd_grad off, approx_batch_vjp — the same numbers, bit for bit"""
    th, nm = TC.draws((1, 1, 1, 20, 6))
    mu, nu = np.linspace(-0.1, 0.1, 6), np.linspace(0.8, 1.2, 6)
    ds = _StubDataset()
    got = ds.logpdf_theta_grad(pj.DoubleBendingPowerLaw, th, nm, TC.F_MIN, TC.F_MAX, 20, basis_function="DRWCelerite", mu=mu, nu=nu)
    same = ds.logpdf_theta_grad(pj.DoubleBendingPowerLaw, th, nm, TC.F_MIN, TC.F_MAX, 20, basis_function="DRWCelerite", mu=mu, nu=nu, approx_on="host")
    A, Bc, C, Dd = pj.approx_batch(pj.DoubleBendingPowerLaw, th, TC.F_MIN, TC.F_MAX, 20, nm, basis_function="DRWCelerite")
    call = ds.calls[0]
    assert np.array_equal(call["A"], A) and np.array_equal(call["Bc"], Bc) and np.array_equal(call["C"], C) and call["cd_grad"] is False
    g = _StubDataset().logl_grad(A, Bc, C, Dd)
    gth, gn = pj.approx_batch_vjp(pj.DoubleBendingPowerLaw, th, TC.F_MIN, TC.F_MAX, 20, nm, g["grad_a"], g["grad_b"], basis_function="DRWCelerite")
    assert sorted(got) == ["grad_mu", "grad_norm", "grad_nu", "grad_shift", "grad_theta", "logl", "status"]
    for res in (got, same):
        assert np.array_equal(res["grad_theta"], gth) and np.array_equal(res["grad_norm"], gn) and np.array_equal(res["logl"], g["logl"])
        assert np.array_equal(res["grad_nu"], g["grad_nu"]) and np.array_equal(res["grad_mu"], g["grad_mu"]) and res["grad_shift"] is None
    with pytest.raises(ValueError):
        ds.logpdf_theta_grad(pj.DoubleBendingPowerLaw, th, nm, TC.F_MIN, TC.F_MAX, 20, approx_on="elsewhere")
