"""Posterior mean of a celerite GP at new times from a KNOWN z = K^-1 (y - mu): numpy twin, in fp64, of the windowed mean path as its
kernels index it (pioran_launch_predict_from_gy in pioran.jl_amd/csrc/celerite_predict.hip).

    mu(tau) = sum_n z_n k(|tau - t_n|)
            = sum_r Qf_{n0-1}[r] e^{-c_r (tau - t_{n0-1})} U~_r(tau)  +  sum_r Qb_{n0}[r] e^{-c_r (t_{n0} - tau)} V_r(tau),   n0 = #{t_n < tau}
    Qf_n = phi_n o Qf_{n-1} + z_n V_n            Qb_n = z_n U~_n + phi_{n+1} o Qb_{n+1}

Rows r: a cos and a sin row per term (the sin row dropped where d_j = 0).  The steps follow the kernels one for one:

  pass 0        q_segment_kernel<0>: every segment of QSEG steps from a zero carry -> its sum E_s and the product P_s of its phis; the backward
                direction links step n to n + 1 with the phi of step n + 1, at a segment's upper edge the phi of the next segment's first step
  carries       q_carry_kernel: C_0 = 0, C_{s+1} = E_s + P_s C_s; backward the same from the last segment down
  tau factors   predict_tau_kernel: n0 and Wc = ef cos(d tau), Ws = ef sin(d tau), Wv = eb V(tau); ef / eb zero on a side without data
  fused         q_eval_fused_kernel (tau ascending and M <= N R): the segment walked again from its carry, the evaluation times of a step found by
                the three searches lower(n_lo + 1), lower(n_hi + 1), lower(n_hi) - 1 and the walking pointers mp / nn; the two parts start at
                zero (predict_part_init_kernel) and are added at the end (predict_part_sum_kernel)
  two passes    q_segment_kernel<1> stores Qf, Qb [N][R]; predict_eval16_kernel reads the rows n0 - 1 and n0 CLAMPED into 0 .. N - 1

predict_mean(a, b, c, d, t, z, tau) -> (M,); tau in any order (the switch between the two evaluations is the host entry's).  It takes z as
given: tests/predict_mean_cases.py feeds it an fp64 dense solve.

`mistake` seeds one of the slips this index logic can make (MISTAKES); tests/test_predict_mean_sim_host.py uses them to show that the case list
of tests/predict_mean_cases.py catches each of them.
"""
from __future__ import annotations

import numpy as np

QSEG = 128

MISTAKES = {
    "carry_drops_product": "C_{s+1} = E_s: the carry into a segment forgets what came in before the previous one",
    "no_backward_link": "phn = 0 at every segment's upper edge: the backward recurrence restarts in every segment",
    "fused_misses_segment_end": "m_hi = lower(n_hi): the fused forward walk leaves out the times that wait for a segment's last step",
    "clamped_row_weighted": "ef / eb not zeroed where n0 = 0 / n0 = N: the clamped Qf / Qb row of the two-pass evaluation gets a weight",
    "sin_row_sign": "be = +b on a sin row of the backward U~",
}


def _rows(a, b, c, d):
    """(term, sin_row) per row"""
    term, ks = [], []
    for j in range(len(a)):
        term.append(j); ks.append(False)
        if d[j] != 0.0:
            term.append(j); ks.append(True)
    return np.array(term), np.array(ks)


def predict_mean(a, b, c, d, t, z, tau, mistake=None, path=None):
    """path: None (the entry's switch), "fused" (tau must ascend) or "two_pass"."""
    assert mistake is None or mistake in MISTAKES, mistake
    a, b, c, d, t, z, tau = (np.asarray(v, dtype=np.float64).reshape(-1) for v in (a, b, c, d, t, z, tau))
    N, M = len(t), len(tau)
    term, ks = _rows(a, b, c, d)
    R = len(term)
    ar, br, cr, dr = a[term], b[term], c[term], d[term]
    nseg = (N + QSEG - 1) // QSEG

    # step(n): (v, x, phi) of every row; phi_0 = 0
    co, si = np.cos(dr * t[:, None]), np.sin(dr * t[:, None])
    V = np.where(ks, si, co); X = np.where(ks, co, si)
    PH = np.zeros((N, R))
    PH[1:] = np.exp(-cr * np.diff(t)[:, None])
    al_b = ar                                              # backward U~_n = al v + be x
    be_b = np.where(ks, br if mistake == "sin_row_sign" else -br, br)
    U = al_b * V + be_b * X

    def bounds(s):
        return s * QSEG, min(s * QSEG + QSEG, N)

    def upper_link(n_hi):
        if n_hi < N and mistake != "no_backward_link":
            return PH[n_hi]
        return np.zeros(R)

    # ---- pass 0 ----
    E = np.zeros((2, nseg, R)); P = np.ones((2, nseg, R))
    for s in range(nseg):
        n_lo, n_hi = bounds(s)
        q = np.zeros(R); prod = np.ones(R)
        for n in range(n_lo, n_hi):
            q = z[n] * V[n] + PH[n] * q
            prod = prod * PH[n]
        E[0, s], P[0, s] = q, prod
        q = np.zeros(R); prod = np.ones(R)
        phn = upper_link(n_hi)
        for n in range(n_hi - 1, n_lo - 1, -1):
            ph, phn = phn, PH[n]
            q = z[n] * U[n] + ph * q
            prod = prod * ph
        E[1, s], P[1, s] = q, prod
    # ---- carries ----
    Cin = np.zeros((2, nseg, R))
    for dirn in (0, 1):
        cst = np.zeros(R)
        for k in range(nseg):
            s = k if dirn == 0 else nseg - 1 - k
            Cin[dirn, s] = cst
            cst = E[dirn, s] if mistake == "carry_drops_product" else P[dirn, s] * cst + E[dirn, s]
    # ---- tau-only factors ----
    n0s = np.searchsorted(t, tau, side="left")                # number of t_n < tau
    lo_ok, hi_ok = n0s > 0, n0s < N
    dtf = np.where(lo_ok, tau - t[np.maximum(n0s - 1, 0)], 0.0)
    dtb = np.where(hi_ok, t[np.minimum(n0s, N - 1)] - tau, 0.0)
    ef = np.exp(-cr * dtf[:, None]); eb = np.exp(-cr * dtb[:, None])
    if mistake != "clamped_row_weighted":
        ef = np.where(lo_ok[:, None], ef, 0.0); eb = np.where(hi_ok[:, None], eb, 0.0)
    ct, st = np.cos(dr * tau[:, None]), np.sin(dr * tau[:, None])
    Wc, Ws, Wv = ef * ct, ef * st, eb * np.where(ks, st, ct)
    ae = np.where(ks, -br, ar); bee = np.where(ks, ar, br)   # forward U~_r(tau) = ae cos + bee sin

    tau_sorted = bool(np.all(tau[1:] >= tau[:-1]))
    if path is None:
        path = "fused" if (M > 0 and tau_sorted and M <= N * R) else "two_pass"
    if path == "fused":
        assert tau_sorted
        lower = lambda key: int(np.searchsorted(n0s, key, side="left"))      # first m with n0s[m] >= key
        part = np.zeros((2, M))
        for s in range(nseg):
            n_lo, n_hi = bounds(s)
            # forward: evaluation times with n0 - 1 in [n_lo, n_hi)
            q = Cin[0, s].copy()
            mp = lower(n_lo + 1)
            m_hi = lower(n_hi) if mistake == "fused_misses_segment_end" else lower(n_hi + 1)
            nn = n0s[mp] - 1 if mp < m_hi else N
            for n in range(n_lo, n_hi):
                q = z[n] * V[n] + PH[n] * q
                while nn == n:
                    part[0, mp] = np.sum(q * (ae * Wc[mp] + bee * Ws[mp]))
                    mp += 1
                    nn = n0s[mp] - 1 if mp < m_hi else N
            # backward: evaluation times with n0 in [n_lo, n_hi)
            q = Cin[1, s].copy()
            m_lo = lower(n_lo)
            mp = lower(n_hi) - 1
            nn = n0s[mp] if mp >= m_lo else -1
            phn = upper_link(n_hi)
            for n in range(n_hi - 1, n_lo - 1, -1):
                ph, phn = phn, PH[n]
                q = z[n] * U[n] + ph * q
                while nn == n:
                    part[1, mp] = np.sum(q * Wv[mp])
                    mp -= 1
                    nn = n0s[mp] if mp >= m_lo else -1
        return part[0] + part[1]
    assert path == "two_pass", path
    Qf = np.empty((N, R)); Qb = np.empty((N, R))
    for s in range(nseg):
        n_lo, n_hi = bounds(s)
        q = Cin[0, s].copy()
        for n in range(n_lo, n_hi):
            q = z[n] * V[n] + PH[n] * q
            Qf[n] = q
        q = Cin[1, s].copy()
        phn = upper_link(n_hi)
        for n in range(n_hi - 1, n_lo - 1, -1):
            ph, phn = phn, PH[n]
            q = z[n] * U[n] + ph * q
            Qb[n] = q
    qf = Qf[np.maximum(n0s - 1, 0)]                          # clamped rows: their weight is zero
    qb = Qb[np.minimum(n0s, N - 1)]
    return np.sum(qf * (ae * Wc + bee * Ws) + qb * Wv, axis=1)


if __name__ == "__main__":
    import sys
    from pathlib import Path
    sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
    from oracle import oracle
    t, y, yerr = oracle.synthetic_series(400)
    A, Bc, C, Dd, mu, nu = oracle.theta_to_coefs(oracle.synthetic_theta(3, t, y), t)
    rng = np.random.default_rng(0)
    tau = np.sort(np.concatenate([rng.uniform(t[0] - 5, t[-1] + 5, 150), t[::40]]))
    for bb in range(3):
        dt = np.abs(t[:, None] - t[None, :])[..., None]
        K = (np.exp(-C * dt) * (A[bb] * np.cos(Dd * dt) + Bc[bb] * np.sin(Dd * dt))).sum(-1) + np.diag(nu[bb] * yerr ** 2)
        z = np.linalg.solve(K, y - mu[bb])
        ds = np.abs(tau[:, None] - t[None, :])[..., None]
        ref = (np.exp(-C * ds) * (A[bb] * np.cos(Dd * ds) + Bc[bb] * np.sin(Dd * ds))).sum(-1) @ z          # the dense product with the same z
        for path in ("fused", "two_pass"):
            got = predict_mean(A[bb], Bc[bb], C, Dd, t, z, tau, path=path)
            print(f"draw {bb} {path}: max |delta| / max |y - mu| = {np.abs(got - ref).max() / np.abs(y - mu[bb]).max():.2e}")
