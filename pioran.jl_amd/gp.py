"""GP facade + solver entry points of the hot path, host side (Python over the C ABI).

Mirrors, with the same names and argument meaning:
  ScalableGP(mu, kernel[, solver]) / f(t, sigma2) / logpdf(fx, y)   src/scalable_GP.jl:24-42,162-166
  log_likelihood(cov, tau, y, sigma2; solver)                       src/celerite_solver.jl:262-294
  logl(a, b, c, d, tau, y, sigma2)                                  src/celerite_solver.jl:312-334
  log_likelihood_direct(cov, t, y, sigma2)  (returns +NLL)          src/direct_solver.jl:6-21
plus the batched entry the reference lacks: logpdf_batch / Dataset.logl_batch.

Everything numerical happens in libpioran_hip.so on the GPU.  No CPU fallback.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from .kernels import SemiSeparable, SumOfCelerite

_SOLVERS = ("celerite", "celerite_matrix")
PPC_QUANTILES = (0.025, 0.16, 0.5, 0.84, 0.975)   # what the reference's predictive checks plot (src/plots_diagnostics.jl:805-816)


def _f64(x):
    return np.ascontiguousarray(x, dtype=np.float64)


def _ptr(x):
    return None if x is None else ctypes.c_void_p(x.ctypes.data)


def _theta_args(model, theta, norm, basis_function):
    """(model id, basis id, theta (B, P), norm (B,)) of the entries that run `approx` on the device."""
    from .psd import DoubleBendingPowerLaw, SingleBendingPowerLaw
    mid = {SingleBendingPowerLaw: 0, DoubleBendingPowerLaw: 1}.get(model)
    if mid is None:
        raise ValueError("model must be SingleBendingPowerLaw or DoubleBendingPowerLaw")
    if basis_function not in ("SHO", "DRWCelerite"):
        raise ValueError("Basis function" + basis_function + "not implemented")
    theta = _f64(np.atleast_2d(theta))
    if theta.shape[1] != (3 if mid == 0 else 5):
        raise ValueError("theta has the wrong number of columns for this model")
    return mid, 0 if basis_function == "SHO" else 1, theta, _f64(np.broadcast_to(norm, (theta.shape[0],)))


def _carma_args(p, q, qa, qb, norm, r_alpha, beta):
    """(p, q, form, in1, in2, norm (B,)) of the CARMA entries: form 0 with qa (B, p), qb (B, q) (None for q = 0), or form 1 with the roots as
    (B, p, 2) = (re, im) and beta (B, q + 1)."""
    p, q = int(p), int(q)
    if r_alpha is None:
        if qa is None:
            raise ValueError("give the quadratic factors (qa, qb) or the roots and coefficients (r_alpha, beta)")
        in1 = _f64(np.atleast_2d(qa))
        B = in1.shape[0]
        in2 = np.zeros((B, 0)) if qb is None else _f64(np.asarray(qb, dtype=np.float64).reshape(B, -1))
        if in1.shape[1] != p or in2.shape[1] != q:
            raise ValueError("qa must be (B, p) and qb (B, q)")
        form, in2 = 0, (in2 if q else None)
    else:
        r = np.atleast_2d(np.asarray(r_alpha, dtype=complex))
        B = r.shape[0]
        in2 = _f64(np.atleast_2d(beta))
        if r.shape[1] != p:
            raise ValueError("The length of the roots of the autoregressive polynomial must be equal to the order of the autoregressive polynomial")
        if in2.shape != (B, q + 1):
            raise ValueError("The length of the moving average coefficients must be equal to q + 1")
        form, in1 = 1, _f64(np.stack([r.real, r.imag], axis=-1))
    return p, q, form, in1, in2, _f64(np.broadcast_to(norm, (B,)))


class Context:
    """One GPU + one HIP stream (pioran_ctx).  One per host thread / rank."""

    def __init__(self, device: int = 0, stream: int | None = None):
        L = _lib.lib()
        h = ctypes.c_void_p()
        if stream is None:
            _lib.check(L.pioran_ctx_create(int(device), ctypes.byref(h)))
        else:
            _lib.check(L.pioran_ctx_create_on_stream(int(device), ctypes.c_void_p(stream), ctypes.byref(h)))
        self._h = h
        self.device = int(device)

    def close(self):
        if self._h:
            _lib.lib().pioran_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def synchronize(self):
        _lib.check(_lib.lib().pioran_ctx_synchronize(self._h), self._h)

    def trim(self):
        """Release the context's scratch buffers (gradient / prediction workspaces, staging, the dense slab)."""
        _lib.check(_lib.lib().pioran_ctx_trim(self._h), self._h)

    def set_option(self, key: str, value=None):
        """Diagnostic switch of this context (pioran_ctx_set_option): "scan_config" (a configuration name, "wide", "block" or
        None), "no_wide" / "no_block" / "no_paired" / "no_mixed" / "force_fallback" / "win2" / "no_win2" (truthy = on).
        Tests and tuning tools only."""
        if value is None or value is False:
            v = None
        elif value is True:
            v = b"1"
        else:
            v = str(value).encode()
        _lib.check(_lib.lib().pioran_ctx_set_option(self._h, key.encode(), v), self._h)

    def event_record(self, slot: int):
        _lib.check(_lib.lib().pioran_ctx_event_record(self._h, slot), self._h)

    def fp64_probe(self, waves_per_simd: int = 2, ms: float = 10.0) -> float:
        """The FP64 FMA rate (TFLOP/s) this device sustains now at `waves_per_simd` wavefronts per SIMD (pioran_ctx_fp64_probe)."""
        out = ctypes.c_double()
        _lib.check(_lib.lib().pioran_ctx_fp64_probe(self._h, int(waves_per_simd), float(ms), ctypes.byref(out)), self._h)
        return out.value

    def event_elapsed_ms(self, a: int, b: int) -> float:
        ms = ctypes.c_float()
        _lib.check(_lib.lib().pioran_ctx_event_elapsed_ms(self._h, a, b, ctypes.byref(ms)), self._h)
        return ms.value

    # -- scalar drop-ins ---------------------------------------------------------------------
    def logl(self, a, b, c, d, tau, y, sigma2, return_status=False):
        a, b, c, d, tau, y, sigma2 = map(_f64, (a, b, c, d, tau, y, sigma2))
        if not (len(a) == len(b) == len(c) == len(d)) or not (len(tau) == len(y) == len(sigma2)):
            raise ValueError("inconsistent lengths")
        out = ctypes.c_double()
        st = ctypes.c_int32()
        _lib.check(_lib.lib().pioran_celerite_logl(self._h, len(tau), len(a), _ptr(a), _ptr(b), _ptr(c), _ptr(d),
                                                   _ptr(tau), _ptr(y), _ptr(sigma2), ctypes.byref(out),
                                                   ctypes.byref(st)), self._h)
        return (out.value, st.value) if return_status else out.value

    def simulate(self, A, Bc, C, Dd, t, sigma2, q):
        """GP realisations from standard-normal draws q (B, N): sim of src/celerite_solver.jl:515-549 for B coefficient
        sets (A, Bc: (B, J)) sharing (C, Dd: (J,)) or with (C, Dd: (B, J)) of their own.  sigma2 may be zero (pj.rand at new times).
        Error, measured against a long-double dense truth C q, C the Cholesky factor of K (docs/EXPERIMENTS.md section 24), in units of
        max |y|: <= 8.0e-15 at every edge shape (R 1..143, N 1..257, sigma2 as given, x 1e-6 and 0) on the windowed and the step-by-step
        kernels alike, 1.4e-13 on the worst of 40 random shapes (N = 256, sigma2 / k(0) down to 1.5e-8) where the fp64 references deviate by the same
        1.4e-13.  Returns (B, N)."""
        A, Bc, C, Dd, t, sigma2, q = map(_f64, (A, Bc, C, Dd, t, sigma2, q))
        if A.ndim != 2 or A.shape != Bc.shape or C.shape not in ((A.shape[1],), A.shape) or Dd.shape != C.shape:
            raise ValueError("A, Bc must be (B, J) and C, Dd (J,) or (B, J)")
        B, J = A.shape
        N = len(t)
        if sigma2.shape != (N,) or q.shape != (B, N):
            raise ValueError("sigma2 must be (N,) and q (B, N)")
        out = np.empty((B, N))
        _lib.check(_lib.lib().pioran_celerite_simulate(self._h, N, B, J, _ptr(A), _ptr(Bc), _ptr(C), _ptr(Dd), int(C.ndim == 1), _ptr(t),
                                                       _ptr(sigma2), _ptr(q), _ptr(out)), self._h)
        return out

    def approx_vjp(self, model, theta, norm, grad_a, grad_b, f_min, f_max, n_components=20, S_low=20.0, S_high=20.0, *,
                   is_integrated_power=True, basis_function="SHO"):
        """Chain rule through `approx` on the device (pioran_approx_vjp_batch): dL/da, dL/db (B, J) -> dL/dtheta (B, P), dL/dnorm (B,).
        model, theta, norm and the keywords as in Dataset.logpdf_theta; J = n_components ("SHO") or 2 n_components ("DRWCelerite")."""
        mid, basis, theta, norm = _theta_args(model, theta, norm, basis_function)
        B, P = theta.shape
        grad_a, grad_b = _f64(grad_a), _f64(grad_b)
        if grad_a.shape != (B, n_components * (1 + basis)) or grad_b.shape != grad_a.shape:
            raise ValueError("grad_a, grad_b must be (B, J)")
        gth, gnorm = np.empty((B, P)), np.empty(B)
        _lib.check(_lib.lib().pioran_approx_vjp_batch(self._h, B, mid, int(n_components), basis, int(bool(is_integrated_power)), float(f_min),
                                                      float(f_max), float(S_low), float(S_high), _ptr(theta), _ptr(norm), _ptr(grad_a),
                                                      _ptr(grad_b), _ptr(gth), _ptr(gnorm)), self._h)
        return gth, gnorm

    def approx_qpo_vjp(self, model, theta, norm, qpo, grad_a, grad_b, grad_c, grad_d, f_min, f_max, n_components=20, S_low=20.0, S_high=20.0, *,
                       is_integrated_power=True, basis_function="SHO"):
        """Chain rule through `approx` with QPO features on the device (pioran_approx_qpo_vjp_batch): dL/da, dL/db, dL/dc, dL/dd (B, Jt),
        Jt = J + n_qpo -> dL/dtheta (B, P), dL/dnorm (B,), dL/dqpo (B, n_qpo, 3) = d/d(S0, f0, Q).  qpo: (B, n_qpo, 3) or (B, 3), 1 <= n_qpo <= 8;
        of grad_c, grad_d only the feature columns are read (the continuum's c, d are the grid's).  The rest as in approx_vjp."""
        mid, basis, theta, norm = _theta_args(model, theta, norm, basis_function)
        B, P = theta.shape
        qpo = _f64(np.asarray(qpo, dtype=np.float64).reshape(B, -1, 3))
        n_qpo = qpo.shape[1]
        g = [_f64(v) for v in (grad_a, grad_b, grad_c, grad_d)]
        if any(v.shape != (B, n_components * (1 + basis) + n_qpo) for v in g):
            raise ValueError("grad_a, grad_b, grad_c, grad_d must be (B, J + n_qpo)")
        gth, gnorm, gq = np.empty((B, P)), np.empty(B), np.empty((B, n_qpo, 3))
        _lib.check(_lib.lib().pioran_approx_qpo_vjp_batch(self._h, B, mid, int(n_components), basis, int(bool(is_integrated_power)), float(f_min),
                                                          float(f_max), float(S_low), float(S_high), _ptr(theta), _ptr(norm), n_qpo, _ptr(qpo),
                                                          *map(_ptr, g), _ptr(gth), _ptr(gnorm), _ptr(gq)), self._h)
        return gth, gnorm, gq

    # -- batched Lomb-Scargle periodogram ------------------------------------------------------
    def lombscargle(self, t, Y, yerr, freq, fit_mean=True, center_data=True, return_status=False):
        """Generalised Lomb-Scargle power (standard normalisation) of the B series Y (B, N) sampled at t (N,) at the frequencies freq (F,)
        in cycles per unit time, weights yerr^-2 (None: equal weights): pioran_lombscargle_batch.  Returns (B, F) [, status (B,)]:
        status 2 and a NaN row for a series that is constant or holds a non-finite value."""
        t, Y, freq = _f64(t), _f64(Y), _f64(freq)
        yerr = None if yerr is None else _f64(yerr)
        if t.ndim != 1 or Y.ndim != 2 or Y.shape[1] != len(t) or freq.ndim != 1 or (yerr is not None and yerr.shape != t.shape):
            raise ValueError("t, yerr must be (N,), Y (B, N) and freq (F,)")
        B, N = Y.shape
        F = len(freq)
        power = np.empty((B, F))
        st = np.zeros(B, dtype=np.int32)
        _lib.check(_lib.lib().pioran_lombscargle_batch(self._h, N, B, F, _ptr(t), _ptr(Y), _ptr(yerr), _ptr(freq), int(bool(fit_mean)),
                                                       int(bool(center_data)), _ptr(power), _ptr(st)), self._h)
        return (power, st) if return_status else power

    def lombscargle_dev(self, N, B, F, dt, dY, dyerr=0, dfreq=0, fit_mean=True, center_data=True, dpower=0, dstatus=0):
        """Device-pointer (int addresses) asynchronous variant: dt, dyerr (N,), dY (B, N), dfreq (F,), dpower (B, F), dstatus (B,) int32 in
        HBM; enqueues on the context's stream (pioran_lombscargle_batch_dev).  dyerr, dstatus may be 0."""
        v = ctypes.c_void_p
        _lib.check(_lib.lib().pioran_lombscargle_batch_dev(self._h, int(N), int(B), int(F), v(dt), v(dY), v(dyerr or None), v(dfreq),
                                                           int(bool(fit_mean)), int(bool(center_data)), v(dpower), v(dstatus or None)), self._h)

    # -- quantiles and means over the draw axis ------------------------------------------------
    def quantiles(self, X, probs, status=None, shift=None, cols=None, ref=None, scale=None):
        """Quantiles (Statistics.quantile's default, type 7; the definition is tools/quantiles_proto.py) and mean of every column of X (B, M)
        over its rows, one draw per row: pioran_quantiles_batch.  status (B,) int32: rows with a non-zero entry are left out; shift (B,): the
        values are exp(X + shift_b); cols (Mc,) int: the columns to reduce, any order, repeats allowed; ref, scale (Mc,): the values are
        (ref - v) / scale.  Returns (quant (Q, Mc), mean (Mc,), kept): kept = the number of rows that entered.  At most 4096 rows."""
        probs = _f64(probs).reshape(-1)
        X = np.asarray(X, dtype=np.float64)
        if X.ndim != 2:
            raise ValueError("X must be (B, M): one draw per row")
        B, M = X.shape
        # a view of the leading columns of a wider row-major array goes as it is (ldx = its row stride), anything else as a contiguous copy
        if not (B > 0 and M > 0 and X.strides[1] == 8 and X.strides[0] % 8 == 0 and X.strides[0] >= 8 * M):
            X = np.ascontiguousarray(X)
        ldx = X.strides[0] // 8 if B > 0 and M > 0 else M
        status = None if status is None else np.ascontiguousarray(status, dtype=np.int32)
        shift = None if shift is None else _f64(np.broadcast_to(shift, (B,)))
        cols = None if cols is None else np.ascontiguousarray(cols, dtype=np.int32).reshape(-1)
        Mc = M if cols is None else len(cols)
        if (ref is None) != (scale is None):
            raise ValueError("ref and scale come together")
        ref, scale = (None, None) if ref is None else (_f64(ref).reshape(-1), _f64(scale).reshape(-1))
        if (status is not None and status.shape != (B,)) or (ref is not None and (ref.shape != (Mc,) or scale.shape != (Mc,))):
            raise ValueError("status must be (B,) and ref, scale (Mc,)")
        quant = np.empty((len(probs), Mc))
        mean = np.empty(Mc)
        kept = ctypes.c_int32(-1)
        _lib.check(_lib.lib().pioran_quantiles_batch(self._h, B, M, ldx, _ptr(X), _ptr(status), _ptr(shift), Mc, _ptr(cols), _ptr(ref), _ptr(scale),
                                                     len(probs), _ptr(probs), _ptr(quant), _ptr(mean), ctypes.cast(ctypes.byref(kept), ctypes.c_void_p)),
                   self._h)
        return quant, mean, kept.value

    def quantiles_dev(self, B, M, ldx, dX, probs, dstatus=0, dshift=0, Mc=0, dcols=0, dref=0, dscale=0, dquant=0, dmean=0, dkept=0):
        """Device-pointer (int addresses) asynchronous variant: dX (B, ldx) with the draws in its first M columns, dstatus (B,) int32, dshift (B,),
        dcols (Mc,) int32, dref, dscale (Mc,), dquant (Q, Mc), dmean (Mc,), dkept one int32 in HBM; probs on the host (copied); enqueues on the
        context's stream (pioran_quantiles_batch_dev).  dstatus, dshift, dcols (then all M columns), dref / dscale, dmean, dkept may be 0."""
        v = ctypes.c_void_p
        probs = _f64(probs).reshape(-1)
        _lib.check(_lib.lib().pioran_quantiles_batch_dev(self._h, int(B), int(M), int(ldx), v(dX), v(dstatus or None), v(dshift or None), int(Mc),
                                                         v(dcols or None), v(dref or None), v(dscale or None), len(probs), _ptr(probs), v(dquant),
                                                         v(dmean or None), v(dkept or None)), self._h)

    # -- the PSD model against its basis-function approximation ------------------------------------
    def _psd_check_args(self, model, theta, norm, freq, basis_function):
        mid, basis, theta, norm = _theta_args(model, theta, norm, basis_function)
        freq = _f64(freq).reshape(-1)
        if len(freq) < 1:
            raise ValueError("freq must hold at least one frequency")
        return mid, basis, theta, norm, freq

    def psd_check(self, model, theta, norm, freq, f_min, f_max, n_components=20, S_low=20.0, S_high=20.0, *, basis_function="SHO",
                  is_integrated_power=True, normalise=False, times_f=False, outputs=("psd", "psd_approx", "residuals", "ratios"),
                  amplitudes=False, integ=False):
        """The PSD model and its basis-function approximation for the B draws theta (B, P), norm (B,) at the frequencies freq (F,):
        pioran_psd_check_batch, the arrays of sample_approx_model (src/plots_diagnostics.jl:195-213) with one draw per ROW.  model, theta, norm
        and the grid arguments as in Dataset.logpdf_theta.  normalise: divide both spectra by get_norm_psd as plot_psd_ppc does (:404-409);
        times_f: multiply them by the frequency after that (plot_f_P).  outputs: which of "psd", "psd_approx", "residuals", "ratios" to compute
        and return, (B, F) each; amplitudes / integ: also the amplitudes (B, J) before any scaling and the normalising integral (B,).
        Returns a dict of the requested arrays and "status" (B,): 2, with NaN in the draw's rows, for a draw that cannot be evaluated.
        The call goes chunk by chunk under the context's "workspace_limit_mb"; no limit on B or F."""
        mid, basis, theta, norm, freq = self._psd_check_args(model, theta, norm, freq, basis_function)
        names = ("psd", "psd_approx", "residuals", "ratios")
        if any(o not in names for o in outputs):
            raise ValueError(f"outputs must be among {names}")
        B, F, J = theta.shape[0], len(freq), int(n_components)
        out = {n: np.empty((B, F)) for n in names if n in outputs}
        if amplitudes:
            out["amplitudes"] = np.empty((B, J))
        if integ:
            out["integ"] = np.empty(B)
        out["status"] = np.zeros(B, dtype=np.int32)
        _lib.check(_lib.lib().pioran_psd_check_batch(self._h, B, mid, J, basis, int(bool(is_integrated_power)), float(f_min), float(f_max), float(S_low),
                                                     float(S_high), _ptr(theta), _ptr(norm), F, _ptr(freq), int(bool(normalise)), int(bool(times_f)),
                                                     *(_ptr(out.get(n)) for n in names), _ptr(out.get("amplitudes")), _ptr(out.get("integ")),
                                                     _ptr(out["status"])), self._h)
        return out

    def psd_check_dev(self, B, F, model, dtheta, dnorm, dfreq, f_min, f_max, n_components=20, S_low=20.0, S_high=20.0, *, basis_function="SHO",
                      is_integrated_power=True, normalise=False, times_f=False, dpsd=0, dpsd_approx=0, dresiduals=0, dratios=0, damplitudes=0,
                      dinteg=0, dstatus=0):
        """Device-pointer (int addresses) asynchronous variant: dtheta (B, P), dnorm (B,), dfreq (F,), the outputs (B, F), damplitudes (B, J),
        dinteg (B,), dstatus (B,) int32 in HBM; enqueues on the context's stream (pioran_psd_check_batch_dev).  Any output may be 0, not all."""
        from .psd import DoubleBendingPowerLaw, SingleBendingPowerLaw
        mid = {SingleBendingPowerLaw: 0, DoubleBendingPowerLaw: 1}.get(model)
        if mid is None or basis_function not in ("SHO", "DRWCelerite"):
            raise ValueError("model must be SingleBendingPowerLaw or DoubleBendingPowerLaw and basis_function SHO or DRWCelerite")
        v = ctypes.c_void_p
        _lib.check(_lib.lib().pioran_psd_check_batch_dev(self._h, int(B), mid, int(n_components), 0 if basis_function == "SHO" else 1,
                                                         int(bool(is_integrated_power)), float(f_min), float(f_max), float(S_low), float(S_high),
                                                         v(dtheta), v(dnorm), int(F), v(dfreq), int(bool(normalise)), int(bool(times_f)),
                                                         v(dpsd or None), v(dpsd_approx or None), v(dresiduals or None), v(dratios or None),
                                                         v(damplitudes or None), v(dinteg or None), v(dstatus or None)), self._h)

    def psd_check_summary(self, model, theta, norm, freq, f_min, f_max, n_components=20, S_low=20.0, S_high=20.0, *, basis_function="SHO",
                          is_integrated_power=True, normalise=False, times_f=False, probs=PPC_QUANTILES, mean=True, meta=True):
        """Context.psd_check with its arrays kept on the device and reduced there (pioran_psd_check_summary).  Returns a dict with
        quant (4, Q, F) and mean (4, F): per frequency, over the draws with status 0, of psd, psd_approx, residuals, ratios in this order;
        meta (B, 8): per draw, over the frequencies, mean, median, min |.|, max |.| of the residuals, then of the ratios (NaN for a draw with
        status 2); status (B,) and kept.  At most 4096 draws and 4096 frequencies (the quantile kernel's limit)."""
        mid, basis, theta, norm, freq = self._psd_check_args(model, theta, norm, freq, basis_function)
        probs = _f64(probs).reshape(-1)
        B, F, Q = theta.shape[0], len(freq), len(probs)
        out = dict(quant=np.empty((4, Q, F)), status=np.zeros(B, dtype=np.int32))
        if mean:
            out["mean"] = np.empty((4, F))
        if meta:
            out["meta"] = np.empty((B, 8))
        kept = ctypes.c_int32(-1)
        _lib.check(_lib.lib().pioran_psd_check_summary(self._h, B, mid, int(n_components), basis, int(bool(is_integrated_power)), float(f_min),
                                                       float(f_max), float(S_low), float(S_high), _ptr(theta), _ptr(norm), F, _ptr(freq),
                                                       int(bool(normalise)), int(bool(times_f)), Q, _ptr(probs), _ptr(out["quant"]), _ptr(out.get("mean")),
                                                       _ptr(out.get("meta")), _ptr(out["status"]), ctypes.cast(ctypes.byref(kept), ctypes.c_void_p)),
                   self._h)
        out["kept"] = kept.value
        return out

    # -- CARMA(p, q) models from their sampled parameters ---------------------------------------
    def carma_coefs(self, p, q, qa=None, qb=None, norm=1.0, *, r_alpha=None, beta=None, is_integrated_power=True, bounds=None, return_flags=False):
        """CARMA_celerite_coefs for B draws on the device (pioran_carma_coefs_batch).  Quad form: qa (B, p), qb (B, q), the quadratic factors the
        reference's models sample (r_alpha = quad2roots(qa), beta = roots2coeffs(quad2roots(qb))); roots form: r_alpha (B, p) complex, beta (B, q + 1).
        norm: scalar or (B,); bounds: (f_lo, f_hi) of check_roots_bounds, or None.  Returns A, Bc, C, Dd (B, J), J = (p + 1) // 2, and with
        return_flags the per-draw flag: 0, or why the draw is rejected (1 non-finite parameter, 2 a pair that is not a conjugate pair, 3 a root
        with real part >= 0, 4 outside the bounds); a rejected draw has (1, 0, 1, 0) in every term."""
        p, q, form, in1, in2, norm = _carma_args(p, q, qa, qb, norm, r_alpha, beta)
        B, J = in1.shape[0], (p + 1) // 2
        f_lo, f_hi = (0.0, 0.0) if bounds is None else map(float, bounds)
        A, Bc, C, Dd = (np.empty((B, J)) for _ in range(4))
        flags = np.zeros(B, dtype=np.int32)
        _lib.check(_lib.lib().pioran_carma_coefs_batch(self._h, B, p, q, form, _ptr(in1), _ptr(in2), _ptr(norm), int(bool(is_integrated_power)), f_lo,
                                                       f_hi, _ptr(A), _ptr(Bc), _ptr(C), _ptr(Dd), _ptr(flags)), self._h)
        return (A, Bc, C, Dd, flags) if return_flags else (A, Bc, C, Dd)

    def carma_vjp(self, p, q, qa, qb, norm, grad_a, grad_b, grad_c, grad_d, *, is_integrated_power=True):
        """Chain rule through quad2roots and CARMA_celerite_coefs on the device (pioran_carma_vjp_batch): dL/da, dL/db, dL/dc, dL/dd (B, J) ->
        dL/dqa (B, p), dL/dqb (B, q), dL/dnorm (B,).  Rejected draws get exact zeros."""
        p, q, _, qa, qb, norm = _carma_args(p, q, qa, qb, norm, None, None)
        B, J = qa.shape[0], (p + 1) // 2
        g = [_f64(x) for x in (grad_a, grad_b, grad_c, grad_d)]
        if any(x.shape != (B, J) for x in g):
            raise ValueError("grad_a, grad_b, grad_c, grad_d must be (B, J)")
        gqa, gqb, gnorm = np.empty((B, p)), np.empty((B, q)), np.empty(B)
        _lib.check(_lib.lib().pioran_carma_vjp_batch(self._h, B, p, q, _ptr(qa), _ptr(qb), _ptr(norm), int(bool(is_integrated_power)), *map(_ptr, g),
                                                     _ptr(gqa), _ptr(gqb) if q else None, _ptr(gnorm)), self._h)
        return gqa, gqb, gnorm

    def carma_psd(self, p, q, freq, qa=None, qb=None, norm=1.0, *, r_alpha=None, beta=None, is_integrated_power=True, bounds=None, times_f=False,
                  return_status=False):
        """evaluate(::CARMA, f) for B draws at the frequencies freq (F,): (B, F) (pioran_carma_psd_batch).  The draws as in carma_coefs; times_f:
        multiplied by the frequency (plot_f_P).  status (B,): 3, with NaN in the draw's row, for a rejected draw."""
        p, q, form, in1, in2, norm = _carma_args(p, q, qa, qb, norm, r_alpha, beta)
        freq = _f64(freq).reshape(-1)
        B, F = in1.shape[0], len(freq)
        f_lo, f_hi = (0.0, 0.0) if bounds is None else map(float, bounds)
        psd, st = np.empty((B, F)), np.zeros(B, dtype=np.int32)
        _lib.check(_lib.lib().pioran_carma_psd_batch(self._h, B, p, q, form, _ptr(in1), _ptr(in2), _ptr(norm), int(bool(is_integrated_power)), f_lo, f_hi,
                                                     F, _ptr(freq), int(bool(times_f)), _ptr(psd), _ptr(st)), self._h)
        return (psd, st) if return_status else psd

    def carma_psd_summary(self, p, q, freq, qa=None, qb=None, norm=1.0, *, r_alpha=None, beta=None, is_integrated_power=True, bounds=None,
                          times_f=False, probs=PPC_QUANTILES):
        """carma_psd with its array kept on the device and reduced there (pioran_carma_psd_summary): a dict with quant (Q, F), the quantiles per
        frequency over the draws with status 0, status (B,) and kept.  At most 4096 draws (the quantile kernel's limit)."""
        p, q, form, in1, in2, norm = _carma_args(p, q, qa, qb, norm, r_alpha, beta)
        freq, probs = _f64(freq).reshape(-1), _f64(probs).reshape(-1)
        B, F, Q = in1.shape[0], len(freq), len(probs)
        f_lo, f_hi = (0.0, 0.0) if bounds is None else map(float, bounds)
        out = dict(quant=np.empty((Q, F)), status=np.zeros(B, dtype=np.int32))
        kept = ctypes.c_int32(-1)
        _lib.check(_lib.lib().pioran_carma_psd_summary(self._h, B, p, q, form, _ptr(in1), _ptr(in2), _ptr(norm), int(bool(is_integrated_power)), f_lo,
                                                       f_hi, F, _ptr(freq), int(bool(times_f)), Q, _ptr(probs), _ptr(out["quant"]), _ptr(out["status"]),
                                                       ctypes.cast(ctypes.byref(kept), ctypes.c_void_p)), self._h)
        out["kept"] = kept.value
        return out

    def dense_nll(self, a, b, c, d, t, y, sigma2, return_info=False):
        a, b, c, d, t, y, sigma2 = map(_f64, (a, b, c, d, t, y, sigma2))
        out = ctypes.c_double()
        info = ctypes.c_int32()
        _lib.check(_lib.lib().pioran_dense_nll(self._h, len(t), len(a), _ptr(a), _ptr(b), _ptr(c), _ptr(d), _ptr(t),
                                               _ptr(y), _ptr(sigma2), ctypes.byref(out), ctypes.byref(info)), self._h)
        return (out.value, info.value) if return_info else out.value

    def dense_nll_batch(self, A, Bc, C, Dd, t, y, sigma2, mu=None, nu=None, return_info=False):
        """B dense +NLL values on one data set (pioran_dense_nll_batch): A, Bc (B, J); C, Dd (J,) or (B, J); mu, nu (B,) or
        None.  Independent factorisations run concurrently on the device."""
        A, Bc, C, Dd, t, y, sigma2 = map(_f64, (A, Bc, C, Dd, t, y, sigma2))
        if A.ndim != 2 or A.shape != Bc.shape:
            raise ValueError("A, Bc must be (B, J)")
        B, J = A.shape
        cd_shared = C.ndim == 1
        if C.shape != Dd.shape or C.shape != ((J,) if cd_shared else (B, J)):
            raise ValueError("C, Dd must be (J,) or (B, J)")
        mu = None if mu is None else _f64(np.broadcast_to(mu, (B,)))
        nu = None if nu is None else _f64(np.broadcast_to(nu, (B,)))
        out = np.empty(B); info = np.zeros(B, dtype=np.int32)
        _lib.check(_lib.lib().pioran_dense_nll_batch(self._h, len(t), J, B, _ptr(A), _ptr(Bc), _ptr(C), _ptr(Dd), int(cd_shared),
                                                     _ptr(t), _ptr(y), _ptr(sigma2), _ptr(mu), _ptr(nu), _ptr(out), _ptr(info)), self._h)
        return (out, info) if return_info else out

    def dense_nll_timed(self, a, b, c, d, t, y, sigma2):
        """dense_nll plus the event-timed phases of the call: (nll, info, {"build_ms", "factor_ms", "finish_ms"})."""
        a, b, c, d, t, y, sigma2 = map(_f64, (a, b, c, d, t, y, sigma2))
        out = ctypes.c_double()
        info = ctypes.c_int32()
        ms = (ctypes.c_float * 3)()
        _lib.check(_lib.lib().pioran_dense_nll_timed(self._h, len(t), len(a), _ptr(a), _ptr(b), _ptr(c), _ptr(d), _ptr(t),
                                                     _ptr(y), _ptr(sigma2), ctypes.byref(out), ctypes.byref(info), ms), self._h)
        return out.value, info.value, {"build_ms": ms[0], "factor_ms": ms[1], "finish_ms": ms[2]}

    def dense_predict_cov(self, a, b, c, d, tau, t, sigma2, return_info=False):
        """predict_cov(cov, tau, t, sigma2): posterior covariance at tau, (M, M)   src/direct_solver.jl:28-69."""
        a, b, c, d, tau, t, sigma2 = map(_f64, (a, b, c, d, tau, t, sigma2))
        out = np.empty((len(tau), len(tau)))
        info = ctypes.c_int32()
        _lib.check(_lib.lib().pioran_dense_predict_cov(self._h, len(t), len(a), _ptr(a), _ptr(b), _ptr(c), _ptr(d), _ptr(t),
                                                       _ptr(sigma2), len(tau), _ptr(tau), _ptr(out), ctypes.byref(info)),
                   self._h)
        return (out, info.value) if return_info else out

    def dense_predict(self, a, b, c, d, tau, t, y, sigma2, with_covariance=False, return_info=False):
        """predict_direct(cov, tau, t, y, sigma2[, with_covariance])   src/direct_solver.jl:75-119 (dense solver)."""
        a, b, c, d, tau, t, y, sigma2 = map(_f64, (a, b, c, d, tau, t, y, sigma2))
        mean_ = np.empty(len(tau))
        cov_ = np.empty((len(tau), len(tau))) if with_covariance else None
        info = ctypes.c_int32()
        _lib.check(_lib.lib().pioran_dense_predict(self._h, len(t), len(a), _ptr(a), _ptr(b), _ptr(c), _ptr(d), _ptr(t), _ptr(y),
                                                   _ptr(sigma2), len(tau), _ptr(tau), _ptr(mean_), _ptr(cov_),
                                                   ctypes.byref(info)), self._h)
        res = (mean_, cov_) if with_covariance else mean_
        return (res, info.value) if return_info else res

    def dense_covariance(self, a, b, c, d, t, sigma2):
        a, b, c, d, t, sigma2 = map(_f64, (a, b, c, d, t, sigma2))
        K = np.empty((len(t), len(t)), dtype=np.float64)
        _lib.check(_lib.lib().pioran_dense_covariance(self._h, len(t), len(a), _ptr(a), _ptr(b), _ptr(c), _ptr(d),
                                                      _ptr(t), _ptr(sigma2), _ptr(K)), self._h)
        return K  # symmetric, so row/column-major does not matter


_default_ctx: Context | None = None


def default_context() -> Context:
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(0)
    return _default_ctx


class Dataset:
    """A time series resident in HBM (pioran_ds): upload (t, y, sigma2) once, evaluate many batches."""

    def __init__(self, t, y, sigma2, ctx: Context | None = None):
        self.ctx = ctx or default_context()
        t, y, sigma2 = map(_f64, (t, y, sigma2))
        if not (len(t) == len(y) == len(sigma2)) or len(t) < 1:
            raise ValueError("t, y, sigma2 must be non-empty and of equal length")
        self.N = len(t)
        h = ctypes.c_void_p()
        _lib.check(_lib.lib().pioran_dataset_create(self.ctx._h, self.N, _ptr(t), _ptr(y), _ptr(sigma2),
                                                    ctypes.byref(h)), self.ctx._h)
        self._h = h
        self.J = None

    def close(self):
        if getattr(self, "_h", None) and self.ctx._h:
            _lib.lib().pioran_dataset_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def prepare(self, c, d, real_term=None):
        """Declare the (c, d) shared by the following device-pointer batches; builds the table."""
        c, d = _f64(c), _f64(d)
        rt = None if real_term is None else np.ascontiguousarray(real_term, dtype=np.int32)
        _lib.check(_lib.lib().pioran_dataset_prepare(self._h, len(c), _ptr(c), _ptr(d), _ptr(rt)), self.ctx._h)
        self.J = len(c)

    def logl_batch(self, A, Bc, C, Dd, mu=None, nu=None, Y=None, S2=None, shift=None, return_status=False):
        """B log-likelihoods, host arrays.  A, Bc: (B, J); C, Dd: (J,) shared or (B, J) per draw.
        shift (B,): the data set holds raw flux and yerr**2; draw b is evaluated on log(y - shift_b) with
        variances sigma2 / (y - shift_b)**2, transformed on the device (docs/src/ultranest.md:199-205)."""
        A, Bc, C, Dd = map(_f64, (A, Bc, C, Dd))
        if A.ndim != 2 or A.shape != Bc.shape:
            raise ValueError("A and Bc must be (B, J) arrays of equal shape")
        B, J = A.shape
        cd_shared = C.ndim == 1
        if C.shape != Dd.shape or C.shape != ((J,) if cd_shared else (B, J)):
            raise ValueError("C, Dd must be (J,) or (B, J)")
        mu = None if mu is None else _f64(np.broadcast_to(mu, (B,)))
        nu = None if nu is None else _f64(np.broadcast_to(nu, (B,)))
        if (Y is None) != (S2 is None):
            raise ValueError("Y and S2 must be given together")
        if shift is not None:
            if Y is not None:
                raise ValueError("give either shift or (Y, S2)")
            shift = _f64(np.broadcast_to(shift, (B,)))
            out = np.empty(B)
            st = np.zeros(B, dtype=np.int32)
            _lib.check(_lib.lib().pioran_celerite_logl_batch_shift(self._h, B, J, _ptr(A), _ptr(Bc), _ptr(C), _ptr(Dd),
                                                                   int(cd_shared), _ptr(mu), _ptr(nu), _ptr(shift),
                                                                   _ptr(out), _ptr(st)), self.ctx._h)
            return (out, st) if return_status else out
        if Y is not None:
            Y, S2 = _f64(Y), _f64(S2)
            if Y.shape != (B, self.N) or S2.shape != (B, self.N):
                raise ValueError("Y, S2 must be (B, N)")
        out = np.empty(B)
        st = np.zeros(B, dtype=np.int32)
        _lib.check(_lib.lib().pioran_celerite_logl_batch(self._h, B, J, _ptr(A), _ptr(Bc), _ptr(C), _ptr(Dd),
                                                         int(cd_shared), _ptr(mu), _ptr(nu), _ptr(Y), _ptr(S2),
                                                         _ptr(out), _ptr(st)), self.ctx._h)
        return (out, st) if return_status else out

    def predict(self, A, Bc, C, Dd, tau, mu=None, nu=None, return_status=False):
        """Posterior mean at the times tau (M,), any order, for B coefficient sets sharing (C, Dd: (J,)) or with (C, Dd: (B, J)) of their own:
        pred of src/celerite_solver.jl:363-483 (+ the constant mean mu_b).  Error, measured against a long-double dense truth K* K^-1 (y - mu)
        (docs/EXPERIMENTS.md section 24), in units of max |y - mu|: <= 6.2e-15 at every edge shape (R 1..143, N 1..257, M 1..257, sigma2 as
        given and x 1e-6) on the fused, the two-pass, the per-draw-table and the step-by-step route alike, 1.4e-14 on the worst of 40 random
        shapes; the fp64 references deviate by 1.2e-14 resp. 4.9e-14 on the same draws.  Returns (B, M)."""
        A, Bc, C, Dd, tau = map(_f64, (A, Bc, C, Dd, tau))
        if A.ndim != 2 or A.shape != Bc.shape or C.shape not in ((A.shape[1],), A.shape) or Dd.shape != C.shape or tau.ndim != 1:
            raise ValueError("A, Bc must be (B, J), C, Dd (J,) or (B, J) and tau (M,)")
        B, J = A.shape
        mu = None if mu is None else _f64(np.broadcast_to(mu, (B,)))
        nu = None if nu is None else _f64(np.broadcast_to(nu, (B,)))
        out = np.empty((B, len(tau)))
        st = np.zeros(B, dtype=np.int32)
        _lib.check(_lib.lib().pioran_celerite_predict(self._h, B, J, _ptr(A), _ptr(Bc), _ptr(C), _ptr(Dd), int(C.ndim == 1), _ptr(mu),
                                                      _ptr(nu), len(tau), _ptr(tau), _ptr(out), _ptr(st)), self.ctx._h)
        return (out, st) if return_status else out

    def predict_var(self, A, Bc, C, Dd, tau, nu=None, return_status=False):
        """Posterior variance of the latent process at the times tau (M,), any order, for B coefficient sets, through the celerite
        factorisation in O((N + M) R^2): diag(predict_cov) of src/scalable_GP.jl:103-104 without the dense matrix.  The data set's y
        does not enter.  At most 64 active rows.  Error, measured against a long-double dense truth (docs/EXPERIMENTS.md section 23), in
        units of k(0) = sum(a): <= 5e-15 on well-conditioned draws of any shape (R 1..64, N 1..120), 2.5e-13 at N = 150 and 8.4e-12 at N = 1000
        on draws with nu min(sigma2) / k(0) near 1e-10 (the recurrences' own growth with N: the numpy prototype shows the same).  Returns
        (B, M); status 2 and NaN where a draw is not positive definite."""
        A, Bc, C, Dd, tau = map(_f64, (A, Bc, C, Dd, tau))
        if A.ndim != 2 or A.shape != Bc.shape or C.shape not in ((A.shape[1],), A.shape) or Dd.shape != C.shape or tau.ndim != 1:
            raise ValueError("A, Bc must be (B, J), C, Dd (J,) or (B, J) and tau (M,)")
        if not np.isfinite(tau).all():
            raise ValueError("tau must be finite")
        B, J = A.shape
        nu = None if nu is None else _f64(np.broadcast_to(nu, (B,)))
        out = np.empty((B, len(tau)))
        st = np.zeros(B, dtype=np.int32)
        _lib.check(_lib.lib().pioran_celerite_predict_var(self._h, B, J, _ptr(A), _ptr(Bc), _ptr(C), _ptr(Dd), int(C.ndim == 1), _ptr(nu),
                                                          len(tau), _ptr(tau), _ptr(out), _ptr(st)), self.ctx._h)
        return (out, st) if return_status else out

    def rand_posterior(self, A, Bc, C, Dd, tau, q_data, q_new, eps, mu=None, nu=None, shift=None, return_status=False):
        """Draws of the posterior at the times tau (M,), any order, for B coefficient sets, in O((N + M) R^2) by Matheron's rule
        (pioran_celerite_rand_posterior): a prior draw on the merged grid of (t, tau) from the normals q_data (B, N) and q_new (B, M), corrected
        by the posterior mean of y - f~(t) - sqrt(nu sigma2) eps with eps (B, N).  Jointly N(mean(fp, tau), cov(fp, tau)), also where tau repeats
        or meets a data time (the normal of such a tau is not used).  shift (B,): the data set holds raw flux and yerr**2, draw b conditions on
        log(y - shift_b) and the result is in that scale.  Error, measured against a long-double dense truth (docs/EXPERIMENTS.md section 26),
        in units of max(max |y - mu|, max |f~|): <= 5.7e-14 at every edge shape (R 1..143, N 1..257, tau outside / on the data, tied, crowded;
        sigma2 as given and x 1e-6) on the windowed and the step-by-step route alike, where the fp64 references deviate by up to 7.6e-14.
        Returns (B, M) [, status (B,)]: status 2 and a NaN row for a draw whose matrix is not positive definite — which the zero-noise prior
        draw on the merged grid is, numerically, when a tau lies very close to a data time and the process is smooth — or whose y - shift is
        not positive."""
        A, Bc, C, Dd, tau, q_data, q_new, eps = map(_f64, (A, Bc, C, Dd, tau, q_data, q_new, eps))
        if A.ndim != 2 or A.shape != Bc.shape or C.shape not in ((A.shape[1],), A.shape) or Dd.shape != C.shape or tau.ndim != 1:
            raise ValueError("A, Bc must be (B, J), C, Dd (J,) or (B, J) and tau (M,)")
        if not np.isfinite(tau).all():
            raise ValueError("tau must be finite")
        B, J = A.shape
        M = len(tau)
        if q_data.shape != (B, self.N) or eps.shape != (B, self.N) or q_new.shape != (B, M):
            raise ValueError("q_data, eps must be (B, N) and q_new (B, M)")
        mu = None if mu is None else _f64(np.broadcast_to(mu, (B,)))
        nu = None if nu is None else _f64(np.broadcast_to(nu, (B,)))
        shift = None if shift is None else _f64(np.broadcast_to(shift, (B,)))
        out = np.empty((B, M))
        st = np.zeros(B, dtype=np.int32)
        _lib.check(_lib.lib().pioran_celerite_rand_posterior(self._h, B, J, _ptr(A), _ptr(Bc), _ptr(C), _ptr(Dd), int(C.ndim == 1), _ptr(mu),
                                                             _ptr(nu), _ptr(shift), M, _ptr(tau), _ptr(q_data), _ptr(q_new), _ptr(eps),
                                                             _ptr(out), _ptr(st)), self.ctx._h)
        return (out, st) if return_status else out

    def rand_posterior_summary(self, A, Bc, C, Dd, tau, q_data, q_new, eps, probs=PPC_QUANTILES, mu=None, nu=None, shift=None, backtransform=False,
                               res_cols=None, res_ref=None, res_scale=None):
        """rand_posterior with the draws left on the device and reduced there (pioran_celerite_rand_posterior_summary): the quantiles `probs`
        and the mean over the draws with status 0 at every tau and, with res_cols (Nres,) indices into tau, res_ref, res_scale (Nres,), of the
        residuals (res_ref - draw[res_cols]) / res_scale.  backtransform (needs shift): the summaries are of exp(draw + shift_b).  The draws are
        rand_posterior's for the same arguments, the reduction is Context.quantiles'.  Returns a dict: ts_quantiles (Q, M), ts_mean (M,),
        res_quantiles (Q, Nres), res_mean (Nres,) (None without res_cols), status (B,), kept."""
        A, Bc, C, Dd, tau, q_data, q_new, eps = map(_f64, (A, Bc, C, Dd, tau, q_data, q_new, eps))
        probs = _f64(probs).reshape(-1)
        if A.ndim != 2 or A.shape != Bc.shape or C.shape not in ((A.shape[1],), A.shape) or Dd.shape != C.shape or tau.ndim != 1:
            raise ValueError("A, Bc must be (B, J), C, Dd (J,) or (B, J) and tau (M,)")
        if not np.isfinite(tau).all():
            raise ValueError("tau must be finite")
        B, J = A.shape
        M = len(tau)
        if q_data.shape != (B, self.N) or eps.shape != (B, self.N) or q_new.shape != (B, M):
            raise ValueError("q_data, eps must be (B, N) and q_new (B, M)")
        mu = None if mu is None else _f64(np.broadcast_to(mu, (B,)))
        nu = None if nu is None else _f64(np.broadcast_to(nu, (B,)))
        shift = None if shift is None else _f64(np.broadcast_to(shift, (B,)))
        Q, Nres = len(probs), 0
        res_q = res_m = None
        if res_cols is not None:
            res_cols = np.ascontiguousarray(res_cols, dtype=np.int32).reshape(-1)
            Nres = len(res_cols)
            if res_ref is None or res_scale is None:
                raise ValueError("res_cols needs res_ref and res_scale")
            res_ref, res_scale = _f64(res_ref).reshape(-1), _f64(res_scale).reshape(-1)
            if res_ref.shape != (Nres,) or res_scale.shape != (Nres,):
                raise ValueError("res_ref, res_scale must be (Nres,)")
            res_q, res_m = np.empty((Q, Nres)), np.empty(Nres)
        else:
            res_ref = res_scale = None
        ts_q, ts_m = np.empty((Q, M)), np.empty(M)
        st = np.zeros(B, dtype=np.int32)
        kept = ctypes.c_int32(-1)
        _lib.check(_lib.lib().pioran_celerite_rand_posterior_summary(
            self._h, B, J, _ptr(A), _ptr(Bc), _ptr(C), _ptr(Dd), int(C.ndim == 1), _ptr(mu), _ptr(nu), _ptr(shift), M, _ptr(tau), _ptr(q_data),
            _ptr(q_new), _ptr(eps), int(bool(backtransform)), Q, _ptr(probs), _ptr(ts_q), _ptr(ts_m), Nres, _ptr(res_cols), _ptr(res_ref),
            _ptr(res_scale), _ptr(res_q), _ptr(res_m), _ptr(st), ctypes.cast(ctypes.byref(kept), ctypes.c_void_p)), self.ctx._h)
        return dict(ts_quantiles=ts_q, ts_mean=ts_m, res_quantiles=res_q, res_mean=res_m, status=st, kept=kept.value)

    def logl_grad(self, A, Bc, C, Dd, mu=None, nu=None, series_grad=False, shift=None, cd_grad=True):
        """log L and its gradient for B draws: returns a dict with logl (B,), status, grad_a, grad_b, grad_c, grad_d (B, J),
        grad_mu, grad_nu (B,) and, with series_grad, grad_y, grad_sigma2 (B, N).  C, Dd: (J,) shared by the draws or
        (B, J) per draw (QPO / CARMA / free Celerite terms).  grad_c / grad_d are per draw also when (C, Dd) are shared.
        shift (B,): the shifted log-flux models (the data set holds raw flux and yerr**2); adds grad_shift (B,)."""
        A, Bc, C, Dd = map(_f64, (A, Bc, C, Dd))
        if A.ndim != 2 or A.shape != Bc.shape:
            raise ValueError("A, Bc must be (B, J)")
        B, J = A.shape
        cd_shared = C.ndim == 1
        if C.shape != Dd.shape or C.shape != ((J,) if cd_shared else (B, J)):
            raise ValueError("C, Dd must be (J,) or (B, J)")
        mu_ = None if mu is None else _f64(np.broadcast_to(mu, (B,)))
        nu_ = None if nu is None else _f64(np.broadcast_to(nu, (B,)))
        out = np.empty(B); st = np.zeros(B, dtype=np.int32)
        ga, gb = np.empty((B, J)), np.empty((B, J))
        gc = np.empty((B, J)) if cd_grad else None
        gd = np.empty((B, J)) if cd_grad else None
        gnu, gmu = np.empty(B), np.empty(B)
        L = _lib.lib()
        if shift is not None:
            shift = _f64(np.broadcast_to(shift, (B,)))
            gsh = np.empty(B)
            _lib.check(L.pioran_celerite_logl_grad_shift(self._h, B, J, _ptr(A), _ptr(Bc), _ptr(C), _ptr(Dd), int(cd_shared), _ptr(mu_),
                                                         _ptr(nu_), _ptr(shift), _ptr(out), _ptr(st), _ptr(ga), _ptr(gb), _ptr(gc),
                                                         _ptr(gd), _ptr(gnu), _ptr(gmu), _ptr(gsh)), self.ctx._h)
            return {"logl": out, "status": st, "grad_a": ga, "grad_b": gb, "grad_c": gc, "grad_d": gd, "grad_nu": gnu,
                    "grad_mu": gmu, "grad_shift": gsh, "grad_y": None, "grad_sigma2": None}
        gy = np.empty((B, self.N)) if series_grad else None
        gs = np.empty((B, self.N)) if series_grad else None
        _lib.check(L.pioran_celerite_logl_grad(self._h, B, J, _ptr(A), _ptr(Bc), _ptr(C), _ptr(Dd), int(cd_shared), _ptr(mu_), _ptr(nu_),
                                               _ptr(out), _ptr(st), _ptr(ga), _ptr(gb), _ptr(gc), _ptr(gd), _ptr(gnu), _ptr(gmu),
                                               _ptr(gy), _ptr(gs)), self.ctx._h)
        return {"logl": out, "status": st, "grad_a": ga, "grad_b": gb, "grad_c": gc, "grad_d": gd, "grad_nu": gnu, "grad_mu": gmu,
                "grad_y": gy, "grad_sigma2": gs}

    def logpdf_theta_grad(self, model, theta, norm, f_min, f_max, n_components=20, S_low=20.0, S_high=20.0, *,
                          is_integrated_power=True, basis_function="SHO", mu=None, nu=None, shift=None, approx_on="host",
                          return_coef_grads=False, qpo=None):
        """log L and its gradient with respect to the SAMPLED parameters of the reference's models
        (README.md:38-71: theta = PSD parameters, norm = variance, nu, mu): the device gradient w.r.t. (a, b, nu, mu)
        chained through `approx` on the host (approx_batch_vjp) or, approx_on="device", in one device call
        (pioran_logpdf_batch_theta_grad: approx and its reverse mode run either side of the same reverse-mode kernels).
        Returns a dict: logl, status, grad_theta (B, P), grad_norm, grad_nu, grad_mu (B,) and, with return_coef_grads,
        the intermediate grad_a, grad_b (B, J).
        qpo: (B, n_qpo, 3) or (B, 3) = (S0, f0, Q) of QPO features added to the continuum, as in logpdf_theta: the dict also holds
        grad_qpo (B, n_qpo, 3) and, with return_coef_grads, coef_a .. coef_d and grad_a .. grad_d (B, J + n_qpo); every draw has its own (c, d)
        (pioran_logpdf_batch_theta_qpo_grad on the device, approx_batch_qpo[_vjp] around logl_grad on the host).  On the device a draw the
        reference could not evaluate (non-finite parameters, f0 <= 0, Q <= 1/2) has status 3, logl = -inf and zeros in every gradient row."""
        if approx_on not in ("host", "device"):
            raise ValueError('approx_on must be "host" or "device"')
        if qpo is not None:
            return self._logpdf_theta_qpo_grad(model, theta, norm, qpo, f_min, f_max, n_components, S_low, S_high, is_integrated_power,
                                               basis_function, mu, nu, shift, approx_on, return_coef_grads)
        if approx_on == "device":
            return self._logpdf_theta_grad_device(model, theta, norm, f_min, f_max, n_components, S_low, S_high, is_integrated_power,
                                                  basis_function, mu, nu, shift, return_coef_grads)
        from .psd import approx_batch, approx_batch_vjp
        theta = np.atleast_2d(_f64(theta))
        A, Bc, C, Dd = approx_batch(model, theta, f_min, f_max, n_components, norm, S_low, S_high,
                                    is_integrated_power=is_integrated_power, basis_function=basis_function)
        g = self.logl_grad(A, Bc, C, Dd, mu=mu, nu=nu, shift=shift, cd_grad=False)   # (c, d) are fixed by the spectral grid: windowed reverse mode
        gth, gnorm = approx_batch_vjp(model, theta, f_min, f_max, n_components, norm, g["grad_a"], g["grad_b"], S_low, S_high,
                                      is_integrated_power=is_integrated_power, basis_function=basis_function)
        res = {"logl": g["logl"], "status": g["status"], "grad_theta": gth, "grad_norm": gnorm,
               "grad_nu": g["grad_nu"] if nu is not None else None, "grad_mu": g["grad_mu"] if mu is not None else None,
               "grad_shift": g.get("grad_shift")}
        if return_coef_grads:
            res["grad_a"], res["grad_b"] = g["grad_a"], g["grad_b"]
        return res

    def _logpdf_theta_grad_device(self, model, theta, norm, f_min, f_max, n_components, S_low, S_high, is_integrated_power, basis_function,
                                  mu, nu, shift, return_coef_grads):
        mid, basis, theta, norm = _theta_args(model, theta, norm, basis_function)
        B, P = theta.shape
        mu, nu, shift = (None if v is None else _f64(np.broadcast_to(v, (B,))) for v in (mu, nu, shift))
        out, st = np.empty(B), np.zeros(B, dtype=np.int32)
        gth, gnorm = np.empty((B, P)), np.empty(B)
        gnu, gmu, gsh = (None if v is None else np.empty(B) for v in (nu, mu, shift))
        Jt = n_components * (1 + basis)
        ga = np.empty((B, Jt)) if return_coef_grads else None
        gb = np.empty((B, Jt)) if return_coef_grads else None
        _lib.check(_lib.lib().pioran_logpdf_batch_theta_grad(
            self._h, B, mid, int(n_components), basis, int(bool(is_integrated_power)), float(f_min), float(f_max), float(S_low), float(S_high),
            _ptr(theta), _ptr(norm), _ptr(mu), _ptr(nu), _ptr(shift), _ptr(out), _ptr(st), _ptr(gth), _ptr(gnorm), _ptr(gnu), _ptr(gmu),
            _ptr(gsh), _ptr(ga), _ptr(gb)), self.ctx._h)
        res = {"logl": out, "status": st, "grad_theta": gth, "grad_norm": gnorm, "grad_nu": gnu, "grad_mu": gmu, "grad_shift": gsh}
        if return_coef_grads:
            res["grad_a"], res["grad_b"] = ga, gb
        return res

    def _logpdf_theta_qpo_grad(self, model, theta, norm, qpo, f_min, f_max, n_components, S_low, S_high, is_integrated_power, basis_function,
                               mu, nu, shift, approx_on, return_coef_grads):
        mid, basis, theta, norm = _theta_args(model, theta, norm, basis_function)
        B, P = theta.shape
        qpo = _f64(np.asarray(qpo, dtype=np.float64).reshape(B, -1, 3))
        n_qpo = qpo.shape[1]
        names = ("coef_a", "coef_b", "coef_c", "coef_d", "grad_a", "grad_b", "grad_c", "grad_d")
        if approx_on == "host":
            from .psd import approx_batch_qpo, approx_batch_qpo_vjp
            kw = dict(is_integrated_power=is_integrated_power, basis_function=basis_function)
            co = approx_batch_qpo(model, theta, qpo, f_min, f_max, n_components, norm, S_low, S_high, **kw)
            g = self.logl_grad(*co, mu=mu, nu=nu, shift=shift, cd_grad=True)
            gr = [g[k] for k in names[4:]]
            gth, gnorm, gq = approx_batch_qpo_vjp(model, theta, qpo, f_min, f_max, n_components, norm, *gr, S_low, S_high, **kw)
            res = {"logl": g["logl"], "status": g["status"], "grad_theta": gth, "grad_norm": gnorm, "grad_qpo": gq,
                   "grad_nu": g["grad_nu"] if nu is not None else None, "grad_mu": g["grad_mu"] if mu is not None else None,
                   "grad_shift": g.get("grad_shift")}
            if return_coef_grads:
                res.update(zip(names, [*co, *gr]))
            return res
        mu, nu, shift = (None if v is None else _f64(np.broadcast_to(v, (B,))) for v in (mu, nu, shift))
        out, st = np.empty(B), np.zeros(B, dtype=np.int32)
        gth, gnorm, gq = np.empty((B, P)), np.empty(B), np.empty((B, n_qpo, 3))
        gnu, gmu, gsh = (None if v is None else np.empty(B) for v in (nu, mu, shift))
        Jt = n_components * (1 + basis) + n_qpo
        co = [np.empty((B, Jt)) if return_coef_grads else None for _ in names]
        _lib.check(_lib.lib().pioran_logpdf_batch_theta_qpo_grad(
            self._h, B, mid, int(n_components), basis, int(bool(is_integrated_power)), float(f_min), float(f_max), float(S_low), float(S_high),
            _ptr(theta), _ptr(norm), _ptr(mu), _ptr(nu), _ptr(shift), n_qpo, _ptr(qpo), _ptr(out), _ptr(st), _ptr(gth), _ptr(gnorm), _ptr(gq),
            _ptr(gnu), _ptr(gmu), _ptr(gsh), *map(_ptr, co)), self.ctx._h)
        res = {"logl": out, "status": st, "grad_theta": gth, "grad_norm": gnorm, "grad_qpo": gq, "grad_nu": gnu, "grad_mu": gmu, "grad_shift": gsh}
        if return_coef_grads:
            res.update(zip(names, co))
        return res

    def logl_batch_dev(self, B, dA, dBc, dmu=0, dnu=0, dY=0, dS2=0, dout=0, dstatus=0):
        """Device-pointer (int addresses) asynchronous variant; (c, d) from prepare()."""
        v = ctypes.c_void_p
        _lib.check(_lib.lib().pioran_celerite_logl_batch_dev(self._h, int(B), v(dA), v(dBc), v(dmu or None),
                                                             v(dnu or None), v(dY or None), v(dS2 or None), v(dout),
                                                             v(dstatus or None)), self.ctx._h)


    def logpdf_theta(self, model, theta, norm, f_min, f_max, n_components=20, S_low=20.0, S_high=20.0, *,
                     is_integrated_power=True, basis_function="SHO", mu=None, nu=None, shift=None, qpo=None,
                     return_status=False, return_coefs=False):
        """theta -> log L in one call, `approx` running on the device (pioran_logpdf_batch_theta).
        model: SingleBendingPowerLaw / DoubleBendingPowerLaw (the class); theta: (B, 3 | 5); norm: scalar or (B,)
        — same meaning as the arguments of approx (src/psd.jl:214-289); mu, nu, shift as in logl_batch.
        qpo: (B, n_qpo, 3) or (B, 3) = (S0, f0, Q) of the QPO features added to the continuum (src/psd.jl:15-27, 228-241)."""
        mid, basis, theta, norm = _theta_args(model, theta, norm, basis_function)
        B = theta.shape[0]
        mu, nu, shift = (None if v is None else _f64(np.broadcast_to(v, (B,))) for v in (mu, nu, shift))
        n_qpo = 0
        if qpo is not None:
            qpo = _f64(np.asarray(qpo, dtype=np.float64).reshape(B, -1, 3))
            n_qpo = qpo.shape[1]
        Jt = n_components * (1 if basis == 0 else 2) + n_qpo
        out = np.empty(B)
        st = np.zeros(B, dtype=np.int32)
        Ao = np.empty((B, Jt)) if return_coefs else None
        Bo = np.empty((B, Jt)) if return_coefs else None
        _lib.check(_lib.lib().pioran_logpdf_batch_theta(self._h, B, mid, int(n_components), basis, int(bool(is_integrated_power)),
                                                        float(f_min), float(f_max), float(S_low), float(S_high), _ptr(theta),
                                                        _ptr(norm), _ptr(mu), _ptr(nu), _ptr(shift), n_qpo, _ptr(qpo), _ptr(out), _ptr(st),
                                                        _ptr(Ao), _ptr(Bo)), self.ctx._h)
        res = (out, st) if return_status else (out,)
        if return_coefs:
            res = res + (Ao, Bo)
        return res if len(res) > 1 else res[0]

    def logpdf_carma(self, p, q, qa, qb, norm, *, is_integrated_power=True, bounds=None, mu=None, nu=None, shift=None, return_status=False,
                     return_coefs=False):
        """(qa, qb, norm) -> log L in one call for the CARMA(p, q) models of docs/src/carma.md (pioran_logpdf_batch_carma): quad2roots,
        CARMA_celerite_coefs and the root checks run on the device in front of the per-draw-(c, d) value path.  qa (B, p), qb (B, q); norm scalar
        or (B,); bounds = (f_lo, f_hi) of the models' root checks or None; mu, nu, shift as in logl_batch.  A rejected draw has log L = -inf and
        status 3 (what the models do with @addlogprob! -Inf).  return_coefs: also A, Bc, C, Dd (B, J)."""
        p, q, _, qa, qb, norm = _carma_args(p, q, qa, qb, norm, None, None)
        B, J = qa.shape[0], (p + 1) // 2
        mu, nu, shift = (None if v is None else _f64(np.broadcast_to(v, (B,))) for v in (mu, nu, shift))
        f_lo, f_hi = (0.0, 0.0) if bounds is None else map(float, bounds)
        out, st = np.empty(B), np.zeros(B, dtype=np.int32)
        co = [np.empty((B, J)) if return_coefs else None for _ in range(4)]
        _lib.check(_lib.lib().pioran_logpdf_batch_carma(self._h, B, p, q, _ptr(qa), _ptr(qb), _ptr(norm), int(bool(is_integrated_power)), f_lo, f_hi,
                                                        _ptr(mu), _ptr(nu), _ptr(shift), _ptr(out), _ptr(st), *map(_ptr, co)), self.ctx._h)
        res = (out, st) if return_status else (out,)
        if return_coefs:
            res = res + tuple(co)
        return res if len(res) > 1 else res[0]

    def logpdf_carma_grad(self, p, q, qa, qb, norm, *, is_integrated_power=True, bounds=None, mu=None, nu=None, shift=None, return_coef_grads=False):
        """log L and its gradient with respect to the SAMPLED parameters of the CARMA models (pioran_logpdf_batch_carma_grad): the coefficients, the
        reverse mode with grad_c / grad_d and the chain back through CARMA_celerite_coefs and quad2roots.  Returns a dict: logl, status,
        grad_qa (B, p), grad_qb (B, q), grad_norm (B,), grad_nu, grad_mu, grad_shift (None where the input is None) and, with return_coef_grads, the
        intermediates grad_a, grad_b, grad_c, grad_d (B, J).  A rejected draw: status 3, logl = -inf, exact zeros in every gradient row."""
        p, q, _, qa, qb, norm = _carma_args(p, q, qa, qb, norm, None, None)
        B, J = qa.shape[0], (p + 1) // 2
        mu, nu, shift = (None if v is None else _f64(np.broadcast_to(v, (B,))) for v in (mu, nu, shift))
        f_lo, f_hi = (0.0, 0.0) if bounds is None else map(float, bounds)
        out, st = np.empty(B), np.zeros(B, dtype=np.int32)
        gqa, gqb, gnorm = np.empty((B, p)), np.empty((B, q)), np.empty(B)
        gnu, gmu, gsh = (None if v is None else np.empty(B) for v in (nu, mu, shift))
        co = [np.empty((B, J)) if return_coef_grads else None for _ in range(4)]
        _lib.check(_lib.lib().pioran_logpdf_batch_carma_grad(self._h, B, p, q, _ptr(qa), _ptr(qb), _ptr(norm), int(bool(is_integrated_power)), f_lo,
                                                             f_hi, _ptr(mu), _ptr(nu), _ptr(shift), _ptr(out), _ptr(st), _ptr(gqa), _ptr(gqb) if q else None,
                                                             _ptr(gnorm), _ptr(gnu), _ptr(gmu), _ptr(gsh), *map(_ptr, co)), self.ctx._h)
        res = {"logl": out, "status": st, "grad_qa": gqa, "grad_qb": gqb, "grad_norm": gnorm, "grad_nu": gnu, "grad_mu": gmu, "grad_shift": gsh}
        if return_coef_grads:
            res.update(zip(("grad_a", "grad_b", "grad_c", "grad_d"), co))
        return res

    def logl_batch_shift_dev(self, B, dA, dBc, dmu=0, dnu=0, dshift=0, dout=0, dstatus=0):
        """Device-pointer asynchronous variant of the shifted-log-flux batch; (c, d) from prepare()."""
        v = ctypes.c_void_p
        _lib.check(_lib.lib().pioran_celerite_logl_batch_shift_dev(self._h, int(B), v(dA), v(dBc), v(dmu or None),
                                                                   v(dnu or None), v(dshift), v(dout),
                                                                   v(dstatus or None)), self.ctx._h)


class Farm:
    """In-process farm over several GPUs (pioran_farm): one context + resident data set per listed device, one host
    thread per device per call, contiguous shards of the draws.  For launcher-less hosts (a single Julia / Python
    process driving a node); the process-per-GPU route is pioran.jl_amd/farm.py."""

    def __init__(self, devices, t, y, sigma2):
        t, y, sigma2 = map(_f64, (t, y, sigma2))
        dev = np.ascontiguousarray(devices, dtype=np.int32)
        h = ctypes.c_void_p()
        _lib.check(_lib.lib().pioran_farm_create(len(dev), _ptr(dev), len(t), _ptr(t), _ptr(y), _ptr(sigma2), ctypes.byref(h)))
        self._h = h
        self.N = len(t)

    def __len__(self):
        return _lib.lib().pioran_farm_size(self._h)

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().pioran_farm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def logl_batch(self, A, Bc, C, Dd, mu=None, nu=None, shift=None, Y=None, S2=None, return_status=False):
        """Y, S2: per-draw series (B, N) — e.g. y - mean_b(t) for a CustomMean model
        (examples/ultranest/single_pl_periodicity.jl:115); exclusive with shift."""
        A, Bc, C, Dd = map(_f64, (A, Bc, C, Dd))
        B, J = A.shape
        cd_shared = C.ndim == 1
        mu = None if mu is None else _f64(np.broadcast_to(mu, (B,)))
        nu = None if nu is None else _f64(np.broadcast_to(nu, (B,)))
        shift = None if shift is None else _f64(np.broadcast_to(shift, (B,)))
        out = np.empty(B)
        st = np.zeros(B, dtype=np.int32)
        if (Y is None) != (S2 is None) or (Y is not None and shift is not None):
            raise ValueError("Y and S2 come together, and not with shift")
        if Y is not None:
            Y, S2 = _f64(Y), _f64(S2)
            if Y.shape != (B, self.N) or S2.shape != (B, self.N):
                raise ValueError("Y, S2 must be (B, N)")
            _lib.check(_lib.lib().pioran_farm_logl_batch_series(self._h, B, J, _ptr(A), _ptr(Bc), _ptr(C), _ptr(Dd), int(cd_shared),
                                                                _ptr(mu), _ptr(nu), _ptr(Y), _ptr(S2), _ptr(out), _ptr(st)))
        else:
            _lib.check(_lib.lib().pioran_farm_logl_batch(self._h, B, J, _ptr(A), _ptr(Bc), _ptr(C), _ptr(Dd), int(cd_shared),
                                                         _ptr(mu), _ptr(nu), _ptr(shift), _ptr(out), _ptr(st)))
        return (out, st) if return_status else out


# ---------------------------------------------------------------------------------------------
# mean functions (AbstractGPs ConstMean / ZeroMean / CustomMean as used at scalable_GP.jl:164)
# ---------------------------------------------------------------------------------------------
class CustomMean:
    def __init__(self, f):
        self.f = f

    def __call__(self, x):
        return np.asarray(self.f(np.asarray(x, float)), float)


def _mean_vector(mean, x):
    if isinstance(mean, CustomMean):
        return mean(x)
    return np.full(len(x), float(mean))


class ScalableGP:
    """ScalableGP(kernel) | ScalableGP(mu, kernel) | ScalableGP(mu, kernel, solver)   scalable_GP.jl:24-40."""

    def __init__(self, *args):
        if len(args) == 1:
            mean, kernel, solver = 0.0, args[0], "celerite"
        elif len(args) == 2:
            mean, kernel, solver = args[0], args[1], "celerite"
        elif len(args) == 3:
            mean, kernel, solver = args
        else:
            raise TypeError("ScalableGP(kernel) | ScalableGP(mean, kernel[, solver])")
        if not isinstance(kernel, SemiSeparable):
            raise TypeError("kernel must be a SemiSeparable covariance")
        self.mean, self.kernel, self.solver = mean, kernel, str(solver).lstrip(":")

    def __call__(self, t, sigma2=None):
        t = _f64(t)
        s2 = np.zeros(len(t)) if sigma2 is None else _f64(np.broadcast_to(sigma2, t.shape))
        return FiniteScalableGP(self, t, s2)


class FiniteScalableGP:
    """f(t, sigma2): AbstractGPs.FiniteGP{<:ScalableGP} (scalable_GP.jl:42)."""

    def __init__(self, f: ScalableGP, x, sigma2):
        self.f, self.x, self.sigma2 = f, x, sigma2


class PosteriorGP:
    """posterior(f(t, sigma2), y)   src/scalable_GP.jl:44-55."""

    def __init__(self, fx: "FiniteScalableGP", y):
        self.f, self.y = fx, _f64(y).reshape(-1)
        if len(self.y) != len(fx.x):
            raise ValueError("y must have one value per time stamp")


def posterior(fx: "FiniteScalableGP", y) -> PosteriorGP:
    return PosteriorGP(fx, y)


def predict(cov: SemiSeparable, tau, t, y, sigma2, ctx: Context | None = None):
    """predict(cov, tau, t, y, sigma2): posterior mean of the zero-mean GP   src/celerite_solver.jl:348-361."""
    a, b, c, d = (np.real(np.atleast_1d(v)) for v in cov.celerite_coefs())
    ds = Dataset(t, y, sigma2, ctx)
    try:
        return ds.predict(a[None, :], b[None, :], c, d, tau)[0]
    finally:
        ds.close()


def mean(fp: PosteriorGP, tau=None, ctx: Context | None = None):
    """mean(fp[, tau])   src/scalable_GP.jl:64-72, 90-91: predict on y - mean(t), plus mean(tau)."""
    x = fp.f.x
    tau = x if tau is None else _f64(tau).reshape(-1)
    y0 = fp.y - _mean_vector(fp.f.f.mean, x)
    return predict(fp.f.f.kernel, tau, x, y0, fp.f.sigma2, ctx=ctx) + _mean_vector(fp.f.f.mean, tau)


def predict_cov(cov_fn: SemiSeparable, tau, t, sigma2, ctx: Context | None = None):
    """predict_cov(cov, tau, t, sigma2)   src/direct_solver.jl:28-69 (dense, MFMA Cholesky of the augmented matrix).
    Error, measured against a long-double dense truth (tests/test_gpu_dense_truth.py, docs/EXPERIMENTS.md section 37) in units of k(0): at most
    9.3 eps over all M x M entries at every edge shape (N 1..130, M 1..129, sigma2 as given and x 1e-6), where the fp64 references sit at up to
    7 eps; the mean of predict_direct at most 190 eps of max |mean| (3.6 x the references' deviation).  The panel solve multiplies by explicit
    inverses of 16 x 16 diagonal blocks: see log_likelihood_direct for what that costs on a near-singular block."""
    a, b, c, d = (np.real(np.atleast_1d(v)) for v in cov_fn.celerite_coefs())
    K, info = (ctx or default_context()).dense_predict_cov(a, b, c, d, tau, t, sigma2, return_info=True)
    if info != 0:
        raise np.linalg.LinAlgError(f"matrix is not positive definite; Cholesky factorization failed at pivot {info}")
    return K


def predict_direct(cov_fn: SemiSeparable, tau, t, y, sigma2, with_covariance=False, ctx: Context | None = None):
    """predict_direct(cov, tau, t, y, sigma2[, with_covariance])   src/direct_solver.jl:75-119."""
    a, b, c, d = (np.real(np.atleast_1d(v)) for v in cov_fn.celerite_coefs())
    res, info = (ctx or default_context()).dense_predict(a, b, c, d, tau, t, y, sigma2, with_covariance, return_info=True)
    if info != 0:
        raise np.linalg.LinAlgError(f"matrix is not positive definite; Cholesky factorization failed at pivot {info}")
    return res


def cov(fp: PosteriorGP, tau=None, ctx: Context | None = None):
    """cov(fp[, tau])   src/scalable_GP.jl:73-78, 95-96."""
    tau = fp.f.x if tau is None else _f64(tau).reshape(-1)
    return predict_cov(fp.f.f.kernel, tau, fp.f.x, fp.f.sigma2, ctx=ctx)


def predict_var(cov_fn: SemiSeparable, tau, t, sigma2, ctx: Context | None = None):
    """diag(predict_cov(cov, tau, t, sigma2)) through the celerite factorisation: O((N + M) R^2) instead of the dense (N + M)^3
    (Dataset.predict_var; at most 64 active rows).  Raises like predict_cov when the matrix is not positive definite."""
    a, b, c, d = (np.real(np.atleast_1d(v)) for v in cov_fn.celerite_coefs())
    t = _f64(t).reshape(-1)
    ds = Dataset(t, np.zeros(len(t)), sigma2, ctx)
    try:
        v, st = ds.predict_var(a[None, :], b[None, :], c, d, _f64(tau).reshape(-1), return_status=True)
    finally:
        ds.close()
    if st[0] != 0:
        raise np.linalg.LinAlgError("matrix is not positive definite; the celerite factorisation met a non-positive pivot")
    return v[0]


def var(fp: PosteriorGP, tau=None, ctx: Context | None = None):
    """var(fp[, tau]) = diag(cov(fp, tau)), through the celerite factorisation (predict_var above)."""
    tau = fp.f.x if tau is None else _f64(tau).reshape(-1)
    return predict_var(fp.f.f.kernel, tau, fp.f.x, fp.f.sigma2, ctx=ctx)


def std(fp: PosteriorGP, tau=None, ctx: Context | None = None, solver=None):
    """std(fp[, tau]) = sqrt.(diag(cov))   src/scalable_GP.jl:103-104.  solver="celerite": the diagonal through the celerite
    factorisation (var above: O(N + M), no dense matrix; tiny negative values from rounding are clipped to zero); the default is the
    reference's dense route."""
    if solver is not None:
        if str(solver).lstrip(":") != "celerite":
            raise ValueError(f"solver {solver} not recognised, use None (dense) or 'celerite'")
        return np.sqrt(np.maximum(var(fp, tau, ctx=ctx), 0.0))
    return np.sqrt(np.diag(cov(fp, tau, ctx=ctx)))


def rand_posterior(rng, fp: PosteriorGP, tau=None, n: int = 1, ctx: Context | None = None, solver=None):
    """rand(rng, fp[, tau], N): draws from MvNormal(mean, cov)   src/scalable_GP.jl:106-129.  Returns (len(tau), n).
    solver=None: the reference's dense route (mean, dense covariance, Cholesky on the host).  solver="celerite": Matheron's rule through the
    celerite factorisation in O(N + M) per draw (Dataset.rand_posterior), exact also where tau repeats or meets a data time; `rng` then supplies
    standard_normal((n, N)), ((n, M)), ((n, N)) in this order: the latent normals at the data times, at tau, and the noise normals."""
    tau = fp.f.x if tau is None else _f64(tau).reshape(-1)
    if solver is not None:
        if str(solver).lstrip(":") != "celerite":
            raise ValueError(f"solver {solver} not recognised, use None (dense) or 'celerite'")
        x, N, M = fp.f.x, len(fp.f.x), len(tau)
        a, b, c, d = (np.real(np.atleast_1d(v)) for v in fp.f.f.kernel.celerite_coefs())
        q_data, q_new, eps = rng.standard_normal((n, N)), rng.standard_normal((n, M)), rng.standard_normal((n, N))
        ds = Dataset(x, fp.y - _mean_vector(fp.f.f.mean, x), fp.f.sigma2, ctx)
        try:
            out, st = ds.rand_posterior(np.tile(a, (n, 1)), np.tile(b, (n, 1)), c, d, tau, q_data, q_new, eps, return_status=True)
        finally:
            ds.close()
        if (st != 0).any():
            raise np.linalg.LinAlgError("matrix is not positive definite; the celerite factorisation met a non-positive pivot")
        return (out + _mean_vector(fp.f.f.mean, tau)[None, :]).T
    m, K = mean(fp, tau, ctx=ctx), cov(fp, tau, ctx=ctx)
    L = np.linalg.cholesky(K + 1e-14 * np.trace(K) / len(tau) * np.eye(len(tau)))
    return m[:, None] + L @ rng.standard_normal((len(tau), n))


def simulate(rng, cov: SemiSeparable, tau, sigma2, ctx: Context | None = None):
    """simulate(rng, cov, tau, sigma2)   src/celerite_solver.jl:497-513: one realisation; `rng` is a numpy Generator
    supplying the standard normals (the reference's randn(rng, N), :528)."""
    a, b, c, d = (np.real(np.atleast_1d(v)) for v in cov.celerite_coefs())
    tau = _f64(tau).reshape(-1)
    q = rng.standard_normal(len(tau))
    s2 = _f64(np.broadcast_to(sigma2, tau.shape))
    return (ctx or default_context()).simulate(a[None, :], b[None, :], c, d, tau, s2, q[None, :])[0]


def rand(rng, fx: "FiniteScalableGP", t=None, ctx: Context | None = None):
    """rand(rng, f(t, sigma2)) / rand(rng, f(t, sigma2), t')   src/scalable_GP.jl:137-158 (zero variance at new times)."""
    if t is None:
        return simulate(rng, fx.f.kernel, fx.x, fx.sigma2, ctx=ctx) + _mean_vector(fx.f.mean, fx.x)
    t = _f64(t).reshape(-1)
    return simulate(rng, fx.f.kernel, t, np.zeros(len(t)), ctx=ctx) + _mean_vector(fx.f.mean, t)


def logpdf(fx: FiniteScalableGP, Y, ctx: Context | None = None):
    """Distributions.logpdf(f::FiniteScalableGP, Y)   src/scalable_GP.jl:162-166."""
    Y = _f64(Y).reshape(-1)
    y = Y - _mean_vector(fx.f.mean, fx.x)
    return log_likelihood(fx.f.kernel, fx.x, y, fx.sigma2, solver=fx.f.solver, ctx=ctx)


def log_likelihood(cov: SemiSeparable, tau, y, sigma2, solver="celerite", ctx: Context | None = None):
    """log_likelihood(cov, tau, y, sigma2; solver)   src/celerite_solver.jl:262-294.
    Both solver symbols the reference accepts run the same HIP kernel (the reference's
    :celerite_matrix variant is experimental and untested, src/celerite_solver.jl:160-248)."""
    solver = str(solver).lstrip(":")
    if solver not in _SOLVERS:
        raise ValueError(f"solver {solver} not recognised, use either :celerite or :celerite_matrix")
    a, b, c, d = cov.celerite_coefs()
    a, b, c, d = (np.real(np.atleast_1d(v)) for v in (a, b, c, d))
    return logl(a, b, c, d, tau, y, sigma2, ctx=ctx)


def logl(a, b, c, d, tau, y, sigma2, ctx: Context | None = None):
    """logl(a, b, c, d, tau, y, sigma2)   src/celerite_solver.jl:312-334."""
    val, st = (ctx or default_context()).logl(a, b, c, d, tau, y, sigma2, return_status=True)
    if st == 2 and not np.isfinite(val):
        # the reference throws DomainError from log(D[1] < 0) (celerite_solver.jl:126)
        raise ValueError("log-likelihood is not finite: the covariance matrix is not positive definite")
    return val


def log_likelihood_direct(cov: SemiSeparable, t, y, sigma2, ctx: Context | None = None):
    """log_likelihood_direct(cov, t, y, sigma2): dense solver, returns the POSITIVE NLL like the
    reference (src/direct_solver.jl:19).  Raises like PosDefException when K is not PD.
    Error, measured against long-double and __float128 truths (tests/test_gpu_dense_truth.py, docs/EXPERIMENTS.md section 37) in units of
    sum |log L_nn| + z'z / 2 + N log(2 pi) / 2: below 1 eps on well-conditioned matrices (N 1..320); on near-singular ones (sigma2 / k(0) down
    to 1e-12, the ill-conditioned prior draws at N = 150 .. 3100) within 18 x the deviation LAPACK and the other fp64 references show on the same
    matrix, mostly within 3 x.  One limit: rows below a 64 x 64 diagonal block are solved by products with explicit inverses of its 16 x 16
    sub-blocks, so a row that repeats the time stamp of the block's last row, below a sub-block of condition 6e5 with sigma2 / k(0) = 1e-11,
    lost the pivot of that row to 25 % (0.24 of the scale where LAPACK loses 6e-6); the same series in another order, with both rows in one
    block, is within 4 x LAPACK's deviation."""
    a, b, c, d = (np.real(np.atleast_1d(v)) for v in cov.celerite_coefs())
    val, info = (ctx or default_context()).dense_nll(a, b, c, d, t, y, sigma2, return_info=True)
    if info != 0:
        raise np.linalg.LinAlgError(f"matrix is not positive definite; Cholesky factorization failed at pivot {info}")
    return val


def logpdf_batch(ds: Dataset, A, Bc, C, Dd, mu=None, nu=None, Y=None, S2=None, shift=None, return_status=False):
    """B independent logpdf evaluations on one data set (nested-sampling live points / MCMC walkers)."""
    return ds.logl_batch(A, Bc, C, Dd, mu=mu, nu=nu, Y=Y, S2=S2, shift=shift, return_status=return_status)


_LS_NORMALIZATIONS = ("standard", "model", "log")


def lombscargle(t, y, yerr=None, frequencies=None, fit_mean=True, center_data=True, normalization="standard", ctx: Context | None = None):
    """lombscargle(t, y, yerr, frequencies = freq) of LombScargle.jl with its defaults (generalised periodogram, fit_mean, center_data,
    :standard) as the reference's diagnostics call it (src/plots_diagnostics.jl:544,565), for one series y (N,) -> (F,) or a batch
    (B, N) -> (B, F) in one device call.  frequencies: cycles per unit time (required).  normalization: "standard" (P in [0, 1]),
    "model" (P / (1 - P)) or "log" (-log(1 - P)), the latter two formed on the host from the standard power."""
    normalization = str(normalization).lstrip(":")
    if normalization not in _LS_NORMALIZATIONS:
        raise ValueError(f"normalization {normalization!r} not supported, use one of {list(_LS_NORMALIZATIONS)}")
    if frequencies is None:
        raise ValueError("frequencies is required")
    y = _f64(y)
    if y.ndim not in (1, 2):
        raise ValueError("y must be (N,) or (B, N)")
    P = (ctx or default_context()).lombscargle(t, np.atleast_2d(y), yerr, frequencies, fit_mean=fit_mean, center_data=center_data)
    if normalization == "model":
        P = P / (1.0 - P)
    elif normalization == "log":
        P = -np.log(1.0 - P)
    return P[0] if y.ndim == 1 else P


def lsp_ppc_frequencies(t, n_frequencies=1000, S_low=20, S_high=20):
    """The frequency grid of plot_lsp_ppc (src/plots_diagnostics.jl:522-528): exp(range(log(f_min / S_low), log(f_max S_high), n_frequencies))
    with f_min = 1 / (t[end] - t[1]), f_max = 1 / min(diff(t)) / 2.  All n_frequencies points (the check drops the last, :545)."""
    t = _f64(t).reshape(-1)
    f_min, f_max = 1.0 / (t[-1] - t[0]), 1.0 / np.min(np.diff(t)) / 2.0
    return np.exp(np.linspace(np.log(f_min / S_low), np.log(f_max * S_high), int(n_frequencies)))


def lsp_ppc(rng, t, yerr, A, Bc, C, Dd, mu=None, nu=None, frequencies=None, S_low=20, S_high=20, n_frequencies=1000,
            quantiles=(0.025, 0.16, 0.5, 0.84, 0.975), ctx: Context | None = None):
    """The loop of plot_lsp_ppc (src/plots_diagnostics.jl:530-559) for B posterior draws (A, Bc: (B, J); C, Dd: (J,) or (B, J); mu, nu: (B,)
    or None) in two device calls: latent realisations at t from Context.simulate with zero variance, mu_b and sqrt(nu_b) yerr q noise added
    on the host (the simulate entry's sigma2 is shared by the draws), then the periodogram of every series with weights yerr^-2 (like the
    reference: yerr, not sqrt(nu) yerr).  rng: numpy Generator; it supplies the (B, N) latent normals first, then the (B, N) noise normals.
    Returns (frequencies[:-1], power (B, F - 1), quantiles (len(quantiles), F - 1)); the default grid is lsp_ppc_frequencies(t, ...), and the
    last point is dropped as in the reference (:545).
    The series cross the bus twice (down after the simulation, up for the periodogram: 80 MB each way at B = 1000, N = 1e4);
    Context.lombscargle_dev on series already in device memory avoids that."""
    ctx = ctx or default_context()
    t, yerr, A, Bc = _f64(t).reshape(-1), _f64(yerr).reshape(-1), _f64(A), _f64(Bc)
    B, N = A.shape[0], len(t)
    freq = lsp_ppc_frequencies(t, n_frequencies, S_low, S_high) if frequencies is None else _f64(frequencies).reshape(-1)
    freq = freq[:-1]
    Y = ctx.simulate(A, Bc, C, Dd, t, np.zeros(N), rng.standard_normal((B, N)))
    q = rng.standard_normal((B, N))
    scale = np.ones(B) if nu is None else np.sqrt(_f64(nu).reshape(-1))
    Y = Y + scale[:, None] * yerr[None, :] * q
    if mu is not None:
        Y = Y + _f64(mu).reshape(-1)[:, None]
    P = ctx.lombscargle(t, Y, yerr, freq)
    return freq, P, np.quantile(P, np.asarray(quantiles, dtype=np.float64), axis=0)


def ppc_t_pred(t, t_pred=None):
    """The prediction grid of get_ppc_timeseries (src/plots_diagnostics.jl:643-647): range(t[1], t[end], 2 N) unless given, merged with t:
    sort(unique(vcat(t, t_pred)))."""
    t = _f64(t).reshape(-1)
    t_pred = np.linspace(t[0], t[-1], 2 * len(t)) if t_pred is None else _f64(t_pred).reshape(-1)
    return np.unique(np.concatenate([t, t_pred]))


def ppc_timeseries(rng, t, y, yerr, A, Bc, C, Dd, mu=None, nu=None, shift=None, t_pred=None, ctx: Context | None = None):
    """get_ppc_timeseries (src/plots_diagnostics.jl:640-671) for B posterior samples (A, Bc: (B, J); C, Dd: (J,) or (B, J); mu, nu, shift: (B,)
    or None) in one device call: one realisation of the posterior at t_pred per row of A (Dataset.rand_posterior on the data set
    (t, y, yerr**2)).  t_pred defaults to the reference's grid and is merged with t either way (ppc_t_pred).  shift: the samples of the
    log-transform's constant c; sample b conditions on log(y - c_b) and its realisation is transformed back as the reference writes it,
    exp(realisation + c_b).  rng: numpy Generator; it supplies standard_normal((B, N)), ((B, M)), ((B, N)) in this order.
    Returns (ts_array (len(t_pred), B), t_pred)."""
    t, y, yerr, A = _f64(t).reshape(-1), _f64(y).reshape(-1), _f64(yerr).reshape(-1), _f64(A)
    B, N = A.shape[0], len(t)
    t_pred = ppc_t_pred(t, t_pred)
    M = len(t_pred)
    q_data, q_new, eps = rng.standard_normal((B, N)), rng.standard_normal((B, M)), rng.standard_normal((B, N))
    ds = Dataset(t, y, yerr ** 2, ctx)
    try:
        out = ds.rand_posterior(A, Bc, C, Dd, t_pred, q_data, q_new, eps, mu=mu, nu=nu, shift=shift)
    finally:
        ds.close()
    if shift is not None:
        out = np.exp(out + _f64(np.broadcast_to(shift, (B,)))[:, None])
    return out.T, t_pred


def quantiles(X, probs=PPC_QUANTILES, status=None, shift=None, cols=None, ref=None, scale=None, ctx: Context | None = None):
    """quantile(k, p) for k in eachrow(array), p in probs, and mean(array, dims = 2) of the reference's predictive checks
    (src/plots_diagnostics.jl:805-816, :547-559, :417-447) on the device, for an array that holds one draw per ROW: X (B, M), as
    Dataset.rand_posterior and pj.lombscargle return them (the reference's ts_array is the transpose).  The other arguments as
    Context.quantiles.  Returns (quant (Q, Mc), mean (Mc,), kept)."""
    return (ctx or default_context()).quantiles(X, probs, status=status, shift=shift, cols=cols, ref=ref, scale=scale)


def ppc_timeseries_summary(rng, t, y, yerr, A, Bc, C, Dd, mu=None, nu=None, shift=None, t_pred=None, quantiles=PPC_QUANTILES,
                           ctx: Context | None = None):
    """What plot_ppc_timeseries draws (src/plots_diagnostics.jl:805-816) without the (M, B) array of pj.ppc_timeseries leaving the device: the
    realisations of get_ppc_timeseries for the B posterior samples (arguments and use of the generator exactly as pj.ppc_timeseries:
    standard_normal((B, N)), ((B, M)), ((B, N))), back-transformed with shift as exp(realisation + c_b), reduced over the samples to
    ts_quantiles (Q, M); and the standardised residuals at the data times, (y - ts[indexes]) / yerr with indexes the positions of t in t_pred
    (:807), reduced to res_quantiles (Q, N) and mean_res (N,).  Samples whose draw failed (status 2) are left out of every reduction.
    Returns a dict with t_pred, ts_quantiles, res_quantiles, mean_res, status (B,) and kept."""
    t, y, yerr, A = _f64(t).reshape(-1), _f64(y).reshape(-1), _f64(yerr).reshape(-1), _f64(A)
    B, N = A.shape[0], len(t)
    t_pred = ppc_t_pred(t, t_pred)
    M = len(t_pred)
    q_data, q_new, eps = rng.standard_normal((B, N)), rng.standard_normal((B, M)), rng.standard_normal((B, N))
    indexes = np.searchsorted(t_pred, t)      # t_pred is sorted, distinct and holds every t
    ds = Dataset(t, y, yerr ** 2, ctx)
    try:
        r = ds.rand_posterior_summary(A, Bc, C, Dd, t_pred, q_data, q_new, eps, probs=quantiles, mu=mu, nu=nu, shift=shift,
                                      backtransform=shift is not None, res_cols=indexes, res_ref=y, res_scale=yerr)
    finally:
        ds.close()
    return dict(t_pred=t_pred, ts_quantiles=r["ts_quantiles"], res_quantiles=r["res_quantiles"], mean_res=r["res_mean"], status=r["status"],
                kept=r["kept"])


# ---- the PSD approximation checks: run_diagnostics, plot_psd_ppc, run_posterior_predict_checks as numbers ---------------------------------
_META_NAMES = ("meta_mean", "meta_median", "meta_min", "meta_max", "meta_mean_rat", "meta_median_rat", "meta_min_rat", "meta_max_rat")
_MAX_SUMMARY = 4096     # draws / frequencies of one pioran_psd_check_summary call (the quantile kernel sorts a column in one workgroup)


def _quantiles_host(X, probs, status=None):
    """(quant (Q, M), mean (M,), kept) of the rows of X with status 0, on the host, by the definition of tools/quantiles_proto.py (type 7 with
    its rule for close neighbours; the mean is the long-double sum over the kept rows): the route of the checks above 4096 draws."""
    V = np.asarray(X, dtype=np.float64)
    if status is not None:
        V = V[np.asarray(status) == 0]
    K, M = V.shape
    probs = _f64(probs).reshape(-1)
    quant = np.full((len(probs), M), np.nan)
    if K == 0:
        return quant, np.full(M, np.nan), 0
    S = np.sort(V, axis=0)
    with np.errstate(invalid="ignore", over="ignore"):
        mean = (np.sum(V.astype(np.longdouble), axis=0) / np.longdouble(K)).astype(np.float64)
        has_nan = np.isnan(S[-1])
        for q, p in enumerate(probs):
            aleph = np.float64(K) * p + (np.float64(1.0) - p)
            j = min(max(int(np.trunc(aleph)), 1), K - 1) if K > 1 else 1
            g = min(max(aleph - np.float64(j), np.float64(0.0)), np.float64(1.0))
            a, b = (S[0], S[0]) if K == 1 else (S[j - 1], S[j])
            close = np.isfinite(a) & np.isfinite(b) & (np.abs(a - b) <= np.float64(2.0 ** -26) * np.maximum(np.abs(a), np.abs(b)))
            quant[q] = np.where(has_nan, np.nan, np.where(close, a + g * (b - a), (np.float64(1.0) - g) * a + g * b))
    return quant, mean, K


def _check_grid(f0, fM, n_frequencies):
    """collect(10 .^ range(log10(f0), log10(fM), n_frequencies))   src/plots_diagnostics.jl:200"""
    return 10.0 ** np.linspace(np.log10(f0), np.log10(fM), int(n_frequencies))


def _draws_by_row(samples):
    """the reference's samples (P_params, B), one draw per COLUMN, as (B, P_params); a vector of P_params values is one draw"""
    samples = np.asarray(samples, dtype=np.float64)
    return np.ascontiguousarray(samples.reshape(-1, 1).T if samples.ndim == 1 else samples.T)


def sample_approx_model(samples, norm_samples, f0, fM, model, n_frequencies=1000, basis_function="SHO", n_components=20, ctx: Context | None = None):
    """sample_approx_model(samples, norm_samples, f0, fM, model; n_frequencies, basis_function, n_components) of src/plots_diagnostics.jl:195-213
    in one device call (Context.psd_check).  samples: (P_params, B) like the reference's, one draw per column; model: SingleBendingPowerLaw or
    DoubleBendingPowerLaw (the class).  Returns psd, psd_approx, residuals, ratios, f with the arrays (F, B) like the reference's — transposed
    VIEWS of the (B, F) arrays the device writes — and f the reference's grid 10 .^ range(log10(f0), log10(fM), n_frequencies).  A draw that
    cannot be evaluated (non-finite parameter, model not positive at f[0] or at f0) has NaN in its column."""
    theta = _draws_by_row(samples)
    f = _check_grid(f0, fM, n_frequencies)
    r = (ctx or default_context()).psd_check(model, theta, norm_samples, f, f0, fM, n_components, 1.0, 1.0, basis_function=basis_function)
    return r["psd"].T, r["psd_approx"].T, r["residuals"].T, r["ratios"].T, f


def _diagnostics_dict(f, quant_res, quant_rat, mean_res, mean_rat, meta, kept):
    out = dict(f=f, mean_res=mean_res, mean_rat=mean_rat, res_quantiles=quant_res, rat_quantiles=quant_rat, kept=kept)
    out.update({name: meta[:, k] for k, name in enumerate(_META_NAMES)})
    return out


def run_diagnostics(prior_samples, norm_samples, f_min, f_max, model, S_low=20.0, S_high=20.0, basis_function="SHO", n_components=20,
                    n_frequencies=1000, ctx: Context | None = None):
    """run_diagnostics(prior_samples, norm_samples, f_min, f_max, model, S_low, S_high; basis_function, n_components) of
    src/plots_diagnostics.jl:232-240 as numbers: the content of the three text files the reference writes.  prior_samples (P_params, B).
    Returns a dict with f (F,); mean_res, mean_rat (F,) (plot_mean_approx :150-151); res_quantiles, rat_quantiles (5, F) at PPC_QUANTILES
    (plot_quantiles_approx :93-94); meta_mean, meta_median, meta_min, meta_max, meta_mean_rat, meta_median_rat, meta_min_rat, meta_max_rat (B,)
    (plot_boxplot_psd_approx :43-51); kept: the number of draws that entered the reductions over draws (a draw that cannot be evaluated is left
    out of them and has NaN in its meta entries).
    Up to 4096 draws everything happens in one device call (Context.psd_check_summary) and only these vectors come back.  With more draws —
    or more than 4096 frequencies — the quantile kernel's limit is exceeded: the residuals and ratios are then taken from Context.psd_check
    chunk by chunk and reduced on the host with the definition of tools/quantiles_proto.py (same quantile rule; the means are long-double sums,
    so they may differ from the device's in the last bits)."""
    ctx = ctx or default_context()
    theta = _draws_by_row(prior_samples)
    f0, fM = f_min / S_low, f_max * S_high
    f = _check_grid(f0, fM, n_frequencies)
    B = theta.shape[0]
    if B <= _MAX_SUMMARY and len(f) <= _MAX_SUMMARY:
        r = ctx.psd_check_summary(model, theta, norm_samples, f, f0, fM, n_components, 1.0, 1.0, basis_function=basis_function)
        return _diagnostics_dict(f, r["quant"][2], r["quant"][3], r["mean"][2], r["mean"][3], r["meta"], r["kept"])
    r = ctx.psd_check(model, theta, norm_samples, f, f0, fM, n_components, 1.0, 1.0, basis_function=basis_function, outputs=("residuals", "ratios"))
    st = r["status"]
    meta = np.full((B, 8), np.nan)
    ok = st == 0
    red = {}
    for k, name in enumerate(("residuals", "ratios")):
        X = r[name]
        red[name] = _quantiles_host(X, PPC_QUANTILES, st)
        med, mean, _ = _quantiles_host(X[ok].T, [0.5])
        meta[ok, 4 * k], meta[ok, 4 * k + 1] = mean, med[0]
        meta[ok, 4 * k + 2], meta[ok, 4 * k + 3] = np.min(np.abs(X[ok]), axis=1), np.max(np.abs(X[ok]), axis=1)
    return _diagnostics_dict(f, red["residuals"][0], red["ratios"][0], red["residuals"][1], red["ratios"][1], meta, red["residuals"][2])


def psd_ppc(samples_psd, samples_norm, samples_nu, t, y, yerr, model, S_low=20.0, S_high=20.0, plot_f_P=False, n_frequencies=1000, n_components=20,
            basis_function="SHO", is_integrated_power=True, with_log_transform=False, ctx: Context | None = None):
    """plot_psd_ppc(samples_psd, samples_norm, samples_nu, t, y, yerr, model; ...) of src/plots_diagnostics.jl:371-487 as numbers.  samples_psd
    (B, P_params), one posterior sample per row, as the reference takes them here.  Returns a dict with f (F,); psd_quantiles,
    psd_approx_quantiles (5, F) at PPC_QUANTILES of the model PSD and of its approximation, both divided by get_norm_psd (:404-409) and, with
    plot_f_P, multiplied by f (:419-420); mean_noise_level, median_noise_level (:379-397, host scalars; multiply by f yourself with plot_f_P as
    :435-436 do); f_min, f_max of the data; kept.
    Up to 4096 samples: one device call (Context.psd_check_summary).  With more — a nested-sampling posterior routinely has more equal-weight
    samples, and the reference uses all of them — the two arrays are taken from Context.psd_check chunk by chunk and reduced on the host with
    the definition of tools/quantiles_proto.py."""
    ctx = ctx or default_context()
    t, y, yerr = _f64(t).reshape(-1), _f64(y).reshape(-1), _f64(yerr).reshape(-1)
    theta = _f64(np.atleast_2d(samples_psd))
    dt = np.diff(t)
    f_min, f_max = 1.0 / (t[-1] - t[0]), 1.0 / np.min(dt) / 2.0
    f0, fM = f_min / S_low, f_max * S_high
    sq_err = (yerr / y) ** 2 if with_log_transform else yerr ** 2
    nu = _f64(samples_nu).reshape(-1)
    mean_noise_level = 2.0 * np.mean(nu) * np.mean(sq_err) * np.mean(dt)
    median_noise_level = 2.0 * np.median(nu) * np.median(sq_err) * np.median(dt)
    f = _check_grid(f0, fM, n_frequencies)
    kw = dict(basis_function=basis_function, is_integrated_power=is_integrated_power, normalise=True, times_f=plot_f_P)
    if theta.shape[0] <= _MAX_SUMMARY and len(f) <= _MAX_SUMMARY:
        r = ctx.psd_check_summary(model, theta, samples_norm, f, f_min, f_max, n_components, S_low, S_high, mean=False, meta=False, **kw)
        q_psd, q_approx, kept = r["quant"][0], r["quant"][1], r["kept"]
    else:
        r = ctx.psd_check(model, theta, samples_norm, f, f_min, f_max, n_components, S_low, S_high, outputs=("psd", "psd_approx"), **kw)
        q_psd, _, kept = _quantiles_host(r["psd"], PPC_QUANTILES, r["status"])
        q_approx, _, _ = _quantiles_host(r["psd_approx"], PPC_QUANTILES, r["status"])
    return dict(f=f, psd_quantiles=q_psd, psd_approx_quantiles=q_approx, mean_noise_level=mean_noise_level, median_noise_level=median_noise_level,
                f_min=f_min, f_max=f_max, kept=kept)


def psd_ppc_carma(samples_r_alpha, samples_beta, samples_norm, samples_nu, t, y, yerr, p, q, plot_f_P=False, n_frequencies=1000,
                  with_log_transform=False, ctx: Context | None = None):
    """plot_psd_ppc_CARMA(samples_r_alpha, samples_beta, samples_norm, samples_nu, t, y, yerr, p, q; ...) of src/plots_diagnostics.jl:832-936 as
    numbers.  samples_r_alpha (B, p) complex, samples_beta (B, q + 1), one posterior sample per row.  Returns a dict with f (F,), the reference's
    grid exp.(range(log(f_min / 10), log(10 f_max))) around the observed window f_min = 1 / T, f_max = 1 / (2 min dt); psd_quantiles (5, F) at
    PPC_QUANTILES of evaluate(CARMA(p, q, r_alpha, beta, norm), f), multiplied by f with plot_f_P; mean_noise_level, median_noise_level (host
    scalars; multiply by f yourself with plot_f_P as the reference's lines do); f_min, f_max of the grid; kept.
    Up to 4096 samples: one device call (Context.carma_psd_summary); with more, the array comes from Context.carma_psd chunk by chunk and is
    reduced on the host with the definition of tools/quantiles_proto.py."""
    r = np.asarray(samples_r_alpha, dtype=complex)
    be = np.asarray(samples_beta, dtype=np.float64)
    r, be = (r.reshape(1, -1) if r.ndim == 1 else r), (be.reshape(1, -1) if be.ndim == 1 else be)
    if p != r.shape[1]:
        raise ValueError(f"p={p} is not equal to the number of columns in samples_rα={r.shape[1]}")
    if q + 1 != be.shape[1]:
        raise ValueError(f"q+1={q + 1} is not equal to the number of columns in samples_β={be.shape[1]}")
    t, y, yerr = _f64(t).reshape(-1), _f64(y).reshape(-1), _f64(yerr).reshape(-1)
    dt = np.diff(t)
    f_min, f_max = 1.0 / (t[-1] - t[0]) / 10.0, 1.0 / np.min(dt) / 2.0 * 10.0
    f = np.exp(np.linspace(np.log(f_min), np.log(f_max), int(n_frequencies)))
    sq_err = (yerr / y) ** 2 if with_log_transform else yerr ** 2
    nu = _f64(samples_nu).reshape(-1)
    mean_noise_level = 2.0 * np.mean(nu) * np.mean(sq_err) * np.mean(dt)
    median_noise_level = 2.0 * np.median(nu) * np.median(sq_err) * np.median(dt)
    norm = _f64(samples_norm).reshape(-1)
    ctx = ctx or default_context()
    if r.shape[0] <= _MAX_SUMMARY:
        s = ctx.carma_psd_summary(p, q, f, r_alpha=r, beta=be, norm=norm, times_f=plot_f_P)
        q_psd, kept = s["quant"], s["kept"]
    else:
        psd, st = ctx.carma_psd(p, q, f, r_alpha=r, beta=be, norm=norm, times_f=plot_f_P, return_status=True)
        q_psd, _, kept = _quantiles_host(psd, PPC_QUANTILES, st)
    return dict(f=f, psd_quantiles=q_psd, mean_noise_level=mean_noise_level, median_noise_level=median_noise_level, f_min=f_min, f_max=f_max, kept=kept)


def posterior_predict_checks(rng, samples_psd, samples_norm, samples_nu, samples_mu, samples_c, t, y, yerr, model, with_log_transform=False,
                             S_low=20.0, S_high=20.0, is_integrated_power=True, plots="all", basis_function="SHO", n_frequencies=1000, plot_f_P=False,
                             n_components=20, ctx: Context | None = None):
    """run_posterior_predict_checks (src/plots_diagnostics.jl:276-344) for the models that go through `approx`, as numbers: the three checks in
    the reference's order (:282-307) — pj.psd_ppc, pj.lsp_ppc, pj.ppc_timeseries_summary — on the posterior samples samples_psd (B, P_params),
    samples_norm, samples_nu, samples_mu (B,) or None, and samples_c (B,), the log-transform's constant, used when with_log_transform.  The
    celerite coefficients of the second and third check come from psd.approx_batch.  plots: "all", or a list among "psd", "lsp", "timeseries"
    (:310-341).  rng: numpy Generator, consumed by the periodogram check first, then by the time-series check.
    Returns {"psd": ..., "lsp": ..., "timeseries": ...} with the selected keys, each value what the single call returns for the same generator state."""
    from .psd import approx_batch
    want = ("psd", "lsp", "timeseries") if isinstance(plots, str) and plots == "all" else tuple(plots)
    if any(w not in ("psd", "lsp", "timeseries") for w in want):
        raise ValueError('plots must be "all" or a list among "psd", "lsp", "timeseries"')
    t, y, yerr = _f64(t).reshape(-1), _f64(y).reshape(-1), _f64(yerr).reshape(-1)
    out = {}
    if "psd" in want:
        out["psd"] = psd_ppc(samples_psd, samples_norm, samples_nu, t, y, yerr, model, S_low=S_low, S_high=S_high, plot_f_P=plot_f_P,
                             n_frequencies=n_frequencies, n_components=n_components, basis_function=basis_function,
                             is_integrated_power=is_integrated_power, with_log_transform=with_log_transform, ctx=ctx)
    if "lsp" in want or "timeseries" in want:
        f_min, f_max = 1.0 / (t[-1] - t[0]), 1.0 / np.min(np.diff(t)) / 2.0
        A, Bc, C, Dd = approx_batch(model, samples_psd, f_min, f_max, n_components, samples_norm, S_low, S_high,
                                    is_integrated_power=is_integrated_power, basis_function=basis_function)
        if "lsp" in want:
            out["lsp"] = lsp_ppc(rng, t, yerr, A, Bc, C, Dd, mu=samples_mu, nu=samples_nu, S_low=S_low, S_high=S_high, n_frequencies=n_frequencies, ctx=ctx)
        if "timeseries" in want:
            out["timeseries"] = ppc_timeseries_summary(rng, t, y, yerr, A, Bc, C, Dd, mu=samples_mu, nu=samples_nu,
                                                       shift=samples_c if with_log_transform else None, ctx=ctx)
    return out
