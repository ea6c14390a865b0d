"""Host side of the CARMA(p, q) models — the reference's helpers around `CARMA` with their semantics:

  quad2roots, roots2coeffs                     src/CARMA.jl:175-223
  CARMA_normalisation, evaluate(::CARMA, f)    src/CARMA.jl:150-172, 279-304
  sample_quad                                  src/CARMA.jl:308-407 (a numpy Generator for the reference's AbstractRNG)
  check_conjugate_pair, check_roots_bounds, check_order_imag_roots     src/utils.jl:160-210

The batched device entries are Context.carma_coefs / carma_vjp / carma_psd / carma_psd_summary and Dataset.logpdf_carma / logpdf_carma_grad
(gp.py); these functions are one draw on the host, for setting models up and for checking.
"""
from __future__ import annotations

import numpy as np


def quad2roots(quad):
    """Roots of the polynomial given by its quadratic factors: quad[k], quad[k + 1] = (c, b) of x^2 + b x + c, for odd length the last entry is
    the factor x + quad[-1].  Pairs with a negative discriminant give a conjugate pair (positive imaginary part first), others two real roots."""
    quad = np.asarray(quad, dtype=float)
    n = len(quad)
    r = np.zeros(n, dtype=complex)
    n_ = n
    if n % 2 == 1:
        r[-1] = -quad[-1]
        n_ = n - 1
    for k in range(0, n_, 2):
        b, c = quad[k + 1], quad[k]
        delta = b ** 2 - 4 * c
        if delta < 0:
            r[k] = (-b + 1j * np.sqrt(-delta)) / 2
            r[k + 1] = np.conj(r[k])
        else:
            r[k] = (-b + np.sqrt(delta)) / 2
            r[k + 1] = (-b - np.sqrt(delta)) / 2
    return r


def roots2coeffs(r):
    """Coefficients, ascending and monic, of the polynomial with roots r (Polynomials.fromroots(r).coeffs); complex like the reference's."""
    c = np.ones(1, dtype=complex)
    for root in np.asarray(r, dtype=complex):
        nxt = np.zeros(len(c) + 1, dtype=complex)
        nxt[1:] = c
        nxt[:-1] -= root * c
        c = nxt
    return c


def CARMA_normalisation(r_alpha, beta=None):
    """CARMA_normalisation(r_alpha, beta) or CARMA_normalisation(covariance::CARMA): the variance of the process with norm 1 up to the factor 2 that
    `evaluate` carries (src/CARMA.jl:279-304)."""
    if beta is None:
        r_alpha, beta = r_alpha.r_alpha, r_alpha.beta
    r_alpha = np.asarray(r_alpha, dtype=complex)
    beta = np.asarray(beta, dtype=float)
    powers = np.arange(len(beta))
    variance = 0.0
    for rk in r_alpha:
        num = (beta * rk ** powers).sum() * (beta * (-rk) ** powers).sum()
        den = -2 * rk.real
        for rj in r_alpha[r_alpha != rk]:
            den = den * ((rj - rk) * (np.conj(rj) + rk))
        variance = variance + num / den
    return float(np.real(variance))


def evaluate(model, f):
    """evaluate(model::CARMA, f): the power spectral density at the frequencies f (src/CARMA.jl:150-172)."""
    f = np.atleast_1d(np.asarray(f, dtype=float))
    wi = 2 * np.pi * f * 1j
    alpha = roots2coeffs(model.r_alpha)
    num = sum(model.beta[i] * wi ** i for i in range(model.q + 1))
    den = sum(alpha[j] * wi ** j for j in range(model.p + 1))
    if model.is_integrated_power:
        return 2 * np.abs(num / den) ** 2 * model.norm / CARMA_normalisation(model)
    return 4 * np.abs(num / den) ** 2 * model.norm


def _log_uniform(rng, lo, hi):
    return float(np.exp(rng.uniform(np.log(lo), np.log(hi))))


def _sample_quad_one(n, rng, f_min, f_max):
    quad = np.empty(n)
    if n % 2 == 1:
        quad[-1] = _log_uniform(rng, f_min, f_max)
    n_ = n - n % 2
    for i in range(1, n_, 2):                      # the linear coefficients of the pairs first
        quad[i] = _log_uniform(rng, 2 * f_min, 2 * f_max)
    buff = 0.0
    for j, i in enumerate(range(0, n_, 2)):        # then the constant ones: f0 + b^2 / 4, f0 ascending from pair to pair
        if j == 0:
            buff = quad[i + 1] ** 2 / 4
            quad[i] = _log_uniform(rng, f_min, f_max) + buff
        else:
            start_log = quad[i - 2] - buff
            buff = quad[i + 1] ** 2 / 4
            quad[i] = _log_uniform(rng, start_log, f_max) + buff
    return quad


def sample_quad(p, q, rng, f_min, f_max):
    """sample_quad(p, q, rng, f_min, f_max): quadratic factors (qa [p], qb [q]) whose roots are conjugate pairs within the bounds, ordered by
    magnitude (src/CARMA.jl:328-407).  rng: numpy Generator; the draws come in the reference's order (an odd order's last factor, the pairs'
    linear coefficients, then their constant ones; qa before qb)."""
    return _sample_quad_one(int(p), rng, float(f_min), float(f_max)), _sample_quad_one(int(q), rng, float(f_min), float(f_max))


def check_conjugate_pair(r):
    """True if the roots are complex-conjugate pairs (for an odd number the last one is left alone) with no positive real part."""
    r = np.asarray(r, dtype=complex)
    if np.any(r.real > 0):
        return False
    n = len(r)
    for i in range(0, n - n % 2, 2):
        if r[i] != np.conj(r[i + 1]):
            return False
    return True


def check_roots_bounds(r, f_min, f_max):
    """True if -f_max < Re r < -f_min and -f_max < Im r < f_max for every root."""
    r = np.asarray(r, dtype=complex)
    return bool(np.all((-f_max < r.real) & (r.real < -f_min)) and np.all((-f_max < r.imag) & (r.imag < f_max)))


def check_order_imag_roots(r):
    """True if the imaginary parts of the first roots of the pairs are in ascending order."""
    r = np.asarray(r, dtype=complex)
    n = len(r)
    im = r[0:n - n % 2:2].imag
    return bool(np.array_equal(np.argsort(im, kind="stable"), np.arange(len(im))))
