// Device code that approx.hip (theta -> celerite coefficients) and psd_check.hip (model against approximation) share: the PSD model's closed
// forms, the amplitudes x = B^-1 p through the host's LU factors, and the normalising integral of get_norm_psd over the continuum's amplitudes.
// A draw's vector x is addressed as x[j * stride]: stride 1 where a thread works in its own output row, the batch size where a wavefront's
// accesses to one entry are to be one line.  Every item keeps internal linkage, so each translation unit compiles its own copy.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

namespace {

__device__ __forceinline__ double psd_model(int model, const double* th, double f)
{
    // 0: SingleBendingPowerLaw(alpha1, f1, alpha2); 1: DoubleBendingPowerLaw(alpha1, f1, alpha2, f2, alpha3)
    const double x = f / th[1];
    double v = pow(x, -th[0]) / (1.0 + pow(x, th[2] - th[0]));
    if (model == 1) v /= 1.0 + pow(f / th[3], th[4] - th[2]);
    return v;
}

// p_j = P(f_j) / p0 on the spectral grid (get_normalised_psd, src/psd.jl:52-56)
__device__ __forceinline__ void psd_normalised_on_grid(int model, const double* th, int J, const double* __restrict__ sp, double p0, double* x,
                                                       int64_t stride)
{
    for (int j = 0; j < J; ++j) x[(int64_t)j * stride] = psd_model(model, th, sp[j]) / p0;
}

// x <- B^-1 x with P B = L U from pioran_approx_setup_host: row interchanges, then L y = P p (unit lower), U x = y   (psd_decomp, src/psd.jl:109-112)
__device__ __forceinline__ void psd_lu_solve(int J, const double* __restrict__ LU, const int32_t* __restrict__ piv, double* x, int64_t stride)
{
    for (int j = 0; j < J; ++j) {
        const int pj = piv[j];
        if (pj != j) { const double tmp = x[(int64_t)j * stride]; x[(int64_t)j * stride] = x[(int64_t)pj * stride]; x[(int64_t)pj * stride] = tmp; }
    }
    for (int i = 1; i < J; ++i) {
        double acc = x[(int64_t)i * stride];
        for (int k = 0; k < i; ++k) acc = fma(-LU[i * J + k], x[(int64_t)k * stride], acc);
        x[(int64_t)i * stride] = acc;
    }
    for (int i = J - 1; i >= 0; --i) {
        double acc = x[(int64_t)i * stride];
        for (int k = i + 1; k < J; ++k) acc = fma(-LU[i * J + k], x[(int64_t)k * stride], acc);
        x[(int64_t)i * stride] = acc / LU[i * J + i];
    }
}

// The band integral of one basis function per unit amplitude, int_{f_min}^{f_max} df / (1 + (f / c)^p) (p = 4 SHO, 6 DRWCelerite), for a term far
// below the band, c <= f_min / 2.  There the closed forms below give it as the difference of two primitives of size c that agree to
// (c / f_min)^(p - 1) — seven digits at c = f_min / 20, p = 6 — so it is summed instead as the series in t = c / f, which has no cancellation:
//   c sum_k (-1)^k (th^n_k - tl^n_k) / n_k,   n_k = p (k + 1) - 1,   th = c / f_min <= 1/2,   tl = c / f_max;   16 terms: th^(16 p) < 1e-19.
// pioran_approx_weights_host (approx.hip) and the host mirror (psd.py _band_tail) form the same sum.
#define PIORAN_PSD_TAIL_TERMS 16
__host__ __device__ inline double psd_band_tail(double c, double f_min, double f_max, int p)
{
    const double th = c / f_min, tl = c / f_max;
    double thp = th * th, tlp = tl * tl;
    thp = p == 4 ? thp * thp : thp * thp * thp;
    tlp = p == 4 ? tlp * tlp : tlp * tlp * tlp;
    double uh = thp / th, ul = tlp / tl, sum = 0.0, sign = 1.0;
    for (int k = 0; k < PIORAN_PSD_TAIL_TERMS; ++k) {
        sum += sign * (uh - ul) / (double)(p * (k + 1) - 1);
        uh *= thp; ul *= tlp; sign = -sign;
    }
    return c * sum;
}

// get_norm_psd over the amplitudes of the continuum (src/psd.jl:375-395): the analytic integral over [f_min, f_max] (integral_sho :301-305,
// integral_drwcelerite :318-324; terms with c <= f_min / 2 by psd_band_tail) or the variance form
__device__ __forceinline__ double psd_norm_integral(int J, int basis, int integrated, double f_min, double f_max, const double* __restrict__ sp,
                                                    const double* x, int64_t stride)
{
    if (!integrated) {
        double acc = 0.0;
        for (int j = 0; j < J; ++j) acc += x[(int64_t)j * stride] * sp[j];
        return basis == 0 ? acc * M_PI / 1.4142135623730951 : acc * 2.0 * M_PI / 3.0;
    }
    double hi = 0.0, lo = 0.0, tail = 0.0;      // tail: the terms far below the band (psd_band_tail)
    if (basis == 0) {            // integral_sho :301-305
        const double s2 = 1.4142135623730951;
        for (int j = 0; j < J; ++j) {
            if (sp[j] <= 0.5 * f_min) { tail = fma(x[(int64_t)j * stride], psd_band_tail(sp[j], f_min, f_max, 4), tail); continue; }
            const double c = sp[j], nrm = c * x[(int64_t)j * stride] / (4.0 * s2);
            const double ph = (f_max * f_max + s2 * c * f_max + c * c) / (f_max * f_max - s2 * c * f_max + c * c);
            const double pl = (f_min * f_min + s2 * c * f_min + c * c) / (f_min * f_min - s2 * c * f_min + c * c);
            hi += nrm * (log(ph) + 2.0 * atan2(c * s2 * f_max, c * c - f_max * f_max));
            lo += nrm * (log(pl) + 2.0 * atan2(c * s2 * f_min, c * c - f_min * f_min));
        }
    } else {                     // integral_drwcelerite :318-324
        const double s3 = 1.7320508075688772;
        for (int j = 0; j < J; ++j) {
            if (sp[j] <= 0.5 * f_min) { tail = fma(x[(int64_t)j * stride], psd_band_tail(sp[j], f_min, f_max, 6), tail); continue; }
            const double c = sp[j], nrm = x[(int64_t)j * stride] * c / 3.0;
            const double ph = (f_max * f_max + s3 * c * f_max + c * c) / (f_max * f_max - s3 * c * f_max + c * c);
            const double pl = (f_min * f_min + s3 * c * f_min + c * c) / (f_min * f_min - s3 * c * f_min + c * c);
            hi += nrm * (atan(f_max / c) + 0.5 * atan2(f_max * f_max - c * c, c * f_max) + s3 / 4.0 * log(ph));
            lo += nrm * (atan(f_min / c) + 0.5 * atan2(f_min * f_min - c * c, c * f_min) + s3 / 4.0 * log(pl));
        }
    }
    return (hi - lo) + tail;
}

}  // namespace
