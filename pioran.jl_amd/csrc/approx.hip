// approx on the device: theta -> (a_j, b_j) of the SumOfCelerite kernel, fused in front of the scan.
//
// Restates, per draw, src/psd.jl:214-289 (approx) for a continuum-only PSD model:
//   spectral grid f_j = f0 (fM/f0)^(j/(J-1)),  f0 = f_min/S_low, fM = f_max*S_high          :217-218,77-79
//   p_j = P(f_j) / P(f_0)                                   get_normalised_psd             :52-56
//   amplitudes = B \ p,  B_jk = 1 / (1 + (f_j/f_k)^{4|6})  build_approx / psd_decomp      :73-112
//   integ = analytic integral over [f_min, f_max] (integral_sho / integral_drwcelerite) or
//           the variance form                              get_norm_psd                   :301-324,375-395
//   SHO:          a = b = A_j f_j pi / sqrt2                                               :249-252
//   DRWCelerite:  a = A_j f_j pi / 3, b = sqrt3 a  ++  (a, 0)                             :264-275
// PSD features (QPO, src/psd.jl:15-27, 228-241, 254-261): n_qpo Lorentzians (S0, f0, Q) per draw become one celerite term each,
//   a = S0 w0 Q / 4, b = a / Delta, c = w0 / (2 Q), d = c Delta (Delta = sqrt(4 Q^2 - 1), w0 = 2 pi f0), a and b divided by the
// continuum's P(f_0) like the amplitudes, their integral (integrate_psd_feature :356-358) added to the normalisation when
// is_integrated_power, and appended as (2a, 2b, c, d) after the continuum terms; their (c, d) differ per draw.
// c_j, d_j of the continuum depend only on the grid and stay on the host side of the ABI (pioran_dataset_prepare).
// PSD models are Tonari.jl's closed forms (test/test_psd.jl:3-13).  The J x J matrix B is LU-factorised once
// on the host (partial pivoting, like Julia's `\`); each draw is one thread doing 2 J^2 flops of triangular
// solves in its own output row.  Cost ~ J (2 pow + log + atan2) + 2 J^2 flop per draw: microseconds per batch.
// The model's closed forms, the solve and the continuum's normalising integral are psd_device.h's, shared with psd_check.hip.
// The reverse modes, one thread per draw as well: approx_vjp_kernel (continuum) and approx_qpo_vjp_kernel (with features), closed forms in their comments.
#include "common.h"
#include "psd_device.h"

#include <cmath>
#include <vector>

namespace {

__global__ void __launch_bounds__(64) approx_kernel(int64_t B, int model, int P, int J, int basis, int integrated,
                                                    double f_min, double f_max, const double* __restrict__ sp,
                                                    const double* __restrict__ LU, const int32_t* __restrict__ piv,
                                                    const double* __restrict__ theta, const double* __restrict__ norm,
                                                    int n_qpo, const double* __restrict__ qpo, double* __restrict__ A,
                                                    double* __restrict__ Bc, double* __restrict__ Cq, double* __restrict__ Dq)
{
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int Jc = basis == 0 ? J : 2 * J;       // celerite terms of the continuum
    const int Jt = Jc + n_qpo;                   // + one per feature
    double* x = A + b * Jt;                      // work in place in the output row (first J entries)
    const double* th = theta + b * P;
    const double p0 = psd_model(model, th, sp[0]);
    psd_normalised_on_grid(model, th, J, sp, p0, x, 1);
    psd_lu_solve(J, LU, piv, x, 1);
    // normalisation (src/psd.jl:375-395)
    double integ = psd_norm_integral(J, basis, integrated, f_min, f_max, sp, x, 1);
    if (integrated) {
        // features: integral of the celerite power spectrum between f_min and f_max   (src/psd.jl:330-334, 356-358)
        for (int q = 0; q < n_qpo; ++q) {
            const double S0 = qpo[(b * n_qpo + q) * 3], f0q = qpo[(b * n_qpo + q) * 3 + 1], Q = qpo[(b * n_qpo + q) * 3 + 2];
            const double De = sqrt(4.0 * Q * Q - 1.0), w0 = 2.0 * M_PI * f0q;
            const double fa = S0 * w0 * Q / 4.0 / p0, fb = fa / De, fc = w0 / Q / 2.0, fd = fc * De;
            auto icel = [&](double xx) {
                const double num = fc * fc + (fd + 2.0 * M_PI * xx) * (fd + 2.0 * M_PI * xx);
                const double den = fc * fc + (fd - 2.0 * M_PI * xx) * (fd - 2.0 * M_PI * xx);
                return (2.0 * fa * (atan2(fc, fd - 2.0 * M_PI * xx) - atan2(fc, fd + 2.0 * M_PI * xx)) + fb * log(num / den)) / (2.0 * M_PI);
            };
            integ += icel(f_max) - icel(f_min);
        }
    }
    const double scale = norm[b] / integ;
    double* bb = Bc + b * Jt;
    for (int q = 0; q < n_qpo; ++q) {            // (2a, 2b, c, d) of the feature terms   (:254-261, 276-283)
        const double S0 = qpo[(b * n_qpo + q) * 3], f0q = qpo[(b * n_qpo + q) * 3 + 1], Q = qpo[(b * n_qpo + q) * 3 + 2];
        const double De = sqrt(4.0 * Q * Q - 1.0), w0 = 2.0 * M_PI * f0q;
        const double fa = S0 * w0 * Q / 4.0 / p0 * scale, fc = w0 / Q / 2.0;
        x[Jc + q] = 2.0 * fa;
        bb[Jc + q] = 2.0 * (fa / De);
        Cq[b * Jt + Jc + q] = fc;
        Dq[b * Jt + Jc + q] = fc * De;
    }
    if (basis == 0) {
        for (int j = 0; j < J; ++j) {
            const double a = x[j] * scale * sp[j] * M_PI / 1.4142135623730951;
            x[j] = a;
            bb[j] = a;
        }
    } else {
        for (int j = 0; j < J; ++j) {
            const double a = x[j] * scale * sp[j] * M_PI / 3.0;
            x[j] = a;
            x[J + j] = a;
            bb[j] = 1.7320508075688772 * a;
            bb[J + j] = 0.0;
        }
    }
}

// P(f) of psd_model and its logarithmic derivatives dl[k] = d log P(f) / d theta_k, from the pow values the value needs and one log per bend:
//   x = f / f1, u = x^(a2 - a1), q = u / (1 + u):   d/da1 = -log x / (1 + u),  d/df1 = (a1 + q (a2 - a1)) / f1,  d/da2 = -q log x
//   y = f / f2, v = y^(a3 - a2), r = v / (1 + v):   d/da2 += r log y,  d/df2 = r (a3 - a2) / f2,  d/da3 = -r log y
// (q, r -> 1 where the pow overflows: P is 0 there, the derivative of its logarithm is not)
__device__ __forceinline__ double psd_model_dlog(int model, const double* th, double f, double dl[5])
{
    const double x = f / th[1], lx = log(x);
    const double u = pow(x, th[2] - th[0]);
    const double q = isinf(u) ? 1.0 : u / (1.0 + u);
    double v = pow(x, -th[0]) / (1.0 + u);
    dl[0] = -lx * (1.0 - q);
    dl[1] = (th[0] + q * (th[2] - th[0])) / th[1];
    dl[2] = -q * lx;
    dl[3] = dl[4] = 0.0;
    if (model == 1) {
        const double ly = log(f / th[3]);
        const double w = pow(f / th[3], th[4] - th[2]);
        const double r = isinf(w) ? 1.0 : w / (1.0 + w);
        v /= 1.0 + w;
        dl[2] += r * ly;
        dl[3] = r * (th[4] - th[2]) / th[3];
        dl[4] = -r * ly;
    }
    return v;
}

// xb <- B^-T xb with P B = L U (psd_lu_solve's factors):  U' y = xbar (forward), L' z = y (backward, unit diagonal), pbar = P' z
__device__ __forceinline__ void psd_lu_solve_transposed(int J, const double* __restrict__ LU, const int32_t* __restrict__ piv, double* xb, int64_t B)
{
    for (int i = 0; i < J; ++i) {
        double acc = xb[(int64_t)i * B];
        for (int k = 0; k < i; ++k) acc = fma(-LU[k * J + i], xb[(int64_t)k * B], acc);
        xb[(int64_t)i * B] = acc / LU[i * J + i];
    }
    for (int i = J - 2; i >= 0; --i) {
        double acc = xb[(int64_t)i * B];
        for (int k = i + 1; k < J; ++k) acc = fma(-LU[k * J + i], xb[(int64_t)k * B], acc);
        xb[(int64_t)i * B] = acc;
    }
    // the row interchanges undone in reverse order.  The sparse grids have none; dense ones do (f_max / f_min = 1e3, S_low = S_high = 20: SHO from
    // J = 48 on, DRWCelerite from J = 72 on — tools/approx_vjp_proto.py interchanges(); the tests run both)
    for (int j = J - 1; j >= 0; --j) {
        const int pj = piv[j];
        if (pj != j) { const double tmp = xb[(int64_t)j * B]; xb[(int64_t)j * B] = xb[(int64_t)pj * B]; xb[(int64_t)pj * B] = tmp; }
    }
}

// g_k += sum_j pbar_j p_j (dlog P(f_j)/dtheta_k - dlog P(f_0)/dtheta_k): the pullback of p_j = P(f_j) / P(f_0) (d0: psd_model_dlog at f_0)
__device__ __forceinline__ void psd_theta_pullback(int model, const double* th, int J, const double* __restrict__ sp, double p0, const double d0[5],
                                                   const double* pbar, int64_t B, double g[5])
{
    double dj[5];
    for (int j = 0; j < J; ++j) {
        const double pj = psd_model_dlog(model, th, sp[j], dj) / p0;
        const double t = pbar[(int64_t)j * B] * pj;
#pragma unroll
        for (int k = 0; k < 5; ++k) g[k] = fma(t, dj[k] - d0[k], g[k]);
    }
}

// Reverse mode of approx_kernel for the continuum models: (grad_a, grad_b) [B][Jt] -> grad_theta [B][P], grad_norm [B].  With x = B^-1 p the
// amplitudes, I = w'x the normalising integral (w: pioran_approx_weights_host) and kappa_j x_j norm / I the coefficients, sum(ga a + gb b) is
// (norm / I) h'x with h_j = kappa_j (ga_j + gb_j) (SHO) or kappa_j (ga_j + ga_{J+j} + sqrt3 gb_j) (DRWCelerite; the b of its second half is
// structurally 0), so
//   grad_norm = h'x / I,    xbar = (norm / I) h - (norm / I^2) (h'x) w,    pbar = B^-T xbar,
//   grad_theta_k = sum_j pbar_j p_j (dlog P(f_j)/dtheta_k - dlog P(f_0)/dtheta_k).
// The forward quantities are recomputed (nothing is kept between approx_kernel and this one).  One thread per draw as in approx_kernel: the LU
// entries are uniform over a wavefront (scalar loads), each draw's x and xbar sit in `scratch` [2 J][B] so that a wavefront's accesses to one
// entry are one coalesced line.  No operation mixes draws: a draw's result does not depend on its place in the batch.
__global__ void __launch_bounds__(64) approx_vjp_kernel(int64_t B, int model, int P, int J, int basis, int64_t Jt,
                                                        const double* __restrict__ sp, const double* __restrict__ w,
                                                        const double* __restrict__ LU, const int32_t* __restrict__ piv,
                                                        const double* __restrict__ theta, const double* __restrict__ norm,
                                                        const double* __restrict__ ga, const double* __restrict__ gb,
                                                        double* __restrict__ scratch, double* __restrict__ gtheta, double* __restrict__ gnorm)
{
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double* x = scratch + b;                         // x[j * B]
    double* xb = scratch + (int64_t)J * B + b;       // xbar[j * B]
    const double* th = theta + b * P;
    double d0[5];
    const double p0 = psd_model_dlog(model, th, sp[0], d0);
    // forward: p, then x = B^-1 p (as approx_kernel)
    psd_normalised_on_grid(model, th, J, sp, p0, x, B);
    psd_lu_solve(J, LU, piv, x, B);
    // h, I = w'x, h'x
    const double* gar = ga + b * Jt;
    const double* gbr = gb + b * Jt;
    const double kap = basis == 0 ? M_PI / 1.4142135623730951 : M_PI / 3.0;
    double integ = 0.0, hx = 0.0;
    for (int j = 0; j < J; ++j) {
        const double g = basis == 0 ? gar[j] + gbr[j] : gar[j] + gar[J + j] + 1.7320508075688772 * gbr[j];
        const double h = kap * sp[j] * g, xj = x[(int64_t)j * B];
        integ = fma(w[j], xj, integ);
        hx = fma(h, xj, hx);
        xb[(int64_t)j * B] = h;
    }
    const double s = norm[b] / integ, cw = s * hx / integ;
    gnorm[b] = hx / integ;
    for (int j = 0; j < J; ++j) xb[(int64_t)j * B] = s * xb[(int64_t)j * B] - cw * w[j];
    psd_lu_solve_transposed(J, LU, piv, xb, B);
    double g[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    psd_theta_pullback(model, th, J, sp, p0, d0, xb, B, g);
#pragma unroll
    for (int k = 0; k < 5; ++k)
        if (k < P) gtheta[b * P + k] = g[k];
}

// The two brackets of integral_celerite (src/psd.jl:330-334) at the frequency f per unit (a, b), with u+- = d +- 2 pi f:
//   ia = (atan2(c, u-) - atan2(c, u+)) / pi,    ib = log((c^2 + u+^2) / (c^2 + u-^2)) / (2 pi),
// and their derivatives.  They form a Cauchy-Riemann pair:
//   d ia / dc = (u- / (c^2 + u-^2) - u+ / (c^2 + u+^2)) / pi = -d ib / dd,    d ia / dd = c (1 / (c^2 + u+^2) - 1 / (c^2 + u-^2)) / pi = d ib / dc.
// c > 0, so atan2 stays on one branch whatever the sign of u-.
__device__ __forceinline__ void qpo_brackets(double c, double d, double f, double sign, double& ia, double& ib, double& ia_c, double& ia_d)
{
    const double up = d + 2.0 * M_PI * f, um = d - 2.0 * M_PI * f;
    const double num = c * c + up * up, den = c * c + um * um;
    ia += sign * (atan2(c, um) - atan2(c, up)) / M_PI;
    ib += sign * log(num / den) / (2.0 * M_PI);
    ia_c += sign * (um / den - up / num) / M_PI;
    ia_d += sign * c * (1.0 / num - 1.0 / den) / M_PI;
}

// Reverse mode of approx_kernel with n_qpo >= 1 features: cotangents (ga, gb, gc, gd) [B][Jt], Jt = Jc + n_qpo, of the coefficients ->
// grad_theta [B][P], grad_norm [B], grad_qpo [B][n_qpo][3] = d/d(S0, f0, Q).  Of gc, gd only the feature columns are read: the continuum's (c, d)
// are the grid's.  Forward, per draw, with p0 = P(f_0; theta), x = B^-1 p, and per feature w0 = 2 pi f0, De = sqrt(4 Q^2 - 1), al = S0 w0 Q / 4:
//   fa = al / p0,  fb = fa / De,  c = w0 / (2 Q),  d = c De,
//   I = w'x + [integrated] sum_q (fa_q Ia_q + fb_q Ib_q),     Ia, Ib: qpo_brackets at f_max minus at f_min,
//   a_j = kappa_j x_j norm / I (b_j as in approx_vjp_kernel),   A_q = 2 fa_q norm / I,  B_q = 2 fb_q norm / I,  C_q = c_q,  D_q = d_q.
// Reverse, with h as in approx_vjp_kernel, s = norm / I and T = h'x + sum_q 2 (ga_q fa_q + gb_q fb_q), so that sum(ga a + gb b) = s T:
//   grad_norm = T / I,    Ibar = -s T / I,    xbar = s h + Ibar w,    pbar = B^-T xbar,
//   fabar_q = 2 s ga_q + [i] Ibar Ia_q,    fbbar_q = 2 s gb_q + [i] Ibar Ib_q,
//   cbar_q = gc_q + [i] Ibar (fa_q dIa/dc + fb_q dIb/dc),    dbar_q = gd_q + [i] Ibar (fa_q dIa/dd + fb_q dIb/dd),
//   through fb = fa / De and d = c De:   fabar += fbbar / De,   Debar = -fbbar fb / De + dbar c,   cbar += dbar De,
//   albar = fabar / p0,
//   grad_S0 = albar w0 Q / 4,   grad_f0 = 2 pi (albar S0 Q / 4 + cbar / (2 Q)),   grad_Q = albar S0 w0 / 4 - cbar c / Q + Debar 4 Q / De,
//   grad_theta_k = sum_j pbar_j p_j (dlog P(f_j)/dtheta_k - dlog P(f_0)/dtheta_k) - (sum_q fabar_q fa_q) dlog P(f_0)/dtheta_k
// (the last term: theta acts on the features through 1 / p0; through I it acts by xbar and, for the features' share of I, by fabar).
// In the variance form ([i] = 0) the features do not enter I but are still scaled by s.  One thread per draw, the scratch [2 J][B] and the uniform
// LU loads as in approx_vjp_kernel; a feature's forward values are recomputed in the second pass instead of being kept.  No operation mixes draws.
__global__ void __launch_bounds__(64) approx_qpo_vjp_kernel(int64_t B, int model, int P, int J, int basis, int integrated, int n_qpo, double f_min,
                                                            double f_max, const double* __restrict__ sp, const double* __restrict__ w,
                                                            const double* __restrict__ LU, const int32_t* __restrict__ piv,
                                                            const double* __restrict__ theta, const double* __restrict__ norm,
                                                            const double* __restrict__ qpo, const double* __restrict__ ga, const double* __restrict__ gb,
                                                            const double* __restrict__ gc, const double* __restrict__ gd, double* __restrict__ scratch,
                                                            double* __restrict__ gtheta, double* __restrict__ gnorm, double* __restrict__ gqpo)
{
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double* x = scratch + b;                         // x[j * B]
    double* xb = scratch + (int64_t)J * B + b;       // xbar[j * B]
    const double* th = theta + b * P;
    double d0[5];
    const double p0 = psd_model_dlog(model, th, sp[0], d0);
    psd_normalised_on_grid(model, th, J, sp, p0, x, B);
    psd_lu_solve(J, LU, piv, x, B);
    const int Jc = basis == 0 ? J : 2 * J;
    const int64_t Jt = Jc + n_qpo;
    const double *gar = ga + b * Jt, *gbr = gb + b * Jt, *gcr = gc + b * Jt, *gdr = gd + b * Jt;
    const double kap = basis == 0 ? M_PI / 1.4142135623730951 : M_PI / 3.0;
    double integ = 0.0, T = 0.0;
    for (int j = 0; j < J; ++j) {
        const double g = basis == 0 ? gar[j] + gbr[j] : gar[j] + gar[J + j] + 1.7320508075688772 * gbr[j];
        const double h = kap * sp[j] * g, xj = x[(int64_t)j * B];
        integ = fma(w[j], xj, integ);
        T = fma(h, xj, T);
        xb[(int64_t)j * B] = h;
    }
    const double* qp = qpo + b * n_qpo * 3;
    for (int q = 0; q < n_qpo; ++q) {                // the features' share of I and of T
        const double S0 = qp[3 * q], f0q = qp[3 * q + 1], Q = qp[3 * q + 2];
        const double De = sqrt(4.0 * Q * Q - 1.0), w0 = 2.0 * M_PI * f0q;
        const double fa = S0 * w0 * Q / 4.0 / p0, fb = fa / De, fc = w0 / Q / 2.0, fd = fc * De;
        T += 2.0 * (gar[Jc + q] * fa + gbr[Jc + q] * fb);
        if (integrated) {
            double ia = 0.0, ib = 0.0, ia_c = 0.0, ia_d = 0.0;
            qpo_brackets(fc, fd, f_max, 1.0, ia, ib, ia_c, ia_d);
            qpo_brackets(fc, fd, f_min, -1.0, ia, ib, ia_c, ia_d);
            integ += fa * ia + fb * ib;
        }
    }
    const double s = norm[b] / integ, cw = s * T / integ;   // cw = -Ibar
    gnorm[b] = T / integ;
    for (int j = 0; j < J; ++j) xb[(int64_t)j * B] = s * xb[(int64_t)j * B] - cw * w[j];
    double fsum = 0.0;                               // sum_q fabar_q fa_q
    for (int q = 0; q < n_qpo; ++q) {
        const double S0 = qp[3 * q], f0q = qp[3 * q + 1], Q = qp[3 * q + 2];
        const double De = sqrt(4.0 * Q * Q - 1.0), w0 = 2.0 * M_PI * f0q;
        const double fa = S0 * w0 * Q / 4.0 / p0, fb = fa / De, fc = w0 / Q / 2.0, fd = fc * De;
        double fab = 2.0 * s * gar[Jc + q], fbb = 2.0 * s * gbr[Jc + q], cb = gcr[Jc + q], db = gdr[Jc + q];
        if (integrated) {
            double ia = 0.0, ib = 0.0, ia_c = 0.0, ia_d = 0.0;
            qpo_brackets(fc, fd, f_max, 1.0, ia, ib, ia_c, ia_d);
            qpo_brackets(fc, fd, f_min, -1.0, ia, ib, ia_c, ia_d);
            fab -= cw * ia;
            fbb -= cw * ib;
            cb -= cw * (fa * ia_c + fb * ia_d);      // d ib / dc = d ia / dd
            db -= cw * (fa * ia_d - fb * ia_c);      // d ib / dd = -d ia / dc
        }
        fab += fbb / De;
        const double Deb = db * fc - fbb * fb / De;
        cb += db * De;
        fsum += fab * fa;
        const double alb = fab / p0;
        double* gq = gqpo + (b * n_qpo + q) * 3;
        gq[0] = alb * w0 * Q / 4.0;
        gq[1] = 2.0 * M_PI * (alb * S0 * Q / 4.0 + cb / (2.0 * Q));
        gq[2] = alb * S0 * w0 / 4.0 - cb * fc / Q + Deb * 4.0 * Q / De;
    }
    psd_lu_solve_transposed(J, LU, piv, xb, B);
    double g[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) g[k] = -fsum * d0[k];
    psd_theta_pullback(model, th, J, sp, p0, d0, xb, B, g);
#pragma unroll
    for (int k = 0; k < 5; ++k)
        if (k < P) gtheta[b * P + k] = g[k];
}

}  // namespace

// Host side: the spectral grid, its LU factorisation and the (c, d) that go with it.
int pioran_approx_setup_host(int64_t J, int basis, double f_min, double f_max, double S_low, double S_high,
                             std::vector<double>& sp, std::vector<double>& LU, std::vector<int32_t>& piv,
                             std::vector<double>& c, std::vector<double>& d, std::vector<int32_t>& real_term)
{
    if (J < 2 || J > 256 || !(f_min > 0.0) || !(f_max > f_min)) return PIORAN_ERR_ARG;
    const double f0 = f_min / S_low, fM = f_max * S_high;
    sp.resize(J);
    for (int64_t j = 0; j < J; ++j) sp[j] = f0 * std::pow(fM / f0, (double)j / (double)(J - 1));   // :77-79
    const double pw = basis == 0 ? 4.0 : 6.0;
    LU.assign(J * J, 0.0);
    for (int64_t j = 0; j < J; ++j)
        for (int64_t k = 0; k < J; ++k) LU[j * J + k] = 1.0 / (1.0 + std::pow(sp[j] / sp[k], pw));   // :82-96
    piv.resize(J);
    for (int64_t k = 0; k < J; ++k) {   // LU with partial pivoting (dgetrf, as Julia's `\` on a square matrix)
        int64_t p = k;
        double best = std::fabs(LU[k * J + k]);
        for (int64_t i = k + 1; i < J; ++i)
            if (std::fabs(LU[i * J + k]) > best) { best = std::fabs(LU[i * J + k]); p = i; }
        if (best == 0.0) return PIORAN_ERR_ARG;
        piv[k] = (int32_t)p;
        if (p != k)
            for (int64_t q = 0; q < J; ++q) std::swap(LU[k * J + q], LU[p * J + q]);
        for (int64_t i = k + 1; i < J; ++i) {
            const double l = LU[i * J + k] / LU[k * J + k];
            LU[i * J + k] = l;
            for (int64_t q = k + 1; q < J; ++q) LU[i * J + q] -= l * LU[k * J + q];
        }
    }
    if (basis == 0) {       // :250
        c.resize(J); d.resize(J); real_term.assign(J, 0);
        for (int64_t j = 0; j < J; ++j) c[j] = d[j] = std::sqrt(2.0) * M_PI * sp[j];
    } else {                // :266-273
        c.resize(2 * J); d.resize(2 * J); real_term.assign(2 * J, 0);
        for (int64_t j = 0; j < J; ++j) {
            c[j] = M_PI * sp[j];
            d[j] = std::sqrt(3.0) * c[j];
            c[J + j] = 2.0 * c[j];
            d[J + j] = 0.0;
            real_term[J + j] = 1;
        }
    }
    return PIORAN_OK;
}

int pioran_launch_approx(int64_t B, int model, int P, int J, int basis, int integrated, double f_min, double f_max,
                         const double* sp, const double* LU, const int32_t* piv, const double* theta, const double* norm,
                         int n_qpo, const double* qpo, double* A, double* Bc, double* Cq, double* Dq, hipStream_t stream)
{
    const int64_t blocks = (B + 63) / 64;
    if (blocks <= 0 || blocks > 0x7fffffffLL) return PIORAN_ERR_ARG;
    if (n_qpo > 0 && (!qpo || !Cq || !Dq)) return PIORAN_ERR_ARG;
    hipLaunchKernelGGL(approx_kernel, dim3((unsigned)blocks), dim3(64), 0, stream, B, model, P, J, basis, integrated, f_min,
                       f_max, sp, LU, piv, theta, norm, n_qpo, qpo, A, Bc, Cq, Dq);
    return hipGetLastError() == hipSuccess ? PIORAN_OK : PIORAN_ERR_HIP;
}

// w_j of the normalising integral I = sum_j w_j x_j over the amplitudes x (get_norm_psd, src/psd.jl:375-395; the terms approx_kernel adds up):
// the bracket of integral_sho / integral_drwcelerite between f_min and f_max per unit amplitude, or the variance form's f_j pi / sqrt2, 2 pi f_j / 3.
// They depend on the grid alone: once per call on the host, like the LU factors.
void pioran_approx_weights_host(int basis, int integrated, double f_min, double f_max, const std::vector<double>& sp, std::vector<double>& w)
{
    const double s2 = std::sqrt(2.0), s3 = std::sqrt(3.0);
    w.resize(sp.size());
    for (size_t j = 0; j < sp.size(); ++j) {
        const double c = sp[j];
        if (!integrated) { w[j] = basis == 0 ? c * M_PI / s2 : c * 2.0 * M_PI / 3.0; continue; }
        if (c <= 0.5 * f_min) { w[j] = psd_band_tail(c, f_min, f_max, basis == 0 ? 4 : 6); continue; }   // far below the band: no cancellation
        auto sho = [&](double f) {
            const double ph = (f * f + s2 * c * f + c * c) / (f * f - s2 * c * f + c * c);
            return c / (4.0 * s2) * (std::log(ph) + 2.0 * std::atan2(c * s2 * f, c * c - f * f));
        };
        auto drw = [&](double f) {
            const double ph = (f * f + s3 * c * f + c * c) / (f * f - s3 * c * f + c * c);
            return c / 3.0 * (std::atan(f / c) + 0.5 * std::atan2(f * f - c * c, c * f) + s3 / 4.0 * std::log(ph));
        };
        w[j] = basis == 0 ? sho(f_max) - sho(f_min) : drw(f_max) - drw(f_min);
    }
}

int pioran_launch_approx_vjp(int64_t B, int model, int P, int J, int basis, const double* sp, const double* w, const double* LU,
                             const int32_t* piv, const double* theta, const double* norm, const double* ga, const double* gb,
                             double* scratch, double* gtheta, double* gnorm, hipStream_t stream)
{
    const int64_t blocks = (B + 63) / 64;
    if (blocks <= 0 || blocks > 0x7fffffffLL || J < 2 || J > 256 || model < 0 || model > 1 || P != (model == 0 ? 3 : 5)) return PIORAN_ERR_ARG;
    hipLaunchKernelGGL(approx_vjp_kernel, dim3((unsigned)blocks), dim3(64), 0, stream, B, model, P, J, basis, (int64_t)(basis == 0 ? J : 2 * J),
                       sp, w, LU, piv, theta, norm, ga, gb, scratch, gtheta, gnorm);
    return hipGetLastError() == hipSuccess ? PIORAN_OK : PIORAN_ERR_HIP;
}

int pioran_launch_approx_qpo_vjp(int64_t B, int model, int P, int J, int basis, int integrated, double f_min, double f_max, const double* sp,
                                 const double* w, const double* LU, const int32_t* piv, const double* theta, const double* norm, int n_qpo,
                                 const double* qpo, const double* ga, const double* gb, const double* gc, const double* gd, double* scratch,
                                 double* gtheta, double* gnorm, double* gqpo, hipStream_t stream)
{
    const int64_t blocks = (B + 63) / 64;
    if (blocks <= 0 || blocks > 0x7fffffffLL || J < 2 || J > 256 || model < 0 || model > 1 || P != (model == 0 ? 3 : 5) || basis < 0 || basis > 1)
        return PIORAN_ERR_ARG;
    if (n_qpo < 1 || n_qpo > 8 || !qpo || !ga || !gb || !gc || !gd || !scratch || !gtheta || !gnorm || !gqpo) return PIORAN_ERR_ARG;
    hipLaunchKernelGGL(approx_qpo_vjp_kernel, dim3((unsigned)blocks), dim3(64), 0, stream, B, model, P, J, basis, integrated != 0, n_qpo, f_min, f_max,
                       sp, w, LU, piv, theta, norm, qpo, ga, gb, gc, gd, scratch, gtheta, gnorm, gqpo);
    return hipGetLastError() == hipSuccess ? PIORAN_OK : PIORAN_ERR_HIP;
}
