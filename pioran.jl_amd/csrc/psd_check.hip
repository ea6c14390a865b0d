// The PSD model against its basis-function approximation for a batch of draws: what sample_approx_model (src/plots_diagnostics.jl:195-213), the
// prior check run_diagnostics (:232-240) and the posterior check plot_psd_ppc (:371-487) evaluate draw by draw on the host.  The definition,
// operation by operation, is tools/psd_check_proto.py.  Continuum models only (the two bending power laws of psd_device.h); QPO features and PowerLaw
// are not covered.  (plot_psd_ppc_CARMA: carma.hip.)
//
//   psd_check_draw_kernel   one thread per draw, as approx_kernel: amplitudes amp = B^-1 p (the first half of approx_kernel, the same device code:
//       psd_device.h), the normalising integral of get_norm_psd, the model at the first frequency passed, and the draw's status.
//   psd_check_eval_kernel   a workgroup of four wavefronts owns a tile of 32 draws x 64 frequencies.  A wavefront takes 8 of the draws one after the
//       other with its lanes along the frequency axis: what belongs to the draw (theta, norm, amplitudes) is uniform over the wavefront and comes
//       through the scalar cache into scalar registers, the frequency of a lane stays in a vector register, the spectral points are read from LDS (one
//       address per wavefront: a broadcast).  Stores into the [B][F] arrays are 512-byte runs of a row per wavefront.  The transposed copies
//       [F][ldT] of residuals and ratios go through an LDS tile (rows padded to 65 doubles: the column reads of a half wavefront fall on 32
//       different bank pairs) and leave as 256-byte runs.  min |.| and max |.| over a draw's frequencies: a wavefront reduces its 64 lanes by
//       lane exchanges and writes one partial per (draw, frequency tile); psd_check_meta_kernel combines a draw's partials in tile order — min
//       and max are exact and order-free, no atomics.
//       Every output array may be absent; what is not asked for is neither computed nor stored, and what is asked for does not depend on
//       what else is (no contraction in this file: every operation below is rounded on its own, as the twin's).
//   psd_check_meta_kernel   one thread per draw: meta [B][8] = mean, median, min |.|, max |.| of the residuals, then of the ratios
//       (plot_boxplot_psd_approx :43-51, :72), mean and median taken from the quantile kernel's reduction of the transposed copies.
// Cost at B = 2000, F = 1000, J = 20: 4e7 terms of two divisions and four multiplications, 4e6 model values of two pow — the divisions and
// the pow bound the evaluation kernel, not memory (64 MB of stores with all four arrays and both copies).
#include "common.h"
#include "psd_device.h"

#include <cmath>

#pragma clang fp contract(off)

namespace {

constexpr int PC_TD = 32;        // draws of a tile
constexpr int PC_TF = 64;        // frequencies of a tile: one per lane
constexpr int PC_THREADS = 256;
constexpr int PC_MAXJ = 256;

__global__ void __launch_bounds__(64) psd_check_draw_kernel(int64_t B, int model, int P, int J, int basis, int integrated, int normalise,
                                                            double f_min, double f_max, const double* __restrict__ sp,
                                                            const double* __restrict__ LU, const int32_t* __restrict__ piv,
                                                            const double* __restrict__ theta, const double* __restrict__ norm,
                                                            const double* __restrict__ freq, double* __restrict__ amp,
                                                            double* __restrict__ integ, double* __restrict__ pf0, int32_t* __restrict__ status)
{
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double* x = amp + b * J;                     // work in place in the output row
    const double* th = theta + b * P;
    const double p0 = psd_model(model, th, sp[0]);
    psd_normalised_on_grid(model, th, J, sp, p0, x, 1);
    psd_lu_solve(J, LU, piv, x, 1);
    const double I = psd_norm_integral(J, basis, integrated, f_min, f_max, sp, x, 1);
    const double q0 = psd_model(model, th, freq[0]);   // the normaliser of the model PSD is the model at the FIRST frequency passed (:204), not sp[0]
    bool ok = isfinite(norm[b]);
    for (int k = 0; k < P; ++k) ok = ok && isfinite(th[k]);
    ok = ok && p0 > 0.0 && isfinite(p0) && q0 > 0.0 && isfinite(q0);
    if (normalise) ok = ok && I != 0.0 && isfinite(I);
    status[b] = ok ? 0 : 2;
    if (!ok)
        for (int j = 0; j < J; ++j) x[j] = NAN;
    integ[b] = ok ? I : NAN;
    pf0[b] = ok ? q0 : NAN;
}

// min and max that keep a NaN (numpy's): the reductions of a row that holds one are NaN
__device__ __forceinline__ double nan_min(double a, double b) { return (a != a || b != b) ? NAN : (a < b ? a : b); }
__device__ __forceinline__ double nan_max(double a, double b) { return (a != a || b != b) ? NAN : (a > b ? a : b); }

template <class Op>
__device__ __forceinline__ double wave_reduce(double v, Op op)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v = op(v, __shfl_xor(v, d, 64));
    return v;
}

__global__ void __launch_bounds__(PC_THREADS) psd_check_eval_kernel(PsdCheckEval p)
{
    __shared__ double s_sp[PC_MAXJ];
    __shared__ double tile[2][PC_TD][PC_TF + 1];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t b0 = (int64_t)blockIdx.x * PC_TD, f0 = (int64_t)blockIdx.y * PC_TF;
    const int64_t f = f0 + lane;
    const bool fin = f < p.F;
    const double* __restrict__ theta = p.theta;
    const double* __restrict__ norm = p.norm;
    const double* __restrict__ amp = p.amp;
    const double* __restrict__ integ = p.integ;
    const double* __restrict__ pf0 = p.pf0;
    const int32_t* __restrict__ status = p.status;
    const int J = p.J, P = p.P;
    const bool transposed = p.resT || p.ratT;
    const bool both = p.res || p.rat || transposed || p.part;          // residuals or ratios in any form
    const bool need_model = p.psd || both, need_approx = p.approx || both;

    for (int j = tid; j < J; j += PC_THREADS) s_sp[j] = p.sp[j];
    const double fr = fin ? p.freq[f] : 1.0;
    __syncthreads();

    constexpr int per_wave = PC_TD / (PC_THREADS / 64);
    for (int i = 0; i < per_wave; ++i) {
        const int d = wave * per_wave + i;
        const int64_t b = b0 + d;                // uniform over the wavefront
        if (b >= p.B) continue;
        double vp = NAN, va = NAN, vr = NAN, vq = NAN;
        if (status[b] == 0) {
            const double nb = norm[b];
            if (need_model) vp = psd_model(p.model, theta + b * P, fr) / pf0[b] * nb;                  // :202-205
            if (need_approx) {                                                                          // :207, src/psd.jl:171-179
                const double* a = amp + b * J;
                double acc = 0.0;
                for (int j = 0; j < J; ++j) {
                    const double r = fr / s_sp[j], r2 = r * r, r4 = r2 * r2;
                    const double pw = p.basis == 0 ? r4 : r4 * r2;
                    acc += (a[j] * nb) / (1.0 + pw);
                }
                va = acc;
            }
            if (p.normalise) {                                                                          // :408-409
                const double I = integ[b];
                vp = vp / I;
                va = va / I;
            }
            if (p.times_f) {                                                                            // :419-420
                vp = vp * fr;
                va = va * fr;
            }
            vr = vp - va;                                                                               // :210-211
            vq = va / vp;
        }
        if (fin) {
            const int64_t at = b * p.F + f;
            if (p.psd) p.psd[at] = vp;
            if (p.approx) p.approx[at] = va;
            if (p.res) p.res[at] = vr;
            if (p.rat) p.rat[at] = vq;
        }
        if (transposed) {
            tile[0][d][lane] = vr;
            tile[1][d][lane] = vq;
        }
        if (p.part) {
            const double inf = INFINITY;
            const double ar = fabs(vr), aq = fabs(vq);
            const double mnr = wave_reduce(fin ? ar : inf, nan_min), mxr = wave_reduce(fin ? ar : -inf, nan_max);
            const double mnq = wave_reduce(fin ? aq : inf, nan_min), mxq = wave_reduce(fin ? aq : -inf, nan_max);
            if (lane == 0) {
                double* o = p.part + (b * p.npart + blockIdx.y) * 4;
                o[0] = mnr; o[1] = mxr; o[2] = mnq; o[3] = mxq;
            }
        }
    }
    if (!transposed) return;                     // uniform over the grid
    __syncthreads();
    const int d = tid & (PC_TD - 1);
    const int64_t b = b0 + d;
    for (int k = 0; k < PC_TF / (PC_THREADS / PC_TD); ++k) {
        const int fl = (tid / PC_TD) + (PC_THREADS / PC_TD) * k;
        const int64_t ff = f0 + fl;
        if (b < p.B && ff < p.F) {
            if (p.resT) p.resT[ff * p.ldT + b] = tile[0][d][fl];
            if (p.ratT) p.ratT[ff * p.ldT + b] = tile[1][d][fl];
        }
    }
}

__global__ void __launch_bounds__(64) psd_check_meta_kernel(int64_t B, int64_t npart, const double* __restrict__ part,
                                                            const int32_t* __restrict__ status, const double* __restrict__ med_res,
                                                            const double* __restrict__ mean_res, const double* __restrict__ med_rat,
                                                            const double* __restrict__ mean_rat, double* __restrict__ meta)
{
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double* m = meta + b * 8;
    if (status[b] != 0) {
        for (int k = 0; k < 8; ++k) m[k] = NAN;
        return;
    }
    const double* q = part + b * npart * 4;
    double mnr = q[0], mxr = q[1], mnq = q[2], mxq = q[3];
    for (int64_t t = 1; t < npart; ++t) {
        mnr = nan_min(mnr, q[t * 4]);
        mxr = nan_max(mxr, q[t * 4 + 1]);
        mnq = nan_min(mnq, q[t * 4 + 2]);
        mxq = nan_max(mxq, q[t * 4 + 3]);
    }
    m[0] = mean_res[b]; m[1] = med_res[b]; m[2] = mnr; m[3] = mxr;
    m[4] = mean_rat[b]; m[5] = med_rat[b]; m[6] = mnq; m[7] = mxq;
}

}  // namespace

int64_t pioran_psd_check_ftiles(int64_t F) { return (F + PC_TF - 1) / PC_TF; }

// amp [B][J], integ [B], pf0 [B] (the model at freq[0]) and status [B] of the draws theta [B][P], norm [B]; every pointer on the device
int pioran_launch_psd_check_draws(int64_t B, int model, int P, int J, int basis, int integrated, int normalise, double f_min, double f_max,
                                  const double* sp, const double* LU, const int32_t* piv, const double* theta, const double* norm, const double* freq,
                                  double* amp, double* integ, double* pf0, int32_t* status, hipStream_t stream)
{
    const int64_t blocks = (B + 63) / 64;
    if (blocks <= 0 || blocks > 0x7fffffffLL || J < 2 || J > PC_MAXJ || model < 0 || model > 1 || P != (model == 0 ? 3 : 5) || basis < 0 || basis > 1)
        return PIORAN_ERR_ARG;
    hipLaunchKernelGGL(psd_check_draw_kernel, dim3((unsigned)blocks), dim3(64), 0, stream, B, model, P, J, basis, integrated, normalise, f_min, f_max, sp,
                       LU, piv, theta, norm, freq, amp, integ, pf0, status);
    return hipGetLastError() == hipSuccess ? PIORAN_OK : PIORAN_ERR_HIP;
}

int pioran_launch_psd_check_eval(const PsdCheckEval& p, hipStream_t stream)
{
    if (p.B < 1 || p.F < 1 || p.J < 2 || p.J > PC_MAXJ || p.P != (p.model == 0 ? 3 : 5) || (p.part && p.npart != pioran_psd_check_ftiles(p.F)) ||
        ((p.resT || p.ratT) && p.ldT < p.B))
        return PIORAN_ERR_ARG;
    const int64_t bx = (p.B + PC_TD - 1) / PC_TD, by = pioran_psd_check_ftiles(p.F);
    if (bx > 0x7fffffffLL || by > 65535) return PIORAN_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(psd_check_eval_kernel, dim3((unsigned)bx, (unsigned)by), dim3(PC_THREADS), 0, stream, p);
    return hipGetLastError() == hipSuccess ? PIORAN_OK : PIORAN_ERR_HIP;
}

int pioran_launch_psd_check_meta(int64_t B, int64_t npart, const double* part, const int32_t* status, const double* med_res, const double* mean_res,
                                 const double* med_rat, const double* mean_rat, double* meta, hipStream_t stream)
{
    const int64_t blocks = (B + 63) / 64;
    if (blocks <= 0 || blocks > 0x7fffffffLL || npart < 1) return PIORAN_ERR_ARG;
    hipLaunchKernelGGL(psd_check_meta_kernel, dim3((unsigned)blocks), dim3(64), 0, stream, B, npart, part, status, med_res, mean_res, med_rat, mean_rat,
                       meta);
    return hipGetLastError() == hipSuccess ? PIORAN_OK : PIORAN_ERR_HIP;
}
