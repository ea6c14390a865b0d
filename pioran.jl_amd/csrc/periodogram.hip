// Batched generalised Lomb-Scargle periodogram (Zechmeister & Kuerster 2009, time-shift-free form) — what the reference's posterior
// predictive check evaluates once per simulated series (plot_lsp_ppc, src/plots_diagnostics.jl:514-571, through LombScargle.jl).
//
// The weights and the trigonometric factors depend on (t, yerr, freq) only, so all draws share them; per draw and frequency the work is the
// pair of projections  sum_n w_n y~_bn cos(w_f t_n),  sum_n w_n y~_bn sin(w_f t_n):  one [B x N].[N x 2F] fp64 matrix product.
//   ls_weights_kernel   w_n = yerr_n^-2 / sum yerr^-2 (or 1/N), one workgroup, fixed reduction order
//   ls_table_kernel     G[n][2f] = w_n cos, G[n][2f+1] = w_n sin for a chunk of frequencies, rows padded with zeros to the product's K tile;
//                       partial sums of (C, S, C^, CS^) per block of rows; ls_freq_kernel adds the partials in a fixed order (no atomics)
//   ls_series_kernel    one workgroup per draw: weighted mean, then sum w y~, sum w y~^2, status
//   ls_product_kernel   the product on v_mfma_f64_16x16x4_f64 with the row mean subtracted as the series tile goes to LDS; its epilogue
//                       turns each (Y C^, Y S^) pair into the power, so only [B][F] doubles go to memory
#include "common.h"

#include <cmath>

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int LS_BK = 16;          // K tile of the product: four k-steps of the 16x16x4 instruction
constexpr int LS_ROWS = 64;        // rows of one partial sum of the table kernel
constexpr int LS_THREADS = 256;
constexpr int LS_TF = 64;          // frequencies per workgroup of the table kernel = granularity of a frequency chunk (2 LS_TF columns: one 128-wide tile)

// sum over the workgroup (256 threads) in a fixed order; every thread receives it
__device__ __forceinline__ double block_sum(double v, double* red)
{
    const int tid = threadIdx.x;
    __syncthreads();   // red may still be read from the previous call
    red[tid] = v;
    __syncthreads();
#pragma unroll
    for (int s = LS_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    return red[0];
}

__global__ __launch_bounds__(LS_THREADS) void ls_weights_kernel(int64_t N, const double* __restrict__ yerr, double* __restrict__ w)
{
    __shared__ double red[LS_THREADS];
    if (!yerr) {
        for (int64_t n = threadIdx.x; n < N; n += LS_THREADS) w[n] = 1.0 / (double)N;
        return;
    }
    double s = 0.0;
    for (int64_t n = threadIdx.x; n < N; n += LS_THREADS) s += 1.0 / (yerr[n] * yerr[n]);
    const double tot = block_sum(s, red);
    for (int64_t n = threadIdx.x; n < N; n += LS_THREADS) w[n] = 1.0 / (yerr[n] * yerr[n]) / tot;
}

// (cos, sin)(2 pi f t) with the phase formed in cycles and reduced exactly: p = f t rounded, e its rounding error, r = p - rint(p) is exact,
// so the argument's error does not grow with |f t|
__device__ __forceinline__ void cycle_sincos(double f, double t, double* s, double* c)
{
    const double p = f * t;
    const double e = fma(f, t, -p);
    const double r = p - rint(p);
    sincospi(2.0 * (r + e), s, c);
}

// grid (Npad / LS_ROWS, Fpad / LS_TF) — the long dimension on x, the frequency blocks (at most 16384, pioran_ls_max_fchunk) on y: thread = one frequency, LS_ROWS consecutive rows.  G is [Npad][2 Fpad]; part is [Npad / LS_ROWS][4][Fpad].
__global__ __launch_bounds__(LS_TF) void ls_table_kernel(int64_t N, int64_t Fc, int64_t Fpad, const double* __restrict__ t,
                                                              const double* __restrict__ w, const double* __restrict__ freq,
                                                              double* __restrict__ G, double* __restrict__ part)
{
    const int64_t f = (int64_t)blockIdx.y * LS_TF + threadIdx.x;   // < Fpad: the grid covers Fpad exactly
    const int64_t n0 = (int64_t)blockIdx.x * LS_ROWS;
    const bool live = f < Fc;
    const double fr = live ? freq[f] : 0.0;
    double sc = 0.0, ss = 0.0, scc = 0.0, scs = 0.0;
    for (int i = 0; i < LS_ROWS; ++i) {
        const int64_t n = n0 + i;
        double2 g = make_double2(0.0, 0.0);
        if (live && n < N) {
            double s, c;
            cycle_sincos(fr, t[n], &s, &c);
            const double wn = w[n];
            g = make_double2(wn * c, wn * s);
            sc += g.x;
            ss += g.y;
            scc = fma(g.x, c, scc);
            scs = fma(g.x, s, scs);
        }
        *reinterpret_cast<double2*>(G + (n * Fpad + f) * 2) = g;
    }
    double* p = part + (int64_t)blockIdx.x * 4 * Fpad + f;
    p[0] = sc;
    p[Fpad] = ss;
    p[2 * Fpad] = scc;
    p[3 * Fpad] = scs;
}

// fq [6][Fpad]: C, S (zero without fit_mean), CC, SS, CS, D (NaN where D <= 0 or not finite: the column is NaN)
__global__ __launch_bounds__(LS_THREADS) void ls_freq_kernel(int64_t nblk, int64_t Fc, int64_t Fpad, int fit_mean, const double* __restrict__ part,
                                                             double* __restrict__ fq)
{
    const int64_t f = (int64_t)blockIdx.x * LS_THREADS + threadIdx.x;
    if (f >= Fpad) return;
    double C = 0.0, S = 0.0, Ch = 0.0, CSh = 0.0;
    for (int64_t k = 0; k < nblk; ++k) {
        const double* p = part + k * 4 * Fpad + f;
        C += p[0];
        S += p[Fpad];
        Ch += p[2 * Fpad];
        CSh += p[3 * Fpad];
    }
    if (!fit_mean) C = S = 0.0;
    const double CC = Ch - C * C, SS = (1.0 - Ch) - S * S, CS = CSh - C * S;
    double D = CC * SS - CS * CS;
    if (!(D > 0.0) || !isfinite(D) || f >= Fc) D = NAN;
    fq[f] = C;
    fq[Fpad + f] = S;
    fq[2 * Fpad + f] = CC;
    fq[3 * Fpad + f] = SS;
    fq[4 * Fpad + f] = CS;
    fq[5 * Fpad + f] = D;
}

// dr [3][B]: what the loader subtracts from the series, Y = sum w y~ (zero without fit_mean), YY (NaN for a flagged draw).
// A draw is flagged (status 2) for a non-finite value or a series that is constant to rounding: YY <= 1e-28 sum w y^2.
__global__ __launch_bounds__(LS_THREADS) void ls_series_kernel(int64_t N, int64_t B, const double* __restrict__ Y, const double* __restrict__ w,
                                                               int fit_mean, int center, double* __restrict__ dr, int32_t* __restrict__ status)
{
    __shared__ double red[LS_THREADS];
    const int64_t b = blockIdx.x;
    const double* y = Y + b * N;
    double m = 0.0, q = 0.0;
    for (int64_t n = threadIdx.x; n < N; n += LS_THREADS) {
        m = fma(w[n], y[n], m);
        q = fma(w[n] * y[n], y[n], q);
    }
    const double mean = block_sum(m, red);
    const double raw2 = block_sum(q, red);
    // with a fitted mean the power does not depend on a constant added to the series (YC, YS and YY are invariant), so the weighted mean is taken off
    // whether or not the caller asked for centring: YC = Y C^ - Y C of a series with an offset loses what the offset costs (1.7e-9 at 1000)
    const double sub = (center || fit_mean) ? mean : 0.0;
    double s1 = 0.0, s2 = 0.0;
    for (int64_t n = threadIdx.x; n < N; n += LS_THREADS) {
        const double v = y[n] - sub;
        s1 = fma(w[n], v, s1);
        s2 = fma(w[n] * v, v, s2);
    }
    double Yw = block_sum(s1, red);
    const double Y2 = block_sum(s2, red);
    if (!fit_mean) Yw = 0.0;
    double YY = Y2 - Yw * Yw;
    const bool bad = !isfinite(YY) || !isfinite(mean) || !(YY > 1e-28 * raw2);
    if (threadIdx.x == 0) {
        dr[b] = sub;
        dr[B + b] = Yw;
        dr[2 * B + b] = bad ? NAN : YY;
        if (status) status[b] = bad ? 2 : 0;
    }
}

// power[b][f] of a BM x BN/2 block of (draw, frequency).  Four wavefronts in a 2 x 2 arrangement, each BM/2 x BN/2 of the product.
// LDS images, two buffers each: the series tile As[row][k] (stride 18: the lanes of a k-step's read, row = l & 15 and k = l >> 4, fall on
// 32 different 8-byte banks per half wavefront) and the table tile Bs[k][col] (stride BN + 16, the same property).
template <int BM, int BN>
__global__ __launch_bounds__(LS_THREADS) void ls_product_kernel(int64_t N, int64_t Npad, int64_t B, int64_t Fc, int64_t Fpad, int64_t ldp,
                                                                const double* __restrict__ Y, const double* __restrict__ G,
                                                                const double* __restrict__ fq, const double* __restrict__ dr,
                                                                double* __restrict__ power)
{
    constexpr int AS = LS_BK + 2, BS = BN + 16;
    constexpr int AP = BM / 16;              // loader passes over the series tile: 16 rows each (16 lanes along k)
    constexpr int BKR = 2 * LS_THREADS / BN; // table rows per loader pass (a thread moves two columns)
    constexpr int BP = LS_BK / BKR;
    constexpr int TM = BM / 32, TN = BN / 32;
    __shared__ double As[2][BM * AS];
    __shared__ double Bs[2][LS_BK * BS];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lr = lane & 15, lk = lane >> 4;
    const int64_t row0 = (int64_t)blockIdx.x * BM;
    const int64_t col0 = (int64_t)blockIdx.y * BN;      // column of G: 2 f + (0 cos | 1 sin)
    const int wm0 = (wave >> 1) * (BM / 2), wn0 = (wave & 1) * (BN / 2);

    // loaders.  Series: k = tid & 15, rows (tid >> 4) + 16 i; rows past B and times past N give zeros.  Table: padded, no bounds.
    const int ak = tid & 15, ar = tid >> 4;
    const double* arow[AP];
    double amean[AP];
#pragma unroll
    for (int i = 0; i < AP; ++i) {
        const int64_t r = row0 + ar + 16 * i;
        arow[i] = r < B ? Y + r * N : nullptr;
        amean[i] = r < B ? dr[r] : 0.0;
    }
    const int bc = (tid % (BN / 2)) * 2, bk = tid / (BN / 2);
    const double* gcol = G + col0 + bc;
    const int64_t ldg = 2 * Fpad;

    double areg[AP];
    double2 breg[BP];
    auto fetch = [&](int64_t k0) {
#pragma unroll
        for (int i = 0; i < AP; ++i) areg[i] = (arow[i] && k0 + ak < N) ? arow[i][k0 + ak] - amean[i] : 0.0;
#pragma unroll
        for (int j = 0; j < BP; ++j) breg[j] = *reinterpret_cast<const double2*>(gcol + (k0 + bk + BKR * j) * ldg);
    };
    auto stash = [&](int buf) {
#pragma unroll
        for (int i = 0; i < AP; ++i) As[buf][(ar + 16 * i) * AS + ak] = areg[i];
#pragma unroll
        for (int j = 0; j < BP; ++j) *reinterpret_cast<double2*>(&Bs[buf][(bk + BKR * j) * BS + bc]) = breg[j];
    };

    f64x4 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = f64x4{0.0, 0.0, 0.0, 0.0};

    fetch(0);
    stash(0);
    __syncthreads();
    const int64_t ktiles = Npad / LS_BK;
    for (int64_t kt = 0; kt < ktiles; ++kt) {
        const int buf = (int)(kt & 1);
        if (kt + 1 < ktiles) fetch((kt + 1) * LS_BK);      // in flight while this tile is multiplied
#pragma unroll
        for (int ks = 0; ks < LS_BK / 4; ++ks) {
            double a[TM], bb[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) a[i] = As[buf][(wm0 + 16 * i + lr) * AS + 4 * ks + lk];
#pragma unroll
            for (int j = 0; j < TN; ++j) bb[j] = Bs[buf][(4 * ks + lk) * BS + wn0 + 16 * j + lr];
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], bb[j], acc[i][j], 0, 0, 0);
        }
        if (kt + 1 < ktiles) stash(buf ^ 1);               // the other buffer: last read before the previous barrier
        __syncthreads();
    }

    // epilogue.  Result register g of lane (lk, lr) of tile (i, j): draw row0 + wm0 + 16 i + lk + 4 g, column col0 + wn0 + 16 j + lr; the
    // sin column of a frequency sits in the neighbouring lane.
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int64_t f = (col0 + wn0 + 16 * j + lr) >> 1;     // < Fpad
        const double C = fq[f], S = fq[Fpad + f], CC = fq[2 * Fpad + f], SS = fq[3 * Fpad + f], CS = fq[4 * Fpad + f], D = fq[5 * Fpad + f];
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const double mine = acc[i][j][g];
                const double other = __shfl_xor(mine, 1);
                const int64_t b = row0 + wm0 + 16 * i + lk + 4 * g;
                if ((lr & 1) == 0 && b < B && f < Fc) {
                    const double Yw = dr[B + b], YY = dr[2 * B + b];
                    const double YC = mine - Yw * C, YS = other - Yw * S;
                    power[b * ldp + f] = (SS * YC * YC + CC * YS * YS - 2.0 * CS * YC * YS) / (YY * D);
                }
            }
    }
}

}   // namespace

// ---- host side -----------------------------------------------------------------------------------------------------------------------
// Output tile of the product per workgroup, by measurement (docs/EXPERIMENTS.md section 20; N = 1e4, F = 1000): 64 x 64 takes 1.72 ms at 1000 draws
// and 1.46 ms at 256, 128 x 128 (one workgroup of four wavefronts per CU) 3.46 and 3.45 ms.  The automatic choice is 64 x 64 for every shape;
// 128 x 128 stays reachable through the context option "ls_tile" (same bits).
static int ls_tile(int64_t, int64_t) { return 64; }

int64_t pioran_ls_fpad(int64_t Fc) { return (Fc + LS_TF - 1) / LS_TF * LS_TF; }   // table columns: 2 fpad (a multiple of every tile width)
// most frequencies of one chunk: keeps the y dimension of both grids (frequency blocks of the table kernel, column tiles of the product) under 65536
int64_t pioran_ls_max_fchunk() { return int64_t(1) << 20; }
int64_t pioran_ls_npad(int64_t N) { return (N + LS_ROWS - 1) / LS_ROWS * LS_ROWS; }              // a multiple of the K tile and of the partial-sum block

// doubles of the workspace of one frequency chunk: G | partial sums | fq
size_t pioran_ls_chunk_doubles(int64_t N, int64_t Fc)
{
    const size_t fpad = (size_t)pioran_ls_fpad(Fc), npad = (size_t)pioran_ls_npad(N);
    return npad * 2 * fpad + (npad / LS_ROWS) * 4 * fpad + 6 * fpad;
}

int pioran_launch_ls_weights(int64_t N, const double* yerr, double* w, hipStream_t stream)
{
    ls_weights_kernel<<<1, LS_THREADS, 0, stream>>>(N, yerr, w);
    return hipGetLastError() == hipSuccess ? PIORAN_OK : PIORAN_ERR_HIP;
}

int pioran_launch_ls_series(int64_t N, int64_t B, const double* Y, const double* w, int fit_mean, int center, double* dr, int32_t* status,
                            hipStream_t stream)
{
    ls_series_kernel<<<(unsigned)B, LS_THREADS, 0, stream>>>(N, B, Y, w, fit_mean, center, dr, status);
    return hipGetLastError() == hipSuccess ? PIORAN_OK : PIORAN_ERR_HIP;
}

// table + per-frequency scalars of the Fc frequencies at `freq` into `work` (pioran_ls_chunk_doubles)
int pioran_launch_ls_table(int64_t N, int64_t Fc, const double* t, const double* w, const double* freq, int fit_mean, double* work,
                           hipStream_t stream)
{
    const int64_t fpad = pioran_ls_fpad(Fc), npad = pioran_ls_npad(N), nblk = npad / LS_ROWS;
    double* G = work;
    double* part = G + npad * 2 * fpad;
    double* fq = part + nblk * 4 * fpad;
    ls_table_kernel<<<dim3((unsigned)nblk, (unsigned)(fpad / LS_TF)), LS_TF, 0, stream>>>(N, Fc, fpad, t, w, freq, G, part);
    if (hipGetLastError() != hipSuccess) return PIORAN_ERR_HIP;
    ls_freq_kernel<<<(unsigned)((fpad + LS_THREADS - 1) / LS_THREADS), LS_THREADS, 0, stream>>>(nblk, Fc, fpad, fit_mean, part, fq);
    return hipGetLastError() == hipSuccess ? PIORAN_OK : PIORAN_ERR_HIP;
}

// power[b][f0 .. f0 + Fc) (row stride ldp) of B draws from the chunk's workspace.  tile: 0 automatic, 64 or 128 (tools).
int pioran_launch_ls_product(int64_t N, int64_t B, int64_t Fc, const double* Y, const double* work, const double* dr, double* power,
                             int64_t ldp, int tile, hipStream_t stream)
{
    const int64_t fpad = pioran_ls_fpad(Fc), npad = pioran_ls_npad(N), nblk = npad / LS_ROWS;
    const double* G = work;
    const double* fq = G + npad * 2 * fpad + nblk * 4 * fpad;
    if (tile != 64 && tile != 128) tile = ls_tile(B, Fc);
    const int64_t cols = (2 * Fc + tile - 1) / tile;     // column tiles that hold a live frequency (<= 2 fpad / tile)
    const dim3 grid((unsigned)((B + tile - 1) / tile), (unsigned)cols);
    if (tile == 128)
        ls_product_kernel<128, 128><<<grid, LS_THREADS, 0, stream>>>(N, npad, B, Fc, fpad, ldp, Y, G, fq, dr, power);
    else
        ls_product_kernel<64, 64><<<grid, LS_THREADS, 0, stream>>>(N, npad, B, Fc, fpad, ldp, Y, G, fq, dr, power);
    return hipGetLastError() == hipSuccess ? PIORAN_OK : PIORAN_ERR_HIP;
}
