// Column quantiles and means over the draw axis — what all three posterior predictive checks of the reference end in
// (plot_ppc_timeseries, src/plots_diagnostics.jl:805-816; plot_lsp_ppc :547-559; plot_psd_ppc :417-447): X [B][ldx] holds one draw per row,
// and every output column is reduced to Q quantiles (Statistics.quantile with its defaults, type 7) and a mean over the rows with status 0.
// The definition, operation by operation, is tools/quantiles_proto.py; the interpolation below is the same sequence of individually rounded
// fp64 operations (no contraction anywhere in this file), so the quantiles are the twin's bits.
//
//   quantile_kernel<KP>   a workgroup owns TC = 8192 / KP adjacent output columns, KP the power of two >= B (>= 32) — 8 columns, 64-byte runs of a
//   row, at B = 1000; above 1024 draws only 4 or 2 columns (32- and 16-byte runs: those loads are barely coalesced; not measured):
//     1. the kept rows are numbered by a prefix over status (every workgroup does this itself: no host synchronisation)
//     2. the tile is loaded row by row (runs of TC adjacent doubles), each value formed while loading (gather, exp(v + shift_b), (ref - v) / scale),
//        turned into a 64-bit key whose unsigned order is the total order of the doubles, and stored transposed in LDS at its kept-row number;
//        the rest of a column is padded with the largest key
//     3. each column is sorted by a bitonic network: a thread keeps a run of 32 keys in registers for the compare distances below 32, the
//        distances from 32 on go through LDS
//     4. the keys go back to doubles (padding: zeros), the quantiles are read off, and the column is summed by a halving tree over the sorted
//        positions — an order that depends on (KP, position) only, not on Mc, the tile or the caller's chunking
// LDS image: element e = column * KP + row sits at e + 2 (e >> 5): two doubles of padding behind every run of 32, so the 16-byte accesses of
// the threads' runs (34 doubles apart) fall on different banks; the LDS passes touch 32 consecutive doubles per half wavefront.
#include "common.h"

#include <cmath>

#pragma clang fp contract(off)

namespace {

constexpr int QT_THREADS = 256;
constexpr int QT_RUN = 32;                         // keys a thread keeps in registers
constexpr int QT_TILE = QT_THREADS * QT_RUN;       // keys of a workgroup
constexpr int QT_MAXB = 4096;
constexpr uint64_t QT_PAD = ~uint64_t(0);          // above every key
constexpr uint64_t QT_NAN = ~uint64_t(0) - 1;      // every NaN: above +inf, below the padding
constexpr uint16_t QT_OUT = 0xffff;                // row left out

struct QuantParams {
    int64_t B, M, ldx, Mc, Q;
    const double* X;
    const int32_t* status;
    const double* shift;
    const int32_t* cols;
    const double* ref;
    const double* scale;
    const double* probs;
    double* quant;
    double* mean;
    int32_t* kept;
};

__device__ __forceinline__ int lds_at(int e) { return e + 2 * (e >> 5); }

__device__ __forceinline__ uint64_t to_key(double v)
{
    if (v != v) return QT_NAN;
    const uint64_t u = (uint64_t)__double_as_longlong(v);
    return u ^ ((u >> 63) ? ~uint64_t(0) : (uint64_t(1) << 63));
}

__device__ __forceinline__ double from_key(uint64_t k)
{
    const uint64_t u = k ^ ((k >> 63) ? (uint64_t(1) << 63) : ~uint64_t(0));
    return __longlong_as_double((long long)u);
}

__device__ __forceinline__ void cmpx(uint64_t& x, uint64_t& y, bool asc)
{
    const bool sw = (x > y) == asc;
    const uint64_t lo = sw ? y : x, hi = sw ? x : y;
    x = lo;
    y = hi;
}

template <int KP>
__global__ __launch_bounds__(QT_THREADS) void quantile_kernel(QuantParams p)
{
    constexpr int TC = QT_TILE / KP;                       // columns of a workgroup
    constexpr int RP = KP >= QT_THREADS ? KP / QT_THREADS : 1;   // rows a thread numbers
    __shared__ __attribute__((aligned(16))) uint64_t s[QT_TILE + 2 * (QT_TILE / 32)];
    __shared__ uint16_t pos[KP];
    __shared__ int scan[QT_THREADS];

    const int tid = threadIdx.x;
    const int B = (int)p.B;                                // <= KP <= 4096
    const int64_t m0 = (int64_t)blockIdx.x * TC;

    // 1. kept-row numbers
    int cnt = 0;
    for (int i = 0; i < RP; ++i) {
        const int b = tid * RP + i;
        if (b < B && (!p.status || p.status[b] == 0)) ++cnt;
    }
    scan[tid] = cnt;
    __syncthreads();
    for (int d = 1; d < QT_THREADS; d <<= 1) {
        const int add = tid >= d ? scan[tid - d] : 0;
        __syncthreads();
        scan[tid] += add;
        __syncthreads();
    }
    const int K = scan[QT_THREADS - 1];
    int at = scan[tid] - cnt;
    for (int i = 0; i < RP; ++i) {
        const int b = tid * RP + i;
        if (b < KP) pos[b] = (b < B && (!p.status || p.status[b] == 0)) ? (uint16_t)at++ : QT_OUT;
    }
    const int base = lds_at(tid * QT_RUN);                 // this thread's run: 16-byte aligned
#pragma unroll
    for (int i = 0; i < QT_RUN; ++i) s[base + i] = QT_PAD;
    __syncthreads();

    // 2. load, transform, transpose
    for (int idx = tid; idx < B * TC; idx += QT_THREADS) {
        const int c = idx % TC, b = idx / TC;
        const int64_t m = m0 + c;
        const uint16_t r = pos[b];
        if (m >= p.Mc || r == QT_OUT) continue;
        const int64_t col = p.cols ? (int64_t)p.cols[m] : m;
        double v = (col >= 0 && col < p.M) ? p.X[(int64_t)b * p.ldx + col] : NAN;   // (the device form cannot check cols: no read outside X)
        if (p.shift) v = exp(v + p.shift[b]);
        if (p.ref) v = (p.ref[m] - v) / p.scale[m];
        s[lds_at(c * KP + r)] = to_key(v);
    }
    __syncthreads();

    // 3. bitonic sort of every column, ascending.  Row index of this thread's run within its column: row0 .. row0 + 31.
    const int row0 = (tid * QT_RUN) % KP;
    uint64_t r[QT_RUN];
    auto fetch = [&]() {
#pragma unroll
        for (int i = 0; i < QT_RUN; i += 2) {
            const ulonglong2 w = *reinterpret_cast<const ulonglong2*>(&s[base + i]);
            r[i] = w.x;
            r[i + 1] = w.y;
        }
    };
    auto stash = [&]() {
#pragma unroll
        for (int i = 0; i < QT_RUN; i += 2) *reinterpret_cast<ulonglong2*>(&s[base + i]) = make_ulonglong2(r[i], r[i + 1]);
    };
    fetch();
#pragma unroll
    for (int k = 2; k <= QT_RUN; k <<= 1) {
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1) {
#pragma unroll
            for (int i = 0; i < QT_RUN; ++i)
                if ((i ^ j) > i) cmpx(r[i], r[i ^ j], k < QT_RUN ? (i & k) == 0 : (row0 & QT_RUN) == 0);
        }
    }
    stash();
    __syncthreads();
    for (int k = 2 * QT_RUN; k <= KP; k <<= 1) {
        for (int j = k >> 1; j >= QT_RUN; j >>= 1) {
            for (int pp = tid; pp < QT_TILE / 2; pp += QT_THREADS) {
                const int e = ((pp & ~(j - 1)) << 1) | (pp & (j - 1));   // pair (e, e + j): bit log2(j) of e is clear
                const bool asc = ((e % KP) & k) == 0;
                const int ia = lds_at(e), ib = lds_at(e + j);
                const uint64_t x = s[ia], y = s[ib];
                if ((x > y) == asc) {
                    s[ia] = y;
                    s[ib] = x;
                }
            }
            __syncthreads();
        }
        fetch();
        const bool asc = (row0 & k) == 0;
#pragma unroll
        for (int j = QT_RUN >> 1; j > 0; j >>= 1) {
#pragma unroll
            for (int i = 0; i < QT_RUN; ++i)
                if ((i ^ j) > i) cmpx(r[i], r[i ^ j], asc);
        }
        if (k < KP) {
            stash();
            __syncthreads();
        }
    }

    // 4. back to doubles (this thread's run is in r, sorted); padding becomes zero for the sum
    double* sd = reinterpret_cast<double*>(s);
#pragma unroll
    for (int i = 0; i < QT_RUN; i += 2)
        *reinterpret_cast<double2*>(&sd[base + i]) = make_double2(row0 + i < K ? from_key(r[i]) : 0.0, row0 + i + 1 < K ? from_key(r[i + 1]) : 0.0);
    __syncthreads();

    const double Kd = (double)K;
    for (int64_t idx = tid; idx < p.Q * TC; idx += QT_THREADS) {
        const int c = (int)(idx % TC);
        const int64_t q = idx / TC, m = m0 + c;
        if (m >= p.Mc) continue;
        double out = NAN;
        if (K > 0) {
            const double* v = sd;          // v[lds_at(c * KP + i)], i < K, ascending
            const double pr = p.probs[q];
            const double aleph = Kd * pr + (1.0 - pr);
            int j = (int)aleph;            // trunc: aleph in [1, K]
            j = j > K - 1 ? K - 1 : (j < 1 ? 1 : j);
            double g = aleph - (double)j;
            g = g > 1.0 ? 1.0 : (g < 0.0 ? 0.0 : g);
            const double a = K == 1 ? v[lds_at(c * KP)] : v[lds_at(c * KP + j - 1)];
            const double b = K == 1 ? a : v[lds_at(c * KP + j)];
            const double top = v[lds_at(c * KP + K - 1)];
            const bool close = isfinite(a) && isfinite(b) && fabs(a - b) <= 0x1p-26 * fmax(fabs(a), fabs(b));
            out = close ? a + g * (b - a) : (1.0 - g) * a + g * b;
            if (top != top) out = NAN;     // a NaN among the kept values (they sort last)
        }
        p.quant[q * p.Mc + m] = out;
    }
    __syncthreads();

    // the mean: halving tree over the sorted positions (p.mean is uniform over the grid: every thread leaves or none)
    if (!p.mean) {
        if (p.kept && blockIdx.x == 0 && tid == 0) *p.kept = K;
        return;
    }
    for (int h = KP >> 1; h > 0; h >>= 1) {
        for (int idx = tid; idx < TC * h; idx += QT_THREADS) {
            const int c = idx / h, i = idx % h;
            sd[lds_at(c * KP + i)] += sd[lds_at(c * KP + i + h)];
        }
        __syncthreads();
    }
    for (int c = tid; c < TC; c += QT_THREADS)
        if (m0 + c < p.Mc) p.mean[m0 + c] = sd[lds_at(c * KP)] / Kd;
    if (p.kept && blockIdx.x == 0 && tid == 0) *p.kept = K;
}

template <int KP>
int launch(const QuantParams& p, hipStream_t stream)
{
    constexpr int TC = QT_TILE / KP;
    const int64_t blocks = (p.Mc + TC - 1) / TC;
    if (blocks > 0x7fffffff) return PIORAN_ERR_UNSUPPORTED;
    quantile_kernel<KP><<<(unsigned)blocks, QT_THREADS, 0, stream>>>(p);
    return hipGetLastError() == hipSuccess ? PIORAN_OK : PIORAN_ERR_HIP;
}

}   // namespace

int64_t pioran_quantiles_max_draws() { return QT_MAXB; }

// quant [Q][Mc], mean [Mc] (nullptr: not wanted), kept [1] (nullptr: not wanted) of the rows of X [B][ldx] with status 0; every pointer on the
// device.  cols nullptr: Mc = M columns in order.  B <= pioran_quantiles_max_draws().
int pioran_launch_quantiles(int64_t B, int64_t M, int64_t ldx, const double* X, const int32_t* status, const double* shift, int64_t Mc,
                            const int32_t* cols, const double* ref, const double* scale, int64_t Q, const double* probs, double* quant,
                            double* mean, int32_t* kept, hipStream_t stream)
{
    if (B < 1 || B > QT_MAXB || M < 1 || ldx < M || Mc < 1 || Q < 1) return PIORAN_ERR_ARG;
    const QuantParams p{B, M, ldx, Mc, Q, X, status, shift, cols, ref, scale, probs, quant, mean, kept};
    if (B <= 32) return launch<32>(p, stream);
    if (B <= 64) return launch<64>(p, stream);
    if (B <= 128) return launch<128>(p, stream);
    if (B <= 256) return launch<256>(p, stream);
    if (B <= 512) return launch<512>(p, stream);
    if (B <= 1024) return launch<1024>(p, stream);
    if (B <= 2048) return launch<2048>(p, stream);
    return launch<4096>(p, stream);
}
