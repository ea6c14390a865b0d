// CARMA(p, q) on the device: the sampled parameters of the reference's CARMA models -> celerite coefficients, their reverse mode, and the PSD.
//
// Restates, per draw (tools/carma_proto.py is the numpy twin, operation by operation):
//   quad2roots            src/CARMA.jl:201-223   pairs (c, b) = (quad[k], quad[k+1]) -> (-b +- i sqrt(4c - b^2)) / 2; odd order: last root -quad[end]
//   beta                  roots2coeffs(quad2roots(qb)) (docs/src/carma.md:27,39) formed as the product of the REAL factors x^2 + qb[k+1] x + qb[k]
//                         (and x + qb[end] for odd q): the same monic polynomial, ascending coefficients, no complex arithmetic
//   CARMA_celerite_coefs  src/CARMA.jl:98-143    one term per second root; Frac = -beta(r) beta(-r) / Re r / prod_{r_j != r} (r_j - r)(conj r_j + r)
//   evaluate              src/CARMA.jl:150-172   2 |beta(iw) / alpha(iw)|^2 norm / CARMA_normalisation (:279-300), or 4 |.|^2 norm
//   the models' rejections (docs/src/carma.md:29-37, check_roots_bounds src/utils.jl:187-192)
// Orders: 1 <= p <= 16, 0 <= q <= p (src/CARMA.jl:28-36); J = (p + 1) / 2 terms, for odd p the last one real (b = d = 0).
//
// One thread per draw in 64-thread blocks, as approx_kernel; complex arithmetic written out in doubles.  A draw's roots [p] and beta [q + 1] are arrays
// indexed by loop counters that depend on p and q: they live in LDS, element i of lane l at [i][l] (a wavefront's access to one element is 64 consecutive
// values, conflict-free), so nothing is indexed in private memory and no kernel here uses scratch whatever p and q are.  No operation mixes draws: a
// draw's result does not depend on its place in the batch.
//
// The reverse mode (carma_vjp_kernel) applies the Jacobian direction by direction with forward duals in real arithmetic: the forward map is ONE
// template over the scalar type (double, or Dual = value + derivative along the seeded input), so the derivative code is the value code.  At most
// p + q <= 31 passes of a map that costs O(p (p + q)) flops, plus d/dnorm, which is the value's own sum; nothing is kept between the kernels.
#include "common.h"

#include <cmath>

namespace {

constexpr int kCarmaMaxP = 16;
constexpr int kLanes = 64;

// flag of a rejected draw (0: accepted); the first reason in this order is reported
enum : int32_t { kRejNonFinite = 1, kRejNotPair = 2, kRejRealPart = 3, kRejBounds = 4 };

struct Dual {
    double v, d;
    __device__ Dual() = default;
    __device__ Dual(double x) : v(x), d(0.0) {}
    __device__ Dual(double x, double y) : v(x), d(y) {}
};
__device__ __forceinline__ Dual operator+(Dual a, Dual b) { return {a.v + b.v, a.d + b.d}; }
__device__ __forceinline__ Dual operator-(Dual a, Dual b) { return {a.v - b.v, a.d - b.d}; }
__device__ __forceinline__ Dual operator-(Dual a) { return {-a.v, -a.d}; }
__device__ __forceinline__ Dual operator*(Dual a, Dual b) { return {a.v * b.v, fma(a.v, b.d, a.d * b.v)}; }
__device__ __forceinline__ Dual operator/(Dual a, Dual b)
{
    const double q = a.v / b.v;
    return {q, (a.d - q * b.d) / b.v};
}
__device__ __forceinline__ Dual dsqrt(Dual a)
{
    const double s = sqrt(a.v);
    return {s, a.d / (2.0 * s)};
}
__device__ __forceinline__ double dsqrt(double a) { return sqrt(a); }
__device__ __forceinline__ double val(double a) { return a; }
__device__ __forceinline__ double val(Dual a) { return a.v; }

// input `idx` of the draw (qa: 0 .. p - 1, qb: p .. p + q - 1) as the scalar type: the plain value, or the dual seeded along direction `dir`
struct NoSeed {
    __device__ double operator()(int, double x) const { return x; }
};
struct SeedDir {
    int dir;
    __device__ Dual operator()(int idx, double x) const { return {x, idx == dir ? 1.0 : 0.0}; }
};

// quad2roots: n quadratic-factor coefficients -> n roots (re, im), LDS arrays of stride kLanes
template <class T, class Seed>
__device__ void carma_quad2roots(int n, const double* quad, int seed_off, Seed seed, T* re, T* im)
{
    for (int k = 0; k + 1 < n; k += 2) {
        const T c = seed(seed_off + k, quad[k]), b = seed(seed_off + k + 1, quad[k + 1]);
        const T disc = b * b - T(4.0) * c;                 // < 0 in an accepted draw
        const T h = dsqrt(-disc) * T(0.5), r = -b * T(0.5);
        re[k * kLanes] = r; im[k * kLanes] = h;
        re[(k + 1) * kLanes] = r; im[(k + 1) * kLanes] = -h;
    }
    if (n & 1) {
        re[(n - 1) * kLanes] = -seed(seed_off + n - 1, quad[n - 1]);
        im[(n - 1) * kLanes] = T(0.0);
    }
}

// beta [q + 1], ascending and monic: the product of the real factors x^2 + qb[k + 1] x + qb[k], then x + qb[q - 1] for odd q
template <class T, class Seed>
__device__ void carma_beta_from_quad(int q, const double* qb, int seed_off, Seed seed, T* beta)
{
    beta[0] = T(1.0);
    int deg = 0;
    for (int k = 0; k + 1 < q; k += 2) {
        const T c = seed(seed_off + k, qb[k]), b = seed(seed_off + k + 1, qb[k + 1]);
        for (int i = deg + 2; i >= 0; --i) {               // descending: the entries below i still hold the old polynomial
            T acc = i <= deg ? c * beta[i * kLanes] : T(0.0);
            if (i >= 1 && i - 1 <= deg) acc = acc + b * beta[(i - 1) * kLanes];
            if (i >= 2) acc = acc + beta[(i - 2) * kLanes];
            beta[i * kLanes] = acc;
        }
        deg += 2;
    }
    if (q & 1) {
        const T s = seed(seed_off + q - 1, qb[q - 1]);
        for (int i = deg + 1; i >= 0; --i) {
            T acc = i <= deg ? s * beta[i * kLanes] : T(0.0);
            if (i >= 1) acc = acc + beta[(i - 1) * kLanes];
            beta[i * kLanes] = acc;
        }
    }
}

// Frac of root i (src/CARMA.jl:112-121): -num_1 num_2 / Re r, num_1 = beta(r), num_2 = beta(-r) by Horner's rule, divided by the product of
// (r_j - r)(conj r_j + r) over the roots whose VALUE differs from r (the reference's filter).  CARMA_normalisation's term of the root is Frac / 2.
template <class T>
__device__ void carma_frac(int p, int q, int i, const T* re, const T* im, const T* beta, T& fr, T& fi)
{
    const T xr = re[i * kLanes], xi = im[i * kLanes];
    T ar = beta[q * kLanes], ai = T(0.0), br = ar, bi = T(0.0);
    for (int l = q - 1; l >= 0; --l) {
        const T bl = beta[l * kLanes];
        T t = ar * xr - ai * xi + bl;
        ai = ar * xi + ai * xr;
        ar = t;
        t = bl - (br * xr - bi * xi);
        bi = -(br * xi + bi * xr);
        br = t;
    }
    const T nr = -(ar * br - ai * bi) / xr, ni = -(ar * bi + ai * br) / xr;
    T dr = T(1.0), di = T(0.0);
    for (int j = 0; j < p; ++j) {
        const T ur = re[j * kLanes], ui = im[j * kLanes];
        if (val(ur) == val(xr) && val(ui) == val(xi)) continue;
        const T er = ur - xr, ei = ui - xi, gr = ur + xr, gi = xi - ui;
        const T pr = er * gr - ei * gi, pi = er * gi + ei * gr;
        const T t = dr * pr - di * pi;
        di = dr * pi + di * pr;
        dr = t;
    }
    const T m = dr * dr + di * di;
    fr = (nr * dr + ni * di) / m;
    fi = (ni * dr - nr * di) / m;
}

// (a, b, c, d) of term k before the normalisation (src/CARMA.jl:122-134): paired terms carry both roots of the pair, the last term of an odd p is real
template <class T>
__device__ void carma_term(int p, int q, int k, const T* re, const T* im, const T* beta, T& a, T& b, T& c, T& d)
{
    T fr, fi;
    carma_frac(p, q, 2 * k, re, im, beta, fr, fi);
    const bool real_term = (p & 1) && 2 * k == p - 1;
    a = real_term ? fr : T(2.0) * fr;
    b = real_term ? T(0.0) : T(2.0) * fi;
    c = -re[2 * k * kLanes];
    d = real_term ? T(0.0) : -im[2 * k * kLanes];
}

__device__ bool carma_in_bounds(double re, double im, double f_lo, double f_hi)
{
    return -f_hi < re && re < -f_lo && -f_hi < im && im < f_hi;   // check_roots_bounds, one root
}

// The rejection rules on n quadratic-factor coefficients; `seen` collects the reasons as bits 1 << reason
__device__ void carma_check_quad(int n, const double* quad, bool bounds, double f_lo, double f_hi, unsigned& seen)
{
    for (int k = 0; k < n; ++k)
        if (!isfinite(quad[k])) seen |= 1u << kRejNonFinite;
    for (int k = 0; k + 1 < n; k += 2) {
        const double c = quad[k], b = quad[k + 1], disc = b * b - 4.0 * c;
        if (!(disc < 0.0)) { seen |= 1u << kRejNotPair; continue; }
        const double h = sqrt(-disc) * 0.5, r = -b * 0.5;
        if (!(r < 0.0)) seen |= 1u << kRejRealPart;
        if (bounds && !(carma_in_bounds(r, h, f_lo, f_hi) && carma_in_bounds(r, -h, f_lo, f_hi))) seen |= 1u << kRejBounds;
    }
    if (n & 1) {
        const double r = -quad[n - 1];
        if (!(r < 0.0)) seen |= 1u << kRejRealPart;
        if (bounds && !carma_in_bounds(r, 0.0, f_lo, f_hi)) seen |= 1u << kRejBounds;
    }
}

// ... on p roots (re, im) [p][2] and the q + 1 moving-average coefficients as CARMA(...) holds them
__device__ void carma_check_roots(int p, int q, const double* roots, const double* beta, bool bounds, double f_lo, double f_hi, unsigned& seen)
{
    for (int k = 0; k < 2 * p; ++k)
        if (!isfinite(roots[k])) seen |= 1u << kRejNonFinite;
    for (int k = 0; k <= q; ++k)
        if (!isfinite(beta[k])) seen |= 1u << kRejNonFinite;
    for (int k = 0; k < p; ++k) {
        if (!(roots[2 * k] < 0.0)) seen |= 1u << kRejRealPart;
        if (bounds && !carma_in_bounds(roots[2 * k], roots[2 * k + 1], f_lo, f_hi)) seen |= 1u << kRejBounds;
    }
}

__device__ int32_t carma_first_reason(unsigned seen)
{
    for (int32_t r = kRejNonFinite; r <= kRejBounds; ++r)
        if (seen & (1u << r)) return r;
    return 0;
}

// form 0: in1 = qa [B][p], in2 = qb [B][q] (nullptr for q = 0); form 1: in1 = roots [B][p][2], in2 = beta [B][q + 1]
__device__ int32_t carma_check(int form, int p, int q, const double* in1, const double* in2, double norm, double f_lo, double f_hi)
{
    const bool bounds = f_lo != 0.0 || f_hi != 0.0;
    unsigned seen = isfinite(norm) ? 0u : 1u << kRejNonFinite;
    if (form == 0) {
        carma_check_quad(p, in1, bounds, f_lo, f_hi, seen);
        carma_check_quad(q, in2, bounds, f_lo, f_hi, seen);
    } else {
        carma_check_roots(p, q, in1, in2, bounds, f_lo, f_hi, seen);
    }
    return carma_first_reason(seen);
}

// the draw's roots and beta into LDS (plain values)
__device__ void carma_stage(int form, int p, int q, const double* in1, const double* in2, double* re, double* im, double* beta)
{
    if (form == 0) {
        carma_quad2roots(p, in1, 0, NoSeed{}, re, im);
        carma_beta_from_quad(q, in2, p, NoSeed{}, beta);
    } else {
        for (int k = 0; k < p; ++k) { re[k * kLanes] = in1[2 * k]; im[k * kLanes] = in1[2 * k + 1]; }
        for (int k = 0; k <= q; ++k) beta[k * kLanes] = in2[k];
    }
}

extern __shared__ double carma_lds[];

__global__ void __launch_bounds__(64) carma_coefs_kernel(int64_t B, int p, int q, int form, const double* __restrict__ in1, const double* __restrict__ in2,
                                                         const double* __restrict__ norm, int integrated, double f_lo, double f_hi,
                                                         double* __restrict__ A, double* __restrict__ Bc, double* __restrict__ C, double* __restrict__ D,
                                                         int32_t* __restrict__ flags)
{
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int J = (p + 1) / 2;
    double* re = carma_lds + threadIdx.x;
    double* im = re + p * kLanes;
    double* beta = im + p * kLanes;
    const double* r1 = in1 + b * (form == 0 ? p : 2 * p);
    const double* r2 = form == 0 ? (q ? in2 + b * q : nullptr) : in2 + b * (q + 1);
    double *a = A + b * J, *bb = Bc + b * J, *c = C + b * J, *d = D + b * J;
    const int32_t flag = carma_check(form, p, q, r1, r2, norm[b], f_lo, f_hi);
    if (flags) flags[b] = flag;
    if (flag) {                                      // benign coefficients: the scan that follows runs harmlessly
        for (int k = 0; k < J; ++k) { a[k] = 1.0; bb[k] = 0.0; c[k] = 1.0; d[k] = 0.0; }
        return;
    }
    carma_stage(form, p, q, r1, r2, re, im, beta);
    double variance = 0.0;
    for (int k = 0; k < J; ++k) {
        double ak, bk, ck, dk;
        carma_term(p, q, k, re, im, beta, ak, bk, ck, dk);
        a[k] = ak; bb[k] = bk; c[k] = ck; d[k] = dk;
        variance += ak;
    }
    const double va = integrated ? norm[b] / variance : norm[b];
    for (int k = 0; k < J; ++k) { a[k] *= va; bb[k] *= va; }
}

// Quad form only.  (ga, gb, gc, gd) [B][J] -> grad_qa [B][p], grad_qb [B][q], grad_norm [B].  With (a', b') the terms before the normalisation,
// W = sum ga a' + gb b', V = sum a' and X = sum gc c + gd d, the contraction is G = norm W / V + X (norm W + X without the integrated normalisation):
// each pass carries W, V, X as duals along one input and stores G's derivative; grad_norm = W / V (W) comes out of the first pass.
__global__ void __launch_bounds__(64) carma_vjp_kernel(int64_t B, int p, int q, const double* __restrict__ qa, const double* __restrict__ qb,
                                                       const double* __restrict__ norm, int integrated, double f_lo, double f_hi,
                                                       const double* __restrict__ ga, const double* __restrict__ gb, const double* __restrict__ gc,
                                                       const double* __restrict__ gd, double* __restrict__ gqa, double* __restrict__ gqb,
                                                       double* __restrict__ gnorm)
{
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int J = (p + 1) / 2;
    Dual* re = reinterpret_cast<Dual*>(carma_lds) + threadIdx.x;
    Dual* im = re + p * kLanes;
    Dual* beta = im + p * kLanes;
    const double* r1 = qa + b * p;
    const double* r2 = q ? qb + b * q : nullptr;
    if (carma_check(0, p, q, r1, r2, norm[b], f_lo, f_hi)) {
        for (int k = 0; k < p; ++k) gqa[b * p + k] = 0.0;
        for (int k = 0; k < q; ++k) gqb[b * q + k] = 0.0;
        gnorm[b] = 0.0;
        return;
    }
    const double nb = norm[b];
    for (int dir = 0; dir < p + q; ++dir) {
        const SeedDir seed{dir};
        carma_quad2roots(p, r1, 0, seed, re, im);
        carma_beta_from_quad(q, r2, p, seed, beta);
        Dual W(0.0), V(0.0), X(0.0);
        for (int k = 0; k < J; ++k) {
            Dual ak, bk, ck, dk;
            carma_term(p, q, k, re, im, beta, ak, bk, ck, dk);
            W = W + Dual(ga[b * J + k]) * ak + Dual(gb[b * J + k]) * bk;
            V = V + ak;
            X = X + Dual(gc[b * J + k]) * ck + Dual(gd[b * J + k]) * dk;
        }
        const Dual G = (integrated ? Dual(nb) * W / V : Dual(nb) * W) + X;
        if (dir < p) gqa[b * p + dir] = G.d; else gqb[b * q + dir - p] = G.d;
        if (dir == 0) gnorm[b] = integrated ? W.v / V.v : W.v;
    }
}

// evaluate(::CARMA, f), per draw: the checks, the roots and beta the frequency kernel reads, and the factor in front of |beta(iw) / alpha(iw)|^2 —
// 2 norm / CARMA_normalisation(r_alpha, beta) (the sum of Frac / 2 over ALL roots, real part; src/CARMA.jl:279-300) or 4 norm
__global__ void __launch_bounds__(64) carma_psd_draws_kernel(int64_t B, int p, int q, int form, const double* __restrict__ in1,
                                                             const double* __restrict__ in2, const double* __restrict__ norm, int integrated, double f_lo,
                                                             double f_hi, double* __restrict__ roots, double* __restrict__ betas, double* __restrict__ scale,
                                                             int32_t* __restrict__ status)
{
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double* re = carma_lds + threadIdx.x;
    double* im = re + p * kLanes;
    double* beta = im + p * kLanes;
    const double* r1 = in1 + b * (form == 0 ? p : 2 * p);
    const double* r2 = form == 0 ? (q ? in2 + b * q : nullptr) : in2 + b * (q + 1);
    const int32_t flag = carma_check(form, p, q, r1, r2, norm[b], f_lo, f_hi);
    status[b] = flag ? 3 : 0;
    if (flag) { scale[b] = NAN; return; }
    carma_stage(form, p, q, r1, r2, re, im, beta);
    double s = 4.0 * norm[b];
    if (integrated) {
        double variance = 0.0;
        for (int i = 0; i < p; ++i) {
            double fr, fi;
            carma_frac(p, q, i, re, im, beta, fr, fi);
            variance += 0.5 * fr;
        }
        s = 2.0 * norm[b] / variance;
    }
    scale[b] = s;
    for (int k = 0; k < p; ++k) { roots[b * 2 * p + 2 * k] = re[k * kLanes]; roots[b * 2 * p + 2 * k + 1] = im[k * kLanes]; }
    for (int k = 0; k <= q; ++k) betas[b * (q + 1) + k] = beta[k * kLanes];
}

// ... per draw and frequency, [B][F] with f the fastest index across a wavefront (whole lines stored); the draw's roots, beta and factor are uniform
// over the workgroup (scalar loads).  |alpha(iw)|^2 is formed as prod_l |iw - r_l|^2 = prod_l (Re r_l)^2 + (w - Im r_l)^2: alpha = prod (x - r_l) is the
// same monic polynomial as roots2coeffs(r_alpha) gives (fromroots), evaluated without forming its coefficients.
__global__ void __launch_bounds__(256) carma_psd_eval_kernel(int64_t B, int64_t F, int64_t ftiles, int p, int q, const double* __restrict__ roots,
                                                             const double* __restrict__ betas, const double* __restrict__ scale,
                                                             const int32_t* __restrict__ status, const double* __restrict__ freq, int times_f,
                                                             double* __restrict__ out)
{
    const int64_t draw = blockIdx.x / ftiles, f = (blockIdx.x % ftiles) * 256 + threadIdx.x;
    if (draw >= B || f >= F) return;
    if (status[draw]) { out[draw * F + f] = NAN; return; }
    const double* r = roots + draw * 2 * p;
    const double* be = betas + draw * (q + 1);
    const double fr = freq[f], w = 2.0 * M_PI * fr;
    double nr = be[q], ni = 0.0;                      // beta(iw) by Horner's rule
    for (int l = q - 1; l >= 0; --l) {
        const double t = be[l] - ni * w;
        ni = nr * w;
        nr = t;
    }
    double den = 1.0;
    for (int l = 0; l < p; ++l) {
        const double x = r[2 * l], y = w - r[2 * l + 1];
        den *= x * x + y * y;
    }
    double v = (nr * nr + ni * ni) / den * scale[draw];
    if (times_f) v *= fr;
    out[draw * F + f] = v;
}

bool carma_orders_ok(int p, int q) { return p >= 1 && p <= kCarmaMaxP && q >= 0 && q <= p; }

template <class T>
size_t carma_lds_bytes(int p, int q) { return (size_t)(2 * p + q + 1) * kLanes * sizeof(T); }

}  // namespace

int pioran_carma_max_order() { return kCarmaMaxP; }

int pioran_launch_carma_coefs(int64_t B, int p, int q, int form, const double* in1, const double* in2, const double* norm, int integrated, double f_lo,
                              double f_hi, double* A, double* Bc, double* C, double* D, int32_t* flags, hipStream_t stream)
{
    const int64_t blocks = (B + 63) / 64;
    if (blocks <= 0 || blocks > 0x7fffffffLL || !carma_orders_ok(p, q) || form < 0 || form > 1) return PIORAN_ERR_ARG;
    hipLaunchKernelGGL(carma_coefs_kernel, dim3((unsigned)blocks), dim3(64), carma_lds_bytes<double>(p, q), stream, B, p, q, form, in1, in2, norm,
                       integrated, f_lo, f_hi, A, Bc, C, D, flags);
    return hipGetLastError() == hipSuccess ? PIORAN_OK : PIORAN_ERR_HIP;
}

int pioran_launch_carma_vjp(int64_t B, int p, int q, const double* qa, const double* qb, const double* norm, int integrated, double f_lo, double f_hi,
                            const double* ga, const double* gb, const double* gc, const double* gd, double* gqa, double* gqb, double* gnorm,
                            hipStream_t stream)
{
    const int64_t blocks = (B + 63) / 64;
    if (blocks <= 0 || blocks > 0x7fffffffLL || !carma_orders_ok(p, q)) return PIORAN_ERR_ARG;
    hipLaunchKernelGGL(carma_vjp_kernel, dim3((unsigned)blocks), dim3(64), carma_lds_bytes<Dual>(p, q), stream, B, p, q, qa, qb, norm, integrated, f_lo,
                       f_hi, ga, gb, gc, gd, gqa, gqb, gnorm);
    return hipGetLastError() == hipSuccess ? PIORAN_OK : PIORAN_ERR_HIP;
}

int pioran_launch_carma_psd(int64_t B, int p, int q, int form, const double* in1, const double* in2, const double* norm, int integrated, double f_lo,
                            double f_hi, int64_t F, const double* freq, int times_f, double* roots, double* betas, double* scale, double* psd,
                            int32_t* status, hipStream_t stream)
{
    const int64_t blocks = (B + 63) / 64, ftiles = (F + 255) / 256;
    if (blocks <= 0 || F < 1 || B * ftiles > 0x7fffffffLL || !carma_orders_ok(p, q) || form < 0 || form > 1) return PIORAN_ERR_ARG;
    hipLaunchKernelGGL(carma_psd_draws_kernel, dim3((unsigned)blocks), dim3(64), carma_lds_bytes<double>(p, q), stream, B, p, q, form, in1, in2, norm,
                       integrated, f_lo, f_hi, roots, betas, scale, status);
    if (hipGetLastError() != hipSuccess) return PIORAN_ERR_HIP;
    hipLaunchKernelGGL(carma_psd_eval_kernel, dim3((unsigned)(B * ftiles)), dim3(256), 0, stream, B, F, ftiles, p, q, roots, betas, scale, status, freq,
                       times_f, psd);
    return hipGetLastError() == hipSuccess ? PIORAN_OK : PIORAN_ERR_HIP;
}
