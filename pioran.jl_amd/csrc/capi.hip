// C ABI of libpioran_hip.so — see include/pioran_hip.h for the contract and the reference lines
// each entry point replaces.
#include "../../include/pioran_hip.h"
#include "common.h"
#include "route.h"

#include <cmath>
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <thread>
#include <vector>

// One device allocation and its owner: freed when the owner goes.  Grown by ensure (context buffers: with slack) or ensure_exact; every hipMalloc and
// hipFree of the library is in its two functions.
struct DevMem {
    void* p = nullptr;
    size_t cap = 0;   // bytes
    DevMem() = default;
    DevMem(const DevMem&) = delete;
    DevMem& operator=(const DevMem&) = delete;
    ~DevMem() { (void)release(); }
    hipError_t release()        // frees; p = nullptr, cap = 0 whatever the runtime says
    {
        const hipError_t e = p ? hipFree(p) : hipSuccess;
        p = nullptr;
        cap = 0;
        return e;
    }
    bool alloc(size_t bytes)    // of an empty one; false: no memory
    {
        if (hipMalloc(&p, bytes) != hipSuccess) {
            (void)hipGetLastError();   // the failure is reported through the return code: do not leave it sticky for the callers'
                                       // shrink-and-retry loops (a later launch wrapper would read it as its own error)
            p = nullptr;
            return false;
        }
        cap = bytes;
        return true;
    }
};

// ... seen as an array of T
template <class T>
struct DevArray : DevMem {
    operator T*() const { return (T*)p; }
};

struct pioran_ctx {
    pioran_ctx() = default;
    pioran_ctx(const pioran_ctx&) = delete;
    ~pioran_ctx();   // everything the context owns; the caller has set the device and drained the stream
    int device = 0;
    int ncu = 0;                    // compute units of the device (read once, at creation: the dispatch functions must not call into the runtime per launch)
    hipStream_t stream = nullptr;
    bool own_stream = false;
    hipEvent_t ev[16] = {};
    std::string last_err;
    ScanOptions opt{};   // diagnostic switches: environment at creation, then pioran_ctx_set_option
    // pinned staging of the host-pointer entries: pageable hipMemcpyAsync is staged by the runtime with a hidden
    // synchronisation per call (~0.4 ms each); copies out of / into this buffer are true asynchronous DMA.  A bump
    // allocator, reset at every stream synchronisation; results land here and are handed to the caller after the sync.
    char* pin = nullptr;
    size_t pin_cap = 0, pin_off = 0;
    struct Pending { void* host; const void* pinned; size_t bytes; };
    std::vector<Pending> pending;
    // batched dense solver: independent factorisations on their own streams, one slab each (lazy)
    static constexpr int kDenseStreams = 16;
    hipStream_t dstream[kDenseStreams] = {};
    hipEvent_t dev_[kDenseStreams + 1] = {};
    // second stream + events of the gradient's reverse pass (replay of one segment overlaps the adjoint of the next); lazy
    hipStream_t aux = nullptr;
    hipEvent_t gev[5] = {};
    // growable device staging for the host-pointer entry points.  A Buf enters `bufs` as it is constructed, and cannot be constructed otherwise:
    // `bufs` is the one list of them, what pioran_ctx_trim and the destructor walk.  A new buffer is one more name below.
    struct Buf : DevMem {
        explicit Buf(pioran_ctx* owner) { owner->bufs.push_back(this); }
    };
    std::vector<Buf*> bufs;
    Buf bA{this}, bB{this}, bC{this}, bD{this}, bmu{this}, bnu{this}, bY{this}, bS2{this}, bout{this}, bst{this}, bscratch{this}, bK{this},
        bwork{this}, bshift{this}, bgtab{this}, bq{this}, bpair{this}, btp{this}, btprow{this};
    Buf blstab{this}, blsaux{this};   // periodogram: the cos/sin table of a frequency chunk | weights and per-draw scalars
    // posterior draws (rand_posterior_batch): what the chain holds BESIDE the prediction's buffers, which keep their roles there —
    // the caller's normals q_data | q_new | eps, the normals on the merged grid, the simulation's stores | xi | realisations | log L | status,
    // the index maps, the residual series Y | S2, the shifts, a chunk's draws | their status
    Buf brqd{this}, brqn{this}, breps{this}, brqT{this}, brstores{this}, brxi{this}, brf{this}, brsout{this}, brsst{this}, brmaps{this}, brY{this},
        brS2{this}, brshift{this}, brres{this}, brst{this};
    // quantiles over draws (quantiles.hip): the resident draws [B][M] | their status [B] (the summary entry's sink; the host form's staged X and
    // status), the small inputs probs | shift | ref | scale, the indices cols | kept, the results quant | mean
    Buf bqX{this}, bqst{this}, bqin{this}, bqidx{this}, bqout{this};
    // approx and its reverse mode as the two ends of the gradient (ThetaDraws): the grid's sp | w | LU | piv and the batch's theta | norm, a chunk's
    // grad_theta | grad_norm | the kernel's scratch
    Buf bthin{this}, bthout{this};
    // PSD check (psd_check.hip): the grid's sp | LU | piv, the host forms' theta | norm | freq, a chunk's amp | integ | pf0 | status, a chunk's
    // (the summary: the batch's) arrays psd | psd_approx | residuals | ratios, the summary's transposed copies | partials, its small inputs and results
    Buf bpcgrid{this}, bpcin{this}, bpcdraw{this}, bpcout{this}, bpcT{this}, bpcq{this};
    // CARMA entries (carma.hip): the batch's sampled parameters in1 | in2 | norm | flags, and what the kernels leave beside the coefficients (which
    // land where the value and gradient bodies read them, bA .. bD): the reverse mode's results, the PSD's per-draw roots | beta | factor | status
    Buf bcarma{this}, bcarmaout{this};
    std::vector<double> pcgrid_host;   // what bpcgrid is filled from: the device form returns before the copy has run
    double pcgrid_key[6] = {};         // ... and the (J, basis, f_min, f_max, S_low, S_high) it was built for
    // scalar entry point: the last series' time stamps stay resident (samplers call logl with the same t)
    pioran_ds* scalar_ds = nullptr;
    std::vector<double> scalar_t;
};

// Prepared shared-(c, d) state: table, row map, device copies of (c, d).  A data set holds TWO of them: `user` is what
// pioran_dataset_prepare declared for the asynchronous *_dev entries and is changed by nothing else; `host` is the
// scratch state of the host-pointer entries (logl_batch, mixed mode, theta, predict, grad), which prepare on their own.
struct PrepState {
    int32_t J = 0, R = 0;
    std::vector<double> c_host, d_host;
    std::vector<int32_t> real_host;
    DevArray<double> tab;
    DevArray<int32_t> rowmap;
    DevArray<double> dc;    // c | d
    double* dd = nullptr;   // ... the second half of it
    bool prepared = false;
    // mixed mode (term kind 2): indices of the per-draw terms, on the device
    int32_t npd_terms = 0;
    DevArray<int32_t> dpd_terms;
    // row layout class for the scan's configuration choice (ScanParams::standard_rows / n_complex)
    int32_t row_layout = 0, n_complex = 0;
    // table of the windowed kernel (celerite_block.hip), built on first use for the prepared (c, d)
    DevArray<double> btab;
    bool btab_ready = false;
};

struct pioran_ds {
    pioran_ctx* ctx = nullptr;
    int64_t N = 0;
    DevMem series;                                     // t | y | s2
    double *t = nullptr, *y = nullptr, *s2 = nullptr;  // ... and where each begins
    PrepState user, host;
};

namespace {

#define HIPCHK(ctx, expr)                                                                   \
    do {                                                                                    \
        hipError_t e_ = (expr);                                                             \
        if (e_ != hipSuccess) {                                                             \
            (ctx)->last_err = std::string(#expr) + ": " + hipGetErrorString(e_);            \
            return PIORAN_ERR_HIP;                                                          \
        }                                                                                   \
    } while (0)

// How much NEW device memory a call may take for its chunked workspaces (per-draw tables, factor stores, gradient / prediction
// workspaces): half of what is free, but never more than the context's absolute budget (option "workspace_limit_mb", default 16 GiB —
// the 256-draw chunks of every entry fit: per-draw windowed tables 9.5 GB, prediction 2.6 GB, gradient 6 GB at N = 1e4, J = 20), so
// that a co-resident allocator (torch's caching allocator, a second context) is not starved on a 288 GB device.  The buffers stay in
// the context until pioran_ctx_trim.
static size_t ws_allow(const pioran_ctx* ctx, size_t free_b)
{
    const size_t cap = (size_t)(ctx->opt.workspace_limit_mb > 0 ? ctx->opt.workspace_limit_mb : 16384) << 20;
    return free_b / 2 < cap ? free_b / 2 : cap;
}

// The device memory that is free right now; false when the runtime cannot tell (its error is cleared: the callers go on without the figure,
// and a later launch wrapper must not read it as its own)
static bool device_free_bytes(size_t& free_b)
{
    size_t total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) return true;
    (void)hipGetLastError();
    return false;
}

// May `b` hold `bytes` under the workspace budget?  The runtime is asked for the free memory only when the buffer would have to GROW: the
// asynchronous *_dev entries run this on every launch, and a launch that fits what is already allocated must not block on the host.
static bool ws_fits(pioran_ctx* ctx, const pioran_ctx::Buf& b, size_t bytes)
{
    if (bytes <= b.cap) return true;
    size_t free_b = 0;
    return device_free_bytes(free_b) && bytes <= ws_allow(ctx, free_b) + b.cap;
}

// `m` holds at least `bytes`: what it held is freed and `want` >= bytes allocated where it did not.  PIORAN_ERR_HIP: the runtime refused the free;
// PIORAN_ERR_ALLOC: there is no memory, and `m` is empty.
int grow(pioran_ctx* ctx, DevMem& m, size_t bytes, size_t want)
{
    if (bytes <= m.cap) return PIORAN_OK;
    HIPCHK(ctx, m.release());
    return m.alloc(want) ? PIORAN_OK : PIORAN_ERR_ALLOC;
}

int ensure(pioran_ctx* ctx, pioran_ctx::Buf& b, size_t bytes)
{
    const int rc = grow(ctx, b, bytes, bytes + (bytes < (size_t(1) << 28) ? bytes / 4 : 0) + 256);   // growth slack for small buffers only
    if (rc == PIORAN_ERR_ALLOC) ctx->last_err = "hipMalloc failed";
    return rc;
}

// ... with no slack: the prepared states' tables and the data set's series keep the size they are asked for
int ensure_exact(pioran_ctx* ctx, DevMem& m, size_t bytes) { return grow(ctx, m, bytes, bytes); }

struct BufNeed { pioran_ctx::Buf* b; size_t bytes; };
int ensure_each(pioran_ctx* ctx, std::initializer_list<BufNeed> needs)
{
    for (const BufNeed& n : needs)
        if (int rc = ensure(ctx, *n.b, n.bytes)) return rc;
    return PIORAN_OK;
}

// stream synchronisation + delivery of the results staged in pinned memory + reset of the staging allocator
int ctx_sync(pioran_ctx* ctx)
{
    const hipError_t e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        // nothing is delivered after a failed synchronisation, and nothing may be delivered LATER either: the caller's
        // buffers are only valid for the duration of the call that queued them
        ctx->pending.clear();
        ctx->pin_off = 0;
        ctx->last_err = std::string("hipStreamSynchronize: ") + hipGetErrorString(e);
        return PIORAN_ERR_HIP;
    }
    for (const auto& q : ctx->pending) std::memcpy(q.host, q.pinned, q.bytes);
    ctx->pending.clear();
    ctx->pin_off = 0;
    return PIORAN_OK;
}

// Every host-pointer entry opens with one of these: result deliveries queued by download() refer to memory the caller
// owns only until the entry returns, so an entry that leaves early (any error between download() and the final SYNC)
// must not leave them behind for the next successful ctx_sync of some later call.  On the normal path the queue is
// already empty when the guard runs.
struct PendingGuard {
    pioran_ctx* ctx;
    explicit PendingGuard(pioran_ctx* c) : ctx(c) {}
    ~PendingGuard()
    {
        if (ctx && !ctx->pending.empty()) {
            (void)hipStreamSynchronize(ctx->stream);   // the staged copies may still be in flight: the pinned slots are reused
            ctx->pending.clear();
            ctx->pin_off = 0;
        }
    }
};
#define SYNC(ctx)                      \
    do {                               \
        int rc_sync_ = ctx_sync(ctx);  \
        if (rc_sync_) return rc_sync_; \
    } while (0)

constexpr size_t kPinMaxRequest = size_t(32) << 20;   // larger transfers go straight from / to the caller's memory

// the pinned staging area back to the runtime (nothing in flight uses it: the callers have synchronised)
void pin_release(pioran_ctx* ctx)
{
    if (ctx->pin) (void)hipHostFree(ctx->pin);
    ctx->pin = nullptr;
    ctx->pin_cap = ctx->pin_off = 0;
}

// bytes of pinned staging, 256-byte aligned; nullptr when the request is too large for staging (or pinning fails)
void* pin_reserve(pioran_ctx* ctx, size_t bytes)
{
    if (bytes > kPinMaxRequest) return nullptr;
    const size_t need = (bytes + 255) & ~size_t(255);
    if (ctx->pin_off + need > ctx->pin_cap) {
        if (ctx_sync(ctx) != PIORAN_OK) return nullptr;           // nothing in flight uses the old buffer any more
        if (need > ctx->pin_cap) {
            pin_release(ctx);
            size_t want = need * 4 < (size_t(8) << 20) ? (size_t(8) << 20) : need * 4;
            if (hipHostMalloc((void**)&ctx->pin, want, hipHostMallocDefault) != hipSuccess) { ctx->pin = nullptr; return nullptr; }
            ctx->pin_cap = want;
        }
    }
    void* p = ctx->pin + ctx->pin_off;
    ctx->pin_off += need;
    return p;
}

// caller -> device memory `dev`: through pinned staging where it fits (the caller's memory is then free again), else directly
int upload_to(pioran_ctx* ctx, void* dev, const void* host, size_t bytes)
{
    const void* src = host;
    if (void* st = pin_reserve(ctx, bytes)) {
        std::memcpy(st, host, bytes);
        src = st;
    }
    HIPCHK(ctx, hipMemcpyAsync(dev, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    return PIORAN_OK;
}

int upload(pioran_ctx* ctx, pioran_ctx::Buf& b, const void* host, size_t bytes)
{
    const int rc = ensure(ctx, b, bytes);
    return rc ? rc : upload_to(ctx, b.p, host, bytes);
}

// device -> caller: through pinned staging (delivered by the next ctx_sync) where it fits, else directly
int download(pioran_ctx* ctx, void* host, const void* dev, size_t bytes)
{
    if (void* st = pin_reserve(ctx, bytes)) {
        HIPCHK(ctx, hipMemcpyAsync(st, dev, bytes, hipMemcpyDeviceToHost, ctx->stream));
        ctx->pending.push_back({host, st, bytes});
    } else {
        HIPCHK(ctx, hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, ctx->stream));
    }
    return PIORAN_OK;
}

// ---- what the batched entries share: launch descriptions, one chunk of draws up and down, the size of a chunk ------------------------------------
// element i of an array that may be absent
template <class T>
T* at(T* p, int64_t i) { return p ? p + i : nullptr; }

// Input arrays of some draws, a chunk's on the device or the caller's: A, Bc, C, D [.][J]; mu, nu [.] or nullptr; Y, S2 [.][N] or nullptr.
// (The caller's C, D are [J] where the draws share them: from_draw is for arrays that hold a row per draw.)
struct DrawChunk {
    const double *A, *Bc, *C, *D, *mu, *nu, *Y, *S2;
    DrawChunk from_draw(int64_t b0, int64_t J, int64_t N) const
    {
        return {A + b0 * J, Bc + b0 * J, at(C, b0 * J), at(D, b0 * J), at(mu, b0), at(nu, b0), at(Y, b0 * N), at(S2, b0 * N)};
    }
};

// Launch description of the nb draws `m` on a prepared shared-(c, d) state: everything the data set, the state and the chunk decide (m.C, m.D:
// not used).  out / status and what only one entry uses (gw, g_y, noise, npd_rows, ...) are the caller's.
ScanParams shared_params(const pioran_ds* ds, const PrepState& s, int64_t nb, const DrawChunk& m)
{
    ScanParams p{};
    p.opt = &ds->ctx->opt;
    p.A = m.A; p.Bc = m.Bc; p.mu = m.mu; p.nu = m.nu; p.Y = m.Y; p.S2 = m.S2;
    p.N = ds->N; p.J = s.J; p.R = s.R; p.B = nb;
    p.standard_rows = s.row_layout; p.n_complex = s.n_complex;
    p.rec_stride = rec_stride_of(s.R);
    p.tab = s.tab; p.rowmap = s.rowmap; p.t = ds->t; p.y = ds->y; p.s2 = ds->s2;
    p.C = s.dc; p.D = s.dd;
    return p;
}

// ... of nb draws with (c, d) of their own in every term (m.C, m.D; both rows of each of the J terms: R = 2 J, rowmap the full map): no shared
// table; the per-draw tables are tab_stride (reverse pass: gtab_stride) doubles apart, 0 where the entry has none
ScanParams perdraw_params(const pioran_ds* ds, int32_t J, int32_t R, const int32_t* rowmap, int64_t nb, const DrawChunk& m, int64_t tab_stride,
                          int64_t gtab_stride)
{
    ScanParams p{};
    p.opt = &ds->ctx->opt;
    p.A = m.A; p.Bc = m.Bc; p.mu = m.mu; p.nu = m.nu; p.Y = m.Y; p.S2 = m.S2;
    p.N = ds->N; p.J = J; p.R = R; p.B = nb; p.standard_rows = 1;
    p.rec_stride = rec_stride_of(R);
    p.tab_draw_stride = tab_stride; p.gtab_draw_stride = gtab_stride;
    p.rowmap = rowmap; p.t = ds->t; p.y = ds->y; p.s2 = ds->s2;
    p.C = m.C; p.D = m.D;
    return p;
}

// The windowed kernels' tables of a chunk of draws: the forward table, the reverse pass's (nullptr: the entry has none), and the doubles from one
// draw's table to the next (0: one table for all draws, shared (c, d)).  Filled by build_tables (below, after ensure_btab).
struct ChunkTables { const double *btab = nullptr, *gtab = nullptr; int64_t bstride = 0, gstride = 0; };

// Launch description of the nb draws `m` of an entry that serves both forms: on the prepared state `s` (shared (c, d)), or, per_draw, with the
// row map of `s` and the chunk's own tables
ScanParams chunk_params(const pioran_ds* ds, const PrepState& s, bool per_draw, int64_t nb, const DrawChunk& m, const ChunkTables& tb)
{
    return per_draw ? perdraw_params(ds, s.J, s.R, s.rowmap, nb, m, tb.bstride, tb.gstride) : shared_params(ds, s, nb, m);
}

// Runs one(b) — draw b as a call of its own — for every draw of a batch; the first error ends it.  Where (c, d) per draw do not fit the windowed
// kernels with per-draw tables, every draw is a one-draw batch with its own shared table.
template <class One>
int each_draw(int64_t B, One one)
{
    for (int64_t b = 0; b < B; ++b)
        if (const int rc = one(b)) return rc;
    return PIORAN_OK;
}

// Draws [b0, b0 + nb) of the caller's host arrays into the context's staging buffers bA .. bnu.  C / Dd, mu, nu: nullptr = not part of the
// call (a shared (c, d) lives in the prepared state), and the chunk's pointer is nullptr then.
int upload_draws(pioran_ctx* ctx, int64_t J, int64_t b0, int64_t nb, const double* A, const double* Bc, const double* C, const double* Dd,
                 const double* mu, const double* nu, DrawChunk& m)
{
    int rc;
    const size_t bj = (size_t)nb * (size_t)J * sizeof(double);
    if ((rc = upload(ctx, ctx->bA, A + b0 * J, bj))) return rc;
    if ((rc = upload(ctx, ctx->bB, Bc + b0 * J, bj))) return rc;
    if (C && (rc = upload(ctx, ctx->bC, C + b0 * J, bj))) return rc;
    if (C && (rc = upload(ctx, ctx->bD, Dd + b0 * J, bj))) return rc;
    if (mu && (rc = upload(ctx, ctx->bmu, mu + b0, nb * sizeof(double)))) return rc;
    if (nu && (rc = upload(ctx, ctx->bnu, nu + b0, nb * sizeof(double)))) return rc;
    m = DrawChunk{};
    m.A = (const double*)ctx->bA.p; m.Bc = (const double*)ctx->bB.p;
    if (C) { m.C = (const double*)ctx->bC.p; m.D = (const double*)ctx->bD.p; }
    m.mu = mu ? (const double*)ctx->bmu.p : nullptr; m.nu = nu ? (const double*)ctx->bnu.p : nullptr;
    return PIORAN_OK;
}

// approx on the device as the source of a batch's draws, and its reverse mode as the sink of their gradients (approx.hip): the sampled parameters of the
// whole batch and the grid's constants on the device (bthin), a chunk's results (bthout), the caller's arrays, and what the grid says of the terms
struct ThetaDraws {
    int model = 0, P = 0, J = 0, basis = 0, integrated = 0;
    double f_min = 0.0, f_max = 0.0;
    const double *sp = nullptr, *w = nullptr, *LU = nullptr, *theta = nullptr, *norm = nullptr;
    const int32_t* piv = nullptr;
    double *grad_theta = nullptr, *grad_norm = nullptr;          // the caller's: [B][P], [B]
    int n_qpo = 0;                                               // QPO features per draw (the entries that chain through approx_qpo_vjp_kernel) ...
    const double* qpo = nullptr;                                 // ... and their (S0, f0, Q) [B][n_qpo][3] on the device, behind norm
    std::vector<double> grid, c, d;                              // host: sp | w | LU | piv (what `sp` .. `piv` hold), the shared (c, d) of the celerite terms
    std::vector<int32_t> real;                                   // ... and which of them keep their cos row only
    int64_t terms() const { return basis == 0 ? J : 2 * (int64_t)J; }
};

// The grid of approx and the batch's theta [B][P], norm [B] onto the device.  `td` keeps the host copies until the call's last synchronisation.
int stage_theta(pioran_ctx* ctx, int64_t B, int model, int64_t J, int basis, int integrated, double f_min, double f_max, double S_low, double S_high,
                const double* theta, const double* norm, ThetaDraws& td, int64_t n_qpo = 0, const double* qpo = nullptr)
{
    std::vector<double> sp, w, LU;
    std::vector<int32_t> piv;
    int rc = pioran_approx_setup_host(J, basis, f_min, f_max, S_low, S_high, sp, LU, piv, td.c, td.d, td.real);
    if (rc) return rc;
    pioran_approx_weights_host(basis, integrated, f_min, f_max, sp, w);
    td.model = model; td.P = model == 0 ? 3 : 5; td.J = (int)J; td.basis = basis; td.integrated = integrated; td.f_min = f_min; td.f_max = f_max;
    const size_t nJ = (size_t)J, npiv = (nJ + 1) / 2, ngrid = 2 * nJ + nJ * nJ + npiv, nth = (size_t)B * td.P;
    td.grid.assign(ngrid, 0.0);
    std::memcpy(td.grid.data(), sp.data(), nJ * sizeof(double));
    std::memcpy(td.grid.data() + nJ, w.data(), nJ * sizeof(double));
    std::memcpy(td.grid.data() + 2 * nJ, LU.data(), nJ * nJ * sizeof(double));
    std::memcpy(td.grid.data() + 2 * nJ + nJ * nJ, piv.data(), nJ * sizeof(int32_t));
    const size_t nq = (size_t)B * 3 * (size_t)n_qpo;
    if ((rc = ensure(ctx, ctx->bthin, (ngrid + nth + (size_t)B + nq) * sizeof(double)))) return rc;
    double* dev = (double*)ctx->bthin.p;
    if ((rc = upload_to(ctx, dev, td.grid.data(), ngrid * sizeof(double)))) return rc;
    if ((rc = upload_to(ctx, dev + ngrid, theta, nth * sizeof(double)))) return rc;
    if ((rc = upload_to(ctx, dev + ngrid + nth, norm, (size_t)B * sizeof(double)))) return rc;
    if (nq && (rc = upload_to(ctx, dev + ngrid + nth + B, qpo, nq * sizeof(double)))) return rc;
    td.n_qpo = (int)n_qpo; td.qpo = nq ? dev + ngrid + nth + B : nullptr;
    td.sp = dev; td.w = dev + nJ; td.LU = dev + 2 * nJ; td.piv = (const int32_t*)(dev + 2 * nJ + nJ * nJ);
    td.theta = dev + ngrid; td.norm = dev + ngrid + nth;
    return PIORAN_OK;
}

// a chunk's grad_theta [nb][P] | grad_norm [nb] | the reverse kernel's scratch [2 J][nb] | with features, grad_qpo [nb][n_qpo][3] in bthout
int ensure_theta_grads(pioran_ctx* ctx, const ThetaDraws& td, int64_t nb)
{
    return ensure(ctx, ctx->bthout, (size_t)nb * (size_t)(td.P + 1 + 2 * td.J + 3 * td.n_qpo) * sizeof(double));
}

// (ga, gb) [nb][terms] of draws [b0, b0 + nb), on the device, through the reverse mode of approx to the caller's grad_theta, grad_norm
int theta_grads(pioran_ctx* ctx, const ThetaDraws& td, int64_t b0, int64_t nb, const double* ga, const double* gb)
{
    double* gth = (double*)ctx->bthout.p; double* gn = gth + (size_t)nb * td.P;
    int rc = pioran_launch_approx_vjp(nb, td.model, td.P, td.J, td.basis, td.sp, td.w, td.LU, td.piv, td.theta + b0 * td.P, td.norm + b0, ga, gb, gn + nb,
                                      gth, gn, ctx->stream);
    if (rc) return rc;
    if ((rc = download(ctx, td.grad_theta + b0 * td.P, gth, (size_t)nb * td.P * sizeof(double)))) return rc;
    return download(ctx, td.grad_norm + b0, gn, (size_t)nb * sizeof(double));
}

// Where a chunk's draws come from: draws [b0, b0 + nb) of the caller's host arrays `in` (upload_draws; per_draw: with their (c, d)), or, `td`,
// approx_kernel's coefficients of the sampled parameters, written into the staging buffers upload_draws would have filled (mu, nu: the caller's, `in`'s).
// J counts the features' terms where `td` has any: their (a, b) are the last columns of the rows, and their (c, d) land in the same columns of bC / bD.
int stage_draws(pioran_ctx* ctx, int64_t J, int64_t b0, int64_t nb, const DrawChunk& in, bool per_draw, const ThetaDraws* td, DrawChunk& m)
{
    if (!td) return upload_draws(ctx, J, b0, nb, in.A, in.Bc, per_draw ? in.C : nullptr, in.D, in.mu, in.nu, m);
    int rc;
    const size_t bj = (size_t)nb * (size_t)J * sizeof(double);
    if ((rc = ensure_each(ctx, {{&ctx->bA, bj}, {&ctx->bB, bj}, {&ctx->bC, td->n_qpo ? bj : 0}, {&ctx->bD, td->n_qpo ? bj : 0}}))) return rc;
    if (in.mu && (rc = upload(ctx, ctx->bmu, in.mu + b0, nb * sizeof(double)))) return rc;
    if (in.nu && (rc = upload(ctx, ctx->bnu, in.nu + b0, nb * sizeof(double)))) return rc;
    m = DrawChunk{};
    m.A = (const double*)ctx->bA.p; m.Bc = (const double*)ctx->bB.p;
    if (td->n_qpo) { m.C = (const double*)ctx->bC.p; m.D = (const double*)ctx->bD.p; }
    m.mu = in.mu ? (const double*)ctx->bmu.p : nullptr; m.nu = in.nu ? (const double*)ctx->bnu.p : nullptr;
    return pioran_launch_approx(nb, td->model, td->P, td->J, td->basis, td->integrated, td->f_min, td->f_max, td->sp, td->LU, td->piv,
                                td->theta + b0 * td->P, td->norm + b0, td->n_qpo, at(td->qpo, b0 * 3 * td->n_qpo), (double*)ctx->bA.p, (double*)ctx->bB.p,
                                (double*)m.C, (double*)m.D, ctx->stream);
}

// log L and status of n draws land in bout / bst ...
int ensure_results(pioran_ctx* ctx, int64_t n)
{
    const int rc = ensure(ctx, ctx->bout, n * sizeof(double));
    return rc ? rc : ensure(ctx, ctx->bst, n * sizeof(int32_t));
}

// ... and go from there to the caller's arrays at draw b0 (out, status: nullptr = not wanted)
int download_results(pioran_ctx* ctx, double* out, int32_t* status, int64_t b0, int64_t nb)
{
    int rc;
    if (out && (rc = download(ctx, out + b0, ctx->bout.p, nb * sizeof(double)))) return rc;
    if (status && (rc = download(ctx, status + b0, ctx->bst.p, nb * sizeof(int32_t)))) return rc;
    return PIORAN_OK;
}

// Gradient arrays, the caller's or a chunk's on the device: a, b, c, d [.][J]; nu, mu [.]; y, s2 [.][N].  In the caller's set everything but
// a and b may be nullptr (not wanted); a and b too where the call chains them on (ThetaDraws).
struct GradPtrs {
    double *a, *b, *c, *d, *nu, *mu, *y, *s2;
    GradPtrs from_draw(int64_t b0, int64_t J, int64_t N) const
    {
        return {at(a, b0 * J), at(b, b0 * J), at(c, b0 * J), at(d, b0 * J), at(nu, b0), at(mu, b0), at(y, b0 * N), at(s2, b0 * N)};
    }
};

// the device side of a chunk: grad_a | grad_b | grad_c | grad_d ([chunk][J] each) in `terms`, grad_nu | grad_mu ([chunk] each) in `scalars`,
// the series gradients in bY / bS2
GradPtrs grad_chunk(pioran_ctx* ctx, const pioran_ctx::Buf& terms, const pioran_ctx::Buf& scalars, int64_t chunk, int64_t J)
{
    double* ga = (double*)terms.p; double* gn = (double*)scalars.p;
    const size_t cj = (size_t)chunk * (size_t)J;
    return {ga, ga + cj, ga + 2 * cj, ga + 3 * cj, gn, gn + chunk, (double*)ctx->bY.p, (double*)ctx->bS2.p};
}

// nb draws of a chunk's gradients to the caller's arrays (host: already at the chunk's first draw)
int download_grads(pioran_ctx* ctx, const GradPtrs& host, const GradPtrs& dev, int64_t nb, int64_t J, int64_t N)
{
    int rc;
    const size_t nbj = (size_t)nb * J * sizeof(double), nbn = (size_t)nb * N * sizeof(double);
    if (host.a && (rc = download(ctx, host.a, dev.a, nbj))) return rc;
    if (host.b && (rc = download(ctx, host.b, dev.b, nbj))) return rc;
    if (host.c && (rc = download(ctx, host.c, dev.c, nbj))) return rc;
    if (host.d && (rc = download(ctx, host.d, dev.d, nbj))) return rc;
    if (host.nu && (rc = download(ctx, host.nu, dev.nu, nb * sizeof(double)))) return rc;
    if (host.mu && (rc = download(ctx, host.mu, dev.mu, nb * sizeof(double)))) return rc;
    if (host.y && (rc = download(ctx, host.y, dev.y, nbn))) return rc;
    if (host.s2 && (rc = download(ctx, host.s2, dev.s2, nbn))) return rc;
    return PIORAN_OK;
}

// Sizing a chunk of draws.  `chunk` is halved while need(chunk) bytes of workspace exceed what the call may newly take (ws_allow) plus what
// the buffers in `held`, the ones need() counts, hold already, and halved again while ensure_all(chunk), which grows every buffer the chunk needs,
// cannot allocate.  Returns ensure_all's code for the chunk it leaves in `chunk`.  shrink = false (EntryPlan::shrink: the plans that leave the
// windowed kernels when memory is short): no second halving, PIORAN_ERR_ALLOC for the chunk the budget admits.
using BufList = std::initializer_list<const pioran_ctx::Buf*>;
template <class Need, class EnsureAll>
int size_chunk(pioran_ctx* ctx, int64_t& chunk, BufList held, Need need, EnsureAll ensure_all, bool shrink = true)
{
    size_t free_b = 0;
    if (device_free_bytes(free_b)) {
        size_t allowed = ws_allow(ctx, free_b);
        for (const pioran_ctx::Buf* b : held) allowed += b->cap;
        while (chunk > 1 && need(chunk) > allowed) chunk /= 2;
    }
    for (;;) {
        const int rc = ensure_all(chunk);
        if (rc != PIORAN_ERR_ALLOC || chunk == 1 || !shrink) return rc;
        chunk /= 2;
    }
}

// second stream + events of the gradient's reverse pass and of the remainder launch (split_dispatch): created on first use
int ensure_aux(pioran_ctx* ctx)
{
    if (ctx->aux) return PIORAN_OK;
    HIPCHK(ctx, hipStreamCreateWithFlags(&ctx->aux, hipStreamNonBlocking));
    for (auto& e : ctx->gev) HIPCHK(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    return PIORAN_OK;
}

// 1: ascending (ties allowed), 0: not — or a NaN among the times
int is_sorted(const double* t, int64_t N)
{
    for (int64_t i = 1; i < N; ++i)
        if (!(t[i] >= t[i - 1])) return 0;
    return 1;
}

// A data set that lives for one call: the simulation's series of zeros on the caller's time stamps
struct ScopedDataset {
    pioran_ds* ds = nullptr;
    std::vector<double> zeros;
    ~ScopedDataset() { if (ds) pioran_dataset_destroy(ds); }
    int create_zeros(pioran_ctx* ctx, int64_t N, const double* t, const double* sigma2)
    {
        zeros.assign((size_t)N, 0.0);
        return pioran_dataset_create(ctx, N, t, zeros.data(), sigma2, &ds);
    }
};

// rows kept for a term list.  kind[j]: 0 = shared (c, d): cos + sin row from the shared table;
//   1 = "real" term (b = d = 0 for every draw): cos row only; 2 = per-draw (c, d): cos + sin row from the per-draw table.
// Encoding: term (bits 0-19) | per-draw row index (20-28) | per-draw flag (29) | sin row (30).
std::vector<int32_t> build_rowmap(int64_t J, const int32_t* kind)
{
    // shared rows first, the rows of the per-draw terms LAST (in term order, cos row then sin row): every kernel reads the row
    // map, none assumes an order, and the windowed kernel relies on the per-draw rows being the last ones (celerite_block.hip)
    std::vector<int32_t> rm;
    rm.reserve(2 * J);
    for (int64_t j = 0; j < J; ++j) {
        const int32_t k = kind ? kind[j] : 0;
        if (k == 2) continue;
        rm.push_back((int32_t)j);
        if (k != 1) rm.push_back((int32_t)j | (1 << 30));
    }
    int32_t npd = 0;
    for (int64_t j = 0; j < J; ++j) {
        if (!kind || kind[j] != 2) continue;
        rm.push_back((int32_t)j | ((2 * npd) << 20) | (1 << 29));
        rm.push_back((int32_t)j | ((2 * npd + 1) << 20) | (1 << 29) | (1 << 30));
        ++npd;
    }
    return rm;
}

int set_rowmap(pioran_ds* ds, PrepState& s, const std::vector<int32_t>& rm)
{
    pioran_ctx* ctx = ds->ctx;
    if (const int rc = ensure_exact(ctx, s.rowmap, rm.size() * sizeof(int32_t))) return rc;
    HIPCHK(ctx, hipMemcpyAsync(s.rowmap, rm.data(), rm.size() * sizeof(int32_t), hipMemcpyHostToDevice,
                               ctx->stream));
    // the host vector is about to go out of scope in the callers: finish the copy first
    SYNC(ctx);
    s.R = (int32_t)rm.size();
    return PIORAN_OK;
}

thread_local const char* g_last_kernel = "none";   // which kernel family the calling thread's last launch ran on (diagnostics)

// A launch of the sampled-parameter kernels (approx with features, carma.hip): the family's name for the diagnostics, the launch between the events
// ev0, ev0 + 1 where the call is timed, and the entry's text for a launch the runtime refused
template <class Launch>
int timed_launch(pioran_ctx* ctx, const char* name, int ev0, bool timed, const char* err_text, Launch launch)
{
    g_last_kernel = name;
    if (timed) HIPCHK(ctx, hipEventRecord(ctx->ev[ev0], ctx->stream));
    if (const int rc = launch()) {
        if (rc == PIORAN_ERR_HIP) ctx->last_err = err_text;
        return rc;
    }
    if (timed) HIPCHK(ctx, hipEventRecord(ctx->ev[ev0 + 1], ctx->stream));
    return PIORAN_OK;
}

// The caller's cotangent arrays, n doubles each, one behind the other in bK (where the gradient entries keep a chunk's: grad_chunk); dev: the first
int upload_cotangents(pioran_ctx* ctx, std::initializer_list<const double*> host, size_t n, double*& dev)
{
    int rc;
    if ((rc = ensure(ctx, ctx->bK, host.size() * n * sizeof(double)))) return rc;
    dev = (double*)ctx->bK.p;
    size_t k = 0;
    for (const double* h : host)
        if ((rc = upload_to(ctx, dev + k++ * n, h, n * sizeof(double)))) return rc;
    return PIORAN_OK;
}

// ---- the value path: which family takes a launch is route.hip's to say; here the family's table, workspace, second stream are acquired and it is launched ----
// The prepared state whose shared table a launch reads, if it is one without per-draw terms.  What else a family needs of it is a second test at its
// call: the windowed families (tile, block, split; the time-parallel family's repair pass) read the state's own step records (own_records); the
// time-parallel family itself reads only the device copies of (c, d) — `s->dc && s->dd`, whatever the record stride.
PrepState* plain_state(pioran_ds* ds, const ScanParams& p)
{
    PrepState* s = p.tab == ds->user.tab ? &ds->user : (p.tab == ds->host.tab ? &ds->host : nullptr);
    return s && s->prepared && s->npd_terms == 0 ? s : nullptr;
}
bool own_records(const ScanParams& p, const PrepState& s) { return p.rec_stride == rec_stride_of(s.R); }

// what the rules read of a launch (ds = nullptr: a launch with no prepared state to look at — mixed_core's combined table)
RouteQuery route_query(pioran_ds* ds, const ScanParams& p)
{
    static const ScanOptions kDefaults{};
    RouteQuery q{p.R, p.J, p.B, p.N, p.tab != nullptr, p.npd_rows, p.Y != nullptr, 0, 0, false, false, p.opt ? *p.opt : kDefaults};
    if (const PrepState* s = ds ? plain_state(ds, p) : nullptr) {
        q.plain_state = true;
        q.own_records = own_records(p, *s);
        for (int j = 0; j < s->J; ++j) ++(s->real_host[j] ? q.n_one_row : q.n_two_row);
    }
    return q;
}

int scan_dispatch(const ScanParams& p, hipStream_t stream)
{
    switch (scan_family(route_query(nullptr, p))) {
        case ScanFamily::wide: g_last_kernel = "wide"; return pioran_launch_scan_wide(p, stream);
        case ScanFamily::scan: g_last_kernel = "scan"; return pioran_launch_scan(p, stream);
        default: return PIORAN_ERR_UNSUPPORTED;
    }
}

// the windowed kernel's own table of a prepared (c, d): built on first use (PIORAN_ERR_UNSUPPORTED: too long a series / no memory)
int ensure_btab(pioran_ds* ds, PrepState& s)
{
    pioran_ctx* ctx = ds->ctx;
    if (s.btab_ready) return PIORAN_OK;
    // 60 KB per 16 time stamps at J = 20: very long series (or a device short of memory) stay on the other kernels
    const size_t need = pioran_block_table_doubles(ds->N, s.R, s.J);
    if (need * sizeof(double) > (size_t(2) << 30)) return PIORAN_ERR_UNSUPPORTED;
    int rc = ensure_exact(ctx, s.btab, need * sizeof(double));
    if (rc) return rc == PIORAN_ERR_ALLOC ? PIORAN_ERR_UNSUPPORTED : rc;
    rc = ctx->opt.btab_reference
                 ? pioran_launch_block_table_reference(ds->N, s.R, s.J, s.rowmap, ds->t, s.dc, s.dd, ds->y, ds->s2, s.btab, ctx->stream)
                 : pioran_launch_block_table(ds->N, s.R, s.J, s.rowmap, ds->t, s.dc, s.dd, ds->y, ds->s2, s.btab, ctx->stream);
    if (rc) return rc;
    s.btab_ready = true;
    return PIORAN_OK;
}

// The plan of an entry (route.hip entry_plan) for the prepared state; a refusal comes before any upload or workspace.  A plan on the windowed kernels
// can run on them with (c, d) per draw, which bring their own tables, and with a shared (c, d) where the state's forward table can be had: it is built
// here on first use, and the plan leaves the windowed kernels where it cannot
int plan_entry(pioran_ds* ds, PrepState& s, Entry entry, int64_t B, bool per_draw, int grad_flags, EntryPlan& plan)
{
    plan = entry_plan(entry, s.R, s.J, s.npd_terms, B, per_draw, grad_flags, ds->ctx->opt);
    if (plan.rc || !plan.windowed || per_draw) return plan.rc;
    const int rc = ensure_btab(ds, s);
    if (rc == PIORAN_ERR_UNSUPPORTED) plan.leave_windowed();
    return rc == PIORAN_ERR_UNSUPPORTED ? PIORAN_OK : rc;
}

// The tables of a windowed launch; a chunk loop calls this for shared (c, d) ONCE PER CALL — the state's forward table
// (windowed_ready) and the reverse table, built into `gbuf` — and for (c, d) per draw ONCE PER CHUNK: one pair per draw of the nb draws `m`, into `bbuf`
// and `gbuf`.  gbuf = nullptr: the entry has no reverse pass.  The buffers hold the tables already (the entry's chunk sizing).
int build_tables(pioran_ds* ds, const PrepState& s, bool per_draw, int64_t nb, const DrawChunk& m, const pioran_ctx::Buf& bbuf, const pioran_ctx::Buf* gbuf,
                 ChunkTables& tb)
{
    hipStream_t stream = ds->ctx->stream;
    double* const gtab = gbuf ? (double*)gbuf->p : nullptr;
    tb = ChunkTables{};
    tb.gtab = gtab;
    if (!per_draw) {
        tb.btab = s.btab;
        return gtab ? pioran_launch_block_gtab(ds->N, s.R, s.J, s.rowmap, ds->t, s.dc, s.dd, ds->s2, gtab, stream) : PIORAN_OK;
    }
    tb.btab = (const double*)bbuf.p;
    tb.bstride = (int64_t)pioran_block_table_doubles(ds->N, s.R, s.J);
    tb.gstride = gtab ? (int64_t)pioran_block_gtab_doubles(ds->N, s.R) : 0;
    int rc = pioran_launch_block_table_batch(ds->N, s.R, s.J, nb, s.rowmap, ds->t, m.C, m.D, ds->y, ds->s2, (double*)bbuf.p, tb.bstride, stream);
    if (!rc && gtab) rc = pioran_launch_block_gtab_batch(ds->N, s.R, s.J, nb, s.rowmap, ds->t, m.C, m.D, ds->s2, gtab, tb.gstride, stream);
    return rc;
}
// The dispatchers of launch(): PIORAN_ERR_UNSUPPORTED when the launch is not the family's (the caller goes on to the next one).
int block_dispatch(pioran_ds* ds, const ScanParams& p, const RouteQuery& q)
{
    if (!block_wanted(q)) return PIORAN_ERR_UNSUPPORTED;
    PrepState* s = plain_state(ds, p);
    int rc = ensure_btab(ds, *s);
    if (rc) return rc;
    g_last_kernel = "block";
    return pioran_launch_scan_block(p, s->btab, ds->ctx->stream);
}

static ScanParams slice_draws(const ScanParams& p, int64_t off, int64_t n)
{
    ScanParams q = p;
    q.B = n;
    q.A = p.A + off * p.J; q.Bc = p.Bc + off * p.J;
    if (p.mu) q.mu = p.mu + off;
    if (p.nu) q.nu = p.nu + off;
    if (p.Y) q.Y = p.Y + off * p.N;
    if (p.S2) q.S2 = p.S2 + off * p.N;
    q.out = p.out + off;
    if (p.status) q.status = p.status + off;
    if (p.only_if) q.only_if = p.only_if + off;     // (per draw: celerite_block_kernel)
    return q;
}
int tp_dispatch(pioran_ds* ds, const ScanParams& p, const RouteQuery& rq)
{
    pioran_ctx* ctx = ds->ctx;
    const ScanOptions& o = ctx->opt;
    const TpPlan plan = tp_plan(rq);
    PrepState* s = plan.take ? plain_state(ds, p) : nullptr;
    if (!s || !s->dc || !s->dd) return PIORAN_ERR_UNSUPPORTED;
    // state rows: the two-row terms first (pairs on even / odd lanes), then the one-row terms, padded to the plan's count
    const int J = s->J, RP = plan.RP, nseg = plan.nseg;
    std::vector<int32_t> rows;
    rows.reserve(256);
    std::vector<int32_t> term, kind;
    for (int j = 0; j < J; ++j)
        if (!s->real_host[j]) { term.push_back(j); kind.push_back(0); term.push_back(j); kind.push_back(1); }
    for (int j = 0; j < J; ++j)
        if (s->real_host[j]) { term.push_back(j); kind.push_back(2); }
    while ((int)term.size() < RP) { term.push_back(0); kind.push_back(3); }
    rows = term;
    rows.insert(rows.end(), kind.begin(), kind.end());
    int rc = upload(ctx, ctx->btprow, rows.data(), rows.size() * sizeof(int32_t));
    if (rc) return rc;
    // (B N (6 RP + 5) doubles of records + 133 KB per (draw, segment): 25 GB for eight draws of 64 rows at N = 1e6 — under the same budget as every
    //  other chunked workspace; over it the serial-chain kernels take the call)
    if (!ws_fits(ctx, ctx->btp, pioran_tp_workspace_doubles(p.B, p.N, RP, nseg) * sizeof(double))) return PIORAN_ERR_UNSUPPORTED;
    rc = ensure(ctx, ctx->btp, pioran_tp_workspace_doubles(p.B, p.N, RP, nseg) * sizeof(double));
    if (rc) return rc == PIORAN_ERR_ALLOC ? PIORAN_ERR_UNSUPPORTED : rc;
    ScanParams q = p;
    q.C = s->dc; q.D = s->dd; q.J = J; q.opt = &ctx->opt;
    g_last_kernel = "tp";
    const int32_t* dr = (const int32_t*)ctx->btprow.p;
    // the repair pass (tp_repair_wanted) needs the windowed kernel's table
    bool repair = tp_repair_wanted(rq) && (p.Y == nullptr) == (p.S2 == nullptr);
    if (repair) {
        rc = ensure_btab(ds, *s);
        if (rc == PIORAN_ERR_UNSUPPORTED) repair = false;
        else if (rc) return rc;
    }
    const int mode = tp_mode(plan, repair, o);
    if (mode < 0) return PIORAN_ERR_UNSUPPORTED;
    rc = pioran_launch_tp(q, RP, nseg, plan.L, dr, dr + RP, (double*)ctx->btp.p, ctx->stream, mode);
    if (rc || !repair) return rc;
    ScanParams qr = p;
    qr.only_if = pioran_tp_disc((const double*)ctx->btp.p, p.B, p.N, RP, nseg);
    qr.only_if_tol = pioran_tp_scan_tol(&ctx->opt);
    rc = pioran_launch_scan_block(qr, s->btab, ctx->stream);
    if (rc == PIORAN_ERR_UNSUPPORTED) {
        ctx->last_err = "time-parallel scan: the serial-chain repair pass refused a launch its own conditions admit";
        return PIORAN_ERR_HIP;
    }
    return rc;
}

int tile_dispatch(pioran_ds* ds, const ScanParams& p, const RouteQuery& q)
{
    pioran_ctx* ctx = ds->ctx;
    if (!tile_wanted(q, [&] { return pioran_scan_pass_draws(p, nullptr); })) return PIORAN_ERR_UNSUPPORTED;
    PrepState* s = plain_state(ds, p);
    int rc = ensure_btab(ds, *s);
    if (rc) return rc;
    // workspace: 1 KB per draw and window (the windows' own covariance blocks); large batches in chunks of whole passes
    const int64_t pass = pioran_tile_pass_draws(p.R, ctx->ncu);
    int64_t chunk = p.B;
    while (chunk > pass && !ws_fits(ctx, ctx->bpair, pioran_tile_workspace_doubles(chunk, p.N) * sizeof(double)))
        chunk = ((chunk / 2 + pass - 1) / pass) * pass;
    if (!ws_fits(ctx, ctx->bpair, pioran_tile_workspace_doubles(chunk, p.N) * sizeof(double))) return PIORAN_ERR_UNSUPPORTED;
    rc = ensure(ctx, ctx->bpair, pioran_tile_workspace_doubles(chunk, p.N) * sizeof(double));
    if (rc) return rc == PIORAN_ERR_ALLOC ? PIORAN_ERR_UNSUPPORTED : rc;
    g_last_kernel = "tile";
    for (int64_t off = 0; off < p.B; off += chunk) {
        const ScanParams qc = slice_draws(p, off, p.B - off < chunk ? p.B - off : chunk);
        rc = pioran_launch_scan_tile(qc, s->btab, (double*)ctx->bpair.p, ctx->stream);
        if (rc) return rc;
    }
    return PIORAN_OK;
}

// The remainder of a multi-pass batch (split_plan) on the windowed kernel on the context's second stream, launched first, while the whole passes run
// on the main stream.  The two launches write disjoint slices of out / status; the main stream waits for the second one's event, so the call is
// stream-ordered like any other.
int split_dispatch(pioran_ds* ds, const ScanParams& p, const RouteQuery& q)
{
    pioran_ctx* ctx = ds->ctx;
    const int64_t main_n = split_plan(q, [&] { return pioran_scan_pass_draws(p, nullptr); });
    if (main_n <= 0) return PIORAN_ERR_UNSUPPORTED;
    PrepState* s = plain_state(ds, p);
    int rc = ensure_btab(ds, *s);
    if (rc) return rc;
    if ((rc = ensure_aux(ctx))) return rc;
    // fork: the second stream sees everything the main stream has queued so far (inputs, tables)
    HIPCHK(ctx, hipEventRecord(ctx->gev[3], ctx->stream));
    HIPCHK(ctx, hipStreamWaitEvent(ctx->aux, ctx->gev[3], 0));
    ScanParams qr = slice_draws(p, main_n, p.B - main_n);
    rc = pioran_launch_scan_block(qr, s->btab, ctx->aux);
    if (rc) { if (rc == PIORAN_ERR_HIP) ctx->last_err = "block kernel launch failed"; return rc; }
    HIPCHK(ctx, hipEventRecord(ctx->gev[4], ctx->aux));
    ScanParams qm = slice_draws(p, 0, main_n);
    rc = scan_dispatch(qm, ctx->stream);
    HIPCHK(ctx, hipStreamWaitEvent(ctx->stream, ctx->gev[4], 0));   // join — on every path: the second stream's kernel writes the caller's buffers
    if (rc) { if (rc == PIORAN_ERR_HIP) ctx->last_err = "scan kernel launch failed"; return rc == PIORAN_ERR_UNSUPPORTED ? PIORAN_ERR_HIP : rc; }
    g_last_kernel = "scan + block (remainder)";
    return PIORAN_OK;
}

int scan_or_wide_dispatch(pioran_ds* ds, const ScanParams& p, const RouteQuery&)
{
    return p.R <= pioran_wide_supported_rows() ? scan_dispatch(p, ds->ctx->stream) : PIORAN_ERR_UNSUPPORTED;
}

int launch(pioran_ds* ds, ScanParams& p)
{
    pioran_ctx* ctx = ds->ctx;
    p.opt = &ctx->opt;
    // the ladder: the first family that does not refuse (PIORAN_ERR_UNSUPPORTED) has the launch; what last_err says when its launch fails
    // (split_dispatch names the failing kernel itself)
    static constexpr struct { int (*dispatch)(pioran_ds*, const ScanParams&, const RouteQuery&); const char* failed; } kLadder[] = {
        {tp_dispatch, "time-parallel kernel launch failed"}, {tile_dispatch, "tile kernel launch failed"}, {block_dispatch, "block kernel launch failed"},
        {split_dispatch, nullptr}, {scan_or_wide_dispatch, "scan kernel launch failed"}};
    if (!ctx->opt.force_fallback) {
        const RouteQuery q = route_query(ds, p);
        for (const auto& step : kLadder) {
            const int rc = step.dispatch(ds, p, q);
            if (rc == PIORAN_ERR_UNSUPPORTED) continue;
            if (rc == PIORAN_ERR_HIP && step.failed) ctx->last_err = step.failed;
            return rc;
        }
    }
    const int64_t chunk = p.B < 1024 ? p.B : 1024;
    int rc = ensure(ctx, ctx->bscratch, (size_t)chunk * pioran_fallback_scratch_doubles(p.R) * sizeof(double));
    if (rc) return rc;
    p.scratch = (double*)ctx->bscratch.p;
    g_last_kernel = "fallback";
    rc = pioran_launch_scan_fallback(p, ctx->stream);
    if (rc == PIORAN_ERR_HIP) ctx->last_err = "fallback kernel launch failed";
    return rc;
}

// `value` of option `key` into a set of options (pioran_ctx_set_option; the option string of pioran_value_route)
int set_option(ScanOptions& o, const char* key, const char* value)
{
    const bool on = value && value[0] && std::strcmp(value, "0") != 0;
    if (!std::strcmp(key, "scan_config")) {
        if (value && std::strlen(value) >= sizeof(o.scan_config)) return PIORAN_ERR_ARG;
        std::memset(o.scan_config, 0, sizeof(o.scan_config));
        // "tile": celerite_tile.hip for every launch it can take (any batch size); the launches it cannot take stay automatic
        o.force_tile = value && !std::strcmp(value, "tile");
        o.force_tp = value && !std::strcmp(value, "tp");
        if (value && !o.force_tile && !o.force_tp) std::strcpy(o.scan_config, value);
    } else if (!std::strcmp(key, "no_tp")) o.no_tp = on; else if (!std::strcmp(key, "tp_segments")) o.tp_segments = (value && value[0]) ? std::atoi(value) : 0;
    else if (!std::strcmp(key, "tp_scan")) o.tp_scan = (value && value[0]) ? std::atoi(value) : -1;
    else if (!std::strcmp(key, "tp_walk_repair")) o.tp_walk_repair = on;
    else if (!std::strcmp(key, "tp_unchecked")) o.tp_unchecked = on;
    else if (!std::strcmp(key, "tp_check")) o.tp_check = (value && value[0]) ? std::atoi(value) : 0;
    else if (!std::strcmp(key, "tp_scan_waves")) o.tp_scan_waves = (value && value[0]) ? std::atoi(value) : 0;
    else if (!std::strcmp(key, "tp_scan_lean")) o.tp_scan_lean = (value && value[0]) ? std::atoi(value) : 0;
    else if (!std::strcmp(key, "tp_scan_tol")) o.tp_scan_tol = (value && value[0]) ? std::atof(value) : 0.0;
    else if (!std::strcmp(key, "no_tile")) o.no_tile = on; else if (!std::strcmp(key, "no_wide")) o.no_wide = on;
    else if (!std::strcmp(key, "no_paired")) o.no_paired = on;
    else if (!std::strcmp(key, "no_mixed")) o.no_mixed = on;
    else if (!std::strcmp(key, "force_fallback")) o.force_fallback = on;
    else if (!std::strcmp(key, "no_block")) o.no_block = on;
    else if (!std::strcmp(key, "no_split")) o.no_split = on;
    else if (!std::strcmp(key, "win2")) o.win2 = on;
    else if (!std::strcmp(key, "no_win2")) o.no_win2 = on;
    else if (!std::strcmp(key, "win3")) o.win3 = on;
    else if (!std::strcmp(key, "no_win3")) o.no_win3 = on;
    else if (!std::strcmp(key, "btab_reference")) o.btab_reference = on;
    else if (!std::strcmp(key, "block_emode")) o.block_emode = (value && value[0]) ? std::atoi(value) : -1;
    else if (!std::strcmp(key, "dense_quad_threshold")) o.dense.quad_threshold = (value && value[0]) ? std::atoi(value) : -1;
    else if (!std::strcmp(key, "dense_pair_tiles")) o.dense.pair_tiles = (value && value[0]) ? std::atoi(value) : -1;
    else if (!std::strcmp(key, "dense_half_tile_limit")) o.dense.half_tile_limit = (value && value[0]) ? std::atoi(value) : -1;
    else if (!std::strcmp(key, "dense_batch_pair_threshold")) o.dense.batch_pair_threshold = (value && value[0]) ? std::atoi(value) : -1;
    else if (!std::strcmp(key, "dense_old_chain")) {
        const int v = (value && value[0]) ? std::atoi(value) : 0;
        if (v < 0 || v > 1) return PIORAN_ERR_ARG;
        o.dense.old_chain = v;
    }
    else if (!std::strcmp(key, "dense_no_pairs")) o.dense.no_pairs = on ? 1 : 0;
    else if (!std::strcmp(key, "dense_no_halves")) o.dense.no_halves = on ? 1 : 0;
    else if (!std::strcmp(key, "workspace_limit_mb")) o.workspace_limit_mb = (value && value[0]) ? std::atoll(value) : 0;
    else if (!std::strcmp(key, "dense_streams")) o.dense_streams = (value && value[0]) ? std::atoi(value) : 0;
    else if (!std::strcmp(key, "exp")) o.exp = (value && value[0]) ? std::atoi(value) : 0;
    else if (!std::strcmp(key, "ls_tile")) o.ls_tile = (value && value[0]) ? std::atoi(value) : 0;
    else if (!std::strcmp(key, "ls_only")) o.ls_only = (value && value[0]) ? std::atoi(value) : 0;
    else if (!std::strcmp(key, "rp_events")) o.rp_events = on ? 1 : 0;
    else if (!std::strcmp(key, "theta_events")) o.theta_events = on ? 1 : 0;
    else if (!std::strcmp(key, "pc_events")) o.pc_events = on ? 1 : 0;
    else if (!std::strcmp(key, "carma_events")) o.carma_events = on ? 1 : 0;
    else if (!std::strcmp(key, "wide2")) o.wide2 = on;
    else if (!std::strcmp(key, "no_wide2")) o.no_wide2 = on;
    else return PIORAN_ERR_ARG;
    return PIORAN_OK;
}

}  // namespace

int pioran_tile_choice(int32_t R, int64_t B, int64_t pass, int no_split) { return tile_choice(R, B, pass, no_split); }

int pioran_tile_pairs_slot(int64_t id, int64_t nchunk, int64_t ndb, int64_t* chunk, int64_t* draw_block)
{
    if (nchunk < 1 || ndb < 1 || id < 0 || nchunk > INT64_MAX / ndb || id >= nchunk * ndb || !chunk || !draw_block) return PIORAN_ERR_ARG;
    const PairsSlot s = tile_pairs_slot(id, nchunk, ndb);
    *chunk = s.chunk;
    *draw_block = s.db;
    return PIORAN_OK;
}

// "key=value;key=value" into a set of options
static int parse_options(const char* options, ScanOptions& opt)
{
    for (const char* kv = options ? options : ""; *kv;) {
        const char* end = std::strchr(kv, ';');
        const std::string item = end ? std::string(kv, end) : std::string(kv);
        kv = end ? end + 1 : kv + item.size();
        if (item.empty()) continue;
        const size_t eq = item.find('=');
        if (eq == std::string::npos) return PIORAN_ERR_ARG;
        if (const int rc = set_option(opt, item.substr(0, eq).c_str(), item.c_str() + eq + 1)) return rc;
    }
    return PIORAN_OK;
}

int pioran_value_route(int32_t R, int32_t J, int32_t n_one_row_terms, int64_t B, int64_t N, int per_draw_series, int64_t pass, const char* options,
                       char* name, int name_len, int32_t* tp)
{
    if (J < 1 || n_one_row_terms < 0 || n_one_row_terms > J || R != 2 * J - n_one_row_terms || B < 1 || N < 1 || !name || name_len < 1) return PIORAN_ERR_ARG;
    ScanOptions opt{};
    if (const int rc = parse_options(options, opt)) return rc;
    // every resource granted: a plain prepared state behind the table, the launch on its own step records
    const RouteQuery q{R, J, B, N, true, 0, per_draw_series != 0, J - n_one_row_terms, n_one_row_terms, true, true, opt};
    TpPlan plan;
    std::snprintf(name, (size_t)name_len, "%s", value_route(q, pass, &plan));
    if (tp) { tp[0] = plan.scan; tp[1] = plan.RP; tp[2] = plan.nseg; tp[3] = (int32_t)plan.L; }
    return PIORAN_OK;
}

int pioran_value_route_cd(int32_t n_two_row_terms, int32_t n_one_row_terms, int32_t n_per_draw_terms, int64_t B, int64_t N, int per_draw_series,
                          int must_run, const char* options, char* name, int name_len, int64_t* mixed_chunk)
{
    if (n_two_row_terms < 0 || n_one_row_terms < 0 || n_per_draw_terms < 1 || B < 1 || N < 1 || !name || name_len < 1) return PIORAN_ERR_ARG;
    if ((int64_t)n_two_row_terms + n_one_row_terms + n_per_draw_terms > 0xfffff || N > ((int64_t)1 << 48)) return PIORAN_ERR_ARG;
    ScanOptions opt{};
    if (const int rc = parse_options(options, opt)) return rc;
    int64_t chunk = 0;
    const char* fam = value_route_cd(opt, n_two_row_terms, n_one_row_terms, n_per_draw_terms, B, N, per_draw_series != 0, must_run != 0, &chunk);
    std::snprintf(name, (size_t)name_len, "%s", fam ? fam : "");
    if (mixed_chunk) *mixed_chunk = chunk;
    return fam ? PIORAN_OK : PIORAN_ERR_UNSUPPORTED;
}

int pioran_entry_route(const char* entry, int32_t R, int32_t J, int32_t n_one_row_terms, int64_t B, int per_draw, int shift, int want_c, int want_d,
                       int series_grads, const char* options, char* name, int name_len, int64_t* chunk_cap, int* shrink)
{
    if (!entry || J < 1 || n_one_row_terms < 0 || n_one_row_terms > J || R != 2 * J - n_one_row_terms || B < 1 || !name || name_len < 1) return PIORAN_ERR_ARG;
    ScanOptions opt{};
    if (const int rc = parse_options(options, opt)) return rc;
    const int flags = (shift ? kGradShift : 0) | (want_c ? kGradC : 0) | (want_d ? kGradD : 0) | (series_grads ? kGradSeries : 0);
    const EntryPlan plan = entry_route(entry, R, J, B, per_draw != 0, flags, opt);
    std::snprintf(name, (size_t)name_len, "%s", plan.name);
    if (chunk_cap) *chunk_cap = plan.chunk_cap;
    if (shrink) *shrink = plan.shrink;
    return plan.rc;
}

int pioran_step_route(const char* family, int32_t R, int32_t standard_rows, int32_t n_complex, int64_t B, int shared_table, int32_t npd_rows,
                      int per_draw_tables, const char* options, char* name, int name_len, int32_t* plan)
{
    if (!family || R < 1 || standard_rows < 0 || standard_rows > 2 || n_complex < 0 || B < 1 || npd_rows < 0 || !name || name_len < 1) return PIORAN_ERR_ARG;
    ScanOptions opt{};
    if (const int rc = parse_options(options, opt)) return rc;
    int32_t fields[8] = {};
    int rc = PIORAN_OK;
    if (!std::strcmp(family, "scan")) {
        const ScanPlan sp = scan_plan({R, standard_rows, n_complex, B, shared_table != 0, npd_rows, &opt});
        scan_plan_name(sp, name, (size_t)name_len);
        const int32_t f[8] = {sp.config, sp.form, sp.shared_tab, sp.mixed, sp.ycol, sp.npb, pioran_scan_kernel_exists(sp), sp.config < 0 ? 0 : kScanConfigs[sp.config].capacity()};
        std::memcpy(fields, f, sizeof(f));
        rc = sp.config < 0 ? PIORAN_ERR_UNSUPPORTED : PIORAN_OK;
    } else {
        static const char* const modes[4] = {"value", "store", "simulate", "gradient"};
        int m = 0;
        while (m < 4 && std::strcmp(family, modes[m])) ++m;
        if (m == 4) return PIORAN_ERR_ARG;
        const WidePlan wp = wide_plan((WideMode)m, R, npd_rows, per_draw_tables != 0, &opt);
        wide_plan_name(wp, (WideMode)m, name, (size_t)name_len);
        const int32_t f[8] = {wp.rpl, wp.lean, wp.ycol, wp.lean_adjoint};
        std::memcpy(fields, f, sizeof(f));
        rc = wp.rc;
    }
    if (plan) std::memcpy(plan, fields, sizeof(fields));
    return rc;
}

int pioran_window_route(const char* family, int32_t R, int32_t J, int64_t B, int32_t npd_rows, int per_draw_series, int want_cd, int32_t tp_rows,
                        int32_t tp_segments, int tp_mode, const char* options, char* name, int name_len, int32_t* plan)
{
    if (!family || !name || name_len < 1) return PIORAN_ERR_ARG;
    ScanOptions opt{};
    if (const int rc = parse_options(options, opt)) return rc;
    int32_t fields[12] = {};
    int rc = PIORAN_OK;
    static const char* const block_modes[4] = {"block", "block_grad", "block_solve", "block_sim"};
    int m = 0;
    while (m < 4 && std::strcmp(family, block_modes[m])) ++m;
    if (m < 4) {
        const BlockPlan bp = block_plan((BlockMode)m, R, J, B, npd_rows, want_cd != 0, &opt);
        block_plan_name(bp, (BlockMode)m, name, (size_t)name_len);
        const int32_t f[12] = {bp.NB, bp.emode, bp.pdm, bp.st, bp.threads, (int32_t)bp.lds, bp.cd, bp.tpt, pioran_block_kernel_exists(bp, (BlockMode)m)};
        std::memcpy(fields, f, sizeof(f));
        rc = bp.rc;
    } else if (!std::strcmp(family, "tile") || !std::strcmp(family, "tile_grad")) {
        const TileMode tm = family[4] ? TileMode::gradient : TileMode::value;
        const TilePlan tp = tile_plan(tm, R, J, per_draw_series != 0, want_cd != 0);
        tile_plan_name(tp, tm, name, (size_t)name_len);
        const bool ok = tp.rc == PIORAN_OK;
        const int32_t f[12] = {tp.NB, tp.KL, tp.SER, tp.cd, tp.adj_waves, ok ? 256 : 0, ok ? (int32_t)pioran_tile_lds_bytes(tp.NB) : 0,
                               ok && tm == TileMode::gradient ? (int32_t)pioran_tile_adj_lds_bytes(tp.NB, tp.cd) : 0, pioran_tile_kernel_exists(tp, tm)};
        std::memcpy(fields, f, sizeof(f));
        rc = tp.rc;
    } else if (!std::strcmp(family, "tp")) {
        const TpStepPlan sp = tp_step_plan(tp_rows, tp_segments, tp_mode, &opt);
        tp_step_plan_name(sp, name, (size_t)name_len);
        const bool walk = sp.boundary == TpPhase::small || sp.boundary == TpPhase::wave;
        const int32_t f[12] = {sp.NP, sp.NWV, (int32_t)sp.boundary, walk ? sp.rows : sp.rt, sp.lean, sp.tw, (int32_t)sp.lds, (int32_t)sp.verify,
                               sp.verify == TpPhase::wave ? sp.verify_rows : sp.verify_rt, (int32_t)sp.verify_lds, sp.filter_disc, pioran_tp_kernel_exists(sp)};
        std::memcpy(fields, f, sizeof(f));
        rc = sp.rc;
    } else {
        return PIORAN_ERR_ARG;
    }
    if (plan) std::memcpy(plan, fields, sizeof(fields));
    return rc;
}

extern "C" {

const char* pioran_strerror(int code)
{
    switch (code) {
        case PIORAN_OK: return "ok";
        case PIORAN_ERR_ARG: return "invalid argument";
        case PIORAN_ERR_HIP: return "HIP runtime error";
        case PIORAN_ERR_ALLOC: return "allocation failed";
        case PIORAN_ERR_UNSUPPORTED: return "unsupported size";
        default: return "unknown error";
    }
}

const char* pioran_last_hip_error(const pioran_ctx* ctx) { return ctx ? ctx->last_err.c_str() : ""; }

int pioran_abi_version(void) { return 7; }

// The FP64 FMA rate the device sustains now, at `waves_per_simd` (1 .. 8) wavefronts per SIMD on every SIMD: ~`ms` milliseconds of a pure
// v_fma_f64 stream, event-timed on the context's stream (table.hip).  Diagnostics: bench.py's frac_of_measured_fma_ceiling.
int pioran_ctx_fp64_probe(pioran_ctx* ctx, int waves_per_simd, double ms, double* tflops)
{
    if (!ctx || !tflops || waves_per_simd < 1 || waves_per_simd > 8 || !(ms > 0.0) || ms > 1000.0) return PIORAN_ERR_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int blocks = ctx->ncu * waves_per_simd;
    int rc = ensure(ctx, ctx->bscratch, (size_t)blocks * 256 * sizeof(double));
    if (rc) return rc;
    // 64 FMAs per trip at ~4.6 issue cycles each and `waves_per_simd` wavefronts sharing the SIMD, ~2 GHz
    int iters = (int)(ms * 1e-3 * 2.0e9 / (64.0 * 4.6 * waves_per_simd));
    if (iters < 64) iters = 64;
    double flop = 0.0;
    if ((rc = pioran_launch_fma_stream(blocks, 64, (double*)ctx->bscratch.p, nullptr, ctx->stream))) return rc;   // warm
    // (the context's internal event slots: 0 .. 11 are the caller's, pioran_ctx_event_record)
    HIPCHK(ctx, hipEventRecord(ctx->ev[14], ctx->stream));
    if ((rc = pioran_launch_fma_stream(blocks, iters, (double*)ctx->bscratch.p, &flop, ctx->stream))) return rc;
    HIPCHK(ctx, hipEventRecord(ctx->ev[15], ctx->stream));
    HIPCHK(ctx, hipEventSynchronize(ctx->ev[15]));
    float t = 0.f;
    HIPCHK(ctx, hipEventElapsedTime(&t, ctx->ev[14], ctx->ev[15]));
    *tflops = t > 0.f ? flop / (t * 1e-3) / 1e12 : 0.0;
    return PIORAN_OK;
}

int pioran_ctx_set_option(pioran_ctx* ctx, const char* key, const char* value)
{
    return ctx && key ? set_option(ctx->opt, key, value) : PIORAN_ERR_ARG;
}

static int ctx_create_impl(int device, void* stream, bool own, pioran_ctx** out)
{
    if (!out) return PIORAN_ERR_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return PIORAN_ERR_HIP;
    pioran_ctx* ctx = new (std::nothrow) pioran_ctx;
    if (!ctx) return PIORAN_ERR_ALLOC;
    ctx->device = device;
    // the only place the environment is read
    pioran_ctx_set_option(ctx, "scan_config", std::getenv("PIORAN_SCAN_CONFIG"));
    pioran_ctx_set_option(ctx, "no_wide", std::getenv("PIORAN_NO_WIDE"));
    pioran_ctx_set_option(ctx, "no_paired", std::getenv("PIORAN_NO_PAIRED"));
    pioran_ctx_set_option(ctx, "no_mixed", std::getenv("PIORAN_NO_MIXED"));
    pioran_ctx_set_option(ctx, "force_fallback", std::getenv("PIORAN_FORCE_FALLBACK"));
    pioran_ctx_set_option(ctx, "no_block", std::getenv("PIORAN_NO_BLOCK"));
    pioran_ctx_set_option(ctx, "no_tile", std::getenv("PIORAN_NO_TILE"));
    pioran_ctx_set_option(ctx, "no_tp", std::getenv("PIORAN_NO_TP"));
    pioran_ctx_set_option(ctx, "win2", std::getenv("PIORAN_WIN2"));
    pioran_ctx_set_option(ctx, "no_win2", std::getenv("PIORAN_NO_WIN2"));
    pioran_ctx_set_option(ctx, "wide2", std::getenv("PIORAN_WIDE2"));
    pioran_ctx_set_option(ctx, "no_wide2", std::getenv("PIORAN_NO_WIDE2"));
    if (hipSetDevice(device) != hipSuccess) { delete ctx; return PIORAN_ERR_HIP; }
    if (hipDeviceGetAttribute(&ctx->ncu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || ctx->ncu < 1) { delete ctx; return PIORAN_ERR_HIP; }
    if (own) {
        if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) { delete ctx; return PIORAN_ERR_HIP; }
        ctx->own_stream = true;
    } else {
        ctx->stream = (hipStream_t)stream;
    }
    for (auto& e : ctx->ev)
        if (hipEventCreate(&e) != hipSuccess) { delete ctx; return PIORAN_ERR_HIP; }
    *out = ctx;
    return PIORAN_OK;
}

int pioran_ctx_create(int device, pioran_ctx** out) { return ctx_create_impl(device, nullptr, true, out); }

int pioran_ctx_create_on_stream(int device, void* hip_stream, pioran_ctx** out)
{
    return ctx_create_impl(device, hip_stream, false, out);
}

int pioran_ctx_destroy(pioran_ctx* ctx)
{
    if (!ctx) return PIORAN_ERR_ARG;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    delete ctx;
    return PIORAN_OK;
}

// (a context whose creation failed half-way comes here too: what was never created is null)
pioran_ctx::~pioran_ctx()
{
    if (scalar_ds) pioran_dataset_destroy(scalar_ds);
    for (Buf* b : bufs) (void)b->release();   // before the streams go, as ever; the buffers' own destructors find nothing left
    for (auto& e : ev)
        if (e) (void)hipEventDestroy(e);
    for (auto& e : gev)
        if (e) (void)hipEventDestroy(e);
    for (auto& e : dev_)
        if (e) (void)hipEventDestroy(e);
    for (auto& st : dstream)
        if (st) (void)hipStreamDestroy(st);
    pin_release(this);
    if (aux) (void)hipStreamDestroy(aux);
    if (own_stream && stream) (void)hipStreamDestroy(stream);
}

int pioran_ctx_trim(pioran_ctx* ctx)
{
    if (!ctx) return PIORAN_ERR_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    SYNC(ctx);
    for (pioran_ctx::Buf* b : ctx->bufs) (void)b->release();
    pin_release(ctx);
    return PIORAN_OK;
}

int pioran_ctx_synchronize(pioran_ctx* ctx)
{
    if (!ctx) return PIORAN_ERR_ARG;
    SYNC(ctx);
    return PIORAN_OK;
}

int pioran_ctx_event_record(pioran_ctx* ctx, int slot)
{
    if (!ctx || slot < 0 || slot >= 12) return PIORAN_ERR_ARG;   // 12..15: internal
    HIPCHK(ctx, hipEventRecord(ctx->ev[slot], ctx->stream));
    return PIORAN_OK;
}

int pioran_ctx_event_elapsed_ms(pioran_ctx* ctx, int a, int b, float* ms)
{
    if (!ctx || !ms || a < 0 || a >= 12 || b < 0 || b >= 12) return PIORAN_ERR_ARG;
    HIPCHK(ctx, hipEventSynchronize(ctx->ev[b]));
    HIPCHK(ctx, hipEventElapsedTime(ms, ctx->ev[a], ctx->ev[b]));
    return PIORAN_OK;
}

int pioran_dataset_create(pioran_ctx* ctx, int64_t N, const double* t, const double* y, const double* sigma2,
                          pioran_ds** out)
{
    if (!ctx || !out || N < 1 || !t || !y || !sigma2) return PIORAN_ERR_ARG;
    *out = nullptr;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    pioran_ds* ds = new (std::nothrow) pioran_ds;
    if (!ds) return PIORAN_ERR_ALLOC;
    ds->ctx = ctx;
    ds->N = N;
    const size_t bytes = (size_t)N * sizeof(double);
    if (const int rc = ensure_exact(ctx, ds->series, 3 * bytes)) { delete ds; return rc; }
    double* base = (double*)ds->series.p;
    ds->t = base;
    ds->y = base + N;
    ds->s2 = base + 2 * N;
    hipError_t e = hipMemcpyAsync(ds->t, t, bytes, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(ds->y, y, bytes, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(ds->s2, sigma2, bytes, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        ctx->last_err = hipGetErrorString(e);
        delete ds;
        return PIORAN_ERR_HIP;
    }
    *out = ds;
    return PIORAN_OK;
}

int pioran_dataset_destroy(pioran_ds* ds)
{
    if (!ds) return PIORAN_ERR_ARG;
    (void)hipSetDevice(ds->ctx->device);
    (void)hipStreamSynchronize(ds->ctx->stream);
    delete ds;
    return PIORAN_OK;
}

static int prepare_state(pioran_ds* ds, PrepState& s, int64_t J, const double* c, const double* d, const int32_t* real_term)
{
    if (!ds || J < 1 || J > (1 << 20) || !c || !d) return PIORAN_ERR_ARG;
    pioran_ctx* ctx = ds->ctx;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    std::vector<int32_t> real(J, 0);
    std::vector<double> cc(c, c + J), dv(d, d + J);
    std::vector<int32_t> pdlist;
    for (int64_t j = 0; j < J; ++j) {
        real[j] = real_term ? (real_term[j] == 2 ? 2 : (real_term[j] ? 1 : 0)) : 0;
        if (real[j] == 1 && d[j] != 0.0) return PIORAN_ERR_ARG;  // a real term must have d = 0
        if (real[j] == 2) { cc[j] = 0.0; dv[j] = 0.0; pdlist.push_back((int32_t)j); }   // (c, d) come per draw
    }
    if (pdlist.size() > 255 || J > 0xfffff) return PIORAN_ERR_UNSUPPORTED;
    c = cc.data();
    d = dv.data();
    const bool same = s.prepared && s.J == J && !std::memcmp(s.c_host.data(), c, J * sizeof(double)) &&
                      !std::memcmp(s.d_host.data(), d, J * sizeof(double)) && s.real_host == real;
    if (same) return PIORAN_OK;
    s.prepared = false;
    s.btab_ready = false;
    int rc = ensure_exact(ctx, s.dc, 2 * (size_t)J * sizeof(double));
    if (rc) return rc;
    s.dd = s.dc + J;
    s.c_host.assign(c, c + J);
    s.d_host.assign(d, d + J);
    HIPCHK(ctx, hipMemcpyAsync(s.dc, s.c_host.data(), J * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(s.dd, s.d_host.data(), J * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    rc = set_rowmap(ds, s, build_rowmap(J, real.data()));   // sets s.R
    if (rc) return rc;
    s.npd_terms = (int32_t)pdlist.size();
    if (!pdlist.empty()) {
        if ((rc = ensure_exact(ctx, s.dpd_terms, 256 * sizeof(int32_t)))) return rc;
        HIPCHK(ctx, hipMemcpyAsync(s.dpd_terms, pdlist.data(), pdlist.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
        SYNC(ctx);
    }
    // the table is per ROW (v, x, phi) + (y_n, sigma2_n) per step, see table.hip
    if ((rc = ensure_exact(ctx, s.tab, pioran_table_doubles(ds->N, s.R) * sizeof(double)))) return rc;
    rc = pioran_launch_table(ds->N, s.R, s.rowmap, ds->t, s.dc, s.dd, ds->y, ds->s2, s.tab,
                             rec_stride_of(s.R), ctx->stream);
    if (rc) return rc;
    s.J = (int32_t)J;
    s.real_host = real;
    {   // 1: every term has both rows; 2: two-row terms first, then one-row terms only; 0: anything else
        int64_t nc = 0;
        while (nc < J && real[nc] == 0) ++nc;
        bool rest_real = true;
        for (int64_t j = nc; j < J; ++j) rest_real = rest_real && real[j] == 1;
        s.row_layout = nc == J ? 1 : ((rest_real && pdlist.empty()) ? 2 : 0);
        s.n_complex = (int32_t)nc;
    }
    s.prepared = true;
    return PIORAN_OK;
}

int pioran_dataset_prepare(pioran_ds* ds, int64_t J, const double* c, const double* d, const int32_t* real_term)
{
    if (!ds) return PIORAN_ERR_ARG;
    return prepare_state(ds, ds->user, J, c, d, real_term);
}

static int batch_dev_impl(pioran_ds* ds, const PrepState& s, int64_t B, const double* dA, const double* dBc, const double* dmu,
                          const double* dnu, const double* dY, const double* dS2, double* dout, int32_t* dstatus)
{
    if (!ds || B < 1 || !dA || !dBc || !dout) return PIORAN_ERR_ARG;
    if (!s.prepared || s.npd_terms > 0) return PIORAN_ERR_ARG;   // per-draw terms need the mixed-mode host entry
    if ((dY == nullptr) != (dS2 == nullptr)) return PIORAN_ERR_ARG;
    pioran_ctx* ctx = ds->ctx;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    ScanParams p = shared_params(ds, s, B, {dA, dBc, nullptr, nullptr, dmu, dnu, dY, dS2});
    p.out = dout; p.status = dstatus;
    return launch(ds, p);
}

int pioran_celerite_logl_batch_dev(pioran_ds* ds, int64_t B, const double* dA, const double* dBc, const double* dmu,
                                   const double* dnu, const double* dY, const double* dS2, double* dout,
                                   int32_t* dstatus)
{
    if (!ds) return PIORAN_ERR_ARG;
    return batch_dev_impl(ds, ds->user, B, dA, dBc, dmu, dnu, dY, dS2, dout, dstatus);
}

int pioran_celerite_logl_batch_dev_cd(pioran_ds* ds, int64_t B, int64_t J, const double* dA, const double* dBc,
                                      const double* dC, const double* dDd, const double* dmu, const double* dnu,
                                      const double* dY, const double* dS2, double* dout, int32_t* dstatus)
{
    if (!ds || B < 1 || J < 1 || !dA || !dBc || !dC || !dDd || !dout) return PIORAN_ERR_ARG;
    if ((dY == nullptr) != (dS2 == nullptr)) return PIORAN_ERR_ARG;
    pioran_ctx* ctx = ds->ctx;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // per-draw (c, d): full 2J rows, no table; the prepared shared state is left untouched
    std::vector<int32_t> rm = build_rowmap(J, nullptr);
    int32_t* drm = nullptr;
    int rc = ensure(ctx, ctx->bwork, rm.size() * sizeof(int32_t));
    if (rc) return rc;
    drm = (int32_t*)ctx->bwork.p;
    HIPCHK(ctx, hipMemcpyAsync(drm, rm.data(), rm.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    SYNC(ctx);
    const int32_t R = (int32_t)rm.size();
    const DrawChunk in{dA, dBc, dC, dDd, dmu, dnu, dY, dS2};
    // draws [b0, b0 + nb) of the caller's device arrays, on per-draw tables tab_stride doubles apart (0: no tables)
    auto draws = [&](int64_t b0, int64_t nb, int64_t tab_stride) {
        ScanParams q = perdraw_params(ds, (int32_t)J, R, drm, nb, in.from_draw(b0, J, ds->N), tab_stride, 0);
        q.out = dout + b0; q.status = at(dstatus, b0);
        return q;
    };
    const PerDrawForm form = perdraw_form(ctx->opt, B, R, (int32_t)J);
    if (form == PerDrawForm::no_table) {
        ScanParams p = draws(0, B, 0);
        p.rec_stride = 0;   // no table at all: the kernels evaluate the per-draw transcendentals themselves
        return launch(ds, p);
    }
    // every draw its own table — the step records the latency kernel walks, or the windowed kernel's: a chunk of at most 256 tables in bscratch
    const bool wide = form == PerDrawForm::wide_tables;
    const int64_t tdoubles = wide ? (int64_t)pioran_table_doubles(ds->N, R) : (int64_t)pioran_block_table_doubles(ds->N, R, (int32_t)J);
    int64_t chunk = B < 256 ? B : 256;
    auto bytes = [&](int64_t nb) { return (size_t)nb * (size_t)tdoubles * sizeof(double); };
    if ((rc = size_chunk(ctx, chunk, {&ctx->bscratch}, bytes, [&](int64_t nb) { return ensure(ctx, ctx->bscratch, bytes(nb)); }))) return rc;
    double* const tabs = (double*)ctx->bscratch.p;
    for (int64_t b0 = 0; b0 < B; b0 += chunk) {
        const int64_t nb = std::min(B - b0, chunk);
        ScanParams q = draws(b0, nb, tdoubles);
        if (wide) q.tab = tabs;
        rc = wide ? pioran_launch_table_batch(ds->N, R, (int32_t)J, nb, drm, ds->t, q.C, q.D, ds->y, ds->s2, tabs, q.rec_stride, tdoubles, ctx->stream)
                  : pioran_launch_block_table_batch(ds->N, R, (int32_t)J, nb, drm, ds->t, q.C, q.D, ds->y, ds->s2, tabs, tdoubles, ctx->stream);
        if (rc) return rc;
        g_last_kernel = wide ? "wide (per-draw tables)" : "block (per-draw tables)";
        rc = wide ? pioran_launch_scan_wide(q, ctx->stream) : pioran_launch_scan_block(q, tabs, ctx->stream);
        if (rc == PIORAN_ERR_HIP) ctx->last_err = wide ? "per-draw-table latency kernel launch failed" : "windowed kernel (per-draw tables) launch failed";
        if (rc) return rc;
    }
    return PIORAN_OK;
}

// kind[j] of a batch's terms (build_rowmap): 2 where (c, d) differ between the draws (per_draw: C, Dd are [B][J]; else [J], and C is not read:
// rand_posterior_refuse passes none); 1 where the sin row is
// identically zero for the whole batch (d_j = 0 and b_j = 0 in every draw): the term keeps only its cos row; 0 otherwise
static std::vector<int32_t> classify_terms(int64_t B, int64_t J, const double* Bc, const double* C, const double* Dd, bool per_draw)
{
    std::vector<int32_t> kind(J, 0);
    for (int64_t j = 0; j < J; ++j) {
        bool shared = true;
        for (int64_t b = 1; per_draw && b < B && shared; ++b) shared = C[b * J + j] == C[j] && Dd[b * J + j] == Dd[j];
        if (!shared) { kind[j] = 2; continue; }
        if (Dd[j] != 0.0) continue;
        bool allzero = true;
        for (int64_t b = 0; b < B && allzero; ++b) allzero = Bc[b * J + j] == 0.0;
        kind[j] = allzero;
    }
    return kind;
}

// Shared (c, d): builds (or reuses) the shared table, one-row terms with their cos row only.
static int prepare_shared(pioran_ds* ds, int64_t B, int64_t J, const double* Bc, const double* C, const double* Dd)
{
    return prepare_state(ds, ds->host, J, C, Dd, classify_terms(B, J, Bc, C, Dd, false).data());
}

// The host state of an entry that serves both forms.  per_draw — (C, Dd) [B][J], every term's of its own in every draw: the row map with both rows of
// every term is what the entry uses (the shared table this builds from draw 0 is not)
static int prepare_draws(pioran_ds* ds, bool per_draw, int64_t B, int64_t J, const double* Bc, const double* C, const double* Dd)
{
    return per_draw ? prepare_state(ds, ds->host, J, C, Dd, nullptr) : prepare_shared(ds, B, J, Bc, C, Dd);
}

// Where mixed_core's draws are: `draws` holds the whole batch on the device, or the caller's host arrays, which go up a chunk at a time — their
// per-draw series too, unless the context's bY / bS2 have the whole batch's already (series_on_device: shift transform)
struct MixedSource { DrawChunk draws; bool on_device, series_on_device; };

// draws [b0, b0 + nb) of `src` on the device
static int mixed_chunk(pioran_ds* ds, int64_t J, const MixedSource& src, int64_t b0, int64_t nb, DrawChunk& m)
{
    pioran_ctx* ctx = ds->ctx;
    const DrawChunk& h = src.draws;
    if (src.on_device) { m = h.from_draw(b0, J, ds->N); return PIORAN_OK; }
    int rc;
    if ((rc = upload_draws(ctx, J, b0, nb, h.A, h.Bc, h.C, h.D, h.mu, h.nu, m))) return rc;
    if (h.Y) {
        const size_t bn = (size_t)nb * (size_t)ds->N * sizeof(double);
        if ((rc = upload(ctx, ctx->bY, h.Y + b0 * ds->N, bn))) return rc;
        if ((rc = upload(ctx, ctx->bS2, h.S2 + b0 * ds->N, bn))) return rc;
        m.Y = (const double*)ctx->bY.p; m.S2 = (const double*)ctx->bS2.p;
    } else if (src.series_on_device) {
        m.Y = (const double*)ctx->bY.p + b0 * ds->N; m.S2 = (const double*)ctx->bS2.p + b0 * ds->N;
    }
    return PIORAN_OK;
}

// Mixed mode (route.hip mixed_plan): kind[J] (0 shared two-row, 1 shared real, 2 per-draw) and the shared values (C0, D0: [J], entries of per-draw
// terms ignored) declare the layout; the shared terms keep the shared table, the per-draw terms get per-draw rows, built by a pre-pass kernel for
// chunks of draws.  Results go to the caller's host arrays.  Returns 1 if it handled the batch, 0 if the caller should take the generic per-draw
// path (must_run: if no kernel can take the rows), < 0 on error.
static int mixed_core(pioran_ds* ds, int64_t B, int64_t J, const std::vector<int32_t>& kind, const double* C0, const double* D0, const MixedSource& src,
                      double* out, int32_t* status, bool must_run = false)
{
    pioran_ctx* ctx = ds->ctx;
    PrepState& s = ds->host;
    int32_t npd = 0, rows = 0;
    for (int64_t j = 0; j < J; ++j) { npd += kind[j] == 2; rows += kind[j] == 1 ? 1 : 2; }
    const MixedPlan plan = mixed_plan(ctx->opt, B, ds->N, (int32_t)J, rows, npd, must_run);
    if (!plan.take) return 0;
    int rc;
    if ((rc = prepare_state(ds, s, J, C0, D0, kind.data()))) return rc;
    // The windowed kernel with per-draw rows needs its own table of the shared rows and the per-draw (cos, sin)(d t_n); where that table cannot be
    // had, the scan takes the batch on a combined table — the shared records widened by a chunk's per-draw rows, chunk * 2 npd * 3 doubles
    bool windowed = plan.windowed;
    if (windowed && (rc = ensure_btab(ds, s))) {
        if (rc != PIORAN_ERR_UNSUPPORTED) return rc;
        windowed = false;
    }
    const int64_t chunk = windowed ? std::min<int64_t>(B, 4096) : plan.chunk;
    const int64_t rs_shared = rec_stride_of(rows), rec_stride = rs_shared + chunk * 6 * npd;
    const size_t wdoubles = windowed ? pioran_block_pd_trig_doubles(ds->N, chunk, s.npd_terms) : (size_t)(ds->N + 1) * (size_t)rec_stride;
    if ((rc = ensure(ctx, ctx->bscratch, wdoubles * sizeof(double)))) return rc;
    double* const work = (double*)ctx->bscratch.p;
    // shared rows into the combined layout (same kernel as the plain table, wider record stride)
    if (!windowed && (rc = pioran_launch_table(ds->N, s.R, s.rowmap, ds->t, s.dc, s.dd, ds->y, ds->s2, work, rec_stride, ctx->stream))) return rc;
    if ((rc = ensure_results(ctx, chunk))) return rc;
    for (int64_t b0 = 0; b0 < B; b0 += chunk) {
        const int64_t nb = std::min(B - b0, chunk);
        DrawChunk m{};
        if ((rc = mixed_chunk(ds, J, src, b0, nb, m))) return rc;
        rc = windowed ? pioran_launch_block_pd_trig(ds->N, nb, (int32_t)J, s.npd_terms, s.dpd_terms, ds->t, m.D, work, ctx->stream)
                      : pioran_launch_pd_table(ds->N, nb, (int32_t)J, s.npd_terms, s.dpd_terms, ds->t, m.C, m.D, work, rec_stride, rs_shared, ctx->stream);
        if (rc) return rc;
        ScanParams p = shared_params(ds, s, nb, m);
        p.out = (double*)ctx->bout.p; p.status = (int32_t*)ctx->bst.p;
        p.npd_rows = 2 * s.npd_terms;
        if (windowed) {
            p.pd_C = m.C; p.pd_trig = work; p.pd_npad = (ds->N + 15) / 16 * 16;
            g_last_kernel = "block+pd";
            rc = pioran_launch_scan_block(p, s.btab, ctx->stream);
        } else {
            p.tab = work; p.rec_stride = rec_stride;
            rc = scan_dispatch(p, ctx->stream);
        }
        if (rc) { ctx->last_err = windowed ? "windowed kernel (per-draw rows) launch failed" : "mixed-mode scan launch failed"; return rc; }
        if ((rc = download_results(ctx, out, status, b0, nb))) return rc;
        SYNC(ctx);
    }
    return 1;
}

// kind[J] of a batch whose host arrays hold a (c, d) row per draw.  One draw, or the same rows in every draw: that IS the shared case (table built once,
// windowed kernel for small batches), no term is per-draw.  Else the terms that differ are; under "no_mixed" all of them, unlooked at (mixed_plan
// declines the batch whatever they are: this saves classify_terms' pass over it).
static std::vector<int32_t> draw_layout(const ScanOptions& opt, int64_t B, int64_t J, const double* Bc, const double* C, const double* Dd)
{
    bool same = true;
    for (int64_t b = 1; b < B && same; ++b)
        same = !std::memcmp(C + b * J, C, (size_t)J * sizeof(double)) && !std::memcmp(Dd + b * J, Dd, (size_t)J * sizeof(double));
    if (!same && opt.no_mixed) return std::vector<int32_t>((size_t)J, 2);
    return classify_terms(B, J, Bc, C, Dd, !same);
}

// The transformed series of the shifted log-flux models, all B draws' (dshift: their shifts, on the device), in bY / bS2: where the value bodies read a
// batch's per-draw series
static int stage_shift_dev(pioran_ds* ds, int64_t B, const double* dshift)
{
    pioran_ctx* ctx = ds->ctx;
    const size_t bn = (size_t)B * (size_t)ds->N * sizeof(double);
    int rc;
    if ((rc = ensure_each(ctx, {{&ctx->bY, bn}, {&ctx->bS2, bn}}))) return rc;
    return pioran_launch_shift_transform(ds->N, B, ds->y, ds->s2, dshift, (double*)ctx->bY.p, (double*)ctx->bS2.p, ctx->stream);
}

// ... from the caller's shifts
static int stage_shift(pioran_ds* ds, int64_t B, const double* shift)
{
    const int rc = upload(ds->ctx, ds->ctx->bshift, shift, B * sizeof(double));
    return rc ? rc : stage_shift_dev(ds, B, (const double*)ds->ctx->bshift.p);
}

// The value of a batch from the host's view of its terms: kind[J] as mixed_core reads it, (C0, D0) [J] the values of the terms that are not per-draw.
// No per-draw term: the shared table.  Else mixed mode where its plan takes the batch, else every term from the draws' own (c, d) — which a caller
// whose shared terms have no per-draw copy does not have (must_run: PIORAN_ERR_UNSUPPORTED then).  Results go to the caller's host arrays; the last
// copies are queued, not waited for.
static int value_from_draws(pioran_ds* ds, int64_t B, int64_t J, const MixedSource& src, const std::vector<int32_t>& kind, const double* C0, const double* D0,
                            bool must_run, double* out, int32_t* status)
{
    pioran_ctx* ctx = ds->ctx;
    const bool shared = std::find(kind.begin(), kind.end(), 2) == kind.end();
    int rc;
    if (shared) {
        if ((rc = prepare_state(ds, ds->host, J, C0, D0, kind.data()))) return rc;
    } else {
        if ((rc = mixed_core(ds, B, J, kind, C0, D0, src, out, status, must_run))) return rc < 0 ? rc : PIORAN_OK;
        if (must_run) return PIORAN_ERR_UNSUPPORTED;   // too many rows for the register-resident kernels
    }
    MixedSource whole = src;
    if (shared) whole.draws.C = whole.draws.D = nullptr;   // (host arrays: the table has them, they do not go up)
    DrawChunk m{};
    if ((rc = mixed_chunk(ds, J, whole, 0, B, m))) return rc;
    if ((rc = ensure_results(ctx, B))) return rc;
    double* const dout = (double*)ctx->bout.p; int32_t* const dst = (int32_t*)ctx->bst.p;
    rc = shared ? batch_dev_impl(ds, ds->host, B, m.A, m.Bc, m.mu, m.nu, m.Y, m.S2, dout, dst)
                : pioran_celerite_logl_batch_dev_cd(ds, B, J, m.A, m.Bc, m.C, m.D, m.mu, m.nu, m.Y, m.S2, dout, dst);
    return rc ? rc : download_results(ctx, out, status, 0, B);
}

// host-pointer batch; series_on_device: ctx->bY / ctx->bS2 already hold the per-draw series (shift transform)
static int batch_host_impl(pioran_ds* ds, int64_t B, int64_t J, const double* A, const double* Bc, const double* C,
                           const double* Dd, int cd_shared, const double* mu, const double* nu, const double* Y,
                           const double* S2, bool series_on_device, double* out, int32_t* status)
{
    if (!ds || B < 1 || J < 1 || !A || !Bc || !C || !Dd || !out) return PIORAN_ERR_ARG;
    if ((Y == nullptr) != (S2 == nullptr)) return PIORAN_ERR_ARG;
    pioran_ctx* ctx = ds->ctx;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    PendingGuard pending_guard(ctx);
    const size_t bj = (size_t)B * (size_t)J * sizeof(double);
    const size_t bn = (size_t)B * (size_t)ds->N * sizeof(double);
    int rc;
    const std::vector<int32_t> kind = cd_shared ? classify_terms(B, J, Bc, C, Dd, false) : draw_layout(ctx->opt, B, J, Bc, C, Dd);
    cd_shared = std::find(kind.begin(), kind.end(), 2) == kind.end();
    // Small calls with shared (c, d) — the scalar drop-in, a few walkers (late round 4): the kernels read the coefficients straight from
    // pinned host memory (each value once) and write log L / status straight into it, so the call issues no copy command for them; a
    // per-draw series, which the kernels stream step by step, still goes to HBM, (y | sigma2) in ONE copy.  Scalar call, N = 32: 44 -> 3x us.
    const size_t zc_in = 2 * bj + (mu ? B * sizeof(double) : 0) + (nu ? B * sizeof(double) : 0);
    const size_t zc_all = zc_in + B * sizeof(double) + ((B * sizeof(int32_t) + 7) & ~size_t(7));
    const size_t zc_pad = (zc_all + 255) & ~size_t(255);
    const bool y_staged = Y && zc_pad + 2 * bn <= kPinMaxRequest;      // (ONE reservation: a second one could drain or move the staging area)
    const bool zc_wanted = cd_shared && zc_all <= (size_t(16) << 10) && !(ctx->opt.exp & 64);
    if (zc_wanted && (rc = prepare_state(ds, ds->host, J, C, Dd, kind.data()))) return rc;
    char* zc = zc_wanted ? (char*)pin_reserve(ctx, zc_pad + (y_staged ? 2 * bn : 0)) : nullptr;
    if (zc) {
        const double *dA = (const double*)zc, *dB = dA + B * J, *dmu = nullptr, *dnu = nullptr;
        char* q = zc + 2 * bj;
        std::memcpy(zc, A, bj); std::memcpy(zc + bj, Bc, bj);
        if (mu) { std::memcpy(q, mu, B * sizeof(double)); dmu = (const double*)q; q += B * sizeof(double); }
        if (nu) { std::memcpy(q, nu, B * sizeof(double)); dnu = (const double*)q; q += B * sizeof(double); }
        double* dout = (double*)q; q += B * sizeof(double);
        int32_t* dst = (int32_t*)q;
        const double *dY = nullptr, *dS2 = nullptr;
        if (Y) {
            if ((rc = ensure(ctx, ctx->bY, 2 * bn))) return rc;
            if (y_staged) {
                char* sy = zc + zc_pad;
                std::memcpy(sy, Y, bn); std::memcpy(sy + bn, S2, bn);
                HIPCHK(ctx, hipMemcpyAsync(ctx->bY.p, sy, 2 * bn, hipMemcpyHostToDevice, ctx->stream));
            } else {
                HIPCHK(ctx, hipMemcpyAsync(ctx->bY.p, Y, bn, hipMemcpyHostToDevice, ctx->stream));
                HIPCHK(ctx, hipMemcpyAsync((char*)ctx->bY.p + bn, S2, bn, hipMemcpyHostToDevice, ctx->stream));
            }
            dY = (const double*)ctx->bY.p; dS2 = dY + (size_t)B * (size_t)ds->N;
        } else if (series_on_device) {
            dY = (const double*)ctx->bY.p; dS2 = (const double*)ctx->bS2.p;
        }
        if ((rc = batch_dev_impl(ds, ds->host, B, dA, dB, dmu, dnu, dY, dS2, dout, dst))) return rc;
        ctx->pending.push_back({out, dout, B * sizeof(double)});
        if (status) ctx->pending.push_back({status, dst, B * sizeof(int32_t)});
        SYNC(ctx);
        return PIORAN_OK;
    }
    const MixedSource src{{A, Bc, C, Dd, mu, nu, Y, S2}, false, series_on_device};
    if ((rc = value_from_draws(ds, B, J, src, kind, C, Dd, false, out, status))) return rc;   // row 0 of C, Dd: the shared values
    SYNC(ctx);
    return PIORAN_OK;
}

int pioran_celerite_logl_batch(pioran_ds* ds, int64_t B, int64_t J, const double* A, const double* Bc,
                               const double* C, const double* Dd, int cd_shared, const double* mu, const double* nu,
                               const double* Y, const double* S2, double* out, int32_t* status)
{
    return batch_host_impl(ds, B, J, A, Bc, C, Dd, cd_shared, mu, nu, Y, S2, false, out, status);
}

int pioran_celerite_logl_batch_shift_dev(pioran_ds* ds, int64_t B, const double* dA, const double* dBc, const double* dmu,
                                         const double* dnu, const double* dshift, double* dout, int32_t* dstatus)
{
    if (!ds || B < 1 || !dA || !dBc || !dshift || !dout) return PIORAN_ERR_ARG;
    if (!ds->user.prepared) return PIORAN_ERR_ARG;
    pioran_ctx* ctx = ds->ctx;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (const int rc = stage_shift_dev(ds, B, dshift)) return rc;
    return batch_dev_impl(ds, ds->user, B, dA, dBc, dmu, dnu, (const double*)ctx->bY.p, (const double*)ctx->bS2.p, dout, dstatus);
}

int pioran_celerite_logl_batch_shift(pioran_ds* ds, int64_t B, int64_t J, const double* A, const double* Bc,
                                     const double* C, const double* Dd, int cd_shared, const double* mu, const double* nu,
                                     const double* shift, double* out, int32_t* status)
{
    if (!ds || B < 1 || J < 1 || !A || !Bc || !C || !Dd || !shift || !out) return PIORAN_ERR_ARG;
    pioran_ctx* ctx = ds->ctx;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (const int rc = stage_shift(ds, B, shift)) return rc;
    return batch_host_impl(ds, B, J, A, Bc, C, Dd, cd_shared, mu, nu, nullptr, nullptr, /*series_on_device=*/true, out,
                           status);
}

int pioran_logpdf_batch_theta(pioran_ds* ds, int64_t B, int model, int64_t n_components, int basis, int is_integrated_power,
                              double f_min, double f_max, double S_low, double S_high, const double* theta,
                              const double* norm, const double* mu, const double* nu, const double* shift, int64_t n_qpo,
                              const double* qpo, double* out, int32_t* status, double* A_out, double* Bc_out)
{
    if (!ds || B < 1 || !theta || !norm || !out || model < 0 || model > 1 || basis < 0 || basis > 1) return PIORAN_ERR_ARG;
    if (n_qpo < 0 || n_qpo > 8 || (n_qpo > 0 && !qpo)) return PIORAN_ERR_ARG;
    pioran_ctx* ctx = ds->ctx;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    PendingGuard pending_guard(ctx);
    ThetaDraws td;
    int rc = stage_theta(ctx, B, model, n_components, basis, is_integrated_power, f_min, f_max, S_low, S_high, theta, norm, td, n_qpo, qpo);
    if (rc) return rc;
    const int64_t Jc = td.terms(), Jt = Jc + n_qpo;
    MixedSource src{{}, true, false};
    if ((rc = stage_draws(ctx, Jt, 0, B, {nullptr, nullptr, nullptr, nullptr, mu, nu, nullptr, nullptr}, false, &td, src.draws))) return rc;
    if (shift) {
        if ((rc = stage_shift(ds, B, shift))) return rc;
        src.draws.Y = (const double*)ctx->bY.p; src.draws.S2 = (const double*)ctx->bS2.p;
    }
    // the continuum's terms are the grid's, shared by all draws; the features' (c, d) exist per draw only, and the continuum's per draw not at all
    std::vector<int32_t> kind(td.real);
    kind.resize((size_t)Jt, 2);
    td.c.resize((size_t)Jt, 0.0); td.d.resize((size_t)Jt, 0.0);
    if ((rc = value_from_draws(ds, B, Jt, src, kind, td.c.data(), td.d.data(), /*must_run=*/n_qpo > 0, out, status))) return rc;
    const size_t bj = (size_t)B * (size_t)Jt * sizeof(double);
    if (A_out && (rc = download(ctx, A_out, ctx->bA.p, bj))) return rc;
    if (Bc_out && (rc = download(ctx, Bc_out, ctx->bB.p, bj))) return rc;
    SYNC(ctx);
    return PIORAN_OK;
}

int pioran_celerite_logl(pioran_ctx* ctx, int64_t N, int64_t J, const double* a, const double* b, const double* c,
                         const double* d, const double* t, const double* y, const double* sigma2, double* out,
                         int32_t* status)
{
    if (!ctx || N < 1 || J < 1 || !a || !b || !c || !d || !t || !y || !sigma2 || !out) return PIORAN_ERR_ARG;
    // A sampler calls logl thousands of times with the same t (and usually the same c, d) and a fresh y - mu,
    // sigma2 * nu: keep the series handle (and through it the cos/sin/exp table) while t is unchanged, and pass
    // y, sigma2 as this call's per-draw series.
    int rc;
    const bool same_t = ctx->scalar_ds && (int64_t)ctx->scalar_t.size() == N &&
                        !std::memcmp(ctx->scalar_t.data(), t, (size_t)N * sizeof(double));
    if (!same_t) {
        if (ctx->scalar_ds) pioran_dataset_destroy(ctx->scalar_ds);
        ctx->scalar_ds = nullptr;
        ctx->scalar_t.clear();
        if ((rc = pioran_dataset_create(ctx, N, t, y, sigma2, &ctx->scalar_ds))) return rc;
        ctx->scalar_t.assign(t, t + N);
    }
    return pioran_celerite_logl_batch(ctx->scalar_ds, 1, J, a, b, c, d, 1, nullptr, nullptr, y, sigma2, out, status);
}

// ---- posterior mean / simulation --------------------------------------------------------------------
// The three batched entries below (posterior mean, value and gradient, simulation) each serve both forms of (c, d) in ONE body:
//   shared by the draws — the prepared state's tables; the windowed kernels where the rows fit them, else step by step;
//   per_draw — (c, d) of their own in every term (posterior draws of QPO / CARMA / free Celerite models), several draws: every draw its own
//   windowed-kernel tables, built per chunk, all draws of a chunk in one launch of every kernel.  There is no step-by-step leg: a shape the windowed
//   kernels do not take is PIORAN_ERR_UNSUPPORTED before any upload or allocation, and the public entry goes draw by draw (each_draw).
// The forms differ in the state they prepare (prepare_draws), in who builds the tables and when (build_tables), in the launch description (chunk_params).
// Kernels, refusals, the chunk's cap and what a call short of memory does: the EntryPlan (route.hip entry_plan).  The argument checks: the public entries'.

// Posterior mean of B draws at M times
static int predict_batch(pioran_ds* ds, bool per_draw, int64_t B, int64_t J, const DrawChunk& in, int64_t M, const double* tau, double* mean_out,
                         int32_t* status)
{
    pioran_ctx* ctx = ds->ctx;
    PrepState& s = ds->host;
    if (per_draw && entry_plan(Entry::predict, (int32_t)(2 * J), (int32_t)J, 0, B, true, 0, ctx->opt).rc) return PIORAN_ERR_UNSUPPORTED;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    PendingGuard pending_guard(ctx);
    int rc;
    if ((rc = prepare_draws(ds, per_draw, B, J, in.Bc, in.C, in.D))) return rc;
    EntryPlan plan;
    if ((rc = plan_entry(ds, s, Entry::predict, B, per_draw, 0, plan))) return rc;
    const int64_t N = ds->N;
    // buffer roles: the per-window stores (step by step: the factor) | a chunk's forward tables (per_draw only) | the reverse table(s) | -z and the Q
    // recurrences | the tau-only factors | a chunk's means | tau
    pioran_ctx::Buf &stores = ctx->bwork, &btabs = ctx->bscratch, &gtabs = ctx->bgtab, &qws = ctx->bq, &tauws = ctx->bK, &mean = ctx->bY, &taus = ctx->bshift;
    int64_t chunk = std::min(B, plan.chunk_cap);
    if (plan.windowed) {
        const size_t bt = per_draw ? pioran_block_table_doubles(N, s.R, s.J) : 0, gt = pioran_block_gtab_doubles(N, s.R);
        auto ntab = [&](int64_t nb) { return per_draw ? nb : 1; };      // pairs of tables of nb draws
        auto need = [&](int64_t nb) {
            size_t d = pioran_block_store_workspace_doubles(nb, N, s.R, 2) + pioran_predict_q_workspace_doubles(nb, N, s.R);
            if (per_draw) d += (size_t)nb * (bt + gt) + pioran_predict_tau_workspace_doubles(M, s.R, nb) + (size_t)nb * (size_t)M;
            return d * sizeof(double);
        };
        auto grow = [&](int64_t nb) {
            return ensure_each(ctx, {{&stores, pioran_block_store_workspace_doubles(nb, N, s.R, 2) * sizeof(double)},
                                     {&btabs, (size_t)nb * bt * sizeof(double)},
                                     {&gtabs, (size_t)ntab(nb) * gt * sizeof(double)},
                                     {&qws, pioran_predict_q_workspace_doubles(nb, N, s.R) * sizeof(double)},
                                     {&tauws, pioran_predict_tau_workspace_doubles(M, s.R, ntab(nb)) * sizeof(double)},
                                     {&mean, per_draw ? (size_t)nb * (size_t)M * sizeof(double) : 0}});
        };
        rc = size_chunk(ctx, chunk, per_draw ? BufList{&stores, &btabs, &gtabs, &tauws, &qws} : BufList{&stores, &qws}, need, grow, plan.shrink);
        // (no memory for the chunk the budget admits: not a smaller chunk, the step-by-step kernels)
        if (rc == PIORAN_ERR_ALLOC && !plan.shrink) { plan.leave_windowed(); chunk = std::min(B, plan.chunk_cap); rc = PIORAN_OK; }
        if (rc) return rc;
    }
    if (!plan.windowed && (rc = ensure(ctx, stores, pioran_predict_workspace_doubles(chunk, N, s.R) * sizeof(double)))) return rc;
    if ((rc = upload(ctx, taus, tau, (size_t)M * sizeof(double)))) return rc;
    if ((rc = ensure(ctx, mean, (size_t)chunk * (size_t)M * sizeof(double)))) return rc;   // [chunk][M]
    if ((rc = ensure_results(ctx, chunk))) return rc;
    const int tau_sorted = is_sorted(tau, M);
    ChunkTables tb;
    for (int64_t b0 = 0; b0 < B; b0 += chunk) {
        const int64_t nb = std::min(B - b0, chunk);
        DrawChunk m;
        if ((rc = upload_draws(ctx, J, b0, nb, in.A, in.Bc, per_draw ? in.C : nullptr, in.D, in.mu, in.nu, m))) return rc;
        if (plan.windowed && (per_draw || b0 == 0) && (rc = build_tables(ds, s, per_draw, nb, m, btabs, &gtabs, tb))) return rc;
        ScanParams p = chunk_params(ds, s, per_draw, nb, m, tb);
        p.out = (double*)ctx->bout.p; p.status = (int32_t*)ctx->bst.p;
        g_last_kernel = plan.name;
        if (plan.windowed) {
            p.gw = (double*)stores.p;
            // -z = -K^-1 (y - mu) [nb][N] into the head of the Q workspace
            rc = pioran_launch_block_solve(p, tb.btab, tb.gtab, (double*)qws.p, ctx->stream);
            if (!rc) rc = pioran_launch_predict_from_gy(p, (double*)qws.p, (double*)tauws.p, ds->t, M, (const double*)taus.p, (double*)mean.p, ctx->stream,
                                                        per_draw, tau_sorted);
        } else {
            rc = pioran_launch_predict(p, (double*)stores.p, ds->t, M, (const double*)taus.p, (double*)mean.p, ctx->stream);
        }
        if (rc) { ctx->last_err = "prediction launch failed"; return rc; }
        if ((rc = download(ctx, mean_out + b0 * M, mean.p, (size_t)nb * M * sizeof(double)))) return rc;
        if ((rc = download_results(ctx, nullptr, status, b0, nb))) return rc;
        SYNC(ctx);
    }
    return PIORAN_OK;
}

int pioran_celerite_predict(pioran_ds* ds, int64_t B, int64_t J, const double* A, const double* Bc, const double* C,
                            const double* Dd, int cd_shared, const double* mu, const double* nu, int64_t M, const double* tau,
                            double* mean_out, int32_t* status)
{
    if (!ds || B < 1 || J < 1 || M < 1 || !A || !Bc || !C || !Dd || !tau || !mean_out) return PIORAN_ERR_ARG;
    const DrawChunk in{A, Bc, C, Dd, mu, nu, nullptr, nullptr};
    if (cd_shared || B == 1) return predict_batch(ds, false, B, J, in, M, tau, mean_out, status);
    const int rc = predict_batch(ds, true, B, J, in, M, tau, mean_out, status);
    if (rc != PIORAN_ERR_UNSUPPORTED) return rc;
    return each_draw(B, [&](int64_t b) { return predict_batch(ds, false, 1, J, in.from_draw(b, J, 0), M, tau, mean_out + b * M, at(status, b)); });
}

// ---- posterior variance at new times through the factorisation (celerite_predict.hip) ------------------------------------------------
// shared (c, d), tau ASCENDING (the caller below sorts); draws in chunks sized to the free memory
static int predict_var_shared(pioran_ds* ds, int64_t B, int64_t J, const DrawChunk& in, int64_t M, const double* tau, double* var_out, int32_t* status)
{
    pioran_ctx* ctx = ds->ctx;
    PrepState& s = ds->host;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    PendingGuard pending_guard(ctx);
    int rc;
    if ((rc = prepare_shared(ds, B, J, in.Bc, in.C, in.D))) return rc;
    EntryPlan plan;
    if ((rc = plan_entry(ds, s, Entry::predict_var, B, false, 0, plan))) return rc;
    if (M == 0) {
        if (status) for (int64_t b = 0; b < B; ++b) status[b] = 0;
        return PIORAN_OK;
    }
    int64_t chunk = std::min(B, plan.chunk_cap);
    auto need = [&](int64_t nb) { return pioran_predict_var_workspace_doubles(nb, ds->N, s.R, M) * sizeof(double); };
    rc = size_chunk(ctx, chunk, {&ctx->bwork}, need, [&](int64_t nb) {
        return ensure_each(ctx, {{&ctx->bwork, need(nb)}, {&ctx->bY, (size_t)nb * (size_t)M * sizeof(double)}});
    });
    if (rc) return rc;
    if ((rc = ensure(ctx, ctx->bK, pioran_predict_tau_workspace_doubles(M, s.R, 1) * sizeof(double)))) return rc;
    if ((rc = upload(ctx, ctx->bshift, tau, (size_t)M * sizeof(double)))) return rc;
    if ((rc = ensure_results(ctx, chunk))) return rc;
    for (int64_t b0 = 0; b0 < B; b0 += chunk) {
        const int64_t nb = std::min(B - b0, chunk);
        DrawChunk m;
        if ((rc = upload_draws(ctx, J, b0, nb, in.A, in.Bc, nullptr, nullptr, nullptr, in.nu, m))) return rc;
        ScanParams p = shared_params(ds, s, nb, m);
        p.out = (double*)ctx->bout.p;     // (the status comes from the variance kernel itself: bst below)
        g_last_kernel = plan.name;
        rc = pioran_launch_predict_var(p, (double*)ctx->bwork.p, (double*)ctx->bK.p, ds->t, M, (const double*)ctx->bshift.p, (double*)ctx->bY.p,
                                       (int32_t*)ctx->bst.p, ctx->stream);
        if (rc) { ctx->last_err = "variance launch failed"; return rc; }
        if ((rc = download(ctx, var_out + b0 * M, ctx->bY.p, (size_t)nb * M * sizeof(double)))) return rc;
        if ((rc = download_results(ctx, nullptr, status, b0, nb))) return rc;
        SYNC(ctx);
    }
    return PIORAN_OK;
}

int pioran_celerite_predict_var(pioran_ds* ds, int64_t B, int64_t J, const double* A, const double* Bc, const double* C, const double* Dd,
                                int cd_shared, const double* nu, int64_t M, const double* tau, double* var_out, int32_t* status)
{
    if (!ds || B < 1 || J < 1 || M < 0 || !A || !Bc || !C || !Dd || (M > 0 && (!tau || !var_out))) return PIORAN_ERR_ARG;
    for (int64_t m = 0; m < M; ++m)
        if (!std::isfinite(tau[m])) return PIORAN_ERR_ARG;
    // the kernels walk the evaluation times in ascending order: sort an index, scatter the result back
    const bool sorted = is_sorted(tau, M);
    std::vector<int64_t> idx;
    std::vector<double> ts, vs;
    if (!sorted) {
        idx.resize((size_t)M);
        for (int64_t m = 0; m < M; ++m) idx[(size_t)m] = m;
        std::stable_sort(idx.begin(), idx.end(), [&](int64_t x, int64_t y) { return tau[x] < tau[y]; });
        ts.resize((size_t)M);
        for (int64_t m = 0; m < M; ++m) ts[(size_t)m] = tau[idx[(size_t)m]];
        vs.resize((size_t)B * (size_t)M);
    }
    const double* tq = sorted ? tau : ts.data();
    double* vq = sorted ? var_out : vs.data();
    const DrawChunk in{A, Bc, C, Dd, nullptr, nu, nullptr, nullptr};
    // (c, d) per draw: there is no per-draw-table form, every draw is its own one-draw batch with its own table
    const int rc = cd_shared || B == 1
                       ? predict_var_shared(ds, B, J, in, M, tq, vq, status)
                       : each_draw(B, [&](int64_t b) { return predict_var_shared(ds, 1, J, in.from_draw(b, J, 0), M, tq, vq + b * M, at(status, b)); });
    if (rc) return rc;
    if (!sorted)
        for (int64_t b = 0; b < B; ++b)
            for (int64_t m = 0; m < M; ++m) var_out[b * M + idx[(size_t)m]] = vs[(size_t)(b * M + m)];
    return PIORAN_OK;
}

// ---- value and gradient ------------------------------------------------------------------------------------------------------------
// shift / grad_shift != nullptr: the shifted log-flux models (the data set holds raw flux and yerr^2); grad_y / grad_sigma2 then refer to the
// TRANSFORMED series of each draw.  per_draw (CARMA kernels, QPO features, free Celerite sums under NUTS): the windowed reverse mode with one pair of
// tables per draw, all chains of a chunk in one launch — 16 chains in the time of one instead of 16 one-draw calls; it has no shifted form.
// td != nullptr (shared (c, d) only): the draws are approx of the sampled parameters — `in` holds mu, nu alone, a chunk's (a, b) are made on the device
// (stage_draws), its grad_a, grad_b go through the reverse mode of approx there (theta_grads), and (c, d), with the terms that keep one row, are the grid's.
static int logl_grad_batch(pioran_ds* ds, bool per_draw, int64_t B, int64_t J, const DrawChunk& in, const double* shift, double* out, int32_t* status,
                           const GradPtrs& grad, double* grad_shift, const ThetaDraws* td = nullptr)
{
    pioran_ctx* ctx = ds->ctx;
    PrepState& s = ds->host;
    const int flags = (shift ? kGradShift : 0) | (grad.c ? kGradC : 0) | (grad.d ? kGradD : 0) | (grad.y || grad.s2 ? kGradSeries : 0);
    if (per_draw && entry_plan(Entry::grad, (int32_t)(2 * J), (int32_t)J, 0, B, true, flags, ctx->opt).rc) return PIORAN_ERR_UNSUPPORTED;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    PendingGuard pending_guard(ctx);
    int rc;
    if ((rc = td ? prepare_state(ds, s, J, td->c.data(), td->d.data(), td->real.data()) : prepare_draws(ds, per_draw, B, J, in.Bc, in.C, in.D))) return rc;
    EntryPlan plan;
    if ((rc = plan_entry(ds, s, Entry::grad, B, per_draw, flags, plan))) return rc;
    const int64_t N = ds->N;
    // buffer roles: the reverse mode's workspace | a chunk's forward tables (per_draw) or its transformed series Y | S2 (shift): never both | the reverse
    // table(s) | grad_a | grad_b | grad_c | grad_d of a chunk | grad_nu | grad_mu | shift | grad_shift.  The series gradients: bY, bS2.
    pioran_ctx::Buf &ws = ctx->bwork, &btabs = ctx->bscratch, &shifted = ctx->bscratch, &gtabs = ctx->bgtab, &terms = ctx->bK, &scalars = ctx->bq,
                    &shifts = ctx->bshift;
    // The windowed reverse mode (celerite_block.hip), many chains: the one-draw-per-wavefront reverse mode (celerite_tile.hip), else step by step
    auto ws_bytes = [&](int64_t nb) {
        return (plan.tile ? pioran_tile_grad_workspace_doubles(nb, N, s.R)
                         : (plan.windowed ? pioran_block_grad_workspace_doubles(nb, N, s.R) : pioran_grad_workspace_doubles(nb, N, s.R))) * sizeof(double);
    };
    // doubles of a draw's own forward and reverse table (per_draw: they are part of what a chunk needs)
    const size_t bt = per_draw ? pioran_block_table_doubles(N, s.R, s.J) : 0, gt = per_draw ? pioran_block_gtab_doubles(N, s.R) : 0;
    auto need = [&](int64_t nb) { return ws_bytes(nb) + (size_t)nb * (bt + gt) * sizeof(double); };
    auto grow = [&](int64_t nb) {
        return ensure_each(ctx, {{&ws, ws_bytes(nb)}, {&btabs, (size_t)nb * bt * sizeof(double)}, {&gtabs, (size_t)nb * gt * sizeof(double)}});
    };
    // Step by step, the workspace per draw is (m, D) of every step + S at the checkpoints + two replayed segments (celerite_wide.hip)
    int64_t chunk = std::min(B, plan.chunk_cap);
    if (plan.tile) {
        // whole passes of 2048 (1024) chains.  A sizing rule of its own: the limit holds for the buffer as a whole ("limit + what it holds" let the
        // second call grow a 16 GB buffer to 31 GB), and the chunk is cut by 1024 chains, then halved
        size_t free_b = 0;
        if (device_free_bytes(free_b)) {
            const size_t allowed = ws_allow(ctx, free_b + ws.cap);
            while (chunk > 1 && ws_bytes(chunk) > allowed) chunk = chunk > 1024 ? chunk - 1024 : chunk / 2;
        }
        if ((rc = ensure(ctx, ctx->bpair, pioran_tile_workspace_doubles(chunk, N) * sizeof(double)))) return rc;
        while ((rc = grow(chunk)) == PIORAN_ERR_ALLOC && chunk > 1) chunk /= 2;
    } else {
        rc = per_draw ? size_chunk(ctx, chunk, {&ws, &btabs, &gtabs}, need, grow) : size_chunk(ctx, chunk, {&ws}, need, grow);
    }
    if (rc) return rc;
    // shared (c, d): the reverse pass's table (C o v, C o x in C/D order, C_K, sigma2): 13 KB per window, rebuilt per call (10 us)
    if (plan.windowed && !per_draw && (rc = ensure(ctx, gtabs, pioran_block_gtab_doubles(N, s.R) * sizeof(double)))) return rc;
    const size_t cj = (size_t)chunk * (size_t)J * sizeof(double), cn = (size_t)chunk * (size_t)N * sizeof(double);
    if ((rc = ensure(ctx, terms, 4 * cj))) return rc;
    if ((rc = ensure(ctx, scalars, 2 * chunk * sizeof(double)))) return rc;
    const bool want_series = grad.y || grad.s2 || shift;   // the shift's chain rule needs both series gradients
    if (want_series && (rc = ensure(ctx, ctx->bY, cn))) return rc;
    if (want_series && (rc = ensure(ctx, ctx->bS2, cn))) return rc;
    if (shift && (rc = ensure(ctx, shifted, 2 * cn))) return rc;
    if (shift && (rc = ensure(ctx, shifts, 2 * chunk * sizeof(double)))) return rc;
    if ((rc = ensure_results(ctx, chunk))) return rc;
    if (td && (rc = ensure_theta_grads(ctx, *td, chunk))) return rc;
    const bool timed = td && ctx->opt.theta_events != 0;
    auto mark = [&](int slot) { return timed ? hipEventRecord(ctx->ev[slot], ctx->stream) : hipSuccess; };
    if (!per_draw && (rc = ensure_aux(ctx))) return rc;   // (the step-by-step reverse pass's; the shared form creates it whichever kernel it takes)
    const GradPtrs dev = grad_chunk(ctx, terms, scalars, chunk, J);
    ChunkTables tb;
    for (int64_t b0 = 0; b0 < B; b0 += chunk) {
        const int64_t nb = std::min(B - b0, chunk);
        DrawChunk m;
        if (b0 == 0) HIPCHK(ctx, mark(4));
        if ((rc = stage_draws(ctx, J, b0, nb, in, per_draw, td, m))) return rc;
        if (b0 == 0) HIPCHK(ctx, mark(5));
        if (plan.windowed && (per_draw || b0 == 0) && (rc = build_tables(ds, s, per_draw, nb, m, btabs, &gtabs, tb))) return rc;
        ScanParams p = chunk_params(ds, s, per_draw, nb, m, tb);
        p.out = (double*)ctx->bout.p; p.status = (int32_t*)ctx->bst.p;
        p.g_y = want_series ? (double*)ctx->bY.p : nullptr;
        p.g_s2 = want_series ? (double*)ctx->bS2.p : nullptr;
        double* dshift = (double*)shifts.p;
        if (shift) {
            HIPCHK(ctx, hipMemcpyAsync(dshift, shift + b0, nb * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
            double* dYt = (double*)shifted.p; double* dSt = dYt + (size_t)chunk * (size_t)N;
            if ((rc = pioran_launch_shift_transform(N, nb, ds->y, ds->s2, dshift, dYt, dSt, ctx->stream))) return rc;
            p.Y = dYt; p.S2 = dSt;
        }
        double* const dgc = grad.c ? dev.c : nullptr; double* const dgd = grad.d ? dev.d : nullptr;
        g_last_kernel = plan.name;
        if (plan.tile) {
            p.gw = (double*)ws.p;
            rc = pioran_launch_tile_grad(p, tb.btab, tb.gtab, (double*)ctx->bpair.p, dev.a, dev.b, dev.nu, dev.mu, dgc, dgd, ctx->stream);
        } else if (plan.windowed) {
            p.gw = (double*)ws.p;
            rc = pioran_launch_block_grad(p, tb.btab, tb.gtab, dev.a, dev.b, dev.nu, dev.mu, dgc, dgd, ctx->stream);
        } else {
            rc = pioran_launch_scan_wide_grad(p, (double*)ws.p, dev.a, dev.b, dgc, dgd, dev.nu, dev.mu, ctx->stream, ctx->aux, ctx->gev);
        }
        if (rc) { ctx->last_err = "gradient launch failed"; return rc; }
        if (shift) {
            rc = pioran_launch_shift_grad(N, nb, ds->y, ds->s2, dshift, p.g_y, p.g_s2, dshift + chunk, ctx->stream);
            if (rc) return rc;
            if ((rc = download(ctx, grad_shift + b0, dshift + chunk, nb * sizeof(double)))) return rc;
        }
        if ((rc = download_results(ctx, out, status, b0, nb))) return rc;
        if ((rc = download_grads(ctx, grad.from_draw(b0, J, N), dev, nb, J, N))) return rc;
        if (td) {
            if (b0 == 0) HIPCHK(ctx, mark(6));
            if ((rc = theta_grads(ctx, *td, b0, nb, dev.a, dev.b))) return rc;
            if (b0 == 0) HIPCHK(ctx, mark(7));
        }
        // Chunks follow each other on the stream without a host synchronisation in between (round 4): every transfer is stream-ordered
        // and staged through pinned memory, which drains itself when it fills (pin_reserve); only the large series gradients, which go
        // straight to the caller's pageable memory, are waited for per chunk.  (No change in time: 4096 chains are 16 launches of 7.5 ms, 122 ms.)
        // Both forms: a chunk with (c, d) per draw adds uploads of C, D (upload_draws) and two table launches, all on the same stream.
        if (want_series) SYNC(ctx);
    }
    SYNC(ctx);
    return PIORAN_OK;
}

static int logl_grad_impl(pioran_ds* ds, int64_t B, int64_t J, const double* A, const double* Bc, const double* C,
                          const double* Dd, int cd_shared, const double* mu, const double* nu, const double* shift, double* out,
                          int32_t* status, const GradPtrs& grad, double* grad_shift)
{
    if (!ds || B < 1 || J < 1 || !A || !Bc || !C || !Dd || !out || !grad.a || !grad.b) return PIORAN_ERR_ARG;
    if ((shift == nullptr) != (grad_shift == nullptr)) return PIORAN_ERR_ARG;
    const DrawChunk in{A, Bc, C, Dd, mu, nu, nullptr, nullptr};
    if (cd_shared || B == 1) return logl_grad_batch(ds, false, B, J, in, shift, out, status, grad, grad_shift);
    // per-draw (c, d) — CARMA, QPO features, free Celerite sums under NUTS (a handful of chains): all chains in one launch of the
    // windowed reverse mode where the shape fits it, else every draw is its own one-draw batch with its own table
    const int rc = logl_grad_batch(ds, true, B, J, in, shift, out, status, grad, grad_shift);
    if (rc != PIORAN_ERR_UNSUPPORTED) return rc;
    return each_draw(B, [&](int64_t b) {
        return logl_grad_batch(ds, false, 1, J, in.from_draw(b, J, 0), at(shift, b), out + b, at(status, b), grad.from_draw(b, J, ds->N), at(grad_shift, b));
    });
}

// The gradient of a batch whose coefficients (hA .. hD [B][J], (c, d) per draw) were made on the device from sampled parameters and fetched (QPO features,
// CARMA): the reverse mode of the host-pointer gradient entries on them, their routing and their kernels.  g = grad_a .. grad_d [B][J]: the caller's, or
// all nullptr — they are then made to point into `inter`, for the model's own reverse-mode step to read.  A draw with rejected[b] != 0 ran on benign
// coefficients: log L = -inf, status 3, exact zeros in every gradient row.
static int grad_through_host_coefs(pioran_ds* ds, int64_t B, int64_t J, const double* hA, const double* hB, const double* hC, const double* hD,
                                   const int32_t* rejected, const double* mu, const double* nu, const double* shift, double* out, int32_t* status,
                                   double* grad_nu, double* grad_mu, double* grad_shift, double* (&g)[4], std::vector<double>& inter)
{
    const size_t bj = (size_t)B * (size_t)J;
    if (!g[0]) {
        inter.resize(4 * bj);
        for (int k = 0; k < 4; ++k) g[k] = inter.data() + k * bj;
    }
    std::vector<int32_t> st((size_t)B, 0);
    if (const int rc = logl_grad_impl(ds, B, J, hA, hB, hC, hD, 0, mu, nu, shift, out, st.data(), {g[0], g[1], g[2], g[3], grad_nu, grad_mu, nullptr, nullptr},
                                      grad_shift))
        return rc;
    for (int64_t b = 0; b < B; ++b) {
        if (!rejected[b]) continue;
        out[b] = -INFINITY; st[(size_t)b] = 3;
        for (double* gk : g) std::fill(gk + b * J, gk + (b + 1) * J, 0.0);
        if (grad_nu) grad_nu[b] = 0.0;
        if (grad_mu) grad_mu[b] = 0.0;
        if (grad_shift) grad_shift[b] = 0.0;
    }
    if (status) std::memcpy(status, st.data(), (size_t)B * sizeof(int32_t));
    return PIORAN_OK;
}

int pioran_celerite_logl_grad(pioran_ds* ds, int64_t B, int64_t J, const double* A, const double* Bc, const double* C,
                              const double* Dd, int cd_shared, const double* mu, const double* nu, double* out, int32_t* status,
                              double* grad_a, double* grad_b, double* grad_c, double* grad_d, double* grad_nu, double* grad_mu,
                              double* grad_y, double* grad_sigma2)
{
    return logl_grad_impl(ds, B, J, A, Bc, C, Dd, cd_shared, mu, nu, nullptr, out, status,
                          {grad_a, grad_b, grad_c, grad_d, grad_nu, grad_mu, grad_y, grad_sigma2}, nullptr);
}

int pioran_celerite_logl_grad_shift(pioran_ds* ds, int64_t B, int64_t J, const double* A, const double* Bc, const double* C,
                                    const double* Dd, int cd_shared, const double* mu, const double* nu, const double* shift,
                                    double* out, int32_t* status, double* grad_a, double* grad_b, double* grad_c, double* grad_d,
                                    double* grad_nu, double* grad_mu, double* grad_shift)
{
    if (!shift || !grad_shift) return PIORAN_ERR_ARG;
    return logl_grad_impl(ds, B, J, A, Bc, C, Dd, cd_shared, mu, nu, shift, out, status,
                          {grad_a, grad_b, grad_c, grad_d, grad_nu, grad_mu, nullptr, nullptr}, grad_shift);
}

int pioran_logpdf_batch_theta_grad(pioran_ds* ds, int64_t B, int model, int64_t n_components, int basis, int is_integrated_power, double f_min,
                                   double f_max, double S_low, double S_high, const double* theta, const double* norm, const double* mu, const double* nu,
                                   const double* shift, double* out, int32_t* status, double* grad_theta, double* grad_norm, double* grad_nu,
                                   double* grad_mu, double* grad_shift, double* grad_a, double* grad_b)
{
    if (!ds || B < 1 || !theta || !norm || !out || !grad_theta || !grad_norm || model < 0 || model > 1 || basis < 0 || basis > 1) return PIORAN_ERR_ARG;
    if ((nu == nullptr) != (grad_nu == nullptr) || (mu == nullptr) != (grad_mu == nullptr) || (shift == nullptr) != (grad_shift == nullptr) ||
        (grad_a == nullptr) != (grad_b == nullptr))
        return PIORAN_ERR_ARG;
    pioran_ctx* ctx = ds->ctx;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    PendingGuard pending_guard(ctx);
    ThetaDraws td;
    int rc = stage_theta(ctx, B, model, n_components, basis, is_integrated_power, f_min, f_max, S_low, S_high, theta, norm, td);
    if (rc) return rc;
    td.grad_theta = grad_theta; td.grad_norm = grad_norm;
    const DrawChunk in{nullptr, nullptr, nullptr, nullptr, mu, nu, nullptr, nullptr};
    return logl_grad_batch(ds, false, B, td.terms(), in, shift, out, status, {grad_a, grad_b, nullptr, nullptr, grad_nu, grad_mu, nullptr, nullptr},
                           grad_shift, &td);
}

int pioran_approx_vjp_batch(pioran_ctx* ctx, int64_t B, int model, int64_t n_components, int basis, int is_integrated_power, double f_min, double f_max,
                            double S_low, double S_high, const double* theta, const double* norm, const double* grad_a, const double* grad_b,
                            double* grad_theta, double* grad_norm)
{
    if (!ctx || B < 1 || !theta || !norm || !grad_a || !grad_b || !grad_theta || !grad_norm || model < 0 || model > 1 || basis < 0 || basis > 1)
        return PIORAN_ERR_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    PendingGuard pending_guard(ctx);
    ThetaDraws td;
    int rc = stage_theta(ctx, B, model, n_components, basis, is_integrated_power, f_min, f_max, S_low, S_high, theta, norm, td);
    if (rc) return rc;
    td.grad_theta = grad_theta; td.grad_norm = grad_norm;
    // grad_a | grad_b of the batch where the gradient entries keep a chunk's (grad_chunk)
    const size_t bj = (size_t)B * (size_t)td.terms();
    double* dga;
    if ((rc = upload_cotangents(ctx, {grad_a, grad_b}, bj, dga))) return rc;
    if ((rc = ensure_theta_grads(ctx, td, B))) return rc;
    if ((rc = theta_grads(ctx, td, 0, B, dga, dga + bj))) return rc;
    SYNC(ctx);
    return PIORAN_OK;
}

// ---- continuum + QPO features from their sampled parameters: the gradient (approx.hip approx_qpo_vjp_kernel) ----------------------------------
static const char* const kApproxQpoVjpName = "approx with features (reverse mode of the coefficients)";

// what both entries can see without looking at an array
static int qpo_refuse(const void* handle, int64_t B, int model, int64_t n_components, int basis, const void* theta, const void* norm, int64_t n_qpo,
                      const void* qpo)
{
    if (!handle || B < 1 || !theta || !norm || model < 0 || model > 1 || basis < 0 || basis > 1) return PIORAN_ERR_ARG;
    if (n_components < 2 || n_components > 256 || n_qpo < 1 || n_qpo > 8 || !qpo) return PIORAN_ERR_ARG;
    return PIORAN_OK;
}

// (ga, gb, gc, gd) [B][Jt] of the caller through approx_qpo_vjp_kernel on the staged batch to the caller's grad_theta [B][P], grad_norm [B],
// grad_qpo [B][n_qpo][3].  bthout: grad_theta | grad_norm | scratch [2 J][B] | grad_qpo
static int qpo_vjp_from_host(pioran_ctx* ctx, int64_t B, const ThetaDraws& td, const double* ga, const double* gb, const double* gc, const double* gd,
                             double* grad_theta, double* grad_norm, double* grad_qpo)
{
    int rc;
    const size_t bj = (size_t)B * (size_t)(td.terms() + td.n_qpo), nth = (size_t)B * td.P, nq = (size_t)B * 3 * (size_t)td.n_qpo;
    double* dg;
    if ((rc = upload_cotangents(ctx, {ga, gb, gc, gd}, bj, dg))) return rc;
    if ((rc = ensure_theta_grads(ctx, td, B))) return rc;
    double* gth = (double*)ctx->bthout.p; double* gn = gth + nth; double* scratch = gn + B; double* gq = scratch + 2 * (size_t)td.J * (size_t)B;
    if ((rc = timed_launch(ctx, kApproxQpoVjpName, 6, ctx->opt.theta_events != 0, "approx reverse-mode launch failed", [&] {
            return pioran_launch_approx_qpo_vjp(B, td.model, td.P, td.J, td.basis, td.integrated, td.f_min, td.f_max, td.sp, td.w, td.LU, td.piv, td.theta,
                                                td.norm, td.n_qpo, td.qpo, dg, dg + bj, dg + 2 * bj, dg + 3 * bj, scratch, gth, gn, gq, ctx->stream);
        })))
        return rc;
    if ((rc = download(ctx, grad_theta, gth, nth * sizeof(double)))) return rc;
    if ((rc = download(ctx, grad_norm, gn, (size_t)B * sizeof(double)))) return rc;
    return download(ctx, grad_qpo, gq, nq * sizeof(double));
}

int pioran_approx_qpo_vjp_batch(pioran_ctx* ctx, int64_t B, int model, int64_t n_components, int basis, int is_integrated_power, double f_min, double f_max,
                                double S_low, double S_high, const double* theta, const double* norm, int64_t n_qpo, const double* qpo,
                                const double* grad_a, const double* grad_b, const double* grad_c, const double* grad_d, double* grad_theta,
                                double* grad_norm, double* grad_qpo)
{
    if (const int rc = qpo_refuse(ctx, B, model, n_components, basis, theta, norm, n_qpo, qpo)) return rc;
    if (!grad_a || !grad_b || !grad_c || !grad_d || !grad_theta || !grad_norm || !grad_qpo) return PIORAN_ERR_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    PendingGuard pending_guard(ctx);
    ThetaDraws td;
    int rc = stage_theta(ctx, B, model, n_components, basis, is_integrated_power != 0, f_min, f_max, S_low, S_high, theta, norm, td, n_qpo, qpo);
    if (rc) return rc;
    if ((rc = qpo_vjp_from_host(ctx, B, td, grad_a, grad_b, grad_c, grad_d, grad_theta, grad_norm, grad_qpo))) return rc;
    SYNC(ctx);
    return PIORAN_OK;
}

int pioran_logpdf_batch_theta_qpo_grad(pioran_ds* ds, int64_t B, int model, int64_t n_components, int basis, int is_integrated_power, double f_min,
                                       double f_max, double S_low, double S_high, const double* theta, const double* norm, const double* mu,
                                       const double* nu, const double* shift, int64_t n_qpo, const double* qpo, double* out, int32_t* status,
                                       double* grad_theta, double* grad_norm, double* grad_qpo, double* grad_nu, double* grad_mu, double* grad_shift,
                                       double* coef_a, double* coef_b, double* coef_c, double* coef_d, double* grad_a, double* grad_b, double* grad_c,
                                       double* grad_d)
{
    if (const int rc = qpo_refuse(ds, B, model, n_components, basis, theta, norm, n_qpo, qpo)) return rc;
    if (!out || !grad_theta || !grad_norm || !grad_qpo) return PIORAN_ERR_ARG;
    if ((nu == nullptr) != (grad_nu == nullptr) || (mu == nullptr) != (grad_mu == nullptr) || (shift == nullptr) != (grad_shift == nullptr)) return PIORAN_ERR_ARG;
    const int n_inter = (coef_a != nullptr) + (coef_b != nullptr) + (coef_c != nullptr) + (coef_d != nullptr) + (grad_a != nullptr) + (grad_b != nullptr) +
                        (grad_c != nullptr) + (grad_d != nullptr);
    if (n_inter != 0 && n_inter != 8) return PIORAN_ERR_ARG;
    const int P = model == 0 ? 3 : 5;
    const int64_t J = n_components, Jc = basis == 0 ? J : 2 * J, Jt = Jc + n_qpo;
    // rows of the celerite state: two per SHO term and per feature, three per DRWCelerite pair (its second term keeps the cos row only)
    if ((basis == 0 ? 2 * J : 3 * J) + 2 * n_qpo > pioran_wide_supported_rows()) return PIORAN_ERR_UNSUPPORTED;
    // a draw the reference could not evaluate (non-finite theta, norm or feature; f0 <= 0; Q <= 1/2: DomainError of convert_feature) runs on benign
    // parameters and is overwritten afterwards
    std::vector<double> th(theta, theta + B * P), nm(norm, norm + B), qp(qpo, qpo + B * n_qpo * 3);
    std::vector<int32_t> bad((size_t)B, 0);
    const double f_mid = std::sqrt(f_min * f_max);
    for (int64_t b = 0; b < B; ++b) {
        bool ok = std::isfinite(nm[b]);
        for (int k = 0; k < P; ++k) ok = ok && std::isfinite(th[b * P + k]);
        for (int64_t q = 0; q < n_qpo; ++q) {
            const double* f = &qp[(b * n_qpo + q) * 3];
            ok = ok && std::isfinite(f[0]) && std::isfinite(f[1]) && std::isfinite(f[2]) && f[1] > 0.0 && f[2] > 0.5;
        }
        if (ok) continue;
        bad[(size_t)b] = 1;
        const double benign[5] = {1.0, f_mid, 3.0, f_max, 4.0};
        std::copy(benign, benign + P, th.begin() + b * P);
        nm[b] = 1.0;
        for (int64_t q = 0; q < n_qpo; ++q) { double* f = &qp[(b * n_qpo + q) * 3]; f[0] = 1.0; f[1] = f_mid; f[2] = 2.0; }
    }
    pioran_ctx* ctx = ds->ctx;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    ThetaDraws td;
    int rc;
    const size_t bj = (size_t)B * (size_t)Jt;
    std::vector<double> hA(bj), hB(bj), hC(bj), hD(bj);
    {   // approx_kernel on the staged batch: (a, b) and the features' (c, d) [B][Jt] into bA .. bD, and from there to the host
        PendingGuard guard(ctx);
        if ((rc = stage_theta(ctx, B, model, J, basis, is_integrated_power != 0, f_min, f_max, S_low, S_high, th.data(), nm.data(), td, n_qpo, qp.data())))
            return rc;
        const size_t bytes = bj * sizeof(double);
        DrawChunk m;
        if ((rc = stage_draws(ctx, Jt, 0, B, DrawChunk{}, false, &td, m))) return rc;
        if ((rc = download(ctx, hA.data(), ctx->bA.p, bytes))) return rc;
        if ((rc = download(ctx, hB.data(), ctx->bB.p, bytes))) return rc;
        if ((rc = download(ctx, hC.data(), ctx->bC.p, bytes))) return rc;
        if ((rc = download(ctx, hD.data(), ctx->bD.p, bytes))) return rc;
        SYNC(ctx);
    }
    for (int64_t b = 0; b < B; ++b) {   // the continuum's (c, d) are the grid's: approx_kernel writes the features' columns only
        std::copy(td.c.begin(), td.c.end(), hC.begin() + b * Jt);
        std::copy(td.d.begin(), td.d.end(), hD.begin() + b * Jt);
    }
    std::vector<double> inter;
    double* g[4] = {grad_a, grad_b, grad_c, grad_d};
    if ((rc = grad_through_host_coefs(ds, B, Jt, hA.data(), hB.data(), hC.data(), hD.data(), bad.data(), mu, nu, shift, out, status, grad_nu, grad_mu, grad_shift,
                                      g, inter)))
        return rc;
    if (n_inter) {
        std::copy(hA.begin(), hA.end(), coef_a); std::copy(hB.begin(), hB.end(), coef_b);
        std::copy(hC.begin(), hC.end(), coef_c); std::copy(hD.begin(), hD.end(), coef_d);
    }
    PendingGuard guard(ctx);
    if ((rc = qpo_vjp_from_host(ctx, B, td, g[0], g[1], g[2], g[3], grad_theta, grad_norm, grad_qpo))) return rc;
    SYNC(ctx);
    for (int64_t b = 0; b < B; ++b) {   // (the chain of zero cotangents is zero up to its sign)
        if (!bad[(size_t)b]) continue;
        std::fill(grad_theta + b * P, grad_theta + (b + 1) * P, 0.0);
        grad_norm[b] = 0.0;
        std::fill(grad_qpo + b * n_qpo * 3, grad_qpo + (b + 1) * n_qpo * 3, 0.0);
    }
    return PIORAN_OK;
}

// ---- simulation ----------------------------------------------------------------------------------------------------------------------
// n doubles of a chunk's realisations (bS2) straight into the caller's array, and wait for them
static int download_realisations(pioran_ctx* ctx, double* y_out, int64_t n)
{
    if (hipMemcpyAsync(y_out, ctx->bS2.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess || ctx_sync(ctx) != PIORAN_OK) {
        ctx->last_err = "simulation copy-back failed";
        return PIORAN_ERR_HIP;
    }
    return PIORAN_OK;
}

// B realisations on the caller's time stamps from the normals q [B][N]
static int simulate_batch(pioran_ctx* ctx, bool per_draw, int64_t N, int64_t B, int64_t J, const DrawChunk& in, const double* t, const double* sigma2,
                          const double* q, double* y_out)
{
    if (per_draw && entry_plan(Entry::simulate, (int32_t)(2 * J), (int32_t)J, 0, B, true, 0, ctx->opt).rc) return PIORAN_ERR_UNSUPPORTED;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    ScopedDataset series;
    int rc = series.create_zeros(ctx, N, t, sigma2);
    if (rc) return rc;
    pioran_ds* ds = series.ds;
    if ((rc = prepare_draws(ds, per_draw, B, J, in.Bc, in.C, in.D))) return rc;
    PrepState& s = ds->host;
    EntryPlan plan;
    if ((rc = plan_entry(ds, s, Entry::simulate, B, per_draw, 0, plan))) return rc;
    // buffer roles: the per-window stores | a chunk's forward tables (per_draw only) | xi | the normals | the realisations
    pioran_ctx::Buf &stores = ctx->bwork, &btabs = ctx->bscratch, &xi = ctx->bq, &noise = ctx->bY, &ysim = ctx->bS2;
    int64_t chunk = std::min(B, plan.chunk_cap);
    if (plan.windowed) {
        const size_t bt = per_draw ? pioran_block_table_doubles(N, s.R, s.J) : 0;
        auto need = [&](int64_t nb) {
            size_t d = pioran_block_store_workspace_doubles(nb, N, s.R, 3);
            if (per_draw) d += (size_t)nb * bt + 3 * (size_t)nb * (size_t)N;
            return d * sizeof(double);
        };
        auto grow = [&](int64_t nb) {
            return ensure_each(ctx, {{&stores, pioran_block_store_workspace_doubles(nb, N, s.R, 3) * sizeof(double)},
                                     {&btabs, (size_t)nb * bt * sizeof(double)},
                                     {&xi, (size_t)nb * (size_t)N * sizeof(double)},
                                     {&ctx->bst, nb * sizeof(int32_t)}});
        };
        rc = size_chunk(ctx, chunk, per_draw ? BufList{&stores, &btabs, &xi} : BufList{&stores}, need, grow, plan.shrink);
        // (no memory for the chunk the budget admits: not a smaller chunk, the step-by-step kernel)
        if (rc == PIORAN_ERR_ALLOC && !plan.shrink) { plan.leave_windowed(); chunk = std::min(B, plan.chunk_cap); rc = PIORAN_OK; }
        if (rc) return rc;
    }
    const size_t cn = (size_t)chunk * (size_t)N * sizeof(double);
    if ((rc = ensure(ctx, noise, cn))) return rc;
    if ((rc = ensure(ctx, ysim, cn))) return rc;
    if ((rc = ensure(ctx, ctx->bout, chunk * sizeof(double)))) return rc;
    ChunkTables tb;
    for (int64_t b0 = 0; b0 < B; b0 += chunk) {
        const int64_t nb = std::min(B - b0, chunk);
        DrawChunk m;
        if ((rc = upload_draws(ctx, J, b0, nb, in.A, in.Bc, per_draw ? in.C : nullptr, in.D, nullptr, nullptr, m))) return rc;
        if ((rc = upload(ctx, noise, q + b0 * N, (size_t)nb * N * sizeof(double)))) return rc;
        if (plan.windowed && (per_draw || b0 == 0) && (rc = build_tables(ds, s, per_draw, nb, m, btabs, nullptr, tb))) return rc;
        ScanParams p = chunk_params(ds, s, per_draw, nb, m, tb);
        p.out = (double*)ctx->bout.p;
        p.noise = (const double*)noise.p; p.ysim = (double*)ysim.p;
        g_last_kernel = plan.name;
        if (plan.windowed) {
            p.gw = (double*)stores.p;
            p.status = (int32_t*)ctx->bst.p;
            rc = pioran_launch_block_sim(p, tb.btab, (double*)xi.p, ctx->stream);
        } else {
            rc = pioran_launch_scan_wide_sim(p, ctx->stream);
        }
        if (rc) { ctx->last_err = "simulation launch failed"; return rc; }
        if ((rc = download_realisations(ctx, y_out + b0 * N, nb * N))) return rc;
    }
    return PIORAN_OK;
}

int pioran_celerite_simulate(pioran_ctx* ctx, int64_t N, int64_t B, int64_t J, const double* A, const double* Bc,
                             const double* C, const double* Dd, int cd_shared, const double* t, const double* sigma2,
                             const double* q, double* y_out)
{
    if (!ctx || N < 1 || B < 1 || J < 1 || !A || !Bc || !C || !Dd || !t || !sigma2 || !q || !y_out) return PIORAN_ERR_ARG;
    const DrawChunk in{A, Bc, C, Dd, nullptr, nullptr, nullptr, nullptr};
    if (cd_shared || B == 1) return simulate_batch(ctx, false, N, B, J, in, t, sigma2, q, y_out);
    const int rc = simulate_batch(ctx, true, N, B, J, in, t, sigma2, q, y_out);
    if (rc != PIORAN_ERR_UNSUPPORTED) return rc;
    return each_draw(B, [&](int64_t b) { return simulate_batch(ctx, false, N, 1, J, in.from_draw(b, J, 0), t, sigma2, q + b * N, y_out + b * N); });
}

// ---- posterior draws at new times by Matheron's rule ("(f)-4d posterior draws") ----------------------------------
//   out(tau) = mu + f~(tau) + k*(tau)' K^-1 ((y - mu) - f~(t) - eta),   eta_n = sqrt(nu sigma2_n) eps_n
// with f~ a realisation of the zero-mean prior on the merged grid T = sort(unique(t, tau)): the simulation (sigma2 = 0 on T) followed by the
// prediction on the per-draw series Y_b = y - f~_b(t) - eta_b.  Nothing between the caller's normals and the draws goes to the host.

// The merged grid of a call and its index maps (built once, on the host).  Times are merged only where they compare equal; among equal times the
// first in (t, tau) order gives the normal: a tau on a data time, or on an earlier tau, shares that one's latent value.
struct MergedGrid {
    std::vector<double> T;          // [P] ascending, distinct
    std::vector<int32_t> maps;      // origin [P] (index into (t | tau) of the first occurrence) | it [N] | itau [M] (merged indices)
    int64_t P = 0;
    void build(int64_t N, const double* t, int64_t M, const double* tau)
    {
        const int64_t n = N + M;
        auto at_ = [&](int64_t i) { return i < N ? t[i] : tau[i - N]; };
        std::vector<int64_t> idx((size_t)n);
        for (int64_t i = 0; i < n; ++i) idx[(size_t)i] = i;
        std::stable_sort(idx.begin(), idx.end(), [&](int64_t x, int64_t y) { return at_(x) < at_(y); });
        maps.assign((size_t)(2 * n), 0);
        T.clear();
        std::vector<int32_t> origin, where((size_t)n);
        for (int64_t k = 0; k < n; ++k) {
            const int64_t i = idx[(size_t)k];
            if (T.empty() || at_(i) != T.back()) { T.push_back(at_(i)); origin.push_back((int32_t)i); }
            where[(size_t)i] = (int32_t)(T.size() - 1);
        }
        P = (int64_t)T.size();
        maps.resize((size_t)(P + n));
        std::copy(origin.begin(), origin.end(), maps.begin());
        std::copy(where.begin(), where.end(), maps.begin() + P);
    }
};

// Where the draws of a call go: the caller's host arrays out [B][M] | status [B] (nullptr: not wanted), or — the summary entry — device arrays
// dev_out [.][M] | dev_status [.] that stay resident for the reduction over the draws.  from_draw: the sink of the draws from b0 on.
struct DrawSink {
    double* out = nullptr;
    int32_t* status = nullptr;
    double* dev_out = nullptr;
    int32_t* dev_status = nullptr;
    DrawSink from_draw(int64_t b0, int64_t M) const { return {at(out, b0 * M), at(status, b0), at(dev_out, b0 * M), at(dev_status, b0)}; }
};

// B draws at M times on shared (c, d).  `simds`: the scratch data set on grid.T with y = 0, sigma2 = 0.
static int rand_posterior_batch(pioran_ds* ds, pioran_ds* simds, int64_t B, int64_t J, const DrawChunk& in, const double* shift, const MergedGrid& grid,
                                int64_t M, const double* tau, const double* q_data, const double* q_new, const double* eps, const DrawSink& sink)
{
    pioran_ctx* ctx = ds->ctx;
    PrepState &s = ds->host, &ss = simds->host;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    PendingGuard pending_guard(ctx);
    int rc;
    if ((rc = prepare_shared(ds, B, J, in.Bc, in.C, in.D))) return rc;
    if ((rc = prepare_shared(simds, B, J, in.Bc, in.C, in.D))) return rc;
    EntryPlan plan;
    if ((rc = plan_entry(ds, s, Entry::rand_posterior, B, false, 0, plan))) return rc;
    const int64_t N = ds->N, P = grid.P;
    // Buffer roles.  The simulation's side and everything the chain adds live in buffers of their own (pioran_ctx::br*); the prediction's side keeps the
    // roles it has in predict_batch.  Alive together within a chunk, none shared between two roles:
    //   the caller's normals: q_data | q_new | eps                              brqd | brqn | breps
    //   the normals on the merged grid [nb][P]                                  brqT
    //   simulation: per-window stores | xi | f~ [nb][P] | log L | status        brstores | brxi | brf | brsout | brsst
    //   index maps origin [P] | it [N] | itau [M]                               brmaps
    //   residual series Y | S2 [nb][N], the shifts [nb]                         brY | brS2 | brshift
    //   prediction: per-window stores (step by step: the factor) | reverse table | -z and the Q recurrences | tau-only factors | means [nb][M] | tau
    //                                                                           bwork | bgtab | bq | bK | bY | bshift   (log L, status: bout, bst)
    //   the draws [nb][M] | their status                                        brres | brst
    //   (A, Bc, mu, nu of the chunk: bA, bB, bmu, bnu — one role, read by both sides)
    pioran_ctx::Buf &qd = ctx->brqd, &qn = ctx->brqn, &ep = ctx->breps, &qT = ctx->brqT, &sstores = ctx->brstores, &xi = ctx->brxi, &fsim = ctx->brf,
                    &sout = ctx->brsout, &sst = ctx->brsst, &maps = ctx->brmaps, &Yb = ctx->brY, &S2b = ctx->brS2, &shifts = ctx->brshift,
                    &stores = ctx->bwork, &gtabs = ctx->bgtab, &qws = ctx->bq, &tauws = ctx->bK, &mean = ctx->bY, &taus = ctx->bshift, &res = ctx->brres,
                    &rst = ctx->brst;
    // (the windowed tables of both states, or of neither)
    if (plan.windowed && (rc = ensure_btab(simds, ss)) == PIORAN_ERR_UNSUPPORTED) { plan.leave_windowed(); rc = PIORAN_OK; }
    if (rc) return rc;
    const size_t gt = plan.windowed ? pioran_block_gtab_doubles(N, s.R) : 0;
    auto work_doubles = [&](int64_t nb) {   // the two kernel families' workspaces
        return plan.windowed ? pioran_block_store_workspace_doubles(nb, P, s.R, 3) + pioran_block_store_workspace_doubles(nb, N, s.R, 2) +
                              pioran_predict_q_workspace_doubles(nb, N, s.R)
                        : pioran_predict_workspace_doubles(nb, N, s.R);
    };
    auto need = [&](int64_t nb) { return (work_doubles(nb) + (size_t)nb * (size_t)(3 * P + 4 * N + 3 * M)) * sizeof(double); };
    auto grow = [&](int64_t nb) {
        const size_t bn = (size_t)nb * (size_t)N * sizeof(double), bm = (size_t)nb * (size_t)M * sizeof(double), bp = (size_t)nb * (size_t)P * sizeof(double);
        return ensure_each(ctx, {{&qd, bn}, {&qn, bm}, {&ep, bn}, {&qT, bp}, {&fsim, bp}, {&Yb, bn}, {&S2b, bn}, {&mean, bm}, {&res, bm},
                                 {&sstores, plan.windowed ? pioran_block_store_workspace_doubles(nb, P, s.R, 3) * sizeof(double) : 0},
                                 {&xi, plan.windowed ? bp : 0},
                                 {&stores, (plan.windowed ? pioran_block_store_workspace_doubles(nb, N, s.R, 2) : pioran_predict_workspace_doubles(nb, N, s.R)) * sizeof(double)},
                                 {&qws, plan.windowed ? pioran_predict_q_workspace_doubles(nb, N, s.R) * sizeof(double) : 0},
                                 {&sout, nb * sizeof(double)}, {&sst, nb * sizeof(int32_t)}, {&rst, nb * sizeof(int32_t)}, {&shifts, nb * sizeof(double)}});
    };
    int64_t chunk = std::min(B, plan.chunk_cap);
    if ((rc = size_chunk(ctx, chunk, {&qd, &qn, &ep, &qT, &fsim, &Yb, &S2b, &mean, &res, &sstores, &xi, &stores, &qws}, need, grow))) return rc;
    if (plan.windowed && (rc = ensure_each(ctx, {{&gtabs, gt * sizeof(double)}, {&tauws, pioran_predict_tau_workspace_doubles(M, s.R, 1) * sizeof(double)}}))) return rc;
    if ((rc = upload(ctx, taus, tau, (size_t)M * sizeof(double)))) return rc;
    if ((rc = upload(ctx, maps, grid.maps.data(), grid.maps.size() * sizeof(int32_t)))) return rc;
    if ((rc = ensure_results(ctx, chunk))) return rc;
    const int32_t *origin = (const int32_t*)maps.p, *it = origin + P, *itau = it + N;
    const int tau_sorted = is_sorted(tau, M);
    const bool timed = ctx->opt.rp_events != 0;
    auto mark = [&](int slot) { return timed ? hipEventRecord(ctx->ev[slot], ctx->stream) : hipSuccess; };
    ChunkTables tb, stb;
    for (int64_t b0 = 0; b0 < B; b0 += chunk) {
        const int64_t nb = std::min(B - b0, chunk);
        DrawChunk m;
        if ((rc = upload_draws(ctx, J, b0, nb, in.A, in.Bc, nullptr, nullptr, in.mu, in.nu, m))) return rc;
        if ((rc = upload(ctx, qd, q_data + b0 * N, (size_t)nb * N * sizeof(double)))) return rc;
        if ((rc = upload(ctx, qn, q_new + b0 * M, (size_t)nb * M * sizeof(double)))) return rc;
        if ((rc = upload(ctx, ep, eps + b0 * N, (size_t)nb * N * sizeof(double)))) return rc;
        if (shift && (rc = upload(ctx, shifts, shift + b0, (size_t)nb * sizeof(double)))) return rc;
        if (plan.windowed && b0 == 0) {
            // (shared (c, d): the states' own forward tables; the buffer of per-draw tables is not touched)
            if ((rc = build_tables(ds, s, false, nb, m, ctx->bscratch, &gtabs, tb))) return rc;
            if ((rc = build_tables(simds, ss, false, nb, m, ctx->bscratch, nullptr, stb))) return rc;
        }
        if (b0 == 0) HIPCHK(ctx, mark(4));
        // 1. the normals on the merged grid
        if ((rc = pioran_launch_rp_gather(nb, N, M, P, origin, (const double*)qd.p, (const double*)qn.p, (double*)qT.p, ctx->stream))) return rc;
        if (b0 == 0) HIPCHK(ctx, mark(5));
        // 2. f~ on the merged grid (no mu, no nu: the zero-mean latent process)
        DrawChunk msim = m;
        msim.mu = msim.nu = nullptr;
        ScanParams ps = shared_params(simds, ss, nb, msim);
        ps.out = (double*)sout.p; ps.status = (int32_t*)sst.p;
        ps.noise = (const double*)qT.p; ps.ysim = (double*)fsim.p;
        if (plan.windowed) {
            ps.gw = (double*)sstores.p;
            rc = pioran_launch_block_sim(ps, stb.btab, (double*)xi.p, ctx->stream);
        } else {
            rc = pioran_launch_scan_wide_sim(ps, ctx->stream);
        }
        if (rc) { ctx->last_err = "posterior draw: simulation launch failed"; return rc; }
        if (b0 == 0) HIPCHK(ctx, mark(6));
        // 3. the series the correction is predicted from
        if ((rc = pioran_launch_rp_residual(nb, N, P, it, ds->y, ds->s2, m.nu, shift ? (const double*)shifts.p : nullptr, (const double*)fsim.p,
                                            (const double*)ep.p, (double*)Yb.p, (double*)S2b.p, ctx->stream)))
            return rc;
        if (b0 == 0) HIPCHK(ctx, mark(7));
        // 4. mu + k*' K^-1 (Y - mu)
        m.Y = (const double*)Yb.p; m.S2 = (const double*)S2b.p;
        ScanParams p = shared_params(ds, s, nb, m);
        p.out = (double*)ctx->bout.p; p.status = (int32_t*)ctx->bst.p;
        g_last_kernel = plan.name;
        if (plan.windowed) {
            p.gw = (double*)stores.p;
            rc = pioran_launch_block_solve(p, tb.btab, tb.gtab, (double*)qws.p, ctx->stream);
            if (!rc) rc = pioran_launch_predict_from_gy(p, (double*)qws.p, (double*)tauws.p, ds->t, M, (const double*)taus.p, (double*)mean.p, ctx->stream, 0,
                                                        tau_sorted);
        } else {
            rc = pioran_launch_predict(p, (double*)stores.p, ds->t, M, (const double*)taus.p, (double*)mean.p, ctx->stream);
        }
        if (rc) { ctx->last_err = "posterior draw: prediction launch failed"; return rc; }
        if (b0 == 0) HIPCHK(ctx, mark(8));
        // 5. the draws, in the caller's order of tau: into the chunk's buffer, or straight to their rows of a device sink
        const DrawSink to = sink.from_draw(b0, M);
        if ((rc = pioran_launch_rp_combine(nb, M, P, itau, (const double*)mean.p, (const double*)fsim.p, (const int32_t*)sst.p, (const int32_t*)ctx->bst.p,
                                           to.dev_out ? to.dev_out : (double*)res.p, to.dev_out ? to.dev_status : (int32_t*)rst.p, ctx->stream)))
            return rc;
        if (b0 == 0) HIPCHK(ctx, mark(9));
        // 6. download
        if (to.out && (rc = download(ctx, to.out, res.p, (size_t)nb * M * sizeof(double)))) return rc;
        if (to.out && to.status && (rc = download(ctx, to.status, rst.p, nb * sizeof(int32_t)))) return rc;
        SYNC(ctx);
    }
    return PIORAN_OK;
}

// What pioran_celerite_rand_posterior and its summary form share: the checks that need no GPU (rand_posterior_refuse), then the merged grid
// and the draws into `sink` (rand_posterior_into).
static int rand_posterior_refuse(pioran_ds* ds, int64_t B, int64_t J, const double* A, const double* Bc, const double* C, const double* Dd, int cd_shared,
                                 int64_t M, const double* tau, const double* q_data, const double* q_new, const double* eps)
{
    if (!ds || B < 1 || J < 1 || M < 1 || !A || !Bc || !C || !Dd || !tau || !q_data || !q_new || !eps) return PIORAN_ERR_ARG;
    for (int64_t m = 0; m < M; ++m)
        if (!std::isfinite(tau[m])) return PIORAN_ERR_ARG;
    const int64_t N = ds->N;
    if (N + M > 0x7fffffff) return PIORAN_ERR_UNSUPPORTED;
    // rows past the step-by-step kernels: refused before any upload or allocation (the row count prepare_shared arrives at: a term with d = 0 and
    // b = 0 in every draw of the batch keeps one row)
    auto refused = [&](int64_t nb, const double* bc, const double* dd) {
        const std::vector<int32_t> kind = classify_terms(nb, J, bc, nullptr, dd, false);
        const int64_t rows = 2 * J - std::count(kind.begin(), kind.end(), 1), cap = 1 << 20;   // (beyond any kernel: no overflow of the rule's 32 bits)
        return entry_plan(Entry::rand_posterior, (int32_t)std::min(rows, cap), (int32_t)std::min(J, cap), 0, nb, false, 0, ds->ctx->opt).rc != PIORAN_OK;
    };
    const bool one_batch = cd_shared || B == 1;
    for (int64_t b = 0; b < (one_batch ? 1 : B); ++b)
        if (refused(one_batch ? B : 1, Bc + b * J, Dd + b * J)) return PIORAN_ERR_UNSUPPORTED;
    return PIORAN_OK;
}

static int rand_posterior_into(pioran_ds* ds, int64_t B, int64_t J, const double* A, const double* Bc, const double* C, const double* Dd, int cd_shared,
                               const double* mu, const double* nu, const double* shift, int64_t M, const double* tau, const double* q_data,
                               const double* q_new, const double* eps, const DrawSink& sink)
{
    pioran_ctx* ctx = ds->ctx;
    const int64_t N = ds->N;
    const bool one_batch = cd_shared || B == 1;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // the merged grid and its index maps, once per call: the data times come back from the data set
    std::vector<double> t((size_t)N);
    HIPCHK(ctx, hipMemcpyAsync(t.data(), ds->t, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    SYNC(ctx);
    MergedGrid grid;
    grid.build(N, t.data(), M, tau);
    ScopedDataset series;
    std::vector<double> zero_s2((size_t)grid.P, 0.0);
    int rc = series.create_zeros(ctx, grid.P, grid.T.data(), zero_s2.data());
    if (rc) return rc;
    const DrawChunk in{A, Bc, C, Dd, mu, nu, nullptr, nullptr};
    if (one_batch) return rand_posterior_batch(ds, series.ds, B, J, in, shift, grid, M, tau, q_data, q_new, eps, sink);
    // (c, d) per draw: every draw is its own one-draw batch with its own tables, on the same merged grid
    return each_draw(B, [&](int64_t b) {
        return rand_posterior_batch(ds, series.ds, 1, J, in.from_draw(b, J, 0), at(shift, b), grid, M, tau, q_data + b * N, q_new + b * M, eps + b * N,
                                    sink.from_draw(b, M));
    });
}

int pioran_celerite_rand_posterior(pioran_ds* ds, int64_t B, int64_t J, const double* A, const double* Bc, const double* C, const double* Dd,
                                   int cd_shared, const double* mu, const double* nu, const double* shift, int64_t M, const double* tau,
                                   const double* q_data, const double* q_new, const double* eps, double* out, int32_t* status)
{
    if (!out) return PIORAN_ERR_ARG;
    if (const int rc = rand_posterior_refuse(ds, B, J, A, Bc, C, Dd, cd_shared, M, tau, q_data, q_new, eps)) return rc;
    DrawSink sink;
    sink.out = out;
    sink.status = status;
    return rand_posterior_into(ds, B, J, A, Bc, C, Dd, cd_shared, mu, nu, shift, M, tau, q_data, q_new, eps, sink);
}

// ---- quantiles and means over the draw axis (quantiles.hip) ------------------------------------------------------------------------------
// what both forms can see without looking at a device array
static int quantiles_refuse(const void* ctx, int64_t B, int64_t M, int64_t ldx, const void* X, int64_t Mc, const int32_t* cols, const double* ref,
                            const double* scale, int64_t Q, const double* probs, const double* quant)
{
    if (!ctx || !X || !probs || !quant || B < 1 || M < 1 || Q < 1 || ldx < M) return PIORAN_ERR_ARG;
    if (cols && Mc < 1) return PIORAN_ERR_ARG;
    if ((ref != nullptr) != (scale != nullptr)) return PIORAN_ERR_ARG;
    for (int64_t q = 0; q < Q; ++q)
        if (!(probs[q] >= 0.0 && probs[q] <= 1.0)) return PIORAN_ERR_ARG;   // NaN included
    return B > pioran_quantiles_max_draws() ? PIORAN_ERR_UNSUPPORTED : PIORAN_OK;
}

// ... and what only a host array shows
static int quantiles_refuse_host(int64_t M, int64_t Mc, const int32_t* cols, const double* scale)
{
    for (int64_t m = 0; cols && m < Mc; ++m)
        if (cols[m] < 0 || cols[m] >= M) return PIORAN_ERR_ARG;
    for (int64_t m = 0; scale && m < Mc; ++m)
        if (!std::isfinite(scale[m]) || scale[m] == 0.0) return PIORAN_ERR_ARG;
    return PIORAN_OK;
}

int pioran_quantiles_batch_dev(pioran_ctx* ctx, int64_t B, int64_t M, int64_t ldx, const double* dX, const int32_t* dstatus, const double* dshift,
                               int64_t Mc, const int32_t* dcols, const double* dref, const double* dscale, int64_t Q, const double* probs,
                               double* dquant, double* dmean, int32_t* dkept)
{
    if (const int rc = quantiles_refuse(ctx, B, M, ldx, dX, Mc, dcols, dref, dscale, Q, probs, dquant)) return rc;
    if (!dcols) Mc = M;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (const int rc = upload(ctx, ctx->bqin, probs, (size_t)Q * sizeof(double))) return rc;
    g_last_kernel = "quantiles (sort over draws)";
    return pioran_launch_quantiles(B, M, ldx, dX, dstatus, dshift, Mc, dcols, dref, dscale, Q, (const double*)ctx->bqin.p, dquant, dmean, dkept,
                                   ctx->stream);
}

// The small inputs of a reduction on the device — probs [Q] | shift [B] | ref [Mc] | scale [Mc] in bqin, cols [Mc] | kept [1] in bqidx — and
// the reduction of the resident dX [B][ldx] | dstatus into bqout = quant [Q][Mc] | mean [Mc], which go to the caller's arrays (delivered by the
// next synchronisation).  shift, cols, ref / scale, mean, kept: nullptr = not part of the call.
static int quantiles_reduce(pioran_ctx* ctx, int64_t B, int64_t M, int64_t ldx, const double* dX, const int32_t* dstatus, const double* shift, int64_t Mc,
                            const int32_t* cols, const double* ref, const double* scale, int64_t Q, const double* probs, double* quant, double* mean,
                            int32_t* kept)
{
    int rc;
    std::vector<double> in(probs, probs + Q);
    const size_t o_shift = in.size();
    if (shift) in.insert(in.end(), shift, shift + B);
    const size_t o_ref = in.size();
    if (ref) { in.insert(in.end(), ref, ref + Mc); in.insert(in.end(), scale, scale + Mc); }
    // the two calls of the summary entry follow each other on the stream without a synchronisation: the second must not move the buffers the first reads
    if ((rc = upload(ctx, ctx->bqin, in.data(), in.size() * sizeof(double)))) return rc;
    if ((rc = ensure(ctx, ctx->bqidx, (size_t)(Mc + 1) * sizeof(int32_t)))) return rc;
    if (cols) HIPCHK(ctx, hipMemcpyAsync(ctx->bqidx.p, cols, (size_t)Mc * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    if ((rc = ensure(ctx, ctx->bqout, (size_t)(Q + 1) * (size_t)Mc * sizeof(double)))) return rc;
    const double* din = (const double*)ctx->bqin.p;
    int32_t* didx = (int32_t*)ctx->bqidx.p;
    double* dq = (double*)ctx->bqout.p;
    g_last_kernel = "quantiles (sort over draws)";
    if ((rc = pioran_launch_quantiles(B, M, ldx, dX, dstatus, shift ? din + o_shift : nullptr, Mc, cols ? didx : nullptr, ref ? din + o_ref : nullptr,
                                      ref ? din + o_ref + Mc : nullptr, Q, din, dq, mean ? dq + Q * Mc : nullptr, kept ? didx + Mc : nullptr, ctx->stream))) {
        if (rc == PIORAN_ERR_HIP && ctx->last_err.empty()) ctx->last_err = "quantile launch failed";
        return rc;
    }
    if ((rc = download(ctx, quant, dq, (size_t)Q * (size_t)Mc * sizeof(double)))) return rc;
    if (mean && (rc = download(ctx, mean, dq + Q * Mc, (size_t)Mc * sizeof(double)))) return rc;
    if (kept && (rc = download(ctx, kept, didx + Mc, sizeof(int32_t)))) return rc;
    return PIORAN_OK;
}

// the resident draws [B][ld] and their status: refused with the out-of-memory code where they do not fit what the context may take
static int quantiles_resident(pioran_ctx* ctx, int64_t B, int64_t ld)
{
    const size_t bytes = (size_t)B * (size_t)ld * sizeof(double);
    if (!ws_fits(ctx, ctx->bqX, bytes)) { ctx->last_err = "the draws do not fit the context's workspace budget"; return PIORAN_ERR_ALLOC; }
    if (const int rc = ensure(ctx, ctx->bqX, bytes)) return rc;
    return ensure(ctx, ctx->bqst, (size_t)B * sizeof(int32_t));
}

int pioran_quantiles_batch(pioran_ctx* ctx, int64_t B, int64_t M, int64_t ldx, const double* X, const int32_t* status, const double* shift, int64_t Mc,
                           const int32_t* cols, const double* ref, const double* scale, int64_t Q, const double* probs, double* quant, double* mean,
                           int32_t* kept)
{
    if (const int rc = quantiles_refuse(ctx, B, M, ldx, X, Mc, cols, ref, scale, Q, probs, quant)) return rc;
    if (!cols) Mc = M;
    if (const int rc = quantiles_refuse_host(M, Mc, cols, scale)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    PendingGuard guard(ctx);
    int rc;
    if ((rc = quantiles_resident(ctx, B, ldx))) return rc;
    // (the last row is read up to column M only: the caller's array may end there)
    HIPCHK(ctx, hipMemcpyAsync(ctx->bqX.p, X, ((size_t)(B - 1) * (size_t)ldx + (size_t)M) * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    if (status) HIPCHK(ctx, hipMemcpyAsync(ctx->bqst.p, status, (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    if ((rc = quantiles_reduce(ctx, B, M, ldx, (const double*)ctx->bqX.p, status ? (const int32_t*)ctx->bqst.p : nullptr, shift, Mc, cols, ref, scale, Q,
                               probs, quant, mean, kept)))
        return rc;
    SYNC(ctx);
    return PIORAN_OK;
}

int pioran_celerite_rand_posterior_summary(pioran_ds* ds, int64_t B, int64_t J, const double* A, const double* Bc, const double* C, const double* Dd,
                                           int cd_shared, const double* mu, const double* nu, const double* shift, int64_t M, const double* tau,
                                           const double* q_data, const double* q_new, const double* eps, int backtransform, int64_t Q,
                                           const double* probs, double* ts_quant, double* ts_mean, int64_t Nres, const int32_t* res_cols,
                                           const double* res_ref, const double* res_scale, double* res_quant, double* res_mean, int32_t* status,
                                           int32_t* kept)
{
    // every bad argument first, then what is not supported; nothing here touches the GPU
    const int rdraw = rand_posterior_refuse(ds, B, J, A, Bc, C, Dd, cd_shared, M, tau, q_data, q_new, eps);
    if (rdraw == PIORAN_ERR_ARG) return rdraw;
    if (Nres < 0 || (backtransform && !shift)) return PIORAN_ERR_ARG;
    const bool with_res = Nres > 0;
    if (with_res && (!res_ref || !res_scale || !res_quant || (!res_cols && Nres != M))) return PIORAN_ERR_ARG;
    const int rquant = quantiles_refuse(ds, B, M, M, tau, Nres, with_res ? res_cols : nullptr, with_res ? res_ref : nullptr,
                                        with_res ? res_scale : nullptr, Q, probs, ts_quant);
    if (rquant == PIORAN_ERR_ARG) return rquant;
    if (with_res)
        if (const int rc = quantiles_refuse_host(M, Nres, res_cols, res_scale)) return rc;
    if (rdraw) return rdraw;
    if (rquant) return rquant;
    pioran_ctx* ctx = ds->ctx;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc;
    if ((rc = quantiles_resident(ctx, B, M))) return rc;   // before any draw is computed
    DrawSink sink;
    sink.dev_out = (double*)ctx->bqX.p;
    sink.dev_status = (int32_t*)ctx->bqst.p;
    if ((rc = rand_posterior_into(ds, B, J, A, Bc, C, Dd, cd_shared, mu, nu, shift, M, tau, q_data, q_new, eps, sink))) return rc;
    PendingGuard guard(ctx);
    const double* bt = backtransform ? shift : nullptr;
    if ((rc = quantiles_reduce(ctx, B, M, M, sink.dev_out, sink.dev_status, bt, M, nullptr, nullptr, nullptr, Q, probs, ts_quant, ts_mean, kept))) return rc;
    SYNC(ctx);   // bqin / bqidx / bqout are the second reduction's as well
    if (with_res) {
        if ((rc = quantiles_reduce(ctx, B, M, M, sink.dev_out, sink.dev_status, bt, Nres, res_cols, res_ref, res_scale, Q, probs, res_quant, res_mean, kept)))
            return rc;
    }
    if (status && (rc = download(ctx, status, sink.dev_status, (size_t)B * sizeof(int32_t)))) return rc;
    SYNC(ctx);
    return PIORAN_OK;
}

// ---- batched Lomb-Scargle periodogram (periodogram.hip) --------------------------------------------------------------------------
// The staged series of a draw chunk and the table of a frequency chunk are alive together, so each may take half of what the call may newly
// take (ws_allow): need() of both chunk sizers counts its bytes twice.
// The frequency chunk of a call, sized ONCE per call, and its workspace in blstab.  The free memory is asked for only when the table of all
// frequencies is not allocated already (the asynchronous entry must not block on the host).
static int ls_size_fchunk(pioran_ctx* ctx, int64_t N, int64_t F, int64_t& fchunk)
{
    auto need = [&](int64_t fc) { return 2 * pioran_ls_chunk_doubles(N, fc) * sizeof(double); };
    fchunk = std::min(F, pioran_ls_max_fchunk());
    if (need(fchunk) / 2 <= ctx->blstab.cap) return PIORAN_OK;
    int rc = size_chunk(ctx, fchunk, {&ctx->blstab}, need, [&](int64_t fc) { return ensure(ctx, ctx->blstab, need(fc) / 2); });
    if (rc) return rc;
    fchunk = std::min(F, pioran_ls_fpad(fchunk));   // the padded table of the chunk the budget admits holds this many
    return ensure(ctx, ctx->blstab, need(fchunk) / 2);
}

// blsaux = weights [N] | per-draw scalars [3][Bmax]; the weights are computed here, once per call
static int ls_weights(pioran_ctx* ctx, int64_t N, int64_t Bmax, const double* dyerr)
{
    if (int rc = ensure(ctx, ctx->blsaux, (size_t)(N + 3 * Bmax) * sizeof(double))) return rc;
    if (ctx->opt.ls_only && !(ctx->opt.ls_only & 1)) return PIORAN_OK;
    return pioran_launch_ls_weights(N, dyerr, (double*)ctx->blsaux.p, ctx->stream);
}

// B draws against all F frequencies in chunks of fchunk, on the weights and the workspace the two functions above left.  table_ready: blstab
// holds the table of every frequency already — meaningful only with fchunk == F, and only the caller that built it in this call may say so.
static int ls_run(pioran_ctx* ctx, int64_t N, int64_t B, int64_t F, int64_t fchunk, bool table_ready, const double* dt, const double* dY,
                  const double* dfreq, int fit_mean, int center_data, double* dpower, int32_t* dstatus)
{
    int rc;
    const int only = ctx->opt.ls_only ? ctx->opt.ls_only : 7;
    double* w = (double*)ctx->blsaux.p;
    double* dr = w + N;
    double* work = (double*)ctx->blstab.p;
    table_ready = table_ready && fchunk == F;
    g_last_kernel = "periodogram (fp64 matrix product)";
    if ((only & 2) && (rc = pioran_launch_ls_series(N, B, dY, w, fit_mean, center_data, dr, dstatus, ctx->stream))) return rc;
    for (int64_t f0 = 0; f0 < F; f0 += fchunk) {
        const int64_t fc = std::min(F - f0, fchunk);
        if ((only & 1) && !table_ready && (rc = pioran_launch_ls_table(N, fc, dt, w, dfreq + f0, fit_mean, work, ctx->stream))) return rc;
        if ((only & 4) && (rc = pioran_launch_ls_product(N, B, fc, dY, work, dr, dpower + f0, F, ctx->opt.ls_tile, ctx->stream))) return rc;
    }
    return PIORAN_OK;
}

int pioran_lombscargle_batch_dev(pioran_ctx* ctx, int64_t N, int64_t B, int64_t F, const double* dt, const double* dY, const double* dyerr,
                                 const double* dfreq, int fit_mean, int center_data, double* dpower, int32_t* dstatus)
{
    if (!ctx || !dt || !dY || !dfreq || !dpower || N < 3 || B < 1 || F < 1) return PIORAN_ERR_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc;
    int64_t fchunk;
    if ((rc = ls_size_fchunk(ctx, N, F, fchunk))) return rc;
    if ((rc = ls_weights(ctx, N, B, dyerr))) return rc;
    return ls_run(ctx, N, B, F, fchunk, false, dt, dY, dfreq, fit_mean, center_data, dpower, dstatus);
}

int pioran_lombscargle_batch(pioran_ctx* ctx, int64_t N, int64_t B, int64_t F, const double* t, const double* Y, const double* yerr,
                             const double* freq, int fit_mean, int center_data, double* power, int32_t* status)
{
    if (!ctx || !t || !Y || !freq || !power || N < 3 || B < 1 || F < 1) return PIORAN_ERR_ARG;
    for (int64_t n = 0; n < N; ++n)
        if (!std::isfinite(t[n]) || (yerr && !(std::isfinite(yerr[n]) && yerr[n] > 0.0))) return PIORAN_ERR_ARG;
    for (int64_t f = 0; f < F; ++f)
        if (!(std::isfinite(freq[f]) && freq[f] > 0.0)) return PIORAN_ERR_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    PendingGuard guard(ctx);
    int rc;
    if ((rc = upload(ctx, ctx->bA, t, N * sizeof(double)))) return rc;
    if (yerr && (rc = upload(ctx, ctx->bB, yerr, N * sizeof(double)))) return rc;
    if ((rc = upload(ctx, ctx->bC, freq, F * sizeof(double)))) return rc;
    const double *dt = (const double*)ctx->bA.p, *dyerr = yerr ? (const double*)ctx->bB.p : nullptr, *dfreq = (const double*)ctx->bC.p;
    int64_t chunk = B;
    rc = size_chunk(ctx, chunk, {&ctx->bY, &ctx->bS2}, [&](int64_t nb) { return 2 * (size_t)nb * (size_t)(N + F) * sizeof(double); },
                    [&](int64_t nb) {
                        return ensure_each(ctx, {{&ctx->bY, (size_t)nb * (size_t)N * sizeof(double)}, {&ctx->bS2, (size_t)nb * (size_t)F * sizeof(double)},
                                                 {&ctx->bst, (size_t)nb * sizeof(int32_t)}});
                    });
    if (rc) return rc;
    // the frequency chunk, its workspace and the weights: once, in front of the draw chunks — no buffer of theirs is touched inside the loop
    int64_t fchunk;
    if ((rc = ls_size_fchunk(ctx, N, F, fchunk))) return rc;
    if ((rc = ls_weights(ctx, N, chunk, dyerr))) return rc;
    for (int64_t b0 = 0; b0 < B; b0 += chunk) {
        const int64_t nb = std::min(B - b0, chunk);
        if ((rc = upload(ctx, ctx->bY, Y + b0 * N, (size_t)nb * N * sizeof(double)))) return rc;
        // with one frequency chunk the first draw chunk's table serves the others
        rc = ls_run(ctx, N, nb, F, fchunk, b0 > 0, dt, (const double*)ctx->bY.p, dfreq, fit_mean, center_data, (double*)ctx->bS2.p, (int32_t*)ctx->bst.p);
        if (rc) { if (rc == PIORAN_ERR_HIP && ctx->last_err.empty()) ctx->last_err = "periodogram launch failed"; return rc; }
        if ((rc = download(ctx, power + b0 * F, ctx->bS2.p, (size_t)nb * F * sizeof(double)))) return rc;
        if (status && (rc = download(ctx, status + b0, ctx->bst.p, nb * sizeof(int32_t)))) return rc;
        SYNC(ctx);   // the staging buffers are reused by the next chunk
    }
    return PIORAN_OK;
}

// ---- PSD model against its basis-function approximation (psd_check.hip) -----------------------------------------------------------------------
static const char* const kPsdCheckName = "psd check (model against approximation)";

struct PsdCheckCfg {
    int model, P, J, basis, integrated, normalise, times_f;
    double f_min, f_max, S_low, S_high;
};

// what every form can see without looking at an array
static int psd_check_refuse(const void* ctx, int64_t B, int model, int64_t J, int basis, double f_min, double f_max, double S_low, double S_high,
                            const void* theta, const void* norm, int64_t F, const void* freq, bool any_output)
{
    if (!ctx || !theta || !norm || !freq || !any_output || B < 1 || F < 1) return PIORAN_ERR_ARG;
    if (model < 0 || model > 1 || basis < 0 || basis > 1 || J < 2 || J > 256) return PIORAN_ERR_ARG;
    for (const double v : {f_min, f_max, S_low, S_high})
        if (!(std::isfinite(v) && v > 0.0)) return PIORAN_ERR_ARG;
    return f_min < f_max ? PIORAN_OK : PIORAN_ERR_ARG;
}

// ... and what only a host array shows
static int psd_check_refuse_freq(int64_t F, const double* freq)
{
    for (int64_t f = 0; f < F; ++f)
        if (!(std::isfinite(freq[f]) && freq[f] > 0.0)) return PIORAN_ERR_ARG;
    return PIORAN_OK;
}

static PsdCheckCfg psd_check_cfg(int model, int64_t J, int basis, int integrated, double f_min, double f_max, double S_low, double S_high, int normalise,
                                 int times_f)
{
    return {model, model == 0 ? 3 : 5, (int)J, basis, integrated != 0, normalise != 0, times_f != 0, f_min, f_max, S_low, S_high};
}

// The grid of the approximation on the device, as pioran_logpdf_batch_theta prepares it: sp [J] | LU [J][J] | piv [J] in bpcgrid
struct PsdCheckGrid { const double *sp, *LU; const int32_t* piv; };
static int psd_check_grid(pioran_ctx* ctx, const PsdCheckCfg& c, PsdCheckGrid& g)
{
    const size_t nJ = (size_t)c.J, n = nJ + nJ * nJ + (nJ + 1) / 2;
    const double key[6] = {(double)c.J, (double)c.basis, c.f_min, c.f_max, c.S_low, c.S_high};
    double* dev = (double*)ctx->bpcgrid.p;
    // the grid of the previous call is still there (a sampler's repeated calls: nothing to do, and the device form stays asynchronous)
    if (dev && ctx->pcgrid_host.size() == n && !std::memcmp(key, ctx->pcgrid_key, sizeof(key))) {
        g.sp = dev; g.LU = dev + nJ; g.piv = (const int32_t*)(dev + nJ + nJ * nJ);
        return PIORAN_OK;
    }
    std::vector<double> sp, LU, cc, dd;
    std::vector<int32_t> piv, real;
    int rc = pioran_approx_setup_host(c.J, c.basis, c.f_min, c.f_max, c.S_low, c.S_high, sp, LU, piv, cc, dd, real);
    if (rc) return rc;
    // an earlier call's kernels may still read the old grid, or its copy out of the host image may not have run: wait before either is rewritten
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    ctx->pcgrid_host.clear();
    if ((rc = ensure(ctx, ctx->bpcgrid, n * sizeof(double)))) return rc;
    std::memcpy(ctx->pcgrid_key, key, sizeof(key));
    ctx->pcgrid_host.assign(n, 0.0);
    std::memcpy(ctx->pcgrid_host.data(), sp.data(), nJ * sizeof(double));
    std::memcpy(ctx->pcgrid_host.data() + nJ, LU.data(), nJ * nJ * sizeof(double));
    std::memcpy(ctx->pcgrid_host.data() + nJ + nJ * nJ, piv.data(), nJ * sizeof(int32_t));
    dev = (double*)ctx->bpcgrid.p;
    if ((rc = upload_to(ctx, dev, ctx->pcgrid_host.data(), n * sizeof(double)))) return rc;
    g.sp = dev; g.LU = dev + nJ; g.piv = (const int32_t*)(dev + nJ + nJ * nJ);
    return PIORAN_OK;
}

// a chunk's amp [nb][J] | integ [nb] | pf0 [nb] | status [nb] in bpcdraw
struct PsdCheckDraws { double *amp, *integ, *pf0; int32_t* status; };
static size_t psd_check_draw_bytes(int64_t nb, int J) { return (size_t)nb * ((size_t)J + 2) * sizeof(double) + (size_t)nb * sizeof(int32_t); }
static PsdCheckDraws psd_check_draws_of(pioran_ctx* ctx, int64_t nb, int J)
{
    double* a = (double*)ctx->bpcdraw.p;
    return {a, a + (size_t)nb * J, a + (size_t)nb * J + nb, (int32_t*)(a + (size_t)nb * J + 2 * nb)};
}

// nb draws on the device through the two kernels: `dr` receives the per-draw results, `e` names the arrays that are wanted (its inputs are filled here)
static int psd_check_chunk(pioran_ctx* ctx, const PsdCheckCfg& c, const PsdCheckGrid& g, int64_t nb, const double* dtheta, const double* dnorm, int64_t F,
                           const double* dfreq, const PsdCheckDraws& dr, PsdCheckEval e, bool timed)
{
    auto mark = [&](int slot) { return timed ? hipEventRecord(ctx->ev[slot], ctx->stream) : hipSuccess; };
    int rc;
    g_last_kernel = kPsdCheckName;
    HIPCHK(ctx, mark(4));
    if ((rc = pioran_launch_psd_check_draws(nb, c.model, c.P, c.J, c.basis, c.integrated, c.normalise, c.f_min, c.f_max, g.sp, g.LU, g.piv, dtheta, dnorm,
                                            dfreq, dr.amp, dr.integ, dr.pf0, dr.status, ctx->stream)))
        return rc;
    HIPCHK(ctx, mark(5));
    if (e.psd || e.approx || e.res || e.rat || e.resT || e.ratT || e.part) {
        e.B = nb; e.F = F; e.model = c.model; e.P = c.P; e.J = c.J; e.basis = c.basis; e.normalise = c.normalise; e.times_f = c.times_f;
        e.sp = g.sp; e.theta = dtheta; e.norm = dnorm; e.freq = dfreq; e.amp = dr.amp; e.integ = dr.integ; e.pf0 = dr.pf0; e.status = dr.status;
        if ((rc = pioran_launch_psd_check_eval(e, ctx->stream))) return rc;
    }
    HIPCHK(ctx, mark(6));
    return PIORAN_OK;
}

int pioran_psd_check_batch_dev(pioran_ctx* ctx, int64_t B, int model, int64_t n_components, int basis, int is_integrated_power, double f_min, double f_max,
                               double S_low, double S_high, const double* dtheta, const double* dnorm, int64_t F, const double* dfreq, int normalise,
                               int times_f, double* dpsd, double* dpsd_approx, double* dresiduals, double* dratios, double* damplitudes, double* dinteg,
                               int32_t* dstatus)
{
    const bool any = dpsd || dpsd_approx || dresiduals || dratios || damplitudes || dinteg || dstatus;
    if (const int rc = psd_check_refuse(ctx, B, model, n_components, basis, f_min, f_max, S_low, S_high, dtheta, dnorm, F, dfreq, any)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const PsdCheckCfg c = psd_check_cfg(model, n_components, basis, is_integrated_power, f_min, f_max, S_low, S_high, normalise, times_f);
    PsdCheckGrid g;
    int rc;
    if ((rc = psd_check_grid(ctx, c, g))) return rc;
    if ((rc = ensure(ctx, ctx->bpcdraw, psd_check_draw_bytes(B, c.J)))) return rc;
    PsdCheckDraws dr = psd_check_draws_of(ctx, B, c.J);
    if (damplitudes) dr.amp = damplitudes;
    if (dinteg) dr.integ = dinteg;
    if (dstatus) dr.status = dstatus;
    PsdCheckEval e{};
    e.psd = dpsd; e.approx = dpsd_approx; e.res = dresiduals; e.rat = dratios;
    return psd_check_chunk(ctx, c, g, B, dtheta, dnorm, F, dfreq, dr, e, ctx->opt.pc_events != 0);
}

// theta [B][P] | norm [B] | freq [F] of a host form into bpcin
static int psd_check_upload(pioran_ctx* ctx, const PsdCheckCfg& c, int64_t B, const double* theta, const double* norm, int64_t F, const double* freq,
                            const double*& dtheta, const double*& dnorm, const double*& dfreq)
{
    const size_t nth = (size_t)B * c.P;
    int rc;
    if ((rc = ensure(ctx, ctx->bpcin, (nth + (size_t)B + (size_t)F) * sizeof(double)))) return rc;
    double* dev = (double*)ctx->bpcin.p;
    if ((rc = upload_to(ctx, dev, theta, nth * sizeof(double)))) return rc;
    if ((rc = upload_to(ctx, dev + nth, norm, (size_t)B * sizeof(double)))) return rc;
    if ((rc = upload_to(ctx, dev + nth + B, freq, (size_t)F * sizeof(double)))) return rc;
    dtheta = dev; dnorm = dev + nth; dfreq = dev + nth + B;
    return PIORAN_OK;
}

int pioran_psd_check_batch(pioran_ctx* ctx, int64_t B, int model, int64_t n_components, int basis, int is_integrated_power, double f_min, double f_max,
                           double S_low, double S_high, const double* theta, const double* norm, int64_t F, const double* freq, int normalise, int times_f,
                           double* psd, double* psd_approx, double* residuals, double* ratios, double* amplitudes, double* integ, int32_t* status)
{
    const bool any = psd || psd_approx || residuals || ratios || amplitudes || integ || status;
    if (const int rc = psd_check_refuse(ctx, B, model, n_components, basis, f_min, f_max, S_low, S_high, theta, norm, F, freq, any)) return rc;
    if (const int rc = psd_check_refuse_freq(F, freq)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    PendingGuard guard(ctx);
    const PsdCheckCfg c = psd_check_cfg(model, n_components, basis, is_integrated_power, f_min, f_max, S_low, S_high, normalise, times_f);
    PsdCheckGrid g;
    int rc;
    if ((rc = psd_check_grid(ctx, c, g))) return rc;
    const double *dtheta, *dnorm, *dfreq;
    if ((rc = psd_check_upload(ctx, c, B, theta, norm, F, freq, dtheta, dnorm, dfreq))) return rc;
    double* const host[4] = {psd, psd_approx, residuals, ratios};
    size_t narr = 0;
    for (double* h : host) narr += h != nullptr;
    // the arrays of a chunk of draws, chunk by chunk under the workspace budget, as the periodogram's host form goes
    auto out_bytes = [&](int64_t nb) { return (size_t)nb * (size_t)F * narr * sizeof(double) + 8; };
    int64_t chunk = B;
    rc = size_chunk(ctx, chunk, {&ctx->bpcout, &ctx->bpcdraw}, [&](int64_t nb) { return out_bytes(nb) + psd_check_draw_bytes(nb, c.J); },
                    [&](int64_t nb) { return ensure_each(ctx, {{&ctx->bpcout, out_bytes(nb)}, {&ctx->bpcdraw, psd_check_draw_bytes(nb, c.J)}}); });
    if (rc) return rc;
    const bool timed = ctx->opt.pc_events != 0;
    for (int64_t b0 = 0; b0 < B; b0 += chunk) {
        const int64_t nb = std::min(B - b0, chunk);
        const PsdCheckDraws dr = psd_check_draws_of(ctx, nb, c.J);
        double* dev[4] = {nullptr, nullptr, nullptr, nullptr};
        double* next = (double*)ctx->bpcout.p;
        for (int a = 0; a < 4; ++a)
            if (host[a]) { dev[a] = next; next += (size_t)nb * (size_t)F; }
        PsdCheckEval e{};
        e.psd = dev[0]; e.approx = dev[1]; e.res = dev[2]; e.rat = dev[3];
        rc = psd_check_chunk(ctx, c, g, nb, dtheta + b0 * c.P, dnorm + b0, F, dfreq, dr, e, timed && b0 == 0);
        if (rc) { if (rc == PIORAN_ERR_HIP && ctx->last_err.empty()) ctx->last_err = "psd check launch failed"; return rc; }
        for (int a = 0; a < 4; ++a)
            if (host[a] && (rc = download(ctx, host[a] + b0 * F, dev[a], (size_t)nb * (size_t)F * sizeof(double)))) return rc;
        if (amplitudes && (rc = download(ctx, amplitudes + b0 * c.J, dr.amp, (size_t)nb * c.J * sizeof(double)))) return rc;
        if (integ && (rc = download(ctx, integ + b0, dr.integ, (size_t)nb * sizeof(double)))) return rc;
        if (status && (rc = download(ctx, status + b0, dr.status, (size_t)nb * sizeof(int32_t)))) return rc;
        SYNC(ctx);   // the chunk's buffers are reused by the next
    }
    return PIORAN_OK;
}

int pioran_psd_check_summary(pioran_ctx* ctx, int64_t B, int model, int64_t n_components, int basis, int is_integrated_power, double f_min, double f_max,
                             double S_low, double S_high, const double* theta, const double* norm, int64_t F, const double* freq, int normalise,
                             int times_f, int64_t Q, const double* probs, double* quant, double* mean, double* meta, int32_t* status, int32_t* kept)
{
    // every bad argument first, then what is not supported; nothing here touches the GPU
    if (const int rc = psd_check_refuse(ctx, B, model, n_components, basis, f_min, f_max, S_low, S_high, theta, norm, F, freq, quant != nullptr)) return rc;
    if (const int rc = psd_check_refuse_freq(F, freq)) return rc;
    if (!probs || Q < 1) return PIORAN_ERR_ARG;
    for (int64_t q = 0; q < Q; ++q)
        if (!(probs[q] >= 0.0 && probs[q] <= 1.0)) return PIORAN_ERR_ARG;   // NaN included
    // the draws of a frequency, and for meta the frequencies of a draw, are sorted inside one workgroup's LDS
    if (B > pioran_quantiles_max_draws() || F > pioran_quantiles_max_draws()) return PIORAN_ERR_UNSUPPORTED;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    PendingGuard guard(ctx);
    const PsdCheckCfg c = psd_check_cfg(model, n_components, basis, is_integrated_power, f_min, f_max, S_low, S_high, normalise, times_f);
    const size_t bf = (size_t)B * (size_t)F, npart = (size_t)pioran_psd_check_ftiles(F);
    const size_t x_bytes = 4 * bf * sizeof(double), t_bytes = meta ? (2 * bf + (size_t)B * npart * 4) * sizeof(double) : 0;
    if (!ws_fits(ctx, ctx->bpcout, x_bytes) || !ws_fits(ctx, ctx->bpcT, t_bytes)) {
        ctx->last_err = "the arrays do not fit the context's workspace budget";
        return PIORAN_ERR_ALLOC;
    }
    // bpcq = probs [Q] | 0.5 | quant [4][Q][F] | mean [4][F] | medians [2][B] | means [2][B] | meta [B][8] | kept
    const size_t o_quant = (size_t)Q + 1, o_mean = o_quant + 4 * (size_t)Q * F, o_med = o_mean + 4 * (size_t)F, o_mm = o_med + 2 * (size_t)B,
                 o_meta = o_mm + 2 * (size_t)B, o_kept = o_meta + 8 * (size_t)B;
    PsdCheckGrid g;
    int rc;
    if ((rc = psd_check_grid(ctx, c, g))) return rc;
    const double *dtheta, *dnorm, *dfreq;
    if ((rc = psd_check_upload(ctx, c, B, theta, norm, F, freq, dtheta, dnorm, dfreq))) return rc;
    if ((rc = ensure_each(ctx, {{&ctx->bpcout, x_bytes}, {&ctx->bpcT, t_bytes}, {&ctx->bpcdraw, psd_check_draw_bytes(B, c.J)},
                                {&ctx->bpcq, (o_kept + 1) * sizeof(double)}})))
        return rc;
    std::vector<double> small(probs, probs + Q);
    small.push_back(0.5);
    double* dq = (double*)ctx->bpcq.p;
    if ((rc = upload_to(ctx, dq, small.data(), small.size() * sizeof(double)))) return rc;
    const PsdCheckDraws dr = psd_check_draws_of(ctx, B, c.J);
    double* X = (double*)ctx->bpcout.p;
    double* T = (double*)ctx->bpcT.p;
    PsdCheckEval e{};
    e.psd = X; e.approx = X + bf; e.res = X + 2 * bf; e.rat = X + 3 * bf;
    if (meta) { e.resT = T; e.ratT = T + bf; e.ldT = B; e.part = T + 2 * bf; e.npart = (int64_t)npart; }
    if ((rc = psd_check_chunk(ctx, c, g, B, dtheta, dnorm, F, dfreq, dr, e, ctx->opt.pc_events != 0))) {
        if (rc == PIORAN_ERR_HIP && ctx->last_err.empty()) ctx->last_err = "psd check launch failed";
        return rc;
    }
    // per frequency, over the draws with status 0: the reduction of pioran_quantiles_batch_dev on each [B][F] array
    int32_t* dkept = (int32_t*)(dq + o_kept);
    for (int a = 0; a < 4; ++a)
        if ((rc = pioran_launch_quantiles(B, F, F, X + a * bf, dr.status, nullptr, F, nullptr, nullptr, nullptr, Q, dq, dq + o_quant + (size_t)a * Q * F,
                                          mean ? dq + o_mean + (size_t)a * F : nullptr, a == 0 ? dkept : nullptr, ctx->stream)))
            return rc;
    // per draw, over the frequencies: mean and median of the rows of the transposed copies (rows there are frequencies, all kept)
    if (meta) {
        for (int k = 0; k < 2; ++k)
            if ((rc = pioran_launch_quantiles(F, B, B, T + k * bf, nullptr, nullptr, B, nullptr, nullptr, nullptr, 1, dq + Q, dq + o_med + (size_t)k * B,
                                              dq + o_mm + (size_t)k * B, nullptr, ctx->stream)))
                return rc;
        if ((rc = pioran_launch_psd_check_meta(B, (int64_t)npart, e.part, dr.status, dq + o_med, dq + o_mm, dq + o_med + B, dq + o_mm + B, dq + o_meta,
                                               ctx->stream)))
            return rc;
        if ((rc = download(ctx, meta, dq + o_meta, 8 * (size_t)B * sizeof(double)))) return rc;
    }
    if ((rc = download(ctx, quant, dq + o_quant, 4 * (size_t)Q * F * sizeof(double)))) return rc;
    if (mean && (rc = download(ctx, mean, dq + o_mean, 4 * (size_t)F * sizeof(double)))) return rc;
    if (status && (rc = download(ctx, status, dr.status, (size_t)B * sizeof(int32_t)))) return rc;
    if (kept && (rc = download(ctx, kept, dkept, sizeof(int32_t)))) return rc;
    SYNC(ctx);
    return PIORAN_OK;
}

// ---- CARMA(p, q) models from their sampled parameters (carma.hip) ---------------------------------------------------------------------------
static const char* const kCarmaCoefsName = "carma (sampled parameters to coefficients)";
static const char* const kCarmaVjpName = "carma (reverse mode of the coefficients)";
static const char* const kCarmaPsdName = "carma (power spectral density)";

// The batch's inputs on the device (bcarma): in1 [B][n1] | in2 [B][n2] | norm [B] | flags [B] (int32) — form 0: qa, qb (n1 = p, n2 = q), form 1: roots,
// beta (n1 = 2 p, n2 = q + 1)
struct CarmaDraws {
    int p = 0, q = 0, J = 0, form = 0, integrated = 0, n1 = 0, n2 = 0;
    double f_lo = 0.0, f_hi = 0.0;
    const double *in1 = nullptr, *in2 = nullptr, *norm = nullptr;
    int32_t* flags = nullptr;
};

// what every CARMA entry can see without looking at an array: NULL or inconsistent arguments first, then the orders
static int carma_refuse(const void* handle, int64_t B, int p, int q, int form, const void* in1, const void* in2, const void* norm, double f_lo, double f_hi)
{
    if (!handle || B < 1 || !in1 || !norm || form < 0 || form > 1) return PIORAN_ERR_ARG;
    if (!std::isfinite(f_lo) || !std::isfinite(f_hi) || f_lo < 0.0 || f_hi < f_lo || (f_hi > 0.0 && !(f_lo < f_hi))) return PIORAN_ERR_ARG;
    if (p < 1 || p > pioran_carma_max_order() || q < 0 || q > p) return PIORAN_ERR_UNSUPPORTED;
    if (!in2 && !(form == 0 && q == 0)) return PIORAN_ERR_ARG;
    return PIORAN_OK;
}

static int stage_carma(pioran_ctx* ctx, int64_t B, int p, int q, int form, const double* in1, const double* in2, const double* norm, int integrated,
                       double f_lo, double f_hi, CarmaDraws& cd)
{
    cd.p = p; cd.q = q; cd.J = (p + 1) / 2; cd.form = form; cd.integrated = integrated != 0; cd.f_lo = f_lo; cd.f_hi = f_hi;
    cd.n1 = form == 0 ? p : 2 * p; cd.n2 = form == 0 ? q : q + 1;
    const size_t b1 = (size_t)B * cd.n1, b2 = (size_t)B * cd.n2;
    int rc;
    if ((rc = ensure(ctx, ctx->bcarma, (b1 + b2 + (size_t)B + ((size_t)B + 1) / 2) * sizeof(double)))) return rc;
    double* dev = (double*)ctx->bcarma.p;
    if ((rc = upload_to(ctx, dev, in1, b1 * sizeof(double)))) return rc;
    if (b2 && (rc = upload_to(ctx, dev + b1, in2, b2 * sizeof(double)))) return rc;
    if ((rc = upload_to(ctx, dev + b1 + b2, norm, (size_t)B * sizeof(double)))) return rc;
    cd.in1 = dev; cd.in2 = b2 ? dev + b1 : nullptr; cd.norm = dev + b1 + b2; cd.flags = (int32_t*)(dev + b1 + b2 + B);
    return PIORAN_OK;
}

// carma_coefs_kernel on the staged batch: (a, b, c, d) [B][J] into bA .. bD, where the value and gradient bodies read a batch's coefficients
static int carma_coefs_to_draws(pioran_ctx* ctx, int64_t B, const CarmaDraws& cd, bool timed)
{
    int rc;
    const size_t bj = (size_t)B * (size_t)cd.J * sizeof(double);
    if ((rc = ensure_each(ctx, {{&ctx->bA, bj}, {&ctx->bB, bj}, {&ctx->bC, bj}, {&ctx->bD, bj}}))) return rc;
    return timed_launch(ctx, kCarmaCoefsName, 4, timed, "carma coefficient launch failed", [&] {
        return pioran_launch_carma_coefs(B, cd.p, cd.q, cd.form, cd.in1, cd.in2, cd.norm, cd.integrated, cd.f_lo, cd.f_hi, (double*)ctx->bA.p,
                                         (double*)ctx->bB.p, (double*)ctx->bC.p, (double*)ctx->bD.p, cd.flags, ctx->stream);
    });
}

int pioran_carma_coefs_batch(pioran_ctx* ctx, int64_t B, int p, int q, int form, const double* qa_or_roots, const double* qb_or_beta, const double* norm,
                             int is_integrated_power, double f_lo, double f_hi, double* A, double* Bc, double* C, double* Dd, int32_t* flags)
{
    if (const int rc = carma_refuse(ctx, B, p, q, form, qa_or_roots, qb_or_beta, norm, f_lo, f_hi)) return rc;
    if (!A || !Bc || !C || !Dd) return PIORAN_ERR_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    PendingGuard guard(ctx);
    CarmaDraws cd;
    int rc;
    if ((rc = stage_carma(ctx, B, p, q, form, qa_or_roots, qb_or_beta, norm, is_integrated_power, f_lo, f_hi, cd))) return rc;
    if ((rc = carma_coefs_to_draws(ctx, B, cd, ctx->opt.carma_events != 0))) return rc;
    const size_t bj = (size_t)B * (size_t)cd.J * sizeof(double);
    if ((rc = download(ctx, A, ctx->bA.p, bj))) return rc;
    if ((rc = download(ctx, Bc, ctx->bB.p, bj))) return rc;
    if ((rc = download(ctx, C, ctx->bC.p, bj))) return rc;
    if ((rc = download(ctx, Dd, ctx->bD.p, bj))) return rc;
    if (flags && (rc = download(ctx, flags, cd.flags, (size_t)B * sizeof(int32_t)))) return rc;
    SYNC(ctx);
    return PIORAN_OK;
}

// (ga, gb, gc, gd) [B][J] of the caller through carma_vjp_kernel on the staged batch (quad form) to the caller's grad_qa [B][p], grad_qb [B][q] (may be
// NULL for q = 0), grad_norm [B]
static int carma_vjp_from_host(pioran_ctx* ctx, int64_t B, const CarmaDraws& cd, const double* ga, const double* gb, const double* gc, const double* gd,
                               double* grad_qa, double* grad_qb, double* grad_norm, bool timed)
{
    int rc;
    const size_t bj = (size_t)B * (size_t)cd.J, np = (size_t)B * cd.p, nq = (size_t)B * cd.q;
    double* dg;
    if ((rc = upload_cotangents(ctx, {ga, gb, gc, gd}, bj, dg))) return rc;
    if ((rc = ensure(ctx, ctx->bcarmaout, (np + nq + (size_t)B) * sizeof(double)))) return rc;
    double* dqa = (double*)ctx->bcarmaout.p;
    if ((rc = timed_launch(ctx, kCarmaVjpName, 4, timed, "carma reverse-mode launch failed", [&] {
            return pioran_launch_carma_vjp(B, cd.p, cd.q, cd.in1, cd.in2, cd.norm, cd.integrated, cd.f_lo, cd.f_hi, dg, dg + bj, dg + 2 * bj, dg + 3 * bj, dqa,
                                           dqa + np, dqa + np + nq, ctx->stream);
        })))
        return rc;
    if ((rc = download(ctx, grad_qa, dqa, np * sizeof(double)))) return rc;
    if (nq && grad_qb && (rc = download(ctx, grad_qb, dqa + np, nq * sizeof(double)))) return rc;
    return download(ctx, grad_norm, dqa + np + nq, (size_t)B * sizeof(double));
}

int pioran_carma_vjp_batch(pioran_ctx* ctx, int64_t B, int p, int q, const double* qa, const double* qb, const double* norm, int is_integrated_power,
                           const double* ga, const double* gb, const double* gc, const double* gd, double* grad_qa, double* grad_qb, double* grad_norm)
{
    if (const int rc = carma_refuse(ctx, B, p, q, 0, qa, qb, norm, 0.0, 0.0)) return rc;
    if (!ga || !gb || !gc || !gd || !grad_qa || !grad_norm || (q > 0 && !grad_qb)) return PIORAN_ERR_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    PendingGuard guard(ctx);
    CarmaDraws cd;
    int rc;
    if ((rc = stage_carma(ctx, B, p, q, 0, qa, qb, norm, is_integrated_power, 0.0, 0.0, cd))) return rc;
    if ((rc = carma_vjp_from_host(ctx, B, cd, ga, gb, gc, gd, grad_qa, grad_qb, grad_norm, ctx->opt.carma_events != 0))) return rc;
    SYNC(ctx);
    return PIORAN_OK;
}

// the frequencies of a PSD call onto the device, behind the per-draw workspace in bcarmaout: roots [B][p][2] | beta [B][q + 1] | factor [B] | freq [F] |
// status [B] (int32)
struct CarmaPsdWork { double *roots, *betas, *scale, *freq; int32_t* status; };
static int carma_psd_stage(pioran_ctx* ctx, int64_t B, const CarmaDraws& cd, int64_t F, const double* freq, CarmaPsdWork& w)
{
    const size_t nr = (size_t)B * 2 * cd.p, nb = (size_t)B * (cd.q + 1);
    int rc;
    if ((rc = ensure(ctx, ctx->bcarmaout, (nr + nb + (size_t)B + (size_t)F + ((size_t)B + 1) / 2) * sizeof(double)))) return rc;
    double* dev = (double*)ctx->bcarmaout.p;
    w = {dev, dev + nr, dev + nr + nb, dev + nr + nb + B, (int32_t*)(dev + nr + nb + B + F)};
    return upload_to(ctx, w.freq, freq, (size_t)F * sizeof(double));
}

static int carma_psd_refuse(int64_t F, const double* freq, const void* any_output)
{
    if (!freq || !any_output || F < 1) return PIORAN_ERR_ARG;
    for (int64_t f = 0; f < F; ++f)
        if (!(std::isfinite(freq[f]) && freq[f] > 0.0)) return PIORAN_ERR_ARG;
    return PIORAN_OK;
}

// draws [b0, b0 + nb) of the staged batch through the two PSD kernels into psd [nb][F]
static int carma_psd_chunk(pioran_ctx* ctx, const CarmaDraws& cd, const CarmaPsdWork& w, int64_t b0, int64_t nb, int64_t F, int times_f, double* psd, bool timed)
{
    return timed_launch(ctx, kCarmaPsdName, 4, timed, "carma psd launch failed", [&] {
        return pioran_launch_carma_psd(nb, cd.p, cd.q, cd.form, cd.in1 + b0 * cd.n1, at(cd.in2, b0 * cd.n2), cd.norm + b0, cd.integrated, cd.f_lo, cd.f_hi, F,
                                       w.freq, times_f != 0, w.roots + b0 * 2 * cd.p, w.betas + b0 * (cd.q + 1), w.scale + b0, psd, w.status + b0, ctx->stream);
    });
}

int pioran_carma_psd_batch(pioran_ctx* ctx, int64_t B, int p, int q, int form, const double* qa_or_roots, const double* qb_or_beta, const double* norm,
                           int is_integrated_power, double f_lo, double f_hi, int64_t F, const double* freq, int times_f, double* psd, int32_t* status)
{
    if (const int rc = carma_refuse(ctx, B, p, q, form, qa_or_roots, qb_or_beta, norm, f_lo, f_hi)) return rc;
    if (const int rc = carma_psd_refuse(F, freq, psd)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    PendingGuard guard(ctx);
    CarmaDraws cd;
    CarmaPsdWork w;
    int rc;
    if ((rc = stage_carma(ctx, B, p, q, form, qa_or_roots, qb_or_beta, norm, is_integrated_power, f_lo, f_hi, cd))) return rc;
    if ((rc = carma_psd_stage(ctx, B, cd, F, freq, w))) return rc;
    // the array of a chunk of draws, chunk by chunk under the workspace budget, as the PSD check's host form goes
    auto out_bytes = [&](int64_t nb) { return (size_t)nb * (size_t)F * sizeof(double); };
    int64_t chunk = B;
    if ((rc = size_chunk(ctx, chunk, {&ctx->bpcout}, out_bytes, [&](int64_t nb) { return ensure(ctx, ctx->bpcout, out_bytes(nb)); }))) return rc;
    for (int64_t b0 = 0; b0 < B; b0 += chunk) {
        const int64_t nb = std::min(B - b0, chunk);
        if ((rc = carma_psd_chunk(ctx, cd, w, b0, nb, F, times_f, (double*)ctx->bpcout.p, ctx->opt.carma_events != 0 && b0 == 0))) return rc;
        if ((rc = download(ctx, psd + b0 * F, ctx->bpcout.p, out_bytes(nb)))) return rc;
        if (status && (rc = download(ctx, status + b0, w.status + b0, (size_t)nb * sizeof(int32_t)))) return rc;
        SYNC(ctx);   // the chunk's buffer is reused by the next
    }
    return PIORAN_OK;
}

int pioran_carma_psd_summary(pioran_ctx* ctx, int64_t B, int p, int q, int form, const double* qa_or_roots, const double* qb_or_beta, const double* norm,
                             int is_integrated_power, double f_lo, double f_hi, int64_t F, const double* freq, int times_f, int64_t Q, const double* probs,
                             double* quant, int32_t* status, int32_t* kept)
{
    if (const int rc = carma_refuse(ctx, B, p, q, form, qa_or_roots, qb_or_beta, norm, f_lo, f_hi)) return rc;
    if (const int rc = carma_psd_refuse(F, freq, quant)) return rc;
    if (!probs || Q < 1) return PIORAN_ERR_ARG;
    for (int64_t k = 0; k < Q; ++k)
        if (!(probs[k] >= 0.0 && probs[k] <= 1.0)) return PIORAN_ERR_ARG;   // NaN included
    if (B > pioran_quantiles_max_draws()) return PIORAN_ERR_UNSUPPORTED;    // the draws of a frequency are sorted inside one workgroup's LDS
    HIPCHK(ctx, hipSetDevice(ctx->device));
    PendingGuard guard(ctx);
    const size_t x_bytes = (size_t)B * (size_t)F * sizeof(double);
    if (!ws_fits(ctx, ctx->bpcout, x_bytes)) { ctx->last_err = "the array does not fit the context's workspace budget"; return PIORAN_ERR_ALLOC; }
    CarmaDraws cd;
    CarmaPsdWork w;
    int rc;
    if ((rc = stage_carma(ctx, B, p, q, form, qa_or_roots, qb_or_beta, norm, is_integrated_power, f_lo, f_hi, cd))) return rc;
    if ((rc = carma_psd_stage(ctx, B, cd, F, freq, w))) return rc;
    // bpcq = probs [Q] | quant [Q][F] | kept
    const size_t o_quant = (size_t)Q, o_kept = o_quant + (size_t)Q * F;
    if ((rc = ensure_each(ctx, {{&ctx->bpcout, x_bytes}, {&ctx->bpcq, (o_kept + 1) * sizeof(double)}}))) return rc;
    double* dq = (double*)ctx->bpcq.p;
    if ((rc = upload_to(ctx, dq, probs, (size_t)Q * sizeof(double)))) return rc;
    if ((rc = carma_psd_chunk(ctx, cd, w, 0, B, F, times_f, (double*)ctx->bpcout.p, ctx->opt.carma_events != 0))) return rc;
    // per frequency, over the draws with status 0: the reduction of pioran_quantiles_batch_dev on the [B][F] array
    int32_t* dkept = (int32_t*)(dq + o_kept);
    if ((rc = pioran_launch_quantiles(B, F, F, (const double*)ctx->bpcout.p, w.status, nullptr, F, nullptr, nullptr, nullptr, Q, dq, dq + o_quant, nullptr, dkept,
                                      ctx->stream)))
        return rc;
    if ((rc = download(ctx, quant, dq + o_quant, (size_t)Q * F * sizeof(double)))) return rc;
    if (status && (rc = download(ctx, status, w.status, (size_t)B * sizeof(int32_t)))) return rc;
    if (kept && (rc = download(ctx, kept, dkept, sizeof(int32_t)))) return rc;
    SYNC(ctx);
    return PIORAN_OK;
}

// The coefficients of the staged batch made on the device (bA .. bD), and what the host needs of them to route the call as the host-pointer entries
// route per-draw (c, d): the flags and (b, c, d) — with `a` too for the callers that go on from host arrays
static int carma_coefs_fetch(pioran_ctx* ctx, int64_t B, const CarmaDraws& cd, std::vector<double>* hA, std::vector<double>& hB, std::vector<double>& hC,
                             std::vector<double>& hD, std::vector<int32_t>& hflags)
{
    int rc;
    if ((rc = carma_coefs_to_draws(ctx, B, cd, false))) return rc;
    const size_t bj = (size_t)B * (size_t)cd.J;
    hB.resize(bj); hC.resize(bj); hD.resize(bj); hflags.resize((size_t)B);
    if (hA) { hA->resize(bj); if ((rc = download(ctx, hA->data(), ctx->bA.p, bj * sizeof(double)))) return rc; }
    if ((rc = download(ctx, hB.data(), ctx->bB.p, bj * sizeof(double)))) return rc;
    if ((rc = download(ctx, hC.data(), ctx->bC.p, bj * sizeof(double)))) return rc;
    if ((rc = download(ctx, hD.data(), ctx->bD.p, bj * sizeof(double)))) return rc;
    if ((rc = download(ctx, hflags.data(), cd.flags, (size_t)B * sizeof(int32_t)))) return rc;
    SYNC(ctx);
    return PIORAN_OK;
}

int pioran_logpdf_batch_carma(pioran_ds* ds, int64_t B, int p, int q, const double* qa, const double* qb, const double* norm, int is_integrated_power,
                              double f_lo, double f_hi, const double* mu, const double* nu, const double* shift, double* out, int32_t* status,
                              double* A_out, double* Bc_out, double* C_out, double* Dd_out)
{
    if (const int rc = carma_refuse(ds, B, p, q, 0, qa, qb, norm, f_lo, f_hi)) return rc;
    if (!out) return PIORAN_ERR_ARG;
    pioran_ctx* ctx = ds->ctx;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    PendingGuard guard(ctx);
    CarmaDraws cd;
    int rc;
    if ((rc = stage_carma(ctx, B, p, q, 0, qa, qb, norm, is_integrated_power, f_lo, f_hi, cd))) return rc;
    std::vector<double> hB, hC, hD;
    std::vector<int32_t> hflags;
    if ((rc = carma_coefs_fetch(ctx, B, cd, nullptr, hB, hC, hD, hflags))) return rc;
    const int64_t J = cd.J;
    const size_t bj = (size_t)B * (size_t)J * sizeof(double);
    if (mu && (rc = upload(ctx, ctx->bmu, mu, B * sizeof(double)))) return rc;
    if (nu && (rc = upload(ctx, ctx->bnu, nu, B * sizeof(double)))) return rc;
    if (shift && (rc = stage_shift(ds, B, shift))) return rc;
    const MixedSource src{{(const double*)ctx->bA.p, (const double*)ctx->bB.p, (const double*)ctx->bC.p, (const double*)ctx->bD.p,
                           mu ? (const double*)ctx->bmu.p : nullptr, nu ? (const double*)ctx->bnu.p : nullptr,
                           shift ? (const double*)ctx->bY.p : nullptr, shift ? (const double*)ctx->bS2.p : nullptr}, true, false};
    // routed as the host-pointer entry routes a (c, d) row per draw
    if ((rc = value_from_draws(ds, B, J, src, draw_layout(ctx->opt, B, J, hB.data(), hC.data(), hD.data()), hC.data(), hD.data(), false, out, status)))
        return rc;
    if (A_out && (rc = download(ctx, A_out, ctx->bA.p, bj))) return rc;
    if (Bc_out && (rc = download(ctx, Bc_out, ctx->bB.p, bj))) return rc;
    if (C_out && (rc = download(ctx, C_out, ctx->bC.p, bj))) return rc;
    if (Dd_out && (rc = download(ctx, Dd_out, ctx->bD.p, bj))) return rc;
    SYNC(ctx);
    for (int64_t b = 0; b < B; ++b)   // a rejected draw ran on benign coefficients: its results are overwritten
        if (hflags[(size_t)b]) { out[b] = -INFINITY; if (status) status[b] = 3; }
    return PIORAN_OK;
}

int pioran_logpdf_batch_carma_grad(pioran_ds* ds, int64_t B, int p, int q, const double* qa, const double* qb, const double* norm, int is_integrated_power,
                                   double f_lo, double f_hi, const double* mu, const double* nu, const double* shift, double* out, int32_t* status,
                                   double* grad_qa, double* grad_qb, double* grad_norm, double* grad_nu, double* grad_mu, double* grad_shift, double* grad_a,
                                   double* grad_b, double* grad_c, double* grad_d)
{
    if (const int rc = carma_refuse(ds, B, p, q, 0, qa, qb, norm, f_lo, f_hi)) return rc;
    if (!out || !grad_qa || !grad_norm || (q > 0 && !grad_qb)) return PIORAN_ERR_ARG;
    if ((nu == nullptr) != (grad_nu == nullptr) || (mu == nullptr) != (grad_mu == nullptr) || (shift == nullptr) != (grad_shift == nullptr)) return PIORAN_ERR_ARG;
    const int n_inter = (grad_a != nullptr) + (grad_b != nullptr) + (grad_c != nullptr) + (grad_d != nullptr);
    if (n_inter != 0 && n_inter != 4) return PIORAN_ERR_ARG;
    pioran_ctx* ctx = ds->ctx;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    CarmaDraws cd;
    int rc;
    std::vector<double> hA, hB, hC, hD;
    std::vector<int32_t> hflags;
    {
        PendingGuard guard(ctx);
        if ((rc = stage_carma(ctx, B, p, q, 0, qa, qb, norm, is_integrated_power, f_lo, f_hi, cd))) return rc;
        if ((rc = carma_coefs_fetch(ctx, B, cd, &hA, hB, hC, hD, hflags))) return rc;
    }
    // (all draws in one launch of the windowed reverse mode where the shape fits it; one draw, and every draw of a shifted call, as a batch of its own)
    std::vector<double> inter;
    double* g[4] = {grad_a, grad_b, grad_c, grad_d};
    if ((rc = grad_through_host_coefs(ds, B, cd.J, hA.data(), hB.data(), hC.data(), hD.data(), hflags.data(), mu, nu, shift, out, status, grad_nu, grad_mu,
                                      grad_shift, g, inter)))
        return rc;
    PendingGuard guard(ctx);
    if ((rc = carma_vjp_from_host(ctx, B, cd, g[0], g[1], g[2], g[3], grad_qa, grad_qb, grad_norm, false))) return rc;
    SYNC(ctx);
    return PIORAN_OK;
}

const char* pioran_celerite_config_name(int64_t R)
{
    if (R == -2) return pioran_window_last_name();   // the instantiation of the calling thread's last windowed, tile or time-parallel launch (pioran_window_route)
    if (R < 0) return g_last_kernel;                 // kernel family of the calling thread's last launch: block, block+pd, wide, scan, fallback
    if (R <= 0) return pioran_scan_config_name(0);   // what the calling thread's last step-by-step launch (throughput or latency layout) ran on
    if (R > pioran_wide_supported_rows()) return "fallback";
    if (R > pioran_scan_supported_rows()) return "wide";   // 80 .. 143 rows: the lean latency kernel (80 with a shared table and a large batch: the scan)
    return pioran_scan_config_name((int)R);
}

// ---- in-process farm ----------------------------------------------------------------------------
struct pioran_farm {
    std::vector<pioran_ctx*> ctx;
    std::vector<pioran_ds*> ds;
};

int pioran_farm_create(int ngpu, const int* devices, int64_t N, const double* t, const double* y, const double* sigma2,
                       pioran_farm** out)
{
    if (!out || ngpu < 1 || ngpu > 64 || !devices || N < 1 || !t || !y || !sigma2) return PIORAN_ERR_ARG;
    *out = nullptr;
    pioran_farm* f = new (std::nothrow) pioran_farm;
    if (!f) return PIORAN_ERR_ALLOC;
    int rc = PIORAN_OK;
    for (int g = 0; g < ngpu && rc == PIORAN_OK; ++g) {
        pioran_ctx* c = nullptr;
        pioran_ds* d = nullptr;
        rc = pioran_ctx_create(devices[g], &c);
        if (rc == PIORAN_OK) {
            f->ctx.push_back(c);
            rc = pioran_dataset_create(c, N, t, y, sigma2, &d);
            if (rc == PIORAN_OK) f->ds.push_back(d);
        }
    }
    if (rc != PIORAN_OK) { pioran_farm_destroy(f); return rc; }
    *out = f;
    return PIORAN_OK;
}

int pioran_farm_destroy(pioran_farm* f)
{
    if (!f) return PIORAN_ERR_ARG;
    for (auto* d : f->ds) pioran_dataset_destroy(d);
    for (auto* c : f->ctx) pioran_ctx_destroy(c);
    delete f;
    return PIORAN_OK;
}

int pioran_farm_size(const pioran_farm* f) { return f ? (int)f->ds.size() : PIORAN_ERR_ARG; }

static int farm_batch_impl(pioran_farm* f, int64_t B, int64_t J, const double* A, const double* Bc, const double* C,
                           const double* Dd, int cd_shared, const double* mu, const double* nu, const double* shift,
                           const double* Y, const double* S2, double* out, int32_t* status)
{
    if (!f || f->ds.empty() || B < 1 || J < 1 || !A || !Bc || !C || !Dd || !out) return PIORAN_ERR_ARG;
    if ((Y == nullptr) != (S2 == nullptr) || (Y && shift)) return PIORAN_ERR_ARG;
    const int64_t N = f->ds[0]->N;
    const int64_t G = (int64_t)f->ds.size();
    const int64_t base = B / G, extra = B % G;
    std::vector<int> rcs(G, PIORAN_OK);
    std::vector<std::thread> th;
    for (int64_t g = 0; g < G; ++g) {
        const int64_t lo = g * base + (g < extra ? g : extra), nb = base + (g < extra ? 1 : 0);
        if (nb == 0) continue;
        th.emplace_back([=, &rcs]() {
            const double* Cg = cd_shared ? C : C + lo * J;
            const double* Dg = cd_shared ? Dd : Dd + lo * J;
            const double* mug = mu ? mu + lo : nullptr;
            const double* nug = nu ? nu + lo : nullptr;
            int32_t* stg = status ? status + lo : nullptr;
            rcs[g] = shift ? pioran_celerite_logl_batch_shift(f->ds[g], nb, J, A + lo * J, Bc + lo * J, Cg, Dg, cd_shared, mug,
                                                              nug, shift + lo, out + lo, stg)
                           : pioran_celerite_logl_batch(f->ds[g], nb, J, A + lo * J, Bc + lo * J, Cg, Dg, cd_shared, mug, nug,
                                                        Y ? Y + lo * N : nullptr, S2 ? S2 + lo * N : nullptr, out + lo, stg);
        });
    }
    for (auto& t_ : th) t_.join();
    for (int rc : rcs)
        if (rc != PIORAN_OK) return rc;
    return PIORAN_OK;
}

int pioran_farm_logl_batch(pioran_farm* f, int64_t B, int64_t J, const double* A, const double* Bc, const double* C,
                           const double* Dd, int cd_shared, const double* mu, const double* nu, const double* shift,
                           double* out, int32_t* status)
{
    return farm_batch_impl(f, B, J, A, Bc, C, Dd, cd_shared, mu, nu, shift, nullptr, nullptr, out, status);
}

int pioran_farm_logl_batch_series(pioran_farm* f, int64_t B, int64_t J, const double* A, const double* Bc, const double* C,
                                  const double* Dd, int cd_shared, const double* mu, const double* nu, const double* Y,
                                  const double* S2, double* out, int32_t* status)
{
    if (!Y || !S2) return PIORAN_ERR_ARG;
    return farm_batch_impl(f, B, J, A, Bc, C, Dd, cd_shared, mu, nu, nullptr, Y, S2, out, status);
}

// ---- dense solver -------------------------------------------------------------------------------
// (ascending time stamps — is_sorted — enable the factorised covariance build of dense.hip; anything else takes the direct one)

static int dense_stage(pioran_ctx* ctx, int64_t N, int64_t J, const double* a, const double* b, const double* c,
                       const double* d, const double* t, const double* y, const double* sigma2, double** dv)
{
    // one staging buffer: a b c d (J each) | t y s2 (N each) | out (1) | info
    const size_t nd = 4 * (size_t)J + 3 * (size_t)N + 2;
    int rc = ensure(ctx, ctx->bwork, nd * sizeof(double));
    if (rc) return rc;
    double* base = (double*)ctx->bwork.p;
    const double* src[7] = {a, b, c, d, t, y, sigma2};
    size_t off = 0;
    for (int i = 0; i < 7; ++i) {
        const size_t n = i < 4 ? (size_t)J : (size_t)N;
        dv[i] = base + off;
        if (src[i])
            HIPCHK(ctx, hipMemcpyAsync(dv[i], src[i], n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        else
            HIPCHK(ctx, hipMemsetAsync(dv[i], 0, n * sizeof(double), ctx->stream));
        off += n;
    }
    dv[7] = base + off;      // out
    dv[8] = base + off + 1;  // info (int32 in the first 4 bytes)
    int64_t Mp, ld;
    pioran_dense_dims(N, &Mp, &ld);
    return ensure(ctx, ctx->bK, ((size_t)Mp * (size_t)ld + PIORAN_DENSE_WS) * sizeof(double));
}

static int dense_nll_impl(pioran_ctx* ctx, int64_t N, int64_t J, const double* a, const double* b, const double* c,
                          const double* d, const double* t, const double* y, const double* sigma2, double* out,
                          int32_t* info, float* phase_ms)
{
    if (!ctx || N < 1 || J < 1 || !a || !b || !c || !d || !t || !y || !sigma2 || !out) return PIORAN_ERR_ARG;
    if (N > 46000) return PIORAN_ERR_UNSUPPORTED;  // slab would exceed ~17 GB
    HIPCHK(ctx, hipSetDevice(ctx->device));
    PendingGuard pending_guard(ctx);
    double* dv[9];
    int rc = dense_stage(ctx, N, J, a, b, c, d, t, y, sigma2, dv);
    if (rc) return rc;
    if (phase_ms) HIPCHK(ctx, hipEventRecord(ctx->ev[12], ctx->stream));
    rc = pioran_dense_nll_device(N, (int32_t)J, dv[0], dv[1], dv[2], dv[3], dv[4], dv[5], dv[6], (double*)ctx->bK.p,
                                 phase_ms ? &ctx->ev[13] : nullptr, dv[7], (int32_t*)dv[8], is_sorted(t, N), ctx->stream, 0.0, 1.0, &ctx->opt.dense);
    if (rc) { ctx->last_err = "dense kernel launch failed"; return rc; }
    int32_t hinfo = 0;
    if ((rc = download(ctx, out, dv[7], sizeof(double)))) return rc;
    HIPCHK(ctx, hipMemcpyAsync(&hinfo, dv[8], sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    SYNC(ctx);
    if (info) *info = hinfo;
    if (phase_ms)
        for (int i = 0; i < 3; ++i) HIPCHK(ctx, hipEventElapsedTime(&phase_ms[i], ctx->ev[12 + i], ctx->ev[13 + i]));
    return PIORAN_OK;
}

int pioran_dense_nll(pioran_ctx* ctx, int64_t N, int64_t J, const double* a, const double* b, const double* c,
                     const double* d, const double* t, const double* y, const double* sigma2, double* out,
                     int32_t* info)
{
    return dense_nll_impl(ctx, N, J, a, b, c, d, t, y, sigma2, out, info, nullptr);
}

int pioran_dense_nll_batch(pioran_ctx* ctx, int64_t N, int64_t J, int64_t B, const double* A, const double* Bc, const double* C,
                           const double* Dd, int cd_shared, const double* t, const double* y, const double* sigma2,
                           const double* mu, const double* nu, double* out, int32_t* info)
{
    if (!ctx || N < 1 || J < 1 || B < 1 || !A || !Bc || !C || !Dd || !t || !y || !sigma2 || !out) return PIORAN_ERR_ARG;
    if (N > 46000) return PIORAN_ERR_UNSUPPORTED;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    PendingGuard pending_guard(ctx);
    int rc;
    int64_t Mp, ld;
    pioran_dense_dims(N, &Mp, &ld);
    const size_t slab = (size_t)Mp * (size_t)ld + PIORAN_DENSE_WS;
    // Several factorisations per launch (round 3, late): a single N = 4096 factorisation is a chain of 64 latency-bound steps that
    // leaves most of the chip idle; with gridDim.z = nb matrices every kernel of the chain is launched once per BATCH (16 concurrent
    // streams of single-matrix launches gave 0.96 ms per factorisation, tools/sweep_dense_streams.py).  As many slabs as fit in a
    // third of the free memory, at most 32 (option dense_streams: fewer).
    const int64_t max_batch = ctx->opt.dense_streams > 0 && ctx->opt.dense_streams <= 64 ? ctx->opt.dense_streams : 32;
    int64_t ns = B < max_batch ? B : max_batch;
    {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess)
            while (ns > 1 && (size_t)ns * slab * sizeof(double) > free_b / 3 + ctx->bK.cap) --ns;
    }
    while ((rc = ensure(ctx, ctx->bK, (size_t)ns * slab * sizeof(double))) == PIORAN_ERR_ALLOC && ns > 1) --ns;
    if (rc) return rc;
    // staging: A Bc [B][J] | C D ([J] or [B][J]) | t y s2 [N] | mu nu [B] | out [B] | info [B] (int32)
    const size_t ncd = cd_shared ? (size_t)J : (size_t)B * J;
    const size_t nd = 2 * (size_t)B * J + 2 * ncd + 3 * (size_t)N + 4 * (size_t)B;
    if ((rc = ensure(ctx, ctx->bwork, nd * sizeof(double)))) return rc;
    double* dA = (double*)ctx->bwork.p; double* dB = dA + (size_t)B * J; double* dC = dB + (size_t)B * J; double* dD = dC + ncd;
    double* dt = dD + ncd; double* dy = dt + N; double* ds2 = dy + N; double* dmu = ds2 + N; double* dnu = dmu + B;
    double* dout = dnu + B; int32_t* dinfo = (int32_t*)(dout + B);
    HIPCHK(ctx, hipMemcpyAsync(dA, A, (size_t)B * J * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(dB, Bc, (size_t)B * J * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(dC, C, ncd * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(dD, Dd, ncd * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(dt, t, (size_t)N * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(dy, y, (size_t)N * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(ds2, sigma2, (size_t)N * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    if (mu) HIPCHK(ctx, hipMemcpyAsync(dmu, mu, (size_t)B * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    if (nu) HIPCHK(ctx, hipMemcpyAsync(dnu, nu, (size_t)B * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    const int sorted = is_sorted(t, N);
    for (int64_t b0 = 0; b0 < B; b0 += ns) {
        const int64_t nb = B - b0 < ns ? B - b0 : ns;
        rc = pioran_dense_nll_device_batch(nb, N, (int32_t)J, dA + b0 * J, dB + b0 * J, cd_shared ? dC : dC + b0 * J, cd_shared ? dD : dD + b0 * J,
                                           cd_shared ? 0 : J, dt, dy, ds2, (double*)ctx->bK.p, (int64_t)slab, mu ? dmu + b0 : nullptr,
                                           nu ? dnu + b0 : nullptr, dout + b0, dinfo + b0, sorted, ctx->stream, &ctx->opt.dense);
        if (rc) { ctx->last_err = "dense kernel launch failed"; return rc; }
    }
    if ((rc = download(ctx, out, dout, (size_t)B * sizeof(double)))) return rc;
    if (info) if ((rc = download(ctx, info, dinfo, (size_t)B * sizeof(int32_t)))) return rc;
    SYNC(ctx);
    return PIORAN_OK;
}

int pioran_dense_nll_timed(pioran_ctx* ctx, int64_t N, int64_t J, const double* a, const double* b, const double* c,
                           const double* d, const double* t, const double* y, const double* sigma2, double* out,
                           int32_t* info, float* phase_ms)
{
    if (!phase_ms) return PIORAN_ERR_ARG;
    return dense_nll_impl(ctx, N, J, a, b, c, d, t, y, sigma2, out, info, phase_ms);
}

// predict_direct / predict_cov (src/direct_solver.jl:28-119): y == nullptr: covariance only; cov_out == nullptr: mean only
static int dense_predict_impl(pioran_ctx* ctx, int64_t N, int64_t J, const double* a, const double* b, const double* c,
                              const double* d, const double* t, const double* y, const double* sigma2, int64_t M,
                              const double* tau, double* mean_out, double* cov_out, int32_t* info)
{
    if (!ctx || N < 1 || J < 1 || M < 1 || !a || !b || !c || !d || !t || !sigma2 || !tau) return PIORAN_ERR_ARG;
    if ((y == nullptr) != (mean_out == nullptr) || (!mean_out && !cov_out)) return PIORAN_ERR_ARG;
    const int64_t Mp = (N + 63) / 64 * 64, Mq = (M + 63) / 64 * 64, Mtot = Mp + Mq;
    if (Mtot > 46000) return PIORAN_ERR_UNSUPPORTED;  // slab would exceed ~17 GB
    HIPCHK(ctx, hipSetDevice(ctx->device));
    PendingGuard pending_guard(ctx);
    // [t | NaN padding | tau | NaN padding]: a NaN time is an identity row/column of the augmented matrix
    std::vector<double> te((size_t)Mtot, std::nan("")), s2e((size_t)Mtot, 0.0), ye((size_t)Mtot, 0.0);
    std::memcpy(te.data(), t, (size_t)N * sizeof(double));
    std::memcpy(s2e.data(), sigma2, (size_t)N * sizeof(double));
    std::memcpy(te.data() + Mp, tau, (size_t)M * sizeof(double));
    if (y) std::memcpy(ye.data(), y, (size_t)N * sizeof(double));
    double* dv[9];
    int rc = dense_stage(ctx, Mtot, J, a, b, c, d, te.data(), ye.data(), s2e.data(), dv);
    if (rc) return rc;
    // dense_stage copies asynchronously from the vectors above: they must outlive the copies
    SYNC(ctx);
    if ((rc = ensure(ctx, ctx->bout, (size_t)M * sizeof(double)))) return rc;
    rc = pioran_dense_predict_cov_device(N, M, (int32_t)J, dv[0], dv[1], dv[2], dv[3], dv[4], dv[6], (double*)ctx->bK.p,
                                         (int32_t*)dv[8], y ? dv[5] : nullptr, y ? (double*)ctx->bout.p : nullptr, ctx->stream);
    if (rc) { ctx->last_err = "dense prediction launch failed"; return rc; }
    const int64_t ld = Mtot + 64;
    int32_t hinfo = 0;
    if (cov_out)
        HIPCHK(ctx, hipMemcpy2DAsync(cov_out, (size_t)M * sizeof(double), (const double*)ctx->bK.p + Mp + Mp * ld,
                                     (size_t)ld * sizeof(double), (size_t)M * sizeof(double), (size_t)M, hipMemcpyDeviceToHost,
                                     ctx->stream));
    if (mean_out) if ((rc = download(ctx, mean_out, ctx->bout.p, (size_t)M * sizeof(double)))) return rc;
    HIPCHK(ctx, hipMemcpyAsync(&hinfo, dv[8], sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    SYNC(ctx);
    if (cov_out) {
        // the slab holds the lower triangle (column k, rows i >= k): mirror it
        for (int64_t k = 0; k < M; ++k)
            for (int64_t i = k + 1; i < M; ++i) cov_out[i * M + k] = cov_out[k * M + i];
        if (hinfo != 0)
            for (int64_t e = 0; e < M * M; ++e) cov_out[e] = std::nan("");
    }
    if (info) *info = hinfo;
    return PIORAN_OK;
}

int pioran_dense_predict_cov(pioran_ctx* ctx, int64_t N, int64_t J, const double* a, const double* b, const double* c,
                             const double* d, const double* t, const double* sigma2, int64_t M, const double* tau,
                             double* cov_out, int32_t* info)
{
    if (!cov_out) return PIORAN_ERR_ARG;
    return dense_predict_impl(ctx, N, J, a, b, c, d, t, nullptr, sigma2, M, tau, nullptr, cov_out, info);
}

int pioran_dense_predict(pioran_ctx* ctx, int64_t N, int64_t J, const double* a, const double* b, const double* c,
                         const double* d, const double* t, const double* y, const double* sigma2, int64_t M,
                         const double* tau, double* mean_out, double* cov_out, int32_t* info)
{
    if (!y || !mean_out) return PIORAN_ERR_ARG;
    return dense_predict_impl(ctx, N, J, a, b, c, d, t, y, sigma2, M, tau, mean_out, cov_out, info);
}

int pioran_dense_covariance(pioran_ctx* ctx, int64_t N, int64_t J, const double* a, const double* b, const double* c,
                            const double* d, const double* t, const double* sigma2, double* K_out)
{
    if (!ctx || N < 1 || J < 1 || !a || !b || !c || !d || !t || !K_out) return PIORAN_ERR_ARG;
    if (N > 46000) return PIORAN_ERR_UNSUPPORTED;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    double* dv[9];
    int rc = dense_stage(ctx, N, J, a, b, c, d, t, nullptr, sigma2, dv);
    if (rc) return rc;
    rc = pioran_dense_build_device(N, (int32_t)J, dv[0], dv[1], dv[2], dv[3], dv[4], dv[5], dv[6], (double*)ctx->bK.p,
                                   is_sorted(t, N), ctx->stream);
    if (rc) { ctx->last_err = "dense build launch failed"; return rc; }
    int64_t Mp, ld;
    pioran_dense_dims(N, &Mp, &ld);
    HIPCHK(ctx, hipMemcpy2DAsync(K_out, (size_t)N * sizeof(double), ctx->bK.p, (size_t)ld * sizeof(double),
                                 (size_t)N * sizeof(double), (size_t)N, hipMemcpyDeviceToHost, ctx->stream));
    SYNC(ctx);
    // the slab holds the lower triangle (column-major): mirror it, K is symmetric (src/direct_solver.jl:9-14 fills both)
    for (int64_t k = 0; k < N; ++k)
        for (int64_t i = k + 1; i < N; ++i) K_out[k + i * N] = K_out[i + k * N];
    return PIORAN_OK;
}


}  // extern "C"
