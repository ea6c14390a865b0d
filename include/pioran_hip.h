/*
 * pioran_hip.h — C ABI of libpioran_hip.so: the MI355X (gfx950) implementation of the ScalableGP
 * log-likelihood hot path of mlefkir/Pioran.jl (v1.2.0).
 *
 * This is the drop-in boundary.  The reference is pure Julia and has no FFI on this path; the seam
 * it would bind with `ccall` is the narrow waist
 *     logl(a, b, c, d, τ, y, σ2)                      src/celerite_solver.jl:312-334
 * reached from
 *     Distributions.logpdf(f::FiniteScalableGP, Y)    src/scalable_GP.jl:162-166
 *       -> log_likelihood(cov, τ, y, σ2; solver)      src/celerite_solver.jl:262-294
 * and, for the dense solver,
 *     log_likelihood_direct(cov, t, y, σ²)            src/direct_solver.jl:6-21.
 * INTEGRATION.md shows the Julia-side binding (julia/PioranHIP.jl in the package directory).
 *
 * Conventions
 *   - plain C, all floating point is IEEE fp64, all sizes int64_t, no torch / C++ types;
 *   - "host" pointers are ordinary process memory, "device" pointers are HBM of the ctx's GPU;
 *   - matrices over the batch are "J x B column-major" = Julia `Matrix{Float64}(J, B)` = C `[B][J]`:
 *     draw b's coefficients are contiguous at  A + b*J ;  series over the batch likewise `[B][N]`;
 *   - every entry point returns 0 (PIORAN_OK) or a negative error code; nothing unwinds across the
 *     ABI.  Numerical failures of single draws are reported per draw in `status` (below);
 *   - calls on one ctx must not overlap in time (one ctx per host thread / Julia task); different
 *     ctx objects are independent.  No global mutable state, no HIP call at library load; the
 *     environment is read once, when a context is created (diagnostic switches, pioran_ctx_set_option).
 *   - a data set keeps the state declared by pioran_dataset_prepare (the "(c, d) + table" the asynchronous
 *     *_dev entries use) SEPARATE from the scratch state of the host-pointer entries: pioran_celerite_logl_batch,
 *     _shift, pioran_logpdf_batch_theta, _predict, _logl_grad prepare their own tables and never change what
 *     pioran_dataset_prepare declared, so host-pointer and *_dev calls can be mixed freely on one data set.
 *
 * Accuracy (which kernel family evaluates a draw depends on rows, batch size and per-draw inputs; the calling thread's last family:
 *   pioran_celerite_config_name(-1)).  With ratio = nu min(sigma2) / sum(a) ~ 1 / cond(K) of a draw:
 *   - ratio >= 1e-8: every family is within 4.5e-9 (relative) of the exact value of its fp64 inputs, <= 3e-11 from ratio 1e-5 on
 *     (every stored chain of the reference sits there); families agree to 3e-10 over prior draws of the bench model;
 *   - ratio < 1e-8: the reference's own recurrence in fp64 is up to 7.8e-9 from the exact value; the step-by-step kernels follow it
 *     (6 .. 8e-9), the windowed kernels ("tile", "block": large and small batches from 5 rows on) reach 2 .. 3.2e-8 on single draws,
 *     the time-parallel family ("tp") 1e-10 — for a draw that passes its check: a draw of a long series whose boundary scan fails the check (0.3 .. 2 %
 *     of the prior draws of the SHO models, 6 .. 15 % of DRWCelerite's; option "tp_scan_tol") is evaluated again by the windowed kernel and has ITS
 *     accuracy, under the same name "tp".  Two families can therefore differ by up to 4e-8 on such a draw; no single stage of the
 *     windowed form removes that within 1 % of its time (profiles/r06_window_precision_by_stage.txt).  A caller that needs one
 *     family for every batch size pins it: options "no_tile", "no_block", "no_tp", "scan_config".
 *   - draws flagged in `status` (below): the families agree only to ~1e-6 (which D_n crosses zero within rounding differs).
 *
 * status[b]:  0 ok;  1 some D_n <= 0 (matrix not positive definite — the reference silently uses
 *             log(abs(D_n)) for n >= 2, src/celerite_solver.jl:140, and so does out[b]);
 *             2 non-finite result (the reference would throw DomainError from log(D_1 < 0), :126).
 */
#ifndef PIORAN_HIP_H
#define PIORAN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PIORAN_OK 0
#define PIORAN_ERR_ARG (-1)         /* null pointer, non-positive size, inconsistent arguments */
#define PIORAN_ERR_HIP (-2)         /* a HIP runtime call failed; see pioran_last_hip_error */
#define PIORAN_ERR_ALLOC (-3)       /* device or host allocation failed */
#define PIORAN_ERR_UNSUPPORTED (-4) /* rank / size outside what the kernels handle */

typedef struct pioran_ctx pioran_ctx; /* one GPU + one stream + scratch; not thread-safe */
typedef struct pioran_ds pioran_ds;   /* a time series resident in HBM + its cached shared table */

const char* pioran_strerror(int code);
const char* pioran_last_hip_error(const pioran_ctx* ctx);
/* ABI version of this header (bumped on any signature change). */
int pioran_abi_version(void);   /* currently 7 */

/* ---- context ------------------------------------------------------------------------------- */
/* Creates a context on GPU `device` with its own non-blocking stream. */
int pioran_ctx_create(int device, pioran_ctx** out);
/* Same, but work is enqueued on the caller's hipStream_t (e.g. torch's current stream). */
int pioran_ctx_create_on_stream(int device, void* hip_stream, pioran_ctx** out);
int pioran_ctx_destroy(pioran_ctx* ctx);
int pioran_ctx_synchronize(pioran_ctx* ctx);
/* Releases every scratch buffer the context has grown (staging, gradient / prediction workspaces, the dense slab); they are
 * re-allocated on demand.  Data sets and their tables are not touched. */
int pioran_ctx_trim(pioran_ctx* ctx);
/* Diagnostic switches (none is needed in production; tests and tuning runs use them to pin a code path):
 *   "scan_config"     name of a throughput configuration of the scan, "wide" = latency layout or "block" = windowed kernel for
 *                     any batch; NULL/"" = automatic
 *   "no_wide" / "no_block" / "no_paired" / "no_mixed" / "force_fallback"   value "1" disables the latency layout / the windowed
 *                     small-batch kernel / the column-paired variants / the mixed shared+per-draw table / sends everything through
 *                     the any-rank kernel; NULL, "" or "0" = off.
 *   "win2" / "no_win2"  force / forbid the two-step form of the throughput layouts (default: on up to four rows per lane, i.e. R <= 63)
 *   "win3" / "no_win3"  force / forbid the three-step form (two or three rows per lane; default: on for R = 24 .. 31 in large batches)
 *   "wide2" / "no_wide2"  force / forbid the lean form of the latency layout (default: from 48 rows on; the only form for 96 .. 143 rows);
 *                     also selects the lean / round-1 kernels of the step-by-step gradient, prediction and simulation (64 .. 95 rows)
 *   "no_split"        a batch that is not a whole number of passes runs as one launch (default: the remainder goes to the windowed kernel)
 *   "workspace_limit_mb"  cap on the per-call workspaces (default 16384)
 *   "no_tile"         value "1": never the windowed form with one draw per wavefront (celerite_tile.hip); "scan_config" = "tile" forces it for
 *                     every launch it can take
 *   "no_tp"           value "1": never the time-parallel evaluation (celerite_tp.hip: segments of the series on different CUs, for a handful of
 *                     draws of a long series).  Automatic choice, round 6 (its boundary phase as a scan over the segments' elements): one or two draws with
 *                     3-4 / 5-16 / 24 / 32 / 40-48 / 56-64 state rows from 2048 / 1024 / 1536 / 2048 / 3072 / 4096 steps on, 3 .. 32 draws where a model of its
 *                     time promises 15 % against the serial chains; with the boundary walk of round 5: up to 8 draws with up to 4 / 8 / 12 / 16 state rows
 *                     from 1024 / 2048 / 4096 / 6144 steps on, up to 64 draws at up to 4 rows from 4096, up to 8 draws with up to 24 / 32 / 40 / 48 / 64 rows from
 *                     5120 / 6144 / 8192 / 8192 / 12288;
 *                     "scan_config" = "tp" forces it wherever it applies (shared (c, d), up to 64 state rows, up to 64 draws);
 *                     "tp_segments" its segment count (0 / NULL = automatic);
 *                     "tp_scan" -1 (default) automatic, 0 the boundary walk, 1 the scan wherever the rows allow (3 .. 64);
 *                     "tp_scan_tol" the scan's acceptance threshold: the filter measures how far the scan's boundary states are from the sequential ones (on the scale of the
 *                     innovation variance) and a draw whose largest distance exceeds it is evaluated again on the serial chain — 0.3 .. 2 % of the
 *                     prior draws of the SHO models, 6 .. 15 % of DRWCelerite's (0 / NULL = 1e-3; negative: every draw — tests); the boundary walk is checked the
 *                     same way; "tp_unchecked" = "1" (with "scan_config" = "tp"): the family's own arithmetic, no check, no repair (tests, tools); "tp_walk_repair" = "1": by the family's own
 *                     boundary walk instead; "tp_scan_lean" = "1", "tp_scan_waves" = "4": the forms of the combination kernel that are the default only at
 *                     49 .. 64 rows / up to 16 rows (tests, tools)
 *   "dense_old_chain" 0 one launch per block column (default), 1 the panel / update chain of rounds 1-3 (any other value: PIORAN_ERR_ARG);
 *                     "dense_no_pairs", "dense_no_halves", "dense_pair_tiles", "dense_half_tile_limit", "dense_quad_threshold", "dense_batch_pair_threshold", "dense_streams": schedule knobs
 *   "block_emode", "exp"   tuning / experiment selectors of single kernels (tools/ only; "exp" can make results meaningless)
 *   "pc_events"       timing tools only: the first chunk of a pioran_psd_check_* call records the event slots 4 .. 6 (before the per-draw kernel | after it |
 *                     after the evaluation kernel)
 * Initial values come from the environment variables PIORAN_SCAN_CONFIG, PIORAN_NO_WIDE, PIORAN_NO_BLOCK, PIORAN_NO_TILE, PIORAN_NO_TP, PIORAN_NO_PAIRED,
 * PIORAN_NO_MIXED, PIORAN_FORCE_FALLBACK, PIORAN_WIN2, PIORAN_NO_WIN2, PIORAN_WIDE2, PIORAN_NO_WIDE2, read once when the context is created. */
int pioran_ctx_set_option(pioran_ctx* ctx, const char* key, const char* value);
/* hipEvent-based timing on the ctx stream: record slot i (0..11), elapsed between two slots. */
int pioran_ctx_event_record(pioran_ctx* ctx, int slot);
int pioran_ctx_event_elapsed_ms(pioran_ctx* ctx, int slot_start, int slot_stop, float* ms);

/* ---- data set ------------------------------------------------------------------------------ */
/* Uploads (t, y, sigma2), each of length N (host pointers), once.  y is the raw series: the mean
 * is subtracted per draw (mu), as logpdf does (src/scalable_GP.jl:164). */
int pioran_dataset_create(pioran_ctx* ctx, int64_t N, const double* t, const double* y,
                          const double* sigma2, pioran_ds** out);
int pioran_dataset_destroy(pioran_ds* ds);
/* Declares the (c_j, d_j) shared by every draw of the following *_dev batches and builds the
 * cos/sin/exp table for them (src/celerite_solver.jl:52-54, once instead of per draw).
 * c, d: host, length J.  real_term (host, length J, may be NULL): non-zero marks a term whose
 * b_j = 0 and d_j = 0 for EVERY draw (Exp / DRW terms, src/Exp.jl:29-33, src/psd.jl:270-273); its
 * identically-zero sin row is dropped, which leaves results bit-identical.  (The value 2 — a term whose (c, d)
 * differ per draw — is accepted for table-building purposes but the *_dev entries then return PIORAN_ERR_ARG: per-draw
 * terms go through the host-pointer entry with cd_shared = 0, which builds the mixed table itself.)
 * The declared state persists until the next pioran_dataset_prepare on this data set; no other entry changes it.
 * Device memory: the table takes (6 J + 8)(N + 1) * 8 bytes (10 MB at N = 1e4, J = 20); the first small batch (at most 512
 * draws; 768 with 32 .. 47 rows, 1024 with 36 .. 47 rows; 5 .. 63 rows — and up to 256 draws with 64 .. 95 rows; fewer than five rows: series of 16384 and more stamps, and the scalar call from N = 2048 on) builds a second table for the windowed small-batch kernel,
 * ~(30 J + 300) N bytes (37 MB there), and falls back to the other kernels if that does not fit (2 GB cap).
 * Entries that chunk their draws (per-draw (c, d) tables: 37 MB per draw; prediction: 2.6 GB, simulation: 1.4 GB, gradient: 6 GB per 256 draws at
 * N = 1e4, J = 20) take at most half of the free device memory and never more than the context option "workspace_limit_mb"
 * (default 16384); the buffers stay with the context until pioran_ctx_trim. */
int pioran_dataset_prepare(pioran_ds* ds, int64_t J, const double* c, const double* d,
                           const int32_t* real_term);

/* ---- celerite solver ------------------------------------------------------------------------ */
/* Scalar drop-in for logl(a,b,c,d,τ,y,σ2) (src/celerite_solver.jl:312-334): host vectors in, one
 * double out.  y has the mean already subtracted, as in the reference.  status may be NULL.
 * The series handle (and the tables of (c, d)) is kept while t is unchanged; small calls issue no copy commands for the coefficients
 * and the result (the kernels read / write the context's pinned host memory; late round 4: 39 -> 29 us at N = 32). */
int pioran_celerite_logl(pioran_ctx* ctx, int64_t N, int64_t J, const double* a, const double* b,
                         const double* c, const double* d, const double* t, const double* y,
                         const double* sigma2, double* out, int32_t* status);

/* B independent log-likelihoods on one data set; host pointers; blocks until `out` is filled.
 *   A, Bc      : [B][J]
 *   C, Dd      : [J] when cd_shared != 0, else [B][J] (per-draw decay/frequency: QPO, CARMA, ...)
 *   mu         : [B] or NULL (0):   y_n - mu_b                      (ConstMean, scalable_GP.jl:164)
 *   nu         : [B] or NULL (1):   sigma2_n * nu_b                 (the models' ν, README.md:44)
 *   Y, S2      : [B][N] or NULL: per-draw series / variances that REPLACE the data set's y / sigma2
 *                (models with a sampled shift, docs/src/ultranest.md:199-205); mu, nu still apply
 *   out        : [B]     status: [B] or NULL */
int pioran_celerite_logl_batch(pioran_ds* ds, int64_t B, int64_t J, const double* A,
                               const double* Bc, const double* C, const double* Dd, int cd_shared,
                               const double* mu, const double* nu, const double* Y,
                               const double* S2, double* out, int32_t* status);

/* Same computation with every array already in HBM (device pointers) and (c, d) declared by
 * pioran_dataset_prepare.  Asynchronous: enqueues on the ctx stream and returns; use
 * pioran_ctx_synchronize (or the stream) before reading out/status.  dmu, dnu, dY, dS2, dstatus
 * may be NULL. */
int pioran_celerite_logl_batch_dev(pioran_ds* ds, int64_t B, const double* dA, const double* dBc,
                                   const double* dmu, const double* dnu, const double* dY,
                                   const double* dS2, double* dout, int32_t* dstatus);
/* Per-draw (c, d) variant of the above: dC, dDd are [B][J] device arrays, no shared table. */
int pioran_celerite_logl_batch_dev_cd(pioran_ds* ds, int64_t B, int64_t J, const double* dA,
                                      const double* dBc, const double* dC, const double* dDd,
                                      const double* dmu, const double* dnu, const double* dY,
                                      const double* dS2, double* dout, int32_t* dstatus);
/* Per-draw data transform on the device — the reference's production models sample a shift c_b and fit the
 * log-flux (docs/src/ultranest.md:199-205, examples/ultranest/single_pl.jl:65-86, benchmark/benchmarks.jl:58-59):
 *     y_b      = log(y - shift_b)
 *     sigma2_b = sigma2 / (y - shift_b)^2            (then mu_b, nu_b exactly as above)
 * The data set holds the RAW flux y and sigma2 = yerr^2.  Only shift[B] crosses the boundary; the [B][N]
 * transformed series are built in HBM by a transform kernel.  y - shift_b <= 0 gives status 2 (NaN), where the
 * reference throws DomainError from log.  Host-pointer (blocking) and device-pointer (asynchronous) forms. */
int pioran_celerite_logl_batch_shift(pioran_ds* ds, int64_t B, int64_t J, const double* A, const double* Bc,
                                     const double* C, const double* Dd, int cd_shared, const double* mu,
                                     const double* nu, const double* shift, double* out, int32_t* status);
int pioran_celerite_logl_batch_shift_dev(pioran_ds* ds, int64_t B, const double* dA, const double* dBc,
                                         const double* dmu, const double* dnu, const double* dshift,
                                         double* dout, int32_t* dstatus);
/* theta -> log L in one call: `approx` (src/psd.jl:214-289) runs on the device in front of the scan, so only the
 * sampled parameters cross the boundary.  Continuum PSD models:
 *   model 0  SingleBendingPowerLaw(alpha1, f1, alpha2)                  P = 3 parameters per draw
 *   model 1  DoubleBendingPowerLaw(alpha1, f1, alpha2, f2, alpha3)      P = 5
 * basis 0 "SHO" (J = n_components terms), 1 "DRWCelerite" (J = 2 n_components terms);
 * theta [B][P], norm [B] (the `norm` argument of approx), is_integrated_power / S_low / S_high as in approx;
 * mu, nu, shift: [B] or NULL, as in pioran_celerite_logl_batch[_shift].
 * PSD features (`continuum + QPO(S0, f0, Q) + ...`, src/psd.jl:15-27, 228-241, 254-261): n_qpo (0..8) Lorentzians per draw,
 * qpo [B][n_qpo][3] = (S0, f0, Q) (NULL when n_qpo = 0); each becomes one more celerite term whose (c, d) differ per draw —
 * the scan then runs in the mixed mode (shared table for the continuum, per-draw rows for the features).
 * Host pointers, blocking.  Also returns, when A_out / Bc_out are non-NULL ([B][J + n_qpo] host), the coefficients
 * approx produced (feature terms last, as the reference concatenates them). */
int pioran_logpdf_batch_theta(pioran_ds* ds, int64_t B, int model, int64_t n_components, int basis,
                              int is_integrated_power, double f_min, double f_max, double S_low, double S_high,
                              const double* theta, const double* norm, const double* mu, const double* nu,
                              const double* shift, int64_t n_qpo, const double* qpo, double* out, int32_t* status,
                              double* A_out, double* Bc_out);
/* ---- posterior mean and simulation (the callers either side of the likelihood) -----------
 * predict (src/celerite_solver.jl:348-361 -> pred :363-483; mean(::PosteriorGP, tau) of src/scalable_GP.jl:64-72,90-91):
 *     mean_out[b][m] = mu_b + sum_n z_n k_b(|tau_m - t_n|),   z = K_b^-1 (y - mu_b),  K_b = kernel_b + diag(nu_b sigma2)
 * for B draws of (a, b); (c, d) [J] shared (cd_shared != 0) or [B][J] per draw (see the last paragraph).  tau: M evaluation
 * times, any order (the reference wants them sorted).
 * status (may be NULL) as in pioran_celerite_logl_batch.  Host pointers, blocking.
 * Up to 63 rows (from one row on since late round 4; six before) and shared (c, d) both calls run on the windowed factorisation (celerite_block.hip, round 3): z by a block
 * back-substitution, the two running vectors of `pred` in 128-step segments, the tau-only factors once per call — 6.1 ms per 256
 * draws x 1e4 times at N = 1e4, J = 20 (18.5 ms before); the simulation applies L window by window (5.0 ms per 256 draws, 8.7 before).
 * Workspace: the factor as the consumer reads it (6 KB per 16-step window and draw at three block columns; 8.5 KB for the simulation — up to
 * late round 4 both used the reverse mode's 41 KB layout) + 2 N R doubles per draw for the running vectors (2.6 GB for 256 draws at N = 1e4,
 * R = 40, 8.3 GB before; the chunk of draws shrinks to what is free).  Other shapes: the step-by-step
 * kernels — the factor stored by the latency kernels (the lean one from 64 rows on, round 4): posterior mean and simulation up to 143 rows (the reference
 * benchmark grid's j = 64 is 128); beyond: PIORAN_ERR_UNSUPPORTED before any workspace is taken.  pioran_celerite_config_name(-1)
 * tells which ran ("block (windowed prediction)" / "wide (step-by-step prediction)", likewise "... simulation").
 * cd_shared == 0 with several draws: where 2 J rows fit the windowed kernel all draws of a chunk go through every kernel in one launch, each
 * with its own tables (64 draws: 7.5 ms predict, 4.6 ms simulate at N = M = 1e4, J = 20; draw by draw 910 / 439 ms). */
int pioran_celerite_predict(pioran_ds* ds, int64_t B, int64_t J, const double* A, const double* Bc, const double* C,
                            const double* Dd, int cd_shared, const double* mu, const double* nu, int64_t M, const double* tau,
                            double* mean_out, int32_t* status);
/* Posterior variance of the latent process at new times (what sqrt.(diag(predict_cov(...))) of src/scalable_GP.jl:103-104 obtains from a dense
 * (N + M) x (N + M) Cholesky), through the celerite factorisation in O((N + M) R^2) per draw:
 *     var_out[b][m] = k_b(0) - k*' K_b^-1 k*,   k*_n = k_b(|tau_m - t_n|),  K_b = kernel_b + diag(nu_b sigma2),  k_b(0) = sum_j a_j
 * (no measurement noise added, as predict_cov gives it; mu does not enter and the data set's y is ignored).  The factor (W_n, D_n) is stored by the
 * latency kernel as for the step-by-step prediction; a forward walk carries S+_n = S_n + D_n W_n W_n' and a backward walk
 * B_n = U~_n U~_n'/D_n + A_n' B_{n+1} A_n, A_n = diag(phi_{n+1}) (I - W_n U~_n'), one wavefront per draw with the R x R matrix in registers
 * (celerite_predict.hip); no R x R matrix goes to memory: the workspace beyond the factor is M (R rounded up to 16, + 1) doubles per draw,
 * draws are processed in chunks sized to the free memory.
 * The result is a difference of numbers of the size of k(0): its error is ABSOLUTE on the scale of k(0) (measured: 3e-12 k(0) at N = 2000 against
 * the dense formula, which has the same property with a smaller constant; docs/EXPERIMENTS.md section 16) — a variance far below k(0) carries a correspondingly larger relative error.
 * tau: M >= 0 evaluation times in any order (an index is sorted on the host and the result scattered back); a non-finite tau: PIORAN_ERR_ARG.
 * A tau equal to a data time is an ordinary point.  nu [B] (may be NULL) scales sigma2.  C, Dd: [J] (cd_shared != 0) or [B][J] (each draw then
 * evaluated as its own one-draw batch with its own table).  status (may be NULL): 0, or 2 with NaN in the draw's row where a D_n is not positive.
 * At most 64 active rows; more: PIORAN_ERR_UNSUPPORTED before any workspace is taken.  NULL ds / tau / var_out (with M > 0): PIORAN_ERR_ARG before
 * any GPU call.  Host pointers, blocking.  pioran_celerite_config_name(-1) afterwards: "wide (step-by-step variance)". */
int pioran_celerite_predict_var(pioran_ds* ds, int64_t B, int64_t J, const double* A, const double* Bc, const double* C,
                                const double* Dd, int cd_shared, const double* nu, int64_t M, const double* tau, double* var_out,
                                int32_t* status);
/* log L and its gradient (what ForwardDiff obtains through the generic `logl`,
 * src/celerite_solver.jl:316, test/test_likelihood.jl:55-60) by reverse mode through the recurrence, for B draws:
 *   grad_a, grad_b [B][J] = dlogL/da_j, dlogL/db_j;
 *   grad_c, grad_d [B][J] (may be NULL) = dlogL/dc_j, dlogL/dd_j — what QPO features (src/psd.jl:15-27), CARMA kernels
 *       (src/CARMA.jl:98-143) and free Celerite terms need; per draw also when (c, d) are shared (sum over b for a common parameter);
 *       grad_b_j and grad_d_j of a one-row term (b_j = d_j = 0: no sine row, no phase) are structurally zero, and every reverse mode writes exactly
 *       0.0 there — never the caller's memory left as it was, a stale value of an earlier chunk or a NaN: every kernel family stores all J entries
 *       of each array asked for, and what it adds up for such a term is zero (the step-by-step kernels add nothing for a row without a phase).
 *       tests/test_gpu_grad_truth.py asserts it with == on every family;
 *   grad_nu, grad_mu [B] (may be NULL);
 *   grad_y, grad_sigma2 [B][N] (may be NULL) = dlogL/dy_n and dlogL/dsigma2_n of the series in the data set — what a
 *       model that transforms the data per draw (the sampled shift of docs/src/ultranest.md:199-205) chains through.
 * C, Dd: [J] when cd_shared != 0, else [B][J] (windowed reverse mode: every draw its own tables, all draws in one launch — 16 chains
 *   8 ms at N = 1e4, J = 20; shapes past 63 rows: each draw evaluated as its own one-draw batch).
 * Two reverse modes.  Up to 63 rows (from one row on since late round 4: 16.4 -> 4.4 ms at N = 1e4; six before) the WINDOWED reverse mode runs (celerite_block.hip, round 3): the windowed forward pass leaves T,
 * M', Sigma^-1 X' and Sigma^-1 of every 16-step window (38 KB per window at J = 20: 24 MB per draw at N = 1e4; chains are
 * processed 512 at a time — 12 GB —, fewer when the context option "workspace_limit_mb" or the free memory say so) and the adjoint kernel
 * walks the windows backwards with six GEMM stages each — value + gradient 5.4 ms for one chain, 5.8 ms for 256 (6.1 .. 6.3 ms with
 * grad_c / grad_d).  With 64 .. 143 rows (and as a cross-check: context option "no_block") the STEP-BY-STEP reverse mode runs
 * (celerite_wide.hip: forward pass with checkpoints, replayed segments, lean adjoint kernel since round 4): 40 .. 45 ms at 64 .. 95 rows,
 * 62 .. 157 ms at 96 .. 143 (the reference benchmark grid's j = 64 is 128 rows) at N = 1e4.  More than 143 rows: PIORAN_ERR_UNSUPPORTED.
 * Many chains (round 5): with more than 512 chains, 17 .. 63 rows (round 6: four block columns), shared (c, d), grad_y = grad_sigma2 = NULL (value and
 * d/d(a, b, mu, nu) — what the approx-based models' samplers ask for: (c, d) shared by the chains are fixed by the spectral grid — and, round 6, d/d(c, d) of
 * the shared (c, d): grad_c and grad_d both or neither) the reverse mode
 * with ONE DRAW PER WAVEFRONT runs (celerite_tile.hip): its forward pass keeps only the lower tiles of T per window (7.5 MB per chain at N = 1e4,
 * chunks of 2048 chains under the default workspace limit) and the reverse kernel recomputes the rest — 4096 chains of SHO-20 45.7 ms (56.0 with d/d(c, d);
 * 88 / 100 ms on the small-batch kernels), of DRWCelerite-20 (60 rows) 125 / 154 ms (166 / 175).  Context option "no_tile" keeps every chain count on the small-batch kernels, "scan_config" = "tile" forces the new
 * family from one chain on; config name "tile (windowed gradient, one draw per wavefront)".
 * Memory (step-by-step mode): the forward pass keeps the R x R state only at checkpoints (every ~2 sqrt(N) steps) and the reverse pass replays one
 * segment at a time: ~15 MB of workspace per draw at N = 1e4, J = 20 (two replayed segments + checkpoints 11 MB, stored m / D 4 MB: pioran_grad_workspace_doubles;
 * 55 MB at 80 rows, 105 MB at 128); draws are processed in chunks sized to the free memory.
 * The workspace stays in the context for the next call; pioran_ctx_trim releases it. */
int pioran_celerite_logl_grad(pioran_ds* ds, int64_t B, int64_t J, const double* A, const double* Bc, const double* C,
                              const double* Dd, int cd_shared, const double* mu, const double* nu, double* out,
                              int32_t* status, double* grad_a, double* grad_b, double* grad_c, double* grad_d,
                              double* grad_nu, double* grad_mu, double* grad_y, double* grad_sigma2);
/* The same for the shifted log-flux models (docs/src/turing.md:205-230: c ~ LogUniform(...), y = log.(y .- c),
 * sigma2 = nu sigma.^2 ./ (y .- c).^2): the data set holds the raw flux and yerr^2, the transform runs on the device as in
 * pioran_celerite_logl_batch_shift, and grad_shift [B] = dlogL/dc_b comes out of the series gradients by the chain rule. */
int pioran_celerite_logl_grad_shift(pioran_ds* ds, int64_t B, int64_t J, const double* A, const double* Bc, const double* C,
                                    const double* Dd, int cd_shared, const double* mu, const double* nu, const double* shift,
                                    double* out, int32_t* status, double* grad_a, double* grad_b, double* grad_c,
                                    double* grad_d, double* grad_nu, double* grad_mu, double* grad_shift);
/* log L and its gradient with respect to the SAMPLED parameters in one call: pioran_logpdf_batch_theta's arguments (continuum models 0 and 1, both
 * bases, both normalisations), and out of it
 *   grad_theta [B][P] = dlogL/dtheta_k,  grad_norm [B] = dlogL/dnorm,
 *   grad_nu, grad_mu, grad_shift [B]: each NULL exactly when its input (nu, mu, shift) is NULL,
 *   grad_a, grad_b [B][J] (both or neither; may be NULL): the intermediate dlogL/da_j, dlogL/db_j, for checking.
 * Per chunk of chains approx runs on the device into the buffers the reverse mode reads, the reverse mode is pioran_celerite_logl_grad[_shift]'s for the
 * same (a, b) with the grid's shared (c, d) and grad_c = grad_d = NULL — same kernels, same routing, same out and status —, and the reverse mode of
 * approx (approx_vjp_kernel, csrc/approx.hip) chains its grad_a, grad_b on the device: [B][P + 4] doubles go in and come out instead of [B][2 J] each
 * way and P + 1 host evaluations of approx.  For a draw whose status is not 0 grad_theta / grad_norm chain whatever the reverse mode left in its rows.
 * The chain rule, with p_j = P(f_j) / P(f_0), x = B^-1 p, I = w'x (w_j: the bracket of integral_sho / integral_drwcelerite between f_min and f_max,
 * or f_j pi / sqrt2, 2 pi f_j / 3 for the variance form) and kappa_j = f_j pi / sqrt2 (SHO), f_j pi / 3 (DRWCelerite):
 *   h_j = kappa_j (ga_j + gb_j)   |   kappa_j (ga_j + ga_{J+j} + sqrt3 gb_j),      grad_norm = h'x / I,
 *   xbar = (norm / I) h - (norm / I^2) (h'x) w,   pbar = B^-T xbar (transposed solve on the same LU),
 *   grad_theta_k = sum_j pbar_j p_j (dlog P(f_j)/dtheta_k - dlog P(f_0)/dtheta_k).
 * Continuum + QPO features: pioran_logpdf_batch_theta_qpo_grad below.
 * NULL ds / theta / norm / out / grad_theta / grad_norm, model outside 0 .. 1, basis outside 0 .. 1: PIORAN_ERR_ARG before any GPU call.
 * Host pointers, blocking. */
int pioran_logpdf_batch_theta_grad(pioran_ds* ds, int64_t B, int model, int64_t n_components, int basis, int is_integrated_power,
                                   double f_min, double f_max, double S_low, double S_high, const double* theta, const double* norm,
                                   const double* mu, const double* nu, const double* shift, double* out, int32_t* status,
                                   double* grad_theta, double* grad_norm, double* grad_nu, double* grad_mu, double* grad_shift,
                                   double* grad_a, double* grad_b);
/* The reverse mode of approx alone (what an rrule for `approx` calls; no data set): grad_a, grad_b [B][J] (J = n_components for basis 0,
 * 2 n_components for basis 1) -> grad_theta [B][P], grad_norm [B], by the formulas above.  2 <= n_components <= 256.  NULL ctx or pointer, model or
 * basis out of range: PIORAN_ERR_ARG before any GPU call.  Host pointers, blocking. */
int pioran_approx_vjp_batch(pioran_ctx* ctx, int64_t B, int model, int64_t n_components, int basis, int is_integrated_power,
                            double f_min, double f_max, double S_low, double S_high, const double* theta, const double* norm,
                            const double* grad_a, const double* grad_b, double* grad_theta, double* grad_norm);
/* The reverse mode of approx WITH QPO features (approx_qpo_vjp_kernel, csrc/approx.hip; no data set): 1 <= n_qpo <= 8 features (S0, f0, Q) per draw,
 * qpo [B][n_qpo][3] as in pioran_logpdf_batch_theta; cotangents grad_a, grad_b, grad_c, grad_d [B][Jt], Jt = J + n_qpo (J as above), of the coefficients
 * approx returns -- of grad_c, grad_d only the feature columns are read, the continuum's (c, d) are the grid's -- ->
 *   grad_theta [B][P],  grad_norm [B],  grad_qpo [B][n_qpo][3] = d/d(S0, f0, Q).
 * With p0 = P(f_0; theta), x, w, h, kappa as above, and per feature w0 = 2 pi f0, De = sqrt(4 Q^2 - 1), al = S0 w0 Q / 4:
 *   forward   fa = al / p0, fb = fa / De, c = w0 / (2 Q), d = c De;   I = w'x + [integrated] sum_q (fa_q Ia_q + fb_q Ib_q), Ia, Ib the two brackets of
 *             integral_celerite between f_min and f_max;   a_j = kappa_j x_j norm / I,  A_q = 2 fa_q norm / I,  B_q = 2 fb_q norm / I,  C_q = c_q,  D_q = d_q
 *   reverse   s = norm / I,  T = h'x + sum_q 2 (ga_q fa_q + gb_q fb_q),  grad_norm = T / I,  Ibar = -s T / I,  xbar = s h + Ibar w,  pbar = B^-T xbar,
 *             fabar = 2 s ga_q + [i] Ibar Ia,  fbbar = 2 s gb_q + [i] Ibar Ib,  cbar = gc_q + [i] Ibar (fa dIa/dc + fb dIb/dc),  dbar likewise in d,
 *             fabar += fbbar / De,  Debar = dbar c - fbbar fb / De,  cbar += dbar De,  albar = fabar / p0,
 *             grad_S0 = albar w0 Q / 4,  grad_f0 = 2 pi (albar S0 Q / 4 + cbar / (2 Q)),  grad_Q = albar S0 w0 / 4 - cbar c / Q + Debar 4 Q / De,
 *             grad_theta_k = sum_j pbar_j p_j (dlog P(f_j)/dtheta_k - dlog P(f_0)/dtheta_k) - (sum_q fabar_q fa_q) dlog P(f_0)/dtheta_k.
 * In the variance form ([i] = 0) the features do not enter I but are still scaled by norm / I.  2 <= n_components <= 256.  NULL ctx or pointer, model or
 * basis out of range, n_qpo outside 1 .. 8 (n_qpo = 0: pioran_approx_vjp_batch): PIORAN_ERR_ARG before any GPU call.  Host pointers, blocking. */
int pioran_approx_qpo_vjp_batch(pioran_ctx* ctx, int64_t B, int model, int64_t n_components, int basis, int is_integrated_power,
                                double f_min, double f_max, double S_low, double S_high, const double* theta, const double* norm,
                                int64_t n_qpo, const double* qpo, const double* grad_a, const double* grad_b, const double* grad_c,
                                const double* grad_d, double* grad_theta, double* grad_norm, double* grad_qpo);
/* log L and its gradient with respect to the SAMPLED parameters of a continuum + QPO model in one call: pioran_logpdf_batch_theta's arguments with
 * 1 <= n_qpo <= 8 (n_qpo = 0 is PIORAN_ERR_ARG: pioran_logpdf_batch_theta_grad serves it), and out of it grad_theta [B][P], grad_norm [B],
 * grad_qpo [B][n_qpo][3], grad_nu, grad_mu, grad_shift [B] (each NULL exactly when its input is NULL) and, all eight or none, the coefficients
 * coef_a .. coef_d and their gradients grad_a .. grad_d [B][Jt], for checking.
 * Three steps, as pioran_logpdf_batch_carma_grad: approx_kernel makes the coefficients on the device; they come to the host, where the continuum columns
 * of (c, d) are filled with the grid's values, and go through pioran_celerite_logl_grad[_shift] with (c, d) per draw (cd_shared = 0) -- its routing (the
 * windowed reverse mode with one pair of tables per draw up to 63 rows, each draw a batch of its own step by step up to 143 and for every shifted call),
 * its kernels, its out and status on the same numbers --; approx_qpo_vjp_kernel chains (grad_a .. grad_d) back on the device.  The coefficients and their
 * gradients cross PCIe between the steps ([B][Jt] x 4 doubles each way): accepted, these models run at a handful to a few hundred chains.  Every draw
 * has its own tables; there is no mixed shared / per-draw reverse mode.
 * A draw the reference could not evaluate -- a non-finite theta, norm or feature, f0 <= 0, Q <= 1/2 (a DomainError in convert_feature) -- runs on benign
 * parameters and returns out = -inf, status 3 and exact zeros in every gradient row (its coef_* rows are the benign coefficients).
 * NULL ds / theta / norm / qpo / out / grad_theta / grad_norm / grad_qpo, model or basis outside 0 .. 1, n_components outside 2 .. 256, n_qpo outside
 * 1 .. 8, a gradient whose null-ness differs from its input's, some but not all of the eight [B][Jt] arrays: PIORAN_ERR_ARG; more than 143 rows
 * (2 n_components (SHO) or 3 n_components (DRWCelerite), + 2 n_qpo): PIORAN_ERR_UNSUPPORTED; both before any GPU call.  Host pointers, blocking. */
int pioran_logpdf_batch_theta_qpo_grad(pioran_ds* ds, int64_t B, int model, int64_t n_components, int basis, int is_integrated_power,
                                       double f_min, double f_max, double S_low, double S_high, const double* theta, const double* norm,
                                       const double* mu, const double* nu, const double* shift, int64_t n_qpo, const double* qpo, double* out,
                                       int32_t* status, double* grad_theta, double* grad_norm, double* grad_qpo, double* grad_nu, double* grad_mu,
                                       double* grad_shift, double* coef_a, double* coef_b, double* coef_c, double* coef_d, double* grad_a,
                                       double* grad_b, double* grad_c, double* grad_d);
/* simulate (src/celerite_solver.jl:497-513 -> sim :515-549; rand(f(t, sigma2)) of src/scalable_GP.jl:137-146):
 * realisations y_b = L_b D_b^(1/2) q_b of the GP with kernel (a_b, b_b, c, d) + diag(sigma2) at the times t, from
 * caller-supplied standard-normal draws q [B][N] (the reference draws them with its rng, :528).  y_out [B][N].
 * C, Dd: [J] (cd_shared != 0) or [B][J]. */
int pioran_celerite_simulate(pioran_ctx* ctx, int64_t N, int64_t B, int64_t J, const double* A, const double* Bc,
                             const double* C, const double* Dd, int cd_shared, const double* t, const double* sigma2,
                             const double* q, double* y_out);
/* Posterior draws at new times in O((N + M) R^2) by Matheron's rule (rand(fp, t_pred, 1) of src/scalable_GP.jl:106-112 behind
 * get_ppc_timeseries, src/plots_diagnostics.jl:640-671, without the dense mean and covariance on all N + M points): with f~ a draw of the
 * zero-mean prior on the merged grid T = sort(unique(t, tau)) (times are merged only where they compare equal) and eta_n = sqrt(nu_b sigma2_n) eps_n,
 *     out[b][m] = mu_b + f~_b(tau_m) + k*(tau_m)' K_b^-1 ((y - mu_b) - f~_b(t) - eta_b),   K_b = kernel_b + diag(nu_b sigma2)
 * is a draw of N(mean(fp, tau), cov(fp, tau)), jointly over all of tau: a tau equal to a data time or to another tau gets the same latent value
 * (where the dense covariance is singular).  The chain composes the simulation on T (sigma2 = 0) and the posterior mean on the per-draw series
 * y - f~_b(t) - eta_b, with three streaming kernels between them (celerite_predict.hip); nothing but the normals and the draws crosses the bus.
 * q_data [B][N], q_new [B][M], eps [B][N]: standard normals supplied by the caller (as pioran_celerite_simulate takes its q): of the latent
 * process at the data times, at the new times, and of the measurement noise.  The normal of a tau that coincides with a data time or an earlier tau
 * is not used.  tau: M >= 1 times in any order, out [B][M] in the same order; a non-finite tau: PIORAN_ERR_ARG.
 * mu, nu, shift [B], status [B] may be NULL.  shift: the shifted log-flux models — the data set holds raw flux and yerr^2, draw b conditions on
 * log(y - shift_b) with variances sigma2 / (y - shift_b)^2 (as pioran_celerite_logl_batch_shift) and out is in the transformed scale.
 * status: 0, or 2 with NaN in the draw's row — a non-positive D_n in either factorisation, or y - shift_b <= 0; other draws are unaffected.
 * Routing as predict / simulate: up to 63 rows both on the windowed kernels, to 143 step by step, beyond: PIORAN_ERR_UNSUPPORTED before any upload or
 * allocation.  C, Dd: [J] (cd_shared != 0) or [B][J] (each draw then its own one-draw batch).  Draws go in chunks of at most 256 sized to the free
 * memory.  NULL ds / A .. Dd / tau / q_data / q_new / eps / out, B < 1, J < 1, M < 1: PIORAN_ERR_ARG before any GPU call.  Host pointers, blocking.
 * pioran_celerite_config_name(-1) afterwards: "block (windowed posterior draw)" or "wide (step-by-step posterior draw)". */
int pioran_celerite_rand_posterior(pioran_ds* ds, int64_t B, int64_t J, const double* A, const double* Bc, const double* C,
                                   const double* Dd, int cd_shared, const double* mu, const double* nu, const double* shift,
                                   int64_t M, const double* tau, const double* q_data, const double* q_new, const double* eps,
                                   double* out, int32_t* status);
/* ---- batched Lomb-Scargle periodogram (the per-draw loop of plot_lsp_ppc, src/plots_diagnostics.jl:514-571) --------------------------
 * The generalised Lomb-Scargle periodogram (Zechmeister & Kuerster 2009, time-shift-free form) of B series on one sampling, at F frequencies —
 * what LombScargle.jl evaluates with its defaults fit_mean = true, center_data = true, normalization = :standard:
 *     w_n = yerr_n^-2 / sum yerr^-2  (1/N when yerr is NULL),   omega = 2 pi freq,
 *     C = sum w cos(omega t), S = sum w sin, C^ = sum w cos^2, CS^ = sum w cos sin,   CC = C^ - C^2, SS = (1 - C^) - S^2, CS = CS^ - C S, D = CC SS - CS^2,
 *     y~_b = y_b - sum w y_b when center_data (else y_b),   Y = sum w y~, YY = sum w y~^2 - Y^2,   YC = sum w y~ cos - Y C, YS = sum w y~ sin - Y S,
 *     power[b][f] = (SS YC^2 + CC YS^2 - 2 CS YC YS) / (YY D)   in [0, 1].
 * fit_mean == 0: C, S and Y are taken as zero in CC, SS, CS, YC, YS, YY (the classical periodogram).
 * With fit_mean != 0 the power does not depend on a constant added to a series, and the weighted mean is subtracted before projecting whatever
 * center_data says (the result is the same function of the inputs, evaluated without the cancellation an offset causes).
 * The weights and the cos/sin factors are shared by the draws: a table of w cos, w sin is built once per chunk of frequencies (phase formed in cycles and
 * reduced exactly, so its error does not grow with |omega t|) and the projections are one [B x N].[N x 2F] fp64 matrix product on the matrix cores, the
 * weighted mean subtracted as the series is loaded (centre before projecting); only the powers go to memory.  Results do not depend on how the call is
 * chunked.  t need not be sorted.
 *   t [N], Y [B][N], yerr [N] or NULL, freq [F] in cycles per unit time, power [B][F], status [B] or NULL.
 * PIORAN_ERR_ARG, before any GPU call: NULL ctx / t / Y / freq / power; N < 3, B < 1, F < 1; and in the host form a non-finite t, a freq or yerr
 * that is non-finite or not positive (the device form cannot look at its arrays: such values give NaN there).
 * status[b]: 2, with NaN in the draw's row, for a non-finite value in the series or a series that is constant (YY <= 0; to rounding: YY <= 1e-28 sum w y^2);
 * 0 otherwise.  The other draws of the call are not affected.
 * Degenerate frequencies: a frequency whose D is not positive or not finite gives NaN in its column.  Sampling on a regular grid makes sin(omega t)
 * vanish at multiples of the grid's Nyquist frequency — which is why the reference drops the last point of its frequency grid (:545).
 * Memory: the table of a frequency chunk (2 N doubles per frequency, N and F rounded up to 64: 165 MB at N = 1e4, F = 1000) and, in the host form, the staged series
 * and powers of a draw chunk each take at most half of what the context may newly take ("workspace_limit_mb", the free memory); pioran_ctx_trim
 * releases them.  Context option "ls_tile" (64 / 128) pins the output tile of the product per workgroup (default 64; same results).  "ls_only" is for timing tools ONLY: it
 * runs single phases on the workspace the previous call left, and the powers of a call made while it is set are NOT a result.
 * The host form uploads, runs and downloads chunk by chunk and blocks; the device form takes device pointers and is asynchronous on the context's
 * stream.  pioran_celerite_config_name(-1) afterwards: "periodogram (fp64 matrix product)". */
int pioran_lombscargle_batch(pioran_ctx* ctx, int64_t N, int64_t B, int64_t F, const double* t, const double* Y,
                             const double* yerr, const double* freq, int fit_mean, int center_data, double* power,
                             int32_t* status);
int pioran_lombscargle_batch_dev(pioran_ctx* ctx, int64_t N, int64_t B, int64_t F, const double* dt, const double* dY,
                                 const double* dyerr, const double* dfreq, int fit_mean, int center_data, double* dpower,
                                 int32_t* dstatus);
/* ---- quantiles and means over the draw axis (what every posterior predictive check of the reference ends in: plot_ppc_timeseries,
 * src/plots_diagnostics.jl:805-816; plot_lsp_ppc :547-559; plot_psd_ppc :417-447) --------------------------------------------------------
 * X [B][ldx] holds one draw per row (the layout pioran_celerite_rand_posterior and pioran_lombscargle_batch produce).  Every output column m is
 * reduced over the rows with status 0 (status NULL: all rows) to Q quantiles and a mean.  The value of draw b in column m is formed while loading:
 *     v = X[b][cols ? cols[m] : m];   shift given: v = exp(v + shift[b])  (src/plots_diagnostics.jl:663);
 *     ref, scale given: v = (ref[m] - v) / scale[m]  (the standardised residual of :812).
 * The quantile is Statistics.quantile with its defaults (type 7).  For the K kept values of a column sorted ascending, v[1..K]:
 *     aleph = K p + (1 - p),  j = clamp(trunc(aleph), 1, K - 1),  gamma = clamp(aleph - j, 0, 1),  a = v[j], b = v[j+1]  (K = 1: a = b = v[1]),
 *     q = a + gamma (b - a) where a, b are finite and |a - b| <= 2^-26 max(|a|, |b|), else q = (1 - gamma) a + gamma b,
 * every operation rounded on its own in fp64: the result has the bits of the numpy twin tools/quantiles_proto.py, which is the definition.
 * (The condition on |a - b| is this library's: with it p = 0 and p = 1 return the minimum and the maximum exactly, which the first form alone
 * does not once b - a rounds.)
 * A NaN among the kept values of a column gives NaN in its quantiles and its mean; +-inf sort to the ends and take the second form; K = 0 gives
 * NaN everywhere.  The mean is summed in an order that depends on B and the sorted position only, so neither Mc, cols nor a split of the columns
 * over several calls changes a bit of any output.
 *   X [B][ldx], status [B] or NULL, shift [B] or NULL, cols [Mc] int32 or NULL (any order, repeats allowed; NULL: all M columns, Mc is not read),
 *   ref, scale [Mc] or both NULL, probs [Q] in [0, 1], quant [Q][Mc], mean [Mc] or NULL, kept: one int32 (K) or NULL.
 * A column is sorted inside one workgroup's LDS: B > 4096 is PIORAN_ERR_UNSUPPORTED, before any GPU call.
 * PIORAN_ERR_ARG, before any GPU call: NULL ctx / X / probs / quant; B, M, Q < 1; ldx < M; Mc < 1 with cols; exactly one of ref and scale; a
 * prob outside [0, 1] or NaN; and in the host form a cols entry outside [0, M) or a scale that is zero or not finite (the device form cannot
 * look at its arrays: a column index outside [0, M) reads as NaN there).
 * The host form stages X [B][ldx] in a resident buffer of the context (PIORAN_ERR_ALLOC where it does not fit what the context may take,
 * "workspace_limit_mb"; pioran_ctx_trim releases it) and blocks; the device form takes device pointers for everything but probs, which is
 * on the host and copied, and is asynchronous on the context's stream.  pioran_celerite_config_name(-1) afterwards:
 * "quantiles (sort over draws)". */
int pioran_quantiles_batch(pioran_ctx* ctx, int64_t B, int64_t M, int64_t ldx, const double* X, const int32_t* status,
                           const double* shift, int64_t Mc, const int32_t* cols, const double* ref, const double* scale, int64_t Q,
                           const double* probs, double* quant, double* mean, int32_t* kept);
int pioran_quantiles_batch_dev(pioran_ctx* ctx, int64_t B, int64_t M, int64_t ldx, const double* dX, const int32_t* dstatus,
                               const double* dshift, int64_t Mc, const int32_t* dcols, const double* dref, const double* dscale,
                               int64_t Q, const double* probs, double* dquant, double* dmean, int32_t* dkept);
/* pioran_celerite_rand_posterior with its sink changed: the B draws at tau stay on the device ([B][M] and their status, in buffers of the context
 * that count against "workspace_limit_mb" and are released by pioran_ctx_trim; PIORAN_ERR_ALLOC before any draw is computed where they do not
 * fit), and what comes back are their summaries over the draws with status 0 — the arrays plot_ppc_timeseries draws (src/plots_diagnostics.jl:805-816):
 *   ts_quant [Q][M], ts_mean [M] or NULL: quantiles and mean of the draws at every tau;
 *   Nres > 0: res_quant [Q][Nres], res_mean [Nres] or NULL of (res_ref[k] - draw[res_cols[k]]) / res_scale[k] — with res_cols the positions of the
 *   data times in tau, res_ref = y and res_scale = yerr the standardised residuals of :812 (res_cols NULL: Nres must be M, columns in order);
 *   Nres == 0: no residual summary, the res_* arguments are not read;
 *   status [B] or NULL as pioran_celerite_rand_posterior gives it; kept: the number of draws with status 0, or NULL.
 * backtransform != 0 (needs shift): the summaries are of exp(draw + shift_b), as the reference plots the log-flux models (:663).
 * The draws are the bits pioran_celerite_rand_posterior returns for the same arguments; the reduction is pioran_quantiles_batch's.
 * PIORAN_ERR_ARG / PIORAN_ERR_UNSUPPORTED as the two entries have them, all before any GPU call; Nres < 0 and backtransform without shift
 * are PIORAN_ERR_ARG. */
int pioran_celerite_rand_posterior_summary(pioran_ds* ds, int64_t B, int64_t J, const double* A, const double* Bc, const double* C,
                                           const double* Dd, int cd_shared, const double* mu, const double* nu, const double* shift,
                                           int64_t M, const double* tau, const double* q_data, const double* q_new, const double* eps,
                                           int backtransform, int64_t Q, const double* probs, double* ts_quant, double* ts_mean,
                                           int64_t Nres, const int32_t* res_cols, const double* res_ref, const double* res_scale,
                                           double* res_quant, double* res_mean, int32_t* status, int32_t* kept);
/* ---- the PSD model against its basis-function approximation (sample_approx_model, src/plots_diagnostics.jl:195-213; the prior check
 * run_diagnostics :232-240 and the posterior check plot_psd_ppc :371-487 are reductions of it) ------------------------------------------------
 * For B draws theta [B][P], norm [B] of a continuum model (model 0 = SingleBendingPowerLaw, P = 3; 1 = DoubleBendingPowerLaw, P = 5) and F frequencies,
 * with the grid of `approx` (basis 0 = SHO, power p = 4; 1 = DRWCelerite, p = 6; 2 <= n_components = J <= 256; f0 = f_min / S_low, fM = f_max S_high,
 * sp_j = f0 (fM / f0)^(j / (J - 1)), B_jk = 1 / (1 + (sp_j / sp_k)^p), factorised once per call on the host as pioran_logpdf_batch_theta does):
 *     amp_b = B \ (P_b(sp) / P_b(sp_0))                                                   get_approx_coefficients, src/psd.jl:129-135
 *     psd[b][f] = P_b(freq_f) / P_b(freq_0) * norm_b                                      :202-205 — the normaliser is the model at the FIRST frequency passed
 *     psd_approx[b][f] = sum_j (amp_bj norm_b) / (1 + (freq_f / sp_j)^p)                  :207, src/psd.jl:171-179; j ascending, the power formed by squaring
 *     normalise != 0 (plot_psd_ppc): both divided by integ_b = get_norm_psd(amp_b, sp, f_min, f_max, basis, is_integrated_power)   :404-409
 *     times_f != 0 (plot_f_P): both multiplied by freq_f after that                       :419-420
 *     residuals = psd - psd_approx,   ratios = psd_approx / psd                           :210-211, of the arrays as divided and multiplied
 * every operation rounded on its own in fp64; tools/psd_check_proto.py is the definition.  amplitudes [B][J] and integ [B] (computed whatever
 * `normalise` says) are the amplitudes before any scaling and the normalising integral that pioran_logpdf_batch_theta folds into (a, b).
 * status[b]: 2, with NaN in every output row of the draw (amplitudes and integ included), when a theta or the norm of the draw is not finite, when
 * P_b(freq_0) or P_b(sp_0) is not positive and finite, or, with normalise, when integ_b is zero or not finite; 0 otherwise.  The other draws
 * are not affected, and no output depends on which other outputs are requested or on how the call is chunked.
 *   theta [B][P], norm [B], freq [F] positive and finite (any order), psd / psd_approx / residuals / ratios [B][F] each or NULL,
 *   amplitudes [B][J] or NULL, integ [B] or NULL, status [B] or NULL.
 * Out of scope: QPO features and PowerLaw.  (The CARMA variant plot_psd_ppc_CARMA: pioran_carma_psd_batch / pioran_carma_psd_summary, below.)
 * pioran_psd_check_batch uploads, runs chunk by chunk under "workspace_limit_mb" and downloads, and blocks; pioran_psd_check_batch_dev takes
 * device pointers for every array and is asynchronous on the context's stream (a call with another grid than the previous one waits for the stream first).
 * pioran_psd_check_summary keeps the four arrays in buffers of the context (pioran_ctx_trim releases them; PIORAN_ERR_ALLOC where they do not fit
 * what the context may take) and returns their reductions over the draws with status 0, whose number is `kept`:
 *   quant [4][Q][F], mean [4][F] or NULL: per frequency, the Q quantiles and the mean over the draws of psd, psd_approx, residuals, ratios in this
 *     order (plot_quantiles_approx :93-94, plot_mean_approx :150-151, plot_psd_ppc :446-447) — pioran_quantiles_batch_dev on each [B][F] array,
 *     so the bits of pioran_quantiles_batch applied to what pioran_psd_check_batch returns;
 *   meta [B][8] or NULL: per draw, over the F frequencies, mean, median, min |.|, max |.| of the residuals, then the same four of the ratios
 *     (plot_boxplot_psd_approx :43-51, :72); mean and median (the quantile at 0.5) are pioran_quantiles_batch_dev's on transposed [F][B] copies,
 *     min and max are exact; NaN in the eight entries of a draw with status 2.
 * The quantile kernel sorts a column inside one workgroup: B > 4096 or F > 4096 is PIORAN_ERR_UNSUPPORTED in the summary form, before any GPU call
 * (the array forms have no such limit).
 * PIORAN_ERR_ARG, before any GPU call: NULL ctx / theta / norm / freq; every output NULL (summary: NULL quant or probs); B, F, Q < 1; model, basis or
 * n_components out of range; f_min, f_max, S_low, S_high not positive and finite, or f_min >= f_max; a prob outside [0, 1] or NaN; and in the host
 * forms a freq that is not positive and finite (the device form cannot look at its arrays).
 * pioran_celerite_config_name(-1) afterwards: "psd check (model against approximation)". */
int pioran_psd_check_batch(pioran_ctx* ctx, int64_t B, int model, int64_t n_components, int basis, int is_integrated_power,
                           double f_min, double f_max, double S_low, double S_high, const double* theta, const double* norm,
                           int64_t F, const double* freq, int normalise, int times_f, double* psd, double* psd_approx,
                           double* residuals, double* ratios, double* amplitudes, double* integ, int32_t* status);
int pioran_psd_check_batch_dev(pioran_ctx* ctx, int64_t B, int model, int64_t n_components, int basis, int is_integrated_power,
                               double f_min, double f_max, double S_low, double S_high, const double* dtheta, const double* dnorm,
                               int64_t F, const double* dfreq, int normalise, int times_f, double* dpsd, double* dpsd_approx,
                               double* dresiduals, double* dratios, double* damplitudes, double* dinteg, int32_t* dstatus);
int pioran_psd_check_summary(pioran_ctx* ctx, int64_t B, int model, int64_t n_components, int basis, int is_integrated_power,
                             double f_min, double f_max, double S_low, double S_high, const double* theta, const double* norm,
                             int64_t F, const double* freq, int normalise, int times_f, int64_t Q, const double* probs,
                             double* quant, double* mean, double* meta, int32_t* status, int32_t* kept);
/* ---- CARMA(p, q) models from their sampled parameters (src/CARMA.jl, docs/src/carma.md, log_likelihood(::CARMA, ...) src/celerite_solver.jl:272-282,
 * plot_psd_ppc_CARMA src/plots_diagnostics.jl:832-936) -----------------------------------------------------------------------------------------
 * Orders 1 <= p <= 16, 0 <= q <= p (the constructor's rule, src/CARMA.jl:28-36; outside: PIORAN_ERR_UNSUPPORTED); J = (p + 1) / 2 celerite terms, for
 * odd p the last one real (b = d = 0).  Two input forms:
 *   form 0, quad: qa [B][p], qb [B][q] (NULL for q = 0), the quadratic factors the reference's models sample.  r_alpha = quad2roots(qa) (:201-223) and
 *           beta = roots2coeffs(quad2roots(qb)), formed as the product of the real factors x^2 + qb[k+1] x + qb[k] (x + qb[q-1] for odd q): ascending, monic;
 *   form 1, roots: r_alpha [B][p][2] (re, im), beta [B][q + 1], what CARMA(...) holds and plot_psd_ppc_CARMA receives.
 * norm [B]; is_integrated_power as in CARMA(...).  tools/carma_proto.py is the definition, operation by operation.
 * A draw is REJECTED when a parameter (norm included) is not finite (flag 1); in quad form, when a pair of qa or qb has b^2 - 4c >= 0 — not a conjugate
 * pair, which CARMA_celerite_coefs assumes — (flag 2); when a root has real part >= 0 (flag 3; quad form: of either polynomial, roots form: of r_alpha);
 * or when bounds are given (f_lo = f_hi = 0: none) and check_roots_bounds (src/utils.jl:187-192) fails on r_alpha or, in quad form, on the moving-average
 * roots, as both models of docs/src/carma.md do (flag 4).  The first reason in this order is the flag; 0 = accepted.  Rejected draws never disturb others.
 *
 * pioran_carma_coefs_batch: CARMA_celerite_coefs (:98-143) -> A, Bc, C, Dd [B][J], flags [B] or NULL.  A rejected draw gets (1, 0, 1, 0) in every term.
 * pioran_carma_vjp_batch (quad form): cotangents ga, gb, gc, gd [B][J] of the coefficients -> grad_qa [B][p], grad_qb [B][q] (NULL for q = 0),
 *   grad_norm [B]; the Jacobian applied direction by direction with forward duals, forward quantities recomputed.  Rejected draws (flags 1-3; the entry
 *   takes no bounds) get exact zeros; a zero cotangent gives exact zeros.
 * pioran_carma_psd_batch: evaluate(::CARMA, f) (:150-172) -> psd [B][F] = 2 |beta(iw) / alpha(iw)|^2 norm / CARMA_normalisation(r_alpha, beta), or
 *   4 |.|^2 norm without is_integrated_power; times_f != 0: multiplied by freq_f (plot_f_P).  status [B] or NULL: 3, with NaN in the draw's row, for a
 *   rejected draw.  freq [F] positive and finite.  Chunk by chunk under "workspace_limit_mb": no limit on B or F.
 * pioran_carma_psd_summary: the same array kept on the device and reduced per frequency over the draws with status 0 by the kernel of
 *   pioran_quantiles_batch_dev: quant [Q][F], kept (or NULL) = the number of such draws.  B > 4096: PIORAN_ERR_UNSUPPORTED, before any GPU call.
 * All four take host pointers and block.  PIORAN_ERR_ARG, before any GPU call: NULL ctx or a NULL required array, B / F / Q < 1, form not 0 or 1,
 * bounds that are not finite or not 0 <= f_lo < f_hi (or both 0), a freq that is not positive and finite, a prob outside [0, 1].
 * Timing tools: context option "carma_events" records the event slots 4 | 5 around the kernel(s) of a call (the PSD forms: of its first chunk). */
int pioran_carma_coefs_batch(pioran_ctx* ctx, int64_t B, int p, int q, int form, const double* qa_or_roots, const double* qb_or_beta,
                             const double* norm, int is_integrated_power, double f_lo, double f_hi, double* A, double* Bc, double* C, double* Dd,
                             int32_t* flags);
int pioran_carma_vjp_batch(pioran_ctx* ctx, int64_t B, int p, int q, const double* qa, const double* qb, const double* norm,
                           int is_integrated_power, const double* ga, const double* gb, const double* gc, const double* gd, double* grad_qa,
                           double* grad_qb, double* grad_norm);
int pioran_carma_psd_batch(pioran_ctx* ctx, int64_t B, int p, int q, int form, const double* qa_or_roots, const double* qb_or_beta,
                           const double* norm, int is_integrated_power, double f_lo, double f_hi, int64_t F, const double* freq, int times_f,
                           double* psd, int32_t* status);
int pioran_carma_psd_summary(pioran_ctx* ctx, int64_t B, int p, int q, int form, const double* qa_or_roots, const double* qb_or_beta,
                             const double* norm, int is_integrated_power, double f_lo, double f_hi, int64_t F, const double* freq, int times_f,
                             int64_t Q, const double* probs, double* quant, int32_t* status, int32_t* kept);
/* (qa, qb, norm) -> log L in one call (quad form): pioran_carma_coefs_batch's kernel writes the batch's coefficients where the value bodies read a
 * batch's draws, and the call goes on as pioran_celerite_logl_batch (shift: pioran_celerite_logl_batch_shift) with cd_shared = 0 goes on from there —
 * the same routing, decided from the flags and (b, c, d) the host fetches (one draw, or the same (c, d) in every draw: the shared table; mixed mode
 * where its plan takes the batch; else the per-draw-(c, d) body of pioran_celerite_logl_batch_dev_cd), the same kernels, the same bits.
 * mu, nu, shift [B] or NULL; A_out .. Dd_out [B][J] or NULL: the coefficients.
 * status: as the existing entries (0, 1, 2) plus 3 = rejected by the root checks (above, with the bounds): out = -inf, as the reference's models do with
 * @addlogprob! -Inf; the draw ran on benign coefficients and never disturbs its neighbours.  No other entry of this library returns status 3.
 *
 * pioran_logpdf_batch_carma_grad: ... and the gradient w.r.t. the sampled parameters: grad_qa [B][p], grad_qb [B][q] (NULL for q = 0), grad_norm [B];
 * each of grad_nu, grad_mu, grad_shift [B] is NULL exactly when its input is; grad_a, grad_b, grad_c, grad_d [B][J]: the intermediates, all or none.
 * The coefficients come from the same kernel; the reverse mode is that of pioran_celerite_logl_grad[_shift] with cd_shared = 0 and grad_c / grad_d on
 * these coefficients, with its routing — all draws in one launch of the windowed reverse mode where the shape fits it, one draw as a shared-table call —
 * and pioran_carma_vjp_batch's kernel chains (grad_a .. grad_d) back.  The coefficients and their gradients pass through host memory between the three
 * steps ([B][4 J] doubles each way).  With shift the per-draw reverse mode has no shifted form and the call goes draw by draw, as the existing entry
 * does: a shifted form of the per-draw reverse mode is out of scope.  A rejected draw has status 3, out = -inf and exactly 0.0 in every gradient row. */
int pioran_logpdf_batch_carma(pioran_ds* ds, int64_t B, int p, int q, const double* qa, const double* qb, const double* norm,
                              int is_integrated_power, double f_lo, double f_hi, const double* mu, const double* nu, const double* shift,
                              double* out, int32_t* status, double* A_out, double* Bc_out, double* C_out, double* Dd_out);
int pioran_logpdf_batch_carma_grad(pioran_ds* ds, int64_t B, int p, int q, const double* qa, const double* qb, const double* norm,
                                   int is_integrated_power, double f_lo, double f_hi, const double* mu, const double* nu, const double* shift,
                                   double* out, int32_t* status, double* grad_qa, double* grad_qb, double* grad_norm, double* grad_nu,
                                   double* grad_mu, double* grad_shift, double* grad_a, double* grad_b, double* grad_c, double* grad_d);
/* Name of the kernel configuration a large batch with R active rows (all terms with both rows when R is even) runs on;
 * R == 0: the kernel instantiation the calling thread's last step-by-step launch (throughput or latency layout) actually ran on, as
 * pioran_step_route names it; R == -2: the kernel instantiation of the calling thread's last windowed, tile or time-parallel launch, as
 * pioran_window_route names it ("none" before the first) — after a time-parallel call with a repair pass that is the windowed kernel's, which runs
 * last; any other R < 0: the kernel FAMILY of the
 * calling thread's last launch — "tile" (windowed form, one draw per wavefront: large batches from 49 rows on and batch sizes between the
 * passes of the throughput layouts), "block" (windowed kernel), "block+pd" (with per-draw rows), "block (per-draw tables)", "wide"
 * (latency layout), "scan" (throughput layouts), "fallback", "block (windowed gradient[, per-draw tables])",
 * "wide (step-by-step gradient)", "wide (step-by-step variance)", "periodogram (fp64 matrix product)", "quantiles (sort over draws)",
 * "psd check (model against approximation)" (diagnostics). */
const char* pioran_celerite_config_name(int64_t R);
/* Diagnostics (no GPU needed): the automatic choice between the windowed form with one draw per wavefront (1, "tile") and the other families (0)
 * for a shared-table batch of B draws with R active rows; `pass` = draws per pass of the step-by-step layout of these rows (0 = unknown:
 * returns -1 where the choice depends on it), no_split != 0: option "no_split".  The thresholds come from one sweep (profiles/r05_tile_batch_sweep.txt);
 * tests/test_host.py holds this function against that file, tools/retune_thresholds.py prints both side by side. */
int pioran_tile_choice(int32_t R, int64_t B, int64_t pass, int no_split);
/* Diagnostics (no GPU needed): the slot of the pair workspace that workgroup `id` (in launch order, 0 .. nchunk * ndb - 1) of the tile family's
 * pre-pass fills: *chunk of the nchunk chunks of windows, *draw_block of the ndb blocks of 64 draws.  A bijection.  Workgroups go to the eight XCDs
 * in turn; on the whole eights of chunks, which come first, chunk = id (mod 8) — one L2 reads one eighth of the pair table — and the draw blocks go
 * in groups of four, the workgroups of one chunk and group on ids 8 apart; the nchunk mod 8 last chunks follow on adjacent ids, in the same groups.
 * The kernel calls the same function (csrc/common.h tile_pairs_slot);
 * tests/test_tile_pairs_map_host.py holds it.  PIORAN_ERR_ARG: a count below 1, an id outside the range, a NULL output. */
int pioran_tile_pairs_slot(int64_t id, int64_t nchunk, int64_t ndb, int64_t* chunk, int64_t* draw_block);
/* Diagnostics (no GPU needed): the kernel family a log-likelihood launch takes — shared (c, d) of J terms, n_one_row_terms of them with one row
 * (R = 2 J - n_one_row_terms active rows), B draws of N time stamps, per_draw_series != 0: (y, sigma2) per draw — when every resource it asks
 * for is granted: the table fits, the workspace is within the budget, the time-parallel family's repair pass is available.  `name` receives one of
 * the strings pioran_celerite_config_name(-1) reports after such a launch: "tp", "tile", "block", "scan + block (remainder)", "wide", "scan",
 * "fallback".  `pass` = draws per pass of the step-by-step layout of these rows (0 = unknown: no remainder split; the tile family only where its
 * choice does not depend on it).  `options`: "key=value;key=value" with the keys of pioran_ctx_set_option, NULL or "" for the defaults (the
 * environment is not read).  tp, where not NULL and the family is "tp": {1 the boundary phase as a scan / 0 the walk, padded state rows,
 * segments, steps per segment}; zeros for the other families.  PIORAN_ERR_ARG for inconsistent counts, an unknown key or a NULL name.
 * The rules are csrc/route.hip; tests/test_route.py holds them, tests/test_gpu_route.py holds the launches to them. */
int pioran_value_route(int32_t R, int32_t J, int32_t n_one_row_terms, int64_t B, int64_t N, int per_draw_series, int64_t pass,
                       const char* options, char* name, int name_len, int32_t* tp);
/* Diagnostics (no GPU needed): the same for draws that bring (c, d) of their own in n_per_draw_terms (>= 1) of the terms — what
 * pioran_celerite_logl_batch (cd_shared = 0) does with a batch whose other terms are n_two_row_terms with both rows and n_one_row_terms with one
 * (b = d = 0 in every draw), or, must_run != 0, pioran_logpdf_batch_theta with n_per_draw_terms QPO features on such a continuum; every resource
 * granted.  In the host entry's order: mixed mode where its plan takes the batch (csrc/route.hip mixed_plan: "block+pd", the windowed kernel with
 * per-draw rows, or "scan" / "wide" on a combined table, the last chunk's), else every term per draw (perdraw_form: "block (per-draw tables)",
 * "wide (per-draw tables)", or without tables "scan" / "fallback").  One draw (B = 1) is the shared case to the host entry and not asked here
 * unless must_run.  mixed_chunk, where not NULL: the draws per combined table of mixed mode (also where the windowed kernel is the plan: what the
 * call falls to when that kernel's table cannot be had), 0 where mixed mode is not taken.  PIORAN_ERR_UNSUPPORTED (name ""): must_run and mixed
 * mode refuses the rows.  Under force_fallback mixed mode only loses the windowed kernel: a batch it takes still runs on the scan.  options,
 * name, PIORAN_ERR_ARG: as above; also N above 2^48.  tests/test_route.py, tests/test_gpu_route.py. */
int pioran_value_route_cd(int32_t n_two_row_terms, int32_t n_one_row_terms, int32_t n_per_draw_terms, int64_t B, int64_t N, int per_draw_series,
                          int must_run, const char* options, char* name, int name_len, int64_t* mixed_chunk);
/* Diagnostics (no GPU needed): the plan of the other batched entries — entry = "predict" (pioran_celerite_predict), "predict_var"
 * (pioran_celerite_predict_var), "grad" (pioran_celerite_logl_grad[_shift], pioran_logpdf_batch_theta_grad), "simulate" (pioran_celerite_simulate),
 * "rand_posterior" (pioran_celerite_rand_posterior[_summary]) — for B draws of J terms, n_one_row_terms of them with one row (R = 2 J -
 * n_one_row_terms active rows), every resource granted.  per_draw != 0: (c, d) per draw (cd_shared = 0); gradient only: shift != 0 the shifted
 * log-flux form, want_c / want_d: grad_c / grad_d asked for, series_grads: grad_y or grad_sigma2 asked for.  `name` receives the string
 * pioran_celerite_config_name(-1) reports after the call: "block (windowed ...)", "block (windowed ..., per-draw tables)", "tile (windowed gradient,
 * one draw per wavefront)" or "wide (step-by-step ...)" with ... = prediction, variance, gradient, simulation, posterior draw; for a call with
 * (c, d) per draw whose batch form refuses (more than 63 rows, an option that forbids the windowed kernels, the shifted gradient, an entry without
 * such a form) the name of the one-draw shared calls the entry falls back to.  chunk_cap, where not NULL: the draws per chunk before any memory
 * budget; shrink, where not NULL: 1 where a call short of memory halves its chunk, 0 where it leaves the windowed kernels for the step-by-step ones
 * (shared prediction and simulation).  PIORAN_ERR_UNSUPPORTED (name ""): the entry refuses the rows (143; variance: 64).  options, name,
 * PIORAN_ERR_ARG: as for pioran_value_route; also an unknown entry.  The rule is csrc/route.hip entry_plan; tests/test_route.py holds it,
 * tests/test_gpu_entry_route.py holds the calls to it. */
int pioran_entry_route(const char* entry, int32_t R, int32_t J, int32_t n_one_row_terms, int64_t B, int per_draw, int shift, int want_c, int want_d,
                       int series_grads, const char* options, char* name, int name_len, int64_t* chunk_cap, int* shrink);
/* Diagnostics (no GPU needed): one level below the families — the kernel instantiation a step-by-step launch runs.  family = "scan": the throughput
 * layout (csrc/route.hip scan_plan) for R active rows, standard_rows the row map's kind (0: any; 1: every term has both rows; 2: n_complex two-row
 * terms, then one-row terms), B draws, shared_table != 0: the draws share a table, npd_rows per-draw rows beside it.  family = "value", "store",
 * "simulate" or "gradient": the latency layout's modes (wide_plan) — log-likelihood, factor store of the prediction, simulation, reverse mode — for
 * R rows, npd_rows per-draw rows, per_draw_tables != 0: a table per draw (standard_rows, n_complex, B and shared_table are not read).  `name`
 * receives what pioran_celerite_config_name(0) reports after that launch: the throughput configuration's name with "+win3" on the three-step form
 * ("rpl2_cbr1_nsrc16_p+win3"); "wide_rpl<rows per lane>" (celerite_wide_kernel) or "wide2_rpl<rows per lane>[_y]" (the lean kernel[, y as a
 * vector]), the gradient with "+adjoint" / "+adjoint2" for its reverse pass; "none" where the family refuses (PIORAN_ERR_UNSUPPORTED).  plan, where not
 * NULL, receives 8 integers — scan: {index of the configuration in csrc/scan_configs.h or -1, steps per pass (1, 2, 3), shared table, per-draw rows,
 * y as a vector, pairs per block of the block layout, 1 if celerite_scan.hip holds a kernel for the plan, rows the configuration holds}; latency modes:
 * {rows per lane, lean forward kernel, y as a vector, lean reverse pass, 0 ...}.  options, name, PIORAN_ERR_ARG: as for pioran_value_route; also an
 * unknown family.  tests/test_route.py holds the rules, tests/test_gpu_step_route.py the launches to them. */
int pioran_step_route(const char* family, int32_t R, int32_t standard_rows, int32_t n_complex, int64_t B, int shared_table, int32_t npd_rows,
                      int per_draw_tables, const char* options, char* name, int name_len, int32_t* plan);
/* Diagnostics (no GPU needed): the same for the windowed kernels (csrc/route.hip block_plan), their one-draw-per-wavefront form (tile_plan) and the
 * time-parallel family (tp_step_plan).  `name` receives what pioran_celerite_config_name(-2) reports after that launch, in one-to-one correspondence with
 * the template arguments of the kernels it runs, "none" where the launch is refused (PIORAN_ERR_UNSUPPORTED); plan, where not NULL, receives 12 integers.
 * family = "block" (log-likelihood), "block_grad", "block_solve" (the prediction's K^-1 (y - mu)), "block_sim": R active rows, J terms, B draws,
 * npd_rows per-draw rows (value only), want_cd != 0: the gradient with respect to c or d is asked for; options block_emode and exp are read.  Names:
 * "block_nb<block columns>_e<0 the pair table in one LDS buffer, 1 in two, 2 in global memory>_pd<0 no per-draw rows, 1 a helper wavefront prepares
 * them, 2 the chain wavefront>", the gradient "block_nb2_e0+adjoint[_cd]_<8 | 4 contraction threads per term>", "block_nb2_e0+backsolve",
 * "block_nb2_e0+sim".  plan: {block columns, e, pd, stores (0 none, 1 gradient, 2 solve, 3 simulate), threads per workgroup, dynamic LDS bytes of the
 * forward kernel, cd, contraction threads, 1 if celerite_block.hip holds the kernels, 0 ...}.
 * family = "tile", "tile_grad": R, J, per_draw_series != 0: (y, sigma2) per draw (value only), want_cd.  Names: "tile_nb<block columns>_kl<live K-steps
 * of four rows in the last row block>[_ser]"; "tile_nb<block columns>_kl4_st+adjoint[_cd]_w<draws per workgroup of the adjoint>".  plan: {block
 * columns, kl, a series per draw, cd, draws per workgroup of the adjoint, threads per workgroup of the forward kernel, its dynamic LDS bytes, the
 * adjoint's, 1 if celerite_tile.hip holds the kernels, 0 ...}.
 * family = "tp": tp_rows padded state rows, tp_segments segments, tp_mode the boundary phase's mode (0 the walk, unchecked; 1 the scan, a verification
 * launch and the walk for the draws that fail; 2 the scan, checked by the filter; 4 the walk, checked by the filter); options tp_scan_lean and
 * tp_scan_waves are read.  Names: "tp_np<column pairs per wavefront>x<wavefronts of the element and filter kernels>" and the boundary phase,
 * "+small<2 | 4>", "+wave<6 .. 16>", "+boundary_rt<tiles of 16 rows>" or "+combine[_lean]_rt<tiles>_w<wavefronts>", mode 1 also "+verify_wave<8 | 16>"
 * or "+verify_boundary_rt<tiles>".  plan: {column pairs, wavefronts, boundary phase (1 small, 2 wave, 3 boundary, 4 the scan), its rows (small, wave) or
 * tiles, lean, wavefronts per combination, dynamic LDS bytes of the boundary phase's kernel, verification (0 none, 2 wave, 3 boundary), its rows or
 * tiles, its dynamic LDS bytes, 1 if the filter makes the check, 1 if celerite_tp.hip holds the kernels}.
 * The arguments of the other families are not read.  options, name, PIORAN_ERR_ARG: as for pioran_value_route; also an unknown family.
 * tests/test_route.py holds the rules to what the launch code chose before they existed, tests/test_gpu_window_route.py the launches to them. */
int pioran_window_route(const char* family, int32_t R, int32_t J, int64_t B, int32_t npd_rows, int per_draw_series, int want_cd, int32_t tp_rows,
                        int32_t tp_segments, int tp_mode, const char* options, char* name, int name_len, int32_t* plan);
/* Diagnostics: the FP64 FMA rate (TFLOP/s) the device sustains right now with `waves_per_simd` (1 .. 8) wavefronts on every SIMD — about
 * `ms` milliseconds of a pure stream of independent v_fma_f64, event-timed on the context's stream.  The measured ceiling of any FP64
 * vector kernel on this box at that occupancy (the 78.6 TFLOP/s vendor figure assumes one FMA per SIMD every 4 cycles at 2.4 GHz).
 * Side effects: blocks until the stream has drained; may re-allocate the context's scratch buffer (no call may be in flight on another
 * thread of the same context); uses the context's own event slots, never the caller's 0 .. 11. */
int pioran_ctx_fp64_probe(pioran_ctx* ctx, int waves_per_simd, double ms, double* tflops);

/* ---- in-process farm over several GPUs ---------------------------------------------------------------------------
 * For hosts without a process-per-GPU launcher (a single Julia process driving the 8 GPUs of a node): one context and
 * one resident copy of the data set per listed device, one host thread per device per call.  Draws are independent, so
 * the batch is cut into contiguous shards (the first B % ngpu devices get one more draw) and every device writes its
 * slice of out/status directly — there is no collective.  `devices` may list a device more than once.
 * Arguments of pioran_farm_logl_batch are those of pioran_celerite_logl_batch[_shift] (shift may be NULL);
 * pioran_farm_logl_batch_series takes per-draw series Y, S2 [B][N] instead (the models with a sampled mean FUNCTION, e.g. the
 * sinusoid of examples/ultranest/single_pl_periodicity.jl:115: CustomMean makes y - mean(t) a per-draw series): every device
 * receives the rows of its shard. */
typedef struct pioran_farm pioran_farm;
int pioran_farm_create(int ngpu, const int* devices, int64_t N, const double* t, const double* y,
                       const double* sigma2, pioran_farm** out);
int pioran_farm_destroy(pioran_farm* farm);
int pioran_farm_size(const pioran_farm* farm);
int pioran_farm_logl_batch(pioran_farm* farm, int64_t B, int64_t J, const double* A, const double* Bc,
                           const double* C, const double* Dd, int cd_shared, const double* mu, const double* nu,
                           const double* shift, double* out, int32_t* status);
int pioran_farm_logl_batch_series(pioran_farm* farm, int64_t B, int64_t J, const double* A, const double* Bc,
                                  const double* C, const double* Dd, int cd_shared, const double* mu, const double* nu,
                                  const double* Y, const double* S2, double* out, int32_t* status);

/* ---- dense solver ---------------------------------------------------------------------------- */
/* log_likelihood_direct (src/direct_solver.jl:6-21): builds K_ik = sum_j k_j(|t_i - t_k|) +
 * diag(sigma2) in HBM, Cholesky-factorises it and returns the POSITIVE negative-log-likelihood,
 * like the reference (callers negate, test/test_likelihood.jl:54).  info (may be NULL): 0, or the
 * 1-based index of the first non-positive pivot (LAPACK convention; out is NaN then — the reference
 * throws PosDefException). */
int pioran_dense_nll(pioran_ctx* ctx, int64_t N, int64_t J, const double* a, const double* b,
                     const double* c, const double* d, const double* t, const double* y,
                     const double* sigma2, double* out, int32_t* info);
/* B dense evaluations on one data set (the reference has no batch dimension: one log_likelihood_direct per call).  A, Bc
 * [B][J]; C, Dd [J] (cd_shared != 0) or [B][J]; mu, nu [B] or NULL as in pioran_celerite_logl_batch: y - mu_b, nu_b sigma2.
 * out[b] = +NLL of draw b, info[b] (may be NULL) as above.  The factorisations are independent: up to 32 (fewer when memory is short:
 * one slab of about N^2 doubles each) go through every kernel of the chain in ONE launch (the matrix index is a grid dimension), which is
 * what fills the matrix cores at N of a few thousand — one factorisation alone is a chain of N/64 latency-bound steps (N = 4096, J = 40:
 * 1.65 ms alone, 0.49 ms each in a batch). */
int pioran_dense_nll_batch(pioran_ctx* ctx, int64_t N, int64_t J, int64_t B, const double* A, const double* Bc,
                           const double* C, const double* Dd, int cd_shared, const double* t, const double* y,
                           const double* sigma2, const double* mu, const double* nu, double* out, int32_t* info);
/* Same call with event timing of its phases on the ctx stream: phase_ms[0] covariance build, [1] factorisation (all panel
 * and trailing-update launches), [2] finish kernel — what bench.py reports as the dense path's MFMA utilisation. */
int pioran_dense_nll_timed(pioran_ctx* ctx, int64_t N, int64_t J, const double* a, const double* b,
                           const double* c, const double* d, const double* t, const double* y,
                           const double* sigma2, double* out, int32_t* info, float* phase_ms);
/* predict_cov (src/direct_solver.jl:28-69; cov / std / rand of a PosteriorGP, src/scalable_GP.jl:73-104):
 *     cov_out = K(tau,tau) - K(tau,t) (K(t,t) + diag(sigma2))^-1 K(t,tau),   M x M, symmetric,
 * computed as the Schur complement the blocked MFMA Cholesky of the augmented (N+M) x (N+M) matrix leaves when it stops
 * after the data columns.  info as in pioran_dense_nll (cov_out is NaN when K(t,t) + diag(sigma2) is not PD). */
int pioran_dense_predict_cov(pioran_ctx* ctx, int64_t N, int64_t J, const double* a, const double* b,
                             const double* c, const double* d, const double* t, const double* sigma2, int64_t M,
                             const double* tau, double* cov_out, int32_t* info);
/* predict_direct(cov, tau, t, y, sigma2[, with_covariance]) (src/direct_solver.jl:75-119): the dense posterior mean
 * K(tau,t) (K(t,t) + diag(sigma2))^-1 y from the same partial factorisation (y rides as one more row, as in
 * pioran_dense_nll), and optionally (cov_out != NULL) the covariance of pioran_dense_predict_cov. */
int pioran_dense_predict(pioran_ctx* ctx, int64_t N, int64_t J, const double* a, const double* b,
                         const double* c, const double* d, const double* t, const double* y, const double* sigma2,
                         int64_t M, const double* tau, double* mean_out, double* cov_out, int32_t* info);
/* Covariance build alone (K as N x N column-major host array) — kappa of src/acvf.jl:138-140. */
int pioran_dense_covariance(pioran_ctx* ctx, int64_t N, int64_t J, const double* a, const double* b,
                            const double* c, const double* d, const double* t, const double* sigma2,
                            double* K_out);

#ifdef __cplusplus
}
#endif
#endif /* PIORAN_HIP_H */
