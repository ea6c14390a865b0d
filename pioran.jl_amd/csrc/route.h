// Which kernel family evaluates a batch of log-likelihoods: the measured rules, as pure functions of a RouteQuery (route.hip).  Host code only: no
// runtime call, no context, no data set.  capi.hip fills the query once per launch, asks the rules in the ladder's order (time-parallel, tile,
// windowed, remainder split, scan / latency layout, fallback) and does the rest: tables, workspaces, streams, the launches.  Draws with (c, d) of
// their own are planned before the ladder: mixed_plan where only a few terms differ between the draws, perdraw_form where the caller says all do.
// The other batched entries (prediction, gradient, simulation, posterior draws) have one rule, entry_plan.
// One level down, the step-by-step families name the kernel instantiation a launch runs by the same kind of rule, at the end: scan_plan for the
// throughput layout (celerite_scan.hip), wide_plan for the latency layout (celerite_wide.hip), block_plan for the windowed kernels (celerite_block.hip),
// tile_plan for their one-draw-per-wavefront form (celerite_tile.hip), tp_step_plan for the time-parallel family (celerite_tp.hip).  Those five files
// look the plan's kernels up in a table and launch them; they read no selection option themselves.  pioran_step_route names the first two plans
// without a GPU, pioran_window_route the other three.
#pragma once
#include "common.h"
#include "scan_configs.h"

#include <functional>

// doubles of one step record of the shared table (table.hip): (v, x, phi) of R + 2 rows, then (y_n, sigma2_n)
constexpr int64_t rec_stride_of(int64_t R) { return 3 * (int64_t)(R + 2) + 2; }
// block columns of 16 rows of the windowed kernels (celerite_block.hip, celerite_tile.hip): the R rows and the y row
constexpr int block_columns(int32_t R) { return (R + 1 + 15) / 16; }

// What the rules read of a launch
struct RouteQuery {
    int32_t R, J;                   // active rows, terms
    int64_t B, N;                   // draws, time stamps
    bool shared;                    // the draws share a table (ScanParams::tab)
    int32_t npd_rows;               // per-draw rows (mixed mode)
    bool per_draw_series;           // (Y, S2) per draw
    int32_t n_two_row, n_one_row;   // terms of the prepared state behind the table, by rows kept (0, 0: no such state)
    bool plain_state;               // a prepared state without per-draw terms stands behind the table ...
    bool own_records;               // ... and the launch's step records are that state's own (rec_stride)
    const ScanOptions& opt;
};

// draws per pass of the step-by-step layout that would take the batch (an occupancy query: asked only where a rule needs it)
using PassOf = std::function<int64_t()>;

int tile_choice(int32_t R, int64_t B, int64_t pass, int no_split);
bool tile_wanted(const RouteQuery& q, const PassOf& pass_of);
bool block_wanted(const RouteQuery& q);
enum class ScanFamily { none, wide, scan };
ScanFamily scan_family(const RouteQuery& q);
int64_t split_plan(const RouteQuery& q, const PassOf& pass_of);   // draws on whole passes of the scan (0: no split)

// The time-parallel family's plan: taken or not; the boundary phase as a scan or as the walk; padded state rows, segments, steps per segment
struct TpPlan {
    bool take = false, scan = false;
    int RP = 0, nseg = 0;
    int64_t L = 0;
    int scan_cap = 256;
};
TpPlan tp_plan(const RouteQuery& q);
bool tp_repair_wanted(const RouteQuery& q);                           // may the serial-chain windowed kernel repair the draws that fail the check
int tp_mode(const TpPlan& plan, bool repair, const ScanOptions& o);   // pioran_launch_tp's mode 0 / 1 / 2 / 4; -1: the family refuses the launch

// the family the ladder takes when every resource is granted (pioran_value_route); *tp: the plan, where the family is "tp"
const char* value_route(const RouteQuery& q, int64_t pass, TpPlan* tp);

// Draws that bring (c, d) of their own.  Every term per draw (pioran_celerite_logl_batch_dev_cd, R = 2 J rows): a table per draw for the latency
// kernel, for the windowed kernel, or none — the kernels evaluate the transcendentals themselves, on the ladder above with shared = false
enum class PerDrawForm { no_table, wide_tables, block_tables };
PerDrawForm perdraw_form(const ScanOptions& o, int64_t B, int32_t R, int32_t J);

// A few terms per draw (mixed mode, capi.hip mixed_core): npd of the J terms, `rows` rows in all.  take: mixed mode has the batch (else the caller's
// generic path); windowed: the windowed kernel with per-draw rows is wanted; chunk: the draws per combined table of the scan's leg — also where the
// windowed leg is wanted, for the call whose windowed table cannot be had.  must_run: the caller has no generic path.
struct MixedPlan {
    bool take = false, windowed = false;
    int64_t chunk = 0;
};
MixedPlan mixed_plan(const ScanOptions& o, int64_t B, int64_t N, int32_t J, int32_t rows, int32_t npd, bool must_run);

// what pioran_celerite_config_name(-1) reports after a host call with per-draw (c, d) in npd of the terms, every resource granted
// (pioran_value_route_cd); nullptr: must_run, and mixed mode refuses.  *chunk: the mixed plan's (0: not taken)
const char* value_route_cd(const ScanOptions& o, int32_t n_two_row, int32_t n_one_row, int32_t npd, int64_t B, int64_t N, bool per_draw_series,
                           bool must_run, int64_t* chunk);

// The other batched entries (capi.hip predict_batch, predict_var_shared, logl_grad_batch, simulate_batch, rand_posterior_batch): one rule, entry_plan.
// A body asks it before it prepares its state (per_draw, R = 2 J: refused before any work) and for the prepared state (npd_terms: its terms with
// per-draw rows, which no entry here takes).  grad_flags, gradient only: the shifted log-flux form, d/dc, d/dd, d/dy or d/dsigma2 asked for.
enum class Entry { predict, predict_var, grad, simulate, rand_posterior };
enum { kGradShift = 1, kGradC = 2, kGradD = 4, kGradSeries = 8 };
struct EntryPlan {
    int rc;                  // PIORAN_OK / PIORAN_ERR_UNSUPPORTED
    bool windowed, tile;     // the windowed kernels (celerite_block.hip); of those, the reverse mode with one draw per wavefront (celerite_tile.hip)
    bool shrink;             // short memory: halve the chunk (true) or leave the windowed kernels (false)
    int64_t chunk_cap;       // draws per chunk before any memory budget
    const char* name;        // what pioran_celerite_config_name(-1) reports
    int64_t wide_cap;        // cap and name of the same call step by step: what a shared call falls to where the windowed kernels' table or
    const char* wide_name;   // workspace cannot be had
    void leave_windowed() { windowed = tile = false; shrink = true; chunk_cap = wide_cap; name = wide_name; }
};
EntryPlan entry_plan(Entry entry, int32_t R, int32_t J, int32_t npd_terms, int64_t B, bool per_draw, int grad_flags, const ScanOptions& o);

// what pioran_celerite_config_name(-1) reports after the public entry's call with every resource granted (pioran_entry_route): the batch form's plan,
// or — per_draw and the batch form refuses — the plan of the one-draw shared calls the entry falls back to.  rc PIORAN_ERR_ARG: no such entry
EntryPlan entry_route(const char* entry, int32_t R, int32_t J, int64_t B, bool per_draw, int grad_flags, const ScanOptions& o);

// ---- the step-by-step kernels' instantiations ----------------------------------------------------------------------------------------------------

// A configuration of the throughput layout (scan_configs.h has the list)
struct ScanConfig {
    const char* name;
    int rpl, cbr, nsrc, minw;
    bool paired;
    int npb;
    bool ycol, autopick, preferred;
    // real rows it holds: one slot carries y (unless ycol); a paired config with an odd block keeps one single slot per block
    constexpr int capacity() const
    {
        const int rb = rpl * nsrc;
        if (ycol) return cbr * (paired ? (rb & ~1) : rb);
        return paired ? cbr * (rb & ~1) - ((rb & 1) ? 0 : 1) : rpl * cbr * nsrc - 1;
    }
};
extern const ScanConfig kScanConfigs[kNumScanConfigs];

// What the throughput layout's choice reads of a launch (ScanParams: R, standard_rows, n_complex, B, tab != nullptr, npd_rows, opt)
struct ScanQuery {
    int32_t R, standard_rows, n_complex;
    int64_t B;
    bool shared_tab;
    int32_t npd_rows;
    const ScanOptions* opt;   // nullptr: defaults
};
// The instantiation a launch runs: celerite_scan_kernel<rpl, cbr, nsrc, shared_tab, minw, paired, mixed, npb, form == 2, ycol, form == 3> of
// configuration `config` (-1: none holds the rows — the launch is refused)
struct ScanPlan {
    int config = -1;
    int form = 0;          // steps of the recurrence per pass over T: 1, 2 or 3
    bool shared_tab = false, mixed = false, ycol = false;   // mixed: per-draw rows beside the shared table
    int npb = 0;
    const char* name() const { return config < 0 ? "none" : kScanConfigs[config].name; }
};
ScanPlan scan_plan(const ScanQuery& q);
// what pioran_celerite_config_name(0) reports after the plan's launch: the configuration's name, "+win3" on the three-step form
void scan_plan_name(const ScanPlan& plan, char* buf, size_t len);
bool pioran_scan_kernel_exists(const ScanPlan& plan);   // celerite_scan.hip: its table holds a kernel for the plan

// The latency layout: rows per lane; the forward kernel celerite_wide_kernel or the lean celerite_wide2_kernel, that one in its y-as-a-vector shape
// or not; gradient: the reverse pass on celerite_adjoint_kernel or the lean celerite_adjoint2_kernel
enum class WideMode { value, store, simulate, gradient };
constexpr int kWideMaxRecord = 512;   // staged doubles per step of celerite_wide_kernel: two per thread
struct WidePlan {
    int rc = PIORAN_ERR_UNSUPPORTED;
    int rpl = 0;
    bool lean = false, ycol = false, lean_adjoint = false;
};
WidePlan wide_plan(WideMode mode, int32_t R, int32_t npd_rows, bool per_draw_tables, const ScanOptions* opt);
// its name to pioran_celerite_config_name(0): "wide_rpl3", "wide2_rpl4", "wide2_rpl4_y"; gradient: "+adjoint" / "+adjoint2" behind the forward kernel's
void wide_plan_name(const WidePlan& plan, WideMode mode, char* buf, size_t len);
void pioran_note_wide_launch(const WidePlan& plan, WideMode mode);   // celerite_scan.hip pioran_scan_config_name(0): the thread's last launch was this one

// ---- the windowed, tile and time-parallel kernels' instantiations --------------------------------------------------------------------------------

// celerite_block.hip.  The forward kernel celerite_block_kernel<NB, emode, pdm, st>: NB block columns; emode: where the pair table E lives (0 one LDS
// buffer, 1 two, 2 global memory); pdm: per-draw rows (0 none; 1 a helper wavefront prepares them, 320 threads; 2 the chain wavefront does); st: what
// it stores per window (0 nothing, 1 the reverse pass's operands, 2 the prediction's, 3 the simulation's).  Behind it — gradient:
// celerite_block_adjoint_kernel<NB, cd, tpt> (cd: d/dc or d/dd asked for; tpt: contraction threads per term, 8 up to 32 terms, else 4); solve:
// celerite_block_backsolve_kernel<NB>; simulate: block_sim_xi_kernel<NB> and celerite_block_sim_kernel<NB>.
enum class BlockMode { value, gradient, solve, simulate };
constexpr int kBlockMaxTerms = 64;
constexpr int kBlockMaxPdTerms = 2;
constexpr size_t kBlockLdsMax = 160 * 1024;
struct BlockPlan {
    int rc = PIORAN_ERR_UNSUPPORTED;
    int NB = 0, emode = 0, pdm = 0, st = 0;
    int threads = 0;   // per workgroup of the forward kernel: 256, 320 or 512
    size_t lds = 0;    // ... its dynamic LDS
    bool cd = false;
    int tpt = 0;
};
BlockPlan block_plan(BlockMode mode, int32_t R, int32_t J, int64_t B, int32_t npd_rows, bool want_cd, const ScanOptions* opt);
// "block_nb3_e2_pd0"; gradient "block_nb2_e0+adjoint_cd_8" / "block_nb2_e0+adjoint_4"; "block_nb2_e0+backsolve"; "block_nb2_e0+sim"; "none": refused
void block_plan_name(const BlockPlan& plan, BlockMode mode, char* buf, size_t len);
size_t pioran_block_lds_bytes(int NB, int J, int emode, int npd_terms);    // celerite_block.hip: the forward kernel's dynamic LDS (no runtime call)
bool pioran_block_kernel_exists(const BlockPlan& plan, BlockMode mode);   // ... its tables hold the plan's kernels

// celerite_tile.hip.  Value: celerite_tile_kernel<NB, KL, false, SER> — KL live K-steps of four rows in the last row block, SER: a series per draw.
// Gradient: celerite_tile_kernel<NB, 4, true, false>, then celerite_tile_adjoint_kernel<NB, cd> with adj_waves draws per workgroup and
// tile_pairs_grad_kernel<cd>.
enum class TileMode { value, gradient };
constexpr int kTileMaxTerms = 64;
constexpr int tile_adj_waves_of(int NB, bool cd) { return NB <= 3 ? 4 : (cd ? 2 : 3); }
struct TilePlan {
    int rc = PIORAN_ERR_UNSUPPORTED;
    int NB = 0, KL = 0;
    bool SER = false, cd = false;
    int adj_waves = 0;
};
TilePlan tile_plan(TileMode mode, int32_t R, int32_t J, bool per_draw_series, bool want_cd);
// "tile_nb3_kl2", "tile_nb3_kl2_ser"; gradient "tile_nb3_kl4_st+adjoint_cd_w4" / "tile_nb4_kl4_st+adjoint_w3"; "none": refused
void tile_plan_name(const TilePlan& plan, TileMode mode, char* buf, size_t len);
size_t pioran_tile_lds_bytes(int NB);                    // celerite_tile.hip: the forward kernel's dynamic LDS,
size_t pioran_tile_adj_lds_bytes(int NB, bool cd);      // ... the adjoint's
bool pioran_tile_kernel_exists(const TilePlan& plan, TileMode mode);

// celerite_tp.hip: with which kernels the family runs (whether and how it runs at all: TpPlan, tp_mode above).  tp_element_kernel and
// tp_filter_kernel<NP, NWV>; between them the boundary phase — the walk on tp_boundary_small_kernel<rows> (2 | 4 state rows),
// tp_boundary_wave_kernel<rows> (6 .. 16) or tp_boundary_kernel<4, rt> (rt tiles of 16 rows), or the scan on tp_combine_kernel<rt, tw> /
// tp_combine_lean_kernel<rt, tw> (tw wavefronts per combination); mode 1 only: the verification launch of the scan's kernel and behind it the walk,
// on tp_boundary_wave_kernel<8 | 16> or tp_boundary_kernel<4, rt>, for the draws that fail.
enum class TpPhase { none, small, wave, tiles, scan };
struct TpStepPlan {
    int rc = PIORAN_ERR_UNSUPPORTED;
    int NP = 0, NWV = 0;
    TpPhase boundary = TpPhase::none;
    int rows = 0;                          // small, wave: the template argument
    int rt = 0, tw = 0;                    // tiles, scan: tiles of rows; scan: wavefronts
    bool lean = false;
    size_t lds = 0;                        // dynamic LDS of the boundary phase's kernel
    TpPhase verify = TpPhase::none;        // none, wave or tiles
    int verify_rows = 0, verify_rt = 0;
    size_t verify_lds = 0;
    bool filter_disc = false;              // the filter makes the check on its way (its `disc`)
};
TpStepPlan tp_step_plan(int RP, int nseg, int mode /*pioran_launch_tp's: 0, 1, 2, 4*/, const ScanOptions* opt);
// "tp_np1x1+small2", "tp_np4x1+wave8", "tp_np3x4+boundary_rt2", "tp_np5x4+combine_lean_rt4_w8"; mode 1: "...+verify_wave8" / "...+verify_boundary_rt3"
void tp_step_plan_name(const TpStepPlan& plan, char* buf, size_t len);
bool pioran_tp_kernel_exists(const TpStepPlan& plan);

// The calling thread's last launch of one of these three families (pioran_celerite_config_name(-2)): the launchers note their plan, the name is
// spelled when asked for
void pioran_note_block_launch(const BlockPlan& plan, BlockMode mode);
void pioran_note_tile_launch(const TilePlan& plan, TileMode mode);
void pioran_note_tp_launch(const TpStepPlan& plan);
const char* pioran_window_last_name();
