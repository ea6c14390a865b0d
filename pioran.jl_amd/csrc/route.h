// Which kernel family evaluates a batch of log-likelihoods: the measured rules, as pure functions of a RouteQuery (route.hip).  Host code only: no
// runtime call, no context, no data set.  capi.hip fills the query once per launch, asks the rules in the ladder's order (time-parallel, tile,
// windowed, remainder split, scan / latency layout, fallback) and does the rest: tables, workspaces, streams, the launches.  Draws with (c, d) of
// their own are planned before the ladder: mixed_plan where only a few terms differ between the draws, perdraw_form where the caller says all do.
// The other batched entries (prediction, gradient, simulation, posterior draws) have one rule, entry_plan.
// One level down, the step-by-step families name the kernel instantiation a launch runs by the same kind of rule, at the end: scan_plan for the
// throughput layout (celerite_scan.hip), wide_plan for the latency layout (celerite_wide.hip).  Those files look the plan's kernel up in a table
// and launch it; they read no selection option themselves.  pioran_step_route names both plans without a GPU.
#pragma once
#include "common.h"
#include "scan_configs.h"

#include <functional>

// doubles of one step record of the shared table (table.hip): (v, x, phi) of R + 2 rows, then (y_n, sigma2_n)
constexpr int64_t rec_stride_of(int64_t R) { return 3 * (int64_t)(R + 2) + 2; }

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
