// The routing rules of the value path and of the other batched entries (route.h): thresholds and time models, each with the measurements it was set
// from.  Pure host functions.
#include "route.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>

// The automatic choice between the windowed form with one draw per wavefront ("tile", 1) and the rest (0: step-by-step throughput layouts / the
// small-batch windowed kernel) for a shared-table batch of B draws with R active rows — a PURE function of its arguments, exported so that
// tests/test_host.py can hold it against the committed sweep (profiles/r05_tile_batch_sweep.txt: the choice must be within 5 % of the faster
// family on every measured line) and tools/retune_thresholds.py can print where it is not.  pass = draws per pass of the step-by-step
// layout that would take the batch (pioran_scan_pass_draws; 0 = not known: -1 is returned where the ladder needs it).
int tile_choice(int32_t R, int64_t B, int64_t pass, int no_split)
{
    if (R >= 49) return B > (R > pioran_block_supported_rows() ? 256 : 512) ? 1 : 0;
    if (R < 17 || B <= 512) return 0;
    if (B <= 1024) return 1;
    if (R < 33) return B <= 2048 ? 1 : 0;   // one round of this kernel's workgroups (2048 draws): SHO-12 1536 / 2048 draws 3.5 / 3.6 against 4.3 / 4.4 ms,
                                          // SHO-16 level (5.3 / 5.4 against 5.4); beyond, the step-by-step layouts' pass (8192 / 4096 draws) is ahead
    if (R >= 39 && R <= 47) return 1;   // three block columns cost the same for 33 .. 47 rows, the step-by-step layouts ~R^2: from 39 rows on this
                                        // kernel is ahead on whole passes too (SHO-20, 4096 draws: 10.7 against 11.4 .. 12.0 ms)
    if (pass <= 0) return -1;
    const int64_t r = B % pass;
    // a remainder of up to one round of the small-batch kernel rides beside the scan (split_plan) where that kernel takes these rows
    const bool split = B > pass && r > 0 && r <= (R <= 47 ? 512 : 256) && !no_split;
    return r > 0 && 4 * r <= 3 * pass && !split ? 1 : 0;
}

// Large shared-table batches: the windowed form with one draw per wavefront (celerite_tile.hip, round 5).  Same table as the windowed
// kernel for small batches.  scan_config = "tile" forces it for any batch size.
bool tile_wanted(const RouteQuery& q, const PassOf& pass_of)
{
    const ScanOptions& o = q.opt;
    const bool force = o.force_tile;
    // measured on N = 1e4 (tools/ab_tile.py, profiles/r05_tile_batch_sweep.txt): from 49 rows on (four block columns and more) it beats the
    // step-by-step layouts at every batch size above the small-batch windowed kernel's range — DRWCelerite-20 (60 rows) 1024 draws 6.3
    // against 7.8 ms, 4096 draws 17.5 against 25.1 ms; SHO-40 (80 rows) 512 draws 10.0 against 13.1 ms, 4096 draws 41.3 against 75.3 ms.
    // Up to 48 rows the throughput layouts (two draws per wavefront) are level with it (SHO-20: 11.2 against 11.4 ms) and stay the default.
    // Up to 38 rows (and at 48) the throughput layouts (two and four draws per wavefront) are level with it or ahead on whole passes (SHO-24, 4096
    // draws: 16.5 against 16.9 ms), well ahead of it below 33 rows (SHO-16, 4096 draws: 5.8 against 10.7 ms) — but their time is a staircase of passes
    // (SHO-20: 4096 draws), and this kernel's steps are a quarter of that (1024 draws: one workgroup per CU): it takes what falls between
    // (profiles/r05_tile_batch_sweep.txt: SHO-20 1024 draws 3.96 against 5.31 ms, 3072 draws 9.3 against 11.0, 5000 draws 14.8 against 16.7;
    // SHO-12 / SHO-16 / SHO-24 at 1024 draws 2.9 / 3.9 / 6.2 against 4.2 / 5.6 / 8.2 ms).
    bool automatic = !o.scan_config[0] && !o.no_tile && !o.no_block && q.shared && q.npd_rows == 0;
    if (automatic) {
        int choice = tile_choice(q.R, q.B, 0, o.no_split ? 1 : 0);
        if (choice < 0) choice = tile_choice(q.R, q.B, pass_of(), o.no_split ? 1 : 0);   // (the occupancy query only where the ladder needs it)
        automatic = choice == 1;
    }
    return (force || automatic) && q.shared && q.npd_rows == 0 && pioran_tile_fits(q.R, q.J) && q.plain_state && q.own_records;
}

// Small shared-table batches without per-draw rows: the windowed kernel (celerite_block.hip), which needs its own table.
bool block_wanted(const RouteQuery& q)
{
    const ScanOptions& o = q.opt;
    const char* cfg = o.scan_config[0] ? o.scan_config : nullptr;
    const bool force = cfg && !std::strcmp(cfg, "block");
    // measured on N = 1e4 (tools/sweep_block.py, tools/sweep_midbatch.py, tools/sweep_block_emode.py): faster than both other kernels
    // up to 512 draws from 6 rows on.  Late round 3: with the pair table read from global memory two workgroups share a CU at three
    // block columns, which moves the crossover up — R = 32 .. 35: 768 draws 4.9 vs 5.4 ms; R = 36 .. 47: 1024 draws 5.3 .. 5.8 vs
    // 5.7 .. 7.5 ms on the throughput shapes.  With four block columns (48 rows and more) the table stays in LDS and 512 draws is the
    // limit (DRWCelerite-20 at 768 draws: 7.8 vs 7.1 ms on the throughput shape, which got faster this round).
    // Round 4: five and six block columns (64 .. 95 rows; value only, one workgroup per CU: up to 256 draws).
    // Late round 4 (tools/scalar_small_j.py, profiles/r04_few_rows.txt): five rows 1.84 -> 1.48 ms at N = 1e4; four and fewer rows stay on the
    // throughput layout (1.42 against 1.47 ms) except for long series — its 20-double step records outgrow the L2 (N = 65536: 13.4 against
    // 9.5 ms up to 256 draws, 11.2 at 512) — and for the scalar call, whose series arrive as per-draw (y, sigma2): N = 8192 1.36 -> 1.25 ms.
    const bool few_rows = q.R < 5 && ((q.N >= 16384 && q.B <= 512) || (q.per_draw_series && q.B == 1 && q.N >= 2048));
    const bool automatic = !cfg && !o.no_block &&
                           (q.R < 5 ? few_rows
                            : q.R > pioran_block_supported_rows()
                                ? q.B <= 256
                                : (q.B <= 512 || (q.B <= 768 && q.R >= 32 && q.R <= 47) || (q.B <= 1024 && q.R >= 36 && q.R <= 47)));
    return (force || automatic) && q.shared && q.npd_rows == 0 && pioran_block_fits_value(q.R, q.J) && q.plain_state && q.own_records;
}

// Register-resident scan: small shared-table batches take the latency layout (celerite_wide.hip, one draw per
// workgroup), everything else the throughput layouts (celerite_scan.hip).  PIORAN_SCAN_CONFIG=wide forces the former
// for any batch size, any other value names a throughput configuration; PIORAN_NO_WIDE=1 disables the former.
ScanFamily scan_family(const RouteQuery& q)
{
    const ScanOptions& o = q.opt;
    const char* cfg = o.scan_config[0] ? o.scan_config : nullptr;
    const bool force_wide = cfg && !std::strcmp(cfg, "wide");
    // (below 16 rows the per-step exchange of the latency layout costs more than the whole step of a throughput layout)
    const bool auto_wide = !cfg && q.B <= pioran_wide_max_batch() && q.R >= 16 && !o.no_wide;
    // 80..95 rows: the throughput layouts do not hold S in registers any more, the latency layout still does
    // (exactly 80 rows with a shared table: the throughput layout holds them with y as a vector — large batches go there: 54 k
    //  instead of 43 k evaluations per second at B = 1024 .. 4096, N = 1e4; at 512 draws the latency layout is still ahead,
    //  39 k vs 27 k: tools/sweep_r80.py)
    const bool y80 = q.R == pioran_scan_supported_rows_shared() && q.shared && q.npd_rows == 0 && !o.no_win2 && (q.B > 768 || o.no_wide);
    const bool only_wide = q.R > pioran_scan_supported_rows() && !o.no_wide && !y80;
    if (q.shared && q.R <= pioran_wide_supported_rows() && (force_wide || auto_wide || only_wide)) return ScanFamily::wide;
    if (q.R > pioran_scan_supported_rows() && !y80) return ScanFamily::none;
    return ScanFamily::scan;
}

// Batches that are not a whole number of passes (round 4).  A throughput launch is a sequence of PASSES — every SIMD of the chip holding as
// many wavefronts as the kernel's registers allow (SHO-20: 2 x 1024 wavefronts x 2 draws = 4096 draws) — and a wavefront walks the whole
// series whatever its pass carries: 4200 draws cost two passes' time less what the scheduler backfills (16.9 against 11.9 ms for 4096).
// Small remainders are what the windowed kernel (celerite_block.hip) is fast at, and its workgroups fit BESIDE a resident scan wavefront
// (205 + 250 registers per SIMD lane pair): so the remainder goes to that kernel on the context's second stream, launched first, while the
// whole passes run on the main stream (capi.hip split_dispatch).
int64_t split_plan(const RouteQuery& q, const PassOf& pass_of)
{
    const ScanOptions& o = q.opt;
    if (o.no_split || o.scan_config[0] || o.no_block || o.force_fallback || !q.shared || q.npd_rows != 0 || q.R < 6 || q.R > 95 ||
        !pioran_block_fits_value(q.R, q.J))
        return 0;
    if (!q.plain_state || !q.own_records) return 0;
    const int64_t pass = pass_of();
    if (pass < 1024) return 0;
    // ONE round of the windowed kernel's workgroups: 512 draws (two workgroups per CU) up to three block columns, 256 with four
    // (tools/sweep_batch_sizes.py, profiles/r04_batch_sizes.txt: SHO-20 4200 draws 16.8 -> 13.1 ms, 4608 16.8 -> 14.8; DRWCelerite-20 4200
    // 32.5 -> 28.6.  A second round no longer hides behind the scan — SHO-20 5000 draws: 19.7 against 16.8 ms in one launch — and neither
    // does sending what exceeds HALF a pass: 2500 draws 11.6 against 10.6 ms; both were measured and are not done.)
    const int64_t rem_max = q.R <= 47 ? 512 : 256;   // (64 .. 95 rows, five / six block columns: a pass of the scan is 1024 .. 2048 draws there)
    int64_t main_n = 0;
    const int64_t k = q.B / pass, r = q.B - k * pass;
    if (k >= 1 && r > 0 && r <= rem_max) main_n = k * pass;
    if (main_n <= 0 || main_n >= q.B) return 0;
    // everything that can refuse is asked BEFORE the second stream gets work: the whole passes must be a launch the scan takes
    RouteQuery whole = q;
    whole.B = main_n;
    return scan_family(whole) == ScanFamily::scan ? main_n : 0;
}

// The time model of the time-parallel family, us (measured at 2 .. 48 rows, tools/ab_tp.py; profiles/r06_time_parallel_scan.txt).
// One step of phases 1 + 3: one wavefront per segment up to 16 rows, four above
static double tp_step_us(int RP) { return RP <= 16 ? 0.7 + RP / 8.0 : 1.0 + RP / 32.0; }
// one combination of the scan
static double tp_combine_us(int RP) { return 8.0 + (double)RP * RP / 50.0; }
// one boundary of the walk (2 / 4 rows: one thread per draw; up to 16: one wavefront, in registers; above: four wavefronts, products on the matrix
// cores, four pivots per barrier)
static double tp_boundary_us(int RP) { return RP == 2 ? 0.6 : (RP == 4 ? 2.0 : (RP <= 16 ? 1.3 + RP * RP / 21.0 : 5.0 + (double)RP * RP / 80.0)); }

// A handful of draws of a long series: the time-parallel evaluation (celerite_tp.hip, round 5) — segments of the series on different CUs instead
// of one serial chain per draw.  scan_config = "tp" forces it wherever it applies (shared (c, d), at most 64 state rows, at most 64 draws).
TpPlan tp_plan(const RouteQuery& q)
{
    TpPlan plan;
    const ScanOptions& o = q.opt;
    if (o.no_tp || (!o.force_tp && (o.scan_config[0] || o.force_tile)) || !q.shared || q.npd_rows != 0 || q.B > 64) return plan;
    if (!q.plain_state) return plan;
    // state rows: the two-row terms first (pairs on even / odd lanes), then the one-row terms, padded to an even count
    const int J = q.n_two_row + q.n_one_row;
    const int nrows = 2 * q.n_two_row + q.n_one_row;
    if (nrows > pioran_tp_supported_rows() || q.N < 64) return plan;
    // The boundary phase as a scan over the segments' elements (tp_combine_kernel, round 6: ceil(log2 nseg) launches of one workgroup per (draw, target)
    // instead of nseg - 1 dependent boundary steps) — up to two draws (nseg targets per draw and level want a CU each), 5 .. 64 state rows (padded to
    // a multiple of 8 for it) — moves every crossover (tools/tp_scan_sweep.py, profiles/r06_time_parallel_scan.txt; one scalar call, PCIe included):
    // 8 / 16 rows from 1024 steps on (N = 1024: 0.146 / 0.172 against 0.159 / 0.211 ms on the serial chain; N = 8192: 0.23 / 0.27 against 1.08 / 1.50),
    // 24 rows from 1536 (0.254 against 0.306), 32 from 2048 (0.32 against 0.42), 40 / 48 from 3072 (0.50 / 0.58 against 0.60 / 0.76; N = 1e4:
    // 0.64 / 0.76 against 1.87 / 2.40; N = 65536: 1.19 / 1.35 against 12.0 / 16.4).
    // (three and four rows — the reference grid's j = 2 — padded to eight: N = 8192 0.19 ms against 0.28 on the one-thread boundary walk; from 2048 steps on)
    const bool scan_rows = (nrows > 4 || (nrows > 2 && q.B <= 2 && (q.N >= 2048 || o.tp_scan > 0))) && nrows <= 64;
    // Three to 32 draws (tools/tp_scan_batch_sweep.py, section 8 of the profile): the combinations of one level want a CU slot each — a CU holds kc = 4 / 2 / 1
    // workgroups of tp_combine_kernel at up to 8 / up to 32 / more rows (its LDS) — so the segment count is the largest power of two with B nseg <= 256 kc
    // (SHO-20, N = 1e4, 4 / 8 draws: 64 / 32 segments 0.76 / 1.06 ms against 1.50 / 1.53 on the walk and 1.85 on the serial chains; 128 segments 1.08 / 2.0).
    const int RPs = (nrows + 7) & ~7, kc = RPs <= 8 ? 4 : (RPs <= 32 ? 2 : 1);
    const bool scan_ok = o.tp_scan != 0 && scan_rows && (o.tp_scan > 0 || q.B <= 2 || (q.B <= 32 && 16 * q.B <= 256 * kc));      // the scan is possible
    bool scan = scan_ok;                                                                                                                      // ... and chosen (below)
    int scan_cap = 256;
    if (scan_ok && q.B > 2) { scan_cap = 16; while (2 * scan_cap * q.B <= 256 * kc && scan_cap < 256) scan_cap *= 2; }
    const int RPw = pioran_tp_padded_rows(nrows);        // rows as the boundary walk pads them (RPs: as the scan does)
    // measured (tools/ab_tp.py sweep, profiles/r05_time_parallel_gpu.txt): with up to 8 draws it beats the serial-chain kernels from 1024 steps on at
    // up to 4 state rows (N = 8192: one SHO term 0.17 against 1.16 ms, two 0.27 against 1.15; there also at 64 draws from 4096 steps on: 0.90
    // against 1.16 ms), from 2048 steps at up to 8 rows (four terms, N = 8192: 0.47 against 1.21), from 4096 at up to 12, from 6144 at up to 16
    // (eight terms: 0.96 against 1.47 ms); with more rows the boundary solves (R^3 each, one after the other) eat the gain (20 terms, N = 1e4:
    // 2.6 against 1.83 ms).
    if (!o.force_tp) {
        const bool few = RPw <= 4 && ((q.B <= 8 && q.N >= 1024) || q.N >= 4096);
        const bool mid = RPw > 4 && q.B <= 8 && q.N >= (RPw <= 8 ? 2048 : (RPw <= 12 ? 4096 : 6144)) && RPw <= 16;
        // 17 .. 64 state rows: the boundary solves cost 14 .. 47 us each (four wavefronts, products and rank-4 updates on the matrix cores, four pivots per barrier), and
        // the gain comes with the length of the series (its time grows like sqrt(N), the serial chain's like N): SHO-12 (24 rows) N = 8192 / 1e4 /
        // 65536 0.84 / 0.93 / 2.4 against 1.45 / 1.77 / 11.6 ms; SHO-20 (40 rows) N = 8192 / 1e4 / 65536 1.39 / 1.54 / 3.9 against 1.50 / 1.83 / 11.9;
        // SHO-24 (48 rows; three block columns on the serial chain) N = 1e4 1.80 against 2.47
        // 49 .. 64 state rows: DRWCelerite-20 (60 rows; four block columns on the serial chain) N = 1e4 2.71 against 2.61 (not chosen), N = 16384 / 65536
        // 3.5 / 7.0 against 4.3 / 19.1 ms; SHO-32 (64 rows; FIVE block columns on the serial chain) N = 8192 / 65536 2.45 / 7.0 against 3.7 / 34.4 ms
        const int64_t nwide = q.R + 1 > 64 ? 6144 : 12288;
        const int64_t nmin12 = RPw <= 24 ? 4096 : (RPw <= 32 ? 5120 : (RPw <= 40 ? 8192 : (RPw <= 48 ? 6144 : nwide)));
        const int64_t nmin8 = RPw <= 24 ? 5120 : (RPw <= 32 ? 6144 : (RPw <= 40 ? 8192 : (RPw <= 48 ? 8192 : nwide)));
        const bool many = RPw > 16 && ((q.B <= 2 && q.N >= nmin12) || (q.B <= 8 && q.N >= nmin8));
        // (49 .. 64 rows, tp_combine_lean_kernel: 56 / 60 rows from 4096 steps on — 0.89 / 1.02 against 1.03 / 1.08 ms; N = 1e4: 1.10 / 1.21 against 2.46 / 2.58;
        //  64 rows, five block columns on the serial chain, from 2048 — 0.89 against 0.98; N = 1e4: 1.21 against 4.6)
        const bool scanned = scan_ok && q.N >= (nrows <= 4 ? 2048 : RPs <= 16 ? 1024 : (RPs <= 24 ? 1536 : (RPs <= 32 ? 2048 : (RPs <= 48 ? 3072 : (q.R + 1 > 64 ? 2048 : 4096)))));
        // three and more draws on the scan: a model of its time (records + two phases of N / nseg steps + one combination per level and the check, in us)
        // against the serial chain's time per step (measured at N = 1e4, resident inputs), taken when it promises 15 % off (up to 8 rows, where the model is
        // optimistic at 32 draws: a quarter) — profiles/r06_time_parallel_scan.txt section 8 has the sweep this was held against at N = 2048 / 4096 / 1e4
        bool scanned_b = false;
        if (scan_ok && q.B > 2) {
            const int RP = RPs;
            const double tau = tp_step_us(RP), tc = tp_combine_us(RP);
            int lv = 0;
            for (int c = scan_cap; c > 1; c >>= 1) ++lv;
            // (17 .. 32 rows: two combinations and eight phase wavefronts share a CU at the cap — measured 1.5 x the steps' time there)
            const double load = RP > 16 && RP <= 32 ? (double)q.B * scan_cap * 4.0 / 1024.0 : 1.0, rp = 1.0 + 0.5 * (load > 1.0 ? load - 1.0 : 0.0);
            double t_scan = 35.0 + rp * tau * (double)q.N / scan_cap + (lv + 1) * tc;
            const double s_chain = RP <= 8 ? 0.127 : (RP <= 24 ? 0.178 : (RP <= 40 ? 0.19 : (RP <= 48 ? 0.24 : (q.R + 1 > 64 ? 0.46 : 0.25))));
            // ~2 % of the prior draws of the SHO models and ~7 % of the models with one-row terms (DRWCelerite) fail the check (profiles/r06_time_parallel_scan.txt
            // section 11), and one failing draw sends the launch through the serial chain as well — its expected share
            t_scan += (1.0 - std::pow(nrows != 2 * J ? 0.93 : 0.98, (double)q.B)) * s_chain * (double)q.N;
            scanned_b = (int64_t)scan_cap * 16 <= q.N && t_scan < (RP <= 8 ? 0.75 : 0.85) * s_chain * (double)q.N;
        }
        // the scan where ITS rule says so (o.tp_scan > 0: wherever possible); else the boundary walk where its rules say so — a batch of 8 draws of SHO-20 that the
        // walk's rule admits is better off there (1.53 ms) than on the scan with its expected repair (0.98 + 57 % x 1.86)
        if (o.tp_scan < 0) scan = q.B <= 2 ? scanned : scanned_b;
        if (!scan && !few && !mid && !many) return plan;
    }
    const int RP = scan ? RPs : RPw;
    // segments: phases 1 + 3 cost tau = tp_step_us per step; phase 2 t2 = tp_boundary_us per boundary: N / nseg tau + nseg t2 is least at sqrt(tau N / t2)
    int nseg = o.tp_segments;
    if (nseg <= 0 && scan) {
        // N / nseg tau + ceil(log2 nseg) t_c, t_c = one combination: powers of two
        const double tau = tp_step_us(RP), tc = tp_combine_us(RP);
        double best = 1e300;
        for (int cand = 8, lv = 3; cand <= scan_cap; cand *= 2, ++lv) {
            const double est = tau * (double)q.N / cand + lv * tc;
            if (est < best && (int64_t)cand * 16 <= q.N) { best = est; nseg = cand; }
        }
        if (nseg <= 0) nseg = 1;
    }
    if (nseg <= 0) {
        const double tau = tp_step_us(RP), t2 = tp_boundary_us(RP);
        nseg = (int)std::lround(std::sqrt(tau * (double)q.N / t2));
    }
    if (nseg < 1) nseg = 1;
    if (nseg > (scan ? 256 : 128)) nseg = scan ? 256 : 128;
    if (scan && q.B > 2 && o.tp_segments <= 0) nseg = scan_cap;
    if ((int64_t)nseg * 16 > q.N) nseg = (int)(q.N / 16);
    const int64_t L = (q.N + nseg - 1) / nseg;
    nseg = (int)((q.N + L - 1) / L);
    plan.take = true; plan.scan = scan; plan.RP = RP; plan.nseg = nseg; plan.L = L; plan.scan_cap = scan_cap;
    return plan;
}

// A draw whose boundary states fail the filter's check (tp_filter_kernel: 1 .. 3 % of the prior draws of the SHO models, 6 .. 8 % of the DRWCelerite models; the scan
// or the walk ALONE is wrong by more than 1e-8 on a few per thousand of the latter — tools/tp_scan_accept.py, tp_walk_accuracy.py) is evaluated again by the
// serial-chain windowed kernel (celerite_block_kernel with ScanParams::only_if: its workgroups leave at once for every draw that passed).
bool tp_repair_wanted(const RouteQuery& q)
{
    const ScanOptions& o = q.opt;
    return !o.tp_walk_repair && !o.tp_unchecked && !o.no_block && pioran_block_fits_value(q.R, q.J) && q.own_records;
}

// (no repair pass available — the windowed kernel's table does not fit, "no_block" — and the walk-repair mode not asked for: the boundary walk instead of the
//  scan; the walk-repair mode's own check, a state discrepancy relative to the state's largest entry, lets bad draws through: tools/tp_scan_metrics.py)
// Late round 6: the boundary WALK is checked and repaired the same way (mode 4) — a long segment's element is no better conditioned than a composite of the scan:
// on prior draws of DRWCelerite-10 the walk alone is off by up to 8e-7 where the serial chain holds 4e-10 (tools/tp_walk_accuracy.py).  Without a repair pass the
// family is not an AUTOMATIC choice any more; forced (scan_config "tp"; options tp_unchecked / tp_walk_repair: tools) it runs unchecked as in round 5.
int tp_mode(const TpPlan& plan, bool repair, const ScanOptions& o)
{
    if (!repair && !o.force_tp) return -1;
    const int mode = repair ? (plan.scan ? 2 : 4) : (plan.scan && o.tp_walk_repair ? 1 : 0);
    if (plan.scan && mode == 0 && plan.nseg > 128) return -1;      // (the segment count was chosen for the scan; the walk's kernels take up to 128)
    return mode;
}

const char* value_route(const RouteQuery& q, int64_t pass, TpPlan* tp)
{
    const ScanOptions& o = q.opt;
    const PassOf pass_of = [pass] { return pass; };
    if (!o.force_fallback) {
        const TpPlan plan = tp_plan(q);
        if (plan.take && tp_mode(plan, tp_repair_wanted(q), o) >= 0) {
            if (tp) *tp = plan;
            return "tp";
        }
        if (tile_wanted(q, pass_of)) return "tile";
        if (block_wanted(q)) return "block";
        if (split_plan(q, pass_of) > 0) return "scan + block (remainder)";
        const ScanFamily f = q.R <= pioran_wide_supported_rows() ? scan_family(q) : ScanFamily::none;
        if (f != ScanFamily::none) return f == ScanFamily::wide ? "wide" : "scan";
    }
    return "fallback";
}

// Every term with (c, d) of its own in every draw (pioran_celerite_logl_batch_dev_cd: R = 2 J rows, no shared table)
PerDrawForm perdraw_form(const ScanOptions& o, int64_t B, int32_t R, int32_t J)
{
    if (o.force_fallback) return PerDrawForm::no_table;
    // More rows than the throughput layouts hold (which evaluate per-draw transcendentals in the kernel): every draw gets its
    // OWN table, built for a chunk of draws at a time, and the lean latency kernel walks it (one draw per workgroup) — the
    // reference benchmark's j = 64 with the reference's call pattern (one random (a, b, c, d) per call,
    // benchmark/benchmarks.jl:74-91): 16 k instead of 0.8 k evaluations per second (any-rank kernel, S in HBM).
    if (R > pioran_scan_supported_rows() && R <= pioran_wide_supported_rows()) return PerDrawForm::wide_tables;
    // Small batches, up to 63 rows: every draw gets its own table of the WINDOWED kernel (celerite_block.hip; one workgroup per
    // (window, draw) builds it: ~8 us per table at N = 1e4, J = 20) instead of evaluating 3 J transcendentals per step and draw inside
    // the throughput layout (14.7 ms per launch at N = 1e4, J = 20 whatever the batch): free Celerite / CARMA terms under a sampler
    // (src/CARMA.jl:98-143).  tools/bench_per_draw_small.py.
    const bool automatic = !o.scan_config[0] && !o.no_block && B <= 768 && R >= 6;
    const bool force = !std::strcmp(o.scan_config, "block");
    return (automatic || force) && pioran_block_fits(R, J) ? PerDrawForm::block_tables : PerDrawForm::no_table;
}

// Mixed mode: when only a few terms really differ between draws (QPO features on top of an approx continuum, src/psd.jl:254-261), the shared
// terms keep using the shared table and only the per-draw terms get per-draw rows.
MixedPlan mixed_plan(const ScanOptions& o, int64_t B, int64_t N, int32_t J, int32_t rows, int32_t npd, bool must_run)
{
    MixedPlan plan;
    if (o.no_mixed && !must_run) return plan;
    // Small batches with one or two per-draw terms (a QPO feature on an approx continuum at a few hundred live points): the windowed kernel with
    // per-draw rows (celerite_block.hip; round 3) — same automatic range as for shared batches (block_wanted), whatever the share of per-draw terms
    const char* cfg = o.scan_config[0] ? o.scan_config : nullptr;
    const bool force = cfg && !std::strcmp(cfg, "block");
    // (fewer than six rows, late round 4, tools/per_draw_few_rows.py: the generic per-draw path took 7.5 ms for 16 draws of ONE term at N = 1e4 —
    //  1.7 ms here; 768 draws 8.2 -> 4.2 ms)
    const bool automatic = !cfg && !o.no_block && (rows >= 6 ? B <= 512 : B <= 768);
    // (force_fallback takes this leg away and nothing else: a batch the plan takes still runs its combined table on the scan)
    const bool windowed = (force || automatic) && !o.force_fallback && npd >= 1 && pioran_block_fits_pd(rows, J, npd);
    // all shared is handled by the caller; many per-draw terms: the generic per-draw path is as good.  must_run: the caller has no generic path
    // to fall back to (theta entry: the continuum's (c, d) exist only as a shared table), so the two "not worth it" cuts — a performance
    // heuristic, not a kernel constraint — are skipped
    const bool any_size = must_run || windowed;
    if (npd == 0 || npd > 8 || (!any_size && npd * 2 > J)) return plan;
    if (rows > pioran_scan_supported_rows()) return plan;
    // combined table: (N + 1) records of the shared rows' doubles + chunk * 2 npd * 3 doubles, addressed with 32-bit byte offsets
    const int64_t rs_shared = rec_stride_of(rows);
    int64_t chunk = ((int64_t)0x7fff0000 / ((N + 1) * 8) - rs_shared) / (6 * (int64_t)npd);
    chunk = chunk > B ? B : (chunk >= 16 ? chunk & ~(int64_t)15 : chunk);
    if (chunk < 1 || (!any_size && chunk < 16)) return plan;   // (fewer than 16 draws per table: not worth it)
    plan.take = true; plan.windowed = windowed; plan.chunk = chunk;
    return plan;
}

const char* value_route_cd(const ScanOptions& o, int32_t n_two_row, int32_t n_one_row, int32_t npd, int64_t B, int64_t N, bool per_draw_series,
                           bool must_run, int64_t* chunk)
{
    const int32_t J = n_two_row + n_one_row + npd;
    *chunk = 0;
    if (must_run || B > 1) {   // (one draw is the shared case to the host entry)
        const int32_t rows = 2 * n_two_row + n_one_row + 2 * npd;
        const MixedPlan plan = mixed_plan(o, B, N, J, rows, npd, must_run);
        if (plan.take) {
            *chunk = plan.chunk;
            if (plan.windowed) return "block+pd";
            // the combined table on the scan, chunk by chunk: the name is the last chunk's
            const RouteQuery last{rows, J, B - (B - 1) / plan.chunk * plan.chunk, N, true, 2 * npd, per_draw_series, 0, 0, false, false, o};
            return scan_family(last) == ScanFamily::wide ? "wide" : "scan";
        }
        if (must_run) return nullptr;
    }
    switch (perdraw_form(o, B, 2 * J, J)) {
        case PerDrawForm::wide_tables: return "wide (per-draw tables)";
        case PerDrawForm::block_tables: return "block (per-draw tables)";
        default: break;
    }
    const RouteQuery q{2 * J, J, B, N, false, 0, per_draw_series, 0, 0, false, false, o};
    return value_route(q, 0, nullptr);
}

// ---- the other batched entries: posterior mean and variance, value and gradient, simulation, posterior draws (route.h entry_plan) -------------------

// [entry][step by step, windowed, windowed with per-draw tables, tile]
static const char* const kEntryNames[5][4] = {
    {"wide (step-by-step prediction)", "block (windowed prediction)", "block (windowed prediction, per-draw tables)"},
    {"wide (step-by-step variance)"},
    {"wide (step-by-step gradient)", "block (windowed gradient)", "block (windowed gradient, per-draw tables)", "tile (windowed gradient, one draw per wavefront)"},
    {"wide (step-by-step simulation)", "block (windowed simulation)", "block (windowed simulation, per-draw tables)"},
    {"wide (step-by-step posterior draw)", "block (windowed posterior draw)"}};

EntryPlan entry_plan(Entry entry, int32_t R, int32_t J, int32_t npd_terms, int64_t B, bool per_draw, int grad_flags, const ScanOptions& o)
{
    const bool grad = entry == Entry::grad, var = entry == Entry::predict_var, has_per_draw = !var && entry != Entry::rand_posterior;
    const bool shift = grad_flags & kGradShift, series = grad_flags & kGradSeries, cd_alike = !(grad_flags & kGradC) == !(grad_flags & kGradD);
    // rows past which an entry refuses (the variance kernels of celerite_predict.hip: 64; posterior draws chain the simulation and the prediction)
    const int32_t predict = pioran_predict_supported_rows(), modes = pioran_wide_supported_rows_modes();
    const int32_t max_rows[5] = {predict, 64, pioran_wide_supported_rows_grad(), modes, std::min(predict, modes)};
    // The windowed kernels (celerite_block.hip) whenever the rows fit them: pioran_block_fits bounds the block columns to four, R <= 63.  scan_config: ANY
    // name held in the string forbids, "block" too — forcing the small-batch VALUE kernel sends these entries step by step — while "tile" does not:
    // set_option clears the string for it and sets force_tile.  (tests/test_route.py pins both.)
    // Prediction (round 3): z = K^-1 (y - mu) from the windowed factorisation and a block back-substitution, then the two Q recurrences segment-parallel
    // — no step-by-step factor, no per-step wave reduction; simulation: the windowed factorisation with its per-window stores, then L applied window by
    // window; gradient, with or without d/d(c, d): 6.3 ms (7.0 with d/d(c, d)) instead of 25 at N = 1e4, J = 20 (series gradients and the shifted
    // log-flux models included).
    const bool windowed = !var && !o.no_block && !o.force_fallback && !o.scan_config[0] && pioran_block_fits(R, J);
    // (c, d) per draw: every draw its own windowed-kernel tables or nothing — there is no step-by-step leg, and the shifted gradient has no such form
    if ((per_draw && (!has_per_draw || shift || !windowed)) || R > max_rows[(int)entry] || npd_terms != 0)
        return {PIORAN_ERR_UNSUPPORTED, false, false, true, 0, "", 0, ""};
    // Gradient of many chains (round 5): the one-draw-per-wavefront reverse mode (celerite_tile.hip) — value and d/d(a, b, mu, nu), since round 6 also
    // d/d(c, d) of the SHARED (c, d) (both or neither), shared series.  Its forward pass keeps the lower tiles of T per window (12 KB at three block
    // columns) and the reverse kernel recomputes the rest, where the small-batch kernels keep 41 KB per window and chain and hold one chain per CU.
    // scan_config = "tile" forces it for any chain count.  From 513 chains on (measured, SHO-20 / SHO-12 at N = 1e4: 512 chains 15.1 / 9.3 ms against
    // the small-batch kernels' 11.0 / 9.2; 640 chains 15.2 / 9.4 against 16.6 / 14.0; 2048 chains 27 / 16 against 44 / 36).
    // (48 .. 63 rows — DRWCelerite-20 is 60: three draws per workgroup there (two with d/d(c, d)); 4096 chains take 126 ms (163 with d/d(c, d)) against
    //  166 (175) in 512-chain launches of the small-batch kernels: tools/ab_tile_grad_nb4.py, profiles/r06_tile_grad_four_block_columns.txt.  Until the
    //  reverse kernel stopped spilling at four block columns — T_k and the window's U operands loaded at the head of their own window instead of a
    //  window ahead — it was 177 (208).)
    const bool tile = grad && !per_draw && windowed && cd_alike && !series && !shift && R <= pioran_tile_grad_supported_rows() &&
                      (o.force_tile || (!o.no_tile && B > 512 && R >= 17));
    // Draws per chunk.  Gradient — tile: whole passes of 2048 (1024) chains, 7.7 GB of T per 1024 chains at N = 1e4, three block columns; windowed: 512
    // chains per launch pair (the forward pass then runs two workgroups per CU, the reverse pass two rounds of one), 256 with per-draw tables; step by
    // step: ~15 MB of workspace per draw at N = 1e4, R = 40.  Every other entry: 256.
    // Short memory: a smaller chunk — but the shared prediction and simulation leave the windowed kernels for the step-by-step ones instead
    const char* const* names = kEntryNames[(int)entry];
    return {PIORAN_OK, windowed, tile, !(windowed && !per_draw && (entry == Entry::predict || entry == Entry::simulate)),
            !grad || per_draw ? 256 : (tile ? 4096 : (windowed ? 512 : 1024)), names[tile ? 3 : (windowed ? (per_draw ? 2 : 1) : 0)], grad ? 1024 : 256, names[0]};
}

EntryPlan entry_route(const char* entry, int32_t R, int32_t J, int64_t B, bool per_draw, int grad_flags, const ScanOptions& o)
{
    static const char* const entries[5] = {"predict", "predict_var", "grad", "simulate", "rand_posterior"};
    int e = 0;
    while (e < 5 && std::strcmp(entry, entries[e])) ++e;
    if (e == 5) return {PIORAN_ERR_ARG, false, false, true, 0, "", 0, ""};
    if (per_draw && B > 1) {   // (one draw is the shared case to the public entry)
        const EntryPlan batch = entry_plan((Entry)e, 2 * J, J, 0, B, true, grad_flags, o);
        if (!batch.rc) return batch;
        B = 1;   // draw by draw (capi.hip each_draw)
    }
    return entry_plan((Entry)e, R, J, 0, B, false, grad_flags, o);
}

// ---- the step-by-step kernels' instantiations (route.h scan_plan, wide_plan) ----------------------------------------------------------------------

#define PIORAN_SCAN_DESC(NAME, RPL, CBR, NSRC, MINW, PAIRED, NPB, YCOL, AUTOPICK, PREFERRED) {#NAME, RPL, CBR, NSRC, MINW, PAIRED, NPB, YCOL, AUTOPICK, PREFERRED},
const ScanConfig kScanConfigs[kNumScanConfigs] = {PIORAN_SCAN_CONFIGS(PIORAN_SCAN_DESC)};
#undef PIORAN_SCAN_DESC

static const ScanOptions kDefaultOptions{};

// y-as-a-vector shapes exist in the two-step form for launches without per-draw rows only
static bool ycol_usable(const ScanConfig& c, const ScanQuery& q, const ScanOptions& o)
{
    if (!c.ycol) return true;
    // (per-draw (c, d) launches evaluate the transcendentals in the kernel: at four rows per lane the two-step form then spills —
    // 19.5 k instead of 42.8 k evaluations per second at j = 32 — so those keep the 80-row step-by-step shape)
    return q.shared_tab && q.npd_rows == 0 && !o.no_win2;
}

// does the block layout of `c` hold this row structure?  (shared table, no per-draw rows)
static bool blocked_fits(const ScanConfig& c, const ScanQuery& q)
{
    if (c.npb == 0) return true;
    const int rb = c.rpl * c.nsrc, nsb = rb - 1 - 2 * c.npb;
    return q.standard_rows == 2 && q.shared_tab && q.npd_rows == 0 && q.n_complex == c.npb * c.cbr && q.R - 2 * q.n_complex <= nsb * c.cbr;
}

// The configuration: the one "scan_config" names, where it holds the launch; else the block layout that fits the row structure; else the first
// preferred one with room for the rows — or, on the standard row map, its paired variant
static int scan_pick(const ScanQuery& q, const ScanOptions& o)
{
    const bool standard_rows = q.standard_rows == 1;
    if (o.scan_config[0]) {
        for (int i = 0; i < kNumScanConfigs; ++i) {
            const ScanConfig& c = kScanConfigs[i];
            if (!std::strcmp(o.scan_config, c.name) && c.capacity() >= q.R && (!c.paired || standard_rows) && blocked_fits(c, q) && ycol_usable(c, q, o))
                return i;
        }
    }
    if (!o.no_paired) {
        for (int i = 0; i < kNumScanConfigs; ++i)
            if (kScanConfigs[i].npb > 0 && kScanConfigs[i].autopick && blocked_fits(kScanConfigs[i], q)) return i;
    }
    int best = -1;
    for (int i = 0; i < kNumScanConfigs && best < 0; ++i) {
        const ScanConfig& c = kScanConfigs[i];
        if (c.preferred && c.autopick && c.capacity() >= q.R && ycol_usable(c, q, o)) best = i;
    }
    if (standard_rows && !o.no_paired) {
        // a paired variant of the same shape (or the smallest paired one that fits) wins when the row map allows it
        for (int i = 0; i < kNumScanConfigs; ++i) {
            const ScanConfig& c = kScanConfigs[i];
            if (c.paired && c.npb == 0 && c.autopick && c.capacity() >= q.R && ycol_usable(c, q, o) &&
                (best < 0 || c.rpl * c.cbr * c.nsrc <= kScanConfigs[best].rpl * kScanConfigs[best].cbr * kScanConfigs[best].nsrc))
                return i;
        }
    }
    return best;
}

ScanPlan scan_plan(const ScanQuery& q)
{
    const ScanOptions& o = q.opt ? *q.opt : kDefaultOptions;
    ScanPlan plan;
    plan.config = scan_pick(q, o);
    if (plan.config < 0) return plan;
    // Mid-size batches: up to 2048 draws the four-draws-per-wavefront shapes of this row range put at most one wavefront on
    // half of the chip's 1024 SIMDs, and the launch takes as long as ONE wavefront needs for the series; two draws per
    // wavefront (rpl2_cbr2_nsrc8: half the columns per lane) is then the faster walk (tools/sweep_midbatch.py, N = 1e4,
    // R = 30: 4.2 instead of 5.3 ms for 768 .. 2048 draws; above 2048 draws the denser shape wins again: 5.3 vs 7.3 ms)
    if (!o.scan_config[0] && q.B <= 2048 && q.R >= 24 && q.R <= 31 && kScanConfigs[plan.config].cbr == 1) plan.config = kScan_rpl2_cbr2_nsrc8;
    const ScanConfig& c = kScanConfigs[plan.config];
    plan.ycol = c.ycol;
    plan.npb = c.npb;
    plan.shared_tab = q.shared_tab;
    plan.mixed = q.shared_tab && q.npd_rows > 0;   // (never with the y-as-a-vector shapes or the block layout: ycol_usable, blocked_fits)
    // two-step form: faster wherever its working set fits the register file (tools/sweep_win2.py: RPL <= 3: +10 .. 24 %;
    // RPL = 4: +4 .. 6 % with a few spilled registers); with RPL = 5 it loses 7 %, so there it runs only when forced
    // (context option "win2")
    plan.form = c.ycol || (c.rpl <= 4 && !o.no_win2) || o.win2 ? 2 : 1;
    if (!c.ycol && c.npb == 0 && (c.rpl == 2 || c.rpl == 3)) {
        // three-step form: measured faster where its row vectors fit the register file — two rows per lane from 13 source lanes on
        // (R = 24 .. 31: 2 .. 6 % at B = 4096, tools/sweep_win3.py); with three rows per lane it spills (SHO-20: 18 % slower) and with
        // one the extra row sums outweigh the saved scalings (10 .. 30 % slower): those run it only when the option asks
        const bool auto3 = c.rpl == 2 && c.cbr == 1 && c.nsrc >= 13 && !(o.no_win3 || o.no_win2 || o.win2) && q.B > 2048;
        if ((o.win3 || auto3) && q.shared_tab && q.npd_rows == 0) plan.form = 3;
    }
    return plan;
}

void scan_plan_name(const ScanPlan& plan, char* buf, size_t len) { std::snprintf(buf, len, "%s%s", plan.name(), plan.form == 3 ? "+win3" : ""); }

// The latency layout's kernels (celerite_wide.hip), as they have been chosen since rounds 3 / 4 — the modes' rules differ, and each is kept as it is:
//  value: the lean form from 48 rows on (tools/sweep_wide.py, N = 8192: R = 48 6.0 -> 5.7 ms, 80 9.1 -> 7.5, 94 9.4 -> 7.6; below that the register
//   copies of celerite_wide_kernel are still cheaper: R = 40 4.8 vs 5.1 ms) unless `no_wide2`, on request (`wide2`), above 95 rows and with per-draw
//   tables whatever the options say; in its y-as-a-vector shape at exactly 16 RPL rows, R % 16 == 0, from 48 rows on, without per-draw rows: one row
//   per lane less;
//  store / simulate: lean at 96 .. 143 rows (round 4), and from 64 rows on (where the windowed kernels end) unless `no_wide2` — only without per-draw
//   tables and per-draw rows; `wide2` does NOT force the lean form here;
//  gradient: the lean reverse pass (celerite_adjoint2_kernel) always from 7 rows per lane on, from 4 unless `no_wide2`, or on `wide2`; the lean FORWARD
//   kernel only from 4 rows per lane, under the same condition (64 .. 95 rows: it is the faster one, 9.0 against 13.1 ms at 80 rows) — so `wide2` below
//   4 rows per lane pairs celerite_wide_kernel with the lean reverse pass.
// Refused: more than 143 rows; a step record longer than the kernels stage (kWideMaxRecord doubles; the gradient's, 768 from 7 rows per lane on); what
// only the lean value kernel does — per-draw tables, more than 95 rows with per-draw rows — in another mode.
WidePlan wide_plan(WideMode mode, int32_t R, int32_t npd_rows, bool per_draw_tables, const ScanOptions* opt)
{
    const ScanOptions& o = opt ? *opt : kDefaultOptions;
    WidePlan plan;
    if (R > 143) return plan;
    plan.rpl = (R + 16) / 16;   // R + 1 slots, the y row's among them, 16 per row of the lanes
    if (mode == WideMode::gradient) {
        if (npd_rows != 0 || 3 * (R + 2) + 2 + 3 * npd_rows + 16 * plan.rpl + 1 > (plan.rpl >= 7 ? 768 : kWideMaxRecord)) return plan;
        plan.lean_adjoint = plan.rpl >= 7 || (plan.rpl >= 4 && !o.no_wide2) || o.wide2;
        plan.lean = plan.rpl >= 4 && plan.lean_adjoint;
        plan.rc = PIORAN_OK;
        return plan;
    }
    if (mode == WideMode::value) {
        plan.lean = o.wide2 || (R >= 48 && !o.no_wide2) || R > 95 || per_draw_tables;
        plan.ycol = plan.lean && R % 16 == 0 && R >= 48 && npd_rows == 0;
        if (plan.ycol) plan.rpl = R / 16;
    } else {
        plan.lean = !per_draw_tables && npd_rows == 0 && (R > 95 || (R >= 64 && !o.no_wide2));
    }
    // celerite_wide_kernel: one shared table, up to 95 rows, the record staged in LDS
    if (!plan.lean && (per_draw_tables || 3 * (R + 2) + 2 + 3 * npd_rows > kWideMaxRecord || R > 95)) return plan;
    plan.rc = PIORAN_OK;
    return plan;
}

void wide_plan_name(const WidePlan& plan, WideMode mode, char* buf, size_t len)
{
    if (plan.rc != PIORAN_OK) { std::snprintf(buf, len, "none"); return; }
    std::snprintf(buf, len, "%s_rpl%d%s%s", plan.lean ? "wide2" : "wide", plan.rpl, plan.ycol ? "_y" : "",
                  mode != WideMode::gradient ? "" : (plan.lean_adjoint ? "+adjoint2" : "+adjoint"));
}

// ---- the windowed kernels (celerite_block.hip) --------------------------------------------------------------------------------------------------------
// Where the pair table E lives (tools/sweep_block_emode.py, N = 1e4, late round 3): one LDS buffer is as fast as two or faster at every size measured
// (SHO-20, 256 draws: 1.92 vs 2.10 ms — the second buffer was worth its LDS in round 2, before the shared block shrank), so two buffers are an option
// only (block_emode = 1) — except with per-draw rows up to 256 draws, where they are taken when they fit; above 256 draws what counts is whether TWO
// workgroups fit a CU — if they do not with E in LDS but do without, E is read from global memory (SHO-20, 512 draws: 2.68 instead of 3.75 ms).
// 64 .. 95 rows (five and six block columns, round 4): value only, no per-draw rows; E in LDS where it fits, else from global memory.
// Per-draw rows: a helper wavefront prepares them where the workgroup has room for one (up to three block columns); above 256 draws there, two
// workgroups of four wavefronts per CU (the chain wavefront prepares the per-draw rows, E comes from global memory) instead of one of five.
// Gradient above 256 chains: the forward pass with two workgroups per CU as well (up to three block columns; exp & 16 switches that off: tools); the
// reverse pass stays at one (its LDS holds two copies of a window's block).
BlockPlan block_plan(BlockMode mode, int32_t R, int32_t J, int64_t B, int32_t npd_rows, bool want_cd, const ScanOptions* opt)
{
    const ScanOptions& o = opt ? *opt : kDefaultOptions;
    BlockPlan plan;
    const int NB = plan.NB = block_columns(R), npd = npd_rows / 2;
    const auto fits = [&](int emode, int workgroups = 1) { return workgroups * pioran_block_lds_bytes(NB, J, emode, npd) <= kBlockLdsMax; };
    const auto take = [&](int emode, int pdm) {
        plan.emode = emode;
        plan.pdm = pdm;
        plan.threads = NB < 4 ? (pdm == 1 ? 320 : 256) : 512;
        plan.lds = pioran_block_lds_bytes(NB, J, emode, pdm ? npd : 0);
        plan.rc = PIORAN_OK;
        return plan;
    };
    if (mode != BlockMode::value) {
        if (npd_rows != 0 || !pioran_block_fits(R, J)) return plan;
        plan.st = (int)mode;
        if (mode == BlockMode::gradient) {
            plan.cd = want_cd;
            plan.tpt = J <= 32 ? 8 : 4;
            if (NB <= 3 && B > 256 && fits(2, 2) && !(o.exp & 16)) return take(2, 0);
        }
        return take(0, 0);
    }
    const int em = o.block_emode;   // diagnostics: force an E mode
    if (npd_rows != 0) {
        if ((npd_rows & 1) || !pioran_block_fits_pd(R, J, npd)) return plan;
        const int helper = NB < 4 ? 1 : 2;
        if (NB < 4 && (em == 2 || (em < 0 && B > 256)) && fits(2, 2)) return take(2, 2);
        if (B <= 256 && fits(1)) return take(1, helper);
        return fits(0) ? take(0, helper) : plan;
    }
    if (!pioran_block_fits_value(R, J)) return plan;
    if (NB >= 5) return fits(0) ? take(0, 0) : (fits(2) ? take(2, 0) : plan);
    if (em == 2 && NB < 4) return take(2, 0);
    if (em == 1 && fits(1)) return take(1, 0);
    if (NB < 4 && em < 0 && B > 256 && !fits(0, 2) && fits(2, 2)) return take(2, 0);
    return fits(0) ? take(0, 0) : plan;
}

void block_plan_name(const BlockPlan& plan, BlockMode mode, char* buf, size_t len)
{
    if (plan.rc != PIORAN_OK) { std::snprintf(buf, len, "none"); return; }
    if (mode == BlockMode::value) std::snprintf(buf, len, "block_nb%d_e%d_pd%d", plan.NB, plan.emode, plan.pdm);
    else if (mode == BlockMode::gradient) std::snprintf(buf, len, "block_nb%d_e%d+adjoint%s_%d", plan.NB, plan.emode, plan.cd ? "_cd" : "", plan.tpt);
    else std::snprintf(buf, len, "block_nb%d_e%d+%s", plan.NB, plan.emode, mode == BlockMode::solve ? "backsolve" : "sim");
}

// ---- one draw per wavefront (celerite_tile.hip) ------------------------------------------------------------------------------------------------------
// NB = ceil((R + 1) / 16) block columns, KL = ceil((R - 16 (NB - 1)) / 4) live K-steps in the last row block (NB = 1: R >= 1, KL >= 1).  The reverse
// mode's forward pass keeps all four K-steps; its adjoint runs four draws per workgroup up to three block columns, three at four (DRWCelerite-20),
// two there with d/d(c, d).
TilePlan tile_plan(TileMode mode, int32_t R, int32_t J, bool per_draw_series, bool want_cd)
{
    TilePlan plan;
    plan.NB = block_columns(R);
    if ((R >> 4) != plan.NB - 1) return plan;   // the kernels' compile-time y block column
    if (mode == TileMode::gradient) {
        if (per_draw_series || J > kTileMaxTerms || R < 1 || R > pioran_tile_grad_supported_rows()) return plan;
        plan.KL = 4;
        plan.cd = want_cd;
        plan.adj_waves = tile_adj_waves_of(plan.NB, want_cd);
    } else {
        if (!pioran_tile_fits(R, J)) return plan;
        plan.KL = (R - 16 * (plan.NB - 1) + 3) / 4;
        plan.SER = per_draw_series;
    }
    plan.rc = PIORAN_OK;
    return plan;
}

void tile_plan_name(const TilePlan& plan, TileMode mode, char* buf, size_t len)
{
    if (plan.rc != PIORAN_OK) std::snprintf(buf, len, "none");
    else if (mode == TileMode::value) std::snprintf(buf, len, "tile_nb%d_kl%d%s", plan.NB, plan.KL, plan.SER ? "_ser" : "");
    else std::snprintf(buf, len, "tile_nb%d_kl4_st+adjoint%s_w%d", plan.NB, plan.cd ? "_cd" : "", plan.adj_waves);
}

// ---- the time-parallel family's kernels (celerite_tp.hip) --------------------------------------------------------------------------------------------
// Element and filter kernels: one wavefront per segment and two rows per step of NP up to 12 state rows, four wavefronts and eight rows above (at 16
// rows four are 9 % ahead of one).  The boundary phase as a scan — modes 1 and 2, from two segments on, where pioran_tp_scan_rows — on the lean
// combination at four tiles of rows (only that one fits the LDS) or on request (tp_scan_lean: tests), with eight wavefronts per combination from 17
// rows on (three tiles of rows: nine product tiles and eight column tiles per elimination round — 48.9 -> 40.2 us; four tiles, lean: sixteen and
// twelve) unless tp_scan_waves = 4.  Mode 2 leaves the check to the filter (the caller repairs the draws that fail it: capi.hip tp_dispatch), and so
// does mode 4 behind its walk; mode 1 verifies with one more launch of the scan's kernel and walks the draws that fail.
TpStepPlan tp_step_plan(int RP, int nseg, int mode, const ScanOptions* opt)
{
    const ScanOptions& o = opt ? *opt : kDefaultOptions;
    TpStepPlan plan;
    if (RP < 2 || RP > 64 || RP != pioran_tp_padded_rows(RP) || nseg < 1) return plan;
    plan.NP = RP <= 12 ? RP / 2 : RP / 8;
    plan.NWV = RP <= 12 ? 1 : 4;
    const int rt = (RP + 15) / 16;
    // the walk: two or four rows per thread of a wavefront's 64 draws, one wavefront per draw up to 16 rows, four wavefronts and rt tiles above
    const auto walk = [&](TpPhase& phase, int& rows, int& tiles, size_t& lds) {
        const size_t r16 = (size_t)rt * 16;
        if (RP <= 4) { phase = TpPhase::small; rows = RP; }
        else if (RP <= 16) { phase = TpPhase::wave; rows = RP; }
        else { phase = TpPhase::tiles; tiles = rt; lds = (r16 * (2 * r16 + 3) + 2 * r16 * (r16 + 1) + 192 + 1024) * sizeof(double); }
    };
    plan.filter_disc = mode == 4;
    if (mode != 0 && mode != 4 && nseg >= 2 && pioran_tp_scan_rows(RP)) {
        const size_t r16 = (size_t)rt * 16;
        plan.boundary = TpPhase::scan;
        plan.rt = rt;
        plan.lean = rt == 4 || o.tp_scan_lean;
        plan.tw = rt >= 2 && o.tp_scan_waves != 4 ? 8 : 4;
        plan.lds = plan.lean ? (r16 * (3 * r16 + 3) + r16 * (r16 + 1) + 7 * 64 + 32 + 256 * plan.tw) * sizeof(double)
                             : (r16 * (3 * r16 + 3) + 4 * r16 * (r16 + 1) + 7 * 64 + 256 * plan.tw) * sizeof(double);
        if (mode == 2) plan.filter_disc = true;
        else walk(plan.verify, plan.verify_rows, plan.verify_rt, plan.verify_lds);
    } else {
        walk(plan.boundary, plan.rows, plan.rt, plan.lds);
    }
    plan.rc = PIORAN_OK;
    return plan;
}

void tp_step_plan_name(const TpStepPlan& plan, char* buf, size_t len)
{
    if (plan.rc != PIORAN_OK) { std::snprintf(buf, len, "none"); return; }
    int n = std::snprintf(buf, len, "tp_np%dx%d", plan.NP, plan.NWV);
    const auto add = [&](const char* prefix, TpPhase phase, int rows, int rt) {
        if (n < 0 || (size_t)n >= len) return;
        if (phase == TpPhase::small) n += std::snprintf(buf + n, len - n, "+%ssmall%d", prefix, rows);
        else if (phase == TpPhase::wave) n += std::snprintf(buf + n, len - n, "+%swave%d", prefix, rows);
        else if (phase == TpPhase::tiles) n += std::snprintf(buf + n, len - n, "+%sboundary_rt%d", prefix, rt);
        else if (phase == TpPhase::scan) n += std::snprintf(buf + n, len - n, "+combine%s_rt%d_w%d", plan.lean ? "_lean" : "", rt, plan.tw);
    };
    add("", plan.boundary, plan.rows, plan.rt);
    add("verify_", plan.verify, plan.verify_rows, plan.verify_rt);
}

// the calling thread's last launch of these three families
namespace {
struct LastWindowLaunch {
    int family = 0;   // 0 none yet, 1 block, 2 tile, 3 tp
    int mode = 0;
    BlockPlan block;
    TilePlan tile;
    TpStepPlan tp;
};
thread_local LastWindowLaunch g_last_window;
}  // namespace
void pioran_note_block_launch(const BlockPlan& plan, BlockMode mode) { g_last_window.family = 1; g_last_window.mode = (int)mode; g_last_window.block = plan; }
void pioran_note_tile_launch(const TilePlan& plan, TileMode mode) { g_last_window.family = 2; g_last_window.mode = (int)mode; g_last_window.tile = plan; }
void pioran_note_tp_launch(const TpStepPlan& plan) { g_last_window.family = 3; g_last_window.tp = plan; }
const char* pioran_window_last_name()
{
    static thread_local char buf[96];
    const LastWindowLaunch& l = g_last_window;
    if (l.family == 1) block_plan_name(l.block, (BlockMode)l.mode, buf, sizeof(buf));
    else if (l.family == 2) tile_plan_name(l.tile, (TileMode)l.mode, buf, sizeof(buf));
    else if (l.family == 3) tp_step_plan_name(l.tp, buf, sizeof(buf));
    else std::snprintf(buf, sizeof(buf), "none");
    return buf;
}
