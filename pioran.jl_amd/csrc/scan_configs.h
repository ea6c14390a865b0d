// The configurations of the throughput layout (celerite_scan.hip), described ONCE: route.hip builds the table the rule scan_plan reads from this
// list, celerite_scan.hip the table of kernel pointers, in the same order.
//   X(name, rpl, cbr, nsrc, minw, paired, npb, ycol, autopick, preferred)
// rpl rows per lane, cbr column blocks (DPP rows) per draw, nsrc source lanes per block, minw the kernel's __launch_bounds__ minimum;
// paired: the column-paired variant, needs the standard row map (every term has both rows);
// npb > 0: block layout for "n_complex = npb * cbr two-row terms, then one-row terms" (standard_rows == 2);
// ycol: y rides as a separate vector (kernel template YC): every slot is a row; two-step form, shared table, no per-draw rows;
// autopick false: only selectable by name (measured slower than the default of its row range);
// preferred: a candidate of the automatic choice — in the list's order the first preferred entry whose capacity >= R wins (unless the context
// option "scan_config" names another, or a paired / block-layout variant applies).
// Every entry uses the DPP-folded column blocks (PairFirst / PairSecond); the compiler-scheduled builtin
// variants of round 1 were dropped when the DPP-folded ones became the faster choice in every row range
// (SHO-30: 140 k vs 116 k evals/s, SHO-39: 60 k vs 52 k; profiles/r02_scan_variants.txt).
#pragma once

#define PIORAN_SCAN_CFG(X, RPL, CBR, NSRC, MINW, PREF) X(rpl##RPL##_cbr##CBR##_nsrc##NSRC, RPL, CBR, NSRC, MINW, false, 0, false, true, PREF)
#define PIORAN_SCAN_CFG_P(X, RPL, CBR, NSRC, MINW) X(rpl##RPL##_cbr##CBR##_nsrc##NSRC##_p, RPL, CBR, NSRC, MINW, true, 0, false, true, false)
#define PIORAN_SCAN_CFG_Y(X, RPL, CBR, NSRC, MINW) X(rpl##RPL##_cbr##CBR##_nsrc##NSRC##_y, RPL, CBR, NSRC, MINW, false, 0, true, true, true)
#define PIORAN_SCAN_CFG_YP(X, RPL, CBR, NSRC, MINW) X(rpl##RPL##_cbr##CBR##_nsrc##NSRC##_yp, RPL, CBR, NSRC, MINW, true, 0, true, true, false)

#define PIORAN_SCAN_CONFIGS(X)                                                                                                                       \
    /* (the _y entries: y as a separate vector, one more row than the shape otherwise holds — R = 16, 32, 48, 64 are the reference                \
        benchmark's j = 8, 16, (24,) 32, benchmark/benchmarks.jl:16-18; shared-table launches only) */                                            \
    PIORAN_SCAN_CFG(X, 1, 1, 5, 1, true) PIORAN_SCAN_CFG(X, 1, 1, 9, 1, true) PIORAN_SCAN_CFG(X, 1, 1, 13, 1, true)                                 \
    PIORAN_SCAN_CFG(X, 1, 1, 16, 1, true)                                              /* R <= 15 */                                               \
    PIORAN_SCAN_CFG_Y(X, 1, 1, 16, 1)                                                  /* R = 16 */                                                \
    PIORAN_SCAN_CFG(X, 2, 1, 9, 1, true) PIORAN_SCAN_CFG(X, 2, 1, 11, 1, true) PIORAN_SCAN_CFG(X, 2, 1, 13, 1, true)                                \
    PIORAN_SCAN_CFG(X, 2, 1, 15, 1, true) PIORAN_SCAN_CFG(X, 2, 1, 16, 1, true)        /* R <= 31 */                                               \
    PIORAN_SCAN_CFG_Y(X, 2, 1, 16, 1)                                                  /* R = 32 */                                                \
    PIORAN_SCAN_CFG(X, 3, 2, 6, 1, true) PIORAN_SCAN_CFG(X, 3, 2, 7, 1, true) PIORAN_SCAN_CFG(X, 3, 2, 8, 1, true)   /* R <= 47 */                  \
    PIORAN_SCAN_CFG_Y(X, 3, 2, 8, 1)                                                   /* R = 48 */                                                \
    PIORAN_SCAN_CFG(X, 4, 4, 4, 2, true)                                               /* R <= 63: 256 registers/lane, 2 waves per SIMD */         \
    PIORAN_SCAN_CFG_Y(X, 4, 4, 4, 2)                                                   /* R = 64: y as a separate vector */                        \
    PIORAN_SCAN_CFG(X, 5, 4, 4, 1, true)                                               /* R <= 79 */                                               \
    PIORAN_SCAN_CFG_Y(X, 5, 4, 4, 1)                                                   /* R = 80 (SHO-40: the dense configuration's model) */      \
    /* column-paired variants (standard row map only; picked automatically by scan_plan when applicable) */                                       \
    PIORAN_SCAN_CFG_P(X, 3, 2, 7, 1) PIORAN_SCAN_CFG_P(X, 3, 2, 8, 1) PIORAN_SCAN_CFG_P(X, 3, 2, 6, 1)                                              \
    PIORAN_SCAN_CFG_P(X, 1, 1, 5, 1) PIORAN_SCAN_CFG_P(X, 1, 1, 9, 1) PIORAN_SCAN_CFG_P(X, 1, 1, 13, 1) PIORAN_SCAN_CFG_P(X, 1, 1, 16, 1)           \
    PIORAN_SCAN_CFG_P(X, 2, 1, 9, 1) PIORAN_SCAN_CFG_P(X, 2, 1, 11, 1) PIORAN_SCAN_CFG_P(X, 2, 1, 13, 1) PIORAN_SCAN_CFG_P(X, 2, 1, 15, 1)          \
    PIORAN_SCAN_CFG_P(X, 2, 1, 16, 1)                                                                                                                \
    PIORAN_SCAN_CFG_P(X, 4, 4, 4, 2)                                                                                                                 \
    PIORAN_SCAN_CFG_YP(X, 4, 4, 4, 2) PIORAN_SCAN_CFG_P(X, 5, 4, 4, 1)                                                                              \
    PIORAN_SCAN_CFG_YP(X, 1, 1, 16, 1) PIORAN_SCAN_CFG_YP(X, 2, 1, 16, 1) PIORAN_SCAN_CFG_YP(X, 3, 2, 8, 1) PIORAN_SCAN_CFG_YP(X, 5, 4, 4, 1)       \
    /* DRWCelerite with 20 components: 20 complex + 20 real terms = 5 pairs + 5 singles + 1 spare in each of the 4 blocks */                      \
    X(rpl4_cbr4_nsrc4_b5a, 4, 4, 4, 2, false, 5, false, true, false)                                                                                \
    /* alternatives kept for tuning runs (selected by name) */                                                                                    \
    PIORAN_SCAN_CFG(X, 3, 4, 4, 1, false) PIORAN_SCAN_CFG(X, 2, 2, 8, 1, false)

// index of every configuration in the list: kScan_<name>
#define PIORAN_SCAN_ID(NAME, ...) kScan_##NAME,
enum ScanConfigId : int { PIORAN_SCAN_CONFIGS(PIORAN_SCAN_ID) kNumScanConfigs };
#undef PIORAN_SCAN_ID
