"""CPU tests of the routing rules of the value path (csrc/route.hip) through pioran_value_route: the family the ladder of capi.hip's launch()
takes when every resource is granted.  Routes the GPU tests already assert, transcribed; properties over a grid of ~89 000 queries; the
time-parallel plans against the conditions pioran_launch_tp refuses on.  Likewise pioran_value_route_cd for draws with (c, d) of their own, and
pioran_entry_route for the other batched entries (route.hip entry_plan) against the rules written out in entry_truth.  One level down,
pioran_step_route (scan_plan, wide_plan: the kernel instantiation of a step-by-step launch) against the listing recorded before those rules
existed, the names the GPU tests assert, and properties over the listing's grid; pioran_window_route (block_plan, tile_plan, tp_step_plan) against
the listing recorded before those."""
import importlib.util
import itertools
import json
from pathlib import Path

import pytest

import pioran_jl_amd as pj

ROOT = Path(__file__).resolve().parents[1]


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, ROOT / "tools" / f"{name}.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _tool("route_grid")


def route(rows, n_one, B, N, options="", series=False, pass_draws=0):
    assert (rows + n_one) % 2 == 0
    return G.value_route(rows, (rows + n_one) // 2, n_one, B, N, series, pass_draws, options)


# (rows, one-row terms, B, N, options, per-draw series, pass) -> family ("!tp": any family but that one), each from an assertion on
# pioran_celerite_config_name(-1) (test_abi.py: on pioran_celerite_config_name(R)) in the suite
PINNED = [
    ((40, 0, 37, 257, "scan_config=tile", False, 0), "tile"),        # test_gpu_parity.py:172 (J = 20)
    ((2, 0, 37, 257, "scan_config=tile", False, 0), "tile"),         # test_gpu_parity.py:172 (J = 1)
    ((14, 0, 1, 130, "", False, 0), "block"),                        # test_gpu_parity.py:196 (J = 7, one draw)
    ((4, 0, 1, 130, "", False, 0), "scan"),                          # test_gpu_parity.py:196 (J = 2)
    ((60, 0, 1, 130, "scan_config=tile", False, 0), "tile"),         # test_gpu_parity.py:198 (J = 30)
    ((40, 0, 300, 100, "scan_config=block", False, 0), "block"),     # test_gpu_parity.py:214
    ((46, 0, 1000, 33, "scan_config=block", False, 0), "block"),     # test_gpu_parity.py:214 (J = 23)
    ((40, 0, 9, 333, "", False, 0), "block"),                        # test_gpu_parity.py:237
    ((8, 2, 9, 48, "", False, 0), "block"),                          # test_gpu_parity.py:237 (J = 5, two one-row terms)
    ((40, 0, 4200, 150, "no_tile=1", False, 4096), "scan + block (remainder)"),             # test_gpu_parity.py:282 (SHO-20: 4096 draws per pass)
    ((60, 20, 2125, 150, "no_tile=1", False, 2048), "scan + block (remainder)"),            # test_gpu_parity.py:282 (DRWCelerite-20: 2048)
    ((40, 0, 4200, 150, "no_tile=1;no_split=1", False, 4096), "scan"),                      # test_gpu_parity.py:285
    ((80, 0, 1094, 120, "no_tile=1", False, 1024), "scan + block (remainder)"),             # test_gpu_parity.py:328 (J = 40)
    ((64, 0, 2148, 120, "no_tile=1", False, 2048), "scan + block (remainder)"),             # test_gpu_parity.py:328 (J = 32)
    ((80, 0, 1094, 120, "no_tile=1;no_split=1", False, 1024), "scan"),                      # test_gpu_parity.py:331
    ((2, 0, 4, 2500, "", False, 0), "tp"),                           # test_gpu_parity.py:412 (J = 1; up to four rows: from 1024 steps)
    ((5, 1, 1, 2500, "", False, 0), "tp"),                           # test_gpu_parity.py:412 (J = 3, one one-row term: from 2048)
    ((5, 1, 1, 900, "", False, 0), "!tp"),                           # test_gpu_parity.py:412
    ((4, 0, 3, 16461, "no_tp=1", False, 0), "block"),                # test_gpu_parity.py:417 (long series)
    ((4, 0, 1, 2500, "no_tp=1", False, 0), "scan"),                  # test_gpu_parity.py:417
    ((5, 1, 4, 2500, "no_tp=1", False, 0), "block"),                 # test_gpu_parity.py:417 (five rows)
    ((4, 0, 1, 2500, "no_tp=1", True, 0), "block"),                  # test_gpu_parity.py:421 (the scalar call: per-draw series, from 2048 steps)
    ((4, 0, 1, 900, "no_tp=1", True, 0), "scan"),                    # test_gpu_parity.py:421
    ((80, 0, 300, 61, "no_wide=1;no_block=1", False, 0), "scan"),    # test_gpu_parity.py:452
    ((66, 0, 290, 130, "no_wide=1;no_block=1", False, 0), "scan"),   # test_gpu_parity.py:452 (J = 33)
    ((80, 0, 5, 61, "no_block=1", False, 0), "wide"),                # test_gpu_parity.py:470
    ((64, 0, 4, 300, "", False, 0), "block"),                        # test_gpu_parity.py:492
    ((94, 0, 256, 40, "", False, 0), "block"),                       # test_gpu_parity.py:492 (J = 47)
    ((70, 20, 6, 75, "", True, 0), "block"),                         # test_gpu_parity.py:496 (per-draw series)
    ((94, 0, 256, 40, "no_block=1", False, 0), "wide"),              # test_gpu_parity.py:502
    ((4, 0, 3, 8192, "", False, 0), "tp"),                           # test_gpu_parity.py:2027
    ((4, 0, 9, 8192, "", False, 0), "tp"),                           # test_gpu_parity.py:2036
    ((4, 0, 66, 8192, "", False, 0), "!tp"),                         # test_gpu_parity.py:2038
    ((4, 0, 3, 900, "", False, 0), "!tp"),                           # test_gpu_parity.py:2041
    ((14, 0, 2, 5000, "", False, 0), "tp"),                          # test_gpu_parity.py:2046
    ((14, 0, 4, 5000, "", False, 0), "tp"),                          # test_gpu_parity.py:2049
    ((14, 0, 34, 5000, "", False, 0), "!tp"),                        # test_gpu_parity.py:2051
    ((12, 0, 4, 5000, "", False, 0), "tp"),                          # test_gpu_parity.py:2053
    ((24, 0, 2, 7000, "", False, 0), "tp"),                          # test_gpu_parity.py:2059
    ((40, 0, 4, 7000, "", False, 0), "tp"),                          # test_gpu_parity.py:2061
    ((40, 0, 12, 7000, "", False, 0), "!tp"),                        # test_gpu_parity.py:2063
    ((32, 0, 4, 7000, "", False, 0), "tp"),                          # test_gpu_parity.py:2065
    ((4, 0, 3, 8192, "", True, 0), "tp"),                            # test_gpu_parity.py:2070 (per-draw series)
    ((40, 0, 4200, 10000, "no_tile=1", False, 4096), "scan + block (remainder)"),           # test_gpu_configs.py:67
    ((40, 0, 4200, 10000, "no_tile=1;no_split=1", False, 4096), "scan"),                    # test_gpu_configs.py:67
    ((40, 0, 4096, 10000, "", False, 0), "tile"),                    # test_gpu_configs.py:105 (SHO-20)
    ((60, 20, 4096, 10000, "", False, 0), "tile"),                   # test_gpu_configs.py:105 (DRWCelerite-20)
    ((40, 0, 4096, 10000, "no_tile=1", False, 4096), "scan"),        # test_gpu_configs.py:113
    ((1, 1, 5, 37, "scan_config=tile", False, 0), "tile"),           # test_gpu_tile_ksteps.py:62 (R = 1)
    ((95, 1, 5, 37, "scan_config=tile", False, 0), "tile"),          # test_gpu_tile_ksteps.py:62 (R = 95)
    ((17, 1, 3, 29, "scan_config=tile", True, 0), "tile"),           # test_gpu_tile_ksteps.py:82
    ((128, 0, 4096, 10000, "", False, 0), "wide"),                   # test_abi.py:42 (a large batch of 128 rows)
    ((128, 0, 5, 257, "", False, 0), "wide"),                        # test_abi.py:42
    ((144, 0, 4096, 10000, "", False, 0), "fallback"),               # test_abi.py:43 (a large batch of 144 rows)
    ((144, 0, 5, 257, "", False, 0), "fallback"),                    # test_abi.py:43
]


@pytest.mark.parametrize("query,family", PINNED)
def test_routes_the_suite_already_asserts(query, family):
    rows, n_one, B, N, options, series, pass_draws = query
    got, _ = route(rows, n_one, B, N, options, series, pass_draws)
    assert (got != family[1:]) if family.startswith("!") else (got == family), got


def test_every_family_is_pinned_twice():
    names = [f for _, f in PINNED]
    for fam in ("tp", "tile", "block", "scan + block (remainder)", "wide", "scan", "fallback"):
        assert names.count(fam) >= 2, fam
    assert len(PINNED) >= 25


GRID_B = (1, 2, 3, 8, 9, 32, 33, 64, 65, 256, 512, 513, 768, 1024, 1025, 2048, 4096, 4200)
GRID_N = (1, 63, 64, 1023, 1024, 2048, 10000, 65536, 10 ** 6)
FORBIDS = {"no_tp=1": ("tp",), "no_tile=1": ("tile",), "no_block=1": ("block", "scan + block (remainder)"), "no_wide=1": ("wide",),
           "no_split=1": ("scan + block (remainder)",)}


def check_tp_plan(rows, B, N, plan):
    """What pioran_launch_tp refuses on (celerite_tp.hip), and the segment limits of its two boundary phases."""
    scan, RP, nseg, L = plan
    assert RP >= rows and RP % (2 if RP <= 12 else 8) == 0 and RP <= 64, (rows, B, N, plan)
    assert 1 <= nseg <= (256 if scan else 128), (rows, B, N, plan)
    assert nseg == 1 or 16 * nseg <= N, (rows, B, N, plan)
    assert (nseg - 1) * L < N <= nseg * L, (rows, B, N, plan)


def test_properties_over_the_grid():
    """Default options over rows x B x N, and every forbidding option over the same grid at every third row count: ~89 000 queries.  `pass` = 4096
    (the SHO-20 figure) so that the remainder split and the tile ladder's pass-dependent leg are both reachable."""
    n = 0
    lib = pj._lib.lib()
    for rows, B, N in itertools.product(range(1, 151), GRID_B, GRID_N):
        n_one = rows % 2
        fam, plan = route(rows, n_one, B, N, pass_draws=4096)
        n += 1
        if fam == "tp":
            assert B <= 64 and N >= 64 and rows <= 64, (rows, B, N)
            check_tp_plan(rows, B, N, plan)
        else:
            assert plan == (0, 0, 0, 0)
        if B > 64 or N < 64:
            assert fam != "tp"
        if rows > 143:
            assert fam == "fallback", (rows, B, N, fam)
        if fam == "tile":
            assert lib.pioran_tile_choice(rows, B, 4096, 0) == 1, (rows, B, N)
        assert route(rows, n_one, B, N, "force_fallback=1", pass_draws=4096)[0] == "fallback"
        n += 1
        if rows % 3 == 0:
            for opt, forbidden in FORBIDS.items():
                got, plan = route(rows, n_one, B, N, opt, pass_draws=4096)
                n += 1
                assert got not in forbidden, (rows, B, N, opt, got)
                if got == "tp":
                    check_tp_plan(rows, B, N, plan)
    assert n >= 20000


@pytest.mark.parametrize("options", ["scan_config=tp", "scan_config=tp;tp_scan=1", "scan_config=tp;tp_scan=0", "scan_config=tp;tp_unchecked=1",
                                     "scan_config=tp;tp_segments=7", "scan_config=tp;tp_segments=1000", "tp_scan=1", "no_block=1"])
def test_time_parallel_plans_under_its_options(options):
    """Forced, with either boundary phase, without the repair pass, with a segment count from the caller: still only plans the kernels take."""
    taken = 0
    for rows, B, N in itertools.product((1, 2, 3, 4, 5, 8, 12, 13, 16, 17, 24, 40, 47, 60, 64, 65), (1, 2, 3, 8, 32, 64, 65), GRID_N):
        fam, plan = route(rows, rows % 2, B, N, options)
        if fam == "tp":
            taken += 1
            check_tp_plan(rows, B, N, plan)
            assert B <= 64 and N >= 64 and rows <= 64
    assert taken > 0 or options == "no_block=1"      # (without the windowed kernel there is no repair pass: not an automatic choice)


def test_time_parallel_thresholds_of_the_gpu_grid():
    """tools/route_grid.py's table: per (state rows, draws) the family takes N = threshold and not N = threshold - 64."""
    for rows, thresholds in G.TP_THRESHOLD.items():
        for B, n in zip(G.TP_B, thresholds):
            assert n <= 12288 and n % 64 == 0
            assert route(rows, 0, B, n)[0] == "tp" and route(rows, 0, B, n - 64)[0] != "tp", (rows, B, n)
    for pt in G.batch_points():
        assert G.value_route(G.rows_of(pt), pt.J, pt.n_one, pt.B, pt.N, options=pt.options)[0] != "tp"


def test_argument_validation():
    import ctypes
    L = pj._lib.lib()
    name = ctypes.create_string_buffer(8)
    assert L.pioran_value_route(40, 20, 0, 8, 100, 0, 0, None, name, 8, None) == 0 and name.value == b"block"
    assert L.pioran_value_route(40, 20, 0, 4200, 100, 0, 4096, b"no_tile=1", name, 8, None) == 0 and name.value == b"scan + "   # cut to the buffer
    assert L.pioran_value_route(40, 20, 1, 8, 100, 0, 0, None, name, 8, None) == -1          # 40 rows are not 20 terms with a one-row term
    assert L.pioran_value_route(40, 20, 0, 0, 100, 0, 0, None, name, 8, None) == -1
    assert L.pioran_value_route(40, 20, 0, 8, 100, 0, 0, b"no_such_option=1", name, 8, None) == -1
    assert L.pioran_value_route(40, 20, 0, 8, 100, 0, 0, b"no_block", name, 8, None) == -1
    assert L.pioran_value_route(40, 20, 0, 8, 100, 0, 0, None, None, 8, None) == -1


def test_removed_experiment_options_are_unknown():
    """The row-sum variants ("gsum") and the dense timing experiments (dense_old_chain above 1) are gone from the library: their option
    strings are refused like any unknown key or value, the options that stay are accepted."""
    import ctypes
    L = pj._lib.lib()
    name = ctypes.create_string_buffer(32)
    for options, rc in ((b"gsum=1", -1), (b"dense_old_chain=2", -1), (b"dense_old_chain=1", 0), (b"no_win2=1", 0)):
        assert L.pioran_value_route(40, 20, 0, 8, 100, 0, 0, options, name, 32, None) == rc, options


# ---- draws that bring (c, d) of their own: pioran_value_route_cd (route.hip mixed_plan, perdraw_form) ---------------------------------------------
def route_cd(n_two, n_one, npd, B, N, options="", series=False, must_run=False):
    return G.value_route_cd(n_two, n_one, npd, B, N, series, must_run, options)


EDGE_J = ((3, 1, 0), (7, 2, 1), (15, 1, 0), (16, 2, 3), (23, 1, 0), (24, 2, 0), (30, 2, 0), (31, 1, 0))      # test_block_kernel_per_draw_rows_edges: J < 32
# (two-row, one-row, per-draw terms, B, N, options, must_run) -> family; a tuple: one of these; "~block": a name without "block".  Each from an
# assertion on pioran_celerite_config_name(-1) in the suite, but for the names no test there asserts on these paths — those are points of
# tools/route_grid.py, which tests/test_gpu_route.py holds to the launch and profiles/value_route_cd_listing.txt to the library before the rules moved
PINNED_CD = [
    ((0, 0, 2, 19, 130, "", False), "block+pd"),                                      # test_gpu_parity.py:186 (J = 2; layout "block")
    ((0, 0, 7, 19, 130, "", False), "block (per-draw tables)"),                       # test_gpu_parity.py:186 (J = 7)
    ((0, 0, 20, 19, 130, "", False), "block (per-draw tables)"),                      # test_gpu_parity.py:186 (J = 20)
    ((0, 0, 30, 19, 130, "", False), "block (per-draw tables)"),                      # test_gpu_parity.py:186 (J = 30)
    ((0, 0, 2, 19, 130, "scan_config=tile", False), "block+pd"),                      # test_gpu_parity.py:186 (layout "tile": takes no per-draw (c, d))
    ((0, 0, 20, 19, 130, "scan_config=tile", False), "block (per-draw tables)"),      # test_gpu_parity.py:186
    ((0, 0, 2, 19, 130, "no_block=1;no_wide=1", False), ("scan", "wide")),            # test_gpu_parity.py:188 (layout "throughput")
    ((0, 0, 30, 19, 130, "no_block=1;no_wide=1;no_win2=1", False), ("scan", "wide")), # test_gpu_parity.py:188 ("throughput_steps")
    ((0, 0, 7, 19, 130, "no_block=1", False), ("scan", "wide")),                      # test_gpu_parity.py:188 ("latency")
    ((0, 0, 20, 19, 130, "no_block=1;wide2=1;scan_config=wide", False), ("scan", "wide")),   # test_gpu_parity.py:188 ("latency_lean")
    ((0, 0, 1, 16, 300, "", False), "block+pd"),                                      # test_gpu_parity.py:381
    ((0, 0, 2, 70, 129, "", False), "block+pd"),                                      # test_gpu_parity.py:381
    ((0, 0, 2, 300, 1000, "", False), "block+pd"),                                    # test_gpu_parity.py:381
    ((0, 0, 1, 700, 77, "", False), "block+pd"),                                      # test_gpu_parity.py:381
    ((0, 0, 2, 2, 40, "", False), "block+pd"),                                        # test_gpu_parity.py:381
    ((0, 0, 1, 16, 300, "no_block=1", False), "~block"),                              # test_gpu_parity.py:385
    ((0, 0, 2, 300, 1000, "no_block=1", False), "~block"),                            # test_gpu_parity.py:385
    ((0, 0, 1, 700, 77, "no_block=1", False), "~block"),                              # test_gpu_parity.py:385
    ((20, 0, 1, 37, 140, "", False), "block+pd"),                                     # test_gpu_parity.py:1472 (J = 21, one per draw)
    ((10, 0, 2, 37, 140, "", False), "block+pd"),                                     # test_gpu_parity.py:1472 (J = 12, two)
    ((6, 2, 1, 37, 140, "", False), "block+pd"),                                      # test_gpu_parity.py:1472 (J = 9, two one-row terms)
    ((1, 2, 2, 37, 140, "", False), "block+pd"),                                      # test_gpu_parity.py:1472 (J = 5)
    *[((J - npd - nreal, nreal, npd, B, N, "", False), "block+pd")                    # test_gpu_parity.py:1506 (J < 32)
      for J, npd, nreal in EDGE_J for N, B in ((1, 3), (17, 9), (100, 300))],
    *[((J - npd - nreal, nreal, npd, B, N, "no_block=1", False), ("wide", "scan"))    # test_gpu_parity.py:1516
      for J, npd, nreal in EDGE_J for N, B in ((17, 9), (100, 300))],
    ((20, 0, 1, 24, 10000, "", False), "block+pd"),                                   # test_gpu_parity.py:1539 (approx continuum + one QPO term, 24 draws)
    ((0, 0, 10, 23, 300, "", False), "block (per-draw tables)"),                      # test_gpu_chunking.py:229
    ((0, 0, 40, 8, 130, "", False), "wide (per-draw tables)"),                        # tools/route_grid.py (80 rows)
    ((0, 0, 40, 300, 24, "", False), "wide (per-draw tables)"),                       # tools/route_grid.py (two chunks of tables)
    ((0, 0, 32, 8, 130, "", False), "scan"),                                          # tools/route_grid.py (64 rows: past the windowed tables)
    ((0, 0, 72, 8, 130, "", False), "fallback"),                                      # tools/route_grid.py (144 rows)
    ((5, 0, 3, 37, 130, "", False), "wide"),                                          # tools/route_grid.py (three per draw: the combined table, 16 rows)
    ((5, 0, 3, 8, 130, "", True), "wide"),                                            # tools/route_grid.py theta_points (n_qpo = 3: must run below 16 draws)
    ((5, 0, 1, 8, 130, "", True), "block+pd"),                                        # tools/route_grid.py theta_points (n_qpo = 1)
]
CD_NAMES = ("block+pd", "block (per-draw tables)", "wide (per-draw tables)", "scan", "wide", "fallback")


@pytest.mark.parametrize("query,family", PINNED_CD)
def test_per_draw_routes_the_suite_already_asserts(query, family):
    n_two, n_one, npd, B, N, options, must_run = query
    got, _ = route_cd(n_two, n_one, npd, B, N, options, must_run=must_run)
    assert got in CD_NAMES
    if family == "~block":
        assert "block" not in got, got
    else:
        assert got in ((family,) if isinstance(family, str) else family), got


def test_every_per_draw_name_is_pinned():
    names = [f for _, f in PINNED_CD]
    for fam in CD_NAMES:
        assert fam in names, fam


MIXED_LIMIT = 0x7fff0000      # the combined table is addressed with 32-bit byte offsets


def cd_grid():
    """rows 1 .. 150 with 1, 2, 3, 8, 9 or all terms per draw, the other rows as two-row terms and at most one one-row term."""
    for rows in range(1, 151):
        for npd in (1, 2, 3, 8, 9, "all"):
            if npd == "all":
                if rows % 2:
                    continue
                npd = rows // 2
            rest = rows - 2 * npd
            if rest < 0:
                continue
            yield rows, rest // 2, rest % 2, npd


def check_cd(query, fam, chunk, options=""):
    rows, n_two, n_one, npd, B, N, must_run = query
    J, R = n_two + n_one + npd, 2 * (n_two + n_one + npd)
    forced = "scan_config=block" in options
    assert fam in CD_NAMES or (must_run and fam is None), (query, options, fam)
    if fam == "block+pd":
        assert npd <= 2 and chunk >= 1, (query, options)
        if not forced:
            assert B <= (512 if rows >= 6 else 768), (query, options)
    if fam == "block (per-draw tables)":
        assert 6 <= R <= 63 and B <= 768 or forced, (query, options)
        assert R <= 63
    if fam == "wide (per-draw tables)":
        assert 80 <= R <= 143, (query, options)
    if chunk:        # mixed mode has the batch: the combined table of a chunk stays addressable
        assert fam in ("block+pd", "scan", "wide") and 1 <= chunk <= B and npd <= 8, (query, options, fam, chunk)
        assert (N + 1) * 8 * (3 * (rows + 2) + 2 + 6 * npd * chunk) <= MIXED_LIMIT, (query, options, chunk)
        if not must_run and fam != "block+pd":
            assert chunk >= 16 and (chunk % 16 == 0 or chunk == B), (query, options, chunk)
    elif fam is not None:
        assert fam != "block+pd" and fam != "wide"


def test_per_draw_properties_over_the_grid():
    """Default options over (rows, per-draw terms) x B x N with and without must_run.  B = 1 without must_run is the shared case to the host
    entry: the rule answers for the device entry there."""
    n = 0
    for (rows, n_two, n_one, npd), B, N in itertools.product(cd_grid(), GRID_B, GRID_N):
        for must_run in (False, True):
            fam, chunk = route_cd(n_two, n_one, npd, B, N, must_run=must_run)
            check_cd((rows, n_two, n_one, npd, B, N, must_run), fam, chunk)
            n += 1
    assert n == 2 * 127008


def test_per_draw_options_over_the_grid():
    """The options that forbid or force a family, over the whole grid.  scan_config=block lifts the batch limits and nothing else: the windowed
    kernel with per-draw rows has a batch of any size exactly where it has two draws of the same terms and series length by default (two draws
    are within every batch limit; what remains is what the kernel fits and mixed mode's own cuts), and so have the windowed per-draw tables
    where mixed mode does not take the batch.
    force_fallback takes the windowed kernels away and nothing else of mixed mode: a batch mixed mode takes runs its combined table on the scan
    with the option set (16 858 "scan" and 11 898 "wide" of the 127 008 queries — the library did so before the rules were written down, and
    tools/route_grid.py holds one such launch against it); every other query ends on the fallback kernel."""
    small = {}
    on_scan = 0
    for (rows, n_two, n_one, npd), B, N in itertools.product(cd_grid(), GRID_B, GRID_N):
        q = (rows, n_two, n_one, npd, B, N, False)
        for options in ("no_block=1", "no_block=1;no_wide=1"):
            fam, chunk = route_cd(n_two, n_one, npd, B, N, options)
            check_cd(q, fam, chunk, options)
            assert "block" not in fam, (q, options, fam)
        nb_chunk = chunk
        fam, chunk = route_cd(n_two, n_one, npd, B, N, "no_mixed=1")
        check_cd(q, fam, chunk, "no_mixed=1")
        assert fam != "block+pd" and chunk == 0, (q, fam)
        fam, chunk = route_cd(n_two, n_one, npd, B, N, "scan_config=block")
        check_cd(q, fam, chunk, "scan_config=block")
        key = (n_two, n_one, npd, N)
        if key not in small:
            small[key] = route_cd(n_two, n_one, npd, 2, N)[0]
        if B > 1:
            assert (fam == "block+pd") == (small[key] == "block+pd"), (q, fam, small[key])
            if small[key] == "block (per-draw tables)" and not chunk:      # (unless mixed mode has the larger batch on its combined table)
                assert fam == small[key], (q, fam)
        fam, chunk = route_cd(n_two, n_one, npd, B, N, "force_fallback=1")
        assert chunk == nb_chunk, (q, chunk, nb_chunk)      # mixed mode takes what it takes without the windowed kernel
        assert fam in ("scan", "wide") if chunk else fam == "fallback", (q, fam, chunk)
        on_scan += chunk != 0
    assert on_scan == 28756


def test_per_draw_argument_validation():
    import ctypes
    L = pj._lib.lib()
    name = ctypes.create_string_buffer(8)
    chunk = ctypes.c_int64(-1)
    assert L.pioran_value_route_cd(20, 0, 1, 24, 10000, 0, 0, None, name, 8, ctypes.byref(chunk)) == 0 and name.value == b"block+p"   # cut to the buffer
    assert chunk.value == 24
    assert L.pioran_value_route_cd(20, 0, 0, 24, 100, 0, 0, None, name, 8, None) == -1           # no per-draw term: pioran_value_route's business
    assert L.pioran_value_route_cd(-1, 0, 1, 24, 100, 0, 0, None, name, 8, None) == -1
    assert L.pioran_value_route_cd(20, 0, 1, 0, 100, 0, 0, None, name, 8, None) == -1
    assert L.pioran_value_route_cd(20, 0, 1, 24, 100, 0, 0, b"no_such_option=1", name, 8, None) == -1
    assert L.pioran_value_route_cd(20, 0, 1, 24, 100, 0, 0, None, None, 8, None) == -1
    assert L.pioran_value_route_cd(20, 0, 1, 24, 2 ** 48, 0, 0, None, name, 8, None) == 0            # the longest series the entry answers for
    assert L.pioran_value_route_cd(20, 0, 1, 24, 2 ** 48 + 1, 0, 0, None, name, 8, None) == -1
    # the theta entry with more rows than the scan holds: refused (PIORAN_ERR_UNSUPPORTED), where the host entry goes on to the generic path
    assert L.pioran_value_route_cd(40, 0, 1, 24, 100, 0, 1, None, name, 8, ctypes.byref(chunk)) == -4 and name.value == b"" and chunk.value == 0
    assert L.pioran_value_route_cd(40, 0, 1, 24, 100, 0, 0, None, name, 8, None) == 0 and name.value == b"wide (p"


# ---- the other batched entries: pioran_entry_route (route.hip entry_plan) --------------------------------------------------------------------------
P, V, GR, S, RP = "predict", "predict_var", "grad", "simulate", "rand_posterior"
ENTRY_NAMES = G.ENTRY_NAME_TABLE      # the strings of route.hip kEntryNames: wide, block, block with per-draw tables, tile


def entry(which, rows, n_one, B, per_draw=False, shift=False, cd=(True, True), series=False, options=""):
    assert (rows + n_one) % 2 == 0
    return G.entry_route(which, rows, (rows + n_one) // 2, n_one, B, per_draw, shift, cd[0], cd[1], series, options)


# (entry, rows, one-row terms, B, per draw, shift, (d/dc, d/dd), series gradients, options) -> name, each from an assertion on
# pioran_celerite_config_name(-1) in the suite.  Dataset.logl_grad asks for d/d(c, d) unless cd_grad=False.
PINNED_ENTRY = [
    ((P, 20, 0, 23, False, False, (1, 1), False, ""), ENTRY_NAMES[P][1]),                       # test_gpu_chunking.py:116 (SHO-10, 23 draws)
    ((P, 20, 0, 23, False, False, (1, 1), False, "no_block=1"), ENTRY_NAMES[P][0]),             # test_gpu_chunking.py:116
    ((P, 20, 0, 23, True, False, (1, 1), False, ""), ENTRY_NAMES[P][2]),                        # test_gpu_chunking.py:135
    ((V, 20, 0, 23, False, False, (1, 1), False, ""), ENTRY_NAMES[V][0]),                       # test_gpu_chunking.py:153
    ((GR, 20, 0, 23, False, False, (1, 1), False, ""), ENTRY_NAMES[GR][1]),                     # test_gpu_chunking.py:172
    ((GR, 20, 0, 23, False, False, (1, 1), False, "no_block=1"), ENTRY_NAMES[GR][0]),           # test_gpu_chunking.py:172
    ((GR, 20, 0, 23, False, False, (1, 1), True, ""), ENTRY_NAMES[GR][1]),                      # test_gpu_chunking.py:172 (series gradients)
    ((GR, 20, 0, 23, True, False, (1, 1), False, ""), ENTRY_NAMES[GR][2]),                      # test_gpu_chunking.py:190
    ((S, 20, 0, 23, False, False, (1, 1), False, ""), ENTRY_NAMES[S][1]),                       # test_gpu_chunking.py:209
    ((S, 20, 0, 23, True, False, (1, 1), False, ""), ENTRY_NAMES[S][2]),                        # test_gpu_chunking.py:209
    ((P, 20, 0, 23, True, False, (1, 1), False, "no_block=1"), ENTRY_NAMES[P][0]),              # test_gpu_chunking.py:271 (draw by draw)
    ((V, 20, 0, 23, True, False, (1, 1), False, ""), ENTRY_NAMES[V][0]),                        # test_gpu_chunking.py:285 (no per-draw form)
    ((S, 20, 0, 23, True, False, (1, 1), False, "no_block=1"), ENTRY_NAMES[S][0]),              # test_gpu_chunking.py:293
    ((GR, 20, 0, 23, True, False, (1, 1), True, "no_block=1"), ENTRY_NAMES[GR][0]),             # test_gpu_chunking.py:304
    ((GR, 20, 0, 23, True, True, (1, 1), False, ""), ENTRY_NAMES[GR][1]),                       # test_gpu_chunking.py:319 (the shifted form: draw by draw)
    ((P, 40, 0, 601, False, False, (1, 1), False, ""), ENTRY_NAMES[P][1]),                      # test_gpu_big.py:31 (SHO-20, three chunks)
    ((S, 40, 0, 601, False, False, (1, 1), False, ""), ENTRY_NAMES[S][1]),                      # test_gpu_big.py:65
    ((V, 1, 1, 70, False, False, (1, 1), False, ""), ENTRY_NAMES[V][0]),                        # test_gpu_predict_var.py:334 (R = 1)
    ((V, 64, 0, 70, False, False, (1, 1), False, ""), ENTRY_NAMES[V][0]),                       # test_gpu_predict_var.py:334 (the last row count it takes)
    ((V, 40, 0, 5, False, False, (1, 1), False, ""), ENTRY_NAMES[V][0]),                        # test_gpu_predict_var.py:81, :260 (families of cases)
    ((RP, 40, 0, 5, False, False, (1, 1), False, ""), ENTRY_NAMES[RP][1]),                      # test_gpu_rand_posterior.py:58, :114 (_family :39: up to 63 rows), :182
    ((RP, 63, 1, 5, False, False, (1, 1), False, ""), ENTRY_NAMES[RP][1]),                      # test_gpu_rand_posterior.py:58 (63 rows, one one-row term)
    ((RP, 64, 0, 5, False, False, (1, 1), False, ""), ENTRY_NAMES[RP][0]),                      # test_gpu_rand_posterior.py:58 (_family :39: above)
    ((RP, 40, 0, 5, False, False, (1, 1), False, "no_block=1"), ENTRY_NAMES[RP][0]),            # test_gpu_rand_posterior.py:58, :114 (_family :39: no_block)
    ((GR, 40, 0, 5, False, False, (1, 1), True, ""), ENTRY_NAMES[GR][1]),                       # test_gpu_grad_truth.py:66 (legs :74: default routing, up to 63 rows)
    ((GR, 80, 0, 5, False, False, (1, 1), True, ""), ENTRY_NAMES[GR][0]),                       # test_gpu_grad_truth.py:66 (legs :74: above)
    ((GR, 40, 0, 5, False, False, (1, 1), False, "no_block=1"), ENTRY_NAMES[GR][0]),            # test_gpu_grad_truth.py:66 (legs :86), :174 (leg no_block)
    ((GR, 40, 0, 5, False, False, (0, 0), False, "scan_config=tile"), ENTRY_NAMES[GR][3]),      # test_gpu_grad_truth.py:66 (legs :91), :174 (leg tile)
    ((GR, 40, 0, 5, False, False, (1, 1), False, "scan_config=tile"), ENTRY_NAMES[GR][3]),      # test_gpu_grad_truth.py:66 (legs :92: with d/d(c, d))
    ((GR, 16, 0, 5, True, False, (1, 1), False, ""), ENTRY_NAMES[GR][2]),                       # test_gpu_grad_truth.py:66 (legs :82: 2 J <= 63), :174 (leg per-draw tables)
    ((GR, 80, 0, 5, True, False, (1, 1), False, ""), ENTRY_NAMES[GR][0]),                       # test_gpu_grad_truth.py:66 (legs :82: else draw by draw)
    ((GR, 12, 0, 3, False, False, (1, 1), True, ""), ENTRY_NAMES[GR][1]),                       # test_gpu_fuzz.py:92 (windowed gradient fuzz)
    ((GR, 12, 0, 3, True, False, (1, 1), False, ""), ENTRY_NAMES[GR][2]),                       # test_gpu_fuzz.py:92 (per draw)
    ((P, 30, 0, 3, False, False, (1, 1), False, ""), ENTRY_NAMES[P][1]),                        # test_gpu_fuzz.py:151
    ((S, 30, 0, 3, False, False, (1, 1), False, ""), ENTRY_NAMES[S][1]),                        # test_gpu_fuzz.py:153
    ((P, 30, 0, 3, True, False, (1, 1), False, ""), ENTRY_NAMES[P][2]),                         # test_gpu_fuzz.py:205
    ((S, 30, 0, 3, True, False, (1, 1), False, ""), ENTRY_NAMES[S][2]),                         # test_gpu_fuzz.py:207
    ((GR, 100, 0, 3, False, False, (1, 1), False, ""), ENTRY_NAMES[GR][0]),                     # test_gpu_fuzz.py:278 (past the windowed kernels)
    ((S, 100, 0, 3, False, False, (1, 1), False, ""), ENTRY_NAMES[S][0]),                       # test_gpu_fuzz.py:286
    ((P, 100, 0, 3, False, False, (1, 1), False, ""), ENTRY_NAMES[P][0]),                       # test_gpu_fuzz.py:292
    ((P, 40, 0, 5, False, False, (1, 1), False, ""), ENTRY_NAMES[P][1]),                        # test_gpu_predict_mean_sim.py:71 (_family :46: default, shared)
    ((P, 80, 0, 5, False, False, (1, 1), False, ""), ENTRY_NAMES[P][0]),                        # test_gpu_predict_mean_sim.py:71 (_family :46: above 63 rows)
    ((S, 16, 0, 5, True, False, (1, 1), False, ""), ENTRY_NAMES[S][2]),                         # test_gpu_predict_mean_sim.py:79 (_family :48: 2 J <= 63)
    ((S, 40, 0, 5, False, False, (1, 1), False, "no_block=1"), ENTRY_NAMES[S][0]),              # test_gpu_predict_mean_sim.py:79 (_family :46: no_block)
    ((S, 40, 0, 5, False, False, (1, 1), False, ""), ENTRY_NAMES[S][1]),                        # test_gpu_predict_mean_sim.py:172
    ((GR, 20, 0, 700, False, False, (0, 0), False, ""), ENTRY_NAMES[GR][3]),                    # test_gpu_parity.py:2281, :2313, :2316 (700 chains, 20 rows: the same query)
    ((GR, 20, 0, 700, False, False, (0, 0), False, "workspace_limit_mb=1"), ENTRY_NAMES[GR][3]),  # test_gpu_parity.py:2306 (several launches: the same family)
    ((GR, 20, 0, 512, False, False, (0, 0), False, ""), ENTRY_NAMES[GR][1]),                    # test_gpu_parity.py:2282 (512: the windowed kernels' last)
    ((GR, 20, 0, 700, False, False, (1, 1), False, ""), ENTRY_NAMES[GR][3]),                    # test_gpu_parity.py:2284 (with d/d(c, d))
    ((GR, 16, 0, 700, False, False, (0, 0), False, ""), ENTRY_NAMES[GR][1]),                    # test_gpu_parity.py:2285 (16 rows: below the tile range)
    ((GR, 20, 0, 700, False, False, (0, 0), False, "no_tile=1"), ENTRY_NAMES[GR][1]),           # test_gpu_parity.py:2289
    ((GR, 20, 0, 700, False, False, (1, 1), False, "no_tile=1"), ENTRY_NAMES[GR][1]),           # test_gpu_parity.py:2298
    ((GR, 72, 0, 2, False, True, (1, 1), False, ""), ENTRY_NAMES[GR][0]),                       # test_gpu_parity.py:2667 (36 components, shifted)
    ((GR, 104, 0, 2, False, True, (1, 1), False, ""), ENTRY_NAMES[GR][0]),                      # test_gpu_parity.py:2667 (52 components)
    ((GR, 72, 0, 5, False, False, (1, 1), True, "no_wide2=1"), ENTRY_NAMES[GR][0]),             # test_gpu_grad_truth.py:66 (legs :89), :174 (leg no_wide2)
    ((GR, 48, 0, 5, False, False, (1, 1), True, "no_wide2=1;no_block=1"), ENTRY_NAMES[GR][0]),  # test_gpu_grad_truth.py:66 (legs :89: with no_block below 64 rows)
    ((GR, 63, 35, 1, False, False, (0, 0), False, ""), (ENTRY_NAMES[GR][1], ENTRY_NAMES[GR][0])),  # test_gpu_grad_truth.py:104 (49 terms: either family)
    ((GR, 20, 0, 5, False, False, (1, 1), True, ""), ENTRY_NAMES[GR][1]),                       # test_gpu_grad_truth.py:174 (leg block)
    ((GR, 100, 0, 5, False, False, (1, 1), True, ""), ENTRY_NAMES[GR][0]),                      # test_gpu_grad_truth.py:174 (leg wide)
    ((P, 16, 0, 5, True, False, (1, 1), False, ""), ENTRY_NAMES[P][2]),                         # test_gpu_predict_mean_sim.py:71 (_family :48)
    ((P, 40, 0, 5, False, False, (1, 1), False, "no_block=1"), ENTRY_NAMES[P][0]),              # test_gpu_predict_mean_sim.py:71 (_family :46: no_block)
    ((S, 80, 0, 5, False, False, (1, 1), False, ""), ENTRY_NAMES[S][0]),                        # test_gpu_predict_mean_sim.py:79 (_family :46: above 63 rows)
    ((P, 40, 0, 40, False, False, (1, 1), False, ""), ENTRY_NAMES[P][1]),                       # test_gpu_parity.py:1654 (SHO-20, 40 draws)
    ((P, 40, 0, 40, False, False, (1, 1), False, "no_block=1"), ENTRY_NAMES[P][0]),             # test_gpu_parity.py:1654
    ((P, 62, 0, 2, False, False, (1, 1), False, ""), ENTRY_NAMES[P][1]),                        # test_gpu_parity.py:1654 (J = 31)
    ((P, 24, 0, 9, True, False, (1, 1), False, ""), ENTRY_NAMES[P][2]),                         # test_gpu_parity.py:1672 (J = 12)
    ((P, 40, 0, 20, True, False, (1, 1), False, ""), ENTRY_NAMES[P][2]),                        # test_gpu_parity.py:1672 (J = 20)
    ((S, 24, 0, 9, True, False, (1, 1), False, ""), ENTRY_NAMES[S][2]),                         # test_gpu_parity.py:1687
    ((S, 6, 0, 3, True, False, (1, 1), False, ""), ENTRY_NAMES[S][2]),                          # test_gpu_parity.py:1687 (J = 3)
    ((S, 64, 0, 3, False, False, (1, 1), False, ""), ENTRY_NAMES[S][0]),                        # test_gpu_parity.py:1739 (J = 32)
    ((S, 142, 0, 2, False, False, (1, 1), False, ""), ENTRY_NAMES[S][0]),                       # test_gpu_parity.py:1739 (J = 71)
    ((P, 64, 0, 3, False, False, (1, 1), False, ""), ENTRY_NAMES[P][0]),                        # test_gpu_parity.py:1744
    ((P, 142, 0, 2, False, False, (1, 1), False, ""), ENTRY_NAMES[P][0]),                       # test_gpu_parity.py:1744
    ((P, 2, 0, 3, False, False, (1, 1), False, ""), ENTRY_NAMES[P][1]),                         # test_gpu_parity.py:1804 (one term: fewer than six rows)
    ((S, 1, 1, 2, False, False, (1, 1), False, ""), ENTRY_NAMES[S][1]),                         # test_gpu_parity.py:1804 (one row)
    ((P, 2, 0, 3, False, False, (1, 1), False, "no_block=1"), ENTRY_NAMES[P][0]),               # test_gpu_parity.py:1811
    ((S, 1, 1, 2, False, False, (1, 1), False, "no_block=1"), ENTRY_NAMES[S][0]),               # test_gpu_parity.py:1811
    ((S, 40, 0, 40, False, False, (1, 1), False, ""), ENTRY_NAMES[S][1]),                       # test_gpu_parity.py:1840
    ((S, 40, 0, 40, False, False, (1, 1), False, "no_block=1"), ENTRY_NAMES[S][0]),             # test_gpu_parity.py:1840
    ((GR, 2, 0, 3, False, False, (1, 1), False, ""), ENTRY_NAMES[GR][1]),                       # test_gpu_parity.py:1938 (J = 1)
    ((GR, 40, 0, 3, False, False, (1, 1), False, ""), ENTRY_NAMES[GR][1]),                      # test_gpu_parity.py:1938 (J = 20)
    ((GR, 40, 0, 3, False, False, (1, 1), False, "no_block=1"), ENTRY_NAMES[GR][0]),            # test_gpu_parity.py:1955
    ((GR, 40, 0, 3, False, False, (0, 0), True, ""), ENTRY_NAMES[GR][1]),                       # test_gpu_parity.py:1969 (series gradients, no d/d(c, d))
    ((GR, 2, 0, 3, False, False, (0, 0), False, "scan_config=tile"), ENTRY_NAMES[GR][3]),       # test_gpu_parity.py:2242 (J = 1, forced)
    ((GR, 30, 0, 5, False, False, (1, 1), False, "scan_config=tile"), ENTRY_NAMES[GR][3]),      # test_gpu_parity.py:2246 (with d/d(c, d))
    ((GR, 30, 0, 5, False, False, (1, 1), False, ""), ENTRY_NAMES[GR][1]),                      # test_gpu_parity.py:2250 (the automatic choice at 5 chains)
    ((GR, 60, 20, 300, False, False, (0, 0), False, ""), ENTRY_NAMES[GR][1]),                   # test_gpu_parity.py:2341 (DRWCelerite-20, 300 chains)
    ((GR, 40, 0, 1024, False, False, (0, 0), False, ""), ENTRY_NAMES[GR][3]),                   # test_gpu_parity.py:2345 (SHO-20, 1024 chains)
    ((GR, 45, 15, 1024, False, False, (0, 0), False, ""), ENTRY_NAMES[GR][3]),                  # test_gpu_parity.py:2345 (DRWCelerite-15)
    ((GR, 60, 20, 1024, False, False, (0, 0), False, ""), ENTRY_NAMES[GR][3]),                  # test_gpu_parity.py:2345 (DRWCelerite-20: four block columns)
    ((GR, 60, 20, 1024, False, False, (0, 0), False, "no_tile=1"), ENTRY_NAMES[GR][1]),         # test_gpu_parity.py:2349
    ((GR, 2, 0, 3, True, False, (1, 1), False, ""), ENTRY_NAMES[GR][2]),                        # test_gpu_parity.py:2386 (J = 1)
    ((GR, 62, 0, 2, True, False, (1, 1), False, ""), ENTRY_NAMES[GR][2]),                       # test_gpu_parity.py:2386 (J = 31)
    ((GR, 40, 0, 6, False, True, (1, 1), False, ""), ENTRY_NAMES[GR][1]),                       # test_gpu_parity.py:2407 (shifted log-flux model)
    ((GR, 40, 0, 6, False, True, (1, 1), False, "no_block=1"), ENTRY_NAMES[GR][0]),             # test_gpu_parity.py:2413
    ((GR, 60, 20, 3, False, False, (1, 1), False, ""), ENTRY_NAMES[GR][1]),                     # test_gpu_parity.py:2433 (DRWCelerite-20, windowed)
    ((GR, 60, 20, 3, False, False, (1, 1), False, "no_block=1"), ENTRY_NAMES[GR][0]),           # test_gpu_parity.py:2433
]


@pytest.mark.parametrize("query,name", PINNED_ENTRY)
def test_entry_routes_the_suite_already_asserts(query, name):
    which, rows, n_one, B, per_draw, shift, cd, series, options = query
    assert entry(which, rows, n_one, B, per_draw, shift, cd, series, options)[0] in ((name,) if isinstance(name, str) else name)


def test_every_entry_name_is_pinned_twice():
    names = [n for _, n in PINNED_ENTRY if isinstance(n, str)]
    for which, table in ENTRY_NAMES.items():
        for n in table:
            assert names.count(n) >= 2, n


ENTRY_B = (1, 2, 256, 257, 512, 513, 1024, 1025, 4096, 4097)
ENTRY_LIMIT = {P: 143, V: 64, GR: 143, S: 143, RP: 143}      # pioran_*_supported_rows*(); rand_posterior: the smaller of prediction's and simulation's
# options that take the windowed kernels away.  scan_config=block is the quirk: any name held in the option string forbids them, so forcing
# the small-batch VALUE kernel sends these entries step by step; scan_config=tile does not (set_option turns it into force_tile)
NO_WINDOWED = ("no_block=1", "force_fallback=1", "scan_config=block")
ENTRY_OPTIONS = ("", "no_tile=1", "scan_config=tile") + NO_WINDOWED


def entry_truth(which, rows, J, B, per_draw, shift, cd, series, options):
    """The rules as the issue that introduced pioran_entry_route lists them: (name, chunk cap, shrink), name None where the entry refuses.
    Up to 63 rows of at most 32 terms always fit the windowed kernels' LDS (celerite_block.hip pioran_block_fits: four block columns)."""
    allowed = lambda R: options not in NO_WINDOWED and R <= 63
    batch = per_draw and B > 1 and which in (P, GR, S) and not (which == GR and shift) and allowed(2 * J)
    if batch:
        rows = 2 * J
    elif per_draw and B > 1:
        B = 1       # draw by draw
    if rows > ENTRY_LIMIT[which]:
        return None, 0, True
    windowed = batch or (which != V and allowed(rows))
    tile = (which == GR and not batch and windowed and cd[0] == cd[1] and not series and not shift and rows <= 63 and
            (options == "scan_config=tile" or (options != "no_tile=1" and B > 512 and rows >= 17)))
    name = ENTRY_NAMES[which][3 if tile else (2 if batch else 1) if windowed else 0]
    cap = 256 if which != GR or batch else 4096 if tile else 512 if windowed else 1024
    return name, cap, not (windowed and not batch and which in (P, S))


def test_entry_properties_over_the_grid():
    """rows 1 .. 150 x B x per draw x the gradient's flags under the default options and every option that forbids or forces a family."""
    n = 0
    seen = set()
    for rows, B, per_draw, options in itertools.product(range(1, 151), ENTRY_B, (False, True), ENTRY_OPTIONS):
        n_one = rows % 2
        J = (rows + n_one) // 2
        for which in (P, V, GR, S, RP):
            flags = itertools.product((False, True), ((1, 1), (0, 0), (1, 0), (0, 1)), (False, True)) if which == GR else (((False, (1, 1), False)),)
            for shift, cd, series in flags:
                q = (which, rows, J, B, per_draw, shift, cd, series, options)
                got = entry(which, rows, n_one, B, per_draw, shift, cd, series, options)
                n += 1
                assert got == entry_truth(*q), (q, got)
                name, cap, shrink = got
                # refused exactly past the entry's rows — whatever the form of (c, d): the draw-by-draw calls refuse the same rows
                assert (name is None) == (rows > ENTRY_LIMIT[which]), q
                if name is None:
                    continue
                assert name in ENTRY_NAMES[which], q
                seen.add(name)
                batch = "per-draw tables" in name
                if name.startswith("tile"):
                    assert not shift and not series and cd[0] == cd[1] and rows <= 63 and options != "no_tile=1" and not batch, q
                    assert options == "scan_config=tile" or (B > 512 and rows >= 17), q
                elif (options == "scan_config=tile" and which == GR and rows <= 63 and not shift and not series and cd[0] == cd[1] and
                      not (per_draw and B > 1)):
                    raise AssertionError(("tile forced and not taken", q, name))
                if options in NO_WINDOWED:
                    assert name.startswith("wide"), q
                if batch:
                    assert per_draw and B > 1 and 2 * J <= 63 and not shift, q
                assert cap == (256 if which != GR or batch else {"tile": 4096, "block": 512, "wide": 1024}[name.split(" ")[0]]), q
                assert shrink == (not (which in (P, S) and name.startswith("block") and not batch)), q
    assert n >= 150 * 10 * 2 * 6 * 20
    # every string the library can report for these entries is in the table the tests pin, and the other way round
    assert seen == {name for table in ENTRY_NAMES.values() for name in table}


@pytest.mark.parametrize("rows,refused", [(63, ()), (64, ()), (65, (V,)), (143, (V,)), (144, (P, V, GR, S, RP))])
def test_entry_row_limits(rows, refused):
    for which in (P, V, GR, S, RP):
        for B, per_draw in ((1, False), (8, False), (8, True)):
            name, cap, shrink = entry(which, rows, rows % 2, B, per_draw)
            assert (name is None) == (which in refused), (which, rows, B, per_draw, name)
            if name is not None and which != V:
                # (63 rows of 32 terms with (c, d) per draw: 2 J = 64 rows refuse the batch form, the one-draw calls keep their one-row term)
                assert name.startswith("block") == (rows <= 63), (which, rows, name)
                assert ("per-draw tables" in name) == (per_draw and rows < 63 and which != RP), (which, rows, name)


def test_entry_argument_validation():
    import ctypes
    L = pj._lib.lib()
    name = ctypes.create_string_buffer(8)
    cap, shrink = ctypes.c_int64(-1), ctypes.c_int(-1)
    args = (0, 0, 1, 1, 0)
    assert L.pioran_entry_route(b"grad", 40, 20, 0, 8, *args, None, name, 8, ctypes.byref(cap), ctypes.byref(shrink)) == 0
    assert name.value == b"block (" and cap.value == 512 and shrink.value == 1        # cut to the buffer
    assert L.pioran_entry_route(b"predict", 40, 20, 0, 8, *args, None, name, 8, None, ctypes.byref(shrink)) == 0 and shrink.value == 0
    assert L.pioran_entry_route(b"predict_var", 66, 33, 0, 8, *args, None, name, 8, ctypes.byref(cap), None) == -4 and name.value == b""
    assert L.pioran_entry_route(b"value", 40, 20, 0, 8, *args, None, name, 8, None, None) == -1
    assert L.pioran_entry_route(None, 40, 20, 0, 8, *args, None, name, 8, None, None) == -1
    assert L.pioran_entry_route(b"grad", 40, 20, 1, 8, *args, None, name, 8, None, None) == -1      # 40 rows are not 20 terms with a one-row term
    assert L.pioran_entry_route(b"grad", 40, 20, 0, 0, *args, None, name, 8, None, None) == -1
    assert L.pioran_entry_route(b"grad", 40, 20, 0, 8, *args, b"no_such_option=1", name, 8, None, None) == -1
    assert L.pioran_entry_route(b"grad", 40, 20, 0, 8, *args, None, None, 8, None, None) == -1


# ---- the step-by-step kernels' instantiations: pioran_step_route (route.hip scan_plan, wide_plan) ---------------------------------------------------

def _listing():
    return json.loads((ROOT / "tests" / "golden" / "step_route_listing.json").read_text())


def test_step_route_reproduces_the_listing_recorded_before_the_rules():
    """tests/golden/step_route_listing.json: what the launch code of celerite_scan.hip / celerite_wide.hip chose before scan_plan / wide_plan existed
    (tools/experiments/step_route_listing.py), over R = 1 .. 80 x row maps x batch classes x tables x options (scan) and R = 1 .. 144 x modes x
    per-draw rows x per-draw tables x options (latency layout): the rules name the same instantiation for every entry."""
    listing = _listing()
    scan_keys, wide_keys = G.step_scan_keys(), G.step_wide_keys()
    assert len(listing["scan"]) == len(scan_keys) and len(listing["wide"]) == len(wide_keys)
    n = 0
    for keys, held, answer, rows in ((scan_keys, listing["scan"], G.step_scan_answer, G.STEP_SCAN_ROWS),
                                     (wide_keys, listing["wide"], G.step_wide_answer, G.STEP_WIDE_ROWS)):
        for key in keys:
            want = listing["answers"][held["|".join(map(str, key))]]
            assert want[0][0] == rows[0] and want[-1][1] == rows[-1]
            for first, last, a in want:
                for R in range(first, last + 1):
                    assert answer(key, R) == a, (key, R)
                    n += 1
    assert n == len(scan_keys) * 80 + len(wide_keys) * 144
    # the DRWCelerite-20 shape is on the grid
    assert G.step_n_complex(2, 60) == 20 and G.step_scan_answer((2, 2049, 1, 0, ""), 60)[0] == "rpl4_cbr4_nsrc4_b5a"


# (rows, row map's kind, two-row terms first, B, options) -> what pioran_celerite_config_name(0) reports after the launch (a tuple: starts with;
# "!...": does not start with), each from an assertion in the GPU suite; shared table, no per-draw rows
STEP_PINNED = [
    ((80, 1, 0, 300, ""), ("rpl5_cbr4_nsrc4",)),                # test_gpu_parity.py:451 (J = 40)
    ((66, 1, 0, 290, ""), ("rpl5_cbr4_nsrc4",)),                # test_gpu_parity.py:451 (J = 33)
    ((72, 1, 0, 301, ""), ("rpl5_cbr4_nsrc4",)),                # test_gpu_parity.py:451 (J = 36)
    ((78, 1, 0, 280, ""), ("rpl5_cbr4_nsrc4",)),                # test_gpu_parity.py:451 (J = 39)
    ((80, 1, 0, 7, ""), ("rpl5_cbr4_nsrc4",)),                  # test_gpu_parity.py:451 (J = 40, seven draws)
    ((70, 2, 25, 300, ""), ("rpl5_cbr4_nsrc4",)),               # test_gpu_parity.py:451 (J = 45, 20 one-row terms)
    ((78, 2, 28, 258, ""), ("rpl5_cbr4_nsrc4",)),               # test_gpu_parity.py:451 (J = 50, 22 one-row terms)
    ((80, 2, 38, 259, ""), ("rpl5_cbr4_nsrc4",)),               # test_gpu_parity.py:451 (J = 42, 4 one-row terms)
    ((76, 2, 32, 3, ""), ("rpl5_cbr4_nsrc4",)),                 # test_gpu_parity.py:451 (J = 44, 12 one-row terms)
    ((30, 1, 0, 2100, ""), "rpl2_cbr1_nsrc16_p+win3"),          # test_gpu_parity.py:577
    ((16, 1, 0, 45, ""), "rpl1_cbr1_nsrc16_yp"),                # test_gpu_parity.py:593 (J = 8)
    ((32, 1, 0, 45, ""), "rpl2_cbr1_nsrc16_yp"),                # test_gpu_parity.py:593 (J = 16)
    ((48, 1, 0, 45, ""), "rpl3_cbr2_nsrc8_yp"),                 # test_gpu_parity.py:593 (J = 24)
    ((64, 1, 0, 70, ""), "rpl4_cbr4_nsrc4_yp"),                 # test_gpu_parity.py:622
    ((64, 2, 30, 9, ""), "rpl4_cbr4_nsrc4_y"),                  # test_gpu_parity.py:639 (30 two-row + 4 one-row terms)
    ((60, 2, 20, 300, ""), "rpl4_cbr4_nsrc4_b5a"),              # test_gpu_parity.py:774 (DRWCelerite-20)
    ((36, 2, 12, 300, ""), "rpl3_cbr2_nsrc7"),                  # test_gpu_parity.py:774 (DRWCelerite-12)
    ((60, 2, 20, 300, "no_paired=1"), "!rpl4_cbr4_nsrc4_b5"),   # test_gpu_parity.py:781
    ((36, 2, 12, 300, "no_paired=1"), "!rpl4_cbr4_nsrc4_b5"),   # test_gpu_parity.py:781
    ((40, 1, 0, 4096, ""), ("rpl",)),                           # test_gpu_configs.py:112 (SHO-20)
    ((60, 2, 20, 4096, ""), ("rpl",)),                          # test_gpu_configs.py:112 (DRWCelerite-20)
] + [((40, 1, 0, 21, f"scan_config={name}"), name)              # test_gpu_parity.py:808-813
     for name in ("rpl3_cbr2_nsrc7_p", "rpl3_cbr2_nsrc8_p", "rpl3_cbr2_nsrc7", "rpl3_cbr2_nsrc8", "rpl3_cbr4_nsrc4", "rpl4_cbr4_nsrc4", "rpl5_cbr4_nsrc4",
                  "rpl4_cbr4_nsrc4_p", "rpl5_cbr4_nsrc4_p")]


@pytest.mark.parametrize("query,want", STEP_PINNED)
def test_step_route_names_the_gpu_suite_asserts(query, want):
    R, kind, nc, B, options = query
    name, plan = G.step_route("scan", R, kind, nc, B, True, 0, False, options)
    if isinstance(want, tuple):
        assert name.startswith(want[0]), name
    elif want.startswith("!"):
        assert not name.startswith(want[1:]), name
    else:
        assert name == want
    assert plan[6] == 1


def test_config_name_of_a_row_count():
    """pioran_celerite_config_name(R), R > 0: the configuration alone, with no launch behind it (tests/test_abi.py:40-43) — the rule asked for a
    large batch without a table."""
    L = pj._lib.lib()
    assert L.pioran_celerite_config_name(40) == b"rpl3_cbr2_nsrc7_p"
    assert L.pioran_celerite_config_name(60).startswith(b"rpl4_cbr4")
    assert L.pioran_celerite_config_name(128) == b"wide" and L.pioran_celerite_config_name(80) == b"wide"
    assert L.pioran_celerite_config_name(144) == b"fallback"
    for R in range(1, 80):
        name, plan = G.step_route("scan", R, 1 - R % 2, 0, 1 << 40, False)
        assert L.pioran_celerite_config_name(R).decode() == name.split("+")[0]


def test_step_route_properties_over_the_grid():
    names = set()
    for key in G.step_scan_keys():
        kind, B, shared, npd, options = key
        opt = dict(kv.split("=") for kv in options.split(";") if kv)
        for R in G.STEP_SCAN_ROWS:
            name, (config, form, shared_tab, mixed, ycol, npb, has_kernel, capacity) = G.step_route("scan", R, kind, G.step_n_complex(kind, R), B, shared, npd,
                                                                                                  False, options)
            if name is None:
                # refused: only what no configuration holds — 80 rows without what the y-as-a-vector shapes need (a name that does not hold the
                # launch leaves the automatic choice, so no refusal comes from it)
                assert config == -1 and R == 80 and not (shared and npd == 0 and "no_win2" not in opt)
                continue
            base = name.split("+")[0]
            names.add(base)
            assert base == G.SCAN_CONFIG_NAMES[0] or base in G.SCAN_CONFIG_NAMES
            assert has_kernel == 1                                       # celerite_scan.hip's table holds a kernel for every plan the rule returns
            assert capacity >= R
            rpl = int(base[3])
            if base.endswith(("_p", "_yp")):                            # a paired configuration only on a standard row map
                assert kind == 1
            assert ycol == base.endswith(("_y", "_yp")) and (not ycol or (shared and npd == 0 and "no_win2" not in opt and form == 2))
            assert (npb > 0) == base.endswith("_b5a") and (npb == 0 or (kind == 2 and shared and npd == 0 and form in (1, 2)))
            assert name.endswith("+win3") == (form == 3) and (form != 3 or (shared and npd == 0 and rpl in (2, 3) and not ycol and npb == 0))
            assert shared_tab == shared and mixed == (shared and npd > 0)
            # a forbidding option is honoured; a forcing one too, where the form exists
            if "no_win3" in opt or "no_win2" in opt or "win2" in opt:
                assert form != 3
            if "no_win2" in opt:
                assert form == 1
            if "win2" in opt:
                assert form == 2
            if "win3" in opt and shared and npd == 0 and rpl in (2, 3) and not ycol and npb == 0:
                assert form == 3
            if "no_paired" in opt:
                assert not base.endswith(("_p", "_yp", "_b5a"))
            if "scan_config" not in opt and base == "rpl2_cbr2_nsrc8":   # the mid-batch shape: up to 2048 draws of 24 .. 31 rows
                assert B <= 2048 and 24 <= R <= 31
            if "scan_config" in opt and base != opt["scan_config"]:      # the named configuration does not hold the launch: the automatic choice — but
                # any name turns the mid-batch shape off, so the configuration is that of a batch above 2048 draws
                assert base == G.step_route("scan", R, kind, G.step_n_complex(kind, R), 2049, shared, npd, False, "")[0].split("+")[0]
    assert names == set(G.SCAN_CONFIG_NAMES)                             # every configuration of the list is reached
    for key in G.step_wide_keys():
        mode, npd, per_draw_tables, options = key
        for R in G.STEP_WIDE_ROWS:
            name, (rpl, lean, ycol, lean_adjoint, *_) = G.step_route(mode, R, 0, 0, 1, True, npd, per_draw_tables, options)
            if name is None:
                continue
            assert R <= 143 and rpl == (R // 16 if ycol else R // 16 + 1)
            assert not ycol or (mode == "value" and lean and R % 16 == 0 and npd == 0)
            # celerite_wide_kernel: up to 95 rows of one shared table, the record staged in LDS (the gradient entry does not read per_draw_tables)
            assert lean or (R <= 95 and (not per_draw_tables or mode == "gradient") and 3 * (R + 2) + 2 + 3 * npd <= 512)
            assert not lean_adjoint or mode == "gradient"
            if mode == "gradient":
                assert npd == 0 and (not lean or lean_adjoint) and (rpl < 7 or lean)
                if options == "no_wide2=1":
                    assert lean == (rpl >= 7) == lean_adjoint
            elif options == "no_wide2=1":
                assert lean == (R > 95 or per_draw_tables)               # (store, simulate: per-draw tables are refused above)
            if mode in ("store", "simulate"):
                assert not per_draw_tables and (not lean or npd == 0) and (options != "wide2=1" or lean == (R >= 64 and npd == 0))


# ---- the windowed, tile and time-parallel kernels' instantiations: pioran_window_route (route.hip block_plan, tile_plan, tp_step_plan) -----------------

def test_window_route_reproduces_the_listing_recorded_before_the_rules():
    """tests/golden/window_route_listing.json: the kernels, threads per workgroup and dynamic LDS bytes the launch code of celerite_block.hip,
    celerite_tile.hip and celerite_tp.hip chose before block_plan / tile_plan / tp_step_plan existed (tools/experiments/window_route_listing.py), over
    the grid of route_grid.window_keys: the rules give the same return code, the same kernel instantiations in the same order and, for the kernel the
    plan sizes (the forward kernel; the tile adjoint, the time-parallel boundary phase), the same threads and LDS bytes for every entry, and the files'
    tables hold a kernel for every plan that is not refused.  The threads of the kernels that run behind the forward one are fixed in the launch code and
    in route_grid.window_kernels alike: this test holds the rule, not the launcher's lookup, which tests/test_gpu_window_route.py runs."""
    listing = json.loads((ROOT / "tests" / "golden" / "window_route_listing.json").read_text())
    n = 0
    for family, (keys, xs_of) in G.window_keys().items():
        assert len(listing[family]) == len(keys)
        for key in keys:
            xs = list(xs_of(key))
            for x, want in G.window_expand(listing["runs"][listing[family]["|".join(map(str, key))]], xs):
                q = G.window_query(family, key, x)
                rc, name, plan = G.window_route(family, **q)
                got = rc if rc else G.window_kernels(family, plan, q.get("tp_segments", 2))
                assert got == want, (family, key, x, name)
                assert (name == "none") == (rc != 0)
                if rc == 0:
                    assert plan[11 if family == "tp" else 8] == 1, (family, key, x, name)       # *_kernel_exists
                n += 1
    assert n == 268864
    # the shapes of the benchmarks are on the grid: SHO-20 and DRWCelerite-20 at 512 draws, pair table from global memory, two workgroups per CU
    assert G.window_route("block", R=40, J=20, B=512)[1] == "block_nb3_e2_pd0" and G.window_route("block", R=60, J=40, B=512)[1] == "block_nb4_e0_pd0"


def test_window_route_names_are_one_to_one_with_the_kernels():
    """Two entries of the grid have the same name exactly where they run the same kernel instantiations."""
    by_name = {}
    for family, (keys, xs_of) in G.window_keys().items():
        for key in keys[::7]:
            for x in xs_of(key):
                q = G.window_query(family, key, x)
                rc, name, plan = G.window_route(family, **q)
                if rc == 0:
                    kernels = tuple(k[0] for k in G.window_kernels(family, plan, 2))
                    assert by_name.setdefault(name, kernels) == kernels, name
    assert len(set(by_name.values())) == len(by_name) > 100


def test_launchers_read_no_selection_option():
    """celerite_block.hip, celerite_tile.hip and celerite_tp.hip ask the rules: none names an option the choice goes by."""
    for f in ("celerite_block.hip", "celerite_tile.hip", "celerite_tp.hip"):
        text = (ROOT / "pioran.jl_amd" / "csrc" / f).read_text()
        for word in ("block_emode", "exp & 16", "tp_scan_lean", "tp_scan_waves"):
            assert word not in text, (f, word)


def test_window_route_argument_validation():
    name = __import__("ctypes").create_string_buffer(96)
    L = pj._lib.lib()
    assert L.pioran_window_route(b"block", 40, 20, 1, 0, 0, 0, 0, 0, 0, b"block_emode", name, len(name), None) == -1     # an option without a value
    assert L.pioran_window_route(b"wide", 40, 20, 1, 0, 0, 0, 0, 0, 0, b"", name, len(name), None) == -1
    assert L.pioran_window_route(b"block", 144, 72, 1, 0, 0, 0, 0, 0, 0, b"", name, len(name), None) == -4 and name.value == b"none"
