"""CPU tests of the routing rules of the value path (csrc/route.hip) through pioran_value_route: the family the ladder of capi.hip's launch()
takes when every resource is granted.  Routes the GPU tests already assert, transcribed; properties over a grid of ~89 000 queries; the
time-parallel plans against the conditions pioran_launch_tp refuses on."""
import importlib.util
import itertools
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
