"""GPU tests (-m gpu): the windowed, tile and time-parallel launches run the kernel instantiations their rule names (csrc/route.hip block_plan,
tile_plan and tp_step_plan, asked through pioran_window_route) at the points of tools/route_grid.py window_points().  Windowed and tile: N = 37, two
full windows and a ragged one of five steps; three draws, and 257 where the rule reads B > 256; five draws on the tile kernel (the second workgroup
ragged), seven on its gradient (ragged for two, three and four adjoint wavefronts); a point per block-column count, the K-step edges of three block
columns, a series per draw, per-draw rows at two and four block columns, d/d(c, d) on and off.  Time-parallel: N = 64 in four segments (two scan
levels), 2 .. 64 state rows, the walk unchecked, the scan with its verification launch, and the default repair pass — after which the last launch is
the windowed kernel's.  pioran_celerite_config_name(-2) after the call is the name the rule gives; finite values and status 0.  That the
instantiations are the ones the launch code chose before the rules existed is tests/test_route.py's listing."""
import importlib.util
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import pioran_jl_amd as pj  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]
_spec = importlib.util.spec_from_file_location("route_grid", ROOT / "tools" / "route_grid.py")
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)

FAMILY = {"block": "block", "block_grad": "block (windowed gradient)", "block_solve": "block (windowed prediction)",
          "block_sim": "block (windowed simulation)", "tile": "tile", "tile_grad": "tile (windowed gradient, one draw per wavefront)", "tp": "tp"}


def test_windowed_tile_and_time_parallel_launches_run_the_instantiations_the_rules_name():
    ctx = pj.Context(0)
    seen = set()
    for pt in G.window_points():
        want = G.window_expected(pt)
        family, got, out = G.run_window_point(ctx, pt)
        assert family == ("block+pd" if pt.npd_rows else FAMILY[pt.family]) and got == want, (pt, family, got, want)
        assert (out.get("status", np.zeros(1)) == 0).all(), (pt, got)
        for key, v in out.items():
            assert np.isfinite(v).all(), (pt, got, key)
        seen.add(got)
    # one name per branch of each rule.  Windowed value: the block columns; the pair table in one LDS buffer, in two and in global memory (above 256
    # draws, forced, and at five and six block columns); per-draw rows on the helper wavefront, on the chain wavefront, and there with two workgroups per CU
    assert {"block_nb1_e0_pd0", "block_nb2_e0_pd0", "block_nb3_e0_pd0", "block_nb3_e1_pd0", "block_nb3_e2_pd0", "block_nb4_e0_pd0", "block_nb5_e2_pd0",
            "block_nb6_e2_pd0", "block_nb2_e1_pd1", "block_nb2_e2_pd2", "block_nb4_e0_pd2"} <= seen, seen
    # ... gradient: the forward pass with one and two workgroups per CU, never two at four block columns; d/d(c, d); four contraction threads per term
    assert {"block_nb1_e0+adjoint_8", "block_nb3_e2+adjoint_8", "block_nb3_e2+adjoint_cd_8", "block_nb4_e0+adjoint_8", "block_nb4_e0+adjoint_cd_8",
            "block_nb3_e0+adjoint_4", "block_nb1_e0+backsolve", "block_nb4_e0+backsolve", "block_nb1_e0+sim", "block_nb4_e0+sim"} <= seen, seen
    # tile: the block columns, every K-step count of three block columns, a series per draw; the adjoint's draws per workgroup
    assert {"tile_nb1_kl2", "tile_nb2_kl1", "tile_nb4_kl3", "tile_nb5_kl2", "tile_nb6_kl3", "tile_nb3_kl0", "tile_nb3_kl1", "tile_nb3_kl2", "tile_nb3_kl3",
            "tile_nb3_kl4", "tile_nb3_kl2_ser", "tile_nb1_kl4_st+adjoint_w4", "tile_nb3_kl4_st+adjoint_cd_w4", "tile_nb4_kl4_st+adjoint_w3",
            "tile_nb4_kl4_st+adjoint_cd_w2"} <= seen, seen
    # time-parallel: the three walks, one and four wavefronts per segment, the scan at one, two and four tiles of rows with its verification, lean on request
    assert {"tp_np1x1+small2", "tp_np2x1+small4", "tp_np4x1+wave8", "tp_np6x1+wave12", "tp_np2x4+wave16", "tp_np3x4+boundary_rt2", "tp_np8x4+boundary_rt4",
            "tp_np4x1+combine_rt1_w4+verify_wave8", "tp_np2x4+combine_rt1_w4+verify_wave16", "tp_np3x4+combine_rt2_w8+verify_boundary_rt2",
            "tp_np8x4+combine_lean_rt4_w8+verify_boundary_rt4", "tp_np3x4+combine_lean_rt2_w8+verify_boundary_rt2"} <= seen, seen
