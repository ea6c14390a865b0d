"""GPU tests (-m gpu): the step-by-step launches run the kernel instantiation their rule names (csrc/route.hip scan_plan and wide_plan, asked through
pioran_step_route) at the points of tools/route_grid.py step_points() — N = 37, one launch on each side of every rule: the throughput layout at
15 .. 80 rows (and the batch classes 5, 2048, 2049 draws where the rule reads the batch), the 60-row DRWCelerite-20 shape, and the latency
layout's four modes at three draws, 47 .. 96 rows.  pioran_celerite_config_name(0) after the launch is the name the rule gives; finite values
and status 0.  That the instantiations are the ones the launch code chose before the rules existed is tests/test_route.py's listing."""
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

FAMILY = {"scan": "scan", "value": "wide", "store": "wide (step-by-step prediction)", "simulate": "wide (step-by-step simulation)",
          "gradient": "wide (step-by-step gradient)"}


def test_step_by_step_launches_run_the_instantiation_the_rule_names():
    ctx = pj.Context(0)
    seen = set()
    for pt in G.step_points():
        want = G.step_expected(pt)
        family, got, out = G.run_step_point(ctx, pt)
        assert family == FAMILY[pt.family] and got == want, (pt, family, got, want)
        assert (out.get("status", np.zeros(1)) == 0).all(), (pt, got)
        for key, v in out.items():
            assert np.isfinite(v).all(), (pt, got, key)
        seen.add(got)
    # both sides of the rules were crossed: the forms, the mid-batch shape, y as a vector, the block layout; the latency layout's kernels
    assert {"rpl2_cbr1_nsrc13_p+win3", "rpl2_cbr1_nsrc16+win3", "rpl2_cbr2_nsrc8", "rpl2_cbr1_nsrc16_yp", "rpl4_cbr4_nsrc4_b5a", "rpl5_cbr4_nsrc4_yp",
            "wide_rpl3", "wide2_rpl3", "wide2_rpl3_y", "wide_rpl4", "wide2_rpl4_y", "wide_rpl5", "wide2_rpl5", "wide_rpl3+adjoint", "wide_rpl3+adjoint2",
            "wide2_rpl4+adjoint2", "wide_rpl6+adjoint", "wide2_rpl7+adjoint2"} <= seen, seen
