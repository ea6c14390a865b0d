"""GPU tests (-m gpu): the batched entries besides the value path — posterior mean and variance, value and gradient, simulation, posterior draws —
run the kernels their rule names (csrc/route.hip entry_plan, asked through pioran_entry_route) at every point of tools/route_grid.py
entry_points(): N = 130 (nine 16-step windows, the last ragged), 7 evaluation times, rows and batches either side of every threshold, the
options that forbid or force a family, (c, d) per draw on per-draw tables and draw by draw.  The name that ran, the return code, status 0 and
finite values; what the values are is the truth tests' business, and that the plans are the ones the code made before the rules were written
down is docs/EXPERIMENTS.md section 30's listing against the parent's library."""
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


def test_entries_take_the_plan_the_rule_names():
    ctx = pj.Context(0)
    seen = set()
    for pt in G.entry_points():
        want = G.entry_expected(pt)[0]
        got, rc, out = G.run_entry_point(ctx, pt)
        assert got == want and rc == (0 if want else -4), (pt, got, rc, want)
        if want is None:
            continue
        seen.add(got)
        assert (out.get("status", np.zeros(1)) == 0).all(), (pt, got)
        for key, v in out.items():
            assert np.isfinite(v).all(), (pt, got, key)
    assert seen == {n for names in G.ENTRY_NAME_TABLE.values() for n in names}
