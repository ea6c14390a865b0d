"""CPU tests (-m "not gpu") on the gfx950 assembly of the windowed kernels, compiled with exactly build.py's flags (skipped where no hipcc is found):

* tools/check_dpp_hazards.py finds no DPP read of a register too soon after its write (the inline-assembly LDL' of window_common.h / ldl_steps.inc is not
  interlocked: celerite_tile.hip, celerite_block.hip and dense.hip all carry it);
* the headline instantiation celerite_tile_kernel<3, 2, false, false> (SHO-20 without per-draw series) keeps its window loop free of scalar spills and of the lane
  moves that reload them, issues the 76 matrix instructions of the formulation, and stays within 216 vector registers: two such wavefronts then leave 80
  registers of a SIMD's 512, one wavefront of the 70-register pair pre-pass."""
import importlib.util
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_build = _load("_pioran_build_isa", ROOT / "pioran.jl_amd" / "build.py")
_stats = _load("_pioran_tile_isa_stats", ROOT / "tools" / "tile_isa_stats.py")


@pytest.fixture(scope="module")
def listing_of(tmp_path_factory):
    try:
        cc = _build.hipcc()
    except RuntimeError:
        pytest.skip("no hipcc")
    out = tmp_path_factory.mktemp("isa")
    made = {}

    def make(src: str) -> Path:
        if src not in made:
            path = out / (Path(src).stem + ".s")
            subprocess.run([cc, *_build.FLAGS, *_build.EXTRA_FLAGS.get(src, []), "-S", "--cuda-device-only", str(_build.CSRC / src), "-o", str(path)], check=True)
            made[src] = path
        return made[src]

    return make


@pytest.mark.parametrize("src", ["celerite_tile.hip", "celerite_block.hip", "dense.hip"])
def test_no_dpp_hazards(listing_of, src):
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "check_dpp_hazards.py"), str(listing_of(src))], capture_output=True, text=True)
    last = r.stdout.strip().splitlines()[-1]
    assert r.returncode == 0 and last.endswith(" 0 hazard(s)"), r.stdout[-2000:]
    assert int(last.split()[1]) >= 120          # the 16 x 16 LDL' alone has 120 DPP updates: the check saw the kernels


def test_headline_tile_kernel_window_loop(listing_of):
    stats = _stats.kernel_stats(listing_of("celerite_tile.hip").read_text())
    # every (NB, KL) without the gradient's store exists with and without per-draw series; the gradient's forward pass only without
    for nb in range(1, 7):
        for kl in range(0 if nb > 1 else 1, 5):
            assert (nb, kl, False, False) in stats and (nb, kl, False, True) in stats, (nb, kl)
    assert not any(st and ser for (_, _, st, ser) in stats)
    head = stats[(3, 2, False, False)]
    loop, meta = head["loop"], head["meta"]
    print(_stats.summary(head))
    assert loop["v_mfma_f64_16x16x4_f64"] == 76
    assert loop["v_readlane_b32"] == 0 and loop["v_writelane_b32"] == 0
    assert meta["sgpr_spill_count"] == 0
    assert meta["vgpr_spill_count"] == 0
    assert meta["vgpr_count"] <= 216
