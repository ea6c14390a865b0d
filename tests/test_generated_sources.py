"""CPU test (-m "not gpu"): the generated kernel text in the tree is, byte for byte, what its generator writes —
pioran.jl_amd/csrc/ldl_steps.inc (tools/gen_ldl_steps.py) and the column blocks between the GENERATED markers of celerite_scan.hip (tools/gen_scan_win2.py)."""
import importlib.util
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "pioran.jl_amd" / "csrc"


def _load(name):
    spec = importlib.util.spec_from_file_location("_pioran_" + name, ROOT / "tools" / (name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_ldl_steps_inc_is_the_generators_text():
    assert (CSRC / "ldl_steps.inc").read_text() == _load("gen_ldl_steps").generate()


def test_scan_column_blocks_are_the_generators_text():
    gen = _load("gen_scan_win2")
    text = (CSRC / "celerite_scan.hip").read_text()
    assert text.count(gen.BEGIN) == 1 and text.count(gen.END) == 1
    section = text[text.index(gen.BEGIN):text.index(gen.END) + len(gen.END)]
    assert section == gen.generate()
    # every column block of the file lives in that section: none is written by hand outside it
    rest = text.replace(section, "")
    assert "PD_FMAC(" not in rest.replace("#define PD_FMAC(", "") and "struct Update" not in rest and "struct Pair" not in rest
