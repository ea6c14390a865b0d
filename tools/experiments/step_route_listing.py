#!/usr/bin/env python3
"""Writes tests/golden/step_route_listing.json: which kernel instantiation the step-by-step launches ran BEFORE their choice became the rules
scan_plan / wide_plan of csrc/route.hip, over the grid of tools/route_grid.py (step_scan_keys, step_wide_keys).

The listing comes from a copy of the commit before those rules, with step_route_record.patch applied: SCAN_LAUNCH and the latency layout's
launches record the kernel's template arguments instead of launching, and pioran_record_step asks them without a device:

    git worktree add /tmp/before <commit before scan_plan> && git -C /tmp/before apply $PWD/tools/experiments/step_route_record.patch
    python /tmp/before/pioran.jl_amd/build.py
    python tools/experiments/step_route_listing.py /tmp/before/pioran.jl_amd/libpioran_hip.so

Format: "answers" holds every distinct list of runs [first row, last row, answer] once; "scan" / "wide" map a key of the grid to its list.
A scan answer is [name, steps per pass, shared table, per-draw rows, y as a vector, pairs per block]; a latency answer [name, kernels in launch
order as [template, rows per lane, y as a vector, mode]] — the names are those of the rules (the recorded commit had none for the latency
layout: the listing spells them from the recorded template arguments); null: the launch is refused."""
import ctypes
import importlib.util
import json
import re
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
spec = importlib.util.spec_from_file_location("route_grid", ROOT / "tools" / "route_grid.py")
G = importlib.util.module_from_spec(spec)
spec.loader.exec_module(G)

L = ctypes.CDLL(sys.argv[1])
L.pioran_record_step.restype = ctypes.c_char_p
L.pioran_record_step.argtypes = [ctypes.c_char_p] + [ctypes.c_int32] * 3 + [ctypes.c_int64, ctypes.c_int, ctypes.c_int32, ctypes.c_int, ctypes.c_char_p]


def record(family, R, kind, nc, B, shared, npd, per_draw_tables, options):
    return L.pioran_record_step(family.encode(), R, kind, nc, B, shared, npd, per_draw_tables, options.encode()).decode()


def scan_answer(key, R):
    kind, B, shared, npd, options = key
    rec = record("scan", R, kind, G.step_n_complex(kind, R), B, shared, npd, 0, options)
    if not rec:
        return None
    name, cfg, kern = rec.split("|")
    rpl, cbr, nsrc, paired, npb, ycol = map(int, cfg.split())
    # celerite_scan_kernel<RPL, CBR, NSRC, SHARED_TAB, MINW, PAIRED, MIXED, NPB, WIN2, YC, WIN3>, trailing defaults false / 0
    args = [a.strip() for a in re.search(r"<(.*)>", kern).group(1).split(",")]
    args += ["false", "0", "false", "false", "false"][len(args) - 6:] if len(args) < 11 else []
    flag = lambda a: {"true": 1, "false": 0}[a]
    assert args[:3] == ["RPL", "CBR", "NSRC"] and args[7] in ("0", "NPB") and (args[7] == "NPB") == (npb > 0)
    assert flag(args[9]) == ycol and (args[5] == "PAIRED" or flag(args[5]) == paired) and name.endswith("+win3") == bool(flag(args[10]))
    form = 3 if flag(args[10]) else (2 if flag(args[8]) else 1)
    return [name, form, flag(args[3]), flag(args[6]), ycol, npb]


def wide_answer(key, R):
    mode, npd, per_draw_tables, options = key
    rc, kerns = record(mode, R, 0, 0, 1, 1, npd, per_draw_tables, options).split("|")
    if int(rc):
        assert not kerns
        return None
    out = []
    for k in kerns.split(";")[:-1]:
        if "grad_finish_kernel" in k:
            continue
        text, rpl_var = k.split("@")
        m = re.match(r"\(?(celerite_\w+)<([^>]*)>\)?", text)
        args = [a.strip() for a in m.group(2).split(",")]
        rpl = int(rpl_var) if args[0] == "RPL" else int(args[0])
        if m.group(1) == "celerite_wide_kernel":          # <RPL, MODE = 0>
            md = args[1] if len(args) > 1 else "0"
            out.append([m.group(1), rpl, 0, G.STEP_WIDE_MODES.index(mode) if md == "MODE" else int(md)])
        elif m.group(1) == "celerite_wide2_kernel":       # <RPL, YC = false, SM = 0>
            md = args[2] if len(args) > 2 else "0"
            out.append([m.group(1), rpl, int(len(args) > 1 and args[1] == "true"), G.STEP_WIDE_MODES.index(mode) if md == "MODE" else int(md)])
        else:
            out.append([m.group(1), rpl, 0, 0])
    fwd = out[0]
    name = f"{'wide2' if fwd[0] == 'celerite_wide2_kernel' else 'wide'}_rpl{fwd[1]}{'_y' if fwd[2] else ''}"
    if mode == "gradient":
        name += "+adjoint2" if out[1][0] == "celerite_adjoint2_kernel" else "+adjoint"
    return [name, out]


answers, index = [], {}


def intern(runs):
    k = json.dumps(runs)
    if k not in index:
        index[k] = len(answers)
        answers.append(runs)
    return index[k]


listing = {"answers": answers, "scan": {}, "wide": {}}
for key in G.step_scan_keys():
    listing["scan"]["|".join(map(str, key))] = intern(G.step_runs([(R, scan_answer(key, R)) for R in G.STEP_SCAN_ROWS]))
for key in G.step_wide_keys():
    listing["wide"]["|".join(map(str, key))] = intern(G.step_runs([(R, wide_answer(key, R)) for R in G.STEP_WIDE_ROWS]))
out = ROOT / "tests" / "golden" / "step_route_listing.json"
out.write_text(json.dumps(listing, separators=(",", ":")) + "\n")
print(f"{out}: {len(listing['scan'])} + {len(listing['wide'])} keys, {len(answers)} distinct run lists, {out.stat().st_size} bytes")
