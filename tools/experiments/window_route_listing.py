#!/usr/bin/env python3
"""Writes tests/golden/window_route_listing.json: which kernel instantiations the windowed, tile and time-parallel launches ran BEFORE their choice
became the rules block_plan / tile_plan / tp_step_plan of csrc/route.hip, over the grid of tools/route_grid.py (window_keys).

The listing comes from a copy of the commit before those rules, with window_route_record.patch applied: every launch of celerite_block.hip,
celerite_tile.hip and celerite_tp.hip records the kernel's template arguments, threads per workgroup and dynamic LDS bytes instead of launching, the
runtime calls around them are stubbed, and pioran_record_window asks the launch entries without a device:

    git worktree add /tmp/before <commit before block_plan> && git -C /tmp/before apply $PWD/tools/experiments/window_route_record.patch
    python /tmp/before/pioran.jl_amd/build.py
    python tools/experiments/window_route_listing.py /tmp/before/pioran.jl_amd/libpioran_hip.so

Format: "runs" holds every distinct list of runs once (route_grid.window_runs: [last value of the swept variable, answer], the answer a return code or
the kernels as [name<template arguments>, threads, LDS bytes at 0, LDS bytes per unit of the variable]); every family maps a key of the grid to its
list.  Not listed, because no rule chooses them: the tile family's pair pre-pass, tp_records_kernel, tp_finish_kernel; the scan's repeated launches
of one combination kernel count once."""
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
L.pioran_record_window.restype = ctypes.c_char_p
L.pioran_record_window.argtypes = [ctypes.c_char_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int64, ctypes.c_int32, ctypes.c_int, ctypes.c_int, ctypes.c_int32,
                                   ctypes.c_int32, ctypes.c_int, ctypes.c_char_p]
UNLISTED = ("tile_pairs_mfma_kernel", "tp_records_kernel", "tp_finish_kernel")


def answer(family, key, x):
    q = dict(R=0, J=0, B=1, npd_rows=0, per_draw_series=False, want_cd=False, tp_rows=0, tp_segments=0, tp_mode=0, options="")
    q.update(G.window_query(family, key, x))
    rec = L.pioran_record_window(family.encode(), q["R"], q["J"], q["B"], q["npd_rows"], int(q["per_draw_series"]), int(q["want_cd"]), q["tp_rows"],
                                 q["tp_segments"], q["tp_mode"], q["options"].encode()).decode()
    rc, kerns = rec.split("|")
    if int(rc):
        assert not kerns, rec
        return int(rc)
    out = []
    for k in kerns.split(";")[:-1]:
        text, threads, lds = k.rsplit("@", 2)
        m = re.search(r"\(anonymous namespace\)::(\w+?)(<[^>]*>)?[(>]", text[text.index("&"):])
        if m.group(1) in UNLISTED:
            continue
        entry = [m.group(1) + m.group(2).replace(" ", ""), int(threads), int(lds)]
        if not out or out[-1] != entry:
            out.append(entry)
    return out


runs, index = [], {}


def intern(r):
    k = json.dumps(r)
    if k not in index:
        index[k] = len(runs)
        runs.append(r)
    return index[k]


listing, n = {"runs": runs}, 0
for family, (keys, xs_of) in G.window_keys().items():
    listing[family] = {}
    for key in keys:
        xs = list(xs_of(key))
        answers = [(x, answer(family, key, x)) for x in xs]
        held = G.window_runs(answers)
        assert G.window_expand(held, xs) == answers, (family, key)
        listing[family]["|".join(map(str, key))] = intern(held)
        n += len(xs)
out = ROOT / "tests" / "golden" / "window_route_listing.json"
out.write_text(json.dumps(listing, separators=(",", ":")) + "\n")
print(f"{out}: {n} entries under {sum(len(v) for k, v in listing.items() if k != 'runs')} keys, {len(runs)} distinct run lists, {out.stat().st_size} bytes")
