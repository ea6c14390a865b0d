#!/usr/bin/env python3
"""Static counts of the window loop of the celerite_tile_kernel instantiations (reads a `hipcc -S --cuda-device-only` listing of celerite_tile.hip made
with build.py's flags).  usage: tile_isa_stats.py tile.s [NB KL ST SER] ...   (no selection: every instantiation)
literal_address_adds: the loop's v_add_u32 of a literal and a register the loop never writes (an LDS address a base register could hold).
tests/test_tile_isa.py and tests/test_gpu_tile_table_products.py import kernel_stats()."""
import re
import sys
from collections import Counter

NAME = re.compile(r'^(_ZN12_GLOBAL__N_120celerite_tile_kernelILi(\d+)ELi(\d+)ELb([01])ELb([01])EEEv10ScanParamsPKdS\d+_):', re.M)


LIT_ADD = re.compile(r'^v_add_u32_e32 v\d+, (?:0x[0-9a-f]+|\d+), v(\d+)$')


def _written_vgprs(line: str) -> set:
    """VGPR numbers an instruction line writes: its first operand (v7 or v[4:7]); stores, compares into SGPRs and s_* write none (the DPP updates
    of the inline assembly write their first operand too)."""
    parts = line.split(None, 1)
    if len(parts) < 2 or parts[0].startswith(('s_', 'ds_write', 'buffer_store', 'global_store', ';')):
        return set()
    mm = re.match(r'v(\d+)\b|v\[(\d+):(\d+)\]', parts[1])
    if not mm:
        return set()
    if mm.group(1):
        return {int(mm.group(1))}
    return set(range(int(mm.group(2)), int(mm.group(3)) + 1))


def _meta(listing: str, name: str) -> dict:
    """the kernel's entry of the amdhsa.kernels metadata"""
    k = listing.find('.name:           ' + name + '\n')
    if k < 0:
        return {}
    a = listing.rfind('  - .agpr_count', 0, k)
    a = a if a >= 0 else listing.rfind('  - .args', 0, k)
    b = listing.find('\n  - ', k)
    blk = listing[a:b if b > 0 else len(listing)]
    return {m.group(1): int(m.group(2)) for m in re.finditer(r'\.(\w+):\s+(\d+)\s*$', blk, re.M)}


def kernel_stats(listing: str) -> dict:
    """{(NB, KL, ST, SER): {"loop": Counter of mnemonics inside the window loop, "meta": metadata integers}}; the window loop is the longest backward branch."""
    out = {}
    for m in NAME.finditer(listing):
        name = m.group(1)
        body = listing[m.start():listing.index('.Lfunc_end', m.start())].split('\n')
        labels = {}
        for idx, l in enumerate(body):
            mm = re.match(r'^(\.LBB\d+_\d+):', l)
            if mm:
                labels[mm.group(1)] = idx
        loops = []
        for idx, l in enumerate(body):
            mm = re.search(r's_c?branch\w* (\.LBB\d+_\d+)', l)
            if mm and labels.get(mm.group(1), idx) < idx:
                loops.append((idx - labels[mm.group(1)], labels[mm.group(1)], idx))
        c = Counter()
        lit_adds = 0
        if loops:
            _, a, b = max(loops)
            written = set()
            for l in body[a:b + 1]:
                l = l.strip()
                if not l or l.startswith(('.', ';')) or l.endswith(':'):
                    continue
                c[l.split()[0]] += 1
                written.update(_written_vgprs(l))
            # address sums that a base register could hold: v_add_u32 of a literal and a register the loop never writes
            for l in body[a:b + 1]:
                mm = LIT_ADD.match(l.strip())
                if mm and int(mm.group(1)) not in written:
                    lit_adds += 1
        key = (int(m.group(2)), int(m.group(3)), bool(int(m.group(4))), bool(int(m.group(5))))
        out[key] = {"loop": c, "meta": _meta(listing, name), "literal_address_adds": lit_adds}
    return out


def summary(st: dict) -> str:
    c, md = st["loop"], st["meta"]
    valu = sum(v for k, v in c.items() if k.startswith('v_'))
    lanes = c['v_readlane_b32'] + c['v_writelane_b32']
    return (f"loop={sum(c.values())} v_*={valu} mfma={c['v_mfma_f64_16x16x4_f64']} lane_moves={lanes} v_cndmask={c['v_cndmask_b32_e32'] + c['v_cndmask_b32_e64']} "
            f"v_mov_b64={c['v_mov_b64_e32']} branches={sum(v for k, v in c.items() if k.startswith(('s_cbranch', 's_branch')))} vgpr={md.get('vgpr_count')} "
            f"literal_address_adds={st.get('literal_address_adds')} agpr={md.get('agpr_count')} sgpr_spill={md.get('sgpr_spill_count')} vgpr_spill={md.get('vgpr_spill_count')} scratch={md.get('private_segment_fixed_size')}")


if __name__ == "__main__":
    stats = kernel_stats(open(sys.argv[1]).read())
    sel = [tuple(int(x) for x in sys.argv[i:i + 4]) for i in range(2, len(sys.argv) - 3, 4)]
    for key in sorted(stats):
        if sel and tuple(int(x) for x in key) not in sel:
            continue
        print(f"<{key[0]}, {key[1]}, {str(key[2]).lower()}, {str(key[3]).lower()}>: {summary(stats[key])}")
