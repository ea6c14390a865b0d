"""CPU tests (-m "not gpu") of the workgroup mapping of the tile family's pair pre-pass: pioran_tile_pairs_slot exports tile_pairs_slot (common.h), the
function tile_pairs_mfma_kernel itself calls to find its chunk of windows and its block of 64 draws from its place in the launch order.

* The decode is a bijection from 0 .. nchunk * ndb - 1 onto (chunk, draw block): every slot of the workspace is written, and by one workgroup.
* The property the mapping exists for.  Workgroups start in the order of their ids and go to the eight XCDs, each with an L2 of its own, in turn: ids
  equal modulo 8 share an L2, and ids 8 apart are neighbours in its launch order.  On the whole eights of chunks, whose ids come first, all ids of one
  chunk are congruent to the chunk modulo 8 (one L2 reads one eighth of the pair table and keeps it), the draw blocks are taken in groups of four (the last
  group: what is left), one group after the other, and the ids of one chunk and group are 8 apart, in the order of the draw blocks: those workgroups run
  side by side, and the L2 fetches the chunk once for all of them.  The nchunk mod 8 chunks that are left follow, in the same groups, the ids of one
  chunk and group adjacent.
* Ids outside the range are refused."""
import ctypes

import pytest

import pioran_jl_amd as pj

NCHUNK = (1, 2, 7, 8, 9, 125, 126)
NDB = (1, 2, 7, 8, 9, 64, 65)
GROUP = 4


def slot(i, nchunk, ndb):
    chunk, db = ctypes.c_int64(-1), ctypes.c_int64(-1)
    rc = pj._lib.lib().pioran_tile_pairs_slot(i, nchunk, ndb, ctypes.byref(chunk), ctypes.byref(db))
    return rc, chunk.value, db.value


@pytest.mark.parametrize("ndb", NDB)
@pytest.mark.parametrize("nchunk", NCHUNK)
def test_slot_is_a_bijection(nchunk, ndb):
    seen = set()
    for i in range(nchunk * ndb):
        rc, chunk, db = slot(i, nchunk, ndb)
        assert rc == 0 and 0 <= chunk < nchunk and 0 <= db < ndb, (i, chunk, db)
        seen.add((chunk, db))
    assert len(seen) == nchunk * ndb


@pytest.mark.parametrize("ndb", NDB)
@pytest.mark.parametrize("nchunk", NCHUNK)
def test_workgroups_of_a_chunk_share_an_xcd(nchunk, ndb):
    ids = {}
    for i in range(nchunk * ndb):
        _, chunk, db = slot(i, nchunk, ndb)
        ids.setdefault(chunk, []).append((i, db))
    whole = nchunk // 8 * 8
    first_of_group = {}
    for chunk in range(nchunk):
        lst = ids[chunk]
        assert [db for _, db in lst] == list(range(ndb)), chunk                        # group after group, draw block after draw block
        if chunk < whole:
            assert all(i < whole * ndb and i % 8 == chunk % 8 for i, _ in lst), chunk   # one L2 for the chunk, whatever the draw block
        else:
            assert all(i >= whole * ndb for i, _ in lst), chunk
        for g in range((ndb + GROUP - 1) // GROUP):
            part = [i for i, db in lst if db // GROUP == g]
            step = 8 if chunk < whole else 1
            assert part == list(range(part[0], part[0] + step * len(part), step)), (chunk, g)
            first_of_group.setdefault((chunk < whole, g), []).append(part[0])
    for (_, g), firsts in first_of_group.items():                                        # a group is through before the next one starts
        nxt = first_of_group.get((_, g + 1))
        assert nxt is None or max(firsts) < min(nxt), g


def test_slot_large_counts():
    """a launch at the limits: 65535 draw blocks, 2^31 / 5 chunks — the product is past 32 bits"""
    nchunk, ndb = (2**31 - 1) // 5 + 1, 65535
    assert slot(0, nchunk, ndb) == (0, 0, 0)
    assert slot(8, nchunk, ndb) == (0, 0, 1) and slot(1, nchunk, ndb) == (0, 1, 0)
    assert slot(nchunk * ndb - 1, nchunk, ndb) == (0, nchunk - 1, ndb - 1)
    i = 8 * (GROUP * (nchunk // 8) * 1000 + GROUP * 1 + 1) + 3      # residue 3, group 1000, its second chunk (8 + 3), its second draw block
    assert i > 2**32 and slot(i, nchunk, ndb) == (0, 11, GROUP * 1000 + 1)


def test_slot_refuses_bad_arguments():
    L = pj._lib.lib()
    for i, nchunk, ndb in ((-1, 2, 2), (4, 2, 2), (0, 0, 2), (0, 2, 0), (0, 2**62, 4)):
        assert slot(i, nchunk, ndb)[0] == -1, (i, nchunk, ndb)
    assert L.pioran_tile_pairs_slot(0, 1, 1, None, None) == -1
