"""CPU: the compact coded buffer of a view of a file whose tiles are divided into tile-parts (decode_image_plan.cpp: plan_coded,
rebase_table), through the driver of tests/test_decode_image_plan_cpu.py.  A touched tile contributes the list of its tile-parts,
tile-parts that follow each other in the file are one copy, and every row and move is rebased through the tile-part it lies in."""
import numpy as np
import pytest

import grok_amd as G
import test_decode_image_plan_cpu as DP
import tileparts as TP
import tileparts_cases as TC
from grok_amd.capi import ERR_INVALID

TOUCHED = [0, 1]                    # of four tiles of 64 x 48 in an image of 120 x 90
WINDOW = (1, 1, 119, 47)


def plain_stream():
    """four tiles of 64 x 48 in an image of 120 x 90, with PLT (the model finds the packets through it)"""
    layout = G.ImageLayout.make(120, 90, 64, 48)
    base = G.TileParams.make(64, 48, 3, 8, 3)
    n = sum(G.lib().grk_amd_tile_num_blocks(p) for p in G.layout_tiles(layout, base))
    return G.write_codestream_layout(layout, base, *DP.random_table(n, 11), G.CS_PLT)


def coded_plan(nparts, ntouched):
    L = DP.lib()
    out, parts = np.zeros(4, np.uint64), np.zeros((nparts, 2), np.uint64)
    assert L.dip_coded(DP.ptr(out), DP.ptr(parts)) == 0, L.dip_reason()
    every, up_len, coded_cap, ncopies = (int(v) for v in out)
    part_to, copies = np.zeros(max(1, ntouched), np.uint64), np.zeros((ncopies, 3), np.uint64)
    L.dip_coded_lists(DP.ptr(part_to), DP.ptr(copies))
    return every, up_len, coded_cap, [[int(v) for v in c] for c in copies], parts.astype(np.int64), part_to.astype(np.int64)


@pytest.mark.parametrize("order,ncopies", [("interleave", 6), ("tile", 1)])
def test_a_view_of_two_of_four_tiles_in_tile_parts(order, ncopies):
    base = plain_stream()
    cut = TP.cut(base, boundaries=TP.thirds, order=order, tlm="write" if order == "interleave" else None)
    cs = cut.cs
    csb = np.frombuffer(cs, np.uint8)
    assert len(cut.parts) == 12
    d = DP.plan(cs, window=WINDOW)
    assert d["nunits"] == 2 and not d["all"]
    every, up_len, coded_cap, copies, parts, part_to = coded_plan(len(cut.parts), len(TOUCHED))
    # the located tile-parts: every tile's first, then the others as the file has them
    firsts = [cut.parts_of(t)[0] for t in range(4)]
    later = [p for p in cut.parts if p.tpsot]
    assert [(int(a), int(n)) for a, n in parts] == [(p.at, p.length) for p in firsts + later]
    mine = [p for t in TOUCHED for p in cut.parts_of(t)]
    assert not every and up_len == sum(p.length for p in mine) and coded_cap == up_len
    assert [int(v) for v in part_to[:2]] == [0, sum(p.length for p in cut.parts_of(0))]
    # the copies: the touched tile-parts tile after tile, those that follow each other in the file as one
    want, to = [], 0
    for p in mine:
        if want and want[-1][1] + want[-1][2] == p.at:
            want[-1][2] += p.length
        else:
            want.append([to, p.at, p.length])
        to += p.length
    assert copies == want and len(copies) == ncopies
    # no byte of another tile's tile-part is copied
    others = [p for p in cut.parts if p.tile not in TOUCHED]
    for _, frm, n in copies:
        assert all(frm + n <= p.at or p.at + p.length <= frm for p in others)
    compact = np.zeros(up_len, np.uint8)
    for to, frm, n in copies:
        compact[to:to + n] = csb[frm:frm + n]
    t = DP.rebase()
    assert isinstance(t, dict), t
    seen = 0
    for old, new in zip(t["old_rows"], t["rows"]):
        n = int(new["length"])
        assert n == int(old["length"]) and new["missing_msbs"] == old["missing_msbs"]
        if n:
            assert np.array_equal(compact[int(new["offset"]):int(new["offset"]) + n], csb[int(old["offset"]):int(old["offset"]) + n])
            seen += 1
    assert seen > 20
    # the rows are the undivided file's for those tiles, through the model's map
    whole = G.read_packets(base)
    per_tile = len(whole["rows"]) // 4
    for i, tile in enumerate(TOUCHED):
        a = whole["rows"][tile * per_tile:(tile + 1) * per_tile]
        b = t["old_rows"][i * per_tile:(i + 1) * per_tile]
        assert np.array_equal(a["length"], b["length"])
        keep = a["length"] > 0
        assert np.array_equal(cut.map(a["offset"][keep]), b["offset"][keep].astype(np.int64))
    # a row or a move outside its tile's tile-parts -- in another tile's, between two of its own -- is refused
    assert DP.rebase(1) == (ERR_INVALID, "a block outside its tile-part")
    assert isinstance(DP.rebase(0), dict)


def test_a_layered_view_rebases_its_moves_through_the_tile_parts():
    """three layers, LAZY, 2 x 2 tiles of 40 x 64: the blocks come in pieces, so the reader gives moves and an appendix"""
    base = TC.four_tiles_layered_file(1, G.CS_PLT)
    cut = TP.cut(base, boundaries=TP.thirds, order="interleave", tlm="write")
    cs = cut.cs
    csb = np.frombuffer(cs, np.uint8)
    d = DP.plan(cs, window=(1, 1, 79, 63))
    assert d["nunits"] == 2 and not d["all"]
    every, up_len, coded_cap, copies, parts, part_to = coded_plan(len(cut.parts), 2)
    assert up_len == sum(p.length for t in TOUCHED for p in cut.parts_of(t)) and coded_cap == 2 * up_len and len(copies) == 6
    compact = np.zeros(up_len, np.uint8)
    for to, frm, n in copies:
        compact[to:to + n] = csb[frm:frm + n]
    t = DP.rebase()
    assert isinstance(t, dict) and len(t["moves"]) > 50 and t["appendix_bytes"] > 0
    for old, new in zip(t["old_moves"], t["moves"]):
        n = int(new["len"])
        assert (int(new["dst"]), n) == (int(old["dst"]), int(old["len"]))
        assert np.array_equal(compact[int(new["src"]):int(new["src"]) + n], csb[int(old["src"]):int(old["src"]) + n])
    for old, new in zip(t["old_rows"], t["rows"]):
        if int(new["length"]) and int(old["offset"]) >= len(cs):
            assert int(new["offset"]) == int(old["offset"]) - len(cs) + up_len
    assert DP.rebase(2) == (ERR_INVALID, "a block outside its tile-part")
    assert DP.rebase(1) == (ERR_INVALID, "a block outside its tile-part")
