"""CPU: WRITING tiles divided into tile-parts (GRK_AMD_CS_TP; grok_amd/csrc/t2_writer.cpp, geometry.cpp, t2_parts.h).

The oracle is tests/tileparts.py, the pure-Python model that cuts an undivided file at packet boundaries: grk_amd_write_tile_parts behind
grk_amd_write_main_header_parts, and the whole-file writers under the flag, must give the model's bytes; the readers of
tests/test_tile_parts_cpu.py check the result from the other side, and where oracle/_ref is built the reference's decoder does.

The division rule is held against boundaries this file derives itself: every block's place in the undivided file says which packet
holds it, the block's (component, resolution) is the geometry's, and a tile-part starts where the key of those changes.

tests/c/t2_parts_writer_units.cpp is the divided writer and the t2_parts.h arithmetic as a stand-alone program under AddressSanitizer
and UBSan."""
import bisect
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import grok_amd as G
import refharness as R
import synth
import tileparts as TP
import tileparts_cases as TC
from t2read_cases import EOC, coded, draw_lengths, one_tile_file, subsampled_file, table_of, tile_params

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "grok_amd", "csrc")
SAN = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined"]
HALT = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1")
needs_ref = pytest.mark.skipif(not R.have_ref(), reason="oracle/_ref (the real reference) not built here")
PLT, SOP, EPH, TLM = G.CS_PLT, G.CS_SOP, G.CS_EPH, G.CS_TLM
ORDERS = ["LRCP", "RLCP", "RPCL", "PCRL", "CPRL"]
ERR_OVERFLOW = -5
LETTERS = {G.TP_R: "R", G.TP_L: "L", G.TP_C: "C"}


# ---- what the rule says, restated ----------------------------------------------------------------------------------------------------
def rule(order, letter, levels, comps):
    """the number of tile-parts, or None where a P lies at or before the division letter"""
    n = 1
    for ch in ORDERS[order]:
        if ch == "P":
            return None
        n *= {"L": 1, "R": levels + 1, "C": comps}[ch]
        if ch == LETTERS[letter]:
            return n


def key_of(order, letter, comp, res, levels, comps):
    k = 0
    for ch in ORDERS[order]:
        if ch == "R":
            k = k * (levels + 1) + res
        elif ch == "C":
            k = k * comps + comp
        if ch == LETTERS[letter]:
            return k


def packet_keys(cs, blocks_of_tile, order, letter, levels, comps):
    """per tile of the undivided file `cs`: every packet's key, from the blocks the packet holds (every block here has bytes)"""
    s = TP.scan(cs)
    rows = G.read_packets(cs)["rows"]
    out, row = [], 0
    for T in s["tiles"]:
        blocks = blocks_of_tile(T.index)
        at = np.concatenate([[T.body_at], T.body_at + np.cumsum(T.lens)])
        keys = [None] * len(T.lens)
        for b, r in zip(blocks, rows[row:row + len(blocks)]):
            assert r["length"] > 0
            k = bisect.bisect_right(at, int(r["offset"])) - 1
            key = key_of(order, letter, b[0], b[1], levels, comps)
            assert keys[k] in (None, key), "a packet with blocks of two keys"
            keys[k] = key
        assert None not in keys, "a packet without a block: its key is not known to this test"
        out.append(keys)
        row += len(blocks)
    return out


def starts_from_keys(keys, nparts):
    assert keys == sorted(keys)
    return [bisect.bisect_left(keys, k) for k in range(nparts)]


def plain_blocks(p):
    return [(b.comp, b.res) for b in G.tile_layout(p)[0]]


def check_rule_on(p, flags_extra=0, seed=40):
    tab = table_of(draw_lengths(p, seed), seed + 1)
    for order in range(5):
        cs = one_tile_file(p, tab, PLT | G.CS_PROG(order) | flags_extra)
        for letter in (G.TP_R, G.TP_L, G.TP_C):
            want = rule(order, letter, p.num_levels, p.num_comps)
            flags = G.CS_PROG(order) | G.CS_TP(letter)
            if want is None or want > 255:
                with pytest.raises(G.WriterError) as e:
                    G.tile_part_starts(p, flags)
                assert e.value.code == G.ERR_UNSUPPORTED and e.value.reason, (order, letter)
                continue
            starts, npk = G.tile_part_starts(p, flags)
            keys = packet_keys(cs, lambda t: plain_blocks(p), order, letter, p.num_levels, p.num_comps)[0]
            assert npk == len(keys) and len(starts) == want, (order, letter, starts)
            assert starts == starts_from_keys(keys, want), (order, letter)


def test_the_table_of_part_counts_and_refusals():
    p = tile_params(precincts=[(3, 3), (4, 3)])
    got = {}
    for order in range(5):
        for letter in (G.TP_R, G.TP_L, G.TP_C):
            try:
                got[(ORDERS[order], LETTERS[letter])] = len(G.tile_part_starts(p, G.CS_PROG(order) | G.CS_TP(letter))[0])
            except G.WriterError as e:
                assert e.code == G.ERR_UNSUPPORTED and "P" in e.reason
                got[(ORDERS[order], LETTERS[letter])] = None
    Rn, Cn = p.num_levels + 1, p.num_comps
    assert got == {("LRCP", "R"): Rn, ("LRCP", "L"): 1, ("LRCP", "C"): Rn * Cn, ("RLCP", "R"): Rn, ("RLCP", "L"): Rn, ("RLCP", "C"): Rn * Cn,
                   ("RPCL", "R"): Rn, ("RPCL", "L"): None, ("RPCL", "C"): None, ("PCRL", "R"): None, ("PCRL", "L"): None, ("PCRL", "C"): None,
                   ("CPRL", "R"): None, ("CPRL", "L"): None, ("CPRL", "C"): Cn}
    # no division: one part from packet 0, whatever the order
    assert G.tile_part_starts(p, G.CS_PROG(3)) == ([0], 36)


def test_starts_equal_boundaries_derived_from_the_packets_blocks():
    check_rule_on(tile_params(precincts=[(3, 3), (4, 3)]))
    check_rule_on(TC.many_packets_params(), seed=44)


def test_starts_of_a_420_tile():
    L = G.lib()
    layout = G.ImageLayout.make(70, 38, 40, 38)
    base = G.TileParams.make(40, 38, 3, 8, 2, mct=False, cblk=(3, 3))
    sampling = [(1, 1), (2, 2), (2, 2)]

    def blocks_of(t):
        out = []
        for c, (dx, dy) in enumerate(sampling):
            q = G.TileParams()
            assert L.grk_amd_layout_tile_comp(C.byref(layout), C.byref(base), dx, dy, t, C.byref(q)) == 0
            q.num_comps, q.mct = 1, 0
            out += [(c, b.res) for b in G.tile_layout(q)[0]]
        return out

    # (subsampled_file draws lengths from 0: the rule is held on the packets that have a block with bytes, which fixes every boundary
    #  the keys below need -- a packet of unknown key lies between two known ones of one part or is asserted away)
    tiles = G.layout_tiles(layout, base)
    for order, letter in ((0, G.TP_R), (0, G.TP_C), (1, G.TP_L), (2, G.TP_R), (4, G.TP_C)):
        cs = subsampled_file(PLT | G.CS_PROG(order))
        s = TP.scan(cs)
        rows = G.read_packets(cs)["rows"]
        row = 0
        for T in s["tiles"]:
            blocks = blocks_of(T.index)
            at = np.concatenate([[T.body_at], T.body_at + np.cumsum(T.lens)])
            known = {}
            for b, r in zip(blocks, rows[row:row + len(blocks)]):
                if r["length"]:
                    known[bisect.bisect_right(at, int(r["offset"])) - 1] = key_of(order, letter, b[0], b[1], 2, 3)
            row += len(blocks)
            starts, npk = G.tile_part_starts(tiles[T.index], G.CS_PROG(order) | G.CS_TP(letter), sampling)
            assert npk == len(T.lens) and len(starts) == rule(order, letter, 2, 3) and starts[0] == 0 and starts == sorted(starts)
            assert len(known) > npk // 2
            for k, key in known.items():
                assert bisect.bisect_right(starts, k) - 1 == key, (order, letter, T.index, k)


def offgrid_tile():
    """3 x 2 samples at (5, 3), two levels: resolution 0 is empty (ceil(8 / 4) - ceil(5 / 4) = 0 columns)"""
    return G.TileParams.make(3, 2, 1, 8, 2, cblk=(2, 2), origin=(5, 3))


def test_an_empty_resolution_is_a_part_of_14_bytes():
    p = offgrid_tile()
    n = len(G.tile_layout(p)[0])
    tab = table_of(np.full(n, 7), 3)
    starts, npk = G.tile_part_starts(p, G.CS_TP(G.TP_R))
    assert len(starts) == 3 and starts[0] == starts[1] == 0 and npk == starts[2] + (npk - starts[2])
    body, lens = G.write_tile_parts(p, 0, tab, coded(), PLT | G.CS_TP(G.TP_R))
    assert lens[0] == 14 and sum(lens) == len(body)
    assert body[:14] == b"\xff\x90\x00\x0a\x00\x00" + (14).to_bytes(4, "big") + bytes([0, 3]) + b"\xff\x93"


def test_more_than_255_parts_is_refused():
    # a 4-component tile with enough levels under LRCP + C: 4 x 64 parts
    with pytest.raises(G.WriterError) as e:
        G.tile_part_starts(G.TileParams.make(64, 64, 4, 8, 63, mct=False, cblk=(2, 2)), G.CS_TP(G.TP_C))
    assert e.value.code == G.ERR_UNSUPPORTED and "255" in e.value.reason
    p = G.TileParams.make(64, 64, 4, 8, 5, mct=False, cblk=(2, 2))
    assert len(G.tile_part_starts(p, G.CS_TP(G.TP_C))[0]) == 24
    # (the library codes at most 10 levels and 4 components -- 44 parts: the rule answers before the geometry is looked at, and a
    #  tile the library can code never meets the limit)
    assert len(G.tile_part_starts(G.TileParams.make(2048, 2048, 4, 8, 10, mct=False), G.CS_PROG(1) | G.CS_TP(G.TP_C))[0]) == 44


def test_more_parts_than_one_tlm_segment_lists_is_refused():
    """255 tiles of 52 parts: 13 260 > 13 106 (the files this library writes stay below: 255 tiles of at most 44 parts)"""
    lay = G.ImageLayout.make(16 * 255, 16, 16, 16)
    q = G.TileParams.make(16, 16, 4, 8, 3, mct=False, cblk=(2, 2))
    with pytest.raises(G.WriterError) as e:
        G.write_main_header_parts(lay, q, TLM, [52] * 255, np.full(13260, 14))
    assert e.value.code == G.ERR_UNSUPPORTED and "13 106" in e.value.reason
    hdr = G.write_main_header_parts(lay, q, TLM, [51] * 254 + [152], np.full(13106, 14))
    at = hdr.index(b"\xff\x55")
    assert int.from_bytes(hdr[at + 2:at + 4], "big") == 4 + 5 * 13106 == 65534 and len(hdr) == at + 2 + 65534
    assert len(G.write_main_header_parts(lay, q, 0, [52] * 255, np.full(13260, 14))) < 300          # without TLM: nothing to list
    with pytest.raises(G.WriterError) as e:
        G.write_main_header_parts(lay, q, TLM, [256] + [1] * 254, np.full(510, 14))
    assert e.value.code == G.ERR_INVALID


# ---- host writer == model --------------------------------------------------------------------------------------------------------------
def divided_file(layout, base, tiles, tables, data, flags, starts_of):
    """the file of grk_amd_write_tile_parts per tile behind grk_amd_write_main_header_parts"""
    bodies, lens, per = [], [], []
    for t, (p, tab) in enumerate(zip(tiles, tables)):
        body, ln = G.write_tile_parts(p, t, tab, data, flags, starts=starts_of(t))
        size, ln2 = G.write_tile_parts(p, t, tab, None, flags, starts=starts_of(t), size_only=True)
        assert size == len(body) == sum(ln) and list(ln2[:len(ln)]) == ln
        bodies.append(body); lens += ln; per.append(len(ln))
    return G.write_main_header_parts(layout, base, flags, per, lens) + b"".join(bodies) + EOC


def model(base_cs, boundaries, flags):
    return TP.cut(base_cs, boundaries, plt="keep" if flags & PLT else "drop", tnsot="all", order="tile", tlm="write" if flags & TLM else None, stlm=(1, 1))


def expected(base, cut):
    """the undivided file's table with its positions mapped into the cut file (tests/test_tile_parts_cpu.py)"""
    want = G.read_packets(base)
    rows = want["rows"].copy()
    inside = (rows["length"] > 0) & (rows["offset"] < len(base))
    rows["offset"][inside] = cut.map(rows["offset"][inside])
    behind = (rows["length"] > 0) & ~inside
    rows["offset"][behind] = rows["offset"][behind] - len(base) + len(cut.cs)
    moves = want["moves"].copy()
    if len(moves):
        moves["src"] = cut.map(moves["src"])
    return dict(rows=rows, first_segment=want["first_segment"], segments=want["segments"], moves=moves, appendix_bytes=want["appendix_bytes"])


def reads_back(base, cut, cs):
    want, got = expected(base, cut), G.read_packets_parts(cs, None, 2)
    assert np.array_equal(got["rows"], want["rows"]) and np.array_equal(got["segments"], want["segments"])
    assert np.array_equal(got["first_segment"], want["first_segment"]) and got["appendix_bytes"] == want["appendix_bytes"]


def one_tile_against_model(p, tab, flags, boundaries, data=None):
    data = coded() if data is None else data
    base = one_tile_file(p, tab, flags, data)
    npk = len(TP.scan(base)["tiles"][0].lens)
    b = boundaries(0, npk) if callable(boundaries) else boundaries
    cut = model(base, {0: b}, flags)
    lay = G.ImageLayout.make(p.tile_w, p.tile_h, p.tile_w, p.tile_h)
    got = divided_file(lay, p, [p], [tab], data, flags, lambda t: [0] + list(b))
    assert got == cut.cs, (flags, b)
    return base, cut


Q = tile_params(precincts=[(3, 3), (4, 3)])


@pytest.mark.parametrize("flags", [PLT, PLT | SOP | EPH, SOP, SOP | EPH, PLT | TLM, SOP | TLM | EPH])
def test_thirds_and_empty_middle_equal_the_model(flags):
    for order in (0, 2, 4):
        tab = table_of(draw_lengths(Q, 800 + order), 810 + order)
        for b in (TP.thirds, TP.empty_middle):
            base, cut = one_tile_against_model(Q, tab, flags | G.CS_PROG(order), b)
            reads_back(base, cut, cut.cs)


def test_two_parts_at_every_packet_boundary():
    tab = table_of(draw_lengths(Q, 820), 821)
    for k in range(37):
        base, cut = one_tile_against_model(Q, tab, (PLT if k % 2 == 0 else SOP) | G.CS_PROG(2), [k])
        assert [p.packets for p in cut.parts] == [(0, k), (k, 36 - k)]
        if k in (0, 17, 36):
            reads_back(base, cut, cut.cs)


def test_one_packet_per_part_up_to_the_255th():
    p = TC.many_packets_params()
    for flags in (PLT, SOP | TLM):
        base, cut = one_tile_against_model(p, table_of(draw_lengths(p, 500), 501), flags, TP.every_packet)
        assert len(cut.parts) == 255 and cut.parts[-1].packets == (254, 66)
        reads_back(base, cut, cut.cs)


@pytest.mark.parametrize("tlm", [0, TLM])
def test_three_tiles_of_100_parts_each(tlm):
    p = TC.many_packets_params()
    flags = PLT | tlm
    base = TC.three_tiles_file(flags)
    hundred = lambda tile, n: list(range(1 + tile, 100 + tile))
    cut = model(base, hundred, flags)
    assert len(cut.parts) == 300
    lay = G.ImageLayout.make(120, 64, 40, 64)
    tiles = G.layout_tiles(lay, p)
    tables = [table_of(draw_lengths(p, 600 + t), 610 + t) for t in range(3)]
    got = divided_file(lay, p, tiles, tables, coded(), flags, lambda t: [0] + hundred(t, 320))
    assert got == cut.cs
    reads_back(base, cut, got)


def test_a_block_msbs_table():
    blocks = G.tile_layout(Q)[0]
    rng = np.random.default_rng(330)
    msbs = np.array([rng.integers(0, max(1, b.kmax)) for b in blocks])
    tab = table_of(draw_lengths(Q, 331), 332, msbs)
    base, cut = one_tile_against_model(Q, tab, G.CS_BLOCK_MSBS | PLT | G.CS_PROG(1), TP.thirds)
    reads_back(base, cut, cut.cs)


# ---- named divisions through the whole-file writers -------------------------------------------------------------------------------------
def boundaries_from_flags(tiles, flags, sampling=None):
    out = {}
    for t, p in enumerate(tiles):
        starts, _ = G.tile_part_starts(p, flags, sampling)
        out[t] = starts[1:]
    return out


@pytest.mark.parametrize("order,letter", [(0, G.TP_R), (0, G.TP_C), (1, G.TP_R), (1, G.TP_L), (1, G.TP_C), (2, G.TP_R), (4, G.TP_C)])
def test_write_codestream_layout_under_the_flag_equals_the_model(order, letter):
    lay = G.ImageLayout.make(75, 120, 40, 64)                     # 2 x 2 tiles, the right column and the bottom row ragged
    base = G.TileParams.make(40, 64, 3, 8, 2, mct=False, cblk=(2, 2), precincts=[(2, 2), (3, 3), (4, 3)])
    tiles = G.layout_tiles(lay, base)
    n = sum(len(G.tile_layout(p)[0]) for p in tiles)
    rows = table_of(np.random.default_rng(9).integers(1, 150, n), 10)
    for extra in (PLT | TLM, SOP | EPH):
        flags = extra | G.CS_PROG(order)
        undivided = G.write_codestream_layout(lay, base, rows, coded(), flags)
        got = G.write_codestream_layout(lay, base, rows, coded(), flags | G.CS_TP(letter))
        cut = model(undivided, boundaries_from_flags(tiles, flags | G.CS_TP(letter)), flags)
        assert got == cut.cs, (order, letter, extra)
        assert len(cut.parts) == 4 * rule(order, letter, 2, 3)
        reads_back(undivided, cut, got)
    # ... and through grk_amd_write_codestream_ex, whose tiles share one geometry
    p1 = G.TileParams.make(64, 64, 3, 8, 2, mct=False, cblk=(2, 2))
    rows = table_of(np.random.default_rng(11).integers(1, 150, 4 * len(G.tile_layout(p1)[0])), 12)
    flags = PLT | TLM | G.CS_PROG(order)
    lay1 = G.ImageLayout.make(128, 128, 64, 64)
    a = G.write_codestream(p1, 128, 128, rows, coded(), flags | G.CS_TP(letter))
    assert a == model(G.write_codestream(p1, 128, 128, rows, coded(), flags), boundaries_from_flags(G.layout_tiles(lay1, p1), flags | G.CS_TP(letter)), flags).cs


def _subsampled(flags, cap=None):
    """tests/t2read_cases.subsampled_file with its return code"""
    L = G.lib()
    L.grk_amd_write_codestream_subsampled.restype = C.c_int64
    L.grk_amd_write_codestream_subsampled.argtypes = [C.c_void_p] * 6 + [C.c_uint32, C.c_void_p, C.c_uint64]
    layout = G.ImageLayout.make(70, 38, 40, 38)
    base = G.TileParams.make(40, 38, 3, 8, 2, mct=False, cblk=(3, 3))
    dxs, dys = (C.c_uint8 * 3)(1, 2, 2), (C.c_uint8 * 3)(1, 2, 2)
    n = 0
    for t in range(2):
        for c in range(3):
            q = G.TileParams()
            assert L.grk_amd_layout_tile_comp(C.byref(layout), C.byref(base), int(dxs[c]), int(dys[c]), t, C.byref(q)) == 0
            q.num_comps, q.mct = 1, 0
            n += len(G.tile_layout(q)[0])
    table = table_of(np.random.default_rng(77).integers(0, 120, n), 78)
    data = coded()
    out = np.full((1 << 20) + 64, 0xA5, np.uint8)
    cap = (1 << 20) if cap is None else cap
    got = L.grk_amd_write_codestream_subsampled(C.addressof(layout), C.addressof(base), C.addressof(dxs), C.addressof(dys), table.ctypes.data,
                                                data.ctypes.data, flags, out.ctypes.data, cap)
    assert (out[cap:] == 0xA5).all()
    return got, out[:max(got, 0)].tobytes(), G.layout_tiles(layout, base)


@pytest.mark.parametrize("order,letter", [(0, G.TP_R), (0, G.TP_C), (1, G.TP_L), (2, G.TP_R), (4, G.TP_C)])
def test_write_codestream_subsampled_under_the_flag_equals_the_model(order, letter):
    sampling = [(1, 1), (2, 2), (2, 2)]
    for extra in (PLT | TLM | SOP, SOP):
        flags = extra | G.CS_PROG(order)
        n0, undivided, tiles = _subsampled(flags)
        assert undivided == subsampled_file(flags)
        n, got, _ = _subsampled(flags | G.CS_TP(letter))
        assert n > n0
        cut = model(undivided, boundaries_from_flags(tiles, flags | G.CS_TP(letter), sampling), flags)
        assert got == cut.cs, (order, letter, extra)
        reads_back(undivided, cut, got)
        # one byte short: refused, and nothing written beyond cap
        assert _subsampled(flags | G.CS_TP(letter), cap=n - 1)[0] == ERR_OVERFLOW


def test_lrcp_divided_at_l_is_the_undivided_file_byte_for_byte():
    tab = table_of(draw_lengths(Q, 1), 2)
    for extra in (0, PLT | TLM, SOP | EPH | TLM):
        flags = extra | G.CS_PROG(0)
        assert G.write_codestream(Q, 40, 64, tab, coded(), flags | G.CS_TP(G.TP_L)) == G.write_codestream(Q, 40, 64, tab, coded(), flags)
        body, lens = G.write_tile_parts(Q, 0, tab, coded(), flags | G.CS_TP(G.TP_L))
        assert body == G.write_tile_part(Q, 0, tab, coded(), flags) and lens == [len(body)]
    # ... and no division at all through the divided call
    assert G.write_tile_parts(Q, 5, tab, coded(), PLT | G.CS_PROG(3))[0] == G.write_tile_part(Q, 5, tab, coded(), PLT | G.CS_PROG(3))


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_explicit_starts_that_are_refused():
    tab = table_of(draw_lengths(Q, 1), 2)
    for bad in ([0, 20, 10], [0, 37], [1, 5], [0] * 256, [0, 36, 37]):
        with pytest.raises(G.WriterError) as e:
            G.write_tile_parts(Q, 0, tab, coded(), PLT, starts=bad)
        assert e.value.code == G.ERR_INVALID, bad
    assert len(G.write_tile_parts(Q, 0, tab, coded(), PLT, starts=[0] * 255)[1]) == 255
    assert G.write_tile_parts(Q, 0, tab, coded(), PLT, starts=[0, 36, 36])[1][1:] == [14, 14]


def test_cap_one_byte_short_overflows_and_writes_nothing_beyond_it():
    tab = table_of(draw_lengths(Q, 1), 2)
    for flags, starts in ((PLT, [0, 12, 24]), (SOP | EPH | G.CS_TP(G.TP_R), None)):
        body, _ = G.write_tile_parts(Q, 0, tab, coded(), flags, starts=starts)
        assert G.write_tile_parts(Q, 0, tab, coded(), flags, starts=starts, cap=len(body))[0] == body
        with pytest.raises(G.WriterError) as e:                     # (the wrapper holds a guard behind cap)
            G.write_tile_parts(Q, 0, tab, coded(), flags, starts=starts, cap=len(body) - 1)
        assert e.value.code == ERR_OVERFLOW


def test_plan_tile_part_refuses_the_flag():
    L = G.lib()
    L.grk_amd_plan_tile_part.restype = C.c_int64
    L.grk_amd_plan_tile_part.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
    tab = table_of(draw_lengths(Q, 1), 2)
    nlit, nseg = C.c_uint64(0), C.c_uint64(0)
    for letter in (G.TP_R, G.TP_L, G.TP_C):
        assert L.grk_amd_plan_tile_part(C.addressof(Q), 0, PLT | G.CS_TP(letter), tab.ctypes.data, None, 0, C.byref(nlit), None, 0, C.byref(nseg)) == G.ERR_UNSUPPORTED
    assert L.grk_amd_plan_tile_part(C.addressof(Q), 0, PLT, tab.ctypes.data, None, 0, C.byref(nlit), None, 0, C.byref(nseg)) > 0


def test_unsupported_pairs_through_the_file_writers():
    tab = table_of(draw_lengths(Q, 1), 2)
    for order, letter in ((2, G.TP_L), (2, G.TP_C), (3, G.TP_R), (3, G.TP_L), (3, G.TP_C), (4, G.TP_R), (4, G.TP_L)):
        with pytest.raises(G.WriterError) as e:
            G.write_codestream_layout(G.ImageLayout.make(40, 64, 40, 64), Q, tab, coded(), G.CS_PROG(order) | G.CS_TP(letter))
        assert e.value.code == G.ERR_UNSUPPORTED and "P" in e.value.reason
        with pytest.raises(G.WriterError) as e:
            G.write_tile_parts(Q, 0, tab, coded(), G.CS_PROG(order) | G.CS_TP(letter))
        assert e.value.code == G.ERR_UNSUPPORTED
        assert _subsampled(G.CS_PROG(order) | G.CS_TP(letter))[0] == G.ERR_UNSUPPORTED


# ---- the reference's decoder ------------------------------------------------------------------------------------------------------------
@needs_ref
@pytest.mark.parametrize("order,letter,sizes", [(0, G.TP_R, None), (2, G.TP_R, [(32, 32)]), (4, G.TP_C, None)])
def test_the_reference_decodes_a_divided_file_to_the_undivided_files_pixels(order, letter, sizes):
    """3 x 80 x 96 in four tiles of 64 x 64, three resolutions, the oracle's blocks; PLT and TLM"""
    from test_precincts_cpu import exps_from_sizes, oracle_codestream_prc
    px = synth.g2_mid(3, 80, 96, 8)
    layout = G.ImageLayout.make(96, 80, 64, 64)
    prc = exps_from_sizes(sizes, 2) if sizes else None
    flags = PLT | TLM | G.CS_PROG(order)
    plain = oracle_codestream_prc(px, 8, 2, layout, prc, flags)
    cut = oracle_codestream_prc(px, 8, 2, layout, prc, flags | G.CS_TP(letter))
    found, used = G.locate_tile_parts(cut)
    assert used and len(found) == 4 * rule(order, letter, 2, 3) > 4
    if sizes:
        assert len(TP.scan(plain)["tiles"][0].lens) > 9                  # more than one precinct per resolution
    want = R.decode(plain, 3, 80, 96)
    assert np.array_equal(np.asarray(want), px.astype(np.int32))
    assert np.array_equal(np.asarray(R.decode(cut, 3, 80, 96)), np.asarray(want))


# ---- under the sanitizers ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("t2_parts_writer") / "t2_parts_writer_units")
    subprocess.check_call(["g++"] + SAN + ["-Wall", "-D_GLIBCXX_ASSERTIONS", os.path.join(HERE, "c", "t2_parts_writer_units.cpp")] +
                          [os.path.join(CSRC, f) for f in ("t2_writer.cpp", "geometry.cpp", "host_common.cpp")] + ["-o", path, "-lpthread"])
    return path


def test_the_divided_writer_and_the_frame_arithmetic_under_the_sanitizers(exe):
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=HALT)
    assert r.returncode == 0 and "runtime error" not in r.stdout and "AddressSanitizer" not in r.stdout, r.stdout[-4000:]
    assert "ok:" in r.stdout.strip().split("\n")[-1], r.stdout[-2000:]
