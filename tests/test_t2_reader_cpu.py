"""CPU: the Tier-2 reader (grk_amd_read_header / grk_amd_read_packets, grok_amd/csrc/t2_reader.cpp) against the independent
Python reader tests/j2kparse.py, against the library's own writers, against itself where neither covers (layers, precincts,
several tiles: the pixel proof of those is tests/test_gpu_decode_image.py), its refusals, and hostile input."""
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import grok_amd as G
import cshelp
import j2kparse
import oracle as O
import refharness as R
import synth
from grok_amd.capi import CODED_DTYPE, ERR_INVALID, ERR_UNSUPPORTED

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
needs_ref = pytest.mark.skipif(not R.have_ref(), reason="oracle/_ref (the real reference) not built here")
REF_VARS = ("REF_PROG_ORDER", "REF_PRECINCTS", "REF_CSTY", "REF_WRITE_PLT", "REF_WRITE_TLM", "REF_LAYERS", "REF_IMG_X0", "REF_IMG_Y0")


def ref_stream(monkeypatch, px, prec, env=None, **kw):
    for k in REF_VARS:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, str(v))
    kw.setdefault("mode", 1)                          # (grk_compress of the whole image, as the command-line tool does)
    return R.encode(px, prec, **kw)[0]


def block_bytes(cs, out, i):
    """the bytes of row i: straight out of the codestream, or out of the appendix as the moves fill it"""
    r = out["rows"][i]
    o, n = int(r["offset"]), int(r["length"])
    if o < len(cs):
        return bytes(cs[o:o + n])
    if "appendix" not in out:
        app = bytearray(out["appendix_bytes"])
        for m in out["moves"]:
            app[int(m["dst"]):int(m["dst"]) + int(m["len"])] = cs[int(m["src"]):int(m["src"]) + int(m["len"])]
        out["appendix"] = bytes(app)
    return out["appendix"][o - len(cs):o - len(cs) + n]


def check_against_j2kparse(cs):
    ref = j2kparse.parse(cs)
    info = G.read_header(cs)
    out = G.read_packets(cs, info)
    b = info.base
    lay = info.layout
    assert (lay.x1 - lay.x0, lay.y1 - lay.y0, lay.x0, lay.y0, b.num_comps, b.prec) == (ref["W"], ref["H"], ref["x0"], ref["y0"], ref["C"], ref["prec"])
    assert (b.num_levels, b.cblk_w_exp, b.cblk_h_exp, b.mct, b.irreversible) == (ref["levels"], ref["cbw"], ref["cbh"], ref["mct"], ref["irreversible"])
    assert (int(not b.reserved[0]), b.reserved[1]) == (ref["ht"], 0 if ref["ht"] else ref["cblk_sty"] & 0x3F)
    assert info.guard_bits == ref["guard"] and info.num_tiles == 1 and info.num_layers == 1
    words = list(info.qcd_words)[:info.num_qcd]
    assert [(w >> 11, w & 0x7FF) if info.qstyle else (w >> 3, 0) for w in words] == ref["qcd"][:info.num_qcd]
    for r, (ppx, ppy) in enumerate(ref["prc"]):
        assert (b.precinct_exp[r] or 0xFF) == ppx | ppy << 4
    assert bool(info.flags & G.CS_SOP) == bool(ref["scod"] & 2) and bool(info.flags & G.CS_EPH) == bool(ref["scod"] & 4)
    blocks, _ = G.tile_layout(G.layout_tiles(lay, b)[0])
    rows, coded = j2kparse.decode_table(ref, blocks, bool(b.reserved[0]))
    segs = j2kparse.segment_list(ref, blocks)
    assert len(out["rows"]) == len(rows) == info.num_blocks
    assert len(out["moves"]) == 0 and out["appendix_bytes"] == 0
    for i, (off, n, extra) in enumerate(rows):
        assert block_bytes(cs, out, i) == coded[off:off + n], i
        assert int(out["rows"][i]["missing_msbs"]) == extra, i
        f0, f1 = out["first_segment"][i], out["first_segment"][i + 1]
        assert [(int(s["length"]), int(s["numpasses"])) for s in out["segments"][f0:f1]] == [tuple(s) for s in segs[i]], i
    return info


# ---- 1. against the independent reader ---------------------------------------------------------------------------------------
def test_golden_streams_read_as_j2kparse_reads_them():
    seen = 0
    for f in sorted(os.listdir(GOLDEN)):
        if not f.endswith(".j2k"):
            continue
        cs = open(os.path.join(GOLDEN, f), "rb").read()
        try:
            j2kparse.parse(cs)
        except AssertionError:
            continue                                    # (several tiles: test_golden_four_tiles_against_their_single_blocks)
        check_against_j2kparse(cs)
        seen += 1
    assert seen >= 10


@needs_ref
@pytest.mark.parametrize("ht,irrev,sty", [(1, 0, 0), (0, 0, 0), (0, 1, 0), (0, 0, 0x01), (0, 0, 0x02), (0, 1, 0x04), (0, 0, 0x08), (0, 1, 0x20),
                                          (0, 0, 0x05), (0, 1, 0x3F)])
@pytest.mark.parametrize("offset", [(0, 0), (1, 1)])
def test_fresh_reference_streams_read_as_j2kparse_reads_them(monkeypatch, ht, irrev, sty, offset):
    for prec, Cn, H, W in ((8, 3, 100, 77), (12, 1, 96, 130)):
        px = synth.g2(Cn, H, W, prec)
        cs = ref_stream(monkeypatch, px, prec, {"REF_IMG_X0": offset[0], "REF_IMG_Y0": offset[1]}, TW=W + offset[0], TH=H + offset[1],
                        irrev=irrev, numres=4, ht=ht, cblksty=sty)
        info = check_against_j2kparse(cs)
        assert (info.layout.x0, info.layout.y0) == offset


CBLK_SIZES = [(6, 2), (2, 6), (6, 3), (3, 5), (5, 5), (4, 4), (6, 4), (4, 6), (2, 2), (3, 3)]      # exponents (w, h) of the nominal size


@needs_ref
@pytest.mark.parametrize("ht,sty", [(1, 0), (0, 0), (0, 0x05)])
@pytest.mark.parametrize("cblk", CBLK_SIZES, ids=lambda c: "%dx%d" % (1 << c[0], 1 << c[1]))
def test_fresh_reference_streams_of_small_code_blocks_read_as_j2kparse_reads_them(monkeypatch, cblk, ht, sty):
    """`grk_compress -b w,h`: nominal code-block sizes from 64 x 4 to 4 x 4 -- many blocks per band, tag trees several levels deep,
    precinct-clipped sizes at the low resolutions"""
    for prec, Cn, H, W in ((8, 3, 100, 77), (12, 3, 130, 200)):
        cs = ref_stream(monkeypatch, synth.g2(Cn, H, W, prec), prec, numres=4, ht=ht, cblksty=sty, cblk=(1 << cblk[0], 1 << cblk[1]))
        info = check_against_j2kparse(cs)
        assert (info.base.cblk_w_exp, info.base.cblk_h_exp) == cblk
        blocks, _ = G.tile_layout(G.layout_tiles(info.layout, info.base)[0])
        # (the largest band is (W + 1) // 2 x (H + 1) // 2)
        assert max(b.x1 - b.x0 for b in blocks) == min(1 << cblk[0], (W + 1) // 2) and max(b.y1 - b.y0 for b in blocks) == min(1 << cblk[1], (H + 1) // 2)


@needs_ref
@pytest.mark.parametrize("cblk", [(128, 32), (32, 128), (1024, 4)])
def test_code_blocks_wider_or_taller_than_64_are_refused(monkeypatch, cblk):
    cs = ref_stream(monkeypatch, synth.g2(3, 100, 77, 8), 8, numres=4, cblk=cblk)
    assert j2kparse.parse(cs)["cbw"] == cblk[0].bit_length() - 1 and j2kparse.parse(cs)["cbh"] == cblk[1].bit_length() - 1
    with pytest.raises(G.ReaderError) as e:
        G.read_header(cs)
    assert e.value.code == ERR_UNSUPPORTED and "at most 2^6" in e.value.reason


@pytest.mark.parametrize("cblk", [(1, 6), (7, 6), (6, 7), (6, 1)])
def test_tile_layout_refuses_code_block_exponents_outside_2_to_6(cblk):
    p = G.TileParams.make(100, 77, 3, 8, 3, cblk=cblk)
    assert G.lib().grk_amd_tile_num_blocks(p) == ERR_UNSUPPORTED
    with pytest.raises(ValueError, match=str(ERR_UNSUPPORTED)):
        G.tile_layout(p)


# ---- 2. against the writers ------------------------------------------------------------------------------------------------------
def oracle_tables(px, prec, L, layout, precincts=None):
    Cn = px.shape[0]
    base = G.TileParams.make(1, 1, Cn, prec, L, precincts=precincts)
    tabs, chunks, off = [], [], 0
    for p in G.layout_tiles(layout, base):
        ox, oy = p.tile_x0 - layout.x0, p.tile_y0 - layout.y0
        tile = np.ascontiguousarray(px[:, oy:oy + p.tile_h, ox:ox + p.tile_w])
        _, lens, coded = O.encode_tile_rev(tile, prec, L, origin=(p.tile_x0, p.tile_y0), precincts=precincts)
        t = np.zeros(len(lens), CODED_DTYPE)
        t["length"] = lens
        t["offset"] = off + np.concatenate([[0], np.cumsum(lens)[:-1]]) if len(lens) else 0
        t["missing_msbs"] = 0
        off += int(lens.sum())
        tabs.append(t)
        chunks.append(coded)
    return base, np.concatenate(tabs), np.concatenate(chunks)


def check_against_table(cs, layout, base, table, coded, flags, threads=1):
    info = G.read_header(cs)
    for k in ("x0", "y0", "x1", "y1", "tx0", "ty0", "t_width", "t_height"):
        assert getattr(info.layout, k) == getattr(layout, k), k
    for k in ("num_comps", "prec", "sgnd", "irreversible", "mct", "num_levels", "cblk_w_exp", "cblk_h_exp"):
        assert getattr(info.base, k) == getattr(base, k), k
    assert [info.base.precinct_exp[r] or 0xFF for r in range(base.num_levels + 1)] == [base.precinct_exp[r] or 0xFF for r in range(base.num_levels + 1)]
    assert info.flags == flags and info.num_layers == 1 and info.base.reserved[0] == 0
    out = G.read_packets(cs, info, threads)
    assert len(out["rows"]) == len(table) == info.num_blocks and len(out["moves"]) == 0 and out["appendix_bytes"] == 0
    assert np.array_equal(out["rows"]["length"], table["length"])
    # the writer signals Kmax - 1 zero bit-planes for every block (T1HT.cpp:123): the band's, from the layout
    want_msbs = np.concatenate([[b.kmax - 1 for b in G.tile_layout(p)[0]] for p in G.layout_tiles(layout, base)])
    assert np.array_equal(out["rows"]["missing_msbs"], want_msbs)
    cb = np.frombuffer(cs, np.uint8)
    for i in range(len(table)):
        o, n, t = int(out["rows"][i]["offset"]), int(table[i]["length"]), int(table[i]["offset"])
        assert o + n <= len(cs) and np.array_equal(cb[o:o + n], coded[t:t + n]), i
    assert np.array_equal(out["first_segment"], np.arange(len(table) + 1)) and np.array_equal(out["segments"]["length"], table["length"])
    return out


FLAG_SETS = [0, G.CS_SOP, G.CS_EPH, G.CS_PLT, G.CS_TLM, G.CS_SOP | G.CS_EPH | G.CS_PLT | G.CS_TLM]


@pytest.mark.parametrize("W,H,TW,TH,L,off", [(256, 256, 128, 128, 3, (0, 0)), (256, 200, 100, 77, 3, (0, 0)), (300, 200, 128, 96, 4, (5, 3)),
                                             (2000, 2000, 1000, 1000, 5, (1, 1))])
def test_oracle_streams_of_many_tilings_read_back_as_their_tables(W, H, TW, TH, L, off):
    px = synth.g2(1 if W > 1000 else 3, H, W, 8)
    layout = G.ImageLayout.make(W, H, TW, TH, offset=off)
    base, table, coded = oracle_tables(px, 8, L, layout)
    for flags in (FLAG_SETS if W <= 1000 else [0, G.CS_PLT | G.CS_TLM]):
        for order in ((0, 1, 2, 3, 4) if flags in (0, FLAG_SETS[-1]) and W <= 1000 else (0,)):
            fl = flags | G.CS_PROG(order)
            cs = G.write_codestream_layout(layout, base, table, coded, fl)
            a = check_against_table(cs, layout, base, table, coded, fl, 1)
            b = G.read_packets(cs, None, 16)
            assert all(np.array_equal(a[k], b[k]) for k in ("rows", "first_segment", "segments", "moves"))


@pytest.mark.parametrize("precincts", [[(7, 7), (7, 7), (6, 6), (5, 5)], [(5, 6), (6, 5), (7, 8), (8, 7)], [(4, 4)] * 4])
def test_oracle_streams_with_precincts_in_the_five_orders(precincts):
    px = synth.g2(3, 200, 256, 8)
    layout = G.ImageLayout.make(256, 200, 100, 77, offset=(1, 1))
    base, table, coded = oracle_tables(px, 8, 3, layout, precincts)
    for order in range(5):
        for flags in (0, G.CS_PLT | G.CS_SOP | G.CS_EPH):
            fl = flags | G.CS_PROG(order)
            cs = G.write_codestream_layout(layout, base, table, coded, fl)
            check_against_table(cs, layout, base, table, coded, fl, 1 + order)


def test_write_codestream_ex_and_cshelp_streams():
    px = synth.g2(3, 256, 384, 8)
    for flags in (0, G.CS_PLT | G.CS_TLM):
        cs = cshelp.oracle_codestream(px, 8, 3, 128, 128, flags)
        info = G.read_header(cs)
        out = G.read_packets(cs, info, 3)
        assert info.num_tiles == 6 and info.flags == flags
        p = G.TileParams.make(128, 128, 3, 8, 3)
        at = 0
        for ty in range(2):
            for tx in range(3):
                tile = np.ascontiguousarray(px[:, ty * 128:(ty + 1) * 128, tx * 128:(tx + 1) * 128])
                _, lens, coded = O.encode_tile_rev(tile, 8, 3)
                offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
                for i, n in enumerate(lens):
                    assert block_bytes(cs, out, at + i) == bytes(coded[offs[i]:offs[i + 1]])
                at += len(lens)
        assert at == info.num_blocks == 6 * G.lib().grk_amd_tile_num_blocks(p)


def test_golden_four_tiles_against_their_single_blocks():
    """tests/golden/g2_3x256x256_t128_r4.j2k is the reference's file of four tiles: every block's bytes == the oracle encoder's for
    that tile (the writer tests pin that file byte for byte; here it is read back)"""
    cs = open(os.path.join(GOLDEN, "g2_3x256x256_t128_r4.j2k"), "rb").read()
    px = synth.g2(3, 256, 256, 8)
    info = G.read_header(cs)
    assert info.num_tiles == 4 and (info.layout.t_width, info.layout.t_height) == (128, 128)
    out = G.read_packets(cs, info, 3)
    at = 0
    for ty in range(2):
        for tx in range(2):
            tile = np.ascontiguousarray(px[:, ty * 128:(ty + 1) * 128, tx * 128:(tx + 1) * 128])
            blocks, lens, coded = O.encode_tile_rev(tile, 8, info.base.num_levels)
            offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
            for i in range(len(lens)):
                assert block_bytes(cs, out, at + i) == bytes(coded[offs[i]:offs[i + 1]]), (ty, tx, i)
            at += len(lens)
    assert at == len(out["rows"])


# ---- 3. self-consistency where neither oracle reaches ------------------------------------------------------------------------------
def tile_parts_and_plt(cs):
    """[(offset of the first packet, end of the tile-part, [PLT lengths] or None)] by tile index, parsed here from Annex A"""
    res = {}
    for off, ln, ti in G.locate_tile_parts(cs)[0]:
        pos, plt, v, have = off + 12, [], 0, False
        while cs[pos:pos + 2] != b"\xff\x93":
            m, l = struct.unpack(">HH", cs[pos:pos + 4])
            if m == 0xFF58:
                have = True
                for x in cs[pos + 5:pos + 2 + l]:
                    v = v << 7 | (x & 0x7F)
                    if not x & 0x80:
                        plt.append(v)
                        v = 0
            pos += 2 + l
        res[ti] = (pos + 2, off + ln, plt if have else None)
    return res


@needs_ref
@pytest.mark.parametrize("ht", [1, 0])
@pytest.mark.parametrize("order", [0, 1, 2, 3, 4])
def test_layered_reference_streams_are_consistent(monkeypatch, ht, order):
    """(The reference's encoder writes no PLT when it makes quality layers, whatever REF_WRITE_PLT says: the layered streams come
    without, and the packet lengths are held against PLT on single-layer streams of the same tiling, precincts, SOP and EPH.)"""
    px = synth.g2(3, 200, 256, 8)
    for plt in (0, 1):
        env = {"REF_PROG_ORDER": order, "REF_WRITE_PLT": 1, "REF_PRECINCTS": "64,64,32,32", "REF_CSTY": 6 if plt else 0}
        if not plt:
            env["REF_LAYERS"] = "20,10,1"
        cs = ref_stream(monkeypatch, px, 8, env, TW=100, TH=77, numres=4, ht=ht, cblksty=0 if ht else 0x05 * plt)
        info = G.read_header(cs)
        assert info.num_layers == (1 if plt else 3) and info.num_tiles == 9 and bool(info.flags & G.CS_PLT) == bool(plt)
        # (the reader refuses a tile-part that is not consumed exactly to Psot and a packet whose length differs from its PLT
        #  entry: a table at all means both held; a stream with one PLT entry changed is refused below)
        out = G.read_packets(cs, info, 1)
        for threads in (3, 16):
            o = G.read_packets(cs, info, threads)
            assert all(np.array_equal(out[k], o[k]) for k in ("rows", "first_segment", "segments", "moves"))
        rows, first, segs, moves = out["rows"], out["first_segment"], out["segments"], out["moves"]
        # the moves tile the appendix exactly once
        order_ = np.argsort(moves["dst"], kind="stable")
        dst, ln = moves["dst"][order_].astype(np.int64), moves["len"][order_].astype(np.int64)
        assert len(moves) == 0 or (dst[0] == 0 and np.array_equal(dst[1:], np.cumsum(ln)[:-1]) and dst[-1] + ln[-1] == out["appendix_bytes"])
        assert np.all(moves["src"].astype(np.int64) + ln[np.argsort(order_)] <= len(cs))
        if not ht and not plt:
            assert len(moves) > 0
        # per block: its pieces == its segments' lengths == its row
        seg_sum = np.add.reduceat(np.concatenate([segs["length"].astype(np.int64), [0]]), first[:-1].astype(np.int64)) * (first[1:] > first[:-1])
        assert np.array_equal(seg_sum, rows["length"].astype(np.int64))
        in_app = rows["offset"].astype(np.int64) >= len(cs)
        assert int(rows["length"][in_app].astype(np.int64).sum()) == out["appendix_bytes"]
        assert np.all(rows["offset"][~in_app].astype(np.int64) + rows["length"][~in_app] <= len(cs))
        # every byte between SOD and the end of a tile-part is a packet's: headers + the blocks' bytes
        parts = tile_parts_and_plt(cs)
        assert len(parts) == 9
        body = sum(end - start for start, end, _ in parts.values())
        assert int(rows["length"].astype(np.int64).sum()) < body
        if plt:
            for start, end, lens in parts.values():
                assert sum(lens) == end - start
            # one PLT entry off by one (another gets the byte, so the sum still holds): refused
            bad = bytearray(cs)
            off0 = G.locate_tile_parts(cs)[0][0][0]
            pos = off0 + 12
            assert bad[pos:pos + 2] == b"\xff\x58"
            i = pos + 5
            while bad[i] & 0x80 or bad[i + 1] & 0x80 or (bad[i] & 0x7F) in (0, 0x7F) or (bad[i + 1] & 0x7F) in (0, 0x7F):
                i += 1
            bad[i] += 1
            bad[i + 1] -= 1
            with pytest.raises(G.ReaderError) as e:
                G.read_packets(bytes(bad), None, 1)
            assert e.value.code == ERR_INVALID and "PLT" in e.value.reason


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------
def small_stream(flags=0):
    return cshelp.oracle_codestream(synth.g2(3, 128, 128, 8), 8, 3, 64, 64, flags)


def insert_before_sot(cs, seg, tile_part=False):
    at = cs.index(b"\xff\x90")
    if tile_part:
        at += 12
        psot, = struct.unpack(">I", cs[at - 6:at - 2])
        cs = cs[:at - 6] + struct.pack(">I", psot + len(seg)) + cs[at - 2:]
    return cs[:at] + seg + cs[at:]


def seg(marker, body):
    return struct.pack(">HH", marker, len(body) + 2) + body


@pytest.mark.parametrize("name,patch", [
    ("COC", lambda cs: insert_before_sot(cs, seg(0xFF53, bytes([0, 0, 3, 4, 4, 0x40, 1])))),
    ("QCC", lambda cs: insert_before_sot(cs, seg(0xFF5D, bytes([0, 0x20] + [0x40] * 10)))),
    ("POC", lambda cs: insert_before_sot(cs, seg(0xFF5F, bytes([0, 0, 0, 1, 4, 3, 0])))),
    ("RGN", lambda cs: insert_before_sot(cs, seg(0xFF5E, bytes([0, 0, 3])))),
    ("PPM", lambda cs: insert_before_sot(cs, seg(0xFF60, bytes([0, 0, 0, 0, 0])))),
    ("PLM", lambda cs: insert_before_sot(cs, seg(0xFF57, bytes([0, 0])))),
    ("PPT", lambda cs: insert_before_sot(cs, seg(0xFF61, bytes([0, 0])), tile_part=True)),
])
def test_marker_segments_outside_the_readers_class_are_refused_by_name(name, patch):
    cs = small_stream()
    G.read_packets(cs)                                  # (reads clean as it is)
    with pytest.raises(G.ReaderError) as e:
        G.read_packets(patch(cs))
    assert e.value.code == ERR_UNSUPPORTED and name in e.value.reason


def test_second_tile_part_sqcd_style_1_and_the_other_refusals():
    cs = small_stream()
    parts, _ = G.locate_tile_parts(cs)
    # a second tile-part of tile 0 behind the first: TPsot 1
    off, ln, _ = parts[0]
    extra = struct.pack(">HHHIBB", 0xFF90, 10, 0, 14, 1, 0) + b"\xff\x93"
    with pytest.raises(G.ReaderError) as e:
        G.read_packets(cs[:off + ln] + extra + cs[off + ln:])
    assert e.value.code == ERR_UNSUPPORTED and "tile-part" in e.value.reason
    # Sqcd style 1
    q = cs.index(b"\xff\x5c")
    with pytest.raises(G.ReaderError) as e:
        G.read_header(cs[:q + 4] + bytes([cs[q + 4] & 0xE0 | 1]) + cs[q + 5:])
    assert e.value.code == ERR_UNSUPPORTED and "style 1" in e.value.reason
    # components of differing precision; five components; 11 levels; a custom MCT
    s = cs.index(b"\xff\x51")
    with pytest.raises(G.ReaderError) as e:
        G.read_header(cs[:s + 4 + 36 + 3] + bytes([11]) + cs[s + 4 + 36 + 4:])
    assert e.value.code == ERR_UNSUPPORTED and "precision" in e.value.reason
    five = cs[:s + 2] + struct.pack(">H", 38 + 15) + cs[s + 4:s + 4 + 34] + struct.pack(">H", 5) + bytes([7, 1, 1] * 5) + cs[s + 4 + 36 + 9:]
    with pytest.raises(G.ReaderError) as e:
        G.read_header(five)
    assert e.value.code == ERR_UNSUPPORTED and "components" in e.value.reason
    c = cs.index(b"\xff\x52")
    with pytest.raises(G.ReaderError) as e:
        G.read_header(cs[:c + 9] + bytes([11]) + cs[c + 10:])
    assert e.value.code == ERR_UNSUPPORTED and "levels" in e.value.reason
    with pytest.raises(G.ReaderError) as e:
        G.read_header(cs[:c + 8] + bytes([2]) + cs[c + 9:])
    assert e.value.code == ERR_UNSUPPORTED and "MCT" in e.value.reason
    # malformed: a truncated file, no SOC
    for bad in (cs[:len(cs) // 2], b"\x00" + cs[1:], b""):
        with pytest.raises(G.ReaderError) as e:
            G.read_packets(bad)
        assert e.value.code == ERR_INVALID
    # sub-sampled components are READ
    sub = cs[:s + 4 + 36 + 4] + bytes([2, 2]) + cs[s + 4 + 36 + 6:]
    info = G.read_header(sub)
    assert list(info.comp_dx)[:3] == [1, 2, 1] and list(info.comp_dy)[:3] == [1, 2, 1]


@needs_ref
def test_ht_blocks_with_more_than_one_pass_are_refused(monkeypatch):
    """the pass count of one block's packet-header entry raised from 1 ('0') to 2 ('10') cannot be patched in place; a Part-1
    stream relabelled HT in COD has blocks of many passes"""
    cs = ref_stream(monkeypatch, synth.g2(1, 64, 64, 8), 8, numres=3, ht=0)
    c = cs.index(b"\xff\x52")
    with pytest.raises(G.ReaderError) as e:
        G.read_packets(cs[:c + 12] + bytes([cs[c + 12] | 0x40]) + cs[c + 13:])
    assert e.value.code == ERR_UNSUPPORTED and "more than one pass" in e.value.reason


# ---- 5. hostile input --------------------------------------------------------------------------------------------------------------
def hostile_driver():
    out = os.path.join(tempfile.mkdtemp(prefix="reader_hostile_"), "reader_hostile")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(HERE, "..", "include"),
                           os.path.join(HERE, "c", "reader_hostile.cpp"), "-o", out, "-ldl"])
    return out


def run_hostile(driver, cs, corruptions, seed):
    with tempfile.NamedTemporaryFile(suffix=".j2k", delete=False) as f:
        f.write(cs)
    try:
        r = subprocess.run([driver, G.lib_path(), f.name, str(corruptions), str(seed)], capture_output=True, text=True, timeout=900)
    finally:
        os.unlink(f.name)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-500:])
    clean, refused, broken = [int(v) for v in r.stdout.split()[1::2]]
    assert broken == 0 and refused > len(cs) // 2 and clean + refused == len(cs) + corruptions
    return clean, refused


def test_hostile_input_ht_stream_every_prefix_and_corruptions():
    cs = cshelp.oracle_codestream(synth.g2(3, 64, 96, 8), 8, 2, 32, 32, G.CS_PLT | G.CS_SOP | G.CS_EPH)
    run_hostile(hostile_driver(), cs, 1500, 1)


@needs_ref
def test_hostile_input_layered_part1_stream_every_prefix_and_corruptions(monkeypatch):
    cs = ref_stream(monkeypatch, synth.g2(3, 48, 64, 8), 8, {"REF_LAYERS": "20,10,1", "REF_PRECINCTS": "32,32,16,16", "REF_PROG_ORDER": 2},
                    TW=40, TH=48, numres=3, ht=0, cblksty=0x05)
    assert G.read_header(cs).num_layers == 3 and len(G.read_packets(cs)["moves"]) > 0
    run_hostile(hostile_driver(), cs, 1500, 2)


# ---- 6. threads ------------------------------------------------------------------------------------------------------------------
def test_threads_give_identical_output():
    px = synth.g2(3, 256, 256, 8)
    for TW, flags in ((256, G.CS_PLT), (256, 0), (64, G.CS_PLT), (64, 0)):
        cs = cshelp.oracle_codestream(px, 8, 4, TW, TW, flags | G.CS_PROG(2))
        outs = [G.read_packets(cs, None, t) for t in (1, 3, 16)]
        for o in outs[1:]:
            assert all(np.array_equal(outs[0][k], o[k]) for k in ("rows", "first_segment", "segments", "moves"))
