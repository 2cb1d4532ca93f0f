"""The tile-part-divided codestreams of tests/test_tile_parts_cpu.py and tests/test_gpu_tile_parts.py: files built on the CPU with the
host writer from tables of the tests' choosing (fixed seeds, as tests/t2read_cases.py: the same bytes wherever they are built), then
cut by the model tests/tileparts.py.

cases()    -> [(name, undivided file, Cut)]: the cut file must read as the undivided one does, offsets mapped
refusals() -> [(name, bytes, code, words the reason must hold)]"""
import numpy as np

import grok_amd as G
import t2layers_cases as LC
import t2layers_model as LM
import tileparts as TP
from t2read_cases import EOC, coded, draw_lengths, one_tile_file, subsampled_file, table_of, tile_params

PLT, SOP, EPH = G.CS_PLT, G.CS_SOP, G.CS_EPH


def many_packets_params():
    """4 components x (40 + 40) precincts: 320 packets"""
    return G.TileParams.make(40, 64, 4, 8, 1, mct=False, cblk=(2, 2), precincts=[(2, 2), (3, 3)])


def many_packets_file(flags, seed=500):
    p = many_packets_params()
    return one_tile_file(p, table_of(draw_lengths(p, seed), seed + 1), flags)


def three_tiles_file(flags):
    """three tiles of 320 packets in one row"""
    p = many_packets_params()
    parts = [G.write_tile_part(p, t, table_of(draw_lengths(p, 600 + t), 610 + t), coded(), flags) for t in range(3)]
    return G.write_main_header(p, 120, 64, flags, [len(x) for x in parts]) + b"".join(parts) + EOC


def layered_file(order, flags):
    """three layers, LAZY, every block in pieces: moves and an appendix"""
    p = LC.tile(1)
    return LM.build(p, 40, 64, 3, order, flags, 1, LM.draw_table(p, 3, 1, 700 + order), seed=710 + order)[0]


def four_tiles_layered_file(order, flags, sty=1):
    """2 x 2 tiles of 40 x 64, three layers: the layered model's tile-parts behind one main header"""
    p = LC.tile(sty)
    built = [LM.build(p, 80, 128, 3, order, flags, sty, LM.draw_table(p, 3, sty, 720 + t), seed=730 + t)[0] for t in range(4)]
    sot = built[0].index(b"\xff\x90\x00\x0a")
    parts = [b[sot:sot + 4] + t.to_bytes(2, "big") + b[sot + 6:-2] for t, b in enumerate(built)]
    return built[0][:sot] + b"".join(parts) + EOC


def cases():
    out = []

    def add(name, cs, **kw):
        out.append((name, cs, TP.cut(cs, **kw)))

    # every progression order, SOP / EPH on and off: thirds
    q = tile_params(precincts=[(3, 3), (4, 3)])
    for order in range(5):
        for n, flags in enumerate((PLT, PLT | SOP | EPH, SOP, SOP | EPH)):
            cs = one_tile_file(q, table_of(draw_lengths(q, 800 + order), 810 + order), flags | G.CS_PROG(order))
            add("order-%d-f%x" % (order, flags), cs, boundaries=TP.thirds, plt="keep" if flags & PLT else "drop", tnsot=("all", "last", "none")[(order + n) % 3])
    # one tile in two parts at every packet boundary in turn (the first and the last: a part without packets)
    cs = one_tile_file(q, table_of(draw_lengths(q, 820), 821), PLT | G.CS_PROG(2))
    npk = len(TP.scan(cs)["tiles"][0].lens)
    assert npk == 36
    for k in range(npk + 1):
        add("two-parts-at-%02d" % k, cs, boundaries={0: [k]}, plt="drop" if k % 2 else "keep", empty_plt=k == npk)
    # one packet per part up to the 255th part
    big = many_packets_file(PLT)
    assert len(TP.scan(big)["tiles"][0].lens) == 320
    add("255-parts", big, boundaries=TP.every_packet)
    add("255-parts-no-plt-tlm", many_packets_file(SOP), boundaries=TP.every_packet, plt="drop", tlm="write", tnsot="none")
    # a part whose PLT holds more than 256 entries
    add("plt-of-300-entries", big, boundaries={0: [300]})
    # three tiles out of order with 100 parts each: more than 256 tile-parts
    t3 = three_tiles_file(PLT)
    hundred = lambda tile, n: list(range(1 + tile, 100 + tile))
    for tlm in (None, "write"):
        for order in ("tile", "interleave"):
            add("three-tiles-300-parts-%s%s" % (order, "-tlm" if tlm else ""), t3, boundaries=hundred, tile_order=(2, 0, 1), order=order, tlm=tlm,
                tnsot="last" if tlm else "all", last_psot_zero=order == "tile")
    add("three-tiles-tlm-8-bit-index-16-bit-length", t3, boundaries=TP.thirds, tile_order=(1, 2, 0), tlm="write", stlm=(1, 0), order="interleave")
    # 4:2:0, two tiles
    for flags in (PLT | SOP, SOP):
        add("420-two-tiles-f%x" % flags, subsampled_file(flags), boundaries=TP.thirds, order="interleave", plt="keep" if flags & PLT else "drop")
    # three layers, LAZY: cut between the layers (LRCP) and inside a precinct's layers (RPCL)
    cs = layered_file(0, PLT | EPH)
    npk = len(TP.scan(cs)["tiles"][0].lens)
    assert npk == 6
    add("layers-lrcp-between-layers", cs, boundaries={0: [npk // 3, 2 * npk // 3]})
    add("layers-lrcp-between-layers-no-plt", layered_file(0, SOP), boundaries={0: [npk // 3, 2 * npk // 3]}, plt="drop")
    cs = layered_file(2, PLT)
    add("layers-rpcl-inside-a-precinct", cs, boundaries={0: [1, 2, 4]})
    add("layers-rpcl-inside-a-precinct-no-plt", layered_file(2, SOP | EPH), boundaries={0: [1, 5]}, plt="drop", tnsot="none")
    add("four-tiles-layers-interleaved-tlm", four_tiles_layered_file(1, PLT), boundaries=TP.thirds, order="interleave", tlm="write")
    # only some parts carry PLT
    cs = one_tile_file(q, table_of(draw_lengths(q, 830), 831), PLT | SOP | G.CS_PROG(3))
    add("plt-in-some-parts", cs, boundaries={0: [5, 11, 11, 30]}, plt=lambda tile, k: k in (0, 3))
    add("plt-in-all-but-an-empty-part", cs, boundaries={0: [5, 5, 30]})
    names = [x[0] for x in out]
    assert len(set(names)) == len(names)
    return out


def _patch(b, at, new):
    return b[:at] + bytes(new) + b[at + len(new):]


def refusals():
    INVALID, UNSUPPORTED = G.ERR_INVALID, G.ERR_UNSUPPORTED
    out = []
    q = tile_params(precincts=[(3, 3), (4, 3)])
    cs = one_tile_file(q, table_of(draw_lengths(q, 900), 901), PLT | SOP)
    c = TP.cut(cs, boundaries={0: [9, 20]})
    p0, p1, p2 = c.parts
    good = c.cs
    # TPsot missing, repeated, out of file order
    out.append(("tpsot-missing", good[:p1.at] + good[p2.at:], INVALID, ["tile 0", "tile-part 2"]))
    out.append(("tpsot-repeated", _patch(good, p2.at + 10, [1]), INVALID, ["tile 0", "tile-part 1"]))
    out.append(("tpsot-out-of-order", good[:p1.at] + good[p2.at:p2.at + p2.length] + good[p1.at:p2.at] + good[p2.at + p2.length:], INVALID, ["tile 0", "tile-part 2"]))
    # TNsot: two values; not above a TPsot seen; more than the parts found
    out.append(("tnsot-two-values", _patch(good, p1.at + 11, [4]), INVALID, ["tile 0", "tile-part 1", "TNsot"]))
    out.append(("tnsot-not-above-tpsot", _patch(_patch(_patch(good, p0.at + 11, [2]), p1.at + 11, [2]), p2.at + 11, [2]), INVALID, ["tile 0", "tile-part 2", "TNsot"]))
    only_first = TP.cut(cs, boundaries={0: [9, 20]}, tnsot="none").cs
    out.append(("tnsot-beyond-the-parts", _patch(only_first, p0.at + 11, [4]), INVALID, ["tile 0", "tile-part 3", "TNsot"]))
    # a boundary that is no packet boundary: 3 bytes of part 1's first packet moved to the end of part 0 (Psot and PLT follow)
    nopl = TP.cut(cs, boundaries={0: [9, 20]}, plt="drop")
    a, b = nopl.parts[0], nopl.parts[1]
    moved = bytearray(nopl.cs[:a.at + a.length] + nopl.cs[b.body_at:b.body_at + 3] + nopl.cs[b.at:b.body_at] + nopl.cs[b.body_at + 3:])
    moved[a.at + 6:a.at + 10] = (a.length + 3).to_bytes(4, "big")
    moved[b.at + 3 + 6:b.at + 3 + 10] = (b.length - 3).to_bytes(4, "big")
    out.append(("packet-across-a-boundary", bytes(moved), INVALID, ["tile 0", "tile-part"]))
    # packets left over / missing at the last part: the last part's last packet cut away, or a packet of the first given twice
    c2 = nopl.parts[2]
    lens = TP.scan(cs)["tiles"][0].lens
    short = bytearray(nopl.cs[:c2.at + c2.length - lens[-1]] + nopl.cs[c2.at + c2.length:])
    short[c2.at + 6:c2.at + 10] = (c2.length - lens[-1]).to_bytes(4, "big")
    out.append(("packets-missing", bytes(short), INVALID, ["tile 0", "tile-part 2"]))
    extra = bytes([0x80]) if not (G.read_header(cs).flags & SOP) else b"\xff\x91\x00\x04" + (36).to_bytes(2, "big") + b"\x00"
    more = bytearray(nopl.cs[:c2.at + c2.length] + extra + nopl.cs[c2.at + c2.length:])
    more[c2.at + 6:c2.at + 10] = (c2.length + len(extra)).to_bytes(4, "big")
    out.append(("packets-left-over", bytes(more), INVALID, ["tile 0", "tile-part 2"]))
    # PLT lengths that do not add up to their part: one entry of part 1 raised by one
    k = next(i for i in range(p1.at + 12 + 5, p1.body_at - 2) if 1 <= good[i] <= 0x7E)
    out.append(("plt-does-not-add-up", _patch(good, k, [good[k] + 1]), INVALID, ["tile 0", "tile-part 1", "PLT"]))
    # (the same with PLT only in that part: the tile is read as one chain and the entry held against the packet)
    some = TP.cut(cs, boundaries={0: [9, 20]}, plt=lambda t, i: i == 1)
    s1 = some.parts[1]
    k = next(i for i in range(s1.at + 12 + 5, s1.body_at - 2) if 1 <= some.cs[i] <= 0x7E)
    out.append(("plt-entry-in-a-chain-tile", _patch(some.cs, k, [some.cs[k] + 1]), INVALID, ["tile 0", "tile-part 1", "PLT"]))
    # a Psot that leaves the stream; Psot 0 before the last part
    out.append(("psot-leaves-the-stream", _patch(good, p2.at + 6, (len(good)).to_bytes(4, "big")), INVALID, ["tile 0", "tile-part 2", "Psot"]))
    out.append(("psot-0-in-the-middle", _patch(good, p1.at + 6, bytes(4)), INVALID, ["tile 0", "tile-part"]))
    # a tile without a part
    t3 = three_tiles_file(PLT)
    c3 = TP.cut(t3, boundaries=TP.thirds)
    gone = [p for p in c3.parts if p.tile == 1]
    out.append(("tile-without-a-part", c3.cs[:gone[0].at] + c3.cs[gone[-1].at + gone[-1].length:], INVALID, ["tile 1"]))
    # COD / QCD / COC / QCC / RGN / POC / PPT in a tile-part header (here: of the second part)
    for name, seg in (("COD", b"\xff\x52\x00\x0c" + bytes(10)), ("QCD", b"\xff\x5c\x00\x04\x40\x40"), ("COC", b"\xff\x53\x00\x09" + bytes(7)),
                      ("QCC", b"\xff\x5d\x00\x05\x00\x40\x40"), ("RGN", b"\xff\x5e\x00\x05\x00\x00\x03"), ("POC", b"\xff\x5f\x00\x09" + bytes(7)),
                      ("PPT", b"\xff\x61\x00\x04\x00\x00")):
        bad = bytearray(good[:p1.at + 12] + seg + good[p1.at + 12:])
        bad[p1.at + 6:p1.at + 10] = (p1.length + len(seg)).to_bytes(4, "big")
        out.append(("%s-in-a-tile-part-header" % name.lower(), bytes(bad), UNSUPPORTED, [name]))
    # a 256th part of one tile
    big = many_packets_file(SOP)
    c = TP.cut(big, boundaries=TP.every_packet, plt="drop", tnsot="none")
    last = c.parts[-1]
    first_len = TP.scan(big)["tiles"][0].lens[254]
    head = bytearray(c.cs[:last.body_at + first_len])
    head[last.at + 6:last.at + 10] = (last.body_at - last.at + first_len).to_bytes(4, "big")
    rest = c.cs[last.body_at + first_len:-2]
    part256 = b"\xff\x90\x00\x0a\x00\x00" + (14 + len(rest)).to_bytes(4, "big") + bytes([255, 0]) + b"\xff\x93" + rest
    out.append(("256th-part", bytes(head) + part256 + EOC, UNSUPPORTED, ["tile 0", "255"]))
    names = [x[0] for x in out]
    assert len(set(names)) == len(names)
    return out
