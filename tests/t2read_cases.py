"""The codestreams that the device Tier-2 reader's GPU tests hand to the kernels (tests/test_gpu_t2_read_device.py), built on the CPU
from tables of the tests' choosing with the host writer -- fixed seeds, the same bytes wherever they are built.
tests/test_t2_parse_cpu.py puts every one of them through tests/c/t2_parse_units.cpp (the kernels' parse core on the CPU, under
AddressSanitizer) first: the GPU sees only inputs that program has passed.

cases() -> [(name, bytes, code)]: code None where the stream reads (the rows are the host reader's), else the host reader's code."""
import ctypes as C
import glob
import os

import numpy as np

import grok_amd as G
import t2model as M

HERE = os.path.dirname(os.path.abspath(__file__))
EOC = b"\xff\xd9"
CODED_BYTES = 1 << 20


def tile_params(**kw):
    """4 x 4 blocks: grids of 10 x 16 at the top resolution, trees of five levels"""
    return G.TileParams.make(40, 64, 1, 8, 1, cblk=(2, 2), **kw)


def coded(seed=1):
    return np.random.default_rng(seed).integers(0, 256, CODED_BYTES, dtype=np.uint8)


def table_of(lengths, seed, msbs=None):
    rng = np.random.default_rng(seed)
    t = np.zeros(len(lengths), G.capi.CODED_DTYPE)
    t["length"] = lengths
    t["offset"] = rng.integers(0, CODED_BYTES - np.asarray(lengths, np.int64) + 1)
    if msbs is not None:
        t["missing_msbs"] = msbs
    return t


def num_blocks(p):
    return len(G.tile_layout(p)[0]) * 1


def draw_lengths(p, seed, zero_every=0):
    rng = np.random.default_rng(seed)
    n = num_blocks(p)
    ln = rng.integers(1, 200, n)
    ones = (1 << rng.integers(1, 9, n)) - 1
    pick = rng.random(n) < 0.4
    ln[pick] = ones[pick]
    if zero_every:
        ln[::zero_every] = 0
    return ln


def one_tile_file(p, table, flags, data=None):
    part = G.write_tile_part(p, 0, table, coded() if data is None else data, flags)
    return G.write_main_header(p, p.tile_w, p.tile_h, flags, [len(part)]) + part + EOC


def pack_header(bits):
    """raw header bits -> (the bytes B.10.1 makes of them, without the byte behind a last 0xFF; whether the last byte is 0xFF)"""
    out, cur, room = bytearray(), 0, 8
    for b in bits:
        cur = cur << 1 | int(b)
        room -= 1
        if room == 0:
            out.append(cur)
            room = 7 if cur == 0xFF else 8
            cur = 0
    if room != (7 if out and out[-1] == 0xFF else 8):
        out.append(cur << room)
    return bytes(out), bool(out) and out[-1] == 0xFF


def stuffing_lengths(p, want_end):
    """fixed-seed draws until a packet's header has 0xFF inside it (want_end False) or ENDS on 0xFF -> (lengths, that packet's header)"""
    packets = M.packets_of(p)
    for seed in range(4000):
        ln = draw_lengths(p, 7000 + seed)
        for k in packets:
            data, ends = pack_header(M.raw_bits(k["bands"], ln[k["rows"]]))
            if (ends if want_end else (0xFF in data[:-1] and not ends)):
                return ln, data + (b"\x00" if ends else b"")
    raise AssertionError("no draw with the stuffing wanted")


def three_tiles(tlm, order=(2, 0, 1)):
    """three tiles in one row, their tile-parts in the file in `order`"""
    p = tile_params()
    flags = G.CS_PLT | (G.CS_TLM if tlm else 0)
    parts = [G.write_tile_part(p, t, table_of(draw_lengths(p, 40 + t), 50 + t), coded(), flags) for t in range(3)]
    hdr = bytearray(G.write_main_header(p, 120, 64, flags, [len(x) for x in parts]))
    if tlm:
        # the writer's TLM lists the tiles in index order: its entries again, in file order
        at = hdr.index(b"\xff\x55")
        ltlm, stlm = int.from_bytes(hdr[at + 2:at + 4], "big"), hdr[at + 5]
        st, sp = (stlm >> 4) & 3, (stlm >> 6) & 1
        rec = st + (4 if sp else 2)
        assert st in (1, 2) and ltlm == 4 + 3 * rec
        for i, t in enumerate(order):
            q = at + 6 + i * rec
            hdr[q:q + rec] = t.to_bytes(st, "big") + len(parts[t]).to_bytes(4 if sp else 2, "big")
    return bytes(hdr) + b"".join(parts[t] for t in order) + EOC


def subsampled_file(flags=0):
    """4:2:0, two tiles"""
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
    rng = np.random.default_rng(77)
    table = table_of(rng.integers(0, 120, n), 78)
    data = coded()
    out = np.empty(1 << 20, np.uint8)
    got = L.grk_amd_write_codestream_subsampled(C.addressof(layout), C.addressof(base), C.addressof(dxs), C.addressof(dys), table.ctypes.data,
                                                data.ctypes.data, flags, out.ctypes.data, out.size)
    assert got > 0, got
    return out[:got].tobytes()


def long_header_file(com_bytes=6000):
    """a COM segment spliced in front of the first SOT: the main header is longer than the device call's first copy"""
    p = tile_params()
    cs = one_tile_file(p, table_of(draw_lengths(p, 90), 91), G.CS_PLT)
    sot = cs.index(b"\xff\x90")
    com = b"\xff\x64" + (com_bytes + 4).to_bytes(2, "big") + b"\x00\x01" + bytes(com_bytes)
    return cs[:sot] + com + cs[sot:]


def grid_file(w, h):
    """a band grid of 65 x 1 or 1 x 65 blocks: tag trees of eight levels"""
    p = G.TileParams.make(w, h, 1, 8, 0, cblk=(2, 2))
    return one_tile_file(p, table_of(draw_lengths(p, w), w + 1), G.CS_PLT | G.CS_EPH)


def good_file():
    p = tile_params()
    return one_tile_file(p, table_of(draw_lengths(p, 5), 6), G.CS_PLT | G.CS_SOP | G.CS_EPH | G.CS_TLM)


def reading_cases():
    out = []
    p = tile_params()
    for f in range(16):
        out.append(("flags-%02d" % f, one_tile_file(p, table_of(draw_lengths(p, 100 + f), 200 + f), f), None))
    for order in range(5):
        q = tile_params(precincts=[(3, 3), (4, 3)]) if order >= 2 else p
        out.append(("order-%d" % order, one_tile_file(q, table_of(draw_lengths(q, 300 + order), 310 + order), G.CS_PLT | G.CS_SOP | G.CS_PROG(order)), None))
    q = tile_params(precincts=[(3, 3), (4, 4)])
    out.append(("precinct-grid", one_tile_file(q, table_of(draw_lengths(q, 320), 321), G.CS_EPH), None))
    out.append(("precinct-grid-plt", one_tile_file(q, table_of(draw_lengths(q, 322), 323), G.CS_PLT), None))
    blocks = G.tile_layout(p)[0]
    rng = np.random.default_rng(330)
    msbs = np.array([rng.integers(0, max(1, b.kmax)) for b in blocks])
    out.append(("block-msbs", one_tile_file(p, table_of(draw_lengths(p, 331), 332, msbs), G.CS_BLOCK_MSBS | G.CS_PLT), None))
    out.append(("block-msbs-chain", one_tile_file(p, table_of(draw_lengths(p, 333), 334, msbs), G.CS_BLOCK_MSBS | G.CS_SOP), None))
    out.append(("zero-lengths", one_tile_file(p, table_of(draw_lengths(p, 340, zero_every=2), 341), G.CS_PLT), None))
    out.append(("all-zero-lengths", one_tile_file(p, table_of(np.zeros(num_blocks(p), np.int64), 342), 0), None))
    ln = draw_lengths(p, 350)
    ln[len(ln) // 2] = (1 << 20) - 1
    out.append(("one-long-block", one_tile_file(p, table_of(ln, 351), G.CS_PLT), None))
    for want_end in (False, True):
        ln, header = stuffing_lengths(p, want_end)
        cs = one_tile_file(p, table_of(ln, 360), G.CS_SOP | G.CS_EPH | G.CS_PLT)
        # (on the CPU, before any launch: the file has the header that was drawn, between an SOP segment and EPH)
        assert cs.count(header + b"\xff\x92") >= 1 and (header[-2] == 0xFF if want_end else 0xFF in header[:-1])
        out.append(("header-ends-on-ff" if want_end else "ff-inside-header", cs, None))
    out.append(("three-tiles-out-of-order", three_tiles(False), None))
    out.append(("three-tiles-out-of-order-tlm", three_tiles(True), None))
    out.append(("420-two-tiles", subsampled_file(0), None))
    out.append(("420-two-tiles-plt", subsampled_file(G.CS_PLT | G.CS_SOP), None))
    out.append(("long-main-header", long_header_file(), None))
    out.append(("grid-65x1", grid_file(260, 4), None))
    out.append(("grid-1x65", grid_file(4, 260), None))
    return out


def _plt_span(cs):
    at = cs.index(b"\xff\x58")
    return at + 5, at + 2 + int.from_bytes(cs[at + 2:at + 4], "big")


def corruption_cases():
    """the twelve named corruptions of good_file() (PLT | TLM | SOP | EPH, one tile) and of the three-tile file"""
    INVALID = G.ERR_INVALID
    g = good_file()
    # (len - 1 of a file whose one tile-part runs to EOC, Psot = 0: the tile-part loses its last byte)
    p0 = tile_params()
    open_end = bytearray(one_tile_file(p0, table_of(draw_lengths(p0, 5), 6), G.CS_PLT | G.CS_SOP | G.CS_EPH))
    s0 = open_end.index(b"\xff\x90")
    open_end[s0 + 6:s0 + 10] = bytes(4)
    out = [("cut-last-byte", bytes(open_end[:-1]), INVALID)]
    sop = [i for i in range(len(g) - 5) if g[i:i + 4] == b"\xff\x91\x00\x04"]
    out.append(("cut-inside-packet-header", g[:sop[-1] + 7], INVALID))
    lo, hi = _plt_span(g)
    # the first PLT entry whose last byte can go up and down by one
    k = next(i for i in range(lo, hi) if 1 <= g[i] <= 0x7E)
    out.append(("plt-entry-plus-1", g[:k] + bytes([g[k] + 1]) + g[k + 1:], INVALID))
    out.append(("plt-entry-minus-1", g[:k] + bytes([g[k] - 1]) + g[k + 1:], INVALID))
    # one entry too few: the last entry goes, Lplt, Psot and TLM's length shrink by its bytes
    first = hi - 1
    while first > lo and g[first - 1] >= 0x80:
        first -= 1
    cut = hi - first
    at = lo - 5
    short = bytearray(g[:first] + g[hi:])
    short[at + 2:at + 4] = (int.from_bytes(g[at + 2:at + 4], "big") - cut).to_bytes(2, "big")
    sot = g.index(b"\xff\x90")
    psot = int.from_bytes(g[sot + 6:sot + 10], "big")
    short[sot + 6:sot + 10] = (psot - cut).to_bytes(4, "big")
    tlm = g.index(b"\xff\x55")
    q = bytes(short).index(psot.to_bytes(4, "big"), tlm, sot)
    short[q:q + 4] = (psot - cut).to_bytes(4, "big")
    out.append(("plt-one-entry-too-few", bytes(short), INVALID))
    s = sop[1]
    out.append(("wrong-sop-number", g[:s + 5] + bytes([g[s + 5] ^ 1]) + g[s + 6:], INVALID))
    e = g.index(b"\xff\x92", sop[0])
    out.append(("missing-eph", g[:e] + b"\x00\x00" + g[e + 2:], INVALID))
    # a packet header that is ones to the end of the tile-part: the Lblock run never ends; zeros: the zero-bit-plane tree never does
    p = tile_params()
    plain = one_tile_file(p, table_of(draw_lengths(p, 5), 6), 0)
    sod = plain.index(b"\xff\x93") + 2
    body = len(plain) - 2 - sod
    # (the first packet's band is 5 x 8 blocks, trees of four levels: present, four ones include the first block, four more make its
    #  zero bit-planes 0, a zero says one pass -- then Lblock's ones; or, behind the inclusion, zeros)
    ones = (b"\xff\x5f" + b"\xff\x7f" * body)[:body]
    out.append(("lblock-ones-to-the-end", plain[:sod] + ones + EOC, INVALID))
    out.append(("zero-planes-zeros-to-the-end", plain[:sod] + b"\xf8" + bytes(body - 1) + EOC, INVALID))
    t3 = three_tiles(False)
    sots = [i for i in range(len(t3) - 11) if t3[i:i + 4] == b"\xff\x90\x00\x0a"]
    out.append(("psot-beyond-len", t3[:sots[2] + 6] + (len(t3)).to_bytes(4, "big") + t3[sots[2] + 10:], INVALID))
    out.append(("isot-beyond-grid", t3[:sots[1] + 4] + b"\x00\x07" + t3[sots[1] + 6:], INVALID))
    out.append(("same-isot-twice", t3[:sots[1] + 4] + t3[sots[0] + 4:sots[0] + 6] + t3[sots[1] + 6:], G.ERR_UNSUPPORTED))
    assert len(out) == 12
    return out


def golden_cases():
    out = []
    for f in sorted(glob.glob(os.path.join(HERE, "golden", "*.j2k"))):
        name = os.path.basename(f)
        unsupported = "_sty05_" in name or "_sty3f_" in name
        out.append((name, open(f, "rb").read(), G.ERR_UNSUPPORTED if unsupported else None))
    return out
