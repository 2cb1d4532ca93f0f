"""The model of tile-part division (T.800 A.4.2, B.12; what `grk_compress -u R|L|C` does to a file): a codestream with one tile-part
per tile is cut into tile-parts at packet boundaries of the caller's choice.  Pure Python, no library call -- the readers under test
never see their own work here, and a writer of tile-parts has this as its model.

A tile's packet sequence is the concatenation of its tile-parts' bodies, so nothing inside a packet changes: the expected table of a
cut file is the undivided file's with every offset sent through Cut.map.

    scan(cs)                -> the file taken apart: main header, per tile its header's marker segments, body and packet lengths
    cut(cs, boundaries, ..) -> Cut(cs=the new file, parts=[Part in file order], map(old positions) -> new positions)

Packet lengths come from PLT where the file has it, else from SOP marker segments (tests/t2layers_cases.plt_from_sop shows the scan);
a file with neither cannot be cut here."""
import bisect
from collections import namedtuple

import numpy as np

SOT, SOD, PLT, TLM, SOP, EOC = 0xFF90, 0xFF93, 0xFF58, 0xFF55, b"\xff\x91\x00\x04", b"\xff\xd9"
Tile = namedtuple("Tile", "index markers body_at body_end lens")          # markers: the tile-part header's segments other than PLT
Part = namedtuple("Part", "tile tpsot at length body_at body_end packets has_plt")     # positions in the cut file; packets: (first, count)


def u16(b, i):
    return int.from_bytes(b[i:i + 2], "big")


def u32(b, i):
    return int.from_bytes(b[i:i + 4], "big")


def scan(cs):
    cs = bytes(cs)
    assert cs[:2] == b"\xff\x4f"
    at, header = 2, []                                   # the main header's marker segments, TLM left out
    while u16(cs, at) != SOT:
        n = 2 + u16(cs, at + 2)
        if u16(cs, at) != TLM:
            header.append(cs[at:at + n])
        at += n
    tiles = []
    while cs[at:at + 2] == b"\xff\x90":
        assert u16(cs, at + 2) == 10 and cs[at + 10] == 0 and cs[at + 11] in (0, 1), "one tile-part per tile is what is cut"
        psot = u32(cs, at + 6)
        end = at + psot if psot else len(cs) - 2
        pos, markers, lens, have_plt, v = at + 12, b"", [], False, 0
        while u16(cs, pos) != SOD:
            n = 2 + u16(cs, pos + 2)
            if u16(cs, pos) == PLT:
                have_plt = True
                for x in cs[pos + 5:pos + n]:
                    v = v << 7 | (x & 0x7F)
                    if not x & 0x80:
                        lens.append(v)
                        v = 0
            else:
                markers += cs[pos:pos + n]
            pos += n
        body = pos + 2
        if not have_plt:
            starts, i = [], cs.find(SOP, body, end)
            assert i == body or body == end, "neither PLT nor SOP: the packets' lengths are not known"
            while i >= 0:
                starts.append(i)
                i = cs.find(SOP, i + 6, end)
            lens = [b - a for a, b in zip(starts, starts[1:] + [end])]
        assert sum(lens) == end - body, "the packet lengths do not add up to the tile-part"
        tiles.append(Tile(u16(cs, at + 4), markers, body, end, lens))
        at = end
    assert cs[at:] == EOC
    assert sorted(t.index for t in tiles) == list(range(len(tiles)))
    return dict(cs=cs, header=b"\xff\x4f" + b"".join(header), tiles=sorted(tiles, key=lambda t: t.index), file_order=[t.index for t in tiles])


def plt_segments(lens):
    """PLT marker segments of these packet lengths: Zplt from 0, no entry runs on into the next segment"""
    out, z, cur = b"", 0, b""
    for n in list(lens) + [None]:
        e = None
        if n is not None:
            e = [n & 0x7F]
            n >>= 7
            while n:
                e.insert(0, 0x80 | (n & 0x7F))
                n >>= 7
            e = bytes(e)
        if e is None or len(cur) + len(e) > 60000:
            out += b"\xff\x58" + (3 + len(cur)).to_bytes(2, "big") + bytes([z]) + cur
            z, cur = z + 1, b""
        if e is not None:
            cur += e
    return out


def tlm_segment(entries, st=2, sp=1):
    """one TLM marker segment: entries [(tile, length)] in file order; st: bytes of the tile index (0: none), sp: 32-bit lengths"""
    body = b"".join((t.to_bytes(st, "big") if st else b"") + n.to_bytes(4 if sp else 2, "big") for t, n in entries)
    assert len(body) + 4 <= 0xFFFF
    return b"\xff\x55" + (4 + len(body)).to_bytes(2, "big") + bytes([0, st << 4 | sp << 6]) + body


class Cut:
    def __init__(self, cs, parts, spans):
        self.cs, self.parts = cs, parts
        self._old = [s[0] for s in spans]
        self._spans = spans                             # (old start, old end, new start), rising old start

    def map(self, positions):
        """old positions of bytes inside packets -> where those bytes lie in the cut file"""
        out = []
        for p in np.asarray(positions, np.int64).ravel():
            k = bisect.bisect_right(self._old, int(p)) - 1
            a, b, to = self._spans[k]
            assert k >= 0 and a <= p < b, "not a position inside a packet"
            out.append(int(p) - a + to)
        return np.array(out, np.int64).reshape(np.shape(positions))

    def parts_of(self, tile):
        return [p for p in self.parts if p.tile == tile]


def cut(cs, boundaries, plt="keep", tnsot="all", order="tile", tile_order=None, tlm=None, stlm=(2, 1), last_psot_zero=False, empty_plt=False):
    """boundaries: {tile: [packet numbers at which a new tile-part starts]} or a function of (tile, number of packets); numbers may
         repeat or be 0 or the packet count: tile-parts that hold no packet.  A tile left out stays one tile-part.
    plt: "keep" every tile-part that holds packets lists them | "drop" | a function (tile, tpsot) -> bool: some do
    tnsot: "all" TNsot in every tile-part | "last" in the tile's last only | "none" 0 everywhere
    order: "tile" a tile's parts together | "interleave" every tile's first part, then every tile's second, ... | [(tile, tpsot)]
    tile_order: the tiles' order in the file (default: as in `cs`)
    tlm: None no TLM | "write" one entry per tile-part in file order, of the form stlm = (ST, SP)
    last_psot_zero: Psot = 0 in the file's last tile-part;  empty_plt: a tile-part without packets carries a PLT of no entry"""
    s = scan(cs)
    src = s["cs"]
    tile_order = list(tile_order) if tile_order is not None else s["file_order"]
    pieces = {}                                          # (tile, tpsot) -> (first packet, count)
    for T in s["tiles"]:
        b = boundaries(T.index, len(T.lens)) if callable(boundaries) else boundaries.get(T.index, [])
        b = [0] + list(b) + [len(T.lens)]
        assert b == sorted(b) and len(b) - 1 <= 255
        for k in range(len(b) - 1):
            pieces[(T.index, k)] = (b[k], b[k + 1] - b[k])
    nparts = {t: 1 + max(k for (tt, k) in pieces if tt == t) for t in tile_order}
    if order == "tile":
        seq = [(t, k) for t in tile_order for k in range(nparts[t])]
    elif order == "interleave":
        seq = [(t, k) for k in range(max(nparts.values())) for t in tile_order if k < nparts[t]]
    else:
        seq = list(order)
        assert sorted(seq) == sorted(pieces)
    blobs, meta = [], []
    for n, (t, k) in enumerate(seq):
        T = s["tiles"][t]
        first, count = pieces[(t, k)]
        lens = T.lens[first:first + count]
        with_plt = plt == "keep" or (callable(plt) and plt(t, k))
        hdr = T.markers if k == 0 else b""
        if with_plt and (count or empty_plt):
            hdr += plt_segments(lens)
        a = T.body_at + sum(T.lens[:first])
        body = src[a:a + sum(lens)]
        total = 12 + len(hdr) + 2 + len(body)
        tn = nparts[t] if tnsot == "all" or (tnsot == "last" and k == nparts[t] - 1) else 0
        psot = 0 if last_psot_zero and n == len(seq) - 1 else total
        blobs.append(b"\xff\x90\x00\x0a" + t.to_bytes(2, "big") + psot.to_bytes(4, "big") + bytes([k, tn]) + hdr + b"\xff\x93" + body)
        meta.append((t, k, total, 12 + len(hdr) + 2, a, first, count, with_plt and bool(count or empty_plt)))
    header = s["header"]
    if tlm == "write":
        header += tlm_segment([(m[0], m[2]) for m in meta], *stlm)
    else:
        assert tlm is None
    at, parts, spans = len(header), [], []
    for t, k, total, hlen, a, first, count, has in meta:
        parts.append(Part(t, k, at, total, at + hlen, at + total, (first, count), has))
        if total > hlen:
            spans.append((a, a + total - hlen, at + hlen))
        at += total
    return Cut(header + b"".join(blobs) + EOC, parts, sorted(spans))


# ---- the cuts the tests share ------------------------------------------------------------------------------------------------
def thirds(tile, n):
    return [n // 3, 2 * n // 3]


def every_packet(tile, n):
    return list(range(1, min(n, 255)))


def empty_middle(tile, n):
    return [n // 2, n // 2]


NINE_CUTS = [
    ("thirds", dict(boundaries=thirds)),
    ("no-plt", dict(boundaries=thirds, plt="drop")),
    ("tnsot-last", dict(boundaries=thirds, tnsot="last")),
    ("tnsot-none", dict(boundaries=thirds, tnsot="none")),
    ("interleaved", dict(boundaries=thirds, order="interleave")),
    ("tlm", dict(boundaries=thirds, tlm="write")),
    ("tlm-interleaved", dict(boundaries=thirds, tlm="write", order="interleave")),
    ("empty-middle", dict(boundaries=empty_middle)),
    ("packet-per-part", dict(boundaries=every_packet)),
]
