"""A writer of LAYERED one-tile codestreams from tables of the tests' choosing, restated in Python from ITU-T T.800 B.10 for the tests
of the general device Tier-2 reader (tests/t2layers_cases.py; pinned on the host reader by tests/test_t2_layers_model_cpu.py).

  build(p, w, h, layers, order, flags, sty, table, ...) -> (codestream, want)
      p        G.TileParams of one tile, one precinct per resolution; w, h: the image = the tile
      order    0 LRCP .. 4 CPRL: with one precinct per resolution the packets are the loops over l, r, c in the five nestings
      flags    G.CS_SOP | G.CS_EPH | G.CS_PLT
      sty      None: HT blocks; else the Part-1 code-block style (0, 0x01 LAZY, 0x04 TERMALL, 0x05)
      table    per row of the tile's table dict(zbp=zero bit-planes, layers={layer: (passes, [bytes of every codeword segment the
               contribution touches])}); a row without layers is never included
      want     what the host reader must return for the file: rows, first_segment, segments, moves (in the order of dst),
               appendix_bytes -- and pieces, per row [(source position, bytes)]

Tag trees in their general form (B.10.2), "included before" bits, Table B.4, Lblock raised by the smallest increment that fits and
carried from layer to layer (B.10.7.1), one length per codeword segment (B.10.7.2), bit stuffing (B.10.1).  Block bytes are random
and hold no 0xFF."""
import numpy as np

import grok_amd as G


def seg_capacity(sty, idx):
    if sty is None or sty & 4:
        return 1
    if sty & 1:
        return 10 if idx == 0 else (2 if idx & 1 else 1)
    return 1 << 30


class TagTree:
    """the encoder's side of B.10.2: values at the leaves, minima above; encode(x, y, threshold) emits the bits a decoder needs to
    learn whether the leaf's value is below the threshold"""

    def __init__(self, gw, gh, values):
        self.dims = []
        w, h = gw, gh
        while True:
            self.dims.append((w, h))
            if w == 1 and h == 1:
                break
            w, h = (w + 1) >> 1, (h + 1) >> 1
        self.val = [np.asarray(values, np.int64).reshape(gh, gw)]
        for lv in range(1, len(self.dims)):
            w, h = self.dims[lv]
            below = self.val[-1]
            up = np.full((h, w), 1 << 40, np.int64)
            for y in range(below.shape[0]):
                for x in range(below.shape[1]):
                    up[y >> 1, x >> 1] = min(up[y >> 1, x >> 1], below[y, x])
            self.val.append(up)
        self.low = [np.zeros((h, w), np.int64) for w, h in self.dims]
        self.known = [np.zeros((h, w), bool) for w, h in self.dims]

    def encode(self, x, y, threshold, bits):
        low = 0
        for lv in range(len(self.dims) - 1, -1, -1):
            yy, xx = y >> lv, x >> lv
            if self.low[lv][yy, xx] < low:
                self.low[lv][yy, xx] = low
            while not self.known[lv][yy, xx] and self.low[lv][yy, xx] < threshold:
                if self.low[lv][yy, xx] >= self.val[lv][yy, xx]:
                    bits.append(1)
                    self.known[lv][yy, xx] = True
                else:
                    bits.append(0)
                    self.low[lv][yy, xx] += 1
            low = self.low[lv][yy, xx]


def put(bits, value, n):
    assert 0 <= value < (1 << n) or n == 0
    for k in range(n - 1, -1, -1):
        bits.append((value >> k) & 1)


def put_passes(bits, n):
    """Table B.4"""
    assert 1 <= n <= 164
    if n == 1:
        bits.append(0)
    elif n == 2:
        bits += [1, 0]
    elif n <= 5:
        bits += [1, 1]
        put(bits, n - 3, 2)
    elif n <= 36:
        bits += [1, 1, 1, 1]
        put(bits, n - 6, 5)
    else:
        bits += [1] * 9
        put(bits, n - 37, 7)


def stuff(bits):
    """B.10.1: a byte behind 0xFF carries seven bits; a header that ends on 0xFF is followed by a zero byte"""
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
    if out and out[-1] == 0xFF:
        out.append(0)
    return bytes(out)


def packet_sequence(order, layers, keys):
    """keys: the (res, comp) of the tile's precincts -> [(layer, key)] in file order"""
    res = sorted(set(r for r, _ in keys))
    comps = sorted(set(c for _, c in keys))
    has = set(keys)
    if order == 0:
        seq = [(l, (r, c)) for l in range(layers) for r in res for c in comps]
    elif order == 1:
        seq = [(l, (r, c)) for r in res for l in range(layers) for c in comps]
    elif order == 2:
        seq = [(l, (r, c)) for r in res for c in comps for l in range(layers)]
    else:
        seq = [(l, (r, c)) for c in comps for r in res for l in range(layers)]
    return [s for s in seq if s[1] in has]


def split_passes(sty, seg_idx, seg_fill, passes):
    """the passes of one contribution over the codeword segments it touches -> ([passes per touched segment], seg_idx, seg_fill)"""
    out, left = [], passes
    while left:
        cap = seg_capacity(sty, seg_idx)
        k = min(left, cap - seg_fill)
        out.append(k)
        seg_fill += k
        if seg_fill == cap:
            seg_idx, seg_fill = seg_idx + 1, 0
        left -= k
    return out, seg_idx, seg_fill


def build(p, w, h, layers, order, flags, sty, table, empty_packets=True, seed=1):
    blocks, _ = G.tile_layout(p)
    assert len(table) == len(blocks)
    rng = np.random.default_rng(seed)
    ht = sty is None
    # the precincts (one per resolution and component) with their bands' grids and rows
    keys = {}
    for row, b in enumerate(blocks):
        assert b.precinct == 0, "one precinct per resolution"
        keys.setdefault((b.res, b.comp), {}).setdefault(b.band, []).append(row)
    prec = {}
    for key, bands in keys.items():
        out = []
        for band in sorted(bands):
            rows = bands[band]
            gw = len(set(blocks[r].x0 for r in rows))
            gh = len(rows) // gw
            assert rows == list(range(rows[0], rows[0] + gw * gh))
            first = [min(table[r]["layers"]) if table[r]["layers"] else layers for r in rows]
            out.append(dict(rows=rows, gw=gw, gh=gh, incl=TagTree(gw, gh, first), zbp=TagTree(gw, gh, [table[r]["zbp"] for r in rows])))
        prec[key] = out
    state = [dict(included=False, lblock=3, passes=0, seg_idx=0, seg_fill=0, segs=[], pieces=[]) for _ in blocks]
    sop, eph, plt = bool(flags & G.CS_SOP), bool(flags & G.CS_EPH), bool(flags & G.CS_PLT)
    body = bytearray()
    lengths = []
    # where the packets start in the file is known once the headers in front of them are: positions relative to the first packet
    for number, (l, key) in enumerate(packet_sequence(order, layers, list(keys))):
        start = len(body)
        if sop:
            body += b"\xff\x91\x00\x04" + (number & 0xFFFF).to_bytes(2, "big")
        bits, todo = [], []
        contributes = any(l in table[r]["layers"] for band in prec[key] for r in band["rows"])
        if not contributes and empty_packets:
            bits.append(0)
        else:
            bits.append(1)
            for band in prec[key]:
                for i, r in enumerate(band["rows"]):
                    x, y = i % band["gw"], i // band["gw"]
                    s, t = state[r], table[r]
                    if not s["included"]:
                        band["incl"].encode(x, y, l + 1, bits)
                        if l not in t["layers"] or min(t["layers"]) != l:
                            assert l not in t["layers"]
                            continue
                        band["zbp"].encode(x, y, t["zbp"] + 1, bits)
                        s["included"] = True
                    else:
                        bits.append(1 if l in t["layers"] else 0)
                        if l not in t["layers"]:
                            continue
                    passes, lens = t["layers"][l]
                    put_passes(bits, passes)
                    opens = s["seg_fill"] == 0
                    ks, s["seg_idx"], s["seg_fill"] = split_passes(sty, s["seg_idx"], s["seg_fill"], passes)
                    s["passes"] += passes
                    assert len(ks) == len(lens), (r, l, ks, lens)
                    need = max(int(n).bit_length() - (int(k).bit_length() - 1) for k, n in zip(ks, lens))
                    inc = max(0, need - s["lblock"])
                    bits += [1] * inc + [0]
                    s["lblock"] += inc
                    for j, (k, n) in enumerate(zip(ks, lens)):
                        put(bits, n, s["lblock"] + int(k).bit_length() - 1)
                        if j == 0 and not opens:
                            s["segs"][-1][0] += n
                            s["segs"][-1][1] += k
                        else:
                            s["segs"].append([n, k])
                    if sum(lens):
                        todo.append((r, sum(lens)))
        body += stuff(bits)
        if eph:
            body += b"\xff\x92"
        for r, n in todo:
            state[r]["pieces"].append((len(body), n))
            body += rng.integers(0, 255, n, dtype=np.uint8).tobytes()
        lengths.append(len(body) - start)
    # the tile-part: SOT [PLT] SOD packets
    marker = b""
    if plt:
        entries = []
        for n in lengths:
            e = [n & 0x7F]
            n >>= 7
            while n:
                e.insert(0, 0x80 | (n & 0x7F))
                n >>= 7
            entries.append(bytes(e))
        z, cur = 0, b""
        for e in entries + [None]:
            if e is None or len(cur) + len(e) > 60000:
                marker += b"\xff\x58" + (3 + len(cur)).to_bytes(2, "big") + bytes([z]) + cur
                z, cur = z + 1, b""
            if e is not None:
                cur += e
    psot = 12 + len(marker) + 2 + len(body)
    part = b"\xff\x90\x00\x0a\x00\x00" + psot.to_bytes(4, "big") + b"\x00\x01" + marker + b"\xff\x93"
    hdr = bytearray(G.write_main_header(p, w, h, (flags & (G.CS_SOP | G.CS_EPH)) | G.CS_PROG(order), None))
    cod = hdr.index(b"\xff\x52") + 4                  # Scod, then SGcod: progression, layers (2), MCT; SPcod: levels, cbw, cbh, style
    assert hdr[cod + 1] == order
    hdr[cod + 2:cod + 4] = layers.to_bytes(2, "big")
    hdr[cod + 8] = 0x40 if ht else sty
    at = len(hdr) + len(part)
    cs = bytes(hdr) + part + bytes(body) + b"\xff\xd9"
    # what the reader must give
    rows = np.zeros(len(blocks), G.capi.CODED_DTYPE)
    first = np.zeros(len(blocks) + 1, np.uint32)
    segments, moves, pieces = [], [], []
    app = 0
    for r, s in enumerate(state):
        total = sum(n for _, n in s["pieces"])
        where = [(at + o, n) for o, n in s["pieces"]]
        pieces.append(where)
        rows["length"][r] = total
        rows["offset"][r] = where[0][0] if where else 0
        if ht:
            rows["missing_msbs"][r] = table[r]["zbp"] if s["included"] else 0
        elif total:
            rows["missing_msbs"][r] = (int(blocks[r].kmax) - table[r]["zbp"]) | s["passes"] << 8
        first[r] = len(segments)
        segments += [tuple(x) for x in s["segs"]]
        if len(where) > 1:
            rows["offset"][r] = len(cs) + app
            for src, n in where:
                moves.append((app, src, n, 1))
                app += n
    first[len(blocks)] = len(segments)
    want = dict(rows=rows, first_segment=first, segments=np.array(segments, G.capi.SEGMENT_DTYPE) if segments else np.zeros(0, G.capi.SEGMENT_DTYPE),
                moves=np.array(moves, G.capi.MOVE_DTYPE) if moves else np.zeros(0, G.capi.MOVE_DTYPE), appendix_bytes=app, pieces=pieces)
    return cs, want


def draw_table(p, layers, sty, seed, never=0.1, skip=0.3, max_len=60):
    """a fixed-seed table: blocks first included in any layer or never, layers skipped, contributions of 1 .. 6 passes within what
    the block's bit-planes hold, lengths of 0 .. max_len bytes per touched segment"""
    blocks, _ = G.tile_layout(p)
    rng = np.random.default_rng(seed)
    ht = sty is None
    table = []
    for b in blocks:
        kmax = max(1, int(b.kmax))
        zbp = int(rng.integers(0, kmax))
        room = 1 if ht else 3 * (kmax - zbp) - 2
        t = dict(zbp=zbp, layers={})
        if rng.random() >= never:
            first = int(rng.integers(0, layers))
            seg_idx = seg_fill = 0
            for l in range(first, layers):
                if room <= 0 or (l > first and rng.random() < skip):
                    continue
                passes = int(min(room, rng.integers(1, 7)))
                room -= passes
                ks, seg_idx, seg_fill = split_passes(sty, seg_idx, seg_fill, passes)
                lens = [int(rng.integers(0, max_len + 1)) for _ in ks]
                if ht and not sum(lens):
                    lens = [1]
                t["layers"][l] = (passes, lens)
        table.append(t)
    return table
