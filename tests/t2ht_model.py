"""A writer of HTJ2K codestreams whose code-blocks carry REFINEMENT passes, from tables and block bytes of the tests' choosing: beside
tests/t2layers_model.py (whose tag trees, Table B.4, bit stuffing and packet order it uses), for the readers that take such files
(grk_amd_read_packets_refine, grk_amd_read_packets_device_refine) and the whole-image decoders.  No encoder at hand writes these
files, so the tests do.  Pinned by tests/test_t2_ht_model_cpu.py: with every block at one pass the bytes are t2layers_model.build's.

The signalling (T.814 over T.800 B.10.7): an HT block's passes are one HT set -- Cleanup, SigProp, MagRef --, numbered across the
layers.  The cleanup pass is a codeword segment of its own, SigProp and MagRef share the next one: segment idx holds 2 passes where
idx is odd, else 1.  A segment's length field has Lblock + floor(log2 k) bits for the k passes of it in the contribution; a segment
filled by two contributions accumulates its length.  (The alternation is carried on beyond the first HT set only so that the files
the readers must REFUSE can be written: four passes at once, one and then three.)

  build(p, w, h, layers, order, flags, tables, tile=None, by_layer=False, ...) -> (codestream, want)
      p         G.TileParams of the image's HT tiles (the base: the tile's size is taken from `tile`), one precinct per resolution
      w, h      the image; tile: (TW, TH), or None: one tile
      tables    per tile (one tile: the table itself) per row dict(zbp=, layers={layer: (passes, [bytes of every codeword segment
                the contribution touches])}, data=the block's bytes, cleanup segment first, or None: drawn, without 0xFF)
      by_layer  the one tile divided into a tile-part per layer (LRCP), each with its own PLT where flags ask for PLT
      cut       > 0: the file ends `cut` bytes before the end of its last packet's header (that packet's bodies left out): want None
      want      t2layers_model.build's: rows, first_segment, segments, moves (in the order of dst), appendix_bytes, pieces -- over
                all tiles, tile after tile"""
import numpy as np

import grok_amd as G
from t2layers_model import TagTree, put, put_passes, stuff, packet_sequence


def seg_capacity(idx):
    return 2 if idx & 1 else 1


def split_passes(seg_idx, seg_fill, passes):
    """the passes of one contribution over the codeword segments it touches -> ([passes per touched segment], seg_idx, seg_fill)"""
    out, left = [], passes
    while left:
        cap = seg_capacity(seg_idx)
        k = min(left, cap - seg_fill)
        out.append(k)
        seg_fill += k
        if seg_fill == cap:
            seg_idx, seg_fill = seg_idx + 1, 0
        left -= k
    return out, seg_idx, seg_fill


def plt_marker(lengths):
    entries = []
    for n in lengths:
        e = [n & 0x7F]
        n >>= 7
        while n:
            e.insert(0, 0x80 | (n & 0x7F))
            n >>= 7
        entries.append(bytes(e))
    marker, z, cur = b"", 0, b""
    for e in entries + [None]:
        if e is None or len(cur) + len(e) > 60000:
            marker += b"\xff\x58" + (3 + len(cur)).to_bytes(2, "big") + bytes([z]) + cur
            z, cur = z + 1, b""
        if e is not None:
            cur += e
    return marker


def tile_packets(p, layers, order, flags, table, rng, empty_packets=True):
    """one tile's packets in file order -> ([(layer, header bytes incl. SOP / EPH, [(row, bytes)])], the rows' state)"""
    blocks, _ = G.tile_layout(p)
    assert len(table) == len(blocks)
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
    state = [dict(included=False, lblock=3, passes=0, seg_idx=0, seg_fill=0, segs=[], used=0) for _ in blocks]
    sop, eph = bool(flags & G.CS_SOP), bool(flags & G.CS_EPH)
    packets = []
    for number, (l, key) in enumerate(packet_sequence(order, layers, list(keys))):
        head = b""
        if sop:
            head += b"\xff\x91\x00\x04" + (number & 0xFFFF).to_bytes(2, "big")
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
                    ks, s["seg_idx"], s["seg_fill"] = split_passes(s["seg_idx"], s["seg_fill"], passes)
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
        head += stuff(bits)
        if eph:
            head += b"\xff\x92"
        bodies = []
        for r, n in todo:
            data = table[r].get("data")
            if data is None:
                piece = rng.integers(0, 255, n, dtype=np.uint8).tobytes()
            else:
                piece = bytes(data[state[r]["used"]:state[r]["used"] + n])
                assert len(piece) == n, "row %d: its bytes end before its contributions" % r
            state[r]["used"] += n
            bodies.append((r, piece))
        packets.append((l, head, bodies))
    for r, s in enumerate(state):
        data = table[r].get("data")
        assert data is None or s["used"] == len(data), "row %d: %d bytes given, %d signalled" % (r, len(data), s["used"])
    return packets, state


def build(p, w, h, layers, order, flags, tables, tile=None, by_layer=False, empty_packets=True, seed=1, cut=0):
    assert not p.reserved[0], "HT tiles"
    one = isinstance(tables[0], dict)
    if one:
        tables = [tables]
    layout = G.ImageLayout.make(w, h, *(tile or (w, h)))
    tiles = G.layout_tiles(layout, p)
    assert len(tiles) == len(tables) and (not by_layer or (len(tiles) == 1 and order == 0))
    rng = np.random.default_rng(seed)
    plt = bool(flags & G.CS_PLT)
    # every tile's tile-parts: (header, [packets]); a piece's place is known once everything in front of it is
    parts, states = [], []
    for t, (tp, table) in enumerate(zip(tiles, tables)):
        packets, state = tile_packets(tp, layers, order, flags, table, rng, empty_packets)
        states.append(state)
        groups = [[q for q in packets if q[0] == l] for l in range(layers)] if by_layer else [packets]
        for k, group in enumerate(groups):
            last = cut and t == len(tiles) - 1 and k == len(groups) - 1
            sizes = [len(head) + sum(len(d) for _, d in bodies) for _, head, bodies in group]
            if last:
                _, head, _ = group[-1]
                assert not plt and cut < len(head) - (6 if flags & G.CS_SOP else 0)
                group = group[:-1] + [(group[-1][0], head[:len(head) - cut], [])]
                sizes = sizes[:-1] + [len(head) - cut]
            marker = plt_marker(sizes) if plt else b""
            psot = 12 + len(marker) + 2 + sum(sizes)
            sot = b"\xff\x90\x00\x0a" + t.to_bytes(2, "big") + psot.to_bytes(4, "big") + bytes([k, len(groups)])
            parts.append((t, sot + marker + b"\xff\x93", group, psot))
    hflags = (flags & (G.CS_SOP | G.CS_EPH)) | G.CS_PROG(order)
    if len(tiles) == 1 and not by_layer:
        hdr = bytearray(G.write_main_header(p, w, h, hflags, None))
    else:
        per_tile = [sum(1 for q in parts if q[0] == t) for t in range(len(tiles))]
        hdr = bytearray(G.write_main_header_parts(layout, p, hflags, per_tile, [q[3] for q in parts]))
    cod = hdr.index(b"\xff\x52") + 4                  # Scod, then SGcod: progression, layers (2), MCT; SPcod: levels, cbw, cbh, style
    assert hdr[cod + 1] == order and hdr[cod + 8] == 0x40
    hdr[cod + 2:cod + 4] = layers.to_bytes(2, "big")
    cs = bytearray(hdr)
    where = [[[] for _ in s] for s in states]             # [tile][row]: (position, bytes) of its pieces
    for t, head, group, _ in parts:
        cs += head
        for _, phead, bodies in group:
            cs += phead
            for r, d in bodies:
                where[t][r].append((len(cs), len(d)))
                cs += d
    cs += b"\xff\xd9"
    if cut:
        return bytes(cs), None
    nrows = sum(len(s) for s in states)
    rows = np.zeros(nrows, G.capi.CODED_DTYPE)
    first = np.zeros(nrows + 1, np.uint32)
    segments, moves, pieces = [], [], []
    app, i = 0, 0
    for t, state in enumerate(states):
        for r, s in enumerate(state):
            pcs = where[t][r]
            pieces.append(pcs)
            rows["length"][i] = sum(n for _, n in pcs)
            rows["offset"][i] = pcs[0][0] if pcs else 0
            rows["missing_msbs"][i] = tables[t][r]["zbp"] if s["included"] else 0
            first[i] = len(segments)
            segments += [tuple(x) for x in s["segs"]]
            if len(pcs) > 1:
                rows["offset"][i] = len(cs) + app
                for src, n in pcs:
                    moves.append((app, src, n, 1))
                    app += n
            i += 1
    first[nrows] = len(segments)
    want = dict(rows=rows, first_segment=first, segments=np.array(segments, G.capi.SEGMENT_DTYPE) if segments else np.zeros(0, G.capi.SEGMENT_DTYPE),
                moves=np.array(moves, G.capi.MOVE_DTYPE) if moves else np.zeros(0, G.capi.MOVE_DTYPE), appendix_bytes=app, pieces=pieces)
    return bytes(cs), want


# ---- contribution patterns ------------------------------------------------------------------------------------------------------
# name -> the passes a block adds layer by layer (None: the layer is skipped); a pattern needs as many layers as it is long
PATTERNS = {
    "3": [3], "1|2": [1, 2], "1|1|1": [1, 1, 1], "2": [2], "1|-|1": [1, None, 1], "1": [1], "2|1": [2, 1], "1|1": [1, 1],
}


def contributions(pattern, first, cup, ref):
    """the table's `layers` of a block that adds PATTERNS[pattern] from layer `first` on, with a cleanup segment of `cup` bytes and
    a refinement segment of `ref` (SigProp and MagRef: the first half -- rounded down -- arrives with SigProp where they come apart)"""
    out, seg_idx, seg_fill, done = {}, 0, 0, 0
    for k, np_ in enumerate(PATTERNS[pattern]):
        if np_ is None:
            continue
        ks, seg_idx, seg_fill = split_passes(seg_idx, seg_fill, np_)
        lens = []
        for n in ks:
            if done == 0:
                lens.append(cup)
            elif done == 1 and n == 1 and sum(x for x in PATTERNS[pattern] if x) == 3:
                lens.append(ref // 2)                  # SigProp alone, MagRef to follow
            elif done == 2:
                lens.append(ref - ref // 2)
            else:
                lens.append(ref)
            done += n
        out[first + k] = (np_, lens)
    return out
