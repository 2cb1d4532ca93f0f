"""A packet header of the single-layer HT packets this encoder writes, restated in Python for the tests of Tier-2 on the device
(tests/test_gpu_t2_tables.py; pinned on the host writer by tests/test_t2_model_cpu.py).

  raw_bits(bands, lengths)   the header's bits BEFORE stuffing: '1' (the packet is not empty), then per band (gw, gh, kmax) and per
                             block in raster order: nn ones (inclusion: the new nodes of the block's tag-tree path), for the band's
                             first block kmax - 1 zeros (the zero-bit-plane tree's root), nn ones, the pass bit 0, Lblock's comma
                             code (inc ones, a zero), the length in 3 + inc bits
  walk(bits)                 the sequential stuffing walk: a byte that follows an 0xFF carries seven bits -> (bytes, where every
                             step starts, which steps are an 0xFF's)
  meters(nbits, starts, ff, win)
                             what the device's header kernel (KT1, kernels_t2.hip) meets on such a header: it cuts the chain of byte
                             starts into chunks of 256 raw bits, super-chunks of 16 chunks and LDS windows of `win` bits, and a chain
                             enters each at an offset of 0 .. 14 bits -- the entry offsets per kind of boundary, and the 0xFF steps
                             (an 0xFF and the seven bits behind it: 15 raw bits) that straddle a window boundary
  packets_of(params)         the packets of a tile in LRCP order, one precinct per resolution: rows and band grids from
                             grok_amd.tile_layout
"""
import numpy as np

CHUNK_BITS = 256
SUPER_BITS = 16 * CHUNK_BITS


def tag_tree_height(gw, gh):
    h = 1
    while gw * gh > 1:
        gw, gh, h = (gw + 1) >> 1, (gh + 1) >> 1, h + 1
    return h


def block_fields(bands, lengths):
    """-> per block, in the packet's order: nn, zeros, inc (int64 arrays)"""
    lengths = np.asarray(lengths, np.int64)
    nn, zeros = [], []
    for gw, gh, kmax in bands:
        height = tag_tree_height(gw, gh)
        m = (np.arange(gw, dtype=np.int64)[None, :] | np.arange(gh, dtype=np.int64)[:, None]).reshape(-1)
        ctz = np.zeros(m.size, np.int64)
        for z in range(1, 32):
            ctz += (m & ((1 << z) - 1)) == 0
        n = np.minimum(ctz + 1, height)
        n[0] = height
        z0 = np.zeros(m.size, np.int64)
        z0[0] = kmax - 1
        nn.append(n); zeros.append(z0)
    nn, zeros = np.concatenate(nn), np.concatenate(zeros)
    assert nn.size == lengths.size
    fl = np.zeros(lengths.size, np.int64)
    for k in range(1, 32):
        fl += lengths >= (1 << k)
    inc = np.maximum(fl + 1 - 3, 0)
    return nn, zeros, inc


def raw_bits(bands, lengths):
    """-> the header's raw bits, one uint8 per bit"""
    lengths = np.asarray(lengths, np.int64)
    nn, zeros, inc = block_fields(bands, lengths)
    width = 3 + inc
    nbits = 2 * nn + zeros + 1 + (inc + 1) + width
    at = 1 + np.concatenate([[0], np.cumsum(nbits)])
    total = int(at[-1])
    edge = np.zeros(total + 1, np.int64)               # runs of ones as +1 / -1 edges
    edge[0] += 1; edge[1] -= 1
    for start, n in ((at[:-1], nn), (at[:-1] + nn + zeros, nn), (at[:-1] + 2 * nn + zeros + 1, inc)):
        np.add.at(edge, start, 1)
        np.add.at(edge, start + n, -1)
    bits = (np.cumsum(edge)[:total] > 0).astype(np.uint8)
    first = at[:-1] + 2 * nn + zeros + 1 + inc + 1     # the length's first bit
    for j in range(int(width.max()) if width.size else 0):
        sel = width > j
        bits[first[sel] + j] = (lengths[sel] >> (width[sel] - 1 - j)) & 1
    return bits


def walk(bits):
    """-> (the stuffed header's bytes, the raw bit position every step starts at, whether that step is an 0xFF's)"""
    n = bits.size
    padded = np.concatenate([bits, np.zeros(16, np.uint8)]).astype(np.uint32)
    byte_at = np.zeros(n, np.uint32)
    for k in range(8):
        byte_at |= padded[k:k + n] << (7 - k)
    v = byte_at.tolist()
    out, starts = bytearray(), []
    p = 0
    while p < n:
        starts.append(p)
        b = v[p]
        out.append(b)
        if b == 0xFF:
            out.append(v[p + 8] >> 1 if p + 8 < n else 0)
            p += 15
        else:
            p += 8
    starts = np.asarray(starts, np.int64)
    return bytes(out), starts, byte_at[starts] == 0xFF


def meters(nbits, starts, ff, win_bits):
    """-> dict(chunk, super, window: the sets of entry offsets at the boundaries of each kind that the chain crosses;
               straddle: the number of 0xFF steps with raw bits on both sides of a window boundary)"""
    out = {}
    for name, step in (("chunk", CHUNK_BITS), ("super", SUPER_BITS), ("window", win_bits)):
        b = np.arange(step, nbits, step, dtype=np.int64)
        i = np.searchsorted(starts, b)
        ok = i < starts.size
        off = starts[i[ok]] - b[ok]
        assert off.size == 0 or (0 <= off.min() and off.max() <= 14)
        out[name] = set(int(x) for x in off)
        if name == "window":
            prev = i[ok] - 1
            out["straddle"] = int(np.count_nonzero(ff[prev] & (starts[prev] < b[ok]) & (starts[prev] + 15 > b[ok])))
    return out


def packets_of(params):
    """-> [dict(rows: the packet's rows of the tile's table in header order, bands: [(gw, gh, kmax)])], LRCP, one precinct per resolution"""
    import grok_amd as G
    blocks, _ = G.tile_layout(params)
    keys = {}
    for row, b in enumerate(blocks):
        assert b.precinct == 0, "one precinct per resolution"
        keys.setdefault((b.res, b.comp), {}).setdefault(b.band, []).append((row, b))
    out = []
    for key in sorted(keys):
        rows, bands = [], []
        for band in sorted(keys[key]):
            rb = keys[key][band]
            gw = len(set(b.x0 for _, b in rb))
            assert len(rb) % gw == 0 and [r for r, _ in rb] == list(range(rb[0][0], rb[0][0] + len(rb)))
            bands.append((gw, len(rb) // gw, int(rb[0][1].kmax)))
            rows += [r for r, _ in rb]
        out.append(dict(rows=np.asarray(rows, np.int64), bands=bands))
    return out


def header(bands, lengths, win_bits):
    """-> (the stuffed header, its meters)"""
    bits = raw_bits(bands, lengths)
    data, starts, ff = walk(bits)
    return data, meters(bits.size, starts, ff, win_bits)
