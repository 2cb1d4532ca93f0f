"""A packet header under the GENERAL zero-bit-plane tag tree -- every code-block with its own missing_msbs (GRK_AMD_CS_BLOCK_MSBS) --
restated in Python for the tests of KT1's msbs instance (tests/test_gpu_t2_msbs.py; pinned on the host writer by
tests/test_t2_msbs_model_cpu.py).  It stands beside tests/t2model.py, whose stuffing walk and meters it uses.

  levels(gw, gh, msbs)            the tree's node values: [level] a 2-D array, level 0 the leaves (raster), every level above the
                                  minimum of up to 2 x 2 children
  block_fields(bands, lengths, msbs)
                                  per block of the packet, in header order: nn (new nodes on its path), zeros (v_0 - v_nn: what its
                                  new nodes emit in front of their ones; v_nn = 0 above the root), inc, and its bit count
                                  2 nn + zeros + 1 + (inc + 1) + (3 + inc)
  raw_bits(bands, lengths, msbs)  the header's bits before stuffing: '1', then per block nn ones | for l = nn - 1 .. 0:
                                  (v_l - v_(l+1)) zeros, a one | the pass bit 0 | inc ones, a zero | the length in 3 + inc bits
  header(bands, lengths, msbs, win_bits)
                                  -> (the stuffed header, t2model's meters)
  late_minimum_levels(gw, gh, msbs)
                                  the levels (1 ..) with a node whose minimum is NOT at its first leaf (the one the uniform inclusion
                                  tree passes first): where a kernel that read a node's first child only would go wrong
`bands` is t2model's: [(gw, gh, kmax)] (kmax is not used: the values are the rows' own); lengths and msbs in the packet's header order."""
import numpy as np

import t2model as M


def levels(gw, gh, msbs):
    cur = np.asarray(msbs, np.int64).reshape(gh, gw)
    out = [cur]
    while cur.size > 1:
        h, w = cur.shape
        big = np.full((2 * ((h + 1) // 2), 2 * ((w + 1) // 2)), 1 << 30, np.int64)
        big[:h, :w] = cur
        cur = np.minimum(np.minimum(big[0::2, 0::2], big[0::2, 1::2]), np.minimum(big[1::2, 0::2], big[1::2, 1::2]))
        out.append(cur)
    assert len(out) == M.tag_tree_height(gw, gh)
    return out


def _band_paths(gw, gh, msbs):
    """-> (nn [blocks], v [height + 1][blocks]: the value of every block's node at every level, 0 above the root)"""
    lv = levels(gw, gh, msbs)
    height = len(lv)
    x = np.tile(np.arange(gw, dtype=np.int64), gh)
    y = np.repeat(np.arange(gh, dtype=np.int64), gw)
    m = x | y
    ctz = np.zeros(m.size, np.int64)
    for z in range(1, 32):
        ctz += (m & ((1 << z) - 1)) == 0
    nn = np.minimum(ctz + 1, height)
    nn[0] = height
    v = np.zeros((height + 1, m.size), np.int64)
    for l in range(height):
        v[l] = lv[l][y >> l, x >> l]
    return nn, v


def block_fields(bands, lengths, msbs):
    lengths = np.asarray(lengths, np.int64)
    msbs = np.asarray(msbs, np.int64)
    nn, zeros, at = [], [], 0
    for gw, gh, _ in bands:
        n, v = _band_paths(gw, gh, msbs[at:at + gw * gh])
        nn.append(n)
        zeros.append(v[0] - v[n, np.arange(n.size)])
        at += gw * gh
    nn, zeros = np.concatenate(nn), np.concatenate(zeros)
    assert nn.size == lengths.size == msbs.size
    fl = np.zeros(lengths.size, np.int64)
    for k in range(1, 32):
        fl += lengths >= (1 << k)
    inc = np.maximum(fl + 1 - 3, 0)
    return nn, zeros, inc, 2 * nn + zeros + 1 + (inc + 1) + (3 + inc)


def raw_bits(bands, lengths, msbs):
    lengths = np.asarray(lengths, np.int64)
    msbs = np.asarray(msbs, np.int64)
    nn, zeros, inc, nbits = block_fields(bands, lengths, msbs)
    start = 1 + np.concatenate([[0], np.cumsum(nbits)])
    bits = np.zeros(int(start[-1]), np.uint8)
    bits[0] = 1
    j, at = 0, 0
    for gw, gh, _ in bands:
        n, v = _band_paths(gw, gh, msbs[at:at + gw * gh])
        at += gw * gh
        for i in range(n.size):
            p = int(start[j])
            k = int(n[i])
            bits[p:p + k] = 1
            p += k
            for l in range(k - 1, -1, -1):
                p += int(v[l, i] - v[l + 1, i])
                bits[p] = 1
                p += 1
            p += 1                                     # the pass bit 0
            bits[p:p + int(inc[j])] = 1
            p += int(inc[j]) + 1
            w = 3 + int(inc[j])
            ln = int(lengths[j])
            for q in range(w):
                bits[p + q] = (ln >> (w - 1 - q)) & 1
            assert p + w == int(start[j + 1])
            j += 1
    return bits


def header(bands, lengths, msbs, win_bits):
    bits = raw_bits(bands, lengths, msbs)
    data, starts, ff = M.walk(bits)
    return data, M.meters(bits.size, starts, ff, win_bits)


def late_minimum_levels(gw, gh, msbs):
    lv = levels(gw, gh, msbs)
    out = set()
    for l in range(1, len(lv)):
        h, w = lv[l].shape
        first = lv[0][(np.arange(h) << l)[:, None], (np.arange(w) << l)[None, :]]
        if np.any(lv[l] < first):
            out.add(l)
    return out
