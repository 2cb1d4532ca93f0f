"""-m gpu: Tier-2 on the device under the GENERAL zero-bit-plane tag tree -- every code-block with its own missing_msbs, what a rate-
or quality-targeted encode signals -- on block tables of the test's choosing, handed to KT1's msbs instance (kernels_t2.hip) by
grk_amd_stage_assemble_msbs.

Every case is exact against two oracles: the host writer (grk_amd_write_tile_part with CS_BLOCK_MSBS), tile by tile and byte for byte,
and the project's Tier-2 reader (grk_amd_read_packets) over main header + the device's tile-parts + EOC, which must find the rows'
lengths AND their missing_msbs.  The shapes are the smallest at which the kernel can go wrong in a way of its own: one block (a tree
of height 1); grids odd at every level (3 x 5, 1 x 9, 9 x 1); each of the three launch widths; a packet the block loop passes twice;
a raw header beyond one LDS window; three-band packets, small precincts, every progression order, several tiles per call.  The value
patterns are those of tests/c/t2_msbs_units.cpp: constant, random, raster-rising / -falling (every node's minimum at its first / last
leaf), one leaf apart from all others at the first, a middle and the last place.  Conditions a case is there for are asserted ON THE
CPU, BEFORE THE LAUNCH, with tests/t2msbs_model.py (pinned on the host writer by tests/test_t2_msbs_model_cpu.py)."""
import numpy as np
import pytest

import grok_amd as G
import gpuutil as U
import t2model as M
import t2msbs_model as MM

pytestmark = pytest.mark.gpu

LIMIT = G.t2_max_block_bytes() + 1
EOC = b"\xff\xd9"
MSBS = G.CS_BLOCK_MSBS


def _coded(seed, nbytes):
    return np.random.default_rng(seed).integers(0, 256, nbytes, dtype=np.uint8)


def _lengths(rng, n, hi):
    """0 .. hi, a third of them 2^k - 1 (runs of ones in the header) and a few 2^k, 2^k + 1"""
    ln = rng.integers(0, hi + 1, n)
    k = rng.integers(1, int(hi).bit_length() + 1, n)
    pick = rng.random(n)
    ln = np.where(pick < 0.33, (1 << k) - 1, np.where(pick < 0.4, 1 << k, np.where(pick < 0.47, (1 << k) + 1, ln)))
    return np.clip(ln, 0, hi)


def _table(lengths, msbs, rng, coded_bytes):
    t = np.zeros(len(lengths), G.capi.CODED_DTYPE)
    t["length"] = lengths
    t["offset"] = rng.integers(0, coded_bytes - np.asarray(lengths, np.int64) + 1)
    t["missing_msbs"] = msbs
    return t


def patterns(n, rng):
    """the value patterns over a grid of n leaves in raster order -> [(name, values)]"""
    out = [("constant %d" % c, np.full(n, c)) for c in (0, 11, 63)]
    out.append(("random", rng.integers(0, 64, n)))
    rising = (np.arange(n) * 63 // max(n - 1, 1)) if n > 1 else np.array([63])
    out += [("rising", rising), ("falling", rising[::-1].copy())]
    for at in sorted(set([0, n // 2, n - 1])):
        v = np.full(n, 63); v[at] = 0
        w = np.zeros(n, np.int64); w[at] = 63
        out += [("a 0 among 63s at %d" % at, v), ("a 63 among 0s at %d" % at, w)]
    return out


def _host_parts(p, idx, table, coded, flags):
    bpt = len(table) // len(idx)
    return [G.write_tile_part(p, int(t), table[i * bpt:(i + 1) * bpt], coded, flags | MSBS) for i, t in enumerate(idx)]


def _read_back(p, parts, flags):
    body = bytearray()
    for i, part in enumerate(parts):
        body += part[:4] + bytes([i >> 8, i & 255]) + part[6:]
    hdr = G.write_main_header(p, p.tile_w * len(parts), p.tile_h, flags & ~MSBS, None)
    cs = np.frombuffer(hdr + bytes(body) + EOC, np.uint8)
    return G.read_packets(cs)["rows"], cs


def _check(p, idx, table, coded, flags=0, assemble=None):
    """device tile-parts == the host writer's under CS_BLOCK_MSBS; the reader finds the rows' lengths, missing_msbs and bytes in them"""
    want = _host_parts(p, idx, table, coded, flags)
    n, lens = (assemble or U.ctx().stage_assemble_msbs)(p, idx, table, coded, flags)
    assert [int(v) for v in lens] == [len(w) for w in want]
    assert n == sum(len(w) for w in want)
    got = U.ctx().fetch_assembled(0, n)
    at, parts = 0, []
    for i, w in enumerate(want):
        g = got[at:at + len(w)]
        if g.tobytes() != w:
            first = int(np.nonzero(g != np.frombuffer(w, np.uint8))[0][0])
            raise AssertionError("tile-part %d differs from byte %d of %d" % (i, first, len(w)))
        parts.append(g.tobytes())
        at += len(w)
    rows, cs = _read_back(p, parts, flags)
    assert np.array_equal(rows["length"], table["length"])
    assert np.array_equal(rows["missing_msbs"], table["missing_msbs"])
    view, src = memoryview(cs), memoryview(np.ascontiguousarray(coded))
    for o, s, ln in zip(rows["offset"].tolist(), table["offset"].tolist(), table["length"].tolist()):
        assert view[o:o + ln] == src[s:s + ln], "the row behind byte %d of the stream" % o
    return want


def _pattern_tiles(p, seed, hi):
    """one tile per value pattern (applied band by band of every packet), lengths drawn per tile -> (lengths, msbs: [tile][row], names)"""
    packets = M.packets_of(p)
    bpt = sum(k["rows"].size for k in packets)
    rng = np.random.default_rng(seed)
    names = [name for name, _ in patterns(max(gw * gh for k in packets for gw, gh, _ in k["bands"]), rng)]
    lengths, msbs = [], []
    for i in range(len(names)):
        v = np.zeros(bpt, np.int64)
        for k in packets:
            at = 0
            for gw, gh, _ in k["bands"]:
                pat = patterns(gw * gh, rng)
                v[k["rows"][at:at + gw * gh]] = pat[min(i, len(pat) - 1)][1]
                at += gw * gh
        lengths.append(_lengths(rng, bpt, hi)); msbs.append(v)
    return lengths, msbs, names


def _batch(lengths, msbs, seed, coded_bytes):
    rng = np.random.default_rng(seed)
    return np.concatenate([_table(ln, v, rng, coded_bytes) for ln, v in zip(lengths, msbs)])


def _largest(p):
    return max(k["rows"].size for k in M.packets_of(p))


def _longest_string(p, lengths, msbs):
    return max(int(MM.block_fields(k["bands"], ln[k["rows"]], v[k["rows"]])[3].max()) for ln, v in zip(lengths, msbs) for k in M.packets_of(p))


def _late_levels(p, v):
    """per band of the tile's largest packet: the levels with a node whose minimum is not at its first leaf"""
    k = max(M.packets_of(p), key=lambda q: q["rows"].size)
    out, at = [], 0
    for gw, gh, _ in k["bands"]:
        out.append((M.tag_tree_height(gw, gh), MM.late_minimum_levels(gw, gh, v[k["rows"][at:at + gw * gh]])))
        at += gw * gh
    return out


# ---- one block: a tree of height 1 -----------------------------------------------------------------------------------------------------

def test_one_block_at_0_1_kmax_minus_1_and_the_limit():
    p = G.TileParams.make(64, 64, 1, 8, 0)
    blocks, _ = G.tile_layout(p)
    assert len(blocks) == 1 and G.t2_max_block_msbs() == 63
    values = [0, 1, int(blocks[0].kmax) - 1, 63]
    coded = _coded(1, 4096)
    rng = np.random.default_rng(2)
    for ln in (0, 1, 7, 8, 300):
        table = np.concatenate([_table([ln], [v], rng, coded.size) for v in values])
        _check(p, [0, 1, 2, 3], table, coded)


# ---- grids odd at every level, one wave -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h,grid", [(192, 320, (3, 5)), (64, 576, (1, 9)), (576, 64, (9, 1))])
def test_odd_grids_under_every_value_pattern(w, h, grid):
    p = G.TileParams.make(w, h, 1, 8, 0)
    (k,) = M.packets_of(p)
    assert [(gw, gh) for gw, gh, _ in k["bands"]] == [grid] and _largest(p) <= 128
    lengths, msbs, names = _pattern_tiles(p, 10 + w, 70000)
    assert _longest_string(p, lengths, msbs) > 64
    height = M.tag_tree_height(*grid)
    assert _late_levels(p, msbs[names.index("falling")]) == [(height, set(range(1, height)))]
    assert _late_levels(p, msbs[names.index("rising")]) == [(height, set())]
    coded = _coded(11, 1 << 17)
    _check(p, list(range(len(names))), _batch(lengths, msbs, 12, coded.size), coded, G.CS_PLT)


# ---- the 64-, 256- and 1024-lane launches -----------------------------------------------------------------------------------------------

def test_the_64_lane_launch_passes_its_blocks_twice_over_three_bands():
    """120 blocks in the resolution-1 packet (three bands of 5 x 8): one wave, two passes; 30 % of the rows of one more tile are empty and
    stand at Kmax - 1, as the block coder leaves a block it skipped."""
    p = G.TileParams.make(40, 64, 1, 8, 1, cblk=(2, 2))
    assert 64 < _largest(p) == 120 <= 128
    lengths, msbs, names = _pattern_tiles(p, 20, 2047)
    blocks, _ = G.tile_layout(p)
    rng = np.random.default_rng(21)
    skip = rng.random(len(blocks)) < 0.3
    lengths.append(np.where(skip, 0, _lengths(rng, len(blocks), 2047)))
    msbs.append(np.where(skip, np.array([b.kmax - 1 for b in blocks]), rng.integers(0, 8, len(blocks))))
    assert 0.2 < skip.mean() < 0.4
    coded = _coded(22, 4096)
    _check(p, list(range(len(lengths))), _batch(lengths, msbs, 23, coded.size), coded, G.CS_SOP)


def test_the_256_lane_launch():
    """1008 blocks in the resolution-1 packet (three bands of 16 x 21): the <512> instance with 256 lanes, four passes; the raw headers of
    the patterns with 63s pass several windows of 512 words."""
    p = G.TileParams.make(128, 168, 1, 8, 1, cblk=(2, 2))
    assert 128 < _largest(p) == 1008 <= 1024
    lengths, msbs, names = _pattern_tiles(p, 30, 2047)
    big = max(M.packets_of(p), key=lambda q: q["rows"].size)
    i = names.index("random")
    assert MM.raw_bits(big["bands"], lengths[i][big["rows"]], msbs[i][big["rows"]]).size > 2 * 512 * 32
    assert all(late == set(range(1, height)) for height, late in _late_levels(p, msbs[i]))
    coded = _coded(31, 4096)
    _check(p, list(range(len(names))), _batch(lengths, msbs, 32, coded.size), coded, G.CS_EPH)


def test_the_1024_lane_launch_passes_an_odd_grid_twice():
    """41 x 35 = 1435 blocks of 4 x 4 samples in one band, a tree of seven levels: the <4096> instance, the block loop runs twice, every
    level is odd along one side at least.  (No table on this grid reaches the end of one 4096-word window: a block's string is at most
    2 nn + 63 + 39 bits, at most three of the four leaves of a node stand above it, and 1435 x (2.7 + 47.25 + 39) < 131 072 -- asserted
    below; the window's boundary is the next test's.)"""
    p = G.TileParams.make(164, 140, 1, 8, 0, cblk=(2, 2))
    (k,) = M.packets_of(p)
    assert [(gw, gh) for gw, gh, _ in k["bands"]] == [(41, 35)] and M.tag_tree_height(41, 35) == 7 and _largest(p) == 1435 > 1024
    lengths, msbs, names = _pattern_tiles(p, 40, 2047)
    assert _late_levels(p, msbs[names.index("random")]) == [(7, set(range(1, 7)))]
    assert _longest_string(p, lengths, msbs) > 64
    # the longest header this grid can have: three leaves of four at 63 above a 0, and -- in the model alone -- every length at the
    # limit - 1 (a tile-part of 1.5 GB); the tile goes to the device with lengths of its own
    x, y = np.meshgrid(np.arange(41), np.arange(35))
    heavy = np.where(((x | y) & 1).reshape(-1) == 1, 63, 0)
    heavy[0] = 63; heavy[1] = 0
    assert 100000 < MM.raw_bits(k["bands"], np.full(1435, LIMIT - 1), heavy).size < 4096 * 32
    lengths.append(_lengths(np.random.default_rng(43), 1435, 2047)); msbs.append(heavy)
    coded = _coded(41, 4096)
    _check(p, list(range(len(lengths))), _batch(lengths, msbs, 42, coded.size), coded)


def test_a_raw_header_beyond_one_window_of_4096_words():
    """61 x 49 = 2989 blocks: the same instance with a raw header that, by the model, passes the boundary of the first 4096-word window
    -- the stuffing chain carries its state over into a window whose bits the general tree wrote."""
    p = G.TileParams.make(244, 196, 1, 8, 0, cblk=(2, 2))
    (k,) = M.packets_of(p)
    assert [(gw, gh) for gw, gh, _ in k["bands"]] == [(61, 49)]
    rng = np.random.default_rng(50)
    x, y = np.meshgrid(np.arange(61), np.arange(49))
    heavy = np.where(((x | y) & 1).reshape(-1) == 1, rng.integers(56, 64, 2989), rng.integers(0, 4, 2989))
    ln = _lengths(rng, 2989, 2047)
    data, meters = MM.header(k["bands"], ln, heavy, 4096 * 32)
    assert len(meters["window"]) == 1 and 4096 * 32 < MM.raw_bits(k["bands"], ln, heavy).size < 2 * 4096 * 32
    coded = _coded(51, 4096)
    _check(p, [0], _table(ln, heavy, rng, coded.size), coded, G.CS_PLT)


# ---- three-band packets, precincts, progression orders, tiles ----------------------------------------------------------------------------

@pytest.mark.parametrize("order", range(5))
def test_three_components_two_levels_small_precincts_in_every_order(order):
    """128 x 128, 3 components, 2 levels, 64 x 64 precincts, 16 x 16 code-blocks: packets of three bands of 2 x 2 blocks with values of
    their own per band, SOP | EPH | PLT, three tiles in one call, each with its own values."""
    p = G.TileParams.make(128, 128, 3, 8, 2, cblk=(4, 4), precincts=[(6, 6)] * 3)
    blocks, _ = G.tile_layout(p)
    bpt = len(blocks)
    rng = np.random.default_rng(60 + order)
    band = np.array([b.band for b in blocks]); res = np.array([b.res for b in blocks])
    assert len(set(band[res > 0].tolist())) == 3 and int(np.array([b.precinct for b in blocks]).max()) > 0
    lengths, msbs = [], []
    for t in range(3):
        # a base per band, a draw per block on top: no two bands of a packet share their values
        v = (7 * band + 3 * t + rng.integers(0, 6 + 20 * t, bpt)) % 64
        lengths.append(_lengths(rng, bpt, 5000)); msbs.append(v)
    assert len(set(tuple(v.tolist()) for v in msbs)) == 3
    coded = _coded(61, 8192)
    _check(p, [5, 0, 65535], _batch(lengths, msbs, 62 + order, coded.size), coded, G.CS_SOP | G.CS_EPH | G.CS_PLT | G.CS_PROG(order))


# ---- against the constant tree, and what is refused --------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h,levels,cblk", [(40, 64, 1, (2, 2)), (128, 168, 1, (2, 2)), (164, 140, 0, (2, 2))])
def test_every_row_at_kmax_minus_1_is_the_constant_trees_output(w, h, levels, cblk):
    c = U.ctx()
    p = G.TileParams.make(w, h, 1, 8, levels, cblk=cblk)
    blocks, _ = G.tile_layout(p)
    rng = np.random.default_rng(70 + w)
    coded = _coded(71, 4096)
    table = _table(_lengths(rng, 2 * len(blocks), 2047), np.array([b.kmax - 1 for b in blocks] * 2), rng, coded.size)
    n0, lens0 = c.stage_assemble(p, [0, 1], table, coded, G.CS_PLT)
    plain = c.fetch_assembled(0, n0).tobytes()
    n1, lens1 = c.stage_assemble_msbs(p, [0, 1], table, coded, G.CS_PLT | MSBS)
    assert n1 == n0 and np.array_equal(lens0, lens1) and c.fetch_assembled(0, n1).tobytes() == plain
    assert plain == b"".join(_host_parts(p, [0, 1], table, coded, G.CS_PLT))


def test_a_row_above_the_limit_is_refused_on_the_host():
    c = U.ctx()
    p = G.TileParams.make(40, 64, 1, 8, 1, cblk=(2, 2))
    blocks, _ = G.tile_layout(p)
    rng = np.random.default_rng(80)
    coded = _coded(81, 4096)
    good = _table(_lengths(rng, 2 * len(blocks), 100), rng.integers(0, 64, 2 * len(blocks)), rng, coded.size)
    n0, _ = c.stage_assemble_msbs(p, [0, 1], good, coded)
    kept = c.fetch_assembled(0, n0).tobytes()
    assert kept == b"".join(_host_parts(p, [0, 1], good, coded, 0))
    bad = good.copy(); bad["missing_msbs"][len(blocks) + 3] = 64
    with pytest.raises(G.StageError, match=r"row %d: 64 zero bit-planes, the device writer takes at most 63" % (len(blocks) + 3)) as e:
        c.stage_assemble_msbs(p, [0, 1], bad, coded)
    assert e.value.code == G.ERR_UNSUPPORTED and e.value.reason.startswith("grk_amd_stage_assemble_msbs: ")
    bad = good.copy(); bad["length"][7] = LIMIT
    with pytest.raises(G.StageError, match=r"row 7: a length of %d bytes" % LIMIT) as e:
        c.stage_assemble_msbs(p, [0, 1], bad, _coded(82, LIMIT + 16))
    assert e.value.code == G.ERR_UNSUPPORTED
    with pytest.raises(G.StageError, match=r"a tile index beyond 65 535") as e:
        c.stage_assemble_msbs(p, [0, 65536], good, coded)
    assert e.value.code == G.ERR_INVALID
    # nothing was launched: what the last good call assembled is still there -- and the plain call still refuses the flag
    assert c.fetch_assembled(0, n0).tobytes() == kept
    with pytest.raises(G.StageError, match=r"per-block zero bit-planes") as e:
        c.stage_assemble(p, [0, 1], good, coded, MSBS)
    assert e.value.code == G.ERR_UNSUPPORTED
    assert c.fetch_assembled(0, n0).tobytes() == kept
