"""-m gpu: Tier-2 on the device (KT1 headers, KT1b frames, KT2 gather: kernels_t2.hip) on block tables of the test's choosing, handed
to the kernels by grk_amd_stage_assemble.  The other Tier-2 files reach the kernels through pixels and the block coder, with whatever
lengths come out; here the table is made for the kernels' own edges.

Every case is exact against two oracles: the host writer (grk_amd_write_tile_part, pinned on the reference's files elsewhere), tile by
tile and length by length, and the project's Tier-2 reader (grk_amd_read_packets) over main header + the device's tile-parts + EOC,
which must find the table's lengths and, at its offsets, the rows' bytes.  Every case asserts ON THE CPU, BEFORE THE LAUNCH, that its
table meets the condition it is there for -- with tests/t2model.py (pinned on the host writer by tests/test_t2_model_cpu.py) for the
stuffing chain's boundaries.  The tables are fixed-seed draws, steered where needed by drawing a few lengths ahead of a boundary again.

No case hands the kernels a length at or above the device writer's limit or an offset outside the coded bytes: the stage call
refuses those on the host, and that refusal is what test_refusals_come_from_the_host_check checks."""
import numpy as np
import pytest

import grok_amd as G
import gpuutil as U
import j2kparse
import synth
import t2model as M

pytestmark = pytest.mark.gpu

LIMIT = G.t2_max_block_bytes() + 1            # lengths the device writer takes lie below this
EOC = b"\xff\xd9"
ALL15 = set(range(15))


def _coded(seed, nbytes):
    return np.random.default_rng(seed).integers(0, 256, nbytes, dtype=np.uint8)


def _draw_lengths(rng, n, lo, hi):
    """lengths lo .. hi, half of them of the form 2^k - 1: runs of ones in the header, the stuff 0xFF bytes are made of"""
    ln = rng.integers(lo, hi + 1, n)
    ones = (1 << rng.integers(max(int(lo).bit_length(), 1), int(hi).bit_length() + 1, n)) - 1
    pick = rng.random(n) < 0.5
    ln[pick] = np.clip(ones[pick], lo, hi)
    return ln


def _table(lengths, rng, coded_bytes):
    t = np.zeros(len(lengths), G.capi.CODED_DTYPE)
    t["length"] = lengths
    t["offset"] = rng.integers(0, coded_bytes - np.asarray(lengths, np.int64) + 1)
    return t


def _host_parts(p, idx, table, coded, flags):
    bpt = len(table) // len(idx)
    return [G.write_tile_part(p, int(t), table[i * bpt:(i + 1) * bpt], coded, flags) for i, t in enumerate(idx)]


def _read_back(p, parts, flags):
    """the tile-parts as the tiles of one row of an image, behind its main header, through the reader -> (rows, the stream, the header's
    length).  (Isot is rewritten to the tile's place in that row: the frame's own bytes are the host writer's comparison.)"""
    body = bytearray()
    for i, part in enumerate(parts):
        body += part[:4] + bytes([i >> 8, i & 255]) + part[6:]
    hdr = G.write_main_header(p, p.tile_w * len(parts), p.tile_h, flags, None)
    cs = np.frombuffer(hdr + bytes(body) + EOC, np.uint8)
    return G.read_packets(cs)["rows"], cs, len(hdr)


def _check(p, idx, table, coded, flags=0, want=None):
    """device tile-parts == the host writer's; the reader finds the table in them.  -> the host writer's tile-parts"""
    if want is None:
        want = _host_parts(p, idx, table, coded, flags)
    n, lens = U.ctx().stage_assemble(p, idx, table, coded, flags)
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
    rows, cs, _ = _read_back(p, parts, flags)
    assert np.array_equal(rows["length"], table["length"])
    view, src = memoryview(cs), memoryview(np.ascontiguousarray(coded))
    for o, s, ln in zip(rows["offset"].tolist(), table["offset"].tolist(), table["length"].tolist()):
        assert view[o:o + ln] == src[s:s + ln], "the row behind byte %d of the stream" % o
    return want


def _largest(packets):
    return max(k["rows"].size for k in packets)


# ---- a, b, c: the stuffing chain ----------------------------------------------------------------------------------------------------

def _stuffing_tables(p, ntiles, lo, hi, win_bits, seed, want_window):
    """ntiles draws; then, for every window entry offset (or class of offsets) of want_window that no tile's largest packet has, the
    lengths of a few blocks in front of the window boundary of a tile whose own offset others have too are drawn again until it has.
    -> (lengths [tile][row], the meters' unions over the batch)"""
    packets = M.packets_of(p)
    big = max(packets, key=lambda k: k["rows"].size)
    bpt = sum(k["rows"].size for k in packets)
    rng = np.random.default_rng(seed)
    lengths = [_draw_lengths(rng, bpt, lo, hi) for _ in range(ntiles)]

    def big_meter(t):
        return M.header(big["bands"], lengths[t][big["rows"]], win_bits)[1]

    mt = [big_meter(t) for t in range(ntiles)]
    for m in mt:
        assert len(m["window"]) >= 1, "the largest packet's raw header has to pass a window boundary"
    klass = lambda m: [i for i, c in enumerate(want_window) if m["window"] & c]
    for i, c in enumerate(want_window):
        if any(i in klass(m) for m in mt):
            continue
        counts = [sum(1 for m in mt if set(klass(m)) & set(klass(mt[t]))) for t in range(ntiles)]
        t = int(np.argmax(counts))                   # a tile of the most crowded class
        assert counts[t] > 1
        # where the boundary falls among the packet's blocks: a dozen blocks up to it are drawn again
        nn, zeros, inc = M.block_fields(big["bands"], lengths[t][big["rows"]])
        edge = int(np.searchsorted(np.cumsum(2 * nn + zeros + 5 + 2 * inc), win_bits))
        rows = big["rows"][edge - 10:edge + 2]
        for _ in range(2000):
            lengths[t][rows] = _draw_lengths(rng, rows.size, lo, hi)
            m = big_meter(t)
            if m["window"] & c:
                mt[t] = m
                break
        else:
            raise AssertionError("no draw enters the window at %s" % sorted(c))
    if not any(m["straddle"] for m in mt):
        raise AssertionError("no 0xFF step across a window boundary")
    total = dict(chunk=set(), super=set(), window=set(), straddle=0)
    for t in range(ntiles):
        for k in packets:
            m = mt[t] if k is big else M.header(k["bands"], lengths[t][k["rows"]], win_bits)[1]
            for name in ("chunk", "super", "window"):
                total[name] |= m[name]
            total["straddle"] += m["straddle"]
    return lengths, total


def _batch(lengths, seed, coded_bytes):
    rng = np.random.default_rng(seed)
    return np.concatenate([_table(ln, rng, coded_bytes) for ln in lengths])


def test_stuffing_chain_of_the_256_lane_launch_meets_every_boundary_at_every_offset():
    """a. 1008 blocks in the resolution-1 packet: the <512> instance with 256 lanes, ~19 000 raw bits -- one window boundary (16 384
    bits) per tile.  Over the batch the chain enters a chunk, a super-chunk AND a window at every offset 0 .. 14, and an 0xFF step lies
    across a window boundary."""
    p = G.TileParams.make(128, 168, 1, 8, 1, cblk=(2, 2))
    assert 128 < _largest(M.packets_of(p)) == 1008 <= 1024
    lengths, total = _stuffing_tables(p, 64, 64, 2047, 512 * 32, 1, [{o} for o in range(15)])
    assert total["chunk"] == ALL15 and total["super"] == ALL15 and total["window"] == ALL15 and total["straddle"] >= 1, total
    coded = _coded(2, 4096)
    _check(p, list(range(64)), _batch(lengths, 3, coded.size), coded)


def test_stuffing_chain_of_the_1024_lane_launch_carries_its_state_over_a_window():
    """b. 12 288 blocks in the resolution-1 packet: the <4096> instance, twelve passes of 1024 lanes, ~200 000 raw bits -- one window
    boundary (131 072 bits) per tile, entered at offset 0, at one of 1 .. 7 and, behind an 0xFF across the boundary, at one of 8 .. 14."""
    p = G.TileParams.make(512, 512, 1, 8, 1, cblk=(2, 2))
    assert _largest(M.packets_of(p)) == 12288 > 1024
    classes = [{0}, set(range(1, 8)), set(range(8, 15))]
    lengths, total = _stuffing_tables(p, 4, 32, 255, 4096 * 32, 4, classes)
    assert all(total["window"] & c for c in classes) and total["straddle"] >= 1, total
    assert total["chunk"] == ALL15 and total["super"] == ALL15, total
    coded = _coded(5, 4096)
    _check(p, [0, 1, 2, 3], _batch(lengths, 6, coded.size), coded, G.CS_EPH)


def test_stuffing_chain_of_the_64_lane_launch():
    """c. 120 blocks in the resolution-1 packet: one wave, two passes over the blocks."""
    p = G.TileParams.make(40, 64, 1, 8, 1, cblk=(2, 2))
    packets = M.packets_of(p)
    assert 64 < _largest(packets) == 120 <= 128
    rng = np.random.default_rng(7)
    bpt = sum(k["rows"].size for k in packets)
    lengths = [_draw_lengths(rng, bpt, 64, 2047) for _ in range(16)]
    chunk = set()
    for ln in lengths:
        for k in packets:
            chunk |= M.header(k["bands"], ln[k["rows"]], 512 * 32)[1]["chunk"]
    assert chunk == ALL15, chunk
    coded = _coded(8, 4096)
    _check(p, list(range(16)), _batch(lengths, 9, coded.size), coded, G.CS_SOP)


# ---- d: the length field ----------------------------------------------------------------------------------------------------------------

def test_length_field_extremes_on_the_root_and_on_a_leaf_of_a_tree_of_nine_levels():
    """d. One row of 256 blocks per band (tag trees of height 9): the lengths 0, 1, 7, 8, every 2^k - 1 and 2^k below the limit and
    the limit - 1, each on a band's first block (all nine nodes of its path are new, Kmax - 1 zeros) and on a block with one new node."""
    p = G.TileParams.make(2048, 8, 1, 8, 1, cblk=(2, 2))
    packets = M.packets_of(p)
    assert all(M.tag_tree_height(gw, gh) == 9 for k in packets for gw, gh, _ in k["bands"])
    extremes = sorted(set([0, 1, 7, 8, LIMIT - 1] + [v for k in range(LIMIT.bit_length() - 1) for v in ((1 << k) - 1, 1 << k)]))
    assert extremes[-1] == LIMIT - 1 and extremes[-2] == LIMIT >> 1 and all(v < LIMIT for v in extremes)
    roots = [int(k["rows"][at]) for k in packets for at in np.cumsum([0] + [gw * gh for gw, gh, _ in k["bands"]])[:-1]]
    assert len(roots) == 4
    ntiles = -(-len(extremes) // len(roots))
    bpt = sum(k["rows"].size for k in packets)
    rng = np.random.default_rng(10)
    lengths = [rng.integers(0, 41, bpt) for _ in range(ntiles)]
    on_root, on_leaf = set(), set()
    for i, v in enumerate(extremes):
        t, r = divmod(i, len(roots))
        lengths[t][roots[r]] = v                       # x = 0: the whole path
        lengths[t][roots[r] + 1 + 2 * (i % 100)] = v   # x odd: nn = 1
        on_root.add(v); on_leaf.add(v)
    nn = np.concatenate([M.block_fields(k["bands"], lengths[0][k["rows"]])[0] for k in packets])
    rows = np.concatenate([k["rows"] for k in packets])
    assert all(nn[rows == r][0] == 9 for r in roots) and all(nn[rows == r + 1 + 2 * j][0] == 1 for r in roots for j in range(100))
    assert on_root == on_leaf == set(extremes)
    coded = _coded(11, LIMIT)
    table = _batch(lengths, 12, coded.size)
    assert int(table["length"].max()) == LIMIT - 1 and int(table["length"].astype(np.int64).sum()) < 16 << 20
    _check(p, list(range(ntiles)), table, coded, G.CS_PLT)


# ---- e: empty and flat tables ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h,lanes", [(40, 64, 64), (128, 168, 256), (512, 512, 1024)])
@pytest.mark.parametrize("length", [0, 7])
def test_empty_and_flat_tables_at_the_three_launch_widths(w, h, lanes, length):
    """e. Every length 0 (Lblock stays 3, three zero bits: the header is the tag trees' ones and zeros alone); every length 7: ones but
    for two zeros per block -- the flat frame's runs of ones by construction, an 0xFF wherever a block's path has three new nodes or
    more and the chain stands right."""
    p = G.TileParams.make(w, h, 1, 8, 1, cblk=(2, 2))
    packets = M.packets_of(p)
    big = _largest(packets)
    assert (64 if big <= 128 else 256 if big <= 1024 else 1024) == lanes
    bpt = sum(k["rows"].size for k in packets)
    k = max(packets, key=lambda q: q["rows"].size)
    data, _ = M.header(k["bands"], np.full(k["rows"].size, length), 512 * 32)
    bits = M.raw_bits(k["bands"], np.full(k["rows"].size, length))
    assert bits.size - int(bits.sum()) == (5 if length == 0 else 2) * k["rows"].size + sum(kmax - 1 for _, _, kmax in k["bands"])
    if length == 7:
        assert 0xFF in data
    coded = _coded(13, 64)
    lengths = [np.full(bpt, length)] * 2
    _check(p, [0, 1], _batch(lengths, 14, coded.size), coded, G.CS_PLT | G.CS_EPH)


# ---- f: the gather's alignments ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flags", [0, G.CS_SOP | G.CS_EPH])
def test_gather_copies_at_every_pair_of_alignments_and_every_short_length(flags):
    """f. wave_copy's head (up to the destination's 16-byte boundary), vector body (aligned stores, unaligned loads) and tail: among
    the blocks of at least 48 bytes every pair (destination & 15, source & 15) occurs, and every length 0 .. 47 occurs.  The
    destinations are where the reader finds the rows in the host writer's tile-part -- the device's output starts on a 16-byte
    boundary --; the sources are then dealt out so that every destination alignment meets every source alignment."""
    p = G.TileParams.make(128, 168, 1, 8, 1, cblk=(2, 2))
    bpt = sum(k["rows"].size for k in M.packets_of(p))
    rng = np.random.default_rng(15 + flags)
    ln = rng.integers(48, 200, bpt)
    short = rng.choice(bpt, 96, replace=False)
    ln[short] = np.arange(96) % 48
    coded = _coded(16, 4096)
    table = _table(ln, rng, coded.size - 16)
    want = _host_parts(p, [0], table, coded, flags)
    rows, _, hdr_len = _read_back(p, want, flags)
    dst = (rows["offset"].astype(np.int64) - hdr_len) & 15
    turn = np.zeros(16, np.int64)
    for r in np.nonzero(ln >= 48)[0]:
        table["offset"][r] = (int(table["offset"][r]) & ~15) + turn[dst[r]] % 16
        turn[dst[r]] += 1
    assert int((table["offset"] + table["length"]).max()) <= coded.size
    big = ln >= 48
    pairs = set(zip(dst[big].tolist(), (table["offset"][big] & 15).tolist()))
    assert len(pairs) == 256 and set(ln.tolist()) >= set(range(48))
    _check(p, [0], table, coded, flags)
    assert U.ctx().assembled_device_ptr() % 16 == 0


# ---- g: PLT ----------------------------------------------------------------------------------------------------------------------------

def _packet_of_exactly(k, total, rng):
    """three lengths whose packet -- header and bodies -- is `total` bytes long"""
    n = k["rows"].size
    share = rng.integers(45, 56, n).astype(np.float64)
    hdr = 0
    for _ in range(8):
        body = total - hdr
        ln = np.floor(share / share.sum() * body).astype(np.int64)
        ln[-1] = body - ln[:-1].sum()
        now = len(M.header(k["bands"], ln, 512 * 32)[0])
        if now == hdr:
            return ln
        hdr = now
    raise AssertionError("no lengths make a packet of %d bytes" % total)


def test_plt_closes_a_marker_segment_at_65532_and_at_65531_bytes_of_lengths():
    """g. 40 960 packets per tile (8 x 8 precincts of 4 x 4 code-blocks), two tiles in one batch.  Packet lengths of 127 | 128 and 16 383 |
    16 384 and 2 097 151 | 2 097 152 bytes -- where a number in PLT grows by a byte; the last two of three blocks each, so that no block
    reaches the limit -- and two bytes for every other packet: in tile one the first marker segment fills to 65 532 bytes exactly
    (Lplt 65 535), in tile two, with one one-byte number less, to 65 531 where the next two-byte number does not fit (Lplt 65 534)."""
    p = G.TileParams.make(1280, 1024, 1, 8, 1, cblk=(2, 2), precincts=[(2, 2), (3, 3)])
    blocks, _ = G.tile_layout(p)
    res = np.array([b.res for b in blocks]); prc = np.array([b.precinct for b in blocks])
    npk = 2 * (int(prc.max()) + 1)
    assert npk == 40960
    rng = np.random.default_rng(17)
    edges = [127, 128, 16383, 16384, 2097151, 2097152]
    lengths = []
    for tile, specials in enumerate(([127] + edges, edges)):
        ln = np.where(res == 0, rng.integers(126, 161, len(blocks)), rng.integers(43, 61, len(blocks)))
        for i, v in enumerate(specials):
            rows = np.nonzero((res == 1) & (prc == 100 + 7 * i + tile))[0]
            k = dict(rows=rows, bands=[(1, 1, int(blocks[r].kmax)) for r in rows])
            assert rows.size == 3 and [blocks[r].band for r in rows] == sorted(blocks[r].band for r in rows)
            ln[rows] = _packet_of_exactly(k, v, rng)
        lengths.append(ln)
    assert max(int(ln.max()) for ln in lengths) < LIMIT
    coded = _coded(18, LIMIT)
    table = _batch(lengths, 19, coded.size)
    flags = G.CS_PLT
    want = _host_parts(p, [0, 1], table, coded, flags)
    for part, first_lplt, specials in zip(want, (65535, 65534), ([127] + edges, edges)):
        segs = j2kparse.plt_segments(part)
        assert [s[1] for s in segs] == list(range(len(segs))) and len(segs) == 2
        assert segs[0][0] == first_lplt, [s[0] for s in segs]
        vals = segs[0][2] + segs[1][2]
        assert len(vals) == npk and sorted(v for v in vals if v < 128 or v > 16383) == sorted(v for v in specials if v < 128 or v > 16383)
        assert set(edges) <= set(vals)
        # (the segment closes where the test says it does: the number that opens the second one takes two bytes)
        assert 128 <= segs[1][2][0] < 16384
    got = _check(p, [0, 1], table, coded, flags, want=want)
    assert [j2kparse.plt_segments(g)[0][0] for g in got] == [65535, 65534]


# ---- h: bookkeeping over the tiles of a batch --------------------------------------------------------------------------------------------

def test_tiles_of_very_different_totals_in_one_batch():
    """h. Five tiles: a few bytes, all empty, ~20 MB, a few KB, all empty -- lengths, places and totals as the device keeps them for an
    exchange (grk_amd_assembled_table_ptr), tile indices 0 and 65 535."""
    c = U.ctx()
    p = G.TileParams.make(40, 64, 1, 8, 1, cblk=(2, 2))
    bpt = sum(k["rows"].size for k in M.packets_of(p))
    rng = np.random.default_rng(20)
    lengths = [rng.integers(0, 3, bpt), np.zeros(bpt, np.int64), rng.integers(100000, 150000, bpt), rng.integers(0, 64, bpt),
               np.zeros(bpt, np.int64)]
    idx = [65535, 0, 7, 65535, 300]
    coded = _coded(21, 1 << 18)
    table = _batch(lengths, 22, coded.size)
    want = _check(p, idx, table, coded, G.CS_PLT | G.CS_SOP)
    sizes = np.array([len(w) for w in want], np.uint64)
    assert sizes[2] > 15 << 20 and sizes[1] == sizes[4] < 256 and [w[4:6] for w in want] == [bytes([i >> 8, i & 255]) for i in idx]
    places = U.from_dev_ptr(c.assembled_table_ptr(0), 8 * 5).view(np.uint64)
    assert np.array_equal(places, np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.uint64))
    assert np.array_equal(U.from_dev_ptr(c.assembled_table_ptr(1), 4 * 5).view(np.uint32), sizes.astype(np.uint32))
    assert U.from_dev_ptr(c.assembled_table_ptr(2), 16).view(np.uint64).tolist() == [int(sizes.sum()), int(sizes.sum())]


# ---- i: what the stage call refuses, and what it leaves alone ------------------------------------------------------------------------------

def test_refusals_come_from_the_host_check():
    """i. Nothing of these reaches a kernel: the texts are the host check's (a kernel's refusal -- status bit 2 -- reads 'a code-block
    longer than the device writer takes')."""
    c = U.ctx()
    p = G.TileParams.make(40, 64, 1, 8, 1, cblk=(2, 2))
    bpt = sum(k["rows"].size for k in M.packets_of(p))
    coded = _coded(23, 4096)
    rng = np.random.default_rng(24)
    good = _table(rng.integers(0, 100, 2 * bpt), rng, coded.size)
    n0, _ = c.stage_assemble(p, [0, 1], good, coded)
    kept = c.fetch_assembled(0, n0).tobytes()

    def refused(code, text, idx=(0, 1), table=good, flags=0, coded=coded):
        with pytest.raises(G.StageError, match=text) as e:
            c.stage_assemble(p, list(idx), table, coded, flags)
        assert e.value.code == code and e.value.reason.startswith("grk_amd_stage_assemble: ")

    bad = good.copy(); bad["offset"][bpt + 5] = coded.size - 10; bad["length"][bpt + 5] = 11
    refused(G.ERR_INVALID, r"row %d: offset 4086 \+ length 11 lies beyond the 4096 coded bytes" % (bpt + 5), table=bad)
    bad = good.copy(); bad["offset"][3] = (1 << 64) - 4; bad["length"][3] = 8          # (offset + length wraps around 2^64)
    refused(G.ERR_INVALID, r"row 3: .* lies beyond", table=bad)
    bad = good.copy(); bad["length"][7] = LIMIT
    refused(G.ERR_UNSUPPORTED, r"row 7: a length of %d bytes, the device writer takes less than %d" % (LIMIT, LIMIT), table=bad,
            coded=_coded(25, LIMIT + 16))
    refused(G.ERR_INVALID, r"a tile index beyond 65 535", idx=(0, 65536))
    refused(G.ERR_UNSUPPORTED, r"per-block zero bit-planes", flags=G.CS_BLOCK_MSBS)
    # ... and nothing was launched: what the last good call assembled is still there
    assert c.fetch_assembled(0, n0).tobytes() == kept
    limit_ok = good.copy(); limit_ok["length"][7] = LIMIT - 1; limit_ok["offset"][7] = 3
    big = _coded(25, LIMIT + 16)
    _check(p, [0, 1], limit_ok, big)


def test_an_encode_and_its_assembly_are_what_they_were_around_a_stage_call():
    """grk_amd_encode_tiles + grk_amd_assemble_device behind a stage call, and with a stage call of the same parameters BETWEEN the two:
    the stage call's rows and bytes live in buffers of their own."""
    c = U.ctx()
    p = G.TileParams.make(160, 128, 3, 8, 3)
    px = synth.g2(3, 2 * 128, 160, 8, seed=26).reshape(2, 3, 128, 160)
    bpt = len(G.tile_layout(p)[0])
    coded = _coded(27, 4096)
    other = _table(np.random.default_rng(28).integers(0, 300, 2 * bpt), np.random.default_rng(29), coded.size)
    flags = G.CS_PLT | G.CS_PROG(2)
    want_other = _host_parts(p, [4, 5], other, coded, flags)
    n, _ = c.stage_assemble(p, [4, 5], other, coded, flags)
    assert c.fetch_assembled(0, n).tobytes() == b"".join(want_other)
    table, enc = c.encode_host(p, px, ntiles=2)
    want = b"".join(_host_parts(p, [1, 2], table, enc, flags))
    n, lens = c.assemble_device(p, [1, 2], flags)
    assert c.fetch_assembled(0, n).tobytes() == want
    n, _ = c.stage_assemble(p, [4, 5], other, coded, flags)
    assert c.fetch_assembled(0, n).tobytes() == b"".join(want_other)
    n, lens2 = c.assemble_device(p, [1, 2], flags)
    assert c.fetch_assembled(0, n).tobytes() == want and np.array_equal(lens, lens2)
