"""CPU: the decode path's host planning (grok_amd/csrc/decode_plan.cpp) -- which block goes to which Part-1 decoder, which table
rows are refused, the HT launch list and refinement table, which blocks a window skips, the reduced decode's segment list, the
shape and kernel instance of an inverse DWT level -- through the small driver tests/c/decode_plan_units.cpp, built on first use with g++ together with decode_plan.cpp and
geometry.cpp: no GPU, no HIP, no libgrok_amd.so.  -D_GLIBCXX_ASSERTIONS: an index past the end of a std::vector aborts.

What the planner does, where one might expect otherwise:
  * the lane lists are sorted by length in 4-byte buckets: within a group the lengths do not increase from BUCKET to bucket;
  * with t1_lanes = 1 the lists stand exactly when 0.9 ns x all bytes exceeds 2.5 ns x the longest block: blocks of EQUAL length
    always take the lanes (0.9 x 64 blocks' bytes is above 2.5 x one block's), and what goes to K8 alone is a few short blocks
    beside one much longer one.  The model's 10 ns per lane byte cannot turn that decision: a lane block is no longer than a
    quarter of the longest (or 64 bytes), and 64 of them weigh more at 0.9 ns than one does at 10;
  * a 64 x 64 tile with 32 x 32 blocks has ONE block per band of the top resolution, which no window can do without; the corner
    windows are checked with 16 x 16 blocks (four per band)."""
import ctypes as C
import itertools
import os
import subprocess
import tempfile

import numpy as np
import pytest

from grok_amd.capi import CODED_DTYPE, SEGMENT_DTYPE, TileParams

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OK, UNSUPPORTED, INVALID = 0, -2, -3
_lib = None


def lib():
    global _lib
    if _lib is None:
        csrc = os.path.join(ROOT, "grok_amd", "csrc")
        out = os.path.join(tempfile.mkdtemp(prefix="decode_plan_units_"), "libdecode_plan_units.so")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-D_GLIBCXX_ASSERTIONS", "-fPIC", "-shared",
                               os.path.join(HERE, "c", "decode_plan_units.cpp"), os.path.join(csrc, "decode_plan.cpp"),
                               os.path.join(csrc, "geometry.cpp"), "-o", out, "-Wl,--no-undefined", "-lpthread"])
        _lib = C.CDLL(out)
        _lib.dp_reason.restype = C.c_char_p
        _lib.dp_region.restype = C.c_int64
        _lib.dp_ipk_strip_cols.restype = C.c_uint32
    return _lib


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def constants():
    out = np.zeros(5, np.uint32)
    lib().dp_constants(ptr(out))
    return dict(zip(("skip", "noblock", "max_planes", "min_rows", "work_bytes"), (int(v) for v in out)))


def rows(specs):
    """[(length, passes, planes)] -> table rows laid end to end in the coded buffer (missing_msbs = planes | passes << 8)"""
    t = np.zeros(len(specs), CODED_DTYPE)
    at = 0
    for i, (length, passes, planes) in enumerate(specs):
        t[i] = (at, length, planes | passes << 8)
        at += length
    return t


# ---- the Part-1 launch lists --------------------------------------------------------------------------------------------------

def t1_lists(table, heights=None, lanes=2, sync=True, cblksty=0, segments=False):
    """-> (lane list, tail list, buckets); heights: per block (one tile), default 64"""
    n = len(table)
    h = np.full(n, 64, np.uint16) if heights is None else np.asarray(heights, np.uint16)
    lane, tail, out = np.zeros(2 * n, np.uint32), np.zeros(n, np.uint32), np.zeros(3, np.uint32)
    rc = lib().dp_t1_lists(ptr(table), C.c_uint64(n), ptr(h), n, cblksty, lanes, int(sync), int(segments), ptr(lane), ptr(tail), ptr(out))
    assert rc == OK, lib().dp_reason()
    return [int(v) for v in lane[:out[0]]], [int(v) for v in tail[:out[1]]], int(out[2])


def check_lists(table, lane, tail):
    """what holds for every pair of lists: a partition of the rows, whole waves of one (passes, planes) key, longest first"""
    no = constants()["noblock"]
    assert len(lane) % 64 == 0 and len(lane) > 0
    used = [i for i in lane if i != no] + tail
    assert sorted(used) == list(range(len(table))), "every block exactly once in lane + tail"
    for w in range(0, len(lane), 64):
        wave = [i for i in lane[w:w + 64] if i != no]
        assert wave, "no wave of spare lanes only"
        assert len({int(table["missing_msbs"][i]) for i in wave}) == 1, "a wave's blocks share passes and planes"
    groups = {}
    for i in lane:
        if i != no:
            groups.setdefault(int(table["missing_msbs"][i]), []).append(int(table["length"][i]) >> 2)     # (the sort's 4-byte buckets)
    for lens in groups.values():
        assert lens == sorted(lens, reverse=True), "lengths do not increase within a group"


def short_lengths(n, seed):
    return [int(v) for v in np.random.default_rng(seed).integers(8, 65, n)]      # (<= 64 bytes: none above the length threshold)


def test_t1_one_full_wave():
    table = rows([(ln, 4, 2) for ln in short_lengths(64, 1)])
    lane, tail, _ = t1_lists(table)
    assert len(lane) == 64 and constants()["noblock"] not in lane and tail == []
    check_lists(table, lane, tail)


def test_t1_one_block_short_of_a_wave():
    lane, tail, buckets = t1_lists(rows([(ln, 4, 2) for ln in short_lengths(63, 2)]))
    assert lane == [] and tail == [] and buckets > 0             # K8 in table order (the lists were tried)


def test_t1_groups_of_70_and_60():
    specs = [(ln, 4, 2) for ln in short_lengths(70, 3)] + [(ln, 7, 3) for ln in short_lengths(60, 4)]
    order = np.random.default_rng(5).permutation(len(specs))
    table = rows([specs[i] for i in order])
    lane, tail, _ = t1_lists(table)
    check_lists(table, lane, tail)
    assert len(lane) == 128 and lane.count(constants()["noblock"]) == 58
    assert len(tail) == 60 and {int(table["missing_msbs"][i]) for i in tail} == {3 | 7 << 8}


def test_t1_ineligible_rows_go_to_the_tail():
    k = constants()
    good = [(ln, 4, 2) for ln in short_lengths(128, 6)]
    bad = {"no data": (0, 4, 2), "no passes": (40, 0, 2), "no planes": (40, 4, 0),
           "too many planes": (40, 4, k["max_planes"] + 1), "more passes than the planes have": (40, 8, 3),
           "the longest": (1000, 4, 2), "above a quarter of the longest": (300, 4, 2), "few rows": (40, 4, 2), "skipped": (0, 0, 0)}
    names = sorted(bad)
    table = rows(good + [bad[n] for n in names])
    at = {n: len(good) + i for i, n in enumerate(names)}
    table[at["skipped"]] = (0, 0, k["skip"])
    heights = np.full(len(table), 64, np.uint16)
    heights[at["few rows"]] = k["min_rows"] - 1
    lane, tail, _ = t1_lists(table, heights)
    check_lists(table, lane, tail)
    for n in names:
        assert at[n] in tail, n
    assert sorted(tail) == sorted(at.values()) and len(lane) == 128
    # (above, a bad row's key has no 63 others and would go to the tail for that alone.)  Free-running lanes, no grouping by key:
    # nothing but the row's own eligibility keeps it from the lane list
    lane, tail, _ = t1_lists(table, heights, sync=False)
    assert sorted(tail) == sorted(at.values()) and sorted(lane) == list(range(128))
    # ... and pass-synchronous with 64 rows of each bad kind: a wave's worth, were the rows taken
    crowd = rows(good + [bad[n] for n in names for _ in range(64)])
    crowd["missing_msbs"][[128 + 64 * names.index("skipped") + i for i in range(64)]] = k["skip"]
    heights = np.full(len(crowd), 64, np.uint16)
    heights[128 + 64 * names.index("few rows"):][:64] = k["min_rows"] - 1
    lane, tail, _ = t1_lists(crowd, heights)
    check_lists(crowd, lane, tail)
    assert sorted(lane) == list(range(128)) and len(tail) == 64 * len(names)
    # and each limit from its other side: the lane decoder takes these
    edge = rows(good + [(250, 4, 2), (40, 4, k["max_planes"]), (40, 7, 3), (1000, 4, 2)])
    heights = np.full(len(edge), 64, np.uint16)
    heights[len(good) + 1] = k["min_rows"]
    lane, tail, _ = t1_lists(edge, heights, sync=False)          # (free-running lanes: no grouping by key)
    assert tail == [len(edge) - 1] and len(lane) == 131


def test_t1_hostile_length_costs_no_large_table():
    claimed = 0x30000000
    table = rows([(ln, 4, 2) for ln in short_lengths(128, 7)] + [(claimed, 4, 2)])
    assert lib().dp_check_table(ptr(table), C.c_uint64(len(table)), C.c_uint64(0x40000000)) == OK
    lane, tail, buckets = t1_lists(table)
    check_lists(table, lane, tail)
    assert tail == [128]
    assert buckets == (64 << 10) // 4 + 3                        # the clamp's table: lengths up to 64 KiB in 4-byte buckets


def test_t1_cost_model_regimes():
    """t1_lanes = 1: one long block (K8's in any case) and N short ones of one key.  The lists stand when 0.9 ns x all bytes
    > 2.5 ns x the longest block; the cases lie 5 % and more to either side of that line."""
    def lists(short_len, n, lanes=1):
        table = rows([(1600, 4, 2)] + [(short_len, 4, 2)] * n)
        lane, tail, _ = t1_lists(table, lanes=lanes)
        if lane:
            check_lists(table, lane, tail)
        return len(lane), tail
    # 64 short blocks of 40 bytes: 0.9 x 4160 = 3744 < 2.5 x 1600 = 4000 -> K8 alone, in the time of the long block
    assert lists(40, 64) == (0, [])
    assert lists(40, 64, lanes=2) == (64, [0])                  # (the lists that were set aside)
    # ... of 48 bytes: 0.9 x 4672 = 4205 > 4000 -> the lanes take them
    assert lists(48, 64) == (64, [0])
    # the same blocks, more of them: 80 x 40 bytes -> 0.9 x 4800 = 4320 > 4000 stays with the lanes, 60 cannot fill a wave
    assert lists(40, 80) == (128, [0])
    assert lists(40, 60) == (0, [])
    # a large call: K8's throughput is the bound by far
    assert lists(40, 20000) == (20032, [0])
    # equal lengths throughout: the lanes at either size
    assert len(t1_lists(rows([(40, 4, 2)] * 64), lanes=1)[0]) == 64
    assert len(t1_lists(rows([(40, 4, 2)] * 20000), lanes=1)[0]) == 20032


@pytest.mark.parametrize("how", [dict(lanes=0), dict(cblksty=1), dict(cblksty=0x20), dict(segments=True)], ids=str)
def test_t1_no_lane_list(how):
    assert t1_lists(rows([(40, 4, 2)] * 256), **how) == ([], [], 0)


# ---- table checks, the HT launch list -----------------------------------------------------------------------------------------

def ht_blocks(table, coded_bytes):
    active, out = np.zeros(len(table), np.uint32), np.zeros(2, np.uint32)
    rc = lib().dp_ht_blocks(ptr(table), C.c_uint64(len(table)), C.c_uint64(coded_bytes), ptr(active), ptr(out))
    return rc, [int(v) for v in active[:out[0]]], int(out[1])


def test_table_rows_outside_the_coded_buffer():
    table = rows([(100, 1, 1)] * 8)
    total = 800
    for bad in ((total + 1, 0, 0), (total - 50, 51, 0), (2 ** 63, 1, 0)):
        t = table.copy()
        t[5] = bad
        assert lib().dp_check_table(ptr(t), C.c_uint64(8), C.c_uint64(total)) == INVALID
        assert lib().dp_reason() == b"block table row points outside the coded buffer"
        assert ht_blocks(t, total)[0] == INVALID
        assert lib().dp_reason() == b"block table row points outside the coded buffer"
    t = table.copy()
    t[5] = (total, 0, 0)                                        # (an empty row at the very end is inside)
    t[6] = (total - 50, 50, 0)
    assert lib().dp_check_table(ptr(t), C.c_uint64(8), C.c_uint64(total)) == OK
    assert lib().dp_check_table(ptr(table), C.c_uint64(8), C.c_uint64(total - 1)) == INVALID


def test_ht_blocks_longer_than_48k_are_unsupported():
    table = rows([(100, 0, 3), ((48 << 10) + 1, 0, 3)])
    assert ht_blocks(table, 1 << 20)[0] == UNSUPPORTED and lib().dp_reason() == b"code-block longer than 48 KiB"
    table = rows([(100, 0, 3), (48 << 10, 0, 3)])
    assert ht_blocks(table, 1 << 20) == (OK, [0, 1], 48 << 10)


def test_ht_active_list_is_the_rows_with_data():
    lengths = [int(v) for v in np.random.default_rng(8).integers(0, 3, 300) * 17]
    table = rows([(ln, 0, 2) for ln in lengths])
    total = sum(lengths)
    table[11] = (0, 0, constants()["skip"])
    lengths[11] = 0
    rc, active, longest = ht_blocks(table, total)
    assert rc == OK and longest == 34
    assert active == [i for i, ln in enumerate(lengths) if ln]


# ---- the HT refinement table --------------------------------------------------------------------------------------------------

def refinement(table, per_block):
    """per_block = [[(length, passes), ...], ...] -> (rc, [(bytes, passes)], largest refinement segment)"""
    first = np.cumsum([0] + [len(s) for s in per_block]).astype(np.uint32)
    segs = np.array([s for blk in per_block for s in blk] or [(0, 0)], SEGMENT_DTYPE)
    ref, longest = np.zeros(len(table), SEGMENT_DTYPE), np.zeros(1, np.uint32)
    rc = lib().dp_ht_refinement(ptr(table), C.c_uint64(len(table)), ptr(first), C.c_uint64(len(first)), ptr(segs),
                                C.c_uint64(int(first[-1])), ptr(ref), ptr(longest))
    return rc, [(int(r["length"]), int(r["numpasses"])) for r in ref], int(longest[0])


def test_ht_refinement_table():
    table = rows([(100, 0, 2), (0, 0, 2), (250, 0, 2), (90, 0, 2), (70, 0, 2), (60, 0, 2), (30000, 0, 2)])
    segs = [[(100, 1)], [], [(200, 1), (50, 1)], [(60, 1), (30, 2)], [(50, 1), (20, 5)], [(60, 1), (0, 2)], [(30000 - (16 << 10), 1), (16 << 10, 2)]]
    rc, ref, longest = refinement(table, segs)
    assert rc == OK and longest == 16 << 10
    assert ref == [(0, 1), (0, 1), (50, 2), (30, 3), (20, 3), (0, 1), (16 << 10, 3)]


def test_ht_refinement_refusals():
    table = rows([(100, 0, 2), (250, 0, 2), (30000, 0, 2)])
    fine = [[(100, 1)], [(200, 1), (50, 1)], [(30000, 1)]]
    assert refinement(table, fine)[0] == OK
    assert refinement(table, [[(50, 1), (25, 1), (25, 1)]] + fine[1:])[0] == INVALID
    assert lib().dp_reason() == b"an HT code-block has at most two codeword segments"
    assert refinement(table, [fine[0], [(200, 1), (49, 1)], fine[2]])[0] == INVALID
    assert lib().dp_reason() == b"segment lengths do not add up to the block's length"
    assert refinement(table, fine[:2] + [[(30000 - (16 << 10) - 1, 1), ((16 << 10) + 1, 2)]])[0] == UNSUPPORTED
    assert lib().dp_reason() == b"refinement segment longer than 16 KiB"
    assert refinement(table, fine[:2])[0] == INVALID                         # a list for two of the three blocks
    assert lib().dp_reason() == b"segment list does not match the number of blocks"


# ---- region planning ------------------------------------------------------------------------------------------------------------

TILES = {"37x29 at (5, 3), 5/3": TileParams.make(37, 29, 3, 8, 3, cblk=(3, 3), origin=(5, 3)),
         "37x29 at (5, 3), 9/7": TileParams.make(37, 29, 3, 8, 3, irreversible=True, cblk=(3, 3), origin=(5, 3)),
         "64x64, 5/3": TileParams.make(64, 64, 1, 8, 3, cblk=(4, 4)),
         "64x64, 9/7": TileParams.make(64, 64, 1, 8, 3, irreversible=True, cblk=(4, 4))}


def region(p, win):
    """-> (levels[L + 1][12], skipped row indices, resolution of every row)"""
    L = p.num_levels
    levels, table, res = np.zeros((L + 1, 12), np.uint32), np.zeros(4096, CODED_DTYPE), np.zeros(4096, np.uint8)
    table["length"], table["offset"], table["missing_msbs"] = 1, 7, 3
    n = lib().dp_region(C.byref(p), ptr(np.array(win, np.uint32)), ptr(levels), ptr(table), ptr(res), C.c_uint64(len(table)))
    assert n > 0, n
    skip = constants()["skip"]
    skipped = [i for i in range(n) if int(table["missing_msbs"][i]) == skip]
    for i in range(n):                  # a row is either untouched or {0, 0, kSkipBlock}
        assert tuple(table[i]) == ((0, 0, skip) if i in skipped else (7, 1, 3))
    assert tuple(table[n]) == (7, 1, 3)
    return levels, skipped, [int(v) for v in res[:n]]


@pytest.mark.parametrize("name", sorted(TILES))
def test_region_plan(name):
    p = TILES[name]
    W, H, L = p.tile_w, p.tile_h, p.num_levels
    nested = [(0, 0, W, H), (8, 6, 30, 20), (10, 8, 20, 15), (12, 9, 13, 10)]
    corners = [(0, 0, 1, 1), (W - 1, 0, W, 1), (0, H - 1, 1, H), (W - 1, H - 1, W, H)]
    counts = []
    for win in nested + corners:
        levels, skipped, res = region(p, win)
        for l in range(L + 1):
            x0, y0, x1, y1, w, h = (int(v) for v in levels[l][:6])
            assert x0 < x1 <= w and y0 < y1 <= h, "need[%d] of %s" % (l, win)
            if l < L:
                x0, y0, x1, y1, w, h = (int(v) for v in levels[l][6:])
                assert x0 < x1 <= w and y0 < y1 <= h, "pairs[%d] of %s" % (l, win)
        assert tuple(int(v) for v in levels[0][:4]) == win
        if win in nested:
            counts.append(len(skipped))
        elif W == 64:
            assert any(res[i] == L for i in skipped), "corner %s keeps every block of the top resolution" % (win,)
    assert counts[0] == 0, "the whole tile skips nothing"
    assert counts == sorted(counts), "a window inside another never skips fewer blocks"
    assert counts[-1] > 0


# ---- the reduced decode's segment list ----------------------------------------------------------------------------------------

def reduce_segments(groups, full, kept, counts, nfirst=None):
    first = np.cumsum([0] + counts).astype(np.uint32)
    segs = np.array([(100 + i, i % 3 + 1) for i in range(int(first[-1]))], SEGMENT_DTYPE)
    red_first, red_segs, out = np.zeros(64, np.uint32), np.zeros(64, SEGMENT_DTYPE), np.zeros(2, np.uint64)
    rc = lib().dp_reduce_segments(C.c_uint64(groups), full, kept, ptr(first), C.c_uint64(len(first) if nfirst is None else nfirst),
                                  ptr(segs), C.c_uint64(len(segs)), ptr(red_first), C.c_uint64(64), ptr(red_segs), C.c_uint64(64), ptr(out))
    return rc, [int(v) for v in red_first[:int(out[0])]], [(int(s["length"]), int(s["numpasses"])) for s in red_segs[:int(out[1])]]


def test_reduced_segment_list():
    # two components of 7 blocks, the first 3 of each kept; segments per block:
    counts = [1, 2, 0, 1, 1, 3, 1,
              2, 1, 1, 0, 0, 1, 2]
    rc, first, segs = reduce_segments(2, 7, 3, counts)
    assert rc == OK
    assert first == [0, 1, 3, 3, 5, 6, 7]
    assert segs == [(100, 1), (101, 2), (102, 3), (109, 1), (110, 2), (111, 3), (112, 1)]
    assert reduce_segments(2, 7, 3, counts[:-1])[0] == INVALID               # a list over 13 blocks
    assert lib().dp_reason() == b"segment list does not match the number of blocks"
    assert reduce_segments(2, 7, 3, counts + [1])[0] == INVALID
    assert reduce_segments(2, 7, 3, counts, nfirst=14)[0] == INVALID         # the index cut short: its last entry is not the segment count


# ---- the shape of an inverse DWT level ----------------------------------------------------------------------------------------

HEAD = ("packed", "strip_pairs", "seg_pairs", "grid_x", "grid_y", "strip0", "nstrips", "seg0", "nsegs", "wx0", "wy0", "wx1", "wy1")


def idwt(cw, ch, px=0, py=0, ll_stride=None, m_stride=None, out_stride=None, h16=True, pk=True, irreversible=False, zslots=1, need=None,
         fused=False, px_bytes=1, lo=0, hi=255, mct=False, px_lay=0, px_chan=0, px_row=0, px_tile=0, px_align=0):
    """-> the shape's head as a dict; "inst": the instances of the part of one component and of the MCT triple, each
    (("pk", NC, PXO, CH) or ("k", F97, NC, PXO, H16, STR), grid_x)"""
    out = np.zeros(33, np.uint32)
    stride = (cw + 31) & ~31
    strides = [stride if v is None else v for v in (ll_stride, m_stride, out_stride)]
    lib().dp_idwt_level(ptr(np.array([cw, ch, px, py] + strides + [h16, pk, irreversible, zslots, need is not None] + list(need or (0, 0, 0, 0)) +
                                     [fused, px_bytes, lo, hi, mct, px_lay, px_chan, px_row, px_tile, px_align], np.int64)), ptr(out))
    got = dict(zip(HEAD, (int(v) for v in out[:13])))
    got["inst"] = []
    for i in range(2):
        row = [int(v) for v in out[13 + 10 * i:23 + 10 * i]]
        got["inst"].append((("pk",) + tuple(row[7:10]) if row[0] else ("k",) + tuple(row[2:7]), row[1]))
    return got


def head(got):
    return {k: got[k] for k in HEAD}


def idwt_tables():
    out = np.zeros(5 * 64, np.uint32)
    n = lib().dp_idwt_instances(ptr(out))
    k = [("k",) + tuple(int(v) for v in out[5 * i:5 * i + 5]) for i in range(n)]
    n = lib().dp_idwt_pk_instances(ptr(out))
    pk = [("pk",) + tuple(int(v) for v in out[3 * i:3 * i + 3]) for i in range(n)]
    n = lib().dp_egress_instances(ptr(out))
    return k, pk, [tuple(int(v) for v in out[3 * i:3 * i + 3]) for i in range(n)]


def segment_pairs(strips, row_pairs, zslots):
    """row_segment_pairs at the inverse transform's floor of 4096 workgroups"""
    fits = [seg for seg in (64, 32, 16, 8) if strips * ((row_pairs + seg - 1) // seg) * zslots >= 4096]
    return fits[0] if fits else 8


def test_idwt_constants():
    out = np.zeros(5, np.uint32)
    lib().dp_idwt_constants(ptr(out))
    assert [int(v) for v in out] == [224, 2, 960, 4096, 16]


def test_idwt_packed_condition():
    """every clause of the packed condition on its own"""
    assert idwt(256, 16)["packed"] and idwt(256, 16)["inst"][0] == (("pk", 1, 0, 0), 1)
    for kw in (dict(cw=252), dict(ch=14), dict(ch=17), dict(cw=258), dict(px=1), dict(py=1), dict(irreversible=True), dict(pk=False),
               dict(h16=False), dict(need=(0, 0, 256, 16)), dict(m_stride=1 << 27), dict(out_stride=1 << 27)):
        args = dict(cw=256, ch=16)
        args.update(kw)
        got = idwt(**args)
        assert not got["packed"] and got["strip_pairs"] == 224 and got["inst"][0][0][0] == "k", kw
    assert idwt(256, 16, m_stride=(1 << 27) - 32)["packed"], "one row short of 2^31"
    assert idwt(256, 16, ll_stride=1 << 27)["packed"], "the LL is read through flat addresses"


def test_idwt_strips():
    """256: one strip of 256 columns.  960: one of 960.  964: two of 512 (482 -> 512).  1920: two of 960.  961 is no multiple of 4:
    the 32-bit kernel, 481 pairs in three strips of 224."""
    assert [lib().dp_ipk_strip_cols(cw) for cw in (256, 960, 961, 964, 1920)] == [256, 960, 512, 512, 960]
    for cw, strip_pairs, grid_x in ((256, 128, 1), (960, 480, 1), (964, 256, 2), (1920, 480, 2)):
        got = idwt(cw, 64)
        assert got["packed"] and (got["strip_pairs"], got["grid_x"]) == (strip_pairs, grid_x), cw
        assert got["inst"][0] == (("pk", 1, 0, 0), grid_x)
    got = idwt(961, 64)
    assert (got["packed"], got["strip_pairs"], got["grid_x"]) == (0, 224, 3)
    assert idwt(448, 64, pk=False)["grid_x"] == 1 and idwt(448, 64, pk=False, px=1)["grid_x"] == 2, "an odd start's phantom column counts"
    for cw, ch, z, pk in itertools.product((256, 448, 964, 4096, 8192), (16, 100, 1024, 8192), (1, 3, 48), (True, False)):
        got = idwt(cw, ch, pk=pk, zslots=z)
        strips = -(-(cw // 2) // got["strip_pairs"])
        assert got["seg_pairs"] == segment_pairs(strips, (ch + 1) // 2, z)
        assert got["grid_y"] == -(-((ch + 1) // 2) // got["seg_pairs"])
        assert got["grid_x"] == strips
    assert idwt(64, 17, py=1, pk=False)["grid_y"] == 2 and idwt(64, 15, py=1, pk=False)["grid_y"] == 1


def test_idwt_fused_extras():
    """what the fused last level asks beyond the packed condition: each flips the instance and nothing else of the shape"""
    base = dict(cw=256, ch=16, fused=True)
    want = idwt(**base)
    assert want["packed"] and want["inst"][0] == (("pk", 1, 1, 0), 1)

    def flipped(inst, part=0, **kw):
        args = dict(base)
        args.update(kw)
        got = idwt(**args)
        ref = idwt(**dict(base, **{k: v for k, v in kw.items() if k in ("mct", "px_lay", "px_chan", "px_row", "px_tile")}))
        assert head(got) == head(ref) == head(want), kw
        assert got["inst"][part] == (inst, 1), kw
    flipped(("k", 0, 1, 2, 1, 0), px_bytes=2)
    flipped(("k", 0, 1, 1, 1, 0), lo=-128, hi=127)                  # signed
    flipped(("k", 0, 1, 1, 1, 0), hi=127)                           # precision 7
    flipped(("k", 0, 1, 1, 1, 0), lo=1)
    flipped(("k", 0, 3, 1, 1, 0), part=1)                           # three components side by side without a colour transform
    flipped(("pk", 3, 1, 0), part=1, mct=True)
    # a layout of the caller's: interleaved pixels of 1, 3, 4 samples
    lay1 = dict(px_lay=2, px_chan=1, px_row=256, px_tile=4096)
    flipped(("pk", 1, 1, 1), **lay1)
    for kw in (dict(px_align=1), dict(px_align=2), dict(px_row=257), dict(px_tile=4098), dict(px_row=1 << 27), dict(px_lay=1), dict(hi=127),
               dict(px_bytes=2)):
        flipped(("k", 0, 1, 2 if "px_bytes" in kw else 1, 1, 1), **dict(lay1, **kw))
    for chan, inst3, inst1 in ((1, ("k", 0, 3, 1, 1, 1), ("pk", 1, 1, 1)), (2, ("k", 0, 3, 1, 1, 1), ("k", 0, 1, 1, 1, 1)),
                               (3, ("pk", 3, 1, 3), ("k", 0, 1, 1, 1, 1)), (4, ("pk", 3, 1, 4), ("k", 0, 1, 1, 1, 1))):
        lay = dict(px_lay=2, px_chan=chan, px_row=256 * chan, px_tile=4096 * chan, mct=True)
        flipped(inst3, part=1, **lay)
        flipped(inst1, part=0, **lay)
        flipped(("k", 0, 3, 1, 1, 1), part=1, **dict(lay, mct=False))
    # a window: a region decode never runs packed (the condition's own clause), and the pixels are the window's
    got = idwt(256, 16, fused=True, need=(3, 2, 200, 9))
    assert not got["packed"] and got["inst"][0][0] == ("k", 0, 1, 1, 1, 0)
    assert (got["wx0"], got["wy0"], got["wx1"], got["wy1"]) == (3, 2, 200, 9)
    got = idwt(256, 16, fused=False, need=(3, 2, 200, 9))
    assert (got["wx0"], got["wy0"], got["wx1"], got["wy1"]) == (0, 0, 256, 16), "only the level that writes pixels has a window"


@pytest.mark.parametrize("name,kw", [("signed 8-bit", dict(lo=-128, hi=127)), ("precision 7", dict(hi=127)),
                                     ("two-channel layout", dict(px_lay=2, px_chan=2, px_row=2 * 8192, px_tile=2 * 8192 * 8192, mct=False, zslots=2)),
                                     ("odd pointer", dict(px_lay=2, px_chan=3, px_row=3 * 8192, px_tile=3 * 8192 * 8192, px_align=1))])
def test_idwt_row_segments_follow_the_packed_strips(name, kw):
    """KNOWN MISMATCH, reproduced on purpose: the row segments of the fused level are sized from the packed kernel's strips whenever the
    packed condition holds, also where the level then runs the 32-bit kernel on strips of 224 pairs.  8192 x 8192: packed strips of
    960 columns = 480 pairs -> 9 strips; one z slot: 9 x (4096 / 16) = 2304 < 4096 workgroups -> 8 row pairs per workgroup.  The 32-bit
    kernel's own 19 strips reach 19 x 256 = 4864 at 16.  (Two z slots: 16 against 32.)"""
    args = dict(cw=8192, ch=8192, fused=True, mct=True, zslots=1)
    args.update(kw)
    got = idwt(**args)
    part = 1 if args["mct"] else 0
    assert got["packed"] and got["strip_pairs"] == 480
    assert got["inst"][part][0][0] == "k" and got["inst"][part][1] == 19, "the 32-bit kernel on its own strips"
    assert got["seg_pairs"] == segment_pairs(9, 4096, args["zslots"]) == (8 if args["zslots"] == 1 else 16)
    assert segment_pairs(19, 4096, args["zslots"]) == 2 * got["seg_pairs"], "what its own strips would give"
    assert got["grid_y"] == 4096 // got["seg_pairs"]
    packed = idwt(**dict(args, lo=0, hi=255, px_lay=0, px_align=0, mct=True, zslots=1))
    assert packed["inst"][1] == (("pk", 3, 1, 0), 9) and packed["seg_pairs"] == 8


def test_idwt_region_subgrid():
    """windows at the tile's corners and across a strip / row segment boundary: strips of 224 pairs, segments of 16, counted on the
    coordinate grid (sample k of the level = coordinate k + parity)"""
    W, H = 1000, 600
    for (px, py), need in itertools.product(((0, 0), (1, 0), (0, 1), (1, 1)),
                                           ((0, 0, 1, 1), (W - 1, 0, W, 1), (0, H - 1, 1, H), (W - 1, H - 1, W, H), (0, 0, W, H),
                                            (440, 20, 460, 40), (447, 31, 448, 32), (447, 31, 449, 33), (448, 32, 449, 33))):
        x0, y0, x1, y1 = need
        for fused in (False, True):
            got = idwt(W, H, px=px, py=py, need=need, fused=fused, zslots=3)
            strip0, seg0 = ((x0 + px) // 2) // 224, ((y0 + py) // 2) // 16
            nstrips, nsegs = ((x1 - 1 + px) // 2) // 224 - strip0 + 1, ((y1 - 1 + py) // 2) // 16 - seg0 + 1
            assert (got["strip0"], got["nstrips"], got["seg0"], got["nsegs"]) == (strip0, nstrips, seg0, nsegs), (px, py, need)
            assert (got["seg_pairs"], got["grid_x"], got["grid_y"]) == (16, nstrips, nsegs)
            assert got["inst"][0][1] == nstrips and (not fused or got["inst"][1][1] == nstrips)
            assert (got["wx0"], got["wy0"], got["wx1"], got["wy1"]) == (need if fused else (0, 0, W, H))
    # the boundary cases by hand, on the origin: column 447 is pair 223 = strip 0, column 448 pair 224 = strip 1; row 31 pair 15, row 32 pair 16
    assert [idwt(W, H, need=n)[k] for n in ((447, 31, 448, 32), (447, 31, 449, 33), (448, 32, 449, 33))
            for k in ("strip0", "nstrips", "seg0", "nsegs")] == [0, 1, 0, 1, 0, 2, 0, 2, 1, 1, 1, 1]


# ---- kernel instances ---------------------------------------------------------------------------------------------------------

def old_is_pk(cw, ch, px, py, m_stride, out_stride, h16, pk, irreversible, region):
    """idwt_level_is_pk as it stood in kernels_idwt.hip (run_idwt cleared a.pk for a region, the launcher saw the sub-grid)"""
    near = m_stride * ch < 1 << 31 and out_stride * ch < 1 << 31
    return bool(h16 and pk and not irreversible and (px | py) == 0 and (cw & 3) == 0 and cw >= 256 and ch >= 16 and (ch & 1) == 0 and
                not region and near)


def old_inverse_ladder(fused, nc, is_pk, whole, ch, irreversible, h16, px_bytes, lo, hi, mct, px_lay, px_chan, px_row, px_tile, px_align):
    """the nested ifs of launch_idwt_level / launch_idwt_level0_fused as they stood before the lists (dwt_instances.h), rung by rung"""
    def k(f97, nc, pxo, h16=0, str_=0):
        return ("k", f97, nc, pxo, 1 if h16 else 0, str_)
    if not fused:
        if is_pk:
            return ("pk", 1, 0, 0)
        if irreversible:
            return k(1, 1, 0)
        return k(0, 1, 0, 1) if h16 else k(0, 1, 0)
    px = 1 if px_bytes == 1 else 2
    if irreversible and px_lay != 0:
        return k(1, nc, px, 0, 1)
    if irreversible:
        return k(1, nc, px)
    if px_lay != 0:
        al = ((px_align | px_row | px_tile) & 3) == 0 and px_row * ch < 1 << 31
        shape = px_lay == 2 and ((px_chan == 1 and nc == 1) or (px_chan in (3, 4) and nc == 3 and mct))
        if px == 1 and is_pk and lo == 0 and hi == 255 and whole and al and shape:
            return ("pk", 1, 1, 1) if px_chan == 1 else ("pk", 3, 1, 3) if px_chan == 3 else ("pk", 3, 1, 4)
        return k(0, nc, px, h16, 1)
    if px == 1 and is_pk and lo == 0 and hi == 255 and whole and (nc == 1 or mct):
        return ("pk", 3, 1, 0) if nc == 3 else ("pk", 1, 1, 0)
    return k(0, nc, px, h16, 0)


def test_idwt_instance_tables_against_the_old_ladder():
    """Over the descriptor's discrete fields: the planner's key is what the old ladder picked, it is in its kernel's list, its strips are
    that kernel's, and every row of both lists is picked at least once."""
    k_rows, pk_rows, _ = idwt_tables()
    assert len(k_rows) == len(set(k_rows)) == 27 and len(pk_rows) == len(set(pk_rows)) == 6
    seen = set()
    plain = [dict(fused=False)]
    fused = [dict(fused=True, px_bytes=b, lo=lo, hi=hi, mct=mct, px_lay=lay, px_chan=chan, px_row=row * chan * b, px_tile=4096 * chan * b,
                  px_align=al)
             for b, (lo, hi), mct, (lay, chan), row, al in itertools.product(
                 (1, 2), ((0, 255), (-128, 127), (0, 127)), (False, True), ((0, 0), (1, 1), (2, 1), (2, 2), (2, 3), (2, 4)), (256, 257), (0, 1))
             if lay or (row, al) == (256, 0)]
    for (cw, ch), irreversible, h16, pk, need, extra in itertools.product(
            ((256, 16), (34, 18), (33, 17)), (False, True), (False, True), (False, True), (None, "whole", "part"), plain + fused):
        need = {None: None, "whole": (0, 0, cw, ch), "part": (1, 1, cw - 1, ch - 1)}[need]
        kw = dict(h16=h16, pk=pk and need is None, irreversible=irreversible, need=need, **extra)
        got = idwt(cw, ch, **kw)
        stride = (cw + 31) & ~31
        is_pk = old_is_pk(cw, ch, 0, 0, stride, stride, h16, kw["pk"], irreversible, need is not None)
        assert bool(got["packed"]) == is_pk
        whole = need is None or need == (0, 0, cw, ch)
        for nc in (1, 3) if extra["fused"] else (1,):
            inst, grid_x = got["inst"][nc == 3]
            e = dict(dict(px_bytes=0, lo=0, hi=0, mct=False, px_lay=0, px_chan=0, px_row=0, px_tile=0, px_align=0), **extra)
            want = old_inverse_ladder(e["fused"], nc, is_pk, whole, ch, irreversible, h16, e["px_bytes"], e["lo"], e["hi"], e["mct"],
                                      e["px_lay"], e["px_chan"], e["px_row"], e["px_tile"], e["px_align"])
            assert inst == want, (cw, ch, nc, kw)
            assert inst in (pk_rows if inst[0] == "pk" else k_rows), (cw, ch, nc, kw)
            if inst[0] == "pk":
                assert grid_x == -(-cw // lib().dp_ipk_strip_cols(cw))
            else:
                assert grid_x == (got["nstrips"] if need else -(-((cw + 1) // 2) // 224))
            seen.add(inst)
    assert seen == set(k_rows) | set(pk_rows), "rows no descriptor selects: %s" % sorted((set(k_rows) | set(pk_rows)) - seen)
    # a level between planes has one part: the triple's slot holds a key that is in no list (the launcher refuses it)
    inst, _ = idwt(256, 16)["inst"][1]
    assert inst not in k_rows and inst not in pk_rows


def test_egress_instances_against_the_old_ladder():
    """launch_egress's macro as it stood: a layout of the caller's for 8- / 16-bit pixels, else by size, int32 in the default layout; one
    to four components"""
    _, _, rows = idwt_tables()
    assert len(rows) == len(set(rows)) == 20
    seen = set()
    for px_lay, b, ncomp in itertools.product((0, 1, 2), (1, 2, 4), (1, 2, 3, 4)):
        out = np.zeros(3, np.uint32)
        lib().dp_egress_key(px_lay, b, ncomp, ptr(out))
        got = tuple(int(v) for v in out)
        want = (1, ncomp, 1) if px_lay and b == 1 else (2, ncomp, 1) if px_lay and b == 2 else (1, ncomp, 0) if b == 1 else (2, ncomp, 0) if b == 2 \
            else (4, ncomp, 0)
        assert got == want and got in rows
        seen.add(got)
    assert seen == set(rows)
    for ncomp in (0, 5):                   # (the geometry admits 1..4 components; anything else names no instance)
        out = np.zeros(3, np.uint32)
        lib().dp_egress_key(0, 1, ncomp, ptr(out))
        assert tuple(int(v) for v in out) not in rows
