"""CPU: what a rate-targeted encode of a sub-sampled image or a video surface needs from the host -- the sub-sampled Tier-2 writer
(grk_amd_write_codestream_subsampled, grok_amd/csrc/t2_writer.cpp) coding the zero-bit-plane tag trees from the rows' own
missing_msbs (GRK_AMD_CS_BLOCK_MSBS), read back by the library's reader and accepted by the reference's decoder where oracle/_ref is
present; the cases in which the flag changes no byte; and the planning of the joint tables (grok_amd/csrc/encode_plan.cpp:
plan_rate_joint) through tests/c/rate_joint_units.cpp -- as a library, and as a stand-alone program under AddressSanitizer and
UBSan."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import grok_amd as G
import oracle as O
import refharness as R
import synth
from grok_amd.capi import CODED_DTYPE

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
MSBS = G.CS_BLOCK_MSBS
needs_ref = pytest.mark.skipif(not R.have_ref(), reason="oracle/_ref (the real reference) not built here")

# the 4:2:0 image of the writer tests: 96 x 80 in tiles of 64 x 48 (2 x 2 tiles, ragged), 2 levels, no colour transform
W, H, TW, TH, LEVELS = 96, 80, 64, 48, 2
SAMPLING = [(1, 1), (2, 2), (2, 2)]


def _lib():
    L = G.lib()
    L.grk_amd_layout_tile_comp.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
    L.grk_amd_write_codestream_subsampled.restype = C.c_int64
    L.grk_amd_write_codestream_subsampled.argtypes = [C.c_void_p] * 6 + [C.c_uint32, C.c_void_p, C.c_uint64]
    return L


def image():
    return G.ImageLayout.make(W, H, TW, TH), G.TileParams.make(1, 1, len(SAMPLING), 8, LEVELS, mct=False)


def tile_comps(layout, base, sampling=SAMPLING):
    """the tile-components in the writer's order -- tile by tile, within a tile component by component -> [(tile, comp, params)]"""
    L = _lib()
    out = []
    for t in range(L.grk_amd_layout_num_tiles(C.byref(layout))):
        for c, (dx, dy) in enumerate(sampling):
            p = G.TileParams()
            assert L.grk_amd_layout_tile_comp(C.addressof(layout), C.addressof(base), dx, dy, t, C.addressof(p)) == 0
            p.num_comps = 1
            out.append((t, c, p))
    return out


def write_subsampled(layout, base, table, coded, flags, sampling=SAMPLING, size_only=False):
    L = _lib()
    dxs = (C.c_uint8 * len(sampling))(*[a for a, _ in sampling])
    dys = (C.c_uint8 * len(sampling))(*[b for _, b in sampling])
    table = np.ascontiguousarray(table)
    out = np.empty(int(table["length"].sum()) + len(table) * 16 + (1 << 16), np.uint8)
    n = L.grk_amd_write_codestream_subsampled(C.addressof(layout), C.addressof(base), C.addressof(dxs), C.addressof(dys), table.ctypes.data,
                                              None if size_only else coded.ctypes.data, flags, None if size_only else out.ctypes.data,
                                              0 if size_only else out.size)
    assert n > 0, n
    return int(n) if size_only else out[:n].tobytes()


def forged_table(layout, base, seed, constant=False):
    """rows made by hand for every tile-component: lengths 0 .. 299 (one in eight 0), bytes below 0x80 (no marker can appear),
    missing_msbs in [kmax - 1 - 6, kmax - 1] (kmax - 1 everywhere when constant) -> (table, coded, the rows' kmax - 1)"""
    rng = np.random.default_rng(seed)
    tabs, tops, off = [], [], 0
    for _, _, p in tile_comps(layout, base):
        blocks, _ = G.tile_layout(p)
        t = np.zeros(len(blocks), CODED_DTYPE)
        lens = np.where(rng.random(len(blocks)) < 0.125, 0, rng.integers(1, 300, len(blocks)))
        t["length"] = lens
        t["offset"] = off + np.concatenate([[0], np.cumsum(lens)[:-1]])
        top = np.array([b.kmax - 1 for b in blocks])
        t["missing_msbs"] = top if constant else np.maximum(top - rng.integers(0, 7, len(blocks)), 0)
        off += int(lens.sum())
        tabs.append(t)
        tops.append(top)
    return np.concatenate(tabs), rng.integers(0, 0x80, max(off, 1)).astype(np.uint8), np.concatenate(tops)


# ---- 1. the writer ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, G.CS_SOP | G.CS_EPH, G.CS_PLT | G.CS_TLM | G.CS_SOP | G.CS_EPH])
@pytest.mark.parametrize("order", range(5))
def test_forged_rows_of_a_420_image_read_back(order, flags):
    """rows with their own missing_msbs and lengths -> grk_amd_write_codestream_subsampled with GRK_AMD_CS_BLOCK_MSBS ->
    grk_amd_read_header / grk_amd_read_packets give the rows back: missing_msbs, lengths, the bytes at the offsets"""
    layout, base = image()
    table, coded, tops = forged_table(layout, base, [order, flags])
    assert (table["missing_msbs"] != tops).sum() * 2 > len(table) and (table["missing_msbs"] == tops).any()
    fl = flags | G.CS_PROG(order) | MSBS
    cs = write_subsampled(layout, base, table, coded, fl)
    assert write_subsampled(layout, base, table, None, fl, size_only=True) == len(cs)          # out == NULL: the length alone
    info = G.read_header(cs)
    out = G.read_packets(cs, info)
    assert len(out["rows"]) == len(table) == info.num_blocks and len(out["moves"]) == 0
    assert np.array_equal(out["rows"]["length"], table["length"])
    assert np.array_equal(out["rows"]["missing_msbs"], table["missing_msbs"])
    cb = np.frombuffer(cs, np.uint8)
    for i in range(len(table)):
        o, n, t = int(out["rows"][i]["offset"]), int(table[i]["length"]), int(table[i]["offset"])
        assert o + n <= len(cs) and np.array_equal(cb[o:o + n], coded[t:t + n]), i
    assert info.flags == fl & ~MSBS                           # (nothing in the headers says how the trees were made)
    # without the flag the column is not looked at: every row comes back at kmax - 1
    plain = G.read_packets(write_subsampled(layout, base, table, coded, fl & ~MSBS))
    assert np.array_equal(plain["rows"]["missing_msbs"], tops)


def test_constant_rows_give_the_same_bytes_with_and_without_the_flag():
    """every row at Kmax - 1: the bytes are those without the flag, for the five progression orders and SOP / EPH / PLT / TLM"""
    layout, base = image()
    table, coded, tops = forged_table(layout, base, 11, constant=True)
    other = table.copy()
    other["missing_msbs"] = np.random.default_rng(3).integers(0, 30, len(table))
    for order in range(5):
        for flags in (0, G.CS_SOP, G.CS_EPH, G.CS_PLT, G.CS_TLM, G.CS_SOP | G.CS_EPH | G.CS_PLT | G.CS_TLM):
            fl = flags | G.CS_PROG(order)
            plain = write_subsampled(layout, base, table, coded, fl)
            assert write_subsampled(layout, base, table, coded, fl | MSBS) == plain, (order, flags)
            assert write_subsampled(layout, base, other, coded, fl) == plain                 # (flag off: the column is ignored)
            assert write_subsampled(layout, base, other, coded, fl | MSBS) != plain


@needs_ref
@pytest.mark.parametrize("order", [0, 2, 4])
def test_reference_decoder_accepts_the_forged_headers(order):
    """The reference reads a 4:2:0 file whose packet headers carry per-block zero bit-planes.  The blocks are the oracle's (d = 0, so
    that their bytes are blocks a decoder takes); a random half of them is left out -- length 0 -- under forged zero bit-planes in
    [kmax - 1 - 6, kmax - 1]: the file decodes, and with nothing left out and every row at kmax - 1 it is lossless."""
    layout, base = image()
    planes = [synth.g2(1, (H + dy - 1) // dy, (W + dx - 1) // dx, 8, seed=50 + 3 * c)[0] for c, (dx, dy) in enumerate(SAMPLING)]
    rng = np.random.default_rng(order)
    tabs, chunks, off = [], [], 0
    for _, c, p in tile_comps(layout, base):
        sub = np.ascontiguousarray(planes[c][p.tile_y0:p.tile_y0 + p.tile_h, p.tile_x0:p.tile_x0 + p.tile_w])[None]
        _, lens, coded = O.encode_tile_rev(sub, 8, LEVELS, mct=False, origin=(p.tile_x0, p.tile_y0))
        blocks, _ = G.tile_layout(p)
        tt = np.zeros(len(lens), CODED_DTYPE)
        tt["length"] = lens
        tt["offset"] = off + np.concatenate([[0], np.cumsum(lens)[:-1]])
        tt["missing_msbs"] = [b.kmax - 1 for b in blocks]
        off += int(np.sum(lens))
        tabs.append(tt)
        chunks.append(coded)
    table, coded = np.concatenate(tabs), np.concatenate(chunks)
    whole = write_subsampled(layout, base, table, coded, G.CS_PROG(order) | MSBS)
    for a, b in zip(R.decode_planes(whole, SAMPLING, W, H), planes):
        assert np.array_equal(a, b.astype(np.int32))
    forged = table.copy()
    out_ = rng.random(len(table)) < 0.5
    forged["length"][out_] = 0
    forged["missing_msbs"][out_] = np.maximum(forged["missing_msbs"][out_].astype(np.int64) - rng.integers(0, 7, int(out_.sum())), 0)
    assert out_.any() and (~out_).any() and len(set(forged["missing_msbs"])) > 3
    cs = write_subsampled(layout, base, forged, coded, G.CS_PROG(order) | MSBS)
    back = R.decode_planes(cs, SAMPLING, W, H)
    assert [b.shape for b in back] == [p.shape for p in planes]
    assert not all(np.array_equal(a, b) for a, b in zip(back, planes))           # (blocks are missing: not the source)
    rows = G.read_packets(cs)["rows"]
    assert np.array_equal(rows["missing_msbs"], forged["missing_msbs"]) and np.array_equal(rows["length"], forged["length"])


# ---- 2. plan_rate_joint ----------------------------------------------------------------------------------------------------------
_units = None


def _sources():
    csrc = os.path.join(ROOT, "grok_amd", "csrc")
    return [os.path.join(HERE, "c", "rate_joint_units.cpp"), os.path.join(csrc, "encode_plan.cpp"), os.path.join(csrc, "geometry.cpp")]


def units():
    global _units
    if _units is None:
        out = os.path.join(tempfile.mkdtemp(prefix="rate_joint_units_"), "librate_joint_units.so")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-D_GLIBCXX_ASSERTIONS", "-fPIC", "-shared"] + _sources() +
                              ["-o", out, "-Wl,--no-undefined", "-lpthread"])
        _units = C.CDLL(out)
        _units.rj_plan.argtypes = [C.c_uint32, C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p]
        _units.rj_max_blocks.restype = C.c_uint64
    return _units


def plan(unit_blocks, batches, max_drop=6, skip=True):
    """-> None when refused, else (n, first_row [unit], [map of every batch], per_unit [batch], info)"""
    ub = np.asarray(unit_blocks, np.uint64)
    members = np.asarray([u for b in batches for u in b], np.uint32)
    lens = np.asarray([len(b) for b in batches], np.uint32)
    first, maps, per = np.zeros(len(ub), np.uint64), np.zeros(max(len(members), 1), np.uint64), np.zeros(max(len(lens), 1), np.uint32)
    info = np.zeros(6, np.uint64)
    ok = units().rj_plan(max_drop, int(skip), ub.ctypes.data, len(ub), members.ctypes.data, lens.ctypes.data, len(lens), first.ctypes.data,
                         maps.ctypes.data, per.ctypes.data, info.ctypes.data)
    assert ok in (0, 1)
    if not ok:
        return None
    at = np.concatenate([[0], np.cumsum(lens)]).astype(int)
    return int(info[0]), first, [maps[at[k]:at[k + 1]] for k in range(len(lens))], per[:len(lens)], info


def image_units(sampling, w, h, tw, th):
    """the units of a sub-sampled image as the encoders cut it -- tile by tile, within a tile run by run (consecutive components of
    equal factors) -> (block count of every unit, its geometry key, the writer's rows per unit)"""
    layout = G.ImageLayout.make(w, h, tw, th)
    base = G.TileParams.make(1, 1, len(sampling), 8, LEVELS, mct=False)
    runs, c0 = [], 0
    while c0 < len(sampling):
        n = 1
        while c0 + n < len(sampling) and sampling[c0 + n] == sampling[c0]:
            n += 1
        runs.append((c0, n))
        c0 += n
    comps = tile_comps(layout, base, sampling)
    blocks, keys = [], []
    for t in range(len(comps) // len(sampling)):
        for c0, n in runs:
            p = comps[t * len(sampling) + c0][2]
            blocks.append(len(G.tile_layout(p)[0]) * n)
            keys.append((n, p.tile_w, p.tile_h, p.tile_x0 % (TW * 2), p.tile_y0 % (TH * 2)))
    writer_rows = [len(G.tile_layout(p)[0]) for _, _, p in comps]
    return blocks, keys, writer_rows


@pytest.mark.parametrize("sampling", [[(1, 1), (2, 2), (2, 2)], [(1, 1), (2, 1), (2, 1)], [(1, 1), (2, 2), (2, 2), (1, 1)]], ids=["420", "422", "420+a"])
def test_joint_rows_are_the_writers_and_a_partition(sampling):
    """The rows are a partition of 0 .. N - 1 without a permutation inside a unit: unit u's rows are first_row[u] .. + its blocks, the
    units one behind the other in the writer's order (tile, run, component), and every batch's map points at its members' first rows"""
    blocks, keys, writer_rows = image_units(sampling, 250, 190, 128, 96)
    groups = {}                                     # (the planner asks of a batch only that its members have one block count)
    for u in range(len(blocks)):
        groups.setdefault(blocks[u], []).append(u)
    batches = list(groups.values())
    assert len(batches) > 1 and any(len(b) > 1 and max(b) - min(b) >= len(b) for b in batches)       # members not adjacent in joint order
    n, first, maps, per, info = plan(blocks, batches)
    assert n == sum(blocks) == sum(writer_rows)                        # the table the writer takes, row for row
    assert np.array_equal(first, np.concatenate([[0], np.cumsum(blocks)[:-1]]))
    hits = np.zeros(n, np.int64)
    for b, m, bpu in zip(batches, maps, per):
        assert np.array_equal(m, first[b]) and all(blocks[u] == bpu for u in b)
        for r in m:
            hits[int(r):int(r) + int(bpu)] += 1
    assert (hits == 1).all()
    assert list(info[1:]) == [8, 8 * n * 4, 8 * n * 8, n * 8, n]


def test_joint_order_does_not_depend_on_the_batches():
    """the same units as geometry groups, as one batch per unit, with shuffled members and shuffled batches: the same unit rows"""
    blocks, keys, _ = image_units([(1, 1), (2, 2), (2, 2)], 250, 190, 128, 96)
    groups = {}
    for u in range(len(blocks)):
        groups.setdefault(blocks[u], []).append(u)
    by_group = list(groups.values())
    per_unit = [[u] for u in range(len(blocks))]
    rng = np.random.default_rng(1)
    shuffled = [list(rng.permutation(b)) for b in by_group]
    shuffled = [shuffled[i] for i in rng.permutation(len(shuffled))]
    want = plan(blocks, by_group)
    for other in (per_unit, shuffled):
        got = plan(blocks, other)
        assert got[0] == want[0] and np.array_equal(got[1], want[1])
        for b, m in zip(other, got[2]):
            assert np.array_equal(m, want[1][b])
    same = [21] * 6                                                     # units of one geometry: one batch, or two, in any order
    assert np.array_equal(plan(same, [[0, 1, 2, 3, 4, 5]])[1], plan(same, [[5, 0, 3], [1, 4, 2]])[1])


def test_joint_plan_refusals():
    ub = [40, 14, 28, 10, 34, 14, 22, 10]
    good = [[0], [1, 5], [2], [3, 7], [4], [6]]
    assert plan(ub, good) is not None
    assert plan(ub, good, max_drop=13) is None
    assert plan(ub, good[:-1]) is None                                  # a unit in no batch
    assert plan(ub, good + [[0]]) is None                               # a unit in two
    assert plan(ub, [[0, 1], [5], [2], [3, 7], [4], [6]]) is None       # members of different block counts
    assert plan(ub, [[0], [1, 5], [2], [3, 8], [4], [6]]) is None       # no such unit
    assert plan([4, 0, 4], [[0, 2], [1]]) is None                       # an empty unit
    # more rows than the kernels index (2^31 - 1): refused -- the plan holds a row per unit, nothing of that size is allocated
    top = int(units().rj_max_blocks())
    assert top == 2 ** 31 - 1
    assert plan([1 << 30, (1 << 30) - 1], [[0], [1]])[0] == top
    assert plan([1 << 30, 1 << 30], [[0, 1]]) is None
    assert plan([top + 1], [[0]]) is None
    assert plan([2 ** 64 - 1, 2], [[0], [1]]) is None                   # (no wrap-around of the sum)


def test_joint_plan_driver_under_sanitizers():
    """tests/c/rate_joint_units.cpp as a program of its own (its main walks the same cases) under AddressSanitizer and UBSan"""
    exe = os.path.join(tempfile.mkdtemp(prefix="rate_joint_main_"), "rate_joint_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-D_GLIBCXX_ASSERTIONS", "-DRATE_JOINT_MAIN",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] + _sources() + ["-o", exe, "-lpthread"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "0 failure(s)" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, \
        r.stdout + r.stderr
