"""CPU: the encode path's host planning (grok_amd/csrc/encode_plan.cpp) -- K3's block classes, their LDS buffers, the arena and its
allocator, which class goes to which stream and when, the call's route, the shape of a forward DWT level -- through the small driver
tests/c/encode_plan_units.cpp, built on first use with g++ together with encode_plan.cpp and geometry.cpp: no GPU, no HIP, no
libgrok_amd.so.  -D_GLIBCXX_ASSERTIONS: an index past the end of a std::vector aborts.

The expected numbers are literals, worked out by hand from the formulas of the code this planner was lifted out of (the working is in
each test's docstring); the properties (partitions, "big" blocks) are checked against the block table the geometry gives, with the
worst-case LDS formula restated here in lds_worst()."""
import ctypes as C
import itertools
import os
import subprocess
import tempfile

import numpy as np
import pytest

from grok_amd.capi import TileParams

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TOP, REST, ALL, TOP_SMALL, TOP_BIG, REST_SMALL, REST_BIG = range(7)          # HtRole
AFTER_LEVEL0, AFTER_LAST_LEVEL, RUN_HT = range(3)                            # HtPoint
NOT_HERE, MAIN, SIDE, SIDE2 = range(4)                                       # HtStream
_lib = None


def lib():
    global _lib
    if _lib is None:
        csrc = os.path.join(ROOT, "grok_amd", "csrc")
        out = os.path.join(tempfile.mkdtemp(prefix="encode_plan_units_"), "libencode_plan_units.so")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-D_GLIBCXX_ASSERTIONS", "-fPIC", "-shared",
                               os.path.join(HERE, "c", "encode_plan_units.cpp"), os.path.join(csrc, "encode_plan.cpp"),
                               os.path.join(csrc, "geometry.cpp"), "-o", out, "-Wl,--no-undefined", "-lpthread"])
        _lib = C.CDLL(out)
        _lib.ep_lds_bytes.restype = C.c_uint64
        _lib.ep_pk_strip_cols.restype = C.c_uint32
    return _lib


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def constants():
    out = np.zeros(14, np.uint64)
    lib().ep_constants(ptr(out))
    names = ("max_classes", "regions", "chunk", "chunk_small", "alloc_bytes", "lds_16_waves", "lds_per_cu", "max_waves",
             "frame_stream_samples", "min_wgs_packed", "min_wgs", "pk_lane_cols", "strip_cols", "schedule_rows")
    return dict(zip(names, (int(v) for v in out)))


def test_constants():
    """what the kernels and the planner agree on, as the issue of this split lists it (GRK_HT_ALLOC_REGIONS not overridden: 64)"""
    k = constants()
    assert (k["max_classes"], k["regions"], k["chunk"], k["chunk_small"]) == (24, 64, 64 << 10, 32 << 10)
    assert k["alloc_bytes"] == 256 * 65
    assert (k["lds_16_waves"], k["lds_per_cu"], k["max_waves"]) == (10240, 160 << 10, 32)
    assert k["frame_stream_samples"] == 16 << 20
    assert (k["min_wgs_packed"], k["min_wgs"], k["pk_lane_cols"], k["strip_cols"]) == (2048, 4096, 4, 448)


# ---- block classes ---------------------------------------------------------------------------------------------------------------

def classes(p, lds_cap, kmax=None):
    """-> (blocks [rows][res, samples, quads, kmax], [(role, rows of the class, its record)])"""
    cap = 1 << 16
    blocks, sel, cls, out = np.zeros((cap, 4), np.uint32), np.zeros(4 * cap, np.uint32), np.zeros((24, 7), np.uint32), np.zeros(3, np.uint32)
    k = None if kmax is None else ptr(np.asarray(kmax, np.uint8))
    rc = lib().ep_classes(C.byref(p), int(lds_cap), k, ptr(blocks), C.c_uint64(cap), ptr(sel), C.c_uint64(4 * cap), ptr(cls), ptr(out))
    assert rc == 0
    nrows, nsel, ncls = (int(v) for v in out)
    res = []
    for c in cls[:ncls]:
        rec = dict(zip(("count", "max_kmax", "max_samples", "max_quads", "cap_kmax", "first", "role"), (int(v) for v in c)))
        res.append((rec["role"], [int(v) for v in sel[rec["first"]:rec["first"] + rec["count"]]], rec))
    assert sum(len(r) for _, r, _ in res) == nsel, "the classes' lists fill the selection list"
    return blocks[:nrows].astype(np.int64), res


def lds_worst(samples, quads, kmax):
    """the worst-case LDS need of a block, restated: (kmax + 2) bits per sample and 15 per quad + 4, each stream rounded up to words
    + 4 words of slack, to a multiple of 4 words; the staging area (vlc bits / 7 + 16 bytes, to 16, at least 512); 256 MEL bytes"""
    ms, vlc = samples * (kmax + 2), quads * 15 + 4
    words = lambda bits: ((bits + 31) // 32 + 4 + 3) & ~3
    return (words(ms) + words(vlc)) * 4 + max((vlc // 7 + 16 + 15) & ~15, 512) + 256


GEOMETRIES = {
    "256x256x3 L5 cblk64": lambda: TileParams.make(256, 256, 3, 8, 5),
    "200x136 off the origin cblk32": lambda: TileParams.make(200, 136, 3, 8, 3, cblk=(5, 5), origin=(37, 21)),
    "0 levels": lambda: TileParams.make(96, 80, 3, 8, 0, cblk=(5, 5)),
    "1 component 16 bits": lambda: TileParams.make(192, 192, 1, 16, 4),
    "16 bits 9/7": lambda: TileParams.make(192, 192, 3, 16, 4, irreversible=True),
}


def check_extents(blocks, rows, rec):
    """count, the worst extents and the sample-weighted exponent (a tie: the lower one) of a class, from its rows"""
    b = blocks[rows]
    assert rec["count"] == len(rows) > 0, "an empty class is not emitted"
    assert (rec["max_kmax"], rec["max_samples"], rec["max_quads"]) == (b[:, 3].max(), b[:, 1].max(), b[:, 2].max())
    hist = np.zeros(64, np.int64)
    np.add.at(hist, b[:, 3], b[:, 1])
    assert rec["cap_kmax"] == int(np.argmax(hist)), "the exponent with the most samples (argmax: the first = the lower of a tie)"


@pytest.mark.parametrize("name", sorted(GEOMETRIES))
def test_classes_with_the_cap(name):
    """three classes: top and rest partition the tile's blocks, the all class lists every block once, in table order"""
    p = GEOMETRIES[name]()
    blocks, cls = classes(p, True)
    n, L = len(blocks), p.num_levels
    by_role = {role: rows for role, rows, _ in cls}
    is_top = (blocks[:, 0] == L) & (L >= 1)
    assert by_role[ALL] == list(range(n))
    assert by_role.get(TOP, []) == [i for i in range(n) if is_top[i]]
    assert by_role[REST] == [i for i in range(n) if not is_top[i]]
    assert [role for role, _, _ in cls] == ([TOP, REST, ALL] if L else [REST, ALL]), "with 0 levels no block is top; no empty class"
    for _, rows, rec in cls:
        check_extents(blocks, rows, rec)


@pytest.mark.parametrize("name", sorted(GEOMETRIES))
def test_classes_without_the_cap(name):
    """up to four classes that partition the blocks; a block is big exactly when its worst-case LDS need exceeds 10240 bytes"""
    p = GEOMETRIES[name]()
    blocks, cls = classes(p, False)
    n, L = len(blocks), p.num_levels
    want = {TOP_SMALL: [], TOP_BIG: [], REST_SMALL: [], REST_BIG: []}
    for i, (res, samples, quads, kmax) in enumerate(blocks):
        big = lds_worst(samples, quads, kmax) > 10240
        assert lib().ep_lds_bytes(int(samples), int(quads), int(kmax)) == lds_worst(samples, quads, kmax)
        want[(TOP_BIG if big else TOP_SMALL) if (res == L and L >= 1) else (REST_BIG if big else REST_SMALL)].append(i)
    order = [r for r in (TOP_SMALL, TOP_BIG, REST_SMALL, REST_BIG) if want[r]]
    assert [role for role, _, _ in cls] == order, "classes in this order, empty ones left out"
    assert sorted(i for _, rows, _ in cls for i in rows) == list(range(n)), "a partition"
    for role, rows, rec in cls:
        assert rows == want[role]
        check_extents(blocks, rows, rec)


def test_class_counts_256():
    """256 x 256 x 3, 5 levels, 64 x 64 blocks.  Per component, in table order (coarsest resolution first): resolution 0 the 8 x 8 LL
    (1 block), resolutions 1 .. 4 three bands (HL, LH, HH) of one block each (12), resolution 5 three 128 x 128 bands of 4 blocks
    (12): 25 rows, 75 in all; top 36, rest 39.  The exponents are set here (the geometry's come from the filters' gains): LL 8,
    HL / LH 9, HH 10.  A 64 x 64 block needs 512 x (Kmax + 2) + 4448 bytes: 10592 at Kmax 10 (> 10240: big), 10080 at 9 (small); 64 x 64
    are the blocks of resolution 5 and the three of resolution 4.  Big: the 4 HH blocks of resolution 5 per component (12) and the HH
    block of resolution 4 (3).  Most samples of the top: Kmax 9 (8 x 4096 per component against 4 x 4096 at 10); of the rest: 9 as
    well (2 x (64 + 256 + 1024 + 4096) = 10880 against 5440 at 10 and 64 at 8)."""
    p = GEOMETRIES["256x256x3 L5 cblk64"]()
    kmax = [8] + [9, 9, 10] * 4 + [9] * 8 + [10] * 4
    blocks, cap = classes(p, True, kmax=kmax)
    assert [int(v) for v in blocks[:25, 0]] == [0] + [r for r in (1, 2, 3, 4) for _ in range(3)] + [5] * 12, "the table order assumed above"
    assert [(role, rec["count"]) for role, _, rec in cap] == [(TOP, 36), (REST, 39), (ALL, 75)]
    assert [(rec["max_kmax"], rec["max_samples"], rec["max_quads"], rec["cap_kmax"]) for _, _, rec in cap] == [(10, 4096, 1024, 9)] * 3
    assert [rec["first"] for _, _, rec in cap] == [0, 36, 75]
    _, nocap = classes(p, False, kmax=kmax)
    assert [(role, rec["count"]) for role, _, rec in nocap] == [(TOP_SMALL, 24), (TOP_BIG, 12), (REST_SMALL, 36), (REST_BIG, 3)]
    assert [rec["max_kmax"] for _, _, rec in nocap] == [9, 10, 10, 10], "(the small HH blocks of resolutions 1 .. 3 are at 10)"


def test_cap_kmax_tie_goes_to_the_lower_exponent():
    """0 levels, 128 x 64, one component, 64 x 64 blocks: two LL blocks of 4096 samples.  Exponents 9 and 7: a tie, 7 wins;
    a third of the width more for the 9 (192 x 64: blocks of exponents 9, 7, 9) and 9 wins."""
    _, cls = classes(TileParams.make(128, 64, 1, 8, 0), True, kmax=[9, 7])
    assert [(role, rec["cap_kmax"], rec["max_kmax"]) for role, _, rec in cls] == [(REST, 7, 9), (ALL, 7, 9)]
    _, cls = classes(TileParams.make(192, 64, 1, 8, 0), True, kmax=[9, 7, 9])
    assert [rec["cap_kmax"] for _, _, rec in cls] == [9, 9]


# ---- LDS layout ----------------------------------------------------------------------------------------------------------------------

def lds(max_kmax, cap_kmax, irrev=False, fallback=True, samples=4096, quads=1024):
    out = np.zeros(15, np.uint64)
    lib().ep_lds(samples, quads, max_kmax, cap_kmax, int(irrev), int(fallback), ptr(out))
    names = ("ms_words", "vlc_words", "ms_cap_bits", "vlc_cap_bits", "stage_bytes", "bytes", "waves")
    v = [int(x) for x in out]
    return dict(zip(names, v[:7])), dict(zip(names, v[7:14])), bool(v[14])


def test_lds_64x64_kmax_10():
    """64 x 64, 1024 quads, Kmax 10, reversible.
    Capped: 8 bits per sample (Kmax <= 11) = 32768 bits = 1024 words, + 4, to a multiple of 4: 1028.  VLC 10 x 1024 + 4 = 10244 bits
    = 321 words, + 4 -> 328.  Staging 10244 / 7 = 1463, + 16 = 1479, to 16: 1488.  (1028 + 328) x 4 + 1488 + 256 = 7168 (the "7.0 KB
    per wave" of VERDICT.md); 163840 / 7168 = 22 waves.
    Worst case: 12 bits per sample = 49152 bits = 1536 words -> 1540.  VLC 15 x 1024 + 4 = 15364 bits = 481 words -> 488.  Staging
    15364 / 7 = 2194, + 16 = 2210 -> 2224.  (1540 + 488) x 4 + 2224 + 256 = 10592; 15 waves.  22 > 15: the cap is used."""
    full, cap, use_cap = lds(10, 10)
    assert cap == dict(ms_words=1028, vlc_words=328, ms_cap_bits=32768, vlc_cap_bits=10244, stage_bytes=1488, bytes=7168, waves=22)
    assert full == dict(ms_words=1540, vlc_words=488, ms_cap_bits=49152, vlc_cap_bits=15364, stage_bytes=2224, bytes=10592, waves=15)
    assert use_cap
    assert not lds(10, 10, fallback=False)[2], "no fallback list: worst-case buffers"


def test_lds_irreversible_kmax_20():
    """irreversible: 8 bits per sample whatever the exponent -- the capped layout of Kmax 10 above; the worst case 22 bits per
    sample = 2816 words -> 2820, (2820 + 488) x 4 + 2224 + 256 = 15712 bytes, 10 waves"""
    full, cap, use_cap = lds(20, 20, irrev=True)
    assert (cap["ms_words"], cap["vlc_words"], cap["stage_bytes"], cap["bytes"], cap["waves"]) == (1028, 328, 1488, 7168, 22)
    assert (full["ms_words"], full["bytes"], full["waves"]) == (2820, 15712, 10)
    assert use_cap and not lds(20, 20, irrev=True, fallback=False)[2]


def test_lds_reversible_kmax_14():
    """reversible above Kmax 11: Kmax - 3 = 11 bits per sample = 45056 bits = 1408 words -> 1412; (1412 + 328) x 4 + 1488 + 256 =
    8704 bytes, 18 waves.  Worst case 16 bits = 2048 words -> 2052, (2052 + 488) x 4 + 2480 = 12640, 12 waves.
    The cap goes by cap_kmax, the worst case by max_kmax: a class whose samples sit at Kmax 9 (8 bits per sample) with one block at 14"""
    full, cap, use_cap = lds(14, 14)
    assert (cap["ms_words"], cap["ms_cap_bits"], cap["bytes"], cap["waves"]) == (1412, 45056, 8704, 18)
    assert (full["ms_words"], full["bytes"], full["waves"]) == (2052, 12640, 12)
    assert use_cap
    full, cap, _ = lds(14, 9)
    assert (full["bytes"], cap["bytes"]) == (12640, 7168)


def test_lds_small_blocks_gain_nothing():
    """a 16 x 16 block (64 quads) at Kmax 10: worst case 3072 bits = 96 words -> 100, VLC 964 bits = 31 words -> 36, staging 512:
    (100 + 36) x 4 + 512 + 256 = 1312 bytes -- 32 waves either way, the cap buys nothing and is not used"""
    full, cap, use_cap = lds(10, 10, samples=256, quads=64)
    assert (full["bytes"], full["waves"], cap["waves"], use_cap) == (1312, 32, 32, False)


# ---- allocator -------------------------------------------------------------------------------------------------------------------

def arena(nblocks, cls, raw=0, ntiles=1):
    out = np.zeros(5 + len(cls), np.uint64)
    lib().ep_arena(C.c_uint64(nblocks), C.c_uint64(raw), ntiles, ptr(np.asarray(cls, np.uint32).reshape(-1)), len(cls), ptr(out))
    v = [int(x) for x in out]
    return dict(regions=v[0], chunk=v[1], worst_block=v[2], arena_bytes=v[3], ovf_entries=v[4], ovf_base=v[5:])


B64_K10 = (1, 10, 4096, 1024)       # a class of 64 x 64 blocks at Kmax 10: (count, max_kmax, max_samples, max_quads)


@pytest.mark.parametrize("nblocks,regions", [(1, 1), (127, 1), (128, 2), (4095, 32), (4096, 64), (10 ** 6, 64)])
def test_allocator_regions(nblocks, regions):
    """doubled while a region would still hold 64 blocks, up to 64: 127 / 2 = 63 -> 1; 128 / 2 = 64 -> 2 (128 / 4 = 32);
    4095 / 64 = 63 -> 32; 4096 / 64 = 64 -> 64"""
    assert arena(nblocks, [B64_K10])["regions"] == regions


def test_allocator_chunk():
    """64 x 64 at Kmax 10: (4096 x 12 + 1024 x 15) x 16 / 15 / 8 + 280 = 64512 -> 68812 -> 8601 + 280 = 8881 bytes; twice that fits the
    32 KiB chunk: small jobs (below 16384 blocks) take it.  At Kmax 31: (4096 x 33 + 15360) x 16 / 15 / 8 + 280 = 150528 -> 160563 ->
    20070 + 280 = 20350; twice that is above 32 KiB: the large chunk at any size.  The worst block is the worst over the classes."""
    assert arena(16383, [B64_K10]) == dict(regions=64, chunk=32 << 10, worst_block=8881, arena_bytes=16383 * 64 + 65 * 65536 + (1 << 20),
                                           ovf_entries=2 * 16383, ovf_base=[0])
    assert arena(16384, [B64_K10])["chunk"] == 64 << 10
    k31 = (1, 31, 4096, 1024)
    assert arena(100, [k31])["worst_block"] == 20350
    assert arena(100, [k31])["chunk"] == 64 << 10 and arena(10 ** 6, [k31])["chunk"] == 64 << 10
    assert arena(100, [B64_K10, k31, B64_K10])["worst_block"] == 20350


def test_arena_bytes_and_fallback_bases():
    """256 x 256 x 3 at 8 bits, 2 tiles: raw 393216, 150 blocks -> 2 regions.  786432 + 9600 + 196608 + 1048576 = 2041216 (2 x raw, 64 per block, 3 chunks, 2^20).
    The classes' parts of the fallback list: the running sum of count x ntiles -- top 36, rest 39, all 75 -> 0, 72, 150 (300 entries)"""
    a = arena(150, [(36, 10, 4096, 1024), (39, 10, 4096, 1024), (75, 10, 4096, 1024)], raw=393216, ntiles=2)
    assert (a["regions"], a["arena_bytes"], a["ovf_entries"], a["ovf_base"]) == (2, 2041216, 300, [0, 72, 150])


# ---- schedule ------------------------------------------------------------------------------------------------------------------------

def launches(roles, overlapped, pipelined, L):
    """-> {role: [(point, stream)]} over the points of one call: run_dwt asks after level 0 and -- when that is not the last level as
    well -- after the last level, overlapped calls only; run_ht asks once"""
    points = [RUN_HT]
    if overlapped:
        points = [AFTER_LEVEL0] + ([AFTER_LAST_LEVEL] if L > 1 else []) + [RUN_HT]
    got = {}
    for role in roles:
        got[role] = []
        for at in points:
            st = lib().ep_class_stream(role, int(overlapped), int(pipelined), at, int(L == 1))
            if st != NOT_HERE:
                got[role].append((at, st))
    return got


@pytest.mark.parametrize("cap,overlapped,pipelined,L", list(itertools.product((True, False), (False, True), (False, True), (1, 2, 5))))
def test_schedule(cap, overlapped, pipelined, L):
    """every class that holds blocks is launched exactly once per call -- but the all class exactly when the call is not overlapped,
    and then alone.  (L = 0 is never overlapped and has no top class.)
    Checked once by hand: with the row {Rest, overlapped, pipelined, AfterLastLevel, Side2} of kHtSchedule removed the three cases
    [cap, overlapped, pipelined, L = 1 / 2 / 5] of this test fail ("launched exactly once") and the row count below; with it
    duplicated test_schedule_table_has_no_duplicates fails (14 rows, two for one key)."""
    roles = [TOP, REST, ALL] if cap else [TOP_SMALL, TOP_BIG, REST_SMALL, REST_BIG]
    got = launches(roles, overlapped, pipelined, L)
    last = AFTER_LEVEL0 if L == 1 else AFTER_LAST_LEVEL           # (where the last level's launches are asked for)
    for role in roles:
        if role == ALL:
            assert got[role] == ([] if overlapped else [(RUN_HT, MAIN)])
        elif cap and not overlapped:
            assert got[role] == [], "the all class is the only one launched"
        else:
            assert len(got[role]) == 1, "launched exactly once"
    if not overlapped:
        assert all(v in ([], [(RUN_HT, MAIN)]) for v in got.values())
        return
    streams = {role: v[0] for role, v in got.items() if v}
    if pipelined:
        assert all(st != MAIN for _, st in streams.values()), "nothing goes to the main stream"
    small_rest = REST if cap else REST_SMALL
    assert streams[small_rest] == ((last, SIDE2) if pipelined else (RUN_HT, MAIN))
    for role in (TOP, TOP_SMALL):
        if role in streams:
            assert streams[role] == (AFTER_LEVEL0, SIDE)
    if not cap:
        assert streams[TOP_BIG] == (AFTER_LEVEL0, SIDE2)
        assert streams[REST_BIG] == (last, SIDE2)


def test_schedule_table_has_no_duplicates():
    """13 rows; no (role, overlapped, pipelined) is spoken of twice -- the lookup takes the first row that fits, a second would be dead"""
    assert constants()["schedule_rows"] == 13
    for role, ov, pip in itertools.product(range(7), (0, 1), (0, 1)):
        assert lib().ep_schedule_rows_for(role, ov, pip) <= 1, (role, ov, pip)


# ---- route -----------------------------------------------------------------------------------------------------------------------

def test_planes16_ok():
    """4 x 2^prec x 2.25^(L - 1) + 8 L < 32767.  8 bits: L = 5: 1024 x 25.63 = 26244 + 40: yes; L = 6: 59049: no.
    7 bits: L = 6: 512 x 57.67 = 29525 + 48: yes.  Never for 9/7, above 8 bits or without a level."""
    ok = lambda *a, **k: bool(lib().ep_planes16_ok(C.byref(TileParams.make(256, 256, 3, *a, **k))))
    assert [ok(8, L) for L in range(1, 7)] == [True] * 5 + [False]
    assert ok(7, 6) and not ok(7, 7)
    assert not ok(8, 0) and not ok(9, 1) and not ok(8, 3, irreversible=True)


def test_pk16_level_ok():
    """8 M_l + 16 < 32767 with M_0 = 2^prec, M_(l+1) = 2.25 M_l + 4.  8 bits: 256, 580, 1309, 2949.25, 6639.8: 8 x 2949.25 + 16 =
    23610: yes; 8 x 6639.8 = 53118: no.  Signed samples: never."""
    p = TileParams.make(256, 256, 3, 8, 5)
    assert [bool(lib().ep_pk16_level_ok(C.byref(p), l)) for l in range(5)] == [True, True, True, True, False]
    s = TileParams.make(256, 256, 3, 8, 5, sgnd=True)
    assert not any(lib().ep_pk16_level_ok(C.byref(s), l) for l in range(5))


def route(p, overlap=True, pipelining=True, frame_streams=1, planes16=True, side=True, side2=True, on_device=True, align=0, samples=1 << 20):
    out = np.zeros(4, np.int32)
    lib().ep_route(C.byref(p), ptr(np.array([overlap, pipelining, frame_streams, planes16, side, side2, on_device, align, samples], np.uint64)),
                   ptr(out))
    return dict(zip(("fused", "overlap", "frame_stream", "h16"), (bool(v) for v in out)))


def test_route():
    p = TileParams.make(512, 512, 3, 8, 5)
    assert route(p) == dict(fused=True, overlap=True, frame_stream=True, h16=True)
    # fused: at least one level and a 4-byte-aligned pointer; without it no int16 planes and no frame stream
    for kw, q in (({"align": a}, p) for a in (1, 2, 3)):
        assert route(q, **kw) == dict(fused=False, overlap=True, frame_stream=False, h16=False)
    assert route(TileParams.make(512, 512, 3, 8, 0)) == dict(fused=False, overlap=False, frame_stream=False, h16=False)
    # overlap: the setting, a level, the side stream
    assert not route(p, overlap=False)["overlap"] and not route(p, side=False)["overlap"]
    # h16: the setting, fused, planes16_ok
    assert not route(p, planes16=False)["h16"] and not route(TileParams.make(512, 512, 3, 8, 6))["h16"]
    assert not route(TileParams.make(512, 512, 3, 12, 5))["h16"]
    # frame_stream: device pixels, fused, pipelining, both side streams, overlap
    for kw in ({"on_device": False}, {"pipelining": False}, {"side": False}, {"side2": False}, {"overlap": False}, {"align": 2}):
        assert not route(p, **kw)["frame_stream"], kw
    # ... and the size: frame_streams = 1 up to 16 << 20 samples, 0 never, 2 always
    assert route(p, samples=16 << 20)["frame_stream"] and not route(p, samples=(16 << 20) + 1)["frame_stream"]
    assert not route(p, frame_streams=0, samples=1)["frame_stream"]
    assert route(p, frame_streams=2, samples=1 << 40)["frame_stream"]


# ---- level shape -----------------------------------------------------------------------------------------------------------------

def _level(cw, ch, px=0, py=0, in_stride=None, m_stride=None, h16=True, pk=True, irreversible=False, px_lay=0, px_chan=0, px_row=0, zslots=1,
           fused=False, px_bytes=1):
    out = np.zeros(29, np.uint32)
    stride = (cw + 31) & ~31
    lib().ep_level(ptr(np.array([cw, ch, px, py, stride if in_stride is None else in_stride, stride if m_stride is None else m_stride,
                                 h16, pk, irreversible, px_lay, px_chan, px_row, zslots, fused, px_bytes], np.uint64)), ptr(out))
    return [int(v) for v in out]


def level(*args, **kw):
    return dict(zip(("packed", "lanes", "strip_cols", "all_fast", "seg_pairs", "grid_x", "grid_y"), _level(*args, **kw)[:7]))


def level_inst(nc, *args, **kw):
    """the instance of the part of nc components (1, or 3: the MCT triple): ("pk", NC, PX, NT, CH) or ("k", F97, NC, PX, H16, GEN, STR)"""
    row = _level(*args, **kw)[7 + 11 * (nc == 3):][:11]
    return ("pk",) + tuple(row[7:11]) if row[0] else ("k",) + tuple(row[1:7])


def test_level_packed_or_not():
    assert level(256, 16)["packed"] and level(1024, 1024)["packed"]
    for kw in (dict(cw=252), dict(cw=258), dict(ch=14), dict(ch=17), dict(px=1), dict(py=1), dict(h16=False), dict(pk=False),
               dict(irreversible=True), dict(px_lay=1), dict(px_lay=2, px_chan=2, px_row=2048),
               dict(cw=1 << 16, ch=1 << 15), dict(m_stride=1 << 22), dict(in_stride=1 << 22), dict(px_lay=2, px_chan=4, px_row=1 << 22)):
        args = dict(cw=1024, ch=1024)
        args.update(kw)
        got = level(**args)
        assert not got["packed"], kw
        assert (got["lanes"], got["strip_cols"]) == (256, 448), "the 32-bit kernels: 256 lanes, strips of 448 columns"
    for chan in (1, 3, 4):
        assert level(1024, 1024, px_lay=2, px_chan=chan, px_row=1024 * chan)["packed"]


def test_level_all_fast():
    """on the origin, even width >= 4, even height >= 16"""
    assert level(4, 16, pk=False)["all_fast"] and level(1000, 18, pk=False)["all_fast"]
    for kw in (dict(cw=2), dict(cw=5), dict(ch=14), dict(ch=17), dict(px=1), dict(py=1)):
        args = dict(cw=64, ch=64, pk=False)
        args.update(kw)
        assert not level(**args)["all_fast"], kw


def test_level_strips():
    """128 lanes up to 2048 columns (strips of up to 126 x 4 = 504 -> 448), 256 above (254 x 4 = 1016 -> 960); the strips share the
    width evenly in multiples of 64 columns and cover it.  2048: 5 strips of 448 (ceil(2048 / 5) = 410 -> 448).  2052: 3 strips of
    704 (684 -> 704).  1024: 3 strips of 384 (342 -> 384).  256: one of 256."""
    assert (level(2048, 64)["lanes"], level(2052, 64)["lanes"]) == (128, 256)
    assert [(level(cw, 64)["strip_cols"], level(cw, 64)["grid_x"]) for cw in (256, 1024, 2048, 2052)] == [(256, 1), (384, 3), (448, 5), (704, 3)]
    for cw in list(range(256, 4200, 4)) + [8192, 16384, 40000]:
        got = level(cw, 64)
        most = 448 if cw <= 2048 else 960
        assert got["packed"] and got["strip_cols"] % 64 == 0 and 64 <= got["strip_cols"] <= most
        assert got["strip_cols"] == lib().ep_pk_strip_cols(cw, got["lanes"])
        assert got["grid_x"] * got["strip_cols"] >= cw > (got["grid_x"] - 1) * got["strip_cols"], "the strips cover the width, none is empty"
    # the 32-bit kernels count the phantom column of an odd start
    assert level(448, 64, pk=False)["grid_x"] == 1 and level(448, 64, pk=False, px=1)["grid_x"] == 2


def test_level_row_segments():
    """seg_pairs: the largest of 64, 32, 16, 8 with strips x segments x z slots at the floor (2048 for a level asked to be packed,
    4096 else), or 8"""
    for cw, ch, z, pk in itertools.product((256, 448, 1000, 4096), (16, 100, 1024, 4097), (1, 3, 48), (True, False)):
        got = level(cw, ch, pk=pk, zslots=z)
        floor, pairs = (2048 if pk else 4096), (ch + 1) // 2
        wgs = lambda seg: got["grid_x"] * ((pairs + seg - 1) // seg) * z
        fits = [seg for seg in (64, 32, 16, 8) if wgs(seg) >= floor]
        assert got["seg_pairs"] == (fits[0] if fits else 8)
        assert got["grid_y"] == (pairs + got["seg_pairs"] - 1) // got["seg_pairs"]
    # an odd start's phantom row counts: 17 rows from an odd row are 9 pairs
    assert level(64, 17, py=1, pk=False)["grid_y"] == 2 and level(64, 15, py=1, pk=False)["grid_y"] == 1


def test_level_headline_8k():
    """8192 x 8192 x 3, level 0, packed, the MCT triple in one z slot.  kPkLaneCols = 4: 256 lanes (8192 > 2048) own at most
    254 x 4 = 1016 -> 960 columns; ceil(8192 / 960) = 9 strips, ceil(8192 / 9) = 911 -> 960 columns each: grid x = 9.  4096 row pairs:
    64 per workgroup give 9 x 64 = 576 workgroups, 32 give 1152, 16 give 9 x 256 = 2304 >= 2048: seg_pairs = 16 -- the "32-row
    segments" of the comment on kDwtMinWgsPacked --, grid y = 256.  At the 32-bit kernels' floor of 4096 it would be 8 (16-row segments)."""
    got = level(8192, 8192, zslots=1, px_lay=0)
    assert got == dict(packed=1, lanes=256, strip_cols=960, all_fast=1, seg_pairs=16, grid_x=9, grid_y=256)
    assert 2 * got["seg_pairs"] == 32
    # (the 32-bit kernels' 19 strips of 448 columns at their floor of 4096: 19 x 128 = 2432, 19 x 256 = 4864 -> 16 as well)
    assert level(8192, 8192, zslots=1, pk=False) == dict(packed=0, lanes=256, strip_cols=448, all_fast=1, seg_pairs=16, grid_x=19, grid_y=256)


# ---- kernel instances ------------------------------------------------------------------------------------------------------------

def instance_tables():
    out = np.zeros(6 * 64, np.uint32)
    n = lib().ep_dwt_instances(ptr(out))
    k = [("k",) + tuple(int(v) for v in out[6 * i:6 * i + 6]) for i in range(n)]
    n = lib().ep_dwt_pk_instances(ptr(out))
    return k, [("pk",) + tuple(int(v) for v in out[4 * i:4 * i + 4]) for i in range(n)]


def old_forward_ladder(fused, nc, packed, lanes, all_fast, irreversible, h16, px_bytes, px_lay, px_chan):
    """the nested ifs of launch_dwt_level / launch_dwt_level0_fused as they stood before the lists (dwt_instances.h), rung by rung;
    sh.packed, sh.lanes, sh.all_fast came from plan_dwt_level then as now"""
    def k(f97, nc, px, h16=0, gen=1, str_=0):
        return ("k", f97, nc, px, h16, gen, str_)

    def l0(f97, nc, px):                       # GRK_L0: the all-fast form where every strip is fast
        return k(f97, nc, px, 0, 0 if all_fast else 1)
    if not fused:
        if packed:
            return ("pk", 1, 0, lanes, 0)
        if irreversible:
            return k(1, 1, 0)
        return k(0, 1, 0, 1) if h16 else k(0, 1, 0)
    px = 1 if px_bytes == 1 else 2
    if px_lay != 0:
        if not irreversible and px == 1 and packed:
            if px_chan == 1:
                return ("pk", 1, 1, lanes, 1)
            if px_chan == 3:
                return ("pk", 3 if nc == 3 else 1, 1, lanes, 3)
            return ("pk", 3 if nc == 3 else 1, 1, lanes, 4)
        if irreversible:
            return k(1, nc, px, 0, 1, 1)
        if h16 and px == 1:
            return k(0, nc, 1, 1, 1, 1)
        return k(0, nc, px, 0, 1, 1)
    if irreversible:
        return l0(1, nc, px)
    if px == 1 and packed:
        return ("pk", nc, 1, lanes, 0)
    if h16 and px == 1:
        return k(0, nc, 1, 1)
    return l0(0, nc, px)


def test_level_parts():
    """the MCT triple, then each further component on its own; or every component on its own, as z slots of one launch"""
    def parts(mct, ncomp):
        out = np.zeros(16, np.uint32)
        n = lib().ep_level_parts(mct, ncomp, ptr(out))
        return int(out[0]), [tuple(int(v) for v in out[1 + 3 * i:4 + 3 * i]) for i in range(n)]
    assert parts(1, 3) == (1, [(0, 1, 3)])
    assert parts(1, 4) == (1, [(0, 1, 3), (3, 1, 1)])
    assert parts(1, 6) == (1, [(0, 1, 3), (3, 1, 1), (4, 1, 1), (5, 1, 1)])
    for ncomp in (1, 2, 3, 4):
        assert parts(0, ncomp) == (ncomp, [(0, ncomp, 1)])
    assert parts(1, 2) == (2, [(0, 2, 1)]) and parts(1, 1) == (1, [(0, 1, 1)])       # (no triple to transform)


def test_instance_tables_against_the_old_ladder():
    """Over the descriptor's discrete fields (shapes: packed with 128 and with 256 lanes, all-fast, general): the planner's key is what
    the old ladder picked, it is in its kernel's list, and every row of both lists is picked at least once."""
    k_rows, pk_rows = instance_tables()
    assert len(k_rows) == len(set(k_rows)) == 31 and len(pk_rows) == len(set(pk_rows)) == 16
    seen = set()
    for (cw, ch), fused, irreversible, h16, pk, px_bytes, px_lay, px_chan in itertools.product(
            ((1024, 64), (4096, 64), (34, 18), (33, 17)), (False, True), (False, True), (False, True), (False, True), (1, 2), (0, 1, 2),
            (1, 2, 3, 4)):
        kw = dict(h16=h16, pk=pk, irreversible=irreversible, px_lay=px_lay if fused else 0, px_chan=px_chan if fused else 0,
                  px_row=cw * px_chan * px_bytes if fused else 0, fused=fused, px_bytes=px_bytes)
        sh = level(cw, ch, **kw)
        for nc in (1, 3) if fused else (1,):
            got = level_inst(nc, cw, ch, **kw)
            want = old_forward_ladder(fused, nc, sh["packed"], sh["lanes"], sh["all_fast"], irreversible, h16, px_bytes, kw["px_lay"], kw["px_chan"])
            assert got == want, (cw, ch, nc, kw)
            assert got in (pk_rows if got[0] == "pk" else k_rows), (cw, ch, nc, kw)
            seen.add(got)
    assert seen == set(k_rows) | set(pk_rows), "rows no descriptor selects: %s" % sorted((set(k_rows) | set(pk_rows)) - seen)


def test_unfused_level_names_no_triple_instance():
    """a level between planes has one part; the triple's slot holds a key that is in no list (the launcher refuses it)"""
    k_rows, pk_rows = instance_tables()
    row = _level(1024, 64)[18:]
    assert ("k",) + tuple(row[1:7]) not in k_rows and ("pk",) + tuple(row[7:11]) not in pk_rows
