"""CPU: the host planning of two forward DWT levels in one launch (grok_amd/csrc/encode_plan.cpp plan_dwt_pair / plan_dwt_pair_at,
encode_constants.h dwt_pair_rows) through the small driver tests/c/dwt_pair_plan_units.cpp, built on first use with g++ together with
encode_plan.cpp and geometry.cpp: no GPU, no HIP, no libgrok_amd.so.

When a pair is planned: both levels are packed levels, the route is fused with int16 planes, the width is a
multiple of 8 of at least 512, the height a multiple of 4 of at least 32, both origins are even, the pixels are planar 8-bit planes of
an MCT triple.  Which rows a segment computes: the kernel takes them from the same dwt_pair_rows."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from grok_amd.capi import TileParams

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_lib = None


def _sources():
    csrc = os.path.join(ROOT, "grok_amd", "csrc")
    return [os.path.join(HERE, "c", "dwt_pair_plan_units.cpp"), os.path.join(csrc, "encode_plan.cpp"), os.path.join(csrc, "geometry.cpp")]


def lib():
    global _lib
    if _lib is None:
        out = os.path.join(tempfile.mkdtemp(prefix="dwt_pair_plan_units_"), "libdwt_pair_plan_units.so")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-D_GLIBCXX_ASSERTIONS", "-fPIC", "-shared"] + _sources() +
                              ["-o", out, "-Wl,--no-undefined", "-lpthread"])
        _lib = C.CDLL(out)
    return _lib


def plan(p, l=0, ntiles=1, planes16=True, interleaved=False, switch=True):
    """-> None when there is no pair, else dict(lanes, strip_cols, seg_pairs, grid_x, grid_y, key)"""
    out = np.zeros(9, np.uint32)
    lib().dp_plan(C.byref(p), l, ntiles, int(planes16), int(interleaved), int(switch), out.ctypes.data_as(C.c_void_p))
    v = [int(x) for x in out]
    if not v[0]:
        return None
    return dict(lanes=v[1], strip_cols=v[2], seg_pairs=v[3], grid_x=v[4], grid_y=v[5], key=tuple(v[6:9]))


def rows(seg, seg_pairs, ch):
    out = np.zeros(6, np.int32)
    lib().dp_rows(seg, seg_pairs, ch, out.ctypes.data_as(C.c_void_p))
    return dict(zip(("store0", "store1", "first", "last", "low0", "low1"), (int(x) for x in out)))


def test_instances():
    """the pair's own list: the triple from 8-bit pixel planes, 128 and 256 lanes"""
    out = np.zeros(3 * 16, np.uint32)
    n = lib().dp_instances(out.ctypes.data_as(C.c_void_p))
    assert sorted(tuple(int(x) for x in out[3 * i:3 * i + 3]) for i in range(n)) == [(3, 1, 128), (3, 1, 256)]


def test_headline():
    """8192^2 x 3, 8 bits: 256 lanes, nine strips of 960 columns (as level 0 alone: two halo lanes a side still leave 252 x 4 >= 960),
    and segments of 32 level-0 pairs: the floor of 1024 workgroups halves 64 while 9 x (4096 / seg) stays below it -- 9 x 64 = 576
    at 64, 9 x 128 = 1152 at 32.  64 tiles of 1024^2: three strips of 384 columns, 3 x 8 x 64 = 1536 workgroups at 64 pairs already,
    but a segment has 32 pairs at the most"""
    assert lib().dp_min_wgs() == 1024
    s = plan(TileParams.make(8192, 8192, 3, 8, 5))
    assert s == dict(lanes=256, strip_cols=960, seg_pairs=32, grid_x=9, grid_y=128, key=(3, 1, 256))
    s = plan(TileParams.make(1024, 1024, 3, 8, 5), ntiles=64)
    assert s == dict(lanes=128, strip_cols=384, seg_pairs=32, grid_x=3, grid_y=16, key=(3, 1, 128))


def test_small_shapes():
    """widths up to 2048 take 128 lanes; short levels end at segments of 8 pairs (the least row_segment_pairs gives)"""
    assert plan(TileParams.make(512, 32, 3, 8, 5)) == dict(lanes=128, strip_cols=256, seg_pairs=8, grid_x=2, grid_y=2, key=(3, 1, 128))
    assert plan(TileParams.make(512, 36, 3, 8, 2)) == dict(lanes=128, strip_cols=256, seg_pairs=8, grid_x=2, grid_y=3, key=(3, 1, 128))
    assert plan(TileParams.make(1000, 48, 3, 8, 5)) == dict(lanes=128, strip_cols=384, seg_pairs=8, grid_x=3, grid_y=3, key=(3, 1, 128))
    assert plan(TileParams.make(2056, 40, 3, 8, 5)) == dict(lanes=256, strip_cols=704, seg_pairs=8, grid_x=3, grid_y=3, key=(3, 1, 256))
    assert plan(TileParams.make(512, 32, 3, 8, 2), ntiles=8)["key"] == (3, 1, 128)


REFUSED = {
    "width 516": dict(p=lambda: TileParams.make(516, 32, 3, 8, 5)),
    "width 504": dict(p=lambda: TileParams.make(504, 32, 3, 8, 5)),
    "height 34": dict(p=lambda: TileParams.make(512, 34, 3, 8, 5)),
    "height 28": dict(p=lambda: TileParams.make(512, 28, 3, 8, 5)),
    "12 bits": dict(p=lambda: TileParams.make(512, 32, 3, 12, 5)),
    "irreversible": dict(p=lambda: TileParams.make(512, 32, 3, 8, 5, irreversible=True)),
    "interleaved": dict(p=lambda: TileParams.make(512, 32, 3, 8, 5), interleaved=True),
    "odd origin": dict(p=lambda: TileParams.make(512, 32, 3, 8, 5, origin=(1, 0))),
    "level 1 on an odd origin": dict(p=lambda: TileParams.make(512, 32, 3, 8, 5, origin=(0, 2))),
    "one level": dict(p=lambda: TileParams.make(512, 32, 3, 8, 1)),
    "int32 planes": dict(p=lambda: TileParams.make(512, 32, 3, 8, 5), planes16=False),
    "mono": dict(p=lambda: TileParams.make(512, 32, 1, 8, 5)),
    "four components": dict(p=lambda: TileParams.make(512, 32, 4, 8, 5)),
    "no colour transform": dict(p=lambda: TileParams.make(512, 32, 3, 8, 5, mct=False)),
    "signed": dict(p=lambda: TileParams.make(512, 32, 3, 8, 5, sgnd=True)),
    "the switch": dict(p=lambda: TileParams.make(512, 32, 3, 8, 5), switch=False),
    "levels 1 and 2": dict(p=lambda: TileParams.make(2048, 64, 3, 8, 5), l=1),
}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_refusals(name):
    """one condition each; the same call without it has a pair"""
    kw = dict(REFUSED[name])
    p = kw.pop("p")()
    assert plan(p, **kw) is None
    assert plan(TileParams.make(512, 32, 3, 8, 5)) is not None and plan(TileParams.make(2048, 64, 3, 8, 5)) is not None


@pytest.mark.parametrize("w,h", [(512, 32), (512, 36), (1000, 48), (2056, 40), (8192, 8192)])
def test_segment_rows(w, h):
    """for every segment: the level-0 pairs it computes cover what its level-1 pairs read (level-1 pair j: LL rows 2j - 2 .. 2j + 2, the
    first two through the high-pass term it shares with pair j - 1), every pair of either level is stored by exactly one segment,
    segments start on even pairs, and nothing is further than one reflection outside the level"""
    s = plan(TileParams.make(w, h, 3, 8, 5))
    sh, sh1 = h // 2, h // 4
    assert s["seg_pairs"] % 2 == 0 and s["grid_y"] == -(-sh // s["seg_pairs"])
    up, low = np.zeros(sh, int), np.zeros(sh1, int)
    for seg in range(s["grid_y"]):
        r = rows(seg, s["seg_pairs"], h)
        assert r["store0"] % 2 == 0 and r["store1"] % 2 == 0 and 0 <= r["store0"] < r["store1"] <= sh
        assert (r["low0"], r["low1"]) == (r["store0"] // 2, r["store1"] // 2)
        up[r["store0"]:r["store1"]] += 1
        low[r["low0"]:r["low1"]] += 1
        need = range(2 * r["low0"] - 2, 2 * r["low1"] + 1)
        assert r["first"] <= need[0] and need[-1] <= r["last"] and r["first"] <= r["store0"] and r["store1"] - 1 <= r["last"]
        assert -2 <= r["first"] and r["last"] <= sh
    assert (up == 1).all() and (low == 1).all()
    if (w, h) == (512, 36):
        assert rows(s["grid_y"] - 1, s["seg_pairs"], h) == dict(store0=16, store1=18, first=14, last=18, low0=8, low1=9), "a last segment of two pairs"


def test_driver_under_sanitizers():
    """tests/c/dwt_pair_plan_units.cpp as a program of its own (its main walks the same cases) under AddressSanitizer and UBSan"""
    exe = os.path.join(tempfile.mkdtemp(prefix="dwt_pair_plan_main_"), "dwt_pair_plan_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-D_GLIBCXX_ASSERTIONS", "-DDWT_PAIR_MAIN",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] + _sources() + ["-o", exe, "-lpthread"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "0 failure(s)" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, \
        r.stdout + r.stderr
