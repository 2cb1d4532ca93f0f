"""CPU: the host planning of quality-targeted encodes (grok_amd/csrc/encode_plan.cpp: plan_quality, quality_samples) through
tests/c/quality_plan_units.cpp, built on first use with g++ together with encode_plan.cpp and geometry.cpp: no GPU, no HIP.  The
budget D = S * peak^2 * 10^(-psnr / 10) against Python's own pow to 1e-12 relative (a few ulps of pow, with room to spare); S, the sum
over the components of the component's OWN samples, against the sum over the units the encoders cut an image into."""
import ctypes as C
import math
import os
import subprocess
import tempfile

import pytest

import grok_amd as G
from test_t2_reader_subsampled_cpu import num_tiles, tile_comp

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_lib = None


def lib():
    global _lib
    if _lib is None:
        csrc = os.path.join(ROOT, "grok_amd", "csrc")
        out = os.path.join(tempfile.mkdtemp(prefix="quality_plan_units_"), "libquality_plan_units.so")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-D_GLIBCXX_ASSERTIONS", "-fPIC", "-shared",
                               os.path.join(HERE, "c", "quality_plan_units.cpp"), os.path.join(csrc, "encode_plan.cpp"),
                               os.path.join(csrc, "geometry.cpp"), "-o", out, "-Wl,--no-undefined", "-lpthread"])
        _lib = C.CDLL(out)
        _lib.qp_quality.argtypes = [C.c_double, C.c_double, C.c_uint32, C.c_uint64, C.POINTER(C.c_double)]
        _lib.qp_samples.restype = C.c_uint64
        _lib.qp_samples.argtypes = [C.POINTER(C.c_uint32), C.c_uint32, C.c_void_p, C.c_void_p]
        _lib.qp_psnr.restype = C.c_double
        _lib.qp_psnr.argtypes = [C.c_double, C.c_double]
    return _lib


def plan(psnr, dist, prec, samples):
    out = (C.c_double * 2)()
    ok = lib().qp_quality(psnr, dist, prec, samples, out)
    return bool(ok), out[0], out[1]


def samples(layout, sampling):
    area = (C.c_uint32 * 8)(layout.x0, layout.y0, layout.x1, layout.y1, layout.tx0, layout.ty0, layout.t_width, layout.t_height)
    if sampling is None:
        return lib().qp_samples(area, 3, None, None)
    dx = (C.c_uint8 * len(sampling))(*[a for a, _ in sampling])
    dy = (C.c_uint8 * len(sampling))(*[b for _, b in sampling])
    return lib().qp_samples(area, len(sampling), C.addressof(dx), C.addressof(dy))


@pytest.mark.parametrize("prec", [1, 8, 10, 12, 16])
@pytest.mark.parametrize("psnr", [0.5, 20.0, 30.0, 40.0, 50.0, 63.7, 120.0])
def test_budget_is_the_formula(psnr, prec):
    for S in (1, 128 * 128 * 3, 100 * 76 * 3, 4096 * 4096 * 3, (1 << 40) + 7):
        ok, D, signal = plan(psnr, 123.0, prec, S)            # (the distortion field is not read when a PSNR is given)
        peak = (1 << prec) - 1
        want = S * peak ** 2 * 10 ** (-psnr / 10)
        assert ok and abs(D - want) <= 1e-12 * want and signal == float(S * peak ** 2)
        assert abs(lib().qp_psnr(signal, D) - psnr) <= 1e-9


def test_infinite_psnr_and_a_distortion_of_the_callers():
    assert plan(math.inf, 5.0, 8, 1000) == (True, 0.0, 1000.0 * 255 * 255)
    assert plan(0.0, 5.5, 8, 1000) == (True, 5.5, 1000.0 * 255 * 255)
    assert plan(0.0, 0.0, 8, 1000)[:2] == (True, 0.0)
    assert plan(0.0, math.inf, 8, 1000)[:2] == (True, math.inf)
    assert lib().qp_psnr(100.0, 0.0) == math.inf and lib().qp_psnr(100.0, 100.0) == 0.0


def test_refusals():
    for psnr, dist, prec, S in ((-1.0, 0.0, 8, 100), (math.nan, 0.0, 8, 100), (-math.inf, 0.0, 8, 100), (0.0, -1.0, 8, 100),
                                (0.0, math.nan, 8, 100), (-0.5, 10.0, 8, 100), (30.0, 0.0, 0, 100), (30.0, 0.0, 17, 100), (30.0, 0.0, 8, 0)):
        assert plan(psnr, dist, prec, S) == (False, 0.0, 0.0), (psnr, dist, prec, S)
    assert plan(30.0, -1.0, 8, 100)[0] and plan(30.0, math.nan, 8, 100)[0]          # not read


S444 = None
S420 = [(1, 1), (2, 2), (2, 2)]
S422 = [(1, 1), (2, 1), (2, 1)]


@pytest.mark.parametrize("sampling", [S444, S420, S422], ids=["444", "420", "422"])
@pytest.mark.parametrize("area", [(128, 128, None, (0, 0)), (100, 76, (64, 48), (0, 0)), (251, 191, (128, 96), (0, 0)),
                                  (101, 77, (64, 48), (5, 3)), (1, 1, None, (0, 0)), (3, 5, None, (1, 1))],
                         ids=["128", "100x76-in-64x48", "251x191-odd", "off-origin", "one sample", "3x5 at 1,1"])
def test_samples_are_the_components_own(area, sampling):
    """S == the sum over tiles and components of the component's rectangle in the tile (grk_amd_layout_tile_comp): every component
    counts its own samples, however the area is tiled; 4:2:0 of an odd area rounds each component up, not the sum"""
    w, h, tile, off = area
    layout = G.ImageLayout.make(w, h, *(tile or (None, None)), offset=off)
    base = G.TileParams.make(1, 1, 3, 8, 2, mct=False)
    facs = sampling or [(1, 1)] * 3
    want = sum(tile_comp(layout, base, dx, dy, t).tile_w * tile_comp(layout, base, dx, dy, t).tile_h
               for t in range(num_tiles(layout)) for dx, dy in facs)
    ceil = lambda a, d: -(-a // d)
    closed = sum((ceil(off[0] + w, dx) - ceil(off[0], dx)) * (ceil(off[1] + h, dy) - ceil(off[1], dy)) for dx, dy in facs)
    assert samples(layout, sampling) == want == closed
    if sampling is None:
        assert want == 3 * w * h


def test_samples_refusals():
    layout = G.ImageLayout.make(16, 16)
    assert samples(layout, [(1, 1), (0, 1), (1, 1)]) == 0
    empty = G.ImageLayout.make(16, 16)
    empty.x1 = empty.x0
    assert samples(empty, None) == 0
