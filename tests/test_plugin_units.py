"""CPU: the parts of the Grok plugin that need no GPU -- the codestream / JP2 main-header reader, the PNM reader, the
grk_plugin_tile tree against the library's block layout, and the two mappings onto grk_amd_tile_params -- through the small
driver tests/c/plugin_units.cpp, built on first use with g++ together with the plugin's units (grok_amd/csrc/plugin*.cpp) and
linked against libgrok_amd.so.  -D_GLIBCXX_ASSERTIONS: an index past the end of a std::vector aborts instead of passing by luck."""
import ctypes as C
import glob
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import grok_amd as G
import j2kparse

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = sorted(glob.glob(os.path.join(HERE, "golden", "*.j2k")))
_lib = None


def lib():
    global _lib
    if _lib is None:
        G.lib()
        libdir = os.path.dirname(G.lib_path())
        out = os.path.join(tempfile.mkdtemp(prefix="plugin_units_"), "libplugin_units.so")
        units = sorted(glob.glob(os.path.join(ROOT, "grok_amd", "csrc", "plugin*.cpp")))
        assert len(units) == 5, units
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-D_GLIBCXX_ASSERTIONS", "-fPIC", "-shared",
                               "-I", os.path.join(ROOT, "include"), os.path.join(HERE, "c", "plugin_units.cpp")] + units +
                              ["-o", out, "-L" + libdir, "-lgrok_amd", "-Wl,-rpath," + libdir, "-ldl", "-lpthread"])
        _lib = C.CDLL(out)
    return _lib


def u32(*v):
    return np.array(v, np.uint32)


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


# ---- read_stream_header ---------------------------------------------------------------------------------------------

def read_header(data):
    """-> None (declined) or dict(file_size, guard, qstyle, overrides, words)"""
    fd, path = tempfile.mkstemp(suffix=".bin")
    with os.fdopen(fd, "wb") as f:
        f.write(bytes(data))
    try:
        out, words = np.zeros(5, np.uint64), np.zeros(512, np.uint16)
        if not lib().pu_read_stream_header(path.encode(), ptr(out), ptr(words), 512):
            return None
        return dict(file_size=int(out[0]), guard=int(out[1]), qstyle=int(out[2]), overrides=bool(out[3]),
                    words=[int(w) for w in words[:int(out[4])]])
    finally:
        os.unlink(path)


def segments(cs, pos=2):
    """[(marker, position, Lxx)] of the marker segments from pos up to SOT / SOD (T.800 A.1.3: marker, 16-bit length that counts itself)"""
    out = []
    while True:
        m, = struct.unpack(">H", cs[pos:pos + 2])
        if m in (0xFF90, 0xFF93):
            return out, pos
        ln, = struct.unpack(">H", cs[pos + 2:pos + 4])
        out.append((m, pos, ln))
        pos += 2 + ln


def qcd_of(cs):
    """(guard bits, style, SPqcd words) read from the stream's QCD by the test itself (A.6.4)"""
    for m, pos, ln in segments(cs)[0]:
        if m == 0xFF5C:
            body = cs[pos + 4:pos + 2 + ln]
            style = body[0] & 0x1F
            words = list(body[1:]) if style == 0 else list(struct.unpack(">%dH" % ((len(body) - 1) // 2), body[1:]))
            return body[0] >> 5, style, words
    raise AssertionError("no QCD")


def box(kind, payload, xl=False):
    if xl:
        return struct.pack(">I4sQ", 1, kind, 16 + len(payload)) + payload
    return struct.pack(">I4s", 8 + len(payload), kind) + payload


def jp2(cs, xl):
    return box(b"jP  ", b"\r\n\x87\n") + box(b"ftyp", b"jp2 \0\0\0\0jp2 ", xl) + box(b"jp2c", cs, xl)


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p) for p in GOLDEN])
def test_stream_header_of_every_golden_stream(path):
    cs = open(path, "rb").read()
    guard, style, words = qcd_of(cs)
    try:                                        # (the test-side parser takes single-tile streams only)
        info = j2kparse.parse(cs)
    except AssertionError:
        info = None
    if info is not None:
        assert guard == info["guard"]
        assert [((w >> 3, 0) if style == 0 else (w >> 11, w & 0x7FF)) for w in words] == info["qcd"]
    want = dict(file_size=len(cs), guard=guard, qstyle=style, overrides=False, words=words)
    assert read_header(cs) == want
    for xl in (False, True):
        wrapped = jp2(cs, xl)
        assert read_header(wrapped) == dict(want, file_size=len(wrapped)), "JP2, XLBox=%s" % xl


def test_stream_header_declines_damaged_input():
    cs = open(GOLDEN[0], "rb").read()
    assert read_header(b"") is None
    assert read_header(cs[:1]) is None
    sig, ftyp, body = box(b"jP  ", b"\r\n\x87\n"), b"jp2 \0\0\0\0jp2 ", box(b"jp2c", cs)
    assert read_header(sig + box(b"ftyp", ftyp) + body) is not None
    assert read_header(sig + struct.pack(">I4s", 4, b"ftyp") + ftyp + body) is None              # a box shorter than its header
    assert read_header(sig + struct.pack(">I4sQ", 1, b"ftyp", 8) + ftyp + body) is None          # ... in the XLBox form
    assert read_header(sig + struct.pack(">I4s", 0x7FFFFFFF, b"ftyp") + ftyp + body) is None     # a box past the end of the file
    assert read_header(sig + struct.pack(">I4sQ", 1, b"ftyp", 1 << 62) + ftyp + body) is None
    assert read_header(sig + box(b"ftyp", ftyp)) is None                                         # no codestream box
    assert read_header(sig + box(b"ftyp", ftyp) + struct.pack(">I", 1)) is None                  # cut inside a box header
    segs, _ = segments(cs)
    pos = {m: (p, ln) for m, p, ln in segs}
    cod, qcd = pos[0xFF52], pos[0xFF5C]
    assert read_header(cs[:cod[0] + 2 + cod[1] - 1]) is None        # a marker segment whose length runs past the end
    assert read_header(cs[:qcd[0] + 3]) is None                     # cut inside the QCD: in its length, ...
    assert read_header(cs[:qcd[0] + 5]) is None                     # ... after Sqcd
    assert read_header(cs[:qcd[0] + 2 + qcd[1] - 1]) is None        # ... a byte short
    assert read_header(cs[:qcd[0] + 2 + qcd[1]]) is not None        # (all of the QCD, nothing after it: enough)
    assert read_header(cs[:qcd[0]]) is None                         # no QCD at all
    assert read_header(b"\xff\x4e" + cs[2:]) is None                # no SOC


@pytest.mark.parametrize("marker", [0xFF5D, 0xFF53, 0xFF5E, 0xFF5F], ids=["QCC", "COC", "RGN", "POC"])
def test_stream_header_flags_main_header_overrides(marker):
    cs = open(GOLDEN[0], "rb").read()
    qcd = [p for m, p, _ in segments(cs)[0] if m == 0xFF5C][0]
    seg = struct.pack(">HH", marker, 2 + 5) + b"\0\1\2\3\4"
    for at in (qcd, segments(cs)[1]):                               # before the QCD, and last in the main header
        h = read_header(cs[:at] + seg + cs[at:])
        assert h is not None and h["overrides"] and h["words"] == qcd_of(cs)[2]


@pytest.mark.parametrize("marker", [0xFF52, 0xFF5C, 0xFF53, 0xFF5D], ids=["COD", "QCD", "COC", "QCC"])
def test_stream_header_flags_tile_part_overrides(marker):
    cs = open(GOLDEN[0], "rb").read()
    sot = segments(cs)[1]
    assert cs[sot:sot + 4] == b"\xff\x90\x00\x0a" and cs[sot + 12:sot + 14] == b"\xff\x93"
    seg = struct.pack(">HH", marker, 2 + 5) + b"\0\1\2\3\4"
    h = read_header(cs[:sot + 12] + seg + cs[sot + 12:])
    assert h is not None and h["overrides"]
    assert read_header(cs)["overrides"] is False


# ---- read_pnm ---------------------------------------------------------------------------------------------------------

def read_pnm(data):
    fd, path = tempfile.mkstemp(suffix=".pnm")
    with os.fdopen(fd, "wb") as f:
        f.write(data)
    try:
        dims, out = np.zeros(5, np.uint32), np.zeros(1 << 20, np.uint8)
        if not lib().pu_read_pnm(path.encode(), ptr(dims), ptr(out), out.size):
            return None
        w, h, comps, prec, nbytes = (int(v) for v in dims)
        px = out[:nbytes].view(np.uint16 if prec > 8 else np.uint8)
        return prec, px.reshape(comps, h, w).copy()
    finally:
        os.unlink(path)


@pytest.mark.parametrize("comps,maxval", [(1, 255), (3, 255), (1, 65535), (3, 4095), (1, 1), (3, 256)])
def test_pnm_reader(comps, maxval):
    w, h = 37, 21
    rng = np.random.default_rng(comps * 100000 + maxval)
    img = rng.integers(0, maxval + 1, (h, w, comps)).astype(np.uint16)
    raster = img.astype(">u2").tobytes() if maxval > 255 else img.astype(np.uint8).tobytes()
    head = b"P%d\n# made by the test\n%d # columns\n#\n%d\n# maxval follows\n%d\n" % (6 if comps == 3 else 5, w, h, maxval)
    got = read_pnm(head + raster)
    assert got is not None
    prec, px = got
    assert prec == int(maxval).bit_length()
    assert np.array_equal(px, img.transpose(2, 0, 1))
    assert read_pnm(head + raster[:-1]) is None                     # a truncated raster
    assert read_pnm(head[:-1]) is None


@pytest.mark.parametrize("head", [b"P5\n4 4\n0\n", b"P5\n4 4\n65536\n", b"P4\n4 4\n255\n", b"P5\n0 4\n255\n", b"P5\n4\n", b""])
def test_pnm_reader_refuses(head):
    assert read_pnm(head + b"\0" * 64) is None


# ---- the tree of make_owner against grk_amd_tile_layout ---------------------------------------------------------------

def comp_params(p, dx, dy):
    """the rectangle of a component sub-sampled by dx, dy in tile p (grk_amd_layout_tile_comp), one component, no MCT"""
    im = G.ImageLayout(p.tile_x0, p.tile_y0, p.tile_x0 + p.tile_w, p.tile_y0 + p.tile_h, p.tile_x0, p.tile_y0, p.tile_w, p.tile_h)
    out = G.TileParams()
    assert G.lib().grk_amd_layout_tile_comp(C.byref(im), C.byref(p), dx, dy, 0, C.byref(out)) == 0
    out.num_comps, out.mct = 1, 0
    return out


def precincts(p):
    counts = (C.c_uint32 * (p.num_levels + 1))()
    G.lib().grk_amd_tile_precincts(C.byref(p), counts)
    return list(counts)


TREES = {
    "plain": (G.TileParams.make(256, 192, 3, 8, 3), None),
    "irreversible": (G.TileParams.make(200, 120, 3, 12, 2, irreversible=True), None),
    "precincts": (G.TileParams.make(300, 260, 1, 8, 3, precincts=[(5, 5), (6, 5), (6, 6), (7, 7)]), None),
    "origin off the block grid": (G.TileParams.make(150, 97, 3, 8, 3, cblk=(5, 4), origin=(37, 19)), None),
    "precincts off the grid": (G.TileParams.make(170, 130, 1, 8, 2, origin=(45, 70), precincts=[(4, 5), (5, 5), (6, 6)]), None),
    "empty resolutions": (G.TileParams.make(5, 3, 1, 8, 6), None),
    "empty resolutions off the origin": (G.TileParams.make(3, 2, 3, 8, 5, origin=(8, 16)), None),
    "4:2:0": (G.TileParams.make(255, 131, 3, 8, 3, mct=False), [(1, 1), (2, 2), (2, 2)]),
    "4:2:2 + alpha": (G.TileParams.make(190, 90, 4, 10, 2, mct=False, origin=(3, 5), precincts=[(5, 5), (6, 6), (6, 6)]),
                      [(1, 1), (2, 1), (2, 1), (1, 1)]),
    "4:2:0, five levels on a small tile": (G.TileParams.make(9, 7, 3, 8, 5, mct=False), [(1, 1), (2, 2), (2, 2)]),
}


@pytest.mark.parametrize("name", sorted(TREES))
def test_tile_tree_walk_is_the_layout(name):
    p, factors = TREES[name]
    L = p.num_levels
    cps = [comp_params(p, dx, dy) for dx, dy in factors] if factors else None
    want, nprec = [], []
    for c, pc in enumerate(cps if cps else [p]):
        for b in G.tile_layout(pc)[0]:
            want.append((b.x0, b.y0, b.x1, b.y1, c if cps else b.comp, b.res, b.band, b.precinct, b.stepsize))
    for c in range(p.num_comps):
        nprec.append(precincts(cps[c] if cps else p))
    assert len({w[4] for w in want}) == p.num_comps
    nbands = p.num_comps * (3 * L + 1)
    blocks, bands = np.zeros((len(want) + 1, 8), np.uint32), np.zeros((nbands + 1, 5), np.uint32)
    steps, counts = np.zeros(nbands + 1, np.float32), np.zeros(5, np.uint64)
    arr = (G.TileParams * p.num_comps)(*cps) if cps else None
    assert lib().pu_walk_tree(C.byref(p), arr, ptr(blocks), C.c_uint64(len(blocks)), ptr(bands), ptr(steps), C.c_uint64(len(bands)),
                              ptr(counts)) == 1
    # the walk visits exactly the layout's rectangles, in the layout's order
    assert int(counts[4]) == len(want)
    assert [tuple(int(v) for v in row) for row in blocks[:len(want)]] == [w[:8] for w in want]
    # components, resolutions, bands; precincts as grk_amd_tile_precincts counts them (a resolution without samples keeps one
    # empty entry per band, so that the arrays stay well-formed)
    assert [int(v) for v in counts[:3]] == [p.num_comps, p.num_comps * (L + 1), nbands]
    first, j, total = 0, 0, 0
    for c in range(p.num_comps):
        for r in range(L + 1):
            for orient in ([0] if r == 0 else [1, 2, 3]):
                bc, br, bo, bn, nblk = (int(v) for v in bands[j])
                assert (bc, br, bo) == (c, r, orient)
                assert bn == max(nprec[c][r], 1)
                if nprec[c][r] == 0:
                    assert nblk == 0
                assert nblk == sum(1 for w in want if (w[4], w[5], w[6]) == (c, r, orient))
                assert float(steps[j]) == (want[first][8] if nblk else 1.0), "band stepsize = its first block's"
                first, j, total = first + nblk, j + 1, total + bn
    assert int(counts[3]) == total


def test_tile_tree_declines_what_the_layout_declines():
    p = G.TileParams.make(64, 64, 3, 8, 2)
    p.tile_w = 0
    assert lib().pu_walk_tree(C.byref(p), None, None, C.c_uint64(0), None, None, C.c_uint64(0), None) == 0


# ---- gra_cparameters -> grk_amd_tile_params ----------------------------------------------------------------------------------

def from_cparameters(w, h, comps, prec, multi=False, prcw=(), prch=(), **kw):
    f = dict(isHT=1, cblk_sty=0x40, tile_size_on=0, tx0=0, ty0=0, t_width=0, t_height=0, numpocs=0, roi_compno=-1, dx=1, dy=1,
             off_x=0, off_y=0, numresolution=6, irreversible=0, tcp_mct=255, cblockw=64, cblockh=64, csty=0, res_spec=0, layers=1)
    assert set(kw) <= set(f), kw
    f.update(kw)
    cfg = u32(f["isHT"], f["cblk_sty"], f["tile_size_on"], f["tx0"], f["ty0"], f["t_width"], f["t_height"], f["numpocs"],
              f["roi_compno"] + 1, f["dx"], f["dy"], f["off_x"], f["off_y"], f["numresolution"], f["irreversible"], f["tcp_mct"],
              f["cblockw"], f["cblockh"], f["csty"], f["res_spec"], f["layers"])
    pw, ph = np.zeros(33, np.uint32), np.zeros(33, np.uint32)
    pw[:len(prcw)], ph[:len(prch)] = prcw, prch
    p = G.TileParams()
    ok = lib().pu_params_from_cparameters(ptr(cfg), ptr(pw), ptr(ph), ptr(u32(w, h, comps, prec, int(multi))), C.byref(p))
    return p if ok else None


def test_cparameters_defaults_and_mct_not_set():
    p = from_cparameters(640, 480, 3, 8)
    assert (p.tile_w, p.tile_h, p.num_comps, p.prec, p.sgnd, p.irreversible) == (640, 480, 3, 8, 0, 0)
    assert (p.num_levels, p.cblk_w_exp, p.cblk_h_exp, p.tile_x0, p.tile_y0) == (5, 6, 6, 0, 0)
    assert list(p.precinct_exp) == [0] * 12
    # tcp_mct == 255 is "not set": the colour transform for three or more components
    assert p.mct == 1 and from_cparameters(640, 480, 1, 8).mct == 0 and from_cparameters(640, 480, 2, 8).mct == 0
    assert from_cparameters(640, 480, 3, 8, tcp_mct=0).mct == 0 and from_cparameters(640, 480, 4, 8, tcp_mct=1).mct == 1
    assert from_cparameters(640, 480, 3, 8, tcp_mct=2) is None                    # custom array MCT
    assert from_cparameters(640, 480, 3, 8, isHT=0) is None and from_cparameters(640, 480, 3, 8, cblk_sty=0) is None
    assert from_cparameters(640, 480, 3, 8, numresolution=0) is None and from_cparameters(640, 480, 3, 8, numresolution=12) is None
    assert from_cparameters(640, 480, 3, 8, cblockw=32, cblockh=16).cblk_h_exp == 4


def test_cparameters_precinct_list_expansion():
    """grk_compress -c: sizes from the highest resolution down, the last one halved for the resolutions beyond the list,
    exponent = floor(log2) (CodeStreamCompress.cpp:475-514)"""
    numres, prcw, prch = 6, [256, 128], [256, 64]
    p = from_cparameters(1000, 700, 3, 8, numresolution=numres, csty=1, res_spec=2, prcw=prcw, prch=prch)
    want = [0] * 12
    for q in range(numres):
        pw = prcw[q] if q < len(prcw) else prcw[-1] >> (q - (len(prcw) - 1))
        ph = prch[q] if q < len(prch) else prch[-1] >> (q - (len(prch) - 1))
        want[numres - 1 - q] = (pw.bit_length() - 1) | ((ph.bit_length() - 1) << 4)
    assert want[:6] == [3 | 2 << 4, 4 | 3 << 4, 5 | 4 << 4, 6 | 5 << 4, 7 | 6 << 4, 8 | 8 << 4]
    assert list(p.precinct_exp) == want
    # a size that is no power of two: floor
    p = from_cparameters(1000, 700, 3, 8, numresolution=2, csty=1, res_spec=2, prcw=[300, 100], prch=[255, 64])
    assert list(p.precinct_exp)[:2] == [6 | 6 << 4, 8 | 7 << 4]
    # csty without the precinct bit, or an empty list: one precinct per resolution
    assert list(from_cparameters(1000, 700, 3, 8, csty=0, res_spec=2, prcw=prcw, prch=prch).precinct_exp) == [0] * 12
    # the 1 x 1 precinct (exponent byte 0 = "not set" in grk_amd_tile_params) is the host's own business
    assert from_cparameters(1000, 700, 3, 8, numresolution=1, csty=1, res_spec=1, prcw=[1], prch=[1]) is None
    assert from_cparameters(1000, 700, 3, 8, numresolution=3, csty=1, res_spec=1, prcw=[2], prch=[2]) is None
    assert from_cparameters(1000, 700, 3, 8, numresolution=1, csty=1, res_spec=1, prcw=[65536], prch=[64]) is None


def test_cparameters_offsets_and_subsampling():
    p = from_cparameters(100, 80, 3, 8, dx=2, dy=3, off_x=4, off_y=9)
    assert (p.tile_x0, p.tile_y0, p.tile_w, p.tile_h) == (2, 3, 100, 80)          # ceil(offset / d), the file's samples
    assert from_cparameters(100, 80, 3, 8, dx=2, dy=3, off_x=3, off_y=9) is None   # not a multiple of the factor
    assert from_cparameters(100, 80, 3, 8, dx=2, dy=3, off_x=4, off_y=10) is None
    assert from_cparameters(100, 80, 3, 8, dx=0) is None and from_cparameters(100, 80, 3, 8, dy=256) is None
    # one tile: the grid cell must cover the image area, (w - 1) dx + 1 wide on the reference grid
    assert from_cparameters(100, 80, 1, 8, tile_size_on=1, t_width=100, t_height=80) is not None
    assert from_cparameters(100, 80, 1, 8, tile_size_on=1, t_width=99, t_height=80) is None
    assert from_cparameters(100, 80, 1, 8, tile_size_on=1, t_width=199, t_height=80, dx=2) is not None
    assert from_cparameters(100, 80, 1, 8, tile_size_on=1, t_width=198, t_height=80, dx=2) is None
    # several tiles: the base parameters, tile size clipped to the image, no sub-sampling, one layer
    p = from_cparameters(100, 80, 1, 8, multi=True, tile_size_on=1, t_width=64, t_height=128)
    assert (p.tile_w, p.tile_h, p.tile_x0, p.tile_y0) == (64, 80, 0, 0)
    assert from_cparameters(100, 80, 1, 8, multi=True, tile_size_on=1, t_width=64, t_height=64, dx=2) is None
    assert from_cparameters(100, 80, 1, 8, multi=True, tile_size_on=1, t_width=64, t_height=64, layers=2) is None
    assert from_cparameters(100, 80, 1, 8, numpocs=1) is None and from_cparameters(100, 80, 1, 8, roi_compno=0) is None


# ---- the host's main header -> grk_amd_tile_params -----------------------------------------------------------------------------

def ceil_div(a, b):
    return -(-a // b)


def from_header(bounds, comps, reduce=0, prcw=(), prch=(), **kw):
    """comps = [(dx, dy, w, h, x0, y0, prec, sgnd)] -> None (declined) or (tp, alike, cps[4], cdx, cdy)"""
    f = dict(cblockw=64, cblockh=64, irreversible=0, mct=0, numresolutions=6, csty=0, cblk_sty=0x40, tgw=1, tgh=1)
    assert set(kw) <= set(f), kw
    f.update(kw)
    hdr = u32(f["cblockw"], f["cblockh"], f["irreversible"], f["mct"], f["numresolutions"], f["csty"], f["cblk_sty"], f["tgw"], f["tgh"])
    pw, ph = np.zeros(33, np.uint32), np.zeros(33, np.uint32)
    pw[:len(prcw)], ph[:len(prch)] = prcw, prch
    cs = np.array(comps, np.uint32).reshape(-1, 8)
    tp, alike, cps = G.TileParams(), C.c_int(-1), (G.TileParams * 4)()
    cdx, cdy = np.zeros(4, np.uint8), np.zeros(4, np.uint8)
    ok = lib().pu_tile_params_from_header(ptr(hdr), ptr(pw), ptr(ph), ptr(u32(*bounds)), len(cs), ptr(cs), int(reduce), C.byref(tp),
                                          C.byref(alike), cps, ptr(cdx), ptr(cdy))
    return (tp, bool(alike.value), list(cps), list(cdx), list(cdy)) if ok else None


def full_comps(bounds, factors, prec=8, sgnd=0, reduce=0):
    """the components the host reports for an image with these bounds: [ceil(x0 / d), ceil(x1 / d)), at 1 / 2^reduce"""
    out = []
    for dx, dy in factors:
        x0, y0, x1, y1 = ceil_div(bounds[0], dx), ceil_div(bounds[1], dy), ceil_div(bounds[2], dx), ceil_div(bounds[3], dy)
        s = 1 << reduce
        rx0, ry0, rx1, ry1 = ceil_div(x0, s), ceil_div(y0, s), ceil_div(x1, s), ceil_div(y1, s)
        out.append((dx, dy, rx1 - rx0, ry1 - ry0, rx0, ry0, prec, sgnd))
    return out


def test_header_components_alike():
    bounds = (0, 0, 640, 480)
    tp, alike, _, cdx, cdy = from_header(bounds, full_comps(bounds, [(1, 1)] * 3, prec=12, sgnd=1), mct=1, numresolutions=4,
                                         cblockw=32, cblockh=128)
    assert alike and (cdx, cdy) == ([1] * 4, [1] * 4)
    assert (tp.tile_w, tp.tile_h, tp.tile_x0, tp.tile_y0, tp.num_comps, tp.prec, tp.sgnd) == (640, 480, 0, 0, 3, 12, 1)
    assert (tp.irreversible, tp.mct, tp.num_levels, tp.cblk_w_exp, tp.cblk_h_exp) == (0, 1, 3, 5, 7)
    assert list(tp.reserved)[:2] == [0, 0] and list(tp.precinct_exp) == [0] * 12            # HT blocks
    # classic blocks: reserved[0] = 1, [1] = the style bits; irreversible goes with them only
    tp = from_header(bounds, full_comps(bounds, [(1, 1)]), cblk_sty=0x22, irreversible=1)[0]
    assert list(tp.reserved)[:2] == [1, 0x22] and tp.irreversible == 1
    assert from_header(bounds, full_comps(bounds, [(1, 1)]), cblk_sty=0x40, irreversible=1) is None
    assert from_header(bounds, full_comps(bounds, [(1, 1)]), cblk_sty=0x01) is None        # LAZY / TERMALL: several segments
    assert from_header(bounds, full_comps(bounds, [(1, 1)]), cblk_sty=0x04) is None
    assert from_header(bounds, full_comps(bounds, [(1, 1)]), tgw=2) is None                # several tiles
    assert from_header(bounds, [], numresolutions=3) is None
    # all components sub-sampled alike: one geometry, the component rectangle at ceil(offset / d)
    b2 = (6, 9, 207, 100)
    tp, alike = from_header(b2, full_comps(b2, [(2, 3)] * 2))[:2]
    assert alike and (tp.tile_x0, tp.tile_y0, tp.tile_w, tp.tile_h) == (3, 3, 104 - 3, 34 - 3)
    # one precision and signedness
    mixed = full_comps(bounds, [(1, 1)] * 2)
    mixed[1] = mixed[1][:6] + (10, 0)
    assert from_header(bounds, mixed) is None
    assert from_header(bounds, full_comps(bounds, [(1, 1)], prec=17)) is None
    assert from_header(bounds, full_comps(bounds, [(256, 1)])) is None


def test_header_precincts():
    bounds = (0, 0, 640, 480)
    comps = full_comps(bounds, [(1, 1)])
    prcw, prch = [32, 64, 128, 32768], [64, 64, 256, 32768]
    tp = from_header(bounds, comps, numresolutions=4, csty=1, prcw=prcw, prch=prch)[0]
    want = [(w.bit_length() - 1) | ((h.bit_length() - 1) << 4) for w, h in zip(prcw, prch)]
    assert want == [5 | 6 << 4, 6 | 6 << 4, 7 | 8 << 4, 15 | 15 << 4]
    assert list(tp.precinct_exp) == want + [0] * 8
    assert list(from_header(bounds, comps, numresolutions=4, csty=0, prcw=prcw, prch=prch)[0].precinct_exp) == [0] * 12
    assert from_header(bounds, comps, numresolutions=2, csty=1, prcw=[1, 64], prch=[1, 64]) is None      # the 1 x 1 precinct
    assert from_header(bounds, comps, numresolutions=2, csty=1, prcw=[1, 64], prch=[2, 64]) is not None
    assert from_header(bounds, comps, numresolutions=2, csty=1, prcw=[64, 65536], prch=[64, 64]) is None


def test_header_reduce():
    bounds = (5, 3, 645, 483)
    for reduce in (0, 1, 3):
        tp, alike = from_header(bounds, full_comps(bounds, [(1, 1)] * 3, reduce=reduce), reduce=reduce, numresolutions=4)[:2]
        # the tree is the FULL tile's, whatever the host's components are reduced to
        assert alike and (tp.tile_x0, tp.tile_y0, tp.tile_w, tp.tile_h, tp.num_levels) == (5, 3, 640, 480, 3)
    assert from_header(bounds, full_comps(bounds, [(1, 1)] * 3, reduce=3), reduce=4, numresolutions=4) is None     # reduce >= numresolutions
    assert from_header(bounds, full_comps(bounds, [(1, 1)] * 3, reduce=4), reduce=4, numresolutions=4) is None
    assert from_header(bounds, full_comps(bounds, [(1, 1)] * 3), reduce=0, numresolutions=0) is None
    # a component that is not the rectangle the reduced tile covers is left to the host
    comps = full_comps(bounds, [(1, 1)], reduce=2)
    wider = [comps[0][:2] + (comps[0][2] + 1,) + comps[0][3:]]
    assert from_header(bounds, comps, reduce=2) is not None and from_header(bounds, wider, reduce=2) is None


def test_header_components_each_in_its_own_way():
    bounds = (3, 5, 258, 136)
    factors = [(1, 1), (2, 2), (2, 2), (1, 2)]
    got = from_header(bounds, full_comps(bounds, factors), numresolutions=3)
    tp, alike, cps, cdx, cdy = got
    assert not alike and (cdx, cdy) == ([1, 2, 2, 1], [1, 2, 2, 2])
    # the tile on the reference grid; every component its own rectangle, one component, no colour transform
    assert (tp.tile_x0, tp.tile_y0, tp.tile_w, tp.tile_h, tp.num_comps, tp.mct) == (3, 5, 255, 131, 4, 0)
    for (dx, dy), pc in zip(factors, cps):
        x0, y0, x1, y1 = ceil_div(3, dx), ceil_div(5, dy), ceil_div(258, dx), ceil_div(136, dy)
        assert (pc.tile_x0, pc.tile_y0, pc.tile_w, pc.tile_h, pc.num_comps, pc.mct, pc.num_levels) == (x0, y0, x1 - x0, y1 - y0, 1, 0, 2)
    assert from_header(bounds, full_comps(bounds, factors), numresolutions=3, mct=1) is None       # a transform across sizes
    assert from_header(bounds, full_comps(bounds, factors + [(1, 1)]), numresolutions=3) is None   # more than four
    assert from_header(bounds, full_comps(bounds, factors, reduce=1), reduce=1, numresolutions=3) is not None
    comps = full_comps(bounds, factors)
    comps[1] = comps[1][:3] + (comps[1][3] - 1,) + comps[1][4:]                                     # not what SIZ implies
    assert from_header(bounds, comps, numresolutions=3) is None
