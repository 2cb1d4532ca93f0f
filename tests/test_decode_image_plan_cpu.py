"""CPU: the host planning of the whole-image decodes (grok_amd/csrc/decode_image_plan.cpp, the staging plan of surface_plan.cpp)
through the small driver tests/c/decode_image_plan_units.cpp, built on first use with g++ from the library's HIP-free sources only
(-Wl,--no-undefined: that it links is the test that the planner and what it stands on need no HIP).  -D_GLIBCXX_ASSERTIONS: an
index past the end of a std::vector aborts.

The streams are made here on the CPU: block lengths and bytes are random, so no GPU and no reference are needed.  A, A1, C, C1 come
from the library's writers.  Those write one layer and one HT pass per block, so the two streams that need more -- A2 (Part-1, two
layers with most blocks in both: the reader produces moves and an appendix) and P (Part-1, TERMALL: a codeword segment per pass,
the decode needs the segment lists) -- get their tile-parts from a small packet writer below (LRCP, one precinct per resolution,
every block included in the first layer with no zero bit-plane) behind the library's main header with COD patched.

What is covered exactly once: in every layout used here except the pitched one every byte of the destination is a sample, so the
painted map is all ones; the pitched case computes the sample bytes from the resolved layout and holds the gaps at zero."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import grok_amd as G
from grok_amd.capi import CODED_DTYPE, MOVE_DTYPE, SEGMENT_DTYPE, ERR_INVALID, ERR_OVERFLOW, ERR_UNSUPPORTED
from test_t2_reader_subsampled_cpu import S420, tile_comp, write_subsampled

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DIRECT, REGION, RUNS, STAGED, SURFACE = range(5)
NO_CAP = (1 << 64) - 1
_lib = None


def lib():
    global _lib
    if _lib is None:
        csrc = os.path.join(ROOT, "grok_amd", "csrc")
        out = os.path.join(tempfile.mkdtemp(prefix="decode_image_plan_units_"), "libdecode_image_plan_units.so")
        srcs = ["decode_image_plan.cpp", "image_view_plan.cpp", "surface_plan.cpp", "t2_reader.cpp", "t2_writer.cpp", "geometry.cpp", "host_common.cpp"]
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-D_GLIBCXX_ASSERTIONS", "-fPIC", "-shared",
                               os.path.join(HERE, "c", "decode_image_plan_units.cpp")] + [os.path.join(csrc, s) for s in srcs] +
                              ["-o", out, "-Wl,--no-undefined", "-lpthread"])
        _lib = C.CDLL(out)
        _lib.dip_reason.restype = C.c_char_p
    return _lib


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


# ---- the streams ---------------------------------------------------------------------------------------------------------------
def random_table(n, seed):
    rng = np.random.default_rng(seed)
    t = np.zeros(n, CODED_DTYPE)
    t["length"] = rng.integers(1, 40, n)
    t["offset"] = np.concatenate([[0], np.cumsum(t["length"])[:-1]])
    return t, rng.integers(0, 255, int(t["length"].sum()), dtype=np.uint8)          # (no 0xFF: nothing that looks like a marker)


def plain_stream(W, H, TW, TH, off, seed=1):
    layout = G.ImageLayout.make(W, H, TW, TH, offset=off)
    base = G.TileParams.make(TW, TH, 3, 8, 3)
    n = sum(G.lib().grk_amd_tile_num_blocks(p) for p in G.layout_tiles(layout, base))
    return G.write_codestream_layout(layout, base, *random_table(n, seed))


def sub_stream(W, H, TW, TH, off=(0, 0), seed=2):
    layout = G.ImageLayout.make(W, H, TW, TH, offset=off)
    base = G.TileParams.make(TW, TH, 3, 8, 3, mct=False)
    nt = G.lib().grk_amd_layout_num_tiles(C.byref(layout))
    n = sum(G.lib().grk_amd_tile_num_blocks(tile_comp(layout, base, dx, dy, t)) for t in range(nt) for dx, dy in S420)
    return write_subsampled(layout, base, S420, *random_table(n, seed), 0)


class HeaderBits:
    """a packet header's bits, MSB first, a byte behind 0xFF carrying 7 (B.10.1)"""

    def __init__(self):
        self.out, self.cur, self.n, self.cap = bytearray(), 0, 0, 8

    def put(self, v, k):
        for i in reversed(range(k)):
            self.cur = self.cur << 1 | (v >> i & 1)
            self.n += 1
            if self.n == self.cap:
                self.out.append(self.cur)
                self.cap = 7 if self.cur == 0xFF else 8
                self.cur = self.n = 0

    def done(self):
        if self.n:
            self.out.append(self.cur << (self.cap - self.n))
        if self.out and self.out[-1] == 0xFF:
            self.out.append(0)
        return bytes(self.out)


def put_passes(hb, n):          # Table B.4
    if n == 1:
        hb.put(0, 1)
    elif n == 2:
        hb.put(2, 2)
    elif n <= 5:
        hb.put(3, 2), hb.put(n - 3, 2)
    else:
        assert n <= 36
        hb.put(15, 4), hb.put(n - 6, 5)


def part1_stream(W, H, TW, TH, off, layers, termall, seed):
    """-> (codestream, per block in table order [[(bytes, passes) per codeword segment]]): Part-1 blocks of random bytes, every block
    in layer 0, most again in the later layers"""
    rng = np.random.default_rng(seed)
    layout = G.ImageLayout.make(W, H, TW, TH, offset=off)
    base = G.TileParams.make(TW, TH, 3, 8, 3)
    head = bytearray(G.write_codestream_layout(layout, base, np.zeros(1 << 12, CODED_DTYPE), np.zeros(1, np.uint8)))
    head = head[:head.index(b"\xff\x90")]
    c = head.index(b"\xff\x52")
    head[c + 6:c + 8] = layers.to_bytes(2, "big")
    head[c + 12] = 0x04 if termall else 0x00                    # SPcod code-block style: no HT bit -> Part-1
    out, all_segs = bytearray(head), []
    for t, p in enumerate(G.layout_tiles(layout, base)):
        blocks, _ = G.tile_layout(p)
        nb = len(blocks) // 3
        # the bands' grids, comp 0: {(res, band): (first block, gw, gh)} -- raster order within a band
        grids = {}
        for i, b in enumerate(blocks[:nb]):
            first, gw, n = grids.get((b.res, b.band), (i, 0, 0))
            grids[(b.res, b.band)] = (first, gw + (b.y0 == blocks[first].y0), n + 1)
        state = [dict(lblock=3, open=0, segs=[]) for _ in blocks]           # open: passes of a segment that the next layer continues
        body = bytearray()
        for layer in range(layers):
            for r in range(base.num_levels + 1):
                assert any(k[0] == r for k in grids), "a resolution without blocks has no packet: not written here"
                for comp in range(3):
                    hb, data = HeaderBits(), bytearray()
                    hb.put(1, 1)
                    for (res, band), (first, gw, n) in sorted(grids.items()):
                        if res != r:
                            continue
                        seen = set()
                        for k in range(n):
                            s = state[comp * nb + first + k]
                            x, y, lev, new = k % gw, k // gw, 0, 0
                            while True:                                   # the tag tree's nodes first met on the way to this leaf
                                new += (lev, x >> lev, y >> lev) not in seen
                                seen.add((lev, x >> lev, y >> lev))
                                if ((gw - 1) >> lev) == 0 and ((n // gw - 1) >> lev) == 0:
                                    break
                                lev += 1
                            if layer == 0:
                                hb.put((1 << 2 * new) - 1, 2 * new)       # included in layer 0, no zero bit-plane: every new node's value is 0
                            else:
                                go = rng.random() < 0.7
                                hb.put(int(go), 1)
                                if not go:
                                    continue
                            npass = int(rng.integers(1, 5))
                            put_passes(hb, npass)
                            if termall:
                                chunks = [(1, int(rng.integers(1, 30))) for _ in range(npass)]
                            else:
                                chunks = [(npass, int(rng.integers(1, 60)))]
                            need = max(ln.bit_length() - (k_.bit_length() - 1) for k_, ln in chunks)
                            inc = max(0, need - s["lblock"])
                            hb.put((1 << inc + 1) - 2, inc + 1)
                            s["lblock"] += inc
                            for k_, ln in chunks:
                                hb.put(ln, s["lblock"] + k_.bit_length() - 1)
                                if s["open"]:
                                    s["segs"][-1] = (s["segs"][-1][0] + ln, s["segs"][-1][1] + k_)
                                else:
                                    s["segs"].append((ln, k_))
                                data += rng.integers(0, 255, ln, dtype=np.uint8).tobytes()
                            s["open"] = 0 if termall else 1
                    body += hb.done() + data
        out += b"\xff\x90" + (10).to_bytes(2, "big") + t.to_bytes(2, "big") + (14 + len(body)).to_bytes(4, "big") + b"\x00\x01\xff\x93" + body
        all_segs += [s["segs"] for s in state]
    return bytes(out + b"\xff\xd9"), all_segs


_streams = {}


def stream(name):
    if name not in _streams:
        _streams[name] = {
            "A": lambda: plain_stream(200, 136, 64, 48, (5, 3)),
            "A1": lambda: plain_stream(200, 136, 200 + 5, 136 + 3, (5, 3)),
            "C": lambda: sub_stream(202, 138, 64, 48),
            "C1": lambda: sub_stream(202, 138, 202, 138),
            "C_off": lambda: sub_stream(202, 138, 64, 48, (5, 3)),
            "C1_odd": lambda: sub_stream(201, 137, 201, 137),
            "A2": lambda: part1_stream(200, 136, 64, 48, (5, 3), 2, False, 5)[0],
            "P": lambda: part1_stream(200, 136, 64, 48, (5, 3), 1, True, 6)[0],
        }[name]()
    return _streams[name]


def test_the_streams_are_what_the_cases_need():
    for name, tiles, runs in (("A", 12, 1), ("A2", 12, 1), ("A1", 1, 1), ("C", 12, 2), ("C1", 1, 2), ("P", 12, 1)):
        info = G.read_header(stream(name))
        assert info.num_tiles == tiles and (info.comp_dx[1] == 2) == (runs == 2)
    a2, p = G.read_header(stream("A2")), G.read_header(stream("P"))
    assert a2.num_layers == 2 and a2.base.reserved[0] == 1 and a2.base.reserved[1] == 0
    out = G.read_packets(stream("A2"), a2)
    assert len(out["moves"]) > 100 and out["appendix_bytes"] > 0
    assert p.num_layers == 1 and p.base.reserved[0] == 1 and p.base.reserved[1] == 4
    cs, segs = part1_stream(200, 136, 64, 48, (5, 3), 1, True, 6)
    out = G.read_packets(cs, p)
    first = out["first_segment"]
    assert [[(int(s["length"]), int(s["numpasses"])) for s in out["segments"][first[i]:first[i + 1]]] for i in range(len(segs))] == segs
    assert max(len(s) for s in segs) >= 4 and min(len(s) for s in segs) == 1


# ---- a plan out of the driver --------------------------------------------------------------------------------------------------
DEST = ("route sub up ht want_segs all bps nr W H total kstep group_bytes ngroups nplaces nfills nunits lay channels xstep row ipx_kstep ipx_bytes "
        "unit_ch upload_image rx0 ry0 rx1 ry1 tl_interleaved tl_channels tl_fill").split()
GROUP = "tile_w tile_h tile_x0 tile_y0 num_comps uw uh unit_size skip place_at nunits nin_place nlaunches".split()
LAUNCH = "first count run at ncomp bps w h row kstep dx dy".split()


def plan(cs, reduce=0, window=None, layout=None, upsample=False, on_device=True, cap=NO_CAP, align=0, direct=True, surface=None, view=True, only=None):
    """-> (rc, reason) for a refusal, else the destination plan as a dict"""
    L = lib()
    buf = np.frombuffer(cs, np.uint8)
    v = G.ImageView.make(reduce, window)
    keep = np.asarray(only if only is not None else [], np.uint32)
    rc = L.dip_plan(ptr(buf), C.c_uint64(buf.size), C.byref(v) if view else None, C.byref(layout) if layout is not None else None, int(upsample), int(on_device),
                    C.c_uint64(cap), align, int(direct), C.byref(surface) if surface is not None else None, ptr(keep) if only is not None else None, len(keep))
    if rc:
        return rc, L.dip_reason().decode()
    out = np.zeros(32, np.uint64)
    L.dip_dest(ptr(out))
    d = dict(zip(DEST, (int(x) for x in out)))
    nc = G.read_header(cs).base.num_comps
    planes = np.zeros((nc, 5), np.uint64)
    L.dip_planes(ptr(planes))
    d["planes"] = planes.astype(np.int64)
    d["places"] = np.zeros((d["nplaces"], 2), np.int32)
    L.dip_places(ptr(d["places"]))
    d["fills"] = np.zeros((d["nfills"], 6), np.uint32)
    L.dip_fills(ptr(d["fills"]))
    d["run_dest"] = np.zeros((d["nr"] if d["route"] == RUNS else 0, 3), np.uint64)
    L.dip_run_dest(ptr(d["run_dest"]))
    d["units"] = np.zeros((d["nunits"], 11), np.int64)
    L.dip_units(ptr(d["units"]))
    d["surf_comps"], d["surf_routes"] = np.zeros((nc, 7), np.uint64), np.zeros((d["nr"], 6), np.uint64)
    if d["route"] == SURFACE:
        L.dip_surface(ptr(d["surf_comps"]), ptr(d["surf_routes"]))
    d["groups"] = []
    for k in range(d["ngroups"]):
        g = np.zeros(13, np.uint64)
        L.dip_group(k, ptr(g))
        g = dict(zip(GROUP, (int(x) for x in g)))
        g["units"], g["in_place"] = np.zeros(g["nunits"], np.uint32), np.zeros(g["nin_place"], np.uint32)
        la = np.zeros((g["nlaunches"], 12), np.uint64)
        L.dip_group_lists(k, ptr(g["units"]), ptr(g["in_place"]), ptr(la))
        g["launches"] = [dict(zip(LAUNCH, (int(x) for x in row))) for row in la]
        d["groups"].append(g)
    return d


def nv12(cs):
    info = G.read_header(cs)
    return G.Surface.make("NV12", info.layout)[0]


# ---- a. routes and refusals ------------------------------------------------------------------------------------------------------
def test_routes():
    assert plan(stream("A1"))["route"] == DIRECT
    r = plan(stream("A1"), window=(3, 4, 50, 60))
    assert (r["route"], r["rx0"], r["ry0"], r["rx1"], r["ry1"]) == (REGION, 3, 4, 50, 60)
    assert plan(stream("A1"), reduce=3, window=(1, 1, 9, 9))["route"] == STAGED            # no DWT level left for the region decoder
    assert plan(stream("A1"), reduce=3)["route"] == DIRECT                                 # (the whole tile: held wholly)
    a = plan(stream("A"))
    assert (a["route"], a["sub"], a["up"], a["ht"], a["want_segs"], a["all"]) == (STAGED, 0, 0, 1, 0, 1)
    assert plan(stream("A"), view=False)["route"] == STAGED
    assert plan(stream("C1"))["route"] == RUNS
    c = plan(stream("C"))
    assert (c["route"], c["sub"], c["up"]) == (STAGED, 1, 0)
    c = plan(stream("C"), upsample=True)
    assert (c["route"], c["sub"], c["up"]) == (STAGED, 1, 1)
    assert plan(stream("C1"), upsample=True)["route"] == STAGED
    for name in ("C", "C1"):
        s = plan(stream(name), surface=nv12(stream(name)), view=False)
        assert (s["route"], s["sub"], s["up"]) == (SURFACE, 1, 0)
    assert (plan(stream("P"))["ht"], plan(stream("P"))["want_segs"], plan(stream("A2"))["want_segs"]) == (0, 1, 0)


def test_refusals_with_their_codes_and_texts():
    """(the texts: those of decode_image.cpp before the planning moved out of it)"""
    A, C_ = stream("A"), stream("C")
    assert plan(C_, reduce=1, upsample=True) == (ERR_UNSUPPORTED, "a reduced resolution of sub-sampled components together with upsampling (grk_amd_set_decode_upsample)")
    for lay in (G.PixelLayout.make(interleaved=True), G.PixelLayout.make(row_pitch=256), G.PixelLayout.make(interleaved=True, channels=4)):
        assert plan(C_, layout=lay) == (ERR_UNSUPPORTED, "a decode pixel layout for sub-sampled components without upsampling (grk_amd_set_decode_upsample)")
    # the colour transform signalled over components of different size: COD's MCT byte of C set
    c = C_.index(b"\xff\x52")
    assert plan(C_[:c + 8] + b"\x01" + C_[c + 9:]) == (ERR_UNSUPPORTED, "the colour transform across components of different size")
    total = 3 * 200 * 136
    assert plan(A, cap=total - 1) == (ERR_OVERFLOW, "the image does not fit `cap`")
    assert plan(A, cap=total)["total"] == total
    assert plan(C_, cap=202 * 138 + 2 * 101 * 69 - 1) == (ERR_OVERFLOW, "the image does not fit `cap`")
    assert plan(C_, surface=nv12(C_), cap=202 * 138 + 202 * 69 - 1, view=False) == (ERR_OVERFLOW, "the image does not fit `cap`")
    assert plan(A, layout=G.PixelLayout.make(row_pitch=199)) == (ERR_INVALID, "pixel layout: row_pitch is smaller than a row")
    assert plan(A, layout=G.PixelLayout.make(interleaved=True, channels=2)) == (ERR_INVALID, "pixel layout: channels below num_comps or above 4")
    assert plan(A, layout=G.PixelLayout.make(interleaved=True, plane_pitch=8)) == (ERR_INVALID, "pixel layout: plane_pitch belongs to the planar layout")
    # QCD exponents that are not the library's: one exponent of A's reversible QCD raised
    q = A.index(b"\xff\x5c")
    bad = A[:q + 5] + bytes([A[q + 5] + 8]) + A[q + 6:]
    assert plan(bad) == (ERR_UNSUPPORTED, "an HT stream whose QCD exponents are not the ones this library derives for the geometry")
    # (a view plan never comes without tiles -- an empty window is invalid there --: the refusal stands behind it, for a plan cut to none)
    assert plan(A, only=[]) == (ERR_INVALID, "a view that touches no tile")
    # two components of a surface on one byte
    s = nv12(C_)
    s.comp[2].offset = s.comp[1].offset
    assert plan(C_, surface=s, view=False) == (ERR_INVALID, "surface: two components of a destination share bytes")


def test_a_run_off_the_alignment_in_device_memory_is_decoded_beside_it():
    c1 = plan(stream("C1"))
    assert [list(map(int, r)) for r in c1["run_dest"]] == [[0, 202 * 138, 0], [27876, 2 * 101 * 69, 0]]
    odd = plan(stream("C1_odd"))                          # 201 x 137: luma 27 537 bytes, chroma 101 x 69
    assert [list(map(int, r)) for r in odd["run_dest"]] == [[0, 27537, 0], [27537, 2 * 101 * 69, 1]]
    assert [int(r[2]) for r in plan(stream("C1_odd"), on_device=False)["run_dest"]] == [0, 0]
    assert [int(r[2]) for r in plan(stream("C1_odd"), align=3)["run_dest"]] == [1, 0]       # (the base itself off: luma beside, chroma on)


# ---- b. the destination is covered exactly once ----------------------------------------------------------------------------------
def paint(cover, at, x0, x1, y0, y1, row, xstep, nbytes):
    """the samples [x0, x1) x [y0, y1) of a plane at `at`: nbytes each, xstep and row bytes apart"""
    if x1 <= x0 or y1 <= y0:
        return
    idx = at + np.arange(y0, y1)[:, None, None] * row + np.arange(x0, x1)[None, :, None] * xstep + np.arange(nbytes)[None, None, :]
    np.add.at(cover, idx.reshape(-1), 1)


def painted(d, info):
    cover = np.zeros(d["total"], np.int32)
    bps = d["bps"]
    for f in d["fills"]:
        comp, x0, y0, w, h, _ = (int(v) for v in f)
        paint(cover, comp * d["kstep"], x0, x0 + w, y0, y0 + h, d["row"], d["xstep"], bps)
    for g in d["groups"]:
        for u in g["in_place"]:                          # a surface's run through its layout
            in_place, at, inter, ch, row, plane = (int(v) for v in d["surf_routes"][u % d["nr"]])
            assert in_place
            tw, th, ncomp = (int(v) for v in d["units"][u][[2, 3, 4]])
            for k in range(ncomp):
                paint(cover, at + (k * bps if inter else k * plane), 0, tw, 0, th, row, ch * bps if inter else bps, bps)
        if g["skip"]:
            assert not g["launches"] or d["route"] == STAGED
            continue
        covered = 0
        for la in g["launches"]:
            assert la["first"] == covered and all(u % d["nr"] == la["run"] for u in g["units"][la["first"]:la["first"] + la["count"]])
            covered += la["count"]
            for i in range(la["first"], la["first"] + la["count"]):
                x, y = (int(v) for v in d["places"][g["place_at"] + i])
                if d["route"] == SURFACE:               # KD: every component of the run wherever the surface has it
                    first = int(d["units"][g["units"][i]][5])
                    for k in range(g["num_comps"]):
                        off, pitch, w, h, _, _, step = (int(v) for v in d["surf_comps"][first + k])
                        assert 0 <= x and x + g["uw"] <= w and 0 <= y and y + g["uh"] <= h
                        paint(cover, off, x, x + g["uw"], y, y + g["uh"], pitch, step * bps, bps)
                elif d["up"]:                           # KU: the footprints, clipped to the image area
                    ix0, iy0 = info.layout.x0, info.layout.y0
                    X0, X1 = max(ix0, x * la["dx"]), min(ix0 + la["w"], (x + g["uw"]) * la["dx"])
                    Y0, Y1 = max(iy0, y * la["dy"]), min(iy0 + la["h"], (y + g["uh"]) * la["dy"])
                    assert x * la["dx"] < ix0 + la["w"] and y * la["dy"] < iy0 + la["h"]
                    for k in range(la["ncomp"]):
                        paint(cover, la["at"] + k * la["kstep"], X0 - ix0, X1 - ix0, Y0 - iy0, Y1 - iy0, la["row"], d["xstep"], la["bps"])
                else:                                   # KP: clipped to the target's planes
                    row = la["row"] or la["w"] * la["bps"]
                    plane = la["kstep"] or la["h"] * row
                    for k in range(la["ncomp"]):
                        paint(cover, la["at"] + k * plane, max(0, x), min(la["w"], x + g["uw"]), max(0, y), min(la["h"], y + g["uh"]), row, la["bps"], la["bps"])
        assert covered == g["nunits"]
    return cover


def check_cover(name, **kw):
    cs = stream(name)
    d = plan(cs, **kw)
    assert isinstance(d, dict), d
    assert d["route"] in (STAGED, SURFACE)
    cover = painted(d, G.read_header(cs))
    assert cover.min() == 1 and cover.max() == 1, (name, kw, int((cover == 0).sum()), int((cover > 1).sum()))
    return d


@pytest.mark.parametrize("reduce", [0, 1, 2, 3])
@pytest.mark.parametrize("name", ["A", "C"])
def test_every_sample_is_placed_exactly_once_at_every_reduce(name, reduce):
    d = check_cover(name, reduce=reduce)
    sizes = G.image_view_size(G.read_header(stream(name)), reduce)
    assert d["total"] == sum(w * h for w, h in sizes) and [(int(p[1]), int(p[2])) for p in d["planes"]] == sizes
    assert int(d["planes"][1][0]) == sizes[0][0] * sizes[0][1]
    # the staging buffer holds the largest batch, and every batch's units are of one size
    assert d["group_bytes"] == max(g["unit_size"] * g["nunits"] for g in d["groups"])
    for g in d["groups"]:
        assert g["unit_size"] == g["uw"] * g["uh"] * g["num_comps"] and all(tuple(d["units"][u][[6, 7]]) == (g["uw"], g["uh"]) for u in g["units"])
    assert sorted(int(u) for g in d["groups"] for u in g["units"]) == list(range(d["nunits"]))
    assert [g["place_at"] for g in d["groups"]] == list(np.cumsum([0] + [g["nunits"] for g in d["groups"]])[:-1])


def test_windows_and_layouts_are_covered_exactly_once():
    d = check_cover("A", reduce=1, window=(3, 4, 50, 60))
    assert (d["W"], d["H"], d["all"]) == (47, 56, 0) and any(x < 0 or y < 0 for x, y in d["places"])
    # whole pixels of four channels: KP places pixels as they are, the fourth channel is the tile decoder's fill -- no fill launch
    d = check_cover("A", layout=G.PixelLayout.make(interleaved=True, channels=4, fill=77))
    assert (d["unit_ch"], d["tl_interleaved"], d["tl_channels"], d["tl_fill"], d["nfills"], d["upload_image"]) == (4, 1, 4, 77, 0, 1)
    assert all(la["ncomp"] == 1 and la["bps"] == 4 for g in d["groups"] for la in g["launches"]) and d["total"] == 4 * 200 * 136
    # a pitched planar layout: the gaps stay untouched
    lay = G.PixelLayout.make(row_pitch=208, plane_pitch=208 * 140)
    d = plan(stream("A"), layout=lay)
    cover = painted(d, G.read_header(stream("A")))
    want = np.zeros(d["total"], np.int32)
    for k in range(3):
        paint(want, k * 208 * 140, 0, 200, 0, 136, 208, 1, 1)
    assert d["total"] == 2 * 208 * 140 + 135 * 208 + 200 and np.array_equal(cover, want) and d["upload_image"] == 1


def test_upsampled_components_are_covered_exactly_once_fills_included():
    d = check_cover("C", upsample=True)
    assert d["total"] == 3 * 202 * 138 and all(int(f[3]) * int(f[4]) == 0 for f in d["fills"]) and d["nfills"] == 6      # (origin 0: empty strips)
    d = check_cover("C_off", upsample=True)
    # image area from (5, 3): chroma's first sample (3, 2) covers from (6, 4): a strip of one column and one row, per chroma component
    assert [[int(v) for v in f] for f in d["fills"]] == [[0, 0, 0, 0, 138, 0], [0, 0, 0, 202, 0, 0], [1, 0, 0, 1, 138, 0], [1, 1, 0, 201, 1, 0],
                                                        [2, 0, 0, 1, 138, 0], [2, 1, 0, 201, 1, 0]]
    d = check_cover("C_off", upsample=True, layout=G.PixelLayout.make(interleaved=True, channels=4, fill=9))
    assert [int(v) for v in d["fills"][-1]] == [3, 0, 0, 202, 138, 9] and d["kstep"] == 1 and d["total"] == 4 * 202 * 138


@pytest.mark.parametrize("direct", [True, False])
def test_a_surface_is_covered_exactly_once(direct):
    d = check_cover("C", surface=nv12(stream("C")), direct=direct, view=False)
    assert d["total"] == 202 * 138 + 202 * 69 and not any(g["nin_place"] for g in d["groups"])           # (12 tiles: nothing in place)
    d = check_cover("C1", surface=nv12(stream("C1")), direct=direct, view=False)
    assert [g["nin_place"] for g in d["groups"]] == ([1, 1] if direct else [0, 0])
    assert sum(g["nunits"] for g in d["groups"]) == (0 if direct else 2)


# ---- c. compaction and rebase ----------------------------------------------------------------------------------------------------
A_COLS, A_ROWS = [0, 59, 123, 187, 200], [0, 45, 93, 136]            # the tile grid of A in image coordinates


def window_of(tiles):
    """a window inside the given tiles' bounding box that touches exactly them (they form a rectangle of the grid)"""
    xs, ys = [t % 4 for t in tiles], [t // 4 for t in tiles]
    return (A_COLS[min(xs)] + 1, A_ROWS[min(ys)] + 1, A_COLS[max(xs) + 1] - 1, A_ROWS[max(ys) + 1] - 1)


def coded_plan(cs, nt):
    L = lib()
    out, parts = np.zeros(4, np.uint64), np.zeros((nt, 2), np.uint64)
    assert L.dip_coded(ptr(out), ptr(parts)) == 0, L.dip_reason()
    every, up_len, coded_cap, ncopies = (int(v) for v in out)
    part_to, copies = np.zeros(max(1, nt), np.uint64), np.zeros((ncopies, 3), np.uint64)
    L.dip_coded_lists(ptr(part_to), ptr(copies))
    return every, up_len, coded_cap, [[int(v) for v in c] for c in copies], parts.astype(np.int64), part_to.astype(np.int64)


def rebase(corrupt=0):
    L = lib()
    n = np.zeros(4, np.uint64)
    rc = L.dip_read_and_rebase(corrupt, ptr(n))
    if rc:
        return rc, L.dip_reason().decode()
    nrows, nmoves, nsegs, app = (int(v) for v in n)
    t = dict(old_rows=np.zeros(nrows, CODED_DTYPE), rows=np.zeros(nrows, CODED_DTYPE), old_moves=np.zeros(nmoves, MOVE_DTYPE), moves=np.zeros(nmoves, MOVE_DTYPE),
             first=np.zeros(nrows + 1, np.uint32), segments=np.zeros(max(1, nsegs), SEGMENT_DTYPE), appendix_bytes=app)
    unit_row = np.zeros(1 << 10, np.uint64)
    L.dip_table(ptr(t["old_rows"]), ptr(t["rows"]), ptr(t["old_moves"]), ptr(t["moves"]), ptr(t["first"]), ptr(t["segments"]), ptr(unit_row))
    t["segments"], t["unit_row"] = t["segments"][:nsegs], unit_row
    return t


@pytest.mark.parametrize("tiles,ncopies", [([5], 1), ([1, 2], 1), ([0, 5, 10], 3), (list(range(12)), 1)])
@pytest.mark.parametrize("name", ["A", "A2"])
def test_compaction_and_rebase_move_the_right_bytes(name, tiles, ncopies):
    cs = stream(name)
    csb = np.frombuffer(cs, np.uint8)
    if tiles == [0, 5, 10]:
        d = plan(cs, only=tiles)              # (no window touches exactly a diagonal: the whole image's plan cut down to it)
    else:
        d = plan(cs, window=window_of(tiles)) if len(tiles) < 12 else plan(cs)
    touched = tiles
    assert d["nunits"] == len(tiles) and d["all"] == (len(tiles) == 12)
    every, up_len, coded_cap, copies, parts, part_to = coded_plan(cs, 12)
    assert every == (len(touched) == 12) and len(copies) == ncopies
    layers = G.read_header(cs).num_layers
    if every:
        assert up_len == len(cs) and copies == [[0, 0, len(cs)]]
    else:
        assert up_len == sum(int(parts[t][1]) for t in touched)
        # the copies: the maximal runs of tile-parts that follow each other in the file
        runs = 1 + sum(int(parts[a][0] + parts[a][1]) != int(parts[b][0]) for a, b in zip(touched, touched[1:]))
        assert len(copies) == runs and sum(c[2] for c in copies) == up_len
        assert [int(part_to[i]) for i in range(len(touched))] == [sum(int(parts[t][1]) for t in touched[:i]) for i in range(len(touched))]
    assert coded_cap == up_len * (2 if layers > 1 else 1)
    compact = np.zeros(up_len, np.uint8)
    for to, frm, n in copies:
        compact[to:to + n] = csb[frm:frm + n]
    t = rebase()
    assert isinstance(t, dict), t
    assert (len(t["moves"]) > 0) == (name == "A2")
    for old, new in zip(t["old_rows"], t["rows"]):
        n = int(new["length"])
        assert n == int(old["length"]) and new["missing_msbs"] == old["missing_msbs"]
        if not n:
            continue
        if int(old["offset"]) >= len(cs):
            assert int(new["offset"]) == int(old["offset"]) - len(cs) + up_len                          # the appendix behind what is uploaded
        else:
            assert np.array_equal(compact[int(new["offset"]):int(new["offset"]) + n], csb[int(old["offset"]):int(old["offset"]) + n])
    for old, new in zip(t["old_moves"], t["moves"]):
        n = int(new["len"])
        assert (int(new["dst"]), n) == (int(old["dst"]), int(old["len"]))
        assert np.array_equal(compact[int(new["src"]):int(new["src"]) + n], csb[int(old["src"]):int(old["src"]) + n])
    # unit_row: the tiles' rows one after the other
    assert int(t["unit_row"][len(touched)]) == len(t["rows"]) and int(t["unit_row"][0]) == 0


@pytest.mark.parametrize("tiles", [[5], [1, 2], [0, 5, 10]])
def test_corrupted_tables_are_refused(tiles):
    for name in ("A", "A2"):
        cs = stream(name)
        plan(cs, only=tiles)
        coded_plan(cs, 12)
        assert rebase(1) == (ERR_INVALID, "a block outside its tile-part")
        assert rebase(3) == (ERR_INVALID, "the reader's table does not fit the tiles")
        if name == "A2":
            assert rebase(2) == (ERR_INVALID, "a block outside its tile-part")
        assert isinstance(rebase(0), dict)


# ---- d. group tables ---------------------------------------------------------------------------------------------------------------
def group_tables(units):
    L = lib()
    n = np.zeros(3, np.uint64)
    u = np.asarray(units, np.uint32)
    L.dip_group_tables(ptr(u), C.c_uint64(len(u)), ptr(n))
    rows, first, segs = np.zeros(int(n[0]), CODED_DTYPE), np.zeros(max(1, int(n[1])), np.uint32), np.zeros(max(1, int(n[2])), SEGMENT_DTYPE)
    L.dip_group_tables_get(ptr(rows), ptr(first), ptr(segs))
    return rows, first[:int(n[1])], segs[:int(n[2])]


def test_group_tables_are_the_units_rows_and_segment_lists_in_the_groups_order():
    cs = stream("P")
    d = plan(cs)
    coded_plan(cs, 12)
    t = rebase()
    assert d["want_segs"] == 1 and len(d["groups"]) > 1
    ur, first_all = t["unit_row"].astype(np.int64), t["first"].astype(np.int64)
    for g in d["groups"]:
        rows, first, segs = group_tables(g["units"])
        want_rows = np.concatenate([t["rows"][ur[u]:ur[u + 1]] for u in g["units"]])
        assert np.array_equal(rows, want_rows) and len(first) == len(rows) + 1
        want_segs = np.concatenate([t["segments"][first_all[ur[u]]:first_all[ur[u + 1]]] for u in g["units"]])
        assert np.array_equal(segs, want_segs) and int(first[-1]) == len(segs) and int(first[0]) == 0
        counts = np.concatenate([np.diff(first_all[ur[u]:ur[u + 1] + 1]) for u in g["units"]])
        assert np.array_equal(np.diff(first.astype(np.int64)), counts) and counts.max() >= 4
    # an HT stream: no list
    cs = stream("A")
    d = plan(cs)
    coded_plan(cs, 12)
    t = rebase()
    rows, first, segs = group_tables(d["groups"][0]["units"])
    assert len(rows) == sum(int(ur_) for ur_ in np.diff(t["unit_row"].astype(np.int64))[d["groups"][0]["units"]]) and len(first) == 0 and len(segs) == 0


# ---- e. one staging plan, two callers --------------------------------------------------------------------------------------------
def test_the_staging_plan_of_a_surface_is_the_same_for_encode_and_decode():
    cs = stream("C")
    info = G.read_header(cs)
    surf = nv12(cs)
    L = lib()
    dxs, dys = (C.c_uint8 * 4)(1, 2, 2, 0), (C.c_uint8 * 4)(1, 2, 2, 0)
    out = np.zeros(3, np.uint64)
    assert L.dip_encode_staging(C.byref(info.layout), C.byref(info.base), dxs, dys, C.byref(surf), C.c_uint64(NO_CAP), 0, 0, ptr(out)) == 0, L.dip_reason()
    ngroups, nstaged, group_bytes = (int(v) for v in out)
    units, group_of, origins, segs = np.zeros(nstaged, np.uint32), np.zeros(nstaged, np.uint32), np.zeros((nstaged, 2), np.uint32), np.zeros((64, 4), np.uint32)
    nsegs = L.dip_encode_staging_lists(ptr(units), ptr(group_of), ptr(origins), ptr(segs), 64)
    segs = segs[:nsegs]
    # expected from the tile grid: columns 0 64 128 192 202, rows 0 48 96 138; chroma on the halved grid
    lay = info.layout
    want = {}
    for t in range(12):
        for run, (dx, dy) in enumerate(((1, 1), (2, 2))):
            p = tile_comp(lay, info.base, dx, dy, t)
            want[2 * t + run] = (p.tile_x0, p.tile_y0)                 # (the planes' x0, y0 are 0: the image starts at the origin)
    assert nstaged == 24 and sorted(int(u) for u in units) == list(range(24))
    assert sum(1 for u in units if u % 2 == 0) == 12 and sum(1 for u in units if u % 2 == 1) == 12
    assert all(tuple(int(v) for v in origins[i]) == want[int(u)] for i, u in enumerate(units))
    got = {int(u): tuple(int(v) for v in origins[i]) for i, u in enumerate(units)}
    assert (got[2 * 5], got[2 * 5 + 1], got[2 * 11 + 1]) == ((64, 48), (32, 24), (96, 48))             # tile 5's luma and chroma, tile 11's chroma
    # one launch per (group, run), the group's units of a run in one piece
    assert len(segs) == len({(int(g), int(u) % 2) for g, u in zip(group_of, units)})
    for g in range(ngroups):
        mine = [int(u) for u, k in zip(units, group_of) if k == g]
        assert [u % 2 for u in mine] == sorted(u % 2 for u in mine)
        assert [(int(s[1]), int(s[2])) for s in segs if s[0] == g] == [(mine.index(next(u for u in mine if u % 2 == r)), sum(u % 2 == r for u in mine))
                                                                       for r in sorted({u % 2 for u in mine})]
    # the decode's plan of the same surface: the same units, origins, segments and bytes
    d = plan(cs, surface=surf, direct=False, view=False)
    assert [int(u) for g in d["groups"] for u in g["units"]] == [int(u) for u in units]
    assert np.array_equal(d["places"].astype(np.uint32), origins) and d["group_bytes"] == group_bytes
    assert [(k, la["first"], la["count"], la["run"]) for k, g in enumerate(d["groups"]) for la in g["launches"]] == [tuple(int(v) for v in s) for s in segs]
    assert group_bytes == max(g["unit_size"] * g["nunits"] for g in d["groups"])


# ---- f. the functions that moved ------------------------------------------------------------------------------------------------------
def test_add_unit_groups_tiles_as_same_tile_geometry_says():
    info = G.read_header(stream("A"))
    tiles = G.layout_tiles(info.layout, info.base)
    arr = (G.TileParams * 12)(*tiles)
    of = np.zeros(12, np.uint32)
    ngroups = lib().dip_add_units(arr, 12, ptr(of))
    assert ngroups == len(set(of.tolist())) and 1 < ngroups < 12
    for a in range(12):
        for b in range(12):
            assert (of[a] == of[b]) == G.same_tile_geometry(tiles[a], tiles[b]), (a, b)
    assert list(of[:1]) == [0] and all(of[i] <= max(of[:i]) + 1 for i in range(1, 12))       # groups are numbered in the order they appear


def test_resolve_pixel_layout_on_hand_worked_layouts():
    """a 5 x 3 tile of 3 components, 8 bits: tight planar, pitched planar, four interleaved channels -> {lay, channels, xstep, fill, row, kstep, tile, bytes}"""
    p = G.TileParams.make(5, 3, 3, 8, 1)
    L = lib()
    out = np.zeros(8, np.uint64)

    def resolve(lay, ntiles=1):
        ok = L.dip_resolve_layout(C.byref(p), C.byref(lay) if lay is not None else None, 0, 0, ntiles, ptr(out))
        return [int(v) for v in out] if ok else L.dip_reason().decode()
    assert resolve(None) == [0, 1, 1, 0, 5, 15, 45, 45]
    assert resolve(G.PixelLayout.make(row_pitch=5, plane_pitch=15, tile_pitch=45), 2) == [0, 1, 1, 0, 5, 15, 45, 90]      # the default, however it is said
    assert resolve(G.PixelLayout.make(row_pitch=8, plane_pitch=32), 2) == [1, 1, 1, 0, 8, 32, 96, 96 + 64 + 2 * 8 + 5]
    assert resolve(G.PixelLayout.make(interleaved=True, channels=4, fill=200)) == [2, 4, 4, 200, 20, 1, 60, 60]
    assert resolve(G.PixelLayout.make(interleaved=True, channels=4, row_pitch=24), 3) == [2, 4, 4, 0, 24, 1, 72, 2 * 72 + 2 * 24 + 20]
    assert resolve(G.PixelLayout.make(row_pitch=4)) == "pixel layout: row_pitch is smaller than a row"
    p16 = G.TileParams.make(5, 3, 3, 12, 1)
    assert L.dip_resolve_layout(C.byref(p16), C.byref(G.PixelLayout.make(row_pitch=11)), 0, 0, 1, ptr(out)) == 0
    assert L.dip_reason() == b"pixel layout: a pitch is no multiple of the sample size"


def test_parallel_for_runs_every_item_once():
    hits = np.zeros(1000, np.uint32)
    assert lib().dip_parallel_for(1000, 7, ptr(hits)) == 0 and np.array_equal(hits, np.ones(1000, np.uint32))
