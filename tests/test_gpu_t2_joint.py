"""GPU: Tier-2 on the device for sub-sampled images, video surfaces and packed frames (grok_amd/csrc/assemble.hip: encode_joint_device;
kernels_t2keep.hip).  Every case makes its file by the device route, makes it again by the same call under GRK_AMD_IMAGE_T2=host, and
asserts that the two are equal AND -- from grk_amd_encode_route_counters -- that the first really was assembled on the device and the
second written by the host writer: a silent fallback would make the comparison trivially true.  Where oracle/_ref is present and
the shape is one the reference's encoder is pinned on by tests/test_gpu_subsampled.py (reversible, image at the origin, 64 x 64
code-blocks, its own precinct rule) the file must be the reference's too.  The _device calls: the bytes behind the returned device
pointer are the host call's file, and decode back to the source planes.  All comparisons are exact; the shapes are the smallest at
which each mechanism can go wrong (the CPU side: tests/test_t2_joint_plan_cpu.py)."""
import numpy as np
import pytest

import grok_amd as G
import gpuutil as U
import packedref as P
import refharness as R
import synth
from test_t2_reader_subsampled_cpu import make_planes

pytestmark = pytest.mark.gpu
S420, S422 = [(1, 1), (2, 2), (2, 2)], [(1, 1), (2, 1), (2, 1)]
S3RUNS, S4 = [(1, 1), (2, 1), (1, 2)], [(1, 1), (2, 2), (2, 2), (1, 1)]
ALL = G.CS_PLT | G.CS_TLM | G.CS_SOP | G.CS_EPH


def routes(monkeypatch, c, make):
    """make() by the device route and under GRK_AMD_IMAGE_T2=host -> the file, both equal, each by the route it was asked for"""
    monkeypatch.delenv("GRK_AMD_IMAGE_T2", raising=False)
    before = c.encode_route_counters()
    dev = make()
    after = c.encode_route_counters()
    assert (after[0] - before[0], after[1] - before[1]) == (1, 0), "the default route did not assemble on the device"
    monkeypatch.setenv("GRK_AMD_IMAGE_T2", "host")
    host = make()
    assert c.encode_route_counters() == (after[0], after[1] + 1), "GRK_AMD_IMAGE_T2=host did not go to the host writer"
    monkeypatch.delenv("GRK_AMD_IMAGE_T2")
    assert len(dev) == len(host) and dev == host
    return dev


# name: W, H, sampling, prec, levels, keywords (tile, offset, cblk, precincts, irreversible), flags, compared with the reference
IMAGES = {
    "420-64x48": (64, 48, S420, 8, 2, {}, [0], True),                                    # the smallest
    "420-101x77-5levels": (101, 77, S420, 8, 5, {}, [0, G.CS_PLT], True),                # chroma bands empty at the deep levels
    "422-130x66-10bit": (130, 66, S422, 10, 3, {}, [0], True),
    "three-runs": (90, 70, S3RUNS, 8, 3, {}, [0, ALL | G.CS_PROG(2)], True),             # three batches
    "four-components": (100, 76, S4, 8, 3, {}, [0, ALL | G.CS_PROG(4)], True),           # Y and A: two units of a tile in one batch
    "97-420-96x80": (96, 80, S420, 8, 3, {"irreversible": True}, [0], False),            # Kmax differs by band
    "precincts-32": (128, 128, S420, 8, 3, {"precincts": [(5, 5)] * 4}, [0, ALL | G.CS_PROG(3)], False),
    "cblk-4x4": (256, 256, S420, 8, 1, {"cblk": (2, 2)}, [0], False),                    # a luma packet of > 1024 blocks: t2_header_kernel<4096>
}


def image(name):
    W, H, sampling, prec, L, kw, flags, ref = IMAGES[name]
    layout = G.ImageLayout.make(W, H, *kw.get("tile", (None, None)), offset=kw.get("offset", (0, 0)))
    base = G.TileParams.make(1, 1, len(sampling), prec, L, mct=False, irreversible=kw.get("irreversible", False), cblk=kw.get("cblk", (6, 6)),
                             precincts=kw.get("precincts"))
    return layout, base, sampling, make_planes(layout, sampling, prec, seed=len(name)), flags, ref


@pytest.mark.parametrize("name", sorted(IMAGES))
def test_encode_image_subsampled_device_route(monkeypatch, name):
    layout, base, sampling, planes, flag_list, ref = image(name)
    W, H, _, prec, L = IMAGES[name][:5]
    c = U.ctx()
    for flags in flag_list:
        got = routes(monkeypatch, c, lambda: c.encode_image_subsampled(layout, base, sampling, planes, flags))
        if not base.irreversible:
            assert all(np.array_equal(a, b) for a, b in zip(c.decode_image_planes(got), planes))
        if ref and R.have_ref():
            for k, v in (("REF_PROG_ORDER", (flags >> 8) & 7 if flags else 0), ("REF_WRITE_TLM", int(bool(flags & G.CS_TLM))),
                         ("REF_WRITE_PLT", int(bool(flags & G.CS_PLT))), ("REF_CSTY", (2 if flags & G.CS_SOP else 0) | (4 if flags & G.CS_EPH else 0))):
                monkeypatch.setenv(k, str(v))
            assert got == R.encode_planes(planes, sampling, prec, W, H, numres=L + 1, mct=0), (name, flags, "the reference's file")


TILED = (200, 136, S420, 8, 3, {"tile": (96, 64), "offset": (6, 10)})


@pytest.mark.parametrize("flags", [0] + [ALL | G.CS_PROG(o) for o in range(5)], ids=["plain", "lrcp", "rlcp", "rpcl", "pcrl", "cprl"])
def test_ragged_tiles_under_an_image_offset(monkeypatch, flags):
    """200 x 136 at (6, 10) in tiles of 96 x 64: several tile classes, each framed by a call of its own behind the one before"""
    W, H, sampling, prec, L, kw = TILED
    layout = G.ImageLayout.make(W, H, *kw["tile"], offset=kw["offset"])
    base = G.TileParams.make(1, 1, 3, prec, L, mct=False)
    planes = make_planes(layout, sampling, prec, seed=11)
    c = U.ctx()
    got = routes(monkeypatch, c, lambda: c.encode_image_subsampled(layout, base, sampling, planes, flags))
    assert all(np.array_equal(a, b) for a, b in zip(c.decode_image_planes(got), planes))


# ---- surfaces and packed frames -----------------------------------------------------------------------------------------------------
def surface_case(fmt, tile):
    layout = G.ImageLayout.make(70, 38, *(tile or (None, None)))
    surface, sampling, nbytes = G.Surface.make(fmt, layout, None, 0)
    prec = G.SURFACE_FORMATS_MSB[fmt][1] if fmt in G.SURFACE_FORMATS_MSB else 8
    base = G.TileParams.make(1, 1, len(sampling), prec, 2, mct=False)
    planes = make_planes(layout, sampling, prec, seed=3)
    buf = np.random.default_rng(9).integers(0, 256, nbytes, dtype=np.uint8)
    surface.scatter(buf, planes, (prec + 7) // 8)
    return layout, base, sampling, surface, nbytes, planes, buf


@pytest.mark.parametrize("direct", [True, False], ids=["direct", "staged"])
@pytest.mark.parametrize("tile", [None, (32, 32)], ids=["one-tile", "tiles"])
@pytest.mark.parametrize("fmt", ["NV12", "I420", "NV16", "P010"])
def test_encode_surface_device_route(monkeypatch, fmt, tile, direct):
    layout, base, sampling, surface, nbytes, planes, buf = surface_case(fmt, tile)
    c = U.ctx()
    if direct:
        monkeypatch.delenv("GRK_AMD_SURFACE_DIRECT", raising=False)
    else:
        monkeypatch.setenv("GRK_AMD_SURFACE_DIRECT", "0")
    d_buf = U.to_dev(buf)
    flags = G.CS_PLT | G.CS_PROG(2)
    host = routes(monkeypatch, c, lambda: c.encode_surface(layout, base, sampling, surface, buf, flags))
    dev = routes(monkeypatch, c, lambda: c.encode_surface(layout, base, sampling, surface, d_buf.data_ptr(), flags, cap=nbytes))
    assert host == dev
    monkeypatch.setenv("GRK_AMD_IMAGE_T2", "host")
    assert host == c.encode_image_subsampled(layout, base, sampling, planes, flags)
    monkeypatch.delenv("GRK_AMD_IMAGE_T2")
    if R.have_ref() and tile is None:
        monkeypatch.setenv("REF_PROG_ORDER", "2")
        monkeypatch.setenv("REF_WRITE_PLT", "1")
        assert host == R.encode_planes(planes, sampling, base.prec, 70, 38, numres=3, mct=0)
    # the file left in device memory: the same bytes, and they decode to the source
    before = c.encode_route_counters()
    ptr, n = c.encode_surface_device(layout, base, sampling, surface, d_buf.data_ptr(), flags, cap=nbytes)
    assert c.encode_route_counters() == (before[0] + 1, before[1])
    got = U.from_dev_ptr(ptr, n).tobytes()
    assert got == host
    assert all(np.array_equal(a, b) for a, b in zip(c.decode_image_planes(got), planes))
    ptr, n = c.encode_surface_device(layout, base, sampling, surface, buf, flags)                    # a host surface
    assert U.from_dev_ptr(ptr, n).tobytes() == host


def test_device_file_of_another_size_on_the_same_context(monkeypatch):
    """a second _device call with a different size, tile classes out of tile order (the file is put together tile by tile), TLM"""
    c = U.ctx()
    for (w, h, tile, offset) in ((70, 38, None, (0, 0)), (200, 136, (96, 64), (6, 10)), (50, 20, None, (0, 0))):
        layout = G.ImageLayout.make(w, h, *(tile or (None, None)), offset=offset)
        surface, sampling, nbytes = G.Surface.make("I420", layout, None, 0)
        base = G.TileParams.make(1, 1, 3, 8, 3, mct=False)
        planes = make_planes(layout, sampling, 8, seed=w)
        buf = np.zeros(nbytes, np.uint8)
        surface.scatter(buf, planes, 1)
        flags = ALL | G.CS_PROG(3)
        ptr, n = c.encode_surface_device(layout, base, sampling, surface, buf, flags)
        got = U.from_dev_ptr(ptr, n).tobytes()
        monkeypatch.setenv("GRK_AMD_IMAGE_T2", "host")
        assert got == c.encode_surface(layout, base, sampling, surface, buf, flags)
        monkeypatch.delenv("GRK_AMD_IMAGE_T2")
        assert all(np.array_equal(a, b) for a, b in zip(c.decode_image_planes(got), planes))


def test_device_calls_have_no_host_writer_behind_them():
    layout, base, sampling, surface, nbytes, planes, buf = surface_case("NV12", None)
    c = U.ctx()
    before = c.encode_route_counters()
    with pytest.raises(G.SurfaceError) as e:
        c.encode_surface_device(layout, base, sampling, surface, buf, G.CS_BLOCK_MSBS)
    assert e.value.code == -2 and c.encode_route_counters() == before


@pytest.mark.parametrize("fmt,prec,w,h", [(P.YUY2, 8, 66, 10), (P.V210, 10, 48, 6)], ids=["yuy2-66x10", "v210-48x6"])
def test_encode_packed_device_route(monkeypatch, fmt, prec, w, h):
    rng = np.random.default_rng(fmt)
    dt = np.uint8 if prec <= 8 else np.uint16
    planes = [rng.integers(0, 1 << prec, (h, n)).astype(dt) for n in (w, (w + 1) // 2, (w + 1) // 2)]
    frame = P.pack(fmt, prec, *planes, 0, rng.integers(0, 256, P.frame_bytes(fmt, w, h, 0), dtype=np.uint8))
    layout = G.ImageLayout.make(w, h)
    base = G.TileParams.make(1, 1, 3, prec, 2, mct=False)
    c = U.ctx()
    d_buf = U.to_dev(np.concatenate([np.zeros(16, np.uint8), frame]))
    host = routes(monkeypatch, c, lambda: c.encode_packed(layout, base, fmt, frame, 0, G.CS_PLT))
    dev = routes(monkeypatch, c, lambda: c.encode_packed(layout, base, fmt, d_buf.data_ptr() + 16, 0, G.CS_PLT, cap=frame.size))
    assert host == dev
    if R.have_ref():
        monkeypatch.setenv("REF_WRITE_PLT", "1")
        assert host == R.encode_planes(planes, S422, prec, w, h, numres=3, mct=0)
    ptr, n = c.encode_packed_device(layout, base, fmt, d_buf.data_ptr() + 16, 0, G.CS_PLT, cap=frame.size)
    got = U.from_dev_ptr(ptr, n).tobytes()
    assert got == host
    assert all(np.array_equal(a, b) for a, b in zip(c.decode_image_planes(got), planes))


def test_device_route_on_a_pipelining_context(monkeypatch):
    """a context whose consecutive encodes are pipelined rotates its table and arena from batch to batch (small frames run their
    whole chain on a side stream): KK takes each batch's own set, behind its side streams -- the same files"""
    monkeypatch.delenv("GRK_AMD_IMAGE_T2", raising=False)
    c = G.Context(0)
    c.set_pipelining(2)
    for fmt, tile in (("NV12", None), ("I420", (32, 32)), ("NV12", None)):
        layout, base, sampling, surface, nbytes, planes, buf = surface_case(fmt, tile)
        want = U.ctx().encode_surface(layout, base, sampling, surface, buf, G.CS_PLT)
        before = c.encode_route_counters()
        d_buf = U.to_dev(buf)
        assert c.encode_surface(layout, base, sampling, surface, d_buf.data_ptr(), G.CS_PLT, cap=nbytes) == want
        ptr, n = c.encode_surface_device(layout, base, sampling, surface, buf, G.CS_PLT)
        assert U.from_dev_ptr(ptr, n).tobytes() == want
        assert c.encode_route_counters() == (before[0] + 2, before[1])
    c.set_pipelining(False)


# ---- the plan caches ----------------------------------------------------------------------------------------------------------------
def test_interleaved_calls_on_one_context(monkeypatch):
    """sub-sampled image, plain image, sub-sampled image on ONE context: each the bytes a fresh context gives; and a plain
    grk_amd_encode_tiles + grk_amd_assemble_device between them still equals the host writer"""
    monkeypatch.delenv("GRK_AMD_IMAGE_T2", raising=False)
    W, H = 128, 96
    layout = G.ImageLayout.make(W, H)
    sub_base = G.TileParams.make(1, 1, 3, 8, 3, mct=False)
    sub_planes = make_planes(layout, S420, 8, seed=1)
    other = G.ImageLayout.make(96, 80)
    other_planes = make_planes(other, S422, 8, seed=2)
    px = synth.g2(3, H, W, 8, seed=4)
    plain_base = G.TileParams.make(1, 1, 3, 8, 3)
    flags = G.CS_PLT | G.CS_PROG(2)

    def fresh(call):
        f = G.Context(0)
        try:
            return call(f)
        finally:
            del f

    calls = [lambda k: k.encode_image_subsampled(layout, sub_base, S420, sub_planes, flags),
             lambda k: k.encode_image(layout, plain_base, px, flags),
             lambda k: k.encode_image_subsampled(other, sub_base, S422, other_planes, flags),
             lambda k: k.encode_image_subsampled(layout, sub_base, S420, sub_planes, flags),
             lambda k: k.encode_image_subsampled(layout, sub_base, S420, sub_planes, G.CS_PLT | G.CS_PROG(4))]
    want = [fresh(call) for call in calls]
    c = G.Context(0)
    before = c.encode_route_counters()
    for i, call in enumerate(calls[:2]):
        assert call(c) == want[i], i
    # a plain batch and its device assembly in between: the context's own table, the plain plan cache
    p = G.TileParams.make(W, H, 3, 8, 3)
    table, coded = c.encode_host(p, px)
    n, lens = c.assemble_device(p, [0], flags)
    assert bytes(c.fetch_assembled(0, n)) == G.write_tile_part(p, 0, table, coded, flags)
    for i, call in enumerate(calls[2:], 2):
        assert call(c) == want[i], i
    after = c.encode_route_counters()
    assert (after[0] - before[0], after[1] - before[1]) == (4, 0)
