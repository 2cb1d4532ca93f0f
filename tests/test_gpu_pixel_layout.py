"""-m gpu: pixels in a layout of the caller's (grk_amd_set_pixel_layout: interleaved, pitched, a skipped fourth channel) code to
exactly the blocks the same samples give in the default layout -- transposed to planes on the host and coded by the same context --
and a decode into such a layout (grk_amd_set_decode_pixel_layout) writes exactly the default-layout decode's samples, there.
The planar paths are held to the oracle by the other files, so no tolerance and no golden data here.  Every gap and every skipped
channel holds random bytes (pixlayout.pack): a result that depended on them would differ from the planar one."""
import os

import numpy as np
import pytest
import torch

import grok_amd as G
import synth
import gpuutil as U
import pixlayout as X

pytestmark = pytest.mark.gpu

INVALID = -3
UNSUPPORTED = -2


def content(C, H, W, prec, sgnd=False, nt=1, seed=7):
    """(nt, C, H, W) samples: structure (so that every sub-band has something to code) plus noise, full range"""
    rng = np.random.default_rng(seed + W + 31 * H + C)
    px = np.stack([synth.g2(C, H, W, prec, seed=seed + t) for t in range(nt)]).astype(np.int64)
    px = (px + rng.integers(0, 1 << max(prec - 3, 1), size=px.shape)) % (1 << prec)
    if sgnd:
        return (px - (1 << (prec - 1))).astype(np.int8 if prec <= 8 else np.int16)
    return px.astype(np.uint8 if prec <= 8 else np.uint16)


def blocks_of(c, p, nt, ptr, on_device):
    table, tot = c.encode_tiles(p, nt, ptr, on_device)
    coded = c.fetch_coded(tot)
    return list(table["length"]), list(table["missing_msbs"]), U.split_blocks(table, coded)


def planar_blocks(c, p, px):
    c.set_pixel_layout(None)
    host = np.ascontiguousarray(px)
    return blocks_of(c, p, px.shape[0], host.ctypes.data, False)


def layout_blocks(c, p, px, lay, on_device=True, offset=0, seed=1):
    """the same samples in `lay` (device pixels `offset` bytes into their allocation, or host pixels)"""
    buf = X.pack(px, lay, seed)
    assert buf.size == G.pixel_bytes(p, lay, 0, 0, px.shape[0])
    c.set_pixel_layout(lay)
    try:
        if on_device:
            d = U.to_dev(np.concatenate([np.zeros(offset, np.uint8), buf]))
            return blocks_of(c, p, px.shape[0], d.data_ptr() + offset, True)
        return blocks_of(c, p, px.shape[0], buf.ctypes.data, False)
    finally:
        c.set_pixel_layout(None)


def same(a, b):
    assert a[0] == b[0], "block lengths differ"
    assert a[1] == b[1], "missing_msbs differ"
    assert a[2] == b[2], "block bytes differ"


IL = dict(interleaved=True)
# id: W, H, C, prec, levels, TileParams extras, layout, tiles
ENCODE_CASES = {
    # dwt53_pk_kernel, 128 lanes, two strips (both mirrored edge groups and an interior halo)
    "pk128-rgb": (512, 32, 3, 8, 3, {}, IL, 1),
    "pk128-mono": (512, 32, 1, 8, 3, {}, IL, 1),
    "pk128-4comp": (512, 32, 4, 8, 3, {}, IL, 1),                       # MCT triple + a fourth component on its own
    "pk128-3comp-nomct": (512, 32, 3, 8, 3, dict(mct=False), IL, 1),    # every component its own workgroup
    "pk128-rgbx": (512, 32, 3, 8, 3, {}, dict(interleaved=True, channels=4), 1),
    "pk128-rgbx-nomct": (512, 32, 3, 8, 2, dict(mct=False), dict(interleaved=True, channels=4), 1),
    "pk128-rgb-pitch": (512, 32, 3, 8, 3, {}, dict(interleaved=True, row_extra=13), 1),
    "pk128-rgbx-pitch": (512, 32, 3, 8, 3, {}, dict(interleaved=True, channels=4, row_extra=13), 1),
    "pk128-mono-pitch": (512, 32, 1, 8, 3, {}, dict(interleaved=True, row_extra=13), 1),
    "pk128-rgb-3tiles": (512, 32, 3, 8, 3, {}, dict(interleaved=True, row_extra=13, tile_extra=77), 3),
    # ... 256 lanes, three strips
    "pk256-rgb": (2052, 16, 3, 8, 2, {}, IL, 1),
    "pk256-rgbx": (2052, 16, 3, 8, 1, {}, dict(interleaved=True, channels=4, row_extra=13), 1),
    # dwt_level_kernel with int16 planes (FAST strips: even width; GEN: odd width)
    "h16-67x35": (67, 35, 3, 8, 2, {}, IL, 1),
    "h16-252x18": (252, 18, 3, 8, 2, {}, IL, 1),
    "h16-252x18-planar-pitch": (252, 18, 3, 8, 2, {}, dict(row_extra=13), 1),
    "pk-shape-planar-pitch": (512, 32, 3, 8, 3, {}, dict(row_extra=13, plane_extra=40, tile_extra=24), 3),
    # GEN path: odd sizes off the origin, two components (no fast shape of their own)
    "gen-61x47": (61, 47, 3, 8, 3, dict(origin=(3, 5)), dict(interleaved=True, row_extra=13), 1),
    "gen-2comp": (61, 47, 2, 8, 3, dict(mct=False), IL, 1),
    "gen-2comp-of-4": (256, 32, 2, 8, 2, dict(mct=False), dict(interleaved=True, channels=4), 1),
    "signed8": (96, 40, 3, 8, 2, dict(sgnd=True), IL, 1),
    # 16-bit pixels
    "p12-rev": (96, 40, 3, 12, 2, {}, dict(interleaved=True, row_extra=6), 1),
    "p16-rev": (96, 40, 3, 16, 2, {}, IL, 1),
    "p12-97": (96, 40, 3, 12, 2, dict(irreversible=True), dict(interleaved=True, channels=4), 1),
    "p16-97-mono": (61, 47, 1, 16, 3, dict(irreversible=True), dict(interleaved=True, row_extra=6), 1),
    "p12-rev-mono-signed": (61, 47, 1, 12, 3, dict(sgnd=True), IL, 1),
    "p16-planar-pitch": (96, 40, 3, 16, 2, {}, dict(row_extra=6, plane_extra=10, tile_extra=4), 3),
    "p8-97": (96, 40, 3, 8, 2, dict(irreversible=True), dict(interleaved=True, row_extra=13), 1),
    # no DWT level: ingest_kernel
    "ingest-8": (40, 24, 3, 8, 0, {}, dict(interleaved=True, row_extra=13), 1),
    "ingest-16": (40, 24, 3, 12, 0, {}, dict(interleaved=True, channels=4), 1),
    "ingest-8-planar-pitch": (40, 24, 3, 8, 0, {}, dict(row_extra=13, plane_extra=5, tile_extra=3), 3),
}


def make_layout(spec, C, H, W, bps):
    """row_extra / plane_extra / tile_extra: bytes beyond the tight pitch"""
    inter = bool(spec.get("interleaved"))
    ch = spec.get("channels", 0)
    n = (ch or C) if inter else 1
    row = W * n * bps + spec.get("row_extra", 0)
    plane = 0
    if not inter and ("plane_extra" in spec):
        plane = row * H + spec["plane_extra"]
    tile = 0
    if "tile_extra" in spec:
        tile = (row * H if inter else (plane or row * H) * C) + spec["tile_extra"]
    return G.PixelLayout.make(inter, ch, row_pitch=row if "row_extra" in spec else 0, plane_pitch=plane, tile_pitch=tile)


@pytest.mark.parametrize("case", list(ENCODE_CASES))
def test_encode_from_a_layout_equals_planar(case):
    W, H, C, prec, L, extra, spec, nt = ENCODE_CASES[case]
    p = G.TileParams.make(W, H, C, prec, L, **extra)
    px = content(C, H, W, prec, extra.get("sgnd", False), nt)
    lay = make_layout(spec, C, H, W, px.dtype.itemsize)
    c = U.ctx()
    want = planar_blocks(c, p, px)
    assert sum(want[0]) > 0
    same(layout_blocks(c, p, px, lay), want)


@pytest.mark.parametrize("spec", [dict(interleaved=True, row_extra=13), dict(interleaved=True, channels=4),
                                  dict(row_extra=13, plane_extra=40, tile_extra=24)], ids=["rgb-pitch", "rgbx", "planar-pitch"])
def test_host_pixels_in_a_layout(spec):
    """the extent grk_amd_pixel_bytes gives goes up as one copy, gaps included"""
    p = G.TileParams.make(512, 32, 3, 8, 3)
    px = content(3, 32, 512, 8, nt=2)
    c = U.ctx()
    same(layout_blocks(c, p, px, make_layout(spec, 3, 32, 512, 1), on_device=False), planar_blocks(c, p, px))


@pytest.mark.parametrize("spec,levels", [(IL, 3), (dict(interleaved=True, channels=4, row_extra=13), 3), (dict(row_extra=13), 3), (IL, 0)],
                         ids=["rgb", "rgbx-pitch", "planar-pitch", "rgb-no-level"])
def test_device_pixels_off_alignment(spec, levels):
    """an 8-bit device pointer one byte into its allocation: the separate ingest pass (ingest_kernel), then int32 planes"""
    p = G.TileParams.make(512, 32, 3, 8, levels)
    px = content(3, 32, 512, 8)
    c = U.ctx()
    same(layout_blocks(c, p, px, make_layout(spec, 3, 32, 512, 1), offset=1), planar_blocks(c, p, px))


def test_stage_ingest_follows_the_layout():
    p = G.TileParams.make(70, 33, 3, 8, 0)
    px = content(3, 33, 70, 8, nt=2)
    c = U.ctx()
    got = []
    for lay in (None, make_layout(dict(interleaved=True, channels=4, row_extra=13, tile_extra=9), 3, 33, 70, 1)):
        d_px = U.to_dev(X.pack(px, lay))
        d_pl = U.dev_planes(p, 6)
        c.set_pixel_layout(lay)
        try:
            c.stage_ingest_mct(p, 2, d_px.data_ptr(), d_pl.data_ptr())
            c.synchronize()
        finally:
            c.set_pixel_layout(None)
        got.append(U.planes_to_numpy(d_pl, p, 6).copy())
    assert np.array_equal(got[0], got[1])


@pytest.mark.parametrize("env", ["GRK_AMD_DWT_PK", "GRK_AMD_PLANES16"])
def test_switched_off_instances(env, monkeypatch):
    """without the packed kernel the interleaved level 0 is dwt_level_kernel's (int16 planes), without int16 planes its int32 form"""
    monkeypatch.setenv(env, "0")
    c = G.Context(0)
    try:
        p = G.TileParams.make(512, 32, 3, 8, 3)
        px = content(3, 32, 512, 8)
        want = planar_blocks(c, p, px)
        same(layout_blocks(c, p, px, make_layout(IL, 3, 32, 512, 1)), want)
        same(layout_blocks(c, p, px, make_layout(dict(interleaved=True, channels=4, row_extra=13), 3, 32, 512, 1)), want)
    finally:
        c.close()
    same(want, planar_blocks(U.ctx(), p, px))


@pytest.mark.parametrize("frame_streams", ["1", "0"])
def test_pipelined_frames_through_two_buffers(frame_streams, monkeypatch):
    """(a frame's whole chain on a stream of the context's own, or level 0 on the caller's stream beside the previous frame's block coder)
    Six interleaved frames of three contents rotate through two device buffers behind grk_amd_stream_wait_pixels (the refill is
    queued on torch's stream, which waits for the encoder's read of the buffer): every frame's blocks == the planar, un-pipelined ones."""
    p = G.TileParams.make(512, 32, 3, 8, 3)
    frames = [content(3, 32, 512, 8, seed=s) for s in (1, 2, 3)]
    lay = make_layout(dict(interleaved=True, row_extra=13), 3, 32, 512, 1)
    want = [planar_blocks(U.ctx(), p, f) for f in frames]
    packed = [torch.from_numpy(X.pack(f, lay, seed=5 + i)).pin_memory() for i, f in enumerate(frames)]
    monkeypatch.setenv("GRK_AMD_FRAME_STREAMS", frame_streams)
    c = G.Context(0)
    try:
        c.set_pipelining(True)
        c.set_pixel_layout(lay)
        bufs = [torch.empty(packed[0].numel(), dtype=torch.uint8, device="cuda") for _ in range(2)]
        mine = torch.cuda.Stream()
        c.set_stream(mine.cuda_stream)
        nb = len(want[0][0])
        for i in range(6):
            with torch.cuda.stream(mine):
                bufs[i % 2].copy_(packed[i % 3], non_blocking=True)      # (stream order: behind the read two frames ago ...)
            c.encode_tiles(p, 1, bufs[i % 2].data_ptr(), True, fetch=False)
            c.stream_wait_pixels(mine.cuda_stream)                       # (... and explicitly behind this frame's)
            table, tot = c.fetch_table(nb)
            coded = c.fetch_coded(tot)
            same((list(table["length"]), list(table["missing_msbs"]), U.split_blocks(table, coded)), want[i % 3])
        c.synchronize()
    finally:
        c.close()


def test_whole_image_in_a_layout():
    """grk_amd_encode_image of a 200 x 136 x 3 interleaved, pitched image -- ragged 128 x 64 tiles, and one tile: the planar call's file"""
    W, H = 200, 136
    px = content(3, H, W, 8)
    base = G.TileParams.make(128, 64, 3, 8, 3)
    c = U.ctx()
    for tw, th in ((128, 64), (None, None)):
        im = G.ImageLayout.make(W, H, tw, th)
        c.set_pixel_layout(None)
        want = c.encode_image(im, base, px[0])
        for spec in (IL, dict(interleaved=True, channels=4, row_extra=13), dict(row_extra=13, plane_extra=21)):
            lay = make_layout(spec, 3, H, W, 1)
            c.set_pixel_layout(lay)
            try:
                assert c.encode_image(im, base, X.pack(px, lay)) == want
            finally:
                c.set_pixel_layout(None)
    assert want[:2] == b"\xff\x4f"


def test_subsampled_image_refuses_a_layout():
    W, H = 64, 48
    base = G.TileParams.make(W, H, 3, 8, 2, mct=False)
    im = G.ImageLayout.make(W, H)
    planes = [content(1, H, W, 8)[0, 0], content(1, H, W // 2, 8)[0, 0], content(1, H, W // 2, 8)[0, 0]]
    c = U.ctx()
    c.set_pixel_layout(G.PixelLayout.make(True))
    try:
        with pytest.raises(RuntimeError, match=r"failed: %d " % UNSUPPORTED):
            c.encode_image_subsampled(im, base, [(1, 1), (2, 1), (2, 1)], planes)
    finally:
        c.set_pixel_layout(None)
    assert len(c.encode_image_subsampled(im, base, [(1, 1), (2, 1), (2, 1)], planes)) > 0


def test_invalid_layout_is_refused_and_null_restores():
    p = G.TileParams.make(512, 32, 3, 8, 3)
    px = content(3, 32, 512, 8)
    c = U.ctx()
    want = planar_blocks(c, p, px)
    d = U.to_dev(X.pack(px, G.PixelLayout.make(True, 4)))
    L = G.lib()
    for bad in (G.PixelLayout.make(True, 2), G.PixelLayout.make(True, 3, row_pitch=512 * 3 - 1), G.PixelLayout.make(True, 3, plane_pitch=1 << 20),
                G.PixelLayout.make(False, tile_pitch=100)):
        c.set_pixel_layout(bad)
        try:
            rc = L.grk_amd_encode_tiles(c._h, p, 1, d.data_ptr(), 1, None, None)
            assert rc == INVALID
            assert b"pixel layout" in L.grk_amd_last_error(c._h)
            d_pl = U.dev_planes(G.TileParams.make(512, 32, 3, 8, 0), 3)
            assert L.grk_amd_stage_ingest_mct(c._h, G.TileParams.make(512, 32, 3, 8, 0), 1, d.data_ptr(), d_pl.data_ptr()) == INVALID
            torch.cuda.synchronize()
            assert int(d_pl.abs().max()) == 0, "a refused call launched something"
        finally:
            c.set_pixel_layout(None)
    same(planar_blocks(c, p, px), want)


# ---- decode: the pixels a decode writes (grk_amd_set_decode_pixel_layout) ------------------------------------------------------------
# Oracle: the default-layout decode of the same table, put into the layout on the host (pixlayout.expected).  The destination starts
# as 0xA5 bytes: every gap byte has to be that still, every channel no component owns the layout's `fill`.
SENTINEL = 0xA5
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def smooth(C, H, W, nt=1):
    """low-contrast ramps: every coefficient stays far inside +-2047, what the packed inverse transform takes"""
    yy, xx = np.mgrid[0:H, 0:W]
    return np.stack([np.stack([(100 + 7 * k + 3 * t + ((xx // (5 + k)) + (yy // (3 + t))) % 23).astype(np.uint8) for k in range(C)])
                     for t in range(nt)])


def encoded(c, p, px):
    c.set_pixel_layout(None)
    table, coded = c.encode_host(p, np.ascontiguousarray(px), px.shape[0])
    return table, coded


def decode_into_layout(c, p, table, coded, nt, lay, on_device=True, want=None):
    """decodes into a sentinel-filled buffer in `lay`, compares with the planar decode (`want`, or made here)"""
    if want is None:
        c.set_decode_pixel_layout(None)
        want = c.decode_host(p, table, coded, nt)
    _, _, w, h = c.decode_size(p)
    fill = int(lay.fill) if lay is not None else 0
    exp = X.expected(want, lay, SENTINEL, fill)
    assert exp.size == G.pixel_bytes(p, lay, w, h, nt)
    if on_device:
        d = U.to_dev(np.full(exp.size, SENTINEL, np.uint8))
        d_coded = U.to_dev(coded)
        c.set_decode_pixel_layout(lay)
        try:
            c.decode_device(p, nt, table, d_coded.data_ptr(), coded.size, d.data_ptr())
            c.decode_status()              # OK: no value left the int16 planes -- the path taken first was the one that ran
        finally:
            c.set_decode_pixel_layout(None)
        got = d.cpu().numpy()
    else:
        got = c.decode_host(p, table, coded, nt, layout=lay, out=np.full(exp.size, SENTINEL, np.uint8))
    assert np.array_equal(got, exp), "samples, fill or gap bytes differ (first at byte %d)" % int(np.flatnonzero(got != exp)[0])
    return want


DECODE_LAYOUTS = {
    "rgb": dict(interleaved=True),
    "rgb-pitch13": dict(interleaved=True, row_extra=13),                  # rows on every alignment: the strided back end
    "rgb-pitch12": dict(interleaved=True, row_extra=12, tile_extra=40),   # aligned gaps: still whole-pixel-group stores
    "rgbx-255": dict(interleaved=True, channels=4, fill=255),
    "rgbx-pitch13": dict(interleaved=True, channels=4, row_extra=13, fill=7),
    "planar-pitch": dict(row_extra=13, plane_extra=9, tile_extra=5),
}


def decode_layout(spec, C, H, W, bps):
    lay = make_layout(spec, C, H, W, bps)
    lay.fill = spec.get("fill", 0)
    return lay


@pytest.mark.parametrize("lay", list(DECODE_LAYOUTS))
@pytest.mark.parametrize("W,H,L,nt", [(512, 32, 3, 2), (2052, 16, 2, 1)])
def test_decode_full_tile_packed_path(W, H, L, nt, lay):
    p = G.TileParams.make(W, H, 3, 8, L)
    px = smooth(3, H, W, nt)
    c = U.ctx()
    table, coded = encoded(c, p, px)
    want = decode_into_layout(c, p, table, coded, nt, decode_layout(DECODE_LAYOUTS[lay], 3, H, W, 1))
    assert np.array_equal(want, px)


@pytest.mark.parametrize("C,mct,spec", [(1, False, dict(interleaved=True)), (1, False, dict(interleaved=True, row_extra=12)),
                                        (4, True, dict(interleaved=True)), (3, False, dict(interleaved=True, channels=4, fill=9)),
                                        (2, False, dict(interleaved=True, channels=3, fill=200))],
                         ids=["mono", "mono-pitch", "4comp", "3comp-nomct-rgbx", "2comp-of-3"])
def test_decode_component_counts(C, mct, spec):
    p = G.TileParams.make(512, 32, C, 8, 3, mct=mct)
    px = smooth(C, 32, 512)
    c = U.ctx()
    table, coded = encoded(c, p, px)
    assert np.array_equal(decode_into_layout(c, p, table, coded, 1, decode_layout(spec, C, 32, 512, 1)), px)


@pytest.mark.parametrize("case", ["gen-61x47", "gen-2comp", "h16-67x35", "signed8", "p12-rev", "p16-rev", "p12-97", "p16-97-mono", "p12-rev-mono-signed",
                                  "p8-97", "ingest-8", "ingest-16"])
@pytest.mark.parametrize("on_device", [True, False], ids=["device", "host"])
def test_decode_32bit_paths(case, on_device):
    """odd sizes off the origin, 16-bit samples, 9/7, signed samples, no DWT level (egress_kernel): the encode cases' tables"""
    W, H, C, prec, L, extra, spec, nt = ENCODE_CASES[case]
    p = G.TileParams.make(W, H, C, prec, L, **extra)
    px = content(C, H, W, prec, extra.get("sgnd", False), nt)
    c = U.ctx()
    table, coded = encoded(c, p, px)
    bps = px.dtype.itemsize
    lay = decode_layout(dict(spec, fill=0x1234 if bps == 2 else 0x5B), C, H, W, bps)
    want = decode_into_layout(c, p, table, coded, nt, lay, on_device).view(px.dtype)
    if not extra.get("irreversible"):
        assert np.array_equal(want, px)


@pytest.mark.parametrize("levels", [3, 0])
def test_decode_with_separate_egress(levels, monkeypatch):
    monkeypatch.setenv("GRK_AMD_FUSE_EGRESS", "0")
    c = G.Context(0)
    try:
        p = G.TileParams.make(96, 40, 3, 8, levels)
        px = content(3, 40, 96, 8, nt=2)
        table, coded = encoded(c, p, px)
        for spec in (dict(interleaved=True, channels=4, fill=255, row_extra=13, tile_extra=3), dict(row_extra=13, plane_extra=2)):
            assert np.array_equal(decode_into_layout(c, p, table, coded, 2, decode_layout(spec, 3, 40, 96, 1)), px)
    finally:
        c.close()


def test_stage_egress_follows_the_layout():
    p = G.TileParams.make(70, 33, 3, 8, 0)
    rng = np.random.default_rng(3)
    planes = rng.integers(-100, 100, size=(6, 33, 70)).astype(np.int32)
    c = U.ctx()
    d_pl = U.upload_planes(planes, p)
    d0 = U.to_dev(np.zeros(6 * 33 * 70, np.uint8))
    c.stage_egress(p, 2, d_pl.data_ptr(), d0.data_ptr())
    c.synchronize()
    want = d0.cpu().numpy().reshape(2, 3, 33, 70)
    lay = decode_layout(dict(interleaved=True, channels=4, row_extra=13, tile_extra=9, fill=33), 3, 33, 70, 1)
    exp = X.expected(want, lay, SENTINEL, 33)
    d1 = U.to_dev(np.full(exp.size, SENTINEL, np.uint8))
    c.set_decode_pixel_layout(lay)
    try:
        c.stage_egress(p, 2, d_pl.data_ptr(), d1.data_ptr())
        c.synchronize()
    finally:
        c.set_decode_pixel_layout(None)
    assert np.array_equal(d1.cpu().numpy(), exp)


@pytest.mark.parametrize("spec", [dict(interleaved=True, row_extra=13), dict(interleaved=True, channels=4, fill=255), dict(row_extra=13, plane_extra=7)],
                         ids=["rgb-pitch", "rgbx", "planar-pitch"])
def test_decode_region_of_an_odd_window(spec):
    p = G.TileParams.make(96, 64, 3, 8, 3)
    px = content(3, 64, 96, 8)
    c = U.ctx()
    table, coded = encoded(c, p, px)
    x0, y0, x1, y1 = 5, 3, 59, 41
    c.set_decode_pixel_layout(None)
    want = c.decode_region_host(p, table, coded, x0, y0, x1, y1)
    assert np.array_equal(want, px[0][:, y0:y1, x0:x1])
    lay = decode_layout(spec, 3, y1 - y0, x1 - x0, 1)
    exp = X.expected(want[None], lay, SENTINEL, int(lay.fill))
    got = c.decode_region_host(p, table, coded, x0, y0, x1, y1, layout=lay, out=np.full(exp.size, SENTINEL, np.uint8))
    assert np.array_equal(got, exp)
    d = U.to_dev(np.full(exp.size, SENTINEL, np.uint8))
    d_coded = U.to_dev(coded)
    c.set_decode_pixel_layout(lay)
    try:
        c.decode_region_device(p, table, d_coded.data_ptr(), coded.size, x0, y0, x1, y1, d.data_ptr())
        c.decode_status()
    finally:
        c.set_decode_pixel_layout(None)
    assert np.array_equal(d.cpu().numpy(), exp)


def test_decode_at_reduced_resolution():
    p = G.TileParams.make(96, 64, 3, 8, 3)
    px = content(3, 64, 96, 8, nt=2)
    c = U.ctx()
    table, coded = encoded(c, p, px)
    c.set_decode_reduce(1)
    try:
        assert c.decode_size(p)[2:] == (48, 32)
        for spec in (dict(interleaved=True, row_extra=13, tile_extra=11), dict(interleaved=True, channels=4, fill=255)):
            for on_device in (True, False):
                decode_into_layout(c, p, table, coded, 2, decode_layout(spec, 3, 32, 48, 1), on_device)
    finally:
        c.set_decode_reduce(0)


def test_decode_sequence_with_two_frames_in_flight():
    p = G.TileParams.make(512, 32, 3, 8, 3)
    frames = [smooth(3, 32, 512) + np.uint8(5 * i) for i in range(4)]
    c0 = U.ctx()
    enc = [encoded(c0, p, f) for f in frames]
    lay = decode_layout(dict(interleaved=True, channels=4, fill=255, row_extra=16), 3, 32, 512, 1)
    exp = [X.expected(f, lay, SENTINEL, 255) for f in frames]
    c = G.Context(0)
    try:
        c.set_decode_pipelining(2)
        c.set_decode_pixel_layout(lay)
        outs = [U.to_dev(np.full(exp[0].size, SENTINEL, np.uint8)) for _ in frames]
        codeds = [U.to_dev(e[1]) for e in enc]
        for i in range(4):
            c.decode_device(p, 1, enc[i][0], codeds[i].data_ptr(), enc[i][1].size, outs[i].data_ptr())
        c.synchronize()
        c.decode_status()
        for i in range(4):
            assert np.array_equal(outs[i].cpu().numpy(), exp[i]), "frame %d" % i
    finally:
        c.close()


@pytest.mark.parametrize("name", ["dec_p1_rev_3x100x77_r3", "g2_3x256x256_t128_r4"])
def test_decode_image_of_golden_streams(name):
    """a Part-1 stream of one tile (straight into the destination) and a tiled HT one (tight tiles in the layout, placed by rows of pixels)"""
    cs = open(os.path.join(GOLD, name + ".j2k"), "rb").read()
    c = U.ctx()
    want = c.decode_image(cs)
    C, H, W = want.shape
    for spec in (dict(interleaved=True, channels=4, fill=255, row_extra=13), dict(interleaved=True), dict(row_extra=13, plane_extra=3)):
        lay = decode_layout(spec, C, H, W, want.dtype.itemsize)
        exp = X.expected(want[None], lay, SENTINEL, int(lay.fill))
        assert np.array_equal(c.decode_image(cs, layout=lay, out=np.full(exp.size, SENTINEL, np.uint8)), exp)
        d = U.to_dev(np.full(exp.size, SENTINEL, np.uint8))
        c.set_decode_pixel_layout(lay)
        try:
            c.decode_image_device(cs, d.data_ptr(), exp.size)
            c.decode_status()
        finally:
            c.set_decode_pixel_layout(None)
        assert np.array_equal(d.cpu().numpy(), exp)
    assert np.array_equal(c.decode_image(cs), want)


def test_whole_image_round_trip_in_a_layout():
    """the files test_whole_image_in_a_layout compares, decoded into an interleaved, pitched destination == the planar result transposed"""
    W, H = 200, 136
    px = synth.g2(3, H, W, 8)[None]
    base = G.TileParams.make(128, 64, 3, 8, 3)
    c = U.ctx()
    for tw, th in ((128, 64), (None, None)):
        cs = c.encode_image(G.ImageLayout.make(W, H, tw, th), base, px[0])
        want = c.decode_image(cs)
        assert np.array_equal(want, px[0])
        for spec in (dict(interleaved=True, row_extra=13), dict(interleaved=True, channels=4, fill=255, row_extra=24)):
            lay = decode_layout(spec, 3, H, W, 1)
            exp = X.expected(want[None], lay, SENTINEL, int(lay.fill))
            assert np.array_equal(c.decode_image(cs, layout=lay, out=np.full(exp.size, SENTINEL, np.uint8)), exp)


def test_invalid_decode_layout_is_refused_and_null_restores():
    p = G.TileParams.make(96, 40, 3, 8, 2)
    px = content(3, 40, 96, 8)
    c = U.ctx()
    table, coded = encoded(c, p, px)
    d = U.to_dev(np.full(96 * 40 * 4 + 64, SENTINEL, np.uint8))
    d_coded = U.to_dev(coded)
    L = G.lib()
    t = np.ascontiguousarray(table)
    for bad in (G.PixelLayout.make(True, 2), G.PixelLayout.make(True, 3, row_pitch=96 * 3 - 1), G.PixelLayout.make(True, 3, plane_pitch=1 << 20),
                G.PixelLayout.make(False, plane_pitch=96 * 40 - 1)):
        c.set_decode_pixel_layout(bad)
        try:
            assert L.grk_amd_decode_tiles(c._h, p, 1, t.ctypes.data, d_coded.data_ptr(), coded.size, 1, d.data_ptr(), 1) == INVALID
            assert b"pixel layout" in L.grk_amd_last_error(c._h)
            assert L.grk_amd_decode_region(c._h, p, t.ctypes.data, d_coded.data_ptr(), coded.size, 1, 0, 0, 96, 40, d.data_ptr(), 1) == INVALID
        finally:
            c.set_decode_pixel_layout(None)
        torch.cuda.synchronize()
        assert int((d != SENTINEL).sum()) == 0, "a refused call wrote pixels"
    assert np.array_equal(c.decode_host(p, table, coded), px)
