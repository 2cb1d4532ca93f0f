"""Pixel layouts (grk_amd_pixel_layout) restated in numpy for the tests: where every sample of a batch of tiles lies, the extent of
the buffer, and buffers in a layout whose gaps and skipped channels hold random bytes."""
import numpy as np


def sample_offsets(layout, ntiles, C, H, W, bps):
    """Byte offset of sample (tile, component, y, x), an int64 array (ntiles, C, H, W) -- the header's definition, field by field."""
    if layout is None:
        inter, ch, row, plane, tile = 0, 0, 0, 0, 0
    else:
        inter, ch, row, plane, tile = (int(layout.interleaved), int(layout.channels), int(layout.row_pitch), int(layout.plane_pitch),
                                       int(layout.tile_pitch))
    t, k, y, x = np.ogrid[0:ntiles, 0:C, 0:H, 0:W]
    if inter:
        ch = ch or C
        row = row or W * ch * bps
        tile = tile or H * row
        return (t * tile + y * row + (x * ch + k) * bps).astype(np.int64)
    row = row or W * bps
    plane = plane or H * row
    tile = tile or C * plane
    return (t * tile + k * plane + y * row + x * bps).astype(np.int64)


def extent(layout, ntiles, C, H, W, bps):
    """first sample .. end of the last one; interleaved: of the last PIXEL, the channels an encode skips included (they are memory
    the buffer has, and whole pixels are what the kernels load)"""
    if layout is not None and layout.interleaved:
        C = int(layout.channels) or C
    return int(sample_offsets(layout, ntiles, C, H, W, bps).max()) + bps


def pack(px, layout, seed=1):
    """px: (ntiles, C, H, W) uint8 / int8 / uint16 / int16 -> a uint8 buffer of the layout's extent holding those samples (host
    endian), every other byte random (fixed seed)."""
    nt, C, H, W = px.shape
    bps = px.dtype.itemsize
    off = sample_offsets(layout, nt, C, H, W, bps)
    buf = np.random.default_rng(seed).integers(0, 256, size=extent(layout, nt, C, H, W, bps), dtype=np.uint8)
    raw = np.ascontiguousarray(px).view(np.uint8).reshape(nt, C, H, W, bps)
    for b in range(bps):
        buf[off + b] = raw[..., b]
    return buf


def expected(px, layout, sentinel, fill=0):
    """What a decode of `px` (ntiles, C, H, W) into a buffer pre-filled with the byte `sentinel` has to leave: the samples in their
    places, `fill` (a sample) in the channels of interleaved pixels that no component owns, every other byte the sentinel."""
    nt, C, H, W = px.shape
    bps = px.dtype.itemsize
    buf = np.full(extent(layout, nt, C, H, W, bps), sentinel, np.uint8)
    ch = C
    if layout is not None and layout.interleaved:
        ch = int(layout.channels) or C
    allp = np.empty((nt, ch, H, W), px.dtype)
    allp[:, :C] = px
    allp[:, C:] = np.array(fill).astype(px.dtype)
    off = sample_offsets(layout, nt, ch, H, W, bps)
    raw = np.ascontiguousarray(allp).view(np.uint8).reshape(nt, ch, H, W, bps)
    for b in range(bps):
        buf[off + b] = raw[..., b]
    return buf
