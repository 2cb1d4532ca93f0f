"""CPU: grk_amd_pixel_bytes -- the extent of a pixel buffer in a layout, and the layouts it refuses."""
import itertools

import pytest

import grok_amd as G
import pixlayout as X


def layouts(C, H, W, bps):
    """tight and pitched, planar and interleaved (channels 0 / 3 / 4 where they can hold C components)"""
    yield None
    yield G.PixelLayout.make()
    yield G.PixelLayout.make(row_pitch=W * bps + 13 * bps)
    yield G.PixelLayout.make(row_pitch=W * bps + 6, plane_pitch=(W * bps + 6) * (H + 3))
    yield G.PixelLayout.make(plane_pitch=W * bps * H + 2 * bps, tile_pitch=(W * bps * H + 2 * bps) * C + 64)
    yield G.PixelLayout.make(tile_pitch=C * H * W * bps + 128)
    for ch in (0, 3, 4):
        if ch and ch < C:
            continue
        n = ch or C
        yield G.PixelLayout.make(True, ch)
        yield G.PixelLayout.make(True, ch, row_pitch=W * n * bps + 13 * bps)
        yield G.PixelLayout.make(True, ch, row_pitch=W * n * bps + 6, tile_pitch=(W * n * bps + 6) * (H + 1))
        yield G.PixelLayout.make(True, ch, tile_pitch=W * n * bps * H + 4 * bps)


@pytest.mark.parametrize("prec,C", list(itertools.product((8, 12, 16), (1, 2, 3, 4))))
def test_pixel_bytes_is_the_extent(prec, C):
    bps = (prec + 7) // 8
    p = G.TileParams.make(40, 24, C, prec, 2, mct=False)
    n = 0
    for lay in layouts(C, 24, 40, bps):
        for nt in (1, 3):
            assert G.pixel_bytes(p, lay, 0, 0, nt) == X.extent(lay, nt, C, 24, 40, bps), (lay and [getattr(lay, f) for f, _ in lay._fields_], nt)
            n += 1
    # an explicit size (what a region or reduced decode, or a whole image, passes): pitches sized for it
    for lay in layouts(C, 7, 61, bps):
        for nt in (1, 3):
            assert G.pixel_bytes(p, lay, 61, 7, nt) == X.extent(lay, nt, C, 7, 61, bps)
            n += 1
    assert n >= 24
    assert G.pixel_bytes(p, None, 0, 0, 3) == 3 * C * 24 * 40 * bps          # the default: tight planes back to back


def test_pixel_bytes_refuses_invalid_layouts():
    W, H = 40, 24
    p8 = G.TileParams.make(W, H, 3, 8, 2)
    p16 = G.TileParams.make(W, H, 3, 12, 2)
    mk = G.PixelLayout.make
    bad8 = [mk(True, 2),                                    # channels below num_comps
            mk(True, 5),                                    # ... above 4
            mk(True, 3, row_pitch=W * 3 - 1),               # a row pitch smaller than a row
            mk(True, 4, row_pitch=W * 4 - 1),
            mk(False, row_pitch=W - 1),
            mk(False, plane_pitch=W * H - 1),               # a plane pitch smaller than a plane
            mk(False, row_pitch=W + 8, plane_pitch=(W + 8) * (H - 1) + W - 1),
            mk(False, tile_pitch=3 * W * H - 1),            # a tile pitch smaller than a tile
            mk(True, 3, tile_pitch=3 * W * H - 1),
            mk(True, 3, plane_pitch=3 * W * H)]             # plane_pitch together with interleaved
    for lay in bad8:
        assert G.pixel_bytes(p8, lay, 0, 0, 2) == 0, [getattr(lay, f) for f, _ in lay._fields_]
    bad16 = [mk(False, row_pitch=2 * W + 1),                # pitches that are no multiple of the sample size
             mk(True, 3, row_pitch=6 * W + 3),
             mk(False, plane_pitch=2 * W * H + 1),
             mk(False, tile_pitch=6 * W * H + 1),
             mk(True, 0, tile_pitch=6 * W * H + 1)]
    for lay in bad16:
        assert G.pixel_bytes(p16, lay, 0, 0, 2) == 0, [getattr(lay, f) for f, _ in lay._fields_]
        lay8 = mk(lay.interleaved, lay.channels, lay.row_pitch // 2, lay.plane_pitch // 2, lay.tile_pitch // 2)
        assert G.pixel_bytes(p8, lay8, 0, 0, 2) != 0        # (the same shape in 8-bit samples is fine)
    # the smallest valid pitches are valid: the last row / plane / tile ends where its samples end
    assert G.pixel_bytes(p8, mk(False, row_pitch=W + 8, plane_pitch=(W + 8) * (H - 1) + W), 0, 0, 2) == \
        X.extent(mk(False, row_pitch=W + 8, plane_pitch=(W + 8) * (H - 1) + W), 2, 3, H, W, 1)
    assert G.pixel_bytes(p8, mk(True, 4), 0, 0, 0) == 0     # no tiles
