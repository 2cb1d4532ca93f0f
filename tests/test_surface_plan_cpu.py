"""CPU: the host planning of grk_amd_encode_surface / grk_amd_decode_surface (grok_amd/csrc/surface_plan.cpp) -- the named formats
against offsets, pitches and extents worked out here from the component sizes, the extent of a surface and the reason text of every
refusal, the rule that two components of a destination share no byte, and which route the plan picks for each run."""
import pytest

import grok_amd as G

UNSUPPORTED, INVALID, OVERFLOW = -2, -3, -5
S420, S422, S444 = [(1, 1), (2, 2), (2, 2)], [(1, 1), (2, 1), (2, 1)], [(1, 1)] * 3
SAMPLING = {"NV12": S420, "NV21": S420, "I420": S420, "YV12": S420, "NV16": S422, "I422": S422, "I444": S444}


def cdiv(a, b):
    return (a + b - 1) // b


def comp_size(layout, dx, dy):
    return cdiv(layout.x1, dx) - cdiv(layout.x0, dx), cdiv(layout.y1, dy) - cdiv(layout.y0, dy)


def roundup(a, b):
    return cdiv(a, b) * b


def expected_format(fmt, layout, prec, pitch):
    """[(offset, row_pitch, step)], extent -- from the definitions of the formats"""
    bps = (prec + 7) // 8
    W, H = layout.x1 - layout.x0, layout.y1 - layout.y0
    (dx, dy) = SAMPLING[fmt][1]
    wc, hc = comp_size(layout, dx, dy)
    pairs = fmt in ("NV12", "NV21", "NV16")
    if not pitch:
        pitch = max(W, 2 * wc if pairs else 0) * bps
    chroma = H * pitch
    if pairs:
        first, second = (chroma, pitch, 2), (chroma + bps, pitch, 2)
        extent = chroma + (hc - 1) * pitch + 2 * wc * bps
    else:
        cp = pitch if fmt == "I444" else roundup(cdiv(pitch, 2), bps)
        first, second = (chroma, cp, 1), (chroma + hc * cp, cp, 1)
        extent = chroma + hc * cp + (hc - 1) * cp + wc * bps
    cb, cr = (second, first) if fmt in ("NV21", "YV12") else (first, second)
    return [(0, pitch, 1), cb, cr], extent


@pytest.mark.parametrize("fmt", sorted(G.SURFACE_FORMATS))
@pytest.mark.parametrize("size", [(202, 138), (7, 5)])
@pytest.mark.parametrize("origin", [(0, 0), (5, 3)])
def test_named_formats(fmt, size, origin):
    layout = G.ImageLayout.make(*size, offset=origin)
    for prec in (8, 12):
        bps = (prec + 7) // 8
        for pitch in (0, roundup(size[0] + 1, 2) * bps + 6 * bps):
            s, sampling, nbytes = G.Surface.make(fmt, layout, prec, pitch)
            want, extent = expected_format(fmt, layout, prec, pitch)
            assert sampling == SAMPLING[fmt]
            assert [(c.offset, c.row_pitch, c.step) for c in s.comp[:3]] == want, (fmt, prec, pitch)
            assert nbytes == extent
            base = G.TileParams.make(1, 1, 3, prec, 2, mct=False)
            assert G.surface_bytes(layout, base, sampling, s) == extent
            # a destination in this format is accepted, and the plan counts its runs
            assert len(G.surface_plan(layout, base, sampling, s, extent, decode=True)) == (1 if fmt == "I444" else 2)
            # (the number of the format works like its name)
            s2, _, n2 = G.Surface.make(G.SURFACE_FORMATS[fmt], layout, prec, pitch)
            assert bytes(s2) == bytes(s) and n2 == nbytes


def test_format_refusals():
    layout = G.ImageLayout.make(202, 138)
    with pytest.raises(G.SurfaceError) as e:
        G.Surface.make("NV12", layout, 8, 201)               # a pitch below a row
    assert e.value.code == INVALID
    with pytest.raises(G.SurfaceError) as e:
        G.Surface.make("NV12", layout, 12, 405)              # ... no multiple of the sample size
    assert e.value.code == INVALID
    with pytest.raises(G.SurfaceError) as e:
        G.Surface.make("NV12", layout, 17, 0)
    assert e.value.code == UNSUPPORTED
    with pytest.raises(G.SurfaceError) as e:
        G.Surface.make(7, layout, 8, 0)
    assert e.value.code == INVALID


def test_surface_bytes_and_reasons():
    layout = G.ImageLayout.make(202, 138)
    p8 = G.TileParams.make(1, 1, 3, 8, 2, mct=False)
    p12 = G.TileParams.make(1, 1, 3, 12, 2, mct=False)
    nv12 = [(0, 256, 1), (138 * 256, 256, 2), (138 * 256 + 1, 256, 2)]
    assert G.surface_bytes(layout, p8, S420, G.Surface.of(nv12)) == 138 * 256 + 68 * 256 + 202
    # pitch 0 = tight: ((w - 1) * step + 1) * bps; step 0 reads as 1
    assert G.surface_bytes(layout, p8, S420, G.Surface.of([(0, 0, 0), (27876, 0, 2), (50000, 0, 2)])) == 50000 + 68 * 201 + 201
    assert G.surface_bytes(layout, p12, S420, G.Surface.of([(0, 0, 1), (60000, 0, 1), (80000, 0, 4)])) == 80000 + 68 * 802 + 802

    def refused(base, comps, code, text):
        with pytest.raises(G.SurfaceError) as e:
            G.surface_bytes(layout, base, S420, G.Surface.of(comps))
        assert e.value.code == code and text in e.value.reason, e.value.reason
        with pytest.raises(G.SurfaceError) as e:
            G.surface_plan(layout, base, S420, G.Surface.of(comps), 1 << 30)
        assert e.value.code == code and text in e.value.reason

    refused(p8, [(0, 201, 1)] + nv12[1:], INVALID, "a row pitch is smaller than a row")
    refused(p8, [nv12[0], (138 * 256, 200, 2), nv12[2]], INVALID, "a row pitch is smaller than a row")       # ((101 - 1) * 2 + 1 = 201)
    refused(p12, [(0, 405, 1), (70000, 404, 2), (70002, 404, 2)], INVALID, "a row pitch is no multiple of the sample size")
    refused(p12, [(0, 404, 1), (70001, 404, 2), (70003, 404, 2)], INVALID, "an offset is no multiple of the sample size")
    refused(p8, [nv12[0], (138 * 256, 1024, 5), nv12[2]], INVALID, "a step above 4")
    refused(G.TileParams.make(1, 1, 3, 17, 2, mct=False), [(0, 0, 1), (200000, 0, 1), (300000, 0, 1)], UNSUPPORTED, "more than 16 bits")
    # cap: the extent fits exactly, one byte less does not
    s = G.Surface.of(nv12)
    n = G.surface_bytes(layout, p8, S420, s)
    assert len(G.surface_plan(layout, p8, S420, s, n)) == 2
    for decode in (False, True):
        with pytest.raises(G.SurfaceError) as e:
            G.surface_plan(layout, p8, S420, s, n - 1, decode=decode)
        assert e.value.code == OVERFLOW and "does not fit" in e.value.reason


def test_overlap_rule_is_for_destinations():
    layout = G.ImageLayout.make(202, 138)
    p = G.TileParams.make(1, 1, 3, 8, 2, mct=False)
    Y = (0, 256, 1)
    at = 138 * 256

    def check(comps, ok, sampling=S420):
        s = G.Surface.of(comps)
        assert len(G.surface_plan(layout, p, sampling, s, 1 << 30, decode=False)) >= 1           # an encode only reads
        if ok:
            assert len(G.surface_plan(layout, p, sampling, s, 1 << 30, decode=True)) >= 1
        else:
            with pytest.raises(G.SurfaceError) as e:
                G.surface_plan(layout, p, sampling, s, 1 << 30, decode=True)
            assert e.value.code == INVALID and "share bytes" in e.value.reason

    check([Y, (at, 256, 2), (at + 1, 256, 2)], True)                 # interleaved partners
    check([Y, (at + 1, 256, 2), (at, 256, 2)], True)                 # ... Cr first
    check([Y, (at, 202, 2), (at + 1, 202, 2)], True)                 # ... in the tightest pitch that holds both
    check([Y, (at, 201, 2), (at + 1, 201, 2)], False)                # Cr's last sample of a row is Cb's first of the next
    check([Y, (at, 256, 1), (at + 128, 256, 1)], True)               # side by side inside one pitch (101 + 101 <= 256)
    check([Y, (at, 256, 1), (at + 100, 256, 1)], False)              # ... one column too close
    check([Y, (at, 256, 1), (at + 200, 256, 1)], False)              # ... wrapping into the next row
    check([Y, (202, 256, 1), (at, 256, 1)], False)                   # Cb beside Y, but 202 + 101 > 256
    check([(0, 512, 1), (256, 512, 1), (256 + 128, 512, 1)], True)   # all three side by side
    check([Y, (at, 300, 1), (at + 150, 200, 1)], False)              # rows that interlock with different pitches
    check([Y, (at, 256, 2), (at, 256, 2)], False)                    # Cb on top of Cr
    check([Y, (at, 256, 1), (at, 256, 1)], False)
    check([Y, (at, 256, 2), (at + 2, 256, 2)], False)                # partners a whole step apart: the same bytes, shifted
    check([Y, (at, 1024, 4), (at + 3, 1024, 4)], True)               # partners three bytes apart of a step of four
    check([Y, (at, 256, 2), (at + 1 + 256 * 69, 256, 2)], True)      # disjoint extents


def routes(layout, base, sampling, surface, decode, cap=1 << 30, **kw):
    return [r[0] for r in G.surface_plan(layout, base, sampling, surface, cap, decode=decode, **kw)]


def test_routes():
    one = G.ImageLayout.make(202, 138)
    tiled = G.ImageLayout.make(202, 138, 101, 69)                  # 2 x 2 tiles
    p = G.TileParams.make(1, 1, 3, 8, 3, mct=False)
    for decode in (False, True):
        s, sampling, n = G.Surface.make("NV12", one, 8, 256)
        plan = G.surface_plan(one, p, sampling, s, n, decode=decode)
        assert [r[0] for r in plan] == [True, True]                # NV12, one tile, aligned: both runs in place
        (_, ly, aty), (_, lc, atc) = plan
        assert (ly.interleaved, ly.row_pitch, ly.plane_pitch, aty) == (0, 256, 0, 0)                   # Y: a pitched plane
        assert (lc.interleaved, lc.channels, lc.row_pitch, atc) == (1, 2, 256, 138 * 256)              # Cb/Cr: two-channel pixels
        assert routes(one, p, sampling, s, decode, n, allow_direct=False) == [False, False]
        assert routes(tiled, p, sampling, s, decode, n) == [False, False]                              # any 2 x 2-tile image: all staged
        s, sampling, n = G.Surface.make("NV21", one, 8, 256)
        assert routes(one, p, sampling, s, decode, n) == [True, False]                                 # reversed pairs: chroma staged
        s, sampling, n = G.Surface.make("YV12", one, 8, 256)
        assert routes(one, p, sampling, s, decode, n) == [True, False]                                 # V plane first: chroma staged
        s, sampling, n = G.Surface.make("I420", one, 8, 256)
        plan = G.surface_plan(one, p, sampling, s, n, decode=decode)
        assert [r[0] for r in plan] == [True, True]
        assert (plan[1][1].interleaved, plan[1][1].row_pitch, plan[1][1].plane_pitch, plan[1][2]) == (0, 128, 69 * 128, 138 * 256)
        assert routes(tiled, p, sampling, s, decode, n) == [False, False]
        # a plane pitch below a plane's span is no layout
        s = G.Surface.of([(0, 256, 1), (40192, 256, 1), (40320, 256, 1)])
        assert routes(one, p, S420, s, decode) == [True, False]
    # a surface base off 4-byte alignment: staged on decode, in place on encode
    s, sampling, n = G.Surface.make("NV12", one, 8, 256)
    for align in (1, 2, 3):
        assert routes(one, p, sampling, s, True, n, base_align=align) == [False, False]
        assert routes(one, p, sampling, s, False, n, base_align=align) == [True, True]
    # ... and an offset that brings the first sample back onto it
    s = G.Surface.of([(3, 256, 1), (40003, 256, 2), (40004, 256, 2)])
    assert routes(one, p, S420, s, True, base_align=1) == [True, True]
    assert routes(one, p, S420, s, True, base_align=0) == [False, False]
    # 16-bit samples: an encode needs the first sample on an even address
    p12 = G.TileParams.make(1, 1, 3, 12, 3, mct=False)
    s, sampling, n = G.Surface.make("NV12", one, 12, 512)
    assert routes(one, p12, sampling, s, False, n, base_align=1) == [False, False]
    assert routes(one, p12, sampling, s, False, n, base_align=2) == [True, True]
    assert routes(one, p12, sampling, s, True, n, base_align=2) == [False, False]
    # a lone Cb inside pairs (Cr elsewhere, at another size): in place on encode with channels = 2, staged on decode
    lone = [(1, 1), (2, 2), (2, 1)]
    s = G.Surface.of([(0, 256, 1), (40000, 256, 2), (80000, 256, 1)])
    plan = G.surface_plan(one, p, lone, s, 1 << 30, decode=False)
    assert [r[0] for r in plan] == [True, True, True] and (plan[1][1].interleaved, plan[1][1].channels) == (1, 2)
    assert routes(one, p, lone, s, True) == [True, False, True]
    # ... but not where the skipped channel of the last pixel lies beyond `cap`, nor in a pitch that holds no whole pixels
    last = G.Surface.of([(0, 256, 1), (40000, 256, 1), (80000, 256, 2)])
    n = G.surface_bytes(one, p, lone, last)
    assert n == 80000 + 137 * 256 + 201
    assert routes(one, p, lone, last, False, n) == [True, True, False]
    assert routes(one, p, lone, last, False, n + 1) == [True, True, True]
    assert routes(one, p, lone, G.Surface.of([(0, 256, 1), (40000, 201, 2), (80000, 256, 1)]), False) == [True, False, True]
    # RGBX-style: step 4, all factors 1 -- in place on encode (X skipped) where the last pixel's X is inside `cap`, staged on decode
    rgbx = G.Surface.of([(0, 1024, 4), (1, 1024, 4), (2, 1024, 4)])
    pm = G.TileParams.make(1, 1, 3, 8, 3, mct=True)
    plan = G.surface_plan(one, pm, S444, rgbx, 138 * 1024, decode=False)
    assert [r[0] for r in plan] == [True] and (plan[0][1].interleaved, plan[0][1].channels, plan[0][1].row_pitch) == (1, 4, 1024)
    assert routes(one, pm, S444, rgbx, True, 138 * 1024) == [False]
    assert routes(one, pm, S444, G.Surface.of([(0, 606, 3), (1, 606, 3), (2, 606, 3)]), True) == [True]      # RGB pixels: both ways
    assert routes(one, pm, S444, G.Surface.of([(2, 606, 3), (1, 606, 3), (0, 606, 3)]), False) == [False]    # BGR: staged
