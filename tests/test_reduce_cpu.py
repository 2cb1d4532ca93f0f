"""CPU: decode at reduced resolution (grk_decompress -r N) -- the reduced tile's rectangle against the reference's header, and the
reference's reduced decode pinned to something independent of it (its own forward 5/3 and RCT)."""

import numpy as np
import pytest

import grok_amd as G
import j2kparse as J
import reducehost as RH
import refharness as R
import synth

needs_ref = pytest.mark.skipif(not RH.have(), reason="oracle/_ref not built")

# C, H, W, prec, numres, image origin
SHAPES = [(1, 64, 64, 8, 4, (0, 0)), (3, 61, 77, 8, 5, (0, 0)), (1, 37, 129, 12, 6, (5, 3)), (3, 50, 33, 8, 3, (7, 9)),
          (1, 100, 70, 8, 5, (13, 31)), (3, 8, 9, 8, 4, (1, 2))]


def _stream(monkeypatch, C_, H, W, prec, numres, off, **kw):
    monkeypatch.setenv("REF_IMG_X0", str(off[0]))
    monkeypatch.setenv("REF_IMG_Y0", str(off[1]))
    px = synth.g2(C_, H, W, prec)
    cs, _ = R.encode(px, prec, TW=off[0] + W, TH=off[1] + H, numres=numres, mode=1, **kw)    # one tile: the whole grid
    return px, cs


def _params(cs):
    info = J.parse(cs)
    return G.TileParams.make(info["W"], info["H"], info["C"], info["prec"], info["levels"],
                             irreversible=bool(info["irreversible"]), mct=bool(info["mct"]), origin=(info["x0"], info["y0"]))


@needs_ref
@pytest.mark.parametrize("C_,H,W,prec,numres,off", SHAPES)
def test_reduced_tile_rect_matches_reference_header(monkeypatch, C_, H, W, prec, numres, off):
    """grk_amd_reduced_tile_rect == the component rectangle grk_decompress_read_header reports with cp_reduce = r, for every r
    in 0..L (origins that are not multiples of 2^r included); r > L is refused by both."""
    _, cs = _stream(monkeypatch, C_, H, W, prec, numres, off)
    p = _params(cs)
    assert (p.tile_x0, p.tile_y0, p.tile_w, p.tile_h) == (off[0], off[1], W, H)
    L = p.num_levels
    for r in range(L + 1):
        want = RH.header_rects(cs, r)
        assert not isinstance(want, int), "reference refused reduce %d: %d" % (r, want)
        got = G.reduced_tile_rect(p, r)
        for k in range(C_):
            if off[0] % (1 << r) == 0 and off[1] % (1 << r) == 0:
                assert want[k] == got, (r, k)
            else:
                # (an origin off the 2^r grid: the reference's composite image is ceil(w / 2^r) wide -- up to one column / row
                #  more than the tile's resolution holds, RH.crop; the origin and the samples of the rectangle are the same)
                assert want[k][:2] == got[:2], (r, k)
                assert got[2] <= want[k][2] <= got[2] + 1 and got[3] <= want[k][3] <= got[3] + 1, (r, k)
    assert isinstance(RH.header_rects(cs, L + 1), int)
    with pytest.raises(ValueError):
        G.reduced_tile_rect(p, L + 1)


def test_reduced_tile_rect_formula():
    """ceil(x / 2^r) of the tile bounds (rectceildivpow2), independent of the reference."""
    for (x0, y0, w, h, L) in [(0, 0, 64, 64, 4), (5, 3, 129, 37, 5), (7, 9, 33, 50, 2), (1, 1, 1, 1, 3), (1023, 4097, 8191, 3, 10)]:
        p = G.TileParams.make(w, h, 1, 8, L, origin=(x0, y0))
        for r in range(L + 1):
            cx = lambda v: -(-v // (1 << r))
            assert G.reduced_tile_rect(p, r) == (cx(x0), cx(y0), cx(x0 + w) - cx(x0), cx(y0 + h) - cx(y0))
        with pytest.raises(ValueError):
            G.reduced_tile_rect(p, L + 1)


def test_set_decode_reduce_symbol_exported():
    L = G.lib()
    assert hasattr(L, "grk_amd_set_decode_reduce") and hasattr(L, "grk_amd_reduced_tile_rect")


@needs_ref
@pytest.mark.parametrize("C_,H,W,prec,numres,off", [(3, 61, 77, 8, 5, (0, 0)), (3, 50, 33, 8, 3, (7, 9)), (1, 37, 129, 12, 4, (5, 3)),
                                                      (3, 100, 70, 12, 4, (3, 6))])
@pytest.mark.parametrize("ht", [1, 0])
def test_reference_reduced_decode_is_ll_band(monkeypatch, C_, H, W, prec, numres, off, ht):
    """The shim's reduced decode of a reversible RCT + 5/3 stream == inverse RCT + DC shift (clamped) of the LL band after r forward
    levels of the reference's own 5/3 (ref_dwt53_fwd_at) at the tile's origin."""
    px, cs = _stream(monkeypatch, C_, H, W, prec, numres, off, ht=ht)
    L = R.lib()
    dc, hi = 1 << (prec - 1), (1 << prec) - 1
    for r in range(numres):
        planes = [np.ascontiguousarray(px[k].astype(np.int32) - dc) for k in range(C_)]
        if C_ >= 3:
            L.ref_rct(planes[0].ctypes.data, planes[1].ctypes.data, planes[2].ctypes.data, planes[0].size)
        x0, y0, w, h = G.reduced_tile_rect(_params(cs), r)
        ll = []
        for a in planes:
            L.ref_dwt53_fwd_at(a.ctypes.data, W, H, W, r, off[0], off[1])
            ll.append(a[:h, :w].astype(np.int64))
        if C_ >= 3:
            y, cb, cr = ll[:3]
            g = y - ((cb + cr) >> 2)
            ll[:3] = [cr + g, g, cb + g]
        want = [np.clip(v + dc, 0, hi) for v in ll]
        got = RH.decode(cs, r)
        assert not isinstance(got, int), "reference refused reduce %d: %d" % (r, got)
        got = RH.crop(got, (w, h))
        for k in range(C_):
            assert got[k].shape == (h, w)
            assert np.array_equal(got[k], want[k]), (r, k)
    assert isinstance(RH.decode(cs, numres), int)
