"""GPU: grk_amd_decode_image_view -- a whole codestream at reduced resolution and / or by window: against the reference's reduced
decode (grk_decompress -r) and window (grk_decompress_set_window), against crops of its own whole views, the clipping placement
kernel alone, what the call reads and uploads, and what it leaves on the context."""
import os

import numpy as np
import pytest
import torch

import grok_amd as G
import gpuutil as U
import pixlayout as PL
import refharness as R
import reducehost
import synth

pytestmark = pytest.mark.gpu
needs_ref = pytest.mark.skipif(not R.have_ref(), reason="oracle/_ref (the real reference) not built here")
REF_VARS = ("REF_PROG_ORDER", "REF_PRECINCTS", "REF_CSTY", "REF_WRITE_PLT", "REF_WRITE_TLM", "REF_LAYERS", "REF_IMG_X0", "REF_IMG_Y0")
W, H, L = 200, 136, 3
CODERS = {"ht53": (1, 0), "p153": (0, 0), "p197": (0, 1)}
_cache = {}


def stream(coder, tile, off=(0, 0), prec=8, levels=L, env=(), w=W, h=H):
    """the reference encoder's file (mode 1) of synth.g2 content, cached; tile None: one tile"""
    key = ("cs", coder, tile, off, prec, levels, env, w, h)
    if key not in _cache:
        keep = {k: os.environ.pop(k, None) for k in REF_VARS}
        try:
            os.environ["REF_IMG_X0"], os.environ["REF_IMG_Y0"] = str(off[0]), str(off[1])
            for k, v in env:
                os.environ[k] = str(v)
            ht, irrev = CODERS[coder]
            px = synth.g2_mid(3, h, w, prec) if prec == 16 else synth.g2(3, h, w, prec)
            TW, TH = tile if tile else (w + off[0], h + off[1])
            _cache[key] = (R.encode(px, prec, TW=TW, TH=TH, irrev=irrev, numres=levels + 1, ht=ht, mode=1)[0], px)
        finally:
            for k in REF_VARS:
                os.environ.pop(k, None)
                if keep[k] is not None:
                    os.environ[k] = keep[k]
    return _cache[key]


def ref_full(cs, w=W, h=H):
    key = ("full", cs)
    if key not in _cache:
        _cache[key] = R.decode(cs, 3, h, w)
    return _cache[key]


def whole_view(cs, r):
    """this library's whole view at reduce r (test 1 pins it to the reference), cached"""
    key = ("view", cs, r)
    if key not in _cache:
        _cache[key] = U.ctx().decode_image_view(cs, r)
    return _cache[key]


# ---- 1. reduce == the reference's reduced decode ----------------------------------------------------------------------------------
REDUCE_STREAMS = [(coder, tile, off) for coder in CODERS for tile in (None, (64, 48)) for off in ((0, 0), (5, 3))]


def _check_reduce(cs, levels=L):
    info = G.read_header(cs)
    for r in range(1, levels + 1):
        w, h = G.image_view_size(info, r)[0]
        want = np.stack(reducehost.crop(reducehost.decode(cs, r), (w, h)))
        got = U.ctx().decode_image_view(cs, r)
        assert got.shape == (3, h, w)
        assert np.array_equal(got.astype(np.int32), want), r


@needs_ref
@pytest.mark.parametrize("coder,tile,off", REDUCE_STREAMS, ids=lambda v: str(v).replace(" ", ""))
def test_reduced_view_equals_the_reference(coder, tile, off):
    _check_reduce(stream(coder, tile, off)[0])


@needs_ref
@pytest.mark.parametrize("tile", [None, (64, 48)])
def test_reduced_view_of_12_bit_irreversible_part1(tile):
    _check_reduce(stream("p197", tile, (5, 3), prec=12)[0])


@needs_ref
@pytest.mark.parametrize("coder", ["ht53", "p153"])
def test_reduced_view_with_precincts_and_layers(coder):
    """several pieces per block: the appendix is gathered for the kept resolutions of the touched tiles only"""
    cs = stream(coder, (64, 48), (5, 3), env=(("REF_PRECINCTS", "64,64,32,32"), ("REF_LAYERS", "20,10,1")))[0]
    assert G.read_header(cs).num_layers == 3
    _check_reduce(cs)
    full = ref_full(cs)
    for win in [(60, 40, 140, 100), (0, 0, 1, 1)]:
        got = U.ctx().decode_image_view(cs, 0, win)
        assert np.array_equal(got.astype(np.int32), full[:, win[1]:win[3], win[0]:win[2]])


# ---- 2. sub-sampled components --------------------------------------------------------------------------------------------------
S420 = [(1, 1), (2, 2), (2, 2)]


@needs_ref
@pytest.mark.parametrize("tile", [None, (64, 48)])
def test_reduced_view_of_sub_sampled_components(tile):
    Ws, Hs = 202, 138
    planes = [synth.g2(1, (Hs + dy - 1) // dy, (Ws + dx - 1) // dx, 8, seed=70 + k)[0] for k, (dx, dy) in enumerate(S420)]
    cs = R.encode_planes(planes, S420, 8, Ws, Hs, TW=tile[0] if tile else None, TH=tile[1] if tile else None, numres=4)
    c = U.ctx()
    for r, sizes in [(1, [(101, 69), (51, 35), (51, 35)]), (2, [(51, 35), (26, 18), (26, 18)])]:
        assert G.image_view_size(G.read_header(cs), r) == sizes
        want = reducehost.decode(cs, r)
        got = c.decode_image_view_planes(cs, r)
        for k in range(3):
            assert got[k].shape == want[k].shape == sizes[k][::-1]
            assert np.array_equal(got[k].astype(np.int32), want[k]), (r, k)
    assert all(np.array_equal(a, b) for a, b in zip(c.decode_image_view_planes(cs, 0), c.decode_image_planes(cs)))
    c.set_decode_upsample(True)
    try:
        with pytest.raises(RuntimeError, match="upsampl"):
            c.decode_image_view_planes(cs, 1)
        with pytest.raises(RuntimeError):
            c.decode_image_view(cs, 0, (0, 0, 10, 10))
    finally:
        c.set_decode_upsample(False)
    with pytest.raises(RuntimeError):
        c.decode_image_view(cs, 0, (0, 0, 10, 10))


# ---- 3. windows -------------------------------------------------------------------------------------------------------------------
WINDOWS = [(0, 0, 70, 50), (60, 40, 140, 100), (63, 47, 66, 50), (131, 77, 200, 136), (10, 10, 190, 120), (100, 0, 101, 136)]
WINDOW_STREAMS = {"ht53-64x48": ("ht53", (64, 48), L), "p197-100x77": ("p197", (100, 77), L), "ht53-100x68-l4": ("ht53", (100, 68), 4),
                  "ht53-one": ("ht53", None, L)}


@needs_ref
@pytest.mark.parametrize("name", list(WINDOW_STREAMS))
def test_window_equals_the_crop_and_the_reference_window(name):
    coder, tile, levels = WINDOW_STREAMS[name]
    cs = stream(coder, tile, levels=levels)[0]
    full = ref_full(cs)
    for win in WINDOWS:
        x0, y0, x1, y1 = win
        got = U.ctx().decode_image_view(cs, 0, win).astype(np.int32)
        assert np.array_equal(got, full[:, y0:y1, x0:x1]), win
        assert np.array_equal(got, R.decode_window(cs, 3, x0, y0, x1, y1)), win


@needs_ref
def test_window_counts_from_the_image_origin():
    """image at (5, 3): the window is relative to the image's top-left sample (the reference's own window is wrong for one of
    these there, its defect D12: the crop of its full decode is the oracle)"""
    cs = stream("p153", (64, 48), (5, 3))[0]
    full = ref_full(cs)
    for x0, y0, x1, y1 in WINDOWS:
        got = U.ctx().decode_image_view(cs, 0, (x0, y0, x1, y1)).astype(np.int32)
        assert np.array_equal(got, full[:, y0:y1, x0:x1]), (x0, y0, x1, y1)


def test_window_refusals():
    cs = stream("ht53", (64, 48))[0] if R.have_ref() else _own_stream()[0]
    c = U.ctx()
    for win in [(10, 10, 10, 20), (10, 20, 30, 20), (0, 0, W + 1, H), (0, 0, W, H + 1)]:
        with pytest.raises(RuntimeError):
            c.decode_image_view(cs, 0, win)
    with pytest.raises(RuntimeError):
        c.decode_image_view(cs, L + 1)
    with pytest.raises(RuntimeError):
        c.decode_image_view(cs, 1, (0, 0, W // 2 + 1, H // 2))          # the window counts in the reduced image


def _own_stream(w=W, h=H, tile=(64, 48), flags=G.CS_PLT):
    """a reversible HT file of this library's encoder: decodes to its pixels"""
    key = ("own", w, h, tile, flags)
    if key not in _cache:
        px = synth.g2(3, h, w, 8)
        _cache[key] = (U.ctx().encode_image(G.ImageLayout.make(w, h, *tile), G.TileParams.make(tile[0], tile[1], 3, 8, L), px, flags), px)
    return _cache[key]


# ---- 4. window and reduce together ------------------------------------------------------------------------------------------------
@needs_ref
@pytest.mark.parametrize("tile", [(64, 48), None], ids=["64x48", "one"])
@pytest.mark.parametrize("r", [1, 2, 3])
def test_window_of_a_reduced_view_equals_its_crop(tile, r):
    """(r = 3 = the levels: no DWT level is left for the region decoder -- a one-tile stream is then decoded whole and clipped)"""
    cs = stream("ht53", tile)[0]
    whole = whole_view(cs, r)
    w, h = whole.shape[2], whole.shape[1]
    seam = 64 >> r
    for x0, y0, x1, y1 in [(seam, 1, seam + 1, h - 1), (0, 0, w // 2 + 3, h // 2 + 1), (w // 3, h // 3, w, h), (seam - 1, (48 >> r) - 1, seam + 1, (48 >> r) + 1)]:
        got = U.ctx().decode_image_view(cs, r, (x0, y0, x1, y1))
        assert np.array_equal(got, whole[:, y0:y1, x0:x1]), (x0, y0, x1, y1)


# ---- 5. the placement kernel alone, clipping ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bps", [1, 2])
@pytest.mark.parametrize("channels", [0, 4], ids=["planar", "rgbx"])
def test_clipping_placement_kernel_equals_numpy_slicing(bps, channels):
    c = U.ctx()
    rng = np.random.default_rng(17 + bps + channels)
    dt = np.uint8 if bps == 1 else np.uint16
    w, h, ncomp, img_w, img_h = 37, 21, 3, 120, 70
    # inside; cut left, right, top, bottom; two sides at once (corners); wholly outside (left, below, right) -- no two overlap
    pos = [(40, 24), (-10, 24), (100, 24), (40, -8), (40, 60), (-30, -15), (110, 60), (-37, 10), (20, 70), (120, 0)]
    n = len(pos)
    sentinel = 0xA5 if bps == 1 else 0xA5A5
    if channels:
        tiles = rng.integers(0, 1 << (8 * bps), size=(n, h, w, channels)).astype(dt)
        want = np.full((img_h, img_w, channels), sentinel, dt)
    else:
        tiles = rng.integers(0, 1 << (8 * bps), size=(n, ncomp, h, w)).astype(dt)
        want = np.full((ncomp, img_h, img_w), sentinel, dt)
    for t, (x, y) in enumerate(pos):
        ax0, ay0, ax1, ay1 = max(x, 0), max(y, 0), min(x + w, img_w), min(y + h, img_h)
        if ax0 >= ax1 or ay0 >= ay1:
            continue
        if channels:
            want[ay0:ay1, ax0:ax1] = tiles[t, ay0 - y:ay1 - y, ax0 - x:ax1 - x]
        else:
            want[:, ay0:ay1, ax0:ax1] = tiles[t, :, ay0 - y:ay1 - y, ax0 - x:ax1 - x]
    # (guard samples before and behind the destination: nothing outside it is written)
    guard = 64
    img = np.full(guard + want.size + guard, sentinel, dt)
    d_tiles, d_img = U.to_dev(tiles), U.to_dev(img)
    c.place_tiles_clipped_device(d_tiles.data_ptr(), n, w, h, ncomp, bps, pos, d_img.data_ptr() + guard * bps, img_w, img_h, channels=channels)
    c.synchronize()
    got = d_img.cpu().numpy()
    assert np.all(got[:guard] == sentinel) and np.all(got[-guard:] == sentinel)
    assert np.array_equal(got[guard:-guard].reshape(want.shape), want)
    # a unit wholly inside moves what the plain placement moves
    d_a, d_b = U.to_dev(np.zeros(want.size, dt)), U.to_dev(np.zeros(want.size, dt))
    if not channels:
        c.place_tiles_device(d_tiles.data_ptr(), 1, w, h, ncomp, bps, [pos[0]], d_a.data_ptr(), img_w, img_h)
        c.place_tiles_clipped_device(d_tiles.data_ptr(), 1, w, h, ncomp, bps, [pos[0]], d_b.data_ptr(), img_w, img_h)
        c.synchronize()
        assert np.array_equal(d_a.cpu().numpy(), d_b.cpu().numpy())


# ---- 6. the reader and the upload follow the view --------------------------------------------------------------------------------------
@needs_ref
@pytest.mark.parametrize("marks", [0, 1], ids=["plain", "tlm-plt"])
def test_only_the_touched_tiles_are_read_and_uploaded(marks):
    cs, px = stream("ht53", (64, 48), env=(("REF_WRITE_TLM", marks), ("REF_WRITE_PLT", marks)), w=256, h=192)
    parts, used_tlm = G.locate_tile_parts(cs)
    assert len(parts) == 16 and used_tlm == bool(marks)
    part_len = {t: n for _, n, t in parts}
    c = U.ctx()
    for win, tiles in [((70, 50, 100, 80), [5]), ((63, 47, 66, 50), [0, 1, 4, 5]), ((200, 140, 256, 192), [11, 15])]:
        assert list(G.plan_image_view(G.read_header(cs), 0, win)["tiles"]) == tiles
        t0, b0 = c.decode_image_counters()
        got = c.decode_image_view(cs, 0, win)
        t1, b1 = c.decode_image_counters()
        assert np.array_equal(got, px[:, win[1]:win[3], win[0]:win[2]])
        assert t1 - t0 == len(tiles)
        assert 0 < b1 - b0 <= sum(part_len[t] for t in tiles) + 64 * len(tiles), (win, b1 - b0)
    t0, b0 = c.decode_image_counters()
    assert np.array_equal(c.decode_image_view(cs), px)
    t1, b1 = c.decode_image_counters()
    assert t1 - t0 == 16 and b1 - b0 <= len(cs)
    t0, _ = c.decode_image_counters()
    assert np.array_equal(c.decode_image(cs), px)
    assert c.decode_image_counters()[0] - t0 == 16


# ---- 7. equivalences and state --------------------------------------------------------------------------------------------------------
@needs_ref
@pytest.mark.parametrize("coder,tile,off", REDUCE_STREAMS, ids=lambda v: str(v).replace(" ", ""))
def test_the_all_zero_view_is_decode_image(coder, tile, off):
    cs = stream(coder, tile, off)[0]
    c = U.ctx()
    want = c.decode_image(cs)
    assert np.array_equal(c.decode_image_view(cs), want)
    assert np.array_equal(c.decode_image_view(cs, 0, (0, 0, W, H)), want)               # the window that is the image
    out = U._settled(torch.zeros(want.nbytes, dtype=torch.uint8, device="cuda"))
    c.decode_image_view_device(cs, out.data_ptr(), want.nbytes)
    c.decode_status()
    assert np.array_equal(out.cpu().numpy().view(want.dtype).reshape(want.shape), want)
    # ... and a reduced window into device pixels
    view = whole_view(cs, 1)[:, 5:40, 20:70]
    out = U._settled(torch.zeros(view.nbytes, dtype=torch.uint8, device="cuda"))
    c.decode_image_view_device(cs, out.data_ptr(), view.nbytes, 1, (20, 5, 70, 40))
    c.decode_status()
    assert np.array_equal(out.cpu().numpy().view(view.dtype).reshape(view.shape), view)


@needs_ref
@pytest.mark.parametrize("tile", [(64, 48), None], ids=["64x48", "one"])
def test_interleaved_pitched_view_equals_the_planar_one(tile):
    cs = stream("ht53", tile)[0]
    r, win = 1, (20, 5, 70, 40)
    planar = U.ctx().decode_image_view(cs, r, win)
    layout = G.PixelLayout.make(interleaved=True, channels=4, row_pitch=(win[2] - win[0]) * 4 + 12, fill=0x5A)
    want = PL.expected(planar[None], layout, 0xC3, fill=0x5A)
    out = np.full(want.size, 0xC3, np.uint8)
    got = U.ctx().decode_image_view(cs, r, win, layout=layout, out=out)
    assert np.array_equal(got[:want.size], want)


@needs_ref
def test_refusals_on_the_context_and_settings_put_back():
    c = U.ctx()
    cs = stream("p197", (64, 48), (5, 3), prec=12)[0]
    px = synth.g2(3, 128, 128, 8)
    p = G.TileParams.make(128, 128, 3, 8, 3, irreversible=True)
    table, coded = c.encode_host(p, px)
    before = c.decode_host(p, table, coded)[0]
    c.set_decode_reduce(1)
    try:
        with pytest.raises(RuntimeError, match="reduced"):
            c.decode_image_view(cs, 1)
    finally:
        c.set_decode_reduce(0)
    c.set_decode_pipelining(2)
    try:
        with pytest.raises(RuntimeError, match="sequence"):
            c.decode_image_view(cs, 1)
    finally:
        c.set_decode_pipelining(0)
    c.decode_image_view(cs, 2, (3, 3, 30, 20))
    assert np.array_equal(c.decode_host(p, table, coded)[0], before)          # at full size, with its own QCD words, as before


def test_reduced_view_of_an_irreversible_ht_stream_is_its_tiles_placed_by_the_plan():
    """9/7 HT: no reference bytes exist (its defect D1) -- the reduced view of a file of this encoder == decode_tiles of every tile
    under set_decode_reduce(1), at the positions the plan gives"""
    c = U.ctx()
    Ww, Hh, TW, TH = 300, 260, 128, 100
    px = synth.g2(3, Hh, Ww, 12)
    layout = G.ImageLayout.make(Ww, Hh, TW, TH)
    base = G.TileParams.make(TW, TH, 3, 12, 3, irreversible=True)
    cs = c.encode_image(layout, base, px, G.CS_PLT)
    info = G.read_header(cs)
    rows = G.read_packets(cs, info)["rows"]
    plan = G.plan_image_view(info, 1)
    (w, h), = set(G.image_view_size(info, 1))
    want = np.zeros((3, h, w), np.uint16)
    at = 0
    c.set_decode_reduce(1)
    try:
        for p, u in zip(G.layout_tiles(info.layout, info.base), plan["units"]):
            n = len(G.tile_layout(p)[0])
            tile = c.decode_host(p, rows[at:at + n], np.frombuffer(cs, np.uint8))[0]
            at += n
            assert tile.shape == (3, u["h"], u["w"])
            want[:, u["y"]:u["y"] + u["h"], u["x"]:u["x"] + u["w"]] = tile
    finally:
        c.set_decode_reduce(0)
    assert at == len(rows)
    assert np.array_equal(c.decode_image_view(cs, 1), want)
    assert np.array_equal(c.decode_image_view(cs, 1, (60, 40, 70, 60)), want[:, 40:60, 60:70])
