"""GPU: grk_amd_decode_image -- a whole codestream (any tile layout, the five progression orders, precincts, layers, SOP / EPH /
PLT / TLM; HT and Part-1) to pixels, with the library's own Tier-2 reader in front: against grk_decompress, against the encoder's
own files, against the existing table route, at size, and its two kernels alone."""
import os

import numpy as np
import pytest
import torch

import grok_amd as G
import gpuutil as U
import refharness as R
import synth
from grok_amd.capi import CODED_DTYPE, MOVE_DTYPE

pytestmark = pytest.mark.gpu
needs_ref = pytest.mark.skipif(not R.have_ref(), reason="oracle/_ref (the real reference) not built here")
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REF_VARS = ("REF_PROG_ORDER", "REF_PRECINCTS", "REF_CSTY", "REF_WRITE_PLT", "REF_WRITE_TLM", "REF_LAYERS", "REF_IMG_X0", "REF_IMG_Y0")


# ---- 1. == grk_decompress ----------------------------------------------------------------------------------------------------------
# factors: coder x transform (HT + 9/7 of the reference's encoder is broken, defect D1: left out), tiling, precincts, order,
# markers, layers, offset; every value of every factor at least twice (the corners), then a seeded sample of the product
CODERS = [("ht", 0), ("p1", 0), ("p1", 1)]
TILINGS = ["one", "2x2", "ragged"]
W, H, L = 256, 200, 3


def _cases():
    rng = np.random.default_rng(2024)
    seen, out = set(), []

    def add(coder, tiling, prc, order, marks, layers, off, prec):
        k = (coder, tiling, prc, order, marks, layers, off, prec)
        if k not in seen:
            seen.add(k)
            out.append(k)
    # corners: each factor walks its values twice against two different settings of the others
    for rep in range(2):
        base = [CODERS[rep], TILINGS[rep + 1], rep, rep * 3, rep, 1 + 2 * rep, (rep, rep), 8]
        for i, vals in enumerate([CODERS, TILINGS, [0, 1], [0, 1, 2, 3, 4], [0, 1], [1, 3], [(0, 0), (1, 1)], [8, 12, 16]]):
            for v in vals:
                c = list(base)
                c[i] = v
                add(*c)
    while len(out) < 90:
        add(CODERS[rng.integers(3)], TILINGS[rng.integers(3)], int(rng.integers(2)), int(rng.integers(5)), int(rng.integers(2)),
            int(rng.choice([1, 3])), [(0, 0), (1, 1)][rng.integers(2)], int(rng.choice([8, 12, 16])))
    return out


def _id(k):
    (coder, irrev), tiling, prc, order, marks, layers, off, prec = k
    return "%s%s-%s-%s-o%d-%s-l%d-off%d-p%d" % (coder, "97" if irrev else "53", tiling, "prc" if prc else "dflt", order, "sopeph" if marks else "plain",
                                                 layers, off[0], prec)


@needs_ref
@pytest.mark.parametrize("case", _cases(), ids=_id)
def test_decode_image_equals_grk_decompress(monkeypatch, case):
    (coder, irrev), tiling, prc, order, marks, layers, off, prec = case
    ht = coder == "ht"
    Cn = 3
    px = synth.g2_mid(Cn, H, W, prec) if prec == 16 else synth.g2(Cn, H, W, prec)
    TW, TH = {"one": (W + off[0], H + off[1]), "2x2": ((W + off[0] + 1) // 2, (H + off[1] + 1) // 2), "ragged": (100, 77)}[tiling]
    for k in REF_VARS:
        monkeypatch.delenv(k, raising=False)
    env = {"REF_PROG_ORDER": order, "REF_IMG_X0": off[0], "REF_IMG_Y0": off[1], "REF_CSTY": 6 if marks else 0, "REF_WRITE_TLM": order & 1,
           "REF_WRITE_PLT": 1 - (order & 1)}
    if prc:
        env["REF_PRECINCTS"] = "64,64,32,32"
    if layers > 1:
        env["REF_LAYERS"] = "20,10,1"
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    cs, _ = R.encode(px, prec, TW=TW, TH=TH, irrev=irrev, numres=L + 1, ht=int(ht), mode=1)
    info = G.read_header(cs)
    assert info.num_layers == layers and info.num_tiles == {"one": 1, "2x2": 4, "ragged": 9}[tiling]
    want = R.decode(cs, Cn, H, W)
    got = U.ctx().decode_image(cs)
    assert np.array_equal(got.astype(np.int32), want)
    if not irrev:
        assert np.array_equal(got, px)


# ---- 2. round trip of the library's own files -------------------------------------------------------------------------------
@pytest.mark.parametrize("Cn,Hh,Ww,TW,TH,off,prec", [(3, 1024, 1024, 256, 256, (0, 0), 8), (3, 2000, 2000, 1000, 1000, (1, 1), 8),
                                                     (1, 600, 500, 200, 256, (0, 0), 16), (3, 300, 260, 128, 100, (3, 5), 12)])
def test_decode_image_of_encode_image_is_the_image(Cn, Hh, Ww, TW, TH, off, prec):
    c = U.ctx()
    px = synth.g2_mid(Cn, Hh, Ww, prec) if prec == 16 else synth.g2(Cn, Hh, Ww, prec)
    layout = G.ImageLayout.make(Ww, Hh, TW, TH, offset=off)
    base = G.TileParams.make(TW, TH, Cn, prec, 5 if Ww >= 1000 else 3)
    for flags in (0, G.CS_PLT | G.CS_TLM | G.CS_SOP | G.CS_EPH | G.CS_PROG(2)):
        cs = c.encode_image(layout, base, px, flags)
        gathers, places = c.decode_image_launches()
        assert np.array_equal(c.decode_image(cs), px)
        assert c.decode_image_launches() == (gathers, places + len(_groups(layout, base)))
        # device pixels: asynchronous, decode_status joins
        out = U._settled(torch.zeros(px.nbytes, dtype=torch.uint8, device="cuda"))
        c.decode_image_device(cs, out.data_ptr(), px.nbytes)
        c.decode_status()
        assert np.array_equal(out.cpu().numpy().view(px.dtype).reshape(px.shape), px)


def _groups(layout, base):
    groups = []
    for p in G.layout_tiles(layout, base):
        for g in groups:
            if G.same_tile_geometry(g, p):
                break
        else:
            groups.append(p)
    return groups


def test_decode_image_ht_irreversible_equals_decode_tiles_per_tile():
    """9/7 HT: no reference bytes exist (defect D1); decode_image of a file of this encoder's tiles == decode_tiles of every tile
    with the table the encoder returned"""
    c = U.ctx()
    Ww, Hh, TW, TH = 300, 260, 128, 100
    px = synth.g2(3, Hh, Ww, 8)
    layout = G.ImageLayout.make(Ww, Hh, TW, TH, offset=(1, 1))
    base = G.TileParams.make(TW, TH, 3, 8, 3, irreversible=True)
    tabs, chunks, want, at = [], [], np.zeros_like(px), 0
    for p in G.layout_tiles(layout, base):
        ox, oy = p.tile_x0 - 1, p.tile_y0 - 1
        tile = np.ascontiguousarray(px[:, oy:oy + p.tile_h, ox:ox + p.tile_w])
        table, coded = c.encode_host(p, tile)
        want[:, oy:oy + p.tile_h, ox:ox + p.tile_w] = c.decode_host(p, table, coded)[0]
        t = table.copy()
        # (the arena's offsets are not dense: the blocks packed end to end, as a writer's input may be)
        dense = np.concatenate([coded[int(o):int(o) + int(n)] for o, n in zip(table["offset"], table["length"])]) if len(table) else coded[:0]
        t["offset"] = at + np.concatenate([[0], np.cumsum(table["length"].astype(np.int64))[:-1]])
        at += dense.size
        tabs.append(t)
        chunks.append(dense)
    cs = G.write_codestream_layout(layout, base, np.concatenate(tabs), np.concatenate(chunks), G.CS_PLT)
    assert synth.psnr_db(want, px, 8) > 40
    assert np.array_equal(c.decode_image(cs), want)


# ---- 3. the same pixels as the existing route ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dec_p1_irrev_3x96x160_r5", "dec_p1_irrev_3x128x128_p12_r6", "dec_p1_rev_3x100x77_r3", "dec_ht_rev_1x128x128_r4",
                                  "dec_p1_sty3f_irrev_3x96x128_p10_r4", "dec_p1_sty05_rev_1x128x96_p12_r3", "g2_3x192x160_r4", "g2u16_1x128x128_r5"])
def test_single_tile_streams_decode_as_through_j2kparse(name):
    from test_gpu_decode import _gpu_decode_reference_stream
    cs = open(os.path.join(GOLD, name + ".j2k"), "rb").read()
    want = _gpu_decode_reference_stream(cs, part1="_p1_" in name)
    c = U.ctx()
    gathers, places = c.decode_image_launches()
    assert np.array_equal(c.decode_image(cs), want)
    assert c.decode_image_launches() == (gathers, places)              # one tile, one layer: neither kernel


# ---- 4. at size --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,T", [(8192, 8192), (4096, 1024)])
def test_decode_image_at_size(S, T):
    c = U.ctx()
    px = synth.g2(3, S, S, 8)
    layout = G.ImageLayout.make(S, S, T, T)
    cs = c.encode_image(layout, G.TileParams.make(T, T, 3, 8, 5), px, G.CS_PLT)
    gathers, places = c.decode_image_launches()
    got = c.decode_image(cs)
    assert np.array_equal(got, px)
    assert c.decode_image_launches() == (gathers, places + (0 if S == T else 1))


# ---- 5. the kernels alone ------------------------------------------------------------------------------------------------------------
def test_gather_kernel_equals_the_moves_applied_with_numpy():
    c = U.ctx()
    rng = np.random.default_rng(11)
    src = rng.integers(0, 256, size=300000, dtype=np.uint8)
    lens = np.concatenate([rng.integers(0, 40, 300), rng.integers(40, 3000, 200), [0, 1, 15, 16, 17, 4096]]).astype(np.uint32)
    rng.shuffle(lens)
    moves = np.zeros(lens.size, MOVE_DTYPE)
    moves["len"] = lens
    moves["kind"] = 1
    moves["src"] = [rng.integers(0, src.size - int(n) + 1) for n in lens]
    moves["dst"] = np.concatenate([[0], np.cumsum(lens.astype(np.int64))[:-1]]) + 3          # (an odd start: every alignment occurs)
    total = int(lens.sum()) + 3
    want = np.full(total + 5, 0xA5, np.uint8)
    for m in moves:
        want[int(m["dst"]):int(m["dst"]) + int(m["len"])] = src[int(m["src"]):int(m["src"]) + int(m["len"])]
    d_src = U.to_dev(src)
    d_dst = U.to_dev(np.full(total + 5, 0xA5, np.uint8))
    c.gather_device(moves, d_src.data_ptr(), src.size, d_dst.data_ptr(), total)
    c.synchronize()
    assert np.array_equal(d_dst.cpu().numpy(), want)
    # a move outside its buffers is refused before anything is launched
    bad = moves[:1].copy()
    bad["src"] = src.size - 1
    bad["len"] = 2
    with pytest.raises(RuntimeError, match="outside"):
        c.gather_device(bad, d_src.data_ptr(), src.size, d_dst.data_ptr(), total)


@needs_ref
def test_gathered_appendix_of_a_layered_stream(monkeypatch):
    """the appendix decode_image builds on the device for a layered Part-1 stream == the reader's moves applied with numpy (the
    pixels of such streams: test 1)"""
    for k in REF_VARS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("REF_LAYERS", "20,10,1")
    px = synth.g2(3, 200, 256, 8)
    cs, _ = R.encode(px, 8, TW=100, TH=77, numres=4, ht=0, mode=1)
    out = G.read_packets(cs, None, 3)
    assert len(out["moves"]) > 0
    b = np.frombuffer(cs, np.uint8)
    want = np.zeros(out["appendix_bytes"], np.uint8)
    for m in out["moves"]:
        want[int(m["dst"]):int(m["dst"]) + int(m["len"])] = b[int(m["src"]):int(m["src"]) + int(m["len"])]
    c = U.ctx()
    d_src = U.to_dev(b)
    d_dst = U.to_dev(np.zeros(want.size, np.uint8))
    gathers, _ = c.decode_image_launches()
    c.gather_device(out["moves"], d_src.data_ptr(), b.size, d_dst.data_ptr(), want.size)
    c.synchronize()
    assert np.array_equal(d_dst.cpu().numpy(), want)
    assert np.array_equal(c.decode_image(cs), px)
    assert c.decode_image_launches()[0] == gathers + 2


@pytest.mark.parametrize("bps", [1, 2])
def test_placement_kernel_equals_numpy_slicing(bps):
    c = U.ctx()
    rng = np.random.default_rng(5 + bps)
    dt = np.uint8 if bps == 1 else np.uint16
    for (w, h, ncomp, img_w, img_h, n) in [(37, 21, 3, 301, 97, 7), (64, 64, 1, 256, 128, 8), (1, 1, 2, 9, 7, 5), (129, 3, 4, 517, 40, 6), (100, 77, 3, 257, 201, 4)]:
        tiles = rng.integers(0, 1 << (8 * bps), size=(n, ncomp, h, w)).astype(dt)
        # tiles that do not overlap: places on a grid of cells, each tile somewhere inside its cell
        cols, rows = img_w // w, img_h // h
        cells = rng.permutation(cols * rows)[:n]
        rects = [((k % cols) * w + (k % cols == cols - 1) * (img_w - cols * w), (k // cols) * h + (k // cols == rows - 1) * (img_h - rows * h))
                 for k in cells]                          # (the last column / row of cells ends with the image)
        # the image starts one byte into its buffer for 1-byte samples (a destination on an odd address), one sample for 2-byte ones
        img = rng.integers(0, 1 << (8 * bps), size=1 + ncomp * img_h * img_w).astype(dt)
        want = img.copy()
        planes = want[1:].reshape(ncomp, img_h, img_w)
        for t, (x, y) in enumerate(rects):
            planes[:, y:y + h, x:x + w] = tiles[t]
        d_tiles, d_img = U.to_dev(tiles), U.to_dev(img)
        c.place_tiles_device(d_tiles.data_ptr(), n, w, h, ncomp, bps, rects, d_img.data_ptr() + bps, img_w, img_h)
        c.synchronize()
        assert np.array_equal(d_img.cpu().numpy(), want), (w, h, ncomp, bps)
    with pytest.raises(RuntimeError, match="outside"):
        c.place_tiles_device(d_tiles.data_ptr(), 1, 100, 77, 3, bps, [(200, 0)], d_img.data_ptr(), 257, 201)


# ---- the int16-plane range rule, and 6. settings put back ----------------------------------------------------------------------------
def _forged_8bit_stream(tiles):
    """The stream test_decode_int16_planes_and_their_range_check builds, as a file: the blocks of a 16-bit checkerboard under
    8-bit parameters -- coefficients far outside +-2047.  Written as the 16-bit image it is, then SIZ says 8 bits and QCD carries
    the 8-bit exponents (the zero bit-planes in the packet headers stay the 16-bit tile's, as in that test's table)."""
    Hh, Ww, Lv = 256, 320, 5
    yy, xx = np.mgrid[0:Hh, 0:Ww]
    px16 = (((yy + xx) & 1) * 30000 + 10000).astype(np.uint16)[None]
    TW, TH = Ww // tiles, Hh // tiles
    layout = G.ImageLayout.make(Ww, Hh, TW, TH)
    p16, p8 = G.TileParams.make(TW, TH, 1, 16, Lv), G.TileParams.make(TW, TH, 1, 8, Lv)
    c = U.ctx()
    tabs, chunks, want, at = [], [], np.zeros((1, Hh, Ww), np.uint8), 0
    for t16 in G.layout_tiles(layout, p16):                          # (tiles off the 2^levels x 64 grid: several geometries)
        x, y = t16.tile_x0, t16.tile_y0
        t8 = G.TileParams.make(t16.tile_w, t16.tile_h, 1, 8, Lv, origin=(x, y))
        tile = np.ascontiguousarray(px16[:, y:y + TH, x:x + TW])
        table, coded = c.encode_host(t16, tile)
        c.set_decode_planes16(False)
        try:
            want[:, y:y + TH, x:x + TW] = c.decode_host(t8, table, coded)[0]
        finally:
            c.set_decode_planes16(True)
        t = table.copy()
        t["offset"] += at
        at += coded.size
        tabs.append(t)
        chunks.append(coded)
    cs = bytearray(G.write_codestream_layout(layout, p16, np.concatenate(tabs), np.concatenate(chunks), G.CS_PLT))
    s, q = cs.index(b"\xff\x51"), cs.index(b"\xff\x5c")
    assert cs[s + 4 + 36] == 15
    cs[s + 4 + 36] = 7
    _, q8 = G.tile_layout(p8)
    _, q16 = G.tile_layout(p16)
    assert bytes(cs[q + 5:q + 5 + len(q16)]) == bytes(w & 0xFF for w in q16)
    cs[q + 5:q + 5 + len(q8)] = bytes(w & 0xFF for w in q8)
    return bytes(cs), want


@pytest.mark.parametrize("tiles", [1, 2])
def test_decode_image_repeats_a_group_that_leaves_the_int16_planes(tiles):
    cs, want = _forged_8bit_stream(tiles)
    c = U.ctx()
    assert np.array_equal(c.decode_image(cs), want)                 # host pixels: int16 planes -> range flag -> that group again with int32 planes
    out = U._settled(torch.zeros(want.size, dtype=torch.uint8, device="cuda"))
    c.decode_image_device(cs, out.data_ptr(), want.size)            # device pixels: reported
    with pytest.raises(RuntimeError, match="16-bit planes"):
        c.decode_status()
    c.set_decode_planes16(False)
    try:
        c.decode_image_device(cs, out.data_ptr(), want.size)
        c.decode_status()
    finally:
        c.set_decode_planes16(True)
    assert np.array_equal(out.cpu().numpy().reshape(want.shape), want)


@needs_ref
def test_context_settings_are_put_back_after_decode_image(monkeypatch):
    """a context that decoded a Part-1 9/7 stream of several segments per block (QCD words, segment lists set by the call) decodes
    a plain decode_tiles call as before -- and keeps settings the caller made"""
    for k in REF_VARS:
        monkeypatch.delenv(k, raising=False)
    c = U.ctx()
    px = synth.g2(3, 256, 256, 8)
    p = G.TileParams.make(256, 256, 3, 8, 4, irreversible=True)
    table, coded = c.encode_host(p, px)
    before = c.decode_host(p, table, coded)[0]
    cs, _ = R.encode(synth.g2(3, 200, 256, 10), 10, TW=100, TH=77, irrev=1, numres=4, ht=0, mode=1, cblksty=0x05)
    assert np.array_equal(c.decode_image(cs).astype(np.int32), R.decode(cs, 3, 200, 256))
    assert np.array_equal(c.decode_host(p, table, coded)[0], before)
    # the caller's own QCD words survive the call
    _, words = G.tile_layout(p)
    coarse = [w - (1 << 11) for w in words]                         # every exponent one less: steps twice as large
    c.set_decode_qcd(coarse)
    try:
        other = c.decode_host(p, table, coded)[0]
        assert not np.array_equal(other, before)
        c.decode_image(cs)
        assert np.array_equal(c.decode_host(p, table, coded)[0], other)
    finally:
        c.set_decode_qcd([])
    assert np.array_equal(c.decode_host(p, table, coded)[0], before)
    # refusals of the call itself
    c.set_decode_reduce(1)
    try:
        with pytest.raises(RuntimeError, match="reduced"):
            c.decode_image(cs)
    finally:
        c.set_decode_reduce(0)
