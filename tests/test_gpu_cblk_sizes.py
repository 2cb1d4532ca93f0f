"""-m gpu: nominal code-block sizes below 64 x 64 (COD SPcod exponents 2..6 in both directions) through the decoders and the
block coders.  A 64 x 4 block is one Part-1 stripe and two HT quad rows, a 4 x 64 one leaves 60 lanes of a row idle, a tile cut
into 16 x 16 blocks has sixteen times the blocks: whole codestreams of the reference's encoders (HT 5/3, Part-1 5/3, Part-1
9/7) through grk_amd_decode_image, the table route with its reduced and windowed decodes and the plugin; this library's own
HT 9/7 tiles against the oracle chain; the encoder's int32 planes, LDS fallback and device Tier-2 against the reference's files;
and synthetic blocks (HT refinement, ragged HT encode / decode, the Part-1 lane decoder).  Everything is bit-exact."""
import functools
import os

import numpy as np
import pytest

import grok_amd as G
import chain
import gpuutil as U
import j2kparse as J
import refharness as R
import synth

pytestmark = pytest.mark.gpu
needs_ref = pytest.mark.skipif(not R.have_ref(), reason="oracle/_ref (the real reference) not built here")

FLAT, TALL = (6, 2), (2, 6)
SIZES = [FLAT, TALL, (6, 3), (3, 5), (5, 5), (4, 4), (6, 4), (4, 6), (2, 2)]
CORE = [FLAT, TALL, (4, 4), (3, 5)]
ENC_SIZES = [FLAT, TALL, (6, 3), (3, 5), (3, 3)]
SYNTH_SIZES = [FLAT, TALL, (4, 4)]
# (the reference's HT + 9/7 encoder is broken, defect D1: 2c below covers that pair with this library's own tiles)
CODERS = [("ht", 0), ("p1", 0), ("p1", 1)]
IMAGES = [(3, 100, 77, 8), (3, 130, 200, 12)]            # C, H, W, prec; both coded with numres 4
REF_VARS = ("REF_PROG_ORDER", "REF_PRECINCTS", "REF_CSTY", "REF_WRITE_PLT", "REF_WRITE_TLM", "REF_LAYERS", "REF_IMG_X0", "REF_IMG_Y0")


def _sz(cblk):
    return "%dx%d" % (1 << cblk[0], 1 << cblk[1])


def _coder_id(c):
    return c[0] + ("97" if c[1] else "53")


def _img_id(i):
    return "%dx%dx%dp%d" % i


@functools.lru_cache(maxsize=None)
def _ref_stream(image, coder, cblk, sty=0, env=(), TW=None, TH=None):
    """(codestream of the reference's encoder, the reference's decode of it): made once, shared by the tests, never written to"""
    Cn, H, W, prec = image
    keep = {k: os.environ.pop(k, None) for k in REF_VARS}
    try:
        for k, v in env:
            os.environ[k] = str(v)
        cs, _ = R.encode(synth.g2(Cn, H, W, prec), prec, TW=TW, TH=TH, irrev=coder[1], numres=4, ht=int(coder[0] == "ht"), mode=1,
                         cblk=(1 << cblk[0], 1 << cblk[1]), cblksty=sty)
    finally:
        for k in REF_VARS:
            os.environ.pop(k, None)
            if keep[k] is not None:
                os.environ[k] = keep[k]
    want = R.decode(cs, Cn, H, W)
    want.setflags(write=False)
    return cs, want


def _check_header(cs, cblk, coder, sty=0):
    info = G.read_header(cs)
    assert (info.base.cblk_w_exp, info.base.cblk_h_exp) == cblk
    assert info.base.reserved[0] == int(coder[0] != "ht") and info.base.irreversible == coder[1]
    if coder[0] != "ht":
        assert info.base.reserved[1] == sty
    return info


def _where(got, want):
    """where two (C, H, W) arrays differ, for the assertion message"""
    d = np.argwhere(np.asarray(got) != np.asarray(want))
    return "%d samples differ, the first at (comp, y, x) = %s" % (len(d), tuple(int(v) for v in d[0])) if len(d) else "equal"


# ---- a. whole codestreams: grk_amd_decode_image == grk_decompress --------------------------------------------------------------
def _decode_image_case(image, coder, cblk, sty=0, env=(), TW=None, TH=None, layers=1, tiles=1):
    Cn, H, W, prec = image
    cs, want = _ref_stream(image, coder, cblk, sty, env, TW, TH)
    info = _check_header(cs, cblk, coder, sty)
    assert info.num_layers == layers and info.num_tiles == tiles
    got = U.ctx().decode_image(cs)
    what = "%s blocks, %s, style 0x%02x" % (_sz(cblk), _coder_id(coder), sty)
    assert np.array_equal(got.astype(np.int32), want), "%s: %s" % (what, _where(got, want))
    if not coder[1]:
        assert np.array_equal(got, synth.g2(Cn, H, W, prec)), what


@needs_ref
@pytest.mark.parametrize("image", IMAGES, ids=_img_id)
@pytest.mark.parametrize("coder", CODERS, ids=_coder_id)
@pytest.mark.parametrize("cblk", SIZES, ids=_sz)
def test_decode_image_at_every_block_size(cblk, coder, image):
    _decode_image_case(image, coder, cblk)


@needs_ref
@pytest.mark.parametrize("coder", CODERS, ids=_coder_id)
@pytest.mark.parametrize("cblk", CORE, ids=_sz)
def test_decode_image_ragged_nine_tiles(cblk, coder):
    """256 x 200 at offset (1, 1) in tiles of 100 x 77: nine tiles, several geometries, edge tiles a few samples wide"""
    _decode_image_case((3, 200, 256, 8), coder, cblk, env=(("REF_IMG_X0", 1), ("REF_IMG_Y0", 1)), TW=100, TH=77, tiles=9)


@needs_ref
@pytest.mark.parametrize("coder", CODERS, ids=_coder_id)
@pytest.mark.parametrize("cblk", CORE, ids=_sz)
def test_decode_image_with_precincts(cblk, coder):
    """precincts of 64 x 64 and 32 x 32: in the bands 32 x 32 and 16 x 16, which clip the nominal size in one direction or both"""
    _decode_image_case(IMAGES[0], coder, cblk, env=(("REF_PRECINCTS", "64,64,32,32"),))
    _decode_image_case(IMAGES[1], coder, cblk, env=(("REF_PRECINCTS", "64,64,32,32"),))


@needs_ref
@pytest.mark.parametrize("coder", CODERS, ids=_coder_id)
@pytest.mark.parametrize("cblk", CORE, ids=_sz)
def test_decode_image_with_three_layers(cblk, coder):
    """three quality layers: blocks gathered from several packets; for HT the SigProp / MagRef segments of small blocks"""
    _decode_image_case(IMAGES[0], coder, cblk, env=(("REF_LAYERS", "20,10,1"),), layers=3)
    _decode_image_case(IMAGES[1], coder, cblk, env=(("REF_LAYERS", "20,10,1"),), layers=3)


@needs_ref
@pytest.mark.parametrize("sty", [0x3F, 0x05, 0x08])
@pytest.mark.parametrize("irrev", [0, 1])
@pytest.mark.parametrize("cblk", CORE, ids=_sz)
def test_decode_image_part1_styles(cblk, irrev, sty):
    """every style, LAZY + TERMALL, and VSC alone -- in a 64 x 4 block the one stripe is the whole block"""
    for image in IMAGES:
        _decode_image_case(image, ("p1", irrev), cblk, sty=sty)


# ---- b. the table route (grk_amd_decode_tiles with the test-side Tier-2 reader) and what hangs off it ---------------------------
@needs_ref
@pytest.mark.parametrize("image", IMAGES, ids=_img_id)
@pytest.mark.parametrize("coder", CODERS, ids=_coder_id)
@pytest.mark.parametrize("cblk", CORE, ids=_sz)
def test_table_route_full_reduced_and_windowed(cblk, coder, image):
    from test_gpu_decode import _gpu_decode_reference_stream
    from test_gpu_reduce import _reference_stream, _gpu_reduced, _ref
    Cn, H, W, prec = image
    cs, want = _ref_stream(image, coder, cblk)
    part1 = coder[0] != "ht"
    what = "%s blocks, %s" % (_sz(cblk), _coder_id(coder))
    got = _gpu_decode_reference_stream(cs, part1=part1)
    assert np.array_equal(got.astype(np.int32), want), "%s: %s" % (what, _where(got, want))
    p, table, data, qcd, segs = _reference_stream(cs, part1)
    assert (p.cblk_w_exp, p.cblk_h_exp) == cblk
    c = U.ctx()
    for r in (1, 2):
        _, _, w, h = G.reduced_tile_rect(p, r)
        red = _gpu_reduced(c, p, table, data, r, qcd, segs)[0]
        assert red.shape == (Cn, h, w)
        ref = _ref(cs, r, (w, h))
        assert np.array_equal(red.astype(np.int32), ref), "%s, reduce %d: %s" % (what, r, _where(red, ref))
    # windows that cut through blocks of every resolution: a corner and the middle == grk_decompress_set_window; the last columns
    # and rows == the crop of the full decode only -- with blocks below 64 x 64 the reference's windowed decode leaves windows
    # away from the origin undecoded (defect D12, as test_random_reference_streams_full_and_windowed notes), which the first
    # two are checked not to be
    c.set_decode_qcd(list(qcd))
    if segs:
        c.set_decode_segments(segs)
    try:
        for k, (x0, y0, x1, y1) in enumerate(((0, 0, W // 3, H // 3), (W // 6 + 1, H // 10 + 1, W - 7, H - 9), (W - 13, H - 5, W, H))):
            win = c.decode_region_host(p, table, data, x0, y0, x1, y1).astype(np.int32)
            crop = want[:, y0:y1, x0:x1]
            assert np.array_equal(win, crop), "%s, window %s: %s" % (what, (x0, y0, x1, y1), _where(win, crop))
            if k < 2:
                assert np.array_equal(R.decode_window(cs, Cn, x0, y0, x1, y1), crop), "the reference's window differs from its own full decode"
    finally:
        c.set_decode_qcd([])
        c.set_decode_segments(None)


@needs_ref
@pytest.mark.parametrize("coder", CODERS, ids=_coder_id)
@pytest.mark.parametrize("cblk", [FLAT, (4, 4)], ids=_sz)
def test_plugin_decode(cblk, coder):
    """through the reference's loader and decode protocol: cblockw_init / cblockh_init of the header give the tree its blocks"""
    assert R.plugin_load() == 1
    assert R.plugin_init(0) == 1
    for image in IMAGES:
        Cn, H, W, prec = image
        cs, want = _ref_stream(image, coder, cblk)
        got, stages = R.plugin_decompress(cs, Cn, H, W)
        assert not isinstance(got, int), "plugin declined %s %s: %s (stages %s)" % (_sz(cblk), _coder_id(coder), got, stages)
        assert stages[1] >= 1 and stages[2] >= 1, stages
        assert np.array_equal(got, want), "%s %s: %s" % (_sz(cblk), _coder_id(coder), _where(got, want))


# ---- c. HT 9/7: no reference bytes exist (D1); this encoder's own tile against the oracle chain ---------------------------------
def _split(table, coded):
    return [bytes(coded[int(o):int(o) + int(n)]) for o, n in zip(table["offset"], table["length"])]


def _differing(blocks, got, want):
    return [(i, b.res, b.band, b.x1 - b.x0, b.y1 - b.y0, len(got[i]), len(want[i])) for i, b in enumerate(blocks) if got[i] != want[i]]


@pytest.mark.parametrize("cblk", CORE, ids=_sz)
def test_ht_irreversible_tile_equals_oracle_chain(cblk):
    px = synth.g2(3, 128, 192, 10)
    p, blocks, qcd, otable, ocoded = chain.encode_tile_oracle(px, 10, 3, irrev=True, cblk=cblk)
    assert (p.cblk_w_exp, p.cblk_h_exp) == cblk and max(b.x1 - b.x0 for b in blocks) == 1 << cblk[0] and max(b.y1 - b.y0 for b in blocks) == 1 << cblk[1]
    table, coded = U.ctx().encode_host(p, px)
    bad = _differing(blocks, _split(table, coded), _split(otable, ocoded))
    assert not bad, "%s: blocks differing from the oracle (idx, res, band, w, h, len_gpu, len_oracle): %s" % (_sz(cblk), bad[:8])
    want = chain.decode_tile_oracle(p, blocks, qcd, table, coded)
    got = U.ctx().decode_host(p, table, coded)[0]
    assert np.array_equal(got.astype(np.int32), want), "%s: %s" % (_sz(cblk), _where(got, want))


# ---- d. the encoder beyond the packed pair form ------------------------------------------------------------------------------------
@needs_ref
@pytest.mark.parametrize("prec", [12, 16])
@pytest.mark.parametrize("cblk", ENC_SIZES, ids=_sz)
def test_encode_int32_planes_file_equals_reference(cblk, prec):
    """12 and 16 bits: K3 reads int32 planes (the packed pair form is the 8-bit path's)"""
    from test_gpu_stages import gpu_codestream
    px = (synth.g2_mid if prec == 16 else synth.g2)(3, 130, 200, prec)
    want, _ = R.encode(px, prec, numres=4, mode=1, cblk=(1 << cblk[0], 1 << cblk[1]))
    got = gpu_codestream(px, prec, 3, cblk=cblk)
    assert got == want, "%s at %d bits: %d bytes, the reference's file has %d" % (_sz(cblk), prec, len(got), len(want))


@pytest.mark.parametrize("cblk", ENC_SIZES, ids=_sz)
def test_encode_8bit_planes_and_lds_settings_agree(cblk, monkeypatch):
    """8 bits: int16 planes and capped LDS buffers (default) == int32 planes (GRK_AMD_PLANES16=0) == worst-case LDS buffers without
    the fallback launch (GRK_AMD_LDS_CAP=0) == the oracle chain; 0 / 255 checkerboards in the upper half push the coefficients"""
    C_, H, W, L = 3, 130, 200, 3
    px = synth.g2(C_, H, W, 8)
    yy, xx = np.mgrid[0:H, 0:W]
    px[:, :H // 2] = np.where(((yy[:H // 2] // 3 + xx[:H // 2] // 5) & 1) == 0, 0, 255).astype(np.uint8)
    p = G.TileParams.make(W, H, C_, 8, L, cblk=cblk)
    blocks, _ = G.tile_layout(p)
    got = {}
    for planes16, cap in (("1", "1"), ("0", "1"), ("1", "0"), ("0", "0")):
        monkeypatch.setenv("GRK_AMD_PLANES16", planes16)
        monkeypatch.setenv("GRK_AMD_LDS_CAP", cap)
        c = G.Context(0)
        try:
            t, coded = c.encode_host(p, px)
            got[(planes16, cap)] = _split(t, coded)
        finally:
            c.close()
    _, _, _, otable, ocoded = chain.encode_tile_oracle(px, 8, L, cblk=cblk)
    want = _split(otable, ocoded)
    for k, v in got.items():
        bad = _differing(blocks, v, want)
        assert not bad, "%s, GRK_AMD_PLANES16=%s GRK_AMD_LDS_CAP=%s: blocks differing from the oracle (idx, res, band, w, h, len_gpu, len_oracle): %s" % (
            (_sz(cblk),) + k + (bad[:8],))


@needs_ref
@pytest.mark.parametrize("tiles", [(256, 192), (128, 96)], ids=["one", "2x2"])
@pytest.mark.parametrize("cblk", [FLAT, (2, 2)], ids=_sz)
def test_encode_image_both_tier2_routes_equal_reference(cblk, tiles, monkeypatch):
    """grk_amd_encode_image with Tier-2 on the device and on the host: one file, the reference's.  With 4 x 4 blocks a 256 x 192
    tile has 3 000 blocks a component: long packet headers, deep tag trees"""
    W, H, L = 256, 192, 3
    TW, TH = tiles
    px = synth.g2(3, H, W, 8)
    want, _ = R.encode(px, 8, TW=TW, TH=TH, numres=L + 1, mode=1, cblk=(1 << cblk[0], 1 << cblk[1]))
    layout = G.ImageLayout.make(W, H, TW, TH)
    base = G.TileParams.make(1, 1, 3, 8, L, cblk=cblk)
    c = U.ctx()
    monkeypatch.delenv("GRK_AMD_IMAGE_T2", raising=False)
    dev = c.encode_image(layout, base, px)
    monkeypatch.setenv("GRK_AMD_IMAGE_T2", "host")
    host = c.encode_image(layout, base, px)
    assert host == want, "%s, host Tier-2: %d bytes, the reference's file has %d" % (_sz(cblk), len(host), len(want))
    assert dev == want, "%s, device Tier-2: %d bytes, the reference's file has %d" % (_sz(cblk), len(dev), len(want))


# ---- e. synthetic blocks: the content is chosen, not found -----------------------------------------------------------------------
@pytest.mark.parametrize("cblk", SYNTH_SIZES, ids=_sz)
def test_ht_refinement_passes(cblk):
    """cleanup-only, two- and three-pass blocks mixed, every eleventh refinement segment truncated (test_gpu_ht_refine._case)"""
    from test_gpu_ht_refine import _case
    n = _case(200, 120, 2, 3, 8, False, 31, lambda i: (i % 3) + 1, cblk=cblk)
    assert n[1] >= 1 and n[2] >= 1 and n[3] >= 1
    _case(130, 67, 4, 1, 12, True, 32, lambda i: 3 if i % 2 else 2, cblk=cblk)
    _case(37, 3, 1, 1, 8, True, 33, lambda i: 3, cblk=cblk)


RAGGED = [(200, 120, 2, 3, 8), (130, 67, 5, 1, 12), (37, 3, 1, 1, 8)]


@pytest.mark.parametrize("W,H,L,C_,prec", RAGGED)
@pytest.mark.parametrize("cblk", SYNTH_SIZES, ids=_sz)
def test_ht_encode_blocks_ragged(cblk, W, H, L, C_, prec):
    from test_gpu_stages import _ht_case
    _ht_case(W, H, L, C_, prec, 1, W + H, cblk=cblk)


@pytest.mark.parametrize("W,H,L,C_,prec", RAGGED)
@pytest.mark.parametrize("cblk", SYNTH_SIZES, ids=_sz)
def test_ht_decode_blocks_ragged(cblk, W, H, L, C_, prec):
    from test_gpu_decode import _ht_dec_case
    _ht_dec_case(W, H, L, C_, prec, 1, W + H, cblk=cblk)
    _ht_dec_case(W, H, L, C_, prec, 1, W + H + 1, irrev=True, cblk=cblk)


def _lane_routes(p, table, coded):
    """the tile through the four routes of test_gpu_t1_lanes: pass-synchronous lanes, free-running lanes, waves, the default"""
    from test_gpu_t1_lanes import _ctx_with
    d_c = U.to_dev(np.frombuffer(coded, np.uint8))
    outs = {}
    for name, env in (("lanes", {"GRK_AMD_T1_LANES": "2"}), ("free", {"GRK_AMD_T1_LANES": "2", "GRK_AMD_T1_SYNC": "0"}),
                      ("waves", {"GRK_AMD_T1_LANES": "0"}), ("auto", {})):
        c = _ctx_with(env)
        d_m = U.dev_planes(p, 1)
        c.stage_ht_decode(p, 1, table, d_c.data_ptr(), d_c.numel(), d_m.data_ptr())
        c.synchronize()
        outs[name] = U.planes_to_numpy(d_m, p, 1)[0].copy()
        c.close()
    return outs


def _check_routes(outs, want, blocks, cblk):
    half = np.where(want < 0, -((-want) // 2), want // 2)          # ShiftFilter: v / 2 toward zero
    for name, got in outs.items():
        bad = [(i, b.res, b.band, b.x1 - b.x0, b.y1 - b.y0) for i, b in enumerate(blocks)
               if not np.array_equal(got[b.py:b.py + b.y1 - b.y0, b.px:b.px + b.x1 - b.x0], half[b.py:b.py + b.y1 - b.y0, b.px:b.px + b.x1 - b.x0])]
        assert not bad, "%s blocks, route %s: blocks differing from the oracle (idx, res, band, w, h): %s" % (_sz(cblk), name, bad[:8])
        assert np.array_equal(got, half)


def _planned_lanes(table, blocks, sync=True):
    """the lane list plan_t1_lists makes of this table with the lane decoder forced on (GRK_AMD_T1_LANES=2), spare lanes left out"""
    import test_decode_plan_cpu as DP
    lane, tail, _ = DP.t1_lists(table, [b.y1 - b.y0 for b in blocks], lanes=2, sync=sync)
    return [i for i in lane if i != DP.constants()["noblock"]]


# W, H, L, bits: mono 12-bit tiles of at most 1 500 blocks.  The lane list takes blocks no longer than 64 bytes or a quarter of the
# longest.  With 256 samples a block, one bit-plane stays under 64 bytes: every full block goes to the lanes.  With more
# bit-planes (more than the clean-up pass), and at the 1 024-sample sizes, the lanes' blocks are those of a last block column
# two to ten samples wide -- W is chosen so that there are 64 of them -- beside full blocks in the wave decoder's tail
LANE_CASES = [((4, 4), 500, 330, 1, 1), ((4, 4), 134, 530, 1, 3), (TALL, 260, 330, 1, 1), (TALL, 260, 330, 1, 2), ((3, 5), 260, 330, 1, 1),
              ((3, 5), 68, 1040, 1, 2), ((6, 4), 148, 1060, 1, 3), ((5, 5), 140, 1100, 1, 3)]


@needs_ref
@pytest.mark.parametrize("cblk,W,H,L,bits", LANE_CASES, ids=["%s-%dbit" % (_sz(k[0]), k[4]) for k in LANE_CASES])
def test_lane_decoder_at_small_block_sizes(cblk, W, H, L, bits):
    from test_gpu_t1_lanes import _tile
    rng = np.random.default_rng(W + H + bits)
    p, blocks, table, coded, want = _tile(rng, W, H, L, bits, 12, cblk=cblk)
    assert len(blocks) <= 1500 and max(b.y1 - b.y0 for b in blocks) == 1 << cblk[1]
    groups = {}
    for i, b in enumerate(blocks):
        if b.y1 - b.y0 >= 9:
            groups[int(table["missing_msbs"][i])] = groups.get(int(table["missing_msbs"][i]), 0) + 1
    assert max(groups.values()) >= 64, "the case must reach the lane decoder"
    assert len(_planned_lanes(table, blocks)) >= 64 and len(_planned_lanes(table, blocks, sync=False)) >= 64, "the plan must use the lanes"
    _check_routes(_lane_routes(p, table, coded), want, blocks, cblk)


@needs_ref
@pytest.mark.parametrize("cblk", [FLAT, (6, 3)], ids=_sz)
def test_blocks_under_nine_rows_stay_with_the_wave_decoder(cblk):
    """4 and 8 rows: one and two stripes, below the lane decoder's three -- none is planned for the lanes even where they are forced
    on, and what the wave decoder makes of them == the oracle"""
    from test_gpu_t1_lanes import _tile
    rng = np.random.default_rng(7 + cblk[1])
    p, blocks, table, coded, want = _tile(rng, 520, 200, 1, 2, 12, cblk=cblk)
    assert len(blocks) <= 1500 and max(b.y1 - b.y0 for b in blocks) == 1 << cblk[1] < 9
    assert _planned_lanes(table, blocks) == [] and _planned_lanes(table, blocks, sync=False) == []
    _check_routes(_lane_routes(p, table, coded), want, blocks, cblk)
