"""CPU: the plan of grk_amd_decode_image_view (grok_amd/csrc/image_view_plan.cpp through grk_amd_plan_image_view /
grk_amd_image_view_size) -- which tiles a view touches, what every unit delivers at the view's reduce and where it goes -- against
hand-worked literals, the partition property, grk_amd_layout_tile and, where oracle/_ref is present, the reference's header."""
import numpy as np
import pytest

import grok_amd as G
import refharness as R
import synth
from grok_amd.capi import CODED_DTYPE
from test_t2_reader_subsampled_cpu import S420, write_subsampled

REF_VARS = ("REF_PROG_ORDER", "REF_PRECINCTS", "REF_CSTY", "REF_WRITE_PLT", "REF_WRITE_TLM", "REF_LAYERS", "REF_IMG_X0", "REF_IMG_Y0")
NO_BLOCKS = np.zeros(1 << 16, CODED_DTYPE)          # (every block empty: the plan needs the main header only)


def plain_info(W, H, TW, TH, off, levels):
    layout = G.ImageLayout.make(W, H, TW, TH, offset=off)
    base = G.TileParams.make(TW, TH, 3, 8, levels)
    return G.read_header(G.write_codestream_layout(layout, base, NO_BLOCKS, np.zeros(1, np.uint8)))


def info_a():       # 200 x 136 at (5, 3), tiles 64 x 48: columns 5 64 128 192 205, rows 3 48 96 139 -> 4 x 3 tiles
    return plain_info(200, 136, 64, 48, (5, 3), 3)


def info_b():       # 150 x 90 at (7, 9), tiles 50 x 30: columns 7 50 100 150 157, rows 9 30 60 90 99 -> 4 x 4 tiles
    return plain_info(150, 90, 50, 30, (7, 9), 2)


def info_c():       # 202 x 138, 4:2:0, tiles 64 x 48: 4 x 3 tiles of two runs (luma; the two chroma components)
    layout = G.ImageLayout.make(202, 138, 64, 48)
    base = G.TileParams.make(64, 48, 3, 8, 3, mct=False)
    return G.read_header(write_subsampled(layout, base, S420, NO_BLOCKS, np.zeros(1, np.uint8), 0))


def test_view_sizes_are_the_ceilings_of_the_image_bounds():
    # A: ceil(205 / 2^r) - ceil(5 / 2^r), ceil(139 / 2^r) - ceil(3 / 2^r)
    assert [G.image_view_size(info_a(), r)[0] for r in range(4)] == [(200, 136), (100, 68), (50, 34), (25, 17)]
    # B: at r = 2 the resolutions hold 40 - 2 = 38 columns and 25 - 3 = 22 rows (the reference's header says 38 x 23)
    assert [G.image_view_size(info_b(), r)[0] for r in range(3)] == [(150, 90), (75, 45), (38, 22)]
    # C: every component from its own bounds
    c = info_c()
    assert G.image_view_size(c, 0) == [(202, 138), (101, 69), (101, 69)]
    assert G.image_view_size(c, 1) == [(101, 69), (51, 35), (51, 35)]
    assert G.image_view_size(c, 2) == [(51, 35), (26, 18), (26, 18)]
    assert G.image_view_size(c, 3) == [(26, 18), (13, 9), (13, 9)]
    # a window's size is the window's, in every component
    assert G.image_view_size(info_a(), 1, (3, 4, 50, 60)) == [(47, 56)] * 3


def test_reduced_units_of_stream_a_at_r1_are_these():
    plan = G.plan_image_view(info_a(), 1)
    assert list(plan["tiles"]) == list(range(12))
    u = plan["units"]
    # columns 5 64 128 192 205 -> 3 32 64 96 103; rows 3 48 96 139 -> 2 24 48 70; the view starts at (3, 2)
    assert [int(v) for v in u["x"][:4]] == [0, 29, 61, 93] and [int(v) for v in u["w"][:4]] == [29, 32, 32, 7]
    assert [int(v) for v in u["y"][0::4]] == [0, 22, 46] and [int(v) for v in u["h"][0::4]] == [22, 24, 22]
    assert all(u["whole"] == 1) and all(u["num_comps"] == 3) and all(u["first_comp"] == 0)


@pytest.mark.parametrize("make,levels", [(info_a, 3), (info_b, 2), (info_c, 3)])
def test_reduced_rectangles_partition_the_view(make, levels):
    info = make()
    for r in range(levels + 1):
        sizes = G.image_view_size(info, r)
        plan = G.plan_image_view(info, r)
        assert len(plan["tiles"]) == info.num_tiles
        for k, (w, h) in enumerate(sizes):
            cover = np.zeros((h, w), np.int32)
            for u in plan["units"]:
                if u["first_comp"] <= k < u["first_comp"] + u["num_comps"]:
                    assert u["x"] >= 0 and u["y"] >= 0 and u["whole"] == 1
                    cover[u["y"]:u["y"] + u["h"], u["x"]:u["x"] + u["w"]] += 1
            assert cover.min() == 1 and cover.max() == 1, (r, k)


def test_touched_tiles_and_signed_positions_of_windows():
    a = info_a()                                   # tile columns start at 0 59 123 187 of the image, rows at 0 45 93
    one = G.plan_image_view(a, 0, (70, 50, 100, 80))
    assert list(one["tiles"]) == [5]
    u = one["units"][0]
    assert (u["tile"], u["w"], u["h"], u["x"], u["y"], u["whole"]) == (5, 64, 48, 59 - 70, 45 - 50, 0)
    corner = G.plan_image_view(a, 0, (58, 44, 60, 46))
    assert list(corner["tiles"]) == [0, 1, 4, 5]
    assert [(int(v["x"]), int(v["y"])) for v in corner["units"]] == [(-58, -44), (1, -44), (-58, 1), (1, 1)]
    assert [(int(v["w"]), int(v["h"])) for v in corner["units"]] == [(59, 45), (64, 45), (59, 48), (64, 48)]
    # the same image at the origin: the seams are the tile grid's
    o = plain_info(200, 136, 64, 48, (0, 0), 3)
    corner = G.plan_image_view(o, 0, (63, 47, 66, 50))
    assert list(corner["tiles"]) == [0, 1, 4, 5]
    assert [(int(v["x"]), int(v["y"])) for v in corner["units"]] == [(-63, -47), (1, -47), (-63, 1), (1, 1)]
    assert list(G.plan_image_view(o, 0, (64, 48, 128, 96))["tiles"]) == [5]            # exactly one tile: held wholly
    assert G.plan_image_view(o, 0, (64, 48, 128, 96))["units"][0]["whole"] == 1
    assert list(G.plan_image_view(o, 0, (0, 0, 200, 136))["tiles"]) == list(range(12))
    # window and reduce: the window counts in the reduced image's samples.  B at r = 1: columns 7 50 100 150 157 -> 4 25 50 75 79,
    # rows 9 30 60 90 99 -> 5 15 30 45 50; the view starts at (4, 5): a window one sample wide left of the seam at 25 - 4 = 21
    b = G.plan_image_view(info_b(), 1, (20, 0, 21, 45))
    assert list(b["tiles"]) == [0, 4, 8, 12]
    assert [(int(v["x"]), int(v["y"]), int(v["w"]), int(v["h"])) for v in b["units"]] == [(-20, 0, 21, 10), (-20, 10, 21, 15), (-20, 25, 21, 15), (-20, 40, 21, 5)]
    b = G.plan_image_view(info_b(), 1, (21, 10, 22, 11))
    assert list(b["tiles"]) == [5] and (int(b["units"][0]["x"]), int(b["units"][0]["y"])) == (0, 0)


@pytest.mark.parametrize("make", [info_a, info_b])
def test_the_all_zero_view_is_the_tiles_of_layout_tile(make):
    info = make()
    plan = G.plan_image_view(info)
    tiles = G.layout_tiles(info.layout, info.base)
    assert list(plan["tiles"]) == list(range(len(tiles))) and len(plan["units"]) == len(tiles)
    for p, u in zip(tiles, plan["units"]):
        assert (u["w"], u["h"], u["x"], u["y"], u["whole"]) == (p.tile_w, p.tile_h, p.tile_x0 - info.layout.x0, p.tile_y0 - info.layout.y0, 1)
    assert G.image_view_size(info) == [(info.layout.x1 - info.layout.x0, info.layout.y1 - info.layout.y0)] * 3


def test_the_all_zero_view_of_sub_sampled_components_is_their_tile_components():
    from test_t2_reader_subsampled_cpu import tile_comp
    info = info_c()
    plan = G.plan_image_view(info)
    assert G.image_view_size(info) == G.stream_comp_sizes(info)
    assert len(plan["units"]) == 2 * info.num_tiles
    for t in range(info.num_tiles):
        for run, (first, n, (dx, dy)) in enumerate([(0, 1, (1, 1)), (1, 2, (2, 2))]):
            p, u = tile_comp(info.layout, info.base, dx, dy, t), plan["units"][2 * t + run]
            assert (u["tile"], u["first_comp"], u["num_comps"], u["w"], u["h"], u["x"], u["y"]) == (t, first, n, p.tile_w, p.tile_h, p.tile_x0, p.tile_y0)


def test_refusals():
    a, c = info_a(), info_c()
    with pytest.raises(ValueError, match="invalid"):
        G.image_view_size(a, 4)                                # more than the levels
    assert G.image_view_size(a, 3)[0] == (25, 17)              # == levels: the LL band
    for win in [(10, 10, 10, 20), (10, 10, 20, 10), (30, 10, 20, 20), (0, 0, 0, 5), (0, 0, 201, 136), (0, 0, 200, 137), (199, 135, 201, 136)]:
        with pytest.raises(ValueError, match="invalid"):
            G.plan_image_view(a, 0, win)
    with pytest.raises(ValueError, match="invalid"):
        G.plan_image_view(a, 1, (0, 0, 101, 68))               # the window counts in the REDUCED image: 100 x 68
    G.plan_image_view(a, 1, (0, 0, 100, 68))
    for r in (0, 1):
        with pytest.raises(ValueError, match="unsupported"):
            G.plan_image_view(c, r, (0, 0, 10, 10))            # a window of sub-sampled components
        with pytest.raises(ValueError, match="unsupported"):
            G.image_view_size(c, r, (0, 0, 10, 10))
    with pytest.raises(ValueError, match="invalid"):
        G.plan_image_view(c, 4)


@pytest.mark.skipif(not R.have_ref(), reason="oracle/_ref (the real reference) not built here")
@pytest.mark.parametrize("off", [(0, 0), (4, 8), (5, 3)])
def test_view_size_against_the_reference_header(monkeypatch, off):
    """on the 2^r grid the reference's header gives the same size; off it, it sizes the image from its width: at most one more"""
    import reducehost
    for k in REF_VARS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("REF_IMG_X0", str(off[0]))
    monkeypatch.setenv("REF_IMG_Y0", str(off[1]))
    cs, _ = R.encode(synth.g2(3, 136, 200, 8), 8, TW=64, TH=48, numres=4, mode=1)
    info = G.read_header(cs)
    for r in (1, 2, 3):
        w, h = G.image_view_size(info, r)[0]
        for _, _, rw, rh in reducehost.header_rects(cs, r):
            on_grid = off[0] % (1 << r) == 0 and off[1] % (1 << r) == 0
            if on_grid:
                assert (w, h) == (rw, rh), (r, off)
            else:
                assert 0 <= rw - w <= 1 and 0 <= rh - h <= 1, (r, off, (w, h), (rw, rh))
