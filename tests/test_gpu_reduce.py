"""GPU: decode at reduced resolution (grk_amd_set_decode_reduce; grk_decompress -r N) == the reference's decode with cp_reduce,
pixel for pixel, through every decode mode of the C ABI."""
import numpy as np
import pytest
import torch

import grok_amd as G
import gpuutil as U
import j2kparse as J
import reducehost as RH
import refharness as R
import synth

pytestmark = pytest.mark.gpu
needs_ref = pytest.mark.skipif(not RH.have(), reason="oracle/_ref not shipped")


def _ref(cs, r, wh):
    got = RH.decode(cs, r)
    assert not isinstance(got, int), "reference refused reduce %d: %d" % (r, got)
    return np.stack(RH.crop(got, wh))


def _signed(a, p):
    return a.view(np.int8 if p.prec <= 8 else np.int16).astype(np.int32) if p.sgnd else a.astype(np.int32)


def _reference_stream(cs, part1):
    """(params, table, coded, QCD words, segment list) of a reference stream, as _gpu_decode_reference_stream builds them"""
    info = J.parse(cs)
    p = G.TileParams.make(info["W"], info["H"], info["C"], info["prec"], info["levels"],
                          irreversible=bool(info["irreversible"]), mct=bool(info["mct"]), part1=part1,
                          cblksty=info["cblk_sty"] & 0x3F if part1 else 0, origin=(info["x0"], info["y0"]),
                          precincts=info["prc"] if info["scod"] & 1 else None, cblk=(info["cbw"], info["cbh"]))
    blocks, _ = G.tile_layout(p)
    rows, data = J.decode_table(info, blocks, part1)
    qcd = [(e << 11) | m for e, m in info["qcd"]] if info["irreversible"] else []
    segs = J.segment_list(info, blocks) if part1 and info["cblk_sty"] & 0x05 else None
    return p, np.array(rows, dtype=G.capi.CODED_DTYPE), data, qcd, segs


def _gpu_reduced(c, p, table, data, r, qcd=(), segs=None, ntiles=1):
    c.set_decode_qcd(list(qcd))
    if segs:
        c.set_decode_segments(segs)
    c.set_decode_reduce(r)
    try:
        return c.decode_host(p, table, data, ntiles=ntiles)
    finally:
        c.set_decode_reduce(0)
        c.set_decode_qcd([])
        c.set_decode_segments(None)


def test_reduce_symbols_exported_and_checked():
    """the two entry points exist; a reduce above the tile's levels is refused by the call, the rectangle helper refuses it too"""
    L = G.lib()
    assert hasattr(L, "grk_amd_set_decode_reduce") and hasattr(L, "grk_amd_reduced_tile_rect")
    c = U.ctx()
    p = G.TileParams.make(64, 48, 1, 8, 2)
    px = synth.g2(1, 48, 64, 8)
    table, coded = c.encode_host(p, px)
    c.set_decode_reduce(3)
    try:
        with pytest.raises(RuntimeError, match="-3"):
            c.decode_host(p, table, coded)
    finally:
        c.set_decode_reduce(0)
    assert np.array_equal(c.decode_host(p, table, coded)[0], px)


# C, H, W, prec, numres, image origin, precincts (grk_compress -c, highest resolution first)
SHAPES = [(3, 96, 160, 8, 5, (0, 0), None), (1, 128, 128, 8, 4, (0, 0), None), (3, 100, 77, 12, 4, (3, 6), None),
          (3, 256, 192, 8, 5, (0, 0), "128,128,64,64,32,32"), (1, 61, 97, 10, 3, (5, 2), None)]


@needs_ref
@pytest.mark.parametrize("C_,H,W,prec,numres,off,prc", SHAPES)
@pytest.mark.parametrize("kind", ["ht", "part1", "part1_97"])
def test_reduced_decode_of_reference_streams(monkeypatch, C_, H, W, prec, numres, off, prc, kind):
    """grk_compress streams (HT reversible, Part-1 reversible, Part-1 ICT + 9/7) decoded with every r in 0..L == the reference's
    decode with cp_reduce = r"""
    monkeypatch.setenv("REF_IMG_X0", str(off[0]))
    monkeypatch.setenv("REF_IMG_Y0", str(off[1]))
    if prc:
        monkeypatch.setenv("REF_PRECINCTS", prc)
    px = synth.g2(C_, H, W, prec)
    cs, _ = R.encode(px, prec, TW=off[0] + W, TH=off[1] + H, numres=numres, mode=1, ht=int(kind == "ht"),
                     irrev=int(kind == "part1_97"))
    p, table, data, qcd, segs = _reference_stream(cs, kind != "ht")
    c = U.ctx()
    for r in range(numres):
        _, _, w, h = G.reduced_tile_rect(p, r)
        got = _gpu_reduced(c, p, table, data, r, qcd, segs)[0]
        assert got.shape == (C_, h, w)
        assert np.array_equal(got.astype(np.int32), _ref(cs, r, (w, h))), "reduce %d" % r


@needs_ref
@pytest.mark.parametrize("sty", [0x01, 0x04, 0x01 | 0x04, 0x3F])
@pytest.mark.parametrize("irrev", [0, 1])
def test_reduced_decode_of_styled_part1_streams(sty, irrev):
    """grk_compress -M streams with several codeword segments per block (the segment list over the FULL tile's blocks): r = 1 and
    r = L == the reference"""
    px = synth.g2(3, 128, 192, 10)
    cs, _ = R.encode(px, 10, numres=4, mode=1, ht=0, irrev=irrev, cblksty=sty)
    p, table, data, qcd, segs = _reference_stream(cs, True)
    assert segs
    c = U.ctx()
    for r in (1, p.num_levels):
        _, _, w, h = G.reduced_tile_rect(p, r)
        got = _gpu_reduced(c, p, table, data, r, qcd, segs)[0]
        assert np.array_equal(got.astype(np.int32), _ref(cs, r, (w, h))), "reduce %d" % r


def _own_stream(c, p, px):
    table, coded = c.encode_host(p, px)
    cs = G.write_codestream(p, p.tile_w, p.tile_h, table, coded)
    return table, coded, cs


@needs_ref
@pytest.mark.parametrize("C_,H,W,prec,L", [(3, 256, 256, 8, 5), (3, 200, 136, 12, 4), (1, 128, 192, 10, 3)])
def test_reduced_decode_of_own_ht_irreversible_stream(C_, H, W, prec, L):
    """this library's HT irreversible stream with its DEFAULT step sizes (no set_decode_qcd): r = 1, 2 == the reference's reduced
    decode of the same file -- the steps are the full tile's, not those of a tile with fewer levels"""
    c = U.ctx()
    p = G.TileParams.make(W, H, C_, prec, L, irreversible=True)
    px = synth.g2_mid(C_, H, W, prec)                     # (content the reference's HT decoder accepts: defect D5, synth.g2_mid)
    table, coded, cs = _own_stream(c, p, px)
    assert np.array_equal(c.decode_host(p, table, coded)[0].astype(np.int32), _ref(cs, 0, (W, H)))
    for r in (1, 2):
        _, _, w, h = G.reduced_tile_rect(p, r)
        c.set_decode_reduce(r)
        try:
            got = c.decode_host(p, table, coded)[0]
        finally:
            c.set_decode_reduce(0)
        assert np.array_equal(got.astype(np.int32), _ref(cs, r, (w, h))), "reduce %d" % r


@needs_ref
@pytest.mark.parametrize("prec,sgnd", [(1, False), (8, False), (12, False), (16, False), (12, True)])
def test_reduced_decode_to_ll_band_at_every_depth(prec, sgnd):
    """r = L (the LL band, no inverse level) and r = L - 1 at precisions 1, 8, 12, 16 and signed 12 bits == the reference.  Content
    whose blocks the reference's HT decoder refuses (U_q > missing_msbs, defect D5) is refused by ours as well; at least one kind
    of content per precision is decoded."""
    C_, H, W, L = 3, 96, 144, 3
    c = U.ctx()
    p = G.TileParams.make(W, H, C_, prec, L, sgnd=sgnd)
    decoded = 0
    for kind in ("ramp", "impulse", "checker", "low"):
        u = synth.content(kind, C_, H, W, prec)
        px = (u.astype(np.int32) - (1 << (prec - 1))).astype(np.int8 if prec <= 8 else np.int16) if sgnd else u
        table, coded, cs = _own_stream(c, p, px)
        for r in (L - 1, L):
            _, _, w, h = G.reduced_tile_rect(p, r)
            want = RH.decode(cs, r)
            c.set_decode_reduce(r)
            try:
                if isinstance(want, int):
                    with pytest.raises(RuntimeError):
                        c.decode_host(p, table, coded)
                    continue
                got = c.decode_host(p, table, coded)[0]
            finally:
                c.set_decode_reduce(0)
            assert got.shape == (C_, h, w)
            assert np.array_equal(_signed(got, p), np.stack(RH.crop(want, (w, h)))), (kind, r)
            decoded += 1
    assert decoded >= 2


@needs_ref
def test_reduced_decode_int16_planes_on_and_off():
    """8-bit reversible HT: the reduced output with int16 planes == with int32 planes == the reference"""
    C_, H, W, L = 3, 192, 256, 5
    c = U.ctx()
    p = G.TileParams.make(W, H, C_, 8, L)
    px = synth.g2(C_, H, W, 8)
    table, coded, cs = _own_stream(c, p, px)
    try:
        for r in (1, 2, 4):
            _, _, w, h = G.reduced_tile_rect(p, r)
            outs = []
            for on in (1, 0):
                c.set_decode_planes16(on)
                c.set_decode_reduce(r)
                outs.append(c.decode_host(p, table, coded)[0])
            assert np.array_equal(outs[0], outs[1])
            assert np.array_equal(outs[0].astype(np.int32), _ref(cs, r, (w, h))), "reduce %d" % r
    finally:
        c.set_decode_planes16(1)
        c.set_decode_reduce(0)


@pytest.mark.parametrize("irrev", [0, 1])
def test_reduced_region_decode_equals_crop(irrev):
    """grk_amd_decode_region with r = 1, 2: windows in the reduced tile's coordinates == the crop of the reduced full decode"""
    C_, H, W, L = 3, 300, 420, 4
    c = U.ctx()
    p = G.TileParams.make(W, H, C_, 8, L, irreversible=bool(irrev))
    px = synth.g2(C_, H, W, 8)
    table, coded = c.encode_host(p, px)
    try:
        for r in (1, 2):
            c.set_decode_reduce(r)
            _, _, w, h = G.reduced_tile_rect(p, r)
            full = c.decode_host(p, table, coded)[0]
            assert full.shape == (C_, h, w)
            wins = [(0, 0, 1, 1), (w - 1, 0, w, h), (0, h - 1, w, h), (0, 0, w, h), (w - 1, h - 1, w, h), (27, 25, 41, 40)]
            if r == 1:
                # (x = y = 128 of the reduced tile is band coordinate 64 of its top resolution: the window straddles a code-block
                #  boundary of every band there -- blocks on both sides needed, the next ones skipped)
                wins.append((121, 119, 136, 137))
            for (x0, y0, x1, y1) in wins:
                got = c.decode_region_host(p, table, coded, x0, y0, x1, y1)
                assert np.array_equal(got, full[:, y0:y1, x0:x1]), (r, (x0, y0, x1, y1))
            with pytest.raises(RuntimeError):
                c.decode_region_host(p, table, coded, 0, 0, w + 1, h)
    finally:
        c.set_decode_reduce(0)


def test_reduced_batch_equals_single_tiles():
    """ntiles = 3 in one call == three single-tile reduced decodes"""
    C_, H, W, L = 3, 128, 160, 4
    c = U.ctx()
    p = G.TileParams.make(W, H, C_, 8, L)
    tiles = [synth.g2(C_, H, W, 8, seed=40 + t) for t in range(3)]
    d_px = U.to_dev(np.concatenate([t.reshape(-1) for t in tiles]))
    table, tot = c.encode_tiles(p, 3, d_px.data_ptr(), True)
    coded = c.fetch_coded(tot)
    nb = len(table) // 3
    try:
        for r in (1, 2, L):
            c.set_decode_reduce(r)
            batch = c.decode_host(p, table, coded, ntiles=3)
            for t in range(3):
                one = c.decode_host(p, table[t * nb:(t + 1) * nb], coded)[0]
                assert np.array_equal(batch[t], one), (r, t)
    finally:
        c.set_decode_reduce(0)


def test_reduced_decode_sequence_alternating_r():
    """a sequence with 3 frames in flight whose frames alternate r = 0, 1, 2 on rotating device buffers (the slot wait of the
    header): each frame == its single-call result"""
    C_, H, W, prec, L = 3, 256, 384, 8, 4
    p = G.TileParams.make(W, H, C_, prec, L)
    c = G.Context(0)
    frames = []
    for f in range(9):
        px = synth.g2(C_, H, W, prec, seed=700 + f)
        table, coded = c.encode_host(p, px)
        r = f % 3
        c.set_decode_reduce(r)
        want = c.decode_host(p, table, coded)[0]
        frames.append((r, table, U.to_dev(np.frombuffer(bytes(coded), np.uint8).copy()), want))
    c.set_decode_reduce(0)
    cap = max(int(d.numel()) for _, _, d, _ in frames)
    n = 3
    cbuf = [torch.zeros(cap, dtype=torch.uint8, device="cuda") for _ in range(n)]
    obuf = [torch.zeros(C_ * H * W, dtype=torch.uint8, device="cuda") for _ in range(n)]
    kept = [torch.zeros(C_ * H * W, dtype=torch.uint8, device="cuda") for _ in frames]
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    c.set_stream(st.cuda_stream)
    c.set_decode_pipelining(n)
    try:
        with torch.cuda.stream(st):
            for f, (r, table, d_c, _) in enumerate(frames):
                c.decode_stream_wait_slot(st.cuda_stream)
                if f >= n:
                    kept[f - n].copy_(obuf[f % n], non_blocking=True)
                cbuf[f % n][:d_c.numel()].copy_(d_c, non_blocking=True)
                c.set_decode_reduce(r)
                c.decode_device(p, 1, table, cbuf[f % n].data_ptr(), d_c.numel(), obuf[f % n].data_ptr())
        c.synchronize()
        c.decode_status()
        torch.cuda.synchronize()
        for f in range(len(frames) - n, len(frames)):
            kept[f].copy_(obuf[f % n])
        torch.cuda.synchronize()
        for f, (r, _, _, want) in enumerate(frames):
            got = kept[f].cpu().numpy()[:want.size].reshape(want.shape)
            assert np.array_equal(got, want), "frame %d (reduce %d)" % (f, r)
    finally:
        c.set_decode_reduce(0)
        c.set_decode_pipelining(0)


@needs_ref
def test_plugin_with_cp_reduce():
    """Through the test host and the real loader with cp_reduce = 1 (grk_decompress -r 1): for an HT stream and a 4:2:0 stream the
    plugin serves the decode -- its Tier-2 and post-T1 stages ran -- and the pixels == the reference's reduced decode without the
    plugin; with cp_reduce above the stream's levels the outcome == the host's without the plugin (refused)."""
    assert hasattr(G.lib(), "grk_amd_set_decode_reduce")
    assert R.plugin_load() == 1
    assert R.plugin_init(0) == 1
    px = synth.g2(3, 192, 256, 8)
    cs, _ = R.encode(px, 8, numres=5, mode=1, ht=1)
    rc, planes, stages = RH.plugin_decompress(cs, 0)
    assert rc == 0 and stages[1] >= 1 and stages[2] >= 1, (rc, stages)
    assert np.array_equal(np.stack(planes), px.astype(np.int32))
    sub = [synth.g2(1, 96, 128, 8, seed=3)[0], synth.g2(1, 48, 64, 8, seed=4)[0], synth.g2(1, 48, 64, 8, seed=5)[0]]
    cs420 = R.encode_planes(sub, [(1, 1), (2, 2), (2, 2)], 8, 128, 96, numres=4)
    for stream, levels in ((cs, 4), (cs420, 3)):
        for r in (1, 2):
            want = RH.decode(stream, r)
            assert not isinstance(want, int)
            rc, planes, stages = RH.plugin_decompress(stream, r)
            assert rc == 0 and stages[1] >= 1 and stages[2] >= 1, (r, rc, stages)
            assert len(planes) == len(want)
            for k in range(len(want)):
                assert np.array_equal(planes[k], want[k]), (r, k)
        want = RH.decode(stream, levels + 3)
        assert isinstance(want, int)                     # the host refuses cp_reduce >= numresolutions ...
        rc, planes, stages = RH.plugin_decompress(stream, levels + 3)
        assert rc != 0 and planes is None, (rc, stages)  # ... and so does the route through the plugin
        assert stages[1] == 0, stages


@needs_ref
def test_reduced_decode_at_size():
    """one 8192 x 8192 x 3 8-bit HT frame with r = 2 == the reference's reduced decode of the same file"""
    C_, H, W, L = 3, 8192, 8192, 5
    c = U.ctx()
    p = G.TileParams.make(W, H, C_, 8, L)
    px = synth.g2(C_, H, W, 8)
    d_px = U.to_dev(px.reshape(-1))
    table, tot = c.encode_tiles(p, 1, d_px.data_ptr(), True)
    coded = c.fetch_coded(tot)
    del d_px
    cs = G.write_codestream(p, W, H, table, coded)
    _, _, w, h = G.reduced_tile_rect(p, 2)
    c.set_decode_reduce(2)
    try:
        got = c.decode_host(p, table, coded)[0]
    finally:
        c.set_decode_reduce(0)
    assert got.shape == (C_, h, w)
    assert np.array_equal(got.astype(np.int32), _ref(cs, 2, (w, h)))
