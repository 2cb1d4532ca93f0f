"""-m gpu: the decode-side HIP kernels against the CPU oracle, through the C-ABI, bit-exact."""
import numpy as np
import pytest
import torch

import grok_amd as G
import oracle as O
import chain
import synth
import gpuutil as U

pytestmark = pytest.mark.gpu

IDWT_CASES = [(8, 8, 1), (64, 64, 3), (65, 33, 3), (100, 77, 5), (17, 1, 2), (1, 9, 2), (3, 3, 1), (2, 2, 1),
              (255, 257, 5), (512, 512, 5), (1024, 1024, 5), (1500, 700, 4), (4, 600, 3), (1009, 64, 2)]


@pytest.mark.parametrize("W,H,L", IDWT_CASES)
def test_idwt53(W, H, L):
    rng = np.random.default_rng(W * 13 + H)
    a = rng.integers(-3000, 3000, size=(2, H, W)).astype(np.int32)         # arbitrary Mallat content
    p = G.TileParams.make(W, H, 1, 8, L, mct=False)
    d_in = U.upload_planes(a, p)
    d_out = U.dev_planes(p, 2)
    U.ctx().stage_dwt_inv(p, 2, d_in.data_ptr(), d_out.data_ptr())
    U.ctx().synchronize()
    got = U.planes_to_numpy(d_out, p, 2)
    for k in range(2):
        assert np.array_equal(got[k], O.dwt53_inv(a[k], L)), "plane %d" % k


@pytest.mark.parametrize("W,H,L", IDWT_CASES)
def test_idwt97_bit_exact(W, H, L):
    rng = np.random.default_rng(W * 17 + H)
    a = (rng.standard_normal((2, H, W)) * 200).astype(np.float32)
    p = G.TileParams.make(W, H, 1, 8, L, irreversible=True, mct=False)
    d_in = U.upload_planes(a.view(np.int32), p)
    d_out = U.dev_planes(p, 2)
    U.ctx().stage_dwt_inv(p, 2, d_in.data_ptr(), d_out.data_ptr())
    U.ctx().synchronize()
    got = U.planes_to_numpy(d_out, p, 2)
    for k in range(2):
        want = O.dwt97_inv(a[k], L).view(np.int32)
        assert np.array_equal(got[k], want), "plane %d: max int diff %d" % (
            k, np.abs(got[k].astype(np.int64) - want).max())


def test_fwd_then_inv_53_is_identity_8k():
    """Full-size property (one 8192^2 plane): the GPU inverse undoes the GPU forward transform."""
    rng = np.random.default_rng(5)
    W = H = 8192
    a = rng.integers(-128, 128, size=(1, H, W)).astype(np.int32)
    p = G.TileParams.make(W, H, 1, 8, 5, mct=False)
    d_in = U.upload_planes(a, p)
    d_m = U.dev_planes(p, 1)
    d_out = U.dev_planes(p, 1)
    U.ctx().stage_dwt_fwd(p, 1, d_in.data_ptr(), d_m.data_ptr())
    U.ctx().stage_dwt_inv(p, 1, d_m.data_ptr(), d_out.data_ptr())
    U.ctx().synchronize()
    assert np.array_equal(U.planes_to_numpy(d_out, p, 1)[0], a[0])


@pytest.mark.parametrize("C,H,W,prec,irrev", [(3, 64, 64, 8, 0), (3, 33, 70, 8, 0), (1, 17, 5, 8, 0), (3, 128, 256, 16, 0),
                                              (3, 64, 64, 8, 1), (3, 50, 101, 12, 1), (1, 64, 64, 8, 1), (4, 32, 36, 8, 0),
                                              (4, 32, 36, 10, 1)])
def test_egress(C, H, W, prec, irrev):
    rng = np.random.default_rng(C * 100 + W + prec)
    span = 1 << prec
    if irrev:
        planes = (rng.standard_normal((2, C, H, W)) * span / 3).astype(np.float32)
        planes[0, :, 0, :8] = np.array([0.5, 1.5, 2.5, -0.5, -1.5, 1e9, -1e9, 0.49999997], np.float32)[:min(8, W)] \
            if W >= 8 else planes[0, :, 0, :8]
        raw = planes.view(np.int32)
    else:
        raw = rng.integers(-span, span, size=(2, C, H, W)).astype(np.int32)
    p = G.TileParams.make(W, H, C, prec, 0, irreversible=bool(irrev))
    d_pl = U.upload_planes(raw.reshape(2 * C, H, W), p)
    bps = (prec + 7) // 8
    d_px = U._settled(torch.zeros(2 * C * H * W * bps, dtype=torch.uint8, device="cuda"))
    U.ctx().stage_egress(p, 2, d_pl.data_ptr(), d_px.data_ptr())
    U.ctx().synchronize()
    got = d_px.cpu().numpy().view(np.uint8 if bps == 1 else np.uint16).reshape(2, C, H, W)
    for t in range(2):
        want = np.stack(O.color_inv_store([raw[t, k] for k in range(C)], prec, bool(irrev), C >= 3))
        assert np.array_equal(got[t].astype(np.int32), want)


# ---- K5: HT cleanup decoder + dequantisation ------------------------------------------------------
def _ht_dec_case(W, H, L, C, prec, mode, seed, irrev=False, cblk=(6, 6)):
    """Random in-range Mallat planes -> oracle block encoder -> HIP decoder == the planes (rev) /
    == oracle decode (irrev)."""
    rng = np.random.default_rng(seed)
    p = G.TileParams.make(W, H, C, prec, L, irreversible=irrev, cblk=cblk)
    blocks, qcd = G.tile_layout(p)
    planes = np.zeros((C, H, W), np.int32)
    table = np.zeros(len(blocks), G.capi.CODED_DTYPE)
    chunks, off = [], 0
    for i, b in enumerate(blocks):
        bw, bh = b.x1 - b.x0, b.y1 - b.y0
        kb = b.kmax - 2                                   # decodable range (defect D5)
        mag = rng.integers(0, (1 << kb) + 1, size=(bh, bw))
        if mode == 1:
            mag = mag >> rng.integers(0, kb + 1, size=(bh, bw))
        elif mode == 2:
            mag = np.where(rng.random((bh, bw)) < 0.93, 0, mag & 7)
        elif mode == 3:
            mag = np.zeros((bh, bw), np.int64)
        elif mode == 4:
            mag = np.full((bh, bw), 1 << kb)
        sign = np.where(rng.random((bh, bw)) < 0.5, -1, 1)
        coef = (mag * sign).astype(np.int32)
        planes[b.comp, b.py:b.py + bh, b.px:b.px + bw] = coef
        cb = O.ht_encode_sm(O.signmag(coef, b.kmax), b.kmax)
        if mode == 3 and i % 3 == 0:
            cb = b""                                      # block without data
        table["offset"][i] = off; table["length"][i] = len(cb); table["missing_msbs"][i] = b.kmax - 1
        chunks.append(cb + b"\0" * (-len(cb) % 16)); off += len(chunks[-1])
    coded = b"".join(chunks) or b"\0" * 16
    d_c = U.to_dev(np.frombuffer(coded, np.uint8))
    d_m = U.dev_planes(p, C)
    U.ctx().stage_ht_decode(p, 1, table, d_c.data_ptr(), d_c.numel(), d_m.data_ptr())
    U.ctx().synchronize()
    got = U.planes_to_numpy(d_m, p, C)
    if not irrev:
        assert np.array_equal(got, planes)
    else:
        for i, b in enumerate(blocks):
            bw, bh = b.x1 - b.x0, b.y1 - b.y0
            sm = O.ht_decode_block(chunks[i][:int(table["length"][i])], b.kmax - 1, bw, bh) if table["length"][i] else np.zeros((bh, bw), np.uint32)
            want = O.ht_dequant_irrev(sm, chain.band_scale_dec(prec, qcd[chain.band_index(b)], b.kmax))
            assert np.array_equal(got[b.comp, b.py:b.py + bh, b.px:b.px + bw], want.view(np.int32)), "block %d" % i


@pytest.mark.parametrize("mode", [0, 1, 2, 3, 4])
def test_ht_decode_blocks_512(mode):
    _ht_dec_case(512, 512, 3, 1, 8, mode, 300 + mode)


@pytest.mark.parametrize("W,H,L,C,prec", [(200, 120, 2, 3, 8), (130, 67, 5, 1, 12), (1024, 1024, 5, 3, 8),
                                           (64, 64, 0, 1, 16), (37, 3, 1, 1, 8), (1, 1, 0, 1, 8)])
def test_ht_decode_blocks_ragged(W, H, L, C, prec):
    _ht_dec_case(W, H, L, C, prec, 1, W + H)


def test_ht_decode_irreversible_scale():
    _ht_dec_case(256, 192, 3, 3, 10, 1, 77, irrev=True)


def test_ht_decode_rejects_corrupt_block():
    p = G.TileParams.make(64, 64, 1, 8, 0)
    blocks, _ = G.tile_layout(p)
    cb = bytearray(O.ht_encode_sm(O.signmag(np.ones((64, 64), np.int32), blocks[0].kmax), blocks[0].kmax))
    cb[-1] = 0xFF; cb[-2] |= 0x0F
    table = np.zeros(1, G.capi.CODED_DTYPE)
    table["length"][0] = len(cb); table["missing_msbs"][0] = blocks[0].kmax - 1
    d_c = U.to_dev(np.frombuffer(bytes(cb) + b"\0" * 16, np.uint8))
    d_m = U.dev_planes(p, 1)
    with pytest.raises(RuntimeError):
        U.ctx().stage_ht_decode(p, 1, table, d_c.data_ptr(), d_c.numel(), d_m.data_ptr())


def test_ht_decode_vlc_cursor_past_its_segment_reads_the_blocks_own_padding():
    """A stream whose Scup claims a VLC / MEL segment much shorter than the block needs: K5a's cursors run past the
    words K5p prepared.  They must then read the block's OWN padding (zeros / ones) -- not the neighbour block's scratch, not memory
    behind the buffer: the planes such a call leaves (whether or not the block ends up rejected) do not depend on what the
    neighbours hold or on what an earlier call left in the scratch."""
    p = G.TileParams.make(128, 64, 1, 8, 0)
    blocks, _ = G.tile_layout(p)
    rng = np.random.default_rng(5)
    kmax = blocks[0].kmax

    def coded(mag_bits):
        coef = (rng.integers(0, 1 << mag_bits, size=(64, 64)) * np.where(rng.random((64, 64)) < 0.5, -1, 1)).astype(np.int32)
        return bytearray(O.ht_encode_sm(O.signmag(coef, kmax), kmax))

    bad = coded(kmax - 2)
    bad[-1] = 0x00; bad[-2] = (bad[-2] & 0xF0) | 0x03            # Scup = 3: one VLC byte, two MEL bytes
    outs = []
    for neighbour_bits, warm in ((kmax - 2, False), (2, True), (kmax - 3, True)):
        nb = coded(neighbour_bits)
        table = np.zeros(2, G.capi.CODED_DTYPE)
        # the malformed block LAST: its scratch ends the buffer
        table["offset"][0] = 0; table["length"][0] = len(nb); table["missing_msbs"][0] = kmax - 1
        off1 = (len(nb) + 15) & ~15
        table["offset"][1] = off1; table["length"][1] = len(bad); table["missing_msbs"][1] = kmax - 1
        buf = bytes(nb) + b"\0" * (off1 - len(nb)) + bytes(bad)
        if warm:                                                      # other contents in the scratch from a call before
            t2 = table.copy(); t2["length"][1] = 0
            d2 = U.to_dev(np.frombuffer(buf, np.uint8)); m2 = U.dev_planes(p, 1)
            U.ctx().stage_ht_decode(p, 1, t2, d2.data_ptr(), d2.numel(), m2.data_ptr()); U.ctx().synchronize()
        d_c = U.to_dev(np.frombuffer(buf, np.uint8))
        d_m = U.dev_planes(p, 1)
        try:
            U.ctx().stage_ht_decode(p, 1, table, d_c.data_ptr(), d_c.numel(), d_m.data_ptr())
        except RuntimeError:
            pass                                                      # (rejected: fine -- what it wrote must still be the same)
        U.ctx().synchronize()
        outs.append(U.planes_to_numpy(d_m, p, 1)[0, :, 64:128].copy())
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])


# ---- whole decode path ------------------------------------------------------------------------------
@pytest.mark.parametrize("C,H,W,prec,L,gen", [(1, 512, 512, 8, 3, "g2"), (3, 256, 384, 8, 5, "g2"), (3, 128, 128, 16, 4, "g2"),
                                               (3, 100, 77, 8, 3, "g2"), (1, 64, 64, 12, 0, "g2"), (3, 1024, 1024, 8, 5, "g2")])
def test_lossless_round_trip(C, H, W, prec, L, gen):
    """GPU encode -> GPU decode == source pixels (RCT + 5/3 + HT, both directions on the device)."""
    px = getattr(synth, gen)(C, H, W, prec)
    p = G.TileParams.make(W, H, C, prec, L)
    table, coded = U.ctx().encode_host(p, px)
    back = U.ctx().decode_host(p, table, coded)
    assert np.array_equal(back[0], px)


@pytest.mark.parametrize("C,H,W,prec,L", [(1, 128, 128, 8, 3), (3, 96, 160, 8, 4), (3, 128, 192, 12, 5), (1, 67, 45, 8, 2)])
def test_decode_irreversible_equals_oracle_chain(C, H, W, prec, L):
    """ICT + 9/7 + quantiser: blocks from the oracle encoder, decoded on the GPU == the oracle decode
    chain, which tests/test_oracle_decode.py pins to grk_decompress pixel for pixel."""
    px = synth.g2(C, H, W, prec)
    p, blocks, qcd, table, coded = chain.encode_tile_oracle(px, prec, L, irrev=True)
    table["missing_msbs"] = [b.kmax - 1 for b in blocks]
    want = chain.decode_tile_oracle(p, blocks, qcd, table, coded)
    got = U.ctx().decode_host(p, table, coded + b"\0" * 16)
    assert np.array_equal(got[0].astype(np.int32), want)


def test_decode_multi_tile_batch():
    tile = synth.g2(3, 256, 256, 8)
    batch = np.ascontiguousarray(np.stack([tile, tile[:, ::-1].copy(), np.roll(tile, 5, axis=2)]))
    p = G.TileParams.make(256, 256, 3, 8, 4)
    table, coded = U.ctx().encode_host(p, batch, ntiles=3)
    back = U.ctx().decode_host(p, table, coded, ntiles=3)
    assert np.array_equal(back, batch)


def test_round_trip_8k_property():
    """BASELINE full size: 8192^2 x 3 encode -> decode on the device returns the source (lossless)."""
    px = synth.g2(3, 8192, 8192, 8)
    p = G.TileParams.make(8192, 8192, 3, 8, 5)
    c = U.ctx()
    d_px = U.to_dev(px.reshape(-1))
    table, tot = c.encode_tiles(p, 1, d_px.data_ptr(), True)
    d_out = U._settled(torch.zeros(px.size, dtype=torch.uint8, device="cuda"))
    c.decode_device(p, 1, table, c.coded_device_ptr(), tot, d_out.data_ptr())
    c.decode_status()
    assert torch.equal(d_out, d_px)


# ---- K8: Part-1 (EBCOT/MQ) block decoder ------------------------------------
import refharness as R

needs_ref = pytest.mark.skipif(not R.have_ref(), reason="oracle/_ref not shipped")


def _part1_tile(px, prec, L):
    """Forward chain on the CPU (oracle RCT + 5/3), every block coded by Grok's own Part-1 T1."""
    C, H, W = px.shape
    p = G.TileParams.make(W, H, C, prec, L, part1=True)
    blocks, _ = G.tile_layout(p)
    planes = [px[c].astype(np.int32) - (1 << (prec - 1)) for c in range(C)]
    if C >= 3:
        planes[:3] = O.rct_fwd(*planes[:3])
    mall = [O.dwt53_fwd(v, L) for v in planes]
    table = np.zeros(len(blocks), G.capi.CODED_DTYPE)
    chunks, off = [], 0
    for i, b in enumerate(blocks):
        bw, bh = b.x1 - b.x0, b.y1 - b.y0
        cb, npass, nbps = R.t1_encode_block(mall[b.comp][b.py:b.py + bh, b.px:b.px + bw], b.band)
        table["offset"][i] = off; table["length"][i] = len(cb); table["missing_msbs"][i] = nbps | (npass << 8)
        chunks.append(cb + b"\0" * (-len(cb) % 16 + 16)); off += len(chunks[-1])
    return p, blocks, mall, table, b"".join(chunks)


@needs_ref
@pytest.mark.parametrize("C,H,W,prec,L,gen", [(1, 128, 128, 8, 3, "g2"), (3, 96, 160, 8, 4, "g2"), (3, 100, 77, 12, 3, "g2"),
                                               (1, 64, 64, 8, 0, "g0"), (3, 256, 256, 8, 5, "g0")])
def test_part1_decode_round_trip(C, H, W, prec, L, gen):
    """Blocks from the reference's EBCOT encoder -> GPU (MQ decode, dequantise, inverse 5/3, inverse RCT)
    == source pixels; the Mallat planes after K8 equal the coefficients that were coded."""
    px = getattr(synth, gen)(C, H, W, prec)
    p, blocks, mall, table, coded = _part1_tile(px, prec, L)
    d_c = U.to_dev(np.frombuffer(coded, np.uint8))
    d_m = U.dev_planes(p, C)
    U.ctx().stage_ht_decode(p, 1, table, d_c.data_ptr(), d_c.numel(), d_m.data_ptr())
    U.ctx().synchronize()
    got = U.planes_to_numpy(d_m, p, C)
    for c in range(C):
        assert np.array_equal(got[c], mall[c]), "component %d" % c
    back = U.ctx().decode_host(p, table, coded)
    assert np.array_equal(back[0], px)


@needs_ref
def test_part1_decode_truncated_passes_equal_oracle():
    """Fewer passes than coded (quality-layer truncation): GPU == oracle == reference T1, block by block."""
    rng = np.random.default_rng(11)
    p = G.TileParams.make(256, 192, 1, 10, 2, part1=True)
    blocks, _ = G.tile_layout(p)
    table = np.zeros(len(blocks), G.capi.CODED_DTYPE)
    chunks, off, want = [], 0, np.zeros((192, 256), np.int32)
    for i, b in enumerate(blocks):
        bw, bh = b.x1 - b.x0, b.y1 - b.y0
        coef = (rng.integers(-400, 400, size=(bh, bw)) >> rng.integers(0, 9, size=(bh, bw))).astype(np.int32)
        cb, npass, nbps = R.t1_encode_block(coef, b.band)
        keep = max(1, npass - int(rng.integers(0, 6)))
        table["offset"][i] = off; table["length"][i] = len(cb); table["missing_msbs"][i] = nbps | (keep << 8)
        chunks.append(cb + b"\0" * (-len(cb) % 16 + 16)); off += len(chunks[-1])
        want[b.py:b.py + bh, b.px:b.px + bw] = O.t1_dequant_rev(O.t1_decode_block(cb, keep, nbps, b.band, bw, bh))
    d_c = U.to_dev(np.frombuffer(b"".join(chunks), np.uint8))
    d_m = U.dev_planes(p, 1)
    U.ctx().stage_ht_decode(p, 1, table, d_c.data_ptr(), d_c.numel(), d_m.data_ptr())
    U.ctx().synchronize()
    assert np.array_equal(U.planes_to_numpy(d_m, p, 1)[0], want)


STYLES = [0x01, 0x02, 0x04, 0x08, 0x10, 0x20, 0x01 | 0x04, 0x02 | 0x08 | 0x20, 0x3F, 0x04 | 0x10]


@needs_ref
@pytest.mark.parametrize("sty", STYLES)
def test_part1_decode_code_block_styles(sty):
    """Row a13's code-block styles: blocks coded by the reference's T1 with LAZY / RESET / TERMALL / VSC / PTERM /
    SEGSYM (and mixes), handed over with their codeword segments, decode on the GPU to what the reference's T1
    and the oracle make of them -- also with trailing segments dropped."""
    rng = np.random.default_rng(100 + sty)
    p = G.TileParams.make(200, 136, 1, 12, 2, part1=True, cblksty=sty)
    blocks, _ = G.tile_layout(p)
    for drop in (0, 1):
        table = np.zeros(len(blocks), G.capi.CODED_DTYPE)
        chunks, off, want, seglist = [], 0, np.zeros((136, 200), np.int32), []
        for i, b in enumerate(blocks):
            bw, bh = b.x1 - b.x0, b.y1 - b.y0
            coef = (rng.integers(-2000, 2000, size=(bh, bw)) >> rng.integers(0, 11, size=(bh, bw))).astype(np.int32)
            cb, segs, nbps = R.t1_encode_block_sty(coef, b.band, sty)
            if drop and len(segs) > 1:
                segs = segs[:max(1, len(segs) - int(rng.integers(1, 4)))]
            n = sum(a for a, _ in segs)
            table["offset"][i] = off; table["length"][i] = n
            table["missing_msbs"][i] = nbps | (sum(k for _, k in segs) << 8)
            seglist.append(segs)
            chunks.append(cb[:n] + b"\0" * (-n % 16 + 16)); off += len(chunks[-1])
            ref = R.t1_decode_block_sty(cb[:n], segs, nbps, b.band, sty, bw, bh) if segs else np.zeros((bh, bw), np.int32)
            if segs:
                assert np.array_equal(O.t1_decode_block_sty(cb[:n], segs, nbps, b.band, sty, bw, bh)[0], ref)
            want[b.py:b.py + bh, b.px:b.px + bw] = O.t1_dequant_rev(ref)
            if not drop:
                assert np.array_equal(want[b.py:b.py + bh, b.px:b.px + bw], coef)
        d_c = U.to_dev(np.frombuffer(b"".join(chunks), np.uint8))
        d_m = U.dev_planes(p, 1)
        U.ctx().set_decode_segments(seglist)
        try:
            U.ctx().stage_ht_decode(p, 1, table, d_c.data_ptr(), d_c.numel(), d_m.data_ptr())
            U.ctx().synchronize()
        finally:
            U.ctx().set_decode_segments(None)
        assert np.array_equal(U.planes_to_numpy(d_m, p, 1)[0], want)


@needs_ref
def test_part1_single_segment_styles_without_segment_list():
    """RESET / VSC / SEGSYM / PTERM keep one codeword segment: the table row alone describes the block (what the
    reference's plugin bridge hands over, plugin_bridge.cpp:63-76)."""
    rng = np.random.default_rng(5)
    sty = 0x02 | 0x08 | 0x10 | 0x20
    p = G.TileParams.make(128, 128, 1, 10, 1, part1=True, cblksty=sty)
    blocks, _ = G.tile_layout(p)
    table = np.zeros(len(blocks), G.capi.CODED_DTYPE)
    chunks, off, want = [], 0, np.zeros((128, 128), np.int32)
    for i, b in enumerate(blocks):
        bw, bh = b.x1 - b.x0, b.y1 - b.y0
        coef = (rng.integers(-500, 500, size=(bh, bw)) >> rng.integers(0, 9, size=(bh, bw))).astype(np.int32)
        cb, segs, nbps = R.t1_encode_block_sty(coef, b.band, sty)
        assert len(segs) == 1
        table["offset"][i] = off; table["length"][i] = len(cb); table["missing_msbs"][i] = nbps | (segs[0][1] << 8)
        chunks.append(cb + b"\0" * (-len(cb) % 16 + 16)); off += len(chunks[-1])
        want[b.py:b.py + bh, b.px:b.px + bw] = coef
    d_c = U.to_dev(np.frombuffer(b"".join(chunks), np.uint8))
    d_m = U.dev_planes(p, 1)
    U.ctx().stage_ht_decode(p, 1, table, d_c.data_ptr(), d_c.numel(), d_m.data_ptr())
    U.ctx().synchronize()
    assert np.array_equal(U.planes_to_numpy(d_m, p, 1)[0], want)


@needs_ref
def test_part1_decode_irreversible_dequant():
    """ScaleFilter path: (float)v * stepsize/2 with the band's step from the QCD words (Quantizer.cpp:41-45,
    decode side: log2_gain 0); the entropy-decoded integers are the same as in the reversible case."""
    rng = np.random.default_rng(21)
    prec, L = 10, 3
    p = G.TileParams.make(192, 128, 1, prec, L, irreversible=True, mct=False, part1=True)
    blocks, qcd = G.tile_layout(p)
    table = np.zeros(len(blocks), G.capi.CODED_DTYPE)
    chunks, off, want = [], 0, np.zeros((128, 192), np.float32)
    for i, b in enumerate(blocks):
        bw, bh = b.x1 - b.x0, b.y1 - b.y0
        coef = (rng.integers(-300, 300, size=(bh, bw)) >> rng.integers(0, 8, size=(bh, bw))).astype(np.int32)
        cb, npass, nbps = R.t1_encode_block(coef, b.band)
        table["offset"][i] = off; table["length"][i] = len(cb); table["missing_msbs"][i] = nbps | (npass << 8)
        chunks.append(cb + b"\0" * (-len(cb) % 16 + 16)); off += len(chunks[-1])
        wq = qcd[chain.band_index(b)]
        step = np.float32((1.0 + (wq & 0x7FF) / 2048.0) * 2.0 ** (prec - (wq >> 11)))
        want[b.py:b.py + bh, b.px:b.px + bw] = O.t1_dequant_irrev(O.t1_decode_block(cb, npass, nbps, b.band, bw, bh), step)
    d_c = U.to_dev(np.frombuffer(b"".join(chunks), np.uint8))
    d_m = U.dev_planes(p, 1)
    U.ctx().stage_ht_decode(p, 1, table, d_c.data_ptr(), d_c.numel(), d_m.data_ptr())
    U.ctx().synchronize()
    assert np.array_equal(U.planes_to_numpy(d_m, p, 1)[0], want.view(np.int32))


# ---- streams of the reference's OWN encoders, through the test-side Tier-2 reader ------------------------
import j2kparse as J


def _gpu_decode_reference_stream(cs, part1):
    info = J.parse(cs)
    p = G.TileParams.make(info["W"], info["H"], info["C"], info["prec"], info["levels"],
                          irreversible=bool(info["irreversible"]), mct=bool(info["mct"]), part1=part1,
                          cblksty=info["cblk_sty"] & 0x3F if part1 else 0, origin=(info["x0"], info["y0"]),
                          precincts=info["prc"] if info["scod"] & 1 else None, cblk=(info["cbw"], info["cbh"]))
    blocks, _ = G.tile_layout(p)
    rows, data = J.decode_table(info, blocks, part1)
    table = np.array(rows, dtype=G.capi.CODED_DTYPE)
    c = U.ctx()
    c.set_decode_qcd([(e << 11) | m for e, m in info["qcd"]] if info["irreversible"] else [])
    if part1 and info["cblk_sty"] & 0x05:                      # LAZY / TERMALL: several codeword segments per block
        c.set_decode_segments(J.segment_list(info, blocks))
    try:
        return c.decode_host(p, table, data)[0]
    finally:
        c.set_decode_qcd([])
        c.set_decode_segments(None)


@needs_ref
@pytest.mark.parametrize("C,H,W,prec,numres", [(3, 96, 160, 8, 5), (1, 128, 128, 8, 4), (3, 256, 256, 12, 6), (3, 100, 77, 8, 3)])
@pytest.mark.parametrize("ht", [1, 0])
def test_decode_reference_lossless_stream(C, H, W, prec, numres, ht):
    """grk_compress output (HT and Part-1, RCT + 5/3) decoded on the GPU == the source == grk_decompress."""
    px = synth.g2(C, H, W, prec)
    cs, _ = R.encode(px, prec, numres=numres, mode=1, ht=ht)
    got = _gpu_decode_reference_stream(cs, part1=not ht)
    assert np.array_equal(got, px)
    assert np.array_equal(got.astype(np.int32), R.decode(cs, C, H, W))


@needs_ref
@pytest.mark.parametrize("C,H,W,prec,numres", [(3, 96, 160, 8, 5), (1, 128, 128, 8, 4), (3, 256, 256, 12, 6), (3, 100, 77, 8, 3)])
def test_decode_reference_part1_irreversible_stream(C, H, W, prec, numres):
    """BASELINE configs[4] shape: Part-1 EBCOT + ICT + 9/7 coded by the reference, decoded on the GPU (MQ decode,
    ScaleFilter, inverse 9/7, inverse ICT) == grk_decompress pixel for pixel; and close to the source."""
    px = synth.g2(C, H, W, prec)
    cs, _ = R.encode(px, prec, numres=numres, mode=1, ht=0, irrev=1)
    got = _gpu_decode_reference_stream(cs, part1=True).astype(np.int32)
    ref = R.decode(cs, C, H, W)
    if C == 3:      # (without MCT the reference's irreversible encoder scales by 2048, TileProcessor.cpp:928-931: not a usable source)
        assert np.abs(ref - px.astype(np.int32)).max() <= max(2, (1 << prec) // 64)
    assert np.array_equal(got, ref)


@needs_ref
@pytest.mark.parametrize("sty", [0x01, 0x02, 0x04, 0x08, 0x20, 0x01 | 0x04, 0x3F])
@pytest.mark.parametrize("irrev", [0, 1])
def test_decode_reference_part1_styled_stream(sty, irrev):
    """`grk_compress -M sty` streams (code-block styles, codeword segments through Tier-2) decoded on the GPU ==
    grk_decompress pixel for pixel."""
    px = synth.g2(3, 128, 192, 10)
    cs, _ = R.encode(px, 10, numres=4, mode=1, ht=0, irrev=irrev, cblksty=sty)
    got = _gpu_decode_reference_stream(cs, part1=True).astype(np.int32)
    assert np.array_equal(got, R.decode(cs, 3, 128, 192))
    if not irrev:
        assert np.array_equal(got, px.astype(np.int32))


@pytest.mark.parametrize("C,H,W,prec,L", [(1, 96, 128, 8, 3), (3, 128, 160, 8, 4), (3, 64, 96, 12, 2)])
def test_signed_samples_round_trip_and_blocks(C, H, W, prec, L):
    """Signed input (int8/int16 samples, DC shift 0): GPU blocks == oracle chain's, GPU decode returns the source."""
    u = synth.g2(C, H, W, prec).astype(np.int32)
    px = (u - (1 << (prec - 1))).astype(np.int8 if prec <= 8 else np.int16)
    p, blocks, qcd, otable, ocoded = chain.encode_tile_oracle(px, prec, L, sgnd=True)
    table, coded = U.ctx().encode_host(p, px)
    got = U.split_blocks(table, coded)
    want = [bytes(ocoded[int(o):int(o) + int(l)]) for o, l in zip(otable["offset"], otable["length"])]
    assert got == want
    back = U.ctx().decode_host(p, table, coded)[0]
    assert np.array_equal(back.view(px.dtype), px)


# ---- region (windowed) decode: SURVEY.md §8f N4 ---------------------------------------------------------------
WINDOWS = [(0, 0, 64, 64), (100, 37, 227, 201), (1, 1, 2, 2), (0, 0, None, None), (333, 250, None, None), (65, 130, 66, 400),
           (2, 0, 700, 9), (511, 301, 513, 303)]


@pytest.mark.parametrize("C,H,W,prec,L,irrev", [(3, 512, 768, 8, 5, False), (1, 517, 700, 12, 3, False), (3, 512, 768, 10, 4, True),
                                                (3, 600, 1100, 8, 1, False)])
def test_region_decode_equals_crop_of_full_decode(C, H, W, prec, L, irrev):
    """grk_amd_decode_region == the same crop of grk_amd_decode_tiles, bit for bit (5/3 and 9/7), for windows at the
    corners, across strip / segment / code-block boundaries, one pixel wide, and the whole tile -- although only the
    blocks and the parts of each DWT level the window depends on are computed (what grk_decompress_set_window does
    on the host, whose windowed output equals the crop of its full output as well: tests/test_oracle_decode.py)."""
    px = synth.g2(C, H, W, prec)
    p = G.TileParams.make(W, H, C, prec, L, irreversible=irrev)
    table, coded = U.ctx().encode_host(p, px)
    full = U.ctx().decode_host(p, table, coded)[0]
    if not irrev:
        assert np.array_equal(full, px)
    for (x0, y0, x1, y1) in WINDOWS:
        x1 = W if x1 is None else min(x1, W); y1 = H if y1 is None else min(y1, H)
        if x0 >= x1 or y0 >= y1:
            continue
        # poison the planes the previous call left behind: whatever the window does not depend on must not leak in
        try:
            U.ctx().decode_host(p, table, _scrambled(table, coded))
        except Exception:
            pass                                  # (a scrambled block may be rejected; the planes are dirty either way)
        got = U.ctx().decode_region_host(p, table, coded, x0, y0, x1, y1)
        assert np.array_equal(got, full[:, y0:y1, x0:x1]), (x0, y0, x1, y1)


def _scrambled(table, coded):
    """The same blocks with their payload bit-flipped in the middle: decodes to different (garbage) coefficients."""
    c = np.frombuffer(coded, np.uint8).copy()
    for o, l in zip(table["offset"], table["length"]):
        if l > 8:
            c[int(o) + 1:int(o) + int(l) // 2] ^= 0x55
    return c


@needs_ref
@pytest.mark.parametrize("ht,irrev", [(1, 0), (0, 0), (0, 1)])
def test_region_decode_of_reference_stream_equals_reference_window(ht, irrev):
    """A grk_compress stream (HT, classic, classic ICT + 9/7): our windowed decode == grk_decompress with
    grk_decompress_set_window on the same window."""
    px = synth.g2(3, 384, 512, 8)
    cs, _ = R.encode(px, 8, numres=5, mode=1, ht=ht, irrev=irrev)
    info = J.parse(cs)
    p = G.TileParams.make(512, 384, 3, 8, 4, irreversible=bool(irrev), mct=True, part1=not ht)
    blocks, _ = G.tile_layout(p)
    rows, data = J.decode_table(info, blocks, not ht)
    table = np.array(rows, dtype=G.capi.CODED_DTYPE)
    c = U.ctx()
    c.set_decode_qcd([(e << 11) | m for e, m in info["qcd"]] if irrev else [])
    try:
        for (x0, y0, x1, y1) in ((0, 0, 100, 100), (131, 77, 390, 300), (500, 380, 512, 384)):
            got = c.decode_region_host(p, table, data, x0, y0, x1, y1).astype(np.int32)
            assert np.array_equal(got, R.decode_window(cs, 3, x0, y0, x1, y1)), (x0, y0, x1, y1)
    finally:
        c.set_decode_qcd([])


def _random_streams(n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        C = int(rng.choice([1, 3]))
        W, H = int(rng.integers(33, 520)), int(rng.integers(33, 400))
        prec = int(rng.choice([8, 10, 12]))
        numres = int(rng.integers(1, 6))
        ht = int(rng.integers(0, 2))
        irrev = 0 if ht else int(rng.integers(0, 2))            # (the reference's HT + 9/7 encoder is broken: D1)
        if irrev and C == 1:
            irrev = 0                                           # (irreversible without MCT: scaled by 2048, D1)
        sty = 0 if ht else int(rng.choice([0, 0, 0x01, 0x02, 0x04, 0x08, 0x20, 0x05, 0x2A, 0x3F]))
        out.append((C, H, W, prec, numres, ht, irrev, sty))
    return out


@needs_ref
@pytest.mark.parametrize("C,H,W,prec,numres,ht,irrev,sty", _random_streams(20, 11))
def test_random_reference_streams_full_and_windowed(C, H, W, prec, numres, ht, irrev, sty):
    """A seeded sweep over grk_compress streams -- HT / classic, 5/3 and ICT + 9/7, every code-block style, odd sizes,
    1..5 resolutions: the GPU decode of the blocks Tier-2 hands over == grk_decompress, and two random windows == the
    crop of it == grk_decompress_set_window (except where the reference's own windowed decode is broken, D12)."""
    px = synth.g2(C, H, W, prec)
    cs, _ = R.encode(px, prec, numres=numres, mode=1, ht=ht, irrev=irrev, cblksty=sty)
    info = J.parse(cs)
    part1 = not ht
    p = G.TileParams.make(W, H, C, prec, info["levels"], irreversible=bool(irrev), mct=bool(info["mct"]), part1=part1,
                          cblksty=info["cblk_sty"] & 0x3F if part1 else 0)
    blocks, _ = G.tile_layout(p)
    rows, data = J.decode_table(info, blocks, part1)
    table = np.array(rows, dtype=G.capi.CODED_DTYPE)
    c = U.ctx()
    c.set_decode_qcd([(e << 11) | m for e, m in info["qcd"]] if irrev else [])
    if part1 and info["cblk_sty"] & 0x05:
        c.set_decode_segments(J.segment_list(info, blocks))
    try:
        full = c.decode_host(p, table, data)[0].astype(np.int32)
        assert np.array_equal(full, R.decode(cs, C, H, W))
        rng = np.random.default_rng(W * 7 + H)
        if info["levels"] >= 1:
            for _ in range(2):
                x0, y0 = int(rng.integers(0, W - 1)), int(rng.integers(0, H - 1))
                x1, y1 = int(rng.integers(x0 + 1, W + 1)), int(rng.integers(y0 + 1, H + 1))
                got = c.decode_region_host(p, table, data, x0, y0, x1, y1).astype(np.int32)
                crop = full[:, y0:y1, x0:x1]
                assert np.array_equal(got, crop), (x0, y0, x1, y1)
                refw = R.decode_window(cs, C, x0, y0, x1, y1)
                if not np.array_equal(refw, crop):
                    # reference defect D12: for some narrow windows grk_decompress_set_window returns an undecoded
                    # (mid-grey) area instead of the crop of its own full decode; nothing to be compatible with
                    assert np.all(refw == refw.flat[0]), "reference window differs from its own full decode in an unexpected way"
    finally:
        c.set_decode_qcd([])
        c.set_decode_segments(None)


# ---- corrupt input (the reference fuzzes its decoder, tests/fuzzers/grk_decompress_fuzzer.cpp; one corrupt-HT case in
#      its regression suite): garbage must be rejected or decoded to garbage, never fault, hang or poison later calls
@pytest.mark.parametrize("part1", [False, True])
def test_corrupt_streams_do_not_fault(part1):
    rng = np.random.default_rng(99 + part1)
    px = synth.g2(3, 192, 256, 8)
    if part1:
        if not R.have_ref():
            pytest.skip("oracle/_ref not shipped")
        p, blocks, mall, table, coded = _part1_tile(px, 8, 3)
    else:
        p = G.TileParams.make(256, 192, 3, 8, 3)
        table, coded = U.ctx().encode_host(p, px)
    good = np.frombuffer(coded, np.uint8).copy()
    c = U.ctx()
    for trial in range(12):
        bad = good.copy()
        t = table.copy()
        kind = trial % 4
        if kind == 0:                                    # random bytes everywhere
            bad[:] = rng.integers(0, 256, size=bad.size, dtype=np.uint8)
        elif kind == 1:                                  # a few flipped bits per block
            for o, l in zip(t["offset"], t["length"]):
                for _ in range(3):
                    if l:
                        bad[int(o) + int(rng.integers(0, l))] ^= 1 << int(rng.integers(0, 8))
        elif kind == 2:                                  # truncated blocks
            t["length"] = (t["length"] * rng.random(len(t))).astype(np.uint32)
        else:                                            # wrong side information
            if part1:
                t["missing_msbs"] = (rng.integers(0, 30, size=len(t)) | (rng.integers(0, 60, size=len(t)) << 8)).astype(np.uint32)
            else:
                t["missing_msbs"] = rng.integers(0, 40, size=len(t)).astype(np.uint32)
        try:
            c.decode_host(p, t, bad)
        except RuntimeError:
            pass
    # rows pointing outside the buffer are refused on the host
    t = table.copy(); t["offset"][len(t) // 2] = good.size + 5
    with pytest.raises(RuntimeError):
        c.decode_host(p, t, good)
    t = table.copy(); t["length"][0] = good.size + 1
    with pytest.raises(RuntimeError):
        c.decode_host(p, t, good)
    # and the context still decodes the intact stream
    back = c.decode_host(p, table, good)[0]
    assert np.array_equal(back, px)


@pytest.mark.parametrize("C,H,W,prec,L,irrev", [(3, 200, 333, 8, 3, False), (3, 256, 256, 12, 5, True), (1, 129, 65, 10, 2, False),
                                                (4, 128, 192, 8, 2, False)])
def test_fused_last_level_equals_separate_egress(C, H, W, prec, L, irrev, monkeypatch):
    """K7 inside the last inverse DWT level (default) == inverse DWT to int32 planes + the stand-alone egress kernel
    (GRK_AMD_FUSE_EGRESS=0), for the MCT triple, extra components, odd sizes, 5/3 and 9/7."""
    px = synth.g2(C, H, W, prec)
    p = G.TileParams.make(W, H, C, prec, L, irreversible=irrev)
    table, coded = U.ctx().encode_host(p, px)
    out = {}
    for fuse in ("1", "0"):
        monkeypatch.setenv("GRK_AMD_FUSE_EGRESS", fuse)
        c = G.Context(0)
        out[fuse] = c.decode_host(p, table, coded)[0]
        c.close()
    assert np.array_equal(out["1"], out["0"])
    if not irrev:
        assert np.array_equal(out["1"], px)


def test_decode_int16_planes_and_their_range_check():
    """8-bit reversible HT tiles are decoded with int16 planes between K5b and K6 (default).  Same pixels as with int32
    planes on ordinary and on extreme (0 / 255 checkerboard) content; a stream whose values do NOT fit -- here the blocks of
    a 16-bit checkerboard decoded as if they belonged to an 8-bit tile -- is never decoded to other pixels: the
    synchronous call repeats itself with int32 planes, the asynchronous one reports it."""
    c = U.ctx()
    H, W, L = 256, 320, 5
    yy, xx = np.mgrid[0:H, 0:W]
    # (a 0 / 255 checkerboard itself is rejected by both decoders, defect D5; so is one with different phases per channel: the RCT doubles it)
    for px in (synth.g2(3, H, W, 8), np.stack([((yy + xx) & 1) * 150 + 50 for k in range(3)]).astype(np.uint8)):
        p = G.TileParams.make(W, H, 3, 8, L)
        table, coded = c.encode_host(p, px)
        a = c.decode_host(p, table, coded)[0]
        c.set_decode_planes16(False)
        try:
            b = c.decode_host(p, table, coded)[0]
        finally:
            c.set_decode_planes16(True)
        assert np.array_equal(a, px) and np.array_equal(b, px)
    # out of range for int16: the blocks of a 16-bit half-scale checkerboard under 8-bit parameters
    px12 = (((yy + xx) & 1) * 30000 + 10000).astype(np.uint16)[None]
    p12 = G.TileParams.make(W, H, 1, 16, L)
    table, coded = c.encode_host(p12, px12)
    p8 = G.TileParams.make(W, H, 1, 8, L)
    c.set_decode_planes16(False)
    try:
        want = c.decode_host(p8, table, coded)[0]
    finally:
        c.set_decode_planes16(True)
    got = c.decode_host(p8, table, coded)[0]                # int16 planes -> range flag -> repeated with int32 planes
    assert np.array_equal(got, want)
    # in between: values that fit int16 but not the packed inverse transform's range (+-2047, pk16.h) -- coefficients beyond it
    # (flagged by the block decoder), or coefficients inside it whose synthesis grows past it (flagged by the level that
    # writes such an LL): smooth ramps, noise and checkerboards of rising amplitude, all the same pixels as with int32 planes
    rng = np.random.default_rng(5)
    for amp in (300, 700, 1500, 4000, 9000):
        for kind in range(3):
            if kind == 0: v = (yy * amp // H + xx * amp // W) // 2
            elif kind == 1: v = rng.integers(0, amp, size=(H, W))
            else: v = (((yy // 4) + (xx // 4)) & 1) * amp
            pxa = (v + 32768 - amp // 2).astype(np.uint16)[None]
            table, coded = c.encode_host(p12, pxa)
            c.set_decode_planes16(False)
            try:
                want_a = c.decode_host(p8, table, coded)[0]
            finally:
                c.set_decode_planes16(True)
            assert np.array_equal(c.decode_host(p8, table, coded)[0], want_a), (amp, kind)
    table, coded = c.encode_host(p12, px12)
    d_c = U.to_dev(np.concatenate([coded, np.zeros(64, np.uint8)]))
    out = U._settled(torch.zeros(H * W, dtype=torch.uint8, device="cuda"))
    c.decode_device(p8, 1, table, d_c.data_ptr(), coded.size, out.data_ptr())
    with pytest.raises(RuntimeError, match="16-bit planes"):
        c.decode_status()
    c.set_decode_planes16(False)
    try:
        c.decode_device(p8, 1, table, d_c.data_ptr(), coded.size, out.data_ptr())
        c.decode_status()
    finally:
        c.set_decode_planes16(True)
    assert np.array_equal(out.cpu().numpy().reshape(1, H, W), want)


def test_mixed_packed_and_unpacked_inverse_levels_keep_the_packed_range():
    """a 1024 x 1024 tile with 6 levels runs its inverse levels 5, 4 and 3 (32 .. 128 columns) through the generic
    int16 kernel and levels 2 .. 0 through the packed one, whose sums need inputs inside +-2047.  Coefficients all inside that
    range (the block decoder raises nothing; 2^(Kmax - 2), the largest magnitude both decoders accept everywhere, in every band
    of the five coarsest resolutions) whose synthesis grows past it -- the 128 x 128 LL reaches 2560 -- used to pass the generic
    level's "fits int16" check.  Now the level that writes such an LL raises the range flag: the synchronous decode repeats
    itself with int32 planes (same pixels as with int32 planes from the start, and as the oracle's inverse chain), the
    asynchronous one reports GRK_AMD_ERR_RANGE."""
    W = H = 1024
    L = 6
    p = G.TileParams.make(W, H, 1, 8, L)
    blocks, _ = G.tile_layout(p)
    planes = np.zeros((1, H, W), np.int32)
    for b in blocks:
        if b.res <= L - 2:
            planes[0, b.py:b.py + (b.y1 - b.y0), b.px:b.px + (b.x1 - b.x0)] = 1 << (b.kmax - 2)
    assert np.abs(planes).max() <= 2047 and np.abs(O.dwt53_inv(planes[0, :128, :128].copy(), L - 3)).max() > 2047
    c = U.ctx()
    d_m = U.upload_planes(planes, p)
    c.stage_ht_encode(p, 1, d_m.data_ptr())
    table, tot = c.fetch_table(len(blocks))
    coded = c.fetch_coded(tot)
    c.set_decode_planes16(False)
    try:
        want = c.decode_host(p, table, coded)[0]
    finally:
        c.set_decode_planes16(True)
    px = np.clip(O.dwt53_inv(planes[0], L) + 128, 0, 255).astype(np.uint8)
    assert np.array_equal(want[0], px)
    assert np.array_equal(c.decode_host(p, table, coded)[0], want)
    d_c = U.to_dev(np.concatenate([coded, np.zeros(64, np.uint8)]))
    out = U._settled(torch.zeros(H * W, dtype=torch.uint8, device="cuda"))
    c.decode_device(p, 1, table, d_c.data_ptr(), coded.size, out.data_ptr())
    with pytest.raises(RuntimeError, match="16-bit planes"):
        c.decode_status()


def test_tile_without_any_coded_block_decodes_to_the_dc_level():
    """Every row of the table empty (length 0): no K5p wave and no K5a lane has anything to do, K5b still writes the zeros the
    inverse transform reads -- stale coefficients of the call before must not come back."""
    p = G.TileParams.make(192, 128, 3, 8, 3)
    c = U.ctx()
    px = synth.g2(3, 128, 192, 8)
    table, coded = c.encode_host(p, px)
    assert np.array_equal(c.decode_host(p, table, coded)[0], px)      # (leaves its coefficients in the planes)
    empty = table.copy()
    empty["length"] = 0; empty["offset"] = 0
    back = c.decode_host(p, empty, coded)
    assert np.all(back[0] == 128)


def test_decode_with_and_without_the_side_stream_and_tables_of_consecutive_calls():
    """K5b of the top resolution on the side stream (overlap on) == everything on one stream; consecutive calls on the device with
    DIFFERENT tables -- each call's pinned table set is refilled while the call before may still be queued -- keep their own."""
    import torch
    p = G.TileParams.make(512, 384, 3, 8, 4)
    c = G.Context(0)
    imgs = [synth.g2(3, 384, 512, 8, seed=s) for s in (3, 4, 5)]
    enc = [c.encode_host(p, im) for im in imgs]
    tot = sum(len(cd) + 64 for _, cd in enc)
    blob = np.zeros(tot, np.uint8)
    tabs, at = [], 0
    for t, cd in enc:
        blob[at:at + len(cd)] = np.frombuffer(cd, np.uint8)
        t2 = t.copy(); t2["offset"] += at
        tabs.append(t2); at += len(cd) + 64
    d_c = torch.from_numpy(blob).cuda()
    outs = [torch.empty(imgs[0].size, dtype=torch.uint8, device="cuda") for _ in range(6)]
    for ov in (True, False):
        c.set_overlap(ov)
        for rep in range(2):
            for i in range(3):
                c.decode_device(p, 1, tabs[i], d_c.data_ptr(), d_c.numel(), outs[3 * rep + i].data_ptr())
        c.decode_status()
        torch.cuda.synchronize()
        for k in range(6):
            assert np.array_equal(outs[k].cpu().numpy().reshape(imgs[0].shape), imgs[k % 3]), (ov, k)
            outs[k].zero_()


def test_decode_sequence_mode_frames_in_flight():
    """grk_amd_set_decode_pipelining(ctx, 3): consecutive decode calls on three internal buffer / stream sets in turn.  Every frame of a
    sequence of DIFFERENT frames comes out as the one-at-a-time decode gives it; a corrupt frame in the middle is reported by
    grk_amd_decode_status whichever set decoded it; switching the mode off again leaves a context that works as before."""
    C, H, W, prec, L = 3, 256, 384, 8, 4
    p = G.TileParams.make(W, H, C, prec, L)
    c = G.Context(0)
    frames = []
    for f in range(7):
        px = synth.g2(C, H, W, prec, seed=100 + f)
        table, coded = c.encode_host(p, px)
        frames.append((px, table, U.to_dev(np.frombuffer(bytes(coded), np.uint8).copy())))
    c.set_decode_pipelining(3)
    try:
        outs = [torch.zeros(C * H * W, dtype=torch.uint8, device="cuda") for _ in frames]
        torch.cuda.synchronize()                              # (torch's fills have landed before the context's streams write)
        for rep in range(2):                                  # (twice: every set has decoded, then decodes again)
            for (px, table, d_c), o in zip(frames, outs):
                c.decode_device(p, 1, table, d_c.data_ptr(), d_c.numel(), o.data_ptr())
        c.synchronize()
        c.decode_status()
        for (px, _, _), o in zip(frames, outs):
            assert np.array_equal(o.cpu().numpy().reshape(C, H, W), px)
        # a frame with a corrupt block, decoded by one of the other sets
        px, table, d_c = frames[1]
        bad = d_c.clone()
        i = int(np.argmax(table["length"]))
        off, ln = int(table["offset"][i]), int(table["length"][i])
        bad[off + ln - 1] = 0xFF; bad[off + ln - 2] |= 0x0F         # Scup > Lcup
        c.decode_device(p, 1, frames[0][1], frames[0][2].data_ptr(), frames[0][2].numel(), outs[0].data_ptr())
        c.decode_device(p, 1, table, bad.data_ptr(), bad.numel(), outs[1].data_ptr())
        c.decode_device(p, 1, frames[2][1], frames[2][2].data_ptr(), frames[2][2].numel(), outs[2].data_ptr())
        with pytest.raises(RuntimeError):
            c.decode_status()
    finally:
        c.set_decode_pipelining(0)
    o = torch.zeros(C * H * W, dtype=torch.uint8, device="cuda")
    c.decode_device(p, 1, frames[3][1], frames[3][2].data_ptr(), frames[3][2].numel(), o.data_ptr())
    c.synchronize()
    assert np.array_equal(o.cpu().numpy().reshape(C, H, W), frames[3][0])


def test_decode_sequence_on_a_context_that_did_nothing_else():
    """A context whose FIRST use is a sequence (frames in flight set before any encode / decode on the context itself): every frame
    runs on the internal sets, and grk_amd_decode_status has nothing of the context's own to fetch -- it reports the sets' status
    (r04: it failed with "fetch status: invalid argument")."""
    C, H, W, prec, L = 3, 128, 192, 8, 3
    p = G.TileParams.make(W, H, C, prec, L)
    enc = G.Context(0)
    px = synth.g2(C, H, W, prec, seed=5)
    table, coded = enc.encode_host(p, px)
    d_c = U.to_dev(np.frombuffer(bytes(coded), np.uint8).copy())
    c = G.Context(0)
    c.set_decode_pipelining(3)
    try:
        outs = [torch.zeros(C * H * W, dtype=torch.uint8, device="cuda") for _ in range(4)]
        torch.cuda.synchronize()
        for o in outs:
            c.decode_device(p, 1, table, d_c.data_ptr(), d_c.numel(), o.data_ptr())
        c.synchronize()
        c.decode_status()
        for o in outs:
            assert np.array_equal(o.cpu().numpy().reshape(C, H, W), px)
    finally:
        c.set_decode_pipelining(0)


@needs_ref
def test_decode_sequence_that_changes_its_kind_of_frames():
    """HT frames, then Part-1 frames, then HT frames again through ONE sequence (three in flight): the internal contexts re-make
    their streams when the kind of frame changes (Part-1: over both priority levels' hardware-queue pools; HT: plain streams) --
    every frame comes out as its source whichever streams decoded it, and the status stays clean."""
    C, H, W, prec, L = 3, 128, 192, 8, 3
    p_ht = G.TileParams.make(W, H, C, prec, L)
    enc = G.Context(0)
    ht = []
    for f in range(4):
        px = synth.g2(C, H, W, prec, seed=40 + f)
        table, coded = enc.encode_host(p_ht, px)
        ht.append((px, table, U.to_dev(np.frombuffer(bytes(coded), np.uint8).copy())))
    p1 = []
    for f in range(4):
        px = synth.g2(C, H, W, prec, seed=60 + f)
        p, _, _, table, coded = _part1_tile(px, prec, L)
        p1.append((px, table, U.to_dev(np.frombuffer(coded, np.uint8).copy()), p))
    c = G.Context(0)
    c.set_decode_pipelining(3)
    try:
        outs = []
        for rnd in range(2):                                  # HT, Part-1, HT, Part-1: two changes each way
            for kind in ("ht", "p1"):
                for fr in (ht if kind == "ht" else p1):
                    o = U._settled(torch.zeros(C * H * W, dtype=torch.uint8, device="cuda"))     # (the fill has landed)
                    c.decode_device(fr[3] if kind == "p1" else p_ht, 1, fr[1], fr[2].data_ptr(), fr[2].numel(), o.data_ptr())
                    outs.append((o, fr[0]))
        c.synchronize()
        c.decode_status()
        for i, (o, px) in enumerate(outs):
            assert np.array_equal(o.cpu().numpy().reshape(C, H, W), px), "frame %d" % i
    finally:
        c.set_decode_pipelining(0)


def test_decode_sequence_reuses_two_buffers_behind_the_slot_event():
    """Buffer lifetime in a sequence (include/grok_amd.h): TWO coded and TWO pixel buffers for two frames in flight, every frame's
    coded bytes copied into its buffer on a stream of the caller's that first waits for the set's last frame
    (grk_amd_decode_stream_wait_slot) -- ten different frames come out right, and the pixels of frame f are read on that stream
    behind the same wait, without a host synchronisation in between."""
    C, H, W, prec, L = 3, 256, 384, 8, 4
    p = G.TileParams.make(W, H, C, prec, L)
    c = G.Context(0)
    frames = []
    for f in range(10):
        px = synth.g2(C, H, W, prec, seed=500 + f)
        table, coded = c.encode_host(p, px)
        frames.append((px, table, U.to_dev(np.frombuffer(bytes(coded), np.uint8).copy())))
    cap = max(int(d.numel()) for _, _, d in frames)
    n = 2
    cbuf = [torch.zeros(cap, dtype=torch.uint8, device="cuda") for _ in range(n)]
    obuf = [torch.zeros(C * H * W, dtype=torch.uint8, device="cuda") for _ in range(n)]
    kept = [torch.zeros(C * H * W, dtype=torch.uint8, device="cuda") for _ in frames]
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    c.set_stream(st.cuda_stream)                                  # the caller's uploads and the calls share this stream
    c.set_decode_pipelining(n)
    try:
        with torch.cuda.stream(st):
            for f, (px, table, d_c) in enumerate(frames):
                c.decode_stream_wait_slot(st.cuda_stream)         # the set of frame f - n is done with cbuf / obuf [f % n]
                if f >= n:
                    kept[f - n].copy_(obuf[f % n], non_blocking=True)     # ... so its pixels can be taken
                cbuf[f % n][:d_c.numel()].copy_(d_c, non_blocking=True)   # ... and its coded buffer overwritten
                c.decode_device(p, 1, table, cbuf[f % n].data_ptr(), d_c.numel(), obuf[f % n].data_ptr())
        c.synchronize()
        c.decode_status()
        torch.cuda.synchronize()
        for f in range(len(frames) - n, len(frames)):
            kept[f].copy_(obuf[f % n])
        torch.cuda.synchronize()
        for f, (px, _, _) in enumerate(frames):
            assert np.array_equal(kept[f].cpu().numpy().reshape(C, H, W), px), f
    finally:
        c.set_decode_pipelining(0)
        c.set_stream(0)
