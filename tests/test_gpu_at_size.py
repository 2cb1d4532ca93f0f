"""-m gpu: the BASELINE configurations at their full sizes.

cfg3  8192x8192x3 16-bit, ICT + 9/7 + dead-zone quantiser + HT: the GPU's sub-band coefficients == the oracle's
      (and the real reference's dwt97) to the bit -- north_star asks for <= 1 ULP --, and sampled code-blocks ==
      the oracle chain's bytes.  This is the only place the 9/7 kernel runs with the row-segment sizes the
      8K launch heuristic picks (encode.hip run_dwt: seg >= 16 needs >= 4K images).
cfg4  a 64-tile batch (8192x8192 cut into 1024x1024 tiles, every tile different content): whole codestream ==
      grk_compress's, byte for byte; the batch decode returns the source.  And the configuration itself: 16384x16384 as 256
      tiles on one GPU == grk_compress's file (the N = 1 point of its scaling curve).
cfg5  8192x8192x3 12-bit Part-1 (EBCOT/MQ) + ICT + 9/7 stream written by the reference's encoder, decoded on the
      GPU == grk_decompress, pixel for pixel.
"""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest
import torch

import grok_amd as G
import oracle as O
import chain
import synth
import gpuutil as U
import refharness as R
import j2kparse as J

pytestmark = pytest.mark.gpu
needs_ref = pytest.mark.skipif(not R.have_ref(), reason="oracle/_ref (the real reference) not shipped")


def _dev_view(ptr, n, typestr):
    class _H:
        pass
    h = _H()
    h.__cuda_array_interface__ = {"shape": (int(n),), "typestr": typestr, "data": (int(ptr), False), "version": 2}
    return torch.as_tensor(h, device="cuda")


def test_cfg3_8k_16bit_ict_dwt97_coefficients_and_blocks():
    W = H = 8192
    prec, L, Cn = 16, 5, 3
    px = synth.g2(Cn, H, W, prec)
    p = G.TileParams.make(W, H, Cn, prec, L, irreversible=True)
    c = U.ctx()
    table, coded = c.encode_host(p, px)
    stride = G.lib().grk_amd_plane_stride(p)
    # the Mallat planes the encode left on the device (float32 bit patterns; irreversible content never uses int16 planes)
    mall_gpu = _dev_view(c.plane_device_ptr(1), Cn * H * stride, "<i4").cpu().numpy().reshape(Cn, H, stride)[:, :, :W]
    planes = [px[k].astype(np.int32) - (1 << (prec - 1)) for k in range(Cn)]
    ycc = O.ict_fwd(*planes)
    del planes
    mall = []
    for k in range(Cn):
        want = O.dwt97_fwd(ycc[k], L)
        diff = mall_gpu[k] != want.view(np.int32)
        assert not diff.any(), "component %d: %d coefficients differ from the oracle, max |ulp| %d" % (
            k, int(diff.sum()), int(np.abs(mall_gpu[k].astype(np.int64) - want.view(np.int32)).max()))
        mall.append(want)
    if R.have_ref():       # the real reference's 9/7 (WaveletFwd.cpp:911-994) on one component, live
        ref = np.ascontiguousarray(ycc[1]).copy()
        R.lib().ref_dwt97_fwd(ref.ctypes.data, W, H, W, L)
        assert np.array_equal(ref.view(np.int32), mall_gpu[1]), "GPU 9/7 coefficients differ from grk::dwt97"
    # EVERY block (cfg3 has no reference bytes to match, reference defect D1: the oracle chain is the only check there is):
    # quantiser + HT cleanup bytes == the oracle chain's
    blocks, _ = G.tile_layout(p)
    got = U.split_blocks(table, coded)
    assert len(blocks) == 49152
    OL = O.lib()
    bad = []
    for i in range(len(blocks)):
        b = blocks[i]
        bw, bh = b.x1 - b.x0, b.y1 - b.y0
        sub = np.ascontiguousarray(mall[b.comp][b.py:b.py + bh, b.px:b.px + bw])
        sm = np.zeros((bh, bw), np.uint32)
        OL.orc_ht_signmag_irrev(sub.ctypes.data, bw, bw, bh, b.kmax, C.c_float(np.float32(1.0) / np.float32(b.stepsize)),
                                sm.ctypes.data)
        if got[i] != O.ht_encode_sm(sm, b.kmax):
            bad.append(i)
    assert not bad, "blocks differing from the oracle chain: %s" % bad[:10]
    del mall, ycc, mall_gpu
    # The last link: a GPU-made 16-bit cfg3 codestream through the REFERENCE's decoder (grk_decompress,
    # T1HT.cpp:129-179 + ScaleHTFilter PostDecompressFilters.h:60-71 + inverse 9/7 + inverse ICT): close to the source within the
    # bound tests/test_oracle_decode.py pins the oracle chain with at this bit depth, and the GPU's own decode of the same
    # stream (K5 -> dequantisation -> K6 -> K7 at 16 bits, 8192 x 8192) returns the reference decoder's pixels exactly.
    # Content: G2 clipped into the middle of the range -- the reference's decoder refuses plain G2's darkest LL block (defect D5,
    # synth.g2_mid), and so, mirroring it, does ours.
    if R.have_ref():
        with pytest.raises(RuntimeError):
            c.decode_host(p, table, coded)                 # (plain G2: the D5 check of the reference's decoder, mirrored)
        R.lib(threads=os.cpu_count() or 1)
        px = synth.g2_mid(Cn, H, W, prec)
        table, coded = c.encode_host(p, px)
        cs = G.write_codestream(p, W, H, table, coded)
        ref = R.decode(cs, Cn, H, W)
        err = int(np.abs(ref.astype(np.int64) - px.astype(np.int64)).max())
        psnr = synth.psnr_db(ref, px, prec)
        assert err <= 8 and psnr >= 90.0, (err, psnr)
        back = c.decode_host(p, table, coded)[0].astype(np.int32)
        assert np.array_equal(back, ref), "GPU decode of the cfg3 stream differs from grk_decompress at %d samples" % int((back != ref).sum())


@needs_ref
@pytest.mark.parametrize("Cn,H,W,L,gen", [(3, 256, 256, 5, "g2"), (1, 200, 333, 3, "g2_mid"), (3, 1024, 1024, 5, "g2_mid"), (3, 1536, 640, 4, "g2_mid")])
def test_cfg3_bit_depth_small_gpu_stream_through_reference_decoder(Cn, H, W, L, gen):
    """16-bit ICT + 9/7 + quantiser + HT at a size the whole oracle chain runs at: the GPU's codestream -> grk_decompress ==
    the oracle's decode chain of the GPU's blocks == the GPU's decode, and all of them within 8 / 65 536 of the source."""
    prec = 16
    px = getattr(synth, gen)(Cn, H, W, prec)
    p = G.TileParams.make(W, H, Cn, prec, L, irreversible=True)
    c = U.ctx()
    table, coded = c.encode_host(p, px)
    _, blocks, qcd, otable, ocoded = chain.encode_tile_oracle(px, prec, L, irrev=True)
    assert U.split_blocks(table, coded) == [bytes(ocoded[int(o):int(o) + int(n)]) for o, n in zip(otable["offset"], otable["length"])]
    cs = G.write_codestream(p, W, H, table, coded)
    ref = R.decode(cs, Cn, H, W)
    assert np.abs(ref.astype(np.int64) - px.astype(np.int64)).max() <= 8 and synth.psnr_db(ref, px, prec) >= 90.0
    assert np.array_equal(chain.decode_tile_oracle(p, blocks, qcd, table, bytes(coded)), ref)
    assert np.array_equal(c.decode_host(p, table, coded)[0].astype(np.int32), ref)


@needs_ref
def test_cfg4_64_tile_batch_equals_grk_compress_and_decodes():
    W = H = 8192
    T, L = 1024, 5
    px = synth.g2(3, H, W, 8)
    R.lib(threads=os.cpu_count() or 1)
    want, _ = R.encode(px, 8, TW=T, TH=T, numres=L + 1, mode=1)
    p = G.TileParams.make(T, T, 3, 8, L)
    tiles = np.ascontiguousarray(np.stack([px[:, ty * T:(ty + 1) * T, tx * T:(tx + 1) * T]
                                           for ty in range(H // T) for tx in range(W // T)]))
    assert tiles.shape[0] == 64
    c = U.ctx()
    table, coded = c.encode_host(p, tiles, ntiles=64)
    cs = G.write_codestream(p, W, H, table, coded)
    assert len(cs) == len(want) and hashlib.md5(cs).hexdigest() == hashlib.md5(want).hexdigest()
    # one tile of the batch through the oracle chain, block for block (the file equality above already implies it)
    bpt = len(table) // 64
    t = 37
    _, _, _, otable, ocoded = chain.encode_tile_oracle(tiles[t], 8, L)
    got = U.split_blocks(table[t * bpt:(t + 1) * bpt], coded)
    assert got == [bytes(ocoded[int(o):int(o) + int(n)]) for o, n in zip(otable["offset"], otable["length"])]
    # and back: the batch decode returns every tile
    back = c.decode_host(p, table, coded, ntiles=64)
    assert np.array_equal(back, tiles)


@needs_ref
def test_cfg4_whole_16k_image_256_tiles_equals_grk_compress():
    """BASELINE configs[3] itself on one GPU: 16384 x 16384 x 3 8-bit, 256 tiles of 1024 x 1024 in one batch, every tile
    different content; the codestream == the file Grok's CPU encoder writes for the image."""
    W = H = 16384
    T, L = 1024, 5
    px = synth.g2(3, H, W, 8)
    R.lib(threads=os.cpu_count() or 1)
    want, _ = R.encode(px, 8, TW=T, TH=T, numres=L + 1, mode=1)
    want_md5, want_len = hashlib.md5(want).hexdigest(), len(want)
    del want
    p = G.TileParams.make(T, T, 3, 8, L)
    tiles = np.ascontiguousarray(np.stack([px[:, ty * T:(ty + 1) * T, tx * T:(tx + 1) * T]
                                           for ty in range(H // T) for tx in range(W // T)]))
    del px
    assert tiles.shape[0] == 256
    c = U.ctx()
    table, coded = c.encode_host(p, tiles, ntiles=256)
    cs = G.write_codestream(p, W, H, table, coded)
    assert len(cs) == want_len and hashlib.md5(cs).hexdigest() == want_md5


@needs_ref
def test_cfg5_8k_12bit_part1_ict97_decode_equals_grk_decompress():
    S, prec, Cn = 8192, 12, 3
    R.lib(threads=os.cpu_count() or 1)
    px = synth.g2(Cn, S, S, prec)
    cs, _ = R.encode(px, prec, numres=6, mode=1, ht=0, irrev=1)
    ref = R.decode(cs, Cn, S, S)
    info = J.parse(cs)
    p = G.TileParams.make(S, S, Cn, prec, info["levels"], irreversible=True, mct=True, part1=True)
    blocks, _ = G.tile_layout(p)
    rows, data = J.decode_table(info, blocks, True)
    table = np.array(rows, dtype=G.capi.CODED_DTYPE)
    c = U.ctx()
    c.set_decode_qcd([(e << 11) | m for e, m in info["qcd"]])
    try:
        got = c.decode_host(p, table, data)[0].astype(np.int32)
    finally:
        c.set_decode_qcd([])
    assert np.array_equal(got, ref), "GPU decode differs from grk_decompress at %d samples" % int((got != ref).sum())
    assert np.abs(ref - px.astype(np.int32)).max() <= max(2, (1 << prec) // 64)


def test_16k_single_tile_round_trip_and_strip_checksums():
    """One 16384 x 16384 x 3 8-bit tile (805 MB of pixels, 196 608 code-blocks): four times the 8K frame through the same
    kernels -- 18 strips of the packed 5/3 kernels, 32-bit row offsets up to 512 MB into a plane.  Too large for the oracle
    in a test's time, so size-independent properties: the lossless round trip, and the blocks of its top-left 2048 x 2048
    corner's finest sub-bands, which depend on that corner + a margin only, equal the blocks of a 4096 x 4096 tile cut from the
    same pixels (that one checked against the oracle chain elsewhere in its class)."""
    S = 16384
    base = synth.g2(3, 4096, 4096, 8, seed=3)
    px = np.tile(base, (1, 4, 4))
    px[:, 5000:, :] = 255 - px[:, 5000:, :]                    # (not periodic in y)
    px[:, :, 9000:] = px[:, ::-1, 9000:]                      # (nor in x; x ^ 0x55 would be full-scale noise: defect D5)
    p = G.TileParams.make(S, S, 3, 8, 5)
    c = G.Context(0)
    d = U.to_dev(px.reshape(-1))
    table, tot = c.encode_tiles(p, 1, d.data_ptr(), True)
    back = U._settled(torch.zeros_like(d))
    c.decode_device(p, 1, table, c.coded_device_ptr(), tot, back.data_ptr())
    c.decode_status()
    assert torch.equal(back, d)
    coded = np.empty(tot, np.uint8)
    G.lib().grk_amd_fetch_coded(c._h, coded.ctypes.data, tot)
    # the whole file against the reference's own encoder on the same 16384 x 16384 single tile (the size
    # was covered by properties only) -- every one of the 196 608 blocks, Tier-2 and headers, byte for byte
    if R.have_ref():
        R.lib(threads=os.cpu_count() or 1)
        want, _ = R.encode(px, 8, numres=6, mode=1)
        cs = G.write_codestream(p, S, S, table, coded)
        assert len(cs) == len(want) and hashlib.md5(cs).hexdigest() == hashlib.md5(want).hexdigest()
        del want, cs
    # the same corner as its own 4096^2 tile
    small = np.ascontiguousarray(px[:, :4096, :4096])
    p4 = G.TileParams.make(4096, 4096, 3, 8, 5)
    t4, c4 = U.ctx().encode_host(p4, small)
    blocks16, _ = G.tile_layout(p)
    blocks4, _ = G.tile_layout(p4)
    big = {(b.comp, b.res, b.band, b.x0, b.y0): i for i, b in enumerate(blocks16)}
    checked = 0
    for j, b in enumerate(blocks4):
        if b.res != 5 or b.x1 > 1024 or b.y1 > 1024:     # finest resolution, well inside the corner
            continue
        i = big[(b.comp, b.res, b.band, b.x0, b.y0)]
        assert bytes(coded[int(table["offset"][i]):int(table["offset"][i]) + int(table["length"][i])]) == \
               bytes(c4[int(t4["offset"][j]):int(t4["offset"][j]) + int(t4["length"][j])]), (b.comp, b.band, b.x0, b.y0)
        checked += 1
    assert checked >= 3 * 3 * 256


def test_32k_single_tile_round_trip():
    """32768 x 32768 x 3 8-bit as ONE tile (3.2 G samples, 786 432 code-blocks, 2 GB per int16 plane -- the largest the packed
    kernels' 32-bit row offsets reach; larger planes take the flat-addressing kernels): lossless round trip."""
    S = 32768
    base = synth.g2(3, 4096, 4096, 8, seed=5)
    px = np.tile(base, (1, S // 4096, S // 4096))
    px[:, S // 3:, :] = 255 - px[:, S // 3:, :]
    p = G.TileParams.make(S, S, 3, 8, 5)
    c = G.Context(0)
    d = U.to_dev(px.reshape(-1))
    del px
    table, tot = c.encode_tiles(p, 1, d.data_ptr(), True)
    assert len(table) == 786432 and tot > 0
    back = U._settled(torch.zeros_like(d))
    c.decode_device(p, 1, table, c.coded_device_ptr(), tot, back.data_ptr())
    c.decode_status()
    assert torch.equal(back, d)
    # ... and the whole file against the reference's encoder on the same single tile (786 432 blocks, ~0.4 GB of codestream)
    if R.have_ref() and os.environ.get("GRK_AMD_SKIP_32K_REF") != "1":
        coded = np.empty(tot, np.uint8)
        G.lib().grk_amd_fetch_coded(c._h, coded.ctypes.data, tot)
        px = d.cpu().numpy().reshape(3, S, S)
        R.lib(threads=os.cpu_count() or 1)
        want, _ = R.encode(px, 8, numres=6, mode=1)
        cs = G.write_codestream(p, S, S, table, coded)
        assert len(cs) == len(want) and hashlib.md5(cs).hexdigest() == hashlib.md5(want).hexdigest()
