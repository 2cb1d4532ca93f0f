"""-m gpu: the HT block decoder (K5a ht_dec_vlc_kernel, K5b ht_dec_ms_kernel, K5c) on cleanup segments framed as OTHER encoders may
frame them (tests/htframes.py: MagSgn padded with zeros or with its 0xFF kept, spare bytes behind it, MEL and VLC never fused, MEL
padded with ones, zero bytes between MEL and VLC up to Scup 4079).  Every block of every case was, until here, framed by the one
encoder algorithm the oracle, the reference and K3 share; a decoder that leaned on that algorithm's habits would have passed.
All comparisons are exact; what is expected comes from the source samples or from the oracle, never from the GPU.  That every
variant changes bytes in every case is counted on the CPU (tests/test_ht_frames_cpu.py), from the same seeds."""
import numpy as np
import pytest
import torch

import grok_amd as G
import chain
import gpuutil as U
import htframes as F
import oracle as O
import refharness as R
import synth

pytestmark = pytest.mark.gpu
needs_ref = pytest.mark.skipif(not R.have_ref(), reason="oracle/_ref (the real reference) not built here")


def _place(items, variant=None, filler=None, pad16=True, first=0):
    """-> (table, coded bytes, [segments]).  pad16: every block at a 16-byte offset of a zero-padded buffer (the habit of the other
    tests); otherwise the blocks end to end, the k-th one in the buffer behind `filler(k)` bytes, nothing behind the last one.
    first: the block that lies first in the buffer (the others follow in table order, cyclically)."""
    n = len(items)
    table = np.zeros(n, G.capi.CODED_DTYPE)
    chunks, segs, off = [], [None] * n, 0
    for k in range(n):
        i = (first + k) % n
        it = items[i]
        cup = it.framed(variant) if it.raw is not None else b""
        data = cup + it.seg
        table["offset"][i] = off; table["length"][i] = len(data); table["missing_msbs"][i] = it.mm
        tail = b"\0" * (-len(data) % 16) if pad16 else (filler(k) if filler and k + 1 < n else b"")
        chunks.append(data + tail); off += len(chunks[-1])
        segs[i] = [(len(cup), 1)] + ([(len(it.seg), it.npasses - 1)] if it.seg else [])
    return table, b"".join(chunks) + (b"\0" * 16 if pad16 else b""), segs


def _source_planes(p, blocks, items):
    planes = np.zeros((p.num_comps, p.tile_h, p.tile_w), np.int32)
    for b, it in zip(blocks, items):
        planes[b.comp, b.py:b.py + b.y1 - b.y0, b.px:b.px + b.x1 - b.x0] = it.coef
    return planes


def _decode(p, table, coded, planes16=False, segs=None):
    assert len(coded) > 0
    d_c = U.to_dev(np.frombuffer(coded, np.uint8).copy())
    assert d_c.numel() == len(coded)                                  # (nothing behind the coded bytes but the allocator's own slack)
    C = p.num_comps
    d_m = U.dev_planes16(p, C) if planes16 else U.dev_planes(p, C)
    c = U.ctx()
    if segs is not None:
        c.set_decode_segments(segs)
    try:
        (c.stage_ht_decode16 if planes16 else c.stage_ht_decode)(p, 1, table, d_c.data_ptr(), len(coded), d_m.data_ptr())
        c.synchronize()
    finally:
        if segs is not None:
            c.set_decode_segments(None)
    return (U.planes16_to_numpy if planes16 else U.planes_to_numpy)(d_m, p, C)


def _differing(blocks, items, got, want_of):
    bad = []
    for i, (b, it) in enumerate(zip(blocks, items)):
        bw, bh = b.x1 - b.x0, b.y1 - b.y0
        g, w = got[b.comp, b.py:b.py + bh, b.px:b.px + bw], want_of(i, b, it)
        if not np.array_equal(g, w):
            bad.append((i, it.name, bw, bh, int((g != w).sum())))
    return bad


# ---- a. stage_ht_decode, reversible -----------------------------------------------------------------------------------------------
REV_CASES = ["rev-64x64", "rev-130x67", "rev-128-cblk64x4", "rev-128-cblk4x64", "rev-200x120-p12"]


@pytest.mark.parametrize("case", REV_CASES)
def test_rotating_framings_decode_to_the_source(case):
    """variant_of(i) per block: the lanes of one K5a wave read differently framed blocks; content modes 0, 1, 2, 4 rotate, every
    7th block is absent"""
    p, blocks, _, items = F.build_case(case)
    assert [F.CASES[k]["geom"] for k in REV_CASES] == F.REV_GEOMS
    table, coded, _ = _place(items)
    got = _decode(p, table, coded)
    bad = _differing(blocks, items, got, lambda i, b, it: it.coef)
    assert not bad, "blocks differing from the source (idx, framing, w, h, samples): %s" % bad[:8]
    assert np.array_equal(got, _source_planes(p, blocks, items))


@pytest.mark.parametrize("name", F.VARIANT_NAMES)
def test_whole_tile_in_one_framing_decodes_to_the_source(name):
    p, blocks, _, items = F.build_case("rev-130x67")
    table, coded, _ = _place(items, variant=name)
    assert np.array_equal(_decode(p, table, coded), _source_planes(p, blocks, items))


# ---- b. irreversible --------------------------------------------------------------------------------------------------------------
def test_rotating_framings_irreversible_scale():
    """as test_gpu_decode.test_ht_decode_irreversible_scale: the planes are ht_dequant_irrev of the oracle's decode (of the habitual
    framing: the CPU tests hold every variant to the same words)"""
    p, blocks, qcd, items = F.build_case("irrev-256x192")
    table, coded, _ = _place(items)
    got = _decode(p, table, coded)

    def want(i, b, it):
        bw, bh = b.x1 - b.x0, b.y1 - b.y0
        sm = O.ht_decode_block(it.habit(), b.kmax - 1, bw, bh) if it.raw is not None else np.zeros((bh, bw), np.uint32)
        return O.ht_dequant_irrev(sm, chain.band_scale_dec(p.prec, qcd[chain.band_index(b)], b.kmax)).view(np.int32)
    bad = _differing(blocks, items, got, want)
    assert not bad, "blocks differing from the oracle (idx, framing, w, h, samples): %s" % bad[:8]


# ---- c. stage_ht_decode16 -----------------------------------------------------------------------------------------------------------
def test_rotating_framings_int16_planes():
    p, blocks, _, items = F.build_case("dec16-130x67")
    planes = _source_planes(p, blocks, items)
    assert 256 < np.abs(planes).max() <= 2047
    table, coded, _ = _place(items)
    got = _decode(p, table, coded, planes16=True)
    assert got.dtype == np.int16 and np.array_equal(got, planes)


# ---- d. placement -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", [None, 0x00, 0xFF], ids=["end-to-end", "filler-00", "filler-ff"])
def test_blocks_end_to_end_and_behind_filler_bytes(fill):
    """No padding anywhere: the first block at offset 0, the offsets of the others at every residue mod 4 and mod 16, the last byte of
    the last block the last byte of the device buffer, coded_bytes exact; then 1 .. 3 filler bytes between the blocks.  (The interface
    asks for no padding; K5a's and K5b's wide loads are guarded.)"""
    p, blocks, _, items = F.build_case("rev-130x67")
    n = len(items)
    filler = (lambda k: bytes([fill]) * (1 + k % 3)) if fill is not None else None
    want = _source_planes(p, blocks, items)
    # 26 coded blocks do not take 16 residues in one buffer: the tile is decoded from two, with block 0 and with block 1 lying first
    seen = set()
    for first in (0, 1):
        last = (first - 1) % n
        table, coded, _ = _place(items, pad16=False, filler=filler, first=first)
        offs = {int(o) for o, ln in zip(table["offset"], table["length"]) if ln}
        seen |= {o % 16 for o in offs}
        assert table["length"][first] > 0 and table["offset"][first] == 0 and {o % 4 for o in offs} == {0, 1, 2, 3}
        assert int(table["offset"][last]) + int(table["length"][last]) == len(coded) and table["length"][last] > 0
        if fill is not None:
            a = np.frombuffer(coded, np.uint8)
            ends = [int(o) + int(ln) for o, ln in zip(table["offset"], table["length"]) if ln and int(o) + int(ln) < len(coded)]
            assert ends and all(a[e] == fill for e in ends)
        assert np.array_equal(_decode(p, table, coded), want), first
    assert len(seen) == 16


# ---- e. refinement passes behind framed cleanup segments ----------------------------------------------------------------------------
def test_refinement_segments_behind_rotating_framings():
    p, blocks, _, items = F.build_case("refine-200x120")
    table, coded, segs = _place(items)
    assert sum(len(s) == 2 for s in segs) > len(items) // 2
    got = _decode(p, table, coded, segs=segs)

    def want(i, b, it):
        bw, bh = b.x1 - b.x0, b.y1 - b.y0
        words = O.ht_refine_decode(O.ht_decode_block(it.habit(), it.mm, bw, bh), it.mm, it.seg, it.npasses)
        return O.ht_dequant_rev(words, it.mm)
    bad = _differing(blocks, items, got, want)
    assert not bad, "blocks differing from the oracle (idx, framing, w, h, samples): %s" % bad[:8]


# ---- f. missing_msbs above the block's own Kmax ---------------------------------------------------------------------------------------
def test_rotating_framings_at_missing_msbs_above_kmax():
    """the GPU twin of test_oracle_decode.test_ht_decode_every_missing_msbs_vs_reference: a block coded at kb decodes at any
    missing_msbs from kb - 1 to 29"""
    p, blocks, _, items = F.build_case("mm-130x67")
    over = [it.mm - (it.kmax - 1) for it in items]
    assert min(over) == 0 and max(it.mm for it in items) == 29 and len(set(over)) > 8
    table, coded, _ = _place(items)
    got = _decode(p, table, coded)

    def want(i, b, it):
        h, w = it.coef.shape
        v = O.ht_dequant_rev(O.ht_decode_block(it.framed(), it.mm, w, h), it.mm)
        assert np.array_equal(v, it.coef)
        return v
    bad = _differing(blocks, items, got, want)
    assert not bad, "blocks differing from the oracle (idx, framing, w, h, samples): %s" % bad[:8]


# ---- g. a whole tile and a whole file ---------------------------------------------------------------------------------------------
def _image():
    px = synth.g2(3, 96, 160, 8)
    p, blocks, _, items = F.build_case("image-96x160")
    table, coded, _ = _place(items, pad16=False)
    return px, p, table, coded


def test_whole_tile_of_rotating_framings_decodes_to_the_pixels():
    px, p, table, coded = _image()
    assert np.array_equal(U.ctx().decode_host(p, table, coded)[0], px)


def test_whole_file_of_rotating_framings_decodes_to_the_pixels():
    px, p, table, coded = _image()
    cs = G.write_codestream(p, 160, 96, table, coded)
    c = U.ctx()
    assert np.array_equal(c.decode_image(cs), px)
    d = U.to_dev(np.frombuffer(cs, np.uint8))
    out = U._settled(torch.zeros(px.nbytes, dtype=torch.uint8, device="cuda"))
    c.decode_image_resident_ex(d.data_ptr(), d.numel(), out.data_ptr(), out.numel())
    c.decode_status()
    assert np.array_equal(out.cpu().numpy().reshape(px.shape), px)


@needs_ref
def test_whole_file_of_rotating_framings_through_the_reference_decoder():
    px, p, table, coded = _image()
    cs = G.write_codestream(p, 160, 96, table, coded)
    assert np.array_equal(R.decode(cs, 3, 96, 160), px.astype(np.int32))


# ---- h. refusal -------------------------------------------------------------------------------------------------------------------
def test_scup_4080_is_refused_and_the_context_goes_on():
    p, blocks, _, items = F.build_case("rev-64x64")
    it = items[0]
    bad = F.frame(it.raw, fuse=False, scup=4080)
    assert F.scup_of(bad) == 4080 and O.ht_decode_block(bad, it.mm, 64, 64) is None
    table = np.zeros(1, G.capi.CODED_DTYPE)
    table["length"][0] = len(bad); table["missing_msbs"][0] = it.mm
    with pytest.raises(RuntimeError):
        _decode(p, table, bad)
    good = F.frame(it.raw, fuse=False, scup=4079)
    table["length"][0] = len(good)
    assert np.array_equal(_decode(p, table, good), _source_planes(p, blocks, items))
