"""-m gpu: every precision from 1 to 16 through the whole GPU route (the file suites elsewhere run 8 and 12 bits; the packed int16
planes take every reversible precision up to 8, the egress clamps both rails).  Reversible HT files == grk_compress byte for byte
(host and device Tier-2), unsigned and signed, and decode back to the source; irreversible blocks == the oracle chain's, decoded ==
its decode chain and grk_decompress; Part-1 streams of the reference at 13 .. 16 bits decode as grk_decompress does.  A seeded
selection of the cross product keeps the sweep short; tests/test_oracle_golden.py runs the whole product on the CPU chain."""
import numpy as np
import pytest

import grok_amd as G
import chain
import gpuutil as U
import j2kparse as J
import refharness as R
import synth

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not R.have_ref(), reason="oracle/_ref not shipped")]


def _cases(n, seed):
    """every precision at least twice, with components, levels and content kinds drawn for each"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        prec = k % 16 + 1
        C = int(rng.choice([1, 3]))
        L = int(rng.choice([0, 1, 5]))
        kind = synth.KINDS[int(rng.integers(0, len(synth.KINDS)))]
        out.append((prec, C, L, kind, k % 3 == 0))
    return out


def _shape(L):
    return (37, 53) if L < 5 else (70, 90)


@pytest.mark.parametrize("prec,C,L,kind,device_t2", _cases(48, 2026))
def test_reversible_file_every_precision_equals_grk_compress(prec, C, L, kind, device_t2):
    H, W = _shape(L)
    px = synth.content(kind, C, H, W, prec, seed=prec * 31 + C + L)
    want, _ = R.encode(px, prec, numres=L + 1, mode=1)
    c = U.ctx()
    p = G.TileParams.make(W, H, C, prec, L)
    table, coded = c.encode_host(p, px)
    assert G.write_codestream(p, W, H, table, coded) == want, "host Tier-2"
    if device_t2:
        assert c.encode_image(G.ImageLayout.make(W, H), G.TileParams.make(1, 1, C, prec, L), px) == want, "device Tier-2"
    try:
        ref = R.decode(want, C, H, W)
    except RuntimeError:                  # full-scale content: the reference's decoder refuses U_q > missing_msbs (D5), so does ours
        with pytest.raises(RuntimeError):
            c.decode_host(p, table, coded)
        return
    assert np.array_equal(ref, px.astype(np.int32))
    assert np.array_equal(c.decode_host(p, table, coded)[0], px)


@pytest.mark.parametrize("prec", range(2, 17))
def test_signed_file_every_precision_equals_grk_compress(prec):
    """Signed components (SIZ Ssiz bit 7): the GPU file == grk_compress's file of the unsigned image u = s + 2^(prec-1) marked signed
    (R.with_signed_siz; pinned to grk_compress of the signed samples in test_oracle_golden.py), grk_decompress of it and the GPU
    decode == the source."""
    rng = np.random.default_rng(prec)
    C, L = (1, 3) if prec % 2 else (3, 1)
    kind = ("ramp", "noise", "checker", "low", "high")[prec % 5]
    H, W = 41, 67
    u = synth.content(kind, C, H, W, prec, seed=int(rng.integers(0, 1000)))
    px = (u.astype(np.int32) - (1 << (prec - 1))).astype(np.int8 if prec <= 8 else np.int16)
    want = R.with_signed_siz(R.encode(u, prec, numres=L + 1, mode=1)[0])
    if R.reads_signed():
        assert R.encode(px, prec, numres=L + 1, mode=1)[0] == want
    c = U.ctx()
    p = G.TileParams.make(W, H, C, prec, L, sgnd=True)
    table, coded = c.encode_host(p, px)
    assert G.write_codestream(p, W, H, table, coded) == want
    try:
        ref = R.decode(want, C, H, W)
    except RuntimeError:
        with pytest.raises(RuntimeError):
            c.decode_host(p, table, coded)
        return
    assert np.array_equal(ref, px.astype(np.int32))
    assert np.array_equal(c.decode_host(p, table, coded)[0].view(px.dtype), px)


@pytest.mark.parametrize("prec", range(1, 17))
def test_irreversible_every_precision_equals_oracle_chain(prec):
    """ICT + 9/7 + dead-zone quantiser at every precision (no reference HT bytes to match: D1): blocks == the oracle chain's; the
    decode == the oracle's decode chain, and == grk_decompress where it accepts the stream."""
    C = 3 if prec % 2 else 1
    L = (1, 3, 5)[prec % 3]
    kind = ("noise", "checker", "ramp", "impulse")[prec % 4]
    H, W = 48, 70
    px = synth.content(kind, C, H, W, prec, seed=prec + 100)
    p, blocks, qcd, otable, ocoded = chain.encode_tile_oracle(px, prec, L, irrev=True)
    c = U.ctx()
    table, coded = c.encode_host(p, px)
    got = U.split_blocks(table, coded)
    want = [bytes(ocoded[int(o):int(o) + int(l)]) for o, l in zip(otable["offset"], otable["length"])]
    bad = [i for i in range(len(want)) if got[i] != want[i]]
    assert not bad, "blocks differing from the oracle chain: %s" % bad[:10]
    try:
        ref = chain.decode_tile_oracle(p, blocks, qcd, otable, ocoded)
    except AssertionError:
        with pytest.raises(RuntimeError):
            c.decode_host(p, table, coded)
        return
    back = c.decode_host(p, table, coded)[0].astype(np.int32)
    assert np.array_equal(back, ref.astype(np.int32))
    cs = G.write_codestream(p, W, H, table, coded)
    try:
        grk = R.decode(cs, C, H, W)
    except RuntimeError:
        return
    assert np.array_equal(back, grk)


@pytest.mark.parametrize("prec", [13, 14, 15, 16])
@pytest.mark.parametrize("irrev,sty", [(0, 0), (0, 0x01), (1, 0x04), (0, 0x3F), (1, 0)])
def test_part1_reference_stream_deep_precision(prec, irrev, sty):
    """grk_compress Part-1 streams at 13 .. 16 bits (code-blocks of 12 .. 18 bit-planes: K8's int32 workspace), reversible and
    ICT + 9/7, with code-block styles: full decode == grk_decompress (== the source when reversible), a window == the crop of it
    and == grk_decompress_set_window (except D12: the reference's own narrow windows left undecoded)."""
    C, H, W, L = 3, 96, 136, 4
    px = synth.content(("noise", "ramp", "checker", "impulse")[prec % 4], C, H, W, prec, seed=prec)
    cs, _ = R.encode(px, prec, numres=L + 1, mode=1, ht=0, irrev=irrev, cblksty=sty)
    info = J.parse(cs)
    p = G.TileParams.make(W, H, C, prec, L, irreversible=bool(irrev), mct=True, part1=True, cblksty=sty & 0x3F)
    blocks, _ = G.tile_layout(p)
    rows, data = J.decode_table(info, blocks, True)
    table = np.array(rows, dtype=G.capi.CODED_DTYPE)
    c = U.ctx()
    c.set_decode_qcd([(e << 11) | m for e, m in info["qcd"]] if irrev else [])
    if sty & 0x05:
        c.set_decode_segments(J.segment_list(info, blocks))
    try:
        full = c.decode_host(p, table, data)[0].astype(np.int32)
        assert np.array_equal(full, R.decode(cs, C, H, W))
        if not irrev:
            assert np.array_equal(full, px.astype(np.int32))
        x0, y0, x1, y1 = 17, 9, 120, 70
        got = c.decode_region_host(p, table, data, x0, y0, x1, y1).astype(np.int32)
        assert np.array_equal(got, full[:, y0:y1, x0:x1])
        refw = R.decode_window(cs, C, x0, y0, x1, y1)
        if not np.array_equal(refw, got):
            assert np.all(refw == refw.flat[0]), "reference window differs from its own full decode in an unexpected way"
    finally:
        c.set_decode_qcd([])
        c.set_decode_segments(None)
