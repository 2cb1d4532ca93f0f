"""-m gpu: the kernels' branches on a code-block's bit-plane count, at the deep end.
K3 (HT encoder): wide quads (Kmax + 2 > 16), one-piece and split MagSgn packing chosen by wave-wide ballots, the irreversible
quantiser's clamp at 2^Kmax - 1, the capped LDS streams at 16 bits.  K5 / K5c (HT decoder, refinement passes): Kmax up to a
16-bit geometry's maximum, missing_msbs below Kmax - 1 (streams of other HT encoders).  K8 / K8L (Part-1 decoders): 13 .. 24
planes in one launch, every code-block style, truncated passes, both dequantisations, and the 25-plane refusal.
Every result is compared with the oracle (pinned to the reference on the CPU) or with the reference itself."""
import ctypes as C_
import os

import numpy as np
import pytest

import grok_amd as G
import chain
import gpuutil as U
import oracle as O
import refharness as R
from test_gpu_stages import _dev_view
from test_oracle_ebcot import deep_block

pytestmark = pytest.mark.gpu
needs_ref = pytest.mark.skipif(not R.have_ref(), reason="oracle/_ref not shipped")

# (W, H, L, C, prec): every band Kmax from 15 up to what 16-bit samples reach (reversible 15 .. 20, irreversible 16 .. 22)
GEOMS = [(64, 64, 0, 1, 16), (130, 67, 1, 3, 16), (200, 136, 3, 1, 16), (256, 192, 5, 1, 16), (96, 80, 3, 1, 13), (77, 45, 1, 3, 14)]


def _magnitudes(rng, bh, bw, top, mode):
    """magnitudes < 2^top: 0 uniform, 1 shifted down at random, 4 all at the top, 5 wide and narrow quads side by side (the
    wave's MagSgn ballots disagree), 6 every sample of 17 bits or more (a pair's two samples above 16 bits each)"""
    if mode == 0:
        return rng.integers(0, 1 << top, size=(bh, bw))
    if mode == 1:
        return rng.integers(0, 1 << top, size=(bh, bw)) >> rng.integers(0, top + 1, size=(bh, bw))
    if mode == 4:
        return np.full((bh, bw), (1 << top) - 1)
    if mode == 5:
        wide = np.kron(rng.random(((bh + 1) // 2, (bw + 1) // 2)) < 0.3, np.ones((2, 2), bool))[:bh, :bw]
        return np.where(wide, rng.integers(1 << (top - 1), 1 << top, size=(bh, bw)), rng.integers(0, 16, size=(bh, bw)))
    if mode == 6:
        lo = min(16, top - 1)
        return rng.integers(1 << lo, 1 << top, size=(bh, bw))
    raise ValueError(mode)


def _planes(p, blocks, rng, mode, top_of):
    C, H, W = p.num_comps, p.tile_h, p.tile_w
    planes = np.zeros((C, H, W), np.int64)
    for b in blocks:
        bw, bh = b.x1 - b.x0, b.y1 - b.y0
        mag = _magnitudes(rng, bh, bw, top_of(b), mode)
        planes[b.comp, b.py:b.py + bh, b.px:b.px + bw] = mag * np.where(rng.random((bh, bw)) < 0.5, -1, 1)
    return planes.astype(np.int32)


def _gpu_blocks(p, planes, nblocks):
    d_m = U.upload_planes(planes, p)
    c = U.ctx()
    c.stage_ht_encode(p, 1, d_m.data_ptr())
    table, tot = c.fetch_table(nblocks)
    return U.split_blocks(table, c.fetch_coded(tot))


# ---- K3 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,L,C,prec", GEOMS)
@pytest.mark.parametrize("mode", [0, 1, 4, 5, 6])
def test_k3_deep_kmax_blocks_equal_oracle(W, H, L, C, prec, mode):
    rng = np.random.default_rng(W * 7 + H + L * 3 + mode)
    p = G.TileParams.make(W, H, C, prec, L)
    blocks, _ = G.tile_layout(p)
    assert max(b.kmax for b in blocks) >= 15
    planes = _planes(p, blocks, rng, mode, lambda b: b.kmax)
    got = _gpu_blocks(p, planes, len(blocks))
    bad = []
    for i, b in enumerate(blocks):
        bw, bh = b.x1 - b.x0, b.y1 - b.y0
        want = O.ht_encode_sm(O.signmag(planes[b.comp, b.py:b.py + bh, b.px:b.px + bw], b.kmax), b.kmax)
        if got[i] != want:
            bad.append((i, b.kmax, bw, bh, len(got[i]), len(want)))
    assert not bad, "blocks differing from the oracle (idx, kmax, w, h, len_gpu, len_oracle): %s" % bad[:8]


@pytest.mark.parametrize("W,H,L,C,prec", [(64, 64, 0, 1, 16), (200, 136, 3, 1, 16), (130, 67, 5, 3, 12), (96, 64, 2, 1, 8)])
def test_k3_irreversible_quantiser_clamp(W, H, L, C, prec):
    """Float Mallat planes whose quantised magnitudes run up to and past lim = 2^Kmax - 1 (up to 4 lim): the kernel's
    min(q, lim) == orc_ht_signmag_irrev's clamp, block for block."""
    rng = np.random.default_rng(W + H + prec)
    p = G.TileParams.make(W, H, C, prec, L, irreversible=True, mct=False)
    blocks, _ = G.tile_layout(p)
    planes = np.zeros((C, H, W), np.float32)
    for b in blocks:
        bw, bh = b.x1 - b.x0, b.y1 - b.y0
        lim = float((1 << b.kmax) - 1)
        q = np.where(rng.random((bh, bw)) < 0.3, rng.uniform(0.9 * lim, 4.0 * lim, size=(bh, bw)), rng.uniform(0, lim, size=(bh, bw)))
        q[0, 0] = lim + 0.5
        if bw > 1:
            q[0, 1] = lim - 0.5
        v = (q * np.float64(b.stepsize)).astype(np.float32)
        planes[b.comp, b.py:b.py + bh, b.px:b.px + bw] = np.where(rng.random((bh, bw)) < 0.5, -v, v)
    got = _gpu_blocks(p, planes.view(np.int32), len(blocks))
    L_ = O.lib()
    bad, clamped = [], 0
    for i, b in enumerate(blocks):
        bw, bh = b.x1 - b.x0, b.y1 - b.y0
        sub = np.ascontiguousarray(planes[b.comp, b.py:b.py + bh, b.px:b.px + bw])
        sm = np.zeros((bh, bw), np.uint32)
        L_.orc_ht_signmag_irrev(sub.ctypes.data, bw, bw, bh, b.kmax, C_.c_float(np.float32(1.0) / np.float32(b.stepsize)), sm.ctypes.data)
        clamped += int(np.sum(((sm & 0x7FFFFFFF) >> np.uint32(30 - b.kmax)) == (1 << b.kmax) - 1))
        if got[i] != O.ht_encode_sm(sm, b.kmax):
            bad.append((i, b.kmax, bw, bh))
    assert clamped > len(blocks)
    assert not bad, "blocks differing from the oracle (idx, kmax, w, h): %s" % bad[:8]


@pytest.mark.parametrize("irrev", [False, True])
@pytest.mark.parametrize("kind", ["noise", "mixed"])
def test_k3_lds_cap_and_fallback_at_16_bits(irrev, kind, monkeypatch):
    """The capped LDS streams (kmax - 3 bits per sample above Kmax 11, 8 when irreversible) at 16 bits: noise overflows them, so the
    fallback launch codes those blocks again; GRK_AMD_LDS_CAP=1 == =0 == the oracle chain."""
    rng = np.random.default_rng(16 + irrev)
    C, H, W, L = 3, 256, 384, 5
    noise = rng.integers(0, 1 << 16, size=(C, H, W)).astype(np.uint16)
    smooth = np.clip(np.arange(W)[None, None, :] * 170 + np.arange(H)[None, :, None] * 9 + rng.integers(0, 64, size=(C, H, W)),
                     0, 65535).astype(np.uint16)
    px = noise if kind == "noise" else np.where((np.arange(W) // 128 % 2 == 0)[None, None, :], noise, smooth)
    px = np.ascontiguousarray(px)
    p = G.TileParams.make(W, H, C, 16, L, irreversible=irrev)
    got = {}
    for cap in ("1", "0"):
        monkeypatch.setenv("GRK_AMD_LDS_CAP", cap)
        c = G.Context(0)
        try:
            t, coded = c.encode_host(p, px)
            got[cap] = U.split_blocks(t, coded)
            handed = int(_dev_view(c.table_device_ptr(3), 24, "<i8").cpu().sum())
        finally:
            c.close()
        if cap == "0":
            assert handed == 0
        else:
            assert handed > 0, "no block reached the fallback launch"
    assert got["1"] == got["0"]
    _, _, _, otable, ocoded = chain.encode_tile_oracle(px, 16, L, irrev=irrev)
    assert got["1"] == [bytes(ocoded[int(o):int(o) + int(l)]) for o, l in zip(otable["offset"], otable["length"])]


# ---- K5 / K5c -------------------------------------------------------------------------------------------------------------
def _k5_case(W, H, L, C, prec, mode, seed, irrev=False, below=False):
    """HT blocks of the oracle's encoder -> K5 == the oracle's decode + dequantisation.  below: each block's missing_msbs is drawn
    from 1 .. Kmax - 1 and the block is coded at its own Kmax = missing_msbs + 1 (another encoder's zero-bit-plane counts)."""
    rng = np.random.default_rng(seed)
    p = G.TileParams.make(W, H, C, prec, L, irreversible=irrev, mct=False)
    blocks, qcd = G.tile_layout(p)
    table = np.zeros(len(blocks), G.capi.CODED_DTYPE)
    chunks, want, off, mms = [], [], 0, []
    for i, b in enumerate(blocks):
        bw, bh = b.x1 - b.x0, b.y1 - b.y0
        mm = int(rng.integers(1, b.kmax)) if below else b.kmax - 1
        kb = mm + 1
        coef = (_magnitudes(rng, bh, bw, max(kb - 2, 1), mode) * np.where(rng.random((bh, bw)) < 0.5, -1, 1)).astype(np.int32)
        if kb - 2 < 1:
            coef = np.clip(coef, -1, 1)
        cb = O.ht_encode_sm(O.signmag(coef, kb), kb)
        sm = O.ht_decode_block(cb, mm, bw, bh)
        assert sm is not None
        if irrev:
            want.append(O.ht_dequant_irrev(sm, chain.band_scale_dec(prec, qcd[chain.band_index(b)], b.kmax)).view(np.int32))
        else:
            want.append(O.ht_dequant_rev(sm, mm))
            assert np.array_equal(want[-1], coef)
        table["offset"][i] = off; table["length"][i] = len(cb); table["missing_msbs"][i] = mm
        chunks.append(cb + b"\0" * (-len(cb) % 16)); off += len(chunks[-1])
        mms.append(mm)
    coded = b"".join(chunks) + b"\0" * 16
    d_c = U.to_dev(np.frombuffer(coded, np.uint8))
    d_m = U.dev_planes(p, C)
    U.ctx().stage_ht_decode(p, 1, table, d_c.data_ptr(), d_c.numel(), d_m.data_ptr())
    U.ctx().synchronize()
    got = U.planes_to_numpy(d_m, p, C)
    bad = [(i, b.kmax, mms[i]) for i, b in enumerate(blocks)
           if not np.array_equal(got[b.comp, b.py:b.py + b.y1 - b.y0, b.px:b.px + b.x1 - b.x0], want[i])]
    assert not bad, "blocks differing from the oracle (idx, kmax, missing_msbs): %s" % bad[:8]
    return mms


@pytest.mark.parametrize("W,H,L,C,prec", GEOMS)
@pytest.mark.parametrize("mode", [0, 1, 4, 5])
def test_k5_deep_kmax_blocks_equal_oracle(W, H, L, C, prec, mode):
    _k5_case(W, H, L, C, prec, mode, W + H + mode)


@pytest.mark.parametrize("W,H,L,C,prec", [(200, 136, 3, 1, 16), (256, 192, 5, 1, 16), (130, 67, 2, 3, 8)])
@pytest.mark.parametrize("irrev", [False, True])
def test_k5_missing_msbs_below_kmax(W, H, L, C, prec, irrev):
    mms = _k5_case(W, H, L, C, prec, 1, W * 3 + irrev, irrev=irrev, below=True)
    assert min(mms) <= 2 and len(set(mms)) > 4


@needs_ref
@pytest.mark.parametrize("irrev", [False, True])
def test_k5c_refinement_at_deep_kmax(irrev):
    """SigProp / MagRef passes with cleanup magnitudes up to each block's own Kmax (the 16-bit geometry's 17 .. 22), not capped at 14."""
    from test_gpu_ht_refine import _case
    _case(200, 136, 3, 1, 16, irrev, 31 + irrev, lambda i: (i % 3) + 1, cap=None)
    _case(64, 64, 0, 1, 16, irrev, 41 + irrev, lambda i: 3, cap=None)


# ---- K8 / K8L -------------------------------------------------------------------------------------------------------------
DEEP_NBPS = [13, 14, 15, 16, 20, 24]


def _ctx_with(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return G.Context(0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _part1_deep_tile(rng, W, H, L, prec, irrev, sty, nbps_of, sparse_of, truncate):
    p = G.TileParams.make(W, H, 1, prec, L, part1=True, irreversible=irrev, mct=False, cblksty=sty)
    blocks, qcd = G.tile_layout(p)
    table = np.zeros(len(blocks), G.capi.CODED_DTYPE)
    chunks, off, seglist, nb = [], 0, [], []
    want = np.zeros((H, W), np.float32 if irrev else np.int32)
    for i, b in enumerate(blocks):
        bw, bh = b.x1 - b.x0, b.y1 - b.y0
        nbps = nbps_of(i)
        coef = deep_block(rng, bw, bh, nbps)
        if sparse_of(i):
            coef = np.where(rng.random((bh, bw)) < 0.97, 0, coef >> 4).astype(np.int32)
            coef[0, 0] = (1 << (nbps - 1)) + 1
        if sty:
            cb, segs, got_nbps = R.t1_encode_block_sty(coef, b.band, sty)
            if truncate(i) and len(segs) > 1:
                segs = segs[:max(1, len(segs) - int(rng.integers(1, 4)))]
            n = sum(a for a, _ in segs)
            ref = R.t1_decode_block_sty(cb[:n], segs, got_nbps, b.band, sty, bw, bh)
            npass = sum(k for _, k in segs)
            seglist.append(segs)
        else:
            cb, npass, got_nbps = R.t1_encode_block(coef, b.band)
            if truncate(i):
                npass = max(1, npass - int(rng.integers(1, 7)))
            n = len(cb)
            ref = R.t1_decode_block(cb, npass, got_nbps, b.band, bw, bh)
        assert got_nbps == nbps
        nb.append(nbps)
        table["offset"][i] = off; table["length"][i] = n; table["missing_msbs"][i] = got_nbps | (npass << 8)
        chunks.append(cb[:n] + b"\0" * (-n % 16 + 16)); off += len(chunks[-1])
        if irrev:
            wq = qcd[chain.band_index(b)]
            step = np.float32((1.0 + (wq & 0x7FF) / 2048.0) * 2.0 ** (prec - (wq >> 11)))
            want[b.py:b.py + bh, b.px:b.px + bw] = O.t1_dequant_irrev(ref, step)
        else:
            want[b.py:b.py + bh, b.px:b.px + bw] = O.t1_dequant_rev(ref)
            if not truncate(i):
                assert np.array_equal(want[b.py:b.py + bh, b.px:b.px + bw], coef)
    return p, blocks, table, b"".join(chunks), want, (seglist if sty else None), nb


def _k8_run(c, p, table, coded, seglist):
    d_c = U.to_dev(np.frombuffer(coded, np.uint8))
    d_m = U.dev_planes(p, 1)
    if seglist is not None:
        c.set_decode_segments(seglist)
    try:
        c.stage_ht_decode(p, 1, table, d_c.data_ptr(), d_c.numel(), d_m.data_ptr())
        c.synchronize()
    finally:
        if seglist is not None:
            c.set_decode_segments(None)
    return U.planes_to_numpy(d_m, p, 1)[0].copy()


@needs_ref
@pytest.mark.parametrize("irrev,truncate", [(False, False), (False, True), (True, True)])
def test_k8_and_k8l_on_both_sides_of_14_planes(irrev, truncate):
    """One launch with blocks of 13 .. 24 planes: short 13- and 14-plane blocks go to the lane decoder (K8L, free-running and
    pass-synchronous) and long ones of 13 .. 24 planes to the wave decoder (K8, int16 workspace up to 14 planes, int32 beyond);
    every route == the reference's T1 + the oracle's dequantisation."""
    rng = np.random.default_rng(13 + 2 * irrev + truncate)
    W, H = 1280, 1024
    # i % 4 == 1 / 2: sparse blocks of 13 / 14 planes, all passes (groups of 80 equal rows: the pass-synchronous waves take them);
    # 0: dense blocks of 13 .. 24 planes, 3: dense blocks of 13 / 14 planes -- long, K8's
    nbps_of = lambda i: DEEP_NBPS[(i // 4) % 6] if i % 4 == 0 else 13 if i % 4 == 1 else 14 if i % 4 == 2 else (13, 14)[(i // 4) % 2]
    sparse = lambda i: i % 4 in (1, 2)
    trunc = (lambda i: not sparse(i) and i % 8 >= 3) if truncate else (lambda i: False)
    p, blocks, table, coded, want, _, nb = _part1_deep_tile(rng, W, H, 0, 12, irrev, 0, nbps_of, sparse, trunc)
    lens = table["length"].astype(np.int64)
    thr = max(64, lens.max() // 4)
    lane_ok = [i for i, b in enumerate(blocks) if nb[i] <= 14 and lens[i] <= thr and b.y1 - b.y0 >= 9]
    assert len(lane_ok) >= 128 and {13, 14} <= {nb[i] for i in lane_ok}
    assert {nb[i] for i in range(len(blocks)) if lens[i] > thr} >= {13, 14, 15, 16, 20, 24}
    if irrev:
        U.ctx().set_decode_qcd([])
    for env in ({"GRK_AMD_T1_LANES": "2"}, {"GRK_AMD_T1_LANES": "2", "GRK_AMD_T1_SYNC": "0"}, {"GRK_AMD_T1_LANES": "0"}):
        c = _ctx_with(env)
        try:
            got = _k8_run(c, p, table, coded, None)
        finally:
            c.close()
        assert np.array_equal(got, want.view(np.int32)), "%s: %d samples differ" % (env, int((got != want.view(np.int32)).sum()))


@needs_ref
@pytest.mark.parametrize("sty", [0x01, 0x02, 0x04, 0x08, 0x10, 0x20, 0x01 | 0x04, 0x02 | 0x08 | 0x20, 0x3F, 0x04 | 0x10])
def test_k8_deep_planes_every_style(sty):
    rng = np.random.default_rng(500 + sty)
    p, blocks, table, coded, want, segs, _ = _part1_deep_tile(rng, 256, 136, 1, 12, bool(sty & 0x10), sty,
                                                              lambda i: DEEP_NBPS[i % 6], lambda i: False, lambda i: i % 2 == 1)
    got = _k8_run(U.ctx(), p, table, coded, segs)
    assert np.array_equal(got, want.view(np.int32)), "%d samples differ" % int((got != want.view(np.int32)).sum())


@needs_ref
def test_k8_refuses_25_planes_as_a_part1_block():
    """numbps >= 25: the reference's T1 refuses the block (pinned in test_oracle_ebcot.py); the GPU decode fails with a Part-1
    error and leaves the block's samples at zero, its neighbours decoded."""
    rng = np.random.default_rng(25)
    p, blocks, table, coded, want, _, _ = _part1_deep_tile(rng, 128, 64, 0, 12, False, 0, lambda i: 24, lambda i: False, lambda i: False)
    table["missing_msbs"][1] = 25 | (int(table["missing_msbs"][1]) & 0xFFFFFF00)
    with pytest.raises(RuntimeError):
        R.t1_decode_block(coded[int(table["offset"][1]):int(table["offset"][1]) + int(table["length"][1])],
                          int(table["missing_msbs"][1]) >> 8, 25, blocks[1].band, 64, 64)
    c = G.Context(0)
    try:
        d_c = U.to_dev(np.frombuffer(coded, np.uint8))
        d_m = U.dev_planes(p, 1)
        with pytest.raises(RuntimeError, match="Part-1"):
            c.stage_ht_decode(p, 1, table, d_c.data_ptr(), d_c.numel(), d_m.data_ptr())
        got = U.planes_to_numpy(d_m, p, 1)[0]
    finally:
        c.close()
    assert np.array_equal(got[:, :64], want[:, :64])
    assert not got[:, 64:].any()
