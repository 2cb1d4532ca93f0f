"""-m gpu: quality-targeted encodes, whole calls -- grk_amd_encode_tiles_quality, _image_quality (one tile, 2 x 2 tiles, tiles of
several geometries over one set of joint tables), _image_subsampled_quality (4:2:0), _surface_quality (NV12) and _packed_quality
(YUY2).  3 components, 8 bits, 2 levels, 32 x 32 code-blocks, 5/3 and 9/7, Dmax 6 with SKIP; targets of 50, 40 and 30 dB and D = 0.
The allocation is held against the call's own tables (grk_amd_rate_tables) restated in numpy, the files against their rows, the
plain file and the decoders.  The PSNR of the decoded pixels is printed beside the model's, not asserted: the model leaves out the
9/7 quantiser's own error and the transform's departure from orthogonality (include/grok_amd.h; profiles/quality.txt has an MI355X's
figures)."""
import math

import numpy as np
import pytest

import grok_amd as G
import gpuutil as U
import packedref as PR
import refharness as R
import synth
from grok_amd.capi import ERR_INVALID, ERR_UNSUPPORTED
from test_t2_reader_subsampled_cpu import make_planes, num_tiles, tile_comp

pytestmark = pytest.mark.gpu
SKIP = G.DROP_SKIP
DMAX, NC = 6, 8
S420 = [(1, 1), (2, 2), (2, 2)]
S422 = [(1, 1), (2, 1), (2, 1)]
TARGETS = (50.0, 40.0, 30.0)
LEVELS, CBLK = 2, (5, 5)


def clip(planes, irrev):
    """9/7 content in the middle of the range, as synth.g2_mid clips it: the plain file's darkest LL block is then one the decoders
    take (tests/test_gpu_rate_joint.py has the story)"""
    return [np.clip(p, 32, 224).astype(p.dtype) for p in planes] if irrev else list(planes)


class Case:
    """one input: call(psnr, distortion) -> (file, QualityResult); plain() -> the plain file under GRK_AMD_IMAGE_T2=host; kmax: Kmax
    of every block in joint order; planes: the source, one array per component; ref(cs): the reference's decode"""

    def __init__(self, kind, irrev):
        c = self.c = U.ctx()
        self.kind, self.irrev = kind, irrev
        kw = dict(max_drop=DMAX, allow_skip=True)
        if kind in ("one tile", "2x2 tiles", "ragged"):
            W, H, TW, TH = {"one tile": (128, 128, 128, 128), "2x2 tiles": (128, 128, 64, 64), "ragged": (100, 76, 64, 48)}[kind]
            layout = G.ImageLayout.make(W, H, TW, TH)
            base = G.TileParams.make(TW, TH, 3, 8, LEVELS, irreversible=irrev, cblk=CBLK)
            px = np.stack(clip(list(synth.g2(3, H, W, 8)), irrev))
            self.planes = list(px)
            self.kmax = [b.kmax for p in G.layout_tiles(layout, base) for b in G.tile_layout(p)[0]]
            self.call = lambda psnr, dist=0.0: c.encode_image_quality(layout, base, px, psnr, dist, **kw)
            self.plain = lambda: c.encode_image(layout, base, px)
            self.ref = lambda cs: list(R.decode(cs, 3, H, W))
            self.units = len(G.layout_tiles(layout, base))
        else:
            sampling = S422 if kind in ("YUY2", "NV16") else S420
            W, H, tile = (70, 37, (32, 32)) if kind in ("YUY2", "NV16") else (100, 76, (64, 48))
            layout = G.ImageLayout.make(W, H, *tile)
            base = G.TileParams.make(1, 1, 3, 8, LEVELS, mct=False, irreversible=irrev, cblk=CBLK)
            self.planes = planes = clip(make_planes(layout, sampling, 8, seed=9), irrev)
            self.kmax = [b.kmax for t in range(num_tiles(layout)) for dx, dy in sampling for b in G.tile_layout(tile_comp(layout, base, dx, dy, t))[0]]
            self.ref = lambda cs: R.decode_planes(cs, sampling, W, H)
            self.units = 2 * num_tiles(layout)
            if kind == "420":
                self.call = lambda psnr, dist=0.0: c.encode_image_subsampled_quality(layout, base, sampling, planes, psnr, dist, **kw)
                self.plain = lambda: c.encode_image_subsampled(layout, base, sampling, planes)
            elif kind in ("NV12", "NV16"):
                surface, samp, nbytes = G.Surface.make(kind, layout, pitch=W + 14)
                assert samp == sampling
                buf = np.random.default_rng(3).integers(0, 256, nbytes, dtype=np.uint8)
                surface.scatter(buf, planes, 1)
                self.call = lambda psnr, dist=0.0: c.encode_surface_quality(layout, base, sampling, surface, buf, psnr, dist, **kw)
                self.plain = lambda: c.encode_surface(layout, base, sampling, surface, buf)
            else:
                frame = PR.pack(PR.YUY2, 8, *planes, 0, np.random.default_rng(4).integers(0, 256, PR.frame_bytes(PR.YUY2, W, H, 0), dtype=np.uint8))
                self.call = lambda psnr, dist=0.0: c.encode_packed_quality(layout, base, "YUY2", frame, psnr, dist, **kw)
                self.plain = lambda: c.encode_packed(layout, base, "YUY2", frame)
        self.samples = sum(p.size for p in self.planes)

    def plain_host(self, monkeypatch):
        monkeypatch.setenv("GRK_AMD_IMAGE_T2", "host")
        try:
            return self.plain()
        finally:
            monkeypatch.delenv("GRK_AMD_IMAGE_T2")


def tables(c):
    n = c.rate_num_blocks()
    L, E, W, drop = c.rate_tables(n, DMAX)
    return n, L.astype(np.int64), E, W, drop, np.where(drop == SKIP, DMAX + 1, drop).astype(np.int64)


def model_distortion(W, E, cand):
    return float((W * E[cand, np.arange(len(W))].astype(np.float64)).sum())


def check_allocation(case, psnr, cs, res):
    """one call's result against its own tables -> (candidates, the decoded planes)"""
    c = case.c
    n, L, E, W, drop, cand = tables(c)
    ar = np.arange(n)
    what = "%s %s at %s dB" % (case.kind, "9/7" if case.irrev else "5/3", psnr)
    # the budget is plan_quality's
    want = 0.0 if math.isinf(psnr) else case.samples * 255.0 ** 2 * 10 ** (-psnr / 10)
    assert abs(res.budget - want) <= 1e-12 * want and c.quality_last_budget() == res.budget and c.rate_last_budget() == 0, what
    assert n == len(case.kmax) and len(c.rate_unit_rows()) == case.units, what
    # within the budget, up to the rounding a fixed-order sum of n positive terms can carry
    assert res.distortion <= res.budget * (1 + n * 2.0 ** -52), (what, res.distortion, res.budget)
    dist = model_distortion(W, E, cand)
    assert abs(res.distortion - dist) <= 1e-9 * max(dist, 1e-300), (what, res.distortion, dist)
    if res.distortion == 0:
        assert res.psnr == math.inf, what
    else:
        assert abs(res.psnr - 10 * math.log10(case.samples * 255.0 ** 2 / res.distortion)) < 1e-9, what
    # the bytes are the chosen candidates', and so are the file's rows
    bytes_ = int(L[cand, ar].sum())
    assert res.block_bytes == bytes_ and res.file_bytes == len(cs) and res.lagrange_bytes >= res.block_bytes, what
    rows = G.read_packets(cs)["rows"]
    assert np.array_equal(rows["length"], L[cand, ar]), what
    assert np.array_equal(rows["missing_msbs"], [k - 1 if d == SKIP else k - 1 - min(int(d), k - 1) for k, d in zip(case.kmax, drop)]), what
    # after the trim: no block's next coarser candidate with fewer bytes has a delta within the slack
    slack = res.budget - res.distortion
    coarser = np.minimum(cand + 1, NC - 1)
    delta = W * (E[coarser, ar].astype(np.int64) - E[cand, ar].astype(np.int64)).astype(np.float64)
    could = (cand + 1 < NC) & (L[coarser, ar] < L[cand, ar]) & (delta <= slack)
    assert not could.any(), (what, np.flatnonzero(could)[:8], slack)
    # the Lagrange choice restated (ties: the finer candidate, argmin's first); the trim only ever moves a block to a coarser one
    if math.isinf(res.lambda_):
        again = np.array([min(range(NC), key=lambda k: (L[k, b], k)) for b in range(n)])
    else:
        again = np.argmin(W[None, :] * E.astype(np.float64) + res.lambda_ * L.astype(np.float64), axis=0)
    assert int(L[again, ar].sum()) == res.lagrange_bytes and (cand >= again).all(), what
    # (numpy's W E + lambda L is the kernel's arithmetic, rounding for rounding: the library is built with -ffp-contract=off, so no
    #  product is fused into the sum.)  The allocator alone on the fetched tables gives the call's answer
    if res.budget > 0:
        sdrops, sres = c.stage_quality_alloc(L, E, W, DMAX, True, res.budget)
        assert np.array_equal(sdrops, drop), what
        assert (sres.lagrange_bytes, sres.block_bytes, sres.distortion, sres.lambda_, sres.steps) == (res.lagrange_bytes, res.block_bytes, res.distortion, res.lambda_, res.steps), what
    # no uniform drop whose model distortion is <= the Lagrange choice's has fewer bytes
    lag_dist = model_distortion(W, E, again)
    assert lag_dist <= res.budget * (1 + n * 2.0 ** -52), what
    for u in range(NC):
        if model_distortion(W, E, np.full(n, u)) <= lag_dist:
            assert int(L[u].sum()) >= res.lagrange_bytes, (what, u)
    back = c.decode_image_planes(cs) if len(set(p.shape for p in case.planes)) > 1 else list(c.decode_image(cs))
    if R.have_ref():
        for a, b in zip(back, case.ref(cs)):
            assert np.array_equal(np.asarray(a).astype(np.int32), b), what
    return cand, drop, back


KINDS = ["one tile", "2x2 tiles", "ragged", "420", "NV12", "YUY2"]


@pytest.mark.parametrize("irrev", [False, True], ids=["5/3", "9/7"])
@pytest.mark.parametrize("kind", KINDS)
def test_quality_targets(kind, irrev, monkeypatch):
    """50, 40 and 30 dB and D = 0 on one input: every assertion of check_allocation; lagrange_bytes does not rise as the target
    falls; the D = 0 file is the plain host-writer file, byte for byte; a second call gives the same drops; the 5/3 calls that dropped
    anything leave the reversible note.  Printed for 9/7: target, model and decoded PSNR.
    The YUY2 frame (70 x 37 in tiles of 32) has blocks of a few samples with a coarser candidate of EQUAL error in fewer bytes -- in
    the model a lone odd magnitude survives one dropped plane.  The allocator alone takes such a candidate at any budget, 0 included;
    the encode calls therefore answer D = 0 without it, which is what makes the plain file come back here."""
    case = Case(kind, irrev)
    c = case.c
    plain = case.plain_host(monkeypatch)
    plain_blocks = int(G.read_packets(plain)["rows"]["length"].sum())
    runs, report = [], []
    for psnr in TARGETS:
        cs, res = case.call(psnr)
        note = c.last_error()
        cand, drop, back = check_allocation(case, psnr, cs, res)
        assert ("mu >> d" in note) == (not irrev and res.block_bytes < plain_blocks), (kind, psnr, note)
        decoded = synth.psnr_db(np.concatenate([np.asarray(a).reshape(-1) for a in back]), np.concatenate([p.reshape(-1) for p in case.planes]), 8)
        report.append((psnr, round(res.psnr, 2), round(decoded, 2), len(cs), res.steps))
        runs.append((res, drop))
    assert runs[0][0].lagrange_bytes >= runs[1][0].lagrange_bytes >= runs[2][0].lagrange_bytes
    assert runs[0][0].distortion <= runs[1][0].distortion <= runs[2][0].distortion and len(set(runs[2][1].tolist())) > 1
    print("%s %s: plain %d bytes; (target dB, model dB, decoded dB, file bytes, steps) %s" % (kind, "9/7" if irrev else "5/3", len(plain), report))
    # a second call: the same drops
    cs2, res2 = case.call(40.0)
    assert np.array_equal(tables(c)[4], runs[1][1]) and res2.block_bytes == runs[1][0].block_bytes
    # D = 0, as a PSNR of +inf and as a distortion of 0: nothing dropped, the plain file
    for psnr, dist in ((math.inf, 0.0), (0.0, 0.0)):
        cs, res = case.call(psnr, dist)
        assert cs == plain and res.budget == 0 and res.distortion == 0 and res.psnr == math.inf and c.last_error() == "", (kind, psnr)
        assert not tables(c)[4].any() and res.block_bytes == res.lagrange_bytes == plain_blocks and res.file_bytes == len(cs)
        assert c.quality_last_budget() == 0 and c.rate_last_budget() == 0 and res.lambda_ == 0 and res.steps == 0
    # ... which decodes, like every file here, and as the reference decodes it
    back = c.decode_image_planes(cs) if len(set(p.shape for p in case.planes)) > 1 else list(c.decode_image(cs))
    assert irrev or all(np.array_equal(a, b) for a, b in zip(back, case.planes))
    if R.have_ref():
        for a, b in zip(back, case.ref(cs)):
            assert np.array_equal(np.asarray(a).astype(np.int32), b), kind
    # a distortion budget of the caller's, where target_psnr is 0
    cs, res = case.call(0.0, runs[1][0].budget)
    assert res.budget == runs[1][0].budget and np.array_equal(tables(c)[4], runs[1][1])


@pytest.mark.parametrize("irrev", [False, True], ids=["5/3", "9/7"])
def test_packed_file_is_the_surface_calls(irrev):
    """the YUY2 frame's file == grk_amd_encode_surface_quality's for the same samples on an NV16 surface == the sub-sampled call's
    for the same samples as tight planes"""
    packed, surf = Case("YUY2", irrev), Case("NV16", irrev)
    assert all(np.array_equal(a, b) for a, b in zip(packed.planes, surf.planes))
    c = packed.c
    layout = G.ImageLayout.make(70, 37, 32, 32)
    base = G.TileParams.make(1, 1, 3, 8, LEVELS, mct=False, irreversible=irrev, cblk=CBLK)
    for psnr in (40.0, 30.0):
        got, res = packed.call(psnr)
        want, wres = surf.call(psnr)
        assert got == want and (res.block_bytes, res.distortion, res.lambda_, res.steps) == (wres.block_bytes, wres.distortion, wres.lambda_, wres.steps)
        tight, _ = c.encode_image_subsampled_quality(layout, base, S422, packed.planes, psnr, max_drop=DMAX, allow_skip=True)
        assert tight == got


@pytest.mark.parametrize("irrev", [False, True], ids=["5/3", "9/7"])
def test_tiles_quality(irrev):
    """grk_amd_encode_tiles_quality on two 128 x 128 tiles: the allocation of the stage call on the call's own tables at
    grk_amd_quality_last_budget; the rows are the chosen candidates'"""
    c = U.ctx()
    p = G.TileParams.make(128, 128, 3, 8, LEVELS, irreversible=irrev, cblk=CBLK)
    px = np.stack([np.stack(clip(list(synth.g2(3, 128, 128, 8, seed=s)), irrev)) for s in (1, 2)])
    table, tot, res = c.encode_tiles_quality(p, 2, px.ctypes.data, False, 38.0, max_drop=DMAX, allow_skip=True)
    n, L, E, W, drop, cand = tables(c)
    S = 2 * 128 * 128 * 3
    want = S * 255.0 ** 2 * 10 ** -3.8
    assert n == len(table) == 2 * len(G.tile_layout(p)[0]) and abs(res.budget - want) <= 1e-12 * want and c.quality_last_budget() == res.budget
    drops, sres = c.stage_quality_alloc(L, E, W, DMAX, True, res.budget)
    assert np.array_equal(drops, drop) and sres.feasible == 1 and sres.floor == 0
    assert (sres.block_bytes, sres.lagrange_bytes, sres.distortion, sres.lambda_, sres.steps) == (res.block_bytes, res.lagrange_bytes, res.distortion, res.lambda_, res.steps)
    assert np.array_equal(table["length"], L[cand, np.arange(n)]) and res.distortion <= res.budget * (1 + n * 2.0 ** -52) and res.file_bytes == 0
    assert 0 < res.block_bytes < int(L[0].sum()) and len(set(drop.tolist())) > 2
    assert ("mu >> d" in c.last_error()) == (not irrev)


def test_refusals():
    """pipelining on: GRK_AMD_ERR_UNSUPPORTED from every call; a negative or NaN PSNR, a negative or NaN distortion where it is used,
    max_drop 13: GRK_AMD_ERR_INVALID -- all before any work; a plain encode still takes no GRK_AMD_CS_BLOCK_MSBS"""
    layout = G.ImageLayout.make(128, 128)
    p = G.TileParams.make(128, 128, 3, 8, LEVELS, cblk=CBLK)
    base = G.TileParams.make(1, 1, 3, 8, LEVELS, mct=False, cblk=CBLK)
    px = synth.g2(3, 128, 128, 8)
    planes = make_planes(layout, S420, 8, seed=1)
    surface, sampling, nbytes = G.Surface.make("NV12", layout, pitch=128)
    buf = np.zeros(nbytes, np.uint8)
    surface.scatter(buf, planes, 1)
    frame = np.zeros(PR.frame_bytes(PR.YUY2, 128, 128, 0), np.uint8)
    c = G.Context(0)
    calls = (lambda **k: c.encode_tiles_quality(p, 1, px.ctypes.data, False, **k),
             lambda **k: c.encode_image_quality(layout, p, px, **k),
             lambda **k: c.encode_image_subsampled_quality(layout, base, S420, planes, **k),
             lambda **k: c.encode_surface_quality(layout, base, sampling, surface, buf, **k),
             lambda **k: c.encode_packed_quality(layout, base, "YUY2", frame, **k))
    try:
        c.set_pipelining(True)
        for call in calls:
            with pytest.raises(G.RateError) as e:
                call(psnr=40.0)
            assert e.value.code == ERR_UNSUPPORTED and "pipelin" in e.value.reason
        c.set_pipelining(False)
        before = c.surface_counters()
        for call in calls:
            for kw in (dict(psnr=-1.0), dict(psnr=math.nan), dict(psnr=0.0, distortion=-1.0), dict(psnr=0.0, distortion=math.nan),
                       dict(psnr=40.0, max_drop=13)):
                with pytest.raises(G.RateError) as e:
                    call(**kw)
                assert e.value.code == ERR_INVALID, kw
        assert c.surface_counters() == before and c.rate_num_blocks() == 0
        cs, res = calls[1](psnr=40.0)
        assert res.file_bytes == len(cs) and c.rate_num_blocks() > 0
        # a refused call leaves no tables of an earlier call behind, whichever entry point refuses
        for call in calls:
            calls[1](psnr=40.0)
            assert c.rate_num_blocks() > 0
            with pytest.raises(G.RateError):
                call(psnr=-1.0)
            assert c.rate_num_blocks() == 0
        with pytest.raises(RuntimeError, match=str(ERR_UNSUPPORTED)):
            c.encode_image_subsampled(layout, base, S420, planes, G.CS_BLOCK_MSBS)
    finally:
        c.close()
