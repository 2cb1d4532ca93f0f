"""-m gpu: rate-targeted HT encodes.  The block coder's instances that take a per-block drop (grk_amd_stage_ht_encode_drops) against the
oracle's block coder at the reduced exponent bound; the statistics kernel against a numpy restatement; the trial lengths; the
allocator's result against its own tables (grk_amd_rate_tables); whole files of at most N bytes (grk_amd_encode_image_rate) read back
by grk_amd_decode_image and by the reference; the refusals."""
import numpy as np
import pytest
import torch

import grok_amd as G
import gpuutil as U
import oracle as O
import ratemodel as RM
import rateplanes as RP
import refharness as R
import synth
from grok_amd.capi import ERR_OVERFLOW, ERR_UNSUPPORTED
from rateplanes import FORMS, GEOMS

pytestmark = pytest.mark.gpu
SKIP = G.DROP_SKIP
DMAX = 6


# ---- 1. the block coder with drops == the oracle at the exponent bound kmax - d ------------------------------------------------
def planes_case(form, geom, seed, mode_of=None):
    """rateplanes.planes_case: -> (params, blocks, the device planes, planes16, [sign-magnitude words of every block as the d = 0
    coder sees them])"""
    return RP.planes_case(form, geom, seed, mode_of)[:5]


def expected_block(sm, kmax, drop):
    """-> (bytes, missing_msbs): SKIP and a block with d > 0 of which the shift leaves nothing have no bytes; everything else is the
    oracle's block at the exponent bound kmax - d, d clamped to kmax - 1"""
    if drop == SKIP:
        return b"", kmax - 1
    d = min(int(drop), kmax - 1)
    mu = (sm & 0x7FFFFFFF) >> (30 - kmax)
    if d > 0 and not (mu >> d).any():
        return b"", kmax - 1 - d
    return O.ht_encode_sm(sm, kmax - d), kmax - 1 - d


def run_drops(c, p, dev, h16, drops):
    d_drops = U.to_dev(np.asarray(drops, np.uint8))
    c.stage_ht_encode_drops(p, 1, dev.data_ptr(), h16, d_drops.data_ptr())
    table, tot = c.fetch_table(len(drops))
    return table, U.split_blocks(table, c.fetch_coded(tot))


def check_against_oracle(table, got, blocks, sms, drops, what):
    bad = []
    for i, b in enumerate(blocks):
        want, mm = expected_block(sms[i], b.kmax, drops[i])
        if got[i] != want or int(table["missing_msbs"][i]) != mm:
            bad.append((i, b.kmax, int(drops[i]), len(got[i]), len(want), int(table["missing_msbs"][i]), mm))
    assert not bad, "%s: (block, kmax, drop, len gpu, len oracle, msbs gpu, msbs wanted) %s" % (what, bad[:8])


def forced_modes(i):
    # block 2: small magnitudes (nothing left behind d = 3); blocks 3 and 4: all zero
    return {2: ("below", 8), 3: 3, 4: 3}.get(i, [0, 1, 2, 5, "P", 4][i % 6])


def forced_drops(blocks, seed):
    rng = np.random.default_rng(seed)
    drops = rng.choice(list(range(DMAX + 1)) + [SKIP], len(blocks)).astype(np.uint8)
    drops[0] = blocks[0].kmax - 1          # the largest drop there is
    drops[1] = blocks[1].kmax + 5          # clamped to kmax - 1
    drops[2] = 3                           # all zero behind the shift: no bytes
    drops[3] = 0                           # an all-zero block, nothing dropped: the d = 0 coder's bytes
    drops[4] = 2                           # an all-zero block with a drop: no bytes
    return drops


@pytest.mark.parametrize("geom", list(GEOMS))
@pytest.mark.parametrize("form", list(FORMS))
def test_blocks_with_drops_equal_the_oracle(form, geom):
    """Every block's bytes == orc_ht_encode_sm(sm, kmax - d), every row's missing_msbs == kmax - 1 - d, for random drops in
    {0 .. 6, SKIP} and the forced cases (d = kmax - 1, d > kmax - 1, nothing left behind the shift, all-zero blocks).
    One reading had to be chosen: a block with d > 0 whose shifted samples are all zero has NO bytes (include/grok_amd.h says so: such a block costs a rate-targeted file nothing), not the
    few bytes the oracle writes for an all-zero block -- expected_block says so; with d = 0 an all-zero block keeps those bytes."""
    p, blocks, dev, h16, sms = planes_case(form, geom, [len(form), len(geom)], forced_modes)
    assert len(blocks) >= 7
    drops = forced_drops(blocks, 5)
    table, got = run_drops(U.ctx(), p, dev, h16, drops)
    check_against_oracle(table, got, blocks, sms, drops, "%s, %s" % (form, geom))
    assert got[2] == b"" and got[4] == b"" and len(got[3]) > 0 and len(got[0]) > 0
    assert {SKIP} | set(range(DMAX + 1)) <= set(int(d) for d in drops) or len(blocks) < 40
    # d = 0 everywhere: the bytes of the plain stage
    zero = np.zeros(len(blocks), np.uint8)
    t0, g0 = run_drops(U.ctx(), p, dev, h16, zero)
    c = U.ctx()
    (c.stage_ht_encode16(p, 1, dev.data_ptr()) if h16 else c.stage_ht_encode(p, 1, dev.data_ptr()))
    tp, tot = c.fetch_table(len(blocks))
    assert g0 == U.split_blocks(tp, c.fetch_coded(tot)) and np.array_equal(t0["missing_msbs"], tp["missing_msbs"])


@pytest.mark.parametrize("form", list(FORMS))
def test_blocks_with_drops_worst_case_lds_and_fallback(form, monkeypatch):
    """GRK_AMD_LDS_CAP=0 (worst-case buffers, no fallback) and, with the cap on, dense content at the top of the range that outgrows
    the capped raw streams: the fallback launch of the drop instances codes it -- the same bytes either way, the oracle's."""
    handed = {}
    for cap in ("0", "1"):
        monkeypatch.setenv("GRK_AMD_LDS_CAP", cap)
        c = G.Context(0)
        try:
            p, blocks, dev, h16, sms = planes_case(form, "cblk 64", 9, lambda i: 4 if i % 2 else 0)
            drops = np.array([i % 2 for i in range(len(blocks))], np.uint8)        # d in {0, 1}: the streams stay long
            table, got = run_drops(c, p, dev, h16, drops)
            check_against_oracle(table, got, blocks, sms, drops, "%s, GRK_AMD_LDS_CAP=%s" % (form, cap))
            handed[cap] = int(U.from_dev_ptr(c.table_device_ptr(3), 24 * 8).view("<u8").sum())
        finally:
            c.close()
    print("blocks handed to the fallback launch of the drop instances (%s): %s" % (form, handed))
    assert handed["0"] == 0 and handed["1"] > 0


# ---- 2 - 4. statistics, lengths, allocation ----------------------------------------------------------------------------------------
_rate_cache = {}


def rate_run(irrev, budget_div, skip=True, dmax=DMAX):
    """256 x 256 x 3, 8 bits, 3 levels, code-blocks of 32: one rate-targeted encode of the tile at 1 / budget_div of the plain blocks'
    bytes -> everything the checks below need (computed once per case)"""
    key = (irrev, budget_div, skip, dmax)
    if key in _rate_cache:
        return _rate_cache[key]
    c = U.ctx()
    p = G.TileParams.make(256, 256, 3, 8, 3, irreversible=irrev, cblk=(5, 5))
    px = synth.g2(3, 256, 256, 8)
    blocks, _ = G.tile_layout(p)
    n = len(blocks)
    plain, _ = c.encode_host(p, px)
    budget = int(plain["length"].sum()) // budget_div
    table, tot, res = c.encode_tiles_rate(p, 1, px.ctypes.data, False, budget, dmax, skip)
    note = c.last_error()
    coded = c.fetch_coded(tot)
    L, E, W, drop = c.rate_tables(n, dmax)
    h16 = c.plane_sample_bytes(p)[0] == 2
    stride, elems = G.lib().grk_amd_plane_stride(p), G.lib().grk_amd_plane_elems(p)
    raw = U.from_dev_ptr(c.plane_device_ptr(1), 3 * elems * (2 if h16 else 4))
    planes = raw.view(np.int16 if h16 else np.float32 if irrev else np.int32).reshape(3, -1)[:, :256 * stride].reshape(3, 256, stride)[:, :, :256]
    out = dict(p=p, blocks=blocks, plain=plain, budget=budget, table=table, coded=coded, res=res, L=L, E=E, W=W, drop=drop, planes=planes.copy(), h16=h16, note=note)
    _rate_cache[key] = out
    return out


def quantised(r, b):
    """the magnitudes the d = 0 coder codes for block b (ratemodel.quantised)"""
    sub = r["planes"][b.comp, b.py:b.py + b.y1 - b.y0, b.px:b.px + b.x1 - b.x0]
    return RM.quantised(sub, b.kmax, b.stepsize, bool(r["p"].irreversible))


def restated_errors(r, dmax):
    """E as include/grok_amd.h defines it (ratemodel.errors): c taken as min(c, kmax - 1), the drop the coder clamps to"""
    want = np.zeros_like(r["E"])
    for i, b in enumerate(r["blocks"]):
        want[:, i] = RM.errors(quantised(r, b), b.kmax, dmax)
    return want


@pytest.mark.parametrize("irrev", [False, True], ids=["5/3", "9/7"])
def test_statistics_equal_the_formula(irrev):
    """E[c][b] == sum over the block of (2 q - 2 r_c(q))^2, r_c(q) = q (c = 0); 0 where q >> c == 0 and for SKIP; else
    ((q >> c) << c) + 2^(c - 1) -- exactly (every band of this tile has kmax - 1 > Dmax = 6: the clamp of c plays no part);
    W == (w_mct * w_band * stepsize)^2 / 4 of grk_amd_block_distortion"""
    r = rate_run(irrev, 4)
    assert r["h16"] == (not irrev)                               # (8-bit reversible content: the int16 planes)
    assert min(b.kmax for b in r["blocks"]) - 1 > DMAX
    want = restated_errors(r, DMAX)
    assert np.array_equal(r["E"], want)
    assert want[1:].any(axis=1).all()
    assert ("mu >> d" in r["note"]) == (not irrev)               # the note a reversible call that dropped planes leaves
    c = U.ctx()
    c.encode_host(r["p"], synth.g2(3, 256, 256, 8))
    dist = c.block_distortion(len(r["blocks"]))                  # w^2 * sum q^2 = W * E[SKIP]
    assert np.allclose(r["W"] * r["E"][DMAX + 1].astype(np.float64), dist, rtol=1e-12, atol=0)


def test_statistics_of_candidates_beyond_the_coders_clamp():
    """Dmax = 12 on 8-bit content: bands with kmax - 1 < 12.  The coder clamps d to kmax - 1, so rows c >= kmax - 1 of L are the row
    kmax - 1 -- and so are the rows of E: a row describes the block as coded"""
    r = rate_run(False, 4, True, 12)
    top = np.array([b.kmax - 1 for b in r["blocks"]])
    assert top.min() < 12 and len(set(top)) > 1
    assert np.array_equal(r["E"], restated_errors(r, 12))
    ar = np.arange(len(top))
    for c in range(13):
        assert np.array_equal(r["L"][c], r["L"][np.minimum(c, top), ar]) and np.array_equal(r["E"][c], r["E"][np.minimum(c, top), ar]), c
    assert r["res"].block_bytes <= r["budget"]


@pytest.mark.parametrize("irrev", [False, True], ids=["5/3", "9/7"])
def test_lengths_are_the_trial_launches(irrev):
    """L[c] == the lengths of the drop instances with d = c everywhere on the same planes; L[SKIP] == 0; L[0] == the plain encode's"""
    r = rate_run(irrev, 4)
    c, n = U.ctx(), len(r["blocks"])
    planes = r["planes"] if not irrev else r["planes"].view(np.int32)
    dev = U.upload_planes16(planes, r["p"]) if r["h16"] else U.upload_planes(planes.astype(np.int32), r["p"])
    for d in range(DMAX + 1):
        d_drops = U.to_dev(np.full(n, d, np.uint8))
        c.stage_ht_encode_drops(r["p"], 1, dev.data_ptr(), r["h16"], d_drops.data_ptr())
        table, _ = c.fetch_table(n)
        assert np.array_equal(r["L"][d], table["length"]), d
        assert np.array_equal(table["missing_msbs"], [b.kmax - 1 - min(d, b.kmax - 1) for b in r["blocks"]])
    assert not r["L"][DMAX + 1].any() and np.array_equal(r["L"][0], r["plain"]["length"])
    assert (r["L"][:DMAX + 1].sum(axis=1)[1:] < r["L"][:DMAX + 1].sum(axis=1)[:-1]).all()      # totals fall as d rises


@pytest.mark.parametrize("skip", [True, False], ids=["skip", "noskip"])
@pytest.mark.parametrize("irrev", [False, True], ids=["5/3", "9/7"])
def test_allocation_against_its_tables(irrev, skip):
    runs = [rate_run(irrev, div, skip) for div in (10, 4, 2)]
    for r in runs:
        L, E, W, drop, res, budget = r["L"].astype(np.int64), r["E"], r["W"], r["drop"], r["res"], r["budget"]
        n = len(drop)
        cand = np.where(drop == SKIP, DMAX + 1, drop).astype(np.int64)
        assert skip or not (drop == SKIP).any()
        ar = np.arange(n)
        bytes_ = int(L[cand, ar].sum())
        dist = float((W * E[cand, ar].astype(np.float64)).sum())
        print("budget %d: blocks %d, lagrange %d, distortion %.6g, lambda %.6g, drops %s" % (
            budget, res.block_bytes, res.lagrange_bytes, res.distortion, res.lambda_, np.bincount(cand, minlength=DMAX + 2).tolist()))
        assert res.block_bytes <= budget and res.lagrange_bytes <= res.block_bytes
        assert res.block_bytes == bytes_ == int(r["table"]["length"].sum())
        assert abs(res.distortion - dist) <= 1e-9 * dist
        # the rows of the final launch are those candidates
        assert np.array_equal(r["table"]["length"], L[cand, ar])
        assert np.array_equal(r["table"]["missing_msbs"], [b.kmax - 1 if d == SKIP else b.kmax - 1 - min(int(d), b.kmax - 1) for b, d in zip(r["blocks"], drop)])
        # nothing left to spend: no block's next finer candidate lowers W E and fits the slack
        slack = budget - bytes_
        finer = np.maximum(cand - 1, 0)
        could = (cand > 0) & (E[finer, ar] < E[cand, ar]) & (L[finer, ar] - L[cand, ar] <= slack)
        assert not could.any(), np.flatnonzero(could)[:8]
        # no uniform drop within the Lagrange solution's bytes does better
        for c in range(DMAX + 2 if skip else DMAX + 1):
            if L[c].sum() <= res.lagrange_bytes:
                assert (W * E[c].astype(np.float64)).sum() >= dist * (1 - 1e-9), c
    assert [r["res"].block_bytes for r in runs] == sorted(r["res"].block_bytes for r in runs)
    assert [r["res"].distortion for r in runs] == sorted((r["res"].distortion for r in runs), reverse=True)
    # a second run: the same drops
    r = runs[1]
    c = U.ctx()
    px = synth.g2(3, 256, 256, 8)
    c.encode_tiles_rate(r["p"], 1, px.ctypes.data, False, r["budget"], DMAX, skip)
    assert np.array_equal(c.rate_tables(len(r["drop"]), DMAX)[3], r["drop"])


# ---- 5. whole files -------------------------------------------------------------------------------------------------------------
needs_ref = pytest.mark.skipif(not R.have_ref(), reason="oracle/_ref (the real reference) not built here")
# tiling -> (W, H, tile w, tile h); "ragged": 2 x 2 tiles of four sizes -- four geometry groups, each with its own tables and share
TILINGS = {"one tile": (256, 256, 256, 256), "2x2 tiles": (256, 256, 128, 128), "ragged": (250, 190, 128, 96)}
TARGETS = (("2x", 2, 1), ("1/2", 1, 2), ("1/4", 1, 4), ("1/10", 1, 10))
_files = {}


def rate_files(irrev, tiling):
    """-> (source pixels, the plain host-writer file, {target name: (target, file, result, note)}), made once per case"""
    key = (irrev, tiling)
    if key not in _files:
        import os
        c = U.ctx()
        W, H, TW, TH = TILINGS[tiling]
        px = synth.g2(3, H, W, 8)
        layout = G.ImageLayout.make(W, H, TW, TH)
        base = G.TileParams.make(TW, TH, 3, 8, 3, irreversible=irrev)
        keep = os.environ.get("GRK_AMD_IMAGE_T2")
        os.environ["GRK_AMD_IMAGE_T2"] = "host"
        try:
            plain = c.encode_image(layout, base, px)
        finally:
            if keep is None:
                del os.environ["GRK_AMD_IMAGE_T2"]
            else:
                os.environ["GRK_AMD_IMAGE_T2"] = keep
        out = {}
        for name, mul, div in TARGETS:
            target = len(plain) * mul // div
            cs, res = c.encode_image_rate(layout, base, px, target, max_drop=DMAX, allow_skip=True)
            out[name] = (target, cs, res, c.last_error())
        _files[key] = (px, layout, base, plain, out)
    return _files[key]


@pytest.mark.parametrize("tiling", list(TILINGS))
@pytest.mark.parametrize("irrev", [False, True], ids=["5/3", "9/7"])
def test_files_of_at_most_n_bytes(irrev, tiling):
    """3 components, 8 bits: targets of 2 x the plain file's size and 1/2, 1/4, 1/10 of it.  Every file is at most its target; the
    2 x file is the plain one byte for byte -- also where the tiles fall into several geometry groups ("ragged"), each of which gets
    its share of the budget: at or above the plain size every group's share is its own plain bytes.  PSNR of grk_amd_decode_image
    against the source is printed, not asserted (DESIGN.md section 3 has the figures of an MI355X).  In the REVERSIBLE files both
    decoders return a block with d planes dropped as mu >> d (tests/test_rate_writer_cpu.py pins why): their PSNR says so, and so
    does the note the call leaves in grk_amd_last_error."""
    c = U.ctx()
    px, layout, base, plain, files = rate_files(irrev, tiling)
    if tiling == "ragged":
        groups = []
        for p in G.layout_tiles(layout, base):
            if not any(G.same_tile_geometry(g, p) for g in groups):
                groups.append(p)
        assert len(groups) == 4
    psnr = {}
    for name, (target, cs, res, note) in files.items():
        assert len(cs) <= target and res.file_bytes == len(cs) and 1 <= res.passes <= 4
        if name == "2x":
            assert cs == plain and res.passes == 1 and note == ""
        else:
            assert ("mu >> d" in note) == (not irrev)
        psnr[name] = (len(cs), res.passes, round(float(synth.psnr_db(c.decode_image(cs), px, 8)), 2))
    print("%s, %s: plain %d bytes; target -> (file bytes, rounds, PSNR dB) %s" % ("9/7" if irrev else "5/3", tiling, len(plain), psnr))
    if not irrev:
        assert np.array_equal(c.decode_image(plain), px)
    with pytest.raises(G.RateError) as e:
        c.encode_image_rate(layout, base, px, 200, max_drop=DMAX, allow_skip=False)
    assert e.value.code == ERR_OVERFLOW and "bytes" in e.value.reason
    with pytest.raises(G.RateError) as e:                            # below the headers alone, SKIP allowed
        c.encode_image_rate(layout, base, px, 60, max_drop=DMAX, allow_skip=True)
    assert e.value.code == ERR_OVERFLOW and "no byte of any block" in e.value.reason


@needs_ref
@pytest.mark.parametrize("tiling", list(TILINGS))
@pytest.mark.parametrize("irrev", [False, True], ids=["5/3", "9/7"])
def test_files_decode_as_the_reference_decodes_them(irrev, tiling):
    """grk_amd_decode_image of every such file == the reference's decode, exactly (what tests/test_gpu_decode_image.py asks of 9/7
    streams)"""
    c = U.ctx()
    px, layout, base, plain, files = rate_files(irrev, tiling)
    H, W = px.shape[1:]
    for name, (target, cs, res, note) in files.items():
        assert np.array_equal(c.decode_image(cs).astype(np.int32), R.decode(cs, 3, H, W)), name


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals():
    px = synth.g2(3, 128, 128, 8)
    p = G.TileParams.make(128, 128, 3, 8, 2)
    layout = G.ImageLayout.make(128, 128, 128, 128)
    c = G.Context(0)
    try:
        c.set_pipelining(True)
        with pytest.raises(G.RateError) as e:
            c.encode_tiles_rate(p, 1, px.ctypes.data, False, 10000)
        assert e.value.code == ERR_UNSUPPORTED
        with pytest.raises(G.RateError) as e:
            c.encode_image_rate(layout, p, px, 10000)
        assert e.value.code == ERR_UNSUPPORTED
        c.set_pipelining(False)
        table, tot, res = c.encode_tiles_rate(p, 1, px.ctypes.data, False, 10000)
        assert res.block_bytes <= 10000
        # Tier-2 on the device does not take per-block zero bit-planes
        with pytest.raises(RuntimeError, match=str(ERR_UNSUPPORTED)):
            c.assemble_device(p, [0], G.CS_BLOCK_MSBS)
        assert c.assemble_device(p, [0], 0)[0] > 0
        # no encode of sub-sampled components drops bit-planes
        planes = [px[0], px[1][::2, ::2], px[2][::2, ::2]]
        with pytest.raises(RuntimeError, match=str(ERR_UNSUPPORTED)):
            c.encode_image_subsampled(layout, G.TileParams.make(128, 128, 3, 8, 2, mct=False), [(1, 1), (2, 2), (2, 2)], planes, G.CS_BLOCK_MSBS)
        with pytest.raises(G.RateError) as e:
            c.encode_tiles_rate(p, 1, px.ctypes.data, False, 10000, max_drop=13)
        assert e.value.code != 0
    finally:
        c.close()
