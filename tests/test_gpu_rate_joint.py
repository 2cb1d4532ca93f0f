"""-m gpu: rate-targeted encodes over JOINT tables -- sub-sampled images (grk_amd_encode_image_subsampled_rate), video surfaces
(grk_amd_encode_surface_rate) and grk_amd_rate::joint = 1 on grk_amd_encode_image_rate.  The joint tables' columns against the tables
of each unit coded alone (grk_amd_encode_tiles_rate); the allocation against the joint tables, one multiplier over all units
restated in numpy; files of at most N bytes, read back by grk_amd_decode_image and -- where oracle/_ref is built -- by the reference;
surfaces against the same samples as tight planes, in place and staged; the joint route beside the split one; the refusals.
Dmax 6 plus SKIP and synth.g2 content throughout; the sub-sampled images carry no colour transform."""
import numpy as np
import pytest

import grok_amd as G
import gpuutil as U
import refharness as R
import synth
from grok_amd.capi import ERR_OVERFLOW, ERR_UNSUPPORTED
from test_t2_reader_subsampled_cpu import make_planes, num_tiles, tile_comp

pytestmark = pytest.mark.gpu
SKIP = G.DROP_SKIP
DMAX = 6
S420 = [(1, 1), (2, 2), (2, 2)]
S422 = [(1, 1), (2, 1), (2, 1)]
S420A = [(1, 1), (2, 2), (2, 2), (1, 1)]


def runs_of(sampling):
    """consecutive components of equal factors -> [(first, count)]"""
    out, c0 = [], 0
    while c0 < len(sampling):
        n = 1
        while c0 + n < len(sampling) and sampling[c0 + n] == sampling[c0]:
            n += 1
        out.append((c0, n))
        c0 += n
    return out


def units_of(layout, base, sampling, planes):
    """the units in joint order -- tile by tile, run by run -> [(params of the unit, its pixels component-major)]"""
    out = []
    for t in range(num_tiles(layout)):
        for c0, n in runs_of(sampling):
            p = tile_comp(layout, base, *sampling[c0], t)
            crop = [np.ascontiguousarray(planes[c0 + k][p.tile_y0 - layout.y0 // sampling[c0][1]:, p.tile_x0 - layout.x0 // sampling[c0][0]:]
                                         [:p.tile_h, :p.tile_w]) for k in range(n)]
            p.num_comps, p.mct = n, 0
            out.append((p, np.stack(crop)))
    return out


def joint_tables(c):
    n = c.rate_num_blocks()
    return (n, c.rate_unit_rows()) + tuple(c.rate_tables(n, DMAX))


# ---- 3. the joint tables' columns == the tables of every unit alone ------------------------------------------------------------------
@pytest.mark.parametrize("irrev", [False, True], ids=["5/3", "9/7"])
@pytest.mark.parametrize("size,tile", [((128, 128), None), ((250, 190), (128, 96)), ((256, 256), (128, 128))],
                         ids=["128-one-tile", "250x190-in-128x96", "256-in-128"])
def test_joint_columns_equal_the_single_batch_tables(size, tile, irrev):
    """4:2:0, 2 levels.  The rows of every unit in the joint L, E, W equal, exactly, the tables of grk_amd_encode_tiles_rate on that
    unit alone: the Y plane of the tile, the two-component CbCr batch.  250 x 190 in tiles of 128 x 96: eight units of eight
    geometries, each a batch of its own; 256 x 256 in tiles of 128: two batches of four units that alternate in joint order -- where a
    wrong map shows."""
    c = U.ctx()
    layout = G.ImageLayout.make(*size, *(tile or (None, None)))
    base = G.TileParams.make(1, 1, 3, 8, 2, mct=False, irreversible=irrev)
    planes = make_planes(layout, S420, 8, seed=7)
    plain = c.encode_image_subsampled(layout, base, S420, planes)
    cs, res = c.encode_image_subsampled_rate(layout, base, S420, planes, len(plain) // 3, max_drop=DMAX, allow_skip=True)
    n, first, L, E, W, drop = joint_tables(c)
    units = units_of(layout, base, S420, planes)
    assert len(first) == len(units) == 2 * num_tiles(layout) and first[0] == 0
    at = 0
    for u, (p, px) in enumerate(units):
        nb = len(G.tile_layout(p)[0])
        assert int(first[u]) == at, u                                     # unit after unit, the writer's order
        c.encode_tiles_rate(p, 1, px.ctypes.data, False, 1 << 30, DMAX, True)
        Lu, Eu, Wu, _ = c.rate_tables(nb, DMAX)
        assert np.array_equal(L[:, at:at + nb], Lu), ("L", u)
        assert np.array_equal(E[:, at:at + nb], Eu), ("E", u)
        assert np.array_equal(W[at:at + nb], Wu), ("W", u)
        at += nb
    assert at == n and L[:DMAX + 1].any(axis=1).all() and not L[DMAX + 1].any()


# ---- 4. the allocation against the joint tables ------------------------------------------------------------------------------------
@pytest.mark.parametrize("irrev", [False, True], ids=["5/3", "9/7"])
def test_allocation_against_the_joint_tables(irrev):
    """4:2:0, 250 x 190 in tiles of 128 x 96, at 1/2, 1/4 and 1/10 of the plain blocks' bytes (the file's target: that plus what the
    plain file spends beside its blocks): what tests/test_gpu_rate.py::test_allocation_against_its_tables asserts, on the joint tables,
    and ONE slope -- argmin_c W E + lambda L with the reported lambda, recomputed here over all units together."""
    c = U.ctx()
    layout = G.ImageLayout.make(250, 190, 128, 96)
    base = G.TileParams.make(1, 1, 3, 8, 2, mct=False, irreversible=irrev)
    planes = make_planes(layout, S420, 8, seed=11)
    plain = c.encode_image_subsampled(layout, base, S420, planes)
    plain_blocks = int(G.read_packets(plain)["rows"]["length"].sum())
    kmax = np.concatenate([[b.kmax for b in G.tile_layout(tile_comp(layout, base, dx, dy, t))[0]] for t in range(4) for dx, dy in S420])
    runs = []
    for div in (10, 4, 2):
        target = len(plain) - plain_blocks + plain_blocks // div
        cs, res = c.encode_image_subsampled_rate(layout, base, S420, planes, target, max_drop=DMAX, allow_skip=True)
        n, first, L, E, W, drop = joint_tables(c)
        budget = c.rate_last_budget()
        L = L.astype(np.int64)
        assert n == len(kmax) and len(cs) <= target and budget <= plain_blocks // div and (res.passes > 1 or budget == plain_blocks // div)
        cand = np.where(drop == SKIP, DMAX + 1, drop).astype(np.int64)
        ar = np.arange(n)
        bytes_ = int(L[cand, ar].sum())
        dist = float((W * E[cand, ar].astype(np.float64)).sum())
        print("1/%d: target %d, budget %d, file %d, blocks %d, lagrange %d, rounds %d, lambda %.6g, drops %s" % (
            div, target, budget, len(cs), res.block_bytes, res.lagrange_bytes, res.passes, res.lambda_, np.bincount(cand, minlength=DMAX + 2).tolist()))
        # within the budget; the result's bytes are the chosen candidates'
        assert res.block_bytes <= budget and res.lagrange_bytes <= res.block_bytes
        assert res.block_bytes == bytes_ and abs(res.distortion - dist) <= 1e-9 * dist
        # the file's rows are those candidates
        rows = G.read_packets(cs)["rows"]
        assert np.array_equal(rows["length"], L[cand, ar])
        assert np.array_equal(rows["missing_msbs"], [k - 1 if d == SKIP else k - 1 - min(int(d), k - 1) for k, d in zip(kmax, drop)])
        # nothing left to spend: no block's next finer candidate lowers W E and fits the slack
        slack = budget - bytes_
        finer = np.maximum(cand - 1, 0)
        could = (cand > 0) & (E[finer, ar] < E[cand, ar]) & (L[finer, ar] - L[cand, ar] <= slack)
        assert not could.any(), np.flatnonzero(could)[:8]
        # one slope over all units: the Lagrange solution restated (ties: the finer candidate, argmin's first), its bytes, and the
        # fill only ever moves a block to a finer candidate
        cost = W[None, :] * E.astype(np.float64) + res.lambda_ * L.astype(np.float64)
        again = np.argmin(cost, axis=0)
        assert res.lambda_ > 0 and int(L[again, ar].sum()) == res.lagrange_bytes
        assert (cand <= again).all()
        assert len(set(again[int(first[0]):int(first[1])])) > 1 or len(set(again)) > 1
        runs.append((res, drop, target))
    assert [r[0].block_bytes for r in runs] == sorted(r[0].block_bytes for r in runs)
    assert [r[0].distortion for r in runs] == sorted((r[0].distortion for r in runs), reverse=True)
    # a second run: the same drop bytes
    c.encode_image_subsampled_rate(layout, base, S420, planes, runs[1][2], max_drop=DMAX, allow_skip=True)
    assert np.array_equal(joint_tables(c)[5], runs[1][1])


# ---- 5. files of at most N bytes -----------------------------------------------------------------------------------------------------
SAMPLINGS = {"420": S420, "422": S422, "420+full": S420A}
TILINGS = {"one tile": (256, 256, 256, 256), "2x2 tiles": (256, 256, 128, 128), "ragged": (250, 190, 128, 96)}
TARGETS = (("2x", 2, 1), ("1/2", 1, 2), ("1/4", 1, 4), ("1/10", 1, 10))


@pytest.mark.parametrize("tiling", list(TILINGS))
@pytest.mark.parametrize("irrev", [False, True], ids=["5/3", "9/7"])
@pytest.mark.parametrize("samp", list(SAMPLINGS))
def test_files_of_at_most_n_bytes(samp, irrev, tiling):
    """Targets of 2 x the plain grk_amd_encode_image_subsampled file and 1/2, 1/4, 1/10 of it: every file is at most its target in at
    most four rounds; the 2 x file is the plain one byte for byte in one round; the note in grk_amd_last_error appears exactly on
    reversible files that dropped something.  PSNR per plane of grk_amd_decode_image against the source is printed, not asserted
    (DESIGN.md section 3 has an MI355X's figures); where oracle/_ref is built the planes equal the reference's decode exactly.
    Content: synth.g2 per plane for 5/3; for 9/7 the same clipped as synth.g2_mid clips it.  Without a colour transform the PLAIN 9/7
    file of full-range g2 planes -- grk_amd_encode_image_subsampled's, nothing dropped -- holds an LL block that needs all Kmax
    bit-planes, which the reference's HT decoder and this library's refuse (defect D5, synth.g2_mid; measured on an MI355X: the plain
    file of every sampling and tiling here is refused with "U_q > missing_msbs", the clipped ones and all their targets decode),
    so no file of that content could be compared."""
    c = U.ctx()
    sampling = SAMPLINGS[samp]
    W, H, TW, TH = TILINGS[tiling]
    layout = G.ImageLayout.make(W, H, TW, TH)
    base = G.TileParams.make(1, 1, len(sampling), 8, 3, mct=False, irreversible=irrev)
    planes = make_planes(layout, sampling, 8, seed=3)
    if irrev:
        planes = [np.clip(pl, 32, 224).astype(pl.dtype) for pl in planes]
    plain = c.encode_image_subsampled(layout, base, sampling, planes)
    report = {}
    for name, mul, div in TARGETS:
        target = len(plain) * mul // div
        cs, res = c.encode_image_subsampled_rate(layout, base, sampling, planes, target, max_drop=DMAX, allow_skip=True)
        note = c.last_error()
        assert len(cs) <= target and res.file_bytes == len(cs) and 1 <= res.passes <= 4, (name, len(cs), target, res.passes)
        if name == "2x":
            assert cs == plain and res.passes == 1 and note == ""
        else:
            assert ("mu >> d" in note) == (not irrev), (name, note)
        back = c.decode_image_planes(cs)
        report[name] = (len(cs), res.passes, [round(float(synth.psnr_db(a, b, 8)), 2) for a, b in zip(back, planes)])
        if R.have_ref():
            for a, b in zip(back, R.decode_planes(cs, sampling, W, H)):
                assert np.array_equal(a.astype(np.int32), b), name
    print("%s %s, %s: plain %d bytes; target -> (file bytes, rounds, PSNR dB per plane) %s" % (samp, "9/7" if irrev else "5/3", tiling, len(plain), report))


# ---- 6. surfaces -------------------------------------------------------------------------------------------------------------------
FORMATS = {"NV12": 8, "I420": 8, "P010": 10, "NV21": 8}
SURFACE_TILINGS = {"one tile": (250, 190, None), "2x2 tiles": (250, 190, (128, 96)), "one tile 256": (256, 192, None)}


def delta(c, call):
    before = c.surface_counters()
    out = call()
    return out, tuple(a - b for a, b in zip(c.surface_counters(), before))


@pytest.mark.parametrize("tiling", list(SURFACE_TILINGS))
@pytest.mark.parametrize("fmt", list(FORMATS))
def test_surfaces(fmt, tiling, monkeypatch):
    """A surface with pitches wider than a row, in host and in device memory, 5/3 and 9/7: grk_amd_encode_surface_rate's file ==
    grk_amd_encode_image_subsampled_rate's for the same samples as tight planes and the same target, byte for byte (2 x the plain
    file: grk_amd_encode_surface's own), also with GRK_AMD_SURFACE_DIRECT=0 -- in place or staged, the same bytes; the counters show
    in-place units where grk_amd_encode_surface has them; grk_amd_decode_surface of the 9/7 file onto a poisoned surface writes
    samples and nothing else (PSNR printed)."""
    c, rng = U.ctx(), np.random.default_rng(len(fmt) + len(tiling))
    W, H, tile = SURFACE_TILINGS[tiling]
    prec = FORMATS[fmt]
    bps = (prec + 7) // 8
    layout = G.ImageLayout.make(W, H, *(tile or (None, None)))
    surface, sampling, nbytes = G.Surface.make(fmt, layout, pitch=bps * W + 14)
    assert sampling == S420 and (prec == 8 or surface.comp[0].shift == 6)
    planes = make_planes(layout, sampling, prec, seed=5)
    if prec > 8:        # (the middle of the range: a 9/7 file whose darkest LL block a decoder takes -- tests/test_gpu_surface_msb.py)
        planes = [np.clip(pl, (1 << prec) // 8, 7 * (1 << prec) // 8).astype(pl.dtype) for pl in planes]
    assert any(pl.shape[1] % 2 for pl in planes[1:]) or W % 4 == 0
    buf = rng.integers(0, 256, nbytes, dtype=np.uint8)
    surface.scatter(buf, planes, bps)
    d_buf = U.to_dev(buf)
    in_place = set()
    for irrev in (False, True):
        base = G.TileParams.make(1, 1, 3, prec, 2, mct=False, irreversible=irrev)
        plain, d_plain = delta(c, lambda: c.encode_surface(layout, base, sampling, surface, buf))
        assert plain == c.encode_image_subsampled(layout, base, sampling, planes)
        in_place.add(d_plain[0])
        for mul, div in ((2, 1), (1, 4)):
            target = len(plain) * mul // div
            want, wres = c.encode_image_subsampled_rate(layout, base, sampling, planes, target, max_drop=DMAX, allow_skip=True)
            assert len(want) <= target and (div > 1 or want == plain)
            for where, ptr, cap in (("host", buf, None), ("device", d_buf.data_ptr(), nbytes)):
                (got, res), d = delta(c, lambda: c.encode_surface_rate(layout, base, sampling, surface, ptr, target, cap=cap, max_drop=DMAX,
                                                                       allow_skip=True))
                assert got == want, (fmt, tiling, irrev, div, where)
                assert (res.block_bytes, res.passes, res.lambda_) == (wres.block_bytes, wres.passes, wres.lambda_)
                assert d[:2] == d_plain[:2] and d[2] >= d_plain[2], (d, d_plain)           # a unit counts once per call
                if div > 1:
                    monkeypatch.setenv("GRK_AMD_SURFACE_DIRECT", "0")
                    (staged, _), ds = delta(c, lambda: c.encode_surface_rate(layout, base, sampling, surface, ptr, target, cap=cap,
                                                                             max_drop=DMAX, allow_skip=True))
                    monkeypatch.delenv("GRK_AMD_SURFACE_DIRECT")
                    assert staged == want and ds[0] == 0 and ds[1] == sum(d_plain[:2]), (fmt, tiling, irrev, div, where, ds)
            assert np.array_equal(d_buf.cpu().numpy(), buf)                                # an encode only reads
        if irrev:
            back = c.decode_image_planes(want)
            before = np.full(nbytes, 0xA5, np.uint8)
            expect = before.copy()
            surface.scatter(expect, back, bps)
            host = before.copy()
            c.decode_surface(want, surface, host)
            assert np.array_equal(host, expect), "host: a byte that is no sample changed"
            dev = U.to_dev(before)
            c.decode_surface(want, surface, dev.data_ptr(), cap=nbytes)
            c.decode_status()
            assert np.array_equal(dev.cpu().numpy(), expect), "device"
            print("%s, %s, 9/7 at 1/4 (%d of %d bytes): PSNR dB per plane %s" % (
                fmt, tiling, len(want), len(plain), [round(float(synth.psnr_db(a, b, prec)), 2) for a, b in zip(back, planes)]))
    if tile is None and prec == 8:          # (one tile, no shift: at least the Y plane is read where it lies)
        assert min(in_place) > 0, "no unit of a one-tile %s surface was coded in place" % fmt
    else:
        assert in_place == {0}


# ---- 7. grk_amd_rate::joint on grk_amd_encode_image_rate ------------------------------------------------------------------------------
@pytest.mark.parametrize("irrev", [False, True], ids=["5/3", "9/7"])
def test_joint_on_encode_image_rate(irrev, monkeypatch):
    """250 x 190 x 3 in tiles of 128 x 96: four geometry groups.  joint = 1: files within their targets, the 2 x file the plain
    host-writer file; joint = 0 in the same process still meets its targets.  Both routes' distortion and PSNR are printed side by
    side, not asserted: a Lagrangian solution plus a greedy fill carries no strict guarantee against a lucky split."""
    c = U.ctx()
    W, H = 250, 190
    px = synth.g2(3, H, W, 8)
    layout = G.ImageLayout.make(W, H, 128, 96)
    base = G.TileParams.make(128, 96, 3, 8, 3, irreversible=irrev)
    monkeypatch.setenv("GRK_AMD_IMAGE_T2", "host")
    plain = c.encode_image(layout, base, px)
    monkeypatch.delenv("GRK_AMD_IMAGE_T2")
    for name, mul, div in (("2x", 2, 1), ("1/2", 1, 2), ("1/4", 1, 4), ("1/10", 1, 10)):
        target = len(plain) * mul // div
        out = {}
        for joint in (1, 0):
            cs, res = c.encode_image_rate(layout, base, px, target, max_drop=DMAX, allow_skip=True, joint=joint)
            note = c.last_error()
            assert len(cs) <= target and res.file_bytes == len(cs) and 1 <= res.passes <= 4, (name, joint)
            if name == "2x":
                assert cs == plain and res.passes == 1 and note == ""
            else:
                assert ("mu >> d" in note) == (not irrev)
            if joint:
                n, first = c.rate_num_blocks(), c.rate_unit_rows()
                assert len(first) == 4 and n == sum(len(G.tile_layout(p)[0]) for p in G.layout_tiles(layout, base))
            out[joint] = (len(cs), res.passes, res.distortion, round(float(synth.psnr_db(c.decode_image(cs), px, 8)), 2))
        print("%s %s (target %d): joint (bytes, rounds, distortion, PSNR dB) %s | split %s" % ("9/7" if irrev else "5/3", name, target, out[1], out[0]))


# ---- 8. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals():
    layout = G.ImageLayout.make(128, 128)
    base = G.TileParams.make(1, 1, 3, 8, 2, mct=False)
    planes = make_planes(layout, S420, 8, seed=1)
    surface, sampling, nbytes = G.Surface.make("NV12", layout, pitch=128)
    buf = np.zeros(nbytes, np.uint8)
    surface.scatter(buf, planes, 1)
    c = G.Context(0)
    try:
        c.set_pipelining(True)
        with pytest.raises(G.RateError) as e:
            c.encode_image_subsampled_rate(layout, base, S420, planes, 10000)
        assert e.value.code == ERR_UNSUPPORTED
        with pytest.raises(G.RateError) as e:
            c.encode_surface_rate(layout, base, sampling, surface, buf, 10000)
        assert e.value.code == ERR_UNSUPPORTED
        with pytest.raises(G.RateError) as e:
            c.encode_image_rate(layout, G.TileParams.make(128, 128, 3, 8, 2), synth.g2(3, 128, 128, 8), 10000, joint=True)
        assert e.value.code == ERR_UNSUPPORTED
        c.set_pipelining(False)
        cs, res = c.encode_image_subsampled_rate(layout, base, S420, planes, 10000)
        assert len(cs) <= 10000
        # a target below the headers, SKIP allowed; below what the largest drop everywhere takes, without SKIP
        for call in (lambda t, s: c.encode_image_subsampled_rate(layout, base, S420, planes, t, max_drop=DMAX, allow_skip=s),
                     lambda t, s: c.encode_surface_rate(layout, base, sampling, surface, buf, t, max_drop=DMAX, allow_skip=s)):
            with pytest.raises(G.RateError) as e:
                call(60, True)
            assert e.value.code == ERR_OVERFLOW and "no byte of any block" in e.value.reason
            with pytest.raises(G.RateError) as e:
                call(200, False)
            assert e.value.code == ERR_OVERFLOW and "bytes" in e.value.reason
        for call in (lambda: c.encode_image_subsampled_rate(layout, base, S420, planes, 10000, max_drop=13),
                     lambda: c.encode_surface_rate(layout, base, sampling, surface, buf, 10000, max_drop=13)):
            with pytest.raises(G.RateError) as e:
                call()
            assert e.value.code != 0 and "max_drop" in e.value.reason
        # a surface that does not fit `cap`: before any work
        before = c.surface_counters()
        with pytest.raises(G.RateError) as e:
            c.encode_surface_rate(layout, base, sampling, surface, buf, 10000, cap=nbytes - 1)
        assert e.value.code == ERR_OVERFLOW and c.surface_counters() == before
        # a plain encode of sub-sampled components drops nothing
        with pytest.raises(RuntimeError, match=str(ERR_UNSUPPORTED)):
            c.encode_image_subsampled(layout, base, S420, planes, G.CS_BLOCK_MSBS)
    finally:
        c.close()
