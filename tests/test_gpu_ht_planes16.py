"""-m gpu: the HT block coder instances that 8-bit reversible content runs, on chosen coefficient planes.

An encode of 8-bit reversible pixels keeps int16 Mallat planes and launches ht_encode_kernel<false, true, ROOM> -- the two-quads-per-
lane pair form (phase_a2) for aligned 64 x 64 blocks, the general path with int16 loads elsewhere, ht_encode_fallback_kernel<false,
true> behind capped LDS streams --, a decode keeps int16 planes behind K5b with a range flag.  grk_amd_stage_ht_encode16 /
grk_amd_stage_ht_decode16 run exactly those on planes of the test's choosing: content that breaks block coders (0xFF-dense MagSgn,
sparse, wide beside narrow quads, one sample in an empty block, exponent boundaries), the whole contract range |c| < 2^(Kmax+1) with
the refusal one value beyond it, and the decoder's range flag at the values where it has to change.
Reference: the oracle's block coder (pinned to the reference's, up to Kmax + 1 bits, in test_oracle_golden.py)."""
import numpy as np
import pytest

import grok_amd as G
import gpuutil as U
import oracle as O
import synth
import ht_content as HC
from test_gpu_stages import _dev_view

pytestmark = pytest.mark.gpu

ROOM = G.capi.STAGE_HT_ROOM
# name -> (W, H, L, C, tiles, origin); every case 8-bit reversible
GEOMS = {"a": (128, 128, 1, 1, 1, (0, 0)), "b": (132, 132, 1, 1, 1, (0, 0)), "c": (130, 130, 1, 1, 1, (0, 0)),
         "d": (256, 192, 3, 3, 2, (0, 0)), "e": (37, 3, 1, 1, 1, (0, 0)), "e1": (1, 1, 1, 1, 1, (0, 0)),
         "f": (257, 129, 2, 1, 1, (33, 95))}


def _params(name):
    W, H, L, C, T, origin = GEOMS[name]
    return G.TileParams.make(W, H, C, 8, L, origin=origin), T


def _dims(b):
    return b.x1 - b.x0, b.y1 - b.y0


def _pair_form(p, b):
    """the kernel's condition for phase_a2: a 64 x 64 block whose plane column and the plane stride are multiples of 4"""
    return _dims(b) == (64, 64) and (b.px | G.lib().grk_amd_plane_stride(p)) % 4 == 0


def _assert_geometry(name, p, blocks):
    """what the geometry is in the list for, from the layout itself (so that no case goes vacuous)"""
    stride = G.lib().grk_amd_plane_stride(p)
    full = [b for b in blocks if _dims(b) == (64, 64)]
    sizes = {_dims(b) for b in blocks}
    kmax = [b.kmax for b in blocks]
    assert min(kmax) >= 8 and max(kmax) <= 12             # |c| < 2^(Kmax + 1) <= 8192 fits an int16 plane
    if name == "a":
        assert len(blocks) == 4 and len(full) == 4 and all(_pair_form(p, b) for b in blocks) and stride % 4 == 0
    elif name == "b":
        assert any(b.px % 2 == 0 and b.px % 4 != 0 for b in full) and {(2, 64), (64, 2)} <= sizes
        assert not any(_pair_form(p, b) for b in blocks if b.px % 4 != 0)
    elif name == "c":
        assert any(b.px % 2 == 1 for b in full)
    elif name == "d":
        assert p.num_comps == 3 and len(blocks) * 2 > 64       # two tiles; many blocks reserve their bytes in one allocation region
        assert any(_pair_form(p, b) for b in blocks) and any(not _pair_form(p, b) for b in blocks)
    elif name == "f":
        assert (p.tile_x0, p.tile_y0) == (33, 95) and any(b.x0 % 64 or b.y0 % 64 for b in blocks)     # off the block grid
        assert any(w < 64 or h < 64 for w, h in sizes)


def _oracle_blocks(blocks, planes, ntiles):
    C = max(b.comp for b in blocks) + 1
    want = []
    for t in range(ntiles):
        for b in blocks:
            bw, bh = _dims(b)
            want.append(O.ht_encode_sm(O.signmag(planes[t * C + b.comp, b.py:b.py + bh, b.px:b.px + bw], b.kmax), b.kmax))
    return want


def _encode16(c, p, ntiles, planes, nblocks, flags):
    d_m = U.upload_planes16(planes, p)
    c.stage_ht_encode16(p, ntiles, d_m.data_ptr(), flags)
    table, tot = c.fetch_table(nblocks * ntiles)
    return U.split_blocks(table, c.fetch_coded(tot))


def _encode32(c, p, ntiles, planes, nblocks):
    d_m = U.upload_planes(planes.astype(np.int32), p)
    c.stage_ht_encode(p, ntiles, d_m.data_ptr())
    table, tot = c.fetch_table(nblocks * ntiles)
    return U.split_blocks(table, c.fetch_coded(tot))


def _check_all_instances(c, p, ntiles, blocks, planes, what):
    """int16 stage (plain and ROOM instance) and the int32 stage on the same planes == the oracle, block for block"""
    want = _oracle_blocks(blocks, planes, ntiles)
    for inst, got in (("int16", _encode16(c, p, ntiles, planes, len(blocks), 0)),
                      ("int16 ROOM", _encode16(c, p, ntiles, planes, len(blocks), ROOM)),
                      ("int32", _encode32(c, p, ntiles, planes, len(blocks)))):
        bad = [(i, blocks[i % len(blocks)].kmax) + _dims(blocks[i % len(blocks)]) + (len(got[i]), len(want[i]))
               for i in range(len(want)) if got[i] != want[i]]
        assert not bad, "%s, %s: blocks differing from the oracle (idx, kmax, w, h, len_gpu, len_oracle): %s" % (what, inst, bad[:8])
    return want


def _fill(p, ntiles, blocks, per_block):
    """planes (ntiles * C, H, W) int64 with per_block(index over all tiles, block) -> (bh, bw) signed values"""
    C = p.num_comps
    planes = np.zeros((ntiles * C, p.tile_h, p.tile_w), np.int64)
    for t in range(ntiles):
        for i, b in enumerate(blocks):
            bw, bh = _dims(b)
            planes[t * C + b.comp, b.py:b.py + bh, b.px:b.px + bw] = per_block(t * len(blocks) + i, b)
    return planes


# ---- K3: content modes on every geometry ------------------------------------------------------------------------------------
@pytest.mark.parametrize("above", [0, 1], ids=["top=Kmax", "top=Kmax+1"])
@pytest.mark.parametrize("mode", HC.MODES)
@pytest.mark.parametrize("geom", list(GEOMS))
def test_k3_planes16_content_modes(geom, mode, above):
    p, T = _params(geom)
    blocks, _ = G.tile_layout(p)
    _assert_geometry(geom, p, blocks)
    rng = np.random.default_rng([ord(geom[0]), len(geom), HC.MODES.index(mode), above])
    planes = _fill(p, T, blocks, lambda i, b: HC.signed(rng, HC.magnitudes(rng, _dims(b)[1], _dims(b)[0], b.kmax + above, mode)))
    if mode != 3 and planes.size >= 64:          # (the 1 x 1 tile's one random sample may be zero)
        assert np.count_nonzero(planes) >= planes.size // 64
    if mode == 4:
        assert np.abs(planes).max() == (1 << (max(b.kmax for b in blocks) + above)) - 1
    _check_all_instances(U.ctx(), p, T, blocks, planes, "%s mode %s" % (geom, mode))


@pytest.mark.parametrize("above", [0, 1], ids=["top=Kmax", "top=Kmax+1"])
@pytest.mark.parametrize("small", [True, False], ids=["mag=1", "mag=2^top-1"])
@pytest.mark.parametrize("geom", list(GEOMS))
def test_k3_planes16_one_significant_sample_per_block(geom, small, above):
    """One sample in an otherwise empty block, at each position of a quad in the first and last quad row and column: block i of
    pass s takes position (i + s) mod 16, four passes of stride 4, so that the four 64 x 64 blocks of geometry (a) see all 16."""
    p, T = _params(geom)
    blocks, _ = G.tile_layout(p)
    rng = np.random.default_rng(7)
    for s in range(0, 16, 4):
        planes = _fill(p, T, blocks, lambda i, b: HC.signed(rng, HC.single_sample(_dims(b)[1], _dims(b)[0], i + s,
                                                                                  1 if small else (1 << (b.kmax + above)) - 1)))
        assert np.count_nonzero(planes) == len(blocks) * T
        _check_all_instances(U.ctx(), p, T, blocks, planes, "%s pass %d" % (geom, s))


@pytest.mark.parametrize("above", [0, 1], ids=["top=Kmax", "top=Kmax+1"])
@pytest.mark.parametrize("kind", HC.Q_KINDS)
@pytest.mark.parametrize("geom", list(GEOMS))
def test_k3_planes16_quad_patterns(geom, kind, above):
    p, T = _params(geom)
    blocks, _ = G.tile_layout(p)
    rng = np.random.default_rng([ord(geom[0]), HC.Q_KINDS.index(kind), above])
    planes = _fill(p, T, blocks, lambda i, b: HC.signed(rng, HC.quad_pattern(rng, _dims(b)[1], _dims(b)[0], b.kmax + above, kind)))
    _check_all_instances(U.ctx(), p, T, blocks, planes, "%s %s" % (geom, kind))


def test_k3_pair_form_block_counts():
    """How many blocks of each geometry take the pair form (phase_a2) and how many the general int16 path, from the layout."""
    got = {}
    for name in GEOMS:
        p, T = _params(name)
        blocks, _ = G.tile_layout(p)
        pair = sum(_pair_form(p, b) for b in blocks) * T
        got[name] = (pair, len(blocks) * T - pair)
    print("blocks in (pair form, general path):", got)
    assert got["a"] == (4, 0) and got["e"][0] == 0 and got["e1"][0] == 0 and got["b"][1] > 0 and got["c"][1] > 0
    assert got["d"][0] > 0 and got["d"][1] > 0 and got["f"][1] > 0


# ---- K3: capped LDS streams and the fallback launch ---------------------------------------------------------------------------
@pytest.mark.parametrize("geom", ["a", "d"])
def test_k3_planes16_lds_cap_and_fallback(geom, monkeypatch):
    """Modes 0 and 4 at both tops in fresh contexts with GRK_AMD_LDS_CAP=1 and =0: the same bytes, the oracle's.  With the cap on the
    raw streams hold 8 bits per sample (Kmax <= 11); uniform magnitudes below 2^Kmax need ~Kmax of them, all-at-the-top content
    Kmax + 1 or Kmax + 2: the blocks outgrow the capped streams and ht_encode_fallback_kernel<false, true> codes them -- in every
    one of these cases (all 4 blocks of geometry (a), 54 of the 114 of (d)), on both instances."""
    p, T = _params(geom)
    blocks, _ = G.tile_layout(p)
    cases = []
    for mode in (0, 4):
        for above in (0, 1):
            rng = np.random.default_rng([mode, above, ord(geom)])
            cases.append(((mode, above), _fill(p, T, blocks, lambda i, b: HC.signed(
                rng, HC.magnitudes(rng, _dims(b)[1], _dims(b)[0], b.kmax + above, mode)))))
    want = {k: _oracle_blocks(blocks, planes, T) for k, planes in cases}
    handed = {}
    for cap in ("1", "0"):
        monkeypatch.setenv("GRK_AMD_LDS_CAP", cap)
        c = G.Context(0)
        try:
            for k, planes in cases:
                for flags in (0, ROOM):
                    got = _encode16(c, p, T, planes, len(blocks), flags)
                    handed[(cap, k, flags)] = int(_dev_view(c.table_device_ptr(3), 24, "<i8").cpu().sum())
                    assert got == want[k], "GRK_AMD_LDS_CAP=%s mode %d top Kmax+%d flags %d" % ((cap,) + k + (flags,))
        finally:
            c.close()
    print("blocks handed to the fallback launch:", handed)
    assert all(n == 0 for (cap, _, _), n in handed.items() if cap == "0")
    for k, _ in cases:
        assert handed[("1", k, 0)] > 0 and handed[("1", k, ROOM)] > 0, "no block of mode %d top Kmax+%d reached the fallback launch" % k


# ---- the stage is what an encode launches ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["noise", "g2"])
def test_stage16_on_an_encodes_own_planes_gives_the_encodes_blocks(kind):
    """Pixels -> grk_amd_encode_tiles (plain context, GRK_AMD_PLANES16 at its default): the int16 Mallat planes it kept, fed to
    grk_amd_stage_ht_encode16, give the encode's own blocks -- the stage and the encode run the same kernels on the same layout."""
    C, H, W, L = 3, 192, 256, 3
    px = synth.g2(C, H, W, 8) if kind == "g2" else np.random.default_rng(3).integers(0, 256, size=(C, H, W)).astype(np.uint8)
    p = G.TileParams.make(W, H, C, 8, L)
    c = U.ctx()
    assert c.plane_sample_bytes(p)[0] == 2
    table, coded = c.encode_host(p, px)
    mine = U.split_blocks(table, coded)
    n16 = int(G.lib().grk_amd_plane_elems(p)) * C
    c.synchronize()
    kept = U.from_dev_ptr(c.plane_device_ptr(1), n16 * 2).view(np.int16)
    stride = G.lib().grk_amd_plane_stride(p)
    blocks, _ = G.tile_layout(p)
    # (they are the oracle's coefficients: the planes read here are what was coded)
    ing = [px[k].astype(np.int32) - 128 for k in range(C)]
    ing = O.rct_fwd(*ing)
    for k in range(C):
        assert np.array_equal(kept.reshape(C, H, stride)[k, :, :W], O.dwt53_fwd(ing[k], L))
    d_m = U.to_dev(kept)
    for flags in (0, ROOM):
        c.stage_ht_encode16(p, 1, d_m.data_ptr(), flags)
        t2, tot = c.fetch_table(len(blocks))
        assert U.split_blocks(t2, c.fetch_coded(tot)) == mine, "flags %d" % flags


def test_stage16_refuses_parameters_without_int16_planes():
    c = U.ctx()
    for p in (G.TileParams.make(128, 128, 1, 8, 1, irreversible=True), G.TileParams.make(128, 128, 1, 12, 1),
              G.TileParams.make(64, 64, 1, 8, 0)):
        d_m = U.dev_planes16(p, 1)
        with pytest.raises(RuntimeError, match=r"-3 \("):
            c.stage_ht_encode16(p, 1, d_m.data_ptr(), 0)
    p = G.TileParams.make(128, 128, 1, 8, 1)
    with pytest.raises(RuntimeError, match=r"-3 \("):
        c.stage_ht_encode16(p, 1, U.dev_planes16(p, 1).data_ptr(), 2)


# ---- K3's contract edge: |c| = 2^(Kmax+1) is refused, 2^(Kmax+1) - 1 is coded -----------------------------------------------------
def _edge_cases():
    """(geometry, which block, column parity inside the block, why)"""
    return [("a", "full", 0, "pair form, low half of the packed word"), ("a", "full", 1, "pair form, high half: the fold"),
            ("b", "unaligned", 0, "general int16 path, 64 x 64"), ("b", "unaligned", 1, "general int16 path, 64 x 64"),
            ("b", "edge", 1, "general int16 path, 2 x 64 edge block")]


@pytest.mark.parametrize("geom,which,col,why", _edge_cases(), ids=["%s-%s-col%d" % t[:3] for t in _edge_cases()])
@pytest.mark.parametrize("sign", [1, -1], ids=["pos", "neg"])
def test_k3_contract_edge(geom, which, col, why, sign):
    """A tile whose planes are zero but for ONE sample.  Magnitude 2^(Kmax+1): status bit 1, fetch_table raises -- on the int16
    stage (both instances) and the int32 stage.  Magnitude 2^(Kmax+1) - 1: coded, the oracle's bytes.
    (The single sample is what keeps the refused block inside its LDS streams: its MagSgn value has Kmax + 2 bits, the quad's u is
    Kmax + 2 <= 14 -- inside the 32-entry UVLC table --, against streams of >= 8 bits per sample of a block of >= 128 samples.)"""
    p, T = _params(geom)
    blocks, _ = G.tile_layout(p)
    if which == "full":
        b = next(b for b in blocks if _pair_form(p, b) and b.px > 0)
    elif which == "unaligned":
        b = next(b for b in blocks if _dims(b) == (64, 64) and b.px % 4 == 2)
    else:
        b = next(b for b in blocks if _dims(b) == (2, 64))
    assert _dims(b)[0] * _dims(b)[1] >= 128
    x = b.px + (10 if _dims(b)[0] == 64 else 0) + col
    assert (x - b.px) % 2 == col and (which != "full" or x % 2 == col)       # (pair form: column parity = half of the packed word)
    c = U.ctx()
    for mag, ok in (((1 << (b.kmax + 1)) - 1, True), (1 << (b.kmax + 1), False)):
        planes = np.zeros((1, p.tile_h, p.tile_w), np.int64)
        planes[0, b.py + 5, x] = sign * mag
        if ok:
            _check_all_instances(c, p, 1, blocks, planes, why)
            continue
        for run in (lambda: _encode16(c, p, 1, planes, len(blocks), 0), lambda: _encode16(c, p, 1, planes, len(blocks), ROOM),
                    lambda: _encode32(c, p, 1, planes, len(blocks))):
            with pytest.raises(RuntimeError, match="exceeds Kmax\\+1 bits"):
                run()


# ---- K5: the int16 store path ---------------------------------------------------------------------------------------------------
def _decode16(c, p, ntiles, table, coded):
    d_c = U.to_dev(np.frombuffer(coded, np.uint8).copy())
    d_m = U.dev_planes16(p, ntiles * p.num_comps)
    c.stage_ht_decode16(p, ntiles, table, d_c.data_ptr(), d_c.numel(), d_m.data_ptr())
    c.synchronize()
    return U.planes16_to_numpy(d_m, p, ntiles * p.num_comps)


@pytest.mark.parametrize("mode", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("geom", ["a", "b", "d", "e", "e1"])
def test_k5_planes16_blocks_equal_source(geom, mode):
    """Planes with magnitudes <= 2^(Kmax - 2) (what both decoders accept: defect D5) -> the oracle's block encoder ->
    grk_amd_stage_ht_decode16 == the planes, exactly; mode 3 has blocks without data."""
    p, T = _params(geom)
    blocks, _ = G.tile_layout(p)
    rng = np.random.default_rng([ord(geom[0]), len(geom), mode])
    C = p.num_comps
    planes = np.zeros((T * C, p.tile_h, p.tile_w), np.int32)
    table = np.zeros(len(blocks) * T, G.capi.CODED_DTYPE)
    chunks, off, empty = [], 0, 0
    for t in range(T):
        for i, b in enumerate(blocks):
            bw, bh = _dims(b)
            kb = b.kmax - 2
            mag = rng.integers(0, (1 << kb) + 1, size=(bh, bw))
            if mode == 1:
                mag = mag >> rng.integers(0, kb + 1, size=(bh, bw))
            elif mode == 2:
                mag = np.where(rng.random((bh, bw)) < 0.93, 0, mag & 7)
            elif mode == 3:
                mag = np.zeros((bh, bw), np.int64)
            elif mode == 4:
                mag = np.full((bh, bw), 1 << kb)
            coef = HC.signed(rng, mag).astype(np.int32)
            planes[t * C + b.comp, b.py:b.py + bh, b.px:b.px + bw] = coef
            cb = O.ht_encode_sm(O.signmag(coef, b.kmax), b.kmax)
            if mode == 3 and i % 3 == 0:
                cb = b""; empty += 1
            r = t * len(blocks) + i
            table["offset"][r] = off; table["length"][r] = len(cb); table["missing_msbs"][r] = b.kmax - 1
            chunks.append(cb + b"\0" * (-len(cb) % 16)); off += len(chunks[-1])
    assert mode != 3 or empty > 0
    assert np.abs(planes).max() <= 1024            # inside the packed inverse transform's range: no flag
    got = _decode16(U.ctx(), p, T, table, b"".join(chunks) + b"\0" * 16)
    assert got.dtype == np.int16 and np.array_equal(got, planes)


RANGE_GEOM = (130, 134, 1)         # LL 65 x 67: a 64 x 64 block, and edge blocks of height 3


def _range_case(value, edge, bottom, fill=0):
    """one coded block (missing_msbs 17: a 16-bit tile's block under 8-bit parameters), all zero but `value` on the top / bottom
    row of its quad -- and, with fill != 0, the rest of that sample's column at `fill`; -> (params, table, coded bytes, the
    oracle's plane)"""
    W, H, L = RANGE_GEOM
    p = G.TileParams.make(W, H, 1, 8, L)
    blocks, _ = G.tile_layout(p)
    i = next(i for i, b in enumerate(blocks) if (_dims(b) == (64, 3) if edge else _dims(b) == (64, 64)))
    b = blocks[i]
    bw, bh = _dims(b)
    coef = np.zeros((bh, bw), np.int64)
    y = (1 if bottom else 2) if edge else (11 if bottom else 10)       # (row 2 of 3: the top row of a quad without a bottom row)
    coef[:, 7] = fill
    coef[y, 7] = value
    cb = O.ht_encode_sm(O.signmag(coef, 18), 18)
    sm = O.ht_decode_block(cb, 17, bw, bh)
    assert sm is not None
    want = np.zeros((1, H, W), np.int64)
    want[0, b.py:b.py + bh, b.px:b.px + bw] = O.ht_dequant_rev(sm, 17)
    assert want[0, b.py + y, b.px + 7] == value and np.count_nonzero(want) == (bh if fill else 1)
    table = np.zeros(len(blocks), G.capi.CODED_DTYPE)
    table["length"][i] = len(cb); table["missing_msbs"][i] = 17
    return p, table, cb + b"\0" * 32, want


@pytest.mark.parametrize("edge", [False, True], ids=["64x64", "64x3"])
@pytest.mark.parametrize("bottom", [False, True], ids=["ot", "ob"])
@pytest.mark.parametrize("pk", [1, 0], ids=["bias2048", "bias32768"])
def test_k5_planes16_range_flag_at_its_edge(pk, bottom, edge, monkeypatch):
    """The flag is range >= 2 * bias on value + bias: [-bias, bias) decodes, bias and -bias - 1 raise GRK_AMD_ERR_RANGE.  bias 2048
    with the packed inverse transform behind (the default; pk16.h kPkDecodeBound = 2047), 32768 with GRK_AMD_DWT_PK=0.
    A lane ORs value + bias over its sample column and a zero sample contributes `bias` itself, so beside zeros +bias gives
    3 * bias: only a column of nothing but -bias (-> 0) and +bias (-> 2 * bias) leaves exactly 2 * bias in front of the comparison
    -- the last case, the one that tells >= from >."""
    bias = 2048 if pk else 32768
    if pk:
        c = U.ctx()
    else:
        monkeypatch.setenv("GRK_AMD_DWT_PK", "0")
        c = G.Context(0)

    def raises_and_int32_decodes(p, table, coded, want, what):
        with pytest.raises(RuntimeError, match="16-bit planes"):
            _decode16(c, p, 1, table, coded)
        d_c = U.to_dev(np.frombuffer(coded, np.uint8).copy())
        d_m = U.dev_planes(p, 1)
        c.stage_ht_decode(p, 1, table, d_c.data_ptr(), d_c.numel(), d_m.data_ptr())
        c.synchronize()
        assert np.array_equal(U.planes_to_numpy(d_m, p, 1), want), what

    try:
        for value in (bias - 1, -bias):
            p, table, coded, want = _range_case(value, edge, bottom)
            assert np.array_equal(_decode16(c, p, 1, table, coded), want), value
        for value in (bias, -bias - 1):
            raises_and_int32_decodes(*_range_case(value, edge, bottom), value)
        # the sample's whole column at -bias: still inside; one +bias among them: outside, and value + bias == 2 * bias is then
        # ALL the lane has seen
        p, table, coded, want = _range_case(-bias, edge, bottom, fill=-bias)
        assert np.array_equal(_decode16(c, p, 1, table, coded), want)
        raises_and_int32_decodes(*_range_case(bias, edge, bottom, fill=-bias), "column")
    finally:
        if not pk:
            c.close()


def test_stage_decode16_refusals():
    c = U.ctx()
    good = G.TileParams.make(128, 128, 1, 8, 1)
    nb = len(G.tile_layout(good)[0])
    d_c = U.to_dev(np.zeros(64, np.uint8))

    def run(p):
        table = np.zeros(len(G.tile_layout(p)[0]), G.capi.CODED_DTYPE)
        c.stage_ht_decode16(p, 1, table, d_c.data_ptr(), d_c.numel(), U.dev_planes16(p, 1).data_ptr())

    for p in (G.TileParams.make(128, 128, 1, 8, 1, irreversible=True), G.TileParams.make(128, 128, 1, 12, 1),
              G.TileParams.make(128, 128, 1, 8, 1, part1=True)):
        with pytest.raises(RuntimeError, match=r"-3 \("):
            run(p)
    c.set_decode_segments([[(0, 1)]] * nb)
    try:
        with pytest.raises(RuntimeError, match=r"-3 \("):
            run(good)
    finally:
        c.set_decode_segments(None)
    run(good)            # (and without the list the same call is taken: every block absent)
