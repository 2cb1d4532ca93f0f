"""GPU: MSB-aligned surfaces (grk_amd_surface_comp::shift -- P010, P012, P210 ...).  First the two kernels alone
(grok_amd/csrc/kernels_surface.hip through grk_amd_surface_cut_device / grk_amd_surface_place_device) with numpy index arithmetic as
the oracle: a cut equals word >> shift; a placement runs into a buffer of random bytes, the samples equal v << shift cut to the
container and the WHOLE buffer is compared, so a byte written outside a sample -- the other partner's included -- shows.  Widths
across one and several 16-byte lines with every head and tail, first samples at every alignment of the first line, every step, the
partner pair by one launch and as two, surfaces and unit planes on odd addresses (the sample-by-sample fallback).  Then the whole
calls: grk_amd_encode_surface's file == grk_amd_encode_image_subsampled's of the planes word >> shift, whatever the low bits hold;
grk_amd_decode_surface writes plane << shift and nothing else; both staged.  All comparisons are exact."""
import numpy as np
import pytest

import grok_amd as G
import gpuutil as U
from test_gpu_surface import sample_index
from test_t2_reader_subsampled_cpu import make_planes

pytestmark = pytest.mark.gpu
WIDTHS = (1, 3, 4, 5, 7, 8, 9, 17, 65, 130)
HEIGHTS = (1, 5)
FIRSTS = (0, 2, 4, 6, 10, 14)
SHIFTS = (0, 4, 6)
POISON = 0xA5


def geometry(w, h, bps, step, first, ncomp, partner, pitch_extra=0):
    """two units of w x h at (0, 0) and (w + 3, 2); `ncomp` components: partners a sample apart, or planes of their own"""
    origins = [(0, 0), (w + 3, 2)]
    cols, rows = origins[1][0] + w, origins[1][1] + h
    span = ((cols - 1) * step + 1) * bps + ((ncomp - 1) * bps if partner else 0)
    pitch = span + 5 * bps + pitch_extra
    comps, at = [], first
    for k in range(ncomp):
        comps.append((at, pitch, step))
        at += bps if partner else rows * pitch + 3 * bps
    nbytes = max(c[0] for c in comps) + (rows - 1) * pitch + ((cols - 1) * step + 1) * bps
    return origins, comps, nbytes


def words(b, bps):
    """[..., bps] bytes -> integers (host endian: little)"""
    return b[..., 0].astype(np.uint32) if bps == 1 else b[..., 0].astype(np.uint32) | (b[..., 1].astype(np.uint32) << 8)


def unwords(v, bps):
    return np.stack([(v >> (8 * k)) & 0xFF for k in range(bps)], axis=-1).astype(np.uint8)


def run_cut(c, rng, w, h, bps, origins, comps, nbytes, base=0, tiles_base=0):
    """comps: (offset, pitch, step, shift); base / tiles_base: bytes into their allocations at which the surface / the planes start"""
    surf = rng.integers(0, 256, base + nbytes + 7, dtype=np.uint8)
    d_surf = U.to_dev(surf)
    n = len(origins) * len(comps) * h * w * bps
    d_tiles = U.to_dev(np.full(tiles_base + n + 16, POISON, np.uint8))
    c.surface_cut_device(d_surf.data_ptr() + base, nbytes, comps, bps, len(origins), w, h, origins, d_tiles.data_ptr() + tiles_base)
    c.synchronize()
    got = d_tiles.cpu().numpy()
    want = np.concatenate([unwords(words(surf[base:][sample_index(cp[:3], bps, ox, oy, w, h)], bps) >> cp[3], bps).reshape(-1)
                           for ox, oy in origins for cp in comps])
    assert np.array_equal(got[tiles_base:tiles_base + n], want), ("cut", w, h, bps, comps, base, tiles_base)
    assert np.all(got[:tiles_base] == POISON) and np.all(got[tiles_base + n:] == POISON)


def run_place(c, rng, w, h, bps, origins, comps, nbytes, one_by_one=False, base=0, tiles_base=0):
    n = len(origins) * len(comps) * h * w * bps
    tiles = rng.integers(0, 256, n, dtype=np.uint8)                      # (every bit set somewhere: what leaves the container is cut)
    before = rng.integers(0, 256, base + nbytes + 64, dtype=np.uint8)
    want = before.copy()
    t = tiles.reshape(len(origins), len(comps), h, w, bps)
    for u, (ox, oy) in enumerate(origins):
        for k, cp in enumerate(comps):
            want[base:][sample_index(cp[:3], bps, ox, oy, w, h)] = unwords((words(t[u, k], bps) << cp[3]) & ((1 << 8 * bps) - 1), bps)
    d_surf = U.to_dev(before)
    pad = np.zeros(tiles_base, np.uint8)
    if one_by_one:
        for k, cp in enumerate(comps):
            d_tiles = U.to_dev(np.concatenate([pad, np.ascontiguousarray(t[:, k]).reshape(-1)]))
            c.surface_place_device(d_tiles.data_ptr() + tiles_base, len(origins), w, h, bps, origins, [cp], d_surf.data_ptr() + base, nbytes)
            c.synchronize()
    else:
        d_tiles = U.to_dev(np.concatenate([pad, tiles]))
        c.surface_place_device(d_tiles.data_ptr() + tiles_base, len(origins), w, h, bps, origins, comps, d_surf.data_ptr() + base, nbytes)
        c.synchronize()
    got = d_surf.cpu().numpy()
    assert np.array_equal(got, want), ("place", w, h, bps, comps, base, tiles_base, one_by_one, np.flatnonzero(got != want)[:8])


def shifted(comps, shifts):
    return [cp + (sh,) for cp, sh in zip(comps, shifts)]


@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("step", [1, 2, 3, 4])
def test_lone_two_byte_component(step, shift):
    """step 1: the shifting row move; step 2: four samples out of each 16-byte line on the cut, stores of its own samples on the
    placement; steps 3 and 4: sample by sample"""
    c, rng = U.ctx(), np.random.default_rng(100 + 10 * step + shift)
    for w in WIDTHS:
        for h in HEIGHTS:
            for first in FIRSTS:
                origins, comps, nbytes = geometry(w, h, 2, step, first, 1, False)
                run_cut(c, rng, w, h, 2, origins, shifted(comps, [shift]), nbytes)
                run_place(c, rng, w, h, 2, origins, shifted(comps, [shift]), nbytes)


@pytest.mark.parametrize("shift", SHIFTS)
def test_two_byte_partner_pair_by_one_launch_and_as_two(shift):
    """Cb / Cr of P010 / P210 in either order: one launch (four samples of each plane merged into aligned 16-byte stores) == two lone
    launches (each leaving the other partner's bytes alone) == the oracle; the partners' shifts may differ"""
    c, rng = U.ctx(), np.random.default_rng(200 + shift)
    for w in WIDTHS:
        for h in HEIGHTS:
            for first in FIRSTS:
                origins, comps, nbytes = geometry(w, h, 2, 2, first, 2, True)
                for shifts in ([shift, shift], [shift, 6 - shift]):
                    cs = shifted(comps, shifts)
                    for order in (cs, cs[::-1]):
                        run_cut(c, rng, w, h, 2, origins, order, nbytes)
                        run_place(c, rng, w, h, 2, origins, order, nbytes)
                run_place(c, rng, w, h, 2, origins, shifted(comps, [shift, shift]), nbytes, one_by_one=True)


@pytest.mark.parametrize("shift", SHIFTS)
def test_two_byte_samples_on_odd_addresses(shift):
    """a surface one byte into its allocation, and unit planes one byte into theirs: no 16-byte form and no two-byte access is taken
    (an odd PITCH of two-byte samples is refused on the host, so the kernels never meet one: checked here too)"""
    c, rng = U.ctx(), np.random.default_rng(300 + shift)
    for w in (1, 7, 9, 65, 130):
        for first in (0, 6):
            for base, tiles_base in ((1, 0), (0, 1), (1, 1)):
                for step in (1, 2, 3):
                    origins, comps, nbytes = geometry(w, 5, 2, step, first, 1, False)
                    run_cut(c, rng, w, 5, 2, origins, shifted(comps, [shift]), nbytes, base, tiles_base)
                    run_place(c, rng, w, 5, 2, origins, shifted(comps, [shift]), nbytes, False, base, tiles_base)
                origins, comps, nbytes = geometry(w, 5, 2, 2, first, 2, True)
                for order in (shifted(comps, [shift, 2]), shifted(comps, [shift, 2])[::-1]):
                    run_cut(c, rng, w, 5, 2, origins, order, nbytes, base, tiles_base)
                    run_place(c, rng, w, 5, 2, origins, order, nbytes, False, base, tiles_base)
                    run_place(c, rng, w, 5, 2, origins, order, nbytes, True, base, tiles_base)
    origins, comps, nbytes = geometry(17, 5, 2, 1, 0, 1, False)
    odd = [(comps[0][0], comps[0][1] + 1, 1, shift)]
    d = U.to_dev(np.zeros(2 * nbytes, np.uint8))
    before = c.surface_counters()[2]
    with pytest.raises(G.SurfaceError) as e:
        c.surface_cut_device(d.data_ptr(), 2 * nbytes, odd, 2, 2, 17, 5, origins, d.data_ptr())
    assert e.value.code == -3 and c.surface_counters()[2] == before


def test_one_byte_samples_with_a_shift():
    """4 bits in the high nibble: steps 1 and 2, the pair by one launch and as two, even and odd pitches and first bytes; and the
    unshifted one-byte forms beside a shifted partner"""
    c, rng = U.ctx(), np.random.default_rng(400)
    for w in WIDTHS:
        for h in HEIGHTS:
            for first in (0, 1, 5, 14):
                for extra in (0, 1):
                    for step in (1, 2):
                        origins, comps, nbytes = geometry(w, h, 1, step, first, 1, False, extra)
                        run_cut(c, rng, w, h, 1, origins, shifted(comps, [4]), nbytes)
                        run_place(c, rng, w, h, 1, origins, shifted(comps, [4]), nbytes)
                    origins, comps, nbytes = geometry(w, h, 1, 2, first, 2, True, extra)
                    for shifts in ([4, 4], [0, 4]):
                        cs = shifted(comps, shifts)
                        for order in (cs, cs[::-1]):
                            run_cut(c, rng, w, h, 1, origins, order, nbytes)
                            run_place(c, rng, w, h, 1, origins, order, nbytes)
                    run_place(c, rng, w, h, 1, origins, shifted(comps, [4, 4]), nbytes, one_by_one=True)


def test_a_shift_of_the_whole_container_is_refused():
    c = U.ctx()
    origins, comps, nbytes = geometry(17, 5, 2, 1, 0, 1, False)
    d_surf = U.to_dev(np.full(nbytes + 64, POISON, np.uint8))
    d_tiles = U.to_dev(np.zeros(2 * 2 * 17 * 5, np.uint8))
    before = c.surface_counters()[2]
    for bps, sh in ((2, 16), (1, 8)):
        with pytest.raises(G.SurfaceError) as e:
            c.surface_place_device(d_tiles.data_ptr(), 2, 17, 5, bps, origins, shifted(comps, [sh]), d_surf.data_ptr(), nbytes)
        assert e.value.code == -3 and "shift" in e.value.reason
        with pytest.raises(G.SurfaceError) as e:
            c.surface_cut_device(d_surf.data_ptr(), nbytes, shifted(comps, [sh]), bps, 2, 17, 5, origins, d_tiles.data_ptr())
        assert e.value.code == -3 and "shift" in e.value.reason
    c.synchronize()
    assert c.surface_counters()[2] == before and np.all(d_surf.cpu().numpy() == POISON)


# ---- whole calls -----------------------------------------------------------------------------------------------------------------
# name: (format, size, image offset, tile, levels, irreversible); odd chroma sizes throughout (25 x 17, 35 x 25 at 4:2:0).  The 9/7 case
# is the one of 2 levels: grk_amd_decode_image refuses this encoder's 9/7 files of ONE level (U_q > missing_msbs), whatever the content
CASES = {
    "p010-one-tile": ("P010", (50, 34), (0, 0), None, 2, False),
    "p212-one-tile": ("P212", (50, 34), (0, 0), None, 2, False),
    "p010-tiles": ("P010", (70, 50), (3, 5), (32, 32), 1, False),
    "p212-tiles": ("P212", (70, 50), (3, 5), (32, 32), 1, False),
    "p010-one-tile-97": ("P010", (50, 34), (0, 0), None, 2, True),
}
_made = {}


def case(name):
    """(layout, base, sampling, surface, bytes, planes, the planes' file by encode_image_subsampled, its decode_image planes,
    units) -- made once, left unchanged"""
    if name not in _made:
        fmt, size, origin, tile, levels, irreversible = CASES[name]
        prec = G.SURFACE_FORMATS_MSB[fmt][1]
        layout = G.ImageLayout.make(*size, *(tile or (None, None)), offset=origin)
        pitch = 2 * size[0] + 14                                                # (some slack behind the rows)
        surface, sampling, nbytes = G.Surface.make(fmt, layout, pitch=pitch)
        assert [cp.shift for cp in surface.comp[:3]] == [16 - prec] * 3
        base = G.TileParams.make(1, 1, 3, prec, levels, mct=False, irreversible=irreversible)
        planes = make_planes(layout, sampling, prec, seed=len(name))
        if irreversible:
            # (as synth.g2_mid: with the 9/7 path's default steps the block under the darkest corner of the full-range ramp needs
            # all Kmax bit-planes, and the block decoder refuses such a block -- grk_amd_decode_image could not give the planes to
            # compare with; the middle three quarters of the range make a file that decodes)
            planes = [np.clip(pl, (1 << prec) // 8, 7 * (1 << prec) // 8).astype(pl.dtype) for pl in planes]
        assert any(pl.shape[1] % 2 for pl in planes[1:]) and all(pl.dtype == np.uint16 for pl in planes)
        c = U.ctx()
        cs = c.encode_image_subsampled(layout, base, sampling, planes, G.CS_PLT)
        back = c.decode_image_planes(cs)
        assert irreversible or all(np.array_equal(a, b) for a, b in zip(back, planes))
        ntiles = 1 if tile is None else -(-(origin[0] + size[0]) // tile[0]) * -(-(origin[1] + size[1]) // tile[1])
        _made[name] = (layout, base, sampling, surface, nbytes, planes, cs, back, 2 * ntiles)
    return _made[name]


def delta(c, call):
    before = c.surface_counters()
    out = call()
    c.decode_status()
    return out, tuple(a - b for a, b in zip(c.surface_counters(), before))


@pytest.mark.parametrize("name", sorted(CASES))
def test_encode_surface_reads_word_shr_shift(name):
    layout, base, sampling, surface, nbytes, planes, want, _, units = case(name)
    c, rng = U.ctx(), np.random.default_rng(7)
    sizes = [pl.shape[::-1] for pl in planes]
    shift = surface.comp[0].shift
    clean = rng.integers(0, 256, nbytes, dtype=np.uint8)
    surface.scatter(clean, planes, 2)
    # the same samples above random low bits: discarded, not checked
    noisy = clean.copy()
    unshifted = G.Surface.of([(cp.offset, cp.row_pitch, cp.step) for cp in surface.comp[:3]])
    low = [rng.integers(0, 1 << shift, pl.shape, dtype=np.uint16) for pl in planes]
    unshifted.scatter(noisy, [(pl.astype(np.uint16) << shift) | lo for pl, lo in zip(planes, low)], 2)
    assert not np.array_equal(noisy, clean)
    for buf in (clean, noisy):
        assert all(np.array_equal(a, b) for a, b in zip(surface.gather(buf, sizes, 2), planes))
        got, d = delta(c, lambda: c.encode_surface(layout, base, sampling, surface, buf, G.CS_PLT))
        assert got == want, (name, "host")
        assert d[0] == 0 and d[1] == units and d[2] >= 2, d                                  # all staged, none in place
        d_buf = U.to_dev(buf)
        assert d_buf.data_ptr() % 4 == 0
        got, d = delta(c, lambda: c.encode_surface(layout, base, sampling, surface, d_buf.data_ptr(), G.CS_PLT, cap=nbytes))
        assert got == want, (name, "device")
        assert d[0] == 0 and d[1] == units and d[2] >= 2, d
        assert np.array_equal(d_buf.cpu().numpy(), buf)                                      # an encode only reads


@pytest.mark.parametrize("name", sorted(CASES))
def test_decode_surface_writes_plane_shl_shift(name):
    layout, base, sampling, surface, nbytes, planes, cs, back, units = case(name)
    c = U.ctx()
    before = np.random.default_rng(8).integers(0, 256, nbytes, dtype=np.uint8)
    want = before.copy()
    surface.scatter(want, back, 2)
    assert not np.array_equal(want, before)
    sizes = [pl.shape[::-1] for pl in planes]
    shift = surface.comp[0].shift
    unshifted = G.Surface.of([(cp.offset, cp.row_pitch, cp.step) for cp in surface.comp[:3]])
    host = before.copy()
    _, d = delta(c, lambda: c.decode_surface(cs, surface, host))
    for word, plane in zip(unshifted.gather(host, sizes, 2), back):
        assert np.array_equal(word, plane.astype(np.uint16) << shift), (name, "host")         # (the low bits: zero)
    assert np.array_equal(host, want), (name, "host: a byte that is no sample changed")
    assert d[0] == 0 and d[1] == units and d[2] >= 2, d
    dev = U.to_dev(before)
    assert dev.data_ptr() % 4 == 0
    _, d = delta(c, lambda: c.decode_surface(cs, surface, dev.data_ptr(), cap=nbytes))
    assert np.array_equal(dev.cpu().numpy(), want), (name, "device")
    assert d[0] == 0 and d[1] == units and d[2] >= 2, d


@pytest.mark.parametrize("fmt,plain", [("P016", "NV12"), ("P216", "NV16")])
def test_sixteen_bits_are_the_plain_formats(fmt, plain):
    """prec 16: shift 0 -- the file and the surface of NV12 / NV16 at 16 bits"""
    c, rng = U.ctx(), np.random.default_rng(9)
    layout = G.ImageLayout.make(50, 34)
    surface, sampling, nbytes = G.Surface.make(fmt, layout, pitch=112)
    ref, ref_sampling, ref_bytes = G.Surface.make(plain, layout, 16, 112)
    assert bytes(surface) == bytes(ref) and (sampling, nbytes) == (ref_sampling, ref_bytes)
    base = G.TileParams.make(1, 1, 3, 16, 2, mct=False)
    planes = make_planes(layout, sampling, 16, seed=3)
    buf = rng.integers(0, 256, nbytes, dtype=np.uint8)
    surface.scatter(buf, planes, 2)
    want = c.encode_image_subsampled(layout, base, sampling, planes, G.CS_PLT)
    for pixels, cap in ((buf, None), (U.to_dev(buf), nbytes)):
        ptr = pixels if cap is None else pixels.data_ptr()
        assert c.encode_surface(layout, base, sampling, surface, ptr, G.CS_PLT, cap=cap) == want
        assert c.encode_surface(layout, base, sampling, ref, ptr, G.CS_PLT, cap=cap) == want
    before = rng.integers(0, 256, nbytes, dtype=np.uint8)
    outs = []
    for s in (surface, ref):
        host = before.copy()
        c.decode_surface(want, s, host)
        dev = U.to_dev(before)
        c.decode_surface(want, s, dev.data_ptr(), cap=nbytes)
        c.decode_status()
        assert np.array_equal(dev.cpu().numpy(), host)
        outs.append(host)
    assert np.array_equal(outs[0], outs[1])
    filled = before.copy()
    ref.scatter(filled, planes, 2)
    assert np.array_equal(outs[0], filled)
