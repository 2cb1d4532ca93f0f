"""GPU: the two surface kernels alone (grok_amd/csrc/kernels_surface.hip) through grk_amd_surface_cut_device /
grk_amd_surface_place_device, numpy indexing as the oracle.  KS (cut) is compared against slices of a random surface; KD (place) runs
into a buffer filled with a poison value and the WHOLE buffer is compared, so a byte written outside a sample shows.  Widths around
the 16-byte paths' heads, tails and lane counts, one row and more rows than a workgroup's band, every step, first samples at every
byte alignment, odd pitches; the partner pair of NV12 chroma by one launch and as two lone components."""
import numpy as np
import pytest

import grok_amd as G
import gpuutil as U

pytestmark = pytest.mark.gpu
WIDTHS = (1, 15, 16, 17, 63, 64, 65, 130)
HEIGHTS = (1, 17)
POISON = 0xA5


def sample_index(comp, bps, ox, oy, w, h):
    """byte indices [h, w, bps] of a unit's samples of one component on the surface"""
    off, pitch, step = comp
    y = (oy + np.arange(h, dtype=np.int64))[:, None, None]
    x = (ox + np.arange(w, dtype=np.int64))[None, :, None]
    return off + y * pitch + x * step * bps + np.arange(bps, dtype=np.int64)[None, None, :]


def geometry(w, h, bps, step, first, ncomp, partner, odd_pitch):
    """two units of w x h; comps of `ncomp` components: partners k * bps apart (interleaved), or planes of their own"""
    origins = [(0, 0), (w + 3, 2)] if h > 1 else [(0, 0), (w + 1, 0)]
    cols, rows = origins[1][0] + w, origins[1][1] + h
    span = ((cols - 1) * step + 1) * bps
    if partner:
        span += (ncomp - 1) * bps
    pitch = span + 5 * bps
    if bps == 1 and odd_pitch != (pitch & 1):
        pitch += 1
    comps, at = [], first
    for k in range(ncomp):
        comps.append((at, pitch, step))
        at += bps if partner else rows * pitch + 3 * bps
    nbytes = max(c[0] for c in comps) + (rows - 1) * pitch + ((cols - 1) * step + 1) * bps
    return origins, comps, nbytes


def run_cut(c, rng, w, h, bps, origins, comps, nbytes):
    surf = rng.integers(0, 256, nbytes + 7, dtype=np.uint8)
    d_surf = U.to_dev(surf)
    n = len(origins) * len(comps) * h * w * bps
    d_tiles = U.to_dev(np.full(n + 16, POISON, np.uint8))
    c.surface_cut_device(d_surf.data_ptr(), nbytes, comps, bps, len(origins), w, h, origins, d_tiles.data_ptr())
    c.synchronize()
    got = d_tiles.cpu().numpy()
    want = np.concatenate([surf[sample_index(cp, bps, ox, oy, w, h)].reshape(-1) for ox, oy in origins for cp in comps])
    assert np.array_equal(got[:n], want), ("cut", w, h, bps, comps)
    assert np.all(got[n:] == POISON)


def run_place(c, rng, w, h, bps, origins, comps, nbytes, one_by_one=False):
    n = len(origins) * len(comps) * h * w * bps
    tiles = rng.integers(0, 256, n, dtype=np.uint8)
    want = np.full(nbytes + 64, POISON, np.uint8)
    t = tiles.reshape(len(origins), len(comps), h, w, bps)
    for u, (ox, oy) in enumerate(origins):
        for k, cp in enumerate(comps):
            want[sample_index(cp, bps, ox, oy, w, h)] = t[u, k]
    d_surf = U.to_dev(np.full(nbytes + 64, POISON, np.uint8))
    if one_by_one:
        for k, cp in enumerate(comps):
            d_tiles = U.to_dev(np.ascontiguousarray(t[:, k]).reshape(-1))
            c.surface_place_device(d_tiles.data_ptr(), len(origins), w, h, bps, origins, [cp], d_surf.data_ptr(), nbytes)
            c.synchronize()
    else:
        d_tiles = U.to_dev(tiles)
        c.surface_place_device(d_tiles.data_ptr(), len(origins), w, h, bps, origins, comps, d_surf.data_ptr(), nbytes)
        c.synchronize()
    got = d_surf.cpu().numpy()
    assert np.array_equal(got, want), ("place", w, h, bps, comps, np.flatnonzero(got != want)[:8])


@pytest.mark.parametrize("bps", [1, 2])
@pytest.mark.parametrize("step", [1, 2, 3, 4])
def test_lone_component(bps, step):
    """one component of its own: every path of both kernels that a single component takes"""
    c, rng = U.ctx(), np.random.default_rng(10 * bps + step)
    firsts = (0, 1, 2, 3, 5) if bps == 1 else (0, 2, 4, 6, 10)
    before = c.surface_counters()[2]
    n = 0
    for w in WIDTHS:
        for h in HEIGHTS:
            for first in firsts:
                origins, comps, nbytes = geometry(w, h, bps, step, first, 1, False, odd_pitch=(first & 1) == 0)
                run_cut(c, rng, w, h, bps, origins, comps, nbytes)
                run_place(c, rng, w, h, bps, origins, comps, nbytes)
                n += 2
    assert c.surface_counters()[2] - before == n


@pytest.mark.parametrize("bps", [1, 2])
def test_partner_pair_by_one_launch_and_as_two(bps):
    """Cb / Cr of NV12 and NV16: step 2, one sample apart, in either order -- one launch (8-bit: merged 16-byte stores) == two lone
    components == the oracle"""
    c, rng = U.ctx(), np.random.default_rng(20 + bps)
    for w in WIDTHS:
        for h in HEIGHTS:
            for first in ((0, 1, 2, 3, 5) if bps == 1 else (0, 2, 6)):
                for odd in (False, True):
                    origins, comps, nbytes = geometry(w, h, bps, 2, first, 2, True, odd_pitch=odd)
                    for cs in (comps, comps[::-1]):
                        run_cut(c, rng, w, h, bps, origins, cs, nbytes)
                        run_place(c, rng, w, h, bps, origins, cs, nbytes)
                    run_place(c, rng, w, h, bps, origins, comps, nbytes, one_by_one=True)


@pytest.mark.parametrize("bps", [1, 2])
def test_planes_and_pixels_of_several_components(bps):
    """three planes of their own (I444) and the components of four-channel pixels, each launch placing all of them"""
    c, rng = U.ctx(), np.random.default_rng(30 + bps)
    for w in (17, 65, 130):
        for h in HEIGHTS:
            origins, comps, nbytes = geometry(w, h, bps, 1, 3 * bps, 3, False, odd_pitch=True)
            run_cut(c, rng, w, h, bps, origins, comps, nbytes)
            run_place(c, rng, w, h, bps, origins, comps, nbytes)
            origins, comps, nbytes = geometry(w, h, bps, 4, bps, 3, True, odd_pitch=True)
            run_cut(c, rng, w, h, bps, origins, comps, nbytes)
            run_place(c, rng, w, h, bps, origins, comps, nbytes)


def test_bounds_are_checked_on_the_host():
    c = U.ctx()
    w, h, bps = 17, 5, 1
    origins, comps, nbytes = geometry(w, h, bps, 2, 1, 2, True, odd_pitch=True)
    d_surf = U.to_dev(np.full(nbytes + 64, POISON, np.uint8))
    d_tiles = U.to_dev(np.zeros(2 * 2 * w * h, np.uint8))
    before = c.surface_counters()[2]

    def refused(call, text):
        with pytest.raises(G.SurfaceError) as e:
            call()
        assert e.value.code == -3 and text in e.value.reason, e.value.reason

    place = lambda cs, n, org=origins: c.surface_place_device(d_tiles.data_ptr(), 2, w, h, bps, org, cs, d_surf.data_ptr(), n)
    cut = lambda cs, n, org=origins: c.surface_cut_device(d_surf.data_ptr(), n, cs, bps, 2, w, h, org, d_tiles.data_ptr())
    refused(lambda: place(comps, nbytes - 1), "outside the surface")
    refused(lambda: cut(comps, nbytes - 1), "outside the surface")
    refused(lambda: cut(comps, nbytes, [(0, 0), (w + 3, 3)]), "outside the surface")
    refused(lambda: cut([(comps[0][0], comps[0][1] - 8, 2)], nbytes), "smaller than a row")
    refused(lambda: cut([(comps[0][0], comps[0][1], 5)], nbytes), "step")
    refused(lambda: place([comps[0], comps[0]], nbytes), "share bytes")
    refused(lambda: place([comps[0], (comps[0][0] + 2, comps[0][1], 2)], nbytes + 2), "share bytes")
    with pytest.raises(G.SurfaceError):
        c.surface_place_device(d_tiles.data_ptr(), 2, w, h, 3, origins, comps, d_surf.data_ptr(), nbytes)
    c.synchronize()
    assert c.surface_counters()[2] == before
    assert np.all(d_surf.cpu().numpy() == POISON)
