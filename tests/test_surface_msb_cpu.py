"""CPU: MSB-aligned surfaces in the host planning (grok_amd/csrc/surface_plan.cpp) -- grk_amd_surface_comp::shift, the zero bits below a
sample in its container.  The named formats P016 / P216 against NV12 / NV16 field by field, the rule prec + shift <= 8 * bps and its
reason text, the extent of a surface (a shift moves no byte), and the plan: a run with a shifted component is staged whatever
allow_direct says, every other run keeps the route it had."""
import pytest

import grok_amd as G

INVALID = -3
S420, S422 = [(1, 1), (2, 2), (2, 2)], [(1, 1), (2, 1), (2, 1)]
MSB = {"P016": ("NV12", S420), "P216": ("NV16", S422)}
NAMES = {("P016", 10): "P010", ("P016", 12): "P012", ("P016", 16): "P016", ("P216", 10): "P210", ("P216", 12): "P212", ("P216", 16): "P216"}


def placement(s):
    return [(c.offset, c.row_pitch, c.step) for c in s.comp[:3]]


def layout_fields(l):
    return (l.interleaved, l.channels, l.fill, l.row_pitch, l.plane_pitch)


def with_shifts(surface, shifts):
    return G.Surface.of([(c.offset, c.row_pitch, c.step, sh) for c, sh in zip(surface.comp[:3], shifts)])


@pytest.mark.parametrize("fmt", sorted(MSB))
@pytest.mark.parametrize("size,origin", [((202, 138), (0, 0)), ((7, 5), (0, 0)), ((201, 137), (5, 3))])
def test_p016_p216_are_nv12_nv16_with_a_shift(fmt, size, origin):
    plain, sampling = MSB[fmt]
    number = {"P016": 7, "P216": 8}[fmt]
    layout = G.ImageLayout.make(*size, offset=origin)
    for prec in (10, 12, 16):
        for pitch in (0, (size[0] + 2) // 2 * 4 + 12):
            s, got_sampling, nbytes = G.Surface.make(number, layout, prec, pitch)
            ref, ref_sampling, ref_bytes = G.Surface.make(plain, layout, prec, pitch)
            assert got_sampling == ref_sampling == sampling
            assert placement(s) == placement(ref) and nbytes == ref_bytes, (fmt, prec, pitch)
            assert [c.shift for c in s.comp[:3]] == [16 - prec] * 3 and [c.shift for c in ref.comp[:3]] == [0] * 3
            assert s.comp[3].shift == 0 and placement(s)[0][2] == 1 and placement(s)[1][2] == 2
            # the name: the id and the precision in one; a caller's precision may repeat it, not contradict it
            named, named_sampling, named_bytes = G.Surface.make(NAMES[fmt, prec], layout, pitch=pitch)
            assert bytes(named) == bytes(s) and (named_sampling, named_bytes) == (got_sampling, nbytes)
            assert bytes(G.Surface.make(NAMES[fmt, prec], layout, prec, pitch)[0]) == bytes(s)
            with pytest.raises(ValueError):
                G.Surface.make(NAMES[fmt, prec], layout, 11, pitch)
            if prec == 16:
                assert bytes(s) == bytes(ref)                        # P016 / P216 at 16 bits: NV12 / NV16 themselves
            # the extent and the destination rule do not see the shift
            base = G.TileParams.make(1, 1, 3, prec, 2, mct=False)
            assert G.surface_bytes(layout, base, sampling, s) == nbytes
            assert len(G.surface_plan(layout, base, sampling, s, nbytes, decode=True)) == 2
    for prec in (1, 8):
        with pytest.raises(G.SurfaceError) as e:
            G.Surface.make(number, layout, prec, 0)
        assert e.value.code == INVALID
    with pytest.raises(G.SurfaceError) as e:
        G.Surface.make(9, layout, 10, 0)
    assert e.value.code == INVALID
    assert G.SURFACE_FORMATS_MSB[NAMES[fmt, 10]] == (number, 10)


def test_surface_bytes_with_a_shift():
    layout = G.ImageLayout.make(202, 138)
    p10 = G.TileParams.make(1, 1, 3, 10, 2, mct=False)
    comps = [(0, 512, 1), (138 * 512, 512, 2), (138 * 512 + 2, 512, 2)]
    want = 138 * 512 + 68 * 512 + 101 * 4
    assert G.surface_bytes(layout, p10, S420, G.Surface.of(comps)) == want
    for shifts in ([6, 6, 6], [6, 0, 0], [0, 3, 6], [1, 2, 3]):
        assert G.surface_bytes(layout, p10, S420, G.Surface.of([c + (sh,) for c, sh in zip(comps, shifts)])) == want

    def refused(base, surface):
        with pytest.raises(G.SurfaceError) as e:
            G.surface_bytes(layout, base, S420, surface)
        assert e.value.code == INVALID and "precision plus shift" in e.value.reason, e.value.reason
        with pytest.raises(G.SurfaceError) as e:
            G.surface_plan(layout, base, S420, surface, 1 << 30)
        assert e.value.code == INVALID and "precision plus shift" in e.value.reason

    refused(p10, G.Surface.of([c + (7,) for c in comps]))                          # 10 + 7 > 16
    refused(p10, G.Surface.of([comps[0], comps[1], comps[2] + (7,)]))              # ... one component is enough
    # one-byte samples: 4 bits in the high nibble are fine, 5 bits there are not
    nv12 = [(0, 256, 1), (138 * 256, 256, 2), (138 * 256 + 1, 256, 2)]
    p4 = G.TileParams.make(1, 1, 3, 4, 2, mct=False)
    assert G.surface_bytes(layout, p4, S420, G.Surface.of([c + (4,) for c in nv12])) == 138 * 256 + 68 * 256 + 202
    assert G.surface_bytes(layout, p4, S420, G.Surface.of(nv12)) == 138 * 256 + 68 * 256 + 202
    refused(G.TileParams.make(1, 1, 3, 5, 2, mct=False), G.Surface.of([c + (4,) for c in nv12]))
    refused(G.TileParams.make(1, 1, 3, 16, 2, mct=False), G.Surface.of([c + (1,) for c in comps]))


def test_a_shifted_run_is_never_in_place():
    """(fails on a library without the shift: it reports the Y run of an aligned one-tile P010 surface as in place)"""
    one = G.ImageLayout.make(202, 138)
    p10 = G.TileParams.make(1, 1, 3, 10, 3, mct=False)
    s, sampling, n = G.Surface.make("P010", one, pitch=512)
    nv12, _, n12 = G.Surface.make("NV12", one, 10, 512)
    assert n == n12
    unshifted = with_shifts(s, [0, 0, 0])
    assert bytes(unshifted) == bytes(nv12)
    for decode in (False, True):
        for allow in (True, False):
            plan = G.surface_plan(one, p10, sampling, s, n, base_align=0, decode=decode, allow_direct=allow)
            assert [r[0] for r in plan] == [False, False], (decode, allow)
        # shift = 0: the plan of the 16-bit NV12 surface, field by field
        got = G.surface_plan(one, p10, sampling, unshifted, n, base_align=0, decode=decode, allow_direct=True)
        want = G.surface_plan(one, p10, sampling, nv12, n, base_align=0, decode=decode, allow_direct=True)
        assert [r[0] for r in want] == [True, True]
        assert [(r[0], layout_fields(r[1]), r[2]) for r in got] == [(r[0], layout_fields(r[1]), r[2]) for r in want]
        (_, ly, aty), (_, lc, atc) = got
        assert (ly.interleaved, ly.row_pitch, ly.plane_pitch, aty) == (0, 512, 0, 0)
        assert (lc.interleaved, lc.channels, lc.row_pitch, atc) == (1, 2, 512, 138 * 512)
    # P210 and a planar surface with MSB-aligned samples (I010's planes, shifted) alike
    s2, sampling2, n2 = G.Surface.make("P210", one, pitch=512)
    i420, s420, n420 = G.Surface.make("I420", one, 10, 512)
    for decode in (False, True):
        assert [r[0] for r in G.surface_plan(one, p10, sampling2, s2, n2, decode=decode)] == [False, False]
        assert [r[0] for r in G.surface_plan(one, p10, s420, i420, n420, decode=decode)] == [True, True]
        assert [r[0] for r in G.surface_plan(one, p10, s420, with_shifts(i420, [6, 6, 6]), n420, decode=decode)] == [False, False]


def test_only_the_shifted_run_is_forced_to_staging():
    one = G.ImageLayout.make(202, 138)
    p10 = G.TileParams.make(1, 1, 3, 10, 3, mct=False)
    nv12, sampling, n = G.Surface.make("NV12", one, 10, 512)
    for decode in (False, True):
        want = G.surface_plan(one, p10, sampling, nv12, n, decode=decode)
        got = G.surface_plan(one, p10, sampling, with_shifts(nv12, [6, 0, 0]), n, decode=decode)
        assert [r[0] for r in got] == [False, True]
        assert (layout_fields(got[1][1]), got[1][2]) == (layout_fields(want[1][1]), want[1][2])
        # one shifted partner takes its whole run along, and leaves Y alone
        for shifts in ([0, 6, 0], [0, 0, 6], [0, 6, 6]):
            got = G.surface_plan(one, p10, sampling, with_shifts(nv12, shifts), n, decode=decode)
            assert [r[0] for r in got] == [True, False]
            assert (layout_fields(got[0][1]), got[0][2]) == (layout_fields(want[0][1]), want[0][2])
