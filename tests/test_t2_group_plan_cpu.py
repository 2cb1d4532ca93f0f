"""CPU: what a geometry group of the whole-image encoders shares is valid for EVERY member of the group, not only for its leader.

grk_amd_encode_image and the node group their tiles (add_unit, image.h), code each group as one grk_amd_encode_tiles batch and have
grk_amd_assemble_device frame the batch with ONE t2_device_plan -- the plan of the group's first tile.  For the position-major
progression orders the packet sequence depends on where a tile lies on the reference grid (the precinct corners of the resolutions
are clipped to the tile, so which of them coincide changes from tile to tile), which same_geometry does not compare: two tiles of one
geometry can need different plans.  Here every tile's own plan is compared with its leader's, through the small driver
tests/c/t2_group_units.cpp -- built on first use with g++ together with geometry.cpp and t2_writer.cpp: no GPU, no HIP -- which takes
the groups from add_unit itself, called the way plain_image calls it.

The pinned layouts (PINNED; tests/test_gpu_t2_groups.py codes the same ones on the device) each hold tiles that same_geometry accepts
as one group and whose PCRL / CPRL sequences differ.  The sweep draws layouts with image offsets and tile-grid offsets and asserts the
same property, with conditions on what it has to contain so that it cannot pass by missing the case."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import grok_amd as G
from test_offgrid_cpu import ref_defects

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_lib = None

# name: image area [x0, x1) x [y0, y1), tile grid origin, tile size, components, levels, code-block exponents, precinct exponents
# (one pair: every resolution; else r = 0 .. levels), pairs of tiles of one geometry whose PCRL and CPRL sequences differ
PINNED = {
    # image offset only, 64 x 64 blocks, precincts 8 x 8: tiles 0 / 2 are 244 x 16 (402 packets), tiles 1 / 3 are 46 x 16 (93 packets)
    "offset-8x8": ((48, 338, 30, 62), (0, 0), (292, 46), 3, 2, (6, 6), [(3, 3)], [(0, 2), (1, 3)]),
    "offset-16x16": ((134, 591, 191, 255), (0, 0), (157, 223), 3, 2, (6, 6), [(4, 4)], [(0, 4), (1, 5), (2, 6), (3, 7)]),
    # one component, 32 x 32 blocks, tiles 16 wide.  (The image starts at y = 74, not at 76 or 75, where the first row of tiles would be
    # one or two samples high: for those tiles the reference's PLT lengths do not add up to its own tile-part -- 12, 12, 27, 21, 24, 23
    # for packets of 12, 6, 9, 7, 8, 8 bytes --, while its packets and this writer's PLT agree with the tile-part; a layout that is to
    # be compared with the reference's files under PLT has to stay clear of that.)
    "offset-1comp-32x32-blocks": ((13, 45, 74, 274), (0, 0), (29, 77), 1, 2, (5, 5), [(3, 3)], [(0, 1), (2, 3), (4, 5), (6, 7)]),
    # image and tile grid at one offset, five levels
    "grid-at-image": ((236, 748, 142, 465), (236, 142), (256, 323), 3, 5, (6, 6), [(4, 4)], [(0, 1)]),
    # image offset and tile-grid offset, different
    "grid-and-image": ((274, 502, 172, 545), (254, 126), (64, 200), 1, 2, (4, 4), [(5, 5)], [(1, 2)]),
    # ... with precincts that are not square and differ from resolution to resolution, 17-sample-wide tiles
    "grid-and-image-nonsquare": ((159, 221, 193, 270), (156, 176), (17, 200), 3, 2, (5, 6), [(4, 5), (4, 5), (1, 7)], [(0, 3)]),
}


def pinned(name):
    """-> (ImageLayout, base TileParams, divergent pairs)"""
    (x0, x1, y0, y1), (tx0, ty0), (tw, th), nc, L, cblk, prc, pairs = PINNED[name]
    layout = G.ImageLayout(x0, y0, x1, y1, tx0, ty0, tw, th)
    base = G.TileParams.make(1, 1, nc, 8, L, cblk=cblk, precincts=prc * (L + 1) if len(prc) == 1 else prc)
    return layout, base, pairs


def reference_takes_part(name):
    """The reference's encoder can be asked for this layout's file: its tile grid is anchored at the origin, the precinct sizes follow
    its own rule (one size at every resolution here) and the layout does not run into its defect D13 (test_offgrid_cpu.ref_defects)."""
    layout, base, _ = pinned(name)
    return (layout.tx0, layout.ty0) == (0, 0) and len(PINNED[name][6]) == 1 and not ref_defects(layout, base.num_levels)[0]


def lib():
    global _lib
    if _lib is None:
        csrc = os.path.join(ROOT, "grok_amd", "csrc")
        out = os.path.join(tempfile.mkdtemp(prefix="t2_group_units_"), "libt2_group_units.so")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-D_GLIBCXX_ASSERTIONS", "-fPIC", "-shared",
                               os.path.join(HERE, "c", "t2_group_units.cpp"), os.path.join(csrc, "geometry.cpp"),
                               os.path.join(csrc, "t2_writer.cpp"), "-o", out, "-Wl,--no-undefined", "-lpthread"])
        _lib = C.CDLL(out)
        _lib.t2g_layout.restype = C.c_int64
    return _lib


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def groups_and_plans(layout, base, flags):
    """-> ([tile] its group as add_unit makes them under the flags' order, [tile] its own t2_device_plan, flattened)"""
    n = G.lib().grk_amd_layout_num_tiles(C.byref(layout))
    group, at = np.zeros(n, np.uint32), np.zeros(n + 1, np.uint64)
    assert lib().t2g_layout(C.byref(layout), C.byref(base), flags, ptr(group), None, C.c_uint64(0), ptr(at)) == n
    flat = np.zeros(int(at[n]), np.uint32)
    assert lib().t2g_layout(C.byref(layout), C.byref(base), flags, ptr(group), ptr(flat), C.c_uint64(flat.size), ptr(at)) == n
    return [int(g) for g in group], [flat[int(at[t]):int(at[t + 1])] for t in range(n)]


def same_sequence(a, b, order):
    rc = lib().t2g_same_sequence(C.byref(a), C.byref(b), order)
    assert rc in (0, 1), rc
    return bool(rc)


@pytest.mark.parametrize("order", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("name", sorted(PINNED))
def test_every_member_of_a_group_has_its_leaders_plan(name, order):
    layout, base, _ = pinned(name)
    for flags in (G.CS_PROG(order), G.CS_PROG(order) | G.CS_TLM | G.CS_PLT | G.CS_SOP | G.CS_EPH):
        group, plans = groups_and_plans(layout, base, flags)
        for t, g in enumerate(group):
            lead = group.index(g)
            if not np.array_equal(plans[t], plans[lead]):
                n = min(plans[t].size, plans[lead].size)
                first = int(np.nonzero(plans[t][:n] != plans[lead][:n])[0][0]) if not np.array_equal(plans[t][:n], plans[lead][:n]) else n
                raise AssertionError("%s, order %d: tile %d is in the group of tile %d, but its own plan differs from word %d on (packet %d; "
                                     "%d and %d words)" % (name, order, t, lead, first, first // 14, plans[t].size, plans[lead].size))


@pytest.mark.parametrize("name", sorted(PINNED))
def test_pinned_layouts_diverge_where_they_are_said_to_and_group_no_finer_than_they_must(name):
    """What makes the layouts worth pinning: the named pairs are one geometry, their sequences agree for LRCP, RLCP and RPCL and differ for
    PCRL and CPRL -- and grk_amd_same_tile_packets says exactly that.  For orders 0 and 1 the groups stay same_geometry's."""
    layout, base, pairs = pinned(name)
    tiles = G.layout_tiles(layout, base)
    for a, b in pairs:
        assert G.same_tile_geometry(tiles[a], tiles[b]), (a, b)
        for order in range(5):
            assert same_sequence(tiles[a], tiles[b], order) == (order <= 2), (a, b, order)
            assert G.same_tile_packets(tiles[a], tiles[b], G.CS_PROG(order)) == (order <= 2), (a, b, order)
    for order in range(5):
        group, _ = groups_and_plans(layout, base, G.CS_PROG(order))
        for a in range(len(tiles)):
            for b in range(a + 1, len(tiles)):
                geo = G.same_tile_geometry(tiles[a], tiles[b])
                want = geo and (order <= 1 or same_sequence(tiles[a], tiles[b], order))
                assert (group[a] == group[b]) == want, (order, a, b)
                assert G.same_tile_packets(tiles[a], tiles[b], G.CS_PROG(order)) == want, (order, a, b)


def test_the_predicate_counts_components_and_passes_errors_on():
    a = G.TileParams.make(64, 64, 3, 8, 2)
    b = G.TileParams.make(64, 64, 1, 8, 2)
    assert G.same_tile_geometry(a, b) and not G.same_tile_packets(a, b, G.CS_PROG(3)) and not G.same_tile_packets(a, b, 0)
    assert G.same_tile_packets(a, G.TileParams.make(64, 64, 3, 8, 2, origin=(64, 128)), G.CS_PROG(4))
    assert not G.same_tile_packets(a, G.TileParams.make(64, 63, 3, 8, 2), 0)
    with pytest.raises(ValueError):
        G.same_tile_packets(a, G.TileParams.make(64, 64, 3, 8, 40), 0)


def test_enough_pinned_layouts_meet_the_reference():
    """The GPU tests compare a pinned layout's files with the reference's where reference_takes_part: at least two must."""
    assert sum(reference_takes_part(name) for name in PINNED) >= 2


SWEEP_SEED, SWEEP_DRAWS, SWEEP_MAX_TILES = 20261020, 2000, 40


def test_sweep_of_layouts_every_member_has_its_leaders_plan():
    """t2g_sweep (tests/c/t2_group_units.cpp says what it draws): for all five orders every tile's own plan is its group leader's;
    orders 0 and 1 group as same_geometry does, and so do all five for layouts with image and tile grid at the origin;
    grk_amd_same_tile_packets is same_geometry and equal sequences.  The conditions keep the sweep from passing by missing the case:
    at least 12 pairs of one geometry whose PCRL sequences differ, at least 1 000 whose sequences agree, every kind of layout."""
    out = np.zeros(24, np.uint64)
    msg = C.create_string_buffer(1024)
    rc = lib().t2g_sweep(C.c_uint64(SWEEP_SEED), SWEEP_DRAWS, SWEEP_MAX_TILES, ptr(out), msg, 1024)
    o = [int(v) for v in out]
    said = ("%d layouts kept of %d draws (at the origin %d, image offset only %d, tile grid at the image offset %d, both and different %d; "
            "%d failed to build); %d pairs of one geometry: PCRL sequences agree for %d and differ for %d (RPCL %d, CPRL %d); members whose "
            "plan is not the leader's, by order: %s; pairs grouped other than same_geometry where they must be, by order: %s; pairs where "
            "the predicate disagrees: %d; first failure: %s"
            % (o[0], SWEEP_DRAWS, o[1], o[2], o[3], o[4], o[21], o[5], o[6], o[7], o[19], o[20], o[8:13], o[13:18], o[18],
               msg.value.decode() or "none"))
    print(said)
    assert rc == 0 and o[21] == 0, said
    assert o[8:13] == [0] * 5, said
    assert o[13:18] == [0] * 5, said
    assert o[18] == 0, said
    assert o[7] >= 12 and o[6] >= 1000 and o[5] == o[6] + o[7], said
    assert min(o[2], o[3], o[4]) >= 1 and o[1] >= 1, said
