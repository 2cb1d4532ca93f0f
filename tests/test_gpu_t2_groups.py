"""-m gpu: the files of layouts whose geometry groups hold tiles of DIFFERENT packet sequences (test_t2_group_plan_cpu.PINNED: every
layout has tiles that same_geometry puts into one grk_amd_encode_tiles batch and whose PCRL / CPRL packet orders differ), on every
route that frames a group with one device plan: grk_amd_encode_image on the device route against the host writer (which builds its
geometry tile by tile and is pinned on the reference's files off the origin by test_precincts_cpu), against the reference where it can
be asked, back through grk_amd_decode_image, through a node of one and of two workers on either Tier-2 route, and the C ABI's
grk_amd_assemble_device as a caller that batches tiles itself meets it.  Content synth.g2, 8 bits, reversible; all five orders,
without markers and with TLM, PLT, SOP and EPH."""
import contextlib
import functools
import os

import numpy as np
import pytest

import grok_amd as G
import gpuutil as U
import refharness as R
import synth
from test_gpu_t2_device import _check
from test_t2_group_plan_cpu import PINNED, pinned, reference_takes_part

pytestmark = pytest.mark.gpu
needs_ref = pytest.mark.skipif(not R.have_ref(), reason="oracle/_ref not built")

NAMES = sorted(PINNED)
MARKERS = G.CS_TLM | G.CS_PLT | G.CS_SOP | G.CS_EPH
cases = pytest.mark.parametrize("name,order,extra", [(n, o, e) for n in NAMES for o in range(5) for e in (0, MARKERS)])


@contextlib.contextmanager
def _env(**kv):
    keep = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in keep.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@functools.lru_cache(maxsize=None)
def _pixels(name):
    layout, base, _ = pinned(name)
    px = synth.g2(base.num_comps, layout.y1 - layout.y0, layout.x1 - layout.x0, 8, seed=NAMES.index(name) + 3)
    px.setflags(write=False)
    return px


@functools.lru_cache(maxsize=None)
def _file(name, order, extra, route):
    """grk_amd_encode_image's file with Tier-2 on the device (GRK_AMD_IMAGE_T2 unset) or from the host writer -- made once, shared"""
    layout, base, _ = pinned(name)
    with _env(GRK_AMD_IMAGE_T2="host" if route == "host" else None):
        return U.ctx().encode_image(layout, base, _pixels(name), G.CS_PROG(order) | extra)


def _same_file(got, want, what):
    """byte for byte; on failure the first differing tile-part and byte (the tile-parts located in the file that is right)"""
    got, want = bytes(got), bytes(want)
    if got == want:
        return
    n = min(len(got), len(want))
    d = np.nonzero(np.frombuffer(got[:n], np.uint8) != np.frombuffer(want[:n], np.uint8))[0]
    first = int(d[0]) if d.size else n
    for off, ln, t in G.locate_tile_parts(want)[0]:
        if off <= first < off + ln:
            raise AssertionError("%s: tile-part %d differs from byte %d of %d (files of %d and %d bytes)" % (what, t, first - off, ln, len(got), len(want)))
    raise AssertionError("%s: differs from byte %d, outside the tile-parts (files of %d and %d bytes)" % (what, first, len(got), len(want)))


@cases
def test_the_device_route_writes_the_host_writers_file(name, order, extra):
    _same_file(_file(name, order, extra, "device"), _file(name, order, extra, "host"), "device route against host writer")


@needs_ref
@pytest.mark.parametrize("name,order,extra", [(n, o, e) for n in NAMES if reference_takes_part(n) for o in range(5) for e in (0, MARKERS)])
def test_both_routes_write_the_reference_file(monkeypatch, name, order, extra):
    layout, base, _ = pinned(name)
    L = base.num_levels
    monkeypatch.setenv("REF_IMG_X0", str(layout.x0))
    monkeypatch.setenv("REF_IMG_Y0", str(layout.y0))
    monkeypatch.setenv("REF_PRECINCTS", ",".join("%d,%d" % (1 << (base.precinct_exp[r] & 15), 1 << (base.precinct_exp[r] >> 4)) for r in range(L, -1, -1)))
    monkeypatch.setenv("REF_PROG_ORDER", str(order))
    monkeypatch.setenv("REF_WRITE_TLM", "1" if extra & G.CS_TLM else "0")
    monkeypatch.setenv("REF_WRITE_PLT", "1" if extra & G.CS_PLT else "0")
    monkeypatch.setenv("REF_CSTY", str((2 if extra & G.CS_SOP else 0) | (4 if extra & G.CS_EPH else 0)))
    want, _ = R.encode(_pixels(name), 8, TW=layout.t_width, TH=layout.t_height, numres=L + 1, mode=1,
                       cblk=(1 << base.cblk_w_exp, 1 << base.cblk_h_exp))
    _same_file(_file(name, order, extra, "host"), want, "host writer against the reference")
    _same_file(_file(name, order, extra, "device"), want, "device route against the reference")


def test_the_reference_takes_part():
    assert sum(reference_takes_part(n) for n in NAMES) >= 2


@cases
def test_the_device_routes_file_decodes_to_the_pixels(name, order, extra):
    assert np.array_equal(U.ctx().decode_image(_file(name, order, extra, "device")), _pixels(name))


@pytest.fixture(scope="module", params=[[0], [0, 0]], ids=["one-worker", "two-workers"])
def node(request):
    nd = G.Node(request.param)
    yield nd
    nd.close()


@pytest.mark.parametrize("name", NAMES)
def test_a_node_writes_the_same_file_on_either_route(node, name):
    layout, base, _ = pinned(name)
    for order in range(5):
        for extra in (0, MARKERS):
            want = _file(name, order, extra, "host")
            for route in (None, "host"):
                with _env(GRK_AMD_NODE_T2=route):
                    got = node.encode_image(layout, base, _pixels(name), G.CS_PROG(order) | extra)
                _same_file(got, want, "node of %d, order %d, flags %d, GRK_AMD_NODE_T2=%s" % (node.size, order, extra, route or "default"))


def test_assemble_device_frames_every_tile_as_a_tile_at_ps_origin():
    """The C ABI as a caller that batches tiles itself uses it: tiles 0 and 2 of "offset-8x8" are one geometry, coded as one batch of
    two under tile 0's parameters and assembled with assemble_device(p0, [0, 2], PCRL).  The documented contract: every tile of the call
    is framed with the packet order of a tile at p0's origin -- tile-part 0 is the host writer's for tile 0, tile-part 1 the host
    writer's for a tile AT TILE 0'S ORIGIN with tile 2's pixels, which is not tile 2's own tile-part; grk_amd_same_tile_packets says
    that the two may not share the call."""
    layout, base, _ = pinned("offset-8x8")
    tiles = G.layout_tiles(layout, base)
    p0, p2 = tiles[0], tiles[2]
    px = _pixels("offset-8x8")
    cut = lambda p: px[:, p.tile_y0 - layout.y0:p.tile_y0 - layout.y0 + p.tile_h, p.tile_x0 - layout.x0:p.tile_x0 - layout.x0 + p.tile_w]
    batch = np.ascontiguousarray(np.stack([cut(p0), cut(p2)]))
    for flags in (G.CS_PROG(3), G.CS_PROG(3) | G.CS_PLT | G.CS_SOP | G.CS_EPH):
        assert G.same_tile_geometry(p0, p2) and not G.same_tile_packets(p0, p2, flags)
        want = _check(p0, batch, [0, 2], flags, ntiles=2)              # (the host writer under p0 for both tiles, byte for byte)
        table, coded = U.ctx().encode_host(p0, batch, ntiles=2)
        bpt = len(table) // 2
        own = G.write_tile_part(p2, 2, table[bpt:], coded, flags)
        assert len(own) == len(want[1]) and own != want[1]
        # ... and under an order the two tiles share, tile 2's own tile-part is what the call writes
        shared = G.CS_PROG(2) | (flags & 0xFF)
        assert G.same_tile_packets(p0, p2, shared)
        assert _check(p0, batch, [0, 2], shared, ntiles=2)[1] == G.write_tile_part(p2, 2, table[bpt:], coded, shared)
