"""GPU: grk_amd_encode_surface / grk_amd_decode_surface -- whole images from and to video surfaces (NV12, NV21, I420, YV12, NV16,
I444, RGBX-style pixels, 4:2:0 plus a full-size fourth component), each as a host surface and as a device surface, with
GRK_AMD_SURFACE_DIRECT unset and = 0.  Encode: the file's bytes == grk_amd_encode_image_subsampled of the same samples gathered into
tight planes (all factors 1: == grk_amd_encode_image).  Decode: the samples on the surface == grk_amd_decode_image's planes and every
other byte of a poisoned buffer is unchanged.  All comparisons are exact."""
import ctypes as C

import numpy as np
import pytest

import grok_amd as G
import gpuutil as U
import refharness as R
import synth
from test_gpu_decode_image import _forged_8bit_stream
from test_t2_reader_cpu import REF_VARS
from test_t2_reader_subsampled_cpu import make_planes, ref_subsampled_stream

pytestmark = pytest.mark.gpu
needs_ref = pytest.mark.skipif(not R.have_ref(), reason="oracle/_ref (the real reference) not built here")
UNSUPPORTED, INVALID, OVERFLOW = -2, -3, -5
W, H, LEVELS = 202, 138, 3
S444 = [(1, 1)] * 3


def rgbx(layout, prec, pitch):
    bps = (prec + 7) // 8
    w, h = layout.x1 - layout.x0, layout.y1 - layout.y0
    pitch = pitch or w * 4 * bps
    return G.Surface.of([(k * bps, pitch, 4) for k in range(3)]), S444, h * pitch


def nv12_alpha(layout, prec, pitch):
    """NV12 and, behind it, a full-size fourth plane"""
    s, sampling, n = G.Surface.make("NV12", layout, prec, pitch)
    at = (n + 63) // 64 * 64
    s.comp[3] = G.SurfaceComp(at, s.comp[0].row_pitch, 1, 0)
    return s, sampling + [(1, 1)], at + (layout.y1 - layout.y0 - 1) * s.comp[0].row_pitch + (layout.x1 - layout.x0) * ((prec + 7) // 8)


def named(fmt):
    return lambda layout, prec, pitch: G.Surface.make(fmt, layout, prec, pitch)


# name: (surface builder, luma pitch, colour transform)
SURFACES = {
    "nv12-p256": (named("NV12"), 256, False),
    "nv21": (named("NV21"), 0, False),
    "i420": (named("I420"), 0, False),
    "i420-p256": (named("I420"), 256, False),
    "yv12": (named("YV12"), 0, False),
    "nv16": (named("NV16"), 0, False),
    "i444-p256-mct": (named("I444"), 256, True),
    "rgbx-mct": (rgbx, 0, True),
    "nv12-alpha": (nv12_alpha, 208, False),
}
# name: (surface, tile, origin, prec)
CASES = {}
for _s in SURFACES:
    CASES[_s] = (_s, None, (0, 0), 8)
    CASES[_s + "-t64x48"] = (_s, (64, 48), (0, 0), 8)
CASES["nv12-origin53"] = ("nv12-p256", None, (5, 3), 8)
CASES["nv12-origin53-t64x48"] = ("nv12-p256", (64, 48), (5, 3), 8)
CASES["nv12-12bit"] = ("nv12-p256", None, (0, 0), 12)
CASES["i420-12bit-t64x48"] = ("i420", (64, 48), (0, 0), 12)
_made = {}


def case(name):
    """(layout, base, sampling, surface, bytes, planes, bps, the file of the planes by encode_image_subsampled, its decode_image
    planes) -- made once, left unchanged"""
    if name not in _made:
        sname, tile, origin, prec = CASES[name]
        build, pitch, mct = SURFACES[sname]
        bps = (prec + 7) // 8
        layout = G.ImageLayout.make(W, H, *(tile or (None, None)), offset=origin)
        surface, sampling, nbytes = build(layout, prec, pitch * bps)
        base = G.TileParams.make(1, 1, len(sampling), prec, LEVELS, mct=mct)
        planes = make_planes(layout, sampling, prec, seed=len(name))
        assert G.surface_bytes(layout, base, sampling, surface) <= nbytes
        c = U.ctx()
        cs = c.encode_image_subsampled(layout, base, sampling, planes, G.CS_PLT)
        back = c.decode_image_planes(cs)
        assert all(np.array_equal(a, b) for a, b in zip(back, planes))
        _made[name] = (layout, base, sampling, surface, nbytes, planes, bps, cs, back)
    return _made[name]


def surface_of(name, seed=0):
    """the planes on their surface, in a buffer whose other bytes are random"""
    layout, base, sampling, surface, nbytes, planes, bps, cs, back = case(name)
    buf = np.random.default_rng(seed).integers(0, 256, nbytes, dtype=np.uint8)
    surface.scatter(buf, planes, bps)
    return buf


def direct(monkeypatch, on):
    if on:
        monkeypatch.delenv("GRK_AMD_SURFACE_DIRECT", raising=False)
    else:
        monkeypatch.setenv("GRK_AMD_SURFACE_DIRECT", "0")


@pytest.mark.parametrize("name", sorted(CASES))
def test_encode_surface_equals_encode_image_subsampled(monkeypatch, name):
    layout, base, sampling, surface, nbytes, planes, bps, want, _ = case(name)
    c = U.ctx()
    buf = surface_of(name)
    sizes = [pl.shape[::-1] for pl in planes]
    assert all(np.array_equal(a, b) for a, b in zip(surface.gather(buf, sizes, bps), planes))
    d_buf = U.to_dev(buf)
    one_tile = CASES[name][1] is None
    for on in (True, False):
        direct(monkeypatch, on)
        before = c.surface_counters()
        assert c.encode_surface(layout, base, sampling, surface, buf, G.CS_PLT) == want, (name, on, "host")
        assert c.encode_surface(layout, base, sampling, surface, d_buf.data_ptr(), G.CS_PLT, cap=nbytes) == want, (name, on, "device")
        after = c.surface_counters()
        if not (on and one_tile):
            assert after[0] == before[0] and after[1] > before[1] and after[2] > before[2]          # all staged
        else:
            assert after[0] > before[0]
    assert np.array_equal(d_buf.cpu().numpy(), buf)                                                 # an encode only reads
    if all(s == (1, 1) for s in sampling):
        assert c.encode_image(layout, base, np.stack(planes), G.CS_PLT) == want


@pytest.mark.parametrize("name", sorted(CASES))
def test_decode_surface_equals_decode_image(monkeypatch, name):
    layout, base, sampling, surface, nbytes, planes, bps, cs, back = case(name)
    c = U.ctx()
    poison = np.random.default_rng(5).integers(0, 256, nbytes, dtype=np.uint8)
    want = poison.copy()
    surface.scatter(want, back, bps)
    assert not np.array_equal(want, poison)
    sizes = [pl.shape[::-1] for pl in planes]
    for on in (True, False):
        direct(monkeypatch, on)
        host = poison.copy()
        c.decode_surface(cs, surface, host)
        assert all(np.array_equal(a, b) for a, b in zip(surface.gather(host, sizes, bps), back)), (name, on, "host")
        assert np.array_equal(host, want), (name, on, "host: a byte that is no sample changed")
        dev = U.to_dev(poison)
        c.decode_surface(cs, surface, dev.data_ptr(), cap=nbytes)          # (cap: exactly the buffer)
        c.decode_status()
        assert np.array_equal(dev.cpu().numpy(), want), (name, on, "device")


@pytest.mark.parametrize("name", ["nv12-p256", "nv21", "nv12-p256-t64x48"])
def test_cap_is_checked_before_anything_is_written(name):
    layout, base, sampling, surface, nbytes, planes, bps, cs, back = case(name)
    c = U.ctx()
    need = G.surface_bytes(layout, base, sampling, surface)
    poison = np.full(need, 0x5A, np.uint8)
    dev = U.to_dev(poison)
    c.decode_surface(cs, surface, dev.data_ptr(), cap=need)                # exactly grk_amd_surface_bytes: fine
    c.decode_status()
    sizes = [pl.shape[::-1] for pl in planes]
    assert all(np.array_equal(a, b) for a, b in zip(surface.gather(dev.cpu().numpy(), sizes, bps), back))
    dev = U.to_dev(poison)
    before = c.surface_counters()
    with pytest.raises(G.SurfaceError) as e:
        c.decode_surface(cs, surface, dev.data_ptr(), cap=need - 1)
    assert e.value.code == OVERFLOW
    host = poison.copy()
    with pytest.raises(G.SurfaceError) as e:
        c.decode_surface(cs, surface, host, cap=need - 1)
    assert e.value.code == OVERFLOW
    c.synchronize()
    assert np.array_equal(dev.cpu().numpy(), poison) and np.array_equal(host, poison) and c.surface_counters() == before
    with pytest.raises(G.SurfaceError) as e:
        c.encode_surface(layout, base, sampling, surface, surface_of(name)[:need], cap=need - 1)
    assert e.value.code == OVERFLOW and c.surface_counters() == before


def test_counters(monkeypatch):
    c = U.ctx()
    layout, base, sampling, surface, nbytes, planes, bps, cs, back = case("nv12-p256")
    d_buf = U.to_dev(surface_of("nv12-p256"))
    assert d_buf.data_ptr() % 4 == 0

    def delta(call):
        before = c.surface_counters()
        call()
        c.decode_status()
        return tuple(a - b for a, b in zip(c.surface_counters(), before))

    enc = lambda: c.encode_surface(layout, base, sampling, surface, d_buf.data_ptr(), cap=nbytes)
    dec = lambda: c.decode_surface(cs, surface, d_buf.data_ptr(), cap=nbytes)
    direct(monkeypatch, True)
    assert delta(enc) == (2, 0, 0) and delta(dec) == (2, 0, 0)             # NV12, one tile: Y and Cb/Cr in place, no kernel of ours
    direct(monkeypatch, False)
    assert delta(enc) == (0, 2, 2) and delta(dec) == (0, 2, 2)
    direct(monkeypatch, True)
    # a device surface off 4-byte alignment: the decode is staged, the encode still in place
    odd = U.to_dev(np.concatenate([np.zeros(1, np.uint8), surface_of("nv12-p256")]))
    assert delta(lambda: c.encode_surface(layout, base, sampling, surface, odd.data_ptr() + 1, cap=nbytes)) == (2, 0, 0)
    assert delta(lambda: c.decode_surface(cs, surface, odd.data_ptr() + 1, cap=nbytes)) == (0, 2, 2)
    # NV21: the pairs are reversed -- chroma staged
    l2, b2, s2, surf2, n2, _, _, cs2, _ = case("nv21")
    d2 = U.to_dev(surface_of("nv21"))
    assert delta(lambda: c.encode_surface(l2, b2, s2, surf2, d2.data_ptr(), cap=n2)) == (1, 1, 1)
    assert delta(lambda: c.decode_surface(cs2, surf2, d2.data_ptr(), cap=n2)) == (1, 1, 1)
    # tiles: every unit staged (4 x 3 tiles of two runs)
    l3, b3, s3, surf3, n3, _, _, cs3, _ = case("nv12-p256-t64x48")
    d3 = U.to_dev(surface_of("nv12-p256-t64x48"))
    for got in (delta(lambda: c.encode_surface(l3, b3, s3, surf3, d3.data_ptr(), cap=n3)), delta(lambda: c.decode_surface(cs3, surf3, d3.data_ptr(), cap=n3))):
        assert got[0] == 0 and got[1] == 4 * 3 * 2 and got[2] >= 2


def test_odd_device_base_gives_the_same_samples():
    """the surface one byte into an allocation: every path off its alignment"""
    c = U.ctx()
    for name in ("nv12-p256", "i420", "nv12-p256-t64x48"):
        layout, base, sampling, surface, nbytes, planes, bps, cs, back = case(name)
        buf = surface_of(name, seed=3)
        d = U.to_dev(np.concatenate([np.full(1, 7, np.uint8), buf, np.full(3, 7, np.uint8)]))
        assert c.encode_surface(layout, base, sampling, surface, d.data_ptr() + 1, G.CS_PLT, cap=nbytes) == cs
        poison = np.full(nbytes + 4, 0xC3, np.uint8)
        want = poison.copy()
        surface.scatter(want[1:], back, bps)
        d = U.to_dev(poison)
        c.decode_surface(cs, surface, d.data_ptr() + 1, cap=nbytes)
        c.decode_status()
        assert np.array_equal(d.cpu().numpy(), want), name


def test_context_state_is_left_alone():
    c = U.ctx()
    layout, base, sampling, surface, nbytes, planes, bps, cs, back = case("nv12-p256")
    buf = surface_of("nv12-p256")
    # the context's own layouts: an interleaved RGBX encode / decode of a tile before and after
    p = G.TileParams.make(64, 48, 3, 8, 2)
    px = np.ascontiguousarray(np.concatenate([synth.g2(3, 48, 64, 8), np.full((1, 48, 64), 77, np.uint8)]).transpose(1, 2, 0))      # (H, W, RGBX)
    lay = G.PixelLayout.make(True, 4, fill=200)
    c.set_pixel_layout(lay)
    c.set_decode_pixel_layout(lay)
    c.set_decode_upsample(True)
    def decode_raw(table, coded):
        """grk_amd_decode_tiles in whatever layout the CONTEXT holds (the binding's decode_host sets one of its own)"""
        out = np.full(G.pixel_bytes(p, lay), 3, np.uint8)
        t = np.ascontiguousarray(table)
        c._check(c._L.grk_amd_decode_tiles(c._h, C.byref(p), 1, t.ctypes.data, coded.ctypes.data, coded.size, 0, out.ctypes.data, 0), "decode_tiles")
        return out

    try:
        table, coded = c.encode_host(p, px)
        first = decode_raw(table, coded)
        assert np.array_equal(first.reshape(48, 64, 4)[:, :, :3], px[:, :, :3]) and np.all(first.reshape(48, 64, 4)[:, :, 3] == 200)
        up_before = c.decode_image(cs, layout=lay)                     # (upsampling on: the image on the reference grid, in the layout)
        assert up_before.size == W * H * 4
        assert c.encode_surface(layout, base, sampling, surface, buf, G.CS_PLT) == cs
        host = buf.copy()
        c.decode_surface(cs, surface, host)
        assert np.array_equal(host, buf)                               # (lossless: the surface decodes onto itself)
        t2, c2 = c.encode_host(p, px)
        assert U.split_blocks(t2, c2) == U.split_blocks(table, coded) and np.array_equal(t2["missing_msbs"], table["missing_msbs"])   # (the arena's order is free)
        assert np.array_equal(decode_raw(table, coded), first)
        assert np.array_equal(c.decode_image(cs, layout=lay), up_before)
        # encode_image_subsampled with a layout set is refused as before
        with pytest.raises(RuntimeError, match=r"failed: -2"):
            c.encode_image_subsampled(layout, base, sampling, planes)
    finally:
        c.set_pixel_layout(None)
        c.set_decode_pixel_layout(None)
        c.set_decode_upsample(False)
    # QCD words the caller set survive the call
    pi = G.TileParams.make(64, 48, 3, 8, 2, irreversible=True)
    tpx = synth.g2(3, 48, 64, 8)
    table, coded = c.encode_host(pi, tpx)
    plain = c.decode_host(pi, table, coded)[0]
    _, words = G.tile_layout(pi)
    c.set_decode_qcd([w - (1 << 11) for w in words])
    try:
        other = c.decode_host(pi, table, coded)[0]
        assert not np.array_equal(other, plain)
        c.decode_surface(cs, surface, buf.copy())
        assert np.array_equal(c.decode_host(pi, table, coded)[0], other)
    finally:
        c.set_decode_qcd([])
    assert np.array_equal(c.decode_host(pi, table, coded)[0], plain)
    # a context with a decode reduce or a decode sequence is refused
    c.set_decode_reduce(1)
    try:
        with pytest.raises(G.SurfaceError) as e:
            c.decode_surface(cs, surface, buf.copy())
        assert e.value.code == UNSUPPORTED and "reduced" in e.value.reason
    finally:
        c.set_decode_reduce(0)
    k = G.Context(0)
    try:
        k.set_decode_pipelining(2)
        with pytest.raises(G.SurfaceError) as e:
            k.decode_surface(cs, surface, buf.copy())
        assert e.value.code == UNSUPPORTED and "sequence" in e.value.reason
    finally:
        k.close()
    # components of a destination that share bytes
    bad = G.Surface.of([(0, 256, 1), (138 * 256, 256, 2), (138 * 256, 256, 2)])
    with pytest.raises(G.SurfaceError) as e:
        c.decode_surface(cs, bad, buf.copy())
    assert e.value.code == INVALID and "share bytes" in e.value.reason
    assert len(c.encode_surface(layout, base, sampling, bad, buf)) > 0          # (an encode only reads)


@pytest.mark.parametrize("tiles", [1, 2])
def test_int16_plane_rule_per_group(tiles):
    """a stream whose values leave the int16 planes: a host surface repeats the group with int32 planes by itself, a device
    surface reports through decode_status"""
    cs, want = _forged_8bit_stream(tiles)
    c = U.ctx()
    h, w = want.shape[1:]
    surface = G.Surface.of([(64, w + 19, 1)])
    n = 64 + (h - 1) * (w + 19) + w
    host = np.full(n, 9, np.uint8)
    c.decode_surface(cs, surface, host)
    assert np.array_equal(surface.gather(host, [(w, h)], 1)[0], want[0])
    dev = U.to_dev(np.full(n, 9, np.uint8))
    c.decode_surface(cs, surface, dev.data_ptr(), cap=n)
    with pytest.raises(RuntimeError, match="16-bit planes"):
        c.decode_status()
    c.set_decode_planes16(False)
    try:
        c.decode_surface(cs, surface, dev.data_ptr(), cap=n)
        c.decode_status()
    finally:
        c.set_decode_planes16(True)
    assert np.array_equal(dev.cpu().numpy(), host)


@needs_ref
def test_reference_reads_an_nv12_file_and_its_streams_decode_onto_surfaces(monkeypatch):
    c = U.ctx()
    layout, base, sampling, surface, nbytes, planes, bps, cs, back = case("nv12-p256")
    got = c.encode_surface(layout, base, sampling, surface, surface_of("nv12-p256"))
    for a, b in zip(R.decode_planes(got, sampling, W, H), planes):
        assert np.array_equal(a, b.astype(np.int32))
    # streams the reference encoder wrote: HT (refharness.encode_planes), and Part-1 reversible (encode_planes writes HT only: the
    # same encoder through the reader tests' helper) -- in tiles, so that both routes meet them
    for k in REF_VARS:
        monkeypatch.delenv(k, raising=False)
    streams = [R.encode_planes(planes, sampling, 8, W, H, numres=LEVELS + 1),
               ref_subsampled_stream(monkeypatch, planes, sampling, 8, W, H, numres=LEVELS + 1, ht=0),
               ref_subsampled_stream(monkeypatch, planes, sampling, 8, W, H, None, 64, 48, numres=LEVELS + 1, ht=0)]
    assert G.read_header(streams[1]).base.reserved[0] == 1
    for ref_cs in streams:
        poison = np.full(nbytes, 0x3C, np.uint8)
        want = poison.copy()
        surface.scatter(want, planes, bps)
        host = poison.copy()
        c.decode_surface(ref_cs, surface, host)
        assert np.array_equal(host, want)
        dev = U.to_dev(poison)
        c.decode_surface(ref_cs, surface, dev.data_ptr(), cap=nbytes)
        c.decode_status()
        assert np.array_equal(dev.cpu().numpy(), want)
