"""GPU: packed 4:2:2 frames -- YUY2, UYVY, YVYU, Y216 (at 10 and 16 bits), v210 -- with the numpy reference tests/packedref.py as the
oracle of the formats.  The two kernels alone (grk_amd_packed_unpack_device / grk_amd_packed_pack_device): KU's planes, and KK onto a
canvas of random bytes with the WHOLE buffer compared, so a byte written that is no sample shows; widths with every head and tail,
the frame at several alignments inside one torch buffer.  Then the whole calls: grk_amd_encode_packed's file ==
grk_amd_encode_image_subsampled's of the same samples as planes, from host and device frames, in place (one tile) and staged (tiles);
grk_amd_decode_packed == the reference's pack of grk_amd_decode_image's planes onto the canvas; the rate-targeted call ==
grk_amd_encode_image_subsampled_rate's file; the refusals that need a context; a v210 round trip.  All comparisons are exact."""
import numpy as np
import pytest

import grok_amd as G
import gpuutil as U
import packedref as R

pytestmark = pytest.mark.gpu
UNSUPPORTED, INVALID, OVERFLOW = -2, -3, -5
S422 = [(1, 1), (2, 1), (2, 1)]
FORMATS = [(R.YUY2, 8), (R.UYVY, 8), (R.YVYU, 8), (R.Y216, 10), (R.Y216, 16), (R.V210, 10)]
IDS = ["%s-%d" % (R.NAMES[f], p) for f, p in FORMATS]
POISON = 0xA5
# a one-tile image (its planes go to the tile coder in place) and one of odd width in tiles with partial ones (staged units)
SHAPES = {"one": (50, 20, None), "tiled": (70, 37, (32, 32))}
LEVELS = 2
_made = {}


def random_planes(rng, w, h, prec):
    dt = np.uint8 if prec <= 8 else np.uint16
    cw = (w + 1) // 2
    return [rng.integers(0, 1 << prec, (h, n)).astype(dt) for n in (w, cw, cw)]


def case(shape, prec, flags=G.CS_PLT):
    """(layout, base, planes, the planes' file by encode_image_subsampled, its decode_image planes) -- made once, left unchanged"""
    key = (shape, prec, flags)
    if key not in _made:
        w, h, tile = SHAPES[shape]
        layout = G.ImageLayout.make(w, h, *(tile or (None, None)))
        base = G.TileParams.make(1, 1, 3, prec, LEVELS, mct=False)
        planes = random_planes(np.random.default_rng(1000 + 17 * prec + w), w, h, prec)
        c = U.ctx()
        cs = c.encode_image_subsampled(layout, base, S422, planes, flags)
        back = c.decode_image_planes(cs)
        assert all(np.array_equal(a, b) for a, b in zip(back, planes))
        _made[key] = (layout, base, planes, cs, back)
    return _made[key]


def pitch_of(fmt, shape):
    """the default pitch for the one-tile shape, a larger one on the format's alignment for the tiled"""
    w = SHAPES[shape][0]
    return 0 if shape == "one" else R.default_pitch(fmt, w) + 48


def noisy_frame(fmt, prec, planes, pitch, seed):
    """the planes packed onto random bytes, the bits an encode ignores set at random too"""
    h, w = planes[0].shape
    rng = np.random.default_rng(seed)
    frame = R.pack(fmt, prec, *planes, pitch, rng.integers(0, 256, R.frame_bytes(fmt, w, h, pitch), dtype=np.uint8))
    p, row = pitch or R.default_pitch(fmt, w), R.row_bytes(fmt, w)
    for y in range(h):
        r = frame[y * p:y * p + row]
        if fmt == R.Y216:
            low = (1 << (16 - prec)) - 1
            r[0::2] |= rng.integers(0, 256, row // 2, dtype=np.uint8) & (low & 0xFF)
            r[1::2] |= rng.integers(0, 256, row // 2, dtype=np.uint8) & (low >> 8)
        if fmt == R.V210:
            r[3::4] |= rng.integers(0, 4, row // 4, dtype=np.uint8) << 6
            # the last block's fields past the width
            last = r[row - 16:].view("<u4")
            for table, n in ((R.V210_Y, w), (R.V210_CB, (w + 1) // 2), (R.V210_CR, (w + 1) // 2)):
                for k, (word, field) in enumerate(table):
                    if (row // 16 - 1) * len(table) + k >= n:
                        last[word] |= int(rng.integers(0, 1024)) << (10 * field)
    assert all(np.array_equal(a, b) for a, b in zip(R.unpack(fmt, prec, frame, w, h, pitch), planes))
    return frame


# ---- 1. the kernels alone ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,prec", FORMATS, ids=IDS)
def test_kernels_alone(fmt, prec):
    c, rng = U.ctx(), np.random.default_rng(10 * fmt + prec)
    bps, h = 1 if prec <= 8 else 2, 17
    before = c.packed_counters()
    launches = 0
    for w in (1, 6, 7, 49, 97):
        cw = (w + 1) // 2
        nplanes = (w + 2 * cw) * h * bps
        for base in (0, 1, 2, 16):
            if base % R.align(fmt):
                continue
            for pitch in (R.default_pitch(fmt, w), R.default_pitch(fmt, w) + 3 * 16):
                nbytes = R.frame_bytes(fmt, w, h, pitch)
                # KU: a frame of random bytes (what an encode ignores included) -> planes, nothing written beside them
                buf = rng.integers(0, 256, base + nbytes + 32, dtype=np.uint8)
                d_buf, d_planes = U.to_dev(buf), U.to_dev(np.full(nplanes + 64, POISON, np.uint8))
                c.packed_unpack_device(fmt, prec, w, h, d_buf.data_ptr() + base, pitch, nbytes, d_planes.data_ptr() + 32, nplanes)
                c.synchronize()
                got = d_planes.cpu().numpy()
                want = np.concatenate([p.reshape(-1).view(np.uint8) for p in R.unpack(fmt, prec, buf[base:base + nbytes], w, h, pitch)])
                assert np.array_equal(got[32:32 + nplanes], want), ("unpack", w, base, pitch)
                assert np.all(got[:32] == POISON) and np.all(got[32 + nplanes:] == POISON), ("unpack wrote beside the planes", w, base, pitch)
                assert np.array_equal(d_buf.cpu().numpy(), buf)
                # KK: planes of the full range onto a canvas of random bytes, the whole buffer compared
                planes = random_planes(rng, w, h, prec)
                flat = np.concatenate([p.reshape(-1).view(np.uint8) for p in planes])
                canvas = rng.integers(0, 256, base + nbytes + 32, dtype=np.uint8)
                want = canvas.copy()
                want[base:base + nbytes] = R.pack(fmt, prec, *planes, pitch, canvas[base:base + nbytes])
                d_canvas, d_planes = U.to_dev(canvas), U.to_dev(flat)
                c.packed_pack_device(fmt, prec, w, h, d_planes.data_ptr(), nplanes, d_canvas.data_ptr() + base, pitch, nbytes)
                c.synchronize()
                got = d_canvas.cpu().numpy()
                assert np.array_equal(got, want), ("pack", w, base, pitch, np.flatnonzero(got != want)[:8])
                launches += 1
    after = c.packed_counters()
    assert (after[0] - before[0], after[1] - before[1]) == (launches, launches)


def test_kernel_calls_check_their_sizes_on_the_host():
    c = U.ctx()
    w, h = 49, 17
    nbytes, nplanes = R.frame_bytes(R.V210, w, h), (w + 2 * 25) * h * 2
    d_frame, d_planes = U.to_dev(np.zeros(nbytes, np.uint8)), U.to_dev(np.full(nplanes, POISON, np.uint8))
    before = c.packed_counters()
    for args in ((nbytes - 1, nplanes), (nbytes, nplanes - 1)):
        with pytest.raises(G.SurfaceError) as e:
            c.packed_unpack_device(R.V210, 10, w, h, d_frame.data_ptr(), 0, args[0], d_planes.data_ptr(), args[1])
        assert e.value.code == OVERFLOW
        with pytest.raises(G.SurfaceError) as e:
            c.packed_pack_device(R.V210, 10, w, h, d_planes.data_ptr(), args[1], d_frame.data_ptr(), 0, args[0])
        assert e.value.code == OVERFLOW
    with pytest.raises(G.SurfaceError) as e:
        c.packed_unpack_device(R.V210, 12, w, h, d_frame.data_ptr(), 0, nbytes, d_planes.data_ptr(), nplanes)
    assert e.value.code == INVALID
    c.synchronize()
    assert c.packed_counters() == before and np.all(d_planes.cpu().numpy() == POISON)


# ---- 2. encode --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("fmt,prec", FORMATS, ids=IDS)
def test_encode_packed_equals_encode_image_subsampled(fmt, prec, shape):
    layout, base, planes, want, _ = case(shape, prec)
    c = U.ctx()
    pitch = pitch_of(fmt, shape)
    frame = noisy_frame(fmt, prec, planes, pitch, seed=fmt)
    assert G.packed_bytes(fmt, layout, prec, pitch)[0] == frame.size
    # (the frame 16 bytes into its buffer: the alignment every format takes)
    d_buf = U.to_dev(np.concatenate([np.zeros(16, np.uint8), frame]))
    before, kernels = c.surface_counters(), c.packed_counters()
    assert c.encode_packed(layout, base, fmt, frame, pitch, G.CS_PLT) == want, "host"
    assert c.encode_packed(layout, base, fmt, d_buf.data_ptr() + 16, pitch, G.CS_PLT, cap=frame.size) == want, "device"
    after = c.surface_counters()
    assert c.packed_counters() == (kernels[0] + 2, kernels[1])
    if shape == "one":
        # Y and the Cb / Cr run, twice: the tile coder read the context's planes where KU left them
        assert (after[0] - before[0], after[1] - before[1]) == (4, 0)
    else:
        assert after[0] == before[0] and after[1] > before[1]
    assert np.array_equal(d_buf.cpu().numpy()[16:], frame)                              # an encode only reads


def test_encode_packed_with_sop_eph_and_another_order():
    flags = G.CS_PLT | G.CS_SOP | G.CS_EPH | G.CS_PROG(2)
    layout, base, planes, want, _ = case("tiled", 8, flags)
    assert want != case("tiled", 8)[3]
    frame = noisy_frame(R.UYVY, 8, planes, 0, seed=3)
    assert U.ctx().encode_packed(layout, base, "UYVY", frame, 0, flags) == want


# ---- 3. decode --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("fmt,prec", FORMATS, ids=IDS)
def test_decode_packed_equals_decode_image(fmt, prec, shape):
    layout, base, planes, cs, back = case(shape, prec)
    c = U.ctx()
    w, h = SHAPES[shape][:2]
    pitch = pitch_of(fmt, shape)
    nbytes = R.frame_bytes(fmt, w, h, pitch)
    canvas = np.random.default_rng(50 + fmt).integers(0, 256, 16 + nbytes + 16, dtype=np.uint8)
    want = R.pack(fmt, prec, *back, pitch, canvas[16:16 + nbytes])
    assert not np.array_equal(want, canvas[16:16 + nbytes])
    kernels = c.packed_counters()
    host = canvas[16:16 + nbytes].copy()
    c.decode_packed(cs, fmt, host, pitch)
    assert np.array_equal(host, want), ("host", np.flatnonzero(host != want)[:8])
    dev = U.to_dev(canvas)
    c.decode_packed(cs, fmt, dev.data_ptr() + 16, pitch, cap=nbytes)                    # (cap: exactly the frame)
    c.decode_status()                                                                   # (raises unless the status is 0)
    got = dev.cpu().numpy()
    assert np.array_equal(got[16:16 + nbytes], want), ("device", np.flatnonzero(got[16:16 + nbytes] != want)[:8])
    assert np.array_equal(got[:16], canvas[:16]) and np.array_equal(got[16 + nbytes:], canvas[16 + nbytes:])
    assert c.packed_counters() == (kernels[0], kernels[1] + 2)
    if fmt == R.V210:
        # the bytes behind the last block of each row keep their values (pitch > a row's blocks in both shapes)
        p, row = pitch or R.default_pitch(fmt, w), R.row_bytes(fmt, w)
        assert p > row
        for y in range(h - 1):
            assert np.array_equal(got[16 + y * p + row:16 + (y + 1) * p], canvas[16 + y * p + row:16 + (y + 1) * p])


# ---- 4. rate ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,prec", [(R.YUY2, 8), (R.V210, 10)], ids=["YUY2-8", "V210-10"])
def test_encode_packed_rate_equals_encode_image_subsampled_rate(fmt, prec):
    layout, base, planes, plain, _ = case("tiled", prec)
    c = U.ctx()
    target = len(plain) * 6 // 10
    want, _ = c.encode_image_subsampled_rate(layout, base, S422, planes, target, G.CS_PLT)
    assert len(want) <= target
    frame = noisy_frame(fmt, prec, planes, 0, seed=9)
    got, res = c.encode_packed_rate(layout, base, fmt, frame, target, 0, G.CS_PLT)
    assert got == want and len(got) <= target and res.file_bytes == len(got)
    d_frame = U.to_dev(frame)
    got, _ = c.encode_packed_rate(layout, base, fmt, d_frame.data_ptr(), target, 0, G.CS_PLT, cap=frame.size)
    assert got == want


# ---- 5. refusals that need a context --------------------------------------------------------------------------------------------
def refused(call, code, text=None):
    with pytest.raises(G.SurfaceError) as e:
        call()
    assert e.value.code == code and (text is None or text in str(e.value)), str(e.value)


def test_refusals():
    layout, base, planes, cs, back = case("one", 10)
    c = U.ctx()
    w, h = SHAPES["one"][:2]
    frame = noisy_frame(R.V210, 10, planes, 0, seed=1)
    before = (c.packed_counters(), c.surface_counters())
    # an odd x0
    odd = G.ImageLayout.make(w, h, offset=(3, 0))
    refused(lambda: c.encode_packed(odd, base, "V210", frame), UNSUPPORTED, "odd x0")
    # the tile parameters
    refused(lambda: c.encode_packed(layout, G.TileParams.make(1, 1, 2, 10, LEVELS, mct=False), "V210", frame), INVALID, "three components")
    refused(lambda: c.encode_packed(layout, G.TileParams.make(1, 1, 3, 10, LEVELS, mct=True), "V210", frame), INVALID, "colour transform")
    refused(lambda: c.encode_packed(layout, G.TileParams.make(1, 1, 3, 12, LEVELS, mct=False), "V210", frame), INVALID, "precision")
    refused(lambda: c.encode_packed(layout, base, 7, frame), INVALID, "unknown format")
    refused(lambda: c.decode_packed(cs, 7, frame.copy()), INVALID, "unknown format")
    # pitch and base alignment
    refused(lambda: c.encode_packed(layout, base, "V210", frame, pitch=128), INVALID, "smaller than a row")
    refused(lambda: c.encode_packed(layout, base, "V210", frame, pitch=264), INVALID, "alignment")
    poison = np.full(frame.size + 32, POISON, np.uint8)
    dev = U.to_dev(poison)
    for off in (2, 8):
        refused(lambda: c.encode_packed(layout, base, "V210", dev.data_ptr() + off, cap=frame.size), INVALID, "device base")
        refused(lambda: c.decode_packed(cs, "V210", dev.data_ptr() + off, cap=frame.size), INVALID, "device base")
    refused(lambda: c.decode_packed(case("one", 10)[3], "Y216", dev.data_ptr() + 1, cap=poison.size - 1), INVALID, "device base")
    # cap one byte short: OVERFLOW, nothing written
    host = poison[:frame.size].copy()
    refused(lambda: c.decode_packed(cs, "V210", host, cap=frame.size - 1), OVERFLOW)
    refused(lambda: c.decode_packed(cs, "V210", dev.data_ptr(), cap=frame.size - 1), OVERFLOW)
    refused(lambda: c.encode_packed(layout, base, "V210", frame, cap=frame.size - 1), OVERFLOW)
    # a stream that is no 4:2:2 of the format's precision
    s420 = [(1, 1), (2, 2), (2, 2)]
    p420 = [planes[0], planes[1][:h // 2], planes[2][:h // 2]]
    cs420 = c.encode_image_subsampled(layout, base, s420, p420, G.CS_PLT)
    refused(lambda: c.decode_packed(cs420, "V210", host), UNSUPPORTED, "factors")
    refused(lambda: c.decode_packed(cs, "YUY2", host), UNSUPPORTED, "precision")
    refused(lambda: c.decode_packed(case("one", 8)[3], "V210", host), UNSUPPORTED, "precision")
    # what grk_amd_decode_surface refuses of the context is passed on
    c.set_decode_reduce(1)
    try:
        refused(lambda: c.decode_packed(cs, "V210", host), UNSUPPORTED, "grk_amd_decode_packed at reduced resolution")
    finally:
        c.set_decode_reduce(0)
    c.synchronize()
    assert np.all(host == POISON) and np.all(dev.cpu().numpy() == POISON)
    assert (c.packed_counters(), c.surface_counters()) == before


# ---- 6. round trip ----------------------------------------------------------------------------------------------------------------
def test_v210_round_trip_clears_the_ignored_bits():
    layout, base, planes, _, _ = case("tiled", 10)
    c = U.ctx()
    w, h = SHAPES["tiled"][:2]
    frame = noisy_frame(R.V210, 10, planes, 0, seed=77)
    cleared = R.pack(R.V210, 10, *R.unpack(R.V210, 10, frame, w, h), 0, np.zeros(frame.size, np.uint8))
    assert not np.array_equal(cleared, frame)                                           # (the noise, and the fields past the width)
    cs = c.encode_packed(layout, base, "V210", frame)
    out = np.zeros(frame.size, np.uint8)
    c.decode_packed(cs, "V210", out)
    assert np.array_equal(out, cleared)
    assert np.array_equal(out.view("<u4") >> 30, np.zeros(out.size // 4, np.uint32))
