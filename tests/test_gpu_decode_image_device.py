"""-m gpu: grk_amd_decode_image_device -- a codestream that lies in device memory decoded where it lies -- against grk_amd_decode_image
of the same bytes on the host (and, for lossless files, the source pixels): an encode's device-resident file straight back through
the decoder on the same context, edge tiles with 9/7, 4:2:0 with and without up-sampling, a Part-1 file of the reference's, an
interleaved pitched destination, what the call may copy either way (counters), and the refusals on the context."""
import os

import numpy as np
import pytest
import torch

import grok_amd as G
import gpuutil as U
import synth

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _dev(cs):
    return torch.from_numpy(np.frombuffer(cs, np.uint8).copy()).cuda()


def _resident_to_host(c, cs, nbytes):
    """the stream uploaded by the TEST (it then is a device-resident file), decoded into host pixels -> uint8 buffer"""
    d = _dev(cs)
    out = np.zeros(nbytes, np.uint8)
    c.decode_image_resident(d.data_ptr(), d.numel(), out.ctypes.data, out.nbytes, on_device=False)
    return out


def _planes(layout, sampling, seed):
    rng = np.random.default_rng(seed)
    out = []
    for dx, dy in sampling:
        w = -(-layout.x1 // dx) - -(-layout.x0 // dx)
        h = -(-layout.y1 // dy) - -(-layout.y0 // dy)
        out.append((rng.integers(0, 40, (h, w)) + np.arange(w)[None, :] % 200).astype(np.uint8))
    return out


@pytest.mark.parametrize("flags", [0, G.CS_PLT | G.CS_TLM], ids=["plain", "plt-tlm"])
def test_loop_back_of_a_device_resident_file(flags):
    """96 x 80 x 3 through a _device encoder; its file never leaves the device"""
    c = U.ctx()
    layout = G.ImageLayout.make(96, 80)
    surface, sampling, nbytes = G.Surface.make("I444", layout, None, 0)
    base = G.TileParams.make(1, 1, 3, 8, 3, mct=False)
    planes = _planes(layout, sampling, 11)
    buf = np.zeros(nbytes, np.uint8)
    surface.scatter(buf, planes, 1)
    d_buf = torch.from_numpy(buf).cuda()
    ptr, n = c.encode_surface_device(layout, base, sampling, surface, d_buf.data_ptr(), flags, cap=nbytes)
    total = sum(p.size for p in planes)
    d_px = torch.zeros(total, dtype=torch.uint8, device="cuda")
    before = c.read_device_counters()
    c.decode_image_resident(ptr, n, d_px.data_ptr(), total)
    c.decode_status()
    got = d_px.cpu().numpy()
    at = 0
    for p in planes:
        assert np.array_equal(got[at:at + p.size].reshape(p.shape), p)
        at += p.size
    cs = U.from_dev_ptr(ptr, n).tobytes()
    assert bool(G.read_header(cs).flags & G.CS_PLT) == bool(flags & G.CS_PLT)
    host = c.decode_image_planes(cs)
    assert all(np.array_equal(a, b) for a, b in zip(host, planes))
    # what the call copied: device -> host the main header (its first copy at most 4096 bytes), the status word and 16 bytes per
    # row; host -> device the reader's descriptors, nothing that grows with the file
    after = c.read_device_counters()
    info = G.read_header(cs)
    parts, _ = G.locate_tile_parts(cs)
    tp_headers = sum(cs.index(b"\xff\x93", o) + 2 - o for o, _, _ in parts)
    assert after[0] - before[0] <= cs.index(b"\xff\x90") + 16 * info.num_blocks + tp_headers + 4096
    assert after[1] - before[1] <= 4096 and after[2] - before[2] == 1


def test_edge_tiles_irreversible_and_counters():
    c = U.ctx()
    px = synth.g2(3, 76, 100, 8)
    layout = G.ImageLayout.make(100, 76, 64, 48)
    base = G.TileParams.make(64, 48, 3, 8, 3, irreversible=True)
    cs = c.encode_image(layout, base, px, G.CS_PLT)
    want = c.decode_image(cs)
    before = c.read_device_counters()
    up = c.decode_image_counters()
    got = _resident_to_host(c, cs, want.nbytes).view(want.dtype).reshape(want.shape)
    assert np.array_equal(got, want)
    after = c.read_device_counters()
    info = G.read_header(cs)
    parts, _ = G.locate_tile_parts(cs)
    tp_headers = sum(cs.index(b"\xff\x93", o) + 2 - o for o, _, _ in parts)
    assert after[0] - before[0] <= cs.index(b"\xff\x90") + 16 * info.num_blocks + tp_headers + 4096
    assert after[1] - before[1] <= 8192            # (four tile classes' descriptors: no term in the file's length)
    assert c.decode_image_counters() == up         # nothing of the file was uploaded by the decoder


@pytest.mark.parametrize("tile", [None, (48, 32)], ids=["one-tile", "2x2-tiles"])
@pytest.mark.parametrize("upsample", [False, True], ids=["planes", "upsampled"])
def test_subsampled(tile, upsample):
    c = U.ctx()
    layout = G.ImageLayout.make(90, 60, *(tile or (None, None)))
    sampling = [(1, 1), (2, 2), (2, 2)]
    base = G.TileParams.make(1, 1, 3, 8, 2, mct=False)
    planes = _planes(layout, sampling, 5)
    cs = c.encode_image_subsampled(layout, base, sampling, planes, G.CS_PLT if tile else 0)
    c.set_decode_upsample(upsample)
    try:
        if upsample:
            want = c.decode_image(cs)
            got = _resident_to_host(c, cs, want.nbytes).view(want.dtype).reshape(want.shape)
            assert np.array_equal(got, want)
        else:
            want = c.decode_image_planes(cs)
            got = _resident_to_host(c, cs, sum(p.size for p in want))
            at = 0
            for p, src in zip(want, planes):
                assert np.array_equal(got[at:at + p.size].reshape(p.shape), p) and np.array_equal(p, src)
                at += p.size
    finally:
        c.set_decode_upsample(False)


def test_part1_file_of_the_reference():
    c = U.ctx()
    cs = open(os.path.join(HERE, "golden", "dec_p1_rev_3x100x77_r3.j2k"), "rb").read()
    want = c.decode_image(cs)
    got = _resident_to_host(c, cs, want.nbytes).view(want.dtype).reshape(want.shape)
    assert np.array_equal(got, want)


def test_interleaved_pitched_destination():
    c = U.ctx()
    px = synth.g2(3, 50, 70, 8)
    layout = G.ImageLayout.make(70, 50, 32, 32)
    cs = c.encode_image(layout, G.TileParams.make(32, 32, 3, 8, 2), px, 0)
    lay = G.PixelLayout.make(interleaved=True, channels=4, row_pitch=70 * 4 + 24, fill=0x5A)
    want = c.decode_image(cs, lay, np.full(50 * (70 * 4 + 24), 0xA5, np.uint8))
    d = _dev(cs)
    got = np.full(want.size, 0xA5, np.uint8)
    c._with_decode_layout(lay, lambda: c.decode_image_resident(d.data_ptr(), d.numel(), got.ctypes.data, got.nbytes, on_device=False))
    assert np.array_equal(got, want)


def test_context_refusals_hold():
    c = G.Context(0)
    px = synth.g2(1, 32, 32, 8)
    cs = c.encode_image(G.ImageLayout.make(32, 32), G.TileParams.make(32, 32, 1, 8, 2), px, 0)
    d = _dev(cs)
    out = np.zeros(32 * 32, np.uint8)
    c.set_decode_reduce(1)
    with pytest.raises(G.ReaderError) as e:
        c.decode_image_resident(d.data_ptr(), d.numel(), out.ctypes.data, out.nbytes, on_device=False)
    assert e.value.code == G.ERR_UNSUPPORTED
    c.set_decode_reduce(0)
    c.set_decode_pipelining(2)
    with pytest.raises(G.ReaderError) as e:
        c.decode_image_resident(d.data_ptr(), d.numel(), out.ctypes.data, out.nbytes, on_device=False)
    assert e.value.code == G.ERR_UNSUPPORTED
    c.set_decode_pipelining(0)
    c.decode_image_resident(d.data_ptr(), d.numel(), out.ctypes.data, out.nbytes, on_device=False)
    assert np.array_equal(out.reshape(1, 32, 32), px)
    c.close()
