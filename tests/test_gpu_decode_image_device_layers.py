"""-m gpu: grk_amd_decode_image_device_ex -- a layered or multi-segment codestream that lies in device memory decoded where it lies --
against grk_amd_decode_image of the same bytes on the host, pixel for pixel: the two LAZY / TERMALL goldens (no appendix: nothing
is copied), the reference's three-layer Part-1 and HT streams of nine tiles into host and into device pixels (Part-1: the stream is
staged in front of its appendix, once), a layered 4:2:0 stream with up-sampling, and the appendix the call gathers from moves that
never left the device against the reader's moves applied with numpy."""
import os

import numpy as np
import pytest
import torch

import grok_amd as G
import gpuutil as U
import refharness as R
import t2layers_cases as K

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
needs_ref = pytest.mark.skipif(not R.have_ref(), reason="oracle/_ref (the real reference) not built here")


def _dev(cs, pad=0):
    """the stream in device memory; pad: bytes of 0xFF behind it (the call assumes nothing about them and leaves them alone)"""
    return torch.from_numpy(np.concatenate([np.frombuffer(cs, np.uint8), np.full(pad, 0xFF, np.uint8)])).cuda()


def _to_host(c, cs, like):
    d = _dev(cs, 64)
    out = np.zeros(like.nbytes, np.uint8)
    c.decode_image_resident_ex(d.data_ptr(), len(cs), out.ctypes.data, out.nbytes, on_device=False)
    back = d.cpu().numpy()
    assert back[:len(cs)].tobytes() == cs and np.all(back[len(cs):] == 0xFF), "the caller's buffer was written"
    return out.view(like.dtype).reshape(like.shape)


def test_lazy_and_termall_goldens_without_a_copy():
    c = U.ctx()
    for name, cs, _, _ in K.golden_cases():
        want = c.decode_image(cs)
        before = c.read_device_counters()
        got = _to_host(c, cs, want)
        assert np.array_equal(got, want), name
        after = c.read_device_counters()
        assert after[4] == before[4] and after[5] == before[5] + 1, name
        d = _dev(cs)
        with pytest.raises(G.ReaderError) as e:
            c.decode_image_resident(d.data_ptr(), d.numel(), got.ctypes.data, got.nbytes, on_device=False)
        assert e.value.code == G.ERR_UNSUPPORTED


@needs_ref
@pytest.mark.parametrize("ht", [0, 1], ids=["part1", "ht"])
def test_three_layers_nine_tiles_to_host_and_to_device_pixels(monkeypatch, ht):
    c = U.ctx()
    cs = K.reference_stream(monkeypatch, ht, 0)
    info = G.read_header(cs)
    assert info.num_layers == 3 and info.num_tiles == 9
    host = G.read_packets(cs)
    want = c.decode_image(cs)
    before = c.read_device_counters()
    got = _to_host(c, cs, want)
    assert np.array_equal(got, want)
    after = c.read_device_counters()
    if not ht:
        assert host["appendix_bytes"] > 0
    assert after[4] - before[4] == (len(cs) if host["appendix_bytes"] else 0)
    # device pixels: asynchronous, decode_status joins
    d = _dev(cs)
    out = U._settled(torch.zeros(want.nbytes, dtype=torch.uint8, device="cuda"))
    c.decode_image_resident_ex(d.data_ptr(), d.numel(), out.data_ptr(), want.nbytes)
    c.decode_status()
    assert np.array_equal(out.cpu().numpy().view(want.dtype).reshape(want.shape), want)
    # with PLT: the chains are the precincts
    with_plt = K.plt_from_sop(cs)
    assert np.array_equal(_to_host(c, with_plt, want), want)


@needs_ref
def test_layered_420_with_upsampling(monkeypatch):
    from test_t2_reader_subsampled_cpu import S420, make_planes, ref_subsampled_stream
    c = U.ctx()
    layout = G.ImageLayout.make(256, 192, 128, 96)
    planes = make_planes(layout, S420, 8, seed=3)
    cs = ref_subsampled_stream(monkeypatch, planes, S420, 8, 256, 192, {"REF_LAYERS": "20,1"}, 128, 96, numres=4, ht=0)
    assert G.read_header(cs).num_layers == 2 and G.read_packets(cs)["appendix_bytes"] > 0
    c.set_decode_upsample(True)
    try:
        want = c.decode_image(cs)
        assert np.array_equal(_to_host(c, cs, want), want)
    finally:
        c.set_decode_upsample(False)


@needs_ref
def test_gathered_appendix_is_the_readers_moves_applied(monkeypatch):
    """behind a decode the context's coded buffer holds [stream | appendix]"""
    c = G.Context(0)
    cs = K.reference_stream(monkeypatch, 0, 2)
    out = G.read_packets(cs)
    assert len(out["moves"]) > 0
    b = np.frombuffer(cs, np.uint8)
    want = np.zeros(out["appendix_bytes"], np.uint8)
    for m in out["moves"]:
        want[int(m["dst"]):int(m["dst"]) + int(m["len"])] = b[int(m["src"]):int(m["src"]) + int(m["len"])]
    px = c.decode_image(cs)
    gathers, _ = c.decode_image_launches()
    got = _to_host(c, cs, px)
    assert np.array_equal(got, px)
    assert c.decode_image_launches()[0] == gathers + 1
    d = _dev(cs)
    moves = c.read_packets_device_ex(d.data_ptr(), d.numel())["moves"]
    assert np.array_equal(moves, np.sort(out["moves"], order="dst"))
    # the moves the placement kernel wrote, through the gather kernel
    d_dst = U.to_dev(np.zeros(want.size, np.uint8))
    c.gather_device(moves, d.data_ptr(), b.size, d_dst.data_ptr(), want.size)
    c.synchronize()
    assert np.array_equal(d_dst.cpu().numpy(), want)
    c.close()
