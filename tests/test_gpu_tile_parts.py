"""GPU: codestreams whose tiles are divided into tile-parts through the device reader (grk_amd_read_packets_device_parts: KL-P, KH-P
and KC-L over the part table, field for field what grk_amd_read_packets_parts gives) and through the decode calls that read a file by
themselves -- grk_amd_decode_image, grk_amd_decode_image_view, grk_amd_decode_image_device_ex.  The files are cut by tests/tileparts.py (tests/test_tile_parts_cpu.py holds that
model against the reader's table and, where the reference is built, against the reference's decoder); here the pixels of a cut file
must be the undivided file's, bit for bit.  With TNsot = 0 in every tile-part the reference's own decoder stops early without an
error, so every cut -- that one included -- is held to this library's decode of the undivided file; the undivided files themselves are
held to the reference in tests/test_gpu_decode_image.py."""
import numpy as np
import pytest
import torch

import grok_amd as G
import gpuutil as U
import refharness as R
import synth
import tileparts as TP
import tileparts_cases as TC
import test_tile_parts_cpu as CPU
from test_t2_reader_subsampled_cpu import S420, make_planes
from test_tile_parts_cpu import REF_KINDS, ref_file

pytestmark = pytest.mark.gpu
needs_ref = pytest.mark.skipif(not R.have_ref(), reason="oracle/_ref (the real reference) not built here")
W, H, TW, TH = 96, 80, 64, 64                # four tiles, the right and the lower ones cut by the image


def own_file(irrev, flags=G.CS_PLT):
    px = synth.g2_mid(3, H, W, 8)
    layout = G.ImageLayout.make(W, H, TW, TH)
    base = G.TileParams.make(TW, TH, 3, 8, 2, irreversible=irrev)
    return px, U.ctx().encode_image(layout, base, px, flags)


def cuts_of(cs):
    """the nine cuts; a file without PLT (its packets found through SOP) gets PLT in two of them"""
    have = bool(G.read_header(cs).flags & G.CS_PLT)
    for name, kw in TP.NINE_CUTS:
        kw = dict(kw)
        if not have and "plt" not in kw:
            kw["plt"] = "keep" if name in ("thirds", "interleaved") else "drop"
        yield name, TP.cut(cs, **kw)


@pytest.mark.parametrize("irrev", [False, True], ids=["53", "97"])
def test_decode_image_of_cut_ht_files_is_the_undivided_files_image(irrev):
    px, cs = own_file(irrev)
    c = U.ctx()
    want = c.decode_image(cs)
    if not irrev:
        assert np.array_equal(want, px)
    for name, cut in cuts_of(cs):
        assert len(cut.parts) > 4
        assert np.array_equal(c.decode_image(cut.cs), want), name
    # SOP / EPH in the packets, PLT dropped, the tiles out of order, Psot 0 in the last tile-part
    px, cs = own_file(irrev, G.CS_SOP | G.CS_EPH | G.CS_PROG(2))
    cut = TP.cut(cs, boundaries=TP.thirds, plt="drop", tile_order=(3, 1, 0, 2), order="interleave", tnsot="last", last_psot_zero=True)
    assert np.array_equal(c.decode_image(cut.cs), want)


@needs_ref
@pytest.mark.parametrize("kind", REF_KINDS)
def test_decode_image_of_cut_reference_files(monkeypatch, kind):
    """HT and Part-1, one and three layers, as the reference writes them"""
    px, cs = ref_file(monkeypatch, kind)
    c = U.ctx()
    want = c.decode_image(cs)
    assert np.array_equal(want.astype(np.int32), R.decode(cs, 3, H, W))
    layered = G.read_header(cs).num_layers > 1
    for name, cut in cuts_of(cs):
        gathers, _ = c.decode_image_launches()
        assert np.array_equal(c.decode_image(cut.cs), want), (kind, name)
        if layered and kind.startswith("p1"):
            assert c.decode_image_launches()[0] > gathers, "a layered Part-1 file's blocks come in pieces: gathered"


@needs_ref
def test_decode_image_of_a_cut_irreversible_part1_file(monkeypatch):
    for k in ("REF_PROG_ORDER", "REF_PRECINCTS", "REF_CSTY", "REF_WRITE_PLT", "REF_WRITE_TLM", "REF_LAYERS", "REF_IMG_X0", "REF_IMG_Y0"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("REF_WRITE_PLT", "1")
    cs = R.encode(synth.g2_mid(3, H, W, 8), 8, mode=1, TW=TW, TH=TH, numres=3, ht=0, irrev=1)[0]
    c = U.ctx()
    want = c.decode_image(cs)
    for name, cut in cuts_of(cs):
        assert np.array_equal(c.decode_image(cut.cs), want), name


def test_subsampled_planes_and_the_upsampled_image_of_a_cut_file():
    layout = G.ImageLayout.make(130, 99, 64, 48, offset=(3, 1))
    planes = make_planes(layout, S420, 8, seed=7)
    base = G.TileParams.make(1, 1, 3, 8, 3, mct=False)
    c = U.ctx()
    cs = c.encode_image_subsampled(layout, base, S420, planes, G.CS_PLT | G.CS_PROG(2))
    cut = TP.cut(cs, boundaries=TP.thirds, order="interleave", tlm="write", tnsot="none")
    assert len(cut.parts) == 3 * G.read_header(cs).num_tiles
    for a, b in zip(c.decode_image_planes(cut.cs), planes):
        assert a.shape == b.shape and np.array_equal(a, b)
    c.set_decode_upsample(True)
    try:
        assert np.array_equal(c.decode_image(cut.cs), c.decode_image(cs))
    finally:
        c.set_decode_upsample(False)


@pytest.mark.parametrize("view", [dict(window=(66, 3, 90, 40)), dict(reduce=1), dict(reduce=1, window=(2, 33, 30, 39))], ids=["window", "reduce-1", "both"])
def test_views_of_an_interleaved_tlm_file_upload_only_the_touched_tiles_parts(view):
    px, cs = own_file(False)
    cut = TP.cut(cs, boundaries=TP.thirds, order="interleave", tlm="write")
    c = U.ctx()
    want = c.decode_image_view(cs, **view)
    tiles0, up0 = c.decode_image_counters()
    got = c.decode_image_view(cut.cs, **view)
    tiles1, up1 = c.decode_image_counters()
    assert np.array_equal(got, want)
    if "window" in view:
        # the window lies inside one tile: tile 1 (the full-size window), tile 2 (the window of the half-size image)
        tile = 1 if "reduce" not in view else 2
        assert tiles1 - tiles0 == 1
        assert up1 - up0 == sum(p.length for p in cut.parts_of(tile)) <= sum(p.length for p in cut.parts_of(tile)) + cut.parts[0].at
    else:
        assert tiles1 - tiles0 == 4 and up1 - up0 == len(cut.cs)


def test_the_single_layer_device_decode_still_refuses_a_cut_file():
    px, cs = own_file(False)
    cut = TP.cut(cs, boundaries=TP.thirds)
    c = U.ctx()
    d_cs = U._settled(torch.from_numpy(np.frombuffer(cut.cs, np.uint8).copy()).cuda())
    out = U._settled(torch.zeros(px.nbytes, dtype=torch.uint8, device="cuda"))
    with pytest.raises(G.ReaderError) as e:
        c.decode_image_resident(d_cs.data_ptr(), d_cs.numel(), out.data_ptr(), px.nbytes)
    assert e.value.code == G.ERR_UNSUPPORTED
    # and the context reads a good file right after
    assert np.array_equal(c.decode_image(cut.cs), px)


# ---- the device reader -------------------------------------------------------------------------------------------------------------
def _dev(cs):
    return U._settled(torch.from_numpy(np.frombuffer(cs, np.uint8).copy()).cuda())


@pytest.fixture(scope="module")
def cases():
    return TC.cases()


@pytest.fixture(scope="module")
def refusals():
    return TC.refusals()


def _equal_tables(c, cs, name):
    d = _dev(cs)
    want = G.read_packets_parts(cs)
    info = c.read_header_device(d.data_ptr(), d.numel())
    assert bytes(info) == bytes(G.read_header(cs))
    got = c.read_packets_device_parts(d.data_ptr(), d.numel(), info)
    assert got["rows"].size == want["rows"].size, name
    for f in ("offset", "length", "missing_msbs"):
        assert np.array_equal(got["rows"][f], want["rows"][f]), (name, f)
    assert np.array_equal(got["first_segment"], want["first_segment"]), name
    assert np.array_equal(got["segments"], want["segments"]), name
    assert got["appendix_bytes"] == want["appendix_bytes"], name
    assert np.array_equal(np.sort(got["moves"], order="dst"), np.sort(want["moves"], order="dst")), name


def test_the_streams_are_the_ones_the_sanitized_cpu_program_ran(cases, refusals):
    assert [c[0] for c in cases] + [r[0] for r in refusals] == CPU.case_names()


def test_device_reader_equals_the_host_reader_on_every_cut_file(cases):
    c = U.ctx()
    launches = c.read_device_parts_launches()
    for name, base, cut in cases:
        _equal_tables(c, cut.cs, name)
    # (two calls per file -- the sizes, then the tables --, KL-P and KH-P's two steps in each)
    assert c.read_device_parts_launches() == launches + 6 * len(cases)
    # an undivided file reads the same through the new call
    for name, base, cut in cases[::11]:
        _equal_tables(c, base, name)


def test_device_reader_refuses_with_the_host_readers_code_and_reads_on(cases, refusals):
    c = U.ctx()
    good = cases[0][2].cs
    for name, cs, code, _ in refusals:
        d = _dev(cs)
        with pytest.raises(G.ReaderError) as e:
            c.read_packets_device_parts(d.data_ptr(), d.numel())
        assert e.value.code == code, (name, e.value.reason)
        assert "tile" in e.value.reason, (name, e.value.reason)
        _equal_tables(c, good, name)


def test_the_older_device_calls_still_refuse_a_cut_file(cases):
    c = U.ctx()
    d = _dev(cases[0][2].cs)
    for call in (c.read_packets_device, c.read_packets_device_ex):
        with pytest.raises(G.ReaderError) as e:
            call(d.data_ptr(), d.numel())
        assert e.value.code == G.ERR_UNSUPPORTED and "tile-part" in e.value.reason


def _resident_ex(c, cs, shape, dtype):
    d = _dev(cs)
    out = U._settled(torch.zeros(int(np.prod(shape)) * np.dtype(dtype).itemsize, dtype=torch.uint8, device="cuda"))
    c.decode_image_resident_ex(d.data_ptr(), d.numel(), out.data_ptr(), out.numel())
    c.decode_status()
    return out.cpu().numpy().view(dtype).reshape(shape)


def test_device_decode_of_a_cut_single_layer_file_in_place():
    px, cs = own_file(False)
    c = U.ctx()
    for name, cut in cuts_of(cs):
        before, launches = c.read_device_counters(), c.read_device_parts_launches()
        assert np.array_equal(_resident_ex(c, cut.cs, px.shape, px.dtype), px), name
        after = c.read_device_counters()
        assert after[4] == before[4], "no appendix: the stream is the coded buffer where it lies"
        assert c.read_device_parts_launches() == launches + 3
    # an undivided file takes the route it always took: no launch of KL-P / KH-P
    launches = c.read_device_parts_launches()
    assert np.array_equal(_resident_ex(c, cs, px.shape, px.dtype), px)
    assert c.read_device_parts_launches() == launches


@needs_ref
def test_device_decode_of_a_cut_three_layer_file_staged(monkeypatch):
    px, cs = ref_file(monkeypatch, "p1-layers-rpcl")
    c = U.ctx()
    want = c.decode_image(cs)
    for name, cut in cuts_of(cs):
        before = c.read_device_counters()
        assert np.array_equal(_resident_ex(c, cut.cs, want.shape, want.dtype), want), name
        assert c.read_device_counters()[4] == before[4] + len(cut.cs), "an appendix: the stream staged in front of it"
