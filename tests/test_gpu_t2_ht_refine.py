"""-m gpu: grk_amd_read_packets_device_refine -- the device Tier-2 reader with the HT blocks' refinement passes read (KL-P, KH-P, KC-L,
KF, KP of kernels_t2read.hip over the plan of two segments and min(layers, 3) pieces per row) -- against the host reader with the
same option (grk_amd_read_packets_refine) on the same bytes: rows, first_segment and segments field for field, appendix_bytes, the
moves as sets, and its code where it refuses.

The files are tests/t2ht_cases.py's: every one the CPU tests read (tests/test_t2_ht_refine_cpu.py, which has put each through the
kernels' parse core on the CPU under AddressSanitizer first) -- tables of every contribution pattern, the wide tile, 2 x 2 tiles, the
tile divided by layer, the refused files -- and the files with real content that the pixel tests decode."""
import numpy as np
import pytest
import torch

import grok_amd as G
import gpuutil as U
import t2ht_cases as K

pytestmark = pytest.mark.gpu


def _dev(cs):
    return torch.from_numpy(np.frombuffer(cs, np.uint8).copy()).cuda()


def _equal_tables(c, cs, want, name):
    d = _dev(cs)
    torch.cuda.synchronize()
    info = c.read_header_device(d.data_ptr(), d.numel())
    assert bytes(info) == bytes(G.read_header(cs))
    got = c.read_packets_device_refine(d.data_ptr(), d.numel(), info)
    assert got["rows"].size == want["rows"].size, name
    for f in ("offset", "length", "missing_msbs"):
        assert np.array_equal(got["rows"][f], want["rows"][f]), (name, f)
    assert np.array_equal(got["first_segment"], want["first_segment"]), name
    assert np.array_equal(got["segments"], want["segments"]), name
    assert got["appendix_bytes"] == want["appendix_bytes"], name
    assert np.array_equal(np.sort(got["moves"], order="dst"), np.sort(want["moves"], order="dst")), name


@pytest.fixture(scope="module")
def cases():
    return K.table_cases()


def test_chosen_tables_read_as_the_host_refine_reader_reads_them(cases):
    c = U.ctx()
    read = appendices = 0
    for name, cs, code, _ in cases:
        if code is not None:
            continue
        want = G.read_packets_refine(cs)
        _equal_tables(c, cs, want, name)
        read += 1
        appendices += want["appendix_bytes"] > 0
    assert read >= 38 and appendices >= 20


def test_refused_files_get_the_host_readers_code(cases):
    c = U.ctx()
    seen = 0
    for name, cs, code, _ in cases:
        if code is None:
            continue
        with pytest.raises(G.ReaderError) as host:
            G.read_packets_refine(cs)
        assert host.value.code == code, name
        d = _dev(cs)
        torch.cuda.synchronize()
        with pytest.raises(G.ReaderError) as e:
            c.read_packets_device_refine(d.data_ptr(), d.numel())
        assert e.value.code == code, (name, e.value.reason)
        assert "tile" in e.value.reason and ("more than one pass" in e.value.reason) == (code == G.ERR_UNSUPPORTED), e.value.reason
        seen += 1
    assert seen == 6
    # ... and the reader is as good as new behind them
    name, cs, _, _ = cases[0]
    _equal_tables(c, cs, G.read_packets_refine(cs), name)


def test_real_content_files():
    c = U.ctx()
    for k in K.content_cases():
        _equal_tables(c, k.cs, G.read_packets_refine(k.cs), k.name)


def test_the_other_device_readers_keep_refusing(cases):
    c = U.ctx()
    cs, _ = K.three_pass_file()
    for f in (cs, cases[3][1]):
        d = _dev(f)
        torch.cuda.synchronize()
        for call in (c.read_packets_device, c.read_packets_device_ex, c.read_packets_device_parts):
            with pytest.raises(G.ReaderError) as e:
                call(d.data_ptr(), d.numel())
            assert e.value.code == G.ERR_UNSUPPORTED, e.value.reason
        pixels = torch.zeros(40 * 64 * 3, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        with pytest.raises(G.ReaderError) as e:
            c.decode_image_resident(d.data_ptr(), d.numel(), pixels.data_ptr(), pixels.numel())
        assert e.value.code == G.ERR_UNSUPPORTED, e.value.reason
    # a cleanup-only file: the refine reader's tables are the other readers'
    k = K.content_file(K.SHAPES[4], False, K.PLT, refine=False)
    d = _dev(k.cs)
    torch.cuda.synchronize()
    a, b = c.read_packets_device_parts(d.data_ptr(), d.numel()), c.read_packets_device_refine(d.data_ptr(), d.numel())
    for f in ("rows", "first_segment", "segments", "moves"):
        assert np.array_equal(a[f], b[f]), f
