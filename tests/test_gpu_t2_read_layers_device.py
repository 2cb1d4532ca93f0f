"""-m gpu: the GENERAL device Tier-2 reader (grk_amd_read_packets_device_ex; KL, KH, KC-L, KF, KP of kernels_t2read.hip) against the
host reader on the same bytes: rows, first_segment and segments field for field, the moves as sets (both sorted by dst),
appendix_bytes, and its code where it refuses.

The streams are tests/t2layers_cases.py's: layered files written from chosen tables (tests/t2layers_model.py, pinned on the host
reader by tests/test_t2_layers_model_cpu.py), the two LAZY / TERMALL goldens and, where the reference is built, its own layered files
as written and with PLT.  tests/test_t2_parse_layers_cpu.py has put every one of them through the kernels' parse core on the CPU
under AddressSanitizer."""
import numpy as np
import pytest
import torch

import grok_amd as G
import gpuutil as U
import refharness as R
import t2layers_cases as K
import t2read_cases as K1

pytestmark = pytest.mark.gpu
needs_ref = pytest.mark.skipif(not R.have_ref(), reason="oracle/_ref (the real reference) not built here")


def _dev(cs):
    return torch.from_numpy(np.frombuffer(cs, np.uint8).copy()).cuda()


def _equal_tables(c, cs, name=""):
    d = _dev(cs)
    want = G.read_packets(cs)
    info = c.read_header_device(d.data_ptr(), d.numel())
    assert bytes(info) == bytes(G.read_header(cs))
    got = c.read_packets_device_ex(d.data_ptr(), d.numel(), info)
    assert got["rows"].size == want["rows"].size, name
    for f in ("offset", "length", "missing_msbs"):
        assert np.array_equal(got["rows"][f], want["rows"][f]), (name, f)
    assert np.array_equal(got["first_segment"], want["first_segment"]), name
    assert np.array_equal(got["segments"], want["segments"]), name
    assert got["appendix_bytes"] == want["appendix_bytes"], name
    assert np.array_equal(np.sort(got["moves"], order="dst"), np.sort(want["moves"], order="dst")), name
    return want


def _refused(c, cs, code, name=""):
    d = _dev(cs)
    with pytest.raises(G.ReaderError) as e:
        c.read_packets_device_ex(d.data_ptr(), d.numel())
    assert e.value.code == code, (name, e.value.reason)
    assert "tile" in e.value.reason, e.value.reason


@pytest.fixture(scope="module")
def cases():
    return K.model_cases() + K.golden_cases()


def test_chosen_tables_and_goldens(cases):
    c = U.ctx()
    before = c.read_device_counters()
    appendices = 0
    for name, cs, code, _ in cases:
        if code is None:
            appendices += _equal_tables(c, cs, name)["appendix_bytes"] > 0
        else:
            with pytest.raises(G.ReaderError) as host:
                G.read_packets(cs)
            assert host.value.code == code, name
            _refused(c, cs, code, name)
    after = c.read_device_counters()
    # (a read through the binding is two calls: the sizes, then the tables)
    reads = sum(1 for _, _, code, _ in cases if code is None)
    assert after[5] - before[5] == 2 * reads + (len(cases) - reads) and after[2] == before[2]
    assert appendices > 20


def test_counter_5_rises_by_one_per_call(cases):
    c = U.ctx()
    cs = dict((n, b) for n, b, _, _ in cases)["both-kinds-of-block"]
    d = _dev(cs)
    info = c.read_header_device(d.data_ptr(), d.numel())
    L = G.lib()
    before = c.read_device_counters()[5]
    for k in range(3):
        assert L.grk_amd_read_packets_device_ex(c._h, d.data_ptr(), d.numel(), info, None, 0, None, None, 0, None, None, 0, None, None) == info.num_blocks
        assert c.read_device_counters()[5] == before + k + 1
    # a capacity too small
    rows = np.zeros(int(info.num_blocks), G.capi.CODED_DTYPE)
    assert L.grk_amd_read_packets_device_ex(c._h, d.data_ptr(), d.numel(), info, rows.ctypes.data, rows.size - 1, None, None, 0, None, None, 0, None,
                                            None) == G.capi.ERR_OVERFLOW
    # (moves == NULL where there are moves)
    assert L.grk_amd_read_packets_device_ex(c._h, d.data_ptr(), d.numel(), info, rows.ctypes.data, rows.size, None, None, 0, None, None, 0, None,
                                            None) == G.capi.ERR_OVERFLOW


def test_layered_then_a_smaller_single_layer_file_then_layered_again(cases):
    """stale nodes, row state, logs and status of the file before, on one context, through both readers"""
    c = U.ctx()
    files = dict((n, b) for n, b, _, _ in cases)
    layered = [n for n in files if n.startswith("drawn-o2-plt-sty05")][0]
    _equal_tables(c, files[layered], layered)
    small = K1.grid_file(260, 4)
    d = _dev(small)
    got = c.read_packets_device(d.data_ptr(), d.numel())
    want = G.read_packets(small)["rows"]
    for f in ("offset", "length", "missing_msbs"):
        assert np.array_equal(got[f], want[f]), f
    _equal_tables(c, small, "the single-layer file through the general reader")
    for name in ("lazy-layer-boundaries-fa", layered, "130-layers-first-inclusion-in-129-f2", "passes-with-length-0"):
        _equal_tables(c, files[name], name)
    _refused(c, files["passes-165-f2"], G.ERR_INVALID)
    _equal_tables(c, files[layered], layered)


def test_the_single_layer_reader_still_refuses_layers_and_segments(cases):
    c = U.ctx()
    files = dict((n, b) for n, b, _, _ in cases)
    names = [n for n in files if "_sty05_" in n or "_sty3f_" in n] + ["both-kinds-of-block", "termall-f2", "drawn-o0-chain-ht-f0-c3"]
    assert len(names) == 5
    for name in names:
        d = _dev(files[name])
        with pytest.raises(G.ReaderError) as e:
            c.read_packets_device(d.data_ptr(), d.numel())
        assert e.value.code == G.ERR_UNSUPPORTED, name


@needs_ref
def test_reference_written_layered_streams_as_written_and_with_plt(monkeypatch):
    c = U.ctx()
    n = 0
    for name, cs, _, _ in K.reference_cases(monkeypatch):
        want = _equal_tables(c, cs, name)
        n += len(want["moves"]) > 0
    assert n >= 10
