"""-m gpu: the device Tier-2 reader (grk_amd_read_header_device / grk_amd_read_packets_device; KL, KH, KC of kernels_t2read.hip) against
the host reader on the same bytes: the rows field for field where it accepts, its code where it refuses.

The streams are tests/t2read_cases.py's: the reference-written files under tests/golden, files the host writer makes from chosen
tables on a tile of 4 x 4 blocks (deep trees), tile-parts out of index order, 4:2:0, a main header longer than the call's first copy,
band grids of 65 x 1 and 1 x 65 blocks, and twelve named corruptions.  tests/test_t2_parse_cpu.py has put every one of them through
the kernels' parse core on the CPU under AddressSanitizer; the cases about stuffing assert their property there, while the file is
built, before any launch."""
import numpy as np
import pytest
import torch

import grok_amd as G
import gpuutil as U
import t2read_cases as K

pytestmark = pytest.mark.gpu


def _dev(cs):
    return torch.from_numpy(np.frombuffer(cs, np.uint8).copy()).cuda()


def _equal_rows(c, cs):
    d = _dev(cs)
    want = G.read_packets(cs)["rows"]
    info = c.read_header_device(d.data_ptr(), d.numel())
    assert bytes(info) == bytes(G.read_header(cs))
    got = c.read_packets_device(d.data_ptr(), d.numel(), info)
    assert got.size == want.size
    for f in ("offset", "length", "missing_msbs"):
        assert np.array_equal(got[f], want[f]), f
    return d


@pytest.fixture(scope="module")
def reading():
    return K.reading_cases()


def test_golden_files_have_no_plt_or_tlm_and_read_alike():
    c = U.ctx()
    n = 0
    for name, cs, code in K.golden_cases():
        flags = G.read_header(cs).flags
        assert not flags & (G.CS_PLT | G.CS_TLM), name
        if code is None:
            _equal_rows(c, cs)
            n += 1
        else:
            d = _dev(cs)
            with pytest.raises(G.ReaderError) as e:
                c.read_packets_device(d.data_ptr(), d.numel())
            assert e.value.code == G.ERR_UNSUPPORTED, name
    assert n == 10 and G.read_header(dict((a, b) for a, b, _ in K.golden_cases())["g2_3x256x256_t128_r4.j2k"]).num_tiles == 4


def test_chosen_tables(reading):
    c = U.ctx()
    before = c.read_device_counters()
    for name, cs, _ in reading:
        try:
            _equal_rows(c, cs)
        except AssertionError as e:
            raise AssertionError("%s: %s" % (name, e))
    after = c.read_device_counters()
    assert after[2] - before[2] == len(reading) and after[3] > before[3]


def test_long_main_header_takes_a_second_copy(reading):
    c = U.ctx()
    cs = dict((a, b) for a, b, _ in reading)["long-main-header"]
    assert cs.index(b"\xff\x90") > G.capi.READ_DEVICE_FIRST_COPY
    d = _dev(cs)
    before = c.read_device_counters()[0]
    info = c.read_header_device(d.data_ptr(), d.numel())
    assert bytes(info) == bytes(G.read_header(cs))
    assert G.capi.READ_DEVICE_FIRST_COPY < c.read_device_counters()[0] - before <= len(cs)


def test_second_file_with_fewer_blocks_on_one_context(reading):
    """stale tree nodes, rows and status of the file before"""
    c = U.ctx()
    files = dict((a, b) for a, b, _ in reading)
    for name in ("block-msbs-chain", "grid-65x1", "420-two-tiles", "all-zero-lengths", "flags-15"):
        _equal_rows(c, files[name])


def test_twelve_corruptions_are_refused_with_the_host_readers_code():
    c = U.ctx()
    good = K.good_file()
    cases = K.corruption_cases()
    assert len(cases) == 12
    for name, cs, code in cases:
        with pytest.raises(G.ReaderError) as host:
            G.read_packets(cs)
        assert host.value.code == code, name
        d = _dev(cs)
        with pytest.raises(G.ReaderError) as e:
            c.read_packets_device(d.data_ptr(), d.numel())
        assert e.value.code == code, (name, e.value.reason)
        assert "tile" in e.value.reason, e.value.reason
        _equal_rows(c, good)            # ... and a good file reads on the same context afterwards
