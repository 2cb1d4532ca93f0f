"""CPU: tests/t2model.py -- the Python restatement of a packet header that tests/test_gpu_t2_tables.py steers its tables with -- pinned on
the host writer: for a few small geometries and random tables the model's stuffed bytes are the header bytes inside
grk_amd_write_tile_part's output, packet by packet.  The model's meters (entry offsets at chunk, super-chunk and window boundaries,
0xFF steps across a window boundary) are worth what this comparison is worth; two of them are checked on headers made by hand."""
import numpy as np
import pytest

import grok_amd as G
import t2model as M


def random_table(rng, nrows, lo, hi, coded_bytes):
    """lengths lo .. hi, half of them of the form 2^k - 1 (runs of ones in the header: 0xFF bytes), offsets anywhere in the coded bytes"""
    t = np.zeros(nrows, G.capi.CODED_DTYPE)
    ln = rng.integers(lo, hi + 1, nrows)
    ones = (1 << rng.integers(max(int(lo).bit_length(), 1), int(hi).bit_length() + 1, nrows)) - 1
    pick = rng.random(nrows) < 0.5
    ln[pick] = np.clip(ones[pick], lo, hi)
    t["length"] = ln
    t["offset"] = rng.integers(0, coded_bytes - hi, nrows)
    return t


@pytest.mark.parametrize("make,lo,hi", [
    (dict(w=128, h=168, comps=1, prec=8, levels=1, cblk=(2, 2)), 64, 2047),
    (dict(w=40, h=64, comps=1, prec=8, levels=1, cblk=(2, 2)), 0, 300),
    (dict(w=2048, h=8, comps=1, prec=8, levels=1, cblk=(2, 2)), 0, 70000),
    (dict(w=200, h=136, comps=3, prec=12, levels=3, cblk=(3, 4)), 0, 4095),
    (dict(w=64, h=64, comps=1, prec=8, levels=0), 7, 7),
])
def test_model_headers_are_the_host_writers(make, lo, hi):
    p = G.TileParams.make(make.pop("w"), make.pop("h"), make.pop("comps"), make.pop("prec"), make.pop("levels"), **make)
    packets = M.packets_of(p)
    nrows = sum(k["rows"].size for k in packets)
    rng = np.random.default_rng(nrows + hi)
    coded = rng.integers(0, 256, hi + 4096, dtype=np.uint8)
    for rep in range(3):
        table = random_table(rng, nrows, lo, hi, coded.size)
        part = G.write_tile_part(p, 3, table, coded, 0)
        assert G.write_tile_part(p, 3, table, None, 0, size_only=True) == len(part)
        at = 14                                        # SOT 12, SOD 2
        for k in packets:
            lengths = table["length"][k["rows"]]
            data, _ = M.header(k["bands"], lengths, 512 * 32)
            assert part[at:at + len(data)] == data, "packet at byte %d" % at
            at += len(data)
            for r in k["rows"]:
                o, n = int(table["offset"][r]), int(table["length"][r])
                assert part[at:at + n] == coded[o:o + n].tobytes()
                at += n
        assert at == len(part)


def test_meters_on_headers_made_by_hand():
    # no 0xFF anywhere: every step takes eight bits, every boundary is entered at offset 0
    bits = np.zeros(3 * 16384, np.uint8)
    data, starts, ff = M.walk(bits)
    m = M.meters(bits.size, starts, ff, 16384)
    assert data == bytes(bits.size // 8) and m == dict(chunk={0}, super={0}, window={0}, straddle=0)
    # one 0xFF at bits 16376 .. 16383, flush with the first window: its step ends at 16391 -- the next window is entered at offset 7,
    # across the boundary
    bits[16376:16384] = 1
    data, starts, ff = M.walk(bits)
    m = M.meters(bits.size, starts, ff, 16384)
    assert m["window"] == {7} and m["straddle"] == 1 and m["super"] == {0, 7} and 7 in m["chunk"]
    assert data[2047] == 0xFF and data[2048] == 0 and len(data) == 3 * 2048 + 1
    # ... and one a byte earlier: its step ends at 16383, and it is a plain byte that crosses the boundary -- offset 7 again, no straddle
    bits[:] = 0
    bits[16368:16376] = 1
    data, starts, ff = M.walk(bits)
    m = M.meters(bits.size, starts, ff, 16384)
    assert ff.sum() == 1 and m["window"] == {7} and m["straddle"] == 0
    # ... and a chain whose byte starts an 0xFF in front has moved to 7 modulo 8: eight ones that no byte start meets make no 0xFF
    bits[:] = 0
    bits[16361:16369] = 1
    bits[0:8] = 1                                      # (byte starts 0, 15, 23, ...)
    data, starts, ff = M.walk(bits)
    m = M.meters(bits.size, starts, ff, 16384)
    assert (16367 in starts) and ff.sum() == 1         # (16361 is no byte start of this chain: the ones there make no 0xFF)
    bits[16367:16375] = 1; bits[16361:16367] = 0       # the 0xFF at byte start 16367: its step ends at 16382
    data, starts, ff = M.walk(bits)
    m = M.meters(bits.size, starts, ff, 16384)
    assert ff.sum() == 2 and m["window"] == {6} and m["straddle"] == 0
    bits[16367:16375] = 0; bits[16375:16383] = 1       # the 0xFF at byte start 16375: 16375 + 15 = 16390 -- offset 6, across the boundary
    data, starts, ff = M.walk(bits)
    m = M.meters(bits.size, starts, ff, 16384)
    assert ff.sum() == 2 and m["window"] == {6} and m["straddle"] == 1
