"""CPU: tests/t2msbs_model.py -- the Python restatement of a packet header under the general zero-bit-plane tag tree, which
tests/test_gpu_t2_msbs.py asserts its tables' conditions with -- pinned on the host writer: for a few small geometries and random
tables the model's stuffed bytes are the header bytes inside grk_amd_write_tile_part(..., flags | CS_BLOCK_MSBS), packet by packet; the
node minima and the per-block fields are checked on trees made by hand."""
import numpy as np
import pytest

import grok_amd as G
import t2model as M
import t2msbs_model as MM


@pytest.mark.parametrize("make,hi", [
    (dict(w=64, h=64, comps=1, prec=8, levels=0), 300),
    (dict(w=192, h=320, comps=1, prec=8, levels=0), 4095),
    (dict(w=164, h=140, comps=1, prec=8, levels=0, cblk=(2, 2)), 100),
    (dict(w=40, h=64, comps=1, prec=8, levels=1, cblk=(2, 2)), 300),
    (dict(w=200, h=136, comps=3, prec=12, levels=3, cblk=(3, 4)), 70000),
])
def test_model_headers_are_the_host_writers_with_block_msbs(make, hi):
    p = G.TileParams.make(make.pop("w"), make.pop("h"), make.pop("comps"), make.pop("prec"), make.pop("levels"), **make)
    packets = M.packets_of(p)
    nrows = sum(k["rows"].size for k in packets)
    rng = np.random.default_rng(nrows + hi)
    coded = rng.integers(0, 256, hi + 4096, dtype=np.uint8)
    for rep in range(3):
        table = np.zeros(nrows, G.capi.CODED_DTYPE)
        table["length"] = rng.integers(0, hi + 1, nrows)
        table["offset"] = rng.integers(0, coded.size - hi, nrows)
        table["missing_msbs"] = rng.integers(0, 64, nrows) if rep else rng.integers(0, 3, nrows)
        part = G.write_tile_part(p, 3, table, coded, G.CS_BLOCK_MSBS)
        at, total = 14, 0                              # SOT 12, SOD 2
        for k in packets:
            lengths, msbs = table["length"][k["rows"]], table["missing_msbs"][k["rows"]]
            data, _ = MM.header(k["bands"], lengths, msbs, 512 * 32)
            assert part[at:at + len(data)] == data, "packet at byte %d" % at
            total += int(MM.block_fields(k["bands"], lengths, msbs)[3].sum()) + 1
            assert MM.raw_bits(k["bands"], lengths, msbs).size == int(MM.block_fields(k["bands"], lengths, msbs)[3].sum()) + 1
            at += len(data)
            for r in k["rows"]:
                o, n = int(table["offset"][r]), int(table["length"][r])
                assert part[at:at + n] == coded[o:o + n].tobytes()
                at += n
        assert at == len(part)


def test_constant_values_are_the_plain_model():
    bands = [(3, 5, 9), (7, 2, 9)]
    rng = np.random.default_rng(1)
    lengths = rng.integers(0, 5000, 29)
    assert np.array_equal(MM.raw_bits(bands, lengths, np.full(29, 8)), M.raw_bits(bands, lengths))
    nn, zeros, inc, _ = MM.block_fields(bands, lengths, np.full(29, 8))
    n0, z0, i0 = M.block_fields(bands, lengths)
    assert np.array_equal(nn, n0) and np.array_equal(zeros, z0) and np.array_equal(inc, i0)


def test_node_minima_and_fields_on_a_tree_made_by_hand():
    # 3 x 2:   5 7 | 2        level 1 (2 x 1): min(5, 7, 6, 9) = 5 | min(2, 4) = 2     level 2: 2
    #          6 9 | 4
    msbs = [5, 7, 2, 6, 9, 4]
    lv = MM.levels(3, 2, msbs)
    assert [a.tolist() for a in lv] == [[[5, 7, 2], [6, 9, 4]], [[5, 2]], [[2]]]
    nn, zeros, inc, nbits = MM.block_fields([(3, 2, 10)], [0] * 6, msbs)
    # block 0: three new nodes, zeros up to its own 5; (1, 0): one new node under the 5; (2, 0): two new nodes under the root's 2
    assert nn.tolist() == [3, 1, 2, 1, 1, 1] and zeros.tolist() == [5, 2, 0, 1, 4, 2]
    assert nbits.tolist() == [2 * n + z + 5 for n, z in zip(nn.tolist(), zeros.tolist())]
    bits = MM.raw_bits([(3, 2, 10)], [0] * 6, msbs)
    #               '1'  block 0: 111 | 00 1 (root 2) | 000 1 (5) | 1 (5) | 0 0 000
    assert "".join(map(str, bits[:1 + 16].tolist())) == "1" + "111" + "001" + "0001" + "1" + "0" + "0" + "000"
    # the root's minimum lies at its last leaf but one, level 1's second node has its at its first: level 2 alone is "late"
    assert MM.late_minimum_levels(3, 2, msbs) == {2}
    assert MM.late_minimum_levels(3, 2, [1, 2, 3, 4, 5, 6]) == set()
    assert MM.late_minimum_levels(3, 2, [6, 5, 4, 3, 2, 1]) == {1, 2}
