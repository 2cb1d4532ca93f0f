"""CPU: tests/t2ht_model.py, the writer of HT codestreams with refinement passes, pinned where something else can say what the bytes
must be: with every block at one pass its file is tests/t2layers_model.py's for the same table and seed, byte for byte, and what it
says the readers must return is what that model says; bytes handed in by the caller end up where `want` says they lie."""
import numpy as np
import pytest

import grok_amd as G
import t2layers_model as LM
import t2ht_model as HM
from t2layers_cases import tile, wide, SOP, EPH, PLT


def _same_want(a, b):
    for k in ("rows", "first_segment", "segments", "moves"):
        assert np.array_equal(a[k], b[k]), k
    assert a["appendix_bytes"] == b["appendix_bytes"] and a["pieces"] == b["pieces"]


@pytest.mark.parametrize("order", range(5))
@pytest.mark.parametrize("flags", [0, PLT, SOP | EPH, PLT | SOP | EPH])
def test_one_pass_per_block_is_the_layered_models_file(order, flags):
    for p, w, h, layers in ((tile(None, 3), 40, 64, 3), (wide(None), 260, 4, 2), (tile(None), 40, 64, 1)):
        table = LM.draw_table(p, layers, None, 40 + order)
        assert all(n == 1 for t in table for n, _ in t["layers"].values())
        for empty in (True, False):
            a, wa = LM.build(p, w, h, layers, order, flags, None, table, empty_packets=empty, seed=7)
            b, wb = HM.build(p, w, h, layers, order, flags, table, empty_packets=empty, seed=7)
            assert a == b
            _same_want(wa, wb)


def test_segments_of_an_ht_set():
    assert [HM.seg_capacity(i) for i in range(4)] == [1, 2, 1, 2]
    assert HM.split_passes(0, 0, 3) == ([1, 2], 2, 0)
    assert HM.split_passes(1, 0, 1) == ([1], 1, 1) and HM.split_passes(1, 1, 1) == ([1], 2, 0)
    assert HM.contributions("1|1|1", 0, 9, 7) == {0: (1, [9]), 1: (1, [3]), 2: (1, [4])}
    assert HM.contributions("1|-|1", 1, 9, 7) == {1: (1, [9]), 3: (1, [7])}
    assert HM.contributions("3", 2, 9, 7) == {2: (3, [9, 7])}
    assert HM.contributions("2|1", 0, 9, 7) == {0: (2, [9, 3]), 1: (1, [4])}


def test_the_callers_bytes_lie_where_want_says():
    p = tile(None)
    blocks, _ = G.tile_layout(p)
    rng = np.random.default_rng(3)
    table = []
    for i, b in enumerate(blocks):
        data = rng.integers(0, 256, 12, dtype=np.uint8).tobytes()
        table.append(dict(zbp=1, layers=HM.contributions(["3", "1|1|1", "1|2", "1"][i % 4], 0, 5, 7 if i % 4 != 3 else 0), data=data[:12 if i % 4 != 3 else 5]))
    for kw in (dict(), dict(by_layer=True)):
        cs, want = HM.build(p, 40, 64, 3, 0, PLT, table, **kw)
        for i, t in enumerate(table):
            got = b"".join(cs[at:at + n] for at, n in want["pieces"][i])
            assert got == t["data"], i
            s0, s1 = want["first_segment"][i], want["first_segment"][i + 1]
            assert [tuple(x) for x in want["segments"][s0:s1]] == ([(5, 1), (7, 2)] if i % 4 != 3 else [(5, 1)])
        assert want["appendix_bytes"] == sum(12 for i in range(len(table)) if i % 4 in (1, 2))
    assert cs.count(b"\xff\x90\x00\x0a") == 3
