"""CPU: the Python writer of layered codestreams (tests/t2layers_model.py) pinned on the host reader: G.read_packets of every file it
writes returns the table the file was written from -- lengths, passes, segments, pieces --, and refuses the files built to be refused
with the code the case names.  The goldens and the host reader's own tests (tests/test_t2_reader_cpu.py) stay the ground under it."""
import numpy as np
import pytest

import grok_amd as G
import t2layers_cases as K
import t2layers_model as LM


@pytest.fixture(scope="module")
def cases():
    return K.model_cases()


def test_the_host_reader_returns_the_chosen_tables(cases):
    read = 0
    for name, cs, code, want in cases:
        if code is not None:
            with pytest.raises(G.ReaderError) as e:
                G.read_packets(cs)
            assert e.value.code == code, (name, e.value.reason)
            continue
        got = G.read_packets(cs)
        for f in ("offset", "length", "missing_msbs"):
            assert np.array_equal(got["rows"][f], want["rows"][f]), (name, f)
        assert np.array_equal(got["first_segment"], want["first_segment"]), name
        assert np.array_equal(got["segments"], want["segments"]), name
        assert got["appendix_bytes"] == want["appendix_bytes"], name
        assert np.array_equal(np.sort(got["moves"], order="dst"), want["moves"]), name
        # the pieces: a row's bytes are its pieces' in order, out of the file or out of the appendix the moves fill
        app = bytearray(got["appendix_bytes"])
        for m in got["moves"]:
            app[int(m["dst"]):int(m["dst"]) + int(m["len"])] = cs[int(m["src"]):int(m["src"]) + int(m["len"])]
        for r, pieces in enumerate(want["pieces"]):
            o, n = int(got["rows"]["offset"][r]), int(got["rows"]["length"][r])
            have = cs[o:o + n] if o < len(cs) else bytes(app[o - len(cs):o - len(cs) + n])
            assert have == b"".join(cs[s:s + k] for s, k in pieces), (name, r)
        read += 1
    assert read >= 60


def test_the_cases_cover_what_they_name(cases):
    by = dict((n, (cs, code, want)) for n, cs, code, want in cases)
    infos = dict((n, G.read_header(cs)) for n, (cs, _, _) in by.items())
    assert set((i.flags >> 8) & 7 for i in infos.values()) == {0, 1, 2, 3, 4}
    assert {1, 3} <= set(i.base.num_comps for i in infos.values())
    assert {0, 1, 4, 5} <= set(i.base.reserved[1] for i in infos.values() if i.base.reserved[0]) and any(not i.base.reserved[0] for i in infos.values())
    for flag in (G.CS_SOP, G.CS_EPH, G.CS_PLT):
        assert any(i.flags & flag for i in infos.values()) and any(not i.flags & flag for i in infos.values())
    assert infos["130-layers-first-inclusion-in-129-f0"].num_layers == 130
    want = by["one-piece-per-block-f2"][2]
    assert want["appendix_bytes"] == 0 and len(want["moves"]) == 0
    want = by["both-kinds-of-block"][2]
    pieces = [len(p) for p in want["pieces"]]
    assert want["appendix_bytes"] > 0 and pieces.count(1) > 10 and sum(1 for n in pieces if n > 1) > 10
    # LAZY: ten passes over two layers in the first segment, then the raw pair and the clean-up pass
    want = by["lazy-layer-boundaries-f8"][2]
    r = int(np.nonzero(want["rows"]["length"])[0][0])
    f0, f1 = int(want["first_segment"][r]), int(want["first_segment"][r + 1])
    assert [tuple(s) for s in want["segments"][f0:f1].tolist()] == [(24, 10), (5, 2), (2, 1)]
    want = by["one-segment-growing-over-three-layers"][2]
    r = int(np.nonzero(want["rows"]["length"])[0][0])
    assert int(want["first_segment"][r + 1]) - int(want["first_segment"][r]) == 1 and tuple(want["segments"][0].tolist()) == (543, 6)
    assert len(want["pieces"][r]) == 3
    # 164 passes in all are accepted
    want = by["passes-164-f0"][2]
    assert sorted(int(s["numpasses"]) for s in want["segments"]) == [87, 164]


def test_tag_tree_and_stuffing_of_the_model():
    bits = []
    t = LM.TagTree(3, 2, [1, 3, 2, 3, 2, 3])
    t.encode(0, 0, 1, bits)            # the root (the minimum, 1) is not below 1: one zero, nothing known yet
    assert bits == [0] and not t.known[0][0, 0]
    t.encode(0, 0, 2, bits)            # the root is 1, the node below it is 1, the leaf is 1
    assert bits == [0, 1, 1, 1] and t.known[0][0, 0]
    assert LM.stuff([1] * 8) == b"\xff\x00" and LM.stuff([1] * 8 + [1, 0, 1]) == b"\xff\x50" and LM.stuff([0, 1]) == b"\x40"
