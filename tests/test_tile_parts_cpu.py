"""CPU: codestreams whose tiles are divided into tile-parts, through grk_amd_read_packets_parts (grok_amd/csrc/t2_reader.cpp).

The files come from tests/tileparts.py, the pure-Python model that cuts a file with one tile-part per tile at packet boundaries; a
tile's packet sequence is the concatenation of its tile-parts' bodies, so the cut file must read as the undivided file does with every
offset sent through the model's map.  Where the reference is built its decoder says the same of its own files: the pixels of a cut
file are the undivided file's -- which is what makes the model's files trustworthy.

tests/c/t2_parts_units.cpp is the reader as a stand-alone program under AddressSanitizer and UBSan; every stream of
tests/tileparts_cases.py -- the good ones and the refused ones -- goes through it, each in a heap buffer of exactly its length."""
import os
import subprocess

import numpy as np
import pytest

import grok_amd as G
import refharness as R
import synth
import tileparts as TP
import tileparts_cases as TC

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "grok_amd", "csrc")
SAN = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined"]
HALT = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1")
needs_ref = pytest.mark.skipif(not R.have_ref(), reason="oracle/_ref (the real reference) not built here")
REF_VARS = ("REF_PROG_ORDER", "REF_PRECINCTS", "REF_CSTY", "REF_WRITE_PLT", "REF_WRITE_TLM", "REF_LAYERS", "REF_IMG_X0", "REF_IMG_Y0")


@pytest.fixture(scope="module")
def cases():
    return TC.cases()


@pytest.fixture(scope="module")
def refusals():
    return TC.refusals()


def expected(base, cut):
    """the undivided file's table with its positions mapped into the cut file"""
    want = G.read_packets(base)
    rows = want["rows"].copy()
    inside = (rows["length"] > 0) & (rows["offset"] < len(base))
    rows["offset"][inside] = cut.map(rows["offset"][inside])
    behind = (rows["length"] > 0) & ~inside
    rows["offset"][behind] = rows["offset"][behind] - len(base) + len(cut.cs)
    moves = want["moves"].copy()
    if len(moves):
        moves["src"] = cut.map(moves["src"])
    return dict(rows=rows, first_segment=want["first_segment"], segments=want["segments"], moves=moves, appendix_bytes=want["appendix_bytes"])


def move_set(moves):
    return sorted((int(m["dst"]), int(m["src"]), int(m["len"])) for m in moves)


def same_table(got, want):
    assert np.array_equal(got["rows"], want["rows"])
    assert np.array_equal(got["first_segment"], want["first_segment"]) and np.array_equal(got["segments"], want["segments"])
    assert move_set(got["moves"]) == move_set(want["moves"]) and got["appendix_bytes"] == want["appendix_bytes"]


def check_cut(base, cut):
    want = expected(base, cut)
    for threads in (1, 4):
        same_table(G.read_packets_parts(cut.cs, None, threads), want)
    # every block's bytes are the undivided file's
    a, b = np.frombuffer(base, np.uint8), np.frombuffer(cut.cs, np.uint8)
    old = G.read_packets(base)["rows"]
    for r0, r1 in zip(old, want["rows"]):
        n = int(r0["length"])
        if n and int(r0["offset"]) < len(base):
            assert np.array_equal(a[int(r0["offset"]):int(r0["offset"]) + n], b[int(r1["offset"]):int(r1["offset"]) + n])


# ---- the model itself ------------------------------------------------------------------------------------------------------------
def test_the_model_cuts_only_between_packets_and_keeps_every_byte():
    p = TC.tile_params(precincts=[(3, 3), (4, 3)])
    cs = TC.one_tile_file(p, TC.table_of(TC.draw_lengths(p, 1), 2), G.CS_PLT | G.CS_SOP)
    lens = TP.scan(cs)["tiles"][0].lens
    c = TP.cut(cs, boundaries={0: [4, 4, 30]}, tlm="write")
    assert [p_.packets for p_ in c.parts] == [(0, 4), (4, 0), (4, 26), (30, 6)] and [p_.tpsot for p_ in c.parts] == [0, 1, 2, 3]
    body = b"".join(c.cs[p_.body_at:p_.body_end] for p_ in c.parts)
    t = TP.scan(cs)["tiles"][0]
    assert body == cs[t.body_at:t.body_end] and sum(lens) == len(body)
    for p_ in c.parts:
        assert c.cs[p_.at:p_.at + 4] == b"\xff\x90\x00\x0a" and TP.u32(c.cs, p_.at + 6) == p_.length and c.cs[p_.body_at - 2:p_.body_at] == b"\xff\x93"
        assert c.cs[p_.at + 10] == p_.tpsot and c.cs[p_.at + 11] == 4
    # the library's own locator finds them through the model's TLM as through the Psot chain
    found, used = G.locate_tile_parts(c.cs)
    assert used and [(o, n, t_) for o, n, t_ in found] == [(p_.at, p_.length, 0) for p_ in c.parts]
    found, used = G.locate_tile_parts(TP.cut(cs, boundaries={0: [4, 4, 30]}).cs)
    assert not used and [n for _, n, _ in found] == [p_.length - 0 for p_ in TP.cut(cs, boundaries={0: [4, 4, 30]}).parts]
    # the uncut file through the model is the file without TLM
    same = TP.cut(cs, boundaries={})
    assert same.cs == cs and int(same.map([t.body_at])[0]) == t.body_at


# ---- the reader --------------------------------------------------------------------------------------------------------------------
def test_table_built_cut_files_read_as_their_undivided_files(cases):
    assert len(cases) > 70
    for name, base, cut in cases:
        try:
            check_cut(base, cut)
        except (AssertionError, G.ReaderError) as e:
            raise AssertionError("%s: %s" % (name, e))


def test_the_older_call_still_refuses_every_cut_file(cases):
    for name, base, cut in cases[:3] + cases[-3:]:
        with pytest.raises(G.ReaderError) as e:
            G.read_packets(cut.cs)
        assert e.value.code == G.ERR_UNSUPPORTED and "more than one tile-part per tile" in e.value.reason, name


def test_an_undivided_file_reads_the_same_through_both_calls(cases):
    for name, base, cut in cases[::9]:
        same_table(G.read_packets_parts(base, None, 3), G.read_packets(base, None, 3))


def test_refusals_by_code_with_a_reason_that_names_tile_and_part(refusals):
    assert len(refusals) >= 20
    for name, cs, code, words in refusals:
        for threads in (1, 4):
            with pytest.raises(G.ReaderError) as e:
                G.read_packets_parts(cs, None, threads)
            assert e.value.code == code, (name, threads, e.value.code, e.value.reason)
            assert all(w in e.value.reason for w in words), (name, threads, e.value.reason)


# ---- under the sanitizers ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("t2_parts") / "t2_parts_units")
    subprocess.check_call(["g++"] + SAN + ["-Wall", "-D_GLIBCXX_ASSERTIONS", os.path.join(HERE, "c", "t2_parts_units.cpp")] +
                          [os.path.join(CSRC, f) for f in ("t2_read_plan.cpp", "t2_reader.cpp", "t2_writer.cpp", "geometry.cpp", "host_common.cpp")] + ["-o", path, "-lpthread"])
    return path


def _run(args):
    r = subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=HALT)
    assert r.returncode == 0 and "runtime error" not in r.stdout and "AddressSanitizer" not in r.stdout, r.stdout[-4000:]
    return r.stdout


def case_names():
    """what the sanitized program is given, in order (tests/test_gpu_tile_parts.py holds its own list against this one)"""
    return [c[0] for c in TC.cases()] + [r[0] for r in TC.refusals()]


def test_every_stream_through_the_sanitized_program(exe, cases, refusals, tmp_path):
    files, want = [], []
    for name, base, cut in cases:
        files.append((name, cut.cs))
        want.append(0)
    for name, cs, code, _ in refusals:
        files.append((name, cs))
        want.append(code)
    assert [f[0] for f in files] == case_names()
    paths = []
    for name, cs in files:
        paths.append(str(tmp_path / (name + ".j2k")))
        open(paths[-1], "wb").write(cs)
    lines = _run([exe, "read"] + paths).strip().split("\n")
    assert len(lines) == len(files)
    for (name, cs), code, line in zip(files, want, lines):
        assert int(line.split()[1]) == code, line
    # the good files: the table the library gave Python
    for (name, base, cut), line in zip(cases, lines):
        got = G.read_packets_parts(cut.cs)
        f = line.split()
        assert [int(v) for v in f[2:6]] == [len(got["rows"]), len(got["segments"]), len(got["moves"]), got["appendix_bytes"]], line


def test_the_kernels_played_on_the_cpu_give_the_host_readers_rows_and_codes(exe, cases, refusals, tmp_path):
    """KL-P, KH-P and KC-L's part stepping from the shared headers, under the sanitizers, on every stream a GPU test hands to them"""
    files = [(name, cut.cs) for name, base, cut in cases] + [(name, base) for name, base, cut in cases[::7]] + [(name, cs) for name, cs, code, _ in refusals]
    paths = []
    for k, (name, cs) in enumerate(files):
        paths.append(str(tmp_path / ("%03d-%s.j2k" % (k, name))))
        open(paths[-1], "wb").write(cs)
    lines = _run([exe, "play"] + paths).strip().split("\n")
    assert len(lines) == len(files), lines[-3:]
    for (name, base, cut), line in zip(cases, lines):
        assert line.split()[1] == "0", line
    for (name, cs, code, _), line in zip(refusals, lines[-len(refusals):]):
        assert int(line.split()[1]) == code, line


def test_every_prefix_and_every_tile_part_header_byte_changed(exe, cases, tmp_path):
    """hostile input: the reader may read or refuse, under the sanitizers it must do neither with a byte outside the stream"""
    names = ("order-2-f%x" % (TC.PLT | TC.SOP | TC.EPH), "plt-in-some-parts", "layers-rpcl-inside-a-precinct", "420-two-tiles-f%x" % TC.SOP)
    chosen = [c for c in cases if c[0] in names]
    assert len(chosen) == 4
    paths = []
    for name, base, cut in chosen:
        paths.append(str(tmp_path / (name + ".j2k")))
        open(paths[-1], "wb").write(cut.cs)
    for line, (name, base, cut) in zip(_run([exe, "prefixes"] + paths).strip().split("\n"), chosen):
        good, refused = (int(v) for v in line.split()[1:])
        assert refused >= len(cut.cs) and good >= 0


# ---- the reference's own files ---------------------------------------------------------------------------------------------------
def ref_file(monkeypatch, kind):
    """a 3 x 80 x 96 image of smooth content in four tiles of 64 x 64, three resolutions, as the reference writes it"""
    for k in REF_VARS:
        monkeypatch.delenv(k, raising=False)
    env, kw = {
        "ht-lrcp-plt": (dict(REF_PROG_ORDER=0, REF_WRITE_PLT=1), dict(ht=1)),
        "ht-cprl": (dict(REF_PROG_ORDER=4, REF_CSTY=2), dict(ht=1)),
        "p1-layers-lrcp": (dict(REF_PROG_ORDER=0, REF_LAYERS="20,5,1", REF_CSTY=2), dict(ht=0)),
        "p1-layers-rpcl": (dict(REF_PROG_ORDER=2, REF_LAYERS="20,5,1", REF_CSTY=2), dict(ht=0)),
        "ht-layers-rlcp": (dict(REF_PROG_ORDER=1, REF_LAYERS="20,5,1", REF_CSTY=2), dict(ht=1)),
    }[kind]
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    px = synth.g2_mid(3, 80, 96, 8)
    return px, R.encode(px, 8, mode=1, TW=64, TH=64, numres=3, cblksty=0, **kw)[0]


REF_KINDS = ["ht-lrcp-plt", "ht-cprl", "p1-layers-lrcp", "p1-layers-rpcl", "ht-layers-rlcp"]


@needs_ref
@pytest.mark.parametrize("kind", REF_KINDS)
def test_reference_files_cut_nine_ways_read_as_undivided_and_decode_to_the_same_pixels_in_the_reference(monkeypatch, kind):
    """The reference's decoder returns the undivided file's pixels for every cut but TNsot = 0 in every tile-part: there it returns
    other pixels without an error (it evidently stops early), so that cut is held to the undivided file's table alone -- and, on the
    GPU, to this library's own decode of the undivided file -- never to the reference's pixels."""
    px, cs = ref_file(monkeypatch, kind)
    assert G.read_header(cs).num_tiles == 4
    want = R.decode(cs, 3, 80, 96)
    for name, kw in TP.NINE_CUTS:
        kw = dict(kw)
        if not G.read_header(cs).flags & G.CS_PLT and "plt" not in kw:
            kw["plt"] = "keep" if name in ("thirds", "interleaved") else "drop"
        c = TP.cut(cs, **kw)
        assert len(c.parts) > 4, name
        try:
            check_cut(cs, c)
        except (AssertionError, G.ReaderError) as e:
            raise AssertionError("%s %s: %s" % (kind, name, e))
        if name != "tnsot-none":
            got = R.decode(c.cs, 3, 80, 96)
            assert np.array_equal(np.asarray(got), np.asarray(want)), (kind, name)
