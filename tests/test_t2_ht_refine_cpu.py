"""CPU: HTJ2K codestreams whose code-blocks carry refinement passes, through the host reader that takes them
(grk_amd_read_packets_refine) and through the device reader's parse core with the same option.

  * the host reader against the model (tests/t2ht_model.py, tests/t2ht_cases.py), field for field: rows, first_segment, segments,
    moves, appendix_bytes -- every order, 1 .. 3 layers, SOP / EPH / PLT, every contribution pattern, the wide tile, 2 x 2 tiles
    with edge tiles, the tile divided into a tile-part per layer, on one thread and on four;
  * its refusals, and the older calls' unchanged refusal of every such file;
  * tests/c/t2_parse_ht_units.cpp, a stand-alone program under AddressSanitizer and UBSan: the parse core with the option over every
    file the GPU tests use (the real-content files among them) must give the host reader's tables or its code, the plan its
    numbers, and a sweep of single-byte changes and truncations must be read or refused alike."""
import os
import subprocess

import numpy as np
import pytest

import grok_amd as G
import t2ht_cases as K

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "grok_amd", "csrc")
SAN = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined"]
HALT = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1")


@pytest.fixture(scope="module")
def cases():
    return K.table_cases()


@pytest.fixture(scope="module")
def contents():
    return K.content_cases()


def same_tables(got, want, name):
    assert np.array_equal(got["rows"], want["rows"]), name
    assert np.array_equal(got["first_segment"], want["first_segment"]), name
    assert np.array_equal(got["segments"], want["segments"]), name
    assert got["appendix_bytes"] == want["appendix_bytes"], name
    order = lambda m: np.sort(m, order=["dst"])
    assert np.array_equal(order(got["moves"]), order(want["moves"])), name


def test_host_reader_returns_the_models_tables(cases):
    read, patterns = 0, set()
    for name, cs, code, want in cases:
        if code is not None:
            continue
        for threads in (1, 4):
            same_tables(G.read_packets_refine(cs, threads=threads), want, name)
        read += 1
        f, s = want["first_segment"], want["segments"]
        for i in range(len(want["rows"])):
            patterns.add((len(want["pieces"][i]), tuple(int(x) for x in s["numpasses"][f[i]:f[i + 1]]), bool(f[i + 1] - f[i] == 2 and s["length"][f[i] + 1] == 0)))
    assert read >= 30 + 2 + 3 + 3
    # pieces, passes per segment, refinement segment of no bytes: one piece with 3, 2, 1 passes; two and three pieces; never included;
    # two and three passes over a refinement segment of 0 bytes
    for need in ((1, (1, 2), False), (1, (1, 1), False), (1, (1,), False), (0, (), False), (2, (1, 2), False), (3, (1, 2), False), (2, (1, 1), False),
                 (1, (1, 2), True), (1, (1, 1), True)):
        assert need in patterns, need


def test_real_content_files_read_as_built(contents):
    for c in contents:
        got = G.read_packets_refine(c.cs)
        same_tables(got, c.want, c.name)
        # (one layer: every block in one piece; three: the blocks with refinement bytes go through moves into the appendix)
        assert got["appendix_bytes"] == 0 or c.name.endswith("L3"), c.name
        if c.name.endswith("L3") and len(got["rows"]) > 4:
            assert got["appendix_bytes"] > 0 and len(got["moves"]) > len(got["rows"]) // 2, c.name


def test_refusals_of_the_refine_reader(cases):
    seen = 0
    for name, cs, code, _ in cases:
        if code is None:
            continue
        for threads in (1, 4):
            with pytest.raises(G.ReaderError) as e:
                G.read_packets_refine(cs, threads=threads)
            assert e.value.code == code, name
            if code == G.ERR_UNSUPPORTED:
                assert "more than one pass" in str(e.value) and "placeholder passes or a second HT set" in str(e.value), name
            else:
                assert "runs past" in str(e.value), name
        seen += 1
    assert seen == 6


def test_the_older_calls_keep_refusing(cases, contents):
    cs, _ = K.three_pass_file()
    files = [cs] + [c.cs for c in contents[:2]] + [x[1] for x in cases if x[2] is None and "-L1-" not in x[0]][:6]
    for f in files:
        for call in (G.read_packets, G.read_packets_parts):
            with pytest.raises(G.ReaderError) as e:
                call(f)
            assert e.value.code == G.ERR_UNSUPPORTED and "an HT code-block with more than one pass" in e.value.reason and "of a kind" not in e.value.reason, str(e.value)


def test_a_cleanup_only_file_reads_the_same_through_every_call():
    c = K.content_file(K.SHAPES[1], False, K.PLT, refine=False)
    a, b, r = G.read_packets(c.cs), G.read_packets_parts(c.cs), G.read_packets_refine(c.cs)
    for k in ("rows", "first_segment", "segments", "moves"):
        assert np.array_equal(a[k], r[k]) and np.array_equal(b[k], r[k]), k
    same_tables(r, c.want, c.name)


# ---- the parse core on the CPU -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("t2_parse_ht") / "t2_parse_ht_units")
    subprocess.check_call(["g++"] + SAN + ["-Wall", "-Wno-unused-function", "-D_GLIBCXX_ASSERTIONS", os.path.join(HERE, "c", "t2_parse_ht_units.cpp")] +
                          [os.path.join(CSRC, f) for f in ("t2_read_plan.cpp", "t2_reader.cpp", "t2_writer.cpp", "geometry.cpp", "host_common.cpp")] +
                          ["-o", path, "-lpthread"])
    return path


@pytest.fixture(scope="module")
def files(tmp_path_factory, cases, contents):
    """[(name, path, code)] of every file the GPU tests use"""
    d = tmp_path_factory.mktemp("t2_ht_files")
    out = []
    for name, cs, code in [(n, cs, code) for n, cs, code, _ in cases] + [(c.name, c.cs, None) for c in contents] + [("three-pass", K.three_pass_file()[0], None)]:
        (d / name).write_bytes(cs)
        out.append((name, str(d / name), code))
    return out


def _run(args):
    r = subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=HALT)
    assert r.returncode == 0 and "runtime error" not in r.stdout and "AddressSanitizer" not in r.stdout, r.stdout[-4000:]
    return r.stdout


def test_every_gpu_input_passes_the_core_first(exe, files):
    out = _run([exe, "check"] + [path for _, path, _ in files])
    seen, reasons = {}, {}
    last = None
    for line in out.splitlines():
        w = line.split()
        if len(w) == 7 and w[1] == "host":
            seen[w[0]] = (int(w[2]), int(w[4]), w[6])
            last = w[0]
        elif line.startswith("  core: ") and last:
            reasons[last] = line[8:]
    for name, _, code in files:
        host, core, tables = seen[name]
        assert host == core == (code or 0), (name, host, core)
        assert tables == ("equal" if code is None else "-"), name
        if code == G.ERR_UNSUPPORTED:
            assert "more than one pass" in reasons[name], (name, reasons[name])
        if code == G.ERR_INVALID:
            assert "runs past" in reasons[name], (name, reasons[name])
    assert sum(1 for _, _, code in files if code is not None) == 6


def test_the_reader_without_the_option_refuses_them(exe, files):
    out = _run([exe, "old"] + [path for name, path, code in files if code is None and "-L1-" not in name and not name.endswith("cleanup")])
    lines = [l for l in out.splitlines() if " old " in l]
    assert len(lines) >= 20
    for l in lines:
        assert " old -2 " in l and "an HT code-block with more than one pass" in l and "of a kind" not in l, l


def test_single_byte_changes_and_truncations_read_or_are_refused_alike(exe, files):
    out = _run([exe, "sweep"] + [path for _, path, code in files if code is None])
    assert out.startswith("ok: "), out[-800:]
    w = out.split()
    assert int(w[1]) >= 2000
    accepted, refused, unsupported = (int(w[w.index(k) - 1]) for k in ("accepted", "refused", "unsupported"))
    assert accepted > 100 and refused > 100 and unsupported > 0


def test_plan_numbers_with_the_option(exe, files):
    assert _run([exe, "plan"] + [path for _, path, _ in files]).strip().endswith("ok: plan")
