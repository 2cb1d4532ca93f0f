"""CPU: the device Tier-2 reader's parse core (grok_amd/csrc/t2_parse.h) and plan (t2_read_plan.cpp) against the host reader.

tests/c/t2_parse_units.cpp plays the three kernels of kernels_t2read.hip on the CPU, one chain after the other, under AddressSanitizer
and UBSan, every stream in a heap buffer of exactly its length:
  * the sweep: files it writes with the host writer from fixed-seed tables -- PLT, TLM, SOP, EPH on and off, the five orders,
    precinct grids, one and three components, 4:2:0, tiles of differing geometry, per-block zero bit-planes, lengths 0, 2^k - 1, 2^k,
    2^k + 1 up to 2^20, band grids of 65 x 1 and 1 x 65 blocks, headers with 0xFF inside and at their end (counted) -- must give the
    rows of read_stream_packets (threads 1); several thousand fixed-seed single-byte changes and truncations over every region (tallied)
    must give its rows where it accepts and its code where it refuses, with every loop of the core inside its stated bound;
  * the plan's numbers against the tiles' precincts and blocks, its shared descriptors, its refusals;
  * every stream the GPU tests use (tests/t2read_cases.py), the twelve named corruptions among them, before a GPU sees it."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "grok_amd", "csrc")
SAN = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined"]
HALT = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("t2_parse") / "t2_parse_units")
    subprocess.check_call(["g++"] + SAN + ["-Wall", "-Wno-unused-function", "-D_GLIBCXX_ASSERTIONS", os.path.join(HERE, "c", "t2_parse_units.cpp")] +
                          [os.path.join(CSRC, f) for f in ("t2_read_plan.cpp", "t2_reader.cpp", "t2_writer.cpp", "geometry.cpp", "host_common.cpp")] +
                          ["-o", path, "-lpthread"])
    return path


def _run(args):
    r = subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=HALT)
    assert r.returncode == 0 and "runtime error" not in r.stdout and "AddressSanitizer" not in r.stdout, r.stdout[-4000:]
    return r.stdout


def test_rows_and_refusals_are_the_host_readers_under_sanitizers(exe):
    out = _run([exe])
    assert out.startswith("ok: "), out[-800:]
    words = out.replace(",", " ").replace("[", " ").replace("]", " ").split()
    num = lambda key: int(words[words.index(key) + 1])
    assert int(words[1]) > 5000 and int(words[words.index("corruptions") - 1]) >= 3000
    for region in ("main", "sot", "plt", "sop/eph", "header", "last"):
        assert num(region) > 0, region
    assert num("inside") > 0 and int(words[words.index("ending") + 3]) > 0        # headers with 0xFF inside, headers ending on 0xFF


def test_plan_numbers_shared_descriptors_and_refusals(exe):
    assert _run([exe, "plan"]).strip().endswith("ok: plan")


def test_every_gpu_input_passes_the_core_first(exe, tmp_path):
    import t2read_cases as K
    cases = K.reading_cases() + K.corruption_cases() + K.golden_cases()
    names = [n for n, _, _ in cases]
    assert len(set(names)) == len(names)
    for name, data, _ in cases:
        (tmp_path / name).write_bytes(data)
    out = _run([exe, "check"] + [str(tmp_path / n) for n in names])
    seen = {}
    for line in out.splitlines():
        w = line.split()
        if len(w) == 7 and w[1] == "host":
            seen[w[0]] = (int(w[2]), int(w[4]), w[6])
    for name, _, code in cases:
        host, core, rows = seen[name]
        if "_sty05_" in name or "_sty3f_" in name:
            assert core == code          # (the plan refuses what the host reader takes: several codeword segments)
            continue
        assert host == core == (code or 0), (name, host, core)
        assert rows == ("equal" if code is None else "-"), name
    assert sum(1 for n, _, c in K.corruption_cases() if c) == 12
