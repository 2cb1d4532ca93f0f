"""CPU: the GENERAL device Tier-2 reader's parse core (grok_amd/csrc/t2_parse_layers.h) and plan (plan_t2_read_layers) against the
host reader.

tests/c/t2_parse_layers_units.cpp plays KL, KH, KC-L, KF and KP of kernels_t2read.hip on the CPU under AddressSanitizer and UBSan,
chain by chain -- in rising and in falling order --, every stream in a heap buffer of exactly its length:
  * every stream the GPU tests use (tests/t2layers_cases.py) must give the host reader's rows, first_segment, segments and
    appendix_bytes field for field and its moves as a set, or its code where it refuses -- before a GPU sees it;
  * a fixed-seed sweep of single-byte changes and truncations over the files, tallied by region, must give its tables where it
    accepts and its code where it refuses, with every loop of the core inside its stated bound;
  * the plan's numbers (chains, the file-order numbering, every scratch size) against a brute-force count from the geometry."""
import os
import subprocess

import pytest

import refharness as R
import t2layers_cases as K

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "grok_amd", "csrc")
SAN = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined"]
HALT = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1")
needs_ref = pytest.mark.skipif(not R.have_ref(), reason="oracle/_ref (the real reference) not built here")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("t2_parse_layers") / "t2_parse_layers_units")
    subprocess.check_call(["g++"] + SAN + ["-Wall", "-Wno-unused-function", "-D_GLIBCXX_ASSERTIONS", os.path.join(HERE, "c", "t2_parse_layers_units.cpp")] +
                          [os.path.join(CSRC, f) for f in ("t2_read_plan.cpp", "t2_reader.cpp", "t2_writer.cpp", "geometry.cpp", "host_common.cpp")] +
                          ["-o", path, "-lpthread"])
    return path


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """[(name, path, code)] of the model's and the goldens' cases"""
    d = tmp_path_factory.mktemp("t2_layers_files")
    out = []
    for name, cs, code, _ in K.model_cases() + K.golden_cases():
        (d / name).write_bytes(cs)
        out.append((name, str(d / name), code))
    return out


def _run(args):
    r = subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=HALT)
    assert r.returncode == 0 and "runtime error" not in r.stdout and "AddressSanitizer" not in r.stdout, r.stdout[-4000:]
    return r.stdout


def _check(exe, cases):
    out = _run([exe, "check"] + [path for _, path, _ in cases])
    seen = {}
    for line in out.splitlines():
        w = line.split()
        if len(w) == 7 and w[1] == "host":
            seen[w[0]] = (int(w[2]), int(w[4]), w[6])
    for name, _, code in cases:
        host, core, tables = seen[name]
        assert host == core == (code or 0), (name, host, core)
        assert tables == ("equal" if code is None else "-"), name


def test_every_gpu_input_passes_the_core_first(exe, files):
    _check(exe, files)
    assert sum(1 for _, _, code in files if code is not None) >= 7


def test_single_byte_changes_and_truncations_read_or_are_refused_alike(exe, files):
    out = _run([exe, "sweep"] + [path for _, path, code in files if code is None])
    assert out.startswith("ok: "), out[-800:]
    words = out.replace(",", " ").replace("[", " ").replace("]", " ").replace("(", " ").split()
    num = lambda key: int(words[words.index(key) + 1])
    assert int(words[1]) >= 2000
    for region in ("main", "sot", "plt", "sop/eph", "header", "last"):
        assert num(region) > 0, region
    assert int(words[words.index("accepted") - 1]) > 100 and int(words[words.index("refused") - 1]) > 100


def test_plan_numbers_against_the_geometry(exe, files):
    golden = [os.path.join(HERE, "golden", f) for f in sorted(os.listdir(os.path.join(HERE, "golden"))) if f.endswith(".j2k")]
    assert _run([exe, "plan"] + [path for _, path, _ in files] + golden).strip().endswith("ok: plan")


@needs_ref
def test_reference_written_layered_streams_as_written_and_with_plt(exe, tmp_path, monkeypatch):
    cases = []
    for name, cs, code, _ in K.reference_cases(monkeypatch):
        (tmp_path / name).write_bytes(cs)
        cases.append((name, str(tmp_path / name), code))
    assert len(cases) == 20
    _check(exe, cases)
    assert _run([exe, "plan"] + [path for _, path, _ in cases]).strip().endswith("ok: plan")
