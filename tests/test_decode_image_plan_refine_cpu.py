"""CPU: what a whole-image decode decides about an HT file with refinement passes (grok_amd/csrc/decode_image_plan.cpp:
read_decode_packets, replan_for_refinement, plan_image_dest with ImageDestIn::ht_refine, group_checks_planes16; decode_plan.cpp:
decode_takes_planes16), through tests/c/decode_image_plan_refine_units.cpp -- a stand-alone program that goes decode_view's way
up to the first launch, built from the library's HIP-free sources.

  * a file with refinement segments is read twice (refused, then by the reader that takes them), gets its segment lists
    (want_segs), leaves the int16 planes and their status check alone, and a window of a one-tile file goes the Staged route instead
    of the region decoder's;
  * a cleanup-only file is read once and decided exactly as before -- int16 planes, region decoder and all;
  * a reduced decode drops the dropped resolutions' rows and their segment lists together: what is left adds up
    (plan_ht_refinement checks every kept row's segments against its length)."""
import os
import subprocess

import pytest

import grok_amd as G
import t2ht_cases as K

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DIRECT, REGION, RUNS, STAGED, SURFACE = range(5)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    csrc = os.path.join(ROOT, "grok_amd", "csrc")
    out = str(tmp_path_factory.mktemp("decode_image_plan_refine") / "decode_image_plan_refine_units")
    srcs = ["decode_image_plan.cpp", "decode_plan.cpp", "image_view_plan.cpp", "surface_plan.cpp", "t2_reader.cpp", "t2_writer.cpp", "geometry.cpp", "host_common.cpp"]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-D_GLIBCXX_ASSERTIONS", "-fsanitize=address,undefined",
                           os.path.join(HERE, "c", "decode_image_plan_refine_units.cpp")] + [os.path.join(csrc, s) for s in srcs] + ["-o", out, "-lpthread"])
    return out


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("refine_files")
    out = {}
    for shape in K.SHAPES:
        for layered in (False, True):
            for refine in (True, False):
                if not refine and layered:
                    continue
                c = K.content_file(shape, layered, K.PLT, refine=refine)
                (d / c.name).write_bytes(c.cs)
                out[c.name] = (str(d / c.name), c)
    return out


def decide(exe, path, reduce=0, window=(0, 0, 0, 0), planes16=1):
    r = subprocess.run([exe, path, str(reduce)] + [str(v) for v in window] + [str(planes16)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       env=dict(os.environ, UBSAN_OPTIONS="halt_on_error=1"))
    assert r.returncode == 0 and "runtime error" not in r.stdout and "AddressSanitizer" not in r.stdout, r.stdout[-3000:]
    w = r.stdout.split()
    assert w[0] == "first", r.stdout
    out = {}
    i = 0
    while i < len(w):
        k = w[i]
        n = 2 if k in ("route", "want_segs", "checks16") else 1
        out[k] = tuple(int(x) for x in w[i + 1:i + 1 + n]) if n == 2 else int(w[i + 1])
        i += 1 + n
    return out


def test_refined_files_get_segment_lists_and_int32_planes(exe, files):
    for name, (path, c) in files.items():
        if name.endswith("cleanup"):
            continue
        d = decide(exe, path)
        assert d["first"] == G.ERR_UNSUPPORTED and d["reread"] == 1 and d["second"] == 1, name
        assert d["want_segs"] == (0, 1) and d["h16"] == 0 and d["checks16"][1] == 0, name
        tiles = len(c.tiles)
        assert d["route"] == ((DIRECT, DIRECT) if tiles == 1 else (STAGED, STAGED)), name
        f, s = c.want["first_segment"], c.want["segments"]
        want = sum(1 for i in range(len(f) - 1) if f[i + 1] - f[i] == 2 and s["length"][f[i] + 1] > 0)          # (K5c's blocks: a second segment that has bytes)
        assert d["rows"] == len(c.want["rows"]) and d["refined"] == want and d["dropped"] == 0, name
    # the int16-plane trap: 8-bit reversible with at least one level would have gone to the int16 planes
    assert decide(exe, files["200x120-L1"][0])["checks16"] == (1, 0)
    assert decide(exe, files["200x120-L3"][0], reduce=1)["checks16"] == (1, 0)
    assert decide(exe, files["100x70-tiles-L3"][0])["checks16"] == (0, 0)          # (9/7: never theirs)


def test_cleanup_only_files_are_decided_as_before(exe, files):
    for name, (path, c) in files.items():
        if not name.endswith("cleanup"):
            continue
        d = decide(exe, path)
        assert d["first"] == 0 and d["reread"] == 0 and d["second"] == 0 and d["want_segs"] == (0, 0) and d["refined"] == 0, name
        assert d["route"][0] == d["route"][1] and d["checks16"][0] == d["checks16"][1], name
    d = decide(exe, files["200x120-L1-cleanup"][0])
    assert d["checks16"] == (1, 1) and d["h16"] == 1
    assert decide(exe, files["200x120-L1-cleanup"][0], planes16=0)["h16"] == 0
    # ... and its window by the region decoder
    assert decide(exe, files["200x120-L1-cleanup"][0], window=(33, 17, 81, 57))["route"] == (REGION, REGION)


def test_a_window_of_a_one_tile_refined_file_goes_the_staged_route(exe, files):
    for name in ("130x67-L1", "130x67-L3", "200x120-L3"):
        d = decide(exe, files[name][0], window=(33, 17, 81, 57))
        assert d["route"] == (REGION, STAGED) and d["want_segs"] == (0, 1) and d["batches"] == 1 and d["refined"] > 0, name
    # (no level left: the region decoder never took it)
    assert decide(exe, files["64x64-L3"][0], window=(3, 5, 40, 41))["route"] == (STAGED, STAGED)
    # a window of a tiled file touches some tiles: theirs are the rows and the segment lists
    d = decide(exe, files["100x70-tiles-L3"][0], window=(70, 50, 100, 70))
    assert d["route"] == (STAGED, STAGED) and d["want_segs"] == (0, 1) and d["rows"] == len(G.tile_layout(files["100x70-tiles-L3"][1].tiles[3])[0])


def test_reduced_decodes_drop_rows_and_segment_lists_together(exe, files):
    for name, reduce in (("200x120-L1", 1), ("200x120-L3", 1), ("200x120-L3", 2), ("130x67-L3", 2), ("130x67-L1", 4), ("100x70-tiles-L3", 1)):
        path, c = files[name]
        d = decide(exe, path, reduce=reduce)
        levels = c.shape[4]
        kept = sum(1 for tp in c.tiles for b in G.tile_layout(tp)[0] if b.res + reduce <= levels)
        assert d["second"] == 1 and d["want_segs"] == (0, 1) and d["rows"] == kept and d["dropped"] == len(c.want["rows"]) - kept and d["dropped"] > 0, name
        assert d["refined"] > 0 or kept < 4, name
