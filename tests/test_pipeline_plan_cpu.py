"""CPU: the pipelined encode's host planning (grok_amd/csrc/encode_plan.cpp) -- ht_class_stream with the frame parity that sends
consecutive pipelined frames' K3 classes to the two side streams in turn -- through tests/c/pipeline_plan_units.cpp, built on first
use with g++ together with encode_plan.cpp and geometry.cpp: no GPU, no HIP, no libgrok_amd.so."""
import ctypes as C
import itertools
import os
import subprocess
import tempfile

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TOP, REST, ALL, TOP_SMALL, TOP_BIG, REST_SMALL, REST_BIG = range(7)          # HtRole
AFTER_LEVEL0, AFTER_LAST_LEVEL, RUN_HT = range(3)                            # HtPoint
NOT_HERE, MAIN, SIDE, SIDE2 = range(4)                                       # HtStream
_lib = None


def lib():
    global _lib
    if _lib is None:
        csrc = os.path.join(ROOT, "grok_amd", "csrc")
        out = os.path.join(tempfile.mkdtemp(prefix="pipeline_plan_units_"), "libpipeline_plan_units.so")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-D_GLIBCXX_ASSERTIONS", "-fPIC", "-shared",
                               os.path.join(HERE, "c", "pipeline_plan_units.cpp"), os.path.join(csrc, "encode_plan.cpp"),
                               os.path.join(csrc, "geometry.cpp"), "-o", out, "-Wl,--no-undefined", "-lpthread"])
        _lib = C.CDLL(out)
    return _lib


# ---- K3's classes on the two side streams in turn ---------------------------------------------------------------------------------

def stream(role, ov, pip, at, one_level, parity=None):
    if parity is None:
        return lib().pp_class_stream_default(role, int(ov), int(pip), at, int(one_level))
    return lib().pp_class_stream(role, int(ov), int(pip), at, int(one_level), parity)


def schedule():
    row = (C.c_int * 5)()
    n = lib().pp_schedule_row(0, row)
    out = []
    for i in range(n):
        lib().pp_schedule_row(i, row)
        out.append(tuple(row))
    return out


def where(role, parity, one_level=False):
    """(point, stream) of the role's launch in a pipelined overlapped encode (one level: level 0 is the last level as well, and
    AFTER_LEVEL0 answers for both points -- AFTER_LAST_LEVEL is not asked)"""
    points = (AFTER_LEVEL0, RUN_HT) if one_level else (AFTER_LEVEL0, AFTER_LAST_LEVEL, RUN_HT)
    hits = [(at, stream(role, True, True, at, one_level, parity)) for at in points]
    hits = [(at, s) for at, s in hits if s != NOT_HERE]
    assert len(hits) == 1, (role, parity, hits)
    return hits[0]


def test_parity_0_is_the_table():
    """every row of kHtSchedule, asked with parity 0 and through the five-argument call, answers with the row's stream"""
    rows = schedule()
    assert len(rows) == 13
    for role, ov, pip, at, to in rows:
        for p in ((0, 1) if pip < 0 else (pip,)):
            assert stream(role, ov, p, at, False, 0) == to
            assert stream(role, ov, p, at, False) == to
            assert stream(role, ov, p, at, False, 2) == to          # (the parity's low bit counts)


def test_parity_matters_only_for_pipelined_overlapped_encodes():
    for role, ov, pip, at, one in itertools.product(range(7), (0, 1), (0, 1), range(3), (0, 1)):
        if ov and pip:
            continue
        assert stream(role, ov, pip, at, one, 1) == stream(role, ov, pip, at, one, 0)


@pytest.mark.parametrize("one_level", [False, True])
def test_every_role_lands_on_a_side_stream_in_both_parities(one_level):
    """pipelined: the main stream carries nothing but the DWT chain; parity 1 is parity 0 with the side streams exchanged, at the
    same point of the call"""
    for role in (TOP, REST, TOP_SMALL, TOP_BIG, REST_SMALL, REST_BIG):
        at0, s0 = where(role, 0, one_level)
        at1, s1 = where(role, 1, one_level)
        assert at0 == at1
        assert {s0, s1} == {SIDE, SIDE2}
    for parity in (0, 1):               # the class of every block belongs to encodes that overlap nothing
        assert all(stream(ALL, True, True, at, one_level, parity) == NOT_HERE for at in range(3))


@pytest.mark.parametrize("parity", [0, 1])
def test_top_and_rest_never_share_a_stream_within_a_frame(parity):
    for top, rest in ((TOP, REST), (TOP_SMALL, REST_SMALL)):
        assert where(top, parity)[1] != where(rest, parity)[1]
    # consecutive frames: top(n + 1) on the stream rest(n) used, rest(n + 1) behind top(n)
    assert where(TOP, parity ^ 1)[1] == where(REST, parity)[1]
    assert where(REST, parity ^ 1)[1] == where(TOP, parity)[1]
