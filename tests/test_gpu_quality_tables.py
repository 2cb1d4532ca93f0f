"""-m gpu: the quality allocator (KQ, grok_amd/csrc/kernels_rate.hip) on tables of the tests' choosing, handed to it by
grk_amd_stage_quality_alloc.  Every table is built on the CPU (tests/qualitytables.py), the answer is predicted in exact arithmetic
(tests/qualitymodel.py, itself pinned by brute force in tests/test_quality_model_cpu.py), and the kernel has to give that answer
exactly: the multiplier bit for bit, the steps of its search, every drop byte, the bytes before and after the trim, the floor, and the
distortion as the exact value.

The kernel computes in doubles, the model in rationals.  qualitytables.conditions asserts, before a table goes to the kernel, that this
cannot matter: weights that are powers of two and E < 2^30 make every W E, every partial sum in any order and every trim delta an
exact double, and the costs the search compares are 2^-50 apart, relative, wherever it looks."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

import grok_amd as G
import gpuutil as U
import qualitymodel as QM
import qualitytables as QT
import synth
from grok_amd.capi import ERR_INVALID

pytestmark = pytest.mark.gpu
SKIP = G.DROP_SKIP


@pytest.fixture(scope="module")
def cases():
    """{name: (case, the model's answer)} -- every table built, predicted and held against the conditions once, before any launch"""
    out = {}
    for c in QT.all_cases():
        m = QT.predict(c)
        assert QT.conditions(c, m)
        out[c["name"]] = (c, m)
    return out


def result_bytes(res):
    return bytes(C.string_at(C.addressof(res), C.sizeof(res)))


def check_alloc(c, m, twice=True):
    """one launch of the allocator on the case's tables == the model's answer, exactly"""
    L, E, W, dmax, skip, D = c["L"], c["E"], c["W"], c["dmax"], c["skip"], c["budget"]
    ctx = U.ctx()
    drops, res = ctx.stage_quality_alloc(L, E, W, dmax, skip, D)
    what = "%s (D %r): lambda %r (model %s), steps %d (model %d), blocks %d, lagrange %d, distortion %r (model %r)" % (
        c["name"], D, res.lambda_, "inf" if m["lam"] is QM.INF else repr(float(m["lam"])), res.steps, m["steps"], res.block_bytes,
        res.lagrange_bytes, res.distortion, float(m["distortion"]))
    assert bool(res.feasible) == m["feasible"] and Fraction(res.floor) == m["floor"] and res.shortest_bytes == m["shortest_bytes"], what
    if m["lam"] is QM.INF:
        assert math.isinf(res.lambda_) and res.lambda_ > 0, what
    else:
        assert Fraction(res.lambda_) == m["lam"], what                      # bit for bit: the model's multiplier is a double
    assert res.steps == m["steps"], what
    want = np.array(m["drops"], np.uint8)
    assert np.array_equal(drops, want), "%s: first differing blocks %s" % (what, np.flatnonzero(drops != want)[:8])
    assert res.block_bytes == m["block_bytes"] and res.lagrange_bytes == m["lagrange"], what
    assert Fraction(res.distortion) == m["distortion"], what
    assert not m["feasible"] or Fraction(res.distortion) <= Fraction(D), what
    if twice:
        drops2, res2 = ctx.stage_quality_alloc(L, E, W, dmax, skip, D)
        assert np.array_equal(drops, drops2) and result_bytes(res) == result_bytes(res2), what
    return drops, res


@pytest.mark.parametrize("n", QT.SIZES)
def test_allocator_sizes(cases, n):
    """n blocks for n around the wave (64), the trim's chunk (256), the fill's (512), the workgroup (1024) and beyond, Dmax 1, 6 and
    12, with and without SKIP"""
    for dmax in QT.DROPS:
        for skip in ("SKIP", "no SKIP"):
            check_alloc(*cases["n %d, Dmax %d, %s" % (n, dmax, skip)], twice=dmax == 6)


def test_allocator_budgets_on_the_steps_of_the_distortion_curve(cases):
    """one table; EVERY distortion T its curve takes (169 of them) as the budget -- exactly the step, where <= must admit it --
    and one unit below; D = 0: nothing dropped; D at and above the shortest choice's distortion: lambda = +inf, steps = 0, everything
    skipped; one unit below that: a search again"""
    names = [k for k in cases if k.startswith("step budget")]
    assert len(names) >= 2 * 169
    for k, name in enumerate(names):
        check_alloc(*cases[name], twice=k % 16 == 0)
    c, m = cases["step budget 0"]
    drops, res = check_alloc(c, m)
    assert res.feasible == 1 and res.distortion == 0 and not drops.any() and res.block_bytes == int(c["L"][0].sum())
    d, unit = QT.dist_units(c)
    short = d.of(QM.RM.shortest(c["L"], 8))
    for k in (short, 2 * short):
        drops, res = check_alloc(*cases["step budget %d" % k])
        assert res.lambda_ == math.inf and res.steps == 0 and (drops == SKIP).all() and res.block_bytes == 0 == res.lagrange_bytes
    drops, res = check_alloc(*cases["step budget %d" % (short - 1)])
    assert math.isfinite(res.lambda_) and res.steps > 40 and res.block_bytes > 0


@pytest.mark.parametrize("k", QT.SCALES)
def test_allocator_multiplier_far_from_one(cases, k):
    """the weights times 2^k: the search walks about |k| - 20 halvings or doublings from 1 (the lengths carry 20 more bits than the
    errors) before the forty bisections"""
    drops, res = check_alloc(*cases["weights x 2^%d" % k])
    assert res.steps > 40 + 120 and (res.lambda_ > 1) == (k > 0)


def test_allocator_below_the_floor(cases):
    """D one unit below the floor of a table whose row 0 is not zero: feasible = 0, no search, no trim, every block at its least-E
    candidate -- the finer of two equal ones --, and no error of the call"""
    c, m = cases["below the floor"]
    drops, res = check_alloc(c, m)
    cand = np.where(drops == SKIP, 7, drops)
    assert res.feasible == 0 and res.lambda_ == 0 and res.steps == 0 and res.distortion == res.floor > c["budget"]
    assert np.array_equal(cand, np.argmin(c["E"], axis=0)) and len(set(cand.tolist())) == 8


def test_allocator_exact_tie_goes_to_the_finer_candidate(cases):
    """at the multiplier 1, the first the search looks at, block 0's candidates cost exactly 10 both: the finer one wins, the
    distortion 0 fits, 2 does not, and the multiplier is still 1 after the forty bisections"""
    drops, res = check_alloc(*cases["dyadic tie"])
    assert res.steps == 40 and res.lambda_ == 1.0 and drops.tolist() == [0, 0]


def test_allocator_non_convex_block_and_negative_delta(cases):
    """block 1 stays at its Lagrange choice because the next coarser candidate is LONGER (the trim walks one candidate at a time: a
    limit of the design, asserted so that a change of it is seen); block 2's second step gives distortion back, which block 3 takes"""
    c, m = cases["non-convex, negative delta"]
    drops, res = check_alloc(c, m)
    assert drops.tolist() == [0, 1, 2, 1] and res.distortion == 319 and res.lagrange_bytes == 1000 + 30 + 40 + 9


def test_allocator_trim_order(cases):
    """The trim across its chunks of 256 blocks: block 1 walks 13 moves from candidate 0 to SKIP, the longest chain there is; block
    255 takes its step, 256 -- the first of the next chunk -- is passed over; block 511 leaves 30, block 512 wants 100 and sees exactly
    those 30, block 513 takes them, block 514 finds nothing.  The same table reversed gives the other answer the model predicts."""
    c, m = cases["trim order"]
    drops, res = check_alloc(c, m)
    assert [int(drops[b]) for b in (0, 1, 255, 256, 511, 512, 513, 514)] == [0, SKIP, 1, 0, 1, 0, 1, 0] and res.distortion == c["budget"]
    check_alloc(*cases["trim order, reversed"])


def test_allocator_refusals_and_the_latest_calls_tables(cases):
    """NaN and negative D, max_drop 0 and 13, no block, null tables, a length of 2^31: refused before any launch.  The stage uses
    buffers of its own: the tables, the drops and the budget of an earlier grk_amd_encode_tiles_rate on the same context read back
    unchanged afterwards."""
    ctx = G.Context(0)
    try:
        p = G.TileParams.make(128, 128, 3, 8, 2)
        px = synth.g2(3, 128, 128, 8)
        nblocks = len(G.tile_layout(p)[0])
        ctx.encode_tiles_rate(p, 1, px.ctypes.data, False, 9000, 6, True)
        before = [a.copy() for a in ctx.rate_tables(nblocks, 6)]
        c, m = cases["n 65, Dmax 6, SKIP"]
        L, E, W = c["L"], c["E"], c["W"]
        for D in (float("nan"), -1.0, -0.0 - 1e-300):
            with pytest.raises(G.StageError) as e:
                ctx.stage_quality_alloc(L, E, W, 6, True, D)
            assert e.value.code == ERR_INVALID and "negative or not a number" in e.value.reason
        for dmax, rows in ((0, 2), (13, 15)):
            with pytest.raises(G.StageError) as e:
                ctx.stage_quality_alloc(np.zeros((rows, 65), np.uint32), np.zeros((rows, 65), np.uint64), W, dmax, True, 100.0)
            assert e.value.code == ERR_INVALID and e.value.reason.startswith("grk_amd_stage_quality_alloc: max_drop")
        with pytest.raises(G.StageError) as e:
            ctx.stage_quality_alloc(np.zeros((8, 0), np.uint32), np.zeros((8, 0), np.uint64), np.zeros(0), 6, True, 100.0)
        assert e.value.code == ERR_INVALID and "no block" in e.value.reason
        for tables in ((None, E, W), (L, None, W), (L, E, None)):
            with pytest.raises(G.StageError) as e:
                ctx.stage_quality_alloc(*tables, 6, True, 100.0)
            assert e.value.code == ERR_INVALID and "null pointer" in e.value.reason
        big = L.copy()
        big[3, 7] = 1 << 31
        with pytest.raises(G.StageError) as e:
            ctx.stage_quality_alloc(big, E, W, 6, True, 100.0)
        assert e.value.code == ERR_INVALID and "2^31" in e.value.reason
        drops, res = ctx.stage_quality_alloc(L, E, W, 6, True, c["budget"])
        assert np.array_equal(drops, np.array(m["drops"], np.uint8))
        after = ctx.rate_tables(nblocks, 6)
        assert all(np.array_equal(a, b) for a, b in zip(before, after)) and ctx.rate_last_budget() == 9000 and ctx.quality_last_budget() == 0.0
    finally:
        ctx.close()
