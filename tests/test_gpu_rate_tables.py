"""-m gpu: the two kernels of the rate-targeted encodes (grok_amd/csrc/kernels_rate.hip) on tables and planes of the tests' choosing,
handed to them by grk_amd_stage_rate_alloc and grk_amd_stage_rate_stats.  The other rate files reach the kernels through pixels, the
transform and the block coder, with whatever tables one tile happens to produce; here every table is built on the CPU
(tests/ratetables.py), the answer is predicted in exact arithmetic (tests/ratemodel.py, itself pinned by brute force in
tests/test_rate_model_cpu.py), and the kernel has to give that answer: the multiplier, the evaluations its search made, the bytes
before and after the fill, every drop byte.

The allocator computes its costs in doubles, the model in integers.  Before a table goes to the kernel, ratetables.conditions
asserts that this cannot matter: at every multiplier the documented search visits, the best cost of every block it evaluates and the
next distinct one are at least 2^-50 apart, relative (a bound from the roundings of a double cost, derived at ratemodel.NEAR), and at
the final multiplier at least 2^-30 for every block but the one whose threshold the bisection has just converged onto -- that block's
gap is below 2^-39 by construction, in any table.  One exact tie is built on purpose, of exact doubles."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

import grok_amd as G
import gpuutil as U
import ratemodel as RM
import rateplanes as RP
import ratetables as RT
import synth
from grok_amd.capi import ERR_INVALID

pytestmark = pytest.mark.gpu
SKIP = G.DROP_SKIP


# ---- the allocator ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cases():
    """{name: (case, the model's answer)} -- every table built, predicted and held against the conditions once, before any launch"""
    out = {}
    for c in RT.all_cases():
        m = RT.predict(c)
        assert RT.conditions(c, m)
        out[c["name"]] = (c, m)
    return out


def result_bytes(res):
    return bytes(C.string_at(C.addressof(res), C.sizeof(res)))


def check_alloc(c, m, twice=True):
    """one launch of the allocator on the case's tables == the model's answer (the numbers are those of the issue's list)"""
    L, E, W, dmax, skip, budget = c["L"], c["E"], c["W"], c["dmax"], c["skip"], c["budget"]
    n, nc = len(W), RT.ncand(c)
    ctx = U.ctx()
    drops, res = ctx.stage_rate_alloc(L, E, W, dmax, skip, budget)
    lam = Fraction(res.lambda_)
    what = "%s (budget %d): lambda %r (model %r), steps %d (model %d), blocks %d, lagrange %d" % (
        c["name"], budget, res.lambda_, float(m["lam"]), res.steps, m["steps"], res.block_bytes, res.lagrange_bytes)
    # 1. feasible == (least(L) <= budget), least_bytes == least(L)
    lst = RM.least(L, nc)
    assert bool(res.feasible) == (lst <= budget) == m["feasible"] and res.least_bytes == lst, what
    # 2. the multiplier is the right one: the model's total at it fits, the total a hair below it does not; 0 exactly when the
    #    finest choice fits
    finest = int(L[0].astype(np.int64).sum())
    if m["feasible"] and m["bracketed"]:
        at = RM.choice_at(L, E, W, lam, nc)[0]
        assert RM.total_at(L, at) <= budget, what
        if lam > 0:
            assert RM.total_at(L, RM.choice_at(L, E, W, lam * RT.BELOW, nc)[0]) > budget, what
        assert (lam == 0) == (finest <= budget), what
        start = at
    else:
        # not feasible (lambda stays 0), or 200 doublings found no multiplier that fits (lambda is the last one tried)
        assert lam == m["lam"] and (not m["feasible"] or lam == Fraction(2) ** RM.BRACKET_LIMIT), what
        start = RM.shortest(L, nc)
    # 3. lagrange_bytes == the model's total of the choice the fill starts from
    assert res.lagrange_bytes == RM.total_at(L, start) == m["lagrange"], what
    # 4. the drop bytes == the fill of that choice, byte for byte; candidate Dmax + 1 is 0xFF
    cand = RM.fill(L, E, start, budget) if m["feasible"] else start
    want = np.array([k if k <= dmax else SKIP for k in cand], np.uint8)
    assert np.array_equal(drops, want), "%s: first differing blocks %s" % (what, np.flatnonzero(drops != want)[:8])
    assert cand == m["cand"] and lam == m["lam"], what
    # 5. block_bytes == the bytes of those drops
    assert res.block_bytes == RM.total_at(L, cand), what
    assert not m["feasible"] or res.block_bytes <= budget, what
    # 6. steps == the evaluations the documented search makes
    assert res.steps == m["steps"], what                     # (ratemodel.bracket_steps: the steps of ratemodel.search)
    # 7. distortion == the exact sum of W E of those drops, to a relative (ceil(n / 1024) + 12) 2^-53.  Every term is non-negative, so
    #    relative errors of partial sums never grow by cancellation and simply add up, to first order: a thread adds up to
    #    ceil(n / 1024) terms, each a product rounded once and added with one more rounding (fused: one rounding for both), the first
    #    of them to an exact 0 -- at most ceil(n / 1024) roundings on the way of any one term through the thread's sum, counting its
    #    product's; the tree over 1024 threads adds ten more, one per level; E and W are exact (E < 2^53).  That is ceil(n / 1024) + 10
    #    factors (1 + d), |d| <= 2^-53, on each term; 12 in the bound leave room for the second-order terms.
    exact = sum(Fraction(float(W[b])) * int(E[k][b]) for b, k in enumerate(cand))
    assert exact == m["distortion"]
    tol = (math.ceil(n / 1024) + 12) * Fraction(1, 1 << 53)
    assert abs(Fraction(res.distortion) - exact) <= tol * exact, "%s: distortion %r, exact %r" % (what, res.distortion, float(exact))
    # 8. a second call: the same bytes and the same result, bit for bit
    if twice:
        drops2, res2 = ctx.stage_rate_alloc(L, E, W, dmax, skip, budget)
        assert np.array_equal(drops, drops2) and result_bytes(res) == result_bytes(res2), what
    return drops, res


@pytest.mark.parametrize("n", RT.SIZES)
def test_allocator_sizes(cases, n):
    """n blocks for n around the wave (64), the fill's chunk (512), the workgroup (1024) and beyond -- threads that stride through the
    tables, chunks with a remainder --, Dmax 1, 6 and 12, with and without SKIP; convex curves with slopes from a fixed seed"""
    for dmax in RT.DROPS:
        for skip in ("SKIP", "no SKIP"):
            check_alloc(*cases["n %d, Dmax %d, %s" % (n, dmax, skip)])


def test_allocator_budgets_on_the_steps_of_the_rate_curve(cases):
    """one table; every total T its rate curve takes (at most 64 of them) as the budget, and T - 1 and T + 1; the finest total (the
    multiplier is 0) and one below; 0 with SKIP: every block skipped, feasible; without SKIP the shortest choice's bytes and one
    below, which is not feasible and reports the shortest choice"""
    names = [k for k in cases if k.startswith("step budget") or k.startswith("no SKIP, budget")]
    assert len(names) > 100
    for k, name in enumerate(names):
        check_alloc(*cases[name], twice=k % 16 == 0)
    drops, res = check_alloc(*cases["step budget 0"])
    assert res.feasible == 1 and res.block_bytes == 0 and (drops == SKIP).all()
    drops, res = check_alloc(*cases["no SKIP, budget least-1"])
    assert res.feasible == 0 and res.lambda_ == 0 and res.steps == 0 and (drops == 6).all() and res.block_bytes == res.least_bytes > cases["no SKIP, budget least-1"][0]["budget"]


@pytest.mark.parametrize("k", RT.SCALES)
def test_allocator_multiplier_far_from_one(cases, k):
    """the weights times 2^k: the critical slope moves with them and the search's steps follow -- about |k| halvings or doublings
    from 1 before the forty bisections.  k = 230: the search gives up after 200 doublings; the result is the shortest choice followed
    by the fill, within the budget"""
    c, m = cases["weights x 2^%d" % k]
    drops, res = check_alloc(c, m)
    if k == 230:
        assert res.steps == 240 and res.lambda_ == 2.0 ** 200 and res.feasible == 1 and res.lagrange_bytes == res.least_bytes == 0
        assert 0 < res.block_bytes <= c["budget"]
    else:
        assert abs((res.steps - 40) - abs(k)) < 25 and (res.lambda_ > 1) == (k > 0)


def test_allocator_plateaus_and_an_all_zero_block(cases):
    """Rows c >= top equal in L and E, what the coder's clamp produces: the finest of them is chosen.  An all-zero block (E 0 in every
    row, bytes only at c = 0) sits at candidate 1 as soon as the multiplier is positive, and the fill never moves it.
    A plateau of E in the middle of a chain (E[1] == E[2] of block 3): the fill stops at candidate 2 although candidates 1 and 0
    would fit what is left and candidate 0 has the smaller error.  That is the documented behaviour -- a block moves only while E
    strictly falls, one candidate at a time -- and a LIMIT of the design, not a goal: asserted so that a change of it is seen."""
    c, m = cases["plateaus"]
    drops, res = check_alloc(c, m)
    assert drops.tolist() == [1, 0, 1, 2, 0] and res.lambda_ > 0
    left = c["budget"] - res.block_bytes
    assert left >= int(c["L"][0][3]) - int(c["L"][2][3]) and int(c["E"][0][3]) < int(c["E"][2][3])


def test_allocator_exact_tie_goes_to_the_finer_candidate(cases):
    """the one tie of this file: at the multiplier 1, the first the search looks at, block 0's candidates cost exactly 10 both (weights
    1: the costs are exact doubles).  The finer one wins, the total at 1 does not fit, the search walks up: one doubling, forty
    bisections, and the multiplier ends one step of 2^-40 above 1"""
    c, m = cases["dyadic tie"]
    drops, res = check_alloc(c, m)
    assert res.steps == 41 and res.lambda_ == 1.0 + 2.0 ** -40 and drops.tolist() == [1, 0]


def test_allocator_non_convex_block(cases):
    """a candidate above the hull of its neighbours is never the Lagrange choice and is reached by the fill; the step behind it is
    SHORTER than it (a negative delta) and gives bytes back to the next block"""
    c, m = cases["non-convex"]
    L, E, W = c["L"], c["E"], c["W"]
    for lam in [Fraction(k, 16) for k in range(0, 400)]:
        assert RM.choice_at(L, E, W, lam, 4)[0][1] != 2
    drops, res = check_alloc(c, m)
    assert drops.tolist() == [1, 1, 0, 1] and res.block_bytes == c["budget"] and res.lagrange_bytes == c["budget"] - 25


def test_allocator_fill_order(cases):
    """The fill across its chunks of 512 blocks: block 511 takes all but 3 bytes of what is left, block 512 -- the first of the next
    chunk -- wants 10 and sees exactly those 3, block 513 takes them, block 514 finds nothing: a block that does not fit between two
    that do.  Block 1 walks from SKIP to candidate 0 at Dmax 12: 13 moves, the longest chain there is.  The same table reversed
    gives the other answer the model predicts."""
    c, m = cases["fill order"]
    drops, res = check_alloc(c, m)
    assert [int(drops[b]) for b in (0, 1, 511, 512, 513, 514)] == [1, 0, 0, 1, 0, 1] and res.block_bytes == c["budget"]
    c, m = cases["fill order, reversed"]
    drops, res = check_alloc(c, m)
    n = RT.ORDER_N - 1
    assert [int(drops[n - b]) for b in (0, 1, 511, 512, 513, 514)] == [1, 3, 0, 0, 0, 0] and res.block_bytes == c["budget"] - 4


def test_allocator_refusals_and_the_latest_calls_tables(cases):
    """max_drop 0 and 13, no block, null tables: refused before any launch.  The stage uses buffers of its own: the tables, the drops
    and the budget of an earlier grk_amd_encode_tiles_rate on the same context read back unchanged afterwards."""
    ctx = G.Context(0)
    try:
        p = G.TileParams.make(128, 128, 3, 8, 2)
        px = synth.g2(3, 128, 128, 8)
        nblocks = len(G.tile_layout(p)[0])
        ctx.encode_tiles_rate(p, 1, px.ctypes.data, False, 9000, 6, True)
        before = [a.copy() for a in ctx.rate_tables(nblocks, 6)]
        budget = ctx.rate_last_budget()
        c, m = cases["n 65, Dmax 6, SKIP"]
        L, E, W = c["L"], c["E"], c["W"]
        for dmax, rows in ((0, 2), (13, 15)):
            with pytest.raises(G.StageError) as e:
                ctx.stage_rate_alloc(np.zeros((rows, 65), np.uint32), np.zeros((rows, 65), np.uint64), W, dmax, True, 100)
            assert e.value.code == ERR_INVALID and e.value.reason.startswith("grk_amd_stage_rate_alloc: max_drop")
        with pytest.raises(G.StageError) as e:
            ctx.stage_rate_alloc(np.zeros((8, 0), np.uint32), np.zeros((8, 0), np.uint64), np.zeros(0), 6, True, 100)
        assert e.value.code == ERR_INVALID and "no block" in e.value.reason
        for tables in ((None, E, W), (L, None, W), (L, E, None)):
            with pytest.raises(G.StageError) as e:
                ctx.stage_rate_alloc(*tables, 6, True, 100)
            assert e.value.code == ERR_INVALID and "null pointer" in e.value.reason
        big = L.copy()
        big[3, 7] = 1 << 31
        with pytest.raises(G.StageError) as e:
            ctx.stage_rate_alloc(big, E, W, 6, True, 100)
        assert e.value.code == ERR_INVALID and "2^31" in e.value.reason
        drops, res = ctx.stage_rate_alloc(L, E, W, 6, True, c["budget"])
        assert np.array_equal(drops, np.array(m["drops"], np.uint8))
        after = ctx.rate_tables(nblocks, 6)
        assert all(np.array_equal(a, b) for a, b in zip(before, after)) and ctx.rate_last_budget() == budget == 9000
    finally:
        ctx.close()


# ---- the statistics ---------------------------------------------------------------------------------------------------------------------
def edge_values(kmax, dmax):
    """every value of {2^c - 1, 2^c, 2^c + 1 : c <= dmax} that fits kmax bits"""
    return sorted(set(v for c in range(dmax + 1) for v in ((1 << c) - 1, 1 << c, (1 << c) + 1) if v < 1 << kmax))


def content(dmax, irrev):
    """block i's magnitudes, chosen by its kmax: all 2^kmax - 1; all zero; the values on and beside every power of two up to 2^dmax,
    where q >> c changes; uniform; and for 9/7 values a factor 1.5 beyond the quantiser's clamp"""
    def all_max(rng, bh, bw, b):
        return np.full((bh, bw), (1 << b.kmax) - 1)

    def zeros(rng, bh, bw, b):
        return np.zeros((bh, bw), np.int64)

    def edges(rng, bh, bw, b):
        return rng.choice(edge_values(b.kmax, dmax), (bh, bw))

    def uniform(rng, bh, bw, b):
        return rng.integers(0, 1 << b.kmax, (bh, bw))

    def beyond(rng, bh, bw, b):
        return np.full((bh, bw), max(1, 3 * (1 << b.kmax) // 2)) if irrev else rng.choice(edge_values(b.kmax, dmax), (bh, bw))

    modes = [all_max, edges, zeros, uniform, beyond, edges, uniform]
    return lambda i: modes[i % len(modes)]


def expected_errors(p, blocks, planes, dmax, tile=0):
    """-> E [dmax + 2][blocks] of one tile's planes (host, (components, H, W)) by ratemodel"""
    want = np.zeros((dmax + 2, len(blocks)), np.uint64)
    for i, b in enumerate(blocks):
        sub = planes[b.comp, b.py:b.py + b.y1 - b.y0, b.px:b.px + b.x1 - b.x0]
        want[:, i] = RM.errors(RM.quantised(sub, b.kmax, b.stepsize, bool(p.irreversible)), b.kmax, dmax)
    return want


def check_stats(form, geom, dmax, seed):
    prec, irrev, h16 = RP.FORMS[form] if isinstance(form, str) else form
    p, blocks, dev, h16, _, planes = RP.planes_case(form, geom, seed, content(dmax, irrev), signmag=False)
    got = U.ctx().stage_rate_stats(p, 1, dev.data_ptr(), h16, dmax)
    want = expected_errors(p, blocks, planes, dmax)
    bad = np.argwhere(got != want)
    assert not len(bad), "%s, %s, Dmax %d: (row, block) %s of %d blocks" % (form, geom, dmax, bad[:8].tolist(), len(blocks))
    assert want[dmax + 1].any() and not want[0].any()
    return p, blocks, want


@pytest.mark.parametrize("geom", list(RP.STATS_GEOMS))
@pytest.mark.parametrize("form", list(RP.FORMS))
def test_statistics_equal_the_formula_on_chosen_planes(form, geom):
    """E == ratemodel.errors of ratemodel.quantised of the planes, exactly, every row -- the three forms of the kernel (int16 planes,
    int32 reversible, int32 irreversible with the quantiser and its clamp inside) on code-blocks of 64 (a wave wide), 32 and 4, on
    the ragged last column and row of 77 x 53, and on 200 x 70 with a 64-wide block beside a ragged one"""
    p, blocks, want = check_stats(form, geom, RT.DROPS[1], [len(form), len(geom), 3])
    widths = set(b.x1 - b.x0 for b in blocks)
    if geom == "200x70 cblk 64":
        assert 64 in widths and any(w % 64 for w in widths)
    if geom == "ragged 77x53":
        assert any(w < 32 and w % 4 for w in widths)


CLAMP_FORMS = [(prec, irrev, h16) for prec in (8, 1, 2) for irrev, h16 in ((False, True), (False, False), (True, False))]


@pytest.mark.parametrize("form", CLAMP_FORMS, ids=["%d bits, %s" % (f[0], "int16" if f[2] else "9/7" if f[1] else "int32 5/3") for f in CLAMP_FORMS])
def test_statistics_with_candidates_beyond_the_coders_clamp(form):
    """Dmax 12 on 8-, 1- and 2-bit content: most bands have Kmax - 1 < 12 and rows c >= Kmax - 1 describe the block as coded, c
    clamped to Kmax - 1 -- in every form of the kernel, the int32 reversible one on 8-bit content (GRK_AMD_PLANES16=0) among them"""
    p, blocks, want = check_stats(form, "cblk 32", 12, [form[0], int(form[1]), int(form[2]), 5])
    top = np.array([max(b.kmax - 1, 0) for b in blocks])
    assert top.min() < 12 and (top < 12).sum() * 2 > len(top)
    ar = np.arange(len(top))
    for c in range(1, 13):
        assert np.array_equal(want[c], want[np.minimum(c, top), ar])


@pytest.mark.parametrize("form", list(RP.FORMS))
def test_statistics_of_three_tiles_through_a_map(form):
    """three tiles with different planes written through first rows [5, 5 + bpt + 3, 2 (5 + bpt + 3)] into rows of n entries, n larger
    than needed: the columns the map names hold the model's values, every other entry still holds the sentinel it was given"""
    dmax = 6
    prec, irrev, h16 = RP.FORMS[form]
    tiles = [RP.planes_case(form, "ragged 77x53", [7, t], content(dmax, irrev), signmag=False) for t in range(3)]
    p, blocks = tiles[0][0], tiles[0][1]
    bpt = len(blocks)
    stride, elems = G.lib().grk_amd_plane_stride(p), G.lib().grk_amd_plane_elems(p)
    H, W = p.tile_h, p.tile_w
    assert elems >= H * stride
    buf = np.zeros(3 * elems, np.int16 if h16 else np.int32)
    for t in range(3):
        host = tiles[t][5] if not irrev else tiles[t][5].view(np.int32)
        buf[t * elems:t * elems + H * stride].reshape(H, stride)[:, :W] = host[0]
    dev = U.to_dev(buf)
    first = [5, 5 + bpt + 3, 2 * (5 + bpt + 3)]
    n = first[2] + bpt + 9
    sentinel = np.uint64(0xA5A5A5A5A5A5A5A5)
    got = U.ctx().stage_rate_stats(p, 3, dev.data_ptr(), h16, dmax, first, n, np.full((dmax + 2, n), sentinel))
    want = np.full((dmax + 2, n), sentinel)
    for t in range(3):
        want[:, first[t]:first[t] + bpt] = expected_errors(p, blocks, tiles[t][5], dmax)
    assert not np.array_equal(tiles[0][5], tiles[1][5]) and np.array_equal(got, want), np.argwhere(got != want)[:8].tolist()
    assert (got[:, :5] == sentinel).all() and (got[:, first[1] + bpt:first[2]] == sentinel).all() and (got[:, -9:] == sentinel).all()
    # without a map the same three tiles fill a table of their own, column i = block i of the call
    plain = U.ctx().stage_rate_stats(p, 3, dev.data_ptr(), h16, dmax)
    assert np.array_equal(plain, np.concatenate([want[:, f:f + bpt] for f in first], axis=1))


def test_statistics_refusals():
    """max_drop 0 and 13, a first row whose tile would end beyond n, int16 planes with 9/7: refused before any launch"""
    ctx = U.ctx()
    p, blocks, dev, h16, _, planes = RP.planes_case("int16", "cblk 32", 1, content(6, False), signmag=False)
    bpt = len(blocks)
    for dmax in (0, 13):
        with pytest.raises(G.StageError) as e:
            ctx.stage_rate_stats(p, 1, dev.data_ptr(), True, dmax)
        assert e.value.code == ERR_INVALID and "max_drop" in e.value.reason
    for first, n in (([1], bpt), ([bpt + 1], bpt + 1), ([0], bpt - 1)):
        with pytest.raises(G.StageError) as e:
            ctx.stage_rate_stats(p, 1, dev.data_ptr(), True, 6, first, n, np.zeros((8, n), np.uint64))
        assert e.value.code == ERR_INVALID and "end beyond" in e.value.reason
    assert ctx.stage_rate_stats(p, 1, dev.data_ptr(), True, 6, [1], bpt + 1, np.zeros((8, bpt + 1), np.uint64)).shape == (8, bpt + 1)
    p97 = G.TileParams.make(128, 128, 1, 8, 2, irreversible=True, mct=False, cblk=(5, 5))
    with pytest.raises(G.StageError) as e:
        ctx.stage_rate_stats(p97, 1, dev.data_ptr(), True, 6)
    assert e.value.code == ERR_INVALID and "int16" in e.value.reason


# ---- the staged kernels are the ones production runs ----------------------------------------------------------------------------------
def test_a_rate_targeted_encode_runs_the_staged_kernels():
    """grk_amd_encode_tiles_rate of a 12-bit reversible 128 x 128 tile: its E (grk_amd_rate_tables) equals the model's from the planes
    the encode left -- rate_stats_kernel<int32_t, false> through production --, and its drop bytes equal grk_amd_stage_rate_alloc of
    its own L, E, W at grk_amd_rate_last_budget"""
    ctx = U.ctx()
    dmax = 6
    p = G.TileParams.make(128, 128, 3, 12, 2, cblk=(5, 5))
    px = synth.g2(3, 128, 128, 12)
    blocks, _ = G.tile_layout(p)
    n = len(blocks)
    plain, _ = ctx.encode_host(p, px)
    budget = int(plain["length"].sum()) // 4
    table, tot, res = ctx.encode_tiles_rate(p, 1, px.ctypes.data, False, budget, dmax, True)
    L, E, W, drop = ctx.rate_tables(n, dmax)
    assert ctx.plane_sample_bytes(p)[0] == 4 and ctx.rate_last_budget() == budget
    stride, elems = G.lib().grk_amd_plane_stride(p), G.lib().grk_amd_plane_elems(p)
    raw = U.from_dev_ptr(ctx.plane_device_ptr(1), 3 * elems * 4)
    planes = raw.view(np.int32).reshape(3, -1)[:, :128 * stride].reshape(3, 128, stride)[:, :, :128]
    assert np.array_equal(E, expected_errors(p, blocks, planes, dmax))
    drops, sres = ctx.stage_rate_alloc(L, E, W, dmax, True, ctx.rate_last_budget())
    assert np.array_equal(drops, drop)
    assert (sres.block_bytes, sres.lagrange_bytes, sres.distortion, sres.lambda_) == (res.block_bytes, res.lagrange_bytes, res.distortion, res.lambda_)
    assert sres.feasible == 1 and 0 < sres.block_bytes <= budget and len(set(drop.tolist())) > 2
