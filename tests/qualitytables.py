"""Tables of the tests' choosing for the quality allocator (KQ, grk_amd_stage_quality_alloc): the constructors -- on top of
tests/ratetables.py's --, the conditions every table has to meet before a kernel sees it, and the prediction of tests/qualitymodel.py.
tests/test_quality_model_cpu.py runs every constructor and asserts the conditions without a GPU; tests/test_gpu_quality_tables.py runs
the same cases on the kernel.

A case is ratetables' dict with `budget` the distortion D, a float.  The weights are snapped to powers of two in [1/4, 4] * wscale and
E < 2^30, so that with unit = wscale / 4 every W E is an integer count of units below 2^34, every sum of up to 3073 of them -- in ANY
order, which is what lets the kernel's tree of partial sums be compared with one exact number -- stays below 2^46, and every trim
delta is such a count too: all of them exact doubles.  D is an exact multiple of the same unit."""
from fractions import Fraction

import numpy as np

import qualitymodel as QM
import ratemodel as RM
import ratetables as RT

SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 3073)     # the issue's, and the trim's chunk of 256
DROPS = RT.DROPS
ABOVE = 1 + Fraction(1, 1 << 39)           # forty bisections of a bracket within a factor of two leave hi <= lo (1 + 2^-40) < lo * ABOVE
TRIM_CHUNK = 256                           # kFillChunk / 2


def snap(W, wscale=1.0):
    """each weight to the nearest power of two in [1/4, 4], times wscale (a power of two)"""
    k = np.clip(np.rint(np.log2(np.asarray(W, np.float64) / wscale)), -2, 2)
    return np.exp2(k) * wscale


def case(name, L, E, W, dmax, skip, budget, tie=()):
    c = RT.case(name, L, E, W, dmax, skip, 0, tie)
    assert int(c["E"].max()) < 1 << 30
    c["budget"] = float(budget)
    assert Fraction(c["budget"]) == Fraction(budget)
    return c


ncand = RT.ncand


L_SHIFT = 20


def snapped_table(n, dmax, seed, wscale=1.0):
    """ratetables.convex_table with the weights snapped and every length but SKIP's 0 times 2^20 plus 20 random bits.  With weights
    that are powers of two and small integer tables, two candidates would cost the same at 1, 2, 4 ... -- the first multipliers any
    search visits -- in many blocks of any table: W dE = lambda dL has small solutions.  A tie at a dyadic lambda needs the odd part
    of dL to divide dE, and an odd part of about 2^20 random bits does not."""
    L, E, W = RT.convex_table(n, dmax, seed, wscale)
    rng = np.random.default_rng([n, dmax, seed, 99])
    L = L * (1 << L_SHIFT) + rng.integers(0, 1 << L_SHIFT, L.shape) * (L > 0)
    assert int(L.max()) < 1 << 31 and (np.diff(L, axis=0) < 0).all()
    return L, E, snap(W, wscale)


def dist_units(c):
    """-> (qualitymodel._Dist of the case, its unit as a Fraction)"""
    d = QM._Dist(RM._Tables(c["L"], c["E"], c["W"], ncand(c)))
    return d, d.unit


def budget_between(L, E, W, nc, frac):
    """a budget `frac` of the way from 0 to the shortest choice's distortion, a whole number of units"""
    d = QM._Dist(RM._Tables(L, E, W, nc))
    return int(d.of(RM.shortest(L, nc)) * frac) * d.unit


# the seed of a size's table where seed 1 puts a multiplier the search visits on, or within 2^-50 of, a block's threshold (with
# weights that are powers of two a threshold W dE / dL is a short dyadic number whenever dL is a power of two)
SIZE_SEEDS = {}


def size_cases():
    out = []
    for k, n in enumerate(SIZES):
        for dmax in DROPS:
            for skip in (True, False):
                L, E, W = snapped_table(n, dmax, SIZE_SEEDS.get((n, dmax, skip), 1))
                frac = (0.1, 0.35, 0.7)[(k + dmax + skip) % 3]
                out.append(case("n %d, Dmax %d, %s" % (n, dmax, "SKIP" if skip else "no SKIP"), L, E, W, dmax, skip,
                                budget_between(L, E, W, dmax + 1 + skip, frac)))
    return out


STEP_TABLE = (24, 6, 8)            # n, Dmax, seed of the table whose distortion curve the budgets walk (the first seed with which EVERY
                                   # budget meets the conditions below: 1 .. 7 each put a bisection step within 2^-50 of a threshold for some budget)


def curve_distortions(L, E, W, nc):
    """every distortion (in units) the curve lambda -> dist_at(lambda) takes: at and just above every multiplier at which two
    candidates of a block cost the same, and at 0"""
    t = RM._Tables(L, E, W, nc)
    d = QM._Dist(t)
    lams = {Fraction(0)}
    for b in range(t.n):
        w = Fraction(float(W[b]))
        for i in range(nc):
            for j in range(nc):
                if t.L[i, b] > t.L[j, b] and t.E[j, b] > t.E[i, b]:
                    lams.add(w * Fraction(t.E[j, b] - t.E[i, b], t.L[i, b] - t.L[j, b]))
    lams = sorted(lams)
    seen = set()
    for k, lam in enumerate(lams):
        above = (lam + lams[k + 1]) / 2 if k + 1 < len(lams) else lam * 2 + 1
        seen.update((d.of(t.choice(lam)), d.of(t.choice(above))))
    return sorted(seen), d.unit


def step_cases():
    """one table, budgets on the steps of its distortion curve: EVERY distortion T the curve takes (169 of them): T itself, where <=
    must admit it, and one unit below; 0; the shortest choice's distortion (lambda = +inf), one unit below it and twice it"""
    n, dmax, seed = STEP_TABLE
    L, E, W = snapped_table(n, dmax, seed)
    nc = dmax + 2
    totals, unit = curve_distortions(L, E, W, nc)
    short = QM._Dist(RM._Tables(L, E, W, nc)).of(RM.shortest(L, nc))
    assert totals[0] == 0 and totals[-1] == short
    budgets = sorted(set(b for T in totals for b in (T - 1, T) if b >= 0) | {0, short, short - 1, 2 * short})
    return [case("step budget %d" % b, L, E, W, dmax, True, b * unit) for b in budgets]


SCALES = (-160, 160)


def scale_cases():
    """the weights times 2^k: the critical slope moves with them, and so do the search's steps"""
    out = []
    for k in SCALES:
        L, E, W = snapped_table(65, 6, 5, 2.0 ** k)
        out.append(case("weights x 2^%d" % k, L, E, W, 6, True, budget_between(L, E, W, 8, 0.4)))
    return out


def infeasible_case():
    """Dmax 6 with SKIP, 70 blocks, E anything between 5 and 1000 with row 0 not zero and the least E at any candidate -- at two
    candidates for some blocks, where the finer one is taken; D one unit below the floor"""
    rng = np.random.default_rng(77)
    n, rows = 70, 8
    L = rng.integers(1, 400, (rows, n))
    E = rng.integers(5, 1000, (rows, n))
    for b in range(0, n, 5):                          # the least value twice
        lo = np.argsort(E[:, b])[:2]
        E[lo[1], b] = E[lo[0], b]
    W = snap(rng.uniform(0.25, 4.0, n))
    d = QM._Dist(RM._Tables(L, E, W, rows))
    assert int(E[0].min()) > 0
    return case("below the floor", L, E, W, 6, True, (d.floor() - 1) * d.unit)


def tie_case():
    """Dmax 1, no SKIP, weights 1: at the multiplier 1 -- the first value the search looks at -- block 0's candidates cost 0 + 10 and
    8 + 2: an exact tie of exact doubles, which the finer candidate wins.  With it the distortion at 1 is 0 and fits D = 7; at 2 block
    0 has moved (8 > 7), and the forty bisections between 1 and 2 never fit: the multiplier stays 1 after 40 steps.  A kernel that gave
    the tie to the coarser candidate would see 8 at 1, halve, and end below 1 after 41."""
    L, E, W = RT._table(1, [([10, 2], [0, 8], 1.0), ([12, 2], [0, 17], 1.0)])
    return case("dyadic tie", L, E, W, 1, False, 7, tie=(0,))


def hull_case():
    """Dmax 3, no SKIP, D = 324.  Block 0 sets the multiplier (its one step costs 10020 at slope 10.02).  Block 1 is not convex:
    candidate 2 is longer AND worse than candidate 1, so the Lagrange choice 1 stays where it is -- the trim moves only while L
    strictly falls, one candidate at a time -- although candidate 3 would be shorter: a LIMIT of the design, asserted so that a change
    of it is seen.  Block 2: E FALLS from candidate 1 to 2: the trim takes the step 0 -> 1 with all 300 that are left and gets 50 back
    on 1 -> 2 (a negative delta), which block 3's step of 45 then takes."""
    blocks = [([1000, 0], [0, 10020], 1.0),
              ([50, 30, 35, 10], [0, 24, 60, 450], 1.0),
              ([40, 30, 20], [0, 300, 250], 1.0),
              ([9, 8], [0, 45], 1.0)]
    L, E, W = RT._table(3, blocks)
    return case("non-convex, negative delta", L, E, W, 3, False, 24 + 300)


ORDER_N = 600


def order_case(reverse=False):
    """Dmax 12 with SKIP, 600 blocks of which seven can move; every weight 1.  Block 0 sets the multiplier (slope 10.02); every
    other step of every block is steeper, so the Lagrange choice is candidate 0 everywhere and the trim does the rest with a slack of
    949 + 40 + 990 + 30.  Block 1 walks all 13 moves to SKIP (949).  Block 255, the last of the first chunk of 256, takes 40; block
    256 wants 3000 and is passed over.  Block 511 takes 990 and leaves 30; block 512 -- the first block of the third chunk -- wants
    100 and does not fit; block 513 takes exactly 30; block 514 wants 13 and finds nothing.  Reversed, the walk meets them the other
    way round."""
    inert = ([4], [7], 1.0)
    blocks = [inert] * ORDER_N
    blocks[0] = ([5000, 10], [0, 50000], 1.0)
    blocks[1] = ([5 * (13 - c) for c in range(14)], [60 * c + c * c for c in range(14)], 1.0)
    blocks[255] = ([5, 3], [0, 40], 1.0)
    blocks[256] = ([200, 2], [0, 3000], 1.0)
    blocks[511] = ([90, 2], [0, 990], 1.0)
    blocks[512] = ([12, 10], [0, 100], 1.0)
    blocks[513] = ([4, 3], [0, 30], 1.0)
    blocks[514] = ([2, 1], [0, 13], 1.0)
    if reverse:
        blocks = blocks[::-1]
    L, E, W = RT._table(12, blocks)
    return case("trim order%s" % (", reversed" if reverse else ""), L, E, W, 12, True, 7 * (ORDER_N - 8) + 949 + 40 + 990 + 30)


def special_cases():
    return [infeasible_case(), tie_case(), hull_case(), order_case(), order_case(True)]


def all_cases():
    return size_cases() + step_cases() + scale_cases() + special_cases()


# ---- the prediction and the conditions ------------------------------------------------------------------------------------------------
def predict(c):
    log = {}
    m = QM.allocate_quality(c["L"], c["E"], c["W"], Fraction(c["budget"]), c["dmax"], c["skip"], log)
    m["log"] = log
    return m


def conditions(c, m):
    """What has to hold before the kernel sees the table (asserted, never skipped):
    1. the sums are exact: every W E is a whole number of units, the sum of every block's LARGEST W E stays below 2^53 units (so does
       every partial sum of any choice in any order, and every difference of two of them: the trim's deltas and its remainder), D is a
       whole number of units below 2^53, and nothing leaves the double range; the float sum of the final choice equals the exact one;
    2. at every multiplier the search visits, for every block evaluated there, the best cost and the next one that is not exactly
       equal are at least ratemodel.NEAR = 2^-50 apart, relative;
    3. an exact tie between candidates with different (L, E) is met only by the blocks the case names;
    4. at the final multiplier and at (1 + 2^-39) times it, best and next-best distinct cost are at least 2^-30 apart -- for every
       block but those whose choice differs between the two (the bisection ends within 2^-40 relative BELOW such a block's threshold)."""
    L, E, W, nc = c["L"], c["E"], c["W"], ncand(c)
    d, unit = dist_units(c)
    D = Fraction(c["budget"])
    assert len(W) <= 3073 and (W > 0).all() and int(E.max()) < 1 << 30
    assert int((d.wi * d.t.E.max(axis=0)).sum()) < 1 << 53 and (D / unit).denominator == 1 and D / unit < 1 << 53
    assert float(unit) > 1e-300 and np.isfinite(float(W.max()) * float(1 << 53))
    ar = np.arange(len(W))
    cand = np.array(m["cand"])
    assert Fraction(float((W * E[cand, ar].astype(np.float64)).sum())) == m["distortion"]
    assert Fraction(float((W * E[cand, ar].astype(np.float64))[::-1].sum())) == m["distortion"]
    log = m["log"]
    assert not log.get("near"), "%s: costs within 2^-50 at (multiplier, block) %s" % (c["name"], log["near"][:4])
    tied = set(b for lam, b in log.get("ties", ()) if lam != 0)
    assert tied <= c["tie"], "%s: exact ties at blocks %s" % (c["name"], sorted(tied - c["tie"])[:8])
    lam = m["lam"]
    if m["feasible"] and lam is not QM.INF and lam > 0:
        assert np.isfinite(float(lam) * float(L.max()))
        at, g_at, t_at = RM.choice_at(L, E, W, lam, nc)
        above, g_above, t_above = RM.choice_at(L, E, W, lam * ABOVE, nc)
        moved = [b for b in range(len(at)) if at[b] != above[b]]
        assert moved, c["name"]
        for b in range(len(at)):
            if b in moved:
                continue
            assert not (t_at[b] or t_above[b]) or b in c["tie"], (c["name"], b)
            for g in (g_at[b], g_above[b]):
                assert g is None or g >= RT.GAP, "%s: block %d: costs %s apart at the final multiplier" % (c["name"], b, float(g))
        m["moved"] = moved
    return True
