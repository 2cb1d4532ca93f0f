"""Tables of the tests' choosing for the rate allocator (KR2, grk_amd_stage_rate_alloc): the constructors, the conditions every table
has to meet before a kernel sees it, and the prediction of tests/ratemodel.py.  tests/test_rate_model_cpu.py runs every constructor
and asserts the conditions without a GPU; tests/test_gpu_rate_tables.py runs the same cases on the kernel.

A case is a dict: name, L uint32 [dmax + 2][n], E uint64 [dmax + 2][n], W float64 [n], dmax, skip, budget, tie (the blocks that may
meet an exact tie between different candidates: a table says so on purpose)."""
from fractions import Fraction

import numpy as np

import ratemodel as RM

SIZES = (1, 2, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 1537, 3073)
DROPS = (1, 6, 12)
GAP = Fraction(1, 1 << 30)                 # best and next-best distinct cost at the final multiplier: at least this far apart, relative
BELOW = 1 - Fraction(1, 1 << 39)           # forty bisections of a bracket within a factor of two leave lo >= hi / (1 + 2^-40) > hi * BELOW


def case(name, L, E, W, dmax, skip, budget, tie=()):
    L, E, W = np.ascontiguousarray(L, np.uint32), np.ascontiguousarray(E, np.uint64), np.ascontiguousarray(W, np.float64)
    assert L.shape == E.shape == (dmax + 2, len(W)) and int(L.max()) < 1 << 31 and int(E.max()) < 1 << 53
    return dict(name=name, L=L, E=E, W=W, dmax=dmax, skip=bool(skip), budget=int(budget), tie=frozenset(tie))


def ncand(c):
    return c["dmax"] + 1 + (1 if c["skip"] else 0)


# ---- constructors ------------------------------------------------------------------------------------------------------------------
def convex_table(n, dmax, seed, wscale=1.0):
    """Per block a convex curve: towards coarser candidates L falls to 0 at SKIP, E rises, and the slope dE / dL of each step is at
    least 1.6 times the step before: every candidate is on the hull.  Weights in [1/4, 4) times wscale (a power of two: exact)."""
    rng = np.random.default_rng([n, dmax, seed])
    rows = dmax + 2
    dl = rng.integers(5, 60, (rows, n))                      # [c]: bytes saved by the step c - 1 -> c
    slope = np.ones((rows, n))
    slope[1] = rng.uniform(1.0, 8.0, n)
    for c in range(2, rows):
        slope[c] = slope[c - 1] * rng.uniform(1.6, 3.0, n)
    de = np.maximum(np.rint(slope * dl).astype(np.int64), 1)
    L = np.zeros((rows, n), np.int64)
    E = np.zeros((rows, n), np.int64)
    for c in range(rows - 1, 0, -1):
        L[c - 1] = L[c] + dl[c]
    for c in range(1, rows):
        E[c] = E[c - 1] + de[c]
    W = rng.uniform(0.25, 4.0, n) * wscale
    return L, E, W


def budget_between(L, nc, frac):
    """a budget `frac` of the way from the shortest choice's bytes to the finest's"""
    lo, hi = RM.least(L, nc), int(L[0].astype(np.int64).sum())
    return lo + int((hi - lo) * frac)


# the seed of a size's table where seed 1 puts a bisection step within 2^-50 of a block's threshold (conditions, 2.)
SIZE_SEEDS = {(65, 6): 2}


def size_cases():
    out = []
    for k, n in enumerate(SIZES):
        for dmax in DROPS:
            for skip in (True, False):
                L, E, W = convex_table(n, dmax, SIZE_SEEDS.get((n, dmax), 1))
                frac = (0.15, 0.45, 0.8)[(k + dmax + skip) % 3]
                out.append(case("n %d, Dmax %d, %s" % (n, dmax, "SKIP" if skip else "no SKIP"), L, E, W, dmax, skip,
                                budget_between(L, dmax + 1 + skip, frac)))
    return out


STEP_TABLE = (24, 6, 6)            # n, Dmax, seed of the table whose rate curve the budgets walk (a seed with which every budget meets
                                   # the conditions below; 3, 4 and 5 each put a bisection step within 2^-50 of a threshold for some budget)


def curve_totals(L, E, W, nc):
    """every total the rate curve takes: the totals at and just above every multiplier at which two candidates of a block cost the
    same, and at 0"""
    t = RM._Tables(L, E, W, nc)
    lams = {Fraction(0)}
    for b in range(t.n):
        w = Fraction(float(W[b]))
        for i in range(nc):
            for j in range(nc):
                if t.L[i, b] > t.L[j, b] and t.E[j, b] > t.E[i, b]:
                    lams.add(w * Fraction(t.E[j, b] - t.E[i, b], t.L[i, b] - t.L[j, b]))
    lams = sorted(lams)
    totals = set()
    for k, lam in enumerate(lams):
        above = (lam + lams[k + 1]) / 2 if k + 1 < len(lams) else lam * 2 + 1
        totals.update((t.bytes_of(t.choice(lam)), t.bytes_of(t.choice(above))))
    return sorted(totals)


def step_cases():
    """one table, budgets on the steps of its rate curve: every total T the curve takes (at most 64 of them, evenly spread), T - 1 and
    T + 1; the finest total and one below; least and least - 1 (not feasible); 0 with SKIP (every block skipped)"""
    n, dmax, seed = STEP_TABLE
    L, E, W = convex_table(n, dmax, seed)
    nc = dmax + 2
    totals = curve_totals(L, E, W, nc)
    if len(totals) > 64:
        totals = [totals[int(round(i * (len(totals) - 1) / 63.0))] for i in range(64)]
    finest, lst = int(L[0].sum()), RM.least(L, nc)
    assert lst == 0 and finest == max(totals) and 0 in totals
    budgets = sorted(set(b for T in totals for b in (T - 1, T, T + 1) if b >= 0) | {finest, finest - 1, 0})
    out = [case("step budget %d" % b, L, E, W, dmax, True, b) for b in budgets]
    # without SKIP the shortest choice takes bytes: least and least - 1
    lst = RM.least(L, dmax + 1)
    assert lst > 0
    out += [case("no SKIP, budget least%+d" % d, L, E, W, dmax, False, lst + d) for d in (0, -1, 1)]
    return out


SCALES = (-160, -40, 40, 160, 230)


def scale_cases():
    """the weights times 2^k: the critical slope moves with them, and so do the search's steps; at 2^230 the search gives up after
    200 doublings"""
    out = []
    for k in SCALES:
        L, E, W = convex_table(65, 6, 5, 2.0 ** k)
        out.append(case("weights x 2^%d" % k, L, E, W, 6, True, budget_between(L, 8, 0.4)))
    return out


def _rows(dmax, first, rest=None):
    """a block's column of dmax + 2 entries: `first`, then its last entry (or `rest`) repeated"""
    first = list(first)
    return first + [first[-1] if rest is None else rest] * (dmax + 2 - len(first))


def _table(dmax, blocks):
    """blocks: [(L column, E column, W)] -> L, E, W"""
    L = np.array([_rows(dmax, b[0]) for b in blocks], np.int64).T
    E = np.array([_rows(dmax, b[1]) for b in blocks], np.int64).T
    return L, E, np.array([b[2] for b in blocks], np.float64)


def plateau_case():
    """Dmax 6 with SKIP; weights 1 for block 0 and 1.1 behind it (no multiplier the search visits is a block's threshold).  Block 0 sets the multiplier (its one step costs 1000 bytes at slope 10.02).  Block 1: rows c >= 3 equal in L
    and E, what the coder's clamp produces.  Block 2: all zero -- E 0 everywhere, 3 bytes at c = 0, none elsewhere.  Block 3: E[1] ==
    E[2], a plateau in the middle of its chain.  Block 4: an ordinary block behind them."""
    blocks = [([1000, 0], [0, 10020], 1.0),
              ([50, 40, 30, 20], [0, 10, 40, 130], 1.1),
              ([3, 0], [0, 0], 1.1),
              ([60, 50, 45, 20], [0, 5, 5, 30], 1.1),
              ([90, 60, 40, 25, 0], [0, 100, 340, 900, 5000], 1.1)]
    L, E, W = _table(6, blocks)
    # just above 10.02: 0 + 20 + 0 + 20 + 60 bytes; 900 more leave block 0's step out of reach and everything else within it
    return case("plateaus", L, E, W, 6, True, 100 + 900)


def tie_case():
    """Dmax 1, no SKIP, weights 1: at the multiplier 1 -- the first value the search looks at -- block 0's candidates cost 0 + 10 and
    8 + 2: an exact tie of exact doubles, which the finer candidate wins.  With it the total at 1 is 22 and does not fit 14, the search
    walks up, and ends just above 1 with block 0 at the coarser candidate; a kernel that gave the tie to the coarser candidate would
    find 14 bytes fitting at 1, walk down, and end at 1."""
    L, E, W = _table(1, [([10, 2], [0, 8], 1.0), ([12, 2], [0, 17], 1.0)])
    return case("dyadic tie", L, E, W, 1, False, 14, tie=(0,))


def nonconvex_case():
    """Dmax 3, no SKIP.  Block 0 sets the multiplier.  Block 1: candidate 2 lies above the hull of its neighbours (longer AND worse
    than candidate 1): never the Lagrange choice, reached by the fill on its way from 3 to 1 -- and the step 2 -> 1 is 5 bytes
    SHORTER, which block 2's 5-byte step then takes."""
    blocks = [([1000, 0], [0, 10020], 1.0),
              ([50, 30, 35, 10], [0, 20, 60, 200], 1.1),
              ([25, 20], [0, 30], 1.1),
              ([9, 8], [0, 4], 1.1)]
    L, E, W = _table(3, blocks)
    # just above 10.02: 0 + 10 + 20 + 8; 25 more: block 1 walks 3 -> 2 (25 bytes, nothing left) -> 1 (5 back), block 2 takes the 5
    return case("non-convex", L, E, W, 3, False, 38 + 25)


ORDER_N, ORDER_SLACK = 600, 1000


def order_case(reverse=False):
    """Dmax 12 with SKIP, 600 blocks of which six can move.  Block 0 sets the multiplier: its step costs 4990 bytes, the budget leaves
    1000.  Block 1 sits at SKIP and walks all 13 moves to candidate 0, 5 bytes each.  Block 511, the last of the first chunk of
    512, takes all but 3 of what is left; block 512, the first of the next chunk, would take 10 and does not fit; block 513 takes
    exactly 3; block 514 would take 1 and finds nothing.  Reversed, the walk meets them the other way round."""
    inert = ([4], [7], 1.1)
    blocks = [inert] * ORDER_N
    blocks[0] = ([5000, 10], [0, 50000], 1.0)
    blocks[1] = ([5 * (13 - c) for c in range(14)], [c * (c + 1) for c in range(14)], 1.1)
    blocks[511] = ([ORDER_SLACK - 65 - 3 + 2, 2], [0, 900], 1.1)
    blocks[512] = ([12, 2], [0, 11], 1.1)
    blocks[513] = ([4, 1], [0, 5], 1.1)
    blocks[514] = ([2, 1], [0, 3], 1.1)
    if reverse:
        blocks = blocks[::-1]
    L, E, W = _table(12, blocks)
    start = 10 + 0 + 2 + 2 + 1 + 1 + 4 * (ORDER_N - 6)
    return case("fill order%s" % (", reversed" if reverse else ""), L, E, W, 12, True, start + ORDER_SLACK)


def special_cases():
    return [plateau_case(), tie_case(), nonconvex_case(), order_case(), order_case(True)]


def all_cases():
    return size_cases() + step_cases() + scale_cases() + special_cases()


# ---- the prediction and the conditions ------------------------------------------------------------------------------------------------
def predict(c):
    """RM.allocate of the case with the search's log -> the model's answer; the conditions are asserted on it by `conditions`"""
    log = {}
    m = RM.allocate(c["L"], c["E"], c["W"], c["budget"], c["dmax"], c["skip"], log)
    m["log"] = log
    return m


def conditions(c, m):
    """What has to hold before the kernel sees the table (asserted, never skipped):
    1. no total of L reaches 2^63 and no product W E leaves the double range;
    2. at every multiplier the search visits, for every block evaluated there (ratemodel.search: every block at the bracket's ends,
       and in between those whose choice is not yet settled), the best cost and the next one that is not exactly equal are at least
       ratemodel.NEAR = 2^-50 apart, relative: a computation in doubles judges them as the exact one does, so the kernel walks the
       model's path to the model's multiplier;
    3. an exact tie between candidates with different (L, E) is met only by the blocks the case names, with costs that are exact
       doubles;
    4. at the final multiplier and at (1 - 2^-39) times it, best and next-best distinct cost are at least 2^-30 apart -- for every
       block but those whose choice differs between the two: the bisection ends within 2^-40 relative ABOVE the multiplier at which
       such a block's two candidates cost the same, so its gap there is below 2^-39 by construction (there is always one such block);
       for them condition 2 is what protects the comparison."""
    L, E, W, nc = c["L"], c["E"], c["W"], ncand(c)
    assert int(L.astype(np.uint64).max(axis=0).sum()) < 1 << 63
    assert np.isfinite(W.astype(np.float64) * E.max(axis=0).astype(np.float64)).all() and (W > 0).all()
    assert np.isfinite(float(m["lam"]) * float(L.max())) and (W * 1.0 > 1e-300).all()
    log = m["log"]
    assert not log.get("near"), "%s: costs within 2^-50 at (multiplier, block) %s" % (c["name"], log["near"][:4])
    # (at the multiplier 0 a cost is W E alone: candidates with equal E cost the same in any arithmetic)
    tied = set(b for lam, b in log.get("ties", ()) if lam != 0)
    assert tied <= c["tie"], "%s: exact ties at blocks %s" % (c["name"], sorted(tied - c["tie"])[:8])
    if m["feasible"] and m["bracketed"] and m["lam"] > 0:
        at, g_at, t_at = RM.choice_at(L, E, W, m["lam"], nc)
        below, g_below, t_below = RM.choice_at(L, E, W, m["lam"] * BELOW, nc)
        moved = [b for b in range(len(at)) if at[b] != below[b]]
        assert moved, c["name"]
        for b in range(len(at)):
            if b in moved:
                continue
            assert not (t_at[b] or t_below[b]) or b in c["tie"], (c["name"], b)
            for g in (g_at[b], g_below[b]):
                assert g is None or g >= GAP, "%s: block %d: costs %s apart at the final multiplier" % (c["name"], b, float(g))
        m["moved"] = moved
    return True
