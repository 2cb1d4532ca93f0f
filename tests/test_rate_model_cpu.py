"""tests/ratemodel.py pinned on something that is not the model: every assignment of small tables enumerated by brute force, a
hand-written walk for the fill, three examples with the answer written out.  Then every table tests/test_gpu_rate_tables.py hands
the allocator kernel is built here and held against the conditions of tests/ratetables.py -- without a GPU."""
import itertools
from fractions import Fraction

import numpy as np
import pytest

import ratemodel as RM
import ratetables as RT

DRAWS = 300
LAMS = [Fraction(0)] + [Fraction(k, 8) for k in (1, 2, 3, 5, 8, 11, 16, 24, 40, 64, 100, 160, 400, 1000)]


def small_table(rng):
    """2 .. 6 blocks, 3 .. 4 candidates, small integers (ties, plateaus and non-convex columns among them); weights k / 4"""
    n, nc = int(rng.integers(2, 7)), int(rng.integers(3, 5))
    L = rng.integers(0, 9, (nc, n))
    E = rng.integers(0, 9, (nc, n))
    if rng.random() < 0.7:                 # mostly the usual shape: L falling, E rising
        L, E = -np.sort(-L, axis=0), np.sort(E, axis=0)
    W = rng.integers(1, 9, n) / 4.0
    return L, E, W, n, nc


def every_assignment(L, E, W, n, nc):
    """-> [(assignment, bytes, 4 x the sum of W E: an integer, the weights are k / 4)]"""
    w4 = [int(w * 4) for w in W]
    assert all(Fraction(k, 4) == Fraction(float(w)) for k, w in zip(w4, W))
    Li, Ei = [[int(v) for v in r] for r in L], [[int(v) * w4[b] for b, v in enumerate(r)] for r in E]
    out = []
    for a in itertools.product(range(nc), repeat=n):
        out.append((a, sum(Li[c][b] for b, c in enumerate(a)), sum(Ei[c][b] for b, c in enumerate(a))))
    return out


def test_choice_minimises_the_lagrangian_over_every_assignment():
    rng = np.random.default_rng(20)
    for _ in range(DRAWS):
        L, E, W, n, nc = small_table(rng)
        every = every_assignment(L, E, W, n, nc)
        before = None
        for lam in LAMS:
            choice, gaps, ties = RM.choice_at(L, E, W, lam, nc)
            got_l = RM.total_at(L, choice)
            got_d = 4 * sum(Fraction(float(W[b])) * int(E[c][b]) for b, c in enumerate(choice))
            lam32 = int(lam * 32)                                       # (the multipliers are k / 8)
            assert 8 * got_d + lam32 * got_l == min(8 * d + lam32 * l for _, l, d in every)
            # the finer candidate of an exact tie: no block could move to a finer candidate at the same cost
            for b, c in enumerate(choice):
                cost = [Fraction(float(W[b])) * int(E[k][b]) + lam * int(L[k][b]) for k in range(nc)]
                assert cost[c] == min(cost) and all(cost[k] > cost[c] for k in range(c))
                rest = [v for v in cost if v != cost[c]]
                assert gaps[b] == (Fraction(min(rest) - cost[c], cost[c]) if rest and cost[c] > 0 else None)
                assert ties[b] == any(cost[k] == cost[c] and (L[k][b], E[k][b]) != (L[c][b], E[c][b]) for k in range(nc))
            # no assignment with at most these bytes has a smaller sum of W E
            assert all(d >= got_d for _, l, d in every if l <= got_l)
            # the bytes never rise as the multiplier grows
            assert before is None or got_l <= before
            before = got_l


def walk_by_hand(L, E, cand, budget):
    """the fill told step by step, one move at a time with the remainder carried along -> (candidates, [(block, remainder when the
    walk left the block)])"""
    cand = list(cand)
    spent = sum(int(L[c][b]) for b, c in enumerate(cand))
    seen = []
    for b in range(len(cand)):
        moved = True
        while moved:
            moved = False
            if cand[b] == 0:
                break
            finer = cand[b] - 1
            lowers = int(E[finer][b]) < int(E[cand[b]][b])
            added = int(L[finer][b]) - int(L[cand[b]][b])
            if lowers and spent + added <= budget:
                spent += added
                cand[b] = finer
                moved = True
        seen.append((b, budget - spent))
    return cand, seen


def test_fill_stays_within_the_budget_and_leaves_nothing_it_could_take():
    rng = np.random.default_rng(21)
    for _ in range(DRAWS):
        L, E, W, n, nc = small_table(rng)
        start = [int(c) for c in rng.integers(0, nc, n)]
        spent = RM.total_at(L, start)
        for budget in (spent, spent + 1, spent + 3, spent + 8, spent + 40):
            got = RM.fill(L, E, start, budget)
            assert RM.total_at(L, got) <= budget
            assert all(g <= s for g, s in zip(got, start))
            want, seen = walk_by_hand(L, E, start, budget)
            assert got == want
            # when the walk left block b, its next finer candidate did not both lower E and fit the remainder of that moment
            for b, left in seen:
                c = got[b]
                assert c == 0 or not (int(E[c - 1][b]) < int(E[c][b]) and int(L[c - 1][b]) - int(L[c][b]) <= left)


def test_fill_on_three_examples_written_out():
    # 1. a block that does not fit is passed over, the walk goes on with the remainder: 10 left; block 0 wants 12, block 1 takes 4,
    #    block 2 takes 6, block 3 wants 1 and finds 0
    L = [[20, 9, 11, 3], [8, 5, 5, 2]]
    E = [[0, 0, 0, 0], [9, 9, 9, 9]]
    assert RM.fill(L, E, [1, 1, 1, 1], 20 + 10) == [1, 0, 0, 1]
    # 2. a plateau of E stops a chain although the finer rows would fit; a chain walks as far as the bytes reach
    L = [[9, 30], [8, 20], [7, 10], [6, 0]]
    E = [[0, 0], [4, 1], [4, 2], [5, 3]]
    assert RM.fill(L, E, [3, 3], 6 + 100) == [2, 0]
    assert RM.fill(L, E, [3, 3], 6 + 25) == [2, 1]
    # 3. a finer candidate that is SHORTER gives bytes back: block 0 walks 2 -> 1 (3 bytes, nothing left) -> 0 (2 back), block 1
    #    takes the 2
    L = [[6, 5], [8, 3], [5, 0]]
    E = [[0, 0], [1, 7], [2, 0]]
    assert RM.fill(L, E, [2, 1], 8 + 3) == [0, 0]
    assert RM.fill(L, E, [2, 1], 8 + 2) == [2, 0]


def test_shortest_least_and_the_search_against_plain_evaluations():
    """shortest / least by enumeration; ratemodel.search, which evaluates only the blocks still undecided, against the documented
    search told plainly: every total from choice_at over all blocks"""
    rng = np.random.default_rng(22)
    for k in range(60):
        L, E, W, n, nc = small_table(rng)
        L = L * 7 + np.arange(nc)[::-1, None]                  # (longer tables, fewer accidental ties)
        E = E * 5
        every = every_assignment(L, E, W, n, nc)
        W = W * float(2.0 ** int(rng.integers(-12, 13)))
        lst = min(l for _, l, _ in every)
        assert RM.least(L, nc) == lst
        sh = RM.shortest(L, nc)
        assert RM.total_at(L, sh) == lst and all(int(L[c][b]) > int(L[sh[b]][b]) for b in range(n) for c in range(sh[b]))
        for budget in sorted(set([lst - 1, lst, (lst + int(L[0].sum())) // 2, int(L[0].sum()) - 1, int(L[0].sum())])):
            if budget < 0:
                continue
            total = lambda lam: RM.total_at(L, RM.choice_at(L, E, W, lam, nc)[0])
            lam, steps, bracketed = Fraction(0), 0, True
            if lst <= budget and total(0) > budget:
                hi = Fraction(1)
                if total(hi) <= budget:
                    while steps < 200 and total(hi / 2) <= budget:
                        hi, steps = hi / 2, steps + 1
                    lo = hi / 2 if steps < 200 else Fraction(0)
                else:
                    while True:
                        hi, steps = hi * 2, steps + 1
                        if steps >= 200 or total(hi) <= budget:
                            break
                    bracketed = total(hi) <= budget
                    lo = hi / 2
                for _ in range(40):
                    mid = (lo + hi) / 2
                    if total(mid) <= budget:
                        hi = mid
                    else:
                        lo = mid
                    steps += 1
                lam = hi
            got = RM.search(L, E, W, budget, nc)
            assert (got["feasible"], got["least"], got["lam"], got["steps"], got["bracketed"]) == (lst <= budget, lst, lam, steps, bracketed)
            assert RM.bracket_steps(L, E, W, budget, nc) == steps
            # every multiplier of the search is a double
            assert Fraction(float(lam)) == lam


def test_errors_on_values_written_out():
    # kmax 4: c clamps to 3.  q = 5: c = 1 -> (5 >> 1 << 1) + 1 = 5: 0; c = 2 -> 4 + 2 = 6: (2)^2 = 4; c = 3 -> 0: (10)^2 = 100
    assert RM.errors(np.array([5]), 4, 5) == [0, 0, 4, 100, 100, 100, 100]
    # q = 8 on a power of two: c = 3 -> 8 + 4 = 12: 64; q = 7: c = 3 -> 0: 196
    assert RM.errors(np.array([8, 7]), 6, 3) == [0, 4 + 0, 16 + 4, 64 + 196, 256 + 196]
    # the 9/7 quantiser: the float32 product by the float32 reciprocal, truncated, clamped to 2^kmax - 1
    step = np.float32(0.3)
    got = RM.quantised(np.array([[-1.0, 0.29, 0.3 * 40, 1000.0]], np.float32), 5, step, True)
    inv = np.float32(1.0) / step
    assert got.tolist() == [[int(np.float32(1.0) * inv), 0, min(int(np.float32(np.float32(0.3 * 40) * inv)), 31), 31]]
    assert RM.quantised(np.array([[-7, 0, 9]]), 5, 1.0, False).tolist() == [[7, 0, 9]]


# ---- the tables the kernel is given ------------------------------------------------------------------------------------------------
CASES = RT.all_cases()


def test_the_listed_cases_are_all_there():
    names = [c["name"] for c in CASES]
    assert len(set(names)) == len(names)
    assert sum(n.startswith("n ") for n in names) == len(RT.SIZES) * len(RT.DROPS) * 2
    assert sum(n.startswith("weights x") for n in names) == 5
    assert {"plateaus", "dyadic tie", "non-convex", "fill order", "fill order, reversed"} <= set(names)
    # (the tie is the only one allowed in the file)
    assert [c["name"] for c in CASES if c["tie"]] == ["dyadic tie"]


@pytest.fixture(scope="module")
def predicted():
    return {c["name"]: RT.predict(c) for c in CASES}


def test_every_table_meets_the_conditions(predicted):
    for c in CASES:
        assert RT.conditions(c, predicted[c["name"]])


def test_the_tables_reach_the_paths_they_are_for(predicted):
    by = {c["name"]: (c, predicted[c["name"]]) for c in CASES}
    # sizes: a search, a multiplier, a fill that moved something, somewhere
    sized = [by[n] for n in by if n.startswith("n ")]
    assert all(m["feasible"] and m["bracketed"] and m["lam"] > 0 for _, m in sized)
    assert sum(m["cand"] != m["start"] for _, m in sized) > len(sized) // 2
    # steps: budgets on and beside the steps; not feasible below least; everything skipped at 0; the finest at the top
    steps = [by[n] for n in by if n.startswith("step budget")]
    assert len(steps) > 100
    c, m = by["step budget 0"]
    assert m["feasible"] and set(m["drops"]) == {RM.SKIP_BYTE} and m["block_bytes"] == 0
    finest = int(c["L"][0].sum())
    assert by["step budget %d" % finest][1]["lam"] == 0 and by["step budget %d" % (finest - 1)][1]["lam"] > 0
    assert any(m["lagrange"] == c["budget"] for c, m in steps) and any(m["lagrange"] == c["budget"] - 1 for c, m in steps)
    assert not by["no SKIP, budget least-1"][1]["feasible"] and by["no SKIP, budget least+0"][1]["feasible"]
    assert by["no SKIP, budget least-1"][1]["drops"] == [6] * RT.STEP_TABLE[0]
    # scales: the steps follow the weights; 2^230 is beyond the search
    st = [by["weights x 2^%d" % k][1] for k in RT.SCALES]
    assert [m["bracketed"] for m in st] == [True, True, True, True, False]
    assert st[0]["steps"] > 40 + 140 and 40 + 25 < st[1]["steps"] < 40 + 50 and 40 + 35 < st[2]["steps"] < 40 + 60 and st[3]["steps"] > 40 + 150
    assert st[4]["steps"] == 240 and st[4]["lam"] == Fraction(2) ** 200 and st[4]["start"] == RM.shortest(by["weights x 2^230"][0]["L"], 8)
    assert st[4]["block_bytes"] <= by["weights x 2^230"][0]["budget"] and st[4]["cand"] != st[4]["start"]
    # plateaus: the clamp's rows, the all-zero block at candidate 1, the fill stopped by E[1] == E[2] with bytes to spare
    c, m = by["plateaus"]
    assert m["start"] == [1, 3, 1, 3, 1] and m["cand"] == [1, 0, 1, 2, 0]
    assert c["budget"] - m["block_bytes"] >= int(c["L"][0][3]) - int(c["L"][2][3])
    # the tie
    c, m = by["dyadic tie"]
    assert m["lam"] == 1 + Fraction(1, 1 << 40) and m["steps"] == 41 and m["cand"] == [1, 0]
    assert (1, 0) in [(int(lam), b) for lam, b in m["log"]["ties"] if lam == 1]
    # non-convex: candidate 2 of block 1 is passed through, its 5 bytes come back
    c, m = by["non-convex"]
    assert m["start"] == [1, 3, 1, 1] and m["cand"] == [1, 1, 0, 1] and m["block_bytes"] == c["budget"]
    # the order
    c, m = by["fill order"]
    assert [m["start"][b] for b in (0, 1, 511, 512, 513, 514)] == [1, 13, 1, 1, 1, 1]
    assert [m["cand"][b] for b in (0, 1, 511, 512, 513, 514)] == [1, 0, 0, 1, 0, 1] and m["block_bytes"] == c["budget"]
    c, m = by["fill order, reversed"]
    n = RT.ORDER_N - 1
    assert [m["cand"][n - b] for b in (0, 1, 511, 512, 513, 514)] == [1, 3, 0, 0, 0, 0]
