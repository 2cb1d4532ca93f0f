"""tests/qualitymodel.py pinned on something that is not the model -- every assignment of small tables enumerated by brute force, a
hand-written walk for the trim, examples with the answer written out -- and every table tests/test_gpu_quality_tables.py hands the
quality allocator built here and held against the conditions of tests/qualitytables.py, without a GPU."""
from fractions import Fraction

import numpy as np
import pytest

import qualitymodel as QM
import qualitytables as QT
import ratemodel as RM
from test_rate_model_cpu import every_assignment, small_table

DRAWS = 200


def budgets_of(every):
    """distortion budgets for a small table, in quarters (every_assignment counts 4 x the sum of W E): below the floor, the floor,
    steps in between, the largest distortion there is"""
    ds = sorted(set(d for _, _, d in every))
    picks = {ds[0] - 1, ds[0], ds[len(ds) // 4], ds[len(ds) // 2], ds[len(ds) // 2] - 1, ds[-1], ds[-1] + 5}
    return [Fraction(d, 4) for d in sorted(picks) if d >= 0]


def test_the_answer_by_brute_force_over_every_assignment():
    """n <= 6, ncand <= 4.  The answer's distortion is <= D whenever anything's is; no choice whose distortion is <= the Lagrange
    choice's has fewer bytes than lagrange_bytes (for a multiplier > 0 -- at 0 a coarser candidate of EQUAL error may be shorter,
    which is what the trim then takes); after the trim no single coarser step with strictly fewer bytes fits what is left.
    The last holds where E does not fall towards coarser candidates: then every delta is >= 0, the remainder only shrinks, and a step
    that did not fit when the walk passed cannot fit afterwards.  A table with a negative delta can hand slack back to blocks the
    walk has already left (the kernel walks once): there the property asserted is the walk's own -- tested below, step by step."""
    rng = np.random.default_rng(30)
    searched = trimmed = 0
    for _ in range(DRAWS):
        L, E, W, n, nc = small_table(rng)
        L = L * 7 + np.arange(nc)[::-1, None]                  # (fewer accidental ties between candidates)
        rising = bool((np.diff(E, axis=0) >= 0).all())
        every = every_assignment(L, E, W, n, nc)
        floor4 = min(d for _, _, d in every)
        for D in budgets_of(every):
            dmax = nc - 2
            m = QM.allocate_quality(L, E, W, D, dmax, True)
            assert m["feasible"] == (Fraction(floor4, 4) <= D) and m["floor"] == Fraction(floor4, 4)
            if not m["feasible"]:
                assert m["cand"] == m["start"] == QM.least_error(E, nc) and m["distortion"] == m["floor"] and m["steps"] == 0
                continue
            assert m["distortion"] <= D and m["lagrange_distortion"] <= D
            assert m["block_bytes"] <= m["lagrange"] and all(c >= s for c, s in zip(m["cand"], m["start"]))
            if m["lam"] is QM.INF:
                assert m["start"] == RM.shortest(L, nc) == m["cand"] and m["lagrange"] == min(l for _, l, _ in every)
            elif m["lam"] > 0:
                searched += 1
                assert all(l >= m["lagrange"] for _, l, d in every if Fraction(d, 4) <= m["lagrange_distortion"])
            if rising:
                left = D - m["distortion"]
                for b, c in enumerate(m["cand"]):
                    if c + 1 < nc and int(L[c + 1][b]) < int(L[c][b]):
                        assert Fraction(float(W[b])) * (int(E[c + 1][b]) - int(E[c][b])) > left, (b, c)
                trimmed += m["cand"] != m["start"]
    assert searched > DRAWS and trimmed > DRAWS // 4


def walk_by_hand(L, E, W, cand, D):
    """the trim told one move at a time with the distortion spent carried along -> (candidates, [(block, remainder when the walk
    left the block)])"""
    cand = list(cand)
    spent = QM.distortion(E, W, cand)
    seen = []
    for b in range(len(cand)):
        while cand[b] + 1 < len(L):
            nxt = cand[b] + 1
            added = Fraction(float(W[b])) * (int(E[nxt][b]) - int(E[cand[b]][b]))
            if not (int(L[nxt][b]) < int(L[cand[b]][b]) and spent + added <= D):
                break
            spent += added
            cand[b] = nxt
        seen.append((b, D - spent))
    return cand, seen


def test_trim_against_a_walk_by_hand():
    rng = np.random.default_rng(31)
    moved = 0
    for _ in range(DRAWS):
        L, E, W, n, nc = small_table(rng)
        start = [int(c) for c in rng.integers(0, nc, n)]
        spent = QM.distortion(E, W, start)
        for D in (spent, spent + Fraction(1, 4), spent + 3, spent + 8, spent + 40):
            got = QM.trim(L, E, W, start, D)
            want, seen = walk_by_hand(L, E, W, start, D)
            assert got == want and QM.distortion(E, W, got) <= D and all(g >= s for g, s in zip(got, start))
            assert RM.total_at(L, got) <= RM.total_at(L, start)
            for b, left in seen:             # when the walk left block b its next coarser candidate was not both shorter and within the remainder
                c = got[b]
                assert c + 1 == nc or not (int(L[c + 1][b]) < int(L[c][b]) and Fraction(float(W[b])) * (int(E[c + 1][b]) - int(E[c][b])) <= left)
            moved += got != start
    assert moved > DRAWS


def test_trim_and_least_error_on_examples_written_out():
    W = [1.0, 2.0, 0.5, 1.0]
    # 1. a block that does not fit is passed over: 10 left; block 0 wants 12, block 1 takes 2 x 2 = 4, block 2 takes 0.5 x 12 = 6,
    #    block 3 wants 1 and finds 0
    L = [[20, 9, 11, 3], [8, 5, 5, 2]]
    E = [[0, 0, 0, 0], [12, 2, 12, 1]]
    assert QM.trim(L, E, W, [0, 0, 0, 0], 10) == [0, 1, 1, 0]
    # 2. a candidate that is not shorter stops a chain although the one behind it would be; a chain walks as far as D reaches
    L = [[9, 30], [9, 20], [7, 10], [6, 0]]
    E = [[0, 0], [0, 1], [0, 2], [0, 3]]
    assert QM.trim(L, E, [1.0, 1.0], [0, 0], 100) == [0, 3]
    assert QM.trim(L, E, [1.0, 1.0], [0, 0], 2) == [0, 2]
    # 3. E falling towards a coarser candidate gives distortion back: block 0 walks 0 -> 1 (3, nothing left) -> 2 (2 back), block 1 takes them
    L = [[9, 5], [8, 3], [5, 3]]
    E = [[0, 0], [3, 2], [1, 9]]
    assert QM.trim(L, E, [1.0, 1.0], [0, 0], 3) == [2, 1]
    assert QM.trim(L, E, [1.0, 1.0], [0, 0], 2) == [0, 1]
    # the least error: the finer of equal ones
    assert QM.least_error([[5, 3, 9], [5, 3, 2], [4, 7, 2]], 3) == [2, 0, 1]


def test_search_against_plain_evaluations():
    """qualitymodel.search_quality, which evaluates only the blocks still undecided, against the documented search told plainly"""
    rng = np.random.default_rng(32)
    for k in range(60):
        L, E, W, n, nc = small_table(rng)
        L = L * 7 + np.arange(nc)[::-1, None]
        E = E * 5
        every = every_assignment(L, E, W, n, nc)
        scale = int(rng.integers(-12, 13))
        W = W * float(2.0 ** scale)
        dist = lambda lam: QM.distortion(E, W, RM.choice_at(L, E, W, lam, nc)[0])
        for D4 in budgets_of(every):
            D = D4 * Fraction(2) ** scale
            floor = sum(Fraction(float(W[b])) * min(int(E[c][b]) for c in range(nc)) for b in range(n))
            lam, steps = Fraction(0), 0
            feasible = floor <= D
            short = QM.distortion(E, W, RM.shortest(L, nc)) <= D
            if feasible and short:
                lam = QM.INF
            elif feasible:
                lo = Fraction(1)
                if dist(lo) <= D:
                    while steps < 200 and dist(lo * 2) <= D:
                        lo, steps = lo * 2, steps + 1
                    hi = lo * 2
                else:
                    while True:
                        lo, steps = lo / 2, steps + 1
                        fits = dist(lo) <= D
                        if fits or steps >= 200:
                            break
                    hi = lo * 2
                    if not fits:
                        lo = Fraction(0)
                for _ in range(40):
                    mid = (lo + hi) / 2
                    if dist(mid) <= D:
                        lo = mid
                    else:
                        hi = mid
                    steps += 1
                lam = lo
            got = QM.search_quality(L, E, W, D, nc)
            assert (got["feasible"], got["floor"], got["lam"], got["steps"]) == (feasible, floor, lam, steps)
            assert lam is QM.INF or Fraction(float(lam)) == lam                 # every multiplier of the search is a double


# ---- the tables the kernel is given ------------------------------------------------------------------------------------------------
CASES = QT.all_cases()


def test_the_listed_cases_are_all_there():
    names = [c["name"] for c in CASES]
    assert len(set(names)) == len(names)
    assert set((1, 2, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 3073)) <= set(QT.SIZES) and QT.DROPS == (1, 6, 12)
    assert sum(n.startswith("n ") for n in names) == len(QT.SIZES) * len(QT.DROPS) * 2
    assert {"weights x 2^-160", "weights x 2^160", "below the floor", "dyadic tie", "non-convex, negative delta", "trim order",
            "trim order, reversed", "step budget 0"} <= set(names)
    assert [c["name"] for c in CASES if c["tie"]] == ["dyadic tie"]
    for c in CASES:                      # the weights are powers of two within a factor of 16 of each other, E below 2^30
        m, e = np.frexp(c["W"])
        assert (m == 0.5).all() and e.max() - e.min() <= 4 and int(c["E"].max()) < 1 << 30 and len(c["W"]) <= 3073


@pytest.fixture(scope="module")
def predicted():
    return {c["name"]: QT.predict(c) for c in CASES}


def test_every_table_meets_the_conditions(predicted):
    for c in CASES:
        assert QT.conditions(c, predicted[c["name"]])


def test_the_tables_reach_the_paths_they_are_for(predicted):
    by = {c["name"]: (c, predicted[c["name"]]) for c in CASES}
    # sizes: a search with a finite multiplier, and a trim that moved something, somewhere
    sized = [by[n] for n in by if n.startswith("n ")]
    assert all(m["feasible"] and m["lam"] is not QM.INF and m["lam"] > 0 and m["steps"] > 40 for _, m in sized)
    assert sum(m["cand"] != m["start"] for _, m in sized) > len(sized) // 2
    assert all(m["distortion"] <= Fraction(c["budget"]) for c, m in sized)
    # steps: budgets on the steps (the Lagrange choice spends D to the unit) and one unit below; 0; the shortest choice
    steps = [by[n] for n in by if n.startswith("step budget")]
    L, E, W = QT.snapped_table(*QT.STEP_TABLE)
    curve = QT.curve_distortions(L, E, W, 8)[0]
    d, unit = QT.dist_units(steps[0][0])
    have = set(Fraction(c["budget"]) / unit for c, m in steps)
    assert len(curve) == 169 and all(T in have and (T == 0 or T - 1 in have) for T in curve)          # every step and one unit below it
    assert sum(m["lagrange_distortion"] == Fraction(c["budget"]) for c, m in steps) > 100
    c, m = by["step budget 0"]
    assert m["feasible"] and set(m["drops"]) == {0} and m["distortion"] == 0 and m["block_bytes"] == int(c["L"][0].sum())
    d, unit = QT.dist_units(c)
    short = d.of(RM.shortest(c["L"], 8))
    for k, inf in ((short, True), (2 * short, True), (short - 1, False)):
        m = by["step budget %d" % k][1]
        assert (m["lam"] is QM.INF) == inf and (not inf or (m["steps"] == 0 and set(m["drops"]) == {RM.SKIP_BYTE} and m["block_bytes"] == 0))
    # scales: the steps follow the weights
    lo, hi = by["weights x 2^-160"][1], by["weights x 2^160"][1]
    assert lo["steps"] > 40 + 150 and 40 + 120 < hi["steps"] < 40 + 160 and lo["lam"] < 1 < hi["lam"]
    # below the floor: no search, the least-E drops, the finer of two equal ones
    c, m = by["below the floor"]
    assert not m["feasible"] and m["steps"] == 0 and m["lam"] == 0 and m["cand"] == m["start"] == QM.least_error(c["E"], 8)
    assert len(set(m["cand"])) == 8 and m["distortion"] == m["floor"] > Fraction(c["budget"])
    assert any((c["E"][:, b] == c["E"][:, b].min()).sum() == 2 for b in range(70))
    # the tie
    c, m = by["dyadic tie"]
    assert m["lam"] == 1 and m["steps"] == 40 and m["cand"] == [0, 0] and (1, 0) in [(int(lam), b) for lam, b in m["log"]["ties"] if lam == 1]
    # non-convex and negative delta
    c, m = by["non-convex, negative delta"]
    assert m["start"] == [0, 1, 0, 0] and m["cand"] == [0, 1, 2, 1] and m["distortion"] == 319 and Fraction(1002, 100) - Fraction(1, 1000) < m["lam"] < Fraction(1002, 100)
    # the order, across the chunks of 256
    c, m = by["trim order"]
    at = (0, 1, 255, 256, 511, 512, 513, 514)
    assert set(m["start"]) == {0} and [m["cand"][b] for b in at] == [0, 13, 1, 0, 1, 0, 1, 0] and m["distortion"] == Fraction(c["budget"])
    assert m["drops"][1] == RM.SKIP_BYTE
    c, m = by["trim order, reversed"]
    n = QT.ORDER_N - 1
    assert [m["cand"][n - b] for b in at] != [0, 13, 1, 0, 1, 0, 1, 0] and m["distortion"] <= Fraction(c["budget"])
