"""The rate-targeted encodes' two kernels (grok_amd/csrc/kernels_rate.hip) restated in exact arithmetic: the statistics KR1 writes
and the choice KR2 makes, as include/grok_amd.h and the kernels' comments word them.

Nothing here computes in floating point.  A double is an exact rational, so a cost W E + lambda L is one too; the candidates of a block
are compared as integers over a common positive denominator (which is what comparing fractions.Fraction values does, without the
reductions).  The model therefore says what the documented search does when every cost is compared exactly; the tests that hold the
kernel against it first assert, on the CPU, that their tables leave the kernel's double arithmetic no room to differ (best and
next-best cost apart by 2^-30 relative where it matters, deliberate ties made of exact doubles)."""
from fractions import Fraction

import numpy as np

BISECT_STEPS = 40          # kRateBisectSteps
BRACKET_LIMIT = 200        # doublings or halvings from 1 before the search gives up
SKIP_BYTE = 0xFF           # kHtDropSkip
# Two exact costs a < b with (b - a) / a >= NEAR compare the same way in double arithmetic.  L and E below 2^53 convert exactly; each
# product rounds once (u = 2^-53), the sum of the two non-negative terms once more -- or, fused, one rounding fewer --, so a computed
# cost is the exact one times (1 + d) with |d| <= 2 u + u^2, and a (1 + d1) < b (1 + d2) holds as soon as b / a > (1 + 2.001 u) /
# (1 - 2.001 u), that is from a relative gap of about 4 u = 2^-51: 2^-50 leaves a factor of two.
NEAR = Fraction(1, 1 << 50)


# ---- KR1 ---------------------------------------------------------------------------------------------------------------------------
def quantised(plane_block, kmax, stepsize, irrev):
    """the magnitudes the d = 0 coder codes for a block of a plane: |x|, or trunc(|c| * (1 / step)) in float32 -- the float32 product
    by the float32 reciprocal --, clamped to 2^kmax - 1"""
    sub = np.asarray(plane_block)
    if not irrev:
        return np.abs(sub.astype(np.int64))
    q = (np.abs(sub).astype(np.float32) * (np.float32(1.0) / np.float32(stepsize))).astype(np.float32)
    return np.minimum(np.trunc(q).astype(np.int64), (1 << kmax) - 1)


def errors(q, kmax, dmax):
    """E of one block as include/grok_amd.h defines it -> dmax + 2 Python integers.  Row 0: 0.  Row c = 1 .. dmax: the sum over the
    block of (2 q - 2 r_c(q))^2 with r_c(q) = 0 where q >> c == 0, else ((q >> c) << c) + 2^(c - 1), c taken as min(c, kmax - 1), the
    drop the coder clamps to.  Row dmax + 1, SKIP: the sum of (2 q)^2."""
    q = np.asarray(q).astype(np.int64)
    assert q.size == 0 or (0 <= int(q.min()) and int(q.max()) < 1 << 25)         # (int64 holds the sums of a 64 x 64 block)
    out = [0] * (dmax + 2)
    for c in range(1, dmax + 1):
        ce = min(c, max(kmax - 1, 0))
        rc = np.where(q >> ce == 0, 0, ((q >> ce) << ce) + ((1 << ce) >> 1))
        out[c] = int(((2 * q - 2 * rc) ** 2).sum())
    out[dmax + 1] = int(((2 * q) ** 2).sum())
    return out


# ---- KR2 ---------------------------------------------------------------------------------------------------------------------------
class _Tables:
    """L, E [ncand][n] and the weights as Python integers (object arrays): cost_c(b) * (den(W_b) * den(lam)) =
    num(W_b) den(lam) E + num(lam) den(W_b) L"""

    def __init__(self, L, E, W, ncand):
        self.n = len(W)
        self.ncand = ncand
        self.L = np.array([[int(v) for v in L[c]] for c in range(ncand)], dtype=object).reshape(ncand, self.n)
        self.E = np.array([[int(v) for v in E[c]] for c in range(ncand)], dtype=object).reshape(ncand, self.n)
        w = [Fraction(v) for v in W]
        assert all(v > 0 for v in w)
        self.wn = np.array([v.numerator for v in w], dtype=object)
        self.wd = np.array([v.denominator for v in w], dtype=object)

    def costs(self, lam, idx=None):
        lam = Fraction(lam)
        sl = slice(None) if idx is None else idx
        return (self.wn[sl] * lam.denominator)[None, :] * self.E[:, sl] + (self.wd[sl] * lam.numerator)[None, :] * self.L[:, sl]

    def choice(self, lam, idx=None, log=None):
        """argmin_c of the cost; numpy's argmin takes the first of equal values: the finer candidate wins an exact tie.
        log (a dict): log["near"] gets (lam, block) for every block whose best cost and the next one that is not exactly equal lie
        within NEAR relative, log["ties"] the same for every block where a candidate with another (L, E) pair costs exactly as much
        as the best -- the evaluations a double computation could judge differently."""
        cost = self.costs(lam, idx)
        m = cost.shape[1]
        if not m:
            return np.zeros(0, np.int64)
        ch = np.argmin(cost, axis=0).astype(np.int64)
        if log is not None:
            cols = np.arange(self.n) if idx is None else np.asarray(idx)
            best = cost[ch, np.arange(m)]
            other = cost != best[None, :]
            big = max(int(v) for v in cost.max(axis=0)) + 1
            nxt = np.where(other, cost, big).min(axis=0)
            near = other.any(axis=0) & np.array([(int(n) - int(b)) * NEAR.denominator < int(b) * NEAR.numerator for n, b in zip(nxt, best)], bool)
            Ls, Es = self.L[:, cols], self.E[:, cols]
            same = (Ls == Ls[ch, np.arange(m)][None, :]) & (Es == Es[ch, np.arange(m)][None, :])
            tie = (~other & ~same).any(axis=0)
            log.setdefault("near", []).extend((lam, int(b)) for b in cols[near])
            log.setdefault("ties", []).extend((lam, int(b)) for b in cols[tie])
        return ch

    def bytes_of(self, cand, idx=None):
        cols = np.arange(self.n) if idx is None else idx
        return int(sum(self.L[cand, cols])) if len(cols) else 0


def choice_at(L, E, W, lam, ncand):
    """-> (choice [n], gaps [n], ties [n]).  choice: each block's argmin_c W E + lam L over c < ncand, exactly, the finer candidate
    on an exact tie.  gaps: per block, (next - best) / best as a Fraction for the smallest cost that is not exactly equal to the best
    one -- None where there is none, or where the best cost is 0 and the gap has no scale.  ties: per block, whether a candidate with
    ANOTHER (L, E) pair costs exactly as much as the best (candidates with the same L and E are the same numbers to any arithmetic)."""
    t = _Tables(L, E, W, ncand)
    cost = t.costs(lam)
    choice = [int(c) for c in np.argmin(cost, axis=0)]
    gaps, ties = [], []
    for b in range(t.n):
        col = [cost[c, b] for c in range(ncand)]
        best = col[choice[b]]
        rest = [v for v in col if v != best]
        gaps.append(Fraction(min(rest) - best, best) if rest and best > 0 else None)
        ties.append(any(col[c] == best and (t.L[c, b], t.E[c, b]) != (t.L[choice[b], b], t.E[choice[b], b]) for c in range(ncand)))
    return choice, gaps, ties


def total_at(L, choice):
    return sum(int(L[c][b]) for b, c in enumerate(choice))


def fill(L, E, cand, budget):
    """The header's wording in integers: in table order, a block moves to the next finer candidate while E strictly falls and the
    added bytes -- which may be negative -- fit what is left; a block that does not fit is passed over and the walk goes on with the
    remainder.  -> the candidates afterwards"""
    cand = [int(c) for c in cand]
    left = budget - total_at(L, cand)
    for b in range(len(cand)):
        c = cand[b]
        while c > 0 and int(E[c - 1][b]) < int(E[c][b]) and int(L[c - 1][b]) - int(L[c][b]) <= left:
            left -= int(L[c - 1][b]) - int(L[c][b])
            c -= 1
        cand[b] = c
    return cand


def shortest(L, ncand):
    """the fallback choice: every block at its shortest candidate, the finer one of equally short ones"""
    n = len(L[0])
    return [min(range(ncand), key=lambda c: (int(L[c][b]), c)) for b in range(n)]


def least(L, ncand):
    return total_at(L, shortest(L, ncand))


def search(L, E, W, budget, ncand, log=None):
    """The documented multiplier search with every total computed exactly -> dict(feasible, least, lam (Fraction), steps, bracketed).
    Not feasible, or the finest choice fits: no search, lam 0.  Else from 1: halve while the smaller value still fits, or double
    until one fits -- both stop at BRACKET_LIMIT --, then BISECT_STEPS bisections that keep the upper end fitting.  Every value the
    search visits is a dyadic rational with at most 41 significant bits: exactly the double the kernel holds.
    The bisection evaluates only blocks whose choice differs between the bracket's ends: a block with the same choice c at both
    ends has cost_c - cost_j, which is linear in the multiplier, <= 0 at both (< 0 for finer j), hence in between -- and its relative
    distance to cost_c, a quotient of linear functions, is monotone in between: no smaller than at the nearer end.
    log: see _Tables.choice; every evaluation the search makes is logged (the bracket's ends for every block)."""
    t = _Tables(L, E, W, ncand)
    lst = least(L, ncand)
    out = dict(feasible=lst <= budget, least=lst, lam=Fraction(0), steps=0, bracketed=True)
    if not out["feasible"] or t.bytes_of(t.choice(0, log=log)) <= budget:
        return out
    hi, steps = Fraction(1), 0
    ch_hi = t.choice(hi, log=log)
    if t.bytes_of(ch_hi) <= budget:
        lo, ch_lo = Fraction(0), None
        while steps < BRACKET_LIMIT:
            ch = t.choice(hi / 2, log=log)
            if t.bytes_of(ch) > budget:
                lo, ch_lo = hi / 2, ch
                break
            hi, ch_hi, steps = hi / 2, ch, steps + 1
        if ch_lo is None:
            ch_lo = t.choice(0, log=log)
    else:
        while True:
            ch_lo = ch_hi
            hi, steps = hi * 2, steps + 1
            ch_hi = t.choice(hi, log=log)
            fits = t.bytes_of(ch_hi) <= budget
            if fits or steps >= BRACKET_LIMIT:
                break
        out["bracketed"] = fits
        lo = hi / 2
    act = np.flatnonzero(ch_lo != ch_hi)
    settled = np.flatnonzero(ch_lo == ch_hi)
    fixed = t.bytes_of(ch_hi[settled], settled)
    for _ in range(BISECT_STEPS):
        mid = (lo + hi) / 2
        ch = t.choice(mid, act, log=log)
        if fixed + t.bytes_of(ch, act) <= budget:
            hi, ch_hi[act] = mid, ch
        else:
            lo, ch_lo[act] = mid, ch
        same = ch_lo[act] == ch_hi[act]
        fixed += t.bytes_of(ch_hi[act[same]], act[same])
        act = act[~same]
    out["lam"], out["steps"] = hi, steps + BISECT_STEPS
    return out


def bracket_steps(L, E, W, budget, ncand):
    """the number of multiplier evaluations the documented search makes"""
    return search(L, E, W, budget, ncand)["steps"]


def allocate(L, E, W, budget, dmax, allow_skip, log=None):
    """The kernel's whole answer as the documentation words it -> dict: the search's fields, start (the choice the fill starts from:
    the Lagrange choice at lam, or -- not feasible, or no multiplier found -- the shortest choice), lagrange (its bytes), cand (after
    the fill; a budget that is not feasible gets no fill), drops (cand as drop bytes: dmax + 1 is SKIP_BYTE), block_bytes,
    distortion (the exact sum of W E, a Fraction)."""
    ncand = dmax + 1 + (1 if allow_skip else 0)
    out = search(L, E, W, budget, ncand, log)
    if out["feasible"] and out["bracketed"]:
        start = choice_at(L, E, W, out["lam"], ncand)[0]
    else:
        start = shortest(L, ncand)
    cand = fill(L, E, start, budget) if out["feasible"] else list(start)
    out.update(start=start, lagrange=total_at(L, start), cand=cand, drops=[c if c <= dmax else SKIP_BYTE for c in cand],
               block_bytes=total_at(L, cand), distortion=sum(Fraction(W[b]) * int(E[c][b]) for b, c in enumerate(cand)))
    return out
