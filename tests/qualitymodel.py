"""The quality allocator (KQ, grok_amd/csrc/kernels_rate.hip) restated in exact arithmetic on top of ratemodel._Tables, as
include/grok_amd.h and grok_amd/csrc/kernels.h word it: the largest multiplier whose Lagrange choice keeps the sum of W E within a
distortion budget D, then the trim in table order.

Nothing here computes in floating point: weights, D and the multipliers are exact rationals, a distortion is an integer count of a
unit every weight is a multiple of (doubles are dyadic: the unit is 1 / the largest denominator).  The model says what the documented
search does when every cost and every sum is exact; tests/qualitytables.py asserts, on the CPU, that its tables leave the kernel's
double arithmetic no room to differ."""
from fractions import Fraction

import numpy as np

import ratemodel as RM

BISECT_STEPS = RM.BISECT_STEPS
BRACKET_LIMIT = RM.BRACKET_LIMIT
SKIP_BYTE = RM.SKIP_BYTE
INF = None                   # how a multiplier of +infinity is written here


class _Dist:
    """sums of W E as integers: W_b = wi[b] * unit"""

    def __init__(self, t):
        self.t = t
        # the largest power of two every weight is a whole multiple of (a double n / d in lowest terms: 1 / d, or n's lowest set bit)
        self.unit = min(Fraction(1, int(d)) if int(d) > 1 else Fraction(int(n) & -int(n)) for n, d in zip(t.wn, t.wd))
        self.wi = np.array([int(Fraction(int(n), int(d)) / self.unit) for n, d in zip(t.wn, t.wd)], dtype=object)
        assert all(v * self.unit == Fraction(int(n), int(d)) for v, n, d in zip(self.wi, t.wn, t.wd))

    def of(self, cand, idx=None):
        """the exact distortion of candidates `cand` for the blocks `idx` (all), in units"""
        cols = np.arange(self.t.n) if idx is None else np.asarray(idx)
        if not len(cols):
            return 0
        cand = np.asarray(cand, dtype=np.int64)
        return int((self.wi[cols] * self.t.E[cand, cols]).sum())

    def floor(self):
        return int((self.wi * self.t.E.min(axis=0)).sum())


def least_error(E, ncand):
    """every block at its least-E candidate, the finer of equal ones"""
    n = len(E[0])
    return [min(range(ncand), key=lambda c: (int(E[c][b]), c)) for b in range(n)]


def distortion(E, W, cand):
    return sum(Fraction(float(W[b])) * int(E[c][b]) for b, c in enumerate(cand))


def search_quality(L, E, W, D, ncand, log=None):
    """The documented search with every distortion computed exactly -> dict(feasible, floor (Fraction), lam (Fraction; INF: the
    shortest choice fits), steps, all_short).  Not feasible: no search.  The shortest choice within D: no search, lam INF.  Else from
    1: double while the doubled multiplier still fits (a probe that does not fit is not a step) or halve until one fits -- both stop
    at BRACKET_LIMIT, halving that never fits ends at 0 --, then BISECT_STEPS bisections that keep the LOWER end fitting.
    As ratemodel.search, the bisection evaluates only blocks whose choice differs between the bracket's ends, and every evaluation
    is logged (log: see ratemodel._Tables.choice)."""
    t = RM._Tables(L, E, W, ncand)
    d = _Dist(t)
    budget = Fraction(D) / d.unit                          # in units; a fit is an integer <= this
    out = dict(feasible=d.floor() <= budget, floor=d.floor() * d.unit, lam=Fraction(0), steps=0, all_short=False)
    if not out["feasible"]:
        return out
    if d.of(RM.shortest(L, ncand)) <= budget:
        out.update(all_short=True, lam=INF)
        return out
    lo, steps = Fraction(1), 0
    ch_lo = t.choice(lo, log=log)
    if d.of(ch_lo) <= budget:
        ch_hi = None
        while steps < BRACKET_LIMIT:
            ch = t.choice(lo * 2, log=log)
            if d.of(ch) > budget:
                ch_hi = ch
                break
            lo, ch_lo, steps = lo * 2, ch, steps + 1
        hi = lo * 2
        if ch_hi is None:
            ch_hi = t.choice(hi, log=log)
    else:
        while True:
            ch_hi = ch_lo
            lo, steps = lo / 2, steps + 1
            ch_lo = t.choice(lo, log=log)
            fits = d.of(ch_lo) <= budget
            if fits or steps >= BRACKET_LIMIT:
                break
        hi = lo * 2
        if not fits:
            lo, ch_lo = Fraction(0), t.choice(0, log=log)
    act = np.flatnonzero(ch_lo != ch_hi)
    settled = np.flatnonzero(ch_lo == ch_hi)
    fixed = d.of(ch_lo[settled], settled)
    for _ in range(BISECT_STEPS):
        mid = (lo + hi) / 2
        ch = t.choice(mid, act, log=log)
        if fixed + d.of(ch, act) <= budget:
            lo, ch_lo[act] = mid, ch
        else:
            hi, ch_hi[act] = mid, ch
        same = ch_lo[act] == ch_hi[act]
        fixed += d.of(ch_lo[act[same]], act[same])
        act = act[~same]
    out["lam"], out["steps"] = lo, steps + BISECT_STEPS
    return out


def trim(L, E, W, cand, D):
    """The header's wording: in table order, a block moves to the next coarser candidate while L strictly falls and the distortion
    it adds -- W (E[c + 1] - E[c]), which may be negative -- fits what is left of D; a block that does not fit is passed over and the
    walk goes on with the remainder.  -> the candidates afterwards"""
    ncand = len(L)
    cand = [int(c) for c in cand]
    left = Fraction(D) - distortion(E, W, cand)
    for b in range(len(cand)):
        c, w = cand[b], Fraction(float(W[b]))
        while c + 1 < ncand and int(L[c + 1][b]) < int(L[c][b]) and w * (int(E[c + 1][b]) - int(E[c][b])) <= left:
            left -= w * (int(E[c + 1][b]) - int(E[c][b]))
            c += 1
        cand[b] = c
    return cand


def allocate_quality(L, E, W, D, dmax, allow_skip, log=None):
    """The kernel's whole answer -> dict: the search's fields, start (the choice the trim starts from: the Lagrange choice at lam,
    the shortest choice, or -- not feasible -- the least-E choice, which gets no trim), lagrange (its bytes), lagrange_distortion,
    cand, drops, block_bytes, shortest_bytes, distortion (exact, a Fraction)."""
    ncand = dmax + 1 + (1 if allow_skip else 0)
    Lc, Ec = [L[c] for c in range(ncand)], [E[c] for c in range(ncand)]
    out = search_quality(L, E, W, D, ncand, log)
    if not out["feasible"]:
        start = least_error(E, ncand)
    elif out["all_short"]:
        start = RM.shortest(L, ncand)
    else:
        start = RM.choice_at(L, E, W, out["lam"], ncand)[0]
    cand = trim(Lc, Ec, W, start, D) if out["feasible"] else list(start)
    out.update(start=start, lagrange=RM.total_at(L, start), lagrange_distortion=distortion(E, W, start), cand=cand,
               drops=[c if c <= dmax else SKIP_BYTE for c in cand], block_bytes=RM.total_at(L, cand),
               shortest_bytes=RM.least(L, ncand), distortion=distortion(E, W, cand))
    return out
