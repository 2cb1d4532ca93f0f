"""CPU: what a rate-targeted encode needs from the host -- the Tier-2 writer's zero-bit-plane tag trees over the rows' own
missing_msbs (GRK_AMD_CS_BLOCK_MSBS, grok_amd/csrc/t2_writer.cpp), read back by the library's reader and by tests/j2kparse.py; the
cases in which the flag changes no byte; the format assumption itself -- a block coded as mu >> d under Kmax - 1 - d zero
bit-planes -- against the real reference decoder where oracle/_ref is present; and the host planning of the new block-coder
instances and tables (grok_amd/csrc/encode_plan.cpp) through tests/c/rate_plan_units.cpp."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import grok_amd as G
import j2kparse
import oracle as O
import refharness as R
import synth
from grok_amd.capi import CODED_DTYPE, ERR_UNSUPPORTED

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
MSBS = G.CS_BLOCK_MSBS
needs_ref = pytest.mark.skipif(not R.have_ref(), reason="oracle/_ref (the real reference) not built here")


def hand_table(layout, base, seed, constant=False):
    """rows built by hand for every tile of the layout: lengths 0 .. 299 (one in eight 0), bytes below 0x80 (no marker can appear),
    missing_msbs in [kmax - 1 - 6, kmax - 1] (kmax - 1 everywhere when constant)"""
    rng = np.random.default_rng(seed)
    tabs, off = [], 0
    for p in G.layout_tiles(layout, base):
        blocks, _ = G.tile_layout(p)
        t = np.zeros(len(blocks), CODED_DTYPE)
        lens = np.where(rng.random(len(blocks)) < 0.125, 0, rng.integers(1, 300, len(blocks)))
        t["length"] = lens
        t["offset"] = off + np.concatenate([[0], np.cumsum(lens)[:-1]])
        top = np.array([b.kmax - 1 for b in blocks])
        t["missing_msbs"] = top if constant else np.maximum(top - rng.integers(0, 7, len(blocks)), 0)
        off += int(lens.sum())
        tabs.append(t)
    table = np.concatenate(tabs)
    return table, rng.integers(0, 0x80, max(off, 1)).astype(np.uint8)


def read_back(cs, table, coded):
    info = G.read_header(cs)
    out = G.read_packets(cs, info)
    assert len(out["rows"]) == len(table) == info.num_blocks and len(out["moves"]) == 0
    assert np.array_equal(out["rows"]["length"], table["length"])
    assert np.array_equal(out["rows"]["missing_msbs"], table["missing_msbs"])
    cb = np.frombuffer(cs, np.uint8)
    for i in range(len(table)):
        o, n, t = int(out["rows"][i]["offset"]), int(table[i]["length"]), int(table[i]["offset"])
        assert o + n <= len(cs) and np.array_equal(cb[o:o + n], coded[t:t + n]), i
    return info


CASES = {
    # name: (W, H, tile w, tile h, comps, levels, code-block exponents, precincts, image offset)
    "one tile, precincts, cblk 16": (200, 136, 200, 136, 3, 3, (4, 4), [(7, 7), (7, 7), (6, 6), (5, 5)], (0, 0)),
    "one tile, cblk 4": (77, 53, 77, 53, 1, 2, (2, 2), None, (0, 0)),
    "one tile, cblk 64": (300, 260, 300, 260, 3, 2, (6, 6), None, (0, 0)),
    "2x2 tiles": (256, 256, 128, 128, 3, 3, (5, 5), None, (0, 0)),
    "2x2 ragged tiles off the origin, precincts": (250, 190, 128, 96, 3, 3, (4, 4), [(5, 6), (6, 5), (7, 8), (8, 7)], (5, 3)),
}


# ---- 1. the reader's round trip ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, G.CS_SOP | G.CS_EPH, G.CS_PLT | G.CS_TLM | G.CS_SOP | G.CS_EPH])
@pytest.mark.parametrize("order", [0, 2])
@pytest.mark.parametrize("name", sorted(CASES))
def test_per_block_zero_bit_planes_read_back(name, order, flags):
    """rows with their own missing_msbs -> GRK_AMD_CS_BLOCK_MSBS file -> grk_amd_read_header / grk_amd_read_packets give the rows
    back (missing_msbs, lengths, the bytes at the offsets); a one-tile file is also read by tests/j2kparse.py, which agrees.
    (Without the flag the writer signals Kmax - 1 for every block: the rows would not come back.)"""
    W, H, TW, TH, Cn, L, cblk, prc, off = CASES[name]
    layout = G.ImageLayout.make(W, H, TW, TH, offset=off)
    base = G.TileParams.make(1, 1, Cn, 8, L, cblk=cblk, precincts=prc)
    table, coded = hand_table(layout, base, [len(name), order, flags])
    tops = np.concatenate([[b.kmax - 1 for b in G.tile_layout(p)[0]] for p in G.layout_tiles(layout, base)])
    assert (table["missing_msbs"] != tops).sum() * 2 > len(table) and (table["missing_msbs"] == tops).any()
    fl = flags | G.CS_PROG(order) | MSBS
    cs = G.write_codestream_layout(layout, base, table, coded, fl)
    info = read_back(cs, table, coded)
    assert info.flags == fl & ~MSBS                           # (nothing in the headers says how the trees were made)
    if TW == W and off == (0, 0) and order == 0:              # (what j2kparse reads: one tile, LRCP / RLCP)
        ref = j2kparse.parse(cs)
        rows, cb = j2kparse.decode_table(ref, G.tile_layout(G.layout_tiles(layout, base)[0])[0], False)
        assert [r[1] for r in rows] == list(table["length"]) and [r[2] for r in rows] == list(table["missing_msbs"])
        for (o, n, _), row in zip(rows, table):
            assert cb[o:o + n] == coded[int(row["offset"]):int(row["offset"]) + n].tobytes()


def test_the_writer_without_the_flag_signals_kmax_minus_1():
    """the parent's behaviour, kept: without the flag the rows' missing_msbs are not looked at"""
    W, H, TW, TH, Cn, L, cblk, prc, off = CASES["one tile, precincts, cblk 16"]
    layout = G.ImageLayout.make(W, H, TW, TH, offset=off)
    base = G.TileParams.make(1, 1, Cn, 8, L, cblk=cblk, precincts=prc)
    table, coded = hand_table(layout, base, 5)
    out = G.read_packets(G.write_codestream_layout(layout, base, table, coded, 0))
    assert list(out["rows"]["missing_msbs"]) == [b.kmax - 1 for b in G.tile_layout(G.layout_tiles(layout, base)[0])[0]]


# ---- 2. where the flag changes nothing -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_constant_rows_give_the_same_bytes_with_and_without_the_flag(name):
    W, H, TW, TH, Cn, L, cblk, prc, off = CASES[name]
    layout = G.ImageLayout.make(W, H, TW, TH, offset=off)
    base = G.TileParams.make(1, 1, Cn, 8, L, cblk=cblk, precincts=prc)
    table, coded = hand_table(layout, base, 11, constant=True)
    other = table.copy()
    other["missing_msbs"] = np.random.default_rng(3).integers(0, 30, len(table))
    tiles = G.layout_tiles(layout, base)
    for order in range(5):
        for flags in (0, G.CS_SOP | G.CS_EPH | G.CS_PLT | G.CS_TLM):
            fl = flags | G.CS_PROG(order)
            plain = G.write_codestream_layout(layout, base, table, coded, fl)
            assert G.write_codestream_layout(layout, base, table, coded, fl | MSBS) == plain
            assert G.write_codestream_layout(layout, base, other, coded, fl) == plain       # (flag off: the column is ignored)
            at = 0
            for t, p in enumerate(tiles):
                n = len(G.tile_layout(p)[0])
                part = G.write_tile_part(p, t, table[at:at + n], coded, fl)
                assert G.write_tile_part(p, t, table[at:at + n], coded, fl | MSBS) == part
                assert G.write_tile_part(p, t, table[at:at + n], None, fl | MSBS, size_only=True) == len(part)
                at += n
    if TW == W and off == (0, 0):
        p = tiles[0]
        assert G.write_codestream(p, W, H, table, coded, MSBS) == G.write_codestream(p, W, H, table, coded, 0)
        assert G.write_main_header(p, W, H, MSBS) == G.write_main_header(p, W, H, 0)


def test_the_plan_writer_refuses_the_flag():
    p = G.TileParams.make(128, 128, 1, 8, 2)
    table, _ = hand_table(G.ImageLayout.make(128, 128, 128, 128), G.TileParams.make(1, 1, 1, 8, 2), 1)
    L = G.lib()
    L.grk_amd_plan_tile_part.restype = C.c_int64
    L.grk_amd_plan_tile_part.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                                         C.c_uint64, C.c_void_p]
    nl, ns = C.c_uint64(0), C.c_uint64(0)
    args = (C.addressof(p), 0, MSBS, table.ctypes.data, None, 0, C.addressof(nl), None, 0, C.addressof(ns))
    assert L.grk_amd_plan_tile_part(*args) == ERR_UNSUPPORTED
    assert L.grk_amd_plan_tile_part(*(args[:2] + (0,) + args[3:])) > 0


# ---- 3. the format assumption against the real decoder --------------------------------------------------------------------------
def mixed_drop_file(px, drops):
    """128 x 128 x 1, 2 levels, reversible: every block coded by the oracle as mu >> d under the exponent bound kmax - d
    (orc_ht_encode_sm(sm, kmax - d)), DROP_SKIP blocks left out -> (file, table, the coefficient planes the oracle chain -- orc_ht_decode_block
    -> orc_ht_dequant_rev -- gives for those blocks, the planes whose blocks hold the coarser bins' centres)"""
    p = G.TileParams.make(128, 128, 1, 8, 2, mct=False)
    blocks, _ = G.tile_layout(p)
    assert len(blocks) == len(drops) == 7                        # LL, then HL LH HH of the two resolutions
    mall = O.dwt53_fwd(px[0].astype(np.int32) - 128, 2)
    chain, centres = np.zeros((128, 128), np.int32), np.zeros((128, 128), np.int32)
    table = np.zeros(len(blocks), CODED_DTYPE)
    chunks, off = [], 0
    for i, b in enumerate(blocks):
        bw, bh, d = b.x1 - b.x0, b.y1 - b.y0, drops[i]
        sub = mall[b.py:b.py + bh, b.px:b.px + bw]
        cb = b"" if d == G.DROP_SKIP else O.ht_encode_sm(O.signmag(sub, b.kmax), b.kmax - d)
        mm = b.kmax - 1 if d == G.DROP_SKIP else b.kmax - 1 - d
        table[i] = (off, len(cb), mm)
        chunks.append(cb)
        off += len(cb)
        if cb:
            words = O.ht_decode_block(cb, mm, bw, bh)
            assert words is not None
            # the decoder's words hold the centres: sign << 31 | (2 (mu >> d) + 1) << (p - 1), p = 31 - kmax + d, which the band's
            # shift (k_msbs = kmax - 1) turns into ((mu >> d) << d) + 2^(d - 1)
            q = np.abs(sub) >> d
            centres[b.py:b.py + bh, b.px:b.px + bw] = np.sign(sub) * np.where(q > 0, (q << d) + ((1 << d) >> 1), 0)
            assert np.array_equal(O.ht_dequant_rev(words, b.kmax - 1), centres[b.py:b.py + bh, b.px:b.px + bw])
            # the chain as the reference runs it: ShiftHTFilter shifts by the BLOCK's zero bit-planes (k_msbs = mm)
            chain[b.py:b.py + bh, b.px:b.px + bw] = O.ht_dequant_rev(words, mm)
            assert np.array_equal(chain[b.py:b.py + bh, b.px:b.px + bw], np.sign(sub) * q)
    cs = G.write_codestream(p, 128, 128, table, np.frombuffer(b"".join(chunks), np.uint8), MSBS)
    return cs, table, chain, centres


def pixels_of(mallat):
    return np.clip(O.dwt53_inv(mallat, 2) + 128, 0, 255)


@needs_ref
def test_reference_decoder_reads_mixed_drops_as_the_oracle_chain_does():
    """The reference reads the file -- per-block zero bit-planes, a zero-length block -- and decodes every block's words exactly as
    the oracle's block decoder does; its pixels equal the oracle chain's.
    What this pins about the REVERSIBLE path: the reference's dequantiser (PostDecompressFilters.h ShiftHTFilter) shifts a block's
    words by that block's own zero bit-planes, not by the band's, so a block with d planes dropped comes back as mu >> d instead
    of the coarser bin's centre ((mu >> d) << d) + 2^(d - 1), which the same words hold under the band's shift.  A 9/7 file is
    scaled by the band's step (ScaleHTFilter) and does come back at the centres (tests/test_gpu_rate.py decodes such files)."""
    px = synth.g2(1, 128, 128, 8)
    drops = [0, 3, 1, 2, 1, 2, G.DROP_SKIP]
    cs, table, chain, centres = mixed_drop_file(px, drops)
    assert len(set(table["missing_msbs"])) > 3 and table["length"][-1] == 0 and (table["length"][:-1] > 0).all()
    got = R.decode(cs, 1, 128, 128)
    assert np.array_equal(got[0], pixels_of(chain))
    assert not np.array_equal(got[0], pixels_of(centres))
    # ... and with nothing dropped the chain is the lossless one
    cs0, _, chain0, centres0 = mixed_drop_file(px, [0] * 7)
    assert np.array_equal(chain0, centres0) and np.array_equal(pixels_of(chain0), px[0])
    assert np.array_equal(R.decode(cs0, 1, 128, 128)[0], px[0])


def test_oracle_block_with_d_planes_dropped_decodes_to_the_coarser_bin_centre():
    """orc_ht_encode_sm(sm, kmax - d) read with missing_msbs = kmax - 1 - d: sign << 31 | (2 (mu >> d) + 1) << (p - 1), p = 31 - kmax + d.
    (Magnitudes below 2^(kmax - 2): a decoder refuses a block with a quad exponent above its zero bit-planes, at every d.)"""
    rng = np.random.default_rng(4)
    for w, h, kmax in ((64, 64, 9), (5, 7, 9), (32, 64, 14)):
        mu = rng.integers(0, 1 << (kmax - 2), (h, w))
        neg = rng.random((h, w)) < 0.5
        sm = O.signmag(np.where(neg, -mu, mu), kmax)
        for d in range(5):
            words = O.ht_decode_block(O.ht_encode_sm(sm, kmax - d), kmax - 1 - d, w, h)
            q = mu >> d
            want = np.where(q > 0, (neg.astype(np.int64) << 31) | ((2 * q + 1) << (31 - kmax + d - 1)), 0)
            assert np.array_equal(words.astype(np.int64), want), (w, h, kmax, d)


# ---- 4. host planning ---------------------------------------------------------------------------------------------------------
_units = None


def units():
    global _units
    if _units is None:
        csrc = os.path.join(ROOT, "grok_amd", "csrc")
        out = os.path.join(tempfile.mkdtemp(prefix="rate_plan_units_"), "librate_plan_units.so")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-D_GLIBCXX_ASSERTIONS", "-fPIC", "-shared",
                               os.path.join(HERE, "c", "rate_plan_units.cpp"), os.path.join(csrc, "encode_plan.cpp"),
                               os.path.join(csrc, "geometry.cpp"), "-o", out, "-Wl,--no-undefined", "-lpthread"])
        _units = C.CDLL(out)
        _units.rp_rate.argtypes = [C.c_uint32, C.c_int, C.c_uint64, C.c_void_p]
    return _units


def test_plan_constants():
    k = np.zeros(7, np.uint32)
    units().rp_constants(k.ctypes.data_as(C.c_void_p))
    assert list(k) == [0xFF, 6, 12, 14, 1024, 40, 4] and G.DROP_SKIP == 0xFF


@pytest.mark.parametrize("irrev,h16,want", [(0, 0, (1, 0, 0)), (1, 0, (1, 1, 0)), (0, 1, (1, 0, 1)), (1, 1, (0, 0, 0))])
def test_plan_drop_instance(irrev, h16, want):
    """the instance follows the plane form a non-pipelined encode holds; irreversible int16 planes do not exist"""
    out = np.zeros(3, np.uint32)
    units().rp_drop_instance(irrev, h16, out.ctypes.data_as(C.c_void_p))
    assert tuple(out) == want


@pytest.mark.parametrize("max_drop,skip,n,want", [
    # ok, dmax, rows, ncand, trials, L bytes, E bytes, W bytes, drop bytes
    (0, 0, 1000, (1, 6, 8, 7, 7, 32000, 64000, 8000, 1000)),                 # 0 = the default 6
    (0, 1, 1000, (1, 6, 8, 8, 7, 32000, 64000, 8000, 1000)),                 # SKIP: one more candidate, the same rows
    (1, 1, 3, (1, 1, 3, 3, 2, 36, 72, 24, 3)),
    (12, 1, 49152, (1, 12, 14, 14, 13, 14 * 49152 * 4, 14 * 49152 * 8, 49152 * 8, 49152)),
    (13, 0, 10, (0, 0, 0, 0, 0, 0, 0, 0, 0)),                                # above the limit: refused
])
def test_plan_rate(max_drop, skip, n, want):
    out = np.zeros(9, np.uint64)
    units().rp_rate(max_drop, skip, n, out.ctypes.data_as(C.c_void_p))
    assert tuple(int(v) for v in out) == want


def test_drop_bytes_and_zero_bit_planes():
    u = units()
    assert [u.rp_drop_byte(c, 6) for c in range(8)] == [0, 1, 2, 3, 4, 5, 6, 0xFF]
    for kmax in (1, 2, 9, 14):
        for d in (0, 1, kmax - 1, kmax, 40, 254):
            assert u.rp_missing_msbs(kmax, d) == kmax - 1 - min(d, kmax - 1)       # clamped to kmax - 1
        assert u.rp_missing_msbs(kmax, 0xFF) == kmax - 1                             # SKIP: the all-zero row


# ---- 5. the budgets of a whole-image call's rounds, and the split route's shares of them ----------------------------------------------
def c_shares(budget, samples, plain):
    u = units()
    u.rp_group_shares.argtypes = [C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    s, p, out = np.array(samples, np.uint64), np.array(plain, np.uint64), np.zeros(len(samples), np.uint64)
    u.rp_group_shares(budget, len(samples), s.ctypes.data, p.ctypes.data, out.ctypes.data)
    return [int(v) for v in out]


def shares_restated(budget, samples, plain):
    """group_shares in exact integers: every open group's share is floor(left * samples / open samples); a group whose share reaches
    its plain bytes takes exactly those and closes, and the rest is shared anew; the last open group takes the rounding's remainder --
    unless that lifts it above its own plain bytes, in which case it closes too"""
    n = len(samples)
    share, full = [0] * n, [False] * n
    while True:
        left = budget - sum(share[k] for k in range(n) if full[k])
        opened = [k for k in range(n) if not full[k]]
        total = sum(samples[k] for k in opened)
        if not total:
            return share
        k = next((k for k in opened if left * samples[k] // total >= plain[k]), None)
        if k is None:
            floors = {j: left * samples[j] // total for j in opened[:-1]}
            k = opened[-1]
            if left - sum(floors.values()) <= plain[k]:
                for j, v in floors.items():
                    share[j] = v
                share[k] = left - sum(floors.values())
                return share
        share[k], full[k] = plain[k], True


def check_shares(budget, samples, plain):
    got = c_shares(budget, samples, plain)
    assert got == shares_restated(budget, samples, plain), (budget, samples, plain)
    assert all(g <= p for g, p in zip(got, plain)), (budget, samples, plain, got)
    assert sum(got) == min(budget, sum(plain)), (budget, samples, plain, got)
    if budget >= sum(plain):
        assert got == list(plain)
    return got


def test_group_shares_chosen_cases():
    samples, plain = [64 * 48 * 3, 36 * 48 * 3, 64 * 28 * 3, 36 * 28 * 3], [5000, 3100, 2900, 1700]
    for budget in (sum(plain), sum(plain) + 1, 2 ** 40, 2 ** 64 - 1, sum(plain) - 1, sum(plain) // 2, 1, 0):
        check_shares(budget, samples, plain)
    assert check_shares(4000, samples, [5000, 0, 2900, 1700])[1] == 0              # a group without plain bytes
    assert check_shares(700, [5], [777]) == [700] and check_shares(778, [5], [777]) == [777]      # one group
    assert check_shares(1001, [3, 5, 7], [1000, 1000, 1000]) == [200, 333, 468]    # every floor division inexact
    assert check_shares(5, [1, 1, 1], [2, 2, 2]) == [1, 2, 2]                      # the remainder does not lift the last group above its own
    big = [(1 << 40) + 1, (1 << 41) + 3, 7]                                        # products beyond 2^64
    check_shares((1 << 62) + 12345, big, [1 << 62, 1 << 61, 1 << 60])
    check_shares(2 ** 64 - 1, big, [1 << 62, 1 << 61, 1 << 60])
    check_shares((1 << 63) + 1, [2 ** 63 - 1, 2 ** 62 + 1], [1 << 63, 1 << 62])


def test_group_shares_random_cases():
    """3000 cases of 1 .. 6 groups: sample counts and plain bytes of every magnitude (the sums stay below 2^64, as sums of an image's
    bytes and samples do), budgets around the plain bytes and far from them"""
    rng = np.random.default_rng(11)
    for _ in range(3000):
        n = int(rng.integers(1, 7))
        bits = int(rng.choice([8, 16, 33, 60]))
        samples = [int(rng.integers(1, 1 << int(rng.integers(1, bits + 1)))) for _ in range(n)]
        plain = [int(rng.integers(0, 1 << int(rng.integers(1, bits + 1)))) for _ in range(n)]
        all_ = sum(plain)
        budgets = [0, 1, all_ - 1, all_, all_ + 1, all_ // 2, all_ // 3 + 1, int(rng.integers(0, all_ + 2)), 2 * all_]
        check_shares(max(budgets[int(rng.integers(0, len(budgets)))], 0), samples, plain)


def next_budget(budget, blocks, file_bytes, target):
    u = units()
    u.rp_next_budget.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p]
    out = C.c_uint64(0)
    left = u.rp_next_budget(budget, blocks, file_bytes, target, C.byref(out))
    return int(out.value) if left else None


def test_round_budgets():
    """The first budget: the plain blocks' bytes for a target at or above the plain file, else the target less what the plain file
    spends beside its blocks, 0 where the target does not cover that.  The next: the smaller of the budget and the bytes the round's
    blocks took, less the file's overshoot, down to 0; nothing is left once the budget or the blocks' bytes are 0.
    A round is followed by another only when its file overshoots, by one byte at least: so the budgets never rise, fall by one at
    least per round, and any sequence of overshoots ends in 0 or in "nothing left" after at most the first budget's worth of rounds
    (the library stops after kRateMaxRounds of them)."""
    u = units()
    u.rp_first_budget.restype = C.c_uint64
    u.rp_first_budget.argtypes = [C.c_uint64] * 3
    rng = np.random.default_rng(12)
    for _ in range(3000):
        blocks = int(rng.integers(0, 1 << int(rng.integers(1, 40))))
        plain = blocks + int(rng.integers(1, 5000))
        targets = [0, 1, plain - blocks - 1, plain - blocks, plain - blocks + 1, plain - 1, plain, plain + 1, 2 * plain, int(rng.integers(0, plain + 1))]
        target = targets[int(rng.integers(0, len(targets)))]
        want = blocks if target >= plain else max(target - (plain - blocks), 0)
        assert u.rp_first_budget(target, plain, blocks) == want <= blocks, (target, plain, blocks)
    assert u.rp_first_budget(2 ** 64 - 1, 2 ** 63, 2 ** 63 - 5) == 2 ** 63 - 5
    assert next_budget(500, 480, 640, 600) == 440 and next_budget(500, 480, 2000, 600) == 0 and next_budget(480, 500, 601, 600) == 479
    assert next_budget(0, 0, 640, 600) is None and next_budget(0, 10, 640, 600) is None and next_budget(10, 0, 640, 600) is None
    for _ in range(300):
        budget = first = int(rng.integers(0, 400))
        target = int(rng.integers(50, 1000))
        rounds = 0
        while True:
            blocks = int(rng.integers(0, budget + 1)) if rng.integers(0, 4) == 0 else budget - int(rng.integers(0, budget // 8 + 1))
            over = int(rng.choice([1, 1, 2, int(rng.integers(1, 60))]))
            nxt = next_budget(budget, blocks, target + over, target)
            want = None if budget == 0 or blocks == 0 else max(min(budget, blocks) - over, 0)
            assert nxt == want, (budget, blocks, over)
            if nxt is None:
                break
            assert nxt < budget
            budget = nxt
            rounds += 1
        assert rounds <= first


def test_round_budgets_driver_under_sanitizers():
    """tests/c/rate_plan_units.cpp as a program of its own (its main walks the chosen cases) under AddressSanitizer and UBSan"""
    csrc = os.path.join(ROOT, "grok_amd", "csrc")
    exe = os.path.join(tempfile.mkdtemp(prefix="rate_plan_main_"), "rate_plan_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-D_GLIBCXX_ASSERTIONS", "-DRATE_PLAN_MAIN",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", os.path.join(HERE, "c", "rate_plan_units.cpp"),
                           os.path.join(csrc, "encode_plan.cpp"), os.path.join(csrc, "geometry.cpp"), "-o", exe, "-lpthread"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "0 failure(s)" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, \
        r.stdout + r.stderr
