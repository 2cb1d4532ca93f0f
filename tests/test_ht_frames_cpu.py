"""CPU: tests/htframes.py, the framer that writes HT cleanup segments the way encoders other than ours may (T.814 leaves the ends of
the MagSgn, MEL and VLC streams and what lies between them to the encoder).  Its habitual framing is the oracle encoder's, byte for
byte; every variant in htframes.VARIANTS decodes through the oracle decoder -- and, where oracle/_ref is built, through the
reference's own (ojph_decode_codeblock) -- to the habitual framing's words; the two candidates that are not conforming are recorded
as such.  tests/test_gpu_ht_frames.py then holds the HIP decoder to the same variants; that every variant really changes bytes in
every one of its cases is counted here, from the same seeds.  (No variant had to be dropped: the oracle and the reference agree on
all of them.)"""
import numpy as np
import pytest

import htframes as F
import oracle as O
import refharness as R

needs_ref = pytest.mark.skipif(not R.have_ref(), reason="oracle/_ref (the real reference) not built here")

# (w, h, Kmax, content mode of test_gpu_decode._ht_dec_case, seed): 7 sizes x the modes 0, 1, 2, 4 + two empty blocks (mode 3)
SIZES = [(64, 64), (64, 4), (4, 64), (37, 3), (1, 1), (63, 31), (32, 32)]
BLOCKS = [(w, h, 5 + (si * 4 + mi) * 3 % 16, mode, 10 * si + mi) for si, (w, h) in enumerate(SIZES) for mi, mode in enumerate(F.MODES)] + \
    [(64, 64, 9, 3, 90), (5, 7, 14, 3, 91)]
_cache = {}


def _block(k):
    """-> (source samples, raw streams, the oracle's decode of the habitual framing)"""
    if k not in _cache:
        w, h, kmax, mode, seed = BLOCKS[k]
        coef = F.block_coef(np.random.default_rng(seed), w, h, kmax - 2, mode)
        r = F.raw(O.signmag(coef, kmax), kmax)
        _cache[k] = (coef, r, O.ht_decode_block(r["habit"], kmax - 1, w, h))
    return _cache[k]


def test_block_list_covers_what_it_says():
    assert {(64, 64), (64, 4), (4, 64), (37, 3), (1, 1), (63, 31)} <= {b[:2] for b in BLOCKS}
    assert {b[3] for b in BLOCKS} == {0, 1, 2, 3, 4}
    assert min(b[2] for b in BLOCKS) == 5 and max(b[2] for b in BLOCKS) == 20


def test_habitual_framing_is_the_oracle_encoder():
    for k, (w, h, kmax, mode, _) in enumerate(BLOCKS):
        coef, r, base = _block(k)
        assert F.frame(r) == r["habit"] == O.ht_encode_sm(O.signmag(coef, kmax), kmax), BLOCKS[k]
        assert base is not None and np.array_equal(O.ht_dequant_rev(base, kmax - 1), coef), BLOCKS[k]
        assert F.obeys_byte_rules(r["habit"])


@pytest.mark.parametrize("name", F.VARIANT_NAMES)
def test_variant_decodes_to_the_habitual_framings_words(name):
    changed = 0
    for k, (w, h, kmax, mode, _) in enumerate(BLOCKS):
        coef, r, base = _block(k)
        cb = F.frame(r, **F.choices(name))
        got = O.ht_decode_block(cb, kmax - 1, w, h)
        assert got is not None and np.array_equal(got, base), BLOCKS[k]
        assert np.array_equal(O.ht_dequant_rev(got, kmax - 1), coef), BLOCKS[k]
        assert len(cb) <= 48 << 10                                   # (the HIP decoder's limit for one block)
        changed += cb != r["habit"]
    print("%s: changes %d / %d blocks" % (name, changed, len(BLOCKS)))
    assert changed > 0


@needs_ref
@pytest.mark.parametrize("name", F.VARIANT_NAMES)
def test_variant_decodes_the_same_through_the_reference_decoder(name):
    for k, (w, h, kmax, mode, _) in enumerate(BLOCKS):
        coef, r, base = _block(k)
        assert np.array_equal(R.ht_decode_block(F.frame(r, **F.choices(name)), kmax - 1, w, h), base), BLOCKS[k]


@pytest.mark.parametrize("name", F.VARIANT_NAMES)
def test_variant_obeys_the_byte_rules(name):
    """no byte pair above 0xFF8F, the last byte is not 0xFF, 2 <= Scup <= min(Lcup, 4079) -- and the choice did what its name says"""
    ch = F.choices(name)
    for k in range(len(BLOCKS)):
        _, r, _ = _block(k)
        cb, hb = F.frame(r, **ch), r["habit"]
        assert F.obeys_byte_rules(cb), BLOCKS[k]
        if ch.get("gap") == "max":
            assert F.scup_of(cb) == 4079
        elif ch.get("gap"):
            assert F.scup_of(cb) >= F.scup_of(hb) + ch["gap"]
        if ch.get("magsgn_spare"):
            ms = len(cb) - F.scup_of(cb)
            assert ms >= ch["magsgn_spare"] and cb[ms - ch["magsgn_spare"]:ms] == bytes(ch["magsgn_spare"])


def test_scup_4079_decodes_and_4080_is_refused():
    for k, (w, h, kmax, mode, _) in enumerate(BLOCKS):
        _, r, base = _block(k)
        top, over = F.frame(r, fuse=False, scup=4079), F.frame(r, fuse=False, scup=4080)
        assert F.scup_of(top) == 4079 and F.scup_of(over) == 4080 and len(over) == len(top) + 1
        assert np.array_equal(O.ht_decode_block(top, kmax - 1, w, h), base)
        assert O.ht_decode_block(over, kmax - 1, w, h) is None


@needs_ref
def test_scup_4080_is_refused_by_the_reference_decoder():
    for k, (w, h, kmax, mode, _) in enumerate(BLOCKS):
        _, r, base = _block(k)
        assert np.array_equal(R.ht_decode_block(F.frame(r, fuse=False, scup=4079), kmax - 1, w, h), base)
        with pytest.raises(RuntimeError):
            R.ht_decode_block(F.frame(r, fuse=False, scup=4080), kmax - 1, w, h)


@pytest.mark.parametrize("name", [n for n, _ in F.EXCLUDED])
def test_excluded_candidates_are_not_conforming(name):
    """why these two are not in VARIANTS: on at least one listed block the oracle decodes them to OTHER words than the habitual
    framing's (or refuses them)"""
    differ, changed = [], 0
    for k, (w, h, kmax, mode, _) in enumerate(BLOCKS):
        _, r, base = _block(k)
        cb = F.frame(r, **dict(F.EXCLUDED)[name])
        changed += cb != r["habit"]
        got = O.ht_decode_block(cb, kmax - 1, w, h)
        if got is None or not np.array_equal(got, base):
            differ.append(BLOCKS[k])
    print("%s: changes %d blocks, %d of them decode differently" % (name, changed, len(differ)))
    assert differ and changed >= len(differ)


@needs_ref
@pytest.mark.parametrize("name", [n for n, _ in F.EXCLUDED])
def test_excluded_candidates_decode_differently_through_the_reference_too(name):
    differ = 0
    for k, (w, h, kmax, mode, _) in enumerate(BLOCKS):
        _, r, base = _block(k)
        try:
            got = R.ht_decode_block(F.frame(r, **dict(F.EXCLUDED)[name]), kmax - 1, w, h)
        except RuntimeError:
            got = None
        differ += got is None or not np.array_equal(got, base)
    assert differ > 0


# ---- non-vacuity of tests/test_gpu_ht_frames.py: counted here, from the seeds it uses -----------------------------------------------
@pytest.mark.parametrize("case", sorted(F.CASES))
def test_every_variant_changes_bytes_in_every_gpu_case(case):
    """every variant the rotation hands to a block of the case changes the bytes of at least one such block (a 64 x 64 tile has one
    block and so one variant; together the rotating cases use every variant)"""
    p, blocks, qcd, items = F.build_case(case)
    ch = F.changed_per_variant(items)
    print(case, ch)
    assert ch and all(c > 0 for c, _ in ch.values()), ch
    for it in items:
        if it.raw is not None:
            assert F.obeys_byte_rules(it.framed()) and len(it.framed()) <= 48 << 10
    if len(items) >= 2 * len(F.VARIANTS):
        assert set(ch) == set(F.VARIANT_NAMES)


@pytest.mark.parametrize("name", F.VARIANT_NAMES)
def test_every_variant_changes_bytes_when_the_whole_tile_is_framed_that_way(name):
    """the 130 x 67 tile, one call per variant with every block in that variant"""
    c, t = F.changed_per_variant(F.build_case("rev-130x67")[3], name)[name]
    print(name, c, t)
    assert c > 0


def test_cases_decode_to_their_sources_through_the_oracle():
    """what the GPU tests expect of every case: the framed block decodes at its missing_msbs to the source samples"""
    for case in F.CASES:
        for it in F.build_case(case)[3]:
            if it.raw is None or it.coef is None:
                continue
            h, w = it.coef.shape
            got = O.ht_decode_block(it.framed(), it.mm, w, h)
            assert got is not None and np.array_equal(O.ht_dequant_rev(got, it.mm), it.coef), (case, it.name)
