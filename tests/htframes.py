"""HT cleanup segments framed as encoders other than ours frame them (test helper; no GPU, no conftest).

Every HT code-block this project decodes came out of one encoder algorithm (the oracle's, which is the reference's, which is K3's).
That algorithm makes choices T.814 leaves open: how the MagSgn, MEL and VLC byte streams END and what lies BETWEEN them.  T.814
fixes only what a decoder reads -- MagSgn forwards from byte 0 with ones behind its end, MEL forwards from Lcup - Scup, VLC backwards
from Lcup - 3, 2 <= Scup <= min(Lcup, 4079) -- so everything a decoder does not consume is the encoder's business.

`raw(sm, kmax)` takes a block's quad decisions from the oracle encoder as un-stuffed bit streams (orc_ht_raw_streams) and
`frame(raw, **choices)` packs them into a cleanup segment.  With no choices the bytes are the oracle encoder's
(tests/test_ht_frames_cpu.py holds that for every listed block); every other choice is a framing that decodes to the same samples.

The habit                                   and what else is legal (a choice of `frame`)
  MagSgn  unused bits of the last byte are    magsgn="zeros": they are zeros, nothing dropped (a MagSgn that ends on a complete 0xFF
          ones; a last byte 0xFF is dropped     gets the 0x00 the 7-bit byte behind it is); magsgn="ones-keep": ones, nothing dropped,
          (the decoder feeds 0xFF itself)       a last byte 0xFF gets one 0x00 behind it;  magsgn_spare=k: k zero bytes behind a complete
                                                MagSgn ("zeros" / "ones-keep" only, see below)
  fusing  MEL's last byte and VLC's last      fuse=False: always two bytes
          byte are one byte when their bits
          do not collide
  MEL     unused bits of the last byte are    mel_pad=1: they are ones (0xFE where that would give 0xFF: the segment holds no 0xFF
          zeros                                 followed by a byte above 0x8F); the byte is never fused
  between no byte between MEL and VLC:        gap=k: k zero bytes between them (fuse=False); gap="max": as many as make Scup 4079
          Scup is the smallest possible
The four placeholder bits of the VLC stream (vlc_init's 0xF) end up as Scup's low nibble in either case.

VARIANTS is the named list the tests iterate over, `variant_of(i)` rotates through it.  Share of blocks whose BYTES differ from the
habitual framing, over the 30 blocks of tests/test_ht_frames_cpu.py::BLOCKS (printed there, asserted > 0 for every variant):
    ms-zeros 23/30   ms-ones-keep 3/30   ms-zeros-spare1, ms-ones-keep-spare9, ms-zeros-spare3000 30/30
    never-fused 22/30   mel-ones 29/30   gap1, gap3, gap40, gap-max 30/30   all 30/30
("ones-keep" changes a block only where the habit dropped a 0xFF -- 7 of the 26 coded blocks of the 130 x 67 tile, a tenth to a
quarter elsewhere; the seeds of the GPU cases are chosen so that every variant changes at least one block of every case that uses
it, which test_ht_frames_cpu.py counts.)

Two candidates are NOT conforming and are excluded (EXCLUDED; the CPU tests record that the oracle decodes them to other samples):
  "spare-after-drop"  zero bytes behind a MagSgn whose trailing 0xFF was dropped: the ones the decoder would have synthesised behind
                      the segment's end are now the spare bytes' zeros.
  "mel-unflushed"     the last MEL run left open (no closing 1 bit): the decoder reads the zero pad bits behind it as a "0" codeword,
                      a one event where the run went on -- every listed block with an open run (6 / 30) decodes differently.
"""
import ctypes as C
import numpy as np

import oracle as O

MAX_SCUP = 4079


def raw(sm, kmax):
    """-> the block's streams before framing: {"ms": MagSgn bits (uint8 array, reading order), "vlc": VLC bits (starting with the
    four placeholder ones), "mel": complete MEL bytes, "acc" / "left" / "run": the MEL coder's pending state, "habit": the oracle's
    own bytes}"""
    L = O._bind_model()
    a = np.ascontiguousarray(sm, np.uint32)
    h, w = a.shape
    msw = w * h * 32 // 32 + 8
    vw = 1024 + w * h // 8
    ms = np.zeros(msw, np.uint32)
    vl = np.zeros(vw, np.uint32)
    mel = np.zeros(512 + w * h // 8, np.uint8)
    st = (C.c_int * 4)()
    mb, vb = C.c_uint32(0), C.c_uint32(0)
    n = L.orc_ht_raw_streams(a.ctypes.data, kmax, w, h, ms.ctypes.data, msw, C.byref(mb), vl.ctypes.data, vw, C.byref(vb),
                             mel.ctypes.data, st)
    assert n > 0 and mb.value <= msw * 32 and vb.value <= vw * 32
    bits = lambda words, nb: np.unpackbits(words.view(np.uint8), bitorder="little")[:nb]
    return {"ms": bits(ms, mb.value), "vlc": bits(vl, vb.value), "mel": bytes(mel[:st[0]]), "acc": st[1], "left": st[2],
            "run": st[3], "habit": O.ht_encode_sm(a, kmax)}


def _windows(bits):
    """value of the 8 bits from every position on (LSB first, zeros behind the end) as a list"""
    b = np.concatenate([bits.astype(np.uint32), np.zeros(8, np.uint32)])
    n = len(bits)
    w = np.zeros(n + 1, np.uint32)
    for i in range(8):
        w |= b[i:i + n + 1] << np.uint32(i)
    return w.tolist()


def _pack_magsgn(bits):
    """LSB first, the byte after 0xFF carries 7 bits -> (complete bytes, pending bits, their count, width of the pending byte)"""
    win, n = _windows(bits), len(bits)
    out, pos, limit = bytearray(), 0, 8
    while pos + limit <= n:
        b = win[pos] & ((1 << limit) - 1)
        out.append(b)
        pos += limit
        limit = 7 if b == 0xFF else 8
    used = n - pos
    return out, win[pos] & ((1 << used) - 1), used, limit


def _pack_vlc(bits):
    """LSB first, growing downwards: a byte after one above 0x8F carries 7 bits when those are all ones (the stream starts as if
    behind such a byte) -> (complete bytes in WRITING order, pending bits, their count)"""
    win, n = _windows(bits), len(bits)
    out, pos, prev = [], 0, True
    while True:
        if prev and n - pos >= 7 and (win[pos] & 0x7F) == 0x7F:
            out.append(0x7F); pos += 7; prev = False
        elif n - pos >= 8:
            out.append(win[pos]); pos += 8; prev = win[pos - 8] > 0x8F
        else:
            break
    used = n - pos
    return out, win[pos] & ((1 << used) - 1), used


def _packed(r):
    if "_ms" not in r:
        r["_ms"] = _pack_magsgn(r["ms"])
        r["_vlc"] = _pack_vlc(r["vlc"])
    return r["_ms"], r["_vlc"]


def frame(r, magsgn="ones-drop", magsgn_spare=0, fuse=True, mel_pad=0, gap=0, scup=None, mel_flush=True, spare_after_drop=False):
    """One cleanup segment of the block `r = raw(...)`.  (mel_flush=False and spare_after_drop=True make the two EXCLUDED
    candidates; nothing else should use them.  scup=n: the gap that makes Scup n -- 4080 for a block every decoder must refuse.)"""
    (ms_bytes, ms_acc, ms_used, ms_limit), (vlc_bytes, vlc_acc, vlc_used) = _packed(r)
    # ---- MagSgn
    ms = bytearray(ms_bytes)
    assert magsgn in ("ones-drop", "zeros", "ones-keep")
    assert not magsgn_spare or magsgn != "ones-drop" or spare_after_drop, "spare bytes need a complete MagSgn"
    if magsgn == "zeros":
        if ms_used or ms_limit == 7:
            ms.append(ms_acc)
    else:
        if ms_used:
            b = ms_acc | (((1 << ms_limit) - 1) & ~((1 << ms_used) - 1))
            if b != 0xFF:
                ms.append(b)
            elif magsgn == "ones-keep":
                ms += b"\xff\x00"
        elif ms_limit == 7:
            if magsgn == "ones-keep":
                ms.append(0x00)
            else:
                ms.pop()
    ms += bytes(magsgn_spare)
    # ---- MEL: the pending run, then the last byte
    mel = bytearray(r["mel"])
    acc, left = r["acc"], r["left"]
    if r["run"] > 0 and mel_flush:
        acc = (acc << 1) | 1
        left -= 1
        if left == 0:
            mel.append(acc)
            left = 7 if acc == 0xFF else 8
            acc = 0
    mel_acc, mel_mask = (acc << left) & 0xFF, (0xFF << left) & 0xFF
    vlc_mask = 0xFF >> (8 - vlc_used)
    vlc = list(vlc_bytes)                                     # writing order: the first one is the highest address but one
    if mel_pad:
        fuse = False
        mel_acc |= ~mel_mask & 0xFF
        if mel_acc == 0xFF:
            mel_acc = 0xFE
    if gap or scup is not None:
        assert not fuse, "a gap needs MEL's and VLC's last bytes apart"
    fused = mel_acc | vlc_acc
    if mel_mask | vlc_mask and fuse and ((fused ^ mel_acc) & mel_mask) | ((fused ^ vlc_acc) & vlc_mask) == 0 and fused != 0xFF \
            and len(vlc) > 0:
        mel.append(fused)
    elif mel_mask | vlc_mask or mel_pad:
        mel.append(mel_acc)
        vlc.append(vlc_acc)
    tail = bytes(reversed(vlc)) + b"\xff"
    if gap == "max" or scup is not None:
        gap = (MAX_SCUP if scup is None else scup) - len(mel) - len(tail)
    assert gap >= 0
    out = bytearray(bytes(ms) + bytes(mel) + bytes(gap) + tail)
    n = len(mel) + gap + len(tail)
    out[-1] = n >> 4
    out[-2] = (out[-2] & 0xF0) | (n & 0xF)
    return bytes(out)


def scup_of(cb):
    return (cb[-1] << 4) | (cb[-2] & 0xF)


def obeys_byte_rules(cb):
    """no byte pair above 0xFF8F anywhere in the segment, its last byte is not 0xFF, 2 <= Scup <= min(Lcup, 4079)"""
    a = np.frombuffer(cb, np.uint8)
    pairs_ok = not np.any((a[:-1] == 0xFF) & (a[1:] > 0x8F))
    return bool(pairs_ok) and cb[-1] != 0xFF and 2 <= scup_of(cb) <= min(len(cb), MAX_SCUP)


VARIANTS = [
    ("ms-zeros", dict(magsgn="zeros")),
    ("gap1", dict(fuse=False, gap=1)),
    ("ms-ones-keep", dict(magsgn="ones-keep")),
    ("never-fused", dict(fuse=False)),
    ("ms-zeros-spare1", dict(magsgn="zeros", magsgn_spare=1)),
    ("mel-ones", dict(mel_pad=1)),
    ("gap40", dict(fuse=False, gap=40)),
    ("ms-ones-keep-spare9", dict(magsgn="ones-keep", magsgn_spare=9)),
    ("gap3", dict(fuse=False, gap=3)),
    ("ms-zeros-spare3000", dict(magsgn="zeros", magsgn_spare=3000)),
    ("gap-max", dict(fuse=False, gap="max")),
    ("all", dict(magsgn="zeros", magsgn_spare=2, fuse=False, mel_pad=1, gap=7)),
]
VARIANT_NAMES = [n for n, _ in VARIANTS]
EXCLUDED = [
    ("spare-after-drop", dict(magsgn_spare=2, spare_after_drop=True)),
    ("mel-unflushed", dict(mel_flush=False)),
]


def variant_of(i):
    return VARIANTS[i % len(VARIANTS)]


def choices(name):
    return dict(VARIANTS)[name]


# ---- the blocks and tiles of the tests: built here, on the CPU, so that tests/test_ht_frames_cpu.py can count from the same seeds how
#      many blocks of every GPU case each variant really changes ---------------------------------------------------------------------
MODES = (0, 1, 2, 4)


def block_coef(rng, w, h, kb, mode):
    """the content modes of test_gpu_decode._ht_dec_case, magnitudes <= 2^kb (kb = Kmax - 2: the D5-decodable range)"""
    mag = rng.integers(0, (1 << kb) + 1, size=(h, w))
    if mode == 1:
        mag = mag >> rng.integers(0, kb + 1, size=(h, w))
    elif mode == 2:
        mag = np.where(rng.random((h, w)) < 0.93, 0, mag & 7)
    elif mode == 3:
        mag = np.zeros((h, w), np.int64)
    elif mode == 4:
        mag = np.full((h, w), 1 << kb)
    return (mag * np.where(rng.random((h, w)) < 0.5, -1, 1)).astype(np.int32)


class Item:
    """one code-block of a case: .coef (source samples, or None), .kmax it is coded at, .mm it is decoded at, .raw (None: the block
    is absent), .name / .choices of its framing, .seg / .npasses of a refinement segment"""

    def __init__(self, coef, kmax, r, variant, mm=None, seg=b"", npasses=1):
        self.coef, self.kmax, self.raw, self.mm = coef, kmax, r, kmax - 1 if mm is None else mm
        self.name, self.choices = variant
        self.seg, self.npasses = seg, npasses

    def habit(self):
        return self.raw["habit"]

    def framed(self, variant=None):
        return frame(self.raw, **(self.choices if variant is None else choices(variant)))


# (W, H, L, C, prec, cblk) of the reversible stage_ht_decode cases
REV_GEOMS = [(64, 64, 0, 1, 8, (6, 6)), (130, 67, 2, 3, 8, (6, 6)), (128, 128, 1, 1, 8, (6, 2)), (128, 128, 1, 1, 8, (2, 6)),
             (200, 120, 2, 1, 12, (6, 6))]
CASES = {
    "rev-64x64": dict(kind="tile", geom=REV_GEOMS[0], seed=101, rot=10),            # (its one block: Scup 4079)
    "rev-130x67": dict(kind="tile", geom=REV_GEOMS[1], seed=201),
    "rev-128-cblk64x4": dict(kind="tile", geom=REV_GEOMS[2], seed=302),
    "rev-128-cblk4x64": dict(kind="tile", geom=REV_GEOMS[3], seed=401),
    "rev-200x120-p12": dict(kind="tile", geom=REV_GEOMS[4], seed=558),
    "irrev-256x192": dict(kind="tile", geom=(256, 192, 3, 3, 10, (6, 6)), seed=601, irrev=True),
    "dec16-130x67": dict(kind="tile", geom=(130, 67, 2, 3, 8, (6, 6)), seed=702, cap=10, rot=5),
    "refine-200x120": dict(kind="refine", geom=(200, 120, 2, 3, 8, (6, 6)), seed=802),
    "mm-130x67": dict(kind="mm", geom=(130, 67, 2, 3, 8, (6, 6)), seed=902),
    "image-96x160": dict(kind="image", seed=0, rot=1),
}
_built = {}


def build_case(name):
    """-> (TileParams, blocks, qcd, [Item]); built once per process"""
    if name not in _built:
        _built[name] = _build(**CASES[name])
    return _built[name]


def _build(kind, seed, geom=None, rot=0, irrev=False, cap=None):
    import grok_amd as G
    rng = np.random.default_rng(seed)
    if kind == "image":
        import chain
        import synth
        px = synth.g2(3, 96, 160, 8)
        p, blocks, qcd, table, coded = chain.encode_tile_oracle(px, 8, 4)
        items = []
        for i, b in enumerate(blocks):
            o, n = int(table["offset"][i]), int(table["length"][i])
            bw, bh = b.x1 - b.x0, b.y1 - b.y0
            coef = O.ht_dequant_rev(O.ht_decode_block(coded[o:o + n], b.kmax - 1, bw, bh), b.kmax - 1)
            r = raw(O.signmag(coef, b.kmax), b.kmax)
            assert r["habit"] == coded[o:o + n]
            items.append(Item(coef, b.kmax, r, variant_of(i + rot)))
        return p, blocks, qcd, items
    W, H, L, C, prec, cblk = geom
    p = G.TileParams.make(W, H, C, prec, L, irreversible=irrev, cblk=cblk)
    blocks, qcd = G.tile_layout(p)
    items = []
    for i, b in enumerate(blocks):
        bw, bh = b.x1 - b.x0, b.y1 - b.y0
        mode = MODES[(i + i // len(VARIANTS)) % 4]
        var = variant_of(i + rot)
        if kind == "tile":
            kb = b.kmax - 2 if cap is None else min(b.kmax - 2, cap)
            coef = block_coef(rng, bw, bh, kb, mode)
            r = raw(O.signmag(coef, b.kmax), b.kmax) if i % 7 != 6 else None           # every 7th block is absent
            if r is None:
                coef = np.zeros_like(coef)
            items.append(Item(coef, b.kmax, r, var))
        elif kind == "mm":                       # coded at its own kb, decoded at missing_msbs from kb - 1 to 29
            kb = int(rng.integers(3, 19))
            mm = (kb - 1, 29, int(rng.integers(kb - 1, 30)))[min(i % 5, 2)]
            coef = block_coef(rng, bw, bh, kb - 2, mode)
            items.append(Item(coef, kb, raw(O.signmag(coef, kb), kb), var, mm=mm))
        elif kind == "refine":                   # the cleanup segment of test_oracle_ht_refine.code_block, framed, + its refinement segment
            from test_oracle_ht_refine import make_block
            npasses = 2 + (i + i // len(VARIANTS)) % 2
            mag, sign = make_block(rng, bw, bh, min(b.kmax, 14), int(rng.integers(0, 5)))
            mu = (mag >> 1).astype(np.uint32)
            sm = np.where(mu == 0, 0, (sign.astype(np.uint32) << 31) | (mu << np.uint32(30 - b.kmax))).astype(np.uint32)
            seg, _ = O.ht_refine_encode(mag, sign, npasses)
            items.append(Item(None, b.kmax, raw(sm, b.kmax), var, seg=seg, npasses=npasses))
    return p, blocks, qcd, items


def changed_per_variant(items, variant=None):
    """{variant name: (blocks framed that way whose bytes differ from the habitual framing, blocks framed that way)}"""
    out = {}
    for it in items:
        if it.raw is None:
            continue
        n = it.name if variant is None else variant
        c, t = out.get(n, (0, 0))
        out[n] = (c + (it.framed(variant) != it.habit()), t + 1)
    return out
