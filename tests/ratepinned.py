"""What tests/test_gpu_rate_pinned.py pins of the rate- and quality-targeted encodes, and how it is computed: CASES maps a case's name
to a function of a context that makes one call and returns everything deterministic about it as JSON values.  The fixture
tests/golden/rate_pinned.json holds these records as a known-good library gave them (tools/rate_pinned_record.py writes it).

3 components, 8 bits, 2 levels, 32 x 32 code-blocks, Dmax 6.  Whole-image calls: the sha256 of the file, the result struct (doubles as
hex floats), the text grk_amd_last_error leaves, and afterwards rate_num_blocks, rate_unit_rows, rate_last_budget,
quality_last_budget and a sha256 of each of the four rate_tables.  Tile calls: per row the length, the missing_msbs and a sha256 of the
row's bytes (no arena offsets: their order is not fixed), the result and the same state."""
import hashlib
import os

import numpy as np

import grok_amd as G
import packedref as PR
import synth
from test_t2_reader_subsampled_cpu import make_planes

DMAX, LEVELS, CBLK = 6, 2, (5, 5)
S420 = [(1, 1), (2, 2), (2, 2)]
KW = dict(max_drop=DMAX, allow_skip=True)
XF = {"5/3": False, "9/7": True}


def sha(a):
    return hashlib.sha256(a if isinstance(a, bytes) else np.ascontiguousarray(a).tobytes()).hexdigest()


def fields(res):
    return {name: float(v).hex() if isinstance(v, float) else int(v)
            for name, v in ((f[0], getattr(res, f[0])) for f in res._fields_ if f[0] != "reserved")}


def state(c):
    """what the accessors answer after a call (tables and unit rows: None where the call left none)"""
    n = c.rate_num_blocks()
    return {"rate_num_blocks": n, "rate_last_budget": c.rate_last_budget(), "quality_last_budget": float(c.quality_last_budget()).hex(),
            "rate_unit_rows": [int(v) for v in c.rate_unit_rows()] if n else None,
            "rate_tables": [sha(t) for t in c.rate_tables(n, DMAX)] if n else None}


def whole(c, call):
    try:
        cs, res = call()
        out = {"code": 0, "file": sha(cs), "file_bytes": len(cs), "result": fields(res)}
    except G.RateError as e:
        out = {"code": e.code, "file": None, "file_bytes": None, "result": None}
    out["last_error"] = c.last_error()
    out.update(state(c))
    return out


def plain_host(call):
    """the plain file as the host writer makes it: what the byte targets are fractions of"""
    keep = os.environ.get("GRK_AMD_IMAGE_T2")
    os.environ["GRK_AMD_IMAGE_T2"] = "host"
    try:
        return call()
    finally:
        if keep is None:
            del os.environ["GRK_AMD_IMAGE_T2"]
        else:
            os.environ["GRK_AMD_IMAGE_T2"] = keep


def clip(a):
    return np.clip(a, 32, 224).astype(a.dtype)


# byte targets: (numerator, denominator) of the plain file, or an absolute count below the headers
BYTES = {"2x": (2, 1), "1/2": (1, 2), "1/4": (1, 4), "below headers": 60}
# quality targets: (psnr, distortion)
QUALITY = {"35dB": (35.0, 0.0), "50dB": (50.0, 0.0), "D0": (0.0, 0.0)}
TILINGS = {"ragged": (64, 48), "one tile": (100, 76)}
CASES = {}


def target_of(plain, t):
    return t if isinstance(t, int) else len(plain) * t[0] // t[1]


def image_case(tiling, xf, joint=None, bytes_=None, quality=None):
    def run(c):
        TW, TH = TILINGS[tiling]
        layout = G.ImageLayout.make(100, 76, TW, TH)
        base = G.TileParams.make(TW, TH, 3, 8, LEVELS, irreversible=XF[xf], cblk=CBLK)
        px = clip(synth.g2(3, 76, 100, 8))
        if quality:
            return whole(c, lambda: c.encode_image_quality(layout, base, px, *QUALITY[quality], **KW))
        target = target_of(plain_host(lambda: c.encode_image(layout, base, px)), BYTES[bytes_])
        return dict(whole(c, lambda: c.encode_image_rate(layout, base, px, target, joint=joint, **KW)), target=target)
    return run


def frame_case(kind, xf, bytes_=None, quality=None):
    """kind: "420" (the 100 x 76 image in tiles of 64 x 48, tight planes), "NV12" and "YUY2" (64 x 48, one tile)"""
    def run(c):
        W, H, tile = (100, 76, (64, 48)) if kind == "420" else (64, 48, (64, 48))
        sampling = S420 if kind != "YUY2" else [(1, 1), (2, 1), (2, 1)]
        layout = G.ImageLayout.make(W, H, *tile)
        base = G.TileParams.make(1, 1, 3, 8, LEVELS, mct=False, irreversible=XF[xf], cblk=CBLK)
        planes = [clip(p) for p in make_planes(layout, sampling, 8, seed=9)]
        if kind == "420":
            plain = lambda: c.encode_image_subsampled(layout, base, sampling, planes)
            rate = lambda t: c.encode_image_subsampled_rate(layout, base, sampling, planes, t, **KW)
            qual = lambda p, d: c.encode_image_subsampled_quality(layout, base, sampling, planes, p, d, **KW)
        elif kind == "NV12":
            surface, samp, nbytes = G.Surface.make(kind, layout, pitch=W + 14)
            buf = np.random.default_rng(3).integers(0, 256, nbytes, dtype=np.uint8)
            surface.scatter(buf, planes, 1)
            plain = lambda: c.encode_surface(layout, base, sampling, surface, buf)
            rate = lambda t: c.encode_surface_rate(layout, base, sampling, surface, buf, t, **KW)
            qual = lambda p, d: c.encode_surface_quality(layout, base, sampling, surface, buf, p, d, **KW)
        else:
            frame = PR.pack(PR.YUY2, 8, *planes, 0, np.random.default_rng(4).integers(0, 256, PR.frame_bytes(PR.YUY2, W, H, 0), dtype=np.uint8))
            plain = lambda: c.encode_packed(layout, base, "YUY2", frame)
            rate = lambda t: c.encode_packed_rate(layout, base, "YUY2", frame, t, **KW)
            qual = lambda p, d: c.encode_packed_quality(layout, base, "YUY2", frame, p, d, **KW)
        if quality:
            return whole(c, lambda: qual(*QUALITY[quality]))
        target = target_of(plain_host(plain), BYTES[bytes_])
        return dict(whole(c, lambda: rate(target)), target=target)
    return run


def tiles_case(xf, goal, skip):
    """2 tiles of 64 x 48: half the plain blocks' bytes, or 35 dB"""
    def run(c):
        p = G.TileParams.make(64, 48, 3, 8, LEVELS, irreversible=XF[xf], cblk=CBLK)
        px = np.stack([clip(synth.g2(3, 48, 64, 8, seed=s)) for s in (1, 2)])
        out = {}
        if goal == "rate":
            plain, _ = c.encode_tiles(p, 2, px.ctypes.data, False)
            out["target"] = int(plain["length"].sum()) // 2
            table, tot, res = c.encode_tiles_rate(p, 2, px.ctypes.data, False, out["target"], DMAX, skip)
        else:
            table, tot, res = c.encode_tiles_quality(p, 2, px.ctypes.data, False, 35.0, max_drop=DMAX, allow_skip=skip)
        out["last_error"] = c.last_error()
        coded = c.fetch_coded(tot)
        out["rows"] = [[int(r["length"]), int(r["missing_msbs"]), sha(coded[int(r["offset"]):int(r["offset"]) + int(r["length"])])] for r in table]
        out["result"] = fields(res)
        out.update(state(c))
        return out
    return run


for _xf in XF:
    for _tiling in TILINGS:
        for _joint in (0, 1):
            for _b in BYTES:
                CASES["image %s %s joint%d %s" % (_tiling, _xf, _joint, _b)] = image_case(_tiling, _xf, joint=_joint, bytes_=_b)
        for _q in QUALITY:
            CASES["image %s %s quality %s" % (_tiling, _xf, _q)] = image_case(_tiling, _xf, quality=_q)
    for _kind in ("420", "NV12", "YUY2"):
        CASES["%s %s 1/2" % (_kind, _xf)] = frame_case(_kind, _xf, bytes_="1/2")
        CASES["%s %s quality 35dB" % (_kind, _xf)] = frame_case(_kind, _xf, quality="35dB")
    for _goal in ("rate", "quality"):
        for _skip in (True, False):
            CASES["tiles %s %s %s" % (_xf, _goal, "skip" if _skip else "noskip")] = tiles_case(_xf, _goal, _skip)


def record(c):
    return {name: run(c) for name, run in CASES.items()}
