"""One case per row of the DWT and egress kernels' instance lists (grok_amd/csrc/dwt_instances.h), at the smallest shape that selects
the row.  Every case first asks the CPU planner drivers (tests/c/*_plan_units.cpp, no GPU) for the instance its parameters map to --
test_case_selects_its_instance runs without a GPU as well --, then runs the call that launches it:
  * reversible: encode, decode, the pixels are the input's;
  * 9/7 encode: the blocks are the oracle chain's (chain.encode_tile_oracle); in a layout of the caller's also the default layout's;
  * 9/7 decode: the pixels of the same call with the stand-alone egress kernel (GRK_AMD_FUSE_EGRESS=0), exactly -- what
    tests/test_gpu_decode.py asks of fused against separate.
Shapes: 34 x 18 with two levels for the 32-bit kernels (even: the all-fast forms), 33 x 17 for the general forms, 256 x 16 with one
level for the packed kernels (2052 x 16: 256 lanes); 512 x 32 / 4104 x 32 with two levels put a packed level between planes.

Rows no call reaches (NO_CASE): int16 planes exist for samples of at most 8 bits, so their 16-bit-pixel forms of the fused inverse
level never run, and samples have at most 16 bits, so the stand-alone egress never writes int32.  The lists keep them: the set of
instantiated kernels is what it was."""
import os

import numpy as np
import pytest

import grok_amd as G
import pixlayout as X
import synth
import test_decode_plan_cpu as DP
import test_encode_plan_cpu as EP

IL, RGBX = dict(interleaved=True), dict(interleaved=True, channels=4)
P16, DEC_P16 = {"GRK_AMD_PLANES16": "0"}, {"GRK_AMD_DEC_PLANES16": "0"}
SENTINEL = 0xA5


def case(kind, key, W, H, C, prec, L, irrev=False, mct=None, lay=None, env=None, level=0):
    return dict(kind=kind, key=key, W=W, H=H, C=C, prec=prec, L=L, irrev=irrev, mct=C >= 3 if mct is None else mct, lay=lay, env=env or {},
                level=level)


def _cases():
    out = []
    sizes = ((34, 18, 0), (33, 17, 1))                 # (W, H, GEN)
    # ---- dwt_level_kernel<F97, NC, PX, H16, GEN, STR>
    out += [case("enc", ("k", 1, 1, 0, 0, 1, 0), 34, 18, 1, 8, 2, irrev=True, level=1),
            case("enc", ("k", 0, 1, 0, 1, 1, 0), 34, 18, 1, 8, 2, level=1),
            case("enc", ("k", 0, 1, 0, 0, 1, 0), 34, 18, 1, 12, 2, level=1)]
    for nc, (px, prec) in ((nc, pp) for nc in (3, 1) for pp in ((1, 8), (2, 12))):
        out.append(case("enc", ("k", 1, nc, px, 0, 1, 1), 34, 18, nc, prec, 2, irrev=True, lay=IL))
        for W, H, gen in sizes:
            out.append(case("enc", ("k", 1, nc, px, 0, gen, 0), W, H, nc, prec, 2, irrev=True))
            out.append(case("enc", ("k", 0, nc, px, 0, gen, 0), W, H, nc, prec, 2, env=P16 if px == 1 else None))
        out.append(case("enc", ("k", 0, nc, px, 0, 1, 1), 34, 18, nc, prec, 2, lay=IL, env=P16 if px == 1 else None))
    for nc in (3, 1):
        out.append(case("enc", ("k", 0, nc, 1, 1, 1, 1), 34, 18, nc, 8, 2, lay=IL))
        out.append(case("enc", ("k", 0, nc, 1, 1, 1, 0), 34, 18, nc, 8, 2))
    # ---- dwt53_pk_kernel<NC, PX, NT, CH>
    out += [case("enc", ("pk", 1, 0, 128, 0), 512, 32, 1, 8, 2, level=1), case("enc", ("pk", 1, 0, 256, 0), 4104, 32, 1, 8, 2, level=1)]
    for nt, W in ((128, 256), (256, 2052)):
        out += [case("enc", ("pk", 1, 1, nt, 1), W, 16, 1, 8, 1, lay=IL), case("enc", ("pk", 3, 1, nt, 3), W, 16, 3, 8, 1, lay=IL),
                case("enc", ("pk", 1, 1, nt, 3), W, 16, 3, 8, 1, mct=False, lay=IL), case("enc", ("pk", 3, 1, nt, 4), W, 16, 3, 8, 1, lay=RGBX),
                case("enc", ("pk", 1, 1, nt, 4), W, 16, 4, 8, 1, lay=IL), case("enc", ("pk", 3, 1, nt, 0), W, 16, 3, 8, 1),
                case("enc", ("pk", 1, 1, nt, 0), W, 16, 1, 8, 1)]
    # ---- idwt_level_kernel<F97, NC, PXO, H16, STR>
    out += [case("dec", ("k", 1, 1, 0, 0, 0), 34, 18, 1, 8, 2, irrev=True, level=1),
            case("dec", ("k", 0, 1, 0, 1, 0), 34, 18, 1, 8, 2, level=1),
            case("dec", ("k", 0, 1, 0, 0, 0), 34, 18, 1, 12, 2, level=1)]
    for nc, (pxo, prec), lay in ((nc, pp, lay) for nc in (3, 1) for pp in ((1, 8), (2, 12)) for lay in (None, IL)):
        str_ = 1 if lay else 0
        out.append(case("dec", ("k", 1, nc, pxo, 0, str_), 34, 18, nc, prec, 2, irrev=True, lay=lay))
        out.append(case("dec", ("k", 0, nc, pxo, 0, str_), 33, 17, nc, prec, 2, lay=lay, env=DEC_P16 if pxo == 1 else None))
        if pxo == 1:
            out.append(case("dec", ("k", 0, nc, 1, 1, str_), 34, 18, nc, 8, 2, lay=lay))
    # ---- idwt53_pk_kernel<NC, PXO, CH>
    out += [case("dec", ("pk", 1, 0, 0), 512, 32, 1, 8, 2, level=1), case("dec", ("pk", 1, 1, 1), 256, 16, 1, 8, 1, lay=IL),
            case("dec", ("pk", 3, 1, 3), 256, 16, 3, 8, 1, lay=IL), case("dec", ("pk", 3, 1, 4), 256, 16, 3, 8, 1, lay=RGBX),
            case("dec", ("pk", 3, 1, 0), 256, 16, 3, 8, 1), case("dec", ("pk", 1, 1, 0), 256, 16, 1, 8, 1)]
    # ---- egress_kernel<PIX, NC, STR>: a tile without a DWT level leaves through the stand-alone kernel
    for (b, prec), nc, lay in ((bp, nc, lay) for bp in ((1, 8), (2, 12)) for nc in (1, 2, 3, 4) for lay in (None, IL)):
        out.append(case("egress", (b, nc, 1 if lay else 0), 33, 17, nc, prec, 0, lay=lay))
    return out


CASES = _cases()
NO_CASE = [("k", 0, nc, 2, 1, str_) for nc in (3, 1) for str_ in (0, 1)] + [(4, nc, 0) for nc in (1, 2, 3, 4)]


def case_id(c):
    return "%s-%s-%dx%dx%d-p%d%s%s" % (c["kind"], "_".join(str(v) for v in c["key"]), c["W"], c["H"], c["C"], c["prec"],
                                       "-il%d" % c["lay"].get("channels", c["C"]) if c["lay"] else "", "".join("-" + k[8:] for k in c["env"]))


def params(c):
    return G.TileParams.make(c["W"], c["H"], c["C"], c["prec"], c["L"], irreversible=c["irrev"], mct=c["mct"])


def layout(c):
    return G.PixelLayout.make(True, c["lay"].get("channels", 0)) if c["lay"] else None


def planned_instance(c):
    """the descriptor run_dwt / run_idwt / run_egress make of the case's level, through the planners"""
    p, bps = params(c), (c["prec"] + 7) // 8
    l = c["level"]
    cw, ch = -(-c["W"] >> l), -(-c["H"] >> l)
    chan = c["lay"].get("channels", c["C"]) if c["lay"] else 0
    px = dict(px_lay=2, px_chan=chan, px_row=c["W"] * chan * bps) if c["lay"] and l == 0 else {}
    part = 3 if c["mct"] and c["key"][0] == "pk" and c["key"][1] == 3 or c["key"][0] == "k" and c["key"][2] == 3 else 1
    env = dict(dict(GRK_AMD_PLANES16="1", GRK_AMD_DEC_PLANES16="1", GRK_AMD_DWT_PK="1", GRK_AMD_FUSE_EGRESS="1"), **c["env"])
    if c["kind"] == "enc":
        h16 = env["GRK_AMD_PLANES16"] == "1" and bool(EP.lib().ep_planes16_ok(EP.C.byref(p)))
        pk = h16 and env["GRK_AMD_DWT_PK"] == "1" and bool(EP.lib().ep_pk16_level_ok(EP.C.byref(p), l))
        return EP.level_inst(part, cw, ch, h16=h16, pk=pk, irreversible=c["irrev"], fused=l == 0, px_bytes=bps, **px)
    if c["kind"] == "dec":
        h16 = env["GRK_AMD_DEC_PLANES16"] == "1" and env["GRK_AMD_FUSE_EGRESS"] == "1" and not c["irrev"] and c["prec"] <= 8
        pk = h16 and env["GRK_AMD_DWT_PK"] == "1"
        if px:
            px["px_tile"] = px["px_row"] * c["H"]
        return DP.idwt(cw, ch, h16=h16, pk=pk, irreversible=c["irrev"], fused=l == 0, px_bytes=bps, lo=0, hi=(1 << c["prec"]) - 1, mct=c["mct"],
                       **px)["inst"][part == 3][0]
    out = np.zeros(3, np.uint32)
    DP.lib().dp_egress_key(2 if c["lay"] else 0, bps, c["C"], DP.ptr(out))
    return tuple(int(v) for v in out)


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_case_selects_its_instance(c):
    assert planned_instance(c) == c["key"]


def test_every_row_has_a_case():
    fk, fpk = EP.instance_tables()
    ik, ipk, eg = DP.idwt_tables()
    for kind, rows in (("enc", fk + fpk), ("dec", ik + ipk), ("egress", eg)):
        have = [c["key"] for c in CASES if c["kind"] == kind]
        assert len(have) == len(set(have))
        assert sorted(have + [r for r in NO_CASE if r in rows]) == sorted(rows), kind
    assert all(r in ik + eg for r in NO_CASE)


# ---- on the GPU ----------------------------------------------------------------------------------------------------------------
_ctxs = {}


def ctx(env=None):
    """a context per set of environment switches (they are read when a context is made), kept for the file"""
    key = tuple(sorted((env or {}).items()))
    if key not in _ctxs:
        keep = {k: os.environ.get(k) for k, _ in key}
        os.environ.update(dict(key))
        try:
            _ctxs[key] = G.Context(0)
        finally:
            for k, v in keep.items():
                if v is None:
                    os.environ.pop(k)
                else:
                    os.environ[k] = v
    return _ctxs[key]


def content(c):
    """The transformed 34 x 18 and 33 x 17 tiles: structure plus noise, as tests/test_gpu_pixel_layout.py codes it.  The packed kernels'
    shapes and the tiles without a DWT level: low-contrast ramps in every component -- they keep every coefficient inside the packed
    inverse transform's +-2047, and busy content in 8-row code-blocks or in untransformed RCT chroma is refused by the HT block decoder
    (as it is at the parent of this file's commit: the block coders' matter, not the transform's or the egress's, whose arithmetic is
    as exact on ramps)."""
    C, H, W, prec = c["C"], c["H"], c["W"], c["prec"]
    if W >= 256 or c["kind"] == "egress":
        yy, xx = np.mgrid[0:H, 0:W]
        px = np.stack([100 + 7 * k + ((xx // (5 + k)) + (yy // 3)) % 23 for k in range(C)]) << (prec - 8)
        return px.astype(np.uint8 if prec <= 8 else np.uint16)[None]
    rng = np.random.default_rng(W + 31 * H + C)
    px = synth.g2(C, H, W, prec, seed=7).astype(np.int64)
    px = (px + rng.integers(0, 1 << max(prec - 3, 1), size=px.shape)) % (1 << prec)
    return px.astype(np.uint8 if prec <= 8 else np.uint16)[None]


def blocks(table, coded):
    return list(table["length"]), list(table["missing_msbs"]), [bytes(coded[int(o):int(o) + int(n)]) for o, n in zip(table["offset"], table["length"])]


def decode(cx, p, table, coded, lay, px):
    """-> (the bytes the decode wrote -- in `lay` into a sentinel-filled buffer --, what they are if the samples are px's)"""
    if lay is None:
        return cx.decode_host(p, table, coded), px
    exp = X.expected(px, lay, SENTINEL, 0)
    return cx.decode_host(p, table, coded, layout=lay, out=np.full(exp.size, SENTINEL, np.uint8)), exp


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_instance(c):
    assert planned_instance(c) == c["key"]
    p, lay, px = params(c), layout(c), content(c)
    plain = ctx()
    if c["kind"] == "enc":
        cx = ctx(c["env"])
        table, coded = cx.encode_host(p, X.pack(px, lay) if lay else px, layout=lay)
        if c["irrev"]:
            _, _, _, otable, ocoded = __import__("chain").encode_tile_oracle(px[0], c["prec"], c["L"], irrev=True, mct=c["mct"])
            got, want = blocks(table, coded), blocks(otable, np.frombuffer(ocoded, np.uint8))
            assert (got[0], got[2]) == (want[0], want[2])          # (the oracle's table carries no missing_msbs)
            if lay:
                assert blocks(table, coded) == blocks(*plain.encode_host(p, px))
        else:
            assert np.array_equal(plain.decode_host(p, table, coded).view(px.dtype), px)
        return
    table, coded = plain.encode_host(p, px)
    got, exp = decode(ctx(c["env"]), p, table, coded, lay, px)
    if c["irrev"]:
        want, _ = decode(ctx(dict(c["env"], GRK_AMD_FUSE_EGRESS="0")), p, table, coded, lay, px)
        assert np.array_equal(got, want)
    else:
        assert np.array_equal(got.view(exp.dtype), exp)
        ctx(c["env"]).decode_status()          # (no value left the int16 planes: the path taken first is the one that ran)
