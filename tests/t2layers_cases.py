"""The codestreams of the general device Tier-2 reader's tests (tests/test_gpu_t2_read_layers_device.py), built on the CPU: layered
files from tables of the tests' choosing (tests/t2layers_model.py -- fixed seeds, the same bytes wherever they are built), the two
LAZY / TERMALL goldens, and -- where the reference is built -- layered files it writes, as written and with PLT put in by
plt_from_sop.  tests/test_t2_parse_layers_cpu.py puts every one of them through tests/c/t2_parse_layers_units.cpp (the kernels' parse
core on the CPU, under AddressSanitizer) first: the GPU sees only inputs that program has passed.

model_cases() -> [(name, bytes, code, want)]: code None where the stream reads (want: the table it was built from, which the host
reader must return), else the host reader's code."""
import os

import numpy as np

import grok_amd as G
import t2layers_model as LM

HERE = os.path.dirname(os.path.abspath(__file__))
SOP, EPH, PLT = G.CS_SOP, G.CS_EPH, G.CS_PLT


def tile(sty, comps=1):
    """4 x 4 blocks: grids of 10 x 16 at the top resolution, trees of five levels (as tests/t2read_cases.py)"""
    return G.TileParams.make(40, 64, comps, 8, 1, cblk=(2, 2), part1=sty is not None, cblksty=sty or 0)


def wide(sty):
    """band grids of 65 x 1 blocks: trees of eight levels"""
    return G.TileParams.make(260, 4, 1, 8, 0, cblk=(2, 2), part1=sty is not None, cblksty=sty or 0)


def never(n):
    return [dict(zbp=0, layers={}) for _ in range(n)]


def num_blocks(p):
    return len(G.tile_layout(p)[0])


def plt_from_sop(cs):
    """A stream written with SOP and without PLT -> the same stream with PLT marker segments in every tile-part: the packet lengths
    are the distances between the SOP marker segments (0xFF91 0x0004 cannot occur inside stuffed headers or coded bytes), Psot
    is fixed up (the stream carries no TLM).  The host reader checks every packet against PLT: reading the result validates this."""
    cs = bytes(cs)
    assert not G.read_header(cs).flags & G.CS_TLM
    out = bytearray()
    at = cs.index(b"\xff\x90\x00\x0a")
    out += cs[:at]
    while cs[at:at + 2] == b"\xff\x90":
        psot = int.from_bytes(cs[at + 6:at + 10], "big")
        end = at + psot if psot else len(cs) - 2
        sod = cs.index(b"\xff\x93", at + 12) + 2
        assert cs[at + 12:at + 14] == b"\xff\x93", "a tile-part header with marker segments of its own"
        starts = []
        i = cs.find(b"\xff\x91\x00\x04", sod, end)
        assert i == sod
        while i >= 0:
            starts.append(i)
            i = cs.find(b"\xff\x91\x00\x04", i + 6, end)
        marker, z, cur = b"", 0, b""
        # (entries of 7 bits per byte, the last byte of one with bit 7 clear; no entry runs on into the next marker segment)
        entries = []
        for a, b in zip(starts, starts[1:] + [end]):
            n = b - a
            e = [n & 0x7F]
            n >>= 7
            while n:
                e.insert(0, 0x80 | (n & 0x7F))
                n >>= 7
            entries.append(bytes(e))
        for e in entries + [None]:
            if e is None or len(cur) + len(e) > 60000:
                marker += b"\xff\x58" + (3 + len(cur)).to_bytes(2, "big") + bytes([z]) + cur
                z, cur = z + 1, b""
            if e is not None:
                cur += e
        out += cs[at:at + 6] + (end - at + len(marker)).to_bytes(4, "big") + cs[at + 10:at + 12] + marker + cs[at + 12:end]
        at = end
    out += cs[at:]
    return bytes(out)


def _row_of(p, res, band, index=0):
    """the index-th row of the band (res, band) of component 0"""
    rows = [i for i, b in enumerate(G.tile_layout(p)[0]) if b.res == res and b.band == band and b.comp == 0]
    return rows[index]


def model_cases():
    out = []

    def add(name, p, w, h, layers, order, flags, sty, table, code=None, **kw):
        cs, want = LM.build(p, w, h, layers, order, flags, sty, table, **kw)
        out.append((name, cs, code, want if code is None else None))

    # every order with and without PLT, SOP / EPH on and off, every style, one and three components: drawn tables
    n = 0
    for order in range(5):
        for plt in (0, PLT):
            for sty in (None, 0, 1, 4, 5):
                comps = 3 if (n % 3) == 0 else 1
                flags = plt | (SOP if n & 1 else 0) | (EPH if n & 2 else 0)
                p = tile(sty, comps)
                add("drawn-o%d-%s-%s-f%x-c%d" % (order, "plt" if plt else "chain", "ht" if sty is None else "sty%02x" % sty, flags, comps), p, 40, 64,
                    3 + n % 2, order, flags, sty, LM.draw_table(p, 3 + n % 2, sty, 100 + n), seed=200 + n, empty_packets=bool(n % 4))
                n += 1
    for sty in (None, 0, 5):
        p = wide(sty)
        add("grid-65x1-%s" % ("ht" if sty is None else "sty%02x" % sty), p, 260, 4, 3, 0, PLT | EPH, sty, LM.draw_table(p, 3, sty, 300), seed=301)
    # the named tables: a Part-1 tile of one component, everything else never included
    p = tile(0)
    nb = num_blocks(p)
    kmax = [int(b.kmax) for b in G.tile_layout(p)[0]]
    r0, r1, r2, r3 = (_row_of(p, 1, 1, i) for i in (0, 1, 7, 39))
    L = 4
    t = never(nb)
    t[r0] = dict(zbp=1, layers={0: (1, [7])})
    t[r1] = dict(zbp=0, layers={1: (2, [9])})
    t[r2] = dict(zbp=2, layers={L - 1: (1, [3])})
    for flags in (0, PLT | SOP):
        add("first-inclusion-0-1-last-never-f%x" % flags, p, 40, 64, L, 0, flags, 0, t)
    t = never(nb)
    t[r0] = dict(zbp=0, layers={0: (1, [4]), 2: (2, [6]), 3: (1, [1])})
    t[_row_of(p, 0, 0, 3)] = dict(zbp=1, layers={1: (1, [2]), 3: (1, [2])})
    add("skips-a-layer-and-comes-back", p, 40, 64, L, 2, PLT, 0, t)
    # (no block contributes in layers 1 and 3: every packet of them is one zero bit)
    t = never(nb)
    t[r0] = dict(zbp=0, layers={0: (1, [4]), 2: (1, [5])})
    t[r3] = dict(zbp=1, layers={2: (1, [8])})
    for flags in (SOP | EPH, PLT):
        add("empty-packets-in-the-middle-and-last-f%x" % flags, p, 40, 64, L, 1, flags, 0, t)
    t = never(nb)
    t[r0] = dict(zbp=0, layers={0: (2, [0]), 1: (1, [5]), 2: (1, [0])})
    t[r1] = dict(zbp=0, layers={1: (3, [0])})
    add("passes-with-length-0", p, 40, 64, L, 0, PLT, 0, t)
    t = never(nb)
    t[r0] = dict(zbp=0, layers={0: (1, [5]), 1: (1, [3000]), 2: (1, [2]), 3: (1, [100000])})
    add("lblock-raised-later-and-carried", p, 40, 64, L, 3, 0, 0, t)
    # Table B.4's five branches; 164 passes in all (of no bytes: no band here has the bit-planes for them) and one more
    for last, code in ((137, None), (138, G.ERR_INVALID)):
        t = never(nb)
        t[r0] = dict(zbp=0, layers={0: (1, [0]), 1: (2, [0]), 2: (4, [0]), 3: (20, [0]), 4: (last, [0])})
        t[r1] = dict(zbp=0, layers={0: (36, [0]), 1: (37, [0]), 2: (6, [0]), 3: (5, [0]), 4: (3, [0])})
        for flags in (0, PLT):
            add("passes-%d-f%x" % (27 + last, flags), p, 40, 64, 5, 4, flags, 0, t, code)
    # LAZY: a layer boundary on a segment's end (10 = 4 + 6) and inside one; the raw pair and the clean-up pass behind
    q = tile(1)
    t = never(nb)
    t[r0] = dict(zbp=0, layers={0: (4, [11]), 1: (6, [13]), 2: (3, [5, 2])})
    t[r1] = dict(zbp=0, layers={0: (4, [9]), 1: (3, [1]), 2: (5, [2, 6]), 3: (2, [1, 4])})
    assert min(kmax[r0], kmax[r1]) >= 6
    for flags in (EPH, PLT | EPH):
        add("lazy-layer-boundaries-f%x" % flags, q, 40, 64, L, 0, flags, 1, t)
    q = tile(4)
    t = never(nb)
    t[r0] = dict(zbp=0, layers={0: (3, [4, 0, 9]), 2: (2, [1, 1])})
    t[r2] = dict(zbp=1, layers={3: (1, [200])})
    for flags in (0, PLT):
        add("termall-f%x" % flags, q, 40, 64, L, 2, flags, 4, t)
    t = never(nb)
    t[r0] = dict(zbp=0, layers={0: (1, [3]), 1: (3, [40]), 2: (2, [500])})
    add("one-segment-growing-over-three-layers", p, 40, 64, L, 0, PLT, 0, t)
    # every block has one piece: no appendix; beside it blocks of both kinds
    t = LM.draw_table(p, L, 0, 400)
    for x in t:
        keep = [l for l in x["layers"] if sum(x["layers"][l][1])][:1]
        x["layers"] = {l: x["layers"][l] for l in keep}
    for flags in (SOP, PLT):
        add("one-piece-per-block-f%x" % flags, p, 40, 64, L, 1, flags, 0, t)
    assert out[-1][3]["appendix_bytes"] == 0 and len(out[-1][3]["segments"]) > 100, "a table of one piece per block has no appendix"
    t2 = LM.draw_table(p, L, 0, 401)
    for i in range(0, nb, 2):
        t2[i] = t[i]
    add("both-kinds-of-block", p, 40, 64, L, 1, PLT, 0, t2)
    # 130 layers, a block first included in layer 129: a node of one byte cannot hold its bound
    t = never(nb)
    t[r0] = dict(zbp=0, layers={129: (1, [6])})
    t[r3] = dict(zbp=0, layers={0: (1, [2]), 64: (1, [2]), 128: (1, [2])})
    for flags in (0, PLT):
        add("130-layers-first-inclusion-in-129-f%x" % flags, p, 40, 64, 130, 0, flags, 0, t)
    # HT: two passes in all -- in one contribution, and over two layers
    q = tile(None)
    t = never(nb)
    t[r0] = dict(zbp=0, layers={0: (2, [3, 3])})
    add("ht-two-passes-at-once", q, 40, 64, 2, 0, PLT, None, t, G.ERR_UNSUPPORTED)
    t = never(nb)
    t[r0] = dict(zbp=0, layers={0: (1, [3]), 1: (1, [3])})
    for flags in (0, PLT):
        add("ht-two-passes-over-two-layers-f%x" % flags, q, 40, 64, 2, 0, flags, None, t, G.ERR_UNSUPPORTED)
    # Part-1: more passes over the layers than the block's bit-planes hold (one bit-plane: one pass)
    t = never(nb)
    t[r0] = dict(zbp=kmax[r0] - 1, layers={0: (1, [3]), 1: (1, [3])})
    for flags in (0, PLT):
        add("more-passes-than-bit-planes-f%x" % flags, p, 40, 64, 2, 0, flags, 0, t, G.ERR_INVALID)
    names = [x[0] for x in out]
    assert len(set(names)) == len(names)
    return out


def golden_cases():
    """the two goldens that the single-layer device reader refuses"""
    out = []
    for f in sorted(os.listdir(os.path.join(HERE, "golden"))):
        if "_sty05_" in f or "_sty3f_" in f:
            out.append((f, open(os.path.join(HERE, "golden", f), "rb").read(), None, None))
    assert len(out) == 2
    return out


REF_VARS = ("REF_PROG_ORDER", "REF_PRECINCTS", "REF_CSTY", "REF_WRITE_PLT", "REF_WRITE_TLM", "REF_LAYERS", "REF_IMG_X0", "REF_IMG_Y0")


def reference_stream(monkeypatch, ht, order, px=None, **kw):
    """the reference's own layered file: 200 x 256 x 3 in 9 tiles of 100 x 77, three layers, precincts, SOP and EPH"""
    import refharness as R
    import synth
    for k in REF_VARS:
        monkeypatch.delenv(k, raising=False)
    for k, v in dict(REF_PROG_ORDER=order, REF_PRECINCTS="64,64,32,32", REF_CSTY=6, REF_LAYERS="20,10,1").items():
        monkeypatch.setenv(k, str(v))
    px = synth.g2(3, 200, 256, 8) if px is None else px
    kw.setdefault("TW", 100); kw.setdefault("TH", 77); kw.setdefault("numres", 4)
    return R.encode(px, 8, mode=1, ht=ht, cblksty=0, **kw)[0]


def reference_cases(monkeypatch):
    out = []
    for ht in (1, 0):
        for order in range(5):
            cs = reference_stream(monkeypatch, ht, order)
            info = G.read_header(cs)
            assert info.num_layers == 3 and info.num_tiles == 9 and not info.flags & G.CS_PLT
            name = "ref-%s-o%d" % ("ht" if ht else "p1", order)
            out.append((name, cs, None, None))
            with_plt = plt_from_sop(cs)
            assert G.read_header(with_plt).flags & G.CS_PLT
            out.append((name + "-plt", with_plt, None, None))
    return out
