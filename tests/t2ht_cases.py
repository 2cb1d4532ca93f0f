"""The codestreams of the tests of HT blocks with refinement passes (tests/test_t2_ht_refine_cpu.py, tests/test_gpu_t2_ht_refine.py,
tests/test_gpu_ht_refine_files.py), built on the CPU by tests/t2ht_model.py from fixed seeds: the same bytes wherever they are built.
tests/test_t2_ht_refine_cpu.py puts every one of them through tests/c/t2_parse_ht_units.cpp (the kernels' parse core on the CPU,
under AddressSanitizer) first: the GPU sees only inputs that program has passed.

table_cases()   -> [(name, bytes, code, want)]: tables of chosen contribution patterns over random block bytes; code None where the
                   file reads (want: what the refine readers must return), else the code they must refuse it with
content_cases() -> [Content]: files whose blocks are real HT code-blocks (the oracle's cleanup encoder and refinement encoder, as
                   tests/test_gpu_ht_refine.py takes them), with what every block decodes to"""
import numpy as np

import grok_amd as G
import t2ht_model as HM
from t2layers_cases import tile, wide, SOP, EPH, PLT

# contribution patterns by the layers they need; "/0": the refinement segment has no bytes (the block decodes as cleanup only)
BY_LAYERS = {
    1: ["3", "2", "1", "never", "3/0", "2/0"],
    2: ["1|2", "1|1", "2|1", "1|2/0"],
    3: ["1|1|1", "1|-|1", "1|1|1/0"],
}


def patterns_for(layers):
    return [q for need in range(1, layers + 1) for q in BY_LAYERS[need]]


def draw_table(p, layers, seed, max_len=60):
    """every pattern the layer count allows, mixed over the tile's blocks; a pattern starts in any layer that leaves it room"""
    blocks, _ = G.tile_layout(p)
    rng = np.random.default_rng(seed)
    kinds = patterns_for(layers)
    table, used = [], {}
    for i, b in enumerate(blocks):
        kind = kinds[(i + int(rng.integers(0, 2))) % len(kinds)]
        used[kind] = used.get(kind, 0) + 1
        t = dict(zbp=int(rng.integers(0, max(1, int(b.kmax)))), layers={})
        if kind != "never":
            name, _, zero = kind.partition("/")
            first = int(rng.integers(0, layers - len(HM.PATTERNS[name]) + 1))
            t["layers"] = HM.contributions(name, first, int(rng.integers(1, max_len + 1)), 0 if zero else int(rng.integers(1, max_len + 1)))
        table.append(t)
    assert len(used) == len(kinds), "a tile too small for its patterns"
    return table


def never(n):
    return [dict(zbp=0, layers={}) for _ in range(n)]


def table_cases():
    out = []

    def add(name, p, w, h, layers, order, flags, tables, code=None, **kw):
        cs, want = HM.build(p, w, h, layers, order, flags, tables, **kw)
        out.append((name, cs, code, want if code is None else None))

    # the 40 x 64 tile of 4 x 4 blocks (five-level trees): every order, 1 .. 3 layers, the flags as the layered cases combine them
    n = 0
    for order in range(5):
        for layers in (1, 2, 3):
            for plt in (0, PLT):
                comps = 3 if (n % 3) == 0 else 1
                flags = plt | (SOP if n & 1 else 0) | (EPH if n & 2 else 0)
                p = tile(None, comps)
                add("drawn-o%d-L%d-%s-f%x-c%d" % (order, layers, "plt" if plt else "chain", flags, comps), p, 40, 64, layers, order, flags,
                    draw_table(p, layers, 500 + n), seed=600 + n, empty_packets=bool(n % 4))
                n += 1
    # the wide tile: trees of eight levels
    p = wide(None)
    for layers, flags in ((3, PLT | EPH), (2, SOP)):
        add("grid-65x1-L%d-f%x" % (layers, flags), p, 260, 4, layers, 0, flags, draw_table(p, layers, 700 + layers), seed=701)
    # 100 x 70 in tiles of 64 x 48: the edge tiles have another geometry
    base = G.TileParams.make(64, 48, 1, 8, 1, cblk=(2, 2))
    layout = G.ImageLayout.make(100, 70, 64, 48)
    for order, layers, flags in ((0, 3, PLT), (2, 2, SOP | EPH), (4, 3, 0)):
        tables = [draw_table(tp, layers, 800 + 10 * order + k) for k, tp in enumerate(G.layout_tiles(layout, base))]
        add("tiles-2x2-o%d-L%d-f%x" % (order, layers, flags), base, 100, 70, layers, order, flags, tables, tile=(64, 48), seed=801 + order)
    # the tile divided into a tile-part per layer
    p = tile(None)
    for flags in (0, PLT, PLT | SOP | EPH):
        add("by-layer-f%x" % flags, p, 40, 64, 3, 0, flags, draw_table(p, 3, 900), by_layer=True, seed=901)
    # ---- refused: placeholder passes or a second HT set (UNSUPPORTED), a header cut inside the second length field (INVALID)
    nb = len(G.tile_layout(p)[0])
    r0 = [i for i, b in enumerate(G.tile_layout(p)[0]) if b.res == 1 and b.band == 1][0]
    for flags in (0, PLT):
        t = never(nb)
        t[r0] = dict(zbp=0, layers={0: (4, [5, 6, 7])})
        add("four-passes-at-once-f%x" % flags, p, 40, 64, 2, 0, flags, t, G.ERR_UNSUPPORTED)
        t = never(nb)
        t[r0] = dict(zbp=0, layers={0: (1, [5]), 1: (3, [6, 7])})
        add("one-pass-then-three-f%x" % flags, p, 40, 64, 2, 0, flags, t, G.ERR_UNSUPPORTED)
    # the last block of the last packet has three passes, a cleanup segment of 5 bytes and a refinement segment of 40000: Lblock is
    # raised to 15, the second length has 16 bits -- the header's last two bytes hold nothing else
    t = never(nb)
    t[nb - 1] = dict(zbp=0, layers={0: (3, [5, 40000])})
    for cut in (1, 2):
        add("cut-in-the-second-length-%d" % cut, p, 40, 64, 1, 0, 0, t, G.ERR_INVALID, cut=cut)
    names = [x[0] for x in out]
    assert len(set(names)) == len(names)
    return out


def three_pass_file():
    """one small file with a three-pass block: what the readers without the option must refuse"""
    p = tile(None)
    t = never(len(G.tile_layout(p)[0]))
    t[0] = dict(zbp=0, layers={0: (3, [4, 6])})
    return HM.build(p, 40, 64, 1, 0, 0, t)


# ---- files with real content ------------------------------------------------------------------------------------------------------
class Content:
    """name, cs, want (the refine readers' tables), layout, base, tiles (G.layout_tiles), words: per tile per row the block's decoded
    sign-magnitude words (None: a block without bytes), passes: per tile per row 0 .. 3"""


# (name, W, H, tile or None, levels, components, precision, irreversible, code-block exponents)
SHAPES = [
    ("130x67", 130, 67, None, 4, 1, 12, True, (6, 6)),
    ("200x120", 200, 120, None, 2, 3, 8, False, (6, 6)),
    ("37x3", 37, 3, None, 1, 1, 8, True, (6, 6)),
    ("64x64", 64, 64, None, 0, 1, 9, True, (6, 6)),
    ("100x70-tiles", 100, 70, (64, 48), 2, 1, 8, True, (5, 5)),
]


def passes_of(i):
    return 1 if i % 5 == 2 else 2 if i % 7 == 3 else 3


def content_file(shape, layered, flags=0, refine=True):
    """refine False: the same samples with every block cleanup-only"""
    import oracle as O
    import refharness as R
    from test_oracle_ht_refine import make_block, code_block
    name, W, H, tl, L, C, prec, irrev, cblk = shape
    base = G.TileParams.make(*(tl or (W, H)), C, prec, L, irreversible=irrev, cblk=cblk)
    layout = G.ImageLayout.make(W, H, *(tl or (W, H)))
    tiles = G.layout_tiles(layout, base)
    rng = np.random.default_rng(sum(map(ord, name)) + 2)
    tables, words, npasses = [], [], []
    i = 0
    for tp in tiles:
        table, tw, tn = [], [], []
        for b in G.tile_layout(tp)[0]:
            bw, bh = b.x1 - b.x0, b.y1 - b.y0
            want = passes_of(i) if refine else 1
            # (Kmax - 1 zero bit-planes, as tests/test_gpu_ht_refine.py makes its blocks: the 9/7 dequantisation keeps every refined bit;
            #  in the 5/3 file the refined bits lie below the samples' integer bit, so that file holds the plumbing, the colour
            #  transform and the int16-plane trap, and the 9/7 files hold the refined values)
            kk = b.kmax
            mag, sign = make_block(rng, bw, bh, min(kk, 14), int(rng.integers(0, 5)))
            cup, seg, _ = code_block(mag, sign, kk, max(want, 2))
            if want == 1:
                seg = b""
            if i % 11 == 5:
                seg = seg[:len(seg) // 2]                # a truncated refinement segment: zeros are read beyond its end
            mm = kk - 1
            if R.have_ref():
                w = R.ht_decode_block_passes(cup + seg, len(cup), len(seg), want, mm, bw, bh)
            else:
                w = O.ht_refine_decode(O.ht_decode_block(cup, mm, bw, bh), mm, seg, want)
            assert w is not None
            if want == 1:
                lay = {0: (1, [len(cup)])}
            elif layered:
                lay = HM.contributions("1|1|1" if want == 3 else "1|-|1", 0, len(cup), len(seg))
            else:
                lay = HM.contributions(str(want), 0, len(cup), len(seg))
            table.append(dict(zbp=mm, layers=lay, data=cup + seg))
            tw.append(w); tn.append(want)
            i += 1
        tables.append(table); words.append(tw); npasses.append(tn)
    c = Content()
    c.name = "%s-%s%s" % (name, "L3" if layered else "L1", "" if refine else "-cleanup")
    c.cs, c.want = HM.build(base, W, H, 3 if layered else 1, 0, flags, tables, tile=tl, seed=1)
    c.layout, c.base, c.tiles, c.words, c.passes, c.shape = layout, base, tiles, words, npasses, shape
    return c


def content_cases():
    return [content_file(s, layered, PLT if k & 1 else 0) for k, s in enumerate(SHAPES) for layered in (False, True)]


def expected_pixels(c, reduce=0):
    """the oracle's decode of the file's blocks: dequantisation, inverse transform (of the resolutions a reduce leaves), inverse
    colour transform, DC shift and clamp -- tile after tile at its place -> (C, H, W) int32"""
    import chain
    import oracle as O
    name, W, H, tl, L, C, prec, irrev, cblk = c.shape
    rw, rh = -(-W >> reduce), -(-H >> reduce)
    img = np.zeros((C, rh, rw), np.int32)
    for t, tp in enumerate(c.tiles):
        blocks, qcd = G.tile_layout(tp)
        mall = [np.zeros((tp.tile_h, tp.tile_w), np.float32 if irrev else np.int32) for _ in range(C)]
        for b, w in zip(blocks, c.words[t]):
            bw, bh = b.x1 - b.x0, b.y1 - b.y0
            v = O.ht_dequant_irrev(w, chain.band_scale_dec(prec, qcd[chain.band_index(b)], b.kmax)) if irrev else O.ht_dequant_rev(w, b.kmax - 1)
            mall[b.comp][b.py:b.py + bh, b.px:b.px + bw] = v
        x0, y0, w, h = G.reduced_tile_rect(tp, reduce)
        assert x0 == -(-tp.tile_x0 >> reduce) and y0 == -(-tp.tile_y0 >> reduce)
        low = [np.ascontiguousarray(m[:h, :w]) for m in mall]          # (the Mallat plane's corner: the resolutions that are left)
        planes = [O.dwt97_inv(m, L - reduce) if irrev else O.dwt53_inv(m, L - reduce) for m in low]
        planes = [pl.view(np.int32) if irrev else pl for pl in planes]
        px = np.stack(O.color_inv_store(planes, prec, irrev, bool(tp.mct), sgnd=bool(tp.sgnd)))
        img[:, y0:y0 + h, x0:x0 + w] = px
    return img
