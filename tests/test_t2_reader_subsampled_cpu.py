"""CPU: the Tier-2 reader on codestreams with sub-sampled components (SIZ XRsiz / YRsiz: 4:2:2, 4:2:0, ...): every component of a
tile with its own rectangle, precinct grid and tag trees, the packets in the order the writer's packet_order gives with the factors.
Against this library's own writer (grk_amd_write_codestream_subsampled over the oracle's blocks), against itself on the reference
encoder's streams, and on hostile input.  (The pixels of such streams: tests/test_gpu_decode_image_subsampled.py.)"""
import ctypes as C

import numpy as np
import pytest

import grok_amd as G
import oracle as O
import refharness as R
import synth
from grok_amd.capi import CODED_DTYPE
from test_t2_reader_cpu import REF_VARS, hostile_driver, run_hostile, tile_parts_and_plt

needs_ref = pytest.mark.skipif(not R.have_ref(), reason="oracle/_ref (the real reference) not built here")
S420, S422 = [(1, 1), (2, 2), (2, 2)], [(1, 1), (2, 1), (2, 1)]


def cdiv(a, b):
    return (a + b - 1) // b


def comp_shape(layout, dx, dy):
    """(h, w) of a component of the image in its own samples"""
    return cdiv(layout.y1, dy) - cdiv(layout.y0, dy), cdiv(layout.x1, dx) - cdiv(layout.x0, dx)


def make_planes(layout, sampling, prec, seed=0):
    return [synth.g2(1, *comp_shape(layout, dx, dy), prec, seed=60 + 5 * c + seed)[0] for c, (dx, dy) in enumerate(sampling)]


def tile_comp(layout, base, dx, dy, t):
    """grk_amd_layout_tile_comp as one component: the rectangle of a component of tile t in the component's samples"""
    L = G.lib()
    L.grk_amd_layout_tile_comp.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
    p = G.TileParams()
    assert L.grk_amd_layout_tile_comp(C.addressof(layout), C.addressof(base), dx, dy, t, C.addressof(p)) == 0
    p.num_comps, p.mct = 1, 0
    return p


def num_tiles(layout):
    return G.lib().grk_amd_layout_num_tiles(C.byref(layout))


def precincts_from_sizes(sizes, L):
    """grk_compress -c [w,h],[w,h]: from the highest resolution down, the last one halved beyond the list -> COD exponents by resolution"""
    v = list(zip(sizes[0::2], sizes[1::2]))
    out = []
    for r in range(L + 1):
        q = L - r
        pw, ph = v[q] if q < len(v) else (v[-1][0] >> (q - len(v) + 1), v[-1][1] >> (q - len(v) + 1))
        out.append((max(1, int(pw).bit_length() - 1), max(1, int(ph).bit_length() - 1)))
    return out


def write_subsampled(layout, base, sampling, table, coded, flags):
    L = G.lib()
    L.grk_amd_write_codestream_subsampled.restype = C.c_int64
    L.grk_amd_write_codestream_subsampled.argtypes = [C.c_void_p] * 6 + [C.c_uint32, C.c_void_p, C.c_uint64]
    dxs = (C.c_uint8 * len(sampling))(*[a for a, _ in sampling])
    dys = (C.c_uint8 * len(sampling))(*[b for _, b in sampling])
    out = np.empty(coded.size + len(table) * 8 + (1 << 20), np.uint8)
    n = L.grk_amd_write_codestream_subsampled(C.addressof(layout), C.addressof(base), C.addressof(dxs), C.addressof(dys), table.ctypes.data,
                                              coded.ctypes.data, flags, out.ctypes.data, out.size)
    assert n > 0, n
    return out[:n].tobytes()


# ---- 1. against this library's own writer ------------------------------------------------------------------------------------
SHAPES = [
    # W, H, sampling, prec, levels, tile, offset
    (256, 192, S420, 8, 4, None, (0, 0)),
    (300, 200, S422, 8, 3, None, (0, 0)),
    (200, 150, S420 + [(1, 1)], 12, 3, None, (0, 0)),
    (256, 256, [(2, 2)] * 3, 8, 4, None, (0, 0)),
    (259, 131, [(1, 1), (4, 1), (1, 4)], 8, 2, (100, 70), (0, 0)),
    (130, 99, S420, 8, 3, (64, 48), (2, 2)),
    (130, 99, S420, 8, 3, (64, 48), (3, 1)),
]
_coded = {}


def oracle_tables(shape, prc):
    """the oracle's blocks of every tile-component of the image, tile-major and component-major: (layout, base, table, coded, kmax - 1)"""
    key = (SHAPES.index(shape), prc)
    if key not in _coded:
        W, H, sampling, prec, L, tile, off = shape
        layout = G.ImageLayout.make(W, H, *(tile or (None, None)), offset=off)
        precincts = precincts_from_sizes([128, 128, 64, 64], L) if prc else None
        base = G.TileParams.make(1, 1, len(sampling), prec, L, mct=False, precincts=precincts)
        planes = make_planes(layout, sampling, prec)
        tabs, chunks, msbs, at = [], [], [], 0
        for t in range(num_tiles(layout)):
            for c, (dx, dy) in enumerate(sampling):
                p = tile_comp(layout, base, dx, dy, t)
                x, y = p.tile_x0 - cdiv(layout.x0, dx), p.tile_y0 - cdiv(layout.y0, dy)
                sub = np.ascontiguousarray(planes[c][y:y + p.tile_h, x:x + p.tile_w])[None]
                _, lens, coded = O.encode_tile_rev(sub, prec, L, mct=False, origin=(p.tile_x0, p.tile_y0), precincts=precincts)
                tt = np.zeros(len(lens), CODED_DTYPE)
                tt["length"] = lens
                tt["offset"] = at + np.concatenate([[0], np.cumsum(lens)[:-1]])
                at += int(lens.sum())
                tabs.append(tt)
                chunks.append(coded)
                msbs.append([b.kmax - 1 for b in G.tile_layout(p)[0]])
                assert len(msbs[-1]) == len(lens) == G.lib().grk_amd_tile_num_blocks(p)
        _coded[key] = (layout, base, np.concatenate(tabs), np.concatenate(chunks), np.concatenate(msbs))
    return _coded[key]


ALL_MARKS = G.CS_SOP | G.CS_EPH | G.CS_PLT | G.CS_TLM


@pytest.mark.parametrize("prc", [0, 1], ids=["dflt", "prc"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d-%s-t%s-off%d.%d" % (s[0], s[1], "".join("%d%d" % f for f in s[2]), s[5] and s[5][0], *s[6]))
def test_own_subsampled_streams_read_back_as_their_tables(shape, prc):
    layout, base, table, coded, msbs = oracle_tables(shape, prc)
    sampling = shape[2]
    for order in range(5):
        for flags in (0, G.CS_PLT, ALL_MARKS):
            fl = flags | G.CS_PROG(order)
            cs = write_subsampled(layout, base, sampling, table, coded, fl)
            info = G.read_header(cs)
            assert [(info.comp_dx[c], info.comp_dy[c]) for c in range(len(sampling))] == sampling
            assert info.flags == fl and info.num_blocks == len(table) and info.num_tiles == num_tiles(layout)
            assert G.stream_comp_sizes(info) == [comp_shape(layout, dx, dy)[::-1] for dx, dy in sampling]
            out = G.read_packets(cs, info, 1)
            assert len(out["rows"]) == len(table) and len(out["moves"]) == 0 and out["appendix_bytes"] == 0
            assert np.array_equal(out["rows"]["length"], table["length"])
            assert np.array_equal(out["rows"]["missing_msbs"], msbs)
            cb = np.frombuffer(cs, np.uint8)
            for i in range(len(table)):
                o, n, t = int(out["rows"][i]["offset"]), int(table[i]["length"]), int(table[i]["offset"])
                assert o + n <= len(cs) and np.array_equal(cb[o:o + n], coded[t:t + n]), i
            assert np.array_equal(out["first_segment"], np.arange(len(table) + 1)) and np.array_equal(out["segments"]["length"], table["length"])
            four = G.read_packets(cs, info, 4)
            assert all(np.array_equal(out[k], four[k]) for k in ("rows", "first_segment", "segments", "moves"))


# ---- 2. against the reference's encoder --------------------------------------------------------------------------------------
def ref_subsampled_stream(monkeypatch, planes, sampling, prec, W, H, env=None, TW=None, TH=None, numres=4, irrev=0, ht=1, cblksty=0, mct=0):
    """grk_compress of the planes (tests/test_gpu_subsampled.py: REF_COMP_SUBSAMPLING with EncCfg) -> codestream bytes"""
    for k in REF_VARS:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, str(v))
    monkeypatch.setenv("REF_COMP_SUBSAMPLING", ",".join("%d,%d" % s for s in sampling))
    monkeypatch.setenv("REF_TCP_MCT", str(int(mct)))
    flat = np.concatenate([np.ascontiguousarray(pl).reshape(-1) for pl in planes])
    cfg = R.EncCfg(len(sampling), W, H, TW or W + int((env or {}).get("REF_IMG_X0", 0)), TH or H + int((env or {}).get("REF_IMG_Y0", 0)), prec, irrev,
                   numres, ht, 1, 0, 0, 0, cblksty)
    out = np.zeros(flat.size * flat.itemsize * 4 + (1 << 20), np.uint8)
    secs = C.c_double(0)
    n = R.lib().ref_encode(C.byref(cfg), flat.ctypes.data, out.ctypes.data, out.size, C.byref(secs), None)
    assert n > 0, n
    return out[:n].tobytes()


REF_CASES = [
    # W, H, sampling, prec, numres, tile, offset, ht, irrev, cblksty, env
    (256, 192, S420, 8, 5, None, (0, 0), 1, 0, 0, {"REF_WRITE_PLT": 1}),
    (300, 200, S422, 8, 4, None, (0, 0), 0, 0, 0, {"REF_PROG_ORDER": 2, "REF_WRITE_PLT": 1, "REF_CSTY": 6}),
    (259, 131, [(1, 1), (4, 1), (1, 4)], 8, 3, (100, 70), (0, 0), 1, 0, 0, {"REF_PROG_ORDER": 3, "REF_WRITE_PLT": 1, "REF_WRITE_TLM": 1}),
    (130, 99, S420, 8, 4, (64, 48), (2, 2), 0, 1, 0x05, {"REF_PROG_ORDER": 4, "REF_WRITE_PLT": 1, "REF_PRECINCTS": "64,64,32,32"}),
    (320, 200, S420, 10, 4, (128, 128), (0, 0), 0, 1, 0, {"REF_PROG_ORDER": 1}),
    (200, 150, S420 + [(1, 1)], 12, 4, (100, 75), (0, 0), 1, 0, 0, {"REF_PROG_ORDER": 4, "REF_CSTY": 6}),
    (256, 192, S420, 8, 4, (128, 96), (0, 0), 0, 0, 0, {"REF_LAYERS": "20,1", "REF_PROG_ORDER": 2}),
    (256, 192, S420, 8, 4, None, (2, 2), 1, 0, 0, {"REF_LAYERS": "20,1"}),
]


@needs_ref
@pytest.mark.parametrize("case", REF_CASES, ids=lambda k: "%dx%d-%s-o%s" % (k[0], k[1], "ht" if k[7] else "p1", k[10].get("REF_PROG_ORDER", 0)))
def test_reference_subsampled_streams_are_consistent(monkeypatch, case):
    W, H, sampling, prec, numres, tile, off, ht, irrev, sty, env = case
    layout = G.ImageLayout.make(W, H, *(tile or (None, None)), offset=off)
    planes = make_planes(layout, sampling, prec, seed=2)
    env = dict(env, REF_IMG_X0=off[0], REF_IMG_Y0=off[1])
    cs = ref_subsampled_stream(monkeypatch, planes, sampling, prec, W, H, env, *(tile or (None, None)), numres=numres, irrev=irrev, ht=ht, cblksty=sty)
    info = G.read_header(cs)
    layers = len(str(env.get("REF_LAYERS", "1")).split(","))
    assert info.num_layers == layers and [(info.comp_dx[c], info.comp_dy[c]) for c in range(len(sampling))] == sampling
    assert all(getattr(info.layout, k) == getattr(layout, k) for k in ("x0", "y0", "x1", "y1", "t_width", "t_height"))
    nt = num_tiles(layout)
    want_blocks = sum(G.lib().grk_amd_tile_num_blocks(tile_comp(info.layout, info.base, dx, dy, t)) for t in range(nt) for dx, dy in sampling)
    assert info.num_blocks == want_blocks and info.num_tiles == nt
    # (the reader refuses a packet whose length differs from its PLT entry and a tile-part that is not consumed exactly: a table at
    #  all means both held)
    out = G.read_packets(cs, info, 1)
    four = G.read_packets(cs, info, 4)
    assert all(np.array_equal(out[k], four[k]) for k in ("rows", "first_segment", "segments", "moves"))
    rows, first, segs, moves = out["rows"], out["first_segment"], out["segments"], out["moves"]
    assert len(rows) == want_blocks
    # the moves tile the appendix exactly once
    order_ = np.argsort(moves["dst"], kind="stable")
    dst, ln = moves["dst"][order_].astype(np.int64), moves["len"][order_].astype(np.int64)
    assert len(moves) == 0 or (dst[0] == 0 and np.array_equal(dst[1:], np.cumsum(ln)[:-1]) and dst[-1] + ln[-1] == out["appendix_bytes"])
    assert np.all(moves["src"].astype(np.int64) + moves["len"].astype(np.int64) <= len(cs))
    if layers > 1 and not ht:
        assert len(moves) > 0
    # per block: its segments' lengths == its row
    seg_sum = np.add.reduceat(np.concatenate([segs["length"].astype(np.int64), [0]]), first[:-1].astype(np.int64)) * (first[1:] > first[:-1])
    assert np.array_equal(seg_sum, rows["length"].astype(np.int64))
    in_app = rows["offset"].astype(np.int64) >= len(cs)
    assert int(rows["length"][in_app].astype(np.int64).sum()) == out["appendix_bytes"]
    assert np.all(rows["offset"][~in_app].astype(np.int64) + rows["length"][~in_app] <= len(cs))
    # every byte between SOD and the end of a tile-part is a packet's: the headers (at least one byte a packet, SOP and EPH on
    # top) plus the blocks' bytes -- with PLT to the byte, the entries being the packets' lengths
    parts = tile_parts_and_plt(cs)
    assert len(parts) == nt
    body = sum(end - start for start, end, _ in parts.values())
    coded_bytes = int(rows["length"].astype(np.int64).sum())
    assert coded_bytes < body
    if info.flags & G.CS_PLT:
        csty = int(env.get("REF_CSTY", 0))
        per_packet = (6 if csty & 2 else 0) + (2 if csty & 4 else 0)
        npk = 0
        for start, end, lens in parts.values():
            assert sum(lens) == end - start
            npk += len(lens)
        assert coded_bytes + npk * (1 + per_packet) <= body
        # one PLT entry off by one (another gets the byte, so the sum still holds): refused
        bad = bytearray(cs)
        pos = G.locate_tile_parts(cs)[0][0][0] + 12
        assert bad[pos:pos + 2] == b"\xff\x58"
        plt_len = int.from_bytes(bad[pos + 2:pos + 4], "big")
        last = [i for i in range(pos + 5, pos + 2 + plt_len) if not bad[i] & 0x80 and bad[i] not in (0, 0x7F)]      # entries' last bytes
        assert len(last) >= 2
        bad[last[0]] += 1
        bad[last[1]] -= 1
        with pytest.raises(G.ReaderError) as e:
            G.read_packets(bytes(bad), None, 1)
        assert e.value.code == G.capi.ERR_INVALID and "PLT" in e.value.reason


# ---- 3. hostile input ----------------------------------------------------------------------------------------------------------
@needs_ref
@pytest.mark.parametrize("ht", [1, 0], ids=["ht", "p1-layers"])
def test_hostile_input_subsampled_streams_every_prefix_and_corruptions(monkeypatch, ht):
    W, H = 96, 64
    layout = G.ImageLayout.make(W, H, 64, 64)
    planes = make_planes(layout, S420, 8, seed=4)
    env = {"REF_WRITE_PLT": 1, "REF_CSTY": 6} if ht else {"REF_LAYERS": "20,1", "REF_PRECINCTS": "32,32,16,16", "REF_PROG_ORDER": 2}
    cs = ref_subsampled_stream(monkeypatch, planes, S420, 8, W, H, env, 64, 64, numres=3, ht=ht, cblksty=0 if ht else 0x05)
    info = G.read_header(cs)
    assert info.num_layers == (1 if ht else 2) and info.num_tiles == 2 and (info.comp_dx[1], info.comp_dy[2]) == (2, 2)
    assert ht or len(G.read_packets(cs)["moves"]) > 0
    run_hostile(hostile_driver(), cs, 1500, 3 + ht)
