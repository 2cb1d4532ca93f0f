"""GPU: forward DWT levels 0 and 1 of the packed 5/3 encoder in one launch (kernels_dwt.hip pair::dwt53_pk_kernel, planned by
plan_dwt_pair) against the same encode with GRK_AMD_DWT_PAIR=0, which launches the two levels one by one: the Mallat planes, the block
table and the coded bytes are equal, and decoding returns the pixels.

Shapes (C = 3, 8 bits, MCT), the smallest at which the kernel can go wrong: 512 x 32 (128 lanes, two strips, two row segments),
512 x 36 (a last segment of two pairs), 1000 x 48 (three strips of 384 columns, the right one ragged, an interior segment),
2056 x 40 (256 lanes, an interior strip), 8 tiles of 512 x 32 (batch).  Content: G2, 0 / 255 checkerboards of period 1 and 2 in both
directions (the range extremes of levels 0 and 1), uniform random bytes.  L = 2 (the
pair is also the last level) and L = 5."""
import os

import numpy as np
import pytest

import gpuutil as U
import grok_amd as G
import oracle as O
import synth
import test_dwt_pair_plan_cpu as PP

SHAPES = {"512x32": (512, 32, 1), "512x36": (512, 36, 1), "1000x48": (1000, 48, 1), "2056x40": (2056, 40, 1), "8x512x32": (512, 32, 8)}
CONTENTS = ("g2", "checker1", "checker2", "random")
OFF = {"GRK_AMD_DWT_PAIR": "0"}
_ctxs, _px = {}, {}


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


def pixels(shape, content, seed=0):
    key = (shape, content, seed)
    if key not in _px:
        W, H, T = SHAPES[shape]
        if content == "g2":
            px = np.stack([synth.g2(3, H, W, 8, seed=11 + seed + t) for t in range(T)])
        elif content == "random":
            px = np.random.default_rng(5 + seed).integers(0, 256, size=(T, 3, H, W)).astype(np.uint8)
        else:
            n = int(content[-1])
            yy, xx = np.mgrid[0:H, 0:W]
            board = ((((xx + seed) // n + yy // n) & 1) * 255).astype(np.uint8)
            px = np.stack([np.stack([board, board, board]) for _ in range(T)])
        _px[key] = px
    return _px[key]


def encode(cx, p, px, T):
    """-> (table fields, blocks, the Mallat planes inside the tile)"""
    table, coded = cx.encode_host(p, px, ntiles=T)
    cx.synchronize()
    assert cx.plane_sample_bytes(p)[0] == 2
    stride, elems = int(G.lib().grk_amd_plane_stride(p)), int(G.lib().grk_amd_plane_elems(p))
    raw = U.from_dev_ptr(cx.plane_device_ptr(1), T * 3 * elems * 2).view(np.int16)
    planes = raw.reshape(T * 3, elems)[:, :p.tile_h * stride].reshape(T * 3, p.tile_h, stride)[:, :, :p.tile_w].copy()
    return (list(table["length"]), list(table["missing_msbs"])), U.split_blocks(table, coded), planes, table, coded


def blocks_of(cx, p, nb):
    table, tot = cx.fetch_table(nb)
    coded = cx.fetch_coded(tot)
    return (list(table["length"]), list(table["missing_msbs"])), U.split_blocks(table, coded)


def test_the_shapes_have_a_pair():
    for W, H, T in SHAPES.values():
        for L in (2, 5):
            assert PP.plan(G.TileParams.make(W, H, 3, 8, L), ntiles=T) is not None
    assert PP.plan(G.TileParams.make(516, 32, 3, 8, 2)) is None


@pytest.mark.gpu
@pytest.mark.parametrize("L", [2, 5])
@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_pair_equals_level_by_level(shape, content, L):
    W, H, T = SHAPES[shape]
    p, px = G.TileParams.make(W, H, 3, 8, L), pixels(shape, content)
    fields, blocks, planes, _, _ = encode(ctx(), p, px, T)
    wfields, wblocks, wplanes, _, _ = encode(ctx(OFF), p, px, T)
    bad = np.argwhere(planes != wplanes)
    assert bad.size == 0, "Mallat planes differ at %d samples, first (plane, row, column) %s" % (len(bad), bad[:4].tolist())
    assert fields == wfields and blocks == wblocks


def reference_refuses(p, table, coded, T):
    """whether the reference's HT block decoder, as the oracle restates it (tests/test_oracle_decode.py pins the two together),
    refuses a block of the stream: it takes no block whose top magnitude needs the upper two of its Kmax bit-planes (U_q >
    missing_msbs, ojph_block_decoder.cpp:1194, defect D5 -- tests/synth.py g2_mid, tests/test_gpu_bit_depths.py)"""
    blocks, _ = G.tile_layout(p)
    assert len(table) == T * len(blocks)
    for i, row in enumerate(table):
        b = blocks[i % len(blocks)]
        if int(row["length"]) and O.ht_decode_block(coded[int(row["offset"]):int(row["offset"]) + int(row["length"])], int(row["missing_msbs"]),
                                                    b.x1 - b.x0, b.y1 - b.y0) is None:
            return True
    return False


@pytest.mark.gpu
@pytest.mark.parametrize("L", [2, 5])
@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_decode_returns_the_pixels(shape, content, L):
    """Decoding what the pair encoded returns the pixels.  Full-range random bytes and the period-2 checkerboard drive blocks of the
    fine bands into the two top bit-planes of their Kmax, which the reference's HT block decoder refuses (defect D5) and this decoder,
    reproducing it, refuses as well -- from either encode: the bytes are those of the level-by-level launches.  The arbiter is that
    decoder on every block of the stream, not the outcome here: where it takes every block the decode must return the pixels (G2 and
    the period-1 checkerboard: every shape); where it refuses one, the decode must refuse as well, and the same content scaled into
    the middle half of the range (64 .. 191), which it takes whole, must come back exact."""
    W, H, T = SHAPES[shape]
    p, px = G.TileParams.make(W, H, 3, 8, L), pixels(shape, content)
    _, _, _, table, coded = encode(ctx(), p, px, T)
    if not reference_refuses(p, table, coded, T):
        assert np.array_equal(ctx().decode_host(p, table, coded, ntiles=T), px)
        return
    assert content in ("random", "checker2"), "G2 and the period-1 checkerboard are inside the reference decoder's range"
    with pytest.raises(RuntimeError):
        ctx().decode_host(p, table, coded, ntiles=T)
    mid = (64 + px.astype(np.uint16) // 2).astype(np.uint8)
    _, _, _, table, coded = encode(ctx(), p, mid, T)
    assert not reference_refuses(p, table, coded, T)
    assert np.array_equal(ctx().decode_host(p, table, coded, ntiles=T), mid)


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["no overlap", "overlap", "pipelined frame streams", "pipelined overlapped"])
@pytest.mark.parametrize("L", [2, 5])
@pytest.mark.parametrize("shape", ["512x32", "2056x40"])
def test_routes(shape, L, route):
    """the un-overlapped route, the overlapped one, and pipelined encodes -- small frames take one side stream each
    (GRK_AMD_FRAME_STREAMS=0: the overlapped pipeline of large frames): three distinct frames in rotation, six calls, every frame
    against its plain level-by-level encode"""
    W, H, T = SHAPES[shape]
    p = G.TileParams.make(W, H, 3, 8, L)
    frames = [pixels(shape, "g2"), pixels(shape, "random", 1), pixels(shape, "checker2", 1)]
    want = [encode(ctx(OFF), p, f, T)[:2] for f in frames]
    if not route.startswith("pipelined"):
        cx = ctx()
        cx.set_overlap(route == "overlap")
        try:
            for f, w in zip(frames, want):
                assert encode(cx, p, f, T)[:2] == w
        finally:
            cx.set_overlap(True)
        return
    cx = ctx({"GRK_AMD_FRAME_STREAMS": "0"} if route.endswith("overlapped") else None)
    nb = len(want[0][1])
    dev = [U.to_dev(f.reshape(-1)) for f in frames]
    cx.set_pipelining(True)
    try:
        for i in range(6):
            cx.encode_tiles(p, T, dev[i % 3].data_ptr(), True, fetch=False)
            assert blocks_of(cx, p, nb) == want[i % 3], "call %d" % i
        cx.synchronize()
    finally:
        cx.set_pipelining(False)


@pytest.mark.gpu
@pytest.mark.parametrize("L", [2, 5])
def test_a_refused_shape(L):
    """516 x 32 (the width is no multiple of 8): no pair, the same bytes with the switch on and off"""
    p = G.TileParams.make(516, 32, 3, 8, L)
    px = np.random.default_rng(9).integers(0, 256, size=(1, 3, 32, 516)).astype(np.uint8)
    a, b = encode(ctx(), p, px, 1), encode(ctx(OFF), p, px, 1)
    assert a[:2] == b[:2] and np.array_equal(a[2], b[2])
