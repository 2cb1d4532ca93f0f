"""Decode at reduced resolution (grk_amd_set_decode_reduce) on the GPU -- timing only, no assertions (dev tool).

ms per 8192 x 8192 x 3 8-bit HT frame at r = 0, 1, 2, 3, one frame at a time (decode_device back to back, host-synchronised per
block of calls) and as a sequence of 4 frames in flight (grk_amd_set_decode_pipelining); then the Part-1 frame of bench.py's
cfg5 shape (8192^2 x 3 12-bit, EBCOT + ICT + 9/7, written by the reference's encoder: needs oracle/_ref) at r = 0 and 1.
Also the cost of changing r from call to call (r = 0 / 1 and 0 / 1 / 2 in turn): a context keeps the tables of one geometry.
The settings alternate within every repeat and the medians over the repeats are printed (REPEATS, CALLS: environment)."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import grok_amd as G  # noqa: E402
import synth  # noqa: E402

REPEATS = int(os.environ.get("REPEATS", "7"))
CALLS = int(os.environ.get("CALLS", "8"))
S = int(os.environ.get("PROF_SIZE", "8192"))


def per_frame_ms(ctx, p, table, d_coded, nbytes, outs, r):
    ctx.set_decode_reduce(r)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(CALLS):
        ctx.decode_device(p, 1, table, d_coded, nbytes, outs[i % len(outs)].data_ptr())
    ctx.synchronize()
    ctx.decode_status()
    return (time.perf_counter() - t0) / CALLS * 1e3


def run(tag, ctx, seq, p, table, d_coded, nbytes, rs):
    outs = [torch.empty(p.num_comps * S * S * (2 if p.prec > 8 else 1), dtype=torch.uint8, device="cuda") for _ in range(4)]
    for r in rs:                                                          # warm-up: geometry, buffers, first launches
        per_frame_ms(ctx, p, table, d_coded, nbytes, outs, r)
        per_frame_ms(seq, p, table, d_coded, nbytes, outs, r)
    res = {(m, r): [] for m in ("single", "seq4") for r in rs}
    for k in range(REPEATS):
        order = rs[k % len(rs):] + rs[:k % len(rs)]
        for r in order:
            res[("single", r)].append(per_frame_ms(ctx, p, table, d_coded, nbytes, outs, r))
            res[("seq4", r)].append(per_frame_ms(seq, p, table, d_coded, nbytes, outs, r))
    ctx.set_decode_reduce(0)
    seq.set_decode_reduce(0)
    for (m, r), v in sorted(res.items()):
        print("%-8s %-7s r=%d  median %.3f ms/frame  (min %.3f max %.3f, %d x %d calls)" % (
            tag, m, r, statistics.median(v), min(v), max(v), REPEATS, CALLS), flush=True)


def alternating(tag, ctx, seq, p, table, d_coded, nbytes, rs):
    """the cost of changing r between calls: every call's r differs from the previous call's (the context keeps one geometry)"""
    outs = [torch.empty(p.num_comps * S * S * (2 if p.prec > 8 else 1), dtype=torch.uint8, device="cuda") for _ in range(4)]
    for name, c in (("single", ctx), ("seq4", seq)):
        v = []
        for k in range(REPEATS + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(CALLS):
                c.set_decode_reduce(rs[i % len(rs)])
                c.decode_device(p, 1, table, d_coded, nbytes, outs[i % len(outs)].data_ptr())
            c.synchronize()
            c.decode_status()
            if k:                                                         # (the first round: warm-up)
                v.append((time.perf_counter() - t0) / CALLS * 1e3)
        c.set_decode_reduce(0)
        print("%-8s %-7s r alternating %s per call  median %.3f ms/frame  (min %.3f max %.3f, %d x %d calls)" % (
            tag, name, "/".join(map(str, rs)), statistics.median(v), min(v), max(v), REPEATS, CALLS), flush=True)


def main():
    torch.cuda.init()
    ctx = G.Context(0)
    seq = G.Context(0)
    seq.set_decode_pipelining(4)
    # HT 8-bit, this library's encoder
    p = G.TileParams.make(S, S, 3, 8, 5)
    d_px = torch.from_numpy(synth.g2(3, S, S, 8).reshape(-1)).cuda()
    ctx.encode_tiles(p, 1, d_px.data_ptr(), True, fetch=False)
    table, tot = ctx.fetch_table(G.lib().grk_amd_tile_num_blocks(p))
    coded = ctx.fetch_coded(tot)
    d_coded = torch.from_numpy(np.frombuffer(bytes(coded), np.uint8).copy()).cuda()
    del d_px
    run("HT", ctx, seq, p, table, d_coded.data_ptr(), d_coded.numel(), [0, 1, 2, 3])
    alternating("HT", ctx, seq, p, table, d_coded.data_ptr(), d_coded.numel(), [0, 1])
    alternating("HT", ctx, seq, p, table, d_coded.data_ptr(), d_coded.numel(), [0, 1, 2])
    # Part-1 (cfg5 shape), the reference's own encoder
    import refharness as R
    if not R.have_ref():
        print("Part-1 cfg5: skipped (oracle/_ref not present)")
        return
    import j2kparse as J
    px = synth.g2(3, S, S, 12)
    cs, _ = R.encode(px, 12, numres=6, mode=1, ht=0, irrev=1)
    info = J.parse(cs)
    p5 = G.TileParams.make(S, S, 3, 12, info["levels"], irreversible=True, mct=True, part1=True)
    blocks, _ = G.tile_layout(p5)
    rows, data = J.decode_table(info, blocks, True)
    t5 = np.array(rows, dtype=G.capi.CODED_DTYPE)
    words = [(e << 11) | m for e, m in info["qcd"]]
    ctx.set_decode_qcd(words)
    seq.set_decode_qcd(words)
    d5 = torch.from_numpy(np.frombuffer(bytes(data), np.uint8).copy()).cuda()
    run("Part-1", ctx, seq, p5, t5, d5.data_ptr(), d5.numel(), [0, 1])


if __name__ == "__main__":
    main()
