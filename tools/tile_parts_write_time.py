#!/usr/bin/env python3
"""What WRITING tiles divided into tile-parts (GRK_AMD_CS_TP) costs beside the undivided twin, on the device:

  * one 8192^2 x 3 tile, LRCP, PLT: undivided against TP(R) -- 6 parts;
  * 16384^2 x 3 in 256 tiles, CPRL, PLT: undivided against TP(C) -- 3 parts per tile, 768 in the call;

for each, grk_amd_assemble_device alone (the latest grk_amd_encode_tiles call assembled again and again: KT1 + KT1b + KT2 against
KT1 + KT1p + KT1q + KT1r + KT2p) and the whole encode with the file left in device memory (grk_amd_encode_surface_device of an I444
surface in device memory).  Medians with min .. max of --repeats (7) on one box, the two settings of a pair alternated within each
repeat; host wall clock around a synchronous call.  The divided output is checked against the host divided writer once, before timing.

    python tools/tile_parts_write_time.py [--repeats 7] [--small] > profiles/tile_parts_write.txt
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import grok_amd as G  # noqa: E402
from decode_device_time import alternated, image, show  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--small", action="store_true", help="2048 / 4096 instead of 8192 / 16384 (a quick look)")
    a = ap.parse_args()
    c = G.Context(0)
    S1, S2 = (2048, 4096) if a.small else (8192, 16384)
    L = 5
    print("# tools/tile_parts_write_time.py: medians (min .. max) of %d repeats, the two settings alternated within a repeat; %s" % (a.repeats, torch.cuda.get_device_name(0)))
    shapes = (("one tile %d^2 x 3, LRCP, TP(R)" % S1, S1, S1, 0, G.TP_R), ("256 tiles, %d^2 x 3, CPRL, TP(C)" % S2, S2, S2 // 16, 4, G.TP_C))
    for shape, S, T, order, letter in shapes:
        ntiles = (S // T) ** 2
        flags = G.CS_PLT | G.CS_PROG(order)
        div = flags | G.CS_TP(letter)
        p = G.TileParams.make(T, T, 3, 8, L, mct=False)
        # ---- grk_amd_assemble_device alone: ntiles tiles of one content, coded once ----
        tile = image(T)
        d_px = torch.from_numpy(np.tile(tile.reshape(1, -1), (ntiles, 1)).reshape(-1)).cuda()
        torch.cuda.synchronize()
        idx = list(range(ntiles))
        table, tot = c.encode_tiles(p, ntiles, d_px.data_ptr(), True)
        coded = c.fetch_coded(tot)
        bpt = len(table) // ntiles
        n, lens = c.assemble_device(p, idx, div)
        want, want_lens = G.write_tile_parts(p, idx[-1], table[(ntiles - 1) * bpt:], coded, div)
        got = bytes(c.fetch_assembled(n - int(lens[-1]), int(lens[-1])))
        assert got == want, "the divided tile-parts differ from the host writer's"
        nparts = c.assembled_parts()
        n0, _ = c.assemble_device(p, idx, flags)
        print("# %s: %d bytes undivided, %d bytes in %d tile-parts (%d per tile)" % (shape, n0, n, nparts * ntiles, nparts))
        res = alternated({"assemble_device, undivided": lambda: c.assemble_device(p, idx, flags),
                          "assemble_device, divided": lambda: c.assemble_device(p, idx, div)}, a.repeats)
        show(shape + ": grk_amd_assemble_device alone", res)
        u, k = res["assemble_device, undivided"][0], res["assemble_device, divided"][0]
        print("    the divided call takes %.2f x its undivided twin (%+.3f ms)" % (k / u, k - u))
        del d_px
        # ---- the whole encode, the file left in device memory ----
        layout = G.ImageLayout.make(S, S, T, T)
        surface, sampling, nbytes = G.Surface.make("I444", layout, None, 0)
        base = G.TileParams.make(1, 1, 3, 8, L, mct=False)
        px = image(S)
        buf = np.zeros(nbytes, np.uint8)
        surface.scatter(buf, [px[k] for k in range(3)], 1)
        d_buf = torch.from_numpy(buf).cuda()
        torch.cuda.synchronize()
        tlm = G.CS_TLM if ntiles <= 255 else 0                  # (one-byte Ttlm: a file with TLM holds at most 255 tiles)
        sizes = {}
        for name, f in (("undivided", flags | tlm), ("divided", div | tlm)):
            ptr, m = c.encode_surface_device(layout, base, sampling, surface, d_buf.data_ptr(), f, cap=nbytes)
            sizes[name] = m
        print("# %s: the file %d bytes undivided, %d divided" % (shape, sizes["undivided"], sizes["divided"]))
        res = alternated({"encode_surface_device, undivided": lambda: c.encode_surface_device(layout, base, sampling, surface, d_buf.data_ptr(), flags | tlm, cap=nbytes),
                          "encode_surface_device, divided": lambda: c.encode_surface_device(layout, base, sampling, surface, d_buf.data_ptr(), div | tlm, cap=nbytes)},
                         a.repeats)
        show(shape + ": the file left in device memory (%s)" % ("PLT | TLM" if tlm else "PLT"), res)
        u, k = res["encode_surface_device, undivided"][0], res["encode_surface_device, divided"][0]
        print("    the divided file takes %.2f x its undivided twin (%+.3f ms)" % (k / u, k - u))
        del px, buf, d_buf
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
