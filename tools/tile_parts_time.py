#!/usr/bin/env python3
"""What a file cut into TILE-PARTS costs grk_amd_decode_image_device_ex beside its undivided twin: the codestream and the pixels in
device memory.  The files are this library's own HT files (grk_amd_encode_image), cut by the model tests/tileparts.py:

  * 8192^2 x 3 in one tile, LRCP, cut per resolution (what `grk_compress -u R` does);
  * 16384^2 x 3 in 256 tiles, CPRL, cut per component (`-u C`), a tile's tile-parts together;

each with PLT (a chain per packet) and without (written with SOP so that the model finds the packets, PLT dropped: one serial chain
per tile).  An undivided file goes through KL / KH / KC-L; a cut one is refused by KL for its second tile-part and read again through
KL-P / KH-P and KC-L over the part table, so its figure holds that first attempt too.  Medians with min..max of --repeats (7) on one
box, the two settings of a pair alternated within each repeat; host wall clock around a synchronised call.

    python tools/tile_parts_time.py [--repeats 7] [--small] > profiles/tile_parts.txt
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
import tileparts as TP  # noqa: E402
from decode_device_time import alternated, image, show  # noqa: E402


def per_resolution(levels, comps):
    return lambda tile, n: [comps * r for r in range(1, levels + 1)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--small", action="store_true", help="2048 / 4096 instead of 8192 / 16384 (a quick look)")
    a = ap.parse_args()
    c = G.Context(0)
    S1, S2 = (2048, 4096) if a.small else (8192, 16384)
    L = 5
    print("# tools/tile_parts_time.py: medians (min .. max) of %d repeats, the two settings alternated within a repeat; %s" % (a.repeats, torch.cuda.get_device_name(0)))
    shapes = (("one tile %d^2 x 3, LRCP, cut per resolution" % S1, S1, S1, 0, per_resolution(L, 3)),
              ("256 tiles, %d^2 x 3, CPRL, cut per component" % S2, S2, S2 // 16, 4, TP.thirds))
    for shape, S, T, order, boundaries in shapes:
        px = image(S)
        layout = G.ImageLayout.make(S, S, T, T)
        base = G.TileParams.make(T, T, 3, 8, L)
        d_out = torch.zeros(3 * S * S, dtype=torch.uint8, device="cuda")
        for plt in (1, 0):
            whole = c.encode_image(layout, base, px, (G.CS_PLT if plt else G.CS_SOP) | G.CS_PROG(order))
            cut = TP.cut(whole, boundaries=boundaries, plt="keep" if plt else "drop")
            name = "%s, HT, %s" % (shape, "PLT" if plt else "no PLT (SOP)")
            print("# %s: %d bytes undivided, %d bytes in %d tile-parts" % (name, len(whole), len(cut.cs), len(cut.parts)))
            dev = {k: torch.from_numpy(np.frombuffer(v, np.uint8).copy()).cuda() for k, v in (("undivided", whole), ("cut", cut.cs))}
            torch.cuda.synchronize()
            outs = {}
            for k, d in dev.items():
                d_out.zero_()
                torch.cuda.synchronize()
                c.decode_image_resident_ex(d.data_ptr(), d.numel(), d_out.data_ptr(), d_out.numel())
                c.decode_status()
                outs[k] = d_out.cpu().numpy().copy()
            assert np.array_equal(outs["undivided"], outs["cut"]) and np.array_equal(outs["cut"].reshape(px.shape), px)

            def run(d):
                def fn():
                    c.decode_image_resident_ex(d.data_ptr(), d.numel(), d_out.data_ptr(), d_out.numel())
                    c.decode_status()
                return fn

            res = alternated({"decode_image_device_ex, undivided": run(dev["undivided"]), "decode_image_device_ex, cut into tile-parts": run(dev["cut"])}, a.repeats)
            show(name, res)
            u, k = res["decode_image_device_ex, undivided"][0], res["decode_image_device_ex, cut into tile-parts"][0]
            print("    the cut file takes %.2f x its undivided twin (%+.3f ms)" % (k / u, k - u))
            del dev
        del px, d_out
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
