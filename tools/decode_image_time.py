#!/usr/bin/env python3
"""What reading a whole codestream costs (grk_amd_decode_image): the Tier-2 reader alone, the whole call beside
grk_amd_decode_tiles with a table prepared beforehand (what the call adds: reader + plumbing) and beside grk_decompress, and the
two kernels beside a plain device-to-device copy of the same bytes; and views of the 256-tile file (grk_amd_decode_image_view: a 1024^2
interior window, the whole image at reduce 2) beside the full decode -- with GRK_AMD_LIB naming a library built from an earlier commit,
--view-only gives that commit's full decode on the same box for the comparison.  Medians of --repeats (7) on one box, the settings of a group
alternated within each repeat (not one setting's repeats after the other's); host wall clock around a synchronised call.

    python tools/decode_image_time.py [--repeats 7] [--ref-repeats 3] [--small] > profiles/decode_image.txt
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import grok_amd as G  # noqa: E402
import refharness as R  # noqa: E402
import synth  # noqa: E402
from grok_amd.capi import MOVE_DTYPE  # noqa: E402


def alternated(settings, repeats):
    """settings: {name: fn} -> {name: median ms}, every repeat runs each setting once, in turn"""
    ms = {k: [] for k in settings}
    for fn in settings.values():
        fn()                                            # warm
    for _ in range(repeats):
        for k, fn in settings.items():
            t0 = time.perf_counter()
            fn()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    return {k: float(np.median(v)) for k, v in ms.items()}


def show(title, res, bytes_moved=None):
    print(title)
    for k, v in res.items():
        print("    %-58s %9.3f ms%s" % (k, v, "   %7.1f GB/s" % (bytes_moved / v / 1e6) if bytes_moved else ""))
    sys.stdout.flush()


def image(S):
    """S x S x 3 8-bit: a 2048 x 2048 synthetic image repeated (generating 16384^2 samples one by one takes minutes)"""
    base = synth.g2(3, min(S, 2048), min(S, 2048), 8)
    return np.ascontiguousarray(np.tile(base, (1, S // base.shape[1], S // base.shape[2])))


def views(c, file, repeats):
    """the 256-tile file: the full decode, a T x T window across an interior 4-tile corner, the whole image at reduce 2; device pixels,
    the codestream in pinned memory"""
    S, T, cs, info = file
    pinned = c.host_array(cs.size)
    pinned[:] = cs
    d_out = torch.zeros(3 * S * S, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    settings, uploaded = {}, {}

    def full():
        c.decode_image_device(pinned, d_out.data_ptr(), d_out.numel())
        c.decode_status()
    settings["decode_image, the whole image (%d tile-parts)" % info.num_tiles] = full
    if hasattr(c._L, "grk_amd_decode_image_view"):
        win = (S // 2 - T // 2, S // 2 - T // 2, S // 2 + T // 2, S // 2 + T // 2)
        for name, kw in (("decode_image_view, %d^2 window across a 4-tile corner" % T, dict(window=win)), ("decode_image_view, reduce 2 (%d^2)" % (S // 4), dict(reduce=2))):
            def view(kw=kw):
                c.decode_image_view_device(pinned, d_out.data_ptr(), d_out.numel(), **kw)
                c.decode_status()
            b0 = c.decode_image_counters()
            view()
            b1 = c.decode_image_counters()
            uploaded[name] = (b1[0] - b0[0], b1[1] - b0[1])
            settings[name] = view
    show("views of the 256-tile file, device pixels, codestream in pinned memory (%s)" % os.path.basename(os.path.dirname(G.lib_path())), alternated(settings, repeats))
    for name, (tiles, nbytes) in uploaded.items():
        print("    %-58s %d tiles read, %d of %d bytes uploaded" % (name, tiles, nbytes, cs.size))
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--ref-repeats", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="2048 / 4096 instead of 8192 / 16384 (a quick look)")
    ap.add_argument("--view-only", action="store_true", help="only the views of the 256-tile file beside its full decode")
    a = ap.parse_args()
    c = G.Context(0)
    S1, S2 = (2048, 4096) if a.small else (8192, 16384)
    print("# tools/decode_image_time.py: medians of %d repeats (grk_decompress: %d), settings alternated within a repeat; %s" %
          (a.repeats, a.ref_repeats, torch.cuda.get_device_name(0)))
    files = {}
    for name, S, T, flags in (("one tile %d^2 x 3, PLT" % S1, S1, S1, G.CS_PLT), ("one tile %d^2 x 3, no PLT" % S1, S1, S1, 0),
                              ("256 tiles, %d^2 x 3, PLT" % S2, S2, S2 // 16, G.CS_PLT)):
        if a.view_only and S != S2:
            continue
        px = image(S)
        cs = np.frombuffer(c.encode_image(G.ImageLayout.make(S, S, T, T), G.TileParams.make(T, T, 3, 8, 5), px, flags), np.uint8)
        info = G.read_header(cs)
        files[name] = (S, T, cs, info)
        print("# %s: %d bytes, %d tiles, %d code-blocks" % (name, cs.size, info.num_tiles, info.num_blocks))
        del px
    views(c, files["256 tiles, %d^2 x 3, PLT" % S2], a.repeats)
    if a.view_only:
        return
    # ---- the reader alone
    for name, (S, T, cs, info) in files.items():
        show("reader alone (header + packets), %s" % name,
             alternated({"%2d thread(s)" % t: (lambda t=t: G.read_packets(cs, info, t)) for t in (1, 16)}, a.repeats))
    # ---- decode_image beside decode_tiles with a prepared table, beside grk_decompress
    R.lib(threads=16)
    for name, (S, T, cs, info) in files.items():
        if "no PLT" in name:
            continue
        tab = G.read_packets(cs, info, 16)
        p = G.layout_tiles(info.layout, info.base)[0]
        nt = info.num_tiles
        d_cs = torch.from_numpy(np.concatenate([cs, np.zeros(64, np.uint8)])).cuda()
        d_out = torch.zeros(3 * S * S, dtype=torch.uint8, device="cuda")
        host = np.zeros((3, S, S), np.uint8)
        pinned = c.host_array(cs.size)
        pinned[:] = cs
        torch.cuda.synchronize()

        def tiles_prepared():
            c.decode_device(p, nt, tab["rows"], d_cs.data_ptr(), cs.size, d_out.data_ptr())
            c.decode_status()

        def image_device():
            c.decode_image_device(pinned, d_out.data_ptr(), d_out.numel())
            c.decode_status()

        def image_device_pageable():
            c.decode_image_device(cs, d_out.data_ptr(), d_out.numel())
            c.decode_status()

        def image_host():
            c._check(c._L.grk_amd_decode_image(c._h, cs.ctypes.data, cs.size, host.ctypes.data, host.nbytes, 0), "decode_image")

        show("decode, %s" % name, alternated({
            "decode_tiles, table prepared, bytes resident (device px)": tiles_prepared,
            "decode_image, device pixels, codestream in pinned memory": image_device,
            "decode_image, device pixels, codestream in pageable memory": image_device_pageable,
            "decode_image, host pixels (pageable)": image_host}, a.repeats))
        assert np.array_equal(host[:, :64, :64], image(S)[:, :64, :64])
        if R.have_ref():
            show("", alternated({"grk_decompress (oracle/_ref), 16 threads": lambda: R.decode(cs.tobytes(), 3, S, S)}, a.ref_repeats))
        del d_cs, d_out, host
    # ---- the two kernels beside a plain copy
    rng = np.random.default_rng(3)
    lens = rng.integers(64, 2048, size=65536).astype(np.uint32)               # pieces as a layer leaves them: ~1 KB
    moves = np.zeros(lens.size, MOVE_DTYPE)
    moves["len"], moves["kind"] = lens, 1
    moves["dst"] = np.concatenate([[0], np.cumsum(lens.astype(np.int64))[:-1]])
    total = int(lens.sum())
    moves["src"] = moves["dst"][rng.permutation(lens.size)] % (total - 2048)
    d_src = torch.randint(0, 255, (total,), dtype=torch.uint8, device="cuda")
    d_dst = torch.zeros(total, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def gather():
        c.gather_device(moves, d_src.data_ptr(), total, d_dst.data_ptr(), total)
        c.synchronize()

    def plain():
        d_dst.copy_(d_src)
        torch.cuda.synchronize()

    empty = moves.copy()
    empty["len"] = 0

    def gather_nothing():
        c.gather_device(empty, d_src.data_ptr(), total, d_dst.data_ptr(), total)
        c.synchronize()

    show("gather: %d pieces of 64..2047 bytes, %.1f MB (a call uploads its move list first: %d bytes)" % (lens.size, total / 1e6, moves.nbytes),
         alternated({"KG gather (the call: list upload + kernel)": gather, "the same call with every length 0 (list upload + launch alone)": gather_nothing,
                     "plain device-to-device copy of the same bytes": plain}, a.repeats), total)
    S, T = S2, S2 // 16
    d_tiles = torch.randint(0, 255, (3 * S * S,), dtype=torch.uint8, device="cuda")
    d_img = torch.zeros(3 * S * S, dtype=torch.uint8, device="cuda")
    rects = [(x * T, y * T) for y in range(16) for x in range(16)]
    torch.cuda.synchronize()

    def place():
        c.place_tiles_device(d_tiles.data_ptr(), 256, T, T, 3, 1, rects, d_img.data_ptr(), S, S)
        c.synchronize()

    def plain2():
        d_img.copy_(d_tiles)
        torch.cuda.synchronize()

    show("placement: 256 tiles of %d^2 x 3 bytes into %d^2 x 3" % (T, S),
         alternated({"KP placement": place, "plain device-to-device copy of the same bytes": plain2}, a.repeats), 3 * S * S)


if __name__ == "__main__":
    main()
