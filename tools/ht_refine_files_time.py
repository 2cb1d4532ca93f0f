#!/usr/bin/env python3
"""What K5c costs inside a whole-image decode, and what reading refinement passes costs the readers: a 4096 x 4096 x 3 8-bit
reversible HTJ2K file (16 tiles of 1024^2, five levels, 64 x 64 blocks, PLT, one layer) whose blocks all have three passes, beside
the same samples cleanup-only, through grk_amd_decode_image (codestream in pinned host memory, device pixels),
grk_amd_decode_image_device_ex (codestream in device memory) and the device readers (tables: two calls, sizes then tables).  Two more
files isolate the parts: the cleanup-only bytes with every block SIGNALLING three passes over a refinement segment of 0 bytes (the
second reading, the segment lists, the refinement table's upload and its synchronise, int32 planes -- and no K5c work), and the
cleanup-only file decoded with the int16 planes switched off (int32 planes alone).  With GRK_AMD_LIB naming a library built from the
commit before, the same program gives that commit's figures for the cleanup-only file.  Medians and the range of --repeats (9) on
one box, the settings of a group alternated within each repeat; host wall clock around a call that ends synchronised.

The files are written by tests/t2ht_model.py from 48 distinct blocks per block size (the oracle's encoders, seeded), repeated.

    python tools/ht_refine_files_time.py [--repeats 9] [--size 4096] [--cache DIR] >> profiles/ht_refine_files.txt
"""
import argparse
import os
import pickle
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import grok_amd as G  # noqa: E402
import t2ht_model as HM  # noqa: E402
from test_oracle_ht_refine import make_block, code_block  # noqa: E402


def alternated(settings, repeats):
    """settings: {name: fn} -> {name: (median, min, max) ms}, every repeat runs each setting once, in turn"""
    ms = {k: [] for k in settings}
    for fn in settings.values():
        fn()                                            # warm
    for _ in range(repeats):
        for k, fn in settings.items():
            t0 = time.perf_counter()
            fn()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    return {k: (float(np.median(v)), float(min(v)), float(max(v))) for k, v in ms.items()}


def show(title, res):
    print(title)
    for k, (med, lo, hi) in res.items():
        print("    %-74s %9.3f ms   (%.3f .. %.3f)" % (k, med, lo, hi))
    sys.stdout.flush()


def files(S, T):
    """-> {kind: bytes}: three-pass, cleanup-only, three passes signalled over 0 refinement bytes"""
    base = G.TileParams.make(T, T, 3, 8, 5, cblk=(6, 6))
    layout = G.ImageLayout.make(S, S, T, T)
    rng = np.random.default_rng(4096)
    pool = {}
    tables = {"three-pass": [], "cleanup-only": [], "three-pass-signalled": []}
    for tp in G.layout_tiles(layout, base):
        rows = {k: [] for k in tables}
        for i, b in enumerate(G.tile_layout(tp)[0]):
            key = (b.x1 - b.x0, b.y1 - b.y0, int(b.kmax), i % 48)
            if key not in pool:
                mag, sign = make_block(rng, key[0], key[1], min(key[2], 10), 1 if i % 3 else 0)
                pool[key] = code_block(mag, sign, key[2], 3)[:2]
            cup, seg = pool[key]
            mm = int(b.kmax) - 1
            rows["three-pass"].append(dict(zbp=mm, layers={0: (3, [len(cup), len(seg)])}, data=cup + seg))
            rows["cleanup-only"].append(dict(zbp=mm, layers={0: (1, [len(cup)])}, data=cup))
            rows["three-pass-signalled"].append(dict(zbp=mm, layers={0: (3, [len(cup), 0])}, data=cup))
        for k in tables:
            tables[k].append(rows[k])
    return {k: np.frombuffer(HM.build(base, S, S, 1, 0, G.CS_PLT, t, tile=(T, T))[0], np.uint8) for k, t in tables.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--cache", default=None)
    a = ap.parse_args()
    S, T = a.size, min(a.size, 1024)
    path = a.cache and os.path.join(a.cache, "ht_refine_files_%d.pickle" % S)
    if path and os.path.exists(path):
        f = pickle.load(open(path, "rb"))
    else:
        t0 = time.perf_counter()
        f = files(S, T)
        print("(files written in %.1f s)" % (time.perf_counter() - t0))
        if path:
            os.makedirs(a.cache, exist_ok=True)
            pickle.dump(f, open(path, "wb"))
    assert torch.cuda.is_available(), "this measures on the GPU"
    c = G.Context(0)
    new = hasattr(G.lib(), "grk_amd_read_packets_refine")
    lib = os.path.basename(os.path.dirname(G.lib_path()))
    print("== %d x %d x 3, 8-bit 5/3, %d tiles; library: %s (%s); %d repeats" % (S, S, (S // T) ** 2, lib, "this change" if new else "the commit before", a.repeats))
    for k, v in f.items():
        print("    %-22s %10d bytes" % (k, v.size))
    kinds = list(f) if new else ["cleanup-only"]
    pinned, dev = {}, {}
    for k in kinds:
        pinned[k] = c.host_array(f[k].size)
        pinned[k][:] = f[k]
        dev[k] = torch.from_numpy(f[k].copy()).cuda()
    d_out = torch.zeros(3 * S * S, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    out = {}

    def image(k):
        c.decode_image_device(pinned[k], d_out.data_ptr(), d_out.numel())
        c.decode_status()

    def resident(k):
        c.decode_image_resident_ex(dev[k].data_ptr(), dev[k].numel(), d_out.data_ptr(), d_out.numel())
        c.decode_status()

    def planes32(fn, k):
        c.set_decode_planes16(0)
        try:
            fn(k)
        finally:
            c.set_decode_planes16(1)

    for name, fn in (("grk_amd_decode_image", image), ("grk_amd_decode_image_device_ex", resident)):
        settings = {"%s, %s" % (name, k): (lambda fn=fn, k=k: fn(k)) for k in kinds}
        settings["%s, cleanup-only, int16 planes off" % name] = lambda fn=fn: planes32(fn, "cleanup-only")
        for k in kinds:                                  # the decodes of one sample set agree (device pixels, first repeat)
            fn(k)
            out[k] = d_out.cpu().numpy().copy()
        show("%s, device pixels" % name, alternated(settings, a.repeats))
        if new:
            assert np.array_equal(out["cleanup-only"], out["three-pass-signalled"]), "a refinement segment of 0 bytes decodes as the cleanup pass alone"
    readers = {"grk_amd_read_packets_device_parts, cleanup-only": lambda: c.read_packets_device_parts(dev["cleanup-only"].data_ptr(), dev["cleanup-only"].numel())}
    if new:
        readers["grk_amd_read_packets_device_refine, cleanup-only"] = lambda: c.read_packets_device_refine(dev["cleanup-only"].data_ptr(), dev["cleanup-only"].numel())
        readers["grk_amd_read_packets_device_refine, three-pass"] = lambda: c.read_packets_device_refine(dev["three-pass"].data_ptr(), dev["three-pass"].numel())
        t0 = time.perf_counter()
        G.read_packets_refine(f["three-pass"], threads=16)
        print("    (host: grk_amd_read_packets_refine, three-pass, 16 threads, first call: %.3f ms)" % ((time.perf_counter() - t0) * 1e3))
    show("the device readers' tables (two calls: sizes, then tables)", alternated(readers, a.repeats))
    rows = len(c.read_packets_device_parts(dev["cleanup-only"].data_ptr(), dev["cleanup-only"].numel())["rows"])
    print("    (%d rows: the refinement table of a batch is 8 bytes a row, uploaded from pageable memory and synchronised)" % rows)


if __name__ == "__main__":
    main()
