#!/usr/bin/env python3
"""A rate-targeted encode that leaves its file in device memory (grk_amd_encode_surface_rate_device) beside the host-memory call
(grk_amd_encode_surface_rate): 4096 x 4096 x 3, 8 bits, an I444 surface resident in device memory, one tile, reversible HT, 5 levels,
the target at half the plain file (the size of profiles/rate_paths.txt).  Per call: min / median / max ms of --repeats (7) runs, the two
calls alternated within each repeat, host wall clock around a synchronised call; the rounds; the Tier-2 passes that ran on the device
and the bytes of coded blocks that crossed the link (grk_amd_rate_device_counters; for the host-memory call: the coded bytes of
every round's merge, which is each round's block bytes).  Then KT1 alone on the call's own tables: grk_amd_stage_assemble (the
constant zero-bit-plane tree) against grk_amd_stage_assemble_msbs (the general one) over the rate-targeted table of the same image as
ONE tile of grk_amd_encode_tiles_rate -- whole stage calls, upload included, so the difference is the header kernel's.

    python tools/rate_device_time.py [--repeats 7] [--size 4096] >> profiles/rate_device.txt
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
import synth  # noqa: E402


def alternated_spread(settings, repeats):
    """settings: {name: fn} -> {name: (min, median, max) ms}; every repeat runs each setting once, in turn"""
    ms = {k: [] for k in settings}
    for fn in settings.values():
        fn()                                            # warm
    for _ in range(repeats):
        for k, fn in settings.items():
            t0 = time.perf_counter()
            fn()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    return {k: (float(np.min(v)), float(np.median(v)), float(np.max(v))) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--size", type=int, default=4096)
    a = ap.parse_args()
    S = a.size
    c = G.Context(0)
    layout = G.ImageLayout.make(S, S)
    base = G.TileParams.make(1, 1, 3, 8, 5, mct=False)
    surface, sampling, nbytes = G.Surface.make("I444", layout)
    px = synth.g2(3, S, S, 8)
    buf = np.zeros(nbytes, np.uint8)
    surface.scatter(buf, [px[k] for k in range(3)], 1)
    d_buf = torch.from_numpy(buf).cuda()
    args = (layout, base, sampling, surface, d_buf.data_ptr())
    plain = c.encode_surface(*args, cap=nbytes)
    target = len(plain) // 2
    kw = dict(cap=nbytes, max_drop=6, allow_skip=True)
    want, wres = c.encode_surface_rate(*args, target, **kw)
    d_file, n, res = c.encode_surface_rate_device(*args, target, **kw)
    import gpuutil as U   # (the file is the context's: copied down for the comparison alone)
    assert U.from_dev_ptr(d_file, n).tobytes() == want, "the device file is not the host-memory call's"
    passes, fetched = c.rate_device_counters()
    print("%d x %d x 3, 8 bits, I444 in device memory, one tile, 5/3, 5 levels; plain file %d bytes, target %d, file %d bytes in %d round(s)"
          % (S, S, len(plain), target, n, res.passes))
    t = alternated_spread({"grk_amd_encode_surface_rate (file in host memory)": lambda: c.encode_surface_rate(*args, target, **kw),
                           "grk_amd_encode_surface_rate_device (file in device memory)": lambda: c.encode_surface_rate_device(*args, target, **kw)},
                          a.repeats)
    for k, (lo, med, hi) in t.items():
        print("    %-62s min %9.3f  median %9.3f  max %9.3f ms" % (k, lo, med, hi))
    print("    host-memory call: Tier-2 on the host, %d bytes of coded blocks across the link (%d round(s))" % (wres.block_bytes * wres.passes, wres.passes))
    print("    _device call:     %d Tier-2 pass(es) on the device, %d bytes of coded blocks across the link" % (passes, fetched))
    # ---- KT1 alone: the general instance against the constant one on the same table
    p = G.TileParams.make(S, S, 3, 8, 5, mct=False)
    d_px = torch.from_numpy(np.ascontiguousarray(px).reshape(-1)).cuda()
    plain_table, _ = c.encode_tiles(p, 1, d_px.data_ptr(), True)
    table, tot, _ = c.encode_tiles_rate(p, 1, d_px.data_ptr(), True, int(plain_table["length"].sum()) // 2, 6, True)
    coded = c.fetch_coded(tot)
    t = alternated_spread({"grk_amd_stage_assemble (constant tree)": lambda: c.stage_assemble(p, [0], table, coded),
                           "grk_amd_stage_assemble_msbs (general tree)": lambda: c.stage_assemble_msbs(p, [0], table, coded)}, a.repeats)
    print("the stage calls over the rate-targeted table of the same image as one tile (%d blocks, %d coded bytes uploaded by each):" % (len(table), tot))
    for k, (lo, med, hi) in t.items():
        print("    %-62s min %9.3f  median %9.3f  max %9.3f ms" % (k, lo, med, hi))
    sys.stdout.flush()


if __name__ == "__main__":
    main()
