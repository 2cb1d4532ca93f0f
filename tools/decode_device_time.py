#!/usr/bin/env python3
"""What reading a codestream that lies in DEVICE memory costs: grk_amd_read_packets_device (KL, KH, KC) beside the host reader on 16
threads over the same bytes, and grk_amd_decode_image_device beside the bounce -- the file copied down into pinned memory and handed
to grk_amd_decode_image, the only way from the same starting point to the same pixels without the device reader.  Device pixels.
Medians with min..max of --repeats (7) on one box, the settings of a group alternated within each repeat; host wall clock around a
synchronised call.

    python tools/decode_device_time.py [--repeats 7] [--small] > profiles/decode_device.txt
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


def alternated(settings, repeats):
    ms = {k: [] for k in settings}
    for fn in settings.values():
        fn()                                            # warm
    for _ in range(repeats):
        for k, fn in settings.items():
            t0 = time.perf_counter()
            fn()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    return {k: (float(np.median(v)), float(np.min(v)), float(np.max(v))) for k, v in ms.items()}


def show(title, res):
    print(title)
    for k, (med, lo, hi) in res.items():
        print("    %-66s %9.3f ms  (%.3f .. %.3f)" % (k, med, lo, hi))
    sys.stdout.flush()


def image(S):
    base = synth.g2(3, min(S, 2048), min(S, 2048), 8)
    return np.ascontiguousarray(np.tile(base, (1, S // base.shape[1], S // base.shape[2])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--small", action="store_true", help="2048 / 4096 instead of 8192 / 16384 (a quick look)")
    a = ap.parse_args()
    c = G.Context(0)
    S1, S2 = (2048, 4096) if a.small else (8192, 16384)
    print("# tools/decode_device_time.py: medians (min .. max) of %d repeats, settings alternated within a repeat; %s" % (a.repeats, torch.cuda.get_device_name(0)))
    cases = (("one tile %d^2 x 3, PLT" % S1, S1, S1, G.CS_PLT, None),
             ("one tile %d^2 x 3, no PLT" % S1, S1, S1, 0, None),
             ("one tile %d^2 x 3, 256 x 256 precincts, PLT" % S1, S1, S1, G.CS_PLT, [(8, 8)] * 6),
             ("256 tiles, %d^2 x 3, PLT" % S2, S2, S2 // 16, G.CS_PLT, None),
             ("256 tiles, %d^2 x 3, no PLT" % S2, S2, S2 // 16, 0, None))
    px_of = {}
    for name, S, T, flags, precincts in cases:
        if S not in px_of:
            px_of.clear()
            px_of[S] = image(S)
        try:
            cs = np.frombuffer(c.encode_image(G.ImageLayout.make(S, S, T, T), G.TileParams.make(T, T, 3, 8, 5, precincts=precincts), px_of[S], flags), np.uint8)
        except RuntimeError as e:
            print("# %s: not encoded (%s)" % (name, e))
            continue
        info = G.read_header(cs)
        d_cs = torch.from_numpy(cs.copy()).cuda()
        d_out = torch.zeros(3 * S * S, dtype=torch.uint8, device="cuda")
        pinned = c.host_array(cs.size)
        t_pinned = torch.from_numpy(pinned)
        torch.cuda.synchronize()
        before = c.read_device_counters()
        rows = c.read_packets_device(d_cs.data_ptr(), cs.size, info)
        after = c.read_device_counters()
        assert np.array_equal(rows, G.read_packets(cs, info, 16)["rows"])
        print("# %s: %d bytes, %d tiles, %d code-blocks, %d chains; the first read copies %d bytes down, %d up" %
              (name, cs.size, info.num_tiles, info.num_blocks, after[3] - before[3], after[0] - before[0], after[1] - before[1]))

        def read_device():
            c.read_packets_device(d_cs.data_ptr(), cs.size, info)

        def read_host():
            G.read_packets(cs, info, 16)

        def decode_resident():
            c.decode_image_resident(d_cs.data_ptr(), cs.size, d_out.data_ptr(), d_out.numel())
            c.decode_status()

        def bounce():
            t_pinned.copy_(d_cs)
            torch.cuda.synchronize()
            c.decode_image_device(pinned, d_out.data_ptr(), d_out.numel())
            c.decode_status()

        show("rows, %s" % name, alternated({"grk_amd_read_packets_device (file in device memory)": read_device,
                                           "grk_amd_read_packets, 16 threads (file in host memory)": read_host}, a.repeats))
        show("pixels, %s" % name, alternated({"grk_amd_decode_image_device": decode_resident,
                                             "the bounce: file to pinned memory + grk_amd_decode_image": bounce}, a.repeats))
        want = px_of[S][:, :64, :64]
        assert np.array_equal(d_out[:3 * S * S].view(3, S, S)[:, :64, :64].cpu().numpy(), want)
        del d_cs, d_out, pinned, t_pinned


if __name__ == "__main__":
    main()
