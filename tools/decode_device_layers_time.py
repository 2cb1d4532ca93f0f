#!/usr/bin/env python3
"""What reading a LAYERED codestream that lies in DEVICE memory costs: grk_amd_read_packets_device_ex (KL, KH, KC-L, KF, KP) beside the
host reader on 16 threads over the same bytes, and grk_amd_decode_image_device_ex beside the bounce -- the file copied down into
pinned memory and handed to grk_amd_decode_image.  The files are the reference's own (oracle/_ref: three layers, SOP; it writes no
PLT with layers), each as written -- one serial chain per tile -- and with PLT put in from the SOP positions -- a chain per
precinct.  Part-1 files have an appendix (the _ex decode stages the file: one device-to-device copy), HT files have none.  Device
pixels.  Medians with min..max of --repeats (7) on one box, the settings of a group alternated within each repeat; host wall clock
around a synchronised call.

    python tools/decode_device_layers_time.py [--repeats 7] [--small] > profiles/decode_device_layers.txt
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
import refharness as R  # noqa: E402
import t2layers_cases as K  # noqa: E402
from decode_device_time import alternated, image, show  # noqa: E402


def reference_file(px, T, ht, precincts):
    for k in K.REF_VARS:
        os.environ.pop(k, None)
    os.environ.update(REF_LAYERS="20,10,1", REF_CSTY="2")
    if precincts:
        os.environ["REF_PRECINCTS"] = precincts
    return R.encode(px, 8, TW=T, TH=T, numres=6, ht=ht, mode=1)[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--small", action="store_true", help="2048 / 4096 instead of 8192 / 16384 (a quick look)")
    a = ap.parse_args()
    if not R.have_ref():
        sys.exit("oracle/_ref (the reference) is not built here: it writes the layered files")
    c = G.Context(0)
    S1, S2 = (2048, 4096) if a.small else (8192, 16384)
    print("# tools/decode_device_layers_time.py: medians (min .. max) of %d repeats, settings alternated within a repeat; %s" % (a.repeats, torch.cuda.get_device_name(0)))
    shapes = (("256 tiles, %d^2 x 3" % S2, S2, S2 // 16, None),
              ("one tile %d^2 x 3, 256 x 256 precincts" % S1, S1, S1, "256,256"),
              ("one tile %d^2 x 3" % S1, S1, S1, None))
    px_of = {}
    for shape, S, T, precincts in shapes:
        if S not in px_of:
            px_of.clear()
            px_of[S] = image(S)
        for ht in (1, 0):
            written = reference_file(px_of[S], T, ht, precincts)
            for plt in (0, 1):
                name = "%s, %s, three layers, %s" % (shape, "HT" if ht else "Part-1", "PLT" if plt else "no PLT")
                cs = np.frombuffer(K.plt_from_sop(written) if plt else written, np.uint8)
                info = G.read_header(cs)
                assert info.num_layers == 3
                d_cs = torch.from_numpy(cs.copy()).cuda()
                d_out = torch.zeros(3 * S * S, dtype=torch.uint8, device="cuda")
                pinned = c.host_array(cs.size)
                t_pinned = torch.from_numpy(pinned)
                torch.cuda.synchronize()
                before = c.read_device_counters()
                got = c.read_packets_device_ex(d_cs.data_ptr(), cs.size, info)
                after = c.read_device_counters()
                want = G.read_packets(cs, info, 16)
                assert all(np.array_equal(got[k], want[k]) for k in ("rows", "first_segment", "segments")) and got["appendix_bytes"] == want["appendix_bytes"]
                print("# %s: %d bytes, %d tiles, %d code-blocks, %d chains, %d moves, an appendix of %d bytes" %
                      (name, cs.size, info.num_tiles, info.num_blocks, (after[3] - before[3]) // 2, len(got["moves"]), got["appendix_bytes"]))

                def read_device():
                    c.read_packets_device_ex(d_cs.data_ptr(), cs.size, info)

                def read_host():
                    G.read_packets(cs, info, 16)

                def decode_resident():
                    c.decode_image_resident_ex(d_cs.data_ptr(), cs.size, d_out.data_ptr(), d_out.numel())
                    c.decode_status()

                def bounce():
                    t_pinned.copy_(d_cs)
                    torch.cuda.synchronize()
                    c.decode_image_device(pinned, d_out.data_ptr(), d_out.numel())
                    c.decode_status()

                show("tables, %s" % name, alternated({"grk_amd_read_packets_device_ex, sizes then tables (file in device memory)": read_device,
                                                     "grk_amd_read_packets, 16 threads (file in host memory)": read_host}, a.repeats))
                show("pixels, %s" % name, alternated({"grk_amd_decode_image_device_ex": decode_resident,
                                                     "the bounce: file to pinned memory + grk_amd_decode_image": bounce}, a.repeats))
                assert np.array_equal(d_out[:3 * S * S].view(3, S, S)[:, :64, :64].cpu().numpy(), px_of[S][:, :64, :64])
                del d_cs, d_out, pinned, t_pinned


if __name__ == "__main__":
    main()
