#!/usr/bin/env python3
"""What a video surface costs on its way into and out of a codestream (grk_amd_encode_surface / grk_amd_decode_surface): a 7680 x 4320
NV12 8-bit frame resident in device memory, one tile, reversible HT, 5 levels -- in place, staged (GRK_AMD_SURFACE_DIRECT=0), and what
a caller had to do before these calls existed (encode: de-interleave the chroma on the device with torch, copy the three planes to
the host, grk_amd_encode_image_subsampled; decode: grk_amd_decode_image to tight device planes, then a torch interleave) -- those entry
points are unchanged, so one library times all three.  And the two kernels alone beside a plain device-to-device copy of the same
bytes.  Medians of --repeats (7) on one box, the variants alternated within each repeat; host wall clock around a synchronised call.

    python tools/surface_time.py [--repeats 7] [--small] > profiles/surface.txt
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
        print("    %-74s %9.3f ms%s" % (k, v, "   %7.1f GB/s" % (bytes_moved / v / 1e6) if bytes_moved else ""))
    sys.stdout.flush()


def plane(w, h, seed):
    base = synth.g2(1, min(h, 2048), min(w, 2048), 8, seed=seed)[0]
    return np.ascontiguousarray(np.tile(base, ((h + base.shape[0] - 1) // base.shape[0], (w + base.shape[1] - 1) // base.shape[1]))[:h, :w])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--small", action="store_true", help="1920 x 1080 instead of 7680 x 4320 (a quick look)")
    a = ap.parse_args()
    W, H = (1920, 1080) if a.small else (7680, 4320)
    c = G.Context(0)
    print("# tools/surface_time.py: medians of %d repeats, variants alternated within a repeat; %s" % (a.repeats, torch.cuda.get_device_name(0)))
    layout = G.ImageLayout.make(W, H)
    surface, sampling, nbytes = G.Surface.make("NV12", layout, 8, 0)
    base = G.TileParams.make(1, 1, 3, 8, 5, mct=False)
    planes = [plane(W, H, 1), plane(W // 2, H // 2, 2), plane(W // 2, H // 2, 3)]
    frame = np.zeros(nbytes, np.uint8)
    surface.scatter(frame, planes, 1)
    d_frame = torch.from_numpy(frame).cuda()
    torch.cuda.synchronize()
    print("# NV12 %d x %d: %d bytes; one tile, reversible HT, 5 levels" % (W, H, nbytes))
    files = {}

    def enc(direct):
        def run():
            if direct:
                os.environ.pop("GRK_AMD_SURFACE_DIRECT", None)
            else:
                os.environ["GRK_AMD_SURFACE_DIRECT"] = "0"
            files[direct] = c.encode_surface(layout, base, sampling, surface, d_frame.data_ptr(), cap=nbytes)
            os.environ.pop("GRK_AMD_SURFACE_DIRECT", None)
        return run

    def enc_before():
        y = d_frame[:W * H].reshape(H, W)
        uv = d_frame[W * H:].reshape(H // 2, W // 2, 2)
        cb, cr = uv[:, :, 0].contiguous(), uv[:, :, 1].contiguous()
        files["before"] = c.encode_image_subsampled(layout, base, sampling, [y.cpu().numpy(), cb.cpu().numpy(), cr.cpu().numpy()])

    res = alternated({"encode_surface, in place": enc(True), "encode_surface, staged (GRK_AMD_SURFACE_DIRECT=0)": enc(False),
                      "before: torch de-interleave + 3 planes to the host + encode_image_subsampled": enc_before}, a.repeats)
    assert files[True] == files[False] == files["before"]
    show("encode, device-resident NV12 frame -> file of %d bytes in host memory" % len(files[True]), res)
    cs = np.frombuffer(files[True], np.uint8)
    pinned = c.host_array(cs.size)
    pinned[:] = cs
    d_out = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    d_planes = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    d_nv12 = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def dec(direct):
        def run():
            if direct:
                os.environ.pop("GRK_AMD_SURFACE_DIRECT", None)
            else:
                os.environ["GRK_AMD_SURFACE_DIRECT"] = "0"
            c.decode_surface(pinned, surface, d_out.data_ptr(), cap=nbytes)
            c.decode_status()
            os.environ.pop("GRK_AMD_SURFACE_DIRECT", None)
        return run

    def dec_before():
        c.decode_image_device(pinned, d_planes.data_ptr(), nbytes)
        c.decode_status()
        d_nv12[:W * H] = d_planes[:W * H]
        q = W * H // 4
        d_nv12[W * H:].reshape(q, 2)[:, 0] = d_planes[W * H:W * H + q]
        d_nv12[W * H:].reshape(q, 2)[:, 1] = d_planes[W * H + q:]
        torch.cuda.synchronize()

    res = alternated({"decode_surface, in place": dec(True), "decode_surface, staged (GRK_AMD_SURFACE_DIRECT=0)": dec(False),
                      "before: decode_image to tight device planes + torch interleave": dec_before}, a.repeats)
    assert np.array_equal(d_out.cpu().numpy(), frame) and np.array_equal(d_nv12.cpu().numpy(), frame)
    show("decode, file in pinned host memory -> device-resident NV12 frame", res)
    # ---- the two kernels beside a plain copy: the whole frame as one unit per run
    d_tiles = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    y_comp = [(surface.comp[0].offset, surface.comp[0].row_pitch, 1)]
    uv_comp = [(surface.comp[k].offset, surface.comp[k].row_pitch, 2) for k in (1, 2)]
    torch.cuda.synchronize()

    def cut():
        c.surface_cut_device(d_frame.data_ptr(), nbytes, y_comp, 1, 1, W, H, [(0, 0)], d_tiles.data_ptr())
        c.surface_cut_device(d_frame.data_ptr(), nbytes, uv_comp, 1, 1, W // 2, H // 2, [(0, 0)], d_tiles.data_ptr() + W * H)
        c.synchronize()

    def place():
        c.surface_place_device(d_tiles.data_ptr(), 1, W, H, 1, [(0, 0)], y_comp, d_out.data_ptr(), nbytes)
        c.surface_place_device(d_tiles.data_ptr() + W * H, 1, W // 2, H // 2, 1, [(0, 0)], uv_comp, d_out.data_ptr(), nbytes)
        c.synchronize()

    def cut_uv():
        c.surface_cut_device(d_frame.data_ptr(), nbytes, uv_comp, 1, 1, W // 2, H // 2, [(0, 0)], d_tiles.data_ptr() + W * H)
        c.synchronize()

    def place_uv():
        c.surface_place_device(d_tiles.data_ptr() + W * H, 1, W // 2, H // 2, 1, [(0, 0)], uv_comp, d_out.data_ptr(), nbytes)
        c.synchronize()

    def plain(n):
        def run():
            d_out[:n].copy_(d_frame[:n])
            torch.cuda.synchronize()
        return run

    show("the kernels alone, the whole frame (two calls each: Y, Cb/Cr; a call uploads its origins first)",
         alternated({"KS cut, Y + Cb/Cr": cut, "KD place, Y + Cb/Cr": place, "plain device-to-device copy of the same bytes": plain(nbytes)}, a.repeats), nbytes)
    assert np.array_equal(d_out.cpu().numpy(), frame)
    show("the kernels alone, the interleaved chroma plane only",
         alternated({"KS cut, Cb/Cr (de-interleave)": cut_uv, "KD place, Cb/Cr (merged stores)": place_uv,
                     "plain device-to-device copy of the same bytes": plain(nbytes - W * H)}, a.repeats), nbytes - W * H)


if __name__ == "__main__":
    main()
