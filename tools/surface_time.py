#!/usr/bin/env python3
"""What a video surface costs on its way into and out of a codestream (grk_amd_encode_surface / grk_amd_decode_surface): a 7680 x 4320
NV12 8-bit frame resident in device memory, one tile, reversible HT, 5 levels -- in place, staged (GRK_AMD_SURFACE_DIRECT=0), and what
a caller had to do before these calls existed (encode: de-interleave the chroma on the device with torch, copy the three planes to
the host, grk_amd_encode_image_subsampled; decode: grk_amd_decode_image to tight device planes, then a torch interleave) -- those entry
points are unchanged, so one library times all three.  And the two kernels alone beside a plain device-to-device copy of the same
bytes.  Then the same frame with 10-bit samples as P010 (two-byte containers, the sample in the high bits): grk_amd_encode_surface /
grk_amd_decode_surface on the P010 surface (always staged: KS / KD shift on the way) beside what a caller had to do without the
shift -- a torch shift pass over the frame and the LSB-aligned call -- and beside the staged LSB-aligned 16-bit NV12 calls, whose
chroma takes the 16-byte two-byte forms of step 2.  --sixteen-only runs just those staged 16-bit NV12 rows, with min and max: they
work on a library without the shift as well (GRK_AMD_LIB, tools/build_variant.sh), which is how this tree and its parent commit are
compared.  --t2 runs the rows of profiles/surface_t2.txt alone, with min / median / max: the 8K NV12 8-bit frame and the 8K P010
frame, device-resident, encoded by the default route (Tier-2 on the device) and under GRK_AMD_IMAGE_T2=host (the host writer), with
grk_amd_encode_surface_device (the file stays in device memory) and a plain device-to-device copy of the file's bytes beside them;
on a library without these (the parent commit's: GRK_AMD_LIB) the first two rows are the same host route and the third is left out.
Medians of --repeats (7) on one box, the variants alternated within each repeat; host wall clock around a synchronised call.

    python tools/surface_time.py [--repeats 7] [--small] [--sixteen-only] > profiles/surface.txt
    python tools/surface_time.py --t2 [--label tree] >> profiles/surface_t2.txt
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


def alternated_spread(settings, repeats):
    """as alternated: {name: (min, median, max) ms}"""
    ms = {k: [] for k in settings}
    for fn in settings.values():
        fn()
    for _ in range(repeats):
        for k, fn in settings.items():
            t0 = time.perf_counter()
            fn()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    return {k: (float(np.min(v)), float(np.median(v)), float(np.max(v))) for k, v in ms.items()}


def plane(w, h, seed, prec=8):
    base = synth.g2(1, min(h, 2048), min(w, 2048), prec, seed=seed)[0]
    return np.ascontiguousarray(np.tile(base, ((h + base.shape[0] - 1) // base.shape[0], (w + base.shape[1] - 1) // base.shape[1]))[:h, :w])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--small", action="store_true", help="1920 x 1080 instead of 7680 x 4320 (a quick look)")
    ap.add_argument("--sixteen-only", action="store_true", help="only the staged 16-bit NV12 rows, min / median / max (any library)")
    ap.add_argument("--t2", action="store_true", help="only the Tier-2 route rows (profiles/surface_t2.txt), min / median / max (any library)")
    ap.add_argument("--label", default="tree", help="what --sixteen-only's and --t2's lines are called")
    a = ap.parse_args()
    W, H = (1920, 1080) if a.small else (7680, 4320)
    c = G.Context(0)
    layout = G.ImageLayout.make(W, H)
    if a.sixteen_only:
        sixteen_bit(c, a, layout, W, H)
        return
    if a.t2:
        tier2_routes(c, a, layout, W, H)
        return
    print("# tools/surface_time.py: medians of %d repeats, variants alternated within a repeat; %s" % (a.repeats, torch.cuda.get_device_name(0)))
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
    sixteen_bit(c, a, layout, W, H)


def tier2_routes(c, a, layout, W, H):
    """the encode's Tier-2 routes: device-resident NV12 8-bit and P010 frames, the default route, GRK_AMD_IMAGE_T2=host, the _device call"""
    have_device = hasattr(c._L, "grk_amd_encode_route_counters")
    for fmt, prec in (("NV12", 8), ("P010", 10)):
        surface, sampling, nbytes = G.Surface.make(fmt, layout, None if fmt == "P010" else prec, 0)
        bps = (prec + 7) // 8
        base = G.TileParams.make(1, 1, 3, prec, 5, mct=False)
        planes = [plane(W, H, 1, prec), plane(W // 2, H // 2, 2, prec), plane(W // 2, H // 2, 3, prec)]
        frame = np.zeros(nbytes, np.uint8)
        surface.scatter(frame, planes, bps)
        d_frame = torch.from_numpy(frame).cuda()
        torch.cuda.synchronize()
        files, counters = {}, {}

        def enc(host):
            def run():
                if host:
                    os.environ["GRK_AMD_IMAGE_T2"] = "host"
                before = c.encode_route_counters() if have_device else (0, 0)
                try:
                    files[host] = c.encode_surface(layout, base, sampling, surface, d_frame.data_ptr(), cap=nbytes)
                finally:
                    os.environ.pop("GRK_AMD_IMAGE_T2", None)
                after = c.encode_route_counters() if have_device else (0, 0)
                counters[host] = (after[0] - before[0], after[1] - before[1])
            return run

        def enc_device():
            files["device"] = c.encode_surface_device(layout, base, sampling, surface, d_frame.data_ptr(), cap=nbytes)

        settings = {"encode_surface 8K %s, default route" % fmt: enc(False), "encode_surface 8K %s, GRK_AMD_IMAGE_T2=host" % fmt: enc(True)}
        if have_device:
            settings["encode_surface_device 8K %s (file stays in device memory)" % fmt] = enc_device
        enc(False)()
        d_copy = torch.zeros(len(files[False]), dtype=torch.uint8, device="cuda")
        d_src = torch.zeros(len(files[False]), dtype=torch.uint8, device="cuda")

        def plain_copy():
            d_copy.copy_(d_src)
            torch.cuda.synchronize()

        settings["plain device-to-device copy of the file's %d bytes" % len(files[False])] = plain_copy
        res = alternated_spread(settings, a.repeats)
        assert files[False] == files[True]
        if have_device:
            assert counters[False] == (1, 0) and counters[True] == (0, 1), counters
            import gpuutil
            assert gpuutil.from_dev_ptr(*files["device"]).tobytes() == files[False]
        for k, (lo, med, hi) in res.items():
            print("    %s | %-66s min %9.3f  median %9.3f  max %9.3f ms" % (a.label, k, lo, med, hi))
        sys.stdout.flush()


def sixteen_bit(c, a, layout, W, H):
    """the 10-bit frame: P010 beside a torch shift pass + the LSB-aligned call, and the staged LSB-aligned 16-bit NV12 calls"""
    prec, shift = 10, 6
    nv12, sampling, nbytes = G.Surface.make("NV12", layout, prec, 0)
    base = G.TileParams.make(1, 1, 3, prec, 5, mct=False)
    planes = [plane(W, H, 1, prec), plane(W // 2, H // 2, 2, prec), plane(W // 2, H // 2, 3, prec)]
    lsb = np.zeros(nbytes, np.uint8)
    nv12.scatter(lsb, planes, 2)
    d_lsb = torch.from_numpy(lsb).cuda()
    d_out = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    files = {}

    def staged(fn):
        def run():
            os.environ["GRK_AMD_SURFACE_DIRECT"] = "0"
            try:
                fn()
            finally:
                os.environ.pop("GRK_AMD_SURFACE_DIRECT", None)
        return run

    def enc16():
        files["nv12"] = c.encode_surface(layout, base, sampling, nv12, d_lsb.data_ptr(), cap=nbytes)

    enc16()
    pinned = c.host_array(len(files["nv12"]))
    pinned[:] = np.frombuffer(files["nv12"], np.uint8)

    def dec16():
        c.decode_surface(pinned, nv12, d_out.data_ptr(), cap=nbytes)
        c.decode_status()

    if a.sixteen_only:
        res = alternated_spread({"encode_surface 8K NV12 16-bit containers, staged": staged(enc16),
                                 "decode_surface 8K NV12 16-bit containers, staged": staged(dec16)}, a.repeats)
        assert np.array_equal(d_out.cpu().numpy(), lsb)
        for k, (lo, med, hi) in res.items():
            print("    %s | %-58s min %9.3f  median %9.3f  max %9.3f ms" % (a.label, k, lo, med, hi))
        return
    p010, _, n010 = G.Surface.make("P010", layout, pitch=0)
    assert n010 == nbytes
    msb = np.zeros(nbytes, np.uint8)
    p010.scatter(msb, planes, 2)
    d_msb = torch.from_numpy(msb).cuda()
    d_tmp = torch.zeros(nbytes // 2, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    print("# P010 %d x %d, 10 bits: %d bytes; one tile, reversible HT, 5 levels" % (W, H, nbytes))

    def enc_p010():
        files["p010"] = c.encode_surface(layout, base, sampling, p010, d_msb.data_ptr(), cap=nbytes)

    def enc_shift_pass(fn):
        def run():
            # (int16 views: torch has no shifts of uint16; the arithmetic shift's sign bits are masked off)
            torch.bitwise_and(torch.bitwise_right_shift(d_msb.view(torch.int16), shift), (1 << prec) - 1, out=d_tmp)
            torch.cuda.synchronize()
            files["shifted"] = c.encode_surface(layout, base, sampling, nv12, d_tmp.data_ptr(), cap=nbytes)
        return fn(run) if fn else run

    res = alternated({"encode_surface, P010 (staged, KS shifts)": enc_p010,
                      "before: torch shift pass + encode_surface NV12 16-bit, in place": enc_shift_pass(None),
                      "before: torch shift pass + encode_surface NV12 16-bit, staged": enc_shift_pass(staged),
                      "encode_surface, NV12 16-bit LSB-aligned, in place": enc16,
                      "encode_surface, NV12 16-bit LSB-aligned, staged": staged(enc16)}, a.repeats)
    assert files["p010"] == files["shifted"] == files["nv12"]
    show("encode, device-resident 10-bit frame -> file of %d bytes in host memory" % len(files["p010"]), res)
    d_p010 = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    d_shifted = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def dec_p010():
        c.decode_surface(pinned, p010, d_p010.data_ptr(), cap=nbytes)
        c.decode_status()

    def dec_shift_pass(fn):
        def decode():
            c.decode_surface(pinned, nv12, d_shifted.data_ptr(), cap=nbytes)
            c.decode_status()
        decode = fn(decode) if fn else decode

        def run():
            decode()
            v = d_shifted.view(torch.int16)
            torch.bitwise_left_shift(v, shift, out=v)
            torch.cuda.synchronize()
        return run

    res = alternated({"decode_surface, P010 (staged, KD shifts)": dec_p010,
                      "before: decode_surface NV12 16-bit, in place + torch shift pass": dec_shift_pass(None),
                      "before: decode_surface NV12 16-bit, staged + torch shift pass": dec_shift_pass(staged),
                      "decode_surface, NV12 16-bit LSB-aligned, in place": dec16,
                      "decode_surface, NV12 16-bit LSB-aligned, staged": staged(dec16)}, a.repeats)
    assert np.array_equal(d_p010.cpu().numpy(), msb) and np.array_equal(d_shifted.cpu().numpy(), msb) and np.array_equal(d_out.cpu().numpy(), lsb)
    show("decode, file in pinned host memory -> device-resident 10-bit frame", res)


if __name__ == "__main__":
    main()
