"""The two tables of DESIGN.md section 3 on rate-targeted encodes over joint tables (profiles/rate_joint.txt holds a run's output):
(a) 256 x 256 4:2:0, 8 bits, synth.g2 (9/7: clipped as synth.g2_mid), 3 levels, Dmax 6 + SKIP: file bytes / PSNR per plane at 1/2, 1/4, 1/10 of the plain file, 5/3
    and 9/7; and 250 x 190 x 3 in tiles of 128 x 96 (four geometry groups) through grk_amd_encode_image_rate with joint = 1 beside
    joint = 0: file bytes, rounds, the allocator's distortion, PSNR;
(b) a 3840 x 2160 NV12 and a P010 frame in device memory: grk_amd_encode_surface_rate at 1/2, 1/4, 1/10 of the plain file, wall time,
    median of three, beside plain grk_amd_encode_surface of the same frame in the same process, median of five, with the
    grk_amd_enable_timing split of one rate-targeted call (family 9: the allocator; family 2: the block coder's launches).
Usage: python tools/rate_joint_tables.py [a] [b]"""
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import grok_amd as G  # noqa: E402
import synth  # noqa: E402

DMAX = 6
S420 = [(1, 1), (2, 2), (2, 2)]


def planes_of(w, h, sampling, prec, seed=3):
    return [synth.g2(1, -(-h // dy), -(-w // dx), prec, seed=60 + 5 * k + seed)[0] for k, (dx, dy) in enumerate(sampling)]


def table_a(c):
    print("(a) 256 x 256 4:2:0, 3 levels, Dmax 6 + SKIP: target -> file bytes / rounds / PSNR dB of Y, Cb, Cr")
    for tiling, (tw, th) in (("one tile", (256, 256)), ("2x2 tiles of 128", (128, 128))):
        for irrev in (True, False):
            layout = G.ImageLayout.make(256, 256, tw, th)
            base = G.TileParams.make(1, 1, 3, 8, 3, mct=False, irreversible=irrev)
            planes = planes_of(256, 256, S420, 8)
            if irrev:       # (as synth.g2_mid: a decoder refuses the plain 9/7 file of full-range planes without a colour transform)
                planes = [np.clip(pl, 32, 224).astype(pl.dtype) for pl in planes]
            plain = c.encode_image_subsampled(layout, base, S420, planes)
            row = ["plain %d" % len(plain)]
            for div in (2, 4, 10):
                cs, res = c.encode_image_subsampled_rate(layout, base, S420, planes, len(plain) // div, max_drop=DMAX, allow_skip=True)
                back = c.decode_image_planes(cs)
                row.append("1/%d %d / %d / %s" % (div, len(cs), res.passes, " ".join("%.2f" % synth.psnr_db(a, b, 8) for a, b in zip(back, planes))))
            print("  %s, %s: %s" % ("9/7" if irrev else "5/3", tiling, " | ".join(row)))
    print("    250 x 190 x 3 in tiles of 128 x 96 (four geometry groups), grk_amd_encode_image_rate: joint = 1 beside joint = 0 (the split by sample count)")
    px = synth.g2(3, 190, 250, 8)
    layout = G.ImageLayout.make(250, 190, 128, 96)
    for irrev in (True, False):
        base = G.TileParams.make(128, 96, 3, 8, 3, irreversible=irrev)
        os.environ["GRK_AMD_IMAGE_T2"] = "host"
        plain = c.encode_image(layout, base, px)
        del os.environ["GRK_AMD_IMAGE_T2"]
        for div in (2, 4, 10):
            out = []
            for joint in (1, 0):
                cs, res = c.encode_image_rate(layout, base, px, len(plain) // div, max_drop=DMAX, allow_skip=True, joint=joint)
                out.append("%s %d bytes / %d rounds / distortion %.6g / %.2f dB" % ("joint" if joint else "split", len(cs), res.passes, res.distortion,
                                                                                     synth.psnr_db(c.decode_image(cs), px, 8)))
            print("  %s, plain %d, 1/%d: %s | %s" % ("9/7" if irrev else "5/3", len(plain), div, out[0], out[1]))


def wall(call, n):
    ts = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def table_b(c):
    print("(b) 3840 x 2160 surfaces in device memory, one tile, 5 levels, 9/7, Dmax 6 + SKIP: wall ms of a call, file fetched")
    W, H = 3840, 2160
    layout = G.ImageLayout.make(W, H)
    for fmt, prec in (("NV12", 8), ("P010", 10)):
        bps = (prec + 7) // 8
        surface, sampling, nbytes = G.Surface.make(fmt, layout, pitch=bps * W)
        planes = planes_of(W, H, sampling, prec)
        planes = [np.clip(pl, (1 << prec) // 8, 7 * (1 << prec) // 8).astype(pl.dtype) for pl in planes]        # (as synth.g2_mid)
        buf = np.zeros(nbytes, np.uint8)
        surface.scatter(buf, planes, bps)
        d_buf = torch.from_numpy(buf).cuda()
        base = G.TileParams.make(1, 1, 3, prec, 5, mct=False, irreversible=True)

        def plain_call():
            return c.encode_surface(layout, base, sampling, surface, d_buf.data_ptr(), cap=nbytes)
        plain = plain_call()
        row = ["plain %d bytes %.2f ms" % (len(plain), wall(plain_call, 5))]
        for div in (2, 4, 10):
            def rate_call():
                return c.encode_surface_rate(layout, base, sampling, surface, d_buf.data_ptr(), len(plain) // div, cap=nbytes, max_drop=DMAX,
                                             allow_skip=True)
            cs, res = rate_call()
            ms = wall(rate_call, 3)
            c.enable_timing(True)
            rate_call()
            c.synchronize()
            (a9, n9), (a2, n2) = c.kernel_ms(9), c.kernel_ms(2)
            c.enable_timing(False)
            row.append("1/%d %d bytes, %d rounds, %.1f ms (family 9: %d x %.3f ms; family 2: %d x %.3f ms)" % (div, len(cs), res.passes, ms, n9, a9, n2, a2))
        print("  %s: %s" % (fmt, " | ".join(row)))


if __name__ == "__main__":
    which = sys.argv[1:] or ["a", "b"]
    ctx = G.Context(0)
    if "a" in which:
        table_a(ctx)
    if "b" in which:
        table_b(ctx)
    ctx.close()
