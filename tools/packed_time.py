#!/usr/bin/env python3
"""What a packed 4:2:2 frame costs on its way into and out of a codestream (grk_amd_encode_packed / grk_amd_decode_packed): a 7680 x
4320 frame resident in device memory as UYVY (8 bits) and as v210 (10 bits), one tile, reversible HT, 5 levels -- beside what a caller
had to do before these calls existed (encode: unpack the frame to three tight planes with torch, grk_amd_encode_surface on them as
I422; decode: grk_amd_decode_surface onto I422 planes, then a torch pack), and the two kernels alone (KU, KK: kernels_packed.hip)
beside a plain device-to-device copy of the frame's bytes.  The protocol of tools/surface_time.py: medians of --repeats (7) on one
box, the variants alternated within each repeat, host wall clock around a synchronised call.

    python tools/packed_time.py [--repeats 7] [--small] >> profiles/packed.txt
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
import packedref as R  # noqa: E402
from surface_time import alternated, plane, show  # noqa: E402


def torch_unpack(fmt, d_frame, W, H, d_planes):
    """the frame -> tight planes Y, Cb, Cr at d_planes (uint8 / int16), with torch"""
    cw = W // 2
    if fmt == R.UYVY:
        m = d_frame.reshape(H, cw, 4)
        d_planes[:W * H].reshape(H, cw, 2).copy_(m[:, :, 1::2])
        d_planes[W * H:W * H + cw * H].reshape(H, cw).copy_(m[:, :, 0])
        d_planes[W * H + cw * H:].reshape(H, cw).copy_(m[:, :, 2])
        return
    w = d_frame.view(torch.int32).reshape(H, W // 6, 4)
    f = torch.stack([w & 0x3FF, (w >> 10) & 0x3FF, (w >> 20) & 0x3FF], dim=3).to(torch.int16)      # [row][block][dword][field]
    p = d_planes.view(torch.int16)
    p[:W * H].reshape(H, W // 6, 6).copy_(torch.stack([f[:, :, a, b] for a, b in R.V210_Y], dim=2))
    p[W * H:W * H + cw * H].reshape(H, W // 6, 3).copy_(torch.stack([f[:, :, a, b] for a, b in R.V210_CB], dim=2))
    p[W * H + cw * H:].reshape(H, W // 6, 3).copy_(torch.stack([f[:, :, a, b] for a, b in R.V210_CR], dim=2))


def torch_pack(fmt, d_planes, W, H, d_frame):
    cw = W // 2
    if fmt == R.UYVY:
        m = d_frame.reshape(H, cw, 4)
        m[:, :, 1::2] = d_planes[:W * H].reshape(H, cw, 2)
        m[:, :, 0] = d_planes[W * H:W * H + cw * H].reshape(H, cw)
        m[:, :, 2] = d_planes[W * H + cw * H:].reshape(H, cw)
        return
    p = d_planes.view(torch.int16)
    planes = (p[:W * H].reshape(H, W // 6, 6).to(torch.int32), p[W * H:W * H + cw * H].reshape(H, W // 6, 3).to(torch.int32),
              p[W * H + cw * H:].reshape(H, W // 6, 3).to(torch.int32))
    w = torch.zeros(H, W // 6, 4, dtype=torch.int32, device="cuda")
    for pl, table in zip(planes, (R.V210_Y, R.V210_CB, R.V210_CR)):
        for k, (word, field) in enumerate(table):
            w[:, :, word] |= pl[:, :, k] << (10 * field)
    d_frame.view(torch.int32).reshape(H, W // 6, 4).copy_(w)


def one_format(c, a, name, fmt, prec, W, H):
    layout = G.ImageLayout.make(W, H)
    base = G.TileParams.make(1, 1, 3, prec, 5, mct=False)
    bps = 1 if prec <= 8 else 2
    planes = [plane(W, H, 1, prec), plane(W // 2, H, 2, prec), plane(W // 2, H, 3, prec)]
    frame = R.pack(fmt, prec, *planes)
    nbytes, pitch = G.packed_bytes(fmt, layout, prec)
    assert nbytes == frame.size
    i422, sampling, nplanes = G.Surface.make("I422", layout, prec, 0)
    assert nplanes == 2 * W * H * bps
    d_frame = torch.from_numpy(frame).cuda()
    d_planes = torch.zeros(nplanes, dtype=torch.uint8, device="cuda")
    d_out = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    d_out2 = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    print("# %s %d x %d, %d bits: %d bytes (pitch %d); one tile, reversible HT, 5 levels" % (name, W, H, prec, nbytes, pitch))
    files = {}

    def enc():
        files["packed"] = c.encode_packed(layout, base, fmt, d_frame.data_ptr(), cap=nbytes)

    def enc_before():
        torch_unpack(fmt, d_frame, W, H, d_planes)
        torch.cuda.synchronize()
        files["before"] = c.encode_surface(layout, base, sampling, i422, d_planes.data_ptr(), cap=nplanes)

    res = alternated({"encode_packed": enc, "before: torch unpack to three planes + encode_surface I422, in place": enc_before}, a.repeats)
    assert files["packed"] == files["before"]
    show("encode, device-resident %s frame -> file of %d bytes in host memory" % (name, len(files["packed"])), res)
    pinned = c.host_array(len(files["packed"]))
    pinned[:] = np.frombuffer(files["packed"], np.uint8)

    def dec():
        c.decode_packed(pinned, fmt, d_out.data_ptr(), cap=nbytes)
        c.decode_status()

    def dec_before():
        c.decode_surface(pinned, i422, d_planes.data_ptr(), cap=nplanes)
        c.decode_status()
        torch_pack(fmt, d_planes, W, H, d_out2)
        torch.cuda.synchronize()

    res = alternated({"decode_packed": dec, "before: decode_surface I422, in place + torch pack": dec_before}, a.repeats)
    assert np.array_equal(d_out.cpu().numpy(), frame) and np.array_equal(d_out2.cpu().numpy(), frame)
    show("decode, file in pinned host memory -> device-resident %s frame" % name, res)

    def unpack():
        c.packed_unpack_device(fmt, prec, W, H, d_frame.data_ptr(), pitch, nbytes, d_planes.data_ptr(), nplanes)
        c.synchronize()

    def pack():
        c.packed_pack_device(fmt, prec, W, H, d_planes.data_ptr(), nplanes, d_out.data_ptr(), pitch, nbytes)
        c.synchronize()

    def plain():
        d_out2.copy_(d_frame)
        torch.cuda.synchronize()

    res = alternated({"KU unpack, frame -> Y, Cb, Cr": unpack, "KK pack, Y, Cb, Cr -> frame": pack,
                      "plain device-to-device copy of the frame's bytes": plain}, a.repeats)
    assert np.array_equal(d_out.cpu().numpy(), frame)
    show("the kernels alone, the whole frame, one launch each (GB/s: the frame's bytes, read or written once; the planes' %d bytes travel "
         "the other way)" % nplanes, res, nbytes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--small", action="store_true", help="1920 x 1080 instead of 7680 x 4320 (a quick look)")
    a = ap.parse_args()
    W, H = (1920, 1080) if a.small else (7680, 4320)
    c = G.Context(0)
    print("# tools/packed_time.py: medians of %d repeats, variants alternated within a repeat; %s" % (a.repeats, torch.cuda.get_device_name(0)))
    one_format(c, a, "UYVY", R.UYVY, 8, W, H)
    one_format(c, a, "v210", R.V210, 10, W, H)


if __name__ == "__main__":
    main()
