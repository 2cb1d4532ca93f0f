"""numpy reference of the packed 4:2:2 formats (include/grok_amd.h: GRK_AMD_PACKED_*), written from their definitions alone -- a
helper of tests/test_packed_cpu.py and tests/test_gpu_packed.py, not a test.

Macropixel m of a row holds Y[2m], Y[2m+1], Cb[m], Cr[m].  YUY2 / UYVY / YVYU: 4 bytes Y0 Cb Y1 Cr / Cb Y0 Cr Y1 / Y0 Cr Y1 Cb.  Y216: four
little-endian 16-bit words Y0 Cb Y1 Cr, each v << (16 - prec).  v210: a 16-byte block of four little-endian dwords with three 10-bit
fields each holds three macropixels (the table V210 below).

pack() reproduces a decode's write rules: exactly the bytes of samples are written (an odd width's last Y1 and everything between a
row's end and the pitch keep the canvas's values); v210: every block that holds a sample is written whole, fields past the width and
bits 30-31 zero, the bytes behind a row's last block keep theirs.  unpack() reads what an encode reads: the low 16 - prec bits of a
Y216 word, bits 30-31 of a v210 dword and every field past the width are ignored."""
import numpy as np

YUY2, UYVY, YVYU, Y216, V210 = range(5)
NAMES = {YUY2: "YUY2", UYVY: "UYVY", YVYU: "YVYU", Y216: "Y216", V210: "V210"}
# container index inside a macropixel of Y0, Y1, Cb, Cr
SLOTS = {YUY2: (0, 2, 1, 3), UYVY: (1, 3, 0, 2), YVYU: (0, 2, 3, 1), Y216: (0, 2, 1, 3)}
# v210: (dword, field) inside a block of luma 6b + k, chroma 3b + k
V210_Y = ((0, 1), (1, 0), (1, 2), (2, 1), (3, 0), (3, 2))
V210_CB = ((0, 0), (1, 1), (2, 2))
V210_CR = ((0, 2), (2, 0), (3, 1))


def prec_ok(fmt, prec):
    return 1 <= prec <= 8 if fmt <= YVYU else 9 <= prec <= 16 if fmt == Y216 else prec == 10


def align(fmt):
    """what the base address and the pitch are multiples of"""
    return 16 if fmt == V210 else 2 if fmt == Y216 else 1


def row_bytes(fmt, w):
    """bytes from a row's first byte to the end of its last container"""
    cw = (w + 1) // 2
    return (w + 5) // 6 * 16 if fmt == V210 else cw * (8 if fmt == Y216 else 4)


def default_pitch(fmt, w):
    return (w + 47) // 48 * 128 if fmt == V210 else row_bytes(fmt, w)


def frame_bytes(fmt, w, h, pitch=0):
    pitch = pitch or default_pitch(fmt, w)
    return (h - 1) * pitch + row_bytes(fmt, w)


def _rows(buf, fmt, w, h, pitch):
    """the frame's rows as an (h, row_bytes) view of the uint8 array `buf`"""
    n = row_bytes(fmt, w)
    assert buf.dtype == np.uint8 and buf.ndim == 1 and buf.size >= (h - 1) * pitch + n
    return np.lib.stride_tricks.as_strided(buf, (h, n), (pitch, 1))


def unpack(fmt, prec, frame, w, h, pitch=0):
    """frame (1-D uint8) -> [Y (h x w), Cb, Cr (h x ceil(w / 2))], uint8 for prec <= 8, else uint16"""
    assert prec_ok(fmt, prec)
    pitch = pitch or default_pitch(fmt, w)
    cw = (w + 1) // 2
    rows = _rows(frame, fmt, w, h, pitch)
    dt = np.uint8 if prec <= 8 else np.uint16
    Y, Cb, Cr = np.zeros((h, w), dt), np.zeros((h, cw), dt), np.zeros((h, cw), dt)
    if fmt == V210:
        words = np.ascontiguousarray(rows).view("<u4").reshape(h, -1, 4)              # [row][block][dword]
        for planes, table, n in ((Y, V210_Y, w), (Cb, V210_CB, cw), (Cr, V210_CR, cw)):
            per = len(table)
            for k, (word, field) in enumerate(table):
                got = (words[:, :, word] >> (10 * field)) & 0x3FF
                cols = np.arange(k, n, per)
                planes[:, cols] = got[:, :len(cols)]
        return [Y, Cb, Cr]
    if fmt == Y216:
        cont = np.ascontiguousarray(rows).view("<u2").reshape(h, cw, 4) >> (16 - prec)
    else:
        cont = rows.reshape(h, cw, 4)
    y0, y1, cb, cr = SLOTS[fmt]
    Y[:, 0::2] = cont[:, :, y0]
    Y[:, 1::2] = cont[:, :w // 2, y1]
    Cb[:, :] = cont[:, :, cb]
    Cr[:, :] = cont[:, :, cr]
    return [Y, Cb, Cr]


def pack(fmt, prec, Y, Cb, Cr, pitch=0, canvas=None):
    """planes -> the frame as a new 1-D uint8 array: `canvas` (the destination's prior contents; None: zeros of the frame's size)
    with what a decode writes"""
    assert prec_ok(fmt, prec)
    h, w = Y.shape
    cw = (w + 1) // 2
    assert Cb.shape == (h, cw) and Cr.shape == (h, cw)
    pitch = pitch or default_pitch(fmt, w)
    out = np.zeros(frame_bytes(fmt, w, h, pitch), np.uint8) if canvas is None else np.array(canvas, np.uint8).reshape(-1)
    rows = _rows(out, fmt, w, h, pitch)
    if fmt == V210:
        words = np.zeros((h, (w + 5) // 6, 4), np.uint32)
        for plane, table, n in ((Y, V210_Y, w), (Cb, V210_CB, cw), (Cr, V210_CR, cw)):
            per = len(table)
            for k, (word, field) in enumerate(table):
                cols = np.arange(k, n, per)
                words[:, :len(cols), word] |= (plane[:, cols].astype(np.uint32) & 0x3FF) << (10 * field)
        rows[:, :] = words.astype("<u4").view(np.uint8).reshape(h, -1)
        return out
    y0, y1, cb, cr = SLOTS[fmt]
    if fmt == Y216:
        sh = 16 - prec

        def put(slot, plane, ncols):
            v = ((plane.astype(np.uint32) << sh) & 0xFFFF).astype(np.uint16)
            rows[:, 8 * np.arange(ncols) + 2 * slot] = (v & 0xFF).astype(np.uint8)
            rows[:, 8 * np.arange(ncols) + 2 * slot + 1] = (v >> 8).astype(np.uint8)
    else:
        def put(slot, plane, ncols):
            rows[:, 4 * np.arange(ncols) + slot] = plane.astype(np.uint8)
    put(y0, Y[:, 0::2], cw)
    put(y1, Y[:, 1::2], w // 2)
    put(cb, Cb, cw)
    put(cr, Cr, cw)
    return out
