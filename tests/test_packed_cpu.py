"""CPU: packed 4:2:2 frames (YUY2, UYVY, YVYU, Y216, v210) without a GPU -- grk_amd_packed_bytes and the default pitches against the
formats' definitions, every refusal of a frame that needs no context with its code and reason, the numpy reference (tests/packedref.py)
against itself and against frames written out by hand, and the two kernels' own code (grok_amd/csrc/kernels_packed.hip) as host C++:
tests/c/packed_kernels_sim.cpp compiles the file against the stand-in for the HIP runtime (tests/c/hip_sim) and runs every launch thread
after thread under AddressSanitizer and UBSan, in heap blocks of exactly the frame's and the planes' sizes.  (The GPU runs:
tests/test_gpu_packed.py.)"""
import os
import subprocess

import numpy as np
import pytest

import grok_amd as G
import packedref as R

HERE = os.path.dirname(os.path.abspath(__file__))
UNSUPPORTED, INVALID, OVERFLOW = -2, -3, -5
CASES = [("YUY2", 8), ("UYVY", 8), ("YVYU", 5), ("Y216", 10), ("Y216", 16), ("V210", 10)]
WIDTHS = [1, 2, 5, 6, 7, 47, 48, 49]


def cdiv(a, b):
    return (a + b - 1) // b


def expected(fmt, w, h, pitch=0):
    """(bytes, pitch) from the definitions: 4 bytes / four 16-bit words per macropixel, 16 bytes per 6 luma samples, v210 rows by
    convention in units of 48 samples = 128 bytes"""
    cw = cdiv(w, 2)
    row = {"YUY2": 4 * cw, "UYVY": 4 * cw, "YVYU": 4 * cw, "Y216": 8 * cw, "V210": 16 * cdiv(w, 6)}[fmt]
    pitch = pitch or (cdiv(w, 48) * 128 if fmt == "V210" else row)
    return (h - 1) * pitch + row, pitch


@pytest.mark.parametrize("fmt,prec", CASES)
def test_packed_bytes_and_default_pitches(fmt, prec):
    for w in WIDTHS:
        for h in (1, 3):
            for offset in ((0, 0), (2, 5)):
                layout = G.ImageLayout.make(w, h, offset=offset)
                assert G.packed_bytes(fmt, layout, prec) == expected(fmt, w, h), (w, h, offset)
                assert G.packed_bytes(G.PACKED_FORMATS[fmt], layout, prec) == expected(fmt, w, h)
                # a larger pitch on the format's alignment is taken as it is
                _, least = expected(fmt, w, h)
                pitch = least + 16 * 3
                assert G.packed_bytes(fmt, layout, prec, pitch) == expected(fmt, w, h, pitch), (w, h, pitch)
                assert R.frame_bytes(G.PACKED_FORMATS[fmt], w, h) == expected(fmt, w, h)[0]
                assert R.frame_bytes(G.PACKED_FORMATS[fmt], w, h, pitch) == expected(fmt, w, h, pitch)[0]


def test_v210_takes_any_pitch_of_whole_blocks_that_covers_a_row():
    layout = G.ImageLayout.make(49, 4)
    assert G.packed_bytes("V210", layout, 10, 9 * 16) == (3 * 144 + 144, 144)       # ceil(49 / 6) = 9 blocks: below the default 256
    refused("V210", layout, 10, 8 * 16, INVALID, "smaller than a row")


def refused(fmt, layout, prec, pitch, code, text):
    with pytest.raises(G.SurfaceError) as e:
        G.packed_bytes(fmt, layout, prec, pitch)
    assert e.value.code == code and text in str(e.value), str(e.value)


def test_refusals_of_a_frame():
    even = G.ImageLayout.make(10, 4)
    refused(5, even, 8, 0, INVALID, "unknown format")
    refused(-1, even, 8, 0, INVALID, "unknown format")
    # a precision outside the format's range
    for fmt, precs in (("YUY2", (0, 9, 10)), ("UYVY", (9, 16)), ("YVYU", (12,)), ("Y216", (8, 17)), ("V210", (8, 9, 11, 12))):
        for prec in precs:
            refused(fmt, even, prec, 0, INVALID, "precision outside the format's range")
    # a pitch below a row
    refused("YUY2", even, 8, 19, INVALID, "smaller than a row")
    refused("Y216", even, 10, 38, INVALID, "smaller than a row")
    refused("V210", even, 10, 16, INVALID, "smaller than a row")
    # a pitch off the format's alignment (the byte formats have none)
    assert G.packed_bytes("YUY2", even, 8, 21) == (3 * 21 + 20, 21)
    refused("Y216", even, 10, 41, INVALID, "off the format's alignment")
    refused("V210", even, 10, 40, INVALID, "off the format's alignment")
    refused("V210", even, 10, 136, INVALID, "off the format's alignment")
    # an odd x0: the chroma grid does not start on a macropixel
    for fmt, prec in CASES:
        refused(fmt, G.ImageLayout.make(10, 4, offset=(3, 0)), prec, 0, UNSUPPORTED, "odd x0")
        assert G.packed_bytes(fmt, G.ImageLayout.make(10, 4, offset=(4, 1)), prec)[0] > 0
    # an empty area
    empty = G.ImageLayout.make(10, 4)
    empty.x1 = empty.x0
    refused("YUY2", empty, 8, 0, INVALID, "empty image area")


def test_reference_frames_written_by_hand():
    """packedref against frames spelled out byte by byte from the formats' tables"""
    Y = np.array([[1, 2, 3]], np.uint8)
    Cb, Cr = np.array([[10, 11]], np.uint8), np.array([[20, 21]], np.uint8)
    canvas = np.full(8, 0xEE, np.uint8)
    assert R.pack(R.YUY2, 8, Y, Cb, Cr, 0, canvas).tolist() == [1, 10, 2, 20, 3, 11, 0xEE, 21]
    assert R.pack(R.UYVY, 8, Y, Cb, Cr, 0, canvas).tolist() == [10, 1, 20, 2, 11, 3, 21, 0xEE]
    assert R.pack(R.YVYU, 8, Y, Cb, Cr, 0, canvas).tolist() == [1, 20, 2, 10, 3, 21, 0xEE, 11]
    assert canvas.tolist() == [0xEE] * 8                                         # (the canvas itself is left alone)
    Y16, Cb16, Cr16 = np.array([[0x3FF]], np.uint16), np.array([[0x201]], np.uint16), np.array([[0x155]], np.uint16)
    got = R.pack(R.Y216, 10, Y16, Cb16, Cr16, 0, np.full(8, 0xEE, np.uint8))
    assert got.tolist() == [0xC0, 0xFF, 0x40, 0x80, 0xEE, 0xEE, 0x40, 0x55]
    # v210, 7 luma samples: two blocks, the second with one macropixel's worth of fields, the bytes behind it untouched
    Y = np.arange(1, 8, dtype=np.uint16).reshape(1, 7) + 0x300
    Cb, Cr = np.array([[0x11, 0x12, 0x13, 0x14]], np.uint16), np.array([[0x21, 0x22, 0x23, 0x24]], np.uint16)
    got = R.pack(R.V210, 10, Y, Cb, Cr, 0, np.full(32, 0xFF, np.uint8)).view("<u4").tolist()
    assert got == [0x11 | 0x301 << 10 | 0x21 << 20, 0x302 | 0x12 << 10 | 0x303 << 20, 0x22 | 0x304 << 10 | 0x13 << 20, 0x305 | 0x23 << 10 | 0x306 << 20,
                   0x14 | 0x307 << 10 | 0x24 << 20, 0, 0, 0]
    wide = R.pack(R.V210, 10, Y, Cb, Cr, 48, np.full(48 + 32, 0xFF, np.uint8))
    assert wide[32:48].tolist() == [0xFF] * 16 and wide[:32].view("<u4").tolist() == got


@pytest.mark.parametrize("fmt,prec", [(R.YUY2, 8), (R.UYVY, 3), (R.YVYU, 8), (R.Y216, 10), (R.Y216, 16), (R.V210, 10)])
def test_reference_round_trip_and_untouched_bytes(fmt, prec):
    rng = np.random.default_rng(fmt * 31 + prec)
    for w in (1, 2, 5, 6, 7, 13, 49):
        for h in (1, 3):
            pitch = R.default_pitch(fmt, w) + 2 * R.align(fmt)
            cw = (w + 1) // 2
            dt = np.uint8 if prec <= 8 else np.uint16
            planes = [rng.integers(0, 1 << prec, (h, n)).astype(dt) for n in (w, cw, cw)]
            canvas = rng.integers(0, 256, R.frame_bytes(fmt, w, h, pitch)).astype(np.uint8)
            frame = R.pack(fmt, prec, *planes, pitch, canvas)
            for a, b in zip(R.unpack(fmt, prec, frame, w, h, pitch), planes):
                assert a.dtype == b.dtype and np.array_equal(a, b)
            # what lies between a row's end and the pitch is the canvas's
            row = R.row_bytes(fmt, w)
            for y in range(h):
                assert np.array_equal(frame[y * pitch + row:(y + 1) * pitch], canvas[y * pitch + row:(y + 1) * pitch])
            if fmt != R.V210 and w % 2:
                # Y1 of an odd width's last macropixel
                at = (cw - 1) * (8 if fmt == R.Y216 else 4) + R.SLOTS[fmt][1] * (2 if fmt == R.Y216 else 1)
                assert frame[at] == canvas[at]
            # an encode's ignored bits: garbage there reads as the same samples
            if fmt == R.Y216 and prec < 16:
                noisy = frame.copy()
                low = (1 << (16 - prec)) - 1
                for y in range(h):
                    noisy[y * pitch:y * pitch + row:2] |= low & 0xFF
                    noisy[y * pitch + 1:y * pitch + row:2] |= low >> 8
                for a, b in zip(R.unpack(fmt, prec, noisy, w, h, pitch), planes):
                    assert np.array_equal(a, b)
            if fmt == R.V210:
                noisy = frame.copy()
                for y in range(h):
                    noisy[y * pitch + 3:y * pitch + row:4] |= 0xC0
                for a, b in zip(R.unpack(fmt, prec, noisy, w, h, pitch), planes):
                    assert np.array_equal(a, b)


def test_packed_kernels_thread_by_thread_under_sanitizers(tmp_path):
    exe = str(tmp_path / "packed_kernels_sim")
    subprocess.check_call(["g++", "-x", "c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-Wno-attributes", "-I" + os.path.join(HERE, "c", "hip_sim"), os.path.join(HERE, "c", "packed_kernels_sim.cpp"), "-o", exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0, run.stdout[-4000:]
    assert run.stdout.startswith("ok: ") and int(run.stdout.split()[1]) > 10000, run.stdout[-400:]
