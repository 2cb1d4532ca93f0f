"""The figures of profiles/quality.txt, on an MI355X: for 9/7 quality-targeted files the target PSNR, the model's PSNR (what the
allocator accounts for: the planes dropped from the magnitudes a plain encode codes) and the PSNR of the decoded pixels against the
source -- the gap is the 9/7 base quantiser's own error and the transform's departure from orthogonality, which the model leaves out --
for the shapes of tests/test_gpu_quality.py and one 4096 x 4096 x 3 frame; for that frame the quality allocator's time (timing family
9) beside the rate allocator's on the same tables, and the whole call beside a rate-targeted call for the same frame.

    python tools/quality_figures.py [--out profiles/quality.txt] [--size 4096] [--parent-lib build/abl/parent/libgrok_amd.so]

--parent-lib: a library built from the parent commit (its sources through tools/build_variant.sh); its rate-targeted call is timed
beside this build's, each in a fresh process that loads its library through GRK_AMD_LIB.

Times: host clock around synchronous calls, median of five after a warm-up call; the kernels by grk_amd_enable_timing's events."""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import grok_amd as G          # noqa: E402
import synth                  # noqa: E402

TARGETS = (50.0, 45.0, 40.0, 35.0, 30.0)


def psnr_rows(c, name, layout, base, px, targets=TARGETS):
    rows = []
    os.environ["GRK_AMD_IMAGE_T2"] = "host"
    plain = c.encode_image(layout, base, px)
    del os.environ["GRK_AMD_IMAGE_T2"]
    plain_db = synth.psnr_db(c.decode_image(plain), px, 8)
    for t in targets:
        cs, res = c.encode_image_quality(layout, base, px, t, max_drop=6, allow_skip=True)
        dec = synth.psnr_db(c.decode_image(cs), px, 8)
        rows.append("%-22s %6.1f %9.2f %9.2f %+8.2f %10d %8.3f %6d" % (name, t, res.psnr, dec, dec - t, len(cs), len(cs) / len(plain), res.steps))
    rows.append("%-22s   plain: %d bytes, %.2f dB decoded (the 9/7 quantiser's own error alone)" % (name, len(plain), plain_db))
    return rows


def timed(fn):
    """median, min, max in ms of five calls after a warm-up call (host clock; the calls are synchronous)"""
    fn()
    ts = []
    for _ in range(5):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def family9(c, fn):
    """timing family 9 (the allocator) of five calls of fn, one at a time -> (median, min, max in ms per launch, launches per call)"""
    ms, launches = [], 0
    for _ in range(5):
        c.enable_timing(True)                               # (resets the families: an average per launch since then)
        fn()
        v, launches = c.kernel_ms(9)
        ms.append(v)
    c.enable_timing(False)
    return statistics.median(ms), min(ms), max(ms), launches


def frame(N):
    return synth.g2_mid(3, N, N, 8), G.ImageLayout.make(N, N, N, N), G.TileParams.make(N, N, 3, 8, 5, irreversible=True)


def rate_only(N, target):
    """the rate-targeted call alone, for a child process that loads another build of the library through GRK_AMD_LIB"""
    px, layout, base = frame(N)
    c = G.Context(0)
    print("RATE %.3f %.3f %.3f" % timed(lambda: c.encode_image_rate(layout, base, px, target, max_drop=6, allow_skip=True, joint=True)))


def child_rate(N, target, lib):
    """rate_only in a fresh process, with `lib` (or this tree's library for None) -> (median, min, max)"""
    env = dict(os.environ)
    env.pop("GRK_AMD_LIB", None)
    if lib:
        env["GRK_AMD_LIB"] = lib
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--size", str(N), "--rate-only", str(target)], env=env, check=True,
                         capture_output=True, text=True, timeout=300).stdout
    return tuple(float(v) for v in [l for l in out.splitlines() if l.startswith("RATE ")][-1].split()[1:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quality.txt"))
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--parent-lib", default=None, help="libgrok_amd.so built from the parent commit: its rate-targeted call is timed beside this build's")
    ap.add_argument("--rate-only", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.rate_only:
        return rate_only(a.size, a.rate_only)
    c = G.Context(0)
    out = ["quality-targeted encodes, 9/7, 3 components, 8 bits, Dmax 6 + SKIP (tools/quality_figures.py)", "",
           "%-22s %6s %9s %9s %8s %10s %8s %6s" % ("image", "target", "model dB", "decoded", "dec-tgt", "file bytes", "of plain", "steps")]
    for name, (W, H, TW, TH) in {"128x128 one tile": (128, 128, 128, 128), "128x128 2x2 tiles": (128, 128, 64, 64),
                                 "100x76 in 64x48": (100, 76, 64, 48)}.items():
        px = synth.g2_mid(3, H, W, 8)
        out += psnr_rows(c, name, G.ImageLayout.make(W, H, TW, TH), G.TileParams.make(TW, TH, 3, 8, 2, irreversible=True, cblk=(5, 5)), px)
    N = a.size
    px, layout, base = frame(N)
    out += psnr_rows(c, "%dx%d one tile" % (N, N), layout, base, px)
    # times on that frame: the quality call at 40 dB, a rate-targeted call (joint tables) for the bytes that call produced
    quality = lambda: c.encode_image_quality(layout, base, px, 40.0, max_drop=6, allow_skip=True)
    cs, res = quality()
    target = len(cs)
    n = c.rate_num_blocks()
    rate = lambda: c.encode_image_rate(layout, base, px, target, max_drop=6, allow_skip=True, joint=True)
    _, rres = rate()
    q, r = timed(quality), timed(rate)
    kq, kr = family9(c, quality), family9(c, rate)
    fmt = "%.2f (%.2f .. %.2f) ms"
    out += ["", "%dx%dx3 one tile, %d blocks, 40 dB -> %d bytes; the rate-targeted call is given those bytes as its target (joint tables, %d round(s))" % (N, N, n, target, rres.passes),
            "timing family 9 per launch, median (min .. max) of 5 calls: KQ %.3f (%.3f .. %.3f) ms, %d launch per call, %d steps; KR2 %.3f (%.3f .. %.3f) ms, %d launch(es) per call" % (
                kq[:3] + (kq[3], res.steps) + kr),
            "whole call, host pixels, median (min .. max) of 5: quality " + fmt % q + "; rate-targeted " + fmt % r]
    if a.parent_lib:
        c.close()
        out.append("the rate-targeted call alone in a fresh process each, this build and the parent commit's in turn, twice:")
        for k in range(2):
            out.append("  this build " + fmt % child_rate(N, target, None) + "; parent commit " + fmt % child_rate(N, target, os.path.abspath(a.parent_lib)))
    text = "\n".join(out) + "\n"
    print(text)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
