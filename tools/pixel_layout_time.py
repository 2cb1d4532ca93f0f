#!/usr/bin/env python3
"""What a pixel layout costs: the bench headline's protocol (8192 x 8192 x 3 8-bit lossless, device-resident pixels, consecutive
encodes pipelined, three frames in rotation, median of the timed regions) for

  a  planar, a build of the PARENT commit (--parent-lib: its libgrok_amd.so, built in a second worktree)
  b  planar, this tree
  c  interleaved RGB                      (grk_amd_set_pixel_layout)
  d  interleaved RGBX, the fourth channel skipped
  e  interleaved RGB rows with a pitch (a 8192-wide window of a wider frame)
  f  what a caller without layouts does: permute(2, 0, 1).contiguous() of the H x W x C frame, then the planar encode

and the 8K HT decode into interleaved pixels against the planar decode + the transpose back.  (a) and (b) alternate, process by
process, on one box: their difference has to lie within the spread the alternation itself shows.

    python tools/pixel_layout_time.py [--size 8192] [--steps 20] [--regions 5] [--rounds 3] [--parent-lib PATH] [--only a,b]

--only a,b: nothing but the alternation, a process each, the order turned round every round (a b, b a, a b ...).

One library per process (GRK_AMD_LIB picks it): a round is one process for (a) and one for everything else, each configuration
with a context of its own.  Prints one JSON line per configuration and round, and a summary."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PREWARM = 40


def worker(a):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch
    import synth
    S = a.size
    dev = torch.device("cuda:0")
    cache = os.path.join(tempfile.gettempdir(), "pixel_layout_time_frames_%d.npy" % S)       # (the rounds' processes share the frames)
    if os.path.exists(cache):
        host = np.load(cache)
    else:
        host = np.stack([synth.g2(3, S, S, 8, seed=12345 + i) for i in range(3)])
        np.save(cache + ".%d.npy" % os.getpid(), host)
        os.replace(cache + ".%d.npy" % os.getpid(), cache)
    frames = [torch.from_numpy(host[i]).to(dev) for i in range(3)]                              # (C, H, W)
    for kind in a.worker.split(","):
        run_config(a, kind, frames)


def run_config(a, kind, frames):
    import torch
    import grok_amd as G
    S = a.size
    dev = frames[0].device
    p = G.TileParams.make(S, S, 3, 8, 5)
    ctx = G.Context(0)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    lay = None
    if kind in ("c", "f", "dec_il"):
        src = [f.permute(1, 2, 0).contiguous() for f in frames]                                            # (H, W, 3)
        lay = G.PixelLayout.make(True, 3)
    elif kind in ("d", "dec_rgbx"):
        src = [torch.cat([f.permute(1, 2, 0), torch.full((S, S, 1), 77, dtype=torch.uint8, device=dev)], 2).contiguous() for f in frames]
        lay = G.PixelLayout.make(True, 4, fill=255)
    elif kind == "e":
        wide = [torch.zeros((S, S + 256, 3), dtype=torch.uint8, device=dev) for _ in frames]
        for w, f in zip(wide, frames):
            w[:, 64:64 + S] = f.permute(1, 2, 0)
        src = [w[:, 64:64 + S] for w in wide]                                                              # a view: data_ptr + stride(0)
        lay = G.PixelLayout.make(True, 3, row_pitch=wide[0].stride(0))
    else:
        src = frames
    torch.cuda.synchronize()

    if kind.startswith("dec"):
        table, tot = ctx.encode_tiles(p, 1, frames[0].data_ptr(), True)
        coded = torch.from_numpy(ctx.fetch_coded(tot)).to(dev)
        out = torch.empty(S * S * (4 if kind == "dec_rgbx" else 3), dtype=torch.uint8, device=dev)
        back = torch.empty((S, S, 3), dtype=torch.uint8, device=dev)
        ctx.set_decode_pixel_layout(lay)

        def one(i):
            with torch.cuda.stream(stream):
                ctx.decode_device(p, 1, table, coded.data_ptr(), tot, out.data_ptr())
                if kind == "dec_planar_transpose":       # what a caller without layouts does to get H x W x C
                    back.copy_(out.view(3, S, S).permute(1, 2, 0))
    else:
        if lay is not None and kind != "f":
            ctx.set_pixel_layout(lay)
        ctx.set_pipelining(True)
        planar = [torch.empty((3, S, S), dtype=torch.uint8, device=dev) for _ in range(3)]

        def one(i):
            with torch.cuda.stream(stream):
                s = src[i % 3]
                if kind == "f":                           # the transpose pass, into a second frame-sized buffer
                    planar[i % 3].copy_(s.permute(2, 0, 1))
                    s = planar[i % 3]
                ctx.encode_tiles(p, 1, s.data_ptr(), True, fetch=False)

    for i in range(PREWARM):
        one(i)
    torch.cuda.synchronize()
    regions = []
    for _ in range(a.regions):
        for i in range(3):
            one(i)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(a.steps):
            one(i)
        torch.cuda.synchronize()
        regions.append((time.perf_counter() - t0) / a.steps * 1e3)
    if kind.startswith("dec"):
        ctx.decode_status()
        want = frames[0].permute(1, 2, 0)
        got = out.view(3, S, S).permute(1, 2, 0) if kind.startswith("dec_planar") else out.view(S, S, -1)[:, :, :3]
        assert torch.equal(got, want), "decoded pixels differ from the source"
    print(json.dumps({"config": kind, "size": S, "ms_per_frame_median": round(statistics.median(regions), 4),
                      "min": round(min(regions), 4), "max": round(max(regions), 4), "regions": a.regions, "steps": a.steps,
                      "lib": os.environ.get("GRK_AMD_LIB", "tree")}), flush=True)
    ctx.synchronize()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3, help="how often the list of configurations is gone through (a and b alternate)")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--worker", default=None)
    ap.add_argument("--only", default=None, help="comma list of configurations (default: all)")
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    tree = ["b", "c", "d", "e", "f", "dec_planar", "dec_planar_transpose", "dec_il", "dec_rgbx"]
    if a.only:
        tree = [k for k in tree if k in a.only.split(",")]
    kinds = (["a"] if a.parent_lib else []) + tree
    got = {k: [] for k in kinds}

    def process(worker_kinds, names, lib):
        print("# " + ",".join(names), flush=True)
        env = dict(os.environ)
        env.pop("GRK_AMD_LIB", None)
        if lib:
            env["GRK_AMD_LIB"] = lib
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", ",".join(worker_kinds), "--size", str(a.size),
                            "--steps", str(a.steps), "--regions", str(a.regions)], env=env, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            print(r.stdout + r.stderr)
            raise SystemExit("%s failed (exit %d): nothing more is started" % (",".join(names), r.returncode))
        lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
        for name, line in zip(names, lines):
            line["config"] = name
            print(json.dumps(line), flush=True)
            got[name].append(line["ms_per_frame_median"])

    for r in range(a.rounds):
        first = a.parent_lib and not (a.only and r % 2)
        if first:
            process(["b"], ["a"], a.parent_lib)
        process(tree, tree, None)
        if a.parent_lib and not first:
            process(["b"], ["a"], a.parent_lib)
    print("\nconfig  median of runs  [each run's median ms per frame]")
    for k in kinds:
        print("%-22s %8.4f  %s" % (k, statistics.median(got[k]), got[k]))
    if "a" in got:
        spread = max(max(got["a"]) - min(got["a"]), max(got["b"]) - min(got["b"]))
        print("a vs b: %+.4f ms (%.2f %%); spread within a configuration across the alternation: %.4f ms"
              % (statistics.median(got["b"]) - statistics.median(got["a"]),
                 100.0 * (statistics.median(got["b"]) / statistics.median(got["a"]) - 1.0), spread))
    if "c" in got and "f" in got:
        print("c vs f: %.4f vs %.4f ms -- interleaved input %s than transpose + planar"
              % (statistics.median(got["c"]), statistics.median(got["f"]), "FASTER" if statistics.median(got["c"]) < statistics.median(got["f"]) else "SLOWER"))


if __name__ == "__main__":
    main()
