"""Small frames, where the host's launch path is what a call costs: bench.py's pipelined encode loop (grk_amd_set_pipelining) and its
sequence-mode decode loop (grk_amd_set_decode_pipelining, two frames in flight) at 512^2 and 2048^2 x 3, 8-bit, 5/3, 5 levels.
usage: [GRK_AMD_LIB=<another build's libgrok_amd.so>] python tools/launch_path_time.py <label> [repeats] [frames per repeat]
One line per workload: min / median / max of the repeats' ms per frame.  profiles/idwt_plan.txt: the parent commit's library and this
tree's in turn, one process each."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import grok_amd as G  # noqa: E402
import synth  # noqa: E402


def main():
    label = sys.argv[1] if len(sys.argv) > 1 else "tree"
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 9
    frames = int(sys.argv[3]) if len(sys.argv) > 3 else 200
    dev = torch.device("cuda:0")
    ctx = G.Context(0)
    stream = torch.cuda.Stream(dev)
    ctx.set_stream(stream.cuda_stream)
    for S in (512, 2048):
        params = G.TileParams.make(S, S, 3, 8, 5)
        d_px = torch.from_numpy(synth.g2(3, S, S, 8).reshape(-1)).to(dev)
        nblocks = G.lib().grk_amd_tile_num_blocks(params)
        torch.cuda.synchronize(dev)
        # ---- encode, consecutive calls pipelined (bench.py: _encode_workload)
        ctx.set_overlap(True)
        ctx.set_pipelining(True)
        times = []
        for r in range(repeats + 1):                   # (the first stretch warms clocks and pipeline up)
            t0 = time.perf_counter()
            for _ in range(frames):
                ctx.encode_tiles(params, 1, d_px.data_ptr(), True, fetch=False)
            torch.cuda.synchronize(dev)
            times.append((time.perf_counter() - t0) / frames * 1e3)
        ctx.set_pipelining(False)
        report(label, "encode %4d^2 x 3, pipelined" % S, times[1:])
        # ---- decode, a sequence of frames through the context, two in flight (bench.py: sequence_mode)
        ctx.encode_tiles(params, 1, d_px.data_ptr(), True, fetch=False)
        table, total = ctx.fetch_table(nblocks)
        backs = [torch.empty_like(d_px) for _ in range(2)]
        torch.cuda.synchronize(dev)
        ctx.set_decode_pipelining(2)
        times = []
        for r in range(repeats + 1):
            t0 = time.perf_counter()
            for k in range(frames):
                ctx.decode_device(params, 1, table, ctx.coded_device_ptr(), total, backs[k % 2].data_ptr())
            ctx.synchronize()
            times.append((time.perf_counter() - t0) / frames * 1e3)
        ctx.decode_status()
        ctx.set_decode_pipelining(0)
        assert all(bool(torch.equal(b, d_px)) for b in backs), "the decode is not the encoder's input"
        report(label, "decode %4d^2 x 3, sequence of frames, 2 in flight" % S, times[1:])
    ctx.close()


def report(label, what, times):
    print("    %-8s | %-52s min %8.4f  median %8.4f  max %8.4f ms per frame (%d repeats)" %
          (label, what, min(times), float(np.median(times)), max(times), len(times)), flush=True)


if __name__ == "__main__":
    main()
