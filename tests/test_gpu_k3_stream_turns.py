"""GPU: K3's classes of consecutive pipelined frames on the two side streams in turn (GRK_AMD_K3_ALT=0: fixed streams) change no
result: eight pipelined encodes, each fetched inside its validity window, equal the un-pipelined encode of the same frame; again
with white noise, whose blocks outgrow the capped LDS buffers, so that blocks go through the fallback launches in both parities."""
import numpy as np
import pytest
import torch

import grok_amd as G
import synth
import gpuutil as U

pytestmark = pytest.mark.gpu


def dev_view(ptr, n, typestr):
    class _H:
        pass
    h = _H()
    h.__cuda_array_interface__ = {"shape": (int(n),), "typestr": typestr, "data": (int(ptr), False), "version": 2}
    return torch.as_tensor(h, device="cuda")


@pytest.mark.parametrize("alt", ["1", "0"])
@pytest.mark.parametrize("content", ["g2", "noise"])
@pytest.mark.parametrize("depth", [1, 4])
def test_pipelined_frames_take_the_side_streams_in_turn(depth, content, alt, monkeypatch):
    """Eight pipelined encodes of 256 x 256 x 3, 2 levels (a top class and a rest class), out of four different frames, on the route
    that large frames take (GRK_AMD_FRAME_STREAMS=0: the DWT chain on the main stream, K3 on the side streams): frame k's table and
    bytes, read from its buffer set once `depth` more encodes are queued, equal the un-pipelined encode's.  Noise: blocks of the fine
    sub-bands outgrow the capped buffers, so in both parities blocks go through the fallback launches (one workgroup per CU walks the
    list) -- the count the launches leave in the set's allocator words is above 0 in every frame.  `alt`: GRK_AMD_K3_ALT -- "0" keeps
    every frame's classes on the same streams (and the fallback grid of up to 1024 workgroups): the same bytes."""
    monkeypatch.setenv("GRK_AMD_FRAME_STREAMS", "0")
    monkeypatch.setenv("GRK_AMD_K3_ALT", alt)
    W = H = 256
    p = G.TileParams.make(W, H, 3, 8, 2)
    rng = np.random.default_rng(11)
    if content == "g2":
        frames = [synth.g2(3, H, W, 8, seed=60 + i) for i in range(4)]
    else:
        frames = [rng.integers(0, 256, size=(3, H, W), dtype=np.uint8) for _ in range(4)]
    nb = G.lib().grk_amd_tile_num_blocks(p)
    plain = G.Context(0)
    want = []
    for im in frames:
        t, coded = plain.encode_host(p, im)
        want.append(U.split_blocks(t, coded))
    plain.close()
    c = G.Context(0)
    c.set_pipelining(depth)
    d = [U.to_dev(im.reshape(-1)) for im in frames]
    held, checked = [], 0

    def check(k):
        arena_p, off_p, len_p, used_p, handed_p = held[k]
        torch.cuda.synchronize()
        used = int(dev_view(used_p, 1, "<i8").cpu()[0])
        offs = dev_view(off_p, nb, "<i8").cpu().numpy()
        lens = dev_view(len_p, nb, "<i4").cpu().numpy()
        arena = dev_view(arena_p, used, "|u1").cpu().numpy()
        assert [bytes(arena[int(o):int(o) + int(l)]) for o, l in zip(offs, lens)] == want[k % 4], "encode %d" % k
        handed = dev_view(handed_p, 24, "<i8").cpu().numpy()
        print("encode %d: blocks handed to the fallback launches per class %s" % (k, handed[:4].tolist()))
        if content == "noise":
            assert handed.sum() > 0, "encode %d: no block went through a fallback launch" % k
        return 1

    for k in range(8):
        c.encode_tiles(p, 1, d[k % 4].data_ptr(), True, fetch=False)
        held.append((c.coded_device_ptr(), c.table_device_ptr(0), c.table_device_ptr(1), c.table_device_ptr(2), c.table_device_ptr(3)))
        if k >= depth:                   # encode k - depth, now that `depth` more encodes are queued: the last call that leaves it valid
            checked += check(k - depth)
    c.synchronize()
    for k in range(8 - depth, 8):        # the sets still in rotation
        checked += check(k)
    assert checked == 8
    c.set_pipelining(False)
    c.close()
