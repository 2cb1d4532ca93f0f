"""-m gpu: the rate- and quality-targeted calls that leave their file in device memory (grk_amd_encode_surface_rate_device /
_quality_device, grk_amd_encode_packed_rate_device / _quality_device) and grk_amd_assemble_rate_device.

The same image goes through both routes: the device file, copied down, must be the host-memory call's bytes, and the result structs
equal field by field -- the budgets and rounds are shared, so a difference is one of Tier-2 on the device: KK's zero bit-planes from the
chosen drops, KT1's general tag tree, the image-wide tables over several batches and tile classes.  grk_amd_decode_image_device of the
device file, where it lies, gives the pixels grk_amd_decode_image gives for the host bytes.  The counters: as many Tier-2 passes on
the device as the call took rounds (1 for a quality target), no byte of a coded block copied to the host, one more file on the
device route."""
import numpy as np
import pytest
import torch

import grok_amd as G
import gpuutil as U
import packedref as PR
import synth
from grok_amd.capi import ERR_INVALID, ERR_UNSUPPORTED
from test_t2_reader_subsampled_cpu import make_planes

pytestmark = pytest.mark.gpu
DMAX = 3
S444 = [(1, 1), (1, 1), (1, 1)]
S420 = [(1, 1), (2, 2), (2, 2)]
S422 = [(1, 1), (2, 1), (2, 1)]


def _fields(res):
    return {name: getattr(res, name) for name, _ in res._fields_}


class Job:
    """one image on both routes: plain() -> bytes; rate(target) / quality(psnr) -> (bytes, result) from the host-memory call;
    rate_device(target) / quality_device(psnr) -> (device pointer, length, result)"""

    def __init__(self, kind, irreversible, cblk=(6, 6)):
        c = self.c = U.ctx()
        kw = dict(max_drop=DMAX, allow_skip=True)
        if kind == "I444":        # 96 x 80, one tile
            layout, sampling, fmt = G.ImageLayout.make(96, 80), S444, "I444"
        elif kind == "NV12":      # 128 x 96 in two tiles 64 wide: two batches, the luma and the chroma runs of different geometry
            layout, sampling, fmt = G.ImageLayout.make(128, 96, 64, 96), S420, "NV12"
        else:                     # YUY2 66 x 10
            layout, sampling, fmt = G.ImageLayout.make(66, 10), S422, None
        base = G.TileParams.make(1, 1, 3, 8, 2, mct=False, irreversible=irreversible, cblk=cblk)
        planes = [np.clip(p, 32, 224).astype(p.dtype) for p in make_planes(layout, sampling, 8, seed=7)]
        if fmt:
            surface, samp, nbytes = G.Surface.make(fmt, layout)
            assert samp == sampling
            buf = np.zeros(nbytes, np.uint8)
            surface.scatter(buf, planes, 1)
            a = (layout, base, sampling, surface, buf)
            self.plain = lambda: c.encode_surface(*a)
            self.rate = lambda t, **k: c.encode_surface_rate(*a, t, **dict(kw, **k))
            self.quality = lambda p, **k: c.encode_surface_quality(*a, p, **dict(kw, **k))
            self.rate_device = lambda t, **k: c.encode_surface_rate_device(*a, t, **dict(kw, **k))
            self.quality_device = lambda p, **k: c.encode_surface_quality_device(*a, p, **dict(kw, **k))
        else:
            W, H = layout.x1, layout.y1
            frame = PR.pack(PR.YUY2, 8, *planes, 0, np.zeros(PR.frame_bytes(PR.YUY2, W, H, 0), np.uint8))
            a = (layout, base, "YUY2", frame)
            self.plain = lambda: c.encode_packed(*a)
            self.rate = lambda t, **k: c.encode_packed_rate(*a, t, **dict(kw, **k))
            self.quality = lambda p, **k: c.encode_packed_quality(*a, p, 0.0, **dict(kw, **k))
            self.quality_device = lambda p, **k: c.encode_packed_quality_device(*a, p, 0.0, **dict(kw, **k))
            self.rate_device = lambda t, **k: c.encode_packed_rate_device(*a, t, **dict(kw, **k))

    def same(self, host, device):
        """the device call's file and result == the host-memory call's; the counters; the decode of the file where it lies"""
        c = self.c
        want, wres = host()
        routes = c.encode_route_counters()
        d_file, n, res = device()
        got = U.from_dev_ptr(d_file, n).tobytes()
        assert n == len(want)
        assert got == want, "the device file differs from byte %d of %d" % (next(i for i in range(n) if got[i] != want[i]), n)
        assert _fields(res) == _fields(wres)
        passes = getattr(wres, "passes", 1)
        assert c.rate_device_counters() == (passes, 0)
        assert c.encode_route_counters() == (routes[0] + 1, routes[1])
        back = np.concatenate([np.ascontiguousarray(pl).reshape(-1) for pl in c.decode_image_planes(want)])
        d_out = torch.zeros(back.nbytes, dtype=torch.uint8, device="cuda")
        c.decode_image_resident(d_file, n, d_out.data_ptr(), back.nbytes)
        c.decode_status()
        assert np.array_equal(d_out.cpu().numpy().view(back.dtype), back)
        return want, wres


@pytest.mark.parametrize("kind,irreversible", [("I444", False), ("NV12", True), ("YUY2", False)])
def test_rate_targeted_file_in_device_memory_is_the_host_memory_calls(kind, irreversible):
    job = Job(kind, irreversible)
    plain = job.plain()
    target = len(plain) * 6 // 10
    want, res = job.same(lambda: job.rate(target), lambda: job.rate_device(target))
    assert len(want) <= target < len(plain) and res.block_bytes > 0


@pytest.mark.parametrize("kind,irreversible", [("I444", True), ("NV12", True), ("YUY2", False)])
def test_quality_targeted_file_in_device_memory_is_the_host_memory_calls(kind, irreversible):
    job = Job(kind, irreversible)
    plain = job.plain()
    psnr = 32.0
    want, res = job.same(lambda: job.quality(psnr), lambda: job.quality_device(psnr))
    assert len(want) < len(plain), "the target drops no plane"


def test_a_target_that_takes_two_rounds():
    """the first round's file overshoots where the general tag trees cost more than the plain file's headers left room for -- many
    small code-blocks, each with a value of its own --: the targets are scanned on the host route, from the plain file's length down,
    for the first that takes it two rounds"""
    found = None
    for kind, irreversible, cblk in (("NV12", False, (3, 3)), ("NV12", True, (3, 3)), ("I444", False, (3, 3)), ("NV12", False, (2, 2)),
                                     ("NV12", False, (6, 6))):
        job = Job(kind, irreversible, cblk)
        plain = job.plain()
        for target in [len(plain) - j for j in (1, 2, 4, 8, 16, 32, 64)] + [len(plain) * k // 64 for k in range(62, 1, -1)]:
            try:
                _, res = job.rate(target)
            except G.RateError:
                break
            if res.passes >= 2:
                found = target
                break
        if found is not None:
            break
    assert found is not None, "no target of the scan takes the host route two rounds"
    _, res = job.same(lambda: job.rate(found), lambda: job.rate_device(found))
    assert res.passes >= 2


def test_a_target_so_low_that_every_block_is_skipped():
    """the smallest target the host route meets: the file with no byte of any block -- an empty arena, which must still assemble"""
    job = Job("I444", False)
    plain = job.plain()

    def feasible(t):
        try:
            return job.rate(t)[1]
        except G.RateError:
            return None

    lo, hi = 60, len(plain) // 4               # lo fails (below the headers), hi succeeds
    assert feasible(lo) is None and feasible(hi) is not None
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if feasible(mid) is None:
            lo = mid
        else:
            hi = mid
    assert feasible(hi).block_bytes == 0
    want, res = job.same(lambda: job.rate(hi), lambda: job.rate_device(hi))
    assert res.block_bytes == 0 and len(want) == hi


def test_refusals_are_the_twins():
    fresh = G.Context(0)
    try:
        layout = G.ImageLayout.make(96, 80)
        base = G.TileParams.make(1, 1, 3, 8, 2, mct=False)
        surface, sampling, nbytes = G.Surface.make("I444", layout)
        buf = np.zeros(nbytes, np.uint8)
        fresh.set_pipelining(True)
        reasons = []
        for call in (fresh.encode_surface_rate, fresh.encode_surface_rate_device):
            with pytest.raises(G.RateError) as e:
                call(layout, base, sampling, surface, buf, 10000)
            assert e.value.code == ERR_UNSUPPORTED
            reasons.append(e.value.reason)
        assert reasons[0] == reasons[1] and "pipelined" in reasons[0]
        reasons = []
        for call in (fresh.encode_surface_quality, fresh.encode_surface_quality_device):
            with pytest.raises(G.RateError) as e:
                call(layout, base, sampling, surface, buf, 40.0)
            assert e.value.code == ERR_UNSUPPORTED
            reasons.append(e.value.reason)
        assert reasons[0] == reasons[1]
        fresh.set_pipelining(False)
        for call in (fresh.encode_surface_rate, fresh.encode_surface_rate_device):
            with pytest.raises(G.RateError) as e:
                call(layout, base, sampling, surface, buf, 10000, max_drop=13)
            assert e.value.code == ERR_INVALID and "max_drop" in e.value.reason
        for call in (fresh.encode_surface_quality, fresh.encode_surface_quality_device):
            with pytest.raises(G.RateError) as e:
                call(layout, base, sampling, surface, buf, float("nan"))
            assert e.value.code == ERR_INVALID
    finally:
        fresh.set_pipelining(False)


@pytest.mark.parametrize("goal", ["rate", "quality"])
def test_assemble_rate_device_after_a_targeted_tile_call(goal):
    """two tiles of 64 x 48: the tile-parts of the call's own table under CS_BLOCK_MSBS, made without the table leaving the device;
    after a plain encode_tiles the call is refused"""
    c = U.ctx()
    p = G.TileParams.make(64, 48, 3, 8, 2, irreversible=(goal == "quality"), cblk=(4, 4))
    px = np.stack([np.clip(synth.g2(3, 48, 64, 8, seed=s), 32, 224).astype(np.uint8) for s in (1, 2)])
    plain, _ = c.encode_tiles(p, 2, px.ctypes.data, False)
    with pytest.raises(G.RateError) as e:
        c.assemble_rate_device(p, [0, 1])
    assert e.value.code == ERR_INVALID
    if goal == "rate":
        table, tot, _ = c.encode_tiles_rate(p, 2, px.ctypes.data, False, int(plain["length"].sum()) // 2, DMAX, True)
    else:
        table, tot, _ = c.encode_tiles_quality(p, 2, px.ctypes.data, False, 32.0, max_drop=DMAX, allow_skip=True)
    blocks, _ = G.tile_layout(p)
    kmax = np.array([b.kmax for b in blocks] * 2)
    assert np.any(table["missing_msbs"] != kmax - 1), "the call dropped nothing"
    coded = c.fetch_coded(tot)
    bpt = len(blocks)
    for flags in (0, G.CS_PLT | G.CS_SOP | G.CS_PROG(2)):
        n, lens = c.assemble_rate_device(p, [3, 4], flags)
        want = [G.write_tile_part(p, 3 + i, table[i * bpt:(i + 1) * bpt], coded, flags | G.CS_BLOCK_MSBS) for i in range(2)]
        assert [int(v) for v in lens] == [len(w) for w in want] and c.fetch_assembled(0, n).tobytes() == b"".join(want)
    # the plain call still refuses the flag, and assembles the constant tree
    with pytest.raises(RuntimeError):
        c.assemble_device(p, [3, 4], G.CS_BLOCK_MSBS)
