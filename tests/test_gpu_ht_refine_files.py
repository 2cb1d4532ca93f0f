"""-m gpu: HTJ2K FILES whose code-blocks carry refinement passes, decoded whole: grk_amd_decode_image, grk_amd_decode_image_device_ex
and grk_amd_decode_image_view reach K5c (the SigProp / MagRef passes on the device) through the readers that take such files.

The expected pixels are computed on the CPU by the oracle: every block's words from the reference's block decoder where it is built
(refharness.ht_decode_block_passes), else from oracle.ht_decode_block + ht_refine_decode, then the oracle's dequantisation, inverse
transform and colour / DC stage (tests/t2ht_cases.py: expected_pixels) -- never this library's own table route.  The files are the
shapes tests/test_gpu_ht_refine.py holds K5c to, written by tests/t2ht_model.py as one layer of three-pass blocks and as three layers
1 | 1 | 1 (pieces, moves, the appendix), every eleventh block's refinement segment cut to half, cleanup-only blocks mixed in.

At the commit before this change grk_amd_decode_image refuses every one of these files: GRK_AMD_ERR_UNSUPPORTED, "... an HT
code-block with more than one pass"."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import grok_amd as G
import gpuutil as U
import t2ht_cases as K

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
PARENT = os.path.join(HERE, "golden", "ht_refine_parent_counters.json")


@pytest.fixture(scope="module")
def contents():
    out = {}
    for c in K.content_cases():
        c.pixels = K.expected_pixels(c)
        out[c.name] = c
    return out


def _dev(cs):
    d = torch.from_numpy(np.frombuffer(cs, np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    return d


NAMES = ["%s-%s" % (s[0], l) for s in K.SHAPES for l in ("L1", "L3")]


@pytest.mark.parametrize("name", NAMES)
def test_decode_image_equals_the_oracle(contents, name):
    c = contents[name]
    assert sum(n > 1 for t in c.passes for n in t) >= 1 and (len(c.want["rows"]) < 8 or sum(n == 1 for t in c.passes for n in t) >= 1)
    got = U.ctx().decode_image(c.cs)
    assert got.shape == c.pixels.shape
    assert np.array_equal(got.astype(np.int32), c.pixels), "%d samples differ" % int((got.astype(np.int32) != c.pixels).sum())


@pytest.mark.parametrize("name", NAMES)
def test_decode_image_device_ex_equals_the_oracle(contents, name):
    c = contents[name]
    ctx = U.ctx()
    d = _dev(c.cs)
    staged = ctx.read_device_counters()[4]
    out = np.zeros(c.pixels.shape, np.uint8 if c.shape[6] <= 8 else np.uint16)
    ctx.decode_image_resident_ex(d.data_ptr(), d.numel(), out.ctypes.data, out.nbytes, on_device=False)
    assert np.array_equal(out.astype(np.int32), c.pixels), "%d samples differ" % int((out.astype(np.int32) != c.pixels).sum())
    # (an appendix: the stream is staged in front of it, once)
    assert ctx.read_device_counters()[4] - staged == (len(c.cs) if c.want["appendix_bytes"] else 0)
    # ... and into device pixels
    px = torch.zeros(out.nbytes, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.decode_image_resident_ex(d.data_ptr(), d.numel(), px.data_ptr(), px.numel())
    ctx.decode_status()
    assert np.array_equal(px.cpu().numpy().view(out.dtype).reshape(out.shape), out)


def test_the_int16_plane_setting_is_left_as_it_was_and_a_cleanup_only_file_still_decodes(contents):
    ctx = U.ctx()
    c = K.content_file(K.SHAPES[1], False, K.PLT, refine=False)
    want = K.expected_pixels(c)
    assert np.array_equal(ctx.decode_image(c.cs).astype(np.int32), want)
    r = contents["200x120-L3"]
    assert np.array_equal(ctx.decode_image(r.cs).astype(np.int32), r.pixels)
    assert np.array_equal(ctx.decode_image(c.cs).astype(np.int32), want)
    # (the refinement passes are visible in the pixels of the 9/7 files)
    for shape in (K.SHAPES[0], K.SHAPES[4]):
        plain = K.expected_pixels(K.content_file(shape, False, K.PLT, refine=False))
        assert (plain != contents[shape[0] + "-L1"].pixels).mean() > 0.1


@pytest.mark.parametrize("name", ["200x120-L1", "200x120-L3"])
def test_reduced_view_equals_the_oracles_reduced_decode(contents, name):
    c = contents[name]
    got = U.ctx().decode_image_view(c.cs, 1)
    want = K.expected_pixels(c, reduce=1)
    assert got.shape == want.shape == (3, 60, 100)
    assert np.array_equal(got.astype(np.int32), want), "%d samples differ" % int((got.astype(np.int32) != want).sum())


@pytest.mark.parametrize("name", ["130x67-L1", "130x67-L3", "100x70-tiles-L3"])
def test_window_equals_the_crop_of_the_full_decode(contents, name):
    c = contents[name]
    got = U.ctx().decode_image_view(c.cs, 0, (33, 17, 81, 57))
    assert got.shape == (1, 40, 48)
    assert np.array_equal(got.astype(np.int32), c.pixels[:, 17:57, 33:81])


def test_a_cleanup_only_file_costs_what_it_cost_before():
    """the launch and upload counters of grk_amd_decode_image for a cleanup-only file are the ones a build of the commit before this
    change gave for the same bytes (tests/golden/ht_refine_parent_counters.json: written by tools/ht_refine_parent_counters.py from a run
    of that build on the device)"""
    parent = json.load(open(PARENT))
    ctx = U.ctx()
    seen = 0
    for shape in K.SHAPES:
        c = K.content_file(shape, False, K.PLT, refine=False)
        rec = parent[c.name]
        assert hashlib.sha256(c.cs).hexdigest() == rec["sha256"], "the recorded run decoded another file"
        l0, n0 = ctx.decode_image_launches(), ctx.decode_image_counters()
        got = ctx.decode_image(c.cs)
        l1, n1 = ctx.decode_image_launches(), ctx.decode_image_counters()
        assert [l1[0] - l0[0], l1[1] - l0[1]] == rec["launches"] and [n1[0] - n0[0], n1[1] - n0[1]] == rec["counters"], c.name
        assert hashlib.sha256(got.tobytes()).hexdigest() == rec["pixels_sha256"], c.name
        seen += 1
    assert seen == 5
