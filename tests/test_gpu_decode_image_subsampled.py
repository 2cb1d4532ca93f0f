"""GPU: grk_amd_decode_image on codestreams with sub-sampled components (4:2:2, 4:2:0, ...).  Without upsampling one plane per
component of its own size: against grk_decompress, against the source through this library's encoder, its refusals; with
grk_amd_set_decode_upsample the image on the reference grid in every pixel layout, against the rule written in numpy; and the
upsampling placement kernel alone."""
import ctypes as C

import numpy as np
import pytest
import torch

import grok_amd as G
import gpuutil as U
import refharness as R
import synth
from grok_amd.capi import CODED_DTYPE
from test_t2_reader_subsampled_cpu import S420, S422, cdiv, comp_shape, make_planes, num_tiles, ref_subsampled_stream, tile_comp, write_subsampled

pytestmark = pytest.mark.gpu
needs_ref = pytest.mark.skipif(not R.have_ref(), reason="oracle/_ref (the real reference) not built here")
ODD = [(1, 1), (4, 1), (1, 4)]

# W, H, sampling, prec, numres, tile, offset, ht, irrev, cblksty, mct, env
REF_CASES = {
    "420": (256, 192, S420, 8, 5, None, (0, 0), 1, 0, 0, 0, {}),
    "422": (300, 200, S422, 8, 4, None, (0, 0), 1, 0, 0, 0, {}),
    "420-alpha-p12": (200, 150, S420 + [(1, 1)], 12, 4, None, (0, 0), 1, 0, 0, 0, {}),
    "420-p16": (256, 192, S420, 16, 4, None, (0, 0), 1, 0, 0, 0, {}),
    "all22-mct": (256, 256, [(2, 2)] * 3, 8, 5, None, (0, 0), 1, 0, 0, 1, {}),
    "tiles128": (320, 256, S420, 8, 5, (128, 128), (0, 0), 1, 0, 0, 0, {}),
    "odd-factors": (259, 131, ODD, 8, 3, (100, 70), (0, 0), 1, 0, 0, 0, {}),
    "offset22": (130, 99, S420, 8, 4, (64, 48), (2, 2), 1, 0, 0, 0, {}),
    "rpcl-tlm-plt-p12": (320, 240, S420, 12, 5, (160, 120), (0, 0), 1, 0, 0, 0, {"REF_PROG_ORDER": 2, "REF_WRITE_TLM": 1, "REF_WRITE_PLT": 1}),
    "pcrl-sopeph": (384, 256, S420, 8, 5, None, (0, 0), 1, 0, 0, 0, {"REF_PROG_ORDER": 3, "REF_CSTY": 6}),
    "cprl-prc": (384, 256, S420, 8, 5, (192, 128), (0, 0), 1, 0, 0, 0, {"REF_PROG_ORDER": 4, "REF_PRECINCTS": "128,128,64,64"}),
    "p1-53": (256, 192, S420, 8, 5, None, (0, 0), 0, 0, 0, 0, {}),
    "p1-97-p10-tiles": (320, 200, S420, 10, 4, (128, 128), (0, 0), 0, 1, 0, 0, {}),
    "p1-layers": (256, 192, S420, 8, 4, (128, 96), (0, 0), 0, 0, 0, 0, {"REF_LAYERS": "20,1"}),
    # (for the upsampling tests: tile origins that are odd)
    "odd-tiles": (259, 131, S420, 8, 3, (99, 67), (0, 0), 1, 0, 0, 0, {}),
    "odd-factors-odd-tiles": (259, 131, ODD, 8, 3, (99, 70), (0, 0), 1, 0, 0, 0, {}),
    "odd-tiles-p12": (131, 99, S420, 12, 3, (67, 49), (0, 0), 1, 0, 0, 0, {}),
}
_streams = {}


def ref_case(monkeypatch, name):
    """(codestream, source planes, layout, sampling, prec, irrev, what grk_decompress makes of it) -- made once"""
    if name not in _streams:
        W, H, sampling, prec, numres, tile, off, ht, irrev, sty, mct, env = REF_CASES[name]
        layout = G.ImageLayout.make(W, H, *(tile or (None, None)), offset=off)
        planes = make_planes(layout, sampling, prec, seed=len(name))
        env = dict(env, REF_IMG_X0=off[0], REF_IMG_Y0=off[1])
        cs = ref_subsampled_stream(monkeypatch, planes, sampling, prec, W, H, env, *(tile or (None, None)), numres=numres, irrev=irrev, ht=ht,
                                   cblksty=sty, mct=mct)
        _streams[name] = (cs, planes, layout, sampling, prec, irrev, R.decode_planes(cs, sampling, W, H))
    return _streams[name]


# ---- 4. planes == grk_decompress ---------------------------------------------------------------------------------------------------
@needs_ref
@pytest.mark.parametrize("name", [k for k in REF_CASES if not k.startswith("odd-tiles")])
def test_planes_equal_grk_decompress(monkeypatch, name):
    cs, planes, layout, sampling, prec, irrev, want = ref_case(monkeypatch, name)
    info = G.read_header(cs)
    assert info.base.mct == REF_CASES[name][10] and info.num_tiles == num_tiles(layout)
    if "layers" in name:
        assert info.num_layers == 2 and len(G.read_packets(cs, info)["moves"]) > 0
    got = U.ctx().decode_image_planes(cs)
    assert len(got) == len(want)
    for a, b, src in zip(got, want, planes):
        assert a.shape == b.shape and np.array_equal(a.astype(np.int32), b)
        if not irrev:
            assert np.array_equal(a, src)


# ---- 5. round trip through this library's encoder --------------------------------------------------------------------------------
OWN_CASES = [
    # W, H, sampling, prec, levels, tile, offset, flags
    (256, 192, S420, 8, 4, None, (0, 0), 0),
    (130, 99, S420, 8, 3, (64, 48), (3, 1), G.CS_PLT | G.CS_PROG(2)),
    (3, 2, S420, 8, 1, None, (0, 0), 0),
    (131, 67, S422 + [(1, 1)], 12, 2, (50, 40), (1, 0), G.CS_SOP | G.CS_EPH | G.CS_PROG(4)),
]


def own_stream(case):
    W, H, sampling, prec, L, tile, off, flags = case
    layout = G.ImageLayout.make(W, H, *(tile or (None, None)), offset=off)
    planes = make_planes(layout, sampling, prec, seed=7)
    base = G.TileParams.make(1, 1, len(sampling), prec, L, mct=False)
    return U.ctx().encode_image_subsampled(layout, base, sampling, planes, flags), planes, layout


@pytest.mark.parametrize("case", OWN_CASES, ids=lambda k: "%dx%d-off%d.%d" % (k[0], k[1], *k[6]))
def test_planes_of_own_subsampled_files_are_the_planes(case):
    cs, planes, _ = own_stream(case)
    got = U.ctx().decode_image_planes(cs)
    assert len(got) == len(planes)
    for a, b in zip(got, planes):
        assert a.shape == b.shape and np.array_equal(a, b)


def test_ht_irreversible_planes_equal_decode_tiles_per_unit():
    """9/7 HT: no reference bytes exist (defect D1); the planes of a file of this encoder's units == decode_tiles of every unit
    (a tile's run of components of one size) with the table the encoder returned"""
    c = U.ctx()
    W, H, sampling, prec, L = 200, 131, S420 + [(1, 1)], 8, 3
    layout = G.ImageLayout.make(W, H, 100, 70, offset=(1, 1))
    base = G.TileParams.make(1, 1, len(sampling), prec, L, mct=False, irreversible=True)
    planes = make_planes(layout, sampling, prec, seed=8)
    want = [np.zeros_like(p) for p in planes]
    tabs, chunks, at = [], [], 0
    for t in range(num_tiles(layout)):
        for first, count in ((0, 1), (1, 2), (3, 1)):
            dx, dy = sampling[first]
            p = tile_comp(layout, base, dx, dy, t)
            p.num_comps = count
            x, y = p.tile_x0 - cdiv(layout.x0, dx), p.tile_y0 - cdiv(layout.y0, dy)
            unit = np.ascontiguousarray(np.stack([planes[first + k][y:y + p.tile_h, x:x + p.tile_w] for k in range(count)]))
            table, coded = c.encode_host(p, unit)
            back = c.decode_host(p, table, coded)[0]
            for k in range(count):
                want[first + k][y:y + p.tile_h, x:x + p.tile_w] = back[k]
            tt = table.copy()
            dense = np.concatenate([coded[int(o):int(o) + int(n)] for o, n in zip(table["offset"], table["length"])]) if len(table) else coded[:0]
            tt["offset"] = at + np.concatenate([[0], np.cumsum(table["length"].astype(np.int64))[:-1]])
            at += dense.size
            tabs.append(tt)
            chunks.append(dense)
    cs = write_subsampled(layout, base, sampling, np.concatenate(tabs).astype(CODED_DTYPE), np.concatenate(chunks), G.CS_PLT)
    got = c.decode_image_planes(cs)
    for a, b, src in zip(got, want, planes):
        assert np.array_equal(a, b)
        assert synth.psnr_db(a, src, prec) > 40                      # (sanity, as for the full-size images: a 9/7 decode of these samples)


# ---- 6. device destination and refusals -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [OWN_CASES[0], OWN_CASES[1], (65, 33, S420, 8, 2, None, (0, 0), 0)], ids=["one-tile", "tiles", "odd-planes"])
def test_device_destination_cap_and_launch_counts(case):
    c = U.ctx()
    cs, planes, layout = own_stream(case)
    flat = np.concatenate([p.reshape(-1) for p in planes])
    out = U._settled(torch.full((flat.nbytes + 4,), 0xA5, dtype=torch.uint8, device="cuda"))
    gathers, places = c.decode_image_launches()
    c.decode_image_device(cs, out.data_ptr(), flat.nbytes)
    c.decode_status()
    got = out.cpu().numpy()
    assert np.array_equal(got[:flat.nbytes].view(flat.dtype), flat) and np.all(got[flat.nbytes:] == 0xA5)
    if num_tiles(layout) == 1:
        assert c.decode_image_launches() == (gathers, places)          # one tile, no upsampling: run by run straight in
    else:
        assert c.decode_image_launches()[1] > places
    with pytest.raises(RuntimeError, match=r"-5 \(.*cap"):
        c.decode_image_device(cs, out.data_ptr(), flat.nbytes - 1)


def test_layout_without_upsampling_and_forged_mct_are_refused():
    c = U.ctx()
    cs, planes, layout = own_stream(OWN_CASES[0])
    with pytest.raises(RuntimeError, match=r"-2 \(.*pixel layout.*upsampl"):
        c.decode_image(cs, G.PixelLayout.make(interleaved=True))
    cod = cs.index(b"\xff\x52")
    assert cs[cod + 8] == 0
    forged = cs[:cod + 8] + b"\x01" + cs[cod + 9:]
    with pytest.raises(RuntimeError, match=r"-2 \(.*colour transform across components of different size"):
        c.decode_image_planes(forged)
    c.set_decode_upsample(True)
    try:
        with pytest.raises(RuntimeError, match=r"-2 \(.*colour transform across components of different size"):
            c.decode_image(forged)
    finally:
        c.set_decode_upsample(False)
    assert all(np.array_equal(a, b) for a, b in zip(c.decode_image_planes(cs), planes))        # (and the context is as it was)


# ---- 7. upsampling -------------------------------------------------------------------------------------------------------------------
def upsampled(planes, sampling, layout):
    """The rule: image sample (gx, gy) of the reference grid = component sample (gx // dx, gy // dy) where that exists, i.e. from
    dx * ceil(X0 / dx) and dy * ceil(Y0 / dy) on, and 0 before."""
    W, H = layout.x1 - layout.x0, layout.y1 - layout.y0
    out = np.zeros((len(planes), H, W), planes[0].dtype)
    for k, (pl, (dx, dy)) in enumerate(zip(planes, sampling)):
        rep = np.repeat(np.repeat(pl, dy, axis=0), dx, axis=1)
        ox, oy = dx * cdiv(layout.x0, dx) - layout.x0, dy * cdiv(layout.y0, dy) - layout.y0
        out[k, oy:, ox:] = rep[:H - oy, :W - ox]
    return out


def in_layout(want, lay, poison):
    """the bytes of the (C, H, W) image `want` in the pixel layout `lay`, every byte no sample owns = poison"""
    Cn, H, W = want.shape
    bps = want.dtype.itemsize
    p = G.TileParams.make(W, H, Cn, 8 * bps, 0)
    buf = np.full(G.pixel_bytes(p, lay, W, H, 1), poison, np.uint8)
    if lay.interleaved:
        ch = lay.channels or Cn
        row = lay.row_pitch or W * ch * bps
        for y in range(H):
            px = buf[y * row:y * row + W * ch * bps].view(want.dtype).reshape(W, ch)
            px[:, :Cn] = want[:, y, :].T
            px[:, Cn:] = lay.fill
    else:
        row = lay.row_pitch or W * bps
        plane = lay.plane_pitch or H * row
        for k in range(Cn):
            for y in range(H):
                buf[k * plane + y * row:k * plane + y * row + W * bps].view(want.dtype)[:] = want[k, y]
    return buf


def layouts_for(want):
    Cn, H, W = want.shape
    bps = want.dtype.itemsize
    row = W * bps + (3 if bps == 1 else 2)
    if row % 4 == 0:
        row += bps
    return [G.PixelLayout.make(row_pitch=row), G.PixelLayout.make(row_pitch=row, plane_pitch=H * row + 5 * bps),
            G.PixelLayout.make(interleaved=True), G.PixelLayout.make(interleaved=True, channels=4, fill=(1 << (8 * bps)) - 3, row_pitch=4 * W * bps + 4 * bps)]


def check_upsampled_in_every_layout(cs, want):
    c = U.ctx()
    c.set_decode_upsample(True)
    try:
        _, places = c.decode_image_launches()
        got = c.decode_image(cs)
        assert got.shape == want.shape and np.array_equal(got, want)
        assert c.decode_image_launches()[1] > places                      # (also a one-tile image goes through the placement)
        for lay in layouts_for(want):
            expect = in_layout(want, lay, 0xA5)
            got = c.decode_image(cs, lay, np.full(expect.size, 0xA5, np.uint8))
            assert np.array_equal(got, expect), (lay.interleaved, lay.channels, lay.row_pitch, lay.plane_pitch)
            # the same into device memory
            d = U._settled(torch.full((expect.size,), 0xA5, dtype=torch.uint8, device="cuda"))
            c.set_decode_pixel_layout(lay)
            try:
                c.decode_image_device(cs, d.data_ptr(), expect.size)
                c.decode_status()
            finally:
                c.set_decode_pixel_layout(None)
            assert np.array_equal(d.cpu().numpy(), expect)
    finally:
        c.set_decode_upsample(False)


@needs_ref
@pytest.mark.parametrize("name", ["odd-tiles", "odd-factors-odd-tiles", "422", "odd-tiles-p12", "420-alpha-p12"])
def test_upsampled_reference_streams_equal_the_rule(monkeypatch, name):
    cs, planes, layout, sampling, prec, irrev, ref = ref_case(monkeypatch, name)
    dt = np.uint8 if prec <= 8 else np.uint16
    check_upsampled_in_every_layout(cs, upsampled([p.astype(dt) for p in ref], sampling, layout))


@pytest.mark.parametrize("case", [OWN_CASES[1], OWN_CASES[2], OWN_CASES[3], (37, 21, S420, 16, 2, None, (3, 3), 0)],
                         ids=lambda k: "%dx%d-off%d.%d-p%d" % (k[0], k[1], *k[6], k[3]))
def test_upsampled_own_files_equal_the_rule(case):
    cs, planes, layout = own_stream(case)
    want = upsampled(planes, case[2], layout)
    if case[6] == (3, 1):
        assert not want[1, 0].any() and not want[1, :, 0].any() and want[0, 0].any()       # (the zero row and column of the chroma)
    check_upsampled_in_every_layout(cs, want)


def test_upsample_switch_leaves_streams_without_subsampling_alone():
    import synth
    c = U.ctx()
    px = synth.g2(3, 150, 200, 8)
    layout = G.ImageLayout.make(200, 150, 96, 80, offset=(1, 1))
    cs = c.encode_image(layout, G.TileParams.make(96, 80, 3, 8, 3), px, G.CS_PLT)
    off = c.decode_image(cs)
    lay = G.PixelLayout.make(interleaved=True, channels=4, fill=9)
    off_lay = c.decode_image(cs, lay)
    c.set_decode_upsample(True)
    try:
        assert np.array_equal(c.decode_image(cs), off) and np.array_equal(off, px)
        assert np.array_equal(c.decode_image(cs, lay), off_lay)
    finally:
        c.set_decode_upsample(False)


# ---- 8. KU alone -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bps", [1, 2])
@pytest.mark.parametrize("dx,dy", [(1, 1), (2, 1), (1, 2), (2, 2), (4, 1), (3, 2)])
def test_upsampling_placement_kernel_equals_numpy(bps, dx, dy):
    c = U.ctx()
    rng = np.random.default_rng(100 * bps + 10 * dx + dy)
    dt = np.uint8 if bps == 1 else np.uint16
    for w in (1, 2, 3, 63, 64, 65):
        for shift in range(4):
            # a component cut into 3 x 2 units of w x h.  The image area starts inside the cell in front of the component's first
            # sample (a strip of zx columns and zy rows that no cell covers: not written) and ends inside the last cells (clipped);
            # `shift` samples in front of the image and the strip move the destination through every alignment
            h, ncomp, cols, rows = 5, 2, 3, 2
            cx0, cy0 = 7 + shift, 3
            zx, zy = shift % dx, 1 if dy > 1 else 0
            img_x0, img_y0 = cx0 * dx - zx, cy0 * dy - zy
            cw, chh = cols * w, rows * h
            img_w, img_h = zx + cw * dx - (dx - 1), zy + chh * dy - (dy - 1)
            comp = rng.integers(0, 1 << (8 * bps), size=(ncomp, chh, cw)).astype(dt)
            units = np.stack([comp[:, j * h:(j + 1) * h, i * w:(i + 1) * w] for j in range(rows) for i in range(cols)])
            origins = [(cx0 + i * w, cy0 + j * h) for j in range(rows) for i in range(cols)]
            order = rng.permutation(len(origins))
            units, origins = np.ascontiguousarray(units[order]), [origins[k] for k in order]
            lead = shift
            img = rng.integers(0, 1 << (8 * bps), size=lead + ncomp * img_h * img_w + 3).astype(dt)
            want = img.copy()
            rep = np.repeat(np.repeat(comp, dy, axis=1), dx, axis=2)
            want[lead:lead + ncomp * img_h * img_w].reshape(ncomp, img_h, img_w)[:, zy:, zx:] = rep[:, :img_h - zy, :img_w - zx]
            d_units, d_img = U.to_dev(units), U.to_dev(img)
            c.place_upsampled_device(d_units.data_ptr(), len(origins), w, h, ncomp, bps, origins, dx, dy, d_img.data_ptr() + lead * bps,
                                     img_x0, img_y0, img_w, img_h)
            c.synchronize()
            assert np.array_equal(d_img.cpu().numpy(), want), (w, shift)
    # a cell that starts outside the image area is refused before anything is launched
    for bad in ((cx0 - 1, cy0), (cx0, cy0 - 1), (cx0 + cw - w + 1, cy0), (cx0, cy0 + chh - h + 1)):
        with pytest.raises(RuntimeError, match="outside the image"):
            c.place_upsampled_device(d_units.data_ptr(), 1, w, h, ncomp, bps, [bad], dx, dy, d_img.data_ptr(), img_x0, img_y0, img_w, img_h)
