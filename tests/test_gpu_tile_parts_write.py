"""-m gpu: WRITING tiles divided into tile-parts on the device (GRK_AMD_CS_TP; KT1p / KT1q / KT1r / KT2p of kernels_t2parts.hip behind
KT1) against the host divided writer (grk_amd_write_tile_parts), which tests/test_tile_parts_writer_cpu.py holds to the model
tests/tileparts.py byte for byte.

  chosen starts, chosen tables   grk_amd_stage_assemble_parts: every two-part boundary of a 36-packet tile, thirds / an empty middle part
                                 with PLT / SOP / EPH on and off, 255 parts of one packet, three tiles in one call
  the serial PLT path            65 536 packets of two-byte entries: part 0's entries pass one marker segment, part 1's do not
  real encodes                   every supported (order, letter) through grk_amd_assemble_device, appended calls, table 3, the
                                 asynchronous form, the refusals
  whole images                   grk_amd_encode_image, grk_amd_encode_surface(_device), grk_amd_encode_packed on both routes against the
                                 model's cut of the undivided file, and decoded back
All comparisons are exact."""
import numpy as np
import pytest
import torch

import grok_amd as G
import gpuutil as U
import packedref as P
import synth
import tileparts as TP
import tileparts_cases as TC
from t2read_cases import coded, draw_lengths, table_of, tile_params
from test_precincts_cpu import exps_from_sizes
from test_t2_reader_subsampled_cpu import make_planes

pytestmark = pytest.mark.gpu
PLT, SOP, EPH, TLM = G.CS_PLT, G.CS_SOP, G.CS_EPH, G.CS_TLM
Q = tile_params(precincts=[(3, 3), (4, 3)])
SUPPORTED = [(0, G.TP_R), (0, G.TP_L), (0, G.TP_C), (1, G.TP_R), (1, G.TP_L), (1, G.TP_C), (2, G.TP_R), (4, G.TP_C)]
UNSUPPORTED = [(2, G.TP_L), (2, G.TP_C), (3, G.TP_R), (3, G.TP_L), (3, G.TP_C), (4, G.TP_R), (4, G.TP_L)]


def _differs(got, want, what):
    if got != want:
        g, w = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
        n = min(g.size, w.size)
        d = np.nonzero(g[:n] != w[:n])[0]
        raise AssertionError("%s: %d bytes against %d, the first difference at byte %s" % (what, g.size, w.size, int(d[0]) if d.size else n))


def _staged(p, idx, table, data, flags, starts):
    """the staged divided call == the host divided writer, tile by tile and part by part -> the device's bytes"""
    c = U.ctx()
    bpt = len(table) // len(idx)
    want = [G.write_tile_parts(p, int(t), table[i * bpt:(i + 1) * bpt], data, flags, starts=starts) for i, t in enumerate(idx)]
    n, lens = c.stage_assemble_parts(p, idx, table, data, flags, starts=starts)
    assert c.assembled_parts() == len(want[0][1])
    assert lens.tolist() == [w[1] for w in want]
    assert n == sum(len(w[0]) for w in want)
    got = bytes(c.fetch_assembled(0, n))
    _differs(got, b"".join(w[0] for w in want), "starts %s flags %x" % (starts if starts is None or len(starts) < 6 else "...", flags))
    # the tables: the tiles' spans in 0 / 1, the parts' lengths in 3
    spans = U.from_dev_ptr(c.assembled_table_ptr(1), 4 * len(idx)).view(np.uint32)
    assert spans.tolist() == [len(w[0]) for w in want]
    at = U.from_dev_ptr(c.assembled_table_ptr(0), 8 * len(idx)).view(np.uint64)
    assert at.tolist() == np.concatenate([[0], np.cumsum(spans)[:-1]]).tolist()
    t3 = U.from_dev_ptr(c.assembled_table_ptr(3), 4 * lens.size).view(np.uint32).reshape(lens.shape)
    assert np.array_equal(t3, lens) and t3.sum(axis=1).tolist() == spans.tolist()
    return got


def test_two_parts_at_every_packet_boundary():
    tab = table_of(draw_lengths(Q, 820), 821)
    for k in range(37):
        got = _staged(Q, [0], tab, coded(), (PLT if k % 2 == 0 else SOP | EPH) | G.CS_PROG(2), [0, k])
        assert got[10:12] == bytes([0, 2])
    # a part without packets carries no PLT: 14 bytes
    assert _staged(Q, [0], tab, coded(), PLT, [0, 0])[:14] == b"\xff\x90\x00\x0a\x00\x00" + (14).to_bytes(4, "big") + bytes([0, 2]) + b"\xff\x93"


@pytest.mark.parametrize("flags", [0, PLT, PLT | SOP | EPH, SOP, EPH, PLT | EPH])
def test_thirds_and_an_empty_middle_part(flags):
    for order in (0, 3):
        tab = table_of(draw_lengths(Q, 800 + order), 810 + order)
        for b in (TP.thirds(0, 36), TP.empty_middle(0, 36)):
            _staged(Q, [7], tab, coded(), flags | G.CS_PROG(order), [0] + b)


def test_one_packet_per_part_up_to_the_255th():
    p = TC.many_packets_params()
    tab = table_of(draw_lengths(p, 500), 501)
    got = _staged(p, [0], tab, coded(), PLT | SOP, [0] + TP.every_packet(0, 320))
    assert U.ctx().assembled_parts() == 255 and got[10:12] == bytes([0, 255])


def test_three_tiles_in_one_call():
    p = TC.many_packets_params()
    tab = np.concatenate([table_of(draw_lengths(p, 600 + t), 610 + t) for t in range(3)])
    got = _staged(p, [3, 0, 65534], tab, coded(), PLT | EPH | G.CS_PROG(1), [0, 40, 40, 100, 319, 320])
    assert got[4:6] == bytes([0, 3])
    # ... and divided by name: the staged call takes the flags' division when no starts are given
    c = U.ctx()
    starts, npk = G.tile_part_starts(p, G.CS_PROG(1) | G.CS_TP(G.TP_C))
    assert npk == 320 and len(starts) == 8
    a = _staged(p, [3, 0, 65534], tab, coded(), PLT | G.CS_PROG(1) | G.CS_TP(G.TP_C), None)
    assert a == _staged(p, [3, 0, 65534], tab, coded(), PLT | G.CS_PROG(1), starts) and c.assembled_parts() == 8


def test_refusals_come_from_the_host_check():
    c = U.ctx()
    tab = table_of(draw_lengths(Q, 1), 2)
    for bad in ([0, 20, 10], [0, 37], [1, 5], [0] * 256):
        with pytest.raises(G.StageError) as e:
            c.stage_assemble_parts(Q, [0], tab, coded(), PLT, starts=bad)
        assert e.value.code == G.ERR_INVALID and e.value.reason, bad
    for order, letter in UNSUPPORTED:
        with pytest.raises(G.StageError) as e:
            c.stage_assemble_parts(Q, [0], tab, coded(), G.CS_PROG(order) | G.CS_TP(letter))
        assert e.value.code == G.ERR_UNSUPPORTED and "P" in e.value.reason


def _plt_segments(frame):
    """[Lplt] of the PLT marker segments of a tile-part, read from its header"""
    at, out = 12, []
    while frame[at:at + 2] == b"\xff\x58":
        out.append(int.from_bytes(frame[at + 2:at + 4], "big"))
        assert frame[at + 4] == len(out) - 1
        at += 2 + out[-1]
    assert frame[at:at + 2] == b"\xff\x93"
    return out


def test_a_part_whose_plt_passes_one_marker_segment_takes_the_serial_path():
    """65 536 packets of one block each (precincts of 2 x 2 samples, no DWT level), every row 128 .. 140 bytes out of one run of 64 KB:
    two-byte PLT entries.  Cut at packet 40 000: part 0's 80 000 entry bytes pass 65 532, part 1's 51 072 do not."""
    p = G.TileParams.make(512, 512, 1, 8, 0, cblk=(2, 2), precincts=[(1, 1)])
    rng = np.random.default_rng(3)
    n = len(G.tile_layout(p)[0])
    assert n == 65536
    data = rng.integers(0, 256, 1 << 16, dtype=np.uint8)
    tab = np.zeros(n, G.capi.CODED_DTYPE)
    tab["length"] = rng.integers(128, 141, n)
    tab["offset"] = rng.integers(0, (1 << 16) - 140, n)
    got = _staged(p, [0], tab, data, PLT, [0, 40000])
    first = int.from_bytes(got[6:10], "big")
    segs0, segs1 = _plt_segments(got), _plt_segments(got[first:])
    assert len(segs0) == 2 and segs0[0] == 3 + 65532 and segs0[1] == 3 + 80000 - 65532
    assert segs1 == [3 + 2 * 25536]


# ---- real encodes ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def encoded():
    """3 x 192 x 256, 4 levels, precincts 128 / 64 (the shape of tests/test_gpu_t2_device.py::test_orders_and_markers)"""
    px = synth.g2(3, 192, 256, 8, seed=5)
    return G.TileParams.make(256, 192, 3, 8, 4, precincts=exps_from_sizes([(128, 128), (64, 64)], 4)), px


def _reencode(encoded):
    """the context's latest encode is this one (the arena's order is the run's: the table is this call's) -> parameters, table, bytes"""
    p, px = encoded
    table, data = U.ctx().encode_host(p, px)
    return p, table, data


@pytest.mark.parametrize("order,letter", SUPPORTED)
def test_assemble_device_under_the_flag_equals_the_host_writer(encoded, order, letter):
    p, table, data = _reencode(encoded)
    c = U.ctx()
    for extra in (PLT, SOP | EPH):
        flags = extra | G.CS_PROG(order) | G.CS_TP(letter)
        want, want_lens = G.write_tile_parts(p, 5, table, data, flags)
        n, lens = c.assemble_device(p, [5], flags)
        assert n == len(want) == int(lens[0])
        _differs(bytes(c.fetch_assembled(0, n)), want, "order %d letter %d flags %x" % (order, letter, extra))
        k = c.assembled_parts()
        assert k == len(want_lens) and U.from_dev_ptr(c.assembled_table_ptr(3), 4 * k).view(np.uint32).tolist() == want_lens
        if (order, letter) == (0, G.TP_L):
            assert k == 1
        else:
            assert k > 1, "the flag must divide: %d parts" % k
    # LRCP + L is the undivided call's output, and an undivided call behind a divided one is what it was
    if (order, letter) == (0, G.TP_L):
        plain = G.write_tile_part(p, 5, table, data, PLT)
        for f in (PLT | G.CS_TP(G.TP_L), PLT):
            n, _ = c.assemble_device(p, [5], f)
            assert bytes(c.fetch_assembled(0, n)) == plain and c.assembled_parts() == 1


def test_an_appended_call_and_the_asynchronous_form(encoded):
    p, table, data = _reencode(encoded)
    c = U.ctx()
    f1, f2 = PLT | G.CS_PROG(1) | G.CS_TP(G.TP_C), PLT | SOP | G.CS_PROG(2) | G.CS_TP(G.TP_R)
    a, b = G.write_tile_parts(p, 1, table, data, f1)[0], G.write_tile_parts(p, 2, table, data, f2)[0]
    n1, _ = c.assemble_device(p, [1], f1)
    n2, lens2 = c.assemble_device(p, [2], f2, dst_offset=n1)
    assert (n1, n2) == (len(a), len(b))
    _differs(bytes(c.fetch_assembled(0, n1 + n2)), a + b, "a call appended behind another")
    assert U.from_dev_ptr(c.assembled_table_ptr(0), 8).view(np.uint64).tolist() == [n1]
    # the asynchronous form on a stream of the caller's
    st = torch.cuda.Stream()
    c.assemble_device_async(p, [2], f2, st.cuda_stream)
    st.synchronize()
    total = U.from_dev_ptr(c.assembled_table_ptr(2), 16).view(np.uint64)
    assert int(total[0]) == len(b) and c.assembled_parts() == 5
    _differs(bytes(U.from_dev_ptr(c.assembled_device_ptr(), len(b))), b, "the asynchronous form")
    assert U.from_dev_ptr(c.assembled_table_ptr(3), 20).view(np.uint32).sum() == len(b)


def test_unsupported_pairs_raise_before_any_launch(encoded):
    p, table, data = _reencode(encoded)
    c = U.ctx()
    for order, letter in UNSUPPORTED:
        with pytest.raises(G.StageError) as e:
            c.assemble_device(p, [0], PLT | G.CS_PROG(order) | G.CS_TP(letter))
        assert e.value.code == G.ERR_UNSUPPORTED and "P" in e.value.reason
    n, _ = c.assemble_device(p, [0], PLT)
    assert bytes(c.fetch_assembled(0, n)) == G.write_tile_part(p, 0, table, data, PLT)


# ---- whole images ------------------------------------------------------------------------------------------------------------------------
def routes(monkeypatch, c, make):
    """make() by the device route and under GRK_AMD_IMAGE_T2=host -> the file, both equal, each by the route it was asked for
    (tests/test_gpu_t2_joint.py)"""
    monkeypatch.delenv("GRK_AMD_IMAGE_T2", raising=False)
    before = c.encode_route_counters()
    dev = make()
    after = c.encode_route_counters()
    assert (after[0] - before[0], after[1] - before[1]) == (1, 0), "the default route did not assemble on the device"
    monkeypatch.setenv("GRK_AMD_IMAGE_T2", "host")
    host = make()
    assert c.encode_route_counters() == (after[0], after[1] + 1), "GRK_AMD_IMAGE_T2=host did not go to the host writer"
    monkeypatch.delenv("GRK_AMD_IMAGE_T2")
    _differs(dev, host, "the device route against the host route")
    return dev


def _model_cut(undivided, tiles, flags, sampling=None):
    b = {t: G.tile_part_starts(p, flags, sampling)[0][1:] for t, p in enumerate(tiles)}
    return TP.cut(undivided, b, plt="keep" if flags & PLT else "drop", tnsot="all", order="tile", tlm="write" if flags & TLM else None, stlm=(1, 1))


LAYOUTS = {"2x2": dict(w=320, h=256, tile=(160, 128)), "ragged": dict(w=300, h=200, tile=(128, 96), offset=(6, 10))}


@pytest.mark.parametrize("order", [0, 2], ids=["lrcp", "rpcl"])
@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_encode_image_divided_on_both_routes_equals_the_models_cut(monkeypatch, name, order):
    kw = LAYOUTS[name]
    layout = G.ImageLayout.make(kw["w"], kw["h"], *kw["tile"], offset=kw.get("offset", (0, 0)))
    base = G.TileParams.make(1, 1, 3, 8, 3, precincts=[(4, 4), (5, 5), (5, 5), (6, 6)] if order == 2 else None)
    px = synth.g2(3, kw["h"], kw["w"], 8, seed=order + len(name))
    c = U.ctx()
    flags = TLM | PLT | G.CS_PROG(order)
    # grk_amd_encode_image is not among the calls the route counters count: which route ran is read from the context's latest
    # assemble call -- the device route leaves four parts per tile behind, the host writer leaves the undivided call's one
    monkeypatch.delenv("GRK_AMD_IMAGE_T2", raising=False)
    undivided = c.encode_image(layout, base, px, flags)
    assert c.assembled_parts() == 1
    got = c.encode_image(layout, base, px, flags | G.CS_TP(G.TP_R))
    assert c.assembled_parts() == 4, "the default route did not assemble on the device"
    assert c.encode_image(layout, base, px, flags) == undivided and c.assembled_parts() == 1
    monkeypatch.setenv("GRK_AMD_IMAGE_T2", "host")
    host = c.encode_image(layout, base, px, flags | G.CS_TP(G.TP_R))
    assert c.assembled_parts() == 1, "GRK_AMD_IMAGE_T2=host did not go to the host writer"
    monkeypatch.delenv("GRK_AMD_IMAGE_T2")
    _differs(got, host, "the device route against the host route")
    tiles = G.layout_tiles(layout, base)
    cut = _model_cut(undivided, tiles, flags | G.CS_TP(G.TP_R))
    assert len(cut.parts) == 4 * len(tiles)
    _differs(got, cut.cs, "the divided file against the model's cut of the undivided one")
    assert np.array_equal(np.asarray(c.decode_image(got)).reshape(px.shape), px)
    # a pair the rule refuses is refused before any work: RPCL + C, PCRL + R
    refused = TLM | PLT | (G.CS_PROG(2) | G.CS_TP(G.TP_C) if order == 2 else G.CS_PROG(3) | G.CS_TP(G.TP_R))
    with pytest.raises(RuntimeError, match=r"failed: -2 \(.*P"):
        c.encode_image(layout, base, px, refused)


def test_an_nv12_surface_under_cprl_divided_at_c(monkeypatch):
    layout = G.ImageLayout.make(70, 38, 32, 32)
    surface, sampling, nbytes = G.Surface.make("NV12", layout, None, 0)
    base = G.TileParams.make(1, 1, 3, 8, 2, mct=False)
    planes = make_planes(layout, sampling, 8, seed=3)
    buf = np.random.default_rng(9).integers(0, 256, nbytes, dtype=np.uint8)
    surface.scatter(buf, planes, 1)
    c = U.ctx()
    flags = PLT | TLM | G.CS_PROG(4)
    undivided = c.encode_surface(layout, base, sampling, surface, buf, flags)
    host = routes(monkeypatch, c, lambda: c.encode_surface(layout, base, sampling, surface, buf, flags | G.CS_TP(G.TP_C)))
    cut = _model_cut(undivided, G.layout_tiles(layout, base), flags | G.CS_TP(G.TP_C), sampling)
    assert len(cut.parts) == 3 * 6
    _differs(host, cut.cs, "the divided surface file against the model's cut")
    # the file left in device memory, decoded where it lies
    d_buf = U.to_dev(buf)
    ptr, n = c.encode_surface_device(layout, base, sampling, surface, d_buf.data_ptr(), flags | G.CS_TP(G.TP_C), cap=nbytes)
    _differs(U.from_dev_ptr(ptr, n).tobytes(), host, "the file in device memory")
    total = sum(a.size for a in planes)
    out = U._settled(torch.zeros(total, dtype=torch.uint8, device="cuda"))
    c.decode_image_resident_ex(ptr, n, out.data_ptr(), out.numel())
    c.decode_status()
    assert np.array_equal(out.cpu().numpy(), np.concatenate([a.reshape(-1) for a in planes]))
    # the rate-targeted twin refuses the flag
    with pytest.raises(G.RateError) as e:
        c.encode_surface_rate(layout, base, sampling, surface, buf, 4000, flags | G.CS_TP(G.TP_C))
    assert e.value.code == G.ERR_UNSUPPORTED and "GRK_AMD_CS_TP" in e.value.reason


def test_a_packed_frame_divided(monkeypatch):
    w, h, fmt = 66, 10, P.YUY2
    rng = np.random.default_rng(fmt)
    planes = [rng.integers(0, 256, (h, n)).astype(np.uint8) for n in (w, (w + 1) // 2, (w + 1) // 2)]
    frame = P.pack(fmt, 8, *planes, 0, rng.integers(0, 256, P.frame_bytes(fmt, w, h, 0), dtype=np.uint8))
    layout = G.ImageLayout.make(w, h)
    base = G.TileParams.make(1, 1, 3, 8, 2, mct=False)
    c = U.ctx()
    flags = PLT | G.CS_PROG(1)
    undivided = c.encode_packed(layout, base, fmt, frame, 0, flags)
    got = routes(monkeypatch, c, lambda: c.encode_packed(layout, base, fmt, frame, 0, flags | G.CS_TP(G.TP_C)))
    cut = _model_cut(undivided, G.layout_tiles(layout, base), flags | G.CS_TP(G.TP_C), [(1, 1), (2, 1), (2, 1)])
    assert len(cut.parts) == 9
    _differs(got, cut.cs, "the divided packed frame against the model's cut")
    assert all(np.array_equal(a, b) for a, b in zip(c.decode_image_planes(got), planes))


# ---- what does not write tile-parts says so ----------------------------------------------------------------------------------------------
def _refusal_case():
    """a 64 x 48 image as planes (4:4:4, 4:2:0), an NV12 surface and a YUY2 frame, on the host and on the device"""
    layout = G.ImageLayout.make(64, 48)
    surface, s420, nbytes = G.Surface.make("NV12", layout, None, 0)
    planes = make_planes(layout, s420, 8, seed=7)
    buf = np.zeros(nbytes, np.uint8)
    surface.scatter(buf, planes, 1)
    rng = np.random.default_rng(8)
    yuv = [rng.integers(0, 256, (48, n)).astype(np.uint8) for n in (64, 32, 32)]
    frame = P.pack(P.YUY2, 8, *yuv, 0, np.zeros(P.frame_bytes(P.YUY2, 64, 48, 0), np.uint8))
    return dict(layout=layout, surface=surface, s420=s420, nbytes=nbytes, planes=planes, buf=buf, frame=frame,
                px=synth.g2(3, 48, 64, 8, seed=9), plain=G.TileParams.make(1, 1, 3, 8, 2), sub=G.TileParams.make(1, 1, 3, 8, 2, mct=False))


# every rate- and quality-targeted whole-image call: name -> the call with `flags` on context c and case k
TARGETED = {
    "image_rate": lambda c, k, f: c.encode_image_rate(k["layout"], k["plain"], k["px"], 1 << 20, f),
    "image_rate_joint": lambda c, k, f: c.encode_image_rate(k["layout"], k["plain"], k["px"], 1 << 20, f, joint=True),
    "image_quality": lambda c, k, f: c.encode_image_quality(k["layout"], k["plain"], k["px"], 40.0, flags=f),
    "image_subsampled_rate": lambda c, k, f: c.encode_image_subsampled_rate(k["layout"], k["sub"], k["s420"], k["planes"], 1 << 20, f),
    "image_subsampled_quality": lambda c, k, f: c.encode_image_subsampled_quality(k["layout"], k["sub"], k["s420"], k["planes"], 40.0, flags=f),
    "surface_rate": lambda c, k, f: c.encode_surface_rate(k["layout"], k["sub"], k["s420"], k["surface"], k["buf"], 1 << 20, f),
    "surface_quality": lambda c, k, f: c.encode_surface_quality(k["layout"], k["sub"], k["s420"], k["surface"], k["buf"], 40.0, flags=f),
    "surface_rate_device": lambda c, k, f: c.encode_surface_rate_device(k["layout"], k["sub"], k["s420"], k["surface"], k["buf"], 1 << 20, f),
    "surface_quality_device": lambda c, k, f: c.encode_surface_quality_device(k["layout"], k["sub"], k["s420"], k["surface"], k["buf"], 40.0, flags=f),
    "packed_rate": lambda c, k, f: c.encode_packed_rate(k["layout"], k["sub"], P.YUY2, k["frame"], 1 << 20, 0, f),
    "packed_quality": lambda c, k, f: c.encode_packed_quality(k["layout"], k["sub"], P.YUY2, k["frame"], 40.0, flags=f),
    "packed_rate_device": lambda c, k, f: c.encode_packed_rate_device(k["layout"], k["sub"], P.YUY2, k["frame"], 1 << 20, 0, f),
    "packed_quality_device": lambda c, k, f: c.encode_packed_quality_device(k["layout"], k["sub"], P.YUY2, k["frame"], 40.0, flags=f),
}


@pytest.mark.parametrize("name", sorted(TARGETED))
def test_every_rate_and_quality_targeted_call_refuses_the_flag(name):
    """LRCP + R, a pair the plain calls write: GRK_AMD_ERR_UNSUPPORTED with a reason that names the flag, never an undivided (or a
    divided) file; the same call without the flag goes through"""
    c, k = U.ctx(), _refusal_case()
    with pytest.raises(G.RateError) as e:
        TARGETED[name](c, k, PLT | G.CS_TP(G.TP_R))
    assert e.value.code == G.ERR_UNSUPPORTED and "GRK_AMD_CS_TP" in e.value.reason, e.value.reason
    out = TARGETED[name](c, k, PLT)
    assert out[1] > 0 if name.endswith("_device") else len(out[0]) > 0


def test_a_staged_table_with_its_own_zero_bit_planes_divided():
    """the general zero-bit-plane tree's plan (KT1's msbs instance, what grk_amd_assemble_rate_device runs) under a division of the flags"""
    c = U.ctx()
    blocks = G.tile_layout(Q)[0]
    rng = np.random.default_rng(330)
    msbs = np.array([rng.integers(0, max(1, b.kmax)) for b in blocks])
    tab = table_of(draw_lengths(Q, 331), 332, msbs)
    for order, letter, extra in ((0, G.TP_R, PLT), (1, G.TP_C, SOP | EPH), (2, G.TP_R, PLT | SOP)):
        flags = extra | G.CS_PROG(order) | G.CS_TP(letter)
        want, want_lens = G.write_tile_parts(Q, 9, tab, coded(), flags | G.CS_BLOCK_MSBS)
        assert len(want_lens) == 2
        n, lens = c.stage_assemble_msbs(Q, [9], tab, coded(), flags)
        assert n == len(want) == int(lens[0]) and c.assembled_parts() == 2
        _differs(bytes(c.fetch_assembled(0, n)), want, "msbs plan, order %d" % order)
        assert U.from_dev_ptr(c.assembled_table_ptr(3), 8).view(np.uint32).tolist() == want_lens
        assert want != G.write_tile_parts(Q, 9, tab, coded(), flags)[0], "the table's zero bit-planes must matter"


def test_the_node_refuses_the_flag():
    nd = G.Node([0])
    try:
        layout = G.ImageLayout.make(64, 64)
        base = G.TileParams.make(1, 1, 1, 8, 2)
        with pytest.raises(RuntimeError, match="-2"):
            nd.encode_image(layout, base, np.zeros((1, 64, 64), np.uint8), G.CS_TP(G.TP_R))
        assert len(nd.encode_image(layout, base, np.zeros((1, 64, 64), np.uint8), 0)) > 0
        d_px = U.to_dev(np.zeros((1, 64, 64), np.uint8))
        with pytest.raises(RuntimeError, match=r"failed: -2 \(.*GRK_AMD_CS_TP"):
            nd.encode_image_device(layout, base, d_px.data_ptr(), 64 * 64, 0, G.CS_TP(G.TP_R))
        assert len(nd.encode_image_device(layout, base, d_px.data_ptr(), 64 * 64, 0, 0)) > 0
    finally:
        nd.close()
