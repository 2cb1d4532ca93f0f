"""ctypes wrapper of tests/c/reduce_host.cpp: the reference decoder with cp_reduce (grk_decompress -r N), on its own and through
the plugin loader.  Built on first use into a temporary directory against oracle/_ref/libgrokj2k_ref.so as refharness loads it;
available where oracle/_ref is (tests skip otherwise, as with refharness)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import refharness as R

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.join(_HERE, "..")
_lib = None


def have():
    return R.have_ref()


def lib():
    global _lib
    if _lib is None:
        R.lib()                                 # the reference library (RTLD_GLOBAL) and the harness, initialised
        out = os.path.join(tempfile.mkdtemp(prefix="reduce_host_"), "libreduce_host.so")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fPIC", "-shared",
                               "-I", os.path.join(_ROOT, "include"), os.path.join(_HERE, "c", "reduce_host.cpp"), "-o", out])
        # (the grk_* symbols stay undefined: they bind to the reference library refharness loaded with RTLD_GLOBAL -- the instance
        #  whose plugin loader ref_plugin_load set up)
        L = C.CDLL(out)
        vp, u32, u64, i32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int32
        L.rh_read_header.restype = i32
        L.rh_read_header.argtypes = [vp, u64, u32, vp, i32]
        L.rh_decode.restype = i32
        L.rh_decode.argtypes = [vp, u64, u32, vp, u64, vp, i32]
        L.rh_plugin_decompress.restype = i32
        L.rh_plugin_decompress.argtypes = [vp, u64, C.c_char_p, u32, vp, u64, vp, i32, vp]
        _lib = L
    return _lib


def _ncomps(cs):
    b = bytes(cs[:42])
    assert b[0:4] == b"\xff\x4f\xff\x51"
    return (b[40] << 8) | b[41]


def header_rects(cs, reduce):
    """grk_decompress_read_header with cp_reduce = reduce -> [(x0, y0, w, h)] of every component, or the negative code"""
    Cn = _ncomps(cs)
    buf = np.frombuffer(cs, np.uint8).copy()
    dims = np.zeros((Cn, 4), np.uint32)
    rc = lib().rh_read_header(buf.ctypes.data, buf.size, int(reduce), dims.ctypes.data, Cn)
    return [tuple(int(v) for v in d) for d in dims] if rc == 0 else int(rc)


def _planes(out, dims):
    res, at = [], 0
    for _, _, w, h in dims:
        res.append(out[at:at + int(w) * int(h)].reshape(int(h), int(w)).copy())
        at += int(w) * int(h)
    return res


def decode(cs, reduce):
    """the reference's decode with cp_reduce = reduce -> [(h_c, w_c) int32] per component, or the negative code"""
    Cn = _ncomps(cs)
    buf = np.frombuffer(cs, np.uint8).copy()
    cap = max(1 << 16, len(cs) * 64)
    hdr = header_rects(cs, reduce)
    if not isinstance(hdr, int):
        cap = max(cap, sum(w * h for _, _, w, h in hdr))
    out = np.zeros(cap, np.int32)
    dims = np.zeros((Cn, 4), np.uint32)
    rc = lib().rh_decode(buf.ctypes.data, buf.size, int(reduce), out.ctypes.data, cap, dims.ctypes.data, Cn)
    return _planes(out, dims) if rc == 0 else int(rc)


def crop(planes, wh):
    """The reduced tile (w, h = grk_amd_reduced_tile_rect) out of the reference's reduced components.  With an origin off the 2^r
    grid the reference's composite image is ceil(w / 2^r) x ceil(h / 2^r) -- a column / row more than the tile's resolution holds
    (its header sizes the components from the width, CodeStreamDecompress.cpp:412-420 from the bounds); what lies beyond the
    resolution is not defined by the stream."""
    w, h = wh
    for p in planes:
        assert p.shape[0] >= h and p.shape[1] >= w, (p.shape, wh)
    return [np.ascontiguousarray(p[:h, :w]) for p in planes]


def plugin_decompress(cs, reduce):
    """grk_plugin_decompress with cp_reduce = reduce, through the plugin R.plugin_load / R.plugin_init loaded, the stream in a file
    as with grk_decompress -i -> (rc, [(h_c, w_c) int32] or None, stages [header, Tier-2, post-T1, clean])"""
    Cn = _ncomps(cs)
    buf = np.frombuffer(cs, np.uint8).copy()
    hdr = header_rects(cs, reduce)
    if isinstance(hdr, int):                    # (a reduce the host refuses: room for the full image)
        hdr = header_rects(cs, 0)
    cap = max(1 << 16, sum(w * h for _, _, w, h in hdr))
    out = np.zeros(cap, np.int32)
    dims = np.zeros((Cn, 4), np.uint32)
    stages = np.zeros(4, np.int32)
    fd, path = tempfile.mkstemp(suffix=".j2k")
    with os.fdopen(fd, "wb") as f:
        f.write(bytes(cs))
    try:
        rc = lib().rh_plugin_decompress(buf.ctypes.data, buf.size, path.encode(), int(reduce), out.ctypes.data, cap,
                                        dims.ctypes.data, Cn, stages.ctypes.data)
    finally:
        os.unlink(path)
    stored = int(stages[2]) > 0 and int(dims[:, 2].sum()) > 0
    return int(rc), (_planes(out, dims) if stored else None), [int(v) for v in stages]
