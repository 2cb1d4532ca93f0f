"""ctypes binding of include/grok_amd.h (no compute in Python; fails loudly without the .so)."""
import ctypes as C
import os
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
MAX_LEVELS = 10


class NativeLibraryMissing(RuntimeError):
    pass


def lib_path():
    # (GRK_AMD_LIB: another build of the same library, for A/B timing on one box -- tools/build_variant.sh)
    return os.environ.get("GRK_AMD_LIB") or os.path.join(_HERE, "lib", "libgrok_amd.so")


class TileParams(C.Structure):
    _fields_ = [("tile_w", C.c_uint32), ("tile_h", C.c_uint32), ("num_comps", C.c_uint16),
                ("prec", C.c_uint8), ("sgnd", C.c_uint8), ("irreversible", C.c_uint8),
                ("mct", C.c_uint8), ("num_levels", C.c_uint8), ("cblk_w_exp", C.c_uint8),
                ("cblk_h_exp", C.c_uint8), ("reserved", C.c_uint8 * 3),
                ("tile_x0", C.c_uint32), ("tile_y0", C.c_uint32), ("precinct_exp", C.c_uint8 * 12)]

    @classmethod
    def make(cls, w, h, comps, prec, levels, irreversible=False, mct=None, sgnd=False, cblk=(6, 6), part1=False, cblksty=0,
             origin=(0, 0), precincts=None):
        """origin = (x0, y0): where the tile lies on the canonical grid (image offset / tile grid position).
        precincts = [(PPx, PPy), ...] for resolutions 0 (coarsest) .. levels, exponents as in the COD marker; None: one
        precinct per resolution."""
        if mct is None:
            mct = comps >= 3
        p = cls(w, h, comps, prec, int(sgnd), int(irreversible), int(mct), levels, cblk[0], cblk[1])
        p.reserved[0] = int(part1)
        p.reserved[1] = int(cblksty)       # Part-1 decode: LAZY 1, RESET 2, TERMALL 4, VSC 8, PTERM 16, SEGSYM 32
        p.tile_x0, p.tile_y0 = int(origin[0]), int(origin[1])
        if precincts is not None:
            assert len(precincts) == levels + 1
            for r, (ppx, ppy) in enumerate(precincts):
                p.precinct_exp[r] = int(ppx) | (int(ppy) << 4)
        return p


class ImageLayout(C.Structure):
    """grk_amd_image_layout: image area [x0, x1) x [y0, y1) on the canonical grid, tile grid anchored at (tx0, ty0)."""
    _fields_ = [("x0", C.c_uint32), ("y0", C.c_uint32), ("x1", C.c_uint32), ("y1", C.c_uint32),
                ("tx0", C.c_uint32), ("ty0", C.c_uint32), ("t_width", C.c_uint32), ("t_height", C.c_uint32)]

    @classmethod
    def make(cls, w, h, tile_w=None, tile_h=None, offset=(0, 0), tile_origin=(0, 0)):
        return cls(offset[0], offset[1], offset[0] + w, offset[1] + h, tile_origin[0], tile_origin[1],
                   tile_w or offset[0] + w - tile_origin[0], tile_h or offset[1] + h - tile_origin[1])


class PixelLayout(C.Structure):
    """grk_amd_pixel_layout: how the pixels an encode reads / a decode writes lie in memory (all zero: tiles back to back, component
    planes, tight)."""
    _fields_ = [("interleaved", C.c_uint8), ("channels", C.c_uint8), ("fill", C.c_uint16), ("reserved", C.c_uint32),
                ("row_pitch", C.c_uint64), ("plane_pitch", C.c_uint64), ("tile_pitch", C.c_uint64)]

    @classmethod
    def make(cls, interleaved=False, channels=0, row_pitch=0, plane_pitch=0, tile_pitch=0, fill=0):
        return cls(int(bool(interleaved)), int(channels), int(fill), 0, int(row_pitch), int(plane_pitch), int(tile_pitch))


class Block(C.Structure):
    _fields_ = [("x0", C.c_uint32), ("y0", C.c_uint32), ("x1", C.c_uint32), ("y1", C.c_uint32),
                ("px", C.c_uint32), ("py", C.c_uint32), ("comp", C.c_uint16), ("res", C.c_uint8),
                ("band", C.c_uint8), ("kmax", C.c_uint8), ("reserved", C.c_uint8 * 3),
                ("stepsize", C.c_float), ("precinct", C.c_uint32)]


class CodedBlock(C.Structure):
    _fields_ = [("offset", C.c_uint64), ("length", C.c_uint32), ("missing_msbs", C.c_uint32)]


class StreamInfo(C.Structure):
    """grk_amd_stream_info: what a codestream's main header says (read_header)."""
    _fields_ = [("layout", ImageLayout), ("base", TileParams), ("flags", C.c_uint32), ("num_layers", C.c_uint16),
                ("guard_bits", C.c_uint8), ("qstyle", C.c_uint8), ("qcd_words", C.c_uint16 * (3 * MAX_LEVELS + 1)),
                ("num_qcd", C.c_uint32), ("comp_dx", C.c_uint8 * 4), ("comp_dy", C.c_uint8 * 4), ("num_tiles", C.c_uint32),
                ("num_blocks", C.c_uint64)]


class Rate(C.Structure):
    """grk_amd_rate: target_bytes (the blocks' bytes for encode_tiles_rate, the whole file for encode_image_rate), max_drop (Dmax;
    0 = 6, at most 12), allow_skip, joint (encode_image_rate: one set of tables and one multiplier over all geometry groups)"""
    _fields_ = [("target_bytes", C.c_uint64), ("max_drop", C.c_uint8), ("allow_skip", C.c_uint8), ("joint", C.c_uint8),
                ("reserved", C.c_uint8 * 5)]


class RateResult(C.Structure):
    """grk_amd_rate_result"""
    _fields_ = [("block_bytes", C.c_uint64), ("lagrange_bytes", C.c_uint64), ("file_bytes", C.c_uint64), ("distortion", C.c_double),
                ("lambda_", C.c_double), ("passes", C.c_uint32), ("reserved", C.c_uint32)]


class RateAllocResult(C.Structure):
    """grk_amd_rate_alloc_result: everything the allocator kernel reports (Context.stage_rate_alloc)"""
    _fields_ = [("block_bytes", C.c_uint64), ("lagrange_bytes", C.c_uint64), ("least_bytes", C.c_uint64), ("distortion", C.c_double),
                ("lambda_", C.c_double), ("feasible", C.c_uint32), ("steps", C.c_uint32)]


class Quality(C.Structure):
    """grk_amd_quality: target_psnr (dB over all samples of all components; > 0: used, inf: D = 0), target_distortion (used when
    target_psnr == 0: D in the units of RateResult.distortion), max_drop (Dmax; 0 = 6, at most 12), allow_skip"""
    _fields_ = [("target_psnr", C.c_double), ("target_distortion", C.c_double), ("max_drop", C.c_uint8), ("allow_skip", C.c_uint8),
                ("reserved", C.c_uint8 * 6)]


class QualityResult(C.Structure):
    """grk_amd_quality_result"""
    _fields_ = [("block_bytes", C.c_uint64), ("lagrange_bytes", C.c_uint64), ("file_bytes", C.c_uint64), ("distortion", C.c_double),
                ("budget", C.c_double), ("psnr", C.c_double), ("lambda_", C.c_double), ("steps", C.c_uint32), ("reserved", C.c_uint32)]


class QualityAllocResult(C.Structure):
    """grk_amd_quality_alloc_result: everything the quality allocator kernel reports (Context.stage_quality_alloc)"""
    _fields_ = [("block_bytes", C.c_uint64), ("lagrange_bytes", C.c_uint64), ("shortest_bytes", C.c_uint64), ("distortion", C.c_double),
                ("floor", C.c_double), ("lambda_", C.c_double), ("feasible", C.c_uint32), ("steps", C.c_uint32)]


class RateError(RuntimeError):
    """a rate-targeted call refused: .code (ERR_UNSUPPORTED -2, ERR_INVALID -3, ERR_OVERFLOW -5) and the context's reason"""

    def __init__(self, what, code, reason):
        RuntimeError.__init__(self, "%s failed: %d (%s)" % (what, code, reason))
        self.code, self.reason = int(code), reason


class ImageView(C.Structure):
    """grk_amd_image_view: reduce (the N finest resolutions dropped) and a window [x0, x1) x [y0, y1) of the (reduced) image, all
    four 0 = the whole image"""
    _fields_ = [("reduce", C.c_uint32), ("x0", C.c_uint32), ("y0", C.c_uint32), ("x1", C.c_uint32), ("y1", C.c_uint32)]

    @classmethod
    def make(cls, reduce=0, window=None):
        x0, y0, x1, y1 = window if window is not None else (0, 0, 0, 0)
        return cls(int(reduce), int(x0), int(y0), int(x1), int(y1))


class SurfaceComp(C.Structure):
    """grk_amd_surface_comp: where one component lies on a surface (bytes; step in samples, 0 reads as 1; shift: the zero bits below
    a sample in its container, 0 = LSB-aligned)"""
    _fields_ = [("offset", C.c_uint64), ("row_pitch", C.c_uint64), ("step", C.c_uint32), ("shift", C.c_uint32)]


SURFACE_FORMATS = {"NV12": 0, "NV21": 1, "I420": 2, "YV12": 3, "NV16": 4, "I422": 5, "I444": 6}
# the MSB-aligned two-byte forms of NV12 (GRK_AMD_SURFACE_P016 = 7) and NV16 (GRK_AMD_SURFACE_P216 = 8): name -> (id, the precision
# the name implies); shift = 16 - prec on every component
SURFACE_FORMATS_MSB = {"P010": (7, 10), "P012": (7, 12), "P016": (7, 16), "P210": (8, 10), "P212": (8, 12), "P216": (8, 16)}


class SurfaceError(RuntimeError):
    """a surface call refused: .code (ERR_UNSUPPORTED -2, ERR_INVALID -3, ERR_OVERFLOW -5) and the reason"""

    def __init__(self, what, code, reason):
        RuntimeError.__init__(self, "%s failed: %d (%s)" % (what, code, reason))
        self.code, self.reason = int(code), reason


class Surface(C.Structure):
    """grk_amd_surface: a video surface component by component -- sample (x, y) of component c at
    base + comp[c].offset + y * comp[c].row_pitch + x * comp[c].step * bps"""
    _fields_ = [("comp", SurfaceComp * 4)]

    @classmethod
    def of(cls, comps):
        """comps: [(offset, row_pitch, step)] or [(offset, row_pitch, step, shift)] per component"""
        s = cls()
        for k, comp in enumerate(comps):
            s.comp[k] = _surface_comp(comp)
        return s

    @classmethod
    def make(cls, fmt, layout, prec=None, pitch=0):
        """A named format ("NV12", "NV21", "I420", "YV12", "NV16", "I422", "I444", "P010", "P012", "P016", "P210", "P212", "P216" or a
        format's number) for the image area of `layout` (grk_amd_surface_format) -> (surface, [(dx, dy)] per component, bytes).
        prec: 8 where neither given nor implied by the name; a P0xx / P2xx name implies its own and a different one is an error"""
        if fmt in SURFACE_FORMATS_MSB:
            number, implied = SURFACE_FORMATS_MSB[fmt]
            if prec is not None and int(prec) != implied:
                raise ValueError("%s holds %d-bit samples, not %d" % (fmt, implied, prec))
            fmt, prec = number, implied
        elif prec is None:
            prec = 8
        s = cls()
        dx, dy = (C.c_uint8 * 4)(), (C.c_uint8 * 4)()
        nc, nbytes = C.c_uint32(0), C.c_uint64(0)
        rc = lib().grk_amd_surface_format(SURFACE_FORMATS.get(fmt, fmt), C.byref(layout), int(prec), int(pitch), C.byref(s), dx, dy,
                                          C.byref(nc), C.byref(nbytes))
        if rc:
            raise SurfaceError("surface_format", rc, "format %r, pitch %d, %d bits" % (fmt, pitch, prec))
        return s, [(dx[k], dy[k]) for k in range(nc.value)], int(nbytes.value)

    def gather(self, buf, sizes, bps):
        """component k's samples out of the uint8 array `buf` holding the surface: [2-D array] (sizes: [(w, h)], pitches resolved)"""
        out = []
        for k, (w, h) in enumerate(sizes):
            c = self.comp[k]
            step = c.step or 1
            pitch = c.row_pitch or ((w - 1) * step + 1) * bps
            rows = np.lib.stride_tricks.as_strided(buf[c.offset:], (h, w, bps), (pitch, step * bps, 1))
            out.append(np.ascontiguousarray(rows).view(np.uint8 if bps == 1 else np.uint16).reshape(h, w) >> c.shift)
        return out

    def scatter(self, buf, planes, bps):
        """the reverse: plane k's samples, << shift, onto the surface in `buf` (nothing else is written)"""
        for k, pl in enumerate(planes):
            h, w = pl.shape
            c = self.comp[k]
            step = c.step or 1
            pitch = c.row_pitch or ((w - 1) * step + 1) * bps
            rows = np.lib.stride_tricks.as_strided(buf[c.offset:], (h, w, bps), (pitch, step * bps, 1))
            rows[...] = (np.ascontiguousarray(pl, np.uint8 if bps == 1 else np.uint16) << c.shift).view(np.uint8).reshape(h, w, bps)


def _surface_comp(comp):
    """(offset, row_pitch, step[, shift]) -> SurfaceComp"""
    offset, row_pitch, step = comp[:3]
    return SurfaceComp(int(offset), int(row_pitch), int(step), int(comp[3]) if len(comp) > 3 else 0)


def _sampling(sampling):
    return (C.c_uint8 * 4)(*[int(a) for a, _ in sampling]), (C.c_uint8 * 4)(*[int(b) for _, b in sampling])


def surface_bytes(layout, base, sampling, surface):
    """Bytes from the base to the end of the last sample of any component (grk_amd_surface_bytes); SurfaceError with the reason for
    an invalid surface"""
    dx, dy = _sampling(sampling)
    why = C.c_char_p()
    n = lib().grk_amd_surface_bytes(C.byref(layout), C.byref(base), dx, dy, C.byref(surface), C.byref(why))
    if n == 0:
        reason = (why.value or b"").decode()
        raise SurfaceError("surface_bytes", -2 if "16 bits" in reason else -3, reason)
    return int(n)


def surface_plan(layout, base, sampling, surface, cap, base_align=0, decode=False, allow_direct=True):
    """The plan of encode_surface / decode_surface (grk_amd_surface_plan): per run of components (in_place, PixelLayout, offset of
    its first sample); SurfaceError with the refusal"""
    dx, dy = _sampling(sampling)
    why = C.c_char_p()
    flags = (C.c_uint8 * 4)()
    lays = (PixelLayout * 4)()
    at = (C.c_uint64 * 4)()
    n = lib().grk_amd_surface_plan(C.byref(layout), C.byref(base), dx, dy, C.byref(surface), int(cap), int(base_align), int(bool(decode)),
                                   int(bool(allow_direct)), flags, lays, at, 4, C.byref(why))
    if n < 0:
        raise SurfaceError("surface_plan", n, (why.value or b"").decode())
    return [(bool(flags[r]), lays[r], int(at[r])) for r in range(n)]


PACKED_FORMATS = {"YUY2": 0, "UYVY": 1, "YVYU": 2, "Y216": 3, "V210": 4}


def packed_bytes(fmt, layout, prec, pitch=0):
    """A packed 4:2:2 frame (a name of PACKED_FORMATS or the format's number) for the image area of `layout` at `prec` bits
    (grk_amd_packed_bytes) -> (bytes from the base to the end of the last row's last container, the pitch: `pitch`, or the format's
    default for 0); SurfaceError with the refusal's code and reason"""
    p, why = C.c_uint64(int(pitch)), C.c_char_p()
    n = lib().grk_amd_packed_bytes(PACKED_FORMATS.get(fmt, fmt), C.byref(layout), int(prec), C.byref(p), C.byref(why))
    if n == 0:
        reason = (why.value or b"").decode()
        raise SurfaceError("packed_bytes", -2 if "odd x0" in reason else -3, reason)
    return int(n), int(p.value)


VIEW_UNIT_DTYPE = np.dtype([("tile", np.uint32), ("first_comp", np.uint32), ("num_comps", np.uint32), ("w", np.uint32), ("h", np.uint32),
                            ("x", np.int32), ("y", np.int32), ("whole", np.uint32)])


class ReaderError(RuntimeError):
    """read_header / read_packets refused: .code (ERR_UNSUPPORTED -2, ERR_INVALID -3, ...) and the reader's reason."""

    def __init__(self, what, code, reason):
        RuntimeError.__init__(self, "%s failed: %d (%s)" % (what, code, reason))
        self.code, self.reason = int(code), reason


class StageError(RuntimeError):
    """Context.stage_assemble refused or failed: .code (ERR_UNSUPPORTED -2, ERR_INVALID -3, ...) and the context's reason."""

    def __init__(self, what, code, reason):
        RuntimeError.__init__(self, "%s failed: %d (%s)" % (what, code, reason))
        self.code, self.reason = int(code), reason


class WriterError(RuntimeError):
    """a host writer call refused: .code (ERR_UNSUPPORTED -2, ERR_INVALID -3, -5 overflow) and grk_amd_writer_last_error's reason."""

    def __init__(self, what, code):
        L = lib()
        L.grk_amd_writer_last_error.restype = C.c_char_p
        L.grk_amd_writer_last_error.argtypes = []
        self.code, self.reason = int(code), L.grk_amd_writer_last_error().decode()
        RuntimeError.__init__(self, "%s failed: %d (%s)" % (what, code, self.reason))


_lib = None


def lib():
    global _lib
    if _lib is None:
        p = lib_path()
        if not os.path.exists(p):
            raise NativeLibraryMissing(
                "%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(there is no CPU fallback)" % p)
        L = C.CDLL(p)
        vp, u32, u64, i32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int
        PP = C.POINTER(TileParams)
        L.grk_amd_version.restype = C.c_char_p
        L.grk_amd_last_error.restype = C.c_char_p
        L.grk_amd_last_error.argtypes = [vp]
        L.grk_amd_create.argtypes = [i32, i32, C.POINTER(vp)]
        L.grk_amd_destroy.argtypes = [vp]
        L.grk_amd_destroy.restype = None
        L.grk_amd_set_stream.argtypes = [vp, vp]
        L.grk_amd_tile_num_blocks.restype = C.c_int64
        L.grk_amd_tile_num_blocks.argtypes = [PP]
        L.grk_amd_tile_layout.restype = C.c_int64
        L.grk_amd_tile_layout.argtypes = [PP, vp, u64, vp]
        L.grk_amd_tile_precincts.argtypes = [PP, vp]
        L.grk_amd_plane_stride.restype = u32
        L.grk_amd_plane_stride.argtypes = [PP]
        L.grk_amd_plane_elems.restype = u64
        L.grk_amd_plane_elems.argtypes = [PP]
        L.grk_amd_encode_tiles.argtypes = [vp, PP, u32, vp, i32, vp, C.POINTER(u64)]
        if hasattr(L, "grk_amd_set_pixel_layout"):            # (absent from older builds loaded through GRK_AMD_LIB for A/B timing)
            L.grk_amd_set_pixel_layout.argtypes = [vp, C.POINTER(PixelLayout)]
            L.grk_amd_set_decode_pixel_layout.argtypes = [vp, C.POINTER(PixelLayout)]
            L.grk_amd_pixel_bytes.restype = u64
            L.grk_amd_pixel_bytes.argtypes = [PP, C.POINTER(PixelLayout), u32, u32, u32]
        L.grk_amd_fetch_table.argtypes = [vp, vp, C.POINTER(u64)]
        L.grk_amd_fetch_coded.argtypes = [vp, vp, u64]
        L.grk_amd_coded_device_ptr.restype = vp
        L.grk_amd_coded_device_ptr.argtypes = [vp]
        L.grk_amd_table_device_ptr.restype = vp
        L.grk_amd_table_device_ptr.argtypes = [vp, i32]
        L.grk_amd_plane_device_ptr.restype = vp
        L.grk_amd_plane_device_ptr.argtypes = [vp, i32]
        L.grk_amd_synchronize.argtypes = [vp]
        L.grk_amd_stage_ingest_mct.argtypes = [vp, PP, u32, vp, vp]
        L.grk_amd_stage_dwt_fwd.argtypes = [vp, PP, u32, vp, vp]
        L.grk_amd_stage_ht_encode.argtypes = [vp, PP, u32, vp]
        L.grk_amd_stage_ht_encode16.argtypes = [vp, PP, u32, vp, u32]
        if hasattr(L, "grk_amd_encode_tiles_rate"):       # (absent from older builds loaded through GRK_AMD_LIB for A/B timing)
            L.grk_amd_stage_ht_encode_drops.argtypes = [vp, PP, u32, vp, i32, vp]
            L.grk_amd_encode_tiles_rate.argtypes = [vp, PP, u32, vp, i32, C.POINTER(Rate), vp, C.POINTER(u64), C.POINTER(RateResult)]
            L.grk_amd_encode_image_rate.restype = C.c_int64
            L.grk_amd_encode_image_rate.argtypes = [vp, C.POINTER(ImageLayout), PP, vp, u32, C.POINTER(Rate), vp, u64, C.POINTER(RateResult)]
            L.grk_amd_rate_tables.argtypes = [vp, i32, vp, u64]
        if hasattr(L, "grk_amd_encode_surface_rate"):
            L.grk_amd_encode_image_subsampled_rate.restype = C.c_int64
            L.grk_amd_encode_image_subsampled_rate.argtypes = [vp, C.POINTER(ImageLayout), PP, vp, vp, vp, u32, C.POINTER(Rate), vp, u64,
                                                               C.POINTER(RateResult)]
            L.grk_amd_encode_surface_rate.restype = C.c_int64
            L.grk_amd_encode_surface_rate.argtypes = [vp, C.POINTER(ImageLayout), PP, vp, vp, vp, vp, u64, i32, u32, C.POINTER(Rate), vp, u64,
                                                      C.POINTER(RateResult)]
            L.grk_amd_rate_num_blocks.restype = u64
            L.grk_amd_rate_num_blocks.argtypes = [vp]
            L.grk_amd_rate_unit_rows.argtypes = [vp, vp, u32]
            L.grk_amd_rate_last_budget.restype = u64
            L.grk_amd_rate_last_budget.argtypes = [vp]
        if hasattr(L, "grk_amd_encode_tiles_quality"):
            PQ, PQR, f64 = C.POINTER(Quality), C.POINTER(QualityResult), C.c_double
            L.grk_amd_encode_tiles_quality.argtypes = [vp, PP, u32, vp, i32, PQ, vp, C.POINTER(u64), PQR]
            L.grk_amd_encode_image_quality.restype = C.c_int64
            L.grk_amd_encode_image_quality.argtypes = [vp, C.POINTER(ImageLayout), PP, vp, u32, PQ, vp, u64, PQR]
            L.grk_amd_encode_image_subsampled_quality.restype = C.c_int64
            L.grk_amd_encode_image_subsampled_quality.argtypes = [vp, C.POINTER(ImageLayout), PP, vp, vp, vp, u32, PQ, vp, u64, PQR]
            L.grk_amd_encode_surface_quality.restype = C.c_int64
            L.grk_amd_encode_surface_quality.argtypes = [vp, C.POINTER(ImageLayout), PP, vp, vp, vp, vp, u64, i32, u32, PQ, vp, u64, PQR]
            L.grk_amd_encode_packed_quality.restype = C.c_int64
            L.grk_amd_encode_packed_quality.argtypes = [vp, C.POINTER(ImageLayout), PP, i32, u64, vp, u64, i32, u32, PQ, vp, u64, PQR]
            L.grk_amd_quality_last_budget.restype = f64
            L.grk_amd_quality_last_budget.argtypes = [vp]
            L.grk_amd_stage_quality_alloc.argtypes = [vp, vp, vp, vp, u64, u32, i32, f64, vp, vp]
        if hasattr(L, "grk_amd_rate_device_counters"):   # (absent from older builds loaded through GRK_AMD_LIB for A/B timing)
            # the rate- and quality-targeted calls that leave their file in device memory
            PQ, PQR = C.POINTER(Quality), C.POINTER(QualityResult)
            PV, PLy = C.POINTER(vp), C.POINTER(ImageLayout)
            for name, args in (("grk_amd_encode_surface_rate_device", [vp, PLy, PP, vp, vp, vp, vp, u64, i32, u32, C.POINTER(Rate), PV, C.POINTER(RateResult)]),
                               ("grk_amd_encode_surface_quality_device", [vp, PLy, PP, vp, vp, vp, vp, u64, i32, u32, PQ, PV, PQR]),
                               ("grk_amd_encode_packed_rate_device", [vp, PLy, PP, i32, u64, vp, u64, i32, u32, C.POINTER(Rate), PV, C.POINTER(RateResult)]),
                               ("grk_amd_encode_packed_quality_device", [vp, PLy, PP, i32, u64, vp, u64, i32, u32, PQ, PV, PQR]),
                               ("grk_amd_assemble_rate_device", [vp, PP, u32, vp, u32, u64, vp])):
                getattr(L, name).restype = C.c_int64
                getattr(L, name).argtypes = args
            L.grk_amd_rate_device_counters.restype = u64
            L.grk_amd_rate_device_counters.argtypes = [vp, i32]
        L.grk_amd_stage_dwt_inv.argtypes = [vp, PP, u32, vp, vp]
        L.grk_amd_stage_ht_decode.argtypes = [vp, PP, u32, vp, vp, u64, vp]
        L.grk_amd_stage_ht_decode16.argtypes = [vp, PP, u32, vp, vp, u64, vp]
        L.grk_amd_decode_tiles.argtypes = [vp, PP, u32, vp, vp, u64, i32, vp, i32]
        L.grk_amd_decode_status.argtypes = [vp]
        L.grk_amd_set_decode_qcd.argtypes = [vp, vp, u32]
        L.grk_amd_set_decode_segments.argtypes = [vp, vp, vp, u32]
        L.grk_amd_set_decode_steps.argtypes = [vp, vp, u32]
        L.grk_amd_decode_region.argtypes = [vp, PP, vp, vp, u64, i32, u32, u32, u32, u32, vp, i32]
        L.grk_amd_set_decode_reduce.argtypes = [vp, u32]
        L.grk_amd_reduced_tile_rect.argtypes = [PP] + [u32] + [C.POINTER(u32)] * 4
        L.grk_amd_set_overlap.argtypes = [vp, i32]
        L.grk_amd_set_decode_planes16.argtypes = [vp, i32]
        if hasattr(L, "grk_amd_plane_sample_bytes"):      # (absent from older builds loaded through GRK_AMD_LIB for A/B timing)
            L.grk_amd_plane_sample_bytes.argtypes = [vp, PP, i32, C.POINTER(u32)]
        L.grk_amd_set_pipelining.argtypes = [vp, i32]
        if hasattr(L, "grk_amd_set_decode_pipelining"):
            L.grk_amd_set_decode_pipelining.argtypes = [vp, i32]
        L.grk_amd_stream_wait_results.argtypes = [vp, vp]
        if hasattr(L, "grk_amd_block_distortion"):
            L.grk_amd_block_distortion.argtypes = [vp, vp, u64]
        if hasattr(L, "grk_amd_set_pixel_hold"):
            L.grk_amd_set_pixel_hold.argtypes = [vp, i32]
            L.grk_amd_stream_wait_pixels.argtypes = [vp, vp]
        if hasattr(L, "grk_amd_decode_stream_wait_slot"):
            L.grk_amd_decode_stream_wait_slot.argtypes = [vp, vp]
        L.grk_amd_stage_egress.argtypes = [vp, PP, u32, vp, vp]
        L.grk_amd_enable_timing.argtypes = [vp, i32]
        L.grk_amd_kernel_ms.restype = C.c_double
        L.grk_amd_kernel_ms.argtypes = [vp, i32, C.POINTER(u32)]
        L.grk_amd_write_codestream.restype = C.c_int64
        L.grk_amd_write_codestream.argtypes = [PP, u32, u32, vp, vp, vp, u64]
        L.grk_amd_write_codestream_ex.restype = C.c_int64
        L.grk_amd_write_codestream_ex.argtypes = [PP, u32, u32, vp, vp, u32, vp, u64]
        L.grk_amd_write_main_header.restype = C.c_int64
        L.grk_amd_write_main_header.argtypes = [PP, u32, u32, u32, vp, vp, u64]
        L.grk_amd_write_tile_part.restype = C.c_int64
        L.grk_amd_write_tile_part.argtypes = [PP, u32, u32, vp, vp, vp, u64]
        if hasattr(L, "grk_amd_node_create"):
            L.grk_amd_host_alloc.restype = vp
            L.grk_amd_host_alloc.argtypes = [vp, u64]
            L.grk_amd_host_free.argtypes = [vp, vp]
            L.grk_amd_node_create.argtypes = [vp, u32, i32, C.POINTER(vp)]
            L.grk_amd_node_destroy.argtypes = [vp]
            L.grk_amd_node_size.restype = u32
            L.grk_amd_node_size.argtypes = [vp]
            L.grk_amd_node_ctx.restype = vp
            L.grk_amd_node_ctx.argtypes = [vp, u32]
            L.grk_amd_node_last_error.restype = C.c_char_p
            L.grk_amd_node_last_error.argtypes = [vp]
            L.grk_amd_node_encode_image.restype = C.c_int64
            L.grk_amd_node_encode_image.argtypes = [vp, C.POINTER(ImageLayout), PP, vp, u32, vp, u64]
        L.grk_amd_locate_tile_parts.restype = C.c_int64
        L.grk_amd_locate_tile_parts.argtypes = [vp, u64, vp, vp, vp, u64, C.POINTER(i32)]
        PL = C.POINTER(ImageLayout)
        L.grk_amd_layout_num_tiles.restype = C.c_int64
        L.grk_amd_layout_num_tiles.argtypes = [PL]
        L.grk_amd_layout_tile.argtypes = [PL, PP, u32, PP]
        L.grk_amd_same_tile_geometry.argtypes = [PP, PP]
        L.grk_amd_same_tile_packets.argtypes = [PP, PP, u32]
        L.grk_amd_write_codestream_layout.restype = C.c_int64
        L.grk_amd_write_codestream_layout.argtypes = [PL, PP, vp, vp, u32, vp, u64]
        L.grk_amd_write_main_header_layout.restype = C.c_int64
        L.grk_amd_write_main_header_layout.argtypes = [PL, PP, u32, vp, vp, u64]
        L.grk_amd_encode_image.restype = C.c_int64
        L.grk_amd_encode_image.argtypes = [vp, PL, PP, vp, u32, vp, u64]
        if hasattr(L, "grk_amd_read_header"):
            L.grk_amd_read_header.argtypes = [vp, u64, C.POINTER(StreamInfo)]
            L.grk_amd_read_packets.restype = C.c_int64
            L.grk_amd_read_packets.argtypes = [vp, u64, C.POINTER(StreamInfo), u32, vp, u64, vp, vp, u64, C.POINTER(u64), vp, u64,
                                               C.POINTER(u64), C.POINTER(u64)]
            L.grk_amd_read_packets_parts.restype = C.c_int64
            L.grk_amd_read_packets_parts.argtypes = L.grk_amd_read_packets.argtypes
            if hasattr(L, "grk_amd_read_packets_refine"):          # (GRK_AMD_LIB may name a build from before it)
                L.grk_amd_read_packets_refine.restype = C.c_int64
                L.grk_amd_read_packets_refine.argtypes = L.grk_amd_read_packets.argtypes
            L.grk_amd_reader_last_error.restype = C.c_char_p
            L.grk_amd_decode_image.argtypes = [vp, vp, u64, vp, u64, i32]
            L.grk_amd_decode_image_launches.restype = u64
            L.grk_amd_decode_image_launches.argtypes = [vp, i32]
            L.grk_amd_gather_device.argtypes = [vp, vp, u64, vp, u64, vp, u64]
            L.grk_amd_place_tiles_device.argtypes = [vp, vp, u32, u32, u32, u32, u32, vp, vp, u32, u32]
        if hasattr(L, "grk_amd_set_decode_upsample"):
            L.grk_amd_set_decode_upsample.argtypes = [vp, i32]
            L.grk_amd_stream_comp_size.argtypes = [C.POINTER(StreamInfo), u32, C.POINTER(u32), C.POINTER(u32)]
            L.grk_amd_place_upsampled_device.argtypes = [vp, vp, u32, u32, u32, u32, u32, vp, u32, u32, vp, u32, u32, u32, u32]
        if hasattr(L, "grk_amd_decode_image_view"):
            PV = C.POINTER(ImageView)
            L.grk_amd_image_view_size.argtypes = [C.POINTER(StreamInfo), PV, u32, C.POINTER(u32), C.POINTER(u32)]
            L.grk_amd_plan_image_view.restype = C.c_int64
            L.grk_amd_plan_image_view.argtypes = [C.POINTER(StreamInfo), PV, vp, u64, C.POINTER(u64), vp, u64]
            L.grk_amd_decode_image_view.argtypes = [vp, vp, u64, PV, vp, u64, i32]
            L.grk_amd_decode_image_counters.restype = u64
            L.grk_amd_decode_image_counters.argtypes = [vp, i32]
            L.grk_amd_place_tiles_clipped_device.argtypes = [vp, vp, u32, u32, u32, u32, u32, u32, vp, vp, u32, u32]
        if hasattr(L, "grk_amd_encode_surface"):
            PS, pu8 = C.POINTER(Surface), C.POINTER(C.c_uint8)
            L.grk_amd_surface_bytes.restype = u64
            L.grk_amd_surface_bytes.argtypes = [PL, PP, pu8, pu8, PS, C.POINTER(C.c_char_p)]
            L.grk_amd_surface_format.argtypes = [i32, PL, u32, u64, PS, pu8, pu8, C.POINTER(u32), C.POINTER(u64)]
            L.grk_amd_surface_plan.argtypes = [PL, PP, pu8, pu8, PS, u64, u32, i32, i32, pu8, C.POINTER(PixelLayout), C.POINTER(u64), u32,
                                               C.POINTER(C.c_char_p)]
            L.grk_amd_encode_surface.restype = C.c_int64
            L.grk_amd_encode_surface.argtypes = [vp, PL, PP, pu8, pu8, PS, vp, u64, i32, u32, vp, u64]
            L.grk_amd_decode_surface.argtypes = [vp, vp, u64, PS, vp, u64, i32]
            L.grk_amd_surface_counters.restype = u64
            L.grk_amd_surface_counters.argtypes = [vp, i32]
            L.grk_amd_surface_cut_device.argtypes = [vp, vp, u64, C.POINTER(SurfaceComp), u32, u32, u32, u32, u32, vp, vp]
            L.grk_amd_surface_place_device.argtypes = [vp, vp, u32, u32, u32, u32, u32, vp, C.POINTER(SurfaceComp), vp, u64]
        if hasattr(L, "grk_amd_encode_packed"):
            L.grk_amd_packed_bytes.restype = u64
            L.grk_amd_packed_bytes.argtypes = [i32, PL, u32, C.POINTER(u64), C.POINTER(C.c_char_p)]
            L.grk_amd_encode_packed.restype = C.c_int64
            L.grk_amd_encode_packed.argtypes = [vp, PL, PP, i32, u64, vp, u64, i32, u32, vp, u64]
            L.grk_amd_encode_packed_rate.restype = C.c_int64
            L.grk_amd_encode_packed_rate.argtypes = [vp, PL, PP, i32, u64, vp, u64, i32, u32, C.POINTER(Rate), vp, u64, C.POINTER(RateResult)]
            L.grk_amd_decode_packed.argtypes = [vp, vp, u64, i32, u64, vp, u64, i32]
            L.grk_amd_packed_unpack_device.argtypes = [vp, i32, u32, u32, u32, vp, u64, u64, vp, u64]
            L.grk_amd_packed_pack_device.argtypes = [vp, i32, u32, u32, u32, vp, u64, vp, u64, u64]
            L.grk_amd_packed_counters.restype = u64
            L.grk_amd_packed_counters.argtypes = [vp, i32]
        if hasattr(L, "grk_amd_encode_route_counters"):
            L.grk_amd_encode_surface_device.restype = C.c_int64
            L.grk_amd_encode_surface_device.argtypes = [vp, PL, PP, pu8, pu8, PS, vp, u64, i32, u32, C.POINTER(vp)]
            L.grk_amd_encode_packed_device.restype = C.c_int64
            L.grk_amd_encode_packed_device.argtypes = [vp, PL, PP, i32, u64, vp, u64, i32, u32, C.POINTER(vp)]
            L.grk_amd_encode_route_counters.restype = u64
            L.grk_amd_encode_route_counters.argtypes = [vp, i32]
        _lib = L
    return _lib


def tile_layout(params):
    """Host-only geometry: (list of Block, qcd words)."""
    L = lib()
    n = L.grk_amd_tile_num_blocks(C.byref(params))
    if n < 0:
        raise ValueError("grk_amd_tile_num_blocks failed: %d" % n)
    blocks = (Block * n)()
    qcd = (C.c_uint16 * (3 * MAX_LEVELS + 1))()
    rc = L.grk_amd_tile_layout(C.byref(params), blocks, n, qcd)
    if rc < 0:
        raise ValueError("grk_amd_tile_layout failed: %d" % rc)
    return list(blocks), list(qcd)[:3 * params.num_levels + 1]


def pixel_bytes(params, layout=None, w=0, h=0, ntiles=1):
    """Bytes `ntiles` tiles of w x h (0: the tile's size) span in `layout` (None: the default); 0 for a layout that is invalid for
    these parameters (grk_amd_pixel_bytes)."""
    return int(lib().grk_amd_pixel_bytes(C.byref(params), C.byref(layout) if layout is not None else None, int(w), int(h), int(ntiles)))


def reduced_tile_rect(params, reduce):
    """(x0, y0, w, h) of the tile at 1 / 2^reduce of its size, on the reduced grid (grk_amd_reduced_tile_rect)."""
    v = [C.c_uint32(0) for _ in range(4)]
    rc = lib().grk_amd_reduced_tile_rect(C.byref(params), int(reduce), *[C.byref(x) for x in v])
    if rc != 0:
        raise ValueError("grk_amd_reduced_tile_rect(reduce=%d) failed: %d" % (reduce, rc))
    return tuple(x.value for x in v)


CS_TLM, CS_PLT, CS_SOP, CS_EPH = 1, 2, 4, 8
CS_BLOCK_MSBS = 16           # the zero-bit-plane tag trees from the rows' own missing_msbs (the host writers only)
DROP_SKIP = 0xFF             # a block's drop byte: not coded (grk_amd_stage_ht_encode_drops, rate_tables(3))
STAGE_HT_ROOM = 1            # grk_amd_stage_ht_encode16 flags


TP_R, TP_L, TP_C = 1, 2, 3   # the division letters of CS_TP


def CS_TP(letter):
    """tiles divided into tile-parts at this letter of the progression order (TP_R / TP_L / TP_C, grk_compress -u); 0: not divided"""
    return int(letter) << 12


def CS_PROG(order):
    """progression order for the writer's flags: 0 LRCP, 1 RLCP, 2 RPCL, 3 PCRL, 4 CPRL"""
    return int(order) << 8


def write_codestream(params, img_w, img_h, table, coded, flags=0):
    """table: ctypes array / numpy structured array of CodedBlock rows; coded: bytes-like; flags: CS_TLM | CS_PLT."""
    L = lib()
    cbuf = np.frombuffer(coded, np.uint8) if not isinstance(coded, np.ndarray) else coded
    cap = int(cbuf.size) + len(table) * 8 + (1 << 20)
    out = np.empty(cap, np.uint8)
    tptr = table.ctypes.data if isinstance(table, np.ndarray) else C.addressof(table)
    n = L.grk_amd_write_codestream_ex(C.byref(params), img_w, img_h, tptr, cbuf.ctypes.data, flags, out.ctypes.data, cap)
    if n < 0:
        raise RuntimeError("grk_amd_write_codestream failed: %d" % n)
    return out[:n].tobytes()


def layout_tiles(layout, base):
    """The parameters of every tile of the layout (raster order): base with the tile's size and origin."""
    L = lib()
    n = L.grk_amd_layout_num_tiles(C.byref(layout))
    if n < 0:
        raise ValueError("grk_amd_layout_num_tiles failed: %d" % n)
    out = []
    for t in range(n):
        p = TileParams()
        rc = L.grk_amd_layout_tile(C.byref(layout), C.byref(base), t, C.byref(p))
        if rc:
            raise ValueError("grk_amd_layout_tile failed: %d" % rc)
        out.append(p)
    return out


def same_tile_geometry(a, b):
    rc = lib().grk_amd_same_tile_geometry(C.byref(a), C.byref(b))
    if rc < 0:
        raise ValueError("grk_amd_same_tile_geometry failed: %d" % rc)
    return bool(rc)


def same_tile_packets(a, b, flags=0):
    """May tiles a and b share one assemble_device call under the progression order of `flags` (CS_PROG)?  Same component count, same
    geometry and the same packet sequence (grk_amd_same_tile_packets)."""
    rc = lib().grk_amd_same_tile_packets(C.byref(a), C.byref(b), int(flags))
    if rc < 0:
        raise ValueError("grk_amd_same_tile_packets failed: %d" % rc)
    return bool(rc)


def write_codestream_layout(layout, base, table, coded, flags=0):
    """table: the tiles' rows one tile after the other (every tile with the rows of ITS geometry, layout_tiles())."""
    L = lib()
    cbuf = np.frombuffer(coded, np.uint8) if not isinstance(coded, np.ndarray) else coded
    cap = int(cbuf.size) + len(table) * 8 + (1 << 20)
    out = np.empty(cap, np.uint8)
    t = np.ascontiguousarray(table)
    n = L.grk_amd_write_codestream_layout(C.byref(layout), C.byref(base), t.ctypes.data, cbuf.ctypes.data, flags, out.ctypes.data, cap)
    if n < 0:
        raise WriterError("grk_amd_write_codestream_layout", n)
    return out[:n].tobytes()


def t2_max_block_bytes():
    """grk_amd_t2_max_block_bytes: the longest code-block Tier-2 on the device takes"""
    L = lib()
    L.grk_amd_t2_max_block_bytes.restype = C.c_uint32
    L.grk_amd_t2_max_block_bytes.argtypes = []
    return int(L.grk_amd_t2_max_block_bytes())


def t2_max_block_msbs():
    """grk_amd_t2_max_block_msbs: the most zero bit-planes of a code-block the device writer's general tag tree takes"""
    L = lib()
    L.grk_amd_t2_max_block_msbs.restype = C.c_uint32
    L.grk_amd_t2_max_block_msbs.argtypes = []
    return int(L.grk_amd_t2_max_block_msbs())


def write_tile_part(params, tile_index, tile_table, coded, flags=0, size_only=False):
    """One tile-part (SOT [PLT] SOD packets) as bytes, or only its length (no coded bytes needed)."""
    L = lib()
    t = np.ascontiguousarray(tile_table)
    if size_only:
        n = L.grk_amd_write_tile_part(C.byref(params), tile_index, flags, t.ctypes.data, None, None, 0)
        if n < 0:
            raise RuntimeError("grk_amd_write_tile_part failed: %d" % n)
        return int(n)
    cbuf = np.frombuffer(coded, np.uint8) if not isinstance(coded, np.ndarray) else coded
    cap = int(t["length"].sum()) + len(t) * 8 + 4096
    out = np.empty(cap, np.uint8)
    n = L.grk_amd_write_tile_part(C.byref(params), tile_index, flags, t.ctypes.data, cbuf.ctypes.data, out.ctypes.data, cap)
    if n < 0:
        raise RuntimeError("grk_amd_write_tile_part failed: %d" % n)
    return out[:n].tobytes()


def write_main_header(params, img_w, img_h, flags=0, tile_part_bytes=None):
    L = lib()
    out = np.empty(4096 + (5 * len(tile_part_bytes) if tile_part_bytes is not None else 0), np.uint8)
    tp = np.ascontiguousarray(tile_part_bytes, np.uint32) if tile_part_bytes is not None else None
    n = L.grk_amd_write_main_header(C.byref(params), img_w, img_h, flags, tp.ctypes.data if tp is not None else None,
                                    out.ctypes.data, out.size)
    if n < 0:
        raise RuntimeError("grk_amd_write_main_header failed: %d" % n)
    return out[:n].tobytes()


def _u8s(values):
    return (C.c_uint8 * len(values))(*[int(v) for v in values]) if values is not None else None


def tile_part_starts(tile, flags, sampling=None):
    """grk_amd_tile_part_starts: (the first packet number of every tile-part of `tile` under flags' order and division, the tile's
    packets).  tile: the tile on the reference grid (layout_tiles); sampling: [(dx, dy)] per component or None.  WriterError."""
    L = lib()
    L.grk_amd_tile_part_starts.restype = C.c_int64
    L.grk_amd_tile_part_starts.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]
    dx = _u8s([a for a, _ in sampling]) if sampling else None
    dy = _u8s([b for _, b in sampling]) if sampling else None
    starts = np.zeros(256, np.uint32)
    npk = C.c_uint32(0)
    n = L.grk_amd_tile_part_starts(C.addressof(tile), dx, dy, int(flags), starts.ctypes.data, starts.size, C.byref(npk))
    if n < 0:
        raise WriterError("grk_amd_tile_part_starts", n)
    return [int(v) for v in starts[:n]], int(npk.value)


def write_tile_parts(params, tile_index, tile_table, coded, flags=0, starts=None, size_only=False, cap=None):
    """A tile divided into tile-parts (grk_amd_write_tile_parts) at the packets `starts`, or with starts None under the division of
    `flags` -> (the parts' bytes one behind the other, [their lengths]); size_only: (the length, [lengths]).  WriterError."""
    L = lib()
    L.grk_amd_write_tile_parts.restype = C.c_int64
    L.grk_amd_write_tile_parts.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p]
    t = np.ascontiguousarray(tile_table)
    s = np.ascontiguousarray(starts, np.uint32) if starts is not None else None
    lens = np.zeros(max(256, 0 if s is None else s.size), np.uint32)
    args = (C.addressof(params), tile_index, int(flags), t.ctypes.data)
    div = (s.ctypes.data if s is not None else None, s.size if s is not None else 0)
    if size_only:
        n = L.grk_amd_write_tile_parts(*args, None, *div, None, 0, lens.ctypes.data if s is None or s.size <= 255 else None)
        if n < 0:
            raise WriterError("grk_amd_write_tile_parts", n)
        return int(n), lens
    cbuf = np.frombuffer(coded, np.uint8) if not isinstance(coded, np.ndarray) else coded
    if cap is None:
        cap = int(t["length"].sum()) + len(t) * 8 + 4096 + 32 * 256
    out = np.empty(cap + 64, np.uint8)
    out[cap:] = 0xA5                                         # (a guard the call must not touch)
    n = L.grk_amd_write_tile_parts(*args, cbuf.ctypes.data, *div, out.ctypes.data, cap, lens.ctypes.data if s is None or s.size <= 255 else None)
    assert (out[cap:] == 0xA5).all(), "grk_amd_write_tile_parts wrote beyond cap"
    if n < 0:
        raise WriterError("grk_amd_write_tile_parts", n)
    k = s.size if s is not None else int(np.count_nonzero(lens))
    return out[:n].tobytes(), [int(v) for v in lens[:k]]


def write_main_header_parts(layout, base, flags, parts_per_tile, part_bytes):
    """grk_amd_write_main_header_parts: the main header of a file of divided tiles; TLM (CS_TLM) lists part_bytes in file order"""
    L = lib()
    L.grk_amd_write_main_header_parts.restype = C.c_int64
    L.grk_amd_write_main_header_parts.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
    ppt = np.ascontiguousarray(parts_per_tile, np.uint32)
    pb = np.ascontiguousarray(part_bytes, np.uint32)
    out = np.empty(4096 + 5 * pb.size, np.uint8)
    n = L.grk_amd_write_main_header_parts(C.addressof(layout), C.addressof(base), int(flags), ppt.ctypes.data, pb.ctypes.data, out.ctypes.data, out.size)
    if n < 0:
        raise WriterError("grk_amd_write_main_header_parts", n)
    return out[:n].tobytes()


def locate_tile_parts(cs):
    """-> ([(offset, length, tile index)], used_tlm)"""
    L = lib()
    buf = np.frombuffer(cs, np.uint8)
    n = L.grk_amd_locate_tile_parts(buf.ctypes.data, buf.size, None, None, None, 0, None)
    if n < 0:
        raise RuntimeError("grk_amd_locate_tile_parts failed: %d" % n)
    off = np.zeros(n, np.uint64); ln = np.zeros(n, np.uint32); ti = np.zeros(n, np.uint16)
    used = C.c_int(0)
    L.grk_amd_locate_tile_parts(buf.ctypes.data, buf.size, off.ctypes.data, ln.ctypes.data, ti.ctypes.data, n, C.byref(used))
    return [(int(a), int(b), int(c)) for a, b, c in zip(off, ln, ti)], bool(used.value)


CODED_DTYPE = np.dtype([("offset", np.uint64), ("length", np.uint32), ("missing_msbs", np.uint32)])
SEGMENT_DTYPE = np.dtype([("length", np.uint32), ("numpasses", np.uint32)])
MOVE_DTYPE = np.dtype([("dst", np.uint64), ("src", np.uint64), ("len", np.uint32), ("kind", np.uint32)])
ERR_UNSUPPORTED, ERR_INVALID, ERR_OVERFLOW, ERR_RANGE = -2, -3, -5, -6
READ_DEVICE_FIRST_COPY = 4096          # GRK_AMD_READ_DEVICE_FIRST_COPY: the first copy grk_amd_read_header_device makes of a main header


def _cs_array(cs):
    return cs if isinstance(cs, np.ndarray) else np.frombuffer(cs, np.uint8)


def read_header(cs):
    """grk_amd_read_header: the main header of a codestream (bytes-like) -> StreamInfo; ReaderError when it is refused."""
    L = lib()
    buf = _cs_array(cs)
    info = StreamInfo()
    rc = L.grk_amd_read_header(buf.ctypes.data if buf.size else None, buf.size, C.byref(info))
    if rc:
        raise ReaderError("read_header", rc, L.grk_amd_reader_last_error().decode())
    return info


def stream_comp_sizes(info):
    """[(w, h)] of every component of the image in its own samples (grk_amd_stream_comp_size)"""
    L = lib()
    out = []
    for k in range(info.base.num_comps):
        w, h = C.c_uint32(0), C.c_uint32(0)
        rc = L.grk_amd_stream_comp_size(C.byref(info), k, C.byref(w), C.byref(h))
        if rc:
            raise ValueError("grk_amd_stream_comp_size failed: %d" % rc)
        out.append((w.value, h.value))
    return out


def _view_error(what, rc):
    kind = {ERR_UNSUPPORTED: "unsupported", ERR_INVALID: "invalid", ERR_OVERFLOW: "overflow"}.get(rc, "error")
    return ValueError("%s refused the view: %s (%d)" % (what, kind, rc))


def image_view_size(info, reduce=0, window=None):
    """[(w, h)] of every component of the view (grk_amd_image_view_size): the planes decode_image_view writes.  ValueError, naming
    the code (unsupported / invalid), for a view the call refuses."""
    L = lib()
    view = ImageView.make(reduce, window)
    out = []
    for k in range(info.base.num_comps):
        w, h = C.c_uint32(0), C.c_uint32(0)
        rc = L.grk_amd_image_view_size(C.byref(info), C.byref(view), k, C.byref(w), C.byref(h))
        if rc:
            raise _view_error("image_view_size", rc)
        out.append((w.value, h.value))
    return out


def plan_image_view(info, reduce=0, window=None):
    """grk_amd_plan_image_view -> dict(tiles: the touched tiles in index order (uint32), units: VIEW_UNIT_DTYPE rows, per touched tile
    and run of components its (reduced) size w x h, its signed position x, y in the view and whether the view holds it wholly)"""
    L = lib()
    view = ImageView.make(reduce, window)
    nt = C.c_uint64(0)
    n = L.grk_amd_plan_image_view(C.byref(info), C.byref(view), None, 0, C.byref(nt), None, 0)
    if n < 0:
        raise _view_error("plan_image_view", int(n))
    tiles = np.zeros(nt.value, np.uint32)
    units = np.zeros(n, VIEW_UNIT_DTYPE)
    n = L.grk_amd_plan_image_view(C.byref(info), C.byref(view), tiles.ctypes.data, tiles.size, C.byref(nt), units.ctypes.data, units.size)
    if n < 0:
        raise _view_error("plan_image_view", int(n))
    return dict(tiles=tiles, units=units)


def read_packets(cs, info=None, threads=1, _call="grk_amd_read_packets"):
    """grk_amd_read_packets: every packet header of every tile -> dict(rows CODED_DTYPE, first_segment uint32 [rows + 1],
    segments SEGMENT_DTYPE, moves MOVE_DTYPE, appendix_bytes).  A row's offset points into `cs`, or -- at or behind len(cs) --
    into the appendix that `moves` fill."""
    L = lib()
    call = getattr(L, _call)
    buf = _cs_array(cs)
    if info is None:
        info = read_header(buf)
    nseg, nmov, app = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    # sized for what a single-layer stream without split codeword segments needs: one parse; anything else says how much
    # it needs (ERR_OVERFLOW with the sizes set) and is parsed again
    nrows, seg_cap, move_cap = int(info.num_blocks), int(info.num_blocks), 0
    while True:
        rows = np.zeros(nrows, CODED_DTYPE)
        first = np.zeros(nrows + 1, np.uint32)
        segs = np.zeros(seg_cap, SEGMENT_DTYPE)
        moves = np.zeros(move_cap, MOVE_DTYPE)
        n = call(buf.ctypes.data, buf.size, C.byref(info), threads, rows.ctypes.data, rows.size, first.ctypes.data,
                 segs.ctypes.data, segs.size, C.byref(nseg), moves.ctypes.data, moves.size, C.byref(nmov), C.byref(app))
        if n == ERR_OVERFLOW and (nseg.value > seg_cap or nmov.value > move_cap):
            seg_cap, move_cap = max(seg_cap, int(nseg.value)), max(move_cap, int(nmov.value))
            continue
        if n < 0:
            raise ReaderError(_call[len("grk_amd_"):], n, L.grk_amd_reader_last_error().decode())
        break
    segs, moves = segs[:nseg.value], moves[:nmov.value]
    return dict(rows=rows, first_segment=first, segments=segs, moves=moves, appendix_bytes=int(app.value))


def read_packets_parts(cs, info=None, threads=1):
    """grk_amd_read_packets_parts: read_packets for a codestream whose tiles may be divided into tile-parts (1..255 per tile); the
    same dict, every offset and every move's src a position in `cs`."""
    return read_packets(cs, info, threads, "grk_amd_read_packets_parts")


def read_packets_refine(cs, info=None, threads=1):
    """grk_amd_read_packets_refine: read_packets_parts for an HTJ2K codestream whose code-blocks carry SigProp / MagRef passes; the
    same dict, an HT block's segments {Lcup, 1} alone or {Lcup, 1}, {Lref, 1 | 2}."""
    return read_packets(cs, info, threads, "grk_amd_read_packets_refine")


class Context:
    """One GPU context (grk_amd_ctx)."""

    def __init__(self, device=0, verbose=False):
        self._L = lib()
        h = C.c_void_p()
        rc = self._L.grk_amd_create(device, int(verbose), C.byref(h))
        if rc != 0:
            raise RuntimeError("grk_amd_create(device=%d) failed: %d (no usable HIP device?)" % (device, rc))
        self._h = h
        self._reduce = 0
        self._layout = None
        self._dec_layout = None

    def close(self):
        if self._h:
            self._L.grk_amd_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            raise RuntimeError("%s failed: %d (%s)" % (what, rc, self._L.grk_amd_last_error(self._h).decode()))

    def last_error(self):
        """grk_amd_last_error: why the latest failing call failed -- or the note a successful rate-targeted call left"""
        return self._L.grk_amd_last_error(self._h).decode()

    def set_stream(self, stream_ptr):
        self._check(self._L.grk_amd_set_stream(self._h, stream_ptr), "set_stream")

    def synchronize(self):
        self._check(self._L.grk_amd_synchronize(self._h), "synchronize")

    def set_pixel_layout(self, layout):
        """The layout of the pixels every later encode reads (grk_amd_set_pixel_layout); None: the default."""
        self._check(self._L.grk_amd_set_pixel_layout(self._h, C.byref(layout) if layout is not None else None), "set_pixel_layout")
        self._layout = layout

    def set_decode_pixel_layout(self, layout):
        """The layout of the pixels every later decode writes (grk_amd_set_decode_pixel_layout); None: the default."""
        self._check(self._L.grk_amd_set_decode_pixel_layout(self._h, C.byref(layout) if layout is not None else None), "set_decode_pixel_layout")
        self._dec_layout = layout

    def _out_in_layout(self, params, layout, w, h, ntiles, out):
        """the destination of a host decode in `layout`: the caller's uint8 array (gaps are left as they are) or zeros of the extent"""
        n = pixel_bytes(params, layout, w, h, ntiles)
        if n == 0:
            raise ValueError("the layout is invalid for these parameters")
        if out is None:
            out = np.zeros(n, np.uint8)
        if out.dtype != np.uint8 or not out.flags.c_contiguous or out.size < n:
            raise ValueError("out: a contiguous uint8 array of at least %d bytes" % n)
        return out

    def _with_decode_layout(self, layout, call):
        keep = self._dec_layout
        self.set_decode_pixel_layout(layout)
        try:
            return call()
        finally:
            self.set_decode_pixel_layout(keep)

    def encode_tiles(self, params, ntiles, pixels_ptr, on_device, fetch=True):
        """Runs the hot path. Returns (table ndarray, total_bytes) when fetch else None."""
        if fetch:
            n = self._L.grk_amd_tile_num_blocks(C.byref(params)) * ntiles
            table = np.zeros(n, CODED_DTYPE)
            tot = C.c_uint64(0)
            self._check(self._L.grk_amd_encode_tiles(self._h, C.byref(params), ntiles, pixels_ptr, int(on_device),
                                                     table.ctypes.data, C.byref(tot)), "encode_tiles")
            return table, tot.value
        self._check(self._L.grk_amd_encode_tiles(self._h, C.byref(params), ntiles, pixels_ptr, int(on_device),
                                                 None, None), "encode_tiles")
        return None

    def encode_host(self, params, pixels, ntiles=1, layout=None):
        """pixels: numpy array holding the tiles back to back (host memory) -- in `layout` (for this call) if one is given, else in
        the context's."""
        px = np.ascontiguousarray(pixels)
        if layout is None:
            table, tot = self.encode_tiles(params, ntiles, px.ctypes.data, False)
        else:
            if px.nbytes < pixel_bytes(params, layout, 0, 0, ntiles):
                raise ValueError("the array is smaller than %d tiles in this layout" % ntiles)
            keep = self._layout
            self.set_pixel_layout(layout)
            try:
                table, tot = self.encode_tiles(params, ntiles, px.ctypes.data, False)
            finally:
                self.set_pixel_layout(keep)
        coded = np.empty(tot, np.uint8)
        if tot:
            self._check(self._L.grk_amd_fetch_coded(self._h, coded.ctypes.data, tot), "fetch_coded")
        return table, coded

    def host_array(self, nbytes):
        """A uint8 numpy array over pinned host memory (grk_amd_host_alloc): crosses the link in one DMA.  Freed with the
        array (keep a reference while the context uses it)."""
        p = self._L.grk_amd_host_alloc(self._h, int(nbytes))
        if not p:
            raise MemoryError("grk_amd_host_alloc(%d) failed" % nbytes)
        buf = (C.c_uint8 * int(nbytes)).from_address(p)
        arr = np.frombuffer(buf, np.uint8)
        L = self._L
        import weakref
        weakref.finalize(buf, lambda: L.grk_amd_host_free(None, C.c_void_p(p)))     # (no context needed: it may be gone by then)
        return arr

    def encode_image(self, layout, base, pixels, flags=0):
        """Whole image of any tile layout -> codestream bytes (grk_amd_encode_image): (C, H, W), or the image as the context's pixel
        layout says (set_pixel_layout: (H, W, C) with row_pitch the image's)."""
        px = np.ascontiguousarray(pixels)
        cap = px.size * 4 + (1 << 20)
        out = np.empty(cap, np.uint8)
        n = self._L.grk_amd_encode_image(self._h, C.byref(layout), C.byref(base), px.ctypes.data, flags, out.ctypes.data, cap)
        if n < 0:
            raise RuntimeError("encode_image failed: %d (%s)" % (n, self._L.grk_amd_last_error(self._h).decode()))
        return out[:n].tobytes()

    def encode_image_subsampled(self, layout, base, sampling, planes, flags=0):
        """Image with sub-sampled components -> codestream bytes (grk_amd_encode_image_subsampled).  sampling: [(dx, dy)] per
        component; planes: one 2-D array per component, component c of ceil(x1 / dx) - ceil(x0 / dx) columns."""
        dx = (C.c_uint8 * len(sampling))(*[int(a) for a, _ in sampling])
        dy = (C.c_uint8 * len(sampling))(*[int(b) for _, b in sampling])
        px = np.concatenate([np.ascontiguousarray(pl).reshape(-1) for pl in planes])
        cap = px.size * px.itemsize * 4 + (1 << 20)
        out = np.empty(cap, np.uint8)
        self._L.grk_amd_encode_image_subsampled.restype = C.c_int64
        self._L.grk_amd_encode_image_subsampled.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                            C.c_uint32, C.c_void_p, C.c_uint64]
        n = self._L.grk_amd_encode_image_subsampled(self._h, C.addressof(layout), C.addressof(base), C.addressof(dx), C.addressof(dy),
                                                    px.ctypes.data, flags, out.ctypes.data, cap)
        if n < 0:
            raise RuntimeError("encode_image_subsampled failed: %d (%s)" % (n, self._L.grk_amd_last_error(self._h).decode()))
        return out[:n].tobytes()

    def _surface_fail(self, what, rc):
        raise SurfaceError(what, rc, self._L.grk_amd_last_error(self._h).decode())

    def encode_surface(self, layout, base, sampling, surface, pixels, flags=0, cap=None):
        """A video surface -> codestream bytes (grk_amd_encode_surface).  pixels: a uint8 numpy array holding the surface (host), or a
        device pointer (int) together with `cap`, the bytes behind it."""
        dx, dy = _sampling(sampling)
        on_device = not isinstance(pixels, np.ndarray)
        if on_device:
            ptr, nbytes = int(pixels), int(cap)
        else:
            if pixels.dtype != np.uint8 or not pixels.flags.c_contiguous:
                raise ValueError("pixels: a contiguous uint8 array")
            ptr, nbytes = pixels.ctypes.data, pixels.nbytes if cap is None else int(cap)
        out_cap = nbytes * 4 + (1 << 20)
        out = np.empty(out_cap, np.uint8)
        n = self._L.grk_amd_encode_surface(self._h, C.byref(layout), C.byref(base), dx, dy, C.byref(surface), ptr, nbytes, int(on_device),
                                           flags, out.ctypes.data, out_cap)
        if n < 0:
            self._surface_fail("encode_surface", n)
        return out[:n].tobytes()

    def encode_surface_device(self, layout, base, sampling, surface, pixels, flags=0, cap=None):
        """grk_amd_encode_surface_device: the file left in device memory -> (device pointer, length); the bytes belong to the context
        and stay valid until its next encode call.  pixels as encode_surface takes them."""
        dx, dy = _sampling(sampling)
        ptr, nbytes, on_device = self._frame_arg(pixels, cap)
        d_file = C.c_void_p(0)
        n = self._L.grk_amd_encode_surface_device(self._h, C.byref(layout), C.byref(base), dx, dy, C.byref(surface), ptr, nbytes, on_device,
                                                  flags, C.byref(d_file))
        if n < 0:
            self._surface_fail("encode_surface_device", n)
        return int(d_file.value), int(n)

    def encode_packed_device(self, layout, base, fmt, pixels, pitch=0, flags=0, cap=None):
        """grk_amd_encode_packed_device: encode_packed with the file left in device memory -> (device pointer, length)"""
        ptr, nbytes, on_device = self._frame_arg(pixels, cap)
        d_file = C.c_void_p(0)
        n = self._L.grk_amd_encode_packed_device(self._h, C.byref(layout), C.byref(base), PACKED_FORMATS.get(fmt, fmt), int(pitch), ptr, nbytes,
                                                 on_device, flags, C.byref(d_file))
        if n < 0:
            self._surface_fail("encode_packed_device", n)
        return int(d_file.value), int(n)

    def encode_route_counters(self):
        """(files whose tile-parts were assembled on the device, files written by the host writer) by this context's encode_image_subsampled,
        encode_surface, encode_packed and _device calls so far"""
        return tuple(int(self._L.grk_amd_encode_route_counters(self._h, k)) for k in range(2))

    def decode_surface(self, cs, surface, pixels, cap=None):
        """Codestream -> the components' samples on a surface (grk_amd_decode_surface); every other byte keeps its value.  pixels: a
        uint8 numpy array (host: written in place) or a device pointer (int) with `cap` (asynchronous: decode_status joins)."""
        buf = _cs_array(cs)
        on_device = not isinstance(pixels, np.ndarray)
        if on_device:
            ptr, nbytes = int(pixels), int(cap)
        else:
            if pixels.dtype != np.uint8 or not pixels.flags.c_contiguous:
                raise ValueError("pixels: a contiguous uint8 array")
            ptr, nbytes = pixels.ctypes.data, pixels.nbytes if cap is None else int(cap)
        rc = self._L.grk_amd_decode_surface(self._h, buf.ctypes.data, buf.size, C.byref(surface), ptr, nbytes, int(on_device))
        if rc:
            self._surface_fail("decode_surface", rc)

    def surface_counters(self):
        """(units handled in place, units staged, launches of the two surface kernels) by this context's surface calls so far"""
        return tuple(int(self._L.grk_amd_surface_counters(self._h, k)) for k in range(3))

    def surface_cut_device(self, d_surface, surface_bytes, comps, bps, nunits, w, h, origins, d_tiles):
        """KS alone: comps [(offset, row_pitch, step[, shift])], origins [(x, y)] of every unit's first sample in the components"""
        cs = (SurfaceComp * len(comps))(*[_surface_comp(cp) for cp in comps])
        r = np.ascontiguousarray(origins, np.uint32).reshape(-1)
        rc = self._L.grk_amd_surface_cut_device(self._h, d_surface, int(surface_bytes), cs, len(comps), bps, nunits, w, h, r.ctypes.data, d_tiles)
        if rc:
            self._surface_fail("surface_cut_device", rc)

    def surface_place_device(self, d_tiles, nunits, w, h, bps, origins, comps, d_surface, surface_bytes):
        """KD alone (the reverse)"""
        cs = (SurfaceComp * len(comps))(*[_surface_comp(cp) for cp in comps])
        r = np.ascontiguousarray(origins, np.uint32).reshape(-1)
        rc = self._L.grk_amd_surface_place_device(self._h, d_tiles, nunits, w, h, len(comps), bps, r.ctypes.data, cs, d_surface, int(surface_bytes))
        if rc:
            self._surface_fail("surface_place_device", rc)

    @staticmethod
    def _frame_arg(pixels, cap):
        """a frame or surface argument: a contiguous uint8 numpy array (host) or a device pointer (int) with `cap` -> (ptr, bytes, on_device)"""
        if not isinstance(pixels, np.ndarray):
            return int(pixels), int(cap), 1
        if pixels.dtype != np.uint8 or not pixels.flags.c_contiguous:
            raise ValueError("pixels: a contiguous uint8 array")
        return pixels.ctypes.data, pixels.nbytes if cap is None else int(cap), 0

    def encode_packed(self, layout, base, fmt, pixels, pitch=0, flags=0, cap=None):
        """A packed 4:2:2 frame (a name of PACKED_FORMATS or the format's number; pitch 0 = the format's default) -> codestream bytes
        (grk_amd_encode_packed).  pixels: a uint8 numpy array holding the frame (host), or a device pointer (int) together with `cap`"""
        ptr, nbytes, on_device = self._frame_arg(pixels, cap)
        out_cap = nbytes * 4 + (1 << 20)
        out = np.empty(out_cap, np.uint8)
        n = self._L.grk_amd_encode_packed(self._h, C.byref(layout), C.byref(base), PACKED_FORMATS.get(fmt, fmt), int(pitch), ptr, nbytes, on_device,
                                          flags, out.ctypes.data, out_cap)
        if n < 0:
            self._surface_fail("encode_packed", n)
        return out[:n].tobytes()

    def encode_packed_rate(self, layout, base, fmt, pixels, target_bytes, pitch=0, flags=0, cap=None, max_drop=0, allow_skip=False):
        """grk_amd_encode_packed_rate: encode_packed in a file of at most target_bytes -> (codestream bytes, RateResult)"""
        ptr, nbytes, on_device = self._frame_arg(pixels, cap)
        out_cap = nbytes * 4 + (1 << 20)
        out = np.empty(out_cap, np.uint8)
        rate, res = Rate(int(target_bytes), int(max_drop), int(bool(allow_skip)), 1), RateResult()
        n = self._L.grk_amd_encode_packed_rate(self._h, C.byref(layout), C.byref(base), PACKED_FORMATS.get(fmt, fmt), int(pitch), ptr, nbytes,
                                               on_device, flags, C.byref(rate), out.ctypes.data, out_cap, C.byref(res))
        if n < 0:
            raise RateError("encode_packed_rate", n, self._L.grk_amd_last_error(self._h).decode())
        return out[:n].tobytes(), res

    def decode_packed(self, cs, fmt, pixels, pitch=0, cap=None):
        """Codestream -> a packed 4:2:2 frame (grk_amd_decode_packed); what is no sample keeps its value.  pixels: a uint8 numpy array
        (host: written in place) or a device pointer (int) with `cap` (asynchronous: decode_status joins)."""
        buf = _cs_array(cs)
        ptr, nbytes, on_device = self._frame_arg(pixels, cap)
        rc = self._L.grk_amd_decode_packed(self._h, buf.ctypes.data, buf.size, PACKED_FORMATS.get(fmt, fmt), int(pitch), ptr, nbytes, on_device)
        if rc:
            self._surface_fail("decode_packed", rc)

    def packed_unpack_device(self, fmt, prec, w, h, d_packed, pitch, packed_bytes, d_planes, planes_bytes):
        """KU alone: the frame at d_packed -> tight planes Y, Cb, Cr back to back at d_planes (device pointers; queued on the stream)"""
        rc = self._L.grk_amd_packed_unpack_device(self._h, PACKED_FORMATS.get(fmt, fmt), int(prec), int(w), int(h), d_packed, int(pitch),
                                                  int(packed_bytes), d_planes, int(planes_bytes))
        if rc:
            self._surface_fail("packed_unpack_device", rc)

    def packed_pack_device(self, fmt, prec, w, h, d_planes, planes_bytes, d_packed, pitch, packed_bytes):
        """KK alone (the reverse)"""
        rc = self._L.grk_amd_packed_pack_device(self._h, PACKED_FORMATS.get(fmt, fmt), int(prec), int(w), int(h), d_planes, int(planes_bytes),
                                                d_packed, int(pitch), int(packed_bytes))
        if rc:
            self._surface_fail("packed_pack_device", rc)

    def packed_counters(self):
        """(launches of the unpack kernel, launches of the pack kernel) by this context so far"""
        return tuple(int(self._L.grk_amd_packed_counters(self._h, k)) for k in range(2))

    def fetch_table(self, nblocks):
        table = np.zeros(nblocks, CODED_DTYPE)
        tot = C.c_uint64(0)
        self._check(self._L.grk_amd_fetch_table(self._h, table.ctypes.data, C.byref(tot)), "fetch_table")
        return table, tot.value

    def fetch_coded(self, nbytes):
        coded = np.empty(nbytes, np.uint8)
        if nbytes:
            self._check(self._L.grk_amd_fetch_coded(self._h, coded.ctypes.data, nbytes), "fetch_coded")
        return coded

    def assemble_device(self, params, tile_index, flags=0, dst_offset=0):
        """Tier-2 on the device for the latest encode_tiles call (grk_amd_assemble_device) -> (bytes assembled, [tile-part lengths])."""
        idx = np.ascontiguousarray(np.asarray(tile_index, np.uint32))
        lens = np.zeros(idx.size, np.uint32)
        self._L.grk_amd_assemble_device.restype = C.c_int64
        self._L.grk_amd_assemble_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p]
        n = self._L.grk_amd_assemble_device(self._h, C.addressof(params), idx.size, idx.ctypes.data, flags, dst_offset, lens.ctypes.data)
        if n < 0:
            raise StageError("assemble_device", n, self._L.grk_amd_last_error(self._h).decode())
        return int(n), lens

    def assembled_parts(self):
        """grk_amd_assembled_parts: the tile-parts per tile of the latest assemble call (1: undivided)"""
        self._L.grk_amd_assembled_parts.restype = C.c_uint32
        self._L.grk_amd_assembled_parts.argtypes = [C.c_void_p]
        return int(self._L.grk_amd_assembled_parts(self._h))

    def stage_assemble_parts(self, params, tile_index, table, coded, flags=0, starts=None):
        """grk_amd_stage_assemble_parts: stage_assemble with every tile divided into tile-parts at the packets `starts` (None: under
        the division of `flags`) -> (bytes assembled, the parts' lengths [tile][part]).  StageError."""
        idx = np.ascontiguousarray(np.asarray(tile_index, np.uint32))
        t = np.ascontiguousarray(table, CODED_DTYPE)
        cbuf = np.ascontiguousarray(np.frombuffer(coded, np.uint8) if not isinstance(coded, np.ndarray) else coded)
        s = np.ascontiguousarray(starts, np.uint32) if starts is not None else None
        lens = np.zeros((idx.size, 256), np.uint32)
        fn = self._L.grk_amd_stage_assemble_parts
        fn.restype = C.c_int64
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p]
        n = fn(self._h, C.addressof(params), idx.size, idx.ctypes.data, int(flags), t.ctypes.data, cbuf.ctypes.data if cbuf.size else None,
               cbuf.size, s.ctypes.data if s is not None else None, s.size if s is not None else 0, lens.ctypes.data)
        if n < 0:
            raise StageError("stage_assemble_parts", n, self._L.grk_amd_last_error(self._h).decode())
        k = self.assembled_parts()
        return int(n), lens.reshape(-1)[:idx.size * k].reshape(idx.size, k).copy()

    def stage_assemble(self, params, tile_index, table, coded, flags=0, _fn="grk_amd_stage_assemble"):
        """Tier-2 on the device for a table of the caller's (grk_amd_stage_assemble): `table` CODED_DTYPE, len(tile_index) x (blocks of a
        tile) rows whose offsets point into `coded` (uint8; rows may share bytes) -> (bytes assembled, [tile-part lengths]); the bytes
        are fetch_assembled's.  StageError with the code and the context's reason when the call refuses."""
        idx = np.ascontiguousarray(np.asarray(tile_index, np.uint32))
        t = np.ascontiguousarray(table, CODED_DTYPE)
        cbuf = np.ascontiguousarray(np.frombuffer(coded, np.uint8) if not isinstance(coded, np.ndarray) else coded)
        lens = np.zeros(idx.size, np.uint32)
        fn = getattr(self._L, _fn)
        fn.restype = C.c_int64
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
        n = fn(self._h, C.addressof(params), idx.size, idx.ctypes.data, flags, t.ctypes.data, cbuf.ctypes.data if cbuf.size else None,
               cbuf.size, lens.ctypes.data)
        if n < 0:
            raise StageError(_fn[len("grk_amd_"):], n, self._L.grk_amd_last_error(self._h).decode())
        return int(n), lens

    def stage_assemble_msbs(self, params, tile_index, table, coded, flags=0):
        """stage_assemble with the rows' missing_msbs written (grk_amd_stage_assemble_msbs): the general zero-bit-plane tag tree, the
        tile-parts write_tile_part writes under CS_BLOCK_MSBS (accepted in `flags`, and implied)."""
        return self.stage_assemble(params, tile_index, table, coded, flags, _fn="grk_amd_stage_assemble_msbs")

    def assemble_device_async(self, params, tile_index, flags, stream_ptr):
        """grk_amd_assemble_device_async: Tier-2 of the latest encode queued on `stream_ptr`; results stay on the device."""
        idx = np.ascontiguousarray(np.asarray(tile_index, np.uint32))
        self._L.grk_amd_assemble_device_async.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]
        self._check(self._L.grk_amd_assemble_device_async(self._h, C.addressof(params), idx.size, idx.ctypes.data, flags, stream_ptr), "assemble_device_async")

    def assembled_table_ptr(self, which):
        self._L.grk_amd_assembled_table_ptr.restype = C.c_void_p
        self._L.grk_amd_assembled_table_ptr.argtypes = [C.c_void_p, C.c_int]
        return self._L.grk_amd_assembled_table_ptr(self._h, which)

    def fetch_assembled(self, offset, nbytes):
        out = np.empty(nbytes, np.uint8)
        self._L.grk_amd_fetch_assembled.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]
        if nbytes:
            self._check(self._L.grk_amd_fetch_assembled(self._h, offset, nbytes, out.ctypes.data), "fetch_assembled")
        return out

    def assembled_device_ptr(self):
        self._L.grk_amd_assembled_device_ptr.restype = C.c_void_p
        self._L.grk_amd_assembled_device_ptr.argtypes = [C.c_void_p]
        return self._L.grk_amd_assembled_device_ptr(self._h)

    def coded_device_ptr(self):
        return self._L.grk_amd_coded_device_ptr(self._h)

    def table_device_ptr(self, which):
        return self._L.grk_amd_table_device_ptr(self._h, which)

    def plane_device_ptr(self, which):
        return self._L.grk_amd_plane_device_ptr(self._h, which)

    def stage_ingest_mct(self, params, ntiles, d_pixels, d_planes):
        self._check(self._L.grk_amd_stage_ingest_mct(self._h, C.byref(params), ntiles, d_pixels, d_planes), "stage_ingest_mct")

    def stage_dwt_fwd(self, params, nplanes, d_in, d_out):
        self._check(self._L.grk_amd_stage_dwt_fwd(self._h, C.byref(params), nplanes, d_in, d_out), "stage_dwt_fwd")

    def stage_ht_encode(self, params, ntiles, d_mallat):
        self._check(self._L.grk_amd_stage_ht_encode(self._h, C.byref(params), ntiles, d_mallat), "stage_ht_encode")

    def stage_ht_encode16(self, params, ntiles, d_mallat16, flags=0):
        """K3 from int16 Mallat planes (grk_amd_stage_ht_encode16); flags: STAGE_HT_ROOM."""
        self._check(self._L.grk_amd_stage_ht_encode16(self._h, C.byref(params), ntiles, d_mallat16, flags), "stage_ht_encode16")

    def stage_ht_encode_drops(self, params, ntiles, d_mallat, planes16, d_drops):
        """K3 through the instances that take a per-block drop (grk_amd_stage_ht_encode_drops): d_drops = ntiles * blocks_per_tile
        bytes on the device, 0 .. 254 bit-planes left out or DROP_SKIP; keep them until the table has been fetched."""
        self._check(self._L.grk_amd_stage_ht_encode_drops(self._h, C.byref(params), ntiles, d_mallat, int(bool(planes16)), d_drops),
                    "stage_ht_encode_drops")

    def stage_rate_stats(self, params, ntiles, d_mallat, planes16, max_drop, first_rows=None, n=0, E=None):
        """The statistics kernel on planes of the caller's (grk_amd_stage_rate_stats) -> E uint64 [max_drop + 2, n].  first_rows: the
        map of a joint table (one first row per tile, rows of n entries), with E the table's contents beforehand; without one n is
        the call's blocks.  StageError with the code and the context's reason when the call refuses."""
        self._L.grk_amd_stage_rate_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_uint64,
                                                     C.c_void_p]
        rows = None
        if first_rows is None:
            n = self._L.grk_amd_tile_num_blocks(C.byref(params)) * ntiles
            out = np.zeros((int(max_drop) + 2, max(int(n), 0)), np.uint64)
        else:
            rows = np.ascontiguousarray(np.asarray(first_rows, np.uint64))
            out = np.array(E, np.uint64, order="C").reshape(int(max_drop) + 2, int(n))
        rc = self._L.grk_amd_stage_rate_stats(self._h, C.addressof(params), ntiles, d_mallat, int(bool(planes16)), int(max_drop),
                                              rows.ctypes.data if rows is not None else None, int(n), out.ctypes.data)
        if rc:
            raise StageError("stage_rate_stats", rc, self._L.grk_amd_last_error(self._h).decode())
        return out

    def _stage_alloc(self, name, L, E, W, max_drop, allow_skip, budget, res):
        """stage_rate_alloc and stage_quality_alloc: grk_amd_<name> with `budget` as the call takes it -> (drop bytes, res filled in)"""
        Lc = None if L is None else np.ascontiguousarray(L, np.uint32)
        Ec = None if E is None else np.ascontiguousarray(E, np.uint64)
        Wc = None if W is None else np.ascontiguousarray(W, np.float64)
        n = next((a.shape[-1] for a in (Wc, Lc, Ec) if a is not None), 0)
        rows = int(max_drop) + 2
        for a in (Lc, Ec):
            if a is not None and a.size != rows * n:
                raise ValueError("%s: a table of %d entries, not (max_drop + 2) x %d" % (name, a.size, n))
        if Wc is not None and Wc.size != n:
            raise ValueError("%s: %d weights for %d blocks" % (name, Wc.size, n))
        drops = np.zeros(max(n, 1), np.uint8)
        rc = getattr(self._L, "grk_amd_" + name)(self._h, *(a.ctypes.data if a is not None else None for a in (Lc, Ec, Wc)), n,
                                                 int(max_drop), int(bool(allow_skip)), budget, drops.ctypes.data, C.addressof(res))
        if rc:
            raise StageError(name, rc, self._L.grk_amd_last_error(self._h).decode())
        return drops[:n], res

    def stage_rate_alloc(self, L, E, W, max_drop, allow_skip, budget):
        """The allocator kernel on tables of the caller's (grk_amd_stage_rate_alloc): L uint32 and E uint64 [max_drop + 2, n], W
        float64 [n] -> (drop bytes uint8 [n], RateAllocResult).  None for a table passes a null pointer.  StageError when the call
        refuses."""
        self._L.grk_amd_stage_rate_alloc.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, C.c_uint64,
                                                     C.c_void_p, C.c_void_p]
        return self._stage_alloc("stage_rate_alloc", L, E, W, max_drop, allow_skip, int(budget), RateAllocResult())

    def encode_tiles_rate(self, params, ntiles, pixels_ptr, on_device, target_bytes, max_drop=0, allow_skip=False):
        """grk_amd_encode_tiles_rate: the batch's blocks in at most target_bytes -> (table, total arena bytes, RateResult)"""
        n = self._L.grk_amd_tile_num_blocks(C.byref(params)) * ntiles
        table = np.zeros(n, CODED_DTYPE)
        tot = C.c_uint64(0)
        rate, res = Rate(int(target_bytes), int(max_drop), int(bool(allow_skip))), RateResult()
        rc = self._L.grk_amd_encode_tiles_rate(self._h, C.byref(params), ntiles, pixels_ptr, int(on_device), C.byref(rate), table.ctypes.data,
                                               C.byref(tot), C.byref(res))
        if rc:
            raise RateError("encode_tiles_rate", rc, self._L.grk_amd_last_error(self._h).decode())
        return table, tot.value, res

    def encode_image_rate(self, layout, base, pixels, target_bytes, flags=0, max_drop=0, allow_skip=False, joint=False):
        """grk_amd_encode_image_rate: the image as a file of at most target_bytes -> (codestream bytes, RateResult).  joint: one set of
        tables and one multiplier over all geometry groups instead of a share of the budget for each"""
        px = np.ascontiguousarray(pixels)
        cap = px.size * 4 + (1 << 20)
        out = np.empty(cap, np.uint8)
        rate, res = Rate(int(target_bytes), int(max_drop), int(bool(allow_skip)), int(bool(joint))), RateResult()
        n = self._L.grk_amd_encode_image_rate(self._h, C.byref(layout), C.byref(base), px.ctypes.data, flags, C.byref(rate), out.ctypes.data,
                                              cap, C.byref(res))
        if n < 0:
            raise RateError("encode_image_rate", n, self._L.grk_amd_last_error(self._h).decode())
        return out[:n].tobytes(), res

    def encode_image_subsampled_rate(self, layout, base, sampling, planes, target_bytes, flags=0, max_drop=0, allow_skip=False):
        """grk_amd_encode_image_subsampled_rate: encode_image_subsampled in a file of at most target_bytes -> (codestream bytes,
        RateResult); one set of tables and one multiplier over every component"""
        dx = (C.c_uint8 * len(sampling))(*[int(a) for a, _ in sampling])
        dy = (C.c_uint8 * len(sampling))(*[int(b) for _, b in sampling])
        px = np.concatenate([np.ascontiguousarray(pl).reshape(-1) for pl in planes])
        cap = px.size * px.itemsize * 4 + (1 << 20)
        out = np.empty(cap, np.uint8)
        rate, res = Rate(int(target_bytes), int(max_drop), int(bool(allow_skip)), 1), RateResult()
        n = self._L.grk_amd_encode_image_subsampled_rate(self._h, C.byref(layout), C.byref(base), C.addressof(dx), C.addressof(dy),
                                                         px.ctypes.data, flags, C.byref(rate), out.ctypes.data, cap, C.byref(res))
        if n < 0:
            raise RateError("encode_image_subsampled_rate", n, self._L.grk_amd_last_error(self._h).decode())
        return out[:n].tobytes(), res

    def encode_surface_rate(self, layout, base, sampling, surface, pixels, target_bytes, flags=0, cap=None, max_drop=0, allow_skip=False):
        """grk_amd_encode_surface_rate: encode_surface in a file of at most target_bytes -> (codestream bytes, RateResult).  pixels: a
        uint8 numpy array holding the surface (host), or a device pointer (int) together with `cap`"""
        dx, dy = _sampling(sampling)
        ptr, nbytes, on_device = self._frame_arg(pixels, cap)
        out_cap = nbytes * 4 + (1 << 20)
        out = np.empty(out_cap, np.uint8)
        rate, res = Rate(int(target_bytes), int(max_drop), int(bool(allow_skip)), 1), RateResult()
        n = self._L.grk_amd_encode_surface_rate(self._h, C.byref(layout), C.byref(base), C.cast(dx, C.c_void_p), C.cast(dy, C.c_void_p),
                                                C.byref(surface), ptr, nbytes, on_device, flags, C.byref(rate), out.ctypes.data, out_cap,
                                                C.byref(res))
        if n < 0:
            raise RateError("encode_surface_rate", n, self._L.grk_amd_last_error(self._h).decode())
        return out[:n].tobytes(), res

    # ---- quality-targeted encodes: the rate calls' twins, for a PSNR (or, with psnr = 0, a distortion budget) ----
    @staticmethod
    def _quality(psnr, distortion, max_drop, allow_skip):
        return Quality(float(psnr), float(distortion), int(max_drop), int(bool(allow_skip))), QualityResult()

    def stage_quality_alloc(self, L, E, W, max_drop, allow_skip, budget):
        """The quality allocator kernel on tables of the caller's (grk_amd_stage_quality_alloc): L uint32 and E uint64 [max_drop + 2, n],
        W float64 [n], budget: the distortion D -> (drop bytes uint8 [n], QualityAllocResult).  None for a table passes a null
        pointer.  StageError when the call refuses."""
        return self._stage_alloc("stage_quality_alloc", L, E, W, max_drop, allow_skip, float(budget), QualityAllocResult())

    def encode_tiles_quality(self, params, ntiles, pixels_ptr, on_device, psnr, distortion=0.0, max_drop=0, allow_skip=False):
        """grk_amd_encode_tiles_quality: the batch's blocks in the fewest bytes for the target -> (table, total arena bytes, QualityResult)"""
        n = self._L.grk_amd_tile_num_blocks(C.byref(params)) * ntiles
        table = np.zeros(n, CODED_DTYPE)
        tot = C.c_uint64(0)
        q, res = self._quality(psnr, distortion, max_drop, allow_skip)
        rc = self._L.grk_amd_encode_tiles_quality(self._h, C.byref(params), ntiles, pixels_ptr, int(on_device), C.byref(q), table.ctypes.data,
                                                  C.byref(tot), C.byref(res))
        if rc:
            raise RateError("encode_tiles_quality", rc, self._L.grk_amd_last_error(self._h).decode())
        return table, tot.value, res

    def encode_image_quality(self, layout, base, pixels, psnr, distortion=0.0, flags=0, max_drop=0, allow_skip=False):
        """grk_amd_encode_image_quality: the image as the shortest file the allocator finds for the target, over joint tables ->
        (codestream bytes, QualityResult)"""
        px = np.ascontiguousarray(pixels)
        cap = px.size * 4 + (1 << 20)
        out = np.empty(cap, np.uint8)
        q, res = self._quality(psnr, distortion, max_drop, allow_skip)
        n = self._L.grk_amd_encode_image_quality(self._h, C.byref(layout), C.byref(base), px.ctypes.data, flags, C.byref(q), out.ctypes.data,
                                                 cap, C.byref(res))
        if n < 0:
            raise RateError("encode_image_quality", n, self._L.grk_amd_last_error(self._h).decode())
        return out[:n].tobytes(), res

    def encode_image_subsampled_quality(self, layout, base, sampling, planes, psnr, distortion=0.0, flags=0, max_drop=0, allow_skip=False):
        """grk_amd_encode_image_subsampled_quality -> (codestream bytes, QualityResult)"""
        dx = (C.c_uint8 * len(sampling))(*[int(a) for a, _ in sampling])
        dy = (C.c_uint8 * len(sampling))(*[int(b) for _, b in sampling])
        px = np.concatenate([np.ascontiguousarray(pl).reshape(-1) for pl in planes])
        cap = px.size * px.itemsize * 4 + (1 << 20)
        out = np.empty(cap, np.uint8)
        q, res = self._quality(psnr, distortion, max_drop, allow_skip)
        n = self._L.grk_amd_encode_image_subsampled_quality(self._h, C.byref(layout), C.byref(base), C.addressof(dx), C.addressof(dy),
                                                            px.ctypes.data, flags, C.byref(q), out.ctypes.data, cap, C.byref(res))
        if n < 0:
            raise RateError("encode_image_subsampled_quality", n, self._L.grk_amd_last_error(self._h).decode())
        return out[:n].tobytes(), res

    def encode_surface_quality(self, layout, base, sampling, surface, pixels, psnr, distortion=0.0, flags=0, cap=None, max_drop=0,
                               allow_skip=False):
        """grk_amd_encode_surface_quality -> (codestream bytes, QualityResult).  pixels: a uint8 numpy array holding the surface (host),
        or a device pointer (int) together with `cap`"""
        dx, dy = _sampling(sampling)
        ptr, nbytes, on_device = self._frame_arg(pixels, cap)
        out_cap = nbytes * 4 + (1 << 20)
        out = np.empty(out_cap, np.uint8)
        q, res = self._quality(psnr, distortion, max_drop, allow_skip)
        n = self._L.grk_amd_encode_surface_quality(self._h, C.byref(layout), C.byref(base), C.cast(dx, C.c_void_p), C.cast(dy, C.c_void_p),
                                                   C.byref(surface), ptr, nbytes, on_device, flags, C.byref(q), out.ctypes.data, out_cap,
                                                   C.byref(res))
        if n < 0:
            raise RateError("encode_surface_quality", n, self._L.grk_amd_last_error(self._h).decode())
        return out[:n].tobytes(), res

    def encode_packed_quality(self, layout, base, fmt, pixels, psnr, distortion=0.0, pitch=0, flags=0, cap=None, max_drop=0, allow_skip=False):
        """grk_amd_encode_packed_quality -> (codestream bytes, QualityResult)"""
        ptr, nbytes, on_device = self._frame_arg(pixels, cap)
        out_cap = nbytes * 4 + (1 << 20)
        out = np.empty(out_cap, np.uint8)
        q, res = self._quality(psnr, distortion, max_drop, allow_skip)
        n = self._L.grk_amd_encode_packed_quality(self._h, C.byref(layout), C.byref(base), PACKED_FORMATS.get(fmt, fmt), int(pitch), ptr, nbytes,
                                                  on_device, flags, C.byref(q), out.ctypes.data, out_cap, C.byref(res))
        if n < 0:
            raise RateError("encode_packed_quality", n, self._L.grk_amd_last_error(self._h).decode())
        return out[:n].tobytes(), res

    # ---- the rate- and quality-targeted calls that leave their file in device memory -> (device pointer, length, result) ----
    def _rate_device(self, what, fn, head, goal, res):
        d_file = C.c_void_p(0)
        n = fn(*(head + [C.byref(goal), C.byref(d_file), C.byref(res)]))
        if n < 0:
            raise RateError(what, n, self._L.grk_amd_last_error(self._h).decode())
        return int(d_file.value), int(n), res

    def _surface_head(self, layout, base, sampling, surface, pixels, flags, cap):
        dx, dy = _sampling(sampling)
        ptr, nbytes, on_device = self._frame_arg(pixels, cap)
        return [self._h, C.byref(layout), C.byref(base), C.cast(dx, C.c_void_p), C.cast(dy, C.c_void_p), C.byref(surface), ptr, nbytes,
                on_device, flags]

    def _packed_head(self, layout, base, fmt, pixels, pitch, flags, cap):
        ptr, nbytes, on_device = self._frame_arg(pixels, cap)
        return [self._h, C.byref(layout), C.byref(base), PACKED_FORMATS.get(fmt, fmt), int(pitch), ptr, nbytes, on_device, flags]

    def encode_surface_rate_device(self, layout, base, sampling, surface, pixels, target_bytes, flags=0, cap=None, max_drop=0, allow_skip=False):
        """grk_amd_encode_surface_rate_device: encode_surface_rate with Tier-2 on the device and the file left in device memory ->
        (device pointer, length, RateResult); the bytes belong to the context and stay valid until its next encode call"""
        return self._rate_device("encode_surface_rate_device", self._L.grk_amd_encode_surface_rate_device,
                                 self._surface_head(layout, base, sampling, surface, pixels, flags, cap),
                                 Rate(int(target_bytes), int(max_drop), int(bool(allow_skip)), 1), RateResult())

    def encode_surface_quality_device(self, layout, base, sampling, surface, pixels, psnr, distortion=0.0, flags=0, cap=None, max_drop=0,
                                      allow_skip=False):
        """grk_amd_encode_surface_quality_device -> (device pointer, length, QualityResult)"""
        q, res = self._quality(psnr, distortion, max_drop, allow_skip)
        return self._rate_device("encode_surface_quality_device", self._L.grk_amd_encode_surface_quality_device,
                                 self._surface_head(layout, base, sampling, surface, pixels, flags, cap), q, res)

    def encode_packed_rate_device(self, layout, base, fmt, pixels, target_bytes, pitch=0, flags=0, cap=None, max_drop=0, allow_skip=False):
        """grk_amd_encode_packed_rate_device -> (device pointer, length, RateResult)"""
        return self._rate_device("encode_packed_rate_device", self._L.grk_amd_encode_packed_rate_device,
                                 self._packed_head(layout, base, fmt, pixels, pitch, flags, cap),
                                 Rate(int(target_bytes), int(max_drop), int(bool(allow_skip)), 1), RateResult())

    def encode_packed_quality_device(self, layout, base, fmt, pixels, psnr, distortion=0.0, pitch=0, flags=0, cap=None, max_drop=0,
                                     allow_skip=False):
        """grk_amd_encode_packed_quality_device -> (device pointer, length, QualityResult)"""
        q, res = self._quality(psnr, distortion, max_drop, allow_skip)
        return self._rate_device("encode_packed_quality_device", self._L.grk_amd_encode_packed_quality_device,
                                 self._packed_head(layout, base, fmt, pixels, pitch, flags, cap), q, res)

    def rate_device_counters(self):
        """grk_amd_rate_device_counters of the latest such call: (Tier-2 passes on the device, bytes of coded blocks copied to the host)"""
        return tuple(int(self._L.grk_amd_rate_device_counters(self._h, k)) for k in range(2))

    def assemble_rate_device(self, params, tile_index, flags=0, dst_offset=0):
        """grk_amd_assemble_rate_device: assemble_device for the encode_tiles_rate / encode_tiles_quality call before it, the rows' zero
        bit-planes written -> (bytes assembled, [tile-part lengths]); RateError when the latest encode was not such a call"""
        idx = np.ascontiguousarray(np.asarray(tile_index, np.uint32))
        lens = np.zeros(idx.size, np.uint32)
        n = self._L.grk_amd_assemble_rate_device(self._h, C.byref(params), idx.size, idx.ctypes.data, flags, dst_offset, lens.ctypes.data)
        if n < 0:
            raise RateError("assemble_rate_device", n, self._L.grk_amd_last_error(self._h).decode())
        return int(n), lens

    def quality_last_budget(self):
        """grk_amd_quality_last_budget: the distortion budget the quality allocator last ran with (0.0 after a rate-targeted call)"""
        return float(self._L.grk_amd_quality_last_budget(self._h))

    def rate_num_blocks(self):
        """grk_amd_rate_num_blocks: the blocks the latest rate-targeted call's tables are over (a joint call: the whole image's)"""
        return int(self._L.grk_amd_rate_num_blocks(self._h))

    def rate_last_budget(self):
        """grk_amd_rate_last_budget: the blocks' budget of the latest allocator run (a whole-image call: its last round's)"""
        return int(self._L.grk_amd_rate_last_budget(self._h))

    def rate_unit_rows(self):
        """grk_amd_rate_unit_rows: the first row of every unit of those tables, in unit order (uint64 array)"""
        n = self._L.grk_amd_rate_unit_rows(self._h, None, 0)
        if n < 0:
            self._check(n, "rate_unit_rows")
        out = np.zeros(n, np.uint64)
        self._check(min(self._L.grk_amd_rate_unit_rows(self._h, out.ctypes.data, n), 0), "rate_unit_rows")
        return out

    def rate_tables(self, nblocks, max_drop=0):
        """The tables of the latest rate-targeted call (grk_amd_rate_tables) -> (L uint32 [Dmax + 2, nblocks], E uint64 [Dmax + 2,
        nblocks] (last row: SKIP), W float64 [nblocks], drop uint8 [nblocks])"""
        rows = (int(max_drop) or 6) + 2
        out = (np.zeros((rows, nblocks), np.uint32), np.zeros((rows, nblocks), np.uint64), np.zeros(nblocks, np.float64),
               np.zeros(nblocks, np.uint8))
        for which, a in enumerate(out):
            self._check(self._L.grk_amd_rate_tables(self._h, which, a.ctypes.data, a.nbytes), "rate_tables")
        return out

    def stage_ht_decode(self, params, ntiles, table, d_coded, coded_bytes, d_mallat):
        t = np.ascontiguousarray(table)
        self._check(self._L.grk_amd_stage_ht_decode(self._h, C.byref(params), ntiles, t.ctypes.data, d_coded, coded_bytes,
                                                    d_mallat),
                    "stage_ht_decode")

    def stage_ht_decode16(self, params, ntiles, table, d_coded, coded_bytes, d_mallat16):
        """K5 into int16 Mallat planes, with their range check (grk_amd_stage_ht_decode16)."""
        t = np.ascontiguousarray(table)
        self._check(self._L.grk_amd_stage_ht_decode16(self._h, C.byref(params), ntiles, t.ctypes.data, d_coded, coded_bytes,
                                                      d_mallat16),
                    "stage_ht_decode16")

    def decode_host(self, params, table, coded, ntiles=1, layout=None, out=None):
        """table: CODED_DTYPE rows, coded: bytes-like (host). Returns pixels (ntiles, C, H, W) -- or, with a `layout` (for this call),
        the uint8 buffer `out` (or a new one) holding them in that layout."""
        t = np.ascontiguousarray(table)
        cb = np.frombuffer(coded, np.uint8) if not isinstance(coded, np.ndarray) else np.ascontiguousarray(coded)
        dt = np.uint8 if params.prec <= 8 else np.uint16
        _, _, w, h = self.decode_size(params)
        if layout is not None:
            out = self._out_in_layout(params, layout, w, h, ntiles, out)
            self._with_decode_layout(layout, lambda: self._check(self._L.grk_amd_decode_tiles(
                self._h, C.byref(params), ntiles, t.ctypes.data, cb.ctypes.data, cb.size, 0, out.ctypes.data, 0), "decode_tiles"))
            return out
        out = np.zeros((ntiles, params.num_comps, h, w), dt)
        self._check(self._L.grk_amd_decode_tiles(self._h, C.byref(params), ntiles, t.ctypes.data, cb.ctypes.data, cb.size, 0,
                                                 out.ctypes.data, 0), "decode_tiles")
        return out

    def set_decode_reduce(self, reduce):
        """Decode at 1 / 2^reduce of the size from now on (grk_decompress -r; 0: full resolution).  Tables, coded bytes and
        segment lists stay the full tile's; decode_host returns, and decode_device writes, the reduced tiles."""
        self._check(self._L.grk_amd_set_decode_reduce(self._h, int(reduce)), "set_decode_reduce")
        self._reduce = int(reduce)

    def decode_size(self, params):
        """(x0, y0, w, h) of the tile the decode calls return under the current reduce setting (the full tile's size when the
        setting exceeds the tile's levels: the call itself refuses that)."""
        if self._reduce and self._reduce <= params.num_levels:
            return reduced_tile_rect(params, self._reduce)
        return params.tile_x0, params.tile_y0, params.tile_w, params.tile_h

    def decode_region_host(self, params, table, coded, x0, y0, x1, y1, layout=None, out=None):
        """Windowed decode of one tile -> pixels (C, y1 - y0, x1 - x0); the window is in the coordinates of the tile decode_size
        describes (the reduced tile under set_decode_reduce).  With a `layout` (its pitches the window's): the uint8 buffer."""
        t = np.ascontiguousarray(table)
        cb = np.frombuffer(coded, np.uint8) if not isinstance(coded, np.ndarray) else np.ascontiguousarray(coded)
        dt = np.uint8 if params.prec <= 8 else np.uint16
        if layout is not None:
            out = self._out_in_layout(params, layout, x1 - x0, y1 - y0, 1, out)
            self._with_decode_layout(layout, lambda: self._check(self._L.grk_amd_decode_region(
                self._h, C.byref(params), t.ctypes.data, cb.ctypes.data, cb.size, 0, x0, y0, x1, y1, out.ctypes.data, 0), "decode_region"))
            return out
        out = np.zeros((params.num_comps, y1 - y0, x1 - x0), dt)
        self._check(self._L.grk_amd_decode_region(self._h, C.byref(params), t.ctypes.data, cb.ctypes.data, cb.size, 0,
                                                  x0, y0, x1, y1, out.ctypes.data, 0), "decode_region")
        return out

    def decode_region_device(self, params, table, d_coded, coded_bytes, x0, y0, x1, y1, d_pixels):
        t = np.ascontiguousarray(table)
        self._check(self._L.grk_amd_decode_region(self._h, C.byref(params), t.ctypes.data, d_coded, coded_bytes, 1,
                                                  x0, y0, x1, y1, d_pixels, 1), "decode_region")

    def decode_device(self, params, ntiles, table, d_coded, coded_bytes, d_pixels):
        t = np.ascontiguousarray(table)
        self._check(self._L.grk_amd_decode_tiles(self._h, C.byref(params), ntiles, t.ctypes.data, d_coded, coded_bytes, 1,
                                                 d_pixels, 1), "decode_tiles")

    def decode_image(self, cs, layout=None, out=None):
        """Codestream (bytes-like, host) -> pixels (C, H, W) of the image area (grk_amd_decode_image, host pixels) -- or, with a
        `layout` (row_pitch the image's), the uint8 buffer holding the image in it."""
        buf = _cs_array(cs)
        info = read_header(buf)
        if layout is not None:
            out = self._out_in_layout(info.base, layout, info.layout.x1 - info.layout.x0, info.layout.y1 - info.layout.y0, 1, out)
            self._with_decode_layout(layout, lambda: self._check(self._L.grk_amd_decode_image(
                self._h, buf.ctypes.data, buf.size, out.ctypes.data, out.nbytes, 0), "decode_image"))
            return out
        out = np.zeros((info.base.num_comps, info.layout.y1 - info.layout.y0, info.layout.x1 - info.layout.x0),
                       np.uint8 if info.base.prec <= 8 else np.uint16)
        self._check(self._L.grk_amd_decode_image(self._h, buf.ctypes.data, buf.size, out.ctypes.data, out.nbytes, 0), "decode_image")
        return out

    def decode_image_view(self, cs, reduce=0, window=None, layout=None, out=None):
        """A view of the codestream's image (grk_amd_decode_image_view, host pixels): at 1 / 2^reduce of its size and / or the window
        (x0, y0, x1, y1) of that (reduced) image -> pixels (C, h, w) of the view -- or, with a `layout` (row_pitch the view's), the
        uint8 buffer holding the view in it."""
        buf = _cs_array(cs)
        info = read_header(buf)
        view = ImageView.make(reduce, window)
        w, h = C.c_uint32(0), C.c_uint32(0)
        rc = self._L.grk_amd_image_view_size(C.byref(info), C.byref(view), 0, C.byref(w), C.byref(h))
        if rc:                                   # (the call itself says why)
            out = np.zeros(16, np.uint8)
            self._check(self._L.grk_amd_decode_image_view(self._h, buf.ctypes.data, buf.size, C.byref(view), out.ctypes.data, 0, 0), "decode_image_view")
            raise _view_error("decode_image_view", rc)
        if layout is not None:
            out = self._out_in_layout(info.base, layout, w.value, h.value, 1, out)
            self._with_decode_layout(layout, lambda: self._check(self._L.grk_amd_decode_image_view(
                self._h, buf.ctypes.data, buf.size, C.byref(view), out.ctypes.data, out.nbytes, 0), "decode_image_view"))
            return out
        out = np.zeros((info.base.num_comps, h.value, w.value), np.uint8 if info.base.prec <= 8 else np.uint16)
        self._check(self._L.grk_amd_decode_image_view(self._h, buf.ctypes.data, buf.size, C.byref(view), out.ctypes.data, out.nbytes, 0),
                    "decode_image_view")
        return out

    def decode_image_view_planes(self, cs, reduce):
        """The same for a stream with sub-sampled components (upsampling off): one 2-D array per component, each of the component's
        own size at that reduce (image_view_size)."""
        buf = _cs_array(cs)
        info = read_header(buf)
        view = ImageView.make(reduce)
        dt = np.uint8 if info.base.prec <= 8 else np.uint16
        sizes = image_view_size(info, reduce)
        out = np.zeros(sum(w * h for w, h in sizes), dt)
        self._check(self._L.grk_amd_decode_image_view(self._h, buf.ctypes.data, buf.size, C.byref(view), out.ctypes.data, out.nbytes, 0),
                    "decode_image_view")
        at = np.concatenate([[0], np.cumsum([w * h for w, h in sizes])])
        return [out[at[k]:at[k + 1]].reshape(h, w) for k, (w, h) in enumerate(sizes)]

    def decode_image_view_device(self, cs, d_pixels, cap, reduce=0, window=None):
        """The same into device memory (asynchronous behind the reader: decode_status joins and reports)."""
        buf = _cs_array(cs)
        view = ImageView.make(reduce, window)
        self._check(self._L.grk_amd_decode_image_view(self._h, buf.ctypes.data, buf.size, C.byref(view), d_pixels, int(cap), 1), "decode_image_view")

    # ---- a codestream that lies in device memory (grk_amd_read_*_device, grk_amd_decode_image_device) ----
    def _read_device_fns(self):
        L = self._L
        if not getattr(L, "_read_device_bound", False):
            vp, u64 = C.c_void_p, C.c_uint64
            L.grk_amd_read_header_device.argtypes = [vp, vp, u64, C.POINTER(StreamInfo)]
            L.grk_amd_read_packets_device.restype = C.c_int64
            L.grk_amd_read_packets_device.argtypes = [vp, vp, u64, C.POINTER(StreamInfo), vp, u64]
            L.grk_amd_decode_image_device.argtypes = [vp, vp, u64, vp, u64, C.c_int]
            L.grk_amd_read_packets_device_ex.restype = C.c_int64
            L.grk_amd_read_packets_device_ex.argtypes = [vp, vp, u64, C.POINTER(StreamInfo), vp, u64, vp, vp, u64, C.POINTER(u64), vp, u64, C.POINTER(u64),
                                                         C.POINTER(u64)]
            L.grk_amd_decode_image_device_ex.argtypes = [vp, vp, u64, vp, u64, C.c_int]
            L.grk_amd_read_packets_device_parts.restype = C.c_int64
            L.grk_amd_read_packets_device_parts.argtypes = L.grk_amd_read_packets_device_ex.argtypes
            if hasattr(L, "grk_amd_read_packets_device_refine"):
                L.grk_amd_read_packets_device_refine.restype = C.c_int64
                L.grk_amd_read_packets_device_refine.argtypes = L.grk_amd_read_packets_device_ex.argtypes
            L.grk_amd_read_device_counters.restype = u64
            L.grk_amd_read_device_counters.argtypes = [vp, C.c_int]
            L._read_device_bound = True
        return L

    def read_header_device(self, d_cs, nbytes):
        """grk_amd_read_header_device: the main header of a codestream at device pointer d_cs -> StreamInfo; ReaderError when refused."""
        L = self._read_device_fns()
        info = StreamInfo()
        rc = L.grk_amd_read_header_device(self._h, int(d_cs), int(nbytes), C.byref(info))
        if rc:
            raise ReaderError("read_header_device", rc, self.last_error())
        return info

    def read_packets_device(self, d_cs, nbytes, info=None):
        """grk_amd_read_packets_device: every packet header of the codestream at device pointer d_cs, parsed on the device -> rows
        (CODED_DTYPE, host), what read_packets(...)["rows"] gives for the same bytes; ReaderError with its code when refused."""
        L = self._read_device_fns()
        if info is None:
            info = self.read_header_device(d_cs, nbytes)
        rows = np.zeros(int(info.num_blocks), CODED_DTYPE)
        n = L.grk_amd_read_packets_device(self._h, int(d_cs), int(nbytes), C.byref(info), rows.ctypes.data, rows.size)
        if n < 0:
            raise ReaderError("read_packets_device", n, self.last_error())
        return rows[:n]

    def decode_image_resident(self, d_cs, nbytes, pixels, cap, on_device=True):
        """grk_amd_decode_image_device: the codestream at device pointer d_cs (it is the coded buffer: nothing of it crosses the link)
        -> pixels at `pixels` (a device pointer, asynchronous behind the reader: decode_status joins; or with on_device False a host
        address).  ReaderError where the reader refuses the stream."""
        L = self._read_device_fns()
        rc = L.grk_amd_decode_image_device(self._h, int(d_cs), int(nbytes), int(pixels), int(cap), int(bool(on_device)))
        if rc:
            raise ReaderError("decode_image_resident", rc, self.last_error())

    def read_packets_device_parts(self, d_cs, nbytes, info=None):
        """grk_amd_read_packets_device_parts: read_packets_device_ex for a codestream whose tiles may be divided into tile-parts -> the
        dict read_packets_parts gives for the same bytes (the moves in the order of their dst)."""
        return self.read_packets_device_ex(d_cs, nbytes, info, "grk_amd_read_packets_device_parts")

    def read_packets_device_refine(self, d_cs, nbytes, info=None):
        """grk_amd_read_packets_device_refine: read_packets_device_parts for an HTJ2K codestream whose code-blocks carry refinement
        passes -> the dict read_packets_refine gives for the same bytes (the moves in the order of their dst)."""
        return self.read_packets_device_ex(d_cs, nbytes, info, "grk_amd_read_packets_device_refine")

    def read_device_parts_launches(self):
        """launches of KL-P / KH-P by this context's calls so far (grk_amd_read_device_counters, index 6)"""
        return int(self._read_device_fns().grk_amd_read_device_counters(self._h, 6))

    def read_packets_device_ex(self, d_cs, nbytes, info=None, _call="grk_amd_read_packets_device_ex"):
        """grk_amd_read_packets_device_ex: the general reader -- layers, LAZY / TERMALL -- of the codestream at device pointer d_cs
        -> the dict read_packets gives for the same bytes (the moves in the order of their dst); ReaderError with its code when
        refused."""
        L = self._read_device_fns()
        call = getattr(L, _call)
        if info is None:
            info = self.read_header_device(d_cs, nbytes)
        nseg, nmov, app = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        # the sizes first, then the tables
        n = call(self._h, int(d_cs), int(nbytes), C.byref(info), None, 0, None, None, 0, C.byref(nseg), None, 0, C.byref(nmov),
                                             C.byref(app))
        if n < 0:
            raise ReaderError(_call[len("grk_amd_"):], n, self.last_error())
        rows = np.zeros(int(n), CODED_DTYPE)
        first = np.zeros(int(n) + 1, np.uint32)
        segs = np.zeros(int(nseg.value), SEGMENT_DTYPE)
        moves = np.zeros(int(nmov.value), MOVE_DTYPE)
        n = call(self._h, int(d_cs), int(nbytes), C.byref(info), rows.ctypes.data, rows.size, first.ctypes.data, segs.ctypes.data,
                                             segs.size, C.byref(nseg), moves.ctypes.data, moves.size, C.byref(nmov), C.byref(app))
        if n < 0:
            raise ReaderError(_call[len("grk_amd_"):], n, self.last_error())
        return dict(rows=rows, first_segment=first, segments=segs, moves=moves, appendix_bytes=int(app.value))

    def decode_image_resident_ex(self, d_cs, nbytes, pixels, cap, on_device=True):
        """grk_amd_decode_image_device_ex: decode_image_resident on top of the general reader.  Without an appendix the stream is the
        coded buffer; with one it is staged in front of its appendix in the context's own buffer (read_device_counters()[4])."""
        L = self._read_device_fns()
        rc = L.grk_amd_decode_image_device_ex(self._h, int(d_cs), int(nbytes), int(pixels), int(cap), int(bool(on_device)))
        if rc:
            raise ReaderError("decode_image_resident_ex", rc, self.last_error())

    def read_device_counters(self):
        """(bytes copied device -> host, bytes copied host -> device, KC launches, chains parsed, bytes the _ex decode copied device
        to device, KC-L launches) by the calls above so far"""
        L = self._read_device_fns()
        return tuple(int(L.grk_amd_read_device_counters(self._h, k)) for k in range(6))

    def decode_image_counters(self):
        """(tiles whose packets were read, codestream bytes uploaded) by this context's decode_image / decode_image_view calls so far"""
        return int(self._L.grk_amd_decode_image_counters(self._h, 0)), int(self._L.grk_amd_decode_image_counters(self._h, 1))

    def place_tiles_clipped_device(self, d_tiles, ntiles, w, h, ncomp, bps, pos, d_image, img_w, img_h, channels=0):
        """pos: [(x, y)] of every unit in the destination's planes, signed; what falls outside img_w x img_h is not written.
        channels != 0: units and destination hold interleaved pixels of that many samples"""
        r = np.ascontiguousarray(pos, np.int32).reshape(-1)
        self._check(self._L.grk_amd_place_tiles_clipped_device(self._h, d_tiles, ntiles, w, h, ncomp, bps, channels, r.ctypes.data, d_image,
                                                               img_w, img_h), "place_tiles_clipped_device")

    def set_decode_upsample(self, on):
        """decode_image delivers sub-sampled components on the reference grid, W x H each (grk_amd_set_decode_upsample)"""
        self._check(self._L.grk_amd_set_decode_upsample(self._h, int(bool(on))), "set_decode_upsample")

    def decode_image_planes(self, cs):
        """Codestream -> one 2-D array per component, each of the component's own size (stream_comp_sizes): what decode_image
        writes for a stream with sub-sampled components while upsampling is off."""
        buf = _cs_array(cs)
        info = read_header(buf)
        dt = np.uint8 if info.base.prec <= 8 else np.uint16
        sizes = stream_comp_sizes(info)
        out = np.zeros(sum(w * h for w, h in sizes), dt)
        self._check(self._L.grk_amd_decode_image(self._h, buf.ctypes.data, buf.size, out.ctypes.data, out.nbytes, 0), "decode_image")
        at = np.concatenate([[0], np.cumsum([w * h for w, h in sizes])])
        return [out[at[k]:at[k + 1]].reshape(h, w) for k, (w, h) in enumerate(sizes)]

    def decode_image_device(self, cs, d_pixels, cap):
        """The same into device memory (asynchronous behind the reader: decode_status joins and reports)."""
        buf = _cs_array(cs)
        self._check(self._L.grk_amd_decode_image(self._h, buf.ctypes.data, buf.size, d_pixels, int(cap), 1), "decode_image")

    def decode_image_launches(self):
        """(gather launches, placement launches) of this context's decode_image calls so far"""
        return int(self._L.grk_amd_decode_image_launches(self._h, 0)), int(self._L.grk_amd_decode_image_launches(self._h, 1))

    def gather_device(self, moves, d_src, src_bytes, d_dst, dst_bytes):
        m = np.ascontiguousarray(moves, MOVE_DTYPE)
        self._check(self._L.grk_amd_gather_device(self._h, m.ctypes.data if m.size else None, m.size, d_src, int(src_bytes), d_dst,
                                                  int(dst_bytes)), "gather_device")

    def place_upsampled_device(self, d_tiles, nunits, w, h, ncomp, bps, origins, dx, dy, d_image, img_x0, img_y0, img_w, img_h):
        """origins: [(x, y)] of every unit's first sample in its component; the image area starts at (img_x0, img_y0) of the reference grid"""
        r = np.ascontiguousarray(origins, np.uint32).reshape(-1)
        self._check(self._L.grk_amd_place_upsampled_device(self._h, d_tiles, nunits, w, h, ncomp, bps, r.ctypes.data, dx, dy, d_image,
                                                           img_x0, img_y0, img_w, img_h), "place_upsampled_device")

    def place_tiles_device(self, d_tiles, ntiles, w, h, ncomp, bps, rects, d_image, img_w, img_h):
        """rects: [(x, y)] of every tile in the image's planes"""
        r = np.ascontiguousarray(rects, np.uint32).reshape(-1)
        self._check(self._L.grk_amd_place_tiles_device(self._h, d_tiles, ntiles, w, h, ncomp, bps, r.ctypes.data, d_image, img_w, img_h),
                    "place_tiles_device")

    def set_decode_steps(self, steps):
        """Band step sizes as the host's decoder holds them, [comp][band] (None / empty: back to the QCD words)."""
        a = np.ascontiguousarray(steps if steps is not None else [], np.float32).reshape(-1)
        self._check(self._L.grk_amd_set_decode_steps(self._h, a.ctypes.data if a.size else None, a.size), "set_decode_steps")

    def stream_wait_results(self, hip_stream):
        self._check(self._L.grk_amd_stream_wait_results(self._h, C.c_void_p(hip_stream)), "stream_wait_results")

    def block_distortion(self, nblocks):
        """Distortion decrease of every block of the latest encode (the rate-control hook, include/grok_amd.h)."""
        out = np.zeros(int(nblocks), np.float64)
        self._check(self._L.grk_amd_block_distortion(self._h, out.ctypes.data, int(nblocks)), "block_distortion")
        return out

    def probe_streams(self):
        """The context's stream probe now (grk_amd_probe_streams); returns the side streams replaced so far (-1: probe off)."""
        self._check(self._L.grk_amd_probe_streams(self._h), "probe_streams")
        return int(self._L.grk_amd_stream_probe_result(self._h))

    def internal_stream(self, which):
        self._L.grk_amd_internal_stream.restype = C.c_void_p
        self._L.grk_amd_internal_stream.argtypes = [C.c_void_p, C.c_int]
        return self._L.grk_amd_internal_stream(self._h, which)

    def streams_side_by_side(self, a, b):
        self._L.grk_amd_streams_side_by_side.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        r = self._L.grk_amd_streams_side_by_side(self._h, a, b)
        if r < 0:
            raise RuntimeError("streams_side_by_side failed: %d" % r)
        return bool(r)

    def set_pixel_hold(self, on):
        """True: the caller keeps a call's device pixels untouched until stream_wait_pixels / synchronize (include/grok_amd.h)."""
        if hasattr(self._L, "grk_amd_set_pixel_hold"):
            self._check(self._L.grk_amd_set_pixel_hold(self._h, int(bool(on))), "set_pixel_hold")

    def stream_wait_pixels(self, hip_stream):
        self._check(self._L.grk_amd_stream_wait_pixels(self._h, C.c_void_p(hip_stream)), "stream_wait_pixels")

    def set_decode_pipelining(self, frames_in_flight):
        """2..8: consecutive decode_device calls run on that many internal buffer / stream sets in turn (0 / 1: off)"""
        self._check(self._L.grk_amd_set_decode_pipelining(self._h, int(frames_in_flight)), "set_decode_pipelining")

    def set_pipelining(self, on):
        """False / True (two buffer sets) / 2 (three: results valid until the third next call)."""
        self._check(self._L.grk_amd_set_pipelining(self._h, int(on)), "set_pipelining")

    def decode_stream_wait_slot(self, stream_handle):
        """Makes that stream wait until the internal set the NEXT decode call uses has finished its last frame: the buffers handed
        over `frames in flight` calls ago may then be overwritten / read on it (include/grok_amd.h: buffer lifetime in a sequence)."""
        self._check(self._L.grk_amd_decode_stream_wait_slot(self._h, C.c_void_p(stream_handle)), "decode_stream_wait_slot")

    def set_decode_planes16(self, on):
        self._check(self._L.grk_amd_set_decode_planes16(self._h, int(on)), "set_decode_planes16")

    def plane_sample_bytes(self, params, decode=False):
        """(bytes per coefficient of the LL / Mallat planes the encode / decode path keeps for such tiles: 2 or 4, forward DWT
        levels that run on packed int16 pairs)"""
        n = C.c_uint32(0)
        b = self._L.grk_amd_plane_sample_bytes(self._h, C.byref(params), int(decode), C.byref(n))
        self._check(min(b, 0), "plane_sample_bytes")
        return b, n.value

    def set_overlap(self, on):
        self._check(self._L.grk_amd_set_overlap(self._h, int(bool(on))), "set_overlap")

    def set_decode_segments(self, per_block):
        """Part-1 blocks with several codeword segments (LAZY / TERMALL): per_block = [[(bytes, passes), ...], ...] in
        table order; None or [] returns to one segment per block."""
        if not per_block:
            self._check(self._L.grk_amd_set_decode_segments(self._h, None, None, 0), "set_decode_segments")
            return
        first = np.zeros(len(per_block) + 1, np.uint32)
        first[1:] = np.cumsum([len(b) for b in per_block])
        segs = np.array([v for b in per_block for s in b for v in s], np.uint32).reshape(-1, 2)
        self._check(self._L.grk_amd_set_decode_segments(self._h, first.ctypes.data, segs.ctypes.data if segs.size else None,
                                                        len(per_block)), "set_decode_segments")

    def set_decode_qcd(self, words):
        w = np.ascontiguousarray(words, np.uint16)
        self._check(self._L.grk_amd_set_decode_qcd(self._h, w.ctypes.data if w.size else None, w.size), "set_decode_qcd")

    def decode_status(self):
        self._check(self._L.grk_amd_decode_status(self._h), "decode_status")

    def stage_dwt_inv(self, params, nplanes, d_mallat, d_out):
        self._check(self._L.grk_amd_stage_dwt_inv(self._h, C.byref(params), nplanes, d_mallat, d_out), "stage_dwt_inv")

    def stage_egress(self, params, ntiles, d_planes, d_pixels):
        self._check(self._L.grk_amd_stage_egress(self._h, C.byref(params), ntiles, d_planes, d_pixels), "stage_egress")

    def enable_timing(self, on=True):
        self._check(self._L.grk_amd_enable_timing(self._h, int(on)), "enable_timing")

    def kernel_ms(self, which):
        n = C.c_uint32(0)
        ms = self._L.grk_amd_kernel_ms(self._h, which, C.byref(n))
        return ms, n.value


NODE_GATHER = 0x80000000


class Node:
    """grk_amd_node: one image over several GPUs natively -- a context + a host thread per entry of `devices` (None: all of
    the node; an entry may repeat: two contexts on one GPU), tiles t -> device t mod R, one codestream."""

    def __init__(self, devices=None, verbose=False):
        self._L = lib()
        h = C.c_void_p()
        if devices:
            arr = (C.c_int * len(devices))(*devices)
            rc = self._L.grk_amd_node_create(arr, len(devices), int(verbose), C.byref(h))
        else:
            rc = self._L.grk_amd_node_create(None, 0, int(verbose), C.byref(h))
        if rc != 0:
            raise RuntimeError("grk_amd_node_create failed: %d" % rc)
        self._h = h

    @property
    def size(self):
        return int(self._L.grk_amd_node_size(self._h))

    def encode_image(self, layout, base, pixels, flags=0, out=None):
        px = pixels if isinstance(pixels, np.ndarray) and pixels.flags["C_CONTIGUOUS"] else np.ascontiguousarray(pixels)
        cap = px.size * px.itemsize * 2 + (1 << 20)
        if out is None:
            out = np.empty(cap, np.uint8)
        n = self._L.grk_amd_node_encode_image(self._h, C.byref(layout), C.byref(base), px.ctypes.data, flags, out.ctypes.data, out.size)
        if n < 0:
            raise RuntimeError("node_encode_image failed: %d (%s)" % (n, self._L.grk_amd_node_last_error(self._h).decode()))
        return out[:n]

    def encode_image_device(self, layout, base, pixels_ptr, nbytes, device, flags=0, out=None):
        """The image resident in the memory of HIP device `device` at `pixels_ptr` (nbytes of it): grk_amd_node_encode_image_device."""
        if out is None:
            out = np.empty(nbytes * 2 + (1 << 20), np.uint8)
        fn = self._L.grk_amd_node_encode_image_device
        fn.restype = C.c_int64
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_uint64]
        n = fn(self._h, C.cast(C.byref(layout), C.c_void_p), C.cast(C.byref(base), C.c_void_p), pixels_ptr, int(device), flags, out.ctypes.data, out.size)
        if n < 0:
            raise RuntimeError("node_encode_image_device failed: %d (%s)" % (n, self._L.grk_amd_node_last_error(self._h).decode()))
        return out[:n]

    def close(self):
        if self._h:
            self._L.grk_amd_node_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
