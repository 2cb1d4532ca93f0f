// grok_amd/csrc/packed.cpp -- packed 4:2:2 frames (include/grok_amd.h: GRK_AMD_PACKED_*; packed_format.h) into a codestream and
// back.  The calls are thin: the frame's three tight planes lie in a buffer the context owns (img_planes), every plane from a
// 256-byte boundary; KU (kernels_packed.hip) fills it from the frame and the surface encode (surface.cpp) runs on it as a planar
// 4:2:2 device surface, or the surface decode (decode_image.cpp) fills it and KK packs it into the frame.  Every refusal of the
// frame itself is decided here, on the host, before any GPU work.
#include "context.h"
#include "image.h"
#include "packed_format.h"
#include "t2_reader.h"

using namespace grk_amd;

namespace {

int refuse(const char** why, int rc, const char* text) { if (why) *why = text; return rc; }

// a frame of w x h luma samples: the pitch resolved, the bytes from the base to the end of the last row's last container
struct PackedFrame { uint32_t format, prec, w, h, cw, bps; uint64_t pitch, bytes; };

int check_format(int format, uint32_t prec, const char** why)
{
    if (format < 0 || (uint32_t)format >= kPackedFormats) return refuse(why, GRK_AMD_ERR_INVALID, "packed: an unknown format");
    if (!packed_prec_ok((uint32_t)format, prec)) return refuse(why, GRK_AMD_ERR_INVALID, "packed: a precision outside the format's range");
    return GRK_AMD_OK;
}

int resolve_frame(int format, uint64_t w, uint64_t h, uint32_t prec, uint64_t pitch, PackedFrame& f, const char** why)
{
    { const int rc = check_format(format, prec, why); if (rc) return rc; }
    if (!w || !h || w >> 32 || h >> 32) return refuse(why, GRK_AMD_ERR_INVALID, "packed: an empty image area");
    const uint64_t row = packed_row_bytes((uint32_t)format, w);
    if (!pitch) pitch = packed_default_pitch((uint32_t)format, w);
    if (pitch < row) return refuse(why, GRK_AMD_ERR_INVALID, "packed: a pitch is smaller than a row");
    if (pitch % packed_align((uint32_t)format)) return refuse(why, GRK_AMD_ERR_INVALID, "packed: a pitch off the format's alignment");
    if (pitch >> 48) return refuse(why, GRK_AMD_ERR_INVALID, "packed: a pitch is out of range");
    f = PackedFrame{(uint32_t)format, prec, (uint32_t)w, (uint32_t)h, (uint32_t)((w + 1) / 2), prec <= 8 ? 1u : 2u, pitch, (h - 1) * pitch + row};
    return GRK_AMD_OK;
}

int resolve_image(int format, const grk_amd_image_layout* im, uint32_t prec, uint64_t pitch, PackedFrame& f, const char** why)
{
    if (!im) return refuse(why, GRK_AMD_ERR_INVALID, "packed: a null argument");
    // (the format and its precision first: an unknown format has no other rule to break)
    { const int rc = check_format(format, prec, why); if (rc) return rc; }
    if (im->x1 <= im->x0 || im->y1 <= im->y0) return refuse(why, GRK_AMD_ERR_INVALID, "packed: an empty image area");
    if (im->x0 & 1u) return refuse(why, GRK_AMD_ERR_UNSUPPORTED, "packed: an image area with odd x0 (the chroma grid does not start on a macropixel)");
    return resolve_frame(format, (uint64_t)im->x1 - im->x0, (uint64_t)im->y1 - im->y0, prec, pitch, f, why);
}

uint64_t up256(uint64_t n) { return (n + 255u) & ~(uint64_t)255u; }

// the context's planes for a frame: Y at 0, Cb and Cr each from the next 256-byte boundary -- as a planar 4:2:2 surface
struct PlaneSet {
    uint64_t at[3], total;
    grk_amd_surface surface;
    explicit PlaneSet(const PackedFrame& f)
    {
        const uint64_t ny = (uint64_t)f.w * f.h * f.bps, nc = (uint64_t)f.cw * f.h * f.bps;
        at[0] = 0; at[1] = up256(ny); at[2] = at[1] + up256(nc); total = at[2] + nc;
        surface = grk_amd_surface{};
        surface.comp[0] = grk_amd_surface_comp{at[0], (uint64_t)f.w * f.bps, 1, 0};
        surface.comp[1] = grk_amd_surface_comp{at[1], (uint64_t)f.cw * f.bps, 1, 0};
        surface.comp[2] = grk_amd_surface_comp{at[2], (uint64_t)f.cw * f.bps, 1, 0};
    }
};

const uint8_t kDx[3] = {1, 2, 2}, kDy[3] = {1, 1, 1};

PackedArgs kernel_args(const PackedFrame& f, void* packed, uint8_t* y, uint8_t* cb, uint8_t* cr)
{
    return PackedArgs{(uint8_t*)packed, f.pitch, y, cb, cr, f.w, f.h, f.format, f.prec};
}

int queue_packed_kernel(grk_amd_ctx* c, bool pack, const PackedArgs& a)
{
    HIP_TRY(c, pack ? launch_packed_pack(a, c->stream) : launch_packed_unpack(a, c->stream), pack ? "launch packing" : "launch unpacking");
    ++c->packed_counters[pack ? 1 : 0];
    return GRK_AMD_OK;
}

// what an encode refuses of its tile parameters and its frame; the frame resolved
int open_encode(grk_amd_ctx* c, const grk_amd_image_layout* im, const grk_amd_tile_params* base, int format, uint64_t pitch, const void* pixels,
                uint64_t cap, int pixels_on_device, PackedFrame& f)
{
    const char* why = "";
    if (format < 0 || (uint32_t)format >= kPackedFormats) return fail(c, GRK_AMD_ERR_INVALID, "packed: an unknown format");
    if (base->num_comps != 3) return fail(c, GRK_AMD_ERR_INVALID, "packed: three components");
    if (base->mct) return fail(c, GRK_AMD_ERR_INVALID, "packed: no colour transform (the frame holds Y, Cb, Cr)");
    const int rc = resolve_image(format, im, base->prec, pitch, f, &why);
    if (rc) return fail(c, rc, why);
    if (pixels_on_device && (uintptr_t)pixels % packed_align(f.format)) return fail(c, GRK_AMD_ERR_INVALID, "packed: a device base off the format's alignment");
    if (f.bytes > cap) return fail(c, GRK_AMD_ERR_OVERFLOW, "packed: the frame does not fit `cap`");
    return GRK_AMD_OK;
}

// the frame on the device (a host frame: the context's copy of it) unpacked into the context's planes
int unpack_frame(grk_amd_ctx* c, const PackedFrame& f, const PlaneSet& ps, const void* pixels, int pixels_on_device)
{
    HIP_TRY(c, hipSetDevice(c->device), "set device");
    HIP_TRY(c, c->img_planes.ensure(ps.total), "alloc the planes");
    void* d_frame = const_cast<void*>(pixels);
    if (!pixels_on_device) {
        HIP_TRY(c, c->img_pixels.ensure(f.bytes), "alloc the frame");
        d_frame = c->img_pixels.p;
        const int rc = copy_h2d(c, d_frame, pixels, f.bytes); if (rc) return rc;
    }
    uint8_t* const pl = (uint8_t*)c->img_planes.p;
    return queue_packed_kernel(c, false, kernel_args(f, d_frame, pl + ps.at[0], pl + ps.at[1], pl + ps.at[2]));
}

} // namespace

extern "C" uint64_t grk_amd_packed_bytes(int format, const grk_amd_image_layout* im, uint32_t prec, uint64_t* pitch, const char** why)
{
    if (why) *why = "";
    PackedFrame f;
    if (resolve_image(format, im, prec, pitch ? *pitch : 0, f, why)) return 0;
    if (pitch) *pitch = f.pitch;
    return f.bytes;
}

extern "C" uint64_t grk_amd_packed_counters(grk_amd_ctx* c, int which)
{
    return c && which >= 0 && which < 2 ? c->packed_counters[which] : 0;
}

extern "C" int64_t grk_amd_encode_packed(grk_amd_ctx* c, const grk_amd_image_layout* im, const grk_amd_tile_params* base, int format, uint64_t pitch,
                                         const void* pixels, uint64_t cap, int pixels_on_device, uint32_t flags, uint8_t* out, uint64_t out_cap)
{
    if (!c || !im || !base || !pixels || !out) return GRK_AMD_ERR_INVALID;
    PackedFrame f;
    int rc = open_encode(c, im, base, format, pitch, pixels, cap, pixels_on_device, f);
    if (rc) return rc;
    const PlaneSet ps(f);
    rc = unpack_frame(c, f, ps, pixels, pixels_on_device);
    if (rc) return rc;
    return encode_surface_job(c, im, base, kDx, kDy, &ps.surface, c->img_planes.p, ps.total, 1, flags, out, out_cap);
}

extern "C" int64_t grk_amd_encode_packed_device(grk_amd_ctx* c, const grk_amd_image_layout* im, const grk_amd_tile_params* base, int format,
                                                uint64_t pitch, const void* pixels, uint64_t cap, int pixels_on_device, uint32_t flags, void** d_file)
{
    if (!c || !im || !base || !pixels || !d_file) return GRK_AMD_ERR_INVALID;
    *d_file = nullptr;
    PackedFrame f;
    int rc = open_encode(c, im, base, format, pitch, pixels, cap, pixels_on_device, f);
    if (rc) return rc;
    const PlaneSet ps(f);
    rc = unpack_frame(c, f, ps, pixels, pixels_on_device);
    if (rc) return rc;
    return encode_surface_job(c, im, base, kDx, kDy, &ps.surface, c->img_planes.p, ps.total, 1, flags, nullptr, 0, d_file);
}

extern "C" int64_t grk_amd_encode_packed_rate(grk_amd_ctx* c, const grk_amd_image_layout* im, const grk_amd_tile_params* base, int format,
                                              uint64_t pitch, const void* pixels, uint64_t cap, int pixels_on_device, uint32_t flags,
                                              const grk_amd_rate* rate, uint8_t* out, uint64_t out_cap, grk_amd_rate_result* result)
{
    if (!c || !im || !base || !pixels || !out || !rate) return GRK_AMD_ERR_INVALID;
    PackedFrame f;
    int rc = open_encode(c, im, base, format, pitch, pixels, cap, pixels_on_device, f);
    if (rc) return rc;
    { const int rr = rate_refusal(c, rate); if (rr) return rr; }          // (before any GPU work, as the surface call has it)
    const PlaneSet ps(f);
    rc = unpack_frame(c, f, ps, pixels, pixels_on_device);
    if (rc) return rc;
    return encode_surface_rate_job(c, im, base, kDx, kDy, &ps.surface, c->img_planes.p, ps.total, 1, flags, rate, out, out_cap, result);
}

extern "C" int64_t grk_amd_encode_packed_quality(grk_amd_ctx* c, const grk_amd_image_layout* im, const grk_amd_tile_params* base, int format,
                                                 uint64_t pitch, const void* pixels, uint64_t cap, int pixels_on_device, uint32_t flags,
                                                 const grk_amd_quality* quality, uint8_t* out, uint64_t out_cap, grk_amd_quality_result* result)
{
    if (!c || !im || !base || !pixels || !out || !quality) return GRK_AMD_ERR_INVALID;
    PackedFrame f;
    int rc = open_encode(c, im, base, format, pitch, pixels, cap, pixels_on_device, f);
    if (rc) return rc;
    QualityTarget qt;          // (before any GPU work, as the surface call has it)
    rc = quality_target(c, quality, base->prec, quality_samples(*im, base->num_comps, kDx, kDy), result, qt);
    if (rc) return rc;
    const PlaneSet ps(f);
    rc = unpack_frame(c, f, ps, pixels, pixels_on_device);
    if (rc) return rc;
    return encode_surface_rate_job(c, im, base, kDx, kDy, &ps.surface, c->img_planes.p, ps.total, 1, flags, &qt.rate, out, out_cap, nullptr, &qt.goal);
}

// ... and their twins that leave the file in device memory (grk_amd_encode_surface_rate_device / _quality_device behind the unpack)
extern "C" int64_t grk_amd_encode_packed_rate_device(grk_amd_ctx* c, const grk_amd_image_layout* im, const grk_amd_tile_params* base, int format,
                                                     uint64_t pitch, const void* pixels, uint64_t cap, int pixels_on_device, uint32_t flags,
                                                     const grk_amd_rate* rate, void** d_file, grk_amd_rate_result* result)
{
    if (!c || !im || !base || !pixels || !d_file || !rate) return GRK_AMD_ERR_INVALID;
    *d_file = nullptr;
    PackedFrame f;
    int rc = open_encode(c, im, base, format, pitch, pixels, cap, pixels_on_device, f);
    if (rc) return rc;
    { const int rr = rate_refusal(c, rate); if (rr) return rr; }
    const PlaneSet ps(f);
    rc = unpack_frame(c, f, ps, pixels, pixels_on_device);
    if (rc) return rc;
    return encode_surface_rate_job(c, im, base, kDx, kDy, &ps.surface, c->img_planes.p, ps.total, 1, flags, rate, nullptr, 0, result, nullptr, d_file);
}

extern "C" int64_t grk_amd_encode_packed_quality_device(grk_amd_ctx* c, const grk_amd_image_layout* im, const grk_amd_tile_params* base, int format,
                                                        uint64_t pitch, const void* pixels, uint64_t cap, int pixels_on_device, uint32_t flags,
                                                        const grk_amd_quality* quality, void** d_file, grk_amd_quality_result* result)
{
    if (!c || !im || !base || !pixels || !d_file || !quality) return GRK_AMD_ERR_INVALID;
    *d_file = nullptr;
    PackedFrame f;
    int rc = open_encode(c, im, base, format, pitch, pixels, cap, pixels_on_device, f);
    if (rc) return rc;
    QualityTarget qt;
    rc = quality_target(c, quality, base->prec, quality_samples(*im, base->num_comps, kDx, kDy), result, qt);
    if (rc) return rc;
    const PlaneSet ps(f);
    rc = unpack_frame(c, f, ps, pixels, pixels_on_device);
    if (rc) return rc;
    return encode_surface_rate_job(c, im, base, kDx, kDy, &ps.surface, c->img_planes.p, ps.total, 1, flags, &qt.rate, nullptr, 0, nullptr, &qt.goal, d_file);
}

extern "C" int grk_amd_decode_packed(grk_amd_ctx* c, const uint8_t* cs, uint64_t len, int format, uint64_t pitch, void* pixels, uint64_t cap,
                                     int pixels_on_device)
{
    if (!c || !cs || !pixels) return GRK_AMD_ERR_INVALID;
    if (format < 0 || (uint32_t)format >= kPackedFormats) return fail(c, GRK_AMD_ERR_INVALID, "packed: an unknown format");
    grk_amd_stream_info info;
    std::string err;
    int rc = read_stream_header(cs, len, info, err);
    if (rc) return fail(c, rc, err.c_str());
    bool fits = info.base.num_comps == 3 && packed_prec_ok((uint32_t)format, info.base.prec);
    for (uint32_t k = 0; fits && k < 3; ++k) fits = info.comp_dx[k] == kDx[k] && info.comp_dy[k] == kDy[k];
    if (!fits) return fail(c, GRK_AMD_ERR_UNSUPPORTED, "packed: the stream is not 3 components with factors (1,1), (2,1), (2,1) at a precision of the format");
    PackedFrame f;
    const char* why = "";
    rc = resolve_image(format, &info.layout, info.base.prec, pitch, f, &why);
    if (rc) return fail(c, rc, why);
    if (pixels_on_device && (uintptr_t)pixels % packed_align(f.format)) return fail(c, GRK_AMD_ERR_INVALID, "packed: a device base off the format's alignment");
    if (f.bytes > cap) return fail(c, GRK_AMD_ERR_OVERFLOW, "packed: the frame does not fit `cap`");
    rc = refuse_context(c, "grk_amd_decode_packed", " at reduced resolution"); if (rc) return rc;
    const PlaneSet ps(f);
    HIP_TRY(c, hipSetDevice(c->device), "set device");
    HIP_TRY(c, c->img_planes.ensure(ps.total), "alloc the planes");
    // a host frame travels both ways: what is no sample keeps its value
    void* d_frame = pixels;
    if (!pixels_on_device) {
        HIP_TRY(c, c->img_pixels.ensure(f.bytes), "alloc the frame");
        d_frame = c->img_pixels.p;
        rc = copy_h2d(c, d_frame, pixels, f.bytes); if (rc) return rc;
    }
    rc = decode_onto_surface(c, "grk_amd_decode_packed", cs, len, &ps.surface, c->img_planes.p, ps.total, 1, !pixels_on_device);
    if (rc) return rc;
    uint8_t* const pl = (uint8_t*)c->img_planes.p;
    rc = queue_packed_kernel(c, true, kernel_args(f, d_frame, pl + ps.at[0], pl + ps.at[1], pl + ps.at[2]));
    if (rc || pixels_on_device) return rc;
    rc = copy_d2h(c, pixels, d_frame, f.bytes); if (rc) return rc;
    return grk_amd_decode_status(c);
}

// ---- the kernels alone ---------------------------------------------------------------------------------------------------------
static int packed_kernel_device(grk_amd_ctx* c, bool pack, int format, uint32_t prec, uint32_t w, uint32_t h, void* packed, uint64_t pitch,
                                uint64_t packed_bytes, void* planes, uint64_t planes_bytes)
{
    if (!c || !packed || !planes) return GRK_AMD_ERR_INVALID;
    PackedFrame f;
    const char* why = "";
    const int rc = resolve_frame(format, w, h, prec, pitch, f, &why);
    if (rc) return fail(c, rc, why);
    if ((uintptr_t)packed % packed_align(f.format)) return fail(c, GRK_AMD_ERR_INVALID, "packed: a device base off the format's alignment");
    const uint64_t ny = (uint64_t)f.w * f.h * f.bps, nc = (uint64_t)f.cw * f.h * f.bps;
    if (f.bytes > packed_bytes) return fail(c, GRK_AMD_ERR_OVERFLOW, "packed: the frame does not fit `packed_bytes`");
    if (ny + 2 * nc > planes_bytes) return fail(c, GRK_AMD_ERR_OVERFLOW, "packed: the planes do not fit `planes_bytes`");
    HIP_TRY(c, hipSetDevice(c->device), "set device");
    uint8_t* const pl = (uint8_t*)planes;
    return queue_packed_kernel(c, pack, kernel_args(f, packed, pl, pl + ny, pl + ny + nc));
}

extern "C" int grk_amd_packed_unpack_device(grk_amd_ctx* c, int format, uint32_t prec, uint32_t w, uint32_t h, const void* packed, uint64_t pitch,
                                            uint64_t packed_bytes, void* planes, uint64_t planes_bytes)
{
    return packed_kernel_device(c, false, format, prec, w, h, const_cast<void*>(packed), pitch, packed_bytes, planes, planes_bytes);
}

extern "C" int grk_amd_packed_pack_device(grk_amd_ctx* c, int format, uint32_t prec, uint32_t w, uint32_t h, const void* planes, uint64_t planes_bytes,
                                          void* packed, uint64_t pitch, uint64_t packed_bytes)
{
    return packed_kernel_device(c, true, format, prec, w, h, packed, pitch, packed_bytes, const_cast<void*>(planes), planes_bytes);
}
