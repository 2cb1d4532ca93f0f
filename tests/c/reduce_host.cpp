// tests/c/reduce_host.cpp -- test host for decode at reduced resolution (grk_decompress -r N, grk_dparameters::cp_reduce).
//
// The reference harness has no reduce knob; this host drives the reference library (libgrokj2k_ref.so) with cp_reduce set:
//   rh_read_header      the component rectangles grk_decompress_read_header reports
//   rh_decode           the reference's own decode
//   rh_plugin_decompress grk_plugin_decompress through the real plugin loader (the plugin loaded and initialised by the harness's
//                       ref_plugin_load / ref_plugin_init), with a host callback that does what grk_decompress's does
// Plain types of include/grk_plugin_abi.h and hand-declared prototypes of the few C functions of the reference's grok.h it calls:
// no header of the reference is needed.  Built at test time (tests/reducehost.py) with those symbols left undefined and loaded
// with ctypes after the harness has loaded the reference library process-wide: they bind to that one instance, whose plugin
// manager the harness's ref_plugin_load initialised.
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include "grk_plugin_abi.h"

extern "C" {
// grok.h (the library's C API; the opaque objects are grk_object*)
void grk_decompress_set_default_params(void* parameters);
void* grk_stream_create_mem_stream(uint8_t* buf, size_t buffer_len, bool owns_buffer, bool is_read_stream);
void* grk_decompress_create(int format, void* stream);
bool grk_decompress_init(void* codec, void* parameters);
bool grk_decompress_read_header(void* codec, gra_header_info* header_info);
gra_image* grk_decompress_get_composited_image(void* codec);
bool grk_decompress_set_window(void* codec, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1);
bool grk_decompress(void* codec, gra_plugin_tile* tile);
bool grk_decompress_end(void* codec);
void grk_object_unref(void* obj);
int32_t grk_plugin_decompress(void* decompress_parameters, int32_t (*callback)(void* info));
}

namespace {
constexpr int kCodecJ2K = 0;       // GRK_CODEC_J2K
constexpr int kJ2KFmt = 1;         // GRK_J2K_FMT
constexpr size_t kParamBytes = 1u << 16;      // room for grk_decompress_parameters (its head is gra_decompress_parameters_head)

// grk_plugin_decompress_callback_info (grok.h:1817-1838): what the host's callback is handed
struct HostDecodeInfo {
    size_t deviceId;
    gra_init_decompressors_func init_decompressors_func;
    const char* input_file_name;
    const char* output_file_name;
    int32_t decod_format, cod_format;       /* GRK_SUPPORTED_FILE_FMT */
    void* stream; void* codec;
    gra_header_info header_info;
    void* decompressor_parameters;          /* grk_decompress_parameters */
    gra_image* image;
    bool plugin_owns_image;
    gra_plugin_tile* tile;
    unsigned int error_code;
    uint32_t decompress_flags;
    uint32_t full_image_x0, full_image_y0;
    void* user_data;
};

// components back to back into out (room for cap int32), their sizes into dims [C][4] = x0, y0, w, h
int copy_image(const gra_image* img, int32_t* out, uint64_t cap, uint32_t* dims, int32_t C)
{
    if (!img || img->numcomps != C) return -5;
    uint64_t at = 0;
    for (int k = 0; k < C; ++k) {
        const gra_image_comp& c = img->comps[k];
        if (!c.data || at + (uint64_t)c.w * c.h > cap) return -6;
        dims[4 * k] = c.x0; dims[4 * k + 1] = c.y0; dims[4 * k + 2] = c.w; dims[4 * k + 3] = c.h;
        for (uint32_t y = 0; y < c.h; ++y, at += c.w) std::memcpy(out + at, c.data + (size_t)y * c.stride, (size_t)c.w * 4);
    }
    return 0;
}

struct Params {
    alignas(16) unsigned char bytes[kParamBytes];
    gra_decompress_parameters_head* head() { return reinterpret_cast<gra_decompress_parameters_head*>(bytes); }
};

const uint8_t* g_j2k = nullptr;
uint64_t g_len = 0;
int32_t* g_out = nullptr;
uint64_t g_cap = 0;
uint32_t* g_dims = nullptr;
int32_t g_C = 0;
int32_t g_stage[4];

int32_t host_callback(void* vinfo)
{
    HostDecodeInfo* info = static_cast<HostDecodeInfo*>(vinfo);
    if (!info) return -1;
    if (info->decompress_flags & GRA_PLUGIN_DECODE_CLEAN) {
        g_stage[3]++;
        if (info->stream) grk_object_unref(info->stream);
        info->stream = nullptr;
        if (info->codec) grk_object_unref(info->codec);
        info->codec = nullptr;
        info->image = nullptr;
        return 0;
    }
    if (info->decompress_flags & GRA_DECODE_HEADER) {
        g_stage[0]++;
        if (!info->stream) info->stream = grk_stream_create_mem_stream(const_cast<uint8_t*>(g_j2k), g_len, false, true);
        if (!info->stream) return 1;
        if (!info->codec) {
            info->codec = grk_decompress_create(kCodecJ2K, info->stream);
            if (!info->codec) return 1;
            // (decompressor_parameters is the grk_decompress_parameters, whose first member is the core grk_dparameters)
            if (!grk_decompress_init(info->codec, info->decompressor_parameters)) return 1;
        }
        if (!grk_decompress_read_header(info->codec, &info->header_info)) return 1;
        info->image = grk_decompress_get_composited_image(info->codec);
        if (info->init_decompressors_func) {
            const int rc = info->init_decompressors_func(&info->header_info, info->image);
            if (rc || !(info->decompress_flags & (GRA_DECODE_T2 | GRA_DECODE_T1))) return rc;
        } else if (!(info->decompress_flags & (GRA_DECODE_T2 | GRA_DECODE_T1))) {
            return 0;
        }
    }
    if (info->decompress_flags & (GRA_DECODE_T2 | GRA_DECODE_T1)) {
        g_stage[1]++;
        if (!info->codec) return 1;
        if (!info->tile && !(info->decompress_flags & GRA_DECODE_T1)) return 1;
        if (info->tile) info->tile->decompress_flags = info->decompress_flags;
        if (!grk_decompress_set_window(info->codec, 0, 0, 0, 0)) return 1;
        if (!grk_decompress(info->codec, info->tile)) return 1;
        if (!grk_decompress_end(info->codec)) return 1;
        if (!(info->decompress_flags & GRA_DECODE_T1) || !(info->decompress_flags & GRA_DECODE_POST_T1)) return 0;
    }
    if (info->decompress_flags & GRA_DECODE_POST_T1) {
        g_stage[2]++;
        return copy_image(info->image, g_out, g_cap, g_dims, g_C) ? 1 : 0;
    }
    return -1;
}
} // namespace

extern "C" {
// grk_decompress_read_header with cp_reduce = reduce: dims [C][4] = x0, y0, w, h of every component
int32_t rh_read_header(const uint8_t* j2k, uint64_t len, uint32_t reduce, uint32_t* dims, int32_t C)
{
    Params* prm = new Params();
    std::memset(prm->bytes, 0, kParamBytes);
    grk_decompress_set_default_params(prm->bytes);
    reinterpret_cast<gra_dparameters*>(prm->bytes)->cp_reduce = (uint8_t)reduce;
    void* stream = grk_stream_create_mem_stream(const_cast<uint8_t*>(j2k), len, false, true);
    void* codec = stream ? grk_decompress_create(kCodecJ2K, stream) : nullptr;
    int32_t rc = -1;
    gra_header_info* hi = new gra_header_info();
    do {
        if (!codec) break;
        if (!grk_decompress_init(codec, prm->bytes)) { rc = -2; break; }
        if (!grk_decompress_read_header(codec, hi)) { rc = -3; break; }
        const gra_image* img = grk_decompress_get_composited_image(codec);
        if (!img || img->numcomps != C) { rc = -5; break; }
        for (int k = 0; k < C; ++k) {
            const gra_image_comp& c = img->comps[k];
            dims[4 * k] = c.x0; dims[4 * k + 1] = c.y0; dims[4 * k + 2] = c.w; dims[4 * k + 3] = c.h;
        }
        rc = 0;
    } while (0);
    if (stream) grk_object_unref(stream);
    if (codec) grk_object_unref(codec);
    delete hi;
    delete prm;
    return rc;
}

// the reference's decode with cp_reduce = reduce: components back to back into out (cap int32), sizes into dims [C][4]
int32_t rh_decode(const uint8_t* j2k, uint64_t len, uint32_t reduce, int32_t* out, uint64_t cap, uint32_t* dims, int32_t C)
{
    Params* prm = new Params();
    std::memset(prm->bytes, 0, kParamBytes);
    grk_decompress_set_default_params(prm->bytes);
    reinterpret_cast<gra_dparameters*>(prm->bytes)->cp_reduce = (uint8_t)reduce;
    void* stream = grk_stream_create_mem_stream(const_cast<uint8_t*>(j2k), len, false, true);
    void* codec = stream ? grk_decompress_create(kCodecJ2K, stream) : nullptr;
    int32_t rc = -1;
    gra_header_info* hi = new gra_header_info();
    do {
        if (!codec) break;
        if (!grk_decompress_init(codec, prm->bytes)) { rc = -2; break; }
        if (!grk_decompress_read_header(codec, hi)) { rc = -3; break; }
        if (!grk_decompress(codec, nullptr)) { rc = -4; break; }
        rc = copy_image(grk_decompress_get_composited_image(codec), out, cap, dims, C);
        if (rc == 0) grk_decompress_end(codec);
    } while (0);
    if (stream) grk_object_unref(stream);
    if (codec) grk_object_unref(codec);
    delete hi;
    delete prm;
    return rc;
}

// grk_plugin_decompress with cp_reduce = reduce (the stream also lies in the file `infile`, as with grk_decompress -i):
// returns what grk_plugin_decompress returns (0: the image was decoded and stored), stages[4] = header, Tier-2, post-T1 and
// clean calls of the host callback; the stored image as rh_decode
int32_t rh_plugin_decompress(const uint8_t* j2k, uint64_t len, const char* infile, uint32_t reduce, int32_t* out, uint64_t cap,
                             uint32_t* dims, int32_t C, int32_t* stages)
{
    Params* prm = new Params();
    std::memset(prm->bytes, 0, kParamBytes);
    gra_decompress_parameters_head* h = prm->head();
    grk_decompress_set_default_params(&h->core);
    h->core.cp_reduce = (uint8_t)reduce;
    h->decod_format = kJ2KFmt;
    if (infile) std::strncpy(h->infile, infile, GRA_PATH_LEN - 1);
    g_j2k = j2k; g_len = len; g_out = out; g_cap = cap; g_dims = dims; g_C = C;
    std::memset(g_stage, 0, sizeof(g_stage));
    const int32_t rc = grk_plugin_decompress(prm->bytes, host_callback);
    if (stages) std::memcpy(stages, g_stage, sizeof(g_stage));
    delete prm;
    return rc;
}
}
