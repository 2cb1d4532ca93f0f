// grok_amd/csrc/plugin.cpp -- libgrokj2k_plugin.so: the Grok plugin entry points on top of the
// C-ABI of libgrok_amd.so.  Replaces the in-tree do-nothing stub (src/lib/jp2_plugin/Plugin.cpp)
// and follows the protocol of SURVEY.md §3.3 / §8(b):
//
//   host: grk_initialize(dir) -> dlopen -> minpf_post_load_plugin()      registration
//         grk_plugin_init({deviceId, verbose}) -> plugin_init()          one context per process
//         grk_plugin_compress(params, cb) -> plugin_encode()             read image, run the hot
//             path on the MI355X, build the grk_plugin_tile tree, call the host's callback, which
//             runs grk_compress_with_plugin(codec, tile) (rate control 1, single tile: D2, D3)
//   any request outside the hot path (non-HT, multi-tile, unsupported file type, ...) returns a
//   non-zero code, which the host treats as "not handled" and takes its CPU path
//   (src/bin/jp2/grk_compress.cpp:2125-2168).
//
// The plugin owns the coded bytes the tile tree points at; they stay alive until the callback
// returns (the host aliases them: plugin_bridge.cpp:198-201).
#include "plugin_internal.h"
#include <cstdio>
#include <cstdlib>

namespace plugin {

grk_amd_ctx* g_ctx = nullptr;          // the device Grok named (grk_plugin_init_info.deviceId): the single-file entry points
static bool g_verbose = false;
// Every GPU the plugin may use: g_ctx first, then the node's other GPUs (GRK_AMD_PLUGIN_DEVICES=0,2,5 names them instead; an
// entry may repeat -- two contexts on one GPU).  Grok's batch protocol (grk_compress.cpp:2024-2050: a directory of images,
// each its own codestream) is where a node's GPUs run side by side with no exchange at all: file i goes to whichever device
// is free.
std::vector<std::unique_ptr<Dev>> g_devs;
// Self-check mode (grok.h:1719-1739, GRK_PLUGIN_STATE_DEBUG; set by the environment, GRK_AMD_PLUGIN_DEBUG=1, at
// plugin_init): the host skips its DC shift, MCT and DWT, runs its own Tier-1 over the coefficients the plugin hands it
// as "image" data, and compares every code-block (bytes, rates, pass counts, bounding boxes, step sizes) with the plugin's
// (TileProcessor.cpp:667-690, plugin_bridge.cpp:138-252).  A free parity check by the reference itself.
uint32_t g_debug_state = GRA_PLUGIN_STATE_NO_DEBUG;
std::mutex g_mu;

static int32_t plugin_exit() { drop_tile_cache(); drop_pinned_pool(); return 0; }
static void* plugin_create(gra_minpf_object_params*) { return nullptr; }
static int32_t plugin_destroy(void*) { return 0; }

} // namespace plugin
using namespace plugin;

// ---- the entry points Grok resolves by name (declared extern "C" in include/grk_plugin_abi.h) ---------------------

GRA_EXPORT gra_minpf_exit_func minpf_post_load_plugin(const char*, const gra_minpf_platform_services* services)
{
    if (!services || !services->registerObject) return nullptr;
    gra_minpf_register_params rp;
    rp.version.major = 1;                 // the loader insists on major == 1 (minpf_plugin_manager.cpp:47-72)
    rp.version.minor = 0;
    rp.createFunc = plugin_create;
    rp.destroyFunc = plugin_destroy;
    if (services->registerObject("grok_amd MI355X tile processor", &rp) < 0) return nullptr;
    return plugin_exit;
}

GRA_EXPORT bool plugin_init(gra_plugin_init_info info)
{
    std::lock_guard<std::mutex> lk(g_mu);
    g_verbose = info.verbose;
    if (const char* e = std::getenv("GRK_AMD_PLUGIN_DEBUG")) g_debug_state = std::atoi(e) ? GRA_PLUGIN_STATE_DEBUG : GRA_PLUGIN_STATE_NO_DEBUG;
    if (g_ctx) return true;
    const int rc = grk_amd_create(info.deviceId, info.verbose ? 1 : 0, &g_ctx);
    if (rc != GRK_AMD_OK) {
        if (g_verbose) std::fprintf(stderr, "[grok_amd plugin] no usable MI355X (rc=%d): host falls back to CPU\n", rc);
        g_ctx = nullptr;
        return false;
    }
    // the devices of the batch mode: the one Grok named first (it shares g_mu with the single-file entry points), then the
    // node's other GPUs, or what GRK_AMD_PLUGIN_DEVICES lists after it (e.g. "0,0": a second context on GPU 0)
    g_devs.clear();
    g_devs.emplace_back(new Dev());
    g_devs[0]->ctx = g_ctx; g_devs[0]->mu = &g_mu;
    std::vector<int> more;
    if (const char* e = std::getenv("GRK_AMD_PLUGIN_DEVICES")) {
        bool first = true;
        for (const char* q = e; *q;) {
            char* end = nullptr;
            const long v = std::strtol(q, &end, 10);
            if (end == q) break;
            if (!first) more.push_back((int)v);          // (the first entry is deviceId's place)
            first = false;
            q = *end == ',' ? end + 1 : end;
        }
    } else {
        const int n = grk_amd_device_count();
        for (int d = 0; d < n; ++d) if (d != info.deviceId) more.push_back(d);
    }
    for (int d : more) {
        grk_amd_ctx* c = nullptr;
        if (grk_amd_create(d, info.verbose ? 1 : 0, &c) != GRK_AMD_OK) continue;       // (a GPU that is not there is not used)
        g_devs.emplace_back(new Dev());
        g_devs.back()->ctx = c; g_devs.back()->mu = &g_devs.back()->own;
    }
    if (g_verbose) std::fprintf(stderr, "[grok_amd plugin] %zu device context(s)\n", g_devs.size());
    return true;
}

// (for tests and embedders: how many device contexts the batch mode spreads files over)
GRA_EXPORT uint32_t grk_amd_plugin_num_devices(void) { return (uint32_t)g_devs.size(); }

GRA_EXPORT int32_t plugin_encode(gra_cparameters* params, gra_encode_callback callback)
{
    if (!params) return -1;
    return encode_file(params, params->infile, params->outfile, callback);
}
GRA_EXPORT int32_t plugin_batch_encode(const char* input_dir, const char* output_dir, gra_cparameters* params,
                                       gra_encode_callback callback)
{
    return batch_encode(input_dir, output_dir, params, callback);
}
GRA_EXPORT bool plugin_is_batch_complete(void) { return batch_encode_done() && batch_decompress_done(); }
GRA_EXPORT void plugin_stop_batch_encode(void) { stop_batch_encode(); }

// Decode: Grok's plugin protocol end to end (decompress_file, plugin_decode.cpp); what is outside the hot path's scope is
// declined and the host keeps its CPU decoder (grk_decompress.cpp falls back when the plugin returns non-zero).  In a batch
// such a file is handed back to the host's decoder.
GRA_EXPORT int32_t plugin_decompress(void* decompress_parameters, gra_decode_callback callback)
{
    return decompress_file(decompress_parameters, reinterpret_cast<DecodeUserCallback>(callback));
}
GRA_EXPORT int32_t plugin_init_batch_decompress(const char* input_dir, const char* output_dir, void* decompress_parameters,
                                                gra_decode_callback callback)
{
    return init_batch_decompress(input_dir, output_dir, decompress_parameters, reinterpret_cast<DecodeUserCallback>(callback));
}
GRA_EXPORT int32_t plugin_batch_decompress(void) { return batch_decompress(); }
GRA_EXPORT void plugin_stop_batch_decompress(void) { stop_batch_decompress(); }

GRA_EXPORT uint32_t plugin_get_debug_state(void) { return g_debug_state; }
GRA_EXPORT void plugin_debug_mqc_next_cxd(void*, uint32_t) {}
GRA_EXPORT void plugin_debug_next_cxd(void*, uint32_t) {}
GRA_EXPORT void plugin_debug_mqc_next_plane(void*) {}
