// grok_amd/csrc/plugin_encode.cpp -- the encode side of libgrokj2k_plugin.so: gra_cparameters -> grk_amd_tile_params, one file
// through the plugin protocol (load, GPU, the host's callback), the route of an image of several tiles, the batch thread.
#include "plugin_internal.h"
#include <algorithm>
#include <atomic>
#include <cctype>
#include <condition_variable>
#include <cstdio>
#include <thread>
#include <dlfcn.h>

namespace plugin {

// does the tile grid cell anchored at (tx0, ty0) cover the image area, which starts at (image_offset_x0, image_offset_y0)
// (grk_compress -d, stored as grk_image x0 / y0 by the host's image readers)?  With sub-sampled components (grk_compress -s dx,dy:
// every component of a PNM alike) the area on the reference grid is (w - 1) dx + 1 wide (image_format/PNMFormat.cpp:388-392).
bool single_tile(const gra_cparameters* cp, uint32_t w, uint32_t h)
{
    const uint64_t ox = cp->image_offset_x0, oy = cp->image_offset_y0;
    const uint64_t gw = (uint64_t)(w - 1) * cp->subsampling_dx + 1, gh = (uint64_t)(h - 1) * cp->subsampling_dy + 1;
    return !cp->tile_size_on || !(cp->tx0 > ox || cp->ty0 > oy || (uint64_t)cp->tx0 + cp->t_width < ox + gw ||
                                  (uint64_t)cp->ty0 + cp->t_height < oy + gh);
}

// does the host make quality layers from the passes' rates and distortions (TileProcessor::needs_rate_control,
// tile/TileProcessor.cpp:75-90; grk_compress -r / -q set cp_disto_alloc / cp_fixed_quality and one entry per layer)?
bool wants_rate_control(const gra_cparameters* cp)
{
    for (uint32_t l = 0; l < std::min<uint32_t>(std::max<uint32_t>(cp->tcp_numlayers, 1u), 100u); ++l)
        if ((cp->cp_disto_alloc && cp->tcp_rates[l] > 0.0) || (cp->cp_fixed_quality && cp->tcp_distoratio[l] > 0.0)) return true;
    return cp->tcp_numlayers > 1;
}

// multi = false: the parameters of THE tile of a single-tile image (what the plugin protocol can carry, D3);
// multi = true: the base parameters of an image of several tiles (tile size / origin filled per tile by grk_amd_layout_tile)
bool params_from_cparameters(const gra_cparameters* cp, uint32_t w, uint32_t h, uint32_t comps, uint32_t prec,
                             grk_amd_tile_params& p, bool multi)
{
    if (!cp->isHT || !(cp->cblk_sty & GRA_CBLKSTY_HT)) return false;             // hot path = HTJ2K only
    if (!multi && !single_tile(cp, w, h)) return false;
    if (cp->numpocs || cp->roi_compno >= 0) return false;
    // Quality layers / rate targets: the HOST forms the layers (its Tier-2, from the rates and the distortion decreases the tile tree
    // carries: gpu_step fills them); this library's own writer -- the route an image of several tiles takes -- writes one layer
    if (multi && wants_rate_control(cp)) return false;
    // Sub-sampled components, every component alike (all a PNM can carry): component c of the tile is [ceil(x0 / dx), ceil(x1 / dx))
    // (tile/TileProcessor.cpp:605-612) -- w x h samples whose origin is ceil(offset / d); the sub-sampling itself is the host's SIZ.
    // The several-tiles route writes SIZ itself, with XRsiz = YRsiz = 1: declined there
    if (cp->subsampling_dx < 1 || cp->subsampling_dy < 1 || cp->subsampling_dx > 255 || cp->subsampling_dy > 255) return false;
    if (multi && (cp->subsampling_dx != 1 || cp->subsampling_dy != 1)) return false;
    // (an offset that is not a multiple of the factor: the component the host derives, ceil(x1 / dx) - ceil(x0 / dx), is a column
    //  short of the file's -- the host's own business)
    if (cp->image_offset_x0 % cp->subsampling_dx || cp->image_offset_y0 % cp->subsampling_dy) return false;
    if (cp->numresolution < 1 || cp->numresolution > GRK_AMD_MAX_LEVELS + 1) return false;
    std::memset(&p, 0, sizeof p);
    p.tile_w = w; p.tile_h = h; p.num_comps = (uint16_t)comps; p.prec = (uint8_t)prec; p.sgnd = 0;
    // the tile = the image area, wherever it lies; in the component's own coordinates
    p.tile_x0 = (cp->image_offset_x0 + cp->subsampling_dx - 1) / cp->subsampling_dx;
    p.tile_y0 = (cp->image_offset_y0 + cp->subsampling_dy - 1) / cp->subsampling_dy;
    p.irreversible = cp->irreversible ? 1 : 0;
    // tcp_mct as grk_compress leaves it: 255 = "not set" (the library then applies RCT/ICT to >= 3 components,
    // CodeStreamCompress.cpp:345-352), 0 / 1 as given, 2 = custom array MCT (mct_data) -- outside the hot path
    if (cp->tcp_mct == 2 || cp->mct_data) return false;
    p.mct = cp->tcp_mct == 255 ? (comps >= 3 ? 1 : 0) : (cp->tcp_mct ? 1 : 0);
    p.num_levels = (uint8_t)(cp->numresolution - 1);
    p.cblk_w_exp = (uint8_t)ceil_log2(cp->cblockw_init ? cp->cblockw_init : 64);
    p.cblk_h_exp = (uint8_t)ceil_log2(cp->cblockh_init ? cp->cblockh_init : 64);
    // precincts (grk_compress -c): sizes from the highest resolution down, the last one halved for the resolutions beyond
    // the list, exponent = floor(log2), at least 1 -- CodeStreamCompress.cpp:475-514
    if ((cp->csty & 1u) && cp->res_spec) {
        auto fl = [](uint32_t v) { uint32_t e = 0; while (v >>= 1) ++e; return e; };
        const uint32_t rs = std::min<uint32_t>(cp->res_spec, GRA_J2K_MAXRLVLS);
        for (uint32_t q = 0; q < cp->numresolution; ++q) {
            const uint32_t r = cp->numresolution - 1 - q;
            const uint32_t pw = q < rs ? cp->prcw_init[q] : cp->prcw_init[rs - 1] >> (q - (rs - 1));
            const uint32_t ph = q < rs ? cp->prch_init[q] : cp->prch_init[rs - 1] >> (q - (rs - 1));
            const uint32_t ex = pw < 1 ? 1 : fl(pw), ey = ph < 1 ? 1 : fl(ph);
            if (ex > 15 || ey > 15) return false;
            // (a precinct of ONE sample: exponent byte 0, which grk_amd_tile_params reads as "the default 15 / 15" -- the host
            //  would cut 1 x 1 precincts where we built one; its CPU path takes such a list, as on the decode side)
            if ((ex | (ey << 4)) == 0) return false;
            p.precinct_exp[r] = (uint8_t)(ex | (ey << 4));
        }
    }
    if (multi) { p.tile_w = std::min(w, cp->t_width); p.tile_h = std::min(h, cp->t_height); p.tile_x0 = p.tile_y0 = 0; }
    return grk_amd_tile_num_blocks(&p) > 0;
}

// One file through the protocol in three steps, so that the batch mode can overlap them across files:
//   load      read + de-interleave the PNM                                                  (disk, host)
//   gpu_step  H2D, encode, D2H, the grk_plugin_tile tree (+ the self-check image)            (GPU; holds g_mu)
//   host_step the host's callback: its own Tier-2 over our blocks, the file                  (host library)
namespace {
struct EncodeJob {
    std::string in, out;
    HostPixels px;
    uint32_t w = 0, h = 0, comps = 0, prec = 0;
    grk_amd_tile_params p{};
    gra_plugin_tile* tile = nullptr;
    void* dbg_image = nullptr;
    void (*unref)(void*) = nullptr;
};
}

static bool load_step(EncodeJob& j) { return read_pnm(j.in.c_str(), g_ctx, j.px, j.w, j.h, j.comps, j.prec); }

// self-check mode: the "image" the host gets holds our sub-band coefficients (it skips its own DC shift / MCT / DWT and
// codes them with its own Tier-1).  The image object is made by the host library itself (grk_image_new, resolved from
// the process we were loaded into) so that the host can treat it as any other.
static bool make_debug_image(const gra_cparameters* cp, EncodeJob& j, grk_amd_ctx* ctx)
{
    typedef gra_image* (*image_new_fn)(uint16_t, gra_image_cmptparm*, int32_t, bool);
    auto image_new = reinterpret_cast<image_new_fn>(dlsym(RTLD_DEFAULT, "grk_image_new"));
    j.unref = reinterpret_cast<void (*)(void*)>(dlsym(RTLD_DEFAULT, "grk_object_unref"));
    const grk_amd_tile_params& p = j.p;
    if (!image_new || !j.unref) return false;
    std::vector<gra_image_cmptparm> cps(j.comps);
    for (auto& c : cps) { c.dx = cp->subsampling_dx; c.dy = cp->subsampling_dy; c.w = j.w; c.stride = 0; c.h = j.h; c.x0 = p.tile_x0; c.y0 = p.tile_y0; c.prec = (uint8_t)j.prec; c.sgnd = false; }
    gra_image* img = image_new((uint16_t)j.comps, cps.data(), j.comps >= 3 ? 1 /* GRK_CLRSPC_SRGB */ : 2 /* GRK_CLRSPC_GRAY */, true);
    if (!img) return false;
    img->x0 = cp->image_offset_x0; img->y0 = cp->image_offset_y0;
    img->x1 = img->x0 + (j.w - 1) * cp->subsampling_dx + 1; img->y1 = img->y0 + (j.h - 1) * cp->subsampling_dy + 1;
    bool ok = true;
    for (uint32_t c = 0; c < j.comps && ok; ++c)
        ok = img->comps[c].data && grk_amd_fetch_coefficients(ctx, c, img->comps[c].data, img->comps[c].stride) == GRK_AMD_OK;
    if (!ok) { j.unref(&img->obj); return false; }
    j.dbg_image = img;
    return true;
}

static bool gpu_step(gra_cparameters* cp, EncodeJob& j, Dev* dev = nullptr)
{
    if (!params_from_cparameters(cp, j.w, j.h, j.comps, j.prec, j.p)) return false;
    grk_amd_ctx* const ctx = dev ? dev->ctx : g_ctx;
    std::lock_guard<std::mutex> lk(dev ? *dev->mu : g_mu);
    j.tile = grk_amd_plugin_tile_create(ctx, &j.p, j.px.data(), 0);
    if (!j.tile) return false;
    bool ok = !wants_rate_control(cp) || grk_amd_plugin_tile_fill_distortion(ctx, j.tile) == GRK_AMD_OK;
    if (ok) {
        j.px.reset();                           // the pixels are on the device / coded: the host callback loads its own copy
        ok = !(g_debug_state & GRA_PLUGIN_STATE_DEBUG) || make_debug_image(cp, j, ctx);
    }
    if (!ok) { grk_amd_plugin_tile_destroy(j.tile); j.tile = nullptr; }
    return ok;
}

static int32_t host_step(gra_cparameters* cp, EncodeJob& j, gra_encode_callback cb)
{
    gra_encode_callback_info info{};
    info.input_file_name = j.in.c_str();
    info.outputFileNameIsRelative = false;
    info.output_file_name = j.out.c_str();
    info.compressor_parameters = cp;
    info.image = static_cast<gra_image*>(j.dbg_image);     // nullptr: the host callback loads the image itself (grk_compress.cpp:1636)
    info.tile = j.tile;
    info.error_code = 0;
    cb(&info);
    if (j.dbg_image) j.unref(&static_cast<gra_image*>(j.dbg_image)->obj);
    grk_amd_plugin_tile_destroy(j.tile);
    j.tile = nullptr; j.dbg_image = nullptr;
    return info.error_code;
}

// An image of SEVERAL tiles.  The plugin protocol attaches one grk_plugin_tile to every tile of an image (D3), so the host
// cannot be handed the blocks tile by tile; but the whole file is within reach: every tile through the hot path
// (grk_amd_encode_image: tiles grouped by geometry, one batch per group) and the codestream through our own Tier-2 writer,
// which writes what the reference writes byte for byte (SIZ / COD / QCD / TLM / PLT / SOP / EPH, the progression orders,
// precincts).  Only raw codestreams (.j2k / .j2c / .jpc): the JP2 boxes stay with the host.  Returns 0 (handled: the file
// is written, the host's callback is not needed) or -1 (the host takes its CPU path).
static int32_t encode_multi_tile(gra_cparameters* cp, EncodeJob& j, Dev* dev = nullptr)
{
    if (g_debug_state & GRA_PLUGIN_STATE_DEBUG) return -1;
    const size_t dot = j.out.rfind('.');
    if (dot == std::string::npos) return -1;
    std::string ext = j.out.substr(dot + 1);
    for (auto& ch : ext) ch = (char)std::tolower((unsigned char)ch);
    if (ext != "j2k" && ext != "j2c" && ext != "jpc") return -1;
    grk_amd_tile_params base;
    if (!params_from_cparameters(cp, j.w, j.h, j.comps, j.prec, base, true)) return -1;
    if (cp->prog_order < 0 || cp->prog_order > 4 || cp->cp_num_comments) return -1;
    // what this writer does not write the host's way stays with the host (its CPU path): tile-part division (grk_compress -u),
    // profiles / extensions (-Z ...: rsiz beyond the JPH flag the library sets for HT itself), size caps, rate or quality targets
    if (cp->tp_on || (cp->rsiz & ~0x4000u) || cp->max_cs_size || cp->max_comp_size) return -1;
    for (uint32_t l = 0; l < std::max<uint32_t>(cp->tcp_numlayers, 1u); ++l)
        if (cp->tcp_rates[l] != 0.0 || cp->tcp_distoratio[l] != 0.0) return -1;
    grk_amd_image_layout im{cp->image_offset_x0, cp->image_offset_y0, cp->image_offset_x0 + j.w, cp->image_offset_y0 + j.h,
                            cp->tx0, cp->ty0, cp->t_width, cp->t_height};
    const uint32_t flags = (cp->writeTLM ? GRK_AMD_CS_TLM : 0u) | (cp->writePLT ? GRK_AMD_CS_PLT : 0u) |
                           ((cp->csty & 2u) ? GRK_AMD_CS_SOP : 0u) | ((cp->csty & 4u) ? GRK_AMD_CS_EPH : 0u) |
                           GRK_AMD_CS_PROG((uint32_t)cp->prog_order);
    std::vector<uint8_t> out(j.px.size() * 2 + (1u << 20));
    int64_t n;
    {
        std::lock_guard<std::mutex> lk(dev ? *dev->mu : g_mu);
        n = grk_amd_encode_image(dev ? dev->ctx : g_ctx, &im, &base, j.px.data(), flags, out.data(), out.size());
    }
    if (n <= 0) return -1;
    FILE* f = std::fopen(j.out.c_str(), "wb");
    if (!f) return -1;
    const bool ok = std::fwrite(out.data(), 1, (size_t)n, f) == (size_t)n;
    std::fclose(f);
    return ok ? 0 : -1;
}

int32_t encode_file(gra_cparameters* cp, const char* in, const char* out, gra_encode_callback cb)
{
    if (!g_ctx || !cp || !cb || !in || !out) return -1;
    EncodeJob j;
    j.in = in; j.out = out;
    if (!load_step(j)) return -1;
    if (!single_tile(cp, j.w, j.h)) return encode_multi_tile(cp, j);
    if (!gpu_step(cp, j)) return -1;
    return host_step(cp, j, cb);
}

// ---- batch mode: a worker thread walks the input directory ----------------------------------------
static std::thread g_batch;
static std::atomic<bool> g_batch_done{true}, g_batch_stop{false};

// a hand-over slot between two stages: holds one job
namespace {
struct Slot {
    std::mutex m; std::condition_variable cv; std::unique_ptr<EncodeJob> job; bool closed = false;
    void put(std::unique_ptr<EncodeJob> j) { std::unique_lock<std::mutex> lk(m); cv.wait(lk, [&] { return !job; }); job = std::move(j); cv.notify_all(); }
    std::unique_ptr<EncodeJob> take() { std::unique_lock<std::mutex> lk(m); cv.wait(lk, [&] { return job || closed; }); auto j = std::move(job); cv.notify_all(); return j; }
    void close() { std::lock_guard<std::mutex> lk(m); closed = true; cv.notify_all(); }
};
}

// the files of the directory, then three overlapped stages over them (a file is in one stage at a time, every stage
// works on one file at a time): while the GPU codes file n, file n + 1 is being read and de-interleaved and the host
// library runs its Tier-2 and writes file n - 1.  Hand-over slots hold one job each, so at most three images are
// in flight.
static void batch_encode_thread(const std::string& in, const std::string& out, gra_cparameters* cp, gra_encode_callback callback)
{
    const std::vector<std::string> names = list_files(in, kImageExtensions);
    Slot loaded, coded;
    std::thread reader([&]() {
        for (const auto& name : names) {
            if (g_batch_stop.load()) break;
            auto j = std::make_unique<EncodeJob>();
            j->in = in + "/" + name; j->out = out + "/" + name.substr(0, name.rfind('.')) + ".j2k";
            if (load_step(*j)) loaded.put(std::move(j));
        }
        loaded.close();
    });
    std::thread writer([&]() {
        while (auto j = coded.take()) host_step(cp, *j, callback);
    });
    // one GPU stage per device context: whichever is free takes the next loaded file (files are independent: replicas,
    // no exchange -- SURVEY.md 8(e) "single-tile configs: replicas only")
    std::vector<std::thread> gpus;
    for (size_t d = 0; d < g_devs.size(); ++d)
        gpus.emplace_back([&, d]() {
            Dev* dev = g_devs[d].get();
            while (auto j = loaded.take()) {
                if (g_batch_stop.load()) continue;          // (drain the reader)
                if (!single_tile(cp, j->w, j->h)) { (void)encode_multi_tile(cp, *j, dev); continue; }     // several tiles: the whole file here
                if (gpu_step(cp, *j, dev)) coded.put(std::move(j));
            }
        });
    for (auto& g : gpus) g.join();
    coded.close();
    reader.join();
    writer.join();
    g_batch_done = true;
}

int32_t batch_encode(const char* input_dir, const char* output_dir, gra_cparameters* cp, gra_encode_callback cb)
{
    if (!g_ctx || !input_dir || !output_dir || !cp || !cb) return -1;
    if (!g_batch_done.load()) return -1;
    if (g_batch.joinable()) g_batch.join();
    g_batch_done = false; g_batch_stop = false;
    const std::string in(input_dir), out(output_dir);
    g_batch = std::thread([in, out, cp, cb]() { batch_encode_thread(in, out, cp, cb); });
    return 0;
}

void stop_batch_encode()
{
    g_batch_stop = true;
    if (g_batch.joinable()) g_batch.join();
    g_batch_done = true;
}

bool batch_encode_done() { return g_batch_done.load(); }

} // namespace plugin
