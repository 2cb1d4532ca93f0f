// grok_amd/csrc/plugin_decode.cpp -- the decode side of libgrokj2k_plugin.so: the host's main header -> grk_amd_tile_params, one
// file through Grok's decode protocol stage by stage, the batch thread and its counters.
#include "plugin_internal.h"
#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <thread>

namespace plugin {

static DecodeCallbackInfo make_decode_info(void* params, const char* in_path, const char* out_path, uint32_t flags)
{
    DecodeCallbackInfo info;
    std::memset(&info.header_info, 0, sizeof(info.header_info));
    info.decompressor_parameters = params;
    if (in_path) info.inputFile = in_path;
    if (out_path) info.outputFile = out_path;
    info.decompress_flags = flags;
    return info;
}

static void send_clean(DecodeUserCallback cb, DecodeCallbackInfo& info)
{
    info.decompress_flags = GRA_PLUGIN_DECODE_CLEAN;
    (void)cb(&info);
}

static gra_header_info g_dec_header;           // what the host's header parser told init_decompressors_func
static gra_image* g_dec_image = nullptr;
static int dec_init_decompressors(gra_header_info* h, gra_image* img)
{
    if (!h || !img) return 1;
    g_dec_header = *h;
    g_dec_image = img;
    return 0;
}

// the host's component is the rectangle p covers at 1 / 2^reduce of its size (with an origin off the 2^reduce grid the host's reduced
// header can size a component one column / row larger, SIZMarker.cpp:54: such a component is left to the host)
static bool reduced_matches(const grk_amd_tile_params& p, uint32_t reduce, const gra_image_comp& ck)
{
    uint32_t x0, y0, w, h;
    if (grk_amd_reduced_tile_rect(&p, reduce, &x0, &y0, &w, &h) != GRK_AMD_OK) return false;
    return ck.w == w && ck.h == h && (!reduce || (ck.x0 == x0 && ck.y0 == y0));
}

bool tile_params_from_header(const gra_header_info& h, const gra_image* img, uint32_t reduce, HeaderTile& t)
{
    // grk_decompress -r N (cp_reduce): the host reports its components at the reduced size, but its tile -- the tree its Tier-2
    // synch walks, plugin_bridge.cpp:24-80 -- keeps every resolution.  The tree is therefore the FULL tile's, from the image
    // bounds on the reference grid, and the decode returns it reduced (grk_amd_set_decode_reduce).  N >= numresolutions is refused
    // by the host itself (CodeStreamDecompress.cpp:1604)
    if (reduce >= h.numresolutions) return false;
    // the scope of the hot path: one tile (anywhere on the canonical grid), equal full-resolution components, one
    // layer, one codeword segment per block (the host's bridge throws on more); irreversible only for classic
    // blocks (the reference's own HT + 9/7 encoder is broken, D1: there is no stream to be compatible with)
    if (h.t_grid_width * h.t_grid_height != 1 || img->numcomps == 0 ||
        (h.irreversible && (h.cblk_sty & 0x40u)) || (h.cblk_sty & 0x05u) || h.numresolutions == 0)
        return false;
    const gra_image_comp& c0 = img->comps[0];
    // Components: one precision and signedness; sub-sampled components (SIZ XRsiz / YRsiz) as they come -- all alike (every
    // component then is the same w x h rectangle at ceil(offset / d): one geometry) or each in its own way (4:2:0 ...: every
    // component its own tile-component, the tree built per component, runs of equal factors decoded together)
    t = HeaderTile{};
    bool& alike = t.alike;
    for (uint16_t k = 0; k < img->numcomps; ++k) {
        const gra_image_comp& ck = img->comps[k];
        if (ck.dx < 1 || ck.dy < 1 || ck.dx > 255 || ck.dy > 255 || ck.w == 0 || ck.h == 0 || ck.prec != c0.prec || ck.sgnd != c0.sgnd || ck.prec > 16)
            return false;
        alike = alike && ck.dx == c0.dx && ck.dy == c0.dy && ck.w == c0.w && ck.h == c0.h && ck.x0 == c0.x0 && ck.y0 == c0.y0;
    }
    if (!alike && img->numcomps > 4) return false;
    grk_amd_tile_params& tp = t.tp;
    // alike: the tile IS the component rectangle; else: the tile on the reference grid, the components derived from it
    tp.tile_w = alike ? c0.w : img->x1 - img->x0; tp.tile_h = alike ? c0.h : img->y1 - img->y0; tp.num_comps = img->numcomps;
    tp.tile_x0 = alike ? c0.x0 : img->x0; tp.tile_y0 = alike ? c0.y0 : img->y0;
    if (reduce && alike) {                                // the full component rectangle: ceil(image bounds / d)
        const uint32_t x0 = (uint32_t)(((uint64_t)img->x0 + c0.dx - 1) / c0.dx), x1 = (uint32_t)(((uint64_t)img->x1 + c0.dx - 1) / c0.dx);
        const uint32_t y0 = (uint32_t)(((uint64_t)img->y0 + c0.dy - 1) / c0.dy), y1 = (uint32_t)(((uint64_t)img->y1 + c0.dy - 1) / c0.dy);
        if (x1 <= x0 || y1 <= y0) return false;
        tp.tile_x0 = x0; tp.tile_y0 = y0; tp.tile_w = x1 - x0; tp.tile_h = y1 - y0;
    }
    tp.prec = c0.prec; tp.sgnd = c0.sgnd; tp.irreversible = h.irreversible ? 1 : 0; tp.mct = h.mct ? 1 : 0;
    tp.num_levels = (uint8_t)(h.numresolutions - 1);
    tp.cblk_w_exp = (uint8_t)ceil_log2(h.cblockw_init); tp.cblk_h_exp = (uint8_t)ceil_log2(h.cblockh_init);
    if (h.csty & 1u) {                                      // precinct partition: sizes 2^PPx x 2^PPy per resolution (0 = coarsest)
        for (uint32_t r = 0; r < h.numresolutions; ++r) {
            const uint32_t ex = ceil_log2(h.prcw_init[r]), ey = ceil_log2(h.prch_init[r]);
            if (ex > 15 || ey > 15 || (ex | (ey << 4)) == 0) return false;
            tp.precinct_exp[r] = (uint8_t)(ex | (ey << 4));
        }
    }
    tp.reserved[0] = (h.cblk_sty & 0x40u) ? 0 : 1;         // HT bit clear: classic Part-1 blocks
    tp.reserved[1] = h.cblk_sty & 0x3Fu;
    if (alike) return tp.num_levels >= reduce && reduced_matches(tp, reduce, c0);
    if (tp.mct) return false;                             // (a colour transform across component sizes: no encoder writes that)
    t.cps.resize(tp.num_comps);
    for (uint32_t c = 0; c < tp.num_comps; ++c) {
        const gra_image_comp& ck = img->comps[c];
        t.cdx[c] = (uint8_t)ck.dx; t.cdy[c] = (uint8_t)ck.dy;
        if (comp_tile_params(tp, ck.dx, ck.dy, t.cps[c]) != GRK_AMD_OK) return false;
        if (!reduced_matches(t.cps[c], reduce, ck)) return false;      // (the host's component is not the rectangle SIZ implies)
    }
    return true;
}

// band numbps of an HT stream from ITS quantisation marker (reversible: 8-bit exponents; Quantizer.cpp:49-51); none for
// classic blocks
bool band_numbps_from_qcd(const StreamHeader& sh, const grk_amd_tile_params& tp, std::vector<uint8_t>& band_numbps)
{
    band_numbps.clear();
    if (tp.reserved[0]) return true;
    const size_t nbands = 3u * tp.num_levels + 1u;
    if (sh.qstyle != 0 || sh.words.size() < nbands) return false;
    for (size_t b = 0; b < nbands; ++b) {
        const int v = (int)(sh.words[b] >> 3) + (int)sh.guard_bits - 1;
        if (v < 1 || v > 31) return false;
        band_numbps.push_back((uint8_t)v);
    }
    return true;
}

// a tree whose blocks own buffers the host can copy into: nominal block area x 4 bytes, as the host allocates
// for its own code-blocks (t1/T1Structs.cpp:292-307)
// The host copies getSegBuffersLen() bytes into a block's buffer without asking how large it is
// (plugin_bridge.cpp:69-71 copy_to_contiguous_buffer), so a crafted stream that signals a longer block writes past
// its slot.  No block is longer than the file it comes from: a tail of that size behind the last slot keeps every
// such write inside the allocation, and the lengths are checked against the slots after the Tier-2 callback.
static uint64_t slot_bytes(const gra_plugin_code_block& cb) { return (uint64_t)cb.numPix * 4u + 16u; }
static bool prepare_slots(TileOwner* owner, uint64_t tail)
{
    uint64_t cap = 0;
    for (size_t i = 0; i < owner->blocks.size(); ++i) {
        owner->table[i].offset = cap; owner->table[i].length = 0; owner->table[i].missing_msbs = 0;
        cap += slot_bytes(owner->blocks[i]);
    }
    if (!owner->ensure_coded(g_ctx, cap + tail)) return false;
    std::memset(owner->coded, 0, cap + tail);
    patch_owner(owner);
    for (auto* b : owner->block_ptr) { b->numBitPlanes = 0; b->numPasses = 0; }
    return true;
}
static bool slots_hold(const TileOwner* owner)
{
    for (const gra_plugin_code_block& cb : owner->blocks)
        if (cb.compressedDataLength > slot_bytes(cb)) return false;       // overran its slot: the CPU decoder takes it
    return true;
}

// the decoded planes, tight and back to back, into the host's image
static bool store_planes(gra_image* img, const uint8_t* px, const std::vector<size_t>& plane_at, const std::vector<uint32_t>& plane_w,
                         const std::vector<uint32_t>& plane_h, size_t bps, bool sgnd)
{
    for (uint16_t k = 0; k < img->numcomps; ++k) {
        gra_image_comp& ck = img->comps[k];
        if (ck.w != plane_w[k] || ck.h != plane_h[k]) return false;
        const uint32_t pw = plane_w[k];
        if (!ck.data) {                                   // the host skipped post-T1, so nothing was allocated
            ck.stride = (ck.w + 31u) & ~31u;
            void* mem = nullptr;
            if (posix_memalign(&mem, 64, (size_t)ck.stride * ck.h * sizeof(int32_t)) != 0) return false;
            ck.data = static_cast<int32_t*>(mem);         // freed by the host with the image (grk_aligned_free = free)
        }
        for (uint32_t y = 0; y < ck.h; ++y) {
            int32_t* dst = ck.data + (size_t)y * ck.stride;
            const uint8_t* src = px + plane_at[k] + (size_t)y * pw * bps;
            for (uint32_t x = 0; x < ck.w; ++x) {
                if (bps == 1) dst[x] = sgnd ? (int32_t)(int8_t)src[x] : (int32_t)src[x];
                else { uint16_t v; std::memcpy(&v, src + 2 * x, 2); dst[x] = sgnd ? (int32_t)(int16_t)v : (int32_t)v; }
            }
        }
    }
    return true;
}

// one file's way through the protocol: whatever stage it ends at, the tree goes back and the host gets its clean-up stage
namespace {
struct DecodeSession {
    DecodeUserCallback cb;
    DecodeCallbackInfo info;
    TileOwner* owner = nullptr;
    ~DecodeSession() { if (owner) grk_amd_plugin_tile_destroy(&owner->tile); send_clean(cb, info); }
};
}

// stages 2-4 of decompress_file: the Tier-2 callback over the tree, the GPU decode, the pixels, the post-T1 callback
static bool decode_stages(DecodeSession& s, const HeaderTile& t, const StreamHeader& sh, gra_image* img, uint32_t reduce)
{
    const grk_amd_tile_params& tp = t.tp;
    std::vector<uint8_t> band_numbps;
    if (!band_numbps_from_qcd(sh, tp, band_numbps)) return false;
    s.owner = t.alike ? acquire_owner(tp) : make_owner(tp, &t.cps);
    if (!s.owner) return false;
    s.owner->served_decode = true; s.owner->no_cache = !t.alike;
    if (!prepare_slots(s.owner, sh.file_size + 64)) return false;
    gra_plugin_tile* tree = &s.owner->tile;
    s.info.tile = tree;
    // T2 alone cannot be asked for: without GRK_DECODE_POST_T1 the host never advances to the next tile-part
    // (CodeStreamDecompress.cpp:968-973 skips findNextTile) and its tile loop then fails with "no SOT marker found"
    // (:452-461, :2076) AFTER Tier-2 and the synch have run -- reference defect D11.  With POST_T1 set the host also
    // runs its inverse MCT + DC shift over the (empty) tile buffers and hands them to the image (cheap next to T1 and
    // the DWT, which stay skipped: TileProcessor.cpp:786-818); the pixels are overwritten below.
    s.info.decompress_flags = GRA_DECODE_T2 | GRA_DECODE_POST_T1;
    tree->decompress_flags = GRA_DECODE_T2 | GRA_DECODE_POST_T1;
    if (s.cb(&s.info) != 0 || !slots_hold(s.owner)) return false;
    const size_t bps = (tp.prec + 7u) / 8u;
    std::vector<size_t> plane_at(tp.num_comps + 1u, 0);
    std::vector<uint32_t> plane_w(tp.num_comps), plane_h(tp.num_comps);      // the decoded (reduced) components
    for (uint32_t c = 0; c < tp.num_comps; ++c) {
        uint32_t rx0, ry0;
        if (grk_amd_reduced_tile_rect(t.alike ? &tp : &t.cps[c], reduce, &rx0, &ry0, &plane_w[c], &plane_h[c]) != GRK_AMD_OK) return false;
        plane_at[c + 1] = plane_at[c] + (size_t)plane_w[c] * plane_h[c] * bps;
    }
    std::vector<uint8_t> px(plane_at[tp.num_comps]);
    const uint8_t* const bn = band_numbps.empty() ? nullptr : band_numbps.data();
    const int drc = t.alike ? decode_tree_comps(g_ctx, &tp, tree, 0, bn, (uint32_t)band_numbps.size(), reduce, px.data(), 0)
                            : decode_tree_subsampled(g_ctx, &tp, t.cdx, t.cdy, tree, bn, (uint32_t)band_numbps.size(), reduce, px.data());
    if (drc != GRK_AMD_OK) return false;
    if (!store_planes(s.info.image ? s.info.image : img, px.data(), plane_at, plane_w, plane_h, bps, tp.sgnd != 0)) return false;
    s.info.decompress_flags = GRA_DECODE_POST_T1;
    tree->decompress_flags = GRA_DECODE_POST_T1;
    const int32_t rc = s.cb(&s.info);
    s.info.tile = nullptr;
    return rc == 0;
}

// The plugin side of Grok's decode protocol (grk_decompress.cpp:792-1008 is the host side):
//   1. GRK_DECODE_HEADER: the host opens the stream, reads the main header and calls init_decompressors_func
//   2. GRK_DECODE_T2 with our tile tree attached: the host runs Tier-2 and decompress_synch_plugin_with_host copies
//      every code-block's bytes, numbps and pass count into the tree (plugin_bridge.cpp:24-80); T1 and everything
//      after it are skipped on the host (TileProcessor.cpp:786-789, CodeStreamDecompress.cpp:935-936)
//   3. block decode, inverse DWT, inverse MCT on the GPU; the pixels go into the host's grk_image
//   4. GRK_DECODE_POST_T1: the host stores the image;  5. GRK_PLUGIN_DECODE_CLEAN
// Anything outside the hot path's scope is declined (non-zero) and the host decodes on its CPU.
// in_path / out_path: batch mode -- the host's callback takes them as input_file_name / output_file_name (grok.cpp:698-725),
// otherwise it reads parameters->infile / outfile
int32_t decompress_file(void* params, DecodeUserCallback cb, const char* in_path, const char* out_path)
{
    if (!g_ctx || !cb) return -1;
    std::lock_guard<std::mutex> lk(g_mu);
    DecodeSession s{cb, make_decode_info(params, in_path, out_path, GRA_DECODE_HEADER)};
    s.info.init_decompressors_func = dec_init_decompressors;
    g_dec_image = nullptr;
    if (cb(&s.info) != 0 || !g_dec_image) return -1;
    // the stream's main header, from the file the host was pointed at (grk_decompress -i: parameters->infile,
    // grk_decompress.cpp:552).  A host that decodes from memory gives us nothing to read it from: declined.
    StreamHeader sh;
    const gra_decompress_parameters_head* dp = static_cast<const gra_decompress_parameters_head*>(params);
    const char* path = in_path ? in_path : !dp ? nullptr : dp->infile[0] ? dp->infile : dp->core.infile[0] ? dp->core.infile : nullptr;
    if (!path || !read_stream_header(path, sh) || sh.overrides) return -1;
    const uint32_t reduce = dp ? dp->core.cp_reduce : 0;
    HeaderTile t;
    if (!tile_params_from_header(g_dec_header, g_dec_image, reduce, t)) return -1;
    return decode_stages(s, t, sh, g_dec_image, reduce) ? 0 : -1;
}

// ---- batch decode (plugin/plugin_interface.h:131-143; the host side: grk_decompress.cpp:874-900): a worker thread walks the
//      input directory; a stream outside the hot path's scope is handed back to the host's own decoder in the same callback
//      protocol (all stages in one call, grok.h:1254 GRK_DECODE_ALL), so that every file of the directory comes out
static std::thread g_dbatch;
static std::atomic<bool> g_dbatch_done{true}, g_dbatch_stop{false};
static std::atomic<int> g_dbatch_gpu{0}, g_dbatch_cpu{0}, g_dbatch_failed{0};
static struct { std::string in, out; void* params = nullptr; DecodeUserCallback cb = nullptr; } g_dbatch_job;

static void batch_decompress_thread()
{
    const auto job = g_dbatch_job;
    const auto* dp = static_cast<const gra_decompress_parameters_head*>(job.params);
    std::vector<std::string> names = list_files(job.in, kStreamExtensions);
    std::sort(names.begin(), names.end());
    for (const auto& name : names) {
        if (g_dbatch_stop.load()) break;
        const std::string src = job.in + "/" + name;
        const std::string dst = job.out + "/" + name.substr(0, name.rfind('.')) + out_extension(dp->cod_format);
        if (decompress_file(job.params, job.cb, src.c_str(), dst.c_str()) == 0) { ++g_dbatch_gpu; continue; }
        // outside the hot path: the host decodes this one itself, all stages in one call
        DecodeCallbackInfo info = make_decode_info(job.params, src.c_str(), dst.c_str(),
                                                   GRA_DECODE_HEADER | GRA_DECODE_T2 | GRA_DECODE_T1 | GRA_DECODE_POST_T1);
        const int32_t rc = job.cb(&info);
        send_clean(job.cb, info);
        if (rc == 0) ++g_dbatch_cpu; else ++g_dbatch_failed;
    }
    g_dbatch_done = true;
}

int32_t init_batch_decompress(const char* input_dir, const char* output_dir, void* params, DecodeUserCallback cb)
{
    if (!g_ctx || !input_dir || !output_dir || !params || !cb) return -1;
    if (!g_dbatch_done.load()) return -1;
    if (g_dbatch.joinable()) g_dbatch.join();
    g_dbatch_job.in = input_dir; g_dbatch_job.out = output_dir; g_dbatch_job.params = params;
    g_dbatch_job.cb = cb;
    return 0;
}

int32_t batch_decompress()
{
    if (!g_ctx || !g_dbatch_job.cb || !g_dbatch_done.load()) return -1;
    if (g_dbatch.joinable()) g_dbatch.join();
    g_dbatch_done = false; g_dbatch_stop = false;
    g_dbatch_gpu = 0; g_dbatch_cpu = 0; g_dbatch_failed = 0;
    g_dbatch = std::thread([]() { batch_decompress_thread(); });
    return 0;
}

void stop_batch_decompress()
{
    g_dbatch_stop = true;
    if (g_dbatch.joinable()) g_dbatch.join();
    g_dbatch_done = true;
}

bool batch_decompress_done() { return g_dbatch_done.load(); }

} // namespace plugin
using namespace plugin;

// layout facts of the C++ callback record for the ABI check (oracle/ref_harness/abi_check.cpp, tests)
extern "C" GRA_EXPORT size_t grk_amd_plugin_decode_info_layout(int which)
{
    typedef DecodeCallbackInfo I;
    static const size_t at[15] = {sizeof(I), offsetof(I, init_decompressors_func), offsetof(I, inputFile), offsetof(I, outputFile),
                                  offsetof(I, decod_format), offsetof(I, stream), offsetof(I, codec), offsetof(I, decompressor_parameters),
                                  offsetof(I, header_info), offsetof(I, image), offsetof(I, plugin_owns_image), offsetof(I, tile),
                                  offsetof(I, error_code), offsetof(I, decompress_flags), offsetof(I, user_data)};
    return which >= 0 && which < 15 ? at[which] : 0;
}

// how the last decode batch went: files decoded on the GPU, handed back to the host's decoder, failed
GRA_EXPORT void grk_amd_plugin_batch_decode_counts(int32_t* gpu, int32_t* cpu, int32_t* failed)
{
    if (gpu) *gpu = g_dbatch_gpu.load();
    if (cpu) *cpu = g_dbatch_cpu.load();
    if (failed) *failed = g_dbatch_failed.load();
}
