// grok_amd/csrc/plugin_tile.cpp -- the grk_plugin_tile tree of libgrokj2k_plugin.so: built from the geometry functions of
// libgrok_amd.so, kept per geometry, filled by an encode or walked by a decode; and the library-level drop-in calls
// grk_amd_plugin_tile_* of include/grk_plugin_abi.h on top of it.
#include "plugin_internal.h"
#include <algorithm>
#include <cstdlib>

namespace plugin {

// ---- the tile tree ------------------------------------------------------------------------------
// 49 152 blocks of an 8K frame are 82 MB of gra_plugin_code_block: allocating, zeroing and filling that per frame (and as much
// again for the coded bytes) cost more than the transfers.  A tree is therefore built once per geometry and kept (a few per
// geometry: the batch pipeline holds up to three tiles at a time); a frame patches the three per-block fields that change.
// The coded bytes live in pinned memory (grk_amd_host_alloc): the download is one DMA at the link's rate.
static_assert(offsetof(TileOwner, tile) == 0, "tile must be the first member: destroy() casts back");

static void free_bytes(uint8_t* p, bool pinned) { if (p) { if (pinned) grk_amd_host_free(nullptr, p); else std::free(p); } }

void TileOwner::free_coded()
{
    free_bytes(coded, coded_pinned);
    coded = nullptr; coded_cap = 0;
}

bool TileOwner::ensure_coded(grk_amd_ctx* ctx, size_t n, size_t keep)
{
    if (n <= coded_cap) return true;
    uint8_t* const old = keep ? coded : nullptr;
    const bool old_pinned = coded_pinned;
    if (old) coded = nullptr;
    free_coded();
    const size_t want = n + (n >> 3) + 4096;
    coded = static_cast<uint8_t*>(grk_amd_host_alloc(ctx, want));
    coded_pinned = coded != nullptr;
    if (!coded) coded = static_cast<uint8_t*>(std::malloc(want));
    if (coded) { coded_cap = want; if (old) std::memcpy(coded, old, keep); }
    free_bytes(old, old_pinned);
    return coded != nullptr;
}

static std::mutex g_cache_mu;
static std::vector<TileOwner*> g_tile_cache;           // trees not in use, any geometry
constexpr size_t kTileCacheMax = 8;
constexpr size_t kTileCacheBytes = 512u << 20;   // pinned coded buffers the kept trees may hold together

grk_amd_image_layout tile_as_image(const grk_amd_tile_params& p)
{
    return grk_amd_image_layout{p.tile_x0, p.tile_y0, p.tile_x0 + p.tile_w, p.tile_y0 + p.tile_h, p.tile_x0, p.tile_y0, p.tile_w, p.tile_h};
}

int comp_tile_params(const grk_amd_tile_params& p, uint32_t dx, uint32_t dy, grk_amd_tile_params& out)
{
    const grk_amd_image_layout tile = tile_as_image(p);
    const int rc = grk_amd_layout_tile_comp(&tile, &p, dx, dy, 0, &out);
    out.num_comps = 1; out.mct = 0;
    return rc;
}

bool tree_layout(const grk_amd_tile_params& p, const std::vector<grk_amd_tile_params>* comp_params, TreeLayout& t)
{
    if (comp_params && comp_params->size() != p.num_comps) return false;
    t.blocks.clear();
    t.nprec = std::vector<std::vector<uint32_t>>(p.num_comps, std::vector<uint32_t>((size_t)p.num_levels + 1u, 1u));
    // (components of one geometry: one call lays all of them out, block.comp set)
    for (uint32_t c = 0; c < (comp_params ? p.num_comps : 1u); ++c) {
        const grk_amd_tile_params& pc = comp_params ? (*comp_params)[c] : p;
        const int64_t nbl = grk_amd_tile_num_blocks(&pc);
        if (nbl <= 0) return false;
        const size_t at = t.blocks.size();
        t.blocks.resize(at + (size_t)nbl);
        if (grk_amd_tile_layout(&pc, t.blocks.data() + at, (uint64_t)nbl, nullptr) != nbl) return false;
        if (comp_params) for (size_t i = at; i < t.blocks.size(); ++i) t.blocks[i].comp = (uint16_t)c;
    }
    for (uint32_t c = 0; c < p.num_comps; ++c) (void)grk_amd_tile_precincts(comp_params ? &(*comp_params)[c] : &p, t.nprec[c].data());
    return true;
}

// the geometry-dependent part of the tree: everything but compressedData / compressedDataLength / passes[0] of the blocks
TileOwner* make_owner(const grk_amd_tile_params& p, const std::vector<grk_amd_tile_params>* comp_params)
{
    TreeLayout tl;
    if (!tree_layout(p, comp_params, tl)) return nullptr;
    const std::vector<grk_amd_block>& layout = tl.blocks;
    const uint32_t nres = p.num_levels + 1u;
    auto* o = new TileOwner();
    o->params = p;
    const size_t nb = layout.size();
    o->table.resize(nb);
    const size_t nbands_c = 3 * p.num_levels + 1;
    o->comps.resize(p.num_comps); o->comp_ptr.resize(p.num_comps);
    o->ress.resize((size_t)p.num_comps * nres); o->res_ptr.resize(o->ress.size());
    o->bands.resize((size_t)p.num_comps * nbands_c); o->band_ptr.resize(o->bands.size());
    // precincts per band of every resolution (the same for its three bands)
    size_t total_prec = 0;
    for (auto& v : tl.nprec)
        for (uint32_t r = 0; r < nres; ++r) {
            v[r] = std::max(v[r], 1u);                  // (a resolution without samples: the host's tree has none either,
                                                        //  one empty entry keeps the arrays well-formed)
            total_prec += (size_t)v[r] * (r ? 3 : 1);
        }
    o->precs.resize(total_prec); o->prec_ptr.resize(o->precs.size());
    o->blocks.resize(nb); o->block_ptr.resize(nb);     // (value-initialised: zeros)
    for (size_t i = 0; i < nb; ++i) {
        const grk_amd_block& b = layout[i];
        gra_plugin_code_block& cb = o->blocks[i];
        cb.x0 = b.x0; cb.y0 = b.y0; cb.x1 = b.x1; cb.y1 = b.y1;
        cb.numPix = (b.x1 - b.x0) * (b.y1 - b.y0);
        cb.numBitPlanes = 1;                     // T1HT::compress sets cblk->numbps = 1 (T1HT.cpp:123)
        cb.numPasses = 1;
        cb.passes[0].distortionDecrease = 0.0;
        o->block_ptr[i] = &cb;
    }
    size_t bi = 0, blk = 0, pk = 0;
    for (uint32_t c = 0; c < p.num_comps; ++c) {
        const std::vector<uint32_t>& nprec = tl.nprec[c];
        gra_plugin_tile_component& tc = o->comps[c];
        tc.numResolutions = nres;
        tc.resolutions = &o->res_ptr[(size_t)c * nres];
        o->comp_ptr[c] = &tc;
        for (uint32_t r = 0; r < nres; ++r) {
            gra_plugin_resolution& R = o->ress[(size_t)c * nres + r];
            o->res_ptr[(size_t)c * nres + r] = &R;
            R.level = r;
            R.numBands = r ? 3 : 1;
            R.band = &o->band_ptr[bi];
            for (size_t k = 0; k < R.numBands; ++k, ++bi) {
                gra_plugin_band& B = o->bands[bi];
                o->band_ptr[bi] = &B;
                const uint8_t orient = (uint8_t)(r ? k + 1 : 0);
                B.orientation = orient;
                B.numPrecincts = nprec[r];
                B.precincts = &o->prec_ptr[pk];
                // the blocks of a band are contiguous in enumeration order, precinct by precinct
                const size_t band_first = blk;
                for (uint32_t q = 0; q < nprec[r]; ++q, ++pk) {
                    o->prec_ptr[pk] = &o->precs[pk];
                    const size_t first = blk;
                    while (blk < nb && layout[blk].comp == c && layout[blk].res == r && layout[blk].band == orient && layout[blk].precinct == q) ++blk;
                    o->precs[pk].numBlocks = blk - first;
                    o->precs[pk].blocks = first < nb ? &o->block_ptr[first] : nullptr;
                }
                B.stepsize = blk > band_first ? layout[band_first].stepsize : 1.0f;
            }
        }
    }
    o->tile.decompress_flags = 0;
    o->tile.numComponents = p.num_comps;
    o->tile.tileComponents = o->comp_ptr.data();
    o->band_steps.resize(o->bands.size());
    for (size_t i = 0; i < o->bands.size(); ++i) o->band_steps[i] = o->bands[i].stepsize;
    return o;
}

// what a frame changes: where each block's bytes are and how many
void patch_owner(TileOwner* o)
{
    const size_t nb = o->blocks.size();
    // (a tree that served a decode comes back with the step sizes the host wrote, plugin_bridge.cpp:40)
    for (size_t i = 0; i < o->bands.size() && i < o->band_steps.size(); ++i) o->bands[i].stepsize = o->band_steps[i];
    o->tile.decompress_flags = 0;
    for (size_t i = 0; i < nb; ++i) {
        gra_plugin_code_block& cb = o->blocks[i];
        const uint32_t len = o->table[i].length;
        cb.compressedData = o->coded + o->table[i].offset;
        cb.compressedDataLength = len;
        cb.numBitPlanes = 1;                            // (a tree that served a decode comes back with the host's values)
        cb.numPasses = 1;
        cb.passes[0].rate = len ? len - 1 : 0;          // host uses rate + 1 (plugin_bridge.cpp:230)
        cb.passes[0].length = len;
        cb.passes[0].distortionDecrease = 0.0;          // (grk_amd_plugin_tile_fill_distortion: only when the host makes layers)
    }
}

TileOwner* acquire_owner(const grk_amd_tile_params& p)
{
    {
        std::lock_guard<std::mutex> lk(g_cache_mu);
        for (size_t i = 0; i < g_tile_cache.size(); ++i)
            if (std::memcmp(&g_tile_cache[i]->params, &p, sizeof p) == 0) {
                TileOwner* o = g_tile_cache[i];
                g_tile_cache.erase(g_tile_cache.begin() + (long)i);
                return o;
            }
    }
    return make_owner(p);
}

void release_owner(TileOwner* o)
{
    if (!o) return;
    if (o->no_cache) { delete o; return; }
    // a decode's buffer (16 KB per block + the file: ~0.8 GB pinned for an 8K frame) does not stay with the kept tree; an encode's
    // (the coded bytes of a frame) does, within a budget over the whole cache
    if (o->served_decode || o->coded_cap > kTileCacheBytes) { o->free_coded(); o->served_decode = false; }
    {
        std::lock_guard<std::mutex> lk(g_cache_mu);
        size_t held = o->coded_cap;
        for (TileOwner* t : g_tile_cache) held += t->coded_cap;
        for (size_t i = 0; held > kTileCacheBytes && i < g_tile_cache.size(); ++i) {          // oldest first
            held -= g_tile_cache[i]->coded_cap;
            g_tile_cache[i]->free_coded();
        }
        if (g_tile_cache.size() < kTileCacheMax) { g_tile_cache.push_back(o); return; }
        // full: the oldest goes (another geometry has taken over)
        TileOwner* old = g_tile_cache.front();
        g_tile_cache.erase(g_tile_cache.begin());
        g_tile_cache.push_back(o);
        o = old;
    }
    delete o;
}

void drop_tile_cache()
{
    std::lock_guard<std::mutex> lk(g_cache_mu);
    for (TileOwner* o : g_tile_cache) delete o;
    g_tile_cache.clear();
}

// host keeps rates in uint16_t (plugin_bridge.cpp:174, D7)
static bool lengths_fit_host(const grk_amd_coded_block* rows, size_t n)
{
    for (size_t i = 0; i < n; ++i)
        if (rows[i].length > 65535) return false;
    return true;
}

int decode_tree_subsampled(grk_amd_ctx* ctx, const grk_amd_tile_params* p, const uint8_t* comp_dx, const uint8_t* comp_dy,
                           const gra_plugin_tile* tile, const uint8_t* band_numbps, uint32_t nbands, uint32_t reduce, void* planes)
{
    if (!ctx || !p || !comp_dx || !comp_dy || !tile || !planes || tile->numComponents != p->num_comps) return GRK_AMD_ERR_INVALID;
    const uint32_t bps = (p->prec + 7u) / 8u;
    size_t at = 0;
    for (const CompRun& run : comp_runs(p->num_comps, p->mct != 0, comp_dx, comp_dy)) {
        grk_amd_tile_params pr;
        int rc = comp_tile_params(*p, comp_dx[run.first], comp_dy[run.first], pr);
        if (rc) return rc;
        pr.num_comps = (uint16_t)run.count;
        pr.mct = run.mct ? 1 : 0;
        if (p->mct && run.first == 0 && !run.mct && p->num_comps >= 3) return GRK_AMD_ERR_UNSUPPORTED;     // (a colour transform across sizes: no encoder writes that)
        rc = decode_tree_comps(ctx, &pr, tile, run.first, band_numbps, nbands, reduce, (uint8_t*)planes + at, 0);
        if (rc) return rc;
        uint32_t rx0, ry0, rw, rh;                       // (each component reduced from its own rectangle)
        rc = grk_amd_reduced_tile_rect(&pr, reduce, &rx0, &ry0, &rw, &rh);
        if (rc) return rc;
        at += (size_t)rw * rh * run.count * bps;
    }
    return GRK_AMD_OK;
}

int decode_tree_comps(grk_amd_ctx* ctx, const grk_amd_tile_params* p, const gra_plugin_tile* tile, uint32_t comp0,
                      const uint8_t* band_numbps, uint32_t nbands, uint32_t reduce, void* pixels, int pixels_on_device)
{
    if (band_numbps && nbands != 3u * p->num_levels + 1u) return GRK_AMD_ERR_INVALID;
    const int64_t nb = grk_amd_tile_num_blocks(p);
    if (nb <= 0) return (int)(nb ? nb : GRK_AMD_ERR_UNSUPPORTED);
    std::vector<grk_amd_block> layout((size_t)nb);
    if (grk_amd_tile_layout(p, layout.data(), (uint64_t)nb, nullptr) != nb) return GRK_AMD_ERR_INVALID;
    if (comp0 + p->num_comps > tile->numComponents) return GRK_AMD_ERR_INVALID;
    // walk the tree in the enumeration order both sides share: comp -> resolution -> band -> precinct -> block
    std::vector<grk_amd_coded_block> table((size_t)nb);
    std::vector<uint8_t> coded;
    std::vector<float> steps;            // irreversible: the bands' step sizes; the host's synch stores half (plugin_bridge.cpp:40)
    size_t i = 0;
    for (uint32_t c = comp0; c < comp0 + p->num_comps; ++c) {
        const gra_plugin_tile_component* tc = tile->tileComponents[c];
        for (uint32_t r = 0; r < tc->numResolutions; ++r) {
            const gra_plugin_resolution* res = tc->resolutions[r];
            for (uint32_t b = 0; b < res->numBands; ++b) {
                const gra_plugin_band* band = res->band[b];
                steps.push_back(band->stepsize * 2.0f);
                for (uint64_t pr = 0; pr < band->numPrecincts; ++pr) {
                    const gra_plugin_precinct* prec = band->precincts[pr];
                    for (uint64_t k = 0; k < prec->numBlocks; ++k) {
                        if (i >= (size_t)nb) return GRK_AMD_ERR_INVALID;
                        const gra_plugin_code_block* cb = prec->blocks[k];
                        grk_amd_coded_block& row = table[i];
                        row.offset = coded.size();
                        row.length = cb->compressedData ? cb->compressedDataLength : 0;
                        const uint32_t nbp = (uint32_t)cb->numBitPlanes;
                        if (p->reserved[0]) row.missing_msbs = row.length ? (nbp | ((uint32_t)cb->numPasses << 8)) : 0;
                        else {                                                // band numbps - block numbps
                            const uint32_t bn = band_numbps ? band_numbps[layout[i].res ? 3u * layout[i].res - 2u + (layout[i].band - 1u) : 0u]
                                                            : layout[i].kmax;
                            if (row.length && nbp > bn) return GRK_AMD_ERR_INVALID;
                            row.missing_msbs = row.length ? bn - nbp : 0;
                        }
                        if (row.length) coded.insert(coded.end(), cb->compressedData, cb->compressedData + row.length);
                        coded.resize((coded.size() + 15u) & ~(size_t)15u);
                        ++i;
                    }
                }
            }
        }
    }
    if (i != (size_t)nb) return GRK_AMD_ERR_INVALID;
    coded.resize(coded.size() + 16);
    if (p->irreversible && grk_amd_set_decode_steps(ctx, steps.data(), (uint32_t)steps.size()) != GRK_AMD_OK) return GRK_AMD_ERR_INVALID;
    // (the tree is the full tile's; reduce > 0: the tile at 1 / 2^reduce of its size, the setting reset afterwards)
    int rc = grk_amd_set_decode_reduce(ctx, reduce);
    if (rc == GRK_AMD_OK) rc = grk_amd_decode_tiles(ctx, p, 1, table.data(), coded.data(), coded.size(), 0, pixels, pixels_on_device);
    (void)grk_amd_set_decode_reduce(ctx, 0);
    if (p->irreversible) (void)grk_amd_set_decode_steps(ctx, nullptr, 0);
    return rc;
}

} // namespace plugin
using namespace plugin;

// ---- the exported calls (declared extern "C" in include/grk_plugin_abi.h) ---------------------------

GRA_EXPORT gra_plugin_tile* grk_amd_plugin_tile_create(grk_amd_ctx* ctx, const grk_amd_tile_params* p,
                                                       const void* pixels, int on_device)
{
    if (!ctx || !p || !pixels) return nullptr;
    TileOwner* o = acquire_owner(*p);            // a kept tree of this geometry, or a new one
    if (!o) return nullptr;
    uint64_t total = 0;
    bool ok = grk_amd_encode_tiles(ctx, p, 1, pixels, on_device, o->table.data(), &total) == GRK_AMD_OK;
    ok = ok && lengths_fit_host(o->table.data(), o->table.size());
    ok = ok && o->ensure_coded(ctx, total ? total : 1);
    ok = ok && (!total || grk_amd_fetch_coded(ctx, o->coded, total) == GRK_AMD_OK);      // (pinned: one DMA)
    if (!ok) { release_owner(o); return nullptr; }
    patch_owner(o);
    return &o->tile;
}

// The library-level drop-in for an image whose components are sub-sampled each in its own way (4:2:0 ...): `p` = the tile on the
// REFERENCE grid (tile_x0 / tile_y0 / tile_w / tile_h), component c = [ceil(x0 / dx_c), ceil(x1 / dx_c)) x ... of its own samples
// (tile/TileProcessor.cpp:605-612), `planes` = the components back to back, each tight at its own size.  Runs of consecutive
// components with equal factors are coded together (MCT only for a run that holds components 0..2, else off as the reference has it:
// CodeStreamCompress.cpp:434-447); the tree carries every component's own resolutions / precincts / blocks.
GRA_EXPORT gra_plugin_tile* grk_amd_plugin_tile_create_subsampled(grk_amd_ctx* ctx, const grk_amd_tile_params* p, const uint8_t* comp_dx,
                                                                 const uint8_t* comp_dy, const void* planes)
{
    if (!ctx || !p || !comp_dx || !comp_dy || !planes || p->num_comps == 0) return nullptr;
    const uint32_t nc = p->num_comps, bps = (p->prec + 7u) / 8u;
    std::vector<grk_amd_tile_params> cps(nc);
    std::vector<size_t> plane_at(nc + 1, 0);
    for (uint32_t c = 0; c < nc; ++c) {
        if (comp_tile_params(*p, comp_dx[c], comp_dy[c], cps[c]) != GRK_AMD_OK) return nullptr;
        plane_at[c + 1] = plane_at[c] + (size_t)cps[c].tile_w * cps[c].tile_h * bps;
    }
    TileOwner* o = make_owner(*p, &cps);           // (not cached: the cache is keyed by the tile's parameters alone)
    if (!o) return nullptr;
    bool ok = true;
    size_t row = 0;
    uint64_t used = 0;
    for (const CompRun& run : comp_runs(p->num_comps, p->mct != 0, comp_dx, comp_dy)) {
        grk_amd_tile_params pr = cps[run.first];
        pr.num_comps = (uint16_t)run.count; pr.mct = run.mct ? 1 : 0;
        const int64_t nbl = grk_amd_tile_num_blocks(&pr);
        uint64_t total = 0;
        ok = nbl > 0 && row + (size_t)nbl <= o->table.size() &&
             grk_amd_encode_tiles(ctx, &pr, 1, (const uint8_t*)planes + plane_at[run.first], 0, o->table.data() + row, &total) == GRK_AMD_OK &&
             lengths_fit_host(o->table.data() + row, (size_t)nbl);
        if (!ok) break;
        // (the bytes of the runs one behind the other: a run's encode reuses the context's arena)
        for (size_t i = row; i < row + (size_t)nbl; ++i) o->table[i].offset += used;
        if (total) {
            if (used + total > o->coded_cap) ok = o->ensure_coded(ctx, (used + total) * 2, used);
            ok = ok && grk_amd_fetch_coded(ctx, o->coded + used, total) == GRK_AMD_OK;
        }
        if (!ok) break;
        used += total; row += (size_t)nbl;
    }
    ok = ok && row == o->table.size() && (o->coded || o->ensure_coded(ctx, 1));
    if (!ok) { delete o; return nullptr; }
    patch_owner(o);
    o->no_cache = true;                            // (release_owner: the cache is keyed by the tile's parameters alone)
    return &o->tile;
}

GRA_EXPORT int grk_amd_plugin_tile_fill_distortion(grk_amd_ctx* ctx, gra_plugin_tile* tile)
{
    if (!ctx || !tile) return GRK_AMD_ERR_INVALID;
    TileOwner* o = reinterpret_cast<TileOwner*>(tile);
    std::vector<double> dd(o->blocks.size());
    const int rc = grk_amd_block_distortion(ctx, dd.data(), dd.size());
    if (rc) return rc;
    for (size_t i = 0; i < dd.size(); ++i) o->blocks[i].passes[0].distortionDecrease = dd[i];
    return GRK_AMD_OK;
}

GRA_EXPORT void grk_amd_plugin_tile_destroy(gra_plugin_tile* tile)
{
    release_owner(reinterpret_cast<TileOwner*>(tile));      // kept for the next frame of this geometry
}

GRA_EXPORT int grk_amd_plugin_tile_decode(grk_amd_ctx* ctx, const grk_amd_tile_params* p, const gra_plugin_tile* tile,
                                          void* pixels, int pixels_on_device)
{
    return grk_amd_plugin_tile_decode_qcd(ctx, p, tile, nullptr, 0, pixels, pixels_on_device);
}

GRA_EXPORT int grk_amd_plugin_tile_decode_qcd(grk_amd_ctx* ctx, const grk_amd_tile_params* p, const gra_plugin_tile* tile,
                                              const uint8_t* band_numbps, uint32_t nbands, void* pixels, int pixels_on_device)
{
    if (!ctx || !p || !tile || !pixels) return GRK_AMD_ERR_INVALID;
    if (tile->numComponents != p->num_comps) return GRK_AMD_ERR_INVALID;
    return decode_tree_comps(ctx, p, tile, 0, band_numbps, nbands, 0, pixels, pixels_on_device);
}

// The decode counterpart of grk_amd_plugin_tile_create_subsampled: `p` = the tile on the reference grid, component c of the tree has
// the geometry of [ceil(x0 / dx_c), ceil(x1 / dx_c)) x ...; `planes` receives the components back to back, each tight at its own size.
// Runs of components with equal factors are decoded together (the inverse colour transform only for a run that holds components
// 0..2 of a stream that signals it -- an encoder cannot have applied it across sizes).
GRA_EXPORT int grk_amd_plugin_tile_decode_subsampled(grk_amd_ctx* ctx, const grk_amd_tile_params* p, const uint8_t* comp_dx,
                                                     const uint8_t* comp_dy, const gra_plugin_tile* tile, const uint8_t* band_numbps,
                                                     uint32_t nbands, void* planes)
{
    return decode_tree_subsampled(ctx, p, comp_dx, comp_dy, tile, band_numbps, nbands, 0, planes);
}
