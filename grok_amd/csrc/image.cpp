// grok_amd/csrc/image.cpp -- a whole image of any tile layout through the tile processor (host side, on top of the
// C ABI's own entry points).
//
// grk_amd_encode_tiles codes a batch of tiles that share ONE geometry.  An image whose tile grid does not sit on
// multiples of 2^levels x code-block size -- image offsets (grk_image x0 / y0), tile sizes such as 1000 x 1000, ragged
// last rows and columns -- has tiles of several geometries: sub-band sizes differ by a sample, bands start with partial
// code-blocks, and where a resolution begins on an odd coordinate the lifting starts with a high-pass sample
// (tile/TileProcessor.cpp:100-170 tile rectangle; tile/TileComponent.cpp:131-138 bands; WaveletFwd.cpp:884-905).
// Here the tiles are grouped by geometry, each group goes through grk_amd_encode_tiles as one batch, and the
// tile-parts are written in tile order (codestream/CodeStreamCompress.cpp:535-603); those steps (image.h) serve node.cpp too.
#include "image.h"
#include "context.h"
#include "t2_order.h"
#include "t2_parts.h"
#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

using namespace grk_amd;

extern "C" int grk_amd_same_tile_geometry(const grk_amd_tile_params* a, const grk_amd_tile_params* b)
{
    if (!a || !b) return GRK_AMD_ERR_INVALID;
    TileGeom ga, gb;
    int rc = build_tile_geom(*a, ga); if (rc) return rc;
    rc = build_tile_geom(*b, gb); if (rc) return rc;
    return same_geometry(ga, gb) ? 1 : 0;
}

// ---- the steps of the whole-image encoders (image.h) -------------------------------------------------------------------------
int grk_amd::plain_image(const grk_amd_image_layout* im, const grk_amd_tile_params* base, const void* pixels, uint32_t flags,
                         std::vector<Unit>& units, SourcePlanes& src, UnitGroups& g, const grk_amd_pixel_layout* lay)
{
    const int64_t nt = grk_amd_layout_num_tiles(im);
    if (nt < 0) return (int)nt;
    const uint32_t ntiles = (uint32_t)nt, nc = base->num_comps;
    if ((flags & GRK_AMD_CS_TLM) && ntiles > 255) return GRK_AMD_ERR_UNSUPPORTED;
    const uint64_t W = im->x1 - im->x0, H = im->y1 - im->y0;
    src = SourcePlanes{(const uint8_t*)pixels, (base->prec + 7u) / 8u, {}};
    PixelLayout px;
    const char* why = "";
    if (W >> 32 || H >> 32 || !resolve_pixel_layout(*base, lay, (uint32_t)W, (uint32_t)H, 1, px, &why)) return GRK_AMD_ERR_INVALID;
    src.row_pitch = px.row;
    src.channels = px.lay == 2 ? px.channels : 0;
    for (uint32_t c = 0; c < nc; ++c) src.comp.push_back({c * px.kstep, W, im->x0, im->y0});
    units.assign(ntiles, Unit{{}, 0});
    for (uint32_t t = 0; t < ntiles; ++t) {
        int rc = grk_amd_layout_tile(im, base, t, &units[t].p);
        if (!rc) rc = add_unit(g, units[t].p, (flags >> GRK_AMD_CS_PROG_SHIFT) & 7u);
        if (rc) return rc;
    }
    return GRK_AMD_OK;
}

void grk_amd::stage_units(const SourcePlanes& src, const std::vector<Unit>& units, const std::vector<uint32_t>& idx, uint8_t* dst, uint32_t threads)
{
    const size_t bytes = idx.empty() ? 0 : staged_bytes(src, units[idx[0]]), bps = src.bps;
    const size_t xstep = src.channels ? src.channels * bps : bps;
    (void)parallel_for(threads, threads, [&](size_t j) -> int {
        for (size_t i = 0; i < idx.size(); ++i) {
            const grk_amd_tile_params& q = units[idx[i]].p;
            const size_t y0 = (size_t)q.tile_h * j / threads, y1 = (size_t)q.tile_h * (j + 1) / threads, row = (size_t)q.tile_w * xstep;
            for (uint32_t k = 0; k < (src.channels ? 1u : q.num_comps); ++k) {
                const SourcePlanes::Plane& c = src.comp[units[idx[i]].c0 + k];
                const size_t pitch = src.row_pitch ? src.row_pitch : c.w * bps;
                const uint8_t* from = src.px + c.at + (q.tile_y0 - c.y0) * pitch + (q.tile_x0 - c.x0) * xstep;
                for (size_t y = y0; y < y1; ++y)
                    std::memcpy(dst + i * bytes + ((size_t)k * q.tile_h + y) * row, from + y * pitch, row);
            }
        }
        return GRK_AMD_OK;
    });
}

int grk_amd::encode_groups_host(grk_amd_ctx* ctx, const SourcePlanes& src, const std::vector<Unit>& units, const UnitGroups& g,
                                std::vector<grk_amd_coded_block>& rows, std::vector<uint8_t>& coded)
{
    // unit u's rows start at row_at[u]
    std::vector<uint64_t> row_at(units.size() + 1, 0);
    for (size_t u = 0; u < units.size(); ++u) row_at[u + 1] = row_at[u] + (uint64_t)g.geoms[g.of[u]].blocks_per_comp * units[u].p.num_comps;
    rows.resize(row_at[units.size()]);
    coded.clear();
    std::vector<uint8_t> staging;
    for (size_t k = 0; k < g.members.size(); ++k) {
        const auto& G = g.members[k];
        const grk_amd_tile_params& p = units[G[0]].p;
        staging.resize(staged_bytes(src, units[G[0]]) * G.size());
        stage_units(src, units, G, staging.data(), 1);
        const uint64_t bpu = (uint64_t)g.geoms[k].blocks_per_comp * p.num_comps;
        std::vector<grk_amd_coded_block> table(bpu * G.size());
        uint64_t total = 0;
        int rc = grk_amd_encode_tiles(ctx, &p, (uint32_t)G.size(), staging.data(), 0, table.data(), &total);
        if (rc) return rc;
        const size_t at = coded.size();
        coded.resize(at + total);
        rc = grk_amd_fetch_coded(ctx, coded.data() + at, total);
        if (rc) return rc;
        for (size_t i = 0; i < G.size(); ++i)
            for (uint64_t b = 0; b < bpu; ++b) { rows[row_at[G[i]] + b] = table[i * bpu + b]; rows[row_at[G[i]] + b].offset += at; }
    }
    return GRK_AMD_OK;
}

void grk_amd::planar_rate_call(grk_amd_ctx* ctx, const std::vector<Unit>& units, const SourcePlanes& src, const UnitGroups& g,
                               std::vector<uint8_t>& staging, RateJointCall& call)
{
    for (size_t u = 0; u < units.size(); ++u) call.unit_blocks.push_back((uint64_t)g.geoms[g.of[u]].blocks_per_comp * units[u].p.num_comps);
    for (const std::vector<uint32_t>& G : g.members) call.batches.push_back(RateBatch{units[G[0]].p, G});
    const RateJointCall* const self = &call;
    call.front = [ctx, &units, &src, &staging, self](size_t k, grk_amd_coded_block* table, uint64_t* total) -> int {
        const std::vector<uint32_t>& G = self->batches[k].units;
        staging.resize(staged_bytes(src, units[G[0]]) * G.size());
        stage_units(src, units, G, staging.data(), 1);
        return grk_amd_encode_tiles(ctx, &self->batches[k].p, (uint32_t)G.size(), staging.data(), 0, table, total);
    };
}

int grk_amd::image_division(grk_amd_ctx* c, uint32_t flags, const grk_amd_tile_params* base, uint32_t ntiles)
{
    std::string why;
    const int np = tile_part_count(flags, base->num_levels, base->num_comps, &why);
    if (np < 0) return fail(c, np, why.c_str());
    if (np > 1 && (flags & GRK_AMD_CS_TLM) && (uint64_t)np * ntiles > kMaxTlmEntries)
        return fail(c, GRK_AMD_ERR_UNSUPPORTED, "more tile-parts than one TLM marker segment lists (13 106)");
    return np;
}

int64_t grk_amd::main_header_any(const grk_amd_image_layout* im, const grk_amd_tile_params* base, const uint8_t* comp_dx, const uint8_t* comp_dy,
                                 uint32_t flags, uint32_t ntiles, uint32_t nparts, const uint32_t* tp_bytes, uint8_t* out, uint64_t cap)
{
    if (nparts > 1) {
        const std::vector<uint32_t> per_tile(ntiles, nparts);
        return main_header_parts(im, base, comp_dx, comp_dy, flags, per_tile.data(), tp_bytes, out, cap);
    }
    return comp_dx ? main_header_subsampled(im, base, comp_dx, comp_dy, flags, tp_bytes, out, cap)
                   : grk_amd_write_main_header_layout(im, base, flags, tp_bytes, out, cap);
}

int64_t grk_amd::frame_file(const grk_amd_image_layout* im, const grk_amd_tile_params* base, uint32_t flags,
                            const std::vector<uint32_t>& part_len, uint8_t* out, uint64_t cap,
                            const std::function<int(const std::vector<uint64_t>& at)>& body, const uint8_t* comp_dx, const uint8_t* comp_dy,
                            uint32_t nparts, const uint32_t* tp_bytes)
{
    const int64_t hdr = main_header_any(im, base, comp_dx && comp_dy ? comp_dx : nullptr, comp_dx && comp_dy ? comp_dy : nullptr, flags,
                                        (uint32_t)part_len.size(), nparts, nparts > 1 ? tp_bytes : part_len.data(), out, cap);
    if (hdr < 0) return hdr;
    std::vector<uint64_t> at(part_len.size() + 1, (uint64_t)hdr);
    for (size_t t = 0; t < part_len.size(); ++t) at[t + 1] = at[t] + part_len[t];
    if (at.back() + 2 > cap) return GRK_AMD_ERR_OVERFLOW;
    const int rc = body(at);
    if (rc) return rc;
    uint64_t end = at.back();
    out[end++] = 0xFF; out[end++] = 0xD9;
    return (int64_t)end;
}

extern "C" int64_t grk_amd_encode_image(grk_amd_ctx* ctx, const grk_amd_image_layout* im, const grk_amd_tile_params* base,
                                        const void* pixels, uint32_t flags, uint8_t* out, uint64_t cap)
{
    if (!ctx || !im || !base || !pixels || !out) return GRK_AMD_ERR_INVALID;
    std::vector<Unit> tiles;
    SourcePlanes src;
    UnitGroups g;
    // `pixels` is the whole image in the context's encode layout; the tiles are staged tight in the same kind of layout, and the
    // batches below read them as that
    const grk_amd_pixel_layout whole = ctx->enc_layout;
    int64_t rc = plain_image(im, base, pixels, flags, tiles, src, g, &whole);
    if (rc) return rc;
    KeepLayout staged{ctx->enc_layout, whole};
    ctx->enc_layout = staged_layout(src);
    const uint32_t ntiles = (uint32_t)tiles.size();
    // Tier-2 on the device (grk_amd_assemble_device; GRK_AMD_IMAGE_T2=host: the host writer below, which is also where a layout beyond
    // the device writer's tables goes): every group's finished tile-parts appended in the context's output buffer, then -- their sizes
    // known -- the main header and each tile-part fetched to its place
    // tiles divided into tile-parts (GRK_AMD_CS_TP): what neither route can write is said before any work
    uint32_t nparts = 1;
    { const int np = image_division(ctx, flags, base, ntiles); if (np < 0) return np; nparts = (uint32_t)np; }
    const char* const et2 = std::getenv("GRK_AMD_IMAGE_T2");
    if (!(et2 && std::strcmp(et2, "host") == 0)) {
        std::vector<uint32_t> part_len(ntiles, 0), tp_len((size_t)ntiles * nparts, 0), tpl;
        std::vector<uint64_t> dev_at(ntiles, 0);
        std::vector<uint8_t> staging;
        uint64_t used = 0;
        for (size_t k = 0; k < g.members.size() && rc >= 0; ++k) {
            const auto& G = g.members[k];
            const grk_amd_tile_params& p = tiles[G[0]].p;
            staging.resize(staged_bytes(src, tiles[G[0]]) * G.size());
            stage_units(src, tiles, G, staging.data(), 1);
            rc = grk_amd_encode_tiles(ctx, &p, (uint32_t)G.size(), staging.data(), 0, nullptr, nullptr);
            if (rc < 0) return rc;
            std::vector<uint32_t> lens(G.size());
            rc = grk_amd_assemble_device(ctx, &p, (uint32_t)G.size(), G.data(), flags, used, lens.data());
            if (rc < 0) break;
            for (size_t i = 0; i < G.size(); ++i) { part_len[G[i]] = lens[i]; dev_at[G[i]] = used; used += lens[i]; }
            if (nparts > 1) {           // the parts' lengths for TLM beside the spans
                tpl.resize(G.size() * nparts);
                const int fr = assembled_part_bytes(ctx, (uint32_t)G.size(), tpl.data());
                if (fr) return fr;
                for (size_t i = 0; i < tpl.size(); ++i) tp_len[(size_t)G[i / nparts] * nparts + i % nparts] = tpl[i];
            }
        }
        if (rc >= 0) {
            const int64_t n = frame_file(im, base, flags, part_len, out, cap, [&](const std::vector<uint64_t>& at) -> int {
                for (uint32_t t = 0; t < ntiles; ++t) {
                    // (tile-parts that lie one behind the other on the device as in the file go in one piece)
                    uint32_t t1 = t;
                    uint64_t n = part_len[t];
                    while (t1 + 1 < ntiles && dev_at[t1 + 1] == dev_at[t] + n) { n += part_len[t1 + 1]; ++t1; }
                    const int fr = grk_amd_fetch_assembled(ctx, dev_at[t], n, out + at[t]);
                    if (fr) return fr;
                    t = t1;
                }
                return GRK_AMD_OK;
            }, nullptr, nullptr, nparts, tp_len.data());
            return n;
        }
        if (rc != GRK_AMD_ERR_UNSUPPORTED) return rc;
    }
    std::vector<grk_amd_coded_block> rows;
    std::vector<uint8_t> coded;
    rc = encode_groups_host(ctx, src, tiles, g, rows, coded);
    if (rc) return rc;
    return grk_amd_write_codestream_layout(im, base, rows.data(), coded.data(), flags, out, cap);
}

// ---- sub-sampled components (4:2:2, 4:2:0, ...) ---------------------------------------------------------------------------
// Components of different size are tile-components of different geometry: a RUN of consecutive components with the same factors
// is coded as one unit -- the tile's rectangle in their coordinates, `n` components, the multiple component transform only for a
// run that holds components 0..2 --, the units of all tiles are grouped by geometry, every group is one grk_amd_encode_tiles batch,
// and the codestream writer takes each component with its own geometry (grk_amd_write_codestream_subsampled).
int grk_amd::subsampled_image(grk_amd_ctx* ctx, const grk_amd_image_layout* im, const grk_amd_tile_params* base, const uint8_t* comp_dx,
                              const uint8_t* comp_dy, const void* pixels, std::vector<Unit>& units, SourcePlanes& src, UnitGroups& g)
{
    {   // (components of different sizes have no interleaved form, and the runs are staged as planes)
        const grk_amd_pixel_layout& l = ctx->enc_layout;
        if (l.interleaved || l.channels || l.row_pitch || l.plane_pitch || l.tile_pitch) return GRK_AMD_ERR_UNSUPPORTED;
    }
    const int64_t nt = grk_amd_layout_num_tiles(im);
    if (nt < 0) return (int)nt;
    const uint32_t ntiles = (uint32_t)nt, nc = base->num_comps;
    const uint32_t bps = (base->prec + 7u) / 8u;
    for (uint32_t c = 0; c < nc; ++c) if (!comp_dx[c] || !comp_dy[c]) return GRK_AMD_ERR_INVALID;
    // (MCT over components of different size: switched off, as the reference does with a warning, CodeStreamCompress.cpp:434-447)
    const std::vector<CompRun> runs = comp_runs(nc, base->mct != 0, comp_dx, comp_dy);
    // the image's components in `pixels`: component c is ceil(x1 / dx) - ceil(x0 / dx) columns wide, planes back to back
    auto cdiv = [](uint64_t a, uint64_t b) { return (a + b - 1) / b; };
    src = SourcePlanes{(const uint8_t*)pixels, bps, {}};
    for (uint64_t c = 0, at = 0; c < nc; ++c) {
        const uint64_t x0 = cdiv(im->x0, comp_dx[c]), y0 = cdiv(im->y0, comp_dy[c]), w = cdiv(im->x1, comp_dx[c]) - x0;
        src.comp.push_back({at, w, x0, y0});
        at += w * (cdiv(im->y1, comp_dy[c]) - y0) * bps;
    }
    for (uint32_t t = 0; t < ntiles; ++t)
        for (uint32_t k = 0; k < runs.size(); ++k) {
            Unit u{{}, runs[k].first};
            int rc = grk_amd_layout_tile_comp(im, base, comp_dx[runs[k].first], comp_dy[runs[k].first], t, &u.p);
            if (rc) return rc;
            u.p.num_comps = (uint16_t)runs[k].count;
            u.p.mct = runs[k].mct ? 1 : 0;
            units.push_back(u);
            rc = add_unit(g, u.p);
            if (rc) return rc;
        }
    return GRK_AMD_OK;
}

extern "C" int64_t grk_amd_encode_image_subsampled(grk_amd_ctx* ctx, const grk_amd_image_layout* im, const grk_amd_tile_params* base,
                                                   const uint8_t* comp_dx, const uint8_t* comp_dy, const void* pixels, uint32_t flags,
                                                   uint8_t* out, uint64_t cap)
{
    if (!ctx || !im || !base || !pixels || !out || !comp_dx || !comp_dy) return GRK_AMD_ERR_INVALID;
    // (a plain encode drops nothing: per-block zero bit-planes are grk_amd_encode_image_subsampled_rate's, refused here before any work)
    if (flags & GRK_AMD_CS_BLOCK_MSBS) return GRK_AMD_ERR_UNSUPPORTED;
    std::vector<Unit> units;
    SourcePlanes src;
    UnitGroups g;
    int rc = subsampled_image(ctx, im, base, comp_dx, comp_dy, pixels, units, src, g);
    if (rc) return rc;
    // Tier-2 on the device (encode_joint_device; GRK_AMD_IMAGE_T2=host: the host writer below, which is also where an image beyond
    // the device writer's tables goes): every group coded without a table, its rows and bytes kept on the device
    if (!image_t2_host()) {
        const uint32_t nruns = (uint32_t)comp_runs(base->num_comps, base->mct != 0, comp_dx, comp_dy).size();
        JointT2Call call{im, base, comp_dx, comp_dy, flags, nruns, &g, g.members, {}};
        std::vector<std::vector<uint8_t>> staged(g.members.size());     // (nothing waits between the batches: each keeps its own pixels)
        call.front = [&](size_t k) -> int {
            const auto& G = g.members[k];
            std::vector<uint8_t>& staging = staged[k];
            staging.resize(staged_bytes(src, units[G[0]]) * G.size());
            stage_units(src, units, G, staging.data(), 1);
            return grk_amd_encode_tiles(ctx, &units[G[0]].p, (uint32_t)G.size(), staging.data(), 0, nullptr, nullptr);
        };
        const int64_t n = encode_joint_device(ctx, call, out, cap, nullptr);
        if (n != GRK_AMD_ERR_UNSUPPORTED) return n;
    }
    std::vector<grk_amd_coded_block> rows;                   // tile-major, within a tile component-major (the runs in order)
    std::vector<uint8_t> coded;
    rc = encode_groups_host(ctx, src, units, g, rows, coded);
    if (rc) return rc;
    const int64_t n = grk_amd_write_codestream_subsampled(im, base, comp_dx, comp_dy, rows.data(), coded.data(), flags, out, cap);
    if (n >= 0) ++ctx->route_counters[1];
    return n;
}
