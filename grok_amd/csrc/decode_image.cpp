// grok_amd/csrc/decode_image.cpp -- a whole codestream to pixels (grk_amd_decode_image; on top of the C ABI's own entry points, as
// image.cpp is for encoding).  The reader (t2_reader.cpp) parses the packet headers on the host while the codestream's bytes
// travel to the device; the uploaded codestream is then the coded buffer itself -- a block's table row points into it --, with
// an appendix behind it for the blocks whose bytes come in several pieces (KG gathers those).  The tiles are grouped by geometry
// as the encoder groups them (image.h: add_unit), every group is one grk_amd_decode_tiles batch into a buffer of its own, and KP
// puts the group's tiles at their rectangles in the image.  With sub-sampled components the unit is a tile's run of components of
// one size (image.h: comp_runs), the destination one plane per component of its own size -- or, with grk_amd_set_decode_upsample,
// the image on the reference grid, where KU takes KP's place.
// grk_amd_decode_image_view is the same path for a view of the image (reduced resolution, a window): image_view_plan.cpp says which
// tiles it touches and where every unit goes; only those tiles' packets are read and only their tile-parts uploaded, as one compact
// coded buffer; the tile decoder runs at the view's reduce, and KP clips the tiles that the window holds in part.
// grk_amd_decode_surface is the same path again with a video surface as the destination (surface_plan.h): a one-tile image's runs that
// are a pixel layout are decoded straight onto it, every other unit into tight planes that KD (kernels_surface.hip) places.
#include "context.h"
#include "image.h"
#include "image_view_plan.h"
#include "surface_plan.h"
#include "t2_reader.h"
#include <thread>

namespace {

// what the call sets on the context, put back when it ends (the caller's own switches -- the int16 planes, the pixel layout,
// grk_amd_set_decode_upsample -- are not among it: they are left as they are)
struct SavedSettings {
    grk_amd_ctx* c;
    std::vector<uint16_t> qcd; std::vector<float> steps; std::vector<uint32_t> seg_first; std::vector<grk_amd_segment> segs;
    bool planes16; uint32_t reduce;
    explicit SavedSettings(grk_amd_ctx* ctx) : c(ctx), qcd(ctx->dec_qcd), steps(ctx->dec_steps), seg_first(ctx->dec_seg_first), segs(ctx->dec_segs),
                                               planes16(ctx->dec_planes16), reduce(ctx->dec_reduce) {}
    ~SavedSettings()
    {
        c->dec_qcd.swap(qcd); c->dec_steps.swap(steps); c->dec_seg_first.swap(seg_first); c->dec_segs.swap(segs);
        c->dec_planes16 = planes16; c->dec_reduce = reduce;
        c->have_geom = false;              // (the dequantisation scales follow the QCD words)
    }
};

int check_moves(grk_amd_ctx* c, const grk_amd_tp_segment* moves, uint64_t n, uint64_t src_bytes, uint64_t dst_bytes)
{
    for (uint64_t i = 0; i < n; ++i)
        if (moves[i].src > src_bytes || moves[i].len > src_bytes - moves[i].src || moves[i].dst > dst_bytes || moves[i].len > dst_bytes - moves[i].dst)
            return fail(c, GRK_AMD_ERR_INVALID, "a move outside its buffers");
    return GRK_AMD_OK;
}

int run_gather(grk_amd_ctx* c, const grk_amd_tp_segment* moves, uint64_t n, const void* src, void* dst)
{
    if (!n) return GRK_AMD_OK;
    HIP_TRY(c, c->img_moves.ensure(n * sizeof moves[0]), "alloc moves");
    HIP_TRY(c, hipMemcpy(c->img_moves.p, moves, n * sizeof moves[0], hipMemcpyHostToDevice), "upload moves");
    HIP_TRY(c, launch_t2dec_gather((const grk_amd_tp_segment*)c->img_moves.p, n, (const uint8_t*)src, (uint8_t*)dst, c->stream), "launch gather");
    ++c->img_launches[0];
    return GRK_AMD_OK;
}

} // namespace

extern "C" uint64_t grk_amd_decode_image_launches(grk_amd_ctx* c, int which)
{
    return c && which >= 0 && which < 2 ? c->img_launches[which] : 0;
}

extern "C" int grk_amd_gather_device(grk_amd_ctx* c, const grk_amd_tp_segment* moves, uint64_t num_moves, const void* src_base, uint64_t src_bytes,
                                     void* dst_base, uint64_t dst_bytes)
{
    if (!c || (num_moves && (!moves || !src_base || !dst_base))) return GRK_AMD_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device), "set device");
    int rc = check_moves(c, moves, num_moves, src_bytes, dst_bytes); if (rc) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream), "sync");          // (the moves' device copy may still be read by an earlier call)
    return run_gather(c, moves, num_moves, src_base, dst_base);
}

extern "C" int grk_amd_set_decode_upsample(grk_amd_ctx* c, int on)
{
    if (!c) return GRK_AMD_ERR_INVALID;
    c->dec_upsample = on != 0;
    return GRK_AMD_OK;
}

extern "C" int grk_amd_place_upsampled_device(grk_amd_ctx* c, const void* tiles, uint32_t nunits, uint32_t w, uint32_t h, uint32_t ncomp, uint32_t bps,
                                              const uint32_t* origins, uint32_t dx, uint32_t dy, void* image, uint32_t img_x0, uint32_t img_y0,
                                              uint32_t img_w, uint32_t img_h)
{
    if (!c || !tiles || !origins || !image || !nunits || !w || !h || !ncomp || ncomp > 65535 || nunits > 65535 || !bps || bps > 4 || !dx || !dy ||
        dx > 255 || dy > 255 || !img_w || !img_h || (uint64_t)img_x0 + img_w > 0xFFFFFFFFull || (uint64_t)img_y0 + img_h > 0xFFFFFFFFull)
        return GRK_AMD_ERR_INVALID;
    // every sample's footprint starts inside the image area (it may end beyond it: clipped)
    for (uint32_t u = 0; u < nunits; ++u) {
        const uint64_t fx0 = (uint64_t)origins[2 * u] * dx, fx1 = ((uint64_t)origins[2 * u] + w - 1) * dx;
        const uint64_t fy0 = (uint64_t)origins[2 * u + 1] * dy, fy1 = ((uint64_t)origins[2 * u + 1] + h - 1) * dy;
        if (fx0 < img_x0 || fx1 >= (uint64_t)img_x0 + img_w || fy0 < img_y0 || fy1 >= (uint64_t)img_y0 + img_h)
            return fail(c, GRK_AMD_ERR_INVALID, "a footprint outside the image");
    }
    HIP_TRY(c, hipSetDevice(c->device), "set device");
    HIP_TRY(c, hipStreamSynchronize(c->stream), "sync");
    HIP_TRY(c, c->img_rects.ensure((size_t)nunits * 8), "alloc places");
    HIP_TRY(c, hipMemcpy(c->img_rects.p, origins, (size_t)nunits * 8, hipMemcpyHostToDevice), "upload places");
    const UpsampleArgs a{(const uint8_t*)tiles, nunits, w, h, ncomp, bps, (const uint32_t*)c->img_rects.p, dx, dy, (uint8_t*)image, img_x0, img_y0, img_w, img_h,
                         bps, (uint64_t)img_w * bps, (uint64_t)img_w * img_h * bps};
    HIP_TRY(c, launch_t2dec_upsample(a, c->stream), "launch upsampling placement");
    ++c->img_launches[1];
    return GRK_AMD_OK;
}

extern "C" int grk_amd_place_tiles_device(grk_amd_ctx* c, const void* tiles, uint32_t ntiles, uint32_t w, uint32_t h, uint32_t ncomp, uint32_t bps,
                                          const uint32_t* rects, void* image, uint32_t img_w, uint32_t img_h)
{
    if (!c || !tiles || !rects || !image || !ntiles || !w || !h || !ncomp || ncomp > 65535 || ntiles > 65535 || !bps || bps > 4) return GRK_AMD_ERR_INVALID;
    for (uint32_t t = 0; t < ntiles; ++t)
        if (rects[2 * t] > img_w || w > img_w - rects[2 * t] || rects[2 * t + 1] > img_h || h > img_h - rects[2 * t + 1])
            return fail(c, GRK_AMD_ERR_INVALID, "a tile outside the image");
    HIP_TRY(c, hipSetDevice(c->device), "set device");
    HIP_TRY(c, hipStreamSynchronize(c->stream), "sync");
    HIP_TRY(c, c->img_rects.ensure((size_t)ntiles * 8), "alloc places");
    HIP_TRY(c, hipMemcpy(c->img_rects.p, rects, (size_t)ntiles * 8, hipMemcpyHostToDevice), "upload places");
    const PlaceArgs a{(const uint8_t*)tiles, ntiles, w, h, ncomp, bps, (const int32_t*)c->img_rects.p, (uint8_t*)image, img_w, img_h};
    HIP_TRY(c, launch_t2dec_place(a, c->stream), "launch placement");
    ++c->img_launches[1];
    return GRK_AMD_OK;
}

extern "C" uint64_t grk_amd_decode_image_counters(grk_amd_ctx* c, int which)
{
    return c && which >= 0 && which < 2 ? c->img_counters[which] : 0;
}

extern "C" int grk_amd_place_tiles_clipped_device(grk_amd_ctx* c, const void* tiles, uint32_t ntiles, uint32_t w, uint32_t h, uint32_t ncomp, uint32_t bps,
                                                  uint32_t channels, const int32_t* pos, void* image, uint32_t img_w, uint32_t img_h)
{
    if (!c || !tiles || !pos || !image || !ntiles || !w || !h || ntiles > 65535 || !bps || bps > 4 || channels > 255 || (!channels && (!ncomp || ncomp > 65535)) ||
        !img_w || !img_h || img_w > 0x7FFFFFFFu || img_h > 0x7FFFFFFFu || w > 0x7FFFFFFFu || h > 0x7FFFFFFFu)
        return GRK_AMD_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device), "set device");
    HIP_TRY(c, hipStreamSynchronize(c->stream), "sync");
    HIP_TRY(c, c->img_rects.ensure((size_t)ntiles * 8), "alloc places");
    HIP_TRY(c, hipMemcpy(c->img_rects.p, pos, (size_t)ntiles * 8, hipMemcpyHostToDevice), "upload places");
    // (interleaved pixels are placed as one component of samples as wide as a pixel)
    const PlaceArgs a{(const uint8_t*)tiles, ntiles, w, h, channels ? 1u : ncomp, channels ? channels * bps : bps, (const int32_t*)c->img_rects.p,
                      (uint8_t*)image, img_w, img_h};
    HIP_TRY(c, launch_t2dec_place(a, c->stream), "launch placement");
    ++c->img_launches[1];
    return GRK_AMD_OK;
}

// surf != nullptr (grk_amd_decode_surface): the destination is the caller's surface as *surf describes it -- every component at its own
// size wherever it lies there, sub-sampled or not; the surface is resolved against the stream's header here
static int decode_view(grk_amd_ctx* c, const uint8_t* cs, uint64_t len, const grk_amd_image_view* view, void* pixels, uint64_t cap, int pixels_on_device,
                       const grk_amd_surface* surf = nullptr)
{
    grk_amd_stream_info info;
    std::string why;
    int rc = read_stream_header(cs, len, info, why);
    if (rc) return fail(c, rc, why.c_str());
    const uint32_t nc = info.base.num_comps, bps = (info.base.prec + 7u) / 8u, nt = info.num_tiles;
    ViewPlan plan;
    {
        const char* pwhy = "";
        rc = plan_image_view(info, view, plan, &pwhy);
        if (rc) return fail(c, rc, pwhy);
    }
    const bool sub = plan.sub || surf, up = sub && !surf && c->dec_upsample;
    const uint32_t red = plan.reduce;
    if (red && up) return fail(c, GRK_AMD_ERR_UNSUPPORTED, "a reduced resolution of sub-sampled components together with upsampling (grk_amd_set_decode_upsample)");
    if (sub && !up && !surf) {       // (components of different sizes have no interleaved form, and each plane is tight: as grk_amd_encode_image_subsampled)
        const grk_amd_pixel_layout& l = c->dec_layout;
        if (l.interleaved || l.channels || l.row_pitch || l.plane_pitch || l.tile_pitch)
            return fail(c, GRK_AMD_ERR_UNSUPPORTED, "a decode pixel layout for sub-sampled components without upsampling (grk_amd_set_decode_upsample)");
    }
    // the units of decoding: a touched tile's runs of components of one size (without sub-sampling: the tile)
    const std::vector<CompRun>& runs = plan.runs;
    if (info.base.mct && !runs[0].mct) return fail(c, GRK_AMD_ERR_UNSUPPORTED, "the colour transform across components of different size");
    // the view's image (upsampled components: the image area itself; the plan refused every other view of them)
    const uint64_t W = up ? (uint64_t)info.layout.x1 - info.layout.x0 : plan.comp_w[0], H = up ? (uint64_t)info.layout.y1 - info.layout.y0 : plan.comp_h[0];
    // ... in the context's decode layout (grk_amd_set_decode_pixel_layout: row_pitch the view's; the default: tight planes) ...
    PixelLayout ipx;
    {
        const char* lwhy = "";
        if (W >> 32 || H >> 32 || !resolve_pixel_layout(info.base, surf ? nullptr : &c->dec_layout, (uint32_t)W, (uint32_t)H, 1, ipx, &lwhy)) return fail(c, GRK_AMD_ERR_INVALID, lwhy);
    }
    // ... or, sub-sampled components as they are: component k's plane of its own size, tight, the planes back to back
    struct Plane { uint64_t at, w, h, x0, y0; };          // (x0, y0: the component's first sample at full size, for KU)
    std::vector<Plane> plane(nc);
    uint64_t total = 0;
    for (uint32_t k = 0; k < nc; ++k) {
        const uint64_t dx = info.comp_dx[k], dy = info.comp_dy[k];
        plane[k] = Plane{total, plan.comp_w[k], plan.comp_h[k], (info.layout.x0 + dx - 1) / dx, (info.layout.y0 + dy - 1) / dy};
        total += plane[k].w * plane[k].h * bps;
    }
    if (!sub || up) total = ipx.bytes;
    // ... or wherever the surface puts them: no two of them on one byte, all of it inside `cap`
    ResolvedSurface rs;
    if (surf) {
        const char* swhy = "";
        rc = resolve_surface(&info.layout, &info.base, info.comp_dx, info.comp_dy, surf, rs, &swhy);
        if (!rc) rc = check_surface_disjoint(rs, &swhy);
        if (rc) return fail(c, rc, swhy);
        total = rs.bytes;
    }
    if (total > cap) return fail(c, GRK_AMD_ERR_OVERFLOW, "the image does not fit `cap`");
    // the units, grouped by geometry (units of one group are of one size at every reduce: same_geometry compares every resolution)
    const uint32_t nr = (uint32_t)runs.size(), ntt = (uint32_t)plan.tiles.size(), nu = ntt * nr;
    if (!nu) return fail(c, GRK_AMD_ERR_INVALID, "a view that touches no tile");
    std::vector<grk_amd_tile_params> tp(nu);                  // [touched tile][run]
    UnitGroups g;
    for (uint32_t u = 0; u < nu; ++u) {
        tp[u] = plan.units[u].p;
        rc = add_unit(g, tp[u]);
        if (rc) return fail(c, rc, "a tile's geometry");
    }
    // (runs of one geometry -- luma and alpha -- share a group and its batch; they go to different planes: a group's units run by run)
    for (auto& G : g.members) std::stable_sort(G.begin(), G.end(), [nr](uint32_t a, uint32_t b) { return a % nr < b % nr; });
    const bool ht = !info.base.reserved[0];
    if (ht) {
        // HT blocks are decoded against the band's Kmax of the library's own geometry (ensure_geom), not against the stream's QCD
        for (const TileGeom& tg : g.geoms)
            for (uint32_t r = 0; r <= info.base.num_levels; ++r)
                for (uint32_t bi = 0; bi < tg.res[r].num_bands; ++bi) {
                    const uint32_t q = r ? 3 * (r - 1) + 1 + bi : 0;
                    const uint32_t expn = info.qstyle ? info.qcd_words[q] >> 11 : info.qcd_words[q] >> 3;
                    if (expn + info.guard_bits - 1u != tg.res[r].band[bi].kmax)
                        return fail(c, GRK_AMD_ERR_UNSUPPORTED, "an HT stream whose QCD exponents are not the ones this library derives for the geometry");
                }
    }
    // the coded buffer: the codestream itself, or -- a view that leaves tiles out -- the touched tiles' tile-parts end to end in index
    // order (part_to: where each starts in it).  Where the tile-parts lie: found up front only when the upload depends on it
    // (a view of every tile finds them beside its upload, as the packets are read)
    std::vector<StreamPart> parts;
    const bool all = ntt == nt;
    if (!all) {
        rc = locate_stream_parts(cs, len, info, parts, why);
        if (rc) return fail(c, rc, why.c_str());
    }
    std::vector<uint64_t> part_to(ntt, 0);
    uint64_t up_len = len;
    if (!all) {
        up_len = 0;
        for (uint32_t i = 0; i < ntt; ++i) { part_to[i] = up_len; up_len += parts[plan.tiles[i]].len; }
    }
    HIP_TRY(c, hipSetDevice(c->device), "set device");
    rc = join_side(c); if (rc) return rc;
    // the upload (an appendix holds bytes of what is uploaded: never more than that), the packet headers meanwhile
    const uint64_t coded_cap = up_len + (info.num_layers > 1 ? up_len : 0);
    HIP_TRY(c, c->img_coded.ensure(coded_cap + 64), "alloc the coded buffer");
    StreamTable tab;
    int rrc = GRK_AMD_OK;
    {
        const uint32_t threads = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
        std::thread reader([&]() {
            if (all) rrc = locate_stream_parts(cs, len, info, parts, why);
            if (!rrc) rrc = read_stream_packets_of(cs, len, info, parts, all ? nullptr : &plan.tiles, red, threads, tab, why);
        });
        if (all) rc = copy_h2d(c, c->img_coded.p, cs, len);
        else
            for (uint32_t i = 0, j; i < ntt && !rc; i = j) {        // tile-parts that follow each other in the file: one copy
                uint64_t n = parts[plan.tiles[i]].len;
                for (j = i + 1; j < ntt && parts[plan.tiles[j]].at == parts[plan.tiles[i]].at + n; ++j) n += parts[plan.tiles[j]].len;
                rc = copy_h2d(c, (uint8_t*)c->img_coded.p + part_to[i], cs + parts[plan.tiles[i]].at, n);
            }
        reader.join();
    }
    if (rc) return rc;
    if (rrc) return fail(c, rrc, why.c_str());
    c->img_counters[0] += ntt; c->img_counters[1] += up_len;
    if (!all) {
        // the reader's offsets are positions in the codestream (the appendix behind it): onto the compact buffer
        for (uint32_t i = 0; i < ntt; ++i) {
            const StreamPart& sp = parts[plan.tiles[i]];
            for (uint64_t k = tab.row_at[i]; k < tab.row_at[i + 1]; ++k) {
                grk_amd_coded_block& row = tab.rows[k];
                if (!row.length) continue;
                if (row.offset >= len) row.offset = row.offset - len + up_len;
                else if (row.offset < sp.at || row.offset - sp.at > sp.len) return fail(c, GRK_AMD_ERR_INVALID, "a block outside its tile-part");
                else row.offset = row.offset - sp.at + part_to[i];
            }
            for (uint64_t k = tab.move_at[i]; k < tab.move_at[i + 1]; ++k) {
                grk_amd_tp_segment& m = tab.moves[k];
                if (m.src < sp.at || m.src - sp.at > sp.len) return fail(c, GRK_AMD_ERR_INVALID, "a block outside its tile-part");
                m.src = m.src - sp.at + part_to[i];
            }
        }
    }
    const uint64_t coded_bytes = up_len + tab.appendix_bytes;
    if (coded_bytes > coded_cap) return fail(c, GRK_AMD_ERR_INVALID, "an appendix larger than the codestream");
    rc = check_moves(c, tab.moves.data(), tab.moves.size(), up_len, tab.appendix_bytes); if (rc) return rc;
    // a unit's rows in the reader's table: tile after tile, within a tile component after component
    std::vector<uint64_t> unit_row(nu + 1, 0);
    for (uint32_t u = 0; u < nu; ++u) {
        if (u % nr == 0 && unit_row[u] != tab.row_at[u / nr]) return fail(c, GRK_AMD_ERR_INVALID, "the reader's table does not fit the tiles");
        unit_row[u + 1] = unit_row[u] + (uint64_t)g.geoms[g.of[u]].blocks_per_comp * tp[u].num_comps;
    }
    if (unit_row[nu] != tab.rows.size()) return fail(c, GRK_AMD_ERR_INVALID, "the reader's table does not fit the tiles");
    // (from here on the call only queues work; the small tables below are uploaded with blocking copies into buffers that an
    //  earlier call's kernels may still read)
    HIP_TRY(c, hipStreamSynchronize(c->stream), "sync");
    rc = run_gather(c, tab.moves.data(), tab.moves.size(), c->img_coded.p, (uint8_t*)c->img_coded.p + up_len); if (rc) return rc;

    SavedSettings saved(c);
    c->dec_steps.clear();
    c->dec_reduce = red;                   // (the switch grk_amd_set_decode_reduce sets: every decode below delivers plan.units[u].w x h)
    rc = grk_amd_set_decode_qcd(c, info.qcd_words, info.base.irreversible ? info.num_qcd : 0); if (rc) return rc;
    // Part-1 blocks of several codeword segments need the segment list; one segment per block is what the table row says
    const bool want_segs = !ht && (info.base.reserved[1] & 0x05);
    auto group_tables = [&](const std::vector<uint32_t>& G, std::vector<grk_amd_coded_block>& table) -> int {
        table.clear();
        std::vector<uint32_t> first;
        std::vector<grk_amd_segment> segs;
        for (uint32_t u : G) {
            table.insert(table.end(), tab.rows.begin() + unit_row[u], tab.rows.begin() + unit_row[u + 1]);
            for (uint64_t i = unit_row[u]; want_segs && i < unit_row[u + 1]; ++i) {
                first.push_back((uint32_t)segs.size());
                segs.insert(segs.end(), tab.segments.begin() + tab.first_segment[i], tab.segments.begin() + tab.first_segment[i + 1]);
            }
        }
        if (!want_segs) return grk_amd_set_decode_segments(c, nullptr, nullptr, 0);
        first.push_back((uint32_t)segs.size());
        return grk_amd_set_decode_segments(c, first.data(), segs.data(), (uint32_t)table.size());
    };
    std::vector<grk_amd_coded_block> table;
    // the region decoder's own conditions (grk_amd_decode_region): a DWT level left, samples of at most 16 bits
    const bool region_ok = info.base.num_levels > red && bps <= 2;
    if (!surf && nt == 1 && nr == 1 && !up && (plan.units[0].whole || region_ok)) {
        // one tile: decoded straight into the destination (host pixels: grk_amd_decode_tiles repeats a group that leaves the int16
        // planes by itself) -- a window of it by the region decoder, whose cost follows the window
        const ViewUnit& u = plan.units[0];
        rc = group_tables(g.members[0], table);
        if (rc) return rc;
        if (u.whole) return grk_amd_decode_tiles(c, &tp[0], 1, table.data(), c->img_coded.p, coded_bytes, 1, pixels, pixels_on_device);
        return grk_amd_decode_region(c, &tp[0], table.data(), c->img_coded.p, coded_bytes, 1, (uint32_t)-u.x, (uint32_t)-u.y, (uint32_t)(-u.x + (int64_t)W),
                                     (uint32_t)(-u.y + (int64_t)H), pixels, pixels_on_device);
    }
    HIP_TRY(c, c->img_status.ensure(64), "alloc status");
    if (!surf && nt == 1 && nr > 1 && !up) {
        // one tile of several runs: run by run straight into the run's planes; a decode into device pixels leaves its status to
        // the next one's, so it is kept as for the groups below
        if (pixels_on_device) HIP_TRY(c, hipMemsetAsync(c->img_status.p, 0, 4, c->stream), "clear status");
        for (uint32_t r = 0; r < nr; ++r) {
            rc = group_tables(std::vector<uint32_t>{r}, table); if (rc) return rc;
            uint8_t* const dst = (uint8_t*)pixels + plane[runs[r].first].at;
            // (a plane behind planes of odd size may start off the 4-byte alignment the decoder's pixel stores are written for: such a
            //  run in device memory is decoded beside it and copied)
            const bool beside = pixels_on_device && ((uintptr_t)dst & 3u);
            const size_t run_bytes = (size_t)plan.units[r].w * plan.units[r].h * tp[r].num_comps * bps;
            if (beside) HIP_TRY(c, c->img_tiles.ensure(run_bytes), "alloc a run's planes");
            rc = grk_amd_decode_tiles(c, &tp[r], 1, table.data(), c->img_coded.p, coded_bytes, 1, beside ? c->img_tiles.p : dst, pixels_on_device);
            if (rc) return rc;
            if (beside) HIP_TRY(c, hipMemcpyAsync(dst, c->img_tiles.p, run_bytes, hipMemcpyDeviceToDevice, c->stream), "copy a run's planes");
            if (pixels_on_device)
                HIP_TRY(c, launch_t2dec_or_status((unsigned int*)c->img_status.p, (const unsigned int*)c->flag.p, false, c->stream), "keep status");
        }
        if (pixels_on_device)
            HIP_TRY(c, launch_t2dec_or_status((unsigned int*)c->flag.p, (const unsigned int*)c->img_status.p, true, c->stream), "hand over status");
        return GRK_AMD_OK;
    }
    // a group's batch (`table`: its rows) into device memory at dst, its status kept in the image's
    auto decode_group = [&](const grk_amd_tile_params& p, uint32_t n, void* dst) -> int {
        int drc = grk_amd_decode_tiles(c, &p, n, table.data(), c->img_coded.p, coded_bytes, 1, dst, 1); if (drc) return drc;
        // The int16-plane rule (include/grok_amd.h, grk_amd_set_decode_planes16).  A decode into a device buffer does not repeat
        // itself: with host pixels this call joins behind a group that may use those planes, reads its status and repeats it
        // with int32 planes; with device pixels the status goes to grk_amd_decode_status like any other
        if (!pixels_on_device && c->dec_planes16 && ht && !p.irreversible && p.prec <= 8) {
            drc = grk_amd_decode_status(c);
            if (drc == GRK_AMD_ERR_RANGE) {
                c->dec_planes16 = false;
                drc = grk_amd_decode_tiles(c, &p, n, table.data(), c->img_coded.p, coded_bytes, 1, dst, 1);
                c->dec_planes16 = true;
            }
            if (drc) return drc;
        }
        HIP_TRY(c, launch_t2dec_or_status((unsigned int*)c->img_status.p, (const unsigned int*)c->flag.p, false, c->stream), "keep status");
        return GRK_AMD_OK;
    };
    if (surf) {
        // Onto a surface.  The image's copy of a host surface travels both ways (what is no sample stays); a run of a one-tile image
        // that the plan (surface_plan.h) finds expressible as a pixel layout is decoded straight onto the surface through it, every
        // other unit into tight planes that KD places
        uint8_t* d_surf = (uint8_t*)pixels;
        if (!pixels_on_device) {
            HIP_TRY(c, c->img_pixels.ensure(total), "alloc the surface"); d_surf = (uint8_t*)c->img_pixels.p;
            rc = copy_h2d(c, d_surf, pixels, total); if (rc) return rc;
        }
        const bool direct = surface_direct_allowed();
        std::vector<SurfaceRoute> route(nr);
        for (uint32_t r = 0; r < nr; ++r)
            route[r] = plan_surface_run(rs, runs[r], nt == 1, true, direct, pixels_on_device ? cap : total, (uint32_t)((uintptr_t)d_surf & 3u));
        std::vector<std::vector<uint32_t>> staged(g.members.size());
        std::vector<uint32_t> origins;
        uint64_t group_bytes = 0;
        for (size_t k = 0; k < g.members.size(); ++k) {
            for (uint32_t u : g.members[k]) if (!route[u % nr].in_place) staged[k].push_back(u);      // (sorted run by run above)
            for (uint32_t u : staged[k]) {
                const SurfacePlane& sp = rs.comp[runs[u % nr].first];
                origins.push_back((uint32_t)(tp[u].tile_x0 - sp.x0));
                origins.push_back((uint32_t)(tp[u].tile_y0 - sp.y0));
            }
            if (!staged[k].empty())
                group_bytes = std::max<uint64_t>(group_bytes, (uint64_t)tp[staged[k][0]].tile_w * tp[staged[k][0]].tile_h * tp[staged[k][0]].num_comps * bps * staged[k].size());
        }
        HIP_TRY(c, c->img_tiles.ensure(group_bytes), "alloc a group's units");
        HIP_TRY(c, c->img_rects.ensure(origins.size() * 4 + 8), "alloc origins");
        if (!origins.empty()) HIP_TRY(c, hipMemcpy(c->img_rects.p, origins.data(), origins.size() * 4, hipMemcpyHostToDevice), "upload origins");
        HIP_TRY(c, hipMemsetAsync(c->img_status.p, 0, 4, c->stream), "clear status");
        struct KeepLayout { grk_amd_ctx* c; grk_amd_pixel_layout keep; ~KeepLayout() { c->dec_layout = keep; } } keep{c, c->dec_layout};
        size_t origin_at = 0;
        for (size_t k = 0; k < g.members.size(); ++k) {
            for (uint32_t u : g.members[k]) {
                const SurfaceRoute& r = route[u % nr];
                if (!r.in_place) continue;
                c->dec_layout = r.layout;
                rc = group_tables(std::vector<uint32_t>{u}, table); if (rc) return rc;
                rc = decode_group(tp[u], 1, d_surf + r.at); if (rc) return rc;
                ++c->surf_counters[0];
            }
            const std::vector<uint32_t>& S = staged[k];
            if (S.empty()) continue;
            const grk_amd_tile_params& p = tp[S[0]];
            c->dec_layout = grk_amd_pixel_layout{};
            rc = group_tables(S, table); if (rc) return rc;
            rc = decode_group(p, (uint32_t)S.size(), c->img_tiles.p); if (rc) return rc;
            const size_t unit_size = (size_t)p.tile_w * p.tile_h * p.num_comps * bps;
            for (size_t i0 = 0, i1; i0 < S.size(); i0 = i1) {          // the group's units of one run: one launch
                for (i1 = i0 + 1; i1 < S.size() && S[i1] % nr == S[i0] % nr;) ++i1;
                rc = queue_surface_kernel(c, true, rs, runs[S[i0] % nr], d_surf, (uint8_t*)c->img_tiles.p + i0 * unit_size, (uint32_t)(i1 - i0), p.tile_w, p.tile_h,
                                          (const uint32_t*)c->img_rects.p + 2 * (origin_at + i0));
                if (rc) return rc;
            }
            c->surf_counters[1] += S.size();
            origin_at += S.size();
        }
        HIP_TRY(c, launch_t2dec_or_status((unsigned int*)c->flag.p, (const unsigned int*)c->img_status.p, true, c->stream), "hand over status");
        if (pixels_on_device) return GRK_AMD_OK;
        rc = copy_d2h(c, pixels, d_surf, total); if (rc) return rc;
        return grk_amd_decode_status(c);
    }
    void* d_img = pixels;
    if (!pixels_on_device) {
        HIP_TRY(c, c->img_pixels.ensure(total), "alloc the image"); d_img = c->img_pixels.p;
        // (the extent comes back as one copy: what the caller has in a layout's gaps goes up first)
        if ((!sub || up) && ipx.lay) { rc = copy_h2d(c, d_img, pixels, total); if (rc) return rc; }
    }
    // the tile decoder writes tight tiles in the same kind of layout; KP places them by rows of whole pixels and clips them to the
    // view.  Runs of sub-sampled components are decoded as tight planes: KP places them in the components' planes, KU on the reference grid
    const bool whole_pixels = !sub && ipx.lay == 2;
    const uint32_t unit_ch = whole_pixels ? ipx.channels : 0;
    struct TileLayout { grk_amd_ctx* c; grk_amd_pixel_layout keep; ~TileLayout() { c->dec_layout = keep; } } tile_layout{c, c->dec_layout};
    {
        grk_amd_pixel_layout tl{};
        if (whole_pixels) { tl.interleaved = 1; tl.channels = (uint8_t)ipx.channels; tl.fill = c->dec_layout.fill; }
        c->dec_layout = tl;
    }
    uint64_t group_bytes = 0;
    for (const auto& G : g.members)
        group_bytes = std::max<uint64_t>(group_bytes, (uint64_t)plan.units[G[0]].w * plan.units[G[0]].h * (unit_ch ? unit_ch : tp[G[0]].num_comps) * bps * G.size());
    HIP_TRY(c, c->img_tiles.ensure(group_bytes), "alloc a group's tiles");
    HIP_TRY(c, c->img_rects.ensure((size_t)nu * 8), "alloc places");
    {
        // group after group: where a unit goes in its components' planes of the view (signed: KP clips) -- or, for KU, its first
        // sample in the component
        std::vector<uint32_t> rects;
        for (const auto& G : g.members)
            for (uint32_t u : G) {
                rects.push_back(up ? tp[u].tile_x0 : (uint32_t)plan.units[u].x);
                rects.push_back(up ? tp[u].tile_y0 : (uint32_t)plan.units[u].y);
            }
        HIP_TRY(c, hipMemcpy(c->img_rects.p, rects.data(), rects.size() * 4, hipMemcpyHostToDevice), "upload places");
    }
    HIP_TRY(c, hipMemsetAsync(c->img_status.p, 0, 4, c->stream), "clear status");
    if (up) {
        // what no footprint covers: the strip left of and above a component's first sample (image origins that are no multiple of
        // the factor) is 0, the samples beyond num_comps of interleaved pixels are `fill`
        const uint64_t kstep = ipx.lay == 2 ? bps : ipx.kstep;
        for (uint32_t k = 0; k < nc; ++k) {
            const uint32_t zx = (uint32_t)std::min<uint64_t>(W, plane[k].x0 * info.comp_dx[k] - info.layout.x0);
            const uint32_t zy = (uint32_t)std::min<uint64_t>(H, plane[k].y0 * info.comp_dy[k] - info.layout.y0);
            uint8_t* const at = (uint8_t*)d_img + k * kstep;
            HIP_TRY(c, launch_t2dec_fill(FillArgs{at, 0, 0, zx, (uint32_t)H, bps, 0, ipx.xstep, ipx.row}, c->stream), "launch fill");
            HIP_TRY(c, launch_t2dec_fill(FillArgs{at, zx, 0, (uint32_t)W - zx, zy, bps, 0, ipx.xstep, ipx.row}, c->stream), "launch fill");
        }
        for (uint32_t k = nc; ipx.lay == 2 && k < ipx.channels; ++k)
            HIP_TRY(c, launch_t2dec_fill(FillArgs{(uint8_t*)d_img + k * kstep, 0, 0, (uint32_t)W, (uint32_t)H, bps, ipx.fill, ipx.xstep, ipx.row}, c->stream), "launch fill");
    }
    size_t rect_at = 0;
    for (const auto& G : g.members) {
        const grk_amd_tile_params& p = tp[G[0]];
        const uint32_t uw = plan.units[G[0]].w, uh = plan.units[G[0]].h;        // (the group's units at the view's reduce)
        if (!uw || !uh) { rect_at += G.size(); continue; }                     // nothing of them is left at this reduce
        rc = group_tables(G, table); if (rc) return rc;
        rc = decode_group(p, (uint32_t)G.size(), c->img_tiles.p); if (rc) return rc;
        const size_t unit_size = (size_t)uw * uh * (unit_ch ? unit_ch : p.num_comps) * bps;
        for (size_t i0 = 0, i1; i0 < G.size(); i0 = i1) {          // the group's units of one run: one launch into that run's planes
            for (i1 = i0 + 1; i1 < G.size() && G[i1] % nr == G[i0] % nr;) ++i1;
            const CompRun& run = runs[G[i0] % nr];
            const uint8_t* const staged = (const uint8_t*)c->img_tiles.p + i0 * unit_size;
            const uint32_t* const rects = (const uint32_t*)c->img_rects.p + 2 * (rect_at + i0);
            const uint32_t count = (uint32_t)(i1 - i0);
            if (up) {
                const uint64_t kstep = ipx.lay == 2 ? bps : ipx.kstep;
                const UpsampleArgs a{staged, count, p.tile_w, p.tile_h, run.count, bps, rects, info.comp_dx[run.first],
                                     info.comp_dy[run.first], (uint8_t*)d_img + run.first * kstep, info.layout.x0, info.layout.y0, (uint32_t)W, (uint32_t)H,
                                     ipx.xstep, ipx.row, kstep};
                HIP_TRY(c, launch_t2dec_upsample(a, c->stream), "launch upsampling placement");
            } else if (sub) {
                const Plane& pl = plane[run.first];
                const PlaceArgs a{staged, count, uw, uh, run.count, bps, (const int32_t*)rects, (uint8_t*)d_img + pl.at,
                                  (uint32_t)pl.w, (uint32_t)pl.h, 0, 0};
                HIP_TRY(c, launch_t2dec_place(a, c->stream), "launch placement");
            } else {
                const PlaceArgs a{staged, count, uw, uh, ipx.lay == 2 ? 1u : nc, ipx.lay == 2 ? unit_ch * bps : bps,
                                  (const int32_t*)rects, (uint8_t*)d_img, (uint32_t)W, (uint32_t)H, ipx.lay ? ipx.row : 0, ipx.lay == 1 ? ipx.kstep : 0};
                HIP_TRY(c, launch_t2dec_place(a, c->stream), "launch placement");
            }
            ++c->img_launches[1];
        }
        rect_at += G.size();
    }
    HIP_TRY(c, launch_t2dec_or_status((unsigned int*)c->flag.p, (const unsigned int*)c->img_status.p, true, c->stream), "hand over status");
    if (pixels_on_device) return GRK_AMD_OK;
    rc = copy_d2h(c, pixels, d_img, total); if (rc) return rc;
    return grk_amd_decode_status(c);
}

extern "C" int grk_amd_decode_image(grk_amd_ctx* c, const uint8_t* cs, uint64_t len, void* pixels, uint64_t cap, int pixels_on_device)
{
    if (!c || !cs || !pixels) return GRK_AMD_ERR_INVALID;
    if (c->dec_reduce) return fail(c, GRK_AMD_ERR_UNSUPPORTED, "grk_amd_decode_image at reduced resolution");
    if (!c->dec_kids.empty()) return fail(c, GRK_AMD_ERR_UNSUPPORTED, "grk_amd_decode_image on a context with a decode sequence (grk_amd_set_decode_pipelining)");
    return decode_view(c, cs, len, nullptr, pixels, cap, pixels_on_device);
}

extern "C" int grk_amd_decode_surface(grk_amd_ctx* c, const uint8_t* cs, uint64_t len, const grk_amd_surface* surface, void* pixels, uint64_t cap,
                                      int pixels_on_device)
{
    if (!c || !cs || !pixels || !surface) return GRK_AMD_ERR_INVALID;
    if (c->dec_reduce) return fail(c, GRK_AMD_ERR_UNSUPPORTED, "grk_amd_decode_surface at reduced resolution");
    if (!c->dec_kids.empty()) return fail(c, GRK_AMD_ERR_UNSUPPORTED, "grk_amd_decode_surface on a context with a decode sequence (grk_amd_set_decode_pipelining)");
    return decode_view(c, cs, len, nullptr, pixels, cap, pixels_on_device, surface);
}

extern "C" int grk_amd_decode_image_view(grk_amd_ctx* c, const uint8_t* cs, uint64_t len, const grk_amd_image_view* view, void* pixels, uint64_t cap,
                                         int pixels_on_device)
{
    if (!c || !cs || !pixels) return GRK_AMD_ERR_INVALID;
    // (the view's reduce is the call's own parameter: the context's switch is the tile-level calls')
    if (c->dec_reduce) return fail(c, GRK_AMD_ERR_UNSUPPORTED, "grk_amd_decode_image_view on a context set to a reduced resolution (grk_amd_set_decode_reduce): the view carries its own");
    if (!c->dec_kids.empty()) return fail(c, GRK_AMD_ERR_UNSUPPORTED, "grk_amd_decode_image_view on a context with a decode sequence (grk_amd_set_decode_pipelining)");
    return decode_view(c, cs, len, view, pixels, cap, pixels_on_device);
}
