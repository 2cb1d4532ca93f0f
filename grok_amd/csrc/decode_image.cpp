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
// This file is the executor.  Which route a call takes, every refusal before the first HIP call, every offset, size, group and launch
// segment is the word of decode_image_plan.cpp (HIP-free, tested on the CPU); what is left here is the order of the HIP calls.
#include "context.h"
#include "decode_image_plan.h"
#include <thread>

namespace {

// what the call sets on the context, put back when it ends -- the pixel layout among it, which the staged routes set for their
// batches (the caller's other switches -- the int16 planes, grk_amd_set_decode_upsample -- are left as they are)
struct SavedSettings {
    grk_amd_ctx* c;
    std::vector<uint16_t> qcd; std::vector<float> steps; std::vector<uint32_t> seg_first; std::vector<grk_amd_segment> segs;
    bool planes16; uint32_t reduce; KeepLayout layout;
    explicit SavedSettings(grk_amd_ctx* ctx) : c(ctx), qcd(ctx->dec_qcd), steps(ctx->dec_steps), seg_first(ctx->dec_seg_first), segs(ctx->dec_segs),
                                               planes16(ctx->dec_planes16), reduce(ctx->dec_reduce), layout{ctx->dec_layout, ctx->dec_layout} {}
    ~SavedSettings()
    {
        c->dec_qcd.swap(qcd); c->dec_steps.swap(steps); c->dec_seg_first.swap(seg_first); c->dec_segs.swap(segs);
        c->dec_planes16 = planes16; c->dec_reduce = reduce;
        c->have_geom = false;              // (the dequantisation scales follow the QCD words)
    }
};

int run_gather(grk_amd_ctx* c, const grk_amd_tp_segment* moves, uint64_t n, const void* src, void* dst)
{
    if (!n) return GRK_AMD_OK;
    HIP_TRY(c, c->img_moves.ensure(n * sizeof moves[0]), "alloc moves");
    HIP_TRY(c, hipMemcpy(c->img_moves.p, moves, n * sizeof moves[0], hipMemcpyHostToDevice), "upload moves");
    HIP_TRY(c, launch_t2dec_gather((const grk_amd_tp_segment*)c->img_moves.p, n, (const uint8_t*)src, (uint8_t*)dst, c->stream), "launch gather");
    ++c->img_launches[0];
    return GRK_AMD_OK;
}

// what the grk_amd_place_*_device entry points do behind their own argument checks: the places (x, y per unit) into img_rects --
// which an earlier call's kernel may still read --, the kernel, the count
template <class Launch> int place_units(grk_amd_ctx* c, const void* places, uint32_t nunits, const char* what, Launch launch)
{
    HIP_TRY(c, hipSetDevice(c->device), "set device");
    HIP_TRY(c, hipStreamSynchronize(c->stream), "sync");
    HIP_TRY(c, c->img_rects.ensure((size_t)nunits * 8), "alloc places");
    HIP_TRY(c, hipMemcpy(c->img_rects.p, places, (size_t)nunits * 8, hipMemcpyHostToDevice), "upload places");
    HIP_TRY(c, launch(), what);
    ++c->img_launches[1];
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
    const char* why = "";
    const int rc = check_moves(moves, num_moves, src_bytes, dst_bytes, &why); if (rc) return fail(c, rc, why);
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
    return place_units(c, origins, nunits, "launch upsampling placement", [&]() {
        return launch_t2dec_upsample(UpsampleArgs{(const uint8_t*)tiles, nunits, w, h, ncomp, bps, (const uint32_t*)c->img_rects.p, dx, dy, (uint8_t*)image, img_x0,
                                                  img_y0, img_w, img_h, bps, (uint64_t)img_w * bps, (uint64_t)img_w * img_h * bps}, c->stream);
    });
}

extern "C" int grk_amd_place_tiles_device(grk_amd_ctx* c, const void* tiles, uint32_t ntiles, uint32_t w, uint32_t h, uint32_t ncomp, uint32_t bps,
                                          const uint32_t* rects, void* image, uint32_t img_w, uint32_t img_h)
{
    if (!c || !tiles || !rects || !image || !ntiles || !w || !h || !ncomp || ncomp > 65535 || ntiles > 65535 || !bps || bps > 4) return GRK_AMD_ERR_INVALID;
    for (uint32_t t = 0; t < ntiles; ++t)
        if (rects[2 * t] > img_w || w > img_w - rects[2 * t] || rects[2 * t + 1] > img_h || h > img_h - rects[2 * t + 1])
            return fail(c, GRK_AMD_ERR_INVALID, "a tile outside the image");
    return place_units(c, rects, ntiles, "launch placement", [&]() {
        return launch_t2dec_place(PlaceArgs{(const uint8_t*)tiles, ntiles, w, h, ncomp, bps, (const int32_t*)c->img_rects.p, (uint8_t*)image, img_w, img_h}, c->stream);
    });
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
    // (interleaved pixels are placed as one component of samples as wide as a pixel)
    return place_units(c, pos, ntiles, "launch placement", [&]() {
        return launch_t2dec_place(PlaceArgs{(const uint8_t*)tiles, ntiles, w, h, channels ? 1u : ncomp, channels ? channels * bps : bps,
                                            (const int32_t*)c->img_rects.p, (uint8_t*)image, img_w, img_h}, c->stream);
    });
}

// surf != nullptr (grk_amd_decode_surface): the destination is the caller's surface as *surf describes it -- every component at its own
// size wherever it lies there, sub-sampled or not; the surface is resolved against the stream's header by the plan.
// host_rules: the call behaves as one with a host destination does -- it joins behind a group that may leave the int16 planes and
// repeats it with int32 planes by itself.  That is every call with host pixels, and the packed decode of a host frame (packed.cpp),
// whose planes lie in device memory all the same.
// res != nullptr (grk_amd_decode_image_device): the codestream lies in device memory and IS the coded buffer -- nothing is uploaded,
// no packet is read here: the header and the table are the device reader's (read_device.hip); `cs` is not looked at.
// d_moves (num_moves of them, device memory): the table has an appendix -- the stream is staged in front of it in the context's coded
// buffer (the decoders take one coded base), the gather reads the moves where they lie; *staged: bytes copied so
struct ResidentStream { const void* d_cs; const grk_amd_stream_info* info; StreamTable* tab; const grk_amd_tp_segment* d_moves; uint64_t num_moves; uint64_t* staged; };
static int decode_view(grk_amd_ctx* c, const uint8_t* cs, uint64_t len, const grk_amd_image_view* view, void* pixels, uint64_t cap, int pixels_on_device,
                       const grk_amd_surface* surf = nullptr, bool host_rules = false, const ResidentStream* res = nullptr)
{
    host_rules = host_rules || !pixels_on_device;
    // header -> view plan -> destination plan: every refusal that needs no byte of a packet
    grk_amd_stream_info info;
    std::string why;
    const char* pwhy = "";
    int rc = GRK_AMD_OK;
    if (res) info = *res->info;
    else rc = read_stream_header(cs, len, info, why);
    if (rc) return fail(c, rc, why.c_str());
    ViewPlan plan;
    rc = plan_image_view(info, view, plan, &pwhy);
    if (rc) return fail(c, rc, pwhy);
    // (a host destination's copy on the device is the context's own allocation: aligned far beyond 4 bytes)
    ImageDestIn in{c->dec_layout, c->dec_upsample, pixels_on_device != 0, cap, pixels_on_device ? (uint32_t)((uintptr_t)pixels & 3u) : 0u,
                         surf && surface_direct_allowed()};
    ImageDest d;
    rc = plan_image_dest(info, plan, in, surf, d, &pwhy);
    if (rc) return fail(c, rc, pwhy);
    // the coded buffer.  Where the tile-parts lie: found up front only when the upload depends on it (a view of every tile finds
    // them beside its upload, as the packets are read)
    std::vector<StreamPart> parts;
    if (res && !d.all) return fail(c, GRK_AMD_ERR_UNSUPPORTED, "a view of a codestream in device memory");
    if (!d.all) {
        rc = locate_stream_parts(cs, len, info, parts, why);
        if (rc) return fail(c, rc, why.c_str());
    }
    CodedPlan coded;
    plan_coded(len, info.num_layers, d.all, plan.tiles, parts, coded);
    HIP_TRY(c, hipSetDevice(c->device), "set device");
    rc = join_side(c); if (rc) return rc;
    // the upload, the packet headers meanwhile
    if (!res) HIP_TRY(c, c->img_coded.ensure(coded.coded_cap + 64), "alloc the coded buffer");
    void* coded_buf = res ? const_cast<void*>(res->d_cs) : c->img_coded.p;
    StreamTable tab;
    int rrc = GRK_AMD_OK;
    bool refined = false;                  // the table is the refine reader's
    if (res) {
        tab = std::move(*res->tab);
        refined = !tab.segments.empty();   // (read_device.hip asks for an HT file's segments only behind that reader)
        if (tab.appendix_bytes) {
            if (!res->d_moves || !tab.moves.empty()) return fail(c, GRK_AMD_ERR_INVALID, "an appendix without its moves in device memory");
            HIP_TRY(c, c->img_coded.ensure(coded.coded_cap + 64), "alloc the coded buffer");
            coded_buf = c->img_coded.p;
            HIP_TRY(c, hipMemcpyAsync(coded_buf, res->d_cs, len, hipMemcpyDeviceToDevice, c->stream), "stage the codestream");
            if (res->staged) *res->staged += len;
        }
    } else {
        const uint32_t threads = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
        std::thread reader([&]() {
            if (d.all) rrc = locate_stream_parts(cs, len, info, parts, why);
            // (an HT file whose blocks have refinement passes is read a second time in here, by the reader that takes them)
            if (!rrc) rrc = read_decode_packets(cs, len, info, parts, d.all ? nullptr : &plan.tiles, plan.reduce, threads, tab, why, &refined);
        });
        for (size_t i = 0; i < coded.copies.size() && !rc; ++i)
            rc = copy_h2d(c, (uint8_t*)c->img_coded.p + coded.copies[i].to, cs + coded.copies[i].from, coded.copies[i].n);
        reader.join();
    }
    if (rc) return rc;
    if (rrc) return fail(c, rrc, why.c_str());
    // only the packets show that an HT file has refinement segments: the destination's plan again, now with segment lists (int32
    // planes) and no region decoder
    rc = replan_for_refinement(info, plan, in, surf, tab, refined, d, &pwhy);
    if (rc) return fail(c, rc, pwhy);
    if (!res) { c->img_counters[0] += plan.tiles.size(); c->img_counters[1] += coded.up_len; }
    std::vector<uint64_t> unit_row;
    rc = rebase_table(tab, len, d.all, plan.tiles, parts, coded, d, unit_row, &pwhy);
    if (rc) return fail(c, rc, pwhy);
    const uint64_t coded_bytes = coded.coded_bytes;
    // (from here on the call only queues work; the small tables below are uploaded with blocking copies into buffers that an
    //  earlier call's kernels may still read)
    HIP_TRY(c, hipStreamSynchronize(c->stream), "sync");
    if (res && tab.appendix_bytes) {
        if (res->num_moves) {
            HIP_TRY(c, launch_t2dec_gather(res->d_moves, res->num_moves, (const uint8_t*)coded_buf, (uint8_t*)coded_buf + coded.up_len, c->stream), "launch gather");
            ++c->img_launches[0];
        }
    } else { rc = run_gather(c, tab.moves.data(), tab.moves.size(), coded_buf, (uint8_t*)coded_buf + coded.up_len); if (rc) return rc; }

    SavedSettings saved(c);
    c->dec_steps.clear();
    c->dec_reduce = plan.reduce;           // (the switch grk_amd_set_decode_reduce sets: every decode below delivers plan.units[u].w x h)
    rc = grk_amd_set_decode_qcd(c, info.qcd_words, info.base.irreversible ? info.num_qcd : 0); if (rc) return rc;
    // a batch's rows (`table`) and, for Part-1 blocks of several codeword segments, its segment list on the context
    std::vector<grk_amd_coded_block> table;
    std::vector<uint32_t> first;
    std::vector<grk_amd_segment> segs;
    auto batch_tables = [&](const uint32_t* units, size_t n) -> int {
        group_tables(tab, unit_row, units, n, d.want_segs, table, first, segs);
        if (!d.want_segs) return grk_amd_set_decode_segments(c, nullptr, nullptr, 0);
        return grk_amd_set_decode_segments(c, first.data(), segs.data(), (uint32_t)table.size());
    };
    if (d.route == ImageRoute::Direct || d.route == ImageRoute::Region) {
        // one tile: decoded straight into the destination (host pixels: grk_amd_decode_tiles repeats a group that leaves the int16
        // planes by itself) -- a window of it by the region decoder, whose cost follows the window
        rc = batch_tables(d.g.members[0].data(), d.g.members[0].size());
        if (rc) return rc;
        if (d.route == ImageRoute::Direct) return grk_amd_decode_tiles(c, &d.tp[0], 1, table.data(), coded_buf, coded_bytes, 1, pixels, pixels_on_device);
        return grk_amd_decode_region(c, &d.tp[0], table.data(), coded_buf, coded_bytes, 1, d.region[0], d.region[1], d.region[2], d.region[3], pixels,
                                     pixels_on_device);
    }
    HIP_TRY(c, c->img_status.ensure(64), "alloc status");
    if (d.route == ImageRoute::Runs) {
        // one tile of several runs: run by run straight into the run's planes; a decode into device pixels leaves its status to
        // the next one's, so it is kept as for the groups below
        if (pixels_on_device) HIP_TRY(c, hipMemsetAsync(c->img_status.p, 0, 4, c->stream), "clear status");
        for (uint32_t r = 0; r < d.nr; ++r) {
            const RunDest& rd = d.run_dest[r];
            rc = batch_tables(&r, 1); if (rc) return rc;
            uint8_t* const dst = (uint8_t*)pixels + rd.at;
            if (rd.beside) HIP_TRY(c, c->img_tiles.ensure(rd.bytes), "alloc a run's planes");
            rc = grk_amd_decode_tiles(c, &d.tp[r], 1, table.data(), coded_buf, coded_bytes, 1, rd.beside ? c->img_tiles.p : dst, pixels_on_device);
            if (rc) return rc;
            if (rd.beside) HIP_TRY(c, hipMemcpyAsync(dst, c->img_tiles.p, rd.bytes, hipMemcpyDeviceToDevice, c->stream), "copy a run's planes");
            if (pixels_on_device)
                HIP_TRY(c, launch_t2dec_or_status((unsigned int*)c->img_status.p, (const unsigned int*)c->flag.p, false, c->stream), "keep status");
        }
        if (pixels_on_device)
            HIP_TRY(c, launch_t2dec_or_status((unsigned int*)c->flag.p, (const unsigned int*)c->img_status.p, true, c->stream), "hand over status");
        return GRK_AMD_OK;
    }
    // a batch (`table`: its rows) into device memory at dst, its status kept in the image's
    auto decode_group = [&](const grk_amd_tile_params& p, uint32_t n, void* dst) -> int {
        int drc = grk_amd_decode_tiles(c, &p, n, table.data(), coded_buf, coded_bytes, 1, dst, 1); if (drc) return drc;
        // The int16-plane rule (include/grok_amd.h, grk_amd_set_decode_planes16).  A decode into a device buffer does not repeat
        // itself: with host pixels this call joins behind a group that may use those planes, reads its status and repeats it
        // with int32 planes; with device pixels the status goes to grk_amd_decode_status like any other
        if (host_rules && c->dec_planes16 && group_checks_planes16(d, p)) {
            drc = grk_amd_decode_status(c);
            if (drc == GRK_AMD_ERR_RANGE) {
                c->dec_planes16 = false;
                drc = grk_amd_decode_tiles(c, &p, n, table.data(), coded_buf, coded_bytes, 1, dst, 1);
                c->dec_planes16 = true;
            }
            if (drc) return drc;
        }
        HIP_TRY(c, launch_t2dec_or_status((unsigned int*)c->img_status.p, (const unsigned int*)c->flag.p, false, c->stream), "keep status");
        return GRK_AMD_OK;
    };
    // The image on the device: the caller's, or the context's copy of a host destination.  A host surface travels both ways (what is
    // no sample stays), and so does the extent of a pixel layout (what the caller has in its gaps goes up first)
    const bool surface = d.route == ImageRoute::Surface;
    uint8_t* d_img = (uint8_t*)pixels;
    if (!pixels_on_device) {
        HIP_TRY(c, c->img_pixels.ensure(d.total), surface ? "alloc the surface" : "alloc the image"); d_img = (uint8_t*)c->img_pixels.p;
        if (surface || d.upload_image) { rc = copy_h2d(c, d_img, pixels, d.total); if (rc) return rc; }
    }
    HIP_TRY(c, c->img_tiles.ensure(d.group_bytes), surface ? "alloc a group's units" : "alloc a group's tiles");
    HIP_TRY(c, c->img_rects.ensure(d.places_room), surface ? "alloc origins" : "alloc places");
    if (!surface || !d.places.empty())
        HIP_TRY(c, hipMemcpy(c->img_rects.p, d.places.data(), d.places.size() * 4, hipMemcpyHostToDevice), surface ? "upload origins" : "upload places");
    HIP_TRY(c, hipMemsetAsync(c->img_status.p, 0, 4, c->stream), "clear status");
    for (const FillRect& f : d.fills)
        HIP_TRY(c, launch_t2dec_fill(FillArgs{d_img + f.comp * d.kstep, f.x0, f.y0, f.w, f.h, d.bps, f.value, d.ipx.xstep, d.ipx.row}, c->stream), "launch fill");
    for (const ImageGroup& G : d.groups) {
        // (a surface's runs that are a pixel layout: through it straight onto the surface)
        for (uint32_t u : G.in_place) {
            const SurfaceRoute& r = d.surf_route[u % d.nr];
            c->dec_layout = r.layout;
            rc = batch_tables(&u, 1); if (rc) return rc;
            rc = decode_group(d.tp[u], 1, d_img + r.at); if (rc) return rc;
            ++c->surf_counters[0];
        }
        if (G.skip) continue;
        // the batch into staging -- tight units in the same kind of layout as the image's --, then its units of one run: one launch
        c->dec_layout = d.tile_layout;
        rc = batch_tables(G.units.data(), G.units.size()); if (rc) return rc;
        rc = decode_group(G.p, (uint32_t)G.units.size(), c->img_tiles.p); if (rc) return rc;
        for (const ImageLaunch& l : G.launches) {
            const uint8_t* const staged = (const uint8_t*)c->img_tiles.p + l.seg.first * G.unit_size;
            const uint32_t* const places = (const uint32_t*)c->img_rects.p + 2 * (G.place_at + l.seg.first);
            if (surface) {
                rc = queue_surface_kernel(c, true, d.rs, plan.runs[l.seg.run], d_img, const_cast<uint8_t*>(staged), l.seg.count, G.uw, G.uh, places);
                if (rc) return rc;
                continue;
            }
            if (d.up)
                HIP_TRY(c, launch_t2dec_upsample(UpsampleArgs{staged, l.seg.count, G.uw, G.uh, l.ncomp, l.bps, places, l.dx, l.dy, d_img + l.at, info.layout.x0,
                                                              info.layout.y0, l.w, l.h, d.ipx.xstep, l.row, l.kstep}, c->stream), "launch upsampling placement");
            else
                HIP_TRY(c, launch_t2dec_place(PlaceArgs{staged, l.seg.count, G.uw, G.uh, l.ncomp, l.bps, (const int32_t*)places, d_img + l.at, l.w, l.h, l.row,
                                                        l.kstep}, c->stream), "launch placement");
            ++c->img_launches[1];
        }
        if (surface) c->surf_counters[1] += G.units.size();
    }
    HIP_TRY(c, launch_t2dec_or_status((unsigned int*)c->flag.p, (const unsigned int*)c->img_status.p, true, c->stream), "hand over status");
    if (pixels_on_device) return GRK_AMD_OK;
    rc = copy_d2h(c, pixels, d_img, d.total); if (rc) return rc;
    return grk_amd_decode_status(c);
}

int decode_resident(grk_amd_ctx* c, const void* d_cs, uint64_t len, const grk_amd_stream_info& info, StreamTable& tab, void* pixels, uint64_t cap,
                    int pixels_on_device)
{
    const ResidentStream res{d_cs, &info, &tab, nullptr, 0, nullptr};
    return decode_view(c, nullptr, len, nullptr, pixels, cap, pixels_on_device, nullptr, false, &res);
}

int decode_resident_moves(grk_amd_ctx* c, const void* d_cs, uint64_t len, const grk_amd_stream_info& info, StreamTable& tab, const grk_amd_tp_segment* d_moves,
                          uint64_t num_moves, uint64_t* staged, void* pixels, uint64_t cap, int pixels_on_device)
{
    const ResidentStream res{d_cs, &info, &tab, d_moves, num_moves, staged};
    return decode_view(c, nullptr, len, nullptr, pixels, cap, pixels_on_device, nullptr, false, &res);
}

// what the three whole-image entry points refuse on the context (`reduced`: the text behind the entry point's name)
int refuse_context(grk_amd_ctx* c, const char* name, const char* reduced)
{
    if (c->dec_reduce) return fail(c, GRK_AMD_ERR_UNSUPPORTED, (std::string(name) + reduced).c_str());
    if (!c->dec_kids.empty()) return fail(c, GRK_AMD_ERR_UNSUPPORTED, (std::string(name) + " on a context with a decode sequence (grk_amd_set_decode_pipelining)").c_str());
    return GRK_AMD_OK;
}

extern "C" int grk_amd_decode_image(grk_amd_ctx* c, const uint8_t* cs, uint64_t len, void* pixels, uint64_t cap, int pixels_on_device)
{
    if (!c || !cs || !pixels) return GRK_AMD_ERR_INVALID;
    const int rc = refuse_context(c, "grk_amd_decode_image", " at reduced resolution"); if (rc) return rc;
    return decode_view(c, cs, len, nullptr, pixels, cap, pixels_on_device);
}

// grk_amd_decode_surface behind its null checks, and the way in of grk_amd_decode_packed (packed.cpp: `name`), whose surface is the
// context's own three planes: in device memory, under a host destination's rules where the caller's frame lies on the host
int decode_onto_surface(grk_amd_ctx* c, const char* name, const uint8_t* cs, uint64_t len, const grk_amd_surface* surface, void* pixels, uint64_t cap,
                        int pixels_on_device, bool host_rules)
{
    const int rc = refuse_context(c, name, " at reduced resolution"); if (rc) return rc;
    return decode_view(c, cs, len, nullptr, pixels, cap, pixels_on_device, surface, host_rules);
}

extern "C" int grk_amd_decode_surface(grk_amd_ctx* c, const uint8_t* cs, uint64_t len, const grk_amd_surface* surface, void* pixels, uint64_t cap,
                                      int pixels_on_device)
{
    if (!c || !cs || !pixels || !surface) return GRK_AMD_ERR_INVALID;
    return decode_onto_surface(c, "grk_amd_decode_surface", cs, len, surface, pixels, cap, pixels_on_device, false);
}

extern "C" int grk_amd_decode_image_view(grk_amd_ctx* c, const uint8_t* cs, uint64_t len, const grk_amd_image_view* view, void* pixels, uint64_t cap,
                                         int pixels_on_device)
{
    if (!c || !cs || !pixels) return GRK_AMD_ERR_INVALID;
    // (the view's reduce is the call's own parameter: the context's switch is the tile-level calls')
    const int rc = refuse_context(c, "grk_amd_decode_image_view", " on a context set to a reduced resolution (grk_amd_set_decode_reduce): the view carries its own");
    if (rc) return rc;
    return decode_view(c, cs, len, view, pixels, cap, pixels_on_device);
}
