// grok_amd/csrc/surface.cpp -- a video surface (NV12, I420, NV16 ...; include/grok_amd.h: grk_amd_surface) into a codestream
// (grk_amd_encode_surface), the two surface kernels as calls of their own, and what the decode side (decode_image.cpp:
// grk_amd_decode_surface) shares with it.  The units and groups are grk_amd_encode_image_subsampled's (image.h): a unit is a tile's
// run of components of one size, the units are grouped by geometry, a group is one grk_amd_encode_tiles batch.  Where a unit's pixels
// come from is the plan's word (surface_plan.h): the surface itself through a pixel layout, or tight planes that KS cut out of it --
// which units are staged, their origins and the launches are plan_surface_staging's, the one plan that the decode side
// (decode_image_plan.cpp) uses too.
#include "context.h"
#include "image.h"
#include "surface_plan.h"

using namespace grk_amd;

int queue_surface_kernel(grk_amd_ctx* c, bool place, const ResolvedSurface& rs, const CompRun& run, void* d_surface, void* d_tiles,
                         uint32_t count, uint32_t w, uint32_t h, const uint32_t* d_origins)
{
    SurfaceArgs a{};
    a.surface = (uint8_t*)d_surface; a.tiles = (uint8_t*)d_tiles;
    a.nunits = count; a.w = w; a.h = h; a.ncomp = run.count; a.bps = rs.bps;
    a.origins = d_origins;
    for (uint32_t k = 0; k < run.count && k < 4; ++k) {
        const SurfacePlane& p = rs.comp[run.first + k];
        a.comp[k] = SurfaceKernelComp{p.offset, p.row_pitch, p.step, p.shift};
    }
    HIP_TRY(c, place ? launch_surface_place(a, c->stream) : launch_surface_cut(a, c->stream), place ? "launch surface placement" : "launch surface cut");
    ++c->surf_counters[2];
    return GRK_AMD_OK;
}

extern "C" uint64_t grk_amd_surface_counters(grk_amd_ctx* c, int which)
{
    return c && which >= 0 && which < 3 ? c->surf_counters[which] : 0;
}

// ---- the kernels alone ---------------------------------------------------------------------------------------------------------
static int surface_kernel_device(grk_amd_ctx* c, bool place, void* surface, uint64_t surface_bytes, const grk_amd_surface_comp* comps, uint32_t ncomp,
                                 uint32_t bps, uint32_t nunits, uint32_t w, uint32_t h, const uint32_t* origins, void* tiles)
{
    if (!c || !surface || !comps || !origins || !tiles || !ncomp || ncomp > 4 || (bps != 1 && bps != 2) || !nunits || nunits > 65535 || !w || !h)
        return GRK_AMD_ERR_INVALID;
    ResolvedSurface rs;
    rs.bps = bps;
    uint64_t ox = 0, oy = 0;                         // the farthest origin: every unit is of one size
    for (uint32_t u = 0; u < nunits; ++u) { ox = std::max<uint64_t>(ox, origins[2 * u]); oy = std::max<uint64_t>(oy, origins[2 * u + 1]); }
    for (uint32_t k = 0; k < ncomp; ++k) {
        const grk_amd_surface_comp& sc = comps[k];
        const uint32_t step = sc.step ? sc.step : 1u;
        if (step > 4 || sc.offset % bps || sc.row_pitch % bps || (sc.offset | sc.row_pitch) >> 48) return fail(c, GRK_AMD_ERR_INVALID, "surface: a component's step, offset or pitch");
        if (sc.shift >= 8 * bps) return fail(c, GRK_AMD_ERR_INVALID, "surface: a shift of the whole container");
        // the component as far as the units reach: rows that do not run into the next, the last sample inside the surface
        const uint64_t cols = ox + w, rows = oy + h, row_span = ((cols - 1) * step + 1) * bps;
        if (rows > 1 && sc.row_pitch < row_span) return fail(c, GRK_AMD_ERR_INVALID, "surface: a row pitch is smaller than a row");
        if (sc.offset + (rows - 1) * sc.row_pitch + row_span > surface_bytes) return fail(c, GRK_AMD_ERR_INVALID, "surface: a unit outside the surface");
        rs.comp.push_back(SurfacePlane{sc.offset, sc.row_pitch, cols, rows, 0, 0, step, sc.shift});
    }
    if (place) {
        const char* why = "";
        // (of what the units cover: rectangles of the components' top-left cols x rows)
        if (check_surface_disjoint(rs, &why)) return fail(c, GRK_AMD_ERR_INVALID, why);
    }
    HIP_TRY(c, hipSetDevice(c->device), "set device");
    HIP_TRY(c, hipStreamSynchronize(c->stream), "sync");          // (the origins' device copy may still be read by an earlier call)
    HIP_TRY(c, c->img_rects.ensure((size_t)nunits * 8), "alloc origins");
    HIP_TRY(c, hipMemcpy(c->img_rects.p, origins, (size_t)nunits * 8, hipMemcpyHostToDevice), "upload origins");
    return queue_surface_kernel(c, place, rs, CompRun{0, ncomp, false}, surface, tiles, nunits, w, h, (const uint32_t*)c->img_rects.p);
}

extern "C" int grk_amd_surface_cut_device(grk_amd_ctx* c, const void* surface, uint64_t surface_bytes, const grk_amd_surface_comp* comps, uint32_t ncomp,
                                          uint32_t bps, uint32_t nunits, uint32_t w, uint32_t h, const uint32_t* origins, void* tiles)
{
    return surface_kernel_device(c, false, const_cast<void*>(surface), surface_bytes, comps, ncomp, bps, nunits, w, h, origins, tiles);
}

extern "C" int grk_amd_surface_place_device(grk_amd_ctx* c, const void* tiles, uint32_t nunits, uint32_t w, uint32_t h, uint32_t ncomp, uint32_t bps,
                                            const uint32_t* origins, const grk_amd_surface_comp* comps, void* surface, uint64_t surface_bytes)
{
    return surface_kernel_device(c, true, surface, surface_bytes, comps, ncomp, bps, nunits, w, h, origins, const_cast<void*>(tiles));
}

// ---- surface -> codestream -----------------------------------------------------------------------------------------------------
bool surface_direct_allowed()
{
    const char* const e = std::getenv("GRK_AMD_SURFACE_DIRECT");
    return !(e && std::strcmp(e, "0") == 0);
}

namespace {

// One grk_amd_encode_tiles call of a surface: a unit read in place through its run's layout, or a group's staged units
struct SurfaceBatch { grk_amd_tile_params p; std::vector<uint32_t> units; bool in_place; size_t group, origin_at; bool counted; };

// A surface resolved, routed and staged for encoding -- what grk_amd_encode_surface and grk_amd_encode_surface_rate share: the
// units [tile][run] and their groups, each run's route, the staging plan (surface_plan.h), the surface on the device, and the
// batches in the order they are coded: group after group, a group's in-place units first, then its staged units as one batch.
struct SurfaceJob {
    grk_amd_ctx* c;
    ResolvedSurface rs;
    std::vector<CompRun> runs;
    std::vector<grk_amd_tile_params> units;
    UnitGroups g;
    std::vector<SurfaceRoute> route;
    SurfaceStaging st;
    uint8_t* d_surf = nullptr;
    std::vector<SurfaceBatch> batches;
    std::vector<uint64_t> row_at;                            // unit u's rows start at row_at[u]

    int open(const grk_amd_image_layout* im, const grk_amd_tile_params* base, const uint8_t* comp_dx, const uint8_t* comp_dy,
             const grk_amd_surface* surface, const void* pixels, uint64_t cap, int pixels_on_device)
    {
        {
            const char* why = "";
            const int rc = resolve_surface(im, base, comp_dx, comp_dy, surface, rs, &why);
            if (rc) return fail(c, rc, why);
        }
        if (rs.bytes > cap) return fail(c, GRK_AMD_ERR_OVERFLOW, "surface: it does not fit `cap`");
        const int64_t nt = grk_amd_layout_num_tiles(im);
        if (nt < 0) return (int)nt;
        const uint32_t ntiles = (uint32_t)nt, nc = base->num_comps;
        runs = comp_runs(nc, base->mct != 0, comp_dx, comp_dy);
        const uint32_t nr = (uint32_t)runs.size();
        for (uint32_t t = 0; t < ntiles; ++t)
            for (uint32_t k = 0; k < nr; ++k) {
                grk_amd_tile_params p{};
                int rc = grk_amd_layout_tile_comp(im, base, comp_dx[runs[k].first], comp_dy[runs[k].first], t, &p);
                if (rc) return rc;
                p.num_comps = (uint16_t)runs[k].count;
                p.mct = runs[k].mct ? 1 : 0;
                units.push_back(p);
                rc = add_unit(g, p);
                if (rc) return rc;
            }
        HIP_TRY(c, hipSetDevice(c->device), "set device");
        // the surface on the device: the caller's, or a copy of a host surface's extent
        d_surf = (uint8_t*)const_cast<void*>(pixels);
        if (!pixels_on_device) {
            HIP_TRY(c, c->img_pixels.ensure(rs.bytes + 16), "alloc the surface");
            d_surf = (uint8_t*)c->img_pixels.p;
            const int rc = copy_h2d(c, d_surf, pixels, rs.bytes); if (rc) return rc;
        }
        // each run's route; what is staged (surface_plan.h): the units group after group, within a group run by run, their origins in that order
        const bool direct = surface_direct_allowed();
        route.resize(nr);
        for (uint32_t k = 0; k < nr; ++k)
            route[k] = plan_surface_run(rs, runs[k], ntiles == 1, false, direct, cap, (uint32_t)((uintptr_t)d_surf & 3u));
        st = plan_surface_staging(g.members, route, rs, runs, units);
        if (!st.origins.empty()) {
            HIP_TRY(c, hipStreamSynchronize(c->stream), "sync");      // (the buffers below may still be read by an earlier call's kernels)
            HIP_TRY(c, c->img_tiles.ensure(st.group_bytes), "alloc a group's units");
            HIP_TRY(c, c->img_rects.ensure(st.origins.size() * 4), "alloc origins");
            HIP_TRY(c, hipMemcpy(c->img_rects.p, st.origins.data(), st.origins.size() * 4, hipMemcpyHostToDevice), "upload origins");
        }
        row_at.assign(units.size() + 1, 0);
        for (size_t u = 0; u < units.size(); ++u) row_at[u + 1] = row_at[u] + (uint64_t)g.geoms[g.of[u]].blocks_per_comp * units[u].num_comps;
        size_t origin_at = 0;
        for (size_t k = 0; k < g.members.size(); ++k) {
            for (uint32_t u : g.members[k])
                if (route[u % nr].in_place) batches.push_back(SurfaceBatch{units[u], {u}, true, k, 0, false});
            const std::vector<uint32_t>& S = st.staged[k];
            if (S.empty()) continue;
            batches.push_back(SurfaceBatch{units[S[0]], S, false, k, origin_at, false});
            origin_at += S.size();
        }
        return GRK_AMD_OK;
    }

    // batch b through grk_amd_encode_tiles: the surface itself through the run's layout, or staged planes (cut out of the surface
    // here, every time: the groups share the staging buffer) in the default one -- never the caller's setting, which the public
    // call puts back (KeepLayout)
    int front(size_t b, grk_amd_coded_block* table, uint64_t* total)
    {
        SurfaceBatch& B = batches[b];
        const void* d_px;
        if (B.in_place) {
            const SurfaceRoute& r = route[B.units[0] % runs.size()];
            c->enc_layout = r.layout;
            d_px = d_surf + r.at;
        } else {
            const size_t unit_size = (size_t)B.p.tile_w * B.p.tile_h * B.p.num_comps * rs.bps;
            for (const RunSegment& s : st.segments[B.group]) {
                const int rc = queue_surface_kernel(c, false, rs, runs[s.run], d_surf, (uint8_t*)c->img_tiles.p + s.first * unit_size, s.count,
                                                    B.p.tile_w, B.p.tile_h, (const uint32_t*)c->img_rects.p + 2 * (B.origin_at + s.first));
                if (rc) return rc;
            }
            c->enc_layout = grk_amd_pixel_layout{};
            d_px = c->img_tiles.p;
        }
        const int rc = grk_amd_encode_tiles(c, &B.p, (uint32_t)B.units.size(), d_px, 1, table, total);
        if (rc) return rc;
        if (!B.counted) { c->surf_counters[B.in_place ? 0 : 1] += B.units.size(); B.counted = true; }
        return GRK_AMD_OK;
    }
};

} // namespace

// grk_amd_encode_surface behind its null checks -- and grk_amd_encode_packed's way in (packed.cpp), whose surface is the context's
// own three planes in device memory
int64_t encode_surface_job(grk_amd_ctx* c, const grk_amd_image_layout* im, const grk_amd_tile_params* base, const uint8_t* comp_dx,
                           const uint8_t* comp_dy, const grk_amd_surface* surface, const void* pixels, uint64_t cap, int pixels_on_device,
                           uint32_t flags, uint8_t* out, uint64_t out_cap, void** d_file)
{
    // (a plain encode drops nothing: per-block zero bit-planes are the rate-targeted call's; the device file has no host writer to go to)
    if (d_file && (flags & GRK_AMD_CS_BLOCK_MSBS)) return fail(c, GRK_AMD_ERR_UNSUPPORTED, "per-block zero bit-planes: the host writers only");
    // (a division into tile-parts that neither route writes is refused before any work)
    { const int64_t nt = grk_amd_layout_num_tiles(im); if (nt < 0) return nt; const int np = image_division(c, flags, base, (uint32_t)nt); if (np < 0) return np; }
    SurfaceJob job{c};
    int rc = job.open(im, base, comp_dx, comp_dy, surface, pixels, cap, pixels_on_device);
    if (rc) return rc;
    KeepLayout keep{c->enc_layout, c->enc_layout};
    // Tier-2 on the device (encode_joint_device, image.h; GRK_AMD_IMAGE_T2=host: the host writer below, where a surface beyond the
    // device writer's tables goes as well -- a file in device memory has no such way out): every batch coded without a table
    if (d_file || !image_t2_host()) {
        JointT2Call call{im, base, comp_dx, comp_dy, flags, (uint32_t)job.runs.size(), &job.g, {}, {}};
        for (const SurfaceBatch& B : job.batches) call.batches.push_back(B.units);
        call.front = [&](size_t b) -> int {
            const int fr = job.front(b, nullptr, nullptr);
            // (the next batch's cut writes the staging buffer this one's level 0 reads: in stream order whichever stream read it)
            return fr ? fr : grk_amd_stream_wait_pixels(c, c->stream);
        };
        const int64_t n = encode_joint_device(c, call, out, out_cap, d_file);
        if (d_file || n != GRK_AMD_ERR_UNSUPPORTED) return n;
    }
    std::vector<grk_amd_coded_block> rows(job.row_at.back()), table;
    std::vector<uint8_t> coded;
    // every batch's rows and bytes to the host
    for (size_t b = 0; b < job.batches.size(); ++b) {
        const std::vector<uint32_t>& batch = job.batches[b].units;
        const uint64_t bpu = job.row_at[batch[0] + 1] - job.row_at[batch[0]];
        table.resize(bpu * batch.size());
        uint64_t total = 0;
        rc = job.front(b, table.data(), &total);
        if (rc) return rc;
        const size_t at = coded.size();
        coded.resize(at + total);
        rc = grk_amd_fetch_coded(c, coded.data() + at, total);
        if (rc) return rc;
        for (size_t i = 0; i < batch.size(); ++i)
            for (uint64_t k = 0; k < bpu; ++k) { rows[job.row_at[batch[i]] + k] = table[i * bpu + k]; rows[job.row_at[batch[i]] + k].offset += at; }
    }
    const int64_t n = grk_amd_write_codestream_subsampled(im, base, comp_dx, comp_dy, rows.data(), coded.data(), flags, out, out_cap);
    if (n >= 0) ++c->route_counters[1];
    return n;
}

extern "C" int64_t grk_amd_encode_surface_device(grk_amd_ctx* c, const grk_amd_image_layout* im, const grk_amd_tile_params* base,
                                                 const uint8_t* comp_dx, const uint8_t* comp_dy, const grk_amd_surface* surface,
                                                 const void* pixels, uint64_t cap, int pixels_on_device, uint32_t flags, void** d_file)
{
    if (!c || !im || !base || !comp_dx || !comp_dy || !surface || !pixels || !d_file) return GRK_AMD_ERR_INVALID;
    *d_file = nullptr;
    return encode_surface_job(c, im, base, comp_dx, comp_dy, surface, pixels, cap, pixels_on_device, flags, nullptr, 0, d_file);
}

extern "C" int64_t grk_amd_encode_surface(grk_amd_ctx* c, const grk_amd_image_layout* im, const grk_amd_tile_params* base,
                                          const uint8_t* comp_dx, const uint8_t* comp_dy, const grk_amd_surface* surface,
                                          const void* pixels, uint64_t cap, int pixels_on_device, uint32_t flags, uint8_t* out, uint64_t out_cap)
{
    if (!c || !im || !base || !comp_dx || !comp_dy || !surface || !pixels || !out) return GRK_AMD_ERR_INVALID;
    return encode_surface_job(c, im, base, comp_dx, comp_dy, surface, pixels, cap, pixels_on_device, flags, out, out_cap);
}

// the same for grk_amd_encode_surface_rate and grk_amd_encode_packed_rate -- and, with a quality goal (image.h), their _quality twins
int64_t encode_surface_rate_job(grk_amd_ctx* c, const grk_amd_image_layout* im, const grk_amd_tile_params* base, const uint8_t* comp_dx,
                                const uint8_t* comp_dy, const grk_amd_surface* surface, const void* pixels, uint64_t cap, int pixels_on_device,
                                uint32_t flags, const grk_amd_rate* rate, uint8_t* out, uint64_t out_cap, grk_amd_rate_result* result,
                                const QualityGoal* quality, void** d_file)
{
    { const int rr = rate_refusal(c, rate); if (rr) return rr; }
    if (flags & GRK_AMD_CS_TP(3)) return fail(c, GRK_AMD_ERR_UNSUPPORTED, "GRK_AMD_CS_TP: tiles divided into tile-parts are not written by the rate- and quality-targeted calls");
    flags |= GRK_AMD_CS_BLOCK_MSBS;
    SurfaceJob job{c};
    const int rc = job.open(im, base, comp_dx, comp_dy, surface, pixels, cap, pixels_on_device);
    if (rc) return rc;
    KeepLayout keep{c->enc_layout, c->enc_layout};
    RateJointCall call{base, rate, {}, {}, {}, {}, quality};
    for (size_t u = 0; u < job.units.size(); ++u) call.unit_blocks.push_back(job.row_at[u + 1] - job.row_at[u]);
    for (const SurfaceBatch& B : job.batches) call.batches.push_back(RateBatch{B.p, B.units});
    call.front = [&](size_t b, grk_amd_coded_block* table, uint64_t* total) { return job.front(b, table, total); };
    call.write = [&](const grk_amd_coded_block* rows, const uint8_t* coded, uint8_t* o, uint64_t ocap) -> int64_t {
        return grk_amd_write_codestream_subsampled(im, base, comp_dx, comp_dy, rows, coded, flags, o, ocap);
    };
    if (d_file) {
        // Tier-2 on the device, the general zero-bit-plane tree asked for by the call itself (never through the flag); GRK_AMD_IMAGE_T2
        // is not consulted: a file in device memory has no host writer to go to
        JointT2Call t2{im, base, comp_dx, comp_dy, flags & ~(uint32_t)GRK_AMD_CS_BLOCK_MSBS, (uint32_t)job.runs.size(), &job.g, {}, {}};
        for (const SurfaceBatch& B : job.batches) t2.batches.push_back(B.units);
        const int64_t n = encode_rate_joint_device(c, call, t2, d_file, result);
        if (n >= 0) ++c->route_counters[0];
        return n;
    }
    return encode_rate_joint(c, call, out, out_cap, result);
}

extern "C" int64_t grk_amd_encode_surface_rate(grk_amd_ctx* c, const grk_amd_image_layout* im, const grk_amd_tile_params* base,
                                               const uint8_t* comp_dx, const uint8_t* comp_dy, const grk_amd_surface* surface,
                                               const void* pixels, uint64_t cap, int pixels_on_device, uint32_t flags,
                                               const grk_amd_rate* rate, uint8_t* out, uint64_t out_cap, grk_amd_rate_result* result)
{
    if (!c || !im || !base || !comp_dx || !comp_dy || !surface || !pixels || !out || !rate) return GRK_AMD_ERR_INVALID;
    return encode_surface_rate_job(c, im, base, comp_dx, comp_dy, surface, pixels, cap, pixels_on_device, flags, rate, out, out_cap, result);
}

extern "C" int64_t grk_amd_encode_surface_quality(grk_amd_ctx* c, const grk_amd_image_layout* im, const grk_amd_tile_params* base,
                                                  const uint8_t* comp_dx, const uint8_t* comp_dy, const grk_amd_surface* surface,
                                                  const void* pixels, uint64_t cap, int pixels_on_device, uint32_t flags,
                                                  const grk_amd_quality* quality, uint8_t* out, uint64_t out_cap, grk_amd_quality_result* result)
{
    if (!c || !im || !base || !comp_dx || !comp_dy || !surface || !pixels || !out || !quality) return GRK_AMD_ERR_INVALID;
    QualityTarget qt;
    const int rc = quality_target(c, quality, base->prec, quality_samples(*im, base->num_comps, comp_dx, comp_dy), result, qt);
    if (rc) return rc;
    return encode_surface_rate_job(c, im, base, comp_dx, comp_dy, surface, pixels, cap, pixels_on_device, flags, &qt.rate, out, out_cap, nullptr, &qt.goal);
}

// The rate- and quality-targeted calls that leave their file in device memory: the arguments, refusals and results of
// grk_amd_encode_surface_rate / _quality, `d_file` as grk_amd_encode_surface_device has it.  Tier-2 runs on the device in every round
// (KT1's general zero-bit-plane tree); no coded byte crosses the link (grk_amd_rate_device_counters).
extern "C" int64_t grk_amd_encode_surface_rate_device(grk_amd_ctx* c, const grk_amd_image_layout* im, const grk_amd_tile_params* base,
                                                      const uint8_t* comp_dx, const uint8_t* comp_dy, const grk_amd_surface* surface,
                                                      const void* pixels, uint64_t cap, int pixels_on_device, uint32_t flags,
                                                      const grk_amd_rate* rate, void** d_file, grk_amd_rate_result* result)
{
    if (!c || !im || !base || !comp_dx || !comp_dy || !surface || !pixels || !d_file || !rate) return GRK_AMD_ERR_INVALID;
    *d_file = nullptr;
    return encode_surface_rate_job(c, im, base, comp_dx, comp_dy, surface, pixels, cap, pixels_on_device, flags, rate, nullptr, 0, result, nullptr, d_file);
}

extern "C" int64_t grk_amd_encode_surface_quality_device(grk_amd_ctx* c, const grk_amd_image_layout* im, const grk_amd_tile_params* base,
                                                         const uint8_t* comp_dx, const uint8_t* comp_dy, const grk_amd_surface* surface,
                                                         const void* pixels, uint64_t cap, int pixels_on_device, uint32_t flags,
                                                         const grk_amd_quality* quality, void** d_file, grk_amd_quality_result* result)
{
    if (!c || !im || !base || !comp_dx || !comp_dy || !surface || !pixels || !d_file || !quality) return GRK_AMD_ERR_INVALID;
    *d_file = nullptr;
    QualityTarget qt;
    const int rc = quality_target(c, quality, base->prec, quality_samples(*im, base->num_comps, comp_dx, comp_dy), result, qt);
    if (rc) return rc;
    return encode_surface_rate_job(c, im, base, comp_dx, comp_dy, surface, pixels, cap, pixels_on_device, flags, &qt.rate, nullptr, 0, nullptr, &qt.goal, d_file);
}
