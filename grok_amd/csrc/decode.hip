// grok_amd/csrc/decode.hip -- decode: a call from the caller's table to its pixels (block decoding in decode_blocks.hip, inverse DWT,
// egress), regions, the stage entry points and the decode settings.
#include "decode_internal.h"

namespace {
// d_pixels != nullptr: the last level writes the pixels itself (K7 fused, out_bytes 1 or 2) and d_out is not touched;
// plan != nullptr: only what the window needs is synthesised, and d_pixels is the window (K7 fused required)
int run_idwt(grk_amd_ctx* c, uint32_t nplanes, const void* d_mallat, void* d_out, void* d_pixels = nullptr,
             uint32_t ntiles = 0, uint32_t out_bytes = 0, const RegionPlan* plan = nullptr, bool h16 = false, const PixelLayout* px = nullptr)
{
    const TileGeom& g = c->geom;
    const uint32_t L = g.p.num_levels;
    if (L == 0) {
        HIP_TRY(c, hipMemcpyAsync(d_out, d_mallat, (size_t)nplanes * g.plane_elems * 4, hipMemcpyDeviceToDevice, c->stream), "copy planes");
        return GRK_AMD_OK;
    }
    { const int rc = ensure_ll(c, nplanes); if (rc) return rc; }     // (the same ping-pong storage as the forward transform)
    ScopedTimer t(c, 6);
    const SampleRange r = sample_range(g.p);
    for (int32_t l = (int32_t)L - 1; l >= 0; --l) {
        // describe the level ...
        IdwtLevelArgs a{};
        a.cw = level_geom(g, (uint32_t)l).w; a.ch = level_geom(g, (uint32_t)l).h;
        a.px = level_geom(g, (uint32_t)l).x0 & 1u; a.py = level_geom(g, (uint32_t)l).y0 & 1u;
        const LLPlane from = ll_plane(c, (uint32_t)l + 1, d_out, (void*)d_mallat), to = ll_plane(c, (uint32_t)l, d_out, (void*)d_mallat);
        a.ll = (const int32_t*)from.p; a.ll_stride = from.stride; a.ll_pitch = from.pitch;
        a.mallat = (const int32_t*)d_mallat; a.m_stride = g.stride; a.m_pitch = g.plane_elems;
        a.out = (int32_t*)to.p; a.out_stride = to.stride; a.out_pitch = to.pitch;
        a.nplanes = nplanes;
        a.irreversible = g.p.irreversible;
        a.xcd = c->dwt_xcd;
        a.h16 = h16 ? 1 : 0; a.status = (unsigned int*)c->flag.p;
        a.pk = h16 && c->dwt_pk && !plan;            // (the block decoder flagged every coefficient outside the packed range)
        const bool fused = l == 0 && d_pixels;
        if (fused) {
            if (px && px->lay) set_px_out(a, *px);
            a.pixels = d_pixels; a.px_bytes = out_bytes;
            a.dc = r.dc; a.lo = r.lo; a.hi = r.hi;
            a.mct = g.p.mct;
        }
        // ... plan its kernel instance, strips, row segments and, for a region, the sub-grid that produces need[l] (decode_plan.h) ...
        const uint32_t zslots = fused ? ntiles * level_part_zslots(g.p.mct != 0, g.p.num_comps) : nplanes;
        const IdwtLevelShape shape = plan_idwt_level(IdwtLevelDesc{
            a.cw, a.ch, a.px, a.py, a.ll_stride, a.m_stride, a.out_stride, a.h16 != 0, a.pk != 0, a.irreversible != 0, zslots,
            plan != nullptr, plan ? plan->need[(uint32_t)l] : Rect{}, fused, a.px_bytes, a.lo, a.hi, a.mct != 0,
            a.px_lay, a.px_chan, a.px_row, a.px_tile, (uint32_t)((uintptr_t)a.pixels & 3u)});
        // ... fill what the kernel reads of it ...
        a.seg_pairs = shape.seg_pairs;
        a.strip0 = shape.strip0; a.nstrips = shape.nstrips; a.seg0 = shape.seg0; a.nsegs = shape.nsegs;
        a.wx0 = shape.wx0; a.wy0 = shape.wy0; a.wx1 = shape.wx1; a.wy1 = shape.wy1;
        if (a.cw == 0 || a.ch == 0) continue;       // (a level without samples, see run_dwt)
        // ... and launch
        if (l == 0 && c->dec_top_pending) {           // the top resolution's blocks are decoded on the side stream
            HIP_TRY(c, hipStreamWaitEvent(c->stream, c->ev_dec_top, 0), "wait for the top resolution's blocks");
            c->dec_top_pending = false;
        }
        if (fused) HIP_TRY(c, launch_idwt_level0_fused(a, shape, ntiles, g.p.num_comps, c->stream), "launch fused idwt level 0");
        else       HIP_TRY(c, launch_idwt_level(a, shape, c->stream), "launch idwt level");
    }
    return GRK_AMD_OK;
}

// the context's decode layout for `ntiles` outputs of w x h (0: the tile of the current geometry), or GRK_AMD_ERR_INVALID and the reason
int decode_layout(grk_amd_ctx* c, uint32_t w, uint32_t h, uint32_t ntiles, PixelLayout& px)
{
    const char* why = "";
    if (!resolve_pixel_layout(c->geom.p, &c->dec_layout, w, h, ntiles, px, &why)) return fail(c, GRK_AMD_ERR_INVALID, why);
    if (px.lay && (c->geom.p.prec + 7u) / 8u > 2) return fail(c, GRK_AMD_ERR_UNSUPPORTED, "pixel layout: samples of more than 16 bits leave in the default layout only");
    return GRK_AMD_OK;
}

int run_egress(grk_amd_ctx* c, uint32_t ntiles, const void* d_planes, void* d_pixels, uint32_t out_bytes, const PixelLayout& px)
{
    const TileGeom& g = c->geom;
    const SampleRange r = sample_range(g.p);
    EgressArgs a{};
    set_px_out(a, px);
    a.planes = (const int32_t*)d_planes; a.pixels = d_pixels;
    a.w = g.p.tile_w; a.h = g.p.tile_h; a.stride = g.stride; a.pitch = g.plane_elems;
    a.ncomp = g.p.num_comps; a.ntiles = ntiles;
    a.bytes_per_sample = out_bytes;
    a.dc = r.dc; a.lo = r.lo; a.hi = r.hi;
    a.mct = g.p.mct; a.irreversible = g.p.irreversible;
    ScopedTimer t(c, 7);
    HIP_TRY(c, launch_egress(a, egress_key(a.px_lay, a.bytes_per_sample, a.ncomp), c->stream), "launch egress");
    return GRK_AMD_OK;
}
} // namespace

int decode_impl(grk_amd_ctx* c, const grk_amd_tile_params* p, uint32_t ntiles, const grk_amd_coded_block* table, const void* coded,
                uint64_t coded_bytes, int coded_on_device, void* pixels, int pixels_on_device, const Rect* win, bool force32)
{
    if (!c || !p || !table || !coded || !pixels || ntiles == 0) return GRK_AMD_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device), "set device");
    int rc = join_side(c); if (rc) return rc;        // (the Mallat planes and the status word are shared with the encoder)
    // (the block decoders of the top resolution run on the side stream beside the rest: the two have to be dispatched side by side)
    if (c->overlap && c->side && c->seq_index < 0 && c->stream_probe && c->probed_main != c->stream && probe_streams(c) != GRK_AMD_OK) {
        c->stream_probe = 0; (void)hipGetLastError();
    }
    rc = ensure_geom(c, p, c->dec_reduce); if (rc) return rc;
    const TileGeom& g = c->geom;
    const uint32_t nplanes = ntiles * g.p.num_comps;
    if (g.reduce && !c->dec_seg_first.empty()) {     // the segment list is over the full tile's blocks
        const char* why = "";
        rc = reduce_segments((uint64_t)ntiles * g.p.num_comps, g.full_blocks_per_comp, g.blocks_per_comp, c->dec_seg_first, c->dec_segs,
                             c->red_seg_first, c->red_segs, &why);
        if (rc) return fail(c, rc, why);
    } else {
        c->red_seg_first.clear(); c->red_segs.clear();
    }
    const uint32_t bps = (g.p.prec + 7u) / 8u;
    const bool fuse_out = g.p.num_levels >= 1 && bps <= 2 && c->fuse_egress;
    // region decode: the blocks no sample of the window depends on are not decoded, the synthesis covers what is needed
    RegionPlan plan;
    grk_amd_ctx::DecUpload* up = nullptr;
    rc = stage_table(c, table, (uint64_t)g.blocks_per_comp * g.p.num_comps * ntiles, &up); if (rc) return rc;
    if (win) {
        if (ntiles != 1 || win->x0 >= win->x1 || win->y0 >= win->y1 || win->x1 > g.p.tile_w || win->y1 > g.p.tile_h)
            return fail(c, GRK_AMD_ERR_INVALID, "window outside the tile");
        if (!fuse_out) return fail(c, GRK_AMD_ERR_UNSUPPORTED, "region decode needs at least one DWT level and 8-/16-bit pixels");
        plan = plan_region(g, *win);
        skip_blocks_outside(g, plan, (grk_amd_coded_block*)up->p);
    }
    // the pixels' layout (grk_amd_set_decode_pixel_layout) for what this call writes: the window, the reduced tile, the tile
    PixelLayout px;
    rc = decode_layout(c, win ? win->x1 - win->x0 : 0, win ? win->y1 - win->y0 : 0, ntiles, px); if (rc) return rc;
    const void* d_coded = coded;
    if (!coded_on_device) {
        HIP_TRY(c, c->dec_coded.ensure(coded_bytes + 64), "alloc coded staging");
        rc = copy_h2d(c, c->dec_coded.p, coded, coded_bytes); if (rc) return rc;
        d_coded = c->dec_coded.p;
    }
    const size_t px_bytes = px.bytes;     // (the default layout: the tight window / tiles)
    void* d_px = pixels;
    if (!pixels_on_device) {
        HIP_TRY(c, c->dec_pixels.ensure(px_bytes), "alloc pixel staging");
        d_px = c->dec_pixels.p;
        // the extent comes back as one copy, gaps included -- and what the caller has in the gaps is to stay: it goes up first
        if (px.lay) { rc = copy_h2d(c, d_px, pixels, px_bytes); if (rc) return rc; }
    }
    if (!fuse_out) HIP_TRY(c, c->p0.ensure((size_t)nplanes * g.plane_elems * 4 + 256), "alloc planes");
    HIP_TRY(c, c->p1.ensure((size_t)nplanes * g.plane_elems * 4 + 256), "alloc Mallat planes");
    // 8-bit reversible HT tiles: int16 planes between K5b and K6 (both HBM-side halves of the decode move half the bytes).
    // Every coefficient and every synthesised LL sample of a stream that an 8-bit image produced fits (the encoder's
    // planes16_ok bound); a stream whose values do not is reported by decode_status (GRK_AMD_ERR_RANGE), and a synchronous
    // call decodes it again with int32 planes right here -- never other pixels.
    const bool h16 = decode_takes_planes16(c->dec_planes16, force32, fuse_out, g.p, !c->dec_seg_first.empty());
    {
        ScopedTimer t(c, 3);
        rc = p->reserved[0] ? run_t1_decode(c, ntiles, up, d_coded, coded_bytes, c->p1.p)
                            : run_ht_decode(c, ntiles, up, d_coded, coded_bytes, c->p1.p, h16, true);
        if (rc) return rc;
        // with at least one DWT level and 8-/16-bit pixels the last level writes the pixels itself (K7 fused): the
        // int32 image planes (4 bytes per sample written and read back) never exist
        if (fuse_out) {
            rc = run_idwt(c, nplanes, c->p1.p, nullptr, d_px, ntiles, bps, win ? &plan : nullptr, h16, &px); if (rc) return rc;
        } else {
            rc = run_idwt(c, nplanes, c->p1.p, c->p0.p); if (rc) return rc;
            rc = run_egress(c, ntiles, c->p0.p, d_px, bps, px); if (rc) return rc;
        }
    }
    if (!pixels_on_device) {
        rc = copy_d2h(c, pixels, d_px, px_bytes); if (rc) return rc;
        rc = check_decode_status(c);
        if (rc == GRK_AMD_ERR_RANGE && h16)           // (synchronous call: the exact path, at once)
            return decode_impl(c, p, ntiles, table, coded, coded_bytes, coded_on_device, pixels, pixels_on_device, win, true);
        return rc;
    }
    return GRK_AMD_OK;                 // (a window's adapted table lives in the context's pinned memory: nothing to wait for)
}

extern "C" {
int grk_amd_stage_dwt_inv(grk_amd_ctx* c, const grk_amd_tile_params* p, uint32_t nplanes, const void* d_mallat, void* d_out)
{
    const int rc = stage_enter(c, p, d_mallat && d_out, true); if (rc) return rc;
    return run_idwt(c, nplanes, d_mallat, d_out);
}

int grk_amd_stage_ht_decode(grk_amd_ctx* c, const grk_amd_tile_params* p, uint32_t ntiles,
                            const grk_amd_coded_block* table, const void* d_coded, uint64_t coded_bytes, void* d_mallat)
{
    int rc = stage_enter(c, p, table && d_coded && d_mallat && ntiles != 0, true); if (rc) return rc;
    grk_amd_ctx::DecUpload* up = nullptr;
    rc = stage_table(c, table, (uint64_t)c->geom.blocks_per_comp * c->geom.p.num_comps * ntiles, &up); if (rc) return rc;
    rc = p->reserved[0] ? run_t1_decode(c, ntiles, up, d_coded, coded_bytes, d_mallat)
                        : run_ht_decode(c, ntiles, up, d_coded, coded_bytes, d_mallat);
    if (rc) return rc;
    return check_decode_status(c);
}

// K5b's int16 stores and their range flag as a decode of an 8-bit reversible HT tile runs them (decode_impl's h16 conditions)
int grk_amd_stage_ht_decode16(grk_amd_ctx* c, const grk_amd_tile_params* p, uint32_t ntiles,
                              const grk_amd_coded_block* table, const void* d_coded, uint64_t coded_bytes, void* d_mallat16)
{
    const bool takes = c && p && !p->irreversible && p->prec <= 8 && !p->reserved[0] && c->dec_seg_first.empty();
    int rc = stage_enter(c, p, table && d_coded && d_mallat16 && ntiles != 0, true,
                         takes ? nullptr : "int16 planes are for reversible HT tiles of at most 8 bits without refinement passes");
    if (rc) return rc;
    grk_amd_ctx::DecUpload* up = nullptr;
    rc = stage_table(c, table, (uint64_t)c->geom.blocks_per_comp * c->geom.p.num_comps * ntiles, &up); if (rc) return rc;
    rc = run_ht_decode(c, ntiles, up, d_coded, coded_bytes, d_mallat16, true, false); if (rc) return rc;
    return check_decode_status(c);
}

int grk_amd_stage_egress(grk_amd_ctx* c, const grk_amd_tile_params* p, uint32_t ntiles, const void* d_planes, void* d_pixels)
{
    int rc = stage_enter(c, p, d_planes && d_pixels, false); if (rc) return rc;
    if (!ntiles) return GRK_AMD_ERR_INVALID;
    PixelLayout px;
    rc = decode_layout(c, 0, 0, ntiles, px); if (rc) return rc;
    return run_egress(c, ntiles, d_planes, d_pixels, (p->prec + 7u) / 8u, px);
}

int grk_amd_decode_region(grk_amd_ctx* c, const grk_amd_tile_params* p,
                          const grk_amd_coded_block* table, const void* coded, uint64_t coded_bytes, int coded_on_device,
                          uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, void* pixels, int pixels_on_device)
{
    const Rect win{x0, y0, x1, y1};
    return decode_impl(c, p, 1, table, coded, coded_bytes, coded_on_device, pixels, pixels_on_device, &win);
}

int grk_amd_set_decode_qcd(grk_amd_ctx* c, const uint16_t* words, uint32_t count)
{
    if (!c || (count && !words)) return GRK_AMD_ERR_INVALID;
    c->dec_qcd.assign(words, words + count);
    c->have_geom = false;                  // the per-block dequantisation scales are rebuilt on the next call
    return GRK_AMD_OK;
}

int grk_amd_set_decode_steps(grk_amd_ctx* c, const float* steps, uint32_t count)
{
    if (!c || (count && !steps)) return GRK_AMD_ERR_INVALID;
    c->dec_steps.assign(steps, steps + count);
    c->have_geom = false;                  // the per-block dequantisation scales are rebuilt on the next call
    return GRK_AMD_OK;
}

int grk_amd_set_decode_reduce(grk_amd_ctx* c, uint32_t reduce)
{
    if (!c) return GRK_AMD_ERR_INVALID;
    c->dec_reduce = reduce;                // checked against each call's number of levels (decode_impl -> ensure_geom)
    return GRK_AMD_OK;
}

int grk_amd_reduced_tile_rect(const grk_amd_tile_params* p, uint32_t reduce, uint32_t* x0, uint32_t* y0, uint32_t* w, uint32_t* h)
{
    if (!p || !x0 || !y0 || !w || !h) return GRK_AMD_ERR_INVALID;
    return reduced_tile_rect(*p, reduce, x0, y0, w, h);
}

int grk_amd_set_decode_segments(grk_amd_ctx* c, const uint32_t* first_segment, const grk_amd_segment* segments, uint32_t nblocks)
{
    if (!c || (nblocks && (!first_segment || (first_segment[nblocks] && !segments)))) return GRK_AMD_ERR_INVALID;
    c->dec_seg_first.clear(); c->dec_segs.clear();
    if (nblocks) {
        c->dec_seg_first.assign(first_segment, first_segment + nblocks + 1);
        c->dec_segs.assign(segments, segments + first_segment[nblocks]);
    }
    return GRK_AMD_OK;
}

int grk_amd_decode_status(grk_amd_ctx* c)
{
    if (!c) return GRK_AMD_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device), "set device");
    int rc = check_decode_status(c);
    for (grk_amd_ctx* k : c->dec_kids) {            // (a sequence: the frames decoded on the other contexts as well)
        const int kr = check_decode_status(k);
        if (kr && !rc) { rc = kr; c->err = k->err; }
    }
    return rc;
}

int grk_amd_set_decode_planes16(grk_amd_ctx* c, int on)
{
    if (!c) return GRK_AMD_ERR_INVALID;
    c->dec_planes16 = on != 0;
    return GRK_AMD_OK;
}
} // extern "C"
