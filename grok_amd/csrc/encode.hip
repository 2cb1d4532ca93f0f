// grok_amd/csrc/encode.hip -- encode: ingest, forward DWT, HT block coding (K1-K3), pipelined encodes and their results.
#include "context.h"

namespace {
// the context's encode layout for `ntiles` tiles of the current geometry, or GRK_AMD_ERR_INVALID and the reason
int encode_layout(grk_amd_ctx* c, uint32_t ntiles, PixelLayout& px)
{
    const char* why = "";
    if (!resolve_pixel_layout(c->geom.p, &c->enc_layout, 0, 0, ntiles, px, &why)) return fail(c, GRK_AMD_ERR_INVALID, why);
    return GRK_AMD_OK;
}

int run_ingest(grk_amd_ctx* c, uint32_t ntiles, const void* d_pixels, void* d_planes, const PixelLayout& px)
{
    const TileGeom& g = c->geom;
    const SampleRange r = sample_range(g.p);
    IngestArgs a{};
    set_px_in(a, px);
    a.pixels = d_pixels; a.planes = (int32_t*)d_planes;
    a.w = g.p.tile_w; a.h = g.p.tile_h; a.stride = g.stride; a.pitch = g.plane_elems;
    a.ncomp = g.p.num_comps; a.ntiles = ntiles;
    a.bytes_per_sample = r.bytes;
    a.dc = r.dc; a.sext = r.sext;
    a.mct = g.p.mct; a.irreversible = g.p.irreversible;
    ScopedTimer t(c, 0);
    HIP_TRY(c, launch_ingest(a, c->stream), "launch ingest");
    return GRK_AMD_OK;
}

// K3's arguments for `ntiles` tiles of the current geometry -- its buffers at their sizes, the arena and allocator plan, the classes
// with their lists --, built ONCE per call: every launch of the call, on whichever stream, takes a copy
int make_ht_args(grk_amd_ctx* c, uint32_t ntiles, const void* d_mallat, bool h16, HtArgs& a)
{
    a = HtArgs{};
    const TileGeom& g = c->geom;
    const uint32_t bpt = g.blocks_per_comp * g.p.num_comps;
    const uint64_t nblocks = (uint64_t)bpt * ntiles;
    const uint64_t raw = (uint64_t)ntiles * g.p.num_comps * g.p.tile_w * g.p.tile_h * ((g.p.prec + 7) / 8);
    const HtArenaPlan plan = plan_ht_arena(nblocks, raw, ntiles, c->ht_classes);
    HIP_TRY(c, c->lengths.ensure(nblocks * 4), "alloc lengths");
    HIP_TRY(c, c->offsets.ensure((nblocks + 1) * 8), "alloc offsets");
    HIP_TRY(c, c->flag.ensure(kHtAllocBytes), "alloc allocator state");
    HIP_TRY(c, c->arena.ensure(plan.arena_bytes), "alloc coded arena");
    c->last_arena_bound = plan.arena_bytes;
    HIP_TRY(c, c->ovf.ensure(plan.ovf_entries * 4 + 16), "alloc fallback list");
    a.mallat = (const int32_t*)d_mallat; a.stride = g.stride; a.pitch = g.plane_elems; a.h16 = h16 ? 1 : 0;
    a.blocks = (const HtBlockDesc*)c->blockdesc.p; a.blocks_per_tile = bpt; a.ncomp = g.p.num_comps; a.ntiles = ntiles;
    a.arena = (uint8_t*)c->arena.p; a.arena_bytes = c->arena.cap;
    a.alloc = (unsigned long long*)c->flag.p;        // [0] status flags, [1] bytes used (launch_ht_alloc_init resets them)
    a.lengths = (uint32_t*)c->lengths.p; a.offsets = (unsigned long long*)c->offsets.p;
    a.ovf_list = c->lds_cap ? (uint32_t*)c->ovf.p : nullptr;
    a.region_mask = plan.regions - 1;
    a.chunk_units = plan.chunk / 16u;
    a.irreversible = g.p.irreversible;
    a.num_classes = (uint32_t)c->ht_classes.size();
    for (uint32_t k = 0; k < a.num_classes; ++k) {
        const HtClassPlan& hc = c->ht_classes[k];
        a.classes[k] = HtClass{(const uint32_t*)c->ht_sel.p + hc.first, hc.count, hc.max_kmax, hc.max_samples, hc.max_quads, plan.ovf_base[k], hc.cap_kmax};
    }
    return GRK_AMD_OK;
}

// the classes the schedule (ht_class_stream, encode_plan.h) places at this point of the call, each on its stream
int launch_ht_at(grk_amd_ctx* c, const HtArgs& h, bool overlapped, HtPoint at, bool one_level)
{
    for (uint32_t k = 0; k < h.num_classes; ++k) {
        const HtStream to = ht_class_stream(c->ht_classes[k].role, overlapped, c->pipelining, at, one_level, c->k3_parity);
        if (to == HtStream::NotHere) continue;
        if (to == HtStream::Main) { HIP_TRY(c, launch_ht_classes(h, k, k + 1, c->stream), "launch ht encode"); continue; }
        hipStream_t st = to == HtStream::Side ? c->side : c->side2;
        HIP_TRY(c, hipStreamWaitEvent(st, c->ev_level0, 0), "side stream waits for the level");
        ScopedTimer tt(c, st == c->side ? 4 : 8, st);
        // (consecutive encodes pipelined: the top class is still running when the next encode's level 0 arrives; the frames take
        //  the two side streams in turn, c->k3_parity.  Whichever way round, every launch of the frame on a side stream is queued
        //  by the end of run_dwt's last level, which then records ev_side on `side` AND ev_side2 on `side2`: the pair of events of
        //  the frame's buffer set covers its last launch on each stream, and grk_amd_encode_tiles waits for both before level 0
        //  reuses the set)
        HtArgs hs = h;
        hs.room = c->pipelining ? 1 : 0;
        // pipelined frames in turn: a fallback launch sits between a class and the next frame's launch on its stream, and an empty one
        // of up to 1024 workgroups of worst-case LDS costs 10-14 us of stream time beside K3 -- one workgroup per CU walks the list
        const uint32_t fb = c->pipelining && c->k3_alternate && c->num_cus ? c->num_cus : kHtFallbackGrid;
        HIP_TRY(c, launch_ht_classes(hs, k, k + 1, st, fb), "launch ht encode (side stream)");
    }
    return GRK_AMD_OK;
}

// d_pixels != nullptr: level 0 reads the caller's pixels directly (K1 fused into K2), d_in is unused
// overlap_ht != nullptr: K3 of the classes whose sub-bands are final is queued on the side streams behind level 0 and the last level
int run_dwt(grk_amd_ctx* c, uint32_t nplanes, void* d_in, void* d_out, const void* d_pixels = nullptr, uint32_t ntiles = 0,
            const HtArgs* overlap_ht = nullptr, bool h16 = false, const PixelLayout* px = nullptr)
{
    const TileGeom& g = c->geom;
    const uint32_t L = g.p.num_levels;
    if (L == 0) {
        HIP_TRY(c, hipMemcpyAsync(d_out, d_in, (size_t)nplanes * g.plane_elems * 4, hipMemcpyDeviceToDevice, c->stream), "copy planes");
        return GRK_AMD_OK;
    }
    { const int rc = ensure_ll(c, nplanes); if (rc) return rc; }     // (LL ping-pong storage, context.h: ll_plane)
    ScopedTimer t(c, 1);
    const SampleRange r = sample_range(g.p);
    for (uint32_t l = 0; l < L; ++l) {
        DwtLevelArgs a{};
        a.cw = level_geom(g, l).w; a.ch = level_geom(g, l).h;
        a.px = level_geom(g, l).x0 & 1u; a.py = level_geom(g, l).y0 & 1u;
        const LLPlane from = ll_plane(c, l, d_in, d_out), to = ll_plane(c, l + 1, d_in, d_out);
        a.in = (const int32_t*)from.p; a.in_stride = from.stride; a.in_pitch = from.pitch;
        a.mallat = (int32_t*)d_out; a.m_stride = g.stride; a.m_pitch = g.plane_elems;
        a.ll = (int32_t*)to.p; a.ll_stride = to.stride; a.ll_pitch = to.pitch;
        a.nplanes = nplanes;
        a.irreversible = g.p.irreversible;
        a.h16 = h16 ? 1 : 0;
        a.pk = h16 && c->dwt_pk && pk16_level_ok(g.p, l);
        a.xcd = c->dwt_xcd;
        if (l == 0 && d_pixels && px && px->lay) {     // (before the level is shaped: the layout decides between the level-0 kernels)
            set_px_in(a, *px); a.px_chan = px->channels;
        }
        // the level's kernel instance, strips and row segments (plan_dwt_level, encode_plan.h).  Workgroups along z: planes, or for the
        // fused level 0 tiles (x components when there is no MCT triple)
        const bool fused = l == 0 && d_pixels;
        const uint32_t zslots = fused ? ntiles * level_part_zslots(g.p.mct != 0, g.p.num_comps) : nplanes;
        const DwtLevelShape shape = plan_dwt_level(DwtLevelDesc{a.cw, a.ch, a.px, a.py, a.in_stride, a.m_stride, a.h16 != 0, a.pk != 0,
                                                                a.irreversible != 0, a.px_lay, a.px_chan, a.px_row, zslots, fused, r.bytes});
        a.seg_pairs = shape.seg_pairs;
        // levels l and l + 1 in one launch where the planner has a pair for them (plan_dwt_pair, encode_plan.h; GRK_AMD_DWT_PAIR=0: never)
        uint32_t last = l;                             // the last level this turn's launch covers
        const DwtPairShape pair = plan_dwt_pair_at(g, l, DwtPairAsk{c->dwt_pair != 0, c->dwt_pk != 0, fused, h16, a.px_lay, a.px_chan, a.px_row,
                                                                    r.bytes, to.stride, ntiles});
        if (a.cw == 0 || a.ch == 0) {
            // a level without samples (a narrow tile off the origin: [ceil(x0 / 2^l), ceil((x0 + w) / 2^l)) can be empty):
            // nothing to transform, and nothing deeper either
        } else if (pair.ok) {
            const LLPlane to2 = ll_plane(c, l + 2, d_in, d_out);      // (the LL ping-pong goes on as if both levels had run)
            a.ll2 = (int32_t*)to2.p; a.ll2_stride = to2.stride; a.ll2_pitch = to2.pitch;
            a.pixels = d_pixels; a.px_bytes = r.bytes;
            a.alloc_reset = c->pend_alloc; a.alloc_chunk_units = c->pend_alloc_units; c->pend_alloc = nullptr;
            a.dc = r.dc; a.sext = r.sext;
            HIP_TRY(c, launch_dwt_pair(a, pair, ntiles, c->stream), "launch fused dwt levels 0 and 1");
            if (c->want_px_event) HIP_TRY(c, hipEventRecord(c->ev_px, c->stream), "record the pixels' last read");
            last = l + 1;
        } else if (fused) {
            a.pixels = d_pixels; a.px_bytes = r.bytes;
            a.alloc_reset = c->pend_alloc; a.alloc_chunk_units = c->pend_alloc_units; c->pend_alloc = nullptr;
            a.dc = r.dc; a.sext = r.sext;
            HIP_TRY(c, launch_dwt_level0_fused(a, shape, ntiles, g.p.num_comps, g.p.mct, c->stream), "launch fused dwt level 0");
            if (c->want_px_event) HIP_TRY(c, hipEventRecord(c->ev_px, c->stream), "record the pixels' last read");
        } else {
            HIP_TRY(c, launch_dwt_level(a, shape, c->stream), "launch dwt level");
        }
        if (overlap_ht && (l == 0 || last + 1 == L)) {
            // (a launch that covers level 0 AND the last level -- L == 1, or a pair with L == 2 -- answers for both points)
            HIP_TRY(c, hipEventRecord(c->ev_level0, c->stream), "record level");
            const int rc = launch_ht_at(c, *overlap_ht, true, l == 0 ? HtPoint::AfterLevel0 : HtPoint::AfterLastLevel, l == 0 && last + 1 == L);
            if (rc) return rc;
            if (last + 1 == L) {
                HIP_TRY(c, hipEventRecord(c->ev_side, c->side), "record side stream");
                HIP_TRY(c, hipEventRecord(c->ev_side2, c->side2), "record side stream 2");
            }
        }
        l = last;
    }
    return GRK_AMD_OK;
}

// overlapped: the top resolution and the large-LDS classes are already running on the side streams (run_dwt)
int run_ht(grk_amd_ctx* c, HtArgs a, bool overlapped = false, bool room = false)
{
    a.room = room ? 1 : 0;
    {
        ScopedTimer t(c, 2);
        if (!overlapped) HIP_TRY(c, launch_ht_alloc_init(a, c->stream), "reset arena allocator");
        const int rc = launch_ht_at(c, a, overlapped, HtPoint::RunHt, false);
        if (rc) return rc;
    }
    if (overlapped) {
        c->side_pending = true;
        if (!c->pipelining) { const int jr = join_side(c); if (jr) return jr; }    // pipelining: the next consumer joins
    }
    c->last_ntiles = a.ntiles;
    c->last_nblocks = (uint64_t)a.blocks_per_tile * a.ntiles;
    c->last_drops = nullptr;
    return GRK_AMD_OK;
}
} // namespace

// every block of the call on the main stream, class by class as a non-overlapped encode lays them out, through the drop instances
int ht_encode_drops(grk_amd_ctx* c, uint32_t ntiles, const void* d_mallat, bool h16, const uint8_t* d_drops)
{
    HtArgs a;
    const int rc = make_ht_args(c, ntiles, d_mallat, h16, a); if (rc) return rc;
    const HtDropPlan dp = plan_ht_drop_instance(a.irreversible != 0, a.h16 != 0);
    if (!dp.ok) return fail(c, GRK_AMD_ERR_INVALID, "no encode keeps irreversible int16 planes");
    // (the table's zero bit-planes are made from the drops when it is fetched, which may be long after the caller's buffer is gone)
    const uint64_t nblocks = (uint64_t)a.blocks_per_tile * a.ntiles;
    HIP_TRY(c, c->drops_keep.ensure(nblocks), "alloc drops copy");
    HIP_TRY(c, hipMemcpyAsync(c->drops_keep.p, d_drops, nblocks, hipMemcpyDeviceToDevice, c->stream), "keep the drops");
    {
        ScopedTimer t(c, 2);
        HIP_TRY(c, launch_ht_alloc_init(a, c->stream), "reset arena allocator");
        for (uint32_t k = 0; k < a.num_classes; ++k) {
            if (ht_class_stream(c->ht_classes[k].role, false, false, HtPoint::RunHt, false) != HtStream::Main) continue;
            HIP_TRY(c, launch_ht_classes_drops(a, k, k + 1, d_drops, dp.inst, c->stream), "launch ht encode (drops)");
        }
    }
    c->last_ntiles = a.ntiles;
    c->last_nblocks = (uint64_t)a.blocks_per_tile * a.ntiles;
    c->last_drops = (const uint8_t*)c->drops_keep.p;
    return GRK_AMD_OK;
}

extern "C" {
int grk_amd_stage_ingest_mct(grk_amd_ctx* c, const grk_amd_tile_params* p, uint32_t ntiles, const void* d_pixels, void* d_planes)
{
    int rc = stage_enter(c, p, d_pixels && d_planes, false); if (rc) return rc;
    if (!ntiles) return GRK_AMD_ERR_INVALID;
    PixelLayout px;
    rc = encode_layout(c, ntiles, px); if (rc) return rc;
    return run_ingest(c, ntiles, d_pixels, d_planes, px);
}

int grk_amd_stage_dwt_fwd(grk_amd_ctx* c, const grk_amd_tile_params* p, uint32_t nplanes, void* d_in, void* d_out)
{
    const int rc = stage_enter(c, p, d_in && d_out, true); if (rc) return rc;
    return run_dwt(c, nplanes, d_in, d_out);
}

int grk_amd_stage_ht_encode(grk_amd_ctx* c, const grk_amd_tile_params* p, uint32_t ntiles, const void* d_mallat)
{
    int rc = stage_enter(c, p, d_mallat != nullptr, true); if (rc) return rc;
    HtArgs h;
    rc = make_ht_args(c, ntiles, d_mallat, false, h); if (rc) return rc;
    return run_ht(c, h);
}

// the instances an encode of 8-bit reversible pixels launches (H16; flags bit 0: ROOM), on planes the caller chose
int grk_amd_stage_ht_encode16(grk_amd_ctx* c, const grk_amd_tile_params* p, uint32_t ntiles, const void* d_mallat16, uint32_t flags)
{
    int rc = stage_enter(c, p, d_mallat16 && !(flags & ~GRK_AMD_STAGE_HT_ROOM), true,
                               p && !planes16_ok(*p) ? "no encode keeps int16 planes for these parameters" : nullptr);
    if (rc) return rc;
    HtArgs h;
    rc = make_ht_args(c, ntiles, d_mallat16, true, h); if (rc) return rc;
    return run_ht(c, h, false, (flags & GRK_AMD_STAGE_HT_ROOM) != 0);
}

// the instances that take a per-block drop (kernels_ht.hip DROP), on planes and drops the caller chose
int grk_amd_stage_ht_encode_drops(grk_amd_ctx* c, const grk_amd_tile_params* p, uint32_t ntiles, const void* d_mallat, int planes16,
                                  const uint8_t* d_drops)
{
    const int rc = stage_enter(c, p, d_mallat && d_drops && ntiles, true,
                               planes16 && p && !planes16_ok(*p) ? "no encode keeps int16 planes for these parameters" : nullptr);
    if (rc) return rc;
    return ht_encode_drops(c, ntiles, d_mallat, planes16 != 0, d_drops);
}

int grk_amd_fetch_table(grk_amd_ctx* c, grk_amd_coded_block* table, uint64_t* total)
{
    if (!c || !c->last_nblocks) return GRK_AMD_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device), "set device");
    { const int jr = join_side(c); if (jr) return jr; }
    const uint64_t n = c->last_nblocks;
    uint64_t flagwords[2] = {0, 0};       // [0] low 32 bits: overflow flag, [1]: arena cursor
    std::vector<uint8_t> h_drops;         // the drop bytes of a launch that took them
    HIP_TRY(c, hipMemcpyAsync(flagwords, c->flag.p, 16, hipMemcpyDeviceToHost, c->stream), "fetch flag");
    if (table) {
        c->h_off.resize(n); c->h_len.resize(n);
        HIP_TRY(c, hipMemcpyAsync(c->h_off.data(), c->offsets.p, n * 8, hipMemcpyDeviceToHost, c->stream), "fetch offsets");
        HIP_TRY(c, hipMemcpyAsync(c->h_len.data(), c->lengths.p, n * 4, hipMemcpyDeviceToHost, c->stream), "fetch lengths");
        if (c->last_drops) {
            h_drops.resize(n);
            HIP_TRY(c, hipMemcpyAsync(h_drops.data(), c->last_drops, n, hipMemcpyDeviceToHost, c->stream), "fetch drops");
        }
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream), "sync");
    if (flagwords[0] & 1u) return fail(c, GRK_AMD_ERR_OVERFLOW, "coded arena overflow");
    if (flagwords[0] & 2u) return fail(c, GRK_AMD_ERR_UNSUPPORTED, "coefficient magnitude exceeds Kmax+1 bits");
    if (table) {
        const uint32_t bpt = (uint32_t)c->h_desc.size();
        for (uint64_t i = 0; i < n; ++i) {
            table[i].offset = c->h_off[i]; table[i].length = c->h_len[i];
            table[i].missing_msbs = c->h_desc[i % bpt].kmax - 1u;      // numbps = 1 is signalled (T1HT.cpp:123)
            if (!h_drops.empty()) table[i].missing_msbs = drop_missing_msbs(c->h_desc[i % bpt].kmax, h_drops[i]);   // ... d planes further down
        }
    }
    if (total) *total = flagwords[1];
    return GRK_AMD_OK;
}

int grk_amd_fetch_coded(grk_amd_ctx* c, uint8_t* dst, uint64_t nbytes)
{
    if (!c || !dst) return GRK_AMD_ERR_INVALID;
    if (nbytes > c->arena.cap) return GRK_AMD_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device), "set device");
    { const int jr = join_side(c); if (jr) return jr; }
    { const int rc = copy_d2h(c, dst, c->arena.p, nbytes); if (rc) return rc; }
    HIP_TRY(c, hipStreamSynchronize(c->stream), "sync");
    return GRK_AMD_OK;
}

int grk_amd_fetch_coded_async(grk_amd_ctx* c, uint8_t* dst, uint64_t nbytes)
{
    if (!c || !dst) return GRK_AMD_ERR_INVALID;
    if (nbytes > c->arena.cap) return GRK_AMD_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device), "set device");
    if (!host_is_pinned(dst)) return fail(c, GRK_AMD_ERR_INVALID, "grk_amd_fetch_coded_async needs pinned memory (grk_amd_host_alloc)");
    { const int jr = join_side(c); if (jr) return jr; }
    if (nbytes) HIP_TRY(c, hipMemcpyAsync(dst, c->arena.p, nbytes, hipMemcpyDeviceToHost, c->stream), "download");
    return GRK_AMD_OK;
}

int grk_amd_fetch_coefficients(grk_amd_ctx* c, uint32_t comp, int32_t* dst, uint32_t dst_stride)
{
    // (after a reduced decode the context holds the reduced geometry, not the encoded tile's)
    if (!c || !dst || !c->have_geom || c->geom.reduce || !c->last_nblocks || comp >= c->geom.p.num_comps || dst_stride < c->geom.p.tile_w)
        return GRK_AMD_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device), "set device");
    { const int jr = join_side(c); if (jr) return jr; }
    const TileGeom& g = c->geom;
    const uint32_t W = g.p.tile_w, H = g.p.tile_h;
    if (c->last_h16) {              // 16-bit planes between K2 and K3 (8-bit reversible content): widened here
        std::vector<int16_t> tmp((size_t)g.stride * H);
        HIP_TRY(c, hipMemcpyAsync(tmp.data(), (const int16_t*)c->p1.p + (size_t)comp * g.plane_elems, tmp.size() * 2,
                                  hipMemcpyDeviceToHost, c->stream), "fetch coefficients");
        HIP_TRY(c, hipStreamSynchronize(c->stream), "sync");
        for (uint32_t y = 0; y < H; ++y)
            for (uint32_t x = 0; x < W; ++x) dst[(size_t)y * dst_stride + x] = tmp[(size_t)y * g.stride + x];
    } else {
        HIP_TRY(c, hipMemcpy2DAsync(dst, (size_t)dst_stride * 4, (const int32_t*)c->p1.p + (size_t)comp * g.plane_elems,
                                    (size_t)g.stride * 4, (size_t)W * 4, H, hipMemcpyDeviceToHost, c->stream), "fetch coefficients");
        HIP_TRY(c, hipStreamSynchronize(c->stream), "sync");
    }
    return GRK_AMD_OK;
}

} // extern "C"

// Weights of T1::getwmsedec (t1/t1_part1/T1.cpp:394-414): L2 norms of the synthesis basis functions by orientation and decomposition
// level (dwt_norms / dwt_norms_real, T1.cpp:224-235; T1::getnorm clamps the level, :258-267) and of the inverse colour transform's
// columns (mct_norms_rev / _irrev, point_transform/mct.cpp:30-35)
static double band_norm(uint32_t orient, uint32_t level, bool reversible)
{
    static const double n53[4][10] = {{1.000, 1.500, 2.750, 5.375, 10.68, 21.34, 42.67, 85.33, 170.7, 341.3},
                                      {1.038, 1.592, 2.919, 5.703, 11.33, 22.64, 45.25, 90.48, 180.9, 0},
                                      {1.038, 1.592, 2.919, 5.703, 11.33, 22.64, 45.25, 90.48, 180.9, 0},
                                      {.7186, .9218, 1.586, 3.043, 6.019, 12.01, 24.00, 47.97, 95.93, 0}};
    static const double n97[4][10] = {{1.000, 1.965, 4.177, 8.403, 16.90, 33.84, 67.69, 135.3, 270.6, 540.9},
                                      {2.022, 3.989, 8.355, 17.04, 34.27, 68.63, 137.3, 274.6, 549.0, 0},
                                      {2.022, 3.989, 8.355, 17.04, 34.27, 68.63, 137.3, 274.6, 549.0, 0},
                                      {2.080, 3.865, 8.307, 17.18, 34.71, 69.59, 139.3, 278.6, 557.2, 0}};
    if (orient == 0 && level > 9) level = 9;
    else if (orient > 0 && level > 8) level = 8;
    return reversible ? n53[orient & 3u][level] : n97[orient & 3u][level];
}

double block_weight(const TileGeom& g, uint32_t row)
{
    static const double mct_rev[3] = {1.732, .8292, .8292}, mct_irrev[3] = {1.732, 1.805, 1.573};
    const grk_amd_block& b = g.blocks_comp0[row % g.blocks_per_comp];
    const uint32_t comp = row / g.blocks_per_comp;
    const double w1 = (g.p.mct && g.p.num_comps >= 3 && comp < 3) ? (g.p.irreversible ? mct_irrev[comp] : mct_rev[comp]) : 1.0;
    const double w2 = band_norm(b.band, g.p.num_levels - b.res, !g.p.irreversible);
    return w1 * w2 * (double)b.stepsize;
}

extern "C" {
int grk_amd_block_distortion(grk_amd_ctx* c, double* out, uint64_t cap)
{
    if (!c || !out || !c->have_geom || c->geom.reduce || !c->last_nblocks || cap < c->last_nblocks) return GRK_AMD_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device), "set device");
    { const int jr = join_side(c); if (jr) return jr; }
    const TileGeom& g = c->geom;
    const uint64_t n = c->last_nblocks;
    const uint32_t bpt = (uint32_t)c->h_desc.size();
    HIP_TRY(c, c->energy.ensure(n * 8), "alloc block energies");
    HIP_TRY(c, launch_block_energy(c->p1.p, c->last_h16 ? 1 : 0, g.p.irreversible, g.stride, g.plane_elems, (const HtBlockDesc*)c->blockdesc.p,
                                   bpt, g.p.num_comps, n, (unsigned long long*)c->energy.p, c->stream), "launch block energy");
    std::vector<unsigned long long> e(n);
    HIP_TRY(c, hipMemcpyAsync(e.data(), c->energy.p, n * 8, hipMemcpyDeviceToHost, c->stream), "fetch block energies");
    HIP_TRY(c, hipStreamSynchronize(c->stream), "sync");
    for (uint64_t i = 0; i < n; ++i) {
        const double w = block_weight(g, (uint32_t)(i % bpt));
        out[i] = w * w * (double)e[i];
    }
    return GRK_AMD_OK;
}

void* grk_amd_coded_device_ptr(grk_amd_ctx* c) { return c ? c->arena.p : nullptr; }
void* grk_amd_table_device_ptr(grk_amd_ctx* c, int which)
{
    if (!c) return nullptr;
    switch (which) {
    case 0: return c->offsets.p;                                    // uint64[nblocks]
    case 1: return c->lengths.p;                                    // uint32[nblocks]
    case 2: return c->flag.p ? (uint8_t*)c->flag.p + 8 : nullptr;   // uint64: bytes used in the arena
    case 3: return c->flag.p ? (uint8_t*)c->flag.p + 16 : nullptr;  // uint64[24]: blocks each K3 class handed to its fallback launch
    default: return nullptr;
    }
}

int grk_amd_encode_tiles(grk_amd_ctx* c, const grk_amd_tile_params* p, uint32_t ntiles, const void* pixels,
                         int on_device, grk_amd_coded_block* table, uint64_t* total)
{
    if (!c || !p || !pixels || ntiles == 0) return GRK_AMD_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device), "set device");
    int rc = ensure_geom(c, p); if (rc) return rc;
    const TileGeom& g = c->geom;
    PixelLayout px;                      // (the default layout: px.lay = 0, px.bytes = the tight tiles)
    rc = encode_layout(c, ntiles, px); if (rc) return rc;
    const void* d_px = pixels;
    if (!on_device) {
        HIP_TRY(c, c->pixels.ensure(px.bytes), "alloc pixel staging");
        rc = copy_h2d(c, c->pixels.p, pixels, px.bytes); if (rc) return rc;
        d_px = c->pixels.p;
    }
    const uint32_t nplanes = ntiles * g.p.num_comps;
    // the call's route (plan_route, encode_plan.h)
    const Route route = plan_route(g.p, RouteIn{c->overlap, c->pipelining, c->frame_streams, c->planes16, c->side != nullptr, c->side2 != nullptr,
                                                on_device != 0, (uint32_t)((uintptr_t)d_px & 3u), (uint64_t)nplanes * g.plane_elems});
    const bool fused = route.fused, ov = route.overlap, fs = route.frame_stream, h16 = route.h16;
    if (!fused) HIP_TRY(c, c->p0.ensure((size_t)nplanes * g.plane_elems * 4 + 256), "alloc planes");
    HIP_TRY(c, c->p1.ensure((size_t)nplanes * g.plane_elems * 4 + 256), "alloc Mallat planes");
    {
        ScopedTimer t(c, 3);
        if (ov && c->pipelining && c->seq_index < 0 && probe_streams(c) != GRK_AMD_OK) {
            // (the probe is a convenience: when it cannot run, the streams stay as they are and it is not tried again)
            c->stream_probe = 0; (void)hipGetLastError();
        }
        hipStream_t fs_st = nullptr;
        if (ov && c->pipelining) {
            // take the other buffer set: the blocks of the previous encode may still be being coded from the set used
            // last; the set taken now was last used two encodes ago, and its side-stream work is waited for here
            // (hipStreamWaitEvent on an event never recorded is a no-op)
            auto swap_with = [&](grk_amd_ctx::AltSet& as) {
                std::swap(c->p1, as.p1); std::swap(c->arena, as.arena); std::swap(c->lengths, as.lengths);
                std::swap(c->offsets, as.offsets); std::swap(c->flag, as.flag); std::swap(c->ovf, as.ovf);
                std::swap(c->ev_side, as.ev_side); std::swap(c->ev_side2, as.ev_side2);
            };
            // the oldest of the pipe_depth - 1 other sets becomes current; the set retired here takes its slot as the newest
            swap_with(c->alts[c->alt_head]);
            // (the LL ping-pong buffers belong to the set as well: frames on different streams transform at the same time, and a call
            //  of the other form -- the same geometry, more tiles -- must not take a running frame's)
            std::swap(c->llA, c->alts[c->alt_head].llA); std::swap(c->llB, c->alts[c->alt_head].llB);
            c->alt_head = (c->alt_head + 1) % (c->pipe_depth - 1);
            c->side_pending = false;
            if (fs) {
                fs_st = c->fs_parity ? c->side2 : c->side; c->fs_parity ^= 1;
                HIP_TRY(c, ensure_event(&c->ev_main), "create event");
                rc = order_behind(c, fs_st, c->ev_main, c->stream, "record the caller's stream", "the frame's stream waits for the pixels"); if (rc) return rc;
            }
            HIP_TRY(c, hipStreamWaitEvent(fs ? fs_st : c->stream, c->ev_side, 0), "wait for the buffer set");
            HIP_TRY(c, hipStreamWaitEvent(fs ? fs_st : c->stream, c->ev_side2, 0), "wait for the buffer set");
            HIP_TRY(c, c->p1.ensure((size_t)nplanes * g.plane_elems * 4 + 256), "alloc Mallat planes");
        } else {
            rc = join_side(c); if (rc) return rc;
        }
        c->last_h16 = h16;
        // K3's arguments, once for the call (after the buffer set was taken: they point into it)
        HtArgs h;
        rc = make_ht_args(c, ntiles, c->p1.p, h16, h); if (rc) return rc;
        if (fs) {
            t.cancel();
            // the whole frame on its stream, as the non-overlapped path lays it out (one K3 launch of every block, the ROOM instance)
            struct StreamSwap { grk_amd_ctx* c; hipStream_t keep; StreamSwap(grk_amd_ctx* c_, hipStream_t s) : c(c_), keep(c_->stream) { c->stream = s; }
                                ~StreamSwap() { c->stream = keep; } } on_frame_stream(c, fs_st);
            HIP_TRY(c, ensure_event(&c->ev_px), "create event");
            ScopedTimer tf(c, 3);              // (the call's timer on the stream that carries the call)
            c->want_px_event = true;
            rc = run_dwt(c, nplanes, nullptr, c->p1.p, d_px, ntiles, nullptr, h16, &px);
            c->want_px_event = false;
            if (rc) return rc;
            // the pixel-lifetime contract of every other path: work queued on the context's stream after this call comes after the read
            c->px_event_valid = true;
            if (!c->px_hold)
                HIP_TRY(c, hipStreamWaitEvent(on_frame_stream.keep, c->ev_px, 0), "the context's stream waits for the pixels' last read");
            rc = run_ht(c, h, false, true); if (rc) return rc;
            HIP_TRY(c, hipEventRecord(c->ev_side, fs_st), "record the frame's stream");
            HIP_TRY(c, hipEventRecord(c->ev_side2, fs_st), "record the frame's stream");
            c->side_pending = true;
            if (table || total) return grk_amd_fetch_table(c, table, total);
            return GRK_AMD_OK;
        }
        c->px_event_valid = false;          // (the pixels are read on the context's stream itself from here on)
        if (ov) {       // the allocator must be reset before the first K3 launch of either stream
            // (with the fused level 0 its first workgroup does it: one launch less on the main stream's chain)
            if (fused) { c->pend_alloc = h.alloc; c->pend_alloc_units = h.chunk_units; }
            else HIP_TRY(c, launch_ht_alloc_init(h, c->stream), "reset arena allocator");
        }
        if (fused) {
            rc = run_dwt(c, nplanes, nullptr, c->p1.p, d_px, ntiles, ov ? &h : nullptr, h16, &px); if (rc) return rc;
        } else {
            rc = run_ingest(c, ntiles, d_px, c->p0.p, px); if (rc) return rc;
            rc = run_dwt(c, nplanes, c->p0.p, c->p1.p, nullptr, ntiles, ov ? &h : nullptr); if (rc) return rc;
        }
        rc = run_ht(c, h, ov); if (rc) return rc;
        if (ov && c->pipelining && c->k3_alternate) c->k3_parity ^= 1u;      // the next pipelined frame: the side streams the other way round
    }
    if (table || total) return grk_amd_fetch_table(c, table, total);
    return GRK_AMD_OK;
}

int grk_amd_stream_wait_results(grk_amd_ctx* c, void* hip_stream)
{
    if (!c || !hip_stream) return GRK_AMD_ERR_INVALID;
    hipStream_t s = (hipStream_t)hip_stream;
    HIP_TRY(c, ensure_event(&c->ev_main), "create event");
    { const int rc = order_behind(c, s, c->ev_main, c->stream, "record main stream", "wait for the main stream"); if (rc) return rc; }
    if (c->side_pending) {
        HIP_TRY(c, hipStreamWaitEvent(s, c->ev_side, 0), "wait for the side stream");
        HIP_TRY(c, hipStreamWaitEvent(s, c->ev_side2, 0), "wait for the side stream 2");
    }
    return GRK_AMD_OK;
}

int grk_amd_set_pixel_hold(grk_amd_ctx* c, int on)
{
    if (!c) return GRK_AMD_ERR_INVALID;
    c->px_hold = on != 0;
    return GRK_AMD_OK;
}

int grk_amd_stream_wait_pixels(grk_amd_ctx* c, void* hip_stream)
{
    if (!c || !hip_stream) return GRK_AMD_ERR_INVALID;
    hipStream_t s = (hipStream_t)hip_stream;
    if (c->px_event_valid) { HIP_TRY(c, hipStreamWaitEvent(s, c->ev_px, 0), "wait for the pixels' last read"); return GRK_AMD_OK; }
    if (s == c->stream) return GRK_AMD_OK;        // (stream order)
    HIP_TRY(c, ensure_event(&c->ev_main), "create event");
    return order_behind(c, s, c->ev_main, c->stream, "record main stream", "wait for the main stream");
}

int grk_amd_get_pipelining(grk_amd_ctx* c)
{
    return c && c->pipelining && c->overlap && c->side ? c->pipe_depth - 1 : 0;
}

int grk_amd_set_pipelining(grk_amd_ctx* c, int on)
{
    if (!c) return GRK_AMD_ERR_INVALID;
    const int rc = grk_amd_synchronize(c);
    c->pipelining = on != 0 && c->side != nullptr && c->side2 != nullptr;
    c->pipe_depth = std::min(std::max(on, 1) + 1, grk_amd_ctx::kMaxAltSets + 1);
    c->alt_head = 0;
    c->k3_parity = 0;
    return rc;
}
} // extern "C"
