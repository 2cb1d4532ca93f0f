// grok_amd/csrc/decode_blocks.hip -- decode: a call's tables on their way to the device, the block decoders' launches (HT K5,
// Part-1 K8 / K8L) and the status word they leave.  What is launched on what is planned in decode_plan.cpp.
#include "decode_internal.h"

int stage_table(grk_amd_ctx* c, const grk_amd_coded_block* table, uint64_t nblocks, grk_amd_ctx::DecUpload** out)
{
    grk_amd_ctx::DecUpload* u = &c->dec_up[c->dec_turn++ & 1u];
    HIP_TRY(c, ensure_event(&u->ev), "create event");
    HIP_TRY(c, hipEventSynchronize(u->ev), "wait for the tables' last upload");
    const size_t need = (size_t)nblocks * (sizeof(grk_amd_coded_block) + 16) + 64;        // rows + the launch lists behind them
    if (u->cap < need) {
        if (u->p) (void)hipHostFree(u->p);
        u->p = u->dp = nullptr; u->cap = 0;
        HIP_TRY(c, hipHostMalloc((void**)&u->p, need, hipHostMallocDefault), "alloc pinned tables");
        HIP_TRY(c, hipHostGetDevicePointer((void**)&u->dp, u->p, 0), "map pinned tables");
        u->cap = need;
    }
    const TileGeom& g = c->geom;
    if (g.reduce) {             // the caller's rows are the full tile's: each component keeps its first blocks_per_comp rows
        const uint64_t groups = nblocks / g.blocks_per_comp;
        for (uint64_t k = 0; k < groups; ++k)
            std::memcpy(u->p + k * g.blocks_per_comp * sizeof(grk_amd_coded_block), table + k * g.full_blocks_per_comp,
                        (size_t)g.blocks_per_comp * sizeof(grk_amd_coded_block));
    } else {
        std::memcpy(u->p, table, (size_t)nblocks * sizeof(grk_amd_coded_block));
    }
    *out = u;
    return GRK_AMD_OK;
}

namespace {
// rows (+ the lists behind them) -> dec_table on the call's stream, the status block cleared
int upload_table(grk_amd_ctx* c, grk_amd_ctx::DecUpload* u, size_t bytes)
{
    HIP_TRY(c, c->dec_table.ensure(bytes + 64), "alloc decode table");
    HIP_TRY(c, c->flag.ensure(kHtAllocBytes), "alloc status");
    HIP_TRY(c, launch_dec_upload(u->dp, c->dec_table.p, bytes, c->flag.p, c->stream), "upload decode tables");
    HIP_TRY(c, hipEventRecord(u->ev, c->stream), "record the tables' upload");
    return GRK_AMD_OK;
}

// the segment list that applies to this call's rows (decode_impl made the reduced one)
int call_segments(grk_amd_ctx* c, uint64_t nblocks, SegList* sl)
{
    const char* why = "";
    const int rc = select_segments(c->geom.reduce != 0, c->dec_seg_first, c->dec_segs, c->red_seg_first, c->red_segs, nblocks, sl, &why);
    return rc ? fail(c, rc, why) : GRK_AMD_OK;
}
static_assert(sizeof(HtDecBlock) == sizeof(grk_amd_coded_block), "decode table rows are grk_amd_coded_block");
static_assert(sizeof(grk_amd_segment) == sizeof(uint2), "segments are {bytes, passes}");
} // namespace

int run_ht_decode(grk_amd_ctx* c, uint32_t ntiles, grk_amd_ctx::DecUpload* up, const void* d_coded, uint64_t coded_bytes, void* d_mallat,
                  bool h16, bool split)
{
    const TileGeom& g = c->geom;
    const uint32_t bpt = g.blocks_per_comp * g.p.num_comps;
    const uint64_t nblocks = (uint64_t)bpt * ntiles;
    const grk_amd_coded_block* const table = (const grk_amd_coded_block*)up->p;
    const char* why = "";
    // behind the rows: the blocks that have data at all
    uint32_t* const h_active = (uint32_t*)(up->p + nblocks * sizeof(grk_amd_coded_block));
    uint32_t nactive = 0, max_len = 0;
    { const int rc = plan_ht_blocks(table, nblocks, coded_bytes, h_active, &nactive, &max_len, &why); if (rc) return fail(c, rc, why); }
    HIP_TRY(c, c->dec_quads.ensure(nblocks * 1024 * 2 + 64), "alloc quad info");
    HIP_TRY(c, c->dec_mslen.ensure(nblocks * 4), "alloc ms lengths");
    { const int rc = upload_table(c, up, nblocks * sizeof(HtDecBlock) + (size_t)nactive * 4); if (rc) return rc; }
    const uint32_t* const d_active = (const uint32_t*)((const char*)c->dec_table.p + nblocks * sizeof(HtDecBlock));
    HtDecArgs a{};
    a.table = (const HtDecBlock*)c->dec_table.p;
    a.blocks = (const HtBlockDesc*)c->dec_desc.p; a.blocks_per_tile = bpt; a.nblocks = (uint32_t)nblocks; a.ncomp = g.p.num_comps;
    a.coded = (const uint8_t*)d_coded; a.coded_bytes = coded_bytes;
    a.quads = (uint32_t*)c->dec_quads.p; a.ms_len = (uint32_t*)c->dec_mslen.p; a.status = (unsigned int*)c->flag.p;
    a.active = nactive == nblocks ? nullptr : d_active; a.nactive = nactive;
    a.mallat = (int32_t*)d_mallat; a.stride = g.stride; a.pitch = g.plane_elems;
    a.irreversible = g.p.irreversible;
    a.h16 = h16 ? 1 : 0;
    a.h16_bias = (h16 && c->dwt_pk) ? 2048 : 32768;        // (pk16.h kPkDecodeBound + 1: the inverse transform runs on packed pairs)
    SegList sl;
    { const int rc = call_segments(c, nblocks, &sl); if (rc) return rc; }
    if (sl.nfirst) {
        std::vector<grk_amd_segment> ref(nblocks);
        { const int rc = plan_ht_refinement(table, nblocks, sl, ref.data(), &a.max_refine_bytes, &why); if (rc) return fail(c, rc, why); }
        HIP_TRY(c, c->dec_seg_dev.ensure(nblocks * sizeof(uint2) + 16), "alloc refinement table");
        HIP_TRY(c, hipMemcpyAsync(c->dec_seg_dev.p, ref.data(), nblocks * sizeof(uint2), hipMemcpyHostToDevice, c->stream), "upload refinement table");
        HIP_TRY(c, hipStreamSynchronize(c->stream), "sync refinement table");       // (uploaded from a local)
        a.refine = (const uint2*)c->dec_seg_dev.p;
    }
    // K5b in two parts when the call goes on with the inverse transform (decode_impl): the levels below the last one need the
    // blocks of the lower resolutions only -- a quarter of them --, and those short, latency-bound launches hide beside the
    // top resolution's K5b on the low-priority side stream
    const uint32_t L = g.p.num_levels;
    const uint32_t first_top = L >= 1 ? g.res[L].band[0].first_block : 0;
    if (split && c->overlap && c->side && L >= 2 && !a.refine && first_top > 0 && first_top < g.blocks_per_comp) {
        HIP_TRY(c, ensure_event(&c->ev_dec_front), "create event");
        HIP_TRY(c, ensure_event(&c->ev_dec_top), "create event");
        HIP_TRY(c, launch_ht_decode_front(a, c->stream), "launch ht decode");
        HIP_TRY(c, hipEventRecord(c->ev_dec_front, c->stream), "record K5a");
        HIP_TRY(c, hipStreamWaitEvent(c->side, c->ev_dec_front, 0), "side stream waits for K5a");
        a.ms_bpc = g.blocks_per_comp;
        a.ms_first = first_top; a.ms_count = g.blocks_per_comp - first_top;
        HIP_TRY(c, launch_ht_decode_ms(a, max_len, c->side), "launch K5b, top resolution");
        HIP_TRY(c, hipEventRecord(c->ev_dec_top, c->side), "record K5b");
        c->dec_top_pending = true;
        a.ms_first = 0; a.ms_count = first_top;
        HIP_TRY(c, launch_ht_decode_ms(a, max_len, c->stream), "launch K5b, lower resolutions");
        return GRK_AMD_OK;
    }
    ScopedTimer t(c, 5);
    HIP_TRY(c, launch_ht_decode(a, max_len, c->stream), "launch ht decode");
    return GRK_AMD_OK;
}

int run_t1_decode(grk_amd_ctx* c, uint32_t ntiles, grk_amd_ctx::DecUpload* up, const void* d_coded, uint64_t coded_bytes, void* d_mallat)
{
    const TileGeom& g = c->geom;
    const uint32_t bpt = g.blocks_per_comp * g.p.num_comps;
    const uint64_t nblocks = (uint64_t)bpt * ntiles;
    const grk_amd_coded_block* const table = (const grk_amd_coded_block*)up->p;
    const char* why = "";
    { const int rc = check_table(table, nblocks, coded_bytes, &why); if (rc) return fail(c, rc, why); }
    static_assert(kT1WorkBytes == 4096 * 4, "K8 and K8L share a block's part of the workspace");
    HIP_TRY(c, c->dec_work.ensure(nblocks * kT1WorkBytes), "alloc Part-1 workspace");
    // K8L's and K8's lists behind the rows in the pinned tables (stage_table leaves 16 bytes per block)
    uint32_t* const h_lane = (uint32_t*)(up->p + nblocks * sizeof(grk_amd_coded_block));      // (room for 2 nblocks entries: padding)
    uint32_t* const h_tail = h_lane + 2 * nblocks;
    T1PlanIn in{};
    in.table = table; in.nblocks = nblocks;
    std::vector<uint16_t> block_h(bpt);
    for (uint32_t i = 0; i < bpt; ++i) block_h[i] = c->h_desc_dec[i].h;
    in.block_h = block_h.data(); in.blocks_per_tile = bpt;
    in.cblksty = g.p.reserved[1]; in.t1_lanes = c->t1_lanes; in.pass_sync = c->t1_pass_sync; in.have_segments = !c->dec_seg_first.empty();
    T1Lists lists;
    { const int rc = plan_t1_lists(in, h_lane, h_tail, &lists, &why); if (rc) return fail(c, rc, why); }
    const uint32_t n_lane = lists.n_lane, n_tail = lists.n_tail;
    { const int rc = upload_table(c, up, nblocks * sizeof(HtDecBlock) + nblocks * 12); if (rc) return rc; }
    const uint32_t* const d_lane = (const uint32_t*)((const char*)c->dec_table.p + nblocks * sizeof(HtDecBlock));
    T1DecArgs a{};
    a.table = (const HtDecBlock*)c->dec_table.p;
    a.blocks = (const HtBlockDesc*)c->dec_desc.p; a.blocks_per_tile = bpt; a.nblocks = (uint32_t)nblocks; a.ncomp = g.p.num_comps;
    a.coded = (const uint8_t*)d_coded; a.coded_bytes = coded_bytes;
    a.work = (int32_t*)c->dec_work.p; a.status = (unsigned int*)c->flag.p;
    a.mallat = (int32_t*)d_mallat; a.stride = g.stride; a.pitch = g.plane_elems;
    a.irreversible = g.p.irreversible;
    a.cblksty = g.p.reserved[1];
    SegList sl;
    { const int rc = call_segments(c, nblocks, &sl); if (rc) return rc; }
    if (sl.nfirst) {
        const size_t nf = sl.nfirst * 4, ns = sl.nsegs * sizeof(grk_amd_segment);
        const size_t ns_off = (nf + 15) & ~(size_t)15;
        HIP_TRY(c, c->dec_seg_dev.ensure(ns_off + ns + 16), "alloc segment list");
        HIP_TRY(c, hipMemcpyAsync(c->dec_seg_dev.p, sl.first, nf, hipMemcpyHostToDevice, c->stream), "upload segment index");
        if (ns) HIP_TRY(c, hipMemcpyAsync((char*)c->dec_seg_dev.p + ns_off, sl.segs, ns, hipMemcpyHostToDevice, c->stream), "upload segments");
        a.seg_first = (const uint32_t*)c->dec_seg_dev.p;
        a.segs = (const uint2*)((const char*)c->dec_seg_dev.p + ns_off);
    }
    ScopedTimer t(c, 5);
    if (n_lane) {
        T1LaneArgs la{};
        la.table = a.table; la.blocks = a.blocks; la.blocks_per_tile = bpt; la.ncomp = a.ncomp;
        la.list = d_lane; la.count = n_lane;
        la.coded = a.coded; la.coded_bytes = coded_bytes;
        la.work = (uint64_t*)c->dec_work.p;
        la.mallat = a.mallat; la.stride = a.stride; la.pitch = a.pitch; la.irreversible = a.irreversible;
        la.pass_sync = c->t1_pass_sync ? 1 : 0;
        a.list = d_lane + 2 * nblocks; a.count = n_tail;
        // one launch, one stream (r06): the long chains are the launch's first workgroups, the lane waves follow; a decode SEQUENCE then
        // needs one hardware queue per frame in flight instead of two
        if (n_tail) {
            HIP_TRY(c, launch_t1_fused(a, la, c->stream), "launch Part-1 decode (both decoders)");
            return GRK_AMD_OK;
        }
        if (c->overlap && c->side) {
            // the long chains on the call's stream, the lanes beside them on the side stream
            HIP_TRY(c, ensure_event(&c->ev_dec_front), "create event");
            HIP_TRY(c, ensure_event(&c->ev_dec_top), "create event");
            HIP_TRY(c, hipEventRecord(c->ev_dec_front, c->stream), "record the tables");
            HIP_TRY(c, hipStreamWaitEvent(c->side, c->ev_dec_front, 0), "side stream waits for the tables");
            HIP_TRY(c, launch_t1_decode(a, c->stream), "launch Part-1 decode (long blocks)");
            HIP_TRY(c, launch_t1_lanes(la, c->side), "launch Part-1 decode (lanes)");
            HIP_TRY(c, hipEventRecord(c->ev_dec_top, c->side), "record the lanes");
            HIP_TRY(c, hipStreamWaitEvent(c->stream, c->ev_dec_top, 0), "join the lanes");
        } else {
            HIP_TRY(c, launch_t1_decode(a, c->stream), "launch Part-1 decode (long blocks)");
            HIP_TRY(c, launch_t1_lanes(la, c->stream), "launch Part-1 decode (lanes)");
        }
        return GRK_AMD_OK;
    }
    HIP_TRY(c, launch_t1_decode(a, c->stream), "launch Part-1 decode");
    return GRK_AMD_OK;
}

int check_decode_status(grk_amd_ctx* c)
{
    uint32_t st = 0;
    if (!c->flag.p) return GRK_AMD_OK;                 // nothing was decoded on this context (a sequence's frames are on its children)
    HIP_TRY(c, hipMemcpyAsync(&st, c->flag.p, 4, hipMemcpyDeviceToHost, c->stream), "fetch status");
    HIP_TRY(c, hipStreamSynchronize(c->stream), "sync");
    if (st & 4u) return fail(c, GRK_AMD_ERR_INVALID, "corrupt HT code-block (bad Scup or U_q > missing_msbs)");
    if (st & 16u) return fail(c, GRK_AMD_ERR_INVALID, "Part-1 code-block with more than 24 bit-planes (k_max_bit_planes)");
    if (st & 8u) return fail(c, GRK_AMD_ERR_RANGE, "a coefficient left the 16-bit planes: decode again after grk_amd_set_decode_planes16(ctx, 0)");
    return GRK_AMD_OK;
}
