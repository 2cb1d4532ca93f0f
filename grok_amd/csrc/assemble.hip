// grok_amd/csrc/assemble.hip -- Tier-2 on the device.
#include "context.h"
#include "image.h"
#include "t2_order.h"
#include "t2_parts.h"

// The finished tile-parts of coded blocks that lie on the device, made where they are (kernels_t2.hip): KT1 writes every packet's
// header, KT1b frames the tile-parts (SOT, PLT, SOD) and says where every packet goes, KT2 gathers headers, code-block bytes and frames
// into the output.  Nothing has to come to the host in between.  grk_amd_assemble_device serves the LATEST grk_amd_encode_tiles call
// from the context's own table and arena; encode_joint_device (image.h) an image whose units several calls coded, from image-wide
// tables that KK (kernels_t2keep.hip) filled behind each of them.
namespace {
// What one call of the writer frames: `ntiles` tiles of ONE plan (on the host and on the device), whose rows lie tile after tile, bpt
// per tile, in `lengths` / `offsets` (into `arena`; the rows' lengths sum to at most arena_bytes); the status word the kernels
// raise their bits in
struct T2Source {
    const T2Plan* plan; uint32_t max_blocks; const void* d_packets; const void* d_pob;
    uint32_t bpt;
    const uint32_t* lengths; const uint64_t* offsets; const uint8_t* arena; uint64_t arena_bytes;
    unsigned int* status;
    const uint8_t* msbs = nullptr;    // [tile][row]: the rows' missing_msbs for the general zero-bit-plane tree (`plan` made for it); NULL: the constant one
};

// the kernels queued on `st`, which must already be ordered behind the source's tables and bytes; `o` takes the tile-parts from
// dst_offset on (what lies below is kept when the buffer has to grow; 16 bytes stay free behind them).  The scratch is the
// context's: one stream at a time.
// Tiles divided into tile-parts (GRK_AMD_CS_TP) take a path of their own: `starts` / `nparts` are the caller's division
// (grk_amd_stage_assemble_parts), or with starts == NULL the plan's (T2Plan::part_starts, made from the flags); an undivided call
// -- one part, none named -- runs KT1, KT1b and KT2 as before.  Divided: KT1, KT1p, KT1q, KT1r, KT2p (kernels_t2parts.hip).
int assemble_enqueue(grk_amd_ctx* c, const T2Source& src, uint32_t ntiles, const uint32_t* tile_index, uint32_t flags, uint64_t dst_offset,
                     hipStream_t st, grk_amd_ctx::T2Out& o, const uint32_t* starts = nullptr, uint32_t nparts = 0)
{
    const T2Plan& plan = *src.plan;
    const size_t npk = plan.packets.size();
    const uint32_t bpt = src.bpt;
    const uint64_t nblocks = (uint64_t)bpt * ntiles;
    const size_t nq = npk * ntiles;
    if (!starts && plan.part_starts.size() > 1) { starts = plan.part_starts.data(); nparts = (uint32_t)plan.part_starts.size(); }
    const bool divided = starts != nullptr;
    const bool plt = (flags & GRK_AMD_CS_PLT) != 0;
    // the parts' frames in a tile's frame scratch, each with room for what its packets can need (t2_parts.h), on 16-byte boundaries
    std::vector<T2Part>& parts = c->t2_parts_host;
    if (divided) {
        if (!nparts || nparts > kMaxTileParts || starts[0] != 0) return GRK_AMD_ERR_INVALID;
        parts.assign(nparts, T2Part{});
        uint64_t at = 0;
        for (uint32_t k = 0; k < nparts; ++k) {
            const uint64_t first = starts[k], last = k + 1 < nparts ? starts[k + 1] : npk;
            if (first > last || last > npk) return GRK_AMD_ERR_INVALID;
            parts[k] = T2Part{(uint32_t)first, (uint32_t)(last - first), (uint32_t)at};
            at += (part_frame_bound(last - first, plt) + 15) & ~15ull;
        }
        if (at >> 32) return GRK_AMD_ERR_UNSUPPORTED;
    }
    o.nparts = divided ? nparts : 1u;
    // a frame: SOT 12, SOD 2, PLT: at most 6 bytes per packet and 5 per marker segment of 65 532
    const uint32_t lit_stride = divided ? parts.back().frame_at + (uint32_t)((part_frame_bound(parts.back().count, plt) + 15) & ~15ull)
                                        : (uint32_t)((14 + 6 * npk + 5 * (6 * npk / 65000 + 2) + 15) & ~(size_t)15);
    const size_t nframes = (size_t)ntiles * (divided ? nparts : 1u);
    // what the call can write at most: every byte of the arena, every header, every frame
    const uint64_t bound = src.arena_bytes + (uint64_t)ntiles * (plan.h_bytes + lit_stride + 8ull * npk) + 16;
    auto need = [&](DevBuf& b, size_t n, const char* what) -> int {
        if (n <= b.cap) return GRK_AMD_OK;
        // (a scratch buffer about to be replaced may be in use by kernels queued earlier on the stream)
        HIP_TRY(c, hipStreamSynchronize(st), "sync");
        HIP_TRY(c, b.ensure(n), what);
        return GRK_AMD_OK;
    };
    int rc;
    if ((rc = need(c->t2_u, (size_t)plan.u_words * 4 * ntiles + 16, "alloc header bits"))) return rc;
    if ((rc = need(c->t2_h, (size_t)plan.h_bytes * ntiles + 16, "alloc headers"))) return rc;
    if (src.msbs && (rc = need(c->t2_nodes, (size_t)plan.v_bytes * ntiles + 16, "alloc tag-tree nodes"))) return rc;
    if ((rc = need(c->t2_rel, nblocks * 4, "alloc block places"))) return rc;
    if ((rc = need(c->t2_pkhdr, nq * 4, "alloc packet lengths"))) return rc;
    if ((rc = need(c->t2_pkbody, nq * 8, "alloc packet lengths"))) return rc;
    if ((rc = need(c->t2_pkdst, nq * 8, "alloc packet places"))) return rc;
    if ((rc = need(c->t2_lit, (size_t)lit_stride * ntiles, "alloc frames"))) return rc;
    if ((rc = need(c->t2_litlen, nframes * 4, "alloc frames"))) return rc;
    if (divided) {
        if ((rc = need(c->t2_parts, (size_t)nparts * sizeof(T2Part), "alloc the tile-parts' table"))) return rc;
        if ((rc = need(o.tp_len, nframes * 4, "alloc the parts' lengths"))) return rc;
        if ((rc = need(o.tp_dst, nframes * 8, "alloc the parts' places"))) return rc;
    }
    if ((rc = need(c->t2_index, (size_t)ntiles * 4, "alloc tile numbers"))) return rc;
    if ((rc = need(o.tile_dst, (size_t)ntiles * 8, "alloc tile-part places"))) return rc;
    if ((rc = need(o.part_len, (size_t)ntiles * 4, "alloc tile-part lengths"))) return rc;
    if ((rc = need(o.total, 16, "alloc tile-part total"))) return rc;
    if (o.out.cap < dst_offset + bound) {
        DevBuf bigger;
        HIP_TRY(c, hipStreamSynchronize(st), "sync");
        HIP_TRY(c, bigger.ensure(dst_offset + bound), "alloc tile-parts");
        // (a file assembled in place starts behind room for its header: there may be nothing below dst_offset yet)
        const size_t keep = (size_t)std::min<uint64_t>(dst_offset, o.out.cap);
        if (keep) HIP_TRY(c, hipMemcpyAsync(bigger.p, o.out.p, keep, hipMemcpyDeviceToDevice, st), "keep tile-parts");
        HIP_TRY(c, hipStreamSynchronize(st), "sync");
        o.out.release();
        o.out = bigger;
    }
    HIP_TRY(c, hipMemsetAsync(c->t2_u.p, 0, (size_t)plan.u_words * 4 * ntiles, st), "clear header bits");
    // (the tile numbers: pageable memory of the caller's -- the runtime has staged them when the call returns)
    HIP_TRY(c, hipMemcpyAsync(c->t2_index.p, tile_index, (size_t)ntiles * 4, hipMemcpyHostToDevice, st), "upload");
    T2HeaderArgs ha{};
    ha.packets = (const T2Packet*)src.d_packets; ha.npackets = (uint32_t)npk;
    ha.lengths = src.lengths; ha.bpt = bpt; ha.ntiles = ntiles;
    ha.ubits = (uint32_t*)c->t2_u.p; ha.u_words = plan.u_words;
    ha.hdr = (uint8_t*)c->t2_h.p; ha.h_bytes = plan.h_bytes;
    ha.rel = (uint32_t*)c->t2_rel.p; ha.pk_hdr = (uint32_t*)c->t2_pkhdr.p; ha.pk_body = (uint64_t*)c->t2_pkbody.p;
    ha.status = src.status;
    ha.msbs = src.msbs; ha.nodes = src.msbs ? (uint8_t*)c->t2_nodes.p : nullptr; ha.v_bytes = plan.v_bytes;
    HIP_TRY(c, launch_t2_header(ha, src.max_blocks, st), "launch Tier-2 headers");
    const uint32_t sop = (flags & GRK_AMD_CS_SOP) ? 6u : 0u, eph = (flags & GRK_AMD_CS_EPH) ? 2u : 0u;
    if (divided) {
        // (pageable memory of the context's, like the tile numbers above: the runtime has staged the table when hipMemcpyAsync returns,
        //  so the next call -- of grk_amd_assemble_device_async too, which waits for nothing -- may write c->t2_parts_host anew)
        HIP_TRY(c, hipMemcpyAsync(c->t2_parts.p, parts.data(), (size_t)nparts * sizeof(T2Part), hipMemcpyHostToDevice, st), "upload");
        T2PartsArgs pa{};
        pa.npackets = (uint32_t)npk; pa.ntiles = ntiles; pa.nparts = nparts; pa.parts = (const T2Part*)c->t2_parts.p;
        pa.pk_hdr = ha.pk_hdr; pa.pk_body = ha.pk_body; pa.tile_index = (const uint32_t*)c->t2_index.p;
        pa.extra = sop + eph; pa.plt = plt ? 1u : 0u; pa.dst_offset = dst_offset;
        pa.lit = (uint8_t*)c->t2_lit.p; pa.lit_stride = lit_stride; pa.lit_len = (uint32_t*)c->t2_litlen.p;
        pa.tp_len = (uint32_t*)o.tp_len.p; pa.tp_dst = (unsigned long long*)o.tp_dst.p; pa.pk_dst = (uint64_t*)c->t2_pkdst.p;
        pa.part_len = (uint32_t*)o.part_len.p; pa.tile_dst = (unsigned long long*)o.tile_dst.p; pa.total = (unsigned long long*)o.total.p;
        pa.status = src.status;
        HIP_TRY(c, launch_t2_part_frames(pa, st), "launch tile-part frames");
        HIP_TRY(c, launch_t2_part_places(pa, st), "launch tile-part places");
        HIP_TRY(c, launch_t2_part_packets(pa, st), "launch tile-part packet places");
        T2GatherArgs ga{};
        ga.packets = (const T2Packet*)src.d_packets; ga.npackets = (uint32_t)npk; ga.packet_of_block = (const uint32_t*)src.d_pob;
        ga.lengths = src.lengths; ga.offsets = src.offsets; ga.arena = src.arena;
        ga.bpt = bpt; ga.ntiles = ntiles;
        ga.hdr = (const uint8_t*)c->t2_h.p; ga.h_bytes = plan.h_bytes;
        ga.rel = (const uint32_t*)c->t2_rel.p; ga.pk_hdr = (const uint32_t*)c->t2_pkhdr.p; ga.pk_dst = (const uint64_t*)c->t2_pkdst.p;
        ga.lit = (const uint8_t*)c->t2_lit.p; ga.lit_stride = lit_stride; ga.lit_len = (const uint32_t*)c->t2_litlen.p;
        ga.tile_dst = (const unsigned long long*)o.tile_dst.p;
        ga.out = (uint8_t*)o.out.p;
        ga.sop = sop; ga.eph = eph;
        HIP_TRY(c, launch_t2_gather_parts(ga, pa.parts, nparts, pa.tp_dst, st), "launch Tier-2 gather");
        return GRK_AMD_OK;
    }
    T2FrameArgs fa{};
    fa.npackets = (uint32_t)npk; fa.ntiles = ntiles; fa.pk_hdr = ha.pk_hdr; fa.pk_body = ha.pk_body;
    fa.tile_index = (const uint32_t*)c->t2_index.p; fa.extra = sop + eph; fa.plt = (flags & GRK_AMD_CS_PLT) ? 1u : 0u;
    fa.dst_offset = dst_offset;
    fa.lit = (uint8_t*)c->t2_lit.p; fa.lit_stride = lit_stride; fa.lit_len = (uint32_t*)c->t2_litlen.p;
    fa.pk_dst = (uint64_t*)c->t2_pkdst.p;
    fa.part_len = (uint32_t*)o.part_len.p; fa.tile_dst = (unsigned long long*)o.tile_dst.p; fa.total = (unsigned long long*)o.total.p;
    fa.status = src.status;
    HIP_TRY(c, launch_t2_frame(fa, st), "launch Tier-2 frames");
    T2GatherArgs ga{};
    ga.packets = (const T2Packet*)src.d_packets; ga.npackets = (uint32_t)npk; ga.packet_of_block = (const uint32_t*)src.d_pob;
    ga.lengths = src.lengths; ga.offsets = src.offsets; ga.arena = src.arena;
    ga.bpt = bpt; ga.ntiles = ntiles;
    ga.hdr = (const uint8_t*)c->t2_h.p; ga.h_bytes = plan.h_bytes;
    ga.rel = (const uint32_t*)c->t2_rel.p; ga.pk_hdr = (const uint32_t*)c->t2_pkhdr.p; ga.pk_dst = (const uint64_t*)c->t2_pkdst.p;
    ga.lit = (const uint8_t*)c->t2_lit.p; ga.lit_stride = lit_stride; ga.lit_len = (const uint32_t*)c->t2_litlen.p;
    ga.tile_dst = (const unsigned long long*)o.tile_dst.p;
    ga.out = (uint8_t*)o.out.p;
    ga.sop = sop; ga.eph = eph;
    HIP_TRY(c, launch_t2_gather(ga, st), "launch Tier-2 gather");
    return GRK_AMD_OK;
}

// a plan's tables on the device, complete on return (what read the buffers' earlier contents is drained first)
int upload_plan(grk_amd_ctx* c, const T2Plan& plan, DevBuf& packets, DevBuf& pob, hipStream_t st)
{
    HIP_TRY(c, hipStreamSynchronize(st), "sync");
    HIP_TRY(c, hipStreamSynchronize(c->stream), "sync");
    HIP_TRY(c, packets.ensure(plan.packets.size() * sizeof(T2Packet) + 16), "alloc packet table");
    HIP_TRY(c, pob.ensure(plan.packet_of_block.size() * 4 + 16), "alloc packet-of-block table");
    HIP_TRY(c, hipMemcpyAsync(packets.p, plan.packets.data(), plan.packets.size() * sizeof(T2Packet), hipMemcpyHostToDevice, st), "upload");
    HIP_TRY(c, hipMemcpyAsync(pob.p, plan.packet_of_block.data(), plan.packet_of_block.size() * 4, hipMemcpyHostToDevice, st), "upload");
    HIP_TRY(c, hipStreamSynchronize(st), "sync");
    return GRK_AMD_OK;
}

uint32_t plan_max_blocks(const T2Plan& plan)
{
    uint32_t m = 0;
    for (const T2Packet& k : plan.packets) m = std::max(m, k.nblocks);
    return m;
}

// the plan of the context's geometry in the order of `flags` -- cached in c->t2 on the parameters and the order
// (msbs: the plan of the general zero-bit-plane tree, asked for by the calls that write it -- never through the flag)
int call_plan(grk_amd_ctx* c, const grk_amd_tile_params* p, uint32_t flags, hipStream_t st, bool msbs = false)
{
    const uint32_t order = (flags >> GRK_AMD_CS_PROG_SHIFT) & 7u;
    if (!msbs && (flags & GRK_AMD_CS_BLOCK_MSBS)) return fail(c, GRK_AMD_ERR_UNSUPPORTED, "per-block zero bit-planes: the host writers only");
    const uint32_t tp = (flags >> GRK_AMD_CS_TP_SHIFT) & 3u;
    { std::string why; const int np = tile_part_count(flags, p->num_levels, p->num_comps, &why); if (np < 0) return fail(c, np, why.c_str()); }
    auto& T = c->t2;
    if (!T.valid || !same_params(T.p, *p) || T.order != order || T.tp != tp || T.msbs != msbs) {
        T.valid = false;
        int rc = msbs ? t2_device_plan_msbs(c->geom, flags, T.plan) : t2_device_plan(c->geom, flags, T.plan);
        if (rc) return fail(c, rc, "tile layout beyond the device writer's tables");
        T.max_blocks = plan_max_blocks(T.plan);
        // (the tables of the plan before may still be read by a gather that is queued: drained first)
        if ((rc = upload_plan(c, T.plan, T.packets, T.pob, st))) return rc;
        T.p = *p; T.order = order; T.tp = tp; T.msbs = msbs; T.valid = true;
    }
    return GRK_AMD_OK;
}

// the latest grk_amd_encode_tiles call as a source: the context's own table and arena under the plan of its geometry
int latest_call_source(grk_amd_ctx* c, const grk_amd_tile_params* p, uint32_t ntiles, uint32_t flags, hipStream_t st, T2Source& src)
{
    { const int rc = call_plan(c, p, flags, st); if (rc) return rc; }
    auto& T = c->t2;
    src = T2Source{&T.plan, T.max_blocks, T.packets.p, T.pob.p, (uint32_t)(c->last_nblocks / ntiles), (const uint32_t*)c->lengths.p,
                   (const uint64_t*)c->offsets.p, (const uint8_t*)c->arena.p, (uint64_t)c->arena.cap, (unsigned int*)c->flag.p};
    return GRK_AMD_OK;
}

int assemble_check(grk_amd_ctx* c, const grk_amd_tile_params* p, uint32_t ntiles, const uint32_t* tile_index)
{
    if (!c || !p || !ntiles || !tile_index) return GRK_AMD_ERR_INVALID;
    if (!c->have_geom || !same_params(c->gp, *p) || c->geom.reduce || ntiles != c->last_ntiles || !c->last_nblocks)
        return fail(c, GRK_AMD_ERR_INVALID, "grk_amd_assemble_device assembles the grk_amd_encode_tiles call before it: same tiles, same parameters");
    for (uint32_t i = 0; i < ntiles; ++i)
        if (tile_index[i] > 65535u) return fail(c, GRK_AMD_ERR_INVALID, "grk_amd_assemble_device: a tile index beyond 65 535 (Isot is 16 bits)");
    return GRK_AMD_OK;
}

// the status word's bits as an error (bits 0-1: K3's, 2 and 4: KT1's, 3: KT1b's)
int status_error(grk_amd_ctx* c, uint64_t word)
{
    if (word & 1u) return fail(c, GRK_AMD_ERR_OVERFLOW, "coded arena overflow");
    if (word & 2u) return fail(c, GRK_AMD_ERR_UNSUPPORTED, "coefficient magnitude exceeds Kmax+1 bits");
    if (word & 4u) return fail(c, GRK_AMD_ERR_UNSUPPORTED, "a code-block longer than the device writer takes");
    if (word & 8u) return fail(c, GRK_AMD_ERR_UNSUPPORTED, "tile-part beyond 4 GB or packet lengths beyond what PLT can carry");
    if (word & 16u) return fail(c, GRK_AMD_ERR_UNSUPPORTED, "a code-block with more zero bit-planes than the device writer takes");
    return GRK_AMD_OK;
}

// ---- the joint route ---------------------------------------------------------------------------------------------------------------
// The plans of the image's tile classes in c->t2j: made when the image (layout, parameters, factors, order) is not the one they were
// made for.  A class is framed by ONE assemble_enqueue call, which wants its tiles' rows one tile after the other: the image's tables
// therefore hold the classes one behind the other, within a class the tiles in order, within a tile the runs in order -- for an
// image of one class (any single-tile image, any image on its grid) the order of the host writers' tables.
int joint_plans(grk_amd_ctx* c, const JointT2Call& call, bool msbs)
{
    auto& J = c->t2j;
    const uint32_t flags = call.flags, order = (flags >> GRK_AMD_CS_PROG_SHIFT) & 7u, nr = call.nruns, nc = call.base->num_comps;
    const UnitGroups& g = *call.g;
    const uint32_t tp = (flags >> GRK_AMD_CS_TP_SHIFT) & 3u;
    if (J.valid && J.msbs == msbs && std::memcmp(&J.im, call.im, sizeof J.im) == 0 && same_params(J.base, *call.base) && J.order == order && J.tp == tp && J.dx.size() == nc &&
        std::memcmp(J.dx.data(), call.comp_dx, nc) == 0 && std::memcmp(J.dy.data(), call.comp_dy, nc) == 0 && J.unit_row.size() == g.of.size())
        return GRK_AMD_OK;
    J.valid = false;
    const uint32_t ntiles = (uint32_t)(g.of.size() / nr);
    const std::vector<CompRun> runs = comp_runs(nc, call.base->mct != 0, call.comp_dx, call.comp_dy);
    if (runs.size() != nr || (size_t)ntiles * nr != g.of.size()) return GRK_AMD_ERR_INVALID;
    // a tile's components as the tile-part writer takes them: cg[c] the geometry of the tile's OWN unit (a group's geometry stands
    // for its first unit's place on the grid only), row0[c]
    struct TileComps { std::vector<TileGeom> geoms; std::vector<const TileGeom*> cg; std::vector<uint64_t> row0; grk_amd_tile_params tile; };
    auto comps_of = [&](uint32_t t, TileComps& tc) -> int {
        int rc = grk_amd_layout_tile(call.im, call.base, t, &tc.tile);
        if (rc) return rc;
        tc.geoms.assign(nr, TileGeom{}); tc.cg.assign(nc, nullptr); tc.row0.assign(nc, 0);
        uint64_t rows = 0;
        for (uint32_t k = 0; k < nr; ++k) {
            grk_amd_tile_params p{};
            if ((rc = grk_amd_layout_tile_comp(call.im, call.base, call.comp_dx[runs[k].first], call.comp_dy[runs[k].first], t, &p))) return rc;
            p.num_comps = (uint16_t)runs[k].count; p.mct = runs[k].mct ? 1 : 0;
            if ((rc = build_tile_geom(p, tc.geoms[k]))) return rc;
            for (uint32_t i = 0; i < runs[k].count; ++i) { tc.cg[runs[k].first + i] = &tc.geoms[k]; tc.row0[runs[k].first + i] = rows; rows += tc.geoms[k].blocks_per_comp; }
        }
        return GRK_AMD_OK;
    };
    std::vector<std::vector<Pk>> seq(order >= 2 ? ntiles : 0);
    TileComps tc;
    for (uint32_t t = 0; t < (uint32_t)seq.size(); ++t) {
        const int rc = comps_of(t, tc);
        if (rc) return rc;
        seq[t] = packet_order(tc.cg, call.comp_dx, call.comp_dy, tc.tile.tile_x0, tc.tile.tile_y0, order);
    }
    std::vector<uint32_t> class_of;
    const uint32_t nclasses = joint_tile_classes(g.of, nr, order, seq, class_of);
    // (the tables of the classes before may still be read by a gather that is queued)
    HIP_TRY(c, hipStreamSynchronize(c->stream), "sync");
    for (size_t k = nclasses; k < J.classes.size(); ++k) { J.classes[k].packets.release(); J.classes[k].pob.release(); }
    J.classes.resize(nclasses);
    for (auto& K : J.classes) K.tiles.clear();
    for (uint32_t t = 0; t < ntiles; ++t) J.classes[class_of[t]].tiles.push_back(t);
    J.unit_row.assign(g.of.size(), 0);
    uint64_t row = 0;
    for (auto& K : J.classes) {
        int rc = comps_of(K.tiles[0], tc);
        if (rc) return rc;
        // (the general zero-bit-plane tree is asked for by name, never through the flag)
        if ((rc = msbs ? t2_device_plan_joint_msbs(tc.cg, tc.row0, call.comp_dx, call.comp_dy, tc.tile.tile_x0, tc.tile.tile_y0, flags, K.plan)
                       : t2_device_plan_joint(tc.cg, tc.row0, call.comp_dx, call.comp_dy, tc.tile.tile_x0, tc.tile.tile_y0, flags, K.plan))) return rc;
        K.max_blocks = plan_max_blocks(K.plan);
        K.bpt = (uint32_t)K.plan.packet_of_block.size();
        K.row_begin = row;
        for (uint32_t t : K.tiles)
            for (uint32_t k = 0; k < nr; ++k) {
                const TileGeom& G = g.geoms[g.of[(size_t)t * nr + k]];
                J.unit_row[(size_t)t * nr + k] = row;
                row += (uint64_t)G.blocks_per_comp * G.p.num_comps;
            }
        if (row - K.row_begin != (uint64_t)K.bpt * K.tiles.size()) return GRK_AMD_ERR_INVALID;
        if ((rc = upload_plan(c, K.plan, K.packets, K.pob, c->stream))) return rc;
    }
    J.rows = row;
    J.im = *call.im; J.base = *call.base; J.order = order; J.tp = tp; J.msbs = msbs;
    J.dx.assign(call.comp_dx, call.comp_dx + nc); J.dy.assign(call.comp_dy, call.comp_dy + nc);
    J.valid = true;
    return GRK_AMD_OK;
}

// `b` at least n bytes, its first `keep` bytes kept (the stream drained around the move)
int grow_keeping(grk_amd_ctx* c, DevBuf& b, size_t n, size_t keep, const char* what)
{
    if (n <= b.cap) return GRK_AMD_OK;
    HIP_TRY(c, hipStreamSynchronize(c->stream), "sync");
    DevBuf bigger;
    HIP_TRY(c, bigger.ensure(n), what);
    if (keep) HIP_TRY(c, hipMemcpy(bigger.p, b.p, keep, hipMemcpyDeviceToDevice), what);
    b.release();
    b = bigger;
    return GRK_AMD_OK;
}
} // namespace

int grk_amd::assembled_part_bytes(grk_amd_ctx* c, uint32_t ntiles, uint32_t* out)
{
    auto& o = c->t2_outs[c->t2_cur];
    HIP_TRY(c, hipMemcpyAsync(out, o.nparts > 1 ? o.tp_len.p : o.part_len.p, (size_t)ntiles * o.nparts * 4, hipMemcpyDeviceToHost, c->stream), "fetch the parts' lengths");
    HIP_TRY(c, hipStreamSynchronize(c->stream), "sync");
    return GRK_AMD_OK;
}

bool grk_amd::image_t2_host()
{
    const char* const e = std::getenv("GRK_AMD_IMAGE_T2");
    return e && std::strcmp(e, "host") == 0;
}

// ---- encode_joint_device in its three parts: plans and buffers | a batch, coded by the caller, kept | the classes framed, the file ----
int grk_amd::joint_device_open(JointT2Run& r)
{
    grk_amd_ctx* const c = r.c;
    const JointT2Call& call = *r.call;
    const uint32_t nr = call.nruns;
    const UnitGroups& g = *call.g;
    if (!nr || g.of.empty() || g.of.size() % nr) return GRK_AMD_ERR_INVALID;
    r.ntiles = (uint32_t)(g.of.size() / nr);
    if ((call.flags & GRK_AMD_CS_TLM) && r.ntiles > 255) return GRK_AMD_ERR_UNSUPPORTED;
    {   // tiles divided into tile-parts: the plain encodes alone (a rate's byte budget would have to count the extra frames)
        if (r.msbs && (call.flags & GRK_AMD_CS_TP(3))) return fail(c, GRK_AMD_ERR_UNSUPPORTED, "GRK_AMD_CS_TP: not taken by the rate- and quality-targeted calls");
        const int np = image_division(c, call.flags, call.base, r.ntiles);
        if (np < 0) return np;
        r.nparts = (uint32_t)np;
    }
    HIP_TRY(c, hipSetDevice(c->device), "set device");
    { const int rc = joint_plans(c, call, r.msbs); if (rc) return rc; }
    auto& J = c->t2j;
    // the file's main header does not depend on the lengths it will carry (fixed-width TLM fields): its size now
    r.part_len.assign(r.ntiles, 0);
    r.tp_len.assign((size_t)r.ntiles * r.nparts, 0);
    r.hdr_bytes = main_header_any(call.im, call.base, call.comp_dx, call.comp_dy, call.flags, r.ntiles, r.nparts, r.nparts > 1 ? r.tp_len.data() : r.part_len.data(), nullptr, 0);
    if (r.hdr_bytes < 0) return (int)r.hdr_bytes;
    r.nb = call.batches.size();
    std::vector<uint64_t>& rowlist = r.rowlist;              // (uploaded in stream order: it lives as long as the run)
    rowlist.clear();
    r.batch_at.assign(r.nb + 1, 0);
    for (size_t b = 0; b < r.nb; ++b) {
        for (uint32_t u : call.batches[b]) { if (u >= J.unit_row.size()) return GRK_AMD_ERR_INVALID; rowlist.push_back(J.unit_row[u]); }
        r.batch_at[b + 1] = rowlist.size();
    }
    if (rowlist.size() != g.of.size()) return GRK_AMD_ERR_INVALID;           // (every unit in exactly one batch: the sizes at least)
    // (every call of this route ends synchronised: none of these buffers is in use)
    HIP_TRY(c, c->jt_len.ensure(J.rows * 4 + 16), "alloc the image's lengths");
    HIP_TRY(c, c->jt_off.ensure(J.rows * 8 + 16), "alloc the image's offsets");
    if (r.msbs) HIP_TRY(c, c->jt_msbs.ensure(J.rows + 16), "alloc the image's zero bit-planes");
    HIP_TRY(c, c->jt_state.ensure((r.nb + 1) * 8 + 16), "alloc the image's cursors");
    HIP_TRY(c, c->jt_rowat.ensure(rowlist.size() * 8 + 16), "alloc the units' rows");
    HIP_TRY(c, hipMemcpyAsync(c->jt_rowat.p, rowlist.data(), rowlist.size() * 8, hipMemcpyHostToDevice, c->stream), "upload the units' rows");
    return joint_device_reset(r);
}

// the image's cursors and status word at zero: before the first batch of the image -- or of a round that codes every batch again
int grk_amd::joint_device_reset(JointT2Run& r)
{
    grk_amd_ctx* const c = r.c;
    HIP_TRY(c, hipMemsetAsync(c->jt_state.p, 0, (r.nb + 1) * 8 + 16, c->stream), "clear the image's cursors");
    r.bound_at = 0;
    return GRK_AMD_OK;
}

// batch b, which the caller has just coded (its table, bytes and -- a launch with drops -- drop bytes are the context's), kept: KK
int grk_amd::joint_device_keep(JointT2Run& r, size_t b)
{
    grk_amd_ctx* const c = r.c;
    const JointT2Call& call = *r.call;
    const UnitGroups& g = *call.g;
    const std::vector<uint32_t>& B = call.batches[b];
    if (B.empty()) return GRK_AMD_ERR_INVALID;
    const TileGeom& G = g.geoms[g.of[B[0]]];
    const uint64_t bpu = (uint64_t)G.blocks_per_comp * G.p.num_comps;
    unsigned long long* const cursors = (unsigned long long*)c->jt_state.p;
    int rc;
    if ((rc = join_side(c))) return rc;
    if (c->last_nblocks != bpu * B.size() || bpu >> 32) return fail(c, GRK_AMD_ERR_INVALID, "a batch's table is not its units'");
    // the image's arena: sized from the arena K3's plan asked for -- known before the launch, never read back
    const uint64_t ab = std::min<uint64_t>((c->last_arena_bound + 15u) & ~15ull, (uint64_t)c->arena.cap & ~15ull);
    if ((rc = grow_keeping(c, c->jt_arena, r.bound_at + ab + 16, r.bound_at, "alloc the image's arena"))) return rc;
    T2KeepArgs ka{};
    ka.lengths = (const uint32_t*)c->lengths.p; ka.offsets = (const unsigned long long*)c->offsets.p;
    ka.arena = (const uint8_t*)c->arena.p; ka.arena_bound = ab;
    ka.batch_state = (const unsigned long long*)c->flag.p;
    ka.nunits = (uint32_t)B.size(); ka.bpu = (uint32_t)bpu;
    ka.row_at = (const unsigned long long*)c->jt_rowat.p + r.batch_at[b];
    ka.j_lengths = (uint32_t*)c->jt_len.p; ka.j_offsets = (unsigned long long*)c->jt_off.p;
    ka.j_arena = (uint8_t*)c->jt_arena.p; ka.j_cap = r.bound_at + ab;
    ka.cursors = cursors + b; ka.status = (unsigned int*)(cursors + r.nb + 1);
    if (r.msbs) {
        // the rows' zero bit-planes from the drops the batch was coded with (a plain launch: none dropped), under the batch's own Kmax
        ka.drops = c->last_drops; ka.blocks = (const HtBlockDesc*)c->blockdesc.p; ka.j_msbs = (uint8_t*)c->jt_msbs.p;
    }
    HIP_TRY(c, launch_t2_keep(ka, c->stream), "launch keep");
    r.bound_at += ab;
    return GRK_AMD_OK;
}

int64_t grk_amd::joint_device_finish(JointT2Run& r, uint8_t* out, uint64_t cap, void** d_file)
{
    grk_amd_ctx* const c = r.c;
    const JointT2Call& call = *r.call;
    const uint32_t flags = call.flags, ntiles = r.ntiles;
    const int64_t hdr_bytes = r.hdr_bytes;
    const uint64_t bound_at = r.bound_at;
    std::vector<uint32_t>& part_len = r.part_len;
    auto& J = c->t2j;
    unsigned int* const status = (unsigned int*)((unsigned long long*)c->jt_state.p + r.nb + 1);
    if (!out && !d_file) return GRK_AMD_ERR_INVALID;
    // ---- the tile-parts, class by class, each behind the one before ----
    // a file in device memory is assembled in place behind its header when the classes' tile-parts come in the file's order
    bool in_order = true;
    { uint32_t next = 0; for (const auto& K : J.classes) for (uint32_t t : K.tiles) in_order = in_order && t == next++; }
    const bool in_place = d_file && in_order;
    auto& o = c->t2_outs[c->t2_cur];
    std::vector<uint64_t> dev_at(ntiles, 0);
    const uint64_t first = in_place ? (uint64_t)hdr_bytes : 0;
    uint64_t used = first;
    uint32_t status_word = 0;
    for (const auto& K : J.classes) {
        const T2Source src{&K.plan, K.max_blocks, K.packets.p, K.pob.p, K.bpt, (const uint32_t*)c->jt_len.p + K.row_begin,
                           (const uint64_t*)c->jt_off.p + K.row_begin, (const uint8_t*)c->jt_arena.p, bound_at, status,
                           r.msbs ? (const uint8_t*)c->jt_msbs.p + K.row_begin : nullptr};
        const int rc = assemble_enqueue(c, src, (uint32_t)K.tiles.size(), K.tiles.data(), flags, used, c->stream, o);
        if (rc) return rc;
        // only the tile-parts' lengths (and the status word) come to the host
        std::vector<uint32_t> lens(K.tiles.size()), tpl(r.nparts > 1 ? K.tiles.size() * r.nparts : 0);
        HIP_TRY(c, hipMemcpyAsync(lens.data(), o.part_len.p, lens.size() * 4, hipMemcpyDeviceToHost, c->stream), "fetch tile-part lengths");
        // (divided tiles: the parts' lengths for TLM beside the spans)
        if (!tpl.empty()) HIP_TRY(c, hipMemcpyAsync(tpl.data(), o.tp_len.p, tpl.size() * 4, hipMemcpyDeviceToHost, c->stream), "fetch the parts' lengths");
        HIP_TRY(c, hipMemcpyAsync(&status_word, status, 4, hipMemcpyDeviceToHost, c->stream), "fetch status");
        HIP_TRY(c, hipStreamSynchronize(c->stream), "sync");
        { const int se = status_error(c, status_word); if (se) return se; }
        for (size_t i = 0; i < lens.size(); ++i) { part_len[K.tiles[i]] = lens[i]; dev_at[K.tiles[i]] = used; used += lens[i]; }
        for (size_t i = 0; i < tpl.size(); ++i) r.tp_len[(size_t)K.tiles[i / r.nparts] * r.nparts + i % r.nparts] = tpl[i];
    }
    c->t2_out_used = used;

    if (!d_file) {
        const int64_t n = frame_file(call.im, call.base, flags, part_len, out, cap, [&](const std::vector<uint64_t>& at) -> int {
            for (uint32_t t = 0; t < ntiles; ++t) {
                // (tile-parts that lie one behind the other on the device as in the file go in one piece)
                uint32_t t1 = t;
                uint64_t n1 = part_len[t];
                while (t1 + 1 < ntiles && dev_at[t1 + 1] == dev_at[t] + n1) { n1 += part_len[t1 + 1]; ++t1; }
                const int fr = grk_amd_fetch_assembled(c, dev_at[t], n1, out + at[t]);
                if (fr) return fr;
                t = t1;
            }
            return GRK_AMD_OK;
        }, call.comp_dx, call.comp_dy, r.nparts, r.tp_len.data());
        return n;
    }
    // the file on the device: the header -- written now that the lengths are known -- and EOC around the tile-parts
    std::vector<uint8_t> hdr((size_t)hdr_bytes + 2);
    const int64_t hn = main_header_any(call.im, call.base, call.comp_dx, call.comp_dy, flags, ntiles, r.nparts, r.nparts > 1 ? r.tp_len.data() : part_len.data(), hdr.data(), (uint64_t)hdr_bytes);
    if (hn != hdr_bytes) return hn < 0 ? hn : GRK_AMD_ERR_INVALID;
    const uint64_t body = used - first, total = (uint64_t)hdr_bytes + body + 2;
    uint8_t* file = (uint8_t*)o.out.p;                     // (assemble_enqueue left 16 bytes free behind the tile-parts)
    if (!in_place) {
        HIP_TRY(c, c->jt_file.ensure(total + 16), "alloc the file");
        file = (uint8_t*)c->jt_file.p;
        uint64_t at = (uint64_t)hdr_bytes;
        for (uint32_t t = 0; t < ntiles; ++t) {
            HIP_TRY(c, hipMemcpyAsync(file + at, (const uint8_t*)o.out.p + dev_at[t], part_len[t], hipMemcpyDeviceToDevice, c->stream), "place a tile-part");
            at += part_len[t];
        }
    }
    const uint8_t eoc[2] = {0xFF, 0xD9};
    HIP_TRY(c, hipMemcpyAsync(file, hdr.data(), (size_t)hdr_bytes, hipMemcpyHostToDevice, c->stream), "upload the main header");
    HIP_TRY(c, hipMemcpyAsync(file + hdr_bytes + body, eoc, 2, hipMemcpyHostToDevice, c->stream), "upload EOC");
    HIP_TRY(c, hipStreamSynchronize(c->stream), "sync");
    *d_file = file;
    return (int64_t)total;
}

int64_t grk_amd::encode_joint_device(grk_amd_ctx* c, const JointT2Call& call, uint8_t* out, uint64_t cap, void** d_file)
{
    if (!out && !d_file) return GRK_AMD_ERR_INVALID;
    // what the device writer does not reach is said before any batch is coded
    if (call.flags & GRK_AMD_CS_BLOCK_MSBS) return GRK_AMD_ERR_UNSUPPORTED;
    JointT2Run r{c, &call, false};
    { const int rc = joint_device_open(r); if (rc) return rc; }
    // ---- every batch coded and kept (no host step between them but what grk_amd_encode_tiles has itself) ----
    for (size_t b = 0; b < r.nb; ++b) {
        if (call.batches[b].empty()) return GRK_AMD_ERR_INVALID;
        int rc = call.front(b);
        if (rc) return rc;
        if ((rc = joint_device_keep(r, b))) return rc;
    }
    const int64_t n = joint_device_finish(r, out, cap, d_file);
    if (n >= 0) ++c->route_counters[0];
    return n;
}

extern "C" {
uint64_t grk_amd_encode_route_counters(grk_amd_ctx* c, int which)
{
    return c && which >= 0 && which < 2 ? c->route_counters[which] : 0;
}

int64_t grk_amd_assemble_device(grk_amd_ctx* c, const grk_amd_tile_params* p, uint32_t ntiles, const uint32_t* tile_index, uint32_t flags,
                                uint64_t dst_offset, uint32_t* part_bytes)
{
    { const int rc = assemble_check(c, p, ntiles, tile_index); if (rc) return rc; }
    if (dst_offset > c->t2_out_used) return fail(c, GRK_AMD_ERR_INVALID, "grk_amd_assemble_device: dst_offset lies behind what has been assembled");
    HIP_TRY(c, hipSetDevice(c->device), "set device");
    { const int jr = join_side(c); if (jr) return jr; }
    auto& o = c->t2_outs[c->t2_cur];
    T2Source src;
    { const int rc = latest_call_source(c, p, ntiles, flags, c->stream, src); if (rc) return rc; }
    { const int rc = assemble_enqueue(c, src, ntiles, tile_index, flags, dst_offset, c->stream, o); if (rc) return rc; }
    uint64_t flagwords[2] = {0, 0}, total[2] = {0, 0};
    HIP_TRY(c, hipMemcpyAsync(flagwords, c->flag.p, 16, hipMemcpyDeviceToHost, c->stream), "fetch flag");
    HIP_TRY(c, hipMemcpyAsync(total, o.total.p, 16, hipMemcpyDeviceToHost, c->stream), "fetch total");
    if (part_bytes) HIP_TRY(c, hipMemcpyAsync(part_bytes, o.part_len.p, (size_t)ntiles * 4, hipMemcpyDeviceToHost, c->stream), "fetch tile-part lengths");
    HIP_TRY(c, hipStreamSynchronize(c->stream), "sync");
    { const int se = status_error(c, flagwords[0]); if (se) return se; }
    c->t2_out_used = total[1];
    return (int64_t)total[0];
}

// grk_amd_assemble_device for the grk_amd_encode_tiles_rate / _quality call before it (any launch of the block coder's drop instances):
// the rows' zero bit-planes are written, made on the device from the context's copy of the drop bytes the blocks were coded with --
// those calls are identity runs, the drops are in table order.  GRK_AMD_ERR_INVALID when the latest encode took no drops.
int64_t grk_amd_assemble_rate_device(grk_amd_ctx* c, const grk_amd_tile_params* p, uint32_t ntiles, const uint32_t* tile_index, uint32_t flags,
                                     uint64_t dst_offset, uint32_t* part_bytes)
{
    { const int rc = assemble_check(c, p, ntiles, tile_index); if (rc) return rc; }
    if (!c->last_drops) return fail(c, GRK_AMD_ERR_INVALID, "grk_amd_assemble_rate_device assembles a rate- or quality-targeted grk_amd_encode_tiles call: the latest encode dropped nothing");
    if (dst_offset > c->t2_out_used) return fail(c, GRK_AMD_ERR_INVALID, "grk_amd_assemble_rate_device: dst_offset lies behind what has been assembled");
    HIP_TRY(c, hipSetDevice(c->device), "set device");
    { const int jr = join_side(c); if (jr) return jr; }
    flags &= ~(uint32_t)GRK_AMD_CS_BLOCK_MSBS;                                // (accepted and implied)
    { const int rc = call_plan(c, p, flags, c->stream, true); if (rc) return rc; }
    auto& T = c->t2;
    const uint32_t bpt = (uint32_t)(c->last_nblocks / ntiles);
    HIP_TRY(c, hipStreamSynchronize(c->stream), "sync");                      // (st_msbs may still be read by an earlier call)
    HIP_TRY(c, c->st_msbs.ensure(c->last_nblocks + 16), "alloc zero bit-planes");
    HIP_TRY(c, launch_t2_drop_msbs(c->last_drops, (const HtBlockDesc*)c->blockdesc.p, bpt, c->last_nblocks, (uint8_t*)c->st_msbs.p, c->stream), "launch zero bit-planes");
    const T2Source src{&T.plan, T.max_blocks, T.packets.p, T.pob.p, bpt, (const uint32_t*)c->lengths.p, (const uint64_t*)c->offsets.p,
                       (const uint8_t*)c->arena.p, (uint64_t)c->arena.cap, (unsigned int*)c->flag.p, (const uint8_t*)c->st_msbs.p};
    auto& o = c->t2_outs[c->t2_cur];
    { const int rc = assemble_enqueue(c, src, ntiles, tile_index, flags, dst_offset, c->stream, o); if (rc) return rc; }
    uint64_t flagwords[2] = {0, 0}, total[2] = {0, 0};
    HIP_TRY(c, hipMemcpyAsync(flagwords, c->flag.p, 16, hipMemcpyDeviceToHost, c->stream), "fetch flag");
    HIP_TRY(c, hipMemcpyAsync(total, o.total.p, 16, hipMemcpyDeviceToHost, c->stream), "fetch total");
    if (part_bytes) HIP_TRY(c, hipMemcpyAsync(part_bytes, o.part_len.p, (size_t)ntiles * 4, hipMemcpyDeviceToHost, c->stream), "fetch tile-part lengths");
    HIP_TRY(c, hipStreamSynchronize(c->stream), "sync");
    { const int se = status_error(c, flagwords[0]); if (se) return se; }
    c->t2_out_used = total[1];
    return (int64_t)total[0];
}

// Tier-2 on the device for a table of the caller's choosing (the stage call of KT1 / KT1b / KT2, as grk_amd_stage_ht_encode16 is
// K3's): `table` holds num_tiles x (blocks of a tile) rows in the order of grk_amd_fetch_table, whose offsets point into the `coded`
// bytes -- rows may share bytes.  Everything is checked on the host before anything is launched; the tile-parts are read with
// grk_amd_fetch_assembled.  The rows and bytes go to buffers of their own: the latest grk_amd_encode_tiles call stays assemblable.
// (msbs: grk_amd_stage_assemble_msbs, `who` -- the rows' missing_msbs are written, through the general zero-bit-plane tree)
// (starts / nparts: grk_amd_stage_assemble_parts -- the tiles divided at these packets, part_bytes then [tile][part]; NULL: no division
//  but the flags')
static int64_t stage_assemble_any(grk_amd_ctx* c, const grk_amd_tile_params* p, uint32_t ntiles, const uint32_t* tile_index, uint32_t flags,
                                  const grk_amd_coded_block* table, const uint8_t* coded, uint64_t coded_bytes, uint32_t* part_bytes,
                                  bool msbs, const char* who, const uint32_t* starts = nullptr, uint32_t nparts = 0, bool per_part = false)
{
    char msg[200];
    if (!c || !p || !ntiles || !tile_index || !table || (!coded && coded_bytes) || (!starts != !nparts)) return GRK_AMD_ERR_INVALID;
    if (starts) {
        flags &= ~(uint32_t)GRK_AMD_CS_TP(3);                                 // (the caller's division, not the flags')
        bool ok = nparts <= kMaxTileParts && starts[0] == 0;
        for (uint32_t k = 1; ok && k < nparts; ++k) ok = starts[k - 1] <= starts[k];
        if (!ok) { std::snprintf(msg, sizeof msg, "%s: 1 .. 255 tile-parts whose first packets do not decrease, the first at 0", who); return fail(c, GRK_AMD_ERR_INVALID, msg); }
    }
    if (msbs) flags &= ~(uint32_t)GRK_AMD_CS_BLOCK_MSBS;                      // (accepted and implied)
    if (flags & GRK_AMD_CS_BLOCK_MSBS) return fail(c, GRK_AMD_ERR_UNSUPPORTED, "grk_amd_stage_assemble: per-block zero bit-planes: the host writers only");
    for (uint32_t i = 0; i < ntiles; ++i)
        if (tile_index[i] > 65535u) {
            std::snprintf(msg, sizeof msg, "%s: a tile index beyond 65 535 (Isot is 16 bits)", who);
            return fail(c, GRK_AMD_ERR_INVALID, msg);
        }
    { const int rc = stage_enter(c, p, true, true); if (rc) return rc; }
    const uint64_t bpt = (uint64_t)c->geom.blocks_per_comp * p->num_comps, rows = bpt * ntiles;
    if (bpt >> 32) { std::snprintf(msg, sizeof msg, "%s: tile layout beyond the device writer's tables", who); return fail(c, GRK_AMD_ERR_UNSUPPORTED, msg); }
    std::vector<uint32_t> h_len(rows);
    std::vector<uint64_t> h_off(rows);
    std::vector<uint8_t> h_msbs(msbs ? rows : 0);
    uint64_t sum = 0;
    for (uint64_t i = 0; i < rows; ++i) {
        const grk_amd_coded_block& r = table[i];
        if (!t2_len_ok(r.length)) {
            std::snprintf(msg, sizeof msg, "%s: row %llu: a length of %u bytes, the device writer takes less than %u",
                          who, (unsigned long long)i, r.length, 1u << kT2MaxLenBits);
            return fail(c, GRK_AMD_ERR_UNSUPPORTED, msg);
        }
        if (r.offset > coded_bytes || r.length > coded_bytes - r.offset) {
            std::snprintf(msg, sizeof msg, "%s: row %llu: offset %llu + length %u lies beyond the %llu coded bytes",
                          who, (unsigned long long)i, (unsigned long long)r.offset, r.length, (unsigned long long)coded_bytes);
            return fail(c, GRK_AMD_ERR_INVALID, msg);
        }
        if (msbs && r.missing_msbs > kT2MaxMsbs) {
            std::snprintf(msg, sizeof msg, "%s: row %llu: %u zero bit-planes, the device writer takes at most %u",
                          who, (unsigned long long)i, r.missing_msbs, kT2MaxMsbs);
            return fail(c, GRK_AMD_ERR_UNSUPPORTED, msg);
        }
        h_len[i] = r.length; h_off[i] = r.offset; sum += r.length;
        if (msbs) h_msbs[i] = (uint8_t)r.missing_msbs;
    }
    { const int rc = call_plan(c, p, flags, c->stream, msbs); if (rc) return rc; }
    if (starts && starts[nparts - 1] > c->t2.plan.packets.size()) {
        std::snprintf(msg, sizeof msg, "%s: a tile-part from packet %u on, the tile has %zu", who, starts[nparts - 1], c->t2.plan.packets.size());
        return fail(c, GRK_AMD_ERR_INVALID, msg);
    }
    // (no call of this entry leaves work behind: the buffers are free)
    HIP_TRY(c, c->st_len.ensure(rows * 4 + 16), "alloc the stage's lengths");
    HIP_TRY(c, c->st_off.ensure(rows * 8 + 16), "alloc the stage's offsets");
    HIP_TRY(c, c->st_arena.ensure(coded_bytes + 16), "alloc the stage's coded bytes");
    HIP_TRY(c, c->st_status.ensure(16), "alloc the stage's status word");
    HIP_TRY(c, hipMemcpyAsync(c->st_len.p, h_len.data(), rows * 4, hipMemcpyHostToDevice, c->stream), "upload lengths");
    HIP_TRY(c, hipMemcpyAsync(c->st_off.p, h_off.data(), rows * 8, hipMemcpyHostToDevice, c->stream), "upload offsets");
    if (msbs) {
        HIP_TRY(c, c->st_msbs.ensure(rows + 16), "alloc the stage's zero bit-planes");
        HIP_TRY(c, hipMemcpyAsync(c->st_msbs.p, h_msbs.data(), rows, hipMemcpyHostToDevice, c->stream), "upload zero bit-planes");
    }
    if (coded_bytes) { const int rc = copy_h2d(c, c->st_arena.p, coded, coded_bytes); if (rc) return rc; }
    HIP_TRY(c, hipMemsetAsync(c->st_status.p, 0, 16, c->stream), "clear status");
    auto& T = c->t2;
    // (rows may share bytes: what the call writes is bounded by the sum of the lengths, not by the bytes they point into)
    const T2Source src{&T.plan, T.max_blocks, T.packets.p, T.pob.p, (uint32_t)bpt, (const uint32_t*)c->st_len.p, (const uint64_t*)c->st_off.p,
                       (const uint8_t*)c->st_arena.p, sum, (unsigned int*)c->st_status.p, msbs ? (const uint8_t*)c->st_msbs.p : nullptr};
    auto& o = c->t2_outs[c->t2_cur];
    c->t2_out_used = 0;
    { const int rc = assemble_enqueue(c, src, ntiles, tile_index, flags, 0, c->stream, o, starts, nparts); if (rc) return rc; }
    uint32_t status_word = 0;
    uint64_t total[2] = {0, 0};
    HIP_TRY(c, hipMemcpyAsync(&status_word, c->st_status.p, 4, hipMemcpyDeviceToHost, c->stream), "fetch status");
    HIP_TRY(c, hipMemcpyAsync(total, o.total.p, 16, hipMemcpyDeviceToHost, c->stream), "fetch total");
    if (part_bytes && per_part && o.nparts > 1) HIP_TRY(c, hipMemcpyAsync(part_bytes, o.tp_len.p, (size_t)ntiles * o.nparts * 4, hipMemcpyDeviceToHost, c->stream), "fetch the parts' lengths");
    else if (part_bytes) HIP_TRY(c, hipMemcpyAsync(part_bytes, o.part_len.p, (size_t)ntiles * 4, hipMemcpyDeviceToHost, c->stream), "fetch tile-part lengths");
    HIP_TRY(c, hipStreamSynchronize(c->stream), "sync");
    { const int se = status_error(c, status_word); if (se) return se; }
    c->t2_out_used = total[1];
    return (int64_t)total[0];
}

int64_t grk_amd_stage_assemble(grk_amd_ctx* c, const grk_amd_tile_params* p, uint32_t ntiles, const uint32_t* tile_index, uint32_t flags,
                               const grk_amd_coded_block* table, const uint8_t* coded, uint64_t coded_bytes, uint32_t* part_bytes)
{
    return stage_assemble_any(c, p, ntiles, tile_index, flags, table, coded, coded_bytes, part_bytes, false, "grk_amd_stage_assemble");
}

// The same with the rows' missing_msbs written: the zero-bit-plane tag trees in their general form (KT1's instance of it), what
// grk_amd_write_tile_part writes under GRK_AMD_CS_BLOCK_MSBS -- the flag is accepted here and implied.  The same host checks before
// any launch, and GRK_AMD_ERR_UNSUPPORTED for a row above grk_amd_t2_max_block_msbs().
int64_t grk_amd_stage_assemble_msbs(grk_amd_ctx* c, const grk_amd_tile_params* p, uint32_t ntiles, const uint32_t* tile_index, uint32_t flags,
                                    const grk_amd_coded_block* table, const uint8_t* coded, uint64_t coded_bytes, uint32_t* part_bytes)
{
    return stage_assemble_any(c, p, ntiles, tile_index, flags, table, coded, coded_bytes, part_bytes, true, "grk_amd_stage_assemble_msbs");
}

// grk_amd_stage_assemble with the tiles divided into tile-parts: at the caller's packets (starts[nparts], as grk_amd_write_tile_parts
// takes them), or with starts == NULL under the division of `flags`.  part_bytes: [num_tiles][parts], the parts' lengths.
int64_t grk_amd_stage_assemble_parts(grk_amd_ctx* c, const grk_amd_tile_params* p, uint32_t ntiles, const uint32_t* tile_index, uint32_t flags,
                                     const grk_amd_coded_block* table, const uint8_t* coded, uint64_t coded_bytes,
                                     const uint32_t* starts, uint32_t nparts, uint32_t* part_bytes)
{
    return stage_assemble_any(c, p, ntiles, tile_index, flags, table, coded, coded_bytes, part_bytes, false, "grk_amd_stage_assemble_parts", starts, nparts, true);
}

uint32_t grk_amd_assembled_parts(grk_amd_ctx* c) { return c ? c->t2_outs[c->t2_cur].nparts : 0; }

uint32_t grk_amd_t2_max_block_msbs(void) { return kT2MaxMsbs; }
uint32_t grk_amd_t2_max_block_bytes(void) { return (1u << kT2MaxLenBits) - 1u; }

// The same without the host: queued on `hip_stream` (made to wait for the encode's results first, as grk_amd_stream_wait_results does),
// nothing is waited for.  Pipelined encodes rotate as many outputs as buffer sets: a frame's tile-parts, their places / lengths and the
// total (grk_amd_assembled_device_ptr, grk_amd_assembled_table_ptr) stay untouched until that many further calls -- time for an
// exchange to send them.  Every asynchronous call of a context has to use the SAME stream (the scratch is shared, stream order keeps
// the calls apart); errors (bits 0-3 of the encode's status word) are the consumer's to find: the bytes will not parse.
int grk_amd_assemble_device_async(grk_amd_ctx* c, const grk_amd_tile_params* p, uint32_t ntiles, const uint32_t* tile_index, uint32_t flags,
                                  void* hip_stream)
{
    { const int rc = assemble_check(c, p, ntiles, tile_index); if (rc) return rc; }
    if (!hip_stream) return GRK_AMD_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device), "set device");
    { const int rc = grk_amd_stream_wait_results(c, hip_stream); if (rc) return rc; }
    const int nsets = c->pipelining ? std::max(1, std::min(c->pipe_depth, grk_amd_ctx::kMaxAltSets + 1)) : 1;
    c->t2_cur = (c->t2_cur + 1) % nsets;
    c->t2_out_used = 0;
    T2Source src;
    { const int rc = latest_call_source(c, p, ntiles, flags, (hipStream_t)hip_stream, src); if (rc) return rc; }
    return assemble_enqueue(c, src, ntiles, tile_index, flags, 0, (hipStream_t)hip_stream, c->t2_outs[c->t2_cur]);
}

void* grk_amd_assembled_device_ptr(grk_amd_ctx* c) { return c ? c->t2_outs[c->t2_cur].out.p : nullptr; }
// of the latest assemble call -- 0: uint64[tiles] where each tile-part starts, 1: uint32[tiles] its length, 2: uint64[2] {bytes the call
// assembled, end of the output}
void* grk_amd_assembled_table_ptr(grk_amd_ctx* c, int which)
{
    if (!c) return nullptr;
    auto& o = c->t2_outs[c->t2_cur];
    // (3: uint32[tiles][grk_amd_assembled_parts] the tile-parts' lengths; tables 0 and 1 are the tiles' -- of a divided tile its span)
    return which == 0 ? o.tile_dst.p : which == 1 ? o.part_len.p : which == 2 ? o.total.p : which == 3 ? (o.nparts > 1 ? o.tp_len.p : o.part_len.p) : nullptr;
}

// bytes [offset, offset + nbytes) of the assembled tile-parts to host memory: pinned memory in one DMA, pageable memory through the
// context's pinned chunks on several copy threads (copy_d2h); complete on return
int grk_amd_fetch_assembled(grk_amd_ctx* c, uint64_t offset, uint64_t nbytes, uint8_t* dst)
{
    if (!c || !dst || offset > c->t2_out_used || nbytes > c->t2_out_used - offset) return GRK_AMD_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device), "set device");
    if (!nbytes) return GRK_AMD_OK;
    { const int rc = copy_d2h(c, dst, (const uint8_t*)c->t2_outs[c->t2_cur].out.p + offset, nbytes); if (rc) return rc; }
    HIP_TRY(c, hipStreamSynchronize(c->stream), "sync");
    return GRK_AMD_OK;
}

// the same queued on the context's stream, for pinned memory only; complete after grk_amd_synchronize
int grk_amd_fetch_assembled_async(grk_amd_ctx* c, uint64_t offset, uint64_t nbytes, uint8_t* dst)
{
    if (!c || !dst || offset > c->t2_out_used || nbytes > c->t2_out_used - offset) return GRK_AMD_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device), "set device");
    if (!host_is_pinned(dst)) return fail(c, GRK_AMD_ERR_INVALID, "grk_amd_fetch_assembled_async needs pinned memory (grk_amd_host_alloc)");
    if (nbytes) HIP_TRY(c, hipMemcpyAsync(dst, (const uint8_t*)c->t2_outs[c->t2_cur].out.p + offset, nbytes, hipMemcpyDeviceToHost, c->stream), "download");
    return GRK_AMD_OK;
}
} // extern "C"
