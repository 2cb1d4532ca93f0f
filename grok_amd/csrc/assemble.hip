// grok_amd/csrc/assemble.hip -- Tier-2 on the device.
#include "context.h"

extern "C" {
// The finished tile-parts of the LATEST grk_amd_encode_tiles call, made where the coded bytes are (kernels_t2.hip): KT1 writes every
// packet's header, KT1b frames the tile-parts (SOT, PLT, SOD) and says where every packet goes, KT2 gathers headers, code-block bytes
// and frames into the output.  Nothing has to come to the host in between.
namespace {
// the kernels queued on `st`, which must already be ordered behind the encode's results; `o` takes the tile-parts from dst_offset on
// (what lies below is kept when the buffer has to grow).  The scratch is the context's: one stream at a time.
int assemble_enqueue(grk_amd_ctx* c, const grk_amd_tile_params* p, uint32_t ntiles, const uint32_t* tile_index, uint32_t flags,
                     uint64_t dst_offset, hipStream_t st, grk_amd_ctx::T2Out& o)
{
    const TileGeom& g = c->geom;
    const uint32_t order = (flags >> GRK_AMD_CS_PROG_SHIFT) & 7u;
    if (flags & GRK_AMD_CS_BLOCK_MSBS) return fail(c, GRK_AMD_ERR_UNSUPPORTED, "per-block zero bit-planes: the host writers only");
    auto& T = c->t2;
    if (!T.valid || !same_params(T.p, *p) || T.order != order) {
        T.valid = false;
        const int rc = t2_device_plan(g, flags, T.plan);
        if (rc) return fail(c, rc, "tile layout beyond the device writer's tables");
        T.max_blocks = 0;
        for (const T2Packet& k : T.plan.packets) T.max_blocks = std::max(T.max_blocks, k.nblocks);
        // (the tables of the plan before may still be read by a gather that is queued: drained first)
        HIP_TRY(c, hipStreamSynchronize(st), "sync");
        HIP_TRY(c, hipStreamSynchronize(c->stream), "sync");
        HIP_TRY(c, T.packets.ensure(T.plan.packets.size() * sizeof(T2Packet)), "alloc packet table");
        HIP_TRY(c, T.pob.ensure(T.plan.packet_of_block.size() * 4), "alloc packet-of-block table");
        HIP_TRY(c, hipMemcpyAsync(T.packets.p, T.plan.packets.data(), T.plan.packets.size() * sizeof(T2Packet), hipMemcpyHostToDevice, st), "upload");
        HIP_TRY(c, hipMemcpyAsync(T.pob.p, T.plan.packet_of_block.data(), T.plan.packet_of_block.size() * 4, hipMemcpyHostToDevice, st), "upload");
        HIP_TRY(c, hipStreamSynchronize(st), "sync");
        T.p = *p; T.order = order; T.valid = true;
    }
    const size_t npk = T.plan.packets.size();
    const uint32_t bpt = (uint32_t)(c->last_nblocks / ntiles);
    const size_t nq = npk * ntiles;
    // a frame: SOT 12, SOD 2, PLT: at most 6 bytes per packet and 5 per marker segment of 65 532
    const uint32_t lit_stride = (uint32_t)((14 + 6 * npk + 5 * (6 * npk / 65000 + 2) + 15) & ~(size_t)15);
    // what the call can write at most: every byte of the arena, every header, every frame
    const uint64_t bound = (uint64_t)c->arena.cap + (uint64_t)ntiles * (T.plan.h_bytes + lit_stride + 8ull * npk);
    auto need = [&](DevBuf& b, size_t n, const char* what) -> int {
        if (n <= b.cap) return GRK_AMD_OK;
        // (a scratch buffer about to be replaced may be in use by kernels queued earlier on the stream)
        HIP_TRY(c, hipStreamSynchronize(st), "sync");
        HIP_TRY(c, b.ensure(n), what);
        return GRK_AMD_OK;
    };
    int rc;
    if ((rc = need(c->t2_u, (size_t)T.plan.u_words * 4 * ntiles + 16, "alloc header bits"))) return rc;
    if ((rc = need(c->t2_h, (size_t)T.plan.h_bytes * ntiles + 16, "alloc headers"))) return rc;
    if ((rc = need(c->t2_rel, c->last_nblocks * 4, "alloc block places"))) return rc;
    if ((rc = need(c->t2_pkhdr, nq * 4, "alloc packet lengths"))) return rc;
    if ((rc = need(c->t2_pkbody, nq * 8, "alloc packet lengths"))) return rc;
    if ((rc = need(c->t2_pkdst, nq * 8, "alloc packet places"))) return rc;
    if ((rc = need(c->t2_lit, (size_t)lit_stride * ntiles, "alloc frames"))) return rc;
    if ((rc = need(c->t2_litlen, (size_t)ntiles * 4, "alloc frames"))) return rc;
    if ((rc = need(c->t2_index, (size_t)ntiles * 4, "alloc tile numbers"))) return rc;
    if ((rc = need(o.tile_dst, (size_t)ntiles * 8, "alloc tile-part places"))) return rc;
    if ((rc = need(o.part_len, (size_t)ntiles * 4, "alloc tile-part lengths"))) return rc;
    if ((rc = need(o.total, 16, "alloc tile-part total"))) return rc;
    if (o.out.cap < dst_offset + bound) {
        DevBuf bigger;
        HIP_TRY(c, hipStreamSynchronize(st), "sync");
        HIP_TRY(c, bigger.ensure(dst_offset + bound), "alloc tile-parts");
        if (dst_offset) HIP_TRY(c, hipMemcpyAsync(bigger.p, o.out.p, dst_offset, hipMemcpyDeviceToDevice, st), "keep tile-parts");
        HIP_TRY(c, hipStreamSynchronize(st), "sync");
        o.out.release();
        o.out = bigger;
    }
    HIP_TRY(c, hipMemsetAsync(c->t2_u.p, 0, (size_t)T.plan.u_words * 4 * ntiles, st), "clear header bits");
    // (the tile numbers: pageable memory of the caller's -- the runtime has staged them when the call returns)
    HIP_TRY(c, hipMemcpyAsync(c->t2_index.p, tile_index, (size_t)ntiles * 4, hipMemcpyHostToDevice, st), "upload");
    T2HeaderArgs ha{};
    ha.packets = (const T2Packet*)T.packets.p; ha.npackets = (uint32_t)npk;
    ha.lengths = (const uint32_t*)c->lengths.p; ha.bpt = bpt; ha.ntiles = ntiles;
    ha.ubits = (uint32_t*)c->t2_u.p; ha.u_words = T.plan.u_words;
    ha.hdr = (uint8_t*)c->t2_h.p; ha.h_bytes = T.plan.h_bytes;
    ha.rel = (uint32_t*)c->t2_rel.p; ha.pk_hdr = (uint32_t*)c->t2_pkhdr.p; ha.pk_body = (uint64_t*)c->t2_pkbody.p;
    ha.status = (unsigned int*)c->flag.p;
    HIP_TRY(c, launch_t2_header(ha, T.max_blocks, st), "launch Tier-2 headers");
    const uint32_t sop = (flags & GRK_AMD_CS_SOP) ? 6u : 0u, eph = (flags & GRK_AMD_CS_EPH) ? 2u : 0u;
    T2FrameArgs fa{};
    fa.npackets = (uint32_t)npk; fa.ntiles = ntiles; fa.pk_hdr = ha.pk_hdr; fa.pk_body = ha.pk_body;
    fa.tile_index = (const uint32_t*)c->t2_index.p; fa.extra = sop + eph; fa.plt = (flags & GRK_AMD_CS_PLT) ? 1u : 0u;
    fa.dst_offset = dst_offset;
    fa.lit = (uint8_t*)c->t2_lit.p; fa.lit_stride = lit_stride; fa.lit_len = (uint32_t*)c->t2_litlen.p;
    fa.pk_dst = (uint64_t*)c->t2_pkdst.p;
    fa.part_len = (uint32_t*)o.part_len.p; fa.tile_dst = (unsigned long long*)o.tile_dst.p; fa.total = (unsigned long long*)o.total.p;
    fa.status = (unsigned int*)c->flag.p;
    HIP_TRY(c, launch_t2_frame(fa, st), "launch Tier-2 frames");
    T2GatherArgs ga{};
    ga.packets = (const T2Packet*)T.packets.p; ga.npackets = (uint32_t)npk; ga.packet_of_block = (const uint32_t*)T.pob.p;
    ga.lengths = (const uint32_t*)c->lengths.p; ga.offsets = (const uint64_t*)c->offsets.p; ga.arena = (const uint8_t*)c->arena.p;
    ga.bpt = bpt; ga.ntiles = ntiles;
    ga.hdr = (const uint8_t*)c->t2_h.p; ga.h_bytes = T.plan.h_bytes;
    ga.rel = (const uint32_t*)c->t2_rel.p; ga.pk_hdr = (const uint32_t*)c->t2_pkhdr.p; ga.pk_dst = (const uint64_t*)c->t2_pkdst.p;
    ga.lit = (const uint8_t*)c->t2_lit.p; ga.lit_stride = lit_stride; ga.lit_len = (const uint32_t*)c->t2_litlen.p;
    ga.tile_dst = (const unsigned long long*)o.tile_dst.p;
    ga.out = (uint8_t*)o.out.p;
    ga.sop = sop; ga.eph = eph;
    HIP_TRY(c, launch_t2_gather(ga, st), "launch Tier-2 gather");
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
} // namespace

int64_t grk_amd_assemble_device(grk_amd_ctx* c, const grk_amd_tile_params* p, uint32_t ntiles, const uint32_t* tile_index, uint32_t flags,
                                uint64_t dst_offset, uint32_t* part_bytes)
{
    { const int rc = assemble_check(c, p, ntiles, tile_index); if (rc) return rc; }
    if (dst_offset > c->t2_out_used) return fail(c, GRK_AMD_ERR_INVALID, "grk_amd_assemble_device: dst_offset lies behind what has been assembled");
    HIP_TRY(c, hipSetDevice(c->device), "set device");
    { const int jr = join_side(c); if (jr) return jr; }
    auto& o = c->t2_outs[c->t2_cur];
    { const int rc = assemble_enqueue(c, p, ntiles, tile_index, flags, dst_offset, c->stream, o); if (rc) return rc; }
    uint64_t flagwords[2] = {0, 0}, total[2] = {0, 0};
    HIP_TRY(c, hipMemcpyAsync(flagwords, c->flag.p, 16, hipMemcpyDeviceToHost, c->stream), "fetch flag");
    HIP_TRY(c, hipMemcpyAsync(total, o.total.p, 16, hipMemcpyDeviceToHost, c->stream), "fetch total");
    if (part_bytes) HIP_TRY(c, hipMemcpyAsync(part_bytes, o.part_len.p, (size_t)ntiles * 4, hipMemcpyDeviceToHost, c->stream), "fetch tile-part lengths");
    HIP_TRY(c, hipStreamSynchronize(c->stream), "sync");
    if (flagwords[0] & 1u) return fail(c, GRK_AMD_ERR_OVERFLOW, "coded arena overflow");
    if (flagwords[0] & 2u) return fail(c, GRK_AMD_ERR_UNSUPPORTED, "coefficient magnitude exceeds Kmax+1 bits");
    if (flagwords[0] & 4u) return fail(c, GRK_AMD_ERR_UNSUPPORTED, "a code-block longer than the device writer takes");
    if (flagwords[0] & 8u) return fail(c, GRK_AMD_ERR_UNSUPPORTED, "tile-part beyond 4 GB or packet lengths beyond what PLT can carry");
    c->t2_out_used = total[1];
    return (int64_t)total[0];
}

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
    return assemble_enqueue(c, p, ntiles, tile_index, flags, 0, (hipStream_t)hip_stream, c->t2_outs[c->t2_cur]);
}

void* grk_amd_assembled_device_ptr(grk_amd_ctx* c) { return c ? c->t2_outs[c->t2_cur].out.p : nullptr; }
// of the latest assemble call -- 0: uint64[tiles] where each tile-part starts, 1: uint32[tiles] its length, 2: uint64[2] {bytes the call
// assembled, end of the output}
void* grk_amd_assembled_table_ptr(grk_amd_ctx* c, int which)
{
    if (!c) return nullptr;
    auto& o = c->t2_outs[c->t2_cur];
    return which == 0 ? o.tile_dst.p : which == 1 ? o.part_len.p : which == 2 ? o.total.p : nullptr;
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
