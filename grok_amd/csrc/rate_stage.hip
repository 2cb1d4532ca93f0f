// grok_amd/csrc/rate_stage.hip -- the stage calls of the rate path's kernels (kernels_rate.hip), as grk_amd_stage_ht_encode_drops is the
// drop instances': the statistics KR1 on planes of the caller's choosing, the allocators KR2 and KQ on tables of the caller's
// choosing.  Each works on buffers of its own (st_r*): the context's rate state (rate.hip) is not touched.  Everything is checked on
// the host before anything is launched.
#include "context.h"

namespace {

// KR2 or KQ on the caller's tables: one launch.  name: the entry point, for its refusals; what: "rate" or "quality"; budget_ok: the
// check only KQ's budget needs
template <class Args, class Result, class Budget>
int stage_alloc(grk_amd_ctx* c, const char* name, const char* what, hipError_t (*launch)(const Args&, hipStream_t), const uint32_t* L,
                const uint64_t* E, const double* W, uint64_t n, uint32_t max_drop, int allow_skip, Budget budget, bool budget_ok, uint8_t* drops,
                void* result)
{
    if (!c) return GRK_AMD_ERR_INVALID;
    char msg[128];
    const auto refuse = [&](const char* why) { std::snprintf(msg, sizeof(msg), "%s: %s", name, why); return fail(c, GRK_AMD_ERR_INVALID, msg); };
    if (!L || !E || !W || !drops || !result) return refuse("a null pointer");
    if (max_drop == 0 || max_drop > kRateMaxDrop) return refuse("max_drop is 1 .. 12");
    if (!n || n > kRateMaxBlocks) return refuse("no block, or more than the allocator indexes");
    if (!budget_ok) return refuse("a distortion budget that is negative or not a number");
    const uint64_t rows = max_drop + 2u;
    for (uint64_t i = 0; i < rows * n; ++i)
        if (L[i] >> 31) return refuse("a length of 2^31 bytes or more");
    HIP_TRY(c, hipSetDevice(c->device), "set device");
    HIP_TRY(c, c->st_rL.ensure(rows * n * 4u), "alloc the stage's lengths");
    HIP_TRY(c, c->st_rE.ensure(rows * n * 8u), "alloc the stage's errors");
    HIP_TRY(c, c->st_rW.ensure(n * 8u), "alloc the stage's weights");
    HIP_TRY(c, c->st_rdrop.ensure(n), "alloc the stage's drops");
    HIP_TRY(c, c->st_rres.ensure(sizeof(Result)), "alloc the stage's result");
    HIP_TRY(c, hipMemcpyAsync(c->st_rL.p, L, rows * n * 4u, hipMemcpyHostToDevice, c->stream), "upload lengths");
    HIP_TRY(c, hipMemcpyAsync(c->st_rE.p, E, rows * n * 8u, hipMemcpyHostToDevice, c->stream), "upload errors");
    HIP_TRY(c, hipMemcpyAsync(c->st_rW.p, W, n * 8u, hipMemcpyHostToDevice, c->stream), "upload weights");
    HIP_TRY(c, hipMemsetAsync(c->st_rres.p, 0, sizeof(Result), c->stream), "clear the result");
    const Args a = rate_alloc_args<Args>(c->st_rL, c->st_rE, c->st_rW, c->st_rdrop, c->st_rres, n, max_drop, max_drop + 1u + (allow_skip ? 1u : 0u), budget);
    std::snprintf(msg, sizeof(msg), "launch %s allocator", what);
    HIP_TRY(c, launch(a, c->stream), msg);
    std::snprintf(msg, sizeof(msg), "fetch %s result", what);
    HIP_TRY(c, hipMemcpyAsync(result, c->st_rres.p, sizeof(Result), hipMemcpyDeviceToHost, c->stream), msg);
    HIP_TRY(c, hipMemcpyAsync(drops, c->st_rdrop.p, n, hipMemcpyDeviceToHost, c->stream), "fetch drops");
    HIP_TRY(c, hipStreamSynchronize(c->stream), "sync");
    return GRK_AMD_OK;
}

} // namespace

extern "C" {

// KR1 on planes of the caller's choosing: over the context's block descriptors for *p, into a buffer of the stage's own -- through a
// map where the caller gives first rows, with the caller's E uploaded first
int grk_amd_stage_rate_stats(grk_amd_ctx* c, const grk_amd_tile_params* p, uint32_t ntiles, const void* d_mallat, int planes16, uint32_t max_drop,
                             const uint64_t* first_rows, uint64_t n, uint64_t* E)
{
    if (!c || !p || !ntiles || !d_mallat || !E) return GRK_AMD_ERR_INVALID;
    if (max_drop == 0 || max_drop > kRateMaxDrop) return fail(c, GRK_AMD_ERR_INVALID, "grk_amd_stage_rate_stats: max_drop is 1 .. 12");
    { const int rc = stage_enter(c, p, true, true, planes16 && !planes16_ok(*p) ? "grk_amd_stage_rate_stats: no encode keeps int16 planes for these parameters" : nullptr);
      if (rc) return rc; }
    const TileGeom& g = c->geom;
    const uint64_t bpt = (uint64_t)g.blocks_per_comp * g.p.num_comps, nblocks = bpt * ntiles;
    if (!first_rows) n = nblocks;
    if (!bpt || (bpt >> 32) || nblocks > kRateMaxBlocks || n > kRateMaxBlocks) return fail(c, GRK_AMD_ERR_UNSUPPORTED, "grk_amd_stage_rate_stats: more blocks than the statistics index");
    for (uint32_t t = 0; first_rows && t < ntiles; ++t)
        if (first_rows[t] > n || bpt > n - first_rows[t]) {
            char msg[160];
            std::snprintf(msg, sizeof msg, "grk_amd_stage_rate_stats: tile %u: rows %llu + %llu end beyond the %llu of the table", t,
                          (unsigned long long)first_rows[t], (unsigned long long)bpt, (unsigned long long)n);
            return fail(c, GRK_AMD_ERR_INVALID, msg);
        }
    const uint64_t e_bytes = (uint64_t)(max_drop + 2u) * n * 8u;
    HIP_TRY(c, c->st_rE.ensure(e_bytes), "alloc the stage's errors");
    if (first_rows) {
        HIP_TRY(c, c->st_rmap.ensure((uint64_t)ntiles * 8u), "alloc the stage's map");
        HIP_TRY(c, hipMemcpyAsync(c->st_rmap.p, first_rows, (uint64_t)ntiles * 8u, hipMemcpyHostToDevice, c->stream), "upload the map");
        HIP_TRY(c, hipMemcpyAsync(c->st_rE.p, E, e_bytes, hipMemcpyHostToDevice, c->stream), "upload the errors");
    }
    RateStatsArgs sa{};
    sa.mallat = d_mallat; sa.h16 = planes16 ? 1 : 0; sa.irreversible = g.p.irreversible; sa.stride = g.stride; sa.pitch = g.plane_elems;
    sa.blocks = (const HtBlockDesc*)c->blockdesc.p; sa.blocks_per_tile = (uint32_t)bpt; sa.ncomp = g.p.num_comps; sa.nblocks = nblocks;
    sa.dmax = max_drop; sa.E = (unsigned long long*)c->st_rE.p;
    sa.map = first_rows ? (const unsigned long long*)c->st_rmap.p : nullptr; sa.n = n;
    HIP_TRY(c, launch_rate_stats(sa, c->stream), "launch rate statistics");
    HIP_TRY(c, hipMemcpyAsync(E, c->st_rE.p, e_bytes, hipMemcpyDeviceToHost, c->stream), "fetch the errors");
    HIP_TRY(c, hipStreamSynchronize(c->stream), "sync");
    return GRK_AMD_OK;
}

int grk_amd_stage_rate_alloc(grk_amd_ctx* c, const uint32_t* L, const uint64_t* E, const double* W, uint64_t n, uint32_t max_drop, int allow_skip,
                             uint64_t budget, uint8_t* drops, grk_amd_rate_alloc_result* result)
{
    static_assert(sizeof(grk_amd_rate_alloc_result) == sizeof(RateAllocResult) && offsetof(grk_amd_rate_alloc_result, steps) == offsetof(RateAllocResult, steps),
                  "grk_amd_rate_alloc_result is RateAllocResult");
    return stage_alloc<RateAllocArgs, RateAllocResult>(c, "grk_amd_stage_rate_alloc", "rate", launch_rate_alloc, L, E, W, n, max_drop, allow_skip, budget, true,
                                                       drops, result);
}

int grk_amd_stage_quality_alloc(grk_amd_ctx* c, const uint32_t* L, const uint64_t* E, const double* W, uint64_t n, uint32_t max_drop, int allow_skip,
                                double D, uint8_t* drops, grk_amd_quality_alloc_result* result)
{
    static_assert(sizeof(grk_amd_quality_alloc_result) == sizeof(RateQualityResult) && offsetof(grk_amd_quality_alloc_result, steps) == offsetof(RateQualityResult, steps) &&
                  offsetof(grk_amd_quality_alloc_result, floor) == offsetof(RateQualityResult, floor), "grk_amd_quality_alloc_result is RateQualityResult");
    return stage_alloc<RateQualityArgs, RateQualityResult>(c, "grk_amd_stage_quality_alloc", "quality", launch_rate_quality, L, E, W, n, max_drop, allow_skip, D,
                                                           D >= 0.0, drops, result);
}

} // extern "C"
