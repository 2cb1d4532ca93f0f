// grok_amd/csrc/rate.hip -- rate-targeted HT encodes: a batch of tiles in at most N bytes of code-blocks, a whole image in a file of
// at most N bytes.
//
// The front end and a plain K3 run as in grk_amd_encode_tiles.  Then, on the planes that encode left: KR1 (kernels_rate.hip) gives
// every candidate's error per block, Dmax + 1 trial launches of the block coder's drop instances (kernels_ht.hip DROP; uniform
// d = 0 .. Dmax, the arena rewound in between, only the length column kept) give every candidate's exact length, KR2 chooses each
// block's drop for the budget, and a last launch codes the blocks with those drops.  No per-block data comes to the host before the
// final table does.
#include "context.h"
#include "image.h"

namespace {

// front end + plain K3 + the tables L, E, W for `ntiles` tiles of *p.  plain_table (optional, host): the rows of the plain encode
int rate_prepare(grk_amd_ctx* c, const grk_amd_tile_params* p, uint32_t ntiles, const void* pixels, int on_device, const grk_amd_rate* rate,
                 grk_amd_coded_block* plain_table)
{
    if (!c || !p || !pixels || !ntiles || !rate) return GRK_AMD_ERR_INVALID;
    c->rate.valid = false;
    if (c->pipelining) return fail(c, GRK_AMD_ERR_UNSUPPORTED, "rate-targeted encodes are not pipelined (grk_amd_set_pipelining(ctx, 0))");
    if (!plan_rate(rate->max_drop, rate->allow_skip != 0, 0).ok) return fail(c, GRK_AMD_ERR_INVALID, "grk_amd_rate::max_drop above 12");
    // (synchronous, with the arena / range flags checked: the trial launches below code from the planes this leaves)
    uint64_t total = 0;
    int rc = grk_amd_encode_tiles(c, p, ntiles, pixels, on_device, plain_table, &total); if (rc) return rc;
    const TileGeom& g = c->geom;
    const uint64_t n = c->last_nblocks;
    const uint32_t bpt = (uint32_t)(n / ntiles);
    const RatePlan rp = plan_rate(rate->max_drop, rate->allow_skip != 0, n);
    HIP_TRY(c, c->rate_L.ensure(rp.l_bytes), "alloc rate lengths");
    HIP_TRY(c, c->rate_E.ensure(rp.e_bytes), "alloc rate errors");
    HIP_TRY(c, c->rate_W.ensure(rp.w_bytes), "alloc rate weights");
    HIP_TRY(c, c->rate_drop.ensure(rp.drop_bytes), "alloc drops");
    HIP_TRY(c, c->rate_res.ensure(sizeof(RateAllocResult)), "alloc rate result");
    // W_b = (w_mct * w_band * stepsize)^2 / 4: E counts half steps
    std::vector<double> w(n);
    for (uint32_t i = 0; i < bpt; ++i) { const double v = block_weight(g, i); w[i] = v * v * 0.25; }
    for (uint64_t i = bpt; i < n; ++i) w[i] = w[i - bpt];
    HIP_TRY(c, hipMemcpyAsync(c->rate_W.p, w.data(), n * 8, hipMemcpyHostToDevice, c->stream), "upload rate weights");
    HIP_TRY(c, hipStreamSynchronize(c->stream), "sync");
    RateStatsArgs sa{};
    sa.mallat = c->p1.p; sa.h16 = c->last_h16 ? 1 : 0; sa.irreversible = g.p.irreversible; sa.stride = g.stride; sa.pitch = g.plane_elems;
    sa.blocks = (const HtBlockDesc*)c->blockdesc.p; sa.blocks_per_tile = bpt; sa.ncomp = g.p.num_comps; sa.nblocks = n;
    sa.dmax = rp.dmax; sa.E = (unsigned long long*)c->rate_E.p;
    HIP_TRY(c, launch_rate_stats(sa, c->stream), "launch rate statistics");
    HIP_TRY(c, hipMemsetAsync(c->rate_L.p, 0, rp.l_bytes, c->stream), "clear rate lengths");          // (the SKIP row stays 0)
    for (uint32_t d = 0; d < rp.trials; ++d) {
        HIP_TRY(c, hipMemsetAsync(c->rate_drop.p, (int)d, n, c->stream), "uniform drops");
        rc = ht_encode_drops(c, ntiles, c->p1.p, c->last_h16, (const uint8_t*)c->rate_drop.p); if (rc) return rc;
        HIP_TRY(c, hipMemcpyAsync((uint32_t*)c->rate_L.p + (uint64_t)d * n, c->lengths.p, n * 4, hipMemcpyDeviceToDevice, c->stream), "keep the lengths");
    }
    c->rate.valid = true; c->rate.plan = rp; c->rate.nblocks = n; c->rate.ntiles = ntiles;
    return GRK_AMD_OK;
}

// KR2 for `budget` bytes of code-blocks over the prepared tables, then the blocks coded with the chosen drops
int rate_allocate(grk_amd_ctx* c, uint64_t budget, RateAllocResult& res)
{
    if (!c->rate.valid) return GRK_AMD_ERR_INVALID;
    const RatePlan& rp = c->rate.plan;
    RateAllocArgs a{};
    a.L = (const uint32_t*)c->rate_L.p; a.E = (const unsigned long long*)c->rate_E.p; a.W = (const double*)c->rate_W.p;
    a.nblocks = c->rate.nblocks; a.dmax = rp.dmax; a.ncand = rp.ncand; a.budget = budget;
    a.drop = (uint8_t*)c->rate_drop.p; a.res = (RateAllocResult*)c->rate_res.p;
    {
        ScopedTimer t(c, 9);
        HIP_TRY(c, launch_rate_alloc(a, c->stream), "launch rate allocator");
    }
    HIP_TRY(c, hipMemcpyAsync(&res, c->rate_res.p, sizeof(res), hipMemcpyDeviceToHost, c->stream), "fetch rate result");
    HIP_TRY(c, hipStreamSynchronize(c->stream), "sync");
    if (!res.feasible) {
        char msg[160];
        std::snprintf(msg, sizeof(msg), "the budget of %llu bytes is below the %llu that %s everywhere takes", (unsigned long long)budget,
                      res.least_bytes, rp.ncand == rp.dmax + 2u ? "SKIP" : "the largest drop");
        return fail(c, GRK_AMD_ERR_OVERFLOW, msg);
    }
    return ht_encode_drops(c, c->rate.ntiles, c->p1.p, c->last_h16, (const uint8_t*)c->rate_drop.p);
}

void fill_result(grk_amd_rate_result* out, const RateAllocResult& r, uint64_t file_bytes, uint32_t passes)
{
    if (!out) return;
    std::memset(out, 0, sizeof(*out));
    out->block_bytes = r.block_bytes; out->lagrange_bytes = r.lagrange_bytes; out->file_bytes = file_bytes;
    out->distortion = r.distortion; out->lambda = r.lambda; out->passes = passes;
}

// Several geometry groups: each its share of the budget by sample count, but never more than its plain bytes -- what a group cannot
// use goes to the others, again by sample count (so a budget of all the plain bytes gives every group exactly its own: nothing is
// dropped anywhere); the last group still open takes the rounding's remainder
std::vector<uint64_t> group_shares(uint64_t budget, const std::vector<uint64_t>& samples, const std::vector<uint64_t>& plain)
{
    const size_t n = samples.size();
    std::vector<uint64_t> share(n, 0);
    std::vector<bool> full(n, false);
    for (;;) {
        uint64_t open_samples = 0, left = budget;
        for (size_t k = 0; k < n; ++k) { if (full[k]) left -= share[k]; else open_samples += samples[k]; }
        if (!open_samples) break;
        bool again = false;
        for (size_t k = 0; k < n && !again; ++k) {
            if (full[k]) continue;
            if ((uint64_t)((unsigned __int128)left * samples[k] / open_samples) >= plain[k]) { share[k] = plain[k]; full[k] = true; again = true; }
        }
        if (again) continue;
        uint64_t given = 0;
        size_t last = n;
        for (size_t k = 0; k < n; ++k) if (!full[k]) last = k;
        for (size_t k = 0; k < n; ++k) {
            if (full[k]) continue;
            share[k] = k == last ? left - given : (uint64_t)((unsigned __int128)left * samples[k] / open_samples);
            given += share[k];
        }
        break;
    }
    return share;
}

// a successful call's note to grk_amd_last_error: what the decoders at hand make of a reversible file with planes dropped
void note_reversible(grk_amd_ctx* c, const grk_amd_tile_params& p, bool dropped)
{
    c->err = (!p.irreversible && dropped)
        ? "note: 5/3 blocks with d planes dropped are returned as mu >> d by Grok's and this library's reversible dequantiser (not the bin centre the reported distortion assumes); use the 9/7 transform for such decoders"
        : "";
}

// the file's length for a table (sizes only: nothing is written)
int64_t sized_file(const grk_amd_image_layout* im, const grk_amd_tile_params* base, uint32_t flags, const std::vector<grk_amd_coded_block>& rows)
{
    const int64_t nt = grk_amd_layout_num_tiles(im);
    if (nt < 0) return nt;
    std::vector<uint32_t> part((size_t)nt, 0);
    uint64_t sum = 0, row = 0;
    for (uint32_t t = 0; t < (uint32_t)nt; ++t) {
        grk_amd_tile_params p;
        const int rc = grk_amd_layout_tile(im, base, t, &p); if (rc) return rc;
        const int64_t len = grk_amd_write_tile_part(&p, t, flags, rows.data() + row, nullptr, nullptr, 0);
        if (len < 0) return len;
        const int64_t nb = grk_amd_tile_num_blocks(&p);
        if (nb < 0) return nb;
        row += (uint64_t)nb; sum += (uint64_t)len; part[t] = (uint32_t)len;
    }
    const int64_t hdr = grk_amd_write_main_header_layout(im, base, flags, part.data(), nullptr, 0);
    return hdr < 0 ? hdr : (int64_t)(hdr + sum + 2);
}

} // namespace

extern "C" {

int grk_amd_encode_tiles_rate(grk_amd_ctx* c, const grk_amd_tile_params* p, uint32_t ntiles, const void* pixels, int on_device,
                              const grk_amd_rate* rate, grk_amd_coded_block* table, uint64_t* total, grk_amd_rate_result* result)
{
    if (!c) return GRK_AMD_ERR_INVALID;
    int rc = rate_prepare(c, p, ntiles, pixels, on_device, rate, nullptr); if (rc) return rc;
    RateAllocResult r{};
    rc = rate_allocate(c, rate->target_bytes, r); if (rc) return rc;
    fill_result(result, r, 0, 1);
    if (table || total) { rc = grk_amd_fetch_table(c, table, total); if (rc) return rc; }
    note_reversible(c, *p, r.lambda > 0.0);
    return GRK_AMD_OK;
}

int grk_amd_rate_tables(grk_amd_ctx* c, int which, void* dst, uint64_t cap_bytes)
{
    if (!c || !dst || !c->rate.valid) return GRK_AMD_ERR_INVALID;
    const RatePlan& rp = c->rate.plan;
    const void* src; uint64_t bytes;
    switch (which) {
    case 0: src = c->rate_L.p; bytes = rp.l_bytes; break;
    case 1: src = c->rate_E.p; bytes = rp.e_bytes; break;
    case 2: src = c->rate_W.p; bytes = rp.w_bytes; break;
    case 3: src = c->rate_drop.p; bytes = rp.drop_bytes; break;
    default: return GRK_AMD_ERR_INVALID;
    }
    if (cap_bytes < bytes) return GRK_AMD_ERR_OVERFLOW;
    HIP_TRY(c, hipSetDevice(c->device), "set device");
    HIP_TRY(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream), "fetch rate table");
    HIP_TRY(c, hipStreamSynchronize(c->stream), "sync");
    return GRK_AMD_OK;
}

// Headers and packet headers depend on the allocation: the blocks' budget is the target less what the file of the round before spent
// beside its blocks (first: the plain file), and a file that still overshoots lowers the budget by its overshoot.
int64_t grk_amd_encode_image_rate(grk_amd_ctx* ctx, const grk_amd_image_layout* im, const grk_amd_tile_params* base, const void* pixels,
                                  uint32_t flags, const grk_amd_rate* rate, uint8_t* out, uint64_t cap, grk_amd_rate_result* result)
{
    if (!ctx || !im || !base || !pixels || !out || !rate) return GRK_AMD_ERR_INVALID;
    if (ctx->pipelining) return fail(ctx, GRK_AMD_ERR_UNSUPPORTED, "rate-targeted encodes are not pipelined (grk_amd_set_pipelining(ctx, 0))");
    flags |= GRK_AMD_CS_BLOCK_MSBS;
    std::vector<Unit> tiles;
    SourcePlanes src;
    UnitGroups g;
    const grk_amd_pixel_layout whole = ctx->enc_layout;
    int64_t rc = plain_image(im, base, pixels, flags, tiles, src, g, &whole);
    if (rc) return rc;
    KeepLayout staged{ctx->enc_layout, whole};
    ctx->enc_layout = staged_layout(src);
    const size_t ngroups = g.members.size();
    std::vector<uint64_t> row_at(tiles.size() + 1, 0), samples(ngroups, 0), plain_of(ngroups, 0);
    for (size_t u = 0; u < tiles.size(); ++u) {
        row_at[u + 1] = row_at[u] + (uint64_t)g.geoms[g.of[u]].blocks_per_comp * tiles[u].p.num_comps;
        samples[g.of[u]] += (uint64_t)tiles[u].p.tile_w * tiles[u].p.tile_h * tiles[u].p.num_comps;
    }
    std::vector<grk_amd_coded_block> rows(row_at.back());
    std::vector<uint8_t> coded, staging;
    // a group's tiles staged, coded plainly, its tables made (one group: once for all rounds)
    auto prepare = [&](size_t k, bool keep_plain) -> int {
        const auto& G = g.members[k];
        const grk_amd_tile_params& p = tiles[G[0]].p;
        staging.resize(staged_bytes(src, tiles[G[0]]) * G.size());
        stage_units(src, tiles, G, staging.data(), 1);
        const uint64_t bpu = (uint64_t)g.geoms[k].blocks_per_comp * p.num_comps;
        std::vector<grk_amd_coded_block> table(keep_plain ? bpu * G.size() : 0);
        const int pr = rate_prepare(ctx, &p, (uint32_t)G.size(), staging.data(), 0, rate, keep_plain ? table.data() : nullptr);
        if (pr) return pr;
        for (size_t i = 0; keep_plain && i < G.size(); ++i)
            for (uint64_t b = 0; b < bpu; ++b) rows[row_at[G[i]] + b] = table[i * bpu + b];
        return GRK_AMD_OK;
    };
    // the plain file's size and what it spends beside its blocks
    uint64_t plain_blocks = 0;
    for (size_t k = 0; k < ngroups; ++k) { rc = prepare(k, true); if (rc) return rc; }
    for (size_t u = 0; u < tiles.size(); ++u)
        for (uint64_t b = row_at[u]; b < row_at[u + 1]; ++b) { plain_of[g.of[u]] += rows[b].length; plain_blocks += rows[b].length; }
    const int64_t plain = sized_file(im, base, flags, rows);
    if (plain < 0) return plain;
    const uint64_t target = rate->target_bytes;
    uint64_t overhead = (uint64_t)plain - plain_blocks;
    uint64_t budget = target >= (uint64_t)plain ? plain_blocks : target > overhead ? target - overhead : 0;
    RateAllocResult sum{};
    for (uint32_t round = 1; round <= kRateMaxRounds; ++round) {
        coded.clear();
        sum = RateAllocResult{};
        const std::vector<uint64_t> share = group_shares(budget, samples, plain_of);
        for (size_t k = 0; k < ngroups; ++k) {
            if (ngroups > 1) { rc = prepare(k, false); if (rc) return rc; }
            RateAllocResult r{};
            rc = rate_allocate(ctx, share[k], r); if (rc) return rc;
            sum.block_bytes += r.block_bytes; sum.lagrange_bytes += r.lagrange_bytes; sum.distortion += r.distortion; sum.lambda = r.lambda;
            const auto& G = g.members[k];
            const uint64_t bpu = (uint64_t)g.geoms[k].blocks_per_comp * tiles[G[0]].p.num_comps;
            std::vector<grk_amd_coded_block> table(bpu * G.size());
            uint64_t total = 0;
            rc = grk_amd_fetch_table(ctx, table.data(), &total); if (rc) return rc;
            const size_t at = coded.size();
            coded.resize(at + total);
            if (total) { rc = grk_amd_fetch_coded(ctx, coded.data() + at, total); if (rc) return rc; }
            for (size_t i = 0; i < G.size(); ++i)
                for (uint64_t b = 0; b < bpu; ++b) { rows[row_at[G[i]] + b] = table[i * bpu + b]; rows[row_at[G[i]] + b].offset += at; }
        }
        const int64_t len = sized_file(im, base, flags, rows);
        if (len < 0) return len;
        if ((uint64_t)len <= target) {
            coded.push_back(0);                     // (the writer wants a buffer even when every block was skipped)
            const int64_t wrote = grk_amd_write_codestream_layout(im, base, rows.data(), coded.data(), flags, out, cap);
            if (wrote >= 0) { fill_result(result, sum, (uint64_t)wrote, round); note_reversible(ctx, *base, sum.block_bytes < plain_blocks); }
            return wrote;
        }
        const uint64_t over = (uint64_t)len - target;
        if (budget == 0 || sum.block_bytes == 0)          // nothing left to take from the blocks: the headers alone are too long
            return fail(ctx, GRK_AMD_ERR_OVERFLOW, "the target is below what the file takes with no byte of any block in it");
        budget = std::min<uint64_t>(budget, sum.block_bytes);
        budget = budget > over ? budget - over : 0;
    }
    return fail(ctx, GRK_AMD_ERR_OVERFLOW, "the file was still above the target after 4 allocate + write rounds (the target may be feasible: the rounds ran out)");
}

} // extern "C"
