// grok_amd/csrc/rate.hip -- rate-targeted HT encodes: a batch of tiles in at most N bytes of code-blocks, a whole image in a file of
// at most N bytes.
//
// The front end and a plain K3 run as in grk_amd_encode_tiles.  Then, on the planes that encode left: KR1 (kernels_rate.hip) gives
// every candidate's error per block, Dmax + 1 trial launches of the block coder's drop instances (kernels_ht.hip DROP; uniform
// d = 0 .. Dmax, the arena rewound in between, only the length column kept) give every candidate's exact length, KR2 chooses each
// block's drop for the budget, and a last launch codes the blocks with those drops.  No per-block data comes to the host before the
// final table does.
//
// A whole image whose units fall into several batches (tiles of several geometries; luma and chroma of a sub-sampled image or of a
// video surface) has ONE set of tables over all its blocks in the order the file's writer takes them (encode_rate_joint; the row
// order, the batches' maps and the bounds are plan_rate_joint's, encode_plan.h): each batch's KR1 and trial launches write their
// columns through the batch's map, KR2 runs once per round over the joint tables -- one multiplier for every block of every
// component --, and a batch is coded with its slice of the chosen drops.  The tables are made once per call.
//
// Quality-targeted encodes (grk_amd_encode_*_quality) take the same tables and, instead of KR2 and its rounds, run KQ once for a
// distortion budget (plan_quality, encode_plan.h), code the batches and write the file once.
#include "context.h"
#include "image.h"

namespace {

// KR1 and the Dmax + 1 trial launches over the planes the latest front end left (`ntiles` units of the context's geometry): the
// batch's columns of E and L, in rows of N entries -- through `map` (device: the units' first rows, plan_rate_joint), or with
// map == nullptr at the batch's own indices (N: its blocks).  drops: device scratch of one byte per block of the batch
int batch_tables(grk_amd_ctx* c, const RatePlan& rp, uint32_t ntiles, const unsigned long long* map, uint64_t N, void* drops)
{
    const TileGeom& g = c->geom;
    const uint64_t n = c->last_nblocks;
    const uint32_t bpt = (uint32_t)(n / ntiles);
    RateStatsArgs sa{};
    sa.mallat = c->p1.p; sa.h16 = c->last_h16 ? 1 : 0; sa.irreversible = g.p.irreversible; sa.stride = g.stride; sa.pitch = g.plane_elems;
    sa.blocks = (const HtBlockDesc*)c->blockdesc.p; sa.blocks_per_tile = bpt; sa.ncomp = g.p.num_comps; sa.nblocks = n;
    sa.dmax = rp.dmax; sa.E = (unsigned long long*)c->rate_E.p; sa.map = map; sa.n = N;
    HIP_TRY(c, launch_rate_stats(sa, c->stream), "launch rate statistics");
    for (uint32_t d = 0; d < rp.trials; ++d) {
        HIP_TRY(c, hipMemsetAsync(drops, (int)d, n, c->stream), "uniform drops");
        const int rc = ht_encode_drops(c, ntiles, c->p1.p, c->last_h16, (const uint8_t*)drops); if (rc) return rc;
        uint32_t* const row = (uint32_t*)c->rate_L.p + (uint64_t)d * N;
        if (map) HIP_TRY(c, launch_rate_map(RateMapArgs{c->lengths.p, row, map, bpt, n, 4u, 0}, c->stream), "keep the lengths");
        else HIP_TRY(c, hipMemcpyAsync(row, c->lengths.p, n * 4, hipMemcpyDeviceToDevice, c->stream), "keep the lengths");
    }
    return GRK_AMD_OK;
}

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
    HIP_TRY(c, hipMemsetAsync(c->rate_L.p, 0, rp.l_bytes, c->stream), "clear rate lengths");          // (the SKIP row stays 0)
    rc = batch_tables(c, rp, ntiles, nullptr, n, c->rate_drop.p); if (rc) return rc;
    c->rate.valid = true; c->rate.plan = rp; c->rate.nblocks = n; c->rate.ntiles = ntiles;
    c->rate.unit_rows.resize(ntiles);
    for (uint32_t t = 0; t < ntiles; ++t) c->rate.unit_rows[t] = (uint64_t)t * bpt;
    return GRK_AMD_OK;
}

// KR2 for `budget` bytes of code-blocks over the prepared tables: the chosen drop bytes in rate_drop
int rate_choose(grk_amd_ctx* c, uint64_t budget, RateAllocResult& res)
{
    if (!c->rate.valid) return GRK_AMD_ERR_INVALID;
    const RatePlan& rp = c->rate.plan;
    RateAllocArgs a{};
    a.L = (const uint32_t*)c->rate_L.p; a.E = (const unsigned long long*)c->rate_E.p; a.W = (const double*)c->rate_W.p;
    a.nblocks = c->rate.nblocks; a.dmax = rp.dmax; a.ncand = rp.ncand; a.budget = budget;
    a.drop = (uint8_t*)c->rate_drop.p; a.res = (RateAllocResult*)c->rate_res.p;
    c->rate.budget = budget; c->rate.qbudget = 0;
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
    return GRK_AMD_OK;
}

// KQ for a distortion budget over the prepared tables: the chosen drop bytes in rate_drop.  plain_blocks: the bytes of row 0 of L.
// A budget of 0 is answered without the allocator: nothing may be lost, so every block keeps d = 0 and the file is the plain one.
// (KQ alone would still take a coarser candidate of EQUAL error in fewer bytes -- in the model a lone odd magnitude survives one
// dropped plane -- which the 5/3 decoders at hand, positioning a block by its own zero bit-planes, do not return exactly.)
// The call around it is not shortened for that budget: it still makes all Dmax + 1 trial tables, which grk_amd_rate_tables serves
// afterwards as after any call, and codes every batch once more with drops of 0 to get the plain rows back -- work a caller who
// wants the plain file saves by asking for it (grk_amd_encode_image and its kin).
int quality_choose(grk_amd_ctx* c, double budget, uint64_t plain_blocks, RateQualityResult& res)
{
    if (!c->rate.valid) return GRK_AMD_ERR_INVALID;
    const RatePlan& rp = c->rate.plan;
    if (budget == 0.0) {
        HIP_TRY(c, hipMemsetAsync(c->rate_drop.p, 0, rp.drop_bytes, c->stream), "no drops");
        c->rate.budget = 0; c->rate.qbudget = 0;
        res = RateQualityResult{};
        res.block_bytes = res.lagrange_bytes = plain_blocks; res.feasible = 1;
        return GRK_AMD_OK;
    }
    HIP_TRY(c, c->rate_res.ensure(sizeof(RateQualityResult)), "alloc quality result");
    RateQualityArgs a{};
    a.L = (const uint32_t*)c->rate_L.p; a.E = (const unsigned long long*)c->rate_E.p; a.W = (const double*)c->rate_W.p;
    a.nblocks = c->rate.nblocks; a.dmax = rp.dmax; a.ncand = rp.ncand; a.budget = budget;
    a.drop = (uint8_t*)c->rate_drop.p; a.res = (RateQualityResult*)c->rate_res.p;
    c->rate.budget = 0; c->rate.qbudget = budget;
    {
        ScopedTimer t(c, 9);
        HIP_TRY(c, launch_rate_quality(a, c->stream), "launch quality allocator");
    }
    HIP_TRY(c, hipMemcpyAsync(&res, c->rate_res.p, sizeof(res), hipMemcpyDeviceToHost, c->stream), "fetch quality result");
    HIP_TRY(c, hipStreamSynchronize(c->stream), "sync");
    // (E[0] = 0 everywhere in the tables of an encode: the floor is 0 and every D >= 0 feasible)
    if (!res.feasible) return fail(c, GRK_AMD_ERR_OVERFLOW, "the distortion budget is below what the finest candidates leave");
    return GRK_AMD_OK;
}

void fill_quality_result(const QualityGoal& goal, const RateQualityResult& r, uint64_t file_bytes)
{
    grk_amd_quality_result* out = goal.result;
    if (!out) return;
    std::memset(out, 0, sizeof(*out));
    out->block_bytes = r.block_bytes; out->lagrange_bytes = r.lagrange_bytes; out->file_bytes = file_bytes;
    out->distortion = r.distortion; out->budget = goal.budget; out->psnr = quality_psnr(goal.signal, r.distortion);
    out->lambda = r.lambda; out->steps = r.steps;
}

// ... then the blocks of the one batch the tables are over coded with the chosen drops
int rate_allocate(grk_amd_ctx* c, uint64_t budget, RateAllocResult& res)
{
    const int rc = rate_choose(c, budget, res); if (rc) return rc;
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
int64_t sized_file(const grk_amd_image_layout* im, const grk_amd_tile_params* base, uint32_t flags, const grk_amd_coded_block* rows)
{
    const int64_t nt = grk_amd_layout_num_tiles(im);
    if (nt < 0) return nt;
    std::vector<uint32_t> part((size_t)nt, 0);
    uint64_t sum = 0, row = 0;
    for (uint32_t t = 0; t < (uint32_t)nt; ++t) {
        grk_amd_tile_params p;
        const int rc = grk_amd_layout_tile(im, base, t, &p); if (rc) return rc;
        const int64_t len = grk_amd_write_tile_part(&p, t, flags, rows + row, nullptr, nullptr, 0);
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

int grk_amd_encode_tiles_quality(grk_amd_ctx* c, const grk_amd_tile_params* p, uint32_t ntiles, const void* pixels, int on_device,
                                 const grk_amd_quality* quality, grk_amd_coded_block* table, uint64_t* total, grk_amd_quality_result* result)
{
    if (!c || !p || !pixels || !ntiles || !quality) return GRK_AMD_ERR_INVALID;
    c->rate.valid = false;
    QualityTarget qt;
    int rc = quality_target(c, quality, p->prec, (uint64_t)ntiles * p->tile_w * p->tile_h * p->num_comps, result, qt); if (rc) return rc;
    const int64_t bpt = grk_amd_tile_num_blocks(p);
    if (bpt < 0) return (int)bpt;
    std::vector<grk_amd_coded_block> plain((size_t)bpt * ntiles);
    rc = rate_prepare(c, p, ntiles, pixels, on_device, &qt.rate, plain.data()); if (rc) return rc;
    uint64_t plain_blocks = 0;
    for (const grk_amd_coded_block& r : plain) plain_blocks += r.length;
    RateQualityResult r{};
    rc = quality_choose(c, qt.goal.budget, plain_blocks, r); if (rc) return rc;
    rc = ht_encode_drops(c, ntiles, c->p1.p, c->last_h16, (const uint8_t*)c->rate_drop.p); if (rc) return rc;
    fill_quality_result(qt.goal, r, 0);
    if (table || total) { rc = grk_amd_fetch_table(c, table, total); if (rc) return rc; }
    note_reversible(c, *p, r.block_bytes < plain_blocks);
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

} // extern "C"

namespace {

// The rounds of every whole-image call. Headers and packet headers depend on the allocation: the blocks' budget is the target less
// what the file of the round before spent beside its blocks (first: the plain file), and a file that still overshoots lowers the
// budget by its overshoot.  `rows` hold the plain encode's rows on entry; round(budget, sum): KR2 and the final launches -- `rows` and
// `coded` as the file's writer takes them; file(out, cap): the file of `rows` and `coded`, or with out == nullptr its length.
int64_t rate_rounds(grk_amd_ctx* ctx, const grk_amd_tile_params& base, uint64_t target, const std::vector<grk_amd_coded_block>& rows,
                    std::vector<uint8_t>& coded, const std::function<int(uint64_t budget, RateAllocResult& sum)>& round,
                    const std::function<int64_t(uint8_t* out, uint64_t cap)>& file, uint8_t* out, uint64_t cap, grk_amd_rate_result* result)
{
    uint64_t plain_blocks = 0;
    for (const grk_amd_coded_block& r : rows) plain_blocks += r.length;
    const int64_t plain = file(nullptr, 0);
    if (plain < 0) return plain;
    uint64_t overhead = (uint64_t)plain - plain_blocks;
    uint64_t budget = target >= (uint64_t)plain ? plain_blocks : target > overhead ? target - overhead : 0;
    for (uint32_t pass = 1; pass <= kRateMaxRounds; ++pass) {
        RateAllocResult sum{};
        const int rc = round(budget, sum); if (rc) return rc;
        const int64_t len = file(nullptr, 0);
        if (len < 0) return len;
        if ((uint64_t)len <= target) {
            coded.push_back(0);                     // (the writer wants a buffer even when every block was skipped)
            const int64_t wrote = file(out, cap);
            if (wrote >= 0) { fill_result(result, sum, (uint64_t)wrote, pass); note_reversible(ctx, base, sum.block_bytes < plain_blocks); }
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

} // namespace

// ---- joint tables --------------------------------------------------------------------------------------------------------------
int grk_amd::rate_refusal(grk_amd_ctx* ctx, const grk_amd_rate* rate)
{
    if (ctx->pipelining) return fail(ctx, GRK_AMD_ERR_UNSUPPORTED, "rate-targeted encodes are not pipelined (grk_amd_set_pipelining(ctx, 0))");
    if (!plan_rate(rate->max_drop, rate->allow_skip != 0, 0).ok) return fail(ctx, GRK_AMD_ERR_INVALID, "grk_amd_rate::max_drop above 12");
    return GRK_AMD_OK;
}

int grk_amd::quality_target(grk_amd_ctx* ctx, const grk_amd_quality* quality, uint32_t prec, uint64_t samples, grk_amd_quality_result* result,
                            QualityTarget& out)
{
    ctx->rate.valid = false;          // (a refused call leaves no tables behind, as a refused rate-targeted call leaves none)
    if (ctx->pipelining) return fail(ctx, GRK_AMD_ERR_UNSUPPORTED, "quality-targeted encodes are not pipelined (grk_amd_set_pipelining(ctx, 0))");
    if (!plan_rate(quality->max_drop, quality->allow_skip != 0, 0).ok) return fail(ctx, GRK_AMD_ERR_INVALID, "grk_amd_quality::max_drop above 12");
    const QualityPlan qp = plan_quality(quality->target_psnr, quality->target_distortion, prec, samples);
    if (!qp.ok) return fail(ctx, GRK_AMD_ERR_INVALID, "grk_amd_quality: a target that is negative or not a number");
    out.rate = grk_amd_rate{};
    out.rate.max_drop = quality->max_drop; out.rate.allow_skip = quality->allow_skip; out.rate.joint = 1;
    out.goal = QualityGoal{qp.budget, qp.signal, result};
    return GRK_AMD_OK;
}

namespace {

// A joint call's tables and the coding of its batches -- what a byte goal's rounds and a distortion goal's one pass share
struct JointRun {
    grk_amd_ctx* c;
    const RateJointCall& call;
    RateJointPlan jp;
    std::vector<size_t> map_at;
    std::vector<grk_amd_coded_block> rows, table;       // the file's rows in joint order (first: the plain encode's); a batch's
    std::vector<uint8_t> coded;
    size_t resident = 0;                                // the batch whose planes and geometry the context holds

    const unsigned long long* map_of(size_t k) const { return (const unsigned long long*)c->rate_map.p + map_at[k]; }
    void keep_rows(size_t k, size_t at)
    {
        const uint64_t bpu = jp.per_unit[k];
        for (size_t i = 0; i < jp.map[k].size(); ++i)
            for (uint64_t b = 0; b < bpu; ++b) { rows[jp.map[k][i] + b] = table[i * bpu + b]; rows[jp.map[k][i] + b].offset += at; }
    }

    // the tables L, E, W over all units, made once: batch by batch the plain rows, the weights, KR1 and the trial launches through
    // the batch's map
    int tables()
    {
        c->rate.valid = false;
        { const int rc = rate_refusal(c, call.rate); if (rc) return rc; }
        const size_t nbatches = call.batches.size();
        std::vector<std::vector<uint32_t>> members;
        for (const RateBatch& b : call.batches) members.push_back(b.units);
        jp = plan_rate_joint(call.rate->max_drop, call.rate->allow_skip != 0, call.unit_blocks, members);
        if (!jp.ok) return fail(c, GRK_AMD_ERR_UNSUPPORTED, "rate tables: more blocks than the allocator indexes");
        const RatePlan& rp = jp.tables;
        const uint64_t N = jp.n;
        // the batches' maps one behind the other on the device, the largest batch's drop bytes, the tables
        std::vector<unsigned long long> maps;
        map_at.resize(nbatches);
        uint64_t largest = 0;
        for (size_t k = 0; k < nbatches; ++k) {
            map_at[k] = maps.size();
            maps.insert(maps.end(), jp.map[k].begin(), jp.map[k].end());
            largest = std::max<uint64_t>(largest, (uint64_t)jp.per_unit[k] * jp.map[k].size());
        }
        HIP_TRY(c, hipSetDevice(c->device), "set device");
        HIP_TRY(c, hipStreamSynchronize(c->stream), "sync");          // (the buffers below may still be read by an earlier call)
        HIP_TRY(c, c->rate_L.ensure(rp.l_bytes), "alloc rate lengths");
        HIP_TRY(c, c->rate_E.ensure(rp.e_bytes), "alloc rate errors");
        HIP_TRY(c, c->rate_W.ensure(rp.w_bytes), "alloc rate weights");
        HIP_TRY(c, c->rate_drop.ensure(rp.drop_bytes), "alloc drops");
        HIP_TRY(c, c->rate_res.ensure(sizeof(RateAllocResult)), "alloc rate result");
        HIP_TRY(c, c->rate_map.ensure(maps.size() * 8), "alloc rate maps");
        HIP_TRY(c, c->rate_bdrop.ensure(largest), "alloc a batch's drops");
        HIP_TRY(c, hipMemcpy(c->rate_map.p, maps.data(), maps.size() * 8, hipMemcpyHostToDevice), "upload rate maps");
        HIP_TRY(c, hipMemsetAsync(c->rate_L.p, 0, rp.l_bytes, c->stream), "clear rate lengths");          // (the SKIP row stays 0)
        rows.resize(N);
        std::vector<double> w(N);
        resident = nbatches;
        for (size_t k = 0; k < nbatches; ++k) {
            const uint32_t bpu = jp.per_unit[k], nunits = (uint32_t)jp.map[k].size();
            const uint64_t n = (uint64_t)bpu * nunits;
            table.resize(n);
            uint64_t total = 0;
            // (synchronous, with the arena / range flags checked: the trial launches below code from the planes this leaves)
            int rc = call.front(k, table.data(), &total); if (rc) return rc;
            resident = k;
            const TileGeom& g = c->geom;
            if (c->last_nblocks != n) return fail(c, GRK_AMD_ERR_INVALID, "rate tables: a batch's blocks are not its units'");
            keep_rows(k, 0);
            // W_b = (w_mct * w_band * stepsize)^2 / 4 of the unit's own geometry: E counts half steps
            for (uint32_t i = 0; i < bpu; ++i) {
                const double v = block_weight(g, i);
                for (uint64_t at : jp.map[k]) w[at + i] = v * v * 0.25;
            }
            rc = batch_tables(c, rp, nunits, map_of(k), N, c->rate_bdrop.p); if (rc) return rc;
        }
        HIP_TRY(c, hipMemcpyAsync(c->rate_W.p, w.data(), N * 8, hipMemcpyHostToDevice, c->stream), "upload rate weights");
        HIP_TRY(c, hipStreamSynchronize(c->stream), "sync");
        c->rate.valid = true; c->rate.plan = rp; c->rate.nblocks = N; c->rate.ntiles = 0; c->rate.unit_rows = jp.first_row;
        return GRK_AMD_OK;
    }

    // every batch -- its front end again where another batch has taken the context since -- coded with its slice of the chosen
    // drops: `rows` and `coded` as the file's writer takes them
    int code()
    {
        coded.clear();
        for (size_t k = 0; k < call.batches.size(); ++k) {
            const uint32_t bpu = jp.per_unit[k], nunits = (uint32_t)jp.map[k].size();
            const uint64_t n = (uint64_t)bpu * nunits;
            uint64_t total = 0;
            int rc;
            if (resident != k) { rc = call.front(k, nullptr, &total); if (rc) return rc; resident = k; }
            const RateMapArgs ma{c->rate_bdrop.p, c->rate_drop.p, map_of(k), bpu, n, 1u, 1};
            HIP_TRY(c, launch_rate_map(ma, c->stream), "gather the batch's drops");
            rc = ht_encode_drops(c, nunits, c->p1.p, c->last_h16, (const uint8_t*)c->rate_bdrop.p); if (rc) return rc;
            table.resize(n);
            rc = grk_amd_fetch_table(c, table.data(), &total); if (rc) return rc;
            const size_t at = coded.size();
            coded.resize(at + total);
            if (total) { rc = grk_amd_fetch_coded(c, coded.data() + at, total); if (rc) return rc; }
            keep_rows(k, at);
        }
        return GRK_AMD_OK;
    }
};

} // namespace

int64_t grk_amd::encode_rate_joint(grk_amd_ctx* c, const RateJointCall& call, uint8_t* out, uint64_t cap, grk_amd_rate_result* result)
{
    JointRun run{c, call};
    { const int rc = run.tables(); if (rc) return rc; }
    if (call.quality) {
        // a distortion budget: KQ once, the batches coded, the file written once
        uint64_t plain_blocks = 0;
        for (const grk_amd_coded_block& r : run.rows) plain_blocks += r.length;
        RateQualityResult r{};
        int rc = quality_choose(c, call.quality->budget, plain_blocks, r); if (rc) return rc;
        rc = run.code(); if (rc) return rc;
        run.coded.push_back(0);                     // (the writer wants a buffer even when every block was skipped)
        const int64_t wrote = call.write(run.rows.data(), run.coded.data(), out, cap);
        if (wrote >= 0) { fill_quality_result(*call.quality, r, (uint64_t)wrote); note_reversible(c, *call.base, r.block_bytes < plain_blocks); }
        return wrote;
    }
    // ---- a round: KR2 over the joint tables, then every batch coded with its slice of the drops
    auto round = [&](uint64_t budget, RateAllocResult& sum) -> int {
        const int rc = rate_choose(c, budget, sum); if (rc) return rc;
        return run.code();
    };
    return rate_rounds(c, *call.base, call.rate->target_bytes, run.rows, run.coded, round,
                       [&](uint8_t* o, uint64_t ocap) { return call.write(run.rows.data(), run.coded.data(), o, ocap); }, out, cap, result);
}

extern "C" {

uint64_t grk_amd_rate_num_blocks(grk_amd_ctx* c) { return c && c->rate.valid ? c->rate.nblocks : 0; }
uint64_t grk_amd_rate_last_budget(grk_amd_ctx* c) { return c && c->rate.valid ? c->rate.budget : 0; }
double grk_amd_quality_last_budget(grk_amd_ctx* c) { return c && c->rate.valid ? c->rate.qbudget : 0.0; }

int grk_amd_rate_unit_rows(grk_amd_ctx* c, uint64_t* first_row, uint32_t cap)
{
    if (!c || !c->rate.valid) return GRK_AMD_ERR_INVALID;
    for (size_t u = 0; u < c->rate.unit_rows.size() && u < cap && first_row; ++u) first_row[u] = c->rate.unit_rows[u];
    return (int)c->rate.unit_rows.size();
}

// KR1 on planes of the caller's choosing (the stage call of the statistics, as grk_amd_stage_ht_encode_drops is the drop instances'):
// over the context's block descriptors for *p, into a buffer of the stage's own -- through a map where the caller gives first rows,
// with the caller's E uploaded first.  Everything is checked on the host before anything is launched.
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

// KR2 on tables of the caller's choosing: one launch over buffers of the stage's own (the context's rate state is not touched)
int grk_amd_stage_rate_alloc(grk_amd_ctx* c, const uint32_t* L, const uint64_t* E, const double* W, uint64_t n, uint32_t max_drop, int allow_skip,
                             uint64_t budget, uint8_t* drops, grk_amd_rate_alloc_result* result)
{
    static_assert(sizeof(grk_amd_rate_alloc_result) == sizeof(RateAllocResult) && offsetof(grk_amd_rate_alloc_result, steps) == offsetof(RateAllocResult, steps),
                  "grk_amd_rate_alloc_result is RateAllocResult");
    if (!c) return GRK_AMD_ERR_INVALID;
    if (!L || !E || !W || !drops || !result) return fail(c, GRK_AMD_ERR_INVALID, "grk_amd_stage_rate_alloc: a null pointer");
    if (max_drop == 0 || max_drop > kRateMaxDrop) return fail(c, GRK_AMD_ERR_INVALID, "grk_amd_stage_rate_alloc: max_drop is 1 .. 12");
    if (!n || n > kRateMaxBlocks) return fail(c, GRK_AMD_ERR_INVALID, "grk_amd_stage_rate_alloc: no block, or more than the allocator indexes");
    const uint64_t rows = max_drop + 2u;
    for (uint64_t i = 0; i < rows * n; ++i)
        if (L[i] >> 31) return fail(c, GRK_AMD_ERR_INVALID, "grk_amd_stage_rate_alloc: a length of 2^31 bytes or more");
    HIP_TRY(c, hipSetDevice(c->device), "set device");
    HIP_TRY(c, c->st_rL.ensure(rows * n * 4u), "alloc the stage's lengths");
    HIP_TRY(c, c->st_rE.ensure(rows * n * 8u), "alloc the stage's errors");
    HIP_TRY(c, c->st_rW.ensure(n * 8u), "alloc the stage's weights");
    HIP_TRY(c, c->st_rdrop.ensure(n), "alloc the stage's drops");
    HIP_TRY(c, c->st_rres.ensure(sizeof(RateAllocResult)), "alloc the stage's result");
    HIP_TRY(c, hipMemcpyAsync(c->st_rL.p, L, rows * n * 4u, hipMemcpyHostToDevice, c->stream), "upload lengths");
    HIP_TRY(c, hipMemcpyAsync(c->st_rE.p, E, rows * n * 8u, hipMemcpyHostToDevice, c->stream), "upload errors");
    HIP_TRY(c, hipMemcpyAsync(c->st_rW.p, W, n * 8u, hipMemcpyHostToDevice, c->stream), "upload weights");
    HIP_TRY(c, hipMemsetAsync(c->st_rres.p, 0, sizeof(RateAllocResult), c->stream), "clear the result");
    RateAllocArgs a{};
    a.L = (const uint32_t*)c->st_rL.p; a.E = (const unsigned long long*)c->st_rE.p; a.W = (const double*)c->st_rW.p;
    a.nblocks = n; a.dmax = max_drop; a.ncand = max_drop + 1u + (allow_skip ? 1u : 0u); a.budget = budget;
    a.drop = (uint8_t*)c->st_rdrop.p; a.res = (RateAllocResult*)c->st_rres.p;
    HIP_TRY(c, launch_rate_alloc(a, c->stream), "launch rate allocator");
    HIP_TRY(c, hipMemcpyAsync(result, c->st_rres.p, sizeof(RateAllocResult), hipMemcpyDeviceToHost, c->stream), "fetch rate result");
    HIP_TRY(c, hipMemcpyAsync(drops, c->st_rdrop.p, n, hipMemcpyDeviceToHost, c->stream), "fetch drops");
    HIP_TRY(c, hipStreamSynchronize(c->stream), "sync");
    return GRK_AMD_OK;
}

// grk_amd_encode_image_rate, and -- quality != nullptr: always over joint tables -- grk_amd_encode_image_quality
static int64_t image_rate(grk_amd_ctx* ctx, const grk_amd_image_layout* im, const grk_amd_tile_params* base, const void* pixels, uint32_t flags,
                          const grk_amd_rate* rate, const QualityGoal* quality, uint8_t* out, uint64_t cap, grk_amd_rate_result* result)
{
    if (ctx->pipelining) return fail(ctx, GRK_AMD_ERR_UNSUPPORTED, "rate-targeted encodes are not pipelined (grk_amd_set_pipelining(ctx, 0))");
    flags |= GRK_AMD_CS_BLOCK_MSBS;
    std::vector<Unit> tiles;
    SourcePlanes src;
    UnitGroups g;
    const grk_amd_pixel_layout whole = ctx->enc_layout;
    // (grouped without the progression order, by geometry alone: the file is the host writer's, tile by tile, and the split route's
    //  budgets go by group)
    int64_t rc = plain_image(im, base, pixels, flags & ~(7u << GRK_AMD_CS_PROG_SHIFT), tiles, src, g, &whole);
    if (rc) return rc;
    KeepLayout staged{ctx->enc_layout, whole};
    ctx->enc_layout = staged_layout(src);
    const size_t ngroups = g.members.size();
    std::vector<uint8_t> staging;
    // a group's tiles staged and coded plainly
    auto stage_group = [&](size_t k) {
        const auto& G = g.members[k];
        staging.resize(staged_bytes(src, tiles[G[0]]) * G.size());
        stage_units(src, tiles, G, staging.data(), 1);
    };
    if (rate->joint || quality) {
        RateJointCall call{base, rate, {}, {}, {}, {}, quality};
        for (size_t u = 0; u < tiles.size(); ++u) call.unit_blocks.push_back((uint64_t)g.geoms[g.of[u]].blocks_per_comp * tiles[u].p.num_comps);
        for (size_t k = 0; k < ngroups; ++k) call.batches.push_back(RateBatch{tiles[g.members[k][0]].p, g.members[k]});
        call.front = [&](size_t k, grk_amd_coded_block* table, uint64_t* total) -> int {
            stage_group(k);
            return grk_amd_encode_tiles(ctx, &call.batches[k].p, (uint32_t)g.members[k].size(), staging.data(), 0, table, total);
        };
        call.write = [&](const grk_amd_coded_block* rows, const uint8_t* coded, uint8_t* o, uint64_t ocap) -> int64_t {
            if (!o) return sized_file(im, base, flags, rows);
            return grk_amd_write_codestream_layout(im, base, rows, coded, flags, o, ocap);
        };
        return encode_rate_joint(ctx, call, out, cap, result);
    }
    // the split route: every group alone on its own tables, its share of the budget by sample count
    std::vector<uint64_t> row_at(tiles.size() + 1, 0), samples(ngroups, 0), plain_of(ngroups, 0);
    for (size_t u = 0; u < tiles.size(); ++u) {
        row_at[u + 1] = row_at[u] + (uint64_t)g.geoms[g.of[u]].blocks_per_comp * tiles[u].p.num_comps;
        samples[g.of[u]] += (uint64_t)tiles[u].p.tile_w * tiles[u].p.tile_h * tiles[u].p.num_comps;
    }
    std::vector<grk_amd_coded_block> rows(row_at.back());
    std::vector<uint8_t> coded;
    // ... its tables made (one group: once for all rounds)
    auto prepare = [&](size_t k, bool keep_plain) -> int {
        const auto& G = g.members[k];
        const grk_amd_tile_params& p = tiles[G[0]].p;
        stage_group(k);
        const uint64_t bpu = (uint64_t)g.geoms[k].blocks_per_comp * p.num_comps;
        std::vector<grk_amd_coded_block> table(keep_plain ? bpu * G.size() : 0);
        const int pr = rate_prepare(ctx, &p, (uint32_t)G.size(), staging.data(), 0, rate, keep_plain ? table.data() : nullptr);
        if (pr) return pr;
        for (size_t i = 0; keep_plain && i < G.size(); ++i)
            for (uint64_t b = 0; b < bpu; ++b) rows[row_at[G[i]] + b] = table[i * bpu + b];
        return GRK_AMD_OK;
    };
    for (size_t k = 0; k < ngroups; ++k) { rc = prepare(k, true); if (rc) return rc; }
    for (size_t u = 0; u < tiles.size(); ++u)
        for (uint64_t b = row_at[u]; b < row_at[u + 1]; ++b) plain_of[g.of[u]] += rows[b].length;
    auto round = [&](uint64_t budget, RateAllocResult& sum) -> int {
        coded.clear();
        const std::vector<uint64_t> share = group_shares(budget, samples, plain_of);
        for (size_t k = 0; k < ngroups; ++k) {
            int rr;
            if (ngroups > 1) { rr = prepare(k, false); if (rr) return rr; }
            RateAllocResult r{};
            rr = rate_allocate(ctx, share[k], r); if (rr) return rr;
            sum.block_bytes += r.block_bytes; sum.lagrange_bytes += r.lagrange_bytes; sum.distortion += r.distortion; sum.lambda = r.lambda;
            const auto& G = g.members[k];
            const uint64_t bpu = (uint64_t)g.geoms[k].blocks_per_comp * tiles[G[0]].p.num_comps;
            std::vector<grk_amd_coded_block> table(bpu * G.size());
            uint64_t total = 0;
            rr = grk_amd_fetch_table(ctx, table.data(), &total); if (rr) return rr;
            const size_t at = coded.size();
            coded.resize(at + total);
            if (total) { rr = grk_amd_fetch_coded(ctx, coded.data() + at, total); if (rr) return rr; }
            for (size_t i = 0; i < G.size(); ++i)
                for (uint64_t b = 0; b < bpu; ++b) { rows[row_at[G[i]] + b] = table[i * bpu + b]; rows[row_at[G[i]] + b].offset += at; }
        }
        return GRK_AMD_OK;
    };
    return rate_rounds(ctx, *base, rate->target_bytes, rows, coded, round, [&](uint8_t* o, uint64_t ocap) -> int64_t {
        if (!o) return sized_file(im, base, flags, rows.data());
        return grk_amd_write_codestream_layout(im, base, rows.data(), coded.data(), flags, o, ocap);
    }, out, cap, result);
}

// KQ on tables of the caller's choosing: grk_amd_stage_rate_alloc's rules and buffers
int grk_amd_stage_quality_alloc(grk_amd_ctx* c, const uint32_t* L, const uint64_t* E, const double* W, uint64_t n, uint32_t max_drop, int allow_skip,
                                double D, uint8_t* drops, grk_amd_quality_alloc_result* result)
{
    static_assert(sizeof(grk_amd_quality_alloc_result) == sizeof(RateQualityResult) && offsetof(grk_amd_quality_alloc_result, steps) == offsetof(RateQualityResult, steps) &&
                  offsetof(grk_amd_quality_alloc_result, floor) == offsetof(RateQualityResult, floor), "grk_amd_quality_alloc_result is RateQualityResult");
    if (!c) return GRK_AMD_ERR_INVALID;
    if (!L || !E || !W || !drops || !result) return fail(c, GRK_AMD_ERR_INVALID, "grk_amd_stage_quality_alloc: a null pointer");
    if (max_drop == 0 || max_drop > kRateMaxDrop) return fail(c, GRK_AMD_ERR_INVALID, "grk_amd_stage_quality_alloc: max_drop is 1 .. 12");
    if (!n || n > kRateMaxBlocks) return fail(c, GRK_AMD_ERR_INVALID, "grk_amd_stage_quality_alloc: no block, or more than the allocator indexes");
    if (!(D >= 0.0)) return fail(c, GRK_AMD_ERR_INVALID, "grk_amd_stage_quality_alloc: a distortion budget that is negative or not a number");
    const uint64_t rows = max_drop + 2u;
    for (uint64_t i = 0; i < rows * n; ++i)
        if (L[i] >> 31) return fail(c, GRK_AMD_ERR_INVALID, "grk_amd_stage_quality_alloc: a length of 2^31 bytes or more");
    HIP_TRY(c, hipSetDevice(c->device), "set device");
    HIP_TRY(c, c->st_rL.ensure(rows * n * 4u), "alloc the stage's lengths");
    HIP_TRY(c, c->st_rE.ensure(rows * n * 8u), "alloc the stage's errors");
    HIP_TRY(c, c->st_rW.ensure(n * 8u), "alloc the stage's weights");
    HIP_TRY(c, c->st_rdrop.ensure(n), "alloc the stage's drops");
    HIP_TRY(c, c->st_rres.ensure(sizeof(RateQualityResult)), "alloc the stage's result");
    HIP_TRY(c, hipMemcpyAsync(c->st_rL.p, L, rows * n * 4u, hipMemcpyHostToDevice, c->stream), "upload lengths");
    HIP_TRY(c, hipMemcpyAsync(c->st_rE.p, E, rows * n * 8u, hipMemcpyHostToDevice, c->stream), "upload errors");
    HIP_TRY(c, hipMemcpyAsync(c->st_rW.p, W, n * 8u, hipMemcpyHostToDevice, c->stream), "upload weights");
    HIP_TRY(c, hipMemsetAsync(c->st_rres.p, 0, sizeof(RateQualityResult), c->stream), "clear the result");
    RateQualityArgs a{};
    a.L = (const uint32_t*)c->st_rL.p; a.E = (const unsigned long long*)c->st_rE.p; a.W = (const double*)c->st_rW.p;
    a.nblocks = n; a.dmax = max_drop; a.ncand = max_drop + 1u + (allow_skip ? 1u : 0u); a.budget = D;
    a.drop = (uint8_t*)c->st_rdrop.p; a.res = (RateQualityResult*)c->st_rres.p;
    HIP_TRY(c, launch_rate_quality(a, c->stream), "launch quality allocator");
    HIP_TRY(c, hipMemcpyAsync(result, c->st_rres.p, sizeof(RateQualityResult), hipMemcpyDeviceToHost, c->stream), "fetch quality result");
    HIP_TRY(c, hipMemcpyAsync(drops, c->st_rdrop.p, n, hipMemcpyDeviceToHost, c->stream), "fetch drops");
    HIP_TRY(c, hipStreamSynchronize(c->stream), "sync");
    return GRK_AMD_OK;
}

int64_t grk_amd_encode_image_rate(grk_amd_ctx* ctx, const grk_amd_image_layout* im, const grk_amd_tile_params* base, const void* pixels,
                                  uint32_t flags, const grk_amd_rate* rate, uint8_t* out, uint64_t cap, grk_amd_rate_result* result)
{
    if (!ctx || !im || !base || !pixels || !out || !rate) return GRK_AMD_ERR_INVALID;
    return image_rate(ctx, im, base, pixels, flags, rate, nullptr, out, cap, result);
}

int64_t grk_amd_encode_image_quality(grk_amd_ctx* ctx, const grk_amd_image_layout* im, const grk_amd_tile_params* base, const void* pixels,
                                     uint32_t flags, const grk_amd_quality* quality, uint8_t* out, uint64_t cap, grk_amd_quality_result* result)
{
    if (!ctx || !im || !base || !pixels || !out || !quality) return GRK_AMD_ERR_INVALID;
    QualityTarget qt;
    const int rc = quality_target(ctx, quality, base->prec, quality_samples(*im, base->num_comps, nullptr, nullptr), result, qt);
    if (rc) return rc;
    return image_rate(ctx, im, base, pixels, flags, &qt.rate, &qt.goal, out, cap, nullptr);
}

// grk_amd_encode_image_subsampled_rate and, with quality != nullptr, grk_amd_encode_image_subsampled_quality
static int64_t subsampled_rate(grk_amd_ctx* ctx, const grk_amd_image_layout* im, const grk_amd_tile_params* base, const uint8_t* comp_dx,
                               const uint8_t* comp_dy, const void* pixels, uint32_t flags, const grk_amd_rate* rate, const QualityGoal* quality,
                               uint8_t* out, uint64_t cap, grk_amd_rate_result* result)
{
    { const int rr = rate_refusal(ctx, rate); if (rr) return rr; }
    flags |= GRK_AMD_CS_BLOCK_MSBS;
    std::vector<Unit> units;
    SourcePlanes src;
    UnitGroups g;
    const int rc = subsampled_image(ctx, im, base, comp_dx, comp_dy, pixels, units, src, g);
    if (rc) return rc;
    std::vector<uint8_t> staging;
    RateJointCall call{base, rate, {}, {}, {}, {}, quality};
    for (size_t u = 0; u < units.size(); ++u) call.unit_blocks.push_back((uint64_t)g.geoms[g.of[u]].blocks_per_comp * units[u].p.num_comps);
    for (size_t k = 0; k < g.members.size(); ++k) call.batches.push_back(RateBatch{units[g.members[k][0]].p, g.members[k]});
    call.front = [&](size_t k, grk_amd_coded_block* table, uint64_t* total) -> int {
        const auto& G = g.members[k];
        staging.resize(staged_bytes(src, units[G[0]]) * G.size());
        stage_units(src, units, G, staging.data(), 1);
        return grk_amd_encode_tiles(ctx, &call.batches[k].p, (uint32_t)G.size(), staging.data(), 0, table, total);
    };
    call.write = [&](const grk_amd_coded_block* rows, const uint8_t* coded, uint8_t* o, uint64_t ocap) -> int64_t {
        return grk_amd_write_codestream_subsampled(im, base, comp_dx, comp_dy, rows, coded, flags, o, ocap);
    };
    return encode_rate_joint(ctx, call, out, cap, result);
}

int64_t grk_amd_encode_image_subsampled_rate(grk_amd_ctx* ctx, const grk_amd_image_layout* im, const grk_amd_tile_params* base,
                                             const uint8_t* comp_dx, const uint8_t* comp_dy, const void* pixels, uint32_t flags,
                                             const grk_amd_rate* rate, uint8_t* out, uint64_t cap, grk_amd_rate_result* result)
{
    if (!ctx || !im || !base || !pixels || !out || !comp_dx || !comp_dy || !rate) return GRK_AMD_ERR_INVALID;
    return subsampled_rate(ctx, im, base, comp_dx, comp_dy, pixels, flags, rate, nullptr, out, cap, result);
}

int64_t grk_amd_encode_image_subsampled_quality(grk_amd_ctx* ctx, const grk_amd_image_layout* im, const grk_amd_tile_params* base,
                                                const uint8_t* comp_dx, const uint8_t* comp_dy, const void* pixels, uint32_t flags,
                                                const grk_amd_quality* quality, uint8_t* out, uint64_t cap, grk_amd_quality_result* result)
{
    if (!ctx || !im || !base || !pixels || !out || !comp_dx || !comp_dy || !quality) return GRK_AMD_ERR_INVALID;
    QualityTarget qt;
    const int rc = quality_target(ctx, quality, base->prec, quality_samples(*im, base->num_comps, comp_dx, comp_dy), result, qt);
    if (rc) return rc;
    return subsampled_rate(ctx, im, base, comp_dx, comp_dy, pixels, flags, &qt.rate, &qt.goal, out, cap, nullptr);
}

} // extern "C"
