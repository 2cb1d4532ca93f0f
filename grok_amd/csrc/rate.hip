// grok_amd/csrc/rate.hip -- rate- and quality-targeted HT encodes: a batch of tiles in at most N bytes of code-blocks, a whole image
// in a file of at most N bytes, either in the fewest bytes for a distortion.
//
// Every call takes ONE path to its tables and its coded blocks, a run (RateRun) over units (a tile; a run of a tile's components of
// one size) in batches, each one grk_amd_encode_tiles call over units of one geometry.  Per batch the front end and a plain K3 run;
// then, on the planes that left, KR1 (kernels_rate.hip) gives every candidate's error per block and Dmax + 1 trial launches of the
// block coder's drop instances (kernels_ht.hip DROP; uniform d = 0 .. Dmax, the arena rewound in between, only the length column
// kept) every candidate's exact length -- into ONE set of tables over all the run's blocks in the order the file's writer takes them
// (plan_rate_joint, encode_plan.h: the row order, the batches' maps, the bounds).  The allocator -- KR2 for bytes, KQ for a
// distortion (plan_quality) -- runs over all of them, one multiplier for every block of every component, and each batch is coded
// with its slice of the chosen drops.  No per-block data comes to the host before a final table does.
// A whole-image call for bytes goes in rounds (rate_rounds), one for a distortion writes its file once.  The tile calls and each
// geometry group of grk_amd_encode_image_rate's split route are identity runs: one batch in row order, no maps.
// The stage calls of the statistics and the allocators are in rate_stage.hip.
#include "context.h"
#include "image.h"
#include <numeric>

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

// ---- the run: tables, and the coding of the batches with the chosen drops ------------------------------------------------------------
// unit_blocks, batches and front are a RateJointCall's (image.h); `rows` and `coded` are the file's, as its writer takes them -- the
// run's own, or on the split route one file's that every group's run fills its part of.
struct RateRun {
    grk_amd_ctx* c;
    const grk_amd_rate* rate;
    std::vector<uint64_t> unit_blocks;
    std::vector<RateBatch> batches;
    decltype(RateJointCall::front) front;
    std::vector<grk_amd_coded_block>& rows;
    std::vector<uint8_t>& coded;
    bool identity = false;                              // one batch, its units in row order: no maps, the chosen drops are the batch's
    const std::vector<uint64_t>* place = nullptr;       // where the units' rows go in `rows` (nullptr: the tables' own rows, `rows` sized to them)
    RateJointPlan jp{};
    std::vector<size_t> map_at{};
    std::vector<grk_amd_coded_block> table{};           // a batch's rows in batch order
    size_t resident = 0;                                // the batch whose planes and geometry the context holds

    const unsigned long long* map_of(size_t k) const { return identity ? nullptr : (const unsigned long long*)c->rate_map.p + map_at[k]; }
    void keep_rows(size_t k, size_t at)
    {
        const uint64_t bpu = jp.per_unit[k];
        const std::vector<uint64_t>& first = place ? *place : jp.map[k];
        for (size_t i = 0; i < first.size(); ++i)
            for (uint64_t b = 0; b < bpu; ++b) { rows[first[i] + b] = table[i * bpu + b]; rows[first[i] + b].offset += at; }
    }

    // the tables L, E, W over all units: batch by batch the plain encode (plain_rows: its rows kept in `rows`), the weights, KR1 and
    // the trial launches through the batch's map
    int tables(bool plain_rows)
    {
        c->rate.valid = false;
        { const int rc = rate_refusal(c, rate); if (rc) return rc; }
        const size_t nbatches = batches.size();
        std::vector<std::vector<uint32_t>> members;
        for (const RateBatch& b : batches) members.push_back(b.units);
        jp = plan_rate_joint(rate->max_drop, rate->allow_skip != 0, unit_blocks, members);
        if (!jp.ok) return fail(c, GRK_AMD_ERR_UNSUPPORTED, "rate tables: more blocks than the allocator indexes");
        const RatePlan& rp = jp.tables;
        const uint64_t N = jp.n;
        HIP_TRY(c, hipSetDevice(c->device), "set device");
        HIP_TRY(c, hipStreamSynchronize(c->stream), "sync");          // (the buffers below may still be read by an earlier call)
        HIP_TRY(c, c->rate_L.ensure(rp.l_bytes), "alloc rate lengths");
        HIP_TRY(c, c->rate_E.ensure(rp.e_bytes), "alloc rate errors");
        HIP_TRY(c, c->rate_W.ensure(rp.w_bytes), "alloc rate weights");
        HIP_TRY(c, c->rate_drop.ensure(rp.drop_bytes), "alloc drops");
        HIP_TRY(c, c->rate_res.ensure(sizeof(RateAllocResult)), "alloc rate result");
        if (!identity) {
            // the batches' maps one behind the other on the device, the largest batch's drop bytes
            std::vector<unsigned long long> maps;
            map_at.resize(nbatches);
            uint64_t largest = 0;
            for (size_t k = 0; k < nbatches; ++k) {
                map_at[k] = maps.size();
                maps.insert(maps.end(), jp.map[k].begin(), jp.map[k].end());
                largest = std::max<uint64_t>(largest, (uint64_t)jp.per_unit[k] * jp.map[k].size());
            }
            HIP_TRY(c, c->rate_map.ensure(maps.size() * 8), "alloc rate maps");
            HIP_TRY(c, c->rate_bdrop.ensure(largest), "alloc a batch's drops");
            HIP_TRY(c, hipMemcpy(c->rate_map.p, maps.data(), maps.size() * 8, hipMemcpyHostToDevice), "upload rate maps");
        }
        HIP_TRY(c, hipMemsetAsync(c->rate_L.p, 0, rp.l_bytes, c->stream), "clear rate lengths");          // (the SKIP row stays 0)
        if (!place) rows.resize(N);
        std::vector<double> w(N);
        resident = nbatches;
        for (size_t k = 0; k < nbatches; ++k) {
            const uint32_t bpu = jp.per_unit[k], nunits = (uint32_t)jp.map[k].size();
            const uint64_t n = (uint64_t)bpu * nunits;
            table.resize(n);
            uint64_t total = 0;
            // (synchronous, with the arena / range flags checked: the trial launches below code from the planes this leaves)
            int rc = front(k, plain_rows ? table.data() : nullptr, &total); if (rc) return rc;
            resident = k;
            const TileGeom& g = c->geom;
            if (c->last_nblocks != n) return fail(c, GRK_AMD_ERR_INVALID, "rate tables: a batch's blocks are not its units'");
            if (plain_rows) keep_rows(k, 0);
            // W_b = (w_mct * w_band * stepsize)^2 / 4 of the unit's own geometry: E counts half steps
            for (uint32_t i = 0; i < bpu; ++i) {
                const double v = block_weight(g, i);
                for (uint64_t at : jp.map[k]) w[at + i] = v * v * 0.25;
            }
            rc = batch_tables(c, rp, nunits, map_of(k), N, identity ? c->rate_drop.p : c->rate_bdrop.p); if (rc) return rc;
        }
        HIP_TRY(c, hipMemcpyAsync(c->rate_W.p, w.data(), N * 8, hipMemcpyHostToDevice, c->stream), "upload rate weights");
        HIP_TRY(c, hipStreamSynchronize(c->stream), "sync");
        c->rate.valid = true; c->rate.plan = rp; c->rate.nblocks = N; c->rate.unit_rows = jp.first_row;
        return GRK_AMD_OK;
    }

    // batch k -- its front end again where another batch has taken the context since -- coded with its slice of the chosen drops; the
    // table and the bytes stay on the device
    int code(size_t k)
    {
        const uint32_t nunits = (uint32_t)jp.map[k].size();
        uint64_t total = 0;
        if (resident != k) { const int rc = front(k, nullptr, &total); if (rc) return rc; resident = k; }
        if (!identity) {
            const RateMapArgs ma{c->rate_bdrop.p, c->rate_drop.p, map_of(k), jp.per_unit[k], (uint64_t)jp.per_unit[k] * nunits, 1u, 1};
            HIP_TRY(c, launch_rate_map(ma, c->stream), "gather the batch's drops");
        }
        return ht_encode_drops(c, nunits, c->p1.p, c->last_h16, (const uint8_t*)(identity ? c->rate_drop.p : c->rate_bdrop.p));
    }

    // ... and brought to the host: its rows into `rows`, its bytes behind those `coded` holds
    int merge(size_t k)
    {
        table.resize((uint64_t)jp.per_unit[k] * jp.map[k].size());
        uint64_t total = 0;
        int rc = grk_amd_fetch_table(c, table.data(), &total); if (rc) return rc;
        const size_t at = coded.size();
        coded.resize(at + total);
        if (total) { rc = grk_amd_fetch_coded(c, coded.data() + at, total); if (rc) return rc; }
        c->rate_dev_counters[1] += total;
        keep_rows(k, at);
        return GRK_AMD_OK;
    }

    // every batch coded and merged: `rows` and `coded` as the file's writer takes them
    int code_all()
    {
        coded.clear();
        for (size_t k = 0; k < batches.size(); ++k) {
            int rc = code(k); if (rc) return rc;
            rc = merge(k); if (rc) return rc;
        }
        return GRK_AMD_OK;
    }
};

// an identity run: `n` units of `bpu` blocks in row order, one batch of parameters p
RateRun identity_run(grk_amd_ctx* c, const grk_amd_rate* rate, const grk_amd_tile_params& p, size_t n, uint64_t bpu, decltype(RateJointCall::front) front,
                     std::vector<grk_amd_coded_block>& rows, std::vector<uint8_t>& coded, const std::vector<uint64_t>* place = nullptr)
{
    RateRun run{c, rate, std::vector<uint64_t>(n, bpu), {RateBatch{p, std::vector<uint32_t>(n)}}, std::move(front), rows, coded, true, place};
    std::iota(run.batches[0].units.begin(), run.batches[0].units.end(), 0u);
    return run;
}

uint64_t length_sum(const std::vector<grk_amd_coded_block>& rows)
{
    uint64_t sum = 0;
    for (const grk_amd_coded_block& r : rows) sum += r.length;
    return sum;
}

// ---- choose: the allocator over the run's tables, the chosen drop bytes in rate_drop.  KR2 for `budget` bytes of code-blocks
int rate_choose(grk_amd_ctx* c, uint64_t budget, RateAllocResult& res)
{
    if (!c->rate.valid) return GRK_AMD_ERR_INVALID;
    const RatePlan& rp = c->rate.plan;
    c->rate.budget = budget; c->rate.qbudget = 0;
    {
        ScopedTimer t(c, 9);
        const RateAllocArgs a = rate_alloc_args<RateAllocArgs>(c->rate_L, c->rate_E, c->rate_W, c->rate_drop, c->rate_res, c->rate.nblocks, rp.dmax, rp.ncand, budget);
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

// KQ for a distortion budget.  plain_blocks: the bytes of row 0 of L.
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
    c->rate.budget = 0; c->rate.qbudget = budget;
    {
        ScopedTimer t(c, 9);
        const RateQualityArgs a = rate_alloc_args<RateQualityArgs>(c->rate_L, c->rate_E, c->rate_W, c->rate_drop, c->rate_res, c->rate.nblocks, rp.dmax, rp.ncand, budget);
        HIP_TRY(c, launch_rate_quality(a, c->stream), "launch quality allocator");
    }
    HIP_TRY(c, hipMemcpyAsync(&res, c->rate_res.p, sizeof(res), hipMemcpyDeviceToHost, c->stream), "fetch quality result");
    HIP_TRY(c, hipStreamSynchronize(c->stream), "sync");
    // (E[0] = 0 everywhere in the tables of an encode: the floor is 0 and every D >= 0 feasible)
    if (!res.feasible) return fail(c, GRK_AMD_ERR_OVERFLOW, "the distortion budget is below what the finest candidates leave");
    return GRK_AMD_OK;
}

void fill_result(grk_amd_rate_result* out, const RateAllocResult& r, uint64_t file_bytes, uint32_t passes)
{
    if (!out) return;
    std::memset(out, 0, sizeof(*out));
    out->block_bytes = r.block_bytes; out->lagrange_bytes = r.lagrange_bytes; out->file_bytes = file_bytes;
    out->distortion = r.distortion; out->lambda = r.lambda; out->passes = passes;
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

// a successful call's note to grk_amd_last_error: what the decoders at hand make of a reversible file with planes dropped
void note_reversible(grk_amd_ctx* c, const grk_amd_tile_params& p, bool dropped)
{
    c->err = (!p.irreversible && dropped)
        ? "note: 5/3 blocks with d planes dropped are returned as mu >> d by Grok's and this library's reversible dequantiser (not the bin centre the reported distortion assumes); use the 9/7 transform for such decoders"
        : "";
}

// ---- the rounds of every whole-image call for bytes -----------------------------------------------------------------------------------
// Headers and packet headers depend on the allocation: the blocks' budget is the target less what the file of the round before spent
// beside its blocks (first: the plain file), and a file that still overshoots lowers the budget by its overshoot (rate_first_budget,
// rate_next_budget: encode_plan.h).  `rows` hold the plain encode's rows on entry; round(budget, sum): KR2 and the final launches --
// `rows` and `coded` as the file's writer takes them; file(out, cap): the file of `rows` and `coded`, or with out == nullptr its length.
int64_t rate_rounds(grk_amd_ctx* ctx, const grk_amd_tile_params& base, uint64_t target, const std::vector<grk_amd_coded_block>& rows,
                    std::vector<uint8_t>& coded, const std::function<int(uint64_t budget, RateAllocResult& sum)>& round,
                    const std::function<int64_t(uint8_t* out, uint64_t cap)>& file, uint8_t* out, uint64_t cap, grk_amd_rate_result* result)
{
    const uint64_t plain_blocks = length_sum(rows);
    const int64_t plain = file(nullptr, 0);
    if (plain < 0) return plain;
    uint64_t budget = rate_first_budget(target, (uint64_t)plain, plain_blocks);
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
        const RateNextBudget next = rate_next_budget(budget, sum.block_bytes, (uint64_t)len, target);
        if (!next.left)                                   // nothing left to take from the blocks: the headers alone are too long
            return fail(ctx, GRK_AMD_ERR_OVERFLOW, "the target is below what the file takes with no byte of any block in it");
        budget = next.budget;
    }
    return fail(ctx, GRK_AMD_ERR_OVERFLOW, "the file was still above the target after 4 allocate + write rounds (the target may be feasible: the rounds ran out)");
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

// the tile calls: an identity run over `ntiles` tiles of *p (plain != nullptr: the plain encode's rows kept there), choose(), the final
// launch -- coded and left on the device
int tiles_run(grk_amd_ctx* c, const grk_amd_tile_params* p, uint32_t ntiles, const void* pixels, int on_device, const grk_amd_rate* rate,
              std::vector<grk_amd_coded_block>* plain, const std::function<int()>& choose)
{
    const int64_t bpt = grk_amd_tile_num_blocks(p);
    if (bpt < 0) return fail(c, (int)bpt, "unsupported tile parameters");
    std::vector<grk_amd_coded_block> rows;
    std::vector<uint8_t> coded;
    RateRun run = identity_run(c, rate, *p, ntiles, (uint64_t)bpt, [&](size_t, grk_amd_coded_block* table, uint64_t* total) {
        return grk_amd_encode_tiles(c, p, ntiles, pixels, on_device, table, total);
    }, plain ? *plain : rows, coded);
    int rc = run.tables(plain != nullptr); if (rc) return rc;
    rc = choose(); if (rc) return rc;
    return run.code(0);
}

// grk_amd_encode_image_rate, and -- quality != nullptr: always over joint tables -- grk_amd_encode_image_quality
int64_t image_rate(grk_amd_ctx* ctx, const grk_amd_image_layout* im, const grk_amd_tile_params* base, const void* pixels, uint32_t flags,
                   const grk_amd_rate* rate, const QualityGoal* quality, uint8_t* out, uint64_t cap, grk_amd_rate_result* result)
{
    if (ctx->pipelining) return rate_refusal(ctx, rate);          // (max_drop is looked at behind plain_image's checks, by the run)
    // (a byte budget would have to count the extra frames)
    if (flags & GRK_AMD_CS_TP(3)) return fail(ctx, GRK_AMD_ERR_UNSUPPORTED, "GRK_AMD_CS_TP: tiles divided into tile-parts are not written by the rate- and quality-targeted calls");
    flags |= GRK_AMD_CS_BLOCK_MSBS;
    std::vector<Unit> tiles;
    SourcePlanes src;
    UnitGroups g;
    const grk_amd_pixel_layout whole = ctx->enc_layout;
    // (grouped without the progression order, by geometry alone: the file is the host writer's, tile by tile, and the split route's
    //  budgets go by group)
    const int rc = plain_image(im, base, pixels, flags & ~(7u << GRK_AMD_CS_PROG_SHIFT), tiles, src, g, &whole);
    if (rc) return rc;
    KeepLayout staged{ctx->enc_layout, whole};
    ctx->enc_layout = staged_layout(src);
    std::vector<uint8_t> staging;
    RateJointCall call{base, rate, {}, {}, {}, {}, quality};
    planar_rate_call(ctx, tiles, src, g, staging, call);
    call.write = [&](const grk_amd_coded_block* rows, const uint8_t* coded, uint8_t* o, uint64_t ocap) -> int64_t {
        if (!o) return sized_file(im, base, flags, rows);
        return grk_amd_write_codestream_layout(im, base, rows, coded, flags, o, ocap);
    };
    if (rate->joint || quality) return encode_rate_joint(ctx, call, out, cap, result);
    // the split route: every group an identity run over the file's shared rows and bytes, its share of the budget by sample count.
    // The context holds one set of tables: several groups make theirs anew in every round
    const size_t ngroups = g.members.size();
    std::vector<uint64_t> row_at(tiles.size() + 1, 0), samples(ngroups, 0), plain_of(ngroups, 0);
    for (size_t u = 0; u < tiles.size(); ++u) {
        row_at[u + 1] = row_at[u] + call.unit_blocks[u];
        samples[g.of[u]] += (uint64_t)tiles[u].p.tile_w * tiles[u].p.tile_h * tiles[u].p.num_comps;
    }
    std::vector<grk_amd_coded_block> rows(row_at.back());
    std::vector<uint8_t> coded;
    std::vector<std::vector<uint64_t>> place(ngroups);
    std::vector<RateRun> runs;
    for (size_t k = 0; k < ngroups; ++k) {
        const std::vector<uint32_t>& G = g.members[k];
        for (uint32_t u : G) place[k].push_back(row_at[u]);
        runs.push_back(identity_run(ctx, rate, call.batches[k].p, G.size(), call.unit_blocks[G[0]], [&call, k](size_t, grk_amd_coded_block* table, uint64_t* total) {
            return call.front(k, table, total);
        }, rows, coded, &place[k]));
        const int rr = runs[k].tables(true); if (rr) return rr;
    }
    for (size_t u = 0; u < tiles.size(); ++u)
        for (uint64_t b = row_at[u]; b < row_at[u + 1]; ++b) plain_of[g.of[u]] += rows[b].length;
    auto round = [&](uint64_t budget, RateAllocResult& sum) -> int {
        coded.clear();
        const std::vector<uint64_t> share = group_shares(budget, samples, plain_of);
        for (size_t k = 0; k < ngroups; ++k) {
            int rr;
            if (ngroups > 1) { rr = runs[k].tables(false); if (rr) return rr; }
            RateAllocResult r{};
            rr = rate_choose(ctx, share[k], r); if (rr) return rr;
            sum.block_bytes += r.block_bytes; sum.lagrange_bytes += r.lagrange_bytes; sum.distortion += r.distortion; sum.lambda = r.lambda;
            rr = runs[k].code(0); if (rr) return rr;
            rr = runs[k].merge(0); if (rr) return rr;
        }
        return GRK_AMD_OK;
    };
    return rate_rounds(ctx, *base, rate->target_bytes, rows, coded, round,
                       [&](uint8_t* o, uint64_t ocap) { return call.write(rows.data(), coded.data(), o, ocap); }, out, cap, result);
}

// grk_amd_encode_image_subsampled_rate and, with quality != nullptr, grk_amd_encode_image_subsampled_quality
int64_t subsampled_rate(grk_amd_ctx* ctx, const grk_amd_image_layout* im, const grk_amd_tile_params* base, const uint8_t* comp_dx,
                        const uint8_t* comp_dy, const void* pixels, uint32_t flags, const grk_amd_rate* rate, const QualityGoal* quality,
                        uint8_t* out, uint64_t cap, grk_amd_rate_result* result)
{
    { const int rr = rate_refusal(ctx, rate); if (rr) return rr; }
    if (flags & GRK_AMD_CS_TP(3)) return fail(ctx, GRK_AMD_ERR_UNSUPPORTED, "GRK_AMD_CS_TP: tiles divided into tile-parts are not written by the rate- and quality-targeted calls");
    flags |= GRK_AMD_CS_BLOCK_MSBS;
    std::vector<Unit> units;
    SourcePlanes src;
    UnitGroups g;
    const int rc = subsampled_image(ctx, im, base, comp_dx, comp_dy, pixels, units, src, g);
    if (rc) return rc;
    std::vector<uint8_t> staging;
    RateJointCall call{base, rate, {}, {}, {}, {}, quality};
    planar_rate_call(ctx, units, src, g, staging, call);
    call.write = [&](const grk_amd_coded_block* rows, const uint8_t* coded, uint8_t* o, uint64_t ocap) -> int64_t {
        return grk_amd_write_codestream_subsampled(im, base, comp_dx, comp_dy, rows, coded, flags, o, ocap);
    };
    return encode_rate_joint(ctx, call, out, cap, result);
}

} // namespace

int grk_amd::rate_refusal(grk_amd_ctx* ctx, const grk_amd_rate* rate, const char* goal)
{
    char msg[96];
    if (ctx->pipelining) {
        std::snprintf(msg, sizeof(msg), "%s-targeted encodes are not pipelined (grk_amd_set_pipelining(ctx, 0))", goal);
        return fail(ctx, GRK_AMD_ERR_UNSUPPORTED, msg);
    }
    if (!plan_rate(rate->max_drop, rate->allow_skip != 0, 0).ok) {
        std::snprintf(msg, sizeof(msg), "grk_amd_%s::max_drop above 12", goal);
        return fail(ctx, GRK_AMD_ERR_INVALID, msg);
    }
    return GRK_AMD_OK;
}

int grk_amd::quality_target(grk_amd_ctx* ctx, const grk_amd_quality* quality, uint32_t prec, uint64_t samples, grk_amd_quality_result* result,
                            QualityTarget& out)
{
    ctx->rate.valid = false;          // (a refused call leaves no tables behind, as a refused rate-targeted call leaves none)
    out.rate = grk_amd_rate{};
    out.rate.max_drop = quality->max_drop; out.rate.allow_skip = quality->allow_skip; out.rate.joint = 1;
    { const int rc = rate_refusal(ctx, &out.rate, "quality"); if (rc) return rc; }
    const QualityPlan qp = plan_quality(quality->target_psnr, quality->target_distortion, prec, samples);
    if (!qp.ok) return fail(ctx, GRK_AMD_ERR_INVALID, "grk_amd_quality: a target that is negative or not a number");
    out.goal = QualityGoal{qp.budget, qp.signal, result};
    return GRK_AMD_OK;
}

int64_t grk_amd::encode_rate_joint(grk_amd_ctx* c, const RateJointCall& call, uint8_t* out, uint64_t cap, grk_amd_rate_result* result)
{
    std::vector<grk_amd_coded_block> rows;
    std::vector<uint8_t> coded;
    RateRun run{c, call.rate, call.unit_blocks, call.batches, call.front, rows, coded};
    { const int rc = run.tables(true); if (rc) return rc; }
    const auto file = [&](uint8_t* o, uint64_t ocap) { return call.write(rows.data(), coded.data(), o, ocap); };
    if (call.quality) {
        // a distortion budget: KQ once, the batches coded, the file written once
        const uint64_t plain_blocks = length_sum(rows);
        RateQualityResult r{};
        int rc = quality_choose(c, call.quality->budget, plain_blocks, r); if (rc) return rc;
        rc = run.code_all(); if (rc) return rc;
        coded.push_back(0);                     // (the writer wants a buffer even when every block was skipped)
        const int64_t wrote = file(out, cap);
        if (wrote >= 0) { fill_quality_result(*call.quality, r, (uint64_t)wrote); note_reversible(c, *call.base, r.block_bytes < plain_blocks); }
        return wrote;
    }
    // a round: KR2 over the tables, then every batch coded with its slice of the drops
    return rate_rounds(c, *call.base, call.rate->target_bytes, rows, coded, [&](uint64_t budget, RateAllocResult& sum) -> int {
        const int rc = rate_choose(c, budget, sum); if (rc) return rc;
        return run.code_all();
    }, file, out, cap, result);
}

int64_t grk_amd::encode_rate_joint_device(grk_amd_ctx* c, const RateJointCall& call, const JointT2Call& t2, void** d_file, grk_amd_rate_result* result)
{
    c->rate_dev_counters[0] = c->rate_dev_counters[1] = 0;
    if (!d_file || t2.batches.size() != call.batches.size()) return GRK_AMD_ERR_INVALID;
    for (size_t k = 0; k < call.batches.size(); ++k) if (t2.batches[k] != call.batches[k].units) return GRK_AMD_ERR_INVALID;
    std::vector<grk_amd_coded_block> rows;
    std::vector<uint8_t> coded;                              // (stays empty: the bytes stay on the device)
    RateRun run{c, call.rate, call.unit_blocks, call.batches, call.front, rows, coded};
    // what the device writer does not reach is said before any batch is coded
    JointT2Run jr{c, &t2, true};
    { const int rc = joint_device_open(jr); if (rc) return rc; }
    { const int rc = run.tables(true); if (rc) return rc; }
    // a Tier-2 pass: every batch coded with its slice of the chosen drops and kept, the classes framed -> the file's length
    const auto pass = [&]() -> int64_t {
        int rc = joint_device_reset(jr); if (rc) return rc;
        for (size_t k = 0; k < call.batches.size(); ++k) {
            rc = run.code(k); if (rc) return rc;
            rc = joint_device_keep(jr, k); if (rc) return rc;
        }
        const int64_t n = joint_device_finish(jr, nullptr, 0, d_file);
        if (n >= 0) ++c->rate_dev_counters[0];
        return n;
    };
    const uint64_t plain_blocks = length_sum(rows);
    if (call.quality) {
        RateQualityResult r{};
        const int rc = quality_choose(c, call.quality->budget, plain_blocks, r); if (rc) return rc;
        const int64_t n = pass();
        if (n >= 0) { fill_quality_result(*call.quality, r, (uint64_t)n); note_reversible(c, *call.base, r.block_bytes < plain_blocks); }
        return n;
    }
    // the rounds of rate_rounds, the file's length the device's
    const uint64_t target = call.rate->target_bytes;
    const int64_t plain = call.write(rows.data(), nullptr, nullptr, 0);
    if (plain < 0) return plain;
    uint64_t budget = rate_first_budget(target, (uint64_t)plain, plain_blocks);
    for (uint32_t round = 1; round <= kRateMaxRounds; ++round) {
        RateAllocResult sum{};
        const int rc = rate_choose(c, budget, sum); if (rc) return rc;
        const int64_t len = pass();
        if (len < 0) return len;
        if ((uint64_t)len <= target) {
            fill_result(result, sum, (uint64_t)len, round);
            note_reversible(c, *call.base, sum.block_bytes < plain_blocks);
            return len;
        }
        const RateNextBudget next = rate_next_budget(budget, sum.block_bytes, (uint64_t)len, target);
        if (!next.left) return fail(c, GRK_AMD_ERR_OVERFLOW, "the target is below what the file takes with no byte of any block in it");
        budget = next.budget;
    }
    return fail(c, GRK_AMD_ERR_OVERFLOW, "the file was still above the target after 4 allocate + write rounds (the target may be feasible: the rounds ran out)");
}

extern "C" {

uint64_t grk_amd_rate_device_counters(grk_amd_ctx* c, int which)
{
    return c && which >= 0 && which < 2 ? c->rate_dev_counters[which] : 0;
}

int grk_amd_encode_tiles_rate(grk_amd_ctx* c, const grk_amd_tile_params* p, uint32_t ntiles, const void* pixels, int on_device,
                              const grk_amd_rate* rate, grk_amd_coded_block* table, uint64_t* total, grk_amd_rate_result* result)
{
    if (!c || !p || !pixels || !ntiles || !rate) return GRK_AMD_ERR_INVALID;
    c->rate.valid = false;
    int rc = rate_refusal(c, rate); if (rc) return rc;
    RateAllocResult r{};
    rc = tiles_run(c, p, ntiles, pixels, on_device, rate, nullptr, [&] { return rate_choose(c, rate->target_bytes, r); }); if (rc) return rc;
    fill_result(result, r, 0, 1);
    if (table || total) { rc = grk_amd_fetch_table(c, table, total); if (rc) return rc; }
    note_reversible(c, *p, r.lambda > 0.0);
    return GRK_AMD_OK;
}

int grk_amd_encode_tiles_quality(grk_amd_ctx* c, const grk_amd_tile_params* p, uint32_t ntiles, const void* pixels, int on_device,
                                 const grk_amd_quality* quality, grk_amd_coded_block* table, uint64_t* total, grk_amd_quality_result* result)
{
    if (!c || !p || !pixels || !ntiles || !quality) return GRK_AMD_ERR_INVALID;
    QualityTarget qt;
    int rc = quality_target(c, quality, p->prec, (uint64_t)ntiles * p->tile_w * p->tile_h * p->num_comps, result, qt); if (rc) return rc;
    std::vector<grk_amd_coded_block> plain;
    uint64_t plain_blocks = 0;
    RateQualityResult r{};
    rc = tiles_run(c, p, ntiles, pixels, on_device, &qt.rate, &plain, [&] {
        plain_blocks = length_sum(plain);
        return quality_choose(c, qt.goal.budget, plain_blocks, r);
    });
    if (rc) return rc;
    fill_quality_result(qt.goal, r, 0);
    if (table || total) { rc = grk_amd_fetch_table(c, table, total); if (rc) return rc; }
    note_reversible(c, *p, r.block_bytes < plain_blocks);
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

// ---- what the latest call left ----
uint64_t grk_amd_rate_num_blocks(grk_amd_ctx* c) { return c && c->rate.valid ? c->rate.nblocks : 0; }
uint64_t grk_amd_rate_last_budget(grk_amd_ctx* c) { return c && c->rate.valid ? c->rate.budget : 0; }
double grk_amd_quality_last_budget(grk_amd_ctx* c) { return c && c->rate.valid ? c->rate.qbudget : 0.0; }

int grk_amd_rate_unit_rows(grk_amd_ctx* c, uint64_t* first_row, uint32_t cap)
{
    if (!c || !c->rate.valid) return GRK_AMD_ERR_INVALID;
    for (size_t u = 0; u < c->rate.unit_rows.size() && u < cap && first_row; ++u) first_row[u] = c->rate.unit_rows[u];
    return (int)c->rate.unit_rows.size();
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
