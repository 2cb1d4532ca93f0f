// grok_amd/csrc/encode_plan.cpp -- the host's planning for an encode call (encode_plan.h): block classes, LDS buffers, arena,
// class schedule, route, DWT level shapes.
#include "encode_plan.h"
#include <algorithm>

namespace grk_amd {

// ---- K3 block classes ------------------------------------------------------------------------------------------------------------
HtClasses plan_ht_classes(const TileGeom& g, uint32_t ncomp, bool lds_cap)
{
    HtClasses out;
    const uint32_t bpc = (uint32_t)g.blocks_comp0.size();
    auto add_class = [&](HtRole role, int top, int big) {      // top: 1 top resolution, 0 the rest, -1 every block;  big: -1 any, 0 / 1 by LDS need
        HtClassPlan cl{0, 0, 0, 0, 0, (uint32_t)out.sel.size(), role};
        uint32_t hist[64] = {0};
        for (uint32_t i = 0; i < ncomp * bpc; ++i) {
            const grk_amd_block& b = g.blocks_comp0[i % bpc];
            if (top >= 0 && (int)(b.res == g.p.num_levels && g.p.num_levels >= 1) != top) continue;
            const uint32_t w = b.x1 - b.x0, h = b.y1 - b.y0;
            const uint32_t samples = w * h, quads = ((w + 1u) / 2u) * ((h + 1u) / 2u);
            if (big >= 0 && (int)(ht_lds_bytes(samples, quads, b.kmax) > kLdsFor16Waves) != big) continue;
            cl.count++;
            cl.max_kmax = std::max<uint32_t>(cl.max_kmax, b.kmax);
            cl.max_samples = std::max(cl.max_samples, samples);
            cl.max_quads = std::max(cl.max_quads, quads);
            hist[b.kmax & 63u] += samples;
            out.sel.push_back(i);
        }
        for (uint32_t k = 0; k < 64; ++k) if (hist[k] > hist[cl.cap_kmax]) cl.cap_kmax = k;     // where most of the samples are
        if (cl.count) out.classes.push_back(cl);
    };
    if (lds_cap) { add_class(HtRole::Top, 1, -1); add_class(HtRole::Rest, 0, -1); add_class(HtRole::All, -1, -1); }
    else { add_class(HtRole::TopSmall, 1, 0); add_class(HtRole::TopBig, 1, 1); add_class(HtRole::RestSmall, 0, 0); add_class(HtRole::RestBig, 0, 1); }
    return out;
}

// ---- the LDS buffers of a class ---------------------------------------------------------------------------------------------------
HtLdsPlan ht_lds_layout(uint32_t samples, uint32_t quads, uint32_t kmax, bool capped, bool irrev)
{
    HtLdsPlan L{};
    const uint32_t per_sample = !capped ? kmax + 2u : irrev ? std::min(kmax + 2u, 8u) : std::min(kmax + 2u, kmax <= 11u ? 8u : kmax - 3u);
    const uint32_t ms_bits = samples * per_sample;
    const uint32_t vlc_bits = quads * (capped ? 10u : 15u) + 4u;
    L.ms_cap_bits = ms_bits;
    L.vlc_cap_bits = vlc_bits;
    L.ms_words = ((ms_bits + 31u) / 32u + 4u + 3u) & ~3u;           // slack: or_bits64 / window reads touch two words beyond;
    L.vlc_words = ((vlc_bits + 31u) / 32u + 4u + 3u) & ~3u;         // multiples of 4 words: cleared as uint4
    // behind the raw streams: the UVLC table (64 x 8 bytes) while phase A runs, then the staged VLC bytes (phase B1: the stuffed
    // bytes of the stream's capacity) in the same place; then 256 MEL bytes.  (A raw stream's windows read up to 65 words past its
    // end: the two areas are at least 192 words.)
    L.stage_bytes = std::max<uint32_t>(((vlc_bits / 7u + 16u) + 15u) & ~15u, 512u);
    L.bytes = (size_t)(L.ms_words + L.vlc_words) * 4u + L.stage_bytes + 256u;
    return L;
}

size_t ht_waves_per_cu(size_t lds_bytes) { return std::min(kMaxWavesPerCu, kLdsPerCu / std::max<size_t>(lds_bytes, 1)); }

HtClassLds plan_ht_lds(uint32_t max_samples, uint32_t max_quads, uint32_t max_kmax, uint32_t cap_kmax, bool irrev, bool have_fallback)
{
    HtClassLds r;
    r.full = ht_lds_layout(max_samples, max_quads, max_kmax, false, false);
    r.cap = ht_lds_layout(max_samples, max_quads, cap_kmax, true, irrev);
    r.use_cap = have_fallback && ht_waves_per_cu(r.cap.bytes) > ht_waves_per_cu(r.full.bytes);
    return r;
}

// ---- the instances that take a per-block drop, and a rate-targeted call's tables ----------------------------------------------------
HtDropPlan plan_ht_drop_instance(bool irreversible, bool h16)
{
    if (irreversible && h16) return HtDropPlan{false, {false, false}};
    return HtDropPlan{true, {irreversible, h16}};
}

RatePlan plan_rate(uint32_t max_drop, bool allow_skip, uint64_t nblocks)
{
    RatePlan r{};
    r.ok = max_drop <= kRateMaxDrop;
    if (!r.ok) return r;
    r.dmax = max_drop ? max_drop : kRateDefaultDrop;
    r.rows = r.dmax + 2u;
    r.ncand = r.dmax + 1u + (allow_skip ? 1u : 0u);
    r.trials = r.dmax + 1u;
    r.l_bytes = (uint64_t)r.rows * nblocks * 4u;
    r.e_bytes = (uint64_t)r.rows * nblocks * 8u;
    r.w_bytes = nblocks * 8u;
    r.drop_bytes = nblocks;
    return r;
}

RateJointPlan plan_rate_joint(uint32_t max_drop, bool allow_skip, const std::vector<uint64_t>& unit_blocks,
                              const std::vector<std::vector<uint32_t>>& batches)
{
    const RateJointPlan refused{};
    if (max_drop > kRateMaxDrop || unit_blocks.empty() || batches.empty()) return refused;
    RateJointPlan r{};
    r.first_row.resize(unit_blocks.size());
    for (size_t u = 0; u < unit_blocks.size(); ++u) {
        if (!unit_blocks[u] || unit_blocks[u] > kRateMaxBlocks) return refused;
        r.first_row[u] = r.n;
        r.n += unit_blocks[u];
        if (r.n > kRateMaxBlocks) return refused;
    }
    std::vector<bool> taken(unit_blocks.size(), false);
    size_t members = 0;
    for (const std::vector<uint32_t>& b : batches) {
        if (b.empty()) return refused;
        std::vector<uint64_t> m;
        for (uint32_t u : b) {
            if (u >= unit_blocks.size() || taken[u] || unit_blocks[u] != unit_blocks[b[0]]) return refused;
            taken[u] = true;
            m.push_back(r.first_row[u]);
        }
        members += b.size();
        r.map.push_back(m);
        r.per_unit.push_back((uint32_t)unit_blocks[b[0]]);
    }
    if (members != unit_blocks.size()) return refused;
    r.tables = plan_rate(max_drop, allow_skip, r.n);
    r.ok = r.tables.ok;
    return r;
}

uint64_t rate_first_budget(uint64_t target, uint64_t plain_file_bytes, uint64_t plain_block_bytes)
{
    const uint64_t overhead = plain_file_bytes - plain_block_bytes;
    return target >= plain_file_bytes ? plain_block_bytes : target > overhead ? target - overhead : 0;
}

RateNextBudget rate_next_budget(uint64_t budget, uint64_t block_bytes, uint64_t file_bytes, uint64_t target)
{
    if (budget == 0 || block_bytes == 0) return RateNextBudget{false, 0};
    const uint64_t over = file_bytes - target;
    budget = std::min(budget, block_bytes);
    return RateNextBudget{true, budget > over ? budget - over : 0};
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
        // (the remainder of up to one byte per other open group can lift the last one above its plain bytes: it takes those, the
        //  others share the rest anew)
        if (share[last] > plain[last]) { share[last] = plain[last]; full[last] = true; continue; }
        break;
    }
    return share;
}

QualityPlan plan_quality(double target_psnr, double target_distortion, uint32_t prec, uint64_t samples)
{
    const QualityPlan refused{};
    if (!(target_psnr >= 0.0) || prec == 0 || prec > 16 || !samples) return refused;
    QualityPlan r{};
    const double peak = (double)((1u << prec) - 1u);
    r.signal = (double)samples * peak * peak;
    if (target_psnr > 0.0) r.budget = std::isinf(target_psnr) ? 0.0 : r.signal * std::pow(10.0, -target_psnr / 10.0);
    else if (target_distortion >= 0.0) r.budget = target_distortion;
    else return refused;
    r.ok = true;
    return r;
}

uint64_t quality_samples(const grk_amd_image_layout& im, uint32_t num_comps, const uint8_t* comp_dx, const uint8_t* comp_dy)
{
    if (im.x1 <= im.x0 || im.y1 <= im.y0) return 0;
    uint64_t s = 0;
    for (uint32_t c = 0; c < num_comps; ++c) {
        const uint64_t dx = comp_dx ? comp_dx[c] : 1u, dy = comp_dy ? comp_dy[c] : 1u;
        if (!dx || !dy) return 0;
        s += ((im.x1 + dx - 1) / dx - (im.x0 + dx - 1) / dx) * ((im.y1 + dy - 1) / dy - (im.y0 + dy - 1) / dy);
    }
    return s;
}

// ---- the arena and its allocator ---------------------------------------------------------------------------------------------------
HtArenaPlan plan_ht_arena(uint64_t nblocks, uint64_t raw_bytes, uint32_t ntiles, const std::vector<HtClassPlan>& classes)
{
    HtArenaPlan a{};
    a.regions = 1;
    while (a.regions < kHtAllocRegions && nblocks / (a.regions * 2) >= kHtBlocksPerRegion) a.regions *= 2;
    // (a chunk holds at least two of the largest blocks the geometry can produce: worst case (Kmax + 2) bits per sample and 15 VLC
    //  bits per quad, stuffing 1 bit in 15, 256 MEL bytes -- ~20 KiB for a 64 x 64 block at Kmax 31)
    uint32_t ovf_base = 0;
    for (size_t k = 0; k < classes.size() && k < kHtMaxClasses; ++k) {
        const HtClassPlan& hc = classes[k];
        a.worst_block = std::max(a.worst_block, ((size_t)hc.max_samples * (hc.max_kmax + 2u) + (size_t)hc.max_quads * 15u) * 16u / 15u / 8u + 280u);
        a.ovf_base[k] = ovf_base;
        ovf_base += hc.count * ntiles;
    }
    a.chunk = (nblocks < kHtSmallJobBlocks && 2 * a.worst_block <= kHtAllocChunkSmall) ? kHtAllocChunkSmall : kHtAllocChunk;
    // arena: worst case of the HT cleanup pass is ~ (kmax+1)/8 * 8/7 bytes per sample + VLC/MEL;
    // twice the raw input size plus per-block slack covers every lossless case we accept
    a.arena_bytes = raw_bytes * 2 + nblocks * 64 + (uint64_t)(a.regions + 1) * kHtAllocChunk + (1u << 20);
    a.ovf_entries = 2 * nblocks;
    return a;
}

// ---- which class goes to which stream, and when ------------------------------------------------------------------------------------
HtStream ht_class_stream(HtRole role, bool overlapped, bool pipelined, HtPoint at, bool one_level, uint32_t parity)
{
    const bool swap = overlapped && pipelined && (parity & 1u);
    for (const HtScheduleRow& r : kHtSchedule) {
        if (r.role != role || r.overlapped != overlapped || (r.pipelined >= 0 && (r.pipelined != 0) != pipelined)) continue;
        if (r.at == at || (one_level && at == HtPoint::AfterLevel0 && r.at == HtPoint::AfterLastLevel))
            return !swap ? r.to : r.to == HtStream::Side ? HtStream::Side2 : r.to == HtStream::Side2 ? HtStream::Side : r.to;
    }
    return HtStream::NotHere;
}

// ---- the call's route ----------------------------------------------------------------------------------------------------------------
bool planes16_ok(const grk_amd_tile_params& p)
{
    if (p.irreversible || p.prec > 8 || p.num_levels == 0) return false;
    double bound = (double)(1u << p.prec) * 4.0;
    for (uint32_t l = 1; l < p.num_levels; ++l) bound *= 2.25;
    return bound + 8.0 * p.num_levels < 32767.0;
}

bool pk16_level_ok(const grk_amd_tile_params& p, uint32_t l)
{
    if (p.sgnd) return false;                        // (the packed unpacking is written for unsigned pixels)
    double m = (double)(1u << p.prec);
    for (uint32_t i = 0; i < l; ++i) m = m * 2.25 + 4.0;
    return 8.0 * m + 16.0 < 32767.0;
}

Route plan_route(const grk_amd_tile_params& p, const RouteIn& in)
{
    Route r;
    r.fused = p.num_levels >= 1 && in.px_align == 0;
    r.overlap = in.overlap && p.num_levels >= 1 && in.have_side;
    r.frame_stream = r.overlap && in.pipelining && in.have_side2 && in.on_device && r.fused &&
                     (in.frame_streams == 2 || (in.frame_streams == 1 && in.samples <= kFrameStreamSamples));
    r.h16 = in.planes16 && r.fused && planes16_ok(p);
    return r;
}

// ---- the shape of a forward DWT level --------------------------------------------------------------------------------------------
// the instance of a part of nc components (1, or 3: the MCT triple) of a level of shape s
static DwtInstance dwt_instance(const DwtLevelDesc& d, const DwtLevelShape& s, uint8_t nc)
{
    DwtInstance in{};
    const uint8_t px = d.px_bytes == 1 ? 1 : 2;
    const bool h16 = d.h16 && !d.irreversible;
    if (!d.fused) {
        in.packed = s.packed;
        in.pk = DwtPkKey{1, 0, (uint16_t)s.lanes, 0};
        in.k = DwtKey{d.irreversible, 1, 0, h16, true, false};
    } else if (d.px_lay != 0) {        // a layout of the caller's: the interleaved packed instances, else the strided front end
        in.packed = !d.irreversible && px == 1 && s.packed;
        const uint8_t ch = d.px_chan == 1 ? 1 : d.px_chan == 3 ? 3 : 4;
        in.pk = DwtPkKey{ch == 1 ? (uint8_t)1 : nc, 1, (uint16_t)s.lanes, ch};
        in.k = DwtKey{d.irreversible, nc, px, h16 && px == 1, true, true};
    } else {
        in.packed = !d.irreversible && px == 1 && s.packed;
        in.pk = DwtPkKey{nc, 1, (uint16_t)s.lanes, 0};
        // 16-bit planes exist for 8-bit pixels only (planes16_ok), and only in the general form
        if (h16 && px == 1) in.k = DwtKey{false, nc, 1, true, true, false};
        else                in.k = DwtKey{d.irreversible, nc, px, false, !s.all_fast, false};
    }
    return in;
}

DwtLevelShape plan_dwt_level(const DwtLevelDesc& d)
{
    DwtLevelShape s{};
    // (row offsets are 32-bit byte offsets from a plane's first sample: planes of 2^31 samples and more keep the flat addressing)
    const bool near = (uint64_t)d.m_stride * d.ch < (1ull << 31) && (uint64_t)d.cw * d.ch < (1ull << 31) && (uint64_t)d.in_stride * d.ch < (1ull << 31);
    // the caller's pixels: planes of the default layout, or interleaved with 1, 3 or 4 samples per pixel (rows at their real pitch);
    // planar pitches and two-channel pixels go through dwt_level_kernel's strided front end
    const bool lay = d.px_lay == 0 || (d.px_lay == 2 && (d.px_chan == 1 || d.px_chan == 3 || d.px_chan == 4) && d.px_row * d.ch < (1ull << 31));
    s.packed = d.h16 && d.pk && !d.irreversible && (d.px | d.py) == 0 && (d.cw & 3u) == 0 && d.cw >= 256u &&
               d.ch >= 16 && (d.ch & 1u) == 0 && near && lay;
    s.lanes = s.packed && d.cw <= kPkNarrowCols ? 128u : 256u;
    s.strip_cols = s.packed ? pk_strip_cols(d.cw, s.lanes) : kDwtStripCols;
    s.all_fast = (d.px | d.py) == 0 && (d.cw & 1u) == 0 && d.cw >= 4 && d.ch >= 16 && (d.ch & 1u) == 0;
    const uint32_t row_pairs = (d.ch + d.py + 1) >> 1;        // row pairs on the coordinate grid
    // (the packed kernel takes levels on the even grid only: d.px is 0 there)
    s.grid_x = (uint32_t)(((uint64_t)d.cw + d.px + s.strip_cols - 1) / s.strip_cols);
    s.seg_pairs = row_segment_pairs(s.grid_x, row_pairs, d.zslots, d.pk ? kDwtMinWgsPacked : kDwtMinWgs);
    s.grid_y = (row_pairs + s.seg_pairs - 1) / s.seg_pairs;
    s.inst[0] = dwt_instance(d, s, 1);
    if (d.fused) s.inst[1] = dwt_instance(d, s, 3);
    return s;
}

// ---- two forward DWT levels in one launch -------------------------------------------------------------------------------------------
DwtPairShape plan_dwt_pair(const DwtPairDesc& d)
{
    DwtPairShape s{};
    const DwtLevelDesc& u = d.upper;
    const DwtLevelShape up = plan_dwt_level(u), low = plan_dwt_level(d.lower);
    const bool levels = up.packed && low.packed && up.inst[1].packed && low.inst[0].packed;
    const bool pixels = u.fused && u.px_lay == 0 && u.px_bytes == 1 && d.mct && d.ncomp == 3 && u.h16 && !u.irreversible;
    const bool shape = (u.cw & 7u) == 0 && u.cw >= 512 && (u.ch & 3u) == 0 && u.ch >= 32 && (u.px | u.py | d.lower.px | d.lower.py) == 0 &&
                       d.lower.cw == u.cw >> 1 && d.lower.ch == u.ch >> 1;
    const bool near = (uint64_t)u.m_stride * u.ch * 2u < (1ull << 31);       // bytes of a Mallat plane of int16
    if (!(levels && pixels && shape && near && d.ntiles > 0)) return s;
    s.ok = true;
    s.lanes = up.lanes;
    s.strip_cols = up.strip_cols;                                            // (leaves two halo lanes a side: kernels_dwt.hip)
    s.grid_x = up.grid_x;
    s.seg_pairs = std::min(kDwtPairMaxSeg, row_segment_pairs(s.grid_x, u.ch >> 1, d.ntiles, kDwtPairMinWgs));
    s.grid_y = ((u.ch >> 1) + s.seg_pairs - 1) / s.seg_pairs;
    s.inst = DwtPairKey{3, 1, (uint16_t)s.lanes};
    return s;
}

DwtPairShape plan_dwt_pair_at(const TileGeom& g, uint32_t l, const DwtPairAsk& q)
{
    if (!q.pair || !q.fused || l != 0 || l + 1 >= g.p.num_levels) return DwtPairShape{};     // (the instances there are read pixels)
    const ResGeom& g0 = level_geom(g, l);
    const ResGeom& g1 = level_geom(g, l + 1);
    const bool irrev = g.p.irreversible != 0;
    const uint32_t zslots = q.ntiles * level_part_zslots(g.p.mct != 0, g.p.num_comps);
    const DwtLevelDesc upper{g0.w, g0.h, g0.x0 & 1u, g0.y0 & 1u, g.stride, g.stride, q.h16, q.h16 && q.dwt_pk && pk16_level_ok(g.p, l), irrev,
                             q.px_lay, q.px_chan, q.px_row, zslots, true, q.px_bytes};
    const DwtLevelDesc lower{g1.w, g1.h, g1.x0 & 1u, g1.y0 & 1u, q.mid_stride, g.stride, q.h16, q.h16 && q.dwt_pk && pk16_level_ok(g.p, l + 1), irrev,
                             0, 0, 0, q.ntiles * g.p.num_comps, false, q.px_bytes};
    return plan_dwt_pair(DwtPairDesc{upper, lower, g.p.mct != 0, g.p.num_comps, q.ntiles});
}

} // namespace grk_amd
