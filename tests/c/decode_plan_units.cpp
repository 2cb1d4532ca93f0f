// tests/c/decode_plan_units.cpp -- the decode path's host planning (grok_amd/csrc/decode_plan.cpp) behind plain C entry points, for
// tests/test_decode_plan_cpu.py: built at test time with g++ together with decode_plan.cpp and geometry.cpp, no GPU, no HIP.
// Every planner's refusal text is kept for dp_reason().
#include "../../grok_amd/csrc/decode_plan.h"
#include <algorithm>
#include <cstring>

using namespace grk_amd;

namespace {
const char* g_why = "";
}

extern "C" {
const char* dp_reason(void) { return g_why; }

// kSkipBlock, kT1NoBlock, kT1LaneMaxPlanes, kT1LaneMinRows, kT1WorkBytes
void dp_constants(uint32_t* out)
{
    out[0] = kSkipBlock; out[1] = kT1NoBlock; out[2] = kT1LaneMaxPlanes; out[3] = kT1LaneMinRows; out[4] = kT1WorkBytes;
}

// heights: one uint16 per block of a tile; lane: 2 nblocks entries, tail: nblocks; out = {n_lane, n_tail, buckets}
int dp_t1_lists(const grk_amd_coded_block* table, uint64_t nblocks, const uint16_t* heights, uint32_t blocks_per_tile, uint32_t cblksty,
                int t1_lanes, int pass_sync, int have_segments, uint32_t* lane, uint32_t* tail, uint32_t* out)
{
    T1PlanIn in{};
    in.table = table; in.nblocks = nblocks;
    in.block_h = heights; in.blocks_per_tile = blocks_per_tile;
    in.cblksty = cblksty; in.t1_lanes = t1_lanes; in.pass_sync = pass_sync != 0; in.have_segments = have_segments != 0;
    T1Lists l;
    g_why = "";
    const int rc = plan_t1_lists(in, lane, tail, &l, &g_why);
    out[0] = l.n_lane; out[1] = l.n_tail; out[2] = l.buckets;
    return rc;
}

int dp_check_table(const grk_amd_coded_block* table, uint64_t nblocks, uint64_t coded_bytes)
{
    g_why = "";
    return check_table(table, nblocks, coded_bytes, &g_why);
}

// active: nblocks entries; out = {nactive, max_len}
int dp_ht_blocks(const grk_amd_coded_block* table, uint64_t nblocks, uint64_t coded_bytes, uint32_t* active, uint32_t* out)
{
    g_why = "";
    out[0] = out[1] = 0;
    return plan_ht_blocks(table, nblocks, coded_bytes, active, &out[0], &out[1], &g_why);
}

// the full segment list checked against nblocks (select_segments), then the refinement table: ref = nblocks x {bytes, passes}
int dp_ht_refinement(const grk_amd_coded_block* table, uint64_t nblocks, const uint32_t* first, uint64_t nfirst, const grk_amd_segment* segs,
                     uint64_t nsegs, grk_amd_segment* ref, uint32_t* max_refine_bytes)
{
    const std::vector<uint32_t> f(first, first + nfirst), none;
    const std::vector<grk_amd_segment> s(segs, segs + nsegs), none_s;
    SegList sl;
    g_why = "";
    int rc = select_segments(false, f, s, none, none_s, nblocks, &sl, &g_why);
    if (rc || !sl.nfirst) return rc;
    *max_refine_bytes = 0;
    return plan_ht_refinement(table, nblocks, sl, ref, max_refine_bytes, &g_why);
}

// out = {entries of red_first, entries of red_segs}; the reduced list is then selected for groups x kept rows (as a reduced call does)
int dp_reduce_segments(uint64_t groups, uint32_t full_per_comp, uint32_t kept_per_comp, const uint32_t* first, uint64_t nfirst,
                       const grk_amd_segment* segs, uint64_t nsegs, uint32_t* red_first, uint64_t first_cap, grk_amd_segment* red_segs,
                       uint64_t segs_cap, uint64_t* out)
{
    const std::vector<uint32_t> f(first, first + nfirst);
    const std::vector<grk_amd_segment> s(segs, segs + nsegs);
    std::vector<uint32_t> rf;
    std::vector<grk_amd_segment> rs;
    g_why = "";
    int rc = reduce_segments(groups, full_per_comp, kept_per_comp, f, s, rf, rs, &g_why);
    if (rc) return rc;
    SegList sl;
    rc = select_segments(true, f, s, rf, rs, groups * kept_per_comp, &sl, &g_why);
    if (rc) return rc;
    if (sl.nfirst != rf.size() || sl.nsegs != rs.size() || rf.size() > first_cap || rs.size() > segs_cap) return -100;
    std::copy(rf.begin(), rf.end(), red_first);
    std::copy(rs.begin(), rs.end(), red_segs);
    out[0] = rf.size(); out[1] = rs.size();
    return 0;
}

// The plan of window win = {x0, y0, x1, y1} of tile p and what it skips.
//   levels[l] (l = 0 .. L), 12 words: need[l] (4), the size of LL_l (2), and for l < L pairs[l] (4) and the pair grid's size (2)
//   rows: one tile's table rows ([comp][block]); the skipped ones come back as {0, 0, kSkipBlock}
//   res:  the resolution of each row's block
// returns the number of rows, or a negative GRK_AMD_* code
int64_t dp_region(const grk_amd_tile_params* p, const uint32_t* win, uint32_t* levels, grk_amd_coded_block* rows, uint8_t* res, uint64_t rows_cap)
{
    TileGeom g;
    const int rc = build_tile_geom(*p, g);
    if (rc) return rc;
    const uint32_t L = g.p.num_levels;
    const uint64_t nrows = (uint64_t)g.blocks_per_comp * g.p.num_comps;
    if (nrows > rows_cap) return -100;
    const RegionPlan plan = plan_region(g, Rect{win[0], win[1], win[2], win[3]});
    if (plan.need.size() != L + 1 || plan.pairs.size() != L) return -101;
    for (uint32_t l = 0; l <= L; ++l) {
        uint32_t* o = levels + 12 * l;
        const ResGeom& R = g.res[L - l];
        const Rect n = plan.need[l];
        o[0] = n.x0; o[1] = n.y0; o[2] = n.x1; o[3] = n.y1; o[4] = R.w; o[5] = R.h;
        if (l == L) continue;
        const Rect q = plan.pairs[l];
        o[6] = q.x0; o[7] = q.y0; o[8] = q.x1; o[9] = q.y1;
        o[10] = (R.w + (R.x0 & 1u) + 1) >> 1; o[11] = (R.h + (R.y0 & 1u) + 1) >> 1;
    }
    skip_blocks_outside(g, plan, rows);
    for (uint64_t i = 0; i < nrows; ++i) res[i] = g.blocks_comp0[i % g.blocks_per_comp].res;
    return (int64_t)nrows;
}

// kIdwtStripPairs, kIdwtHaloPairs, kIpkStripCols, kIdwtMinWgs, kIdwtRegionSegPairs
void dp_idwt_constants(uint32_t* out)
{
    out[0] = kIdwtStripPairs; out[1] = kIdwtHaloPairs; out[2] = kIpkStripCols; out[3] = kIdwtMinWgs; out[4] = kIdwtRegionSegPairs;
}
uint32_t dp_ipk_strip_cols(uint32_t cw) { return ipk_strip_cols(cw); }

// in = {cw, ch, px, py, ll_stride, m_stride, out_stride, h16, pk, irreversible, zslots, region, need x0, y0, x1, y1, fused, px_bytes, lo, hi,
//       mct, px_lay, px_chan, px_row, px_tile, px_align}
// out = {packed, strip_pairs, seg_pairs, grid_x, grid_y, strip0, nstrips, seg0, nsegs, wx0, wy0, wx1, wy1}, then for the part of one
//       component and for the MCT triple {packed, grid_x, 32-bit key: f97, nc, pxo, h16, str, packed key: nc, pxo, ch}
void dp_idwt_level(const int64_t* in, uint32_t* out)
{
    IdwtLevelDesc d{};
    d.cw = (uint32_t)in[0]; d.ch = (uint32_t)in[1]; d.px = (uint32_t)in[2]; d.py = (uint32_t)in[3];
    d.ll_stride = (uint32_t)in[4]; d.m_stride = (uint32_t)in[5]; d.out_stride = (uint32_t)in[6];
    d.h16 = in[7] != 0; d.pk = in[8] != 0; d.irreversible = in[9] != 0; d.zslots = (uint32_t)in[10];
    d.region = in[11] != 0; d.need = Rect{(uint32_t)in[12], (uint32_t)in[13], (uint32_t)in[14], (uint32_t)in[15]};
    d.fused = in[16] != 0; d.px_bytes = (uint32_t)in[17]; d.lo = (int32_t)in[18]; d.hi = (int32_t)in[19]; d.mct = in[20] != 0;
    d.px_lay = (uint32_t)in[21]; d.px_chan = (uint32_t)in[22]; d.px_row = (uint64_t)in[23]; d.px_tile = (uint64_t)in[24];
    d.px_align = (uint32_t)in[25];
    const IdwtLevelShape s = plan_idwt_level(d);
    const uint32_t head[13] = {s.packed, s.strip_pairs, s.seg_pairs, s.grid_x, s.grid_y, s.strip0, s.nstrips, s.seg0, s.nsegs, s.wx0, s.wy0, s.wx1, s.wy1};
    std::copy(head, head + 13, out);
    for (int i = 0; i < 2; ++i) {
        const IdwtInstance& n = s.inst[i];
        const uint32_t row[10] = {n.packed, n.grid_x, n.k.f97, n.k.nc, n.k.pxo, n.k.h16, n.k.str, n.pk.nc, n.pk.pxo, n.pk.ch};
        std::copy(row, row + 10, out + 13 + 10 * i);
    }
}
// out = {bytes, nc, str}
void dp_egress_key(uint32_t px_lay, uint32_t bytes_per_sample, uint32_t ncomp, uint32_t* out)
{
    const EgressKey k = egress_key(px_lay, bytes_per_sample, ncomp);
    out[0] = k.bytes; out[1] = k.nc; out[2] = k.str;
}
// the inverse kernels' instance lists (dwt_instances.h): rows of {f97, nc, pxo, h16, str} / {nc, pxo, ch} / {bytes, nc, str}; each returns
// the number of rows
uint32_t dp_idwt_instances(uint32_t* out)
{
    uint32_t n = 0;
    for (const IdwtKey& k : kIdwtInstances) { const uint32_t row[5] = {k.f97, k.nc, k.pxo, k.h16, k.str}; std::copy(row, row + 5, out + 5 * n++); }
    return n;
}
uint32_t dp_idwt_pk_instances(uint32_t* out)
{
    uint32_t n = 0;
    for (const IdwtPkKey& k : kIdwtPkInstances) { const uint32_t row[3] = {k.nc, k.pxo, k.ch}; std::copy(row, row + 3, out + 3 * n++); }
    return n;
}
uint32_t dp_egress_instances(uint32_t* out)
{
    uint32_t n = 0;
    for (const EgressKey& k : kEgressInstances) { const uint32_t row[3] = {k.bytes, k.nc, k.str}; std::copy(row, row + 3, out + 3 * n++); }
    return n;
}
} // extern "C"
