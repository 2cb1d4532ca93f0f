// tests/c/dwt_pair_plan_units.cpp -- the host planning of two forward DWT levels in one launch (grok_amd/csrc/encode_plan.cpp:
// plan_dwt_pair, plan_dwt_pair_at; encode_constants.h: dwt_pair_rows) behind plain C entry points, for tests/test_dwt_pair_plan_cpu.py:
// built at test time with g++ together with encode_plan.cpp and geometry.cpp, no GPU, no HIP.  With -DDWT_PAIR_MAIN it is a program
// of its own that walks the same cases (the test runs it under AddressSanitizer and UBSan).
#include "../../grok_amd/csrc/encode_plan.h"
#include <algorithm>
#include <cstdio>
#include <vector>

using namespace grk_amd;

namespace {
// the pair for levels l, l + 1 of tile p as an encode of `ntiles` tiles asks for it: every switch on, the fused route; h16 = the route
// keeps int16 planes (the setting and planes16_ok); interleaved = pixels of three interleaved channels instead of planes
DwtPairShape pair_of(const grk_amd_tile_params& p, uint32_t l, uint32_t ntiles, bool planes16, bool interleaved, bool pair_switch)
{
    TileGeom g;
    if (build_tile_geom(p, g)) return DwtPairShape{};
    const bool h16 = planes16 && planes16_ok(p);
    const uint32_t w1 = (p.tile_w + 1) >> 1;
    return plan_dwt_pair_at(g, l, DwtPairAsk{pair_switch, true, true, h16, interleaved ? 2u : 0u, interleaved ? 3u : 0u,
                                             interleaved ? (uint64_t)p.tile_w * 3u : 0u, (uint32_t)((p.prec + 7) / 8), (w1 + 31u) & ~31u, ntiles});
}
}

extern "C" {
// out = {ok, lanes, strip_cols, seg_pairs, grid_x, grid_y, key nc, key px, key nt}
void dp_plan(const grk_amd_tile_params* p, uint32_t l, uint32_t ntiles, int planes16, int interleaved, int pair_switch, uint32_t* out)
{
    const DwtPairShape s = pair_of(*p, l, ntiles, planes16 != 0, interleaved != 0, pair_switch != 0);
    const uint32_t row[9] = {s.ok, s.lanes, s.strip_cols, s.seg_pairs, s.grid_x, s.grid_y, s.inst.nc, s.inst.px, s.inst.nt};
    std::copy(row, row + 9, out);
}
// out = {store0, store1, first, last, low0, low1} of segment seg
void dp_rows(uint32_t seg, uint32_t seg_pairs, uint32_t ch, int32_t* out)
{
    const DwtPairRows r = dwt_pair_rows(seg, seg_pairs, ch);
    const int32_t row[6] = {r.store0, r.store1, r.first, r.last, r.low0, r.low1};
    std::copy(row, row + 6, out);
}
// rows of {nc, px, nt}; returns the number of rows
uint32_t dp_instances(uint32_t* out)
{
    uint32_t n = 0;
    for (const DwtPairKey& k : kDwtPairInstances) { const uint32_t row[3] = {k.nc, k.px, k.nt}; std::copy(row, row + 3, out + 3 * n++); }
    return n;
}
uint32_t dp_min_wgs() { return kDwtPairMinWgs; }
}

#ifdef DWT_PAIR_MAIN
namespace {
int failures = 0;
#define EXPECT(c) do { if (!(c)) { ++failures; std::printf("line %d: %s\n", __LINE__, #c); } } while (0)

grk_amd_tile_params params(uint32_t w, uint32_t h, uint16_t comps, uint8_t prec, uint8_t levels)
{
    grk_amd_tile_params p{};
    p.tile_w = w; p.tile_h = h; p.num_comps = comps; p.prec = prec; p.mct = comps >= 3; p.num_levels = levels;
    p.cblk_w_exp = p.cblk_h_exp = 6;
    return p;
}

// every segment's upper-level pairs cover what its lower-level pairs read, every pair of either level is stored exactly once
void check_segments(uint32_t w, uint32_t h)
{
    const DwtPairShape s = pair_of(params(w, h, 3, 8, 5), 0, 1, true, false, true);
    EXPECT(s.ok);
    if (!s.ok) return;
    const int32_t sh = (int32_t)(h >> 1), sh1 = (int32_t)(h >> 2);
    EXPECT(s.seg_pairs % 2 == 0 && s.grid_y == ((uint32_t)sh + s.seg_pairs - 1) / s.seg_pairs);
    std::vector<int> up(sh, 0), low(sh1, 0);
    for (uint32_t seg = 0; seg < s.grid_y; ++seg) {
        const DwtPairRows r = dwt_pair_rows(seg, s.seg_pairs, h);
        EXPECT(r.store0 % 2 == 0 && r.store1 % 2 == 0 && r.store0 < r.store1 && r.low0 < r.low1);
        for (int32_t j = r.store0; j < r.store1; ++j) { EXPECT(j >= 0 && j < sh); if (j >= 0 && j < sh) ++up[j]; }
        for (int32_t j = r.low0; j < r.low1; ++j) { EXPECT(j >= 0 && j < sh1); if (j >= 0 && j < sh1) ++low[j]; }
        // lower pair j reads LL rows 2j .. 2j + 2 and, through the high-pass term of pair j - 1, rows 2j - 2, 2j - 1
        EXPECT(r.first <= 2 * r.low0 - 2 && r.last >= 2 * r.low1 && r.first <= r.store0 && r.last >= r.store1 - 1);
        EXPECT(r.first >= -2 && r.last <= sh);                 // one reflection at the most
    }
    for (int v : up) EXPECT(v == 1);
    for (int v : low) EXPECT(v == 1);
}
}

int main()
{
    // the headline: 8192^2 x 3, 8 bits, five levels
    const DwtPairShape h = pair_of(params(8192, 8192, 3, 8, 5), 0, 1, true, false, true);
    EXPECT(h.ok && h.lanes == 256 && h.strip_cols == 960 && h.grid_x == 9 && h.grid_y * h.seg_pairs == 4096);
    EXPECT(h.inst.nc == 3 && h.inst.px == 1 && h.inst.nt == 256);
    EXPECT((uint64_t)h.grid_x * h.grid_y >= kDwtPairMinWgs || h.seg_pairs == 8);
    // refusals, one per condition
    EXPECT(!pair_of(params(516, 32, 3, 8, 5), 0, 1, true, false, true).ok);        // width no multiple of 8
    EXPECT(!pair_of(params(512, 34, 3, 8, 5), 0, 1, true, false, true).ok);        // height no multiple of 4
    EXPECT(!pair_of(params(504, 32, 3, 8, 5), 0, 1, true, false, true).ok);        // too narrow
    EXPECT(!pair_of(params(512, 28, 3, 8, 5), 0, 1, true, false, true).ok);        // too low
    EXPECT(!pair_of(params(512, 32, 3, 12, 5), 0, 1, true, false, true).ok);       // 12 bits
    { grk_amd_tile_params p = params(512, 32, 3, 8, 5); p.irreversible = 1; EXPECT(!pair_of(p, 0, 1, true, false, true).ok); }
    EXPECT(!pair_of(params(512, 32, 3, 8, 5), 0, 1, true, true, true).ok);         // interleaved
    { grk_amd_tile_params p = params(512, 32, 3, 8, 5); p.tile_x0 = 1; EXPECT(!pair_of(p, 0, 1, true, false, true).ok); }
    { grk_amd_tile_params p = params(512, 32, 3, 8, 5); p.tile_y0 = 2; EXPECT(!pair_of(p, 0, 1, true, false, true).ok); }   // (level 1 starts odd)
    EXPECT(!pair_of(params(512, 32, 3, 8, 1), 0, 1, true, false, true).ok);        // one level
    EXPECT(!pair_of(params(512, 32, 3, 8, 5), 0, 1, false, false, true).ok);       // int32 planes
    EXPECT(!pair_of(params(512, 32, 1, 8, 5), 0, 1, true, false, true).ok);        // mono
    EXPECT(!pair_of(params(512, 32, 4, 8, 5), 0, 1, true, false, true).ok);        // a fourth component
    { grk_amd_tile_params p = params(512, 32, 3, 8, 5); p.mct = 0; EXPECT(!pair_of(p, 0, 1, true, false, true).ok); }
    EXPECT(!pair_of(params(512, 32, 3, 8, 5), 0, 1, true, false, false).ok);       // the switch
    EXPECT(pair_of(params(512, 32, 3, 8, 5), 0, 1, true, false, true).ok && pair_of(params(512, 32, 3, 8, 2), 0, 8, true, false, true).ok);
    check_segments(512, 32); check_segments(512, 36); check_segments(1000, 48); check_segments(2056, 40); check_segments(8192, 8192);
    std::printf("dwt_pair_plan_units: %d failure(s)\n", failures);
    return failures ? 1 : 0;
}
#endif
