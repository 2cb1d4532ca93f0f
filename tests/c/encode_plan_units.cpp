// tests/c/encode_plan_units.cpp -- the encode path's host planning (grok_amd/csrc/encode_plan.cpp) behind plain C entry points, for
// tests/test_encode_plan_cpu.py: built at test time with g++ together with encode_plan.cpp and geometry.cpp, no GPU, no HIP.
#include "../../grok_amd/csrc/encode_plan.h"
#include <algorithm>
#include <cstring>

using namespace grk_amd;

extern "C" {
// kHtMaxClasses, kHtAllocRegions, kHtAllocChunk, kHtAllocChunkSmall, kHtAllocBytes, kLdsFor16Waves, kLdsPerCu, kMaxWavesPerCu,
// kFrameStreamSamples, kDwtMinWgsPacked, kDwtMinWgs, kPkLaneCols, kDwtStripCols, rows of kHtSchedule
void ep_constants(uint64_t* out)
{
    const uint64_t v[] = {kHtMaxClasses, kHtAllocRegions, kHtAllocChunk, kHtAllocChunkSmall, kHtAllocBytes, kLdsFor16Waves, kLdsPerCu,
                          kMaxWavesPerCu, kFrameStreamSamples, kDwtMinWgsPacked, kDwtMinWgs, (uint64_t)kPkLaneCols, kDwtStripCols,
                          sizeof(kHtSchedule) / sizeof(kHtSchedule[0])};
    std::copy(std::begin(v), std::end(v), out);
}

// The classes of tile p.  kmax (optional): an exponent per block of ONE component that replaces the geometry's (a test's way to a tie).
//   blocks: per row of a tile's table ([comp][block]) {resolution, samples, quads, kmax};  sel: the selection list;
//   cls: per class {count, max_kmax, max_samples, max_quads, cap_kmax, first, role};  out = {rows, entries of sel, classes}
int ep_classes(const grk_amd_tile_params* p, int lds_cap, const uint8_t* kmax, uint32_t* blocks, uint64_t rows_cap, uint32_t* sel,
               uint64_t sel_cap, uint32_t* cls, uint32_t* out)
{
    TileGeom g;
    const int rc = build_tile_geom(*p, g);
    if (rc) return rc;
    if (kmax) for (size_t i = 0; i < g.blocks_comp0.size(); ++i) g.blocks_comp0[i].kmax = kmax[i];
    const uint64_t nrows = (uint64_t)g.blocks_per_comp * p->num_comps;
    const HtClasses pl = plan_ht_classes(g, p->num_comps, lds_cap != 0);
    if (nrows > rows_cap || pl.sel.size() > sel_cap || pl.classes.size() > kHtMaxClasses) return -100;
    for (uint64_t i = 0; i < nrows; ++i) {
        const grk_amd_block& b = g.blocks_comp0[i % g.blocks_per_comp];
        const uint32_t w = b.x1 - b.x0, h = b.y1 - b.y0;
        const uint32_t row[4] = {b.res, w * h, ((w + 1) / 2) * ((h + 1) / 2), b.kmax};
        std::copy(row, row + 4, blocks + 4 * i);
    }
    std::copy(pl.sel.begin(), pl.sel.end(), sel);
    for (size_t k = 0; k < pl.classes.size(); ++k) {
        const HtClassPlan& c = pl.classes[k];
        const uint32_t row[7] = {c.count, c.max_kmax, c.max_samples, c.max_quads, c.cap_kmax, c.first, (uint32_t)c.role};
        std::copy(row, row + 7, cls + 7 * k);
    }
    out[0] = (uint32_t)nrows; out[1] = (uint32_t)pl.sel.size(); out[2] = (uint32_t)pl.classes.size();
    return 0;
}

// out: worst case {ms_words, vlc_words, ms_cap_bits, vlc_cap_bits, stage_bytes, bytes, waves per CU}, the same seven for the cap, use_cap
void ep_lds(uint32_t max_samples, uint32_t max_quads, uint32_t max_kmax, uint32_t cap_kmax, int irrev, int have_fallback, uint64_t* out)
{
    const HtClassLds l = plan_ht_lds(max_samples, max_quads, max_kmax, cap_kmax, irrev != 0, have_fallback != 0);
    const HtLdsPlan* both[2] = {&l.full, &l.cap};
    for (int k = 0; k < 2; ++k) {
        const HtLdsPlan& p = *both[k];
        const uint64_t row[7] = {p.ms_words, p.vlc_words, p.ms_cap_bits, p.vlc_cap_bits, p.stage_bytes, p.bytes, ht_waves_per_cu(p.bytes)};
        std::copy(row, row + 7, out + 7 * k);
    }
    out[14] = l.use_cap;
}
uint64_t ep_lds_bytes(uint32_t samples, uint32_t quads, uint32_t kmax) { return ht_lds_bytes(samples, quads, kmax); }

// cls: per class {count, max_kmax, max_samples, max_quads};  out = {regions, chunk, worst_block, arena_bytes, ovf_entries, ovf_base[n]}
void ep_arena(uint64_t nblocks, uint64_t raw_bytes, uint32_t ntiles, const uint32_t* cls, uint32_t n, uint64_t* out)
{
    std::vector<HtClassPlan> classes;
    for (uint32_t k = 0; k < n; ++k) classes.push_back(HtClassPlan{cls[4 * k], cls[4 * k + 1], cls[4 * k + 2], cls[4 * k + 3], 0, 0, HtRole::All});
    const HtArenaPlan a = plan_ht_arena(nblocks, raw_bytes, ntiles, classes);
    out[0] = a.regions; out[1] = a.chunk; out[2] = a.worst_block; out[3] = a.arena_bytes; out[4] = a.ovf_entries;
    for (uint32_t k = 0; k < n && k < kHtMaxClasses; ++k) out[5 + k] = a.ovf_base[k];
}

// -> HtStream (0 not here, 1 main, 2 side, 3 side2)
int ep_class_stream(int role, int overlapped, int pipelined, int at, int one_level)
{
    return (int)ht_class_stream((HtRole)role, overlapped != 0, pipelined != 0, (HtPoint)at, one_level != 0);
}
// the rows of kHtSchedule that speak of (role, overlapped, pipelined) at whatever point: no two may
int ep_schedule_rows_for(int role, int overlapped, int pipelined)
{
    int n = 0;
    for (const HtScheduleRow& r : kHtSchedule)
        n += (int)r.role == role && r.overlapped == (overlapped != 0) && (r.pipelined < 0 || (r.pipelined != 0) == (pipelined != 0));
    return n;
}

int ep_planes16_ok(const grk_amd_tile_params* p) { return planes16_ok(*p); }
int ep_pk16_level_ok(const grk_amd_tile_params* p, uint32_t l) { return pk16_level_ok(*p, l); }
// in = {overlap, pipelining, frame_streams, planes16, have_side, have_side2, on_device, px_align, samples};  out = {fused, overlap, frame_stream, h16}
void ep_route(const grk_amd_tile_params* p, const uint64_t* in, int* out)
{
    const Route r = plan_route(*p, RouteIn{in[0] != 0, in[1] != 0, (int)in[2], in[3] != 0, in[4] != 0, in[5] != 0, in[6] != 0, (uint32_t)in[7], in[8]});
    out[0] = r.fused; out[1] = r.overlap; out[2] = r.frame_stream; out[3] = r.h16;
}

// in = {cw, ch, px, py, in_stride, m_stride, h16, pk, irreversible, px_lay, px_chan, px_row, zslots, fused, px_bytes}
// out = {packed, lanes, strip_cols, all_fast, seg_pairs, grid_x, grid_y}, then for the part of one component and for the MCT triple
//       {packed, 32-bit key: f97, nc, px, h16, gen, str, packed key: nc, px, nt, ch}
void ep_level(const uint64_t* in, uint32_t* out)
{
    const DwtLevelShape s = plan_dwt_level(DwtLevelDesc{(uint32_t)in[0], (uint32_t)in[1], (uint32_t)in[2], (uint32_t)in[3], (uint32_t)in[4],
                                                        (uint32_t)in[5], in[6] != 0, in[7] != 0, in[8] != 0, (uint32_t)in[9], (uint32_t)in[10],
                                                        in[11], (uint32_t)in[12], in[13] != 0, (uint32_t)in[14]});
    out[0] = s.packed; out[1] = s.lanes; out[2] = s.strip_cols; out[3] = s.all_fast; out[4] = s.seg_pairs; out[5] = s.grid_x; out[6] = s.grid_y;
    for (int i = 0; i < 2; ++i) {
        const DwtInstance& n = s.inst[i];
        const uint32_t row[11] = {n.packed, n.k.f97, n.k.nc, n.k.px, n.k.h16, n.k.gen, n.k.str, n.pk.nc, n.pk.px, n.pk.nt, n.pk.ch};
        std::copy(row, row + 11, out + 7 + 11 * i);
    }
}
// the forward kernels' instance lists (dwt_instances.h): rows of {f97, nc, px, h16, gen, str} / {nc, px, nt, ch}; returns the number of rows
uint32_t ep_dwt_instances(uint32_t* out)
{
    uint32_t n = 0;
    for (const DwtKey& k : kDwtInstances) { const uint32_t row[6] = {k.f97, k.nc, k.px, k.h16, k.gen, k.str}; std::copy(row, row + 6, out + 6 * n++); }
    return n;
}
uint32_t ep_dwt_pk_instances(uint32_t* out)
{
    uint32_t n = 0;
    for (const DwtPkKey& k : kDwtPkInstances) { const uint32_t row[4] = {k.nc, k.px, k.nt, k.ch}; std::copy(row, row + 4, out + 4 * n++); }
    return n;
}
// the parts of a level fused with the pixels: rows of {comp0, zdiv, nc}; out[0] = z slots per tile; returns the number of parts
uint32_t ep_level_parts(int mct, uint32_t ncomp, uint32_t* out)
{
    const uint32_t n = level_part_count(mct != 0, ncomp);
    out[0] = level_part_zslots(mct != 0, ncomp);
    for (uint32_t i = 0; i < n; ++i) { const LevelPart p = level_part(mct != 0, ncomp, i); out[1 + 3 * i] = p.comp0; out[2 + 3 * i] = p.zdiv; out[3 + 3 * i] = p.nc; }
    return n;
}
uint32_t ep_pk_strip_cols(uint32_t cw, uint32_t nt) { return pk_strip_cols(cw, nt); }
} // extern "C"
