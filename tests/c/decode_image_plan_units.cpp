// tests/c/decode_image_plan_units.cpp -- the whole-image decode's host planning (grok_amd/csrc/decode_image_plan.cpp, the staging plan
// of surface_plan.cpp) behind plain C entry points, for tests/test_decode_image_plan_cpu.py: built at test time with g++ together
// with the library's HIP-free sources only, no GPU, no HIP -- that it links is itself the test that none is needed.  Python hands
// over codestream bytes; header and packets are read here, and the plans come back in flat arrays.  One plan at a time is held in
// file-scope state; every refusal's text is kept for dip_reason().
#include "../../grok_amd/csrc/decode_image_plan.h"
#include <algorithm>
#include <cstring>
#include <string>

using namespace grk_amd;

namespace {
std::string g_why;
std::vector<uint8_t> g_cs;
grk_amd_stream_info g_info;
ViewPlan g_plan;
ImageDest g_dest;
std::vector<StreamPart> g_parts;
CodedPlan g_coded;
StreamTable g_tab;
std::vector<grk_amd_coded_block> g_old_rows, g_rows;
std::vector<grk_amd_tp_segment> g_old_moves;
std::vector<uint64_t> g_unit_row;
std::vector<uint32_t> g_first;
std::vector<grk_amd_segment> g_segs;
SurfaceStaging g_staging;

int keep(int rc, const char* why) { g_why = why ? why : ""; return rc; }
} // namespace

extern "C" {
const char* dip_reason(void) { return g_why.c_str(); }

// header -> view plan (view == nullptr: the whole image) -> destination plan.  only (n_only of them, rising): the view plan is cut
// down to these of its tiles first -- tiles that no window touches together, such as a diagonal
int dip_plan(const uint8_t* cs, uint64_t len, const grk_amd_image_view* view, const grk_amd_pixel_layout* layout, int upsample, int on_device, uint64_t cap,
             uint32_t dst_align, int direct, const grk_amd_surface* surf, const uint32_t* only, uint32_t n_only)
{
    g_cs.assign(cs, cs + len);
    std::string err;
    int rc = read_stream_header(g_cs.data(), len, g_info, err);
    if (rc) return keep(rc, err.c_str());
    const char* why = "";
    rc = plan_image_view(g_info, view, g_plan, &why);
    if (rc) return keep(rc, why);
    if (only) {
        ViewPlan cut = g_plan;
        cut.tiles.clear(); cut.units.clear();
        const size_t nr = g_plan.runs.size();
        for (size_t i = 0; i < g_plan.tiles.size(); ++i)
            if (std::find(only, only + n_only, g_plan.tiles[i]) != only + n_only) {
                cut.tiles.push_back(g_plan.tiles[i]);
                cut.units.insert(cut.units.end(), g_plan.units.begin() + i * nr, g_plan.units.begin() + (i + 1) * nr);
            }
        g_plan = cut;
    }
    ImageDestIn in;
    if (layout) in.layout = *layout;
    in.upsample = upsample != 0; in.pixels_on_device = on_device != 0; in.cap = cap; in.dst_align = dst_align; in.surface_direct = direct != 0;
    rc = plan_image_dest(g_info, g_plan, in, surf, g_dest, &why);
    return keep(rc, why);
}

// out[32]
void dip_dest(uint64_t* out)
{
    const ImageDest& d = g_dest;
    const uint64_t v[] = {(uint64_t)d.route, d.sub, d.up, d.ht, d.want_segs, d.all, d.bps, d.nr, d.W, d.H, d.total, d.kstep, d.group_bytes,
                          d.groups.size(), d.places.size() / 2, d.fills.size(), d.tp.size(), d.ipx.lay, d.ipx.channels, d.ipx.xstep, d.ipx.row, d.ipx.kstep,
                          d.ipx.bytes, d.unit_ch, d.upload_image, d.region[0], d.region[1], d.region[2], d.region[3], d.tile_layout.interleaved,
                          d.tile_layout.channels, d.tile_layout.fill};
    std::memcpy(out, v, sizeof v);
}
// [component] x {at, w, h, x0, y0}
void dip_planes(uint64_t* out) { for (const ImagePlane& p : g_dest.plane) { const uint64_t v[] = {p.at, p.w, p.h, p.x0, p.y0}; std::memcpy(out, v, sizeof v); out += 5; } }
void dip_places(int32_t* out) { if (!g_dest.places.empty()) std::memcpy(out, g_dest.places.data(), g_dest.places.size() * 4); }
// [fill] x {comp, x0, y0, w, h, value}
void dip_fills(uint32_t* out) { for (const FillRect& f : g_dest.fills) { const uint32_t v[] = {f.comp, f.x0, f.y0, f.w, f.h, f.value}; std::memcpy(out, v, sizeof v); out += 6; } }
// [run] x {at, bytes, beside}
void dip_run_dest(uint64_t* out) { for (const RunDest& r : g_dest.run_dest) { *out++ = r.at; *out++ = r.bytes; *out++ = r.beside; } }
// [unit] x {tile_x0, tile_y0, tile_w, tile_h, num_comps, first component, w, h, x, y (signed), group}
void dip_units(int64_t* out)
{
    for (size_t u = 0; u < g_dest.tp.size(); ++u) {
        const grk_amd_tile_params& p = g_dest.tp[u];
        const ViewUnit& vu = g_plan.units[u];
        const int64_t v[] = {p.tile_x0, p.tile_y0, p.tile_w, p.tile_h, p.num_comps, g_plan.runs[u % g_dest.nr].first, vu.w, vu.h, vu.x, vu.y, g_dest.g.of[u]};
        std::memcpy(out, v, sizeof v); out += 11;
    }
}
// [component] x {offset, row_pitch, w, h, x0, y0, step}; [run] x {in_place, at, interleaved, channels, row_pitch, plane_pitch}
void dip_surface(uint64_t* comps, uint64_t* routes)
{
    for (const SurfacePlane& p : g_dest.rs.comp) { const uint64_t v[] = {p.offset, p.row_pitch, p.w, p.h, p.x0, p.y0, p.step}; std::memcpy(comps, v, sizeof v); comps += 7; }
    for (const SurfaceRoute& r : g_dest.surf_route) {
        const uint64_t v[] = {r.in_place, r.at, r.layout.interleaved, r.layout.channels, r.layout.row_pitch, r.layout.plane_pitch};
        std::memcpy(routes, v, sizeof v); routes += 6;
    }
}
// out[13] = {tile_w, tile_h, tile_x0, tile_y0, num_comps, uw, uh, unit_size, skip, place_at, units, in-place units, launches}
void dip_group(uint32_t k, uint64_t* out)
{
    const ImageGroup& G = g_dest.groups.at(k);
    const uint64_t v[] = {G.p.tile_w, G.p.tile_h, G.p.tile_x0, G.p.tile_y0, G.p.num_comps, G.uw, G.uh, G.unit_size, G.skip, G.place_at, G.units.size(),
                          G.in_place.size(), G.launches.size()};
    std::memcpy(out, v, sizeof v);
}
// launches: [launch] x {first, count, run, at, ncomp, bps, w, h, row, kstep, dx, dy}
void dip_group_lists(uint32_t k, uint32_t* units, uint32_t* in_place, uint64_t* launches)
{
    const ImageGroup& G = g_dest.groups.at(k);
    for (uint32_t u : G.units) *units++ = u;
    for (uint32_t u : G.in_place) *in_place++ = u;
    for (const ImageLaunch& l : G.launches) {
        const uint64_t v[] = {l.seg.first, l.seg.count, l.seg.run, l.at, l.ncomp, l.bps, l.w, l.h, l.row, l.kstep, l.dx, l.dy};
        std::memcpy(launches, v, sizeof v); launches += 12;
    }
}

// ---- the coded buffer of the plan's view ------------------------------------------------------------------------------------
// out[4] = {all, up_len, coded_cap, copies}; parts: [tile] x {at, len}
int dip_coded(uint64_t* out, uint64_t* parts)
{
    std::string err;
    const int rc = locate_stream_parts(g_cs.data(), g_cs.size(), g_info, g_parts, err);
    if (rc) return keep(rc, err.c_str());
    plan_coded(g_cs.size(), g_info.num_layers, g_dest.all, g_plan.tiles, g_parts, g_coded);
    out[0] = g_dest.all; out[1] = g_coded.up_len; out[2] = g_coded.coded_cap; out[3] = g_coded.copies.size();
    for (const StreamPart& p : g_parts) { *parts++ = p.at; *parts++ = p.len; }
    return keep(GRK_AMD_OK, "");
}
// part_to: [touched tile]; copies: [copy] x {to, from, n}
void dip_coded_lists(uint64_t* part_to, uint64_t* copies)
{
    for (uint64_t v : g_coded.part_to) *part_to++ = v;
    for (const CodedCopy& c : g_coded.copies) { *copies++ = c.to; *copies++ = c.from; *copies++ = c.n; }
}

// the packets of the view's tiles, then (corrupt: 0 none; 1 the first coded row of the first touched tile to just before its
// tile-part; 2 the first move's source behind its tile-part; 3 the last tile's last row dropped) the rebase.  out[4] = {rows, moves, segments,
// appendix bytes}
int dip_read_and_rebase(int corrupt, uint64_t* out)
{
    std::string err;
    g_tab = StreamTable{};
    int rc = read_stream_packets_of(g_cs.data(), g_cs.size(), g_info, g_parts, g_dest.all ? nullptr : &g_plan.tiles, g_plan.reduce, 1, g_tab, err);
    if (rc) return keep(rc, err.c_str());
    const StreamPart& sp = g_parts[g_plan.tiles[0]];
    if (corrupt == 1)
        for (uint64_t k = g_tab.row_at[0]; k < g_tab.row_at[1]; ++k)
            if (g_tab.rows[k].length && g_tab.rows[k].offset < g_cs.size()) { g_tab.rows[k].offset = sp.at - 1; break; }
    if (corrupt == 2) {
        if (g_tab.move_at[1] == g_tab.move_at[0]) return keep(-100, "driver: the tile has no move to corrupt");
        g_tab.moves[g_tab.move_at[0]].src = sp.at + sp.len + 1;
    }
    if (corrupt == 3) { g_tab.rows.pop_back(); --g_tab.row_at.back(); }
    g_old_rows = g_tab.rows; g_old_moves = g_tab.moves;
    const char* why = "";
    rc = rebase_table(g_tab, g_cs.size(), g_dest.all, g_plan.tiles, g_parts, g_coded, g_dest, g_unit_row, &why);
    out[0] = g_tab.rows.size(); out[1] = g_tab.moves.size(); out[2] = g_tab.segments.size(); out[3] = g_tab.appendix_bytes;
    return keep(rc, why);
}
void dip_table(grk_amd_coded_block* old_rows, grk_amd_coded_block* rows, grk_amd_tp_segment* old_moves, grk_amd_tp_segment* moves, uint32_t* first_segment,
               grk_amd_segment* segments, uint64_t* unit_row)
{
    std::copy(g_old_rows.begin(), g_old_rows.end(), old_rows);
    std::copy(g_tab.rows.begin(), g_tab.rows.end(), rows);
    std::copy(g_old_moves.begin(), g_old_moves.end(), old_moves);
    std::copy(g_tab.moves.begin(), g_tab.moves.end(), moves);
    std::copy(g_tab.first_segment.begin(), g_tab.first_segment.end(), first_segment);
    std::copy(g_tab.segments.begin(), g_tab.segments.end(), segments);
    std::copy(g_unit_row.begin(), g_unit_row.end(), unit_row);
}

// a batch's tables, as the plan wants them (want_segs of the destination plan).  out[3] = {rows, entries of first, segments}
void dip_group_tables(const uint32_t* units, uint64_t n, uint64_t* out)
{
    group_tables(g_tab, g_unit_row, units, n, g_dest.want_segs, g_rows, g_first, g_segs);
    out[0] = g_rows.size(); out[1] = g_first.size(); out[2] = g_segs.size();
}
void dip_group_tables_get(grk_amd_coded_block* rows, uint32_t* first, grk_amd_segment* segs)
{
    std::copy(g_rows.begin(), g_rows.end(), rows);
    std::copy(g_first.begin(), g_first.end(), first);
    std::copy(g_segs.begin(), g_segs.end(), segs);
}

// ---- the staging plan as grk_amd_encode_surface asks for it: the units of every tile of the image, the encoder's routes -----
// out[3] = {groups, staged units, group_bytes}
int dip_encode_staging(const grk_amd_image_layout* im, const grk_amd_tile_params* base, const uint8_t* comp_dx, const uint8_t* comp_dy,
                       const grk_amd_surface* surf, uint64_t cap, uint32_t base_align, int direct, uint64_t* out)
{
    ResolvedSurface rs;
    const char* why = "";
    int rc = resolve_surface(im, base, comp_dx, comp_dy, surf, rs, &why);
    if (rc) return keep(rc, why);
    const int64_t nt = grk_amd_layout_num_tiles(im);
    if (nt < 0) return keep((int)nt, "driver: the tile grid");
    const std::vector<CompRun> runs = comp_runs(base->num_comps, base->mct != 0, comp_dx, comp_dy);
    std::vector<grk_amd_tile_params> units;
    UnitGroups g;
    for (uint32_t t = 0; t < (uint32_t)nt; ++t)
        for (const CompRun& run : runs) {
            grk_amd_tile_params p{};
            rc = grk_amd_layout_tile_comp(im, base, comp_dx[run.first], comp_dy[run.first], t, &p);
            if (rc) return keep(rc, "driver: a tile-component");
            p.num_comps = (uint16_t)run.count; p.mct = run.mct ? 1 : 0;
            units.push_back(p);
            rc = add_unit(g, p);
            if (rc) return keep(rc, "driver: a unit's geometry");
        }
    std::vector<SurfaceRoute> route;
    for (const CompRun& run : runs) route.push_back(plan_surface_run(rs, run, nt == 1, false, direct != 0, cap, base_align));
    g_staging = plan_surface_staging(g.members, route, rs, runs, units);
    out[0] = g_staging.staged.size(); out[1] = g_staging.origins.size() / 2; out[2] = g_staging.group_bytes;
    return keep(GRK_AMD_OK, "");
}
// units: the staged units group after group; group_of: [staged unit] its group; segments: [segment] x {group, first, count, run}, at
// most `cap_segments`; returns their number
uint32_t dip_encode_staging_lists(uint32_t* units, uint32_t* group_of, uint32_t* origins, uint32_t* segments, uint32_t cap_segments)
{
    uint32_t n = 0;
    for (size_t k = 0; k < g_staging.staged.size(); ++k) {
        for (uint32_t u : g_staging.staged[k]) { *units++ = u; *group_of++ = (uint32_t)k; }
        for (const RunSegment& s : g_staging.segments[k]) {
            if (n < cap_segments) { const uint32_t v[] = {(uint32_t)k, s.first, s.count, s.run}; std::memcpy(segments + 4 * n, v, sizeof v); }
            ++n;
        }
    }
    std::copy(g_staging.origins.begin(), g_staging.origins.end(), origins);
    return n;
}

// ---- the functions that moved to HIP-free homes ---------------------------------------------------------------------------------
// of: [unit] its group
int dip_add_units(const grk_amd_tile_params* p, uint32_t n, uint32_t* of)
{
    UnitGroups g;
    for (uint32_t i = 0; i < n; ++i) { const int rc = add_unit(g, p[i]); if (rc) return rc; }
    std::copy(g.of.begin(), g.of.end(), of);
    return (int)g.geoms.size();
}
// out[8] = {lay, channels, xstep, fill, row, kstep, tile, bytes}; 1, or 0 and the reason
int dip_resolve_layout(const grk_amd_tile_params* p, const grk_amd_pixel_layout* l, uint32_t w, uint32_t h, uint32_t ntiles, uint64_t* out)
{
    PixelLayout px{};
    const char* why = "";
    const bool ok = resolve_pixel_layout(*p, l, w, h, ntiles, px, &why);
    g_why = why;
    const uint64_t v[] = {px.lay, px.channels, px.xstep, px.fill, px.row, px.kstep, px.tile, px.bytes};
    std::memcpy(out, v, sizeof v);
    return ok ? 1 : 0;
}
// every i in [0, n) exactly once, on `threads` threads: hits[i] counts them
int dip_parallel_for(uint32_t n, uint32_t threads, uint32_t* hits)
{
    return parallel_for(n, threads, [&](size_t i) -> int { ++hits[i]; return GRK_AMD_OK; });
}
} // extern "C"
