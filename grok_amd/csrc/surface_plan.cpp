// grok_amd/csrc/surface_plan.cpp -- the host planning of the surface calls (surface_plan.h) and the host-only entry points around it
// (grk_amd_surface_bytes, grk_amd_surface_format, grk_amd_surface_plan).  No HIP: every bound the kernels of kernels_surface.hip and the
// tile coders trust is decided here, where a CPU test reaches it.
#include "surface_plan.h"
#include <algorithm>

namespace grk_amd {
namespace {
uint64_t cdiv(uint64_t a, uint64_t b) { return (a + b - 1) / b; }
int refuse(const char** why, int rc, const char* text) { if (why) *why = text; return rc; }
// bytes from a row's first sample to the end of its last
uint64_t row_span(const SurfacePlane& p, uint32_t bps) { return ((p.w - 1) * p.step + 1) * bps; }
uint64_t plane_span(const SurfacePlane& p, uint32_t bps) { return (p.h - 1) * p.row_pitch + row_span(p, bps); }
} // namespace

int resolve_surface(const grk_amd_image_layout* im, const grk_amd_tile_params* base, const uint8_t* comp_dx, const uint8_t* comp_dy,
                    const grk_amd_surface* s, ResolvedSurface& out, const char** why)
{
    if (why) *why = "";
    if (!im || !base || !comp_dx || !comp_dy || !s) return refuse(why, GRK_AMD_ERR_INVALID, "surface: a null argument");
    const uint32_t nc = base->num_comps;
    if (!nc || nc > 4) return refuse(why, GRK_AMD_ERR_INVALID, "surface: 1 to 4 components");
    if (!base->prec) return refuse(why, GRK_AMD_ERR_INVALID, "surface: no precision");
    if (base->prec > 16) return refuse(why, GRK_AMD_ERR_UNSUPPORTED, "surface: samples of more than 16 bits");
    if (im->x1 <= im->x0 || im->y1 <= im->y0) return refuse(why, GRK_AMD_ERR_INVALID, "surface: an empty image area");
    out.bps = (base->prec + 7u) / 8u;
    out.comp.clear();
    out.bytes = 0;
    for (uint32_t c = 0; c < nc; ++c) {
        if (!comp_dx[c] || !comp_dy[c]) return refuse(why, GRK_AMD_ERR_INVALID, "surface: a sub-sampling factor of 0");
        const grk_amd_surface_comp& sc = s->comp[c];
        SurfacePlane p{};
        p.x0 = cdiv(im->x0, comp_dx[c]); p.y0 = cdiv(im->y0, comp_dy[c]);
        p.w = cdiv(im->x1, comp_dx[c]) - p.x0; p.h = cdiv(im->y1, comp_dy[c]) - p.y0;
        if (!p.w || !p.h) return refuse(why, GRK_AMD_ERR_INVALID, "surface: a component without samples");
        p.step = sc.step ? sc.step : 1u;
        if (p.step > 4) return refuse(why, GRK_AMD_ERR_INVALID, "surface: a step above 4");
        if (sc.offset % out.bps) return refuse(why, GRK_AMD_ERR_INVALID, "surface: an offset is no multiple of the sample size");
        if (sc.row_pitch % out.bps) return refuse(why, GRK_AMD_ERR_INVALID, "surface: a row pitch is no multiple of the sample size");
        if ((sc.offset | sc.row_pitch) >> 48) return refuse(why, GRK_AMD_ERR_INVALID, "surface: an offset or a row pitch is out of range");
        p.offset = sc.offset;
        p.row_pitch = sc.row_pitch ? sc.row_pitch : row_span(p, out.bps);
        if (p.row_pitch < row_span(p, out.bps)) return refuse(why, GRK_AMD_ERR_INVALID, "surface: a row pitch is smaller than a row");
        if ((uint64_t)base->prec + sc.shift > 8u * out.bps) return refuse(why, GRK_AMD_ERR_INVALID, "surface: precision plus shift exceed the sample's container");
        p.shift = sc.shift;
        out.bytes = std::max(out.bytes, p.offset + plane_span(p, out.bps));
        out.comp.push_back(p);
    }
    return GRK_AMD_OK;
}

int check_surface_disjoint(const ResolvedSurface& rs, const char** why)
{
    const uint32_t bps = rs.bps;
    for (size_t i = 0; i < rs.comp.size(); ++i)
        for (size_t j = i + 1; j < rs.comp.size(); ++j) {
            // (a: the one that starts first)
            const SurfacePlane& a = rs.comp[i].offset <= rs.comp[j].offset ? rs.comp[i] : rs.comp[j];
            const SurfacePlane& b = rs.comp[i].offset <= rs.comp[j].offset ? rs.comp[j] : rs.comp[i];
            if (a.offset + plane_span(a, bps) <= b.offset) continue;                             // disjoint extents
            if (a.row_pitch == b.row_pitch) {
                const uint64_t d = b.offset - a.offset, pitch = a.row_pitch;
                // interleaved partners: b's samples k * bps behind a's, both rows inside one pitch counted from a's row
                if (a.step == b.step && d && d < (uint64_t)a.step * bps && row_span(a, bps) <= pitch && d + row_span(b, bps) <= pitch) continue;
                // side by side: the rows' byte ranges inside a pitch neither wrap nor meet
                const uint64_t ca = a.offset % pitch, cb = b.offset % pitch;
                if (ca + row_span(a, bps) <= pitch && cb + row_span(b, bps) <= pitch && (ca + row_span(a, bps) <= cb || cb + row_span(b, bps) <= ca)) continue;
            }
            return refuse(why, GRK_AMD_ERR_INVALID, "surface: two components of a destination share bytes");
        }
    return GRK_AMD_OK;
}

SurfaceRoute plan_surface_run(const ResolvedSurface& rs, const CompRun& run, bool one_tile, bool decode, bool allow_direct, uint64_t cap,
                              uint32_t base_align)
{
    SurfaceRoute r{false, grk_amd_pixel_layout{}, 0};
    if (!one_tile || !allow_direct || !run.count) return r;
    const uint32_t bps = rs.bps;
    const SurfacePlane& f = rs.comp[run.first];
    // (a shift is applied by KS / KD only)
    for (uint32_t k = 0; k < run.count; ++k) if (rs.comp[run.first + k].shift) return r;
    for (uint32_t k = 1; k < run.count; ++k) {
        const SurfacePlane& p = rs.comp[run.first + k];
        if (p.step != f.step || p.row_pitch != f.row_pitch) return r;
    }
    grk_amd_pixel_layout l{};
    l.row_pitch = f.row_pitch;
    if (f.step == 1) {
        // planar: offsets rising by one plane pitch of at least a plane's span
        if (run.count > 1) {
            const SurfacePlane& s = rs.comp[run.first + 1];
            if (s.offset <= f.offset || s.offset - f.offset < plane_span(f, bps)) return r;
            l.plane_pitch = s.offset - f.offset;
            for (uint32_t k = 2; k < run.count; ++k)
                if (rs.comp[run.first + k].offset != f.offset + k * l.plane_pitch) return r;
        }
    } else {
        // interleaved: offsets bps apart in component order, whole pixels inside a pitch and (their skipped samples too) inside `cap`
        if (decode ? f.step != run.count : f.step < run.count) return r;
        for (uint32_t k = 1; k < run.count; ++k)
            if (rs.comp[run.first + k].offset != f.offset + (uint64_t)k * bps) return r;
        const uint64_t pixel_row = f.w * f.step * bps;
        if (f.row_pitch < pixel_row) return r;
        if (f.offset + (f.h - 1) * f.row_pitch + pixel_row > cap) return r;
        l.interleaved = 1; l.channels = (uint8_t)f.step;
    }
    // the first sample's address: a decode's pixel stores want 4 bytes, an encode's loads a whole sample
    const uint64_t addr = base_align + f.offset;
    if (decode ? (addr & 3u) != 0 : addr % bps != 0) return r;
    r.in_place = true; r.layout = l; r.at = f.offset;
    return r;
}

std::vector<RunSegment> run_segments(const std::vector<uint32_t>& units, uint32_t nr)
{
    std::vector<RunSegment> out;
    for (size_t i0 = 0, i1; i0 < units.size(); i0 = i1) {
        for (i1 = i0 + 1; i1 < units.size() && units[i1] % nr == units[i0] % nr;) ++i1;
        out.push_back(RunSegment{(uint32_t)i0, (uint32_t)(i1 - i0), units[i0] % nr});
    }
    return out;
}

SurfaceStaging plan_surface_staging(const std::vector<std::vector<uint32_t>>& members, const std::vector<SurfaceRoute>& route, const ResolvedSurface& rs,
                                    const std::vector<CompRun>& runs, const std::vector<grk_amd_tile_params>& tp)
{
    const uint32_t nr = (uint32_t)runs.size();
    SurfaceStaging s;
    s.staged.resize(members.size());
    s.segments.resize(members.size());
    for (size_t k = 0; k < members.size(); ++k) {
        std::vector<uint32_t>& S = s.staged[k];
        for (uint32_t u : members[k]) if (!route[u % nr].in_place) S.push_back(u);
        std::stable_sort(S.begin(), S.end(), [nr](uint32_t a, uint32_t b) { return a % nr < b % nr; });
        for (uint32_t u : S) {
            const SurfacePlane& p = rs.comp[runs[u % nr].first];
            s.origins.push_back((uint32_t)(tp[u].tile_x0 - p.x0));
            s.origins.push_back((uint32_t)(tp[u].tile_y0 - p.y0));
        }
        if (!S.empty()) s.group_bytes = std::max<uint64_t>(s.group_bytes, (uint64_t)tp[S[0]].tile_w * tp[S[0]].tile_h * tp[S[0]].num_comps * rs.bps * S.size());
        s.segments[k] = run_segments(S, nr);
    }
    return s;
}

} // namespace grk_amd

using namespace grk_amd;

extern "C" uint64_t grk_amd_surface_bytes(const grk_amd_image_layout* im, const grk_amd_tile_params* base, const uint8_t* comp_dx,
                                          const uint8_t* comp_dy, const grk_amd_surface* surface, const char** why)
{
    ResolvedSurface rs;
    return resolve_surface(im, base, comp_dx, comp_dy, surface, rs, why) ? 0 : rs.bytes;
}

extern "C" int grk_amd_surface_format(int format, const grk_amd_image_layout* im, uint32_t prec, uint64_t pitch, grk_amd_surface* surface,
                                      uint8_t* comp_dx, uint8_t* comp_dy, uint32_t* num_comps, uint64_t* bytes)
{
    if (!im || !surface || !comp_dx || !comp_dy || !prec || im->x1 <= im->x0 || im->y1 <= im->y0) return GRK_AMD_ERR_INVALID;
    if (format < GRK_AMD_SURFACE_NV12 || format > GRK_AMD_SURFACE_P216) return GRK_AMD_ERR_INVALID;
    if (prec > 16) return GRK_AMD_ERR_UNSUPPORTED;
    // P016 / P216: NV12 / NV16 with two-byte samples in the containers' high bits
    uint32_t shift = 0;
    if (format == GRK_AMD_SURFACE_P016 || format == GRK_AMD_SURFACE_P216) {
        if (prec <= 8) return GRK_AMD_ERR_INVALID;
        shift = 16 - prec;
        format = format == GRK_AMD_SURFACE_P016 ? GRK_AMD_SURFACE_NV12 : GRK_AMD_SURFACE_NV16;
    }
    const uint64_t bps = (prec + 7u) / 8u, W = im->x1 - im->x0, H = im->y1 - im->y0;
    const bool pairs = format == GRK_AMD_SURFACE_NV12 || format == GRK_AMD_SURFACE_NV21 || format == GRK_AMD_SURFACE_NV16;
    const bool v_first = format == GRK_AMD_SURFACE_NV21 || format == GRK_AMD_SURFACE_YV12;
    const uint8_t dx = format == GRK_AMD_SURFACE_I444 ? 1 : 2;
    const uint8_t dy = format == GRK_AMD_SURFACE_NV12 || format == GRK_AMD_SURFACE_NV21 || format == GRK_AMD_SURFACE_I420 || format == GRK_AMD_SURFACE_YV12 ? 2 : 1;
    comp_dx[0] = comp_dy[0] = 1;
    comp_dx[1] = comp_dx[2] = dx; comp_dy[1] = comp_dy[2] = dy;
    const uint64_t wc = cdiv(im->x1, dx) - cdiv(im->x0, dx), hc = cdiv(im->y1, dy) - cdiv(im->y0, dy);
    const uint64_t least = std::max(W, pairs ? 2 * wc : (dx == 2 ? 0 : wc)) * bps;
    if (!pitch) pitch = least;
    if (pitch < least || pitch % bps) return GRK_AMD_ERR_INVALID;
    // (planar chroma rows of the 4:2:x forms: half the luma pitch)
    const uint64_t cpitch = pairs || dx == 1 ? pitch : cdiv(cdiv(pitch, 2), bps) * bps;
    if (cpitch < wc * bps) return GRK_AMD_ERR_INVALID;
    *surface = grk_amd_surface{};
    surface->comp[0] = grk_amd_surface_comp{0, pitch, 1, shift};
    const uint64_t chroma = H * pitch;
    const uint32_t u = v_first ? 2 : 1, v = v_first ? 1 : 2;                  // which component lies first in memory
    if (pairs) {
        surface->comp[u] = grk_amd_surface_comp{chroma, cpitch, 2, shift};
        surface->comp[v] = grk_amd_surface_comp{chroma + bps, cpitch, 2, shift};
    } else {
        surface->comp[u] = grk_amd_surface_comp{chroma, cpitch, 1, shift};
        surface->comp[v] = grk_amd_surface_comp{chroma + hc * cpitch, cpitch, 1, shift};
    }
    if (num_comps) *num_comps = 3;
    if (bytes) {
        grk_amd_tile_params p{};
        p.num_comps = 3; p.prec = (uint8_t)prec;
        *bytes = grk_amd_surface_bytes(im, &p, comp_dx, comp_dy, surface, nullptr);
        if (!*bytes) return GRK_AMD_ERR_INVALID;
    }
    return GRK_AMD_OK;
}

extern "C" int grk_amd_surface_plan(const grk_amd_image_layout* im, const grk_amd_tile_params* base, const uint8_t* comp_dx, const uint8_t* comp_dy,
                                    const grk_amd_surface* surface, uint64_t cap, uint32_t base_align, int decode, int allow_direct,
                                    uint8_t* in_place, grk_amd_pixel_layout* layouts, uint64_t* at, uint32_t cap_runs, const char** why)
{
    ResolvedSurface rs;
    int rc = resolve_surface(im, base, comp_dx, comp_dy, surface, rs, why);
    if (rc) return rc;
    if (rs.bytes > cap) return refuse(why, GRK_AMD_ERR_OVERFLOW, "surface: it does not fit `cap`");
    if (decode) { rc = check_surface_disjoint(rs, why); if (rc) return rc; }
    const int64_t nt = grk_amd_layout_num_tiles(im);
    if (nt < 0) return refuse(why, (int)nt, "surface: image area and tile grid do not fit");
    const std::vector<CompRun> runs = comp_runs(base->num_comps, base->mct != 0, comp_dx, comp_dy);
    if (in_place || layouts || at) {
        if (runs.size() > cap_runs) return refuse(why, GRK_AMD_ERR_OVERFLOW, "surface: more runs than `cap_runs`");
        for (size_t r = 0; r < runs.size(); ++r) {
            const SurfaceRoute route = plan_surface_run(rs, runs[r], nt == 1, decode != 0, allow_direct != 0, cap, base_align & 3u);
            if (in_place) in_place[r] = route.in_place ? 1 : 0;
            if (layouts) layouts[r] = route.layout;
            if (at) at[r] = route.at;
        }
    }
    return (int)runs.size();
}
