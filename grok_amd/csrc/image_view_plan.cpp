// grok_amd/csrc/image_view_plan.cpp -- the plan of grk_amd_decode_image_view (image_view_plan.h).  Host only.
//
// Reduce r (grk_decompress -r): component k of the image is [ceil(ceil(X0 / dx) / 2^r), ceil(ceil(X1 / dx) / 2^r)) and likewise in y;
// a tile's component covers the rectangle grk_amd_reduced_tile_rect gives for its tile-component.  Both are ceilings of the same
// bounds, so the tiles' rectangles partition the component's plane.  A window is given in the samples of that plane, counted from
// its top-left sample; a tile is touched when its rectangle meets the window.
#include "image_view_plan.h"
#include <algorithm>

using namespace grk_amd;

int grk_amd::plan_image_view(const grk_amd_stream_info& info, const grk_amd_image_view* view, ViewPlan& plan, const char** why)
{
    auto refuse = [why](int code, const char* text) { if (why) *why = text; return code; };
    plan = ViewPlan{};
    const grk_amd_image_view v = view ? *view : grk_amd_image_view{0, 0, 0, 0, 0};
    const uint32_t nc = info.base.num_comps, r = v.reduce;
    if (!nc || nc > 4) return refuse(GRK_AMD_ERR_INVALID, "a stream of no or more than 4 components");
    if (r > info.base.num_levels) return refuse(GRK_AMD_ERR_INVALID, "a view that drops more resolutions than the stream has levels");
    plan.reduce = r;
    plan.windowed = v.x0 || v.y0 || v.x1 || v.y1;
    for (uint32_t k = 0; k < nc; ++k) {
        if (!info.comp_dx[k] || !info.comp_dy[k]) return refuse(GRK_AMD_ERR_INVALID, "a component with a sub-sampling factor of 0");
        plan.sub = plan.sub || info.comp_dx[k] != 1 || info.comp_dy[k] != 1;
    }
    if (plan.windowed && (v.x1 <= v.x0 || v.y1 <= v.y0)) return refuse(GRK_AMD_ERR_INVALID, "an empty window");
    if (plan.windowed && plan.sub) return refuse(GRK_AMD_ERR_UNSUPPORTED, "a window of a stream with sub-sampled components");
    // the components' planes at this reduction: origin and size
    auto lo = [r](uint64_t a) { return (a + (1ull << r) - 1) >> r; };
    uint64_t ox[4], oy[4];
    for (uint32_t k = 0; k < nc; ++k) {
        const uint64_t dx = info.comp_dx[k], dy = info.comp_dy[k];
        ox[k] = lo((info.layout.x0 + dx - 1) / dx); oy[k] = lo((info.layout.y0 + dy - 1) / dy);
        const uint64_t w = lo(((uint64_t)info.layout.x1 + dx - 1) / dx) - ox[k], h = lo(((uint64_t)info.layout.y1 + dy - 1) / dy) - oy[k];
        if (!w || !h) return refuse(GRK_AMD_ERR_INVALID, "a view without a sample");
        if (w > 0x7FFFFFFFull || h > 0x7FFFFFFFull) return refuse(GRK_AMD_ERR_UNSUPPORTED, "an image of more than 2^31 - 1 columns or rows");
        plan.comp_w[k] = (uint32_t)w; plan.comp_h[k] = (uint32_t)h;
    }
    if (plan.windowed) {
        if (v.x1 > plan.comp_w[0] || v.y1 > plan.comp_h[0]) return refuse(GRK_AMD_ERR_INVALID, "a window outside the view's image");
        for (uint32_t k = 0; k < nc; ++k) { plan.comp_w[k] = v.x1 - v.x0; plan.comp_h[k] = v.y1 - v.y0; }
    }
    plan.runs = comp_runs(nc, info.base.mct != 0, info.comp_dx, info.comp_dy);
    const uint32_t nr = (uint32_t)plan.runs.size();
    std::vector<ViewUnit> of_tile(nr);
    for (uint32_t t = 0; t < info.num_tiles; ++t) {
        bool touched = false;
        for (uint32_t i = 0; i < nr; ++i) {
            const CompRun& run = plan.runs[i];
            ViewUnit& u = of_tile[i];
            u.tile = t; u.run = i;
            int rc;
            if (!plan.sub) rc = grk_amd_layout_tile(&info.layout, &info.base, t, &u.p);
            else {
                rc = grk_amd_layout_tile_comp(&info.layout, &info.base, info.comp_dx[run.first], info.comp_dy[run.first], t, &u.p);
                u.p.num_comps = (uint16_t)run.count; u.p.mct = run.mct ? 1 : 0;
            }
            uint32_t ux0 = 0, uy0 = 0;
            if (!rc) rc = reduced_tile_rect(u.p, r, &ux0, &uy0, &u.w, &u.h);
            if (rc) return refuse(rc, "a tile's geometry");
            const int64_t x = (int64_t)ux0 - (int64_t)ox[run.first] - v.x0, y = (int64_t)uy0 - (int64_t)oy[run.first] - v.y0;
            const int64_t W = plan.comp_w[run.first], H = plan.comp_h[run.first];
            u.x = (int32_t)x; u.y = (int32_t)y;
            u.whole = x >= 0 && y >= 0 && x + u.w <= W && y + u.h <= H;
            touched = touched || (u.w && u.h && x < W && y < H && x + u.w > 0 && y + u.h > 0);
        }
        if (!touched) continue;
        plan.tiles.push_back(t);
        plan.units.insert(plan.units.end(), of_tile.begin(), of_tile.end());
    }
    return GRK_AMD_OK;
}

extern "C" int grk_amd_image_view_size(const grk_amd_stream_info* info, const grk_amd_image_view* view, uint32_t comp, uint32_t* w, uint32_t* h)
{
    if (!info || !w || !h || comp >= info->base.num_comps || comp >= 4) return GRK_AMD_ERR_INVALID;
    ViewPlan plan;
    const int rc = plan_image_view(*info, view, plan, nullptr);
    if (rc) return rc;
    *w = plan.comp_w[comp]; *h = plan.comp_h[comp];
    return GRK_AMD_OK;
}

extern "C" int64_t grk_amd_plan_image_view(const grk_amd_stream_info* info, const grk_amd_image_view* view, uint32_t* tiles, uint64_t tile_cap,
                                           uint64_t* num_tiles, grk_amd_view_unit* units, uint64_t cap)
{
    if (!info) return GRK_AMD_ERR_INVALID;
    ViewPlan plan;
    const int rc = plan_image_view(*info, view, plan, nullptr);
    if (rc) return rc;
    if (num_tiles) *num_tiles = plan.tiles.size();
    if ((tiles && plan.tiles.size() > tile_cap) || (units && plan.units.size() > cap)) return GRK_AMD_ERR_OVERFLOW;
    if (tiles) std::copy(plan.tiles.begin(), plan.tiles.end(), tiles);
    for (size_t i = 0; units && i < plan.units.size(); ++i) {
        const ViewUnit& u = plan.units[i];
        const CompRun& run = plan.runs[u.run];
        units[i] = grk_amd_view_unit{u.tile, run.first, run.count, u.w, u.h, u.x, u.y, u.whole ? 1u : 0u};
    }
    return (int64_t)plan.units.size();
}
