// grok_amd/csrc/image_view_plan.h -- what a view of a codestream's image (grk_amd_image_view: the N finest resolutions dropped, a
// window) asks of grk_amd_decode_image_view, worked out on the host before any byte is read or uploaded (image_view_plan.cpp: plain
// C++, no HIP; tests/test_image_view_plan_cpu.py through grk_amd_plan_image_view).  decode_image.cpp asks this plan, and nothing
// else, which tiles to read, what every unit's decode delivers and where that goes.
#pragma once
#include "../../include/grok_amd.h"
#include "image.h"
#include <vector>

#pragma GCC visibility push(hidden)
namespace grk_amd {

// A unit of decoding -- a touched tile's run of components of one size (image.h: comp_runs; without sub-sampling: the tile).
struct ViewUnit {
    uint32_t tile, run;
    grk_amd_tile_params p;      // the FULL unit, as the reader's table and grk_amd_decode_tiles take it
    uint32_t w, h;              // what its decode at the view's reduce delivers (grk_amd_reduced_tile_rect); either may be 0
    int32_t x, y;               // where that rectangle starts in the view's plane of the run's components: negative left of / above it
    bool whole;                 // the view holds all of it
};

struct ViewPlan {
    uint32_t reduce = 0;
    bool sub = false, windowed = false;
    std::vector<CompRun> runs;
    std::vector<uint32_t> tiles;        // the touched tiles in index order
    std::vector<ViewUnit> units;        // [touched tile][run]
    uint32_t comp_w[4] = {0, 0, 0, 0}, comp_h[4] = {0, 0, 0, 0};      // [component]: its plane in the view
};

// view == nullptr: the whole image at full size.  GRK_AMD_OK, or the refusal and in *why its reason.
int plan_image_view(const grk_amd_stream_info& info, const grk_amd_image_view* view, ViewPlan& plan, const char** why);

} // namespace grk_amd
#pragma GCC visibility pop
