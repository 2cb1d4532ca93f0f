// grok_amd/csrc/surface_plan.h -- the host planning of grk_amd_encode_surface / grk_amd_decode_surface (HIP-free; private to the
// library, defined in surface_plan.cpp and tested on the CPU): a surface resolved against the image's components, the rule that two
// components of a destination share no byte, and per run of components the route -- in place through a grk_amd_pixel_layout, or
// staged through tight planes and the two kernels of kernels_surface.hip --, and the staging plan of a whole call, which
// grk_amd_encode_surface (surface.cpp) and the surface route of the decode (decode_image_plan.cpp) share.
#pragma once
#include "../../include/grok_amd.h"
#include "image.h"
#include <vector>

#pragma GCC visibility push(hidden)       // nothing declared below is part of the library's interface
namespace grk_amd {

// component c of the image on the surface: its size, its first sample at (x0, y0) of the component's grid, every pitch in bytes;
// shift: the zero bits below a sample in its container (P010: 6)
struct SurfacePlane { uint64_t offset, row_pitch, w, h, x0, y0; uint32_t step, shift; };
struct ResolvedSurface {
    uint32_t bps = 0;
    std::vector<SurfacePlane> comp;
    uint64_t bytes = 0;                        // base .. end of the last sample of any component
};
// GRK_AMD_OK, or the refusal and *why
int resolve_surface(const grk_amd_image_layout* im, const grk_amd_tile_params* base, const uint8_t* comp_dx, const uint8_t* comp_dy,
                    const grk_amd_surface* s, ResolvedSurface& out, const char** why);
// a destination's components pairwise: disjoint, interleaved partners, or side by side -- else GRK_AMD_ERR_INVALID and *why
int check_surface_disjoint(const ResolvedSurface& rs, const char** why);

// a run's route: in place (the tile coder on base + at in `layout`) or staged; a run with a shifted component is always staged (the
// shift is KS's and KD's: the tile coders and grk_amd_pixel_layout know none)
struct SurfaceRoute { bool in_place; grk_amd_pixel_layout layout; uint64_t at; };
// one_tile: the image is one tile (the run is the unit); cap: the bytes behind the base; base_align: the base address modulo 4
SurfaceRoute plan_surface_run(const ResolvedSurface& rs, const CompRun& run, bool one_tile, bool decode, bool allow_direct, uint64_t cap,
                              uint32_t base_align);

// `count` units of a batch from its `first`, all of run `run`: one launch of a placement (or cut) kernel
struct RunSegment { uint32_t first, count, run; };
// a batch's units, sorted run by run (unit u is of run u % nr), as its launches: the units of one run, one launch
std::vector<RunSegment> run_segments(const std::vector<uint32_t>& units, uint32_t nr);

// What a surface call stages: per geometry group (members[k]: its units) the units whose run is not handled in place, run by run;
// their origins on the surface's planes (x, y per unit) in that order, group after group -- the one array that is uploaded --; the
// bytes of the largest group's tight planes; and each group's launches of KS / KD
struct SurfaceStaging {
    std::vector<std::vector<uint32_t>> staged;          // [group]
    std::vector<std::vector<RunSegment>> segments;      // [group]
    std::vector<uint32_t> origins;
    uint64_t group_bytes = 0;
};
// route, runs: [run]; tp: [unit], the units' parameters
SurfaceStaging plan_surface_staging(const std::vector<std::vector<uint32_t>>& members, const std::vector<SurfaceRoute>& route, const ResolvedSurface& rs,
                                    const std::vector<CompRun>& runs, const std::vector<grk_amd_tile_params>& tp);

} // namespace grk_amd
#pragma GCC visibility pop
