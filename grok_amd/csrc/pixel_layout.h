// grok_amd/csrc/pixel_layout.h -- a grk_amd_pixel_layout resolved against a tile size (HIP-free; host_common.cpp).  context.h includes
// it for the kernels' launchers, the host planners (decode_image_plan.cpp) include it alone.
#pragma once
#include "../../include/grok_amd.h"

#pragma GCC visibility push(hidden)       // nothing declared below is part of the library's interface
// A pixel layout resolved for tiles of w x h samples per component: every pitch in bytes, `lay` as DwtLevelArgs::px_lay
// (0: what the default layout amounts to), `bytes` the extent of ntiles tiles
struct PixelLayout { uint32_t lay, channels, xstep, fill; uint64_t row, kstep, tile, bytes; };
bool resolve_pixel_layout(const grk_amd_tile_params& p, const grk_amd_pixel_layout* l, uint32_t w, uint32_t h, uint32_t ntiles,
                          PixelLayout& out, const char** why);
#pragma GCC visibility pop
