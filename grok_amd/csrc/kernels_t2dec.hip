// grok_amd/csrc/kernels_t2dec.hip -- the device's share of reading a whole codestream (grk_amd_decode_image): KT2 of kernels_t2.hip
// in the other direction.  Both kernels are plain byte movers, a wave per run of bytes (wave_copy.h).
//   KG  gather     a code-block whose bytes come in several pieces (several layers) gets them end to end in the appendix behind
//                  the uploaded codestream: one wave per piece
//   KP  placement  a geometry group's decoded tiles (back to back, component-major, tight) into the image's planes at each
//                  tile's rectangle: a workgroup per (row band, component, tile), a wave per row
//   the status word of a group's decode is OR-ed into the image's: a later group's decode starts its own from zero
#include "kernels.h"
#include "wave_copy.h"

namespace grk_amd {

__global__ __launch_bounds__(256) void t2dec_gather_kernel(const grk_amd_tp_segment* moves, uint64_t nmoves, const uint8_t* src, uint8_t* dst)
{
    const uint64_t i = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (i >= nmoves) return;
    const grk_amd_tp_segment m = moves[i];
    wave_copy(dst + m.dst, src + m.src, m.len, threadIdx.x & 63u);
}

constexpr uint32_t kPlaceRows = 16;         // rows of a tile-component per workgroup: four per wave

__global__ __launch_bounds__(256) void t2dec_place_kernel(PlaceArgs a)
{
    const uint32_t tile = blockIdx.z, comp = blockIdx.y, lane = threadIdx.x & 63u;
    const uint64_t row_bytes = (uint64_t)a.w * a.bps, img_row = a.img_row ? a.img_row : (uint64_t)a.img_w * a.bps;
    const uint64_t img_plane = a.img_plane ? a.img_plane : (uint64_t)a.img_h * img_row;
    const uint8_t* const s = a.tiles + ((uint64_t)tile * a.ncomp + comp) * a.h * row_bytes;
    uint8_t* const d = a.image + (uint64_t)comp * img_plane + (uint64_t)a.rects[2 * tile + 1] * img_row + (uint64_t)a.rects[2 * tile] * a.bps;
    const uint32_t y1 = min(a.h, (blockIdx.x + 1) * kPlaceRows);
    for (uint32_t y = blockIdx.x * kPlaceRows + (threadIdx.x >> 6); y < y1; y += 4)
        wave_copy(d + y * img_row, s + y * row_bytes, row_bytes, lane);
}

__global__ void t2dec_or_status_kernel(unsigned int* into, const unsigned int* from, int assign)
{
    if (assign) *into = *from; else *into |= *from;
}

hipError_t launch_t2dec_gather(const grk_amd_tp_segment* d_moves, uint64_t nmoves, const uint8_t* src, uint8_t* dst, hipStream_t s)
{
    if (!nmoves) return hipSuccess;
    hipLaunchKernelGGL(t2dec_gather_kernel, dim3((uint32_t)((nmoves + 3) / 4)), dim3(256), 0, s, d_moves, nmoves, src, dst);
    return hipGetLastError();
}

hipError_t launch_t2dec_place(const PlaceArgs& a, hipStream_t s)
{
    if (!a.ntiles || !a.w || !a.h) return hipSuccess;
    hipLaunchKernelGGL(t2dec_place_kernel, dim3((a.h + kPlaceRows - 1) / kPlaceRows, a.ncomp, a.ntiles), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_t2dec_or_status(unsigned int* into, const unsigned int* from, bool assign, hipStream_t s)
{
    hipLaunchKernelGGL(t2dec_or_status_kernel, dim3(1), dim3(1), 0, s, into, from, assign ? 1 : 0);
    return hipGetLastError();
}

} // namespace grk_amd
