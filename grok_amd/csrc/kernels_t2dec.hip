// grok_amd/csrc/kernels_t2dec.hip -- the device's share of reading a whole codestream (grk_amd_decode_image): KT2 of kernels_t2.hip
// in the other direction.  Both kernels are plain byte movers, a wave per run of bytes (wave_copy.h).
//   KG  gather     a code-block whose bytes come in several pieces (several layers) gets them end to end in the appendix behind
//                  the uploaded codestream: one wave per piece
//   KP  placement  a geometry group's decoded tiles (back to back, component-major, tight) into the image's planes at each
//                  tile's rectangle: a workgroup per (row band, component, tile), a wave per row.  The rectangle's position is
//                  signed and the tile is clipped to the destination (a view's window, grk_amd_decode_image_view): rows above or
//                  below it are skipped, a row's surviving run of whole samples (pixels) is what the wave copies
//   KU  upsampling placement: the same for sub-sampled components delivered on the reference grid -- every source sample is
//                  written to its footprint of dx x dy image samples (clipped to the image area), a wave per source row as in KP.
//                  dx = 1 planar rows are copies; dx = 2 rows of one-byte samples into a planar destination are doubled in
//                  registers, eight source bytes to one aligned 16-byte store; every other case stores sample by sample
//                  (interleaved destinations, where components of other runs share the pixels; dx >= 3; 2-byte samples)
//   KF  fill       one value into a rectangle of one component of such an image (the zero strip, the extra samples of pixels)
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
    // the tile's columns [cx0, cx1) and rows [cy0, cy1) that fall into the destination's img_w x img_h (all of them for a tile inside it)
    const int64_t px = a.rects[2 * tile], py = a.rects[2 * tile + 1];
    const int64_t cx0 = max((int64_t)0, -px), cx1 = min((int64_t)a.w, (int64_t)a.img_w - px);
    const int64_t cy0 = max((int64_t)0, -py), cy1 = min((int64_t)a.h, (int64_t)a.img_h - py);
    if (cx0 >= cx1 || cy0 >= cy1) return;
    const uint8_t* const s = a.tiles + ((uint64_t)tile * a.ncomp + comp) * a.h * row_bytes + (uint64_t)cx0 * a.bps;
    uint8_t* const d = a.image + (uint64_t)comp * img_plane + (uint64_t)(px + cx0) * a.bps;
    const uint64_t run = (uint64_t)(cx1 - cx0) * a.bps;
    const uint32_t y1 = min((uint32_t)cy1, (blockIdx.x + 1) * kPlaceRows);
    for (uint32_t y = blockIdx.x * kPlaceRows + (threadIdx.x >> 6); y < y1; y += 4)
        if (y >= (uint32_t)cy0) wave_copy(d + (uint64_t)(py + y) * img_row, s + y * row_bytes, run, lane);
}

// a | b << 8  ->  a | a << 8 | b << 16 | b << 24
__device__ __forceinline__ uint32_t twice(uint32_t v)
{
    const uint32_t x = (v & 0xFFu) | ((v & 0xFF00u) << 8);
    return x | (x << 8);
}

// n destination bytes at d, byte k = s[k >> 1], by one wave: 16-byte stores on the destination's alignment, each from eight source
// bytes (nine where the store starts on the second byte of a pair), head and tail by bytes.  n <= 2 x the source bytes.
__device__ __forceinline__ void wave_double_bytes(uint8_t* d, const uint8_t* s, uint64_t n, uint32_t lane)
{
    const uint64_t head = min(n, (uint64_t)((0 - (uintptr_t)d) & 15u));
    if (lane < head) d[lane] = s[lane >> 1];
    const uint64_t nv = (n - head) >> 4;
    const uint32_t odd = (uint32_t)head & 1u;
    for (uint64_t i = lane; i < nv; i += 64) {
        const uint64_t k = head + 16 * i;
        const uint8_t* const q = s + (k >> 1);
        uint64_t v;
        __builtin_memcpy(&v, q, 8);
        uint32_t e0 = twice((uint32_t)v & 0xFFFFu), e1 = twice((uint32_t)(v >> 16) & 0xFFFFu), e2 = twice((uint32_t)(v >> 32) & 0xFFFFu),
                 e3 = twice((uint32_t)(v >> 48));
        if (odd) {                                  // bytes 1 .. 16 of the doubled run: the last one is the ninth source byte
            const uint32_t top = q[8];
            e0 = (e0 >> 8) | (e1 << 24); e1 = (e1 >> 8) | (e2 << 24); e2 = (e2 >> 8) | (e3 << 24); e3 = (e3 >> 8) | (top << 24);
        }
        *reinterpret_cast<uint4*>(d + k) = make_uint4(e0, e1, e2, e3);
    }
    const uint64_t t0 = head + (nv << 4);
    if (t0 + lane < n) d[t0 + lane] = s[(t0 + lane) >> 1];
}

__device__ __forceinline__ void put_sample(uint8_t* d, const uint8_t* s, uint32_t bps, bool wide)
{
    if (bps == 1) d[0] = s[0];
    else if (wide) *reinterpret_cast<uint16_t*>(d) = *reinterpret_cast<const uint16_t*>(s);
    else for (uint32_t b = 0; b < bps; ++b) d[b] = s[b];
}

__global__ __launch_bounds__(256) void t2dec_upsample_kernel(UpsampleArgs a)
{
    const uint32_t unit = blockIdx.z, comp = blockIdx.y, lane = threadIdx.x & 63u;
    const uint64_t cx0 = a.origins[2 * unit], cy0 = a.origins[2 * unit + 1];
    const uint64_t X1 = (uint64_t)a.x0 + a.img_w, Y1 = (uint64_t)a.y0 + a.img_h;
    const uint64_t src_row = (uint64_t)a.w * a.bps;
    const uint8_t* const s = a.tiles + ((uint64_t)unit * a.ncomp + comp) * a.h * src_row;
    // the unit's columns of the image: its samples' footprints (the host checked cx0 * dx >= x0 and the same for y)
    const uint64_t gxa = cx0 * a.dx - a.x0, n = min((cx0 + a.w) * a.dx, X1) - a.x0 - gxa;
    uint8_t* const d = a.image + (uint64_t)comp * a.img_plane + gxa * a.xstep;
    const bool planar = a.xstep == a.bps;
    // (2-byte samples go as one store where every address is even)
    const bool wide = a.bps == 2 && !(((uintptr_t)a.image | (uintptr_t)a.tiles | a.xstep | a.img_row | a.img_plane) & 1u);
    const uint32_t y1 = min(a.h, (blockIdx.x + 1) * kPlaceRows);
    for (uint32_t y = blockIdx.x * kPlaceRows + (threadIdx.x >> 6); y < y1; y += 4) {
        const uint8_t* const sr = s + y * src_row;
        const uint64_t gya = (cy0 + y) * a.dy - a.y0, gyb = min((cy0 + y + 1) * a.dy, Y1) - a.y0;
        for (uint64_t gy = gya; gy < gyb; ++gy) {
            uint8_t* const dr = d + gy * a.img_row;
            if (planar && a.dx == 1) wave_copy(dr, sr, n * a.bps, lane);
            else if (planar && a.dx == 2 && a.bps == 1) wave_double_bytes(dr, sr, n, lane);
            else
                for (uint64_t g = lane; g < n; g += 64) put_sample(dr + g * a.xstep, sr + (g / a.dx) * a.bps, a.bps, wide);
        }
    }
}

__global__ __launch_bounds__(256) void t2dec_fill_kernel(FillArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    const bool wide = a.bps == 2 && !(((uintptr_t)a.image | a.xstep | a.img_row) & 1u);
    const uint32_t y1 = min(a.h, (blockIdx.x + 1) * kPlaceRows);
    for (uint32_t y = blockIdx.x * kPlaceRows + (threadIdx.x >> 6); y < y1; y += 4) {
        uint8_t* const dr = a.image + ((uint64_t)a.y + y) * a.img_row + (uint64_t)a.x * a.xstep;
        for (uint32_t g = lane; g < a.w; g += 64) {
            uint8_t* const q = dr + g * a.xstep;
            if (wide) *reinterpret_cast<uint16_t*>(q) = (uint16_t)a.value;
            else for (uint32_t b = 0; b < a.bps; ++b) q[b] = (uint8_t)(a.value >> (8 * b));
        }
    }
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
    if (a.img_w > 0x7FFFFFFFu || a.img_h > 0x7FFFFFFFu) return hipErrorInvalidValue;          // (positions are signed 32-bit)
    hipLaunchKernelGGL(t2dec_place_kernel, dim3((a.h + kPlaceRows - 1) / kPlaceRows, a.ncomp, a.ntiles), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_t2dec_upsample(const UpsampleArgs& a, hipStream_t s)
{
    if (!a.nunits || !a.w || !a.h || !a.ncomp) return hipSuccess;
    hipLaunchKernelGGL(t2dec_upsample_kernel, dim3((a.h + kPlaceRows - 1) / kPlaceRows, a.ncomp, a.nunits), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_t2dec_fill(const FillArgs& a, hipStream_t s)
{
    if (!a.w || !a.h) return hipSuccess;
    hipLaunchKernelGGL(t2dec_fill_kernel, dim3((a.h + kPlaceRows - 1) / kPlaceRows), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_t2dec_or_status(unsigned int* into, const unsigned int* from, bool assign, hipStream_t s)
{
    hipLaunchKernelGGL(t2dec_or_status_kernel, dim3(1), dim3(1), 0, s, into, from, assign ? 1 : 0);
    return hipGetLastError();
}

} // namespace grk_amd
