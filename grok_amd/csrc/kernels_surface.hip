// grok_amd/csrc/kernels_surface.hip -- units between a video surface (NV12, I420, NV16 ...; include/grok_amd.h: grk_amd_surface) and
// the tight, component-major unit planes the tile coders take in batches (grk_amd_encode_surface / grk_amd_decode_surface, the staged
// route).  Both kernels are byte movers shaped like KP (kernels_t2dec.hip): a workgroup per (16-row band, component, unit), a wave
// per row.
//   KS  cut    surface -> unit planes.  A component with step 1 is a row copy (wave_copy.h); one-byte samples of step 2 (the chroma
//              of NV12 / NV16) are de-interleaved from aligned 16-byte loads to 8-byte stores, head and tail by bytes; every other
//              case (step 3 / 4, two-byte samples with a step) goes sample by sample
//   KD  place  unit planes -> surface, writing no byte that is no sample of the components it places.  Step 1: a row copy; two
//              one-byte partners of step 2 placed by one launch: eight bytes of each plane merged into one aligned 16-byte store,
//              head and tail by bytes; a lone strided component: stores of its own samples only
// The host checked every sample against the surface's size (surface.cpp): the kernels trust their bounds.
#include "kernels.h"
#include "wave_copy.h"

namespace grk_amd {

constexpr uint32_t kSurfaceRows = 16;       // rows of a unit's component per workgroup: four per wave

struct __attribute__((packed, aligned(1))) U64 { uint32_t x, y; };

// b0 | b1 << 8  ->  b0 | b1 << 16
__device__ __forceinline__ uint32_t spread(uint32_t v) { return (v & 0xFFu) | ((v & 0xFF00u) << 8); }
// bytes 0 and 2 of v  ->  b0 | b2 << 8
__device__ __forceinline__ uint32_t evens(uint32_t v) { return (v & 0xFFu) | ((v >> 8) & 0xFF00u); }

__device__ __forceinline__ void move_sample(uint8_t* d, const uint8_t* s, uint32_t bps, bool wide)
{
    if (bps == 1) d[0] = s[0];
    else if (wide) *reinterpret_cast<uint16_t*>(d) = *reinterpret_cast<const uint16_t*>(s);
    else { d[0] = s[0]; d[1] = s[1]; }
}

// w bytes at d, byte x = s[2 x], by one wave: 16-byte loads of the aligned lines that lie wholly inside the row's span [s, s + 2 w - 1),
// eight samples of each to one 8-byte store; what lies before the first line and behind the last by bytes
__device__ __forceinline__ void wave_every_other_byte(uint8_t* d, const uint8_t* s, uint64_t w, uint32_t lane)
{
    const uint64_t span = 2 * w - 1;
    const uint64_t before = min(span, (uint64_t)((0 - (uintptr_t)s) & 15u));
    const uint64_t hs = (before + 1) >> 1;                      // samples that start before the first line (at most 8)
    if (lane < hs) d[lane] = s[2 * lane];
    const uint32_t shift = 8u * (uint32_t)(2 * hs - before);    // a line's first sample is its byte 0 or 1
    const uint64_t nv = (span - before) >> 4;
    for (uint64_t i = lane; i < nv; i += 64) {
        const uint4 v = *reinterpret_cast<const uint4*>(s + before + 16 * i);
        U64 o;
        o.x = evens(v.x >> shift) | (evens(v.y >> shift) << 16);
        o.y = evens(v.z >> shift) | (evens(v.w >> shift) << 16);
        __builtin_memcpy(d + hs + 8 * i, &o, 8);
    }
    const uint64_t t0 = hs + 8 * nv;                             // (fewer than 16 bytes are left: at most 8 samples)
    if (t0 + lane < w) d[t0 + lane] = s[2 * (t0 + lane)];
}

// n = 2 w bytes at d, byte k = (k odd ? hi : lo)[k >> 1], by one wave: 16-byte stores on the destination's alignment, each from eight
// bytes of either plane, head and tail by bytes
__device__ __forceinline__ void wave_merge_bytes(uint8_t* d, const uint8_t* lo, const uint8_t* hi, uint64_t n, uint32_t lane)
{
    const uint64_t head = min(n, (uint64_t)((0 - (uintptr_t)d) & 15u));
    if (lane < head) d[lane] = (lane & 1u) ? hi[lane >> 1] : lo[lane >> 1];
    const uint64_t nv = (n - head) >> 4;
    const bool odd = (head & 1u) != 0;
    for (uint64_t i = lane; i < nv; i += 64) {
        const uint64_t k = head + 16 * i;
        // byte k is the first plane's, byte k + 1 the second's: a store that starts on an odd byte starts with `hi`
        const uint8_t* const first = (odd ? hi : lo) + (k >> 1);
        const uint8_t* const second = odd ? lo + (k >> 1) + 1 : hi + (k >> 1);
        uint64_t a, b;
        __builtin_memcpy(&a, first, 8);
        __builtin_memcpy(&b, second, 8);
        const uint32_t e0 = spread((uint32_t)a & 0xFFFFu) | (spread((uint32_t)b & 0xFFFFu) << 8);
        const uint32_t e1 = spread((uint32_t)(a >> 16) & 0xFFFFu) | (spread((uint32_t)(b >> 16) & 0xFFFFu) << 8);
        const uint32_t e2 = spread((uint32_t)(a >> 32) & 0xFFFFu) | (spread((uint32_t)(b >> 32) & 0xFFFFu) << 8);
        const uint32_t e3 = spread((uint32_t)(a >> 48)) | (spread((uint32_t)(b >> 48)) << 8);
        *reinterpret_cast<uint4*>(d + k) = make_uint4(e0, e1, e2, e3);
    }
    const uint64_t k = head + (nv << 4) + lane;
    if (k < n) d[k] = (k & 1u) ? hi[k >> 1] : lo[k >> 1];
}

__global__ __launch_bounds__(256) void surface_cut_kernel(SurfaceArgs a)
{
    const uint32_t unit = blockIdx.z, comp = blockIdx.y, lane = threadIdx.x & 63u;
    const SurfaceKernelComp c = a.comp[comp];
    const uint64_t row_bytes = (uint64_t)a.w * a.bps, xstep = (uint64_t)c.step * a.bps;
    uint8_t* const t = a.tiles + ((uint64_t)unit * a.ncomp + comp) * a.h * row_bytes;
    const uint8_t* const s = a.surface + c.offset + (uint64_t)a.origins[2 * unit + 1] * c.row_pitch + (uint64_t)a.origins[2 * unit] * xstep;
    // (2-byte samples go as one access where every address is even)
    const bool wide = a.bps == 2 && !(((uintptr_t)a.surface | (uintptr_t)a.tiles | c.offset | c.row_pitch) & 1u);
    const uint32_t y1 = min(a.h, (blockIdx.x + 1) * kSurfaceRows);
    for (uint32_t y = blockIdx.x * kSurfaceRows + (threadIdx.x >> 6); y < y1; y += 4) {
        const uint8_t* const sr = s + y * c.row_pitch;
        uint8_t* const tr = t + y * row_bytes;
        if (c.step == 1) wave_copy(tr, sr, row_bytes, lane);
        else if (c.step == 2 && a.bps == 1) wave_every_other_byte(tr, sr, a.w, lane);
        else
            for (uint32_t x = lane; x < a.w; x += 64) move_sample(tr + (uint64_t)x * a.bps, sr + x * xstep, a.bps, wide);
    }
}

__global__ __launch_bounds__(256) void surface_place_kernel(SurfaceArgs a)
{
    const uint32_t unit = blockIdx.z, lane = threadIdx.x & 63u;
    const uint64_t row_bytes = (uint64_t)a.w * a.bps;
    const uint32_t y1 = min(a.h, (blockIdx.x + 1) * kSurfaceRows);
    const uint64_t ox = a.origins[2 * unit], oy = a.origins[2 * unit + 1];
    if (a.pair) {
        // the two partners' rows as one run of 2 w bytes from the lower of the two addresses
        const uint32_t first = a.comp[0].offset < a.comp[1].offset ? 0u : 1u;
        const uint8_t* const lo = a.tiles + ((uint64_t)unit * 2 + first) * a.h * row_bytes;
        const uint8_t* const hi = a.tiles + ((uint64_t)unit * 2 + (first ^ 1u)) * a.h * row_bytes;
        uint8_t* const d = a.surface + a.comp[first].offset + oy * a.comp[first].row_pitch + ox * 2;
        for (uint32_t y = blockIdx.x * kSurfaceRows + (threadIdx.x >> 6); y < y1; y += 4)
            wave_merge_bytes(d + y * a.comp[first].row_pitch, lo + y * row_bytes, hi + y * row_bytes, 2 * (uint64_t)a.w, lane);
        return;
    }
    const uint32_t comp = blockIdx.y;
    const SurfaceKernelComp c = a.comp[comp];
    const uint64_t xstep = (uint64_t)c.step * a.bps;
    const uint8_t* const t = a.tiles + ((uint64_t)unit * a.ncomp + comp) * a.h * row_bytes;
    uint8_t* const d = a.surface + c.offset + oy * c.row_pitch + ox * xstep;
    const bool wide = a.bps == 2 && !(((uintptr_t)a.surface | (uintptr_t)a.tiles | c.offset | c.row_pitch) & 1u);
    for (uint32_t y = blockIdx.x * kSurfaceRows + (threadIdx.x >> 6); y < y1; y += 4) {
        const uint8_t* const tr = t + y * row_bytes;
        uint8_t* const dr = d + y * c.row_pitch;
        if (c.step == 1) wave_copy(dr, tr, row_bytes, lane);
        else
            for (uint32_t x = lane; x < a.w; x += 64) move_sample(dr + x * xstep, tr + (uint64_t)x * a.bps, a.bps, wide);
    }
}

static bool surface_args_ok(const SurfaceArgs& a)
{
    return a.ncomp <= 4 && a.nunits <= 65535 && (a.bps == 1 || a.bps == 2);
}

hipError_t launch_surface_cut(const SurfaceArgs& a, hipStream_t s)
{
    if (!a.nunits || !a.w || !a.h || !a.ncomp) return hipSuccess;
    if (!surface_args_ok(a)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(surface_cut_kernel, dim3((a.h + kSurfaceRows - 1) / kSurfaceRows, a.ncomp, a.nunits), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_surface_place(const SurfaceArgs& a0, hipStream_t s)
{
    if (!a0.nunits || !a0.w || !a0.h || !a0.ncomp) return hipSuccess;
    if (!surface_args_ok(a0)) return hipErrorInvalidValue;
    SurfaceArgs a = a0;
    const SurfaceKernelComp &p = a.comp[0], &q = a.comp[1];
    a.pair = a.ncomp == 2 && a.bps == 1 && p.step == 2 && q.step == 2 && p.row_pitch == q.row_pitch &&
             (p.offset + 1 == q.offset || q.offset + 1 == p.offset) ? 1u : 0u;
    hipLaunchKernelGGL(surface_place_kernel, dim3((a.h + kSurfaceRows - 1) / kSurfaceRows, a.pair ? 1u : a.ncomp, a.nunits), dim3(256), 0, s, a);
    return hipGetLastError();
}

} // namespace grk_amd
