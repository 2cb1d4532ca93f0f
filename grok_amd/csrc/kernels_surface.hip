// grok_amd/csrc/kernels_surface.hip -- units between a video surface (NV12, I420, NV16, P010 ...; include/grok_amd.h: grk_amd_surface)
// and the tight, component-major unit planes the tile coders take in batches (grk_amd_encode_surface / grk_amd_decode_surface, the
// staged route).  Both kernels are byte movers shaped like KP (kernels_t2dec.hip): a workgroup per (16-row band, component, unit), a
// wave per row.  A component's samples may sit above `shift` zero bits of their containers (P010: 6): KS reads word >> shift, KD
// writes v << shift; the unit planes are always LSB-aligned.
//   KS  cut    surface -> unit planes.  Step 1: a row copy (wave_copy.h), with a shift a row move of aligned 16-byte loads, eight
//              two-byte samples shifted, 16-byte stores; step 2 without a shift, one-byte samples (the chroma of NV12 / NV16):
//              de-interleaved from aligned 16-byte loads to 8-byte stores, head and tail by bytes; step 2, two-byte samples (the
//              chroma of P010 and 16-bit NV12), any shift: four samples out of each aligned 16-byte line, shifted, to one 8-byte
//              store, head and tail by samples; every other case (step 3 / 4, two-byte samples on odd addresses, one-byte samples
//              with a shift) goes sample by sample
//   KD  place  unit planes -> surface, writing no byte that is no sample of the components it places.  Step 1: a row copy, with a
//              shift the row move above with 16-byte stores on the destination's alignment; two partners of step 2 placed by one
//              launch: eight bytes of each plane (one-byte samples without a shift: eight samples, two-byte samples: four, each
//              shifted by its own component's count) merged into one aligned 16-byte store, head and tail by samples; a lone strided
//              component: stores of its own samples only
// The two-byte 16-byte forms are taken where every address involved is even (`wide`); otherwise samples go one by one, byte by byte.
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

// one sample from s to d: a cut (kPlace = false) drops the `sh` low bits of the surface's word, a placement puts them back as zeros
template <bool kPlace>
__device__ __forceinline__ uint32_t shifted(uint32_t v, uint32_t sh) { return kPlace ? v << sh : v >> sh; }

template <bool kPlace>
__device__ __forceinline__ void move_sample(uint8_t* d, const uint8_t* s, uint32_t bps, bool wide, uint32_t sh)
{
    if (bps == 1) d[0] = (uint8_t)shifted<kPlace>(s[0], sh);
    else if (wide) *reinterpret_cast<uint16_t*>(d) = (uint16_t)shifted<kPlace>(*reinterpret_cast<const uint16_t*>(s), sh);
    else {
        const uint32_t v = shifted<kPlace>(s[0] | (uint32_t)s[1] << 8, sh);
        d[0] = (uint8_t)v; d[1] = (uint8_t)(v >> 8);
    }
}

// both two-byte samples of a dword shifted, each inside its own half
template <bool kPlace>
__device__ __forceinline__ uint32_t shifted_pair(uint32_t v, uint32_t sh)
{
    return kPlace ? (v << sh) & (((0xFFFFu << sh) & 0xFFFFu) * 0x10001u) : (v >> sh) & ((0xFFFFu >> sh) * 0x10001u);
}

// w two-byte samples from s to d (both even addresses), each shifted, by one wave: 16-byte accesses of eight samples, aligned on the
// surface's side -- a cut's loads, a placement's stores --, head and tail by samples
template <bool kPlace>
__device__ __forceinline__ void wave_shift_row(uint8_t* d, const uint8_t* s, uint64_t w, uint32_t sh, uint32_t lane)
{
    const uintptr_t surf = kPlace ? (uintptr_t)d : (uintptr_t)s;
    const uint64_t head = min(w, (uint64_t)(((0 - surf) & 15u) >> 1));
    if (lane < head) move_sample<kPlace>(d + 2 * lane, s + 2 * lane, 2, true, sh);
    d += 2 * head; s += 2 * head; w -= head;
    const uint64_t nv = w >> 3;
    for (uint64_t i = lane; i < nv; i += 64) {
        U128 v;
        if (kPlace) __builtin_memcpy(&v, s + 16 * i, 16);
        else { const uint4 l = *reinterpret_cast<const uint4*>(s + 16 * i); v = U128{l.x, l.y, l.z, l.w}; }
        v.x = shifted_pair<kPlace>(v.x, sh); v.y = shifted_pair<kPlace>(v.y, sh);
        v.z = shifted_pair<kPlace>(v.z, sh); v.w = shifted_pair<kPlace>(v.w, sh);
        if (kPlace) *reinterpret_cast<uint4*>(d + 16 * i) = make_uint4(v.x, v.y, v.z, v.w);
        else __builtin_memcpy(d + 16 * i, &v, 16);
    }
    const uint64_t t0 = (nv << 3) + lane;
    if (t0 < w) move_sample<kPlace>(d + 2 * t0, s + 2 * t0, 2, true, sh);
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

// w two-byte samples at d, sample x = (the word at s + 4 x) >> sh, by one wave (both even addresses): 16-byte loads of the aligned
// lines that lie wholly inside the row's span [s, s + 4 w - 2), the four samples of each to one 8-byte store; what lies before the
// first line and behind the last by samples
__device__ __forceinline__ void wave_every_other_word(uint8_t* d, const uint8_t* s, uint64_t w, uint32_t sh, uint32_t lane)
{
    const uint64_t span = 4 * w - 2;
    const uint64_t before = min(span, (uint64_t)((0 - (uintptr_t)s) & 15u));
    const uint64_t hs = (before + 3) >> 2;                      // samples that start before the first line (at most 4)
    if (lane < hs) move_sample<false>(d + 2 * lane, s + 4 * lane, 2, true, sh);
    const uint32_t half = 8u * (uint32_t)(4 * hs - before) + sh; // a line's first sample is its bytes 0..1 or 2..3
    const uint32_t mask = 0xFFFFu >> sh;
    const uint64_t nv = (span - before) >> 4;
    for (uint64_t i = lane; i < nv; i += 64) {
        const uint4 v = *reinterpret_cast<const uint4*>(s + before + 16 * i);
        U64 o;
        o.x = ((v.x >> half) & mask) | (((v.y >> half) & mask) << 16);
        o.y = ((v.z >> half) & mask) | (((v.w >> half) & mask) << 16);
        __builtin_memcpy(d + 2 * (hs + 4 * i), &o, 8);
    }
    const uint64_t t0 = hs + 4 * nv + lane;                      // (fewer than 16 bytes are left: at most 4 samples)
    if (t0 < w) move_sample<false>(d + 2 * t0, s + 4 * t0, 2, true, sh);
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

// n = 2 w two-byte samples at d, sample k = (k odd ? hi : lo)[k >> 1] << (k odd ? sh_hi : sh_lo), by one wave (all even addresses):
// 16-byte stores on the destination's alignment, each from four samples of either plane, head and tail by samples
__device__ __forceinline__ void wave_merge_words(uint8_t* d, const uint8_t* lo, const uint8_t* hi, uint64_t n, uint32_t sh_lo, uint32_t sh_hi,
                                                 uint32_t lane)
{
    const uint64_t head = min(n, (uint64_t)(((0 - (uintptr_t)d) & 15u) >> 1));
    if (lane < head) move_sample<true>(d + 2 * lane, ((lane & 1u) ? hi : lo) + 2 * (lane >> 1), 2, true, (lane & 1u) ? sh_hi : sh_lo);
    const uint64_t nv = (n - head) >> 3;
    const bool odd = (head & 1u) != 0;
    // sample k is the first plane's, sample k + 1 the second's: a store that starts on an odd sample starts with `hi`
    const uint32_t sh_a = odd ? sh_hi : sh_lo, sh_b = odd ? sh_lo : sh_hi;
    for (uint64_t i = lane; i < nv; i += 64) {
        const uint64_t k = head + 8 * i;
        const uint8_t* const first = (odd ? hi : lo) + 2 * (k >> 1);
        const uint8_t* const second = odd ? lo + 2 * ((k >> 1) + 1) : hi + 2 * (k >> 1);
        U64 a, b;
        __builtin_memcpy(&a, first, 8);
        __builtin_memcpy(&b, second, 8);
        a.x = shifted_pair<true>(a.x, sh_a); a.y = shifted_pair<true>(a.y, sh_a);
        b.x = shifted_pair<true>(b.x, sh_b); b.y = shifted_pair<true>(b.y, sh_b);
        *reinterpret_cast<uint4*>(d + 2 * k) = make_uint4((a.x & 0xFFFFu) | (b.x << 16), (a.x >> 16) | (b.x & 0xFFFF0000u),
                                                          (a.y & 0xFFFFu) | (b.y << 16), (a.y >> 16) | (b.y & 0xFFFF0000u));
    }
    const uint64_t k = head + (nv << 3) + lane;
    if (k < n) move_sample<true>(d + 2 * k, ((k & 1u) ? hi : lo) + 2 * (k >> 1), 2, true, (k & 1u) ? sh_hi : sh_lo);
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
        if (c.step == 1 && !c.shift) wave_copy(tr, sr, row_bytes, lane);
        else if (c.step == 1 && wide) wave_shift_row<false>(tr, sr, a.w, c.shift, lane);
        else if (c.step == 2 && a.bps == 1 && !c.shift) wave_every_other_byte(tr, sr, a.w, lane);
        else if (c.step == 2 && wide) wave_every_other_word(tr, sr, a.w, c.shift, lane);
        else
            for (uint32_t x = lane; x < a.w; x += 64) move_sample<false>(tr + (uint64_t)x * a.bps, sr + x * xstep, a.bps, wide, c.shift);
    }
}

__global__ __launch_bounds__(256) void surface_place_kernel(SurfaceArgs a)
{
    const uint32_t unit = blockIdx.z, lane = threadIdx.x & 63u;
    const uint64_t row_bytes = (uint64_t)a.w * a.bps;
    const uint32_t y1 = min(a.h, (blockIdx.x + 1) * kSurfaceRows);
    const uint64_t ox = a.origins[2 * unit], oy = a.origins[2 * unit + 1];
    if (a.pair) {
        // the two partners' rows as one run of 2 w samples from the lower of the two addresses
        const uint32_t first = a.comp[0].offset < a.comp[1].offset ? 0u : 1u;
        const uint8_t* const lo = a.tiles + ((uint64_t)unit * 2 + first) * a.h * row_bytes;
        const uint8_t* const hi = a.tiles + ((uint64_t)unit * 2 + (first ^ 1u)) * a.h * row_bytes;
        uint8_t* const d = a.surface + a.comp[first].offset + oy * a.comp[first].row_pitch + ox * 2 * a.bps;
        for (uint32_t y = blockIdx.x * kSurfaceRows + (threadIdx.x >> 6); y < y1; y += 4) {
            uint8_t* const dr = d + y * a.comp[first].row_pitch;
            if (a.bps == 1) wave_merge_bytes(dr, lo + y * row_bytes, hi + y * row_bytes, 2 * (uint64_t)a.w, lane);
            else wave_merge_words(dr, lo + y * row_bytes, hi + y * row_bytes, 2 * (uint64_t)a.w, a.comp[first].shift, a.comp[first ^ 1u].shift, lane);
        }
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
        if (c.step == 1 && !c.shift) wave_copy(dr, tr, row_bytes, lane);
        else if (c.step == 1 && wide) wave_shift_row<true>(dr, tr, a.w, c.shift, lane);
        else
            for (uint32_t x = lane; x < a.w; x += 64) move_sample<true>(dr + x * xstep, tr + (uint64_t)x * a.bps, a.bps, wide, c.shift);
    }
}

static bool surface_args_ok(const SurfaceArgs& a)
{
    if (a.ncomp > 4 || a.nunits > 65535 || (a.bps != 1 && a.bps != 2)) return false;
    for (uint32_t k = 0; k < a.ncomp; ++k) if (a.comp[k].shift >= 8 * a.bps) return false;
    return true;
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
    // (one-byte partners without a shift; two-byte partners where every address is even)
    const bool forms = a.bps == 1 ? !p.shift && !q.shift : !(((uintptr_t)a.surface | (uintptr_t)a.tiles | p.offset | p.row_pitch | q.offset | q.row_pitch) & 1u);
    a.pair = a.ncomp == 2 && forms && p.step == 2 && q.step == 2 && p.row_pitch == q.row_pitch &&
             (p.offset + a.bps == q.offset || q.offset + a.bps == p.offset) ? 1u : 0u;
    hipLaunchKernelGGL(surface_place_kernel, dim3((a.h + kSurfaceRows - 1) / kSurfaceRows, a.pair ? 1u : a.ncomp, a.nunits), dim3(256), 0, s, a);
    return hipGetLastError();
}

} // namespace grk_amd
