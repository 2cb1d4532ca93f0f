// grok_amd/csrc/kernels_packed.hip -- a packed 4:2:2 frame (packed_format.h: YUY2, UYVY, YVYU, Y216, v210) and its three tight,
// LSB-aligned planes Y, Cb, Cr (grk_amd_encode_packed / grk_amd_decode_packed and the two kernels as calls of their own).  Byte movers
// shaped like KS / KD (kernels_surface.hip): a workgroup per 16-row band, a wave per row; no LDS, no barrier, no cross-lane operation.
//   KU  unpack  frame -> planes.  Every packed byte is read once: the row's interior by aligned 16-byte loads, a lane taking two
//               lines (eight one-byte macropixels: 16 Y + 8 Cb + 8 Cr bytes; four two-byte macropixels: 8 Y + 4 Cb + 4 Cr samples)
//               or four v210 blocks (24 Y + 12 Cb + 12 Cr samples) so that every plane store is 8 or 16 bytes; the Y216 shift and
//               the v210 fields are taken apart in registers
//   KK  pack    planes -> frame, writing no byte that is no sample (v210: no byte outside a block that holds one): the same shares
//               per lane the other way, 16-byte stores on the frame's alignment, the planes read by unaligned 8- and 16-byte loads
// Macropixels before the first aligned line of a row, behind its last whole share, the half macropixel of an odd width and rows
// whose macropixels do not lie on multiples of their size go macropixel by macropixel (v210: block by block, a block being one
// aligned 16-byte access either way, fields past the width read as nothing and written as zero).
// The host checked format, precision, alignment and every size (packed.cpp): the kernels trust their bounds.
#include "kernels.h"
#include "packed_format.h"
#include "wave_copy.h"

namespace grk_amd {

constexpr uint32_t kPackedRows = 16;        // rows per workgroup: four per wave

struct __attribute__((packed, aligned(1))) U64 { uint32_t x, y; };

// b0 | b1 << 8  ->  b0 | b1 << 16
__device__ __forceinline__ uint32_t spread(uint32_t v) { return (v & 0xFFu) | ((v & 0xFF00u) << 8); }
// bytes 0 and 2 of v  ->  b0 | b2 << 8
__device__ __forceinline__ uint32_t evens(uint32_t v) { return (v & 0xFFu) | ((v >> 8) & 0xFF00u); }
// two-byte sample k of the dwords at d
__device__ __forceinline__ uint32_t half_of(const uint32_t* d, uint32_t k) { return (d[k >> 1] >> (16u * (k & 1u))) & 0xFFFFu; }

// sample i of a plane of `bps`-byte samples at any address
__device__ __forceinline__ uint32_t plane_get(const uint8_t* p, uint64_t i, uint32_t bps)
{
    if (bps == 1) return p[i];
    uint16_t v;
    __builtin_memcpy(&v, p + 2 * i, 2);
    return v;
}
__device__ __forceinline__ void plane_put(uint8_t* p, uint64_t i, uint32_t bps, uint32_t v)
{
    if (bps == 1) { p[i] = (uint8_t)v; return; }
    const uint16_t s = (uint16_t)v;
    __builtin_memcpy(p + 2 * i, &s, 2);
}

__device__ __forceinline__ void load_lines(uint32_t* d, const uint8_t* p, uint32_t lines)
{
    for (uint32_t k = 0; k < lines; ++k) {
        const uint4 v = *reinterpret_cast<const uint4*>(p + 16 * k);
        d[4 * k] = v.x; d[4 * k + 1] = v.y; d[4 * k + 2] = v.z; d[4 * k + 3] = v.w;
    }
}
__device__ __forceinline__ void store_lines(uint8_t* p, const uint32_t* d, uint32_t lines)
{
    for (uint32_t k = 0; k < lines; ++k) *reinterpret_cast<uint4*>(p + 16 * k) = make_uint4(d[4 * k], d[4 * k + 1], d[4 * k + 2], d[4 * k + 3]);
}
// 16 / 8 bytes at any address from / to dwords
__device__ __forceinline__ void get16(uint32_t* d, const uint8_t* p) { U128 v; __builtin_memcpy(&v, p, 16); d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w; }
__device__ __forceinline__ void get8(uint32_t* d, const uint8_t* p) { U64 v; __builtin_memcpy(&v, p, 8); d[0] = v.x; d[1] = v.y; }
__device__ __forceinline__ void put16(uint8_t* p, const uint32_t* d) { const U128 v{d[0], d[1], d[2], d[3]}; __builtin_memcpy(p, &v, 16); }
__device__ __forceinline__ void put8(uint8_t* p, const uint32_t* d) { const U64 v{d[0], d[1]}; __builtin_memcpy(p, &v, 8); }

// one row: the frame's bytes and the three planes' samples of that row
struct PackedRow { uint8_t *p, *y, *cb, *cr; uint32_t w, cw; };

// ---- one-byte macropixels: YUY2, UYVY, YVYU ------------------------------------------------------------------------------------
// macropixels [m0, m1) of a row by one wave, byte by byte; Y1 of an odd width's last macropixel is neither read nor written
template <uint32_t F, bool kPack>
__device__ __forceinline__ void wave_byte_macropixels(const PackedRow& r, uint64_t m0, uint64_t m1, uint32_t lane)
{
    constexpr uint32_t ya = packed_y_at(F), ua = packed_cb_at(F), va = packed_cr_at(F);
    for (uint64_t m = m0 + lane; m < m1; m += 64) {
        uint8_t* const p = r.p + 4 * m;
        const bool two = 2 * m + 1 < r.w;
        if (kPack) {
            p[ya] = r.y[2 * m]; if (two) p[ya + 2] = r.y[2 * m + 1];
            p[ua] = r.cb[m]; p[va] = r.cr[m];
        } else {
            r.y[2 * m] = p[ya]; if (two) r.y[2 * m + 1] = p[ya + 2];
            r.cb[m] = p[ua]; r.cr[m] = p[va];
        }
    }
}

// eight whole macropixels from macropixel m, two aligned lines: 16 Y, 8 Cb, 8 Cr
template <uint32_t F, bool kPack>
__device__ __forceinline__ void lane_byte_share(const PackedRow& r, uint64_t m)
{
    constexpr uint32_t ys = 8 * packed_y_at(F), us = 8 * packed_cb_at(F), vs = 8 * packed_cr_at(F);
    uint32_t d[8], y[4], u[2], v[2];
    if (kPack) {
        get16(y, r.y + 2 * m); get8(u, r.cb + m); get8(v, r.cr + m);
#pragma unroll
        for (uint32_t k = 0; k < 8; ++k)
            d[k] = (spread(half_of(y, k)) << ys) | (((u[k >> 2] >> (8 * (k & 3))) & 0xFFu) << us) | (((v[k >> 2] >> (8 * (k & 3))) & 0xFFu) << vs);
        store_lines(r.p + 4 * m, d, 2);
    } else {
        load_lines(d, r.p + 4 * m, 2);
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) y[k] = evens(d[2 * k] >> ys) | (evens(d[2 * k + 1] >> ys) << 16);
#pragma unroll
        for (uint32_t k = 0; k < 2; ++k) {
            u[k] = ((d[4 * k] >> us) & 0xFFu) | (((d[4 * k + 1] >> us) & 0xFFu) << 8) | (((d[4 * k + 2] >> us) & 0xFFu) << 16) | (((d[4 * k + 3] >> us) & 0xFFu) << 24);
            v[k] = ((d[4 * k] >> vs) & 0xFFu) | (((d[4 * k + 1] >> vs) & 0xFFu) << 8) | (((d[4 * k + 2] >> vs) & 0xFFu) << 16) | (((d[4 * k + 3] >> vs) & 0xFFu) << 24);
        }
        put16(r.y + 2 * m, y); put8(r.cb + m, u); put8(r.cr + m, v);
    }
}

template <uint32_t F, bool kPack>
__device__ __forceinline__ void wave_byte_row(const PackedRow& r, uint32_t lane)
{
    // (a row whose macropixels are no aligned dwords: nothing of it is a line of whole macropixels)
    if ((uintptr_t)r.p & 3u) { wave_byte_macropixels<F, kPack>(r, 0, r.cw, lane); return; }
    const uint64_t whole = r.w >> 1;
    const uint64_t head = min(whole, (uint64_t)(((0 - (uintptr_t)r.p) & 15u) >> 2));
    wave_byte_macropixels<F, kPack>(r, 0, head, lane);
    const uint64_t nv = (whole - head) >> 3;
    for (uint64_t i = lane; i < nv; i += 64) lane_byte_share<F, kPack>(r, head + 8 * i);
    wave_byte_macropixels<F, kPack>(r, head + 8 * nv, r.cw, lane);
}

// ---- Y216: four 16-bit words per macropixel, v << sh ----------------------------------------------------------------------------
template <bool kPack>
__device__ __forceinline__ void wave_word_macropixels(const PackedRow& r, uint64_t m0, uint64_t m1, uint32_t sh, uint32_t lane)
{
    for (uint64_t m = m0 + lane; m < m1; m += 64) {
        uint16_t* const p = reinterpret_cast<uint16_t*>(r.p + 8 * m);           // (base and pitch are even)
        const bool two = 2 * m + 1 < r.w;
        if (kPack) {
            p[0] = (uint16_t)(plane_get(r.y, 2 * m, 2) << sh); if (two) p[2] = (uint16_t)(plane_get(r.y, 2 * m + 1, 2) << sh);
            p[1] = (uint16_t)(plane_get(r.cb, m, 2) << sh); p[3] = (uint16_t)(plane_get(r.cr, m, 2) << sh);
        } else {
            plane_put(r.y, 2 * m, 2, (uint32_t)p[0] >> sh); if (two) plane_put(r.y, 2 * m + 1, 2, (uint32_t)p[2] >> sh);
            plane_put(r.cb, m, 2, (uint32_t)p[1] >> sh); plane_put(r.cr, m, 2, (uint32_t)p[3] >> sh);
        }
    }
}

// four whole macropixels from macropixel m, two aligned lines: 8 Y, 4 Cb, 4 Cr
template <bool kPack>
__device__ __forceinline__ void lane_word_share(const PackedRow& r, uint64_t m, uint32_t sh)
{
    uint32_t d[8], y[4], u[2], v[2];
    if (kPack) {
        get16(y, r.y + 4 * m); get8(u, r.cb + 2 * m); get8(v, r.cr + 2 * m);
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            d[2 * k] = ((half_of(y, 2 * k) << sh) & 0xFFFFu) | ((half_of(u, k) << sh) << 16);
            d[2 * k + 1] = ((half_of(y, 2 * k + 1) << sh) & 0xFFFFu) | ((half_of(v, k) << sh) << 16);
        }
        store_lines(r.p + 8 * m, d, 2);
    } else {
        load_lines(d, r.p + 8 * m, 2);
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) y[k] = ((d[2 * k] & 0xFFFFu) >> sh) | (((d[2 * k + 1] & 0xFFFFu) >> sh) << 16);
#pragma unroll
        for (uint32_t k = 0; k < 2; ++k) {
            u[k] = (d[4 * k] >> 16 >> sh) | ((d[4 * k + 2] >> 16 >> sh) << 16);
            v[k] = (d[4 * k + 1] >> 16 >> sh) | ((d[4 * k + 3] >> 16 >> sh) << 16);
        }
        put16(r.y + 4 * m, y); put8(r.cb + 2 * m, u); put8(r.cr + 2 * m, v);
    }
}

template <bool kPack>
__device__ __forceinline__ void wave_word_row(const PackedRow& r, uint32_t sh, uint32_t lane)
{
    if ((uintptr_t)r.p & 7u) { wave_word_macropixels<kPack>(r, 0, r.cw, sh, lane); return; }
    const uint64_t whole = r.w >> 1;
    const uint64_t head = min(whole, (uint64_t)(((0 - (uintptr_t)r.p) & 15u) >> 3));
    wave_word_macropixels<kPack>(r, 0, head, sh, lane);
    const uint64_t nv = (whole - head) >> 2;
    for (uint64_t i = lane; i < nv; i += 64) lane_word_share<kPack>(r, head + 4 * i, sh);
    wave_word_macropixels<kPack>(r, head + 4 * nv, r.cw, sh, lane);
}

// ---- v210: 16-byte blocks of 6 Y, 3 Cb, 3 Cr in 10-bit fields -------------------------------------------------------------------
// a block's four dwords <-> its samples
__device__ __forceinline__ void block_fields(const uint32_t* w, uint32_t* y, uint32_t* u, uint32_t* v)
{
    const uint32_t m = 0x3FFu;
    u[0] = w[0] & m; y[0] = (w[0] >> 10) & m; v[0] = (w[0] >> 20) & m;
    y[1] = w[1] & m; u[1] = (w[1] >> 10) & m; y[2] = (w[1] >> 20) & m;
    v[1] = w[2] & m; y[3] = (w[2] >> 10) & m; u[2] = (w[2] >> 20) & m;
    y[4] = w[3] & m; v[2] = (w[3] >> 10) & m; y[5] = (w[3] >> 20) & m;
}
__device__ __forceinline__ void block_words(uint32_t* w, const uint32_t* y, const uint32_t* u, const uint32_t* v)
{
    const uint32_t m = 0x3FFu;
    w[0] = (u[0] & m) | ((y[0] & m) << 10) | ((v[0] & m) << 20);
    w[1] = (y[1] & m) | ((u[1] & m) << 10) | ((y[2] & m) << 20);
    w[2] = (v[1] & m) | ((y[3] & m) << 10) | ((u[2] & m) << 20);
    w[3] = (y[4] & m) | ((v[2] & m) << 10) | ((y[5] & m) << 20);
}

// blocks [b0, b1) of a row by one wave, a block per lane: the samples inside the width only, the block itself whole
template <bool kPack>
__device__ __forceinline__ void wave_v210_blocks(const PackedRow& r, uint64_t b0, uint64_t b1, uint32_t lane)
{
    for (uint64_t b = b0 + lane; b < b1; b += 64) {
        uint32_t w[4], y[6], u[3], v[3];
        if (kPack) {
#pragma unroll
            for (uint32_t k = 0; k < 6; ++k) y[k] = 6 * b + k < r.w ? plane_get(r.y, 6 * b + k, 2) : 0u;
#pragma unroll
            for (uint32_t k = 0; k < 3; ++k) {
                u[k] = 3 * b + k < r.cw ? plane_get(r.cb, 3 * b + k, 2) : 0u;
                v[k] = 3 * b + k < r.cw ? plane_get(r.cr, 3 * b + k, 2) : 0u;
            }
            block_words(w, y, u, v);
            store_lines(r.p + 16 * b, w, 1);
        } else {
            load_lines(w, r.p + 16 * b, 1);
            block_fields(w, y, u, v);
#pragma unroll
            for (uint32_t k = 0; k < 6; ++k) if (6 * b + k < r.w) plane_put(r.y, 6 * b + k, 2, y[k]);
#pragma unroll
            for (uint32_t k = 0; k < 3; ++k)
                if (3 * b + k < r.cw) { plane_put(r.cb, 3 * b + k, 2, u[k]); plane_put(r.cr, 3 * b + k, 2, v[k]); }
        }
    }
}

// four whole blocks from block b: 24 Y (three 16-byte accesses of the plane), 12 Cb and 12 Cr (16 + 8 bytes each)
template <bool kPack>
__device__ __forceinline__ void lane_v210_share(const PackedRow& r, uint64_t b)
{
    uint32_t w[16], y[24], u[12], v[12], yd[12], ud[6], vd[6];
    uint8_t* const py = r.y + 12 * b;            // sample 6 b, two bytes each
    uint8_t* const pu = r.cb + 6 * b;
    uint8_t* const pv = r.cr + 6 * b;
    if (kPack) {
        get16(yd, py); get16(yd + 4, py + 16); get16(yd + 8, py + 32);
        get16(ud, pu); get8(ud + 4, pu + 16);
        get16(vd, pv); get8(vd + 4, pv + 16);
#pragma unroll
        for (uint32_t k = 0; k < 24; ++k) y[k] = half_of(yd, k);
#pragma unroll
        for (uint32_t k = 0; k < 12; ++k) { u[k] = half_of(ud, k); v[k] = half_of(vd, k); }
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) block_words(w + 4 * k, y + 6 * k, u + 3 * k, v + 3 * k);
        store_lines(r.p + 16 * b, w, 4);
    } else {
        load_lines(w, r.p + 16 * b, 4);
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) block_fields(w + 4 * k, y + 6 * k, u + 3 * k, v + 3 * k);
#pragma unroll
        for (uint32_t k = 0; k < 12; ++k) yd[k] = y[2 * k] | (y[2 * k + 1] << 16);
#pragma unroll
        for (uint32_t k = 0; k < 6; ++k) { ud[k] = u[2 * k] | (u[2 * k + 1] << 16); vd[k] = v[2 * k] | (v[2 * k + 1] << 16); }
        put16(py, yd); put16(py + 16, yd + 4); put16(py + 32, yd + 8);
        put16(pu, ud); put8(pu + 16, ud + 4);
        put16(pv, vd); put8(pv + 16, vd + 4);
    }
}

template <bool kPack>
__device__ __forceinline__ void wave_v210_row(const PackedRow& r, uint32_t lane)
{
    const uint64_t nv = (r.w / 6u) >> 2;         // shares of four blocks whose every field is a sample
    for (uint64_t i = lane; i < nv; i += 64) lane_v210_share<kPack>(r, 4 * i);
    wave_v210_blocks<kPack>(r, 4 * nv, ((uint64_t)r.w + 5) / 6, lane);
}

template <bool kPack>
__device__ __forceinline__ void packed_rows(const PackedArgs& a)
{
    const uint32_t lane = threadIdx.x & 63u, bps = a.prec <= 8 ? 1u : 2u, cw = (a.w + 1) >> 1;
    const uint64_t y1 = min((uint64_t)a.h, ((uint64_t)blockIdx.x + 1) * kPackedRows);
    for (uint64_t y = (uint64_t)blockIdx.x * kPackedRows + (threadIdx.x >> 6); y < y1; y += 4) {
        const PackedRow r{a.packed + y * a.pitch, a.y + y * a.w * bps, a.cb + y * cw * bps, a.cr + y * cw * bps, a.w, cw};
        switch (a.format) {
        case kPackedYUY2: wave_byte_row<kPackedYUY2, kPack>(r, lane); break;
        case kPackedUYVY: wave_byte_row<kPackedUYVY, kPack>(r, lane); break;
        case kPackedYVYU: wave_byte_row<kPackedYVYU, kPack>(r, lane); break;
        case kPackedY216: wave_word_row<kPack>(r, 16u - a.prec, lane); break;
        default: wave_v210_row<kPack>(r, lane); break;
        }
    }
}

__global__ __launch_bounds__(256) void packed_unpack_kernel(PackedArgs a) { packed_rows<false>(a); }
__global__ __launch_bounds__(256) void packed_pack_kernel(PackedArgs a) { packed_rows<true>(a); }

// what the kernels trust: a known format at its precision, the frame on the format's alignment, rows that do not overlap
static bool packed_args_ok(const PackedArgs& a)
{
    if (a.format >= kPackedFormats || !packed_prec_ok(a.format, a.prec)) return false;
    if (((uintptr_t)a.packed | a.pitch) % packed_align(a.format)) return false;
    return a.h <= 1 || a.pitch >= packed_row_bytes(a.format, a.w);
}

hipError_t launch_packed_unpack(const PackedArgs& a, hipStream_t s)
{
    if (!a.w || !a.h) return hipSuccess;
    if (!packed_args_ok(a)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(packed_unpack_kernel, dim3((a.h + kPackedRows - 1) / kPackedRows), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_packed_pack(const PackedArgs& a, hipStream_t s)
{
    if (!a.w || !a.h) return hipSuccess;
    if (!packed_args_ok(a)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(packed_pack_kernel, dim3((a.h + kPackedRows - 1) / kPackedRows), dim3(256), 0, s, a);
    return hipGetLastError();
}

} // namespace grk_amd
