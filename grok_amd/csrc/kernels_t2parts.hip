// grok_amd/csrc/kernels_t2parts.hip -- Tier-2 on the device for tiles divided into tile-parts (T.800 A.4.2; GRK_AMD_CS_TP).
//
// A packet's bytes do not depend on where tile-parts start: KT1 (kernels_t2.hip) is used as it is.  What changes is the frames -- up
// to 255 per tile, each SOT (TPsot, TNsot, Psot), the PLT marker segments of the part's OWN packets, SOD -- and where everything
// goes.  KT1b walks a tile's packets with one lane; here the packets of a part are spread over a wavefront, and the steps that need
// each other's results are launches of their own (no workgroup waits for another inside a kernel):
//   KT1p t2_part_frame_kernel   one wavefront per (part, tile): the part's frame, its length, the part's length
//   KT1q t2_part_place_kernel   one workgroup: a prefix sum over the (tile, part) lengths in file order -- every part's place, every
//                               tile's span (its parts lie one behind the other), the call's total
//   KT1r t2_part_packet_kernel  one wavefront per (part, tile): where every packet of the part goes, by a scan behind the frame
//   KT2p t2_gather_parts_kernel KT2 (kernels_t2.hip) with ntiles x nparts frame items
// The arithmetic of a frame is t2_parts.h's, which the host writer and tests/c/t2_parts_writer_units.cpp share.
#include "kernels.h"
#include "t2_parts.h"
#include "wave_copy.h"

namespace grk_amd {
namespace {

__device__ __forceinline__ uint64_t wave_sum64(uint64_t v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// inclusive scan over the wave's lanes
__device__ __forceinline__ uint64_t wave_scan64(uint64_t v, uint32_t lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t o = __shfl_up(v, d, 64);
        if ((int)lane >= d) v += o;
    }
    return v;
}

// a packet's bytes in the file; one beyond 32 bits (the part is then beyond 4 GB: status bit 3) is entered as 2^32 - 1, so that no
// entry is longer than the five bytes the frame's room was sized for
__device__ __forceinline__ uint64_t packet_bytes(const T2PartsArgs& a, const uint32_t* hl, const uint64_t* bl, uint32_t i)
{
    return (uint64_t)a.extra + hl[i] + bl[i];
}
__device__ __forceinline__ uint64_t entry_value(uint64_t v) { return v >> 32 ? 0xFFFFFFFFull : v; }

} // namespace

__global__ __launch_bounds__(64) void t2_part_frame_kernel(T2PartsArgs a)
{
    const uint32_t lane = threadIdx.x, k = blockIdx.x, t = blockIdx.y;
    const T2Part P = a.parts[k];
    uint8_t* const f = a.lit + (size_t)t * a.lit_stride + P.frame_at;
    const uint32_t* const hl = a.pk_hdr + (size_t)t * a.npackets + P.first;
    const uint64_t* const bl = a.pk_body + (size_t)t * a.npackets + P.first;
    // the part's body and the bytes of its PLT entries
    uint64_t body = 0, eb = 0;
    for (uint32_t i = lane; i < P.count; i += 64) {
        const uint64_t v = packet_bytes(a, hl, bl, i);
        body += v;
        eb += plt_entry_bytes(entry_value(v));
    }
    body = wave_sum64(body);
    eb = wave_sum64(eb);
    uint32_t pos = 12;
    bool bad = false;
    if (a.plt && P.count) {
        if (eb <= kPltSegEntryBytes) {
            // one marker segment: an exclusive scan places every entry, the lanes write them side by side
            uint64_t carry = 0;
            for (uint32_t base = 0; base < P.count; base += 64) {
                const uint32_t i = base + lane;
                uint64_t v = 0;
                uint32_t n = 0;
                if (i < P.count) { v = entry_value(packet_bytes(a, hl, bl, i)); n = plt_entry_bytes(v); }
                const uint64_t incl = wave_scan64(n, lane);
                uint8_t* const e = f + 12 + kPltSegHead + carry + incl - n;
                for (uint32_t j = 0; j < n; ++j) e[j] = plt_entry_byte(v, n, j);
                carry += __shfl(incl, 63, 64);
            }
            if (lane == 0) {
                f[12] = 0xFF; f[13] = 0x58; f[14] = (uint8_t)((3 + eb) >> 8); f[15] = (uint8_t)(3 + eb); f[16] = 0;
            }
            pos = 12 + kPltSegHead + (uint32_t)eb;
        } else {
            // (rare: more than ~11 000 packets in one part) one lane, segment by segment, by the split rule of KT1b and write_plt
            if (lane == 0) {
                PltSplit sp;
                uint32_t seg = 0;
                for (uint32_t i = 0; i < P.count; ++i) {
                    const uint64_t v = entry_value(packet_bytes(a, hl, bl, i));
                    const uint32_t n = plt_entry_bytes(v);
                    const uint32_t fill = sp.fill;
                    if (sp.add(n)) {
                        if (sp.segments > 1) { f[seg + 2] = (uint8_t)((3 + fill) >> 8); f[seg + 3] = (uint8_t)(3 + fill); }
                        if (sp.segments > 256u) bad = true;             // (Zplt is one byte)
                        seg = pos;
                        f[pos++] = 0xFF; f[pos++] = 0x58; pos += 2; f[pos++] = (uint8_t)(sp.segments - 1u);
                    }
                    for (uint32_t j = 0; j < n; ++j) f[pos++] = plt_entry_byte(v, n, j);
                }
                f[seg + 2] = (uint8_t)((3 + sp.fill) >> 8); f[seg + 3] = (uint8_t)(3 + sp.fill);
            }
            pos = __shfl(pos, 0, 64);
        }
    }
    if (lane == 0) {
        const uint32_t isot = a.tile_index[t];
        const uint64_t len = (uint64_t)pos + 2 + body;
        if (len >> 32) bad = true;                                       // (Psot is 32 bits)
        f[0] = 0xFF; f[1] = 0x90; f[2] = 0; f[3] = 10; f[4] = (uint8_t)(isot >> 8); f[5] = (uint8_t)isot;
        f[6] = (uint8_t)(len >> 24); f[7] = (uint8_t)(len >> 16); f[8] = (uint8_t)(len >> 8); f[9] = (uint8_t)len;
        f[10] = (uint8_t)k; f[11] = (uint8_t)a.nparts;                   // TPsot, TNsot
        f[pos] = 0xFF; f[pos + 1] = 0x93;
        a.lit_len[(size_t)t * a.nparts + k] = pos + 2;
        a.tp_len[(size_t)t * a.nparts + k] = (uint32_t)len;
        if (bad) atomicOr(a.status, 8u);
    }
}

__global__ __launch_bounds__(256) void t2_part_place_kernel(T2PartsArgs a)
{
    __shared__ uint64_t wsum[4];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t n = (uint64_t)a.ntiles * a.nparts;
    uint64_t carry = a.dst_offset;
    for (uint64_t base = 0; base < n; base += 256) {
        const uint64_t i = base + tid;
        const uint64_t v = i < n ? a.tp_len[i] : 0u;
        const uint64_t incl = wave_scan64(v, lane);
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        uint64_t before = 0, total = 0;
        for (uint32_t w = 0; w < 4; ++w) { const uint64_t s = wsum[w]; if (w < wave) before += s; total += s; }
        __syncthreads();
        if (i < n) a.tp_dst[i] = carry + before + incl - v;
        carry += total;
    }
    __syncthreads();
    // a tile's span: from its first part to the next tile's first
    for (uint32_t t = tid; t < a.ntiles; t += 256) {
        const uint64_t at = a.tp_dst[(size_t)t * a.nparts];
        const uint64_t end = t + 1 < a.ntiles ? a.tp_dst[(size_t)(t + 1) * a.nparts] : carry;
        if ((end - at) >> 32) atomicOr(a.status, 8u);
        a.tile_dst[t] = at;
        a.part_len[t] = (uint32_t)(end - at);
    }
    if (tid == 0) { a.total[0] = carry - a.dst_offset; a.total[1] = carry; }
}

__global__ __launch_bounds__(64) void t2_part_packet_kernel(T2PartsArgs a)
{
    const uint32_t lane = threadIdx.x, k = blockIdx.x, t = blockIdx.y;
    const T2Part P = a.parts[k];
    const uint32_t* const hl = a.pk_hdr + (size_t)t * a.npackets + P.first;
    const uint64_t* const bl = a.pk_body + (size_t)t * a.npackets + P.first;
    uint64_t* const dst = a.pk_dst + (size_t)t * a.npackets + P.first;
    uint64_t at = a.tp_dst[(size_t)t * a.nparts + k] + a.lit_len[(size_t)t * a.nparts + k];
    for (uint32_t base = 0; base < P.count; base += 64) {
        const uint32_t i = base + lane;
        const uint64_t v = i < P.count ? packet_bytes(a, hl, bl, i) : 0u;
        const uint64_t incl = wave_scan64(v, lane);
        if (i < P.count) dst[i] = at + incl - v;
        at += __shfl(incl, 63, 64);
    }
}

// KT2 of kernels_t2.hip, its frame items one per (tile, part)
__global__ __launch_bounds__(256) void t2_gather_parts_kernel(T2GatherArgs a, const T2Part* parts, uint32_t nparts, const unsigned long long* tp_dst)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t item = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    const uint64_t nblk = (uint64_t)a.ntiles * a.bpt, npk = (uint64_t)a.ntiles * a.npackets;
    if (item < nblk) {
        const uint64_t tile = item / a.bpt;
        const uint32_t row = (uint32_t)(item - tile * a.bpt);
        const uint64_t q = tile * a.npackets + a.packet_of_block[row];
        const uint32_t len = a.lengths[item];
        if (t2_len_ok(len)) wave_copy(a.out + a.pk_dst[q] + a.sop + a.pk_hdr[q] + a.eph + a.rel[item], a.arena + a.offsets[item], len, lane);
    } else if (item < nblk + npk) {
        const uint64_t q = item - nblk;
        const uint64_t tile = q / a.npackets;
        const uint32_t pk = (uint32_t)(q - tile * a.npackets);
        uint8_t* d = a.out + a.pk_dst[q];
        const uint32_t n = a.pk_hdr[q];
        if (a.sop) {                    // Nsop keeps counting through the tile: the packet's number in the TILE modulo 65536
            if (lane < 6) d[lane] = lane == 0 ? 0xFF : lane == 1 ? 0x91 : lane == 2 ? 0 : lane == 3 ? 4 : lane == 4 ? (uint8_t)(pk >> 8) : (uint8_t)pk;
            d += 6;
        }
        wave_copy(d, a.hdr + tile * a.h_bytes + a.packets[pk].h_at, n, lane);
        if (a.eph && lane < 2) d[n + lane] = lane ? 0x92 : 0xFF;
    } else if (item < nblk + npk + (uint64_t)a.ntiles * nparts) {
        const uint64_t q = item - nblk - npk;
        const uint64_t t = q / nparts;
        wave_copy(a.out + tp_dst[q], a.lit + t * a.lit_stride + parts[q - t * nparts].frame_at, a.lit_len[q], lane);
    }
}

hipError_t launch_t2_part_frames(const T2PartsArgs& a, hipStream_t s)
{
    if (!a.ntiles || !a.nparts) return hipSuccess;
    hipLaunchKernelGGL(t2_part_frame_kernel, dim3(a.nparts, a.ntiles), dim3(64), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_t2_part_places(const T2PartsArgs& a, hipStream_t s)
{
    if (!a.ntiles || !a.nparts) return hipSuccess;
    hipLaunchKernelGGL(t2_part_place_kernel, dim3(1), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_t2_part_packets(const T2PartsArgs& a, hipStream_t s)
{
    if (!a.ntiles || !a.nparts) return hipSuccess;
    hipLaunchKernelGGL(t2_part_packet_kernel, dim3(a.nparts, a.ntiles), dim3(64), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_t2_gather_parts(const T2GatherArgs& a, const T2Part* parts, uint32_t nparts, const unsigned long long* tp_dst, hipStream_t s)
{
    const uint64_t items = (uint64_t)a.ntiles * a.bpt + (uint64_t)a.ntiles * a.npackets + (uint64_t)a.ntiles * nparts;
    if (!items) return hipSuccess;
    hipLaunchKernelGGL(t2_gather_parts_kernel, dim3((uint32_t)((items + 3) / 4)), dim3(256), 0, s, a, parts, nparts, tp_dst);
    return hipGetLastError();
}

} // namespace grk_amd
