// grok_amd/csrc/wave_copy.h -- n bytes from s to d by one wave of 64 lanes (device code; KT2 of kernels_t2.hip and the two kernels
// of kernels_t2dec.hip): 16-byte stores on the destination's alignment, unaligned 16-byte loads, head and tail by bytes.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace grk_amd {

struct __attribute__((aligned(1))) U128 { uint32_t x, y, z, w; };
__device__ __forceinline__ void wave_copy(uint8_t* d, const uint8_t* s, uint64_t n, uint32_t lane)
{
    const uint64_t head = min(n, (uint64_t)((0 - (uintptr_t)d) & 15u));
    if (lane < head) d[lane] = s[lane];
    d += head; s += head; n -= head;
    const uint64_t nv = n >> 4;
    for (uint64_t i = lane; i < nv; i += 64) {
        U128 v;
        __builtin_memcpy(&v, s + 16 * i, 16);
        *reinterpret_cast<uint4*>(d + 16 * i) = make_uint4(v.x, v.y, v.z, v.w);
    }
    const uint64_t t0 = nv << 4;
    if (t0 + lane < n) d[t0 + lane] = s[t0 + lane];
}

} // namespace grk_amd
