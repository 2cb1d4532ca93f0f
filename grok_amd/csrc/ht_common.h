// grok_amd/csrc/ht_common.h -- what the HT block encoder (K3, kernels_ht.hip) and decoder (K5, kernels_htdec.hip) share on the
// device: the MEL exponent table and the wave-wide prefix sum.
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

namespace grk_amd {

// MEL exponents E[k], k = 0..12 = {0,0,0,1,1,1,2,2,2,3,3,4,5} (ojph_block_encoder.cpp:226), one nibble each
constexpr uint64_t kMelE = 0x5433222111000ull;

// v of the lane CTRL names (a DPP move; 0 where there is none)
template <int CTRL, int ROWMASK>
__device__ __forceinline__ uint32_t dpp0(uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROWMASK, 0xF, true);
}
// inclusive prefix sum over the 64 lanes: 4 row_shr steps inside each row of 16, then row_bcast
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v)
{
    v += dpp0<0x111, 0xF>(v);      // row_shr:1
    v += dpp0<0x112, 0xF>(v);      // row_shr:2
    v += dpp0<0x114, 0xF>(v);      // row_shr:4
    v += dpp0<0x118, 0xF>(v);      // row_shr:8
    v += dpp0<0x142, 0xA>(v);      // row_bcast:15 -> rows 1,3
    v += dpp0<0x143, 0xC>(v);      // row_bcast:31 -> rows 2,3
    return v;
}

} // namespace grk_amd
