// grok_amd/csrc/dwt_common.h -- device helpers of the forward (K2, kernels_dwt.hip) and inverse (K6, kernels_idwt.hip) wavelet
// levels: symmetric extension by index mirroring, the separately rounded 9/7 lifting step and its constants; and the forward
// colour transform of one pixel that K1 (kernels_ingest.hip) and K2's fused level 0 apply.
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

namespace grk_amd {

__device__ __forceinline__ uint32_t mirror_idx(int32_t i, uint32_t n)
{
    if (n == 1) return 0;
    const int32_t p = 2 * ((int32_t)n - 1);
    i %= p;
    if (i < 0) i += p;
    return (uint32_t)(i < (int32_t)n ? i : p - i);
}
// same for indices that leave [0, n) by fewer than 16 samples (the row loop): one reflection, no division
// (TALL: the caller knows n >= 16)
template <bool TALL>
__device__ __forceinline__ uint32_t mirror_row(int32_t i, uint32_t n)
{
    if (!TALL && n < 16) return mirror_idx(i, n);
    i = i < 0 ? -i : i;
    return (uint32_t)(i < (int32_t)n ? i : 2 * ((int32_t)n - 1) - i);
}

// 9/7 lifting coefficients and scaling (the inverse runs -delta, -gamma, -beta, -alpha and scales by K and 2 / K)
constexpr float kAlpha   = -1.586134342f;
constexpr float kBeta    = -0.052980118f;
constexpr float kGamma   = 0.882911075f;
constexpr float kDelta   = 0.443506852f;
constexpr float kK       = 1.230174105f;
constexpr float kTwoInvK = 1.625732422f;        // the reference's rounded literal, not 2 / kK

// x + (l + r) * c, every operation rounded on its own (no FMA)
__device__ __forceinline__ float lift(float x, float l, float r, float c)
{
    return __fadd_rn(x, __fmul_rn(__fadd_rn(l, r), c));
}

// forward colour transform of one pixel: RCT (mct.cpp:94-104) or ICT (:541-553: every product / sum rounded separately,
// left-to-right adds; the results as float bit patterns)
__device__ __forceinline__ void color_fwd(int32_t& c0, int32_t& c1, int32_t& c2, bool irrev)
{
    if (!irrev) {
        const int32_t r = c0, g = c1, b = c2;
        c0 = (r + 2 * g + b) >> 2;
        c1 = b - g;
        c2 = r - g;
    } else {
        const float a_r = 0.299f, a_g = 0.587f, a_b = 0.114f;
        const float cb = 0.5f / (1.0f - a_b), cr = 0.5f / (1.0f - a_r);
        const float r = (float)c0, g = (float)c1, b = (float)c2;
        float y = __fmul_rn(a_r, r);
        y = __fadd_rn(y, __fmul_rn(a_g, g));
        y = __fadd_rn(y, __fmul_rn(a_b, b));
        c0 = __float_as_int(y);
        c1 = __float_as_int(__fmul_rn(cb, __fsub_rn(b, y)));
        c2 = __float_as_int(__fmul_rn(cr, __fsub_rn(r, y)));
    }
}

} // namespace grk_amd
