// grok_amd/csrc/decode_constants.h -- what the block decoders' kernels (kernels.h) and the host's launch planning (decode_plan.h)
// agree on.  No HIP in here: decode_plan.cpp is built by a plain C++ compiler as well.
#pragma once
#include <cstdint>

namespace grk_amd {

constexpr uint32_t kSkipBlock = 0xFFFFFFFFu;   // missing_msbs of a zero-length row: the block lies outside the decoded region
constexpr uint32_t kT1WorkBytes = 16384;       // a block's share of the Part-1 workspace (K8: 64 x 64 values; K8L: t1_lanes.h)
constexpr uint32_t kT1LaneMaxPlanes = 14;      // bit-planes whose bitmaps fit behind a block's state there
constexpr uint32_t kT1LaneMinRows = 9;         // a lane block has at least three stripes (t1_lanes.h: stripe hand-over)
constexpr uint32_t kT1NoBlock = 0xFFFFFFFFu;   // list entry of a lane without a block

#if defined(__HIP_DEVICE_COMPILE__) || defined(__HIPCC__)
#define GRK_DEC_FN __host__ __device__ inline
#else
#define GRK_DEC_FN inline
#endif

// ---- K6: the strips of an inverse DWT level (kernels_idwt.hip) ----------------------------------------------------------------------
constexpr uint32_t kIdwtStripPairs = 224;      // coefficient pairs a workgroup of the 32-bit kernels owns (kernels_idwt.hip: kOutPairs)
constexpr uint32_t kIdwtHaloPairs = 2;         // ... and stages beside them, each side
constexpr uint32_t kIpkStripCols = 960;        // output columns a workgroup of the packed 5/3 kernel owns at most (kPkOutCols)
// the strips of a packed level share its width evenly, in multiples of 64 output columns
GRK_DEC_FN uint32_t ipk_strip_cols(uint32_t cw)
{
    const uint32_t n = (cw + kIpkStripCols - 1) / kIpkStripCols;
    const uint32_t even = ((cw + n - 1) / n + 63u) & ~63u;
    return kIpkStripCols < even ? kIpkStripCols : even;
}
constexpr uint32_t kIdwtMinWgs = 4096;         // row segments are halved until a level has this many workgroups (row_segment_pairs)
constexpr uint32_t kIdwtRegionSegPairs = 16;   // row pairs per workgroup of a region decode's levels

} // namespace grk_amd
