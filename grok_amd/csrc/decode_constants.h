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

} // namespace grk_amd
