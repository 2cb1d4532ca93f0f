// grok_amd/csrc/encode_constants.h -- what the encode path's kernels (kernels.h) and the host's launch planning (encode_plan.h)
// agree on.  No HIP in here: encode_plan.cpp is built by a plain C++ compiler as well.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIP_DEVICE_COMPILE__) || defined(__HIPCC__)
#define GRK_ENC_FN __host__ __device__ inline
#else
#define GRK_ENC_FN inline
#endif

namespace grk_amd {

// ---- K3: block classes and the arena allocator (kernels_ht.hip) --------------------------------------------------------------------
constexpr uint32_t kHtMaxClasses = 24;      // (resolution, LDS need): up to 10 levels + 1, two each
// r03: 64 region words and 64 KiB chunks (r01 / r02: 16 and 256 KiB -- the same 4 MiB of slack at most).  An atomic on a region word
// executes at the memory side, one after the other per word, and a block coder waits for its answer: with 16 words the round trip
// was 10.8 % of K3's time (counters of a build that stops behind it), with 64 the 8K frame's K3 takes 0.30 instead of 0.315 ms and
// the pipelined step 0.422 instead of 0.437 (128 / 256 words: the same; two words: 0.77 ms)
#ifndef GRK_HT_ALLOC_REGIONS
#define GRK_HT_ALLOC_REGIONS 64
#endif
constexpr uint32_t kHtAllocRegions = GRK_HT_ALLOC_REGIONS;           // region words available; a launch uses region_mask + 1 of them
constexpr uint32_t kHtAllocChunk = 64u << 10;      // bytes a region takes from the shared cursor at a time (> twice the largest block)
constexpr uint32_t kHtAllocChunkSmall = 32u << 10; // ... in a job of few blocks (the slack of half-used chunks counts there)
constexpr size_t   kHtAllocBytes = 256u * (1u + kHtAllocRegions);   // 32 status / cursor / class words, then one 256-byte line per region word
// Allocation regions: every block reserves its bytes with an atomic on its region's word, and the blocks of a launch that fits
// the machine in one round (up to ~6 000) all arrive there within microseconds of each other -- atomics on ONE address are
// served one after the other, and a chunk refill makes the region's other waves wait.  At least one region per 64 blocks (r04:
// with one per 256, K3 of a 2048^2 frame took 0.151 ms, with this 0.048; 1024^2 0.079 -> 0.038, 3072^2 0.177 -> 0.069; from
// 4096^2 on all 64 regions were in use before: tools/k3_sizes.py); small jobs (below kHtSmallJobBlocks) take smaller chunks, so
// that the slack of the regions' half-used chunks stays small against their coded bytes.
constexpr uint32_t kHtBlocksPerRegion = 64;
constexpr uint32_t kHtSmallJobBlocks = 16384;
// A class's LDS per wave is what fixes K3's occupancy: waves per CU = kLdsPerCu / LDS per wave, at most kMaxWavesPerCu.  Blocks whose
// worst-case need is above kLdsFor16Waves (160 KiB / 16) are "large-LDS" blocks: classes of their own when nothing caps the buffers
constexpr size_t   kLdsPerCu = 160u << 10;
constexpr size_t   kMaxWavesPerCu = 32;
constexpr size_t   kLdsFor16Waves = 10240;

// ---- rate-targeted encodes: dropped bit-planes per block (kernels_ht.hip DROP, kernels_rate.hip) -------------------------------------
constexpr uint32_t kHtDropSkip = 0xFFu;     // a block's drop byte: the block is not coded (length 0, zero bit-planes Kmax - 1)
constexpr uint32_t kRateDefaultDrop = 6;    // grk_amd_rate::max_drop = 0
constexpr uint32_t kRateMaxDrop = 12;       // the largest Dmax a caller may ask for
constexpr uint32_t kRateMaxCand = kRateMaxDrop + 2;   // candidates of a block at most: d = 0 .. Dmax, SKIP
constexpr uint32_t kRateAllocThreads = 1024;          // the allocator's one workgroup
constexpr uint32_t kRateBisectSteps = 40;             // bisection steps of lambda once it is bracketed within a factor of two
constexpr uint64_t kRateMaxBlocks = 0x7FFFFFFFull;    // blocks of a call's tables at most: what KR1, KR2 and the map kernels index
constexpr uint32_t kRateMaxRounds = 4;                // allocate + write rounds of grk_amd_encode_image_rate

// ---- the call's route (encode.hip) -------------------------------------------------------------------------------------------------
// Pipelined encodes of SMALL frames (up to kFrameStreamSamples samples per call): a frame's whole chain on ONE of the two side streams,
// taken in turn -- no event inside a frame (12 instead of 18 runtime calls), consecutive frames overlap through the streams.  A call
// is bound by the host's launches below ~2048^2 x 3: 512^2 x 3 0.058 -> 0.045 ms, 2048^2 x 3 0.073 -> 0.058; at 4096^2 it makes no
// difference, at 8192^2 it loses 19 % (no top-resolution K3 beside the remaining levels, no stream priorities).
// GRK_AMD_FRAME_STREAMS = 0: never, 1 (default): by size, 2: always
constexpr uint64_t kFrameStreamSamples = 16ull << 20;

// ---- K2: the strips and row segments of a forward DWT level (kernels_dwt.hip) ------------------------------------------------------
constexpr uint32_t kDwtStripCols = 448;     // output columns a workgroup of the 32-bit kernels owns (kernels_dwt.hip: kOutCols)
constexpr int      kPkLaneCols = 4;         // columns a lane of the packed 5/3 kernel owns (int: the kernel's column arithmetic is signed)
// 256 lanes for wide levels (8K level 0: 127 us against 138 with 128 lanes), 128 for narrow ones, whose strips would leave half of
// 256 lanes idle (64 tiles of 1024^2: levels 0-2 238 -> 203 us)
constexpr uint32_t kPkNarrowCols = 2048;    // up to this width: 128 lanes
// The strips of a level share its width evenly, in multiples of 64 columns (64 bytes of every sub-band row); at most nt - 2
// lanes of four columns (one halo lane each side): 960 columns for 256 lanes, 448 for 128
GRK_ENC_FN uint32_t pk_strip_cols(uint32_t cw, uint32_t nt)
{
    const uint32_t most = ((nt - 2u) * kPkLaneCols) & ~63u;
    const uint32_t n = (cw + most - 1) / most;
    const uint32_t even = ((cw + n - 1) / n + 63u) & ~63u;
    return even < most ? even : most;
}
// Row segments: enough workgroups to cover the chip several times, few enough to amortise warm-up rows (profiles/r06_dwt_reads.txt: at
// 4096 the 8K level 0 ran 16-row segments and read 1.55 x its pixels; 2048 -> 32-row segments, 1.35 x, the DWT 1 % faster) ...
constexpr uint32_t kDwtMinWgsPacked = 2048;
// (... for the packed 5/3 kernel; the 32-bit kernels -- 448-column strips, twice the workgroups per row -- are better off with
//  the finer cut: cfg3's 9/7 family 0.361 ms at 4096, 0.394 at 2048)
constexpr uint32_t kDwtMinWgs = 4096;
// Two packed levels in one launch (kernels_dwt.hip pair::dwt53_pk_kernel).  Segment `seg` of a level of ch rows (a multiple of 4), cut
// every seg_pairs (even) row pairs: it STORES the upper level's pairs [store0, store1) and the lower level's pairs [low0, low1), and
// to feed those it COMPUTES the upper level's pairs first .. last inclusive: the lower level's recurrence starts at LL row
// 2 low0 - 2 (its own warm-up pair) and its last pair reads LL row 2 low1 -- except at the bottom of the image, where that row is
// the mirror of one it has; pair `last` is computed all the same, from mirrored rows, and not used.  Pairs below 0 are made from
// mirrored rows and equal pairs 2 and 1.
struct DwtPairRows { int32_t store0, store1, first, last, low0, low1; };
GRK_ENC_FN DwtPairRows dwt_pair_rows(uint32_t seg, uint32_t seg_pairs, uint32_t ch)
{
    const int32_t sh = (int32_t)(ch >> 1), j0 = (int32_t)(seg * seg_pairs);
    const int32_t j1 = j0 + (int32_t)seg_pairs < sh ? j0 + (int32_t)seg_pairs : sh;
    return DwtPairRows{j0, j1, j0 - 2, j1, j0 >> 1, j1 >> 1};
}
// The pair's own floor of workgroups, and the most row pairs of a segment.  Every segment computes three pairs more than it stores, so
// the pair wants longer segments than a level alone: at 1024 the 8K frame runs 32-pair segments (1152 workgroups), 0.3200 ms per
// pipelined frame against 0.3230 with 16-pair ones (floor 2048); beyond 32 pairs it loses again -- 64 tiles of 1024^2 0.3395 ms with
// 64-pair segments, 0.3335 with 32 (profiles/dwt_pair.txt)
constexpr uint32_t kDwtPairMinWgs = 1024;
constexpr uint32_t kDwtPairMaxSeg = 32;

} // namespace grk_amd
