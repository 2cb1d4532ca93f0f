// grok_amd/csrc/encode_plan.h -- what an encode call works out on the host before it launches anything: K3's block classes, their
// LDS buffers, the arena and its allocator, which class goes to which stream and when, the call's route, the shape of each forward
// DWT level.  Plain integer code over a TileGeom: no HIP, no grk_amd_ctx, so that a plain C++ compiler builds it and
// tests/c/encode_plan_units.cpp steps through it without a GPU.  These numbers set K3's occupancy, the allocator's contention and
// the streams' overlap.
#pragma once
#include "dwt_instances.h"
#include "encode_constants.h"
#include "geometry.h"
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#pragma GCC visibility push(hidden)       // private to the library, like everything in context.h
namespace grk_amd {

// ---- K3 block classes ------------------------------------------------------------------------------------------------------------
// K3 block classes, each its own launch: the top resolution's sub-bands (3/4 of all blocks) are final after DWT
// level 0, so they are coded beside the remaining levels (run_dwt, overlap), the rest after the last level; a third
// class holds ALL blocks, for when nothing overlaps (one launch, one tail).  The LDS buffers of a launch are sized
// for what the class's typical block needs (capped, plan_ht_lds) -- the LDS per wave is what fixes the occupancy
// -- and the blocks that outgrow them, e.g. the few high-Kmax blocks of the low resolutions, go through the fallback
// launch.  Only with GRK_AMD_LDS_CAP=0 (worst-case buffers, no fallback) are the large-LDS blocks classes of their
// own, so that they do not cost every block a wave per SIMD.  Few classes on purpose: a launch ends with a tail of
// long-running waves, and launches on one stream do not overlap (measured: one class per resolution costs 0.15 ms at 8K).
enum class HtRole : uint8_t { Top, Rest, All, TopSmall, TopBig, RestSmall, RestBig };
struct HtClassPlan {
    uint32_t count;                               // blocks of a tile in the class (never 0: an empty class is not listed)
    uint32_t max_kmax, max_samples, max_quads;    // extents that size the class's worst-case LDS buffers
    uint32_t cap_kmax;                            // the exponent most of the class's samples have (a tie: the lower one)
    uint32_t first;                               // the class's first entry in HtClasses::sel
    HtRole role;
};
struct HtClasses {
    std::vector<uint32_t> sel;                    // per class, the rows of a tile's block table ([comp][block]) it holds, in table order
    std::vector<HtClassPlan> classes;             // lds_cap: Top, Rest, All; else TopSmall, TopBig, RestSmall, RestBig
};
HtClasses plan_ht_classes(const TileGeom& g, uint32_t ncomp, bool lds_cap);

// ---- the LDS buffers of a class ---------------------------------------------------------------------------------------------------
struct HtLdsPlan { uint32_t ms_words, vlc_words, ms_cap_bits, vlc_cap_bits, stage_bytes; size_t bytes; };   // (the kernels' HtLds + the launch's dynamic LDS)
// LDS words of a launch whose largest block has `samples` samples in `quads` quads and exponent kmax
// capped = false: the worst case (m_n <= U_q <= Kmax + 2 inside the contract; cwd <= 7, UVLC prefix <= 3, suffix <= 5
// bits per quad).  capped = true: what real content needs with room to spare -- reversible: 8 bits per sample on
// average for 8-bit content (Kmax <= 11), Kmax - 3 beyond; quantised (irreversible) coefficients: 8 bits whatever the
// exponent (the default step sizes leave ~3 bits per sample of a 16-bit image); 10 VLC bits per quad.
HtLdsPlan ht_lds_layout(uint32_t samples, uint32_t quads, uint32_t kmax, bool capped, bool irrev);
inline size_t ht_lds_bytes(uint32_t samples, uint32_t quads, uint32_t kmax) { return ht_lds_layout(samples, quads, kmax, false, false).bytes; }
size_t ht_waves_per_cu(size_t lds_bytes);          // waves of K3 a CU holds with that much LDS each
// capped LDS when that buys occupancy (there is a fallback list and more waves fit a CU), else worst-case buffers
struct HtClassLds { HtLdsPlan full, cap; bool use_cap; };
HtClassLds plan_ht_lds(uint32_t max_samples, uint32_t max_quads, uint32_t max_kmax, uint32_t cap_kmax, bool irrev, bool have_fallback);

// ---- the instances that take a per-block drop, and a rate-targeted call's tables ----------------------------------------------------
// Which ht_encode_drop_kernel instance a launch takes, from the plane form a non-pipelined encode holds: int32 reversible, int32
// irreversible (float bit patterns), int16 for 8-bit reversible content (read through the general, non-packed fetch).
struct HtDropInstance { bool irrev, h16; };
struct HtDropPlan { bool ok; HtDropInstance inst; };           // ok = false: no such plane form (irreversible int16 planes do not exist)
HtDropPlan plan_ht_drop_instance(bool irreversible, bool h16);
// The candidates of a block and the tables over them.  Candidate c of 0 .. dmax: c bit-planes dropped; candidate dmax + 1: SKIP (its
// row exists in L (all 0) and E whether or not the allocator may choose it).  Tables are candidate-major: row c holds nblocks entries
// in table order.  trials: launches of the drop instances that fill L's rows 0 .. dmax.
struct RatePlan {
    bool ok;                           // max_drop within kRateMaxDrop
    uint32_t dmax, rows, ncand;        // rows = dmax + 2 (of L and E); ncand = what the allocator chooses from: dmax + 1 (+ 1 with SKIP)
    uint32_t trials;
    uint64_t l_bytes, e_bytes, w_bytes, drop_bytes;
};
RatePlan plan_rate(uint32_t max_drop, bool allow_skip, uint64_t nblocks);
// One set of tables over a whole image's units (a tile; a run of a tile's components of one size).  The joint row order is the order
// in which the file's writer takes the table: unit after unit in unit order, unit u's unit_blocks[u] rows at first_row[u] -- whatever
// the batches are.  A batch (one grk_amd_encode_tiles call: units of one geometry, in any order) writes its columns through
// map[batch][i] = the first joint row of its i-th member; every member has per_unit[batch] blocks, so entry e of the batch is joint
// row map[batch][e / per_unit] + e % per_unit < n.
// ok = false (nothing else filled in): max_drop above kRateMaxDrop; more than kRateMaxBlocks rows; no unit, an empty unit or an empty
// batch; a member that is no unit; a unit in no batch or in two; a batch whose members differ in their block counts.
struct RateJointPlan {
    bool ok;
    uint64_t n;                                  // rows of a joint table
    std::vector<uint64_t> first_row;             // [unit]
    std::vector<std::vector<uint64_t>> map;      // [batch][member]
    std::vector<uint32_t> per_unit;              // [batch]
    RatePlan tables;                             // plan_rate over n
};
RateJointPlan plan_rate_joint(uint32_t max_drop, bool allow_skip, const std::vector<uint64_t>& unit_blocks,
                              const std::vector<std::vector<uint32_t>>& batches);
// The blocks' budgets of a whole-image call's rounds (rate_rounds, rate.hip).  The first: all the plain blocks' bytes for a target at
// or above the plain file, else the target less what the plain file spends beside its blocks (0: the target does not cover that).
// The next, after a round whose file is still above the target: the smaller of the budget and what the round's blocks took, less the
// overshoot; left = false: the budget or the blocks' bytes were 0 already -- nothing is left to take.
uint64_t rate_first_budget(uint64_t target, uint64_t plain_file_bytes, uint64_t plain_block_bytes);
struct RateNextBudget { bool left; uint64_t budget; };
RateNextBudget rate_next_budget(uint64_t budget, uint64_t block_bytes, uint64_t file_bytes, uint64_t target);
// The split route's shares of a round's budget: see group_shares in encode_plan.cpp
std::vector<uint64_t> group_shares(uint64_t budget, const std::vector<uint64_t>& samples, const std::vector<uint64_t>& plain);
// A quality target as the distortion budget the quality allocator (KQ) takes: D = S * peak^2 * 10^(-psnr / 10) with peak = 2^prec - 1
// and S the samples the PSNR is over -- the sum over the components of the component's OWN samples in the image area
// (quality_samples): a sub-sampled component counts its own samples, with no area factor, the convention W and `distortion` follow.
// target_psnr > 0: used (+infinity: D = 0); target_psnr == 0: D = target_distortion, which must be >= 0.
// ok = false: a negative or NaN target_psnr, a negative or NaN target_distortion where it is used, prec 0 or above 16, no sample.
struct QualityPlan {
    bool ok;
    double budget;                     // D
    double signal;                     // S * peak^2: the model's PSNR of a distortion d is 10 log10(signal / d)
};
QualityPlan plan_quality(double target_psnr, double target_distortion, uint32_t prec, uint64_t samples);
inline double quality_psnr(double signal, double distortion) { return distortion > 0 ? 10.0 * std::log10(signal / distortion) : INFINITY; }
// S of an image area for components with factors comp_dx / comp_dy (nullptr: all 1): component c holds ceil(x1 / dx) - ceil(x0 / dx)
// columns and ceil(y1 / dy) - ceil(y0 / dy) rows, however the area is tiled.  0: an empty area or a factor of 0.
uint64_t quality_samples(const grk_amd_image_layout& im, uint32_t num_comps, const uint8_t* comp_dx, const uint8_t* comp_dy);
// the drop byte of candidate c, and the row's zero bit-planes for a drop byte (d clamped to Kmax - 1; SKIP: Kmax - 1)
inline uint8_t rate_drop_byte(uint32_t c, uint32_t dmax) { return c <= dmax ? (uint8_t)c : (uint8_t)kHtDropSkip; }
GRK_T2_FN uint32_t drop_missing_msbs(uint32_t kmax, uint32_t drop)
{
    const uint32_t top = kmax ? kmax - 1u : 0u;
    return drop == kHtDropSkip ? top : top - (drop < top ? drop : top);
}

// ---- the arena and its allocator ---------------------------------------------------------------------------------------------------
struct HtArenaPlan {
    uint32_t regions;                  // allocation regions in use (a power of two <= kHtAllocRegions): block i allocates from region i & (regions - 1)
    uint32_t chunk;                    // bytes a region takes from the shared cursor at a time
    size_t   worst_block;              // the largest block the classes can produce
    uint64_t arena_bytes;
    uint64_t ovf_entries;              // entries of the fallback list (every block is in two classes)
    uint32_t ovf_base[kHtMaxClasses];  // each class's first entry there
};
HtArenaPlan plan_ht_arena(uint64_t nblocks, uint64_t raw_bytes, uint32_t ntiles, const std::vector<HtClassPlan>& classes);

// ---- which class goes to which stream, and when ------------------------------------------------------------------------------------
// The points of a call at which K3 launches are queued: run_dwt after level 0 and after the last level, then run_ht
enum class HtPoint : uint8_t { AfterLevel0, AfterLastLevel, RunHt };
enum class HtStream : uint8_t { NotHere, Main, Side, Side2 };
struct HtScheduleRow { HtRole role; bool overlapped; int8_t pipelined /* -1: either */; HtPoint at; HtStream to; };
// Not overlapped: one launch of every block where there is such a class (the roles Top and Rest exist only beside All), else class
// by class.  Overlapped: after level 0 the top resolution's sub-bands are final: its code-blocks (3/4 of all) are coded on
// low-priority side streams while the remaining levels -- short, latency-bound launches that are the critical path -- run on the
// main stream.  After the last level the rest follows: small-LDS class on the main stream (run_ht) beside the tail of the top
// resolution, large-LDS class on the second side stream, so that the launches' tails overlap -- unless consecutive encodes are
// pipelined: then the main stream carries nothing but the DWT chain, so that the next encode's level 0 starts as early as possible,
// and every K3 launch queues on a side stream (the rest's tail then overlaps the top class's).
inline constexpr HtScheduleRow kHtSchedule[] = {
    {HtRole::All,       false, -1, HtPoint::RunHt,          HtStream::Main},
    {HtRole::TopSmall,  false, -1, HtPoint::RunHt,          HtStream::Main},
    {HtRole::TopBig,    false, -1, HtPoint::RunHt,          HtStream::Main},
    {HtRole::RestSmall, false, -1, HtPoint::RunHt,          HtStream::Main},
    {HtRole::RestBig,   false, -1, HtPoint::RunHt,          HtStream::Main},
    {HtRole::Top,       true,  -1, HtPoint::AfterLevel0,    HtStream::Side},
    {HtRole::TopSmall,  true,  -1, HtPoint::AfterLevel0,    HtStream::Side},
    {HtRole::TopBig,    true,  -1, HtPoint::AfterLevel0,    HtStream::Side2},
    {HtRole::RestBig,   true,  -1, HtPoint::AfterLastLevel, HtStream::Side2},
    {HtRole::Rest,      true,   0, HtPoint::RunHt,          HtStream::Main},
    {HtRole::RestSmall, true,   0, HtPoint::RunHt,          HtStream::Main},
    {HtRole::Rest,      true,   1, HtPoint::AfterLastLevel, HtStream::Side2},
    {HtRole::RestSmall, true,   1, HtPoint::AfterLastLevel, HtStream::Side2},
};
// one_level: L == 1, level 0 is the last level as well -- AfterLevel0 then answers for both points and AfterLastLevel is not asked
// parity (pipelined overlapped encodes only; else ignored): consecutive frames take the two side streams in turn -- parity 0 is the
// table above, parity 1 the table with Side and Side2 exchanged.  Launches on one stream do not overlap, so with a fixed table
// top(n + 1) queues behind the last wave of top(n) and its fallback launch: K3's wave supply has a hole at every frame boundary.
// In turn, top(n + 1) queues behind rest(n), which ended long before, and rest(n + 1) behind top(n), where it has slack.  Within
// a frame Top and Rest (and the Small / Big pairs as the table has them) stay on different streams in either parity.
HtStream ht_class_stream(HtRole role, bool overlapped, bool pipelined, HtPoint at, bool one_level, uint32_t parity = 0);

// ---- the call's route ----------------------------------------------------------------------------------------------------------------
// 16-bit planes are safe when no coefficient of any level can leave int16.  Bound (5/3, L1 norms of the analysis
// filters: low-pass 1.5, high-pass 2 per dimension; RCT chroma is one bit wider than the pixels): the LL of level l is
// below M * 2.25^l, a detail band of level l below 4 * M * 2.25^(l-1), with M = 2^prec the largest input magnitude.
bool planes16_ok(const grk_amd_tile_params& p);
// Level l of such a tile on PACKED int16 pairs (kernels_dwt.hip, strip_pk): every intermediate of the 2-D lifting step has to
// stay inside 16 bits as well.  With M the largest magnitude entering the level (2^prec after DC shift and RCT, times the
// low-pass gain 1.5 x 1.5 per level before, plus rounding), the largest is the horizontal update's sum of two high-pass
// values of a vertically high-pass row: 2 x 2 x 2M each, 8M + 2 in all.
bool pk16_level_ok(const grk_amd_tile_params& p, uint32_t l);
struct RouteIn {
    bool overlap, pipelining; int frame_streams; bool planes16;    // the context's settings (grk_amd_ctx)
    bool have_side, have_side2;                                    // ... and whether it has its side streams
    bool on_device;                                                // the caller's pixels are device memory
    uint32_t px_align;                                             // the low two bits of the (device) pixel pointer
    uint64_t samples;                                              // nplanes * plane_elems
};
struct Route {
    bool fused;          // with at least one DWT level, level 0 consumes the pixels itself and the int32 ingest planes (4 bytes per
                         // sample written and read back) never exist
    bool overlap;        // K3 of the top resolution beside the remaining levels
    bool frame_stream;   // the whole frame on one side stream.  Device-resident pixels only: the staging buffer of host pixels is
                         // filled on the main stream, which must then carry level 0; and the fused level 0: the stand-alone ingest
                         // writes planes that are not part of a buffer set
    bool h16;            // 8-bit reversible content: int16 LL / Mallat planes between K2 and K3 (half the bytes written and read
                         // back); needs the fused level 0 (the stand-alone ingest kernel writes int32 planes)
};
Route plan_route(const grk_amd_tile_params& p, const RouteIn& in);

// ---- the shape of a forward DWT level --------------------------------------------------------------------------------------------
struct DwtLevelDesc {                  // (the fields of DwtLevelArgs the shape depends on)
    uint32_t cw, ch, px, py;
    uint32_t in_stride, m_stride;
    bool h16, pk, irreversible;
    uint32_t px_lay, px_chan; uint64_t px_row;
    uint32_t zslots;                   // workgroups along z: planes, or for the fused level 0 tiles (x level_part_zslots)
    bool fused; uint32_t px_bytes;     // level 0 reads the caller's pixels of px_bytes (1 or 2) each
};
struct DwtLevelShape {
    bool packed;                       // the level shape dwt53_pk_kernel takes
    uint32_t lanes;                    // threads of a workgroup: 128 or 256
    uint32_t strip_cols;               // output columns a workgroup owns
    bool all_fast;                     // (what dwt_level_kernel calls `even`: every strip of the level takes a FAST path)
    uint32_t seg_pairs;                // row pairs per workgroup
    uint32_t grid_x, grid_y;           // strips, row segments
    DwtInstance inst[2];               // the kernel instance (dwt_instances.h) of a part of one component [0] and, for the fused
                                       // level, of the MCT triple [1] (every other level: not used, in no list)
};
DwtLevelShape plan_dwt_level(const DwtLevelDesc& d);

// ---- two forward DWT levels in one launch -------------------------------------------------------------------------------------------
// Levels l and l + 1 of the packed 5/3 kernel as one launch (kernels_dwt.hip pair::dwt53_pk_kernel): the lower level is fed from the
// upper one's registers and the LL plane between them is neither written nor read.  `upper` and `lower` are the two levels as
// plan_dwt_level would be asked about them (the lower one: fused = false, zslots = planes).  A pair is planned when both are packed
// levels on even origins, the upper one reads planar 8-bit pixels of an MCT triple (exactly three components), its width is a
// multiple of 8 (at least 512, so that the lower level is wide enough to be a packed level: four LL columns per lane there) and its
// height a multiple of 4 (at least 32), and the Mallat plane stays below 2^31 bytes (lanes that must not store are given a column
// offset beyond the plane).  Otherwise ok = false and the levels are launched one by one.
struct DwtPairDesc { DwtLevelDesc upper, lower; bool mct; uint32_t ncomp, ntiles; };
struct DwtPairShape {
    bool ok;
    uint32_t lanes, strip_cols;        // as the upper level's DwtLevelShape
    uint32_t seg_pairs;                // row pairs of the UPPER level a workgroup stores (even; segments start on even pairs)
    uint32_t grid_x, grid_y;
    DwtPairKey inst;                   // a row of GRK_DWT_PAIR_INSTANCES
};
DwtPairShape plan_dwt_pair(const DwtPairDesc& d);
// ... for levels l and l + 1 of a tile geometry, as run_dwt asks: the context's switches (pair: GRK_AMD_DWT_PAIR, dwt_pk: GRK_AMD_DWT_PK),
// the call's route (fused: level l reads the caller's pixels; h16: int16 planes), the pixels' layout, the stride of the LL plane
// between the two levels, and the tiles of the call.  No pair without the switch, off the fused route, or when l + 1 is no level.
struct DwtPairAsk { bool pair, dwt_pk, fused, h16; uint32_t px_lay, px_chan; uint64_t px_row; uint32_t px_bytes, mid_stride, ntiles; };
DwtPairShape plan_dwt_pair_at(const TileGeom& g, uint32_t l, const DwtPairAsk& q);

} // namespace grk_amd
#pragma GCC visibility pop
