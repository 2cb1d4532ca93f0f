// grok_amd/csrc/kernels.h -- host-callable launchers of the gfx950 kernels.
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>
#include "geometry.h"
#include "decode_constants.h"
#include "encode_constants.h"
#include "encode_plan.h"
#include "decode_plan.h"

namespace grk_amd {

// ---- K1: ingest + DC shift + forward colour transform (kernels_ingest.hip) -------------------
struct IngestArgs {
    const void* pixels;      // tiles back to back, component-major planar, tight -- or as px_lay .. px_tile say
    int32_t*    planes;      // [tile][comp] planes, `stride` elements per row, `pitch` per plane
    uint32_t w, h, stride;
    uint64_t pitch;
    uint32_t ncomp, ntiles;
    uint32_t bytes_per_sample;   // 1 or 2
    int32_t  dc;                 // 2^(prec-1) or 0
    int32_t  sext;               // signed samples: 1 << (8*bytes_per_sample - 1) (stored as int8/int16), else 0
    int      mct;                // apply RCT/ICT to components 0..2
    int      irreversible;
    // a layout other than the default (grk_amd_set_pixel_layout): sample (x, y) of component k of tile t lies at
    // pixels + t * px_tile + y * px_row + k * px_kstep + x * px_xstep (bytes); px_lay = 0: the default, the four are not read
    uint32_t px_lay, px_xstep;
    uint64_t px_row, px_kstep, px_tile;
};
hipError_t launch_ingest(const IngestArgs& a, hipStream_t s);

// ---- K2: one forward DWT level, vertical + horizontal fused (kernels_dwt.hip) ----------------
struct DwtLevelArgs {
    const int32_t* in;  uint32_t in_stride;  uint64_t in_pitch;    // current LL, cw x ch
    int32_t* ll;        uint32_t ll_stride;  uint64_t ll_pitch;    // next LL (sw x sh)
    int32_t* mallat;    uint32_t m_stride;   uint64_t m_pitch;     // HL/LH/HH go to their Mallat slots
    uint32_t cw, ch;      // size of the level being transformed
    uint32_t px, py;      // parity of the level's origin on its grid: 1 = the first column / row is a high-pass sample
    uint32_t nplanes;
    uint32_t seg_pairs;   // row pairs per workgroup
    int      irreversible;
    // level 0 fused with K1 (launch_dwt_level0_fused): rows come from the caller's pixel planes
    const void* pixels;   // as IngestArgs::pixels
    uint32_t px_bytes;    // 1 or 2 bytes per sample
    int32_t  dc;          // 2^(prec-1) or 0
    int32_t  sext;        // signed samples: sign bit of the stored word (see IngestArgs), else 0
    uint32_t ncomp;       // components per tile
    uint32_t comp0, zdiv; // set by the launcher: first component of a z slot, z slots per tile
    // level 0 fused with K1 in a pipelined encode also resets K3's arena allocator (its first workgroup; kernels_ht.hip ht_alloc_reset):
    // one launch less on the chain that bounds frames of 4096 x 4096 and below
    unsigned long long* alloc_reset; uint32_t alloc_chunk_units;
    int      h16;         // reversible, 8-bit pixels: every plane (in, ll, mallat) holds int16 instead of int32
    int      xcd;         // XCD-aware workgroup order (kernels_dwt.hip)
    int      pk;          // h16 and every intermediate of this level within 16 bits: arithmetic on packed int16 pairs
    // level 0 fused with K1 under a pixel layout other than the default (as IngestArgs): px_lay = 0 the default (tight planar, the
    // fields below are not read), 1 planar with pitches, 2 pixel-interleaved with px_chan samples per pixel in memory
    uint32_t px_lay, px_chan, px_xstep;
    uint64_t px_row, px_kstep, px_tile;
    // two levels in one launch (launch_dwt_pair): the LL of the level below this one (cw / 4 x ch / 4); `ll` is not written
    int32_t* ll2;       uint32_t ll2_stride; uint64_t ll2_pitch;
};
// sh: the level's shape (plan_dwt_level, encode_plan.h) -- which kernel instance, its strips and row segments; a.seg_pairs = sh.seg_pairs
hipError_t launch_dwt_level(const DwtLevelArgs& a, const DwtLevelShape& sh, hipStream_t s);
hipError_t launch_dwt_level0_fused(const DwtLevelArgs& a0, const DwtLevelShape& sh, uint32_t ntiles, uint32_t ncomp, int mct, hipStream_t s);
// levels 0 and 1 of the MCT triple straight from the pixels, in one launch (plan_dwt_pair, encode_plan.h); a0 describes level 0
hipError_t launch_dwt_pair(const DwtLevelArgs& a0, const DwtPairShape& sh, uint32_t ntiles, hipStream_t s);

// ---- K3: HT cleanup encoder, one wavefront per code-block (kernels_ht.hip) -------------------
struct HtBlockDesc {        // one per code-block of a tile-component set (all comps of one tile)
    uint32_t px, py;        // origin in the plane
    uint16_t w, h;
    uint16_t comp;
    uint8_t  kmax;
    uint8_t  pad;
    float    inv_step;      // 1/stepsize (irreversible)
};
struct HtClass {
    const uint32_t* sel;      // device: indices (within a tile) of the blocks of this class; nullptr = all blocks in order
    uint32_t count;
    uint32_t max_kmax, max_samples, max_quads;   // extents that size the class's worst-case LDS buffers
    uint32_t ovf_base;        // first entry of the class's part of HtArgs::ovf_list
    uint32_t cap_kmax;        // the exponent most of the class's samples have: sizes the capped LDS buffers
};
struct HtArgs {
    const int32_t* mallat; uint32_t stride; uint64_t pitch;   // planes [tile][comp] (stride, pitch in elements)
    int h16;                                                  // the planes hold int16 coefficients (reversible only)
    int room;                                                 // the launch runs beside the next frame's DWT level 0: the instance that leaves it registers (kernels_ht.hip)
    const HtBlockDesc* blocks; uint32_t blocks_per_tile; uint32_t ncomp; uint32_t ntiles;
    uint8_t*  arena; uint64_t arena_bytes;      // coded bytes of all blocks (chunked region allocator, kernels_ht.hip)
    unsigned long long* alloc;                  // kHtAllocBytes of allocator state: [0] status flags (bit 0 arena
                                                // overflow, bit 1 magnitude out of contract), [1] bytes used, region words
    uint32_t* lengths;                          // [ntiles*blocks_per_tile]
    unsigned long long* offsets;                // [ntiles*blocks_per_tile]
    const uint32_t* sel; uint32_t sel_count;    // set per launch by launch_ht_encode from `classes`
    uint32_t* ovf_list; uint32_t ovf_base;      // [ntiles * blocks_per_tile] blocks whose raw streams outgrew the capped LDS
                                                // buffers (per class from ovf_base; count in alloc[2 + class]): coded again
                                                // by the fallback launch.  nullptr: worst-case buffers, no fallback
    HtClass classes[kHtMaxClasses]; uint32_t num_classes;   // block classes of a tile (= resolutions, finest first), each launched on its own
    uint32_t region_mask;         // (power of two <= kHtAllocRegions) - 1: block i allocates from region i & mask
    uint32_t chunk_units;         // 16-byte units a region takes from the shared cursor at a time (kHtAllocChunk / 16, or half of it for small jobs)
    const uint32_t* vlc_tab;      // the CxtVLC encode table on the device (set by launch_ht_classes)
    int irreversible;
};
// the allocator's initial state, written by `nthreads` lanes of one workgroup (ht_alloc_init_kernel; the fused level 0 of a pipelined
// encode): [0] status flags, [1] cursor (bytes), [2 + class] blocks handed to the fallback launch = 0; every region word "chunk full"
// so that the first allocation refills -- the start field holds a value no real chunk has, otherwise waves waiting for the refill
// could not tell the first chunk (start 0) from this state
__device__ __forceinline__ void ht_alloc_reset(unsigned long long* flagbuf, uint32_t chunk_units, uint32_t t, uint32_t nthreads)
{
    if (t < 32) flagbuf[t] = 0;
    for (uint32_t r = t; r < kHtAllocRegions; r += nthreads) flagbuf[32 * (1 + r)] = (0xFFFFFFFFFFull << 24) | chunk_units;
}
hipError_t launch_ht_encode(const HtArgs& a, hipStream_t s);          // allocator reset + every class
hipError_t launch_ht_alloc_init(const HtArgs& a, hipStream_t s);
// fallback_grid: workgroups of a class's fallback launch at most (they walk the class's list)
constexpr uint32_t kHtFallbackGrid = 1024;
hipError_t launch_ht_classes(const HtArgs& a, uint32_t first, uint32_t last, hipStream_t s, uint32_t fallback_grid = kHtFallbackGrid);   // classes [first, last)
// the same through the instances that take a per-block drop: drops[ntiles * blocks_per_tile] (device), tile-major in table order, each
// 0 .. 254 bit-planes left out (clamped to Kmax - 1) or kHtDropSkip; inst: plan_ht_drop_instance (encode_plan.h) of a's plane form
hipError_t launch_ht_classes_drops(const HtArgs& a, uint32_t first, uint32_t last, const uint8_t* drops, const HtDropInstance& inst, hipStream_t s);
// sum of q^2 over each block of the planes an encode left (kernels_ingest.hip: the rate-control hook)
hipError_t launch_block_energy(const void* mallat, int h16, int irreversible, uint32_t stride, uint64_t pitch, const HtBlockDesc* blocks,
                               uint32_t blocks_per_tile, uint32_t ncomp, uint64_t nblocks, unsigned long long* out, hipStream_t s);

// ---- KR1 / KR2: a rate-targeted encode's statistics and allocator (kernels_rate.hip) -----------------------------------------------
// Tables are candidate-major over the call's nblocks blocks in table order (RatePlan, encode_plan.h): rows 0 .. dmax = that many
// bit-planes dropped, row dmax + 1 = SKIP.
struct RateStatsArgs {
    const void* mallat; int h16, irreversible; uint32_t stride; uint64_t pitch;      // the planes K3 codes from, as HtArgs
    const HtBlockDesc* blocks; uint32_t blocks_per_tile, ncomp; uint64_t nblocks;
    uint32_t dmax;
    unsigned long long* E;             // [dmax + 2][nblocks]: sum of (2 q - 2 r_c(q))^2 over the block
    // a batch's columns of a call's joint tables: tile t's blocks at map[t] .. (device, [nblocks / blocks_per_tile]) of rows of n entries;
    // nullptr: the identity, rows of nblocks entries
    const unsigned long long* map = nullptr; uint64_t n = 0;
};
hipError_t launch_rate_stats(const RateStatsArgs& a, hipStream_t s);
// A batch's column and a joint row: entry i of `batch` is entry map[i / per_unit] + i % per_unit of `joint` (plan_rate_joint's map:
// every such index is inside the joint row).  gather = 0: batch -> joint, elements of 4 bytes (a trial's length column into a row of
// L); gather = 1: joint -> batch, elements of 1 byte (the chosen drop bytes for the batch's final launch)
struct RateMapArgs { void* batch; void* joint; const unsigned long long* map; uint32_t per_unit; uint64_t count; uint32_t elem; int gather; };
hipError_t launch_rate_map(const RateMapArgs& a, hipStream_t s);
struct RateAllocResult {
    unsigned long long block_bytes, lagrange_bytes, least_bytes;      // the choice's bytes; the Lagrange solution's; the fewest any choice takes
    double distortion, lambda;                                        // sum of W E of the choice; the multiplier
    uint32_t feasible, steps;                                         // least_bytes <= budget; evaluations of the multiplier search
};
struct RateAllocArgs {
    const uint32_t* L; const unsigned long long* E; const double* W;   // [rows][nblocks], [rows][nblocks], [nblocks]
    uint64_t nblocks; uint32_t dmax, ncand;                            // ncand = dmax + 1, or dmax + 2 when SKIP may be chosen
    uint64_t budget;
    uint8_t* drop;                     // [nblocks]: the drop bytes for launch_ht_classes_drops
    RateAllocResult* res;
};
hipError_t launch_rate_alloc(const RateAllocArgs& a, hipStream_t s);
// KQ, the quality allocator: one workgroup of kRateAllocThreads like KR2, over the same L, E, W (> 0) and ncand, for a distortion
// budget D (a double, >= 0) instead of a byte budget: the fewest bytes it finds whose sum of W E is <= D.  Fixed-order sums only.
// choose(b, lambda) is KR2's: the smallest W E + lambda L, the finer candidate on a tie.
//   floor = sum over b of W_b * min_c E[c][b]; feasible = floor <= D.
//   Not feasible: every block goes to its least-E candidate, the finer of equal ones; there is no search and no trim; feasible = 0
//   (no error of the stage call).
//   dist_at(lambda) = sum of W_b * (double)E[choose(b, lambda)][b]; in exact arithmetic it does not fall as lambda rises.
//   The shortest choice is KR2's fallback: the smallest L, the finer of equally short ones.  If its distortion is <= D it is the
//   answer; lambda is then reported as +infinity and steps as 0.
//   Otherwise the search mirrors KR2's, with the same limits: it starts from 1; it doubles while the doubled multiplier still fits
//   (dist_at <= D), or halves until one fits; bracketing takes at most 200 steps; kRateBisectSteps bisections follow, which keep the
//   LOWER end fitting; lambda = lo.  Halving that never fits ends at lo = 0, which fits when feasible.
//   The Lagrange choice at lambda gives lagrange_bytes and its distortion.
//   The trim is the fill's mirror image, in table order, kFillChunk / 2 blocks at a time (a table of doubles with kFillSteps columns:
//   at kFillChunk it would not fit a workgroup's 64 KB beside the reduction buffers) in the fill's three phases -- a thread per chain,
//   one walker, a thread per write-back.  A block moves to the next coarser candidate (c + 1 < ncand) while L strictly falls and
//   delta = W_b * (double)((int64)E[c + 1][b] - (int64)E[c][b]) is <= left; then left -= delta.  left starts as D - the Lagrange
//   choice's distortion.  A block that does not fit is passed over and the walk goes on.
//   The drops are written as KR2 writes them (0 .. dmax, 0xFF for SKIP).
struct RateQualityResult {
    unsigned long long block_bytes, lagrange_bytes, shortest_bytes;   // the final choice's bytes; the Lagrange choice's; the shortest choice's
    double distortion, floor, lambda;                                 // sum of W E summed afresh over the final choice; see above
    uint32_t feasible, steps;                                         // floor <= D; evaluations of the multiplier search
};
struct RateQualityArgs {
    const uint32_t* L; const unsigned long long* E; const double* W;   // as RateAllocArgs
    uint64_t nblocks; uint32_t dmax, ncand;
    double budget;                                                     // D
    uint8_t* drop;
    RateQualityResult* res;
};
// refuses what launch_rate_alloc refuses, and a D that is negative or NaN
hipError_t launch_rate_quality(const RateQualityArgs& a, hipStream_t s);

// ---- K5: HT cleanup decoder + dequantisation (kernels_htdec.hip) --------------------------------
struct HtDecBlock {          // one per code-block, same layout as grk_amd_coded_block
    uint64_t offset;         // first byte of the block's cleanup pass inside `coded`
    uint32_t length;         // Lcup (0: block has no data -> all samples zero)
    uint32_t missing_msbs;   // band numbps - block numbps (T1DecompressScheduler.cpp:59)
};
struct HtDecArgs {
    const HtDecBlock* table;                   // [ntiles * blocks_per_tile], device
    const HtBlockDesc* blocks;                 // geometry per block of one tile; inv_step = decode scale (irreversible)
    uint32_t blocks_per_tile, nblocks, ncomp;
    const uint8_t* coded; uint64_t coded_bytes; // device buffer holding every block's bytes
    const uint32_t* active;                    // [nactive] the blocks with data, K5a's lanes (null: all nblocks)
    uint32_t nactive;
    uint32_t* quads;                           // K5a -> K5b: 16 bits per quad, [nblocks][32 * 32] (kernels_htdec.hip: 9 bits of the CxtVLC entry | (u_q + 1) << 9)
    uint32_t* ms_len;                          // [nblocks] MagSgn bytes (0xFFFFFFFF: block rejected)
    unsigned int* status;                      // bit 2: a block was rejected; bit 3: a value did not fit the 16-bit planes
    int32_t* mallat; uint32_t stride; uint64_t pitch;
    int irreversible;
    int h16;                                   // reversible: the planes hold int16 (strides / pitches in elements all the same)
    int h16_bias;                              // ... and a coefficient outside [-bias, bias) raises bit 3 of *status (32768: what fits; 2048:
                                               // what the packed inverse transform takes, pk16.h)
    const uint2* refine;                       // [nblocks] {bytes of the SigProp / MagRef segment at the end of the block's
                                               // data, coding passes in total (1..3)}, or null: cleanup passes only
    uint32_t max_refine_bytes;                 // largest such segment
    uint32_t ms_first, ms_count, ms_bpc;       // K5b of a part of the blocks: [ms_first, ms_first + ms_count) of every component's
                                               // ms_bpc blocks (ms_count = 0: all nblocks)
};
// K5a + K5b (+ K5c) on one stream, or in two parts: front = tables + K5a, ms = K5b (+ K5c) of a.ms_first / ms_count
hipError_t launch_ht_decode(const HtDecArgs& a, uint32_t max_ms_bytes, hipStream_t s);
hipError_t launch_ht_decode_front(const HtDecArgs& a, hipStream_t s);
hipError_t launch_ht_decode_ms(const HtDecArgs& a, uint32_t max_ms_bytes, hipStream_t s);
// a decode call's tables: `bytes` of pinned host memory (device-visible address) -> dst, the 16-byte status block cleared
hipError_t launch_dec_upload(const void* pinned, void* dst, size_t bytes, void* status, hipStream_t s);

// ---- K8: Part-1 (EBCOT) block decoder + dequantisation (kernels_t1dec.hip) -----------------------
struct T1DecArgs {
    const HtDecBlock* table;                   // missing_msbs field carries numbps | numpasses << 8
    const HtBlockDesc* blocks;                 // pad = band orientation, inv_step = band step size (irreversible)
    uint32_t blocks_per_tile, nblocks, ncomp;
    const uint8_t* coded; uint64_t coded_bytes;
    int32_t* work;                             // [nblocks][64*64] decoded values
    unsigned int* status;                      // bit 4: a block with more than 24 bit-planes (refused, left at zero)
    int32_t* mallat; uint32_t stride; uint64_t pitch;
    int irreversible;
    uint32_t cblksty;                          // COD code-block style bits (LAZY 1, RESET 2, TERMALL 4, VSC 8, PTERM 16, SEGSYM 32)
    const uint32_t* seg_first;                 // [nblocks + 1] first codeword segment of each block, or null: one segment
    const uint2* segs;                         // {bytes, passes} per segment
    const uint32_t* list; uint32_t count;      // the blocks this launch decodes (one wave each, in this order), or null: all nblocks
};
hipError_t launch_t1_decode(const T1DecArgs& a, hipStream_t s);

// ---- K8L: the same decoder with one code-block per LANE + reconstruction from bit-plane bitmaps (kernels_t1lanes.hip) ----
struct T1LaneArgs {
    const HtDecBlock* table;                   // as T1DecArgs
    const HtBlockDesc* blocks;
    uint32_t blocks_per_tile, ncomp;
    const uint32_t* list; uint32_t count;      // the blocks of this launch: lane i of wave k decodes list[64 k + i]
    const uint8_t* coded; uint64_t coded_bytes;
    uint64_t* work;                            // [nblocks][kT1WorkBytes / 8]
    int32_t* mallat; uint32_t stride; uint64_t pitch;
    int irreversible;
    int pass_sync;                             // the waves hold blocks of equal bit-plane / pass counts and run them pass by pass
};
hipError_t launch_t1_lanes(const T1LaneArgs& a, hipStream_t s);       // t1_lanes_kernel, then t1_recon_kernel
// both decoders in ONE launch (the blocks of d.list first, then the lane waves), then t1_recon_kernel: a frame's block decoding on one stream
hipError_t launch_t1_fused(const T1DecArgs& d, const T1LaneArgs& a, hipStream_t s);

// ---- K6: one inverse DWT level, horizontal + vertical fused (kernels_idwt.hip) ------------------
struct IdwtLevelArgs {
    const int32_t* ll;     uint32_t ll_stride;  uint64_t ll_pitch;   // LL of the level (sw x sh)
    const int32_t* mallat; uint32_t m_stride;   uint64_t m_pitch;    // HL/LH/HH read from their Mallat slots
    int32_t* out;          uint32_t out_stride; uint64_t out_pitch;  // synthesised level, cw x ch
    uint32_t cw, ch;
    uint32_t px, py;      // parity of the level's origin (as DwtLevelArgs)
    uint32_t nplanes;
    uint32_t seg_pairs;
    int      irreversible;
    // last level fused with K7 (launch_idwt_level0_fused): the rows leave as the caller's pixels
    void*    pixels;      // as EgressArgs::pixels
    uint32_t px_bytes;    // 1 or 2 bytes per sample
    int32_t  dc, lo, hi;  // DC shift and clamp range (EgressArgs)
    int      mct;
    uint32_t ncomp;       // components per tile
    uint32_t comp0, zdiv; // set by the launcher: first component of a z slot, z slots per tile
    uint32_t wx0, wy0, wx1, wy1;   // window of the tile the pixels are for (the whole tile: 0, 0, cw, ch)
    // region decode: only the strips [strip0, strip0 + nstrips) x row segments [seg0, seg0 + nsegs) (0 = all)
    uint32_t strip0, nstrips, seg0, nsegs;
    int      xcd;         // XCD-aware workgroup order (as DwtLevelArgs)
    int      h16;         // reversible: ll / mallat / out hold int16; a synthesised value that does not fit sets bit 3 of *status
    int      pk;          // h16 and every coefficient within +-kPkDecodeBound (pk16.h): arithmetic on packed int16 pairs
    unsigned int* status;
    // the last level fused with K7 under a pixel layout other than the default (grk_amd_set_decode_pixel_layout; as DwtLevelArgs):
    // sample (x, y) of component k of tile t of the window goes to pixels + t * px_tile + y * px_row + k * px_kstep + x * px_xstep
    // (bytes); interleaved pixels with more samples in memory than components: the others receive px_fill
    uint32_t px_lay, px_chan, px_xstep, px_fill;
    uint64_t px_row, px_kstep, px_tile;
};
// sh: the level's shape (plan_idwt_level, decode_plan.h) -- which kernel instance, its strips and row segments; a.seg_pairs, the
// sub-grid and the window = sh's
hipError_t launch_idwt_level(const IdwtLevelArgs& a, const IdwtLevelShape& sh, hipStream_t s);
hipError_t launch_idwt_level0_fused(const IdwtLevelArgs& a0, const IdwtLevelShape& sh, uint32_t ntiles, uint32_t ncomp, hipStream_t s);

// ---- K7: inverse colour transform + DC shift + clamp + store as pixels (kernels_idwt.hip) --------
struct EgressArgs {
    const int32_t* planes;   // [tile][comp] planes (float bit patterns when irreversible)
    void*    pixels;         // tiles back to back, component-major planar, tight -- or as px_lay .. px_tile say
    uint32_t w, h, stride;
    uint64_t pitch;
    uint32_t ncomp, ntiles;
    uint32_t bytes_per_sample;   // 1, 2 or 4 (int32 out)
    int32_t  dc, lo, hi;
    int      mct, irreversible;
    uint32_t px_lay, px_chan, px_xstep, px_fill;       // a layout other than the default (as IdwtLevelArgs)
    uint64_t px_row, px_kstep, px_tile;
};
hipError_t launch_egress(const EgressArgs& a, const EgressKey& key, hipStream_t s);     // key: egress_key (decode_plan.h)

// ---- KT1 / KT2: Tier-2 on the device (kernels_t2.hip) -------------------------------------------------------------------------
struct T2HeaderArgs {
    const T2Packet* packets; uint32_t npackets;      // a tile's packets in progression order (geometry.h)
    const uint32_t* lengths;                         // the call's table: [tile][row]
    uint32_t bpt, ntiles;                            // rows per tile
    uint32_t* ubits; uint32_t u_words;               // raw header bits, per tile, ZEROED by the caller
    uint8_t*  hdr;   uint32_t h_bytes;               // stuffed headers, per tile
    uint32_t* rel;                                   // [tile][row]: the block's offset in its packet's body
    uint32_t* pk_hdr; uint64_t* pk_body;             // [tile][packet]: header / body bytes
    unsigned int* status;                            // bit 2: a block length the writer does not take (>= 2^kT2MaxLenBits)
    // the general zero-bit-plane tree (NULL: the constant one): the rows' missing_msbs, [tile][row], and the node values' scratch,
    // per tile (T2Plan::v_bytes of a plan made for it).  Bit 4 of *status: a row above kT2MaxMsbs, written as if it were at it
    const uint8_t* msbs; uint8_t* nodes; uint32_t v_bytes;
};
hipError_t launch_t2_header(const T2HeaderArgs& a, uint32_t max_blocks_per_packet, hipStream_t s);
struct T2FrameArgs {
    uint32_t npackets, ntiles;
    const uint32_t* pk_hdr; const uint64_t* pk_body;
    const uint32_t* tile_index;                      // [tile]: Isot
    uint32_t extra;                                  // bytes per packet beside header and body (SOP 6, EPH 2)
    uint32_t plt;
    uint64_t dst_offset;                             // where the call's first tile-part goes in the output
    uint8_t* lit; uint32_t lit_stride;               // the frames, lit_stride bytes apart
    uint32_t* lit_len;                               // [tile]
    uint64_t* pk_dst;                                // [tile][packet]
    uint32_t* part_len; unsigned long long* tile_dst;   // [tile]: the tile-part's length and place (what a host or an exchange reads)
    unsigned long long* total;                       // [0] bytes assembled by this call, [1] the end of the output
    unsigned int* status;                            // bit 3: a tile-part beyond 4 GB / PLT beyond 256 marker segments
};
hipError_t launch_t2_frame(const T2FrameArgs& a, hipStream_t s);
struct T2GatherArgs {
    const T2Packet* packets; uint32_t npackets;
    const uint32_t* packet_of_block;                 // [row]
    const uint32_t* lengths; const uint64_t* offsets; const uint8_t* arena;
    uint32_t bpt, ntiles;
    const uint8_t* hdr; uint32_t h_bytes;
    const uint32_t* rel; const uint32_t* pk_hdr;
    const uint64_t* pk_dst;                          // [tile][packet]: where the packet starts in `out`
    const uint8_t* lit; uint32_t lit_stride; const uint32_t* lit_len;    // the tile-parts' frames (SOT .. SOD) as KT1b left them ...
    const unsigned long long* tile_dst;              // ... and where the tile-parts start in `out`
    uint8_t* out;
    uint32_t sop, eph;                               // 6 / 2 when the markers are written, else 0
};
hipError_t launch_t2_gather(const T2GatherArgs& a, hipStream_t s);

// ---- KT1p / KT1q / KT1r / KT2p: tiles divided into tile-parts (kernels_t2parts.hip) -------------------------------------------------
// Part k of every tile of the call holds the tile's packets [first, first + count) and has its frame (SOT with TPsot / TNsot / Psot,
// the PLT marker segments of its own packets, SOD) at frame_at bytes of the tile's frame scratch, part_frame_bound(count) of room
struct T2Part { uint32_t first, count, frame_at; };
struct T2PartsArgs {
    uint32_t npackets, ntiles, nparts;
    const T2Part* parts;                             // [part]: the same division for every tile of the call
    const uint32_t* pk_hdr; const uint64_t* pk_body; // [tile][packet], KT1's
    const uint32_t* tile_index;                      // [tile]: Isot
    uint32_t extra, plt;                             // as T2FrameArgs
    uint64_t dst_offset;
    uint8_t* lit; uint32_t lit_stride;               // the tiles' frame scratch
    uint32_t* lit_len;                               // [tile][part]: the frame's bytes
    uint32_t* tp_len; unsigned long long* tp_dst;    // [tile][part]: the part's length (Psot) and its place in the output
    uint64_t* pk_dst;                                // [tile][packet]
    uint32_t* part_len; unsigned long long* tile_dst;   // [tile]: the tile's SPAN -- all its parts, which lie one behind the other
    unsigned long long* total;
    unsigned int* status;                            // bit 3: a part or a tile's span beyond 4 GB / PLT beyond 256 marker segments in a part
};
hipError_t launch_t2_part_frames(const T2PartsArgs& a, hipStream_t s);     // KT1p
hipError_t launch_t2_part_places(const T2PartsArgs& a, hipStream_t s);     // KT1q
hipError_t launch_t2_part_packets(const T2PartsArgs& a, hipStream_t s);    // KT1r
// KT2p: KT2 with ntiles x nparts frame items (g.lit_len: [tile][part]; g.tile_dst is not read)
hipError_t launch_t2_gather_parts(const T2GatherArgs& g, const T2Part* parts, uint32_t nparts, const unsigned long long* tp_dst, hipStream_t s);

// ---- KK: a batch's table and coded bytes into image-wide tables and an image-wide arena (kernels_t2keep.hip) -----------------------
struct T2KeepArgs {
    const uint32_t* lengths; const unsigned long long* offsets;   // the batch's table: [unit][row], nunits x bpu entries
    const uint8_t* arena;                            // the batch's coded bytes, from a 16-byte boundary
    uint64_t arena_bound;                            // what the image's arena was sized for: at most this many bytes of the batch, a
                                                     // multiple of 16 inside the batch's arena (more in use: bit 0 of *status)
    const unsigned long long* batch_state;           // K3's allocator state: [0] status bits, [1] bytes of the arena in use
    uint32_t nunits, bpu;                            // the batch's units, rows per unit
    const unsigned long long* row_at;                // [unit]: its first row in the image's tables
    uint32_t* j_lengths; unsigned long long* j_offsets;   // the image's tables
    uint8_t* j_arena; uint64_t j_cap;                // the image's arena (16-byte aligned) and its size
    unsigned long long* cursors;                     // [0] where this batch's bytes go (a multiple of 16), [1] written: where the next one's go
    unsigned int* status;                            // the image's status word: the batches' OR-ed
    uint32_t grid;                                   // set by the launcher: workgroups
    // j_msbs != NULL: the rows' zero bit-planes as well, a byte each -- drop_missing_msbs (encode_plan.h) of the drop bytes the batch
    // was coded with (batch order; NULL: a plain launch, nothing dropped) under the Kmax of the batch's block descriptors [bpu]
    const uint8_t* drops; const HtBlockDesc* blocks; uint8_t* j_msbs;
};
hipError_t launch_t2_keep(const T2KeepArgs& a, hipStream_t s);
// msbs[i] = the zero bit-planes of row i of a table of n rows, bpt per tile, coded with drops[i] (as KK makes them): for a call whose
// rows stay where the block coder left them (grk_amd_assemble_rate_device)
hipError_t launch_t2_drop_msbs(const uint8_t* drops, const HtBlockDesc* blocks, uint32_t bpt, uint64_t n, uint8_t* msbs, hipStream_t s);

// ---- KG / KP: the device's share of reading a whole codestream (kernels_t2dec.hip) ----------------------------------------------
// KG: moves[i] = len bytes from src + moves[i].src to dst + moves[i].dst (the host checked them against both buffers)
hipError_t launch_t2dec_gather(const grk_amd_tp_segment* d_moves, uint64_t nmoves, const uint8_t* src, uint8_t* dst, hipStream_t s);
struct PlaceArgs {
    const uint8_t* tiles;                            // ntiles tiles of ncomp x h x w samples of bps bytes, back to back
    uint32_t ntiles, w, h, ncomp, bps;
    const int32_t* rects;                            // [tile]: x, y of the tile in the image's planes; signed: a tile may start left of /
                                                     // above them, and what lies outside img_w x img_h is not written (clipped)
    uint8_t* image; uint32_t img_w, img_h;           // ncomp planes of img_h x img_w samples (< 2^31 each)
    uint64_t img_row, img_plane;                     // bytes between the image's rows / planes (0: tight).  Interleaved pixels are
                                                     // placed as ONE component of samples as wide as a pixel
};
hipError_t launch_t2dec_place(const PlaceArgs& a, hipStream_t s);
// KU: placement of sub-sampled components with upsampling to the reference grid.  nunits tile-components groups ("units") of
// ncomp x h x w samples lie back to back, tight, as for KP; unit u's first sample is sample (origins[2 u], origins[2 u + 1]) of
// its component.  Sample (i, j) of a component fills its FOOTPRINT [i dx, (i + 1) dx) x [j dy, (j + 1) dy) of the reference grid,
// clipped to the image area [x0, x0 + img_w) x [y0, y0 + img_h): the footprints, not the tile rectangles, partition the image.
// The host checked that every footprint starts inside the image area.
struct UpsampleArgs {
    const uint8_t* tiles;
    uint32_t nunits, w, h, ncomp, bps;
    const uint32_t* origins;
    uint32_t dx, dy;
    uint8_t* image;                                  // the first of the unit's components, at the image area's top-left sample
    uint32_t x0, y0, img_w, img_h;
    uint64_t xstep, img_row, img_plane;              // bytes between a row's samples, rows, the unit's components in the image
};
hipError_t launch_t2dec_upsample(const UpsampleArgs& a, hipStream_t s);
// `value` into the samples of w x h at (x, y) of one component of such an image: the strip no sample's footprint covers when the
// image origin is no multiple of a factor, and the samples beyond num_comps of interleaved pixels
struct FillArgs { uint8_t* image; uint32_t x, y, w, h, bps, value; uint64_t xstep, img_row; };
hipError_t launch_t2dec_fill(const FillArgs& a, hipStream_t s);
// *into |= *from (assign: = ) on the stream: a group's decode status into the image's
hipError_t launch_t2dec_or_status(unsigned int* into, const unsigned int* from, bool assign, hipStream_t s);

// ---- KS / KD: units between a video surface and tight unit planes (kernels_surface.hip) ----------------------------------------
// nunits units of ncomp x h x w samples of bps (1 or 2) bytes lie back to back, tight, component-major at `tiles`; unit u's first
// sample is sample (origins[2 u], origins[2 u + 1]) of each component, and sample (x, y) of component k lies at
// surface + comp[k].offset + y * comp[k].row_pitch + x * comp[k].step * bps.  The host checked every sample against the surface's size.
// KS (cut) reads the surface and writes the tiles; KD (place) the reverse, writing no byte of the surface that is no sample.
// comp[k].shift (< 8 bps): the zero bits below a sample in its container -- KS reads word >> shift, KD writes v << shift.
// pair (KD, set by the launcher): ncomp = 2 components of step 2 and one pitch, one sample apart (one-byte samples: no shift;
// two-byte samples: every address even) -- both rows leave merged, in 16-byte stores
struct SurfaceKernelComp { uint64_t offset, row_pitch; uint32_t step, shift; };
struct SurfaceArgs {
    uint8_t* surface; uint8_t* tiles;
    uint32_t nunits, w, h, ncomp, bps;
    const uint32_t* origins;
    SurfaceKernelComp comp[4];
    uint32_t pair;
};
hipError_t launch_surface_cut(const SurfaceArgs& a, hipStream_t s);
hipError_t launch_surface_place(const SurfaceArgs& a, hipStream_t s);

// ---- KU / KK: a packed 4:2:2 frame (packed_format.h) and its three tight planes (kernels_packed.hip) ---------------------------
// Row r of the frame starts at packed + r * pitch; y is w x h, cb and cr ceil(w / 2) x h, tight, LSB-aligned samples of one byte
// (prec <= 8) or two, at any address.  The host checked format, precision, the frame's alignment and every size (packed.cpp).
struct PackedArgs {
    uint8_t* packed; uint64_t pitch;
    uint8_t *y, *cb, *cr;
    uint32_t w, h, format, prec;
};
hipError_t launch_packed_unpack(const PackedArgs& a, hipStream_t s);
hipError_t launch_packed_pack(const PackedArgs& a, hipStream_t s);

// ---- KL / KH / KC: Tier-2 READ on the device (kernels_t2read.hip; the parse core: t2_parse.h, the plan: t2_read_plan.h) ----------
// cs: the codestream in device memory, `len` bytes; no byte outside it is read.  tiles / packets: the plan's, uploaded as they are.
// KL fills part_at / part_len ([tile]; a length of 0: not located), KH body_at ([tile]: behind SOD, 0: header refused), has_plt and
// -- with PLT -- plt_len / pk_start ([tile's pkt_base + packet]), KC every row of `rows`.  status: the call's word (t2_parse.h),
// set to kT2pNoStatus before KL.  KH and KC pass over tiles whose earlier stage left nothing.
struct T2ReadTile; struct T2ReadPacket;
struct T2ReadTlmEntry { uint64_t at; uint32_t ln, idx; };
struct T2ReadArgs {
    const uint8_t* cs; uint64_t len;
    uint32_t num_tiles;
    const T2ReadTile* tiles; const T2ReadPacket* packets;
    uint32_t ht, sop, eph;
    // KL: tlm_n entries from TLM (tlm != nullptr; tlm_count: all of TLM's), or the Psot chain from sot_at
    const T2ReadTlmEntry* tlm; uint32_t tlm_n; uint64_t tlm_count; uint64_t sot_at;
    uint32_t* first_of;                              // [tile] scratch
    unsigned long long* part_at; uint32_t* part_len; unsigned long long* body_at; uint32_t* has_plt;
    uint32_t* plt_len; unsigned long long* pk_start;
    uint8_t* nodes;
    grk_amd_coded_block* rows;
    unsigned long long* status;
    uint64_t chains;                                 // KC's grid
};
hipError_t launch_t2read_locate(const T2ReadArgs& a, hipStream_t s);
hipError_t launch_t2read_headers(const T2ReadArgs& a, hipStream_t s);
hipError_t launch_t2read_chains(const T2ReadArgs& a, hipStream_t s);

// ---- the general reader: several layers, several codeword segments (kernels_t2read_layers.hip) ----------------------------------------
// KL and KH run on `a` as they are (a.tiles: T2ReadLayersPlan's, whose npackets count every layer's); a.nodes is not used.
constexpr uint32_t kT2ReadScanRows = 256;            // rows per workgroup of KF
struct T2ReadLayerPk; struct T2pRowState; struct T2ReadSegRecord; struct T2ReadPieceRecord;
struct T2ReadLayersArgs {
    T2ReadArgs a;
    const T2ReadLayerPk* lpk;
    uint32_t layers, order, sty, seg_per_row, piece_per_row;
    uint32_t* nodes32; T2pRowState* state;
    T2ReadSegRecord* seg_log; T2ReadPieceRecord* piece_log;
    uint32_t* counts;                                // [chain][2]: records in its share of the two logs
    // KF, KP
    uint64_t nrows;
    uint32_t* first_segment;                         // [rows + 1]
    unsigned long long* app_at;                      // [rows]: a row of several pieces' place in the appendix
    uint32_t* move_first;                            // [rows]: its first move
    unsigned long long* sums;                        // [ceil(rows / kT2ReadScanRows)][3] scratch
    unsigned long long* totals;                      // [3]: segments, appendix bytes, moves
    grk_amd_segment* segments; uint64_t seg_cap;
    grk_amd_tp_segment* moves; uint64_t move_cap;
};
hipError_t launch_t2read_chains_layers(const T2ReadLayersArgs& g, hipStream_t s);
hipError_t launch_t2read_finish(const T2ReadLayersArgs& g, hipStream_t s);
hipError_t launch_t2read_place(const T2ReadLayersArgs& g, hipStream_t s);

// ---- tiles divided into tile-parts (KL-P, KH-P, KC-L over a tile's part table; KF and KP as above) ------------------------------------
// g.a.part_at / part_len / first_of and g.a.tlm are not used.  KH-P leaves in g.a.body_at[tile] a non-zero word for a tile whose headers
// were read, in g.a.has_plt[tile] whether it is a PLT tile (every tile-part that holds packets lists exactly its own).
struct T2ReadPartsArgs {
    T2ReadLayersArgs g;
    uint32_t cap;                                    // tile-parts the arrays below hold
    uint32_t n_given;                                // TLM: the file's tile-parts, fo_* filled by the host; 0: KL-P hops along Psot
    // [cap] in file order: where, how long, TLM's tile index (0xFFFFFFFF: TLM names none); KL-P's claim on a table slot
    unsigned long long* fo_at; uint32_t* fo_len; uint32_t* fo_idx; uint32_t* claim;
    // [tile]: its tile-parts, its smallest and largest non-zero TNsot; [tiles + 1]: its slice of the part table
    uint32_t* count; uint32_t* tn_min; uint32_t* tn_max; uint32_t* slice;
    // the part table, [cap]: a tile's tile-parts at slice[tile] + TPsot
    unsigned long long* tp_at; uint32_t* tp_len; uint32_t* tp_tile; uint32_t* tp_file;
    unsigned long long* tp_body; uint32_t* tp_has_plt; uint32_t* tp_npk; uint32_t* tp_first;
    unsigned long long* located;                     // [1]: the tile-parts found
};
hipError_t launch_t2read_locate_parts(const T2ReadPartsArgs& p, hipStream_t s);
hipError_t launch_t2read_headers_parts(const T2ReadPartsArgs& p, uint32_t nparts, hipStream_t s);
hipError_t launch_t2read_chains_parts(const T2ReadPartsArgs& p, hipStream_t s);

} // namespace grk_amd
