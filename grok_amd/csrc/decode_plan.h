// grok_amd/csrc/decode_plan.h -- what a decode call works out on the host before it launches anything: which blocks a window
// needs, which rows of the caller's table are sound, which block goes to which decoder.  Plain integer code over a block table
// and a TileGeom, and the shape of each inverse DWT level: no HIP, no grk_amd_ctx, so that a plain C++ compiler builds it and tests/c/decode_plan_units.cpp steps through
// it without a GPU.  A planner that can refuse returns a GRK_AMD_* code and leaves the reason in *why; the caller reports it.
#pragma once
#include "decode_constants.h"
#include "dwt_instances.h"
#include "geometry.h"
#include <cstddef>
#include <cstdint>
#include <vector>

#pragma GCC visibility push(hidden)       // private to the library, like everything in context.h
namespace grk_amd {

// ---- region decode ---------------------------------------------------------------------------------------------------------------
// Region decode (the reference: grk_decompress_set_window -> WaveletReverse.cpp:1466-2213 partial
// synthesis over a sparse buffer).  need[l] = the part of LL_l (l = 0: the image) that has to be right so that the
// window is; level l is synthesised from the coefficient pairs pairs[l] of LL_{l+1} and of resolution L - l's bands.
// A synthesised sample depends on the pairs within 1 (5/3) or 2 (9/7) of its own, the kernel's strip halo and the
// recurrence warm-up reach 2 pairs further: the margins are conservative on purpose.
struct Rect { uint32_t x0, y0, x1, y1; };
struct RegionPlan { std::vector<Rect> need, pairs; std::vector<uint32_t> px, py; };
RegionPlan plan_region(const TileGeom& g, Rect win);
// the blocks no sample of the window depends on: their rows (one tile's, [comp][block]) become {0, 0, kSkipBlock}
void skip_blocks_outside(const TileGeom& g, const RegionPlan& plan, grk_amd_coded_block* rows);

// ---- the block table -------------------------------------------------------------------------------------------------------------
// every row inside the coded buffer, or GRK_AMD_ERR_INVALID
int check_table(const grk_amd_coded_block* table, uint64_t nblocks, uint64_t coded_bytes, const char** why);
// ... and for the HT decoder: the longest block (GRK_AMD_ERR_UNSUPPORTED above 48 KiB) and the blocks that have data at all, in
// table order -- K5a's lanes (a window's skipped blocks and absent blocks do not cost a lane of a serial chain); `active` has room
// for nblocks entries
int plan_ht_blocks(const grk_amd_coded_block* table, uint64_t nblocks, uint64_t coded_bytes, uint32_t* active, uint32_t* nactive,
                   uint32_t* max_len, const char** why);

// ---- codeword segments -------------------------------------------------------------------------------------------------------------
// A segment list as the kernels' launchers take it: first[nblocks + 1] into segs; nfirst == 0: none was set
struct SegList { const uint32_t* first = nullptr; size_t nfirst = 0; const grk_amd_segment* segs = nullptr; size_t nsegs = 0; };
// the list over the full tile's blocks -> the kept blocks' segments, in the order of the kept rows: each of `groups` components keeps
// its first kept_per_comp of full_per_comp blocks
int reduce_segments(uint64_t groups, uint32_t full_per_comp, uint32_t kept_per_comp, const std::vector<uint32_t>& first,
                    const std::vector<grk_amd_segment>& segs, std::vector<uint32_t>& red_first, std::vector<grk_amd_segment>& red_segs,
                    const char** why);
// the list that applies to a call of nblocks rows (the reduced one for a reduced geometry), checked against that number
int select_segments(bool reduced, const std::vector<uint32_t>& first, const std::vector<grk_amd_segment>& segs,
                    const std::vector<uint32_t>& red_first, const std::vector<grk_amd_segment>& red_segs, uint64_t nblocks,
                    SegList* out, const char** why);
// HT blocks with refinement passes: segment 0 = the cleanup pass, segment 1 = SigProp (+ MagRef), end to end.  ref[nblocks] =
// {bytes of the refinement segment, coding passes in total (1..3)}
int plan_ht_refinement(const grk_amd_coded_block* table, uint64_t nblocks, const SegList& sl, grk_amd_segment* ref,
                       uint32_t* max_refine_bytes, const char** why);

// A decode call keeps its Mallat planes in int16: the caller's setting (grk_amd_set_decode_planes16) and not the exact repeat of a
// call that left them, the fused last level, a reversible HT tile of at most 8 bits -- and no segment list on the context: K5c
// refines the int32 sign-magnitude words K5b leaves in the plane
bool decode_takes_planes16(bool setting, bool force32, bool fuse_out, const grk_amd_tile_params& p, bool have_segments);

// ---- the Part-1 launch lists -----------------------------------------------------------------------------------------------------
struct T1PlanIn {
    const grk_amd_coded_block* table; uint64_t nblocks;
    const uint16_t* block_h; uint32_t blocks_per_tile;      // the heights of a tile's blocks, [blocks_per_tile]
    uint32_t cblksty;                    // COD code-block style bits: the lane decoder takes the default style only
    int t1_lanes; bool pass_sync;        // grk_amd_ctx::t1_lanes, t1_pass_sync
    bool have_segments;                  // a segment list is set: K8 alone reads it
};
struct T1Lists {
    uint32_t n_lane = 0, n_tail = 0;     // entries of lane (kT1NoBlock: a spare lane) and tail; both 0: K8 takes every block in table order
    uint32_t buckets = 0;                // entries of the length sort's table (0: no lists were tried)
};
// lane: room for 2 nblocks entries (padding), tail: for nblocks.  GRK_AMD_ERR_NOMEM when the host has no memory for the sort
int plan_t1_lists(const T1PlanIn& in, uint32_t* lane, uint32_t* tail, T1Lists* out, const char** why);

// ---- the shape of an inverse DWT level -------------------------------------------------------------------------------------------
struct IdwtLevelDesc {                 // (the fields of IdwtLevelArgs the shape depends on)
    uint32_t cw, ch, px, py;
    uint32_t ll_stride, m_stride, out_stride;
    bool h16, pk, irreversible;
    uint32_t zslots;                   // workgroups along z: planes, or for the fused last level tiles (x level_part_zslots)
    bool region; Rect need;            // a region decode: the part of the level that has to be right (RegionPlan::need[l])
    // the last level fused with K7: the rows leave as the caller's pixels
    bool fused; uint32_t px_bytes; int32_t lo, hi; bool mct;
    uint32_t px_lay, px_chan; uint64_t px_row, px_tile;
    uint32_t px_align;                 // the low two bits of the (device) pixel pointer
};
struct IdwtLevelShape {
    bool packed;                       // the level shape idwt53_pk_kernel takes
    uint32_t strip_pairs;              // coefficient pairs a workgroup of that kernel owns
    uint32_t seg_pairs;                // row pairs per workgroup
    uint32_t grid_x, grid_y;           // strips (of inst[0]: the fused level's parts can differ), row segments
    uint32_t strip0, nstrips, seg0, nsegs;     // region decode: the sub-grid that produces `need` (0 = all)
    uint32_t wx0, wy0, wx1, wy1;       // the window of the level the pixels are for
    IdwtInstance inst[2];              // the kernel instance (dwt_instances.h) and its strips: of a part of one component [0] and, for
                                       // the fused level, of the MCT triple [1] (every other level: not used, in no list)
};
IdwtLevelShape plan_idwt_level(const IdwtLevelDesc& d);
// the stand-alone K7's instance
EgressKey egress_key(uint32_t px_lay, uint32_t bytes_per_sample, uint32_t ncomp);

} // namespace grk_amd
#pragma GCC visibility pop
