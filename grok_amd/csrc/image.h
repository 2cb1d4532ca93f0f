// grok_amd/csrc/image.h -- the steps every whole-image encoder takes (grk_amd_encode_image, grk_amd_encode_image_subsampled,
// grk_amd_node_encode_image; private to the library, defined in image.cpp): cut the image into units, group them by geometry, stage
// each group's pixels, code each group as one grk_amd_encode_tiles batch, frame the file.  The header itself is HIP-free, and so are
// the homes of what the host planners (decode_image_plan.cpp, surface_plan.cpp, t2_reader.cpp) take from it: add_unit lives in
// geometry.cpp, parallel_for in host_common.cpp; the whole-image decode's planning is decode_image_plan.h.
#pragma once
#include "../../include/grok_amd.h"
#include "geometry.h"
#include <functional>
#include <vector>

#pragma GCC visibility push(hidden)       // nothing declared below is part of the library's interface
namespace grk_amd {

// A unit of coding: a tile, or a run of a tile's components of one size (sub-sampled images) -- its parameters and its first
// component in the caller's image
struct Unit { grk_amd_tile_params p; uint32_t c0; };

// The run rule of images with sub-sampled components (SIZ XRsiz / YRsiz), for the encoders, the plugin's tile trees and
// grk_amd_decode_image alike: consecutive components with equal factors form a run, which is coded and decoded as one unit of
// `count` components.  mct: the run that starts at component 0 and holds at least three components of an image that signals
// the colour transform -- the only place where the transform can apply.
struct CompRun { uint32_t first, count; bool mct; };
inline std::vector<CompRun> comp_runs(uint32_t num_comps, bool mct, const uint8_t* comp_dx, const uint8_t* comp_dy)
{
    std::vector<CompRun> runs;
    for (uint32_t c0 = 0, n; c0 < num_comps; c0 += n) {
        n = 1;
        while (c0 + n < num_comps && comp_dx[c0 + n] == comp_dx[c0] && comp_dy[c0 + n] == comp_dy[c0]) ++n;
        runs.push_back(CompRun{c0, n, mct && c0 == 0 && n >= 3});
    }
    return runs;
}

// The caller's image: component c's samples start comp[c].at bytes into `px`, in rows of comp[c].w samples, the first of
// them at (comp[c].x0, comp[c].y0) on the component's grid.  Under a pixel layout (grk_amd_set_pixel_layout; plain_image) rows lie
// row_pitch bytes apart (0: tight) and, with channels != 0, the components are interleaved: channels samples per pixel in memory
struct SourcePlanes {
    const uint8_t* px;
    uint32_t bps;                                  // bytes per sample
    struct Plane { uint64_t at, w, x0, y0; };
    std::vector<Plane> comp;
    uint64_t row_pitch = 0;
    uint32_t channels = 0;
};

struct UnitGroups {
    std::vector<TileGeom> geoms;                   // [group]: its first unit's geometry
    std::vector<uint32_t> of;                      // [unit]: its group
    std::vector<std::vector<uint32_t>> members;    // [group]: its units in unit order
};

// the next unit, of parameters `p`, into its group: the first whose num_comps, mct and geometry (same_geometry) it shares -- one
// batch of grk_amd_encode_tiles --, or a new one.  GRK_AMD_OK or build_tile_geom's error.
// `order`: the progression order of a caller whose groups are also framed as one batch each (grk_amd_assemble_device: one packet
// sequence, the first unit's, for the whole batch) -- from RPCL on a group's units share their packet sequence too (same_packets).
// 0 for everybody whose Tier-2 is per tile: the decoders, the rate and surface paths.
int add_unit(UnitGroups& g, const grk_amd_tile_params& p, uint32_t order = 0);

// A plain image (component-major planar, tight, W x H per component): one unit per tile with all components, grouped by geometry
// and by the packet sequence of the progression order in `flags` (add_unit).
// A file with TLM holds at most 255 tiles (one-byte Ttlm): GRK_AMD_ERR_UNSUPPORTED before any work.
// `lay` (or null: that default): the layout of `pixels`, row_pitch the image's; GRK_AMD_ERR_INVALID when it does not fit the image.
int plain_image(const grk_amd_image_layout* im, const grk_amd_tile_params* base, const void* pixels, uint32_t flags,
                std::vector<Unit>& units, SourcePlanes& src, UnitGroups& g, const grk_amd_pixel_layout* lay = nullptr);

inline size_t unit_bytes(const Unit& u, uint32_t bps) { return (size_t)u.p.tile_w * u.p.tile_h * u.p.num_comps * bps; }
// ... as stage_units lays the unit out: an interleaved source keeps its samples per pixel
inline size_t staged_bytes(const SourcePlanes& src, const Unit& u)
{
    return src.channels ? (size_t)u.p.tile_w * u.p.tile_h * src.channels * src.bps : unit_bytes(u, src.bps);
}
// the layout grk_amd_encode_tiles reads what stage_units wrote in
inline grk_amd_pixel_layout staged_layout(const SourcePlanes& src)
{
    grk_amd_pixel_layout l{};
    if (src.channels) { l.interleaved = 1; l.channels = (uint8_t)src.channels; }
    return l;
}

// units[idx[i]]'s rows out of the source into `dst`, tight, component-major (an interleaved source: tight rows of whole pixels, one
// memcpy per row), unit i at i x staged_bytes (a group's units are of one
// size); each of `threads` threads copies its share of the rows of every unit component
void stage_units(const SourcePlanes& src, const std::vector<Unit>& units, const std::vector<uint32_t>& idx, uint8_t* dst, uint32_t threads);

// Every group through grk_amd_encode_tiles with its first unit's parameters, its table and coded bytes to the host: `rows` are the
// units' rows one after the other in unit order, their offsets into `coded` (the groups' bytes back to back).  What the host
// codestream writers take.
int encode_groups_host(grk_amd_ctx* ctx, const SourcePlanes& src, const std::vector<Unit>& units, const UnitGroups& g,
                       std::vector<grk_amd_coded_block>& rows, std::vector<uint8_t>& coded);

// The file around tile-parts of known sizes: main header (TLM from `part_len`), `body(at)` puts tile-part t at out + at[t]
// (at[ntiles]: their end), EOC.  The file's length, or the header writer's error (TLM over 255 tiles: GRK_AMD_ERR_UNSUPPORTED),
// GRK_AMD_ERR_OVERFLOW when `cap` cannot hold it, or the body's error.
// comp_dx / comp_dy (both or neither): the file of an image of sub-sampled components -- SIZ carries the factors, COD no colour
// transform unless components 0..2 share theirs (main_header_subsampled, t2_writer.cpp: the header grk_amd_write_codestream_subsampled writes)
// tp_bytes (tiles divided into tile-parts, GRK_AMD_CS_TP: nparts > 1 each): the parts' lengths in file order for TLM, nparts per tile;
// part_len[t] stays the tile's SPAN -- all its parts, which is what `body` places
int64_t frame_file(const grk_amd_image_layout* im, const grk_amd_tile_params* base, uint32_t flags, const std::vector<uint32_t>& part_len,
                   uint8_t* out, uint64_t cap, const std::function<int(const std::vector<uint64_t>& at)>& body,
                   const uint8_t* comp_dx = nullptr, const uint8_t* comp_dy = nullptr, uint32_t nparts = 1, const uint32_t* tp_bytes = nullptr);
int64_t main_header_subsampled(const grk_amd_image_layout* im, const grk_amd_tile_params* base, const uint8_t* comp_dx, const uint8_t* comp_dy,
                               uint32_t flags, const uint32_t* tile_part_bytes, uint8_t* out, uint64_t cap);
// the main header of a file of divided tiles (grk_amd_write_main_header_parts; comp_dx / comp_dy both or neither: main_header_subsampled's)
int64_t main_header_parts(const grk_amd_image_layout* im, const grk_amd_tile_params* base, const uint8_t* comp_dx, const uint8_t* comp_dy,
                          uint32_t flags, const uint32_t* parts_per_tile, const uint32_t* part_bytes, uint8_t* out, uint64_t cap);
// the header of either kind: nparts parts in every tile (1: the undivided file's header, tp_bytes the tiles' lengths)
int64_t main_header_any(const grk_amd_image_layout* im, const grk_amd_tile_params* base, const uint8_t* comp_dx, const uint8_t* comp_dy,
                        uint32_t flags, uint32_t ntiles, uint32_t nparts, const uint32_t* tp_bytes, uint8_t* out, uint64_t cap);

// ---- Tier-2 on the device for an image whose units are coded by several batches (assemble.hip) -------------------------------------
// The caller names the image's units -- unit t * nruns + k is run k (comp_runs) of tile t, `g` their geometry groups -- and its batches,
// each one grk_amd_encode_tiles call over units of one group, and lends front(b): batch b's pixels where they have to be and the
// call made, without a table (nothing comes to the host).  encode_joint_device keeps every batch's rows and bytes on the device
// (KK, kernels_t2keep.hip), frames the tiles class by class (t2_order.h: joint_tile_classes, t2_device_plan_joint) with the kernels
// of grk_amd_assemble_device, and delivers the file: to `out` (main header and EOC written by the host, the tile-parts fetched), or
// with d_file != nullptr SOC .. EOC contiguous in device memory of the context's, valid until its next encode call (`out`, `cap`
// unused).  The file's length, GRK_AMD_ERR_UNSUPPORTED where the device writer does not reach (GRK_AMD_CS_BLOCK_MSBS, tables beyond
// its fields, TLM over 255 tiles) -- before any batch is coded --, or an error.
struct JointT2Call {
    const grk_amd_image_layout* im; const grk_amd_tile_params* base; const uint8_t* comp_dx; const uint8_t* comp_dy; uint32_t flags;
    uint32_t nruns; const UnitGroups* g;
    std::vector<std::vector<uint32_t>> batches;
    std::function<int(size_t b)> front;
};
int64_t encode_joint_device(grk_amd_ctx* ctx, const JointT2Call& call, uint8_t* out, uint64_t cap, void** d_file);
// encode_joint_device in its three parts, for a caller that codes the batches itself -- the rate- and quality-targeted calls that leave
// their file in device memory (rate.hip: every round codes every batch again, with the drops the allocator chose):
//   joint_device_open     the classes' plans and the image's buffers, the cursors at zero
//   joint_device_reset    the cursors at zero again: before a further round's first batch
//   joint_device_keep     batch b, just coded by the caller, kept in the image's tables and arena (KK)
//   joint_device_finish   the classes framed, the file delivered as encode_joint_device delivers it
// msbs: the rows' zero bit-planes are written -- KK makes them from the drops a batch was coded with, KT1's general instance writes
// their tag trees (plans of t2_device_plan_joint_msbs); asked for here, never through GRK_AMD_CS_BLOCK_MSBS in call.flags.
struct JointT2Run {
    grk_amd_ctx* c; const JointT2Call* call; bool msbs;
    uint32_t ntiles = 0; size_t nb = 0; int64_t hdr_bytes = 0;
    std::vector<uint64_t> rowlist{}, batch_at{};
    uint64_t bound_at = 0;                                   // the kept batches' arena bounds so far
    std::vector<uint32_t> part_len{};
    uint32_t nparts = 1;                                     // tile-parts per tile (GRK_AMD_CS_TP) ...
    std::vector<uint32_t> tp_len{};                          // ... and their lengths in file order, for TLM: [tile][part]
};
int joint_device_open(JointT2Run& r);
int joint_device_reset(JointT2Run& r);
int joint_device_keep(JointT2Run& r, size_t b);
int64_t joint_device_finish(JointT2Run& r, uint8_t* out, uint64_t cap, void** d_file);
// GRK_AMD_CS_TP as a whole-image call meets it, before any work: the tile-parts per tile (1: none), or the refusal with its reason in the
// context -- the rule's (t2_order.h: tile_part_count), or with TLM more parts in the file than one marker segment lists
int image_division(grk_amd_ctx* c, uint32_t flags, const grk_amd_tile_params* base, uint32_t ntiles);
// the tile-parts' lengths of the latest grk_amd_assemble_device call (its table 3: [tile][grk_amd_assembled_parts]) to the host
int assembled_part_bytes(grk_amd_ctx* c, uint32_t ntiles, uint32_t* out);
// GRK_AMD_IMAGE_T2=host, read per call: the whole-image encoders write their files with the host writer
bool image_t2_host();

// An image of sub-sampled components (grk_amd_encode_image_subsampled's `pixels`: the components back to back, tight) cut into units
// -- tile by tile, within a tile run by run (comp_runs) -- and grouped.  GRK_AMD_ERR_UNSUPPORTED under a pixel layout of the caller's
// (components of different sizes have no interleaved form), GRK_AMD_ERR_INVALID for a factor of 0, else the layout's errors.
int subsampled_image(grk_amd_ctx* ctx, const grk_amd_image_layout* im, const grk_amd_tile_params* base, const uint8_t* comp_dx,
                     const uint8_t* comp_dy, const void* pixels, std::vector<Unit>& units, SourcePlanes& src, UnitGroups& g);

// ---- a whole image in a file of at most N bytes, or in the fewest bytes for a distortion, over joint tables (rate.hip) --------------
// The caller names the image's units (unit_blocks[u]: unit u's rows, in the order the file's writer takes the table) and its
// batches -- each one grk_amd_encode_tiles call over units of one geometry -- and lends two steps:
//   front(k, table, total)        batch k's pixels staged where they have to be and coded plainly: grk_amd_encode_tiles with these
//                                 `table` (host rows or null) and `total`; called once for the tables and again before a round's
//                                 final launch whenever another batch's planes have taken the context since
//   write(rows, coded, out, cap)  the file of these rows (joint order; offsets into `coded`), or with out == nullptr its length
// encode_rate_joint is a run (RateRun, rate.hip: the one path every rate- and quality-targeted call takes to its tables and its
// coded blocks) over all units through the batches' maps (plan_rate_joint): the tables L, E, W made once, KR2 once per round over
// them -- one multiplier for every block of the image --, each batch coded with its slice of the chosen drops and merged into the
// file's rows; the rounds are rate_rounds' (rate.hip), shared with the split route.  Returns the file's length or an error.
// The call's goal is bytes (rate->target_bytes, the rounds above), or -- quality != nullptr -- a distortion budget: the same tables,
// then KQ once over them, every batch coded with its slice of the drops and the file written once; no rounds (headers do not enter a
// distortion budget).  rate then carries max_drop and allow_skip only (QualityTarget makes both from a grk_amd_quality), and the
// result goes to quality->result.
struct RateBatch { grk_amd_tile_params p; std::vector<uint32_t> units; };
struct QualityGoal { double budget, signal; grk_amd_quality_result* result; };       // plan_quality's D and S peak^2 (encode_plan.h)
struct RateJointCall {
    const grk_amd_tile_params* base; const grk_amd_rate* rate;
    std::vector<uint64_t> unit_blocks; std::vector<RateBatch> batches;
    std::function<int(size_t k, grk_amd_coded_block* table, uint64_t* total)> front;
    std::function<int64_t(const grk_amd_coded_block* rows, const uint8_t* coded, uint8_t* out, uint64_t cap)> write;
    const QualityGoal* quality = nullptr;
};
// unit_blocks, batches and front of a planar image's call (plain_image's or subsampled_image's units, source and groups: one batch
// per group, staged into `staging`); the caller adds `write`.  Everything passed is referred to, `call` included
void planar_rate_call(grk_amd_ctx* ctx, const std::vector<Unit>& units, const SourcePlanes& src, const UnitGroups& g,
                      std::vector<uint8_t>& staging, RateJointCall& call);
// What every rate- or quality-targeted call refuses before any work: pipelining (GRK_AMD_ERR_UNSUPPORTED), max_drop above 12
// (GRK_AMD_ERR_INVALID).  goal: "rate" or "quality", the word the messages name the call and its struct by
int rate_refusal(grk_amd_ctx* ctx, const grk_amd_rate* rate, const char* goal = "rate");
// A grk_amd_quality checked and turned into what the joint call takes: GRK_AMD_OK, or rate_refusal's answer, or GRK_AMD_ERR_INVALID
// for a target plan_quality refuses.  The tables of an earlier call are invalid from here on, refused or not.
// samples: S of the call (quality_samples, encode_plan.h)
struct QualityTarget { grk_amd_rate rate; QualityGoal goal; };
int quality_target(grk_amd_ctx* ctx, const grk_amd_quality* quality, uint32_t prec, uint64_t samples, grk_amd_quality_result* result,
                   QualityTarget& out);
int64_t encode_rate_joint(grk_amd_ctx* ctx, const RateJointCall& call, uint8_t* out, uint64_t cap, grk_amd_rate_result* result);
// The same call with Tier-2 on the device and the file left in device memory (*d_file: SOC .. EOC, the context's, valid until its next
// encode call): the run drives the parts of encode_joint_device (JointT2Run with msbs) in place of code_all / merge -- per round the
// image's cursors reset, every batch coded with its slice of the drops and kept by KK with its rows' zero bit-planes, the classes framed.
// A round's file length is the device's total; the plain file is sized on the host from the plain rows (call.write with out == nullptr
// and no coded bytes).  Budgets and results are encode_rate_joint's.  t2: the image as encode_joint_device takes it, its batches the
// units of call.batches in the same order (t2.front is not used: the run codes).  No coded byte comes to the host.
int64_t encode_rate_joint_device(grk_amd_ctx* ctx, const RateJointCall& call, const JointT2Call& t2, void** d_file, grk_amd_rate_result* result);

// fn(i) for i in [0, n) on up to `threads` host threads, the caller's among them; items are handed out by a counter and the
// first error wins (no item starts after it)
int parallel_for(size_t n, uint32_t threads, const std::function<int(size_t)>& fn);

} // namespace grk_amd
#pragma GCC visibility pop
