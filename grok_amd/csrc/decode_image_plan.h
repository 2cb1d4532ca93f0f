// grok_amd/csrc/decode_image_plan.h -- the host planning of grk_amd_decode_image / _view / grk_amd_decode_surface (HIP-free; private
// to the library, defined in decode_image_plan.cpp and tested on the CPU through tests/c/decode_image_plan_units.cpp).  Every
// decision and every offset of a whole-image decode is made here, on top of image_view_plan.h (which tiles, what every unit
// delivers) and surface_plan.h (a surface's planes and routes); decode_image.cpp carries the plans out.  A planner returns
// GRK_AMD_OK, or the refusal's code and in *why its reason.
#pragma once
#include "../../include/grok_amd.h"
#include "image.h"
#include "image_view_plan.h"
#include "pixel_layout.h"
#include "surface_plan.h"
#include "t2_reader.h"
#include <vector>

#pragma GCC visibility push(hidden)
namespace grk_amd {

// ---- the destination ---------------------------------------------------------------------------------------------------------
// what the plan takes from the context and the call
struct ImageDestIn {
    grk_amd_pixel_layout layout{};      // the decode pixel layout (grk_amd_set_decode_pixel_layout)
    bool upsample = false;              // grk_amd_set_decode_upsample
    bool pixels_on_device = false;
    uint64_t cap = 0;
    uint32_t dst_align = 0;             // the device destination's address modulo 4 (host pixels: the context's own copy, 0)
    bool surface_direct = true;         // a surface's runs may be decoded in place (GRK_AMD_SURFACE_DIRECT)
    bool ht_refine = false;             // the packets are read and HT blocks among them have refinement passes (table_has_second_segment)
};

enum class ImageRoute {
    Direct,         // one tile, all of it: grk_amd_decode_tiles straight into the caller's pixels
    Region,         // one tile, a window of it: grk_amd_decode_region
    Runs,           // one tile of several runs: run by run into the run's planes
    Staged,         // groups into staging, then KP (the view's image, or -- `sub` -- the components' planes) or KU (`up`)
    Surface,        // a surface: runs in place through a layout, the other units staged and placed by KD
};

struct ImagePlane { uint64_t at, w, h, x0, y0; };          // (x0, y0: the component's first sample at full size, for KU)
struct FillRect { uint32_t comp, x0, y0, w, h, value; };   // KU's fills: channel `comp` of the image, ImageDest::kstep apart
// a run of a one-tile image on the Runs route: its planes at `at`; beside: a device destination off the 4-byte alignment of the
// decoder's pixel stores -- the run is decoded beside it and copied
struct RunDest { uint64_t at, bytes; bool beside; };

// A launch of the route's placement kernel (KP, KU, KD) for a batch's units [seg.first, seg.first + seg.count), all of run seg.run
struct ImageLaunch {
    RunSegment seg;
    uint64_t at = 0;                        // (KP, KU) the target's first byte in the image: the view's image, the run's first plane
    uint32_t ncomp = 0, bps = 0;            // components and bytes of a sample as the kernel sees them (whole pixels: one component)
    uint32_t w = 0, h = 0;                  // the target's planes
    uint64_t row = 0, kstep = 0;            // bytes between its rows / planes (KP: 0 = tight)
    uint32_t dx = 1, dy = 1;                // (KU) the run's factors
};

// One batch of grk_amd_decode_tiles.  Staged: a geometry group; Surface: the group's in-place units one by one (each through
// surf_route[unit % nr]), then its staged units as one batch
struct ImageGroup {
    grk_amd_tile_params p;                  // the batch's parameters
    std::vector<uint32_t> in_place;         // (Surface) units decoded straight onto the surface
    std::vector<uint32_t> units;            // the staged batch, run by run
    uint32_t uw = 0, uh = 0;                // a staged unit at the view's reduce
    uint64_t unit_size = 0;                 // ... and its bytes in staging
    bool skip = false;                      // nothing of the units is left at this reduce
    uint64_t place_at = 0;                  // the batch's first entry in `places` (pairs)
    std::vector<ImageLaunch> launches;      // the placement launches
};

struct ImageDest {
    ImageRoute route = ImageRoute::Staged;
    bool sub = false, up = false, ht = false, want_segs = false, all = false;
    uint32_t bps = 0, nr = 0;
    uint64_t W = 0, H = 0;                  // the view's image (upsampled: the image area)
    PixelLayout ipx{};                      // ... in the context's decode layout
    uint64_t kstep = 0;                     // (KU) from one channel of the image to the next
    std::vector<ImagePlane> plane;          // [component]
    ResolvedSurface rs;                     // (Surface)
    std::vector<SurfaceRoute> surf_route;   // (Surface) [run]
    uint64_t total = 0;                     // the destination's bytes
    std::vector<grk_amd_tile_params> tp;    // [touched tile][run]
    UnitGroups g;                           // the units by geometry, a group's units run by run
    uint32_t region[4] = {0, 0, 0, 0};      // (Region) x0, y0, x1, y1 in the tile
    std::vector<RunDest> run_dest;          // (Runs) [run]
    grk_amd_pixel_layout tile_layout{};     // (Staged) the layout the tile decoder writes staged units in
    uint32_t unit_ch = 0;                   // ... whole pixels of this many channels, 0: planes
    bool upload_image = false;              // (Staged, host pixels) what the caller has in a layout's gaps goes up first
    std::vector<ImageGroup> groups;         // in the order in which they are decoded
    std::vector<uint32_t> places;           // the one array that is uploaded: x, y per staged unit, group after group
    uint64_t places_room = 0;               // ... and the bytes its device buffer is asked for
    uint64_t group_bytes = 0;               // the largest staged batch
    std::vector<FillRect> fills;            // (up) in launch order
};

// surf != nullptr: the destination is the caller's surface.
// An HT file does not announce refinement passes in its header: a decode plans, reads the packets, and -- table_has_second_segment --
// plans again with in.ht_refine.  The batches then carry their segment lists (want_segs), which keeps them off the int16 planes
// (group_checks_planes16: K5c refines int32 words), and a window of a one-tile image goes the Staged route: the region decoder
// empties the rows of the blocks outside the window, whose segment lists would no longer add up to them.
int plan_image_dest(const grk_amd_stream_info& info, const ViewPlan& plan, const ImageDestIn& in, const grk_amd_surface* surf, ImageDest& out,
                    const char** why);

// ---- the coded buffer ----------------------------------------------------------------------------------------------------------
// the codestream itself, or -- a view that leaves tiles out -- the touched tiles' tile-parts end to end: the tiles in index order,
// a tile's tile-parts in theirs
struct CodedCopy { uint64_t to, from, n; };
struct CodedSpan { uint64_t at; uint32_t len; uint64_t to; };      // a tile-part: where it lies in the file, its bytes, where in the buffer
struct CodedPlan {
    std::vector<uint64_t> part_to;          // [touched tile]: where its first tile-part starts in the buffer
    std::vector<uint32_t> span_at;          // [touched tiles + 1]: the tile's tile-parts in `spans`
    std::vector<CodedSpan> spans;
    uint64_t up_len = 0, coded_cap = 0;     // bytes uploaded; with the room of an appendix (never more than what is uploaded)
    uint64_t coded_bytes = 0;               // (rebase_table) bytes uploaded + the appendix the reader found
    std::vector<CodedCopy> copies;          // host to device, tile-parts that follow each other in the file as one
};
// all: every tile is touched (`parts` is not looked at)
void plan_coded(uint64_t len, uint32_t num_layers, bool all, const std::vector<uint32_t>& tiles, const std::vector<StreamPart>& parts, CodedPlan& out);

int check_moves(const grk_amd_tp_segment* moves, uint64_t n, uint64_t src_bytes, uint64_t dst_bytes, const char** why);
// The reader's offsets (positions in the codestream, the appendix behind it) onto the coded buffer, its moves checked, and
// unit_row ([units + 1]: a unit's rows in the reader's table) from the units' geometry, checked against the reader's row_at
int rebase_table(StreamTable& tab, uint64_t len, bool all, const std::vector<uint32_t>& tiles, const std::vector<StreamPart>& parts, CodedPlan& coded,
                 const ImageDest& dest, std::vector<uint64_t>& unit_row, const char** why);

// The packets of the tiles a whole-image decode touches (tiles == nullptr: all), as every such decode reads them: through the reader
// that every file goes through and -- only where that one met an HT block's second pass (StreamTable::met_ht_second_pass) -- again
// through the one that takes refinement passes; *refined: the table is the second reading's.  Every other refusal stands as it is
int read_decode_packets(const uint8_t* cs, uint64_t len, const grk_amd_stream_info& info, const std::vector<StreamPart>& parts, const std::vector<uint32_t>* tiles,
                        uint32_t drop_res, uint32_t threads, StreamTable& tab, std::string& err, bool* refined);
// a row of the reader's table has a second codeword segment (an HT block's: its refinement passes)
bool table_has_second_segment(const StreamTable& tab);
// behind the packets: a refined reading (read_decode_packets, or the device reader's) whose table has a second segment plans the
// destination again with in.ht_refine -- which tiles are touched does not change, a CodedPlan made before stands
int replan_for_refinement(const grk_amd_stream_info& info, const ViewPlan& plan, ImageDestIn& in, const grk_amd_surface* surf, const StreamTable& tab, bool refined,
                          ImageDest& d, const char** why);
// a staged batch of parameters p may have run on the int16 planes: with host pixels its status is read, and it is decoded again on
// int32 planes when a coefficient left them (include/grok_amd.h, grk_amd_set_decode_planes16)
bool group_checks_planes16(const ImageDest& d, const grk_amd_tile_params& p);

// the rows of `units` one unit after the other and -- want_segs -- their segment lists, rebased: first has rows + 1 entries
void group_tables(const StreamTable& tab, const std::vector<uint64_t>& unit_row, const uint32_t* units, size_t n, bool want_segs,
                  std::vector<grk_amd_coded_block>& rows, std::vector<uint32_t>& first, std::vector<grk_amd_segment>& segs);

} // namespace grk_amd
#pragma GCC visibility pop
