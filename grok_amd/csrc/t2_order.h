// grok_amd/csrc/t2_order.h -- the packet sequence of a tile (private to the library; defined in geometry.cpp).  The codestream
// writers emit the packets of a tile in this order, the codestream reader (t2_reader.cpp) meets them in it, and the whole-image
// encoders put only tiles that share it into one device-assembled batch (geometry.h: same_packets).
#pragma once
#include "geometry.h"
#include <cstdint>
#include <string>
#include <vector>

#pragma GCC visibility push(hidden)
namespace grk_amd {

// the packet of precinct `pi` (raster index in the resolution's precinct grid) of resolution r of component c; (x, y): the
// precinct's position on the reference grid, clipped to the tile
struct Pk { uint32_t c, r, pi; uint64_t x, y; };

// One layer's packets in progression order `order` (0 LRCP, 1 RLCP, 2 RPCL, 3 PCRL, 4 CPRL).  cg[c]: the geometry of component
// c's tile-component; comp_dx / comp_dy: its sub-sampling factors (NULL: 1); (gx0, gy0): the tile's origin on the reference grid.
std::vector<Pk> packet_order(const std::vector<const TileGeom*>& cg, const uint8_t* comp_dx, const uint8_t* comp_dy, uint32_t gx0, uint32_t gy0,
                             uint32_t order);

// The device writer's plan (geometry.h: T2Plan) of a tile whose components have geometries of their own -- a sub-sampled image: cg[c]
// and row0[c] (component c's first row in the tile's table) as write_tile_part takes them, the packets in packet_order's sequence.
// packet_of_block covers the tile's rows [0, max row0 + blocks).  GRK_AMD_ERR_UNSUPPORTED for GRK_AMD_CS_BLOCK_MSBS and for tables
// beyond the kernels' 32-bit fields, GRK_AMD_ERR_INVALID for rows that no packet or two packets hold.  t2_device_plan(g, ...) is this
// with every component at g.  (t2_writer.cpp)
int t2_device_plan_joint(const std::vector<const TileGeom*>& cg, const std::vector<uint64_t>& row0, const uint8_t* comp_dx, const uint8_t* comp_dy,
                         uint32_t gx0, uint32_t gy0, uint32_t flags, T2Plan& out);
// The same for the header kernel's general zero-bit-plane tree (the rows' own missing_msbs, each at most kT2MaxMsbs): the raw-bit
// scratch holds kT2MaxMsbs more bits per block, and every packet gets a place (T2Packet::v_at, T2Plan::v_bytes) for its bands' node
// values.  GRK_AMD_CS_BLOCK_MSBS in `flags` is accepted and implied.
int t2_device_plan_joint_msbs(const std::vector<const TileGeom*>& cg, const std::vector<uint64_t>& row0, const uint8_t* comp_dx,
                              const uint8_t* comp_dy, uint32_t gx0, uint32_t gy0, uint32_t flags, T2Plan& out);

// The tiles of an image of `nruns` units per tile (image.h: unit t * nruns + k is run k of tile t, of[] its geometry group) in CLASSES
// that one joint plan frames: the same group for every run, and the same packet sequence under `order` -- seq[t] is tile t's
// packet_order, compared as same_packets compares (component, resolution, precinct); orders 0 and 1 follow from the groups alone and
// `seq` may be empty.  class_of[t]; returns the number of classes, numbered by their first tile.  (geometry.cpp)
uint32_t joint_tile_classes(const std::vector<uint32_t>& of, uint32_t nruns, uint32_t order, const std::vector<std::vector<Pk>>& seq,
                            std::vector<uint32_t>& class_of);

// ---- tiles divided into tile-parts (GRK_AMD_CS_TP; geometry.cpp) ---------------------------------------------------------------------
// The tile-parts of a tile under the order and division of `flags`: their number (1 without a division) -- fixed by the letters'
// extents, whether or not a part has packets -- or GRK_AMD_ERR_UNSUPPORTED with *why: a P at or before the division letter, more than
// 255 parts.
int tile_part_count(uint32_t flags, uint32_t num_levels, uint32_t num_comps, std::string* why = nullptr);
// ... and the first packet of every part in `seq`, the tile's packet_order under the same flags (non-decreasing; equal neighbours: a
// part without packets).  Returns the number of parts.
int tile_part_starts(const std::vector<Pk>& seq, uint32_t flags, uint32_t num_levels, uint32_t num_comps, std::vector<uint32_t>& starts,
                     std::string* why = nullptr);
// the reason of a host writer call's refusal, for grk_amd_writer_last_error (per thread); returns `code`
int writer_refuse(int code, const std::string& why);

} // namespace grk_amd
#pragma GCC visibility pop
