// grok_amd/csrc/t2_order.h -- the packet sequence of a tile (private to the library; defined in geometry.cpp).  The codestream
// writers emit the packets of a tile in this order, the codestream reader (t2_reader.cpp) meets them in it, and the whole-image
// encoders put only tiles that share it into one device-assembled batch (geometry.h: same_packets).
#pragma once
#include "geometry.h"
#include <cstdint>
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

} // namespace grk_amd
#pragma GCC visibility pop
