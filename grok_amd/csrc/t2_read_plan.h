// grok_amd/csrc/t2_read_plan.h -- the host planning of the device Tier-2 reader (HIP-free; private to the library, defined in
// t2_read_plan.cpp and tested on the CPU through tests/c/t2_parse_units.cpp).  From a stream's header: every tile's packets in
// file order with what KC (kernels_t2read.hip) needs to parse them, the chains -- runs of consecutive packets that one wave parses
// in order --, and the size of every scratch buffer.  read_device.hip carries the plan out.
#pragma once
#include "../../include/grok_amd.h"
#include "t2_parse.h"
#include "t2_parse_layers.h"
#include <vector>

#pragma GCC visibility push(hidden)
namespace grk_amd {

// what the kernels read about a tile (uploaded as it is)
struct T2ReadTile {
    uint32_t first_packet, npackets;    // its class's descriptors in T2ReadPlan::packets
    uint32_t row_base;                  // its first row in the image's table
    uint32_t rows;
    uint32_t chain_base, nchains;       // its chains among the call's: with PLT one per packet, else one
    uint32_t pkt_base;                  // its first entry in the PLT scratch (packet lengths and starts)
    uint32_t node_base, node_bytes;     // its share of the node scratch
    uint32_t cls;
};
// tiles of equal geometry and packet sequence share their descriptors
struct T2ReadClass { uint32_t first_packet, npackets, rows, node_bytes, max_chain_blocks; };

struct T2ReadPlan {
    bool ht = true, sop = false, eph = false, plt = false, tlm = false;
    uint32_t num_tiles = 0;
    std::vector<T2ReadPacket> packets;  // class after class, each in the tile's file order
    std::vector<T2ReadClass> classes;
    std::vector<T2ReadTile> tiles;
    uint64_t rows = 0;                  // of the image: info.num_blocks
    uint64_t chains = 0;                // KC's grid
    uint64_t total_packets = 0;         // PLT scratch: uint32 lengths and uint64 starts, one each per packet (with PLT)
    uint64_t node_bytes = 0;            // node scratch
    uint32_t geometry_builds = 0;       // tiles whose geometry was built (the others met their class by key)
    // scratch in bytes, as the executor allocates it
    uint64_t bytes_rows() const { return rows * sizeof(grk_amd_coded_block); }
    uint64_t bytes_plt() const { return plt ? total_packets * 12 : 0; }
    uint64_t bytes_tiles() const { return (uint64_t)tiles.size() * sizeof(T2ReadTile); }
    uint64_t bytes_packets() const { return (uint64_t)packets.size() * sizeof(T2ReadPacket); }
    uint64_t bytes_parts() const { return (uint64_t)num_tiles * 32; }      // per tile: where it lies, its length, its body, flags
};

// GRK_AMD_OK, or the refusal's code and in *why its reason: more than one layer, Part-1 with LAZY or TERMALL (several codeword
// segments), tables beyond the kernels' 32-bit fields -- GRK_AMD_ERR_UNSUPPORTED --, or a tile's geometry error
int plan_t2_read(const grk_amd_stream_info& info, T2ReadPlan& out, const char** why);

// ---- the general reader: several layers, several codeword segments (t2_parse_layers.h; KC-L, KF, KP) ---------------------------------
// what KC-L reads beside a packet descriptor (a precinct here: it has one packet per layer)
struct T2ReadLayerPk {
    uint32_t run_first, run_count;      // RLCP: the precincts of its resolution among the tile's, which follow each other
    uint32_t blocks_before;             // code-blocks of the tile's precincts before it: where its share of the logs starts
    uint32_t pad;
};
// one contribution's share of a codeword segment / one non-empty contribution (what the chains log and KP places)
struct T2ReadSegRecord { uint32_t row, ordinal, len, passes_opens; };           // passes | opens << 31
struct T2ReadPieceRecord { unsigned long long src; uint32_t row, ordinal, len, before; };

struct T2ReadLayersPlan {
    // As plan_t2_read gives it, but: a tile's npackets and pkt_base count the packets of ALL layers (KH's PLT scratch), its chains
    // are its precincts (with PLT: a chain reads the precinct's L packets) or the tile (without), node_base / node_bytes / node_at
    // count 32-bit nodes, and a class's npackets its precincts
    T2ReadPlan base;
    uint32_t layers = 1, order = 0, sty = 0;
    std::vector<T2ReadLayerPk> lpk;     // beside base.packets
    // The logs are sized by the worst case: per row what no stream can exceed (a record carries a pass, a row has 164 at most; see
    // t2_parse_layers.h), so a chain's share -- its rows' -- starts at (the tile's row_base + blocks_before) * records per row
    uint32_t seg_records_per_row = 1, piece_records_per_row = 1, segments_per_row = 1;
    uint64_t bytes_nodes() const { return base.node_bytes * 4; }
    uint64_t bytes_state() const { return base.rows * sizeof(T2pRowState); }
    uint64_t bytes_seg_log() const { return base.rows * seg_records_per_row * sizeof(T2ReadSegRecord); }
    uint64_t bytes_piece_log() const { return base.rows * piece_records_per_row * sizeof(T2ReadPieceRecord); }
    uint64_t bytes_counts() const { return base.chains * 8; }                                  // per chain: records in its two logs
    uint64_t bytes_segments() const { return base.rows * segments_per_row * sizeof(grk_amd_segment); }
    uint64_t bytes_moves() const { return base.rows * piece_records_per_row * sizeof(grk_amd_tp_segment); }
    uint64_t bytes_lpk() const { return (uint64_t)lpk.size() * sizeof(T2ReadLayerPk); }
};
// GRK_AMD_OK, or GRK_AMD_ERR_UNSUPPORTED for tables beyond the kernels' 32-bit fields, or a tile's geometry error.  Takes every
// layer count and code-block style the host reader takes.  ht_refine: an HT block's refinement passes are read (sty carries
// kT2pStyHtRefine): two segments, min(layers, 3) piece records and their sum less one segment records per row
int plan_t2_read_layers(const grk_amd_stream_info& info, T2ReadLayersPlan& out, const char** why, bool ht_refine = false);

// ---- locating the tile-parts from TLM (the host's share of KL) ------------------------------------------------------------------------
// The main header's bytes [0, n) (all of it, to the first SOT) of a stream of `len` bytes: TLM's entries in marker order as
// grk_amd_locate_tile_parts reads them.  *have: the header has TLM; at / ln / idx: the first min(count, num_tiles) tile-parts;
// *count: all of them.  GRK_AMD_OK or GRK_AMD_ERR_INVALID (a marker segment or an entry that does not fit).
int t2_read_tlm(const uint8_t* hdr, uint64_t n, uint64_t len, uint32_t num_tiles, bool* have, std::vector<uint64_t>& at, std::vector<uint32_t>& ln,
                std::vector<uint32_t>& idx, uint64_t* count);

} // namespace grk_amd
#pragma GCC visibility pop
