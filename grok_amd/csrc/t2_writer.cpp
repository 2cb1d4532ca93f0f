// grok_amd/csrc/t2_writer.cpp -- host-side Tier-2 + codestream assembly.
//
// The Grok plugin protocol hands ONE grk_plugin_tile to every tile of an image (defect D3), so
// multi-tile images -- the tile-sharded multi-GPU configuration -- cannot go through
// grk_compress_with_plugin.  This writer produces the same bytes the reference would:
//   main header : CodeStreamCompress.cpp:722-753 (SOC, SIZ markers/SIZMarker.cpp, CAP :936-981,
//                 COD :1060-1105, QCD Quantizer.cpp:87-121, COM :296-309)
//   tile part   : SOT markers/SOTMarker.cpp:41-72, SOD, then one packet per (resolution, component)
//                 in LRCP order (t2/PacketIter.cpp:805-829) -- 1 layer, 1 precinct per resolution,
//                 no SOP/EPH, every code-block included with its single HT cleanup pass
//   packet      : T2Compress::compressPacket t2/T2Compress.cpp:123-333; tag trees t1/TagTree.cpp:170-218;
//                 bit stuffing t1/BitIO.cpp:46-175
// It is O(#code-blocks) host work plus one memcpy of the coded bytes.
#include "../../include/grok_amd.h"
#include "geometry.h"
#include "image.h"
#include "t2_order.h"
#include "t2_parts.h"
#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>

namespace {

using namespace grk_amd;

// p == nullptr: only counts (ovf stays false).  PLAN mode (lit != nullptr): nothing is copied -- what the writer writes itself (marker
// segments, packet headers) collects in `lit`, and the output is described as a list of segments, each either a run of those
// literal bytes or a code-block's bytes in the coded buffer (grk_amd_plan_tile_part: the caller places them, on whatever
// threads or device it likes, once it knows where the tile-part goes).
struct Out {
    uint8_t* p; uint64_t cap; uint64_t n = 0; bool ovf = false;
    std::vector<uint8_t>* lit = nullptr; std::vector<grk_amd_tp_segment>* segs = nullptr;
    void u8(uint32_t v)
    {
        if (lit) {
            if (segs->empty() || segs->back().kind != 0 || segs->back().dst + segs->back().len != n)
                segs->push_back(grk_amd_tp_segment{n, (uint64_t)lit->size(), 0u, 0u});
            lit->push_back((uint8_t)v); segs->back().len++;
        } else if (p) { if (n < cap) p[n] = (uint8_t)v; else ovf = true; }
        ++n;
    }
    void u16(uint32_t v) { u8(v >> 8); u8(v & 0xFF); }
    void u32(uint32_t v) { u16(v >> 16); u16(v & 0xFFFF); }
    void bytes(const uint8_t* s, uint64_t len)               // bytes of the writer's own
    {
        if (lit) { for (uint64_t i = 0; i < len; ++i) u8(s[i]); return; }
        if (p) { if (n + len <= cap) std::memcpy(p + n, s, len); else ovf = true; }
        n += len;
    }
    void body(const uint8_t* coded, uint64_t off, uint64_t len)   // a code-block's bytes
    {
        if (lit) { if (len) segs->push_back(grk_amd_tp_segment{n, off, (uint32_t)len, 1u}); n += len; return; }
        if (p) { if (n + len <= cap) std::memcpy(p + n, coded + off, len); else ovf = true; }
        n += len;
    }
    // (a patch lies in the SOT marker segment or the TLM: literal bytes written in one run -- `lit_at` = where that run began in lit,
    //  `run_dst` = its first byte's place in the output)
    void patch32(uint64_t at, uint32_t v, uint64_t lit_at = 0, uint64_t run_dst = 0)
    {
        uint8_t* q = nullptr;
        if (lit) { const uint64_t i = lit_at + (at - run_dst); if (i + 4 <= lit->size()) q = lit->data() + i; }
        else if (p && at + 4 <= cap) q = p + at;
        if (q) { q[0] = (uint8_t)(v >> 24); q[1] = (uint8_t)(v >> 16); q[2] = (uint8_t)(v >> 8); q[3] = (uint8_t)v; }
    }
};

// MSB-first packet-header bit writer: a byte following 0xFF carries 7 bits (BitIO.cpp:46-175).  Bits collect in a 64-bit
// register and leave a byte at a time; BitIO's own form (one call per bit, the byte written when the NEXT bit arrives) gives the same
// bytes: a full byte is the same byte whenever it is written, and its flush -- the byte in work as it is, then an empty byte if that
// one was 0xFF -- is flush() below.
struct HeaderBits {
    Out& o; uint64_t acc = 0; int n = 0; uint32_t last = 0;
    explicit HeaderBits(Out& out) : o(out) {}
    void drain()
    {
        for (;;) {
            const int take = last == 0xFF ? 7 : 8;
            if (n < take) break;
            last = (uint32_t)(acc >> (n - take)) & ((1u << take) - 1u);
            o.u8(last);
            n -= take;
        }
    }
    void put(uint32_t v, int k) { acc = (acc << k) | v; n += k; drain(); }      // k <= 32 bits of v, MSB first
    void bit(uint32_t b) { put(b & 1u, 1); }
    void ones(int k) { put((uint32_t)((1ull << k) - 1ull), k); }                  // k <= 32
    void zeros(int k) { while (k > 0) { const int t = k > 32 ? 32 : k; put(0, t); k -= t; } }
    void comma(int k) { while (k > 31) { ones(31); k -= 31; } put(((1u << k) - 1u) << 1, k + 1); }   // k ones, then a zero
    void flush()
    {
        if (n) { const int take = last == 0xFF ? 7 : 8; last = (uint32_t)(acc & ((1ull << n) - 1ull)) << (take - n); o.u8(last); n = 0; }
        else if (last == 0xFF) { o.u8(0); last = 0; }
    }
};

// Tag trees (ISO 15444-1 B.10.2; t1/TagTree.cpp:170-218) as this writer meets them.  A packet of the single layer includes every
// code-block, and every block of a band has the same number of missing bit-planes (numbps = 1 is signalled for an HT block,
// T1HT.cpp:123: Kmax - 1 of them): BOTH trees of a band's precinct -- inclusion, all leaves 0 against threshold 1; zero bit-planes,
// all leaves v -- are uniform.  Coding leaf (x, y) then emits, from the root down, one '1' for every node on its path that no
// earlier leaf (raster order) has passed -- the nodes (x >> l, y >> l) with the low l bits of x and y zero: 1 + min(ctz x, ctz y)
// of them, at most the tree's height -- and, for the zero-bit-plane tree's root alone, v '0's in front of its '1'.  (The general
// procedure -- per node a lower bound raised bit by bit to the threshold -- reduces to exactly this when no node's value is
// below its parent's.)
inline int tag_tree_height(uint32_t gw, uint32_t gh)
{
    int h = 1;
    while ((uint64_t)gw * gh > 1) { gw = (gw + 1) >> 1; gh = (gh + 1) >> 1; ++h; }
    return h;
}
inline int new_nodes(uint32_t x, uint32_t y, int height)
{
    const uint32_t m = x | y;
    const int z = m ? __builtin_ctz(m) : 31;
    return z + 1 < height ? z + 1 : height;
}

int floor_log2(uint32_t v) { int r = 0; while (v >>= 1) ++r; return r; }

// The zero-bit-plane tag tree in its general form (GRK_AMD_CS_BLOCK_MSBS: the rows' own missing_msbs, which differ block by block
// once an encode drops bit-planes): level 0 holds the leaves (gw x gh, raster), every level above the minimum of its up to four
// children, up to one root.  A leaf is coded when its block is first included -- in this writer's single layer all of them, in
// raster order -- against a threshold above its value: from the root down every node's lower bound is raised from what its parent
// left to its value with one '0' per step, then a '1' the first time the value is reached (B.10.2; t1/TagTree.cpp:170-218).  With
// every leaf at v this emits v '0's at the root and one '1' per new node: the constant form above, bit for bit.
struct ZbpTree {
    struct Level { uint32_t w, h; size_t at; };
    std::vector<Level> lv;
    std::vector<uint32_t> value, low;
    std::vector<uint8_t> known;
    ZbpTree(const grk_amd_coded_block* cb, uint32_t gw, uint32_t gh)
    {
        size_t n = 0;
        for (uint32_t w = gw, h = gh;; w = (w + 1) >> 1, h = (h + 1) >> 1) {
            lv.push_back(Level{w, h, n});
            n += (size_t)w * h;
            if ((uint64_t)w * h <= 1) break;
        }
        value.assign(n, 0xFFFFFFFFu); low.assign(n, 0); known.assign(n, 0);
        for (size_t i = 0; i < (size_t)gw * gh; ++i) value[i] = cb[i].missing_msbs;
        for (size_t l = 0; l + 1 < lv.size(); ++l)
            for (uint32_t y = 0; y < lv[l].h; ++y)
                for (uint32_t x = 0; x < lv[l].w; ++x) {
                    uint32_t& up = value[lv[l + 1].at + (size_t)(y >> 1) * lv[l + 1].w + (x >> 1)];
                    up = std::min(up, value[lv[l].at + (size_t)y * lv[l].w + x]);
                }
    }
    template <class Bits> void code(Bits& hb, uint32_t x, uint32_t y)
    {
        const uint32_t threshold = value[(size_t)y * lv[0].w + x] + 1u;
        uint32_t lo = 0;
        for (size_t l = lv.size(); l-- > 0;) {
            const size_t i = lv[l].at + (size_t)(y >> l) * lv[l].w + (x >> l);
            lo = std::max(lo, low[i]);
            while (lo < threshold) {
                if (lo >= value[i]) { if (!known[i]) { hb.bit(1); known[i] = 1; } break; }
                hb.bit(0); ++lo;
            }
            low[i] = lo;
        }
    }
};

// tlm_at: where the Ptlm fields of the TLM marker segment start (0: none written)
// parts_per_tile (a file of tiles divided into tile-parts; NULL: one each): TLM lists every tile-part in file order -- a tile's parts
// together, the tiles in order -- and is the header's LAST marker segment, where the model of such files (tests/tileparts.py) puts it
void write_main_header(Out& o, const TileGeom& g, const grk_amd_image_layout& im, uint32_t flags, uint32_t ntiles, uint64_t* tlm_at,
                       const uint8_t* comp_dx = nullptr, const uint8_t* comp_dy = nullptr, const uint32_t* parts_per_tile = nullptr)
{
    if (tlm_at) *tlm_at = 0;
    const grk_amd_tile_params& p = g.p;
    o.u16(0xFF4F);                                                     // SOC
    o.u16(0xFF51); o.u16(38 + 3 * p.num_comps); o.u16(0x4000);         // SIZ, Rsiz: HTJ2K (Part 15)
    o.u32(im.x1); o.u32(im.y1); o.u32(im.x0); o.u32(im.y0);            // Xsiz Ysiz XOsiz YOsiz (markers/SIZMarker.cpp)
    o.u32(im.t_width); o.u32(im.t_height); o.u32(im.tx0); o.u32(im.ty0);
    o.u16(p.num_comps);
    for (uint32_t c = 0; c < p.num_comps; ++c) {                       // Ssiz, XRsiz, YRsiz
        o.u8((p.prec - 1) | (p.sgnd ? 0x80 : 0)); o.u8(comp_dx && comp_dx[c] ? comp_dx[c] : 1); o.u8(comp_dy && comp_dy[c] ? comp_dy[c] : 1);
    }
    // CAP (CodeStreamCompress.cpp:936-981; MAGBp HTParams.cpp:313-329)
    uint32_t B = 0;
    const uint32_t nb = 3 * p.num_levels + 1;
    for (uint32_t i = 0; i < nb; ++i) {
        if (!p.irreversible) B = std::max<uint32_t>(B, (uint32_t)(g.qcd_words[i] >> 3) + 1 - 1);
        else {
            uint32_t lev = p.num_levels - (i ? (i - 1) / 3 : 0);
            B = std::max<uint32_t>(B, (uint32_t)(g.qcd_words[i] >> 11) + 1 - lev);
        }
    }
    uint32_t Bp = B <= 8 ? 0 : (B < 28 ? B - 8 : (B < 48 ? 13 + (B >> 2) : 31));
    o.u16(0xFF50); o.u16(8); o.u32(0x00020000); o.u16((p.irreversible ? 0x0020 : 0) | Bp);
    // COD: Scod = SOP (2) | EPH (4), SGcod = progression order, one layer, MCT
    bool prt = false;                       // user-defined precincts: Scod bit 0 and one size byte per resolution
    for (uint32_t r = 0; r <= p.num_levels; ++r) prt = prt || p.precinct_exp[r] != 0;
    o.u16(0xFF52); o.u16(12 + (prt ? p.num_levels + 1u : 0u));
    o.u8((prt ? 1u : 0u) | ((flags & GRK_AMD_CS_SOP) ? 2u : 0u) | ((flags & GRK_AMD_CS_EPH) ? 4u : 0u));
    o.u8((flags >> GRK_AMD_CS_PROG_SHIFT) & 7u); o.u16(1); o.u8(p.mct ? 1 : 0);
    o.u8(p.num_levels); o.u8(p.cblk_w_exp - 2); o.u8(p.cblk_h_exp - 2); o.u8(0x40); o.u8(p.irreversible ? 0 : 1);
    for (uint32_t r = 0; prt && r <= p.num_levels; ++r) o.u8(p.precinct_exp[r] ? p.precinct_exp[r] : 0xFFu);
    // QCD: one guard bit
    if (!p.irreversible) {
        o.u16(0xFF5C); o.u16(3 + nb); o.u8(0x20);
        for (uint32_t i = 0; i < nb; ++i) o.u8(g.qcd_words[i] & 0xFF);
    } else {
        o.u16(0xFF5C); o.u16(3 + 2 * nb); o.u8(0x22);
        for (uint32_t i = 0; i < nb; ++i) o.u16(g.qcd_words[i]);
    }
    // TLM (markers/LengthMarkers.cpp:166-189, written between QCD and COM: CodeStreamCompress.cpp:734): Ztlm 0, Stlm 0x50 =
    // one-byte tile index + four-byte tile-part length per tile-part; the lengths are patched in once they are known
    if ((flags & GRK_AMD_CS_TLM) && !parts_per_tile) {
        o.u16(0xFF55); o.u16(4 + 5 * ntiles); o.u8(0); o.u8(0x50);
        if (tlm_at) *tlm_at = o.n;
        for (uint32_t t = 0; t < ntiles; ++t) { o.u8(t); o.u32(0); }
    }
    // COM (the reference's default comment, so that whole files compare byte for byte)
    static const char kCom[] = "Created by Grok     version 8.0.2";
    const uint32_t cl = (uint32_t)std::strlen(kCom);
    o.u16(0xFF64); o.u16(4 + cl); o.u16(1);
    o.bytes(reinterpret_cast<const uint8_t*>(kCom), cl);
    if ((flags & GRK_AMD_CS_TLM) && parts_per_tile) {
        uint32_t entries = 0;
        for (uint32_t t = 0; t < ntiles; ++t) entries += parts_per_tile[t];
        o.u16(0xFF55); o.u16(4 + 5 * entries); o.u8(0); o.u8(0x50);
        if (tlm_at) *tlm_at = o.n;
        for (uint32_t t = 0; t < ntiles; ++t)
            for (uint32_t k = 0; k < parts_per_tile[t]; ++k) { o.u8(t); o.u32(0); }
    }
}

// sop: the packet's number in the tile (SOP marker segment in front, T2Compress.cpp:149-164) or < 0; eph: EPH after the header
// the packet of precinct `pi` of resolution r
void write_packet(Out& o, const TileGeom& g, uint32_t r, uint32_t pi, const grk_amd_coded_block* comp_table, const uint8_t* coded,
                  int32_t sop = -1, bool eph = false, bool block_msbs = false)
{
    const ResGeom& R = g.res[r];
    if (sop >= 0) { o.u16(0xFF91); o.u16(4); o.u16((uint32_t)sop & 0xFFFFu); }
    HeaderBits hb(o);
    hb.bit(1);
    for (uint32_t bi = 0; bi < R.num_bands; ++bi) {
        const BandGeom& B = R.band[bi];
        const BandGeom::Prec& P = B.prec[pi];
        if (!P.gw || !P.gh) continue;
        const int height = tag_tree_height(P.gw, P.gh);
        const grk_amd_coded_block* cb = comp_table + P.first_block;
        const std::unique_ptr<ZbpTree> zbp(block_msbs ? new ZbpTree(cb, P.gw, P.gh) : nullptr);
        for (uint32_t y = 0; y < P.gh; ++y)
            for (uint32_t x = 0; x < P.gw; ++x, ++cb) {
                const int nn = new_nodes(x, y, height);
                hb.ones(nn);                                          // inclusion: the path's new nodes
                if (zbp) zbp->code(hb, x, y);                         // zero bit-planes: the rows' own, the general tree
                else {
                    if (!(x | y)) hb.zeros((int)B.kmax - 1);          // zero bit-planes: the root's value ...
                    hb.ones(nn);                                      // ... and the path's new nodes
                }
                const uint32_t len = cb->length;
                int inc = floor_log2(len) + 1 - 3;
                if (inc < 0) inc = 0;
                hb.put(0, 1);                                         // one coding pass
                hb.comma(inc);                                        // Lblock raised from 3 to what the length needs
                hb.put(len, 3 + inc);
            }
    }
    hb.flush();
    if (eph) o.u16(0xFF92);
    for (uint32_t bi = 0; bi < R.num_bands; ++bi) {
        const BandGeom::Prec& P = R.band[bi].prec[pi];
        for (uint32_t k = 0; k < P.gw * P.gh; ++k) {
            const grk_amd_coded_block& cb = comp_table[P.first_block + k];
            o.body(coded, cb.offset, cb.length);
        }
    }
}

// The tiles of an image (ISO 15444-1 B.3; the reference: TileProcessor::init, tile/TileProcessor.cpp:100-170): tile
// (tx, ty) of the grid anchored at (tx0, ty0) is its cell clipped to the image area.
struct Layout { grk_amd_image_layout im; uint32_t tcols, trows; };
int check_layout(const grk_amd_image_layout* im, Layout& l)
{
    if (!im || im->x1 <= im->x0 || im->y1 <= im->y0 || !im->t_width || !im->t_height) return GRK_AMD_ERR_INVALID;
    if (im->tx0 > im->x0 || im->ty0 > im->y0) return GRK_AMD_ERR_INVALID;                              // B.3: XTOsiz <= XOsiz
    if ((uint64_t)im->tx0 + im->t_width <= im->x0 || (uint64_t)im->ty0 + im->t_height <= im->y0) return GRK_AMD_ERR_INVALID;
    l.im = *im;
    l.tcols = (uint32_t)(((uint64_t)im->x1 - im->tx0 + im->t_width - 1) / im->t_width);
    l.trows = (uint32_t)(((uint64_t)im->y1 - im->ty0 + im->t_height - 1) / im->t_height);
    if ((uint64_t)l.tcols * l.trows > 65535) return GRK_AMD_ERR_UNSUPPORTED;
    return GRK_AMD_OK;
}
void tile_of(const Layout& l, const grk_amd_tile_params& base, uint32_t t, grk_amd_tile_params& p)
{
    const uint32_t tx = t % l.tcols, ty = t / l.tcols;
    const uint64_t cx0 = (uint64_t)l.im.tx0 + (uint64_t)tx * l.im.t_width, cy0 = (uint64_t)l.im.ty0 + (uint64_t)ty * l.im.t_height;
    const uint64_t x0 = std::max<uint64_t>(cx0, l.im.x0), y0 = std::max<uint64_t>(cy0, l.im.y0);
    const uint64_t x1 = std::min<uint64_t>(cx0 + l.im.t_width, l.im.x1), y1 = std::min<uint64_t>(cy0 + l.im.t_height, l.im.y1);
    p = base;
    p.tile_x0 = (uint32_t)x0; p.tile_y0 = (uint32_t)y0;
    p.tile_w = (uint32_t)(x1 - x0); p.tile_h = (uint32_t)(y1 - y0);
}
grk_amd_image_layout plain_layout(const grk_amd_tile_params& p, uint32_t img_w, uint32_t img_h)
{
    return grk_amd_image_layout{p.tile_x0, p.tile_y0, p.tile_x0 + img_w, p.tile_y0 + img_h, p.tile_x0, p.tile_y0, p.tile_w, p.tile_h};
}

// SOT, (PLT,) SOD and the packets of one tile in the progression order of `flags`; returns the tile-part's length.
// One layer.  `cg[c]` is the geometry of component c's tile-component (all the same object for an image without sub-sampling),
// `row0[c]` the first of its rows in the tile's table.  The five orders (ISO 15444-1 B.12.1; t2/PacketIter.cpp:805-1100) are
//   LRCP, RLCP  resolution -> component -> precinct (raster)
//   RPCL        resolution -> precinct position -> component
//   PCRL        precinct position -> component -> resolution
//   CPRL        component -> precinct position -> resolution
// where a precinct's position is its top-left corner on the REFERENCE grid (component coordinates times the component's
// sub-sampling factors), clipped to the tile -- the (y, x) at which the standard's position loops meet it; positions are walked
// in raster order, several resolutions / components can share one.  (The sequence is packet_order's: t2_order.h, defined in
// geometry.cpp, where the grouping of tiles compares it too -- the codestream reader walks the same sequence, once per layer.)

// a packet's length as the PLT marker segment carries it: a big-endian base-128 number (continuation bit 0x80)
void plt_length(std::vector<uint8_t>& body, uint64_t v)
{
    uint8_t tmp[10]; int k = 0;
    tmp[k++] = (uint8_t)(v & 0x7F);
    while (v >>= 7) tmp[k++] = (uint8_t)((v & 0x7F) | 0x80);
    while (k) body.push_back(tmp[--k]);
}

// PLT (markers/LengthMarkers.cpp:313-374, written in front of SOD: TileProcessor.cpp:719-726): Zplt 0, then every packet's length.
// Marker segments of at most 65535 bytes (Lplt is 16 bits: Lplt, Zplt and 65532 bytes of lengths), Zplt = 0, 1, ...;
// a packet's length (1-5 bytes, the last one without the continuation bit) is never split over two segments.
// 18 packets of a 6-resolution RGB tile need < 100 bytes; small precincts multiply that: the reference starts another
// segment near 64 KiB as well (LengthMarkers.cpp:313-331 -- its continuation segments lack the Zplt byte, a defect
// this writer does not copy: T.800 A.7.3).
void write_plt(Out& o, const std::vector<uint8_t>& body)
{
    size_t at = 0;
    uint32_t z = 0;
    do {
        size_t end = at, next = at;
        while (next < body.size()) {
            size_t e = next;
            while (body[e] & 0x80) ++e;                        // one length: bytes with the continuation bit, then one without
            ++e;
            if (e - at > 65532) break;
            end = next = e;
        }
        if (z > 255) { o.ovf = true; break; }                  // (Zplt is one byte: > 16 MB of packet lengths in one tile-part does not fit the syntax)
        o.u16(0xFF58); o.u16((uint32_t)(3 + (end - at))); o.u8((uint8_t)z++);
        o.bytes(body.data() + at, end - at);
        at = end;
    } while (at < body.size());
}

// A tile divided into tile-parts (GRK_AMD_CS_TP): the first packet of every part -- the caller's (`starts`, `nparts`), or with
// starts == NULL the division of `flags` (t2_order.h: tile_part_starts).  The writer leaves the parts' lengths in part_bytes and, for
// starts it cannot take, the error in `error`.
struct Division { const uint32_t* starts; uint32_t nparts; std::vector<uint32_t> part_bytes; int error = GRK_AMD_OK; };

uint64_t write_tile_part(Out& o, const std::vector<const TileGeom*>& cg, const std::vector<uint64_t>& row0, const uint8_t* comp_dx,
                         const uint8_t* comp_dy, uint32_t gx0, uint32_t gy0, uint32_t t, uint32_t flags, const grk_amd_coded_block* tt,
                         const uint8_t* coded, Division* dv = nullptr)
{
    const uint64_t sot = o.n, sot_lit = o.lit ? o.lit->size() : 0;
    const uint32_t order = (flags >> GRK_AMD_CS_PROG_SHIFT) & 7u;
    const bool sop = (flags & GRK_AMD_CS_SOP) != 0, eph = (flags & GRK_AMD_CS_EPH) != 0, msbs = (flags & GRK_AMD_CS_BLOCK_MSBS) != 0;
    const std::vector<Pk> seq = packet_order(cg, comp_dx, comp_dy, gx0, gy0, order);
    // packets [first, last) of the tile (Nsop: the packet's number in the TILE)
    auto packets = [&](Out& dst, std::vector<uint8_t>* plt, size_t first = 0, size_t last = ~(size_t)0) {
        last = std::min(last, seq.size());
        for (size_t n = first; n < last; ++n) {
            const Pk& q = seq[n];
            const uint64_t at = dst.n;
            write_packet(dst, *cg[q.c], q.r, q.pi, tt + row0[q.c], coded, sop ? (int32_t)n : -1, eph, msbs);
            if (plt) plt_length(*plt, dst.n - at);
        }
    };
    if (dv) {
        // the parts one behind the other: SOT (TPsot, TNsot), the PLT of the part's own packets (none in a part without), SOD, the packets
        std::vector<uint32_t> from_flags;
        const uint32_t* starts = dv->starts;
        uint32_t nparts = dv->nparts;
        if (!starts) {
            const int n = tile_part_starts(seq, flags, cg[0]->p.num_levels, (uint32_t)cg.size(), from_flags);
            if (n < 0) { dv->error = n; return 0; }
            starts = from_flags.data(); nparts = (uint32_t)n;
        }
        bool ok = nparts >= 1 && nparts <= kMaxTileParts && starts[0] == 0;
        for (uint32_t k = 0; ok && k < nparts; ++k) ok = starts[k] <= seq.size() && (!k || starts[k - 1] <= starts[k]);
        if (!ok) { dv->error = GRK_AMD_ERR_INVALID; return 0; }
        dv->part_bytes.assign(nparts, 0);
        for (uint32_t k = 0; k < nparts; ++k) {
            const size_t first = starts[k], last = k + 1 < nparts ? starts[k + 1] : seq.size();
            const uint64_t at = o.n, at_lit = o.lit ? o.lit->size() : 0;
            o.u16(0xFF90); o.u16(10); o.u16(t); o.u32(0); o.u8(k); o.u8(nparts);
            if ((flags & GRK_AMD_CS_PLT) && last > first) {
                std::vector<uint8_t> body;
                Out cnt{nullptr, 0};
                packets(cnt, &body, first, last);
                write_plt(o, body);
            }
            o.u16(0xFF93);
            packets(o, nullptr, first, last);
            if ((o.n - at) >> 32) o.ovf = true;                 // (Psot is 32 bits)
            o.patch32(at + 6, (uint32_t)(o.n - at), at_lit, at);
            dv->part_bytes[k] = (uint32_t)(o.n - at);
        }
        return o.n - sot;
    }
    o.u16(0xFF90); o.u16(10); o.u16(t); o.u32(0); o.u8(0); o.u8(1);
    if (flags & GRK_AMD_CS_PLT) {
        // the packets are sized with a counting pass
        std::vector<uint8_t> body;
        Out cnt{nullptr, 0};
        packets(cnt, &body);
        write_plt(o, body);
    }
    o.u16(0xFF93);
    packets(o, nullptr);
    o.patch32(sot + 6, (uint32_t)(o.n - sot), sot_lit, sot);
    return o.n - sot;
}

// an image without sub-sampling: every component has the tile's own geometry, comp c's rows start at c * blocks_per_comp
uint64_t write_tile_part(Out& o, const TileGeom& g, uint32_t t, uint32_t flags, const grk_amd_coded_block* tt, const uint8_t* coded,
                         Division* dv = nullptr)
{
    std::vector<const TileGeom*> cg(g.p.num_comps, &g);
    std::vector<uint64_t> row0(g.p.num_comps);
    for (uint32_t c = 0; c < g.p.num_comps; ++c) row0[c] = (uint64_t)c * g.blocks_per_comp;
    return write_tile_part(o, cg, row0, nullptr, nullptr, g.p.tile_x0, g.p.tile_y0, t, flags, tt, coded, dv);
}

// What a file's writer makes of GRK_AMD_CS_TP before any byte: the parts per tile (1: the undivided file, byte for byte), or the
// refusal -- the rule's, or more tile-parts than one TLM marker segment lists
int file_division(uint32_t flags, const grk_amd_tile_params& base, uint32_t ntiles)
{
    std::string why;
    const int n = tile_part_count(flags, base.num_levels, base.num_comps, &why);
    if (n < 0) return writer_refuse(n, why);
    if (n > 1 && (flags & GRK_AMD_CS_TLM) && (uint64_t)n * ntiles > kMaxTlmEntries)
        return writer_refuse(GRK_AMD_ERR_UNSUPPORTED, std::to_string((uint64_t)n * ntiles) + " tile-parts: one TLM marker segment lists at most 13 106");
    return n;
}

} // namespace

extern "C" int64_t grk_amd_layout_num_tiles(const grk_amd_image_layout* im)
{
    Layout l;
    const int rc = check_layout(im, l);
    return rc != GRK_AMD_OK ? rc : (int64_t)l.tcols * l.trows;
}

extern "C" int grk_amd_layout_tile(const grk_amd_image_layout* im, const grk_amd_tile_params* base, uint32_t tile_index,
                                   grk_amd_tile_params* out)
{
    Layout l;
    const int rc = check_layout(im, l);
    if (rc != GRK_AMD_OK) return rc;
    if (!base || !out || tile_index >= l.tcols * l.trows) return GRK_AMD_ERR_INVALID;
    tile_of(l, *base, tile_index, *out);
    return GRK_AMD_OK;
}

extern "C" int64_t grk_amd_write_codestream_layout(const grk_amd_image_layout* im, const grk_amd_tile_params* base,
                                                   const grk_amd_coded_block* table, const uint8_t* coded, uint32_t flags,
                                                   uint8_t* out, uint64_t cap)
{
    if (!base || !table || !coded || !out) return GRK_AMD_ERR_INVALID;
    Layout l;
    int rc = check_layout(im, l);
    if (rc != GRK_AMD_OK) return rc;
    const uint32_t ntiles = l.tcols * l.trows;
    if ((flags & GRK_AMD_CS_TLM) && ntiles > 255) return GRK_AMD_ERR_UNSUPPORTED;     // (one-byte Ttlm, as the reference writes it)
    const int nparts = file_division(flags, *base, ntiles);
    if (nparts < 0) return nparts;
    const std::vector<uint32_t> per_tile(nparts > 1 ? ntiles : 0, (uint32_t)nparts);
    Division dv{nullptr, 0};
    TileGeom g;
    grk_amd_tile_params p;
    Out o{out, cap};
    uint64_t tlm_at = 0, row = 0;
    for (uint32_t t = 0; t < ntiles; ++t) {
        tile_of(l, *base, t, p);
        rc = build_tile_geom(p, g);
        if (rc != GRK_AMD_OK) return rc;
        if (t == 0) write_main_header(o, g, l.im, flags, ntiles, &tlm_at, nullptr, nullptr, nparts > 1 ? per_tile.data() : nullptr);
        const uint64_t len = write_tile_part(o, g, t, flags, table + row, coded, nparts > 1 ? &dv : nullptr);
        if (dv.error) return dv.error;
        row += (uint64_t)g.blocks_per_comp * p.num_comps;
        if (tlm_at && nparts > 1) { for (int k = 0; k < nparts; ++k) o.patch32(tlm_at + 5ull * ((uint64_t)t * nparts + k) + 1, dv.part_bytes[k]); }
        else if (tlm_at) o.patch32(tlm_at + 5ull * t + 1, (uint32_t)len);
    }
    o.u16(0xFFD9);
    if (o.ovf) return GRK_AMD_ERR_OVERFLOW;
    return (int64_t)o.n;
}

// ---- sub-sampled components ------------------------------------------------------------------------------------------
// Component c of a tile [x0, x1) x [y0, y1) of the reference grid is [ceil(x0 / dx_c), ceil(x1 / dx_c)) x [ceil(y0 / dy_c),
// ceil(y1 / dy_c)) in its own coordinates (tile/TileProcessor.cpp:605-612); everything below the tile-component -- resolutions,
// bands, precincts, code-blocks -- is derived from that rectangle as for any tile (tile/TileComponent.cpp:69-170).
namespace {
int tile_comp_of(const Layout& l, const grk_amd_tile_params& base, uint32_t dx, uint32_t dy, uint32_t t, grk_amd_tile_params& p)
{
    tile_of(l, base, t, p);
    dx = dx ? dx : 1; dy = dy ? dy : 1;
    const uint64_t x0 = p.tile_x0, y0 = p.tile_y0, x1 = x0 + p.tile_w, y1 = y0 + p.tile_h;
    const uint64_t cx0 = (x0 + dx - 1) / dx, cy0 = (y0 + dy - 1) / dy, cx1 = (x1 + dx - 1) / dx, cy1 = (y1 + dy - 1) / dy;
    if (cx1 <= cx0 || cy1 <= cy0) return GRK_AMD_ERR_UNSUPPORTED;      // (a tile without a sample of this component)
    p.tile_x0 = (uint32_t)cx0; p.tile_y0 = (uint32_t)cy0; p.tile_w = (uint32_t)(cx1 - cx0); p.tile_h = (uint32_t)(cy1 - cy0);
    return GRK_AMD_OK;
}
} // namespace

extern "C" int grk_amd_layout_tile_comp(const grk_amd_image_layout* im, const grk_amd_tile_params* base, uint32_t dx, uint32_t dy,
                                        uint32_t tile_index, grk_amd_tile_params* out)
{
    Layout l;
    const int rc = check_layout(im, l);
    if (rc != GRK_AMD_OK) return rc;
    if (!base || !out || tile_index >= l.tcols * l.trows || dx > 255 || dy > 255) return GRK_AMD_ERR_INVALID;
    return tile_comp_of(l, *base, dx, dy, tile_index, *out);
}

extern "C" int64_t grk_amd_write_codestream_subsampled(const grk_amd_image_layout* im, const grk_amd_tile_params* base,
                                                       const uint8_t* comp_dx, const uint8_t* comp_dy,
                                                       const grk_amd_coded_block* table, const uint8_t* coded, uint32_t flags,
                                                       uint8_t* out, uint64_t cap)
{
    // (out == NULL: the file's length alone, nothing written and `coded` not read; GRK_AMD_CS_BLOCK_MSBS goes to write_packet with
    //  the other flags)
    if (!base || !table || (out && !coded) || !comp_dx || !comp_dy) return GRK_AMD_ERR_INVALID;
    Layout l;
    int rc = check_layout(im, l);
    if (rc != GRK_AMD_OK) return rc;
    const uint32_t ntiles = l.tcols * l.trows, nc = base->num_comps;
    if ((flags & GRK_AMD_CS_TLM) && ntiles > 255) return GRK_AMD_ERR_UNSUPPORTED;
    // the multiple component transform needs its three components on one grid: otherwise the reference switches it off with a
    // warning (CodeStreamCompress.cpp:434-447), and COD says so
    grk_amd_tile_params based = *base;
    if (based.mct && nc >= 3 && !(comp_dx[0] == comp_dx[1] && comp_dx[1] == comp_dx[2] && comp_dy[0] == comp_dy[1] && comp_dy[1] == comp_dy[2]))
        based.mct = 0;
    base = &based;
    const int nparts = file_division(flags, *base, ntiles);
    if (nparts < 0) return nparts;
    const std::vector<uint32_t> per_tile(nparts > 1 ? ntiles : 0, (uint32_t)nparts);
    Division dv{nullptr, 0};
    std::vector<TileGeom> geoms(nc);
    std::vector<const TileGeom*> cg(nc);
    std::vector<uint64_t> row0(nc);
    grk_amd_tile_params p, pt;
    Out o{out, cap};
    uint64_t tlm_at = 0, row = 0;
    for (uint32_t t = 0; t < ntiles; ++t) {
        tile_of(l, *base, t, pt);
        uint64_t rows = 0;
        for (uint32_t c = 0; c < nc; ++c) {
            if ((rc = tile_comp_of(l, *base, comp_dx[c], comp_dy[c], t, p)) != GRK_AMD_OK) return rc;
            if ((rc = build_tile_geom(p, geoms[c])) != GRK_AMD_OK) return rc;
            cg[c] = &geoms[c]; row0[c] = rows; rows += geoms[c].blocks_per_comp;
        }
        if (t == 0) write_main_header(o, geoms[0], l.im, flags, ntiles, &tlm_at, comp_dx, comp_dy, nparts > 1 ? per_tile.data() : nullptr);
        const uint64_t len = write_tile_part(o, cg, row0, comp_dx, comp_dy, pt.tile_x0, pt.tile_y0, t, flags, table + row, coded, nparts > 1 ? &dv : nullptr);
        if (dv.error) return dv.error;
        row += rows;
        if (tlm_at && nparts > 1) { for (int k = 0; k < nparts; ++k) o.patch32(tlm_at + 5ull * ((uint64_t)t * nparts + k) + 1, dv.part_bytes[k]); }
        else if (tlm_at) o.patch32(tlm_at + 5ull * t + 1, (uint32_t)len);
    }
    o.u16(0xFFD9);
    if (o.ovf) return GRK_AMD_ERR_OVERFLOW;
    return (int64_t)o.n;
}

extern "C" int64_t grk_amd_write_codestream_ex(const grk_amd_tile_params* p, uint32_t img_w, uint32_t img_h,
                                               const grk_amd_coded_block* table, const uint8_t* coded, uint32_t flags,
                                               uint8_t* out, uint64_t cap)
{
    if (!p) return GRK_AMD_ERR_INVALID;
    const grk_amd_image_layout im = plain_layout(*p, img_w, img_h);
    // this entry point serves tables of ONE grk_amd_encode_tiles batch: every tile has to have *p's geometry
    Layout l;
    int rc = check_layout(&im, l);
    if (rc != GRK_AMD_OK) return rc;
    TileGeom g0, g;
    grk_amd_tile_params q;
    rc = build_tile_geom(*p, g0);
    if (rc != GRK_AMD_OK) return rc;
    for (uint32_t t = 1; t < l.tcols * l.trows; ++t) {
        tile_of(l, *p, t, q);
        if ((rc = build_tile_geom(q, g)) != GRK_AMD_OK) return rc;
        if (!same_geometry(g0, g)) return GRK_AMD_ERR_UNSUPPORTED;
    }
    return grk_amd_write_codestream_layout(&im, p, table, coded, flags, out, cap);
}

extern "C" int64_t grk_amd_write_codestream(const grk_amd_tile_params* p, uint32_t img_w, uint32_t img_h,
                                            const grk_amd_coded_block* table, const uint8_t* coded,
                                            uint8_t* out, uint64_t cap)
{
    return grk_amd_write_codestream_ex(p, img_w, img_h, table, coded, 0, out, cap);
}

extern "C" int64_t grk_amd_write_main_header_layout(const grk_amd_image_layout* im, const grk_amd_tile_params* base, uint32_t flags,
                                                    const uint32_t* tile_part_bytes, uint8_t* out, uint64_t cap)
{
    if (!base) return GRK_AMD_ERR_INVALID;
    Layout l;
    int rc = check_layout(im, l);
    if (rc != GRK_AMD_OK) return rc;
    const uint32_t ntiles = l.tcols * l.trows;
    if (flags & GRK_AMD_CS_TLM) { if (ntiles > 255) return GRK_AMD_ERR_UNSUPPORTED; if (!tile_part_bytes) return GRK_AMD_ERR_INVALID; }
    TileGeom g;
    grk_amd_tile_params p;
    tile_of(l, *base, 0, p);
    rc = build_tile_geom(p, g);
    if (rc != GRK_AMD_OK) return rc;
    Out o{out, cap};
    uint64_t tlm_at = 0;
    write_main_header(o, g, l.im, flags, ntiles, &tlm_at);
    for (uint32_t t = 0; tlm_at && t < ntiles; ++t) o.patch32(tlm_at + 5ull * t + 1, tile_part_bytes[t]);
    if (o.ovf) return GRK_AMD_ERR_OVERFLOW;
    return (int64_t)o.n;
}

// the main header grk_amd_write_codestream_subsampled writes, with the tile-parts' lengths in its TLM (image.h)
int64_t grk_amd::main_header_subsampled(const grk_amd_image_layout* im, const grk_amd_tile_params* base, const uint8_t* comp_dx,
                                        const uint8_t* comp_dy, uint32_t flags, const uint32_t* tile_part_bytes, uint8_t* out, uint64_t cap)
{
    if (!base || !comp_dx || !comp_dy) return GRK_AMD_ERR_INVALID;
    Layout l;
    int rc = check_layout(im, l);
    if (rc != GRK_AMD_OK) return rc;
    const uint32_t ntiles = l.tcols * l.trows, nc = base->num_comps;
    if (flags & GRK_AMD_CS_TLM) { if (ntiles > 255) return GRK_AMD_ERR_UNSUPPORTED; if (!tile_part_bytes) return GRK_AMD_ERR_INVALID; }
    grk_amd_tile_params based = *base, p;
    if (based.mct && nc >= 3 && !(comp_dx[0] == comp_dx[1] && comp_dx[1] == comp_dx[2] && comp_dy[0] == comp_dy[1] && comp_dy[1] == comp_dy[2]))
        based.mct = 0;
    TileGeom g;
    if ((rc = tile_comp_of(l, based, comp_dx[0], comp_dy[0], 0, p)) != GRK_AMD_OK) return rc;
    if ((rc = build_tile_geom(p, g)) != GRK_AMD_OK) return rc;
    Out o{out, cap};
    uint64_t tlm_at = 0;
    write_main_header(o, g, l.im, flags, ntiles, &tlm_at, comp_dx, comp_dy);
    for (uint32_t t = 0; tlm_at && t < ntiles; ++t) o.patch32(tlm_at + 5ull * t + 1, tile_part_bytes[t]);
    if (o.ovf) return GRK_AMD_ERR_OVERFLOW;
    return (int64_t)o.n;
}

extern "C" int64_t grk_amd_write_main_header(const grk_amd_tile_params* p, uint32_t img_w, uint32_t img_h, uint32_t flags,
                                             const uint32_t* tile_part_bytes, uint8_t* out, uint64_t cap)
{
    if (!p) return GRK_AMD_ERR_INVALID;
    const grk_amd_image_layout im = plain_layout(*p, img_w, img_h);
    return grk_amd_write_main_header_layout(&im, p, flags, tile_part_bytes, out, cap);
}

extern "C" int64_t grk_amd_write_tile_part(const grk_amd_tile_params* p, uint32_t tile_index, uint32_t flags,
                                           const grk_amd_coded_block* tile_table, const uint8_t* coded, uint8_t* out, uint64_t cap)
{
    if (!p || !tile_table || (out && !coded)) return GRK_AMD_ERR_INVALID;
    TileGeom g;
    int rc = build_tile_geom(*p, g);
    if (rc != GRK_AMD_OK) return rc;
    Out o{out, cap};
    write_tile_part(o, g, tile_index, flags, tile_table, coded);
    if (o.ovf) return GRK_AMD_ERR_OVERFLOW;
    return (int64_t)o.n;
}

extern "C" int64_t grk_amd_write_tile_parts(const grk_amd_tile_params* p, uint32_t tile_index, uint32_t flags, const grk_amd_coded_block* tile_table,
                                            const uint8_t* coded, const uint32_t* starts, uint32_t nparts, uint8_t* out, uint64_t cap, uint32_t* part_bytes)
{
    if (!p || !tile_table || (out && !coded) || (!starts != !nparts)) return GRK_AMD_ERR_INVALID;
    if (starts && (nparts > kMaxTileParts || starts[0] != 0)) return writer_refuse(GRK_AMD_ERR_INVALID, "grk_amd_write_tile_parts: 1 .. 255 tile-parts, the first from packet 0");
    if (!starts) { const int n = file_division(flags & ~(uint32_t)GRK_AMD_CS_TLM, *p, 1); if (n < 0) return n; }
    TileGeom g;
    int rc = build_tile_geom(*p, g);
    if (rc != GRK_AMD_OK) return rc;
    Out o{out, cap};
    Division dv{starts, nparts};
    write_tile_part(o, g, tile_index, flags, tile_table, coded, &dv);
    if (dv.error) return writer_refuse(dv.error, "grk_amd_write_tile_parts: starts that decrease or lie beyond the tile's packets");
    if (o.ovf) return GRK_AMD_ERR_OVERFLOW;
    if (part_bytes) std::copy(dv.part_bytes.begin(), dv.part_bytes.end(), part_bytes);
    return (int64_t)o.n;
}

extern "C" int64_t grk_amd_write_main_header_parts(const grk_amd_image_layout* im, const grk_amd_tile_params* base, uint32_t flags,
                                                   const uint32_t* parts_per_tile, const uint32_t* part_bytes, uint8_t* out, uint64_t cap)
{
    return grk_amd::main_header_parts(im, base, nullptr, nullptr, flags, parts_per_tile, part_bytes, out, cap);
}

// the main header of a file of divided tiles, plain (comp_dx == NULL) or sub-sampled (image.h)
int64_t grk_amd::main_header_parts(const grk_amd_image_layout* im, const grk_amd_tile_params* base, const uint8_t* comp_dx, const uint8_t* comp_dy,
                                   uint32_t flags, const uint32_t* parts_per_tile, const uint32_t* part_bytes, uint8_t* out, uint64_t cap)
{
    if (!base || !parts_per_tile || (!comp_dx != !comp_dy)) return GRK_AMD_ERR_INVALID;
    Layout l;
    int rc = check_layout(im, l);
    if (rc != GRK_AMD_OK) return rc;
    const uint32_t ntiles = l.tcols * l.trows, nc = base->num_comps;
    uint64_t entries = 0;
    for (uint32_t t = 0; t < ntiles; ++t) {
        if (!parts_per_tile[t] || parts_per_tile[t] > kMaxTileParts) return writer_refuse(GRK_AMD_ERR_INVALID, "1 .. 255 tile-parts per tile");
        entries += parts_per_tile[t];
    }
    if (flags & GRK_AMD_CS_TLM) {
        if (ntiles > 255) return GRK_AMD_ERR_UNSUPPORTED;
        if (entries > kMaxTlmEntries) return writer_refuse(GRK_AMD_ERR_UNSUPPORTED, std::to_string(entries) + " tile-parts: one TLM marker segment lists at most 13 106");
        if (!part_bytes) return GRK_AMD_ERR_INVALID;
    }
    grk_amd_tile_params based = *base, p;
    if (comp_dx && based.mct && nc >= 3 && !(comp_dx[0] == comp_dx[1] && comp_dx[1] == comp_dx[2] && comp_dy[0] == comp_dy[1] && comp_dy[1] == comp_dy[2]))
        based.mct = 0;
    TileGeom g;
    if (comp_dx) { if ((rc = tile_comp_of(l, based, comp_dx[0], comp_dy[0], 0, p)) != GRK_AMD_OK) return rc; }
    else tile_of(l, based, 0, p);
    if ((rc = build_tile_geom(p, g)) != GRK_AMD_OK) return rc;
    Out o{out, cap};
    uint64_t tlm_at = 0;
    write_main_header(o, g, l.im, flags, ntiles, &tlm_at, comp_dx, comp_dy, parts_per_tile);
    for (uint64_t e = 0; tlm_at && e < entries; ++e) o.patch32(tlm_at + 5 * e + 1, part_bytes[e]);
    if (o.ovf) return GRK_AMD_ERR_OVERFLOW;
    return (int64_t)o.n;
}

namespace grk_amd {
int64_t plan_tile_part(const grk_amd_tile_params& p, uint32_t tile_index, uint32_t flags, const grk_amd_coded_block* tile_table,
                       std::vector<uint8_t>& lit, std::vector<grk_amd_tp_segment>& segs)
{
    if (flags & GRK_AMD_CS_BLOCK_MSBS) return GRK_AMD_ERR_UNSUPPORTED;      // (per-block zero bit-planes: the host writers only)
    if (flags & GRK_AMD_CS_TP(3)) return GRK_AMD_ERR_UNSUPPORTED;           // (one tile-part per tile)
    TileGeom g;
    const int rc = build_tile_geom(p, g);
    if (rc != GRK_AMD_OK) return rc;
    lit.clear(); segs.clear();
    lit.reserve((size_t)g.blocks_per_comp * p.num_comps * 5 + 256);
    segs.reserve((size_t)g.blocks_per_comp * p.num_comps + 64);
    Out o{nullptr, 0};
    o.lit = &lit; o.segs = &segs;
    write_tile_part(o, g, tile_index, flags, tile_table, nullptr);
    return (int64_t)o.n;
}
} // namespace grk_amd

namespace grk_amd {
// What the header kernel needs to know about a tile's packets: component c's tile-component has the geometry cg[c] and its rows start
// at row0[c] of the tile's table -- the arguments of write_tile_part, and its packet sequence (t2_order.h).
// (msbs: the plan of the header kernel's general zero-bit-plane tree)
static int device_plan(const std::vector<const TileGeom*>& cg, const std::vector<uint64_t>& row0, const uint8_t* comp_dx, const uint8_t* comp_dy,
                       uint32_t gx0, uint32_t gy0, uint32_t flags, bool msbs, T2Plan& out)
{
    if (cg.empty() || row0.size() != cg.size()) return GRK_AMD_ERR_INVALID;
    uint64_t rows = 0;
    for (size_t c = 0; c < cg.size(); ++c) rows = std::max(rows, row0[c] + cg[c]->blocks_per_comp);
    if (rows > 0xFFFFFFFFull) return GRK_AMD_ERR_UNSUPPORTED;               // (T2Packet::row0 and the kernels' rows per tile are 32 bits)
    const std::vector<Pk> seq = packet_order(cg, comp_dx, comp_dy, gx0, gy0, (flags >> GRK_AMD_CS_PROG_SHIFT) & 7u);
    { const int np = tile_part_starts(seq, flags, cg[0]->p.num_levels, (uint32_t)cg.size(), out.part_starts); if (np < 0) return np; }
    out.packets.clear();
    out.packet_of_block.assign((size_t)rows, 0xFFFFFFFFu);
    uint64_t u = 0, h = 0, v = 0;
    for (const Pk& q : seq) {
        const TileGeom& g = *cg[q.c];
        const ResGeom& R = g.res[q.r];
        T2Packet k{};
        k.row0 = (uint32_t)row0[q.c];
        uint64_t bits = 1, nodes = 0;
        for (uint32_t bi = 0; bi < R.num_bands; ++bi) {
            const BandGeom& B = R.band[bi];
            const BandGeom::Prec& P = B.prec[q.pi];
            if (!P.gw || !P.gh) continue;
            const uint32_t b = k.nbands++;
            k.first_block[b] = P.first_block; k.gw[b] = P.gw; k.gh[b] = P.gh; k.kmax[b] = B.kmax;
            k.height[b] = (uint32_t)tag_tree_height(P.gw, P.gh);
            if (k.height[b] > kT2MaxHeight) return GRK_AMD_ERR_UNSUPPORTED;  // (t2_bits.h: a path's ones and the pass bit in 64 bits)
            const uint64_t n = (uint64_t)P.gw * P.gh;
            for (uint64_t i = 0; i < n; ++i) {
                uint32_t& of = out.packet_of_block[k.row0 + P.first_block + i];
                if (of != 0xFFFFFFFFu) return GRK_AMD_ERR_INVALID;          // (components whose rows overlap)
                of = (uint32_t)out.packets.size();
            }
            k.nblocks += (uint32_t)n;
            // per block: two paths of at most `height` nodes, the pass bit, Lblock's comma code and the length
            bits += n * (2ull * k.height[b] + 1 + (kT2MaxLenBits - 3 + 1) + kT2MaxLenBits) + B.kmax;
            // the general tree: a path's zeros end at the block's own value, and every level of the band's tree holds a byte per node
            if (msbs) { bits += n * kT2MaxMsbs; nodes += t2_tree_nodes(P.gw, P.gh); }
        }
        if (bits > 0x7FFFFFFFull) return GRK_AMD_ERR_UNSUPPORTED;
        k.u_at = (uint32_t)u; k.u_words = (uint32_t)((bits + 31) / 32 + 2);
        k.h_at = (uint32_t)h;
        k.v_at = (uint32_t)v;
        u += (k.u_words + 31u) & ~31ull;                         // (packets start on 128-byte lines)
        h += ((bits + 6) / 7 + 2 + 15) & ~15ull;                 // a stuffed byte carries at least 7 bits
        v += (nodes + 15) & ~15ull;
        if (u > 0x3FFFFFFFull || h > 0xFFFFFFFFull || v > 0xFFFFFFFFull) return GRK_AMD_ERR_UNSUPPORTED;
        out.packets.push_back(k);
    }
    for (uint32_t of : out.packet_of_block) if (of == 0xFFFFFFFFu) return GRK_AMD_ERR_INVALID;     // (every block lies in one precinct)
    out.u_words = (uint32_t)u; out.h_bytes = (uint32_t)h; out.v_bytes = (uint32_t)v;
    return GRK_AMD_OK;
}

int t2_device_plan_joint(const std::vector<const TileGeom*>& cg, const std::vector<uint64_t>& row0, const uint8_t* comp_dx, const uint8_t* comp_dy,
                         uint32_t gx0, uint32_t gy0, uint32_t flags, T2Plan& out)
{
    if (flags & GRK_AMD_CS_BLOCK_MSBS) return GRK_AMD_ERR_UNSUPPORTED;      // (the general tree is asked for by name: below)
    return device_plan(cg, row0, comp_dx, comp_dy, gx0, gy0, flags, false, out);
}

int t2_device_plan_joint_msbs(const std::vector<const TileGeom*>& cg, const std::vector<uint64_t>& row0, const uint8_t* comp_dx,
                              const uint8_t* comp_dy, uint32_t gx0, uint32_t gy0, uint32_t flags, T2Plan& out)
{
    return device_plan(cg, row0, comp_dx, comp_dy, gx0, gy0, flags & ~(uint32_t)GRK_AMD_CS_BLOCK_MSBS, true, out);
}

// ... of a tile without sub-sampling: every component has the tile's geometry, component c's rows start at c x blocks_per_comp
int t2_device_plan(const TileGeom& g, uint32_t flags, T2Plan& out)
{
    const grk_amd_tile_params& p = g.p;
    std::vector<const TileGeom*> cg(p.num_comps, &g);
    std::vector<uint64_t> row0(p.num_comps);
    for (uint32_t c = 0; c < p.num_comps; ++c) row0[c] = (uint64_t)c * g.blocks_per_comp;
    return t2_device_plan_joint(cg, row0, nullptr, nullptr, p.tile_x0, p.tile_y0, flags, out);
}

int t2_device_plan_msbs(const TileGeom& g, uint32_t flags, T2Plan& out)
{
    const grk_amd_tile_params& p = g.p;
    std::vector<const TileGeom*> cg(p.num_comps, &g);
    std::vector<uint64_t> row0(p.num_comps);
    for (uint32_t c = 0; c < p.num_comps; ++c) row0[c] = (uint64_t)c * g.blocks_per_comp;
    return t2_device_plan_joint_msbs(cg, row0, nullptr, nullptr, p.tile_x0, p.tile_y0, flags, out);
}

} // namespace grk_amd

extern "C" int64_t grk_amd_plan_tile_part(const grk_amd_tile_params* p, uint32_t tile_index, uint32_t flags,
                                          const grk_amd_coded_block* tile_table, uint8_t* literal, uint64_t literal_cap, uint64_t* literal_len,
                                          grk_amd_tp_segment* segments, uint64_t segment_cap, uint64_t* num_segments)
{
    if (!p || !tile_table || !literal_len || !num_segments) return GRK_AMD_ERR_INVALID;
    if (flags & GRK_AMD_CS_BLOCK_MSBS) return GRK_AMD_ERR_UNSUPPORTED;      // (per-block zero bit-planes: the host writers only)
    if (flags & GRK_AMD_CS_TP(3)) return writer_refuse(GRK_AMD_ERR_UNSUPPORTED, "grk_amd_plan_tile_part plans one tile-part per tile: GRK_AMD_CS_TP is not taken");
    std::vector<uint8_t> lit;
    std::vector<grk_amd_tp_segment> segs;
    const int64_t total = grk_amd::plan_tile_part(*p, tile_index, flags, tile_table, lit, segs);
    if (total < 0) return total;
    struct { uint64_t n; } o{(uint64_t)total};
    *literal_len = lit.size(); *num_segments = segs.size();
    if (literal && segments) {
        if (lit.size() > literal_cap || segs.size() > segment_cap) return GRK_AMD_ERR_OVERFLOW;
        std::memcpy(literal, lit.data(), lit.size());
        std::memcpy(segments, segs.data(), segs.size() * sizeof(grk_amd_tp_segment));
    }
    return (int64_t)o.n;
}

// Random access into a codestream (the reader's side of markers/LengthMarkers.cpp:91-164): where every tile-part starts
// and how long it is -- from the TLM marker segments when the main header carries them (no byte of a tile-part is
// touched), else by hopping from SOT to SOT over Psot.
extern "C" int64_t grk_amd_locate_tile_parts(const uint8_t* cs, uint64_t len, uint64_t* offsets, uint32_t* lengths,
                                             uint16_t* tile_index, uint64_t cap, int* used_tlm)
{
    if (!cs || len < 4 || cs[0] != 0xFF || cs[1] != 0x4F) return GRK_AMD_ERR_INVALID;
    auto be16 = [&](uint64_t i) { return (uint32_t)(cs[i] << 8 | cs[i + 1]); };
    auto be32 = [&](uint64_t i) { return (uint32_t)cs[i] << 24 | (uint32_t)cs[i + 1] << 16 | (uint32_t)cs[i + 2] << 8 | cs[i + 3]; };
    std::vector<std::pair<uint32_t, uint32_t>> tlm;       // (tile index or 0xFFFFFFFF = "next", length), in marker order
    uint64_t at = 2;
    bool have_tlm = false;
    while (at + 4 <= len) {
        const uint32_t m = be16(at);
        if (m == 0xFF90) break;
        const uint32_t l = be16(at + 2);
        if (m < 0xFF00 || l < 2 || at + 2 + l > len) return GRK_AMD_ERR_INVALID;
        if (m == 0xFF55 && l >= 4) {
            have_tlm = true;
            const uint32_t stlm = cs[at + 5], st = (stlm >> 4) & 3u, sp = (stlm >> 6) & 1u;
            const uint32_t rec = st + (sp ? 4u : 2u);
            if (st == 3) return GRK_AMD_ERR_INVALID;
            for (uint64_t q = at + 6; q + rec <= at + 2 + l; q += rec) {
                const uint32_t ti = st == 0 ? 0xFFFFFFFFu : st == 1 ? cs[q] : be16(q);
                tlm.emplace_back(ti, sp ? be32(q + st) : be16(q + st));
            }
        }
        at += 2 + l;
    }
    if (at + 12 > len || be16(at) != 0xFF90) return GRK_AMD_ERR_INVALID;
    if (used_tlm) *used_tlm = have_tlm ? 1 : 0;
    uint64_t n = 0;
    if (have_tlm) {
        uint32_t next = 0;
        for (const auto& e : tlm) {
            const uint32_t ti = e.first == 0xFFFFFFFFu ? next : e.first;
            if (at + e.second > len) return GRK_AMD_ERR_INVALID;
            if (n < cap) { if (offsets) offsets[n] = at; if (lengths) lengths[n] = e.second; if (tile_index) tile_index[n] = (uint16_t)ti; }
            ++n; at += e.second; next = ti + 1;
        }
        return (int64_t)n;
    }
    while (at + 12 <= len && be16(at) == 0xFF90) {
        const uint32_t psot = be32(at + 6);
        const uint64_t l = psot ? psot : len - 2 - at;            // Psot 0: the last tile-part runs to EOC
        if (l < 14 || at + l > len) return GRK_AMD_ERR_INVALID;
        if (n < cap) { if (offsets) offsets[n] = at; if (lengths) lengths[n] = (uint32_t)l; if (tile_index) tile_index[n] = (uint16_t)be16(at + 4); }
        ++n; at += l;
    }
    return (int64_t)n;
}
