// grok_amd/csrc/t2_parse.h -- the Tier-2 READER's parse core as the device reader runs it (kernels_t2read.hip: KL, KH, KC): the
// arithmetic alone, for the kernels and for a host program (tests/c/t2_parse_units.cpp) alike.  No HIP in here.
//
// A second implementation beside t2_reader.cpp, written from ITU-T T.800 Annex A (SOT, PLT), B.10 (packet headers, B.10.1 bit
// stuffing, B.10.2 tag trees, B.10.7 lengths) for files of ONE layer: a precinct has one packet, a block is included once or never,
// an HT block has one pass, a Part-1 block all its passes in one codeword segment.  t2_reader.cpp does not use it and stays the
// oracle.  Every function reads the stream through a source `Src` (uint32_t byte(uint64_t pos)) and only at positions it has
// checked against the end of its container; every loop has a bound that the stream's content cannot raise (kT2p* below).
#pragma once
#include <cstdint>
#include "t2_bits.h"        // GRK_T2_FN

// a host program counts the steps of the core's loops through this (id: T2pLoop, n: the steps one run of the loop took)
#ifndef GRK_T2P_COUNT
#define GRK_T2P_COUNT(id, n) ((void)0)
#endif
// a kernel whose lanes all run the same parse says so about what it loads (a wave-uniform value: KC keeps the parse in scalar registers)
#ifndef GRK_T2P_UNIFORM
#define GRK_T2P_UNIFORM(v) (v)
#endif

namespace grk_amd {

constexpr uint32_t kT2pThreshold = 65;      // the zero-bit-plane tree is walked with this threshold: steps per node
constexpr uint32_t kT2pMaxLblock = 32;
constexpr uint32_t kT2pMaxLenBits = 32;
constexpr uint32_t kT2pMaxPasses = 164;
constexpr uint32_t kT2pMaxLevels = 17;      // tag-tree levels
constexpr uint32_t kT2pPltBytes = 5;        // bytes of one PLT entry
enum T2pLoop : int { kT2pLoopTree = 0, kT2pLoopLblock = 1, kT2pLoopLenBits = 2, kT2pLoopPasses = 3, kT2pLoopLevels = 4, kT2pLoopPlt = 5, kT2pLoops = 6,
                     kT2pSeenFF = 6 /* a header byte behind 0xFF */, kT2pSeenEndFF = 7 /* a header that ends on 0xFF */, kT2pCounts = 8 };

// why a stream is refused; t2p_code() gives the code the host reader has for the same condition
enum T2pWhy : uint32_t {
    kT2pOk = 0,
    kT2pNotLocated, kT2pNoSot, kT2pTileIndex, kT2pMultiPart, kT2pPsotTlm, kT2pManyParts, kT2pNoPart,                      // KL
    kT2pNoSod, kT2pBrokenSegment, kT2pBrokenPlt, kT2pPltWrap, kT2pPltMany, kT2pMarker, kT2pPacketsBytes, kT2pPltCount,    // KH
    kT2pNoSop, kT2pZeroPlanes, kT2pHtPasses, kT2pPasses, kT2pLblock, kT2pLenBits, kT2pBlockWrap, kT2pHeaderPast,          // KC
    kT2pNoEph, kT2pBodyPast, kT2pPltSize, kT2pTail, kT2pPart1Planes,
    kT2pTpsot, kT2pTnsot, kT2pPartsOfTile, kT2pPartsOfFile, kT2pPsotZero, kT2pPartPlt, kT2pTileEnds,                       // KL-P, KH-P, the chains' part stepping
    kT2pHtSet,                                                                                                             // KC-L reading HT refinement passes
    kT2pWhys
};
GRK_T2_FN int t2p_code(uint32_t why)
{
    if (why == kT2pOk) return 0;
    return why == kT2pMultiPart || why == kT2pManyParts || why == kT2pMarker || why == kT2pHtPasses || why == kT2pHtSet || why == kT2pPartsOfTile || why == kT2pPartsOfFile
               ? -2 /* GRK_AMD_ERR_UNSUPPORTED */ : -3 /* GRK_AMD_ERR_INVALID */;
}
GRK_T2_FN const char* t2p_text(uint32_t why)
{
    switch (why) {
    case kT2pNotLocated: return "the tile-parts cannot be located";
    case kT2pNoSot: return "no SOT marker segment where a tile-part should start";
    case kT2pTileIndex: return "a tile-part's tile index";
    case kT2pMultiPart: case kT2pManyParts: return "more than one tile-part per tile";
    case kT2pPsotTlm: return "Psot is not TLM's length";
    case kT2pNoPart: return "a tile without a tile-part";
    case kT2pNoSod: return "no SOD marker";
    case kT2pBrokenSegment: return "a broken marker segment in the tile-part header";
    case kT2pBrokenPlt: return "a broken PLT";
    case kT2pPltWrap: return "a PLT packet length wraps";
    case kT2pPltMany: return "PLT lists more than the tile's packets";
    case kT2pMarker: return "a marker segment in the tile-part header that this reader does not take";
    case kT2pPacketsBytes: return "more packets than bytes";
    case kT2pPltCount: return "PLT does not list the tile's packets";
    case kT2pNoSop: return "no SOP marker segment with the packet's number";
    case kT2pZeroPlanes: return "zero bit-planes without end";
    case kT2pHtPasses: return "an HT code-block with more than one pass";
    case kT2pHtSet: return "an HT code-block with more than one pass of a kind (more than 3 passes: placeholder passes or a second HT set)";
    case kT2pPasses: return "more than 164 coding passes";
    case kT2pLblock: return "Lblock beyond 32";
    case kT2pLenBits: return "a length of more than 32 bits";
    case kT2pBlockWrap: return "a block length wraps";
    case kT2pHeaderPast: return "the header runs past its container";
    case kT2pNoEph: return "no EPH marker";
    case kT2pBodyPast: return "the body runs past its container";
    case kT2pPltSize: return "the packet's size is not PLT's";
    case kT2pTail: return "bytes behind the last packet";
    case kT2pPart1Planes: return "more passes than the block's bit-planes hold";
    case kT2pTpsot: return "a TPsot that is missing, repeated or out of file order";
    case kT2pTnsot: return "TNsot does not fit the tile's tile-parts";
    case kT2pPartsOfTile: return "more than 255 tile-parts of one tile";
    case kT2pPartsOfFile: return "more than 65535 tile-parts";
    case kT2pPsotZero: return "Psot 0 in a tile-part that is not the file's last";
    case kT2pPartPlt: return "the PLT lengths do not add up to the tile-part";
    case kT2pTileEnds: return "the tile's last tile-part ends before its last packet";
    default: return "";
    }
}

// ---- the status word ---------------------------------------------------------------------------------------------------------------
// One 64-bit word per call, combined with atomicMin: the smallest is the failure a reader that goes through the file on one thread
// meets first.  Locating the tile-parts comes before every tile (number: the tile-part in file order; behind them "more tile-parts
// than tiles", then the tiles without one); a tile's stages are 0 its tile-part header, 1 its packets (number: the packet; the
// tile's packets: what is left behind the last), 2 the Part-1 rows' bit-planes (number: the row), as read_tile makes that check last.
constexpr uint64_t kT2pNoStatus = ~0ull;
GRK_T2_FN uint64_t t2p_status_locate(uint32_t number, uint32_t why) { return (uint64_t)number << 8 | why; }
GRK_T2_FN uint64_t t2p_status_tile(uint32_t tile, uint32_t stage, uint32_t number, uint32_t why)
{
    return 1ull << 62 | (uint64_t)(tile & 0xFFFFu) << 42 | (uint64_t)(stage & 3u) << 40 | (uint64_t)number << 8 | why;
}
GRK_T2_FN bool t2p_status_is_tile(uint64_t s) { return (s >> 62) == 1; }
GRK_T2_FN uint32_t t2p_status_tile_of(uint64_t s) { return (uint32_t)(s >> 42) & 0xFFFFu; }
GRK_T2_FN uint32_t t2p_status_stage(uint64_t s) { return (uint32_t)(s >> 40) & 3u; }
GRK_T2_FN uint32_t t2p_status_number(uint64_t s) { return (uint32_t)(s >> 8); }
GRK_T2_FN uint32_t t2p_status_why(uint64_t s) { return (uint32_t)s & 0xFFu; }

// ---- what the plan (t2_read_plan.cpp) says about a packet ---------------------------------------------------------------------------
struct T2ReadBand {
    uint32_t gw, gh;            // the block grid of the band's part of the precinct
    uint32_t first_row;         // its first block's row in the TILE's table (raster order from there)
    uint32_t node_at;           // the inclusion tree's nodes in the tile's node scratch (bytes); the zero-bit-plane tree's follow
    uint32_t nodes, nlev;       // nodes and levels of one tree
    uint32_t kbits;             // Part-1: the band's expn + guard bits - 1
};
struct T2ReadPacket {
    uint32_t c, r, pi, nbands;
    T2ReadBand band[3];
    uint32_t node_at, node_n;   // all of the packet's nodes: bytes [node_at, node_at + node_n) of the tile's node scratch
    uint32_t nblocks, pad;
};

template <class Src> GRK_T2_FN uint32_t t2p_u16(Src& s, uint64_t i) { return s.byte(i) << 8 | s.byte(i + 1); }
template <class Src> GRK_T2_FN uint32_t t2p_u32(Src& s, uint64_t i) { return s.byte(i) << 24 | s.byte(i + 1) << 16 | s.byte(i + 2) << 8 | s.byte(i + 3); }

// ---- the bit reader (B.10.1) ---------------------------------------------------------------------------------------------------------
// MSB first; a byte behind 0xFF carries 7 bits.  Never reads outside [pos at the start, end): past `end` every bit is 0 and err is set.
template <class Src> struct T2pBits {
    Src& s; uint64_t pos, end; uint32_t cur, n; bool err;
    GRK_T2_FN T2pBits(Src& src, uint64_t lo, uint64_t hi) : s(src), pos(lo), end(hi), cur(0), n(0), err(false) {}
    GRK_T2_FN uint32_t bit()
    {
        if (!n) {
            if (pos >= end) { err = true; return 0; }
            const bool ff = cur == 0xFF;
            if (ff) GRK_T2P_COUNT(kT2pSeenFF, 1);
            cur = s.byte(pos++);
            n = ff ? 7u : 8u;
        }
        --n;
        return (cur >> n) & 1u;
    }
    GRK_T2_FN uint32_t bits(uint32_t k)         // k <= kT2pMaxLenBits
    {
        uint32_t v = 0;
        GRK_T2P_COUNT(kT2pLoopLenBits, k);
        for (uint32_t i = 0; i < k && i < kT2pMaxLenBits; ++i) v = (v << 1) | bit();
        return v;
    }
    GRK_T2_FN uint64_t align()                  // the header's end: behind a last byte of 0xFF lies one stuffed byte
    {
        if (cur == 0xFF) { GRK_T2P_COUNT(kT2pSeenEndFF, 1); if (pos >= end) err = true; else ++pos; }
        n = 0; cur = 0;
        return pos;
    }
};

// ---- the tag tree (B.10.2), general form ---------------------------------------------------------------------------------------------
// Per node one byte: the lower bound so far << 1 | "value known" (a bound stays below the threshold, 65 at most).  Level lv of a
// grid of gw x gh leaves is ceil(gw / 2^lv) x ceil(gh / 2^lv); the levels lie one after the other from the leaves up, at most 17.
GRK_T2_FN void t2p_tree_shape(uint32_t gw, uint32_t gh, uint32_t* nlev, uint32_t* nodes)
{
    uint32_t n = 0, l = 0;
    uint64_t w = gw, h = gh;
    for (;;) {
        n += (uint32_t)(w * h); ++l;
        if ((w == 1 && h == 1) || l == kT2pMaxLevels) break;
        w = (w + 1) >> 1; h = (h + 1) >> 1;
    }
    *nlev = l; *nodes = n;
}
GRK_T2_FN uint32_t t2p_level_dim(uint32_t g, uint32_t lv) { return (uint32_t)(((uint64_t)g + (1ull << lv) - 1) >> lv); }

template <class Src>
GRK_T2_FN uint32_t t2p_tree_decode(uint8_t* nodes, uint32_t gw, uint32_t gh, uint32_t nlev, uint32_t total, uint32_t x, uint32_t y,
                                   uint32_t threshold, T2pBits<Src>& br, bool& known)
{
    uint32_t low = 0;
    uint32_t off = total;
    GRK_T2P_COUNT(kT2pLoopLevels, nlev);
    for (uint32_t i = 0; i < nlev && i < kT2pMaxLevels; ++i) {
        const uint32_t lv = nlev - 1 - i;
        const uint32_t w = t2p_level_dim(gw, lv), h = t2p_level_dim(gh, lv);
        off -= w * h;
        uint8_t* const nd = nodes + off + (y >> lv) * w + (x >> lv);
        const uint32_t cell = GRK_T2P_UNIFORM((uint32_t)*nd);
        uint32_t v = cell >> 1;
        bool k = (cell & 1u) != 0;
        if (v < low) v = low;
        uint32_t steps = 0;
        while (!k && v < threshold && steps < kT2pThreshold) { if (br.bit()) k = true; else ++v; ++steps; }
        GRK_T2P_COUNT(kT2pLoopTree, steps);
        *nd = (uint8_t)(v << 1 | (k ? 1u : 0u));
        low = v;
        known = k;
    }
    return low;
}

GRK_T2_FN uint32_t t2p_floor_log2(uint32_t v) { return v ? 31u - (uint32_t)__builtin_clz(v) : 0u; }

// ---- one packet header, one layer -----------------------------------------------------------------------------------------------------
// The packet `q` of the tile's packet `number`, from pos (advanced to behind the packet's bodies) and not beyond `end`; `nodes`: the
// tile's node scratch, the packet's share of it zeroed.  Every block of the packet goes to sink.put(row, length, msbs, rel) in row
// order -- rel: where its bytes start, counted from the end of the header (and of EPH) --, and afterwards *body_at is that end, so
// that a row's offset is *body_at + rel.  A block that is not included, or has no bytes: length 0 and the zero bit-planes met, or 0.
// Part-1 (ht false): msbs is numbps | passes << 8, or 0 for a block without bytes; sink.part1_planes(row) is told of a block whose
// passes its bit-planes cannot hold, and the parse goes on (the host reader makes that check behind the tile's last packet).
template <class Src, class Sink>
GRK_T2_FN uint32_t t2p_read_packet(Src& src, const T2ReadPacket& q, uint8_t* nodes, bool ht, bool sop, bool eph, uint32_t number, uint64_t& pos,
                                   uint64_t end, Sink& sink, uint64_t* body_at)
{
    if (pos > end) return kT2pBodyPast;
    if (sop) {
        if (end - pos < 6 || t2p_u16(src, pos) != 0xFF91 || t2p_u16(src, pos + 2) != 4 || t2p_u16(src, pos + 4) != (number & 0xFFFFu)) return kT2pNoSop;
        pos += 6;
    }
    T2pBits<Src> br(src, pos, end);
    uint64_t sum = 0;
    const bool present = br.bit() != 0;
    for (uint32_t bi = 0; bi < q.nbands && bi < 3; ++bi) {
        const T2ReadBand& B = q.band[bi];
        uint8_t* const incl = nodes + B.node_at;
        uint8_t* const zbpt = incl + B.nodes;
        uint32_t row = B.first_row;
        for (uint32_t y = 0; y < B.gh; ++y)
            for (uint32_t x = 0; x < B.gw; ++x, ++row) {
                if (!present) { sink.put(row, 0, 0, 0); continue; }
                bool known = false;
                const uint32_t v = t2p_tree_decode(incl, B.gw, B.gh, B.nlev, B.nodes, x, y, 1, br, known);
                if (!known || v > 0) { sink.put(row, 0, 0, 0); continue; }
                const uint32_t z = t2p_tree_decode(zbpt, B.gw, B.gh, B.nlev, B.nodes, x, y, kT2pThreshold, br, known);
                if (!known || br.err) return kT2pZeroPlanes;
                uint32_t np;                                       // Table B.4
                if (!br.bit()) np = 1;
                else if (!br.bit()) np = 2;
                else {
                    uint32_t t = br.bits(2);
                    if (t < 3) np = 3 + t;
                    else { t = br.bits(5); np = t < 31 ? 6 + t : 37 + br.bits(7); }
                }
                GRK_T2P_COUNT(kT2pLoopPasses, np);
                if (ht && np != 1) return kT2pHtPasses;
                if (np > kT2pMaxPasses) return kT2pPasses;
                uint32_t lb = 3;
                while (br.bit()) if (++lb > kT2pMaxLblock) return kT2pLblock;
                GRK_T2P_COUNT(kT2pLoopLblock, lb);
                const uint32_t nb = lb + t2p_floor_log2(np);
                if (nb > kT2pMaxLenBits) return kT2pLenBits;
                const uint32_t len = br.bits(nb);
                uint32_t msbs = z;
                if (!ht) {
                    msbs = 0;
                    if (len) {
                        const int numbps = (int)B.kbits - (int)z;
                        if (numbps < 1 || (int)np > 3 * numbps - 2) sink.part1_planes(row);
                        msbs = (uint32_t)numbps | np << 8;
                    }
                }
                sink.put(row, len, msbs, sum);
                sum += len;
            }
    }
    pos = br.align();
    if (br.err) return kT2pHeaderPast;
    if (eph) {
        if (end - pos < 2 || t2p_u16(src, pos) != 0xFF92) return kT2pNoEph;
        pos += 2;
    }
    if (sum > end - pos) return kT2pBodyPast;
    *body_at = pos;
    pos += sum;
    return kT2pOk;
}
// what a row that sink.put() stored becomes once the header's end is known
GRK_T2_FN uint64_t t2p_row_offset(uint32_t length, uint64_t rel, uint64_t body_at) { return length ? body_at + rel : 0; }

// ---- SOT (A.4.2) ------------------------------------------------------------------------------------------------------------------------
// The tile-part that should lie at [at, at + ln) of a stream of `len` bytes: its SOT checked as locate_stream_parts checks it.
// want_isot: the tile index TLM names (or 0xFFFFFFFF: none); *isot: the tile it is for
template <class Src>
GRK_T2_FN uint32_t t2p_check_sot(Src& s, uint64_t len, uint64_t at, uint32_t ln, uint32_t num_tiles, uint32_t want_isot, uint32_t* isot)
{
    if (ln < 14 || at > len || ln > len - at || t2p_u16(s, at) != 0xFF90 || t2p_u16(s, at + 2) != 10) return kT2pNoSot;
    const uint32_t i = t2p_u16(s, at + 4);
    if (i >= num_tiles || (want_isot != 0xFFFFFFFFu && i != (want_isot & 0xFFFFu))) return kT2pTileIndex;
    *isot = i;
    if (s.byte(at + 10) != 0 || s.byte(at + 11) > 1) return kT2pMultiPart;
    const uint32_t psot = t2p_u32(s, at + 6);
    if (psot && psot != ln) return kT2pPsotTlm;
    return kT2pOk;
}
// The same for a file whose tiles may be divided into tile-parts (locate_stream_parts): the SOT alone, TPsot and TNsot handed out
// for the checks across a tile's tile-parts.  last: the tile-part is the file's last (Psot may be 0 there only)
constexpr uint32_t kT2pMaxPartsOfTile = 255, kT2pMaxPartsOfFile = 65535;
template <class Src>
GRK_T2_FN uint32_t t2p_check_sot_part(Src& s, uint64_t len, uint64_t at, uint32_t ln, uint32_t num_tiles, uint32_t want_isot, bool last, uint32_t* isot,
                                      uint32_t* tpsot, uint32_t* tnsot)
{
    if (ln < 14 || at > len || ln > len - at || t2p_u16(s, at) != 0xFF90 || t2p_u16(s, at + 2) != 10) return kT2pNoSot;
    const uint32_t i = t2p_u16(s, at + 4);
    if (i >= num_tiles || (want_isot != 0xFFFFFFFFu && i != (want_isot & 0xFFFFu))) return kT2pTileIndex;
    *isot = i; *tpsot = s.byte(at + 10); *tnsot = s.byte(at + 11);
    const uint32_t psot = t2p_u32(s, at + 6);
    if (psot && psot != ln) return kT2pPsotTlm;
    if (!psot && !last) return kT2pPsotZero;
    return kT2pOk;
}
// One hop of the Psot chain from `at` (a file without TLM): 0 no further tile-part, 1 one of *ln bytes, 2 a tile-part that does
// not fit the stream
template <class Src> GRK_T2_FN int t2p_hop(Src& s, uint64_t len, uint64_t at, uint64_t* ln)
{
    if (at > len || len - at < 12 || t2p_u16(s, at) != 0xFF90) return 0;
    const uint32_t psot = t2p_u32(s, at + 6);
    const uint64_t l = psot ? psot : len - 2 - at;             // Psot 0: the last tile-part runs to EOC
    if (l < 14 || l > len - at) return 2;
    *ln = l;
    return 1;
}

// ---- a tile-part header's marker segments (A.4.2, A.7.3) -------------------------------------------------------------------------------
// The segment at pos of a tile-part that ends at `end`: 0 SOD (*next behind it), 1 PLT with its entries' bytes at [*lo, *hi),
// 2 a segment to pass over, else -why.  *next: the next segment
template <class Src> GRK_T2_FN int t2p_header_segment(Src& s, uint64_t pos, uint64_t end, uint64_t* next, uint64_t* lo, uint64_t* hi)
{
    if (pos > end || end - pos < 2) return -(int)kT2pNoSod;
    const uint32_t m = t2p_u16(s, pos);
    if (m == 0xFF93) { *next = pos + 2; return 0; }
    if (end - pos < 4) return -(int)kT2pNoSod;
    const uint32_t l = t2p_u16(s, pos + 2);
    if (m < 0xFF30 || l < 2 || (uint64_t)l + 2 > end - pos) return -(int)kT2pBrokenSegment;
    *next = pos + 2 + l;
    if (m == 0xFF58) {
        if (l < 3) return -(int)kT2pBrokenPlt;
        *lo = pos + 5; *hi = pos + 2 + l;
        return 1;
    }
    if (m == 0xFF64) return 2;                                  // COM
    return -(int)kT2pMarker;
}
// PLT's entries are numbers of 7 bits per byte, the last byte of one with bit 7 clear.  Is byte i of [lo, hi) such a terminator?
template <class Src> GRK_T2_FN bool t2p_plt_terminator(Src& s, uint64_t i) { return (s.byte(i) & 0x80u) == 0; }
// The entry that the terminator at i ends: its bytes reach back to behind the terminator before it, or to lo -- five at most, and a
// value of 32 bits (an entry does not continue from one PLT marker segment into the next).  kT2pOk or why not
template <class Src> GRK_T2_FN uint32_t t2p_plt_entry(Src& s, uint64_t lo, uint64_t i, uint32_t* value)
{
    uint64_t from = i;
    uint32_t steps = 0;
    while (from > lo && steps < kT2pPltBytes && (s.byte(from - 1) & 0x80u)) { --from; ++steps; }
    GRK_T2P_COUNT(kT2pLoopPlt, steps);
    if (steps == kT2pPltBytes) return kT2pPltWrap;              // (a sixth byte)
    uint64_t v = 0;
    for (uint64_t k = from; k <= i; ++k) v = v << 7 | (s.byte(k) & 0x7Fu);
    if (v > 0xFFFFFFFFull) return kT2pPltWrap;
    *value = (uint32_t)v;
    return kT2pOk;
}

} // namespace grk_amd
