// grok_amd/csrc/t2_parse_layers.h -- the device Tier-2 reader's parse core for files of SEVERAL layers and of Part-1 blocks in
// several codeword segments (LAZY, TERMALL): read_packet of t2_reader.cpp restated for a packet of layer l, beside t2p_read_packet
// (t2_parse.h), with the same rules -- the source is read only at checked positions, every loop has a bound that the stream's
// content cannot raise.  For the kernels (kernels_t2read_layers.hip: KC-L, KF, KP) and a host program
// (tests/c/t2_parse_layers_units.cpp) alike.  No HIP in here.
//
// What a block carries from layer to layer lives in a scratch of one T2pRowState per row, zeroed before the row's first packet.
// A contribution is logged through the sink as records that name their row and their ordinal within it, so that what places them
// (KP) does not depend on the order in which the chains ran:
//   sink.seg(row, ordinal, len, passes, opens)   `len` bytes and `passes` passes for the row's codeword segment `ordinal`; opens:
//                                                the record starts that segment, else it adds to it
//   sink.piece(row, ordinal, rel, len, before)   the row's piece `ordinal` (len > 0 only): its bytes start `rel` behind the end of
//                                                the packet's header; `before`: the row's bytes in earlier pieces
#pragma once
#include "../../include/grok_amd.h"     // grk_amd_coded_block
#include "t2_parse.h"

namespace grk_amd {

constexpr uint32_t kT2pMaxLayers = 65535;   // what COD can declare: the inclusion tree's threshold, steps per node
constexpr uint32_t kT2pStateWords = 8;
enum T2pLayerLoop : int { kT2pLoopInclusion = 0, kT2pLoopSegments = 1, kT2pLayerLoops = 2 };
#ifndef GRK_T2P_COUNT_L
#define GRK_T2P_COUNT_L(id, n) ((void)0)
#endif

// one row's state, eight 32-bit words (all zero: not included yet, Lblock 3)
struct T2pRowState {
    uint32_t src_lo, src_hi;    // where the first piece lies (KC-L sets it once the header's end is known)
    uint32_t total;             // bytes so far
    uint32_t pieces;            // non-empty contributions so far
    uint32_t nsegs;             // codeword segments opened so far
    uint32_t passes_idx;        // passes so far | index of the open segment's capacity << 16
    uint32_t bits;              // Lblock - 3 | included << 8 | zero bit-planes << 16 | the open segment's fill << 24
    uint32_t kbits;             // Part-1: the band's expn + guard bits - 1 (for KF's bit-plane check)
};
static_assert(sizeof(T2pRowState) == 4 * kT2pStateWords, "eight words");

// A bit of the `sty` argument above COD's code-block style bits: the HT blocks' refinement passes are read (T.814 over B.10.7.2).  An HT
// block's passes are one HT set -- Cleanup, SigProp, MagRef, numbered across the layers --, the cleanup pass a codeword segment of its
// own, SigProp and MagRef the next one's: LAZY's alternation without its first segment of 10.  More than three passes are placeholder
// passes or a second HT set, whose lengths no encoder or decoder at hand shows how to read: refused (kT2pHtSet), as every pass
// beyond the first is without the bit (kT2pHtPasses).
constexpr uint32_t kT2pStyHtRefine = 0x100u;
constexpr uint32_t kT2pHtSetPasses = 3;
GRK_T2_FN uint32_t t2p_ht_seg_capacity(uint32_t sty, uint32_t idx) { return (sty & kT2pStyHtRefine) && (idx & 1u) ? 2u : 1u; }
// kT2pOk, or why an HT block that has `before` passes does not take np more
GRK_T2_FN uint32_t t2p_ht_passes_why(uint32_t sty, uint32_t before, uint32_t np)
{
    if (sty & kT2pStyHtRefine) return before + np > kT2pHtSetPasses ? (uint32_t)kT2pHtSet : (uint32_t)kT2pOk;
    return np != 1 || before != 0 ? (uint32_t)kT2pHtPasses : (uint32_t)kT2pOk;
}

// passes a codeword segment holds (B.10.7.2): TERMALL 1; LAZY 10, then 2 and 1 in turn; else all of them
GRK_T2_FN uint32_t t2p_seg_capacity(uint32_t sty, uint32_t idx)
{
    if (sty & 0x04u) return 1;
    if (sty & 0x01u) return idx == 0 ? 10u : (idx & 1u) ? 2u : 1u;
    return 0xFFFFu;
}
// the most segment records and piece records one row can give in a file of `layers` layers: a record carries at least one pass
// and a row has 164 at most; a row opens at most t2p_max_segments() segments and every contribution continues one more at most
GRK_T2_FN uint32_t t2p_max_segments(bool ht, uint32_t sty)
{
    if (ht) return (sty & kT2pStyHtRefine) ? 2u : 1u;
    if (sty & 0x04u) return kT2pMaxPasses;
    if (sty & 0x01u) return 1 + 2 * ((kT2pMaxPasses - 10) / 3) + ((kT2pMaxPasses - 10) % 3 ? 1 : 0);         // 10, then 2 and 1 in turn: 104
    return 1;
}
GRK_T2_FN uint32_t t2p_max_piece_records(bool ht, uint32_t layers) { return ht ? 1u : layers < kT2pMaxPasses ? layers : kT2pMaxPasses; }
// ... with the style word's say: an HT block read with its refinement passes contributes in three layers at most
GRK_T2_FN uint32_t t2p_max_piece_records_sty(bool ht, uint32_t sty, uint32_t layers)
{
    if (ht && (sty & kT2pStyHtRefine)) return layers < kT2pHtSetPasses ? layers : kT2pHtSetPasses;
    return t2p_max_piece_records(ht, layers);
}
GRK_T2_FN uint32_t t2p_max_seg_records(bool ht, uint32_t sty, uint32_t layers)
{
    const uint64_t n = (uint64_t)t2p_max_segments(ht, sty) + t2p_max_piece_records_sty(ht, sty, layers) - 1;
    return n < kT2pMaxPasses ? (uint32_t)n : kT2pMaxPasses;
}

// the tag tree with 32-bit nodes (a bound below the threshold, which is a layer count here: 65535 at most)
template <class Src>
GRK_T2_FN uint32_t t2p_tree_decode32(uint32_t* nodes, uint32_t gw, uint32_t gh, uint32_t nlev, uint32_t total, uint32_t x, uint32_t y,
                                     uint32_t threshold, uint32_t max_steps, T2pBits<Src>& br, bool& known)
{
    uint32_t low = 0;
    uint32_t off = total;
    GRK_T2P_COUNT(kT2pLoopLevels, nlev);
    for (uint32_t i = 0; i < nlev && i < kT2pMaxLevels; ++i) {
        const uint32_t lv = nlev - 1 - i;
        const uint32_t w = t2p_level_dim(gw, lv), h = t2p_level_dim(gh, lv);
        off -= w * h;
        uint32_t* const nd = nodes + off + (y >> lv) * w + (x >> lv);
        const uint32_t cell = GRK_T2P_UNIFORM(*nd);
        uint32_t v = cell >> 1;
        bool k = (cell & 1u) != 0;
        if (v < low) v = low;
        uint32_t steps = 0;
        while (!k && v < threshold && steps < max_steps) { if (br.bit()) k = true; else ++v; ++steps; }
        if (max_steps == kT2pThreshold) GRK_T2P_COUNT(kT2pLoopTree, steps); else GRK_T2P_COUNT_L(kT2pLoopInclusion, steps);
        *nd = v << 1 | (k ? 1u : 0u);
        low = v;
        known = k;
    }
    return low;
}

// ---- one packet header of layer `layer` ---------------------------------------------------------------------------------------------
// The packet `q` (the tile's packet `number` in file order) from pos (advanced to behind the packet's bodies) and not beyond `end`.
// nodes: the tile's node scratch in 32-bit nodes (q's node_at counts nodes here); state: the tile's rows' state.  *body_at: the end
// of the header (and of EPH): a piece's source is *body_at + rel.  sty: the code-block style (Part-1), kT2pStyHtRefine (HT).
template <class Src, class Sink>
GRK_T2_FN uint32_t t2p_read_packet_layer(Src& src, const T2ReadPacket& q, uint32_t* nodes, T2pRowState* state, bool ht, uint32_t sty, bool sop, bool eph,
                                         uint32_t layer, uint32_t number, uint64_t& pos, uint64_t end, Sink& sink, uint64_t* body_at)
{
    if (pos > end) return kT2pBodyPast;
    if (sop) {
        if (end - pos < 6 || t2p_u16(src, pos) != 0xFF91 || t2p_u16(src, pos + 2) != 4 || t2p_u16(src, pos + 4) != (number & 0xFFFFu)) return kT2pNoSop;
        pos += 6;
    }
    T2pBits<Src> br(src, pos, end);
    uint64_t sum = 0;
    if (br.bit()) {
        for (uint32_t bi = 0; bi < q.nbands && bi < 3; ++bi) {
            const T2ReadBand& B = q.band[bi];
            uint32_t* const incl = nodes + B.node_at;
            uint32_t* const zbpt = incl + B.nodes;
            uint32_t row = B.first_row;
            for (uint32_t y = 0; y < B.gh; ++y)
                for (uint32_t x = 0; x < B.gw; ++x, ++row) {
                    uint32_t* const sw = (uint32_t*)(state + row);
                    uint32_t total = GRK_T2P_UNIFORM(sw[2]), pieces = GRK_T2P_UNIFORM(sw[3]), nsegs = GRK_T2P_UNIFORM(sw[4]);
                    const uint32_t pi = GRK_T2P_UNIFORM(sw[5]), bits = GRK_T2P_UNIFORM(sw[6]);
                    uint32_t passes = pi & 0xFFFFu, seg_idx = pi >> 16;
                    uint32_t lb = 3 + (bits & 0xFFu), zbp = (bits >> 16) & 0xFFu, seg_fill = bits >> 24;
                    bool known = false;
                    if (!((bits >> 8) & 1u)) {
                        const uint32_t v = t2p_tree_decode32(incl, B.gw, B.gh, B.nlev, B.nodes, x, y, layer + 1, kT2pMaxLayers, br, known);
                        if (!known || v > layer) continue;
                        zbp = t2p_tree_decode32(zbpt, B.gw, B.gh, B.nlev, B.nodes, x, y, kT2pThreshold, kT2pThreshold, br, known);
                        if (!known || br.err) return kT2pZeroPlanes;
                    } else if (!br.bit()) continue;
                    uint32_t np;                                       // Table B.4
                    if (!br.bit()) np = 1;
                    else if (!br.bit()) np = 2;
                    else {
                        uint32_t t = br.bits(2);
                        if (t < 3) np = 3 + t;
                        else { t = br.bits(5); np = t < 31 ? 6 + t : 37 + br.bits(7); }
                    }
                    GRK_T2P_COUNT(kT2pLoopPasses, np);
                    if (ht) { const uint32_t hw = t2p_ht_passes_why(sty, passes, np); if (hw) return hw; }
                    if (passes + np > kT2pMaxPasses) return kT2pPasses;
                    while (br.bit()) if (++lb > kT2pMaxLblock) return kT2pLblock;
                    GRK_T2P_COUNT(kT2pLoopLblock, lb);
                    uint64_t got = 0;
                    uint32_t left = np, turns = 0;
                    // (a turn takes at least one pass)
                    for (; left && turns < kT2pMaxPasses; ++turns) {
                        const uint32_t cap = ht ? t2p_ht_seg_capacity(sty, seg_idx) : t2p_seg_capacity(sty, seg_idx);
                        const uint32_t room = cap - seg_fill, k = left < room ? left : room;
                        const uint32_t nb = lb + t2p_floor_log2(k);
                        if (nb > kT2pMaxLenBits) return kT2pLenBits;
                        const uint32_t len = br.bits(nb);
                        if (seg_fill == 0) { sink.seg(row, nsegs, len, k, true); ++nsegs; }
                        else sink.seg(row, nsegs - 1, len, k, false);
                        seg_fill += k;
                        if (seg_fill == cap) { seg_idx = (seg_idx + 1) & 0xFFFFu; seg_fill = 0; }
                        left -= k; got += len;
                        // (a segment's length is a sum over the block's contributions: below the block's total, checked next)
                        if (got + total > 0xFFFFFFFFull) return kT2pBlockWrap;
                    }
                    GRK_T2P_COUNT_L(kT2pLoopSegments, turns);
                    passes += np;
                    if (got) { sink.piece(row, pieces, sum, (uint32_t)got, total); ++pieces; total += (uint32_t)got; sum += got; }
                    sw[2] = total; sw[3] = pieces; sw[4] = nsegs; sw[5] = passes | seg_idx << 16;
                    sw[6] = (lb - 3) | 1u << 8 | zbp << 16 | seg_fill << 24; sw[7] = B.kbits;
                }
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

// ---- what KF makes of a row's state ---------------------------------------------------------------------------------------------------
// The row as read_tile leaves it (its offset: the first piece's source; a row of several pieces gets its place in the appendix from
// the caller).  false: a Part-1 block whose passes its bit-planes cannot hold
GRK_T2_FN bool t2p_finish_row(const T2pRowState& s, bool ht, grk_amd_coded_block* row)
{
    row->offset = s.pieces ? ((uint64_t)s.src_hi << 32 | s.src_lo) : 0;
    row->length = s.total;
    row->missing_msbs = 0;
    const uint32_t zbp = (s.bits >> 16) & 0xFFu, passes = s.passes_idx & 0xFFFFu;
    if (ht) { row->missing_msbs = zbp; return true; }
    if (!s.total) return true;
    const int numbps = (int)s.kbits - (int)zbp;
    if (numbps < 1 || (int)passes > 3 * numbps - 2) return false;
    row->missing_msbs = (uint32_t)numbps | passes << 8;
    return true;
}

// the numbering of precinct i's packet of layer l in the tile-part (np precincts, L layers; RLCP: the precinct's resolution run)
GRK_T2_FN uint64_t t2p_packet_number(uint32_t order, uint64_t np, uint64_t L, uint64_t i, uint64_t l, uint32_t run_first, uint32_t run_count)
{
    if (order == 0) return l * np + i;
    if (order == 1) return (uint64_t)run_first * L + l * run_count + (i - run_first);
    return i * L + l;
}

// A tile's packets in file order: fn(i, l, k) for precinct i, layer l, number k, until it returns false.  run(i): precinct i's
// resolution run as {first, count} (RLCP alone asks)
template <class Run, class Fn> GRK_T2_FN void t2p_tile_packets(uint32_t order, uint32_t np, uint32_t L, Run run, Fn fn)
{
    uint32_t k = 0;
    if (order == 0) {
        for (uint32_t l = 0; l < L; ++l) for (uint32_t i = 0; i < np; ++i, ++k) if (!fn(i, l, k)) return;
    } else if (order == 1) {
        for (uint32_t i = 0; i < np;) {
            uint32_t first = 0, count = 1;
            run(i, &first, &count);
            if (!count) count = 1;
            for (uint32_t l = 0; l < L; ++l) for (uint32_t j = i; j < i + count && j < np; ++j, ++k) if (!fn(j, l, k)) return;
            i += count;
        }
    } else {
        for (uint32_t i = 0; i < np; ++i) for (uint32_t l = 0; l < L; ++l, ++k) if (!fn(i, l, k)) return;
    }
}

// ---- a tile divided into tile-parts -----------------------------------------------------------------------------------------------------
// The tile's packet sequence is its tile-parts' bodies end to end, each body whole packets.  What KL-P and KH-P leave about the
// tile's n tile-parts in TPsot order (they rise in the file): where each lies, its body, whether it carries PLT, how many packets
// that lists and where those entries start among the tile's PLT lengths.
struct T2pParts {
    const unsigned long long* at; const uint32_t* len; const unsigned long long* body;
    const uint32_t* has_plt; const uint32_t* npk; const uint32_t* first;
    uint32_t n;
};
GRK_T2_FN uint64_t t2p_load64(const unsigned long long* p)
{
    const uint32_t* const w = (const uint32_t*)p;
    return (uint64_t)GRK_T2P_UNIFORM(w[0]) | (uint64_t)GRK_T2P_UNIFORM(w[1]) << 32;
}
GRK_T2_FN uint64_t t2p_part_end(const T2pParts& P, uint32_t p) { return t2p_load64(P.at + p) + GRK_T2P_UNIFORM(P.len[p]); }
// the tile-part a position lies in: the last that starts at or before it (at most 8 steps for 255 tile-parts)
GRK_T2_FN uint32_t t2p_part_of(const T2pParts& P, uint64_t pos)
{
    uint32_t lo = 0, hi = P.n;
    for (uint32_t step = 0; step < 9 && hi - lo > 1; ++step) { const uint32_t mid = (lo + hi) >> 1; if (t2p_load64(P.at + mid) <= pos) lo = mid; else hi = mid; }
    return lo;
}
// a chain that reads the tile in file order: the tile-part at hand, packets read in it, its end
struct T2pPartWalk { uint32_t p, used; uint64_t end; };
GRK_T2_FN void t2p_part_walk_start(const T2pParts& P, T2pPartWalk& w, uint64_t& pos) { w.p = 0; w.used = 0; w.end = t2p_part_end(P, 0); pos = t2p_load64(P.body); }
// leaving a tile-part: its PLT, if it has one, listed just the packets read in it
GRK_T2_FN uint32_t t2p_part_leave(const T2pParts& P, const T2pPartWalk& w)
{
    return GRK_T2P_UNIFORM(P.has_plt[w.p]) && w.used != GRK_T2P_UNIFORM(P.npk[w.p]) ? (uint32_t)kT2pPartPlt : (uint32_t)kT2pOk;
}
// before a packet: on to the next tile-part that holds a byte when pos has reached the end of the one at hand
GRK_T2_FN uint32_t t2p_part_step(const T2pParts& P, T2pPartWalk& w, uint64_t& pos)
{
    for (uint32_t hop = 0; hop < P.n && pos == w.end; ++hop) {
        const uint32_t why = t2p_part_leave(P, w);
        if (why) return why;
        if (w.p + 1 >= P.n) return kT2pTileEnds;
        ++w.p; w.used = 0;
        pos = t2p_load64(P.body + w.p); w.end = t2p_part_end(P, w.p);
    }
    return kT2pOk;
}
// behind a packet of `size` bytes: the tile-part's PLT entry for it (plt_len: the tile's PLT lengths)
GRK_T2_FN uint32_t t2p_part_packet(const T2pParts& P, T2pPartWalk& w, const uint32_t* plt_len, uint64_t size)
{
    if (GRK_T2P_UNIFORM(P.has_plt[w.p])) {
        if (w.used >= GRK_T2P_UNIFORM(P.npk[w.p])) return kT2pPartPlt;
        if (size != GRK_T2P_UNIFORM(plt_len[GRK_T2P_UNIFORM(P.first[w.p]) + w.used])) return kT2pPltSize;
    }
    ++w.used;
    return kT2pOk;
}
// behind the tile's last packet: it ends its tile-part, and what follows of the tile holds nothing
GRK_T2_FN uint32_t t2p_part_finish(const T2pParts& P, T2pPartWalk& w, uint64_t pos)
{
    for (uint32_t hop = 0; hop < P.n; ++hop) {
        if (pos != w.end) return kT2pTail;
        const uint32_t why = t2p_part_leave(P, w);
        if (why) return why;
        if (w.p + 1 >= P.n) return kT2pOk;
        ++w.p; w.used = 0;
        pos = t2p_load64(P.body + w.p); w.end = t2p_part_end(P, w.p);
    }
    return kT2pOk;
}

} // namespace grk_amd
