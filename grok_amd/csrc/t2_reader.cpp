// grok_amd/csrc/t2_reader.cpp -- the Tier-2 READER: a codestream's main header and every packet header of every tile, host only
// (no HIP call).  The other side of t2_writer.cpp: what SIZ / COD / QCD say, and per code-block where its bytes lie in the file,
// how many coding passes and zero bit-planes it has and how its bytes divide into codeword segments -- the table
// grk_amd_decode_tiles takes (the reference: CodeStreamDecompress::readHeader, T2Decompress::decompressPacket).
// Written from ITU-T T.800 Annex A (marker segments), Annex B (B.10 packet headers, B.10.2 tag trees, B.10.7 lengths, B.12
// progression) and T.814 (the HT code-block style bit), as tests/j2kparse.py was.
//
// A tile may be divided into tile-parts (read_stream_packets with allow_parts, grk_amd_read_packets_parts): its packet sequence is
// its tile-parts' bodies end to end, each body whole packets, so only where a tile's bytes lie changes.
//
// This is a parser of UNTRUSTED input: every read is checked against the end of its container (the codestream, the marker
// segment, the tile-part, with PLT the packet), every count against what the bytes present could hold, sums are made in 64 bits.
#include "t2_reader.h"
#include "geometry.h"
#include "image.h"
#include "t2_order.h"
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <mutex>

using namespace grk_amd;

namespace {

int refuse(std::string& err, int code, const char* fmt, ...)
{
    char buf[256];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    err = buf;
    return code;
}

// the codestream: has(at, k) before any of the unchecked big-endian reads
struct Bytes {
    const uint8_t* d; uint64_t n;
    bool has(uint64_t at, uint64_t k) const { return at <= n && k <= n - at; }
    uint32_t u8(uint64_t i) const { return d[i]; }
    uint32_t u16(uint64_t i) const { return (uint32_t)d[i] << 8 | d[i + 1]; }
    uint32_t u32(uint64_t i) const { return (uint32_t)d[i] << 24 | (uint32_t)d[i + 1] << 16 | (uint32_t)d[i + 2] << 8 | d[i + 3]; }
};

const char* marker_name(uint32_t m)
{
    switch (m) {
    case 0xFF53: return "COC"; case 0xFF5D: return "QCC"; case 0xFF5E: return "RGN"; case 0xFF5F: return "POC";
    case 0xFF60: return "PPM"; case 0xFF61: return "PPT"; case 0xFF57: return "PLM"; case 0xFF52: return "COD"; case 0xFF5C: return "QCD";
    case 0xFF74: return "MCT"; case 0xFF75: return "MCC"; case 0xFF77: return "MCO"; case 0xFF78: return "CBD"; case 0xFF76: return "NLT";
    default: return nullptr;
    }
}

// blocks and precincts an image may have before this reader declines it: a stream of a few bytes can declare any size (a block
// that is not included costs no bit), and the tables are sized by the declaration
constexpr uint64_t kMaxBlocksGuess = 1ull << 23;

int parse_main_header(const Bytes& b, grk_amd_stream_info& info, uint64_t& sot_at, std::string& err)
{
    std::memset(&info, 0, sizeof info);
    if (!b.has(0, 4) || b.u16(0) != 0xFF4F) return refuse(err, GRK_AMD_ERR_INVALID, "no SOC marker");
    uint64_t at = 2;
    bool siz = false, cod = false, qcd = false;
    uint32_t xf = 0, sty = 0;
    for (;;) {
        if (!b.has(at, 4)) return refuse(err, GRK_AMD_ERR_INVALID, "the main header does not end in a tile-part");
        const uint32_t m = b.u16(at);
        if (m == 0xFF90) break;
        const uint32_t l = b.u16(at + 2);
        if (m < 0xFF30 || l < 2 || !b.has(at + 2, l)) return refuse(err, GRK_AMD_ERR_INVALID, "broken marker segment 0x%04X at %llu", m, (unsigned long long)at);
        const uint64_t body = at + 4;
        const uint32_t bl = l - 2;
        if (!siz && m != 0xFF51) return refuse(err, GRK_AMD_ERR_INVALID, "SIZ is not the first marker segment");
        if (m == 0xFF51) {
            if (siz || bl < 39) return refuse(err, GRK_AMD_ERR_INVALID, "broken SIZ");
            siz = true;
            const uint32_t nc = b.u16(body + 34);
            if (nc == 0 || nc > 16384 || bl != 36 + 3 * nc) return refuse(err, GRK_AMD_ERR_INVALID, "SIZ: Lsiz does not fit Csiz = %u", nc);
            if (nc > 4) return refuse(err, GRK_AMD_ERR_UNSUPPORTED, "%u components (at most 4)", nc);
            info.layout = grk_amd_image_layout{b.u32(body + 10), b.u32(body + 14), b.u32(body + 2), b.u32(body + 6),
                                               b.u32(body + 26), b.u32(body + 30), b.u32(body + 18), b.u32(body + 22)};
            info.base.num_comps = (uint16_t)nc;
            for (uint32_t c = 0; c < nc; ++c) {
                const uint32_t ssiz = b.u8(body + 36 + 3 * c), dx = b.u8(body + 37 + 3 * c), dy = b.u8(body + 38 + 3 * c);
                if (!dx || !dy) return refuse(err, GRK_AMD_ERR_INVALID, "SIZ: component %u with XRsiz / YRsiz 0", c);
                if (c && ssiz != b.u8(body + 36)) return refuse(err, GRK_AMD_ERR_UNSUPPORTED, "components of differing precision or sign");
                if ((ssiz & 0x7F) + 1 > 38) return refuse(err, GRK_AMD_ERR_INVALID, "SIZ: precision %u", (ssiz & 0x7F) + 1);
                if ((ssiz & 0x7F) + 1 > 16) return refuse(err, GRK_AMD_ERR_UNSUPPORTED, "precision %u (at most 16)", (ssiz & 0x7F) + 1);
                info.base.prec = (uint8_t)((ssiz & 0x7F) + 1); info.base.sgnd = (uint8_t)(ssiz >> 7);
                info.comp_dx[c] = (uint8_t)dx; info.comp_dy[c] = (uint8_t)dy;
            }
        } else if (m == 0xFF52) {
            if (cod || bl < 10) return refuse(err, GRK_AMD_ERR_INVALID, "broken COD");
            cod = true;
            const uint32_t scod = b.u8(body), prog = b.u8(body + 1), layers = b.u16(body + 2), mct = b.u8(body + 4), levels = b.u8(body + 5);
            const uint32_t cbw = b.u8(body + 6) + 2, cbh = b.u8(body + 7) + 2;
            sty = b.u8(body + 8); xf = b.u8(body + 9);
            if (scod & ~7u) return refuse(err, GRK_AMD_ERR_UNSUPPORTED, "COD: Scod = 0x%02X", scod);
            if (prog > 4 || layers == 0 || levels > 32 || cbw > 10 || cbh > 10 || cbw + cbh > 12)
                return refuse(err, GRK_AMD_ERR_INVALID, "COD: progression %u, %u layers, %u levels, code-blocks 2^%u x 2^%u", prog, layers, levels, cbw, cbh);
            if (mct > 1) return refuse(err, GRK_AMD_ERR_UNSUPPORTED, "a custom MCT (COD: multiple component transformation %u)", mct);
            if (levels > GRK_AMD_MAX_LEVELS) return refuse(err, GRK_AMD_ERR_UNSUPPORTED, "%u decomposition levels (at most %d)", levels, GRK_AMD_MAX_LEVELS);
            if (cbw > 6 || cbh > 6) return refuse(err, GRK_AMD_ERR_UNSUPPORTED, "code-blocks of 2^%u x 2^%u (at most 2^6)", cbw, cbh);
            if (xf > 1) return refuse(err, GRK_AMD_ERR_UNSUPPORTED, "COD: wavelet transformation %u", xf);
            if (sty & 0x80) return refuse(err, GRK_AMD_ERR_UNSUPPORTED, "HT and Part-1 code-blocks mixed (code-block style 0x%02X)", sty);
            if (bl != 10 + ((scod & 1) ? levels + 1 : 0)) return refuse(err, GRK_AMD_ERR_INVALID, "COD: Lcod does not fit %u levels", levels);
            info.flags |= ((scod & 2) ? GRK_AMD_CS_SOP : 0u) | ((scod & 4) ? GRK_AMD_CS_EPH : 0u) | GRK_AMD_CS_PROG(prog);
            info.num_layers = (uint16_t)layers;
            info.base.mct = (uint8_t)mct; info.base.num_levels = (uint8_t)levels;
            info.base.cblk_w_exp = (uint8_t)cbw; info.base.cblk_h_exp = (uint8_t)cbh;
            info.base.irreversible = xf == 0;
            if (!(sty & 0x40)) { info.base.reserved[0] = 1; info.base.reserved[1] = (uint8_t)(sty & 0x3F); }
            for (uint32_t r = 0; (scod & 1) && r <= levels; ++r) {
                const uint32_t pe = b.u8(body + 10 + r);
                if (r && (!(pe & 15u) || !(pe >> 4))) return refuse(err, GRK_AMD_ERR_INVALID, "COD: precinct exponent 0 at resolution %u", r);
                if (!pe) return refuse(err, GRK_AMD_ERR_UNSUPPORTED, "precincts of 1 x 1 at resolution 0");
                info.base.precinct_exp[r] = pe == 0xFF ? 0 : (uint8_t)pe;
            }
        } else if (m == 0xFF5C) {
            if (qcd || bl < 2) return refuse(err, GRK_AMD_ERR_INVALID, "broken QCD");
            qcd = true;
            const uint32_t sq = b.u8(body);
            info.guard_bits = (uint8_t)(sq >> 5); info.qstyle = (uint8_t)(sq & 31u);
            if (info.qstyle == 1) return refuse(err, GRK_AMD_ERR_UNSUPPORTED, "Sqcd style 1 (scalar derived quantisation)");
            if (info.qstyle != 0 && info.qstyle != 2) return refuse(err, GRK_AMD_ERR_INVALID, "QCD: Sqcd = 0x%02X", sq);
            const uint32_t each = info.qstyle ? 2u : 1u, n = (bl - 1) / each;
            if ((bl - 1) % each || n > 3 * 32 + 1) return refuse(err, GRK_AMD_ERR_INVALID, "QCD: Lqcd = %u", l);
            info.num_qcd = std::min<uint32_t>(n, 3 * GRK_AMD_MAX_LEVELS + 1);
            for (uint32_t i = 0; i < info.num_qcd; ++i) info.qcd_words[i] = (uint16_t)(each == 2 ? b.u16(body + 1 + 2 * i) : b.u8(body + 1 + i));
        } else if (m == 0xFF55) {
            info.flags |= GRK_AMD_CS_TLM;
        } else if (m == 0xFF50 || m == 0xFF64 || m == 0xFF63) {
            // CAP, COM, CRG: nothing this reader needs
        } else if (const char* name = marker_name(m)) {
            return refuse(err, GRK_AMD_ERR_UNSUPPORTED, "%s marker segment in the main header", name);
        } else {
            return refuse(err, GRK_AMD_ERR_UNSUPPORTED, "marker segment 0x%04X in the main header", m);
        }
        at += 2 + (uint64_t)l;
    }
    if (!siz || !cod || !qcd) return refuse(err, GRK_AMD_ERR_INVALID, "main header without %s", !siz ? "SIZ" : !cod ? "COD" : "QCD");
    if (info.num_qcd < 3u * info.base.num_levels + 1u)
        return refuse(err, GRK_AMD_ERR_INVALID, "QCD: %u sub-bands for %u levels", info.num_qcd, info.base.num_levels);
    info.num_qcd = 3u * info.base.num_levels + 1u;
    if (info.base.irreversible != (info.qstyle == 2))
        return refuse(err, GRK_AMD_ERR_UNSUPPORTED, "Sqcd style %u with the %s transformation", info.qstyle, info.base.irreversible ? "9/7" : "5/3");
    if (info.base.mct && info.base.num_comps < 3) return refuse(err, GRK_AMD_ERR_INVALID, "COD: component transformation over %u components", info.base.num_comps);
    sot_at = at;
    return GRK_AMD_OK;
}

// ---- packet headers ---------------------------------------------------------------------------------------------------------
// MSB first, a byte that follows 0xFF carries 7 bits (B.10.1).  Past `end` every bit reads as 0 and `err` stays set: the loops
// below all end on zeros.
struct Bits {
    const uint8_t* d; uint64_t pos, end; uint32_t cur = 0; int n = 0; bool err = false;
    uint32_t bit()
    {
        if (!n) {
            if (pos >= end) { err = true; return 0; }
            const bool ff = cur == 0xFF;
            cur = d[pos++];
            n = ff ? 7 : 8;
        }
        --n;
        return (cur >> n) & 1u;
    }
    uint32_t bits(uint32_t k) { uint32_t v = 0; while (k--) v = (v << 1) | bit(); return v; }       // k <= 32
    uint64_t align()                        // a header that ends on 0xFF is followed by a stuffed byte
    {
        if (cur == 0xFF) { if (pos >= end) err = true; else ++pos; }
        n = 0; cur = 0;
        return pos;
    }
};

// Tag tree (B.10.2) in its general form: per node the lower bound so far << 1 | "value known".
struct TreeDim { uint32_t nlev = 0; uint32_t w[17], off[17]; uint32_t nodes = 0; };
TreeDim tree_dim(uint32_t w, uint32_t h)
{
    TreeDim d;
    for (;;) {
        d.w[d.nlev] = w; d.off[d.nlev] = d.nodes; d.nodes += w * h; ++d.nlev;
        if ((w == 1 && h == 1) || d.nlev == 17) break;
        w = (w + 1) >> 1; h = (h + 1) >> 1;
    }
    return d;
}
inline uint32_t tree_decode(uint32_t* nodes, const TreeDim& d, uint32_t x, uint32_t y, uint32_t threshold, Bits& br, bool& known)
{
    uint32_t low = 0;
    for (int lv = (int)d.nlev - 1; lv >= 0; --lv) {
        uint32_t& nd = nodes[d.off[lv] + (y >> lv) * d.w[lv] + (x >> lv)];
        uint32_t v = nd >> 1;
        bool k = (nd & 1u) != 0;
        if (v < low) v = low;
        while (!k && v < threshold) { if (br.bit()) k = true; else ++v; }
        nd = v << 1 | (k ? 1u : 0u);
        low = v;
        known = k;
    }
    return low;
}

struct BlockState {
    uint64_t src0 = 0;              // where the first piece lies
    uint32_t total = 0;             // bytes so far
    uint32_t pieces = 0;            // non-empty contributions (one per layer at most)
    uint32_t last_seg = 0;          // the open codeword segment's record in its precinct's list
    uint16_t passes = 0, seg_idx = 0;
    uint8_t  lblock = 3, included = 0, zbp = 0, seg_fill = 0;
    uint8_t  dropped = 0;           // of a resolution the caller's reduced decode drops
};
struct SegRec { uint32_t row, len, passes; };
struct Piece { uint64_t src; uint32_t row, len; };
// what one precinct's packets leave behind (a block lies in one precinct: its records are all in one of these, in order)
struct Precinct {
    bool ready = false;
    TreeDim dim[3];
    std::vector<uint32_t> nodes;            // per band: inclusion tree, zero-bit-plane tree
    uint32_t at[3][2];
    std::vector<SegRec> segs;
    std::vector<Piece> pieces;
};

struct TileCtx {
    Bytes b;
    const grk_amd_stream_info* info;
    std::vector<TileGeom> geoms;    // the tile-components' geometries: one, or one per kind of sub-sampling factors
    std::vector<const TileGeom*> cg;    // [component]: its geometry ...
    std::vector<uint64_t> row0;         // ... and the first of its rows among the tile's
    uint32_t tile;
    bool ht, sop, eph;
    bool ht_refine;                 // an HT block's refinement passes are read (grk_amd_read_packets_refine)
    std::atomic<bool>* met_ht_second_pass;      // told of the refusal below
    uint32_t sty;
    BlockState* st;                 // the tile's rows
    std::vector<Pk> seq;            // one layer's packets in order
    std::vector<Precinct> prec;     // [seq index]
};

// passes a codeword segment holds (B.10.7.2; T2Decompress.cpp:169-186): TERMALL 1; LAZY 10, then 2 (raw pair) and 1 (cleanup)
// in turn; else all of them
inline uint32_t seg_capacity(uint32_t sty, uint32_t idx)
{
    if (sty & 0x04) return 1;
    if (sty & 0x01) return idx == 0 ? 10u : (idx & 1u) ? 2u : 1u;
    return 0xFFFFu;
}
// ... of an HT block read with its refinement passes (T.814): its passes are one HT set -- Cleanup, SigProp, MagRef, numbered across
// the layers --, the cleanup pass a codeword segment of its own, SigProp and MagRef the next one's
inline uint32_t ht_seg_capacity(bool refine, uint32_t idx) { return refine && (idx & 1u) ? 2u : 1u; }
inline uint32_t floor_log2(uint32_t v) { uint32_t r = 0; while (v >>= 1) ++r; return r; }

// One packet: seq[i] in layer `layer`, the tile's packet number `number`, from pos (advanced) and not beyond `end`.
int read_packet(TileCtx& T, uint32_t i, uint32_t layer, uint32_t number, uint64_t& pos, uint64_t end, std::string& err)
{
    const Pk& q = T.seq[i];
    const ResGeom& R = T.cg[q.c]->res[q.r];
    Precinct& P = T.prec[i];
    if (!P.ready) {
        uint32_t n = 0;
        for (uint32_t bi = 0; bi < R.num_bands; ++bi) {
            const BandGeom::Prec& G = R.band[bi].prec[q.pi];
            if (!G.gw || !G.gh) continue;
            P.dim[bi] = tree_dim(G.gw, G.gh);
            P.at[bi][0] = n; n += P.dim[bi].nodes;
            P.at[bi][1] = n; n += P.dim[bi].nodes;
        }
        P.nodes.assign(n, 0);
        P.ready = true;
    }
    if (T.sop) {
        if (end - pos < 6 || T.b.u16(pos) != 0xFF91 || T.b.u16(pos + 2) != 4 || T.b.u16(pos + 4) != (number & 0xFFFFu))
            return refuse(err, GRK_AMD_ERR_INVALID, "tile %u packet %u: no SOP marker segment with that number", T.tile, number);
        pos += 6;
    }
    struct Todo { uint32_t row, len; };
    static thread_local std::vector<Todo> todo;
    todo.clear();
    Bits br{T.b.d, pos, end};
    if (br.bit()) {
        const uint32_t row0 = (uint32_t)T.row0[q.c];
        for (uint32_t bi = 0; bi < R.num_bands; ++bi) {
            const BandGeom::Prec& G = R.band[bi].prec[q.pi];
            if (!G.gw || !G.gh) continue;
            uint32_t* const incl = P.nodes.data() + P.at[bi][0];
            uint32_t* const zbpt = P.nodes.data() + P.at[bi][1];
            const TreeDim& D = P.dim[bi];
            uint32_t row = row0 + G.first_block;
            for (uint32_t y = 0; y < G.gh; ++y)
                for (uint32_t x = 0; x < G.gw; ++x, ++row) {
                    BlockState& s = T.st[row];
                    bool known = false;
                    if (!s.included) {
                        const uint32_t v = tree_decode(incl, D, x, y, layer + 1, br, known);
                        if (!known || v > layer) continue;
                        // (B.10.5 raises the threshold one by one until the value is known; a node reads bits only once its
                        //  parent is known, so one walk with a threshold beyond any bit-plane count reads the same bits in the same order)
                        const uint32_t z = tree_decode(zbpt, D, x, y, 65, br, known);
                        if (!known || br.err) return refuse(err, GRK_AMD_ERR_INVALID, "tile %u packet %u: zero bit-planes without end", T.tile, number);
                        s.included = 1; s.zbp = (uint8_t)z;
                    } else if (!br.bit()) continue;
                    uint32_t np;                                       // Table B.4
                    if (!br.bit()) np = 1;
                    else if (!br.bit()) np = 2;
                    else {
                        uint32_t v = br.bits(2);
                        if (v < 3) np = 3 + v;
                        else { v = br.bits(5); np = v < 31 ? 6 + v : 37 + br.bits(7); }
                    }
                    if (T.ht && !T.ht_refine && (np != 1 || s.passes)) {
                        T.met_ht_second_pass->store(true, std::memory_order_relaxed);
                        return refuse(err, GRK_AMD_ERR_UNSUPPORTED, "tile %u packet %u: an HT code-block with more than one pass", T.tile, number);
                    }
                    // (a fourth pass is a placeholder pass or a second HT set's: how their lengths are signalled nothing at hand shows)
                    if (T.ht && T.ht_refine && (uint32_t)s.passes + np > 3)
                        return refuse(err, GRK_AMD_ERR_UNSUPPORTED, "tile %u packet %u: an HT code-block with more than one pass of a kind (%u passes: placeholder passes or a second HT set)",
                                      T.tile, number, (uint32_t)s.passes + np);
                    if ((uint32_t)s.passes + np > 164) return refuse(err, GRK_AMD_ERR_INVALID, "tile %u packet %u: more than 164 coding passes", T.tile, number);
                    uint32_t lb = s.lblock;
                    while (br.bit()) if (++lb > 32) return refuse(err, GRK_AMD_ERR_INVALID, "tile %u packet %u: Lblock beyond 32", T.tile, number);
                    s.lblock = (uint8_t)lb;
                    uint64_t sum = 0;
                    for (uint32_t left = np; left;) {
                        const uint32_t cap = T.ht ? ht_seg_capacity(T.ht_refine, s.seg_idx) : seg_capacity(T.sty, s.seg_idx);
                        const uint32_t k = std::min<uint32_t>(left, cap - s.seg_fill);
                        const uint32_t nb = lb + floor_log2(k);
                        if (nb > 32) return refuse(err, GRK_AMD_ERR_INVALID, "tile %u packet %u: a length of %u bits", T.tile, number, nb);
                        const uint32_t len = br.bits(nb);
                        if (s.seg_fill == 0) { s.last_seg = (uint32_t)P.segs.size(); P.segs.push_back(SegRec{row, len, k}); }
                        else {
                            SegRec& sr = P.segs[s.last_seg];
                            if ((uint64_t)sr.len + len > 0xFFFFFFFFull) return refuse(err, GRK_AMD_ERR_INVALID, "tile %u packet %u: a segment length wraps", T.tile, number);
                            sr.len += len; sr.passes += k;
                        }
                        s.seg_fill = (uint8_t)(s.seg_fill + k);
                        if (s.seg_fill == cap) { ++s.seg_idx; s.seg_fill = 0; }
                        left -= k; sum += len;
                    }
                    s.passes = (uint16_t)(s.passes + np);
                    if (sum + s.total > 0xFFFFFFFFull) return refuse(err, GRK_AMD_ERR_INVALID, "tile %u packet %u: a block length wraps", T.tile, number);
                    todo.push_back(Todo{row, (uint32_t)sum});
                }
        }
    }
    pos = br.align();
    if (br.err) return refuse(err, GRK_AMD_ERR_INVALID, "tile %u packet %u: the header runs past its %s", T.tile, number, "container");
    if (T.eph) {
        if (end - pos < 2 || T.b.u16(pos) != 0xFF92) return refuse(err, GRK_AMD_ERR_INVALID, "tile %u packet %u: no EPH marker", T.tile, number);
        pos += 2;
    }
    for (const Todo& t : todo) {
        if (t.len > end - pos) return refuse(err, GRK_AMD_ERR_INVALID, "tile %u packet %u: the body runs past its container", T.tile, number);
        if (t.len) {
            BlockState& s = T.st[t.row];
            if (!s.pieces++) s.src0 = pos;
            s.total += t.len;
            P.pieces.push_back(Piece{pos, t.row, t.len});
            pos += t.len;
        }
    }
    return GRK_AMD_OK;
}

using TilePart = StreamPart;

inline bool subsampled(const grk_amd_stream_info& info)
{
    for (uint32_t c = 0; c < info.base.num_comps && c < 4; ++c) if (info.comp_dx[c] != 1 || info.comp_dy[c] != 1) return true;
    return false;
}
// component c of tile t as a tile of one component: its rectangle in the component's own samples (grk_amd_layout_tile_comp)
int tile_comp_params(const grk_amd_stream_info& info, uint32_t t, uint32_t c, grk_amd_tile_params& p)
{
    const int rc = grk_amd_layout_tile_comp(&info.layout, &info.base, info.comp_dx[c], info.comp_dy[c], t, &p);
    p.num_comps = 1; p.mct = 0;
    return rc;
}
// the rows of tile t (< 0: no geometry): its own grk_amd_tile_num_blocks, or -- sub-sampled components -- every component's
int64_t tile_rows(const grk_amd_stream_info& info, uint32_t t, grk_amd_tile_params& p)
{
    if (!subsampled(info)) {
        const int rc = grk_amd_layout_tile(&info.layout, &info.base, t, &p);
        return rc ? rc : grk_amd_tile_num_blocks(&p);
    }
    int64_t n = 0;
    for (uint32_t c = 0; c < info.base.num_comps; ++c) {
        const int rc = tile_comp_params(info, t, c, p);
        const int64_t nb = rc ? rc : grk_amd_tile_num_blocks(&p);
        if (nb < 0) return nb;
        n += nb;
    }
    return n;
}

// One tile: its tile-parts' headers (PLT), then its packets -- the tile-parts' bodies end to end are the tile's packet sequence,
// and every body holds whole packets.  In file order, or, when PLT gives every packet's place (every tile-part that holds packets
// lists exactly its own), precinct by precinct on `threads` threads (a precinct's packets depend on each other through its tag
// trees and Lblock, on nothing else).  parts[t] is the tile's first tile-part, .next leads to the following ones.
int read_tile(const Bytes& b, const grk_amd_stream_info& info, uint32_t t, const std::vector<TilePart>& parts, BlockState* st, grk_amd_coded_block* rows,
              uint32_t threads, uint32_t drop_res, bool ht_refine, std::atomic<bool>& met_ht_second_pass, std::vector<Precinct>& keep, std::string& err)
{
    TileCtx T;
    T.met_ht_second_pass = &met_ht_second_pass;
    T.b = b; T.info = &info; T.tile = t; T.st = st;
    T.ht = !info.base.reserved[0]; T.sty = info.base.reserved[1]; T.ht_refine = ht_refine;
    T.sop = (info.flags & GRK_AMD_CS_SOP) != 0; T.eph = (info.flags & GRK_AMD_CS_EPH) != 0;
    grk_amd_tile_params p;
    int rc = grk_amd_layout_tile(&info.layout, &info.base, t, &p);
    if (rc) return refuse(err, rc, "tile %u: no geometry (%d)", t, rc);
    const uint32_t nc = p.num_comps;
    const bool sub = subsampled(info);
    // every component's tile-component: the tile's own, or -- sub-sampled components -- its rectangle in the component's samples;
    // components of one size share a geometry
    T.geoms.reserve(nc);
    T.cg.resize(nc); T.row0.resize(nc);
    uint64_t nrows = 0;
    for (uint32_t c = 0; c < nc; ++c) {
        uint32_t like = c;
        for (uint32_t k = 0; k < c; ++k) if (!sub || (info.comp_dx[k] == info.comp_dx[c] && info.comp_dy[k] == info.comp_dy[c])) { like = k; break; }
        if (like == c) {
            grk_amd_tile_params pc = p;
            if (sub) rc = tile_comp_params(info, t, c, pc);
            T.geoms.emplace_back();
            if (!rc) rc = build_tile_geom(pc, T.geoms.back());
            if (rc) return refuse(err, rc, "tile %u component %u: no geometry (%d)", t, c, rc);
            T.cg[c] = &T.geoms.back();
        } else T.cg[c] = T.cg[like];
        T.row0[c] = nrows; nrows += T.cg[c]->blocks_per_comp;
    }
    const uint32_t order = (info.flags >> GRK_AMD_CS_PROG_SHIFT) & 7u, L = info.num_layers;
    T.seq = packet_order(T.cg, sub ? info.comp_dx : nullptr, sub ? info.comp_dy : nullptr, p.tile_x0, p.tile_y0, order);
    const uint64_t np = T.seq.size(), npk = np * L;
    // the tile-part headers: where every body lies, and the PLT entries of all of them one list
    struct Body { uint64_t pos, end; uint64_t plt_at, plt_n; bool have_plt; };
    std::vector<Body> body;
    std::vector<uint32_t> plt;
    const bool multi = parts[t].next != 0;
    char where[48];
    auto at_part = [&](size_t k) -> const char* {           // "tile 3", of a tile in several tile-parts "tile 3 tile-part 1"
        if (multi) std::snprintf(where, sizeof where, "tile %u tile-part %u", t, (unsigned)k);
        else std::snprintf(where, sizeof where, "tile %u", t);
        return where;
    };
    uint64_t body_bytes = 0;
    for (uint32_t idx = t;; idx = parts[idx].next) {
        const TilePart& tp = parts[idx];
        const size_t k = body.size();
        if (k >= 255 || tp.len < 14 || !b.has(tp.at, tp.len)) return refuse(err, GRK_AMD_ERR_INVALID, "%s: the tile-part list", at_part(k));
        const uint64_t end = tp.at + tp.len;
        uint64_t pos = tp.at + 12;
        Body B{0, end, plt.size(), 0, false};
        uint64_t v = 0; bool open = false;
        for (;;) {
            if (end - pos < 2) return refuse(err, GRK_AMD_ERR_INVALID, "%s: no SOD marker", at_part(k));
            const uint32_t m = b.u16(pos);
            if (m == 0xFF93) { pos += 2; break; }
            if (end - pos < 4) return refuse(err, GRK_AMD_ERR_INVALID, "%s: no SOD marker", at_part(k));
            const uint32_t l = b.u16(pos + 2);
            if (m < 0xFF30 || l < 2 || (uint64_t)l + 2 > end - pos) return refuse(err, GRK_AMD_ERR_INVALID, "%s: broken marker segment 0x%04X", at_part(k), m);
            if (m == 0xFF58) {
                if (l < 3) return refuse(err, GRK_AMD_ERR_INVALID, "%s: broken PLT", at_part(k));
                B.have_plt = true;
                for (uint64_t i = pos + 5; i < pos + 2 + l; ++i) {
                    const uint32_t x = b.u8(i);
                    v = v << 7 | (x & 0x7Fu); open = true;
                    if (v > 0xFFFFFFFFull) return refuse(err, GRK_AMD_ERR_INVALID, "%s: a PLT packet length wraps", at_part(k));
                    if (!(x & 0x80u)) {
                        if (plt.size() >= npk) return refuse(err, GRK_AMD_ERR_INVALID, "%s: PLT lists more than the tile's %llu packets", at_part(k), (unsigned long long)npk);
                        plt.push_back((uint32_t)v); v = 0; open = false;
                    }
                }
            } else if (m == 0xFF64) {
                // COM
            } else if (const char* name = marker_name(m)) {
                return refuse(err, GRK_AMD_ERR_UNSUPPORTED, "%s marker segment in a tile-part header", name);
            } else {
                return refuse(err, GRK_AMD_ERR_UNSUPPORTED, "marker segment 0x%04X in a tile-part header", m);
            }
            pos += 2 + (uint64_t)l;
        }
        B.pos = pos; B.plt_n = plt.size() - B.plt_at;
        if (open) return refuse(err, GRK_AMD_ERR_INVALID, "%s: PLT lists %llu packets and a part of one", at_part(k), (unsigned long long)B.plt_n);
        body_bytes += end - pos;
        body.push_back(B);
        if (!tp.next) break;
        if (tp.next >= parts.size()) return refuse(err, GRK_AMD_ERR_INVALID, "%s: the tile-part list", at_part(k));
    }
    if (npk > body_bytes) return refuse(err, GRK_AMD_ERR_INVALID, "tile %u: %llu packets in %llu bytes", t, (unsigned long long)npk, (unsigned long long)body_bytes);
    // a PLT tile: every tile-part that holds packets lists them
    bool plt_tile = !plt.empty();
    for (const Body& B : body) if (B.pos != B.end && !B.have_plt) plt_tile = false;
    if (!multi) plt_tile = body[0].have_plt;
    if (plt_tile && plt.size() != npk)
        return refuse(err, GRK_AMD_ERR_INVALID, "tile %u: PLT lists %llu packets of %llu", t, (unsigned long long)plt.size(), (unsigned long long)npk);
    T.prec.resize(np);
    // RLCP: the layers run inside a resolution -- run[i] = {first packet of seq[i]'s resolution, packets of it}
    std::vector<std::pair<uint32_t, uint32_t>> run;
    if (order == 1) {
        run.resize(np);
        for (uint64_t i = 0; i < np;) {
            uint64_t j = i;
            while (j < np && T.seq[j].r == T.seq[i].r) ++j;
            for (uint64_t k = i; k < j; ++k) run[k] = {(uint32_t)i, (uint32_t)(j - i)};
            i = j;
        }
    }
    // the number (place in the tile's packet sequence) of precinct i's packet of layer l
    auto number_of = [&](uint64_t i, uint64_t l) -> uint64_t {
        if (order == 0) return l * np + i;
        if (order == 1) return (uint64_t)run[i].first * L + l * run[i].second + (i - run[i].first);
        return i * L + l;
    };
    // (a packet's refusal names the tile-part it was read in)
    auto in_part = [&](std::string& e, size_t k) { if (multi) e += " (tile-part " + std::to_string(k) + ")"; };
    if (plt_tile && threads > 1 && np > 1) {
        std::vector<uint64_t> start(npk + 1, 0);
        std::vector<uint8_t> part_of(multi ? npk : 0);
        uint64_t k = 0;
        for (size_t q = 0; q < body.size(); ++q) {
            uint64_t at = body[q].pos;
            for (uint64_t j = 0; j < body[q].plt_n; ++j, ++k) {
                start[k] = at; at += plt[k];
                if (multi) part_of[k] = (uint8_t)q;
                if (at > body[q].end) break;
            }
            if (at != body[q].end) return refuse(err, GRK_AMD_ERR_INVALID, "%s: the PLT lengths do not add up to the tile-part", at_part(q));
        }
        std::mutex mu;
        rc = parallel_for(np, threads, [&](size_t i) -> int {
            std::string e;
            for (uint32_t l = 0; l < L; ++l) {
                const uint64_t k = number_of(i, l);
                uint64_t at = start[k];
                const uint64_t stop = start[k] + plt[k];
                int r = read_packet(T, (uint32_t)i, l, (uint32_t)k, at, stop, e);
                if (!r && at != stop) r = refuse(e, GRK_AMD_ERR_INVALID, "tile %u packet %llu: %llu bytes, PLT says %u", t, (unsigned long long)k,
                                                 (unsigned long long)(at - start[k]), plt[k]);
                if (r) { in_part(e, multi ? part_of[k] : 0); std::lock_guard<std::mutex> lk(mu); if (err.empty()) err = e; return r; }
            }
            return GRK_AMD_OK;
        });
        if (rc) return rc;
    } else {
        uint64_t k = 0, used = 0;            // packets read in all; in the tile-part at hand
        size_t cur = 0;
        uint64_t pos = body[0].pos;
        // a tile-part is left where its last packet ends: its PLT, if it has one, listed just those
        auto leave = [&]() -> int {
            if (body[cur].have_plt && used != body[cur].plt_n)
                return refuse(err, GRK_AMD_ERR_INVALID, "%s: the PLT lengths do not add up to the tile-part (%llu packets listed, %llu read)", at_part(cur),
                              (unsigned long long)body[cur].plt_n, (unsigned long long)used);
            return GRK_AMD_OK;
        };
        auto one = [&](uint64_t i, uint32_t l) -> int {
            while (multi && pos == body[cur].end) {          // on to the next tile-part that holds a byte
                if (int r = leave()) return r;
                if (cur + 1 == body.size())
                    return refuse(err, GRK_AMD_ERR_INVALID, "%s: the tile ends at packet %llu of %llu", at_part(cur), (unsigned long long)k, (unsigned long long)npk);
                ++cur; used = 0; pos = body[cur].pos;
            }
            const Body& B = body[cur];
            const uint64_t from = pos;
            const int r = read_packet(T, (uint32_t)i, l, (uint32_t)k, pos, B.end, err);
            if (r) { in_part(err, cur); return r; }
            if (B.have_plt && (used >= B.plt_n || pos - from != plt[B.plt_at + used])) {
                if (used >= B.plt_n)
                    return refuse(err, GRK_AMD_ERR_INVALID, "%s: the PLT lengths do not add up to the tile-part (packet %llu is not listed)", at_part(cur), (unsigned long long)k);
                refuse(err, GRK_AMD_ERR_INVALID, "tile %u packet %llu: %llu bytes, PLT says %u", t, (unsigned long long)k, (unsigned long long)(pos - from),
                       plt[B.plt_at + used]);
                in_part(err, cur);
                return GRK_AMD_ERR_INVALID;
            }
            ++k; ++used;
            return GRK_AMD_OK;
        };
        if (order == 0) {
            for (uint32_t l = 0; l < L; ++l) for (uint64_t i = 0; i < np; ++i) if ((rc = one(i, l))) return rc;
        } else if (order == 1) {
            for (uint64_t i = 0; i < np; i += run[i].second)
                for (uint32_t l = 0; l < L; ++l) for (uint64_t j = i; j < i + run[i].second; ++j) if ((rc = one(j, l))) return rc;
        } else {
            for (uint64_t i = 0; i < np; ++i) for (uint32_t l = 0; l < L; ++l) if ((rc = one(i, l))) return rc;
        }
        // the tile's last packet ends its tile-part; what follows of the tile holds nothing
        for (;; ++cur, used = 0, pos = body[cur].pos) {
            if (pos != body[cur].end)
                return refuse(err, GRK_AMD_ERR_INVALID, "%s: %llu bytes behind the last packet", at_part(cur), (unsigned long long)(body[cur].end - pos));
            if ((rc = leave())) return rc;
            if (cur + 1 == body.size()) break;
        }
    }
    // the tile's rows (a block of several pieces gets its place in the appendix later)
    for (uint32_t c = 0; c < nc; ++c)
        for (uint32_t i = 0; i < T.cg[c]->blocks_per_comp; ++i) {
            BlockState& s = st[T.row0[c] + i];
            grk_amd_coded_block& row = rows[T.row0[c] + i];
            s.dropped = T.cg[c]->blocks_comp0[i].res + drop_res > info.base.num_levels;
            row.offset = s.pieces ? s.src0 : 0; row.length = s.total; row.missing_msbs = 0;
            if (T.ht) row.missing_msbs = s.zbp;
            else if (s.total) {
                const grk_amd_block& gb = T.cg[c]->blocks_comp0[i];
                const uint32_t bi = gb.res == 0 ? 0u : 3u * gb.res - 2u + (gb.band - 1u);
                const int expn = info.qstyle ? info.qcd_words[bi] >> 11 : info.qcd_words[bi] >> 3;
                const int numbps = expn + (int)info.guard_bits - 1 - (int)s.zbp;
                if (numbps < 1 || (int)s.passes > 3 * numbps - 2)
                    return refuse(err, GRK_AMD_ERR_INVALID, "tile %u block %u: %u passes over %d bit-planes", t, (uint32_t)T.row0[c] + i, s.passes, numbps);
                row.missing_msbs = (uint32_t)numbps | (uint32_t)s.passes << 8;
            }
        }
    for (Precinct& P : T.prec) { std::vector<uint32_t>().swap(P.nodes); }
    keep = std::move(T.prec);
    return GRK_AMD_OK;
}

thread_local std::string g_reader_error;

} // namespace


int grk_amd::read_stream_header(const uint8_t* cs, uint64_t len, grk_amd_stream_info& info, std::string& err)
{
    err.clear();
    if (!cs) return refuse(err, GRK_AMD_ERR_INVALID, "no codestream");
    const Bytes b{cs, len};
    uint64_t sot = 0;
    int rc = parse_main_header(b, info, sot, err);
    if (rc) return rc;
    const int64_t nt = grk_amd_layout_num_tiles(&info.layout);
    if (nt < 0) return refuse(err, (int)nt, nt == GRK_AMD_ERR_UNSUPPORTED ? "SIZ: more than 65535 tiles" : "SIZ: image area and tile grid do not fit");
    info.num_tiles = (uint32_t)nt;
    {   // the tables are sized by what SIZ and COD declare: decline what no real image is before anything is allocated
        uint32_t cxe = info.base.cblk_w_exp, cye = info.base.cblk_h_exp;
        for (uint32_t r = 0; r <= info.base.num_levels; ++r)
            if (const uint32_t pe = info.base.precinct_exp[r]) {
                cxe = std::min<uint32_t>(cxe, (pe & 15u) - (r ? 1u : 0u)); cye = std::min<uint32_t>(cye, (pe >> 4) - (r ? 1u : 0u));
            }
        const uint64_t W = info.layout.x1 - info.layout.x0, H = info.layout.y1 - info.layout.y0;
        if (((W >> cxe) + 1) * ((H >> cye) + 1) * info.base.num_comps > kMaxBlocksGuess)
            return refuse(err, GRK_AMD_ERR_UNSUPPORTED, "an image of %llu x %llu in code-blocks of 2^%u x 2^%u: too many", (unsigned long long)W, (unsigned long long)H, cxe, cye);
    }
    grk_amd_tile_params p;
    for (uint32_t t = 0; t < info.num_tiles; ++t) {
        const int64_t nb = tile_rows(info, t, p);
        if (nb < 0) return refuse(err, (int)nb, "tile %u (%u x %u at %u, %u): no geometry (%d)", t, p.tile_w, p.tile_h, p.tile_x0, p.tile_y0, (int)nb);
        info.num_blocks += (uint64_t)nb;
        if (info.num_blocks > 4 * kMaxBlocksGuess) return refuse(err, GRK_AMD_ERR_UNSUPPORTED, "more than %llu code-blocks", (unsigned long long)(4 * kMaxBlocksGuess));
    }
    (void)grk_amd_layout_tile(&info.layout, &info.base, 0, &p);
    info.base = p;
    // PLT: as the first tile-part's header has it
    for (uint64_t at = sot + 12; b.has(at, 4) && b.u16(at) != 0xFF93; at += 2 + (uint64_t)b.u16(at + 2)) {
        if (b.u16(at) == 0xFF58) { info.flags |= GRK_AMD_CS_PLT; break; }
        if (b.u16(at) < 0xFF30 || b.u16(at + 2) < 2) break;
    }
    return GRK_AMD_OK;
}

int grk_amd::read_stream_packets(const uint8_t* cs, uint64_t len, const grk_amd_stream_info& info, uint32_t threads, StreamTable& out, std::string& err,
                                 bool allow_parts, bool ht_refine)
{
    grk_amd_stream_info own;
    int rc = read_stream_header(cs, len, own, err);
    if (rc) return rc;
    if (std::memcmp(&own, &info, sizeof own) != 0) return refuse(err, GRK_AMD_ERR_INVALID, "info is not what grk_amd_read_header gives for this codestream");
    std::vector<StreamPart> parts;
    rc = allow_parts ? locate_stream_parts(cs, len, info, parts, err) : locate_stream_parts_single(cs, len, info, parts, err);
    if (rc) return rc;
    return read_stream_packets_of(cs, len, info, parts, nullptr, 0, threads, out, err, ht_refine);
}

// Every tile-part of the file, each tile's in TPsot order (T.800 A.4.2; the reference: TileLengthMarkers, CodeStreamDecompress's SOT
// checks): from TLM, else along the Psot chain.  Only SOT marker segments are read here.
int grk_amd::locate_stream_parts(const uint8_t* cs, uint64_t len, const grk_amd_stream_info& info, std::vector<StreamPart>& parts, std::string& err)
{
    const Bytes b{cs, len};
    const uint32_t nt = info.num_tiles;
    constexpr uint32_t kMaxParts = 65535, kMaxPartsOfTile = 255;
    std::vector<uint64_t> off; std::vector<uint32_t> ln; std::vector<uint16_t> idx;
    const bool tlm = (info.flags & GRK_AMD_CS_TLM) != 0;
    if (tlm) {
        int used = 0;
        const int64_t n = grk_amd_locate_tile_parts(cs, len, nullptr, nullptr, nullptr, 0, &used);
        if (n < 0 || !used) return refuse(err, GRK_AMD_ERR_INVALID, "the tile-parts cannot be located");
        if (n > kMaxParts) return refuse(err, GRK_AMD_ERR_UNSUPPORTED, "%lld tile-parts (at most %u)", (long long)n, kMaxParts);
        off.resize(n); ln.resize(n); idx.resize(n);
        (void)grk_amd_locate_tile_parts(cs, len, off.data(), ln.data(), idx.data(), (uint64_t)n, &used);
    } else {
        // SOT to SOT over Psot: every hop is at least 14 bytes, so the walk ends with the stream
        uint64_t at = 2;
        while (b.has(at, 4) && b.u16(at) != 0xFF90) at += 2 + (uint64_t)b.u16(at + 2);       // (the main header: parse_main_header has passed it)
        while (b.has(at, 12) && b.u16(at) == 0xFF90) {
            const uint32_t isot = b.u16(at + 4), psot = b.u32(at + 6), tps = b.u8(at + 10);
            const uint64_t l = psot ? psot : len >= at + 2 ? len - 2 - at : 0;               // Psot 0: the last tile-part runs to EOC
            if (l < 14 || !b.has(at, l))
                return refuse(err, GRK_AMD_ERR_INVALID, "tile %u tile-part %u: Psot %u leaves the stream (%llu bytes from its SOT)", isot, tps, psot,
                              (unsigned long long)(len - at));
            if (off.size() == kMaxParts) return refuse(err, GRK_AMD_ERR_UNSUPPORTED, "more than %u tile-parts", kMaxParts);
            off.push_back(at); ln.push_back((uint32_t)l); idx.push_back((uint16_t)isot);
            at += l;
        }
    }
    const size_t n = off.size();
    parts.assign(nt, StreamPart{});
    parts.reserve(std::max<size_t>(nt, n));
    struct Seen { uint32_t count = 0, declared = 0, last = 0; };          // tile-parts so far, its non-zero TNsot, the place of the latest in `parts`
    std::vector<Seen> seen(nt);
    for (size_t i = 0; i < n; ++i) {
        if (ln[i] < 14 || !b.has(off[i], ln[i]) || b.u16(off[i]) != 0xFF90 || b.u16(off[i] + 2) != 10)
            return refuse(err, GRK_AMD_ERR_INVALID, "tile-part %llu: no SOT marker segment where it should start", (unsigned long long)i);
        const uint32_t isot = b.u16(off[i] + 4), psot = b.u32(off[i] + 6), tps = b.u8(off[i] + 10), tn = b.u8(off[i] + 11);
        if (isot >= nt || (tlm && isot != idx[i])) return refuse(err, GRK_AMD_ERR_INVALID, "tile-part %llu: tile index %u", (unsigned long long)i, isot);
        if (psot && psot != ln[i]) return refuse(err, GRK_AMD_ERR_INVALID, "tile %u tile-part %u: Psot %u, TLM %u", isot, tps, psot, ln[i]);
        if (!psot && i + 1 != n) return refuse(err, GRK_AMD_ERR_INVALID, "tile %u tile-part %u: Psot 0 in a tile-part that is not the file's last", isot, tps);
        Seen& s = seen[isot];
        if (tps >= kMaxPartsOfTile && tps == s.count) return refuse(err, GRK_AMD_ERR_UNSUPPORTED, "tile %u tile-part %u: more than %u tile-parts of one tile", isot, tps, kMaxPartsOfTile);
        if (tps != s.count)
            return refuse(err, GRK_AMD_ERR_INVALID, "tile %u tile-part %u: the file has %u tile-parts of the tile before it (a TPsot missing, repeated or out of order)",
                          isot, tps, s.count);
        if (tn && s.declared && tn != s.declared) return refuse(err, GRK_AMD_ERR_INVALID, "tile %u tile-part %u: TNsot %u, an earlier tile-part said %u", isot, tps, tn, s.declared);
        if (tn) s.declared = tn;
        if (s.declared && s.declared <= tps) return refuse(err, GRK_AMD_ERR_INVALID, "tile %u tile-part %u: TNsot %u", isot, tps, s.declared);
        if (!s.count) { parts[isot] = StreamPart{off[i], ln[i], true, 0}; s.last = isot; }
        else { parts[s.last].next = (uint32_t)parts.size(); s.last = (uint32_t)parts.size(); parts.push_back(StreamPart{off[i], ln[i], true, 0}); }
        ++s.count;
    }
    for (uint32_t t = 0; t < nt; ++t) {
        if (!seen[t].count) return refuse(err, GRK_AMD_ERR_INVALID, "tile %u has no tile-part", t);
        if (seen[t].declared > seen[t].count)
            return refuse(err, GRK_AMD_ERR_INVALID, "tile %u tile-part %u: missing (TNsot %u, %u found)", t, seen[t].count, seen[t].declared, seen[t].count);
    }
    return GRK_AMD_OK;
}

// ... of a file with one tile-part per tile; any other is refused (the three older reader calls)
int grk_amd::locate_stream_parts_single(const uint8_t* cs, uint64_t len, const grk_amd_stream_info& info, std::vector<StreamPart>& parts, std::string& err)
{
    const Bytes b{cs, len};
    const uint32_t nt = info.num_tiles;
    // the tile-parts: one per tile
    parts.assign(nt, StreamPart{});
    std::vector<uint64_t> off(nt); std::vector<uint32_t> ln(nt); std::vector<uint16_t> idx(nt);
    int used = 0;
    const int64_t n = grk_amd_locate_tile_parts(cs, len, off.data(), ln.data(), idx.data(), nt, &used);
    if (n < 0) return refuse(err, GRK_AMD_ERR_INVALID, "the tile-parts cannot be located");
    for (int64_t i = 0; i < std::min<int64_t>(n, nt); ++i) {
        if (ln[i] < 14 || !b.has(off[i], ln[i]) || b.u16(off[i]) != 0xFF90 || b.u16(off[i] + 2) != 10)
            return refuse(err, GRK_AMD_ERR_INVALID, "tile-part %lld: no SOT marker segment where it should start", (long long)i);
        const uint32_t isot = b.u16(off[i] + 4), psot = b.u32(off[i] + 6), tps = b.u8(off[i] + 10), tn = b.u8(off[i] + 11);
        if (isot >= nt || (used && isot != idx[i])) return refuse(err, GRK_AMD_ERR_INVALID, "tile-part %lld: tile index %u", (long long)i, isot);
        if (tps != 0 || tn > 1 || parts[isot].seen) return refuse(err, GRK_AMD_ERR_UNSUPPORTED, "more than one tile-part per tile (tile %u)", isot);
        if (psot && psot != ln[i]) return refuse(err, GRK_AMD_ERR_INVALID, "tile-part %lld: Psot %u, TLM %u", (long long)i, psot, ln[i]);
        parts[isot] = TilePart{off[i], ln[i], true, 0};
    }
    if (n > nt) return refuse(err, GRK_AMD_ERR_UNSUPPORTED, "more than one tile-part per tile (%lld tile-parts, %u tiles)", (long long)n, nt);
    for (uint32_t t = 0; t < nt; ++t) if (!parts[t].seen) return refuse(err, GRK_AMD_ERR_INVALID, "tile %u has no tile-part", t);
    return GRK_AMD_OK;
}

int grk_amd::read_stream_packets_of(const uint8_t* cs, uint64_t len, const grk_amd_stream_info& info, const std::vector<StreamPart>& parts,
                                    const std::vector<uint32_t>* tiles, uint32_t drop_res, uint32_t threads, StreamTable& out, std::string& err, bool ht_refine)
{
    threads = std::max<uint32_t>(1, std::min<uint32_t>(threads, 16));
    const Bytes b{cs, len};
    if (parts.size() < info.num_tiles) return refuse(err, GRK_AMD_ERR_INVALID, "the tile-parts are not this stream's");
    // the tiles to read: tile_of(i), i < nt
    const uint32_t nt = tiles ? (uint32_t)tiles->size() : info.num_tiles;
    auto tile_of = [tiles](size_t i) { return tiles ? (*tiles)[i] : (uint32_t)i; };
    for (uint32_t i = 0; i < nt; ++i)
        if (tile_of(i) >= info.num_tiles || (i && tile_of(i) <= tile_of(i - 1))) return refuse(err, GRK_AMD_ERR_INVALID, "the tile list");
    int rc = GRK_AMD_OK;
    out = StreamTable{};
    out.row_at.assign(nt + 1, 0);
    grk_amd_tile_params p;
    for (uint32_t t = 0; t < nt; ++t) {
        const int64_t nb = tile_rows(info, tile_of(t), p);
        if (nb < 0) return refuse(err, (int)nb, "tile %u: no geometry", tile_of(t));
        out.row_at[t + 1] = out.row_at[t] + (uint64_t)nb;
    }
    const uint64_t nrows = out.row_at[nt];
    if (!tiles && nrows != info.num_blocks) return refuse(err, GRK_AMD_ERR_INVALID, "info.num_blocks");
    out.rows.assign(nrows, grk_amd_coded_block{0, 0, 0});
    std::vector<BlockState> st(nrows);
    std::vector<std::vector<Precinct>> left(nt);
    std::atomic<bool> met{false};
    if (nt >= threads || threads == 1) {
        std::mutex mu;
        rc = parallel_for(nt, threads, [&](size_t t) -> int {
            std::string e;
            const int r = read_tile(b, info, tile_of(t), parts, st.data() + out.row_at[t], out.rows.data() + out.row_at[t], 1, drop_res, ht_refine, met, left[t], e);
            if (r) { std::lock_guard<std::mutex> lk(mu); if (err.empty()) err = e; }
            return r;
        });
    } else {
        for (uint32_t t = 0; t < nt && !rc; ++t)
            rc = read_tile(b, info, tile_of(t), parts, st.data() + out.row_at[t], out.rows.data() + out.row_at[t], threads, drop_res, ht_refine, met, left[t], err);
    }
    if (rc) { if (err.empty()) (void)refuse(err, rc, "the packets cannot be read (%d)", rc); out.met_ht_second_pass = met.load(); return rc; }
    // Segment lists and the appendix, in an order that does not depend on the threads: rows in order, a row's records in the order
    // its precinct met them
    out.first_segment.assign(nrows + 1, 0);
    for (uint32_t t = 0; t < nt; ++t)
        for (const Precinct& P : left[t]) for (const SegRec& s : P.segs) ++out.first_segment[out.row_at[t] + s.row + 1];
    for (uint64_t i = 0; i < nrows; ++i) {
        if ((uint64_t)out.first_segment[i] + out.first_segment[i + 1] > 0xFFFFFFFFull) return refuse(err, GRK_AMD_ERR_UNSUPPORTED, "more than 2^32 codeword segments");
        out.first_segment[i + 1] += out.first_segment[i];
    }
    out.segments.resize(out.first_segment[nrows]);
    std::vector<uint64_t> cursor(nrows);
    for (uint64_t i = 0; i < nrows; ++i) cursor[i] = out.first_segment[i];
    for (uint32_t t = 0; t < nt; ++t)
        for (const Precinct& P : left[t]) for (const SegRec& s : P.segs) out.segments[cursor[out.row_at[t] + s.row]++] = grk_amd_segment{s.len, s.passes};
    uint64_t app = 0;
    for (uint64_t i = 0; i < nrows; ++i)
        if (st[i].pieces > 1 && !st[i].dropped) { out.rows[i].offset = len + app; cursor[i] = app; app += st[i].total; }
    out.appendix_bytes = app;
    out.move_at.assign(nt + 1, 0);
    for (uint32_t t = 0; t < nt; ++t) {
        for (const Precinct& P : left[t])
            for (const Piece& q : P.pieces) {
                if (!app) break;
                const uint64_t i = out.row_at[t] + q.row;
                if (st[i].pieces > 1 && !st[i].dropped) { out.moves.push_back(grk_amd_tp_segment{cursor[i], q.src, q.len, 1u}); cursor[i] += q.len; }
            }
        out.move_at[t + 1] = out.moves.size();
    }
    return GRK_AMD_OK;
}

extern "C" const char* grk_amd_reader_last_error(void) { return g_reader_error.c_str(); }

extern "C" int grk_amd_read_header(const uint8_t* cs, uint64_t len, grk_amd_stream_info* info)
{
    if (!info) { g_reader_error = "no info"; return GRK_AMD_ERR_INVALID; }
    return read_stream_header(cs, len, *info, g_reader_error);
}

extern "C" int grk_amd_stream_comp_size(const grk_amd_stream_info* info, uint32_t comp, uint32_t* w, uint32_t* h)
{
    if (!info || !w || !h || comp >= info->base.num_comps || comp >= 4 || !info->comp_dx[comp] || !info->comp_dy[comp]) return GRK_AMD_ERR_INVALID;
    const uint64_t dx = info->comp_dx[comp], dy = info->comp_dy[comp];
    *w = (uint32_t)((info->layout.x1 + dx - 1) / dx - (info->layout.x0 + dx - 1) / dx);
    *h = (uint32_t)((info->layout.y1 + dy - 1) / dy - (info->layout.y0 + dy - 1) / dy);
    return GRK_AMD_OK;
}

static int64_t read_packets_into(bool allow_parts, bool ht_refine, const uint8_t* cs, uint64_t len, const grk_amd_stream_info* info, uint32_t threads,
                                 grk_amd_coded_block* rows, uint64_t row_cap,
                                 uint32_t* first_segment, grk_amd_segment* segments, uint64_t seg_cap, uint64_t* num_segments,
                                 grk_amd_tp_segment* moves, uint64_t move_cap, uint64_t* num_moves, uint64_t* appendix_bytes)
{
    if (!info) { g_reader_error = "no info"; return GRK_AMD_ERR_INVALID; }
    StreamTable s;
    const int rc = read_stream_packets(cs, len, *info, threads, s, g_reader_error, allow_parts, ht_refine);
    if (rc) return rc;
    if (num_segments) *num_segments = s.segments.size();
    if (num_moves) *num_moves = s.moves.size();
    if (appendix_bytes) *appendix_bytes = s.appendix_bytes;
    if (!rows) return (int64_t)s.rows.size();
    if (s.rows.size() > row_cap || (segments && s.segments.size() > seg_cap) || (moves && s.moves.size() > move_cap) || (!moves && !s.moves.empty()))
        return refuse(g_reader_error, GRK_AMD_ERR_OVERFLOW, "%llu rows, %llu segments, %llu moves do not fit the caller's arrays",
                      (unsigned long long)s.rows.size(), (unsigned long long)s.segments.size(), (unsigned long long)s.moves.size());
    if (!s.rows.empty()) std::memcpy(rows, s.rows.data(), s.rows.size() * sizeof rows[0]);
    if (first_segment) std::memcpy(first_segment, s.first_segment.data(), s.first_segment.size() * sizeof first_segment[0]);
    if (segments && !s.segments.empty()) std::memcpy(segments, s.segments.data(), s.segments.size() * sizeof segments[0]);
    if (moves && !s.moves.empty()) std::memcpy(moves, s.moves.data(), s.moves.size() * sizeof moves[0]);
    return (int64_t)s.rows.size();
}

extern "C" int64_t grk_amd_read_packets(const uint8_t* cs, uint64_t len, const grk_amd_stream_info* info, uint32_t threads,
                                        grk_amd_coded_block* rows, uint64_t row_cap,
                                        uint32_t* first_segment, grk_amd_segment* segments, uint64_t seg_cap, uint64_t* num_segments,
                                        grk_amd_tp_segment* moves, uint64_t move_cap, uint64_t* num_moves, uint64_t* appendix_bytes)
{
    return read_packets_into(false, false, cs, len, info, threads, rows, row_cap, first_segment, segments, seg_cap, num_segments, moves, move_cap, num_moves, appendix_bytes);
}

extern "C" int64_t grk_amd_read_packets_parts(const uint8_t* cs, uint64_t len, const grk_amd_stream_info* info, uint32_t threads,
                                              grk_amd_coded_block* rows, uint64_t row_cap,
                                              uint32_t* first_segment, grk_amd_segment* segments, uint64_t seg_cap, uint64_t* num_segments,
                                              grk_amd_tp_segment* moves, uint64_t move_cap, uint64_t* num_moves, uint64_t* appendix_bytes)
{
    return read_packets_into(true, false, cs, len, info, threads, rows, row_cap, first_segment, segments, seg_cap, num_segments, moves, move_cap, num_moves, appendix_bytes);
}

extern "C" int64_t grk_amd_read_packets_refine(const uint8_t* cs, uint64_t len, const grk_amd_stream_info* info, uint32_t threads,
                                               grk_amd_coded_block* rows, uint64_t row_cap,
                                               uint32_t* first_segment, grk_amd_segment* segments, uint64_t seg_cap, uint64_t* num_segments,
                                               grk_amd_tp_segment* moves, uint64_t move_cap, uint64_t* num_moves, uint64_t* appendix_bytes)
{
    return read_packets_into(true, true, cs, len, info, threads, rows, row_cap, first_segment, segments, seg_cap, num_segments, moves, move_cap, num_moves, appendix_bytes);
}
