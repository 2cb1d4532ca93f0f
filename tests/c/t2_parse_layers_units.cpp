// tests/c/t2_parse_layers_units.cpp -- the GENERAL device Tier-2 reader played on the CPU (tests/test_t2_parse_layers_cpu.py builds it
// with -fsanitize=address,undefined): KL and KH as tests/c/t2_parse_units.cpp plays them, then KC-L, KF and KP of
// grok_amd/csrc/kernels_t2read.hip as plain loops over t2_parse_layers.h and the plan of plan_t2_read_layers, chain by chain -- in
// rising and in falling order --, against the host reader (t2_reader.cpp, threads = 1): rows, first_segment, segments and the
// appendix's size field for field, the moves as a set (both sorted by dst), its code where it refuses.  Every stream sits in a heap
// buffer of exactly its length.
//   t2_parse_layers_units check F..   "<name> host <code> core <code> tables <equal|DIFFER|->" per file (exit 1 where the two differ)
//   t2_parse_layers_units sweep F..   fixed-seed single-byte changes and truncations of every file, tallied by region
//   t2_parse_layers_units plan F..    the plan's numbers (chains, numbering, scratch) against a brute-force count from the geometry
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static uint64_t g_max[8], g_sum[8], g_lmax[2];
#define GRK_T2P_COUNT(id, n) do { const uint64_t n_ = (n); if (n_ > g_max[id]) g_max[id] = n_; g_sum[id] += n_; } while (0)
#define GRK_T2P_COUNT_L(id, n) do { const uint64_t n_ = (n); if (n_ > g_lmax[id]) g_lmax[id] = n_; } while (0)
#include "../../grok_amd/csrc/t2_parse.h"
#include "../../grok_amd/csrc/t2_parse_layers.h"
#include "../../grok_amd/csrc/t2_read_plan.h"
#include "../../grok_amd/csrc/t2_reader.h"
#include "../../grok_amd/csrc/geometry.h"
#include "../../grok_amd/csrc/t2_order.h"

using namespace grk_amd;

namespace {

struct HeapSrc {
    const uint8_t* d; uint64_t len;
    uint32_t byte(uint64_t i) const { if (i >= len) { std::printf("FAIL: the core reads byte %llu of %llu\n", (unsigned long long)i, (unsigned long long)len); std::exit(1); } return d[i]; }
};

enum Region { kMain, kSot, kPlt, kSopEph, kHeader, kLast, kBody, kRegions };
struct Span { uint64_t lo, hi; int kind; };
std::vector<Span> g_spans;
bool g_record = false;
void span(uint64_t lo, uint64_t hi, int kind) { if (g_record && hi > lo) g_spans.push_back(Span{lo, hi, kind}); }

struct Tables {
    std::vector<grk_amd_coded_block> rows;
    std::vector<uint32_t> first_segment;
    std::vector<grk_amd_segment> segments;
    std::vector<grk_amd_tp_segment> moves;
    uint64_t appendix = 0;
};

// a chain's share of the two logs, as KC-L's LogSink fills it
struct LogSink {
    T2ReadSegRecord* segs; uint32_t seg_cap, nseg = 0;
    T2ReadPieceRecord* pieces; uint32_t piece_cap, npiece = 0;
    bool over = false;
    void seg(uint32_t row, uint32_t ordinal, uint32_t len, uint32_t passes, bool opens)
    {
        if (nseg >= seg_cap) { over = true; return; }
        segs[nseg++] = T2ReadSegRecord{row, ordinal, len, passes | (opens ? 1u << 31 : 0u)};
    }
    void piece(uint32_t row, uint32_t ordinal, uint64_t rel, uint32_t len, uint32_t before)
    {
        if (npiece >= piece_cap) { over = true; return; }
        pieces[npiece++] = T2ReadPieceRecord{rel, row, ordinal, len, before};
    }
};

// the kernels in turn; the status word as the call would read it
uint64_t play(const uint8_t* cs, uint64_t len, const T2ReadLayersPlan& Q, bool reversed, Tables& out)
{
    const T2ReadPlan& P = Q.base;
    uint64_t status = kT2pNoStatus;
    auto report = [&](uint64_t w) { if (w < status) status = w; };
    HeapSrc src{cs, len};
    const uint32_t nt = P.num_tiles, L = Q.layers;
    // ---- KL
    bool tlm = false;
    std::vector<uint64_t> at; std::vector<uint32_t> ln, idx;
    uint64_t count = 0;
    if (t2_read_tlm(cs, len, len, nt, &tlm, at, ln, idx, &count)) return t2p_status_locate(0, kT2pNotLocated);
    uint64_t sot = 2;
    while (sot + 4 <= len && !(cs[sot] == 0xFF && cs[sot + 1] == 0x90)) sot += 2 + ((uint64_t)cs[sot + 2] << 8 | cs[sot + 3]);
    span(0, sot, kMain);
    if (!tlm) {
        uint64_t p = sot, hops = 0;
        for (const uint64_t max_hops = len / 14 + 1; hops < max_hops; ++hops) {
            uint64_t l = 0;
            const int r = t2p_hop(src, len, p, &l);
            if (r == 0) break;
            if (r == 2) return t2p_status_locate(0, kT2pNotLocated);
            if (count < nt) { at.push_back(p); ln.push_back((uint32_t)l); idx.push_back(0xFFFFFFFFu); }
            ++count; p += l;
        }
        if (count == 0) return t2p_status_locate(0, kT2pNotLocated);
    }
    const uint32_t n = (uint32_t)std::min<uint64_t>(count, nt);
    std::vector<uint32_t> first_of(nt, 0xFFFFFFFFu), part_len(nt, 0), has_plt(nt, 0);
    std::vector<uint64_t> part_at(nt, 0), body_at(nt, 0);
    std::vector<uint32_t> why_of(n), isot_of(n, 0xFFFFFFFFu);
    for (uint32_t i = 0; i < n; ++i) {
        why_of[i] = t2p_check_sot(src, len, at[i], ln[i], nt, tlm ? idx[i] : 0xFFFFFFFFu, &isot_of[i]);
        if (why_of[i] != kT2pNoSot && why_of[i] != kT2pTileIndex && i < first_of[isot_of[i]]) first_of[isot_of[i]] = i;
    }
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t why = why_of[i];
        if ((why == kT2pOk || why == kT2pPsotTlm) && first_of[isot_of[i]] < i) why = kT2pMultiPart;
        if (why) report(t2p_status_locate(i, why));
        else { part_at[isot_of[i]] = at[i]; part_len[isot_of[i]] = ln[i]; span(at[i], at[i] + 12, kSot); }
    }
    if (count > nt) report(t2p_status_locate(nt, kT2pManyParts));
    for (uint32_t t = 0; t < nt; ++t) if (first_of[t] == 0xFFFFFFFFu) report(t2p_status_locate(nt + 1 + t, kT2pNoPart));
    // ---- KH (a tile's npackets: the packets of every layer)
    std::vector<uint32_t> plt_len(std::max<uint64_t>(P.total_packets, nt), 0);
    std::vector<uint64_t> pk_start(plt_len.size(), 0);
    for (uint32_t t = 0; t < nt; ++t) {
        if (!part_len[t]) continue;
        const T2ReadTile& T = P.tiles[t];
        const uint64_t end = part_at[t] + part_len[t], npk = T.npackets;
        uint64_t pos = part_at[t] + 12, cnt = 0;
        bool have = false, done = false, failed = false;
        for (uint32_t hop = 0, hops = part_len[t] / 4 + 2; hop < hops && !failed; ++hop) {
            uint64_t next = 0, lo = 0, hi = 0;
            const int kind = t2p_header_segment(src, pos, end, &next, &lo, &hi);
            if (kind < 0) { report(t2p_status_tile(t, 0, 0, (uint32_t)-kind)); failed = true; break; }
            pos = next;
            if (kind == 0) { done = true; break; }
            if (kind != 1) continue;
            have = true;
            span(lo - 5, hi, kPlt);
            for (uint64_t i = lo; i < hi && !failed; ++i) {
                if (!t2p_plt_terminator(src, i)) continue;
                uint32_t v = 0;
                const uint32_t why = t2p_plt_entry(src, lo, i, &v);
                if (why) { report(t2p_status_tile(t, 0, 0, why)); failed = true; }
                else if (cnt >= npk) { report(t2p_status_tile(t, 0, 0, kT2pPltMany)); failed = true; }
                else plt_len[T.pkt_base + cnt++] = v;
            }
            if (!failed && hi > lo && !t2p_plt_terminator(src, hi - 1)) { report(t2p_status_tile(t, 0, 0, kT2pPltCount)); failed = true; }
        }
        if (failed) continue;
        if (!done) { report(t2p_status_tile(t, 0, 0, kT2pNoSod)); continue; }
        if (npk > end - pos) { report(t2p_status_tile(t, 0, 0, kT2pPacketsBytes)); continue; }
        if (have && cnt != npk) { report(t2p_status_tile(t, 0, 0, kT2pPltCount)); continue; }
        if (have) {
            uint64_t run = pos;
            for (uint64_t k = 0; k < npk; ++k) { pk_start[T.pkt_base + k] = run; run += plt_len[T.pkt_base + k]; }
            if (run != end) report(t2p_status_tile(t, 1, (uint32_t)npk, kT2pTail));
        }
        body_at[t] = pos; has_plt[t] = have;
    }
    // ---- KC-L: chain after chain (stale nodes, state, logs and counts: a chain clears its own)
    std::vector<uint32_t> nodes(P.node_bytes + 16, 0xAAAAAAAAu);
    std::vector<T2pRowState> state(P.rows + 1);
    std::memset(state.data(), 0xAA, state.size() * sizeof state[0]);
    std::vector<T2ReadSegRecord> seg_log(P.rows * Q.seg_records_per_row + 1, T2ReadSegRecord{0xAAAAAAAAu, 0xAAAAAAAAu, 0xAAAAAAAAu, 0xAAAAAAAAu});
    std::vector<T2ReadPieceRecord> piece_log(P.rows * Q.piece_records_per_row + 1, T2ReadPieceRecord{~0ull, 0xAAAAAAAAu, 0xAAAAAAAAu, 0xAAAAAAAAu, 0xAAAAAAAAu});
    std::vector<uint32_t> counts(2 * P.chains + 2, 0xAAAAAAAAu);
    for (uint64_t turn = 0; turn < P.chains; ++turn) {
        const uint64_t chain = reversed ? P.chains - 1 - turn : turn;
        counts[2 * chain] = counts[2 * chain + 1] = 0;
        uint32_t lo = 0, hi = nt;
        while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (P.tiles[mid].chain_base <= chain) lo = mid; else hi = mid; }
        const uint32_t t = lo;
        const T2ReadTile& T = P.tiles[t];
        if (!body_at[t]) continue;
        const uint64_t end = part_at[t] + part_len[t];
        const uint32_t np = T.npackets / L, i0 = (uint32_t)(chain - T.chain_base);
        const bool plt = has_plt[t] != 0, split = plt && T.nchains == np;
        if (!split && i0) continue;
        const T2ReadPacket* pk = P.packets.data() + T.first_packet;
        const T2ReadLayerPk* lp = Q.lpk.data() + T.first_packet;
        uint32_t* const nd = nodes.data() + T.node_base;
        T2pRowState* const st = state.data() + T.row_base;
        std::memset(nd + (split ? pk[i0].node_at : 0u), 0, 4ull * (split ? pk[i0].node_n : T.node_bytes));
        if (split) for (uint32_t bi = 0; bi < pk[i0].nbands; ++bi) std::memset(st + pk[i0].band[bi].first_row, 0, sizeof st[0] * pk[i0].band[bi].gw * pk[i0].band[bi].gh);
        else std::memset(st, 0, sizeof st[0] * T.rows);
        const uint64_t share = (uint64_t)T.row_base + (split ? lp[i0].blocks_before : 0u);
        const uint32_t share_rows = split ? pk[i0].nblocks : T.rows;
        LogSink sink{seg_log.data() + share * Q.seg_records_per_row, share_rows * Q.seg_records_per_row, 0,
                     piece_log.data() + share * Q.piece_records_per_row, share_rows * Q.piece_records_per_row, 0, false};
        uint64_t pos = body_at[t];
        bool failed = false;
        auto one = [&](uint32_t i, uint32_t l, uint32_t k) -> bool {
            if (split) pos = pk_start[T.pkt_base + k];
            const uint64_t from = pos;
            const uint32_t pieces0 = sink.npiece;
            uint64_t body = 0;
            const uint32_t why = t2p_read_packet_layer(src, pk[i], nd, st, P.ht, Q.sty, P.sop, P.eph, l, k, pos, end, sink, &body);
            if (why) { report(t2p_status_tile(t, 1, k, why)); failed = true; return false; }
            for (uint32_t j = pieces0; j < sink.npiece; ++j) {
                T2ReadPieceRecord& r = sink.pieces[j];
                r.src += body;
                if (r.ordinal == 0) { st[r.row].src_lo = (uint32_t)r.src; st[r.row].src_hi = (uint32_t)(r.src >> 32); }
            }
            if (P.sop) span(from, from + 6, kSopEph);
            if (P.eph) span(body - 2, body, kSopEph);
            span(from + (P.sop ? 6 : 0), body - (P.eph ? 2 : 0), kHeader);
            span(body, pos, kBody);
            if (plt && pos - from != plt_len[T.pkt_base + k]) { report(t2p_status_tile(t, 1, k, kT2pPltSize)); failed = true; return false; }
            return true;
        };
        if (split) {
            for (uint32_t l = 0; l < L; ++l)
                if (!one(i0, l, (uint32_t)t2p_packet_number(Q.order, np, L, i0, l, lp[i0].run_first, lp[i0].run_count))) break;
        } else {
            t2p_tile_packets(Q.order, np, L, [&](uint32_t i, uint32_t* first, uint32_t* cnt) { *first = lp[i].run_first; *cnt = lp[i].run_count; }, one);
            if (!failed && pos != end) report(t2p_status_tile(t, 1, T.npackets, kT2pTail));
        }
        if (sink.over) { std::printf("FAIL: a chain's log is full\n"); std::exit(1); }
        counts[2 * chain] = sink.nseg; counts[2 * chain + 1] = sink.npiece;
    }
    if (len) span(len - 1, len, kLast);
    if (status != kT2pNoStatus) return status;                  // (the call stops here: KF and KP run on what every chain has finished)
    // ---- KF
    out = Tables{};
    out.rows.assign(P.rows, grk_amd_coded_block{0xDEADBEEFull, 0xDEADBEEFu, 0xDEADBEEFu});
    out.first_segment.assign(P.rows + 1, 0xDEADBEEFu);
    std::vector<uint64_t> app_at(P.rows, 0);
    std::vector<uint32_t> move_first(P.rows, 0);
    uint64_t nseg = 0, app = 0, nmoves = 0;
    for (uint64_t r = 0; r < P.rows; ++r) {
        const T2pRowState& s = state[r];
        if (!t2p_finish_row(s, P.ht, &out.rows[r])) {
            uint32_t lo = 0, hi = nt;
            while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (P.tiles[mid].row_base <= r) lo = mid; else hi = mid; }
            report(t2p_status_tile(lo, 2, (uint32_t)(r - P.tiles[lo].row_base), kT2pPart1Planes));
        }
        out.first_segment[r] = (uint32_t)nseg; app_at[r] = app; move_first[r] = (uint32_t)nmoves;
        nseg += s.nsegs;
        if (s.pieces > 1) { out.rows[r].offset = len + app; app += s.total; nmoves += s.pieces; }
    }
    out.first_segment[P.rows] = (uint32_t)nseg;
    out.appendix = app;
    if (status != kT2pNoStatus) return status;
    // ---- KP: chain after chain, a chain's records from the last to the first (their order does not matter)
    out.segments.assign(nseg, grk_amd_segment{0, 0});
    out.moves.assign(nmoves, grk_amd_tp_segment{~0ull, ~0ull, 0xDEADBEEFu, 0xDEADBEEFu});
    for (uint64_t chain = 0; chain < P.chains; ++chain) {
        uint32_t lo = 0, hi = nt;
        while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (P.tiles[mid].chain_base <= chain) lo = mid; else hi = mid; }
        const T2ReadTile& T = P.tiles[lo];
        const uint32_t np = T.npackets / L, i0 = (uint32_t)(chain - T.chain_base);
        const bool split = T.nchains == np && has_plt[lo] != 0;
        const uint64_t share = (uint64_t)T.row_base + (split ? Q.lpk[T.first_packet + i0].blocks_before : 0u);
        for (uint32_t j = counts[2 * chain]; j-- > 0;) {
            const T2ReadSegRecord& r = seg_log[share * Q.seg_records_per_row + j];
            const uint64_t at = (uint64_t)out.first_segment[T.row_base + r.row] + r.ordinal;
            if (r.row >= T.rows || at >= nseg) { std::printf("FAIL: a segment record out of place\n"); std::exit(1); }
            out.segments[at].length += r.len; out.segments[at].numpasses += r.passes_opens & 0x7FFFFFFFu;
        }
        for (uint32_t j = counts[2 * chain + 1]; j-- > 0;) {
            const T2ReadPieceRecord& r = piece_log[share * Q.piece_records_per_row + j];
            if (r.row >= T.rows) { std::printf("FAIL: a piece record out of place\n"); std::exit(1); }
            if (state[T.row_base + r.row].pieces < 2) continue;
            const uint64_t at = (uint64_t)move_first[T.row_base + r.row] + r.ordinal;
            if (at >= nmoves) { std::printf("FAIL: a move out of place\n"); std::exit(1); }
            out.moves[at] = grk_amd_tp_segment{app_at[T.row_base + r.row] + r.before, r.src, r.len, 1u};
        }
    }
    return status;
}

struct Outcome { int host = 0, core = 0; bool equal = false; std::string host_err, core_err; };

bool same_tables(const Tables& a, const StreamTable& h, std::string& why)
{
    auto fail = [&](const std::string& s) { why = s; return false; };
    if (a.rows.size() != h.rows.size()) return fail("the number of rows");
    for (size_t i = 0; i < a.rows.size(); ++i)
        if (a.rows[i].offset != h.rows[i].offset || a.rows[i].length != h.rows[i].length || a.rows[i].missing_msbs != h.rows[i].missing_msbs)
            return fail("row " + std::to_string(i) + ": core {" + std::to_string(a.rows[i].offset) + ", " + std::to_string(a.rows[i].length) + ", " +
                        std::to_string(a.rows[i].missing_msbs) + "} host {" + std::to_string(h.rows[i].offset) + ", " + std::to_string(h.rows[i].length) + ", " +
                        std::to_string(h.rows[i].missing_msbs) + "}");
    if (a.first_segment != h.first_segment) return fail("first_segment");
    if (a.segments.size() != h.segments.size()) return fail("the number of segments");
    for (size_t i = 0; i < a.segments.size(); ++i)
        if (a.segments[i].length != h.segments[i].length || a.segments[i].numpasses != h.segments[i].numpasses) return fail("segment " + std::to_string(i));
    if (a.appendix != h.appendix_bytes) return fail("appendix_bytes");
    if (a.moves.size() != h.moves.size()) return fail("the number of moves");
    std::vector<grk_amd_tp_segment> x = a.moves, y = h.moves;
    auto by_dst = [](const grk_amd_tp_segment& p, const grk_amd_tp_segment& q) { return p.dst < q.dst; };
    std::sort(x.begin(), x.end(), by_dst); std::sort(y.begin(), y.end(), by_dst);
    for (size_t i = 0; i < x.size(); ++i)
        if (x[i].dst != y[i].dst || x[i].src != y[i].src || x[i].len != y[i].len || x[i].kind != y[i].kind) return fail("move " + std::to_string(i));
    return true;
}

Outcome both(const std::vector<uint8_t>& file)
{
    Outcome o;
    uint8_t* cs = (uint8_t*)std::malloc(file.size() ? file.size() : 1);
    std::memcpy(cs, file.data(), file.size());
    const uint64_t len = file.size();
    grk_amd_stream_info info;
    std::string err;
    int rc = read_stream_header(cs, len, info, err);
    if (rc) { o.host = o.core = rc; o.host_err = err; std::free(cs); return o; }          // (the header is the host's on both sides)
    StreamTable tab;
    o.host = read_stream_packets(cs, len, info, 1, tab, err);
    o.host_err = err;
    T2ReadLayersPlan Q;
    const char* why = "";
    rc = plan_t2_read_layers(info, Q, &why);
    if (rc) { o.core = rc; o.core_err = why; std::free(cs); return o; }
    o.equal = true;
    for (int reversed = 0; reversed < 2; ++reversed) {
        Tables t;
        if (!reversed) g_spans.clear();
        const bool rec = g_record; if (reversed) g_record = false;
        const uint64_t st = play(cs, len, Q, reversed != 0, t);
        g_record = rec;
        const int code = st == kT2pNoStatus ? 0 : t2p_code(t2p_status_why(st));
        if (reversed && code != o.core) { o.core_err = "the chains in falling order give another code"; o.equal = false; o.core = code ? code : -99; break; }
        o.core = code;
        if (code) { o.core_err = t2p_text(t2p_status_why(st)); o.equal = false; }
        else if (!o.host) { std::string w; if (!same_tables(t, tab, w)) { o.equal = false; o.core_err = (reversed ? "falling order: " : "") + w; } }
    }
    std::free(cs);
    return o;
}

bool bounds_ok()
{
    const uint64_t lim[6] = {kT2pThreshold, kT2pMaxLblock + 1, kT2pMaxLenBits, kT2pMaxPasses, kT2pMaxLevels, kT2pPltBytes};
    for (int i = 0; i < 6; ++i)
        if (g_max[i] > lim[i]) { std::printf("FAIL: loop %d took %llu steps (bound %llu)\n", i, (unsigned long long)g_max[i], (unsigned long long)lim[i]); return false; }
    if (g_lmax[kT2pLoopInclusion] > kT2pMaxLayers || g_lmax[kT2pLoopSegments] > kT2pMaxPasses) { std::printf("FAIL: a layer loop beyond its bound\n"); return false; }
    return true;
}

std::vector<uint8_t> read_file(const char* path)
{
    std::vector<uint8_t> f;
    std::FILE* fh = std::fopen(path, "rb");
    if (!fh) { std::printf("FAIL: %s cannot be read\n", path); std::exit(1); }
    uint8_t buf[65536];
    for (size_t n; (n = std::fread(buf, 1, sizeof buf, fh)) > 0;) f.insert(f.end(), buf, buf + n);
    std::fclose(fh);
    return f;
}
const char* base_name(const char* p) { const char* b = std::strrchr(p, '/'); return b ? b + 1 : p; }

int check_mode(int argc, char** argv)
{
    int bad = 0;
    for (int i = 2; i < argc; ++i) {
        const Outcome o = both(read_file(argv[i]));
        std::printf("%s host %d core %d tables %s\n", base_name(argv[i]), o.host, o.core, o.host == 0 && o.core == 0 ? (o.equal ? "equal" : "DIFFER") : "-");
        if (o.host != o.core || (o.host == 0 && !o.equal)) { std::printf("  host: %s\n  core: %s\n", o.host_err.c_str(), o.core_err.c_str()); bad = 1; }
    }
    if (!bounds_ok()) bad = 1;
    return bad;
}

uint64_t g_rng = 1;
uint32_t rnd() { g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(g_rng >> 33); }

int region_of(const std::vector<Span>& spans, uint64_t pos)
{
    int kind = kBody;
    for (const Span& s : spans) if (pos >= s.lo && pos < s.hi && s.kind < kind) kind = s.kind;
    for (const Span& s : spans) if (s.kind == kLast && pos >= s.lo && pos < s.hi) kind = kLast;
    return kind;
}

int sweep_mode(int argc, char** argv)
{
    uint64_t tally[kRegions] = {0}, total = 0, accepted = 0, refused = 0;
    const uint32_t files = (uint32_t)(argc - 2);
    if (!files) { std::printf("FAIL: no files\n"); return 1; }
    const uint32_t changes = std::max<uint32_t>(48, 2400 / files), cuts = changes / 4 + 1;
    for (int fi = 2; fi < argc; ++fi) {
        const std::vector<uint8_t> f = read_file(argv[fi]);
        g_record = true;
        const Outcome clean = both(f);
        g_record = false;
        if (clean.host || clean.core || !clean.equal) { std::printf("FAIL: %s: a file to corrupt is refused or differs (%s)\n", base_name(argv[fi]), clean.core_err.c_str()); return 1; }
        const std::vector<Span> spans = g_spans;
        g_rng = (uint64_t)fi * 977 + 5;
        for (uint32_t i = 0; i < changes + cuts; ++i) {
            std::vector<uint8_t> g = f;
            char what[128];
            if (i < changes) {
                uint64_t pos;
                if (i == 0) pos = f.size() - 1;
                else if ((i & 1u) && !spans.empty()) {
                    const Span* s;
                    do s = &spans[rnd() % spans.size()]; while (s->kind == kBody && (rnd() & 3u));
                    pos = s->lo + rnd() % (s->hi - s->lo);
                } else pos = rnd() % f.size();
                const uint32_t how = rnd() % 4;
                g[pos] = how == 0 ? (uint8_t)0xFF : how == 1 ? (uint8_t)(g[pos] ^ (1u << (rnd() % 8))) : how == 2 ? (uint8_t)(g[pos] + 1) : (uint8_t)rnd();
                ++tally[region_of(spans, pos)];
                std::snprintf(what, sizeof what, "%s: byte %llu %02X -> %02X", base_name(argv[fi]), (unsigned long long)pos, f[pos], g[pos]);
            } else {
                const uint64_t n = i == changes ? f.size() - 1 : rnd() % f.size();
                g.resize((size_t)n);
                std::snprintf(what, sizeof what, "%s: cut at %llu of %llu", base_name(argv[fi]), (unsigned long long)n, (unsigned long long)f.size());
            }
            const Outcome o = both(g);
            ++total;
            if (o.host == 0) ++accepted; else ++refused;
            if (o.host != o.core || (o.host == 0 && !o.equal)) {
                std::printf("FAIL: %s: host %d (%s), core %d (%s)\n", what, o.host, o.host_err.c_str(), o.core, o.core_err.c_str());
                return 1;
            }
        }
    }
    if (!bounds_ok()) return 1;
    std::printf("ok: %llu corruptions of %u files (%llu accepted with equal tables, %llu refused alike) [main %llu sot %llu plt %llu sop/eph %llu header %llu last %llu body %llu], "
                "loop maxima tree %llu lblock %llu lenbits %llu passes %llu levels %llu plt %llu inclusion %llu segments %llu\n",
                (unsigned long long)total, files, (unsigned long long)accepted, (unsigned long long)refused, (unsigned long long)tally[kMain], (unsigned long long)tally[kSot],
                (unsigned long long)tally[kPlt], (unsigned long long)tally[kSopEph], (unsigned long long)tally[kHeader], (unsigned long long)tally[kLast],
                (unsigned long long)tally[kBody], (unsigned long long)g_max[0], (unsigned long long)g_max[1], (unsigned long long)g_max[2], (unsigned long long)g_max[3],
                (unsigned long long)g_max[4], (unsigned long long)g_max[5], (unsigned long long)g_lmax[0], (unsigned long long)g_lmax[1]);
    return 0;
}

// the plan's numbers against the geometry, tile by tile
int plan_mode(int argc, char** argv)
{
    bool ok = true;
    for (int fi = 2; fi < argc; ++fi) {
        auto fail = [&](const char* what) { std::printf("FAIL: plan: %s: %s\n", base_name(argv[fi]), what); ok = false; };
        const std::vector<uint8_t> f = read_file(argv[fi]);
        grk_amd_stream_info info; std::string err;
        if (read_stream_header(f.data(), f.size(), info, err)) { fail("header"); continue; }
        T2ReadLayersPlan Q; const char* why = "";
        if (plan_t2_read_layers(info, Q, &why)) { fail(why); continue; }
        const T2ReadPlan& P = Q.base;
        const uint32_t L = info.num_layers, order = (info.flags >> GRK_AMD_CS_PROG_SHIFT) & 7u;
        const bool plt = (info.flags & GRK_AMD_CS_PLT) != 0, ht = !info.base.reserved[0];
        if (Q.layers != L || Q.order != order || Q.sty != info.base.reserved[1]) fail("layers, order or style");
        uint64_t rows = 0, packets = 0, chains = 0, nodes = 0;
        for (uint32_t t = 0; t < info.num_tiles; ++t) {
            // the tile's precincts in the order of one layer's packets, from the geometry
            grk_amd_tile_params p;
            grk_amd_layout_tile(&info.layout, &info.base, t, &p);
            std::vector<TileGeom> geoms(info.base.num_comps);
            std::vector<const TileGeom*> cg(info.base.num_comps);
            uint64_t tr = 0;
            bool sub = false;
            for (uint32_t c = 0; c < info.base.num_comps; ++c) {
                grk_amd_tile_params pc;
                grk_amd_layout_tile_comp(&info.layout, &info.base, info.comp_dx[c], info.comp_dy[c], t, &pc);
                pc.num_comps = 1; pc.mct = 0;
                if (build_tile_geom(pc, geoms[c])) fail("geometry");
                cg[c] = &geoms[c]; tr += geoms[c].blocks_per_comp;
                sub = sub || info.comp_dx[c] != 1 || info.comp_dy[c] != 1;
            }
            const std::vector<Pk> seq = packet_order(cg, sub ? info.comp_dx : nullptr, sub ? info.comp_dy : nullptr, p.tile_x0, p.tile_y0, order);
            const uint64_t np = seq.size();
            const T2ReadTile& T = P.tiles[t];
            if (T.npackets != np * L) fail("a tile's packets are not its precincts times the layers");
            if (T.rows != tr || T.row_base != rows) fail("a tile's rows");
            if (T.nchains != (plt ? np : 1) || T.chain_base != chains || T.pkt_base != packets || T.node_base != nodes) fail("a tile's chains or scratch");
            // the numbering: every (precinct, layer) once, in the order the file-order walk meets them
            std::vector<uint8_t> seen(np * L, 0);
            uint64_t blocks = 0, nn = 0, want_k = 0;
            bool walk_ok = true;
            t2p_tile_packets(order, (uint32_t)np, L, [&](uint32_t i, uint32_t* first, uint32_t* cnt) { *first = Q.lpk[T.first_packet + i].run_first; *cnt = Q.lpk[T.first_packet + i].run_count; },
                             [&](uint32_t i, uint32_t l, uint32_t k) {
                                 const T2ReadLayerPk& lp = Q.lpk[T.first_packet + i];
                                 const uint64_t num = t2p_packet_number(order, np, L, i, l, lp.run_first, lp.run_count);
                                 if (k != want_k++ || num != k || num >= np * L || seen[num]++) walk_ok = false;
                                 // brute force: the packets before it in the file
                                 uint64_t before = 0;
                                 for (uint64_t i2 = 0; i2 < np; ++i2)
                                     for (uint64_t l2 = 0; l2 < L; ++l2) {
                                         bool first;
                                         if (order == 0) first = l2 < l || (l2 == l && i2 < i);
                                         else if (order == 1) first = seq[i2].r < seq[i].r || (seq[i2].r == seq[i].r && (l2 < l || (l2 == l && i2 < i)));
                                         else first = i2 < i || (i2 == i && l2 < l);
                                         before += first;
                                     }
                                 if (before != num) walk_ok = false;
                                 return true;
                             });
            if (!walk_ok || want_k != np * L) fail("the numbering");
            for (uint64_t q = 0; q < np; ++q) {
                const T2ReadPacket& d = P.packets[T.first_packet + q];
                if (Q.lpk[T.first_packet + q].blocks_before != blocks) fail("blocks_before");
                if (d.node_at != nn) fail("a precinct's nodes do not follow the one before");
                const ResGeom& R = cg[seq[q].c]->res[seq[q].r];
                uint64_t pb = 0;
                for (uint32_t bi = 0; bi < R.num_bands; ++bi) pb += (uint64_t)R.band[bi].prec[seq[q].pi].gw * R.band[bi].prec[seq[q].pi].gh;
                for (uint32_t b = 0; b < d.nbands; ++b) { uint32_t nlev = 0, n = 0; t2p_tree_shape(d.band[b].gw, d.band[b].gh, &nlev, &n); nn += 2ull * n; }
                if (d.nblocks != pb || d.node_n != nn - d.node_at) fail("a precinct's blocks or nodes");
                blocks += pb;
            }
            if (blocks != tr || T.node_bytes < nn) fail("a tile's blocks or nodes");
            rows += tr; packets += np * L; chains += T.nchains; nodes += T.node_bytes;
        }
        if (P.rows != rows || P.rows != info.num_blocks || P.total_packets != packets || P.chains != chains || P.node_bytes != nodes) fail("totals");
        const uint32_t sty = info.base.reserved[1];
        const uint64_t pieces = ht ? 1 : std::min<uint64_t>(L, 164), maxseg = ht ? 1 : (sty & 4) ? 164 : (sty & 1) ? 104 : 1;
        const uint64_t segrec = std::min<uint64_t>(164, maxseg + pieces - 1);
        if (Q.piece_records_per_row != pieces || Q.segments_per_row != maxseg || Q.seg_records_per_row != segrec) fail("records per row");
        if (Q.bytes_nodes() != nodes * 4 || Q.bytes_state() != rows * 32 || Q.bytes_seg_log() != rows * segrec * 16 || Q.bytes_piece_log() != rows * pieces * 24 ||
            Q.bytes_counts() != chains * 8 || Q.bytes_segments() != rows * maxseg * 8 || Q.bytes_moves() != rows * pieces * 24 || P.bytes_plt() != (plt ? packets * 12 : 0))
            fail("scratch sizes");
    }
    // LAZY's segments: 10, 2, 1, 2, 1 ... hold 164 passes in 104 segments
    { uint32_t left = 164, n = 0; while (left) { const uint32_t c = t2p_seg_capacity(1, n); left -= std::min(left, c); ++n; } if (n != 104) { std::printf("FAIL: plan: LAZY segments %u\n", n); ok = false; } }
    if (ok) std::printf("ok: plan\n");
    return ok ? 0 : 1;
}

} // namespace

int main(int argc, char** argv)
{
    if (argc > 2 && !std::strcmp(argv[1], "check")) return check_mode(argc, argv);
    if (argc > 2 && !std::strcmp(argv[1], "sweep")) return sweep_mode(argc, argv);
    if (argc > 2 && !std::strcmp(argv[1], "plan")) return plan_mode(argc, argv);
    std::printf("usage: t2_parse_layers_units check|sweep|plan FILE..\n");
    return 2;
}
