// tests/c/t2_parse_ht_units.cpp -- the device Tier-2 reader of HT blocks WITH REFINEMENT PASSES played on the CPU
// (tests/test_t2_ht_refine_cpu.py builds it with -fsanitize=address,undefined; it has its own main and is not loaded into Python):
// KL-P and KH-P as tests/c/t2_parts_units.cpp plays them, KC-L over the part table with its two logs, KF and KP as
// tests/c/t2_parse_layers_units.cpp plays them -- all over t2_parse.h / t2_parse_layers.h and the plan of
// plan_t2_read_layers(.., ht_refine = true), which is what grk_amd_read_packets_device_refine launches -- against the host reader
// with the same option (read_stream_packets(.., allow_parts, ht_refine), threads = 1): rows, first_segment, segments and the
// appendix's size field for field, the moves as a set, its code where it refuses.  Every stream sits in a heap buffer of exactly its
// length, every table is a std::vector indexed with at().
//   t2_parse_ht_units check F..   "<name> host <code> core <code> tables <equal|DIFFER|->" per file (exit 1 where the two differ)
//   t2_parse_ht_units old F..     "<name> old <code> <reason>" per file: the reader WITHOUT the option (grk_amd_read_packets_parts)
//   t2_parse_ht_units sweep F..   fixed-seed single-byte changes and truncations of every file: read or refused alike
//   t2_parse_ht_units plan F..    the plan's numbers with the option: 2 segments, min(L, 3) pieces, their sum less one segment records
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../grok_amd/csrc/t2_parse.h"
#include "../../grok_amd/csrc/t2_parse_layers.h"
#include "../../grok_amd/csrc/t2_read_plan.h"
#include "../../grok_amd/csrc/t2_reader.h"

using namespace grk_amd;

namespace {

struct HeapSrc {
    const uint8_t* d; uint64_t len;
    uint32_t byte(uint64_t i) const { if (i >= len) { std::printf("FAIL: the core reads byte %llu of %llu\n", (unsigned long long)i, (unsigned long long)len); std::exit(1); } return d[i]; }
};

struct Tables {
    std::vector<grk_amd_coded_block> rows;
    std::vector<uint32_t> first_segment;
    std::vector<grk_amd_segment> segments;
    std::vector<grk_amd_tp_segment> moves;
    uint64_t appendix = 0;
};

// a chain's share of the two logs, as KC-L's LogSink fills it
struct LogSink {
    T2ReadSegRecord* segs; uint32_t seg_cap, nseg;
    T2ReadPieceRecord* pieces; uint32_t piece_cap, npiece;
    bool over;
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

// the kernels in turn over the plan Q (made with the option); the status word as the call would read it
uint64_t play(const uint8_t* cs, uint64_t len, const T2ReadLayersPlan& Q, bool reversed, Tables& out)
{
    const T2ReadPlan& P = Q.base;
    const uint32_t nt = P.num_tiles, L = Q.layers;
    HeapSrc src{cs, len};
    uint64_t status = kT2pNoStatus;
    auto report = [&](uint64_t w) { status = std::min(status, w); };
    // the host's share: TLM's places, where the first SOT lies
    bool tlm = false;
    std::vector<uint64_t> at; std::vector<uint32_t> ln, idx;
    uint64_t count = 0, sot_at = 2;
    if (t2_read_tlm(cs, len, len, kT2pMaxPartsOfFile, &tlm, at, ln, idx, &count)) return t2p_status_locate(0, kT2pNotLocated);
    if (tlm && count > kT2pMaxPartsOfFile) return t2p_status_locate(0, kT2pPartsOfFile);
    while (sot_at + 4 <= len && !(cs[sot_at] == 0xFF && cs[sot_at + 1] == 0x90)) sot_at += 2 + ((uint64_t)cs[sot_at + 2] << 8 | cs[sot_at + 3]);
    const uint32_t cap = (uint32_t)(tlm ? std::max<uint64_t>(count, 1) : std::min<uint64_t>(len / 14 + 1, kT2pMaxPartsOfFile));
    std::vector<unsigned long long> fo_at(cap), tp_at(cap), tp_body(cap), body_at(nt), pk_start(std::max<uint64_t>(P.total_packets, nt));
    std::vector<uint32_t> fo_len(cap), fo_idx(cap, 0xFFFFFFFFu), claim(cap, 0xFFFFFFFFu), tp_len(cap), tp_tile(cap), tp_file(cap), tp_has_plt(cap), tp_npk(cap), tp_first(cap);
    std::vector<uint32_t> cnt(nt), tn_min(nt, 0xFFFFFFFFu), tn_max(nt), slice(nt + 1), has_plt(nt), plt_len(std::max<uint64_t>(P.total_packets, nt));
    // ---- KL-P
    uint32_t n = 0;
    if (tlm) { n = (uint32_t)count; if (at.size() != count) return t2p_status_locate(0, kT2pNotLocated); for (uint32_t i = 0; i < n; ++i) { fo_at.at(i) = at.at(i); fo_len.at(i) = ln.at(i); fo_idx.at(i) = idx.at(i); } }
    else {
        uint64_t pos = sot_at;
        uint32_t fail = 0;
        for (uint32_t hop = 0; hop <= cap; ++hop) {
            uint64_t l = 0;
            const int r = t2p_hop(src, len, pos, &l);
            if (r == 0) break;
            if (r == 2) { fail = kT2pNotLocated; break; }
            if (n == cap) { fail = kT2pPartsOfFile; break; }
            fo_at.at(n) = pos; fo_len.at(n) = (uint32_t)l; ++n; pos += l;
        }
        if (!n && !fail) fail = kT2pNotLocated;
        if (fail) return t2p_status_locate(n, fail);
    }
    auto sot = [&](uint32_t i, uint32_t* isot, uint32_t* tps, uint32_t* tn) { return t2p_check_sot_part(src, len, fo_at.at(i), fo_len.at(i), nt, fo_idx.at(i), i + 1 == n, isot, tps, tn); };
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t isot = 0, tps = 0, tn = 0;
        const uint32_t w = sot(i, &isot, &tps, &tn);
        if (w) { report(t2p_status_locate(i, w)); continue; }
        ++cnt.at(isot);
        if (tn) { tn_min.at(isot) = std::min(tn_min.at(isot), tn); tn_max.at(isot) = std::max(tn_max.at(isot), tn); }
    }
    for (uint32_t t = 0; t < nt; ++t) slice.at(t + 1) = slice.at(t) + cnt.at(t);
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t isot = 0, tps = 0, tn = 0;
        if (sot(i, &isot, &tps, &tn)) continue;
        if (tps < cnt.at(isot) && slice.at(isot) + tps < cap) claim.at(slice.at(isot) + tps) = std::min(claim.at(slice.at(isot) + tps), i);
    }
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t isot = 0, tps = 0, tn = 0;
        if (sot(i, &isot, &tps, &tn)) continue;
        const uint32_t c = cnt.at(isot), mn = tn_min.at(isot), mx = tn_max.at(isot), slot = slice.at(isot) + tps;
        uint32_t w = kT2pOk;
        if (c > kT2pMaxPartsOfTile && tps >= kT2pMaxPartsOfTile) w = kT2pPartsOfTile;
        else if (tps >= c || slot >= cap || claim.at(slot) != i) w = kT2pTpsot;
        else if ((tn && mn != mx) || (mx && mx <= tps)) w = kT2pTnsot;
        if (w) { report(t2p_status_locate(i, w)); continue; }
        tp_at.at(slot) = fo_at.at(i); tp_len.at(slot) = fo_len.at(i); tp_tile.at(slot) = isot; tp_file.at(slot) = i;
    }
    for (uint32_t j = 0; j + 1 < n; ++j) {
        if (claim.at(j) == 0xFFFFFFFFu || claim.at(j + 1) == 0xFFFFFFFFu) continue;
        if (tp_len.at(j) && tp_len.at(j + 1) && tp_tile.at(j) == tp_tile.at(j + 1) && tp_file.at(j + 1) < tp_file.at(j)) report(t2p_status_locate(tp_file.at(j + 1), kT2pTpsot));
    }
    for (uint32_t t = 0; t < nt; ++t) {
        if (!cnt.at(t)) report(t2p_status_locate(n + 1 + t, kT2pNoPart));
        else if (tn_max.at(t) > cnt.at(t)) report(t2p_status_locate(n + 1 + t, kT2pTnsot));
    }
    if (status != kT2pNoStatus) return status;                // (the host stops here: KH-P's grid needs the located count)
    // ---- KH-P, first step: a tile-part's header
    auto walk = [&](uint32_t j, uint64_t* body, bool* have, uint64_t* entries, auto fn) -> uint32_t {
        const uint64_t end = tp_at.at(j) + tp_len.at(j);
        uint64_t pos = tp_at.at(j) + 12, k = 0;
        int kind = 2;
        *have = false;
        for (uint32_t hop = 0, hops = tp_len.at(j) / 4 + 2; hop < hops; ++hop) {
            uint64_t next = 0, lo = 0, hi = 0;
            kind = t2p_header_segment(src, pos, end, &next, &lo, &hi);
            if (kind < 0) return (uint32_t)-kind;
            pos = next;
            if (kind == 0) break;
            if (kind != 1) continue;
            *have = true;
            for (uint64_t i = lo; i < hi; ++i)
                if (t2p_plt_terminator(src, i)) {
                    uint32_t v = 0;
                    const uint32_t w = t2p_plt_entry(src, lo, i, &v);
                    if (w) return w;
                    fn(k, v); ++k;
                }
            if (hi > lo && !t2p_plt_terminator(src, hi - 1)) return kT2pPltCount;
        }
        if (kind != 0) return kT2pNoSod;
        *body = pos; *entries = k;
        return kT2pOk;
    };
    for (uint32_t j = 0; j < n; ++j) {
        if (!tp_len.at(j)) continue;
        const uint32_t t = tp_tile.at(j);
        uint64_t body = 0, k = 0; bool have = false;
        uint32_t w = walk(j, &body, &have, &k, [](uint64_t, uint32_t) {});
        if (!w && k > P.tiles.at(t).npackets) w = kT2pPltMany;
        if (w) { report(t2p_status_tile(t, 0, j - slice.at(t), w)); continue; }
        tp_body.at(j) = body; tp_has_plt.at(j) = have; tp_npk.at(j) = (uint32_t)k;
    }
    // ---- KH-P, second step: a tile over its tile-parts
    for (uint32_t t = 0; t < nt; ++t) {
        const uint32_t j0 = slice.at(t), np = slice.at(t + 1) - j0;
        const T2ReadTile& T = P.tiles.at(t);
        if (!np || np > kT2pMaxPartsOfTile) continue;
        uint64_t all = 0, room = 0; bool bad = false, any = false, missing = false;
        for (uint32_t q = 0; q < np; ++q) {
            const uint32_t j = j0 + q;
            if (!tp_body.at(j)) { bad = true; continue; }
            const uint64_t bytes = tp_at.at(j) + tp_len.at(j) - tp_body.at(j);
            tp_first.at(j) = T.pkt_base + (uint32_t)all;
            all += tp_npk.at(j); room += bytes;
            any = any || tp_has_plt.at(j); missing = missing || (bytes && !tp_has_plt.at(j));
        }
        if (bad) continue;
        if (all > T.npackets) { report(t2p_status_tile(t, 0, 0, kT2pPltMany)); continue; }
        if (T.npackets > room) { report(t2p_status_tile(t, 0, 0, kT2pPacketsBytes)); continue; }
        const bool plt_tile = np == 1 ? tp_has_plt.at(j0) != 0 : (any && !missing);
        if (plt_tile && all != T.npackets) { report(t2p_status_tile(t, 0, 0, kT2pPltCount)); continue; }
        for (uint32_t q = 0; q < np; ++q) {
            const uint32_t j = j0 + q;
            if (!tp_has_plt.at(j)) continue;
            uint64_t body = 0, k = 0; bool have = false;
            (void)walk(j, &body, &have, &k, [&](uint64_t e, uint32_t v) { if (e < tp_npk.at(j)) plt_len.at(tp_first.at(j) + e) = v; });
            if (!plt_tile) continue;
            uint64_t run = tp_body.at(j);
            for (uint32_t e = 0; e < tp_npk.at(j); ++e) { pk_start.at(tp_first.at(j) + e) = run; run += plt_len.at(tp_first.at(j) + e); }
            if (run != tp_at.at(j) + tp_len.at(j)) report(t2p_status_tile(t, 0, q, kT2pPartPlt));
        }
        body_at.at(t) = tp_body.at(j0); has_plt.at(t) = plt_tile;
    }
    // ---- KC-L over the part table: chain after chain (stale nodes, state, logs and counts: a chain clears its own)
    std::vector<uint32_t> nodes(P.node_bytes + 16, 0xAAAAAAAAu);
    std::vector<T2pRowState> state(P.rows + 1);
    std::memset(state.data(), 0xAA, state.size() * sizeof state[0]);
    std::vector<T2ReadSegRecord> seg_log(P.rows * Q.seg_records_per_row + 1, T2ReadSegRecord{0xAAAAAAAAu, 0xAAAAAAAAu, 0xAAAAAAAAu, 0xAAAAAAAAu});
    std::vector<T2ReadPieceRecord> piece_log(P.rows * Q.piece_records_per_row + 1, T2ReadPieceRecord{~0ull, 0xAAAAAAAAu, 0xAAAAAAAAu, 0xAAAAAAAAu, 0xAAAAAAAAu});
    std::vector<uint32_t> counts(2 * P.chains + 2, 0xAAAAAAAAu);
    for (uint64_t turn = 0; turn < P.chains; ++turn) {
        const uint64_t chain = reversed ? P.chains - 1 - turn : turn;
        counts.at(2 * chain) = counts.at(2 * chain + 1) = 0;
        uint32_t lo = 0, hi = nt;
        while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (P.tiles.at(mid).chain_base <= chain) lo = mid; else hi = mid; }
        const uint32_t t = lo;
        const T2ReadTile& T = P.tiles.at(t);
        if (!body_at.at(t)) continue;
        const uint32_t j0 = slice.at(t), nparts = slice.at(t + 1) - j0;
        const T2pParts PT{tp_at.data() + j0, tp_len.data() + j0, tp_body.data() + j0, tp_has_plt.data() + j0, tp_npk.data() + j0, tp_first.data() + j0, nparts};
        const uint32_t np = T.npackets / L, i0 = (uint32_t)(chain - T.chain_base);
        const bool split = has_plt.at(t) && T.nchains == np;
        if (!split && i0) continue;
        const T2ReadPacket* const pk = P.packets.data() + T.first_packet;
        const T2ReadLayerPk* const lp = Q.lpk.data() + T.first_packet;
        uint32_t* const nd = nodes.data() + T.node_base;
        T2pRowState* const st = state.data() + T.row_base;
        std::memset(nd + (split ? pk[i0].node_at : 0u), 0, 4ull * (split ? pk[i0].node_n : T.node_bytes));
        if (split) for (uint32_t bi = 0; bi < pk[i0].nbands; ++bi) std::memset(st + pk[i0].band[bi].first_row, 0, sizeof st[0] * pk[i0].band[bi].gw * pk[i0].band[bi].gh);
        else std::memset(st, 0, sizeof st[0] * T.rows);
        const uint64_t share = (uint64_t)T.row_base + (split ? lp[i0].blocks_before : 0u);
        const uint32_t share_rows = split ? pk[i0].nblocks : T.rows;
        LogSink sink{seg_log.data() + share * Q.seg_records_per_row, share_rows * Q.seg_records_per_row, 0,
                     piece_log.data() + share * Q.piece_records_per_row, share_rows * Q.piece_records_per_row, 0, false};
        T2pPartWalk w{0, 0, 0};
        uint64_t pos = 0;
        t2p_part_walk_start(PT, w, pos);
        bool failed = false;
        auto refuse = [&](uint32_t k, uint32_t y) { report(t2p_status_tile(t, 1, k, y)); failed = true; return false; };
        auto one = [&](uint32_t i, uint32_t l, uint32_t k) -> bool {
            uint64_t end = 0;
            if (split) { pos = pk_start.at(T.pkt_base + k); end = t2p_part_end(PT, t2p_part_of(PT, pos)); }
            else { const uint32_t y = t2p_part_step(PT, w, pos); if (y) return refuse(k, y); end = w.end; }
            if (end > len) { std::printf("FAIL: a tile-part's end outside the stream\n"); std::exit(1); }
            const uint64_t from = pos;
            const uint32_t pieces0 = sink.npiece;
            uint64_t body = 0;
            const uint32_t y = t2p_read_packet_layer(src, pk[i], nd, st, P.ht, Q.sty, P.sop, P.eph, l, k, pos, end, sink, &body);
            if (y) return refuse(k, y);
            for (uint32_t j = pieces0; j < sink.npiece; ++j) {
                T2ReadPieceRecord& r = sink.pieces[j];
                r.src += body;
                if (r.ordinal == 0) { st[r.row].src_lo = (uint32_t)r.src; st[r.row].src_hi = (uint32_t)(r.src >> 32); }
            }
            if (split) { if (pos - from != plt_len.at(T.pkt_base + k)) return refuse(k, kT2pPltSize); }
            else { const uint32_t z = t2p_part_packet(PT, w, plt_len.data(), pos - from); if (z) return refuse(k, z); }
            return true;
        };
        if (split) {
            for (uint32_t l = 0; l < L; ++l)
                if (!one(i0, l, (uint32_t)t2p_packet_number(Q.order, np, L, i0, l, lp[i0].run_first, lp[i0].run_count))) break;
        } else {
            t2p_tile_packets(Q.order, np, L, [&](uint32_t i, uint32_t* first, uint32_t* c) { *first = lp[i].run_first; *c = lp[i].run_count; }, one);
            if (!failed) { const uint32_t y = t2p_part_finish(PT, w, pos); if (y) refuse(T.npackets, y); }
        }
        if (sink.over) { std::printf("FAIL: a chain's log is full (the plan's records per row do not hold what the core logs)\n"); std::exit(1); }
        counts.at(2 * chain) = sink.nseg; counts.at(2 * chain + 1) = sink.npiece;
    }
    if (status != kT2pNoStatus) return status;                  // (the call stops here: KF and KP run on what every chain has finished)
    // ---- KF
    out = Tables{};
    out.rows.assign(P.rows, grk_amd_coded_block{0xDEADBEEFull, 0xDEADBEEFu, 0xDEADBEEFu});
    out.first_segment.assign(P.rows + 1, 0xDEADBEEFu);
    std::vector<uint64_t> app_at(P.rows, 0);
    std::vector<uint32_t> move_first(P.rows, 0);
    uint64_t nseg = 0, app = 0, nmoves = 0;
    for (uint64_t r = 0; r < P.rows; ++r) {
        const T2pRowState& s = state.at(r);
        if (!t2p_finish_row(s, P.ht, &out.rows.at(r))) report(t2p_status_tile(0, 2, (uint32_t)r, kT2pPart1Planes));
        if (s.nsegs > Q.segments_per_row || s.pieces > Q.piece_records_per_row) { std::printf("FAIL: row %llu has %u segments in %u pieces\n", (unsigned long long)r, s.nsegs, s.pieces); std::exit(1); }
        out.first_segment.at(r) = (uint32_t)nseg; app_at.at(r) = app; move_first.at(r) = (uint32_t)nmoves;
        nseg += s.nsegs;
        if (s.pieces > 1) { out.rows.at(r).offset = len + app; app += s.total; nmoves += s.pieces; }
    }
    out.first_segment.at(P.rows) = (uint32_t)nseg;
    out.appendix = app;
    if (status != kT2pNoStatus) return status;
    // ---- KP: chain after chain, a chain's records from the last to the first (their order does not matter)
    out.segments.assign(nseg, grk_amd_segment{0, 0});
    out.moves.assign(nmoves, grk_amd_tp_segment{~0ull, ~0ull, 0xDEADBEEFu, 0xDEADBEEFu});
    for (uint64_t chain = 0; chain < P.chains; ++chain) {
        uint32_t lo = 0, hi = nt;
        while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (P.tiles.at(mid).chain_base <= chain) lo = mid; else hi = mid; }
        const T2ReadTile& T = P.tiles.at(lo);
        const uint32_t np = T.npackets / L, i0 = (uint32_t)(chain - T.chain_base);
        const bool split = T.nchains == np && has_plt.at(lo) != 0;
        const uint64_t share = (uint64_t)T.row_base + (split ? Q.lpk.at(T.first_packet + i0).blocks_before : 0u);
        for (uint32_t j = counts.at(2 * chain); j-- > 0;) {
            const T2ReadSegRecord& r = seg_log.at(share * Q.seg_records_per_row + j);
            if (r.row >= T.rows) { std::printf("FAIL: a segment record out of place\n"); std::exit(1); }
            const uint64_t at = (uint64_t)out.first_segment.at(T.row_base + r.row) + r.ordinal;
            if (at >= nseg) { std::printf("FAIL: a segment record out of place\n"); std::exit(1); }
            out.segments.at(at).length += r.len; out.segments.at(at).numpasses += r.passes_opens & 0x7FFFFFFFu;
        }
        for (uint32_t j = counts.at(2 * chain + 1); j-- > 0;) {
            const T2ReadPieceRecord& r = piece_log.at(share * Q.piece_records_per_row + j);
            if (r.row >= T.rows) { std::printf("FAIL: a piece record out of place\n"); std::exit(1); }
            if (state.at(T.row_base + r.row).pieces < 2) continue;
            const uint64_t at = (uint64_t)move_first.at(T.row_base + r.row) + r.ordinal;
            if (at >= nmoves) { std::printf("FAIL: a move out of place\n"); std::exit(1); }
            out.moves.at(at) = grk_amd_tp_segment{app_at.at(T.row_base + r.row) + r.before, r.src, r.len, 1u};
        }
    }
    return status;
}

struct Outcome { int host = 0, core = 0; bool equal = false; std::string host_err, core_err; };

bool same_tables(const Tables& a, const StreamTable& h, uint64_t len, std::string& why)
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
    // what the HT block decoder is handed: one or two segments per block, 1 pass and then 1 or 2, their bytes the row's
    for (size_t i = 0; i + 1 < h.first_segment.size(); ++i) {
        const uint32_t s0 = h.first_segment[i], ns = h.first_segment[i + 1] - s0;
        uint64_t sum = 0;
        for (uint32_t k = 0; k < ns; ++k) sum += h.segments[s0 + k].length;
        if (ns > 2 || sum != h.rows[i].length || (ns >= 1 && h.segments[s0].numpasses != 1) || (ns == 2 && (h.segments[s0 + 1].numpasses < 1 || h.segments[s0 + 1].numpasses > 2)))
            return fail("row " + std::to_string(i) + ": not an HT block's segments");
    }
    if (a.appendix != h.appendix_bytes) return fail("appendix_bytes");
    if (a.moves.size() != h.moves.size()) return fail("the number of moves");
    std::vector<grk_amd_tp_segment> x = a.moves, y = h.moves;
    auto by_dst = [](const grk_amd_tp_segment& p, const grk_amd_tp_segment& q) { return p.dst < q.dst; };
    std::sort(x.begin(), x.end(), by_dst); std::sort(y.begin(), y.end(), by_dst);
    for (size_t i = 0; i < x.size(); ++i)
        if (x[i].dst != y[i].dst || x[i].src != y[i].src || x[i].len != y[i].len || x[i].kind != y[i].kind || x[i].src > len || x[i].len > len - x[i].src)
            return fail("move " + std::to_string(i));
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
    o.host = read_stream_packets(cs, len, info, 1, tab, err, true, true);
    o.host_err = err;
    T2ReadLayersPlan Q;
    const char* why = "";
    rc = plan_t2_read_layers(info, Q, &why, true);
    if (rc) { o.core = rc; o.core_err = why; std::free(cs); return o; }
    o.equal = true;
    for (int reversed = 0; reversed < 2; ++reversed) {
        Tables t;
        const uint64_t st = play(cs, len, Q, reversed != 0, t);
        const int code = st == kT2pNoStatus ? 0 : t2p_code(t2p_status_why(st));
        if (reversed && code != o.core) { o.core_err = "the chains in falling order give another code"; o.equal = false; o.core = code ? code : -99; break; }
        o.core = code;
        if (code) { o.core_err = t2p_text(t2p_status_why(st)); o.equal = false; }
        else if (!o.host) { std::string w; if (!same_tables(t, tab, len, w)) { o.equal = false; o.core_err = (reversed ? "falling order: " : "") + w; } }
    }
    std::free(cs);
    return o;
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
        if (o.host) std::printf("  host: %s\n  core: %s\n", o.host_err.c_str(), o.core_err.c_str());
        if (o.host != o.core || (o.host == 0 && !o.equal)) { std::printf("  host: %s\n  core: %s\n", o.host_err.c_str(), o.core_err.c_str()); bad = 1; }
    }
    return bad;
}

int old_mode(int argc, char** argv)
{
    for (int i = 2; i < argc; ++i) {
        const std::vector<uint8_t> f = read_file(argv[i]);
        grk_amd_stream_info info;
        std::string err;
        StreamTable tab;
        int rc = read_stream_header(f.data(), f.size(), info, err);
        if (!rc) rc = read_stream_packets(f.data(), f.size(), info, 1, tab, err, true, false);
        std::printf("%s old %d %s\n", base_name(argv[i]), rc, err.c_str());
    }
    return 0;
}

uint64_t g_rng = 1;
uint32_t rnd() { g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(g_rng >> 33); }

int sweep_mode(int argc, char** argv)
{
    uint64_t total = 0, accepted = 0, refused = 0, unsupported = 0;
    const uint32_t files = (uint32_t)(argc - 2);
    const uint32_t changes = std::max<uint32_t>(48, 2400 / files), cuts = changes / 4 + 1;
    for (int fi = 2; fi < argc; ++fi) {
        const std::vector<uint8_t> f = read_file(argv[fi]);
        const Outcome clean = both(f);
        if (clean.host || clean.core || !clean.equal) { std::printf("FAIL: %s: a file to corrupt is refused or differs (%s)\n", base_name(argv[fi]), clean.core_err.c_str()); return 1; }
        // where the tile-parts begin: half of the changes fall behind the main header, where the packet headers lie
        size_t sot = 2;
        while (sot + 4 <= f.size() && !(f[sot] == 0xFF && f[sot + 1] == 0x90)) sot += 2 + ((size_t)f[sot + 2] << 8 | f[sot + 3]);
        if (sot >= f.size()) sot = 0;
        g_rng = (uint64_t)fi * 977 + 5;
        for (uint32_t i = 0; i < changes + cuts; ++i) {
            std::vector<uint8_t> g = f;
            char what[128];
            if (i < changes) {
                const uint64_t pos = i == 0 ? f.size() - 1 : (i & 1u) ? sot + rnd() % (f.size() - sot) : rnd() % f.size();
                const uint32_t how = rnd() % 4;
                g[pos] = how == 0 ? (uint8_t)0xFF : how == 1 ? (uint8_t)(g[pos] ^ (1u << (rnd() % 8))) : how == 2 ? (uint8_t)(g[pos] + 1) : (uint8_t)rnd();
                std::snprintf(what, sizeof what, "%s: byte %llu %02X -> %02X", base_name(argv[fi]), (unsigned long long)pos, f[pos], g[pos]);
            } else {
                const uint64_t n = i == changes ? f.size() - 1 : rnd() % f.size();
                g.resize((size_t)n);
                std::snprintf(what, sizeof what, "%s: cut at %llu of %llu", base_name(argv[fi]), (unsigned long long)n, (unsigned long long)f.size());
            }
            const Outcome o = both(g);
            ++total;
            if (o.host == 0) ++accepted; else ++refused;
            if (o.host == GRK_AMD_ERR_UNSUPPORTED) ++unsupported;
            if (o.host != o.core || (o.host == 0 && !o.equal)) {
                std::printf("FAIL: %s: host %d (%s), core %d (%s)\n", what, o.host, o.host_err.c_str(), o.core, o.core_err.c_str());
                return 1;
            }
        }
    }
    std::printf("ok: %llu corruptions of %u files ( %llu accepted with equal tables, %llu refused alike, %llu unsupported among them )\n", (unsigned long long)total, files,
                (unsigned long long)accepted, (unsigned long long)refused, (unsigned long long)unsupported);
    return 0;
}

int plan_mode(int argc, char** argv)
{
    bool ok = true;
    for (int fi = 2; fi < argc; ++fi) {
        auto fail = [&](const char* what) { std::printf("FAIL: plan: %s: %s\n", base_name(argv[fi]), what); ok = false; };
        const std::vector<uint8_t> f = read_file(argv[fi]);
        grk_amd_stream_info info; std::string err;
        if (read_stream_header(f.data(), f.size(), info, err)) { fail("header"); continue; }
        if (info.base.reserved[0]) { fail("not an HT file"); continue; }
        T2ReadLayersPlan Q, Q0; const char* why = "";
        if (plan_t2_read_layers(info, Q, &why, true) || plan_t2_read_layers(info, Q0, &why)) { fail(why); continue; }
        const uint64_t L = info.num_layers, rows = info.num_blocks, pieces = std::min<uint64_t>(L, 3), segs = 2, segrec = segs + pieces - 1;
        if (!(Q.sty & kT2pStyHtRefine) || (Q.sty & 0xFFu) != info.base.reserved[1] || Q.layers != L) fail("the style word");
        if (Q.segments_per_row != segs || Q.piece_records_per_row != pieces || Q.seg_records_per_row != segrec) fail("records per row");
        if (Q.bytes_state() != rows * 32 || Q.bytes_seg_log() != rows * segrec * 16 || Q.bytes_piece_log() != rows * pieces * 24 || Q.bytes_segments() != rows * segs * 8 ||
            Q.bytes_moves() != rows * pieces * 24)
            fail("scratch sizes");
        // without the option: what it always was
        if (Q0.sty != info.base.reserved[1] || Q0.segments_per_row != 1 || Q0.piece_records_per_row != 1 || Q0.seg_records_per_row != 1) fail("the plan without the option");
        if (Q.base.rows != Q0.base.rows || Q.base.chains != Q0.base.chains || Q.base.total_packets != Q0.base.total_packets || Q.base.node_bytes != Q0.base.node_bytes) fail("the base plan");
    }
    // the functions the plan stands on; a Part-1 style word is not touched by the bit
    if (t2p_max_segments(true, kT2pStyHtRefine) != 2 || t2p_max_segments(true, 0) != 1 || t2p_max_segments(false, 0x04u | kT2pStyHtRefine) != kT2pMaxPasses) { std::printf("FAIL: plan: t2p_max_segments\n"); ok = false; }
    for (uint32_t L = 1; L < 6; ++L)
        if (t2p_max_piece_records_sty(true, kT2pStyHtRefine, L) != std::min(L, 3u) || t2p_max_piece_records_sty(true, 0, L) != 1 || t2p_max_piece_records(true, L) != 1 ||
            t2p_max_seg_records(true, kT2pStyHtRefine, L) != 2 + std::min(L, 3u) - 1 || t2p_max_seg_records(true, 0, L) != 1) { std::printf("FAIL: plan: records of %u layers\n", L); ok = false; }
    // an HT set: segments of 1 and 2 passes hold its three passes; the row state's fields hold what they carry
    if (t2p_ht_seg_capacity(kT2pStyHtRefine, 0) != 1 || t2p_ht_seg_capacity(kT2pStyHtRefine, 1) != 2 || t2p_ht_seg_capacity(0, 1) != 1) { std::printf("FAIL: plan: capacities\n"); ok = false; }
    static_assert(sizeof(T2pRowState) == 32, "eight words");
    if (ok) std::printf("ok: plan\n");
    return ok ? 0 : 1;
}

} // namespace

int main(int argc, char** argv)
{
    if (argc > 2 && !std::strcmp(argv[1], "check")) return check_mode(argc, argv);
    if (argc > 2 && !std::strcmp(argv[1], "old")) return old_mode(argc, argv);
    if (argc > 2 && !std::strcmp(argv[1], "sweep")) return sweep_mode(argc, argv);
    if (argc > 2 && !std::strcmp(argv[1], "plan")) return plan_mode(argc, argv);
    std::printf("usage: t2_parse_ht_units check|old|sweep|plan FILE..\n");
    return 2;
}
