// tests/c/t2_parts_units.cpp -- the reader of tile-part-divided codestreams (t2_reader.cpp: locate_stream_parts, read_stream_packets
// with allow_parts) as a stand-alone program for AddressSanitizer and UBSan (tests/test_tile_parts_cpu.py builds and runs it).
// Every stream lies in a heap buffer of exactly its length, so a read one byte outside [cs, cs + len) is reported.
//
//   t2_parts_units read FILE...        per file one line: "<file> <code> <rows> <segments> <moves> <appendix> <fnv of the table>" read on
//                                      one thread, and the same table demanded of four threads; a refusal prints its code and reason
//   t2_parts_units play FILE...        KL-P, KH-P and KC-L's part stepping of kernels_t2read.hip played on one thread from the shared headers
//                                      (t2_parse.h, t2_parse_layers.h; every table a std::vector indexed with at(), the stream read
//                                      through a source that aborts outside it): the rows must be the host reader's, a refusal its code
//   t2_parts_units prefixes FILE...    every prefix of the file, and the file with every byte of its tile-part headers (SOT to SOD)
//                                      changed in turn, through the reader: it may read or refuse, "<file> <read> <refused>"
#include "../../grok_amd/csrc/t2_reader.h"
#include "../../grok_amd/csrc/t2_read_plan.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

using namespace grk_amd;

namespace {

std::unique_ptr<uint8_t[]> exact(const uint8_t* d, size_t n)
{
    std::unique_ptr<uint8_t[]> p(new uint8_t[n ? n : 1]);
    if (n) std::memcpy(p.get(), d, n);
    return p;
}

std::vector<uint8_t> slurp(const char* path)
{
    std::vector<uint8_t> v;
    FILE* f = std::fopen(path, "rb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", path); std::exit(2); }
    uint8_t buf[65536];
    for (size_t n; (n = std::fread(buf, 1, sizeof buf, f)) > 0;) v.insert(v.end(), buf, buf + n);
    std::fclose(f);
    return v;
}

uint64_t fnv(uint64_t h, const void* p, size_t n)
{
    const uint8_t* b = (const uint8_t*)p;
    for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 1099511628211ull;
    return h;
}

int read_all(const uint8_t* cs, uint64_t len, uint32_t threads, StreamTable& tab, std::string& err)
{
    grk_amd_stream_info info;
    const int rc = read_stream_header(cs, len, info, err);
    if (rc) return rc;
    return read_stream_packets(cs, len, info, threads, tab, err, true);
}

uint64_t table_hash(const StreamTable& t, uint64_t len)
{
    uint64_t h = 1469598103934665603ull;
    for (const grk_amd_coded_block& r : t.rows) { h = fnv(h, &r.offset, sizeof r.offset); h = fnv(h, &r.length, sizeof r.length); h = fnv(h, &r.missing_msbs, sizeof r.missing_msbs); }
    if (!t.first_segment.empty()) h = fnv(h, t.first_segment.data(), t.first_segment.size() * sizeof t.first_segment[0]);
    for (const grk_amd_segment& s : t.segments) { h = fnv(h, &s.length, sizeof s.length); h = fnv(h, &s.numpasses, sizeof s.numpasses); }
    for (const grk_amd_tp_segment& m : t.moves) {
        if (m.src > len || m.len > len - m.src) { std::printf("a move's source outside the stream\n"); std::exit(1); }
        h = fnv(h, &m.dst, sizeof m.dst); h = fnv(h, &m.src, sizeof m.src); h = fnv(h, &m.len, sizeof m.len);
    }
    return fnv(h, &t.appendix_bytes, sizeof t.appendix_bytes);
}

int cmd_read(const char* path)
{
    const std::vector<uint8_t> v = slurp(path);
    const auto cs = exact(v.data(), v.size());
    StreamTable a, b;
    std::string ea, eb;
    const int ra = read_all(cs.get(), v.size(), 1, a, ea), rb = read_all(cs.get(), v.size(), 4, b, eb);
    if (ra != rb) { std::printf("%s: %d on one thread, %d on four\n", path, ra, rb); return 1; }
    if (ra) { std::printf("%s %d %s\n", path, ra, ea.c_str()); return 0; }
    for (const grk_amd_coded_block& r : a.rows)
        if (r.length && r.offset < v.size() && r.length > v.size() - r.offset) { std::printf("%s: a row outside the stream\n", path); return 1; }
    const uint64_t ha = table_hash(a, v.size()), hb = table_hash(b, v.size());
    if (ha != hb) { std::printf("%s: the tables of one and of four threads differ\n", path); return 1; }
    std::printf("%s 0 %zu %zu %zu %llu %016llx\n", path, a.rows.size(), a.segments.size(), a.moves.size(), (unsigned long long)a.appendix_bytes, (unsigned long long)ha);
    return 0;
}


// ---- the kernels on one thread -------------------------------------------------------------------------------------------------------
struct PlaySrc {
    const uint8_t* d; uint64_t n;
    uint32_t byte(uint64_t i) const { if (i >= n) { std::printf("a read outside the stream at %llu of %llu\n", (unsigned long long)i, (unsigned long long)n); std::abort(); } return d[i]; }
};
struct PlaySink {
    struct Piece { uint32_t row, ordinal; uint64_t rel; };
    std::vector<Piece> pieces;
    void seg(uint32_t, uint32_t, uint32_t, uint32_t, bool) {}
    void piece(uint32_t row, uint32_t ordinal, uint64_t rel, uint32_t, uint32_t) { pieces.push_back(Piece{row, ordinal, rel}); }
};

// 0 and the rows, or the refusal's code
int play(const uint8_t* cs, uint64_t len, std::vector<grk_amd_coded_block>& rows, std::string& err)
{
    grk_amd_stream_info info;
    int rc = read_stream_header(cs, len, info, err);
    if (rc) return rc;
    T2ReadLayersPlan Q;
    const char* why = "";
    rc = plan_t2_read_layers(info, Q, &why);
    if (rc) { err = why; return rc; }
    const T2ReadPlan& P = Q.base;
    const uint32_t nt = P.num_tiles;
    PlaySrc src{cs, len};
    uint64_t status = kT2pNoStatus;
    auto report = [&](uint64_t w) { status = std::min(status, w); };
    auto refused = [&]() { err = t2p_text(t2p_status_why(status)); return t2p_code(t2p_status_why(status)); };
    // the host's share: TLM's places, where the first SOT lies
    bool tlm = false;
    std::vector<uint64_t> at; std::vector<uint32_t> ln, idx;
    uint64_t count = 0, sot_at = 2;
    if (t2_read_tlm(cs, len, len, kT2pMaxPartsOfFile, &tlm, at, ln, idx, &count)) { err = "TLM"; return GRK_AMD_ERR_INVALID; }
    if (tlm && count > kT2pMaxPartsOfFile) { err = t2p_text(kT2pPartsOfFile); return GRK_AMD_ERR_UNSUPPORTED; }
    while (sot_at + 4 <= len && !(cs[sot_at] == 0xFF && cs[sot_at + 1] == 0x90)) sot_at += 2 + ((uint64_t)cs[sot_at + 2] << 8 | cs[sot_at + 3]);
    const uint32_t cap = (uint32_t)(tlm ? std::max<uint64_t>(count, 1) : std::min<uint64_t>(len / 14 + 1, kT2pMaxPartsOfFile));
    std::vector<unsigned long long> fo_at(cap), tp_at(cap), tp_body(cap), body_at(nt), pk_start(std::max<uint64_t>(P.total_packets, nt));
    std::vector<uint32_t> fo_len(cap), fo_idx(cap, 0xFFFFFFFFu), claim(cap, 0xFFFFFFFFu), tp_len(cap), tp_tile(cap), tp_file(cap), tp_has_plt(cap), tp_npk(cap), tp_first(cap);
    std::vector<uint32_t> cnt(nt), tn_min(nt, 0xFFFFFFFFu), tn_max(nt), slice(nt + 1), has_plt(nt), plt_len(std::max<uint64_t>(P.total_packets, nt));
    // KL-P
    uint32_t n = 0;
    if (tlm) { n = (uint32_t)count; for (uint32_t i = 0; i < n; ++i) { fo_at.at(i) = at.at(i); fo_len.at(i) = ln.at(i); fo_idx.at(i) = idx.at(i); } }
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
        if (fail) { report(t2p_status_locate(n, fail)); return refused(); }
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
    if (status != kT2pNoStatus) return refused();                // (the host stops here: KH-P's grid needs the located count)
    // KH-P, first step: a tile-part's header
    // walk(j, fn): the PLT entries of the tile-part in slot j in order -> fn(k, value); the header's refusal or 0, *body behind SOD
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
    // KH-P, second step: a tile over its tile-parts
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
    // KC-L over the part table, chain after chain
    std::vector<uint32_t> nodes(P.node_bytes + 1);
    std::vector<T2pRowState> state(P.rows + 1);
    for (uint32_t t = 0; t < nt; ++t) {
        const T2ReadTile& T = P.tiles.at(t);
        if (!body_at.at(t)) continue;
        const uint32_t j0 = slice.at(t), nparts = slice.at(t + 1) - j0;
        const T2pParts PT{tp_at.data() + j0, tp_len.data() + j0, tp_body.data() + j0, tp_has_plt.data() + j0, tp_npk.data() + j0, tp_first.data() + j0, nparts};
        const uint32_t L = Q.layers, np = T.npackets / L;
        const bool split = has_plt.at(t) && T.nchains == np;
        const T2ReadPacket* const pk = P.packets.data() + T.first_packet;
        const T2ReadLayerPk* const lp = Q.lpk.data() + T.first_packet;
        uint32_t* const nd = nodes.data() + T.node_base;
        T2pRowState* const st = state.data() + T.row_base;
        for (uint32_t i0 = 0; i0 < T.nchains; ++i0) {
            if (!split && i0) break;
            PlaySink sink;
            T2pPartWalk w{0, 0, 0};
            uint64_t pos = 0;
            t2p_part_walk_start(PT, w, pos);
            bool failed = false;
            auto refuse = [&](uint32_t k, uint32_t y) { report(t2p_status_tile(t, 1, k, y)); failed = true; return false; };
            auto one = [&](uint32_t i, uint32_t l, uint32_t k) -> bool {
                uint64_t end = 0;
                if (split) { pos = pk_start.at(T.pkt_base + k); end = t2p_part_end(PT, t2p_part_of(PT, pos)); }
                else { const uint32_t y = t2p_part_step(PT, w, pos); if (y) return refuse(k, y); end = w.end; }
                if (end > len) { std::printf("a tile-part's end outside the stream\n"); std::abort(); }
                const uint64_t from = pos;
                const size_t p0 = sink.pieces.size();
                uint64_t hdr_end = 0;
                const uint32_t y = t2p_read_packet_layer(src, pk[i], nd, st, P.ht, Q.sty, P.sop, P.eph, l, k, pos, end, sink, &hdr_end);
                if (y) return refuse(k, y);
                for (size_t j = p0; j < sink.pieces.size(); ++j)
                    if (sink.pieces[j].ordinal == 0) { const uint64_t a0 = hdr_end + sink.pieces[j].rel; st[sink.pieces[j].row].src_lo = (uint32_t)a0; st[sink.pieces[j].row].src_hi = (uint32_t)(a0 >> 32); }
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
        }
    }
    if (status != kT2pNoStatus) return refused();
    // KF's rows
    rows.assign(P.rows, grk_amd_coded_block{0, 0, 0});
    for (uint64_t r = 0; r < P.rows; ++r)
        if (!t2p_finish_row(state[r], P.ht, &rows[r])) { err = t2p_text(kT2pPart1Planes); return t2p_code(kT2pPart1Planes); }
    return 0;
}

int cmd_play(const char* path)
{
    const std::vector<uint8_t> v = slurp(path);
    const auto cs = exact(v.data(), v.size());
    StreamTable want;
    std::string ew, eg;
    const int rw = read_all(cs.get(), v.size(), 1, want, ew);
    std::vector<grk_amd_coded_block> rows;
    const int rg = play(cs.get(), v.size(), rows, eg);
    if (rw != rg) { std::printf("%s: the host reader gives %d (%s), the kernels played %d (%s)\n", path, rw, ew.c_str(), rg, eg.c_str()); return 1; }
    if (rw) { std::printf("%s %d %s\n", path, rg, eg.c_str()); return 0; }
    if (rows.size() != want.rows.size()) { std::printf("%s: %zu rows, the host reader %zu\n", path, rows.size(), want.rows.size()); return 1; }
    for (size_t r = 0; r < rows.size(); ++r) {
        const grk_amd_coded_block& a = rows[r]; const grk_amd_coded_block& b = want.rows[r];
        // (a row of several pieces lies in the appendix for the host reader; the play keeps its first piece's place)
        const bool appendix = b.length && b.offset >= v.size();
        if (a.length != b.length || a.missing_msbs != b.missing_msbs || (!appendix && a.offset != b.offset)) {
            std::printf("%s: row %zu is {%llu, %u, %u}, the host reader's {%llu, %u, %u}\n", path, r, (unsigned long long)a.offset, a.length, a.missing_msbs,
                        (unsigned long long)b.offset, b.length, b.missing_msbs);
            return 1;
        }
    }
    std::printf("%s 0 %zu\n", path, rows.size());
    return 0;
}

int cmd_prefixes(const char* path)
{
    const std::vector<uint8_t> v = slurp(path);
    uint64_t good = 0, refused = 0;
    auto once = [&](const uint8_t* d, size_t n, uint32_t threads) {
        const auto cs = exact(d, n);
        StreamTable t;
        std::string e;
        const int rc = read_all(cs.get(), n, threads, t, e);
        if (rc) { ++refused; if (e.empty()) { std::printf("%s: a refusal without a reason\n", path); std::exit(1); } }
        else { ++good; (void)table_hash(t, n); }
    };
    for (size_t n = 0; n < v.size(); ++n) once(v.data(), n, 1 + (n & 1) * 3);
    // the tile-part headers byte by byte: SOT's fields, PLT's entries
    std::vector<uint8_t> w = v;
    for (size_t i = 0; i + 12 <= v.size(); ++i) {
        if (v[i] != 0xFF || v[i + 1] != 0x90 || v[i + 2] != 0 || v[i + 3] != 10) continue;
        size_t end = i + 12;
        while (end + 4 <= v.size() && !(v[end] == 0xFF && v[end + 1] == 0x93)) end += 2 + ((size_t)v[end + 2] << 8 | v[end + 3]);
        end = end + 2 < v.size() ? end + 2 : v.size();
        for (size_t k = i; k < end; ++k)
            for (uint8_t x : {(uint8_t)(v[k] + 1), (uint8_t)(v[k] - 1), (uint8_t)(v[k] ^ 0x80), (uint8_t)0, (uint8_t)0xFF}) {
                if (x == v[k]) continue;
                w[k] = x;
                once(w.data(), w.size(), 1 + (k & 1) * 3);
                w[k] = v[k];
            }
    }
    std::printf("%s %llu %llu\n", path, (unsigned long long)good, (unsigned long long)refused);
    return 0;
}

} // namespace

int main(int argc, char** argv)
{
    if (argc < 3) { std::fprintf(stderr, "usage: t2_parts_units read|play|prefixes FILE...\n"); return 2; }
    const bool prefixes = !std::strcmp(argv[1], "prefixes"), playing = !std::strcmp(argv[1], "play");
    if (!prefixes && !playing && std::strcmp(argv[1], "read")) return 2;
    for (int i = 2; i < argc; ++i)
        if (int rc = prefixes ? cmd_prefixes(argv[i]) : playing ? cmd_play(argv[i]) : cmd_read(argv[i])) return rc;
    return 0;
}
