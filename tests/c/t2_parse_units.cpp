// tests/c/t2_parse_units.cpp -- the device Tier-2 reader played on the CPU (tests/test_t2_parse_cpu.py builds it with
// -fsanitize=address,undefined): KL, KH and KC of grok_amd/csrc/kernels_t2read.hip as plain loops over the functions of t2_parse.h
// and the plan of t2_read_plan.cpp, one chain after the other, against the host reader (t2_reader.cpp, threads = 1) -- the rows
// where it accepts a stream, its code where it refuses.  Every stream sits in a heap buffer of exactly its length.
//   t2_parse_units            the sweep: files this program writes with the host writer from fixed-seed tables, then fixed-seed
//                             single-byte changes and truncations of them
//   t2_parse_units plan       the plan's numbers (chains, packets, scratch, shared descriptors) and its refusals
//   t2_parse_units check F..  the files F: "<name> host <code> core <code> rows <equal|->" per file (exit 1 where the two differ)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static uint64_t g_max[8], g_sum[8];
#define GRK_T2P_COUNT(id, n) do { const uint64_t n_ = (n); if (n_ > g_max[id]) g_max[id] = n_; g_sum[id] += n_; } while (0)
#include "../../grok_amd/csrc/t2_parse.h"
#include "../../grok_amd/csrc/t2_read_plan.h"
#include "../../grok_amd/csrc/t2_reader.h"
#include "../../grok_amd/csrc/geometry.h"

using namespace grk_amd;

namespace {

struct HeapSrc {
    const uint8_t* d; uint64_t len;
    uint32_t byte(uint64_t i) const { if (i >= len) { std::printf("FAIL: the core reads byte %llu of %llu\n", (unsigned long long)i, (unsigned long long)len); std::exit(1); } return d[i]; }
};

// the regions of the latest stream the core accepted: [lo, hi) per kind, for the corruptions' tally
enum Region { kMain, kSot, kPlt, kSopEph, kHeader, kLast, kBody, kRegions };
struct Span { uint64_t lo, hi; int kind; };
std::vector<Span> g_spans;
bool g_record = false;
void span(uint64_t lo, uint64_t hi, int kind) { if (g_record && hi > lo) g_spans.push_back(Span{lo, hi, kind}); }

struct DirectSink {
    grk_amd_coded_block* rows; uint64_t* status; uint32_t tile;
    void put(uint32_t row, uint32_t length, uint32_t msbs, uint64_t rel) { rows[row] = grk_amd_coded_block{rel, length, msbs}; }
    void part1_planes(uint32_t row) { const uint64_t w = t2p_status_tile(tile, 2, row, kT2pPart1Planes); if (w < *status) *status = w; }
};

uint64_t g_ff_inside = 0, g_ff_end = 0;

// the three kernels in turn; the status word as the call would read it
uint64_t play(const uint8_t* cs, uint64_t len, const grk_amd_stream_info& info, const T2ReadPlan& P, std::vector<grk_amd_coded_block>& rows)
{
    uint64_t status = kT2pNoStatus;
    auto report = [&](uint64_t w) { if (w < status) status = w; };
    HeapSrc src{cs, len};
    const uint32_t nt = P.num_tiles;
    rows.assign(P.rows, grk_amd_coded_block{0xDEADBEEFull, 0xDEADBEEFu, 0xDEADBEEFu});
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
    // ---- KH
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
    // ---- KC: chain after chain
    std::vector<uint8_t> nodes(P.node_bytes + 16, 0xAA);           // (stale nodes: a chain clears its own)
    for (uint64_t chain = 0; chain < P.chains; ++chain) {
        uint32_t lo = 0, hi = nt;
        while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (P.tiles[mid].chain_base <= chain) lo = mid; else hi = mid; }
        const uint32_t t = lo;
        const T2ReadTile& T = P.tiles[t];
        if (!body_at[t]) continue;
        const uint64_t end = part_at[t] + part_len[t];
        const bool plt = has_plt[t] != 0, split = plt && T.nchains == T.npackets;
        uint32_t k0 = (uint32_t)(chain - T.chain_base), k1 = k0 + 1;
        if (!split) { if (k0) continue; k1 = T.npackets; }
        const T2ReadPacket* pk = P.packets.data() + T.first_packet;
        uint8_t* const nd = nodes.data() + T.node_base;
        std::memset(nd + (split ? pk[k0].node_at : 0u), 0, split ? pk[k0].node_n : T.node_bytes);
        DirectSink sink{rows.data() + T.row_base, &status, t};
        uint64_t pos = split ? pk_start[T.pkt_base + k0] : body_at[t];
        bool stop = false;
        for (uint32_t k = k0; k < k1 && !stop; ++k) {
            const uint64_t from = pos;
            uint64_t body = 0;
            const uint64_t ff0 = g_sum[kT2pSeenFF], fe0 = g_sum[kT2pSeenEndFF];
            const uint32_t why = t2p_read_packet(src, pk[k], nd, P.ht, P.sop, P.eph, k, pos, end, sink, &body);
            if (why) { report(t2p_status_tile(t, 1, k, why)); stop = true; break; }
            if (g_sum[kT2pSeenFF] > ff0) ++g_ff_inside;
            if (g_sum[kT2pSeenEndFF] > fe0) ++g_ff_end;
            if (P.sop) span(from, from + 6, kSopEph);
            if (P.eph) span(body - 2, body, kSopEph);
            span(from + (P.sop ? 6 : 0), body - (P.eph ? 2 : 0), kHeader);
            span(body, pos, kBody);
            for (uint32_t bi = 0; bi < pk[k].nbands; ++bi) {
                const T2ReadBand& B = pk[k].band[bi];
                grk_amd_coded_block* r = rows.data() + T.row_base + B.first_row;
                for (uint32_t i = 0; i < B.gw * B.gh; ++i) r[i].offset = t2p_row_offset(r[i].length, r[i].offset, body);
            }
            if (plt && pos - from != plt_len[T.pkt_base + k]) { report(t2p_status_tile(t, 1, k, kT2pPltSize)); stop = true; }
        }
        if (!stop && !split && pos != end) report(t2p_status_tile(t, 1, T.npackets, kT2pTail));
    }
    if (len) span(len - 1, len, kLast);
    return status;
}

struct Outcome { int host, core; bool rows_equal; std::string host_err, core_err; bool plan_refused = false; };

// both readers over one stream (a heap copy of exactly len bytes)
Outcome both(const std::vector<uint8_t>& file)
{
    Outcome o{0, 0, false, "", ""};
    uint8_t* cs = (uint8_t*)std::malloc(file.size() ? file.size() : 1);
    std::memcpy(cs, file.data(), file.size());
    const uint64_t len = file.size();
    grk_amd_stream_info info;
    std::string err;
    int rc = read_stream_header(cs, len, info, err);
    if (rc) { o.host = o.core = rc; o.host_err = err; std::free(cs); return o; }      // (the header is the host's on both sides)
    StreamTable tab;
    o.host = read_stream_packets(cs, len, info, 1, tab, err);
    o.host_err = err;
    T2ReadPlan P;
    const char* why = "";
    rc = plan_t2_read(info, P, &why);
    if (rc) { o.core = rc; o.core_err = why; o.plan_refused = true; std::free(cs); return o; }
    std::vector<grk_amd_coded_block> rows;
    g_spans.clear();
    const uint64_t st = play(cs, len, info, P, rows);
    if (st != kT2pNoStatus) { o.core = t2p_code(t2p_status_why(st)); o.core_err = t2p_text(t2p_status_why(st)); }
    else if (!o.host) {
        o.rows_equal = rows.size() == tab.rows.size();
        for (size_t i = 0; o.rows_equal && i < rows.size(); ++i)
            if (rows[i].offset != tab.rows[i].offset || rows[i].length != tab.rows[i].length || rows[i].missing_msbs != tab.rows[i].missing_msbs) {
                o.rows_equal = false;
                o.core_err = "row " + std::to_string(i) + ": core {" + std::to_string(rows[i].offset) + ", " + std::to_string(rows[i].length) + ", " +
                             std::to_string(rows[i].missing_msbs) + "} host {" + std::to_string(tab.rows[i].offset) + ", " + std::to_string(tab.rows[i].length) + ", " +
                             std::to_string(tab.rows[i].missing_msbs) + "}";
            }
    }
    std::free(cs);
    return o;
}

bool bounds_ok()
{
    const uint64_t lim[6] = {kT2pThreshold, kT2pMaxLblock + 1, kT2pMaxLenBits, kT2pMaxPasses, kT2pMaxLevels, kT2pPltBytes};
    for (int i = 0; i < 6; ++i)
        if (g_max[i] > lim[i]) { std::printf("FAIL: loop %d took %llu steps (bound %llu)\n", i, (unsigned long long)g_max[i], (unsigned long long)lim[i]); return false; }
    return true;
}

// ---- the files of the sweep -----------------------------------------------------------------------------------------------------
uint64_t g_rng = 1;
uint32_t rnd() { g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(g_rng >> 33); }

grk_amd_tile_params params(uint32_t w, uint32_t h, uint32_t nc, uint32_t levels, uint32_t cbw, uint32_t cbh)
{
    grk_amd_tile_params p{};
    p.tile_w = w; p.tile_h = h; p.num_comps = (uint16_t)nc; p.prec = 8; p.mct = nc >= 3; p.num_levels = (uint8_t)levels;
    p.cblk_w_exp = (uint8_t)cbw; p.cblk_h_exp = (uint8_t)cbh;
    return p;
}

// lens: 0 = small random lengths (some 0), else the one length every `each`-th block gets
struct Draw { uint32_t special_len = 0, each = 0; bool msbs = false; };

// a file of the layout `im` (tiles of base's coding) with sub-sampling (dx, dy per component; null: none)
std::vector<uint8_t> write_file(const grk_amd_image_layout& im, const grk_amd_tile_params& base, const uint8_t* dx, const uint8_t* dy, uint32_t flags,
                                const Draw& dr, uint64_t seed)
{
    g_rng = seed * 2654435761ull + 12345;
    const int64_t nt = grk_amd_layout_num_tiles(&im);
    std::vector<grk_amd_coded_block> table;
    uint64_t big = 4096;
    for (int64_t t = 0; t < nt; ++t) {
        const uint32_t nruns = dx ? base.num_comps : 1;
        for (uint32_t c = 0; c < nruns; ++c) {
            grk_amd_tile_params p;
            int rc = dx ? grk_amd_layout_tile_comp(&im, &base, dx[c], dy[c], (uint32_t)t, &p) : grk_amd_layout_tile(&im, &base, (uint32_t)t, &p);
            if (dx) { p.num_comps = 1; p.mct = 0; }
            if (rc) { std::printf("FAIL: layout %d\n", rc); std::exit(1); }
            TileGeom tg;
            if (build_tile_geom(p, tg)) { std::printf("FAIL: geometry\n"); std::exit(1); }
            const int64_t nb = (int64_t)tg.blocks_per_comp * p.num_comps;
            std::vector<grk_amd_block> blocks;
            for (uint32_t cc = 0; cc < p.num_comps; ++cc) blocks.insert(blocks.end(), tg.blocks_comp0.begin(), tg.blocks_comp0.end());
            for (int64_t i = 0; i < nb; ++i) {
                grk_amd_coded_block r{0, 0, 0};
                const uint32_t v = rnd();
                r.length = (v & 7u) == 0 ? 0u : 1u + ((v >> 3) % ((v >> 20 & 3u) == 0 ? 300u : 40u));
                if (dr.each && table.size() % dr.each == dr.each / 2) r.length = dr.special_len;
                const uint32_t kmax = blocks[(size_t)i].kmax ? blocks[(size_t)i].kmax : 1;
                r.missing_msbs = dr.msbs ? rnd() % kmax : kmax - 1;
                r.offset = rnd() % 1024;
                big = std::max<uint64_t>(big, r.offset + r.length);
                table.push_back(r);
            }
        }
    }
    std::vector<uint8_t> coded(big);
    for (auto& b : coded) b = (uint8_t)rnd();
    uint64_t total = 0;
    for (const auto& r : table) total += r.length;
    std::vector<uint8_t> out(total + table.size() * 16 + (1u << 16));
    const int64_t n = dx ? grk_amd_write_codestream_subsampled(&im, &base, dx, dy, table.data(), coded.data(), flags, out.data(), out.size())
                         : grk_amd_write_codestream_layout(&im, &base, table.data(), coded.data(), flags, out.data(), out.size());
    if (n < 0) { std::printf("FAIL: the writer refused a file of the sweep (%lld, flags 0x%x)\n", (long long)n, flags); std::exit(1); }
    out.resize((size_t)n);
    return out;
}

grk_amd_image_layout image(uint32_t w, uint32_t h, uint32_t tw, uint32_t th, uint32_t ox = 0, uint32_t oy = 0)
{
    return grk_amd_image_layout{ox, oy, ox + w, oy + h, 0, 0, tw, th};
}

uint64_t g_files = 0, g_accepted = 0, g_refused = 0, g_plan_refused = 0, g_tally[kRegions];

bool expect_equal(const std::vector<uint8_t>& f, const char* what, bool must_accept)
{
    ++g_files;
    const Outcome o = both(f);
    // (what the plan refuses -- several layers, LAZY / TERMALL -- it refuses before a byte of a packet is looked at, whatever the
    //  host reader, which takes such files, finds in them)
    if (o.plan_refused && !must_accept && o.core == GRK_AMD_ERR_UNSUPPORTED) { ++g_plan_refused; return true; }
    const bool ok = o.host == o.core && (o.host != 0 || o.rows_equal) && (!must_accept || o.host == 0);
    if (!ok) std::printf("FAIL: %s: host %d (%s), core %d (%s)\n", what, o.host, o.host_err.c_str(), o.core, o.core_err.c_str());
    if (o.host == 0) ++g_accepted; else ++g_refused;
    return ok;
}

int region_of(uint64_t pos)
{
    int kind = kBody;
    for (const Span& s : g_spans) if (pos >= s.lo && pos < s.hi && s.kind < kind) kind = s.kind;
    for (const Span& s : g_spans) if (s.kind == kLast && pos >= s.lo && pos < s.hi) kind = kLast;
    return kind;
}

// fixed-seed single-byte changes and truncations of a file the core accepted
bool corrupt(const std::vector<uint8_t>& f, uint64_t seed, uint32_t changes, uint32_t cuts)
{
    g_record = true;
    const Outcome clean = both(f);
    g_record = false;
    if (clean.host || clean.core) { std::printf("FAIL: a file to corrupt is refused\n"); return false; }
    const std::vector<Span> spans = g_spans;
    g_rng = seed * 977 + 5;
    bool ok = true;
    char what[96];
    for (uint32_t i = 0; i < changes && ok; ++i) {
        // half of the changes in the spans the parsers read (headers of every kind), the others anywhere; the last byte once
        uint64_t pos;
        if (i == 0) pos = f.size() - 1;
        else if ((i & 1u) && !spans.empty()) {
            const Span* s;
            do s = &spans[rnd() % spans.size()]; while (s->kind == kBody && (rnd() & 3u));
            pos = s->lo + rnd() % (s->hi - s->lo);
        } else pos = rnd() % f.size();
        std::vector<uint8_t> g = f;
        const uint32_t how = rnd() % 4;
        g[pos] = how == 0 ? (uint8_t)0xFF : how == 1 ? (uint8_t)(g[pos] ^ (1u << (rnd() % 8))) : how == 2 ? (uint8_t)(g[pos] + 1) : (uint8_t)rnd();
        g_spans = spans; ++g_tally[region_of(pos)];
        std::snprintf(what, sizeof what, "seed %llu: byte %llu %02X -> %02X", (unsigned long long)seed, (unsigned long long)pos, f[pos], g[pos]);
        ok = expect_equal(g, what, false);
    }
    for (uint32_t i = 0; i < cuts && ok; ++i) {
        const uint64_t n = i == 0 ? f.size() - 1 : rnd() % f.size();
        std::vector<uint8_t> g(f.begin(), f.begin() + (size_t)n);
        std::snprintf(what, sizeof what, "seed %llu: cut at %llu of %llu", (unsigned long long)seed, (unsigned long long)n, (unsigned long long)f.size());
        ok = expect_equal(g, what, false);
    }
    return ok;
}

int sweep()
{
    bool ok = true;
    uint64_t seed = 1, corruptions = 0;
    auto run = [&](const grk_amd_image_layout& im, const grk_amd_tile_params& b, const uint8_t* dx, const uint8_t* dy, uint32_t flags, const Draw& dr,
                   const char* what, uint32_t changes) {
        if (!ok) return;
        const std::vector<uint8_t> f = write_file(im, b, dx, dy, flags, dr, seed++);
        char name[128];
        std::snprintf(name, sizeof name, "%s, flags 0x%x, seed %llu", what, flags, (unsigned long long)(seed - 1));
        ok = expect_equal(f, name, true);
        if (ok && changes) { ok = corrupt(f, seed, changes, changes / 4 + 1); corruptions += changes + changes / 4 + 1; }
    };
    const uint8_t dx420[3] = {1, 2, 2}, dy420[3] = {1, 2, 2};
    // PLT x TLM x SOP x EPH x the five orders x one and three components, deep trees (4 x 4 blocks)
    for (uint32_t order = 0; order < 5; ++order)
        for (uint32_t f = 0; f < 16; ++f)
            for (uint32_t nc = 1; nc <= 3; nc += 2)
                run(image(40, 64, 40, 64), params(40, 64, nc, 1, 2, 2), nullptr, nullptr, f | GRK_AMD_CS_PROG(order), Draw{}, "40x64 tile", order == 2 || f == 15 || f == 0 ? 24 : 6);
    // precinct grids, per-block zero bit-planes
    for (uint32_t order = 0; order < 5; ++order)
        for (uint32_t f = 0; f < 16; f += 5) {
            grk_amd_tile_params p = params(96, 80, 3, 2, 3, 3);
            p.precinct_exp[0] = 4 | 4 << 4; p.precinct_exp[1] = 5 | 4 << 4; p.precinct_exp[2] = 5 | 5 << 4;
            Draw dr; dr.msbs = true;
            run(image(96, 80, 96, 80), p, nullptr, nullptr, f | GRK_AMD_CS_BLOCK_MSBS | GRK_AMD_CS_PROG(order), dr, "precinct grid, block msbs", 16);
            run(image(40, 64, 40, 64), params(40, 64, 1, 1, 2, 2), nullptr, nullptr, f | GRK_AMD_CS_BLOCK_MSBS | GRK_AMD_CS_PROG(order), dr, "block msbs", 12);
        }
    // several tiles of differing geometry (edge tiles, an image off the origin), 4:2:0
    for (uint32_t order = 0; order < 5; ++order)
        for (uint32_t f = 0; f < 16; f += 3) {
            run(image(100, 76, 64, 48), params(64, 48, 3, 2, 4, 3), nullptr, nullptr, (f & ~1u) | GRK_AMD_CS_PROG(order), Draw{}, "2 x 2 tiles", 12);
            run(image(150, 70, 64, 32, 7, 5), params(64, 32, 1, 3, 3, 3), nullptr, nullptr, f | GRK_AMD_CS_PROG(order), Draw{}, "tiles off the origin", 12);
            run(image(66, 50, 66, 50), params(66, 50, 3, 2, 3, 3), dx420, dy420, (f & ~1u) | GRK_AMD_CS_PROG(order), Draw{}, "4:2:0", 12);
            run(image(66, 50, 32, 32), params(32, 32, 3, 1, 3, 3), dx420, dy420, (f & ~1u) | GRK_AMD_CS_PROG(order), Draw{}, "4:2:0 tiles", 12);
        }
    // band grids of 1 x 65 and 65 x 1 blocks: trees of eight levels
    for (uint32_t f = 0; f < 16; f += 5) {
        run(image(260, 4, 260, 4), params(260, 4, 1, 0, 2, 2), nullptr, nullptr, f, Draw{}, "65 x 1 blocks", 12);
        run(image(4, 260, 4, 260), params(4, 260, 1, 0, 2, 2), nullptr, nullptr, f, Draw{}, "1 x 65 blocks", 12);
    }
    // lengths 0, 2^k - 1, 2^k, 2^k + 1 up to 2^20
    for (uint32_t k = 0; k <= 20 && ok; ++k)
        for (int d = -1; d <= 1; ++d) {
            const int64_t v = (1ll << k) + d;
            if (v < 0 || v > (1 << 20) + 1) continue;
            Draw dr; dr.special_len = (uint32_t)v; dr.each = 5;
            run(image(16, 16, 16, 16), params(16, 16, 1, 1, 2, 2), nullptr, nullptr, (k & 1u ? GRK_AMD_CS_PLT : 0u) | (k % 3 == 0 ? GRK_AMD_CS_SOP | GRK_AMD_CS_EPH : 0u), dr, "lengths", 0);
        }
    // headers with 0xFF inside and at their end: tiny tiles over many seeds
    for (uint32_t i = 0; i < 1500 && ok; ++i) {
        Draw dr; dr.msbs = true;
        run(image(8, 8, 8, 8), params(8, 8, 1, 0, 2, 2), nullptr, nullptr, (i % 4) * 2u /* PLT, SOP */ | (i & 8u ? GRK_AMD_CS_EPH : 0u) | GRK_AMD_CS_BLOCK_MSBS, dr, "stuffing", i % 50 == 0 ? 8 : 0);
    }
    if (!ok) return 1;
    if (!bounds_ok()) return 1;
    if (!g_ff_inside || !g_ff_end) { std::printf("FAIL: %llu headers with 0xFF inside, %llu that end on 0xFF\n", (unsigned long long)g_ff_inside, (unsigned long long)g_ff_end); return 1; }
    for (int k = 0; k < kRegions; ++k)
        if (k != kBody && !g_tally[k]) { std::printf("FAIL: no corruption in region %d\n", k); return 1; }
    std::printf("ok: %llu streams (%llu accepted, %llu refused alike, %llu refused by the plan), %llu corruptions [main %llu sot %llu plt %llu sop/eph %llu header %llu last %llu body %llu], "
                "headers with 0xFF inside %llu, ending on 0xFF %llu, loop maxima tree %llu lblock %llu lenbits %llu passes %llu levels %llu plt %llu\n",
                (unsigned long long)g_files, (unsigned long long)g_accepted, (unsigned long long)g_refused, (unsigned long long)g_plan_refused, (unsigned long long)corruptions,
                (unsigned long long)g_tally[kMain], (unsigned long long)g_tally[kSot], (unsigned long long)g_tally[kPlt], (unsigned long long)g_tally[kSopEph],
                (unsigned long long)g_tally[kHeader], (unsigned long long)g_tally[kLast], (unsigned long long)g_tally[kBody],
                (unsigned long long)g_ff_inside, (unsigned long long)g_ff_end, (unsigned long long)g_max[0], (unsigned long long)g_max[1], (unsigned long long)g_max[2],
                (unsigned long long)g_max[3], (unsigned long long)g_max[4], (unsigned long long)g_max[5]);
    return 0;
}

// ---- the plan's numbers -----------------------------------------------------------------------------------------------------------
int plan_mode()
{
    bool ok = true;
    auto fail = [&](const char* what) { std::printf("FAIL: plan: %s\n", what); ok = false; };
    const uint8_t dx420[3] = {1, 2, 2}, dy420[3] = {1, 2, 2};
    struct Case { grk_amd_image_layout im; grk_amd_tile_params p; const uint8_t* dx; const uint8_t* dy; uint32_t classes; };
    grk_amd_tile_params pg = params(96, 80, 3, 2, 3, 3);
    pg.precinct_exp[0] = 4 | 4 << 4; pg.precinct_exp[1] = 5 | 4 << 4; pg.precinct_exp[2] = 5 | 5 << 4;
    const Case cases[] = {
        {image(40, 64, 40, 64), params(40, 64, 1, 1, 2, 2), nullptr, nullptr, 1},
        {image(96, 80, 96, 80), pg, nullptr, nullptr, 1},
        {image(100, 76, 64, 48), params(64, 48, 3, 2, 4, 3), nullptr, nullptr, 4},
        {image(1024, 1024, 64, 64), params(64, 64, 3, 2, 4, 4), nullptr, nullptr, 1},          // 256 tiles, one set of descriptors
        {image(66, 50, 32, 32), params(32, 32, 3, 1, 3, 3), dx420, dy420, 4},
    };
    for (const Case& k : cases)
        for (uint32_t order = 0; order < 5; ++order)
            for (uint32_t plt = 0; plt < 2; ++plt) {
                const std::vector<uint8_t> f = write_file(k.im, k.p, k.dx, k.dy, (plt ? GRK_AMD_CS_PLT : 0u) | GRK_AMD_CS_PROG(order), Draw{}, 7);
                grk_amd_stream_info info; std::string err;
                if (read_stream_header(f.data(), f.size(), info, err)) { fail("header"); continue; }
                T2ReadPlan P; const char* why = "";
                if (plan_t2_read(info, P, &why)) { fail(why); continue; }
                // against grk_amd_tile_precincts / grk_amd_tile_layout tile by tile
                uint64_t rows = 0, packets = 0, chains = 0, nodes = 0;
                for (uint32_t t = 0; t < info.num_tiles; ++t) {
                    uint64_t tp = 0, tr = 0;
                    for (uint32_t c = 0; c < info.base.num_comps; ++c) {
                        grk_amd_tile_params p;
                        grk_amd_layout_tile_comp(&info.layout, &info.base, info.comp_dx[c], info.comp_dy[c], t, &p);
                        p.num_comps = 1; p.mct = 0;
                        // (what grk_amd_tile_precincts and grk_amd_tile_layout report: the tile-component's geometry)
                        TileGeom tg;
                        if (build_tile_geom(p, tg)) fail("geometry");
                        for (uint32_t r = 0; r <= p.num_levels; ++r) tp += (uint64_t)tg.res[r].npw * tg.res[r].nph;
                        tr += tg.blocks_per_comp;
                    }
                    const T2ReadTile& T = P.tiles[t];
                    if (T.npackets != tp) fail("a tile's packets are not its precincts");
                    if (T.rows != tr || T.row_base != rows) fail("a tile's rows");
                    if (T.nchains != (plt ? tp : 1) || T.chain_base != chains || T.pkt_base != packets || T.node_base != nodes) fail("a tile's chains or scratch");
                    uint64_t blocks = 0, nn = 0;
                    for (uint32_t q = 0; q < T.npackets; ++q) {
                        const T2ReadPacket& d = P.packets[T.first_packet + q];
                        if (d.node_at != nn) fail("a packet's nodes do not follow the one before");
                        for (uint32_t b = 0; b < d.nbands; ++b) {
                            uint32_t nlev = 0, n = 0; t2p_tree_shape(d.band[b].gw, d.band[b].gh, &nlev, &n);
                            if (d.band[b].nodes != n || d.band[b].nlev != nlev || d.band[b].first_row + d.band[b].gw * d.band[b].gh > T.rows) fail("a band");
                            blocks += (uint64_t)d.band[b].gw * d.band[b].gh; nn += 2ull * n;
                        }
                        if (d.node_n != nn - d.node_at) fail("a packet's nodes");
                    }
                    if (blocks != tr || T.node_bytes < nn) fail("a tile's blocks or nodes");
                    rows += tr; packets += tp; chains += T.nchains; nodes += T.node_bytes;
                }
                if (P.rows != rows || P.rows != info.num_blocks || P.total_packets != packets || P.chains != chains || P.node_bytes != nodes) fail("totals");
                if (P.bytes_rows() != rows * 16 || P.bytes_plt() != (plt ? packets * 12 : 0)) fail("scratch sizes");
                if (order <= 1 && P.classes.size() != k.classes) { std::printf("(%zu classes, %u builds, %u tiles) ", P.classes.size(), P.geometry_builds, info.num_tiles); fail("shared descriptors"); }
                if (P.geometry_builds != P.classes.size()) fail("a geometry built for a tile that shares its descriptors");
            }
    // refusals
    {
        const std::vector<uint8_t> f = write_file(image(40, 64, 40, 64), params(40, 64, 1, 1, 2, 2), nullptr, nullptr, 0, Draw{}, 3);
        grk_amd_stream_info info; std::string err; T2ReadPlan P; const char* why = "";
        read_stream_header(f.data(), f.size(), info, err);
        grk_amd_stream_info i2 = info; i2.num_layers = 2;
        if (plan_t2_read(i2, P, &why) != GRK_AMD_ERR_UNSUPPORTED) fail("two layers are not refused");
        for (uint32_t sty : {1u, 4u, 5u, 0x3Fu}) {
            i2 = info; i2.base.reserved[0] = 1; i2.base.reserved[1] = (uint8_t)sty;
            if (plan_t2_read(i2, P, &why) != GRK_AMD_ERR_UNSUPPORTED) fail("LAZY / TERMALL is not refused");
        }
        i2 = info; i2.base.reserved[0] = 1; i2.base.reserved[1] = 0x3A;
        if (plan_t2_read(i2, P, &why) != GRK_AMD_OK) fail("Part-1 of one codeword segment is refused");
    }
    if (ok) std::printf("ok: plan\n");
    return ok ? 0 : 1;
}

int check_mode(int argc, char** argv)
{
    int bad = 0;
    for (int i = 2; i < argc; ++i) {
        std::FILE* fh = std::fopen(argv[i], "rb");
        if (!fh) { std::printf("%s cannot be read\n", argv[i]); bad = 1; continue; }
        std::vector<uint8_t> f;
        uint8_t buf[65536];
        for (size_t n; (n = std::fread(buf, 1, sizeof buf, fh)) > 0;) f.insert(f.end(), buf, buf + n);
        std::fclose(fh);
        const Outcome o = both(f);
        const char* base = std::strrchr(argv[i], '/');
        std::printf("%s host %d core %d rows %s\n", base ? base + 1 : argv[i], o.host, o.core, o.host == 0 && o.core == 0 ? (o.rows_equal ? "equal" : "DIFFER") : "-");
        if (o.plan_refused) continue;
        if (o.host != o.core || (o.host == 0 && !o.rows_equal)) { std::printf("  host: %s\n  core: %s\n", o.host_err.c_str(), o.core_err.c_str()); bad = 1; }
    }
    if (!bounds_ok()) bad = 1;
    return bad;
}

} // namespace

int main(int argc, char** argv)
{
    if (argc > 1 && !std::strcmp(argv[1], "plan")) return plan_mode();
    if (argc > 1 && !std::strcmp(argv[1], "check")) return check_mode(argc, argv);
    return sweep();
}
