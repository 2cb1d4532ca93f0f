// grok_amd/csrc/t2_read_plan.cpp -- the host planning of the device Tier-2 reader (t2_read_plan.h).  No HIP call in here.
#include "t2_read_plan.h"
#include "geometry.h"
#include "t2_order.h"
#include <algorithm>
#include <cstring>
#include <map>

using namespace grk_amd;

namespace {

inline bool subsampled(const grk_amd_stream_info& info)
{
    for (uint32_t c = 0; c < info.base.num_comps && c < 4; ++c) if (info.comp_dx[c] != 1 || info.comp_dy[c] != 1) return true;
    return false;
}

// What a tile's descriptors depend on, without building its geometry: per component its rectangle's size, its origin modulo the
// coarsest code-block grid seen from the reference grid, and per resolution and axis where the precinct grid cuts it -- a
// resolution inside one precinct: only whether it starts on the precinct's corner (the position-major orders look at the corners).
// Two tiles of one key have the same packets, grids and rows.
std::vector<uint32_t> tile_key(const grk_amd_stream_info& info, const grk_amd_tile_params& p, bool sub)
{
    std::vector<uint32_t> k;
    const uint32_t L = p.num_levels;
    const uint64_t x0 = p.tile_x0, y0 = p.tile_y0, x1 = x0 + p.tile_w, y1 = y0 + p.tile_h;
    auto cdiv = [](uint64_t a, uint64_t b) { return (a + b - 1) / b; };
    for (uint32_t c = 0; c < p.num_comps; ++c) {
        const uint64_t dx = sub ? info.comp_dx[c] : 1, dy = sub ? info.comp_dy[c] : 1;
        const uint64_t lo[2] = {cdiv(x0, dx), cdiv(y0, dy)}, hi[2] = {cdiv(x1, dx), cdiv(y1, dy)}, org[2] = {x0, y0}, d[2] = {dx, dy};
        const uint32_t cbe[2] = {p.cblk_w_exp, p.cblk_h_exp};
        for (int a = 0; a < 2; ++a) {
            k.push_back((uint32_t)(hi[a] - lo[a]));
            k.push_back((uint32_t)(lo[a] & ((1ull << (L + cbe[a])) - 1)));
            k.push_back((uint32_t)(org[a] % (d[a] << (L + cbe[a]))));
            for (uint32_t r = 0; r <= L; ++r) {
                const uint32_t pe = p.precinct_exp[r], pp = pe ? (a ? pe >> 4 : pe & 15u) : 15u, sh = L - r;
                const uint64_t r0 = (lo[a] + (1ull << sh) - 1) >> sh, r1 = (hi[a] + (1ull << sh) - 1) >> sh;
                const uint64_t in = r0 & ((1ull << pp) - 1);
                const bool single = r1 <= r0 || (r0 >> pp) == ((r1 - 1) >> pp);
                // (the precinct's corner on the reference grid, clipped to the tile: packet_order's position)
                const uint64_t corner = ((((r0 >> pp) << pp) << sh) * d[a]);
                k.push_back(single ? 0x80000000u | (uint32_t)(corner > org[a] ? corner - org[a] : 0) : (uint32_t)in);
            }
        }
    }
    return k;
}

} // namespace

// the plan of a file of L layers (lpk == nullptr: the single-layer reader's, L = 1; else the general reader's, with what its
// chain kernel needs beside every packet descriptor)
static int plan_common(const grk_amd_stream_info& info, T2ReadPlan& out, const char** why, std::vector<T2ReadLayerPk>* lpk, uint64_t L)
{
    out.sop = (info.flags & GRK_AMD_CS_SOP) != 0; out.eph = (info.flags & GRK_AMD_CS_EPH) != 0;
    out.plt = (info.flags & GRK_AMD_CS_PLT) != 0;
    out.num_tiles = info.num_tiles;
    const bool sub = subsampled(info);
    const uint32_t order = (info.flags >> GRK_AMD_CS_PROG_SHIFT) & 7u;
    std::map<std::vector<uint32_t>, uint32_t> seen;
    out.tiles.resize(info.num_tiles);
    uint64_t rows = 0, chains = 0, pkts = 0, nodes = 0;
    for (uint32_t t = 0; t < info.num_tiles; ++t) {
        grk_amd_tile_params p;
        int rc = grk_amd_layout_tile(&info.layout, &info.base, t, &p);
        if (rc) { *why = "a tile without geometry"; return rc; }
        const std::vector<uint32_t> key = tile_key(info, p, sub);
        auto it = seen.find(key);
        if (it == seen.end()) {
            // the tile-components' geometries as read_tile makes them, and the packets in its order
            const uint32_t nc = p.num_comps;
            std::vector<TileGeom> geoms; geoms.reserve(nc);
            std::vector<const TileGeom*> cg(nc);
            std::vector<uint64_t> row0(nc);
            uint64_t nrows = 0;
            for (uint32_t c = 0; c < nc; ++c) {
                uint32_t like = c;
                for (uint32_t k = 0; k < c; ++k) if (!sub || (info.comp_dx[k] == info.comp_dx[c] && info.comp_dy[k] == info.comp_dy[c])) { like = k; break; }
                if (like == c) {
                    grk_amd_tile_params pc = p;
                    if (sub) { rc = grk_amd_layout_tile_comp(&info.layout, &info.base, info.comp_dx[c], info.comp_dy[c], t, &pc); pc.num_comps = 1; pc.mct = 0; }
                    geoms.emplace_back();
                    if (!rc) rc = build_tile_geom(pc, geoms.back());
                    if (rc) { *why = "a tile-component without geometry"; return rc; }
                    cg[c] = &geoms.back();
                } else cg[c] = cg[like];
                row0[c] = nrows; nrows += cg[c]->blocks_per_comp;
            }
            ++out.geometry_builds;
            if (nrows > 0x7FFFFFFFull) { *why = "a tile of more than 2^31 code-blocks"; return GRK_AMD_ERR_UNSUPPORTED; }
            const std::vector<Pk> seq = packet_order(cg, sub ? info.comp_dx : nullptr, sub ? info.comp_dy : nullptr, p.tile_x0, p.tile_y0, order);
            T2ReadClass cl{(uint32_t)out.packets.size(), (uint32_t)seq.size(), (uint32_t)nrows, 0, 0};
            uint64_t node_at = 0, tile_blocks = 0;
            for (const Pk& q : seq) {
                const ResGeom& R = cg[q.c]->res[q.r];
                T2ReadPacket d{};
                d.c = q.c; d.r = q.r; d.pi = q.pi;
                d.node_at = (uint32_t)node_at;
                for (uint32_t bi = 0; bi < R.num_bands; ++bi) {
                    const BandGeom::Prec& G = R.band[bi].prec[q.pi];
                    if (!G.gw || !G.gh) continue;
                    T2ReadBand& B = d.band[d.nbands++];
                    B.gw = G.gw; B.gh = G.gh; B.first_row = (uint32_t)(row0[q.c] + G.first_block);
                    t2p_tree_shape(G.gw, G.gh, &B.nlev, &B.nodes);
                    B.node_at = (uint32_t)node_at; node_at += 2ull * B.nodes;
                    const uint32_t band = q.r == 0 ? 0u : 3u * q.r - 2u + bi;
                    const uint32_t expn = info.qstyle ? info.qcd_words[band] >> 11 : info.qcd_words[band] >> 3;
                    B.kbits = expn + info.guard_bits - 1u;
                    d.nblocks += G.gw * G.gh;
                }
                d.node_n = (uint32_t)(node_at - d.node_at);
                if (lpk) lpk->push_back(T2ReadLayerPk{0, 0, (uint32_t)tile_blocks, 0});
                tile_blocks += d.nblocks;
                cl.max_chain_blocks = std::max(cl.max_chain_blocks, d.nblocks);
                if (node_at > 0x7FFFFFFFull) { *why = "tag trees beyond 2^31 nodes"; return GRK_AMD_ERR_UNSUPPORTED; }
                out.packets.push_back(d);
            }
            if (tile_blocks != nrows) { *why = "a tile whose packets do not hold its code-blocks once each"; return GRK_AMD_ERR_INVALID; }
            if (!out.plt) cl.max_chain_blocks = (uint32_t)nrows;
            // RLCP: the layers run inside a resolution -- a precinct's run: the packets of its resolution, which follow each other
            for (size_t i = 0; lpk && i < seq.size();) {
                size_t j = i;
                while (j < seq.size() && seq[j].r == seq[i].r) ++j;
                for (size_t k = i; k < j; ++k) { (*lpk)[cl.first_packet + k].run_first = (uint32_t)i; (*lpk)[cl.first_packet + k].run_count = (uint32_t)(j - i); }
                i = j;
            }
            cl.node_bytes = (uint32_t)((node_at + 15) & ~15ull);
            it = seen.emplace(key, (uint32_t)out.classes.size()).first;
            out.classes.push_back(cl);
        }
        const T2ReadClass& cl = out.classes[it->second];
        T2ReadTile& T = out.tiles[t];
        if (cl.npackets * L > 0x7FFFFFFFull) { *why = "tables beyond the device reader's 32-bit fields"; return GRK_AMD_ERR_UNSUPPORTED; }
        T.cls = it->second; T.first_packet = cl.first_packet; T.npackets = (uint32_t)(cl.npackets * L);
        T.row_base = (uint32_t)rows; T.rows = cl.rows;
        T.chain_base = (uint32_t)chains; T.nchains = out.plt ? cl.npackets : 1u;
        T.pkt_base = (uint32_t)pkts; T.node_base = (uint32_t)nodes; T.node_bytes = cl.node_bytes;
        rows += cl.rows; chains += T.nchains; pkts += T.npackets; nodes += cl.node_bytes;
        if (rows > 0x7FFFFFFFull || chains > 0x7FFFFFFFull || pkts > 0x7FFFFFFFull || nodes > 0xFFFFFFFFull) {
            *why = "tables beyond the device reader's 32-bit fields"; return GRK_AMD_ERR_UNSUPPORTED;
        }
    }
    if (rows != info.num_blocks) { *why = "info.num_blocks"; return GRK_AMD_ERR_INVALID; }
    out.rows = rows; out.chains = chains; out.total_packets = pkts; out.node_bytes = nodes;
    return GRK_AMD_OK;
}

int grk_amd::plan_t2_read(const grk_amd_stream_info& info, T2ReadPlan& out, const char** why)
{
    const char* dummy; if (!why) why = &dummy;
    *why = "";
    out = T2ReadPlan{};
    if (info.num_layers != 1) { *why = "the device reader takes files of one quality layer"; return GRK_AMD_ERR_UNSUPPORTED; }
    out.ht = !info.base.reserved[0];
    if (!out.ht && (info.base.reserved[1] & 0x05)) {
        *why = "the device reader takes Part-1 code-blocks of one codeword segment (no LAZY, no TERMALL)";
        return GRK_AMD_ERR_UNSUPPORTED;
    }
    return plan_common(info, out, why, nullptr, 1);
}

int grk_amd::plan_t2_read_layers(const grk_amd_stream_info& info, T2ReadLayersPlan& out, const char** why, bool ht_refine)
{
    const char* dummy; if (!why) why = &dummy;
    *why = "";
    out = T2ReadLayersPlan{};
    if (!info.num_layers) { *why = "a file without layers"; return GRK_AMD_ERR_INVALID; }
    T2ReadPlan& B = out.base;
    B.ht = !info.base.reserved[0];
    out.layers = info.num_layers; out.sty = info.base.reserved[1]; out.order = (info.flags >> GRK_AMD_CS_PROG_SHIFT) & 7u;
    if (B.ht && ht_refine) out.sty |= kT2pStyHtRefine;         // (the parse core's option travels in the style word)
    const int rc = plan_common(info, B, why, &out.lpk, info.num_layers);
    if (rc) return rc;
    out.segments_per_row = t2p_max_segments(B.ht, out.sty);
    out.seg_records_per_row = t2p_max_seg_records(B.ht, out.sty, out.layers);
    out.piece_records_per_row = t2p_max_piece_records_sty(B.ht, out.sty, out.layers);
    // (node scratch at four bytes a node; the logs' and tables' entries are counted in 32 bits)
    if (B.node_bytes > 0x3FFFFFFFull || B.rows * out.seg_records_per_row > 0x7FFFFFFFull || B.rows * out.piece_records_per_row > 0x7FFFFFFFull ||
        B.rows * out.segments_per_row > 0x7FFFFFFFull) {
        *why = "tables beyond the device reader's 32-bit fields"; return GRK_AMD_ERR_UNSUPPORTED;
    }
    return GRK_AMD_OK;
}

int grk_amd::t2_read_tlm(const uint8_t* cs, uint64_t n, uint64_t len, uint32_t num_tiles, bool* have, std::vector<uint64_t>& offs, std::vector<uint32_t>& ln,
                         std::vector<uint32_t>& idx, uint64_t* count)
{
    *have = false; *count = 0;
    offs.clear(); ln.clear(); idx.clear();
    if (n > len) n = len;
    if (!cs || n < 4 || cs[0] != 0xFF || cs[1] != 0x4F) return GRK_AMD_ERR_INVALID;
    auto be16 = [&](uint64_t i) { return (uint32_t)(cs[i] << 8 | cs[i + 1]); };
    auto be32 = [&](uint64_t i) { return (uint32_t)cs[i] << 24 | (uint32_t)cs[i + 1] << 16 | (uint32_t)cs[i + 2] << 8 | cs[i + 3]; };
    std::vector<std::pair<uint32_t, uint32_t>> tlm;
    uint64_t at = 2;
    while (at + 4 <= n) {
        const uint32_t m = be16(at);
        if (m == 0xFF90) break;
        const uint32_t l = be16(at + 2);
        if (m < 0xFF00 || l < 2 || at + 2 + l > n) return GRK_AMD_ERR_INVALID;
        if (m == 0xFF55 && l >= 4) {
            *have = true;
            const uint32_t stlm = cs[at + 5], st = (stlm >> 4) & 3u, sp = (stlm >> 6) & 1u;
            const uint32_t rec = st + (sp ? 4u : 2u);
            if (st == 3) return GRK_AMD_ERR_INVALID;
            for (uint64_t q = at + 6; q + rec <= at + 2 + l; q += rec) tlm.emplace_back(st == 0 ? 0xFFFFFFFFu : st == 1 ? cs[q] : be16(q), sp ? be32(q + st) : be16(q + st));
        }
        at += 2 + l;
    }
    if (at + 12 > len || at + 2 > n || be16(at) != 0xFF90) return GRK_AMD_ERR_INVALID;
    if (!*have) return GRK_AMD_OK;
    uint32_t next = 0;
    for (const auto& e : tlm) {
        const uint32_t ti = e.first == 0xFFFFFFFFu ? next : e.first;
        if (at + e.second > len) return GRK_AMD_ERR_INVALID;
        if (*count < num_tiles) { offs.push_back(at); ln.push_back(e.second); idx.push_back(ti & 0xFFFFu); }
        ++*count; at += e.second; next = ti + 1;
    }
    return GRK_AMD_OK;
}
