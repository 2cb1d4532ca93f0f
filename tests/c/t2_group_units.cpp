// tests/c/t2_group_units.cpp -- what a geometry group shares, checked for EVERY member of the group: a small driver for
// tests/test_t2_group_plan_cpu.py, built at test time with g++ together with geometry.cpp and t2_writer.cpp, no GPU, no HIP.
//
// The whole-image encoders group their tiles with add_unit (image.h) and have grk_amd_assemble_device frame each group with ONE
// t2_device_plan, the group leader's.  Here every tile's OWN plan is built (build_tile_geom of the tile's own parameters) and
// compared with its leader's, the groups coming from add_unit itself -- called as plain_image calls it, with the progression order.
#include "../../grok_amd/csrc/geometry.h"
#include "../../grok_amd/csrc/image.h"
#include "../../grok_amd/csrc/t2_order.h"
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

using namespace grk_amd;

namespace {

// a tile's plan as words: per packet row0, nbands, first_block[3], gw[3], gh[3], kmax[3]; then packet_of_block; then u_words, h_bytes
void flatten(const T2Plan& pl, std::vector<uint32_t>& f)
{
    f.clear();
    f.reserve(pl.packets.size() * 14 + pl.packet_of_block.size() + 2);
    for (const T2Packet& k : pl.packets) {
        f.push_back(k.row0); f.push_back(k.nbands);
        for (int b = 0; b < 3; ++b) f.push_back(k.first_block[b]);
        for (int b = 0; b < 3; ++b) f.push_back(k.gw[b]);
        for (int b = 0; b < 3; ++b) f.push_back(k.gh[b]);
        for (int b = 0; b < 3; ++b) f.push_back(k.kmax[b]);
    }
    f.insert(f.end(), pl.packet_of_block.begin(), pl.packet_of_block.end());
    f.push_back(pl.u_words); f.push_back(pl.h_bytes);
}

struct Tiles { std::vector<grk_amd_tile_params> p; std::vector<TileGeom> g; };

int tiles_of(const grk_amd_image_layout* im, const grk_amd_tile_params* base, Tiles& T)
{
    const int64_t nt = grk_amd_layout_num_tiles(im);
    if (nt < 0) return (int)nt;
    T.p.assign((size_t)nt, grk_amd_tile_params{});
    T.g.assign((size_t)nt, TileGeom{});
    for (uint32_t t = 0; t < (uint32_t)nt; ++t) {
        int rc = grk_amd_layout_tile(im, base, t, &T.p[t]);
        if (!rc) rc = build_tile_geom(T.p[t], T.g[t]);
        if (rc) return rc;
    }
    return GRK_AMD_OK;
}

// the groups as plain_image makes them (image.cpp): add_unit, tile after tile, with the progression order of the flags
int groups_of(const Tiles& T, uint32_t flags, UnitGroups& g)
{
    for (const grk_amd_tile_params& p : T.p) {
        const int rc = add_unit(g, p, (flags >> GRK_AMD_CS_PROG_SHIFT) & 7u);
        if (rc) return rc;
    }
    return GRK_AMD_OK;
}

// the (c, r, precinct) sequence of a tile's packets, one word per packet
std::vector<uint64_t> sequence(const TileGeom& g, uint32_t order)
{
    const std::vector<const TileGeom*> cg(g.p.num_comps, &g);
    std::vector<uint64_t> s;
    for (const Pk& q : packet_order(cg, nullptr, nullptr, g.p.tile_x0, g.p.tile_y0, order))
        s.push_back((uint64_t)q.c << 56 | (uint64_t)q.r << 48 | q.pi);
    return s;
}

struct Rng {
    uint64_t s;
    uint64_t next() { uint64_t z = (s += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
    uint32_t in(uint32_t lo, uint32_t hi) { return lo + (uint32_t)(next() % (uint64_t)(hi - lo + 1)); }       // lo .. hi
};

} // namespace

extern "C" {

// Every tile of the layout: group[t] = its group (add_unit under the order of `flags`), its own plan flattened into flat[flat_at[t] ..
// flat_at[t + 1]) (flat == NULL, or too small: the sizes alone).  Returns the number of tiles, or an error.
int64_t t2g_layout(const grk_amd_image_layout* im, const grk_amd_tile_params* base, uint32_t flags, uint32_t* group, uint32_t* flat,
                   uint64_t flat_cap, uint64_t* flat_at)
{
    Tiles T;
    int rc = tiles_of(im, base, T);
    if (rc) return rc;
    UnitGroups g;
    if ((rc = groups_of(T, flags, g))) return rc;
    std::copy(g.of.begin(), g.of.end(), group);
    uint64_t at = 0;
    std::vector<uint32_t> f;
    for (size_t t = 0; t < T.p.size(); ++t) {
        T2Plan pl;
        if ((rc = t2_device_plan(T.g[t], flags, pl))) return rc;
        flatten(pl, f);
        flat_at[t] = at;
        if (flat && at + f.size() <= flat_cap) std::copy(f.begin(), f.end(), flat + at);
        at += f.size();
    }
    flat_at[T.p.size()] = at;
    return (int64_t)T.p.size();
}

// 1 when the (c, r, precinct) sequences of the two tiles' packets are the same under `order` (packet_order itself, not the predicate)
int t2g_same_sequence(const grk_amd_tile_params* a, const grk_amd_tile_params* b, uint32_t order)
{
    TileGeom ga, gb;
    int rc = build_tile_geom(*a, ga); if (rc) return rc;
    rc = build_tile_geom(*b, gb); if (rc) return rc;
    return sequence(ga, order) == sequence(gb, order) ? 1 : 0;
}

// The sweep.  `draws` layouts from `seed`: image offsets and tile-grid offsets (kind 0: everything at the origin, 1: image offset only,
// 2: tile-grid offset equal to the image offset, 3: both, different), 1 and 3 components, 1..5 levels, code-block exponents 2..6,
// precinct exponents 1..8 (one pair for all resolutions, or one per resolution; square or not), tile sides from half a precinct to
// twelve precincts of the top resolution (at most 300) and seldom a multiple of the precinct size, up to 6 x 6 cells; layouts of more
// than `max_tiles` tiles are dropped.  For every kept layout and every progression order:
//   - every tile's own plan against its group leader's                                                  -> out[8 + order] mismatches
//   - orders 0, 1, and all five for kind 0: the groups are same_geometry's                              -> out[13 + order] pairs that are not
//   - grk_amd_same_tile_packets(a, b) == same_geometry(a, b) && the sequences are equal                 -> out[18] pairs where not
// out[0] kept layouts, out[1..4] kept layouts of kind 0..3, out[5] pairs of tiles that same_geometry accepts, out[6] those of them whose
// PCRL sequences agree, out[7] whose PCRL sequences differ, out[19] / out[20] the same for RPCL and CPRL, out[21] layouts that failed
// to build.  `msg`: the first failure, enough to reproduce it.  Returns 0, or the first build error's code with out[21] set.
int t2g_sweep(uint64_t seed, uint32_t draws, uint32_t max_tiles, uint64_t* out, char* msg, uint32_t msg_cap)
{
    std::fill(out, out + 24, 0);
    if (msg_cap) msg[0] = 0;
    Rng R{seed};
    int first_err = 0;
    auto note = [&](const char* what, const grk_amd_image_layout& im, const grk_amd_tile_params& b, uint32_t order, uint32_t ta, uint32_t tb) {
        if (!msg_cap || msg[0]) return;
        std::string pe;
        for (uint32_t r = 0; r <= b.num_levels; ++r) pe += (r ? "," : "") + std::to_string(b.precinct_exp[r] & 15) + "/" + std::to_string(b.precinct_exp[r] >> 4);
        std::snprintf(msg, msg_cap, "%s: order %u, tiles %u and %u of image [%u,%u) x [%u,%u), tile grid at (%u,%u), tiles %u x %u, %u components, "
                      "%u levels, code-block exponents %u/%u, precinct exponents %s", what, order, ta, tb, im.x0, im.x1, im.y0, im.y1, im.tx0, im.ty0,
                      im.t_width, im.t_height, (unsigned)b.num_comps, (unsigned)b.num_levels, (unsigned)b.cblk_w_exp, (unsigned)b.cblk_h_exp, pe.c_str());
    };
    for (uint32_t d = 0; d < draws; ++d) {
        grk_amd_tile_params b{};
        b.num_comps = R.in(0, 1) ? 3 : 1;
        b.prec = 8; b.mct = b.num_comps == 3;
        b.num_levels = (uint8_t)(R.in(0, 3) ? R.in(1, 3) : R.in(4, 5));               // few levels more often
        b.cblk_w_exp = (uint8_t)R.in(2, 6); b.cblk_h_exp = (uint8_t)R.in(2, 6);
        // small precincts more often: the top resolution's exponents, then the others'
        uint32_t ppx = R.in(0, 2) ? R.in(1, 4) : R.in(5, 8), ppy = R.in(0, 1) ? ppx : (R.in(0, 2) ? R.in(1, 4) : R.in(5, 8));
        const bool per_res = R.in(0, 3) == 0;
        for (uint32_t r = 0; r <= b.num_levels; ++r) {
            uint32_t x = ppx, y = ppy;
            if (per_res && r < b.num_levels) { x = R.in(1, 8); y = R.in(0, 1) ? x : R.in(1, 8); }
            b.precinct_exp[r] = (uint8_t)(x | y << 4);
        }
        const uint32_t kind = R.in(0, 7) == 0 ? 0 : R.in(1, 3);
        grk_amd_image_layout im{};
        im.t_width = R.in(std::max(2u, (1u << ppx) / 2), std::min(300u, 12u << ppx));
        im.t_height = R.in(std::max(2u, (1u << ppy) / 2), std::min(300u, 12u << ppy));
        if (kind == 2 || kind == 3) { im.tx0 = R.in(1, 300); im.ty0 = R.in(1, 300); }
        im.x0 = im.tx0; im.y0 = im.ty0;
        if (kind == 1 || kind == 3) {                                                   // inside the first cell, off its corner
            im.x0 += R.in(0, im.t_width - 1); im.y0 += R.in(0, im.t_height - 1);
            if (im.x0 == im.tx0 && im.y0 == im.ty0) { if (im.t_width > 1) im.x0 += 1; else im.y0 += 1; }
        }
        const uint32_t cols = R.in(1, 6), rows = R.in(1, 6);
        im.x1 = im.tx0 + (cols - 1) * im.t_width + R.in(1, im.t_width);
        im.y1 = im.ty0 + (rows - 1) * im.t_height + R.in(1, im.t_height);
        if (im.x1 <= im.x0 || im.y1 <= im.y0) continue;
        const int64_t nt = grk_amd_layout_num_tiles(&im);
        if (nt < 1 || nt > (int64_t)max_tiles) continue;
        Tiles T;
        int rc = tiles_of(&im, &b, T);
        if (rc) { ++out[21]; if (!first_err) { first_err = rc; note("a tile's geometry failed to build", im, b, 0, 0, 0); } continue; }
        ++out[0]; ++out[1 + kind];
        const uint32_t n = (uint32_t)nt;
        std::vector<uint8_t> sg((size_t)n * n, 0);                                       // same_geometry, pair by pair
        for (uint32_t a = 0; a < n; ++a)
            for (uint32_t c = a + 1; c < n; ++c) sg[(size_t)a * n + c] = same_geometry(T.g[a], T.g[c]) ? 1 : 0;
        for (uint32_t order = 0; order < 5; ++order) {
            const uint32_t flags = order << GRK_AMD_CS_PROG_SHIFT;
            UnitGroups g;
            if ((rc = groups_of(T, flags, g))) return rc;
            std::vector<std::vector<uint32_t>> plans(n);
            for (uint32_t t = 0; t < n; ++t) {
                T2Plan pl;
                if ((rc = t2_device_plan(T.g[t], flags, pl))) return rc;
                flatten(pl, plans[t]);
            }
            for (uint32_t t = 0; t < n; ++t) {
                const uint32_t lead = g.members[g.of[t]][0];
                if (plans[t] != plans[lead]) { ++out[8 + order]; note("a member's plan is not its group leader's", im, b, order, lead, t); }
            }
            std::vector<std::vector<uint64_t>> seq(n);
            for (uint32_t t = 0; t < n; ++t) seq[t] = sequence(T.g[t], order);
            for (uint32_t a = 0; a < n; ++a)
                for (uint32_t c = a + 1; c < n; ++c) {
                    const bool geo = sg[(size_t)a * n + c] != 0, same_seq = seq[a] == seq[c];
                    if ((order <= 1 || kind == 0) && (g.of[a] == g.of[c]) != geo) {
                        ++out[13 + order]; note("the groups are not same_geometry's", im, b, order, a, c);
                    }
                    if (!geo && order != 3) continue;             // (the predicate on pairs of different geometry: under one order)
                    const int pred = grk_amd_same_tile_packets(&T.p[a], &T.p[c], flags);
                    if (pred != (geo && same_seq ? 1 : 0)) { ++out[18]; note("grk_amd_same_tile_packets disagrees with the sequences", im, b, order, a, c); }
                    if (!geo) continue;
                    if (order == 0) ++out[5];
                    if (order == 3) ++out[same_seq ? 6 : 7];
                    if (order == 2 && !same_seq) ++out[19];
                    if (order == 4 && !same_seq) ++out[20];
                }
        }
    }
    return first_err;
}

} // extern "C"
