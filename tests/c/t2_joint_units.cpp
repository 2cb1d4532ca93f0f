// tests/c/t2_joint_units.cpp -- the device writer's JOINT plan (t2_device_plan_joint, t2_order.h) and the tile classes of a
// sub-sampled image (joint_tile_classes), checked on the host: a stand-alone program for tests/test_t2_joint_plan_cpu.py, built with
// g++ together with geometry.cpp and t2_writer.cpp under -fsanitize=address,undefined -- no GPU, no HIP.
//
// For 4:2:0, 4:2:2, the factors (1,1),(2,1),(1,2) and a four-component (1,1),(2,2),(2,2),(1,1) image, in one tile and in ragged tiles
// with an image offset, over the five progression orders, every tile:
//   - the plan's packets are packet_order's sequence, each with its component's row0 and its precinct's band grids;
//   - every row of the tile lies in exactly one packet, and packet_of_block says which;
//   - row0 / first_block address the host writer's row order: the writer's own file of random lengths, made with PLT, carries every
//     packet's length, which must be the header the plan leaves room for plus the lengths of exactly the plan's rows;
//   - u_words / h_bytes bound what the host header writer produced for those lengths;
//   - tiles of one class (joint_tile_classes) have equal sequences and equal plans, tiles of different classes differ in a run's
//     geometry group or in their sequence.
// And the single-geometry t2_device_plan, now a call of the joint one, against a copy of the function it replaces, field by field.
// Prints "ok: N checks"; exit status 1 with the case on a failure.
#include "../../grok_amd/csrc/geometry.h"
#include "../../grok_amd/csrc/image.h"
#include "../../grok_amd/csrc/t2_order.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace grk_amd;

static long checks = 0;
static std::string where;
#define CHECK(cond) do { ++checks; if (!(cond)) { std::printf("FAILED %s:%d: %s -- %s\n", __FILE__, __LINE__, #cond, where.c_str()); std::exit(1); } } while (0)

struct Rng {
    uint64_t s;
    uint64_t next() { uint64_t z = (s += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
    uint32_t in(uint32_t lo, uint32_t hi) { return lo + (uint32_t)(next() % (uint64_t)(hi - lo + 1)); }
};

static int tag_tree_height(uint32_t gw, uint32_t gh)
{
    int h = 1;
    while ((uint64_t)gw * gh > 1) { gw = (gw + 1) >> 1; gh = (gh + 1) >> 1; ++h; }
    return h;
}

// the function t2_device_plan was before it became a call of the joint plan
static int old_t2_device_plan(const TileGeom& g, uint32_t flags, T2Plan& out)
{
    const grk_amd_tile_params& p = g.p;
    if (flags & GRK_AMD_CS_BLOCK_MSBS) return GRK_AMD_ERR_UNSUPPORTED;
    std::vector<const TileGeom*> cg(p.num_comps, &g);
    const std::vector<Pk> seq = packet_order(cg, nullptr, nullptr, p.tile_x0, p.tile_y0, (flags >> GRK_AMD_CS_PROG_SHIFT) & 7u);
    out.packets.clear();
    out.packet_of_block.assign((size_t)g.blocks_per_comp * p.num_comps, 0xFFFFFFFFu);
    uint64_t u = 0, h = 0;
    for (const Pk& q : seq) {
        const ResGeom& R = g.res[q.r];
        T2Packet k{};
        k.row0 = q.c * g.blocks_per_comp;
        uint64_t bits = 1;
        for (uint32_t bi = 0; bi < R.num_bands; ++bi) {
            const BandGeom& B = R.band[bi];
            const BandGeom::Prec& P = B.prec[q.pi];
            if (!P.gw || !P.gh) continue;
            const uint32_t b = k.nbands++;
            k.first_block[b] = P.first_block; k.gw[b] = P.gw; k.gh[b] = P.gh; k.kmax[b] = B.kmax;
            k.height[b] = (uint32_t)tag_tree_height(P.gw, P.gh);
            const uint64_t n = (uint64_t)P.gw * P.gh;
            for (uint64_t i = 0; i < n; ++i) out.packet_of_block[k.row0 + P.first_block + i] = (uint32_t)out.packets.size();
            k.nblocks += (uint32_t)n;
            bits += n * (2ull * k.height[b] + 1 + (kT2MaxLenBits - 3 + 1) + kT2MaxLenBits) + B.kmax;
        }
        if (bits > 0x7FFFFFFFull) return GRK_AMD_ERR_UNSUPPORTED;
        k.u_at = (uint32_t)u; k.u_words = (uint32_t)((bits + 31) / 32 + 2);
        k.h_at = (uint32_t)h;
        u += (k.u_words + 31u) & ~31ull;
        h += ((bits + 6) / 7 + 2 + 15) & ~15ull;
        if (u > 0x3FFFFFFFull || h > 0xFFFFFFFFull) return GRK_AMD_ERR_UNSUPPORTED;
        out.packets.push_back(k);
    }
    for (uint32_t v : out.packet_of_block) if (v == 0xFFFFFFFFu) return GRK_AMD_ERR_INVALID;
    out.u_words = (uint32_t)u; out.h_bytes = (uint32_t)h;
    return GRK_AMD_OK;
}

static bool same_plan(const T2Plan& a, const T2Plan& b)
{
    if (a.packets.size() != b.packets.size() || a.packet_of_block != b.packet_of_block || a.u_words != b.u_words || a.h_bytes != b.h_bytes) return false;
    for (size_t i = 0; i < a.packets.size(); ++i) {
        const T2Packet &x = a.packets[i], &y = b.packets[i];
        if (x.row0 != y.row0 || x.nbands != y.nbands || x.nblocks != y.nblocks || x.u_at != y.u_at || x.u_words != y.u_words || x.h_at != y.h_at) return false;
        for (int k = 0; k < 3; ++k)
            if (x.first_block[k] != y.first_block[k] || x.gw[k] != y.gw[k] || x.gh[k] != y.gh[k] || x.kmax[k] != y.kmax[k] || x.height[k] != y.height[k]) return false;
    }
    return true;
}

static grk_amd_tile_params params(uint32_t nc, uint32_t prec, uint32_t levels, uint32_t cbw, uint32_t cbh, uint32_t precinct, bool irreversible)
{
    grk_amd_tile_params p{};
    p.num_comps = (uint16_t)nc; p.prec = (uint8_t)prec; p.num_levels = (uint8_t)levels; p.cblk_w_exp = (uint8_t)cbw; p.cblk_h_exp = (uint8_t)cbh;
    p.irreversible = irreversible ? 1 : 0;
    for (uint32_t r = 0; precinct && r <= levels; ++r) p.precinct_exp[r] = (uint8_t)(precinct | precinct << 4);
    return p;
}

// a tile's components as the tile-part writer takes them
struct TileComps { std::vector<TileGeom> geoms; std::vector<const TileGeom*> cg; std::vector<uint64_t> row0; grk_amd_tile_params tile; uint64_t rows; };
static void comps_of(const grk_amd_image_layout& im, const grk_amd_tile_params& base, const std::vector<uint8_t>& dx, const std::vector<uint8_t>& dy,
                     uint32_t t, TileComps& tc)
{
    const uint32_t nc = base.num_comps;
    CHECK(grk_amd_layout_tile(&im, &base, t, &tc.tile) == GRK_AMD_OK);
    tc.geoms.assign(nc, TileGeom{}); tc.cg.assign(nc, nullptr); tc.row0.assign(nc, 0); tc.rows = 0;
    for (uint32_t c = 0; c < nc; ++c) {
        grk_amd_tile_params p{};
        CHECK(grk_amd_layout_tile_comp(&im, &base, dx[c], dy[c], t, &p) == GRK_AMD_OK);
        CHECK(build_tile_geom(p, tc.geoms[c]) == GRK_AMD_OK);
        tc.cg[c] = &tc.geoms[c]; tc.row0[c] = tc.rows; tc.rows += tc.geoms[c].blocks_per_comp;
    }
}

// a codestream's tile-parts: per tile the PLT's packet lengths
static std::vector<std::vector<uint64_t>> plt_of(const std::vector<uint8_t>& cs, uint32_t ntiles)
{
    auto be16 = [&](size_t i) { return (uint32_t)(cs[i] << 8 | cs[i + 1]); };
    auto be32 = [&](size_t i) { return (uint32_t)cs[i] << 24 | (uint32_t)cs[i + 1] << 16 | (uint32_t)cs[i + 2] << 8 | cs[i + 3]; };
    size_t at = 2;
    while (be16(at) != 0xFF90) at += 2 + be16(at + 2);
    std::vector<std::vector<uint64_t>> out(ntiles);
    for (uint32_t t = 0; t < ntiles; ++t) {
        CHECK(be16(at) == 0xFF90 && be16(at + 4) == t);
        const size_t next = at + be32(at + 6);
        size_t q = at + 12;
        while (be16(q) == 0xFF58) {
            const size_t end = q + 2 + be16(q + 2);
            uint64_t v = 0;
            for (size_t i = q + 5; i < end; ++i) { v = v << 7 | (cs[i] & 0x7Fu); if (!(cs[i] & 0x80u)) { out[t].push_back(v); v = 0; } }
            q = end;
        }
        CHECK(be16(q) == 0xFF93);
        at = next;
    }
    CHECK(be16(at) == 0xFFD9);
    return out;
}

static uint32_t floor_log2(uint32_t v) { uint32_t r = 0; while (v >>= 1) ++r; return r; }

static long classes_seen_max = 0;

static void image_case(const char* name, grk_amd_image_layout im, grk_amd_tile_params base, std::vector<uint8_t> dx, std::vector<uint8_t> dy, Rng& R)
{
    const uint32_t nc = base.num_comps;
    const int64_t nt = grk_amd_layout_num_tiles(&im);
    CHECK(nt > 0);
    const uint32_t ntiles = (uint32_t)nt;
    // the units and groups as subsampled_image makes them: tile by tile, run by run
    const std::vector<CompRun> runs = comp_runs(nc, base.mct != 0, dx.data(), dy.data());
    const uint32_t nr = (uint32_t)runs.size();
    UnitGroups g;
    for (uint32_t t = 0; t < ntiles; ++t)
        for (uint32_t k = 0; k < nr; ++k) {
            grk_amd_tile_params p{};
            CHECK(grk_amd_layout_tile_comp(&im, &base, dx[runs[k].first], dy[runs[k].first], t, &p) == GRK_AMD_OK);
            p.num_comps = (uint16_t)runs[k].count; p.mct = runs[k].mct ? 1 : 0;
            CHECK(add_unit(g, p) == GRK_AMD_OK);
        }
    for (uint32_t order = 0; order < 5; ++order) {
        where = std::string(name) + ", order " + std::to_string(order);
        const uint32_t flags = order << GRK_AMD_CS_PROG_SHIFT;
        std::vector<TileComps> tcs(ntiles);
        std::vector<T2Plan> plans(ntiles);
        std::vector<std::vector<Pk>> seq(ntiles);
        // random lengths in the writer's row order, every block's bytes at offset 0 of a buffer of zeros
        std::vector<grk_amd_coded_block> rows;
        std::vector<uint64_t> tile_row(ntiles + 1, 0);
        uint32_t big = 0;
        for (uint32_t t = 0; t < ntiles; ++t) {
            comps_of(im, base, dx, dy, t, tcs[t]);
            seq[t] = packet_order(tcs[t].cg, dx.data(), dy.data(), tcs[t].tile.tile_x0, tcs[t].tile.tile_y0, order);
            CHECK(t2_device_plan_joint(tcs[t].cg, tcs[t].row0, dx.data(), dy.data(), tcs[t].tile.tile_x0, tcs[t].tile.tile_y0, flags, plans[t]) == GRK_AMD_OK);
            CHECK(t2_device_plan_joint(tcs[t].cg, tcs[t].row0, dx.data(), dy.data(), tcs[t].tile.tile_x0, tcs[t].tile.tile_y0, flags | GRK_AMD_CS_BLOCK_MSBS, plans[t]) == GRK_AMD_ERR_UNSUPPORTED);
            tile_row[t + 1] = tile_row[t] + tcs[t].rows;
            for (uint64_t i = 0; i < tcs[t].rows; ++i) {
                const uint32_t kind = R.in(0, 15);
                uint32_t len = kind == 0 ? 0 : kind < 6 ? R.in(1, 7) : kind < 14 ? R.in(8, 4000) : R.in(4001, 70000);
                if (kind == 15 && big < 3) { len = R.in(1u << 19, (1u << 20) - 1); ++big; }
                rows.push_back(grk_amd_coded_block{0, len, 0});
            }
        }
        std::vector<uint8_t> coded(1u << 20, 0);
        uint64_t sum = 0;
        for (const auto& r : rows) sum += r.length;
        std::vector<uint8_t> cs(sum + rows.size() * 16 + ntiles * 4096 + (1u << 16));
        const int64_t n = grk_amd_write_codestream_subsampled(&im, &base, dx.data(), dy.data(), rows.data(), coded.data(), flags | GRK_AMD_CS_PLT, cs.data(), cs.size());
        CHECK(n > 0);
        cs.resize((size_t)n);
        const std::vector<std::vector<uint64_t>> plt = plt_of(cs, ntiles);
        for (uint32_t t = 0; t < ntiles; ++t) {
            where = std::string(name) + ", order " + std::to_string(order) + ", tile " + std::to_string(t);
            const T2Plan& pl = plans[t];
            const TileComps& tc = tcs[t];
            CHECK(pl.packets.size() == seq[t].size() && plt[t].size() == seq[t].size());
            CHECK(pl.packet_of_block.size() == tc.rows);
            std::vector<uint32_t> covered(tc.rows, 0);
            for (size_t i = 0; i < seq[t].size(); ++i) {
                const Pk& q = seq[t][i];
                const T2Packet& k = pl.packets[i];
                const TileGeom& G = *tc.cg[q.c];
                const ResGeom& Rg = G.res[q.r];
                CHECK(k.row0 == tc.row0[q.c]);
                uint32_t b = 0, nblocks = 0;
                uint64_t body = 0, bits = 1;
                for (uint32_t bi = 0; bi < Rg.num_bands; ++bi) {
                    const BandGeom::Prec& P = Rg.band[bi].prec[q.pi];
                    if (!P.gw || !P.gh) continue;
                    CHECK(b < k.nbands && k.first_block[b] == P.first_block && k.gw[b] == P.gw && k.gh[b] == P.gh && k.kmax[b] == Rg.band[bi].kmax);
                    CHECK(k.height[b] == (uint32_t)tag_tree_height(P.gw, P.gh));
                    for (uint32_t j = 0; j < P.gw * P.gh; ++j) {
                        const uint64_t row = (uint64_t)k.row0 + P.first_block + j;
                        CHECK(row < tc.rows);
                        ++covered[row];
                        CHECK(pl.packet_of_block[row] == i);
                        const uint32_t len = rows[tile_row[t] + row].length, x = j % P.gw, y = j / P.gw, m = x | y;
                        body += len;
                        // the block's header bits as the writer's comments give them (t2_writer.cpp: tag trees as this writer meets them)
                        const uint32_t nn = m ? std::min((uint32_t)__builtin_ctz(m) + 1u, k.height[b]) : k.height[b];
                        const uint32_t fl = len ? floor_log2(len) : 0, inc = fl + 1 > 3 ? fl + 1 - 3 : 0;
                        bits += 2 * nn + (j == 0 ? k.kmax[b] - 1u : 0u) + 1 + (inc + 1) + (3 + inc);
                    }
                    nblocks += P.gw * P.gh;
                    ++b;
                }
                CHECK(b == k.nbands && nblocks == k.nblocks);
                // the host writer's packet: its PLT length less the rows the plan says it holds is its header
                CHECK(plt[t][i] >= body);
                const uint64_t hdr = plt[t][i] - body;
                CHECK(hdr >= (bits + 7) / 8 && hdr <= (bits + 6) / 7 + 1);             // (the formula above is the writer's)
                const uint64_t room = (i + 1 < pl.packets.size() ? pl.packets[i + 1].h_at : pl.h_bytes) - k.h_at;
                CHECK(hdr <= room && k.h_at % 16 == 0);
                CHECK(bits + 64 <= 32ull * k.u_words);                                 // (put_bits touches up to two words behind a string's first)
                CHECK((uint64_t)k.u_at + k.u_words <= (i + 1 < pl.packets.size() ? pl.packets[i + 1].u_at : pl.u_words) && k.u_at % 32 == 0);
            }
            for (uint32_t v : covered) CHECK(v == 1);
        }
        // classes
        where = std::string(name) + ", order " + std::to_string(order) + ", classes";
        std::vector<uint32_t> class_of;
        const uint32_t ncl = joint_tile_classes(g.of, nr, order, order >= 2 ? seq : std::vector<std::vector<Pk>>(), class_of);
        classes_seen_max = std::max<long>(classes_seen_max, ncl);
        CHECK(class_of.size() == ntiles && ncl >= 1);
        auto same_seq = [&](uint32_t a, uint32_t b) {
            if (seq[a].size() != seq[b].size()) return false;
            for (size_t i = 0; i < seq[a].size(); ++i) if (seq[a][i].c != seq[b][i].c || seq[a][i].r != seq[b][i].r || seq[a][i].pi != seq[b][i].pi) return false;
            return true;
        };
        auto same_groups = [&](uint32_t a, uint32_t b) {
            for (uint32_t k = 0; k < nr; ++k) if (g.of[(size_t)a * nr + k] != g.of[(size_t)b * nr + k]) return false;
            return true;
        };
        for (uint32_t a = 0; a < ntiles; ++a)
            for (uint32_t b = a + 1; b < ntiles; ++b) {
                if (class_of[a] == class_of[b]) { CHECK(same_seq(a, b) && same_groups(a, b) && same_plan(plans[a], plans[b])); }
                else CHECK(!same_seq(a, b) || !same_groups(a, b));
            }
    }
}

static void single_geometry_cases()
{
    const uint32_t sizes[][4] = {{64, 48, 0, 0}, {101, 77, 0, 0}, {130, 66, 6, 10}, {200, 136, 13, 74}, {17, 200, 3, 17}, {256, 256, 0, 0}};
    for (const auto& s : sizes)
        for (uint32_t nc : {1u, 3u, 4u})
            for (uint32_t levels : {0u, 1u, 2u, 5u})
                for (uint32_t precinct : {0u, 5u, 7u})
                    for (uint32_t cb : {2u, 4u, 6u})
                        for (uint32_t order = 0; order < 5; ++order)
                            for (bool irr : {false, true}) {
                                grk_amd_tile_params p = params(nc, 8, levels, cb, cb == 4 ? 5 : cb, precinct, irr);
                                if (cb == 2 && s[0] * s[1] > 130 * 66) continue;       // (4 x 4 blocks of the large tiles: slow, nothing new)
                                p.tile_w = s[0]; p.tile_h = s[1]; p.tile_x0 = s[2]; p.tile_y0 = s[3];
                                where = "single geometry " + std::to_string(s[0]) + "x" + std::to_string(s[1]) + " comps " + std::to_string(nc) + " levels " +
                                        std::to_string(levels) + " precinct " + std::to_string(precinct) + " cb " + std::to_string(cb) + " order " + std::to_string(order);
                                TileGeom g;
                                if (build_tile_geom(p, g) != GRK_AMD_OK) continue;
                                T2Plan a, b;
                                const uint32_t flags = order << GRK_AMD_CS_PROG_SHIFT | GRK_AMD_CS_SOP;
                                const int ra = old_t2_device_plan(g, flags, a), rb = t2_device_plan(g, flags, b);
                                CHECK(ra == rb);
                                if (ra == GRK_AMD_OK) CHECK(same_plan(a, b));
                                CHECK(t2_device_plan(g, flags | GRK_AMD_CS_BLOCK_MSBS, b) == GRK_AMD_ERR_UNSUPPORTED);
                            }
}

int main()
{
    Rng R{20261020};
    struct Factors { const char* name; std::vector<uint8_t> dx, dy; };
    const Factors factors[] = {{"4:2:0", {1, 2, 2}, {1, 2, 2}}, {"4:2:2", {1, 2, 2}, {1, 1, 1}}, {"(1,1),(2,1),(1,2)", {1, 2, 1}, {1, 1, 2}},
                               {"Y/CbCr/A", {1, 2, 2, 1}, {1, 2, 2, 1}}};
    for (const Factors& f : factors) {
        const uint32_t nc = (uint32_t)f.dx.size();
        // one tile: 64 x 48 with 2 levels; 101 x 77 with 5 (chroma bands empty at the deep levels: packets without blocks)
        image_case((std::string(f.name) + " 64x48").c_str(), grk_amd_image_layout{0, 0, 64, 48, 0, 0, 64, 48}, params(nc, 8, 2, 6, 6, 0, false), f.dx, f.dy, R);
        image_case((std::string(f.name) + " 101x77").c_str(), grk_amd_image_layout{0, 0, 101, 77, 0, 0, 101, 77}, params(nc, 8, 5, 4, 4, 0, false), f.dx, f.dy, R);
        // ragged tiles of 96 x 64 under an image offset, with and without small precincts
        image_case((std::string(f.name) + " 200x136 at (6,10)").c_str(), grk_amd_image_layout{6, 10, 206, 146, 0, 0, 96, 64}, params(nc, 8, 3, 5, 5, 0, false), f.dx, f.dy, R);
        image_case((std::string(f.name) + " 200x136 at (6,10), precincts 32").c_str(), grk_amd_image_layout{6, 10, 206, 146, 0, 0, 96, 64}, params(nc, 10, 2, 4, 4, 5, true), f.dx, f.dy, R);
        image_case((std::string(f.name) + " 128x128 precincts 32").c_str(), grk_amd_image_layout{0, 0, 128, 128, 0, 0, 128, 128}, params(nc, 8, 3, 4, 4, 5, false), f.dx, f.dy, R);
    }
    where = "classes";
    CHECK(classes_seen_max >= 3);                            // (the ragged layouts really have several)
    single_geometry_cases();
    std::printf("ok: %ld checks\n", checks);
    return 0;
}
