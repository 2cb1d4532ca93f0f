// tests/c/t2_msbs_units.cpp -- a packet header under the GENERAL zero-bit-plane tag tree as the device writer composes it
// (grok_amd/csrc/t2_bits.h: t2_block_bits_msbs / t2_msbs_one_at / t2_tree_nodes, what KT1's msbs instance of kernels_t2.hip uses)
// against the host writer's own (ZbpTree and HeaderBits of t2_writer.cpp, included here as it is, with block_msbs = true): a stand-alone
// program for tests/test_t2_msbs_cpu.py, built with g++ under -fsanitize=address,undefined -- no GPU, no HIP.
//
// The sweep: the grids 1x1, 1xn, nx1, 2x2, 3x5, 41x35 and a row of 256 blocks (a tree of nine levels); per grid the value patterns
// constant (0, 11, 63), uniform random 0 .. 63, raster-rising and raster-falling (every node's minimum at its first / last leaf), one
// leaf at 0 among 63s and one at 63 among 0s at the first, a middle and the last leaf; per table the lengths 0, the limit - 1 and every
// 2^k - 1, 2^k, 2^k + 1 below the limit, dealt over the blocks in turn.  Per case the node values are built as the kernel builds them
// (level 0 the rows' bytes, every level above the minimum of up to 2 x 2 children), every block's pieces go through put_bits as the
// kernel has it (plain ORs) into zeroed words, and the words, stuffed by a plain sequential writer, must be the host writer's header.
// With every leaf at Kmax - 1 the words must also be those of t2_block_bits' pieces.
//
// The plan's units: for each of those grids -- a tile of 4x4 code-blocks without a DWT level -- t2_device_plan_msbs gives the packet at
// least the raw bits and node bytes the sweep used; the unchanged t2_device_plan refuses the flag.  Prints "ok: N checks".
#include "../../grok_amd/csrc/t2_writer.cpp"
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>

static long checks = 0;
static char where[240];
#define CHECK(cond) do { ++checks; if (!(cond)) { std::printf("FAILED %s:%d: %s -- %s\n", __FILE__, __LINE__, #cond, where); std::exit(1); } } while (0)

// put_bits of kernels_t2.hip, on the host: n <= 64 bits of v, MSB first, at bit `pos`
static void put_bits(uint32_t* u, uint32_t pos, uint64_t v, uint32_t n)
{
    if (!n) return;
    const uint64_t a = v << (64 - n);
    const uint32_t o = pos & 31u;
    uint32_t* w = u + (pos >> 5);
    const uint32_t w0 = (uint32_t)(a >> 32) >> o, w1 = (uint32_t)(a >> o), w2 = o ? (uint32_t)(a << (32 - o)) : 0u;
    w[0] |= w0; w[1] |= w1; w[2] |= w2;
}

// raw bits -> bytes: a byte behind an 0xFF takes seven bits; the last byte padded with zeros, an empty byte behind a final 0xFF
static std::vector<uint8_t> stuff(const uint32_t* u, uint32_t nbits)
{
    std::vector<uint8_t> out;
    uint32_t cur = 0, have = 0, room = 8;
    for (uint32_t i = 0; i < nbits; ++i) {
        cur = (cur << 1) | ((u[i >> 5] >> (31u - (i & 31u))) & 1u);
        if (++have == room) { out.push_back((uint8_t)cur); room = cur == 0xFFu ? 7 : 8; cur = 0; have = 0; }
    }
    if (have) out.push_back((uint8_t)(cur << (room - have)));
    else if (room == 7) out.push_back(0);
    return out;
}

// the node values as KT1's general instance lays them out: level 0 first, every level behind the one below it
struct Nodes {
    std::vector<uint8_t> v; std::vector<uint32_t> at, w, h;
    Nodes(const std::vector<uint32_t>& leaves, uint32_t gw, uint32_t gh)
    {
        v.assign((size_t)t2_tree_nodes(gw, gh), 0xFF);
        for (size_t i = 0; i < leaves.size(); ++i) v[i] = (uint8_t)std::min(leaves[i], kT2MaxMsbs);
        uint32_t from = 0, cw = gw, ch = gh;
        at.push_back(0); w.push_back(gw); h.push_back(gh);
        while ((uint64_t)cw * ch > 1) {
            const uint32_t nw = (cw + 1) >> 1, nh = (ch + 1) >> 1, to = from + cw * ch;
            for (uint32_t i = 0; i < nw * nh; ++i) {
                const uint32_t x = 2 * (i % nw), y = 2 * (i / nw);
                uint32_t m = v[from + y * cw + x];
                if (x + 1 < cw) m = std::min<uint32_t>(m, v[from + y * cw + x + 1]);
                if (y + 1 < ch) {
                    m = std::min<uint32_t>(m, v[from + (y + 1) * cw + x]);
                    if (x + 1 < cw) m = std::min<uint32_t>(m, v[from + (y + 1) * cw + x + 1]);
                }
                v[to + i] = (uint8_t)m;
            }
            from = to; cw = nw; ch = nh;
            at.push_back(from); w.push_back(cw); h.push_back(ch);
        }
    }
    uint32_t get(uint32_t l, uint32_t x, uint32_t y) const { return v[at[l] + (y >> l) * w[l] + (x >> l)]; }
};

struct Used { uint32_t bits = 0; uint64_t nodes = 0; bool over64 = false, late_min = false; };

// one table on one grid -> what it used
static void one_table(uint32_t gw, uint32_t gh, const std::vector<uint32_t>& vals, const std::vector<uint32_t>& lens, Used& used)
{
    const uint32_t n = gw * gh, height = (uint32_t)tag_tree_height(gw, gh);
    std::vector<grk_amd_coded_block> cb(n);
    for (uint32_t i = 0; i < n; ++i) cb[i] = grk_amd_coded_block{0, lens[i], vals[i]};
    // the host writer, as write_packet codes a band with block_msbs
    std::vector<uint8_t> want((size_t)n * 24 + 16);
    Out o{want.data(), want.size()};
    HeaderBits hb(o);
    hb.bit(1);
    ZbpTree zbp(cb.data(), gw, gh);
    for (uint32_t y = 0; y < gh; ++y)
        for (uint32_t x = 0; x < gw; ++x) {
            const uint32_t len = cb[y * gw + x].length;
            hb.ones(new_nodes(x, y, (int)height));
            zbp.code(hb, x, y);
            int inc = floor_log2(len) + 1 - 3;
            if (inc < 0) inc = 0;
            hb.put(0, 1); hb.comma(inc); hb.put(len, 3 + inc);
        }
    hb.flush();
    CHECK(!o.ovf);
    // the device writer's arithmetic
    const Nodes nd(vals, gw, gh);
    // (a grid one block wide or high halves along one side only: its levels hold up to 2 n nodes, not 4 n / 3 -- the plan counts them)
    CHECK(nd.at.size() == height && nd.v.size() < 2 * (size_t)n + height);
    const uint64_t bound = 1 + (uint64_t)n * (2 * height + 1 + (kT2MaxLenBits - 3 + 1) + kT2MaxLenBits + kT2MaxMsbs);
    std::vector<uint32_t> u((size_t)(bound + 31) / 32 + 3, 0u);
    uint32_t pos = 0;
    put_bits(u.data(), pos, 1, 1); pos += 1;
    for (uint32_t k = 0; k < n; ++k) {
        const uint32_t x = k % gw, y = k / gw, len = lens[k];
        CHECK(t2_len_ok(len));
        const uint32_t nn = (uint32_t)new_nodes(x, y, (int)height);
        const uint32_t vp = nn < height ? nd.get(nn, x, y) : 0xDEADu;       // (not read above the root)
        const T2MsbsBits mb = t2_block_bits_msbs(x, y, height, nd.get(0, x, y), vp, len);
        CHECK(mb.nn == nn && mb.tail_n >= 5 && mb.tail_n <= 39 && mb.nbits >= 2 * nn + mb.tail_n);
        CHECK(pos + mb.nbits <= bound);
        put_bits(u.data(), pos, (1ull << mb.nn) - 1ull, mb.nn);
        uint32_t below = mb.nbits - mb.tail_n;                               // every one stands in front of the one of the level below
        for (uint32_t l = 0; l < mb.nn; ++l) {
            const uint32_t q = t2_msbs_one_at(mb, l, nd.get(l, x, y));
            CHECK(q >= mb.nn && q < below);
            put_bits(u.data(), pos + q, 1, 1);
            below = q;
            if (l + 1 < height && nd.get(l + 1, x, y) == nd.get(l, x, y) && (((x >> l) | (y >> l)) & 1u)) used.late_min = true;
        }
        put_bits(u.data(), pos + mb.nbits - mb.tail_n, mb.tail, mb.tail_n);
        used.over64 = used.over64 || mb.nbits > 64;
        pos += mb.nbits;
    }
    const std::vector<uint8_t> got = stuff(u.data(), pos);
    CHECK(got.size() == o.n && std::memcmp(got.data(), want.data(), got.size()) == 0);
    used.bits = std::max(used.bits, pos);
    used.nodes = std::max<uint64_t>(used.nodes, nd.v.size());
}

// every leaf at Kmax - 1: the constant form's pieces give the same words
static void constant_is_the_plain_form(uint32_t gw, uint32_t gh, uint32_t kmax, const std::vector<uint32_t>& lens)
{
    const uint32_t n = gw * gh, height = (uint32_t)tag_tree_height(gw, gh);
    const Nodes nd(std::vector<uint32_t>(n, kmax - 1), gw, gh);
    std::vector<uint32_t> a((size_t)n * 8 + 8, 0u), b(a.size(), 0u);
    uint32_t pa = 0, pb = 0;
    for (uint32_t k = 0; k < n; ++k) {
        const uint32_t x = k % gw, y = k / gw;
        const T2BlockBits bb = t2_block_bits(x, y, height, kmax, lens[k]);
        put_bits(a.data(), pa, (1ull << bb.nn) - 1ull, bb.nn);
        put_bits(a.data(), pa + bb.nn + bb.zeros, bb.tail[0], bb.tail_n[0]);
        if (bb.tail_n[1]) put_bits(a.data(), pa + bb.nn + bb.zeros + bb.tail_n[0], bb.tail[1], bb.tail_n[1]);
        pa += bb.nbits;
        const T2MsbsBits mb = t2_block_bits_msbs(x, y, height, kmax - 1, bb.nn < height ? nd.get(bb.nn, x, y) : 0u, lens[k]);
        put_bits(b.data(), pb, (1ull << mb.nn) - 1ull, mb.nn);
        for (uint32_t l = 0; l < mb.nn; ++l) put_bits(b.data(), pb + t2_msbs_one_at(mb, l, nd.get(l, x, y)), 1, 1);
        put_bits(b.data(), pb + mb.nbits - mb.tail_n, mb.tail, mb.tail_n);
        pb += mb.nbits;
        CHECK(mb.nbits == bb.nbits && mb.nn == bb.nn && mb.inc == bb.inc);
    }
    CHECK(pa == pb && a == b);
}

int main()
{
    std::vector<uint32_t> lens = {0, (1u << kT2MaxLenBits) - 1u};
    for (uint32_t k = 0; k < kT2MaxLenBits; ++k)
        for (int d = -1; d <= 1; ++d) { const uint64_t v = (1ull << k) + d; if (v < (1ull << kT2MaxLenBits)) lens.push_back((uint32_t)v); }
    std::sort(lens.begin(), lens.end());
    lens.erase(std::unique(lens.begin(), lens.end()), lens.end());
    const uint32_t grids[][2] = {{1, 1}, {1, 7}, {7, 1}, {2, 2}, {3, 5}, {41, 35}, {256, 1}};
    std::mt19937 rng(12345);
    bool any_over64 = false, any_late = false;
    for (const auto& gr : grids) {
        const uint32_t gw = gr[0], gh = gr[1], n = gw * gh, height = (uint32_t)tag_tree_height(gw, gh);
        std::vector<std::pair<std::string, std::vector<uint32_t>>> pats;
        for (uint32_t c : {0u, 11u, 63u}) pats.push_back({"constant " + std::to_string(c), std::vector<uint32_t>(n, c)});
        { std::vector<uint32_t> v(n); for (auto& e : v) e = rng() % 64u; pats.push_back({"random", v}); }
        { std::vector<uint32_t> v(n); for (uint32_t i = 0; i < n; ++i) v[i] = n > 1 ? (uint32_t)((uint64_t)i * 63u / (n - 1)) : 63u; pats.push_back({"rising", v});
          std::reverse(v.begin(), v.end()); pats.push_back({"falling", v}); }
        for (uint32_t at : {0u, n / 2, n - 1}) {
            std::vector<uint32_t> v(n, 63u); v[at] = 0; pats.push_back({"a 0 among 63s at " + std::to_string(at), v});
            std::vector<uint32_t> w(n, 0u); w[at] = 63; pats.push_back({"a 63 among 0s at " + std::to_string(at), w});
        }
        Used used;
        // every length on every block of a small grid; the lengths dealt over a large grid's blocks from a few starts
        const uint32_t shifts = n <= 35 ? (uint32_t)lens.size() : 3u;
        for (const auto& pt : pats)
            for (uint32_t s = 0; s < shifts; ++s) {
                std::snprintf(where, sizeof where, "grid %u x %u (height %u), %s, lengths from %u on", gw, gh, height, pt.first.c_str(), s);
                std::vector<uint32_t> ln(n);
                for (uint32_t i = 0; i < n; ++i) ln[i] = lens[(i * 7u + s * (n <= 35 ? 1u : 23u)) % lens.size()];
                one_table(gw, gh, pt.second, ln, used);
            }
        any_over64 = any_over64 || used.over64; any_late = any_late || used.late_min;
        for (uint32_t kmax : {1u, 2u, 12u, 38u, 64u}) {
            std::snprintf(where, sizeof where, "grid %u x %u, every leaf at Kmax - 1 = %u", gw, gh, kmax - 1);
            std::vector<uint32_t> ln(n);
            for (uint32_t i = 0; i < n; ++i) ln[i] = lens[(i * 5u + kmax) % lens.size()];
            constant_is_the_plain_form(gw, gh, kmax, ln);
        }
        // ---- the plan: a tile of gw x gh code-blocks of 4 x 4 samples, no DWT level -- one packet of one band ----
        std::snprintf(where, sizeof where, "the plans of grid %u x %u", gw, gh);
        grk_amd_tile_params p{};
        p.tile_w = 4 * gw; p.tile_h = 4 * gh; p.num_comps = 1; p.prec = 8; p.num_levels = 0; p.cblk_w_exp = 2; p.cblk_h_exp = 2;
        TileGeom g;
        CHECK(build_tile_geom(p, g) == GRK_AMD_OK);
        T2Plan plain, general, flagged;
        CHECK(t2_device_plan(g, 0, plain) == GRK_AMD_OK);
        CHECK(t2_device_plan(g, GRK_AMD_CS_BLOCK_MSBS, flagged) == GRK_AMD_ERR_UNSUPPORTED);
        CHECK(t2_device_plan_msbs(g, 0, general) == GRK_AMD_OK);
        CHECK(t2_device_plan_msbs(g, GRK_AMD_CS_BLOCK_MSBS, flagged) == GRK_AMD_OK);
        CHECK(general.packets.size() == 1 && general.packets[0].nbands == 1 && general.packets[0].gw[0] == gw && general.packets[0].gh[0] == gh);
        CHECK(general.packets[0].height[0] == height && general.packets[0].nblocks == n);
        CHECK((uint64_t)general.packets[0].u_words * 32 >= used.bits + 64 && general.u_words >= general.packets[0].u_words);
        CHECK(general.v_bytes >= used.nodes && general.packets[0].v_at == 0);
        CHECK(general.packets[0].u_words >= plain.packets[0].u_words + n * kT2MaxMsbs / 32);
        CHECK(plain.v_bytes == 0 && plain.packets[0].v_at == 0);
        CHECK(flagged.u_words == general.u_words && flagged.h_bytes == general.h_bytes && flagged.v_bytes == general.v_bytes);
        // (a stuffed byte carries at least seven bits)
        CHECK((uint64_t)general.h_bytes * 7 >= used.bits);
    }
    CHECK(any_over64 && any_late);
    // three components, two levels, small precincts: every packet's node bytes lie apart, inside the tile's
    {
        std::snprintf(where, sizeof where, "the plan of 3 components, 2 levels, 64 x 64 precincts");
        grk_amd_tile_params p{};
        p.tile_w = 128; p.tile_h = 128; p.num_comps = 3; p.prec = 8; p.num_levels = 2; p.cblk_w_exp = 4; p.cblk_h_exp = 4; p.mct = 1;
        for (uint32_t r = 0; r <= 2; ++r) p.precinct_exp[r] = 0x66;
        TileGeom g;
        CHECK(build_tile_geom(p, g) == GRK_AMD_OK);
        for (uint32_t order = 0; order < 5; ++order) {
            T2Plan pl;
            CHECK(t2_device_plan_msbs(g, order << GRK_AMD_CS_PROG_SHIFT, pl) == GRK_AMD_OK);
            uint64_t end = 0;
            for (const T2Packet& k : pl.packets) {
                uint64_t nodes = 0;
                for (uint32_t b = 0; b < k.nbands; ++b) nodes += t2_tree_nodes(k.gw[b], k.gh[b]);
                CHECK(k.v_at >= end && (k.v_at & 15u) == 0);
                end = k.v_at + nodes;
            }
            CHECK(end <= pl.v_bytes);
        }
    }
    std::printf("ok: %ld checks\n", checks);
    return 0;
}
