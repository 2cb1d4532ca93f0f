// tests/c/t2_parts_writer_units.cpp -- the WRITER of tiles divided into tile-parts (t2_writer.cpp: grk_amd_write_tile_parts,
// grk_amd_write_main_header_parts, the file writers under GRK_AMD_CS_TP) and the frame arithmetic the device writer shares with it
// (t2_parts.h) as a stand-alone program for AddressSanitizer and UBSan (tests/test_tile_parts_writer_cpu.py builds and runs it).
// Every output lies in a heap block of exactly its size, so a byte written outside it is reported; the size-only pass must give the
// written length.  KT1p's frame (kernels_t2parts.hip) is played here from t2_parts.h -- the one-segment form with its exclusive scan,
// the serial form with the split -- and held against the host writer's bytes.
#include "../../include/grok_amd.h"
#include "../../grok_amd/csrc/t2_parts.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

using namespace grk_amd;

namespace {

int g_checks = 0;
#define CHECK(c) do { ++g_checks; if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

grk_amd_tile_params params(uint32_t w, uint32_t h, uint32_t comps, uint32_t levels, const std::vector<std::pair<int, int>>& prc)
{
    grk_amd_tile_params p{};
    p.tile_w = w; p.tile_h = h; p.num_comps = (uint16_t)comps; p.prec = 8; p.num_levels = (uint8_t)levels;
    p.cblk_w_exp = 2; p.cblk_h_exp = 2;
    for (size_t r = 0; r < prc.size(); ++r) p.precinct_exp[r] = (uint8_t)(prc[r].first | (prc[r].second << 4));
    return p;
}

// the frame of a part as KT1p makes it, from the packets' lengths: -> the frame's bytes (SOT .. SOD)
std::vector<uint8_t> play_frame(const std::vector<uint64_t>& lens, uint32_t isot, uint32_t k, uint32_t nparts, bool plt, uint32_t* segments)
{
    std::vector<uint8_t> f(part_frame_bound(lens.size(), plt), 0xEE);
    uint64_t body = 0, eb = 0;
    for (uint64_t v : lens) { body += v; eb += plt_entry_bytes(v); }
    uint32_t pos = 12;
    *segments = 0;
    if (plt && !lens.empty()) {
        if (eb <= kPltSegEntryBytes) {
            uint64_t at = 0;                                           // the exclusive scan
            for (uint64_t v : lens) {
                const uint32_t n = plt_entry_bytes(v);
                for (uint32_t j = 0; j < n; ++j) f.at(12 + kPltSegHead + at + j) = plt_entry_byte(v, n, j);
                at += n;
            }
            f.at(12) = 0xFF; f.at(13) = 0x58; f.at(14) = (uint8_t)((3 + eb) >> 8); f.at(15) = (uint8_t)(3 + eb); f.at(16) = 0;
            pos = 12 + kPltSegHead + (uint32_t)eb;
            *segments = 1;
        } else {
            PltSplit sp;
            uint32_t seg = 0;
            for (uint64_t v : lens) {
                const uint32_t n = plt_entry_bytes(v), fill = sp.fill;
                if (sp.add(n)) {
                    if (sp.segments > 1) { f.at(seg + 2) = (uint8_t)((3 + fill) >> 8); f.at(seg + 3) = (uint8_t)(3 + fill); }
                    seg = pos;
                    f.at(pos++) = 0xFF; f.at(pos++) = 0x58; pos += 2; f.at(pos++) = (uint8_t)(sp.segments - 1);
                }
                for (uint32_t j = 0; j < n; ++j) f.at(pos++) = plt_entry_byte(v, n, j);
            }
            f.at(seg + 2) = (uint8_t)((3 + sp.fill) >> 8); f.at(seg + 3) = (uint8_t)(3 + sp.fill);
            *segments = sp.segments;
        }
    }
    const uint64_t len = (uint64_t)pos + 2 + body;
    const uint8_t sot[12] = {0xFF, 0x90, 0, 10, (uint8_t)(isot >> 8), (uint8_t)isot, (uint8_t)(len >> 24), (uint8_t)(len >> 16), (uint8_t)(len >> 8),
                             (uint8_t)len, (uint8_t)k, (uint8_t)nparts};
    for (int i = 0; i < 12; ++i) f.at(i) = sot[i];
    f.at(pos) = 0xFF; f.at(pos + 1) = 0x93;
    f.resize(pos + 2);
    return f;
}

// the packets' lengths of the tile, from the PLT of the undivided tile-part
std::vector<uint64_t> packet_lengths(const grk_amd_tile_params& p, uint32_t flags, const std::vector<grk_amd_coded_block>& tab)
{
    const uint8_t dummy = 0;
    const int64_t n = grk_amd_write_tile_part(&p, 0, flags | GRK_AMD_CS_PLT, tab.data(), &dummy, nullptr, 0);
    CHECK(n > 0);
    // (sizes only: no coded byte is read; the real bytes are written below)
    std::vector<uint8_t> coded(1 << 16, 0x5A);
    std::unique_ptr<uint8_t[]> out(new uint8_t[(size_t)n]);
    CHECK(grk_amd_write_tile_part(&p, 0, flags | GRK_AMD_CS_PLT, tab.data(), coded.data(), out.get(), (uint64_t)n) == n);
    std::vector<uint64_t> lens;
    size_t at = 12;
    uint64_t v = 0;
    while (out[at] == 0xFF && out[at + 1] == 0x58) {
        const size_t l = (size_t)out[at + 2] << 8 | out[at + 3];
        for (size_t i = at + 5; i < at + 2 + l; ++i) { v = v << 7 | (out[i] & 0x7F); if (!(out[i] & 0x80)) { lens.push_back(v); v = 0; } }
        at += 2 + l;
    }
    CHECK(out[at] == 0xFF && out[at + 1] == 0x93);
    return lens;
}

std::vector<grk_amd_coded_block> table(const grk_amd_tile_params& p, uint32_t lo, uint32_t hi, uint32_t seed)
{
    const int64_t n = grk_amd_tile_num_blocks(&p);
    CHECK(n > 0);
    std::vector<grk_amd_coded_block> t((size_t)n);
    std::mt19937 rng(seed);
    for (auto& r : t) { r.length = lo + rng() % (hi - lo + 1); r.offset = rng() % ((1u << 16) - r.length); r.missing_msbs = 0; }
    return t;
}

// a division through the writer, every output in a block of its exact size, against the played frames
void check_division(const grk_amd_tile_params& p, uint32_t isot, uint32_t flags, const std::vector<grk_amd_coded_block>& tab,
                    const std::vector<uint32_t>& starts, uint32_t want_segments_part0)
{
    const std::vector<uint8_t> coded(1 << 16, 0x5A);
    const std::vector<uint64_t> lens = packet_lengths(p, flags & ~(uint32_t)GRK_AMD_CS_PLT, tab);
    const uint32_t np = (uint32_t)starts.size();
    std::unique_ptr<uint32_t[]> pb(new uint32_t[np]), pb2(new uint32_t[np]);
    const int64_t n = grk_amd_write_tile_parts(&p, isot, flags, tab.data(), nullptr, starts.data(), np, nullptr, 0, pb.get());
    CHECK(n > 0);
    std::unique_ptr<uint8_t[]> out(new uint8_t[(size_t)n]);
    CHECK(grk_amd_write_tile_parts(&p, isot, flags, tab.data(), coded.data(), starts.data(), np, out.get(), (uint64_t)n, pb2.get()) == n);
    CHECK(std::memcmp(pb.get(), pb2.get(), np * 4) == 0);
    {   // one byte short
        std::unique_ptr<uint8_t[]> small(new uint8_t[(size_t)n - 1]);
        CHECK(grk_amd_write_tile_parts(&p, isot, flags, tab.data(), coded.data(), starts.data(), np, small.get(), (uint64_t)n - 1, nullptr) == GRK_AMD_ERR_OVERFLOW);
    }
    uint64_t at = 0;
    for (uint32_t k = 0; k < np; ++k) {
        const size_t first = starts[k], last = k + 1 < np ? starts[k + 1] : lens.size();
        const std::vector<uint64_t> mine(lens.begin() + first, lens.begin() + last);
        uint32_t segs = 0;
        const std::vector<uint8_t> f = play_frame(mine, isot, k, np, (flags & GRK_AMD_CS_PLT) != 0, &segs);
        CHECK(f.size() <= part_frame_bound(mine.size(), (flags & GRK_AMD_CS_PLT) != 0));
        CHECK(at + f.size() <= (uint64_t)n && std::memcmp(out.get() + at, f.data(), f.size()) == 0);
        if (k == 0 && want_segments_part0) CHECK(segs == want_segments_part0);
        uint64_t body = 0;
        for (uint64_t v : mine) body += v;
        CHECK(pb[k] == f.size() + body);
        at += pb[k];
    }
    CHECK(at == (uint64_t)n);
}

void arithmetic()
{
    // entry bytes: the base-128 digits of the length, most significant first, the continuation bit on all but the last
    for (uint32_t sh = 0; sh <= 32; ++sh)
        for (int d = -2; d <= 2; ++d) {
            const uint64_t v = (uint64_t)((int64_t)(1ull << sh) + d) & 0xFFFFFFFFull;
            uint32_t k = 1;
            while (k < 10 && (v >> (7 * k))) ++k;
            CHECK(plt_entry_bytes(v) == k && k <= 5);
            uint64_t back = 0;
            for (uint32_t j = 0; j < k; ++j) {
                const uint8_t b = plt_entry_byte(v, k, j);
                CHECK(((b & 0x80) != 0) == (j + 1 < k));
                back = back << 7 | (b & 0x7F);
            }
            CHECK(back == v);
        }
    // the split: a segment takes entries until the next would carry it past 65 532 bytes; the bound covers every frame
    std::mt19937 rng(7);
    for (int round = 0; round < 6; ++round) {
        PltSplit sp;
        uint64_t entries = 0, npk = 0, naive_fill = 0, naive_segs = 0;
        const uint32_t kmax = 1 + round % 5;
        while (entries < 300000) {
            const uint32_t k = round == 5 ? 5 : 1 + rng() % kmax;
            const bool open = sp.add(k);
            if (naive_segs == 0 || naive_fill + k > 65532) { ++naive_segs; naive_fill = 0; CHECK(open); } else CHECK(!open);
            naive_fill += k;
            CHECK(sp.fill == naive_fill && sp.fill <= kPltSegEntryBytes && sp.segments == naive_segs);
            entries += k; ++npk;
            CHECK(kPartFrameFixed + entries + (uint64_t)kPltSegHead * sp.segments <= part_frame_bound(npk, true));
        }
    }
    CHECK(part_frame_bound(0, true) == 14 && part_frame_bound(100, false) == 14);
}

} // namespace

int main()
{
    arithmetic();
    // 36 packets (the tile of tests/t2read_cases.py with precincts (3, 3), (4, 3)) under every order: cuts and flags
    const grk_amd_tile_params q = params(40, 64, 1, 1, {{3, 3}, {4, 3}});
    const std::vector<grk_amd_coded_block> tq = table(q, 1, 300, 1);
    for (uint32_t order = 0; order < 5; ++order)
        for (uint32_t extra : {GRK_AMD_CS_PLT, GRK_AMD_CS_PLT | GRK_AMD_CS_SOP | GRK_AMD_CS_EPH, GRK_AMD_CS_SOP, 0u}) {
            const uint32_t flags = extra | GRK_AMD_CS_PROG(order);
            check_division(q, 3, flags, tq, {0, 12, 24}, 0);
            check_division(q, 65534, flags, tq, {0, 18, 18}, 0);
            check_division(q, 0, flags, tq, {0, 0}, 0);
            check_division(q, 0, flags, tq, {0, 36}, 0);
            check_division(q, 0, flags, tq, {0}, 0);
        }
    {   // one packet per part up to the 255th
        const grk_amd_tile_params m = params(40, 64, 4, 1, {{2, 2}, {3, 3}});
        std::vector<uint32_t> s(255);
        for (uint32_t k = 0; k < 255; ++k) s[k] = k;
        check_division(m, 1, GRK_AMD_CS_PLT | GRK_AMD_CS_SOP, table(m, 1, 200, 2), s, 0);
    }
    {   // refusals of explicit starts
        uint32_t bad[4][3] = {{0, 20, 10}, {0, 37, 37}, {1, 5, 6}, {0, 36, 37}};
        for (auto& b : bad) CHECK(grk_amd_write_tile_parts(&q, 0, 0, tq.data(), nullptr, b, 3, nullptr, 0, nullptr) == GRK_AMD_ERR_INVALID);
        std::vector<uint32_t> many(256, 0);
        CHECK(grk_amd_write_tile_parts(&q, 0, 0, tq.data(), nullptr, many.data(), 256, nullptr, 0, nullptr) == GRK_AMD_ERR_INVALID);
        CHECK(grk_amd_write_tile_parts(&q, 0, GRK_AMD_CS_PROG(3) | GRK_AMD_CS_TP(GRK_AMD_TP_R), tq.data(), nullptr, nullptr, 0, nullptr, 0, nullptr) == GRK_AMD_ERR_UNSUPPORTED);
        CHECK(std::strlen(grk_amd_writer_last_error()) > 0);
    }
    {   // the division of the flags, and the main header whose TLM lists the parts, in blocks of their size
        uint32_t starts[8], npk = 0;
        const uint32_t flags = GRK_AMD_CS_PLT | GRK_AMD_CS_TLM | GRK_AMD_CS_PROG(1) | GRK_AMD_CS_TP(GRK_AMD_TP_R);
        const int64_t np = grk_amd_tile_part_starts(&q, nullptr, nullptr, flags, starts, 8, &npk);
        CHECK(np == 2 && npk == 36 && starts[0] == 0 && starts[1] == 12);
        CHECK(grk_amd_tile_part_starts(&q, nullptr, nullptr, flags, starts, 1, &npk) == GRK_AMD_ERR_OVERFLOW);
        check_division(q, 0, flags, tq, {starts[0], starts[1]}, 0);
        const grk_amd_image_layout im{0, 0, 40, 64, 0, 0, 40, 64};
        const uint32_t per[1] = {2}, pbytes[2] = {1000, 2000};
        const int64_t hn = grk_amd_write_main_header_parts(&im, &q, flags, per, pbytes, nullptr, 0);
        CHECK(hn > 0);
        std::unique_ptr<uint8_t[]> hdr(new uint8_t[(size_t)hn]);
        CHECK(grk_amd_write_main_header_parts(&im, &q, flags, per, pbytes, hdr.get(), (uint64_t)hn) == hn);
        // TLM is the header's last marker segment: Ltlm 4 + 5 x 2, Stlm 0x50, {tile 0, 1000}, {tile 0, 2000}
        const uint8_t want[16] = {0xFF, 0x55, 0, 14, 0, 0x50, 0, 0, 0, 0x03, 0xE8, 0, 0, 0, 0x07, 0xD0};
        CHECK(std::memcmp(hdr.get() + hn - 16, want, 16) == 0);
        std::unique_ptr<uint8_t[]> small(new uint8_t[(size_t)hn - 1]);
        CHECK(grk_amd_write_main_header_parts(&im, &q, flags, per, pbytes, small.get(), (uint64_t)hn - 1) == GRK_AMD_ERR_OVERFLOW);
        // the whole file, sized by a first call into a block too large, then in a block of its size
        const std::vector<uint8_t> coded(1 << 16, 0x5A);
        std::vector<uint8_t> big(1 << 20);
        const int64_t fn = grk_amd_write_codestream_layout(&im, &q, tq.data(), coded.data(), flags, big.data(), big.size());
        CHECK(fn > hn);
        std::unique_ptr<uint8_t[]> file(new uint8_t[(size_t)fn]);
        CHECK(grk_amd_write_codestream_layout(&im, &q, tq.data(), coded.data(), flags, file.get(), (uint64_t)fn) == fn);
        CHECK(std::memcmp(file.get(), big.data(), (size_t)fn) == 0);
        std::unique_ptr<uint8_t[]> shortf(new uint8_t[(size_t)fn - 1]);
        CHECK(grk_amd_write_codestream_layout(&im, &q, tq.data(), coded.data(), flags, shortf.get(), (uint64_t)fn - 1) == GRK_AMD_ERR_OVERFLOW);
    }
    {   // 65 536 packets of two-byte entries: part 0's entries pass 65 532 bytes (two marker segments, the serial form), part 1's do not
        const grk_amd_tile_params b = params(512, 512, 1, 0, {{1, 1}});
        const std::vector<grk_amd_coded_block> tb = table(b, 128, 140, 3);
        CHECK(tb.size() == 65536);
        check_division(b, 0, GRK_AMD_CS_PLT, tb, {0, 40000}, 2);
        check_division(b, 0, GRK_AMD_CS_PLT | GRK_AMD_CS_EPH, tb, {0, 32766, 65532}, 1);      // exactly 65 532 bytes: still one segment
        check_division(b, 0, GRK_AMD_CS_PLT, tb, {0, 32767}, 2);                              // two bytes more: the second opens
    }
    std::printf("ok: %d checks\n", g_checks);
    return 0;
}
