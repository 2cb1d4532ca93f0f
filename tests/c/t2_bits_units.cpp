// tests/c/t2_bits_units.cpp -- a code-block's share of a packet header as the device writer composes it (grok_amd/csrc/t2_bits.h, what
// KT1 of kernels_t2.hip includes) against the host writer's own bit writer (HeaderBits of t2_writer.cpp, included here as it is): a
// stand-alone program for tests/test_t2_bits_cpu.py, built with g++ under -fsanitize=address,undefined -- no GPU, no HIP.
//
// The sweep: every tag-tree height the plan admits (1 .. kT2MaxHeight); the band's first block and, for every ctz(x | y) of 0 .. 31,
// the blocks (2^z, 0), (0, 2^z) and (2^z, 3 * 2^z); Kmax of 1, 2, 12 and 38; the lengths 0, 1, 7, 8, the limit - 1 and, for every k below
// the limit's bit count, 2^k - 1, 2^k, 2^k + 1.  Per case the header's string -- t2_block_bits' nn ones, zeros, and the tail's pieces --
// goes through put_bits as the kernel has it (plain ORs instead of atomic ones) into zeroed words, behind 0 .. 8 ones that vary the
// string's phase; the words, stuffed by a plain sequential writer, must be HeaderBits' bytes for the same block, and nbits its bit
// count.  Prints "ok: N checks"; exit status 1 with the case on a failure.
//
// `t2_bits_units parent`: the same sweep over the arithmetic this header replaced -- the tail composed in ONE 64-bit value and
// written by one put_bits call, lengths below 2^29 -- in the same order (height, block, Kmax, length ascending).  Its tail is
// nn + 5 + 2 * inc bits: UBSan reports the shift at the first case that needs more than 64, and the bytes' check names the case.
#include "../../grok_amd/csrc/t2_writer.cpp"
#include <cstdio>
#include <cstdlib>
#include <string>

static long checks = 0;
static char where[200];
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

// raw bits -> bytes, one bit at a time: a byte behind an 0xFF takes seven bits; the last byte padded with zeros, an empty byte behind a
// final 0xFF (ISO 15444-1 B.10.1)
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

// the parent's arithmetic: kernels_t2.hip before t2_bits.h
static uint32_t parent_block(uint32_t* u, uint32_t pos, uint32_t x, uint32_t y, uint32_t height, uint32_t kmax, uint32_t len)
{
    const uint32_t m = x | y;
    const uint32_t nn = m ? std::min((uint32_t)__builtin_ctz(m) + 1u, height) : height;
    const int fl = len ? 31 - __builtin_clz(len) : 0;
    const uint32_t inc = fl + 1 > 3 ? (uint32_t)(fl + 1 - 3) : 0u;
    const uint32_t zeros = m ? 0u : kmax - 1u;
    const uint32_t nbits = 2 * nn + zeros + 1 + (inc + 1) + (3 + inc);
    put_bits(u, pos, (1ull << nn) - 1ull, nn);
    pos += nn + zeros;
    const uint64_t tail = ((((((1ull << nn) - 1ull) << 1) << (inc + 1)) | (((1ull << inc) - 1ull) << 1)) << (3 + inc)) | len;
    put_bits(u, pos, tail, nn + 1 + inc + 1 + 3 + inc);
    return nbits;
}

int main(int argc, char** argv)
{
    const bool parent = argc > 1 && std::string(argv[1]) == "parent";
    const uint32_t len_bits = parent ? 29u : kT2MaxLenBits;
    std::vector<uint32_t> lens = {0, 1, 7, 8, (1u << len_bits) - 1u};
    for (uint32_t k = 0; k < len_bits; ++k)
        for (int d = -1; d <= 1; ++d) { const uint64_t v = (1ull << k) + d; if (v < (1ull << len_bits)) lens.push_back((uint32_t)v); }
    std::sort(lens.begin(), lens.end());
    lens.erase(std::unique(lens.begin(), lens.end()), lens.end());
    std::vector<std::pair<uint32_t, uint32_t>> blocks = {{0, 0}};
    for (uint32_t z = 0; z < 32; ++z) {
        blocks.push_back({1u << z, 0});
        blocks.push_back({0, 1u << z});
        blocks.push_back({1u << z, z < 30 ? 3u << z : 1u << z});
    }
    const uint32_t kmaxes[] = {1, 2, 12, 38};
    uint32_t phase = 0, longest = 0;
    bool two_pieces = false;
    std::vector<uint8_t> want(64);
    for (uint32_t height = 1; height <= kT2MaxHeight; ++height)
        for (const auto& xy : blocks)
            for (uint32_t kmax : kmaxes) {
                if ((xy.first | xy.second) && kmax != kmaxes[0]) continue;     // (Kmax reaches the band's first block alone)
                for (uint32_t len : lens) {
                    const uint32_t x = xy.first, y = xy.second;
                    std::snprintf(where, sizeof where, "tag-tree height %u, block (%u, %u), Kmax %u, length %u", height, x, y, kmax, len);
                    phase = (phase + 1) % 9;
                    // the host writer, as write_packet codes a block
                    Out o{want.data(), want.size()};
                    HeaderBits hb(o);
                    hb.ones((int)phase);
                    const int nn = new_nodes(x, y, (int)height);
                    hb.ones(nn);
                    if (!(x | y)) hb.zeros((int)kmax - 1);
                    hb.ones(nn);
                    int inc = floor_log2(len) + 1 - 3;
                    if (inc < 0) inc = 0;
                    hb.put(0, 1);
                    hb.comma(inc);
                    hb.put(len, 3 + inc);
                    const uint32_t want_bits = phase + 2 * (uint32_t)nn + ((x | y) ? 0u : kmax - 1u) + 1 + ((uint32_t)inc + 1) + (3 + (uint32_t)inc);
                    hb.flush();
                    CHECK(!o.ovf);
                    // the device writer's arithmetic
                    uint32_t u[8] = {0, 0, 0, 0, 0, 0, 0, 0};
                    put_bits(u, 0, (1ull << phase) - 1ull, phase);
                    uint32_t nbits;
                    if (parent) nbits = parent_block(u, phase, x, y, height, kmax, len);
                    else {
                        CHECK(t2_len_ok(len));
                        const T2BlockBits bb = t2_block_bits(x, y, height, kmax, len);
                        CHECK(bb.nn == (uint32_t)nn && bb.inc == (uint32_t)inc && bb.zeros == ((x | y) ? 0u : kmax - 1u));
                        CHECK(bb.tail_n[0] >= 1 && bb.tail_n[0] <= 64 && bb.tail_n[1] <= 64);
                        CHECK(bb.nbits == bb.nn + bb.zeros + bb.tail_n[0] + bb.tail_n[1]);
                        CHECK(bb.nbits + 8 + 64 <= 8 * 32);                     // (this program's words; put_bits touches three)
                        uint32_t pos = phase;
                        put_bits(u, pos, (1ull << bb.nn) - 1ull, bb.nn);
                        pos += bb.nn + bb.zeros;
                        put_bits(u, pos, bb.tail[0], bb.tail_n[0]);
                        if (bb.tail_n[1]) put_bits(u, pos + bb.tail_n[0], bb.tail[1], bb.tail_n[1]);
                        two_pieces = two_pieces || bb.tail_n[1] != 0;
                        longest = std::max(longest, bb.tail_n[0] + bb.tail_n[1]);
                        nbits = bb.nbits;
                    }
                    CHECK(phase + nbits == want_bits);
                    const std::vector<uint8_t> got = stuff(u, phase + nbits);
                    CHECK(got.size() == o.n && std::memcmp(got.data(), want.data(), got.size()) == 0);
                }
            }
    if (!parent) {
        // the limit in force keeps the tail in one piece under every tree a test can afford; the split is taken above that
        CHECK(longest == kT2MaxHeight + 5 + 2 * (kT2MaxLenBits - 3));
        CHECK(two_pieces == (longest > 64));
        CHECK(!t2_len_ok(1u << kT2MaxLenBits) && !t2_len_ok(0xFFFFFFFFu) && t2_len_ok((1u << kT2MaxLenBits) - 1u));
    }
    std::printf("ok: %ld checks\n", checks);
    return 0;
}
