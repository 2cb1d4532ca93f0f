// tests/c/packed_kernels_sim.cpp -- the two packed-frame kernels (grok_amd/csrc/kernels_packed.hip) compiled as host C++ against
// tests/c/hip_sim and run thread after thread, for tests/test_packed_cpu.py: KU's planes and KK's frame against plain index arithmetic
// written from the formats' definitions (include/grok_amd.h), the destination pre-filled with a pattern and compared byte for byte --
// a wrong sample and a byte written that is no sample both show.  The frame and the planes are heap blocks of exactly their sizes, so
// with -fsanitize=address,undefined an access outside them, or a 16-byte / two-byte access off its alignment, ends the program.
// Prints "ok: N launches"; exit status 1 with the case on a mismatch.
#include "../../grok_amd/csrc/kernels_packed.hip"
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>
using namespace grk_amd;

static std::mt19937 rng(7);
static long launches = 0;

// where a sample lies: byte formats and Y216 -- the container's index inside the macropixel; v210 -- (dword, field) inside the block
static const uint32_t kAt[3][4] = {{0, 2, 1, 3}, {1, 3, 0, 2}, {0, 2, 3, 1}};                 // Y0, Y1, Cb, Cr of YUY2, UYVY, YVYU
static const uint32_t kY210[6][2] = {{0, 1}, {1, 0}, {1, 2}, {2, 1}, {3, 0}, {3, 2}};
static const uint32_t kU210[3][2] = {{0, 0}, {1, 1}, {2, 2}}, kV210[3][2] = {{0, 2}, {2, 0}, {3, 1}};

static uint32_t rd16(const uint8_t* p) { return p[0] | (uint32_t)p[1] << 8; }
static uint32_t rd32(const uint8_t* p) { return rd16(p) | rd16(p + 2) << 16; }
static void wr16(uint8_t* p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); }
static void wr32(uint8_t* p, uint32_t v) { wr16(p, v & 0xFFFFu); wr16(p + 2, v >> 16); }

// component c's sample x of a row that starts at `row`: read (unpack), or written into the row (pack)
static uint32_t sample_get(uint32_t f, uint32_t prec, const uint8_t* row, uint32_t c, uint32_t x)
{
    const uint32_t m = c ? x : x >> 1, slot = c ? c + 1 : x & 1u;                              // Y0, Y1, Cb, Cr -> 0..3
    if (f <= kPackedYVYU) return row[4 * m + kAt[f][slot]];
    if (f == kPackedY216) return rd16(row + 8 * m + 2 * kAt[0][slot]) >> (16 - prec);
    const uint32_t* const at = c == 0 ? kY210[x % 6] : c == 1 ? kU210[x % 3] : kV210[x % 3];
    const uint32_t b = c ? x / 3 : x / 6;
    return (rd32(row + 16 * b + 4 * at[0]) >> (10 * at[1])) & 0x3FFu;
}
static void sample_put(uint32_t f, uint32_t prec, uint8_t* row, uint32_t c, uint32_t x, uint32_t v)
{
    const uint32_t m = c ? x : x >> 1, slot = c ? c + 1 : x & 1u;
    if (f <= kPackedYVYU) { row[4 * m + kAt[f][slot]] = (uint8_t)v; return; }
    if (f == kPackedY216) { wr16(row + 8 * m + 2 * kAt[0][slot], (v << (16 - prec)) & 0xFFFFu); return; }
    const uint32_t* const at = c == 0 ? kY210[x % 6] : c == 1 ? kU210[x % 3] : kV210[x % 3];
    uint8_t* const p = row + 16 * (c ? x / 3 : x / 6) + 4 * at[0];
    wr32(p, rd32(p) | (v & 0x3FFu) << (10 * at[1]));                                          // (the block was zeroed first)
}

static void one(uint32_t f, uint32_t prec, uint32_t w, uint32_t h, uint32_t base, uint64_t extra, uint32_t tbase, bool pack)
{
    const uint32_t bps = prec <= 8 ? 1 : 2, cw = (w + 1) / 2;
    const uint64_t pitch = packed_default_pitch(f, w) + extra, fbytes = (uint64_t)(h - 1) * pitch + packed_row_bytes(f, w);
    const size_t ny = (size_t)w * h * bps, nc = (size_t)cw * h * bps, fsize = base + fbytes, tsize = tbase + ny + 2 * nc;
    uint8_t* const fblock = (uint8_t*)malloc(fsize);
    uint8_t* const tblock = (uint8_t*)malloc(tsize);
    if (!fblock || !tblock || (((uintptr_t)fblock | (uintptr_t)tblock) & 15u)) { printf("malloc: no 16-byte aligned block\n"); exit(2); }
    for (size_t i = 0; i < fsize; ++i) fblock[i] = (uint8_t)rng();
    for (size_t i = 0; i < tsize; ++i) tblock[i] = (uint8_t)rng();
    if (pack && bps == 2)                          // samples of the full precision range
        for (size_t i = tbase; i + 1 < tsize; i += 2) wr16(tblock + i, rd16(tblock + i) & ((1u << prec) - 1u));
    if (pack && bps == 1) for (size_t i = tbase; i < tsize; ++i) tblock[i] &= (uint8_t)((1u << prec) - 1u);
    const std::vector<uint8_t> f0(fblock, fblock + fsize), t0(tblock, tblock + tsize);
    uint8_t* const pl = tblock + tbase;
    const PackedArgs a{fblock + base, pitch, pl, pl + ny, pl + ny + nc, w, h, f, prec};
    if ((pack ? launch_packed_pack(a, nullptr) : launch_packed_unpack(a, nullptr)) != hipSuccess) { printf("a launch was refused\n"); exit(2); }
    std::vector<uint8_t> wf = f0, wt = t0;
    const size_t plane_at[3] = {tbase, tbase + ny, tbase + ny + nc};
    for (uint32_t y = 0; y < h; ++y) {
        uint8_t* const row = wf.data() + base + y * pitch;
        if (pack && f == kPackedV210) memset(row, 0, packed_row_bytes(f, w));               // every block that holds a sample, whole
        for (uint32_t c = 0; c < 3; ++c) {
            const uint32_t n = c ? cw : w;
            for (uint32_t x = 0; x < n; ++x) {
                uint8_t* const t = wt.data() + plane_at[c] + ((size_t)y * n + x) * bps;
                if (pack) sample_put(f, prec, row, c, x, bps == 1 ? t[0] : rd16(t));
                else if (bps == 1) t[0] = (uint8_t)sample_get(f, prec, row, c, x);
                else wr16(t, sample_get(f, prec, row, c, x));
            }
        }
    }
    if (memcmp(wf.data(), fblock, fsize) || memcmp(wt.data(), tblock, tsize)) {
        printf("MISMATCH %s: format %u prec %u w %u h %u base %u pitch %llu tbase %u\n", pack ? "pack" : "unpack", f, prec, w, h, base,
               (unsigned long long)pitch, tbase);
        exit(1);
    }
    free(fblock); free(tblock); ++launches;
}

int main()
{
    const uint32_t widths[] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 47, 48, 49, 97};
    const struct { uint32_t f, prec; uint64_t extra; } cases[] = {
        {kPackedYUY2, 8, 5}, {kPackedUYVY, 8, 5}, {kPackedYVYU, 8, 5}, {kPackedYUY2, 3, 4}, {kPackedY216, 10, 6}, {kPackedY216, 12, 8},
        {kPackedY216, 16, 6}, {kPackedY216, 9, 2}, {kPackedV210, 10, 16}};
    for (const auto& k : cases) for (uint32_t w : widths) for (uint32_t h : {1u, 17u})
        for (uint32_t base = 0; base < 16; base += packed_align(k.f)) for (uint64_t extra : {(uint64_t)0, k.extra}) for (uint32_t tbase : {0u, 1u}) {
            one(k.f, k.prec, w, h, base, extra, tbase, false);
            one(k.f, k.prec, w, h, base, extra, tbase, true);
        }
    printf("ok: %ld launches\n", launches);
    return 0;
}
