// tests/c/surface_kernels_sim.cpp -- the two surface kernels (grok_amd/csrc/kernels_surface.hip) compiled as host C++ against
// tests/c/hip_sim and run thread after thread, for tests/test_surface_kernels_sim_cpu.py: every unit of a launch against plain index
// arithmetic (cut: word >> shift; place: v << shift cut to the container, every other byte of the surface unchanged).  The surface and
// the unit planes are heap blocks of exactly their sizes, so with -fsanitize=address,undefined an access outside them, or a 16-byte /
// two-byte access off its alignment, ends the program.  Prints "ok: N launches"; exit status 1 with the case on a mismatch.
#include "../../grok_amd/csrc/kernels_surface.hip"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>
using namespace grk_amd;

static std::mt19937 rng(1);
static long launches = 0;
static uint32_t rd(const uint8_t* p, uint32_t bps) { return bps == 1 ? p[0] : p[0] | p[1] << 8; }
static void wr(uint8_t* p, uint32_t bps, uint32_t v) { p[0] = (uint8_t)v; if (bps == 2) p[1] = (uint8_t)(v >> 8); }

// two units of w x h at (0, 0) and (w + 3, 2); the surface starts `base` bytes into its block, the planes `tbase` into theirs
static void one(uint32_t w, uint32_t h, uint32_t bps, const std::vector<SurfaceKernelComp>& comps, uint64_t nbytes, uint32_t base, uint32_t tbase, bool place)
{
    const uint32_t origins[4] = {0, 0, w + 3, 2};
    const uint32_t nu = 2, nc = (uint32_t)comps.size();
    const size_t n = (size_t)nu * nc * h * w * bps, ssize = base + nbytes, tsize = tbase + n;
    uint8_t* const sblock = (uint8_t*)malloc(ssize);
    uint8_t* const tblock = (uint8_t*)malloc(tsize);
    if (!sblock || !tblock || (((uintptr_t)sblock | (uintptr_t)tblock) & 15u)) { printf("malloc: no 16-byte aligned block\n"); exit(2); }
    for (size_t i = 0; i < ssize; ++i) sblock[i] = (uint8_t)rng();
    for (size_t i = 0; i < tsize; ++i) tblock[i] = (uint8_t)rng();
    const std::vector<uint8_t> s0(sblock, sblock + ssize), t0(tblock, tblock + tsize);
    SurfaceArgs a{};
    a.surface = sblock + base; a.tiles = tblock + tbase; a.nunits = nu; a.w = w; a.h = h; a.ncomp = nc; a.bps = bps; a.origins = origins;
    for (uint32_t k = 0; k < nc; ++k) a.comp[k] = comps[k];
    if ((place ? launch_surface_place(a, nullptr) : launch_surface_cut(a, nullptr)) != hipSuccess) { printf("a launch was refused\n"); exit(2); }
    std::vector<uint8_t> ws = s0, wt = t0;
    for (uint32_t u = 0; u < nu; ++u) for (uint32_t k = 0; k < nc; ++k) for (uint32_t y = 0; y < h; ++y) for (uint32_t x = 0; x < w; ++x) {
        const size_t si = base + comps[k].offset + (size_t)(origins[2 * u + 1] + y) * comps[k].row_pitch + (size_t)(origins[2 * u] + x) * comps[k].step * bps;
        const size_t ti = tbase + ((((size_t)u * nc + k) * h + y) * w + x) * bps;
        if (place) wr(&ws[si], bps, (rd(&t0[ti], bps) << comps[k].shift) & (bps == 1 ? 0xFFu : 0xFFFFu));
        else wr(&wt[ti], bps, rd(&s0[si], bps) >> comps[k].shift);
    }
    if (memcmp(ws.data(), sblock, ssize) || memcmp(wt.data(), tblock, tsize)) {
        printf("MISMATCH %s: w %u h %u bps %u comps %u step %u offset %llu pitch %llu shifts %u %u base %u tbase %u\n", place ? "place" : "cut", w, h, bps, nc,
               comps[0].step, (unsigned long long)comps[0].offset, (unsigned long long)comps[0].row_pitch, comps[0].shift, nc > 1 ? comps[1].shift : 0, base, tbase);
        exit(1);
    }
    free(sblock); free(tblock); ++launches;
}

// `ncomp` components: partners a sample apart, or planes of their own; cut and placed
static void both(uint32_t w, uint32_t h, uint32_t bps, uint32_t step, uint32_t first, bool partner, uint32_t extra, const std::vector<uint32_t>& shifts, bool reverse,
                 uint32_t base, uint32_t tbase)
{
    const uint32_t ncomp = (uint32_t)shifts.size();
    const uint64_t cols = 2 * (uint64_t)w + 3, rows = 2 + h;
    const uint64_t row = ((cols - 1) * step + 1) * bps, pitch = row + (partner ? (ncomp - 1) * bps : 0) + 5 * bps + extra;
    std::vector<SurfaceKernelComp> comps;
    uint64_t at = first, last = 0;
    for (uint32_t k = 0; k < ncomp; ++k) { comps.push_back(SurfaceKernelComp{at, pitch, step, shifts[k]}); last = at; at += partner ? bps : rows * pitch + 3 * bps; }
    const uint64_t nbytes = last + (rows - 1) * pitch + row;
    if (reverse) std::reverse(comps.begin(), comps.end());
    one(w, h, bps, comps, nbytes, base, tbase, false);
    one(w, h, bps, comps, nbytes, base, tbase, true);
}

int main()
{
    const uint32_t widths[] = {1, 3, 4, 5, 7, 8, 9, 17, 65, 130};
    for (uint32_t w : widths) for (uint32_t h : {1u, 5u}) for (uint32_t sh : {0u, 6u, 15u}) {
        // two-byte samples: first samples at every alignment of a 16-byte line, the surface and the planes on even and odd addresses
        for (uint32_t first = 0; first < 16; first += 2) for (uint32_t base : {0u, 1u}) for (uint32_t tbase : {0u, 1u}) {
            for (uint32_t step = 1; step <= 4; ++step) both(w, h, 2, step, first, false, 0, {sh}, false, base, tbase);
            for (bool rev : {false, true}) {
                both(w, h, 2, 2, first, true, 0, {sh, sh}, rev, base, tbase);
                both(w, h, 2, 2, first, true, 0, {sh, 6 - sh % 7}, rev, base, tbase);
            }
            both(w, h, 2, 1, first, false, 0, {sh, 0, 3}, false, base, tbase);
        }
        // one-byte samples: every first byte, even and odd pitches
        if (sh < 8) for (uint32_t first : {0u, 1u, 5u, 14u, 15u}) for (uint32_t extra : {0u, 1u}) for (uint32_t tbase : {0u, 1u}) {
            for (uint32_t step = 1; step <= 4; ++step) both(w, h, 1, step, first, false, extra, {sh}, false, 0, tbase);
            for (bool rev : {false, true}) {
                both(w, h, 1, 2, first, true, extra, {sh, sh}, rev, 0, tbase);
                both(w, h, 1, 2, first, true, extra, {0, sh}, rev, 0, tbase);
            }
        }
    }
    printf("ok: %ld launches\n", launches);
    return 0;
}
