// grok_amd/csrc/t2_bits.h -- a code-block's share of a packet header as the device writer composes it (KT1, kernels_t2.hip): the
// arithmetic alone, for the kernel and for a host program (tests/c/t2_bits_units.cpp) alike.  No HIP in here.
//
// In the single layer of this encoder every block is included and both tag trees of a band's precinct are uniform (t2_writer.cpp,
// "tag trees as this writer meets them"), so block (x, y) of a grid whose trees have `height` levels contributes
//     nn ones | (the band's first block: Kmax - 1 zeros) | nn ones | the pass bit 0 | Lblock: inc ones, a zero | the length, 3 + inc bits
// with nn = min(ctz(x | y) + 1, height) (all of the path for the first block) and inc = what Lblock has to grow from 3 for the length.
#pragma once
#include <cstdint>

#if defined(__HIP_DEVICE_COMPILE__) || defined(__HIPCC__)
#define GRK_T2_FN __host__ __device__ inline
#else
#define GRK_T2_FN inline
#endif

namespace grk_amd {

// Block lengths the device writer takes: below 2^20.  An HT block of 64x64 16-bit coefficients is a few KB, a Part-1 block stays
// under 64 KB: nothing comes near 1 MB, and the plan's scratch bound (t2_device_plan_joint) is sized by this number.
constexpr uint32_t kT2MaxLenBits = 20;
// Tag-tree heights the plan admits (a grid of up to 2^31 x 2^31 blocks): nn ones and the pass bit are one piece of at most 33 bits.
constexpr uint32_t kT2MaxHeight = 32;

GRK_T2_FN bool t2_len_ok(uint32_t len) { return (len >> kT2MaxLenBits) == 0; }

struct T2BlockBits {
    uint32_t nn, zeros, inc;
    uint32_t nbits;                   // all of the block's bits: nn + zeros + the tail's
    // what follows the first nn ones and the zeros, MSB first, in pieces of at most 64 bits: one piece where it fits (every length
    // below the limit under a tree of up to 25 levels), else the ones with the pass bit | Lblock with the length
    uint64_t tail[2]; uint32_t tail_n[2];
};

// height <= kT2MaxHeight, t2_len_ok(len); the band's first block (x = y = 0) carries the zero-bit-plane tree's root: Kmax - 1 zeros
GRK_T2_FN T2BlockBits t2_block_bits(uint32_t x, uint32_t y, uint32_t height, uint32_t kmax, uint32_t len)
{
    T2BlockBits r;
    const uint32_t m = x | y;
    const uint32_t z = m ? (uint32_t)__builtin_ctz(m) + 1u : height;
    r.nn = z < height ? z : height;
    const uint32_t fl = len ? 31u - (uint32_t)__builtin_clz(len) : 0u;
    r.inc = fl + 1u > 3u ? fl + 1u - 3u : 0u;
    r.zeros = m ? 0u : kmax - 1u;
    const uint32_t n0 = r.nn + 1u, n1 = (r.inc + 1u) + (3u + r.inc);
    const uint64_t ones = ((1ull << r.nn) - 1ull) << 1;                               // nn ones, the pass bit 0
    const uint64_t lblock = ((((1ull << r.inc) - 1ull) << 1) << (3u + r.inc)) | len;  // inc ones, a zero, the length
    if (n0 + n1 <= 64u) { r.tail[0] = (ones << n1) | lblock; r.tail_n[0] = n0 + n1; r.tail[1] = 0; r.tail_n[1] = 0; }
    else { r.tail[0] = ones; r.tail_n[0] = n0; r.tail[1] = lblock; r.tail_n[1] = n1; }
    r.nbits = r.nn + r.zeros + n0 + n1;
    return r;
}

// ---- the general zero-bit-plane tree: every block with its own missing_msbs (GRK_AMD_CS_BLOCK_MSBS) ---------------------------------
// Every block of the packet is still included, in raster order, so the inclusion tree stays uniform and the first leaf to pass a node
// is its top-left one: the NEW nodes of block (x, y) are levels nn - 1 .. 0 in both trees.  With v_l the minimum of missing_msbs over
// the leaves below the block's node at level l, ZbpTree::code (t2_writer.cpp) emits for every new node, from the top one down,
// v_l - v_(l+1) zeros and a one -- the parent of the root counts as 0 -- : the block's share is
//     nn ones | for l = nn - 1 .. 0: (v_l - v_(l+1)) zeros, a one | the pass bit 0 | Lblock: inc ones, a zero | the length, 3 + inc bits
// With every leaf at Kmax - 1 that is t2_block_bits' string bit for bit.
//
// The values the device writer takes: above any Kmax - 1 this library's geometry produces.
constexpr uint32_t kT2MaxMsbs = 63;

// the levels of a gw x gh grid's tree, one byte per node, level 0 (the leaves, raster) first: what all of them hold
GRK_T2_FN uint64_t t2_tree_nodes(uint32_t gw, uint32_t gh)
{
    uint64_t n = 0;
    for (;;) {
        n += (uint64_t)gw * gh;
        if ((uint64_t)gw * gh <= 1) break;
        gw = (gw + 1) >> 1; gh = (gh + 1) >> 1;
    }
    return n;
}

struct T2MsbsBits {
    uint32_t nn, inc;
    uint32_t vtop;                    // v_nn: the value the top new node starts from (0 above the root)
    uint32_t nbits;                   // all of the block's bits
    uint64_t tail; uint32_t tail_n;   // the pass bit 0 | Lblock with the length: the string's last tail_n (<= 39) bits
};

// height <= kT2MaxHeight, t2_len_ok(len), v0 <= kT2MaxMsbs the block's own value, vparent that of its node at level nn (not read when
// that node does not exist: nn == height)
GRK_T2_FN T2MsbsBits t2_block_bits_msbs(uint32_t x, uint32_t y, uint32_t height, uint32_t v0, uint32_t vparent, uint32_t len)
{
    T2MsbsBits r;
    const uint32_t m = x | y;
    const uint32_t z = m ? (uint32_t)__builtin_ctz(m) + 1u : height;
    r.nn = z < height ? z : height;
    r.vtop = r.nn < height ? vparent : 0u;
    const uint32_t fl = len ? 31u - (uint32_t)__builtin_clz(len) : 0u;
    r.inc = fl + 1u > 3u ? fl + 1u - 3u : 0u;
    r.tail = ((((1ull << r.inc) - 1ull) << 1) << (3u + r.inc)) | len;                 // (the pass bit: a zero in front)
    r.tail_n = 1u + (r.inc + 1u) + (3u + r.inc);
    r.nbits = 2u * r.nn + (v0 - r.vtop) + r.tail_n;
    return r;
}
// where, from the string's first bit, the one of the new node at level l (< nn) stands, v_l its value: behind the nn inclusion ones,
// the zeros of the levels down to l and the ones of the levels above it.  (The tail stands at nbits - tail_n.)
GRK_T2_FN uint32_t t2_msbs_one_at(const T2MsbsBits& r, uint32_t l, uint32_t vl) { return r.nn + (vl - r.vtop) + (r.nn - 1u - l); }

} // namespace grk_amd
