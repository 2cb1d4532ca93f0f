// grok_amd/csrc/t2_parts.h -- the arithmetic of a tile-part's frame (SOT, the PLT marker segments of the part's own packets, SOD) as
// the host writer (t2_writer.cpp), the device writer (KT1p, kernels_t2parts.hip) and its scratch bounds (assemble.hip) share it, for
// the kernels and for a host program (tests/c/t2_parts_writer_units.cpp) alike.  No HIP in here.
//
// A PLT marker segment is FF58, Lplt (16 bits: Lplt, Zplt and at most 65 532 bytes of entries), Zplt; an entry is the packet's length
// as a big-endian base-128 number, 1 to 5 bytes for the lengths a 32-bit Psot admits, and is never split over two segments (T.800
// A.7.3; write_plt, t2_writer.cpp).
#pragma once
#include "t2_bits.h"        // GRK_T2_FN

namespace grk_amd {

constexpr uint32_t kPltSegEntryBytes = 65532;     // entry bytes one marker segment holds
constexpr uint32_t kPltSegHead = 5;               // FF58, Lplt, Zplt
constexpr uint32_t kPartFrameFixed = 14;          // SOT marker segment 12, SOD 2: a tile-part without packets and without PLT
constexpr uint32_t kMaxTileParts = 255;           // TPsot / TNsot are one byte
constexpr uint32_t kMaxTlmEntries = 13106;        // one TLM marker segment: Ltlm 16 bits, 4 + 5 per entry

// the bytes of a packet length's PLT entry
GRK_T2_FN uint32_t plt_entry_bytes(uint64_t v)
{
    uint32_t k = 1;
    for (v >>= 7; v; v >>= 7) ++k;
    return k;
}

// byte j (0: first) of the k-byte entry of v
GRK_T2_FN uint8_t plt_entry_byte(uint64_t v, uint32_t k, uint32_t j)
{
    const uint32_t sh = 7u * (k - 1u - j);
    return (uint8_t)(((v >> sh) & 0x7Fu) | (j + 1u < k ? 0x80u : 0u));
}

// The serial split: entries go into the open segment until the next one would carry it past kPltSegEntryBytes.
struct PltSplit {
    uint32_t fill = 0, segments = 0;          // entry bytes in the open segment; segments opened so far
    // -> true: a new segment has to be opened in front of this entry (the first entry opens segment 0)
    GRK_T2_FN bool add(uint32_t k)
    {
        const bool open = segments == 0 || fill + k > kPltSegEntryBytes;
        if (open) { ++segments; fill = 0; }
        fill += k;
        return open;
    }
};

// What a part's frame can take at most: every entry 5 bytes, plus a segment head per kPltSegEntryBytes of them begun (a segment is
// never left with fewer than kPltSegEntryBytes - 4 bytes before another opens).  npk: the part's packets
GRK_T2_FN uint64_t part_frame_bound(uint64_t npk, bool plt)
{
    if (!plt || !npk) return kPartFrameFixed;
    const uint64_t entries = 5 * npk;
    return kPartFrameFixed + entries + kPltSegHead * (entries / (kPltSegEntryBytes - 4) + 1);
}

} // namespace grk_amd
