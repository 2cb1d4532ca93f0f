// grok_amd/csrc/packed_format.h -- the packed 4:2:2 formats (include/grok_amd.h: GRK_AMD_PACKED_*): three components Y, Cb, Cr with
// factors (1, 1), (2, 1), (2, 1) in one pitched frame whose components differ in step.  Macropixel m of a row holds Y[2m], Y[2m + 1],
// Cb[m], Cr[m]:
//   YUY2 / UYVY / YVYU   4 bytes per macropixel: Y0 Cb Y1 Cr / Cb Y0 Cr Y1 / Y0 Cr Y1 Cb; 1..8 bits
//   Y216                 4 little-endian 16-bit words Y0 Cb Y1 Cr, each v << (16 - prec); 9..16 bits (10: Y210, 12: Y212)
//   v210                 a 16-byte block of four little-endian dwords, three 10-bit fields each (bits 0-9, 10-19, 20-29; 30-31 zero),
//                        holds three macropixels:  w0 = Cb0 Y0 Cr0   w1 = Y1 Cb1 Y2   w2 = Cr1 Y3 Cb2   w3 = Y4 Cr2 Y5;  exactly 10 bits
// HIP-free: the kernels (kernels_packed.hip), the host side (packed.cpp) and the CPU tests read the formats from here.
#pragma once
#include <cstdint>

namespace grk_amd {

constexpr uint32_t kPackedYUY2 = 0, kPackedUYVY = 1, kPackedYVYU = 2, kPackedY216 = 3, kPackedV210 = 4, kPackedFormats = 5;

// the byte of a one-byte macropixel that holds Y0 (Y1 lies two behind), Cb, Cr
constexpr uint32_t packed_y_at(uint32_t f) { return f == kPackedUYVY ? 1u : 0u; }
constexpr uint32_t packed_cb_at(uint32_t f) { return f == kPackedYUY2 ? 1u : f == kPackedUYVY ? 0u : 3u; }
constexpr uint32_t packed_cr_at(uint32_t f) { return f == kPackedYUY2 ? 3u : f == kPackedUYVY ? 2u : 1u; }

constexpr bool packed_prec_ok(uint32_t f, uint32_t prec)
{
    return f <= kPackedYVYU ? prec >= 1 && prec <= 8 : f == kPackedY216 ? prec >= 9 && prec <= 16 : f == kPackedV210 && prec == 10;
}
// what the base address and the pitch are multiples of
constexpr uint32_t packed_align(uint32_t f) { return f == kPackedV210 ? 16u : f == kPackedY216 ? 2u : 1u; }
// bytes from a row's first byte to the end of its last container, for w luma samples
constexpr uint64_t packed_row_bytes(uint32_t f, uint64_t w)
{
    return f == kPackedV210 ? (w + 5) / 6 * 16 : (w + 1) / 2 * (f == kPackedY216 ? 8u : 4u);
}
// the pitch that 0 stands for: a tight row; v210 rows by convention in units of 48 samples = 128 bytes
constexpr uint64_t packed_default_pitch(uint32_t f, uint64_t w) { return f == kPackedV210 ? (w + 47) / 48 * 128 : packed_row_bytes(f, w); }

} // namespace grk_amd
