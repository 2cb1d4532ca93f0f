// grok_amd/csrc/dwt_instances.h -- the instances of the DWT and egress kernel templates, one list per template, and what both
// transform directions share on the host: the split of a fused level into parts and the row segments of a level.  No HIP in
// here: the planners (encode_plan.cpp, decode_plan.cpp) name an instance by a key -- the template arguments as a small POD --,
// the launchers (kernels_dwt.hip, kernels_idwt.hip) look the key up in the template's list and instantiate exactly the rows of
// that list, and the CPU drivers under tests/c see the same rows.  A key that is in no list is hipErrorInvalidValue at the
// launcher; a row written twice does not compile (two equal case labels).
#pragma once
#include <cstdint>

namespace grk_amd {

// ---- the parts of a level fused with the pixels ------------------------------------------------------------------------------------
// The level that reads or writes the caller's pixels runs the MCT triple side by side in one workgroup (nc = 3) and every component
// beyond it on its own, or -- without a colour transform -- every component on its own, as z slots of one launch.
struct LevelPart { uint32_t comp0, zdiv, nc; };      // first component of a z slot, z slots per tile, components per workgroup
inline bool     level_has_triple(bool mct, uint32_t ncomp) { return mct && ncomp >= 3; }
inline uint32_t level_part_count(bool mct, uint32_t ncomp) { return level_has_triple(mct, ncomp) ? ncomp - 2 : 1; }
inline LevelPart level_part(bool mct, uint32_t ncomp, uint32_t i)
{
    if (!level_has_triple(mct, ncomp)) return LevelPart{0, ncomp, 1};
    return i == 0 ? LevelPart{0, 1, 3} : LevelPart{i + 2, 1, 1};
}
// workgroups along z per tile of the widest part (what the row segments are sized for)
inline uint32_t level_part_zslots(bool mct, uint32_t ncomp) { return level_has_triple(mct, ncomp) ? 1u : ncomp; }

// row pairs per workgroup of a DWT level: halved from 64 (to 8 at the least) while strips x row segments x z slots stay below min_wgs
inline uint32_t row_segment_pairs(uint64_t strips, uint32_t row_pairs, uint32_t zslots, uint32_t min_wgs)
{
    uint32_t seg = 64;
    while (seg > 8 && strips * ((row_pairs + seg - 1) / seg) * zslots < min_wgs) seg >>= 1;
    return seg;
}

// ---- keys: the template arguments of one instance ----------------------------------------------------------------------------------
struct DwtKey {          // dwt_level_kernel<F97, NC, PX, H16, GEN, STR>
    bool f97; uint8_t nc, px; bool h16, gen, str;
    constexpr uint32_t code() const { return (uint32_t)f97 | nc << 1 | px << 4 | (uint32_t)h16 << 6 | (uint32_t)gen << 7 | (uint32_t)str << 8; }
};
struct DwtPkKey {        // dwt53_pk_kernel<NC, PX, NT, CH>
    uint8_t nc, px; uint16_t nt; uint8_t ch;
    constexpr uint32_t code() const { return nc | px << 3 | ch << 5 | (uint32_t)nt << 8; }
};
struct DwtPairKey {      // pair::dwt53_pk_kernel<NC, PX, NT>
    uint8_t nc, px; uint16_t nt;
    constexpr uint32_t code() const { return nc | px << 3 | (uint32_t)nt << 8; }
};
struct IdwtKey {         // idwt_level_kernel<F97, NC, PXO, H16, STR>
    bool f97; uint8_t nc, pxo; bool h16, str;
    constexpr uint32_t code() const { return (uint32_t)f97 | nc << 1 | pxo << 4 | (uint32_t)h16 << 6 | (uint32_t)str << 7; }
};
struct IdwtPkKey {       // idwt53_pk_kernel<NC, PXO, CH>
    uint8_t nc, pxo, ch;
    constexpr uint32_t code() const { return nc | pxo << 3 | ch << 5; }
};
struct EgressKey {       // egress_kernel<PIX, NC, STR>, PIX = the unsigned integer of `bytes` bytes (4: int32_t)
    uint8_t bytes, nc; bool str;
    constexpr uint32_t code() const { return bytes | nc << 3 | (uint32_t)str << 6; }
};
// the instance a launch takes: a row of the packed kernel's list or of the 32-bit kernel's
struct DwtInstance  { bool packed; DwtKey k; DwtPkKey pk; };
struct IdwtInstance { bool packed; IdwtKey k; IdwtPkKey pk; uint32_t grid_x; };     // (the packed kernel's strips are wider)

// ---- the lists -----------------------------------------------------------------------------------------------------------------------
// K2, 32-bit: every level but the fused one (NC 1, PX 0); level 0 from the pixels: default layout (GEN = false: the all-fast form,
// for int32 / float planes only), a layout of the caller's (STR, always GEN); H16 for 8-bit pixels only
#define GRK_DWT_INSTANCES(X) /* F97, NC, PX, H16, GEN, STR */                                                                     \
    X(true, 1, 0, false, true, false) X(false, 1, 0, true, true, false) X(false, 1, 0, false, true, false)                       \
    X(true, 3, 1, false, true, true) X(true, 3, 2, false, true, true) X(true, 1, 1, false, true, true) X(true, 1, 2, false, true, true) \
    X(false, 3, 1, true, true, true) X(false, 1, 1, true, true, true)                                                             \
    X(false, 3, 1, false, true, true) X(false, 3, 2, false, true, true) X(false, 1, 1, false, true, true) X(false, 1, 2, false, true, true) \
    X(true, 3, 1, false, false, false) X(true, 3, 1, false, true, false) X(true, 3, 2, false, false, false) X(true, 3, 2, false, true, false) \
    X(true, 1, 1, false, false, false) X(true, 1, 1, false, true, false) X(true, 1, 2, false, false, false) X(true, 1, 2, false, true, false) \
    X(false, 3, 1, true, true, false) X(false, 1, 1, true, true, false)                                                           \
    X(false, 3, 1, false, false, false) X(false, 3, 1, false, true, false) X(false, 3, 2, false, false, false) X(false, 3, 2, false, true, false) \
    X(false, 1, 1, false, false, false) X(false, 1, 1, false, true, false) X(false, 1, 2, false, false, false) X(false, 1, 2, false, true, false)
// K2, packed 5/3: int16 planes (PX 0), 8-bit pixels in the default layout (CH 0) or interleaved with CH samples per pixel -- the
// triple, or one component (the fourth of four-channel pixels; any of three- / four-channel pixels without a colour transform)
#define GRK_DWT_PK_INSTANCES(X) /* NC, PX, NT, CH */                                                                              \
    X(1, 0, 128, 0) X(1, 0, 256, 0)                                                                                               \
    X(1, 1, 128, 1) X(1, 1, 256, 1) X(3, 1, 128, 3) X(3, 1, 256, 3) X(1, 1, 128, 3) X(1, 1, 256, 3)                               \
    X(3, 1, 128, 4) X(3, 1, 256, 4) X(1, 1, 128, 4) X(1, 1, 256, 4)                                                               \
    X(3, 1, 128, 0) X(1, 1, 128, 0) X(3, 1, 256, 0) X(1, 1, 256, 0)
// K2, two packed 5/3 levels in one launch (pair::dwt53_pk_kernel): the triple from 8-bit pixels in the default layout
#define GRK_DWT_PAIR_INSTANCES(X) /* NC, PX, NT */                                                                                \
    X(3, 1, 128) X(3, 1, 256)
// K6, 32-bit: every level but the fused one (NC 1, PXO 0); the last level to 8- / 16-bit pixels (PXO 1 / 2) in the default layout
// or a layout of the caller's (STR)
#define GRK_IDWT_INSTANCES(X) /* F97, NC, PXO, H16, STR */                                                                        \
    X(true, 1, 0, false, false) X(false, 1, 0, true, false) X(false, 1, 0, false, false)                                          \
    X(true, 3, 1, false, true) X(true, 3, 2, false, true) X(true, 1, 1, false, true) X(true, 1, 2, false, true)                   \
    X(true, 3, 1, false, false) X(true, 3, 2, false, false) X(true, 1, 1, false, false) X(true, 1, 2, false, false)               \
    X(false, 3, 1, true, true) X(false, 3, 2, true, true) X(false, 1, 1, true, true) X(false, 1, 2, true, true)                   \
    X(false, 3, 1, false, true) X(false, 3, 2, false, true) X(false, 1, 1, false, true) X(false, 1, 2, false, true)               \
    X(false, 3, 1, true, false) X(false, 3, 2, true, false) X(false, 1, 1, true, false) X(false, 1, 2, true, false)               \
    X(false, 3, 1, false, false) X(false, 3, 2, false, false) X(false, 1, 1, false, false) X(false, 1, 2, false, false)
// K6, packed 5/3: int16 planes (PXO 0); 8-bit pixels: one-channel pixels at the caller's pitches, the triple into three- / four-channel
// pixels, the default layout
#define GRK_IDWT_PK_INSTANCES(X) /* NC, PXO, CH */                                                                                \
    X(1, 0, 0) X(1, 1, 1) X(3, 1, 3) X(3, 1, 4) X(3, 1, 0) X(1, 1, 0)
// K7 stand-alone: 8- / 16-bit pixels in either kind of layout, int32 in the default one
#define GRK_EGRESS_INSTANCES(X) /* bytes, NC, STR */                                                                              \
    X(1, 1, true) X(1, 2, true) X(1, 3, true) X(1, 4, true) X(2, 1, true) X(2, 2, true) X(2, 3, true) X(2, 4, true)               \
    X(1, 1, false) X(1, 2, false) X(1, 3, false) X(1, 4, false) X(2, 1, false) X(2, 2, false) X(2, 3, false) X(2, 4, false)       \
    X(4, 1, false) X(4, 2, false) X(4, 3, false) X(4, 4, false)

#define GRK_INSTANCE_ROW(...) {__VA_ARGS__},
inline constexpr DwtKey    kDwtInstances[]    = {GRK_DWT_INSTANCES(GRK_INSTANCE_ROW)};
inline constexpr DwtPkKey  kDwtPkInstances[]  = {GRK_DWT_PK_INSTANCES(GRK_INSTANCE_ROW)};
inline constexpr DwtPairKey kDwtPairInstances[] = {GRK_DWT_PAIR_INSTANCES(GRK_INSTANCE_ROW)};
inline constexpr IdwtKey   kIdwtInstances[]   = {GRK_IDWT_INSTANCES(GRK_INSTANCE_ROW)};
inline constexpr IdwtPkKey kIdwtPkInstances[] = {GRK_IDWT_PK_INSTANCES(GRK_INSTANCE_ROW)};
inline constexpr EgressKey kEgressInstances[] = {GRK_EGRESS_INSTANCES(GRK_INSTANCE_ROW)};

} // namespace grk_amd
