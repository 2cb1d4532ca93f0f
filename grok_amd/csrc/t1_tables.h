// grok_amd/csrc/t1_tables.h -- the Part-1 (EBCOT / MQ) coding rules both block decoders take their tables from: T.800 Table C.2
// (MQ states), Table D.1 (zero coding) and Tables D.2 / D.3 (sign coding), and K8's packed forms of them (kernels_t1dec.hip).
// K8L (t1_lanes.h) folds the same rules into its LDS tables.  Plain C++17: it also compiles on the host, where
// tests/test_t1_lanes_sim.py checks every packed form against the rules.
#pragma once
#include <stdint.h>

namespace t1 {

// Table C.2: Qe, NMPS, NLPS, SWITCH
struct MqRow { uint16_t qe; uint8_t nmps, nlps, sw; };
constexpr MqRow kMq[47] = {
    {0x5601, 1, 1, 1},  {0x3401, 2, 6, 0},  {0x1801, 3, 9, 0},  {0x0AC1, 4, 12, 0}, {0x0521, 5, 29, 0},
    {0x0221, 38, 33, 0}, {0x5601, 7, 6, 1},  {0x5401, 8, 14, 0}, {0x4801, 9, 14, 0}, {0x3801, 10, 14, 0},
    {0x3001, 11, 17, 0}, {0x2401, 12, 18, 0}, {0x1C01, 13, 20, 0}, {0x1601, 29, 21, 0}, {0x5601, 15, 14, 1},
    {0x5401, 16, 14, 0}, {0x5101, 17, 15, 0}, {0x4801, 18, 16, 0}, {0x3801, 19, 17, 0}, {0x3401, 20, 18, 0},
    {0x3001, 21, 19, 0}, {0x2801, 22, 19, 0}, {0x2401, 23, 20, 0}, {0x2201, 24, 21, 0}, {0x1C01, 25, 22, 0},
    {0x1801, 26, 23, 0}, {0x1601, 27, 24, 0}, {0x1401, 28, 25, 0}, {0x1201, 29, 26, 0}, {0x1101, 30, 27, 0},
    {0x0AC1, 31, 28, 0}, {0x09C1, 32, 29, 0}, {0x08A1, 33, 30, 0}, {0x0521, 34, 31, 0}, {0x0441, 35, 32, 0},
    {0x02A1, 36, 33, 0}, {0x0221, 37, 34, 0}, {0x0141, 38, 35, 0}, {0x0111, 39, 36, 0}, {0x0085, 40, 37, 0},
    {0x0049, 41, 38, 0}, {0x0025, 42, 39, 0}, {0x0015, 43, 40, 0}, {0x0009, 44, 41, 0}, {0x0005, 45, 42, 0},
    {0x0001, 45, 43, 0}, {0x5601, 46, 46, 0}};

// Zero-coding context (Table D.1) by orientation (0 LL, 1 HL, 2 LH, 3 HH) and the eight neighbour significance bits: row above
// (x-1, x, x+1) in bits 0-2, left and right neighbour in bits 3-4, row below in bits 5-7
constexpr int zc_context(int orient, uint32_t idx)
{
    const uint32_t w0 = idx & 7u, l = (idx >> 3) & 1u, r = (idx >> 4) & 1u, w2 = idx >> 5;
    int hh = (int)l + (int)r;
    int vv = (int)((w0 >> 1) & 1u) + (int)((w2 >> 1) & 1u);
    const int dd = (int)(w0 & 1u) + (int)((w0 >> 2) & 1u) + (int)(w2 & 1u) + (int)((w2 >> 2) & 1u);
    if (orient == 1) { const int t = hh; hh = vv; vv = t; }
    if (orient == 3) {
        const int hv = hh + vv;
        if (dd >= 3) return 8;
        if (dd == 2) return hv >= 1 ? 7 : 6;
        if (dd == 1) return hv >= 2 ? 5 : (hv == 1 ? 4 : 3);
        return hv >= 2 ? 2 : hv;
    }
    if (hh == 2) return 8;
    if (hh == 1) return vv >= 1 ? 7 : (dd >= 1 ? 6 : 5);
    if (vv == 2) return 4;
    if (vv == 1) return 3;
    return dd >= 2 ? 2 : dd;
}
// ... by the NINE bits of a sample's 3 x 3 window as the decoders keep them (row above in bits 0-2, own row in 3-5 -- the centre
// bit does not matter --, row below in 6-8)
constexpr uint32_t zc_context9(int orient, uint32_t nine)
{
    const uint32_t w0 = nine & 7u, w1 = (nine >> 3) & 7u, w2 = nine >> 6;
    return (uint32_t)zc_context(orient, w0 | ((w1 & 1u) << 3) | ((w1 & 4u) << 2) | (w2 << 5));
}

// Sign-coding context and XOR bit (Tables D.2 / D.3) by the significance and sign of the four horizontal / vertical neighbours:
// significant (up, left, right, down) in bits 0, 2, 4, 6 of idx -- bits 1, 3, 5, 7 of a 3 x 3 window shifted down by one --,
// negative in the bit above each
struct SignCx { uint32_t cx, xr; };
constexpr SignCx sign_rule(uint32_t idx)
{
    int c[4] = {0, 0, 0, 0};
    for (int k = 0; k < 4; ++k) c[k] = ((idx >> (2 * k)) & 1u) ? (((idx >> (2 * k + 1)) & 1u) ? -1 : 1) : 0;
    int hc = c[1] + c[2], vc = c[0] + c[3];
    hc = hc > 1 ? 1 : (hc < -1 ? -1 : hc); vc = vc > 1 ? 1 : (vc < -1 ? -1 : vc);
    if (hc == 1) return {vc == 1 ? 13u : (vc == 0 ? 12u : 11u), 0u};
    if (hc == 0) return {vc == 0 ? 9u : 10u, vc == -1 ? 1u : 0u};
    return {vc == 1 ? 11u : (vc == 0 ? 12u : 13u), 1u};
}

// ---- K8's forms: dwords that live across the lanes of one register each and are read with v_readlane ----------------------
// Table C.2, one state per dword: Qe | NMPS << 16 | NLPS << 22 | SWITCH << 28
struct MqWords {
    uint32_t w[47];
    constexpr MqWords() : w{}
    {
        for (int i = 0; i < 47; ++i)
            w[i] = (uint32_t)kMq[i].qe | ((uint32_t)kMq[i].nmps << 16) | ((uint32_t)kMq[i].nlps << 22) | ((uint32_t)kMq[i].sw << 28);
    }
};
// zero-coding contexts by orientation and the nine window bits: 4 bits per entry, eight entries per dword (lane i: entries
// 8 i .. 8 i + 7)
struct ZcLut {
    uint32_t w[4][64];
    constexpr ZcLut() : w{}
    {
        for (int o = 0; o < 4; ++o)
            for (uint32_t i = 0; i < 512; ++i) w[o][i >> 3] |= zc_context9(o, i) << (4 * (i & 7u));
    }
};
// sign-coding context | XOR bit << 4 by the sign index, one byte each
struct SignLut {
    uint32_t w[64];
    constexpr SignLut() : w{}
    {
        for (uint32_t i = 0; i < 256; ++i) {
            const SignCx s = sign_rule(i);
            w[i >> 2] |= (s.cx | (s.xr << 4)) << (8 * (i & 3u));
        }
    }
};

} // namespace t1
