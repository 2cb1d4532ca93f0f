// grok_amd/csrc/geometry.cpp -- see geometry.h for the reference citations.
#include "geometry.h"
#include "image.h"
#include "t2_order.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

namespace grk_amd {

// BIBO gains of the 5/3 analysis filter bank indexed by decomposition count; these are the
// constants OpenJPH/Grok use to size the reversible HT exponents (codestream/HTParams.cpp:139-154).
static const float kBibo53L[] = {1.0000e+00f, 1.5000e+00f, 1.6250e+00f, 1.6875e+00f, 1.6963e+00f,
                                 1.7067e+00f, 1.7116e+00f, 1.7129e+00f, 1.7141e+00f, 1.7145e+00f,
                                 1.7151e+00f, 1.7152e+00f};
static const float kBibo53H[] = {2.0000e+00f, 2.5000e+00f, 2.7500e+00f, 2.8047e+00f, 2.8198e+00f,
                                 2.8410e+00f, 2.8558e+00f, 2.8601e+00f, 2.8628e+00f, 2.8656e+00f,
                                 2.8662e+00f, 2.8667e+00f};
// sqrt of the 9/7 synthesis energy gains (HTParams.cpp:72-87)
static const float kGain97L[] = {1.0000e+00f, 1.4021e+00f, 2.0304e+00f, 2.9012e+00f, 4.1153e+00f,
                                 5.8245e+00f, 8.2388e+00f, 1.1652e+01f, 1.6479e+01f, 2.3304e+01f,
                                 3.2957e+01f, 4.6609e+01f};
static const float kGain97H[] = {1.4425e+00f, 1.9669e+00f, 2.8839e+00f, 4.1475e+00f, 5.8946e+00f,
                                 8.3472e+00f, 1.1809e+01f, 1.6701e+01f, 2.3620e+01f, 3.3403e+01f,
                                 4.7240e+01f, 6.6807e+01f};

static int guard_log2(float g) { return (int)std::ceil(std::log(g * 1.1f) / M_LN2); }

static uint16_t irrev_word(float delta)
{
    uint32_t e = 0;
    while (delta < 1.0f) { ++e; delta *= 2.0f; }
    uint32_t mant = (uint32_t)std::round(delta * (float)(1 << 11)) - (1u << 11);
    if (mant >= (1u << 11)) mant = 0x7FF;
    return (uint16_t)((e << 11) | mant);
}

// QCD words in marker order [LL, then per resolution HL LH HH].
// Reversible: Grok calls qcd.generate() before tcp->mct is set, so the RCT guard bit is never
// added -- reproduced here on purpose.
static void make_qcd(const grk_amd_tile_params& p, uint16_t* w)
{
    const uint32_t L = p.num_levels;
    uint32_t s = 0;
    if (!p.irreversible) {
        int B = p.prec;
        w[s++] = (uint16_t)((B + guard_log2(kBibo53L[L] * kBibo53L[L])) << 3);
        for (int d = (int)L - 1; d >= 0; --d) {
            float l = kBibo53L[d + 1], h = kBibo53H[d];
            uint16_t x = (uint16_t)((B + guard_log2(h * l)) << 3);
            w[s++] = x; w[s++] = x;
            w[s++] = (uint16_t)((B + guard_log2(h * h)) << 3);
        }
    } else {
        float base = 1.0f / (float)(1u << (p.prec + (p.sgnd ? 1 : 0)));
        w[s++] = irrev_word(base / (kGain97L[L] * kGain97L[L]));
        for (int d = (int)L - 1; d >= 0; --d) {
            float l = kGain97L[d + 1], h = kGain97H[d];
            uint16_t x = irrev_word(base / (l * h));
            w[s++] = x; w[s++] = x;
            w[s++] = irrev_word(base / (h * h));
        }
    }
}

static int build_tile_geom_uncached(const grk_amd_tile_params& p, TileGeom& g);

// The geometry of a tile is asked for again and again with the same parameters -- per tile when an image is laid out, per call of
// the codestream writer, twice by a caller that sizes before it writes -- and enumerating the 49 152 code-blocks of an 8K tile takes
// 1.4 ms of host time: the last few are kept (a copy is ~0.05 ms).
int build_tile_geom(const grk_amd_tile_params& p, TileGeom& g)
{
    static std::mutex mu;
    static std::vector<std::shared_ptr<const TileGeom>> cache;             // most recent last
    {
        std::lock_guard<std::mutex> lk(mu);
        for (size_t i = cache.size(); i-- > 0;)
            if (std::memcmp(&cache[i]->p, &p, sizeof p) == 0) { g = *cache[i]; return GRK_AMD_OK; }
    }
    const int rc = build_tile_geom_uncached(p, g);
    if (rc != GRK_AMD_OK) return rc;
    auto keep = std::make_shared<const TileGeom>(g);
    std::lock_guard<std::mutex> lk(mu);
    if (cache.size() >= 8) cache.erase(cache.begin());
    cache.push_back(std::move(keep));
    return GRK_AMD_OK;
}

static int build_tile_geom_uncached(const grk_amd_tile_params& p, TileGeom& g)
{
    if (p.tile_w == 0 || p.tile_h == 0 || p.num_comps == 0 || p.num_comps > 4) return GRK_AMD_ERR_INVALID;
    if (p.prec == 0 || p.prec > 16) return GRK_AMD_ERR_UNSUPPORTED;
    if (p.num_levels > GRK_AMD_MAX_LEVELS) return GRK_AMD_ERR_UNSUPPORTED;
    if (p.cblk_w_exp < 2 || p.cblk_w_exp > 6 || p.cblk_h_exp < 2 || p.cblk_h_exp > 6) return GRK_AMD_ERR_UNSUPPORTED;
    if (p.mct && p.num_comps < 3) return GRK_AMD_ERR_INVALID;
    // one precinct per resolution (default exponent 15, CodeStreamCompress.cpp:514-518)
    if (p.tile_w > 32768 || p.tile_h > 32768) return GRK_AMD_ERR_UNSUPPORTED;
    if ((uint64_t)p.tile_x0 + p.tile_w > 0x7FFFFFFFull || (uint64_t)p.tile_y0 + p.tile_h > 0x7FFFFFFFull) return GRK_AMD_ERR_UNSUPPORTED;


    g.p = p;
    g.stride = (p.tile_w + 31u) & ~31u;                       // util/MemManager.cpp:38-43
    g.plane_elems = (uint64_t)g.stride * p.tile_h;
    const uint32_t L = p.num_levels;
    make_qcd(p, g.qcd_words);
    g.num_bands_total = 3 * L + 1;
    g.res.assign(L + 1, ResGeom{});
    g.blocks_comp0.clear();
    uint32_t nblk = 0;
    // tile-component origin on the canonical grid (dx = dy = 1: the tile's own): resolution r covers
    // [ceil(x0 / 2^(L-r)), ceil((x0 + w) / 2^(L-r))), band b of it [ceil((x0 - 2^(n-1) xb) / 2^n), ...) with n = L - r + 1
    // (TileComponent.cpp:131-138, util/util.cpp:49-58).  The code-blocks of a band are the cells of the 2^cblk grid anchored
    // at the origin of the BAND's coordinates that the band touches (T1Structs.cpp:118-136): a band that starts off that
    // grid begins with a partial block.
    const uint64_t X0 = p.tile_x0, Y0 = p.tile_y0, X1 = X0 + p.tile_w, Y1 = Y0 + p.tile_h;
    auto res_lo = [](uint64_t v, uint32_t n) { return (uint32_t)((v + (1ull << n) - 1) >> n); };
    auto band_lo = [](uint64_t v, uint32_t n, uint32_t hi) {
        const uint64_t off = hi ? (1ull << (n - 1)) : 0;
        return v <= off ? 0u : (uint32_t)((v - off + (1ull << n) - 1) >> n);
    };
    for (uint32_t r = 0; r <= L; ++r) {
        ResGeom& R = g.res[r];
        R.x0 = res_lo(X0, L - r); R.y0 = res_lo(Y0, L - r);
        R.w = res_lo(X1, L - r) - R.x0;
        R.h = res_lo(Y1, L - r) - R.y0;
        uint32_t lw = r ? res_lo(X1, L - r + 1) - res_lo(X0, L - r + 1) : 0;
        uint32_t lh = r ? res_lo(Y1, L - r + 1) - res_lo(Y0, L - r + 1) : 0;
        R.num_bands = r ? 3 : 1;
        // precincts (T1Structs.cpp:449-493, TileComponent.cpp:100-118): the grid of 2^PPx x 2^PPy cells anchored at the
        // origin of the resolution's coordinates that the resolution touches; in a band of resolution r > 0 a precinct is
        // half as large, and a code-block is never larger than the band's part of a precinct
        const uint32_t pe = p.precinct_exp[r];
        R.ppx = pe ? (pe & 15u) : 15u; R.ppy = pe ? (pe >> 4) : 15u;
        if (r && (R.ppx == 0 || R.ppy == 0)) return GRK_AMD_ERR_INVALID;
        R.npw = R.w ? (uint32_t)((((uint64_t)R.x0 + R.w + (1ull << R.ppx) - 1) >> R.ppx) - (R.x0 >> R.ppx)) : 0;
        R.nph = R.h ? (uint32_t)((((uint64_t)R.y0 + R.h + (1ull << R.ppy) - 1) >> R.ppy) - (R.y0 >> R.ppy)) : 0;
        if ((uint64_t)R.npw * R.nph > (1u << 22)) return GRK_AMD_ERR_UNSUPPORTED;
        const uint32_t bpx = R.ppx - (r ? 1u : 0u), bpy = R.ppy - (r ? 1u : 0u);                 // precinct exponents in the bands
        const uint32_t psx = ((R.x0 >> R.ppx) << R.ppx) >> (r ? 1u : 0u), psy = ((R.y0 >> R.ppy) << R.ppy) >> (r ? 1u : 0u);
        const uint32_t cxe = std::min<uint32_t>(p.cblk_w_exp, bpx), cye = std::min<uint32_t>(p.cblk_h_exp, bpy);
        for (uint32_t bi = 0; bi < R.num_bands; ++bi) {
            BandGeom& B = R.band[bi];
            B.orient = (uint8_t)(r ? bi + 1 : 0);
            const uint32_t n = r ? L - r + 1 : L;
            if (n == 0) { B.x0 = (uint32_t)X0; B.y0 = (uint32_t)Y0; B.w = p.tile_w; B.h = p.tile_h; }
            else {
                B.x0 = band_lo(X0, n, B.orient & 1u); B.y0 = band_lo(Y0, n, B.orient >> 1);
                B.w = band_lo(X1, n, B.orient & 1u) - B.x0;
                B.h = band_lo(Y1, n, B.orient >> 1) - B.y0;
            }
            B.ox = (B.orient & 1) ? lw : 0;
            B.oy = (B.orient & 2) ? lh : 0;
            uint32_t qi = r ? 3 * (r - 1) + 1 + bi : 0;
            B.qcd = g.qcd_words[qi];
            uint32_t gain = B.orient == 0 ? 0 : (B.orient == 3 ? 2 : 1);
            if (!p.irreversible) {
                uint32_t expn = B.qcd >> 3;
                B.kmax = (uint8_t)expn;                       // numbps = expn + numgbits(1) - 1
                B.stepsize = (float)std::pow(2.0, (int)(p.prec + gain) - (int)expn);
            } else {
                uint32_t expn = B.qcd >> 11, mant = B.qcd & 0x7FF;
                B.kmax = (uint8_t)expn;
                B.stepsize = (float)((1.0 + mant / 2048.0) * std::pow(2.0, (int)(p.prec + gain) - (int)expn));
            }
            if (B.kmax > 30) return GRK_AMD_ERR_UNSUPPORTED;
            B.first_block = nblk;
            B.prec.assign((size_t)R.npw * R.nph, BandGeom::Prec{0, 0, nblk});
            for (uint32_t pj = 0; pj < R.nph; ++pj)
                for (uint32_t pi = 0; pi < R.npw; ++pi) {
                    BandGeom::Prec& P = B.prec[(size_t)pj * R.npw + pi];
                    P.first_block = nblk;
                    // the band's part of the precinct, in the band's coordinates
                    const uint64_t qx0 = (uint64_t)psx + ((uint64_t)pi << bpx), qy0 = (uint64_t)psy + ((uint64_t)pj << bpy);
                    const uint64_t rx0 = std::max<uint64_t>(qx0, B.x0), rx1 = std::min<uint64_t>(qx0 + (1ull << bpx), (uint64_t)B.x0 + B.w);
                    const uint64_t ry0 = std::max<uint64_t>(qy0, B.y0), ry1 = std::min<uint64_t>(qy0 + (1ull << bpy), (uint64_t)B.y0 + B.h);
                    if (rx0 >= rx1 || ry0 >= ry1) continue;
                    const uint32_t gx0 = (uint32_t)(rx0 >> cxe), gy0 = (uint32_t)(ry0 >> cye);
                    P.gw = (uint32_t)((rx1 + (1ull << cxe) - 1) >> cxe) - gx0;
                    P.gh = (uint32_t)((ry1 + (1ull << cye) - 1) >> cye) - gy0;
                    for (uint32_t by = 0; by < P.gh; ++by)
                        for (uint32_t bx = 0; bx < P.gw; ++bx) {
                            grk_amd_block b;
                            std::memset(&b, 0, sizeof(b));
                            b.x0 = (uint32_t)std::max<uint64_t>((uint64_t)(gx0 + bx) << cxe, rx0);
                            b.y0 = (uint32_t)std::max<uint64_t>((uint64_t)(gy0 + by) << cye, ry0);
                            b.x1 = (uint32_t)std::min<uint64_t>((uint64_t)(gx0 + bx + 1) << cxe, rx1);
                            b.y1 = (uint32_t)std::min<uint64_t>((uint64_t)(gy0 + by + 1) << cye, ry1);
                            b.px = B.ox + (b.x0 - B.x0); b.py = B.oy + (b.y0 - B.y0);
                            b.comp = 0; b.res = (uint8_t)r; b.band = B.orient; b.kmax = B.kmax;
                            b.stepsize = B.stepsize;
                            b.precinct = pj * R.npw + pi;
                            g.blocks_comp0.push_back(b);
                            ++nblk;
                        }
                }
            B.num_blocks = nblk - B.first_block;
        }
    }
    g.blocks_per_comp = nblk;
    g.reduce = 0;
    g.full_blocks_per_comp = nblk;
    g.full_bands_total = g.num_bands_total;
    return GRK_AMD_OK;
}

int reduced_tile_rect(const grk_amd_tile_params& p, uint32_t reduce, uint32_t* x0, uint32_t* y0, uint32_t* w, uint32_t* h)
{
    if (reduce > p.num_levels || p.tile_w == 0 || p.tile_h == 0) return GRK_AMD_ERR_INVALID;
    const uint64_t X0 = p.tile_x0, Y0 = p.tile_y0, X1 = X0 + p.tile_w, Y1 = Y0 + p.tile_h;
    auto lo = [reduce](uint64_t v) { return (uint32_t)((v + (1ull << reduce) - 1) >> reduce); };
    *x0 = lo(X0); *y0 = lo(Y0);
    *w = lo(X1) - lo(X0); *h = lo(Y1) - lo(Y0);
    return GRK_AMD_OK;
}

int reduce_tile_geom(const TileGeom& full, uint32_t reduce, TileGeom& g)
{
    if (full.reduce != 0) return GRK_AMD_ERR_INVALID;
    const uint32_t L = full.p.num_levels;
    if (reduce > L) return GRK_AMD_ERR_INVALID;
    g = full;
    if (reduce == 0) return GRK_AMD_OK;
    const uint32_t Lr = L - reduce;
    const ResGeom& top = full.res[Lr];             // resolution L - reduce is the reduced tile itself (res_lo nests: ceil of ceil)
    g.p.num_levels = (uint8_t)Lr;
    g.p.tile_x0 = top.x0; g.p.tile_y0 = top.y0;
    g.p.tile_w = top.w; g.p.tile_h = top.h;
    g.res.resize(Lr + 1);
    g.blocks_per_comp = Lr < L ? full.res[Lr + 1].band[0].first_block : full.blocks_per_comp;
    g.blocks_comp0.resize(g.blocks_per_comp);
    g.num_bands_total = 3 * Lr + 1;
    g.stride = (g.p.tile_w + 31u) & ~31u;
    g.plane_elems = (uint64_t)g.stride * g.p.tile_h;
    g.reduce = reduce;
    return GRK_AMD_OK;
}

// the same sub-band partition, block partition and lifting variants: what one batch of grk_amd_encode_tiles needs
bool same_geometry(const TileGeom& a, const TileGeom& b)
{
    if (a.p.tile_w != b.p.tile_w || a.p.tile_h != b.p.tile_h || a.blocks_per_comp != b.blocks_per_comp) return false;
    for (size_t r = 0; r < a.res.size(); ++r)
        if (a.res[r].w != b.res[r].w || a.res[r].h != b.res[r].h || a.res[r].npw != b.res[r].npw || a.res[r].nph != b.res[r].nph || ((a.res[r].x0 ^ b.res[r].x0) & 1u) || ((a.res[r].y0 ^ b.res[r].y0) & 1u))
            return false;
    for (size_t i = 0; i < a.blocks_comp0.size(); ++i) {
        const grk_amd_block &x = a.blocks_comp0[i], &y = b.blocks_comp0[i];
        if (x.px != y.px || x.py != y.py || x.x1 - x.x0 != y.x1 - y.x0 || x.y1 - x.y0 != y.y1 - y.y0 || x.res != y.res || x.band != y.band ||
            x.precinct != y.precinct)
            return false;
    }
    return true;
}

// Two tiles of one geometry whose packets come in the same (component, resolution, precinct) sequence.  For LRCP and RLCP the
// sequence is resolution, component, raster -- the geometry's alone.  The position-major orders walk the precincts by their
// corners on the reference grid clipped to the tile: where the corners of different resolutions coincide depends on where the
// tile lies, and same_geometry does not look at that.
bool same_packets(const TileGeom& a, const TileGeom& b, uint32_t order)
{
    if (order <= 1) return true;
    if (a.p.num_comps != b.p.num_comps) return false;
    const std::vector<const TileGeom*> ca(a.p.num_comps, &a), cb(b.p.num_comps, &b);
    const std::vector<Pk> sa = packet_order(ca, nullptr, nullptr, a.p.tile_x0, a.p.tile_y0, order);
    const std::vector<Pk> sb = packet_order(cb, nullptr, nullptr, b.p.tile_x0, b.p.tile_y0, order);
    if (sa.size() != sb.size()) return false;
    for (size_t i = 0; i < sa.size(); ++i)
        if (sa[i].c != sb[i].c || sa[i].r != sb[i].r || sa[i].pi != sb[i].pi) return false;
    return true;
}

} // namespace grk_amd

// One layer's packets of a tile in progression order (t2_order.h; what the five orders are: t2_writer.cpp, with the tile-part writer)
std::vector<grk_amd::Pk> grk_amd::packet_order(const std::vector<const TileGeom*>& cg, const uint8_t* comp_dx, const uint8_t* comp_dy, uint32_t gx0, uint32_t gy0,
                             uint32_t order)
{
    const uint32_t ncomp = (uint32_t)cg.size();
    const grk_amd_tile_params& p = cg[0]->p;
    std::vector<Pk> prec;                                   // every precinct of the tile: component-major, resolution-major, raster
    for (uint32_t c = 0; c < ncomp; ++c) {
        const TileGeom& g = *cg[c];
        const uint64_t dx = comp_dx && comp_dx[c] ? comp_dx[c] : 1, dy = comp_dy && comp_dy[c] ? comp_dy[c] : 1;
        for (uint32_t r = 0; r <= p.num_levels; ++r) {
            const ResGeom& R = g.res[r];
            const uint32_t sh = p.num_levels - r;
            for (uint32_t pj = 0; pj < R.nph; ++pj)
                for (uint32_t pi = 0; pi < R.npw; ++pi) {
                    const uint64_t cx = (((uint64_t)((R.x0 >> R.ppx) + pi) << R.ppx) << sh) * dx, cy = (((uint64_t)((R.y0 >> R.ppy) + pj) << R.ppy) << sh) * dy;
                    prec.push_back(Pk{c, r, pj * R.npw + pi, std::max<uint64_t>(cx, gx0), std::max<uint64_t>(cy, gy0)});
                }
        }
    }
    // (stable sorts of the component-major, resolution-major, raster list: the keys named, everything else in that order)
    if (order <= 1)                // resolution, component, precinct
        std::stable_sort(prec.begin(), prec.end(), [](const Pk& a, const Pk& b) { return a.r != b.r ? a.r < b.r : a.c < b.c; });
    else if (order == 2)           // resolution, position, component
        std::stable_sort(prec.begin(), prec.end(), [](const Pk& a, const Pk& b) {
            return a.r != b.r ? a.r < b.r : a.y != b.y ? a.y < b.y : a.x != b.x ? a.x < b.x : a.c < b.c; });
    else if (order == 3)           // position, component, resolution
        std::stable_sort(prec.begin(), prec.end(), [](const Pk& a, const Pk& b) {
            return a.y != b.y ? a.y < b.y : a.x != b.x ? a.x < b.x : a.c != b.c ? a.c < b.c : a.r < b.r; });
    else                           // component, position, resolution
        std::stable_sort(prec.begin(), prec.end(), [](const Pk& a, const Pk& b) {
            return a.c != b.c ? a.c < b.c : a.y != b.y ? a.y < b.y : a.x != b.x ? a.x < b.x : a.r < b.r; });
    return prec;
}

// the tiles of a sub-sampled image in classes of one joint plan each (t2_order.h)
uint32_t grk_amd::joint_tile_classes(const std::vector<uint32_t>& of, uint32_t nruns, uint32_t order, const std::vector<std::vector<Pk>>& seq,
                                     std::vector<uint32_t>& class_of)
{
    const uint32_t ntiles = nruns ? (uint32_t)(of.size() / nruns) : 0u;
    class_of.assign(ntiles, 0);
    std::vector<uint32_t> lead;                              // [class]: its first tile
    auto same = [&](uint32_t a, uint32_t b) {
        for (uint32_t k = 0; k < nruns; ++k) if (of[(size_t)a * nruns + k] != of[(size_t)b * nruns + k]) return false;
        if (order <= 1) return true;
        if (seq[a].size() != seq[b].size()) return false;
        for (size_t i = 0; i < seq[a].size(); ++i)
            if (seq[a][i].c != seq[b][i].c || seq[a][i].r != seq[b][i].r || seq[a][i].pi != seq[b][i].pi) return false;
        return true;
    };
    for (uint32_t t = 0; t < ntiles; ++t) {
        uint32_t k = 0;
        while (k < lead.size() && !same(lead[k], t)) ++k;
        if (k == lead.size()) lead.push_back(t);
        class_of[t] = k;
    }
    return (uint32_t)lead.size();
}

// the next unit of a whole-image call into its geometry group (image.h)
int grk_amd::add_unit(UnitGroups& g, const grk_amd_tile_params& p, uint32_t order)
{
    TileGeom geom;
    const int rc = build_tile_geom(p, geom);
    if (rc) return rc;
    size_t k = 0;
    for (; k < g.geoms.size(); ++k)
        if (g.geoms[k].p.num_comps == p.num_comps && g.geoms[k].p.mct == p.mct && same_geometry(g.geoms[k], geom) &&
            same_packets(g.geoms[k], geom, order)) break;
    if (k == g.geoms.size()) { g.geoms.push_back(std::move(geom)); g.members.emplace_back(); }
    g.members[k].push_back((uint32_t)g.of.size());
    g.of.push_back((uint32_t)k);
    return GRK_AMD_OK;
}

extern "C" int64_t grk_amd_tile_num_blocks(const grk_amd_tile_params* p)
{
    if (!p) return GRK_AMD_ERR_INVALID;
    grk_amd::TileGeom g;
    int rc = grk_amd::build_tile_geom(*p, g);
    if (rc != GRK_AMD_OK) return rc;
    return (int64_t)g.blocks_per_comp * p->num_comps;
}

extern "C" int grk_amd_same_tile_packets(const grk_amd_tile_params* a, const grk_amd_tile_params* b, uint32_t flags)
{
    if (!a || !b) return GRK_AMD_ERR_INVALID;
    grk_amd::TileGeom ga, gb;
    int rc = grk_amd::build_tile_geom(*a, ga); if (rc) return rc;
    rc = grk_amd::build_tile_geom(*b, gb); if (rc) return rc;
    return a->num_comps == b->num_comps && grk_amd::same_geometry(ga, gb) &&
           grk_amd::same_packets(ga, gb, (flags >> GRK_AMD_CS_PROG_SHIFT) & 7u) ? 1 : 0;
}

// ---- tiles divided into tile-parts (GRK_AMD_CS_TP; t2_order.h) -----------------------------------------------------------------------
// The reference's rule (CodeStreamCompress::get_num_tp, pi_enable_tile_part_generation) for this encoder's one layer: with `pos` the
// place of the division letter in the progression order's name, a packet's key is its coordinates for the letters 0 .. pos, and a new
// tile-part starts where the key changes.  The parts are the keys, whether or not a key has packets: the product of the letters'
// extents (L: 1, R: num_levels + 1, C: num_comps).  A P at or before the division letter multiplies by a bound on the precincts in the
// reference and normally fails its own limit: refused here.
namespace {
thread_local std::string g_writer_error;
const char* const kOrderNames[5] = {"LRCP", "RLCP", "RPCL", "PCRL", "CPRL"};
}

int grk_amd::writer_refuse(int code, const std::string& why) { g_writer_error = why; return code; }
extern "C" const char* grk_amd_writer_last_error(void) { return g_writer_error.c_str(); }

int grk_amd::tile_part_count(uint32_t flags, uint32_t num_levels, uint32_t num_comps, std::string* why)
{
    const uint32_t d = (flags >> GRK_AMD_CS_TP_SHIFT) & 3u, order = (flags >> GRK_AMD_CS_PROG_SHIFT) & 7u;
    if (!d) return 1;
    auto refuse = [&](const std::string& s) { if (why) *why = s; return (int)GRK_AMD_ERR_UNSUPPORTED; };
    if (order > 4) { if (why) *why = "no such progression order"; return GRK_AMD_ERR_INVALID; }
    const char letter = d == GRK_AMD_TP_R ? 'R' : d == GRK_AMD_TP_L ? 'L' : 'C';
    const char* const name = kOrderNames[order];
    uint64_t n = 1;
    for (uint32_t i = 0;; ++i) {
        if (name[i] == 'P')
            return refuse(std::string("tile-parts divided at ") + letter + " under " + name + ": a P at or before the division letter");
        n *= name[i] == 'R' ? num_levels + 1u : name[i] == 'C' ? num_comps : 1u;
        if (name[i] == letter) break;
    }
    if (n > 255) return refuse(std::to_string(n) + " tile-parts per tile: TPsot takes at most 255");
    return (int)n;
}

int grk_amd::tile_part_starts(const std::vector<Pk>& seq, uint32_t flags, uint32_t num_levels, uint32_t num_comps, std::vector<uint32_t>& starts,
                              std::string* why)
{
    const int n = tile_part_count(flags, num_levels, num_comps, why);
    if (n < 0) return n;
    starts.assign((size_t)n, 0);
    if (n == 1) return n;
    const uint32_t d = (flags >> GRK_AMD_CS_TP_SHIFT) & 3u, order = (flags >> GRK_AMD_CS_PROG_SHIFT) & 7u;
    const char letter = d == GRK_AMD_TP_R ? 'R' : d == GRK_AMD_TP_L ? 'L' : 'C';
    const char* const name = kOrderNames[order];
    std::vector<uint32_t> count((size_t)n, 0);
    for (const Pk& q : seq) {
        uint32_t key = 0;                                   // the key as a number: the letters' coordinates, the first the most significant
        for (uint32_t i = 0;; ++i) {
            if (name[i] == 'R') key = key * (num_levels + 1u) + q.r;
            else if (name[i] == 'C') key = key * num_comps + q.c;
            if (name[i] == letter) break;
        }
        ++count[key];
    }
    for (int k = 1; k < n; ++k) starts[k] = starts[k - 1] + count[k - 1];
    return n;
}

extern "C" int64_t grk_amd_tile_part_starts(const grk_amd_tile_params* tile, const uint8_t* comp_dx, const uint8_t* comp_dy, uint32_t flags,
                                            uint32_t* starts, uint32_t cap, uint32_t* num_packets)
{
    using namespace grk_amd;
    if (!tile || !tile->num_comps || (!comp_dx != !comp_dy)) return writer_refuse(GRK_AMD_ERR_INVALID, "grk_amd_tile_part_starts: no tile, or one of comp_dx / comp_dy alone");
    if (((flags >> GRK_AMD_CS_PROG_SHIFT) & 7u) > 4) return writer_refuse(GRK_AMD_ERR_INVALID, "no such progression order");
    const uint32_t nc = tile->num_comps;
    // (the rule's refusals need the letters' extents alone: said before the geometry is looked at)
    { std::string why; const int n = tile_part_count(flags, tile->num_levels, nc, &why); if (n < 0) return writer_refuse(n, why); }
    // component c's tile-component: the tile's rectangle in its own coordinates (grk_amd_layout_tile_comp)
    std::vector<TileGeom> geoms(nc);
    std::vector<const TileGeom*> cg(nc);
    const uint64_t x0 = tile->tile_x0, y0 = tile->tile_y0, x1 = x0 + tile->tile_w, y1 = y0 + tile->tile_h;
    for (uint32_t c = 0; c < nc; ++c) {
        const uint64_t dx = comp_dx && comp_dx[c] ? comp_dx[c] : 1, dy = comp_dy && comp_dy[c] ? comp_dy[c] : 1;
        grk_amd_tile_params p = *tile;
        const uint64_t cx0 = (x0 + dx - 1) / dx, cy0 = (y0 + dy - 1) / dy, cx1 = (x1 + dx - 1) / dx, cy1 = (y1 + dy - 1) / dy;
        if (cx1 <= cx0 || cy1 <= cy0) return writer_refuse(GRK_AMD_ERR_UNSUPPORTED, "a tile without a sample of a component");
        p.tile_x0 = (uint32_t)cx0; p.tile_y0 = (uint32_t)cy0; p.tile_w = (uint32_t)(cx1 - cx0); p.tile_h = (uint32_t)(cy1 - cy0);
        if (c && dx == (comp_dx && comp_dx[c - 1] ? comp_dx[c - 1] : 1) && dy == (comp_dy && comp_dy[c - 1] ? comp_dy[c - 1] : 1)) { cg[c] = cg[c - 1]; continue; }
        const int rc = build_tile_geom(p, geoms[c]);
        if (rc) return writer_refuse(rc, "grk_amd_tile_part_starts: the tile's parameters are refused");
        cg[c] = &geoms[c];
    }
    const std::vector<Pk> seq = packet_order(cg, comp_dx, comp_dy, tile->tile_x0, tile->tile_y0, (flags >> GRK_AMD_CS_PROG_SHIFT) & 7u);
    std::vector<uint32_t> s;
    std::string why;
    const int n = tile_part_starts(seq, flags, tile->num_levels, nc, s, &why);
    if (n < 0) return writer_refuse(n, why);
    if (num_packets) *num_packets = (uint32_t)seq.size();
    if (starts) {
        if ((uint32_t)n > cap) return writer_refuse(GRK_AMD_ERR_OVERFLOW, "grk_amd_tile_part_starts: more tile-parts than `cap`");
        std::copy(s.begin(), s.end(), starts);
    }
    return n;
}
