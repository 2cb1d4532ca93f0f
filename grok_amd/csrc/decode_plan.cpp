// grok_amd/csrc/decode_plan.cpp -- the host's planning for a decode call (decode_plan.h): regions, table checks, launch lists.
#include "decode_plan.h"
#include <algorithm>
#include <new>

namespace grk_amd {
namespace {
inline uint32_t sat(uint32_t a, uint32_t b) { return a > b ? a - b : 0u; }
inline bool row_outside(const grk_amd_coded_block& r, uint64_t coded_bytes) { return r.offset > coded_bytes || r.length > coded_bytes - r.offset; }
inline int refuse(const char** why, int code, const char* what) { *why = what; return code; }
constexpr const char* kRowOutside = "block table row points outside the coded buffer";
constexpr const char* kSegMismatch = "segment list does not match the number of blocks";
} // namespace

// (a level that starts on an odd coordinate works on the coordinate grid shifted by the parity, kernels_idwt.hip: sample c
//  of the level belongs to pair (c + parity) / 2, pair J's low-pass sample has index J - parity, its high-pass sample J)
RegionPlan plan_region(const TileGeom& g, Rect win)
{
    RegionPlan r;
    const uint32_t L = g.p.num_levels, M = g.p.irreversible ? 4u : 2u;
    r.need.resize(L + 1); r.pairs.resize(L); r.px.resize(L); r.py.resize(L);
    r.need[0] = win;
    for (uint32_t l = 0; l < L; ++l) {
        const ResGeom& R = level_geom(g, l);
        const uint32_t px = R.x0 & 1u, py = R.y0 & 1u;
        const uint32_t npx = (R.w + px + 1) >> 1, npy = (R.h + py + 1) >> 1;       // pairs on the coordinate grid
        const uint32_t sw = (R.w + 1 - px) >> 1, sh = (R.h + 1 - py) >> 1;         // low-pass samples
        r.px[l] = px; r.py[l] = py;
        const Rect n = r.need[l];
        Rect q;
        q.x0 = sat((n.x0 + px) / 2, M); q.y0 = sat((n.y0 + py) / 2, M);
        q.x1 = std::min(npx, (n.x1 - 1 + px) / 2 + M + 1); q.y1 = std::min(npy, (n.y1 - 1 + py) / 2 + M + 1);
        r.pairs[l] = q;
        Rect lo;                                             // what of LL_{l+1} those pairs read
        lo.x0 = std::min(sat(q.x0, px), sw); lo.y0 = std::min(sat(q.y0, py), sh);
        lo.x1 = std::min(std::max(sat(q.x1, px), lo.x0 + 1), sw); lo.y1 = std::min(std::max(sat(q.y1, py), lo.y0 + 1), sh);
        r.need[l + 1] = lo;
    }
    return r;
}

void skip_blocks_outside(const TileGeom& g, const RegionPlan& plan, grk_amd_coded_block* rows)
{
    const uint32_t L = g.p.num_levels;
    size_t i = 0;
    for (uint32_t k = 0; k < g.p.num_comps; ++k)
        for (const auto& b : g.blocks_comp0) {
            // the block in its band's own index space against what the synthesis reads of that band: low-pass indices
            // are pair - parity, high-pass indices the pair itself
            const BandGeom& B = g.res[b.res].band[b.res ? b.band - 1 : 0];
            Rect need;
            if (b.res == 0) need = plan.need[L];
            else {
                const uint32_t l = L - b.res;
                const Rect& q = plan.pairs[l];
                const uint32_t px = plan.px[l], py = plan.py[l];
                need.x0 = (b.band & 1) ? q.x0 : sat(q.x0, px); need.x1 = (b.band & 1) ? q.x1 : sat(q.x1, px);
                need.y0 = (b.band & 2) ? q.y0 : sat(q.y0, py); need.y1 = (b.band & 2) ? q.y1 : sat(q.y1, py);
            }
            const uint32_t bx0 = b.x0 - B.x0, bx1 = b.x1 - B.x0, by0 = b.y0 - B.y0, by1 = b.y1 - B.y0;
            if (bx0 >= need.x1 || bx1 <= need.x0 || by0 >= need.y1 || by1 <= need.y0) {
                rows[i].offset = 0; rows[i].length = 0; rows[i].missing_msbs = kSkipBlock;
            }
            ++i;
        }
}

int check_table(const grk_amd_coded_block* table, uint64_t nblocks, uint64_t coded_bytes, const char** why)
{
    for (uint64_t i = 0; i < nblocks; ++i)
        if (row_outside(table[i], coded_bytes)) return refuse(why, GRK_AMD_ERR_INVALID, kRowOutside);
    return GRK_AMD_OK;
}

int plan_ht_blocks(const grk_amd_coded_block* table, uint64_t nblocks, uint64_t coded_bytes, uint32_t* active, uint32_t* nactive,
                   uint32_t* max_len, const char** why)
{
    uint32_t longest = 0, n = 0;
    for (uint64_t i = 0; i < nblocks; ++i) {
        longest = std::max(longest, table[i].length);
        if (row_outside(table[i], coded_bytes)) return refuse(why, GRK_AMD_ERR_INVALID, kRowOutside);
        if (table[i].length) active[n++] = (uint32_t)i;
    }
    if (longest > (48u << 10)) return refuse(why, GRK_AMD_ERR_UNSUPPORTED, "code-block longer than 48 KiB");
    *nactive = n; *max_len = longest;
    return GRK_AMD_OK;
}

int reduce_segments(uint64_t groups, uint32_t full_per_comp, uint32_t kept_per_comp, const std::vector<uint32_t>& first,
                    const std::vector<grk_amd_segment>& segs, std::vector<uint32_t>& red_first, std::vector<grk_amd_segment>& red_segs,
                    const char** why)
{
    if (first.size() != groups * full_per_comp + 1 || first.back() != segs.size()) return refuse(why, GRK_AMD_ERR_INVALID, kSegMismatch);
    red_first.clear(); red_segs.clear();
    for (uint64_t k = 0; k < groups; ++k)
        for (uint64_t i = k * full_per_comp, e = i + kept_per_comp; i < e; ++i) {
            red_first.push_back((uint32_t)red_segs.size());
            red_segs.insert(red_segs.end(), segs.begin() + first[i], segs.begin() + first[i + 1]);
        }
    red_first.push_back((uint32_t)red_segs.size());
    return GRK_AMD_OK;
}

int select_segments(bool reduced, const std::vector<uint32_t>& first, const std::vector<grk_amd_segment>& segs,
                    const std::vector<uint32_t>& red_first, const std::vector<grk_amd_segment>& red_segs, uint64_t nblocks,
                    SegList* out, const char** why)
{
    const std::vector<uint32_t>& f = reduced ? red_first : first;
    const std::vector<grk_amd_segment>& s = reduced ? red_segs : segs;
    *out = SegList{};
    if (f.empty()) return GRK_AMD_OK;
    if (f.size() != nblocks + 1 || f.back() != s.size()) return refuse(why, GRK_AMD_ERR_INVALID, kSegMismatch);
    out->first = f.data(); out->nfirst = f.size(); out->segs = s.data(); out->nsegs = s.size();
    return GRK_AMD_OK;
}

int plan_ht_refinement(const grk_amd_coded_block* table, uint64_t nblocks, const SegList& sl, grk_amd_segment* ref,
                       uint32_t* max_refine_bytes, const char** why)
{
    uint32_t longest = 0;
    for (uint64_t i = 0; i < nblocks; ++i) {
        ref[i] = grk_amd_segment{0u, 1u};
        const uint32_t s0 = sl.first[i], ns = sl.first[i + 1] - s0;
        if (ns > 2) return refuse(why, GRK_AMD_ERR_INVALID, "an HT code-block has at most two codeword segments");
        uint64_t sum = 0;
        for (uint32_t k = 0; k < ns; ++k) sum += sl.segs[s0 + k].length;
        if (ns && sum != table[i].length) return refuse(why, GRK_AMD_ERR_INVALID, "segment lengths do not add up to the block's length");
        if (ns == 2 && sl.segs[s0 + 1].length) {
            const uint32_t passes = 1u + std::min<uint32_t>(sl.segs[s0 + 1].numpasses, 2u);
            ref[i] = grk_amd_segment{sl.segs[s0 + 1].length, passes};
            longest = std::max(longest, ref[i].length);
        }
    }
    if (longest > (16u << 10)) return refuse(why, GRK_AMD_ERR_UNSUPPORTED, "refinement segment longer than 16 KiB");
    *max_refine_bytes = longest;
    return GRK_AMD_OK;
}

bool decode_takes_planes16(bool setting, bool force32, bool fuse_out, const grk_amd_tile_params& p, bool have_segments)
{
    return setting && !force32 && fuse_out && !p.reserved[0] && !p.irreversible && p.prec <= 8 && !have_segments;
}

// Which decoder takes which block.  A block is one dependent chain of MQ decisions (about ten per coded byte); 64 chains
// to a wave (K8L) make the throughput, but a chain alone in a wave (K8) advances ~2.5 times faster, and a frame's time
// is its longest chain's: the blocks longer than a quarter of the longest one -- a handful: the LL band -- and
// whatever the lane form does not take go to K8, longest first; the rest to K8L, sorted by length so that the lanes of a
// wave finish together.
int plan_t1_lists(const T1PlanIn& in, uint32_t* h_lane, uint32_t* h_tail, T1Lists* out, const char** why)
{
    const grk_amd_coded_block* const table = in.table;
    const uint64_t nblocks = in.nblocks;
    uint32_t n_lane = 0, n_tail = 0;
    *out = T1Lists{};
    const bool lanes_on = in.t1_lanes && in.cblksty == 0 && !in.have_segments && nblocks <= 0xFFFFFFFFull;
    if (!lanes_on) return GRK_AMD_OK;
    auto eligible = [&](uint64_t i) {
        const uint32_t bps = table[i].missing_msbs & 0xFFu, np = table[i].missing_msbs >> 8;
        // (a row with more passes than its bit-planes can have -- a malformed packet header -- would alias into another group of
        //  the pass-synchronous waves: K8 takes it and stops where the data does)
        return table[i].length != 0 && table[i].missing_msbs != kSkipBlock && np != 0 && bps != 0 && bps <= kT1LaneMaxPlanes &&
               np <= 3u * bps - 2u && in.block_h[i % in.blocks_per_tile] >= kT1LaneMinRows;
    };
    uint32_t max_len = 0;
    for (uint64_t i = 0; i < nblocks; ++i) max_len = std::max(max_len, table[i].length);
    const uint32_t thr = (uint32_t)std::min<double>((double)max_len, std::max(64.0, 0.25 * max_len));
    // counting sort by length (4-byte buckets), longest first.  The bucket index is clamped: a code-block of 64 x 64 samples
    // cannot need more than 64 KiB, and a row that CLAIMS hundreds of megabytes (a malformed packet header: the length is
    // bounded by the coded buffer only) must not cost a table of that size -- such rows share the top bucket, i.e. sort first
    // and go to K8's list like every long block
    constexpr uint32_t kMaxBucketLen = 64u << 10;
    const uint32_t nb = (std::min(max_len, kMaxBucketLen) >> 2) + 2u;
    auto bucket = [&](uint64_t i) { return nb - 1u - (std::min(table[i].length, kMaxBucketLen) >> 2); };
    std::vector<uint32_t> cnt, order;
    try { cnt.assign(nb + 1, 0u); order.resize(nblocks); }
    catch (const std::bad_alloc&) { return refuse(why, GRK_AMD_ERR_NOMEM, "host memory for the Part-1 launch lists"); }
    out->buckets = nb + 1;
    for (uint64_t i = 0; i < nblocks; ++i) cnt[bucket(i)]++;
    uint32_t run = 0;
    for (uint32_t k = 0; k <= nb; ++k) { const uint32_t v = cnt[k]; cnt[k] = run; run += v; }
    for (uint64_t i = 0; i < nblocks; ++i) order[cnt[bucket(i)]++] = (uint32_t)i;
    for (uint64_t k = 0; k < nblocks; ++k) {
        const uint32_t i = order[k];
        if (table[i].length <= thr && eligible(i)) h_lane[n_lane++] = i; else h_tail[n_tail++] = i;
    }
    if (n_lane >= 64u && in.pass_sync) {
        // pass-synchronous waves: a wave's lanes go from pass to pass together, so a wave holds blocks with the SAME number of
        // bit-planes and passes (table word missing_msbs), longest first within the group; a group fills whole waves (spare
        // lanes: kT1NoBlock); groups too small for a wave go to K8
        std::vector<uint32_t> lane(h_lane, h_lane + n_lane);
        auto key = [&](uint32_t i) { return (((table[i].missing_msbs >> 8) & 0xFFu) << 4) | (table[i].missing_msbs & 0xFu); };   // passes, planes (<= 14)
        constexpr uint32_t kKeys = 256u << 4;
        std::vector<uint32_t> cnt(kKeys, 0u), at(kKeys, 0u);
        for (uint32_t i : lane) cnt[key(i)]++;
        uint32_t filled = 0;
        // (a group that would fill only a few waves runs them from pass to pass half empty, and with more passes than the
        //  bulk it is the kernel's last wave to finish: groups below 0.5 % of the lane blocks go to K8 as well)
        const uint32_t min_group = std::max<uint32_t>(64u, n_lane / 200u);
        for (uint32_t k = kKeys; k-- > 0;) {                              // (more passes first: the longest-running waves start first)
            if (cnt[k] < min_group) { at[k] = kT1NoBlock; continue; }
            at[k] = filled;
            filled += (cnt[k] + 63u) & ~63u;
        }
        for (uint32_t j = 0; j < filled; ++j) h_lane[j] = kT1NoBlock;
        for (uint32_t i : lane) {                                         // (the groups keep the longest-first order)
            const uint32_t k = key(i);
            if (at[k] == kT1NoBlock) h_tail[n_tail++] = i; else h_lane[at[k]++] = i;
        }
        n_lane = filled;
    }
    if (n_lane >= 64u) {
        // Is the lane form the faster one for THIS call?  A lane's chain advances at ~10 ns per coded byte (0.85 us per step, ~10
        // decisions per byte, ~30 % of the steps idle), a wave's at ~2.5 ns per byte, and K8's throughput with every SIMD full is
        // ~0.9 ns per byte (r03: 55 MB in 48 ms): a small image -- fewer blocks than K8 has wave slots -- is done sooner by K8
        // alone, in the time of its longest block.
        uint64_t bytes_all = 0, bytes_tail = 0;
        uint32_t max_lane = 0, max_tail = 0;
        for (uint64_t i = 0; i < nblocks; ++i) bytes_all += table[i].length;
        for (uint32_t j = 0; j < n_lane; ++j) if (h_lane[j] != kT1NoBlock) max_lane = std::max(max_lane, table[h_lane[j]].length);
        for (uint32_t j = 0; j < n_tail; ++j) { bytes_tail += table[h_tail[j]].length; max_tail = std::max(max_tail, table[h_tail[j]].length); }
        const double t_k8 = std::max(2.5e-9 * max_len, 0.9e-9 * (double)bytes_all);
        const double t_mix = std::max(std::max(10.0e-9 * max_lane, 2.5e-9 * max_tail), 0.9e-9 * (double)bytes_tail);
        if (t_k8 <= t_mix && in.t1_lanes != 2) n_lane = 0;
    }
    if (n_lane < 64u) { n_lane = 0; n_tail = 0; }                   // not worth a second launch: K8 in table order
    out->n_lane = n_lane; out->n_tail = n_tail;
    return GRK_AMD_OK;
}

// ---- the shape of an inverse DWT level -------------------------------------------------------------------------------------------
// the instance of a part of nc components (1, or 3: the MCT triple) of a level of shape s, and its strips (strips32: the 32-bit kernels')
static IdwtInstance idwt_instance(const IdwtLevelDesc& d, const IdwtLevelShape& s, uint8_t nc, uint32_t strips32)
{
    IdwtInstance in{};
    const uint8_t pxo = !d.fused ? 0 : d.px_bytes == 1 ? 1 : 2;
    in.packed = s.packed;
    in.pk = IdwtPkKey{nc, pxo, 0};
    if (d.fused) {
        // 8-bit pixels clamped to 0..255 (the packed store saturates to that), the whole tile
        const bool whole = s.wx0 == 0 && s.wy0 == 0 && s.wx1 == d.cw && s.wy1 == d.ch;
        in.packed = s.packed && pxo == 1 && d.lo == 0 && d.hi == 255 && whole;
        if (d.px_lay != 0) {
            // a layout of the caller's: one-channel pixels, or the MCT triple into three- / four-channel ones, tiles and rows on
            // 4-byte alignment (whole dwords are stored), row offsets within 32 bits; the strided back end otherwise
            const bool al = ((d.px_align | d.px_row | d.px_tile) & 3u) == 0 && d.px_row * d.ch < (1ull << 31);
            const bool lay = d.px_lay == 2 && ((d.px_chan == 1 && nc == 1) || ((d.px_chan == 3 || d.px_chan == 4) && nc == 3 && d.mct));
            in.packed = in.packed && al && lay;
            in.pk = IdwtPkKey{nc, 1, (uint8_t)d.px_chan};
        } else {
            in.packed = in.packed && (nc == 1 || d.mct);
        }
    }
    in.k = IdwtKey{d.irreversible, nc, pxo, d.h16 && !d.irreversible, d.fused && d.px_lay != 0};
    in.grid_x = in.packed ? (d.cw + ipk_strip_cols(d.cw) - 1) / ipk_strip_cols(d.cw) : strips32;
    return in;
}

IdwtLevelShape plan_idwt_level(const IdwtLevelDesc& d)
{
    IdwtLevelShape s{};
    const uint32_t col_pairs = (d.cw + d.px + 1) >> 1, row_pairs = (d.ch + d.py + 1) >> 1;      // pairs on the coordinate grid
    // (row offsets are 32-bit byte offsets from a plane's first sample: planes of 2^31 samples and more keep the flat addressing)
    const bool near = (uint64_t)d.m_stride * d.ch < (1ull << 31) && (uint64_t)d.out_stride * d.ch < (1ull << 31);
    // d.pk: the caller's word that the inputs are inside the packed range
    s.packed = d.h16 && d.pk && !d.irreversible && (d.px | d.py) == 0 && (d.cw & 3u) == 0 && d.cw >= 256u && d.ch >= 16 &&
               (d.ch & 1u) == 0 && !d.region && near;
    s.strip_pairs = s.packed ? ipk_strip_cols(d.cw) / 2 : kIdwtStripPairs;
    // The row segments are sized from s.packed's strips, although the fused level can still take the 32-bit kernel and its narrower
    // strips (idwt_instance: signed or fewer than 8 bits, a window, a layout the packed kernel does not write, a misaligned pointer):
    // its grid then has more workgroups than the segments were sized for.  Kept as it was -- it decides grids, so speed.
    s.seg_pairs = row_segment_pairs((col_pairs + s.strip_pairs - 1) / s.strip_pairs, row_pairs, d.zslots, kIdwtMinWgs);
    s.wx0 = 0; s.wy0 = 0; s.wx1 = d.cw; s.wy1 = d.ch;
    if (d.region) {       // the strips and row segments that produce `need`
        const Rect n = d.need;
        s.seg_pairs = kIdwtRegionSegPairs;
        s.strip0 = ((n.x0 + d.px) / 2) / kIdwtStripPairs; s.nstrips = ((n.x1 - 1 + d.px) / 2) / kIdwtStripPairs - s.strip0 + 1;
        s.seg0 = ((n.y0 + d.py) / 2) / s.seg_pairs; s.nsegs = ((n.y1 - 1 + d.py) / 2) / s.seg_pairs - s.seg0 + 1;
        if (d.fused) { s.wx0 = n.x0; s.wy0 = n.y0; s.wx1 = n.x1; s.wy1 = n.y1; }
    }
    // strips x row segments: all of them, or the region's sub-grid
    const uint32_t strips32 = s.nstrips ? s.nstrips : (col_pairs + kIdwtStripPairs - 1) / kIdwtStripPairs;
    s.grid_y = s.nsegs ? s.nsegs : (row_pairs + s.seg_pairs - 1) / s.seg_pairs;
    s.inst[0] = idwt_instance(d, s, 1, strips32);
    if (d.fused) s.inst[1] = idwt_instance(d, s, 3, strips32);
    s.grid_x = s.inst[0].grid_x;
    return s;
}

EgressKey egress_key(uint32_t px_lay, uint32_t bytes_per_sample, uint32_t ncomp)
{
    const uint8_t bytes = bytes_per_sample == 1 ? 1 : bytes_per_sample == 2 ? 2 : 4;      // (4: int32 out)
    return EgressKey{bytes, (uint8_t)(ncomp <= 4 ? ncomp : 0), px_lay != 0 && bytes != 4};
}

} // namespace grk_amd
