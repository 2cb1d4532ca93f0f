// grok_amd/csrc/decode.hip -- decode: block decoding (HT K5, Part-1 K8 / K8L), inverse DWT, egress, regions and sequences.
#include "context.h"

namespace {
// Region decode (the reference: grk_decompress_set_window -> WaveletReverse.cpp:1466-2213 partial
// synthesis over a sparse buffer).  need[l] = the part of LL_l (l = 0: the image) that has to be right so that the
// window is; level l is synthesised from the coefficient pairs pairs[l] of LL_{l+1} and of resolution L - l's bands.
// A synthesised sample depends on the pairs within 1 (5/3) or 2 (9/7) of its own, the kernel's strip halo and the
// recurrence warm-up reach 2 pairs further: the margins below are conservative on purpose.
struct Rect { uint32_t x0, y0, x1, y1; };
struct RegionPlan { std::vector<Rect> need, pairs; std::vector<uint32_t> px, py; };
// (a level that starts on an odd coordinate works on the coordinate grid shifted by the parity, kernels_idwt.hip: sample c
//  of the level belongs to pair (c + parity) / 2, pair J's low-pass sample has index J - parity, its high-pass sample J)
RegionPlan plan_region(const TileGeom& g, Rect win)
{
    RegionPlan r;
    const uint32_t L = g.p.num_levels, M = g.p.irreversible ? 4u : 2u;
    r.need.resize(L + 1); r.pairs.resize(L); r.px.resize(L); r.py.resize(L);
    r.need[0] = win;
    auto sat = [](uint32_t a, uint32_t b) { return a > b ? a - b : 0u; };
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

// d_pixels != nullptr: the last level writes the pixels itself (K7 fused, out_bytes 1 or 2) and d_out is not touched;
// plan != nullptr: only what the window needs is synthesised, and d_pixels is the window (K7 fused required)
int run_idwt(grk_amd_ctx* c, uint32_t nplanes, const void* d_mallat, void* d_out, void* d_pixels = nullptr,
             uint32_t ntiles = 0, uint32_t out_bytes = 0, const RegionPlan* plan = nullptr, bool h16 = false, const PixelLayout* px = nullptr)
{
    const TileGeom& g = c->geom;
    const uint32_t L = g.p.num_levels;
    const uint32_t W = g.p.tile_w, H = g.p.tile_h;
    if (L == 0) {
        HIP_TRY(c, hipMemcpyAsync(d_out, d_mallat, (size_t)nplanes * g.plane_elems * 4, hipMemcpyDeviceToDevice, c->stream), "copy planes");
        return GRK_AMD_OK;
    }
    // same ping-pong storage as the forward transform: A holds LL1, LL3, ...; B holds LL2, LL4, ...
    const uint32_t sA = ll_stride_for(W), hA = (H + 1) >> 1;
    const uint32_t sB = ll_stride_for((W + 1) >> 1), hB = (hA + 1) >> 1;
    const uint64_t pitchA = (uint64_t)sA * hA, pitchB = (uint64_t)sB * hB;
    HIP_TRY(c, c->llA.ensure((size_t)nplanes * pitchA * 4 + 256), "alloc LL ping");
    HIP_TRY(c, c->llB.ensure((size_t)nplanes * pitchB * 4 + 256), "alloc LL pong");
    ScopedTimer t(c, 6);
    for (int32_t l = (int32_t)L - 1; l >= 0; --l) {
        IdwtLevelArgs a{};
        a.cw = level_geom(g, (uint32_t)l).w; a.ch = level_geom(g, (uint32_t)l).h;
        a.px = level_geom(g, (uint32_t)l).x0 & 1u; a.py = level_geom(g, (uint32_t)l).y0 & 1u;
        if ((uint32_t)l + 1 == L) { a.ll = (const int32_t*)d_mallat; a.ll_stride = g.stride; a.ll_pitch = g.plane_elems; }
        else if ((l + 1) & 1) { a.ll = (const int32_t*)c->llA.p; a.ll_stride = sA; a.ll_pitch = pitchA; }
        else { a.ll = (const int32_t*)c->llB.p; a.ll_stride = sB; a.ll_pitch = pitchB; }
        a.mallat = (const int32_t*)d_mallat; a.m_stride = g.stride; a.m_pitch = g.plane_elems;
        if (l == 0) { a.out = (int32_t*)d_out; a.out_stride = g.stride; a.out_pitch = g.plane_elems; }
        else if (l & 1) { a.out = (int32_t*)c->llA.p; a.out_stride = sA; a.out_pitch = pitchA; }
        else { a.out = (int32_t*)c->llB.p; a.out_stride = sB; a.out_pitch = pitchB; }
        a.nplanes = nplanes;
        a.irreversible = g.p.irreversible;
        a.xcd = c->dwt_xcd;
        a.h16 = h16 ? 1 : 0; a.status = (unsigned int*)c->flag.p;
        a.pk = h16 && c->dwt_pk && !plan;            // (the block decoder flagged every coefficient outside the packed range)
        if (l == 0 && d_pixels && px && px->lay) {
            a.px_lay = px->lay; a.px_chan = px->channels; a.px_xstep = px->xstep; a.px_fill = px->fill;
            a.px_row = px->row; a.px_kstep = px->kstep; a.px_tile = px->tile;
        }
        const uint32_t sh = (a.ch + a.py + 1) >> 1;
        uint32_t seg = 64;
        const uint64_t strips = (((a.cw + a.px + 1) >> 1) + idwt_level_strip_pairs(a) - 1) / idwt_level_strip_pairs(a);
        const uint32_t zslots = (l == 0 && d_pixels) ? ntiles * ((g.p.mct && g.p.num_comps >= 3) ? 1u : g.p.num_comps) : nplanes;
        while (seg > 8 && strips * ((sh + seg - 1) / seg) * zslots < 4096) seg >>= 1;
        a.seg_pairs = seg;
        a.wx0 = 0; a.wy0 = 0; a.wx1 = a.cw; a.wy1 = a.ch;
        if (plan) {       // the strips and row segments that produce need[l]
            const Rect n = plan->need[(uint32_t)l];
            const uint32_t op = idwt_strip_pairs();
            seg = 16;
            a.seg_pairs = seg;
            a.strip0 = ((n.x0 + a.px) / 2) / op; a.nstrips = ((n.x1 - 1 + a.px) / 2) / op - a.strip0 + 1;
            a.seg0 = ((n.y0 + a.py) / 2) / seg; a.nsegs = ((n.y1 - 1 + a.py) / 2) / seg - a.seg0 + 1;
            if (l == 0) { a.wx0 = n.x0; a.wy0 = n.y0; a.wx1 = n.x1; a.wy1 = n.y1; }
        }
        if (a.cw == 0 || a.ch == 0) continue;       // (a level without samples, see run_dwt)
        if (l == 0 && c->dec_top_pending) {           // the top resolution's blocks are decoded on the side stream
            HIP_TRY(c, hipStreamWaitEvent(c->stream, c->ev_dec_top, 0), "wait for the top resolution's blocks");
            c->dec_top_pending = false;
        }
        if (l == 0 && d_pixels) {
            a.pixels = d_pixels; a.px_bytes = out_bytes;
            a.dc = g.p.sgnd ? 0 : (1 << (g.p.prec - 1));
            a.lo = g.p.sgnd ? -(1 << (g.p.prec - 1)) : 0;
            a.hi = g.p.sgnd ? (1 << (g.p.prec - 1)) - 1 : (1 << g.p.prec) - 1;
            a.mct = g.p.mct;
            HIP_TRY(c, launch_idwt_level0_fused(a, ntiles, g.p.num_comps, c->stream), "launch fused idwt level 0");
        } else {
            HIP_TRY(c, launch_idwt_level(a, c->stream), "launch idwt level");
        }
    }
    return GRK_AMD_OK;
}

// The pinned tables of this call with the caller's rows in them (room for K5's index behind the rows); the set's last upload
// has been waited for (two calls ago: long done).  nblocks counts the rows of the context's geometry (a reduced one: fewer than
// the caller's table holds)
int stage_table(grk_amd_ctx* c, const grk_amd_coded_block* table, uint64_t nblocks, grk_amd_ctx::DecUpload** out)
{
    grk_amd_ctx::DecUpload* u = &c->dec_up[c->dec_turn++ & 1u];
    if (!u->ev) HIP_TRY(c, hipEventCreateWithFlags(&u->ev, hipEventDisableTiming), "create event");
    HIP_TRY(c, hipEventSynchronize(u->ev), "wait for the tables' last upload");
    const size_t need = (size_t)nblocks * (sizeof(grk_amd_coded_block) + 16) + 64;        // rows + the launch lists behind them
    if (u->cap < need) {
        if (u->p) (void)hipHostFree(u->p);
        u->p = u->dp = nullptr; u->cap = 0;
        HIP_TRY(c, hipHostMalloc((void**)&u->p, need, hipHostMallocDefault), "alloc pinned tables");
        HIP_TRY(c, hipHostGetDevicePointer((void**)&u->dp, u->p, 0), "map pinned tables");
        u->cap = need;
    }
    const TileGeom& g = c->geom;
    if (g.reduce) {             // the caller's rows are the full tile's: each component keeps its first blocks_per_comp rows
        const uint64_t groups = nblocks / g.blocks_per_comp;
        for (uint64_t k = 0; k < groups; ++k)
            std::memcpy(u->p + k * g.blocks_per_comp * sizeof(grk_amd_coded_block), table + k * g.full_blocks_per_comp,
                        (size_t)g.blocks_per_comp * sizeof(grk_amd_coded_block));
    } else {
        std::memcpy(u->p, table, (size_t)nblocks * sizeof(grk_amd_coded_block));
    }
    *out = u;
    return GRK_AMD_OK;
}

// rows (+ `extra` bytes behind them) -> dec_table on the call's stream, the status block cleared
int upload_table(grk_amd_ctx* c, grk_amd_ctx::DecUpload* u, size_t bytes)
{
    HIP_TRY(c, c->dec_table.ensure(bytes + 64), "alloc decode table");
    HIP_TRY(c, c->flag.ensure(kHtAllocBytes), "alloc status");
    HIP_TRY(c, launch_dec_upload(u->dp, c->dec_table.p, bytes, c->flag.p, c->stream), "upload decode tables");
    HIP_TRY(c, hipEventRecord(u->ev, c->stream), "record the tables' upload");
    return GRK_AMD_OK;
}

int run_ht_decode(grk_amd_ctx* c, uint32_t ntiles, grk_amd_ctx::DecUpload* up, const void* d_coded, uint64_t coded_bytes, void* d_mallat,
                  bool h16 = false, bool split = false)
{
    const TileGeom& g = c->geom;
    const uint32_t bpt = g.blocks_per_comp * g.p.num_comps;
    const uint64_t nblocks = (uint64_t)bpt * ntiles;
    const grk_amd_coded_block* const table = (const grk_amd_coded_block*)up->p;
    uint32_t max_len = 0;
    // behind the rows: the blocks that have data at all -- K5a's lanes (a window's skipped blocks and absent blocks do not cost a
    // lane of a serial chain)
    uint32_t* const h_active = (uint32_t*)(up->p + nblocks * sizeof(grk_amd_coded_block));
    uint32_t nactive = 0;
    for (uint64_t i = 0; i < nblocks; ++i) {
        max_len = std::max(max_len, table[i].length);
        if (table[i].offset > coded_bytes || table[i].length > coded_bytes - table[i].offset)
            return fail(c, GRK_AMD_ERR_INVALID, "block table row points outside the coded buffer");
        if (table[i].length) h_active[nactive++] = (uint32_t)i;
    }
    if (max_len > (48u << 10)) return fail(c, GRK_AMD_ERR_UNSUPPORTED, "code-block longer than 48 KiB");
    static_assert(sizeof(HtDecBlock) == sizeof(grk_amd_coded_block), "decode table rows are grk_amd_coded_block");
    HIP_TRY(c, c->dec_quads.ensure(nblocks * 1024 * 2 + 64), "alloc quad info");
    HIP_TRY(c, c->dec_mslen.ensure(nblocks * 4), "alloc ms lengths");
    { const int rc = upload_table(c, up, nblocks * sizeof(HtDecBlock) + (size_t)nactive * 4); if (rc) return rc; }
    const uint32_t* const d_active = (const uint32_t*)((const char*)c->dec_table.p + nblocks * sizeof(HtDecBlock));
    HtDecArgs a{};
    a.table = (const HtDecBlock*)c->dec_table.p;
    a.blocks = (const HtBlockDesc*)c->dec_desc.p; a.blocks_per_tile = bpt; a.nblocks = (uint32_t)nblocks; a.ncomp = g.p.num_comps;
    a.coded = (const uint8_t*)d_coded; a.coded_bytes = coded_bytes;
    a.quads = (uint32_t*)c->dec_quads.p; a.ms_len = (uint32_t*)c->dec_mslen.p; a.status = (unsigned int*)c->flag.p;
    a.active = nactive == nblocks ? nullptr : d_active; a.nactive = nactive;
    a.mallat = (int32_t*)d_mallat; a.stride = g.stride; a.pitch = g.plane_elems;
    a.irreversible = g.p.irreversible;
    a.h16 = h16 ? 1 : 0;
    a.h16_bias = (h16 && c->dwt_pk) ? 2048 : 32768;        // (pk16.h kPkDecodeBound + 1: the inverse transform runs on packed pairs)
    const std::vector<uint32_t>& seg_first = g.reduce ? c->red_seg_first : c->dec_seg_first;
    const std::vector<grk_amd_segment>& segs = g.reduce ? c->red_segs : c->dec_segs;
    if (!seg_first.empty()) {
        // HT blocks with refinement passes: segment 0 = the cleanup pass, segment 1 = SigProp (+ MagRef), end to end
        if (seg_first.size() != nblocks + 1 || seg_first.back() != segs.size())
            return fail(c, GRK_AMD_ERR_INVALID, "segment list does not match the number of blocks");
        std::vector<uint2> ref(nblocks, make_uint2(0u, 1u));
        for (uint64_t i = 0; i < nblocks; ++i) {
            const uint32_t s0 = seg_first[i], ns = seg_first[i + 1] - s0;
            if (ns > 2) return fail(c, GRK_AMD_ERR_INVALID, "an HT code-block has at most two codeword segments");
            uint64_t sum = 0;
            for (uint32_t k = 0; k < ns; ++k) sum += segs[s0 + k].length;
            if (ns && sum != table[i].length) return fail(c, GRK_AMD_ERR_INVALID, "segment lengths do not add up to the block's length");
            if (ns == 2 && segs[s0 + 1].length) {
                const uint32_t passes = 1u + std::min<uint32_t>(segs[s0 + 1].numpasses, 2u);
                ref[i] = make_uint2(segs[s0 + 1].length, passes);
                a.max_refine_bytes = std::max(a.max_refine_bytes, ref[i].x);
            }
        }
        if (a.max_refine_bytes > (16u << 10)) return fail(c, GRK_AMD_ERR_UNSUPPORTED, "refinement segment longer than 16 KiB");
        HIP_TRY(c, c->dec_seg_dev.ensure(nblocks * sizeof(uint2) + 16), "alloc refinement table");
        HIP_TRY(c, hipMemcpyAsync(c->dec_seg_dev.p, ref.data(), nblocks * sizeof(uint2), hipMemcpyHostToDevice, c->stream), "upload refinement table");
        HIP_TRY(c, hipStreamSynchronize(c->stream), "sync refinement table");       // (uploaded from a local)
        a.refine = (const uint2*)c->dec_seg_dev.p;
    }
    // K5b in two parts when the call goes on with the inverse transform (decode_impl): the levels below the last one need the
    // blocks of the lower resolutions only -- a quarter of them --, and those short, latency-bound launches hide beside the
    // top resolution's K5b on the low-priority side stream
    const uint32_t L = g.p.num_levels;
    const uint32_t first_top = L >= 1 ? g.res[L].band[0].first_block : 0;
    if (split && c->overlap && c->side && L >= 2 && !a.refine && first_top > 0 && first_top < g.blocks_per_comp) {
        if (!c->ev_dec_front) HIP_TRY(c, hipEventCreateWithFlags(&c->ev_dec_front, hipEventDisableTiming), "create event");
        if (!c->ev_dec_top) HIP_TRY(c, hipEventCreateWithFlags(&c->ev_dec_top, hipEventDisableTiming), "create event");
        HIP_TRY(c, launch_ht_decode_front(a, c->stream), "launch ht decode");
        HIP_TRY(c, hipEventRecord(c->ev_dec_front, c->stream), "record K5a");
        HIP_TRY(c, hipStreamWaitEvent(c->side, c->ev_dec_front, 0), "side stream waits for K5a");
        a.ms_bpc = g.blocks_per_comp;
        a.ms_first = first_top; a.ms_count = g.blocks_per_comp - first_top;
        HIP_TRY(c, launch_ht_decode_ms(a, max_len, c->side), "launch K5b, top resolution");
        HIP_TRY(c, hipEventRecord(c->ev_dec_top, c->side), "record K5b");
        c->dec_top_pending = true;
        a.ms_first = 0; a.ms_count = first_top;
        HIP_TRY(c, launch_ht_decode_ms(a, max_len, c->stream), "launch K5b, lower resolutions");
        return GRK_AMD_OK;
    }
    ScopedTimer t(c, 5);
    HIP_TRY(c, launch_ht_decode(a, max_len, c->stream), "launch ht decode");
    return GRK_AMD_OK;
}

int run_t1_decode(grk_amd_ctx* c, uint32_t ntiles, grk_amd_ctx::DecUpload* up, const void* d_coded, uint64_t coded_bytes, void* d_mallat)
{
    const TileGeom& g = c->geom;
    const uint32_t bpt = g.blocks_per_comp * g.p.num_comps;
    const uint64_t nblocks = (uint64_t)bpt * ntiles;
    const grk_amd_coded_block* const table = (const grk_amd_coded_block*)up->p;
    for (uint64_t i = 0; i < nblocks; ++i)
        if (table[i].offset > coded_bytes || table[i].length > coded_bytes - table[i].offset)
            return fail(c, GRK_AMD_ERR_INVALID, "block table row points outside the coded buffer");
    static_assert(kT1WorkBytes == 4096 * 4, "K8 and K8L share a block's part of the workspace");
    HIP_TRY(c, c->dec_work.ensure(nblocks * kT1WorkBytes), "alloc Part-1 workspace");
    // Which decoder takes which block.  A block is one dependent chain of MQ decisions (about ten per coded byte); 64 chains
    // to a wave (K8L) make the throughput, but a chain alone in a wave (K8) advances ~2.5 times faster, and a frame's time
    // is its longest chain's: the blocks longer than a quarter of the longest one -- a handful: the LL band -- and
    // whatever the lane form does not take go to K8, longest first; the rest to K8L, sorted by length so that the lanes of a
    // wave finish together.  Both lists behind the rows in the pinned tables (stage_table leaves 8 bytes per block).
    uint32_t* const h_lane = (uint32_t*)(up->p + nblocks * sizeof(grk_amd_coded_block));      // (room for 2 nblocks entries: padding)
    uint32_t* const h_tail = h_lane + 2 * nblocks;
    uint32_t n_lane = 0, n_tail = 0;
    const bool lanes_on = c->t1_lanes && g.p.reserved[1] == 0 && c->dec_seg_first.empty() && nblocks <= 0xFFFFFFFFull;
    if (lanes_on) {
        auto eligible = [&](uint64_t i) {
            const uint32_t bps = table[i].missing_msbs & 0xFFu, np = table[i].missing_msbs >> 8;
            // (a row with more passes than its bit-planes can have -- a malformed packet header -- would alias into another group of
            //  the pass-synchronous waves: K8 takes it and stops where the data does)
            return table[i].length != 0 && table[i].missing_msbs != kSkipBlock && np != 0 && bps != 0 && bps <= kT1LaneMaxPlanes &&
                   np <= 3u * bps - 2u && c->h_desc_dec[i % bpt].h >= kT1LaneMinRows;
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
        catch (const std::bad_alloc&) { return fail(c, GRK_AMD_ERR_NOMEM, "host memory for the Part-1 launch lists"); }
        for (uint64_t i = 0; i < nblocks; ++i) cnt[bucket(i)]++;
        uint32_t run = 0;
        for (uint32_t k = 0; k <= nb; ++k) { const uint32_t v = cnt[k]; cnt[k] = run; run += v; }
        for (uint64_t i = 0; i < nblocks; ++i) order[cnt[bucket(i)]++] = (uint32_t)i;
        for (uint64_t k = 0; k < nblocks; ++k) {
            const uint32_t i = order[k];
            if (table[i].length <= thr && eligible(i)) h_lane[n_lane++] = i; else h_tail[n_tail++] = i;
        }
        if (n_lane >= 64u && c->t1_pass_sync) {
            // pass-synchronous waves: a wave's lanes go from pass to pass together, so a wave holds blocks with the SAME number of
            // bit-planes and passes (table word missing_msbs), longest first within the group; a group fills whole waves (spare
            // lanes: kT1NoBlock); groups too small for a wave go to K8
            std::vector<uint32_t> lane(h_lane, h_lane + n_lane);
            auto key = [&](uint32_t i) { return (((table[i].missing_msbs >> 8) & 0xFFu) << 4) | (table[i].missing_msbs & 0xFu); };   // passes, planes (<= 14)
            constexpr uint32_t kKeys = 256u << 4;
            std::vector<uint32_t> cnt(kKeys, 0u), at(kKeys, 0u);
            for (uint32_t i : lane) cnt[key(i)]++;
            uint32_t out = 0;
            // (a group that would fill only a few waves runs them from pass to pass half empty, and with more passes than the
            //  bulk it is the kernel's last wave to finish: groups below 0.5 % of the lane blocks go to K8 as well)
            const uint32_t min_group = std::max<uint32_t>(64u, n_lane / 200u);
            for (uint32_t k = kKeys; k-- > 0;) {                              // (more passes first: the longest-running waves start first)
                if (cnt[k] < min_group) { at[k] = kT1NoBlock; continue; }
                at[k] = out;
                out += (cnt[k] + 63u) & ~63u;
            }
            for (uint32_t j = 0; j < out; ++j) h_lane[j] = kT1NoBlock;
            for (uint32_t i : lane) {                                         // (the groups keep the longest-first order)
                const uint32_t k = key(i);
                if (at[k] == kT1NoBlock) h_tail[n_tail++] = i; else h_lane[at[k]++] = i;
            }
            n_lane = out;
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
            if (t_k8 <= t_mix && c->t1_lanes != 2) n_lane = 0;
        }
        if (n_lane < 64u) { n_lane = 0; n_tail = 0; }                   // not worth a second launch: K8 in table order
    }
    { const int rc = upload_table(c, up, nblocks * sizeof(HtDecBlock) + nblocks * 12); if (rc) return rc; }
    const uint32_t* const d_lane = (const uint32_t*)((const char*)c->dec_table.p + nblocks * sizeof(HtDecBlock));
    T1DecArgs a{};
    a.table = (const HtDecBlock*)c->dec_table.p;
    a.blocks = (const HtBlockDesc*)c->dec_desc.p; a.blocks_per_tile = bpt; a.nblocks = (uint32_t)nblocks; a.ncomp = g.p.num_comps;
    a.coded = (const uint8_t*)d_coded; a.coded_bytes = coded_bytes;
    a.work = (int32_t*)c->dec_work.p; a.status = (unsigned int*)c->flag.p;
    a.mallat = (int32_t*)d_mallat; a.stride = g.stride; a.pitch = g.plane_elems;
    a.irreversible = g.p.irreversible;
    a.cblksty = g.p.reserved[1];
    const std::vector<uint32_t>& seg_first = g.reduce ? c->red_seg_first : c->dec_seg_first;
    const std::vector<grk_amd_segment>& segs = g.reduce ? c->red_segs : c->dec_segs;
    if (!seg_first.empty()) {
        if (seg_first.size() != nblocks + 1 || seg_first.back() != segs.size())
            return fail(c, GRK_AMD_ERR_INVALID, "segment list does not match the number of blocks");
        static_assert(sizeof(grk_amd_segment) == sizeof(uint2), "segments are {bytes, passes}");
        const size_t nf = seg_first.size() * 4, ns = segs.size() * sizeof(grk_amd_segment);
        const size_t ns_off = (nf + 15) & ~(size_t)15;
        HIP_TRY(c, c->dec_seg_dev.ensure(ns_off + ns + 16), "alloc segment list");
        HIP_TRY(c, hipMemcpyAsync(c->dec_seg_dev.p, seg_first.data(), nf, hipMemcpyHostToDevice, c->stream), "upload segment index");
        if (ns) HIP_TRY(c, hipMemcpyAsync((char*)c->dec_seg_dev.p + ns_off, segs.data(), ns, hipMemcpyHostToDevice, c->stream), "upload segments");
        a.seg_first = (const uint32_t*)c->dec_seg_dev.p;
        a.segs = (const uint2*)((const char*)c->dec_seg_dev.p + ns_off);
    }
    ScopedTimer t(c, 5);
    if (n_lane) {
        T1LaneArgs la{};
        la.table = a.table; la.blocks = a.blocks; la.blocks_per_tile = bpt; la.ncomp = a.ncomp;
        la.list = d_lane; la.count = n_lane;
        la.coded = a.coded; la.coded_bytes = coded_bytes;
        la.work = (uint64_t*)c->dec_work.p;
        la.mallat = a.mallat; la.stride = a.stride; la.pitch = a.pitch; la.irreversible = a.irreversible;
        la.pass_sync = c->t1_pass_sync ? 1 : 0;
        a.list = d_lane + 2 * nblocks; a.count = n_tail;
        // one launch, one stream (r06): the long chains are the launch's first workgroups, the lane waves follow; a decode SEQUENCE then
        // needs one hardware queue per frame in flight instead of two
        if (n_tail) {
            HIP_TRY(c, launch_t1_fused(a, la, c->stream), "launch Part-1 decode (both decoders)");
            return GRK_AMD_OK;
        }
        if (c->overlap && c->side) {
            // the long chains on the call's stream, the lanes beside them on the side stream
            if (!c->ev_dec_front) HIP_TRY(c, hipEventCreateWithFlags(&c->ev_dec_front, hipEventDisableTiming), "create event");
            if (!c->ev_dec_top) HIP_TRY(c, hipEventCreateWithFlags(&c->ev_dec_top, hipEventDisableTiming), "create event");
            HIP_TRY(c, hipEventRecord(c->ev_dec_front, c->stream), "record the tables");
            HIP_TRY(c, hipStreamWaitEvent(c->side, c->ev_dec_front, 0), "side stream waits for the tables");
            HIP_TRY(c, launch_t1_decode(a, c->stream), "launch Part-1 decode (long blocks)");
            HIP_TRY(c, launch_t1_lanes(la, c->side), "launch Part-1 decode (lanes)");
            HIP_TRY(c, hipEventRecord(c->ev_dec_top, c->side), "record the lanes");
            HIP_TRY(c, hipStreamWaitEvent(c->stream, c->ev_dec_top, 0), "join the lanes");
        } else {
            HIP_TRY(c, launch_t1_decode(a, c->stream), "launch Part-1 decode (long blocks)");
            HIP_TRY(c, launch_t1_lanes(la, c->stream), "launch Part-1 decode (lanes)");
        }
        return GRK_AMD_OK;
    }
    HIP_TRY(c, launch_t1_decode(a, c->stream), "launch Part-1 decode");
    return GRK_AMD_OK;
}

int check_decode_status(grk_amd_ctx* c)
{
    uint32_t st = 0;
    if (!c->flag.p) return GRK_AMD_OK;                 // nothing was decoded on this context (a sequence's frames are on its children)
    HIP_TRY(c, hipMemcpyAsync(&st, c->flag.p, 4, hipMemcpyDeviceToHost, c->stream), "fetch status");
    HIP_TRY(c, hipStreamSynchronize(c->stream), "sync");
    if (st & 4u) return fail(c, GRK_AMD_ERR_INVALID, "corrupt HT code-block (bad Scup or U_q > missing_msbs)");
    if (st & 16u) return fail(c, GRK_AMD_ERR_INVALID, "Part-1 code-block with more than 24 bit-planes (k_max_bit_planes)");
    if (st & 8u) return fail(c, GRK_AMD_ERR_RANGE, "a coefficient left the 16-bit planes: decode again after grk_amd_set_decode_planes16(ctx, 0)");
    return GRK_AMD_OK;
}

// the context's decode layout for `ntiles` outputs of w x h (0: the tile of the current geometry), or GRK_AMD_ERR_INVALID and the reason
int decode_layout(grk_amd_ctx* c, uint32_t w, uint32_t h, uint32_t ntiles, PixelLayout& px)
{
    const char* why = "";
    if (!resolve_pixel_layout(c->geom.p, &c->dec_layout, w, h, ntiles, px, &why)) return fail(c, GRK_AMD_ERR_INVALID, why);
    if (px.lay && (c->geom.p.prec + 7u) / 8u > 2) return fail(c, GRK_AMD_ERR_UNSUPPORTED, "pixel layout: samples of more than 16 bits leave in the default layout only");
    return GRK_AMD_OK;
}

int run_egress(grk_amd_ctx* c, uint32_t ntiles, const void* d_planes, void* d_pixels, uint32_t out_bytes, const PixelLayout& px)
{
    const TileGeom& g = c->geom;
    EgressArgs a{};
    a.px_lay = px.lay; a.px_chan = px.channels; a.px_xstep = px.xstep; a.px_fill = px.fill; a.px_row = px.row; a.px_kstep = px.kstep; a.px_tile = px.tile;
    a.planes = (const int32_t*)d_planes; a.pixels = d_pixels;
    a.w = g.p.tile_w; a.h = g.p.tile_h; a.stride = g.stride; a.pitch = g.plane_elems;
    a.ncomp = g.p.num_comps; a.ntiles = ntiles;
    a.bytes_per_sample = out_bytes;
    a.dc = g.p.sgnd ? 0 : (1 << (g.p.prec - 1));
    a.lo = g.p.sgnd ? -(1 << (g.p.prec - 1)) : 0;
    a.hi = g.p.sgnd ? (1 << (g.p.prec - 1)) - 1 : (1 << g.p.prec) - 1;
    a.mct = g.p.mct; a.irreversible = g.p.irreversible;
    ScopedTimer t(c, 7);
    HIP_TRY(c, launch_egress(a, c->stream), "launch egress");
    return GRK_AMD_OK;
}
} // namespace

extern "C" {
int grk_amd_stage_dwt_inv(grk_amd_ctx* c, const grk_amd_tile_params* p, uint32_t nplanes, const void* d_mallat, void* d_out)
{
    if (c) { const int jr = join_side(c); if (jr) return jr; }
    if (!c || !p || !d_mallat || !d_out) return GRK_AMD_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device), "set device");
    int rc = ensure_geom(c, p); if (rc) return rc;
    return run_idwt(c, nplanes, d_mallat, d_out);
}

int grk_amd_stage_ht_decode(grk_amd_ctx* c, const grk_amd_tile_params* p, uint32_t ntiles,
                            const grk_amd_coded_block* table, const void* d_coded, uint64_t coded_bytes, void* d_mallat)
{
    if (c) { const int jr = join_side(c); if (jr) return jr; }
    if (!c || !p || !table || !d_coded || !d_mallat || ntiles == 0) return GRK_AMD_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device), "set device");
    int rc = ensure_geom(c, p); if (rc) return rc;
    grk_amd_ctx::DecUpload* up = nullptr;
    rc = stage_table(c, table, (uint64_t)c->geom.blocks_per_comp * c->geom.p.num_comps * ntiles, &up); if (rc) return rc;
    rc = p->reserved[0] ? run_t1_decode(c, ntiles, up, d_coded, coded_bytes, d_mallat)
                        : run_ht_decode(c, ntiles, up, d_coded, coded_bytes, d_mallat);
    if (rc) return rc;
    return check_decode_status(c);
}

// K5b's int16 stores and their range flag as a decode of an 8-bit reversible HT tile runs them (decode_impl's h16 conditions)
int grk_amd_stage_ht_decode16(grk_amd_ctx* c, const grk_amd_tile_params* p, uint32_t ntiles,
                              const grk_amd_coded_block* table, const void* d_coded, uint64_t coded_bytes, void* d_mallat16)
{
    if (c) { const int jr = join_side(c); if (jr) return jr; }
    if (!c || !p || !table || !d_coded || !d_mallat16 || ntiles == 0) return GRK_AMD_ERR_INVALID;
    if (p->irreversible || p->prec > 8 || p->reserved[0] || !c->dec_seg_first.empty())
        return fail(c, GRK_AMD_ERR_INVALID, "int16 planes are for reversible HT tiles of at most 8 bits without refinement passes");
    HIP_TRY(c, hipSetDevice(c->device), "set device");
    int rc = ensure_geom(c, p); if (rc) return rc;
    grk_amd_ctx::DecUpload* up = nullptr;
    rc = stage_table(c, table, (uint64_t)c->geom.blocks_per_comp * c->geom.p.num_comps * ntiles, &up); if (rc) return rc;
    rc = run_ht_decode(c, ntiles, up, d_coded, coded_bytes, d_mallat16, true, false); if (rc) return rc;
    return check_decode_status(c);
}

static int decode_impl(grk_amd_ctx* c, const grk_amd_tile_params* p, uint32_t ntiles,
                       const grk_amd_coded_block* table, const void* coded, uint64_t coded_bytes, int coded_on_device,
                       void* pixels, int pixels_on_device, const Rect* win, bool force32 = false)
{
    if (!c || !p || !table || !coded || !pixels || ntiles == 0) return GRK_AMD_ERR_INVALID;
    const grk_amd_coded_block* table_in = table;
    HIP_TRY(c, hipSetDevice(c->device), "set device");
    int rc = join_side(c); if (rc) return rc;        // (the Mallat planes and the status word are shared with the encoder)
    // (the block decoders of the top resolution run on the side stream beside the rest: the two have to be dispatched side by side)
    if (c->overlap && c->side && c->seq_index < 0 && c->stream_probe && c->probed_main != c->stream && probe_streams(c) != GRK_AMD_OK) {
        c->stream_probe = 0; (void)hipGetLastError();
    }
    rc = ensure_geom(c, p, c->dec_reduce); if (rc) return rc;
    const TileGeom& g = c->geom;
    const uint32_t nplanes = ntiles * g.p.num_comps;
    if (g.reduce && !c->dec_seg_first.empty()) {
        // the segment list is over the full tile's blocks: the kept blocks' segments, in the order of the kept rows
        const uint64_t groups = (uint64_t)ntiles * g.p.num_comps;
        if (c->dec_seg_first.size() != groups * g.full_blocks_per_comp + 1 || c->dec_seg_first.back() != c->dec_segs.size())
            return fail(c, GRK_AMD_ERR_INVALID, "segment list does not match the number of blocks");
        c->red_seg_first.clear(); c->red_segs.clear();
        for (uint64_t k = 0; k < groups; ++k)
            for (uint64_t i = k * g.full_blocks_per_comp, e = i + g.blocks_per_comp; i < e; ++i) {
                c->red_seg_first.push_back((uint32_t)c->red_segs.size());
                c->red_segs.insert(c->red_segs.end(), c->dec_segs.begin() + c->dec_seg_first[i], c->dec_segs.begin() + c->dec_seg_first[i + 1]);
            }
        c->red_seg_first.push_back((uint32_t)c->red_segs.size());
    } else {
        c->red_seg_first.clear(); c->red_segs.clear();
    }
    const uint32_t bps = (g.p.prec + 7u) / 8u;
    const bool fuse_out = g.p.num_levels >= 1 && bps <= 2 && c->fuse_egress;
    // region decode: the blocks no sample of the window depends on are not decoded, the synthesis covers what is needed
    RegionPlan plan;
    grk_amd_ctx::DecUpload* up = nullptr;
    rc = stage_table(c, table, (uint64_t)g.blocks_per_comp * g.p.num_comps * ntiles, &up); if (rc) return rc;
    if (win) {
        if (ntiles != 1 || win->x0 >= win->x1 || win->y0 >= win->y1 || win->x1 > g.p.tile_w || win->y1 > g.p.tile_h)
            return fail(c, GRK_AMD_ERR_INVALID, "window outside the tile");
        if (!fuse_out) return fail(c, GRK_AMD_ERR_UNSUPPORTED, "region decode needs at least one DWT level and 8-/16-bit pixels");
        plan = plan_region(g, *win);
        const uint32_t L = g.p.num_levels;
        grk_amd_coded_block* const wtable = (grk_amd_coded_block*)up->p;
        size_t i = 0;
        auto sat = [](uint32_t a, uint32_t b) { return a > b ? a - b : 0u; };
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
                    wtable[i].offset = 0; wtable[i].length = 0; wtable[i].missing_msbs = kSkipBlock;
                }
                ++i;
            }
    }
    // the pixels' layout (grk_amd_set_decode_pixel_layout) for what this call writes: the window, the reduced tile, the tile
    PixelLayout px;
    rc = decode_layout(c, win ? win->x1 - win->x0 : 0, win ? win->y1 - win->y0 : 0, ntiles, px); if (rc) return rc;
    const void* d_coded = coded;
    if (!coded_on_device) {
        HIP_TRY(c, c->dec_coded.ensure(coded_bytes + 64), "alloc coded staging");
        rc = copy_h2d(c, c->dec_coded.p, coded, coded_bytes); if (rc) return rc;
        d_coded = c->dec_coded.p;
    }
    const size_t px_bytes = px.bytes;     // (the default layout: the tight window / tiles)
    void* d_px = pixels;
    if (!pixels_on_device) {
        HIP_TRY(c, c->dec_pixels.ensure(px_bytes), "alloc pixel staging");
        d_px = c->dec_pixels.p;
        // the extent comes back as one copy, gaps included -- and what the caller has in the gaps is to stay: it goes up first
        if (px.lay) { rc = copy_h2d(c, d_px, pixels, px_bytes); if (rc) return rc; }
    }
    if (!fuse_out) HIP_TRY(c, c->p0.ensure((size_t)nplanes * g.plane_elems * 4 + 256), "alloc planes");
    HIP_TRY(c, c->p1.ensure((size_t)nplanes * g.plane_elems * 4 + 256), "alloc Mallat planes");
    // 8-bit reversible HT tiles: int16 planes between K5b and K6 (both HBM-side halves of the decode move half the bytes).
    // Every coefficient and every synthesised LL sample of a stream that an 8-bit image produced fits (the encoder's
    // planes16_ok bound); a stream whose values do not is reported by decode_status (GRK_AMD_ERR_RANGE), and a synchronous
    // call decodes it again with int32 planes right here -- never other pixels.
    const bool h16 = c->dec_planes16 && !force32 && fuse_out && !p->reserved[0] && !g.p.irreversible && g.p.prec <= 8 &&
                     c->dec_seg_first.empty();
    {
        ScopedTimer t(c, 3);
        rc = p->reserved[0] ? run_t1_decode(c, ntiles, up, d_coded, coded_bytes, c->p1.p)
                            : run_ht_decode(c, ntiles, up, d_coded, coded_bytes, c->p1.p, h16, true);
        if (rc) return rc;
        // with at least one DWT level and 8-/16-bit pixels the last level writes the pixels itself (K7 fused): the
        // int32 image planes (4 bytes per sample written and read back) never exist
        if (fuse_out) {
            rc = run_idwt(c, nplanes, c->p1.p, nullptr, d_px, ntiles, bps, win ? &plan : nullptr, h16, &px); if (rc) return rc;
        } else {
            rc = run_idwt(c, nplanes, c->p1.p, c->p0.p); if (rc) return rc;
            rc = run_egress(c, ntiles, c->p0.p, d_px, bps, px); if (rc) return rc;
        }
    }
    if (!pixels_on_device) {
        rc = copy_d2h(c, pixels, d_px, px_bytes); if (rc) return rc;
        rc = check_decode_status(c);
        if (rc == GRK_AMD_ERR_RANGE && h16)           // (synchronous call: the exact path, at once)
            return decode_impl(c, p, ntiles, table_in, coded, coded_bytes, coded_on_device, pixels, pixels_on_device, win, true);
        return rc;
    }
    return GRK_AMD_OK;                 // (a window's adapted table lives in the context's pinned memory: nothing to wait for)
}

int grk_amd_decode_tiles(grk_amd_ctx* c, const grk_amd_tile_params* p, uint32_t ntiles,
                         const grk_amd_coded_block* table, const void* coded, uint64_t coded_bytes, int coded_on_device,
                         void* pixels, int pixels_on_device)
{
    if (c && !c->dec_kids.empty() && coded_on_device && pixels_on_device) {
        {
            // (every frame of the sequence on one of the internal contexts, none on this one: the event below must stand for what the
            //  CALLER queued on this context's stream, not for an earlier frame of the sequence)
            grk_amd_ctx* k = c->dec_kids[c->dec_seq++ % (uint32_t)c->dec_kids.size()];
            // what the caller set on the context applies to the frame wherever it is decoded
            if (k->dec_qcd != c->dec_qcd || k->dec_steps != c->dec_steps) { k->dec_qcd = c->dec_qcd; k->dec_steps = c->dec_steps; k->have_geom = false; }
            if (k->dec_seg_first != c->dec_seg_first) k->dec_seg_first = c->dec_seg_first;
            k->dec_reduce = c->dec_reduce; k->dec_layout = c->dec_layout;
            if (k->dec_segs.size() != c->dec_segs.size() ||
                (!c->dec_segs.empty() && std::memcmp(k->dec_segs.data(), c->dec_segs.data(), c->dec_segs.size() * sizeof(c->dec_segs[0])) != 0))
                k->dec_segs = c->dec_segs;
            k->dec_planes16 = c->dec_planes16; k->fuse_egress = c->fuse_egress; k->dwt_pk = c->dwt_pk; k->dwt_xcd = c->dwt_xcd;
            k->overlap = c->overlap && k->side != nullptr; k->t1_lanes = c->t1_lanes;
            HIP_TRY(c, hipSetDevice(c->device), "set device");
            { const int sr = sequence_streams(k, p && p->reserved[0] != 0); if (sr) { c->err = k->err; return sr; } }
            // The contexts' streams, vetted in the contexts' order: a context's two streams against each other and against the (up to
            // three) streams accepted just before -- four dispatch pipes: two frames in flight can have a pipe per stream (HT frames:
            // 0.66 instead of 0.75-0.81 ms per frame when the runtime's choice collides, tools/hwq_alias_dec.py), more cannot
            if (c->stream_probe && !k->seq_vetted) {
                int vr = grk_amd_synchronize(k);
                const int nk = (int)c->dec_kids.size();
                for (int which = 0; which < 2 && vr == GRK_AMD_OK; ++which) {
                    hipStream_t* st = which ? &k->side : &k->stream;
                    if (!*st) continue;
                    // (the streams as they are NOW: a context that changed its kind of frames has re-made its own)
                    std::vector<hipStream_t> against;
                    if (which) against.push_back(k->stream);
                    for (int back = 1; back < nk && against.size() < 3; ++back) {
                        grk_amd_ctx* o = c->dec_kids[(size_t)((k->seq_index - back + nk) % nk)];
                        if (!o->seq_vetted) continue;
                        if (o->side && against.size() < 3) against.push_back(o->side);
                        if (against.size() < 3) against.push_back(o->stream);
                    }
                    vr = vetted_stream(k, st, against, &c->probe_replaced);
                }
                if (vr) { c->stream_probe = 0; (void)hipGetLastError(); }
                k->seq_vetted = true;
            }
            // ... behind whatever the caller queued on this context's stream (its uploads of the coded bytes)
            HIP_TRY(c, hipEventRecord(c->ev_seq, c->stream), "record the caller's stream");
            HIP_TRY(c, hipStreamWaitEvent(k->stream, c->ev_seq, 0), "order the frame behind the caller's stream");
            const int rc = decode_impl(k, p, ntiles, table, coded, coded_bytes, 1, pixels, 1, nullptr);
            // (the frame's last kernels -- the final inverse level, behind its join with the side stream -- are on k's stream; a call
            //  that failed half-way may have queued kernels that still read the coded bytes or write the pixels: the set's event covers
            //  those too, its side stream joined first)
            if (!k->ev_frame_done) HIP_TRY(c, hipEventCreateWithFlags(&k->ev_frame_done, hipEventDisableTiming), "create event");
            if (rc && k->side) {
                if (!k->ev_dec_top) HIP_TRY(c, hipEventCreateWithFlags(&k->ev_dec_top, hipEventDisableTiming), "create event");
                HIP_TRY(c, hipEventRecord(k->ev_dec_top, k->side), "record the side stream");
                HIP_TRY(c, hipStreamWaitEvent(k->stream, k->ev_dec_top, 0), "join the side stream");
                k->dec_top_pending = false;
            }
            HIP_TRY(c, hipEventRecord(k->ev_frame_done, k->stream), "record the frame's end");
            if (rc) c->err = k->err;
            return rc;
        }
    }
    return decode_impl(c, p, ntiles, table, coded, coded_bytes, coded_on_device, pixels, pixels_on_device, nullptr);
}

int grk_amd_decode_stream_wait_slot(grk_amd_ctx* c, void* hip_stream)
{
    if (!c || !hip_stream) return GRK_AMD_ERR_INVALID;
    if (c->dec_kids.empty()) return grk_amd_stream_wait_results(c, hip_stream);       // no sequence: the context's own streams
    grk_amd_ctx* k = c->dec_kids[c->dec_seq % (uint32_t)c->dec_kids.size()];          // the set the NEXT call uses
    if (k->ev_frame_done) HIP_TRY(c, hipStreamWaitEvent((hipStream_t)hip_stream, k->ev_frame_done, 0), "wait for the set's last frame");
    return GRK_AMD_OK;
}

int grk_amd_set_decode_pipelining(grk_amd_ctx* c, int frames_in_flight)
{
    if (!c || frames_in_flight < 0 || frames_in_flight > 8) return GRK_AMD_ERR_INVALID;
    int rc = grk_amd_synchronize(c);
    for (grk_amd_ctx* k : c->dec_kids) grk_amd_destroy(k);
    c->dec_kids.clear();
    c->dec_seq = 0;
    if (rc) return rc;
    if (frames_in_flight >= 2 && !c->ev_seq) HIP_TRY(c, hipEventCreateWithFlags(&c->ev_seq, hipEventDisableTiming), "create event");
    for (int i = 0; i < frames_in_flight && frames_in_flight >= 2; ++i) {
        grk_amd_ctx* k = nullptr;
        rc = create_context(c->device, c->verbose, true, &k);
        if (rc) return fail(c, rc, "a further decode context could not be made");
        k->seq_index = i;
        c->dec_kids.push_back(k);
    }
    return GRK_AMD_OK;
}

int grk_amd_decode_region(grk_amd_ctx* c, const grk_amd_tile_params* p,
                          const grk_amd_coded_block* table, const void* coded, uint64_t coded_bytes, int coded_on_device,
                          uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, void* pixels, int pixels_on_device)
{
    const Rect win{x0, y0, x1, y1};
    return decode_impl(c, p, 1, table, coded, coded_bytes, coded_on_device, pixels, pixels_on_device, &win);
}

int grk_amd_set_decode_qcd(grk_amd_ctx* c, const uint16_t* words, uint32_t count)
{
    if (!c || (count && !words)) return GRK_AMD_ERR_INVALID;
    c->dec_qcd.assign(words, words + count);
    c->have_geom = false;                  // the per-block dequantisation scales are rebuilt on the next call
    return GRK_AMD_OK;
}

int grk_amd_set_decode_steps(grk_amd_ctx* c, const float* steps, uint32_t count)
{
    if (!c || (count && !steps)) return GRK_AMD_ERR_INVALID;
    c->dec_steps.assign(steps, steps + count);
    c->have_geom = false;                  // the per-block dequantisation scales are rebuilt on the next call
    return GRK_AMD_OK;
}

int grk_amd_set_decode_reduce(grk_amd_ctx* c, uint32_t reduce)
{
    if (!c) return GRK_AMD_ERR_INVALID;
    c->dec_reduce = reduce;                // checked against each call's number of levels (decode_impl -> ensure_geom)
    return GRK_AMD_OK;
}

int grk_amd_reduced_tile_rect(const grk_amd_tile_params* p, uint32_t reduce, uint32_t* x0, uint32_t* y0, uint32_t* w, uint32_t* h)
{
    if (!p || !x0 || !y0 || !w || !h) return GRK_AMD_ERR_INVALID;
    return reduced_tile_rect(*p, reduce, x0, y0, w, h);
}

int grk_amd_set_decode_segments(grk_amd_ctx* c, const uint32_t* first_segment, const grk_amd_segment* segments, uint32_t nblocks)
{
    if (!c || (nblocks && (!first_segment || (first_segment[nblocks] && !segments)))) return GRK_AMD_ERR_INVALID;
    c->dec_seg_first.clear(); c->dec_segs.clear();
    if (nblocks) {
        c->dec_seg_first.assign(first_segment, first_segment + nblocks + 1);
        c->dec_segs.assign(segments, segments + first_segment[nblocks]);
    }
    return GRK_AMD_OK;
}

int grk_amd_decode_status(grk_amd_ctx* c)
{
    if (!c) return GRK_AMD_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device), "set device");
    int rc = check_decode_status(c);
    for (grk_amd_ctx* k : c->dec_kids) {            // (a sequence: the frames decoded on the other contexts as well)
        const int kr = check_decode_status(k);
        if (kr && !rc) { rc = kr; c->err = k->err; }
    }
    return rc;
}

int grk_amd_stage_egress(grk_amd_ctx* c, const grk_amd_tile_params* p, uint32_t ntiles, const void* d_planes, void* d_pixels)
{
    if (!c || !p || !d_planes || !d_pixels) return GRK_AMD_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device), "set device");
    int rc = ensure_geom(c, p); if (rc) return rc;
    if (!ntiles) return GRK_AMD_ERR_INVALID;
    PixelLayout px;
    rc = decode_layout(c, 0, 0, ntiles, px); if (rc) return rc;
    return run_egress(c, ntiles, d_planes, d_pixels, (p->prec + 7u) / 8u, px);
}

int grk_amd_set_decode_planes16(grk_amd_ctx* c, int on)
{
    if (!c) return GRK_AMD_ERR_INVALID;
    c->dec_planes16 = on != 0;
    return GRK_AMD_OK;
}
} // extern "C"
