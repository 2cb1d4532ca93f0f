// grok_amd/csrc/context.hip -- the context: create / destroy, errors, host staging, the geometry cache, layout queries, timing.
#include "context.h"

namespace {
bool create_alt_events(grk_amd_ctx* c)
{
    for (auto& as : c->alts)
        if (hipEventCreateWithFlags(&as.ev_side, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&as.ev_side2, hipEventDisableTiming) != hipSuccess) return false;
    return true;
}

#ifndef GRK_AMD_OVERLAP_DEFAULT
#define GRK_AMD_OVERLAP_DEFAULT 1
#endif

void drain_timers(grk_amd_ctx* c)
{
    for (auto& t : c->timers) {
        for (auto& pr : t.ev) {
            float ms = 0;
            if (hipEventSynchronize(pr.second) == hipSuccess && hipEventElapsedTime(&ms, pr.first, pr.second) == hipSuccess) {
                t.total_ms += ms; t.launches++;
            }
            (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second);
        }
        t.ev.clear();
    }
}
} // namespace

int fail(grk_amd_ctx* c, int code, const char* what, hipError_t e)
{
    if (c) {
        c->err = what;
        if (e != hipSuccess) { c->err += ": "; c->err += hipGetErrorString(e); }
        if (c->verbose) fprintf(stderr, "[grok_amd] %s\n", c->err.c_str());
    }
    return code;
}

bool host_is_pinned(const void* p)
{
    hipPointerAttribute_t a{};
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }   // (plain malloc'ed memory: "invalid value")
    return a.type == hipMemoryTypeHost;
}

// Host -> device, ordered after what the context's stream holds so far; on return the source may be reused (pageable) or the
// copy is queued on the stream (pinned).  Device -> host likewise; the caller synchronises the stream before reading pinned
// memory, pageable memory is complete on return.
int copy_h2d(grk_amd_ctx* c, void* dst, const void* src, size_t bytes)
{
    if (bytes < 2 * HostStage::kChunk || host_is_pinned(src)) {
        HIP_TRY(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream), "upload");
        return GRK_AMD_OK;
    }
    HostStage& hs = c->stage;
    HIP_TRY(c, hs.ensure(), "alloc pinned staging");
    HIP_TRY(c, hipEventRecord(hs.ev_in, c->stream), "record");
    const size_t nchunks = (bytes + HostStage::kChunk - 1) / HostStage::kChunk;
    hipError_t errs[HostStage::kLanes] = {};
    std::thread th[HostStage::kLanes];
    for (int t = 0; t < HostStage::kLanes; ++t)
        th[t] = std::thread([&, t]() {
            hipError_t e = hipSetDevice(c->device);
            if (e == hipSuccess) e = hipStreamWaitEvent(hs.st[t], hs.ev_in, 0);
            int k = 0;
            for (size_t i = (size_t)t; i < nchunks && e == hipSuccess; i += HostStage::kLanes, k ^= 1) {
                const size_t off = i * HostStage::kChunk, n = std::min(HostStage::kChunk, bytes - off);
                e = hipEventSynchronize(hs.ev[t][k]);                  // the DMA that last read this chunk (never recorded: returns at once)
                if (e != hipSuccess) break;
                std::memcpy(hs.buf[t][k], (const char*)src + off, n);
                e = hipMemcpyAsync((char*)dst + off, hs.buf[t][k], n, hipMemcpyHostToDevice, hs.st[t]);
                if (e == hipSuccess) e = hipEventRecord(hs.ev[t][k], hs.st[t]);
            }
            if (e == hipSuccess) e = hipEventRecord(hs.ev_out[t], hs.st[t]);
            errs[t] = e;
        });
    for (auto& x : th) x.join();
    for (int t = 0; t < HostStage::kLanes; ++t) {
        HIP_TRY(c, errs[t], "staged upload");
        HIP_TRY(c, hipStreamWaitEvent(c->stream, hs.ev_out[t], 0), "join the copy streams");
    }
    return GRK_AMD_OK;
}

// Device -> pageable host memory: ONE DMA stream (the context's) brings the bytes into a pinned staging area of the transfer's size,
// piece by piece with an event behind each, while a few host threads copy the pieces that have arrived to where they belong -- the link
// runs near its rate (99 MB in 2.17 ms; four lanes with a DMA and a memcpy each in turn: 2.42; into pinned memory 1.78).
int copy_d2h(grk_amd_ctx* c, void* dst, const void* src, size_t bytes)
{
    if (bytes < 2 * HostStage::kChunk || host_is_pinned(dst)) {
        HIP_TRY(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream), "download");
        return GRK_AMD_OK;
    }
    // (measured on 99 MB, ms: pieces of 4 / 8 / 16 / 32 MB with four threads 2.37 / 2.17 / 2.25 / 2.45, eight threads 2.5 / 2.3 / 2.3 / 2.5 --
    //  a DMA of a few MB costs its set-up, a thread its creation; pinned memory: 1.78)
    constexpr size_t kPiece = 8u << 20;
    if (c->d2h_cap < bytes) {
        if (c->d2h_pin) { (void)hipHostFree(c->d2h_pin); c->d2h_pin = nullptr; c->d2h_cap = 0; }
        const size_t want = bytes + (bytes >> 3);
        HIP_TRY(c, hipHostMalloc(&c->d2h_pin, want, hipHostMallocDefault), "alloc pinned staging");
        c->d2h_cap = want;
    }
    struct Piece { size_t off, n; };
    std::vector<Piece> pieces;
    for (size_t off = 0; off < bytes; off += kPiece) pieces.push_back(Piece{off, std::min(kPiece, bytes - off)});
    while (c->d2h_ev.size() < pieces.size()) {
        hipEvent_t ev = nullptr;
        HIP_TRY(c, hipEventCreateWithFlags(&ev, hipEventDisableTiming), "create event");
        c->d2h_ev.push_back(ev);
    }
    std::atomic<size_t> issued{0};
    std::atomic<int> failed{0};
    constexpr int nthr = 4;                       // every thread copies its quarter of every piece: what is left behind the last DMA is 2 MB each
    std::thread th[nthr];
    for (int t = 0; t < nthr; ++t)
        th[t] = std::thread([&, t]() {
            (void)hipSetDevice(c->device);
            for (size_t i = 0; i < pieces.size(); ++i) {
                while (issued.load(std::memory_order_acquire) <= i) { if (failed.load()) return; std::this_thread::yield(); }   // (its event has been recorded)
                if (hipEventSynchronize(c->d2h_ev[i]) != hipSuccess) { failed.store(1); return; }
                const size_t a0 = pieces[i].n * (size_t)t / nthr, a1 = pieces[i].n * (size_t)(t + 1) / nthr;
                std::memcpy((char*)dst + pieces[i].off + a0, (const char*)c->d2h_pin + pieces[i].off + a0, a1 - a0);
            }
        });
    hipError_t e = hipSuccess;
    for (size_t i = 0; i < pieces.size() && e == hipSuccess; ++i) {
        e = hipMemcpyAsync((char*)c->d2h_pin + pieces[i].off, (const char*)src + pieces[i].off, pieces[i].n, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipEventRecord(c->d2h_ev[i], c->stream);
        if (e == hipSuccess) issued.store(i + 1, std::memory_order_release);
    }
    if (e != hipSuccess) failed.store(1);
    for (int t = 0; t < nthr; ++t) th[t].join();
    HIP_TRY(c, e, "staged download");
    if (failed.load()) return fail(c, GRK_AMD_ERR_NO_DEVICE, "staged download");
    return GRK_AMD_OK;
}

bool same_params(const grk_amd_tile_params& a, const grk_amd_tile_params& b)
{
    return a.tile_w == b.tile_w && a.tile_h == b.tile_h && a.num_comps == b.num_comps && a.prec == b.prec &&
           a.sgnd == b.sgnd && a.irreversible == b.irreversible && a.mct == b.mct &&
           a.num_levels == b.num_levels && a.cblk_w_exp == b.cblk_w_exp && a.cblk_h_exp == b.cblk_h_exp &&
           a.reserved[0] == b.reserved[0] && a.reserved[1] == b.reserved[1] && a.tile_x0 == b.tile_x0 && a.tile_y0 == b.tile_y0 &&
           std::memcmp(a.precinct_exp, b.precinct_exp, sizeof a.precinct_exp) == 0;
}

int ensure_geom(grk_amd_ctx* c, const grk_amd_tile_params* p, uint32_t reduce)
{
    if (c->have_geom && same_params(c->gp, *p) && c->geom.reduce == reduce) return GRK_AMD_OK;
    if (reduce > p->num_levels) return fail(c, GRK_AMD_ERR_INVALID, "decode reduce above the tile's number of DWT levels");
    // the tables rebuilt below may still be read by K3 launches of a pipelined predecessor on the side streams
    if (c->side) HIP_TRY(c, hipStreamSynchronize(c->side), "sync side stream");
    if (c->side2) HIP_TRY(c, hipStreamSynchronize(c->side2), "sync side stream 2");
    HIP_TRY(c, hipStreamSynchronize(c->stream), "sync");
    c->side_pending = false;
    c->have_geom = false;                      // valid again only once every table below is on the device
    int rc = build_tile_geom(*p, c->geom);
    if (rc != GRK_AMD_OK) return fail(c, rc, "unsupported tile parameters");
    if (reduce) {
        TileGeom full = std::move(c->geom);
        rc = reduce_tile_geom(full, reduce, c->geom);
        if (rc != GRK_AMD_OK) return fail(c, rc, "reduced geometry");
    }
    c->gp = *p;
    const TileGeom& g = c->geom;
    c->h_desc.clear();
    for (uint32_t k = 0; k < p->num_comps; ++k)
        for (const auto& b : g.blocks_comp0) {
            HtBlockDesc d;
            d.px = b.px; d.py = b.py;
            d.w = (uint16_t)(b.x1 - b.x0); d.h = (uint16_t)(b.y1 - b.y0);
            d.comp = (uint16_t)k; d.kmax = b.kmax; d.pad = b.band;
            d.inv_step = 1.0f / b.stepsize;
            c->h_desc.push_back(d);
        }
    // K3's block classes (encode_plan.h): the lists of all classes on the device, one behind the other
    {
        HtClasses plan = plan_ht_classes(g, p->num_comps, c->lds_cap);
        HIP_TRY(c, c->ht_sel.ensure(plan.sel.size() * 4 + 16), "alloc class index");
        HIP_TRY(c, hipMemcpyAsync(c->ht_sel.p, plan.sel.data(), plan.sel.size() * 4, hipMemcpyHostToDevice, c->stream), "upload class index");
        HIP_TRY(c, hipStreamSynchronize(c->stream), "sync class index");
        c->ht_classes = std::move(plan.classes);
    }
    // decode-side descriptors: inv_step carries the dequantisation scale of the band
    // (codestream/Quantizer.cpp:41-63 with compress = false: log2_gain 0, then / 2^(31 - numbps))
    c->h_desc_dec = c->h_desc;
    {
        size_t i = 0;
        for (uint32_t k = 0; k < p->num_comps; ++k)
            for (const auto& b : g.blocks_comp0) {
                float scale = 1.0f;
                const uint32_t bi = b.res == 0 ? 0u : 3u * b.res - 2u + (b.band - 1u);
                // (both lists are over the full tile's bands, also for a reduced decode: its bands are their first ones)
                if (p->irreversible && c->dec_steps.size() == (size_t)p->num_comps * g.full_bands_total) {
                    scale = c->dec_steps[(size_t)k * g.full_bands_total + bi];     // the host's TileBand::stepsize, fix-ups included
                } else if (p->irreversible) {
                    const uint16_t wq = (c->dec_qcd.size() == g.full_bands_total) ? c->dec_qcd[bi] : g.qcd_words[bi];
                    const double step = (1.0 + (wq & 0x7FF) / 2048.0) * std::pow(2.0, (int)p->prec - (int)(wq >> 11));
                    scale = (float)step;
                    if (!p->reserved[0]) scale /= (float)(1u << (31 - b.kmax));     // HT only (Quantizer.cpp:54-63)
                }
                c->h_desc_dec[i++].inv_step = scale;
            }
    }
    HIP_TRY(c, c->dec_desc.ensure(c->h_desc_dec.size() * sizeof(HtBlockDesc)), "alloc decode block table");
    HIP_TRY(c, hipMemcpyAsync(c->dec_desc.p, c->h_desc_dec.data(), c->h_desc_dec.size() * sizeof(HtBlockDesc),
                              hipMemcpyHostToDevice, c->stream), "upload decode block table");
    HIP_TRY(c, c->blockdesc.ensure(c->h_desc.size() * sizeof(HtBlockDesc)), "alloc block table");
    HIP_TRY(c, hipMemcpyAsync(c->blockdesc.p, c->h_desc.data(), c->h_desc.size() * sizeof(HtBlockDesc),
                              hipMemcpyHostToDevice, c->stream), "upload block table");
    HIP_TRY(c, hipStreamSynchronize(c->stream), "sync block table");
    c->have_geom = true;
    return GRK_AMD_OK;
}

int stage_enter(grk_amd_ctx* c, const grk_amd_tile_params* p, bool args_ok, bool join, const char* refuse)
{
    if (c && join) { const int jr = join_side(c); if (jr) return jr; }
    if (!c || !p || !args_ok) return GRK_AMD_ERR_INVALID;
    if (refuse) return fail(c, GRK_AMD_ERR_INVALID, refuse);
    HIP_TRY(c, hipSetDevice(c->device), "set device");
    return ensure_geom(c, p);
}

// decode_only: one of a decode sequence's internal contexts (grk_amd_set_decode_pipelining) -- the call's stream and ONE side
// stream, nothing else: the HIP runtime deals its (default 4) hardware queues to streams in the order they are made, and two
// frames in flight then sit on four queues of their own whatever else the process has made before (a third stream per context
// that decoding never uses made frame 2's lane kernel share a queue with frame 1's long chains: 14.8 instead of 9.1 ms per frame)
int create_context(int device_id, int verbose, bool decode_only, grk_amd_ctx** out)
{
    if (!out) return GRK_AMD_ERR_INVALID;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return GRK_AMD_ERR_NO_DEVICE;
    if (device_id < 0 || device_id >= n) return GRK_AMD_ERR_INVALID;
    if (hipSetDevice(device_id) != hipSuccess) return GRK_AMD_ERR_NO_DEVICE;
    auto* c = new grk_amd_ctx();
    c->device = device_id; c->verbose = verbose;
    { int cus = 0; if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device_id) == hipSuccess && cus > 0) c->num_cus = (uint32_t)cus; }
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { delete c; return GRK_AMD_ERR_NO_DEVICE; }
    c->own_stream = true;
    {   // side stream for K3 of the top resolution (lowest priority: the DWT chain on the main stream is the critical path)
        int least = 0, greatest = 0;
        (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
        if (const char* e16 = getenv("GRK_AMD_PLANES16")) c->planes16 = atoi(e16) != 0;
        if (const char* ef = getenv("GRK_AMD_FUSE_EGRESS")) c->fuse_egress = atoi(ef) != 0;
        if (const char* ex = getenv("GRK_AMD_DWT_XCD")) c->dwt_xcd = atoi(ex) != 0;
        if (const char* ex = getenv("GRK_AMD_DWT_PK")) c->dwt_pk = atoi(ex) != 0;
        if (const char* ex = getenv("GRK_AMD_DWT_PAIR")) c->dwt_pair = atoi(ex) != 0;
        if (const char* ek = getenv("GRK_AMD_K3_ALT")) c->k3_alternate = atoi(ek) != 0;
        if (const char* ed = getenv("GRK_AMD_DEC_PLANES16")) c->dec_planes16 = atoi(ed) != 0;
        if (const char* el = getenv("GRK_AMD_LDS_CAP")) c->lds_cap = atoi(el) != 0;
        if (const char* ef2 = getenv("GRK_AMD_FRAME_STREAMS")) c->frame_streams = atoi(ef2);
        if (const char* et = getenv("GRK_AMD_T1_LANES")) c->t1_lanes = atoi(et);
        if (const char* ey = getenv("GRK_AMD_T1_SYNC")) c->t1_pass_sync = atoi(ey) != 0;
        if (const char* ep = getenv("GRK_AMD_STREAM_PROBE")) c->stream_probe = atoi(ep);
        c->side_priority = least;
        const char* e = getenv("GRK_AMD_OVERLAP");
        c->overlap = e ? atoi(e) != 0 : GRK_AMD_OVERLAP_DEFAULT;
        if (hipStreamCreateWithPriority(&c->side, hipStreamNonBlocking, least) != hipSuccess ||
            (!decode_only && hipStreamCreateWithPriority(&c->side2, hipStreamNonBlocking, least) != hipSuccess) ||
            hipEventCreateWithFlags(&c->ev_side2, hipEventDisableTiming) != hipSuccess ||
            !create_alt_events(c) ||
            hipEventCreateWithFlags(&c->ev_level0, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&c->ev_side, hipEventDisableTiming) != hipSuccess) {
            c->side = nullptr; c->overlap = false;
        }
    }
    *out = c;
    return GRK_AMD_OK;
}

extern "C" {
const char* grk_amd_version(void) { return "grok_amd 0.1 (gfx950)"; }

int grk_amd_create(int device_id, int verbose, grk_amd_ctx** out) { return create_context(device_id, verbose, false, out); }

void grk_amd_destroy(grk_amd_ctx* c)
{
    if (!c) return;
    for (grk_amd_ctx* k : c->dec_kids) grk_amd_destroy(k);
    c->dec_kids.clear();
    (void)hipSetDevice(c->device);
    if (c->ev_seq) (void)hipEventDestroy(c->ev_seq);
    if (c->ev_frame_done) (void)hipEventDestroy(c->ev_frame_done);
    (void)hipStreamSynchronize(c->stream);
    drain_timers(c);
    for (DevBuf* b : {&c->pixels, &c->p0, &c->p1, &c->llA, &c->llB, &c->blockdesc, &c->lengths,
                      &c->offsets, &c->arena, &c->flag, &c->dec_desc, &c->dec_table, &c->dec_quads, &c->dec_mslen,
                      &c->dec_coded, &c->dec_pixels, &c->dec_work, &c->ht_sel, &c->energy, &c->rate_L, &c->rate_E, &c->rate_W,
                      &c->rate_drop, &c->rate_res, &c->rate_map, &c->rate_bdrop, &c->drops_keep})
        b->release();
    if (c->own_stream) (void)hipStreamDestroy(c->stream);
    if (c->side) { (void)hipStreamSynchronize(c->side); (void)hipStreamDestroy(c->side); }
    if (c->side2) { (void)hipStreamSynchronize(c->side2); (void)hipStreamDestroy(c->side2); }
    if (c->ev_side2) (void)hipEventDestroy(c->ev_side2);
    if (c->ev_main) (void)hipEventDestroy(c->ev_main);
    if (c->ev_px) (void)hipEventDestroy(c->ev_px);
    for (auto& alt_set : c->alts) {
        auto* as = &alt_set;
        if (as->ev_side) (void)hipEventDestroy(as->ev_side);
        if (as->ev_side2) (void)hipEventDestroy(as->ev_side2);
        for (DevBuf* b : {&as->p1, &as->arena, &as->lengths, &as->offsets, &as->flag, &as->ovf, &as->llA, &as->llB}) b->release();
    }
    c->ovf.release();
    for (DevBuf* b : {&c->t2.packets, &c->t2.pob, &c->t2_u, &c->t2_h, &c->t2_rel, &c->t2_pkhdr, &c->t2_pkbody, &c->t2_pkdst, &c->t2_lit,
                      &c->t2_litlen, &c->t2_index, &c->t2_nodes, &c->t2_parts})
        b->release();
    for (auto& o : c->t2_outs) for (DevBuf* b : {&o.out, &o.tile_dst, &o.part_len, &o.total, &o.tp_len, &o.tp_dst}) b->release();
    for (auto& k : c->t2j.classes) { k.packets.release(); k.pob.release(); }
    for (DevBuf* b : {&c->jt_len, &c->jt_off, &c->jt_arena, &c->jt_state, &c->jt_rowat, &c->jt_file, &c->jt_msbs}) b->release();
    for (DevBuf* b : {&c->st_len, &c->st_off, &c->st_arena, &c->st_status, &c->st_msbs}) b->release();
    for (DevBuf* b : {&c->st_rL, &c->st_rE, &c->st_rW, &c->st_rdrop, &c->st_rres, &c->st_rmap}) b->release();
    if (c->ev_level0) (void)hipEventDestroy(c->ev_level0);
    if (c->ev_side) (void)hipEventDestroy(c->ev_side);
    for (DevBuf* b : {&c->dec_seg_dev, &c->img_coded, &c->img_tiles, &c->img_pixels, &c->img_moves, &c->img_rects, &c->img_status, &c->img_planes}) b->release();
    read_device_release(c);
    c->stage.release();
    if (c->d2h_pin) (void)hipHostFree(c->d2h_pin);
    for (hipEvent_t ev : c->d2h_ev) (void)hipEventDestroy(ev);
    if (c->ev_dec_front) (void)hipEventDestroy(c->ev_dec_front);
    if (c->ev_dec_top) (void)hipEventDestroy(c->ev_dec_top);
    for (auto& u : c->dec_up) {
        if (u.p) (void)hipHostFree(u.p);
        if (u.ev) (void)hipEventDestroy(u.ev);
    }
    delete c;
}

int grk_amd_set_pixel_layout(grk_amd_ctx* c, const grk_amd_pixel_layout* l)
{
    if (!c) return GRK_AMD_ERR_INVALID;
    c->enc_layout = l ? *l : grk_amd_pixel_layout{};
    return GRK_AMD_OK;
}

int grk_amd_set_decode_pixel_layout(grk_amd_ctx* c, const grk_amd_pixel_layout* l)
{
    if (!c) return GRK_AMD_ERR_INVALID;
    c->dec_layout = l ? *l : grk_amd_pixel_layout{};
    return GRK_AMD_OK;
}

uint64_t grk_amd_pixel_bytes(const grk_amd_tile_params* p, const grk_amd_pixel_layout* l, uint32_t w, uint32_t h, uint32_t ntiles)
{
    PixelLayout r; const char* why;
    if (!p) return 0;
    return resolve_pixel_layout(*p, l, w, h, ntiles, r, &why) ? r.bytes : 0;
}

const char* grk_amd_last_error(grk_amd_ctx* c) { return c ? c->err.c_str() : "null context"; }

int grk_amd_set_stream(grk_amd_ctx* c, void* s)
{
    if (!c) return GRK_AMD_ERR_INVALID;
    (void)hipStreamSynchronize(c->stream);
    if (c->own_stream) { (void)hipStreamDestroy(c->stream); c->own_stream = false; }
    if (s) c->stream = (hipStream_t)s;
    else {
        if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) return GRK_AMD_ERR_NO_DEVICE;
        c->own_stream = true;
    }
    return GRK_AMD_OK;
}

int64_t grk_amd_tile_layout(const grk_amd_tile_params* p, grk_amd_block* blocks, uint64_t cap, uint16_t* qcd)
{
    if (!p) return GRK_AMD_ERR_INVALID;
    TileGeom g;
    int rc = build_tile_geom(*p, g);
    if (rc != GRK_AMD_OK) return rc;
    const uint64_t n = (uint64_t)g.blocks_per_comp * p->num_comps;
    if (blocks) {
        if (cap < n) return GRK_AMD_ERR_INVALID;
        uint64_t i = 0;
        for (uint32_t k = 0; k < p->num_comps; ++k)
            for (auto b : g.blocks_comp0) { b.comp = (uint16_t)k; blocks[i++] = b; }
    }
    if (qcd) std::memcpy(qcd, g.qcd_words, sizeof(uint16_t) * g.num_bands_total);
    return (int64_t)n;
}

int grk_amd_tile_precincts(const grk_amd_tile_params* p, uint32_t* counts)
{
    if (!p || !counts) return GRK_AMD_ERR_INVALID;
    TileGeom g;
    const int rc = build_tile_geom(*p, g);
    if (rc != GRK_AMD_OK) return rc;
    for (uint32_t r = 0; r <= p->num_levels; ++r) counts[r] = g.res[r].npw * g.res[r].nph;
    return GRK_AMD_OK;
}

uint32_t grk_amd_plane_stride(const grk_amd_tile_params* p) { return p ? ((p->tile_w + 31u) & ~31u) : 0; }
uint64_t grk_amd_plane_elems(const grk_amd_tile_params* p) { return p ? (uint64_t)grk_amd_plane_stride(p) * p->tile_h : 0; }
void* grk_amd_plane_device_ptr(grk_amd_ctx* c, int which) { return c ? (which ? c->p1.p : c->p0.p) : nullptr; }

int grk_amd_synchronize(grk_amd_ctx* c)
{
    if (!c) return GRK_AMD_ERR_INVALID;
    { const int jr = join_side(c); if (jr) return jr; }
    HIP_TRY(c, hipStreamSynchronize(c->stream), "sync");
    if (c->side) HIP_TRY(c, hipStreamSynchronize(c->side), "sync side stream");        // (a pipelined predecessor)
    if (c->side2) HIP_TRY(c, hipStreamSynchronize(c->side2), "sync side stream 2");
    for (grk_amd_ctx* k : c->dec_kids) { const int kr = grk_amd_synchronize(k); if (kr) { c->err = k->err; return kr; } }
    return GRK_AMD_OK;
}

void* grk_amd_host_alloc(grk_amd_ctx* c, uint64_t bytes)
{
    if (!c || !bytes) return nullptr;
    if (hipSetDevice(c->device) != hipSuccess) return nullptr;
    void* p = nullptr;
    if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    return p;
}

void grk_amd_host_free(grk_amd_ctx* c, void* p)
{
    if (p) { if (c) (void)hipSetDevice(c->device); (void)hipHostFree(p); }
}

int grk_amd_plane_sample_bytes(grk_amd_ctx* c, const grk_amd_tile_params* p, int decode, uint32_t* packed_levels)
{
    if (!c || !p) return GRK_AMD_ERR_INVALID;
    const uint32_t bps = (p->prec + 7u) / 8u;
    bool h16;
    if (decode)
        h16 = c->dec_planes16 && p->num_levels >= 1 && bps <= 2 && c->fuse_egress && !p->reserved[0] && !p->irreversible &&
              p->prec <= 8 && c->dec_seg_first.empty();
    else
        h16 = c->planes16 && p->num_levels >= 1 && planes16_ok(*p);
    if (packed_levels) {
        *packed_levels = 0;
        if (h16 && c->dwt_pk && !decode)
            for (uint32_t l = 0; l < p->num_levels; ++l) *packed_levels += pk16_level_ok(*p, l) ? 1u : 0u;
    }
    return h16 ? 2 : 4;
}

int grk_amd_set_overlap(grk_amd_ctx* c, int on)
{
    if (!c) return GRK_AMD_ERR_INVALID;
    (void)grk_amd_synchronize(c);
    c->overlap = on != 0 && c->side != nullptr && c->side2 != nullptr;
    return GRK_AMD_OK;
}

int grk_amd_enable_timing(grk_amd_ctx* c, int on)
{
    if (!c) return GRK_AMD_ERR_INVALID;
    (void)hipStreamSynchronize(c->stream);
    drain_timers(c);
    for (auto& t : c->timers) { t.total_ms = 0; t.launches = 0; }
    c->timing = on != 0;
    return GRK_AMD_OK;
}

double grk_amd_kernel_ms(grk_amd_ctx* c, int which, uint32_t* launches)
{
    if (!c || which < 0 || which > 9) return -1.0;
    (void)hipStreamSynchronize(c->stream);
    drain_timers(c);
    if (launches) *launches = c->timers[which].launches;
    return c->timers[which].launches ? c->timers[which].total_ms / c->timers[which].launches : 0.0;
}
} // extern "C"
