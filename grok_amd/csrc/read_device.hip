// grok_amd/csrc/read_device.hip -- a codestream that lies in DEVICE memory read where it lies (grk_amd_read_header_device,
// grk_amd_read_packets_device, grk_amd_decode_image_device): the executor of t2_read_plan.h over the kernels of kernels_t2read.hip.
// What comes to the host is the main header (read_stream_header runs on the copy), the call's status word and the finished rows;
// what goes up is the plan's descriptors -- once per kind of stream: the plan is kept while the header stays the same -- and TLM's
// places.  No byte of a tile-part crosses the link.  The _ex calls run the general reader (plan_t2_read_layers; KC-L, KF, KP) for
// files of several layers or codeword segments: segment lists come to the host where a caller or the Part-1 decoder wants them,
// the moves only to a caller that asks -- a decode's gather reads them where KP left them.
// grk_amd_read_packets_device_parts is the general reader for tiles divided into tile-parts: KL-P and KH-P build a part table in the
// place of KL and KH, KC-L reads a tile's bytes through it; the _ex decode turns to it when KL refuses a second tile-part.
#include "context.h"
#include "t2_read_plan.h"
#include "t2_reader.h"

struct ReadDevState {
    bool have_plan = false;
    grk_amd_stream_info info{};
    T2ReadPlan plan;
    DevBuf tiles, packets, parts, plt_len, pk_start, nodes, rows, status, tlm;
    uint8_t* pin = nullptr; size_t pin_cap = 0;         // the header's copy, the status word behind a 16-byte boundary
    uint32_t last_why = 0;                              // why the latest status word refused (T2pWhy)
    uint64_t counters[7] = {0, 0, 0, 0, 0, 0, 0};         // [6]: launches of KL-P / KH-P; the located count comes to the host with the status word behind KL-P
    // the general reader (grk_amd_read_packets_device_ex): its own plan and descriptors, the scratch of KC-L, KF and KP
    bool have_lplan = false, lplan_refine = false;
    grk_amd_stream_info linfo{};
    T2ReadLayersPlan lplan;
    DevBuf ltiles, lpackets, lpk, nodes32, rstate, seg_log, piece_log, counts, first_seg, app_at, move_first, sums, totals, segments, moves;
};

void read_device_release(grk_amd_ctx* c)
{
    ReadDevState* r = c->rdev;
    if (!r) return;
    for (DevBuf* b : {&r->tiles, &r->packets, &r->parts, &r->plt_len, &r->pk_start, &r->nodes, &r->rows, &r->status, &r->tlm, &r->ltiles, &r->lpackets, &r->lpk,
                      &r->nodes32, &r->rstate, &r->seg_log, &r->piece_log, &r->counts, &r->first_seg, &r->app_at, &r->move_first, &r->sums, &r->totals,
                      &r->segments, &r->moves}) b->release();
    if (r->pin) (void)hipHostFree(r->pin);
    delete r;
    c->rdev = nullptr;
}

namespace {

ReadDevState* state(grk_amd_ctx* c) { if (!c->rdev) c->rdev = new ReadDevState; return c->rdev; }

int ensure_pin(grk_amd_ctx* c, ReadDevState* r, size_t n)
{
    if (n <= r->pin_cap) return GRK_AMD_OK;
    uint8_t* p = nullptr;
    const size_t want = n + (n >> 1) + 64;
    HIP_TRY(c, hipHostMalloc((void**)&p, want, hipHostMallocDefault), "alloc the header's copy");
    if (r->pin) { std::memcpy(p, r->pin, r->pin_cap); (void)hipHostFree(r->pin); }
    r->pin = p; r->pin_cap = want;
    return GRK_AMD_OK;
}

// What read_stream_header will look at in a stream of `len` bytes of which buf holds the first `have`: the bytes up to where its
// walks end.  <= have: everything it reads is there
uint64_t header_need(const uint8_t* b, uint64_t have, uint64_t len)
{
    auto u16 = [&](uint64_t i) { return (uint32_t)(b[i] << 8 | b[i + 1]); };
    if (have < 4) return std::min<uint64_t>(len, 4);
    uint64_t at = 2;
    for (;;) {
        if (at + 4 > len) return have;
        if (at + 4 > have) return at + 4;
        const uint32_t m = u16(at);
        if (m == 0xFF90) break;
        const uint32_t l = u16(at + 2);
        if (m < 0xFF30 || l < 2 || at + 2 + l > len) return have;
        if (at + 2 + l > have) return std::min<uint64_t>(len, at + 2 + (uint64_t)l + 16);
        at += 2 + (uint64_t)l;
    }
    // (the first tile-part's header says whether the file has PLT: up to its first PLT or SOD)
    for (uint64_t q = at + 12;;) {
        if (q + 4 > len) return have;
        if (q + 4 > have) return q + 4;
        const uint32_t m = u16(q), l = u16(q + 2);
        if (m == 0xFF93 || m == 0xFF58 || m < 0xFF30 || l < 2) return have;
        q += 2 + (uint64_t)l;
    }
}

// The main header to the host, in the order of the context's stream: GRK_AMD_READ_DEVICE_FIRST_COPY bytes, then -- a long COM, a
// TLM of thousands of tiles -- what the first copy shows is missing.  *have: bytes of the stream in r->pin
int fetch_header(grk_amd_ctx* c, ReadDevState* r, const void* d_cs, uint64_t len, uint64_t* have)
{
    uint64_t got = 0, want = std::min<uint64_t>(len, GRK_AMD_READ_DEVICE_FIRST_COPY);
    for (int turn = 0; turn < 64 && want > got; ++turn) {
        const int rc = ensure_pin(c, r, want + 32); if (rc) return rc;
        HIP_TRY(c, hipMemcpyAsync(r->pin + got, (const uint8_t*)d_cs + got, want - got, hipMemcpyDeviceToHost, c->stream), "fetch the main header");
        HIP_TRY(c, hipStreamSynchronize(c->stream), "sync");
        r->counters[0] += want - got;
        got = want;
        const uint64_t need = header_need(r->pin, got, len);
        if (need > got) want = std::min<uint64_t>(len, need + 2048);
    }
    *have = got;
    return GRK_AMD_OK;
}

int header_device(grk_amd_ctx* c, const void* d_cs, uint64_t len, grk_amd_stream_info& info, uint64_t* have)
{
    ReadDevState* r = state(c);
    HIP_TRY(c, hipSetDevice(c->device), "set device");
    int rc = fetch_header(c, r, d_cs, len, have); if (rc) return rc;
    std::string why;
    // (the copy holds every byte read_stream_header looks at: over it the result is what the whole stream gives)
    rc = read_stream_header(r->pin, *have, info, why);
    return rc ? fail(c, rc, why.c_str()) : GRK_AMD_OK;
}

// a call's status word as the call's refusal
int refuse_status(grk_amd_ctx* c, uint64_t st)
{
    char buf[200];
    const uint32_t why = t2p_status_why(st);
    if (c->rdev) c->rdev->last_why = why;
    if (!t2p_status_is_tile(st)) std::snprintf(buf, sizeof buf, "tile-part %u: %s", t2p_status_number(st), t2p_text(why));
    else if (t2p_status_stage(st) == 0) std::snprintf(buf, sizeof buf, "tile %u: %s", t2p_status_tile_of(st), t2p_text(why));
    else std::snprintf(buf, sizeof buf, "tile %u %s %u: %s", t2p_status_tile_of(st), t2p_status_stage(st) == 1 ? "packet" : "block", t2p_status_number(st), t2p_text(why));
    return fail(c, t2p_code(why), buf);
}

// the rows of the stream whose header (info; its first `have` bytes in the pinned copy) the caller has read: into tab.rows on the
// host when tab != nullptr, else into rows[row_cap] (nullptr: counted only)
int64_t packets_device(grk_amd_ctx* c, const void* d_cs, uint64_t len, const grk_amd_stream_info& info, uint64_t have, grk_amd_coded_block* rows,
                       uint64_t row_cap, StreamTable* tab)
{
    ReadDevState* r = state(c);
    const char* pwhy = "";
    HIP_TRY(c, hipStreamSynchronize(c->stream), "sync");          // (the tables below may still be read by an earlier call's kernels)
    if (!r->have_plan || std::memcmp(&r->info, &info, sizeof info) != 0) {
        r->have_plan = false;
        const int rc = plan_t2_read(info, r->plan, &pwhy);
        if (rc) return fail(c, rc, pwhy);
        HIP_TRY(c, r->tiles.ensure(r->plan.bytes_tiles()), "alloc the tiles' descriptors");
        HIP_TRY(c, r->packets.ensure(r->plan.bytes_packets()), "alloc the packets' descriptors");
        HIP_TRY(c, hipMemcpy(r->tiles.p, r->plan.tiles.data(), r->plan.bytes_tiles(), hipMemcpyHostToDevice), "upload the tiles' descriptors");
        HIP_TRY(c, hipMemcpy(r->packets.p, r->plan.packets.data(), r->plan.bytes_packets(), hipMemcpyHostToDevice), "upload the packets' descriptors");
        r->counters[1] += r->plan.bytes_tiles() + r->plan.bytes_packets();
        r->info = info; r->have_plan = true;
    }
    const T2ReadPlan& P = r->plan;
    const uint32_t nt = P.num_tiles;
    // TLM's places, or where the Psot chain starts
    bool tlm = false;
    std::vector<uint64_t> at; std::vector<uint32_t> ln, idx;
    uint64_t count = 0;
    if (t2_read_tlm(r->pin, have, len, nt, &tlm, at, ln, idx, &count)) return fail(c, GRK_AMD_ERR_INVALID, t2p_text(kT2pNotLocated));
    uint64_t sot_at = 2;
    while (sot_at + 4 <= have && !(r->pin[sot_at] == 0xFF && r->pin[sot_at + 1] == 0x90)) sot_at += 2 + ((uint64_t)r->pin[sot_at + 2] << 8 | r->pin[sot_at + 3]);
    const uint64_t entries = std::max<uint64_t>(P.total_packets, nt);
    HIP_TRY(c, r->parts.ensure((size_t)nt * 32), "alloc the tile-parts' places");
    HIP_TRY(c, r->plt_len.ensure(entries * 4), "alloc packet lengths");
    HIP_TRY(c, r->pk_start.ensure(entries * 8), "alloc packet starts");
    HIP_TRY(c, r->nodes.ensure(P.node_bytes + 16), "alloc tag-tree nodes");
    HIP_TRY(c, r->rows.ensure(P.bytes_rows() + 16), "alloc the rows");
    HIP_TRY(c, r->status.ensure(8), "alloc status");
    T2ReadArgs a{};
    a.cs = (const uint8_t*)d_cs; a.len = len; a.num_tiles = nt;
    a.tiles = (const T2ReadTile*)r->tiles.p; a.packets = (const T2ReadPacket*)r->packets.p;
    a.ht = P.ht; a.sop = P.sop; a.eph = P.eph;
    if (tlm) {
        std::vector<T2ReadTlmEntry> e(at.size());
        for (size_t i = 0; i < e.size(); ++i) e[i] = T2ReadTlmEntry{at[i], ln[i], idx[i]};
        HIP_TRY(c, r->tlm.ensure(e.size() * sizeof e[0] + 16), "alloc TLM's places");
        if (!e.empty()) HIP_TRY(c, hipMemcpy(r->tlm.p, e.data(), e.size() * sizeof e[0], hipMemcpyHostToDevice), "upload TLM's places");
        r->counters[1] += e.size() * sizeof e[0];
        a.tlm = (const T2ReadTlmEntry*)r->tlm.p; a.tlm_n = (uint32_t)e.size(); a.tlm_count = count;
    }
    a.sot_at = sot_at;
    uint8_t* const parts = (uint8_t*)r->parts.p;                // per tile 32 bytes: 8 + 8 + 4 + 4 + 4
    a.part_at = (unsigned long long*)parts; a.body_at = (unsigned long long*)(parts + (size_t)nt * 8);
    a.part_len = (uint32_t*)(parts + (size_t)nt * 16); a.has_plt = (uint32_t*)(parts + (size_t)nt * 20); a.first_of = (uint32_t*)(parts + (size_t)nt * 24);
    a.plt_len = (uint32_t*)r->plt_len.p; a.pk_start = (unsigned long long*)r->pk_start.p;
    a.nodes = (uint8_t*)r->nodes.p; a.rows = (grk_amd_coded_block*)r->rows.p;
    a.status = (unsigned long long*)r->status.p; a.chains = P.chains;
    HIP_TRY(c, hipMemsetAsync(r->status.p, 0xFF, 8, c->stream), "clear status");
    HIP_TRY(c, launch_t2read_locate(a, c->stream), "launch KL");
    HIP_TRY(c, launch_t2read_headers(a, c->stream), "launch KH");
    HIP_TRY(c, launch_t2read_chains(a, c->stream), "launch KC");
    ++r->counters[2]; r->counters[3] += P.chains;
    int rc = ensure_pin(c, r, have + 32); if (rc) return rc;
    uint64_t* const h_status = (uint64_t*)(r->pin + ((have + 15) & ~(uint64_t)15));
    HIP_TRY(c, hipMemcpyAsync(h_status, r->status.p, 8, hipMemcpyDeviceToHost, c->stream), "fetch status");
    HIP_TRY(c, hipStreamSynchronize(c->stream), "sync");
    r->counters[0] += 8;
    const uint64_t st = *h_status;
    if (st != kT2pNoStatus) return refuse_status(c, st);
    if (tab) {
        *tab = StreamTable{};
        tab->rows.resize(P.rows);
        tab->row_at.assign(nt + 1, P.rows); tab->move_at.assign(nt + 1, 0);
        for (uint32_t t = 0; t < nt; ++t) tab->row_at[t] = P.tiles[t].row_base;
        tab->first_segment.assign(P.rows + 1, 0);
        rows = tab->rows.data(); row_cap = P.rows;
    }
    if (!rows) return (int64_t)P.rows;
    if (P.rows > row_cap) return fail(c, GRK_AMD_ERR_OVERFLOW, "the rows do not fit the caller's array");
    if (P.rows) { rc = copy_d2h(c, rows, r->rows.p, P.bytes_rows()); if (rc) return rc; }
    r->counters[0] += P.bytes_rows();
    return (int64_t)P.rows;
}

// ---- the general reader ------------------------------------------------------------------------------------------------------------
// What a call of it hands out: host arrays (nullptr: not wanted), or -- tab != nullptr, a decode -- the table with the moves left in
// device memory (r->moves; *num_moves of them)
struct ReadExOut {
    grk_amd_coded_block* rows; uint64_t row_cap;
    uint32_t* first_segment; grk_amd_segment* segments; uint64_t seg_cap; uint64_t* num_segments;
    grk_amd_tp_segment* moves; uint64_t move_cap; uint64_t* num_moves; uint64_t* appendix_bytes;
    StreamTable* tab; bool tab_segments;
};

// parts: tiles divided into tile-parts are read (KL-P, KH-P and KC-L over the part table in the place of KL, KH and KC-L)
// ht_refine: HT blocks' refinement passes are read -- the plan's sizes and the style word KC-L hands the parse core say so
int64_t packets_device_ex(grk_amd_ctx* c, const void* d_cs, uint64_t len, const grk_amd_stream_info& info, uint64_t have, const ReadExOut& o, bool parts = false,
                          bool ht_refine = false)
{
    ReadDevState* r = state(c);
    const char* pwhy = "";
    HIP_TRY(c, hipStreamSynchronize(c->stream), "sync");          // (the tables below may still be read by an earlier call's kernels)
    if (!r->have_lplan || r->lplan_refine != ht_refine || std::memcmp(&r->linfo, &info, sizeof info) != 0) {
        r->have_lplan = false;
        const int rc = plan_t2_read_layers(info, r->lplan, &pwhy, ht_refine);
        if (rc) return fail(c, rc, pwhy);
        const T2ReadLayersPlan& Q = r->lplan;
        HIP_TRY(c, r->ltiles.ensure(Q.base.bytes_tiles()), "alloc the tiles' descriptors");
        HIP_TRY(c, r->lpackets.ensure(Q.base.bytes_packets()), "alloc the packets' descriptors");
        HIP_TRY(c, r->lpk.ensure(Q.bytes_lpk()), "alloc the precincts' descriptors");
        HIP_TRY(c, hipMemcpy(r->ltiles.p, Q.base.tiles.data(), Q.base.bytes_tiles(), hipMemcpyHostToDevice), "upload the tiles' descriptors");
        HIP_TRY(c, hipMemcpy(r->lpackets.p, Q.base.packets.data(), Q.base.bytes_packets(), hipMemcpyHostToDevice), "upload the packets' descriptors");
        HIP_TRY(c, hipMemcpy(r->lpk.p, Q.lpk.data(), Q.bytes_lpk(), hipMemcpyHostToDevice), "upload the precincts' descriptors");
        r->counters[1] += Q.base.bytes_tiles() + Q.base.bytes_packets() + Q.bytes_lpk();
        r->linfo = info; r->have_lplan = true; r->lplan_refine = ht_refine;
    }
    const T2ReadLayersPlan& Q = r->lplan;
    const T2ReadPlan& P = Q.base;
    const uint32_t nt = P.num_tiles;
    bool tlm = false;
    std::vector<uint64_t> at; std::vector<uint32_t> ln, idx;
    uint64_t count = 0;
    if (t2_read_tlm(r->pin, have, len, parts ? kT2pMaxPartsOfFile : nt, &tlm, at, ln, idx, &count)) return fail(c, GRK_AMD_ERR_INVALID, t2p_text(kT2pNotLocated));
    uint64_t sot_at = 2;
    while (sot_at + 4 <= have && !(r->pin[sot_at] == 0xFF && r->pin[sot_at + 1] == 0x90)) sot_at += 2 + ((uint64_t)r->pin[sot_at + 2] << 8 | r->pin[sot_at + 3]);
    const uint64_t entries = std::max<uint64_t>(P.total_packets, nt), nblocks = (P.rows + kT2ReadScanRows - 1) / kT2ReadScanRows;
    // the part table's room: TLM says how many tile-parts the file has; without, the Psot chain cannot have more than len / 14 + 1
    if (parts && tlm && count > kT2pMaxPartsOfFile) return fail(c, GRK_AMD_ERR_UNSUPPORTED, t2p_text(kT2pPartsOfFile));
    const uint64_t cap = !parts ? 0 : tlm ? std::max<uint64_t>(count, 1) : std::min<uint64_t>(len / 14 + 1, kT2pMaxPartsOfFile);
    const size_t tile_words = ((size_t)nt * 4 + 4 + 7) & ~(size_t)7;         // a per-tile array of 32-bit words, 8-byte aligned
    HIP_TRY(c, r->parts.ensure(parts ? (size_t)nt * 8 + 5 * tile_words + (size_t)cap * 64 + 64 : (size_t)nt * 32), "alloc the tile-parts' places");
    HIP_TRY(c, r->plt_len.ensure(entries * 4), "alloc packet lengths");
    HIP_TRY(c, r->pk_start.ensure(entries * 8), "alloc packet starts");
    HIP_TRY(c, r->nodes32.ensure(Q.bytes_nodes() + 16), "alloc tag-tree nodes");
    HIP_TRY(c, r->rows.ensure(P.bytes_rows() + 16), "alloc the rows");
    HIP_TRY(c, r->rstate.ensure(Q.bytes_state() + 16), "alloc the rows' state");
    HIP_TRY(c, r->seg_log.ensure(Q.bytes_seg_log() + 16), "alloc the segment log");
    HIP_TRY(c, r->piece_log.ensure(Q.bytes_piece_log() + 16), "alloc the piece log");
    HIP_TRY(c, r->counts.ensure(Q.bytes_counts() + 16), "alloc the chains' counts");
    HIP_TRY(c, r->first_seg.ensure((P.rows + 1) * 4 + 16), "alloc first_segment");
    HIP_TRY(c, r->app_at.ensure(P.rows * 8 + 16), "alloc the appendix places");
    HIP_TRY(c, r->move_first.ensure(P.rows * 4 + 16), "alloc the rows' first moves");
    HIP_TRY(c, r->sums.ensure(nblocks * 24 + 16), "alloc the scan's sums");
    HIP_TRY(c, r->totals.ensure(32), "alloc the totals");
    HIP_TRY(c, r->status.ensure(16), "alloc status");
    T2ReadLayersArgs g{};
    T2ReadArgs& a = g.a;
    a.cs = (const uint8_t*)d_cs; a.len = len; a.num_tiles = nt;
    a.tiles = (const T2ReadTile*)r->ltiles.p; a.packets = (const T2ReadPacket*)r->lpackets.p;
    a.ht = P.ht; a.sop = P.sop; a.eph = P.eph;
    if (tlm && !parts) {
        std::vector<T2ReadTlmEntry> e(at.size());
        for (size_t i = 0; i < e.size(); ++i) e[i] = T2ReadTlmEntry{at[i], ln[i], idx[i]};
        HIP_TRY(c, r->tlm.ensure(e.size() * sizeof e[0] + 16), "alloc TLM's places");
        if (!e.empty()) HIP_TRY(c, hipMemcpy(r->tlm.p, e.data(), e.size() * sizeof e[0], hipMemcpyHostToDevice), "upload TLM's places");
        r->counters[1] += e.size() * sizeof e[0];
        a.tlm = (const T2ReadTlmEntry*)r->tlm.p; a.tlm_n = (uint32_t)e.size(); a.tlm_count = count;
    }
    a.sot_at = sot_at;
    uint8_t* const pbuf = (uint8_t*)r->parts.p;                 // per tile 32 bytes: 8 + 8 + 4 + 4 + 4
    T2ReadPartsArgs pa{};
    if (!parts) {
        a.part_at = (unsigned long long*)pbuf; a.body_at = (unsigned long long*)(pbuf + (size_t)nt * 8);
        a.part_len = (uint32_t*)(pbuf + (size_t)nt * 16); a.has_plt = (uint32_t*)(pbuf + (size_t)nt * 20); a.first_of = (uint32_t*)(pbuf + (size_t)nt * 24);
    } else {
        // per tile: body_at (8), then has_plt, count, tn_min, tn_max, slice (4 each, slice one more); per tile-part of `cap`: 64 bytes
        uint8_t* q = pbuf;
        a.body_at = (unsigned long long*)q; q += (size_t)nt * 8;
        a.has_plt = (uint32_t*)q; q += tile_words;
        pa.count = (uint32_t*)q; q += tile_words;
        pa.tn_min = (uint32_t*)q; q += tile_words;
        pa.tn_max = (uint32_t*)q; q += tile_words;
        pa.slice = (uint32_t*)q; q += tile_words;
        pa.fo_at = (unsigned long long*)q; q += cap * 8;
        pa.tp_at = (unsigned long long*)q; q += cap * 8;
        pa.tp_body = (unsigned long long*)q; q += cap * 8;
        uint32_t** const words[] = {&pa.fo_len, &pa.fo_idx, &pa.claim, &pa.tp_len, &pa.tp_tile, &pa.tp_file, &pa.tp_has_plt, &pa.tp_npk, &pa.tp_first};
        for (uint32_t** w : words) { *w = (uint32_t*)q; q += cap * 4; }
        pa.cap = (uint32_t)cap; pa.n_given = tlm ? (uint32_t)count : 0u;
        pa.located = (unsigned long long*)r->status.p + 1;
        if (tlm) {
            // (TLM's places go up as the file-order arrays; a.tlm stays unused)
            if (at.size() != count) return fail(c, GRK_AMD_ERR_INVALID, t2p_text(kT2pNotLocated));
            if (count) {
                HIP_TRY(c, hipMemcpy(pa.fo_at, at.data(), count * 8, hipMemcpyHostToDevice), "upload TLM's places");
                HIP_TRY(c, hipMemcpy(pa.fo_len, ln.data(), count * 4, hipMemcpyHostToDevice), "upload TLM's lengths");
                HIP_TRY(c, hipMemcpy(pa.fo_idx, idx.data(), count * 4, hipMemcpyHostToDevice), "upload TLM's tile indices");
            }
        }
    }
    a.plt_len = (uint32_t*)r->plt_len.p; a.pk_start = (unsigned long long*)r->pk_start.p;
    a.rows = (grk_amd_coded_block*)r->rows.p;
    a.status = (unsigned long long*)r->status.p; a.chains = P.chains;
    g.lpk = (const T2ReadLayerPk*)r->lpk.p;
    g.layers = Q.layers; g.order = Q.order; g.sty = Q.sty; g.seg_per_row = Q.seg_records_per_row; g.piece_per_row = Q.piece_records_per_row;
    g.nodes32 = (uint32_t*)r->nodes32.p; g.state = (T2pRowState*)r->rstate.p;
    g.seg_log = (T2ReadSegRecord*)r->seg_log.p; g.piece_log = (T2ReadPieceRecord*)r->piece_log.p; g.counts = (uint32_t*)r->counts.p;
    g.nrows = P.rows; g.first_segment = (uint32_t*)r->first_seg.p; g.app_at = (unsigned long long*)r->app_at.p; g.move_first = (uint32_t*)r->move_first.p;
    g.sums = (unsigned long long*)r->sums.p; g.totals = (unsigned long long*)r->totals.p;
    int rc = ensure_pin(c, r, have + 64); if (rc) return rc;
    uint64_t* const h_words = (uint64_t*)(r->pin + ((have + 15) & ~(uint64_t)15));          // the status word, then the three totals
    auto fetch_status = [&]() -> int {
        HIP_TRY(c, hipMemcpyAsync(h_words, r->status.p, 8, hipMemcpyDeviceToHost, c->stream), "fetch status");
        HIP_TRY(c, hipStreamSynchronize(c->stream), "sync");
        r->counters[0] += 8;
        return GRK_AMD_OK;
    };
    HIP_TRY(c, hipMemsetAsync(r->status.p, 0xFF, 8, c->stream), "clear status");
    HIP_TRY(c, hipMemsetAsync(r->totals.p, 0, 32, c->stream), "clear the totals");
    if (!parts) {
        HIP_TRY(c, launch_t2read_locate(a, c->stream), "launch KL");
        HIP_TRY(c, launch_t2read_headers(a, c->stream), "launch KH");
        HIP_TRY(c, launch_t2read_chains_layers(g, c->stream), "launch KC-L");
    } else {
        // KL-P, then the status word and the located count (one word) to the host: KH-P's grid is the file's tile-parts
        pa.g = g;
        HIP_TRY(c, hipMemsetAsync((uint8_t*)r->status.p + 8, 0, 8, c->stream), "clear the located count");
        HIP_TRY(c, launch_t2read_locate_parts(pa, c->stream), "launch KL-P");
        HIP_TRY(c, hipMemcpyAsync(h_words, r->status.p, 16, hipMemcpyDeviceToHost, c->stream), "fetch status and the located count");
        HIP_TRY(c, hipStreamSynchronize(c->stream), "sync");
        r->counters[0] += 16; ++r->counters[6];
        if (h_words[0] != kT2pNoStatus) return refuse_status(c, h_words[0]);
        const uint64_t located = h_words[1];
        if (!located || located > cap) return fail(c, GRK_AMD_ERR_INVALID, t2p_text(kT2pNotLocated));
        HIP_TRY(c, launch_t2read_headers_parts(pa, (uint32_t)located, c->stream), "launch KH-P");
        r->counters[6] += 2;
        HIP_TRY(c, launch_t2read_chains_parts(pa, c->stream), "launch KC-L");
    }
    ++r->counters[5]; r->counters[3] += P.chains;
    // (a chain that was refused, or never ran, leaves its rows' state as it was: KF and KP run on what every chain has finished)
    rc = fetch_status(); if (rc) return rc;
    if (h_words[0] != kT2pNoStatus) return refuse_status(c, h_words[0]);
    HIP_TRY(c, launch_t2read_finish(g, c->stream), "launch KF");
    HIP_TRY(c, hipMemcpyAsync(h_words + 1, r->totals.p, 24, hipMemcpyDeviceToHost, c->stream), "fetch the totals");
    r->counters[0] += 24;
    rc = fetch_status(); if (rc) return rc;
    if (h_words[0] != kT2pNoStatus) return refuse_status(c, h_words[0]);
    const uint64_t nseg = h_words[1], app = h_words[2], nmoves = h_words[3];
    if (nseg > P.rows * Q.segments_per_row || nmoves > P.rows * Q.piece_records_per_row) return fail(c, GRK_AMD_ERR_INVALID, "the reader's totals");
    if (o.num_segments) *o.num_segments = nseg;
    if (o.num_moves) *o.num_moves = nmoves;
    if (o.appendix_bytes) *o.appendix_bytes = app;
    if (!o.rows && !o.tab) return (int64_t)P.rows;
    if (!o.tab && (P.rows > o.row_cap || (o.segments && nseg > o.seg_cap) || (o.moves && nmoves > o.move_cap) || (!o.moves && nmoves)))
        return fail(c, GRK_AMD_ERR_OVERFLOW, "the rows, segments or moves do not fit the caller's arrays");
    const bool want_segments = o.tab ? o.tab_segments : o.segments != nullptr, want_moves = o.tab ? app != 0 : o.moves != nullptr;
    HIP_TRY(c, r->segments.ensure((want_segments ? nseg : 0) * sizeof(grk_amd_segment) + 16), "alloc the segments");
    HIP_TRY(c, r->moves.ensure((want_moves ? nmoves : 0) * sizeof(grk_amd_tp_segment) + 16), "alloc the moves");
    g.segments = (grk_amd_segment*)r->segments.p; g.seg_cap = want_segments ? nseg : 0;
    g.moves = (grk_amd_tp_segment*)r->moves.p; g.move_cap = want_moves ? nmoves : 0;
    if ((g.seg_cap || g.move_cap)) {
        if (g.seg_cap) HIP_TRY(c, hipMemsetAsync(r->segments.p, 0, nseg * sizeof(grk_amd_segment), c->stream), "clear the segments");
        HIP_TRY(c, launch_t2read_place(g, c->stream), "launch KP");
    }
    grk_amd_coded_block* rows = o.rows;
    uint32_t* first_segment = o.first_segment;
    grk_amd_segment* segments = o.segments;
    if (o.tab) {
        StreamTable& tab = *o.tab;
        tab = StreamTable{};
        tab.rows.resize(P.rows);
        tab.row_at.assign(nt + 1, P.rows); tab.move_at.assign(nt + 1, 0);
        for (uint32_t t = 0; t < nt; ++t) tab.row_at[t] = P.tiles[t].row_base;
        tab.first_segment.assign(P.rows + 1, 0);
        tab.appendix_bytes = app;
        rows = tab.rows.data();
        if (want_segments) { tab.segments.resize(nseg); first_segment = tab.first_segment.data(); segments = tab.segments.data(); }
    }
    if (P.rows) { rc = copy_d2h(c, rows, r->rows.p, P.bytes_rows()); if (rc) return rc; }
    r->counters[0] += P.bytes_rows();
    if (first_segment) { rc = copy_d2h(c, first_segment, r->first_seg.p, (P.rows + 1) * 4); if (rc) return rc; r->counters[0] += (P.rows + 1) * 4; }
    if (segments && nseg) { rc = copy_d2h(c, segments, r->segments.p, nseg * sizeof(grk_amd_segment)); if (rc) return rc; r->counters[0] += nseg * sizeof(grk_amd_segment); }
    if (!o.tab && o.moves && nmoves) { rc = copy_d2h(c, o.moves, r->moves.p, nmoves * sizeof(grk_amd_tp_segment)); if (rc) return rc; r->counters[0] += nmoves * sizeof(grk_amd_tp_segment); }
    HIP_TRY(c, hipStreamSynchronize(c->stream), "sync");
    return (int64_t)P.rows;
}

} // namespace

extern "C" int64_t grk_amd_read_packets_device_ex(grk_amd_ctx* c, const void* d_cs, uint64_t len, const grk_amd_stream_info* info, grk_amd_coded_block* rows,
                                                  uint64_t row_cap, uint32_t* first_segment, grk_amd_segment* segments, uint64_t seg_cap, uint64_t* num_segments,
                                                  grk_amd_tp_segment* moves, uint64_t move_cap, uint64_t* num_moves, uint64_t* appendix_bytes)
{
    if (!c || !d_cs || !info) return GRK_AMD_ERR_INVALID;
    grk_amd_stream_info own;
    uint64_t have = 0;
    const int rc = header_device(c, d_cs, len, own, &have); if (rc) return rc;
    if (std::memcmp(&own, info, sizeof own) != 0) return fail(c, GRK_AMD_ERR_INVALID, "info is not what grk_amd_read_header_device gives for this codestream");
    return packets_device_ex(c, d_cs, len, own, have, ReadExOut{rows, row_cap, first_segment, segments, seg_cap, num_segments, moves, move_cap, num_moves, appendix_bytes, nullptr, false});
}

extern "C" int64_t grk_amd_read_packets_device_parts(grk_amd_ctx* c, const void* d_cs, uint64_t len, const grk_amd_stream_info* info, grk_amd_coded_block* rows,
                                                     uint64_t row_cap, uint32_t* first_segment, grk_amd_segment* segments, uint64_t seg_cap, uint64_t* num_segments,
                                                     grk_amd_tp_segment* moves, uint64_t move_cap, uint64_t* num_moves, uint64_t* appendix_bytes)
{
    if (!c || !d_cs || !info) return GRK_AMD_ERR_INVALID;
    grk_amd_stream_info own;
    uint64_t have = 0;
    const int rc = header_device(c, d_cs, len, own, &have); if (rc) return rc;
    if (std::memcmp(&own, info, sizeof own) != 0) return fail(c, GRK_AMD_ERR_INVALID, "info is not what grk_amd_read_header_device gives for this codestream");
    return packets_device_ex(c, d_cs, len, own, have, ReadExOut{rows, row_cap, first_segment, segments, seg_cap, num_segments, moves, move_cap, num_moves, appendix_bytes, nullptr, false}, true);
}

extern "C" int64_t grk_amd_read_packets_device_refine(grk_amd_ctx* c, const void* d_cs, uint64_t len, const grk_amd_stream_info* info, grk_amd_coded_block* rows,
                                                      uint64_t row_cap, uint32_t* first_segment, grk_amd_segment* segments, uint64_t seg_cap, uint64_t* num_segments,
                                                      grk_amd_tp_segment* moves, uint64_t move_cap, uint64_t* num_moves, uint64_t* appendix_bytes)
{
    if (!c || !d_cs || !info) return GRK_AMD_ERR_INVALID;
    grk_amd_stream_info own;
    uint64_t have = 0;
    const int rc = header_device(c, d_cs, len, own, &have); if (rc) return rc;
    if (std::memcmp(&own, info, sizeof own) != 0) return fail(c, GRK_AMD_ERR_INVALID, "info is not what grk_amd_read_header_device gives for this codestream");
    return packets_device_ex(c, d_cs, len, own, have, ReadExOut{rows, row_cap, first_segment, segments, seg_cap, num_segments, moves, move_cap, num_moves, appendix_bytes, nullptr, false},
                             true, true);
}

extern "C" int grk_amd_decode_image_device_ex(grk_amd_ctx* c, const void* d_cs, uint64_t len, void* pixels, uint64_t cap, int pixels_on_device)
{
    if (!c || !d_cs || !pixels) return GRK_AMD_ERR_INVALID;
    int rc = refuse_context(c, "grk_amd_decode_image_device_ex", " at reduced resolution"); if (rc) return rc;
    grk_amd_stream_info info;
    uint64_t have = 0;
    rc = header_device(c, d_cs, len, info, &have); if (rc) return rc;
    StreamTable tab;
    uint64_t nmoves = 0;
    const bool want_segs = info.base.reserved[0] && (info.base.reserved[1] & 0x05);          // (Part-1 with LAZY / TERMALL: decode_image_plan's want_segs)
    // a file with one tile-part per tile goes the way it always went; one that KL refuses for a second tile-part is read again over
    // the part table (KL-P, KH-P)
    const ReadExOut out{nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr, 0, &nmoves, nullptr, &tab, want_segs};
    c->rdev->last_why = 0;
    int64_t n = packets_device_ex(c, d_cs, len, info, have, out);
    if (n == GRK_AMD_ERR_UNSUPPORTED && (c->rdev->last_why == kT2pMultiPart || c->rdev->last_why == kT2pManyParts)) n = packets_device_ex(c, d_cs, len, info, have, out, true);
    // ... and one that KC-L refuses for an HT block's second pass with the refinement passes read (over the part table: it reads
    // either kind of file), its segment lists to the host: the decode finds the refinement segments there
    if (n == GRK_AMD_ERR_UNSUPPORTED && c->rdev->last_why == kT2pHtPasses) {
        ReadExOut refine = out;
        refine.tab_segments = true;
        n = packets_device_ex(c, d_cs, len, info, have, refine, true, true);
    }
    if (n < 0) return (int)n;
    if (!tab.appendix_bytes) return decode_resident(c, d_cs, len, info, tab, pixels, cap, pixels_on_device);
    return decode_resident_moves(c, d_cs, len, info, tab, (const grk_amd_tp_segment*)c->rdev->moves.p, nmoves, &c->rdev->counters[4], pixels, cap, pixels_on_device);
}

extern "C" int grk_amd_read_header_device(grk_amd_ctx* c, const void* d_cs, uint64_t len, grk_amd_stream_info* info)
{
    if (!c || !d_cs || !info) return GRK_AMD_ERR_INVALID;
    uint64_t have = 0;
    return header_device(c, d_cs, len, *info, &have);
}

extern "C" int64_t grk_amd_read_packets_device(grk_amd_ctx* c, const void* d_cs, uint64_t len, const grk_amd_stream_info* info, grk_amd_coded_block* rows,
                                               uint64_t row_cap)
{
    if (!c || !d_cs || !info) return GRK_AMD_ERR_INVALID;
    grk_amd_stream_info own;
    uint64_t have = 0;
    const int rc = header_device(c, d_cs, len, own, &have); if (rc) return rc;
    if (std::memcmp(&own, info, sizeof own) != 0) return fail(c, GRK_AMD_ERR_INVALID, "info is not what grk_amd_read_header_device gives for this codestream");
    return packets_device(c, d_cs, len, own, have, rows, row_cap, nullptr);
}

extern "C" uint64_t grk_amd_read_device_counters(grk_amd_ctx* c, int which)
{
    return c && c->rdev && which >= 0 && which < 7 ? c->rdev->counters[which] : 0;
}

extern "C" int grk_amd_decode_image_device(grk_amd_ctx* c, const void* d_cs, uint64_t len, void* pixels, uint64_t cap, int pixels_on_device)
{
    if (!c || !d_cs || !pixels) return GRK_AMD_ERR_INVALID;
    int rc = refuse_context(c, "grk_amd_decode_image_device", " at reduced resolution"); if (rc) return rc;
    grk_amd_stream_info info;
    uint64_t have = 0;
    rc = header_device(c, d_cs, len, info, &have); if (rc) return rc;
    StreamTable tab;
    const int64_t n = packets_device(c, d_cs, len, info, have, nullptr, 0, &tab);
    if (n < 0) return (int)n;
    return decode_resident(c, d_cs, len, info, tab, pixels, cap, pixels_on_device);
}
