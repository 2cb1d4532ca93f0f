// grok_amd/csrc/decode_sequence.hip -- decode: a SEQUENCE of frames in flight (grk_amd_set_decode_pipelining): each
// grk_amd_decode_tiles call with device buffers goes to one of the context's internal contexts in turn (context.h: dec_kids).
#include "decode_internal.h"

namespace {
// what the caller set on the context applies to the frame wherever it is decoded
void apply_settings(const grk_amd_ctx* c, grk_amd_ctx* k)
{
    if (k->dec_qcd != c->dec_qcd || k->dec_steps != c->dec_steps) { k->dec_qcd = c->dec_qcd; k->dec_steps = c->dec_steps; k->have_geom = false; }
    if (k->dec_seg_first != c->dec_seg_first) k->dec_seg_first = c->dec_seg_first;
    k->dec_reduce = c->dec_reduce; k->dec_layout = c->dec_layout;
    if (k->dec_segs.size() != c->dec_segs.size() ||
        (!c->dec_segs.empty() && std::memcmp(k->dec_segs.data(), c->dec_segs.data(), c->dec_segs.size() * sizeof(c->dec_segs[0])) != 0))
        k->dec_segs = c->dec_segs;
    k->dec_planes16 = c->dec_planes16; k->fuse_egress = c->fuse_egress; k->dwt_pk = c->dwt_pk; k->dwt_xcd = c->dwt_xcd;
    k->overlap = c->overlap && k->side != nullptr; k->t1_lanes = c->t1_lanes;
}

// The contexts' streams, vetted in the contexts' order: a context's two streams against each other and against the (up to
// three) streams accepted just before -- four dispatch pipes: two frames in flight can have a pipe per stream (HT frames:
// 0.66 instead of 0.75-0.81 ms per frame when the runtime's choice collides, tools/hwq_alias_dec.py), more cannot.
// (A convenience like the encoder's probe: when it cannot run, the streams stay as they are and it is not tried again)
void vet_sequence_streams(grk_amd_ctx* c, grk_amd_ctx* k)
{
    if (!c->stream_probe || k->seq_vetted) return;
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
} // namespace

extern "C" {
int grk_amd_decode_tiles(grk_amd_ctx* c, const grk_amd_tile_params* p, uint32_t ntiles,
                         const grk_amd_coded_block* table, const void* coded, uint64_t coded_bytes, int coded_on_device,
                         void* pixels, int pixels_on_device)
{
    if (!c || c->dec_kids.empty() || !coded_on_device || !pixels_on_device)
        return decode_impl(c, p, ntiles, table, coded, coded_bytes, coded_on_device, pixels, pixels_on_device, nullptr);
    // (every frame of the sequence on one of the internal contexts, none on this one: the event below must stand for what the
    //  CALLER queued on this context's stream, not for an earlier frame of the sequence)
    grk_amd_ctx* k = c->dec_kids[c->dec_seq++ % (uint32_t)c->dec_kids.size()];
    apply_settings(c, k);
    HIP_TRY(c, hipSetDevice(c->device), "set device");
    { const int sr = sequence_streams(k, p && p->reserved[0] != 0); if (sr) { c->err = k->err; return sr; } }
    vet_sequence_streams(c, k);
    // ... behind whatever the caller queued on this context's stream (its uploads of the coded bytes)
    { const int orc = order_behind(c, k->stream, c->ev_seq, c->stream, "record the caller's stream", "order the frame behind the caller's stream"); if (orc) return orc; }
    const int rc = decode_impl(k, p, ntiles, table, coded, coded_bytes, 1, pixels, 1, nullptr);
    // (the frame's last kernels -- the final inverse level, behind its join with the side stream -- are on k's stream; a call
    //  that failed half-way may have queued kernels that still read the coded bytes or write the pixels: the set's event covers
    //  those too, its side stream joined first)
    HIP_TRY(c, ensure_event(&k->ev_frame_done), "create event");
    if (rc && k->side) {
        HIP_TRY(c, ensure_event(&k->ev_dec_top), "create event");
        { const int jrc = order_behind(c, k->stream, k->ev_dec_top, k->side, "record the side stream", "join the side stream"); if (jrc) return jrc; }
        k->dec_top_pending = false;
    }
    HIP_TRY(c, hipEventRecord(k->ev_frame_done, k->stream), "record the frame's end");
    if (rc) c->err = k->err;
    return rc;
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
    if (frames_in_flight >= 2) HIP_TRY(c, ensure_event(&c->ev_seq), "create event");
    for (int i = 0; i < frames_in_flight && frames_in_flight >= 2; ++i) {
        grk_amd_ctx* k = nullptr;
        rc = create_context(c->device, c->verbose, true, &k);
        if (rc) return fail(c, rc, "a further decode context could not be made");
        k->seq_index = i;
        c->dec_kids.push_back(k);
    }
    return GRK_AMD_OK;
}
} // extern "C"
