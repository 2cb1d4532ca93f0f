// grok_amd/csrc/streams.hip -- the context's streams: the probe that vets them, a decode sequence's streams, joining the side streams.
#include "context.h"

// (Streams and hardware queues: the HIP runtime multiplexes a process's streams onto its hardware-queue count of queues, 4 by
//  default, and kernels of two streams that share a queue run one after the other.  A decode sequence with three or more frames in
//  flight -- two streams of long kernels each -- gains nothing over two frames on 4 queues; on 8 the Part-1 sequence goes from 9.1 to
//  6.7 ms per frame.  It is the HOST's setting, process-wide and read when the runtime starts: the library does not touch it,
//  because the encode pipeline beside an RCCL exchange was measured 25 % slower on anything but 4 (profiles/r04_hw_queues.txt).)

namespace {
// 16 384 workgroups that hold 40 KB of LDS (four to a CU) for ~10 us each: ~160 us during which the grid is still being dispatched
__global__ __launch_bounds__(64) void probe_spin_kernel(unsigned int ticks, unsigned int* sink)
{
    extern __shared__ unsigned int pad[];              // 40 KB asked for at the launch
    pad[threadIdx.x] = threadIdx.x;
    const unsigned long long t0 = wall_clock64();
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(8);
    if (sink && pad[threadIdx.x] == 0xFFFFFFFFu) *sink = 1;
}
__global__ void probe_tick_kernel(unsigned int* sink) { if (sink && threadIdx.x == 1024) *sink = 1; }

// does a kernel launched on `b` while a large grid of `a` is in dispatch run at once?  (both streams idle on entry and on return)
int streams_side_by_side(grk_amd_ctx* c, hipStream_t a, hipStream_t b, bool* yes)
{
    hipEvent_t e0 = nullptr, ea = nullptr, eb = nullptr;
    hipError_t e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&ea);
    if (e == hipSuccess) e = hipEventCreate(&eb);
    if (e == hipSuccess) e = hipEventRecord(e0, a);
    if (e == hipSuccess) { hipLaunchKernelGGL(probe_spin_kernel, dim3(16384), dim3(64), 40960, a, 1000u, (unsigned int*)nullptr); e = hipGetLastError(); }
    if (e == hipSuccess) e = hipEventRecord(ea, a);
    // (the small kernel is launched once the grid has started: e0 has passed)
    if (e == hipSuccess) { while ((e = hipEventQuery(e0)) == hipErrorNotReady) {} }
    if (e == hipSuccess) { hipLaunchKernelGGL(probe_tick_kernel, dim3(1), dim3(64), 0, b, (unsigned int*)nullptr); e = hipGetLastError(); }
    if (e == hipSuccess) e = hipEventRecord(eb, b);
    if (e == hipSuccess) e = hipStreamSynchronize(a);
    if (e == hipSuccess) e = hipStreamSynchronize(b);
    float ta = 0, tb = 0;
    if (e == hipSuccess) e = hipEventElapsedTime(&ta, e0, ea);
    if (e == hipSuccess) e = hipEventElapsedTime(&tb, e0, eb);
    if (e0) (void)hipEventDestroy(e0);
    if (ea) (void)hipEventDestroy(ea);
    if (eb) (void)hipEventDestroy(eb);
    if (e != hipSuccess) return fail(c, GRK_AMD_ERR_NO_DEVICE, "stream probe", e);
    *yes = tb < 0.6f * ta;
    if (c->verbose) fprintf(stderr, "[grok_amd] stream probe: grid %.3f ms, small kernel done after %.3f ms -> %s\n", ta, tb, *yes ? "side by side" : "in turn");
    return GRK_AMD_OK;
}

int probe_warmup(grk_amd_ctx* c, hipStream_t st)
{
    if (c->probe_warm) return GRK_AMD_OK;
    hipLaunchKernelGGL(probe_spin_kernel, dim3(256), dim3(64), 40960, st, 10u, (unsigned int*)nullptr);
    hipLaunchKernelGGL(probe_tick_kernel, dim3(1), dim3(64), 0, st, (unsigned int*)nullptr);
    HIP_TRY(c, hipGetLastError(), "stream probe");
    HIP_TRY(c, hipStreamSynchronize(st), "sync");
    c->probe_warm = true;
    return GRK_AMD_OK;
}
} // namespace

// *cur, or a stream made now with *cur's priority, whose kernels are dispatched side by side with every stream of `against` (both
// directions); *cur is replaced (and destroyed) when a better one is found within eight tries, else kept.  All streams idle on entry.
int vetted_stream(grk_amd_ctx* c, hipStream_t* cur, const std::vector<hipStream_t>& against, int* replaced)
{
    int rc = probe_warmup(c, *cur); if (rc) return rc;
    int prio = 0;
    if (hipStreamGetPriority(*cur, &prio) != hipSuccess) { (void)hipGetLastError(); prio = 0; }
    std::vector<hipStream_t> rejects;
    hipStream_t cand = *cur;
    for (int tries = 0; tries < 9; ++tries) {
        bool ok = true;
        for (hipStream_t a : against) {
            if (!a || a == cand) continue;
            rc = streams_side_by_side(c, a, cand, &ok);
            if (rc == GRK_AMD_OK && ok) rc = streams_side_by_side(c, cand, a, &ok);
            if (rc || !ok) break;
        }
        if (rc) break;
        if (ok) { if (cand != *cur) { rejects.push_back(*cur); *cur = cand; if (replaced) ++*replaced; } cand = nullptr; break; }
        if (cand != *cur) rejects.push_back(cand);
        cand = nullptr;
        if (tries == 8 || hipStreamCreateWithPriority(&cand, hipStreamNonBlocking, prio) != hipSuccess) { (void)hipGetLastError(); cand = nullptr; break; }
    }
    if (cand && cand != *cur) rejects.push_back(cand);
    for (hipStream_t r : rejects) (void)hipStreamDestroy(r);
    return rc;
}

int probe_streams(grk_amd_ctx* c)
{
    if (!c->stream_probe || c->probed_main == c->stream || !c->side) return GRK_AMD_OK;
    c->probed_main = c->stream;
    for (hipStream_t seen : c->probed_before) if (seen == c->stream) return GRK_AMD_OK;
    for (int i = 3; i > 0; --i) c->probed_before[i] = c->probed_before[i - 1];
    c->probed_before[0] = c->stream;
    HIP_TRY(c, hipStreamSynchronize(c->stream), "sync");
    HIP_TRY(c, hipStreamSynchronize(c->side), "sync");
    if (c->side2) HIP_TRY(c, hipStreamSynchronize(c->side2), "sync");
    c->side_pending = false;
    { const int wr = probe_warmup(c, c->stream); if (wr) return wr; }
    std::vector<hipStream_t> rejects;                  // kept alive until the end: a stream made now gets another queue than these
    auto good = [&](hipStream_t cand, hipStream_t other, bool* ok) -> int {
        bool y = false;
        int rc = streams_side_by_side(c, c->stream, cand, &y); if (rc) return rc;
        if (y) { rc = streams_side_by_side(c, cand, c->stream, &y); if (rc) return rc; }
        if (y && other) { rc = streams_side_by_side(c, other, cand, &y); if (rc) return rc; }
        if (y && other) { rc = streams_side_by_side(c, cand, other, &y); if (rc) return rc; }
        *ok = y;
        return GRK_AMD_OK;
    };
    int rc = GRK_AMD_OK;
    for (int which = 0; which < 2 && rc == GRK_AMD_OK; ++which) {
        hipStream_t& mine = which ? c->side2 : c->side;
        if (!mine) continue;
        hipStream_t other = which ? c->side : nullptr;
        bool ok = false;
        rc = good(mine, other, &ok);
        for (int tries = 0; rc == GRK_AMD_OK && !ok && tries < 8; ++tries) {
            hipStream_t cand = nullptr;
            if (hipStreamCreateWithPriority(&cand, hipStreamNonBlocking, c->side_priority) != hipSuccess) { (void)hipGetLastError(); break; }
            rc = good(cand, other, &ok);
            if (rc == GRK_AMD_OK && ok) { rejects.push_back(mine); mine = cand; ++c->probe_replaced; }
            else rejects.push_back(cand);
        }
        // (none found: the stream stays as it was)
    }
    for (hipStream_t r : rejects) (void)hipStreamDestroy(r);
    return rc;
}

// everything that reads or overwrites the results of the latest encode on the main stream comes after its side streams
int join_side(grk_amd_ctx* c)
{
    if (!c->side_pending) return GRK_AMD_OK;
    HIP_TRY(c, hipStreamWaitEvent(c->stream, c->ev_side, 0), "join side stream");
    HIP_TRY(c, hipStreamWaitEvent(c->stream, c->ev_side2, 0), "join side stream 2");
    c->side_pending = false;
    return GRK_AMD_OK;
}

// The two streams of one of a sequence's contexts, made for the kind of frames the sequence carries.  The HIP runtime keeps a pool
// of (by default 4) hardware queues PER PRIORITY LEVEL, and kernels of streams that share a queue run one after the other.
// Part-1 frames are two long kernels each (the long chains on the call's stream, the lane kernel on the side stream, ~13 ms
// both): their streams go over the priority levels in turn, so that n frames in flight use the queues of every pool -- three
// frames in flight 10.4 -> 7.4 ms per frame, six 6.8, eight 6.4, with the default hardware-queue count (profiles/r04_hw_queues.txt).  The HT
// decoder's kernels are short and lose with streams of mixed priority (0.74 -> 0.86 ms per frame): plain streams for those.
// A sequence that changes its kind of frames pays one synchronisation per context.
int sequence_streams(grk_amd_ctx* k, bool part1)
{
    const int flavour = part1 ? 1 : 0;
    if (k->seq_index < 0 || k->seq_flavour == flavour || !k->own_stream) return GRK_AMD_OK;
    int least = 0, greatest = 0;
    (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
    const int levels = least - greatest + 1;
    if (levels < 2) { k->seq_flavour = flavour; return GRK_AMD_OK; }
    const int rc = grk_amd_synchronize(k); if (rc) return rc;
    hipStream_t ns = nullptr, nside = nullptr;
    const int p0 = part1 ? greatest + k->seq_index % levels : least, p1 = part1 ? greatest + (k->seq_index + 1) % levels : least;
    hipError_t e = part1 ? hipStreamCreateWithPriority(&ns, hipStreamNonBlocking, p0) : hipStreamCreateWithFlags(&ns, hipStreamNonBlocking);
    if (e == hipSuccess && k->side) e = hipStreamCreateWithPriority(&nside, hipStreamNonBlocking, p1);
    if (e != hipSuccess) { if (ns) (void)hipStreamDestroy(ns); return fail(k, GRK_AMD_ERR_NO_DEVICE, "streams of a decode sequence", e); }
    (void)hipStreamDestroy(k->stream); k->stream = ns;
    if (k->side) { (void)hipStreamDestroy(k->side); k->side = nside; }
    k->seq_flavour = flavour; k->seq_vetted = false;
    return GRK_AMD_OK;
}

extern "C" {
// The probe for a host's own streams (an exchange's stream that waits for the encoder's results holds its dispatch pipe while it waits:
// it must not share the main stream's): 1 when kernels of `a` and `b` are dispatched side by side, in both directions; 0 when one
// waits for the other's grid.  Both streams are synchronised.
int grk_amd_streams_side_by_side(grk_amd_ctx* c, void* a, void* b)
{
    if (!c || !a || !b || a == b) return GRK_AMD_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device), "set device");
    HIP_TRY(c, hipStreamSynchronize((hipStream_t)a), "sync");
    HIP_TRY(c, hipStreamSynchronize((hipStream_t)b), "sync");
    { const int wr = probe_warmup(c, (hipStream_t)a); if (wr) return wr; }
    bool y = false;
    int rc = streams_side_by_side(c, (hipStream_t)a, (hipStream_t)b, &y); if (rc) return rc;
    if (y) { rc = streams_side_by_side(c, (hipStream_t)b, (hipStream_t)a, &y); if (rc) return rc; }
    return y ? 1 : 0;
}
// the context's streams as they are now: 0 the main stream (grk_amd_set_stream's, or its own), 1 / 2 the side streams
void* grk_amd_internal_stream(grk_amd_ctx* c, int which) { return !c ? nullptr : which == 0 ? (void*)c->stream : which == 1 ? (void*)c->side : which == 2 ? (void*)c->side2 : nullptr; }
// the context's own probe now (it runs by itself before the first pipelined encode on a main stream)
int grk_amd_probe_streams(grk_amd_ctx* c)
{
    if (!c) return GRK_AMD_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device), "set device");
    { const int jr = join_side(c); if (jr) return jr; }
    return probe_streams(c);
}

// side streams the probe has replaced so far (-1: the probe is switched off)
int grk_amd_stream_probe_result(grk_amd_ctx* c) { return !c ? GRK_AMD_ERR_INVALID : c->stream_probe ? c->probe_replaced : -1; }
} // extern "C"
