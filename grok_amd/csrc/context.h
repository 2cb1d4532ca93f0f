// grok_amd/csrc/context.h -- the context behind include/grok_amd.h and the helpers its sources share (private to the library).
// One grk_amd_ctx per process per GPU.  All device memory is owned by the context and grows monotonically (288 GB of HBM3E:
// an 8K x 8K x 3 tile needs ~3.6 GB of working planes, a batch of 256 1024^2 tiles ~12 GB), so steady-state encode calls
// perform no allocation and enqueue nothing but kernels on one HIP stream.
#pragma once
#include "../../include/grok_amd.h"
#include "geometry.h"
#include "kernels.h"
#include "pixel_layout.h"
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include <algorithm>
#include <cmath>
#include <atomic>
#include <thread>

using namespace grk_amd;

#pragma GCC visibility push(hidden)       // nothing declared below is part of the library's interface
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    hipError_t ensure(size_t n)
    {
        if (n <= cap) return hipSuccess;
        if (p) { hipError_t e = hipFree(p); if (e != hipSuccess) return e; p = nullptr; cap = 0; }
        size_t want = n + (n >> 3) + 4096;
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) { p = nullptr; return e; }
        cap = want;
        return hipSuccess;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};

struct Timer {
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev;
    double total_ms = 0; uint32_t launches = 0;
};

// Pinned staging for the host-pointer entry points (pixels in, coded bytes / pixels out).  A buffer that IS pinned
// (grk_amd_host_alloc, hipHostMalloc, a pinned torch tensor) goes over the link as it lies -- one DMA at the link's rate.
// Pageable memory is moved through context-owned pinned chunks by kLanes copy threads, each double-buffered on its own
// stream (a memcpy into / out of one chunk while the other chunk's DMA runs): the threads' memcpy rate adds up, where one
// thread -- what a plain hipMemcpy of pageable memory amounts to -- is the limit otherwise.
struct HostStage {
    static constexpr size_t kChunk = 8u << 20;
    static constexpr int kLanes = 4;
    void* buf[kLanes][2] = {};
    hipEvent_t ev[kLanes][2] = {};
    hipEvent_t ev_in = nullptr, ev_out[kLanes] = {};
    hipStream_t st[kLanes] = {};
    bool ready = false;
    hipError_t ensure()
    {
        if (ready) return hipSuccess;
        hipError_t e = hipEventCreateWithFlags(&ev_in, hipEventDisableTiming);
        for (int t = 0; t < kLanes && e == hipSuccess; ++t) {
            e = hipStreamCreateWithFlags(&st[t], hipStreamNonBlocking);
            if (e == hipSuccess) e = hipEventCreateWithFlags(&ev_out[t], hipEventDisableTiming);
            for (int k = 0; k < 2 && e == hipSuccess; ++k) {
                e = hipHostMalloc(&buf[t][k], kChunk, hipHostMallocDefault);
                if (e == hipSuccess) e = hipEventCreateWithFlags(&ev[t][k], hipEventDisableTiming);
            }
        }
        ready = e == hipSuccess;
        return e;
    }
    void release()
    {
        for (int t = 0; t < kLanes; ++t) {
            if (st[t]) { (void)hipStreamSynchronize(st[t]); (void)hipStreamDestroy(st[t]); st[t] = nullptr; }
            if (ev_out[t]) { (void)hipEventDestroy(ev_out[t]); ev_out[t] = nullptr; }
            for (int k = 0; k < 2; ++k) {
                if (buf[t][k]) { (void)hipHostFree(buf[t][k]); buf[t][k] = nullptr; }
                if (ev[t][k]) { (void)hipEventDestroy(ev[t][k]); ev[t][k] = nullptr; }
            }
        }
        if (ev_in) { (void)hipEventDestroy(ev_in); ev_in = nullptr; }
        ready = false;
    }
};

struct grk_amd_ctx {
    int device = 0;
    int verbose = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    std::string err;
    // working set
    DevBuf pixels, p0, p1, llA, llB, blockdesc, lengths, offsets, arena, flag;
    DevBuf dec_desc, dec_table, dec_quads, dec_mslen, dec_coded, dec_pixels, dec_work;
    // geometry cache
    grk_amd_tile_params gp{};
    bool have_geom = false;
    TileGeom geom;
    std::vector<HtBlockDesc> h_desc, h_desc_dec;
    std::vector<uint16_t> dec_qcd;                          // decode: QCD words of a foreign stream (optional)
    std::vector<float> dec_steps;                           // decode: band step sizes as the host holds them (optional), [comp][band]
    std::vector<uint32_t> dec_seg_first;                    // Part-1 decode: codeword segments (optional), [nblocks + 1]
    std::vector<grk_amd_segment> dec_segs;
    grk_amd_pixel_layout enc_layout{};                      // the pixels an encode reads (grk_amd_set_pixel_layout; all zero: the default)
    grk_amd_pixel_layout dec_layout{};                      // the pixels a decode writes (grk_amd_set_decode_pixel_layout)
    bool dec_upsample = false;                              // grk_amd_decode_image delivers sub-sampled components at W x H (grk_amd_set_decode_upsample)
    uint32_t dec_reduce = 0;                                // decode at 1 / 2^dec_reduce of the size (grk_amd_set_decode_reduce)
    std::vector<uint32_t> red_seg_first;                    // ... the segment list of the blocks that decode keeps (decode_impl, decode.hip)
    std::vector<grk_amd_segment> red_segs;
    DevBuf dec_seg_dev;
    std::vector<HtClassPlan> ht_classes;      // block classes of K3 (plan_ht_classes, encode_plan.h); their lists lie in ht_sel
    int seq_index = -1;               // >= 0: one of a decode sequence's internal contexts (grk_amd_set_decode_pipelining)
    int seq_flavour = 0;              // ... whose two streams are made for 0: HT frames, 1: Part-1 frames (sequence_streams)
    hipStream_t side2 = nullptr; hipEvent_t ev_side2 = nullptr;      // the large-LDS classes run beside the small-LDS ones
    hipStream_t side = nullptr;                             // K3 of the top resolution runs here beside DWT levels >= 1
    hipEvent_t ev_level0 = nullptr, ev_side = nullptr;
    bool overlap = false;
    // Pipelining of consecutive encodes (grk_amd_set_pipelining): a second set of per-encode buffers, so that the next
    // encode's DWT can start while the side streams still code the blocks of this one
    static constexpr int kMaxAltSets = 7;
    struct AltSet { DevBuf p1, arena, lengths, offsets, flag, ovf, llA, llB; hipEvent_t ev_side = nullptr, ev_side2 = nullptr; } alts[kMaxAltSets];
    int alt_head = 0;                // the OLDEST of the sets not in use (a ring: the set a call retires becomes the newest)
    int pipe_depth = 2;              // buffer sets in rotation when pipelining: grk_amd_set_pipelining(ctx, n) -> n + 1 of them (2 ..
                                     // 8): the results of a call then stay valid until the (n + 1)-th next call
    DevBuf ovf;                      // K3: blocks handed to the fallback launch (kernels.h: HtArgs::ovf_list)
    bool lds_cap = true;             // K3 with capped LDS buffers + fallback launch (GRK_AMD_LDS_CAP=0: worst-case buffers)
    bool pipelining = false;
    hipEvent_t ev_main = nullptr;
    bool side_pending = false;       // side-stream work of the latest encode has not been joined on the main stream yet
    bool dec_planes16 = true;                               // 16-bit planes between K5b and K6 for 8-bit reversible HT tiles
                                                            // (GRK_AMD_DEC_PLANES16=0 / grk_amd_set_decode_planes16: int32)
    int dwt_pk = 1;                                         // packed int16 pairs in K2 / K6 where the range allows (GRK_AMD_DWT_PK=0: 32-bit)
    int dwt_pair = 1;                                       // levels 0 and 1 of the packed 5/3 encoder in one launch where plan_dwt_pair has one (GRK_AMD_DWT_PAIR=0: level by level)
    bool k3_alternate = true;                               // pipelined encodes: K3's classes on the two side streams in turn (GRK_AMD_K3_ALT=0: fixed)
    uint32_t num_cus = 0;                                   // compute units of the device (0: not known)
    uint32_t k3_parity = 0;                                 // ... which way round this frame; flips per pipelined encode, grk_amd_set_pipelining resets it
    int dwt_xcd = 1;                                        // XCD-aware workgroup order in K2 / K6 (GRK_AMD_DWT_XCD=0: plain)
    bool fuse_egress = true;                                // K7 inside the last inverse DWT level (GRK_AMD_FUSE_EGRESS=0: separate)
    bool planes16 = true;                                   // int16 planes between K2 and K3 where the range allows (GRK_AMD_PLANES16=0: never)
    DevBuf ht_sel;
    DevBuf energy;                   // grk_amd_block_distortion: sum of q^2 per block
    // Tier-2 on the device (grk_amd_assemble_device): the packets of the geometry in the order last asked for, scratch, and the
    // finished tile-parts
    struct T2State {
        bool valid = false; grk_amd_tile_params p{}; uint32_t order = 0;
        uint32_t tp = 0;                                     // the division into tile-parts the plan's part_starts were made for (GRK_AMD_CS_TP's letter)
        bool msbs = false;                                   // the plan of the general zero-bit-plane tree (t2_device_plan_msbs)
        T2Plan plan; uint32_t max_blocks = 0;
        DevBuf packets, pob;
    } t2;
    DevBuf t2_u, t2_h, t2_rel, t2_pkhdr, t2_pkbody, t2_pkdst, t2_lit, t2_litlen, t2_index;      // scratch: ONE stream at a time uses it
    DevBuf t2_nodes;                                         // ... the general zero-bit-plane tree's node values (T2Plan::v_bytes per tile)
    DevBuf t2_parts; std::vector<T2Part> t2_parts_host;      // ... a divided call's tile-parts (kernels.h: T2Part), the same for every tile of the call
    // the finished tile-parts, their places and lengths ([tile]: uint64 / uint32) and {bytes assembled by the call, end of the output};
    // the asynchronous form rotates as many of these as the encoder rotates buffer sets, so that a frame's tile-parts stay where they
    // are while an exchange sends them
    // (a call whose tiles are divided into tile-parts: tile_dst / part_len are the tiles' spans, tp_dst / tp_len [tile][part] the parts')
    struct T2Out { DevBuf out, tile_dst, part_len, total, tp_len, tp_dst; uint32_t nparts = 1; };
    T2Out t2_outs[kMaxAltSets + 1];
    int t2_cur = 0;
    uint64_t t2_out_used = 0;        // (the synchronous form) bytes of t2_outs[t2_cur].out that hold tile-parts
    // Tier-2 on the device over JOINT tables (assemble.hip: encode_joint_device -- sub-sampled images, surfaces, packed frames): the
    // plans of the image's tile classes, cached apart from `t2` (keyed on the image, not on a plain call's parameters: neither
    // serves the other), the image-wide tables and arena that KK (kernels_t2keep.hip) fills batch after batch, the running cursors
    // (uint64[batches + 1]) with the image's status word behind them, the units' first rows batch by batch, and the file of a
    // grk_amd_encode_*_device call whose tile classes do not lie in tile order
    struct T2Joint {
        bool valid = false; grk_amd_image_layout im{}; grk_amd_tile_params base{}; std::vector<uint8_t> dx, dy; uint32_t order = 0, tp = 0;
        bool msbs = false;                                   // the classes' plans are those of the general zero-bit-plane tree
        struct Class { T2Plan plan; uint32_t max_blocks = 0, bpt = 0; uint64_t row_begin = 0; std::vector<uint32_t> tiles; DevBuf packets, pob; };
        std::vector<Class> classes;
        std::vector<uint64_t> unit_row;                      // [unit]: its first row in the image's tables (class-major, see assemble.hip)
        uint64_t rows = 0;
    } t2j;
    DevBuf jt_len, jt_off, jt_arena, jt_state, jt_rowat, jt_file, jt_msbs;
    DevBuf st_len, st_off, st_arena, st_status;              // grk_amd_stage_assemble: the caller's rows and coded bytes, the call's status word
    DevBuf st_msbs;                                          // grk_amd_stage_assemble_msbs: the rows' missing_msbs, a byte each
    DevBuf st_rL, st_rE, st_rW, st_rdrop, st_rres, st_rmap;  // grk_amd_stage_rate_stats / _alloc: the caller's tables, apart from rate_*
    uint64_t rate_dev_counters[2] = {0, 0};                // the latest rate- / quality-targeted _device call: Tier-2 passes on the device, coded bytes fetched
    uint64_t route_counters[2] = {0, 0};                   // images assembled on the device / written by the host writer (grk_amd_encode_route_counters)
    uint64_t last_arena_bound = 0;                           // the arena K3's plan asked for in the latest call (plan_ht_arena), <= arena.cap
    std::vector<uint64_t> h_off;
    std::vector<uint32_t> h_len;
    uint32_t last_ntiles = 0;
    uint64_t last_nblocks = 0;
    bool last_h16 = false;           // the latest encode left int16 coefficients in the Mallat planes
    const uint8_t* last_drops = nullptr;   // the latest K3 launch took per-block drops: the context's copy of them (drops_keep, [last_nblocks]),
    DevBuf drops_keep;                     // from which grk_amd_fetch_table makes the rows' zero bit-planes
    // A rate- or quality-targeted encode (rate.hip, RateRun): the tables over the blocks of the run's units in the run's row order --
    // L, E candidate-major (RatePlan), W, the chosen drop bytes, the allocator's result -- and what they were made for; unit_rows:
    // each unit's first row.  A run over several batches also holds the batches' maps in rate_map (RateJointPlan) and the drop
    // bytes of the batch being coded in rate_bdrop; an identity run (one batch in row order) uses neither.
    DevBuf rate_L, rate_E, rate_W, rate_drop, rate_res, rate_map, rate_bdrop;
    struct RateState { bool valid = false; RatePlan plan{}; uint64_t nblocks = 0; std::vector<uint64_t> unit_rows;
                       uint64_t budget = 0; /* of the latest allocator run (0: that was KQ) */
                       double qbudget = 0; /* the distortion budget of the latest run of KQ (0: that was KR2) */ } rate;
    HostStage stage;                 // pinned chunks for pageable host buffers (copy_h2d)
    void* d2h_pin = nullptr; size_t d2h_cap = 0; std::vector<hipEvent_t> d2h_ev;   // copy_d2h: a staging area of the transfer's size, an event per piece
    // Full decode with overlap on: K5b of the top resolution's blocks (3/4 of them) runs on the side stream beside K5b of the
    // other blocks and the inverse levels that need only those; the last inverse level waits for it
    hipEvent_t ev_dec_front = nullptr, ev_dec_top = nullptr;
    bool dec_top_pending = false;
    // Pipelined encodes of small frames run a frame's whole chain on ONE of the two side streams, taken in turn (encode_constants.h:
    // kFrameStreamSamples; GRK_AMD_FRAME_STREAMS = 0: never, 1 (default): by size, 2: always)
    int frame_streams = 1; int fs_parity = 0;
    // ... the caller's pixels are then read on the frame's stream, not on the context's: level 0 -- their only reader -- is followed by
    // this event, and the context's stream waits for it, so that whatever the caller queues behind the call in stream order (the
    // next frame's pixels into the same buffer, a stream-ordered free) still comes after the read, as it does on the other paths
    // (grk_amd_set_pixel_hold(ctx, 1): the caller keeps a call's pixels untouched until grk_amd_stream_wait_pixels / a synchronisation;
    //  the wait -- two queue hand-overs between consecutive small frames, 0.038 -> 0.057 ms per 512^2 call -- is then left out)
    hipEvent_t ev_px = nullptr; bool want_px_event = false; bool px_hold = false; bool px_event_valid = false;
    // The encoder's three streams have to DISPATCH side by side.  Hardware queues are served by a few dispatch pipes; two queues on one
    // pipe take turns while one of them has a large grid in flight, and which queue a stream gets depends on how many streams the process
    // made before (profiles/r06_hw_queues.txt: 0.37 -> 0.55 ms per 8K frame with 4, 5 or 8 earlier streams).  Before the first
    // overlapped encode on a given main stream the three are probed pairwise (a grid that stays in dispatch for ~150 us on one, a
    // one-workgroup kernel on the other) and a side stream that has to wait is replaced (GRK_AMD_STREAM_PROBE=0: never)
    int stream_probe = 1; hipStream_t probed_main = nullptr; int side_priority = 0;
    hipStream_t probed_before[4] = {};   // main streams probed earlier: a host that alternates between a few streams is not probed at every switch
    int probe_replaced = 0;           // side streams replaced by the probe so far (grk_amd_stream_probe_result)
    bool probe_warm = false;          // the probe's kernels have been launched once (their first launch loads their code: not to be measured)
    bool seq_vetted = false;          // (a sequence's internal context) its streams have been vetted against its neighbours' (vet_sequence_streams, decode_sequence.hip)
    unsigned long long* pend_alloc = nullptr; uint32_t pend_alloc_units = 0;   // K3's allocator reset handed to the fused level 0 (run_dwt)
    // Decode of a SEQUENCE of frames (grk_amd_set_decode_pipelining): consecutive grk_amd_decode_tiles calls with device buffers
    // go in turn to this context and to `dec_kids` -- contexts of their own on the same device: own streams, tables, planes --,
    // each behind an event on the caller's stream.  A frame's serial block-decoding chains (K5a / K8) leave most of the machine
    // idle; the next frame's kernels take what is free.  grk_amd_synchronize / grk_amd_decode_status cover them all.
    std::vector<grk_amd_ctx*> dec_kids;
    uint32_t dec_seq = 0;
    hipEvent_t ev_seq = nullptr;
    hipEvent_t ev_frame_done = nullptr;   // (an internal context of a sequence) behind the last frame it was given: grk_amd_decode_stream_wait_slot
    // Part-1 decode: blocks of the default style go 64 to a wave (K8L, kernels_t1lanes.hip) unless much longer than the rest
    // (GRK_AMD_T1_LANES=0: every block its own wave, K8 as in r01-r03; 2: lanes wherever they can be used; see plan_t1_lists,
    // decode_plan.cpp)
    int t1_lanes = 1;                    // 0: never, 1: where the cost model there says they are faster, 2: wherever they can (tests)
    bool t1_pass_sync = true;            // K8L's waves hold blocks of equal bit-plane / pass counts and run pass by pass (GRK_AMD_T1_SYNC=0: free-running lanes)
    // A decode call's tables -- the code-block rows (a window's skipped blocks marked), behind them the launch lists of the block
    // decoders (decode_blocks.hip) -- are put together in pinned memory the context owns and fetched by a kernel of the call's stream
    // (launch_dec_upload); two sets in turn: the kernel of one call may still be queued when the next call fills its tables
    struct DecUpload { char* p = nullptr; char* dp = nullptr; size_t cap = 0; hipEvent_t ev = nullptr; } dec_up[2];
    uint32_t dec_turn = 0;
    // grk_amd_decode_image: the uploaded codestream + appendix, a group's decoded tiles, the image (host pixels), the gather's
    // moves, the tiles' places, the status of all groups; launches of the gather / placement kernels so far
    DevBuf img_coded, img_tiles, img_pixels, img_moves, img_rects, img_status;
    uint64_t img_launches[2] = {0, 0};
    uint64_t img_counters[2] = {0, 0};                      // tiles read, codestream bytes uploaded (grk_amd_decode_image_counters)
    // grk_amd_encode_surface / grk_amd_decode_surface share those buffers: img_pixels a host surface's copy, img_tiles a group's staged
    // units, img_rects the units' origins; units handled in place, units staged, launches of KS + KD (grk_amd_surface_counters)
    uint64_t surf_counters[3] = {0, 0, 0};
    // grk_amd_encode_packed / grk_amd_decode_packed (packed.cpp): the frame's three tight planes, each from a 256-byte boundary -- the
    // device surface that the surface calls above then work on; a host frame's copy lies in img_pixels; launches of KU, of KK
    DevBuf img_planes;
    uint64_t packed_counters[2] = {0, 0};
    // grk_amd_read_packets_device / grk_amd_decode_image_device (read_device.hip): the plan kept for the latest stream header, its
    // descriptors and scratch on the device, the header's pinned copy, the counters -- made by the first such call
    struct ReadDevState* rdev = nullptr;
    // timing
    bool timing = false;
    Timer timers[10];
};

int fail(grk_amd_ctx* c, int code, const char* what, hipError_t e = hipSuccess);                                 // context.hip
#define HIP_TRY(c, call, what)                                                      \
    do { hipError_t _e = (call); if (_e != hipSuccess) return fail(c, GRK_AMD_ERR_NO_DEVICE, what, _e); } while (0)

struct ScopedTimer {
    grk_amd_ctx* c; int which; hipEvent_t a = nullptr, b = nullptr;
    hipStream_t st;
    ScopedTimer(grk_amd_ctx* c_, int w, hipStream_t s = nullptr) : c(c_), which(w), st(s ? s : c_->stream)
    {
        if (!c->timing) return;
        if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) { a = b = nullptr; return; }
        (void)hipEventRecord(a, st);
    }
    void cancel() { if (a) { (void)hipEventDestroy(a); (void)hipEventDestroy(b); a = b = nullptr; } }
    ~ScopedTimer()
    {
        if (!a) return;
        (void)hipEventRecord(b, st);
        c->timers[which].ev.emplace_back(a, b);
    }
};

inline uint32_t ll_stride_for(uint32_t w) { return (((w + 1) >> 1) + 31u) & ~31u; }
int create_context(int device_id, int verbose, bool decode_only, grk_amd_ctx** out);                             // context.hip
bool host_is_pinned(const void* p);                                                                              // context.hip
int copy_h2d(grk_amd_ctx* c, void* dst, const void* src, size_t bytes);                                          // context.hip
int copy_d2h(grk_amd_ctx* c, void* dst, const void* src, size_t bytes);                                          // context.hip
bool same_params(const grk_amd_tile_params& a, const grk_amd_tile_params& b);                                    // context.hip
int ensure_geom(grk_amd_ctx* c, const grk_amd_tile_params* p, uint32_t reduce = 0);                              // context.hip
int probe_streams(grk_amd_ctx* c);                                                                               // streams.hip
int vetted_stream(grk_amd_ctx* c, hipStream_t* cur, const std::vector<hipStream_t>& against, int* replaced);     // streams.hip
int join_side(grk_amd_ctx* c);                                                                                   // streams.hip
int sequence_streams(grk_amd_ctx* k, bool part1);                                                                // streams.hip

// KS (place = false) or KD for `count` units of w x h samples of one run, tight at d_tiles, their origins (device memory) at
// d_origins; the surface's first byte at d_surface (surface.cpp).  The caller checked the surface against its buffer
namespace grk_amd { struct ResolvedSurface; struct CompRun; struct QualityGoal; }
int queue_surface_kernel(grk_amd_ctx* c, bool place, const grk_amd::ResolvedSurface& rs, const grk_amd::CompRun& run, void* d_surface,
                         void* d_tiles, uint32_t count, uint32_t w, uint32_t h, const uint32_t* d_origins);                  // surface.cpp
bool surface_direct_allowed();            // GRK_AMD_SURFACE_DIRECT != 0, read per call (surface.cpp)
// grk_amd_encode_surface / grk_amd_encode_surface_rate behind their null checks: what the packed calls (packed.cpp) enter too
// (d_file != nullptr: grk_amd_encode_surface_device -- the file stays in device memory, `out` / `out_cap` are not used)
int64_t encode_surface_job(grk_amd_ctx* c, const grk_amd_image_layout* im, const grk_amd_tile_params* base, const uint8_t* comp_dx,
                           const uint8_t* comp_dy, const grk_amd_surface* surface, const void* pixels, uint64_t cap, int pixels_on_device,
                           uint32_t flags, uint8_t* out, uint64_t out_cap, void** d_file = nullptr);                        // surface.cpp
int64_t encode_surface_rate_job(grk_amd_ctx* c, const grk_amd_image_layout* im, const grk_amd_tile_params* base, const uint8_t* comp_dx,
                                const uint8_t* comp_dy, const grk_amd_surface* surface, const void* pixels, uint64_t cap, int pixels_on_device,
                                uint32_t flags, const grk_amd_rate* rate, uint8_t* out, uint64_t out_cap, grk_amd_rate_result* result,
                                const grk_amd::QualityGoal* quality = nullptr, void** d_file = nullptr);   // surface.cpp (quality: image.h,
                                // RateJointCall; d_file != nullptr: the _device twins -- Tier-2 on the device, `out` / `out_cap` are not used)
// grk_amd_decode_surface behind its null checks (`name`: the entry point, for a refusal's text); host_rules: a device surface under
// the rules of a host destination -- a group that leaves the int16 planes is repeated by the call itself
int decode_onto_surface(grk_amd_ctx* c, const char* name, const uint8_t* cs, uint64_t len, const grk_amd_surface* surface, void* pixels,
                        uint64_t cap, int pixels_on_device, bool host_rules);                                                 // decode_image.cpp
// grk_amd_decode_image for a codestream that IS the coded buffer already (d_cs, device memory) and whose header and rows the device
// reader has made (read_device.hip): decode_view's way in for "coded bytes resident, table given"; `tab` is consumed
namespace grk_amd { struct StreamTable; }
int decode_resident(grk_amd_ctx* c, const void* d_cs, uint64_t len, const grk_amd_stream_info& info, grk_amd::StreamTable& tab, void* pixels,
                    uint64_t cap, int pixels_on_device);                                                                      // decode_image.cpp
// ... and for a table with an appendix (tab.appendix_bytes; the general reader's): the moves lie in device memory where the reader's
// placement kernel left them (tab.moves is empty), the stream is staged in front of its appendix in the context's coded buffer --
// one device-to-device copy of `len` bytes, added to *staged -- and d_cs is only read
int decode_resident_moves(grk_amd_ctx* c, const void* d_cs, uint64_t len, const grk_amd_stream_info& info, grk_amd::StreamTable& tab,
                          const grk_amd_tp_segment* d_moves, uint64_t num_moves, uint64_t* staged, void* pixels, uint64_t cap,
                          int pixels_on_device);                                                                              // decode_image.cpp
void read_device_release(grk_amd_ctx* c);                                                                                     // read_device.hip
// what the whole-image decodes refuse on the context: a decode reduce (`reduced`: the text behind the entry point's name), a decode sequence
int refuse_context(grk_amd_ctx* c, const char* name, const char* reduced);                                                    // decode_image.cpp

// a pixel layout of the context that a call sets for its own batches, put back when the call ends (KeepLayout keep{slot, slot};)
struct KeepLayout { grk_amd_pixel_layout& slot; grk_amd_pixel_layout keep; ~KeepLayout() { slot = keep; } };

// ---- what a rate-targeted encode takes from encode.hip ----
// K3 of `ntiles` tiles of the current geometry from the planes at d_mallat (int16 when h16) through the instances that take a
// per-block drop (d_drops: device, tile-major in table order, read in stream order; the context keeps a copy for the table)
int ht_encode_drops(grk_amd_ctx* c, uint32_t ntiles, const void* d_mallat, bool h16, const uint8_t* d_drops);               // encode.hip
// w_mct * w_band * stepsize of row `row` of a tile's block table (T1::getwmsedec; grk_amd_block_distortion)
double block_weight(const TileGeom& g, uint32_t row);                                                                       // encode.hip
// An allocator's arguments over tables on the device (rate_*, a stage call's st_r*): RateAllocArgs (KR2) and RateQualityArgs (KQ)
template <class Args, class Budget>
inline Args rate_alloc_args(const DevBuf& L, const DevBuf& E, const DevBuf& W, const DevBuf& drop, const DevBuf& res, uint64_t nblocks, uint32_t dmax, uint32_t ncand, Budget budget)
{
    Args a{};
    a.L = (const uint32_t*)L.p; a.E = (const unsigned long long*)E.p; a.W = (const double*)W.p;
    a.nblocks = nblocks; a.dmax = dmax; a.ncand = ncand; a.budget = budget;
    a.drop = (uint8_t*)drop.p; a.res = (decltype(a.res))res.p;
    return a;
}

// ---- steps the encode and decode units share ----
// The first steps of a grk_amd_stage_* entry point: the side streams joined (where the stage reads what they write), the null
// checks (args_ok: the stage's other arguments), a refusal the stage has for these parameters (refuse != nullptr), the device,
// the geometry
int stage_enter(grk_amd_ctx* c, const grk_amd_tile_params* p, bool args_ok, bool join, const char* refuse = nullptr);   // context.hip

// an event made when it is first needed
inline hipError_t ensure_event(hipEvent_t* ev) { return *ev ? hipSuccess : hipEventCreateWithFlags(ev, hipEventDisableTiming); }
// what `later` gets from here on comes after what `earlier` holds now
inline int order_behind(grk_amd_ctx* c, hipStream_t later, hipEvent_t ev, hipStream_t earlier, const char* what_record, const char* what_wait)
{
    HIP_TRY(c, hipEventRecord(ev, earlier), what_record);
    HIP_TRY(c, hipStreamWaitEvent(later, ev, 0), what_wait);
    return GRK_AMD_OK;
}

// DC shift, clamp range, the sign bit of a stored sample (signed samples, else 0) and the bytes a sample takes in the pixels
struct SampleRange { int32_t dc, lo, hi, sext; uint32_t bytes; };
inline SampleRange sample_range(const grk_amd_tile_params& p)
{
    SampleRange r;
    r.bytes = (p.prec + 7u) / 8u;
    r.dc = p.sgnd ? 0 : (1 << (p.prec - 1));
    r.lo = p.sgnd ? -(1 << (p.prec - 1)) : 0;
    r.hi = p.sgnd ? (1 << (p.prec - 1)) - 1 : (1 << p.prec) - 1;
    r.sext = p.sgnd ? (1 << (8 * r.bytes - 1)) : 0;
    return r;
}

// a resolved layout into a launcher's px_* fields: what a kernel that READS pixels takes (IngestArgs; DwtLevelArgs adds px_chan) ...
template <class Args> inline void set_px_in(Args& a, const PixelLayout& px)
{
    a.px_lay = px.lay; a.px_xstep = px.xstep; a.px_row = px.row; a.px_kstep = px.kstep; a.px_tile = px.tile;
}
// ... and one that WRITES them (IdwtLevelArgs, EgressArgs)
template <class Args> inline void set_px_out(Args& a, const PixelLayout& px)
{
    set_px_in(a, px); a.px_chan = px.channels; a.px_fill = px.fill;
}

// The LL ping-pong of a transform chain over the context's geometry, forward or inverse: LL_0 is the plane handed in or out,
// LL_L lives in the Mallat plane, and between them llA holds LL1, LL3, ..., llB holds LL2, LL4, ...
struct LLPlane { void* p; uint32_t stride; uint64_t pitch; };
inline LLPlane ll_pingpong(const grk_amd_ctx* c, bool odd)
{
    const uint32_t w = c->geom.p.tile_w, hA = (c->geom.p.tile_h + 1) >> 1;
    if (odd) return {c->llA.p, ll_stride_for(w), (uint64_t)ll_stride_for(w) * hA};
    return {c->llB.p, ll_stride_for((w + 1) >> 1), (uint64_t)ll_stride_for((w + 1) >> 1) * ((hA + 1) >> 1)};
}
inline LLPlane ll_plane(const grk_amd_ctx* c, uint32_t l, void* plane0, void* mallat)
{
    const TileGeom& g = c->geom;
    if (l == 0) return {plane0, g.stride, g.plane_elems};
    if (l == g.p.num_levels) return {mallat, g.stride, g.plane_elems};
    return ll_pingpong(c, (l & 1u) != 0);
}
// ... both buffers large enough for nplanes planes (before the first ll_plane: growing a buffer moves it)
inline int ensure_ll(grk_amd_ctx* c, uint32_t nplanes)
{
    HIP_TRY(c, c->llA.ensure((size_t)nplanes * ll_pingpong(c, true).pitch * 4 + 256), "alloc LL ping");
    HIP_TRY(c, c->llB.ensure((size_t)nplanes * ll_pingpong(c, false).pitch * 4 + 256), "alloc LL pong");
    return GRK_AMD_OK;
}

#pragma GCC visibility pop
