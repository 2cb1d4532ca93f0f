// grok_amd/csrc/kernels_t2read.hip -- Tier-2 READ on the device: a codestream that lies in device memory to the table of its
// code-blocks (grk_amd_read_packets_device; the parse itself: t2_parse.h, what a tile's packets are: t2_read_plan.h).
//   KL  locate     where each tile's one tile-part lies.  With TLM the host has the places (prefix sums of TLM's lengths) and one
//                  lane per tile-part checks its SOT; without, one lane hops along the Psot chain from the first SOT -- every
//                  hop checked against the stream's length, at most len / 14 of them --, then the lanes check the SOTs.  A tile
//                  named twice, an Isot beyond the grid, a tile without a tile-part are refusals.  One workgroup.
//   KH  headers    a workgroup per tile: the marker segments up to SOD one after the other (a handful), PLT's entries in
//                  parallel -- the terminator bytes flagged, a workgroup scan numbers them, each terminator's lane assembles
//                  its entry, a second scan makes packet starts of the lengths.
//   KC  chains     one wave (a workgroup of 64) per chain: with PLT a packet, without a tile's packets in file order.  The parse
//                  is serial, so its control flow is wave-uniform and every lane holds the same state (what a lane reads of the
//                  stream and the nodes is made uniform with readfirstlane: the state lives in scalar registers); the lanes
//                  fetch the stream a window at a time, clear the chain's tag-tree nodes and store rows 64 at a time.
// Refusals go to ONE 64-bit word with atomicMin (t2_parse.h: the status word); a wave that fails stops its own chain, nobody
// waits for anybody.  Plain C++: no inline assembly.
#define GRK_T2P_UNIFORM(v) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(v)))
#include "kernels.h"
#include "t2_parse.h"
#include "t2_read_plan.h"

namespace grk_amd {

namespace {

// the stream as one lane reads it, byte by byte (KL, KH: a handful of bytes per tile)
struct DirectSrc {
    const uint8_t* d;
    __device__ uint32_t byte(uint64_t i) const { return d[i]; }
};

__device__ __forceinline__ void report(unsigned long long* status, uint64_t word) { atomicMin(status, (unsigned long long)word); }

// inclusive scan of v over the workgroup's 256 threads; *total: the sum
__device__ uint64_t scan256(uint64_t v, uint64_t* lds, uint64_t* total)
{
    const uint32_t t = threadIdx.x;
    __syncthreads();
    lds[t] = v;
    __syncthreads();
    for (uint32_t d = 1; d < 256; d <<= 1) {
        const uint64_t add = t >= d ? lds[t - d] : 0;
        __syncthreads();
        lds[t] += add;
        __syncthreads();
    }
    *total = lds[255];
    return lds[t];
}

} // namespace

// ---- KL --------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void t2read_locate_kernel(T2ReadArgs a)
{
    __shared__ unsigned long long s_n;
    __shared__ uint32_t s_fail;
    const uint32_t tid = threadIdx.x, nt = a.num_tiles;
    DirectSrc src{a.cs};
    for (uint32_t t = tid; t < nt; t += 256) { a.first_of[t] = 0xFFFFFFFFu; a.part_len[t] = 0; a.part_at[t] = 0; }
    if (tid == 0) {
        s_fail = 0;
        if (a.tlm) s_n = a.tlm_count;
        else {
            // the Psot chain: the first nt tile-parts are kept (their places in part_at / part_len by FILE order for now: the
            // checks below sort them by tile), the others counted
            uint64_t at = a.sot_at, n = 0;
            const uint64_t max_hops = a.len / 14 + 1;
            for (uint64_t hop = 0; hop < max_hops; ++hop) {
                uint64_t l = 0;
                const int r = t2p_hop(src, a.len, at, &l);
                if (r == 0) break;
                if (r == 2) { s_fail = 1; break; }
                if (n < nt) { a.pk_start[n] = at; a.plt_len[n] = (uint32_t)l; }       // (scratch of at least nt entries: every tile has a packet)
                ++n; at += l;
            }
            if (n == 0) s_fail = 1;
            s_n = n;
        }
    }
    __threadfence_block();
    __syncthreads();
    if (s_fail) { if (tid == 0) report(a.status, t2p_status_locate(0, kT2pNotLocated)); return; }
    const uint64_t n_all = s_n;
    const uint32_t n = (uint32_t)(n_all < nt ? n_all : nt);
    // pass 1: every tile-part's SOT; the first tile-part that names a tile claims it
    for (uint32_t i = tid; i < n; i += 256) {
        const uint64_t at = a.tlm ? a.tlm[i].at : a.pk_start[i];
        const uint32_t ln = a.tlm ? a.tlm[i].ln : a.plt_len[i];
        uint32_t isot = 0xFFFFFFFFu;
        const uint32_t why = t2p_check_sot(src, a.len, at, ln, nt, a.tlm ? a.tlm[i].idx : 0xFFFFFFFFu, &isot);
        if (why != kT2pNoSot && why != kT2pTileIndex) atomicMin(&a.first_of[isot], i);
    }
    __threadfence_block();
    __syncthreads();
    for (uint32_t i = tid; i < n; i += 256) {
        const uint64_t at = a.tlm ? a.tlm[i].at : a.pk_start[i];
        const uint32_t ln = a.tlm ? a.tlm[i].ln : a.plt_len[i];
        uint32_t isot = 0xFFFFFFFFu;
        uint32_t why = t2p_check_sot(src, a.len, at, ln, nt, a.tlm ? a.tlm[i].idx : 0xFFFFFFFFu, &isot);
        if ((why == kT2pOk || why == kT2pPsotTlm) && __hip_atomic_load(&a.first_of[isot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < i) why = kT2pMultiPart;
        if (why) report(a.status, t2p_status_locate(i, why));
        else { a.part_at[isot] = at; a.part_len[isot] = ln; }
    }
    if (n_all > nt && tid == 0) report(a.status, t2p_status_locate(nt, kT2pManyParts));
    for (uint32_t t = tid; t < nt; t += 256)
        if (__hip_atomic_load(&a.first_of[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0xFFFFFFFFu) report(a.status, t2p_status_locate(nt + 1 + t, kT2pNoPart));
}

// ---- KH --------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void t2read_headers_kernel(T2ReadArgs a)
{
    __shared__ uint64_t s_scan[256];
    __shared__ int s_kind;
    __shared__ unsigned long long s_next, s_lo, s_hi;
    __shared__ uint32_t s_fail;
    const uint32_t t = blockIdx.x, tid = threadIdx.x;
    const uint32_t ln = a.part_len[t];
    if (tid == 0) { a.body_at[t] = 0; a.has_plt[t] = 0; }
    if (!ln) return;
    const T2ReadTile T = a.tiles[t];
    const uint64_t at = a.part_at[t], end = at + ln, npk = T.npackets;
    DirectSrc src{a.cs};
    uint64_t pos = at + 12, count = 0;
    bool have_plt = false;
    if (tid == 0) s_fail = 0;
    // (a marker segment takes at least four bytes: the tile-part's length bounds the walk)
    for (uint32_t hop = 0, hops = ln / 4 + 2; hop < hops; ++hop) {
        __syncthreads();
        if (tid == 0) {
            uint64_t next = 0, lo = 0, hi = 0;
            s_kind = t2p_header_segment(src, pos, end, &next, &lo, &hi);
            s_next = next; s_lo = lo; s_hi = hi;
        }
        __syncthreads();
        const int kind = s_kind;
        if (kind < 0) { if (tid == 0) report(a.status, t2p_status_tile(t, 0, 0, (uint32_t)-kind)); return; }
        pos = s_next;
        if (kind == 0) break;
        if (kind != 1) continue;
        have_plt = true;
        const uint64_t lo = s_lo, hi = s_hi;
        for (uint64_t base = lo; base < hi; base += 256) {
            const uint64_t i = base + tid;
            const bool term = i < hi && t2p_plt_terminator(src, i);
            uint64_t total = 0;
            const uint64_t rank = scan256(term ? 1u : 0u, s_scan, &total);
            if (term) {
                const uint64_t k = count + rank - 1;
                uint32_t v = 0;
                const uint32_t why = t2p_plt_entry(src, lo, i, &v);
                if (why) atomicMax(&s_fail, why);
                else if (k >= npk) atomicMax(&s_fail, (uint32_t)kT2pPltMany);
                else a.plt_len[T.pkt_base + k] = v;
            }
            count += total;
            __syncthreads();
            if (s_fail) { if (tid == 0) report(a.status, t2p_status_tile(t, 0, 0, s_fail)); return; }
        }
        // (an entry does not run on into the next marker segment)
        if (hi > lo && !t2p_plt_terminator(src, hi - 1)) { if (tid == 0) report(a.status, t2p_status_tile(t, 0, 0, kT2pPltCount)); return; }
    }
    if (s_kind != 0) { if (tid == 0) report(a.status, t2p_status_tile(t, 0, 0, kT2pNoSod)); return; }
    if (npk > end - pos) { if (tid == 0) report(a.status, t2p_status_tile(t, 0, 0, kT2pPacketsBytes)); return; }
    if (have_plt && count != npk) { if (tid == 0) report(a.status, t2p_status_tile(t, 0, 0, kT2pPltCount)); return; }
    if (have_plt) {
        uint64_t run = pos;
        for (uint64_t base = 0; base < npk; base += 256) {
            const uint64_t k = base + tid;
            const uint64_t v = k < npk ? a.plt_len[T.pkt_base + k] : 0;
            uint64_t total = 0;
            const uint64_t incl = scan256(v, s_scan, &total);
            if (k < npk) a.pk_start[T.pkt_base + k] = run + incl - v;
            run += total;
        }
        // the lengths add up to the tile-part: where they do not, a packet's own chain says so first, or nothing is wrong before the end
        if (run != end && tid == 0) report(a.status, t2p_status_tile(t, 1, (uint32_t)npk, kT2pTail));
    }
    if (tid == 0) { a.body_at[t] = pos; a.has_plt[t] = have_plt ? 1u : 0u; }
}

// ---- KC --------------------------------------------------------------------------------------------------------------------------
constexpr uint32_t kWin = 1024;             // the stream's window in LDS: 16 bytes per lane

namespace {

__device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// the stream through a window that the wave's lanes fill together; bytes at or behind `len` are never read
struct WindowSrc {
    const uint8_t* g; uint64_t len; uint8_t* win; uint64_t base; bool valid;
    __device__ void fill(uint64_t pos)
    {
        const uint32_t lane = threadIdx.x;
        const uint64_t mis = (uint64_t)((uintptr_t)(g + pos) & 15u);
        base = pos >= mis ? pos - mis : pos;
        __syncthreads();
        const uint64_t p = base + (uint64_t)lane * 16u;
        if ((((uintptr_t)(g + p)) & 15u) == 0 && p + 16 <= len) *(uint4*)(win + lane * 16u) = *(const uint4*)(g + p);
        else for (uint32_t k = 0; k < 16; ++k) win[lane * 16u + k] = p + k < len ? g[p + k] : (uint8_t)0;
        __syncthreads();
        valid = true;
    }
    __device__ uint32_t byte(uint64_t pos)
    {
        if (!valid || pos < base || pos - base >= kWin) fill(pos);
        return uni(win[pos - base]);
    }
};

// rows to the table 64 at a time: consecutive rows gather in LDS, lane i stores the i-th
struct RowSink {
    grk_amd_coded_block* rows;          // the tile's
    uint32_t* s_len; uint32_t* s_msbs; unsigned long long* s_rel;
    uint32_t first, n;
    unsigned long long* status; uint32_t tile;
    __device__ void flush()
    {
        if (!n) return;
        __syncthreads();
        const uint32_t lane = threadIdx.x;
        if (lane < n) { grk_amd_coded_block r; r.offset = s_rel[lane]; r.length = s_len[lane]; r.missing_msbs = s_msbs[lane]; rows[first + lane] = r; }
        __syncthreads();
        n = 0;
    }
    __device__ void put(uint32_t row, uint32_t length, uint32_t msbs, uint64_t rel)
    {
        if (n == 64 || (n && row != first + n)) flush();
        if (!n) first = row;
        if (threadIdx.x == 0) { s_len[n] = length; s_msbs[n] = msbs; s_rel[n] = rel; }
        ++n;
    }
    __device__ void part1_planes(uint32_t row) { if (threadIdx.x == 0) report(status, t2p_status_tile(tile, 2, row, kT2pPart1Planes)); }
};

} // namespace

__global__ __launch_bounds__(64) void t2read_chains_kernel(T2ReadArgs a)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_win[kWin];
    __shared__ uint32_t s_len[64], s_msbs[64];
    __shared__ unsigned long long s_rel[64];
    const uint32_t chain = blockIdx.x, lane = threadIdx.x;
    // the chain's tile: the last whose chain_base is not beyond it
    uint32_t lo = 0, hi = a.num_tiles;
    while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (a.tiles[mid].chain_base <= chain) lo = mid; else hi = mid; }
    const uint32_t t = lo;
    const T2ReadTile T = a.tiles[t];
    const uint64_t body = a.body_at[t];
    if (!body) return;                                          // (not located, or its header refused)
    const uint64_t end = a.part_at[t] + a.part_len[t];
    const bool plt = a.has_plt[t] != 0, split = plt && T.nchains == T.npackets;
    uint32_t k0 = chain - T.chain_base, k1 = k0 + 1;
    if (!split) { if (k0) return; k1 = T.npackets; }            // one chain parses the tile
    const T2ReadPacket* const pk = a.packets + T.first_packet;
    uint8_t* const nodes = a.nodes + T.node_base;
    // the chain's nodes zeroed by all lanes
    {
        const uint32_t from = split ? pk[k0].node_at : 0u, n = split ? pk[k0].node_n : T.node_bytes;
        for (uint32_t i = lane; i < n; i += 64) nodes[from + i] = 0;
        __threadfence_block();
        __syncthreads();
    }
    WindowSrc src{a.cs, a.len, s_win, 0, false};
    RowSink sink{a.rows + T.row_base, s_len, s_msbs, s_rel, 0, 0, a.status, t};
    uint64_t pos = split ? a.pk_start[T.pkt_base + k0] : body;
    for (uint32_t k = k0; k < k1; ++k) {
        const T2ReadPacket& q = pk[k];
        const uint64_t from = pos;
        uint64_t body_at = 0;
        const uint32_t why = t2p_read_packet(src, q, nodes, a.ht != 0, a.sop != 0, a.eph != 0, k, pos, end, sink, &body_at);
        sink.flush();
        if (why) { if (lane == 0) report(a.status, t2p_status_tile(t, 1, k, why)); return; }
        // the rows' offsets: relative to the end of the header until now
        __threadfence_block();
        __syncthreads();
        for (uint32_t bi = 0; bi < q.nbands; ++bi) {
            const T2ReadBand& B = q.band[bi];
            const uint32_t nb = B.gw * B.gh;
            grk_amd_coded_block* const r = a.rows + T.row_base + B.first_row;
            for (uint32_t i = lane; i < nb; i += 64) r[i].offset = t2p_row_offset(r[i].length, r[i].offset, body_at);
        }
        if (plt && pos - from != a.plt_len[T.pkt_base + k]) { if (lane == 0) report(a.status, t2p_status_tile(t, 1, k, kT2pPltSize)); return; }
    }
    if (!split && pos != end && lane == 0) report(a.status, t2p_status_tile(t, 1, T.npackets, kT2pTail));
}

hipError_t launch_t2read_locate(const T2ReadArgs& a, hipStream_t s)
{
    hipLaunchKernelGGL(t2read_locate_kernel, dim3(1), dim3(256), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_t2read_headers(const T2ReadArgs& a, hipStream_t s)
{
    if (!a.num_tiles) return hipSuccess;
    hipLaunchKernelGGL(t2read_headers_kernel, dim3(a.num_tiles), dim3(256), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_t2read_chains(const T2ReadArgs& a, hipStream_t s)
{
    if (!a.chains) return hipSuccess;
    hipLaunchKernelGGL(t2read_chains_kernel, dim3((uint32_t)a.chains), dim3(64), 0, s, a);
    return hipGetLastError();
}

} // namespace grk_amd
