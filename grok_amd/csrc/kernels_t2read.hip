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
// waits for anybody.  Plain C++: no inline assembly.  Behind KC: the general reader's kernels (KC-L, KF, KP) for files of several
// layers or codeword segments (grk_amd_read_packets_device_ex; the parse: t2_parse_layers.h), which reuse KL and KH as they are.
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

// ==== the general reader: several layers, several codeword segments (t2_parse_layers.h) ==========================================
//   KC-L chains    one wave per chain, as KC: with PLT a precinct with its L packets, each found through its packet start, without
//                  a tile's packets in file order.  The chain clears its nodes (32-bit) and its rows' state, and logs what every
//                  contribution adds -- segment records and piece records, 64 at a time -- into its rows' share of the two logs.
//   KF  finish     over the rows: the row from its state (the bit-plane check: stage 2), and three exclusive scans -- segments,
//                  appendix bytes and moves of the rows before -- by workgroups of 256 rows, a scan of their sums, and an add.
//   KP  place      a lane per log record: segments[first_segment[row] + ordinal] += the record's (a row's records come from one
//                  wave, the sums are 32-bit atomics on zeroed memory), moves[move_first[row] + ordinal] = the piece's.
namespace {

// records to a chain's share of a log 64 at a time; never beyond the share (a full share: `over`, which no stream can cause)
template <class Rec> struct LogSink {
    Rec* log; uint32_t cap; Rec* s_rec; uint32_t count, n; bool over;
    __device__ void flush()
    {
        if (!n) return;
        __syncthreads();
        const uint32_t lane = threadIdx.x;
        if (lane < n && count + lane < cap) log[count + lane] = s_rec[lane];
        if (count + n > cap) over = true;
        count = count + n > cap ? cap : count + n;
        __syncthreads();
        n = 0;
    }
    __device__ void put(const Rec& r)
    {
        if (n == 64) flush();
        if (threadIdx.x == 0) s_rec[n] = r;
        ++n;
    }
};

struct LayerSink {
    LogSink<T2ReadSegRecord> segs; LogSink<T2ReadPieceRecord> pieces;
    __device__ void seg(uint32_t row, uint32_t ordinal, uint32_t len, uint32_t passes, bool opens) { segs.put(T2ReadSegRecord{row, ordinal, len, passes | (opens ? 1u << 31 : 0u)}); }
    __device__ void piece(uint32_t row, uint32_t ordinal, uint64_t rel, uint32_t len, uint32_t before) { pieces.put(T2ReadPieceRecord{rel, row, ordinal, len, before}); }
};

// the tile of chain / of row: the last whose base is not beyond it
__device__ uint32_t tile_of_chain(const T2ReadTile* tiles, uint32_t nt, uint32_t chain)
{
    uint32_t lo = 0, hi = nt;
    while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (tiles[mid].chain_base <= chain) lo = mid; else hi = mid; }
    return lo;
}
__device__ uint32_t tile_of_row(const T2ReadTile* tiles, uint32_t nt, uint64_t row)
{
    uint32_t lo = 0, hi = nt;
    while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (tiles[mid].row_base <= row) lo = mid; else hi = mid; }
    return lo;
}

} // namespace

__global__ __launch_bounds__(64) void t2read_chains_layers_kernel(T2ReadLayersArgs g)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_win[kWin];
    __shared__ T2ReadSegRecord s_seg[64];
    __shared__ T2ReadPieceRecord s_piece[64];
    const T2ReadArgs& a = g.a;
    const uint32_t chain = blockIdx.x, lane = threadIdx.x;
    if (lane == 0) { g.counts[2 * chain] = 0; g.counts[2 * chain + 1] = 0; }
    const uint32_t t = tile_of_chain(a.tiles, a.num_tiles, chain);
    const T2ReadTile T = a.tiles[t];
    const uint64_t body = a.body_at[t];
    if (!body) return;                                          // (not located, or its header refused)
    const uint64_t end = a.part_at[t] + a.part_len[t];
    const uint32_t L = g.layers, np = T.npackets / L;
    const bool plt = a.has_plt[t] != 0, split = plt && T.nchains == np;
    const uint32_t i0 = chain - T.chain_base;
    if (!split && i0) return;                                   // one chain parses the tile
    const T2ReadPacket* const pk = a.packets + T.first_packet;
    const T2ReadLayerPk* const lp = g.lpk + T.first_packet;
    uint32_t* const nodes = g.nodes32 + T.node_base;
    T2pRowState* const state = g.state + T.row_base;
    // the chain's nodes and its rows' state zeroed by all lanes
    {
        const uint32_t from = split ? pk[i0].node_at : 0u, n = split ? pk[i0].node_n : T.node_bytes;
        for (uint32_t i = lane; i < n; i += 64) nodes[from + i] = 0;
        uint32_t* const sw = (uint32_t*)state;
        if (split) {
            for (uint32_t bi = 0; bi < pk[i0].nbands; ++bi) {
                const T2ReadBand& B = pk[i0].band[bi];
                const uint32_t words = B.gw * B.gh * kT2pStateWords;
                for (uint32_t i = lane; i < words; i += 64) sw[(size_t)B.first_row * kT2pStateWords + i] = 0;
            }
        } else for (uint64_t i = lane; i < (uint64_t)T.rows * kT2pStateWords; i += 64) sw[i] = 0;
        __threadfence_block();
        __syncthreads();
    }
    const uint64_t share = (uint64_t)T.row_base + (split ? lp[i0].blocks_before : 0u);
    const uint32_t share_rows = split ? pk[i0].nblocks : T.rows;
    LayerSink sink{{g.seg_log + share * g.seg_per_row, share_rows * g.seg_per_row, s_seg, 0, 0, false},
                   {g.piece_log + share * g.piece_per_row, share_rows * g.piece_per_row, s_piece, 0, 0, false}};
    WindowSrc src{a.cs, a.len, s_win, 0, false};
    uint64_t pos = body;
    bool failed = false;
    // one packet: precinct i, layer l, the tile's packet k
    auto one = [&](uint32_t i, uint32_t l, uint32_t k) -> bool {
        if (split) pos = a.pk_start[T.pkt_base + k];
        const uint64_t from = pos;
        const uint32_t pieces0 = sink.pieces.count + sink.pieces.n;
        uint64_t body_at = 0;
        const uint32_t why = t2p_read_packet_layer(src, pk[i], nodes, state, a.ht != 0, g.sty, a.sop != 0, a.eph != 0, l, k, pos, end, sink, &body_at);
        sink.segs.flush(); sink.pieces.flush();
        if (why) { if (lane == 0) report(a.status, t2p_status_tile(t, 1, k, why)); failed = true; return false; }
        // the pieces' sources: relative to the end of the header until now; a row's first piece is its offset
        __threadfence_block();
        __syncthreads();
        for (uint32_t j = pieces0 + lane; j < sink.pieces.count; j += 64) {
            T2ReadPieceRecord* const r = sink.pieces.log + j;
            const uint64_t at = body_at + r->src;
            r->src = at;
            if (r->ordinal == 0) { state[r->row].src_lo = (uint32_t)at; state[r->row].src_hi = (uint32_t)(at >> 32); }
        }
        if (plt && pos - from != a.plt_len[T.pkt_base + k]) { if (lane == 0) report(a.status, t2p_status_tile(t, 1, k, kT2pPltSize)); failed = true; return false; }
        return true;
    };
    if (split) {
        for (uint32_t l = 0; l < L; ++l)
            if (!one(i0, l, (uint32_t)t2p_packet_number(g.order, np, L, i0, l, lp[i0].run_first, lp[i0].run_count))) break;
    } else {
        t2p_tile_packets(g.order, np, L, [&](uint32_t i, uint32_t* first, uint32_t* count) { *first = lp[i].run_first; *count = lp[i].run_count; }, one);
        if (!failed && pos != end && lane == 0) report(a.status, t2p_status_tile(t, 1, T.npackets, kT2pTail));
    }
    if ((sink.segs.over || sink.pieces.over) && lane == 0) report(a.status, t2p_status_tile(t, 1, T.npackets, kT2pPasses));
    if (lane == 0) { g.counts[2 * chain] = sink.segs.count; g.counts[2 * chain + 1] = sink.pieces.count; }
}

// ---- KF --------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void t2read_finish_rows_kernel(T2ReadLayersArgs g)
{
    __shared__ uint64_t s_scan[256];
    const uint64_t r = (uint64_t)blockIdx.x * kT2ReadScanRows + threadIdx.x;
    uint64_t nseg = 0, app = 0, mv = 0;
    if (r < g.nrows) {
        const T2pRowState s = g.state[r];
        grk_amd_coded_block row;
        if (!t2p_finish_row(s, g.a.ht != 0, &row)) {
            const uint32_t t = tile_of_row(g.a.tiles, g.a.num_tiles, r);
            report(g.a.status, t2p_status_tile(t, 2, (uint32_t)(r - g.a.tiles[t].row_base), kT2pPart1Planes));
        }
        g.a.rows[r] = row;
        nseg = s.nsegs;
        if (s.pieces > 1) { app = s.total; mv = s.pieces; }
    }
    uint64_t total = 0;
    const uint64_t i0 = scan256(nseg, s_scan, &total);
    if (threadIdx.x == 0) g.sums[3 * (uint64_t)blockIdx.x] = total;
    const uint64_t i1 = scan256(app, s_scan, &total);
    if (threadIdx.x == 0) g.sums[3 * (uint64_t)blockIdx.x + 1] = total;
    const uint64_t i2 = scan256(mv, s_scan, &total);
    if (threadIdx.x == 0) g.sums[3 * (uint64_t)blockIdx.x + 2] = total;
    if (r < g.nrows) { g.first_segment[r] = (uint32_t)(i0 - nseg); g.app_at[r] = i1 - app; g.move_first[r] = (uint32_t)(i2 - mv); }
}
// the workgroups' sums to exclusive ones, in place; the totals
__global__ __launch_bounds__(256) void t2read_finish_scan_kernel(T2ReadLayersArgs g)
{
    __shared__ uint64_t s_scan[256];
    const uint64_t nb = (g.nrows + kT2ReadScanRows - 1) / kT2ReadScanRows;
    for (uint32_t q = 0; q < 3; ++q) {
        uint64_t carry = 0;
        for (uint64_t base = 0; base < nb; base += 256) {
            const uint64_t b = base + threadIdx.x;
            const uint64_t v = b < nb ? g.sums[3 * b + q] : 0;
            uint64_t total = 0;
            const uint64_t incl = scan256(v, s_scan, &total);
            if (b < nb) g.sums[3 * b + q] = carry + incl - v;
            carry += total;
        }
        if (threadIdx.x == 0) { g.totals[q] = carry; if (q == 0) g.first_segment[g.nrows] = (uint32_t)carry; }
    }
}
__global__ __launch_bounds__(256) void t2read_finish_add_kernel(T2ReadLayersArgs g)
{
    const uint64_t r = (uint64_t)blockIdx.x * kT2ReadScanRows + threadIdx.x;
    if (r >= g.nrows) return;
    const unsigned long long* const sum = g.sums + 3 * (uint64_t)blockIdx.x;
    g.first_segment[r] += (uint32_t)sum[0];
    const uint64_t at = g.app_at[r] + sum[1];
    g.app_at[r] = at;
    g.move_first[r] += (uint32_t)sum[2];
    if (g.state[r].pieces > 1) g.a.rows[r].offset = g.a.len + at;       // (behind the stream: the appendix)
}

// ---- KP --------------------------------------------------------------------------------------------------------------------------
constexpr uint32_t kPlaceSlices = 8;                 // workgroups per chain
__global__ __launch_bounds__(256) void t2read_place_kernel(T2ReadLayersArgs g)
{
    const T2ReadArgs& a = g.a;
    const uint32_t chain = blockIdx.x;
    const uint32_t t = tile_of_chain(a.tiles, a.num_tiles, chain);
    const T2ReadTile T = a.tiles[t];
    const uint32_t np = T.npackets / g.layers, i0 = chain - T.chain_base;
    const bool split = T.nchains == np && a.has_plt[t] != 0;
    const uint64_t share = (uint64_t)T.row_base + (split ? g.lpk[T.first_packet + i0].blocks_before : 0u);
    const uint32_t nseg = g.counts[2 * chain], npiece = g.counts[2 * chain + 1];
    const T2ReadSegRecord* const sl = g.seg_log + share * g.seg_per_row;
    const T2ReadPieceRecord* const pl = g.piece_log + share * g.piece_per_row;
    const uint32_t step = 256 * kPlaceSlices;
    for (uint32_t j = blockIdx.y * 256 + threadIdx.x; j < nseg; j += step) {
        const T2ReadSegRecord r = sl[j];
        if (r.row >= T.rows) continue;
        const uint64_t at = (uint64_t)g.first_segment[T.row_base + r.row] + r.ordinal;
        if (at >= g.seg_cap) continue;
        atomicAdd(&g.segments[at].length, r.len);
        atomicAdd(&g.segments[at].numpasses, r.passes_opens & 0x7FFFFFFFu);
    }
    for (uint32_t j = blockIdx.y * 256 + threadIdx.x; j < npiece; j += step) {
        const T2ReadPieceRecord r = pl[j];
        if (r.row >= T.rows || g.state[T.row_base + r.row].pieces < 2) continue;
        const uint64_t at = (uint64_t)g.move_first[T.row_base + r.row] + r.ordinal;
        if (at >= g.move_cap) continue;
        g.moves[at] = grk_amd_tp_segment{g.app_at[T.row_base + r.row] + r.before, r.src, r.len, 1u};
    }
}

hipError_t launch_t2read_chains_layers(const T2ReadLayersArgs& g, hipStream_t s)
{
    if (!g.a.chains) return hipSuccess;
    hipLaunchKernelGGL(t2read_chains_layers_kernel, dim3((uint32_t)g.a.chains), dim3(64), 0, s, g);
    return hipGetLastError();
}
hipError_t launch_t2read_finish(const T2ReadLayersArgs& g, hipStream_t s)
{
    if (!g.nrows) return hipSuccess;
    const uint32_t nb = (uint32_t)((g.nrows + kT2ReadScanRows - 1) / kT2ReadScanRows);
    hipLaunchKernelGGL(t2read_finish_rows_kernel, dim3(nb), dim3(256), 0, s, g);
    hipLaunchKernelGGL(t2read_finish_scan_kernel, dim3(1), dim3(256), 0, s, g);
    hipLaunchKernelGGL(t2read_finish_add_kernel, dim3(nb), dim3(256), 0, s, g);
    return hipGetLastError();
}
hipError_t launch_t2read_place(const T2ReadLayersArgs& g, hipStream_t s)
{
    if (!g.a.chains) return hipSuccess;
    hipLaunchKernelGGL(t2read_place_kernel, dim3((uint32_t)g.a.chains, kPlaceSlices), dim3(256), 0, s, g);
    return hipGetLastError();
}

// ==== tiles divided into tile-parts (grk_amd_read_packets_device_parts) ==============================================================
//   KL-P locate    every tile-part of the file.  With TLM the host has the places; without, one lane hops along the Psot chain, at
//                  most `cap` hops (cap <= len / 14 + 1).  All lanes then check the SOTs (striding: more than 256 tile-parts) and
//                  count the tile-parts of every tile, a scan over the tiles gives each its slice of the part table, and every
//                  tile-part goes to slice + TPsot: a slot claimed twice, a TPsot beyond the tile's count, a slot's file place
//                  before its predecessor's, the TNsot rules and a 256th tile-part are refusals.  One workgroup.
//   KH-P headers   a workgroup per tile-part walks its marker segments and counts its PLT entries; then a workgroup per tile scans
//                  its tile-parts' counts into each one's first PLT entry, decides whether the tile is a PLT tile, checks the counts
//                  against the tile's packets, and assembles the entries (KH's parallel assembly) and, for a PLT tile, the packet starts.
//   KC-L over the part table: a precinct chain looks up the tile-part its packet starts in for the packet's `end`; a chain that reads
//                  the tile in file order steps from body to body (t2_parse_layers.h: t2p_part_step).  KF and KP as they are.
namespace {
__device__ __forceinline__ uint32_t load_u32(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
}

__global__ __launch_bounds__(256) void t2read_locate_parts_kernel(T2ReadPartsArgs p)
{
    __shared__ uint64_t s_scan[256];
    __shared__ unsigned long long s_n;
    __shared__ uint32_t s_fail;
    const T2ReadArgs& a = p.g.a;
    const uint32_t tid = threadIdx.x, nt = a.num_tiles, cap = p.cap;
    DirectSrc src{a.cs};
    for (uint32_t t = tid; t < nt; t += 256) { p.count[t] = 0; p.tn_min[t] = 0xFFFFFFFFu; p.tn_max[t] = 0; p.slice[t] = 0; a.body_at[t] = 0; a.has_plt[t] = 0; }
    if (tid == 0) p.slice[nt] = 0;
    for (uint32_t j = tid; j < cap; j += 256) {
        p.claim[j] = 0xFFFFFFFFu; p.tp_at[j] = 0; p.tp_len[j] = 0; p.tp_tile[j] = 0; p.tp_file[j] = 0;
        p.tp_body[j] = 0; p.tp_has_plt[j] = 0; p.tp_npk[j] = 0; p.tp_first[j] = 0;
    }
    if (tid == 0) {
        s_fail = 0;
        uint64_t n = p.n_given < cap ? p.n_given : cap;
        if (!p.n_given) {
            // the Psot chain: every hop checked against the stream's length and at least 14 bytes long
            uint64_t at = a.sot_at;
            n = 0;
            for (uint32_t hop = 0; hop <= cap; ++hop) {
                uint64_t l = 0;
                const int r = t2p_hop(src, a.len, at, &l);
                if (r == 0) break;
                if (r == 2) { s_fail = kT2pNotLocated; break; }
                if (n == cap) { s_fail = kT2pPartsOfFile; break; }
                p.fo_at[n] = at; p.fo_len[n] = (uint32_t)l; p.fo_idx[n] = 0xFFFFFFFFu;
                ++n; at += l;
            }
            if (n == 0 && !s_fail) s_fail = kT2pNotLocated;
        }
        s_n = n;
        p.located[0] = n;
    }
    __threadfence();
    __syncthreads();
    if (s_fail) { if (tid == 0) report(a.status, t2p_status_locate((uint32_t)s_n, s_fail)); return; }
    const uint32_t n = (uint32_t)s_n;
    // pass 1: every SOT; the tile-parts of every tile counted
    for (uint32_t i = tid; i < n; i += 256) {
        uint32_t isot = 0, tps = 0, tn = 0;
        const uint32_t why = t2p_check_sot_part(src, a.len, p.fo_at[i], p.fo_len[i], nt, p.fo_idx[i], i + 1 == n, &isot, &tps, &tn);
        if (why) { report(a.status, t2p_status_locate(i, why)); continue; }
        atomicAdd(&p.count[isot], 1u);
        if (tn) { atomicMin(&p.tn_min[isot], tn); atomicMax(&p.tn_max[isot], tn); }
    }
    __threadfence();
    __syncthreads();
    // every tile's slice of the table
    uint64_t carry = 0;
    for (uint32_t base = 0; base < nt; base += 256) {
        const uint32_t t = base + tid;
        const uint64_t v = t < nt ? load_u32(&p.count[t]) : 0;
        uint64_t total = 0;
        const uint64_t incl = scan256(v, s_scan, &total);
        if (t < nt) p.slice[t] = (uint32_t)(carry + incl - v);
        carry += total;
    }
    if (tid == 0) p.slice[nt] = (uint32_t)carry;
    __threadfence();
    __syncthreads();
    // pass 2: the slot slice + TPsot, claimed by the first tile-part in the file that names it
    for (uint32_t i = tid; i < n; i += 256) {
        uint32_t isot = 0, tps = 0, tn = 0;
        if (t2p_check_sot_part(src, a.len, p.fo_at[i], p.fo_len[i], nt, p.fo_idx[i], i + 1 == n, &isot, &tps, &tn)) continue;
        if (tps < load_u32(&p.count[isot])) { const uint32_t slot = load_u32(&p.slice[isot]) + tps; if (slot < cap) atomicMin(&p.claim[slot], i); }
    }
    __threadfence();
    __syncthreads();
    for (uint32_t i = tid; i < n; i += 256) {
        uint32_t isot = 0, tps = 0, tn = 0;
        if (t2p_check_sot_part(src, a.len, p.fo_at[i], p.fo_len[i], nt, p.fo_idx[i], i + 1 == n, &isot, &tps, &tn)) continue;
        const uint32_t c = load_u32(&p.count[isot]), mn = load_u32(&p.tn_min[isot]), mx = load_u32(&p.tn_max[isot]);
        const uint32_t slot = load_u32(&p.slice[isot]) + tps;
        uint32_t why = kT2pOk;
        if (c > kT2pMaxPartsOfTile && tps >= kT2pMaxPartsOfTile) why = kT2pPartsOfTile;
        else if (tps >= c || slot >= cap || load_u32(&p.claim[slot]) != i) why = kT2pTpsot;
        else if ((tn && mn != mx) || (mx && mx <= tps)) why = kT2pTnsot;
        if (why) { report(a.status, t2p_status_locate(i, why)); continue; }
        p.tp_at[slot] = p.fo_at[i]; p.tp_len[slot] = p.fo_len[i]; p.tp_tile[slot] = isot; p.tp_file[slot] = i;
    }
    __threadfence();
    __syncthreads();
    // pass 3: a tile's tile-parts lie in the file in TPsot order; every tile has one; TNsot is not beyond them
    for (uint32_t j = tid; j + 1 < n; j += 256) {
        if (load_u32(&p.claim[j]) == 0xFFFFFFFFu || load_u32(&p.claim[j + 1]) == 0xFFFFFFFFu) continue;
        if (p.tp_len[j] && p.tp_len[j + 1] && p.tp_tile[j] == p.tp_tile[j + 1] && p.tp_file[j + 1] < p.tp_file[j])
            report(a.status, t2p_status_locate(p.tp_file[j + 1], kT2pTpsot));
    }
    for (uint32_t t = tid; t < nt; t += 256) {
        const uint32_t c = load_u32(&p.count[t]);
        if (!c) report(a.status, t2p_status_locate(n + 1 + t, kT2pNoPart));
        else if (load_u32(&p.tn_max[t]) > c) report(a.status, t2p_status_locate(n + 1 + t, kT2pTnsot));
    }
}

// KH-P, first step: the tile-part in slot blockIdx.x -- its marker segments walked, its PLT entries counted and checked
__global__ __launch_bounds__(256) void t2read_headers_parts_kernel(T2ReadPartsArgs p)
{
    __shared__ uint64_t s_scan[256];
    __shared__ int s_kind;
    __shared__ unsigned long long s_next, s_lo, s_hi;
    __shared__ uint32_t s_fail;
    const T2ReadArgs& a = p.g.a;
    const uint32_t j = blockIdx.x, tid = threadIdx.x;
    if (j >= p.cap) return;
    const uint32_t ln = p.tp_len[j];
    if (!ln) return;
    const uint32_t t = p.tp_tile[j];
    if (t >= a.num_tiles) return;
    const uint32_t part = j - p.slice[t];
    const uint64_t npk = a.tiles[t].npackets;
    const uint64_t at = p.tp_at[j], end = at + ln;
    DirectSrc src{a.cs};
    uint64_t pos = at + 12, count = 0;
    bool have_plt = false;
    if (tid == 0) s_fail = 0;
    for (uint32_t hop = 0, hops = ln / 4 + 2; hop < hops; ++hop) {
        __syncthreads();
        if (tid == 0) {
            uint64_t next = 0, lo = 0, hi = 0;
            s_kind = t2p_header_segment(src, pos, end, &next, &lo, &hi);
            s_next = next; s_lo = lo; s_hi = hi;
        }
        __syncthreads();
        const int kind = s_kind;
        if (kind < 0) { if (tid == 0) report(a.status, t2p_status_tile(t, 0, part, (uint32_t)-kind)); return; }
        pos = s_next;
        if (kind == 0) break;
        if (kind != 1) continue;
        have_plt = true;
        const uint64_t lo = s_lo, hi = s_hi;
        for (uint64_t base = lo; base < hi; base += 256) {
            const uint64_t i = base + tid;
            const bool term = i < hi && t2p_plt_terminator(src, i);
            uint64_t total = 0;
            (void)scan256(term ? 1u : 0u, s_scan, &total);
            if (term) {
                uint32_t v = 0;
                const uint32_t why = t2p_plt_entry(src, lo, i, &v);
                if (why) atomicMax(&s_fail, why);
            }
            count += total;
            if (count > npk) atomicMax(&s_fail, (uint32_t)kT2pPltMany);
            __syncthreads();
            if (s_fail) { if (tid == 0) report(a.status, t2p_status_tile(t, 0, part, s_fail)); return; }
        }
        if (hi > lo && !t2p_plt_terminator(src, hi - 1)) { if (tid == 0) report(a.status, t2p_status_tile(t, 0, part, kT2pPltCount)); return; }
    }
    if (s_kind != 0) { if (tid == 0) report(a.status, t2p_status_tile(t, 0, part, kT2pNoSod)); return; }
    if (tid == 0) { p.tp_body[j] = pos; p.tp_has_plt[j] = have_plt ? 1u : 0u; p.tp_npk[j] = (uint32_t)count; }
}

// KH-P, second step: the tile blockIdx.x over its tile-parts
__global__ __launch_bounds__(256) void t2read_tile_parts_kernel(T2ReadPartsArgs p)
{
    __shared__ uint64_t s_scan[256];
    __shared__ int s_kind;
    __shared__ unsigned long long s_next, s_lo, s_hi;
    __shared__ uint32_t s_fail, s_any, s_missing;
    const T2ReadArgs& a = p.g.a;
    const uint32_t t = blockIdx.x, tid = threadIdx.x;
    const uint32_t j0 = p.slice[t], np = p.slice[t + 1] - j0;
    if (!np || np > kT2pMaxPartsOfTile || j0 + np > p.cap) return;
    const T2ReadTile T = a.tiles[t];
    const uint64_t npk = T.npackets;
    DirectSrc src{a.cs};
    if (tid == 0) { s_fail = 0; s_any = 0; s_missing = 0; }
    __syncthreads();
    const bool mine = tid < np;
    const uint64_t body = mine ? p.tp_body[j0 + tid] : 0;
    const uint64_t bytes = mine && body ? p.tp_at[j0 + tid] + p.tp_len[j0 + tid] - body : 0;
    const uint32_t cnt = mine ? p.tp_npk[j0 + tid] : 0, has = mine ? p.tp_has_plt[j0 + tid] : 0;
    if (mine && !body) atomicMax(&s_fail, 1u);                   // (a tile-part whose header was refused: reported there)
    if (has) atomicMax(&s_any, 1u);
    if (mine && bytes && !has) atomicMax(&s_missing, 1u);
    uint64_t all = 0, room = 0;
    const uint64_t incl = scan256(cnt, s_scan, &all);
    (void)scan256(bytes, s_scan, &room);
    __syncthreads();
    if (s_fail) return;
    if (all > npk) { if (tid == 0) report(a.status, t2p_status_tile(t, 0, 0, kT2pPltMany)); return; }
    if (npk > room) { if (tid == 0) report(a.status, t2p_status_tile(t, 0, 0, kT2pPacketsBytes)); return; }
    const bool plt_tile = np == 1 ? p.tp_has_plt[j0] != 0 : (s_any && !s_missing);
    if (plt_tile && all != npk) { if (tid == 0) report(a.status, t2p_status_tile(t, 0, 0, kT2pPltCount)); return; }
    if (mine) p.tp_first[j0 + tid] = T.pkt_base + (uint32_t)(incl - cnt);
    __threadfence();
    __syncthreads();
    // the entries, tile-part after tile-part (all <= npk: they fit the tile's share of plt_len)
    for (uint32_t q = 0; q < np; ++q) {
        const uint32_t j = j0 + q;
        if (!p.tp_has_plt[j]) continue;
        const uint32_t first = load_u32(&p.tp_first[j]), want = p.tp_npk[j];
        const uint64_t at = p.tp_at[j], end = at + p.tp_len[j];
        uint64_t pos = at + 12, count = 0;
        for (uint32_t hop = 0, hops = p.tp_len[j] / 4 + 2; hop < hops; ++hop) {
            __syncthreads();
            if (tid == 0) {
                uint64_t next = 0, lo = 0, hi = 0;
                s_kind = t2p_header_segment(src, pos, end, &next, &lo, &hi);
                s_next = next; s_lo = lo; s_hi = hi;
            }
            __syncthreads();
            const int kind = s_kind;
            pos = s_next;
            if (kind <= 0) break;
            if (kind != 1) continue;
            const uint64_t lo = s_lo, hi = s_hi;
            for (uint64_t base = lo; base < hi; base += 256) {
                const uint64_t i = base + tid;
                const bool term = i < hi && t2p_plt_terminator(src, i);
                uint64_t total = 0;
                const uint64_t rank = scan256(term ? 1u : 0u, s_scan, &total);
                if (term) {
                    const uint64_t k = count + rank - 1;
                    uint32_t v = 0;
                    if (!t2p_plt_entry(src, lo, i, &v) && k < want) a.plt_len[first + k] = v;
                }
                count += total;
            }
        }
        if (!plt_tile) continue;
        // a PLT tile: the packet starts; the lengths add up to the tile-part
        __threadfence();
        __syncthreads();
        uint64_t run = p.tp_body[j];
        for (uint64_t base = 0; base < want; base += 256) {
            const uint64_t k = base + tid;
            const uint64_t v = k < want ? a.plt_len[first + k] : 0;
            uint64_t total = 0;
            const uint64_t inc = scan256(v, s_scan, &total);
            if (k < want) a.pk_start[first + k] = run + inc - v;
            run += total;
        }
        if (run != end && tid == 0) report(a.status, t2p_status_tile(t, 0, q, kT2pPartPlt));
    }
    if (tid == 0) { a.body_at[t] = p.tp_body[j0]; a.has_plt[t] = plt_tile ? 1u : 0u; }
}

__global__ __launch_bounds__(64) void t2read_chains_parts_kernel(T2ReadPartsArgs p)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_win[kWin];
    __shared__ T2ReadSegRecord s_seg[64];
    __shared__ T2ReadPieceRecord s_piece[64];
    const T2ReadLayersArgs& g = p.g;
    const T2ReadArgs& a = g.a;
    const uint32_t chain = blockIdx.x, lane = threadIdx.x;
    if (lane == 0) { g.counts[2 * chain] = 0; g.counts[2 * chain + 1] = 0; }
    const uint32_t t = tile_of_chain(a.tiles, a.num_tiles, chain);
    const T2ReadTile T = a.tiles[t];
    if (!a.body_at[t]) return;                                  // (not located, or a header refused)
    const uint32_t j0 = p.slice[t], nparts = p.slice[t + 1] - j0;
    if (!nparts || nparts > kT2pMaxPartsOfTile || j0 + nparts > p.cap) return;
    const T2pParts PT{p.tp_at + j0, p.tp_len + j0, p.tp_body + j0, p.tp_has_plt + j0, p.tp_npk + j0, p.tp_first + j0, nparts};
    const uint32_t L = g.layers, np = T.npackets / L;
    const bool plt = a.has_plt[t] != 0, split = plt && T.nchains == np;
    const uint32_t i0 = chain - T.chain_base;
    if (!split && i0) return;                                   // one chain parses the tile
    const T2ReadPacket* const pk = a.packets + T.first_packet;
    const T2ReadLayerPk* const lp = g.lpk + T.first_packet;
    uint32_t* const nodes = g.nodes32 + T.node_base;
    T2pRowState* const state = g.state + T.row_base;
    {
        const uint32_t from = split ? pk[i0].node_at : 0u, n = split ? pk[i0].node_n : T.node_bytes;
        for (uint32_t i = lane; i < n; i += 64) nodes[from + i] = 0;
        uint32_t* const sw = (uint32_t*)state;
        if (split) {
            for (uint32_t bi = 0; bi < pk[i0].nbands; ++bi) {
                const T2ReadBand& B = pk[i0].band[bi];
                const uint32_t words = B.gw * B.gh * kT2pStateWords;
                for (uint32_t i = lane; i < words; i += 64) sw[(size_t)B.first_row * kT2pStateWords + i] = 0;
            }
        } else for (uint64_t i = lane; i < (uint64_t)T.rows * kT2pStateWords; i += 64) sw[i] = 0;
        __threadfence_block();
        __syncthreads();
    }
    const uint64_t share = (uint64_t)T.row_base + (split ? lp[i0].blocks_before : 0u);
    const uint32_t share_rows = split ? pk[i0].nblocks : T.rows;
    LayerSink sink{{g.seg_log + share * g.seg_per_row, share_rows * g.seg_per_row, s_seg, 0, 0, false},
                   {g.piece_log + share * g.piece_per_row, share_rows * g.piece_per_row, s_piece, 0, 0, false}};
    WindowSrc src{a.cs, a.len, s_win, 0, false};
    T2pPartWalk walk{0, 0, 0};
    uint64_t pos = 0;
    t2p_part_walk_start(PT, walk, pos);
    bool failed = false;
    auto refuse = [&](uint32_t k, uint32_t why) { if (lane == 0) report(a.status, t2p_status_tile(t, 1, k, why)); failed = true; return false; };
    // one packet: precinct i, layer l, the tile's packet k; its `end` is the end of the tile-part it starts in
    auto one = [&](uint32_t i, uint32_t l, uint32_t k) -> bool {
        uint64_t end = 0;
        if (split) {
            pos = a.pk_start[T.pkt_base + k];
            end = t2p_part_end(PT, t2p_part_of(PT, pos));
        } else {
            const uint32_t why = t2p_part_step(PT, walk, pos);
            if (why) return refuse(k, why);
            end = walk.end;
        }
        const uint64_t from = pos;
        const uint32_t pieces0 = sink.pieces.count + sink.pieces.n;
        uint64_t body_at = 0;
        const uint32_t why = t2p_read_packet_layer(src, pk[i], nodes, state, a.ht != 0, g.sty, a.sop != 0, a.eph != 0, l, k, pos, end, sink, &body_at);
        sink.segs.flush(); sink.pieces.flush();
        if (why) return refuse(k, why);
        __threadfence_block();
        __syncthreads();
        for (uint32_t j = pieces0 + lane; j < sink.pieces.count; j += 64) {
            T2ReadPieceRecord* const r = sink.pieces.log + j;
            const uint64_t at = body_at + r->src;
            r->src = at;
            if (r->ordinal == 0) { state[r->row].src_lo = (uint32_t)at; state[r->row].src_hi = (uint32_t)(at >> 32); }
        }
        if (split) { if (pos - from != a.plt_len[T.pkt_base + k]) return refuse(k, kT2pPltSize); }
        else { const uint32_t w2 = t2p_part_packet(PT, walk, a.plt_len, pos - from); if (w2) return refuse(k, w2); }
        return true;
    };
    if (split) {
        for (uint32_t l = 0; l < L; ++l)
            if (!one(i0, l, (uint32_t)t2p_packet_number(g.order, np, L, i0, l, lp[i0].run_first, lp[i0].run_count))) break;
    } else {
        t2p_tile_packets(g.order, np, L, [&](uint32_t i, uint32_t* first, uint32_t* count) { *first = lp[i].run_first; *count = lp[i].run_count; }, one);
        if (!failed) { const uint32_t why = t2p_part_finish(PT, walk, pos); if (why) refuse(T.npackets, why); }
    }
    if ((sink.segs.over || sink.pieces.over) && lane == 0) report(a.status, t2p_status_tile(t, 1, T.npackets, kT2pPasses));
    if (lane == 0) { g.counts[2 * chain] = sink.segs.count; g.counts[2 * chain + 1] = sink.pieces.count; }
}

hipError_t launch_t2read_locate_parts(const T2ReadPartsArgs& p, hipStream_t s)
{
    hipLaunchKernelGGL(t2read_locate_parts_kernel, dim3(1), dim3(256), 0, s, p);
    return hipGetLastError();
}
hipError_t launch_t2read_headers_parts(const T2ReadPartsArgs& p, uint32_t nparts, hipStream_t s)
{
    if (!nparts || !p.g.a.num_tiles) return hipSuccess;
    hipLaunchKernelGGL(t2read_headers_parts_kernel, dim3(nparts), dim3(256), 0, s, p);
    hipLaunchKernelGGL(t2read_tile_parts_kernel, dim3(p.g.a.num_tiles), dim3(256), 0, s, p);
    return hipGetLastError();
}
hipError_t launch_t2read_chains_parts(const T2ReadPartsArgs& p, hipStream_t s)
{
    if (!p.g.a.chains) return hipSuccess;
    hipLaunchKernelGGL(t2read_chains_parts_kernel, dim3((uint32_t)p.g.a.chains), dim3(64), 0, s, p);
    return hipGetLastError();
}

} // namespace grk_amd
