// grok_amd/csrc/kernels_t2keep.hip -- a batch's results kept on the device for an image-wide Tier-2 (assemble.hip: the joint route).
//
// An image of sub-sampled components is coded by several grk_amd_encode_tiles calls (image.h: a batch per geometry group, the surface
// route's in-place units one by one), each of which overwrites the context's table and arena.  KK t2_keep_kernel, queued behind a
// batch's K3, moves what the batch left into image-wide buffers:
//   rows   entry i of the batch's table (unit i / bpu of the batch, row i % bpu of that unit) becomes row row_at[unit] + i % bpu of the
//          image's tables: its length, and its offset plus the batch's base in the image's arena.  The units' first rows come as a
//          list, not as a stride: a batch may hold two units of one tile (Y and A of a Y / CbCr / A image), and a geometry group may
//          be split over several batches.
//   bytes  [0, used) of the batch's arena -- `used` is K3's own cursor, read on the device -- to the image's arena at the base, as
//          whole 16-byte lines: both sides start on a 16-byte boundary (the base is a sum of `used` values rounded up to 16), so every
//          lane loads and stores aligned uint4, consecutive lanes consecutive lines -- one read and one write of the coded bytes, their
//          only extra trip through HBM before the gather.  The blocks keep their offsets relative to the batch's arena.
// The base is a running cursor on the device: batch k reads cursors[k] and writes cursors[k + 1], no host in between.  K3's status
// word (arena overflow, magnitudes out of contract) is OR-ed into the image's, since the next batch resets K3's.
#include "kernels.h"

namespace grk_amd {

constexpr uint32_t kKeepThreads = 256;

__global__ __launch_bounds__(256) void t2_keep_kernel(T2KeepArgs a)
{
    const uint64_t nthr = (uint64_t)a.grid * kKeepThreads, gtid = (uint64_t)blockIdx.x * kKeepThreads + threadIdx.x;
    const uint64_t base = a.cursors[0];
    const uint64_t used = a.batch_state[1];
    // (an overflowed batch may leave a cursor beyond its arena; the image's arena was sized for at most arena_bound bytes of this batch)
    const bool fits = used <= a.arena_bound && base + ((used + 15u) & ~15ull) <= a.j_cap;
    const uint64_t lines = fits ? (used + 15u) >> 4 : 0u;
    if (gtid == 0) {
        a.cursors[1] = base + (lines << 4);
        const unsigned int st = (unsigned int)a.batch_state[0] | (fits ? 0u : 1u);
        if (st) atomicOr(a.status, st);
    }
    const uint64_t nrows = (uint64_t)a.nunits * a.bpu;
    for (uint64_t i = gtid; i < nrows; i += nthr) {
        const uint64_t u = i / a.bpu, j = a.row_at[u] + (i - u * a.bpu);
        a.j_lengths[j] = fits ? a.lengths[i] : 0u;
        a.j_offsets[j] = base + (fits ? a.offsets[i] : 0ull);
        if (a.j_msbs) a.j_msbs[j] = (uint8_t)drop_missing_msbs(a.blocks[i - u * a.bpu].kmax, a.drops ? a.drops[i] : 0u);
    }
    const uint4* const s = reinterpret_cast<const uint4*>(a.arena);
    uint4* const d = reinterpret_cast<uint4*>(a.j_arena + base);
    for (uint64_t v = gtid; v < lines; v += nthr) d[v] = s[v];
}

hipError_t launch_t2_keep(const T2KeepArgs& a0, hipStream_t s)
{
    if (!a0.nunits || !a0.bpu) return hipSuccess;
    // the copy is bound by HBM: a few workgroups per compute unit walk the lines; a small batch takes what its bound needs
    T2KeepArgs a = a0;
    const uint64_t work = (a.arena_bound >> 4) + (uint64_t)a.nunits * a.bpu;
    const uint64_t groups = (work + kKeepThreads - 1) / kKeepThreads;
    a.grid = groups > 1024 ? 1024u : (uint32_t)groups;
    hipLaunchKernelGGL(t2_keep_kernel, dim3(a.grid), dim3(kKeepThreads), 0, s, a);
    return hipGetLastError();
}

} // namespace grk_amd
