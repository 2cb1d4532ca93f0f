// grok_amd/csrc/kernels_rate.hip -- rate-targeted encodes: what dropping bit-planes costs each block, and which drop each block gets.
//
// HTJ2K has one cleanup pass per block and this encoder one layer, so a byte target cannot be met by truncating passes.  What the
// format does offer is the block's zero-bit-plane count: a block coded as mu >> d with Kmax - 1 - d zero bit-planes (kernels_ht.hip,
// the DROP instances) is d bit-planes shorter, and a decoder that positions the block by the band's Kmax reconstructs the coarser
// bin's centre (9/7 everywhere; Grok's and this library's REVERSIBLE dequantiser shifts by the block's own zero bit-planes instead and
// returns mu >> d: DESIGN.md section 3).  Two kernels choose d:
//   KR1 rate_stats_kernel  one wave per block, one pass over its coefficients: for every candidate the exact squared error of what a
//                          decoder reconstructs, in units of (half a quantisation step)^2
//   KR2 rate_alloc_kernel  one workgroup: bisects the Lagrange multiplier over the tables (lengths from trial launches of the DROP
//                          instances, the errors of KR1, the blocks' weights), then spends what the budget has left in table order
// and, for a quality target, one more over the same tables:
//   KQ  rate_quality_kernel  one workgroup: the largest multiplier whose choice keeps the sum of W E within a distortion budget, then
//                          a trim in table order that gives up whatever bytes the slack still pays for
// Everything is integer or a fixed-order double sum: two runs give the same bytes.
#include "kernels.h"

namespace grk_amd {

namespace {

// ---- KR1 ------------------------------------------------------------------------------------------------------------------------------
// q: the magnitude the d = 0 coder codes (|x| reversible; trunc(|c| / step) clamped to 2^Kmax - 1 irreversible: kernels_ht.hip).
// Candidate c reconstructs r_c(q) = q (c = 0); 0 where q >> c == 0, and for SKIP; else ((q >> c) << c) + 2^(c - 1) -- with c clamped
// to Kmax - 1 as the coder clamps it, so that a row describes the block as coded (it differs from the unclamped row only in bands
// with Kmax <= Dmax).
// E[c][block] = sum over the block of (2 q - 2 r_c(q))^2, modulo 2^64 (q < 2^30: a 64 x 64 block stays below 2^64 up to q < 2^25).
// The block's column: its own index in rows of nblocks entries (map == nullptr), or -- a batch writing into a call's joint tables --
// map[tile] + its index in the tile, in rows of n entries (the host planned the map: plan_rate_joint).
template <class PLANE, bool IRREV>
__global__ __launch_bounds__(64) void rate_stats_kernel(const PLANE* mallat, uint32_t stride, uint64_t pitch, const HtBlockDesc* blocks,
                                                        uint32_t blocks_per_tile, uint32_t ncomp, uint64_t nblocks, uint32_t dmax,
                                                        unsigned long long* E, const unsigned long long* map, uint64_t n)
{
    const uint64_t i = blockIdx.x;
    if (i >= nblocks) return;
    const uint32_t lane = threadIdx.x;
    const HtBlockDesc bd = blocks[i % blocks_per_tile];
    const uint32_t tile = (uint32_t)(i / blocks_per_tile);
    const PLANE* src = mallat + ((size_t)tile * ncomp + bd.comp) * pitch + (size_t)bd.py * stride + bd.px;
    unsigned long long acc[kRateMaxDrop + 1];       // [c] for c = 1 .. dmax, [0]: SKIP
#pragma unroll
    for (uint32_t c = 0; c <= kRateMaxDrop; ++c) acc[c] = 0;
    const uint32_t lim = (1u << bd.kmax) - 1u;
    const uint32_t top = bd.kmax ? bd.kmax - 1u : 0u;           // the largest drop the coder takes
    for (uint32_t y = 0; y < bd.h; ++y)
        for (uint32_t x = lane; x < bd.w; x += 64) {
            uint32_t q;
            if constexpr (IRREV) {
                const float cf = __int_as_float((int32_t)src[(size_t)y * stride + x]);
                q = (uint32_t)__fmul_rn(fabsf(cf), bd.inv_step);
                q = q > lim ? lim : q;
            } else {
                const int32_t v = (int32_t)src[(size_t)y * stride + x];
                q = (uint32_t)(v < 0 ? -v : v);
            }
            const unsigned long long all = 4ull * q * q;
            acc[0] += all;
#pragma unroll
            for (uint32_t c = 1; c <= kRateMaxDrop; ++c) {        // (rows beyond dmax are computed and not stored: no dynamic index)
                const uint32_t ce = min(c, top);
                const long long diff = (long long)(q & ((1u << ce) - 1u)) - (long long)((1u << ce) >> 1);
                acc[c] += (q >> ce) ? 4ull * (unsigned long long)(diff * diff) : all;
            }
        }
#pragma unroll
    for (uint32_t c = 0; c <= kRateMaxDrop; ++c)
        for (int off = 32; off > 0; off >>= 1) acc[c] += __shfl_down(acc[c], off, 64);
    if (lane == 0) {
        const uint64_t col = map ? map[tile] + i % blocks_per_tile : i;
        E[col] = 0;                                                 // row 0: nothing dropped
#pragma unroll
        for (uint32_t c = 1; c <= kRateMaxDrop; ++c) if (c <= dmax) E[(uint64_t)c * n + col] = acc[c];
        E[(uint64_t)(dmax + 1u) * n + col] = acc[0];                // row dmax + 1: SKIP
    }
}

// ---- a batch's column of a joint table ------------------------------------------------------------------------------------------------
// Entry i of a batch (unit i / per_unit, tile-major as K3 writes its length column and reads its drops) is entry map[unit] + i %
// per_unit of a joint row.  GATHER = false: batch -> joint (a trial's lengths into row d of L); true: joint -> batch (the chosen drop
// bytes for the batch's final launch).  Every index is inside both arrays: the host planned the map.
template <class T, bool GATHER>
__global__ __launch_bounds__(256) void rate_map_kernel(T* batch, T* joint, const unsigned long long* map, uint32_t per_unit, uint64_t count)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= count) return;
    const uint64_t j = map[i / per_unit] + i % per_unit;
    if constexpr (GATHER) batch[i] = joint[j]; else joint[j] = batch[i];
}

// ---- KR2 ------------------------------------------------------------------------------------------------------------------------------
constexpr uint32_t kFillChunk = 512;                    // blocks the fill takes at a time
constexpr uint32_t kFillSteps = kRateMaxCand - 1;       // moves to a finer candidate a block can make at most

// a workgroup-wide sum in a fixed order (the same tree every run): every thread gets the total
template <class T>
__device__ __forceinline__ T block_sum(T v, T* red)
{
    const uint32_t t = threadIdx.x;
    __syncthreads();
    red[t] = v;
    __syncthreads();
    for (uint32_t s = kRateAllocThreads / 2; s > 0; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    return red[0];
}

// candidate of block b under multiplier lambda: the smallest W E + lambda L, the finer one of a tie (KR2 and KQ)
__device__ __forceinline__ uint32_t rate_choose(const uint32_t* L, const unsigned long long* E, const double* W, uint64_t n, uint32_t ncand,
                                                uint64_t b, double lambda)
{
    const double w = W[b];
    double best = 0; uint32_t bc = 0;
    for (uint32_t c = 0; c < ncand; ++c) {
        const double cost = w * (double)E[(uint64_t)c * n + b] + lambda * (double)L[(uint64_t)c * n + b];
        if (c == 0 || cost < best) { best = cost; bc = c; }
    }
    return bc;
}

// the shortest candidate of block b, the finer one of equally short ones: the choice no multiplier undercuts
__device__ __forceinline__ uint32_t rate_shortest(const uint32_t* L, uint64_t n, uint32_t ncand, uint64_t b)
{
    uint32_t c = 0;
    for (uint32_t k = 1; k < ncand; ++k) if (L[(uint64_t)k * n + b] < L[(uint64_t)c * n + b]) c = k;
    return c;
}

__global__ __launch_bounds__(kRateAllocThreads) void rate_alloc_kernel(RateAllocArgs a)
{
    __shared__ unsigned long long red_u[kRateAllocThreads];
    __shared__ double red_d[kRateAllocThreads];
    __shared__ int32_t fill_delta[kFillChunk][kFillSteps];
    __shared__ uint8_t fill_len[kFillChunk], fill_taken[kFillChunk];
    const uint32_t t = threadIdx.x;
    const uint64_t n = a.nblocks;
    const uint32_t ncand = a.ncand;

    auto choose = [&](uint64_t b, double lambda) -> uint32_t { return rate_choose(a.L, a.E, a.W, n, ncand, b, lambda); };
    auto total_at = [&](double lambda) -> unsigned long long {
        unsigned long long s = 0;
        for (uint64_t b = t; b < n; b += kRateAllocThreads) s += a.L[(uint64_t)choose(b, lambda) * n + b];
        return block_sum(s, red_u);
    };

    // the fewest bytes any choice takes: below that no multiplier helps
    unsigned long long least;
    {
        unsigned long long s = 0;
        for (uint64_t b = t; b < n; b += kRateAllocThreads) {
            uint32_t m = a.L[b];
            for (uint32_t c = 1; c < ncand; ++c) m = min(m, a.L[(uint64_t)c * n + b]);
            s += m;
        }
        least = block_sum(s, red_u);
    }
    const bool feasible = least <= a.budget;
    double lambda = 0;
    uint32_t steps = 0;
    bool bracketed = true;
    if (feasible && total_at(0.0) > a.budget) {
        // bracket within a factor of two, from 1: down while the smaller multiplier still fits, else up until one fits (it does by
        // 2^200: the costs are below 2^130), then bisect.  hi always fits, lo never does.
        double hi = 1.0, lo;
        if (total_at(hi) <= a.budget) {
            while (steps < 200u && total_at(hi * 0.5) <= a.budget) { hi *= 0.5; ++steps; }
            lo = steps < 200u ? hi * 0.5 : 0.0;
        } else {
            unsigned long long at_hi;
            do { hi *= 2.0; ++steps; at_hi = total_at(hi); } while (steps < 200u && at_hi > a.budget);
            bracketed = at_hi <= a.budget;
            lo = hi * 0.5;
        }
        for (uint32_t k = 0; k < kRateBisectSteps; ++k, ++steps) {
            const double mid = 0.5 * (lo + hi);
            if (total_at(mid) <= a.budget) hi = mid; else lo = mid;
        }
        lambda = hi;
    }
    // the choice at lambda (not feasible, or no multiplier found that fits: every block at its shortest candidate -- which fits
    // whenever anything does, and otherwise shows the caller what is missing)
    const bool shortest = !feasible || !bracketed;
    unsigned long long lagrange;
    {
        unsigned long long s = 0;
        for (uint64_t b = t; b < n; b += kRateAllocThreads) {
            uint32_t c;
            if (!shortest) c = choose(b, lambda);
            else c = rate_shortest(a.L, n, ncand, b);
            a.drop[b] = (uint8_t)c;
            s += a.L[(uint64_t)c * n + b];
        }
        lagrange = block_sum(s, red_u);
    }
    // the fill, in table order: a block moves to the next finer candidate while that lowers W E (W > 0: while it lowers E) and the
    // bytes it adds fit what is left; a block that does not fit is passed over and the walk goes on.  kFillChunk blocks at a time: their
    // chains of moves are looked up by a thread each, one thread walks them with the running remainder, a thread each writes them back.
    long long left = (long long)a.budget - (long long)lagrange;       // (thread 0's is the one that counts)
    for (uint64_t base = 0; feasible && base < n; base += kFillChunk) {
        const uint64_t b = base + t;
        uint32_t c = 0;
        if (t < kFillChunk && b < n) {
            c = a.drop[b];
            uint32_t len = 0;
            for (uint32_t s = 0; s < c && s < kFillSteps; ++s) {
                const uint64_t fine = (uint64_t)(c - s - 1u) * n + b, coarse = (uint64_t)(c - s) * n + b;
                if (!(a.E[fine] < a.E[coarse])) break;
                fill_delta[t][s] = (int32_t)((long long)a.L[fine] - (long long)a.L[coarse]);
                ++len;
            }
            fill_len[t] = (uint8_t)len;
        }
        __syncthreads();
        if (t == 0) {
            const uint32_t cnt = (uint32_t)min((uint64_t)kFillChunk, n - base);
            for (uint32_t i = 0; i < cnt; ++i) {
                uint32_t k = 0;
                while (k < fill_len[i] && (long long)fill_delta[i][k] <= left) { left -= fill_delta[i][k]; ++k; }
                fill_taken[i] = (uint8_t)k;
            }
        }
        __syncthreads();
        if (t < kFillChunk && b < n) a.drop[b] = (uint8_t)(c - fill_taken[t]);
        __syncthreads();
    }
    // the result, and the candidates as the drop bytes the block coder takes
    unsigned long long bytes = 0;
    double dist = 0;
    for (uint64_t b = t; b < n; b += kRateAllocThreads) {
        const uint32_t c = a.drop[b];
        bytes += a.L[(uint64_t)c * n + b];
        dist += a.W[b] * (double)a.E[(uint64_t)c * n + b];
        a.drop[b] = c <= a.dmax ? (uint8_t)c : (uint8_t)kHtDropSkip;
    }
    bytes = block_sum(bytes, red_u);
    dist = block_sum(dist, red_d);
    if (t == 0) {
        a.res->block_bytes = bytes; a.res->lagrange_bytes = lagrange; a.res->least_bytes = least;
        a.res->distortion = dist; a.res->lambda = lambda;
        a.res->feasible = feasible ? 1u : 0u; a.res->steps = steps;
    }
}

// ---- KQ -------------------------------------------------------------------------------------------------------------------------------
// The dual of KR2: the fewest bytes whose distortion sum of W E stays within the budget D (kernels.h has the wording).  The trim's
// table of doubles would not fit the 64 KB of a workgroup beside the two reduction buffers at KR2's chunk: KQ takes half of it.
constexpr uint32_t kTrimChunk = kFillChunk / 2;
static_assert(kTrimChunk * kFillSteps * sizeof(double) + kRateAllocThreads * 16u + kTrimChunk * 2u <= 65536u, "KQ's LDS");

__global__ __launch_bounds__(kRateAllocThreads) void rate_quality_kernel(RateQualityArgs a)
{
    __shared__ unsigned long long red_u[kRateAllocThreads];
    __shared__ double red_d[kRateAllocThreads];
    __shared__ double trim_delta[kTrimChunk][kFillSteps];
    __shared__ uint8_t trim_len[kTrimChunk], trim_taken[kTrimChunk];
    const uint32_t t = threadIdx.x;
    const uint64_t n = a.nblocks;
    const uint32_t ncand = a.ncand;
    const double D = a.budget;

    auto dist_of = [&](uint64_t b, uint32_t c) -> double { return a.W[b] * (double)a.E[(uint64_t)c * n + b]; };
    auto dist_at = [&](double lambda) -> double {
        double s = 0;
        for (uint64_t b = t; b < n; b += kRateAllocThreads) s += dist_of(b, rate_choose(a.L, a.E, a.W, n, ncand, b, lambda));
        return block_sum(s, red_d);
    };

    // the least distortion any choice has: below that nothing helps.  The shortest choice: the fewest bytes there are.
    double floor_d, short_d;
    unsigned long long short_l;
    {
        double f = 0, sd = 0;
        unsigned long long sl = 0;
        for (uint64_t b = t; b < n; b += kRateAllocThreads) {
            unsigned long long m = a.E[b];
            for (uint32_t c = 1; c < ncand; ++c) m = min(m, a.E[(uint64_t)c * n + b]);
            f += a.W[b] * (double)m;
            const uint32_t c = rate_shortest(a.L, n, ncand, b);
            sd += dist_of(b, c);
            sl += a.L[(uint64_t)c * n + b];
        }
        floor_d = block_sum(f, red_d);
        short_d = block_sum(sd, red_d);
        short_l = block_sum(sl, red_u);
    }
    const bool feasible = floor_d <= D;
    const bool all_short = feasible && short_d <= D;          // the shortest choice is good enough: no multiplier is finite
    double lambda = 0;
    uint32_t steps = 0;
    if (feasible && !all_short) {
        // bracket within a factor of two, from 1: up while the doubled multiplier still fits, else down until one fits (200 halvings
        // without one: 0, which fits -- its choice has the floor's distortion), then bisect.  lo always fits.
        double lo = 1.0, hi;
        if (dist_at(lo) <= D) {
            while (steps < 200u && dist_at(lo * 2.0) <= D) { lo *= 2.0; ++steps; }
            hi = lo * 2.0;
        } else {
            double at_lo;
            do { lo *= 0.5; ++steps; at_lo = dist_at(lo); } while (steps < 200u && at_lo > D);
            hi = lo * 2.0;
            if (at_lo > D) lo = 0.0;
        }
        for (uint32_t k = 0; k < kRateBisectSteps; ++k, ++steps) {
            const double mid = 0.5 * (lo + hi);
            if (dist_at(mid) <= D) lo = mid; else hi = mid;
        }
        lambda = lo;
    }
    // the choice the trim starts from: the Lagrange choice at lambda; the shortest one; not feasible: every block at its least E
    unsigned long long lagrange;
    double lagrange_d;
    {
        unsigned long long s = 0;
        double d = 0;
        for (uint64_t b = t; b < n; b += kRateAllocThreads) {
            uint32_t c;
            if (all_short) c = rate_shortest(a.L, n, ncand, b);
            else if (feasible) c = rate_choose(a.L, a.E, a.W, n, ncand, b, lambda);
            else { c = 0; for (uint32_t k = 1; k < ncand; ++k) if (a.E[(uint64_t)k * n + b] < a.E[(uint64_t)c * n + b]) c = k; }
            a.drop[b] = (uint8_t)c;
            s += a.L[(uint64_t)c * n + b];
            d += dist_of(b, c);
        }
        lagrange = block_sum(s, red_u);
        lagrange_d = block_sum(d, red_d);
    }
    // the trim, in table order: a block moves to the next coarser candidate while that strictly shortens it and the distortion it
    // adds -- which may be negative -- fits what is left; a block that does not fit is passed over and the walk goes on.  kTrimChunk
    // blocks at a time, in the fill's three phases.
    double left = D - lagrange_d;                                      // (thread 0's is the one that counts)
    for (uint64_t base = 0; feasible && base < n; base += kTrimChunk) {
        const uint64_t b = base + t;
        uint32_t c = 0;
        if (t < kTrimChunk && b < n) {
            c = a.drop[b];
            const double w = a.W[b];
            uint32_t len = 0;
            for (uint32_t s = 0; c + s + 1u < ncand && s < kFillSteps; ++s) {
                const uint64_t fine = (uint64_t)(c + s) * n + b, coarse = (uint64_t)(c + s + 1u) * n + b;
                if (!(a.L[coarse] < a.L[fine])) break;
                trim_delta[t][s] = w * (double)((long long)a.E[coarse] - (long long)a.E[fine]);
                ++len;
            }
            trim_len[t] = (uint8_t)len;
        }
        __syncthreads();
        if (t == 0) {
            const uint32_t cnt = (uint32_t)min((uint64_t)kTrimChunk, n - base);
            for (uint32_t i = 0; i < cnt; ++i) {
                uint32_t k = 0;
                while (k < trim_len[i] && trim_delta[i][k] <= left) { left -= trim_delta[i][k]; ++k; }
                trim_taken[i] = (uint8_t)k;
            }
        }
        __syncthreads();
        if (t < kTrimChunk && b < n) a.drop[b] = (uint8_t)(c + trim_taken[t]);
        __syncthreads();
    }
    // the result, summed afresh over the final choice, and the candidates as the drop bytes the block coder takes
    unsigned long long bytes = 0;
    double dist = 0;
    for (uint64_t b = t; b < n; b += kRateAllocThreads) {
        const uint32_t c = a.drop[b];
        bytes += a.L[(uint64_t)c * n + b];
        dist += dist_of(b, c);
        a.drop[b] = c <= a.dmax ? (uint8_t)c : (uint8_t)kHtDropSkip;
    }
    bytes = block_sum(bytes, red_u);
    dist = block_sum(dist, red_d);
    if (t == 0) {
        a.res->block_bytes = bytes; a.res->lagrange_bytes = lagrange; a.res->shortest_bytes = short_l;
        a.res->distortion = dist; a.res->floor = floor_d; a.res->lambda = all_short ? (double)INFINITY : lambda;
        a.res->feasible = feasible ? 1u : 0u; a.res->steps = steps;
    }
}

} // namespace

hipError_t launch_rate_stats(const RateStatsArgs& a, hipStream_t s)
{
    if (!a.nblocks) return hipSuccess;
    const uint64_t n = a.map ? a.n : a.nblocks;
    if (a.dmax == 0 || a.dmax > kRateMaxDrop || a.nblocks > kRateMaxBlocks || n > kRateMaxBlocks || n < a.nblocks || (a.h16 && a.irreversible))
        return hipErrorInvalidValue;
    const dim3 grid((uint32_t)a.nblocks), block(64);
    if (a.h16) hipLaunchKernelGGL((rate_stats_kernel<int16_t, false>), grid, block, 0, s, (const int16_t*)a.mallat, a.stride, a.pitch, a.blocks, a.blocks_per_tile, a.ncomp, a.nblocks, a.dmax, a.E, a.map, n);
    else if (a.irreversible) hipLaunchKernelGGL((rate_stats_kernel<int32_t, true>), grid, block, 0, s, (const int32_t*)a.mallat, a.stride, a.pitch, a.blocks, a.blocks_per_tile, a.ncomp, a.nblocks, a.dmax, a.E, a.map, n);
    else hipLaunchKernelGGL((rate_stats_kernel<int32_t, false>), grid, block, 0, s, (const int32_t*)a.mallat, a.stride, a.pitch, a.blocks, a.blocks_per_tile, a.ncomp, a.nblocks, a.dmax, a.E, a.map, n);
    return hipGetLastError();
}

hipError_t launch_rate_map(const RateMapArgs& a, hipStream_t s)
{
    if (!a.count) return hipSuccess;
    if (!a.batch || !a.joint || !a.map || !a.per_unit || a.count > kRateMaxBlocks || (a.elem != 1 && a.elem != 4) || (a.gather && a.elem != 1) ||
        (!a.gather && a.elem != 4))
        return hipErrorInvalidValue;
    const dim3 grid((uint32_t)((a.count + 255u) / 256u)), block(256);
    if (a.gather) hipLaunchKernelGGL((rate_map_kernel<uint8_t, true>), grid, block, 0, s, (uint8_t*)a.batch, (uint8_t*)a.joint, a.map, a.per_unit, a.count);
    else hipLaunchKernelGGL((rate_map_kernel<uint32_t, false>), grid, block, 0, s, (uint32_t*)a.batch, (uint32_t*)a.joint, a.map, a.per_unit, a.count);
    return hipGetLastError();
}

hipError_t launch_rate_alloc(const RateAllocArgs& a, hipStream_t s)
{
    if (!a.nblocks || a.nblocks > kRateMaxBlocks || a.dmax == 0 || a.dmax > kRateMaxDrop || a.ncand < a.dmax + 1u || a.ncand > a.dmax + 2u)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(rate_alloc_kernel, dim3(1), dim3(kRateAllocThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_rate_quality(const RateQualityArgs& a, hipStream_t s)
{
    if (!a.nblocks || a.nblocks > kRateMaxBlocks || a.dmax == 0 || a.dmax > kRateMaxDrop || a.ncand < a.dmax + 1u || a.ncand > a.dmax + 2u ||
        !(a.budget >= 0.0))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(rate_quality_kernel, dim3(1), dim3(kRateAllocThreads), 0, s, a);
    return hipGetLastError();
}

} // namespace grk_amd
