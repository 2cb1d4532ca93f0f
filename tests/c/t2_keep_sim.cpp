// tests/c/t2_keep_sim.cpp -- KK (grok_amd/csrc/kernels_t2keep.hip) compiled as host C++ against tests/c/hip_sim and run thread after
// thread, for tests/test_t2_joint_plan_cpu.py: a sequence of batches kept into image-wide tables and an image-wide arena, against a
// plain loop.  Every buffer is a heap block of exactly its size, so with -fsanitize=address,undefined an access outside it, or a
// 16-byte access off its alignment, ends the program.  The sequences: batches with one unit per tile; batches with two units of one
// tile; one unit alone; blocks of length zero; lengths that are no multiple of 16 at odd offsets; a batch whose cursor lies beyond
// what the image's arena was sized for (status bit 0, nothing copied, the rows empty).  Prints "ok: N batches"; exit status 1 with the
// case on a mismatch.
#include <hip/hip_runtime.h>
static inline unsigned int atomicOr(unsigned int* p, unsigned int v) { const unsigned int o = *p; *p = o | v; return o; }
#include "../../grok_amd/csrc/kernels_t2keep.hip"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>
using namespace grk_amd;

static std::mt19937 rng(7);
static long batches_run = 0;

struct Batch { std::vector<uint32_t> units; uint32_t bpu; bool overflow; };

static void* block(size_t n)
{
    void* p = aligned_alloc(16, n ? (n + 15) & ~(size_t)15 : 16);        // (the sanitizer's red zone starts at n rounded up to 16: the arenas' sizes are multiples)
    if (!p) { printf("no memory\n"); exit(2); }
    return p;
}

// `unit_rows[u]`: unit u's rows in the image's tables (any order of the units); the batches name their units
static void run(const char* name, const std::vector<uint32_t>& unit_rows_count, const std::vector<Batch>& batches, bool odd)
{
    const size_t nunits = unit_rows_count.size(), nb = batches.size();
    std::vector<uint64_t> unit_row(nunits + 1, 0);
    for (size_t u = 0; u < nunits; ++u) unit_row[u + 1] = unit_row[u] + unit_rows_count[u];
    const uint64_t rows = unit_row[nunits];
    // the image's buffers, sized as the host sizes them: from the batches' bounds
    std::vector<uint64_t> bound(nb), used(nb);
    std::vector<std::vector<uint32_t>> len(nb);
    std::vector<std::vector<unsigned long long>> off(nb);
    uint64_t j_cap = 0;
    for (size_t b = 0; b < nb; ++b) {
        const size_t n = batches[b].units.size() * (size_t)batches[b].bpu;
        uint64_t at = odd ? 1 + rng() % 5 : 0;
        len[b].resize(n); off[b].resize(n);
        std::vector<size_t> order(n);
        for (size_t i = 0; i < n; ++i) order[i] = i;
        std::shuffle(order.begin(), order.end(), rng);              // (K3's allocator hands out places in no particular order)
        for (size_t i : order) {
            const uint32_t kind = rng() % 8;
            len[b][i] = kind == 0 ? 0u : kind < 4 ? 1u + rng() % 31 : 1u + rng() % 700;
            off[b][i] = at;
            at += len[b][i] + (odd ? rng() % 7 : 0);
        }
        used[b] = at;
        bound[b] = batches[b].overflow ? (used[b] & ~15ull) / 2 & ~15ull : ((used[b] + 15) & ~15ull) + 16 * (rng() % 3);
        j_cap += bound[b];
    }
    uint32_t* const j_len = (uint32_t*)block(rows * 4);
    unsigned long long* const j_off = (unsigned long long*)block(rows * 8);
    uint8_t* const j_arena = (uint8_t*)block(j_cap);
    unsigned long long* const cursors = (unsigned long long*)block((nb + 1) * 8);
    unsigned int* const status = (unsigned int*)block(4);
    for (uint64_t i = 0; i < rows; ++i) { j_len[i] = 0xDEADBEEFu; j_off[i] = ~0ull; }
    for (uint64_t i = 0; i < j_cap; ++i) j_arena[i] = 0xA5;
    for (size_t b = 0; b <= nb; ++b) cursors[b] = b ? ~0ull : 0;
    *status = 0;
    // the reference: a plain loop
    std::vector<uint32_t> want_len(rows, 0xDEADBEEFu);
    std::vector<uint64_t> want_off(rows, ~0ull);
    std::vector<std::vector<uint8_t>> arenas(nb);
    uint64_t base = 0, bound_at = 0;
    unsigned int want_status = 0;
    for (size_t b = 0; b < nb; ++b) {
        const Batch& B = batches[b];
        const size_t n = B.units.size() * (size_t)B.bpu;
        // the batch's arena: exactly its bound (a multiple of 16) -- or, overflowed, as large as what the cursor claims
        const size_t asize = std::max<uint64_t>(bound[b], B.overflow ? used[b] : 0);
        uint8_t* const arena = (uint8_t*)block(asize);
        for (size_t i = 0; i < asize; ++i) arena[i] = (uint8_t)rng();
        arenas[b].assign(arena, arena + asize);
        unsigned long long* const state = (unsigned long long*)block(16);
        const unsigned int bits = b % 3 == 1 ? 2u : 0u;             // (a batch with a status bit of K3's own)
        state[0] = bits; state[1] = used[b];
        unsigned long long* const row_at = (unsigned long long*)block(B.units.size() * 8);
        for (size_t i = 0; i < B.units.size(); ++i) row_at[i] = unit_row[B.units[i]];
        uint32_t* const d_len = (uint32_t*)block(n * 4);
        unsigned long long* const d_off = (unsigned long long*)block(n * 8);
        for (size_t i = 0; i < n; ++i) { d_len[i] = len[b][i]; d_off[i] = off[b][i]; }
        T2KeepArgs a{};
        a.lengths = d_len; a.offsets = d_off; a.arena = arena; a.arena_bound = bound[b]; a.batch_state = state;
        a.nunits = (uint32_t)B.units.size(); a.bpu = B.bpu; a.row_at = row_at;
        a.j_lengths = j_len; a.j_offsets = j_off; a.j_arena = j_arena; a.j_cap = bound_at + bound[b];
        a.cursors = cursors + b; a.status = status;
        if (launch_t2_keep(a, nullptr) != hipSuccess) { printf("a launch was refused\n"); exit(2); }
        want_status |= bits | (B.overflow ? 1u : 0u);
        for (size_t i = 0; i < n; ++i) {
            const uint64_t j = unit_row[B.units[i / B.bpu]] + i % B.bpu;
            want_len[j] = B.overflow ? 0 : len[b][i];
            want_off[j] = base + (B.overflow ? 0 : off[b][i]);
            if (B.overflow) continue;
            if (memcmp(j_arena + want_off[j], arena + off[b][i], len[b][i])) { printf("MISMATCH %s: batch %zu, block %zu: bytes\n", name, b, i); exit(1); }
        }
        if (!B.overflow) base += (used[b] + 15) & ~15ull;
        bound_at += bound[b];
        if (cursors[b + 1] != base) { printf("MISMATCH %s: batch %zu: cursor %llu, expected %llu\n", name, b, cursors[b + 1], (unsigned long long)base); exit(1); }
        free(arena); free(state); free(row_at); free(d_len); free(d_off);
        ++batches_run;
    }
    for (uint64_t j = 0; j < rows; ++j)
        if (j_len[j] != want_len[j] || j_off[j] != want_off[j]) { printf("MISMATCH %s: row %llu\n", name, (unsigned long long)j); exit(1); }
    if (*status != want_status) { printf("MISMATCH %s: status %u, expected %u\n", name, *status, want_status); exit(1); }
    // the blocks' bytes again at the end: no later batch wrote over an earlier one's
    for (size_t b = 0; b < nb; ++b)
        for (size_t i = 0; i < len[b].size() && !batches[b].overflow; ++i) {
            const uint64_t j = unit_row[batches[b].units[i / batches[b].bpu]] + i % batches[b].bpu;
            if (memcmp(j_arena + j_off[j], arenas[b].data() + off[b][i], len[b][i])) { printf("MISMATCH %s: batch %zu, block %zu: bytes at the end\n", name, b, i); exit(1); }
        }
    free(j_len); free(j_off); free(j_arena); free(cursors); free(status);
}

int main()
{
    for (int rep = 0; rep < 6; ++rep)
        for (bool odd : {false, true}) {
            // 3 tiles x 2 runs (luma 40 rows, chroma 2 x 7): units t * 2 + k; a batch per run
            run("a batch per run", {40, 14, 40, 14, 40, 14}, {Batch{{0, 2, 4}, 40, false}, Batch{{1, 3, 5}, 14, false}}, odd);
            // Y / CbCr / A: 2 tiles x 3 runs, Y and A in one group -- one batch holds two units of each tile
            run("two units of a tile", {25, 12, 25, 25, 12, 25}, {Batch{{0, 2, 3, 5}, 25, false}, Batch{{1, 4}, 12, false}}, odd);
            // a group split over batches: in-place units one by one, then the rest
            run("units one by one", {9, 4, 9, 4}, {Batch{{0}, 9, false}, Batch{{2}, 9, false}, Batch{{1, 3}, 4, false}}, odd);
            run("one unit alone", {1}, {Batch{{0}, 1, false}}, odd);
            run("many rows", {3000, 1}, {Batch{{1}, 1, false}, Batch{{0}, 3000, false}}, odd);
            run("a cursor beyond the bound", {30, 8, 30, 8}, {Batch{{0, 2}, 30, false}, Batch{{1, 3}, 8, true}}, odd);
        }
    printf("ok: %ld batches\n", batches_run);
    return 0;
}
