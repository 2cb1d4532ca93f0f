// tools/t2_keep_time.hip -- KK (grok_amd/csrc/kernels_t2keep.hip) alone beside a plain device-to-device copy of the same bytes: a batch
// of one unit whose arena holds `bytes` coded bytes (default: an 8K NV12 frame's 23.7 MB) in `rows` blocks (default 8 192), kept into
// an image-wide arena.  Medians, minima and maxima of 21 launches each, taken in turn, timed with events on one stream.
//
//     hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/t2_keep_time.hip -o build/t2_keep_time && build/t2_keep_time [bytes] [rows]
#include "../grok_amd/csrc/kernels_t2keep.hip"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace grk_amd;

#define TRY(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { std::printf("%s: %s\n", #call, hipGetErrorString(e_)); return 1; } } while (0)

int main(int argc, char** argv)
{
    const uint64_t bytes = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 23716435ull;
    const uint32_t rows = argc > 2 ? (uint32_t)std::strtoul(argv[2], nullptr, 10) : 8192u;
    if (!bytes || !rows || bytes >> 32) { std::printf("usage: t2_keep_time [bytes < 4 GB] [rows]\n"); return 2; }
    const uint64_t bound = (bytes + 15u) & ~15ull;
    // the batch: blocks back to back, the last one takes the remainder
    std::vector<uint32_t> len(rows, (uint32_t)(bytes / rows));
    std::vector<unsigned long long> off(rows);
    len[rows - 1] += (uint32_t)(bytes % rows);
    for (uint32_t i = 0; i < rows; ++i) off[i] = (unsigned long long)(bytes / rows) * i;
    const unsigned long long state[2] = {0, bytes}, row_at[1] = {0}, cursors0[2] = {0, 0};
    void *d_len, *d_off, *d_arena, *d_state, *d_rowat, *j_len, *j_off, *j_arena, *d_cursors, *d_status, *d_plain;
    TRY(hipMalloc(&d_len, rows * 4)); TRY(hipMalloc(&d_off, rows * 8)); TRY(hipMalloc(&d_arena, bound)); TRY(hipMalloc(&d_state, 16));
    TRY(hipMalloc(&d_rowat, 8)); TRY(hipMalloc(&j_len, rows * 4)); TRY(hipMalloc(&j_off, rows * 8)); TRY(hipMalloc(&j_arena, bound));
    TRY(hipMalloc(&d_cursors, 16)); TRY(hipMalloc(&d_status, 16)); TRY(hipMalloc(&d_plain, bound));
    TRY(hipMemcpy(d_len, len.data(), rows * 4, hipMemcpyHostToDevice)); TRY(hipMemcpy(d_off, off.data(), rows * 8, hipMemcpyHostToDevice));
    TRY(hipMemcpy(d_state, state, 16, hipMemcpyHostToDevice)); TRY(hipMemcpy(d_rowat, row_at, 8, hipMemcpyHostToDevice));
    TRY(hipMemcpy(d_cursors, cursors0, 16, hipMemcpyHostToDevice));
    TRY(hipMemset(d_status, 0, 16)); TRY(hipMemset(d_arena, 0x5A, bound));
    T2KeepArgs a{};
    a.lengths = (const uint32_t*)d_len; a.offsets = (const unsigned long long*)d_off; a.arena = (const uint8_t*)d_arena; a.arena_bound = bound;
    a.batch_state = (const unsigned long long*)d_state; a.nunits = 1; a.bpu = rows; a.row_at = (const unsigned long long*)d_rowat;
    a.j_lengths = (uint32_t*)j_len; a.j_offsets = (unsigned long long*)j_off; a.j_arena = (uint8_t*)j_arena; a.j_cap = bound;
    a.cursors = (unsigned long long*)d_cursors; a.status = (unsigned int*)d_status;
    hipStream_t st;
    hipEvent_t e0, e1;
    TRY(hipStreamCreate(&st)); TRY(hipEventCreate(&e0)); TRY(hipEventCreate(&e1));
    std::vector<float> keep, plain;
    for (int i = 0; i < 24; ++i) {
        float ms = 0;
        TRY(hipEventRecord(e0, st)); TRY(launch_t2_keep(a, st)); TRY(hipEventRecord(e1, st)); TRY(hipEventSynchronize(e1));
        TRY(hipEventElapsedTime(&ms, e0, e1));
        if (i >= 3) keep.push_back(ms);
        TRY(hipEventRecord(e0, st)); TRY(hipMemcpyAsync(d_plain, d_arena, bound, hipMemcpyDeviceToDevice, st)); TRY(hipEventRecord(e1, st));
        TRY(hipEventSynchronize(e1)); TRY(hipEventElapsedTime(&ms, e0, e1));
        if (i >= 3) plain.push_back(ms);
    }
    unsigned int status = 0;
    std::vector<uint8_t> back(bound);
    TRY(hipMemcpy(&status, d_status, 4, hipMemcpyDeviceToHost)); TRY(hipMemcpy(back.data(), j_arena, bound, hipMemcpyDeviceToHost));
    for (uint64_t i = 0; i < bytes; ++i) if (back[i] != 0x5A) { std::printf("the kept bytes differ at %llu\n", (unsigned long long)i); return 1; }
    if (status) { std::printf("status %u\n", status); return 1; }
    auto show = [&](const char* what, std::vector<float>& v) {
        std::sort(v.begin(), v.end());
        const float med = v[v.size() / 2];
        std::printf("    %-58s min %7.4f  median %7.4f  max %7.4f ms   %7.1f GB/s copied at the median\n", what, v.front(), med, v.back(), bytes / med / 1e6);
    };
    std::printf("# tools/t2_keep_time: %llu bytes in %u rows, 21 launches each, in turn\n", (unsigned long long)bytes, rows);
    show("KK t2_keep_kernel (rows + bytes)", keep);
    show("hipMemcpyAsync device to device of the same bytes", plain);
    return 0;
}
