// tests/c/reader_hostile.cpp -- drives grk_amd_read_header + grk_amd_read_packets (host code only) over hostile input: every
// prefix of a codestream and seeded single-byte corruptions of it, each mapped so that it ENDS at a page boundary with an
// inaccessible page behind it -- a read past the end is a fault, which the test that runs this as a child process sees as a
// failed assertion.  Usage: reader_hostile <libgrok_amd.so> <file.j2k> <corruptions> <seed>; exit status 0 and a summary line when
// every result was a clean table or a negative code.
#include "grok_amd.h"
#include <dlfcn.h>
#include <sys/mman.h>
#include <unistd.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

typedef int (*read_header_fn)(const uint8_t*, uint64_t, grk_amd_stream_info*);
typedef int64_t (*read_packets_fn)(const uint8_t*, uint64_t, const grk_amd_stream_info*, uint32_t, grk_amd_coded_block*, uint64_t, uint32_t*,
                                   grk_amd_segment*, uint64_t, uint64_t*, grk_amd_tp_segment*, uint64_t, uint64_t*, uint64_t*);

static read_header_fn rh;
static read_packets_fn rp;
static long counts[3];                       // clean tables, refusals, tables that break a promise

// 0: refused, 1: a clean table; 2: a table that does not keep what the header promises
static int one(const uint8_t* cs, uint64_t len, uint32_t threads)
{
    grk_amd_stream_info info;
    if (rh(cs, len, &info) != 0) return 0;
    uint64_t nseg = 0, nmov = 0, app = 0;
    const int64_t n = rp(cs, len, &info, threads, nullptr, 0, nullptr, nullptr, 0, &nseg, nullptr, 0, &nmov, &app);
    if (n < 0) return 0;
    std::vector<grk_amd_coded_block> rows((size_t)n + 1);
    std::vector<uint32_t> first((size_t)n + 1);
    std::vector<grk_amd_segment> segs((size_t)nseg + 1);
    std::vector<grk_amd_tp_segment> moves((size_t)nmov + 1);
    const int64_t m = rp(cs, len, &info, threads, rows.data(), (uint64_t)n, first.data(), segs.data(), nseg, &nseg, moves.data(), nmov, &nmov, &app);
    if (m != n) return 2;
    for (int64_t i = 0; i < n; ++i) {
        const uint64_t o = rows[i].offset, l = rows[i].length;
        if (o > len + app || l > len + app - o) return 2;             // every block inside cs + appendix
        if (o < len && l > len - o) return 2;                         // ... and not across their seam
    }
    for (uint64_t i = 0; i < nmov; ++i)
        if (moves[i].src > len || moves[i].len > len - moves[i].src || moves[i].dst > app || moves[i].len > app - moves[i].dst) return 2;
    if (first[n] != nseg) return 2;
    return 1;
}

int main(int argc, char** argv)
{
    if (argc < 5) return 2;
    void* lib = dlopen(argv[1], RTLD_NOW);
    if (!lib) { std::fprintf(stderr, "%s\n", dlerror()); return 2; }
    rh = (read_header_fn)dlsym(lib, "grk_amd_read_header");
    rp = (read_packets_fn)dlsym(lib, "grk_amd_read_packets");
    if (!rh || !rp) return 2;
    FILE* f = std::fopen(argv[2], "rb");
    if (!f) return 2;
    std::vector<uint8_t> cs;
    for (int ch; (ch = std::fgetc(f)) != EOF;) cs.push_back((uint8_t)ch);
    std::fclose(f);
    const long ncorrupt = std::atol(argv[3]);
    uint64_t seed = (uint64_t)std::atoll(argv[4]) * 2654435761u + 1;
    const size_t page = (size_t)sysconf(_SC_PAGESIZE), span = (cs.size() + page - 1) / page * page;
    uint8_t* map = (uint8_t*)mmap(nullptr, span + page, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
    if (map == MAP_FAILED || mprotect(map + span, page, PROT_NONE) != 0) return 2;
    // the whole stream first: it has to read clean
    uint8_t* at = map + span - cs.size();
    std::memcpy(at, cs.data(), cs.size());
    if (one(at, cs.size(), 1) != 1) { std::fprintf(stderr, "the intact stream does not read clean\n"); return 3; }
    for (size_t n = 0; n < cs.size(); ++n) {           // every prefix, its last byte the last accessible one
        at = map + span - n;
        std::memcpy(at, cs.data(), n);
        counts[one(at, n, 1 + (uint32_t)(n % 3))]++;
    }
    at = map + span - cs.size();
    for (long k = 0; k < ncorrupt; ++k) {
        std::memcpy(at, cs.data(), cs.size());
        seed = seed * 6364136223846793005ull + 1442695040888963407ull;
        const size_t where = (size_t)((seed >> 33) % cs.size());
        seed = seed * 6364136223846793005ull + 1442695040888963407ull;
        // half of them in the first 200 bytes, where the headers are
        const size_t w = (k & 1) ? where % (cs.size() < 200 ? cs.size() : 200) : where;
        at[w] ^= (uint8_t)(1u << ((seed >> 40) & 7u)) | (uint8_t)(((seed >> 50) & 1u) ? (seed >> 20) : 0);
        counts[one(at, cs.size(), 1 + (uint32_t)(k % 4))]++;
    }
    std::printf("clean %ld refused %ld broken %ld\n", counts[1], counts[0], counts[2]);
    return counts[2] ? 4 : 0;
}
