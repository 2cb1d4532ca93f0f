// tests/c/rate_plan_units.cpp -- the host planning of rate-targeted encodes (grok_amd/csrc/encode_plan.cpp: plan_ht_drop_instance,
// plan_rate, the drop byte <-> zero-bit-plane rules, the budgets of a whole-image call's rounds and the split route's shares of them)
// behind a C interface for tests/test_rate_writer_cpu.py.  Built with g++ together with encode_plan.cpp and geometry.cpp: no GPU, no
// HIP.  -DRATE_PLAN_MAIN: a program of its own that walks chosen cases (run under AddressSanitizer and UBSan).
#include "../../grok_amd/csrc/encode_plan.h"

using namespace grk_amd;

extern "C" {

// out: ok, irrev, h16
void rp_drop_instance(int irreversible, int h16, uint32_t* out)
{
    const HtDropPlan p = plan_ht_drop_instance(irreversible != 0, h16 != 0);
    out[0] = p.ok; out[1] = p.inst.irrev; out[2] = p.inst.h16;
}

// out: ok, dmax, rows, ncand, trials, l_bytes, e_bytes, w_bytes, drop_bytes
void rp_rate(uint32_t max_drop, int allow_skip, uint64_t nblocks, uint64_t* out)
{
    const RatePlan r = plan_rate(max_drop, allow_skip != 0, nblocks);
    out[0] = r.ok; out[1] = r.dmax; out[2] = r.rows; out[3] = r.ncand; out[4] = r.trials;
    out[5] = r.l_bytes; out[6] = r.e_bytes; out[7] = r.w_bytes; out[8] = r.drop_bytes;
}

uint32_t rp_drop_byte(uint32_t c, uint32_t dmax) { return rate_drop_byte(c, dmax); }
uint32_t rp_missing_msbs(uint32_t kmax, uint32_t drop) { return drop_missing_msbs(kmax, drop); }

// out: skip byte, default Dmax, largest Dmax, candidates at most, allocator threads, bisection steps, rounds
void rp_constants(uint32_t* out)
{
    out[0] = kHtDropSkip; out[1] = kRateDefaultDrop; out[2] = kRateMaxDrop; out[3] = kRateMaxCand; out[4] = kRateAllocThreads;
    out[5] = kRateBisectSteps; out[6] = kRateMaxRounds;
}

// out: the n groups' shares
void rp_group_shares(uint64_t budget, uint32_t n, const uint64_t* samples, const uint64_t* plain, uint64_t* out)
{
    const std::vector<uint64_t> share = group_shares(budget, std::vector<uint64_t>(samples, samples + n), std::vector<uint64_t>(plain, plain + n));
    for (uint32_t k = 0; k < n; ++k) out[k] = share[k];
}

uint64_t rp_first_budget(uint64_t target, uint64_t plain_file, uint64_t plain_blocks) { return rate_first_budget(target, plain_file, plain_blocks); }

// -> 1 and *next, or 0: nothing left to take from the blocks
int rp_next_budget(uint64_t budget, uint64_t block_bytes, uint64_t file_bytes, uint64_t target, uint64_t* next)
{
    const RateNextBudget r = rate_next_budget(budget, block_bytes, file_bytes, target);
    *next = r.budget;
    return r.left ? 1 : 0;
}

}

#ifdef RATE_PLAN_MAIN
#include <cstdio>

namespace {

int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

typedef std::vector<uint64_t> V;

// the invariants of any answer: no share above the group's plain bytes, the sum min(budget, all plain bytes)
void check_shares(uint64_t budget, const V& samples, const V& plain, const V* want = nullptr)
{
    const V share = group_shares(budget, samples, plain);
    EXPECT(share.size() == samples.size());
    unsigned __int128 sum = 0, all = 0;
    for (size_t k = 0; k < share.size(); ++k) { EXPECT(share[k] <= plain[k]); sum += share[k]; all += plain[k]; }
    EXPECT(sum == (all < budget ? all : (unsigned __int128)budget));
    if (want) EXPECT(share == *want);
}

} // namespace

int main()
{
    const V samples = {64 * 48 * 3, 36 * 48 * 3, 64 * 28 * 3, 36 * 28 * 3}, plain = {5000, 3100, 2900, 1700};
    // at and above all the plain bytes: every group its own; one below: still nobody above its own
    check_shares(12700, samples, plain, &plain);
    check_shares(1ull << 40, samples, plain, &plain);
    check_shares(~0ull, samples, plain, &plain);
    check_shares(12699, samples, plain);
    check_shares(0, samples, plain);
    check_shares(6350, samples, plain);
    // a group without plain bytes takes nothing; one group takes what there is, up to its own
    { const V p = {5000, 0, 2900, 1700}; check_shares(4000, samples, p); EXPECT(group_shares(4000, samples, p)[1] == 0); }
    { const V one = {777}, s = {5}, w1 = {700}, w2 = {777}; check_shares(700, s, one, &w1); check_shares(778, s, one, &w2); }
    // every floor division inexact; the remainder of the rounding on the last group must not lift it above its plain bytes
    { const V s = {1, 1, 1}, p = {2, 2, 2}; check_shares(5, s, p); }
    { const V s = {3, 5, 7}, p = {1000, 1000, 1000}; const V w = {200, 333, 468}; check_shares(1001, s, p, &w); }
    // products beyond 2^64
    { const V s = {(1ull << 40) + 1, (1ull << 41) + 3, 7}, p = {1ull << 62, 1ull << 61, 1ull << 60}; check_shares((1ull << 62) + 12345, s, p); check_shares(~0ull, s, p, &p); }
    // the rounds' budgets
    EXPECT(rate_first_budget(2000, 1000, 900) == 900 && rate_first_budget(1000, 1000, 900) == 900);     // at or above the plain file: all blocks
    EXPECT(rate_first_budget(999, 1000, 900) == 899 && rate_first_budget(101, 1000, 900) == 1);
    EXPECT(rate_first_budget(100, 1000, 900) == 0 && rate_first_budget(0, 1000, 900) == 0);             // the headers alone
    { const RateNextBudget r = rate_next_budget(500, 480, 640, 600); EXPECT(r.left && r.budget == 440); }
    { const RateNextBudget r = rate_next_budget(500, 480, 2000, 600); EXPECT(r.left && r.budget == 0); }
    EXPECT(!rate_next_budget(0, 0, 640, 600).left && !rate_next_budget(0, 10, 640, 600).left && !rate_next_budget(10, 0, 640, 600).left);
    // any overshoots: the budget falls by one at least per round, down to 0, after which nothing is left
    uint64_t budget = 1000, seed = 1;
    for (uint32_t round = 0; ; ++round) {
        seed = seed * 6364136223846793005ull + 1442695040888963407ull;
        const uint64_t blocks = budget - (seed >> 33) % (budget / 4 + 1), over = 1 + (seed >> 50) % 5;
        const RateNextBudget r = rate_next_budget(budget, blocks, 600 + over, 600);
        if (!r.left) { EXPECT(budget == 0 || blocks == 0); break; }
        EXPECT(r.budget < budget && round < 1001);
        if (round >= 1001) break;
        budget = r.budget;
    }
    std::printf("rate_plan_units: %d failure(s)\n", failures);
    return failures ? 1 : 0;
}
#endif
