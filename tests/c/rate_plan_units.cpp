// tests/c/rate_plan_units.cpp -- the host planning of rate-targeted encodes (grok_amd/csrc/encode_plan.cpp: plan_ht_drop_instance,
// plan_rate, the drop byte <-> zero-bit-plane rules) behind a C interface for tests/test_rate_writer_cpu.py.  Built with g++ together
// with encode_plan.cpp and geometry.cpp: no GPU, no HIP.
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

}
