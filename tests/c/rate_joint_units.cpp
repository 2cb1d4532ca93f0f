// tests/c/rate_joint_units.cpp -- the host planning of a rate-targeted call's JOINT tables (grok_amd/csrc/encode_plan.cpp:
// plan_rate_joint) behind a C interface for tests/test_rate_subsampled_cpu.py.  Built with g++ together with encode_plan.cpp and
// geometry.cpp: no GPU, no HIP.  With -DRATE_JOINT_MAIN the file is a program of its own that walks the same cases (the sanitizer
// run: -fsanitize=address,undefined) and returns 0 when every one holds.
#include "../../grok_amd/csrc/encode_plan.h"
#include <cstdio>
#include <cstring>

using namespace grk_amd;

extern "C" {

// units: unit_blocks[nunits]; batches: members[] cut by batch_len[nbatches].  Out: first_row[nunits], map[sum of batch_len] (the batches'
// maps one behind the other), per_unit[nbatches], info[6] = n, rows, l_bytes, e_bytes, w_bytes, drop_bytes.  Returns ok.
int rj_plan(uint32_t max_drop, int allow_skip, const uint64_t* unit_blocks, uint32_t nunits, const uint32_t* members, const uint32_t* batch_len,
            uint32_t nbatches, uint64_t* first_row, uint64_t* map, uint32_t* per_unit, uint64_t* info)
{
    std::vector<uint64_t> ub(unit_blocks, unit_blocks + nunits);
    std::vector<std::vector<uint32_t>> batches;
    for (uint32_t k = 0, at = 0; k < nbatches; at += batch_len[k], ++k) batches.emplace_back(members + at, members + at + batch_len[k]);
    const RateJointPlan r = plan_rate_joint(max_drop, allow_skip != 0, ub, batches);
    if (!r.ok) return 0;
    if (r.first_row.size() != nunits || r.map.size() != nbatches || r.per_unit.size() != nbatches) return -1;
    for (uint32_t u = 0; u < nunits; ++u) first_row[u] = r.first_row[u];
    for (uint32_t k = 0, at = 0; k < nbatches; ++k) {
        if (r.map[k].size() != batch_len[k]) return -1;
        for (uint64_t v : r.map[k]) map[at++] = v;
        per_unit[k] = r.per_unit[k];
    }
    info[0] = r.n; info[1] = r.tables.rows; info[2] = r.tables.l_bytes; info[3] = r.tables.e_bytes; info[4] = r.tables.w_bytes;
    info[5] = r.tables.drop_bytes;
    return 1;
}

uint64_t rj_max_blocks(void) { return kRateMaxBlocks; }

}

#ifdef RATE_JOINT_MAIN
namespace {

int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

// every joint row is written by exactly one (batch, member, block), and unit u's rows are first_row[u] .. + unit_blocks[u] in unit order
void check_partition(const std::vector<uint64_t>& ub, const std::vector<std::vector<uint32_t>>& batches, const RateJointPlan& r)
{
    EXPECT(r.ok);
    if (!r.ok) return;
    uint64_t at = 0;
    for (size_t u = 0; u < ub.size(); ++u) { EXPECT(r.first_row[u] == at); at += ub[u]; }
    EXPECT(r.n == at);
    std::vector<uint32_t> hits(r.n, 0);
    for (size_t k = 0; k < batches.size(); ++k) {
        EXPECT(r.map[k].size() == batches[k].size());
        for (size_t i = 0; i < batches[k].size(); ++i) {
            EXPECT(r.map[k][i] == r.first_row[batches[k][i]] && r.per_unit[k] == ub[batches[k][i]]);
            for (uint64_t b = 0; b < r.per_unit[k]; ++b) { EXPECT(r.map[k][i] + b < r.n); if (r.map[k][i] + b < r.n) ++hits[r.map[k][i] + b]; }
        }
    }
    for (uint64_t j = 0; j < r.n; ++j) EXPECT(hits[j] == 1);
    EXPECT(r.tables.l_bytes == (uint64_t)r.tables.rows * r.n * 4 && r.tables.e_bytes == (uint64_t)r.tables.rows * r.n * 8);
    EXPECT(r.tables.w_bytes == r.n * 8 && r.tables.drop_bytes == r.n);
}

} // namespace

int main()
{
    // a 4:2:0 image of 2 x 2 ragged tiles: [tile][run] units, luma and chroma units of four geometries each
    const std::vector<uint64_t> ub = {40, 14, 28, 10, 34, 14, 22, 10};
    const std::vector<std::vector<uint32_t>> by_group = {{0}, {1, 5}, {2}, {3, 7}, {4}, {6}};
    const std::vector<std::vector<uint32_t>> per_unit = {{0}, {1}, {2}, {3}, {4}, {5}, {6}, {7}};
    const std::vector<std::vector<uint32_t>> shuffled = {{7, 3}, {6}, {5, 1}, {4}, {2}, {0}};
    const RateJointPlan a = plan_rate_joint(6, true, ub, by_group), b = plan_rate_joint(6, true, ub, per_unit), c = plan_rate_joint(6, true, ub, shuffled);
    check_partition(ub, by_group, a);
    check_partition(ub, per_unit, b);
    check_partition(ub, shuffled, c);
    EXPECT(a.first_row == b.first_row && b.first_row == c.first_row && a.n == 172 && a.tables.rows == 8);
    // same-geometry units as one batch
    const std::vector<uint64_t> same(6, 21);
    check_partition(same, {{0, 1, 2, 3, 4, 5}}, plan_rate_joint(0, false, same, {{0, 1, 2, 3, 4, 5}}));
    check_partition(same, {{5, 0, 3}, {1, 4, 2}}, plan_rate_joint(12, true, same, {{5, 0, 3}, {1, 4, 2}}));
    // refusals
    EXPECT(!plan_rate_joint(13, true, ub, by_group).ok);                                  // max_drop
    EXPECT(!plan_rate_joint(6, true, {}, {}).ok);
    EXPECT(!plan_rate_joint(6, true, ub, {{0}, {1, 5}, {2}, {3, 7}, {4}}).ok);            // unit 6 in no batch
    EXPECT(!plan_rate_joint(6, true, ub, {{0}, {1, 5}, {2}, {3, 7}, {4}, {6}, {0}}).ok);  // unit 0 twice
    EXPECT(!plan_rate_joint(6, true, ub, {{0, 1}, {5}, {2}, {3, 7}, {4}, {6}}).ok);       // members of different block counts
    EXPECT(!plan_rate_joint(6, true, ub, {{0}, {1, 5}, {2}, {3, 8}, {4}, {6}}).ok);       // no such unit
    EXPECT(!plan_rate_joint(6, true, ub, {{0}, {1, 5}, {2}, {3, 7}, {4}, {6}, {}}).ok);   // an empty batch
    EXPECT(!plan_rate_joint(6, true, {4, 0, 4}, {{0, 2}, {1}}).ok);                       // an empty unit
    // more rows than the kernels index: two units of 2^30 blocks fit, a third does not (nothing of that size is allocated: the plan
    // holds a row per unit, not per block)
    const std::vector<uint64_t> huge2(2, 1ull << 30), huge3(3, 1ull << 30);
    EXPECT(!plan_rate_joint(6, true, huge2, {{0, 1}}).ok);                                // 2^31 > kRateMaxBlocks = 2^31 - 1
    EXPECT(plan_rate_joint(6, true, {(1ull << 30), (1ull << 30) - 1}, {{0}, {1}}).ok);
    EXPECT(!plan_rate_joint(6, true, huge3, {{0, 1, 2}}).ok);
    EXPECT(!plan_rate_joint(6, true, {kRateMaxBlocks + 1}, {{0}}).ok);
    EXPECT(!plan_rate_joint(6, true, {~0ull, 2}, {{0}, {1}}).ok);                         // (no wrap-around of the sum)
    std::printf("rate_joint_units: %d failure(s)\n", failures);
    return failures ? 1 : 0;
}
#endif
