// tests/c/pipeline_plan_units.cpp -- the pipelined encode's host planning (grok_amd/csrc/encode_plan.cpp: ht_class_stream with a frame
// parity) behind plain C entry points, for tests/test_pipeline_plan_cpu.py: built at test time with g++ together with
// encode_plan.cpp and geometry.cpp, no GPU, no HIP.
#include "../../grok_amd/csrc/encode_plan.h"
#include <algorithm>

using namespace grk_amd;

extern "C" {
// -> HtStream (0 not here, 1 main, 2 side, 3 side2)
int pp_class_stream(int role, int overlapped, int pipelined, int at, int one_level, uint32_t parity)
{
    return (int)ht_class_stream((HtRole)role, overlapped != 0, pipelined != 0, (HtPoint)at, one_level != 0, parity);
}
// the same through the five-argument call every other caller makes
int pp_class_stream_default(int role, int overlapped, int pipelined, int at, int one_level)
{
    return (int)ht_class_stream((HtRole)role, overlapped != 0, pipelined != 0, (HtPoint)at, one_level != 0);
}
// row i of kHtSchedule: {role, overlapped, pipelined (-1: either), at, to}; returns the number of rows
int pp_schedule_row(uint32_t i, int* out)
{
    const uint32_t n = sizeof(kHtSchedule) / sizeof(kHtSchedule[0]);
    if (i < n) {
        const HtScheduleRow& r = kHtSchedule[i];
        out[0] = (int)r.role; out[1] = r.overlapped; out[2] = r.pipelined; out[3] = (int)r.at; out[4] = (int)r.to;
    }
    return (int)n;
}
} // extern "C"
