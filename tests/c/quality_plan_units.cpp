// tests/c/quality_plan_units.cpp -- the host planning of quality-targeted encodes (grok_amd/csrc/encode_plan.cpp: plan_quality,
// quality_samples, quality_psnr) behind a C interface for tests/test_quality_plan_cpu.py.  Built with g++ together with
// encode_plan.cpp and geometry.cpp: no GPU, no HIP.
#include "../../grok_amd/csrc/encode_plan.h"

using namespace grk_amd;

extern "C" {

// out: budget, signal; returns ok
int qp_quality(double target_psnr, double target_distortion, uint32_t prec, uint64_t samples, double* out)
{
    const QualityPlan r = plan_quality(target_psnr, target_distortion, prec, samples);
    out[0] = r.budget; out[1] = r.signal;
    return r.ok ? 1 : 0;
}

// area: x0, y0, x1, y1, tx0, ty0, t_width, t_height; comp_dx / comp_dy: null for full-resolution components
uint64_t qp_samples(const uint32_t* area, uint32_t num_comps, const uint8_t* comp_dx, const uint8_t* comp_dy)
{
    const grk_amd_image_layout im{area[0], area[1], area[2], area[3], area[4], area[5], area[6], area[7]};
    return quality_samples(im, num_comps, comp_dx, comp_dy);
}

double qp_psnr(double signal, double distortion) { return quality_psnr(signal, distortion); }

}
