// unit_flush_exact.hip — launch_downdate, the exact fp32 flushes and the fp64 flushes.
#include "ekf_flush_supertile.h"
#include "ekf_flush_wave.h"
#include "ekf_flush_f64.h"
#include "ekf_units.h"

namespace ekf {

hipError_t launch_downdate(const DowndateParams& p, const FlushPlan& plan, int grid, hipStream_t st, hipEvent_t ev_a,
                           hipEvent_t ev_b)
{
    if (p.nsteps != plan.nsteps) return hipErrorInvalidValue;
    const bool half = plan.storage == EKF_PREC_F16;
    const FlushLaunch go{p, flush_grid_size(plan.grid, p.ncu, grid, p.E, p.d.nb), st, ev_a, ev_b};
    switch (plan.family) {
    case FLUSH_F64_WAVE:
        return with_steps<1, F64_WAVE_MAXS, 1>(p.nsteps, [&](auto ns) { go(flush_f64_wave_kernel<decltype(ns)::value>); });
    case FLUSH_F64_TILE: go(downdate_f64_kernel); break;
    case FLUSH_BF16_2X4: return launch_flush_bf24(go, half, false);
    case FLUSH_F16_2X4: return launch_flush_bf24(go, half, true);
    case FLUSH_F16_QUAD: return launch_flush_f16q(go, half);
    case FLUSH_F16_WAVE: return launch_flush_f16x3(go, half);
    case FLUSH_BF16_WAVE: return launch_flush_bf16x6(go, half);
    case FLUSH_F32_WAVE:
        return with_steps<2, F32_WAVE_MAXS, 2>(p.nsteps, [&](auto ns) {
            constexpr int NS = decltype(ns)::value;
            go(half ? flush_f32_wave_kernel<_Float16, NS> : flush_f32_wave_kernel<float, NS>);
        });
    case FLUSH_F32_PERSIST: go(half ? flush_f32_persist2_kernel<_Float16> : flush_f32_persist2_kernel<float>); break;
    case FLUSH_F32_SUPERTILE: go(half ? flush_f32_sb_kernel<_Float16> : flush_f32_sb_kernel<float>); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace ekf
