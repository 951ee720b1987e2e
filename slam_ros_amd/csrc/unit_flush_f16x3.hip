// unit_flush_f16x3.hip — the split-fp16 wave flush.
#include "ekf_flush_wave.h"
#include "ekf_units.h"

namespace ekf {

hipError_t launch_flush_f16x3(const FlushLaunch& go, bool half)
{
    return with_steps<2, F16X3_MAXS, 2>(go.p.nsteps, [&](auto ns) {
        constexpr int NS = decltype(ns)::value;
        go(half ? flush_f32_wave_kernel<_Float16, NS, true, true> : flush_f32_wave_kernel<float, NS, true, true>);
    });
}

}  // namespace ekf
