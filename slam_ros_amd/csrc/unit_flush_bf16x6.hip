// unit_flush_bf16x6.hip — the split-bf16 wave flush.
#include "ekf_flush_wave.h"
#include "ekf_units.h"

namespace ekf {

hipError_t launch_flush_bf16x6(const FlushLaunch& go, bool half)
{
    return with_steps<2, BF16X6_MAXS, 2>(go.p.nsteps, [&](auto ns) {
        constexpr int NS = decltype(ns)::value;
        go(half ? flush_f32_wave_kernel<_Float16, NS, true> : flush_f32_wave_kernel<float, NS, true>);
    });
}

}  // namespace ekf
