// unit_flush_2x4.hip — the 2 × 4 wave-tile flushes.
#include "ekf_flush_2x4.h"
#include "ekf_units.h"

namespace ekf {

// the 2 × 4 wave-tile forms (EKF_OPT_FLUSH_FORM = 24): split-bf16 (measured 7 % slower than the
// 2 × 2 form at T = 12; kept as an option, bit-identical) and split-fp16
hipError_t launch_flush_bf24(const FlushLaunch& go, bool half, bool f16)
{
    if (!f16)
        return with_steps<2, BF16X6_MAXS, 2>(go.p.nsteps, [&](auto ns) {
            constexpr int NS = decltype(ns)::value;
            go(half ? flush_bf24_kernel<_Float16, NS> : flush_bf24_kernel<float, NS>);
        });
    return with_steps<2, F16X3_MAXS, 2>(go.p.nsteps, [&](auto ns) {
        constexpr int NS = decltype(ns)::value;
        go(half ? flush_bf24_kernel<_Float16, NS, true> : flush_bf24_kernel<float, NS, true>);
    });
}

}  // namespace ekf
