// unit_flush_quad.hip — the split-fp16 quad flush.
#include "ekf_flush_quad.h"
#include "ekf_units.h"

namespace ekf {

hipError_t launch_flush_f16q(const FlushLaunch& go, bool half)
{
    return with_steps<QUAD_MINS, F16X3_MAXS, 2>(go.p.nsteps, [&](auto ns) {
        constexpr int NS = decltype(ns)::value;
        go(half ? flush_f16q_kernel<_Float16, NS> : flush_f16q_kernel<float, NS>, 64 * Q_WAVES);
    });
}

}  // namespace ekf
