// ekf_units.h — what the compilation units of the kernels share on the host side: the launchers
// one unit defines and another calls, and the flush launch helpers.
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <type_traits>

#include "ekf_kernels.h"

namespace ekf {

// The association kernel on 128 / 64 landmarks per workgroup (ScanParams::nt): its HOT
// instantiations (symmetric fp32 operands, kmax = 16; HOT = 2 split-fp16, 1 the others), one
// compilation unit per width
hipError_t launch_scan_nt128(const ScanParams& p, bool half, bool f16x3, hipStream_t st);
hipError_t launch_scan_nt64(const ScanParams& p, bool half, bool f16x3, hipStream_t st);

// The flush launchers. flush_plan (ekf_flush_plan.h) decides the kernel: launch_downdate switches on the
// plan, each launcher turns its step count into the template argument. The split-arithmetic launchers
// are one compilation unit each (their instantiations are most of the device code).

// One flush launch, timed by the dispatch packet itself when ev_a / ev_b are given
struct FlushLaunch {
    const DowndateParams& p;
    unsigned grid;
    hipStream_t st;
    hipEvent_t ev_a, ev_b;
    template <typename K>
    void operator()(K kernel, unsigned block = DD_THREADS) const
    {
        hipExtLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, st, ev_a, ev_b, 0, p);
    }
};

// f(std::integral_constant<int, NS>) for the NS of LO, LO + STEP, ..., HI that equals nsteps, or an error.
// Counts down: the innermost instantiation is emitted first, so a unit's kernels stay in ascending order
template <int LO, int HI, int STEP, typename F>
static hipError_t with_steps(int nsteps, F&& f)
{
    static_assert(HI < LO || (HI - LO) % STEP == 0, "HI is one of the steps");
    if constexpr (HI < LO) {
        return hipErrorInvalidValue;
    } else {
        if (nsteps != HI) return with_steps<LO, HI - STEP, STEP>(nsteps, f);
        f(std::integral_constant<int, HI>{});
        return hipGetLastError();
    }
}

hipError_t launch_flush_bf24(const FlushLaunch& go, bool half, bool f16);
hipError_t launch_flush_f16x3(const FlushLaunch& go, bool half);
hipError_t launch_flush_bf16x6(const FlushLaunch& go, bool half);
hipError_t launch_flush_f16q(const FlushLaunch& go, bool half);

}  // namespace ekf
