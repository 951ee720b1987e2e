// unit_scan_nt128.hip — the association kernel on 128 landmarks per workgroup.
#include "ekf_kernels.hip"
#include "ekf_units.h"

namespace ekf {

hipError_t launch_scan_nt128(const ScanParams& p, bool half, bool f16x3, hipStream_t st)
{
    const dim3 grid(p.G * p.E), block(128 + 64);
    if (f16x3) {
        if (half) hipLaunchKernelGGL((scan_kernel<_Float16, false, 2, 128>), grid, block, 0, st, p);
        else hipLaunchKernelGGL((scan_kernel<float, false, 2, 128>), grid, block, 0, st, p);
    } else {
        if (half) hipLaunchKernelGGL((scan_kernel<_Float16, false, 1, 128>), grid, block, 0, st, p);
        else hipLaunchKernelGGL((scan_kernel<float, false, 1, 128>), grid, block, 0, st, p);
    }
    return hipGetLastError();
}

}  // namespace ekf
