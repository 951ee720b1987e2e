// unit_scan.hip — the association kernel at its default width (and its instrumented build).
#include "ekf_kernels.hip"
#include "ekf_units.h"

namespace ekf {

int scan_blocks_per_cu(int precision)
{
    int nb = 0;
    hipError_t err =
        (precision == EKF_PREC_F64) ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, scan_kernel<double, false, 0>, SCAN_BLOCK, 0)
        : (precision == EKF_PREC_F16) ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, scan_kernel<_Float16, false, 0>, SCAN_BLOCK, 0)
        : hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, scan_kernel<float, false, 0>, SCAN_BLOCK, 0);
    return err == hipSuccess ? nb : 0;
}

size_t scan_lds_bytes(int precision)
{
    hipFuncAttributes a;
    hipError_t err =
        (precision == EKF_PREC_F64) ? hipFuncGetAttributes(&a, reinterpret_cast<const void*>(scan_kernel<double, false, 0>))
        : (precision == EKF_PREC_F16) ? hipFuncGetAttributes(&a, reinterpret_cast<const void*>(scan_kernel<_Float16, false, 0>))
        : hipFuncGetAttributes(&a, reinterpret_cast<const void*>(scan_kernel<float, false, 0>));
    return err == hipSuccess ? a.sharedSizeBytes : 0;
}

hipError_t launch_scan(const ScanParams& p, int precision, hipStream_t st)
{
    if (p.nt != SCAN_THREADS) {   // (the context picks a narrow width for the HOT instantiations only)
        if (p.dbg || precision == EKF_PREC_F64 || p.r_mode == 1 || p.d.kmax != 16) return hipErrorInvalidValue;
        const bool half = precision == EKF_PREC_F16, f16x3 = p.bf == 2;
        if (p.nt == 128) return launch_scan_nt128(p, half, f16x3, st);
        if (p.nt == 64) return launch_scan_nt64(p, half, f16x3, st);
        return hipErrorInvalidValue;
    }
    const dim3 grid(p.G * p.E), block(SCAN_BLOCK);
    if (p.dbg) {   // phase timers (EKF_OPT_SCAN_STAMPS): the instrumented instantiation
        if (precision == EKF_PREC_F64) hipLaunchKernelGGL((scan_kernel<double, true, 0>), grid, block, 0, st, p);
        else if (precision == EKF_PREC_F16) hipLaunchKernelGGL((scan_kernel<_Float16, true, 0>), grid, block, 0, st, p);
        else hipLaunchKernelGGL((scan_kernel<float, true, 0>), grid, block, 0, st, p);
    } else if (precision != EKF_PREC_F64 && p.r_mode != 1 && p.d.kmax == 16 && p.bf == 2) {
        if (precision == EKF_PREC_F16) hipLaunchKernelGGL((scan_kernel<_Float16, false, 2>), grid, block, 0, st, p);
        else hipLaunchKernelGGL((scan_kernel<float, false, 2>), grid, block, 0, st, p);
    } else if (precision != EKF_PREC_F64 && p.r_mode != 1 && p.d.kmax == 16) {
        if (precision == EKF_PREC_F16) hipLaunchKernelGGL((scan_kernel<_Float16, false, 1>), grid, block, 0, st, p);
        else hipLaunchKernelGGL((scan_kernel<float, false, 1>), grid, block, 0, st, p);
    } else {
        if (precision == EKF_PREC_F64) hipLaunchKernelGGL((scan_kernel<double, false, 0>), grid, block, 0, st, p);
        else if (precision == EKF_PREC_F16) hipLaunchKernelGGL((scan_kernel<_Float16, false, 0>), grid, block, 0, st, p);
        else hipLaunchKernelGGL((scan_kernel<float, false, 0>), grid, block, 0, st, p);
    }
    return hipGetLastError();
}

}  // namespace ekf
