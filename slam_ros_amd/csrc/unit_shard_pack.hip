// unit_shard_pack.hip — the partitioned instance's kernels, pack / unpack and the low-rank start.
#include "ekf_shard_kernels.h"
#include "ekf_pack.h"

namespace ekf {

hipError_t launch_shard_run(const ShardParams& p, int precision, hipStream_t st)
{
    const unsigned G = (unsigned)shard_run_workgroups(p.d.N);
    // shard_spec_kernel's LDS holds SH_MAX_LINES lines (ekf_shard_create admits no more)
    if (p.L > SH_MAX_LINES || p.d.max_lines > SH_MAX_LINES) return hipErrorInvalidValue;
    if (precision == EKF_PREC_F64) hipLaunchKernelGGL(shard_spec_kernel<double>, dim3(G), dim3(SPR_THREADS), 0, st, p);
    else if (precision == EKF_PREC_F32) hipLaunchKernelGGL(shard_spec_kernel<float>, dim3(G), dim3(SPR_THREADS), 0, st, p);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t launch_shard(const ShardParams& p, int precision, hipStream_t st)
{
    // every landmark, one per thread, spread over ⌈N/64⌉ CUs
    // (the guesses and the guessed columns: one grid row per line)
    const bool per_line = p.phase == SH_SPEC_COLS || p.phase == SH_GUESS;
    const dim3 grid((unsigned)((p.d.N + SH_THREADS - 1) / SH_THREADS), per_line ? (unsigned)max(p.L, 1) : 1u);
    if (precision == EKF_PREC_F64) hipLaunchKernelGGL(shard_kernel<double>, grid, dim3(SH_THREADS), 0, st, p);
    else if (precision == EKF_PREC_F32) hipLaunchKernelGGL(shard_kernel<float>, grid, dim3(SH_THREADS), 0, st, p);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

static int grid_for(int64_t work, int block)
{
    int64_t g = (work + block - 1) / block;
    if (g > 8192) g = 8192;
    if (g < 1) g = 1;
    return (int)g;
}

hipError_t launch_pack(const Dims& d, int precision, const double* Pfull, void* Pll, double* Rs,
                       const int2* tile_rc, int ex, hipStream_t st, int64_t t0, int64_t t1)
{
    if (t1 < 0) t1 = d.ntiles;
    const int grid = grid_for((t1 - t0) * TILE_ELEMS, 256);
    if (precision == EKF_PREC_F64)
        hipLaunchKernelGGL(pack_kernel<double>, dim3(grid), dim3(256), 0, st, d, Pfull,
                           (double*)Pll, Rs, tile_rc, ex, t0, t1);
    else if (precision == EKF_PREC_F16)
        hipLaunchKernelGGL(pack_kernel<_Float16>, dim3(grid), dim3(256), 0, st, d, Pfull,
                           (_Float16*)Pll, Rs, tile_rc, ex, t0, t1);
    else
        hipLaunchKernelGGL(pack_kernel<float>, dim3(grid), dim3(256), 0, st, d, Pfull,
                           (float*)Pll, Rs, tile_rc, ex, t0, t1);
    return hipGetLastError();
}

hipError_t launch_unpack(const Dims& d, int precision, double* Pfull, const void* Pll,
                         const double* Rs, int ex, hipStream_t st, int64_t t0, int64_t t1)
{
    if (t1 < 0) t1 = d.ntiles;
    const int grid = grid_for((int64_t)d.n * d.n, 256);
    if (precision == EKF_PREC_F64)
        hipLaunchKernelGGL(unpack_kernel<double>, dim3(grid), dim3(256), 0, st, d, Pfull,
                           (const double*)Pll, Rs, ex, t0, t1);
    else if (precision == EKF_PREC_F16)
        hipLaunchKernelGGL(unpack_kernel<_Float16>, dim3(grid), dim3(256), 0, st, d, Pfull,
                           (const _Float16*)Pll, Rs, ex, t0, t1);
    else
        hipLaunchKernelGGL(unpack_kernel<float>, dim3(grid), dim3(256), 0, st, d, Pfull,
                           (const float*)Pll, Rs, ex, t0, t1);
    return hipGetLastError();
}

hipError_t launch_lowrank(const Dims& d, int precision, const double* diag, const double* U,
                          int rank, void* Pll, double* Rs, const int2* tile_rc, int ex, hipStream_t st,
                          int64_t t0, int64_t t1)
{
    if (t1 < 0) t1 = d.ntiles;
    const int grid = grid_for((t1 - t0) * TILE_ELEMS, 256);
    if (precision == EKF_PREC_F64)
        hipLaunchKernelGGL(lowrank_kernel<double>, dim3(grid), dim3(256), 0, st, d, diag, U,
                           rank, (double*)Pll, Rs, tile_rc, ex, t0, t1);
    else if (precision == EKF_PREC_F16)
        hipLaunchKernelGGL(lowrank_kernel<_Float16>, dim3(grid), dim3(256), 0, st, d, diag, U,
                           rank, (_Float16*)Pll, Rs, tile_rc, ex, t0, t1);
    else
        hipLaunchKernelGGL(lowrank_kernel<float>, dim3(grid), dim3(256), 0, st, d, diag, U,
                           rank, (float*)Pll, Rs, tile_rc, ex, t0, t1);
    return hipGetLastError();
}

}  // namespace ekf
