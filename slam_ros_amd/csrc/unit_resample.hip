// unit_resample.hip — ekf_resample's segmented copy: one launch moves every per-instance slice of the
// overwritten instances from the host-built table (ekf_resample_plan.h).
//
// Memory-bound and nothing else: no LDS, no atomics, no wait between workgroups. A workgroup takes
// table entries grid-strided; an entry is at most RS_CHUNK bytes, which 256 lanes move as four
// 16-byte loads each, all in flight before the first store. The next entry is fetched before the
// current one is copied (the table is in pinned host memory: its latency hides behind the copy).
// Entries whose addresses or length are only 8- or 4-byte aligned (strip rows of 3n doubles with n
// odd, the scalars) take the same body at that width. Plain stores: the next reader is another
// kernel, on any XCD.
#include "ekf_kernels.h"
#include "ekf_copy_piece.h"
#include "ekf_resample_plan.h"

namespace ekf {

// grid cap, workgroups per CU: 8 are resident (four waves each); the entries are dealt statically, so
// a grid of only the resident workgroups leaves the slowest of them a tail, and a grid four times
// that lets the dispatcher hand out the rest as workgroups retire (measured 8 / 16 / 32)
#ifndef EKF_RS_BLOCKS_PER_CU
#define EKF_RS_BLOCKS_PER_CU 32
#endif
constexpr int RS_BLOCKS_PER_CU = EKF_RS_BLOCKS_PER_CU;
static_assert(RS_CHUNK == RS_THREADS * 16 * RS_INFLIGHT, "a 16-byte-class chunk is one round of loads");

__global__ __launch_bounds__(RS_THREADS) void resample_kernel(const CopySeg* __restrict__ table, int nseg)
{
    const unsigned tid = threadIdx.x;
    int i = (int)blockIdx.x;
    if (i >= nseg) return;
    CopySeg sg = table[i];
    for (;;) {
        const int nx = i + (int)gridDim.x;
        CopySeg next = sg;
        if (nx < nseg) next = table[nx];
        if (sg.cls == 16) copy_piece<u32x4>(sg.src, sg.dst, sg.bytes, tid);
        else if (sg.cls == 8) copy_piece<u32x2>(sg.src, sg.dst, sg.bytes, tid);
        else copy_piece<unsigned>(sg.src, sg.dst, sg.bytes, tid);
        if (nx >= nseg) break;
        i = nx;
        sg = next;
    }
}

hipError_t launch_resample(const CopySeg* table, int nseg, int ncu, hipStream_t st)
{
    if (nseg < 0 || ncu < 1 || (nseg > 0 && !table)) return hipErrorInvalidValue;
    if (nseg == 0) return hipSuccess;
    const long long cap = (long long)ncu * RS_BLOCKS_PER_CU;
    const unsigned grid = (unsigned)(nseg < cap ? nseg : cap);
    hipLaunchKernelGGL(resample_kernel, dim3(grid), dim3(RS_THREADS), 0, st, table, nseg);
    return hipGetLastError();
}

}  // namespace ekf
