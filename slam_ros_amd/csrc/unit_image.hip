// unit_image.hip — the device forms of ekf_export_instances / ekf_import_instances: one launch moves
// every section of every image from the host-built table (ekf_image_plan.h).
//
// The kernel of unit_resample.hip with two more kinds of piece. Memory-bound: no LDS, no atomics, no
// wait between workgroups; a workgroup takes table entries grid-strided and fetches the next entry
// before it works on the current one (the table is in pinned host memory). A copy piece is
// copy_piece at its class's width. A re-tag piece (import) is the instance's completion words: every
// word is loaded, given the destination's epoch (image_retag) and stored, by the workgroup that owns
// the piece, so no other piece writes those words. A zero piece (export) is a section's padding.
// Plain vector stores: the next reader is another kernel, on any XCD, or a copy engine.
#include "ekf_kernels.h"
#include "ekf_copy_piece.h"
#include "ekf_image_plan.h"

namespace ekf {

// grid cap, workgroups per CU: the value measured for the same loop in unit_resample.hip
constexpr int IMG_BLOCKS_PER_CU = 32;
static_assert(RS_CHUNK == RS_THREADS * 16 * RS_INFLIGHT, "a 16-byte-class chunk is one round of loads");

typedef __attribute__((address_space(1))) unsigned gu32;

__global__ __launch_bounds__(RS_THREADS) void image_kernel(const CopySeg* __restrict__ table, int nseg, unsigned dst_epoch)
{
    const unsigned tid = threadIdx.x;
    int i = (int)blockIdx.x;
    if (i >= nseg) return;
    CopySeg sg = table[i];
    for (;;) {
        const int nx = i + (int)gridDim.x;
        CopySeg next = sg;
        if (nx < nseg) next = table[nx];
        const unsigned cls = sg.cls & 0xffu;
        if (cls == 16) copy_piece<u32x4>(sg.src, sg.dst, sg.bytes, tid);
        else if (cls == 8) copy_piece<u32x2>(sg.src, sg.dst, sg.bytes, tid);
        else if (cls == 4) copy_piece<unsigned>(sg.src, sg.dst, sg.bytes, tid);
        else if (cls == IMAGE_CLS_RETAG) {
            const gu32* s = reinterpret_cast<const gu32*>(sg.src);
            gu32* d = reinterpret_cast<gu32*>(sg.dst);
            const unsigned src_epoch = sg.cls >> 8;
            for (unsigned w = tid; w < sg.bytes / 4; w += RS_THREADS) d[w] = image_retag(s[w], src_epoch, dst_epoch);
        } else if (cls == IMAGE_CLS_ZERO) {
            gu32* d = reinterpret_cast<gu32*>(sg.dst);
            for (unsigned w = tid; w < sg.bytes / 4; w += RS_THREADS) d[w] = 0u;
        }
        if (nx >= nseg) break;
        i = nx;
        sg = next;
    }
}

hipError_t launch_image(const CopySeg* table, int nseg, unsigned dst_epoch, int ncu, hipStream_t st)
{
    if (nseg < 0 || ncu < 1 || (nseg > 0 && !table)) return hipErrorInvalidValue;
    if (nseg == 0) return hipSuccess;
    const long long cap = (long long)ncu * IMG_BLOCKS_PER_CU;
    const unsigned grid = (unsigned)(nseg < cap ? nseg : cap);
    hipLaunchKernelGGL(image_kernel, dim3(grid), dim3(RS_THREADS), 0, st, table, nseg, dst_epoch);
    return hipGetLastError();
}

}  // namespace ekf
