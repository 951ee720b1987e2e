// unit_resample_device.hip — ekf_resample_device: ekf_resample's copy with the source list in device
// memory. The host cannot know which instances are overwritten, so its table lists the pieces of one
// instance's slices (resample_pieces, ekf_resample_plan.h) and two launches do the rest:
//
//   resample_check_kernel  one wave checks the whole list (ekf_loop_plan.h: every entry in [0, E), every
//                          source a fixed point) and writes the plan the copy reads to context scratch:
//                          [count, status, (dst, src) × count], the overwritten instances ascending. A
//                          refused list gives count 0: nothing is copied. The copy never reads the
//                          caller's list, only pairs that passed the check.
//   resample_device_kernel grid-strided over (k < count, piece): item i is piece i mod npieces of pair
//                          i / npieces, so the workgroups are dealt the overwritten instances only and
//                          neighbouring workgroups move neighbouring pieces, whatever E and the grid are.
//                          The body is resample_kernel's (copy_piece: 16-byte accesses, four loads in
//                          flight); the next item's piece and pair are fetched before the current copy.
//                          The grid is the host's worst case, E − 1 overwritten instances, under the same
//                          cap; a workgroup past count · npieces leaves at once. No LDS, no atomics, no
//                          wait between workgroups.
#include "ekf_kernels.h"
#include "ekf_copy_piece.h"
#include "ekf_loop_plan.h"
#include "ekf_resample_plan.h"

namespace ekf {

constexpr int RSD_BLOCKS_PER_CU = 32;   // (unit_resample.hip's cap)
enum { RSD_COUNT = 0, RSD_STATUS = 1, RSD_PAIRS = 2 };   // words of the plan

__global__ __launch_bounds__(64) void resample_check_kernel(const int32_t* __restrict__ src, int E,
                                                            int32_t* __restrict__ plan, int32_t* __restrict__ status)
{
    const int lane = (int)threadIdx.x;
    int code = 0;
    for (int e = lane; e < E; e += 64) {
        const int c = resample_entry_code(src, E, e);
        code = c > code ? c : code;
    }
    for (int m = 32; m > 0; m >>= 1) {
        const int o = __shfl_xor(code, m, 64);
        code = o > code ? o : code;
    }
    int count = 0;
    if (code == 0) {
        // the overwritten instances in ascending order: 64 entries a round, each lane's place from the
        // round's ballot
        for (int e0 = 0; e0 < E; e0 += 64) {
            const int e = e0 + lane;
            const int s = e < E ? src[e] : e;
            const unsigned long long moved = __ballot(s != e);
            if (s != e) {
                const int k = count + __popcll(moved & ((1ull << lane) - 1ull));
                plan[RSD_PAIRS + 2 * k] = e;
                plan[RSD_PAIRS + 2 * k + 1] = s;
            }
            count += __popcll(moved);
        }
    }
    if (lane == 0) {
        plan[RSD_COUNT] = count;
        plan[RSD_STATUS] = resample_code_status(code);
        if (status) *status = resample_code_status(code);
    }
}

struct DeviceItem {
    CopyPiece pc;
    int dst, src;
};

__device__ __forceinline__ DeviceItem resample_item(const CopyPiece* __restrict__ pieces, unsigned npieces,
                                                    const int32_t* __restrict__ plan, unsigned i)
{
    const unsigned k = i / npieces;
    DeviceItem it;
    it.pc = pieces[i - k * npieces];
    it.dst = plan[RSD_PAIRS + 2 * k];
    it.src = plan[RSD_PAIRS + 2 * k + 1];
    return it;
}

__global__ __launch_bounds__(RS_THREADS) void resample_device_kernel(const CopyPiece* __restrict__ pieces,
                                                                     unsigned npieces,
                                                                     const int32_t* __restrict__ plan)
{
    const unsigned tid = threadIdx.x;
    const unsigned total = (unsigned)plan[RSD_COUNT] * npieces;   // (the host bounds (E − 1) · npieces)
    unsigned i = blockIdx.x;
    if (i >= total) return;
    DeviceItem it = resample_item(pieces, npieces, plan, i);
    for (;;) {
        const unsigned nx = i + gridDim.x;
        DeviceItem next = it;
        if (nx < total) next = resample_item(pieces, npieces, plan, nx);
        const uint64_t at = it.pc.base + it.pc.off;
        const uint64_t s = at + (uint64_t)it.src * it.pc.slice, d = at + (uint64_t)it.dst * it.pc.slice;
        if (it.pc.cls == 16) copy_piece<u32x4>(s, d, it.pc.len, tid);
        else if (it.pc.cls == 8) copy_piece<u32x2>(s, d, it.pc.len, tid);
        else copy_piece<unsigned>(s, d, it.pc.len, tid);
        if (nx >= total) break;
        i = nx;
        it = next;
    }
}

size_t resample_device_plan_words(int E) { return (size_t)RSD_PAIRS + 2 * (size_t)(E > 0 ? E : 0); }

hipError_t launch_resample_device(const int32_t* src, int E, int32_t* plan, int32_t* status, const CopyPiece* pieces,
                                  int npieces, int ncu, hipStream_t st)
{
    if (!src || !plan || E < 1 || npieces < 0 || ncu < 1 || (npieces > 0 && !pieces)) return hipErrorInvalidValue;
    const long long worst = (long long)(E - 1) * npieces;
    if (worst > 0x7fffffffLL) return hipErrorInvalidValue;   // (the kernel counts items in 32 bits)
    hipLaunchKernelGGL(resample_check_kernel, dim3(1), dim3(64), 0, st, src, E, plan, status);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess || worst == 0) return err;
    const long long cap = (long long)ncu * RSD_BLOCKS_PER_CU;
    const unsigned grid = (unsigned)(worst < cap ? worst : cap);
    hipLaunchKernelGGL(resample_device_kernel, dim3(grid), dim3(RS_THREADS), 0, st, pieces, (unsigned)npieces, plan);
    return hipGetLastError();
}

}  // namespace ekf
