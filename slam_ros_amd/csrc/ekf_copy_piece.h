// ekf_copy_piece.h — the body of the table-driven copies (device): one piece of a CopySeg table
// (ekf_resample_plan.h), moved by the 256 lanes of a workgroup. Shared by unit_resample.hip and
// unit_image.hip so that both keep one copy.
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

namespace ekf {

constexpr int RS_THREADS = 256;
constexpr int RS_INFLIGHT = 4;
static_assert(RS_INFLIGHT == 4, "copy_piece names its four values");

// (the compiler's own vector types: the accesses carry an address space)
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

template <typename V>
__device__ __forceinline__ void copy_piece(uint64_t src, uint64_t dst, unsigned bytes, unsigned tid)
{
    // (addresses from integers: named global, or the accesses are flat and count on lgkmcnt with the
    // table's scalar loads)
    const __attribute__((address_space(1))) V* s = reinterpret_cast<const __attribute__((address_space(1))) V*>(src);
    __attribute__((address_space(1))) V* d = reinterpret_cast<__attribute__((address_space(1))) V*>(dst);
    const unsigned nv = bytes / (unsigned)sizeof(V);
    unsigned i = tid;
    // whole rounds: four loads in flight per lane, then their stores (named values: an indexed
    // array here is promoted to LDS)
    for (; i + 3 * RS_THREADS < nv; i += RS_INFLIGHT * RS_THREADS) {
        const V a = s[i], b = s[i + RS_THREADS], c = s[i + 2 * RS_THREADS], e = s[i + 3 * RS_THREADS];
        d[i] = a;
        d[i + RS_THREADS] = b;
        d[i + 2 * RS_THREADS] = c;
        d[i + 3 * RS_THREADS] = e;
    }
    for (; i < nv; i += RS_THREADS) d[i] = s[i];
}

}  // namespace ekf
