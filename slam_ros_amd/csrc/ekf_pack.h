// ekf_pack.h — state transfer / initialisation: dense covariance <-> packed tiles, low-rank start.
#pragma once

#include "ekf_device.h"

// (contraction: free, as in the flush headers)
#pragma clang fp contract(fast)

namespace ekf {

template <typename T>
__device__ __forceinline__ void tile_rc_of(int rem, int& r, int& c)
{
    if (sizeof(typename Stor<T>::L) == 4) {
        const int q = rem & 3, lane = (rem >> 2) & 63, grp = rem >> 8;
        c = lane & 31;
        r = q + 4 * (lane >> 5) + 8 * grp;
    } else {
        const int reg = (rem & 1) + 2 * ((rem >> 7) & 1), lane = (rem >> 1) & 63, blk = rem >> 8;
        c = (lane & 15) + 16 * (blk & 1);
        r = (lane >> 4) + 4 * reg + 16 * (blk >> 1);
    }
}

// pack / unpack / lowrank cover the tiles [t0, t1) (a partitioned instance stores a slice; Pll points
// at the slice's first tile, t0)
template <typename T>
__global__ void pack_kernel(Dims d, const double* __restrict__ Pfull, T* __restrict__ Pll,
                            double* __restrict__ Rs, const int2* __restrict__ tile_rc, int ex,
                            int64_t t0, int64_t t1)
{
    const int64_t total = (t1 - t0) * TILE_ELEMS;
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < total;
         g += (int64_t)gridDim.x * blockDim.x) {
        const int64_t t = t0 + g / TILE_ELEMS;
        int r, c;
        tile_rc_of<T>((int)(g % TILE_ELEMS), r, c);
        const int2 rc = tile_rc[t];
        const int i = rc.x * TILE + r, j = rc.y * TILE + c;
        double v = 0.0;
        if (i < d.M && j < d.M) v = Pfull[(size_t)(3 + i) * d.n + (3 + j)];
        Pll[g] = to_store<T>(to_domain<T>(v, ex));
    }
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < 3 * (int64_t)d.n;
         g += (int64_t)gridDim.x * blockDim.x) {
        const int a = (int)(g / d.n), b = (int)(g % d.n);
        Rs[g] = Pfull[(size_t)a * d.n + b];
    }
}

template <typename T>
__global__ void unpack_kernel(Dims d, double* __restrict__ Pfull, const T* __restrict__ Pll,
                              const double* __restrict__ Rs, int ex, int64_t t0, int64_t t1)
{
    const int64_t total = (int64_t)d.n * d.n;
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < total;
         g += (int64_t)gridDim.x * blockDim.x) {
        const int a = (int)(g / d.n), b = (int)(g % d.n);
        double v;
        if (a < 3) v = Rs[(size_t)a * d.n + b];
        else if (b < 3) v = Rs[(size_t)b * d.n + a];
        else {
            // the tiles of another rank read as 0
            const int ba = (a - 3) >> 5, bb = (b - 3) >> 5;
            const int64_t t = tile_index(ba < bb ? ba : bb, ba < bb ? bb : ba, d.nb);
            v = (t >= t0 && t < t1)
                    ? from_domain<T>(from_store<T>(Pll[ll_offset<typename Stor<T>::L>(a - 3, b - 3, d.nb) - t0 * TILE_ELEMS]), ex)
                    : 0.0;
        }
        Pfull[g] = v;
    }
}

template <typename T>
__global__ void lowrank_kernel(Dims d, const double* __restrict__ diag,
                               const double* __restrict__ U, int rank, T* __restrict__ Pll,
                               double* __restrict__ Rs, const int2* __restrict__ tile_rc, int ex,
                               int64_t t0, int64_t t1)
{
    const int64_t total = (t1 - t0) * TILE_ELEMS;
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < total;
         g += (int64_t)gridDim.x * blockDim.x) {
        const int64_t t = t0 + g / TILE_ELEMS;
        int r, c;
        tile_rc_of<T>((int)(g % TILE_ELEMS), r, c);
        const int2 rc = tile_rc[t];
        const int i = rc.x * TILE + r, j = rc.y * TILE + c;
        double v = 0.0;
        if (i < d.M && j < d.M) {
            const double* ui = U + (size_t)(3 + i) * rank;
            const double* uj = U + (size_t)(3 + j) * rank;
            for (int k = 0; k < rank; k++) v += ui[k] * uj[k];
            if (i == j) v += diag[3 + i];
        }
        Pll[g] = to_store<T>(to_domain<T>(v, ex));
    }
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < 3 * (int64_t)d.n;
         g += (int64_t)gridDim.x * blockDim.x) {
        const int a = (int)(g / d.n), b = (int)(g % d.n);
        const double* ua = U + (size_t)a * rank;
        const double* ub = U + (size_t)b * rank;
        double v = 0.0;
        for (int k = 0; k < rank; k++) v += ua[k] * ub[k];
        if (a == b) v += diag[a];
        Rs[g] = v;
    }
}

}  // namespace ekf
