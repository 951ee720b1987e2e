// unit_query.hip — covariance blocks of chosen landmarks, read without a flush (ekf_query_joint,
// ekf_query_marginals, ekf_query_joint_device).
//
// The kernel takes the view the next association kernel would take (ReadView): the last
// materialised landmark block with the pending steps applied on read by pll_block — per step a reset,
// the ordered FMA chain of the downdate, the augmented rows, the fp16 rounding — so under
// EKF_ARITH_EXACT and on fp64 storage every value is bit for bit what the flush will store. On the
// split arithmetics the pending steps run as that exact chain too (the per-element replay), and fp16
// storage takes the group's one rounding at the end. The robot rows, columns and the mean come from
// the committed copy of the strip. It writes nothing but its outputs.
#include "ekf_device.h"

namespace ekf {

template <typename T>
__global__ __launch_bounds__(QUERY_THREADS) void query_kernel(QueryParams p)
{
    __shared__ int4 sh_ctl[PMAX];
    const int tid = threadIdx.x;
    const int row = blockIdx.y;        // the launch's row: index list and outputs
    const int e = p.e0 + row;          // the instance
    view_ctl(p.v, p.pend, e, sh_ctl);
    __syncthreads();
    const Dims d = p.v.d;
    const bool once = p.v.bf != 0;
    const PllView<T> pv = view_pll<T>(p.v, p.pend, e, sh_ctl);

    const int K = p.K;
    const int32_t* lm = p.landmarks ? p.landmarks + (size_t)row * K : nullptr;
    const Committed cm = view_committed(p.v, e);
    const double* Rs = cm.Rs;
    const double* y = cm.y;
    const double nan = __builtin_nan("");

    if (p.mode == QUERY_MARGINALS) {
        const int k = (int)blockIdx.x * QUERY_THREADS + tid;
        if (k >= K) return;
        const int j = lm ? lm[k] : k;
        const bool ok = j >= 0 && j < d.N;
        double o[4] = {nan, nan, nan, nan};
        if (ok) {
            pll_block<T>(pv, 2 * j, 2 * j, o);
            query_round<T>(once, pv.ex, o);
        }
        double* blk = p.blocks + ((size_t)row * K + k) * 4;
        double* cr = p.cross + ((size_t)row * K + k) * 6;
        double* mn = p.mean + ((size_t)row * K + k) * 2;
#pragma unroll
        for (int q = 0; q < 4; q++) blk[q] = o[q];
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int c = 0; c < 2; c++) cr[r * 2 + c] = ok ? Rs[(size_t)r * d.n + 3 + 2 * j + c] : nan;
        mn[0] = ok ? y[3 + 2 * j] : nan;
        mn[1] = ok ? y[4 + 2 * j] : nan;
        return;
    }

    // joint: nq × nq, the landmark part as K × K blocks of 2 × 2. A workgroup holds QUERY_ROWS row
    // landmarks (one per wave) by 64 column landmarks (the lanes): a wave's stores to one row of cov
    // are 64 adjacent 16-byte pieces, and its loads of the row landmark's operand rows are uniform.
    // Every block is computed from its own stored orientation (pll_block transposes on read), so both
    // halves of cov are written by coalesced stores and hold the elements unpack mirrors.
    const size_t nq = 3 + 2 * (size_t)K;
    double* cov = p.cov ? p.cov + (size_t)row * nq * nq : nullptr;
    double* mean = p.mean ? p.mean + (size_t)row * nq : nullptr;
    const int nB = (K + 63) / 64, nA = (K + QUERY_ROWS - 1) / QUERY_ROWS;
    const int nblk = cov ? nA * nB : 0;
    if ((int)blockIdx.x < nblk) {
        const int a = ((int)blockIdx.x / nB) * QUERY_ROWS + (tid >> 6);
        const int b = ((int)blockIdx.x % nB) * 64 + (tid & 63);
        if (a >= K || b >= K) return;
        const int ja = lm ? lm[a] : a, jb = lm ? lm[b] : b;
        double o[4] = {nan, nan, nan, nan};
        if (ja >= 0 && ja < d.N && jb >= 0 && jb < d.N) {
            pll_block<T>(pv, 2 * ja, 2 * jb, o);
            query_round<T>(once, pv.ex, o);
        }
        double* c0 = cov + (3 + 2 * (size_t)a) * nq + 3 + 2 * (size_t)b;
        c0[0] = o[0];
        c0[1] = o[1];
        c0[nq] = o[2];
        c0[nq + 1] = o[3];
        return;
    }
    // the robot rows and columns and the mean: one thread per landmark, one more for the pose block
    const int t = ((int)blockIdx.x - nblk) * QUERY_THREADS + tid;
    if (t < K) {
        const int j = lm ? lm[t] : t;
        const bool ok = j >= 0 && j < d.N;
#pragma unroll
        for (int c = 0; c < 2; c++) {
            const size_t q = 3 + 2 * (size_t)t + c;
            if (cov) {
#pragma unroll
                for (int r = 0; r < 3; r++) {
                    const double v = ok ? Rs[(size_t)r * d.n + 3 + 2 * j + c] : nan;
                    cov[r * nq + q] = v;
                    cov[q * nq + r] = v;   // (unpack mirrors the strip into the columns likewise)
                }
            }
            if (mean) mean[q] = ok ? y[3 + 2 * j + c] : nan;
        }
    } else if (t == K) {
#pragma unroll
        for (int r = 0; r < 3; r++) {
            if (cov) {
#pragma unroll
                for (int c = 0; c < 3; c++) cov[r * nq + c] = Rs[(size_t)r * d.n + c];
            }
            if (mean) mean[r] = y[r];
        }
    }
}

hipError_t launch_query(const QueryParams& p, int precision, hipStream_t st)
{
    if (p.K < 0 || p.K > p.v.d.N || p.E < 1 || p.v.npend < 0 || p.v.npend > PMAX) return hipErrorInvalidValue;
    unsigned gx;
    if (p.mode == QUERY_MARGINALS) {
        if (p.K == 0) return hipSuccess;
        gx = (unsigned)((p.K + QUERY_THREADS - 1) / QUERY_THREADS);
    } else {
        const long long nB = (p.K + 63) / 64, nA = (p.K + QUERY_ROWS - 1) / QUERY_ROWS;
        gx = (unsigned)((p.cov ? nA * nB : 0) + (p.K + 1 + QUERY_THREADS - 1) / QUERY_THREADS);
    }
    const dim3 grid(gx, (unsigned)p.E);
    if (precision == EKF_PREC_F64) hipLaunchKernelGGL(query_kernel<double>, grid, dim3(QUERY_THREADS), 0, st, p);
    else if (precision == EKF_PREC_F32) hipLaunchKernelGGL(query_kernel<float>, grid, dim3(QUERY_THREADS), 0, st, p);
    else if (precision == EKF_PREC_F16) hipLaunchKernelGGL(query_kernel<_Float16>, grid, dim3(QUERY_THREADS), 0, st, p);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace ekf
