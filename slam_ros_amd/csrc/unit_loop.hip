// unit_loop.hip — the three small kernels of the hypothesis loop (slam_ekf.h): the candidate lists from
// the gate's distance matrix, the instances' weights from the search's hits, the resampling plan. None
// reads the filter state; each is a pure function of its arguments, with a result that does not depend on
// scheduling: no atomics, no wait between workgroups.
#include <limits.h>

#include "ekf_kernels.h"
#include "ekf_loop_plan.h"

namespace ekf {

constexpr int CAND_THREADS = 256;
constexpr int CAND_WAVES = CAND_THREADS / 64;

// (key, j) in the lists' order: by the key, the lower landmark first on ties
__device__ __forceinline__ bool cand_before(double ka, int ja, double kb, int jb)
{
    return ka < kb || (ka == kb && ja < jb);
}

// One workgroup per (line, instance) row of d2 [E][max_lines][N]. Round c finds the smallest (key, j)
// among the members strictly after round c − 1's: the row (8 N bytes, L2-resident) is read C times, and
// any number of landmarks may lie inside the gate. key = sqrt(fabs(d2)), the helper's own expression
// (the fp64 square root is correctly rounded); NaN fails key <= gate.
__global__ __launch_bounds__(CAND_THREADS) void gate_candidates_kernel(const double* __restrict__ d2,
                                                                       const int32_t* __restrict__ nlines, int max_lines,
                                                                       int N, int C, double gate,
                                                                       int32_t* __restrict__ cand,
                                                                       int32_t* __restrict__ count)
{
    __shared__ double s_key[2][CAND_WAVES];
    __shared__ int s_j[2][CAND_WAVES];
    __shared__ int s_n[CAND_WAVES];
    const int i = (int)blockIdx.x, e = (int)blockIdx.y, tid = (int)threadIdx.x;
    const size_t row = (size_t)e * (size_t)max_lines + (size_t)i;
    int32_t* out = cand + row * (size_t)C;
    if (i >= nlines[e]) {   // (uniform)
        if (tid < C) out[tid] = -1;
        if (count && tid == 0) count[row] = 0;
        return;
    }
    const double* r = d2 + row * (size_t)N;
    double pk = -1.0;   // the previous round's (key, j): before every member (keys are >= 0)
    int pj = -1;
    int members = 0;
    int c = 0;
    for (; c < C; c++) {
        double bk = __builtin_huge_val();
        int bj = INT_MAX;   // none
        for (int j = tid; j < N; j += CAND_THREADS) {
            const double k = sqrt(fabs(r[j]));
            if (k <= gate) {
                if (c == 0) members++;
                if (cand_before(pk, pj, k, j) && cand_before(k, j, bk, bj)) {
                    bk = k;
                    bj = j;
                }
            }
        }
        for (int m = 32; m > 0; m >>= 1) {
            const double ok = __shfl_xor(bk, m, 64);
            const int oj = __shfl_xor(bj, m, 64);
            if (cand_before(ok, oj, bk, bj)) {
                bk = ok;
                bj = oj;
            }
            if (c == 0) members += __shfl_xor(members, m, 64);
        }
        // (two buffers: round c + 1 writes the other one while a slow wave still reads this one)
        const int buf = c & 1;
        if ((tid & 63) == 0) {
            s_key[buf][tid >> 6] = bk;
            s_j[buf][tid >> 6] = bj;
            if (c == 0) s_n[tid >> 6] = members;
        }
        __syncthreads();
        bk = s_key[buf][0];
        bj = s_j[buf][0];
        for (int w = 1; w < CAND_WAVES; w++)
            if (cand_before(s_key[buf][w], s_j[buf][w], bk, bj)) {
                bk = s_key[buf][w];
                bj = s_j[buf][w];
            }
        if (c == 0 && count && tid == 0) {
            int n = 0;
            for (int w = 0; w < CAND_WAVES; w++) n += s_n[w];
            count[row] = n;
        }
        if (bj == INT_MAX) break;   // (uniform) the list ended
        if (tid == 0) out[c] = bj;
        pk = bk;
        pj = bj;
    }
    if (tid >= c && tid < C) out[tid] = -1;
}

hipError_t launch_gate_candidates(const double* d2, const int32_t* nlines, int E, int max_lines, int N, int C,
                                  double gate, int32_t* cand, int32_t* count, hipStream_t st)
{
    if (!d2 || !nlines || !cand || E < 1 || max_lines < 1 || N < 1 || C < 1 || C > CAND_THREADS)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(gate_candidates_kernel, dim3((unsigned)max_lines, (unsigned)E), dim3(CAND_THREADS), 0, st, d2,
                       nlines, max_lines, N, C, gate, cand, count);
    return hipGetLastError();
}

// ---- weights ----
constexpr double LOG_2PI = 1.8378770664093454835606594728112;

// lw of one instance, and whether it counts (a usable hit and a finite lw)
__device__ __forceinline__ bool log_weight(const ekf_assoc_hit* hits, const int32_t* nlines, double log_unassigned,
                                           const double* logprior, int e, double* lw)
{
    const ekf_assoc_hit& h = hits[e];
    const int m = h.m, left = nlines[e] - m;
    double v = -(h.d2 + h.logdet) * 0.5 - (double)m * LOG_2PI;
    if (left != 0) v += (double)left * log_unassigned;
    if (logprior) v += logprior[e];
    *lw = v;
    return !(h.status & EKF_AS_INVALID) && v - v == 0.0;   // (NaN and ±inf fail)
}

// One wave: the maximum over the instances that count, then exp(lw − max), the maximum itself exactly 1
__global__ __launch_bounds__(64) void assoc_weights_kernel(const ekf_assoc_hit* __restrict__ hits,
                                                           const int32_t* __restrict__ nlines, int E,
                                                           double log_unassigned, const double* __restrict__ logprior,
                                                           double* __restrict__ weights)
{
    const int lane = (int)threadIdx.x;
    double mx = -__builtin_huge_val();
    for (int e = lane; e < E; e += 64) {
        double lw;
        if (log_weight(hits, nlines, log_unassigned, logprior, e, &lw)) mx = lw > mx ? lw : mx;
    }
    for (int m = 32; m > 0; m >>= 1) {
        const double o = __shfl_xor(mx, m, 64);
        mx = o > mx ? o : mx;
    }
    for (int e = lane; e < E; e += 64) {
        double lw;
        const bool in = log_weight(hits, nlines, log_unassigned, logprior, e, &lw);
        weights[e] = !in ? 0.0 : lw == mx ? 1.0 : exp(lw - mx);
    }
}

hipError_t launch_assoc_weights(const ekf_assoc_hit* hits, const int32_t* nlines, int E, double log_unassigned,
                                const double* logprior, double* weights, hipStream_t st)
{
    if (!hits || !nlines || !weights || E < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(assoc_weights_kernel, dim3(1), dim3(64), 0, st, hits, nlines, E, log_unassigned, logprior,
                       weights);
    return hipGetLastError();
}

// ---- the plan: sequential arithmetic over E numbers, one lane (ekf_loop_plan.h) ----
__global__ __launch_bounds__(64) void resample_plan_kernel(const double* __restrict__ weights, int E, double u,
                                                           double ess_below, int32_t* __restrict__ src,
                                                           ekf_plan_info* __restrict__ info)
{
    if (threadIdx.x == 0) resample_plan_sequential(weights, E, u, ess_below, src, info);
}

hipError_t launch_resample_plan(const double* weights, int E, double u, double ess_below, int32_t* src,
                                ekf_plan_info* info, hipStream_t st)
{
    if (!weights || !src || E < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(resample_plan_kernel, dim3(1), dim3(64), 0, st, weights, E, u, ess_below, src, info);
    return hipGetLastError();
}

}  // namespace ekf
