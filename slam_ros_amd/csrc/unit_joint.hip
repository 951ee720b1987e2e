// unit_joint.hip — joint compatibility of line–landmark hypotheses without touching the state
// (ekf_gate_joint, ekf_gate_joint_device).
//
// A hypothesis assigns each line of a scan a landmark or none. Its m assigned lines, in list order,
// stack into one innovation v (2m) with covariance S = H_J·P_J·H_Jᵀ + blockdiag(R) (2m × 2m); the
// kernel reports vᵀS⁻¹v and log det S. One workgroup per (hypothesis, instance), one plain launch,
// no cross-workgroup wait, no atomics: a hit depends on its own hypothesis and the state only.
//   per line   (one thread per assigned line) the candidate exactly as the gate evaluates it
//              (ekf_gate.h: eval_candidate, line_R, gate_predict, predict_cols; the landmark block by
//              pll_block with the pending steps, then query_round): v, H, the diagonal 2×2 block of
//              S with R, d2_each; and, shared through LDS, the predicted strip columns, H and
//              G = H·P[:, 0:3] (innovation_cov's hp rows)
//   per pair   (threads over the pairs a > b) the 2×2 block S_ab = G_a·A_bᵀ + Q_ab·B_bᵀ with
//              Q_ab = A_a·C_b + B_a·D_ab, H = [A | B] on the columns {0, 1, 2 | l, l + 1}, C_b the strip
//              columns of l_b and D_ab = P[l_a, l_b] read in its stored orientation. Every sum is
//              written out in innovation_cov's order (for a = b it is that function's expression)
//   factor     S lower-only, packed by rows, in LDS (row r at r(r+1)/2), with v as row 2m behind it:
//              right-looking Cholesky by columns, the trailing update on all threads. Element (r, c)
//              takes its updates in ascending k whichever thread holds it, and row 2m comes out as
//              z = L⁻¹v, so the forward solve is part of the factorisation. d2 = Σ z_k² and
//              logdet = 2·Σ log L_kk, both summed by ascending k.
// Packed storage: 2m = 128 takes 129·130/2 doubles = 65.5 KiB, so two workgroups share a CU's 160 KiB.
#include "ekf_gate.h"

namespace ekf {

enum { JL_H10 = 0, JL_H11, JL_H1L, JL_G = 3 /* [2][3] */, JL_C = 9 /* [3][2] */, JL_WORDS = 15 };

__device__ __forceinline__ int tri(int r, int c) { return r * (r + 1) / 2 + c; }

template <typename T>
__global__ __launch_bounds__(JOINT_THREADS) void joint_kernel(JointParams p)
{
    extern __shared__ double A[];   // packed lower triangle of S, rows 0 .. 2m − 1, and v as row 2m
    __shared__ int4 sh_ctl[PMAX];
    __shared__ int sh_lm[EKF_MAX_LINES], sh_li[EKF_MAX_LINES];
    __shared__ double sh_ln[EKF_MAX_LINES][JL_WORDS];
    __shared__ int sh_m, sh_bad;
    const int tid = threadIdx.x;
    const int hyp = blockIdx.x;
    const int row = blockIdx.y;        // the launch's row: lines, hypotheses and outputs
    const int e = p.e0 + row;          // the instance
    const Dims d = p.v.d;
    const int L = trial_count(p.t, row, d.max_lines);
    const size_t ho = (size_t)row * p.H + hyp;
    const int32_t* asg = p.assign + ho * p.astride;
    double* each = p.d2_each ? p.d2_each + ho * p.astride : nullptr;
    ekf_joint_hit* hit = p.hits + ho;
    const double nan = __builtin_nan("");

    view_ctl(p.v, p.pend, e, sh_ctl);
    if (tid < 64) {
        // the assigned lines in list order; an entry outside [−1, N) is never used as an index
        const int a = tid < L ? asg[tid] : -1;
        const bool bad = tid < L && (a < -1 || a >= d.N);
        const bool act = tid < L && a >= 0 && !bad;
        const unsigned long long ma = __ballot(act), mb = __ballot(bad);
        if (act) {
            const int pos = __popcll(ma & ((1ull << tid) - 1ull));
            sh_lm[pos] = a;
            sh_li[pos] = tid;
        }
        if (each && tid < L && (!act || mb)) each[tid] = nan;
        if (tid == 0) {
            sh_m = __popcll(ma);
            sh_bad = mb != 0;
        }
    }
    __syncthreads();
    const int m = sh_m;
    if (sh_bad || m == 0) {   // (uniform)
        if (tid == 0) {
            hit->m = m;
            hit->status = sh_bad ? EKF_ST_SINGULAR_S : 0;
            hit->d2 = sh_bad ? nan : 0.0;
            hit->logdet = sh_bad ? nan : 0.0;
        }
        return;
    }
    const int n2 = 2 * m;
    const Committed cm = view_committed(p.v, e);
    const bool once = p.v.bf != 0;
    const PllView<T> pv = view_pll<T>(p.v, p.pend, e, sh_ctl);

    // ---- per line: the gate's candidate, the diagonal block, v ----
    if (tid < m) {
        const int a = tid, j = sh_lm[a], i = sh_li[a];
        TrialRobot rb;
        trial_robot(p.t, e, row, cm.Rs, d.n, rb);
        TrialBlock tb;
        trial_block<T>(pv, once, p.t.enc != nullptr, rb, cm, d.n, j, tb);
        double sn, cs;
        sincos(tb.yb.x, &sn, &cs);
        const ekf_line ln = p.t.lines[(size_t)row * d.max_lines + i];
        double Rm[4];
        line_R(ln, i, p.t.r_mode, Rm);
        Cand c;
        eval_candidate<true>(tb.b5, tb.yb.x, tb.yb.y, sn, cs, rb.xp, ln.alpha, ln.r, Rm, p.t.gate, gate_eta<T>(), c);
        if (each) each[i] = c.d2;
        double S[4], hp0[5], hp1[5];
        innovation_cov(tb.b5, c.h10, c.h11, c.h1l, Rm, S, hp0, hp1);   // (S == c.S; the hp rows are G)
        double* w = sh_ln[a];
        w[JL_H10] = c.h10; w[JL_H11] = c.h11; w[JL_H1L] = c.h1l;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            w[JL_G + k] = hp0[k];
            w[JL_G + 3 + k] = hp1[k];
        }
        w[JL_C + 0] = tb.rr0.x; w[JL_C + 1] = tb.rr0.y;
        w[JL_C + 2] = tb.rr1.x; w[JL_C + 3] = tb.rr1.y;
        w[JL_C + 4] = tb.rr2.x; w[JL_C + 5] = tb.rr2.y;
        // the lower half of the diagonal block (S[2], not S[1]) and the innovation
        A[tri(2 * a, 2 * a)] = c.S[0];
        A[tri(2 * a + 1, 2 * a)] = c.S[2];
        A[tri(2 * a + 1, 2 * a + 1)] = c.S[3];
        A[tri(n2, 2 * a)] = c.v[0];
        A[tri(n2, 2 * a + 1)] = c.v[1];
    }
    __syncthreads();

    // ---- per pair a > b: S_ab = G_a·A_bᵀ + Q_ab·B_bᵀ ----
    const int npair = m * (m - 1) / 2;
    for (int q = tid; q < npair; q += JOINT_THREADS) {
        int a = (int)((1.0f + sqrtf(1.0f + 8.0f * (float)q)) * 0.5f);
        while (a * (a - 1) / 2 > q) a--;
        while ((a + 1) * a / 2 <= q) a++;
        const int b = q - a * (a - 1) / 2;   // 0 <= b < a < m
        double Dab[4];
        pll_block<T>(pv, 2 * sh_lm[a], 2 * sh_lm[b], Dab);   // P[l_a, l_b] (transposed on read if stored so)
        query_round<T>(once, pv.ex, Dab);
        const double* wa = sh_ln[a];
        const double* wb = sh_ln[b];
        const double h10 = wa[JL_H10], h11 = wa[JL_H11], h1l = wa[JL_H1L];
        const double* C = wb + JL_C;   // P[k, l_b + c] at C[2k + c]
        // Q_ab = H_a·P[:, l_b : l_b + 2] past the robot rows (innovation_cov's hp[3], hp[4])
        const double q00 = -C[4] + Dab[0];
        const double q01 = -C[5] + Dab[1];
        const double q10 = h10 * C[0] + h11 * C[2] + h1l * Dab[0] + Dab[2];
        const double q11 = h10 * C[1] + h11 * C[3] + h1l * Dab[1] + Dab[3];
        const double* G = wa + JL_G;
        const double g10 = wb[JL_H10], g11 = wb[JL_H11], g1l = wb[JL_H1L];
        A[tri(2 * a, 2 * b)] = -G[2] + q00;
        A[tri(2 * a, 2 * b + 1)] = G[0] * g10 + G[1] * g11 + q00 * g1l + q01;
        A[tri(2 * a + 1, 2 * b)] = -G[5] + q10;
        A[tri(2 * a + 1, 2 * b + 1)] = G[3] * g10 + G[4] * g11 + q10 * g1l + q11;
    }

    // ---- Cholesky by columns with v as row n2: row n2 becomes z = L⁻¹v ----
    double logsum = 0.0;
    bool singular = false;
    const int tr = tid >> 4, tc = tid & 15;
    for (int k = 0; k < n2; k++) {
        __syncthreads();
        const double piv = A[tri(k, k)];
        if (!(piv > 0.0) || piv == __builtin_inf()) {   // (uniform: every thread reads the same pivot)
            singular = true;
            break;
        }
        const double lkk = sqrt(piv);
        logsum += log(lkk);
        for (int r = k + 1 + tid; r <= n2; r += JOINT_THREADS) A[tri(r, k)] = A[tri(r, k)] / lkk;
        __syncthreads();
        for (int r = k + 1 + tr; r <= n2; r += JOINT_THREADS / 16) {
            const double lrk = A[tri(r, k)];
            const int cmax = min(r, n2 - 1);
            for (int c = k + 1 + tc; c <= cmax; c += 16) {
                const int o = tri(r, c);
                A[o] = fma(-lrk, A[tri(c, k)], A[o]);
            }
        }
    }
    __syncthreads();
    if (tid != 0) return;
    double d2 = 0.0;
    if (!singular)
        for (int k = 0; k < n2; k++) {
            const double z = A[tri(n2, k)];
            d2 = fma(z, z, d2);
        }
    hit->m = m;
    hit->status = singular ? EKF_ST_SINGULAR_S : 0;
    hit->d2 = singular ? nan : d2;
    hit->logdet = singular ? nan : 2.0 * logsum;
}

size_t joint_lds_bytes(int max_lines)
{
    const size_t n2 = 2 * (size_t)max_lines;
    return (n2 + 1) * (n2 + 2) / 2 * sizeof(double);
}

template <typename T>
static hipError_t launch_joint_t(const JointParams& p, hipStream_t st)
{
    const size_t lds = joint_lds_bytes(p.v.d.max_lines);
    if (lds > 48 * 1024) {
        const hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void*>(&joint_kernel<T>),
                                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (err != hipSuccess) return err;
    }
    hipLaunchKernelGGL(joint_kernel<T>, dim3((unsigned)p.H, (unsigned)p.E), dim3(JOINT_THREADS), lds, st, p);
    return hipGetLastError();
}

hipError_t launch_joint(const JointParams& p, int precision, hipStream_t st)
{
    if (p.E < 1 || p.H < 0 || p.v.npend < 0 || p.v.npend > PMAX || p.t.L < 0 || p.t.L > p.v.d.max_lines ||
        p.v.d.max_lines > EKF_MAX_LINES || p.astride < p.t.L || !p.hits || !p.assign || !p.t.lines)
        return hipErrorInvalidValue;
    if (p.H == 0) return hipSuccess;
    if (precision == EKF_PREC_F64) return launch_joint_t<double>(p, st);
    if (precision == EKF_PREC_F32) return launch_joint_t<float>(p, st);
    if (precision == EKF_PREC_F16) return launch_joint_t<_Float16>(p, st);
    return hipErrorInvalidValue;
}

}  // namespace ekf
