// unit_joint.hip — joint compatibility of line–landmark hypotheses without touching the state
// (ekf_gate_joint, ekf_gate_joint_device).
//
// A hypothesis assigns each line of a scan a landmark or none. Its m assigned lines, in list order,
// stack into one innovation v (2m) with covariance S = H_J·P_J·H_Jᵀ + blockdiag(R) (2m × 2m); the
// kernel reports vᵀS⁻¹v and log det S. One workgroup per (hypothesis, instance), one plain launch,
// no cross-workgroup wait, no atomics: a hit depends on its own hypothesis and the state only.
//   per line   (one thread per assigned line) the candidate exactly as the gate evaluates it: v, the
//              diagonal 2×2 block of S with R, d2_each; and, shared through LDS, the pairing's words
//              (ekf_joint_parts.h: joint_line, which the joint-compatibility search shares)
//   per pair   (threads over the pairs a > b) the 2×2 block S_ab (ekf_joint_parts.h: joint_pair)
//   factor     S lower-only, packed by rows, in LDS (row r at r(r+1)/2), with v as row 2m behind it:
//              right-looking Cholesky by columns, the trailing update on all threads. Element (r, c)
//              takes its updates in ascending k whichever thread holds it, and row 2m comes out as
//              z = L⁻¹v, so the forward solve is part of the factorisation. d2 = Σ z_k² and
//              logdet = 2·Σ log L_kk, both summed by ascending k.
// Packed storage: 2m = 128 takes 129·130/2 doubles = 65.5 KiB, so two workgroups share a CU's 160 KiB.
#include "ekf_joint_parts.h"

namespace ekf {

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
        Cand c;
        joint_line<T>(pv, once, p.t, cm, d, e, row, i, j, c, sh_ln[a]);
        if (each) each[i] = c.d2;
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
        double Sab[4];
        joint_pair<T>(pv, once, sh_lm[a], sh_lm[b], sh_ln[a], sh_ln[b], Sab);
        A[tri(2 * a, 2 * b)] = Sab[0];
        A[tri(2 * a, 2 * b + 1)] = Sab[1];
        A[tri(2 * a + 1, 2 * b)] = Sab[2];
        A[tri(2 * a + 1, 2 * b + 1)] = Sab[3];
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
