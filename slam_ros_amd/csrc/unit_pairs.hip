// unit_pairs.hip — every pair of saved landmarks scored against each other, state untouched
// (ekf_gate_landmarks, ekf_gate_landmarks_device): which landmarks of the map are one physical line.
//
// The pair's expression is ekf_pairs.h's pair_eval, on blocks read as unit_query.hip reads them (pll_blocks
// with the pending steps, then query_round) and the committed mean. Two plain launches, no cross-workgroup
// wait, no atomics: every reduction is over a total order, so the results do not depend on the schedule.
//   pairs_pass1_kernel  one workgroup per (instance, pair of 64-landmark blocks I <= J). A wave owns sixteen
//                       row landmarks of block I (wave-uniform operand rows), the lanes are the column
//                       landmarks of block J. I < J: each pair once, serving its row (reduced across the
//                       lanes) and its column (reduced across the waves through LDS). I == J: the block's
//                       64 × 64 pairs from the row side alone. Per (landmark, partner block) one partial
//                       record; the pair's value to both halves of the matrix.
//   pairs_pass2_kernel  one thread per landmark folds its partials in ascending block order into its
//                       ekf_pair_hit; the workgroup writes the matrix's +inf entries.
#include "ekf_pairs.h"

namespace ekf {

__device__ __forceinline__ int pair_first_lane(unsigned long long m) { return m ? __ffsll((long long)m) - 1 : 64; }

__device__ __forceinline__ void pair_empty(ekf_pair_hit& h)
{
    const double nan = __builtin_nan("");
    h.nearest = h.first = -1;
    h.npass = h.status = 0;
    h.d2_nearest = h.d2_first = nan;
    h.C[0] = h.C[1] = h.C[2] = 0.0;
    h.delta[0] = h.delta[1] = 0.0;
}

// `q`, a record over partners that all lie above `h`'s, folded into h
__device__ __forceinline__ void pair_fold(ekf_pair_hit& h, const ekf_pair_hit& q)
{
    h.npass += q.npass;
    h.status |= q.status & EKF_PH_SINGULAR;
    if (h.first < 0 && q.first >= 0) {
        h.first = q.first;
        h.d2_first = q.d2_first;
        h.status |= q.status & EKF_PH_FLIP_FIRST;
    }
    // (h.d2_nearest NaN: none so far; a strict < keeps the lower index on ties)
    if (q.nearest >= 0 && !(h.d2_nearest <= q.d2_nearest)) {
        h.nearest = q.nearest;
        h.d2_nearest = q.d2_nearest;
        h.status = (h.status & ~EKF_PH_FLIP_NEAREST) | (q.status & EKF_PH_FLIP_NEAREST);
        h.C[0] = q.C[0]; h.C[1] = q.C[1]; h.C[2] = q.C[2];
        h.delta[0] = q.delta[0]; h.delta[1] = q.delta[1];
    }
}

template <typename T>
__global__ __launch_bounds__(PAIR_THREADS) void pairs_pass1_kernel(PairParams p)
{
    __shared__ int4 sh_ctl[PMAX];
    __shared__ double sh_D[2][PAIR_BLOCK][4];            // diagonal blocks of block I's and block J's landmarks
    __shared__ double2 sh_y[2][PAIR_BLOCK];              // their means
    __shared__ ekf_pair_hit sh_col[PAIR_THREADS / 64][PAIR_BLOCK];   // the waves' column-side records
    __shared__ double sh_t[PAIR_BLOCK][PAIR_BLOCK + 1];  // the block's distances, for the mirrored half
    const int tid = threadIdx.x;
    const int row = blockIdx.y;        // the launch's row: outputs
    const int e = p.e0 + row;          // the instance
    const Dims d = p.v.d;
    const int nb = pair_blocks(d.N);
    int I = 0, J = (int)blockIdx.x;    // the block pair, rows of the upper triangle in order
    while (I < nb && J >= nb - I) {
        J -= nb - I;
        I++;
    }
    J += I;
    const int saved = min(max(p.saved[e], 0), d.N);
    if (I >= nb || saved < 2 || J * PAIR_BLOCK >= saved) return;   // (uniform; I <= J)
    view_ctl(p.v, p.pend, e, sh_ctl);
    __syncthreads();
    const bool once = p.v.bf != 0;
    const PllView<T> pv = view_pll<T>(p.v, p.pend, e, sh_ctl);
    const Committed cm = view_committed(p.v, e);
    const bool diag = I == J;
    const int cs = diag ? 0 : 1;       // the column landmarks' side of sh_D / sh_y

    if (tid < 2 * PAIR_BLOCK) {        // (wave 0: block I, wave 1: block J)
        const int side = tid >> 6;
        const int j = (side ? J : I) * PAIR_BLOCK + (tid & 63);
        if (j < saved && !(side && diag)) {
            double o[4];
            pll_block<T>(pv, 2 * j, 2 * j, o);
            query_round<T>(once, pv.ex, o);
#pragma unroll
            for (int k = 0; k < 4; k++) sh_D[side][tid & 63][k] = o[k];
            sh_y[side][tid & 63] = *reinterpret_cast<const double2*>(cm.y + 3 + 2 * j);
        }
    }
    __syncthreads();

    const int lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = J * PAIR_BLOCK + lane;       // the lane's column landmark
    const bool bok = b < saved;
    const double g2 = p.gate * p.gate;
    const double inf = __builtin_inf();
    const size_t N = (size_t)d.N;
    double* d2 = p.d2 ? p.d2 + (size_t)row * N * N : nullptr;
    ekf_pair_hit* part = p.part + (size_t)row * N * nb;
    ekf_pair_hit col;                          // the lane's landmark against this wave's rows
    pair_empty(col);
    constexpr int ROWS = PAIR_BLOCK / (PAIR_THREADS / 64);
    for (int k0 = 0; k0 < ROWS; k0 += PAIR_BATCH) {
        const int a0 = I * PAIR_BLOCK + wv * ROWS + k0;
        if (a0 >= saved) break;                // (wave-uniform: the rows ascend)
        int j0[PAIR_BATCH];
#pragma unroll
        for (int k = 0; k < PAIR_BATCH; k++) j0[k] = 2 * (a0 + k < saved ? a0 + k : a0);
        // P[b, a]: the lane's rows owned (loaded once per batch), the wave's row landmarks as columns
        double X[PAIR_BATCH][4];
        if (bok) pll_blocks<T, PAIR_BATCH>(pv, 2 * b, j0, X);
#pragma unroll
        for (int k = 0; k < PAIR_BATCH; k++) {
            const int a = a0 + k;
            if (a >= saved) break;             // (wave-uniform)
            const bool is = bok && a != b;
            PairVal o;
            o.d2 = __builtin_nan("");
            o.flip = o.singular = 0;
            o.C[0] = o.C[1] = o.C[2] = o.delta[0] = o.delta[1] = 0.0;
            if (is) {
                const bool blo = b < a;        // X = P[lo, hi]
                double Xp[4];
                if (blo) {
                    Xp[0] = X[k][0]; Xp[1] = X[k][1]; Xp[2] = X[k][2]; Xp[3] = X[k][3];
                } else if ((a >> 4) == (b >> 4)) {
                    // one diagonal tile stores both orientations: P[a, b] is its own stored element
                    pll_block<T>(pv, 2 * a, 2 * b, Xp);
                } else {
                    Xp[0] = X[k][0]; Xp[1] = X[k][2]; Xp[2] = X[k][1]; Xp[3] = X[k][3];
                }
                query_round<T>(once, pv.ex, Xp);
                const double* Da = sh_D[0][a & 63];
                const double* Db = sh_D[cs][lane];
                const double2 ya = sh_y[0][a & 63], yb = sh_y[cs][lane];
                pair_eval(blo ? Db : Da, blo ? Da : Db, Xp, blo ? yb : ya, blo ? ya : yb, o);
            }
            const bool pass = is && o.d2 <= g2;          // (a NaN fails)
            const bool fin = is && o.d2 < inf;
            if (d2 && is) d2[(size_t)a * N + b] = o.d2;
            if (!diag) sh_t[a & 63][lane] = o.d2;
            // row a against block J: its first passing lane, its pass count, its nearest (the lowest
            // lane at the smallest finite d2)
            const unsigned long long mp = __ballot(pass), mf = __ballot(is && o.flip), ms = __ballot(is && o.singular);
            double best = fin ? o.d2 : inf;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) best = fmin(best, __shfl_xor(best, off, 64));
            const unsigned long long mn = __ballot(fin && o.d2 == best);
            const int lf = pair_first_lane(mp), ln = pair_first_lane(mn);
            ekf_pair_hit* r = part + (size_t)a * nb + J;
            if (lane == 0) {
                r->nearest = ln < 64 ? J * PAIR_BLOCK + ln : -1;
                r->first = lf < 64 ? J * PAIR_BLOCK + lf : -1;
                r->npass = __popcll(mp);
                r->status = (ln < 64 && ((mf >> ln) & 1) ? EKF_PH_FLIP_NEAREST : 0) |
                            (lf < 64 && ((mf >> lf) & 1) ? EKF_PH_FLIP_FIRST : 0) | (ms ? EKF_PH_SINGULAR : 0);
                if (lf == 64) r->d2_first = __builtin_nan("");
                if (ln == 64) {
                    r->d2_nearest = __builtin_nan("");
                    r->C[0] = r->C[1] = r->C[2] = 0.0;
                    r->delta[0] = r->delta[1] = 0.0;
                }
            }
            if (lane == lf) r->d2_first = o.d2;
            if (lane == ln) {
                r->d2_nearest = o.d2;
                r->C[0] = o.C[0]; r->C[1] = o.C[1]; r->C[2] = o.C[2];
                r->delta[0] = o.delta[0]; r->delta[1] = o.delta[1];
            }
            // column b against this wave's rows, ascending
            if (is && !diag) {
                ekf_pair_hit q;
                q.nearest = fin ? a : -1;
                q.first = pass ? a : -1;
                q.npass = pass ? 1 : 0;
                q.status = (o.flip ? (fin ? EKF_PH_FLIP_NEAREST : 0) | (pass ? EKF_PH_FLIP_FIRST : 0) : 0) |
                           (o.singular ? EKF_PH_SINGULAR : 0);
                q.d2_nearest = q.d2_first = o.d2;
                q.C[0] = o.C[0]; q.C[1] = o.C[1]; q.C[2] = o.C[2];
                q.delta[0] = o.delta[0]; q.delta[1] = o.delta[1];
                pair_fold(col, q);
            }
        }
    }
    if (diag) return;                          // (uniform)
    sh_col[wv][lane] = col;
    __syncthreads();
    if (tid < PAIR_BLOCK && bok) {             // column b against block I: the waves' rows ascend with the wave
        ekf_pair_hit h = sh_col[0][lane];
#pragma unroll
        for (int w = 1; w < PAIR_THREADS / 64; w++) pair_fold(h, sh_col[w][lane]);
        part[(size_t)b * nb + I] = h;
    }
    if (d2) {
        // the mirrored half d2[b][a], rows of 64 adjacent entries
        for (int idx = tid; idx < PAIR_BLOCK * PAIR_BLOCK; idx += PAIR_THREADS) {
            const int bb = J * PAIR_BLOCK + (idx >> 6), aa = I * PAIR_BLOCK + (idx & 63);
            if (bb < saved && aa < saved) d2[(size_t)bb * N + aa] = sh_t[idx & 63][idx >> 6];
        }
    }
}

__global__ __launch_bounds__(PAIR_THREADS) void pairs_pass2_kernel(PairParams p)
{
    const int tid = threadIdx.x;
    const int row = blockIdx.y;
    const int e = p.e0 + row;
    const int N = p.v.d.N;
    const int nb = pair_blocks(N);
    const int saved = min(max(p.saved[e], 0), N);
    const int a0 = (int)blockIdx.x * PAIR_THREADS;
    if (p.d2) {
        // the entries pass 1 leaves: the diagonal, and the rows and columns at or past savedLineCount
        const double inf = __builtin_inf();
        for (int r = 0; r < PAIR_THREADS && a0 + r < N; r++) {
            const int a = a0 + r;
            double* out = p.d2 + ((size_t)row * N + a) * N;
            const bool whole = a >= saved || saved < 2;
            for (int c = (whole ? 0 : saved) + tid; c < N; c += PAIR_THREADS) out[c] = inf;
            if (!whole && tid == 0) out[a] = inf;
        }
    }
    const int a = a0 + tid;
    if (a >= N) return;
    ekf_pair_hit h;
    pair_empty(h);
    if (a < saved && saved >= 2) {
        const ekf_pair_hit* part = p.part + ((size_t)row * N + a) * nb;
        const int nbu = pair_blocks(saved);    // the blocks that hold a saved landmark
        for (int Jb = 0; Jb < nbu; Jb++) pair_fold(h, part[Jb]);
    }
    p.hits[(size_t)row * N + a] = h;
}

hipError_t launch_pairs(const PairParams& p, int precision, hipStream_t st)
{
    const Dims& d = p.v.d;
    if (p.E < 1 || p.v.npend < 0 || p.v.npend > PMAX || d.N < 1 || !p.hits || !p.part || !p.saved) return hipErrorInvalidValue;
    const int nb = pair_blocks(d.N);
    const dim3 g1((unsigned)(nb * (nb + 1) / 2), (unsigned)p.E);
    if (precision == EKF_PREC_F64) hipLaunchKernelGGL(pairs_pass1_kernel<double>, g1, dim3(PAIR_THREADS), 0, st, p);
    else if (precision == EKF_PREC_F32) hipLaunchKernelGGL(pairs_pass1_kernel<float>, g1, dim3(PAIR_THREADS), 0, st, p);
    else if (precision == EKF_PREC_F16) hipLaunchKernelGGL(pairs_pass1_kernel<_Float16>, g1, dim3(PAIR_THREADS), 0, st, p);
    else return hipErrorInvalidValue;
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
    const dim3 g2((unsigned)((d.N + PAIR_THREADS - 1) / PAIR_THREADS), (unsigned)p.E);
    hipLaunchKernelGGL(pairs_pass2_kernel, g2, dim3(PAIR_THREADS), 0, st, p);
    return hipGetLastError();
}

}  // namespace ekf
