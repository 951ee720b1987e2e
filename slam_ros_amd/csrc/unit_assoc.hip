// unit_assoc.hip — the joint-compatibility search without touching the state (ekf_associate_joint,
// ekf_associate_joint_device): the jointly compatible assignment of a scan's lines to their candidate
// landmarks with the most pairings and, among those, the smallest joint distance.
//
// Three plain launches per call, no cross-workgroup wait, no atomics (ekf_kernels.h: AssocParams).
//   tables  the usable candidates of a row in (line, list) order (AssocPlan); per candidate the pairing
//           exactly as the joint gate evaluates it (ekf_joint_parts.h: joint_line): v and the diagonal
//           block; per pair of candidates on different lines with different landmarks the block S_ab
//           (joint_pair). This is where the state is read: one pll_block chain per candidate and per
//           pair, spread over ASSOC_TG workgroups (each evaluates the candidates, which the pairs need,
//           and takes its share of the pairs).
//   search  ASSOC_W workgroups of one wave per row. Each copies the row's tables into LDS and then
//           touches no global memory until its record. Depth first over the active lines; at a node the
//           lanes score its children, one child per lane: the two rows the pairing adds to the Cholesky
//           factor of its parent (the bordered form of the joint gate's factorisation: row (r, ·) is S_rc
//           with its updates fma(−L_rk, L_ck, ·) in ascending k, then a division by L_cc; z = L⁻¹v is
//           carried as the extra row), so d2 and logdet continue the parent's chains and come out bit
//           for bit as the joint gate's. The children's rows stay in LDS per level, so a descent copies
//           nothing: the path's factor is a list of row offsets. The nodes at depth ASSOC_SPLIT are
//           numbered in depth-first order and dealt round-robin; the levels above them are walked by
//           every workgroup alike (no incumbent pruning there, so the numbering agrees).
//   reduce  the best record of a row by (m, d2, depth-first order) into its ekf_assoc_hit.
// A subtree is cut only when it cannot beat the workgroup's incumbent strictly in (m, d2): with r lines
// left, m + r < m_best, or m + r == m_best and not d2 < d2_best (d2 never decreases along a path). Every
// loop is bounded by the budget or the caps.
#include "ekf_joint_parts.h"

namespace ekf {

constexpr int AS_ROWS = 16 * EKF_ASSOC_MAX_LINES * (EKF_ASSOC_MAX_LINES + 1);   // doubles: the children's rows
constexpr int AS_PLAN_WORDS = (int)(sizeof(AssocPlan) / sizeof(int));
static_assert(ASSOC_TG * ASSOC_THREADS >= ASSOC_PAIRS, "one pair per thread of the tables launch");
static_assert(EKF_ASSOC_MAX_TOTAL == 64 && EKF_ASSOC_MAX_CAND == 8, "one wave holds the candidates; a child per lane");

// the rows of child c of a node at depth lvl (m <= lvl pairings: rows of 2m + 1 and 2m + 2 entries)
__device__ __forceinline__ int as_rowbase(int lvl, int c) { return 16 * lvl * (lvl + 1) + c * (4 * lvl + 4); }

// ---- the plan: wave 0 of the workgroup, in two parts with the caller's barrier between and behind ----
__device__ __forceinline__ void assoc_plan_a(const AssocParams& p, int row, int e, int L, AssocPlan* sp)
{
    const int lane = threadIdx.x;
    const Dims& d = p.v.d;
    const int saved = min(max(p.t.saved[e], 0), d.N);
    const int32_t* cand = p.cand + (size_t)row * d.max_lines * p.C;
    const int n = L * p.C;
    int base = 0, flags = 0;
    for (int ch = 0; ch < n; ch += 64) {   // (at most EKF_MAX_LINES·EKF_ASSOC_MAX_CAND / 64 = 8 rounds)
        const int idx = ch + lane;
        const bool in = idx < n;
        const int v = in ? cand[idx] : -1;
        const bool bad = in && (v < -1 || v >= d.N);   // never used as an index
        const bool use = in && v >= 0 && v < saved;
        const unsigned long long mu = __ballot(use), mb = __ballot(bad);
        if (mb) flags |= EKF_AS_INVALID;
        if (use) {
            const int pos = base + __popcll(mu & ((1ull << lane) - 1ull));
            if (pos < EKF_ASSOC_MAX_TOTAL) {
                sp->lm[pos] = v;
                sp->line[pos] = idx / p.C;
            }
        }
        base += __popcll(mu);
    }
    if (base > EKF_ASSOC_MAX_TOTAL) {
        flags |= EKF_AS_INVALID;
        base = 0;
    }
    if (lane == 0) {
        sp->total = base;
        sp->flags = flags;
        sp->pad = 0;
    }
}

__device__ __forceinline__ void assoc_plan_b(AssocPlan* sp)
{
    const int lane = threadIdx.x;
    const int total = sp->total;
    const bool isf = lane < total && (lane == 0 || sp->line[lane - 1] != sp->line[lane]);
    const unsigned long long mf = __ballot(isf);
    const int na = __popcll(mf);
    if (na > EKF_ASSOC_MAX_LINES) {
        if (lane == 0) {
            sp->flags |= EKF_AS_INVALID;
            sp->total = 0;
            sp->nactive = 0;
            sp->first[0] = 0;
        }
        return;
    }
    if (isf) {
        const int ord = __popcll(mf & ((1ull << lane) - 1ull));
        sp->first[ord] = lane;
        sp->aline[ord] = sp->line[lane];
    }
    if (lane == 0) {
        sp->first[na] = total;
        sp->nactive = na;
    }
}

// ---- tables ----
template <typename T>
__global__ __launch_bounds__(ASSOC_THREADS) void assoc_tables_kernel(AssocParams p)
{
    __shared__ int4 sh_ctl[PMAX];
    __shared__ AssocPlan sp;
    __shared__ double sh_ln[EKF_ASSOC_MAX_TOTAL][JL_WORDS];
    const int tid = threadIdx.x;
    const int g = blockIdx.x;
    const int row = blockIdx.y;
    const int e = p.e0 + row;
    const Dims d = p.v.d;
    const int L = trial_count(p.t, row, d.max_lines);

    view_ctl(p.v, p.pend, e, sh_ctl);
    for (int k = tid; k < AS_PLAN_WORDS; k += ASSOC_THREADS) reinterpret_cast<int*>(&sp)[k] = -1;
    __syncthreads();
    if (tid < 64) assoc_plan_a(p, row, e, L, &sp);
    __syncthreads();
    if (tid < 64) assoc_plan_b(&sp);
    __syncthreads();
    const int total = sp.total;
    if (g == 0) {
        const int* src = reinterpret_cast<const int*>(&sp);
        int* dst = reinterpret_cast<int*>(p.plan + row);
        for (int k = tid; k < AS_PLAN_WORDS; k += ASSOC_THREADS) dst[k] = src[k];
    }
    if (total == 0) return;   // (uniform)
    const Committed cm = view_committed(p.v, e);
    const bool once = p.v.bf != 0;
    const PllView<T> pv = view_pll<T>(p.v, p.pend, e, sh_ctl);

    // ---- per candidate: the gate's candidate, the diagonal block, v ----
    if (tid < total) {
        Cand c;
        joint_line<T>(pv, once, p.t, cm, d, e, row, sp.line[tid], sp.lm[tid], c, sh_ln[tid]);
        if (g == 0) {
            double* ct = p.ctab + ((size_t)row * EKF_ASSOC_MAX_TOTAL + tid) * ASSOC_CWORDS;
            ct[0] = c.v[0];
            ct[1] = c.v[1];
            ct[2] = c.S[0];
            ct[3] = c.S[2];   // (the lower half, as the joint gate)
            ct[4] = c.S[3];
        }
    }
    __syncthreads();

    // ---- per pair a > b on different lines with different landmarks: S_ab ----
    const int q = g * ASSOC_THREADS + tid;
    if (q >= total * (total - 1) / 2) return;
    int a = (int)((1.0f + sqrtf(1.0f + 8.0f * (float)q)) * 0.5f);
    while (a * (a - 1) / 2 > q) a--;
    while ((a + 1) * a / 2 <= q) a++;
    const int b = q - a * (a - 1) / 2;   // 0 <= b < a < total
    if (sp.line[a] == sp.line[b] || sp.lm[a] == sp.lm[b]) return;   // never on one path
    double Sab[4];
    joint_pair<T>(pv, once, sp.lm[a], sp.lm[b], sh_ln[a], sh_ln[b], Sab);
    double* pt = p.ptab + ((size_t)row * ASSOC_PAIRS + q) * 4;
    pt[0] = Sab[0];
    pt[1] = Sab[1];
    pt[2] = Sab[2];
    pt[3] = Sab[3];
}

// ---- search ----
__device__ __forceinline__ int uni(int x) { return __builtin_amdgcn_readfirstlane(x); }

__global__ __launch_bounds__(64) void assoc_search_kernel(AssocParams p)
{
    extern __shared__ double dyn[];
    double* const sh_pt = dyn;                      // [npair][4]
    double* const rows = dyn + ASSOC_PAIRS * 4;     // [AS_ROWS]
    __shared__ AssocPlan pl;
    __shared__ double sh_ct[EKF_ASSOC_MAX_TOTAL * ASSOC_CWORDS];
    __shared__ double sh_bound[EKF_ASSOC_MAX_LINES + 1];
    // the path: per factor row its offset in `rows` and z; per pairing its candidate; per level the
    // node's (m, d2, logsum), the child taken and the children still to take
    __shared__ int sh_rowoff[2 * EKF_ASSOC_MAX_LINES], sh_pk[EKF_ASSOC_MAX_LINES];
    __shared__ double sh_z[2 * EKF_ASSOC_MAX_LINES];
    __shared__ int sh_nm[EKF_ASSOC_MAX_LINES + 1], sh_pick[EKF_ASSOC_MAX_LINES], sh_mask[EKF_ASSOC_MAX_LINES];
    __shared__ double sh_nd2[EKF_ASSOC_MAX_LINES + 1], sh_nls[EKF_ASSOC_MAX_LINES + 1];
    // the children of each level's node: d2, logsum and the two z
    __shared__ double sh_cd2[EKF_ASSOC_MAX_LINES][EKF_ASSOC_MAX_CAND], sh_cls[EKF_ASSOC_MAX_LINES][EKF_ASSOC_MAX_CAND];
    __shared__ double sh_cz[EKF_ASSOC_MAX_LINES][EKF_ASSOC_MAX_CAND][2];
    __shared__ int sh_bpick[EKF_ASSOC_MAX_LINES];
    const int lane = threadIdx.x;
    const int w = blockIdx.x;
    const int row = blockIdx.y;
    const double inf = __builtin_inf();

    {
        const int* src = reinterpret_cast<const int*>(p.plan + row);
        int* dst = reinterpret_cast<int*>(&pl);
        for (int k = lane; k < AS_PLAN_WORDS; k += 64) dst[k] = src[k];
    }
    __syncthreads();
    const int total = uni(min(max(pl.total, 0), EKF_ASSOC_MAX_TOTAL));
    const int na = uni(min(max(pl.nactive, 0), EKF_ASSOC_MAX_LINES));
    {
        const double* gpt = p.ptab + (size_t)row * ASSOC_PAIRS * 4;
        for (int k = lane; k < total * (total - 1) / 2 * 4; k += 64) sh_pt[k] = gpt[k];
        const double* gct = p.ctab + (size_t)row * EKF_ASSOC_MAX_TOTAL * ASSOC_CWORDS;
        for (int k = lane; k < total * ASSOC_CWORDS; k += 64) sh_ct[k] = gct[k];
        // m <= nactive <= the row's lines, so bound[m] is inside the caller's list
        if (lane <= EKF_ASSOC_MAX_LINES) sh_bound[lane] = lane <= na ? p.bound[lane] : __builtin_nan("");
        if (lane < EKF_ASSOC_MAX_LINES) sh_bpick[lane] = -1;
        if (lane == 0) {
            sh_nm[0] = 0;
            sh_nd2[0] = 0.0;
            sh_nls[0] = 0.0;
        }
    }
    __syncthreads();

    const int split = min(ASSOC_SPLIT, na);
    const int budget = p.budget;
    const long long maxiter = ((long long)budget + 2) * (EKF_ASSOC_MAX_LINES + 1) * (EKF_ASSOC_MAX_CAND + 3);
    bool bvalid = false;
    int bm = -1, border = 0;
    double bd2 = 0.0, bls = 0.0;
    int nodes = 0, flags = 0, counter = 0, cur_order = 0;
    int lvl = 0;
    bool entering = true;
    for (long long it = 0;; it++) {
        if (it >= maxiter) {   // (unreachable: every visit is the root, a scored child or an "unassigned" step)
            flags |= EKF_AS_TRUNCATED;
            break;
        }
        if (entering) {
            entering = false;
            const int m = uni(sh_nm[lvl]);
            const double d2 = sh_nd2[lvl];
            bool skip = false;
            if (lvl == split) {
                const int order = counter++;
                if (order % ASSOC_W != w) skip = true;
                else cur_order = order;
            }
            if (!skip && lvl == na) {   // a leaf: feasible at every step
                if (uni(!bvalid || m > bm || (m == bm && d2 < bd2))) {
                    bvalid = true;
                    bm = m;
                    bd2 = d2;
                    bls = sh_nls[lvl];
                    border = cur_order;
                    if (lane < EKF_ASSOC_MAX_LINES) sh_bpick[lane] = lane < na ? sh_pick[lane] : -1;
                }
                skip = true;
            }
            if (!skip && lvl >= split && bvalid) {
                const int top = m + (na - lvl);
                if (uni(top < bm || (top == bm && !(d2 < bd2)))) skip = true;   // cannot beat the incumbent strictly
            }
            if (skip) {
                if (--lvl < 0) break;
                continue;
            }
            // ---- expand: one child per lane ----
            const int f0 = uni(pl.first[lvl]);
            const int nc = min(uni(pl.first[lvl + 1]) - f0, EKF_ASSOC_MAX_CAND);
            const int pc = f0 + lane;
            bool score = lane < nc;
            if (score) {
                const int lmk = pl.lm[pc];
                for (int a = 0; a < m; a++)
                    if (pl.lm[sh_pk[a]] == lmk) score = false;   // taken on the path
            }
            const int nsc = __popcll(__ballot(score));
            if (nodes + nsc > budget) {
                flags |= EKF_AS_TRUNCATED;
                break;
            }
            nodes += nsc;
            bool feas = false, sing = false;
            if (score) {
                const int r0 = 2 * m;
                double* const R0 = rows + as_rowbase(lvl, lane);
                double* const R1 = R0 + r0 + 1;
                const double* ct = sh_ct + pc * ASSOC_CWORDS;
                const double* pb = sh_pt + (size_t)(pc * (pc - 1) / 2) * 4;
                double d2c = d2, lsc = sh_nls[lvl];
                // row 2m
                for (int c = 0; c < r0; c++) {
                    double acc = pb[sh_pk[c >> 1] * 4 + (c & 1)];
                    const double* Lc = rows + sh_rowoff[c];
                    for (int k = 0; k < c; k++) acc = fma(-R0[k], Lc[k], acc);
                    R0[c] = acc / Lc[c];
                }
                double piv = ct[2];
                for (int k = 0; k < r0; k++) piv = fma(-R0[k], R0[k], piv);
                if (!(piv > 0.0) || piv == inf) {
                    sing = true;
                } else {
                    const double l0 = sqrt(piv);
                    R0[r0] = l0;
                    lsc += log(l0);
                    double acc = ct[0];
                    for (int k = 0; k < r0; k++) acc = fma(-sh_z[k], R0[k], acc);
                    const double z0 = acc / l0;
                    d2c = fma(z0, z0, d2c);
                    // row 2m + 1
                    for (int c = 0; c <= r0; c++) {
                        double a2 = c < r0 ? pb[sh_pk[c >> 1] * 4 + 2 + (c & 1)] : ct[3];
                        const double* Lc = c < r0 ? rows + sh_rowoff[c] : R0;
                        for (int k = 0; k < c; k++) a2 = fma(-R1[k], Lc[k], a2);
                        R1[c] = a2 / Lc[c];
                    }
                    piv = ct[4];
                    for (int k = 0; k <= r0; k++) piv = fma(-R1[k], R1[k], piv);
                    if (!(piv > 0.0) || piv == inf) {
                        sing = true;
                    } else {
                        const double l1 = sqrt(piv);
                        R1[r0 + 1] = l1;
                        lsc += log(l1);
                        acc = ct[1];
                        for (int k = 0; k < r0; k++) acc = fma(-sh_z[k], R1[k], acc);
                        acc = fma(-z0, R1[r0], acc);
                        const double z1 = acc / l1;
                        d2c = fma(z1, z1, d2c);
                        feas = d2c <= sh_bound[m + 1];   // (NaN fails)
                        sh_cd2[lvl][lane] = d2c;
                        sh_cls[lvl][lane] = lsc;
                        sh_cz[lvl][lane][0] = z0;
                        sh_cz[lvl][lane][1] = z1;
                    }
                }
            }
            const unsigned long long mfe = __ballot(feas);
            if (__ballot(sing)) flags |= EKF_AS_SINGULAR;
            if (lane == 0) sh_mask[lvl] = (int)(mfe & 0xffull) | (1 << EKF_ASSOC_MAX_CAND);   // "unassigned" last
            __syncthreads();
        }
        // ---- the next child of the node at lvl ----
        const int mask = uni(sh_mask[lvl]);
        if (mask == 0) {
            if (--lvl < 0) break;
            continue;
        }
        const int c = __ffs(mask) - 1;
        const int m = uni(sh_nm[lvl]);
        __syncthreads();
        if (lane == 0) {
            sh_mask[lvl] = mask & (mask - 1);
            if (c == EKF_ASSOC_MAX_CAND) {
                sh_pick[lvl] = -1;
                sh_nm[lvl + 1] = m;
                sh_nd2[lvl + 1] = sh_nd2[lvl];
                sh_nls[lvl + 1] = sh_nls[lvl];
            } else {
                const int pc = pl.first[lvl] + c;
                sh_pick[lvl] = pc;
                sh_pk[m] = pc;
                sh_nm[lvl + 1] = m + 1;
                sh_nd2[lvl + 1] = sh_cd2[lvl][c];
                sh_nls[lvl + 1] = sh_cls[lvl][c];
                sh_rowoff[2 * m] = as_rowbase(lvl, c);
                sh_rowoff[2 * m + 1] = as_rowbase(lvl, c) + 2 * m + 1;
                sh_z[2 * m] = sh_cz[lvl][c][0];
                sh_z[2 * m + 1] = sh_cz[lvl][c][1];
            }
        }
        lvl++;
        entering = true;
        __syncthreads();
    }
    __syncthreads();
    AssocRec* rec = p.rec + (size_t)row * ASSOC_W + w;
    if (lane == 0) {
        rec->valid = bvalid;
        rec->m = bvalid ? bm : 0;
        rec->flags = flags;
        rec->nodes = nodes;
        rec->order = border;
        rec->pad[0] = rec->pad[1] = rec->pad[2] = 0;
        rec->d2 = bvalid ? bd2 : 0.0;
        rec->logsum = bvalid ? bls : 0.0;
    }
    if (lane < EKF_ASSOC_MAX_LINES) rec->pick[lane] = bvalid ? sh_bpick[lane] : -1;
}

// ---- reduce ----
__global__ __launch_bounds__(64) void assoc_reduce_kernel(AssocParams p)
{
    __shared__ int sh_best;
    const int lane = threadIdx.x;
    const int row = blockIdx.x;
    const AssocPlan* pl = p.plan + row;
    const AssocRec* recs = p.rec + (size_t)row * ASSOC_W;
    ekf_assoc_hit* hit = p.hits + row;
    if (lane == 0) {
        int best = -1, nodes = 0, flags = pl->flags;
        for (int w = 0; w < ASSOC_W; w++) {
            const AssocRec& r = recs[w];
            nodes += r.nodes;
            flags |= r.flags;
            if (!r.valid) continue;
            const AssocRec& b = recs[best < 0 ? w : best];
            if (best < 0 || r.m > b.m || (r.m == b.m && (r.d2 < b.d2 || (r.d2 == b.d2 && r.order < b.order)))) best = w;
        }
        sh_best = best;
        hit->m = best < 0 ? 0 : recs[best].m;   // (no leaf reached: the empty hypothesis, always feasible)
        hit->status = flags;
        hit->nodes = nodes;
        hit->reserved = 0;
        hit->d2 = best < 0 ? 0.0 : recs[best].d2;
        hit->logdet = best < 0 ? 0.0 : 2.0 * recs[best].logsum;
    }
    hit->assign[lane] = -1;   // (EKF_MAX_LINES == 64)
    __syncthreads();
    const int best = sh_best;
    const int na = min(max(pl->nactive, 0), EKF_ASSOC_MAX_LINES);
    if (best >= 0 && lane < na) {
        const int pc = recs[best].pick[lane];
        if (pc >= 0 && pc < EKF_ASSOC_MAX_TOTAL) hit->assign[pl->aline[lane]] = pl->lm[pc];
    }
}
static_assert(EKF_MAX_LINES == 64, "assoc_reduce_kernel writes one assign entry per lane");

size_t assoc_lds_bytes() { return (size_t)(ASSOC_PAIRS * 4 + AS_ROWS) * sizeof(double); }

template <typename T>
static hipError_t launch_assoc_t(const AssocParams& p, hipStream_t st)
{
    hipLaunchKernelGGL(assoc_tables_kernel<T>, dim3(ASSOC_TG, (unsigned)p.E), dim3(ASSOC_THREADS), 0, st, p);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
    const size_t lds = assoc_lds_bytes();
    err = hipFuncSetAttribute(reinterpret_cast<const void*>(&assoc_search_kernel),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(assoc_search_kernel, dim3(ASSOC_W, (unsigned)p.E), dim3(64), lds, st, p);
    err = hipGetLastError();
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(assoc_reduce_kernel, dim3((unsigned)p.E), dim3(64), 0, st, p);
    return hipGetLastError();
}

hipError_t launch_assoc(const AssocParams& p, int precision, hipStream_t st)
{
    if (p.E < 1 || p.v.npend < 0 || p.v.npend > PMAX || p.t.L < 0 || p.t.L > p.v.d.max_lines ||
        p.v.d.max_lines > EKF_MAX_LINES || p.C < 1 || p.C > EKF_ASSOC_MAX_CAND || p.budget < 0 || !p.cand ||
        !p.bound || !p.hits || !p.t.lines || !p.plan || !p.ctab || !p.ptab || !p.rec)
        return hipErrorInvalidValue;
    if (precision == EKF_PREC_F64) return launch_assoc_t<double>(p, st);
    if (precision == EKF_PREC_F32) return launch_assoc_t<float>(p, st);
    if (precision == EKF_PREC_F16) return launch_assoc_t<_Float16>(p, st);
    return hipErrorInvalidValue;
}

}  // namespace ekf
