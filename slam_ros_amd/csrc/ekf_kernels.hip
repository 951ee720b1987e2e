// ekf_kernels.hip — the association kernel of the EKF-SLAM update: scan_kernel and the helpers only
// it uses (the step overview: ekf_device.h). Not compiled on its own: the three unit_scan*.hip include
// it and define the launchers that instantiate their share of it. What it shares with the kernels of
// an instance partitioned over ranks (ekf_shard_kernels.h) — the reject filters, the mailbox, the gain
// package and rows — is ekf_assoc_parts.h; the gate arithmetic of a candidate is ekf_gate.h.
#include "ekf_assoc_parts.h"

// The association arithmetic contracts a·b + c only within one source expression, so a
// function inlined into different kernels or phases rounds identically everywhere (the
// speculative and sequential association paths must agree bit for bit).
#pragma clang fp contract(on)

namespace ekf {

// Certified rejection in fp32 (the second filter of the per-line gate; certified_reject in fp64
// and the exact evaluation run only where it cannot decide). Same bound structure as
// certified_reject, with the fp32 roundings added to it: every input rounded to fp32 (relative
// u = 2^-24), the short fp32 sums of S (≤ 12u of the sum of the absolute values of their terms,
// bounded through Pm and Hs = Σ|H row 1|), and q, det (16u of their magnitudes); sin/cos of the
// landmark angle from the fast fp32 path with EPS = 1e-4 allowed. v0 is the exact fp64 value of
// the evaluation (innovation_angle, no trigonometry), rounded once.
__device__ __forceinline__ bool certified_reject_f32(const Block5& b, double ma, double mr, const double xp[3],
                                                     double za, double zr, const double Rm[4], double gate,
                                                     double eta)
{
    if (!(fabs(ma) <= 8.0) || Rm[1] != Rm[2]) return false;
    constexpr float U = 5.9604645e-08f, EPS = 1e-4f;
    float sn, cs;
    __sincosf((float)ma, &sn, &cs);
    const float x0 = (float)xp[0], x1 = (float)xp[1];
    const float p00 = (float)b.p00, p01 = (float)b.p01, p02 = (float)b.p02;
    const float p10 = (float)b.p10, p11 = (float)b.p11, p12 = (float)b.p12;
    const float p20 = (float)b.p20, p21 = (float)b.p21, p22 = (float)b.p22;
    const float p0a = (float)b.p0a, p1a = (float)b.p1a, p2a = (float)b.p2a;
    const float p0b = (float)b.p0b, p1b = (float)b.p1b, p2b = (float)b.p2b;
    const float daa = (float)b.daa, dab = (float)b.dab, dba = (float)b.dba, dbb = (float)b.dbb;
    const float R0 = (float)Rm[0], R1 = (float)Rm[1], R2 = (float)Rm[2], R3 = (float)Rm[3];
    const float h10 = -cs, h11 = -sn, h1l = x0 * sn - x1 * cs;
    // S = H·P5·Hᵀ + R (innovation_cov's expressions)
    const float a0 = -p20 + p0a, a1 = -p21 + p1a, a2 = -p22 + p2a, a3 = -p2a + daa, a4 = -p2b + dab;
    const float c0 = h10 * p00 + h11 * p10 + h1l * p0a + p0b;
    const float c1 = h10 * p01 + h11 * p11 + h1l * p1a + p1b;
    const float c2 = h10 * p02 + h11 * p12 + h1l * p2a + p2b;
    const float c3 = h10 * p0a + h11 * p1a + h1l * daa + dba;
    const float c4 = h10 * p0b + h11 * p1b + h1l * dab + dbb;
    const float S0 = -a2 + a3 + R0;
    const float S1 = a0 * h10 + a1 * h11 + a3 * h1l + a4 + R1;
    const float S2 = -c2 + c3 + R2;
    const float S3 = c0 * h10 + c1 * h11 + c3 * h1l + c4 + R3;
    const float v0 = (float)innovation_angle(za, ma, xp[2]);
    const float v1 = (float)zr - ((float)mr - (x0 * cs + x1 * sn));
    const float ax = fabsf(x0) + fabsf(x1);
    const float ex = EPS * ax;
    float Pm = fmaxf(fmaxf(fmaxf(fabsf(p00), fabsf(p01)), fmaxf(fabsf(p02), fabsf(p10))),
                     fmaxf(fmaxf(fabsf(p11), fabsf(p12)), fmaxf(fabsf(p20), fabsf(p21))));
    Pm = fmaxf(Pm, fmaxf(fmaxf(fmaxf(fabsf(p22), fabsf(p0a)), fmaxf(fabsf(p1a), fabsf(p2a))),
                         fmaxf(fmaxf(fabsf(p0b), fabsf(p1b)), fabsf(p2b))));
    Pm = fmaxf(Pm, fmaxf(fmaxf(fabsf(daa), fabsf(dab)), fmaxf(fabsf(dba), fabsf(dbb))));
    const float Hs = 1.f + fabsf(h10) + fabsf(h11) + fabsf(h1l);
    const float dh = (2.f * EPS + ex) * Pm;
    // + the storage precision of the gate (gate_eta; |h1l| <= ax, 8u for these sums)
    const float fe = (float)eta * (1.f + 8.f * U);
    const float m0 = fe * 2.f * (fabsf(p22) + fabsf(daa));
    const float m1 = fe * (2.f + ax * ax) * (fabsf(p00) + fabsf(p11) + fabsf(p22) + fabsf(daa) + fabsf(dbb));
    const float dS00 = 12.f * U * (4.f * Pm + fabsf(R0)) + m0;
    const float dS01 = EPS * (fabsf(a0) + fabsf(a1)) + ex * fabsf(a3) + 12.f * U * (2.f * Hs * Pm + fabsf(R1)) +
                       0.5f * (m0 + m1);
    const float dS10 = 2.f * dh + 12.f * U * (2.f * Hs * Pm + fabsf(R2)) + 0.5f * (m0 + m1);
    const float dS11 = dh * (3.f + fabsf(h1l) + ex) + EPS * (fabsf(c0) + fabsf(c1)) + ex * fabsf(c3) +
                       12.f * U * (Hs * Hs * Pm + fabsf(R3)) + m1;
    const float dv1 = ex + 8.f * U * ((float)fabs(zr) + (float)fabs(mr) + ax);
    const float q = v0 * v0 * S3 - v0 * v1 * (S1 + S2) + v1 * v1 * S0;
    const float det = S0 * S3 - S1 * S2;
    const float mag_det = fabsf(S0 * S3) + fabsf(S1 * S2);
    const float mag_q = v0 * v0 * fabsf(S3) + fabsf(v0 * v1) * (fabsf(S1) + fabsf(S2)) + v1 * v1 * fabsf(S0);
    const float av1 = fabsf(v1) + dv1;
    const float dq = v0 * v0 * dS11 + fabsf(v0) * av1 * (dS01 + dS10) + fabsf(v0) * dv1 * fabsf(S1 + S2) +
                     (2.f * fabsf(v1) * dv1 + dv1 * dv1) * fabsf(S0) + av1 * av1 * dS00 + 16.f * U * mag_q + 1e-30f;
    const float ddet = fabsf(S0) * dS11 + fabsf(S3) * dS00 + fabsf(S1) * dS10 + fabsf(S2) * dS01 + dS01 * dS10 +
                       dS00 * dS11 + 16.f * U * mag_det + 1e-30f;
    const float det_lo = det - ddet;
    if (!(det_lo > 1e-4f * mag_det)) return false;              // also false for NaN / Inf
    const float g2 = (float)(gate * gate) * (1.f + 1e-4f);
    return (q - dq) > g2 * (det + ddet);
}

// Diagnostic phase timers (thread 0 of each workgroup; only when p.dbg is set).
#define EKF_STAMP(k)                                                            \
    do {                                                                        \
        if (dbg) {                                                              \
            const unsigned long long _t = __builtin_amdgcn_s_memrealtime();     \
            sh_stamp[k] += _t - t_last;                                         \
            t_last = _t;                                                        \
        }                                                                       \
    } while (0)

constexpr int EKF_NSTAMP = 32;   // diagnostic phase-timer slots per instance (EKF_SCAN_STAMPS=1)
constexpr int HIST_LDS = 8;   // matches per scan whose owned U rows stay in LDS
constexpr int HIST_V = 4;     // ... and whose V rows do (sequential path; the rest in Vst)

__device__ __forceinline__ int wave_min(int v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off, 64));
    return v;
}

// The status bits a speculative line can raise (GSL_EDOM, the gate's precision margin, the
// as-written R), three per line (line i at bits 3i .. 3i + 2 of one word, SPEC_L = 8 lines), so that
// a restart after a failed verdict keeps those of the lines before the first violating one
__device__ __forceinline__ int st_line(int st, int i)
{
    return (((st & EKF_ST_SINGULAR) ? 1 : 0) | ((st & EKF_ST_PRECISION_BIT) ? 2 : 0) | ((st & EKF_ST_NSYM) ? 4 : 0))
           << (3 * i);
}
__device__ __forceinline__ int st_lines(int packed, int upto)   // the bits of lines < upto
{
    const int w = upto >= 8 ? packed : packed & ((1 << (3 * upto)) - 1);
    return ((w & 0x249249) ? (int)EKF_ST_SINGULAR : 0) | ((w & 0x492492) ? (int)EKF_ST_PRECISION_BIT : 0) |
           ((w & 0x924924) ? (int)EKF_ST_NSYM : 0);
}

// ---------------------------------------------------------------------------------------
// 1. association + gain chain + augmentation: ⌈N/256⌉ cooperating workgroups per instance
// ---------------------------------------------------------------------------------------
// Thread (g, tid) of instance e OWNS landmark j = 256·g + tid: its gating candidate, its two
// rows of W/K/U/y, its robot-strip columns and its 2×2 diagonal block, all kept in registers
// for the whole scan. The robot 3×3 block and x_pre are uniform and recomputed identically by
// every thread. The instance's workgroups exchange words through a mailbox (ekf_assoc_parts.h:
// mb_store .. mb_wait_tagged). Every spin is bounded; a timeout sets a status bit.

// End of a launch (rollback protocol). Every workgroup has written its owned columns of the
// robot strip and mean into the inactive copy; it publishes its completion word (done_word) after
// its loads and stores have returned. The lead (workgroup 0, thread 0) waits for the other G − 1
// words of this epoch, bounded, and returns commit_status over all G: the launch commits (the lead
// flips cur[e] and writes the shared state) only if no timeout is in it. The shared inputs every
// workgroup read at its start (pose, saved, x_pre) are rewritten only after every word arrived,
// i.e. after every workgroup has finished reading them.
__device__ __forceinline__ void publish_done(int* sync, int g, unsigned epoch, int st)
{
    __hip_atomic_store(reinterpret_cast<unsigned*>(&sync[SYNC_WG0 + g]), done_word(epoch, st),
                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Run by every thread of workgroup 0 (the words are polled in parallel, thread k word k); the
// folded status of all G words (= commit_status) is returned to every thread.
template <int BLK>   // the workgroup's threads
__device__ __forceinline__ int lead_collect(int* sync, int G, unsigned epoch, int own_status, int spin,
                                            int tid, int* sh_red, int& zg)
{
    // zg: 1 + the highest workgroup whose word carries DONE_NZ (0: none)
    int st = tid == 0 ? commit_fold(0, done_word(epoch, own_status), epoch) : 0;
    int z = (tid == 0 && (own_status & (int)DONE_NZ)) ? 1 : 0;
    const bool late0 = (own_status & EKF_ST_TIMEOUT_BIT) != 0;
    for (int k = 1 + tid; k < G; k += BLK) {
        const unsigned* w = reinterpret_cast<const unsigned*>(&sync[SYNC_WG0 + k]);
        unsigned v = __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        int polls = 0;
        bool late = late0;
        while ((v >> 8) != (epoch & 0xffffffu) && !late) {
            __builtin_amdgcn_s_sleep(1);
            if (++polls > (1 << spin)) late = true;
            v = __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        st = commit_fold(st, v, epoch);
        if ((v >> 8) == (epoch & 0xffffffu) && (v & DONE_NZ)) z = max(z, k + 1);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        st |= __shfl_xor(st, off, 64);
        z = max(z, __shfl_xor(z, off, 64));
    }
    __syncthreads();
    if ((tid & 63) == 0) sh_red[tid >> 6] = st | (z << 8);
    __syncthreads();
    st = 0;
    z = 0;
#pragma unroll
    for (int w = 0; w < BLK / 64; w++) {
        st |= sh_red[w] & 0xff;
        z = max(z, sh_red[w] >> 8);
    }
    zg = z;
    return st;
}

// Cheap guess of the exact gate (fp32 sine/cosine, no error bounds). It only steers the
// speculative association; every decision it feeds is re-checked exactly. The landmark's part
// (predicted measurement, H·P·Hᵀ) does not depend on the line and is computed once.
struct Guess {
    float h0, h1, S[4];
};

__device__ __forceinline__ void guess_prep(const Block5& b, double ma, double mr, const double xp[3],
                                           Guess& gs)
{
    float sf, cf;
    __sincosf((float)ma, &sf, &cf);
    const float x0 = (float)xp[0], x1 = (float)xp[1];
    const float h10 = -cf, h11 = -sf, h1l = x0 * sf - x1 * cf;
    const float p00 = (float)b.p00, p01 = (float)b.p01, p02 = (float)b.p02;
    const float p10 = (float)b.p10, p11 = (float)b.p11, p12 = (float)b.p12;
    const float p20 = (float)b.p20, p21 = (float)b.p21, p22 = (float)b.p22;
    const float p0a = (float)b.p0a, p1a = (float)b.p1a, p2a = (float)b.p2a;
    const float p0b = (float)b.p0b, p1b = (float)b.p1b, p2b = (float)b.p2b;
    const float daa = (float)b.daa, dab = (float)b.dab, dba = (float)b.dba, dbb = (float)b.dbb;
    const float a0 = -p20 + p0a, a1 = -p21 + p1a, a2 = -p22 + p2a, a3 = -p2a + daa, a4 = -p2b + dab;
    const float c0 = h10 * p00 + h11 * p10 + h1l * p0a + p0b;
    const float c1 = h10 * p01 + h11 * p11 + h1l * p1a + p1b;
    const float c2 = h10 * p02 + h11 * p12 + h1l * p2a + p2b;
    const float c3 = h10 * p0a + h11 * p1a + h1l * daa + dba;
    const float c4 = h10 * p0b + h11 * p1b + h1l * dab + dbb;
    gs.S[0] = -a2 + a3;
    gs.S[1] = a0 * h10 + a1 * h11 + a3 * h1l + a4;
    gs.S[2] = -c2 + c3;
    gs.S[3] = c0 * h10 + c1 * h11 + c3 * h1l + c4;
    gs.h0 = (float)normalize_radian(ma - xp[2]);
    gs.h1 = (float)mr - (x0 * cf + x1 * sf);
}

__device__ __forceinline__ bool guess_pass(const Guess& gs, double za, double zr, const double Rm[4],
                                           double gate)
{
    constexpr float TWO_PI = 6.283185307179586f;
    float v0 = (float)za - gs.h0;
    if (fabsf(v0 - TWO_PI) < fabsf(v0)) v0 -= TWO_PI;
    else if (fabsf(v0 + TWO_PI) < fabsf(v0)) v0 += TWO_PI;
    const float v1 = (float)zr - gs.h1;
    const float S0 = gs.S[0] + (float)Rm[0], S1 = gs.S[1] + (float)Rm[1];
    const float S2 = gs.S[2] + (float)Rm[2], S3 = gs.S[3] + (float)Rm[3];
    const float q = v0 * v0 * S3 - v0 * v1 * (S1 + S2) + v1 * v1 * S0;
    const float det = S0 * S3 - S1 * S2;
    return !(det > 0.f) || q <= (float)(gate * gate) * det;
}

constexpr int SPEC_L = HIST_LDS;                    // lines
// guessed candidates per line per workgroup: with SPEC_K = SPEC_L every line's guess can be
// resolved (line t needs its first t + 1 candidates at most: only t earlier lines can take one)
constexpr int SPEC_K = 8;
// list words per (workgroup, line): A = local indices 0..3 (8 bits each), the count (bits 32..35)
// and a more bit (36); B = local indices 4..7, written and read only when the count exceeds 4
constexpr int LW_CNT = 32, LW_MORE = 36;
constexpr int SPEC_PB = 2;                          // guessed columns per pass over the pending steps
#ifndef EKF_SPEC_PB64
#define EKF_SPEC_PB64 4
#endif
constexpr int SPEC_PB64 = EKF_SPEC_PB64;            // ... fp64 operands (pll_shared_step: owned rows once per pass)
#ifndef EKF_STAGED_DEPTH
#define EKF_STAGED_DEPTH 1
#endif
constexpr int SPEC_QMAX = 16;                       // pending steps staged in LDS (T = 16: up to 15)
constexpr int SPEC_WD = 14 + 4 * (SPEC_L - 1);      // winner record: rr, Dj, y, sin/cos, column blocks
// speculative package: the words of build_package, then the robot 3×3 block and x_pre after the
// line's update (robot_update), computed once by the replay wave for every landmark wave
constexpr int PK_R33 = MB_VH, PK_XP = MB_VH + 9, PK_F = MB_VH + 12;   // + the symmetric factor (sym_factor)
// 1.0 if the guessed winner passed its exact gate; 0.0: it failed, the line is unmatched unless
// another landmark passes (which the landmark waves flag), and the other words are not written
constexpr int PK_OK = MB_VH + 15;
constexpr int PKW = MB_VH + 16;                     // package words (speculative lines; V rows in sh_wh)

// Blocks (j, cols[t]) for t < SPEC_L and (j, j) (last; only if `diag`) of the landmark block
// with the pending steps applied, fp32 operands, every pending step with ks <= 8: the guessed
// columns' operand rows come from LDS (stg[t][q][U|V][row half][8], staged by the workgroup),
// the owned rows are loaded once per step (the next step's while this one runs). Per element
// the same chain as pll_blocks, kept in the requested orientation: a block stored transposed
// (its column's tile row first) evolves as fma(X_col·V_own) terms, which equal the owned-first
// products bit for bit (fma(a, b, c) == fma(b, a, c)), so every block runs one pattern on
// O = owned U (or owned V when transposed) and X = staged V (or staged U). Every k-step runs:
// past a step's matches the operands hold −0 (U) and +0 (V), whose products leave a chain as it
// is (x + (−0) == x).
// The stored blocks of staged_blocks, in the requested orientation (issued early: their loads
// share a memory round trip with the staging of the guessed columns' rows).
template <typename T>
__device__ __forceinline__ void staged_blocks_load(const PllView<T>& v, int j, const int (&cols)[8],
                                                   typename Stor<T>::C (&r)[9][4])
{
    using C = typename Stor<T>::C;
    const int i0 = 2 * j;
#pragma unroll
    for (int b = 0; b < 9; b++) {
        const int jb = 2 * (b < 8 ? cols[b] : j);
        const bool swap = (i0 >> 5) > (jb >> 5);
        C a[4];
        load_block<T>(v, swap ? jb : i0, swap ? i0 : jb, a);
        r[b][0] = a[0]; r[b][1] = swap ? a[2] : a[1];
        r[b][2] = swap ? a[1] : a[2]; r[b][3] = a[3];
    }
}

template <typename T>
__device__ __forceinline__ void staged_blocks(const PllView<T>& v, int j, const int (&cols)[8],
                                              const float* stg, typename Stor<T>::C (&r)[9][4],
                                              double (&out)[9][4])
{
    using C = typename Stor<T>::C;
    constexpr int NB = 9;
    const int i0 = 2 * j;
    bool swap[NB];
    int jb[NB];
#pragma unroll
    for (int b = 0; b < NB; b++) {
        jb[b] = 2 * (b < 8 ? cols[b] : j);
        swap[b] = (i0 >> 5) > (jb[b] >> 5);
    }
    const int kh = v.kmax / 2;
    // owned rows i0, i0+1 of U_q: [row half][2 × 4 k]. Symmetric operands (U = −2^x·V, x the
    // fp16 storage exponent, 0 otherwise: gain_rows) make every block's chain one pattern on the
    // owned U rows and the column's V rows, whatever the stored orientation: a block stored
    // transposed evolves as fma(V_own, U_col) terms, and V_own·U_col == U_own·V_col exactly
    // (power-of-two scaling; fma(a, b, c) == fma(b, a, c)).
    auto load_rows = [&](int q, f32x4v (&Ux)[4][2]) {
        const Slot& sq = v.pend[q];
        const float* ou = u_rows_f32(v, sq) + ((size_t)(i0 >> 5) * 64 + (i0 & 31)) * kh;
#pragma unroll
        for (int rh = 0; rh < 4; rh++) {
            const int roff = (rh & 1) * kh + (rh >> 1) * 32 * kh;
#pragma unroll
            for (int h = 0; h < 2; h++) Ux[rh][h] = *reinterpret_cast<const f32x4v*>(ou + roff + 4 * h) * v.us;
        }
    };
    const float vscale = -ldexpf(1.0f, -v.ex);   // V_own = U_own · (−2^−x), exact
    // one pending step on the nine blocks, with that step's owned rows
    auto apply_step = [&](int q, const f32x4v (&U)[4][2]) __attribute__((always_inline)) {
        const Slot& sq = v.pend[q];
        const int4 cw = v.ctl[q];
        if (cw.x) {
#pragma unroll
            for (int b = 0; b < NB; b++) r[b][0] = r[b][1] = r[b][2] = r[b][3] = (C)0;
        } else if (cw.y > 0 || cw.z > 0) {   // (ks = 0: no match, or a rolled-back step: nothing to apply)
            // staged V rows of column b, interleaved by row pair (stage_v_index; block b + 1's
            // read from LDS while block b computes); the diagonal block's are the owned V rows
            auto read_x = [&](int b, f32x4v (&X)[2][4]) __attribute__((always_inline)) {
                const float* xs = stg + (((b * SPEC_QMAX + q) * 2 + 1) * 4) * 8;
#pragma unroll
                for (int pr = 0; pr < 2; pr++)
#pragma unroll
                    for (int kc = 0; kc < 4; kc++) X[pr][kc] = *reinterpret_cast<const f32x4v*>(xs + pr * 16 + 4 * kc);
            };
            f32x4v Xa[2][4], Xb[2][4];
            read_x(0, Xa);
#pragma unroll
            for (int b = 0; b < NB; b++) {
                f32x4v (&Xc)[2][4] = (b & 1) ? Xb : Xa;
                f32x4v (&Xn)[2][4] = (b & 1) ? Xa : Xb;
                if (b + 1 < 8) read_x(b + 1, Xn);
                f32x2v r01 = {(float)r[b][0], (float)r[b][1]}, r23 = {(float)r[b][2], (float)r[b][3]};   // fp32 operands only
#pragma unroll
                for (int kp = 0; kp < 8; kp++) {
                    const int h = kp >> 2, s4 = kp & 3;
                    f32x2v x01, x23;   // (column row 0, row 1) at k-pair kp, even and odd k
                    if (b < 8) {
                        x01 = f32x2v{Xc[0][kp >> 1][2 * (kp & 1)], Xc[0][kp >> 1][2 * (kp & 1) + 1]};
                        x23 = f32x2v{Xc[1][kp >> 1][2 * (kp & 1)], Xc[1][kp >> 1][2 * (kp & 1) + 1]};
                    } else {
                        x01 = f32x2v{U[0][h][s4], U[1][h][s4]} * vscale;
                        x23 = f32x2v{U[2][h][s4], U[3][h][s4]} * vscale;
                    }
                    r01 = __builtin_elementwise_fma(f32x2v{U[0][h][s4], U[0][h][s4]}, x01, r01);
                    r01 = __builtin_elementwise_fma(f32x2v{U[2][h][s4], U[2][h][s4]}, x23, r01);
                    r23 = __builtin_elementwise_fma(f32x2v{U[1][h][s4], U[1][h][s4]}, x01, r23);
                    r23 = __builtin_elementwise_fma(f32x2v{U[3][h][s4], U[3][h][s4]}, x23, r23);
                }
                r[b][0] = vround<T>(v, r01[0]); r[b][1] = vround<T>(v, r01[1]);
                r[b][2] = vround<T>(v, r23[0]); r[b][3] = vround<T>(v, r23[1]);
                // one block at a time (bounds the staged rows in registers)
                __builtin_amdgcn_sched_barrier(0);
            }
            if (cw.z > 0) {
#pragma unroll
                for (int b = 0; b < NB; b++) {
                    C a[4] = {r[b][0], swap[b] ? r[b][2] : r[b][1], swap[b] ? r[b][1] : r[b][2], r[b][3]};
                    patch_block<T>(v, sq, cw, i0, jb[b], swap[b], a);
                    r[b][0] = a[0]; r[b][1] = swap[b] ? a[2] : a[1];
                    r[b][2] = swap[b] ? a[1] : a[2]; r[b][3] = a[3];
                }
            }
        }
    };
    // The next step's rows are loaded while this one runs. The loads are issued on every
    // iteration (the last one re-reads its own step): a conditional prefetch makes the compiler's
    // wait-count merge at the loop join wait for ALL outstanding loads (vmcnt(0)) before the
    // body, which serialised every step behind its successor's loads.
    const int np = v.npend;
#if EKF_STAGED_DEPTH >= 2
    // two steps ahead: three register sets, the loop unrolled by three (static names)
    f32x4v UA[4][2], UB[4][2], UC[4][2];
    if (np > 0) {
        load_rows(0, UA);
        load_rows(min(1, np - 1), UB);
        for (int q = 0; q < np; q += 3) {
            load_rows(min(q + 2, np - 1), UC);
            apply_step(q, UA);
            if (q + 1 >= np) break;
            load_rows(min(q + 3, np - 1), UA);
            apply_step(q + 1, UB);
            if (q + 2 >= np) break;
            load_rows(min(q + 4, np - 1), UB);
            apply_step(q + 2, UC);
        }
    }
#else
    // one step ahead: two register sets, the loop unrolled by two (static names, no copies)
    f32x4v UA[4][2], UB[4][2];
    if (np > 0) {
        load_rows(0, UA);
        for (int q = 0; q < np; q += 2) {
            load_rows(min(q + 1, np - 1), UB);
            apply_step(q, UA);
            if (q + 1 >= np) break;
            load_rows(min(q + 2, np - 1), UA);
            apply_step(q + 1, UB);
        }
    }
#endif
#pragma unroll
    for (int b = 0; b < NB; b++)
#pragma unroll
        for (int k = 0; k < 4; k++) out[b][k] = from_domain<T>(r[b][k], v.ex);
}

// Block (2·wa, 2·wb) of the landmark block with the pending steps applied, when both landmarks
// are guessed columns (guess indices ta, tb): both sides' operand rows come from the staged LDS
// image. Per element the same chain as pll_blocks.
template <typename T>
__device__ __forceinline__ void pair_block_load(const PllView<T>& v, int wa, int wb, typename Stor<T>::C (&acc)[4])
{
    const int i0 = 2 * wa, jb = 2 * wb;
    const bool swap = (i0 >> 5) > (jb >> 5);   // stored orientation: (jb, i0)
    load_block<T>(v, swap ? jb : i0, swap ? i0 : jb, acc);
}

template <typename T>
__device__ __forceinline__ void staged_pair_block(const PllView<T>& v, int wa, int ta, int wb, int tb,
                                                  const float* stg, typename Stor<T>::C (&acc)[4],
                                                  double (&out)[4])
{
    using C = typename Stor<T>::C;
    const int i0 = 2 * wa, jb = 2 * wb;
    const bool swap = (i0 >> 5) > (jb >> 5);   // stored orientation: (jb, i0)
    const int tA = swap ? tb : ta, tB = swap ? ta : tb;
    for (int q = 0; q < v.npend; q++) {
        const int4 cw = v.ctl[q];
        if (cw.x) {
            acc[0] = acc[1] = acc[2] = acc[3] = (C)0;
            continue;
        }
        if (cw.y > 0) {   // every k-step (see staged_blocks); ks = 0: nothing (rolled back or no match)
            const float* cu = stg + (((tA * SPEC_QMAX + q) * 2 + 0) * 4) * 8;
            const float* cv = stg + (((tB * SPEC_QMAX + q) * 2 + 1) * 4) * 8;
#pragma unroll
            for (int h = 0; h < 2; h++) {
                f32x4v A[4];
#pragma unroll
                for (int rh = 0; rh < 4; rh++) A[rh] = *reinterpret_cast<const f32x4v*>(cu + rh * 8 + 4 * h);
#pragma unroll
                for (int s = 0; s < 4; s++) {
                    // the V side is interleaved (stage_v_index): rows 0 and 1 of k = 4h + s
                    const f32x2v b01 = *reinterpret_cast<const f32x2v*>(cv + stage_v_index(0, 4 * h + s));
                    const f32x2v b23 = *reinterpret_cast<const f32x2v*>(cv + stage_v_index(2, 4 * h + s));
                    acc[0] = fmaf(A[2][s], b23[0], fmaf(A[0][s], b01[0], acc[0]));
                    acc[1] = fmaf(A[2][s], b23[1], fmaf(A[0][s], b01[1], acc[1]));
                    acc[2] = fmaf(A[3][s], b23[0], fmaf(A[1][s], b01[0], acc[2]));
                    acc[3] = fmaf(A[3][s], b23[1], fmaf(A[1][s], b01[1], acc[3]));
                }
            }
#pragma unroll
            for (int k = 0; k < 4; k++) acc[k] = vround<T>(v, acc[k]);
        }
        if (cw.z > 0) patch_block<T>(v, v.pend[q], cw, i0, jb, swap, acc);
    }
    if (swap) {
        out[0] = from_domain<T>(acc[0], v.ex); out[1] = from_domain<T>(acc[2], v.ex);
        out[2] = from_domain<T>(acc[1], v.ex); out[3] = from_domain<T>(acc[3], v.ex);
    } else {
        out[0] = from_domain<T>(acc[0], v.ex); out[1] = from_domain<T>(acc[1], v.ex);
        out[2] = from_domain<T>(acc[2], v.ex); out[3] = from_domain<T>(acc[3], v.ex);
    }
}

// fp64 MFMA-replay contexts (plain pending steps, kmax = 16): the guessed winners' operand rows of
// up to M64_QMAX pending steps staged in LDS as doubles, [winner t][step q][U, V][row][kk][s] (k =
// 16·kk + s for s < 4: pll_blocks' fp64 k order), 32 KB for eight winners and eight steps.
constexpr int M64_QMAX = 8;
__device__ __forceinline__ int m64_stage_index(int t, int q, int uv, int rr, int kk)
{
    return ((((t * M64_QMAX + q) * 2 + uv) * 2 + rr) * 4 + kk) * 4;
}

// Block (2·wa, 2·wb) with the pending steps applied when both landmarks are guessed winners (guess
// indices ta, tb), from the fp64 stage: per element pll_blocks' chain (per step the k-steps s <
// ks, k-chunks kk, one fma per element and k), operand for operand. acc: the stored block in its
// stored orientation (pair_block_load).
template <typename T>
__device__ __forceinline__ void m64_pair_block(const PllView<T>& v, int wa, int ta, int wb, int tb, const double* stg,
                                               typename Stor<T>::C (&acc)[4], double (&out)[4])
{
    const int i0 = 2 * wa, jb = 2 * wb;
    const bool swap = (i0 >> 5) > (jb >> 5);   // stored orientation: (jb, i0)
    const int tA = swap ? tb : ta, tB = swap ? ta : tb;
    for (int q = 0; q < v.npend; q++) {
        const int ks = v.ctl[q].y;   // (no reset, no augmented rows on this path)
        if (ks <= 0) continue;
        const double* cu = stg + m64_stage_index(tA, q, 0, 0, 0);
        const double* cv = stg + m64_stage_index(tB, q, 1, 0, 0);
        for (int s = 0; s < ks; s++)
#pragma unroll
            for (int kk = 0; kk < 4; kk++) {
                const double x0 = cu[kk * 4 + s], x1 = cu[16 + kk * 4 + s];
                const double y0 = cv[kk * 4 + s], y1 = cv[16 + kk * 4 + s];
                acc[0] = fma(x0, y0, (double)acc[0]);
                acc[1] = fma(x0, y1, (double)acc[1]);
                acc[2] = fma(x1, y0, (double)acc[2]);
                acc[3] = fma(x1, y1, (double)acc[3]);
            }
#pragma unroll
        for (int k = 0; k < 4; k++) acc[k] = vround<T>(v, acc[k]);
    }
    if (swap) {
        out[0] = from_domain<T>(acc[0], v.ex); out[1] = from_domain<T>(acc[2], v.ex);
        out[2] = from_domain<T>(acc[1], v.ex); out[3] = from_domain<T>(acc[3], v.ex);
    } else {
        out[0] = from_domain<T>(acc[0], v.ex); out[1] = from_domain<T>(acc[1], v.ex);
        out[2] = from_domain<T>(acc[2], v.ex); out[3] = from_domain<T>(acc[3], v.ex);
    }
}

// Split-bf16 contexts (ScanParams::mfrep): the pending steps' share of the blocks a scan reads,
// ΔX = Σ_q V_q(rows)·V_q(cols)ᵀ over the active pending steps (amask: ks > 0; rolled-back steps
// have ks = 0), by v_mfma_f32_16x16x32_bf16 on the operand planes the association kernels wrote
// (V = hi + mid + lo exactly, the six part products of the flush). One instruction takes two
// steps: k-groups 0/1 the even/odd k of step qa, 2/3 those of step qb (the same k permutation on
// both operands). NB M-blocks of 16 rows: A row row_a(mb, r), B (16 columns) row row_b(c); a
// negative or out-of-range row is a zero operand. Lane l holds ΔX[4·(l >> 4) + i][l & 15] of
// M-block mb in acc[mb][i]. Not the fp32 chain of the flush (the split-bf16 flush is not one
// either): held to the same parity bar.
// F16 (EKF_ARITH_F16X3): two fp16 planes (hi, lo of 2^σ·V), three products (lo, hi), (hi, lo),
// (hi, hi) on v_mfma_f32_16x16x32_f16; acc then holds 2^(2σ)·ΔX (the caller scales it back)
// BATCH pairs of pending steps per memory round trip: every operand load of the BATCH pairs is
// issued before the first of their MFMAs (the replay wave's 16 winner rows: a few loads per pair,
// latency-bound; the landmark waves' 128 rows keep BATCH = 1). The MFMAs run in the same order for
// every BATCH, so the accumulators are the same bits.
template <int NB, bool F16, int BATCH = 1, typename RA, typename RB>
__device__ __forceinline__ void plane_replay(const Slot* pend, int e, size_t inst_bf, int M, unsigned amask,
                                             int lane, RA row_a, RB row_b, f32x4v (&acc)[NB])
{
    constexpr int NPL = F16 ? 2 : 3;
    using PV = typename std::conditional<F16, f16x8r, bf16x8r>::type;
#pragma unroll
    for (int mb = 0; mb < NB; mb++) acc[mb] = f32x4v{0.f, 0.f, 0.f, 0.f};
    const int kg = lane >> 4, h = kg & 1, r16 = lane & 15;
    typedef unsigned u32x4r __attribute__((ext_vector_type(4)));
    const PV zero = __builtin_bit_cast(PV, u32x4r{0u, 0u, 0u, 0u});
    const int rb_ = row_b(r16);
    int ra_[NB];
#pragma unroll
    for (int mb = 0; mb < NB; mb++) ra_[mb] = row_a(mb, r16);
    unsigned m = amask;
    while (m) {
        int qa[BATCH];
        PV B[BATCH][NPL], A[BATCH][NB][NPL];
#pragma unroll
        for (int bb = 0; bb < BATCH; bb++) {
            qa[bb] = m ? __builtin_ctz(m) : -1;
            if (m) m &= m - 1;
            const int qb = m ? __builtin_ctz(m) : -1;
            if (qb >= 0) m &= m - 1;
            const int q0 = qa[bb] >= 0 ? qa[bb] : 0;
            const unsigned short* pa = reinterpret_cast<const unsigned short*>(pend[q0].Bop) + (size_t)e * inst_bf;
            const unsigned short* pb = qb >= 0 ? reinterpret_cast<const unsigned short*>(pend[qb].Bop) + (size_t)e * inst_bf : pa;
            const unsigned short* pq = (kg >= 2) ? pb : pa;
            const bool none = qa[bb] < 0 || (kg >= 2 && qb < 0);
#pragma unroll
            for (int pl = 0; pl < NPL; pl++)
                B[bb][pl] = (!none && rb_ >= 0 && rb_ < M) ? *reinterpret_cast<const PV*>(pq + op_index_pl(rb_, h, pl, NPL)) : zero;
#pragma unroll
            for (int mb = 0; mb < NB; mb++)
#pragma unroll
                for (int pl = 0; pl < NPL; pl++)
                    A[bb][mb][pl] = (!none && ra_[mb] >= 0 && ra_[mb] < M)
                                        ? *reinterpret_cast<const PV*>(pq + op_index_pl(ra_[mb], h, pl, NPL)) : zero;
        }
#pragma unroll
        for (int bb = 0; bb < BATCH; bb++) {
            if (qa[bb] < 0) break;   // (uniform)
            if constexpr (F16) {
#pragma unroll
                for (int pp = 0; pp < 3; pp++) {
                    const int a = pp == 0 ? 1 : 0, b = pp == 1 ? 1 : 0;   // (lo, hi), (hi, lo), (hi, hi)
#pragma unroll
                    for (int mb = 0; mb < NB; mb++)
                        acc[mb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(A[bb][mb][a], B[bb][b], acc[mb], 0, 0, 0);
                }
            } else {
#pragma unroll
                for (int pp = 0; pp < 6; pp++) {
                    const int a = (0x102010 >> (4 * (5 - pp))) & 0xf;   // (mid, mid), (hi, lo), (lo, hi),
                    const int b = (0x120100 >> (4 * (5 - pp))) & 0xf;   // (hi, mid), (mid, hi), (hi, hi)
#pragma unroll
                    for (int mb = 0; mb < NB; mb++)
                        acc[mb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A[bb][mb][a], B[bb][b], acc[mb], 0, 0, 0);
                }
            }
        }
    }
}

// Split-plane contexts, EKF_OPT_MFMA_REPLAY = 2: the same ΔX = Σ_q V_q(rows)·V_q(cols)ᵀ by
// v_mfma_f32_16x16x4_f32 on the fp32 operand rows V_q themselves (kmax = 16), exact fp32 products
// accumulated in fp32: within a flush group the association kernel reads the landmark block at
// the precision of the EXACT arithmetic, and the split products enter P only at the group's
// flush (≈3 µs per scan more than the plane replay at T = 20: 4× the MFMA cycles).
// Same bytes per row and step as the two fp16 planes (64). Lane l
// loads one 16-byte quarter of a row's operand row: memory lane (row & 31) + 32·b, slots 4a..4a+3
// with (a, b) = (kk >> 1, kk & 1), kk = l >> 4; chunk c takes slot 4a + c, i.e. k = 2·(4a + c) + b
// on both operands (a k permutation: every dot product keeps its terms). acc layout as
// plane_replay's.
template <int NB, typename RA, typename RB>
__device__ __forceinline__ void f32_replay(const Slot* pend, int e, size_t opstride, int M, unsigned amask,
                                           int lane, RA row_a, RB row_b, f32x4v (&acc)[NB])
{
#pragma unroll
    for (int mb = 0; mb < NB; mb++) acc[mb] = f32x4v{0.f, 0.f, 0.f, 0.f};
    const int kk = lane >> 4, r16 = lane & 15;
    const int qoff = 32 * (kk & 1) * 8 + 4 * (kk >> 1);   // floats, within a row's 32-row block
    auto off = [&](int row) __attribute__((always_inline)) {
        return ((size_t)(row >> 5) * 64 + (row & 31)) * 8 + qoff;
    };
    const f32x4v zero = {0.f, 0.f, 0.f, 0.f};
    const int rb_ = row_b(r16);
    const bool bok = rb_ >= 0 && rb_ < M;
    const size_t boff = bok ? off(rb_) : 0;
    size_t aoff[NB];
    bool aok[NB];
#pragma unroll
    for (int mb = 0; mb < NB; mb++) {
        const int ra = row_a(mb, r16);
        aok[mb] = ra >= 0 && ra < M;
        aoff[mb] = aok[mb] ? off(ra) : 0;
    }
    unsigned m = amask;
    while (m) {
        // two steps per round trip: both steps' rows issued before either step's MFMAs
        const int qa = __builtin_ctz(m);
        m &= m - 1;
        const int qb = m ? __builtin_ctz(m) : -1;
        if (qb >= 0) m &= m - 1;
        const float* va = reinterpret_cast<const float*>(pend[qa].Vop) + (size_t)e * opstride;
        const float* vb = reinterpret_cast<const float*>(pend[qb >= 0 ? qb : qa].Vop) + (size_t)e * opstride;
        f32x4v Ba = bok ? *reinterpret_cast<const f32x4v*>(va + boff) : zero;
        f32x4v Bb = (bok && qb >= 0) ? *reinterpret_cast<const f32x4v*>(vb + boff) : zero;
        f32x4v Aa[NB], Ab[NB];
#pragma unroll
        for (int mb = 0; mb < NB; mb++) {
            Aa[mb] = aok[mb] ? *reinterpret_cast<const f32x4v*>(va + aoff[mb]) : zero;
            Ab[mb] = (aok[mb] && qb >= 0) ? *reinterpret_cast<const f32x4v*>(vb + aoff[mb]) : zero;
        }
#pragma unroll
        for (int c = 0; c < 4; c++)
#pragma unroll
            for (int mb = 0; mb < NB; mb++)
                acc[mb] = __builtin_amdgcn_mfma_f32_16x16x4f32(Aa[mb][c], Ba[c], acc[mb], 0, 0, 0);
#pragma unroll
        for (int c = 0; c < 4; c++)
#pragma unroll
            for (int mb = 0; mb < NB; mb++)
                acc[mb] = __builtin_amdgcn_mfma_f32_16x16x4f32(Ab[mb][c], Bb[c], acc[mb], 0, 0, 0);
    }
}

// EKF_ARITH_F16X3: x = 2^σ·v as hi + lo fp16 (hi = fp16(x) round-to-nearest, lo = fp16(x − hi), the
// remainder exact in fp32): 22 significant bits; (a, b) packed into one dword per part, a low
__device__ __forceinline__ void split_pack_f16(float a, float b, int sig, unsigned (&o)[2])
{
    const float xa = ldexpf(a, sig), xb = ldexpf(b, sig);
    const _Float16 ha = (_Float16)xa, hb = (_Float16)xb;
    const _Float16 la = (_Float16)(xa - (float)ha), lb = (_Float16)(xb - (float)hb);
    o[0] = (unsigned)__builtin_bit_cast(unsigned short, ha) | ((unsigned)__builtin_bit_cast(unsigned short, hb) << 16);
    o[1] = (unsigned)__builtin_bit_cast(unsigned short, la) | ((unsigned)__builtin_bit_cast(unsigned short, lb) << 16);
}

// Speculative association (lines <= SPEC_L, G <= SPEC_GMAX): every line's winner is guessed
// from the pre-update state, the guesses' mutual data are exchanged once, every workgroup
// replays the winners' part of the sequential chain to get all gain packages, then every thread
// runs the sequential gating and gain rows against those packages locally and flags any line
// whose exact first passing candidate differs from the guess. Three exchanges per scan instead
// of one per line; on a flag the scan restarts on the sequential path (identical results).

// ST: phase timers (EKF_OPT_SCAN_STAMPS). HOT (1, 2): the launch guarantees symmetric fp32 operands
// with kmax = 16 (the bench and every EKF_R_INTENDED fp32/fp16 context with max_lines <= 8): the
// per-line loops then carry no code for the other operand forms; HOT = 2 also fixes the plane
// arithmetic to EKF_ARITH_F16X3, HOT = 1 to EKF_ARITH_BF16X6 or none. HOT = 0: decided at run time.
// NT: landmarks (threads) per workgroup, 192 by default; 128 and 64 (ScanParams::nt) spread a small
// map's instances over more CUs (the commit's stores and the replay per CU scale with it)
template <typename T, bool ST, int HOT, int NT = ekf::SCAN_THREADS>
__global__ __launch_bounds__(NT + 64) void scan_kernel(ScanParams p)
{
    // (these hide the namespace defaults for the whole kernel body)
    constexpr int SCAN_THREADS = NT;
    constexpr int SCAN_BLOCK = NT + 64;
    const Dims d = p.d;
    const int r_mode = HOT ? (int)EKF_R_INTENDED : p.r_mode;   // (HOT: the launch checked it)
    constexpr double ETA = gate_eta<T>();
    // 1-D grid, instance-minor: block b is workgroup b / E of instance b % E. Workgroups are
    // dealt round-robin over the 8 XCDs, so with 8 instances per launch each instance's
    // workgroups share one XCD (and its L2) in every launch; correctness never depends on it
    const int g = (int)blockIdx.x / p.E;
    const int e = p.e0 + (int)blockIdx.x % p.E;
    const int G = p.G;
    const int tid = threadIdx.x;
    // threads < SCAN_THREADS own landmark j; the last wave (no landmark) replays the guessed
    // winners' chain in the speculative association
    const int j = tid < SCAN_THREADS ? g * SCAN_THREADS + tid : -1 - tid;
    const bool own = tid < SCAN_THREADS && j < d.N;
    const int n = d.n, N = d.N, M = d.M;
    const int b0 = 3 + 2 * j;                   // its first row of P
    // robot strip and mean: read the committed copy, write the other (committed by the lead at
    // the end only if every workgroup completed: a timed-out launch leaves the state untouched)
    const int cb = p.live[e];
    const double* Rs = p.Rs + ((size_t)cb * p.Etot + e) * 3 * n;
    const double* y = p.y + ((size_t)cb * p.Etot + e) * n;
    double* Rsw = p.Rs + ((size_t)(1 - cb) * p.Etot + e) * 3 * n;
    double* yw = p.y + ((size_t)(1 - cb) * p.Etot + e) * n;
    // diagonal landmark blocks after the last committed step (split-bf16 contexts), same two copies
    const double4* Ddr = p.mfrep ? reinterpret_cast<const double4*>(p.Dd) + ((size_t)cb * p.Etot + e) * d.N : nullptr;
    double4* Ddw = p.mfrep ? reinterpret_cast<double4*>(p.Dd) + ((size_t)(1 - cb) * p.Etot + e) * d.N : nullptr;
    int* sync = p.sync + (size_t)e * p.sync_stride;
    double* mbox = p.mbox + (size_t)e * 2 * G * p.mbw;
    const bool lead = (g == 0 && tid == 0);
    if (p.test_drop == e + 1 && G > 1 && g == G - 1) return;   // test hook: a workgroup that never runs

    __shared__ double sh_pkg[MB_VH + 4 * EKF_MAX_LINES];
    __shared__ int sh_red[SCAN_BLOCK / 64];
    __shared__ int sh_best[MAX_GROUPS];
    __shared__ int sh_extra[EKF_MAX_LINES];
    __shared__ int4 sh_ctl[PMAX];
    __shared__ ekf_line sh_lines[EKF_MAX_LINES];
    // U_q rows of the owned landmark for the first HIST_LDS matches of the scan (the rest in Ust)
    __shared__ double4 sh_uhist[HIST_LDS][SCAN_THREADS];
    // V_q rows (sequential path, for the package); owned blocks of the guessed columns as fp32
    // (speculative path with fp32 operands: the values are fp32 numbers)
    __shared__ double4 sh_vhist[HIST_V][SCAN_THREADS];
    static_assert(sizeof(float4) * SPEC_L == sizeof(double4) * HIST_V, "block buffer aliases sh_vhist");
    float4 (*sh_blk)[SCAN_THREADS] = reinterpret_cast<float4 (*)[SCAN_THREADS]>(&sh_vhist[0][0]);
    // fp64 operands: the owned blocks of the guessed columns in fp64 (48 KB; a placeholder otherwise)
    constexpr bool kB64 = sizeof(typename Stor<T>::C) == 8;
    __shared__ double4 sh_blk64[kB64 ? SPEC_L : 1][kB64 ? SCAN_THREADS : 1];
    // speculative association
    __shared__ unsigned long long sh_wl[SPEC_L][SCAN_THREADS / 64];
    __shared__ unsigned long long sh_lists[SPEC_GMAX * SPEC_L];
    __shared__ unsigned long long sh_listsb[SPEC_GMAX * SPEC_L];   // the B words (count > 4)
    __shared__ int sh_glist[SPEC_L][SPEC_K + 1];
    __shared__ int sh_spec[SPEC_L];
    __shared__ int sh_psg[PMAX];      // pending steps' plane exponents (EKF_ARITH_F16X3)
    __shared__ int sh_flag;
    __shared__ int sh_ready;
    __shared__ int sh_rwst;   // status bits of the replay wave (the winners' GSL_EDOM)
    __shared__ int sh_vto;    // a verdict poll of this workgroup timed out
    __shared__ int sh_first[SPEC_L];   // per line the first guessed candidate (speculative path)
    if (tid < SPEC_L) sh_first[tid] = 0x7fffffff;
    // the replay wave's line counter and status words: set before the first barrier below, since
    // on the MFMA-replay path the landmark waves reach their polls with no barrier after the records
    if (tid == 0) {
        sh_ready = 0;
        sh_rwst = 0;
        sh_vto = 0;
    }
    __shared__ double sh_wd[SPEC_L * SPEC_WD];
    __shared__ double4 sh_wh[SPEC_L][SPEC_L][2];
    __shared__ double sh_pk[SPEC_L][PKW];
    __shared__ __attribute__((aligned(16))) float sh_stg[SPEC_L * SPEC_QMAX * 2 * 4 * 8];   // staged pending-step rows
    __shared__ unsigned long long sh_stamp[EKF_NSTAMP];
    // EKF_ARITH_BF16X6 (fp32 storage): the owned rows' V values of this scan's matches (k-major
    // per row), split into bf16 planes and stored once at the end
    // fp32 operand storage (fp32 and fp16 P): the split-bf16 planes, the MFMA replay
    constexpr bool kPlanes = sizeof(typename Stor<T>::C) == 4;
    __shared__ __attribute__((aligned(16))) float sh_vpl[kPlanes ? SCAN_THREADS * 32 : 4];
    // plane arithmetic (HOT fixes it at compile time): EKF_ARITH_F16X3 planes hold hi + lo fp16 of
    // 2^σ·V. σ follows the largest landmark variance vmax (pvmax[e]) but changes only at the first
    // scan of a flush group (every workgroup of the instance computes it from pvmax), so that a
    // group's steps share one σ and the flush takes its pipelined path; mid-group only a reset
    // (σ empty) or a new landmark 64× above the variance σ was set for (then at the step that adds
    // it: that group and every pending replay over it take the exact forms). The MFMA replay of
    // plain pending steps returns 2^(2σ)·ΔX.
    const bool pf16 = kPlanes && (HOT == 2 || (HOT == 0 && p.bf == 2));
    const int npl = pf16 ? 2 : 3;
    const int psig = !pf16 ? 0 : p.npend == 0 ? plane_sigma(p.pvmax[e]) : p.psig[e];
    const double rsc = pf16 ? ldexp(1.0, -2 * psig) : 1.0;
    // the on-read replay of plain pending steps (EKF_OPT_MFMA_REPLAY): 1 the split products on
    // the planes (plane_replay: 2^(2σ)·ΔX for EKF_ARITH_F16X3), 2 fp32 MFMA on the fp32 operand
    // rows (f32_replay: ΔX unscaled); 1 also takes f32_replay when a pending step's planes were
    // written at another exponent or could not carry the instance's range (PLANE_SIGMA_EXACT),
    // instead of the exact per-element forms (below; the flush still takes the exact forms)
    bool f32rep = kPlanes && p.mfrep == 2;
    double rrsc = f32rep ? 1.0 : rsc;
    // phase timers only in the ST instantiation (EKF_SCAN_STAMPS=1): the product kernel carries
    // no timer code at all (its uniform branches and registers cost ≈2 µs per scan)
    unsigned long long* const pdbg = ST ? p.dbg : nullptr;
    unsigned long long* dbg = (pdbg && lead) ? pdbg + (size_t)e * EKF_NSTAMP : nullptr;
    if (pdbg && tid < EKF_NSTAMP) sh_stamp[tid] = 0;
    unsigned long long t_last = dbg ? __builtin_amdgcn_s_memrealtime() : 0ull;
    const unsigned long long t_first = t_last;

    // owned state, in registers for the whole scan
    double2 rr0, rr1, rr2, yb;
    double R33[9], xp[3];
    double F3[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    // (re)load the owned state and apply the predict (Robot.cpp:130-286, SIMULATIONOFF == true:
    // `rot` unused); the inputs stay untouched until the commit, so a restart is exact
    auto init_state = [&]() {
        rr0 = make_double2(0, 0); rr1 = rr0; rr2 = rr0; yb = rr0;
        if (own) {
            rr0 = *reinterpret_cast<const double2*>(Rs + b0);
            rr1 = *reinterpret_cast<const double2*>(Rs + n + b0);
            rr2 = *reinterpret_cast<const double2*>(Rs + 2 * n + b0);
            yb = *reinterpret_cast<const double2*>(y + b0);
        }
#pragma unroll
        for (int a = 0; a < 9; a++) R33[a] = Rs[(a / 3) * n + (a % 3)];
        if (p.phase & PHASE_PREDICT) {
            const double x0 = p.pose[3 * e + 0], y0 = p.pose[3 * e + 1], t0 = p.pose[3 * e + 2];
            const double* enc = p.enc + 3 * e;
            const double u2 = t0 - enc[2];
            const double dx = x0 - enc[0], dy = y0 - enc[1];
            const double u0 = sqrt(dx * dx + dy * dy);
            const double c = u2 / 2.0 + t0;
            double sc, cc;
            sincos(c, &sc, &cc);
            F3[2] = -u0 * sc;
            F3[5] = u0 * cc;
            // cos/sin(t0 + u2/2) of Robot.cpp:150-151: the same angle as c (addition commutes)
            xp[0] = x0 + u0 * cc;
            xp[1] = y0 + u0 * sc;
            xp[2] = t0 + u2;
            predict_cols(F3, rr0, rr1, rr2);
            // 3×3 block: F3·P33·F3ᵀ + Fu3·Q·Fu3ᵀ (Robot.cpp:178-258)
            const double Fu3[9] = {cc, 0, -u0 * sc / 2.0, sc, 1, u0 * cc / 2.0, 0, 0, 1};
            const double qs = (-1.0 / (1 + fabs(u0)) + 1);
            const double Q[9] = {p.enc_noise * qs, 0, 0, 0, 2 * p.enc_noise * qs, 0, 0, 0,
                                 p.enc_noise * qs};
            double FP[9], FuQ[9];
            for (int a = 0; a < 3; a++)
                for (int b = 0; b < 3; b++) {
                    double s = 0.0, t = 0.0;
                    for (int k = 0; k < 3; k++) {
                        s += F3[a * 3 + k] * R33[k * 3 + b];
                        t += Fu3[a * 3 + k] * Q[k * 3 + b];
                    }
                    FP[a * 3 + b] = s;
                    FuQ[a * 3 + b] = t;
                }
            for (int a = 0; a < 3; a++)
                for (int b = 0; b < 3; b++) {
                    double s = 0.0, t = 0.0;
                    for (int k = 0; k < 3; k++) {
                        s += FP[a * 3 + k] * F3[b * 3 + k];
                        t += FuQ[a * 3 + k] * Fu3[b * 3 + k];
                    }
                    R33[a * 3 + b] = s + t;
                }
        } else {
            xp[0] = p.xpre[3 * e + 0];
            xp[1] = p.xpre[3 * e + 1];
            xp[2] = p.xpre[3 * e + 2];
        }
    };
    // the owned diagonal block as last flushed (the staged speculative path guesses from it),
    // issued with the owned-state loads: the scan's inputs arrive in one memory round trip
    typename Stor<T>::C dj0[4] = {0, 0, 0, 0};
    double4 djb = make_double4(0, 0, 0, 0);   // the kept diagonal block (split-bf16 contexts)
    if (own && (p.phase & PHASE_UPDATE)) {
        PllView<T> v0;
        v0.X = reinterpret_cast<const T*>(p.Pread) + (size_t)e * d.ntiles * TILE_ELEMS;
        v0.nb = d.nb;
        v0.rnd = 1;
        load_block<T>(v0, 2 * j, 2 * j, dj0);
        if (Ddr && p.npend > 0) djb = Ddr[j];
    }
    // the scan's other inputs, issued with the state loads (one memory round trip): the pending
    // steps' control words, the line count, savedLineCount and the line words
    int4 ctl_pre = make_int4(0, 0, 0, 0);
    int psg_pre = 0;
    if ((p.phase & PHASE_UPDATE) && tid < p.npend) {
        const int* r = p.pend[tid].res + (size_t)e * RES_STRIDE;
        ctl_pre = make_int4(r[RES_RESET], r[RES_KSTEPS], r[RES_NADD], r[RES_SAVED_IN]);
        psg_pre = r[RES_PSIG];
    }
    const int L_pre = p.nlines[e];
    const int s_pre = (p.phase & PHASE_UPDATE) ? p.saved[e] : 0;
    constexpr int LW_PER = (EKF_MAX_LINES * 6 + SCAN_BLOCK - 1) / SCAN_BLOCK;
    double lw_pre[LW_PER];
    {
        const double* src = reinterpret_cast<const double*>(p.lines + (size_t)e * d.max_lines);
#pragma unroll
        for (int k = 0; k < LW_PER; k++) {
            const int idx = tid + k * SCAN_BLOCK;
            lw_pre[k] = ((p.phase & PHASE_UPDATE) && idx < d.max_lines * 6) ? src[idx] : 0.0;
        }
    }
    init_state();
    // the owned landmark's angle at the start of the scan and its sin/cos (sincos_near)
    // sin/cos of the owned landmark's scan-start angle: fp32 now (the quick filter's bound and the
    // guess), the exact fp64 ones (sincos_near) only where a lane needs the exact evaluation
    double ma0 = yb.x, s0j = 0.0, c0j = 1.0;
    bool sc_exact = false;
    float s0f = 0.f, c0f = 1.f;
    if (own && (p.phase & PHASE_UPDATE)) __sincosf((float)ma0, &s0f, &c0f);
    auto exact_sc = [&]() {
        if (!sc_exact) {
            sincos(ma0, &s0j, &c0j);
            sc_exact = true;
        }
    };

    if (!(p.phase & PHASE_UPDATE)) {
        // predict only: the predicted robot strip (and the mean, unchanged) into the other copy,
        // the 3×3 block and x_pre by the lead once every workgroup completed
        if (own) {
            *reinterpret_cast<double2*>(Rsw + b0) = rr0;
            *reinterpret_cast<double2*>(Rsw + n + b0) = rr1;
            *reinterpret_cast<double2*>(Rsw + 2 * n + b0) = rr2;
            *reinterpret_cast<double2*>(yw + b0) = yb;
            if (Ddr) Ddw[j] = Ddr[j];
        }
        if (tid == 0 && g != 0) publish_done(sync, g, p.epoch, 0);
        if (g == 0) {
            int zg_unused = 0;
            const int st = lead_collect<SCAN_BLOCK>(sync, G, p.epoch, 0, p.spin_log2, tid, sh_red, zg_unused);
            if (lead) sync[SYNC_WG0] = (int)done_word(p.epoch, st);
            if (lead && !(st & EKF_ST_TIMEOUT_BIT)) {
                for (int a = 0; a < 9; a++) Rsw[(a / 3) * n + (a % 3)] = R33[a];
                yw[0] = y[0]; yw[1] = y[1]; yw[2] = y[2];
                p.xpre[3 * e + 0] = xp[0];
                p.xpre[3 * e + 1] = xp[1];
                p.xpre[3 * e + 2] = xp[2];
                p.live[e] = 1 - cb;
            }
        }
        return;
    }
    EKF_STAMP(0);

    // ---------------- association / update (Robot.cpp:288-904) ----------------
    const size_t opstride = (size_t)d.nb * 64 * (d.kmax / 2);
    double* Ust = p.Ust + (size_t)e * d.max_lines * n * 2;
    double* Vst = p.Vst + (size_t)e * d.max_lines * n * 2;
    using C = typename Stor<T>::C;   // operand (compute) type
    C* Uop = reinterpret_cast<C*>(p.cur.Uop) + (size_t)e * opstride;
    C* Vop = reinterpret_cast<C*>(p.cur.Vop) + (size_t)e * opstride;
    // split-plane arithmetics: V's planes for the split flush (null otherwise)
    unsigned short* Bop = p.cur.Bop ? reinterpret_cast<unsigned short*>(p.cur.Bop) + (size_t)e * opstride * npl
                                    : nullptr;
    // (staged in LDS, sh_vpl, and written once at the end: per-match 2-byte global stores cost
    // ≈4 µs of the chain, since on CDNA every store counts in vmcnt and each later load wait
    // then also waited for them)
    double* patch = p.cur.patch + (size_t)e * d.max_lines * 2 * M;
    double* pdiag = p.cur.patch_diag + (size_t)e * d.max_lines * 4;
    int* res = p.cur.res + (size_t)e * RES_STRIDE;

    PllView<T> pv;
    pv.X = reinterpret_cast<const T*>(p.Pread) + (size_t)e * d.ntiles * TILE_ELEMS;
    pv.nb = d.nb;
    pv.kmax = d.kmax;
    pv.M = M;
    pv.max_lines = d.max_lines;
    pv.e = e;
    pv.ex = storage_exp<T>(p.pexp, e);
    pv.opstride = opstride;
    pv.usym = p.usym;
    pv.us = p.usym ? -ldexpf(1.0f, pv.ex) : 1.0f;
    pv.npend = p.npend;
    pv.pend = p.pend;
    pv.ctl = sh_ctl;
    pv.rnd = !p.bf;
    if (tid < p.npend) {
        sh_ctl[tid] = ctl_pre;
        sh_psg[tid] = psg_pre;
    }

    int L = L_pre;
    L = L < 0 ? 0 : (L > d.max_lines ? d.max_lines : L);
    const int s = s_pre;
#pragma unroll
    for (int k = 0; k < LW_PER; k++) {
        const int idx = tid + k * SCAN_BLOCK;
        if (idx < L * 6) reinterpret_cast<double*>(sh_lines)[idx] = lw_pre[k];
    }
    __syncthreads();   // sh_lines, sh_ctl

    const bool spec_ok = p.spec && L > 0 && L <= SPEC_L && s > 0 && G <= SPEC_GMAX;
    // symmetric downdate operands (sym_factor): fp32 operand storage, every mode but the
    // reference's asymmetric R
    const bool sym = HOT || (r_mode != 1 && sizeof(typename Stor<T>::C) == 4);
    // symmetric fp32 operands with kmax = 16: staged in LDS (sh_vpl) and written at the end
    const bool stage_ops = HOT || (sym && d.kmax == 16);
    // speculative path with fp32 operands and few pending steps: the pending steps' rows of the
    // guessed columns are staged in LDS and one pass per step updates all owned blocks
    bool staged = false;
    // split-bf16 contexts with plain pending steps (no reset, no augmented rows): the pending
    // steps are applied by bf16 MFMA on the operand planes (plane_replay) and the diagonal blocks
    // come from Dd (the last committed step's, exact); fp32 storage
    bool mf = false;
    int rpath = 0;   // diagnostic (RES_DBG): 64 the pending replay took an exact form, 128 a pending
                     // reset, 256 a pending plane exponent other than this scan's
    bool aug_pend = false;   // some pending step adds landmarks (uniform)
    unsigned amask = 0;   // pending steps with a downdate (ks > 0)
    // (the MFMA replay reads the planes, not the LDS stage: any number of pending steps)
    if (spec_ok && sym && sizeof(typename Stor<T>::C) == 4 && d.kmax / 2 >= 8) {
        __syncthreads();   // sh_ctl
        bool st = true;
        for (int q = 0; q < p.npend; q++) st &= sh_ctl[q].y <= 8;
        // pending steps that add landmarks stay on the MFMA replay: a block touching a landmark
        // added at step q* starts from q*'s patch (its V rows are zero before), below; a reset or
        // a plane exponent other than this scan's takes the exact forms
        bool m = st && p.mfrep && kPlanes;
        if (pf16 && p.mfrep == 1) {
            for (int q = 0; q < p.npend; q++) f32rep |= sh_psg[q] != psig;
            rrsc = f32rep ? 1.0 : rsc;
        }
        for (int q = 0; q < p.npend; q++) {
            // (the planes of a step written with another exponent: only the plane replay minds)
            const bool sgx = pf16 && !f32rep && sh_psg[q] != psig;
            m &= !sh_ctl[q].x && !sgx;
            rpath |= (sh_ctl[q].x ? 128 : 0) | (pf16 && sh_psg[q] != psig ? 256 : 0);
            aug_pend |= sh_ctl[q].z > 0;
            if (sh_ctl[q].y > 0) amask |= 1u << q;
        }
        staged = st && (p.npend <= SPEC_QMAX || m);
        mf = m && staged;
    }
    // fp64 storage, plain pending steps (no reset, no augmented rows): the owned rows' blocks of
    // the guessed columns and the owned diagonal blocks by v_mfma_f64_16x16x4f64 over the pending
    // steps' operand rows, the flush's own instruction on its own operands (below, phase (e))
    bool m64 = false;
    if constexpr (sizeof(typename Stor<T>::C) == 8)
        if (spec_ok && p.mfrep64 && d.kmax == 16 && p.npend > 0) {
            bool m = true;
            for (int q = 0; q < p.npend; q++) m &= !sh_ctl[q].x && sh_ctl[q].z == 0;
            m64 = m;
        }
    if (p.npend > 0 && !mf && !m64) rpath |= 64;
    double Dj[4] = {0, 0, 0, 0};   // owned diagonal block
    if (own && j < s) {
        if (mf && p.npend > 0) {
            Dj[0] = djb.x; Dj[1] = djb.y; Dj[2] = djb.z; Dj[3] = djb.w;
        } else if (staged || m64) {
            // the guess only needs it approximately: the last flushed value (exact one below)
#pragma unroll
            for (int a = 0; a < 4; a++) Dj[a] = from_domain<T>(dj0[a], pv.ex);
        } else {
            pll_block(pv, 2 * j, 2 * j, Dj);
        }
    }
    EKF_STAMP(1);

    // writes a match's owned rows: U/V history and the MFMA downdate operands
    // F: the line's symmetric operand factor (sym_factor; unused otherwise)
    bool nzr = false;   // this thread wrote a nonzero operand row (DONE_NZ, RES_ZMAX)
    // the scan's downdate of the owned 2×2 diagonal block, trace (Σ over matches and both rows of
    // −U·V ≥ 0): with the block after the scan it measures the update's cancellation (EKF_ST_PRECISION)
    double dsq = 0.0;
    // uhist: keep the U rows for later corrections (the sequential path; the speculative landmark
    // waves apply each match to the later blocks at once and keep only the last one, in registers)
    auto store_rows = [&](int t, const double kk[4], const double uu[4], bool vhist, const float F[3], bool uhist) {
        nzr = nzr || kk[0] != 0.0 || kk[1] != 0.0 || kk[2] != 0.0 || kk[3] != 0.0 || uu[0] != 0.0 ||
              uu[1] != 0.0 || uu[2] != 0.0 || uu[3] != 0.0;
        if (!uhist) {
        } else if (t < HIST_LDS)
            sh_uhist[t][tid] = make_double4(uu[0], uu[1], uu[2], uu[3]);
        else
            *reinterpret_cast<double4*>(Ust + ((size_t)t * n + b0) * 2) = make_double4(uu[0], uu[1], uu[2], uu[3]);
        if (vhist) {
            if (t < HIST_V)
                sh_vhist[t][tid] = make_double4(kk[0], kk[1], kk[2], kk[3]);
            else
                *reinterpret_cast<double4*>(Vst + ((size_t)t * n + b0) * 2) = make_double4(kk[0], kk[1], kk[2], kk[3]);
        }
#pragma unroll
        for (int pp = 0; pp < 2; pp++) {
            const int lr = 2 * j + pp;
            if constexpr (sizeof(C) == 4) {
                double o0 = uu[2 * pp], o1 = uu[2 * pp + 1], v0 = kk[2 * pp], v1 = kk[2 * pp + 1];
                if (sym) {   // V = K·F, U = −2^x·V (sym_factor)
                    v0 = kk[2 * pp] * (double)F[0] + kk[2 * pp + 1] * (double)F[1];
                    v1 = kk[2 * pp + 1] * (double)F[2];
                    o0 = (double)(float)v0;
                    o1 = (double)(float)v1;
                }
                dsq += o0 * v0 + o1 * v1;   // (row pp's diagonal entry falls by it)
                if (stage_ops) {
                    // staged in LDS: the operand rows (U, V, the bf16 planes) go out once at the end
                    // of the scan as whole 16-byte lane rows
                    if constexpr (kPlanes)
                        *reinterpret_cast<f32x2v*>(sh_vpl + tid * 32 + pp * 16 + 2 * t) = f32x2v{(float)v0, (float)v1};
                } else {
                    if (!p.usym) {   // (symmetric operands: U = −2^x·V, read from V)
                        Uop[op_index_f32(lr, 2 * t, d.kmax)] = to_domain<T>(-o0, pv.ex);
                        Uop[op_index_f32(lr, 2 * t + 1, d.kmax)] = to_domain<T>(-o1, pv.ex);
                    }
                    Vop[op_index_f32(lr, 2 * t, d.kmax)] = (C)v0;
                    Vop[op_index_f32(lr, 2 * t + 1, d.kmax)] = (C)v1;
                }
            } else {
                Uop[op_index_f64(lr, 2 * t, d.kmax)] = (C)(-uu[2 * pp]);
                Uop[op_index_f64(lr, 2 * t + 1, d.kmax)] = (C)(-uu[2 * pp + 1]);
                Vop[op_index_f64(lr, 2 * t, d.kmax)] = (C)kk[2 * pp];
                Vop[op_index_f64(lr, 2 * t + 1, d.kmax)] = (C)kk[2 * pp + 1];
            }
        }
    };
    auto uq_owned = [&](int q) -> double4 {
        return q < HIST_LDS ? sh_uhist[q][tid] : *reinterpret_cast<const double4*>(Ust + ((size_t)q * n + b0) * 2);
    };
    // symmetric operands from their LDS stage (stage_ops): per owned row and k parity h one 16-byte
    // half of the 32-byte lane row, half 0 = k slots 0..3 (matches 0..3), half 1 = slots 4..7; V and
    // U = −2^x·V (exact); k past the matches +0 (V) and −0 (U), so that a flush running every
    // k-step leaves every value as it is (flush_f32_wave_kernel; the other forms and the on-read
    // replay stop at ks). Half 0 is final after the fourth match: the speculative path stores it
    // then, during the later lines (the commit's stores are issue-bound, ≈10 B/clk per CU)
    int ops_early = 0;
    auto store_ops_half = [&](int half, int mm) {   // mm: the matches
        if constexpr (kPlanes) {
            const float us = -ldexpf(1.0f, pv.ex);
            const bool su = !p.usym;   // (usym: U = us·V is not stored; the readers scale V)
#pragma unroll
            for (int pp = 0; pp < 2; pp++) {
                const f32x4v* src = reinterpret_cast<const f32x4v*>(sh_vpl + tid * 32 + pp * 16) + 2 * half;
                float v[8];
#pragma unroll
                for (int i = 0; i < 2; i++) {
                    const f32x4v x = src[i];
#pragma unroll
                    for (int u = 0; u < 4; u++) v[4 * i + u] = (8 * half + 4 * i + u) < 2 * mm ? x[u] : 0.f;
                }
#pragma unroll
                for (int h = 0; h < 2; h++) {
                    const size_t o = op_index_f32(2 * j + pp, h, d.kmax) + 4 * half;   // k = h: s = 0
                    const f32x4v vh = {v[h], v[2 + h], v[4 + h], v[6 + h]};
                    *reinterpret_cast<f32x4v*>(Vop + o) = vh;
                    if (su) *reinterpret_cast<f32x4v*>(Uop + o) = vh * us;
                }
            }
        }
    };

    bool matched = false;
    int m = 0, nextra = 0, status = 0, tstatus = 0;
    int dpath = 0;   // diagnostic: 1 fast guess, 2 collision-resolved guess, 4 unresolved, 8 verdict failed,
                     // 32 a guessed winner failed its exact gate and its line stayed unmatched (16: sequential;
                     // 64-256: rpath)
    int par0 = 0;   // mailbox parity of line 0 on the sequential path
    bool sequential = true;
    // a restart after a failed verdict keeps the lines before the first violating one: every
    // workgroup replays them from the speculative packages (no gate, no exchange; the state, rows
    // and status bits the sequential path computes for them), then the sequential path takes over
    int keep = 0;
    // a restart after a failed verdict: the owned blocks of the guessed columns as the speculative
    // pass computed them (scan start, pending steps applied) serve the lines whose winner was guessed
    bool blk_cached = false;
    float4 (*const sh_cblk)[SCAN_THREADS] = reinterpret_cast<float4 (*)[SCAN_THREADS]>(sh_stg);

    if (spec_ok) {
        // ---- (a) guesses: per line, does the owned landmark pass under the predicted state ----
        unsigned gp = 0;
        if (own && j < s) {
            Block5 b5;
            fill_block5(b5, R33, rr0, rr1, rr2, Dj);
            Guess gs;
            guess_prep(b5, yb.x, yb.y, xp, gs);
#pragma unroll
            for (int t = 0; t < SPEC_L; t++) {
                if (t >= L) break;
                const ekf_line ln = sh_lines[t];
                double Rm[4];
                line_R(ln, t, r_mode, Rm);
                if (guess_pass(gs, ln.alpha, ln.r, Rm, p.gate)) gp |= 1u << t;
            }
            if (p.spec == 2 && L > 1)   // test hook: every guess taken from the next line
                gp = ((gp >> 1) | (gp << (L - 1))) & ((1u << L) - 1u);
            if (p.spec == 3 && L > 3) {
                // test hook: the guesses of lines L/2 .. L − 1 taken from the next of them (the
                // lines before stay right: a failed verdict keeps them)
                const int h = L / 2, nh = L - h;
                const unsigned hi = (gp >> h) & ((1u << nh) - 1u);
                gp = (gp & ((1u << h) - 1u)) | ((((hi >> 1) | (hi << (nh - 1))) & ((1u << nh) - 1u)) << h);
            }
        }
        // per wave and line the guessed candidates (ballot), then the workgroup's first SPEC_K
        // in landmark order: word A = 8-bit local indices 0..3 | count << 32 | more << 36, word B =
        // local indices 4..7
        for (int t = 0; t < L; t++) {
            const unsigned long long mk = __ballot((gp >> t) & 1u);
            if ((tid & 63) == 0 && tid < SCAN_THREADS) sh_wl[t][tid >> 6] = mk;
        }
        __syncthreads();
        if (tid < L) {
            unsigned long long word = 0, wordb = 0;
            int cnt = 0, more = 0;
            for (int w = 0; w < SCAN_THREADS / 64 && !more; w++) {
                unsigned long long mk = sh_wl[tid][w];
                while (mk) {
                    if (cnt == SPEC_K) { more = 1; break; }
                    const int b = __builtin_ctzll(mk);
                    mk &= mk - 1;
                    if (cnt < 4) word |= (unsigned long long)(w * 64 + b) << (8 * cnt);
                    else wordb |= (unsigned long long)(w * 64 + b) << (8 * (cnt - 4));
                    cnt++;
                }
            }
            word |= ((unsigned long long)cnt << LW_CNT) | ((unsigned long long)more << LW_MORE);
            sh_lists[g * SPEC_L + tid] = word;
            sh_listsb[g * SPEC_L + tid] = wordb;
        }
        __syncthreads();
        EKF_STAMP(5);
        // ---- (b) exchange 1 (parity 0): every workgroup's lists ----
        if (G > 1) {
            // self-tagged words per (workgroup, line), polled directly by their readers: A always,
            // B (at SPEC_L words further) only when A's count says it is there
            const int lb = p.mbw - MB_LIST_BACK;
            double* slot = mbox + (size_t)g * p.mbw + lb;
            if (tid < SPEC_L) {
                const unsigned long long wa = tid < L ? sh_lists[g * SPEC_L + tid] : 0ull;
                if (((wa >> LW_CNT) & 15) > 4) mb_store_tagged(slot + SPEC_L + tid, p.epoch, sh_listsb[g * SPEC_L + tid]);
                mb_store_tagged(slot + tid, p.epoch, wa);
            }
            for (int k = tid; k < G * L; k += SCAN_BLOCK) {
                const int gq = k / L, t = k - gq * L;
                if (gq != g) {
                    const double* src = mbox + (size_t)gq * p.mbw + lb;
                    const unsigned long long wa = mb_wait_tagged(src + t, p.epoch, tstatus, p.spin_log2);
                    sh_lists[gq * SPEC_L + t] = wa;
                    if (((wa >> LW_CNT) & 15) > 4)
                        sh_listsb[gq * SPEC_L + t] = mb_wait_tagged(src + SPEC_L + t, p.epoch, tstatus, p.spin_log2);
                }
            }
            __syncthreads();
        }
        EKF_STAMP(2);
        // ---- (c) guessed winners (every workgroup computes the same). Fast form: per line the
        // instance's first guessed candidate (workgroups are in landmark order); if those are
        // distinct they are the winners. Otherwise, per line the first SPEC_K guessed candidates,
        // and in line order the first one not taken by an earlier line. ----
        // per line the first guessed candidate over all workgroups: one list word per thread, an LDS
        // atomic minimum per line (sh_first, reset at the start of the kernel)
        for (int k = tid; k < G * SPEC_L; k += SCAN_BLOCK) {
            const int gq = k / SPEC_L, t = k - gq * SPEC_L;
            const unsigned long long w = sh_lists[gq * SPEC_L + t];
            if (t < L && ((w >> LW_CNT) & 15)) atomicMin(&sh_first[t], gq * SCAN_THREADS + (int)(w & 255));
        }
        __syncthreads();
        {
            int first[SPEC_L];
#pragma unroll
            for (int t = 0; t < SPEC_L; t++) first[t] = sh_first[t];
            if (tid == 0) {
                bool distinct = true;
#pragma unroll
                for (int t = 0; t < SPEC_L; t++)
#pragma unroll
                    for (int q = 0; q < t; q++)
                        distinct &= !(t < L && first[t] != 0x7fffffff && first[t] == first[q]);
#pragma unroll
                for (int t = 0; t < SPEC_L; t++) sh_spec[t] = first[t] == 0x7fffffff ? -1 : first[t];
                sh_flag = distinct ? 0 : 2;
            }
        }
        __syncthreads();
        dpath = sh_flag == 2 ? 2 : 1;
        if (sh_flag == 2) {
            if (tid < L) {
                int cnt = 0, more = 0;
                for (int gq = 0; gq < G && cnt < SPEC_K; gq++) {
                    const unsigned long long w = sh_lists[gq * SPEC_L + tid];
                    const unsigned long long wb = sh_listsb[gq * SPEC_L + tid];
                    const int c = (int)((w >> LW_CNT) & 15);
                    for (int k = 0; k < c; k++) {
                        const int loc = (int)(((k < 4 ? w : wb) >> (8 * (k & 3))) & 255);
                        if (cnt < SPEC_K) sh_glist[tid][cnt++] = gq * SCAN_THREADS + loc;
                        else more = 1;
                    }
                    if ((w >> LW_MORE) & 1) more = 1;
                }
                sh_glist[tid][SPEC_K] = cnt | (more << 8);
            }
            __syncthreads();
            if (tid == 0) {
                int spec[SPEC_L];
                int unresolved = 0;
    #pragma unroll
                for (int t = 0; t < SPEC_L; t++) {
                    spec[t] = -1;
                    if (t < L) {
                        const int info = sh_glist[t][SPEC_K];
                        const int cnt = info & 255;
                        int w = -1;
    #pragma unroll
                        for (int k = 0; k < SPEC_K; k++) {
                            const int cand = sh_glist[t][k];
                            bool taken = false;
    #pragma unroll
                            for (int q = 0; q < t; q++) taken |= (spec[q] == cand);
                            if (k < cnt && w < 0 && !taken) w = cand;
                        }
                        if (w < 0 && (info >> 8)) unresolved = 1;
                        spec[t] = w;
                    }
                }
    #pragma unroll
                for (int t = 0; t < SPEC_L; t++) sh_spec[t] = spec[t];
                sh_flag = unresolved;
            }
            __syncthreads();
        }
        EKF_STAMP(10);

        if (!sh_flag) {
            sequential = false;
            // ---- (d) the winners' records straight from memory, as their owners hold them:
            // predicted robot-strip columns and mean, diagonal block, blocks of the earlier
            // winners' columns; and (staged replay) the guessed columns' rows of the pending
            // steps' operands ----
            // staged path: everything below is issued before one barrier, so that the stored
            // blocks of the owned row (landmark waves), the winners' records and mutual blocks
            // (replay wave) and the staged operand rows arrive in one memory round trip
            int cols[SPEC_L];
#pragma unroll
            for (int t = 0; t < SPEC_L; t++) {
                const int w = t < L ? sh_spec[t] : -1;
                cols[t] = w >= 0 ? w : j;
            }
            // per guessed winner t (lane t of every wave): the latest pending step that added it,
            // or -1; read with __shfl, so that no wave waits for another's (the MFMA-replay path
            // has no barrier between the records and the waves' replays)
            int addq_l = -1;
            if (mf && aug_pend) {
                const int lt = tid & 63;
                const int w = lt < L ? sh_spec[lt] : -1;
                if (w >= 0)
                    for (int q = 0; q < p.npend; q++)
                        if (w >= sh_ctl[q].w && w < sh_ctl[q].w + sh_ctl[q].z) addq_l = q;
            }
            C srow[SPEC_L + 1][4];
            if ((staged || m64) && own) staged_blocks_load<T>(pv, j, cols, srow);
            int pu = 0, pt = 0;   // replay-wave lane → mutual block (pu, pt), pt <= pu
            C pacc[4] = {0, 0, 0, 0};
            const int lane_r = tid - SCAN_THREADS;
            // fp64 MFMA-replay contexts: the winners' mutual blocks from their U and V rows of every
            // pending step staged in LDS (m64s, below) instead of a memory round trip per step
            const bool m64s = m64 && p.npend <= M64_QMAX;
            if ((staged || m64s) && tid >= SCAN_THREADS && lane_r < L * (L + 1) / 2) {
                pt = lane_r;
                while (pt > pu) { pt -= pu + 1; pu++; }
                if (sh_spec[pu] >= 0 && sh_spec[pt] >= 0) pair_block_load<T>(pv, sh_spec[pu], sh_spec[pt], pacc);
            }
            if constexpr (sizeof(C) == 8)
                if (m64s) {
                    // rows 2w, 2w + 1 of U_q and V_q of every guessed winner w and pending step q,
                    // all loads in flight together: pieces of 4 doubles (k = 16·kk + s, s < 4, as
                    // pll_blocks reads them), [t][q][U, V][row][kk][s] (m64_stage_index), in history
                    // slots 1.. (unused until the line loop's second match; slot 0 holds the
                    // landmark waves' diagonal blocks meanwhile, the fp32 stage is not allocated here)
                    static_assert((HIST_LDS - 1) * SCAN_THREADS * sizeof(double4) >= SPEC_L * M64_QMAX * 64 * sizeof(double),
                                  "fp64 winners' stage");
                    double* stg64 = reinterpret_cast<double*>(&sh_uhist[1][0]);
                    typedef double d64x2 __attribute__((ext_vector_type(2)));
                    const int nld = L * p.npend * 16;
                    for (int k = tid; k < nld; k += SCAN_BLOCK) {
                        const int piece = k & 15, tq = k >> 4, q = tq % p.npend, t = tq / p.npend;
                        const int w = sh_spec[t];
                        if (w < 0 || sh_ctl[q].y <= 0) continue;
                        const int uv = piece >> 3, rr = (piece >> 2) & 1, kk = piece & 3;
                        const int r = 2 * w + rr;
                        const double* base = reinterpret_cast<const double*>(uv ? p.pend[q].Vop : p.pend[q].Uop) + e * opstride;
                        const d64x2* src = reinterpret_cast<const d64x2*>(
                            base + ((size_t)(r >> 5) * 64 + (r & 15)) * 8 + ((r >> 4) & 1) * 4 + 128 * kk);
                        d64x2* dst = reinterpret_cast<d64x2*>(stg64 + m64_stage_index(t, q, uv, rr, kk));
                        dst[0] = src[0];
                        dst[1] = src[1];
                    }
                }
            if (!staged && !m64s && tid < L * (L + 1) / 2) {
                int u = 0, t = tid;
                while (t > u) { t -= u + 1; u++; }
                const int wu = sh_spec[u], wt = sh_spec[t];
                if (wu >= 0 && wt >= 0) {
                    double bk[4];
                    pll_block(pv, 2 * wu, 2 * wt, bk);
                    double* r = sh_wd + u * SPEC_WD + (t == u ? 6 : 14 + 4 * t);
                    r[0] = bk[0]; r[1] = bk[1]; r[2] = bk[2]; r[3] = bk[3];
                }
            }
            if (tid >= SCAN_THREADS && tid < SCAN_THREADS + L) {
                const int u = tid - SCAN_THREADS, wu = sh_spec[u];
                if (wu >= 0) {
                    const int bw = 3 + 2 * wu;
                    double2 q0 = *reinterpret_cast<const double2*>(Rs + bw);
                    double2 q1 = *reinterpret_cast<const double2*>(Rs + n + bw);
                    double2 q2 = *reinterpret_cast<const double2*>(Rs + 2 * n + bw);
                    const double2 qy = *reinterpret_cast<const double2*>(y + bw);
                    if (p.phase & PHASE_PREDICT) predict_cols(F3, q0, q1, q2);
                    double* r = sh_wd + u * SPEC_WD;
                    r[0] = q0.x; r[1] = q0.y; r[2] = q1.x; r[3] = q1.y; r[4] = q2.x; r[5] = q2.y;
                    r[10] = qy.x; r[11] = qy.y;   // (sin/cos of the angle: by the replay wave, after the barrier)
                }
            }
            if (staged && !mf) {
                // rows 2w, 2w+1 of U_q and V_q of every guessed column w, pending step q (4 row
                // halves × 8 k each; the V side interleaved, stage_v_index): 16 pieces of 4 floats
                const int kh = d.kmax / 2;
                const int nld = L * p.npend * 16;
                for (int k = tid; k < nld; k += SCAN_BLOCK) {
                    const int piece = k & 15, tq = k >> 4, q = tq % p.npend, t = tq / p.npend;
                    const int w = sh_spec[t];
                    if (w < 0) continue;
                    const size_t rowb = ((size_t)((2 * w) >> 5) * 64 + ((2 * w) & 31)) * kh;
                    float* dst = sh_stg + ((t * SPEC_QMAX + q) * 2) * 32;
                    if (piece < 8) {   // U: row half rh, 4 k
                        const int half = piece & 1, rh = piece >> 1;
                        const float* base = u_rows_f32(pv, p.pend[q]) + rowb;
                        const int roff = (rh & 1) * kh + (rh >> 1) * 32 * kh;
                        *reinterpret_cast<f32x4v*>(dst + rh * 8 + half * 4) =
                            *reinterpret_cast<const f32x4v*>(base + roff + half * 4) * pv.us;
                    } else {           // V: rows of pair pr, k-pairs 2kc, 2kc + 1, interleaved
                        const int pr = (piece - 8) >> 2, kc = (piece - 8) & 3;
                        const float* base = reinterpret_cast<const float*>(p.pend[q].Vop) + e * opstride + rowb;
                        const f32x2v a = *reinterpret_cast<const f32x2v*>(base + (2 * pr) / 2 * 32 * kh + 2 * kc);
                        const f32x2v c = *reinterpret_cast<const f32x2v*>(base + kh + pr * 32 * kh + 2 * kc);
                        *reinterpret_cast<f32x4v*>(dst + 32 + pr * 16 + 4 * kc) = f32x4v{a[0], c[0], a[1], c[1]};
                    }
                }
            }
            // the guessed winners' addition steps of this lane's mutual block (the replay wave), and of
            // every guessed column (the landmark waves): shuffles with the whole wave active
            const int qs_pair = mf && aug_pend ? max(__shfl(addq_l, pu, 64), __shfl(addq_l, pt, 64)) : -1;
            int addq_t[SPEC_L];
#pragma unroll
            for (int t = 0; t < SPEC_L; t++) addq_t[t] = mf && aug_pend ? __shfl(addq_l, t, 64) : -1;
            // MFMA replay (mf): no barrier here. Each wave reads only what it wrote itself or what
            // an earlier barrier published — the replay wave its winners' records (sh_wd), the
            // landmark waves their owned rows' blocks — so the landmark waves replay the pending
            // steps while the replay wave loads the records and replays the winners' mutual blocks,
            // and its chain starts without waiting for them (the packages and the winners' V rows
            // then reach the landmark waves through sh_ready, release / acquire)
            if (!mf) __syncthreads();
            if (mf && tid >= SCAN_THREADS) {
              if constexpr (kPlanes) {
                // the winners' mutual blocks: X minus the pending steps' ΔX of the 16 winner rows
                // against themselves (one M-block of plane_replay), by the replay wave itself
                auto wrow = [&](int c) {
                    const int t = c >> 1;
                    const int w = t < L ? sh_spec[t] : -1;
                    return w >= 0 ? 2 * w + (c & 1) : -1;
                };
                f32x4v dacc[1];
                if (f32rep)
                    f32_replay<1>(p.pend, e, opstride, M, amask, lane_r, [&](int, int r) { return wrow(r); }, wrow, dacc);
                else if (HOT == 2 || (HOT == 0 && pf16))
                    plane_replay<1, true, 4>(p.pend, e, opstride * 2, M, amask, lane_r, [&](int, int r) { return wrow(r); }, wrow, dacc);
                else
                    plane_replay<1, false, 4>(p.pend, e, opstride * 3, M, amask, lane_r, [&](int, int r) { return wrow(r); }, wrow, dacc);
                float* scr = sh_stg;   // (not staged in this mode) 16 × 16 floats
#pragma unroll
                for (int i = 0; i < 4; i++) scr[(4 * (lane_r >> 4) + i) * 16 + (lane_r & 15)] = dacc[0][i];
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                if (lane_r < L * (L + 1) / 2 && sh_spec[pu] >= 0 && sh_spec[pt] >= 0) {
                    const bool swap = ((2 * sh_spec[pu]) >> 5) > ((2 * sh_spec[pt]) >> 5);
                    C xr[4] = {pacc[0], swap ? pacc[2] : pacc[1], swap ? pacc[1] : pacc[2], pacc[3]};
                    const int qs = qs_pair;   // (as for the landmark waves' blocks)
                    if (qs >= 0) patch_block<T>(pv, p.pend[qs], sh_ctl[qs], 2 * sh_spec[pu], 2 * sh_spec[pt], false, xr);
                    double* r = sh_wd + pu * SPEC_WD + (pt == pu ? 6 : 14 + 4 * pt);
#pragma unroll
                    for (int a = 0; a < 4; a++)
                        r[a] = from_domain<T>(xr[a], pv.ex) - (double)scr[(2 * pu + (a >> 1)) * 16 + 2 * pt + (a & 1)] * rrsc;
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
              }
            } else if ((staged || m64s) && tid >= SCAN_THREADS) {
                // the winners' mutual blocks from the staged rows, by the replay wave itself
                // (only it reads them): the landmark waves go straight on
                if (lane_r < L * (L + 1) / 2 && sh_spec[pu] >= 0 && sh_spec[pt] >= 0) {
                    double bk[4];
                    if constexpr (sizeof(C) == 8)
                        m64_pair_block<T>(pv, sh_spec[pu], pu, sh_spec[pt], pt,
                                          reinterpret_cast<const double*>(&sh_uhist[1][0]), pacc, bk);
                    else
                        staged_pair_block<T>(pv, sh_spec[pu], pu, sh_spec[pt], pt, sh_stg, pacc, bk);
                    double* r = sh_wd + pu * SPEC_WD + (pt == pu ? 6 : 14 + 4 * pt);
                    r[0] = bk[0]; r[1] = bk[1]; r[2] = bk[2]; r[3] = bk[3];
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            }
            EKF_STAMP(12);
            __shared__ unsigned long long sh_trec;   // diagnostics: the records' end (thread 0, WG 0)
            if (dbg) sh_trec = t_last;
            // ---- (f) the winners' part of the sequential chain, in the last wave (lane u carries
            // winner u's rows): per line the winner's lane evaluates it and writes the package,
            // then the later winners' lanes apply their gain rows. Meanwhile (g) the landmark
            // waves run every line as soon as its package is published (sh_ready). ----
            int viol = 0;
            int vline = L;   // the line of this thread's violation
            int stp = 0;     // its status bits per line (st_line)
            if (tid >= SCAN_THREADS) {
                const int u = tid - SCAN_THREADS;
                const unsigned long long t_l0 = __builtin_amdgcn_s_memrealtime();
                const bool act = u < L && sh_spec[u] >= 0;
                double R33l[9], xpl[3];
#pragma unroll
                for (int a = 0; a < 9; a++) R33l[a] = R33[a];
                xpl[0] = xp[0]; xpl[1] = xp[1]; xpl[2] = xp[2];
                double2 w0 = make_double2(0, 0), w1 = w0, w2 = w0, wy = w0;
                double wD[4] = {0, 0, 0, 0};
                double wma0 = 0.0, ws0 = 0.0, wc0 = 1.0;
                if (act) {
                    const double* r = sh_wd + u * SPEC_WD;
                    w0 = make_double2(r[0], r[1]); w1 = make_double2(r[2], r[3]);
                    w2 = make_double2(r[4], r[5]); wy = make_double2(r[10], r[11]);
                    wD[0] = r[6]; wD[1] = r[7]; wD[2] = r[8]; wD[3] = r[9];
                    wma0 = r[10];
                    sincos(wma0, &ws0, &wc0);   // sincos_near's scan-start values (as the owner's)
                }
                int ml = 0;
                const bool lst = pdbg && g == 0 && u == 0;
                unsigned long long tl = lst ? __builtin_amdgcn_s_memrealtime() : 0ull;
                // lane u evaluates line u: its line in registers, and the lines with a winner as a
                // wave-uniform mask (no LDS read on the chain)
                ekf_line lnu = {};
                if (u < L) lnu = sh_lines[u];
                const unsigned long long wmask = __ballot(act);
                for (int t = 0; t < L; t++) {
                    if (!((wmask >> t) & 1ull)) continue;
                    double* pk = sh_pk[t];
                    int okl = 1;
                    Cand c;
                    Block5 b5;
                    if (u == t) {
                        const ekf_line ln = lnu;
                        double Rm[4];
                        line_R(ln, t, r_mode, Rm);
                        fill_block5(b5, R33l, w0, w1, w2, wD);
                        double sn, cs;
                        sincos_near(wy.x, wma0, ws0, wc0, sn, cs);
                        // (its storage-precision margin and GSL_EDOM status after the package is out)
                        eval_candidate<false>(b5, wy.x, wy.y, sn, cs, xpl, ln.alpha, ln.r, Rm, p.gate, ETA, c);
                        okl = c.pass ? 1 : 0;
                        pk[PK_OK] = okl ? 1.0 : 0.0;
                    }
                    // the guessed winner failed its exact gate: no update from this line (the
                    // landmark waves check that no other landmark passes it)
                    const int ok = __builtin_amdgcn_readlane(okl, t);
                    if (ok && u == t) {
                        // the package in registers, the robot block after the line from it (for
                        // every lane and every landmark wave), then all of it to LDS
                        double pkl[PKW];
                        build_package(c, R33l, w0, w1, w2, pkl);   // its V rows stay in sh_wh[t]
                        robot_update(R33l, xpl, pkl);
#pragma unroll
                        for (int a = 0; a < 9; a++) pkl[PK_R33 + a] = R33l[a];
                        pkl[PK_XP + 0] = xpl[0]; pkl[PK_XP + 1] = xpl[1]; pkl[PK_XP + 2] = xpl[2];
                        // (the robot rows of K stay in registers: only robot_update, here, reads them;
                        // the symmetric operand factor is the landmark waves' own, from S)
#pragma unroll
                        for (int a = MB_S; a < PK_F; a++)
                            if (a < MB_KR || a >= MB_KR + 6) pk[a] = pkl[a];
                    }
                    // the package is complete: to the other lanes of this wave, and to the
                    // landmark waves (release of lane t's LDS writes, then the line counter)
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                    __builtin_amdgcn_wave_barrier();
                    if (u == 0) __hip_atomic_store(&sh_ready, t + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                    if (u == t) {
                        // GSL_EDOM of the winner (the reference evaluated it: Robot.cpp:454) and the
                        // gate's storage precision (gate_eta), off the line's chain
                        if (c.singular) atomicOr(&sh_rwst, st_line(EKF_ST_SINGULAR, t));
                        if (cand_amb(b5, c, p.gate, ETA)) atomicOr(&sh_rwst, st_line(EKF_ST_PRECISION_BIT, t));
                    }
                    if (!ok) continue;   // (ml counts matches: unchanged)
                    if (u != t) {   // (lane t has them)
#pragma unroll
                        for (int a = 0; a < 9; a++) R33l[a] = pk[PK_R33 + a];
                        xpl[0] = pk[PK_XP + 0]; xpl[1] = pk[PK_XP + 1]; xpl[2] = pk[PK_XP + 2];
                    }
                    if (lst) { const unsigned long long t2 = __builtin_amdgcn_s_memrealtime(); sh_stamp[3] += t2 - tl; tl = t2; }
                    if (act && u > t) {
                        const double* r = sh_wd + u * SPEC_WD + 14 + 4 * t;
                        double blk[4] = {r[0], r[1], r[2], r[3]};
                        double kk[4], uu[4];
                        gain_rows<SPEC_L>(pk, ml, [&](int q) { return sh_wh[u][q][0]; },
                                          [&](int q) { return sh_wh[t][q][1]; }, blk, w0, w1, w2, wy, wD, kk, uu);
                        sh_wh[u][ml][0] = make_double4(uu[0], uu[1], uu[2], uu[3]);
                        sh_wh[u][ml][1] = make_double4(kk[0], kk[1], kk[2], kk[3]);
                    }
                    ml++;
                    if (lst) { const unsigned long long t2 = __builtin_amdgcn_s_memrealtime(); sh_stamp[4] += t2 - tl; tl = t2; }
                }
                if (u == 0) {
                    sh_flag = 0;   // (a failed guessed winner is settled per line by the landmark waves)
                    if (pdbg && g == 0) {
                        const unsigned long long te = __builtin_amdgcn_s_memrealtime();
                        sh_stamp[13] += te - t_l0;
                        sh_stamp[29] += t_l0 - sh_trec;   // the replay wave's chain starts ...
                        sh_stamp[30] += te - sh_trec;     // ... and ends, after the records
                    }
                }
            } else {
                // ---- (e) owned blocks of the guessed columns (Robot.cpp:560 operands), while the
                // last wave runs (f) ----
                if (mf) {
                  if constexpr (kPlanes) {
                    // the owned rows' blocks of the guessed columns: X minus the pending steps' ΔX
                    // of the wave's 128 rows (8 M-blocks) against the 16 winner rows, transposed
                    // through this wave's part of sh_vpl (8 KB; the planes are staged there later)
                    const int l = tid & 63;
                    const int rbase = 2 * (g * SCAN_THREADS + (tid & ~63));
                    auto wrow = [&](int c) {
                        const int t = c >> 1;
                        const int w = t < L ? sh_spec[t] : -1;
                        return w >= 0 ? 2 * w + (c & 1) : -1;
                    };
                    f32x4v dacc[8];
                    if (f32rep)
                        f32_replay<8>(p.pend, e, opstride, M, amask, l,
                                      [&](int mb, int r) { return rbase + 16 * mb + r; }, wrow, dacc);
                    else if (HOT == 2 || (HOT == 0 && pf16))
                        plane_replay<8, true>(p.pend, e, opstride * 2, M, amask, l,
                                              [&](int mb, int r) { return rbase + 16 * mb + r; }, wrow, dacc);
                    else
                        plane_replay<8, false>(p.pend, e, opstride * 3, M, amask, l,
                                               [&](int mb, int r) { return rbase + 16 * mb + r; }, wrow, dacc);
                    float* scr = sh_vpl + (tid & ~63) * 32;
#pragma unroll
                    for (int mb = 0; mb < 8; mb++)
#pragma unroll
                        for (int i = 0; i < 4; i++) scr[(mb * 16 + 4 * (l >> 4) + i) * 16 + (l & 15)] = dacc[mb][i];
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                    __builtin_amdgcn_wave_barrier();
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                    if (own) {
                        const float* r0 = scr + ((l >> 3) * 16 + ((2 * l) & 15)) * 16;
                        f32x4v d0[4], d1[4];
#pragma unroll
                        for (int k = 0; k < 4; k++) {
                            d0[k] = *reinterpret_cast<const f32x4v*>(r0 + 4 * k);
                            d1[k] = *reinterpret_cast<const f32x4v*>(r0 + 16 + 4 * k);
                        }
                        // a block touching a landmark added during the pending steps starts from
                        // the patch of the step that added the later of its two landmarks (the
                        // higher index: landmarks are appended); the replay's ΔX holds only the
                        // steps after it (their V rows are zero before)
                        int qj = -1;
                        if (aug_pend)
                            for (int q = 0; q < p.npend; q++)
                                if (j >= sh_ctl[q].w && j < sh_ctl[q].w + sh_ctl[q].z) qj = q;
#pragma unroll
                        for (int t = 0; t < SPEC_L; t++)
                            if (t < L && sh_spec[t] >= 0) {
                                C b[4] = {srow[t][0], srow[t][1], srow[t][2], srow[t][3]};
                                const int qs = max(qj, addq_t[t]);
                                if (qs >= 0) patch_block<T>(pv, p.pend[qs], sh_ctl[qs], 2 * j, 2 * sh_spec[t], false, b);
                                const int c0 = 2 * t;
                                sh_blk[t][tid] = make_float4(
                                    (float)(from_domain<T>(b[0], pv.ex) - (double)d0[c0 >> 2][c0 & 3] * rrsc),
                                    (float)(from_domain<T>(b[1], pv.ex) - (double)d0[c0 >> 2][(c0 & 3) + 1] * rrsc),
                                    (float)(from_domain<T>(b[2], pv.ex) - (double)d1[c0 >> 2][c0 & 3] * rrsc),
                                    (float)(from_domain<T>(b[3], pv.ex) - (double)d1[c0 >> 2][(c0 & 3) + 1] * rrsc));
                            }
                    }
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                    __builtin_amdgcn_wave_barrier();
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                  }
                } else if (m64) {
                  if constexpr (sizeof(C) == 8) {
                    // fp64: the wave's 128 owned rows (8 M-blocks of 16) against the 16 winner rows
                    // and against themselves (their diagonal blocks), one v_mfma_f64_16x16x4f64 per
                    // M-block and k-chunk on the flush's operand rows in the flush's k order: per
                    // element the flush's own chain, bit for bit. A block stored transposed (the
                    // winner's tile row first) evolves as U_col·V_own: each k-chunk runs both
                    // products with the other one's winner column zeroed (it adds ±0). The chains
                    // start from the stored blocks (srow), handed from the owner threads to the MFMA
                    // lanes and back through LDS: sh_blk64 (winners) and sh_uhist[0] (diagonal
                    // blocks).
                    typedef double d64x2 __attribute__((ext_vector_type(2)));
                    typedef double d64x4 __attribute__((ext_vector_type(4)));
                    constexpr int KH = 8;   // doubles per lane and row block (kmax = 16)
                    const int l = tid & 63;
                    const int wb = tid & ~63;                          // the wave's first thread
                    const int rb0 = (2 * (g * SCAN_THREADS + wb)) >> 5;   // its first tile row (4 of them)
                    double4* dg = sh_uhist[0];   // (this wave's part: free until its first match)
                    if (own) {
#pragma unroll
                        for (int t = 0; t < SPEC_L; t++) sh_blk64[t][tid] = make_double4(srow[t][0], srow[t][1], srow[t][2], srow[t][3]);
                        dg[tid] = make_double4(srow[SPEC_L][0], srow[SPEC_L][1], srow[SPEC_L][2], srow[SPEC_L][3]);
                    } else {
#pragma unroll
                        for (int t = 0; t < SPEC_L; t++) sh_blk64[t][tid] = make_double4(0, 0, 0, 0);
                        dg[tid] = make_double4(0, 0, 0, 0);
                    }
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                    __builtin_amdgcn_wave_barrier();
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                    // this lane's winner column c = l % 16: row wr of winner t = c / 2 (B operands
                    // hold column l % 16 at k-offset l / 16, A operands row l % 16)
                    const int c = l & 15, t = c >> 1;
                    const int wsp = t < L ? sh_spec[t] : -1;
                    const int wr = wsp >= 0 ? 2 * wsp + (c & 1) : 0;
                    const size_t coff = (size_t)(wr >> 5) * 64 * KH + ((wr & 15) + 16 * (l >> 4)) * KH + ((wr >> 4) & 1) * 4;
                    auto comp = [](double4& v, int k) -> double& { return reinterpret_cast<double*>(&v)[k]; };
                    // two tile rows per pass, the pending steps inside: each step's operand loads of
                    // both row blocks are in flight together (a memory round trip per step and pair,
                    // not per step and tile row); per accumulator the same MFMA sequence
#pragma unroll 1
                    for (int r2 = 0; r2 < 4; r2 += 2) {
                        // (the last workgroup's waves may reach past the landmark block: no rows,
                        // no operand rows there)
                        if (rb0 + r2 >= d.nb) break;
                        const bool two = rb0 + r2 + 1 < d.nb;   // (uniform)
                        bool sw[2], nsw[2];
                        d64x4 acc[2][2], dac[2][2];
#pragma unroll
                        for (int x = 0; x < 2; x++) {
                            const int r4 = r2 + x, rb = rb0 + r4;
                            sw[x] = wsp >= 0 && rb > (wr >> 5);   // stored transposed
                            nsw[x] = wsp >= 0 && !sw[x];
#pragma unroll
                            for (int h = 0; h < 2; h++)
#pragma unroll
                                for (int i = 0; i < 4; i++) {
                                    const int rl = 32 * r4 + 16 * h + 4 * i + (l >> 4);   // row in the wave (tile_off_f64)
                                    const int ow = wb + (rl >> 1);
                                    acc[x][h][i] = comp(sh_blk64[t][ow], (rl & 1) * 2 + (c & 1));
                                    const int cl = 32 * r4 + 16 * h + c;
                                    dac[x][h][i] = (rl >> 1) == (cl >> 1) ? comp(dg[ow], (rl & 1) * 2 + (cl & 1)) : 0.0;
                                }
                        }
                        for (int q = 0; q < p.npend; q++) {
                            if (sh_ctl[q].y <= 0) continue;   // no match, or rolled back: nothing
                            const double* Uq = reinterpret_cast<const double*>(p.pend[q].Uop) + e * opstride;
                            const double* Vq = reinterpret_cast<const double*>(p.pend[q].Vop) + e * opstride;
                            d64x2 ua[2][4], va[2][4], cu[2], cv[2];
#pragma unroll
                            for (int x = 0; x < 2; x++) {
                                // (a second row block past the landmark block re-reads the first)
                                const int rb = rb0 + r2 + (two ? x : 0);
                                const d64x2* uo = reinterpret_cast<const d64x2*>(Uq + (size_t)rb * 64 * KH + l * KH);
                                const d64x2* vo = reinterpret_cast<const d64x2*>(Vq + (size_t)rb * 64 * KH + l * KH);
#pragma unroll
                                for (int k = 0; k < 4; k++) { ua[x][k] = uo[k]; va[x][k] = vo[k]; }
                            }
#pragma unroll
                            for (int k = 0; k < 2; k++) {
                                cu[k] = reinterpret_cast<const d64x2*>(Uq + coff)[k];
                                cv[k] = reinterpret_cast<const d64x2*>(Vq + coff)[k];
                            }
#pragma unroll
                            for (int x = 0; x < 2; x++)
#pragma unroll
                                for (int s4 = 0; s4 < 4; s4++) {
                                    const double bv = nsw[x] ? cv[s4 >> 1][s4 & 1] : 0.0;
                                    const double bu = sw[x] ? cu[s4 >> 1][s4 & 1] : 0.0;
#pragma unroll
                                    for (int h = 0; h < 2; h++) {
                                        const double au = ua[x][2 * h + (s4 >> 1)][s4 & 1];
                                        const double av = va[x][2 * h + (s4 >> 1)][s4 & 1];
                                        acc[x][h] = __builtin_amdgcn_mfma_f64_16x16x4f64(au, bv, acc[x][h], 0, 0, 0);
                                        acc[x][h] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bu, acc[x][h], 0, 0, 0);
                                        dac[x][h] = __builtin_amdgcn_mfma_f64_16x16x4f64(au, av, dac[x][h], 0, 0, 0);
                                    }
                                }
                        }
                        __builtin_amdgcn_wave_barrier();   // (every lane read its starting values)
#pragma unroll
                        for (int x = 0; x < 2; x++) {
                            if (x == 1 && !two) break;
                            const int r4 = r2 + x;
#pragma unroll
                            for (int h = 0; h < 2; h++)
#pragma unroll
                                for (int i = 0; i < 4; i++) {
                                    const int rl = 32 * r4 + 16 * h + 4 * i + (l >> 4);
                                    const int ow = wb + (rl >> 1);
                                    comp(sh_blk64[t][ow], (rl & 1) * 2 + (c & 1)) = acc[x][h][i];
                                    const int cl = 32 * r4 + 16 * h + c;
                                    if ((rl >> 1) == (cl >> 1)) comp(dg[ow], (rl & 1) * 2 + (cl & 1)) = dac[x][h][i];
                                }
                        }
                    }
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                    __builtin_amdgcn_wave_barrier();
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                    if (own && j < s) {
                        const double4 dd = dg[tid];
                        Dj[0] = dd.x; Dj[1] = dd.y; Dj[2] = dd.z; Dj[3] = dd.w;
                    }
                  }
                } else if (own) {
                    if (staged) {
                        double blk[SPEC_L + 1][4];
                        staged_blocks<T>(pv, j, cols, sh_stg, srow, blk);
#pragma unroll
                        for (int t = 0; t < SPEC_L; t++)
                            if (t < L && sh_spec[t] >= 0)
                                sh_blk[t][tid] = make_float4((float)blk[t][0], (float)blk[t][1], (float)blk[t][2], (float)blk[t][3]);
                        if (j < s) {
                            Dj[0] = blk[SPEC_L][0]; Dj[1] = blk[SPEC_L][1];
                            Dj[2] = blk[SPEC_L][2]; Dj[3] = blk[SPEC_L][3];
                        }
                    } else if constexpr (sizeof(typename Stor<T>::C) == 4) {
                        for (int t0 = 0; t0 < L; t0 += SPEC_PB) {
                            int cols[SPEC_PB];
                            double bk[SPEC_PB][4];
#pragma unroll
                            for (int b = 0; b < SPEC_PB; b++) {
                                const int w = (t0 + b < L) ? sh_spec[t0 + b] : -1;
                                cols[b] = 2 * (w >= 0 ? w : j);
                            }
                            pll_blocks<T, SPEC_PB>(pv, 2 * j, cols, bk);
#pragma unroll
                            for (int b = 0; b < SPEC_PB; b++)
                                if (t0 + b < L && sh_spec[t0 + b] >= 0)
                                    sh_blk[t0 + b][tid] = make_float4((float)bk[b][0], (float)bk[b][1], (float)bk[b][2], (float)bk[b][3]);
                        }
                    } else {
                        // fp64 operands: the same blocks in fp64, ahead of the line loop (they used
                        // to be read, pending steps replayed, inside it: a memory round trip per
                        // line on the landmark waves' chain)
                        for (int t0 = 0; t0 < L; t0 += SPEC_PB64) {
                            int cols[SPEC_PB64];
                            double bk[SPEC_PB64][4];
#pragma unroll
                            for (int b = 0; b < SPEC_PB64; b++) {
                                const int w = (t0 + b < L) ? sh_spec[t0 + b] : -1;
                                cols[b] = 2 * (w >= 0 ? w : j);
                            }
                            pll_blocks<T, SPEC_PB64>(pv, 2 * j, cols, bk);
#pragma unroll
                            for (int b = 0; b < SPEC_PB64; b++)
                                if (t0 + b < L && sh_spec[t0 + b] >= 0)
                                    sh_blk64[t0 + b][tid] = make_double4(bk[b][0], bk[b][1], bk[b][2], bk[b][3]);
                        }
                    }
                }
                EKF_STAMP(11);
                // ---- (g) the landmark waves: the sequential gating and gain rows against the
                // packages ----
                unsigned long long tq = dbg ? __builtin_amdgcn_s_memrealtime() : 0ull;
                auto sub = [&](int k) {
                    if (dbg) {
                        const unsigned long long t2 = __builtin_amdgcn_s_memrealtime();
                        sh_stamp[k] += t2 - tq;
                        tq = t2;
                    }
                };
                for (int i = 0; i < L && !viol; ++i) {
                    const ekf_line ln = sh_lines[i];
                    double Rm[4];
                    line_R(ln, i, r_mode, Rm);
                    const int w = __builtin_amdgcn_readfirstlane(sh_spec[i]);   // uniform: scalar branches, m scalar
                    int deep = 0;   // diagnostics: 1 past the quick filter, 2 past the fp32 one, 3 past the fp64 one
                    // the gate of line i on the state before it (the guessed winner itself, j == w, is
                    // evaluated exactly by the replay wave, which reports the result in the package
                    // (PK_OK) and its GSL_EDOM in sh_rwst; a failed winner leaves the line unmatched
                    // unless another landmark passes, which flags a violation). Its first filter runs in one block with the line's gain rows,
                    // which do not depend on it: two independent chains for the scheduler to interleave
                    const bool cand = own && j < s && !matched && j != w;
                    Block5 b5;
                    fill_block5(b5, R33, rr0, rr1, rr2, Dj);
                    const double ybx = yb.x, yby = yb.y;
                    const double xpg[3] = {xp[0], xp[1], xp[2]};
                    bool deeper = false;
                    const double* pk = nullptr;
                    bool wok = true;   // the guessed winner passed its exact gate (PK_OK)
                    if (w >= 0) {
                        int polls = 0;
                        while (__hip_atomic_load(&sh_ready, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) <= i) {
                            __builtin_amdgcn_s_sleep(1);
                            if ((tstatus & EKF_ST_TIMEOUT_BIT) || ++polls > (1 << p.spin_log2)) { tstatus |= EKF_ST_TIMEOUT_BIT; viol = 1; vline = i; break; }
                        }
                        sub(17);
                        pk = sh_pk[i];
                        wok = __builtin_amdgcn_readfirstlane(pk[PK_OK] != 0.0 ? 1 : 0) != 0;
                        if (r_mode == 1 && (i == 1 || i == 2) && wok) stp |= st_line(EKF_ST_NSYM, i);
                        if (own) {
                            // the quick filter and the gain rows in one block (independent chains);
                            // the gain rows take effect only if the guessed winner passed (wok,
                            // uniform; otherwise the package words are not written)
                            deeper = cand && !quick_reject(b5, ybx, yby, ma0, s0f, c0f, xpg, ln.alpha, ln.r, Rm, p.gate, ETA);
                            double blk[4];
                            if constexpr (sizeof(typename Stor<T>::C) == 4) {
                                const float4 bk = sh_blk[i][tid];
                                blk[0] = bk.x; blk[1] = bk.y; blk[2] = bk.z; blk[3] = bk.w;
                            } else {
                                const double4 bk = sh_blk64[i][tid];
                                blk[0] = bk.x; blk[1] = bk.y; blk[2] = bk.z; blk[3] = bk.w;
                            }
                            double kk[4], uu[4];
                            double2 g0 = rr0, g1 = rr1, g2 = rr2, gy = yb;
                            double gD[4] = {Dj[0], Dj[1], Dj[2], Dj[3]};
                            gain_rows<SPEC_L>(pk, m, [&](int q) { return sh_uhist[q][tid]; },   // m < SPEC_L = HIST_LDS
                                              [&](int q) { return sh_wh[i][q][1]; }, blk, g0, g1, g2, gy, gD, kk, uu);
                            if (wok) {
                                rr0 = g0; rr1 = g1; rr2 = g2; yb = gy;
                                Dj[0] = gD[0]; Dj[1] = gD[1]; Dj[2] = gD[2]; Dj[3] = gD[3];
                                float F[3];
                                sym_factor(pk, F);   // (the same bits as the replay wave's S gives)
                                store_rows(m, kk, uu, false, F, true);
                            }
                        }
                        sub(18);
                    } else {
                        deeper = cand && !quick_reject(b5, ybx, yby, ma0, s0f, c0f, xpg, ln.alpha, ln.r, Rm, p.gate, ETA);
                    }
                    if (deeper) {   // rare: the certified fp32 and fp64 filters, then the exact evaluation
                        deep = 1;
                        bool pass = false;
                        double sn = 0.0, cs = 1.0;
                        if (!certified_reject_f32(b5, ybx, yby, xpg, ln.alpha, ln.r, Rm, p.gate, ETA) &&
                            (deep = 2, exact_sc(), sincos_near(ybx, ma0, s0j, c0j, sn, cs),
                             !certified_reject(b5, ybx, yby, sn, cs, xpg, ln.alpha, ln.r, Rm, p.gate, ETA))) {
                            deep = 3;
                            Cand c;
                            eval_candidate(b5, ybx, yby, sn, cs, xpg, ln.alpha, ln.r, Rm, p.gate, ETA, c);
                            // GSL_EDOM counts only for candidates the reference evaluates: the
                            // unmatched ones up to the winner (Robot.cpp:313-498 stops there)
                            if (c.singular && (w < 0 || !wok || j <= w)) stp |= st_line(EKF_ST_SINGULAR, i);
                            if (c.amb && (w < 0 || !wok || j <= w)) stp |= st_line(EKF_ST_PRECISION_BIT, i);
                            pass = c.pass;
                        }
                        // the guess must be the first passing unmatched landmark; a guessed
                        // winner that failed leaves the line unmatched only if none passes
                        if (pass && (w < 0 || !wok || j < w)) {
                            viol = 1;
                            vline = i;
                        }
                    }
                    if (pdbg && g == 0) {   // waves of workgroup 0 whose lanes went deeper
                        const bool d1 = __any(deep >= 1), d2 = __any(deep >= 2), d3 = __any(deep >= 3);
                        if ((tid & 63) == 0) {
                            if (d1) atomicAdd(&sh_stamp[20], 1ull);
                            if (d2) atomicAdd(&sh_stamp[21], 1ull);
                            if (d3) atomicAdd(&sh_stamp[23], 1ull);
                            atomicAdd(&sh_stamp[22], 1ull);
                        }
                    }
                    sub(16);
                    if (w < 0 || !wok) {
                        // no match: the line goes to extraLines (Robot.cpp:308-310, 492-496)
                        if (w >= 0) dpath |= 32;   // diagnostics: a guessed winner failed, line unmatched
                        if (lead) {
                            res[RES_MATCH + i] = -1;
                            res[RES_EXTRA + nextra] = i;
                        }
                        if (tid == 0) sh_extra[nextra] = i;
                        nextra++;
                        continue;
                    }
                    // = robot_update(R33, xp, pk), computed by the replay wave
#pragma unroll
                    for (int a = 0; a < 9; a++) R33[a] = pk[PK_R33 + a];
                    xp[0] = pk[PK_XP + 0]; xp[1] = pk[PK_XP + 1]; xp[2] = pk[PK_XP + 2];
                    sub(19);
                    if (j == w) matched = true;
                    if (lead) res[RES_MATCH + i] = w;
                    m++;
                    if (stage_ops && own && m == 4) {
                        store_ops_half(0, m);
                        ops_early = 1;
                    }
                }
            }
            if (dbg) sh_stamp[31] += __builtin_amdgcn_s_memrealtime() - sh_trec;   // landmark wave 0 done
            __syncthreads();
            if (sh_flag) vline = 0;
            const int rwp = sh_rwst;
            EKF_STAMP(14);
            // ---- (h) verdict (exchange 3, parity 0): the first violating line over the workgroups
            // (payload line + 1, 0: none); a violation restarts on the sequential path from there ----
            const int wv = wave_min(tid < SCAN_THREADS ? vline : L);
            __syncthreads();
            if ((tid & 63) == 0 && tid < SCAN_THREADS) sh_red[tid >> 6] = wv;
            __syncthreads();
            int first = L;
#pragma unroll
            for (int w = 0; w < SCAN_THREADS / 64; w++) first = min(first, sh_red[w]);
            if (G > 1) {
                if (tid == 0) mb_tag(mbox + (size_t)g * p.mbw, p.epoch, TAG_SPEC_VERDICT, (unsigned)(first < L ? first + 1 : 0));
                if (tid < G) {
                    int v = mb_poll(mbox, 0, G, tid, p.mbw, p.epoch, TAG_SPEC_VERDICT, tstatus, p.spin_log2);
                    if (p.test_verdict == e + 1 && g == 1 && tid == 0) {   // test hook: this poll timed out
                        tstatus |= EKF_ST_TIMEOUT_BIT;
                        v = -1;
                    }
                    sh_best[tid] = v > 0 ? v - 1 : L;
                    if (v < 0) sh_vto = 1;
                }
                __syncthreads();
                for (int k = 0; k < G; k++) first = min(first, sh_best[k]);
                if (sh_vto) {
                    // a verdict that never arrived: this workgroup does not restart (its peers
                    // may have committed their halves already); it finishes with the timeout bit
                    // in its completion word, and the lead, which collects every word, rolls the
                    // instance's call back
                    tstatus |= EKF_ST_TIMEOUT_BIT;
                    first = L;
                }
            }
            EKF_STAMP(6);
            if (first >= L) {
                status |= st_lines(stp, L) | st_lines(rwp, L);
            } else {
                dpath |= (first > 0 ? 8 | 512 : 8) | (first << 10);   // (512: lines kept; bits 10..12 the line)
                if (dbg) sh_stamp[15] += 1;
                sequential = true;
                keep = first;
                // the first kept line's exchange on parity 1: the verdict tags (parity 0) may still
                // be polled until every workgroup has passed it
                par0 = (first + 1) & 1;
                init_state();
                Dj[0] = Dj[1] = Dj[2] = Dj[3] = 0.0;
                if (own && j < s) {
                    if (mf && p.npend > 0) {
                        // the diagonal block the speculative pass started from (Dd, exact), which
                        // the kept lines' packages were computed against
                        const double4 b = Ddr[j];
                        Dj[0] = b.x; Dj[1] = b.y; Dj[2] = b.z; Dj[3] = b.w;
                    } else {
                        pll_block(pv, 2 * j, 2 * j, Dj);
                    }
                }
                // fp32 operands: out of sh_blk, which aliases the V history the restart writes, into
                // the stage (free once the speculative pass is over); fp64: sh_blk64 as it is
                if constexpr (!kB64)
                    if (own)
#pragma unroll
                        for (int t = 0; t < SPEC_L; t++)
                            if (t < L && sh_spec[t] >= 0) sh_cblk[t][tid] = sh_blk[t][tid];
                blk_cached = true;
                matched = false;
                m = nextra = 0;
                status = st_lines(stp, first) | st_lines(rwp, first);
                dsq = 0.0;
                ops_early = 0;   // (the sequential path rewrites every operand row)
                __syncthreads();   // sh_extra, sh_vhist reuse
            }
        } else {
            par0 = 1;   // the lists' parity-0 words may still be read
            // unresolved guesses: straight to the sequential path, which needs the exact owned
            // diagonal block (the staged path only loaded the last flushed one, for the guess)
            if ((staged || m64) && own && j < s) pll_block(pv, 2 * j, 2 * j, Dj);
        }
    }

    for (int i = 0; sequential && i < L; ++i) {
        if (i < keep) {
            // a kept line (restart): its guessed winner and package, verified by the verdict
            const int w = __builtin_amdgcn_readfirstlane(sh_spec[i]);
            const double* pk = sh_pk[i];
            if (w < 0 || __builtin_amdgcn_readfirstlane(pk[PK_OK] != 0.0 ? 1 : 0) == 0) {
                if (lead) {
                    res[RES_MATCH + i] = -1;
                    res[RES_EXTRA + nextra] = i;
                }
                if (tid == 0) sh_extra[nextra] = i;
                nextra++;
                continue;
            }
            if (own) {
                // the owned block of column w: the speculative pass's (scan start, pending steps
                // applied), as the sequential lines take it (owned_block, blk_cached)
                double blk[4];
                if constexpr (kB64) {
                    const double4 b = sh_blk64[i][tid];
                    blk[0] = b.x; blk[1] = b.y; blk[2] = b.z; blk[3] = b.w;
                } else {
                    const float4 b = sh_cblk[i][tid];
                    blk[0] = b.x; blk[1] = b.y; blk[2] = b.z; blk[3] = b.w;
                }
                double kk[4], uu[4];
                gain_rows<0>(pk, m, uq_owned, [&](int q) { return sh_wh[i][q][1]; }, blk, rr0, rr1, rr2, yb, Dj, kk, uu);
                float F[3] = {0.f, 0.f, 0.f};
                if (sym) sym_factor(pk, F);
                store_rows(m, kk, uu, true, F, true);
            }
            // = robot_update(R33, xp, pk), computed by the replay wave
#pragma unroll
            for (int a = 0; a < 9; a++) R33[a] = pk[PK_R33 + a];
            xp[0] = pk[PK_XP + 0]; xp[1] = pk[PK_XP + 1]; xp[2] = pk[PK_XP + 2];
            if (j == w) matched = true;
            if (lead) res[RES_MATCH + i] = w;
            m++;
            continue;
        }
        const ekf_line ln = sh_lines[i];
        double Rm[4];
        line_R(ln, i, r_mode, Rm);
        // gating of the owned candidate (Robot.cpp:313-498); the first passing unmatched j wins
        int best = 0x7fffffff;
        bool sing = false, amb = false;
        Cand c;
        if (own && j < s && !matched) {
            Block5 b5;
            fill_block5(b5, R33, rr0, rr1, rr2, Dj);
            double sn, cs;
            if (!quick_reject(b5, yb.x, yb.y, ma0, s0f, c0f, xp, ln.alpha, ln.r, Rm, p.gate, ETA) &&
                (exact_sc(), sincos_near(yb.x, ma0, s0j, c0j, sn, cs),
                 !certified_reject(b5, yb.x, yb.y, sn, cs, xp, ln.alpha, ln.r, Rm, p.gate, ETA))) {
                eval_candidate(b5, yb.x, yb.y, sn, cs, xp, ln.alpha, ln.r, Rm, p.gate, ETA, c);
                sing = c.singular;
                amb = c.amb;
                if (c.pass) best = j;
            }
        }
        EKF_STAMP(2);
        const int wbest = wave_min(best);
        if ((tid & 63) == 0 && tid < SCAN_THREADS) sh_red[tid >> 6] = wbest;
        __syncthreads();
        int gbest = sh_red[0];
#pragma unroll
        for (int w = 1; w < SCAN_THREADS / 64; w++) gbest = min(gbest, sh_red[w]);
        const int par = (i + par0) & 1;
        double* slot = mbox + ((size_t)par * G + g) * p.mbw;
        const int npk = MB_VH + 4 * m;
        if (best != 0x7fffffff && best == gbest) {
            // this workgroup's candidate: the uniform gain package and the V rows of the
            // candidate for the earlier matches of this scan (Robot.cpp:560-568 corrections),
            // staged in LDS
            build_package(c, R33, rr0, rr1, rr2, sh_pkg);
            for (int q = 0; q < m; q++) {
                const double4 vq = q < HIST_V ? sh_vhist[q][tid]
                                                : *reinterpret_cast<const double4*>(Vst + ((size_t)q * n + b0) * 2);
                sh_pkg[MB_VH + 4 * q + 0] = vq.x;
                sh_pkg[MB_VH + 4 * q + 1] = vq.y;
                sh_pkg[MB_VH + 4 * q + 2] = vq.z;
                sh_pkg[MB_VH + 4 * q + 3] = vq.w;
            }
        }
        __syncthreads();   // the staged package
        int jstar = gbest, gstar = 0;
        if (G > 1) {
            // to the mailbox, one word per lane; drained and ordered by the barrier before the
            // tagged best word (payload best + 1, 0: no candidate); every workgroup polls all G
            if (gbest != 0x7fffffff)
                for (int k = 1 + tid; k < npk; k += SCAN_BLOCK) mb_store(slot + k, sh_pkg[k]);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (tid == 0) mb_tag(slot, p.epoch, (unsigned)(i + 1), (unsigned)(gbest == 0x7fffffff ? 0 : gbest + 1));
            EKF_STAMP(3);
            for (int k = tid; k < G; k += SCAN_BLOCK) {
                const int bq = mb_poll(mbox, par, G, k, p.mbw, p.epoch, (unsigned)(i + 1), tstatus, p.spin_log2);
                sh_best[k] = bq <= 0 ? 0x7fffffff : bq - 1;
            }
            __syncthreads();
            jstar = 0x7fffffff;
            for (int k = 0; k < G; k++) {
                const int v = sh_best[k];
                if (v < jstar) { jstar = v; gstar = k; }
            }
        } else {
            EKF_STAMP(3);   // one workgroup: the package never leaves LDS
        }
        EKF_STAMP(4);
        // GSL_EDOM counts only for the candidates the reference evaluates (up to the winner)
        if (sing && j <= jstar) status |= EKF_ST_SINGULAR;
        if (amb && j <= jstar) status |= EKF_ST_PRECISION_BIT;
        if (jstar == 0x7fffffff) {
            // no match (or s == 0): the line goes to extraLines (Robot.cpp:308-310, 492-496)
            if (lead) {
                res[RES_MATCH + i] = -1;
                res[RES_EXTRA + nextra] = i;
            }
            if (tid == 0) sh_extra[nextra] = i;
            nextra++;
            continue;
        }
        // ---- match (Robot.cpp:500-641) ----
        // the winner's package and this thread's block of column jstar are independent: issue both
        // loads before waiting on either (another workgroup's winner: every workgroup reloads, its
        // own staged candidate included)
        double blk[4] = {0.0, 0.0, 0.0, 0.0};
        int tsc = -1;   // the winner's guess index, when its blocks are cached (blk_cached)
        if (blk_cached)
#pragma unroll
            for (int t = 0; t < SPEC_L; t++)
                if (t < L && sh_spec[t] == jstar) tsc = t;
        auto owned_block = [&]() {
            if (tsc >= 0) {
                if constexpr (kB64) {
                    const double4 b = sh_blk64[tsc][tid];
                    blk[0] = b.x; blk[1] = b.y; blk[2] = b.z; blk[3] = b.w;
                } else {
                    const float4 b = sh_cblk[tsc][tid];
                    blk[0] = b.x; blk[1] = b.y; blk[2] = b.z; blk[3] = b.w;
                }
            } else {
                pll_block(pv, 2 * j, 2 * jstar, blk);
            }
        };
        if (G > 1) {
            // (every thread passed the poll barrier after its mailbox stores read sh_pkg)
            const double* ps = mbox + ((size_t)par * G + gstar) * p.mbw;
            double pk0 = 0.0, pk1 = 0.0;
            if (tid < npk) pk0 = mb_load(ps + tid);
            if (tid + SCAN_BLOCK < npk) pk1 = mb_load(ps + tid + SCAN_BLOCK);
            if (own) owned_block();
            if (tid < npk) sh_pkg[tid] = pk0;
            if (tid + SCAN_BLOCK < npk) sh_pkg[tid + SCAN_BLOCK] = pk1;
            __syncthreads();
        } else if (own) {
            owned_block();
        }
        if (r_mode == 1 && (i == 1 || i == 2)) status |= EKF_ST_NSYM;
        if (own) {
            double kk[4], uu[4];
            gain_rows<0>(sh_pkg, m, uq_owned,
                         [&](int q) {
                             const double* vh = sh_pkg + MB_VH + 4 * q;
                             return make_double4(vh[0], vh[1], vh[2], vh[3]);
                         },
                         blk, rr0, rr1, rr2, yb, Dj, kk, uu);
            float F[3] = {0.f, 0.f, 0.f};
            if (sym) sym_factor(sh_pkg, F);
            store_rows(m, kk, uu, true, F, true);
        }
        robot_update(R33, xp, sh_pkg);
        if (j == jstar) matched = true;
        if (lead) res[RES_MATCH + i] = jstar;
        m++;
        EKF_STAMP(6);
    }
    status |= tstatus;

    // ---------------- commit (Robot.cpp:702-716) ----------------
    __syncthreads();   // sh_extra
    double pose[3] = {xp[0], xp[1], xp[2]};
    if (L == 0 || m == 0) pose[2] = normalize_radian(xp[2]);   // y[2] stays un-normalised
    const int nadd = min(nextra, N - s);
    const int reset = (s + nadd > N - p.reset_margin) ? 1 : 0;

    // ---------------- augmentation (Robot.cpp:776-866) ----------------
    double vnew = 0.0;   // the lead: the largest variance of the new landmarks (EKF_ARITH_F16X3's σ)
    if (!reset) {
        // the new landmarks' world-frame line and its sin/cos (Robot.cpp:787-803), lane q of every
        // wave for new landmark q (nadd <= max_lines <= 64), then read from that lane: one set of
        // fp64 trigonometry per wave instead of one per new landmark
        double a_r = 0.0, a_al = 0.0, a_sa = 0.0, a_ca = 1.0;
        {
            const int ql = threadIdx.x & 63;
            if (ql < nadd) {
                const ekf_line lq = sh_lines[sh_extra[ql]];
                double alfa = lq.alpha;
                a_r = lq.r + (pose[0] * cos(alfa) + pose[1] * sin(alfa));
                alfa += pose[2];
                sincos(alfa, &a_sa, &a_ca);
                a_al = alfa;
            }
        }
        for (int q = 0; q < nadd; q++) {
            const ekf_line ln = sh_lines[sh_extra[q]];
            const int sq = s + q;
            const double r = __shfl(a_r, q, 64);
            const double alfa = __shfl(a_al, q, 64);
            const double sa = __shfl(a_sa, q, 64), ca = __shfl(a_ca, q, 64);
            if (own && j < sq) {
                // landmark columns of P[l0:l0+2, 0:l0] = Gx·P[0:3, 0:l0] (Robot.cpp:852-862)
                double* prow = patch + (size_t)(q * 2) * M;
                *reinterpret_cast<double2*>(prow + 2 * j) = rr2;
                double2 gx;
                gx.x = ca * rr0.x + sa * rr1.x;
                gx.y = ca * rr0.y + sa * rr1.y;
                *reinterpret_cast<double2*>(prow + M + 2 * j) = gx;
            }
            if (j == sq) {
                // the new landmark: robot part of the same product (its robot-strip columns) and
                // its mean (Robot.cpp:801-803)
                rr0 = make_double2(R33[6], ca * R33[0] + sa * R33[3]);
                rr1 = make_double2(R33[7], ca * R33[1] + sa * R33[4]);
                rr2 = make_double2(R33[8], ca * R33[2] + sa * R33[5]);
                yb = make_double2(normalize_radian(alfa), r);
            }
            if (lead || j == sq) {
                // P_ll = Gx·Prr·Gxᵀ + Gl·R·Glᵀ (Robot.cpp:813-847); Gx = [[0,0,1],[ca,sa,0]],
                // Gl = [[1,0],[y1·ca − y0·sa, 1]]
                const double Gx[6] = {0, 0, 1, ca, sa, 0};
                const double Gl[4] = {1.0, 0, xp[1] * ca - xp[0] * sa, 1};
                double GP[6], GlR[4];
                for (int a = 0; a < 2; a++)
                    for (int b = 0; b < 3; b++) {
                        double acc = 0.0;
                        for (int k = 0; k < 3; k++) acc += Gx[a * 3 + k] * R33[k * 3 + b];
                        GP[a * 3 + b] = acc;
                    }
                for (int a = 0; a < 2; a++)
                    for (int b = 0; b < 2; b++)
                        GlR[a * 2 + b] = Gl[a * 2 + 0] * ln.R[0 * 2 + b] + Gl[a * 2 + 1] * ln.R[1 * 2 + b];
                for (int a = 0; a < 2; a++)
                    for (int b = 0; b < 2; b++) {
                        double gsum = 0.0;
                        for (int k = 0; k < 3; k++) gsum += GP[a * 3 + k] * Gx[b * 3 + k];
                        const double h = GlR[a * 2 + 0] * Gl[b * 2 + 0] + GlR[a * 2 + 1] * Gl[b * 2 + 1];
                        if (j == sq) Dj[a * 2 + b] = gsum + h;   // the new landmark's kept diagonal block
                        if (!lead) continue;
                        pdiag[q * 4 + a * 2 + b] = gsum + h;
                        if (a == b) vnew = fmax(vnew, gsum + h);
                        // fp16 storage: the new landmark's variances bound its whole row and
                        // column (|P_ij| <= sqrt(P_ii P_jj)), and downdates only shrink them
                        if (Stor<T>::half && fabs(ldexp(gsum + h, pv.ex)) > F16_RANGE_WARN)
                            status |= EKF_ST_RANGE_BIT;
                        // fp32 storage: within 2^8 of fp32's range (a diverged filter; SURVEY §8d's
                        // world reaches P ≈ 1e43 after 200 scans)
                        if (sizeof(typename Stor<T>::C) == 4 && !Stor<T>::half && !(fabs(gsum + h) <= F32_RANGE_WARN))
                            status |= EKF_ST_RANGE_BIT;
                    }
            }
        }
    }
    EKF_STAMP(27);
    // fp32 storage: an update that cancels more than 4 of fp32's 24 significant bits of a
    // landmark's variance (trace before / after > PREC_CANCEL = 2^4: the result no longer
    // guaranteed to 2^-20, the P bar), or leaves it non-positive, is flagged EKF_ST_PRECISION; the
    // result still commits (a diverging filter: SURVEY §8d's world)
    if constexpr (sizeof(C) == 4 && !Stor<T>::half)
        if (own && !reset && j < s && dsq > 0.0) {
            const double ta = Dj[0] + Dj[3];
            if (!(ta > 0.0) || ta + dsq > PREC_CANCEL * ta) status |= EKF_ST_PRECISION_BIT;
        }
    // EKF_ARITH_F16X3: an active landmark whose variance sits below the planes' dynamic range at
    // this scan's σ (a filter whose largest variance is ≥ 2^28 times its smallest: SURVEY §8d's
    // world in steady state) makes the step's flush exact (PLANE_SIGMA_EXACT, DONE_PLOSS)
    if (pf16 && own && !reset && j < s + nadd && ldexp(fmin(Dj[0], Dj[3]), 2 * psig) < PLANE_VAR_MIN)
        status |= (int)DONE_PLOSS;
    // write back the owned state (reset: Robot.cpp:893-904 zeroes landmark entries of y and P)
    if (own) {
        if (reset) {
            rr0 = rr1 = rr2 = yb = make_double2(0.0, 0.0);
        }
        *reinterpret_cast<double2*>(Rsw + b0) = rr0;
        *reinterpret_cast<double2*>(Rsw + n + b0) = rr1;
        *reinterpret_cast<double2*>(Rsw + 2 * n + b0) = rr2;
        *reinterpret_cast<double2*>(yw + b0) = yb;
        if (Ddw) Ddw[j] = reset || j >= s + nadd ? make_double4(0, 0, 0, 0) : make_double4(Dj[0], Dj[1], Dj[2], Dj[3]);
    }
    EKF_STAMP(28);
    if (own) {
        if (stage_ops) {
            if (!ops_early) store_ops_half(0, m);
            store_ops_half(1, m);
        } else if (sizeof(C) == 4) {
            // f32 operands: the k columns past the matches hold −0 (U) and +0 (V), so a flush
            // that runs every k-step unconditionally adds −0 there, which leaves every value as
            // it is (flush_f32_wave_kernel; the other forms and the on-read replay stop at ks)
            for (int k = 2 * m; k < d.kmax; k++)
#pragma unroll
                for (int pp = 0; pp < 2; pp++) {
                    if (!p.usym) Uop[op_index_f32(2 * j + pp, k, d.kmax)] = (C)(-0.0f);
                    Vop[op_index_f32(2 * j + pp, k, d.kmax)] = (C)0.0f;
                }
        }
        if (sizeof(C) == 8) {
            // f64 operands: the same −0 (U) / +0 (V) padding past the matches, so that the f64
            // wave flush may run every k-step (flush_f64_wave_kernel) while downdate_f64_kernel
            // and the on-read replay stop at the last 4-wide k-step holding a match
            for (int k = 2 * m; k < d.kmax; k++)
#pragma unroll
                for (int pp = 0; pp < 2; pp++) {
                    Uop[op_index_f64(2 * j + pp, k, d.kmax)] = (C)(-0.0);
                    Vop[op_index_f64(2 * j + pp, k, d.kmax)] = (C)0.0;
                }
        }
    }
    EKF_STAMP(24);
    // status bits seen by this workgroup's threads → its status word (read by ekf_read_results)
    int wgst = 0;
    {
        int st = status;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) st |= __shfl_xor(st, off, 64);
        __shared__ int sh_m;
        if (tid == 0) sh_m = m;   // the matches, as a landmark wave counted them
        __syncthreads();
        if constexpr (kPlanes)
            if (Bop && own) {
                // the owned rows' planes: per row and k parity h (k = 2s + h, s = 0..7) one
                // 16-byte lane row per part; k past the matches +0 (stored early, as the U and V
                // halves are, their split arithmetic lands on the per-line chain: scan +0.8 µs)
                const int m = sh_m;
                typedef unsigned u32x4v __attribute__((ext_vector_type(4)));
#pragma unroll
                for (int pp = 0; pp < 2; pp++) {
                    const f32x4v* src = reinterpret_cast<const f32x4v*>(sh_vpl + tid * 32 + pp * 16);
                    float v[16];
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        const f32x4v x = src[i];
#pragma unroll
                        for (int u = 0; u < 4; u++) v[4 * i + u] = (4 * i + u) < 2 * m ? x[u] : 0.f;
                    }
#pragma unroll
                    for (int h = 0; h < 2; h++) {
                        if (HOT == 2 || (HOT == 0 && pf16)) {   // EKF_ARITH_F16X3: hi, lo of 2^σ·V
                            unsigned w[2][4];
#pragma unroll
                            for (int q = 0; q < 4; q++) {
                                unsigned o[2];
                                split_pack_f16(v[4 * q + h], v[4 * q + 2 + h], psig, o);
                                w[0][q] = o[0];
                                w[1][q] = o[1];
                            }
#pragma unroll
                            for (int pl = 0; pl < 2; pl++)
                                *reinterpret_cast<u32x4v*>(Bop + op_index_pl(2 * j + pp, h, pl, 2)) =
                                    u32x4v{w[pl][0], w[pl][1], w[pl][2], w[pl][3]};
                        }
                        if (HOT == 1 || (HOT == 0 && !pf16)) {   // EKF_ARITH_BF16X6: hi, mid, lo
                            unsigned w[3][4];
#pragma unroll
                            for (int q = 0; q < 4; q++) {
                                unsigned o[3];
                                split_pack(v[4 * q + h], v[4 * q + 2 + h], o);
#pragma unroll
                                for (int pl = 0; pl < 3; pl++) w[pl][q] = o[pl];
                            }
#pragma unroll
                            for (int pl = 0; pl < 3; pl++)
                                *reinterpret_cast<u32x4v*>(Bop + op_index_bf(2 * j + pp, h, pl)) =
                                    u32x4v{w[pl][0], w[pl][1], w[pl][2], w[pl][3]};
                        }
                    }
                }
            }
        if (__ballot(nzr) != 0ull) st |= (int)DONE_NZ;
        if ((tid & 63) == 0 && tid < SCAN_THREADS) sh_red[tid >> 6] = st;
        __syncthreads();
#pragma unroll
        for (int w = 0; w < SCAN_THREADS / 64; w++) wgst |= sh_red[w];
    }
    // completion (rollback protocol, publish_done / lead_collect): the lead commits the launch —
    // flips the instance to the copy of the robot strip and mean written above, writes the shared
    // state and the step's result record — only if every workgroup completed without a timeout.
    // Otherwise the instance keeps its state from before the call, and the step's record applies
    // nothing (no downdate, rows or reset: the flush and later on-read replays skip it).
    // The lead collects on the speculative path too: a workgroup's own verdict poll can time out
    // while the lead's succeeds (the two polls race the spin bound), and that workgroup then
    // finishes with the timeout bit (above); only its completion word tells the lead.
    EKF_STAMP(25);
    if (tid == 0 && g != 0) publish_done(sync, g, p.epoch, wgst);
    int zg = (wgst & (int)DONE_NZ) ? 1 : 0;
    if (g == 0 && (sequential || G > 1)) wgst = lead_collect<SCAN_BLOCK>(sync, G, p.epoch, wgst, p.spin_log2, tid, sh_red, zg);
    const bool ploss = (wgst & (int)DONE_PLOSS) != 0;
    wgst &= ~(int)(DONE_NZ | DONE_PLOSS);
    EKF_STAMP(26);
    if (lead) {
        sync[SYNC_WG0] = (int)done_word(p.epoch, wgst);
        const bool commit = !(wgst & EKF_ST_TIMEOUT_BIT);
        res[RES_NLINES] = L;
        res[RES_SAVED_IN] = s;
        res[RES_DBG] = dpath | rpath | (sequential ? 16 : 0);
        for (int t = 0; t < 5; t++) res[RES_DBG + 1 + t] = t < SPEC_L ? sh_spec[t] : -2;
        if (commit) {
            yw[0] = xp[0];
            yw[1] = xp[1];
            yw[2] = xp[2];
            for (int a = 0; a < 9; a++) Rsw[(a / 3) * n + (a % 3)] = R33[a];
            p.pose[3 * e + 0] = pose[0];
            p.pose[3 * e + 1] = pose[1];
            p.pose[3 * e + 2] = pose[2];
            res[RES_STATUS] = ((nextra > nadd) ? EKF_ST_CAP : 0);
            res[RES_M] = m;
            res[RES_NEXTRA] = nextra;
            res[RES_SAVED] = reset ? 0 : s + nadd;
            res[RES_RESET] = reset;
            res[RES_NADD] = reset ? 0 : nadd;
            res[RES_KSTEPS] = (sizeof(C) == 4) ? m : (m + 1) / 2;
            res[RES_ROLLBACK] = 0;
            res[RES_PSIG] = ploss ? PLANE_SIGMA_EXACT : psig;
            // nonzero operand rows only below zg workgroups' landmarks; new rows below s + nadd
            res[RES_ZMAX] = max(min(zg * SCAN_THREADS, N), reset ? 0 : s + nadd);
            if (p.res_host) {
                // the synchronous call's result without a copy: the words ekf_result takes (the
                // status with every workgroup's bits, as the host's fold of the completion words
                // would give: the lead collected them), the pose and the robot block, then the
                // epoch. A rollback writes none of it (the host then reads the device copies)
                int* rh = p.res_host + (size_t)e * RES_STRIDE;
                rh[RES_NLINES] = L;
                rh[RES_STATUS] = res[RES_STATUS] | (wgst & DONE_STATUS_MASK);
                rh[RES_M] = m;
                rh[RES_NEXTRA] = nextra;
                rh[RES_SAVED] = reset ? 0 : s + nadd;
                rh[RES_RESET] = reset;
                for (int i = 0; i < L; i++) rh[RES_MATCH + i] = res[RES_MATCH + i];
                p.pose_host[3 * e + 0] = pose[0];
                p.pose_host[3 * e + 1] = pose[1];
                p.pose_host[3 * e + 2] = pose[2];
                for (int a = 0; a < 9; a++) p.r33_host[9 * e + a] = R33[a];
                __threadfence_system();
                __hip_atomic_store(p.ep_host + e, p.epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
            }
            p.saved[e] = reset ? 0 : s + nadd;
            p.live[e] = 1 - cb;
            if (pf16) {
                // the plane exponent of the later steps: |V_ik| <= sqrt(P_ii) <= sqrt(vmax), and
                // |2^σ·V| <= 2^12 at σ = plane_sigma(vmax). A larger vmax waits for the next group
                // (the first scan of a group recomputes σ) while |2^σ·V| stays <= 2^15 (fp16's
                // range is 2^16): σ at most 3 above plane_sigma(vmax)
                if (reset) {
                    p.pvmax[e] = 0.0;
                    p.psig[e] = PLANE_SIGMA_EMPTY;
                } else {
                    const double vm = fmax(p.pvmax[e], vnew);
                    const int target = plane_sigma(vm);
                    p.pvmax[e] = vm;
                    p.psig[e] = target < psig - 3 ? target : psig;
                }
            }
        } else {
            res[RES_STATUS] = 0;
            res[RES_M] = 0;
            res[RES_NEXTRA] = 0;
            res[RES_SAVED] = s;
            res[RES_RESET] = 0;
            res[RES_NADD] = 0;
            res[RES_KSTEPS] = 0;
            res[RES_ROLLBACK] = 1;
            res[RES_ZMAX] = 0;
            for (int i = 0; i < L; i++) res[RES_MATCH + i] = -1;
        }
    }
    EKF_STAMP(7);
    if (dbg) {
        // (phase times accumulate in LDS: a global read-modify-write per stamp would add a
        // memory round trip to every phase it measures)
        for (int k = 0; k < EKF_NSTAMP; k++) dbg[k] += sh_stamp[k];
        dbg[8] += t_last - t_first;
        dbg[9] += 1;
    }
}

}  // namespace ekf
