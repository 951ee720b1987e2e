// ekf_assoc_parts.h — the parts of the association that scan_kernel (ekf_kernels.hip) and the kernels
// of an instance partitioned over ranks (ekf_shard_kernels.h) share, one definition each, so that a
// partitioned scan is bit-identical to a single-context one: the certified reject filters of the gate,
// the mailbox through which cooperating workgroups exchange words, and the gain chain of a match (the
// package, a landmark's rows, the robot update). The exact evaluation of a candidate is ekf_gate.h.
#pragma once

#include "ekf_device.h"
#include "ekf_gate.h"

// The association arithmetic contracts a·b + c only within one source expression, so a
// function inlined into different kernels or phases rounds identically everywhere (the
// speculative and sequential association paths must agree bit for bit).
#pragma clang fp contract(on)

namespace ekf {

// sin/cos of a landmark angle from those of its value at the start of the scan: the angle
// moves by small Kalman corrections within a scan, so sin/cos(ma0 + δ) by the addition formula
// with Taylor series in δ (|δ| <= 1/64: truncation below 1e-19), and the full fp64 sincos
// otherwise. Every path that evaluates a candidate uses this form, so they agree bit for bit.
__device__ __forceinline__ void sincos_near(double ma, double ma0, double s0, double c0, double& sn,
                                            double& cs)
{
    const double dl = ma - ma0;
    if (fabs(dl) <= 0.0009765625) {
        // |δ| <= 2^-10: sin δ = δ − δ³/6 (next term ≤ 8e-18), 1 − cos δ = δ²/2 − δ⁴/24 (≤ 2e-21)
        const double d2 = dl * dl;
        const double sd = dl * (1.0 - d2 * (1.0 / 6.0));
        const double cm = d2 * 0.5 * (1.0 - d2 * (1.0 / 12.0));
        sn = s0 - (s0 * cm - c0 * sd);
        cs = c0 - (c0 * cm + s0 * sd);
    } else if (fabs(dl) <= 0.015625) {
        const double d2 = dl * dl;
        const double sd = dl * (1.0 - d2 * (1.0 / 6.0) * (1.0 - d2 * (1.0 / 20.0) * (1.0 - d2 * (1.0 / 42.0))));
        const double cm = d2 * 0.5 * (1.0 - d2 * (1.0 / 12.0) * (1.0 - d2 * (1.0 / 30.0) * (1.0 - d2 * (1.0 / 56.0))));
        sn = s0 - (s0 * cm - c0 * sd);   // s0·cos δ + c0·sin δ, cos δ = 1 − cm
        cs = c0 - (c0 * cm + s0 * sd);   // c0·cos δ − s0·sin δ
    } else {
        sincos(ma, &sn, &cs);
    }
}

// Certified rejection: true only if the exact evaluation is guaranteed to fail the gate. It
// accepts sin/cos with |error| <= EPS (here the exact ones of sincos_near);
// the resulting error in S and v is bounded explicitly and d² = q/det is bounded from below by
// interval arithmetic. Requires a symmetric R and a determinant that is not tiny relative to
// |S00·S11| + |S01·S10| (so that the reference's LU-based d² is within 1e-9 of q/det).
__device__ __forceinline__ bool certified_reject(const Block5& b, double ma, double mr, double sn,
                                                 double cs, const double xp[3], double za, double zr,
                                                 const double Rm[4], double gate, double eta)
{
    if (!(fabs(ma) <= 8.0) || Rm[1] != Rm[2]) return false;
    const double EPS = 1e-5;
    const double h10 = -cs, h11 = -sn, h1l = xp[0] * sn - xp[1] * cs;
    double S[4], hp0[5], hp1[5];
    innovation_cov(b, h10, h11, h1l, Rm, S, hp0, hp1);
    const double v0 = innovation_angle(za, ma, xp[2]);
    const double v1 = zr - (mr - (xp[0] * cs + xp[1] * sn));
    const double ex = EPS * (fabs(xp[0]) + fabs(xp[1]));
    double Pm = fmax(fmax(fmax(fabs(b.p00), fabs(b.p01)), fmax(fabs(b.p02), fabs(b.p10))),
                     fmax(fmax(fabs(b.p11), fabs(b.p12)), fmax(fabs(b.p20), fabs(b.p21))));
    Pm = fmax(Pm, fmax(fmax(fmax(fabs(b.p22), fabs(b.p0a)), fmax(fabs(b.p1a), fabs(b.p2a))),
                       fmax(fmax(fabs(b.p0b), fabs(b.p1b)), fabs(b.p2b))));
    Pm = fmax(Pm, fmax(fmax(fabs(b.daa), fabs(b.dab)), fmax(fabs(b.dba), fabs(b.dbb))));
    const double dh = (2.0 * EPS + ex) * Pm;                   // |Δ hp1[b]|
    // + the storage precision of the gate (gate_eta)
    const double m0 = eta * 2.0 * (fabs(b.p22) + fabs(b.daa));
    const double m1 = eta * (2.0 + (fabs(h1l) + ex) * (fabs(h1l) + ex)) *
                      (fabs(b.p00) + fabs(b.p11) + fabs(b.p22) + fabs(b.daa) + fabs(b.dbb));
    const double dS00 = m0;
    const double dS01 = EPS * (fabs(hp0[0]) + fabs(hp0[1])) + ex * fabs(hp0[3]) + 0.5 * (m0 + m1);
    const double dS10 = 2.0 * dh + 0.5 * (m0 + m1);
    const double dS11 = dh * (3.0 + fabs(h1l) + ex) + EPS * (fabs(hp1[0]) + fabs(hp1[1])) +
                        ex * fabs(hp1[3]) + m1;
    const double dv1 = ex;
    const double q = v0 * v0 * S[3] - v0 * v1 * (S[1] + S[2]) + v1 * v1 * S[0];
    const double det = S[0] * S[3] - S[1] * S[2];
    const double mag_det = fabs(S[0] * S[3]) + fabs(S[1] * S[2]);
    const double mag_q = v0 * v0 * fabs(S[3]) + fabs(v0 * v1) * (fabs(S[1]) + fabs(S[2])) +
                         v1 * v1 * fabs(S[0]);
    const double av1 = fabs(v1) + dv1;
    const double dq = v0 * v0 * dS11 + fabs(v0) * av1 * (dS01 + dS10) +
                      fabs(v0) * dv1 * fabs(S[1] + S[2]) +
                      (2.0 * fabs(v1) * dv1 + dv1 * dv1) * fabs(S[0]) + av1 * av1 * dS00 + 1e-9 * mag_q;
    const double ddet = fabs(S[0]) * dS11 + fabs(S[3]) * dS00 + fabs(S[1]) * dS10 + fabs(S[2]) * dS01 +
                        dS01 * dS10 + dS00 * dS11 + 1e-9 * mag_det;
    const double det_lo = det - ddet;
    if (!(det_lo > 1e-6 * mag_det)) return false;              // also false for NaN / Inf
    return (q - dq) > gate * gate * (1.0 + 1e-6) * (det + ddet);
}

// Certified cheap rejection (the first filter of the per-line gate: ≈35 fp64 operations, no
// trigonometry). For a symmetric positive definite S, vᵀS⁻¹v ≥ v0²/S00 and vᵀS⁻¹v ≥ v1²/S11, so
// the exact evaluation fails the gate (Robot.cpp:489) if either one-dimensional bound exceeds it:
//  * S00 = H0·P5·H0ᵀ + R00 with the constant row H0 = (0, 0, −1, 1, 0): p22 − 2·p2a + daa + R00
//    (innovation_cov's S[0]); the reference's normalizeRadian (Robot.cpp:62-71) and the 2π fold
//    (:465-475) shift za − (ma − x_pre2) by multiples of 2π only, so |v0| ≥ its circular distance
//    to 0;
//  * S11 = H1·P5·H1ᵀ + R11 ≤ ‖H1‖²·tr(P5) + R11 with ‖H1‖² = 2 + h1l² ≤ 2 + (|x0| + |x1|)² (P5,
//    a principal block of a covariance, is positive semidefinite); v1 = zr − (mr − (x0·cos ma +
//    x1·sin ma)) bounded from below with the scan-start sin/cos of ma0 (|Δcos|, |Δsin| ≤ |ma − ma0|).
// It needs R symmetric with R00, R11 large against the storage rounding of P5 (which could
// otherwise make S indefinite: then it never rejects) and finite inputs (NaN never rejects).
// Margins: 1e-6 relative on the gate plus absolute slack, far above the rounding of the bounds
// and of the exact evaluation.
// s0, c0: sin/cos of ma0 within QR_TRIG_EPS (the fp32 __sincosf of (float)ma0 for |ma0| <= 8:
// argument rounding <= 8·2^-24 plus the instruction's own error, ≈1e-6 together).
constexpr double QR_TRIG_EPS = 4e-6;
__device__ __forceinline__ bool quick_reject(const Block5& b, double ma, double mr, double ma0, double s0,
                                             double c0, const double xp[3], double za, double zr,
                                             const double Rm[4], double gate, double eta)
{
    // every bound evaluated, the tests combined without branches (bitwise on bools): the same
    // values as the early-exit form, fewer exec-mask instructions on the per-line chain
    const double tr5 = b.p00 + b.p11 + b.p22 + b.daa + b.dbb;
    const double X = fabs(xp[0]) + fabs(xp[1]);
    const double H2 = 2.0 + X * X;   // ≥ ‖H1‖²
    const bool ok = (Rm[1] == Rm[2]) & (tr5 >= 0.0) & (Rm[0] > 1e-5 * 2.0 * tr5) & (Rm[3] > 1e-5 * H2 * tr5) &
                    (fabs(ma0) <= 8.0);
    const double g2 = gate * gate * (1.0 + 1e-6);
    // S00 + its storage precision (gate_eta): |Δ(p22 − 2·p2a + daa)| <= 2·eta·(|p22| + |daa|)
    const double S00 = b.p22 - 2.0 * b.p2a + b.daa + Rm[0] + 2.0 * eta * (fabs(b.p22) + fabs(b.daa));
    const double x = za - (ma - xp[2]);
    const double cd = fabs(x - 2.0 * EKF_PI * rint(x * (0.5 / EKF_PI)));
    const double a0 = cd - 1e-12 * (1.0 + fabs(x));
    const bool r0 = (S00 > 0.0) & (a0 > 0.0) & (a0 * a0 > g2 * S00);
    const double v1e = zr - (mr - (xp[0] * c0 + xp[1] * s0));
    const double a1 = fabs(v1e) - X * (fabs(ma - ma0) + QR_TRIG_EPS) - 1e-12 * (1.0 + fabs(zr) + fabs(mr) + X);
    const double S11u = H2 * tr5 * (1.0 + 1e-5 + eta) + Rm[3];
    const bool r1 = (a1 > 0.0) & (a1 * a1 > g2 * S11u);
    return ok & (r0 | r1);
}

// The mailbox: cooperating workgroups exchange words through one slot per workgroup and parity,
// written with 8-byte agent-scope atomic stores, drained by s_waitcnt and a workgroup barrier before
// a data-tagged word (launch epoch, phase code, payload) that the readers poll
// (MI355X_MICROARCH.md "Valid forms"). Every spin is bounded; a timeout sets a status bit.
__device__ __forceinline__ void mb_store(double* p, double v)
{
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ double mb_load(const double* p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// mailbox slot words (the package words double as the LDS package layout)
enum { MB_BEST = 0, MB_S = 1, MB_SI = 5, MB_V = 9, MB_H = 11, MB_KR = 14, MB_UR = 20, MB_VH = 26 };

// tag word: bits 63..32 launch epoch, 31..24 phase code, 23..0 payload. Codes 1..64 are the
// lines of the sequential association; the speculative exchanges use their own codes.
enum { TAG_SPEC_LISTS = 0x81, TAG_SPEC_WINNERS = 0x82, TAG_SPEC_VERDICT = 0x83 };

__device__ __forceinline__ void mb_tag(double* slot, unsigned epoch, unsigned code, unsigned payload)
{
    const unsigned long long want = ((unsigned long long)epoch << 8) | code;
    __hip_atomic_store(reinterpret_cast<unsigned long long*>(slot + MB_BEST), (want << 24) | payload,
                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Thread k < G polls workgroup k's tag of the given parity until it carries (epoch, code);
// returns its payload (-1 on timeout, with the status bit set).
// Every wait gives up after 2^spin polls (≈0.5 s at 24) and sets the timeout bit; a thread whose
// status already holds it does not wait again (the launch is rolled back anyway).
__device__ __forceinline__ int mb_poll(const double* mbox, int par, int G, int k, int mbw,
                                       unsigned epoch, unsigned code, int& status, int spin)
{
    const unsigned long long want = ((unsigned long long)epoch << 8) | code;
    const unsigned long long* tw =
        reinterpret_cast<const unsigned long long*>(mbox + ((size_t)par * G + k) * mbw + MB_BEST);
    unsigned long long v = __hip_atomic_load(tw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    int polls = 0;
    while ((v >> 24) != want) {
        __builtin_amdgcn_s_sleep(1);
        if ((status & EKF_ST_TIMEOUT_BIT) || ++polls > (1 << spin)) {   // a workgroup never arrived
            status |= EKF_ST_TIMEOUT_BIT;
            return -1;
        }
        v = __hip_atomic_load(tw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    return (int)(v & 0xffffffu);
}

// Speculative list words carry their own tag: bits 63..40 the launch epoch (mod 2^24), bits
// 39..0 the payload, written with one 8-byte atomic store, so a reader needs one poll of the word
// itself (no separate tag word and second load). They live in the last 16 words of each
// workgroup's parity-0 mailbox slot (MB_LIST_BACK), which nothing else writes, and every
// speculative launch rewrites all SPEC_L of them.
constexpr int LIST_TAG_SHIFT = 40;
constexpr int MB_LIST_BACK = 16;

__device__ __forceinline__ void mb_store_tagged(double* p, unsigned epoch, unsigned long long payload)
{
    const unsigned long long w = ((unsigned long long)(epoch & 0xffffffu) << LIST_TAG_SHIFT) | payload;
    __hip_atomic_store(reinterpret_cast<unsigned long long*>(p), w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ unsigned long long mb_wait_tagged(const double* p, unsigned epoch, int& status, int spin)
{
    const unsigned long long* w = reinterpret_cast<const unsigned long long*>(p);
    const unsigned long long want = epoch & 0xffffffu;
    unsigned long long v = __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    int polls = 0;
    while ((v >> LIST_TAG_SHIFT) != want) {
        __builtin_amdgcn_s_sleep(1);
        if ((status & EKF_ST_TIMEOUT_BIT) || ++polls > (1 << spin)) {
            status |= EKF_ST_TIMEOUT_BIT;
            return 0;
        }
        v = __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    return v & ((1ull << LIST_TAG_SHIFT) - 1);
}

// Symmetric downdate operands (fp32 operand storage, every mode but the reference's asymmetric
// R): the landmark block's share of P −= K·S·Kᵀ (Robot.cpp:560-568) is stored as U·Vᵀ with
// V = K·F and U = −2^x·V (x the fp16 storage exponent, else 0), F·Fᵀ = S: the lower Cholesky
// factor of the symmetrised S, in fp32 like the operands themselves (a non-positive pivot
// contributes 0, which happens only where S is singular and K = 0). Every stored element then
// gets the same products whichever orientation is stored (staged_blocks). The scan's own fp64
// chain (gain_rows: W, K, y, the eager robot-strip and diagonal-block downdates, the corrections
// of later lines) keeps K·S·Kᵀ; only the stored operands take this form.
__device__ __forceinline__ void sym_factor_S(const double S[4], float F[3])
{
    const float a = (float)S[0], b = 0.5f * ((float)S[1] + (float)S[2]);
    const float c = (float)S[3];
    // v_rsq_f32 (1 ulp): F need not be correctly rounded, only the same on every thread
    F[0] = F[1] = F[2] = 0.f;
    if (a > 0.f) {
        const float ra = __builtin_amdgcn_rsqf(a);
        F[0] = a * ra;
        F[1] = b * ra;
        const float dd = c - F[1] * F[1];
        F[2] = dd > 0.f ? dd * __builtin_amdgcn_rsqf(dd) : 0.f;
    } else {
        F[2] = c > 0.f ? c * __builtin_amdgcn_rsqf(c) : 0.f;
    }
}

__device__ __forceinline__ void sym_factor(const double* pk, float F[3])
{
    const double S[4] = {pk[MB_S], pk[MB_S + 1], pk[MB_S + 2], pk[MB_S + 3]};
    sym_factor_S(S, F);
}

// The uniform gain package of a match from the matching landmark's state: S, S⁻¹, v, H row 1
// and the robot rows of K = W·S⁻¹ and U = K·S (Robot.cpp:522-602 for rows 0..2).
__device__ __forceinline__ void build_package(const Cand& c, const double R33[9], double2 rr0,
                                              double2 rr1, double2 rr2, double* pk)
{
    const double RL0[3] = {rr0.x, rr1.x, rr2.x};
    const double RL1[3] = {rr0.y, rr1.y, rr2.y};
    pk[MB_S + 0] = c.S[0]; pk[MB_S + 1] = c.S[1];
    pk[MB_S + 2] = c.S[2]; pk[MB_S + 3] = c.S[3];
    pk[MB_SI + 0] = c.Si[0]; pk[MB_SI + 1] = c.Si[1];
    pk[MB_SI + 2] = c.Si[2]; pk[MB_SI + 3] = c.Si[3];
    pk[MB_V + 0] = c.v[0]; pk[MB_V + 1] = c.v[1];
    pk[MB_H + 0] = c.h10; pk[MB_H + 1] = c.h11; pk[MB_H + 2] = c.h1l;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        // W = P·Hᵀ (Robot.cpp:522), K = W·S⁻¹ (:526), U = K·S (:560)
        const double w0 = -R33[a * 3 + 2] + RL0[a];
        const double w1 = c.h10 * R33[a * 3 + 0] + c.h11 * R33[a * 3 + 1] + c.h1l * RL0[a] + RL1[a];
        const double k0 = w0 * c.Si[0] + w1 * c.Si[2];
        const double k1 = w0 * c.Si[1] + w1 * c.Si[3];
        pk[MB_KR + 2 * a] = k0;
        pk[MB_KR + 2 * a + 1] = k1;
        pk[MB_UR + 2 * a] = k0 * c.S[0] + k1 * c.S[2];
        pk[MB_UR + 2 * a + 1] = k0 * c.S[1] + k1 * c.S[3];
    }
}

// The two rows of one landmark for a match: its block of column jstar with the earlier matches
// of the scan applied (Robot.cpp:560-568, in order), W = P·Hᵀ, K = W·S⁻¹, U = K·S, y += K·v
// (Robot.cpp:522-589), and the eager downdate of its robot-strip columns and diagonal block.
// `uq_of(q)` / `vq_of(q)` return the landmark's U rows and jstar's V rows of the scan's match q.
// MAXQ > 0: at most MAXQ earlier matches (the speculative path). (Applying all MAXQ rows
// branch-free on zeroed rows measured slower: DESIGN.md §10.)
// One earlier match q's correction of a landmark's block of a later match's column (Robot.cpp:560-568
// in order): blk −= U_q(own rows)·V_q(column rows)ᵀ, four independent fused chains. Every path that
// corrects a block (gain_rows, all at once; the speculative landmark waves, one match at a time)
// runs this sequence per element, so they agree bit for bit.
__device__ __forceinline__ void correct_block(double blk[4], const double4& uq, const double4& vh)
{
    blk[0] = fma(-uq.x, vh.x, blk[0]);
    blk[1] = fma(-uq.x, vh.z, blk[1]);
    blk[2] = fma(-uq.z, vh.x, blk[2]);
    blk[3] = fma(-uq.z, vh.z, blk[3]);
    blk[0] = fma(-uq.y, vh.y, blk[0]);
    blk[1] = fma(-uq.y, vh.w, blk[1]);
    blk[2] = fma(-uq.w, vh.y, blk[2]);
    blk[3] = fma(-uq.w, vh.w, blk[3]);
}

// The package words the landmark rows of a match read (Robot.cpp:522-589): S, S⁻¹, v, H row 1 and
// the robot rows of U = K·S
struct PkCore {
    double S[4], Si[4], v[2], h[3], Ur[6];
};
__device__ __forceinline__ void gain_core(const PkCore& P, const double blk[4], double2& rr0, double2& rr1,
                                          double2& rr2, double2& yb, double Dj[4], double kk[4], double uu[4]);

template <int MAXQ, typename UQ, typename VQ>
__device__ __forceinline__ void gain_rows(const double* pk, int t, UQ uq_of, VQ vq_of, double blk[4],
                                          double2& rr0, double2& rr1, double2& rr2, double2& yb,
                                          double Dj[4], double kk[4], double uu[4])
{
    // earlier matches of this scan, in order: four independent fused chains (one per entry), the
    // rows of match q + 1 loaded before match q's products (LDS latency off the chain). t is the
    // scan's match count, the same on every lane: a scalar loop
    auto correct = [&](const double4& uq, const double4& vh) __attribute__((always_inline)) {
        correct_block(blk, uq, vh);
    };
    // matches in pairs (both pairs' rows loaded together: one LDS round trip per two matches),
    // then the odd one; the products in q order either way
    const int tu = __builtin_amdgcn_readfirstlane(MAXQ > 0 ? min(t, MAXQ) : t);
    int q = 0;
#pragma unroll 1
    for (; q + 1 < tu; q += 2) {
        const double4 ua = uq_of(q), va = vq_of(q);
        const double4 ub = uq_of(q + 1), vb = vq_of(q + 1);
        correct(ua, va);
        correct(ub, vb);
    }
    if (q < tu) correct(uq_of(q), vq_of(q));
    PkCore P;
#pragma unroll
    for (int a = 0; a < 4; a++) {
        P.S[a] = pk[MB_S + a];
        P.Si[a] = pk[MB_SI + a];
    }
    P.v[0] = pk[MB_V];
    P.v[1] = pk[MB_V + 1];
    P.h[0] = pk[MB_H];
    P.h[1] = pk[MB_H + 1];
    P.h[2] = pk[MB_H + 2];
#pragma unroll
    for (int a = 0; a < 6; a++) P.Ur[a] = pk[MB_UR + a];
    gain_core(P, blk, rr0, rr1, rr2, yb, Dj, kk, uu);
}

// The gain rows from the corrected block (gain_rows without the earlier matches' corrections),
// the package's words in registers: every path computes them with this one expression set
__device__ __forceinline__ void gain_core(const PkCore& P, const double blk[4], double2& rr0, double2& rr1,
                                          double2& rr2, double2& yb, double Dj[4], double kk[4], double uu[4])
{
    const double S0 = P.S[0], S1 = P.S[1], S2 = P.S[2], S3 = P.S[3];
    const double Si0 = P.Si[0], Si1 = P.Si[1], Si2 = P.Si[2], Si3 = P.Si[3];
    const double v0 = P.v[0], v1 = P.v[1];
    const double h10 = P.h[0], h11 = P.h[1], h1l = P.h[2];
#pragma unroll
    for (int pp = 0; pp < 2; pp++) {
        const double pb0 = pp ? rr0.y : rr0.x;
        const double pb1 = pp ? rr1.y : rr1.x;
        const double pb2 = pp ? rr2.y : rr2.x;
        const double pba = blk[pp * 2 + 0], pbb = blk[pp * 2 + 1];
        const double w0 = -pb2 + pba;
        const double w1 = h10 * pb0 + h11 * pb1 + h1l * pba + pbb;
        const double k0 = w0 * Si0 + w1 * Si2;
        const double k1 = w0 * Si1 + w1 * Si3;
        kk[2 * pp] = k0;
        kk[2 * pp + 1] = k1;
        uu[2 * pp] = k0 * S0 + k1 * S2;
        uu[2 * pp + 1] = k0 * S1 + k1 * S3;
        const double dyv = k0 * v0 + k1 * v1;   // y += K·v (Robot.cpp:585-589)
        if (pp) yb.y += dyv; else yb.x += dyv;
    }
    const double* Ur = P.Ur;
    // eager downdate of the robot-strip columns and the diagonal block (Robot.cpp:568)
    rr0.x -= Ur[0] * kk[0] + Ur[1] * kk[1];
    rr0.y -= Ur[0] * kk[2] + Ur[1] * kk[3];
    rr1.x -= Ur[2] * kk[0] + Ur[3] * kk[1];
    rr1.y -= Ur[2] * kk[2] + Ur[3] * kk[3];
    rr2.x -= Ur[4] * kk[0] + Ur[5] * kk[1];
    rr2.y -= Ur[4] * kk[2] + Ur[5] * kk[3];
    Dj[0] -= uu[0] * kk[0] + uu[1] * kk[1];
    Dj[1] -= uu[0] * kk[2] + uu[1] * kk[3];
    Dj[2] -= uu[2] * kk[0] + uu[3] * kk[1];
    Dj[3] -= uu[2] * kk[2] + uu[3] * kk[3];
}

// uniform: robot 3×3 block and x_pre = y[0..2] after a match (Robot.cpp:568, 579-602)
__device__ __forceinline__ void robot_update(double R33[9], double xp[3], const double* pk)
{
    double Kr[6], Ur[6];
#pragma unroll
    for (int q = 0; q < 6; q++) {
        Kr[q] = pk[MB_KR + q];
        Ur[q] = pk[MB_UR + q];
    }
    const double v0 = pk[MB_V], v1 = pk[MB_V + 1];
    double yn[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        yn[a] = xp[a] + (Kr[2 * a] * v0 + Kr[2 * a + 1] * v1);
#pragma unroll
        for (int cc = 0; cc < 3; cc++)
            R33[a * 3 + cc] -= Ur[2 * a] * Kr[2 * cc] + Ur[2 * a + 1] * Kr[2 * cc + 1];
    }
    xp[0] = yn[0];
    xp[1] = yn[1];
    xp[2] = normalize_radian(yn[2]);   // Robot.cpp:596
}

}  // namespace ekf
