// ekf_device.h — the device code every kernel of the EKF-SLAM update (slam_ros Robot::localize)
// shares: the storage types and the landmark block read with the pending steps applied.
//
// Per scan (one "step"), all E ensemble instances at once:
//   1. scan_kernel (⌈N/256⌉ cooperating 256-thread workgroups per instance, stream S)
//        predict of the robot strip (Robot.cpp:130-286: Fx = I outside rows 0..2), then for
//        every observed line in order: Mahalanobis gating of all unmatched saved landmarks in
//        parallel + min-index reduction (== the reference's first passing candidate,
//        Robot.cpp:313-504); for a match the gain chain in deferred low-rank form
//        (Robot.cpp:515-602): W_t = P_{t-1}·H_tᵀ, K_t = W_t·S_t⁻¹, U_t = K_t·S_t, y += K_t·v_t.
//        Landmark augmentation (Robot.cpp:776-866) and the capacity reset decision
//        (Robot.cpp:893-904) run at the end of the same kernel; the new landmarks' rows of the
//        landmark block go to the step's slot (patch buffers), the rank-2m operands U/V to the
//        slot's MFMA-ordered operand buffers.
//   2. flush (stream S; D when pipelined): one pass over the packed landmark block applying a
//        group of T steps in order — per step X ← X − U_t·V_tᵀ (rank 2m on MFMA, the reference's
//        m dense n×n passes of Robot.cpp:560-572 fused), then that step's augmented rows, or the
//        reset. Each stored tile is read and written once per group. fp32/fp16 storage:
//        flush_f32_wave_kernel (groups of 6-8 steps: barrier-free waves, one wave-tile of
//        prefetch), flush_f32_persist2_kernel (≤ 4 steps, LDS-staged super-tiles),
//        flush_f32_sb_kernel (otherwise); fp64: downdate_f64_kernel (one tile per wave).
//
// Deferred reads: between flushes the association kernels read the landmark block with the
// pending steps applied on read (pll_block): per element, the same k-ordered fp32/fp64 FMA chain
// the MFMA executes, then the patch rounded to storage, so every read sees bit-for-bit the value
// the flush will store (tests/test_gpu_parity.py::test_deferred_flush_equals_drained).
//
// The device code by topic: ekf_kernels.hip (the association: scan_kernel and what only it uses),
// ekf_shard_kernels.h (the kernels of an instance partitioned over ranks), ekf_assoc_parts.h (what those
// two share: the reject filters, the exchange, the gain chain of a match), ekf_gate.h (the gate
// arithmetic of one candidate, shared with the gate
// query), ekf_flush_common.h and one ekf_flush_*.h per flush family, ekf_pack.h;
// unit_query.hip holds the covariance queries' kernel (pll_block on chosen landmarks), unit_gate.hip
// the gate query's two kernels (trial lines against every saved landmark, state untouched),
// unit_joint.hip the joint gate's kernel (a hypothesis' stacked innovation, Cholesky in LDS).
// Each unit_*.hip includes what its launchers instantiate (build.py: UNITS).
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <type_traits>

#include "ekf_kernels.h"

// Floating-point contraction is set per header, so the include order cannot change it: this code
// contracts freely (the compiler's default for device code).
#pragma clang fp contract(fast)

namespace ekf {

#define EKF_PI 3.14159265358979323846


// Storage type T of the landmark block → compute type C (MFMA / FMA chain) and tile layout L.
// fp16 storage computes in fp32 on the f32 layout and rounds to fp16 after every step, in the
// flush and in the on-read replay alike, so the stored value never depends on when it is flushed.
// It holds 2^x·P with a per-instance exponent x (ScanParams/DowndateParams::pexp, default 10:
// |P| < 64 representable, normal down to 6e-8; chosen at upload from the largest landmark
// variance, ekf_state.hip choose_exponent). The fp16 path computes in that scaled domain
// throughout: the scan writes the U operand scaled by 2^x (exact), so flush and on-read replay
// both run acc = 2^x·X − (2^x·U)·Vᵀ, bit-for-bit 2^x × the unscaled chain, and round with two
// conversions per element; values leave the scaled domain only where they are read as P.
template <typename T> struct Stor {
    using C = T;
    using L = T;
    static constexpr bool half = false;
};
template <> struct Stor<_Float16> {
    using C = float;
    using L = float;
    static constexpr bool half = true;
};

template <typename T>
__device__ __forceinline__ T to_store(typename Stor<T>::C x)
{
    return (T)x;
}

template <typename T>
__device__ __forceinline__ typename Stor<T>::C from_store(T h)
{
    return (typename Stor<T>::C)h;
}

template <typename T>
__device__ __forceinline__ typename Stor<T>::C round_step(typename Stor<T>::C x)
{
    if constexpr (Stor<T>::half) {
        // the same instruction on every path: the compiler may otherwise pair two roundings into
        // v_cvt_pk_f16_f32 at some call sites, which does not round fp16 subnormals like
        // v_cvt_f16_f32 (the flush and the on-read replay must round bit-identically)
        float r;
        asm("v_cvt_f16_f32 %0, %1\n\tv_cvt_f32_f16 %0, %0" : "=v"(r) : "v"(x));
        return r;
    } else {
        return (typename Stor<T>::C)(T)x;
    }
}

// P value (fp64) → scaled compute domain (exponent ex, fp16 storage only), and back: power-of-two
// scalings, exact in fp32 / fp64
template <typename T>
__device__ __forceinline__ typename Stor<T>::C to_domain(double v, int ex)
{
    using C = typename Stor<T>::C;
    if constexpr (Stor<T>::half) return ldexpf((C)v, ex);
    else return (C)v;
}

template <typename T>
__device__ __forceinline__ double from_domain(typename Stor<T>::C x, int ex)
{
    if constexpr (Stor<T>::half) return ldexp((double)x, -ex);
    else return (double)x;
}

// the storage exponent of instance e (0 unless fp16)
template <typename T>
__device__ __forceinline__ int storage_exp(const int* pexp, int e);

// A flush's U operand rows of instance e: as stored, or (DowndateParams::usym: symmetric operands,
// U = −2^x·V exactly) the V rows times us_of(). Either way the same fp32 values reach the MFMAs.
template <typename TS>
__device__ __forceinline__ float us_of(const DowndateParams& p, int e)
{
    return p.usym ? -ldexpf(1.0f, storage_exp<TS>(p.pexp, e)) : 1.0f;
}
__device__ __forceinline__ const float* u_rows_flush(const DowndateParams& p, const Slot& sq, int e, size_t opstride)
{
    return reinterpret_cast<const float*>(p.usym ? sq.Vop : sq.Uop) + e * opstride;
}

template <typename T>
__device__ __forceinline__ int storage_exp(const int* pexp, int e)
{
    if constexpr (Stor<T>::half) return pexp[e];
    else return 0;
}

__device__ __forceinline__ double normalize_radian(double rad)
{
    // Robot.cpp:62-71
    if (fabs(rad) <= EKF_PI) return rad;   // (the common case, one test)
    if (rad > EKF_PI) {
        rad = rad - (2.0 * EKF_PI + floor(rad / (2.0 * EKF_PI)) * 2.0 * EKF_PI);
    } else if (rad < -EKF_PI) {
        rad = rad + (2.0 * EKF_PI + floor(fabs(rad) / (2.0 * EKF_PI)) * 2.0 * EKF_PI);
    }
    return rad;
}

// 1/a for a finite nonzero a of moderate exponent: v_rcp_f64 and two Newton steps (within an ulp;
// the association chain's divisions, which sit on its critical path, take this instead of the
// correctly rounded division)
__device__ __forceinline__ double rcp_nr(double a)
{
    double r = __builtin_amdgcn_rcp(a);
    double e = fma(-a, r, 1.0);
    r = fma(r, e, r);
    e = fma(-a, r, 1.0);
    return fma(r, e, r);
}

// gsl_linalg_LU_decomp + LU_invert on 2x2 (Robot.cpp:449-457): partial pivoting, the elimination
// and the two back substitutions of GSL, with the pivots' reciprocals (rcp_nr) in place of the
// divisions (agrees with GSL within an ulp or two per entry); false when U is singular (GSL_EDOM),
// leaving Si untouched.
__device__ __forceinline__ bool lu_invert2(const double S[4], double Si[4])
{
    // the row swap by selects and the elimination unconditionally (a zero pivot makes r0 infinite,
    // and the function then returns before using anything derived from it): the same values as
    // the branching form, without exec-mask branches on the association's serial chain
    const bool sw = fabs(S[2]) > fabs(S[0]);
    double a0 = sw ? S[2] : S[0], a1 = sw ? S[3] : S[1], a2 = sw ? S[0] : S[2], a3 = sw ? S[1] : S[3];
    const int p0 = sw ? 1 : 0, p1 = sw ? 0 : 1;
    const double r0 = rcp_nr(a0);
    const double l = a2 * r0;
    a2 = l;
    a3 -= l * a1;
    if (a0 == 0.0 || a3 == 0.0) return false;
    const double r3 = rcp_nr(a3);
#pragma unroll
    for (int c = 0; c < 2; c++) {
        double b0 = (p0 == c) ? 1.0 : 0.0;
        double b1 = (p1 == c) ? 1.0 : 0.0;
        b1 = b1 - a2 * b0;
        const double x1 = b1 * r3;
        const double x0 = (b0 - a1 * x1) * r0;
        Si[c] = x0;
        Si[2 + c] = x1;
    }
    return true;
}

// ---------------------------------------------------------------------------------------
// Landmark block as seen by a step: X plus the pending (not yet flushed) steps, in order.
// ---------------------------------------------------------------------------------------
template <typename T>
struct PllView {
    const T* X;
    int nb, kmax, M, max_lines;
    int e;            // instance
    int ex;           // storage exponent of instance e (fp16)
    size_t opstride;  // operand elements per instance
    int npend;        // pending steps (oldest first)
    const Slot* pend;
    const int4* ctl;  // per pending step {reset, ks, nadd, s0} of instance e (LDS copy)
    int rnd;          // fp16: round after every pending step, as the exact flush does (0 under
                      // the split-bf16 flush, which rounds once per group)
    int usym;         // symmetric operands: U = us·V, the U rows not stored (ScanParams::usym)
    float us;         // −2^ex if usym, else 1 (U rows read as stored)
};

// Step q's U rows as stored, or its V rows (scaled by v.us on use) for symmetric operands
template <typename T>
__device__ __forceinline__ const float* u_rows_f32(const PllView<T>& v, const Slot& sq)
{
    return reinterpret_cast<const float*>(v.usym ? sq.Vop : sq.Uop) + v.e * v.opstride;
}

// fp16 rounding of a replayed element (identity for fp32 / fp64 storage)
template <typename T>
__device__ __forceinline__ typename Stor<T>::C vround(const PllView<T>& v, typename Stor<T>::C x)
{
    return v.rnd ? round_step<T>(x) : x;
}

typedef float f32x4v __attribute__((ext_vector_type(4)));
typedef float f32x2v __attribute__((ext_vector_type(2)));
// operand planes of the split arithmetics (eight bf16 / fp16 of one lane's MFMA operand)
typedef __bf16 bf16x8r __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8r __attribute__((ext_vector_type(8)));

// Staged rows of a guessed column (LDS, per column and pending step: [U | V][row half][8]):
// the U side as in the operand layout, row half rh = (k parity) · 2 + (row of the pair), 8 k each;
// the V side interleaved by row pair, (rh, k) at (rh >> 1) · 16 + 2k + (rh & 1), so that one
// float2 holds both rows of a k (a packed-FMA operand).
__device__ __forceinline__ int stage_v_index(int rh, int k) { return (rh >> 1) * 16 + 2 * k + (rh & 1); }

// EKF_ARITH_BF16X6: v = hi + mid + lo, each a bf16 (the upper half of an fp32): truncation leaves
// an exact fp32 remainder of at most 16, then 8 significant bits, so the three parts are exact.
// Packs (a, b) into one dword per part, a in the low half (operand element order)
__device__ __forceinline__ void split_pack(float a, float b, unsigned (&o)[3])
{
#pragma unroll
    for (int pl = 0; pl < 3; pl++) {
        const unsigned ua = __builtin_bit_cast(unsigned, a) & 0xffff0000u;
        const unsigned ub = __builtin_bit_cast(unsigned, b) & 0xffff0000u;
        o[pl] = (ua >> 16) | ub;
        a -= __builtin_bit_cast(float, ua);
        b -= __builtin_bit_cast(float, ub);
    }
}

// Stored 2×2 block at rows a0, a0+1 and columns b0, b0+1 (a0, b0 even, a0's tile <= b0's):
// acc = {(a0,b0), (a0,b0+1), (a0+1,b0), (a0+1,b0+1)}. In the f32 tile layout the two rows of a
// column are adjacent and the two columns are 4 elements apart: two paired loads.
template <typename T>
__device__ __forceinline__ void load_block(const PllView<T>& v, int a0, int b0, typename Stor<T>::C (&acc)[4])
{
    using L = typename Stor<T>::L;
    if constexpr (sizeof(L) == 4) {
        const T* x = v.X + ll_offset<L>(a0, b0, v.nb);
        if constexpr (sizeof(T) == 4) {
            const float2 c0 = *reinterpret_cast<const float2*>(x);
            const float2 c1 = *reinterpret_cast<const float2*>(x + 4);
            acc[0] = from_store<T>(c0.x); acc[2] = from_store<T>(c0.y);
            acc[1] = from_store<T>(c1.x); acc[3] = from_store<T>(c1.y);
        } else {
            typedef T t2 __attribute__((ext_vector_type(2)));
            const t2 c0 = *reinterpret_cast<const t2*>(x);
            const t2 c1 = *reinterpret_cast<const t2*>(x + 4);
            acc[0] = from_store<T>(c0.x); acc[2] = from_store<T>(c0.y);
            acc[1] = from_store<T>(c1.x); acc[3] = from_store<T>(c1.y);
        }
    } else {
#pragma unroll
        for (int p = 0; p < 2; p++)
#pragma unroll
            for (int c = 0; c < 2; c++) acc[p * 2 + c] = from_store<T>(v.X[ll_offset<L>(a0 + p, b0 + c, v.nb)]);
    }
}

// The rows a step appended (Robot.cpp:845-862) replace block (i0, j0) if it lies in them:
// requested orientation, rounded as they are stored.
template <typename T>
__device__ __forceinline__ void patch_block(const PllView<T>& v, const Slot& sq, int4 cw, int i0, int j0,
                                            bool swap, typename Stor<T>::C (&acc)[4])
{
    const int nadd = cw.z, s0 = cw.w;
    const int li = i0 >> 1, lj = j0 >> 1;
    const int hi = li > lj ? li : lj;
    if (hi >= s0 && hi < s0 + nadd) {
        const int qa = hi - s0;
        const double* pdg = sq.patch_diag + (size_t)v.e * v.max_lines * 4;
        const double* prw = sq.patch + ((size_t)v.e * v.max_lines + qa) * 2 * v.M;
        double raw[4];
        if (li == lj) {
            raw[0] = pdg[qa * 4 + 0]; raw[1] = pdg[qa * 4 + 1];
            raw[2] = pdg[qa * 4 + 2]; raw[3] = pdg[qa * 4 + 3];
        } else if (li > lj) {
            raw[0] = prw[j0]; raw[1] = prw[j0 + 1];
            raw[2] = prw[v.M + j0]; raw[3] = prw[v.M + j0 + 1];
        } else {
            raw[0] = prw[i0]; raw[1] = prw[v.M + i0];
            raw[2] = prw[i0 + 1]; raw[3] = prw[v.M + i0 + 1];
        }
        if (swap) {
            acc[0] = vround<T>(v, to_domain<T>(raw[0], v.ex)); acc[1] = vround<T>(v, to_domain<T>(raw[2], v.ex));
            acc[2] = vround<T>(v, to_domain<T>(raw[1], v.ex)); acc[3] = vround<T>(v, to_domain<T>(raw[3], v.ex));
        } else {
            acc[0] = vround<T>(v, to_domain<T>(raw[0], v.ex)); acc[1] = vround<T>(v, to_domain<T>(raw[1], v.ex));
            acc[2] = vround<T>(v, to_domain<T>(raw[2], v.ex)); acc[3] = vround<T>(v, to_domain<T>(raw[3], v.ex));
        }
    }
}

// One pending step's downdate on B blocks (i0, j0[b]) in their stored orientations (pll_blocks):
// the owned rows i0, i0+1 of U and V are loaded once per k-chunk (their lanes' addresses are
// spread over many cache lines) and each column landmark's rows once (U_col for a transposed
// block, V_col otherwise; the guessed columns are the same for the whole wave). Per element the
// FMA chain of pll_blocks' per-block form, operand for operand.
template <typename T, int B>
__device__ __forceinline__ void pll_shared_step(const PllView<T>& v, const Slot& sq, int ks, int i0,
                                                const int (&j0)[B], const bool (&swap)[B],
                                                typename Stor<T>::C (&acc)[B][4])
{
    using C = typename Stor<T>::C;
    if constexpr (sizeof(C) == 4) {
        const int kh = v.kmax / 2;
        const float* U = u_rows_f32(v, sq);
        const float* V = reinterpret_cast<const float*>(sq.Vop) + v.e * v.opstride;
        const float us = v.us;
        auto row = [&](int r) { return ((size_t)(r >> 5) * 64 + (r & 31)) * kh; };
        const float* uo = U + row(i0);
        const float* vo = V + row(i0);
        const float* xc[B];
#pragma unroll
        for (int b = 0; b < B; b++) xc[b] = (swap[b] ? U : V) + row(j0[b]);
        for (int s0 = 0; s0 < ks; s0 += 4) {
            // [row, row + 1] × [k half 0, k half 1] of the owned U and V rows
            const f32x4v ue0 = *reinterpret_cast<const f32x4v*>(uo + s0) * us;
            const f32x4v ue1 = *reinterpret_cast<const f32x4v*>(uo + kh + s0) * us;
            const f32x4v uo0 = *reinterpret_cast<const f32x4v*>(uo + 32 * kh + s0) * us;
            const f32x4v uo1 = *reinterpret_cast<const f32x4v*>(uo + 33 * kh + s0) * us;
            const f32x4v ve0 = *reinterpret_cast<const f32x4v*>(vo + s0);
            const f32x4v ve1 = *reinterpret_cast<const f32x4v*>(vo + kh + s0);
            const f32x4v vo0 = *reinterpret_cast<const f32x4v*>(vo + 32 * kh + s0);
            const f32x4v vo1 = *reinterpret_cast<const f32x4v*>(vo + 33 * kh + s0);
#pragma unroll
            for (int b = 0; b < B; b++) {
                const f32x4v ce0 = *reinterpret_cast<const f32x4v*>(xc[b] + s0);
                const f32x4v ce1 = *reinterpret_cast<const f32x4v*>(xc[b] + kh + s0);
                const f32x4v co0 = *reinterpret_cast<const f32x4v*>(xc[b] + 32 * kh + s0);
                const f32x4v co1 = *reinterpret_cast<const f32x4v*>(xc[b] + 33 * kh + s0);
                const bool sw = swap[b];
                const f32x4v ae0 = sw ? ce0 * us : ue0, ae1 = sw ? ce1 * us : ue1, ao0 = sw ? co0 * us : uo0,
                             ao1 = sw ? co1 * us : uo1;
                const f32x4v be0 = sw ? ve0 : ce0, be1 = sw ? ve1 : ce1, bo0 = sw ? vo0 : co0, bo1 = sw ? vo1 : co1;
#pragma unroll
                for (int s = 0; s < 4; s++) {
                    if (s0 + s >= ks) break;
                    acc[b][0] = fmaf(ao0[s], bo0[s], fmaf(ae0[s], be0[s], acc[b][0]));
                    acc[b][1] = fmaf(ao0[s], bo1[s], fmaf(ae0[s], be1[s], acc[b][1]));
                    acc[b][2] = fmaf(ao1[s], bo0[s], fmaf(ae1[s], be0[s], acc[b][2]));
                    acc[b][3] = fmaf(ao1[s], bo1[s], fmaf(ae1[s], be1[s], acc[b][3]));
                }
            }
        }
    } else {
        const int kq = v.kmax / 4;
        const double* U = reinterpret_cast<const double*>(sq.Uop) + v.e * v.opstride;
        const double* V = reinterpret_cast<const double*>(sq.Vop) + v.e * v.opstride;
        auto row = [&](int r) { return ((size_t)(r >> 5) * 64 + (r & 15)) * (2 * kq) + ((r >> 4) & 1) * kq; };
        const double* uo = U + row(i0);
        const double* vo = V + row(i0);
        const double* xc[B];
#pragma unroll
        for (int b = 0; b < B; b++) xc[b] = (swap[b] ? U : V) + row(j0[b]);
        for (int s = 0; s < ks; s++)
#pragma unroll
            for (int kk = 0; kk < 4; kk++) {
                const size_t o = (size_t)16 * kk * 2 * kq + s;
                const double u0 = uo[o], u1 = uo[o + 2 * kq];
                const double w0 = vo[o], w1 = vo[o + 2 * kq];
#pragma unroll
                for (int b = 0; b < B; b++) {
                    const double c0 = xc[b][o], c1 = xc[b][o + 2 * kq];
                    const bool sw = swap[b];
                    const double x0 = sw ? c0 : u0, x1 = sw ? c1 : u1;
                    const double y0 = sw ? w0 : c0, y1 = sw ? w1 : c1;
                    acc[b][0] = fma(x0, y0, (double)acc[b][0]);
                    acc[b][1] = fma(x0, y1, (double)acc[b][1]);
                    acc[b][2] = fma(x1, y0, (double)acc[b][2]);
                    acc[b][3] = fma(x1, y1, (double)acc[b][3]);
                }
            }
    }
#pragma unroll
    for (int b = 0; b < B; b++)
#pragma unroll
        for (int k = 0; k < 4; k++) acc[b][k] = vround<T>(v, acc[b][k]);
}

// 2x2 blocks (i0, i0+1) × (j0[b], j0[b]+1), b < B, of the landmark block (i0, j0[b] even) as
// they will be once the pending steps are flushed: per step (in order) a reset, or the rank-2m
// downdate as the k-ordered FMA chain the MFMA executes, then the step's augmented rows rounded
// to storage. The B blocks share one pass over the pending steps so that their loads overlap.
template <typename T, int B>
__device__ __forceinline__ void pll_blocks(const PllView<T>& v, int i0, const int (&j0)[B], double (&out)[B][4])
{
    using C = typename Stor<T>::C;
    bool swap[B];
    int a0[B], b0[B];
    C acc[B][4];
#pragma unroll
    for (int b = 0; b < B; b++) {
        swap[b] = (i0 >> 5) > (j0[b] >> 5);
        a0[b] = swap[b] ? j0[b] : i0;   // stored orientation
        b0[b] = swap[b] ? i0 : j0[b];
        load_block<T>(v, a0[b], b0[b], acc[b]);
    }
    for (int q = 0; q < v.npend; q++) {
        const Slot& sq = v.pend[q];
        const int4 cw = v.ctl[q];
        if (cw.x) {
#pragma unroll
            for (int b = 0; b < B; b++) acc[b][0] = acc[b][1] = acc[b][2] = acc[b][3] = (C)0;
            continue;
        }
        const int ks = cw.y;
        if (ks > 0 && B > 1) {
            // several blocks: the owned rows' U and V loaded once per k-chunk, each column's
            // one operand per block (a block stored in owned-first orientation runs U_own·V_col,
            // a transposed one U_col·V_own): the same operands as the per-block form below
            pll_shared_step<T, B>(v, sq, ks, i0, j0, swap, acc);
        } else if (ks > 0) {
            if constexpr (sizeof(C) == 4) {
                // v_mfma_f32_32x32x2_f32 = ordered fmaf chain (k0 lanes 0-31, then k1)
                const int kh = v.kmax / 2;
                const float* ua[B];
                const float* vb[B];
#pragma unroll
                for (int b = 0; b < B; b++) {
                    ua[b] = u_rows_f32(v, sq) + ((size_t)(a0[b] >> 5) * 64 + (a0[b] & 31)) * kh;   // row a0; a0+1 at +kh
                    vb[b] = reinterpret_cast<const float*>(sq.Vop) + v.e * v.opstride +
                            ((size_t)(b0[b] >> 5) * 64 + (b0[b] & 31)) * kh;
                }
                for (int s0 = 0; s0 < ks; s0 += 4) {
                    f32x4v ae0[B], ae1[B], ao0[B], ao1[B], be0[B], be1[B], bo0[B], bo1[B];
#pragma unroll
                    for (int b = 0; b < B; b++) {
                        ae0[b] = *reinterpret_cast<const f32x4v*>(ua[b] + s0) * v.us;
                        ae1[b] = *reinterpret_cast<const f32x4v*>(ua[b] + kh + s0) * v.us;
                        ao0[b] = *reinterpret_cast<const f32x4v*>(ua[b] + 32 * kh + s0) * v.us;
                        ao1[b] = *reinterpret_cast<const f32x4v*>(ua[b] + 33 * kh + s0) * v.us;
                        be0[b] = *reinterpret_cast<const f32x4v*>(vb[b] + s0);
                        be1[b] = *reinterpret_cast<const f32x4v*>(vb[b] + kh + s0);
                        bo0[b] = *reinterpret_cast<const f32x4v*>(vb[b] + 32 * kh + s0);
                        bo1[b] = *reinterpret_cast<const f32x4v*>(vb[b] + 33 * kh + s0);
                    }
#pragma unroll
                    for (int s = 0; s < 4; s++) {
                        if (s0 + s >= ks) break;
#pragma unroll
                        for (int b = 0; b < B; b++) {
                            acc[b][0] = fmaf(ao0[b][s], bo0[b][s], fmaf(ae0[b][s], be0[b][s], acc[b][0]));
                            acc[b][1] = fmaf(ao0[b][s], bo1[b][s], fmaf(ae0[b][s], be1[b][s], acc[b][1]));
                            acc[b][2] = fmaf(ao1[b][s], bo0[b][s], fmaf(ae1[b][s], be0[b][s], acc[b][2]));
                            acc[b][3] = fmaf(ao1[b][s], bo1[b][s], fmaf(ae1[b][s], be1[b][s], acc[b][3]));
                        }
                    }
                }
            } else {
                // v_mfma_f64_16x16x4_f64 = ordered fma chain over k = 4s..4s+3
                const int kq = v.kmax / 4;
                const double* ua[B];
                const double* vb[B];
#pragma unroll
                for (int b = 0; b < B; b++) {
                    ua[b] = reinterpret_cast<const double*>(sq.Uop) + v.e * v.opstride +
                            ((size_t)(a0[b] >> 5) * 64 + (a0[b] & 15)) * (2 * kq) + ((a0[b] >> 4) & 1) * kq;
                    vb[b] = reinterpret_cast<const double*>(sq.Vop) + v.e * v.opstride +
                            ((size_t)(b0[b] >> 5) * 64 + (b0[b] & 15)) * (2 * kq) + ((b0[b] >> 4) & 1) * kq;
                }
                for (int s = 0; s < ks; s++)
#pragma unroll
                    for (int kk = 0; kk < 4; kk++) {
                        const size_t o = (size_t)16 * kk * 2 * kq + s;
#pragma unroll
                        for (int b = 0; b < B; b++) {
                            const double x0 = ua[b][o], x1 = ua[b][o + 2 * kq];
                            const double y0 = vb[b][o], y1 = vb[b][o + 2 * kq];
                            acc[b][0] = fma(x0, y0, (double)acc[b][0]);
                            acc[b][1] = fma(x0, y1, (double)acc[b][1]);
                            acc[b][2] = fma(x1, y0, (double)acc[b][2]);
                            acc[b][3] = fma(x1, y1, (double)acc[b][3]);
                        }
                    }
            }
#pragma unroll
            for (int b = 0; b < B; b++)
#pragma unroll
                for (int k = 0; k < 4; k++) acc[b][k] = vround<T>(v, acc[b][k]);
        }
        if (cw.z > 0) {
#pragma unroll
            for (int b = 0; b < B; b++) patch_block<T>(v, sq, cw, i0, j0[b], swap[b], acc[b]);
        }
    }
#pragma unroll
    for (int b = 0; b < B; b++) {
        if (swap[b]) {
            out[b][0] = from_domain<T>(acc[b][0], v.ex); out[b][1] = from_domain<T>(acc[b][2], v.ex);
            out[b][2] = from_domain<T>(acc[b][1], v.ex); out[b][3] = from_domain<T>(acc[b][3], v.ex);
        } else {
            out[b][0] = from_domain<T>(acc[b][0], v.ex); out[b][1] = from_domain<T>(acc[b][1], v.ex);
            out[b][2] = from_domain<T>(acc[b][2], v.ex); out[b][3] = from_domain<T>(acc[b][3], v.ex);
        }
    }
}

template <typename T>
__device__ __forceinline__ void pll_block(const PllView<T>& v, int i0, int j0, double out[4])
{
    const int js[1] = {j0};
    double o[1][4];
    pll_blocks<T, 1>(v, i0, js, o);
    out[0] = o[0][0]; out[1] = o[0][1]; out[2] = o[0][2]; out[3] = o[0][3];
}

// ---- the read-only view (ReadView) of unit_query.hip, unit_gate.hip and unit_joint.hip ----
// sh_ctl[PMAX] (LDS) of instance e from the pending steps' result records; the caller's barrier follows
__device__ __forceinline__ void view_ctl(const ReadView& v, const Slot* pend, int e, int4* sh_ctl)
{
    const int tid = threadIdx.x;
    if (tid < v.npend) {
        // (a rolled-back step reads as a no-op: no reset, ks = 0, no rows)
        const int* r = pend[tid].res + (size_t)e * RES_STRIDE;
        sh_ctl[tid] = make_int4(r[RES_RESET], r[RES_KSTEPS], r[RES_NADD], r[RES_SAVED_IN]);
    }
}

// instance e's landmark block with the pending steps applied on read
template <typename T>
__device__ __forceinline__ PllView<T> view_pll(const ReadView& v, const Slot* pend, int e, const int4* sh_ctl)
{
    const Dims& d = v.d;
    PllView<T> pv;
    pv.X = reinterpret_cast<const T*>(v.Pread) + (size_t)e * d.ntiles * TILE_ELEMS;
    pv.nb = d.nb;
    pv.kmax = d.kmax;
    pv.M = d.M;
    pv.max_lines = d.max_lines;
    pv.e = e;
    pv.ex = storage_exp<T>(v.pexp, e);
    pv.opstride = (size_t)d.nb * 64 * (d.kmax / 2);
    pv.usym = v.usym;
    pv.us = v.usym ? -ldexpf(1.0f, pv.ex) : 1.0f;
    pv.npend = v.npend;
    pv.pend = pend;
    pv.ctl = sh_ctl;
    pv.rnd = !v.bf;
    return pv;
}

// the committed copy of instance e's robot strip ([3][n]) and mean ([n])
struct Committed {
    const double* Rs;
    const double* y;
};
__device__ __forceinline__ Committed view_committed(const ReadView& v, int e)
{
    const int cb = v.live[e] & 1;
    return {v.Rs + ((size_t)cb * v.Etot + e) * 3 * v.d.n, v.y + ((size_t)cb * v.Etot + e) * v.d.n};
}

// the to-storage rounding a split-plane group's flush applies once (fp16 storage, `once` = a
// split-plane context; the per-step rounding of the exact arithmetic already happened in pll_block:
// PllView::rnd): the reads that leave the state untouched (unit_query.hip, unit_gate.hip) apply it
template <typename T>
__device__ __forceinline__ void query_round(bool once, int ex, double (&o)[4])
{
    if constexpr (Stor<T>::half) {
        if (once) {
#pragma unroll
            for (int k = 0; k < 4; k++) o[k] = from_domain<T>(round_step<T>(to_domain<T>(o[k], ex)), ex);
        }
    }
}

}  // namespace ekf
