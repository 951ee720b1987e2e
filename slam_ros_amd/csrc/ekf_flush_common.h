// ekf_flush_common.h — what the flush kernels share: tile loads and stores, the augmented rows'
// values, the general (reset / new rows) path of the wave forms.
#pragma once

#include "ekf_device.h"

// (contraction: free, as in every flush header; the products that matter are MFMA chains)
#pragma clang fp contract(fast)

namespace ekf {

// ---------------------------------------------------------------------------------------
// 2. covariance downdate of the landmark block on MFMA, one pass for a group of steps
// ---------------------------------------------------------------------------------------
// For every stored 32×32 tile and every step of the group, in order: the capacity reset
// (Robot.cpp:893-904), or X ← X − U_t·V_tᵀ summed over the step's matches (rank 2m, the
// reference's m dense passes of Robot.cpp:560-572) followed by the rows of the landmarks that
// step appended (Robot.cpp:845-862). The tile stays in the MFMA accumulators for the whole
// group: one HBM read and one write per tile per group.
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// value of landmark-block element (i, j) written by a step's augmentation
__device__ __forceinline__ double patched_value(const double* prw0, const double* pdg, int M,
                                                int s0, int i, int j)
{
    const int li = i >> 1, lj = j >> 1;
    const int hi = li > lj ? li : lj;
    const int qa = hi - s0;
    if (li == lj) return pdg[qa * 4 + (i & 1) * 2 + (j & 1)];
    const double* prw = prw0 + (size_t)qa * 2 * M;
    return (li > lj) ? prw[(size_t)(i & 1) * M + j] : prw[(size_t)(j & 1) * M + i];
}

// fp32-layout tiles in fp32 or fp16 storage: lane's 4 consecutive elements of accumulator group qq
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

template <typename TS>
__device__ __forceinline__ f32x4 tile_ld(const TS* tile, int lane, int qq)
{
    if constexpr (sizeof(TS) == 4) {
        return __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(tile) + lane + qq * 64);
    } else {
        const f16x4 h = __builtin_nontemporal_load(reinterpret_cast<const f16x4*>(tile) + lane + qq * 64);
        return f32x4{(float)h[0], (float)h[1], (float)h[2], (float)h[3]};
    }
}

template <typename TS>
__device__ __forceinline__ void tile_st(TS* tile, int lane, int qq, const f32x16& a)
{
    if constexpr (sizeof(TS) == 4) {
        const f32x4 v = {a[4 * qq + 0], a[4 * qq + 1], a[4 * qq + 2], a[4 * qq + 3]};
        __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(tile) + lane + qq * 64);
    } else {
        const f16x4 v = {(_Float16)a[4 * qq + 0], (_Float16)a[4 * qq + 1], (_Float16)a[4 * qq + 2],
                         (_Float16)a[4 * qq + 3]};
        __builtin_nontemporal_store(v, reinterpret_cast<f16x4*>(tile) + lane + qq * 64);
    }
}


// fp16 storage: the value a step leaves in the block is its fp16 rounding (see Stor)
template <typename TS>
__device__ __forceinline__ void round_acc(f32x16& a)
{
    if constexpr (sizeof(TS) == 2) {
#pragma unroll
        for (int k = 0; k < 16; k++) a[k] = round_step<_Float16>(a[k]);
    }
}

constexpr int SBK = 8;   // MFMA k-steps per staged chunk (2 float4 per lane per block)

// scalar (constant address space) load of a wave-uniform word that no kernel of this launch
// writes: keeps the control words on lgkmcnt, out of the vmcnt queue the prefetch occupies
template <typename T>
__device__ __forceinline__ T sload(const T* ptr)
{
    return *(const __attribute__((address_space(4))) T*)(ptr);
}

// One WT_R × WT_C wave-tile (instance e, table entry w) through a group of NS steps in order, operands
// loaded in place: per step its reset, or the rank-2m downdate (v_mfma_f32_32x32x2_f32, the exact
// k-ordered chain, fp16 rounding per step; once per group, at the store, under p.bf) and then its augmented rows (one tile at a time through
// acc[0], rotating the accumulators). Tiles outside the triangle are stored to the sink tile. The
// general path of the wave flushes (groups with a reset or new rows in some instance of the wave).
template <typename TS, int NS>
__device__ __forceinline__ void wt_general(const DowndateParams& p, int e, const WtEntry& w, int lane)
{
    const Dims d = p.d;
    const int kh = d.kmax / 2;
    const size_t opstride = (size_t)d.nb * 64 * kh;
    const size_t inst_elems = (size_t)d.ntiles * TILE_ELEMS;
    const TS* Pin = reinterpret_cast<const TS*>(p.Pin);
    TS* Pout = reinterpret_cast<TS*>(p.Pout);
    TS* sink = reinterpret_cast<TS*>(p.sink);
    const int lofs = lane * kh;
    auto op_row = [&](int side, int k) { return (w.rows[side] >> (16 * k)) & 0xffff; };
    f32x16 acc[WT_N];
#pragma unroll
    for (int i = 0; i < WT_N; i++) {
        const TS* tl = Pin + (size_t)e * inst_elems + (size_t)w.tile[i] * TILE_ELEMS;
#pragma unroll
        for (int qq = 0; qq < 4; qq++) {
            const f32x4 v = tile_ld(tl, lane, qq);
#pragma unroll
            for (int j = 0; j < 4; j++) acc[i][4 * qq + j] = v[j];
        }
    }
    const int wr = w.rc & 0xffff, wc = w.rc >> 16;
    for (int q = 0; q < NS; q++) {
        const int* r = p.steps[q].res + (size_t)e * RES_STRIDE;
        const int reset = sload(r + RES_RESET);
        const int kc = reset ? 0 : sload(r + RES_KSTEPS);
        if (kc > 0) {
            const float* U = u_rows_flush(p, p.steps[q], e, opstride) + lofs;
            const float* V = reinterpret_cast<const float*>(p.steps[q].Vop) + e * opstride + lofs;
            const float us = us_of<TS>(p, e);
            f32x4 a[WT_R][2], b[WT_C][2];
#pragma unroll
            for (int rr = 0; rr < WT_R; rr++) {
                const float* src = U + (size_t)op_row(0, rr) * 64 * kh;
                a[rr][0] = *reinterpret_cast<const f32x4*>(src) * us;
                a[rr][1] = *reinterpret_cast<const f32x4*>(src + 4) * us;
            }
#pragma unroll
            for (int c = 0; c < WT_C; c++) {
                const float* src = V + (size_t)op_row(1, c) * 64 * kh;
                b[c][0] = *reinterpret_cast<const f32x4*>(src);
                b[c][1] = *reinterpret_cast<const f32x4*>(src + 4);
            }
#pragma unroll
            for (int s = 0; s < SBK; s++)
                if (s < kc) {
#pragma unroll
                    for (int rr = 0; rr < WT_R; rr++)
#pragma unroll
                        for (int c = 0; c < WT_C; c++)
                            acc[rr * WT_C + c] = __builtin_amdgcn_mfma_f32_32x32x2f32(
                                a[rr][s >> 2][s & 3], b[c][s >> 2][s & 3], acc[rr * WT_C + c], 0, 0, 0);
                }
            if (!p.bf) {   // split-bf16 flushes round fp16 storage once per group (at the store)
#pragma unroll
                for (int i = 0; i < WT_N; i++) round_acc<TS>(acc[i]);
            }
        }
        if (reset) {
#pragma unroll
            for (int i = 0; i < WT_N; i++)
#pragma unroll
                for (int k = 0; k < 16; k++) acc[i][k] = 0.f;
            continue;
        }
        const int nadd = sload(r + RES_NADD), s0 = sload(r + RES_SAVED_IN);
        if (nadd <= 0 || (wc + 1) * WT_C * 16 <= s0 || wc * WT_C * 16 >= s0 + nadd) continue;
        const double* prw0 = p.steps[q].patch + (size_t)e * d.max_lines * 2 * d.M;
        const double* pdg = p.steps[q].patch_diag + (size_t)e * d.max_lines * 4;
        const int ex = storage_exp<TS>(p.pexp, e);
#pragma nounroll
        for (int i = 0; i < WT_N; i++) {
            const int bi = wr * WT_R + i / WT_C, bj = wc * WT_C + i % WT_C;
            if (((w.valid >> i) & 1) && bj * 16 + 15 >= s0 && bj * 16 < s0 + nadd) {
                const int col = bj * 32 + (lane & 31);
#pragma unroll
                for (int k = 0; k < 16; k++) {
                    const int row = bi * 32 + (k & 3) + 8 * (k >> 2) + 4 * (lane >> 5);
                    const int hi = max(row >> 1, col >> 1);
                    if (hi >= s0 && hi < s0 + nadd) {
                        const float v = to_domain<TS>(patched_value(prw0, pdg, d.M, s0, row, col), ex);
                        acc[0][k] = p.bf ? v : round_step<TS>(v);
                    }
                }
            }
            const f32x16 t0 = acc[0];
#pragma unroll
            for (int j = 0; j < WT_N - 1; j++) acc[j] = acc[j + 1];
            acc[WT_N - 1] = t0;
        }
    }
#pragma unroll
    for (int i = 0; i < WT_N; i++) {
        TS* tl = ((w.valid >> i) & 1) ? Pout + (size_t)e * inst_elems + (size_t)w.tile[i] * TILE_ELEMS : sink;
#pragma unroll
        for (int qq = 0; qq < 4; qq++) tile_st(tl, lane, qq, acc[i]);
    }
}

}  // namespace ekf
