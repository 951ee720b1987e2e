// ekf_flush_2x4.h — the split-plane flush on wave-tiles of 2 × 4 tiles.
#pragma once

#include "ekf_flush_common.h"

// (contraction: free, as in every flush header; the products that matter are MFMA chains)
#pragma clang fp contract(fast)

namespace ekf {

// Split-bf16 flush on wave-tiles of 2 × 4 tiles (EKF_ARITH_BF16X6; the default form for its groups).
// The 2 × 2 form of flush_f32_wave_kernel<TS, NS, true> streams 12 KB of operand planes per step
// through a CU's vector memory path per wave (3 KB per tile and step: 62 B per clock for the four
// waves at the MFMA rate) beside its tile stream, and every operand wait of a wave also waits for
// its older tile loads (one in-order vmcnt). Measured at N = 4096, E = 8, T = 12 (timing builds):
// MFMA alone 0.36 ms, + operand planes 0.46, + tiles 0.41, both 0.63. A 2 × 4 wave-tile needs 18 KB
// per step for twice the MFMAs (2.25 KB per tile and step) and amortises each wave-tile's
// boundary and tile-stream waits over twice the MFMA time. Registers: 8 accumulators (128), the
// next wave-tile's tiles (128 fp32 / 64 fp16), a ring of 2 operand step-sets (144). Otherwise the
// 2 × 2 form's scheme: one 4-wave workgroup per CU, barrier-free waves, XCD-ranged K-strided walk
// of a panel-ordered table (p.wt24: 8 wave-tile columns per panel), tile prefetch one wave-tile
// ahead, operand ring one step ahead across wave-tile boundaries, −P in the accumulators (fp16:
// scaled out of the storage exponent), invalid slots stored to the sink. Groups in which some
// instance of the wave resets or adds rows run wt_general on the two 2 × 2 halves.
// F16 (EKF_ARITH_F16X3, EKF_OPT_FLUSH_FORM = 24): two fp16 planes of 2^σ·V, three products; the
// 2 × 2 form then streams 8 KB of planes per wave and step for 12 MFMAs, which at the four waves'
// MFMA rate is more than a CU's 64 B per clock: 2 × 4 streams 12 KB for 24. Groups whose σ
// changes run the general halves too.
constexpr int W4_R = 2, W4_C = 4, W4_N = W4_R * W4_C;
template <typename TS, int NS, bool F16 = false>
__global__ __launch_bounds__(DD_THREADS, 1) void flush_bf24_kernel(DowndateParams p)
{
    static_assert(NS >= 2 && NS % 2 == 0 && NS <= PMAX, "even step count");
    constexpr bool HALF = sizeof(TS) == 2;
    constexpr int NPL = F16 ? 2 : 3;
    constexpr int RD = (F16 && NS % 4 == 0) ? 4 : 2;   // operand ring depth (divides NS)
    typedef typename std::conditional<F16, f16x8r, bf16x8r>::type bf16x8;
    using Raw = typename std::conditional<HALF, f16x4, f32x4>::type;
    const Dims d = p.d;
    const int nwt = p.nwt24;
    const int total = p.E * nwt;
    const int per = (total + 7) / 8;
    const int xcd = blockIdx.x & 7;
    const int K = (int)(gridDim.x >> 3) * (DD_THREADS / 64);     // waves per XCD
    const int g_end = min(total, (xcd + 1) * per);
    const int g0 = __builtin_amdgcn_readfirstlane(
        xcd * per + (int)(blockIdx.x >> 3) * (DD_THREADS / 64) + (int)(threadIdx.x >> 6));
    if (g0 >= g_end) return;
    const int lane = threadIdx.x & 63;
    const int nb = d.nb;
    const size_t inst_elems = (size_t)d.ntiles * TILE_ELEMS;
    const TS* Pin = reinterpret_cast<const TS*>(p.Pin);
    TS* Pout = reinterpret_cast<TS*>(p.Pout);
    TS* sink = reinterpret_cast<TS*>(p.sink);

    bool fast = true;
    {
        const int e_lo = g0 / nwt, e_hi = (g_end - 1) / nwt;
        for (int e = e_lo; e <= e_hi; e++)
#pragma unroll
            for (int q = 0; q < NS; q++) {
                const int* r = p.steps[q].res + (size_t)e * RES_STRIDE;
                fast = fast && !sload(r + RES_RESET) && sload(r + RES_NADD) == 0 && !sload(r + RES_ROLLBACK);
                if (F16) fast = fast && sload(r + RES_PSIG) == sload(p.steps[0].res + (size_t)e * RES_STRIDE + RES_PSIG) &&
                                sload(r + RES_PSIG) != PLANE_SIGMA_EXACT;
            }
    }
    struct Item {
        int e, li, wr, wc;
    };
    auto load_item = [&](int e, int li, Item& t) __attribute__((always_inline)) {
        t.e = e;
        t.li = li;
        const int v = sload(p.wt24 + (e < p.E ? li : 0));
        t.wr = v & 0xffff;
        t.wc = v >> 16;
    };
    auto next_item = [&](const Item& c, Item& t) __attribute__((always_inline)) {
        int li = c.li + K, e = c.e;
        while (li >= nwt) {
            li -= nwt;
            e++;
        }
        load_item(e, li, t);
    };
    // slot (r, c): tile (2wr + r, 4wc + c) if stored, else a stored tile of the wave-tile
    auto slot_tile = [&](const Item& t, int i, bool& valid) __attribute__((always_inline)) {
        const int bi = W4_R * t.wr + i / W4_C, bj = W4_C * t.wc + i % W4_C;
        valid = bi < nb && bj < nb && bi <= bj;
        return valid ? tile_index(bi, bj, nb) : tile_index(W4_R * t.wr, min(W4_C * t.wc + W4_C - 1, nb - 1), nb);
    };
    auto op_rowA = [&](const Item& t, int r) __attribute__((always_inline)) { return min(W4_R * t.wr + r, nb - 1); };
    auto op_rowB = [&](const Item& t, int c) __attribute__((always_inline)) { return min(W4_C * t.wc + c, nb - 1); };

    if (!fast) {
        Item t;
        load_item(g0 / nwt, g0 - (g0 / nwt) * nwt, t);
        for (int g = g0; g < g_end; g += K) {
            if (g != g0) {
                Item n;
                next_item(t, n);
                t = n;
            }
#pragma unroll 1
            for (int h = 0; h < 2; h++) {
                WtEntry w;
                w.valid = 0;
#pragma unroll
                for (int i = 0; i < WT_N; i++) {
                    bool v;
                    w.tile[i] = (int)slot_tile(t, (i / WT_C) * W4_C + 2 * h + i % WT_C, v);
                    w.valid |= (v ? 1 : 0) << i;
                }
                w.rows[0] = op_rowA(t, 0) | (op_rowA(t, 1) << 16);
                w.rows[1] = op_rowB(t, 2 * h) | (op_rowB(t, 2 * h + 1) << 16);
                w.rc = t.wr | ((2 * t.wc + h) << 16);
                wt_general<TS, NS>(p, t.e, w, lane);
            }
        }
        return;
    }

    const size_t pstride = (size_t)nb * NPL * 64;   // 16-byte operands per instance
    auto pl_base = [&](int q) __attribute__((always_inline)) {
        int sl = p.slot0 + q;
        if (sl >= p.nslots) sl -= p.nslots;
        return reinterpret_cast<const bf16x8*>(reinterpret_cast<const char*>(p.bbase) + (size_t)sl * (size_t)p.bslot_bytes);
    };
    Raw pref[W4_N][4];
    f32x16 acc[W4_N];
    bf16x8 R[RD][W4_R + W4_C][NPL];
    auto load_ops = [&](int r, const Item& t, int q) __attribute__((always_inline)) {
        const bf16x8* b = pl_base(q) + t.e * pstride + lane;
#pragma unroll
        for (int i = 0; i < W4_R + W4_C; i++) {
            const bf16x8* rb = b + (size_t)(i < W4_R ? op_rowA(t, i) : op_rowB(t, i - W4_R)) * NPL * 64;
#pragma unroll
            for (int pl = 0; pl < NPL; pl++) R[r][i][pl] = rb[pl * 64];
        }
    };
    auto load_tiles = [&](const Item& t) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < W4_N; i++) {
            bool v;
            const Raw* tl = reinterpret_cast<const Raw*>(Pin + (size_t)t.e * inst_elems + (size_t)slot_tile(t, i, v) * TILE_ELEMS);
#pragma unroll
            for (int qq = 0; qq < 4; qq++) pref[i][qq] = __builtin_nontemporal_load(tl + lane + qq * 64);
        }
    };
    // −P in the accumulators, scaled: fp16 storage out of its exponent x, F16 by 2^(2σ) (the
    // group's one σ): −2^(2σ − x)
    auto in_scale = [&](const Item& t) __attribute__((always_inline)) {
        int ex = F16 ? 2 * sload(p.steps[0].res + (size_t)t.e * RES_STRIDE + RES_PSIG) : 0;
        if constexpr (HALF) ex -= sload(p.pexp + t.e);
        return -ldexpf(1.0f, ex);
    };
    Item cur, nxt, nxt2;
    load_item(g0 / nwt, g0 - (g0 / nwt) * nwt, cur);
    next_item(cur, nxt);
    load_tiles(cur);
#pragma unroll
    for (int q = 0; q < RD - 1; q++) load_ops(q, cur, q);
    int g = g0;
    while (true) {
        const bool more = g + K < g_end;
        next_item(nxt, nxt2);
        const Item ldi = more ? nxt : cur;   // the last wave-tile re-reads its own rows
        const float isc = in_scale(cur);
#pragma unroll
        for (int i = 0; i < W4_N; i++)
#pragma unroll
            for (int qq = 0; qq < 4; qq++)
#pragma unroll
                for (int j = 0; j < 4; j++) acc[i][4 * qq + j] = (float)pref[i][qq][j] * isc;
        if (more) load_tiles(nxt);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int q = 0; q < NS; q++) {
            const int ql = q + RD - 1;
            if (ql < NS) load_ops(ql % RD, cur, ql);
            else load_ops(ql % RD, ldi, ql - NS);
            const int r = q % RD;
            if constexpr (F16) {
                // (lo, hi), (hi, lo), (hi, hi): 24 MFMAs beside the 12 plane loads
#pragma unroll
                for (int pp = 0; pp < 3; pp++) {
                    const int pa = pp == 0 ? 1 : 0, pb = pp == 1 ? 1 : 0;
#pragma unroll
                    for (int rr = 0; rr < W4_R; rr++)
#pragma unroll
                        for (int c = 0; c < W4_C; c++)
                            acc[rr * W4_C + c] = __builtin_amdgcn_mfma_f32_32x32x16_f16(
                                R[r][rr][pa], R[r][W4_R + c][pb], acc[rr * W4_C + c], 0, 0, 0);
                }
#pragma unroll
                for (int i = 0; i < 12; i++) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);   // MFMA
                    __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);   // VMEM read
                }
            } else {
                // part products smallest first: (mid, mid), (hi, lo), (lo, hi), (hi, mid), (mid, hi), (hi, hi)
#pragma unroll
                for (int pp = 0; pp < 6; pp++) {
                    const int pa = (0x102010 >> (4 * (5 - pp))) & 0xf;
                    const int pb = (0x120100 >> (4 * (5 - pp))) & 0xf;
#pragma unroll
                    for (int rr = 0; rr < W4_R; rr++)
#pragma unroll
                        for (int c = 0; c < W4_C; c++)
                            acc[rr * W4_C + c] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                                R[r][rr][pa], R[r][W4_R + c][pb], acc[rr * W4_C + c], 0, 0, 0);
                }
#pragma unroll
                for (int i = 0; i < 6; i++) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 8, 0);   // MFMA
                    __builtin_amdgcn_sched_group_barrier(0x020, 3, 0);   // VMEM read
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        const float osc = 1.0f / isc;   // (a power of two: exact)
#pragma unroll
        for (int i = 0; i < W4_N; i++) {
            bool v;
            const size_t ti = slot_tile(cur, i, v);
            TS* tl = v ? Pout + (size_t)cur.e * inst_elems + ti * TILE_ELEMS : sink;
#pragma unroll
            for (int k = 0; k < 16; k++) acc[i][k] = acc[i][k] * osc;
#pragma unroll
            for (int qq = 0; qq < 4; qq++) tile_st(tl, lane, qq, acc[i]);
        }
        if (!more) break;
        g += K;
        cur = nxt;
        nxt = nxt2;
    }
}

}  // namespace ekf
