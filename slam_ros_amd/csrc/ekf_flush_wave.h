// ekf_flush_wave.h — the barrier-free per-wave flush: exact fp32, split-bf16 and split-fp16.
#pragma once

#include "ekf_flush_common.h"

// (contraction: free, as in every flush header; the products that matter are MFMA chains)
#pragma clang fp contract(fast)

namespace ekf {

// f32/f16 flush, barrier-free per-wave form for groups of an even number of steps NS (2..8,
// kmax <= 16). One wave per SIMD, each working alone (no LDS, no barriers) through a sequence of
// wave-tiles of WT_R × WT_C tiles (four 32×32 accumulators). Software pipeline, one wave-tile
// deep: while wave-tile k runs its NS·32 MFMAs, the tiles of wave-tile k+1 (issued first) and its
// operand rows (step q's issued right after step q's MFMAs free their registers) stream into
// registers, so every wait of a wave-tile covers only loads issued during the one before it. The
// host table wt (WtEntry) gives each wave-tile's tile indices, operand row blocks and validity;
// the entry of wave-tile k+2 is read (scalar loads) during wave-tile k. The wave-tiles of an
// instance are walked in panels and each XCD takes a contiguous range of (instance, wave-tile),
// so the wave-tiles an XCD has in flight share their operand rows in its L2. This pipelined loop
// serves the groups in which no step of the wave's instances resets the map or adds landmarks
// (partial downdates are predicated); otherwise the wave runs a plain per-wave-tile loop. Per
// element the chain is the one every other form runs (k-ordered MFMA steps, fp16 rounding per
// step, then the step's rows or the reset): bit-identical results.
//
// BF (EKF_ARITH_BF16X6, fp32 storage, symmetric operands): the plain groups run each step as six
// v_mfma_f32_32x32x16_bf16 per accumulator on V's exact three-part bf16 split (the scan's
// planes, Slot::Bop). With U = −V the accumulators hold −X (negated on load and store, exact), so
// both operands are V planes: of the wave-tile's row blocks (A) and column blocks (B). Operands
// stream through a ring of RD step-sets, RD − 1 steps ahead, across wave-tile boundaries.
// split-plane flushes: one wave per SIMD (two at <= 256 registers and a ring of 2 measured equal;
// scripts/xp/f16_wave_switches.patch restores that and the other A/B switches of this form)
constexpr int F16_RDMAX = 8;   // split-fp16 flush: the deepest operand ring (step-sets)
// the largest divisor of ns not above rmax (at least 2)
constexpr int ring_depth(int ns, int rmax)
{
    int r = 2;
    for (int k = 2; k <= rmax; k++)
        if (ns % k == 0) r = k;
    return r;
}
template <typename TS, int NS, bool BF = false, bool F16 = false>
__global__ __launch_bounds__(DD_THREADS, 1) void flush_f32_wave_kernel(DowndateParams p)
{
    static_assert(NS >= 2 && NS % 2 == 0 && NS <= PMAX, "even step count");
    static_assert(BF || NS <= 8, "fp32 wave flush: at most 8 steps (operands of every step in registers)");
    constexpr bool HALF = sizeof(TS) == 2;
    constexpr bool AM = HALF;   // fp16 storage: pair-major step order (below)
    const Dims d = p.d;
    const int nwt = p.nwt;
    const int total = p.E * nwt;
    const int per = (total + 7) / 8;
    const int xcd = blockIdx.x & 7;
    const int K = (int)(gridDim.x >> 3) * (DD_THREADS / 64);     // waves per XCD
    const int g_end = min(total, (xcd + 1) * per);
    const int g0 = __builtin_amdgcn_readfirstlane(
        xcd * per + (int)(blockIdx.x >> 3) * (DD_THREADS / 64) + (int)(threadIdx.x >> 6));
    if (g0 >= g_end) return;

    const int lane = threadIdx.x & 63;
    const int kh = d.kmax / 2;   // 8
    const size_t opstride = (size_t)d.nb * 64 * kh;
    const size_t inst_elems = (size_t)d.ntiles * TILE_ELEMS;
    const TS* Pin = reinterpret_cast<const TS*>(p.Pin);
    TS* Pout = reinterpret_cast<TS*>(p.Pout);
    TS* sink = reinterpret_cast<TS*>(p.sink);
    const int lofs = lane * kh;

    // the pipelined loop needs every step of every instance this wave visits to be a plain
    // downdate (no reset, no new rows); the split-plane form also takes steps that add rows (it
    // writes them into the wave-tiles they touch, between the steps' MFMAs)
    bool fast = true, fast_rows = true;
    {
        const int e_lo = g0 / nwt, e_hi = (g_end - 1) / nwt;
        for (int e = e_lo; e <= e_hi; e++)
#pragma unroll
            for (int q = 0; q < NS; q++) {
                const int* r = p.steps[q].res + (size_t)e * RES_STRIDE;
                const bool rb = sload(r + RES_ROLLBACK), rs = sload(r + RES_RESET);
                fast_rows = fast_rows && !rb;
                fast = fast && !rb && !rs && sload(r + RES_NADD) == 0;
            }
    }

    // a wave-tile: instance, table entry (scalar registers)
    struct Item {
        int e, li, g;   // instance, table entry, flat index (g0 + k·K)
        WtEntry w;
    };
    typedef int i32x8 __attribute__((ext_vector_type(8)));
    static_assert(sizeof(WtEntry) == sizeof(i32x8), "one scalar dwordx8 per entry");
    auto load_entry = [&](int li, WtEntry& w) __attribute__((always_inline)) {
        const i32x8 v = sload(reinterpret_cast<const i32x8*>(p.wt + li));
#pragma unroll
        for (int i = 0; i < WT_N; i++) w.tile[i] = v[i];
        w.valid = v[WT_N];
        w.rows[0] = v[WT_N + 1];
        w.rows[1] = v[WT_N + 2];
        w.rc = v[WT_N + 3];
    };
    // the wave's k-th wave-tile follows from the (k−1)-th by adding K to the flat index
    auto first_item = [&](Item& t) __attribute__((always_inline)) {
        t.e = g0 / nwt;
        const int li = g0 - t.e * nwt;
        load_entry(li, t.w);
        t.li = li;
        t.g = g0;
    };
    auto next_item = [&](const Item& c, Item& t) __attribute__((always_inline)) {
        int li = c.li + K, e = c.e;
        while (li >= nwt) {
            li -= nwt;
            e++;
        }
        t.e = e;
        load_entry(e < p.E ? li : 0, t.w);
        t.li = li;
        t.g = c.g + K;
    };
    auto tile_ptr = [&](const Item& t, int i) __attribute__((always_inline)) {
        return (size_t)t.e * inst_elems + (size_t)t.w.tile[i] * TILE_ELEMS;
    };
    // every slot is stored, the invalid ones (outside the packed triangle) to the sink tile: no
    // branch around a store (a conditional store splits the wait-count tracking, and the join
    // then waits for every outstanding load, the next wave-tile's prefetch included)
    auto store_tiles = [&](const Item& t, const f32x16 (&acc)[WT_N], bool skip = false) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < WT_N; i++) {
            TS* tl = ((t.w.valid >> i) & 1) && !skip ? Pout + tile_ptr(t, i) : sink;
#pragma unroll
            for (int qq = 0; qq < 4; qq++) tile_st(tl, lane, qq, acc[i]);
        }
    };
    auto op_row = [&](const Item& t, int side, int k) __attribute__((always_inline)) {
        return (t.w.rows[side] >> (16 * k)) & 0xffff;
    };
    // step q's operand rows (side 0: U, 1: V) from the contiguous slot buffers: scalar arithmetic
    // on a few kernel arguments, not 2·NS pointers (which the compiler reloaded from the kernel
    // arguments inside the loop, each load waited on before the next MFMA could issue)
    auto op_base = [&](int q, int side) __attribute__((always_inline)) {
        int sl = p.slot0 + q;
        if (sl >= p.nslots) sl -= p.nslots;
        return reinterpret_cast<const float*>(reinterpret_cast<const char*>(side || p.usym ? p.vbase : p.ubase) +
                                              (size_t)sl * (size_t)p.slot_bytes);
    };

    if constexpr (BF) {
        if (fast_rows) {
            // planes: BF16X6 hi, mid, lo bf16 (six products); F16X3 hi, lo fp16 of 2^σ·V (three)
            constexpr int NPL = F16 ? 2 : 3;
            typedef typename std::conditional<F16, f16x8r, bf16x8r>::type bf16x8;
            // operand ring depth (divides NS: a ring slot keeps its step index across wave-tiles).
            // F16: the deepest ring of at most F16_RDMAX step-sets, and the next wave-tile's tiles
            // issued RD − 1 steps before its start (late, below)
            constexpr int RD = F16 ? ring_depth(NS, F16_RDMAX) : (NS % 4 == 0 ? 4 : (NS % 3 == 0 ? 3 : 2));
            constexpr bool LATE = F16 && RD >= 3;
            // vmcnt retires in issue order, so every operand wait after the tile loads also waits for
            // them: issued at step TQ, the first such wait comes RD − 1 steps later, and so does
            // the next wave-tile's first use of them
            constexpr int TQ = NS - RD + 1;
            const size_t pstride = (size_t)d.nb * NPL * 64;   // 16-byte operands per instance
            // step q's planes: slot (slot0 + q) mod nslots
            auto pl_base = [&](int q) __attribute__((always_inline)) {
                int sl = p.slot0 + q;
                if (sl >= p.nslots) sl -= p.nslots;
                return reinterpret_cast<const bf16x8*>(reinterpret_cast<const char*>(p.bbase) +
                                                       (size_t)sl * (size_t)p.bslot_bytes);
            };
            // raw tile words in flight (fp16 storage: converted when the wave-tile starts)
            using Raw = typename std::conditional<HALF, f16x4, f32x4>::type;
            Raw pref[WT_N][4];
            f32x16 acc[WT_N];
            bf16x8 R[RD][WT_R + WT_C][NPL];
            // step q of wave-tile t into ring set r: A row blocks, then B row blocks, three planes
            auto load_ops = [&](int r, const Item& t, int q) __attribute__((always_inline)) {
                const bf16x8* b = pl_base(q) + t.e * pstride + lane;
#pragma unroll
                for (int i = 0; i < WT_R + WT_C; i++) {
                    const bf16x8* rb = b + (size_t)(i < WT_R ? op_row(t, 0, i) : op_row(t, 1, i - WT_R)) * NPL * 64;
#pragma unroll
                    for (int pl = 0; pl < NPL; pl++) R[r][i][pl] = rb[pl * 64];
                }
            };
            auto load_tiles = [&](const Item& t) __attribute__((always_inline)) {
#pragma unroll
                for (int i = 0; i < WT_N; i++) {
                    const Raw* tl = reinterpret_cast<const Raw*>(Pin + tile_ptr(t, i));
#pragma unroll
                    for (int qq = 0; qq < 4; qq++) pref[i][qq] = __builtin_nontemporal_load(tl + lane + qq * 64);
                }
            };
            // the accumulators hold −P: fp32 storage −X; fp16 storage −2^−x·X (X = fp16(2^x·P), the
            // instance's exponent; power-of-two scalings, exact), so that both operands are the
            // unscaled V planes; the store scales back and rounds to fp16 once per group. F16X3: the
            // planes of step q carry 2^σ_q·V, so during step q the accumulators hold −2^(2σ_q)·P (σ
            // changes only at a step that adds rows: the accumulators are rescaled after it)
            // per instance of the wave-tiles (uniform, few registers): the landmarks the group's steps
            // add [u_lo, u_hi), σ of the first and last step, the steps after which σ changes
            auto rec_of = [&](int e, int q, int w) __attribute__((always_inline)) {
                return sload(p.steps[q].res + (size_t)e * RES_STRIDE + w);
            };
            // A step that resets the map (Robot.cpp:893-904) zeroes the block: only the landmarks
            // added after the instance's last reset of the group are nonzero at its end, so the
            // union is taken over those steps and every other wave-tile of the instance is stored
            // as zero (rz); σ changes before that reset do not matter.
            int st_e = -1, u_lo = 0, u_hi = 0, sg0 = 0, sgl = 0, zl = 0;
            unsigned smask = 0;
            bool rz = false;
            auto load_steps = [&](int e) __attribute__((always_inline)) {
                u_lo = 0x7fffffff;
                u_hi = 0;
                smask = 0;
                rz = false;
                zl = 0;   // landmarks past every step's RES_ZMAX: zero V rows, no new rows
                int prev = 0;
#pragma unroll
                for (int q = 0; q < NS; q++) {
                    zl = max(zl, rec_of(e, q, RES_ZMAX));
                    if (rec_of(e, q, RES_RESET)) {   // (its own new rows are wiped with the map)
                        u_lo = 0x7fffffff;
                        u_hi = 0;
                        smask = 0;
                        rz = true;
                        continue;
                    }
                    const int na = rec_of(e, q, RES_NADD), s0 = rec_of(e, q, RES_SAVED_IN);
                    if (na > 0) {
                        u_lo = min(u_lo, s0);
                        u_hi = max(u_hi, s0 + na);
                    }
                    const int sg = F16 ? rec_of(e, q, RES_PSIG) : 0;
                    if (q == 0) sg0 = sg;
                    else if (sg != prev) smask |= 1u << (q - 1);
                    if (sg == PLANE_SIGMA_EXACT) smask |= 1u << NS;   // (the whole group exact)
                    prev = sg;
                }
                sgl = prev;
                st_e = e;
            };
            auto in_exp = [&](const Item& t) __attribute__((always_inline)) {
                int ex = 2 * sg0;
                if constexpr (HALF) ex -= sload(p.pexp + t.e);
                return ex;
            };
            auto touched = [&](const Item& t) __attribute__((always_inline)) {
                if (t.e != st_e) load_steps(t.e);
                const int ra = (t.w.rc & 0xffff) * WT_R * 16, ca = (t.w.rc >> 16) * WT_C * 16;   // landmarks
                return (u_lo < ra + WT_R * 16 && u_hi > ra) || (u_lo < ca + WT_C * 16 && u_hi > ca);
            };
            auto skip_of = [&](const Item& t) __attribute__((always_inline)) {
                const bool tc = touched(t);
                return tc || (!rz && smask != 0);
            };
            auto zero_of = [&](const Item& t) __attribute__((always_inline)) {
                const bool tc = touched(t);
                return rz && !tc;
            };
            // a wave-tile whose columns all lie past zl is unchanged by the group (its V-side rows
            // are zero in every step, and no step writes new rows there): not loaded, not stored
            // (a reset zeroes the block: no skipping then)
            auto dead = [&](const Item& t) __attribute__((always_inline)) {
                if (!p.zskip || t.e >= p.E) return false;
                if (t.e != st_e) load_steps(t.e);
                return !rz && (t.w.rc >> 16) * WT_C * 16 >= zl;
            };
            auto next_live = [&](const Item& c, Item& t) __attribute__((always_inline)) {
                next_item(c, t);
                while (t.g < g_end && dead(t)) {
                    const Item u = t;
                    next_item(u, t);
                }
            };
            Item cur, nxt, nxt2;
            bool any_skip = false;
            first_item(cur);
            while (cur.g < g_end && dead(cur)) {
                const Item u = cur;
                next_item(u, cur);
            }
            if (cur.g >= g_end) return;   // (no live wave-tile: nothing to store, no second pass)
            next_live(cur, nxt);
            load_tiles(cur);
            // (the first tiles ahead of every operand load, as in the loop: the wait count at the loop
            // head then covers the tiles without draining the previous wave-tile's stores)
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int q = 0; q < RD - 1; q++) load_ops(q, cur, q);
            while (true) {
                const bool more = nxt.g < g_end;
                next_live(nxt, nxt2);
                const Item ldi = more ? nxt : cur;   // the last wave-tile re-reads its own rows
                // a wave-tile holding a landmark some step of the group added, or of an instance whose
                // σ changes inside the group, is computed here but stored to the sink: the second pass
                // (below) runs it through the general loop
                const bool skip = skip_of(cur);
                const bool zero = zero_of(cur);   // (reset instance, untouched: stored as zero)
                any_skip |= skip;
                const int iex = in_exp(cur);
                const float isc = -ldexpf(1.0f, iex);
#pragma unroll
                for (int i = 0; i < WT_N; i++)
#pragma unroll
                    for (int qq = 0; qq < 4; qq++)
#pragma unroll
                        for (int j = 0; j < 4; j++) acc[i][4 * qq + j] = (float)pref[i][qq][j] * isc;
                if (!LATE && more) load_tiles(nxt);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int q = 0; q < NS; q++) {
                    if (LATE && q == TQ && more) load_tiles(nxt);
                    // ring set of step q + RD − 1 (this wave-tile's, else the next one's)
                    const int ql = q + RD - 1;
                    if (ql < NS) load_ops(ql % RD, cur, ql);
                    else load_ops(ql % RD, ldi, ql - NS);
                    const int r = q % RD;
                    if constexpr (F16) {
                        // (lo, hi), (hi, lo), (hi, hi): 12 MFMAs beside the 8 plane loads
#pragma unroll
                        for (int pp = 0; pp < 3; pp++) {
                            const int pa = pp == 0 ? 1 : 0, pb = pp == 1 ? 1 : 0;
#pragma unroll
                            for (int rr = 0; rr < WT_R; rr++)
#pragma unroll
                                for (int c = 0; c < WT_C; c++)
                                    acc[rr * WT_C + c] = __builtin_amdgcn_mfma_f32_32x32x16_f16(
                                        R[r][rr][pa], R[r][WT_R + c][pb], acc[rr * WT_C + c], 0, 0, 0);
                        }
#pragma unroll
                        for (int i = 0; i < 8; i++) {
                            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);   // MFMA
                            __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);   // VMEM read
                        }
                        __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
                    } else {
                        // part products smallest first: (mid, mid), (hi, lo), (lo, hi), (hi, mid),
                        // (mid, hi), (hi, hi)
#pragma unroll
                        for (int pp = 0; pp < 6; pp++) {
                            const int pa = (0x102010 >> (4 * (5 - pp))) & 0xf;
                            const int pb = (0x120100 >> (4 * (5 - pp))) & 0xf;
#pragma unroll
                            for (int rr = 0; rr < WT_R; rr++)
#pragma unroll
                                for (int c = 0; c < WT_C; c++)
                                    acc[rr * WT_C + c] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                                        R[r][rr][pa], R[r][WT_R + c][pb], acc[rr * WT_C + c], 0, 0, 0);
                        }
#pragma unroll
                        for (int i = 0; i < 12; i++) {
                            __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);   // MFMA
                            __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);   // VMEM read
                        }
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
                // back from the last step's domain (−1, −2^x, −2^(x − 2σ): an exact power of two, no
                // division), as whole-vector products (packed multiplies); a zeroed wave-tile (zero is
                // uniform) takes no multiply at all
                const float osc = -ldexpf(1.0f, -iex - (F16 ? 2 * (sgl - sg0) : 0));
                if (zero) {
#pragma unroll
                    for (int i = 0; i < WT_N; i++) acc[i] = f32x16{};
                } else {
#pragma unroll
                    for (int i = 0; i < WT_N; i++) acc[i] = acc[i] * osc;
                }
                store_tiles(cur, acc, skip);
                if (!more) break;
                cur = nxt;
                nxt = nxt2;
            }
            // second pass: the skipped wave-tiles through the general loop (their input tiles are
            // as read: the first pass stored them to the sink). Exact arithmetic on the fp32 operand
            // rows there, the split arithmetic elsewhere: both within the fp32 bar (slam_ekf.h)
            if (any_skip) {
                Item t;
                first_item(t);
                for (int gg = g0; gg < g_end; gg += K) {
                    if (gg != g0) {
                        Item nn;
                        next_item(t, nn);
                        t = nn;
                    }
                    if (!dead(t) && skip_of(t)) wt_general<TS, NS>(p, t.e, t.w, lane);
                }
            }
            return;
        }
    } else if (fast) {
        // raw tile words in flight (fp16 storage: converted when the wave-tile starts)
        using Raw = typename std::conditional<HALF, f16x4, f32x4>::type;
        Raw pref[WT_N][4];
        f32x4 opA[NS][WT_R][2], opB[NS][WT_C][2];
        f32x16 acc[WT_N];
        // half h (k-steps 4h..4h+3) of step q's operand rows of wave-tile t, into slot q
        auto load_half = [&](int slot, const Item& t, int q, int h) __attribute__((always_inline)) {
            const float* U = op_base(q, 0) + t.e * opstride + lofs + 4 * h;
            const float* V = op_base(q, 1) + t.e * opstride + lofs + 4 * h;
            const float us = us_of<TS>(p, t.e);
#pragma unroll
            for (int r = 0; r < WT_R; r++)
                opA[slot][r][h] = *reinterpret_cast<const f32x4*>(U + (size_t)op_row(t, 0, r) * 64 * kh) * us;
#pragma unroll
            for (int c = 0; c < WT_C; c++)
                opB[slot][c][h] = *reinterpret_cast<const f32x4*>(V + (size_t)op_row(t, 1, c) * 64 * kh);
        };
        auto load_tiles = [&](const Item& t) __attribute__((always_inline)) {
#pragma unroll
            for (int i = 0; i < WT_N; i++) {
                const Raw* tl = reinterpret_cast<const Raw*>(Pin + tile_ptr(t, i));
#pragma unroll
                for (int qq = 0; qq < 4; qq++) pref[i][qq] = __builtin_nontemporal_load(tl + lane + qq * 64);
            }
        };
        // k-steps 4h..4h+3 of step q. Every k-step runs: past the step's matches the scan kernel
        // leaves (−0)·(+0) operand products, and x + (−0) == x for every x (zeros, NaN, inf too)
        auto mfma_half = [&](int q, int h) __attribute__((always_inline)) {
#pragma unroll
            for (int s = 0; s < 4; s++)
#pragma unroll
                for (int r = 0; r < WT_R; r++)
#pragma unroll
                    for (int c = 0; c < WT_C; c++)
                        acc[r * WT_C + c] = __builtin_amdgcn_mfma_f32_32x32x2f32(
                            opA[q][r][h][s], opB[q][c][h][s], acc[r * WT_C + c], 0, 0, 0);
        };
        // one operand load after every group of four MFMAs (4 loads per half step)
        auto interleave = [&]() __attribute__((always_inline)) {
#pragma unroll
            for (int i = 0; i < 4; i++) {
                __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);   // MFMA
                __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);   // VMEM read
            }
        };
        Item cur, nxt, nxt2;
        first_item(cur);
        next_item(cur, nxt);
        load_tiles(cur);
#pragma unroll
        for (int q = 0; q < NS; q++) {
            load_half(q, cur, q, 0);
            load_half(q, cur, q, 1);
        }
        int g = g0;
        while (true) {
            const bool more = g + K < g_end;
            next_item(nxt, nxt2);   // read now, used by the next wave-tile
            // operand rows for the next wave-tile (the last one re-reads its own: no branch
            // splits the MFMA stream)
            const Item ldi = more ? nxt : cur;
#pragma unroll
            for (int i = 0; i < WT_N; i++)
#pragma unroll
                for (int qq = 0; qq < 4; qq++)
#pragma unroll
                    for (int j = 0; j < 4; j++) acc[i][4 * qq + j] = (float)pref[i][qq][j];
            // the next wave-tile's tiles first: the waits of this wave-tile only cover loads issued
            // during the one before it, so these have the whole wave-tile to land
            if (more) load_tiles(nxt);
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (AM) {
                // group-major steps (fp16 storage): the
                // per-step rounding of one group of accumulators runs on the VALU while the other
                // group's MFMAs run, so it leaves the MFMA stream. Per element the chain is
                // unchanged (k-ordered step q, then its rounding). Step q's operand registers are
                // refilled for the next wave-tile during step q+1's first group; the last step's
                // at the end. (Measured: one accumulator's 8 k-steps back to back, rounding the
                // previous accumulator beside them, ran 0.84 ms vs 0.79 for the step-major form.)
                // Pair-major form: group gi = accumulators (gi, 0) and (gi, 1) of the 2 × 2
                // wave-tile, their k-steps alternating (a dependent MFMA two issues later); the
                // previous group's 32 elements are rounded 2 per MFMA gap. The last step rounds
                // group 0 in the first half of group 1 and stores its tiles in the second half.
                auto mfma_grp = [&](int q, int gi, int pg, bool ld, int lq, bool last) __attribute__((always_inline)) {
#pragma unroll
                    for (int m = 0; m < 16; m++) {
                        const int s = m >> 1, c = m & 1, i = gi * WT_C + c;
                        acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(opA[q][gi][s >> 2][s & 3],
                                                                       opB[q][c][s >> 2][s & 3], acc[i], 0, 0, 0);
                        __builtin_amdgcn_sched_barrier(0);
                        if (pg >= 0 && !last) {
                            const int a = pg * WT_C + (m >> 3), k = 2 * (m & 7);
                            acc[a][k] = round_step<TS>(acc[a][k]);
                            acc[a][k + 1] = round_step<TS>(acc[a][k + 1]);
                        }
                        if (last) {
                            if (m < 8) {
                                const int a = pg * WT_C + (m >> 2), k = 4 * (m & 3);
#pragma unroll
                                for (int u = 0; u < 4; u++) acc[a][k + u] = round_step<TS>(acc[a][k + u]);
                            } else {
                                const int a = pg * WT_C + ((m - 8) >> 2), qq = (m - 8) & 3;
                                tile_st(((cur.w.valid >> a) & 1) ? Pout + tile_ptr(cur, a) : sink, lane, qq, acc[a]);
                            }
                        }
                        if (ld && (m & 1)) {
                            // load m/2 of slot lq: half, operand row (A rows, then B rows)
                            const int l = m >> 1, h = l >> 2, o = l & 3;
                            const bool isA = o < WT_R;
                            const float* base = op_base(lq, isA ? 0 : 1) + ldi.e * opstride + lofs + 4 * h;
                            const f32x4 v = *reinterpret_cast<const f32x4*>(
                                base + (size_t)op_row(ldi, isA ? 0 : 1, isA ? o : o - WT_R) * 64 * kh);
                            if (isA) opA[lq][o][h] = v * us_of<TS>(p, ldi.e);
                            else opB[lq][o - WT_R][h] = v;
                        }
                        __builtin_amdgcn_sched_barrier(0);
                    }
                };
                static_assert(WT_R == 2 && WT_C == 2, "pair-major form: two groups of two accumulators");
#pragma unroll
                for (int q = 0; q < NS; q++) {
                    mfma_grp(q, 0, q > 0 ? 1 : -1, q > 0, q > 0 ? q - 1 : 0, false);
                    mfma_grp(q, 1, 0, false, 0, q == NS - 1);
                }
#pragma unroll
                for (int a = 2; a < 4; a++)
#pragma unroll
                    for (int k = 0; k < 16; k++) acc[a][k] = round_step<TS>(acc[a][k]);
                load_half(NS - 1, ldi, NS - 1, 0);
                load_half(NS - 1, ldi, NS - 1, 1);
#pragma unroll
                for (int a = 2; a < 4; a++) {
                    TS* tl = ((cur.w.valid >> a) & 1) ? Pout + tile_ptr(cur, a) : sink;
#pragma unroll
                    for (int qq = 0; qq < 4; qq++) tile_st(tl, lane, qq, acc[a]);
                }
                if (!more) break;
                g += K;
                cur = nxt;
                nxt = nxt2;
                continue;
            }
#pragma unroll
            for (int q = 0; q < NS; q++) {
                // first half of step q, beside the second half of step q−1's rows for the next
                // wave-tile (their registers were last read by step q−1)
                mfma_half(q, 0);
                if (q > 0) {
                    load_half(q - 1, ldi, q - 1, 1);
                    interleave();
                }
                __builtin_amdgcn_sched_barrier(0);
                // second half, beside the first half of step q's rows for the next wave-tile
                mfma_half(q, 1);
#pragma unroll
                for (int i = 0; i < WT_N; i++) round_acc<TS>(acc[i]);
                load_half(q, ldi, q, 0);
                interleave();
                __builtin_amdgcn_sched_barrier(0);
            }
            load_half(NS - 1, ldi, NS - 1, 1);
            store_tiles(cur, acc);
            if (!more) break;
            g += K;
            cur = nxt;
            nxt = nxt2;
        }
        return;
    }

    // general loop: per wave-tile, every step in order with its operands loaded in place, then
    // the step's reset or rows (wt_general)
    Item t;
    first_item(t);
    for (int g = g0; g < g_end; g += K) {
        if (g != g0) {
            Item n;
            next_item(t, n);
            t = n;
        }
        wt_general<TS, NS>(p, t.e, t.w, lane);
    }
}

}  // namespace ekf
