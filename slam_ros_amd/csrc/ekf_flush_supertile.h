// ekf_flush_supertile.h — the exact fp32 flush on LDS-staged super-tiles: flush_f32_sb_kernel and
// the persistent two-workgroups-per-CU form for short groups.
#pragma once

#include "ekf_flush_common.h"

// (contraction: free, as in every flush header; the products that matter are MFMA chains)
#pragma clang fp contract(fast)

namespace ekf {

// f32 flush on super-tiles: a workgroup owns DD_SB × DD_SB tiles (wave w: tile row
// sbi·DD_SB + w, tile columns sbj·DD_SB + 0..3), keeps their 4 accumulators in registers for
// the whole group of steps and stages each step's operands for the DD_SB row blocks and DD_SB
// column blocks through LDS in chunks of 8 MFMA k-steps (double-buffered, one barrier per
// chunk, next chunk prefetched into registers while the current one runs). Operand traffic
// per tile and k-step falls from 512 B to 128 B; the MFMA chain per element is unchanged
// (k-ordered within a step, steps in order), so results are bit-identical to the per-tile form.
namespace {
struct SbStep {
    int reset, ks, nadd, s0;
};

__device__ __forceinline__ SbStep sb_step(const DowndateParams& p, int q, int e)
{
    const int* r = p.steps[q].res + (size_t)e * RES_STRIDE;
    SbStep s;
    s.reset = r[RES_RESET];
    s.ks = s.reset ? 0 : r[RES_KSTEPS];
    s.nadd = r[RES_NADD];
    s.s0 = r[RES_SAVED_IN];
    return s;
}
}  // namespace

template <typename TS>
__global__ __launch_bounds__(DD_THREADS) void flush_f32_sb_kernel(DowndateParams p)
{
    const Dims d = p.d;
    const int nsb = (d.nb + DD_SB - 1) / DD_SB;
    const int64_t nst = (int64_t)nsb * (nsb + 1) / 2;
    const int64_t total = (int64_t)p.E * nst;
    // XCD-aware order: the hardware deals workgroup b to XCD b mod 8; give every XCD a
    // contiguous range of (instance, super-tile) so that its L2 holds one instance's operands
    const int64_t per = (total + 7) / 8;
    const int64_t g = (int64_t)(blockIdx.x & 7) * per + (blockIdx.x >> 3);
    if (g >= total) return;
    const int e = (int)(g / nst);
    const int2 sb = p.stile_rc[g - (int64_t)e * nst];
    const int lane = threadIdx.x & 63;
    const int w = threadIdx.x >> 6;
    const int bi = sb.x * DD_SB + w;
    const int kh = d.kmax / 2;
    const size_t opstride = (size_t)d.nb * 64 * kh;

    // does any step change this super-tile? (uniform)
    bool work = false;
    for (int q = 0; q < p.nsteps; q++) {
        const SbStep s = sb_step(p, q, e);
        work |= s.reset || s.ks > 0 ||
                (s.nadd > 0 && (sb.y + 1) * DD_SB * 16 > s.s0 && sb.y * DD_SB * 16 < s.s0 + s.nadd);
    }
    bool valid[DD_SB];
    size_t toff[DD_SB];
    int vmask = 0;
#pragma unroll
    for (int c = 0; c < DD_SB; c++) {
        const int bj = sb.y * DD_SB + c;
        valid[c] = bi < d.nb && bj < d.nb && bi <= bj;
        vmask |= valid[c] << c;
        toff[c] = valid[c] ? ((size_t)e * d.ntiles + tile_index(bi, bj, d.nb)) * TILE_ELEMS : 0;
    }
    const TS* Pin = reinterpret_cast<const TS*>(p.Pin);
    TS* Pout = reinterpret_cast<TS*>(p.Pout);
    if (!work) {
        if (p.Pin != p.Pout) {
#pragma unroll
            for (int c = 0; c < DD_SB; c++)
                if (valid[c]) {
                    f32x16 t;
#pragma unroll
                    for (int qq = 0; qq < 4; qq++) {
                        const f32x4 v = tile_ld(Pin + toff[c], lane, qq);
                        t[4 * qq + 0] = v[0]; t[4 * qq + 1] = v[1]; t[4 * qq + 2] = v[2]; t[4 * qq + 3] = v[3];
                    }
#pragma unroll
                    for (int qq = 0; qq < 4; qq++) tile_st(Pout + toff[c], lane, qq, t);
                }
        }
        return;
    }
    f32x16 acc[DD_SB];
#pragma unroll
    for (int c = 0; c < DD_SB; c++) {
        if (valid[c]) {
#pragma unroll
            for (int qq = 0; qq < 4; qq++) {
                const f32x4 v = tile_ld(Pin + toff[c], lane, qq);
                acc[c][4 * qq + 0] = v[0];
                acc[c][4 * qq + 1] = v[1];
                acc[c][4 * qq + 2] = v[2];
                acc[c][4 * qq + 3] = v[3];
            }
        } else {
#pragma unroll
            for (int k = 0; k < 16; k++) acc[c][k] = 0.f;
        }
    }

    // [buf][A/B][block][s4][lane] float4: 2 × 2 × 4 × 2 × 64 × 16 B = 32 KB
    __shared__ f32x4 lds[2][2][DD_SB][2][64];
    // staging: thread t moves float4 i = t + 256 j (j < 4): lane, s4, block, A/B
    const float us = us_of<TS>(p, e);
    auto fetch = [&](int q, int k0, f32x4 reg[4]) {
        const float* U = u_rows_flush(p, p.steps[q], e, opstride);
        const float* V = reinterpret_cast<const float*>(p.steps[q].Vop) + e * opstride;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int i = threadIdx.x + 256 * j;
            const int ln = i & 63, s4 = (i >> 6) & 1, blk = (i >> 7) & 3, ab = i >> 9;
            const int rb = (ab ? sb.y : sb.x) * DD_SB + blk;
            if (rb < d.nb) {
                const float* src = (ab ? V : U) + ((size_t)rb * 64 + ln) * kh + k0 + 4 * s4;
                reg[j] = *reinterpret_cast<const f32x4*>(src) * (ab ? 1.0f : us);
            }
        }
    };
    auto stage = [&](int buf, const f32x4 reg[4]) {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int i = threadIdx.x + 256 * j;
            const int ln = i & 63, s4 = (i >> 6) & 1, blk = (i >> 7) & 3, ab = i >> 9;
            lds[buf][ab][blk][s4][ln] = reg[j];
        }
    };
    // reset or augmented rows of step q, after its downdate
    auto post = [&](int q) {
        const SbStep s = sb_step(p, q, e);
        if (s.reset) {
#pragma unroll
            for (int c = 0; c < DD_SB; c++)
#pragma unroll
                for (int k = 0; k < 16; k++) acc[c][k] = 0.f;
            return;
        }
        if (s.nadd <= 0) return;
        const double* prw0 = p.steps[q].patch + (size_t)e * d.max_lines * 2 * d.M;
        const double* pdg = p.steps[q].patch_diag + (size_t)e * d.max_lines * 4;
        // one tile at a time through acc[0], rotating the four accumulators (rare path: keeps
        // a single copy of the per-element code and its registers)
#pragma nounroll
        for (int c = 0; c < DD_SB; c++) {
            const int bj = sb.y * DD_SB + c;
            if (((vmask >> c) & 1) && bj * 16 + 15 >= s.s0 && bj * 16 < s.s0 + s.nadd) {
                const int col = bj * 32 + (lane & 31);
#pragma unroll
                for (int k = 0; k < 16; k++) {
                    const int row = bi * 32 + (k & 3) + 8 * (k >> 2) + 4 * (lane >> 5);
                    const int hi = max(row >> 1, col >> 1);
                    if (hi >= s.s0 && hi < s.s0 + s.nadd)
                        acc[0][k] = round_step<TS>(to_domain<TS>(patched_value(prw0, pdg, d.M, s.s0, row, col), storage_exp<TS>(p.pexp, e)));
                }
            }
            const f32x16 t0 = acc[0];
            acc[0] = acc[1];
            acc[1] = acc[2];
            acc[2] = acc[3];
            acc[3] = t0;
        }
    };
    // first chunk at or after step q (k0 = 0): steps without a downdate are passed through post
    auto first_mfma = [&](int q) {
        while (q < p.nsteps && sb_step(p, q, e).ks == 0) q++;
        return q;
    };

    int q = first_mfma(0);
    for (int t = 0; t < q; t++) post(t);
    int k0 = 0, buf = 0;
    f32x4 reg[4];
    if (q < p.nsteps) fetch(q, 0, reg);
    while (q < p.nsteps) {
        const int ks = sb_step(p, q, e).ks;
        const int kc = min(SBK, ks - k0);
        stage(buf, reg);
        __syncthreads();
        // next chunk
        int qn = q, kn = k0 + SBK;
        if (kn >= ks) {
            qn = first_mfma(q + 1);
            kn = 0;
        }
        if (qn < p.nsteps) fetch(qn, kn, reg);
        const f32x4 a0 = lds[buf][0][w][0][lane];
        const f32x4 a1 = lds[buf][0][w][1][lane];
        f32x4 b0[DD_SB], b1[DD_SB];
#pragma unroll
        for (int c = 0; c < DD_SB; c++) {
            b0[c] = lds[buf][1][c][0][lane];
            b1[c] = lds[buf][1][c][1][lane];
        }
        {
#pragma unroll
            for (int s = 0; s < SBK; s++)
                if (s < kc) {
#pragma unroll
                    for (int c = 0; c < DD_SB; c++)
                        acc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(s < 4 ? a0[s & 3] : a1[s & 3],
                                                                      s < 4 ? b0[c][s & 3] : b1[c][s & 3],
                                                                      acc[c], 0, 0, 0);
                }
        }
        if (qn != q) {
#pragma unroll
            for (int c = 0; c < DD_SB; c++) round_acc<TS>(acc[c]);
            for (int t = q; t < qn && t < p.nsteps; t++) post(t);
        }
        q = qn;
        k0 = kn;
        buf ^= 1;
    }
#pragma unroll
    for (int c = 0; c < DD_SB; c++)
        if (valid[c]) {
#pragma unroll
            for (int qq = 0; qq < 4; qq++) tile_st(Pout + toff[c], lane, qq, acc[c]);
        }
}

// Groups of at most PST_MAXC steps with kmax <= 16 (one operand chunk per step) run the
// persistent form below; otherwise flush_f32_sb_kernel runs.
constexpr int PST_MAXC = 4;
static_assert(PERSIST_MAXS == PST_MAXC, "flush_plan's bound of flush_f32_persist2_kernel");

// f32/f16 flush, persistent 2-workgroups-per-CU form: super-tiles of 4 × 2 tiles (wave w: tile
// row sbi·4 + w, tile columns sbj·2 + 0..1), two accumulators per wave, single-buffered LDS
// operands (48 KB: 4 A blocks + 2 B blocks per chunk), two barriers per super-tile. Two
// independent workgroups per CU (≤ 256 registers per wave) let one workgroup's MFMA chains run
// while the other stages, waits or streams. Per super-tile the control is four scalar words
// (instance, super-tile, packed step flags); when every step of the group is a full 8-k-step
// downdate with nothing else to apply (the steady state) the MFMA block runs without predicates.
constexpr int P2_C = 2;   // tile columns per super-tile

struct P2Info {
    int e, sbi, sbj;
    int flags;   // per step q, byte q: bits 0-3 ks, bit 4 reset, bit 5 augmented rows present
};

template <typename TS>
__global__ __launch_bounds__(DD_THREADS, 2) void flush_f32_persist2_kernel(DowndateParams p)
{
    const Dims d = p.d;
    const int nst = p.nstiles2;
    const int total = p.E * nst;
    const int per = (total + 7) / 8;
    const int xcd = blockIdx.x & 7;
    const int wpx = gridDim.x >> 3;
    const int g_end = min(total, (xcd + 1) * per);
    int g = xcd * per + (blockIdx.x >> 3);
    if (g >= g_end) return;

    const int lane = threadIdx.x & 63;
    const int w = threadIdx.x >> 6;
    const int kh = d.kmax / 2;
    const size_t opstride = (size_t)d.nb * 64 * kh;
    const TS* Pin = reinterpret_cast<const TS*>(p.Pin);
    TS* Pout = reinterpret_cast<TS*>(p.Pout);
    const int nsteps = p.nsteps;
    // this thread's staging slots j < 3 of a chunk: float4 i = tid + 256 j of
    // [A: 4 blocks × 2 × 64 | B: 2 blocks × 2 × 64]; offsets inside a block row are invariant
    const int ln = threadIdx.x & 63, s4 = (threadIdx.x >> 6) & 1, bl = threadIdx.x >> 7;
    const int in_blk = ln * kh + 4 * s4;

    auto load_flags = [&](P2Info& t) {
        int f = 0;
#pragma unroll
        for (int q = 0; q < PST_MAXC; q++) {
            if (q < nsteps) {
                const int* r = p.steps[q].res + (size_t)t.e * RES_STRIDE;
                const int reset = sload(r + RES_RESET);
                const int ks = reset ? 0 : sload(r + RES_KSTEPS);
                const int nadd = sload(r + RES_NADD);
                f |= ((ks & 15) | (reset ? 16 : 0) | (nadd > 0 ? 32 : 0)) << (8 * q);
            }
        }
        t.flags = f;
    };
    auto locate = [&](int li, P2Info& t) {
        const int* rc = reinterpret_cast<const int*>(p.stile2_rc + li);
        t.sbi = sload(rc);
        t.sbj = sload(rc + 1);
    };
    auto tile_off = [&](const P2Info& t, int c, bool& valid) {
        const int bi = t.sbi * DD_SB + w, bj = t.sbj * P2_C + c;
        valid = bi < d.nb && bj < d.nb && bi <= bj;
        return valid ? ((size_t)t.e * d.ntiles + tile_index(bi, bj, d.nb)) * TILE_ELEMS : (size_t)0;
    };
    auto fetch = [&](const P2Info& t, f32x4 opreg[PST_MAXC][3], f32x4 pref[P2_C][4]) {
        const int rA0 = min(t.sbi * DD_SB + bl, d.nb - 1), rA1 = min(t.sbi * DD_SB + 2 + bl, d.nb - 1);
        const int rB = min(t.sbj * P2_C + bl, d.nb - 1);   // rows past the block: unused
#pragma unroll
        for (int c = 0; c < PST_MAXC; c++) {
            const int qc = ((t.flags >> (8 * c)) & 15) ? c : 0;   // absent steps re-read step 0
            const float* U = u_rows_flush(p, p.steps[qc], t.e, opstride);
            const float* V = reinterpret_cast<const float*>(p.steps[qc].Vop) + t.e * opstride;
            const float us = us_of<TS>(p, t.e);
            opreg[c][0] = *reinterpret_cast<const f32x4*>(U + (size_t)rA0 * 64 * kh + in_blk) * us;
            opreg[c][1] = *reinterpret_cast<const f32x4*>(U + (size_t)rA1 * 64 * kh + in_blk) * us;
            opreg[c][2] = *reinterpret_cast<const f32x4*>(V + (size_t)rB * 64 * kh + in_blk);
        }
#pragma unroll
        for (int c = 0; c < P2_C; c++) {
            bool v;
            const TS* tl = Pin + tile_off(t, c, v);
#pragma unroll
            for (int qq = 0; qq < 4; qq++) pref[c][qq] = tile_ld(tl, lane, qq);
        }
    };
    __shared__ f32x4 ldsA[PST_MAXC][DD_SB][2][64];   // 32 KB
    __shared__ f32x4 ldsB[PST_MAXC][P2_C][2][64];    // 16 KB
    P2Info cur;
    cur.e = __builtin_amdgcn_readfirstlane(g / nst);
    int li = __builtin_amdgcn_readfirstlane(g - cur.e * nst);
    locate(li, cur);
    load_flags(cur);
    f32x4 opreg[PST_MAXC][3];
    f32x4 pref[P2_C][4];
    fetch(cur, opreg, pref);
    f32x16 acc[P2_C];
    // steady state: every step of the group a full chunk, no reset, no augmented rows
    int steady = 0;
#pragma unroll
    for (int q = 0; q < PST_MAXC; q++) steady |= (q < nsteps ? SBK : 0) << (8 * q);

    while (true) {
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");   // LDS free
#pragma unroll
        for (int c = 0; c < PST_MAXC; c++) {
            if ((cur.flags >> (8 * c)) & 15) {
                ldsA[c][bl][s4][ln] = opreg[c][0];
                ldsA[c][2 + bl][s4][ln] = opreg[c][1];
                ldsB[c][bl][s4][ln] = opreg[c][2];
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");   // LDS written
#pragma unroll
        for (int c = 0; c < P2_C; c++)
#pragma unroll
            for (int qq = 0; qq < 4; qq++) {
                acc[c][4 * qq + 0] = pref[c][qq][0];
                acc[c][4 * qq + 1] = pref[c][qq][1];
                acc[c][4 * qq + 2] = pref[c][qq][2];
                acc[c][4 * qq + 3] = pref[c][qq][3];
            }
        // next super-tile in flight (the last iteration re-reads its own)
        const int gn = g + wpx;
        const bool more = gn < g_end;
        P2Info nxt;
        nxt.e = cur.e;
        int lin = li;
        if (more) {
            lin += wpx;
            while (lin >= nst) {
                lin -= nst;
                nxt.e++;
            }
        }
        locate(lin, nxt);
        load_flags(nxt);
        fetch(nxt, opreg, pref);

        const int e = cur.e;
        const int bi = cur.sbi * DD_SB + w;
        if (cur.flags == steady) {
            __builtin_amdgcn_s_setprio(1);   // this MFMA cluster ahead of the partner's staging
#pragma unroll
            for (int q = 0; q < PST_MAXC; q++) {
                if (q < nsteps) {
                    const f32x4 a0 = ldsA[q][w][0][lane];
                    const f32x4 a1 = ldsA[q][w][1][lane];
                    const f32x4 b00 = ldsB[q][0][0][lane], b01 = ldsB[q][0][1][lane];
                    const f32x4 b10 = ldsB[q][1][0][lane], b11 = ldsB[q][1][1][lane];
#pragma unroll
                    for (int s = 0; s < 4; s++) {
                        acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[s], b00[s], acc[0], 0, 0, 0);
                        acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[s], b10[s], acc[1], 0, 0, 0);
                    }
#pragma unroll
                    for (int s = 0; s < 4; s++) {
                        acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[s], b01[s], acc[0], 0, 0, 0);
                        acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[s], b11[s], acc[1], 0, 0, 0);
                    }
                    round_acc<TS>(acc[0]);
                    round_acc<TS>(acc[1]);
                }
            }
            __builtin_amdgcn_s_setprio(0);
        } else {
            int vmask = 0;
#pragma unroll
            for (int c = 0; c < P2_C; c++) {
                bool v;
                (void)tile_off(cur, c, v);
                vmask |= (int)v << c;
            }
            auto post = [&](int q) {
                const int fq = (cur.flags >> (8 * q)) & 255;
                if (fq & 16) {
#pragma unroll
                    for (int c = 0; c < P2_C; c++)
#pragma unroll
                        for (int k = 0; k < 16; k++) acc[c][k] = 0.f;
                    return;
                }
                if (!(fq & 32)) return;
                const int* r = p.steps[q].res + (size_t)e * RES_STRIDE;
                const int nadd = sload(r + RES_NADD), s0 = sload(r + RES_SAVED_IN);
                if ((cur.sbj + 1) * P2_C * 16 <= s0 || cur.sbj * P2_C * 16 >= s0 + nadd) return;
                const double* prw0 = p.steps[q].patch + (size_t)e * d.max_lines * 2 * d.M;
                const double* pdg = p.steps[q].patch_diag + (size_t)e * d.max_lines * 4;
                const int ex = storage_exp<TS>(p.pexp, e);
#pragma nounroll
                for (int c = 0; c < P2_C; c++) {
                    const int bj = cur.sbj * P2_C + c;
                    if (((vmask >> c) & 1) && bj * 16 + 15 >= s0 && bj * 16 < s0 + nadd) {
                        const int col = bj * 32 + (lane & 31);
#pragma unroll
                        for (int k = 0; k < 16; k++) {
                            const int row = bi * 32 + (k & 3) + 8 * (k >> 2) + 4 * (lane >> 5);
                            const int hi = max(row >> 1, col >> 1);
                            if (hi >= s0 && hi < s0 + nadd)
                                acc[0][k] = round_step<TS>(to_domain<TS>(patched_value(prw0, pdg, d.M, s0, row, col), ex));
                        }
                    }
                    const f32x16 t0 = acc[0];
                    acc[0] = acc[1];
                    acc[1] = t0;
                }
            };
#pragma unroll
            for (int q = 0; q < PST_MAXC; q++) {
                if (q >= nsteps) break;
                const int kc = (cur.flags >> (8 * q)) & 15;
                if (kc > 0) {
                    const f32x4 a0 = ldsA[q][w][0][lane];
                    const f32x4 a1 = ldsA[q][w][1][lane];
                    f32x4 b0[P2_C], b1[P2_C];
#pragma unroll
                    for (int cc = 0; cc < P2_C; cc++) {
                        b0[cc] = ldsB[q][cc][0][lane];
                        b1[cc] = ldsB[q][cc][1][lane];
                    }
#pragma unroll
                    for (int s = 0; s < SBK; s++)
                        if (s < kc) {
#pragma unroll
                            for (int cc = 0; cc < P2_C; cc++)
                                acc[cc] = __builtin_amdgcn_mfma_f32_32x32x2f32(s < 4 ? a0[s & 3] : a1[s & 3],
                                                                               s < 4 ? b0[cc][s & 3] : b1[cc][s & 3],
                                                                               acc[cc], 0, 0, 0);
                        }
#pragma unroll
                    for (int cc = 0; cc < P2_C; cc++) round_acc<TS>(acc[cc]);
                }
                post(q);
            }
        }
#pragma unroll
        for (int c = 0; c < P2_C; c++) {
            bool v;
            const size_t off = tile_off(cur, c, v);
            if (v) {
#pragma unroll
                for (int qq = 0; qq < 4; qq++) tile_st(Pout + off, lane, qq, acc[c]);
            }
        }
        if (!more) break;
        g = gn;
        li = lin;
        cur = nxt;
    }
}

}  // namespace ekf
