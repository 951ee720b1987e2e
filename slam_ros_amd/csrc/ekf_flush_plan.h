// ekf_flush_plan.h — which flush kernel applies a group of steps: the one definition that the
// launch (launch_downdate), the padding of a partitioned context's odd group (enqueue_flush) and the
// reported kernel name (ekf_flush_kernel_name) all take. Host only (no HIP include).
#pragma once

#include <stdio.h>

#include "../../include/slam_ekf.h"
#include "ekf_tables.h"

namespace ekf {

constexpr int F64_WAVE_MAXS = 8;    // f64 wave flush: steps per launch
constexpr int F16X3_MAXS = 24;      // split-fp16 contexts: flush_interval <= 24
constexpr int BF16X6_MAXS = 16;     // split-bf16 flushes: steps per launch
constexpr int F32_WAVE_MAXS = 8;    // exact f32 wave flush: steps per launch
constexpr int PERSIST_MAXS = 4;     // flush_f32_persist2_kernel: steps per launch (its PST_MAXC)
constexpr int QUAD_MINS = 6;        // split-fp16 quad form: groups of 6-24 steps

// EKF_OPT_FLUSH_FORM (tests and measurements; the forms of one arithmetic are bit-identical)
enum FlushForm {
    FORM_AUTO = 0,
    FORM_SUPERTILE = 2,   // the super-tile (f32) / per-tile (f64) form for every group
    FORM_WAVE = 8,        // the exact f32 wave form also for 2 or 4 steps
    FORM_2X4 = 24,        // split arithmetics: wave-tiles of 2 × 4 tiles
    FORM_QUAD = 44,       // EKF_ARITH_F16X3: groups of 2 × 2 wave-tiles
};
inline bool flush_form_valid(int v)
{
    return v == FORM_AUTO || v == FORM_SUPERTILE || v == FORM_WAVE || v == FORM_2X4 || v == FORM_QUAD;
}

struct FlushKey {
    int precision;      // EKF_PREC_*
    int arith;          // the plane arithmetic that applies: 0 none, 1 EKF_ARITH_BF16X6, 2 EKF_ARITH_F16X3
    int form;           // FlushForm
    int nsteps;         // steps to apply
    int kmax;           // operand k columns (Dims::kmax)
    bool partitioned;   // ekf_shard_create: only the wave tables hold the rank's tile rows
    bool wt, wt64, wt24, wtq;   // the tables present (non-empty)
};

enum FlushFamily {
    FLUSH_F64_WAVE,      // flush_f64_wave_kernel<NS>
    FLUSH_F64_TILE,      // downdate_f64_kernel
    FLUSH_BF16_2X4,      // flush_bf24_kernel<T, NS>
    FLUSH_F16_2X4,       // flush_bf24_kernel<T, NS, true>
    FLUSH_F16_QUAD,      // flush_f16q_kernel<T, NS>
    FLUSH_F16_WAVE,      // flush_f32_wave_kernel<T, NS, true, true>
    FLUSH_BF16_WAVE,     // flush_f32_wave_kernel<T, NS, true>
    FLUSH_F32_WAVE,      // flush_f32_wave_kernel<T, NS>
    FLUSH_F32_PERSIST,   // flush_f32_persist2_kernel<T>
    FLUSH_F32_SUPERTILE, // flush_f32_sb_kernel<T>
    FLUSH_FAMILIES
};

enum FlushGrid {
    GRID_ONE_PER_CU,   // persistent: one workgroup per CU, whole XCDs
    GRID_TWO_PER_CU,   // persistent: two workgroups per CU (48 KB LDS each)
    GRID_SUPERTILES,   // one workgroup per super-tile of every instance, whole XCDs
    GRID_STRIDED,      // the context's grid-strided size (EKF_OPT_FLUSH_BLOCKS_PER_CU)
};

struct FlushPlan {
    FlushFamily family;
    int nsteps;       // steps the launch applies: the key's, plus a partitioned context's padding step
    int storage;      // EKF_PREC_* of the stored block (the kernels' first template argument)
    FlushGrid grid;
};

inline FlushPlan flush_plan(const FlushKey& k)
{
    // a partitioned fp32 context flushes with the wave form only (even groups): its odd group is
    // padded with a step that applies nothing
    const int ns = k.nsteps + ((k.partitioned && k.precision == EKF_PREC_F32 && (k.nsteps & 1)) ? 1 : 0);
    auto plan = [&](FlushFamily f, FlushGrid g) { return FlushPlan{f, ns, k.precision, g}; };
    if (k.precision == EKF_PREC_F64) {
        if (ns <= F64_WAVE_MAXS && k.kmax == 16 && k.wt64 && k.form != FORM_SUPERTILE)
            return plan(FLUSH_F64_WAVE, GRID_ONE_PER_CU);
        return plan(FLUSH_F64_TILE, GRID_STRIDED);
    }
    const bool even = ns >= 2 && ns % 2 == 0 && k.kmax <= 16 && k.wt;
    // split arithmetics: even groups of 2-16 (EKF_ARITH_BF16X6) or 2-24 (EKF_ARITH_F16X3) steps
    if (k.arith && even && ns <= (k.arith == EKF_ARITH_F16X3 ? F16X3_MAXS : BF16X6_MAXS)) {
        const bool f16 = k.arith == EKF_ARITH_F16X3;
        if (k.form == FORM_2X4 && k.wt24) return plan(f16 ? FLUSH_F16_2X4 : FLUSH_BF16_2X4, GRID_ONE_PER_CU);
        if (f16 && k.form == FORM_QUAD && ns >= QUAD_MINS && k.wtq) return plan(FLUSH_F16_QUAD, GRID_ONE_PER_CU);
        return plan(f16 ? FLUSH_F16_WAVE : FLUSH_BF16_WAVE, GRID_ONE_PER_CU);
    }
    // the exact wave flush: groups of 6 or 8 steps; FORM_WAVE forces it also for 2 or 4
    if (even && ns <= F32_WAVE_MAXS && (ns >= 6 || k.form == FORM_WAVE)) return plan(FLUSH_F32_WAVE, GRID_ONE_PER_CU);
    if (ns <= PERSIST_MAXS && k.kmax <= 16 && k.form != FORM_SUPERTILE) return plan(FLUSH_F32_PERSIST, GRID_TWO_PER_CU);
    return plan(FLUSH_F32_SUPERTILE, GRID_SUPERTILES);
}

// Workgroups of the plan's launch: ncu compute units, `strided` the context's grid-strided size, E
// instances of nb tile rows
inline unsigned flush_grid_size(FlushGrid g, int ncu, int strided, int E, int nb)
{
    switch (g) {
    case GRID_ONE_PER_CU: return (unsigned)(8 * ((ncu + 7) / 8));
    case GRID_TWO_PER_CU: return (unsigned)(16 * ((ncu + 7) / 8));
    case GRID_SUPERTILES: {
        const int64_t nsb = (nb + DD_SB - 1) / DD_SB;
        const int64_t total = (int64_t)E * (nsb * (nsb + 1) / 2);
        return (unsigned)(8 * ((total + 7) / 8));
    }
    default: return (unsigned)strided;
    }
}

// The kernel's name as the profiler spells it (bench.py and the tests match on these strings)
inline const char* flush_plan_name(const FlushPlan& p, char* buf, size_t n)
{
    const char* ty = p.storage == EKF_PREC_F16 ? "_Float16" : "float";
    switch (p.family) {
    case FLUSH_F64_WAVE: snprintf(buf, n, "flush_f64_wave_kernel<%d>", p.nsteps); break;
    case FLUSH_F64_TILE: snprintf(buf, n, "downdate_f64_kernel"); break;
    case FLUSH_BF16_2X4: snprintf(buf, n, "flush_bf24_kernel<%s, %d>", ty, p.nsteps); break;
    case FLUSH_F16_2X4: snprintf(buf, n, "flush_bf24_kernel<%s, %d, true>", ty, p.nsteps); break;
    case FLUSH_F16_QUAD: snprintf(buf, n, "flush_f16q_kernel<%s, %d>", ty, p.nsteps); break;
    case FLUSH_F16_WAVE: snprintf(buf, n, "flush_f32_wave_kernel<%s, %d, true, true>", ty, p.nsteps); break;
    case FLUSH_BF16_WAVE: snprintf(buf, n, "flush_f32_wave_kernel<%s, %d, true>", ty, p.nsteps); break;
    case FLUSH_F32_WAVE: snprintf(buf, n, "flush_f32_wave_kernel<%s, %d>", ty, p.nsteps); break;
    case FLUSH_F32_PERSIST: snprintf(buf, n, "flush_f32_persist2_kernel<%s>", ty); break;
    case FLUSH_F32_SUPERTILE: snprintf(buf, n, "flush_f32_sb_kernel<%s>", ty); break;
    default: snprintf(buf, n, "%s", ""); break;
    }
    return buf;
}

}  // namespace ekf
