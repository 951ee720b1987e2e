// ekf_shard_kernels.h — the kernels of one instance whose landmark block is partitioned over ranks
// (ShardParams): shard_kernel, one phase of the scan over every landmark, and
// shard_spec_kernel, the speculative path's lines in one launch. Every expression is the scan kernel's
// (the inline functions of ekf_assoc_parts.h and ekf_gate.h in this contract(on) region), and every
// body that more than one phase or kernel needs has one definition here, so that the protocols are
// bit-identical to one another and to a single context. Only unit_shard_pack.hip includes this file.
#pragma once

#include "ekf_assoc_parts.h"
#include "ekf_gate.h"

// The association arithmetic contracts a·b + c only within one source expression, so a
// function inlined into different kernels or phases rounds identically everywhere (the
// speculative and sequential association paths must agree bit for bit).
#pragma clang fp contract(on)

namespace ekf {

// ---------------------------------------------------------------------------------------
// One instance with its landmark block partitioned over ranks (ShardParams): the
// scan kernel's sequential association path phase by phase over every landmark, one thread per
// landmark, so that a sharded run is bit-identical to a single-context one. Between phases the
// caller sums the [N][4] exchange buffer over the ranks (each fills the blocks its tiles hold).
// Predict (Robot.cpp:130-286) as the scan kernel's init_state: F3, x_pre and the 3×3 block
__device__ __forceinline__ void shard_predict(const double pose[3], const double enc[3], double enc_noise,
                                              double F3[9], double R33[9], double xp[3])
{
    const double x0 = pose[0], y0 = pose[1], t0 = pose[2];
    const double u2 = t0 - enc[2];
    const double dx = x0 - enc[0], dy = y0 - enc[1];
    const double u0 = sqrt(dx * dx + dy * dy);
    const double c = u2 / 2.0 + t0;
    double sc, cc;
    sincos(c, &sc, &cc);
    F3[2] = -u0 * sc;
    F3[5] = u0 * cc;
    xp[0] = x0 + u0 * cc;
    xp[1] = y0 + u0 * sc;
    xp[2] = t0 + u2;
    const double Fu3[9] = {cc, 0, -u0 * sc / 2.0, sc, 1, u0 * cc / 2.0, 0, 0, 1};
    const double qs = (-1.0 / (1 + fabs(u0)) + 1);
    const double Q[9] = {enc_noise * qs, 0, 0, 0, 2 * enc_noise * qs, 0, 0, 0, enc_noise * qs};
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
}

// ---- the replicated state of the running scan: one accessor each ----
// The robot block of the running scan (ShardParams::rob, ROB_WORDS doubles; the same layout in
// shard_spec_kernel's LDS copies): the 3×3 block, then x_pre
constexpr int ROB_WORDS = 12;
struct RobotBlock {
    double R33[9], xp[3];
};
__device__ __forceinline__ void rob_load(const double* rob, RobotBlock& rb)
{
#pragma unroll
    for (int a = 0; a < 9; a++) rb.R33[a] = rob[a];
    rb.xp[0] = rob[9]; rb.xp[1] = rob[10]; rb.xp[2] = rob[11];
}
__device__ __forceinline__ void rob_store(double* rob, const RobotBlock& rb)
{
#pragma unroll
    for (int a = 0; a < 9; a++) rob[a] = rb.R33[a];
    rob[9] = rb.xp[0]; rob[10] = rb.xp[1]; rob[11] = rb.xp[2];
}

// A landmark's record (ShardParams::rec, SH_REC doubles). The 12 running words — its robot-strip
// columns, its mean and its diagonal block — are rewritten by every line applied to it; the scan-start
// words — its angle at the scan's start with its sine and cosine in fp64 (sincos_near) and in fp32
// (quick_reject) — are written once, by SH_BEGIN.
enum { REC_RR0 = 0, REC_RR1 = 2, REC_RR2 = 4, REC_YB = 6, REC_DJ = 8, REC_RUNNING = 12,
       REC_MA0 = 12, REC_S0J = 13, REC_C0J = 14, REC_S0F = 15, REC_C0F = 16, REC_USED = 17 };
struct LmState {
    double2 rr0, rr1, rr2, yb;
    double Dj[4];
};
struct LmStart {
    double ma0, s0j, c0j, s0f, c0f;
};
// (own = false: zeros, for a thread without a landmark)
__device__ __forceinline__ void rec_load(const double* rc, bool own, LmState& lm)
{
    double v[REC_RUNNING];
#pragma unroll
    for (int k = 0; k < REC_RUNNING; k++) v[k] = own ? rc[k] : 0.0;
    lm.rr0 = make_double2(v[REC_RR0], v[REC_RR0 + 1]);
    lm.rr1 = make_double2(v[REC_RR1], v[REC_RR1 + 1]);
    lm.rr2 = make_double2(v[REC_RR2], v[REC_RR2 + 1]);
    lm.yb = make_double2(v[REC_YB], v[REC_YB + 1]);
#pragma unroll
    for (int k = 0; k < 4; k++) lm.Dj[k] = v[REC_DJ + k];
}
__device__ __forceinline__ void rec_load_start(const double* rc, bool own, LmStart& s0)
{
    s0.ma0 = own ? rc[REC_MA0] : 0.0;
    s0.s0j = own ? rc[REC_S0J] : 0.0;
    s0.c0j = own ? rc[REC_C0J] : 0.0;
    s0.s0f = own ? rc[REC_S0F] : 0.0;
    s0.c0f = own ? rc[REC_C0F] : 0.0;
}
__device__ __forceinline__ void rec_store(double* rc, const LmState& lm)
{
    rc[REC_RR0] = lm.rr0.x; rc[REC_RR0 + 1] = lm.rr0.y;
    rc[REC_RR1] = lm.rr1.x; rc[REC_RR1 + 1] = lm.rr1.y;
    rc[REC_RR2] = lm.rr2.x; rc[REC_RR2 + 1] = lm.rr2.y;
    rc[REC_YB] = lm.yb.x; rc[REC_YB + 1] = lm.yb.y;
#pragma unroll
    for (int k = 0; k < 4; k++) rc[REC_DJ + k] = lm.Dj[k];
}
// (SH_BEGIN alone: the whole record, its spare words zero)
__device__ __forceinline__ void rec_store_all(double* rc, const LmState& lm, const LmStart& s0)
{
    rec_store(rc, lm);
    rc[REC_MA0] = s0.ma0;
    rc[REC_S0J] = s0.s0j; rc[REC_C0J] = s0.c0j;
    rc[REC_S0F] = s0.s0f; rc[REC_C0F] = s0.c0f;
#pragma unroll
    for (int k = REC_USED; k < SH_REC; k++) rc[k] = 0.0;
}

// A landmark's history rows of the scan (ShardParams::hist, [max_lines][8] per landmark; the same
// layout in the replay wave's LDS copy): match q's U rows (4), then its V rows (4)
__device__ __forceinline__ void hist_row_store(double* row, const double uu[4], const double kk[4])
{
#pragma unroll
    for (int k = 0; k < 4; k++) {
        row[k] = uu[k];
        row[4 + k] = kk[k];
    }
}
// The winner's V rows of the m earlier matches behind build_package's words (Robot.cpp:560-568: every
// landmark corrects its block of the winner's column with them)
__device__ __forceinline__ void package_v_rows(const double* rows, int m, double* pk)
{
    for (int q = 0; q < m; q++)
#pragma unroll
        for (int k = 0; k < 4; k++) pk[MB_VH + 4 * q + k] = rows[8 * q + 4 + k];
}
// gain_rows' vq_of on such a package
struct PackageV {
    const double* pk;
    __device__ __forceinline__ double4 operator()(int q) const
    {
        const double* vh = pk + MB_VH + 4 * q;
        return make_double4(vh[0], vh[1], vh[2], vh[3]);
    }
};

// block (j, w) of the landmark block is this rank's if the tile that stores it is
__device__ __forceinline__ bool shard_local_blk(const ShardParams& p, int ja, int wb)
{
    const int ba = (2 * ja) >> 5, bb = (2 * wb) >> 5;
    const long long t = tile_index(ba < bb ? ba : bb, ba < bb ? bb : ba, p.d.nb);
    return t >= p.t0 && t < p.t1;
}

// The gate of one landmark for line `line` at the robot state rb, exactly as the sequential path
// (Robot.cpp:313-498): the two certified reject filters, then the exact evaluation (c is set only
// where neither rejects)
struct GateOut {
    bool pass, sing, amb;
};
template <typename T>
__device__ __forceinline__ GateOut shard_gate(const ShardParams& p, int line, const RobotBlock& rb,
                                              const LmState& lm, const LmStart& s0, Cand& c)
{
    constexpr double ETA = gate_eta<T>();
    const ekf_line ln = p.lines[line];
    double Rm[4];
    line_R(ln, line, p.r_mode, Rm);
    Block5 b5;
    fill_block5(b5, rb.R33, lm.rr0, lm.rr1, lm.rr2, lm.Dj);
    double sn, cs;
    GateOut g = {false, false, false};
    if (!quick_reject(b5, lm.yb.x, lm.yb.y, s0.ma0, s0.s0f, s0.c0f, rb.xp, ln.alpha, ln.r, Rm, p.gate, ETA) &&
        (sincos_near(lm.yb.x, s0.ma0, s0.s0j, s0.c0j, sn, cs),
         !certified_reject(b5, lm.yb.x, lm.yb.y, sn, cs, rb.xp, ln.alpha, ln.r, Rm, p.gate, ETA))) {
        eval_candidate(b5, lm.yb.x, lm.yb.y, sn, cs, rb.xp, ln.alpha, ln.r, Rm, p.gate, ETA, c);
        g.sing = c.singular;
        g.amb = c.amb;
        g.pass = c.pass;
    }
    return g;
}

// The status bits line `line` raises at landmark j (jstar: the line's winner, 0x7fffffff none): GSL_EDOM
// and the gate's precision margin count only for the candidates the reference evaluates (up to the
// winner); the as-written R
__device__ __forceinline__ int shard_line_status(const ShardParams& p, int line, int j, int jstar, bool sing,
                                                 bool amb)
{
    int st = sing && j <= jstar ? (int)EKF_ST_SINGULAR : 0;
    if (amb && j <= jstar) st |= EKF_ST_PRECISION_BIT;   // (gate_eta)
    if (p.r_mode == 1 && (line == 1 || line == 2)) st |= EKF_ST_NSYM;
    return st;
}

// The operand rows of match m of landmark j from its gain rows (the scan kernel's store_rows in its
// non-staged form: the same values; symmetric operands as sym_factor's comment). A partitioned context
// stores fp32 or fp64, whose storage exponent is 0 and ignored by to_domain.
template <typename T>
__device__ __forceinline__ void shard_store_ops(const ShardParams& p, int j, int m, const double kk[4],
                                                const double uu[4], const double* pk)
{
    using C = typename Stor<T>::C;
    const bool sym = p.r_mode != 1 && sizeof(C) == 4;
    float F[3] = {0.f, 0.f, 0.f};
    if (sym) sym_factor(pk, F);
    const int kmax = p.d.kmax;
    C* Uop = reinterpret_cast<C*>(p.cur.Uop);
    C* Vop = reinterpret_cast<C*>(p.cur.Vop);
#pragma unroll
    for (int pp = 0; pp < 2; pp++) {
        const int lr = 2 * j + pp;
        if constexpr (sizeof(C) == 4) {
            double o0 = uu[2 * pp], o1 = uu[2 * pp + 1], v0 = kk[2 * pp], v1 = kk[2 * pp + 1];
            if (sym) {
                v0 = kk[2 * pp] * (double)F[0] + kk[2 * pp + 1] * (double)F[1];
                v1 = kk[2 * pp + 1] * (double)F[2];
                o0 = (double)(float)v0;
                o1 = (double)(float)v1;
            }
            Uop[op_index_f32(lr, 2 * m, kmax)] = to_domain<T>(-o0, 0);
            Uop[op_index_f32(lr, 2 * m + 1, kmax)] = to_domain<T>(-o1, 0);
            Vop[op_index_f32(lr, 2 * m, kmax)] = (C)v0;
            Vop[op_index_f32(lr, 2 * m + 1, kmax)] = (C)v1;
        } else {
            Uop[op_index_f64(lr, 2 * m, kmax)] = (C)(-uu[2 * pp]);
            Uop[op_index_f64(lr, 2 * m + 1, kmax)] = (C)(-uu[2 * pp + 1]);
            Vop[op_index_f64(lr, 2 * m, kmax)] = (C)kk[2 * pp];
            Vop[op_index_f64(lr, 2 * m + 1, kmax)] = (C)kk[2 * pp + 1];
        }
    }
}

// ---- the phases of the scan for landmark j (every rank runs every landmark; shard_kernel) ----
// SH_BEGIN: the committed robot block and pose, predicted (every thread the same), every landmark's
// strip columns predicted (Robot.cpp:242) and scan-start angle; the rank's diagonal blocks with the
// pending steps applied into the exchange buffer (zero where another rank's)
template <typename T>
__device__ __forceinline__ void shard_begin(const ShardParams& p, int j, const PllView<T>& pv)
{
    const Dims d = p.d;
    const int n = d.n;
    int* ctl = p.ctl;
    const int s = p.saved[0];
    RobotBlock rb;
#pragma unroll
    for (int a = 0; a < 9; a++) rb.R33[a] = p.Rs[(a / 3) * n + (a % 3)];
    double F3[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    shard_predict(p.pose, p.enc_v, p.enc_noise, F3, rb.R33, rb.xp);
    if (j == 0) {
        // the scan's inputs, handed over as kernel arguments (no host staging copy), for the
        // later phases
        double* enc = const_cast<double*>(p.enc);
        enc[0] = p.enc_v[0]; enc[1] = p.enc_v[1]; enc[2] = p.enc_v[2];
        ekf_line* lines = const_cast<ekf_line*>(p.lines);
        for (int i = 0; i < d.max_lines; i++) lines[i] = p.lines_v[i];
        rob_store(p.rob, rb);
        ctl[SC_WIN] = 0x7fffffff;
        ctl[SC_STATUS] = 0;
        ctl[SC_M] = 0;
        ctl[SC_NEXTRA] = 0;
        ctl[SC_S] = s;
        ctl[SC_NEXT] = 0;
        for (int i = 0; i < EKF_MAX_LINES; i++) ctl[SC_GUESS + i] = 0x7fffffff;
    }
    if (!(j < d.N)) return;
    const int b0 = 3 + 2 * j;
    LmState lm;
    lm.rr0 = *reinterpret_cast<const double2*>(p.Rs + b0);
    lm.rr1 = *reinterpret_cast<const double2*>(p.Rs + n + b0);
    lm.rr2 = *reinterpret_cast<const double2*>(p.Rs + 2 * n + b0);
    lm.yb = *reinterpret_cast<const double2*>(p.y + b0);
    predict_cols(F3, lm.rr0, lm.rr1, lm.rr2);
    // (the record's diagonal block comes with SH_DIAG, summed over the ranks)
    lm.Dj[0] = lm.Dj[1] = lm.Dj[2] = lm.Dj[3] = 0.0;
    double Dj[4] = {0, 0, 0, 0};
    if (j < s && shard_local_blk(p, j, j)) pll_block(pv, 2 * j, 2 * j, Dj);
    double s0j, c0j;
    sincos(lm.yb.x, &s0j, &c0j);
    float s0f, c0f;
    __sincosf((float)lm.yb.x, &s0f, &c0f);
    const LmStart s0 = {lm.yb.x, s0j, c0j, (double)s0f, (double)c0f};
    rec_store_all(p.rec + (size_t)j * SH_REC, lm, s0);
    *reinterpret_cast<double4*>(p.col + 4 * (size_t)j) = make_double4(Dj[0], Dj[1], Dj[2], Dj[3]);
    p.flags[j] = 0;
}

// SH_DIAG (and SH_GUESS with diag_first): the landmark's diagonal block summed over the ranks (every
// rank contributed its own) from the exchange buffer, into its record where `keep`
__device__ __forceinline__ void shard_take_diag(const ShardParams& p, int j, bool keep, double Dj[4])
{
    const double4 dj = *reinterpret_cast<const double4*>(p.col + 4 * (size_t)j);
    Dj[0] = dj.x; Dj[1] = dj.y; Dj[2] = dj.z; Dj[3] = dj.w;
    if (keep) {
        double* rc = p.rec + (size_t)j * SH_REC;
#pragma unroll
        for (int k = 0; k < 4; k++) rc[REC_DJ + k] = Dj[k];
    }
}

// SH_GUESS: every line's first passing landmark at the scan's start (no line applied yet; one line per
// grid row): the speculative path fetches these columns in one exchange, and shard_spec_kernel checks
// each line's real winner against its guess. With diag_first the summed diagonal blocks are taken in
// the same launch (its grid row 0 stores them)
template <typename T>
__device__ __forceinline__ void shard_guess(const ShardParams& p, int line, int j)
{
    const double* rc = p.rec + (size_t)j * SH_REC;
    LmState lm;
    rec_load(rc, true, lm);
    if (p.diag_first) shard_take_diag(p, j, line == 0, lm.Dj);
    if (!(j < p.ctl[SC_S])) return;
    RobotBlock rb;
    rob_load(p.rob, rb);
    LmStart s0;
    rec_load_start(rc, true, s0);
    Cand c;
    if (shard_gate<T>(p, line, rb, lm, s0, c).pass) atomicMin(p.ctl + SC_GUESS + line, j);
}

// SH_SPEC_COLS: the rank's blocks of the guessed column of line `line` (one line per grid row), pending
// steps applied (SH_COLUMN's blocks)
template <typename T>
__device__ __forceinline__ void shard_spec_cols(const ShardParams& p, int line, int j, const PllView<T>& pv)
{
    const int w = p.ctl[SC_GUESS + line];
    double blk[4] = {0, 0, 0, 0};
    if (w != 0x7fffffff && shard_local_blk(p, j, w)) pll_block(pv, 2 * j, 2 * w, blk);
    *reinterpret_cast<double4*>(p.cols + 4 * ((size_t)line * p.d.N + j)) = make_double4(blk[0], blk[1], blk[2], blk[3]);
}

// SH_GATE: the first passing unmatched landmark of the line: every rank finds the same one
template <typename T>
__device__ __forceinline__ void shard_gate_phase(const ShardParams& p, int line, int j)
{
    const int fl = p.flags[j];
    if (!(j < p.ctl[SC_S]) || (fl & 1)) {
        p.flags[j] = fl & 1;
        return;
    }
    const double* rc = p.rec + (size_t)j * SH_REC;
    RobotBlock rb;
    rob_load(p.rob, rb);
    LmState lm;
    LmStart s0;
    rec_load(rc, true, lm);
    rec_load_start(rc, true, s0);
    Cand c;
    const GateOut g = shard_gate<T>(p, line, rb, lm, s0, c);
    p.flags[j] = (fl & 1) | (g.sing ? 2 : 0) | (g.amb ? 4 : 0);
    if (g.pass) atomicMin(p.ctl + SC_WIN, j);
}

// SH_COLUMN: the winner's gain package (its thread) and the rank's blocks of its column, with the
// pending steps applied, into the exchange buffer (zero where another rank's)
template <typename T>
__device__ __forceinline__ void shard_column(const ShardParams& p, int line, int j, const PllView<T>& pv)
{
    const int jstar = p.ctl[SC_WIN];
    double blk[4] = {0, 0, 0, 0};
    if (jstar != 0x7fffffff) {
        if (shard_local_blk(p, j, jstar)) pll_block(pv, 2 * j, 2 * jstar, blk);
        if (j == jstar) {
            const double* rc = p.rec + (size_t)j * SH_REC;
            RobotBlock rb;
            rob_load(p.rob, rb);
            LmState lm;
            LmStart s0;
            rec_load(rc, true, lm);
            rec_load_start(rc, true, s0);
            Cand c;
            shard_gate<T>(p, line, rb, lm, s0, c);
            build_package(c, rb.R33, lm.rr0, lm.rr1, lm.rr2, p.pkg);
            package_v_rows(p.hist + (size_t)j * p.d.max_lines * 8, p.ctl[SC_M], p.pkg);
        }
    }
    *reinterpret_cast<double4*>(p.col + 4 * (size_t)j) = make_double4(blk[0], blk[1], blk[2], blk[3]);
}

// SH_APPLY: the line's status bits, and for a match the landmark's gain rows from its block of the
// winner's column (summed over the ranks): its history and operand rows, its record
template <typename T>
__device__ __forceinline__ void shard_apply(const ShardParams& p, int line, int j)
{
    const int jstar = p.ctl[SC_WIN];
    int fl = p.flags[j];
    const int st = shard_line_status(p, line, j, jstar, (fl & 2) != 0, (fl & 4) != 0);
    if (st) atomicOr(p.ctl + SC_STATUS, st);
    if (jstar == 0x7fffffff) return;
    double* rc = p.rec + (size_t)j * SH_REC;
    LmState lm;
    rec_load(rc, true, lm);
    const double4 cb = *reinterpret_cast<const double4*>(p.col + 4 * (size_t)j);   // summed over ranks
    double blk[4] = {cb.x, cb.y, cb.z, cb.w};
    const double* pk = p.pkg;
    const int m = p.ctl[SC_M];
    double* hist = p.hist + (size_t)j * p.d.max_lines * 8;
    double kk[4], uu[4];
    gain_rows<0>(pk, m,
                 [&](int q) {
                     const double* h = hist + 8 * q;
                     return make_double4(h[0], h[1], h[2], h[3]);
                 },
                 PackageV{pk}, blk, lm.rr0, lm.rr1, lm.rr2, lm.yb, lm.Dj, kk, uu);
    hist_row_store(hist + 8 * m, uu, kk);
    shard_store_ops<T>(p, j, m, kk, uu, pk);
    if (j == jstar) fl |= 1;
    p.flags[j] = fl & 1;
    rec_store(rc, lm);
}

// SH_ROBOT, after line `line` (one thread): the robot block and x_pre after its match
// (Robot.cpp:560-602), the match list, and the winner word reset for the next line's gate
__device__ __forceinline__ void shard_robot(const ShardParams& p, int line)
{
    int* ctl = p.ctl;
    const int jstar = ctl[SC_WIN];
    if (jstar != 0x7fffffff) {
        RobotBlock rb;
        rob_load(p.rob, rb);
        robot_update(rb.R33, rb.xp, p.pkg);
        rob_store(p.rob, rb);
        ctl[SC_MATCH + line] = jstar;
        ctl[SC_M] += 1;
    } else {
        ctl[SC_MATCH + line] = -1;
        ctl[SC_EXTRA + ctl[SC_NEXTRA]] = line;
        ctl[SC_NEXTRA] += 1;
    }
    ctl[SC_WIN] = 0x7fffffff;
}

// SH_END: augmentation (Robot.cpp:776-866) as the scan kernel's commit: the new landmarks' rows
// to the step's patch buffer (every rank all of them: its flush takes the columns of its tiles),
// the new landmarks' strip columns and mean, the 2×2 diagonal blocks; the capacity reset
// (Robot.cpp:893-904)
template <typename T>
__device__ __forceinline__ void shard_end(const ShardParams& p, int j)
{
    using C = typename Stor<T>::C;
    const Dims d = p.d;
    const int n = d.n;
    const int* ctl = p.ctl;
    if (p.end_gate) {
        // (ekf_shard_localize) launched behind the speculative run before the host has read the
        // agreement: a run that stopped short or failed on some rank leaves everything untouched
        const double a0 = p.end_gate[0], a1 = p.end_gate[1];
        if (j == 0) {
            p.end_gate_host[0] = a0;
            p.end_gate_host[1] = a1;
            __threadfence_system();
        }
        if (a0 > 0.0 || a1 != (double)p.L) return;
    }
    RobotBlock rb;
    rob_load(p.rob, rb);
    const double* R33 = rb.R33;
    const double* xp = rb.xp;
    LmState lm;
    rec_load(p.rec + (size_t)j * SH_REC, true, lm);
    double2 rr0 = lm.rr0, rr1 = lm.rr1, rr2 = lm.rr2, yb = lm.yb;
    const int b0 = 3 + 2 * j;
    const int s = ctl[SC_S];
    const int m = ctl[SC_M], nextra = ctl[SC_NEXTRA];
    double pose[3] = {xp[0], xp[1], xp[2]};
    if (p.L == 0 || m == 0) pose[2] = normalize_radian(xp[2]);
    const int N = d.N, M = d.M;
    const int nadd = min(nextra, N - s);
    const int reset = (s + nadd > N - p.reset_margin) ? 1 : 0;
    double* patch = p.cur.patch;
    double* pdiag = p.cur.patch_diag;
    if (!reset) {
        for (int q = 0; q < nadd; q++) {
            const ekf_line lq = p.lines[ctl[SC_EXTRA + q]];
            const int sq = s + q;
            double alfa = lq.alpha;
            const double r = lq.r + (pose[0] * cos(alfa) + pose[1] * sin(alfa));
            alfa += pose[2];
            double sa, ca;
            sincos(alfa, &sa, &ca);
            if (j < sq) {
                double* prow = patch + (size_t)(q * 2) * M;
                *reinterpret_cast<double2*>(prow + 2 * j) = rr2;
                double2 gx;
                gx.x = ca * rr0.x + sa * rr1.x;
                gx.y = ca * rr0.y + sa * rr1.y;
                *reinterpret_cast<double2*>(prow + M + 2 * j) = gx;
            }
            if (j == sq) {
                rr0 = make_double2(R33[6], ca * R33[0] + sa * R33[3]);
                rr1 = make_double2(R33[7], ca * R33[1] + sa * R33[4]);
                rr2 = make_double2(R33[8], ca * R33[2] + sa * R33[5]);
                yb = make_double2(normalize_radian(alfa), r);
            }
            if (j == 0) {
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
                        GlR[a * 2 + b] = Gl[a * 2 + 0] * lq.R[0 * 2 + b] + Gl[a * 2 + 1] * lq.R[1 * 2 + b];
                for (int a = 0; a < 2; a++)
                    for (int b = 0; b < 2; b++) {
                        double gsum = 0.0;
                        for (int k = 0; k < 3; k++) gsum += GP[a * 3 + k] * Gx[b * 3 + k];
                        const double hh = GlR[a * 2 + 0] * Gl[b * 2 + 0] + GlR[a * 2 + 1] * Gl[b * 2 + 1];
                        pdiag[q * 4 + a * 2 + b] = gsum + hh;
                    }
            }
        }
    }
    if (reset) rr0 = rr1 = rr2 = yb = make_double2(0.0, 0.0);
    // the strip columns and mean, the operand padding past the matches
    *reinterpret_cast<double2*>(p.Rs + b0) = rr0;
    *reinterpret_cast<double2*>(p.Rs + n + b0) = rr1;
    *reinterpret_cast<double2*>(p.Rs + 2 * n + b0) = rr2;
    *reinterpret_cast<double2*>(p.y + b0) = yb;
    C* Uop = reinterpret_cast<C*>(p.cur.Uop);
    C* Vop = reinterpret_cast<C*>(p.cur.Vop);
    for (int k = 2 * m; k < d.kmax; k++)
#pragma unroll
        for (int pp = 0; pp < 2; pp++) {
            if constexpr (sizeof(C) == 4) {
                Uop[op_index_f32(2 * j + pp, k, d.kmax)] = (C)(-0.0f);
                Vop[op_index_f32(2 * j + pp, k, d.kmax)] = (C)0.0f;
            } else {
                Uop[op_index_f64(2 * j + pp, k, d.kmax)] = (C)(-0.0);
                Vop[op_index_f64(2 * j + pp, k, d.kmax)] = (C)0.0;
            }
        }
    if (j == 0) {
        // commit (Robot.cpp:702-716)
        for (int a = 0; a < 9; a++) p.Rs[(a / 3) * n + (a % 3)] = R33[a];
        p.y[0] = xp[0]; p.y[1] = xp[1]; p.y[2] = xp[2];
        p.pose[0] = pose[0]; p.pose[1] = pose[1]; p.pose[2] = pose[2];
        int* res = p.cur.res;
        res[RES_NLINES] = p.L;
        res[RES_SAVED_IN] = s;
        res[RES_DBG] = 16;
        res[RES_STATUS] = ((nextra > nadd) ? EKF_ST_CAP : 0) | ctl[SC_STATUS];
        res[RES_M] = m;
        res[RES_NEXTRA] = nextra;
        res[RES_SAVED] = reset ? 0 : s + nadd;
        res[RES_RESET] = reset;
        res[RES_NADD] = reset ? 0 : nadd;
        res[RES_KSTEPS] = (sizeof(C) == 4) ? m : (m + 1) / 2;
        res[RES_ROLLBACK] = 0;
        for (int i = 0; i < p.L; i++) res[RES_MATCH + i] = ctl[SC_MATCH + i];
        for (int q = 0; q < nextra; q++) res[RES_EXTRA + q] = ctl[SC_EXTRA + q];
        p.saved[0] = reset ? 0 : s + nadd;
        if (p.res_host) {
            // the words ekf_result takes, for the host to read after this kernel without a copy
            // (each store crosses to host memory: only these, not the whole record)
            int* rh = p.res_host;
            rh[RES_NLINES] = res[RES_NLINES];
            rh[RES_STATUS] = res[RES_STATUS];
            rh[RES_M] = res[RES_M];
            rh[RES_NEXTRA] = res[RES_NEXTRA];
            rh[RES_SAVED] = res[RES_SAVED];
            rh[RES_RESET] = res[RES_RESET];
            for (int i = 0; i < p.L; i++) rh[RES_MATCH + i] = res[RES_MATCH + i];
            p.pose_host[0] = pose[0]; p.pose_host[1] = pose[1]; p.pose_host[2] = pose[2];
            __threadfence_system();
        }
    }
}

// One phase of the partitioned instance's scan, one landmark per thread
template <typename T>
__global__ __launch_bounds__(SH_THREADS) void shard_kernel(ShardParams p)
{
    __shared__ int4 sh_ctl[PMAX];
    for (int q = threadIdx.x; q < p.npend; q += blockDim.x) {
        const int* r = p.pend[q].res;
        sh_ctl[q] = make_int4(r[RES_RESET], r[RES_KSTEPS], r[RES_NADD], r[RES_SAVED_IN]);
    }
    __syncthreads();
    const Dims d = p.d;
    PllView<T> pv;
    pv.X = reinterpret_cast<const T*>(p.Pread);
    pv.nb = d.nb;
    pv.kmax = d.kmax;
    pv.M = d.M;
    pv.max_lines = d.max_lines;
    pv.e = 0;
    pv.ex = storage_exp<T>(p.pexp, 0);
    pv.opstride = (size_t)d.nb * 64 * (d.kmax / 2);
    pv.usym = 0;   // (the partitioned instance stores its U rows)
    pv.us = 1.0f;
    pv.npend = p.npend;
    pv.pend = p.pend;
    pv.ctl = sh_ctl;
    pv.rnd = 1;
    const int j = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    const bool own = j < d.N;
    const int row = (int)blockIdx.y;   // (SH_GUESS, SH_SPEC_COLS: grid row y = the line)
    switch (p.phase) {
    case SH_BEGIN: shard_begin<T>(p, j, pv); break;
    case SH_DIAG: {
        double Dj[4];
        if (own) shard_take_diag(p, j, true, Dj);
        break;
    }
    case SH_GUESS: if (own) shard_guess<T>(p, row, j); break;
    case SH_SPEC_COLS: if (own) shard_spec_cols<T>(p, row, j, pv); break;
    case SH_GATE: if (own) shard_gate_phase<T>(p, p.line, j); break;
    case SH_COLUMN: if (own) shard_column<T>(p, p.line, j, pv); break;
    case SH_APPLY: if (own) shard_apply<T>(p, p.line, j); break;
    case SH_ROBOT: if (j == 0) shard_robot(p, p.line); break;
    case SH_END: if (own) shard_end<T>(p, j); break;
    default: break;
    }
}

// The speculative path's lines in the association kernel's form (ekf_shard_run, at
// most SH_MAX_LINES lines; G cooperating workgroups, K = ⌈N / (G·SHR_THREADS)⌉ landmarks per thread):
// every workgroup replays the guessed winners' chain itself from the exchanged guessed columns (p.cols,
// which hold every block (j, w_t), the winners' mutual blocks among them) and checks each line's guess
// on its own landmarks; one verdict exchange among the workgroups at the end, no exchange per line.
// Per workgroup: two landmark waves (one landmark per thread, its record, history rows and flags kept
// in registers and LDS) and a replay wave (lane u = line u's guessed winner). Line t: the replay lane t
// evaluates its winner's gate at the state after lines < t and, if it passes, builds the line's
// package (build_package and the winner's V rows of the earlier matches, as SH_COLUMN); every lane
// takes the robot update (robot_update, as SH_ROBOT) and the later winners' lanes apply the line to
// their winners (gain rows, as SH_APPLY). Meanwhile each landmark thread, per line as its package is
// published: its gate at that state (shard_gate, as SH_GATE), a violation if it passes before the guess
// or while the guess fails, and the line's update (as SH_APPLY: gain rows, history row, operand rows).
// The verdict (the first violating line over all workgroups) decides: the records, flags, history rows,
// control words and robot block are written as they stand after the lines before it (recomputed from
// the run's start when a violation cut the lines short), and *next_out = that line (L + 1 when a
// workgroup's exchange timed out or it never arrived: the scan is abandoned); the caller runs the
// per-line phases from there. Every rank holds the same replicated state, so every rank stops at the
// same line. With several landmarks per thread (N > G·SHR_THREADS) each thread checks its landmarks
// one after the other without stores, and after the verdict runs each again over the lines kept, with
// the stores. Every value comes from the functions above, which the per-line phases call on the same
// inputs: bit-identical.
constexpr int SPR_THREADS = SHR_THREADS + 64;   // two landmark waves + the replay wave
template <typename T>
__global__ __launch_bounds__(SPR_THREADS) void shard_spec_kernel(ShardParams p)
{
    constexpr double ETA = gate_eta<T>();
    constexpr int SPK = MB_VH + 4 * SH_MAX_LINES;   // a package: build_package's words + the V rows
    __shared__ int sh_cw[SC_WORDS];
    __shared__ double sh_pk[SH_MAX_LINES][SPK];          // line t's package
    __shared__ double sh_robl[SH_MAX_LINES + 1][ROB_WORDS];   // the robot block and x_pre before line t
    __shared__ int sh_pass[SH_MAX_LINES];                // line t's guessed winner passed its gate
    __shared__ int sh_ready;                              // packages published (lines < sh_ready)
    __shared__ double sh_wh[SH_MAX_LINES][SH_MAX_LINES][8];   // replay lane u: winner u's history rows
    __shared__ double sh_lh[SH_MAX_LINES][4][SHR_THREADS];    // landmark thread tid: its U rows
    __shared__ int sh_red[SPR_THREADS / 64];
    __shared__ int sh_to, sh_bad, sh_first;
    const int tid = threadIdx.x, g = blockIdx.x, G = gridDim.x;
    const Dims d = p.d;
    const int N = d.N, L = p.L;
    for (int k = tid; k < SC_WORDS; k += SPR_THREADS) sh_cw[k] = p.ctl[k];
    if (tid < ROB_WORDS) sh_robl[0][tid] = p.rob[tid];
    if (tid == 0) {
        sh_ready = 0;
        sh_to = sh_bad = 0;
        sh_first = L;
    }
    __syncthreads();
    const int s = sh_cw[SC_S];
    int tstatus = 0;

    if (tid >= SHR_THREADS) {
        // ---- the replay wave: lane u carries line u's guessed winner up to its line ----
        const int u = tid - SHR_THREADS;
        const int wu = u < L ? sh_cw[SC_GUESS + u] : 0x7fffffff;
        const bool act = wu != 0x7fffffff && wu < N;
        const double* rc = p.rec + (size_t)wu * SH_REC;   // (read only where act)
        LmState lm;
        LmStart s0;
        rec_load(rc, act, lm);
        rec_load_start(rc, act, s0);
        double* wh = &sh_wh[act ? u : 0][0][0];   // its winner's history rows (used only where act)
        bool matched = false;
        int m = 0;
        for (int t = 0; t < L; t++) {
            const int wt = sh_cw[SC_GUESS + t];
            bool pass = false;
            if (u == t && act && !matched && wu < s) {
                // the exact evaluation without the reject filters (shard_gate's), which never reject
                // a landmark that passes (the association kernel's replay wave does the same); its
                // status bits come from the landmark's own thread
                Cand c;
                const ekf_line ln = p.lines[t];
                double Rm[4];
                line_R(ln, t, p.r_mode, Rm);
                RobotBlock rb;
                rob_load(sh_robl[t], rb);
                Block5 b5;
                fill_block5(b5, rb.R33, lm.rr0, lm.rr1, lm.rr2, lm.Dj);
                double sn, cs;
                sincos_near(lm.yb.x, s0.ma0, s0.s0j, s0.c0j, sn, cs);
                eval_candidate<false>(b5, lm.yb.x, lm.yb.y, sn, cs, rb.xp, ln.alpha, ln.r, Rm, p.gate, ETA, c);
                pass = c.pass;
                if (pass) {
                    build_package(c, rb.R33, lm.rr0, lm.rr1, lm.rr2, sh_pk[t]);
                    package_v_rows(wh, m, sh_pk[t]);
                }
                sh_pass[t] = pass ? 1 : 0;
            } else if (u == t) {
                sh_pass[t] = 0;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            const bool pt = sh_pass[t] != 0;
            // the robot block and x_pre after line t (SH_ROBOT; every lane the same bits)
            {
                RobotBlock rb;
                rob_load(sh_robl[t], rb);
                if (pt) robot_update(rb.R33, rb.xp, sh_pk[t]);
                if (u == 0) rob_store(sh_robl[t + 1], rb);
            }
            // the later winners take line t's update (SH_APPLY on their own landmark)
            if (pt && act && u > t) {
                const double4 cb = *reinterpret_cast<const double4*>(p.cols + 4 * ((size_t)t * N + wu));
                double blk[4] = {cb.x, cb.y, cb.z, cb.w};
                const double* pk = sh_pk[t];
                double kk[4], uu[4];
                gain_rows<0>(pk, m,
                             [&](int q) {
                                 const double* h = wh + 8 * q;
                                 return make_double4(h[0], h[1], h[2], h[3]);
                             },
                             PackageV{pk}, blk, lm.rr0, lm.rr1, lm.rr2, lm.yb, lm.Dj, kk, uu);
                hist_row_store(wh + 8 * m, uu, kk);
                if (wu == wt) matched = true;
            }
            if (pt) m++;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_wave_barrier();
            if (u == 0) __hip_atomic_store(&sh_ready, t + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
    }

    // ---- the landmark waves: landmark j = g·SHR_THREADS + tid + k·G·SHR_THREADS, k < K ----
    const int K = (N + G * SHR_THREADS - 1) / (G * SHR_THREADS);   // landmarks per thread (uniform)
    const int j0 = g * SHR_THREADS + tid;
    int stacc = 0;   // the status bits of the lines run (SH_APPLY's)
    int viol = L;    // this thread's first violating line
    // one pass over lines [0, upto) for landmark j: gates (check: the violations), updates into
    // the registers; store: the history and operand rows as they come (the same rows are
    // rewritten by the per-line phases for any line not kept)
    auto run_lines = [&](int j, const LmStart& s0, int upto, bool check, bool store, LmState& lm, bool& matched,
                         int& m) {
        const bool own = tid < SHR_THREADS && j < N;
        for (int i = 0; i < upto; i++) {
            if (tid < SHR_THREADS) {
                int polls = 0;
                while (__hip_atomic_load(&sh_ready, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) <= i) {
                    __builtin_amdgcn_s_sleep(1);
                    if ((tstatus & EKF_ST_TIMEOUT_BIT) || ++polls > (1 << p.spin_log2)) {
                        tstatus |= EKF_ST_TIMEOUT_BIT;
                        break;
                    }
                }
            }
            if (!own) continue;
            const int w = sh_cw[SC_GUESS + i];
            const bool pt = sh_pass[i] != 0;
            const int jstar = pt ? w : 0x7fffffff;
            GateOut gt = {false, false, false};
            if (j < s && !matched) {
                Cand c;
                RobotBlock rb;
                rob_load(sh_robl[i], rb);
                gt = shard_gate<T>(p, i, rb, lm, s0, c);
            }
            if (check && gt.pass && (!pt || j < w)) {   // the guess is not the line's first passing landmark
                viol = min(viol, i);
                return;
            }
            stacc |= shard_line_status(p, i, j, jstar, gt.sing, gt.amb);
            if (!pt) continue;
            const double4 cb = *reinterpret_cast<const double4*>(p.cols + 4 * ((size_t)i * N + j));
            double blk[4] = {cb.x, cb.y, cb.z, cb.w};
            const double* pk = sh_pk[i];
            double kk[4], uu[4];
            gain_rows<0>(pk, m,
                         [&](int q) { return make_double4(sh_lh[q][0][tid], sh_lh[q][1][tid], sh_lh[q][2][tid], sh_lh[q][3][tid]); },
                         PackageV{pk}, blk, lm.rr0, lm.rr1, lm.rr2, lm.yb, lm.Dj, kk, uu);
#pragma unroll
            for (int k = 0; k < 4; k++) {
                sh_lh[m][k][tid] = uu[k];
            }
            if (store) {
                hist_row_store(p.hist + ((size_t)j * d.max_lines + m) * 8, uu, kk);
                shard_store_ops<T>(p, j, m, kk, uu, pk);
            }
            if (j == w) matched = true;
            m++;
        }
    };
    // one landmark's pass from its record at the run's start (the run starts at line 0:
    // ekf_shard_run, no match yet), its record and flag written at the end (write)
    auto run_landmark = [&](int j, int upto, bool check, bool store, bool write) {
        const bool own = tid < SHR_THREADS && j < N;
        double* rc = p.rec + (size_t)j * SH_REC;   // (touched only where own)
        LmState lm;
        LmStart s0;
        rec_load(rc, own, lm);
        rec_load_start(rc, own, s0);
        bool matched = own && (p.flags[j] & 1);
        int m = 0;
        run_lines(j, s0, upto, check, store, lm, matched, m);
        if (write && own) {
            rec_store(rc, lm);
            p.flags[j] = matched ? 1 : 0;
        }
    };
    // one landmark per thread (K = 1): its state stays in registers across the verdict and is
    // recomputed (from lm0, its record at the run's start) only when a violation cut the run short
    LmState lm0, lm;
    LmStart s00;
    bool matched = false;
    int m = 0;
    const bool own0 = tid < SHR_THREADS && j0 < N;
    double* rc0 = p.rec + (size_t)j0 * SH_REC;   // (touched only where own0)
    rec_load(rc0, own0 && K == 1, lm0);
    rec_load_start(rc0, own0 && K == 1, s00);
    lm = lm0;
    if (K == 1) {
        matched = own0 && (p.flags[j0] & 1);
        run_lines(j0, s00, L, true, true, lm, matched, m);
    } else {
        // several landmarks per thread: check each in turn (no stores; lines at or past an earlier
        // violation of this thread are never kept), the stores after the verdict
        for (int k = 0; k < K; k++) run_landmark(j0 + k * G * SHR_THREADS, viol, true, false, false);
    }
    // ---- the verdict: the first violating line over every workgroup (one exchange) ----
    {
        int v = viol;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off, 64));
        if ((tid & 63) == 0) sh_red[tid >> 6] = v;
        __syncthreads();
        int wv = L;
        for (int w = 0; w < SHR_THREADS / 64; w++) wv = min(wv, sh_red[w]);
        double* slot = p.mbox + (size_t)g * p.mbw;
        if (tid == 0) mb_tag(slot, p.epoch, TAG_SPEC_VERDICT, (unsigned)(wv + 1));
        for (int k = tid; k < G; k += SPR_THREADS) {
            const int bq = mb_poll(p.mbox, 0, G, k, p.mbw, p.epoch, TAG_SPEC_VERDICT, tstatus, p.spin_log2);
            if (bq <= 0) sh_to = 1;
            else atomicMin(&sh_first, bq - 1);
        }
        if (tstatus & EKF_ST_TIMEOUT_BIT) sh_to = 1;
        __syncthreads();
    }
    const int first = sh_to ? 0 : sh_first;
    if (K == 1) {
        // the state after the lines before `first` (recomputed when the run was cut short)
        if (first < L && !sh_to) {
            lm = lm0;
            matched = own0 && (p.flags[j0] & 1);
            m = 0;
            stacc = 0;
            run_lines(j0, s00, first, false, true, lm, matched, m);
        }
        if (own0 && !sh_to) {
            rec_store(rc0, lm);
            p.flags[j0] = matched ? 1 : 0;
        }
    } else if (!sh_to) {
        stacc = 0;
        for (int k = 0; k < K; k++) run_landmark(j0 + k * G * SHR_THREADS, first, false, true, true);
    }
    const bool own = own0 || (K > 1 && tid < SHR_THREADS);
    int st = own ? stacc : 0;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) st |= __shfl_xor(st, off, 64);
    __syncthreads();
    if ((tid & 63) == 0) sh_red[tid >> 6] = st;
    __syncthreads();
    // every workgroup's outcome to workgroup 0: its stopping line and whether one of its waits timed
    // out, one self-tagged word each (parity-0 slot, last word: the list words' region, which the
    // association kernel of a partitioned context never uses). Workgroup 0 decides over all G of them,
    // so a workgroup whose verdict poll timed out, or that never arrived, makes the run report L + 1,
    // and the scan is abandoned on every rank
    if (tid == 0) {
        int wst = 0;
        for (int w = 0; w < SPR_THREADS / 64; w++) wst |= sh_red[w];
        atomicOr(p.ctl + SC_STATUS, wst | (sh_to ? (int)EKF_ST_TIMEOUT_BIT : 0));
        mb_store_tagged(p.mbox + (size_t)g * p.mbw + p.mbw - 1, p.epoch,
                        ((unsigned long long)first << 1) | (sh_to ? 1ull : 0ull));
    }
    if (g == 0) {
        for (int k = tid; k < G; k += SPR_THREADS) {
            int stw = sh_to ? (int)EKF_ST_TIMEOUT_BIT : 0;
            const unsigned long long w = mb_wait_tagged(p.mbox + (size_t)k * p.mbw + p.mbw - 1, p.epoch, stw, p.spin_log2);
            if (stw || (w & 1ull) || (int)(w >> 1) != first) atomicOr(&sh_bad, 1);
        }
        __syncthreads();
        if (tid == 0) {
            // the control words after the lines kept (SH_ROBOT's bookkeeping, line by line)
            int mm = 0, nx = sh_cw[SC_NEXTRA];
            for (int i = 0; i < first; i++) {
                if (sh_pass[i]) {
                    sh_cw[SC_MATCH + i] = sh_cw[SC_GUESS + i];
                    mm++;
                } else {
                    sh_cw[SC_MATCH + i] = -1;
                    sh_cw[SC_EXTRA + nx] = i;
                    nx++;
                }
            }
            sh_cw[SC_M] += mm;
            sh_cw[SC_NEXTRA] = nx;
            sh_cw[SC_WIN] = 0x7fffffff;
            sh_cw[SC_NEXT] = first;
            *p.next_out = (sh_to || sh_bad) ? (double)(L + 1) : (double)first;
        }
        __syncthreads();
        for (int k = tid; k < SC_WORDS; k += SPR_THREADS)
            if (k != SC_STATUS) p.ctl[k] = sh_cw[k];
        // (the robot block after the lines kept: a word per thread, whatever its layout)
        if (tid < ROB_WORDS) p.rob[tid] = sh_robl[first][tid];
    }
}

}  // namespace ekf
