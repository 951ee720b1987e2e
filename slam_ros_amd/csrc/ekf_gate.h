// ekf_gate.h — the gate arithmetic of the association (Robot.cpp:313-498): the 5×5 block of a
// candidate, its innovation covariance and innovation, the exact fp64 evaluation with the gate
// decision and the storage precision of the gate. Shared by the association kernels (ekf_kernels.hip,
// ekf_shard_kernels.h) and the gate queries (unit_gate.hip, unit_joint.hip: trial_robot, trial_block), so that all evaluate a
// candidate bit for bit alike.
#pragma once

#include "ekf_device.h"

// The association arithmetic contracts a·b + c only within one source expression, so a
// function inlined into different kernels or phases rounds identically everywhere (the
// speculative and sequential association paths must agree bit for bit).
#pragma clang fp contract(on)

namespace ekf {

struct Cand {
    double S[4];
    double Si[4];
    double v[2];
    double h10, h11, h1l;
    double w0, w1, d2;   // S⁻¹v and the distance (cand_amb)
    int pass;
    int singular;
    int amb;   // the decision is within the storage precision of the gate (gate_eta)
};

// The storage precision of the gate (round 5). P as stored differs from the fp64 reference's by
// the roundings of its storage and of the flush's products; eta bounds that difference relative
// to the magnitudes |P_ab| <= sqrt(P_aa·P_bb) of the 5×5 block. With H0 = (0, 0, −1, 1, 0) and
// ‖H1‖² = 2 + h1l², |ΔS_ab| <= eta·s_a·s_b with s_a = Σ_k |H_ak|·√P_kk, and by Cauchy-Schwarz
// s0² <= m0 = 2(|p22| + |daa|), s1² <= m1 = ‖H1‖²·tr|P5|, s0·s1 <= (m0 + m1)/2. The filters add
// these (root-free) bounds to their error bounds (a rejection then
// holds for every P within eta; the decisions themselves are unchanged, so every path still agrees
// bit for bit), and the exact evaluation reports a distance within the first-order bound
// eta·(|w0|·s0 + |w1|·s1)², w = S⁻¹v, of the gate as ambiguous: EKF_ST_PRECISION, the statement
// that this state does not resolve the reference's decision (SURVEY §8d's run-away world, where
// S is the difference of terms 1e10 times larger). fp32 storage: 2^-16 (16 × the
// per-group P bar of 1e-6); fp16: 2^-8; fp64: 2^-44.
template <typename T> constexpr double gate_eta()
{
    return sizeof(T) == 8 ? 0x1p-44 : sizeof(T) == 4 ? 0x1p-16 : 0x1p-8;
}

// 5×5 block {0,1,2, 3+2j, 4+2j} of the current P: robot 3×3 (R33), robot–landmark columns
// (Rs, owned), landmark diagonal block (Dj, owned), and H·P·Hᵀ + R for given H row 1.
struct Block5 {
    double p00, p01, p02, p10, p11, p12, p20, p21, p22;
    double p0a, p1a, p2a, p0b, p1b, p2b;
    double daa, dab, dba, dbb;
};

// S = H·P5·Hᵀ + R in the reference's summation order (Robot.cpp:397-405); also returns the
// intermediate rows hp0 = hr0·P5, hp1 = hr1·P5 (hr0 = (0,0,-1,1,0), hr1 = (h10,h11,0,h1l,1)).
__device__ __forceinline__ void innovation_cov(const Block5& b, double h10, double h11, double h1l,
                                               const double Rm[4], double S[4], double hp0[5],
                                               double hp1[5])
{
    hp0[0] = -b.p20 + b.p0a; hp0[1] = -b.p21 + b.p1a; hp0[2] = -b.p22 + b.p2a;
    hp0[3] = -b.p2a + b.daa; hp0[4] = -b.p2b + b.dab;
    hp1[0] = h10 * b.p00 + h11 * b.p10 + h1l * b.p0a + b.p0b;
    hp1[1] = h10 * b.p01 + h11 * b.p11 + h1l * b.p1a + b.p1b;
    hp1[2] = h10 * b.p02 + h11 * b.p12 + h1l * b.p2a + b.p2b;
    hp1[3] = h10 * b.p0a + h11 * b.p1a + h1l * b.daa + b.dba;
    hp1[4] = h10 * b.p0b + h11 * b.p1b + h1l * b.dab + b.dbb;
    S[0] = -hp0[2] + hp0[3] + Rm[0];
    S[1] = hp0[0] * h10 + hp0[1] * h11 + hp0[3] * h1l + hp0[4] + Rm[1];
    S[2] = -hp1[2] + hp1[3] + Rm[2];
    S[3] = hp1[0] * h10 + hp1[1] * h11 + hp1[3] * h1l + hp1[4] + Rm[3];
}

__device__ __forceinline__ double innovation_angle(double za, double ma, double xp2)
{
    // h0 (Robot.cpp:423-426) and the 2π fold of v0 (Robot.cpp:465-475)
    const double h0 = normalize_radian(ma - xp2);
    double v0 = za - h0;
    if (fabs(v0 - 2.0 * EKF_PI) < fabs(v0)) v0 -= 2.0 * EKF_PI;
    else if (fabs(v0 + 2.0 * EKF_PI) < fabs(v0)) v0 += 2.0 * EKF_PI;
    return v0;
}

__device__ __forceinline__ int cand_amb(const Block5& b, const Cand& c, double gate, double eta);

// Exact candidate evaluation in fp64 (Robot.cpp:367-489). AMB = false leaves c.amb for cand_amb
// (the replay wave evaluates it after it has published the line's package)
template <bool AMB = true>
__device__ __forceinline__ void eval_candidate(const Block5& b, double ma, double mr, double sn,
                                               double cs, const double xp[3], double za, double zr,
                                               const double Rm[4], double gate, double eta, Cand& c)
{
    c.h10 = -cs;
    c.h11 = -sn;
    c.h1l = xp[0] * sn - xp[1] * cs;
    double hp0[5], hp1[5];
    innovation_cov(b, c.h10, c.h11, c.h1l, Rm, c.S, hp0, hp1);
    const double h1 = mr - (xp[0] * cs + xp[1] * sn);
    c.Si[0] = c.Si[1] = c.Si[2] = c.Si[3] = 0.0;
    c.singular = lu_invert2(c.S, c.Si) ? 0 : 1;
    const double v0 = innovation_angle(za, ma, xp[2]);
    const double v1 = zr - h1;
    c.v[0] = v0;
    c.v[1] = v1;
    // vᵀ·S⁻¹·v (Robot.cpp:479-486); gate (:489): a NaN distance passes, as in the reference
    const double vs0 = v0 * c.Si[0] + v1 * c.Si[2];
    const double vs1 = v0 * c.Si[1] + v1 * c.Si[3];
    const double d2 = vs0 * v0 + vs1 * v1;
    // sqrt(|d2|) > gate decided without the square root where |d2| is more than 2^-40 (relative)
    // away from gate²: sqrt is correctly rounded and monotonic, so such a |d2| gives the same
    // answer; near the gate, and for NaN (which passes), the reference's expression itself
    const double a = fabs(d2), g2 = gate * gate;
    if (a < g2 * (1.0 - 0x1p-40)) c.pass = 1;
    else if (a > g2 * (1.0 + 0x1p-40)) c.pass = 0;
    else c.pass = !(sqrt(a) > gate);
    c.w0 = vs0;
    c.w1 = vs1;
    c.d2 = d2;
    c.amb = AMB ? cand_amb(b, c, gate, eta) : 0;
}

// The storage precision of the gate (gate_eta): |ΔS_ab| <= eta·s_a·s_b with s_a = Σ_k |H_ak|·√P_kk
// (H0 = (0, 0, −1, 1, 0), H1 = (h10, h11, 0, h1l, 1) on rows 0, 1, 2, a, b), so to first order
// |Δd²| <= eta·(|w0|·s0 + |w1|·s1)², w = S⁻¹v (the roots in fp32, 2^-8 of slack)
__device__ __forceinline__ int cand_amb(const Block5& b, const Cand& c, double gate, double eta)
{
    auto rt = [](double x) { return (double)__builtin_amdgcn_sqrtf((float)fabs(x)); };
    const double s0 = rt(b.p22) + rt(b.daa);
    const double s1 = fabs(c.h10) * rt(b.p00) + fabs(c.h11) * rt(b.p11) + fabs(c.h1l) * rt(b.daa) + rt(b.dbb);
    const double wv = fabs(c.w0) * s0 + fabs(c.w1) * s1;
    return !c.singular && !(fabs(c.d2 - gate * gate) > eta * (1.0 + 0x1p-8) * wv * wv);
}

// rows 0..2 of Fx·P for one landmark's robot-strip columns (Robot.cpp:242)
__device__ __forceinline__ void predict_cols(const double F3[9], double2& rr0, double2& rr1, double2& rr2)
{
    const double2 a0 = rr0, a1 = rr1, a2 = rr2;
    rr0.x = F3[0] * a0.x + F3[1] * a1.x + F3[2] * a2.x;
    rr0.y = F3[0] * a0.y + F3[1] * a1.y + F3[2] * a2.y;
    rr1.x = F3[3] * a0.x + F3[4] * a1.x + F3[5] * a2.x;
    rr1.y = F3[3] * a0.y + F3[4] * a1.y + F3[5] * a2.y;
    rr2.x = F3[6] * a0.x + F3[7] * a1.x + F3[8] * a2.x;
    rr2.y = F3[6] * a0.y + F3[7] * a1.y + F3[8] * a2.y;
}

// R of a line (Robot.cpp:302-304): r_mode 1 reproduces the reference as written (only the
// first four lines' R[3] lands in a zero-initialised 2×2)
__device__ __forceinline__ void line_R(const ekf_line& ln, int i, int r_mode, double Rm[4])
{
    if (r_mode == 1) {
        Rm[0] = i == 0 ? ln.R[3] : 0.0;
        Rm[1] = i == 1 ? ln.R[3] : 0.0;
        Rm[2] = i == 2 ? ln.R[3] : 0.0;
        Rm[3] = i == 3 ? ln.R[3] : 0.0;
    } else {
        Rm[0] = ln.R[0]; Rm[1] = ln.R[1]; Rm[2] = ln.R[2]; Rm[3] = ln.R[3];
    }
}

__device__ __forceinline__ void fill_block5(Block5& b5, const double R33[9], double2 rr0, double2 rr1,
                                            double2 rr2, const double Dj[4])
{
    b5.p00 = R33[0]; b5.p01 = R33[1]; b5.p02 = R33[2];
    b5.p10 = R33[3]; b5.p11 = R33[4]; b5.p12 = R33[5];
    b5.p20 = R33[6]; b5.p21 = R33[7]; b5.p22 = R33[8];
    b5.p0a = rr0.x; b5.p0b = rr0.y;
    b5.p1a = rr1.x; b5.p1b = rr1.y;
    b5.p2a = rr2.x; b5.p2b = rr2.y;
    b5.daa = Dj[0]; b5.dab = Dj[1]; b5.dba = Dj[2]; b5.dbb = Dj[3];
}

// x_pre, F3 and the predicted 3×3 block of instance e from the committed pose and strip
// (Robot.cpp:130-258), expression for expression the PHASE_PREDICT branch of scan_kernel, so that a
// gate (unit_gate.hip, unit_joint.hip) with an encoder pose sees what ekf_predict would commit, bit for bit
__device__ __forceinline__ void gate_predict(const TrialLines& p, int e, const double* enc, double R33[9],
                                             double xp[3], double F3[9])
{
    const double x0 = p.pose[3 * e + 0], y0 = p.pose[3 * e + 1], t0 = p.pose[3 * e + 2];
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
}

// ---- a trial line's candidate (unit_gate.hip, unit_joint.hip): one sequence from the state to the
// Block5 handed to eval_candidate, so that both kernels evaluate a candidate on the same bits ----

// the lines of launch row `row`
__device__ __forceinline__ int trial_count(const TrialLines& t, int row, int max_lines)
{
    return t.nlines ? min(max(t.nlines[row], 0), max_lines) : t.L;
}

// The robot side of a trial of instance e (launch row `row`): the 3×3 block of the committed strip
// Rs ([3][n]) and the pose the lines are seen from. With an encoder pose the predict is applied on read
// (F3: rows 0..2 of its Fx, else the identity); without one it is x_pre between ekf_predict and
// ekf_update, else the committed pose.
struct TrialRobot {
    double R33[9], xp[3], F3[9];
};
__device__ __forceinline__ void trial_robot(const TrialLines& t, int e, int row, const double* Rs, int n,
                                            TrialRobot& rb)
{
#pragma unroll
    for (int a = 0; a < 9; a++) {
        rb.R33[a] = Rs[(a / 3) * n + (a % 3)];
        rb.F3[a] = a % 4 == 0 ? 1.0 : 0.0;
    }
    if (t.enc) {
        gate_predict(t, e, t.enc + 3 * row, rb.R33, rb.xp, rb.F3);
    } else {
        const double* x = (t.use_xpre ? t.xpre : t.pose) + 3 * e;
        rb.xp[0] = x[0]; rb.xp[1] = x[1]; rb.xp[2] = x[2];
    }
}

// Landmark j's side: its diagonal block as the queries read it (pll_block with the pending steps, then
// query_round), its columns of the strip (predicted when there is motion) and its mean yb, and the
// 5×5 block of the two. The columns are returned too: the joint gate's pairs need them.
struct TrialBlock {
    Block5 b5;
    double2 rr0, rr1, rr2, yb;
};
template <typename T>
__device__ __forceinline__ void trial_block(const PllView<T>& pv, bool once, bool motion, const TrialRobot& rb,
                                            const Committed& cm, int n, int j, TrialBlock& tb)
{
    double Dj[4];
    pll_block<T>(pv, 2 * j, 2 * j, Dj);
    query_round<T>(once, pv.ex, Dj);
    const int b0 = 3 + 2 * j;
    tb.rr0 = *reinterpret_cast<const double2*>(cm.Rs + b0);
    tb.rr1 = *reinterpret_cast<const double2*>(cm.Rs + n + b0);
    tb.rr2 = *reinterpret_cast<const double2*>(cm.Rs + 2 * n + b0);
    tb.yb = *reinterpret_cast<const double2*>(cm.y + b0);
    if (motion) predict_cols(rb.F3, tb.rr0, tb.rr1, tb.rr2);
    fill_block5(tb.b5, rb.R33, tb.rr0, tb.rr1, tb.rr2, Dj);
}

}  // namespace ekf
