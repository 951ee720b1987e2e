// ekf_joint_parts.h — the pieces of the stacked innovation covariance S of a hypothesis that depend on one
// (line, landmark) pairing or on two of them: the joint gate (unit_joint.hip) and the joint-compatibility
// search (unit_assoc.hip) build S from these, one copy, so that both see the same bits.
//   joint_line   the pairing exactly as the gate evaluates it (ekf_gate.h: trial_robot, trial_block,
//                line_R, eval_candidate): v, H, the diagonal 2×2 block of S with R, its own d2; and what a
//                pair needs of it: H row 1, G = H·P[:, 0:3] (innovation_cov's hp rows), the predicted strip
//                columns C of its landmark
//   joint_pair   the 2×2 block S_ab = G_a·A_bᵀ + Q_ab·B_bᵀ of a pairing a on a later line against b on an
//                earlier one, Q_ab = A_a·C_b + B_a·D_ab, H = [A | B] on the columns {0, 1, 2 | l, l + 1},
//                D_ab = P[l_a, l_b] read in its stored orientation. Every sum is written out in
//                innovation_cov's order (for a = b it is that function's expression)
#pragma once

#include "ekf_gate.h"

namespace ekf {

enum { JL_H10 = 0, JL_H11, JL_H1L, JL_G = 3 /* [2][3] */, JL_C = 9 /* [3][2] */, JL_WORDS = 15 };

// line i of launch row `row` (instance e) on landmark j: the candidate c (c.S the diagonal block, c.v, c.d2)
// and the pairing's words w[JL_WORDS]
template <typename T>
__device__ __forceinline__ void joint_line(const PllView<T>& pv, bool once, const TrialLines& t, const Committed& cm,
                                           const Dims& d, int e, int row, int i, int j, Cand& c, double* w)
{
    TrialRobot rb;
    trial_robot(t, e, row, cm.Rs, d.n, rb);
    TrialBlock tb;
    trial_block<T>(pv, once, t.enc != nullptr, rb, cm, d.n, j, tb);
    double sn, cs;
    sincos(tb.yb.x, &sn, &cs);
    const ekf_line ln = t.lines[(size_t)row * d.max_lines + i];
    double Rm[4];
    line_R(ln, i, t.r_mode, Rm);
    eval_candidate<true>(tb.b5, tb.yb.x, tb.yb.y, sn, cs, rb.xp, ln.alpha, ln.r, Rm, t.gate, gate_eta<T>(), c);
    double S[4], hp0[5], hp1[5];
    innovation_cov(tb.b5, c.h10, c.h11, c.h1l, Rm, S, hp0, hp1);   // (S == c.S; the hp rows are G)
    w[JL_H10] = c.h10; w[JL_H11] = c.h11; w[JL_H1L] = c.h1l;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        w[JL_G + k] = hp0[k];
        w[JL_G + 3 + k] = hp1[k];
    }
    w[JL_C + 0] = tb.rr0.x; w[JL_C + 1] = tb.rr0.y;
    w[JL_C + 2] = tb.rr1.x; w[JL_C + 3] = tb.rr1.y;
    w[JL_C + 4] = tb.rr2.x; w[JL_C + 5] = tb.rr2.y;
}

// S_ab ([2][2], row-major) of pairing a (landmark la, words wa) against pairing b on an earlier line
template <typename T>
__device__ __forceinline__ void joint_pair(const PllView<T>& pv, bool once, int la, int lb, const double* wa,
                                           const double* wb, double Sab[4])
{
    double Dab[4];
    pll_block<T>(pv, 2 * la, 2 * lb, Dab);   // P[l_a, l_b] (transposed on read if stored so)
    query_round<T>(once, pv.ex, Dab);
    const double h10 = wa[JL_H10], h11 = wa[JL_H11], h1l = wa[JL_H1L];
    const double* C = wb + JL_C;   // P[k, l_b + c] at C[2k + c]
    // Q_ab = H_a·P[:, l_b : l_b + 2] past the robot rows (innovation_cov's hp[3], hp[4])
    const double q00 = -C[4] + Dab[0];
    const double q01 = -C[5] + Dab[1];
    const double q10 = h10 * C[0] + h11 * C[2] + h1l * Dab[0] + Dab[2];
    const double q11 = h10 * C[1] + h11 * C[3] + h1l * Dab[1] + Dab[3];
    const double* G = wa + JL_G;
    const double g10 = wb[JL_H10], g11 = wb[JL_H11], g1l = wb[JL_H1L];
    Sab[0] = -G[2] + q00;
    Sab[1] = G[0] * g10 + G[1] * g11 + q00 * g1l + q01;
    Sab[2] = -G[5] + q10;
    Sab[3] = G[3] * g10 + G[4] * g11 + q10 * g1l + q11;
}

}  // namespace ekf
