// ekf_pairs.h — the all-pairs gate over the map (slam_ekf.h ekf_gate_landmarks): the launch parameters
// and the one expression that scores a pair of saved landmarks, the Mahalanobis distance of their
// difference in the same-direction and in the flipped form. unit_pairs.hip's two kernels call pair_eval
// for every pair; ekf_read.hip fills PairParams.
#pragma once

#include "ekf_device.h"

// The pair's arithmetic contracts a·b + c only within one source expression (as ekf_gate.h), so that
// pair_eval rounds alike wherever it is inlined: d2[a][b] and d2[b][a] come from the same bits.
#pragma clang fp contract(on)

namespace ekf {

// Every pair of saved landmarks of an instance (unit_pairs.hip). Hit records and distances are per launch
// row; part is the context's scratch: per (landmark, 64-landmark partner block) the landmark's record
// against that block alone, in ekf_pair_hit's own layout.
constexpr int PAIR_THREADS = 256;   // pass 1: four waves, sixteen row landmarks each, 64 column landmarks wide
constexpr int PAIR_BLOCK = 64;      // landmarks per block of the pair grid
constexpr int PAIR_BATCH = 4;       // row landmarks per pll_blocks call
constexpr int pair_blocks(int N) { return (N + PAIR_BLOCK - 1) / PAIR_BLOCK; }
struct PairParams {
    ReadView v;
    double gate;
    const int* saved;     // [Etot]
    int E;                // instances in this launch (grid.y)
    int e0;               // first instance of this launch
    ekf_pair_hit* hits;   // [E][N]
    double* d2;           // [E][N][N] or nullptr
    ekf_pair_hit* part;   // [E][N][pair_blocks(N)]
    Slot pend[PMAX];      // (ReadView)
};
hipError_t launch_pairs(const PairParams& p, int precision, hipStream_t st);

// One pair (lo < hi) as evaluated: the distance, the form that won (flip) and its C = (c00, c01, c11), δ
struct PairVal {
    double d2;
    double C[3], delta[2];
    int flip;       // the value is the flipped form's
    int singular;   // both forms NaN
};

// The distance of one form: Cholesky of C in a fixed order; NaN where a pivot is <= 0 or not finite
__device__ __forceinline__ double pair_form(double c00, double c01, double c11, double d0, double d1)
{
    const double nan = __builtin_nan("");
    if (!(c00 > 0.0) || c00 - c00 != 0.0) return nan;
    const double l00 = sqrt(c00);
    const double l10 = c01 / l00;
    const double t = c11 - l10 * l10;
    if (!(t > 0.0) || t - t != 0.0) return nan;
    const double l11 = sqrt(t);
    const double z0 = d0 / l00;
    const double z1 = (d1 - l10 * z0) / l11;
    return z0 * z0 + z1 * z1;
}

// Landmarks lo < hi: their diagonal blocks Dlo, Dhi, X = P[lo, hi] (all as the queries read them) and
// their means (α, r). Same direction: lo − hi; flipped: hi taken as (α_hi + π, −r_hi), F = diag(1, −1).
// Additions and the IEEE remainder only up to C and δ, so these are reproducible bit for bit anywhere.
__device__ __forceinline__ void pair_eval(const double Dlo[4], const double Dhi[4], const double X[4], double2 ylo,
                                          double2 yhi, PairVal& o)
{
    const double c00 = (Dlo[0] + Dhi[0]) - (X[0] + X[0]);
    const double s01 = (Dlo[1] + Dhi[1]) - (X[1] + X[2]);
    const double s11 = (Dlo[3] + Dhi[3]) - (X[3] + X[3]);
    const double f01 = (Dlo[1] - Dhi[1]) + (X[1] - X[2]);
    const double f11 = (Dlo[3] + Dhi[3]) + (X[3] + X[3]);
    const double da = ylo.x - yhi.x;
    const double s0 = remainder(da, 2.0 * EKF_PI), s1 = ylo.y - yhi.y;
    const double f0 = remainder(da - EKF_PI, 2.0 * EKF_PI), f1 = ylo.y + yhi.y;
    const double ds = pair_form(c00, s01, s11, s0, s1);
    const double df = pair_form(c00, f01, f11, f0, f1);
    const bool same = df != df || ds <= df;
    o.flip = same ? 0 : 1;
    o.d2 = same ? ds : df;
    o.singular = o.d2 != o.d2;
    o.C[0] = c00;
    o.C[1] = same ? s01 : f01;
    o.C[2] = same ? s11 : f11;
    o.delta[0] = same ? s0 : f0;
    o.delta[1] = same ? s1 : f1;
}

}  // namespace ekf
