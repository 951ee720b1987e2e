// ekf_loop_plan.h — the two pieces of the hypothesis loop (slam_ekf.h ekf_resample_plan_device,
// ekf_resample_device) that are plain sequential arithmetic over small arrays: the systematic
// resampling plan and the check of a source list. One copy each, __host__ __device__: the kernels
// (unit_loop.hip, unit_resample_device.hip) call them, and tests/cpp/loop_driver.cpp runs them on a CPU
// against ekf.resample_plan and resample_check (ekf_resample_plan.h). No HIP include, no allocation.
#pragma once

#include <stdint.h>

#include "../../include/slam_ekf.h"

#if defined(__HIPCC__)
#define EKF_LOOP_HD __host__ __device__
#else
#define EKF_LOOP_HD
#endif

namespace ekf {

// One entry of a source list: 0 acceptable, 1 its source is itself overwritten, 2 outside [0, E). An
// out-of-range entry is never used as an index (the entry it names is then not looked at either way: a
// source outside the range is reported at its own place).
EKF_LOOP_HD inline int resample_entry_code(const int32_t* src, int E, int e)
{
    const int32_t s = src[e];
    if (s < 0 || s >= E) return 2;
    const int32_t t = src[s];
    if (t < 0 || t >= E) return 0;   // (entry s reports it)
    return t != s ? 1 : 0;
}

// The whole list: the largest code of its entries, which is resample_check's answer for a list that
// exists (an entry out of range wins over a source that moves)
EKF_LOOP_HD inline int resample_list_code(const int32_t* src, int E)
{
    int code = 0;
    for (int e = 0; e < E; e++) {
        const int c = resample_entry_code(src, E, e);
        code = c > code ? c : code;
    }
    return code;
}

// the status a list's code stands for (what ekf_resample returns)
EKF_LOOP_HD inline int resample_code_status(int code) { return code == 2 ? EKF_ERANGE : code == 1 ? EKF_EINVAL : EKF_OK; }

// Systematic resampling over w[0 .. E), u in [0, 1): src[E] and *info (may be null), as slam_ekf.h states
// it. Every sum runs in ascending index order; src doubles as the scratch (the points per instance, then
// the assigned slots as −1 − source), so the function needs no memory of its own.
EKF_LOOP_HD inline void resample_plan_sequential(const double* w, int E, double u, double ess_below, int32_t* src,
                                                 ekf_plan_info* info)
{
    const double inf = __builtin_huge_val();
    bool ok = E > 0;
    double total = 0.0;
    int last = -1;   // last index with w > 0
    for (int e = 0; e < E; e++) {
        const double v = w[e];
        if (!(v >= 0.0) || v == inf) ok = false;   // negative, NaN, +inf
        total += v;
        if (v > 0.0) last = e;
    }
    if (!(total > 0.0) || total == inf) ok = false;
    double ess = 0.0;
    int status = 0, copies = 0;
    if (ok) {
        double sq = 0.0;
        for (int e = 0; e < E; e++) {
            const double q = w[e] / total;
            sq += q * q;
        }
        ess = 1.0 / sq;
        if (!(ess < ess_below)) status = EKF_RP_KEPT;
    } else {
        status = EKF_RP_INVALID;
    }
    if (status == 0) {
        // points per instance: the points ascend, so the edge they are compared with only moves on
        for (int e = 0; e < E; e++) src[e] = 0;
        int i = 0;                       // upper_bound so far: edges[0 .. i) <= the point
        double edge = w[0] / total;      // edges[i]
        for (int k = 0; k < E; k++) {
            const double p = (u + (double)k) / (double)E;
            while (i < E && !(p < edge)) {
                i++;
                if (i < E) edge += w[i] / total;
            }
            src[i < last ? i : last]++;
        }
        // slots without a point, ascending, take the surplus of the survivors, ascending
        int z = 0, s = 0;
        for (;;) {
            while (s < E && src[s] <= 1) s++;   // (an assigned slot is negative)
            if (s >= E) break;
            while (z < E && src[z] != 0) z++;
            if (z >= E) break;                  // (unreachable: E points, so as many surplus copies as empty slots)
            src[z] = -1 - s;
            src[s]--;
            copies++;
        }
        for (int e = 0; e < E; e++) src[e] = src[e] < 0 ? -1 - src[e] : e;
    } else {
        for (int e = 0; e < E; e++) src[e] = e;
    }
    if (info) {
        info->status = status;
        info->copies = copies;
        info->ess = ess;
        info->total = total;
    }
}

}  // namespace ekf
