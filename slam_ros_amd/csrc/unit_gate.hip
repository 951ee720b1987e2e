// unit_gate.hip — trial lines scored against the map without touching the state (ekf_gate_lines,
// ekf_gate_lines_device).
//
// Every line is gated on its own against every saved landmark, as the first line of a scan would be
// (Robot.cpp:313-498): no sequential update between the lines, no "already matched" skip. The
// candidate arithmetic is the association's (ekf_gate.h: eval_candidate, cand_amb, line_R); the
// landmark blocks are read as unit_query.hip reads them (pll_block with the pending steps, then
// query_round), the robot strip, the mean and the pose from the committed copies. With an encoder
// pose the predict (Robot.cpp:130-286) is applied on read. Two plain launches, no cross-workgroup
// wait, no atomics: the results do not depend on the schedule.
//   gate_pass1_kernel  a thread owns landmark j: its 5×5 block once, then every line; d2[i][j], the
//                      candidate's flag byte, and per wave and line a partial record (GatePart)
//   gate_pass2_kernel  one wave per instance and line: combines the partials into the hit record
#include "ekf_gate.h"

namespace ekf {

// the lowest lane of a wave's ballot, or 64
__device__ __forceinline__ int first_lane(unsigned long long m) { return m ? __ffsll((long long)m) - 1 : 64; }

// the candidate a wave's or an instance's record keeps: distance, S, v
__device__ __forceinline__ void keep_cand(double (&dst)[7], const Cand& c)
{
    dst[0] = c.d2;
#pragma unroll
    for (int k = 0; k < 4; k++) dst[1 + k] = c.S[k];
    dst[5] = c.v[0];
    dst[6] = c.v[1];
}

template <typename T>
__global__ __launch_bounds__(GATE_THREADS) void gate_pass1_kernel(GateParams p)
{
    __shared__ int4 sh_ctl[PMAX];
    __shared__ ekf_line sh_lines[EKF_MAX_LINES];
    const int tid = threadIdx.x;
    const int row = blockIdx.y;        // the launch's row: lines and outputs
    const int e = p.e0 + row;          // the instance
    const Dims d = p.v.d;
    const int L = trial_count(p.t, row, d.max_lines);
    if (L <= 0) return;   // (uniform)
    view_ctl(p.v, p.pend, e, sh_ctl);
    {
        const double* src = reinterpret_cast<const double*>(p.t.lines + (size_t)row * d.max_lines);
        double* dst = reinterpret_cast<double*>(sh_lines);
        for (int k = tid; k < L * 6; k += GATE_THREADS) dst[k] = src[k];
    }
    __syncthreads();

    const int j = (int)blockIdx.x * GATE_THREADS + tid;   // the owned landmark
    const int wv = j >> 6;                                // its wave's partial record
    if ((j & ~63) >= d.N) return;                         // (a wave past the map: wave-uniform)
    const int saved = min(max(p.t.saved[e], 0), d.N);
    const bool cand = j < saved;
    const Committed cm = view_committed(p.v, e);
    TrialRobot rb;
    trial_robot(p.t, e, row, cm.Rs, d.n, rb);

    TrialBlock tb;
    double ma = 0.0, mr = 0.0, sn = 0.0, cs = 1.0;
    if (cand) {
        trial_block<T>(view_pll<T>(p.v, p.pend, e, sh_ctl), p.v.bf != 0, p.t.enc != nullptr, rb, cm, d.n, j, tb);
        ma = tb.yb.x;
        mr = tb.yb.y;
        sincos(ma, &sn, &cs);
    }

    const double eta = gate_eta<T>();
    const double inf = __builtin_inf();
    const int lane = tid & 63;
    for (int i = 0; i < L; i++) {
        const size_t li = (size_t)row * d.max_lines + i;
        Cand c;
        int pass = 0, fl = 0;
        double an = inf;   // |d2|; +inf: no candidate or a NaN distance (never the nearest)
        if (cand) {
            double Rm[4];
            line_R(sh_lines[i], i, p.t.r_mode, Rm);
            eval_candidate<true>(tb.b5, ma, mr, sn, cs, rb.xp, sh_lines[i].alpha, sh_lines[i].r, Rm, p.t.gate, eta, c);
            pass = c.pass;
            fl = (c.singular ? GATE_FL_SINGULAR : 0) | (c.amb ? GATE_FL_AMB : 0);
            const double a = fabs(c.d2);
            if (a == a) an = a;
        }
        if (j < d.N) {
            if (p.d2) p.d2[li * d.N + j] = cand ? c.d2 : inf;
            p.flags[li * d.N + j] = (unsigned char)fl;
        }
        // the wave's partial: its first passing lane, its pass count, its nearest candidate (the
        // lowest lane among those at the smallest |d2|; a finite |d2| only, or none)
        const unsigned long long mp = __ballot(pass);
        double best = an;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) best = fmin(best, __shfl_xor(best, off, 64));
        const unsigned long long mn = __ballot(cand && an == best && best < inf);
        const int lf = first_lane(mp), ln = first_lane(mn);
        GatePart* part = p.part + li * gate_waves(d.N) + wv;
        if (lane == 0) {
            part->first = lf < 64 ? (j + lf) : -1;
            part->nearest = ln < 64 ? (j + ln) : -1;
            part->npass = __popcll(mp);
            part->pad = 0;
        }
        if (lane == lf) keep_cand(part->cf, c);
        if (lane == ln) keep_cand(part->cn, c);
    }
}

// One wave per (line, instance row): the partials of the line's waves, in landmark order
__global__ __launch_bounds__(64) void gate_pass2_kernel(GateParams p)
{
    const int lane = threadIdx.x;
    const int i = blockIdx.x;
    const int row = blockIdx.y;
    const int e = p.e0 + row;
    const Dims d = p.v.d;
    const int L = trial_count(p.t, row, d.max_lines);
    const size_t li = (size_t)row * d.max_lines + i;
    ekf_gate_hit* hit = p.hits + li;
    const double nan = __builtin_nan("");
    const double inf = __builtin_inf();
    ekf_gate_hit h;
    h.first = h.nearest = -1;
    h.npass = 0;
    h.status = 0;
    h.d2_first = h.d2_nearest = nan;
    h.S[0] = h.S[1] = h.S[2] = h.S[3] = 0.0;
    h.v[0] = h.v[1] = 0.0;
    if (i >= L) {   // (uniform) an unused entry of the device form
        if (lane == 0) *hit = h;
        return;
    }
    const int saved = min(max(p.t.saved[e], 0), d.N);
    const GatePart* part = p.part + li * gate_waves(d.N);
    const int nwu = (saved + 63) >> 6;   // the waves that held a candidate
    int wf = 0x7fffffff, wn = 0x7fffffff, np = 0;
    double best = inf;
    for (int w = lane; w < nwu; w += 64) {
        const GatePart& q = part[w];
        if (q.first >= 0 && w < wf) wf = w;
        np += q.npass;
        if (q.nearest >= 0) {
            const double a = fabs(q.cn[0]);
            if (a < best) {   // (w ascending within a lane: the lowest wave on ties)
                best = a;
                wn = w;
            }
        }
    }
    double ball = best;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        wf = min(wf, __shfl_xor(wf, off, 64));
        np += __shfl_xor(np, off, 64);
        ball = fmin(ball, __shfl_xor(ball, off, 64));
    }
    if (!(best == ball && ball < inf)) wn = 0x7fffffff;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) wn = min(wn, __shfl_xor(wn, off, 64));
    const bool hasf = wf != 0x7fffffff, hasn = wn != 0x7fffffff;
    const int first = hasf ? part[wf].first : -1;
    // the flags of the candidates the reference evaluates for this line: 0 .. first, or all
    const int upto = hasf ? first + 1 : saved;
    const unsigned char* fl = p.flags + li * d.N;
    int f = 0;
    for (int j = lane; j < upto; j += 64) f |= fl[j];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) f |= __shfl_xor(f, off, 64);
    if (lane != 0) return;
    h.npass = np;
    h.status = ((f & GATE_FL_SINGULAR) ? EKF_ST_SINGULAR_S : 0) | ((f & GATE_FL_AMB) ? EKF_ST_PRECISION : 0);
    if (hasf) {
        h.first = first;
        h.d2_first = part[wf].cf[0];
    }
    if (hasn) {
        h.nearest = part[wn].nearest;
        h.d2_nearest = part[wn].cn[0];
    }
    const double* src = hasf ? part[wf].cf : hasn ? part[wn].cn : nullptr;
    if (src) {
#pragma unroll
        for (int k = 0; k < 4; k++) h.S[k] = src[1 + k];
        h.v[0] = src[5];
        h.v[1] = src[6];
    }
    *hit = h;
}

hipError_t launch_gate(const GateParams& p, int precision, hipStream_t st)
{
    const Dims& d = p.v.d;
    if (p.E < 1 || p.v.npend < 0 || p.v.npend > PMAX || p.t.L < 0 || p.t.L > d.max_lines || d.max_lines > EKF_MAX_LINES ||
        !p.hits || !p.flags || !p.part)
        return hipErrorInvalidValue;
    const int rows = p.t.nlines ? d.max_lines : p.t.L;   // hit records per instance
    if (rows == 0) return hipSuccess;
    const dim3 g1((unsigned)((d.N + GATE_THREADS - 1) / GATE_THREADS), (unsigned)p.E);
    if (precision == EKF_PREC_F64) hipLaunchKernelGGL(gate_pass1_kernel<double>, g1, dim3(GATE_THREADS), 0, st, p);
    else if (precision == EKF_PREC_F32) hipLaunchKernelGGL(gate_pass1_kernel<float>, g1, dim3(GATE_THREADS), 0, st, p);
    else if (precision == EKF_PREC_F16) hipLaunchKernelGGL(gate_pass1_kernel<_Float16>, g1, dim3(GATE_THREADS), 0, st, p);
    else return hipErrorInvalidValue;
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(gate_pass2_kernel, dim3((unsigned)rows, (unsigned)p.E), dim3(64), 0, st, p);
    return hipGetLastError();
}

}  // namespace ekf
