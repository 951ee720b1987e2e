// ekf_state.hip — the calls that read or write one instance's state without a scan: reset, upload,
// download, low-rank initialisation, rescale, the storage exponent, pose covariance and ellipse. The
// core calls set_robot_ctor from here, once per instance when it creates a context.
#include <math.h>

#include <algorithm>

#include "ekf_ctx.h"
#include "ekf_ellipse.h"

// Every entry point that writes an instance's state without a scan (reset, upload, low-rank
// initialisation, rescale, and any added later) starts here: the synchronous calls' result mirror
// holds the robot block of the last scan, which the write makes stale (ekf_get_pose_cov must not
// serve it), and the write needs the materialised landmark block. The writers read or replace single
// storage exponents of the host's copy: it is brought up to date first (pexp_mirror).
static int begin_state_write(ekf_ctx* c)
{
    c->mirror_epoch = 0;
    c->predicted = 0;
    const int rc = drain(c);
    return rc ? rc : pexp_mirror(c);
}

// ... and a writer of instance e's strip, mean or landmark block goes on with the committed copy, *cb
static int begin_strip_write(ekf_ctx* c, int e, int* cb)
{
    const int rc = begin_state_write(c);
    return rc ? rc : strip_copy(c, e, cb);
}

// The dense n × n fp64 scratch of the state transfers: allocated on first use and kept, so that a
// caller mirroring P after every scan (the drop-in's full mirror) does not allocate per call
static hipError_t dense_scratch(ekf_ctx* c, double** out)
{
    if (!c->dense) {
        const hipError_t err = hipMalloc((void**)&c->dense, sizeof(double) * c->d.n * c->d.n);
        if (err != hipSuccess) {
            c->dense = nullptr;
            return err;
        }
    }
    *out = c->dense;
    return hipSuccess;
}

// fp16 storage exponent for a landmark block whose largest variance is vmax: the largest
// 2^x <= 2^10 with 2^x·vmax <= 2^12 (16× below the fp16 range, 4× below the EKF_ST_RANGE warning)
static int choose_exponent(const ekf_ctx* c, double vmax)
{
    if (c->cfg.precision != EKF_PREC_F16) return 0;
    if (!(vmax > 0.0) || !std::isfinite(vmax)) return ekf::F16_EXP_DEFAULT;
    const int x = (int)std::floor(std::log2(4096.0 / vmax));
    return std::max(-24, std::min(ekf::F16_EXP_DEFAULT, x));
}

// What instance e keeps of its largest landmark variance vmax: the storage exponent (ex, or chosen
// from vmax: EKF_EXP_AUTO) and the EKF_ARITH_F16X3 plane exponent (every context keeps it; only F16X3
// reads it)
static int set_scales(ekf_ctx* c, int e, double vmax, int ex)
{
    if (ex == EKF_EXP_AUTO) ex = choose_exponent(c, vmax);
    c->pexp_h[e] = ex;
    HIP_TRY(hipMemcpy(c->pexp + e, &ex, sizeof(int), hipMemcpyHostToDevice));
    const int sg = ekf::plane_sigma(vmax);
    const double vm = (vmax > 0.0 && std::isfinite(vmax)) ? vmax : 0.0;
    HIP_TRY(hipMemcpy(c->psig + e, &sg, sizeof(int), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->pvmax + e, &vm, sizeof(double), hipMemcpyHostToDevice));
    return EKF_OK;
}

int set_robot_ctor(ekf_ctx* c, int e, double x, double y, double th)
{
    // Robot::Robot (Robot.cpp:20-35): P_t0[0][0] = P_t0[1][1] = 0.05, P_t0[2][2] = 0, the rest
    // (and y, savedLineCount) zero.
    const Dims& d = c->d;
    HIP_TRY(hipMemsetAsync(xinst_ptr(c, cur_buf(c), e), 0, c->xinst * c->elem, c->stream));
    const int zero = 0;
    const double v = 0.05;
    HIP_TRY(hipMemcpyAsync(c->cur + e, &zero, sizeof(int), hipMemcpyHostToDevice, c->stream));
    for (int cb = 0; cb < 2; cb++) {
        HIP_TRY(hipMemsetAsync(strip_of(c, cb, e), 0, sizeof(double) * 3 * d.n, c->stream));
        HIP_TRY(hipMemsetAsync(mean_of(c, cb, e), 0, sizeof(double) * d.n, c->stream));
        HIP_TRY(hipMemcpyAsync(strip_of(c, cb, e) + 0, &v, sizeof(double), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(strip_of(c, cb, e) + d.n + 1, &v, sizeof(double), hipMemcpyHostToDevice,
                               c->stream));
    }
    const double pose[3] = {x, y, th};
    HIP_TRY(hipMemcpyAsync(c->pose + 3 * e, pose, sizeof(pose), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->xpre + 3 * e, pose, sizeof(pose), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->saved + e, &zero, sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return set_scales(c, e, 0.0, EKF_EXP_AUTO);   // an empty map
}

extern "C" int ekf_reset_instance(ekf_ctx* c, int e, double x, double y, double th)
{
    if (!c) return EKF_EINVAL;
    if (e >= c->cfg.instances) return EKF_ERANGE;
    int rc = begin_state_write(c);
    if (rc) return rc;
    if (e < 0) {
        for (int k = 0; k < c->cfg.instances; k++) {
            rc = set_robot_ctor(c, k, x, y, th);
            if (rc) return rc;
        }
        return EKF_OK;
    }
    return set_robot_ctor(c, e, x, y, th);
}

extern "C" int ekf_upload_state(ekf_ctx* c, int e, const double* P, const double* y, int saved,
                                const double pose[3])
{
    if (!c) return EKF_EINVAL;
    if (e < 0 || e >= c->cfg.instances) return EKF_ERANGE;
    if (saved < 0 || saved > c->d.N) return EKF_ERANGE;
    int cb = 0;
    int rc = begin_strip_write(c, e, &cb);
    if (rc) return rc;
    const Dims& d = c->d;
    if (P) {
        double vmax = 0.0;
        for (int i = 3; i < d.n; i++) vmax = std::max(vmax, std::fabs(P[(size_t)i * d.n + i]));
        rc = set_scales(c, e, vmax, EKF_EXP_AUTO);
        if (rc) return rc;
        double* tmp = nullptr;
        HIP_TRY(dense_scratch(c, &tmp));
        hipError_t err = hipMemcpyAsync(tmp, P, sizeof(double) * d.n * d.n, hipMemcpyHostToDevice,
                                        c->stream);
        if (err == hipSuccess)
            err = ekf::launch_pack(d, c->cfg.precision, tmp, xinst_ptr(c, cur_buf(c), e),
                                   strip_of(c, cb, e), c->tile_rc, c->pexp_h[e], c->stream, c->t0, c->t1);
        if (err == hipSuccess) err = hipStreamSynchronize(c->stream);
        HIP_TRY(err);
    }
    if (y)
        HIP_TRY(hipMemcpyAsync(mean_of(c, cb, e), y, sizeof(double) * d.n,
                               hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->saved + e, &saved, sizeof(int), hipMemcpyHostToDevice, c->stream));
    if (pose) {
        HIP_TRY(hipMemcpyAsync(c->pose + 3 * e, pose, sizeof(double) * 3, hipMemcpyHostToDevice,
                               c->stream));
        HIP_TRY(hipMemcpyAsync(c->xpre + 3 * e, pose, sizeof(double) * 3, hipMemcpyHostToDevice,
                               c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    return EKF_OK;
}

extern "C" int ekf_download_state(ekf_ctx* c, int e, double* P, double* y, int* saved,
                                  double pose[3])
{
    if (!c) return EKF_EINVAL;
    if (e < 0 || e >= c->cfg.instances) return EKF_ERANGE;
    // P drains (the pending downdates are flushed first); the mean, pose and savedLineCount are
    // committed by every association kernel, so without P the call only waits for the stream and
    // leaves the flush schedule as it is
    int rc = EKF_OK;
    if (P) rc = drain(c);
    else HIP_TRY(hipStreamSynchronize(c->stream));
    if (!rc && P) rc = pexp_mirror(c);
    if (rc) return rc;
    const Dims& d = c->d;
    int cb = 0;
    rc = strip_copy(c, e, &cb);
    if (rc) return rc;
    if (P) {
        double* tmp = nullptr;
        HIP_TRY(dense_scratch(c, &tmp));
        hipError_t err = ekf::launch_unpack(d, c->cfg.precision, tmp, xinst_ptr(c, cur_buf(c), e),
                                            strip_of(c, cb, e), c->pexp_h[e], c->stream, c->t0, c->t1);
        if (err == hipSuccess)
            err = hipMemcpyAsync(P, tmp, sizeof(double) * d.n * d.n, hipMemcpyDeviceToHost,
                                 c->stream);
        if (err == hipSuccess) err = hipStreamSynchronize(c->stream);
        HIP_TRY(err);
    }
    if (y)
        HIP_TRY(hipMemcpyAsync(y, mean_of(c, cb, e), sizeof(double) * d.n,
                               hipMemcpyDeviceToHost, c->stream));
    if (saved)
        HIP_TRY(hipMemcpyAsync(saved, c->saved + e, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if (pose)
        HIP_TRY(hipMemcpyAsync(pose, c->pose + 3 * e, sizeof(double) * 3, hipMemcpyDeviceToHost,
                               c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return EKF_OK;
}

extern "C" int ekf_init_lowrank(ekf_ctx* c, int e, const double* diag, const double* U, int rank,
                                const double* y, int saved, const double pose[3])
{
    if (!c || !diag || (rank > 0 && !U) || rank < 0) return EKF_EINVAL;
    if (e < 0 || e >= c->cfg.instances) return EKF_ERANGE;
    int cb = 0;
    int rc = begin_strip_write(c, e, &cb);
    if (rc) return rc;
    const Dims& d = c->d;
    double vmax = 0.0;
    for (int i = 3; i < d.n; i++) {
        double v = diag[i];
        for (int k = 0; k < rank; k++) v += U[(size_t)i * rank + k] * U[(size_t)i * rank + k];
        vmax = std::max(vmax, std::fabs(v));
    }
    rc = set_scales(c, e, vmax, EKF_EXP_AUTO);
    if (rc) return rc;
    double *dd = nullptr, *du = nullptr;
    HIP_TRY(hipMalloc((void**)&dd, sizeof(double) * d.n));
    hipError_t err = hipMalloc((void**)&du, sizeof(double) * d.n * (rank > 0 ? rank : 1));
    if (err == hipSuccess)
        err = hipMemcpyAsync(dd, diag, sizeof(double) * d.n, hipMemcpyHostToDevice, c->stream);
    if (err == hipSuccess && rank > 0)
        err = hipMemcpyAsync(du, U, sizeof(double) * d.n * rank, hipMemcpyHostToDevice, c->stream);
    if (err == hipSuccess)
        err = ekf::launch_lowrank(d, c->cfg.precision, dd, du, rank, xinst_ptr(c, cur_buf(c), e),
                                  strip_of(c, cb, e), c->tile_rc, c->pexp_h[e], c->stream, c->t0, c->t1);
    if (err == hipSuccess) err = hipStreamSynchronize(c->stream);
    (void)hipFree(dd);
    if (du) (void)hipFree(du);
    HIP_TRY(err);
    return ekf_upload_state(c, e, nullptr, y, saved, pose);
}

extern "C" int ekf_storage_exponent(const ekf_ctx* c, int e)
{
    if (!c) return 0;
    if (e < 0 || e >= c->cfg.instances) return 0;
    // (after ekf_resample_device the host's copy is re-read from the device: a wait for the stream)
    if (pexp_mirror(const_cast<ekf_ctx*>(c)) != EKF_OK) return 0;
    return c->pexp_h[e];
}

extern "C" int ekf_rescale(ekf_ctx* c, int e, int ex)
{
    if (!c) return EKF_EINVAL;
    if (e < 0 || e >= c->cfg.instances) return EKF_ERANGE;
    if (c->cfg.precision != EKF_PREC_F16) return EKF_OK;
    if (ex != EKF_EXP_AUTO && (ex < -24 || ex > 24)) return EKF_ERANGE;
    int cb = 0;
    int rc = begin_strip_write(c, e, &cb);
    if (rc) return rc;
    const Dims& d = c->d;
    void* X = xinst_ptr(c, cur_buf(c), e);
    double* Rs = strip_of(c, cb, e);
    double* tmp = nullptr;
    HIP_TRY(dense_scratch(c, &tmp));
    std::vector<double> dg(d.n);
    hipError_t err = ekf::launch_unpack(d, c->cfg.precision, tmp, X, Rs, c->pexp_h[e], c->stream);
    if (err == hipSuccess)   // the diagonal of the dense copy (stride n + 1)
        err = hipMemcpy2DAsync(dg.data(), sizeof(double), tmp, sizeof(double) * (d.n + 1), sizeof(double),
                               d.n, hipMemcpyDeviceToHost, c->stream);
    if (err == hipSuccess) err = hipStreamSynchronize(c->stream);
    if (err == hipSuccess) {
        double vmax = 0.0;
        for (int i = 3; i < d.n; i++) vmax = std::max(vmax, std::fabs(dg[i]));
        rc = set_scales(c, e, vmax, ex);
        if (rc == EKF_OK) {
            err = ekf::launch_pack(d, c->cfg.precision, tmp, X, Rs, c->tile_rc, c->pexp_h[e], c->stream);
            if (err == hipSuccess) err = hipStreamSynchronize(c->stream);
        }
    }
    HIP_TRY(err);
    return rc;
}

extern "C" int ekf_get_pose_cov(ekf_ctx* c, int e, double P33[9])
{
    if (!c || !P33) return EKF_EINVAL;
    if (e < 0 || e >= c->cfg.instances) return EKF_ERANGE;
    if (c->mirror_epoch != 0 && c->mirror_epoch == c->scan_epoch) {
        // the robot block the last synchronous call's scan committed (no launch since)
        memcpy(P33, c->h_r33 + 9 * (size_t)e, sizeof(double) * 9);
        return EKF_OK;
    }
    const Dims& d = c->d;
    int cb = 0;
    const int rc = strip_copy(c, e, &cb);
    if (rc) return rc;
    for (int a = 0; a < 3; a++)
        HIP_TRY(hipMemcpyAsync(P33 + 3 * a, strip_of(c, cb, e) + (size_t)a * d.n,
                               sizeof(double) * 3, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return EKF_OK;
}

extern "C" int ekf_ellipse_of_block(const double P22[4], float axii[2], float* angle)
{
    if (!P22 || !axii || !angle) return -EKF_EINVAL;
    return ekf::gsl_ellipse_2x2(P22, axii, angle);
}

extern "C" int ekf_get_ellipse(ekf_ctx* c, int e, float axii[2], float* angle)
{
    // Robot::getEllipse (Robot.cpp:73-124) on P_t0[0:2, 0:2] of instance e (ekf_ellipse.h)
    if (!c || !axii || !angle) return -EKF_EINVAL;
    double P33[9];
    int rc = ekf_get_pose_cov(c, e, P33);
    if (rc) return -rc;
    const double P22[4] = {P33[0], P33[1], P33[3], P33[4]};
    return ekf::gsl_ellipse_2x2(P22, axii, angle);
}

extern "C" size_t ekf_landmark_block_bytes(const ekf_ctx* c)
{
    return c ? c->xinst * c->elem : 0;
}

extern "C" int ekf_state_dim(const ekf_ctx* c) { return c ? c->d.n : 0; }
