// ekf_ellipse.h — Robot::getEllipse (Robot.cpp:73-124) on the 2×2 pose block. Host only (no HIP include,
// no context): ekf_state.hip serves ekf_ellipse_of_block / ekf_get_ellipse from it; tests/test_ellipse.py
// checks it bit for bit against the oracle's restatement, so the operation order below is part of it.
// The reference calls gsl_eigen_nonsymmv on [[P00, P01], [P10, P11]] (GSL is not vendored and its
// version is unpinned, CMakeLists.txt:43-51), sorts with GSL_EIGEN_SORT_ABS_ASC and publishes
// atan2(Re v0, Re v1) of the eigenvector of the larger |λ|. Restated from GSL's published
// algorithm (gsl/eigen/nonsymmv.c with its defaults: no balancing; gsl/eigen/francis.c):
//   * a 2×2 matrix is already Hessenberg (Z = I); the Francis QR of a 2×2 block is the
//     standardisation francis_schur_standardize (LAPACK dlanv2): [a b; c d] = Z [a' b'; 0 d'] Zᵀ
//     with Z = [[cs, -sn], [sn, cs]] (gsl_blas_drot applied to the columns of I);
//   * right eigenvectors of the Schur form by back substitution, x = (1, 0) for a' and
//     x = (-b'/(a'-d'), 1) for d' (denominator floored at smin), back-transformed v = Z·x and
//     scaled to unit 2-norm (gslcblas dnrm2) — positive scalings only, so the sign is Z's;
//   * eigenvalues in diagonal order (a', d'), then sorted by |λ| ascending (selection sort,
//     ties keep their order).
// A complex pair (c' != 0: not produced by a symmetric covariance block) returns 0.
#pragma once

#include <math.h>

namespace ekf {

static inline double gsl_sign(double x) { return x >= 0.0 ? 1.0 : -1.0; }

static inline double gsl_hypot_(double x, double y)
{
    const double xa = fabs(x), ya = fabs(y);
    const double mn = xa < ya ? xa : ya, mx = xa < ya ? ya : xa;
    if (mn == 0.0) return mx;
    const double u = mn / mx;
    return mx * sqrt(1.0 + u * u);
}

static inline double cblas_dnrm2_2(double x0, double x1)
{
    double scale = 0.0, ssq = 1.0;
    const double xs[2] = {x0, x1};
    for (int i = 0; i < 2; i++) {
        if (xs[i] != 0.0) {
            const double ax = fabs(xs[i]);
            if (scale < ax) {
                ssq = 1.0 + ssq * (scale / ax) * (scale / ax);
                scale = ax;
            } else {
                ssq += (ax / scale) * (ax / scale);
            }
        }
    }
    return scale * sqrt(ssq);
}

static inline int gsl_ellipse_2x2(const double P[4], float axii[2], float* angle)
{
    for (int k = 0; k < 4; k++)
        if (!isfinite(P[k])) return 0;
    double a = P[0], b = P[1], c = P[2], d = P[3];
    double cs, sn;
    const double eps = 2.220446049250313e-16;   // GSL_DBL_EPSILON
    if (c == 0.0) {
        cs = 1.0;
        sn = 0.0;
    } else if (b == 0.0) {
        cs = 0.0;
        sn = 1.0;
        const double t = d;
        d = a;
        a = t;
        b = -c;
        c = 0.0;
    } else if ((a - d) == 0.0 && gsl_sign(b) != gsl_sign(c)) {
        cs = 1.0;
        sn = 0.0;
    } else {
        const double tmp = a - d;
        double p = 0.5 * tmp;
        const double bcmax = fmax(fabs(b), fabs(c));
        const double bcmis = fmin(fabs(b), fabs(c)) * gsl_sign(b) * gsl_sign(c);
        const double scale = fmax(fabs(p), bcmax);
        double z = (p / scale) * p + (bcmax / scale) * bcmis;
        if (z >= 4.0 * eps) {
            z = p + gsl_sign(p) * fabs(sqrt(scale) * sqrt(z));
            a = d + z;
            d -= (bcmax / z) * bcmis;
            const double tau = gsl_hypot_(c, z);
            cs = z / tau;
            sn = c / tau;
            b -= c;
            c = 0.0;
        } else {
            const double sigma = b + c;
            const double tau = gsl_hypot_(sigma, tmp);
            cs = sqrt(0.5 * (1.0 + fabs(sigma) / tau));
            sn = -(p / (tau * cs)) * gsl_sign(sigma);
            const double aa = a * cs + b * sn, bb = -a * sn + b * cs;
            const double cc = c * cs + d * sn, dd = -c * sn + d * cs;
            a = aa * cs + cc * sn;
            b = bb * cs + dd * sn;
            c = -aa * sn + cc * cs;
            d = -bb * sn + dd * cs;
            const double t2 = 0.5 * (a + d);
            a = d = t2;
            if (c != 0.0) {
                if (b != 0.0) {
                    if (gsl_sign(b) == gsl_sign(c)) {
                        const double sab = sqrt(fabs(b)), sac = sqrt(fabs(c));
                        p = gsl_sign(c) * fabs(sab * sac);
                        const double tau2 = 1.0 / sqrt(fabs(b + c));
                        a = t2 + p;
                        d = t2 - p;
                        b -= c;
                        c = 0.0;
                        const double cs1 = sab * tau2, sn1 = sac * tau2;
                        const double t3 = cs * cs1 - sn * sn1;
                        sn = cs * sn1 + sn * cs1;
                        cs = t3;
                    }
                } else {
                    b = -c;
                    c = 0.0;
                    const double t3 = cs;
                    cs = -sn;
                    sn = t3;
                }
            }
        }
    }
    if (c != 0.0) return 0;   // complex pair
    // eigenvectors: Z = [[cs, -sn], [sn, cs]]
    double v[2][2];
    v[0][0] = cs;
    v[0][1] = sn;
    {
        const double smlnum = 2.2250738585072014e-308 * (2.0 / eps);
        const double smin = fmax(eps * fabs(d), smlnum);
        double den = a - d;
        if (fabs(den) < smin) den = smin;
        const double x0 = -b / den;
        v[1][0] = x0 * cs + (-sn);
        v[1][1] = x0 * sn + cs;
    }
    for (int k = 0; k < 2; k++) {
        // back substitution ends with a max-norm scaling (as LAPACK dtrevc), the workspace
        // normalises to unit 2-norm afterwards (nonsymmv_normalize_eigenvectors)
        const double emax = fmax(fabs(v[k][0]), fabs(v[k][1]));
        if (emax > 0.0) {
            const double remax = 1.0 / emax;
            v[k][0] *= remax;
            v[k][1] *= remax;
        }
        const double nr = cblas_dnrm2_2(v[k][0], v[k][1]);
        if (nr > 0.0) {
            const double sc = 1.0 / nr;
            v[k][0] *= sc;
            v[k][1] *= sc;
        }
    }
    double lam[2] = {a, d};
    int ord[2] = {0, 1};
    if (fabs(lam[1]) < fabs(lam[0])) {
        ord[0] = 1;
        ord[1] = 0;
    }
    for (int i = 0; i < 2; i++) axii[i] = 2.f * (float)sqrt(5.991 * fabs(lam[ord[i]]));
    *angle = (float)atan2(v[ord[1]][0], v[ord[1]][1]);
    return 1;
}

}  // namespace ekf
