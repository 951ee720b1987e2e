/*
 * slam_ekf.h — C-ABI of the MI355X-native EKF-SLAM update (libslam_ekf.so).
 *
 * Drop-in boundary for HuaiLeiTang/slam_ros `class Robot` (slam_ros/Robot.h:21-77). The
 * reference has no FFI: its interface is the C++ class, so every entry point below names the
 * member (file:line) it replaces. Plain pointers and sizes only; no GSL/ROS/torch types.
 *
 * One context = E independent EKF instances (an ensemble) of capacity N landmarks on one
 * HIP device, one HIP stream. State n = 3 + 2N (Robot.h:13-14 LINESIZE/SLAMSIZE, runtime here).
 * Contexts are not thread-safe (the reference is single-threaded, main.cpp:130-179).
 *
 * Errors: every call returns an int status (EKF_OK == 0). The reference's localize() returns
 * void and only prints GSL error codes (Robot.cpp:128, 909-917); per-instance numeric
 * conditions (singular S, capacity overflow, fp16 range) are reported in ekf_result.status
 * instead and the state is committed, as in the reference. One condition the reference cannot
 * have is handled differently: EKF_ST_SYNC_TIMEOUT (an instance spread over G > 1 cooperating
 * workgroups lost one of them) rolls that instance's call back instead of committing it. A
 * context whose instances fit one workgroup (N <= 192, e.g. the drop-in's N = 100) cannot time
 * out, so there every call commits.
 *
 * The library reads no environment variables: diagnostics and test hooks are per-context
 * options (ekf_set_option), all off by default.
 */
#ifndef SLAM_EKF_H
#define SLAM_EKF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: ekf_debug_scan_stamps fills 32 slots (was 16); ekf_config.arith (formerly reserved) selects
 *    the fp32 flush arithmetic and EKF_ARITH_BF16X6 is rejected (EKF_EINVAL) for configurations
 *    that can never use it; EKF_ST_SYNC_TIMEOUT rolls the call back instead of committing it.
 * 3: ekf_set_option / ekf_get_option replace the environment variables the library used to read
 *    (EKF_SPECULATE, EKF_SPIN_LOG2, EKF_TEST_DROP_WG, EKF_MFREP, EKF_SCAN_STAMPS,
 *    EKF_DD_BLOCKS_PER_CU, EKF_FLUSH_VARIANT); EKF_ARITH_F16X3; the row shard replaced by a
 *    partitioned instance (ekf_shard_create ... ekf_shard_end: tiles partitioned, O(n) state
 *    replicated). Added since, with the number unchanged (entry points only): ekf_query_joint,
 *    ekf_query_marginals, ekf_query_joint_device; ekf_gate_lines, ekf_gate_lines_device;
 *    ekf_gate_joint, ekf_gate_joint_device; ekf_resample, ekf_copy_instance;
 *    ekf_instance_image_bytes, ekf_export_instances(_device), ekf_import_instances(_device);
 *    ekf_associate_joint, ekf_associate_joint_device; ekf_gate_candidates_device,
 *    ekf_assoc_weights_device, ekf_resample_plan_device, ekf_resample_device; ekf_gate_landmarks,
 *    ekf_gate_landmarks_device. */
#define SLAM_EKF_ABI_VERSION 3
#define EKF_MAX_LINES 64 /* lines per scan per instance; main.cpp:99 reserves 20 */

/* status codes */
enum {
    EKF_OK = 0,
    EKF_EINVAL = 1,   /* bad argument */
    EKF_ENOMEM = 2,   /* device / host allocation failed */
    EKF_EDEVICE = 3,  /* HIP runtime error / no device */
    EKF_ERANGE = 4,   /* instance index / line count out of range */
};
/* ekf_result.status bits (per instance, per call) */
enum {
    EKF_ST_SINGULAR_S = 1, /* gsl_linalg_LU_invert → GSL_EDOM on some candidate (Robot.cpp:454) */
    EKF_ST_CAPACITY = 2,   /* augmentation beyond capacity (UB in the reference, Robot.cpp:802) */
    EKF_ST_NONSYM = 4,     /* EKF_R_AS_WRITTEN only: a line with index 1 or 2 matched. Its R has a
                              single off-diagonal entry (Robot.cpp:302-304), so the reference's
                              K·S·Kᵀ — and from then on its P — is not symmetric; the packed
                              symmetric storage keeps the upper triangle. */
    EKF_ST_SYNC_TIMEOUT = 8, /* the instance's cooperating workgroups did not all arrive at an
                                exchange within the spin bound: the call is rolled back (the
                                instance keeps its state from before the call, as if the scan had
                                not been received; the result record reports no matches) */
    EKF_ST_RANGE = 16,     /* EKF_PREC_F16: a landmark this call added has a variance above a
                              quarter of the fp16 range at the instance's storage exponent
                              (2^exp·P stored; values are still finite). ekf_rescale re-chooses
                              the exponent; ignoring it lets later landmarks saturate to ±inf.
                              EKF_PREC_F32: a new landmark variance above 2^120, within 2^8 of
                              fp32's range (a diverged filter: the fp64 storage holds it) */
    EKF_ST_PRECISION = 32, /* EKF_PREC_F32: the call's update shrank some landmark's variance (the
                              trace of its 2x2 block) by more than 2^4, or left it non-positive:
                              more than 4 of fp32's 24 significant bits cancel, so the stored
                              block is no longer guaranteed to resolve the fp64 reference to the
                              1e-6 bar (informational: the state commits; EKF_PREC_F64 holds any
                              filter). Every precision: a gate distance the call evaluated (up to
                              the winner) lies within the storage precision of the gate of the
                              threshold (|ΔP_ab| up to eta·sqrt(P_aa·P_bb), eta 2^-16 for F32,
                              2^-8 F16, 2^-44 F64, first order), so the reference's state may decide
                              that line differently. In SURVEY §8d's world the reference's own
                              motion model runs away and this is how a diverging
                              instance shows */
};

/* storage precision of the landmark-landmark covariance block (robot rows, mean: always fp64).
 * F16: fp16 storage, fp32 MFMA accumulation, the block rounded to fp16 after every scan
 * (BASELINE config 5); the tolerance it meets is stated in tests/test_gpu_parity.py. */
enum { EKF_PREC_F64 = 0, EKF_PREC_F32 = 1, EKF_PREC_F16 = 2 };
/* R source inside the association loop (SURVEY.md §8a parity-mode flags) */
enum { EKF_R_INTENDED = 0, EKF_R_AS_WRITTEN = 1 };
/* arithmetic of the fp32 covariance flush (ekf_config.arith).
 * EXACT: v_mfma_f32_32x32x2_f32; the flush's per-element chain is the ordered fp32 FMA chain the
 *   association kernel replays on read, so the state is bit-identical for every flush interval
 *   and schedule (default; the C++ drop-in uses it).
 * BF16X6: requires EKF_PREC_F32 or EKF_PREC_F16, EKF_R_INTENDED and max_lines <= 8; any other
 *   configuration is rejected by ekf_create with EKF_EINVAL. Every fp32 operand is split exactly
 *   into three bf16 parts (hi + mid + lo), six v_mfma_f32_32x32x16_bf16 per product (all part
 *   products down to 2^-16 relative; the dropped ones are below 2^-24), accumulated in fp32; fp16
 *   storage is scaled out of its exponent on load and rounded to fp16 once per group on store.
 *   Within fp32 rounding of EXACT (the 1e-6 bound of BASELINE holds; fp16: its re-stated 1e-3) but
 *   no longer bit-identical across flush intervals: the state depends on T at the level of fp32
 *   rounding. The association kernel applies pending steps by the same bf16 MFMAs on the planes
 *   (EKF_OPT_MFMA_REPLAY) and keeps the diagonal blocks in fp64. Groups of an even number of steps
 *   (2..16) take the split-bf16 flush, augmentation and resets included: the wave-tiles holding a
 *   landmark the group added are recomputed by the exact general loop in a second pass, and those
 *   of an instance whose map was reset in the group are stored as zero; the wave-tiles past every
 *   step's nonzero operand rows are skipped (EKF_OPT_ACTIVE_FLUSH). An odd-sized group (a partial
 *   group flushed by a drain) takes the EXACT forms (ekf_flush_kernel_name reports the form).
 * F16X3: the same requirements, schedule and fallbacks as BF16X6, with a two-part fp16 split
 *   instead: every operand row is scaled by 2^σ (σ per instance, from the largest landmark variance
 *   vmax: |2^σ·V| <= 2^12 because each step's downdate V·Vᵀ is bounded by the variances it reduces;
 *   σ is chosen at the first scan of a flush group and changes mid-group only on a reset or a new
 *   landmark 64x above the variance it was set for; an instance whose σ changes inside a group,
 *   or one with a landmark whose variance is below 2^-4·4^-σ (the planes would lose bits relative
 *   to that landmark's own scale: PLANE_SIGMA_EXACT, a filter spanning more than 2^28 in
 *   variance), runs that group's flush and on-read replay in the exact forms), split into hi + lo
 *   fp16 parts (22 significant bits), and each product runs as three v_mfma_f32_32x32x16_f16 —
 *   (lo, hi), (hi, lo), (hi, hi) — accumulated in fp32, the accumulators holding P·2^(2σ)
 *   (power-of-two scalings, exact). Half the MFMA work and two thirds of the plane bytes of BF16X6;
 *   per product within ≈2^-21 of the rows' own scale (BF16X6: 2^-23), held to the same bar per scan
 *   from identical inputs (tests/test_bench_config.py, SURVEY §8d's world included). */
enum { EKF_ARITH_EXACT = 0, EKF_ARITH_BF16X6 = 1, EKF_ARITH_F16X3 = 2 };

typedef struct ekf_config {
    int32_t capacity;      /* N = LINESIZE (Robot.h:13); landmarks per instance */
    int32_t instances;     /* E: independent EKF instances in this context */
    int32_t precision;     /* EKF_PREC_* for the landmark block of P */
    int32_t device;        /* HIP device ordinal, -1 = current */
    int32_t max_lines;     /* per-scan line capacity per instance, <= EKF_MAX_LINES */
    int32_t r_mode;        /* EKF_R_* */
    int32_t reset_margin;  /* map wiped when savedLineCount > N - margin (Robot.cpp:893: 10) */
    int32_t pipeline;      /* 1: double-buffer the landmark block so that association kernels
                              may overlap the covariance downdate of earlier scans (applying it on
                              read, bit-identically); 0: in-place, strictly sequential. Overlap
                              happens only when an instance fits one association workgroup
                              (N <= 192): otherwise its cooperating workgroups must not wait on
                              CUs a flush holds, so its association kernels are ordered after the
                              flush in flight, and the second buffer is not allocated */
    int32_t flush_interval;/* T >= 1: the landmark block is rewritten once per T scans by one
                              rank-2·Σm MFMA pass; scans in between read it with the pending
                              downdates applied on read. With EKF_ARITH_EXACT the state is
                              bit-identical for every T (the MFMA chain is an ordered FMA chain);
                              the split arithmetics are within fp32 rounding of it instead.
                              T = 1: once per scan. <= 16 (<= 24 with EKF_ARITH_F16X3) */
    int32_t arith;         /* EKF_ARITH_* (fp32 flush arithmetic); formerly reserved, 0 = EXACT */
    double mahalanobis;    /* MAHALANOBIS gate, Robot.h:15 (0.4) */
    double encoder_noise;  /* ENCODERNOISE, Robot.h:17 (0.024) */
} ekf_config;

/* One observed line: the fields of `line` (simplifyPath.h:62-79) that localize reads. */
typedef struct ekf_line {
    double alpha; /* line.alfa, robot frame */
    double r;     /* line.r */
    double R[4];  /* *line.C_AR, 2x2 row-major */
} ekf_line;

/* Per-instance outcome of one localize (what Robot exposes after the call). */
typedef struct ekf_result {
    double pose[3];            /* xPos, yPos, thetaPos (Robot.h:54-56) */
    int32_t matches;           /* matchesNum (Robot.h:36) */
    int32_t new_landmarks;     /* extraLines.size() (Robot.cpp:291) */
    int32_t saved;             /* savedLineCount after the call (Robot.h:28) */
    int32_t reset;             /* 1 if the capacity reset ran (Robot.cpp:893-904) */
    int32_t status;            /* EKF_ST_* bits */
    int32_t nlines;
    int32_t match[EKF_MAX_LINES]; /* matched saved index per line, -1 = appended as new */
} ekf_result;

typedef struct ekf_ctx ekf_ctx;

void ekf_config_init(ekf_config* cfg);
const char* ekf_strerror(int status);
int ekf_abi_version(void);

/* Robot::Robot(x, y, theta) for every instance (Robot.cpp:20-35), y/P/savedLineCount zeroed. */
int ekf_create(const ekf_config* cfg, ekf_ctx** out);
int ekf_destroy(ekf_ctx* ctx);
/* Order all work after/before the caller's stream (e.g. torch's current stream). NULL = own. */
int ekf_set_stream(ekf_ctx* ctx, void* hip_stream);
int ekf_sync(ekf_ctx* ctx);

/* Per-context options: diagnostics, alternative (result-identical or parity-equivalent) kernel
 * forms and test hooks. A new context has every option at its default; nothing is read from the
 * environment. ekf_set_option drains the context first (the option applies from the next call)
 * and returns EKF_EINVAL for an unknown option, EKF_ERANGE for a value out of range. */
enum {
    /* association path: 1 speculative (default), 0 the sequential chain on every scan (one
     * cross-workgroup exchange per line), 2 test hook: every guess wrong (the speculative path,
     * a failed verdict and the sequential restart on every scan), 3 test hook: the guesses of
     * lines L/2 .. L-1 wrong (a failed verdict keeps the lines before the first wrong one).
     * Results: bit-identical in all four modes under EKF_ARITH_EXACT and on fp64 storage, and on
     * the split arithmetics with the per-element replay (EKF_OPT_MFMA_REPLAY off: it is the
     * sequential chain). On the split arithmetics with the MFMA replay (1 or 2) the association,
     * matches, new landmarks and status of every scan are identical and the state is within the
     * arithmetic's parity bar of the fp64 reference in every mode, but not the same bits: mode 0
     * reads the pending steps by the exact per-step chain, the speculative pass by MFMA, and a
     * restart takes the guessed columns from the MFMA replay and the others from the chain. */
    EKF_OPT_SPECULATE = 1,
    /* spin bound of the association's cross-workgroup waits: 2^v polls, 8 <= v <= 24 (24) */
    EKF_OPT_SPIN_LOG2 = 2,
    /* fp32 / fp16 flush form, all bit-identical within an arithmetic: 0 automatic (default),
     * 2 the super-tile form for every group, 8 the wave form also for groups of 2 and 4 steps,
     * 24 the split-bf16 flush on 2 x 4 wave-tiles, 44 the split-fp16 flush on groups of 2 x 2
     * wave-tiles sharing their operand planes through LDS (groups of 6 or more steps) */
    EKF_OPT_FLUSH_FORM = 3,
    /* workgroups per CU of the grid-strided flush forms, 1..16 (8) */
    EKF_OPT_FLUSH_BLOCKS_PER_CU = 4,
    /* pending steps applied on read by MFMA. 1 (default): split arithmetics by their own split
     * products on the operand planes (a step whose planes cannot carry the instance's dynamic
     * range is replayed exactly, PLANE_SIGMA_EXACT), fp64 storage by the flush's own f64 MFMA
     * (bit-identical); 2: split arithmetics by fp32 MFMA on the fp32 operand rows (exact
     * products: within a flush group the association reads the block at the EXACT arithmetic's
     * precision, ≈3 µs per scan more at T = 20); 0: the per-element replay forms */
    EKF_OPT_MFMA_REPLAY = 5,
    /* 1: the association kernel's instrumented instantiation with phase timers
     * (ekf_debug_scan_stamps); 0 (default) the product kernel */
    EKF_OPT_SCAN_STAMPS = 6,
    /* test hook: e + 1 = the last association workgroup of instance e never runs (its exchanges
     * time out and the instance's calls roll back); 0 off (default) */
    EKF_OPT_TEST_DROP_WG = 7,
    /* test hook: e + 1 = on the speculative path, association workgroup 1 of instance e treats
     * its verdict poll as timed out while every other workgroup completes; 0 off (default) */
    EKF_OPT_TEST_VERDICT_TIMEOUT = 8,
    /* 1 (default): the split-arithmetic flush skips the wave-tiles whose columns lie past every
     * landmark with a nonzero operand row or new row in the group (unchanged by it: a partly
     * filled map streams only its active part); 0: every wave-tile */
    EKF_OPT_ACTIVE_FLUSH = 9,
    /* landmarks per association workgroup: 0 automatic (default: the narrowest that fits), 192,
     * or 128 / 64 (more workgroups per instance, each with fewer landmarks, on more CUs: fp32 /
     * fp16 storage with EKF_R_INTENDED and max_lines <= 8, every flush arithmetic, when an
     * instance then needs at most 64 workgroups and the instances still fit the device in one
     * launch; otherwise 192). Identical results for every value. */
    EKF_OPT_SCAN_THREADS = 10,
};
int ekf_set_option(ekf_ctx* ctx, int option, int value);
int ekf_get_option(const ekf_ctx* ctx, int option, int* value);

/* Robot::Robot(x, y, theta) on one instance (e < 0: all instances). */
int ekf_reset_instance(ekf_ctx* ctx, int e, double x, double y, double theta);

/* Robot::localize(lines, rot, encoder) (Robot.h:74, Robot.cpp:126-904) on every instance.
 * Host buffers: encoder[E*3] (realRoboPose, main.cpp:84-89), lines[E*max_lines] (instance e
 * uses lines[e*max_lines ... + nlines[e]-1]), nlines[E]. out[E] optional. Synchronous.
 * `rot` (wheel rotations) is not an input: SIMULATIONOFF == true (Robot.h:18) never uses it. */
int ekf_localize(ekf_ctx* ctx, const double* encoder, const ekf_line* lines,
                 const int32_t* nlines, ekf_result* out);
/* Same, with all three inputs already resident in device memory; asynchronous on the
 * context stream. Results stay on the device until ekf_read_results(). */
int ekf_localize_device(ekf_ctx* ctx, const double* d_encoder, const ekf_line* d_lines,
                        const int32_t* d_nlines);
/* The two halves of localize: predict = Robot.cpp:130-286 (motion model and
 * P_pre), update = Robot.cpp:288-904 (association, Kalman updates, augmentation, reset).
 * predict followed by update == localize. */
int ekf_predict(ekf_ctx* ctx, const double* encoder);
int ekf_update(ekf_ctx* ctx, const ekf_line* lines, const int32_t* nlines, ekf_result* out);
int ekf_read_results(ekf_ctx* ctx, ekf_result* out);

/* State transfer (fixtures, tests, checkpoints). P_full is the reference's dense row-major
 * n×n P_t0 (Robot.h:62) in fp64; y is Robot::y (Robot.h:26); pose = xPos/yPos/thetaPos. */
int ekf_upload_state(ekf_ctx* ctx, int e, const double* P_full, const double* y, int saved,
                     const double pose[3]);
/* Any pointer may be NULL. With P_full the call drains first (the pending downdates are flushed);
 * without it, it only waits for the context's stream: the mean, pose and savedLineCount are
 * committed by every scan, and the flush schedule is left as it is. */
int ekf_download_state(ekf_ctx* ctx, int e, double* P_full, double* y, int* saved,
                       double pose[3]);
/* Device-side initialisation P = diag(d) + U·Uᵀ (U: n×rank row-major, host pointers). */
int ekf_init_lowrank(ekf_ctx* ctx, int e, const double* diag, const double* U, int rank,
                     const double* y, int saved, const double pose[3]);
/* EKF_PREC_F16 storage exponent: the landmark block is stored as fp16(2^exp·P). Upload and
 * init_lowrank choose it from the largest landmark variance v (exp = min(10, ⌊log2(4096/v)⌋),
 * at least -24; 10 for an empty map); ekf_rescale(ctx, e, EKF_EXP_AUTO) re-chooses it from the
 * current P (EKF_ST_RANGE), or sets the given exponent. Power-of-two rescaling is exact except
 * for values that leave fp16's normal range. For f32 / f64 storage the exponent is 0 and
 * rescale is a no-op. */
#define EKF_EXP_AUTO (-1000)
int ekf_storage_exponent(const ekf_ctx* ctx, int e);
int ekf_rescale(ekf_ctx* ctx, int e, int exp);
/* P_t0[0:3,0:3] of instance e (what getEllipse reads, Robot.cpp:75-77). */
int ekf_get_pose_cov(ekf_ctx* ctx, int e, double P33[9]);
/* Robot::getEllipse(axii, angle) (Robot.h:73, Robot.cpp:73-124): axii sorted by |eigenvalue|,
 * angle = atan2 of the larger eigenvalue's unit eigenvector in GSL's sign convention. Returns 1
 * on success, 0 if the 2x2 eigenproblem failed (as the reference's bool), negative on API error. */
int ekf_get_ellipse(ekf_ctx* ctx, int e, float axii[2], float* angle);
/* The same computation on a given 2x2 block P22 = {P00, P01, P10, P11} (host only, no device):
 * gsl_eigen_nonsymmv + GSL_EIGEN_SORT_ABS_ASC restated (sign convention included). Returns 1,
 * 0 for a non-finite block or a complex eigenvalue pair, negative on API error. Divergence: for a
 * complex pair (only a non-symmetric block has one; P's pose block is symmetric) the reference's
 * nonsymmv succeeds and it publishes |Re λ| and an angle from the real parts of the complex
 * eigenvector; that branch of GSL is not restated here, axii and angle are left untouched. */
int ekf_ellipse_of_block(const double P22[4], float axii[2], float* angle);

/* Covariance blocks of chosen landmarks, read without draining. The reference has no such member (its
 * P_t0 is a host array, Robot.h:62); these replace reading entries of it.
 * Values: cov equals P_full[rows][:, rows] of the matrix ekf_download_state would return at that
 *   point, mean the same entries of y, blocks and cross the corresponding entries of that matrix. The
 *   pending steps of the flush group are applied on read. With EKF_ARITH_EXACT (every storage
 *   precision) and on fp64 storage this holds bit for bit. On the split arithmetics the pending steps
 *   are read by the exact per-element chain, as EKF_OPT_MFMA_REPLAY = 0 does, so the values agree with
 *   the later flush only to the arithmetic's parity bar; with fp16 storage the one to-storage rounding
 *   the group's flush applies is applied, so every returned value is a representable stored value.
 * No drain, no state change: the call writes nothing of the instance's state and enqueues no flush;
 *   the flush schedule, the step count and the result mirror are untouched. The host forms are
 *   synchronous: one kernel, one copy, one wait on the context stream. The device form only enqueues.
 * Indices: duplicates and any order are allowed; a landmark at or past savedLineCount reads as the
 *   zero rows the state holds.
 * Errors: the host forms return EKF_ERANGE for e out of range, K < 0, K > N or an index outside
 *   [0, N), EKF_EINVAL for a NULL context (or a NULL list with K > 0 where one is required); a
 *   partitioned context (ekf_shard_create) returns EKF_EINVAL, as for ekf_localize. In the device form
 *   an index outside [0, N) gives NaN in that landmark's rows and columns of cov and its entries of
 *   mean, and is never dereferenced. K == 0 is valid: the pose block and the pose mean. */
/* Joint marginal of the pose and K landmarks of instance e, of the committed state (every scan
 * enqueued so far): rows/columns {0,1,2, 3+2j, 4+2j : j in landmarks}. */
int ekf_query_joint(ekf_ctx* ctx, int e, const int32_t* landmarks, int K,
                    double* cov /* (3+2K)^2 row-major, may be NULL */,
                    double* mean /* 3+2K, may be NULL */);
/* Per-landmark marginals: blocks[k] = the 2x2 block of landmark k (row-major), cross[k] = the 3x2
 * robot-landmark block P[0:3, 3+2j:5+2j] (row-major), mean[k] = y[3+2j], y[4+2j]. landmarks NULL =
 * 0..K-1; any output may be NULL. */
int ekf_query_marginals(ekf_ctx* ctx, int e, const int32_t* landmarks, int K,
                        double* blocks /* [K][4] */, double* cross /* [K][6] */, double* mean /* [K][2] */);
/* The joint query for every instance at once, all buffers in device memory, asynchronous on the
 * context stream: d_landmarks [E][K], d_cov [E][(3+2K)^2], d_mean [E][3+2K] (either may be NULL). */
int ekf_query_joint_device(ekf_ctx* ctx, const int32_t* d_landmarks, int K, double* d_cov, double* d_mean);

/* Trial lines scored against the map, state untouched: which landmark the association would pick for
 * a line, how far away it is, and whether there was a second candidate. The reference has no such
 * member: its association (Robot.cpp:313-498) is first-fit inside localize, which commits the scan.
 * Independent lines: each line is evaluated on its own against every saved landmark j <
 *   savedLineCount, as the first line of a scan: no sequential update between the lines and no
 *   "already matched" skip. R is what the association builds for index i in the list under the
 *   context's r_mode (EKF_R_AS_WRITTEN: it follows the line's index). d2[i][j] is +inf for
 *   j >= savedLineCount. The gate is the association's own expression, so a NaN distance passes.
 * Pose and P, enc given: the call predicts on read. x_pre, the motion Jacobian and the predicted
 *   3x3 block come from the committed pose exactly as ekf_predict computes them (Robot.cpp:130-286),
 *   and each candidate's robot-landmark columns are predicted likewise; nothing is written.
 *   hits[0].first is therefore the match ekf_localize(enc, lines) would report for line 0.
 * Pose and P, enc == NULL: between ekf_predict and ekf_update the call uses the inputs ekf_update
 *   would use now (the committed, predicted strip and x_pre); otherwise the committed pose and strip
 *   with no motion. Between ekf_predict and ekf_update a call with enc != NULL returns EKF_EINVAL
 *   (the strip is already predicted); the state is "predicted" from ekf_predict until the next
 *   update, localize or state write (reset, upload, ekf_init_lowrank, ekf_rescale).
 * Landmark blocks: read as the covariance queries read them, the pending steps of the flush group
 *   applied on read and, with fp16 storage on the split arithmetics, the group's one to-storage
 *   rounding. With EKF_ARITH_EXACT (every storage precision) and on fp64 storage this is the
 *   association's own view, bit for bit. On the split arithmetics the pending steps are read by the
 *   exact per-element chain, as for the queries, so the distances agree with the association's to the
 *   arithmetic's parity bar.
 * No drain, no state change: the call writes nothing of the instance's state and enqueues no flush;
 *   the flush schedule, the step count and the result mirror are untouched. The host form is
 *   synchronous: two kernels, one copy, one wait on the context stream. The device form only
 *   enqueues; it writes the entries i >= nlines[e] of d_hits as first = nearest = -1, npass = 0.
 * Errors: EKF_ERANGE for e out of range or L outside [0, max_lines]; EKF_EINVAL for a NULL context,
 *   NULL lines with L > 0, NULL hits, or a partitioned context (ekf_shard_create). L == 0 is valid. */
typedef struct ekf_gate_hit {
    int32_t first;     /* lowest landmark index whose distance passes the gate (what Robot.cpp:313-498
                          picks for this line when no earlier line of the scan matched); -1: none */
    int32_t nearest;   /* argmin |d2| over the candidates (lowest index on ties, NaN ignored); -1: none */
    int32_t npass;     /* candidates that pass the gate */
    int32_t status;    /* EKF_ST_SINGULAR_S / EKF_ST_PRECISION (its gate half, at the storage precision
                          of the gate) over the candidates the reference would evaluate: 0..first, or
                          all when first == -1 */
    double d2_first, d2_nearest;   /* vT S^-1 v as the reference computes it (Robot.cpp:479-486); NaN if none */
    double S[4], v[2];             /* innovation covariance and innovation of `first`, or of `nearest`
                                      when nothing passes; zeros when there is no candidate */
} ekf_gate_hit;
int ekf_gate_lines(ekf_ctx* ctx, int e, const double enc[3] /* may be NULL */, const ekf_line* lines, int L,
                   ekf_gate_hit* hits /* [L] */, double* d2 /* [L][N], may be NULL */);
/* Every instance at once, all buffers in device memory, asynchronous on the context stream. */
int ekf_gate_lines_device(ekf_ctx* ctx, const double* d_enc /* [E][3] or NULL */,
                          const ekf_line* d_lines /* [E][max_lines] */, const int32_t* d_nlines /* [E] */,
                          ekf_gate_hit* d_hits /* [E][max_lines] */, double* d_d2 /* [E][max_lines][N] or NULL */);

/* Landmark pairs that are one line, state untouched: every saved landmark scored against every other.
 * The reference's association is first-fit (Robot.cpp:313-498) and appends a line that misses its gate
 * as a new landmark (Robot.cpp:776-866), so a map collects landmarks that are one physical line; a wall
 * seen from both sides is stored twice by construction, as (alpha, r) and (alpha + pi, -r). Its only
 * remedy is to wipe the map (Robot.cpp:893-904). This call finds the pairs; it does not act on them.
 * The pair (lo, hi): lo = min(a, b), hi = max(a, b), whichever side asks, both below savedLineCount, so
 *   d2[a][b] == d2[b][a] bit for bit.
 * Blocks: Dlo, Dhi the two diagonal 2x2 blocks, X = P[lo, hi], each read as the covariance queries read
 *   it: the pending steps of the flush group applied on read and, with fp16 storage on the split
 *   arithmetics, the group's one to-storage rounding. With EKF_ARITH_EXACT and on fp64 storage these are
 *   the bits ekf_download_state would show; on the split arithmetics the exact per-element chain, as for
 *   the queries. The mean is the committed copy of y.
 * Same-direction form, additions only, in this order:
 *   c00 = (Dlo00 + Dhi00) - (X00 + X00), c01 = (Dlo01 + Dhi01) - (X01 + X10),
 *   c11 = (Dlo11 + Dhi11) - (X11 + X11), d0 = remainder(alpha_lo - alpha_hi, 2 pi) (the IEEE
 *   remainder, 2 pi the fp64 constant), d1 = r_lo - r_hi.
 * Flipped form (hi taken as (alpha_hi + pi, -r_hi), F = diag(1, -1)): c00 as above,
 *   c01 = (Dlo01 - Dhi01) + (X01 - X10), c11 = (Dlo11 + Dhi11) + (X11 + X11),
 *   d0 = remainder((alpha_lo - alpha_hi) - pi, 2 pi), d1 = r_lo + r_hi.
 * Distance of one form: Cholesky in fp64 in a fixed order, a*b + c contracted within one expression:
 *   l00 = sqrt(c00), l10 = c01 / l00, t = c11 - l10 l10, l11 = sqrt(t), z0 = d0 / l00,
 *   z1 = (d1 - l10 z0) / l11, d2 = z0 z0 + z1 z1. A form whose c00 or t is <= 0 or not finite is NaN.
 * Distance of the pair: the same-direction value when the flipped one is NaN or the same-direction one
 *   is <= it, else the flipped value. Both NaN: the pair is NaN and EKF_PH_SINGULAR is set in the
 *   records of both lo and hi.
 * Pass: d2 <= gate * gate; a NaN fails, as in ekf_associate_joint.
 * The matrix d2 [N][N]: the pair's value for two different saved landmarks; +inf on the diagonal and
 *   where either index is at or past savedLineCount.
 * The records: hits[a] is a pure function of row a of that matrix, whether or not the matrix is
 *   requested: first the lowest passing index, npass the count of passing entries, nearest the argmin
 *   over the finite entries (lowest index on ties). EKF_PH_FLIP_* says that the reported pair's value is
 *   the flipped form's. A landmark at or past savedLineCount, or a map with fewer than two landmarks,
 *   gets the empty record: -1, -1, 0, 0, NaN, NaN, zeros.
 * No drain, no state change, as ekf_gate_lines: nothing of the state, the schedule, the step count or
 *   the result mirror is written. Valid at any point, also between ekf_predict and ekf_update: the
 *   predict moves neither the landmark block nor the landmark means. The host form is synchronous (two
 *   kernels, one copy, one wait on the context stream) and gives the same bits as the device form,
 *   which only enqueues. The result does not depend on how the device schedules the work: every
 *   reduction is over a total order (min index, integer sum, min of (d2, index)).
 * Errors: EKF_EINVAL for a NULL context, NULL hits, a gate that is not a finite number >= 0, or a
 *   partitioned context (ekf_shard_create); EKF_ERANGE for e out of range. */
enum { EKF_PH_FLIP_NEAREST = 1, EKF_PH_FLIP_FIRST = 2, EKF_PH_SINGULAR = 4 };   /* ekf_pair_hit.status */
typedef struct ekf_pair_hit {      /* landmark a against every other saved landmark; 72 bytes */
    int32_t nearest;   /* partner with the smallest d2 (lowest index on ties, NaN ignored); -1: none */
    int32_t first;     /* lowest partner index whose d2 passes; -1: none */
    int32_t npass;     /* partners that pass */
    int32_t status;    /* EKF_PH_* */
    double d2_nearest, d2_first;   /* NaN if none */
    double C[3], delta[2];         /* c00, c01, c11 and delta of `nearest`, in the form that won; zeros if none */
} ekf_pair_hit;
int ekf_gate_landmarks(ekf_ctx* ctx, int e, double gate, ekf_pair_hit* hits /* [N] */, double* d2 /* [N][N], may be NULL */);
/* Every instance at once, both buffers in device memory, asynchronous on the context stream. */
int ekf_gate_landmarks_device(ekf_ctx* ctx, double gate, ekf_pair_hit* d_hits /* [E][N] */,
                              double* d_d2 /* [E][N][N] or NULL */);

/* Joint compatibility of line-landmark hypotheses, state untouched: the squared Mahalanobis distance
 * and the log determinant of the stacked innovation of a whole assignment. ekf_gate_lines scores each
 * line alone; two pairings that pass alone can be jointly impossible, because their innovations are
 * correlated through the pose and the landmark-landmark blocks of P. The reference has no such
 * member (its association, Robot.cpp:313-498, is first-fit).
 * Hypothesis: assign[h][i] is the landmark of line i, or -1 for "unassigned" (the line is left out).
 *   The m assigned lines enter v (2m long) in list order. The same landmark on two lines is allowed
 *   (R keeps S definite). A landmark in [savedLineCount, N) reads as the zero rows the state holds,
 *   as for the covariance queries.
 * v, H, R per line: exactly what the association and ekf_gate_lines use for (line i, landmark j): the
 *   wrapped angle innovation, H, and R of index i under the context's r_mode. d2_each[h][i] is that
 *   pair's own distance, bit for bit ekf_gate_lines' d2[i][assign[h][i]] for a saved landmark, NaN
 *   where the line is unassigned.
 * S: the 2x2 block (a, b) is H_a P[{0,1,2,l_a},{0,1,2,l_b}] H_b^T, plus R_a when a == b, from the 3x3
 *   robot block, the two landmarks' strip columns and the block P[l_a, l_b], the last read as the
 *   covariance queries read it (pending steps applied on read). The lower triangle is computed and
 *   factored by Cholesky in fp64, in a fixed order: a hit depends only on its own hypothesis and the
 *   state, not on H, its place in the list, or the host / device form.
 * Result: d2 = v^T S^-1 v and logdet = log det S. The log-likelihood of the scan under the
 *   hypothesis is the caller's to form: -(d2 + logdet) / 2 - m log(2 pi).
 * Pose and P: the three cases of ekf_gate_lines (enc given: predict on read; NULL between ekf_predict
 *   and ekf_update: the predicted strip and x_pre; NULL otherwise: the committed pose), and its
 *   EKF_EINVAL for enc != NULL between ekf_predict and ekf_update.
 * No drain, no state change, as ekf_gate_lines. The host form is synchronous: one kernel, one copy,
 *   one wait on the context stream. The device form only enqueues.
 * Errors: as ekf_gate_lines, plus EKF_ERANGE for H < 0 or an assign entry outside [-1, N). In the
 *   device form such an entry is never dereferenced: that hypothesis gets d2 = logdet = NaN and
 *   EKF_ST_SINGULAR_S (d2_each NaN), the others are unaffected; entries i >= nlines[e] are ignored.
 *   H == 0 and L == 0 are valid. EKF_EINVAL for a partitioned context. */
typedef struct ekf_joint_hit {
    int32_t m;        /* lines of the hypothesis that carry a landmark */
    int32_t status;   /* EKF_ST_SINGULAR_S: a pivot of the factorisation of S was <= 0 or not finite (d2, logdet NaN) */
    double d2;        /* v^T S^-1 v of the stacked innovation, 2m long; 0 for m == 0 */
    double logdet;    /* log det S; 0 for m == 0 */
} ekf_joint_hit;
int ekf_gate_joint(ekf_ctx* ctx, int e, const double enc[3] /* may be NULL */, const ekf_line* lines, int L,
                   const int32_t* assign /* [H][L] */, int H, ekf_joint_hit* hits /* [H] */,
                   double* d2_each /* [H][L], may be NULL */);
/* Every instance at once, all buffers in device memory, asynchronous on the context stream. */
int ekf_gate_joint_device(ekf_ctx* ctx, const double* d_enc /* [E][3] or NULL */, const ekf_line* d_lines /* [E][max_lines] */,
                          const int32_t* d_nlines /* [E] */, const int32_t* d_assign /* [E][H][max_lines] */, int H,
                          ekf_joint_hit* d_hits /* [E][H] */, double* d_d2_each /* [E][H][max_lines] or NULL */);

/* The joint-compatibility search on the device, state untouched: given trial lines and each line's
 * candidate landmarks, the jointly compatible assignment with the most pairings and, among those, the
 * smallest joint distance (joint compatibility branch and bound). ekf_gate_joint scores hypotheses the
 * caller forms; this call forms them itself, over a factor of S that grows two rows per pairing, so a
 * scan costs one call instead of one ekf_gate_joint round trip per line. The reference has no such
 * member (its association, Robot.cpp:313-498, is first-fit).
 * Candidates: cand[i][c] is a landmark offered to line i, or -1. An entry is usable when it lies in
 *   [0, savedLineCount); one at or past savedLineCount is skipped silently. An entry outside [-1, N)
 *   is EKF_ERANGE in the host form; in the device form it is never used as an index, it is treated as
 *   -1 and EKF_AS_INVALID is set. At most EKF_ASSOC_MAX_LINES lines may carry a usable candidate and at
 *   most EKF_ASSOC_MAX_TOTAL candidates may be usable over all lines (the search's tables live in LDS:
 *   64 candidates give 2016 pairs of one 2x2 block each, 16 pairings a packed factor of 33 rows): more
 *   is EKF_ERANGE in the host form; in the device form that instance alone gets EKF_AS_INVALID and the
 *   empty hypothesis.
 * Duplicates: a landmark explains at most one line of a hypothesis (ekf_gate_joint allows a duplicate;
 *   the search does not).
 * Tree: the lines are taken in list order. At line i the children are its usable candidates in list
 *   order (those not already taken on the path), then "unassigned" last. A child that assigns a pair is
 *   kept only if its own joint distance satisfies d2 <= bound[m], m the pairings including the new one
 *   (written so that NaN fails). A failed pivot of the factor prunes the child and sets
 *   EKF_AS_SINGULAR. The empty hypothesis is always feasible.
 * Result: among the leaves that are feasible at every assigning step, the largest m, then the smallest
 *   d2 (fp64 compare), then the earliest in that depth-first order: a total order, so the answer does
 *   not depend on how the device explores the tree. A subtree is cut only when it cannot beat the
 *   incumbent strictly in (m, d2); d2 never decreases along a path (an fma sum of squares in ascending
 *   k).
 * Bits: d2 and logdet of the result are bit for bit what ekf_gate_joint returns for hit.assign at the
 *   same point, in the host form and in the device form: v, H, R, the diagonal blocks and the pair
 *   blocks S_ab are ekf_gate_joint's expressions (one copy); the factor row (r, .) is S_rc with its
 *   updates fma(-L_rk, L_ck, .) in ascending k, then a division by L_cc, z carried as the extra row;
 *   d2 = sum z_k^2 as an ascending fma chain and logdet = 2 sum log L_kk, the sum ascending.
 * Budget: max_nodes in [1, EKF_ASSOC_MAX_NODES] (else EKF_ERANGE) bounds the children scored per
 *   instance. When it runs out EKF_AS_TRUNCATED is set and the result is the best feasible hypothesis
 *   found: still feasible, still with the bits above, but neither guaranteed optimal nor reproducible.
 *   Without the flag the result is the unique optimum. The budget is dealt evenly to the search's
 *   workgroups (8), and the first two levels of the tree are scored by each of them and count each
 *   time, so a budget below a few hundred may end before the first leaf: the result is then the empty
 *   hypothesis. Every loop of the kernels is bounded by the budget or by the caps; no kernel waits on
 *   another workgroup.
 * Pose and P: the three cases of ekf_gate_lines (enc given: predict on read; NULL between ekf_predict
 *   and ekf_update: the predicted strip and x_pre; NULL otherwise: the committed pose), and its
 *   EKF_EINVAL for enc != NULL between ekf_predict and ekf_update.
 * No drain, no state change, as ekf_gate_lines. The host form is synchronous: one copy, one wait on
 *   the context stream. The device form only enqueues; bound is shared by all instances.
 * Errors: EKF_EINVAL for a NULL context, bound or hit, NULL lines or cand (the host form: with L > 0),
 *   or a partitioned context;
 *   EKF_ERANGE for e out of range, L outside [0, max_lines], C outside [1, EKF_ASSOC_MAX_CAND] or
 *   max_nodes out of range. L == 0 is valid: the empty hypothesis, no launch. */
#define EKF_ASSOC_MAX_CAND   8    /* C: candidates per line */
#define EKF_ASSOC_MAX_LINES 16    /* lines that carry at least one usable candidate */
#define EKF_ASSOC_MAX_TOTAL 64    /* usable candidates over all lines */
#define EKF_ASSOC_MAX_NODES (1 << 22)
enum { EKF_AS_TRUNCATED = 1, EKF_AS_SINGULAR = 2, EKF_AS_INVALID = 4 };   /* ekf_assoc_hit.status */
typedef struct ekf_assoc_hit {
    int32_t m;        /* pairings of the best hypothesis */
    int32_t status;   /* EKF_AS_* */
    int32_t nodes;    /* children scored; informational, not reproducible between runs */
    int32_t reserved;
    double d2, logdet;               /* of the best hypothesis; 0, 0 for m == 0 */
    int32_t assign[EKF_MAX_LINES];   /* landmark per line or -1; entries >= L are -1 */
} ekf_assoc_hit;
int ekf_associate_joint(ekf_ctx* ctx, int e, const double enc[3] /* may be NULL */, const ekf_line* lines, int L,
                        const int32_t* cand /* [L][C] */, int C, const double* bound /* [L+1] */,
                        int max_nodes, ekf_assoc_hit* hit);
int ekf_associate_joint_device(ekf_ctx* ctx, const double* d_enc /* [E][3] or NULL */, const ekf_line* d_lines /* [E][max_lines] */,
                               const int32_t* d_nlines /* [E] */, const int32_t* d_cand /* [E][max_lines][C] */, int C,
                               const double* d_bound /* [max_lines+1], shared by all instances */,
                               int max_nodes, ekf_assoc_hit* d_hits /* [E] */);

/* Instances copied onto others on the device: what acts on the weights the queries and gates give
 * (fork a hypothesis; drop the unlikely instances of an ensemble and duplicate the likely ones). The
 * reference has one filter and no such member.
 * Instance e takes the whole state of instance src[e]; src[e] == e keeps it. Afterwards every read
 *   entry point (ekf_download_state, ekf_get_pose_cov, ekf_get_ellipse, ekf_query_*, ekf_gate_lines,
 *   ekf_gate_joint, ekf_storage_exponent, ekf_read_results: the source's last result record) returns
 *   for e what it returns for src[e], bit for bit, and fed the same scans e produces the same bits as
 *   src[e] from then on, under every precision, arithmetic, schedule and option.
 * Sources are fixed points: src[src[e]] == src[e] for every e (survivors stay where they are, dead
 *   slots are overwritten: what a resampler produces), else EKF_EINVAL. No slice of the state is then
 *   both read and written, so the copy is one launch with no ordering and no staging.
 * No drain, no flush, no step: the steps pending in the flush group travel with the instance (their
 *   ring slots are copied), the schedule is untouched, and an instance with src[e] == e is afterwards
 *   bit-identical to the same instance of a context that never made the call, also on the split
 *   arithmetics (where a drain would change every instance's bits). ekf_download_state /
 *   ekf_upload_state do the same through the dense n x n matrix on the host, with two drains and a
 *   re-rounding of the block.
 * Asynchronous on the context stream, behind every scan enqueued so far; src is a host list, read
 *   before the call returns.
 * Errors: EKF_EINVAL for a NULL context or list, a source that is not a fixed point, a partitioned
 *   context, or a call between ekf_predict and ekf_update; EKF_ERANGE for an entry outside [0, E).
 *   The identity list is valid and launches nothing. */
int ekf_resample(ekf_ctx* ctx, const int32_t* src /* [E], host */);
/* ekf_resample with src = identity except src[dst] = from (from must keep its state: always true
 * here). EKF_ERANGE for dst or from outside [0, E); dst == from is valid and launches nothing. */
int ekf_copy_instance(ekf_ctx* ctx, int dst, int from);

/* The ensemble's hypothesis loop without a host stop: the four stages between and behind
 * ekf_gate_lines_device and ekf_associate_joint_device, so that a scan's gate -> candidates -> joint search
 * -> weights -> resampling plan -> copy is a sequence of enqueues on the context stream. Device forms only
 * (the host forms are ekf.gate_candidates, ekf.resample_plan and ekf_resample); every buffer is device
 * memory, every call asynchronous on the context stream behind the work enqueued so far. None drains,
 * flushes, adds a step or moves the schedule. The reference has one filter and no such members.
 * EKF_EINVAL for a partitioned context, as their neighbours.
 *
 * ekf_gate_candidates_device: the candidate lists ekf_associate_joint_device takes, from the matrix
 *   ekf_gate_lines_device wrote. A pure function of that matrix: it reads no filter state.
 *   Landmark j is a member of line i's list when sqrt(fabs(d2[e][i][j])) <= gate (NaN and +inf fail). The
 *   list is ordered by that square root, ascending, the lower landmark first on ties; it keeps the first C
 *   members and is padded with -1. count[e][i], if given, is the number of members before the cut. Rows
 *   i >= nlines[e] get -1 / 0. The fp64 square root is correctly rounded, so the lists are bit for bit
 *   those of ekf.gate_candidates on the same matrix. No cap on the members inside the gate, and no
 *   dependence on scheduling: one workgroup per (line, instance) finds, C times, the smallest (key, j)
 *   strictly above the previous one.
 *   Errors: EKF_ERANGE for C outside [1, EKF_ASSOC_MAX_CAND]; EKF_EINVAL for a NULL context, d2, nlines or
 *   cand, or a gate that is not a finite number >= 0. */
int ekf_gate_candidates_device(ekf_ctx* ctx, const double* d_d2 /* [E][max_lines][N] */, const int32_t* d_nlines /* [E] */,
                               int C, double gate, int32_t* d_cand /* [E][max_lines][C] */,
                               int32_t* d_count /* [E][max_lines] or NULL */);
/* ekf_assoc_weights_device: the instances' weights from the search's hits. With m, d2, logdet of hits[e],
 *   lw_e = -(d2 + logdet) / 2 - m log(2 pi) + (nlines[e] - m) log_unassigned + logprior[e]
 *   (log_unassigned: the caller's term per line left out, 0 for the documented likelihood, not applied
 *   when no line is left out; logprior NULL: 0) and weights[e] = exp(lw_e - max lw): the best instance has
 *   weight exactly 1. An instance whose hit carries EKF_AS_INVALID, or whose lw is not finite, is out:
 *   weight 0, and it does not enter the maximum. EKF_AS_TRUNCATED hits are used as they are (still
 *   feasible). Every instance out: all weights 0, which ekf_resample_plan_device reports. One launch.
 *   Errors: EKF_EINVAL for a NULL context, hits, nlines or weights. */
int ekf_assoc_weights_device(ekf_ctx* ctx, const ekf_assoc_hit* d_hits /* [E] */, const int32_t* d_nlines /* [E] */,
                             double log_unassigned, const double* d_logprior /* [E] or NULL */,
                             double* d_weights /* [E] */);
/* ekf_resample_plan_device: systematic resampling (ekf.resample_plan) as a list ekf_resample_device takes.
 *   total = sum of the weights and edges = running sum of q_e = w_e / total, both accumulated in ascending
 *   index order; point k = (u + k) / E goes to min(upper_bound(edges, point), last index with w > 0).
 *   Every instance with a point keeps its state (src[e] = e); the slots without one, ascending, take the
 *   surplus copies of the survivors in ascending survivor order: src[src[e]] == src[e] always.
 *   info (if given): ess = 1 / sum q^2, total, copies = the number of e with src[e] != e, and status:
 *   EKF_RP_KEPT when !(ess < ess_below) (pass +inf for "always resample"): the identity list;
 *   EKF_RP_INVALID when a weight is negative or not finite or the total is not a finite positive number:
 *   the identity list, ess 0.
 *   Errors: EKF_ERANGE for u outside [0, 1); EKF_EINVAL for a NULL context, weights or src, or a NaN
 *   ess_below. */
enum { EKF_RP_INVALID = 1, EKF_RP_KEPT = 2 };   /* ekf_plan_info.status */
typedef struct ekf_plan_info {
    int32_t status;   /* EKF_RP_* */
    int32_t copies;   /* instances the plan overwrites */
    double ess;       /* effective sample size of the weights */
    double total;     /* their sum */
} ekf_plan_info;
int ekf_resample_plan_device(ekf_ctx* ctx, const double* d_weights /* [E] */, double u, double ess_below,
                             int32_t* d_src /* [E] */, ekf_plan_info* d_info /* may be NULL */);
/* ekf_resample_device: ekf_resample with the list in device memory, written by earlier work on the
 *   stream. The contract is ekf_resample's: everything an instance owns travels, the pending ring slots
 *   included, nothing drains, and an instance with src[e] == e is bit-identical to the same instance of a
 *   context that never made the call.
 *   The list is checked on the device, all or nothing: an entry outside [0, E) (never used as an index) or
 *   a source that is not a fixed point copies nothing, leaves every byte as it was, and d_status (if
 *   given) receives EKF_ERANGE or EKF_EINVAL as ekf_resample would return; an accepted list gives EKF_OK.
 *   The return value covers only what the host can see. The copy is dealt over the overwritten instances
 *   found on the device; the identity list moves no byte.
 *   The host's mirror of the storage exponents becomes stale: the next ekf_storage_exponent, state
 *   transfer or image export re-reads it from the device (one small synchronous copy there, none on the
 *   per-scan path).
 *   Errors: EKF_EINVAL for a NULL context or list, a partitioned context, or a call between ekf_predict
 *   and ekf_update. */
int ekf_resample_device(ekf_ctx* ctx, const int32_t* d_src /* [E], device */, int32_t* d_status /* device, may be NULL */);

/* Instance images: instances moved between contexts (the ranks of an ensemble sharded over GPUs, a
 * file), where ekf_resample moves them inside one. The reference has one filter and no such member.
 * An image is everything an instance owns (what ekf_resample copies) in a position-independent form:
 *   one 16-byte padded section per item, no addresses and no ring positions inside. The landmark
 *   buffers come in logical order (the one the scans read, then on the pipelined schedule the newest
 *   flush's output), the pending steps' ring slots oldest first, the newest result record when nothing
 *   is pending. Its size depends on the configuration and on the steps pending now, not on E.
 * Export is a raw copy into images + k * bytes for instance inst[k] and fills desc[k], the image's
 *   host-side label, which travels with it. It changes nothing in the context; the host form and the
 *   device form give the same bytes (padding zero), and so do two exports with nothing in between.
 * Import reads image k into slot inst[k] of a context that is congruent with the image: equal key
 *   (the layout and every ekf_config field but device and instances), equal pending, has_step and
 *   groups. Ranks fed in lockstep from one broadcast scan stream are congruent by construction; the
 *   number of steps so far, the ring position, the buffer parity and the launch epoch may differ (the
 *   import maps the sections onto the destination's own ring slots and buffers, and gives the
 *   completion words of the source's last launch the destination's epoch). Afterwards every read entry
 *   point returns for the slot what it returned for the exported instance at the export, bit for bit
 *   (ekf_read_results: the source's record and status bits), and fed the same scans the slot produces
 *   the source's bits from then on, under every precision, arithmetic, schedule and option: the
 *   contract of ekf_resample across contexts. No other instance receives a byte.
 * Neither call drains, flushes, adds a step or moves the schedule; an instance never imported over is
 *   bit-identical to the same instance of a context that never made a call, also on the split
 *   arithmetics.
 * Host forms: images and desc in host memory; synchronous (one copy per section, one wait, no kernel).
 * Device forms: d_images in device memory, 4-byte aligned (16 for full speed); one launch,
 *   asynchronous on the context stream, behind every scan enqueued so far; inst and desc are host
 *   arrays, read or written before the call returns. The device forms order nothing between two
 *   contexts: the caller orders the import after the export, with one stream shared through
 *   ekf_set_stream (set before the first step: it drains) or with ekf_sync on the exporting context
 *   (which drains it: on the split arithmetics that changes its instances' bits).
 * Errors: EKF_EINVAL for a NULL context, list, buffer or descriptor, a partitioned context, a call
 *   between ekf_predict and ekf_update, an import list with a duplicate slot, and an import of a
 *   descriptor that is not congruent or whose magic, version or bytes are wrong; EKF_ERANGE for K < 0,
 *   K > E or an entry outside [0, E). K == 0 is valid and launches nothing; an export list may repeat
 *   an instance. A refused call leaves every byte as it was. */
typedef struct ekf_image_desc {
    uint32_t magic, version; /* layout version of the image */
    uint64_t key;            /* what two contexts must share */
    uint64_t bytes;          /* bytes of the image (a multiple of 16) */
    int32_t pending;         /* steps of the open flush group inside */
    int32_t has_step;        /* the source had run at least one step (a result record is inside) */
    uint32_t epoch;          /* the source's launch epoch, for its completion words */
    int32_t groups;          /* association workgroups of the source's last launch */
    int32_t storage_exp;     /* the source's host-mirrored storage exponent */
    int32_t reserved[5];
} ekf_image_desc;
/* bytes of one instance's image as the context stands now (0 for NULL or a partitioned context) */
size_t ekf_instance_image_bytes(const ekf_ctx* ctx);
int ekf_export_instances(ekf_ctx* ctx, const int32_t* inst /* [K], host */, int K, void* images /* K * bytes, host */,
                         ekf_image_desc* desc /* [K], host */);
int ekf_import_instances(ekf_ctx* ctx, const int32_t* inst /* [K], host */, int K, const void* images /* host */,
                         const ekf_image_desc* desc /* [K], host */);
int ekf_export_instances_device(ekf_ctx* ctx, const int32_t* inst /* [K], host */, int K, void* d_images /* device */,
                                ekf_image_desc* desc /* [K], host */);
int ekf_import_instances_device(ekf_ctx* ctx, const int32_t* inst /* [K], host */, int K, const void* d_images /* device */,
                                const ekf_image_desc* desc /* [K], host */);

/* One instance with its landmark block partitioned over ranks, for maps
 * whose packed P should not (or cannot) live on one GPU. No reference member maps to these: they
 * replace the single call Robot::localize (Robot.h:34, Robot.cpp:126-904) for an instance spread over
 * processes. ekf_shard_create makes rank `rank` of `world` a context of one instance (instances =
 * 1, EKF_ARITH_EXACT, fp32 or fp64 with flush_interval <= 8, no pipeline, max_lines <= 8)
 * that stores only its share of the packed landmark block: the tiles of tile rows [row_begin,
 * row_end) (ekf_shard_tiles), a contiguous slice balanced by tile count, about 1/world of it
 * (ekf_landmark_block_bytes). Everything of size O(n) (robot strip, mean, the landmarks' scan
 * state and diagonal blocks, the downdate operands) is replicated and evolves identically on every
 * rank. ekf_upload_state / ekf_init_lowrank store the rank's tiles; ekf_download_state returns the
 * full robot rows and mean and the rank's tiles, zero elsewhere (the ranks' landmark blocks sum to
 * the instance's).
 * Per scan (Robot.cpp:126-904, the sequential association), every call asynchronous on the context
 * stream except ekf_shard_end; buf is the caller's device buffer of ekf_shard_buffer_words doubles
 * ([N][4] 2x2 blocks), which the caller sums over the ranks where marked (each rank fills the
 * blocks its tiles hold, zeros elsewhere: the sum is exact):
 *   ekf_shard_begin(enc, lines, L, buf)     predict (Robot.cpp:130-286); the rank's diagonal blocks
 *   SUM buf over ranks
 *   for each line i < L, in order:
 *     ekf_shard_line(i, buf)                gate of every landmark (Robot.cpp:313-498: the first
 *                                           passing unmatched one, found by every rank alike), the
 *                                           winner's package, the rank's blocks of its column
 *     SUM buf over ranks
 *     ekf_shard_apply(i, buf)               gain rows of every landmark, robot update (Robot.cpp:522-602)
 *   ekf_shard_end(out)                      augmentation (Robot.cpp:776-866), the capacity reset
 *                                           (Robot.cpp:893-904), commit; the step joins the flush,
 *                                           which rewrites the rank's tiles only; out[0] as
 *                                           ekf_read_results (synchronous)
 * With the same inputs the state is bit-identical to a single context's (exact arithmetic). A
 * partitioned context rejects ekf_localize, ekf_localize_device, ekf_predict and ekf_update. */
int ekf_shard_create(const ekf_config* cfg, int rank, int world, ekf_ctx** out);
int ekf_shard_tiles(const ekf_ctx* ctx, int* row_begin, int* row_end);
size_t ekf_shard_buffer_words(const ekf_ctx* ctx);
int ekf_shard_begin(ekf_ctx* ctx, const double enc[3], const ekf_line* lines, int nlines, double* buf);
int ekf_shard_line(ekf_ctx* ctx, int line, double* buf);
int ekf_shard_apply(ekf_ctx* ctx, int line, const double* buf);
int ekf_shard_end(ekf_ctx* ctx, ekf_result* out);
/* Abandons the open scan (before ekf_shard_end nothing of the committed state has been written),
 * e.g. after a failed exchange; a phase that fails abandons it too. */
int ekf_shard_abort(ekf_ctx* ctx);
/* The speculative association of a partitioned instance: the per-line exchanges replaced by one.
 *   ekf_shard_begin(enc, lines, L, buf); SUM buf over ranks
 *   ekf_shard_speculate(buf, cols)          every line's first passing landmark at the scan's start
 *                                           (its guess, found by every rank alike), the rank's
 *                                           blocks of every guessed column into cols
 *                                           (ekf_shard_spec_buffer_words doubles, [L][N][4])
 *   SUM cols over ranks
 *   ekf_shard_run(cols, next)               lines 0 .. L−1 as the per-line phases compute them, each
 *                                           winner's column from cols; stops at the first line
 *                                           whose first passing landmark is not its guess and
 *                                           writes that line (or L) as a double to next, device
 *                                           memory of the caller (asynchronous, stream-ordered;
 *                                           L + 1 when its cooperating workgroups' exchange timed
 *                                           out: abandon the scan, ekf_shard_abort)
 *   ekf_shard_resume(line)                  the host's copy of next (every rank reads the same)
 *   for each line i from next: ekf_shard_line, SUM buf, ekf_shard_apply (the per-line protocol)
 *   ekf_shard_end(out)
 * Bit-identical to the per-line protocol; every rank stops at the same line (replicated state).
 * EKF_OPT_SPECULATE = 2 (test hook) makes every line guess landmark 0. */
/* The same scan as one call, with the exchanges on the library's own RCCL communicator (RCCL is
 * loaded on first use; EKF_EDEVICE if it is not available): rank 0 gets an id with
 * ekf_rccl_unique_id, the host hands it to every rank, and each attaches with its (rank, world)
 * of ekf_shard_create. ekf_shard_localize then runs begin, SUM, speculate, SUM, run, MAX, end on
 * the context's stream before its one host read: the end phase commits only if the agreement says
 * every line ran on every rank, and otherwise changes nothing, when resume / the per-line phases
 * and the end follow (a second host read). It is bit-identical to the sequence above (Robot::localize,
 * Robot.cpp:126-904). A phase failing on any rank, or a run whose workgroups timed out, abandons
 * the scan on every rank alike (the error, or EKF_EDEVICE on the ranks where nothing failed);
 * a failed collective returns EKF_EDEVICE. */
int ekf_rccl_unique_id(unsigned char out[128]);
int ekf_shard_attach_rccl(ekf_ctx* ctx, const unsigned char id[128], int rank, int world);
int ekf_shard_localize(ekf_ctx* ctx, const double enc[3], const ekf_line* lines, int nlines, ekf_result* out);
size_t ekf_shard_spec_buffer_words(const ekf_ctx* ctx);
int ekf_shard_speculate(ekf_ctx* ctx, const double* buf, double* cols);
int ekf_shard_run(ekf_ctx* ctx, const double* cols, double* next_line);
int ekf_shard_resume(ekf_ctx* ctx, int line);

/* Introspection for the benchmark's roofline accounting. */
size_t ekf_landmark_block_bytes(const ekf_ctx* ctx); /* stored bytes of P_ll per instance */
int ekf_state_dim(const ekf_ctx* ctx);                /* n */
/* Per-kernel HIP-event timing on the stream each kernel runs on: enable 0 = off, 1 = the flush
 * only (2 events per flush), 2 = also every association kernel. Averages are over the launches
 * recorded since the last enable: scan_ms = association kernel (level 2), downdate_ms = the
 * landmark-block flush, augment_ms = 0 (augmentation is fused into the flush), launches =
 * flushes. */
int ekf_profile_enable(ekf_ctx* ctx, int enable);
int ekf_profile_read(ekf_ctx* ctx, double* scan_ms, double* downdate_ms, double* augment_ms,
                     int* launches);
/* Per-launch flush timing of the launches recorded since the last enable (level >= 1): fills
 * nsteps[k] (steps the launch applied) and ms[k] for k < min(cap, count); returns the count
 * (negative on error). ekf_flush_kernel_name: the kernel form a flush of nsteps steps runs. */
int ekf_profile_flushes(ekf_ctx* ctx, int cap, int* nsteps, float* ms);
const char* ekf_flush_kernel_name(const ekf_ctx* ctx, int nsteps);
/* Diagnostic: association-kernel phase timers (sum over instances, 100 MHz ticks), collected
 * only while EKF_OPT_SCAN_STAMPS is 1. 32 slots (ABI 2; ABI 1 had 16):
 * 0 predict, 1 diagonal gather + barrier, 2 gating, 3 min-reduction barrier, 4 winner package,
 * 5 broadcast barrier, 6 gain rows, 7 commit/augmentation, 8 total, 9 launches; 16-19 per-line
 * phases of the first landmark wave (gate, wait for the package, gain rows, robot update);
 * 20-22 gate-filter counts; the rest scripts/assoc_probe.py names. */
int ekf_debug_scan_stamps(ekf_ctx* ctx, unsigned long long out[32]);
/* Diagnostic: words 0..15 of instance e's result record as of the last ekf_read_results
 * (word 9: association path code, 10..14: the first five guessed winners, 15: 1 if the call was
 * rolled back after EKF_ST_SYNC_TIMEOUT). */
int ekf_debug_result_words(ekf_ctx* ctx, int e, int out[16]);

#ifdef __cplusplus
}
#endif
#endif /* SLAM_EKF_H */
