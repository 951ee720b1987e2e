// ekf_ctx.h — the context behind the C-ABI and everything its five host units share (internal):
//   ekf_api.hip    the core: creation, options, the schedule (scans, flushes, drain), results, profiling;
//   ekf_state.hip  the calls that read or write one instance's state without a scan: reset, upload,
//                  download, low-rank initialisation, rescale, pose covariance, ellipse (ekf_ellipse.h);
//   ekf_shard.hip  the partitioned instance: the ekf_shard_* protocol, RCCL, ekf_shard_localize;
//   ekf_read.hip   the calls that read without draining: covariance queries, gate, joint gate, joint search,
//                  landmark pairs;
//   ekf_copy.hip   the calls that copy instances without draining: ekf_resample, the instance images.
#pragma once

#include <stdio.h>
#include <string.h>

#include <vector>

#include "ekf_kernels.h"   // (the HIP runtime, slam_ekf.h)

using ekf::Dims;

struct EvPair {
    hipEvent_t a, b;
};

// Pinned host memory the kernels read or write through its device pointer, grown to the largest request
// so far and kept (pinned_reserve: the contents are not kept across a growth; free_all releases it)
struct PinnedBuf {
    char* host = nullptr;
    char* dev = nullptr;
    size_t cap = 0;   // bytes
};

struct ekf_ctx {
    ekf_config cfg;
    Dims d;
    int device;
    hipStream_t own_stream;   // S unless the caller supplies one
    hipStream_t stream;       // S
    hipStream_t dstream;      // D
    size_t elem;              // bytes per stored landmark-block element
    size_t op_elem;           // bytes per downdate operand element (fp32 for fp16 storage)
    size_t pll_inst;          // elements per instance (the whole packed block)
    long long t0 = 0, t1 = 0; // tiles stored per instance [t0, t1): all, unless partitioned (ekf_shard_create)
    size_t xinst;             // stored landmark-block elements per instance ((t1 − t0)·TILE_ELEMS)
    size_t op_inst;           // operand elements per instance
    std::vector<void*> dev_mem;      // every device buffer create_ctx made (dev_alloc), freed by free_all
    std::vector<void*> pinned_mem;   // ... and every pinned host buffer (pinned_alloc)
    void* X[2];
    double* Rs;               // [2][E][3][n] robot strip, two copies (the association kernel reads
    double* y;                // [2][E][n]    copy cur[e] and writes the other; the lead commits it)
    int* cur;                 // [E] committed copy per instance (device; read back when needed)
    double* dense = nullptr;   // n × n fp64 scratch of upload / download / rescale (allocated on first use, kept)
    // the host queries' result buffers (ekf_query_joint / ekf_query_marginals), sized to the largest
    // request so far and kept: device scratch, and pinned host memory the one copy lands in, with the
    // request's inputs behind the results (the kernel reads them through q_pin.dev)
    double* q_dev = nullptr;
    size_t q_dev_bytes = 0;
    PinnedBuf q_pin;
    // ekf_gate_lines: the candidates' flag bytes [E][max_lines][N] and the waves' partial records
    // [E][max_lines][⌈N/64⌉] (listed context memory, made on first use); predicted: ekf_predict ran and
    // no update, localize or state write since (the committed strip is the predicted one)
    unsigned char* g_flags = nullptr;
    ekf::GatePart* g_part = nullptr;
    int predicted = 0;
    // ekf_gate_landmarks: the partial records [E][N][⌈N/64⌉] of every landmark against every partner block
    // (ekf_pairs.h PairParams; listed context memory, made on first use)
    ekf_pair_hit* pr_part = nullptr;
    // ekf_associate_joint: the rows' plans, candidate and pair tables and the search workgroups' records
    // (ekf_kernels.h AssocParams; listed context memory, made on first use)
    ekf::AssocPlan* as_plan = nullptr;
    double* as_ctab = nullptr;
    double* as_ptab = nullptr;
    ekf::AssocRec* as_rec = nullptr;
    // ekf_resample and the device forms of the instance images: the copy table in pinned host memory
    // the kernel reads (sized to the largest call so far and kept), and the event behind the last
    // launch that reads it
    PinnedBuf rs_pin;
    hipEvent_t rs_ev = nullptr;
    int rs_pending = 0;
    // ekf_resample_device: the checked list the copy reads (kernels.h resample_device_plan_words; listed
    // context memory, made on first use). The call cannot update pexp_h, so it marks it stale and the
    // readers of pexp_h re-read the device array first (pexp_mirror)
    int32_t* rsd_plan = nullptr;
    int pexp_stale = 0;
    // partitioned instance (ekf_shard_create): rank sh_rank of sh_world stores tile rows [sh_r0, sh_r1);
    // the running scan's replicated state
    int sh_rank = -1, sh_world = 0, sh_r0 = 0, sh_r1 = 0;
    double* sh_rob = nullptr;
    double* sh_rec = nullptr;
    double* sh_hist = nullptr;
    double* sh_pkg = nullptr;
    int* sh_flags = nullptr;
    int* sh_ctl = nullptr;
    int sh_L = 0, sh_line = 0, sh_open = 0;   // sh_open: 1 during a scan; sh_line: the next line expected
    int sh_diag = 0;                           // begin's exchange consumed (SH_DIAG ran) in this scan
    ekf::Slot sh_null;        // a step that applies nothing (pads an odd partial group to the wave flush)
    double* pose;
    double* xpre;
    int* saved;
    double* D;                // [2][E][N][4] diagonal landmark blocks after the last committed step
                              // (split-bf16 contexts: the association kernel's MFMA replay)
    std::vector<ekf::Slot> ring;   // R per-step slots
    double* Ust;              // fp64 gain scratch of the running scan
    double* Vst;
    int2* tile_rc;
    int2* stile_rc;
    int2* stile2_rc;
    int nstiles2;
    ekf::WtEntry* wt;
    int nwt;
    ekf::WtEntry* wt64;
    int nwt64;
    int* wt24;                // split-bf16 wave-tiles of 2 × 4 tiles (wr | wc << 16), panel order
    int nwt24;
    ekf::WtEntry* wtq;        // split-fp16 quad form: groups of 2 × 2 wave-tiles (four entries each)
    int nwtq;
    double* d_enc;            // the scan inputs: views of d_in, staged from h_in by one copy
    ekf_line* d_lines;
    int* d_nlines;
    char* d_in;
    char* h_in;               // pinned
    size_t in_lines, in_nlines, in_bytes;   // byte offsets of the lines and counts, the total
    int in_pending;           // a copy from h_in was enqueued (ev_in)
    hipEvent_t ev_in;
    void* rccl_comm;          // ekf_shard_attach_rccl: the partitioned instance's own communicator
    double* sh_xbuf;          // ... and ekf_shard_localize's exchange buffers (device): [N][4] + flag,
    double* sh_xcols;         // [L][N][4] + flag + stopping line
    double* h_agree;          // pinned: the agreement pair and a flag word
    double* hd_agree;         // (its device pointer)
    int sh_dirty;             // a failed scan left nonzero flag words
    int* h_res;
    double* h_pose;
    // the synchronous calls' result mirror (ScanParams::res_host): pinned, written by the scan's
    // lead; h_r33 the robot block, h_ep the epoch of each instance's last mirrored commit
    double* h_r33;
    unsigned* h_ep;
    int* hd_res;              // (their device pointers)
    double* hd_pose;
    double* hd_r33;
    unsigned* hd_ep;
    int mirror_on;            // the association launch being enqueued writes the mirror
    unsigned mirror_epoch;    // scan_epoch of the mirrored robot blocks (0: none valid)
    int dd_grid;
    int dd_per_cu;            // flush workgroups per CU of the grid-strided forms (EKF_OPT_FLUSH_BLOCKS_PER_CU)
    int dd_variant;           // f32 flush kernel form (EKF_OPT_FLUSH_FORM)
    int ncu;
    int G;                    // association workgroups per instance
    int mbw;                  // mailbox words per workgroup slot
    int spec;                 // speculative association (EKF_OPT_SPECULATE)
    int spin_log2;            // spin bound of the association kernel's waits (EKF_OPT_SPIN_LOG2)
    int test_drop;            // test hook (EKF_OPT_TEST_DROP_WG = e + 1): instance e's last workgroup never runs
    int test_verdict;         // test hook (EKF_OPT_TEST_VERDICT_TIMEOUT = e + 1)
    int mfrep_opt;            // EKF_OPT_MFMA_REPLAY
    int active_flush;         // EKF_OPT_ACTIVE_FLUSH
    int mfrep;                // split-bf16 contexts: MFMA replay of pending steps (bf && mfrep_opt)
    int scan_batch;           // instances per association launch (co-residency bound), 192 wide
    int resident;             // association workgroups the device holds at once
    int nt_opt;               // EKF_OPT_SCAN_THREADS
    int Gmax;                 // workgroups per instance at the narrowest width (mailbox, sync words)
    int last_G;               // workgroups per instance of the last association launch
    unsigned scan_epoch;      // association launches so far (mailbox tags)
    double* mbox;
    int* sync;
    int sync_stride;
    unsigned long long* dbg;  // association-kernel phase timers (EKF_OPT_SCAN_STAMPS = 1, else null)
    int* pexp;                // [E] fp16 storage exponents (device), host copy below
    void* sink;               // scratch tile for the wave flushes (DowndateParams::sink)
    void* ops_u;              // operand rows of every ring slot (U), slot_bytes apart
    void* ops_v;              // ... (V)
    long long slot_bytes;
    void* ops_b;              // split-plane arithmetics: the planes of V of every ring slot (else null)
    long long bslot_bytes;
    bool bf;                  // a split-plane flush applies (arith, fp32 operands, symmetric R, kmax 16)
    int pmode;                // its plane arithmetic: 1 EKF_ARITH_BF16X6, 2 EKF_ARITH_F16X3 (0: none)
    int* psig;                // [E] EKF_ARITH_F16X3 plane exponent σ (device; the association kernel's
    double* pvmax;            // [E] lead lowers it when a new landmark raises the largest variance)
    std::vector<int> pexp_h;
    // flush scheduling (see the top of ekf_api.hip)
    int T;                    // flush interval
    long long nsteps;         // update steps enqueued
    long long unflushed0;     // first step not covered by an enqueued flush
    long long pend0;          // first step not contained in X[base]
    int base;                 // buffer the association kernels read
    int last_out;             // buffer the newest enqueued flush writes (materialised after drain)
    long long nflush;
    hipEvent_t ev_scan;       // recorded on S after each update scan
    hipEvent_t ev_flush[2];   // recorded on D after flush f (f & 1)
    hipEvent_t ev_base;       // event guarding X[base] and the ring (nullptr: none pending)
    // profiling
    int prof;
    std::vector<EvPair> ev[3];   // scan, downdate, patch
    std::vector<int> ev_nsteps;  // steps applied by each timed flush (ev[1])
    std::vector<EvPair> pool;
};

#define HIP_TRY(expr)                                                                       \
    do {                                                                                    \
        hipError_t _e = (expr);                                                             \
        if (_e != hipSuccess) {                                                             \
            fprintf(stderr, "slam_ekf: %s failed: %s\n", #expr, hipGetErrorString(_e));     \
            return EKF_EDEVICE;                                                             \
        }                                                                                   \
    } while (0)

static inline int cur_buf(const ekf_ctx* c) { return c->last_out; }

// instance e's stored tiles in buffer buf (xview: the kernels' view of instance 0)
static inline char* xinst_ptr(const ekf_ctx* c, int buf, int e)
{
    return (char*)c->X[buf] + (size_t)e * c->xinst * c->elem;
}

// copy cb (strip_copy) of instance e's robot strip and mean
static inline double* strip_of(const ekf_ctx* c, int cb, int e)
{
    return c->Rs + ((size_t)cb * c->cfg.instances + e) * 3 * c->d.n;
}

static inline double* mean_of(const ekf_ctx* c, int cb, int e)
{
    return c->y + ((size_t)cb * c->cfg.instances + e) * c->d.n;
}

// ---- what crosses the host units; not exported from the library. Defined in ekf_api.hip, except the
// last two ----
#pragma GCC visibility push(hidden)
bool dev_alloc(ekf_ctx* c, void** p, size_t bytes);   // zeroed device memory on the context's list
int pinned_reserve(PinnedBuf& b, size_t bytes);       // EKF_OK, EKF_ENOMEM or EKF_EDEVICE (b then empty)
int usym_of(const ekf_ctx* c);
const ekf::Slot& slot_of(const ekf_ctx* c, long long k);   // step k's ring slot
void* xview(const ekf_ctx* c, int buf);
// Behind work enqueued on S that reads or writes X[base] or the ring outside a scan: the next flush on D
// waits for it too
int end_read(ekf_ctx* c);
int drain(ekf_ctx* c);           // flushes the partial group, waits for S and D: X[last_out] is the block
int enqueue_flush(ekf_ctx* c);   // one flush of the steps [unflushed0, nsteps), if any (who adds a step calls it at T)
void fill_results(const ekf_ctx* c, ekf_result* out);   // out[E] (or null) from the host copies h_res, h_pose
int strip_copy(ekf_ctx* c, int e, int* cb);   // waits for S; *cb: instance e's committed strip and mean, 0 or 1
int pexp_mirror(ekf_ctx* c);     // before reading pexp_h: if a device-side resample left it stale, waits for S and re-reads pexp
int set_robot_ctor(ekf_ctx* c, int e, double x, double y, double th);   // (ekf_state.hip) Robot::Robot; waits for S
void rccl_destroy(ekf_ctx* c);   // (ekf_shard.hip) the context's communicator, if it has one
#pragma GCC visibility pop
