// ekf_shard.hip — one instance with its landmark block partitioned over ranks:
// the context (ekf_shard_create, beside ekf_create in ekf_api.hip) stores the packed tiles of its tile
// rows only; the scan runs as phases of ekf::shard_kernel over every landmark (replicated state), and the caller sums the
// [N][4] exchange buffer over the ranks between phases: the diagonal blocks after begin, the
// winner's column after each line. Everything is stream-ordered on the context stream: no host
// round trip until ekf_shard_end, where the scan joins the core's schedule as one more step.
#include <dlfcn.h>

#include <rccl/rccl.h>   // (types only: the library loads RCCL on first use, ekf_rccl_unique_id)

#include "ekf_ctx.h"

static ekf::ShardParams shard_params(ekf_ctx* c, int phase, double* buf, double* cols = nullptr)
{
    ekf::ShardParams p;
    memset(&p, 0, sizeof(p));
    p.d = c->d;
    p.phase = phase;
    p.line = c->sh_line;
    p.L = c->sh_L;
    p.r_mode = c->cfg.r_mode;
    p.gate = c->cfg.mahalanobis;
    p.enc_noise = c->cfg.encoder_noise;
    const int np = (int)(c->nsteps - c->pend0);
    p.npend = np;
    p.Pread = xview(c, c->base);
    p.t0 = c->t0;
    p.t1 = c->t1;
    for (int q = 0; q < np; q++) p.pend[q] = slot_of(c, c->pend0 + q);
    p.cur = slot_of(c, c->nsteps);
    p.Rs = strip_of(c, 0, 0);
    p.y = mean_of(c, 0, 0);
    p.pose = c->pose;
    p.saved = c->saved;
    p.rob = c->sh_rob;
    p.rec = c->sh_rec;
    p.hist = c->sh_hist;
    p.flags = c->sh_flags;
    p.pkg = c->sh_pkg;
    p.ctl = c->sh_ctl;
    p.col = buf;
    p.cols = cols;
    p.enc = c->d_enc;
    p.lines = c->d_lines;
    p.pexp = c->pexp;
    p.reset_margin = c->cfg.reset_margin;
    return p;
}

// a HIP failure inside a scan abandons it (slam_ekf.h ekf_shard_abort)
#define SH_TRY(expr)                                                                        \
    do {                                                                                    \
        hipError_t _e = (expr);                                                             \
        if (_e != hipSuccess) {                                                             \
            fprintf(stderr, "slam_ekf: %s failed: %s\n", #expr, hipGetErrorString(_e));     \
            c->sh_open = 0;                                                                 \
            return EKF_EDEVICE;                                                             \
        }                                                                                   \
    } while (0)

extern "C" int ekf_shard_tiles(const ekf_ctx* c, int* row_begin, int* row_end)
{
    if (!c || c->sh_world <= 0 || !row_begin || !row_end) return EKF_EINVAL;
    *row_begin = c->sh_r0;
    *row_end = c->sh_r1;
    return EKF_OK;
}

extern "C" size_t ekf_shard_buffer_words(const ekf_ctx* c) { return (c && c->sh_world > 0) ? 4 * (size_t)c->d.N : 0; }

extern "C" int ekf_shard_begin(ekf_ctx* c, const double enc[3], const ekf_line* lines, int nlines, double* buf)
{
    if (!c || c->sh_world <= 0 || !enc || !buf || (nlines > 0 && !lines) || c->sh_open) return EKF_EINVAL;
    if (nlines < 0 || nlines > c->d.max_lines) return EKF_ERANGE;
    c->sh_line = 0;
    c->sh_L = nlines;
    c->sh_open = 1;
    c->sh_diag = 0;
    // the inputs travel as kernel arguments of the first phase, which stores them for the later
    // ones (stream-ordered: no host staging copy, no wait for the previous scan)
    ekf::ShardParams p = shard_params(c, ekf::SH_BEGIN, buf);
    for (int k = 0; k < 3; k++) p.enc_v[k] = enc[k];
    for (int i = 0; i < c->d.max_lines; i++) {
        if (i < nlines) p.lines_v[i] = lines[i];
        else memset(&p.lines_v[i], 0, sizeof(ekf_line));
    }
    SH_TRY(ekf::launch_shard(p, c->cfg.precision, c->stream));
    return EKF_OK;
}

extern "C" int ekf_shard_line(ekf_ctx* c, int line, double* buf)
{
    if (!c || c->sh_open != 1 || !buf || line != c->sh_line) return EKF_EINVAL;
    if (line < 0 || line >= c->sh_L) return EKF_ERANGE;
    if (!c->sh_diag) {   // the summed diagonal blocks of begin's exchange
        SH_TRY(ekf::launch_shard(shard_params(c, ekf::SH_DIAG, buf), c->cfg.precision, c->stream));
        c->sh_diag = 1;
    }
    SH_TRY(ekf::launch_shard(shard_params(c, ekf::SH_GATE, buf), c->cfg.precision, c->stream));
    SH_TRY(ekf::launch_shard(shard_params(c, ekf::SH_COLUMN, buf), c->cfg.precision, c->stream));
    return EKF_OK;
}

extern "C" int ekf_shard_apply(ekf_ctx* c, int line, const double* buf)
{
    if (!c || c->sh_open != 1 || !buf || line != c->sh_line) return EKF_EINVAL;
    double* b = const_cast<double*>(buf);   // (read only by these phases)
    SH_TRY(ekf::launch_shard(shard_params(c, ekf::SH_APPLY, b), c->cfg.precision, c->stream));
    SH_TRY(ekf::launch_shard(shard_params(c, ekf::SH_ROBOT, b), c->cfg.precision, c->stream));
    c->sh_line++;
    return EKF_OK;
}

extern "C" size_t ekf_shard_spec_buffer_words(const ekf_ctx* c)
{
    return (c && c->sh_world > 0) ? 4 * (size_t)c->d.N * (size_t)c->d.max_lines : 0;
}

extern "C" int ekf_shard_speculate(ekf_ctx* c, const double* buf, double* cols)
{
    if (!c || c->sh_open != 1 || !buf || !cols || c->sh_line != 0 || c->sh_L == 0) return EKF_EINVAL;
    double* b = const_cast<double*>(buf);   // (read only by SH_DIAG)
    ekf::ShardParams pg = shard_params(c, ekf::SH_GUESS, b);
    pg.diag_first = !c->sh_diag;   // (SH_DIAG fused into the guesses' launch)
    c->sh_diag = 1;
    SH_TRY(ekf::launch_shard(pg, c->cfg.precision, c->stream));
    if (c->spec == 2)   // test hook (EKF_OPT_SPECULATE = 2): every line guesses landmark 0
        SH_TRY(hipMemsetAsync(c->sh_ctl + ekf::SC_GUESS, 0, sizeof(int) * c->d.max_lines, c->stream));
    SH_TRY(ekf::launch_shard(shard_params(c, ekf::SH_SPEC_COLS, b, cols), c->cfg.precision, c->stream));
    return EKF_OK;
}

extern "C" int ekf_shard_run(ekf_ctx* c, const double* cols, double* next_line)
{
    if (!c || c->sh_open != 1 || !cols || !next_line || !c->sh_diag || c->sh_line != 0 || c->sh_L == 0)
        return EKF_EINVAL;
    ekf::ShardParams p = shard_params(c, ekf::SH_GATE, nullptr, const_cast<double*>(cols));
    p.next_out = next_line;
    // the run's workgroups exchange through the association kernel's mailbox (unused by a
    // partitioned context: ⌈N/64⌉ ≥ shard_run_workgroups(N) slots per parity)
    p.mbox = c->mbox;
    p.mbw = c->mbw;
    p.epoch = ++c->scan_epoch;
    p.spin_log2 = c->spin_log2;
    SH_TRY(ekf::launch_shard_run(p, c->cfg.precision, c->stream));
    c->sh_line = -1;   // until ekf_shard_resume
    return EKF_OK;
}

extern "C" int ekf_shard_resume(ekf_ctx* c, int line)
{
    if (!c || c->sh_open != 1 || c->sh_line != -1 || line < 0 || line > c->sh_L) return EKF_EINVAL;
    c->sh_line = line;
    return EKF_OK;
}

// SH_END with its results mirrored into the pinned host buffers (one instance), so the result
// needs no copy: only the wait for this kernel, not for a flush behind it. gate (ekf_shard_localize):
// the ranks' agreement [failure flag, stopping line] on the device; the phase commits only if it
// says every line ran, and mirrors the pair into h_agree either way
static int shard_end_launch(ekf_ctx* c, const double* gate)
{
    ekf::ShardParams p = shard_params(c, ekf::SH_END, nullptr);
    p.res_host = c->hd_res;
    p.pose_host = c->hd_pose;
    if (gate) {
        p.end_gate = gate;
        p.end_gate_host = c->hd_agree;
    }
    SH_TRY(ekf::launch_shard(p, c->cfg.precision, c->stream));
    HIP_TRY(hipEventRecord(c->ev_scan, c->stream));
    return EKF_OK;
}

// after a committed SH_END: the step joins the deferred flush of the rank's tiles; the results
// from the mirror once the phase has finished (flushed: the wait was before the flush's launch)
static int shard_end_finish(ekf_ctx* c, ekf_result* out, bool waited)
{
    c->sh_open = 0;
    c->nsteps++;
    if (c->nsteps - c->unflushed0 >= c->T) {
        const int rc = enqueue_flush(c);
        if (rc) return rc;
    }
    if (!waited) HIP_TRY(hipEventSynchronize(c->ev_scan));
    fill_results(c, out);
    return EKF_OK;
}

extern "C" int ekf_shard_end(ekf_ctx* c, ekf_result* out)
{
    if (!c || c->sh_open != 1 || c->sh_line != c->sh_L) return EKF_EINVAL;
    // (with no line, begin's exchange is not consumed: the end needs no diagonal block)
    const int rc = shard_end_launch(c, nullptr);
    if (rc) return rc;
    return shard_end_finish(c, out, false);
}

extern "C" int ekf_shard_abort(ekf_ctx* c)
{
    // before ekf_shard_end nothing of the committed state is written (the phases use the scan's
    // scratch and the current ring slot, which only ekf_shard_end adds to the schedule)
    if (!c || c->sh_world <= 0) return EKF_EINVAL;
    c->sh_open = 0;
    HIP_TRY(hipStreamSynchronize(c->stream));
    return EKF_OK;
}

// The partitioned instance's scan as one call (ekf_shard_localize): the protocol above with the
// exchanges on the library's own RCCL communicator (ekf_shard_attach_rccl), so a C++ host (the
// drop-in Robot over ranks) needs no collective library of its own and a scan costs one call, two
// host reads (the agreement pair, then the results) and no host staging. RCCL is loaded on first
// use (dlopen): the library itself does not depend on it.
namespace {
struct RcclApi {
    ncclResult_t (*get_unique_id)(ncclUniqueId*);
    ncclResult_t (*comm_init_rank)(ncclComm_t*, int, ncclUniqueId, int);
    ncclResult_t (*all_reduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t);
    ncclResult_t (*comm_destroy)(ncclComm_t);
    const char* (*error_string)(ncclResult_t);
};
const RcclApi* rccl_api()
{
    static RcclApi api;
    static int state = 0;   // 0 not tried, 1 loaded, -1 unavailable (one thread: the context's)
    if (state == 0) {
        state = -1;
        void* h = nullptr;
        for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"})
            if ((h = dlopen(name, RTLD_NOW | RTLD_LOCAL)) != nullptr) break;
        if (h) {
            api.get_unique_id = (decltype(api.get_unique_id))dlsym(h, "ncclGetUniqueId");
            api.comm_init_rank = (decltype(api.comm_init_rank))dlsym(h, "ncclCommInitRank");
            api.all_reduce = (decltype(api.all_reduce))dlsym(h, "ncclAllReduce");
            api.comm_destroy = (decltype(api.comm_destroy))dlsym(h, "ncclCommDestroy");
            api.error_string = (decltype(api.error_string))dlsym(h, "ncclGetErrorString");
            if (api.get_unique_id && api.comm_init_rank && api.all_reduce && api.comm_destroy && api.error_string)
                state = 1;
        }
        if (state != 1) fprintf(stderr, "slam_ekf: RCCL (librccl.so) not available\n");
    }
    return state == 1 ? &api : nullptr;
}
}  // namespace

void rccl_destroy(ekf_ctx* c)
{
    const RcclApi* r = c->rccl_comm ? rccl_api() : nullptr;
    if (r) (void)r->comm_destroy((ncclComm_t)c->rccl_comm);
    c->rccl_comm = nullptr;
}

extern "C" int ekf_rccl_unique_id(unsigned char out[128])
{
    const RcclApi* r = rccl_api();
    if (!out) return EKF_EINVAL;
    if (!r) return EKF_EDEVICE;
    ncclUniqueId id;
    if (r->get_unique_id(&id) != ncclSuccess) return EKF_EDEVICE;
    static_assert(sizeof(id) == 128, "ncclUniqueId");
    memcpy(out, &id, sizeof(id));
    return EKF_OK;
}

extern "C" int ekf_shard_attach_rccl(ekf_ctx* c, const unsigned char id[128], int rank, int world)
{
    if (!c || c->sh_world <= 0 || !id || rank != c->sh_rank || world != c->sh_world || c->sh_open) return EKF_EINVAL;
    const RcclApi* r = rccl_api();
    if (!r) return EKF_EDEVICE;
    HIP_TRY(hipSetDevice(c->device));
    rccl_destroy(c);
    ncclUniqueId uid;
    memcpy(&uid, id, sizeof(uid));
    ncclComm_t comm;
    const ncclResult_t e = r->comm_init_rank(&comm, world, uid, rank);
    if (e != ncclSuccess) {
        fprintf(stderr, "slam_ekf: ncclCommInitRank: %s\n", r->error_string(e));
        return EKF_EDEVICE;
    }
    c->rccl_comm = comm;
    const size_t words = 4 * (size_t)c->d.N, swords = words * (size_t)c->d.max_lines;
    if (!c->sh_xbuf || !c->sh_xcols || !c->h_agree) {
        // all three or none: a failure part way frees what was allocated, so a later attach
        // allocates again instead of finding one pointer set and the others null
        auto drop = [c]() {
            if (c->sh_xbuf) (void)hipFree(c->sh_xbuf);
            if (c->sh_xcols) (void)hipFree(c->sh_xcols);
            if (c->h_agree) (void)hipHostFree(c->h_agree);
            c->sh_xbuf = c->sh_xcols = c->h_agree = c->hd_agree = nullptr;
        };
        drop();
        if (hipMalloc((void**)&c->sh_xbuf, sizeof(double) * (words + 1)) != hipSuccess ||
            hipMalloc((void**)&c->sh_xcols, sizeof(double) * (swords + 2)) != hipSuccess ||
            hipHostMalloc((void**)&c->h_agree, sizeof(double) * 4) != hipSuccess ||
            hipHostGetDevicePointer((void**)&c->hd_agree, c->h_agree, 0) != hipSuccess ||
            hipMemset(c->sh_xbuf, 0, sizeof(double) * (words + 1)) != hipSuccess ||
            hipMemset(c->sh_xcols, 0, sizeof(double) * (swords + 2)) != hipSuccess) {
            drop();
            rccl_destroy(c);
            return EKF_EDEVICE;
        }
    }
    c->sh_dirty = 0;
    return EKF_OK;
}

extern "C" int ekf_shard_localize(ekf_ctx* c, const double enc[3], const ekf_line* lines, int nlines, ekf_result* out)
{
    if (!c || c->sh_world <= 0 || !c->rccl_comm || !enc || (nlines > 0 && !lines) || c->sh_open) return EKF_EINVAL;
    if (nlines < 0 || nlines > c->d.max_lines) return EKF_ERANGE;
    const RcclApi* r = rccl_api();
    const int L = nlines;
    const size_t words = 4 * (size_t)c->d.N, swords = words * (size_t)c->d.max_lines;
    double* buf = c->sh_xbuf;
    double* cols = c->sh_xcols;
    double* agree = cols + swords;   // [failure flag (the columns' flag word), stopping line]
    ncclComm_t comm = (ncclComm_t)c->rccl_comm;
    auto sum = [&](double* b, size_t n, ncclRedOp_t op) {
        return r->all_reduce(b, b, n, ncclFloat64, op, comm, c->stream) == ncclSuccess;
    };
    // a phase that fails on one rank must not leave the others waiting in an exchange: every rank
    // runs the whole exchange sequence, a failed one without further phases, and the summed flag
    // words tell every rank alike whether to abandon the scan
    static const double one_l[2] = {1.0, 0.0};
    auto flag = [&](double* w) {
        c->sh_dirty = 1;
        return hipMemcpyAsync(w, one_l, sizeof(double), hipMemcpyHostToDevice, c->stream) == hipSuccess;
    };
    if (c->sh_dirty) {
        HIP_TRY(hipMemsetAsync(buf + words, 0, sizeof(double), c->stream));
        HIP_TRY(hipMemsetAsync(agree, 0, 2 * sizeof(double), c->stream));
        c->sh_dirty = 0;
    }
    int err = ekf_shard_begin(c, enc, lines, L, buf);
    if (err && !flag(buf + words)) return EKF_EDEVICE;
    if (!sum(buf, words + 1, ncclSum)) return EKF_EDEVICE;
    int first = 0;
    bool abandon = false, spec_all = false;
    if (c->spec && L > 0) {
        if (!err) err = ekf_shard_speculate(c, buf, cols);
        if (err && !flag(agree)) return EKF_EDEVICE;
        if (!sum(cols, swords + 1, ncclSum)) return EKF_EDEVICE;
        if (!err) err = ekf_shard_run(c, cols, agree + 1);
        if (err) {
            const double v[2] = {1.0, (double)L};
            HIP_TRY(hipMemcpyAsync(agree, v, sizeof(v), hipMemcpyHostToDevice, c->stream));
            c->sh_dirty = 1;
        }
        if (!sum(agree, 2, ncclMax)) return EKF_EDEVICE;
        // the end phase goes behind the run before the host reads the agreement: it commits only if
        // every line ran on every rank (the common case: one host round trip per scan), and leaves
        // everything untouched otherwise, when the lines from the agreed one follow as below
        bool gated = false;
        if (!err) {
            c->sh_line = L;
            err = shard_end_launch(c, agree);
            gated = !err;
        }
        if (!gated)
            HIP_TRY(hipMemcpyAsync(c->h_agree, agree, 2 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        abandon = c->h_agree[0] > 0.0 || c->h_agree[1] > (double)L;   // (past L: a run timed out)
        first = abandon ? L : (int)c->h_agree[1];
        if (gated && !abandon && first == L) return shard_end_finish(c, out, true);
        if (gated) c->sh_line = -1;   // (not committed: the run's state stands, as after ekf_shard_run)
        // (host bookkeeping only, on the agreed line: it fails on every rank alike or on none)
        if (!abandon && !err) err = ekf_shard_resume(c, first);
        spec_all = first == L;
    }
    for (int i = first; i < L; i++) {
        if (!err) err = ekf_shard_line(c, i, buf);
        if (err && !flag(buf + words)) return EKF_EDEVICE;
        if (!sum(buf, words + 1, ncclSum)) return EKF_EDEVICE;
        if (!err) err = ekf_shard_apply(c, i, buf);
    }
    double failed;
    if (spec_all) {
        failed = c->h_agree[0];   // (the agreement carried every failure flag)
    } else {
        if (L > first) {
            // the last line's apply ran after its exchange: one more word, the MAX over the ranks
            // of the summed flags and of every rank's failure since, so that a rank whose apply
            // failed does not abandon the scan alone while its peers commit it
            if (err && !flag(buf + words)) return EKF_EDEVICE;
            if (!sum(buf + words, 1, ncclMax)) return EKF_EDEVICE;
        }
        HIP_TRY(hipMemcpyAsync(c->h_agree + 2, buf + words, sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        failed = c->h_agree[2];
    }
    if (abandon || failed > 0.0 || err) {
        c->sh_dirty = 1;
        (void)ekf_shard_abort(c);
        return err ? err : EKF_EDEVICE;   // (a peer's phase failed, or the run's exchange timed out)
    }
    return ekf_shard_end(c, out);
}
