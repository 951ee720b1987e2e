// ekf_api.hip — the core of the C-ABI (include/slam_ekf.h) over the gfx950 kernels (launchers: unit_*.hip):
// the context's creation, options, the schedule of scans and flushes, results, profiling. A step's whole
// host path is in this unit. The other host units (ekf_ctx.h lists them and what they share with this
// one): ekf_state.hip, ekf_shard.hip, ekf_read.hip, ekf_copy.hip.
//
// A context owns E instances' state in HBM and two HIP streams:
//   S  association/gain kernels (scan_kernel) — all state except the landmark block — and, on
//      the sequential schedule, the flushes too (stream order is the only dependency);
//   D  the landmark-block flush of the pipelined schedule.
// Every update step k writes its downdate operands, augmented rows and result record into slot
// k mod R of a ring. The landmark block is rewritten by a flush once per group of T =
// flush_interval steps; association kernels read the last materialised block ("base") with the
// steps not yet in it applied on read (bit-identical to flushing first, see ekf_device.h).
//   sequential (pipeline = 0): one buffer, flushed in place on S after the group's last scan;
//     R = T.
//   pipelined  (pipeline = 1): flush f reads X[in] and writes X[out] = the other buffer while the
//     next group's scans run on S reading X[in] — the output of flush f-1 — with the steps of
//     groups f and f+1 pending (< 2T); R = 2T.
// Any call that reads the whole landmark block or replaces it drains (flushes the partial group,
// syncs); the covariance queries (ekf_query_*) and the gate queries (ekf_gate_lines*, ekf_gate_joint*) read chosen
// blocks as an association kernel would, with the pending steps applied on read, and leave the
// schedule as it is. ekf_resample copies instances onto others with their pending steps, mid-group,
// and leaves it as it is too; ekf_export_instances / ekf_import_instances do the same between
// contexts that stand at the same point of their flush groups.
#include <math.h>
#include <stdlib.h>

#include <algorithm>
#include <new>

#include "ekf_ctx.h"

extern "C" {

void ekf_config_init(ekf_config* c)
{
    if (!c) return;
    memset(c, 0, sizeof(*c));
    c->capacity = 100;        // Robot.h:13
    c->instances = 1;
    c->precision = EKF_PREC_F64;
    c->device = -1;
    c->max_lines = 20;        // main.cpp:99 lines.reserve(20)
    c->r_mode = EKF_R_INTENDED;
    c->reset_margin = 10;     // Robot.cpp:893
    c->mahalanobis = 0.4;     // Robot.h:15
    c->encoder_noise = 0.024; // Robot.h:17
}

const char* ekf_strerror(int s)
{
    switch (s) {
    case EKF_OK: return "ok";
    case EKF_EINVAL: return "invalid argument";
    case EKF_ENOMEM: return "out of memory";
    case EKF_EDEVICE: return "HIP device error";
    case EKF_ERANGE: return "index out of range";
    default: return "unknown error";
    }
}

int ekf_abi_version(void) { return SLAM_EKF_ABI_VERSION; }

}  // extern "C"

// The context's memory: every buffer create_ctx makes goes through these two and is freed from the
// lists (free_all); only the buffers made or remade later are freed by name
bool dev_alloc(ekf_ctx* c, void** p, size_t bytes)
{
    if (hipMalloc(p, bytes) != hipSuccess) return false;
    c->dev_mem.push_back(*p);
    return hipMemset(*p, 0, bytes) == hipSuccess;
}

static bool pinned_alloc(ekf_ctx* c, void** p, size_t bytes)
{
    if (hipHostMalloc(p, bytes) != hipSuccess) return false;
    c->pinned_mem.push_back(*p);
    return true;
}

static void pinned_release(PinnedBuf& b)
{
    if (b.host) (void)hipHostFree(b.host);
    b = PinnedBuf();
}

int pinned_reserve(PinnedBuf& b, size_t bytes)
{
    if (bytes <= b.cap) return EKF_OK;
    pinned_release(b);
    if (hipHostMalloc((void**)&b.host, bytes) != hipSuccess) {
        b.host = nullptr;
        return EKF_ENOMEM;
    }
    if (hipHostGetDevicePointer((void**)&b.dev, b.host, 0) != hipSuccess) {
        pinned_release(b);
        return EKF_EDEVICE;
    }
    b.cap = bytes;
    return EKF_OK;
}

// A host-built table (ekf_tables.h) into device memory of its own; *count: its entries
static_assert(sizeof(ekf::TileRC) == sizeof(int2) && alignof(ekf::TileRC) <= alignof(int2) &&
                  offsetof(ekf::TileRC, x) == offsetof(int2, x) && offsetof(ekf::TileRC, y) == offsetof(int2, y),
              "ekf::TileRC is the kernels' int2");
template <typename D, typename V>
static bool upload_table(ekf_ctx* c, D** dst, const std::vector<V>& table, int* count = nullptr)
{
    static_assert(sizeof(D) == sizeof(V), "the table's entries as the kernels read them");
    const size_t bytes = sizeof(V) * table.size();
    if (count) *count = (int)table.size();
    return dev_alloc(c, (void**)dst, bytes) && hipMemcpy(*dst, table.data(), bytes, hipMemcpyHostToDevice) == hipSuccess;
}

static void free_all(ekf_ctx* c)
{
    for (void* p : c->dev_mem) (void)hipFree(p);
    for (void* p : {(void*)c->dbg, (void*)c->dense, (void*)c->q_dev, (void*)c->sh_xbuf, (void*)c->sh_xcols})
        (void)hipFree(p);   // (or null)
    pinned_release(c->q_pin);
    pinned_release(c->rs_pin);
    if (c->rs_ev) (void)hipEventDestroy(c->rs_ev);
    for (void* p : c->pinned_mem) (void)hipHostFree(p);
    if (c->h_agree) (void)hipHostFree(c->h_agree);
    if (c->ev_in) (void)hipEventDestroy(c->ev_in);
    for (auto& v : c->ev)
        for (auto& pr : v) { (void)hipEventDestroy(pr.a); (void)hipEventDestroy(pr.b); }
    for (auto& pr : c->pool) { (void)hipEventDestroy(pr.a); (void)hipEventDestroy(pr.b); }
    if (c->ev_scan) (void)hipEventDestroy(c->ev_scan);
    for (int k = 0; k < 2; k++)
        if (c->ev_flush[k]) (void)hipEventDestroy(c->ev_flush[k]);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    if (c->dstream) (void)hipStreamDestroy(c->dstream);
}

// Flush the partial group and wait for both streams; afterwards X[last_out] is the materialised
// landmark block and nothing is pending.
int drain(ekf_ctx* c)
{
    if (c->nsteps > c->unflushed0) {
        int rc = enqueue_flush(c);
        if (rc) return rc;
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipStreamSynchronize(c->dstream));
    c->base = c->last_out;
    c->pend0 = c->nsteps;
    c->ev_base = nullptr;
    return EKF_OK;
}

int end_read(ekf_ctx* c)
{
    // Pipelined schedule: the next flush (a drain's, or the group's) writes X[base] on D, ordered
    // only after ev_scan, which the last scan recorded before this work was enqueued. ev_scan is
    // recorded again here, behind the work on S, so that flush also waits for it.
    if (c->cfg.pipeline) HIP_TRY(hipEventRecord(c->ev_scan, c->stream));
    return EKF_OK;
}

// the kernels' view of instance 0 in buffer buf, in which tile t sits at t·TILE_ELEMS (a partitioned
// instance stores the tiles [t0, t1) only: the view is shifted)
void* xview(const ekf_ctx* c, int buf)
{
    return (char*)c->X[buf] - (ptrdiff_t)c->t0 * ekf::TILE_ELEMS * (ptrdiff_t)c->elem;
}

// Committed copy of instance e's robot strip and mean (the association kernel flips it when it
// commits a launch): read back after the stream has drained up to here.
int strip_copy(ekf_ctx* c, int e, int* cb)
{
    HIP_TRY(hipMemcpyAsync(cb, c->cur + e, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (*cb != 0 && *cb != 1) return EKF_EDEVICE;
    return EKF_OK;
}

// The host copy of the storage exponents after ekf_resample_device, whose list the host never saw
int pexp_mirror(ekf_ctx* c)
{
    if (!c->pexp_stale) return EKF_OK;
    HIP_TRY(hipMemcpyAsync(c->pexp_h.data(), c->pexp, sizeof(int) * c->pexp_h.size(), hipMemcpyDeviceToHost,
                           c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->pexp_stale = 0;
    return EKF_OK;
}

// ---- create_ctx's steps, in the order it takes them. Each returns a status and leaves what it made on
// the context's lists or in its named members, so one failure path (free_all) serves them all.
#define ALLOC(ptr, bytes) do { if (!dev_alloc(c, (void**)&(ptr), (bytes))) return EKF_ENOMEM; } while (0)

static int validate(const ekf_config* cfg, int* device)
{
    // capacity bound: one association thread per landmark, at most MAX_GROUPS workgroups of
    // SCAN_THREADS per instance (N <= 32768, i.e. n <= 65539)
    if (cfg->capacity < 1 || cfg->capacity > ekf::MAX_CAPACITY ||
        cfg->instances < 1 ||
        cfg->max_lines < 1 ||
        cfg->max_lines > EKF_MAX_LINES ||
        (cfg->precision != EKF_PREC_F64 && cfg->precision != EKF_PREC_F32 &&
         cfg->precision != EKF_PREC_F16) ||
        (cfg->r_mode != EKF_R_INTENDED && cfg->r_mode != EKF_R_AS_WRITTEN) ||
        cfg->flush_interval < 0 ||
        cfg->flush_interval > (cfg->arith == EKF_ARITH_F16X3 ? ekf::F16X3_MAXS : 16) ||
        (cfg->arith != EKF_ARITH_EXACT && cfg->arith != EKF_ARITH_BF16X6 && cfg->arith != EKF_ARITH_F16X3) ||
        // the split-plane flushes need symmetric fp32 operands with kmax = 16 (slam_ekf.h)
        (cfg->arith != EKF_ARITH_EXACT &&
         (cfg->precision == EKF_PREC_F64 || cfg->r_mode != EKF_R_INTENDED || cfg->max_lines > 8)))
        return EKF_EINVAL;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return EKF_EDEVICE;
    if (cfg->device >= 0 && (cfg->device >= ndev || hipSetDevice(cfg->device) != hipSuccess)) return EKF_EDEVICE;
    (void)hipGetDevice(device);
    return EKF_OK;
}

// sizes, the rank's tiles, the association grid
static int set_dims(ekf_ctx* c, int sh_rank, int sh_world)
{
    const ekf_config& cfg = c->cfg;
    c->d = ekf::make_dims(cfg.capacity, cfg.max_lines);
    const Dims& d = c->d;
    c->elem = (cfg.precision == EKF_PREC_F64) ? 8 : (cfg.precision == EKF_PREC_F32) ? 4 : 2;
    c->op_elem = (cfg.precision == EKF_PREC_F64) ? 8 : 4;   // operands in the compute type
    c->pll_inst = (size_t)d.ntiles * ekf::TILE_ELEMS;
    c->t1 = d.ntiles;
    if (sh_world > 0) {
        ekf::tile_partition(d.nb, sh_world, sh_rank, c->sh_r0, c->sh_r1);
        if (c->sh_r0 >= c->sh_r1) return EKF_ERANGE;   // more ranks than wave-tile rows
        c->sh_rank = sh_rank;
        c->sh_world = sh_world;
        c->t0 = ekf::tile_index(c->sh_r0, c->sh_r0, d.nb);
        c->t1 = c->sh_r1 < d.nb ? ekf::tile_index(c->sh_r1, c->sh_r1, d.nb) : d.ntiles;
    }
    c->xinst = (size_t)(c->t1 - c->t0) * ekf::TILE_ELEMS;
    c->op_inst = (size_t)d.nb * 64 * (d.kmax / 2);
    c->G = (d.N + ekf::SCAN_THREADS - 1) / ekf::SCAN_THREADS;
    c->Gmax = (d.N + 63) / 64;   // EKF_OPT_SCAN_THREADS = 64
    c->last_G = c->G;
    // pipeline: the association kernels of an instance spread over G > 1 cooperating workgroups
    // must never wait on CUs a flush holds, so they are ordered after the flush in flight, and
    // nothing would overlap: such contexts run the sequential schedule (slam_ekf.h)
    if (c->G > 1) c->cfg.pipeline = 0;
    return EKF_OK;
}

static int make_state(ekf_ctx* c)
{
    const Dims& d = c->d;
    const int E = c->cfg.instances;
    ALLOC(c->X[0], c->xinst * c->elem * E);
    if (c->cfg.pipeline) ALLOC(c->X[1], c->xinst * c->elem * E);
    ALLOC(c->Rs, sizeof(double) * 3 * d.n * E * 2);
    ALLOC(c->y, sizeof(double) * d.n * E * 2);
    ALLOC(c->cur, sizeof(int) * E);
    ALLOC(c->pose, sizeof(double) * 3 * E);
    ALLOC(c->xpre, sizeof(double) * 3 * E);
    ALLOC(c->saved, sizeof(int) * E);
    ALLOC(c->D, sizeof(double) * 4 * d.N * E * 2);
    ALLOC(c->Ust, sizeof(double) * d.max_lines * d.n * 2 * E);
    ALLOC(c->Vst, sizeof(double) * d.max_lines * d.n * 2 * E);
    return EKF_OK;
}

// the ring of per-step slots and their operand buffers
static int make_ring(ekf_ctx* c)
{
    const Dims& d = c->d;
    const int E = c->cfg.instances;
    c->T = c->cfg.flush_interval > 0 ? c->cfg.flush_interval : 1;
    c->ring.assign((size_t)c->T * (c->cfg.pipeline ? 2 : 1), ekf::Slot{});
    // the operand rows of all slots in two contiguous buffers (fixed slot stride): the wave
    // flush addresses step q's rows from one base and its ring index (DowndateParams::ubase)
    c->slot_bytes = (long long)(((c->op_inst * c->op_elem * E) + 255) / 256 * 256);
    ALLOC(c->ops_u, (size_t)c->slot_bytes * c->ring.size());
    ALLOC(c->ops_v, (size_t)c->slot_bytes * c->ring.size());
    // split-plane flushes: V's planes per slot (written by the association kernel), three bf16
    // (BF16X6) or two fp16 (F16X3) per operand element
    c->bf = c->cfg.arith != EKF_ARITH_EXACT;   // (validated: fp32 / fp16, symmetric R, kmax 16)
    c->pmode = c->bf ? c->cfg.arith : 0;
    if (c->bf) {
        const int npl = c->pmode == EKF_ARITH_F16X3 ? 2 : 3;
        c->bslot_bytes = (long long)((c->op_inst * npl * 2 * E + 255) / 256 * 256);
        ALLOC(c->ops_b, (size_t)c->bslot_bytes * c->ring.size());
    }
    ALLOC(c->psig, sizeof(int) * E);
    ALLOC(c->pvmax, sizeof(double) * E);
    for (size_t i = 0; i < c->ring.size(); i++) {
        ekf::Slot& sl = c->ring[i];
        sl.Uop = (char*)c->ops_u + (size_t)c->slot_bytes * i;
        sl.Vop = (char*)c->ops_v + (size_t)c->slot_bytes * i;
        sl.Bop = c->bf ? (char*)c->ops_b + (size_t)c->bslot_bytes * i : nullptr;
        ALLOC(sl.patch, sizeof(double) * d.max_lines * 2 * d.M * E);
        ALLOC(sl.patch_diag, sizeof(double) * d.max_lines * 4 * E);
        ALLOC(sl.res, sizeof(int) * ekf::RES_STRIDE * E);
    }
    return EKF_OK;
}

// the flush kernels' tile tables (ekf_tables.h). A partitioned instance flushes its tile rows
// only: its wave tables keep those rows, and it has no quad table
static int make_tables(ekf_ctx* c)
{
    const Dims& d = c->d;
    const bool part = c->sh_world > 0;
    const auto wt = ekf::wt_table(d.nb), wt64 = ekf::wt64_table(d.nb);
    if (!upload_table(c, &c->tile_rc, ekf::tile_rc_table(d.nb)) ||
        !upload_table(c, &c->stile_rc, ekf::stile_rc_table(d.nb)) ||
        !upload_table(c, &c->stile2_rc, ekf::stile2_rc_table(d.nb), &c->nstiles2) ||
        !upload_table(c, &c->wt, part ? ekf::keep_tile_rows(wt, ekf::WT_R, c->sh_r0, c->sh_r1) : wt, &c->nwt) ||
        !upload_table(c, &c->wt64, part ? ekf::keep_tile_rows(wt64, 1, c->sh_r0, c->sh_r1) : wt64, &c->nwt64) ||
        !upload_table(c, &c->wt24, ekf::wt24_table(d.nb), &c->nwt24) ||
        (!part && !upload_table(c, &c->wtq, ekf::wtq_table(d.nb), &c->nwtq)))
        return EKF_ENOMEM;
    return EKF_OK;
}

// the scan's device inputs, its mailbox, and the options' defaults
static int make_scan_buffers(ekf_ctx* c)
{
    const Dims& d = c->d;
    const int E = c->cfg.instances;
    c->in_lines = ((sizeof(double) * 3 * E + 15) / 16) * 16;
    c->in_nlines = c->in_lines + ((sizeof(ekf_line) * d.max_lines * E + 15) / 16) * 16;
    c->in_bytes = c->in_nlines + sizeof(int) * E;
    ALLOC(c->d_in, c->in_bytes);
    c->d_enc = reinterpret_cast<double*>(c->d_in);
    c->d_lines = reinterpret_cast<ekf_line*>(c->d_in + c->in_lines);
    c->d_nlines = reinterpret_cast<int*>(c->d_in + c->in_nlines);
    ALLOC(c->pexp, sizeof(int) * E);
    ALLOC(c->sink, 8 * ekf::TILE_ELEMS);
    c->pexp_h.assign(E, 0);
    // whole 128-B lines: the package words, then 16 words for the speculative list words
    c->mbw = ((ekf::MB_WORDS_FIXED + 4 * d.max_lines + 15) / 16) * 16 + 16;
    // options (ekf_set_option): defaults, nothing from the environment
    c->spec = 1;
    c->spin_log2 = 24;
    c->test_drop = 0;
    c->test_verdict = 0;
    c->mfrep_opt = 1;
    c->active_flush = 1;
    c->mfrep = c->bf ? 1 : 0;
    ALLOC(c->mbox, sizeof(double) * 2 * c->Gmax * c->mbw * E);
    return EKF_OK;
}

// the partitioned instance's scan state (replicated on every rank) and a step that applies
// nothing (rolled back: every flush form skips it), which pads an odd partial group
static int make_shard_buffers(ekf_ctx* c)
{
    if (c->sh_world <= 0) return EKF_OK;
    const Dims& d = c->d;
    ALLOC(c->sh_rob, sizeof(double) * 12);
    ALLOC(c->sh_rec, sizeof(double) * d.N * ekf::SH_REC);
    ALLOC(c->sh_hist, sizeof(double) * d.N * d.max_lines * 8);
    ALLOC(c->sh_pkg, sizeof(double) * (ekf::MB_WORDS_FIXED + 4 * d.max_lines));
    ALLOC(c->sh_flags, sizeof(int) * d.N);
    ALLOC(c->sh_ctl, sizeof(int) * ekf::SC_WORDS);
    ALLOC(c->sh_null.res, sizeof(int) * ekf::RES_STRIDE);
    const int one = 1;
    if (hipMemcpy(c->sh_null.res + ekf::RES_ROLLBACK, &one, sizeof(int), hipMemcpyHostToDevice) != hipSuccess)
        return EKF_ENOMEM;
    c->sh_null.Uop = c->ring[0].Uop;
    c->sh_null.Vop = c->ring[0].Vop;
    c->sh_null.patch = c->ring[0].patch;
    c->sh_null.patch_diag = c->ring[0].patch_diag;
    return EKF_OK;
}

// what the results are read from: the workgroups' completion words, the pinned records and the
// synchronous calls' mirror with their device pointers; and the pinned input staging
static int make_host_buffers(ekf_ctx* c)
{
    const int E = c->cfg.instances;
    c->sync_stride = ((ekf::SYNC_WG0 + c->Gmax + 15) / 16) * 16;
    ALLOC(c->sync, sizeof(int) * c->sync_stride * E);
    if (!pinned_alloc(c, (void**)&c->h_res, sizeof(int) * ekf::RES_STRIDE * E) ||
        !pinned_alloc(c, (void**)&c->h_pose, sizeof(double) * 3 * E) ||
        !pinned_alloc(c, (void**)&c->h_r33, sizeof(double) * 9 * E) ||
        !pinned_alloc(c, (void**)&c->h_ep, sizeof(unsigned) * E) ||
        !pinned_alloc(c, (void**)&c->h_in, c->in_bytes) ||
        hipEventCreateWithFlags(&c->ev_in, hipEventDisableTiming) != hipSuccess ||
        hipHostGetDevicePointer((void**)&c->hd_res, c->h_res, 0) != hipSuccess ||
        hipHostGetDevicePointer((void**)&c->hd_pose, c->h_pose, 0) != hipSuccess ||
        hipHostGetDevicePointer((void**)&c->hd_r33, c->h_r33, 0) != hipSuccess ||
        hipHostGetDevicePointer((void**)&c->hd_ep, c->h_ep, 0) != hipSuccess)
        return EKF_ENOMEM;
    memset(c->h_ep, 0, sizeof(unsigned) * E);
    return EKF_OK;
}
#undef ALLOC

static int make_streams(ekf_ctx* c)
{
    if (hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&c->dstream, hipStreamNonBlocking) != hipSuccess)
        return EKF_EDEVICE;
    c->stream = c->own_stream;
    if (hipEventCreateWithFlags(&c->ev_scan, hipEventDisableTiming) != hipSuccess) return EKF_EDEVICE;
    for (int k = 0; k < 2; k++)
        if (hipEventCreateWithFlags(&c->ev_flush[k], hipEventDisableTiming) != hipSuccess) return EKF_EDEVICE;
    return EKF_OK;
}

// the flush grid and how many instances one association launch takes
static int size_launches(ekf_ctx* c)
{
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, c->device) != hipSuccess) return EKF_EDEVICE;
    c->dd_per_cu = 8;   // downdate workgroups per CU (4 waves each; EKF_OPT_FLUSH_BLOCKS_PER_CU)
    c->dd_grid = prop.multiProcessorCount * c->dd_per_cu;
    c->ncu = prop.multiProcessorCount;
    // automatic flush form (EKF_OPT_FLUSH_FORM); a partitioned instance: the wave form for every
    // group (its wave tables hold the rank's tile rows only; the other forms walk every tile)
    c->dd_variant = c->sh_world > 0 ? ekf::FORM_WAVE : ekf::FORM_AUTO;
    // all G workgroups of an instance must be co-resident (they exchange per line). A plain
    // launch gets the same residency as a cooperative one for the same grid
    // (cdna_hip_programming.md §1; the cooperative form only adds a launch-time check of the
    // same occupancy query, which can over-report, for ≈17 µs per launch), so the grid is
    // sized from a bound that cannot over-report: the LDS the kernel declares (one block per
    // CU at 128 KB of 160 KB), capped by the occupancy query less one block of margin when
    // the query allows more than one.
    int per_cu = ekf::scan_blocks_per_cu(c->cfg.precision);
    if (per_cu > 1) per_cu -= 1;
    const size_t lds = ekf::scan_lds_bytes(c->cfg.precision);
    if (lds > 0 && prop.maxSharedMemoryPerMultiProcessor > 0) {
        const int by_lds = (int)(prop.maxSharedMemoryPerMultiProcessor / lds);
        if (by_lds < per_cu) per_cu = by_lds;
    }
    if (per_cu < 1) return EKF_EINVAL;
    c->resident = prop.multiProcessorCount * per_cu;
    c->scan_batch = c->resident / c->G;
    if (c->scan_batch < 1) return EKF_EINVAL;   // one instance does not fit the device
    if (c->scan_batch > c->cfg.instances) c->scan_batch = c->cfg.instances;
    return EKF_OK;
}

static int create_ctx(const ekf_config* cfg, int sh_rank, int sh_world, ekf_ctx** out)
{
    if (!cfg || !out) return EKF_EINVAL;
    *out = nullptr;
    int device = 0;
    int rc = validate(cfg, &device);
    if (rc) return rc;
    ekf_ctx* c = new (std::nothrow) ekf_ctx();   // (zeroed: the steps set what is not zero or null)
    if (!c) return EKF_ENOMEM;
    c->cfg = *cfg;
    c->device = device;
    static int (*const steps[])(ekf_ctx*) = {make_state, make_ring, make_tables, make_scan_buffers,
                                             make_shard_buffers, make_host_buffers, make_streams, size_launches};
    rc = set_dims(c, sh_rank, sh_world);
    for (auto step : steps)
        if (!rc) rc = step(c);
    for (int e = 0; !rc && e < cfg->instances; e++) rc = set_robot_ctor(c, e, 0.0, 0.0, 0.0);
    if (rc) {
        free_all(c);
        delete c;
        return rc;
    }
    *out = c;
    return EKF_OK;
}

extern "C" int ekf_create(const ekf_config* cfg, ekf_ctx** out)
{
    return create_ctx(cfg, -1, 0, out);
}

extern "C" int ekf_shard_create(const ekf_config* cfg, int rank, int world, ekf_ctx** out)
{
    if (!cfg || !out) return EKF_EINVAL;
    *out = nullptr;
    // one instance, the exact arithmetic, fp32 or fp64 storage, the sequential schedule, groups the
    // wave flushes take (fp32 <= 8 steps, fp64 <= 8)
    if (world < 1 || rank < 0 || rank >= world || cfg->instances != 1 || cfg->pipeline ||
        cfg->arith != EKF_ARITH_EXACT || (cfg->precision != EKF_PREC_F32 && cfg->precision != EKF_PREC_F64) ||
        cfg->flush_interval > (cfg->precision == EKF_PREC_F64 ? ekf::F64_WAVE_MAXS : 8) ||
        cfg->max_lines > ekf::SH_MAX_LINES)
        return EKF_EINVAL;
    return create_ctx(cfg, rank, world, out);
}

extern "C" int ekf_destroy(ekf_ctx* c)
{
    if (!c) return EKF_EINVAL;
    (void)hipStreamSynchronize(c->stream);
    (void)hipStreamSynchronize(c->dstream);
    rccl_destroy(c);
    free_all(c);
    delete c;
    return EKF_OK;
}

extern "C" int ekf_set_stream(ekf_ctx* c, void* s)
{
    if (!c) return EKF_EINVAL;
    int rc = drain(c);
    if (rc) return rc;
    c->stream = s ? (hipStream_t)s : c->own_stream;
    return EKF_OK;
}

extern "C" int ekf_sync(ekf_ctx* c)
{
    if (!c) return EKF_EINVAL;
    return drain(c);
}

extern "C" int ekf_set_option(ekf_ctx* c, int opt, int v)
{
    if (!c) return EKF_EINVAL;
    const int E = c->cfg.instances;
    switch (opt) {
    case EKF_OPT_SPECULATE: if (v < 0 || v > 3) return EKF_ERANGE; break;
    case EKF_OPT_SPIN_LOG2: if (v < 8 || v > 24) return EKF_ERANGE; break;
    case EKF_OPT_FLUSH_FORM:
        if (!ekf::flush_form_valid(v)) return EKF_ERANGE;
        // a partitioned context stores only its tile rows; only the wave forms walk the rank's
        // wave tables (the super-tile and tile forms walk every tile of the block)
        if (c->sh_world > 0 && v != ekf::FORM_WAVE) return EKF_EINVAL;
        break;
    case EKF_OPT_FLUSH_BLOCKS_PER_CU: if (v < 1 || v > 16) return EKF_ERANGE; break;
    case EKF_OPT_MFMA_REPLAY: if (v < 0 || v > 2) return EKF_ERANGE; break;
    case EKF_OPT_ACTIVE_FLUSH:
    case EKF_OPT_SCAN_STAMPS: if (v < 0 || v > 1) return EKF_ERANGE; break;
    case EKF_OPT_SCAN_THREADS: if (v != 0 && v != 64 && v != 128 && v != 192) return EKF_ERANGE; break;
    case EKF_OPT_TEST_DROP_WG:
    case EKF_OPT_TEST_VERDICT_TIMEOUT: if (v < 0 || v > E) return EKF_ERANGE; break;
    default: return EKF_EINVAL;
    }
    int rc = drain(c);
    if (rc) return rc;
    switch (opt) {
    case EKF_OPT_SPECULATE: c->spec = v; break;
    case EKF_OPT_SPIN_LOG2: c->spin_log2 = v; break;
    case EKF_OPT_FLUSH_FORM: c->dd_variant = v; break;
    case EKF_OPT_FLUSH_BLOCKS_PER_CU:
        c->dd_per_cu = v;
        c->dd_grid = c->ncu * v;
        break;
    case EKF_OPT_MFMA_REPLAY:
        c->mfrep_opt = v;
        c->mfrep = c->bf ? v : 0;
        break;
    case EKF_OPT_SCAN_STAMPS:
        if (v && !c->dbg) {
            const size_t bytes = sizeof(unsigned long long) * 32 * E;
            if (hipMalloc((void**)&c->dbg, bytes) != hipSuccess) {
                c->dbg = nullptr;
                return EKF_ENOMEM;
            }
            HIP_TRY(hipMemset(c->dbg, 0, bytes));
        } else if (!v && c->dbg) {
            HIP_TRY(hipFree(c->dbg));
            c->dbg = nullptr;
        }
        break;
    case EKF_OPT_TEST_DROP_WG: c->test_drop = v; break;
    case EKF_OPT_TEST_VERDICT_TIMEOUT: c->test_verdict = v; break;
    case EKF_OPT_ACTIVE_FLUSH: c->active_flush = v; break;
    case EKF_OPT_SCAN_THREADS: c->nt_opt = v; break;
    }
    return EKF_OK;
}

extern "C" int ekf_get_option(const ekf_ctx* c, int opt, int* v)
{
    if (!c || !v) return EKF_EINVAL;
    switch (opt) {
    case EKF_OPT_SPECULATE: *v = c->spec; break;
    case EKF_OPT_SPIN_LOG2: *v = c->spin_log2; break;
    case EKF_OPT_FLUSH_FORM: *v = c->dd_variant; break;
    case EKF_OPT_FLUSH_BLOCKS_PER_CU: *v = c->dd_per_cu; break;
    case EKF_OPT_MFMA_REPLAY: *v = c->mfrep_opt; break;
    case EKF_OPT_SCAN_STAMPS: *v = c->dbg ? 1 : 0; break;
    case EKF_OPT_TEST_DROP_WG: *v = c->test_drop; break;
    case EKF_OPT_TEST_VERDICT_TIMEOUT: *v = c->test_verdict; break;
    case EKF_OPT_ACTIVE_FLUSH: *v = c->active_flush; break;
    case EKF_OPT_SCAN_THREADS: *v = c->nt_opt; break;
    default: return EKF_EINVAL;
    }
    return EKF_OK;
}

// profiling level 1 times the flush only (what the roofline needs, 2 events per group);
// level 2 also every association kernel. record = false: the caller hands the pair to the launch
// (hipExtLaunchKernelGGL timestamps the dispatch itself; no marker packets around the flush)
static EvPair* prof_begin(ekf_ctx* c, int kind, hipStream_t st, bool record = true)
{
    if (!c->prof || (kind == 0 && c->prof < 2)) return nullptr;
    EvPair pr;
    if (!c->pool.empty()) {
        pr = c->pool.back();
        c->pool.pop_back();
    } else {
        if (hipEventCreate(&pr.a) != hipSuccess) return nullptr;
        if (hipEventCreate(&pr.b) != hipSuccess) return nullptr;
    }
    c->ev[kind].push_back(pr);
    if (record) (void)hipEventRecord(pr.a, st);
    return &c->ev[kind].back();
}

static void prof_end(ekf_ctx* c, EvPair* pr, hipStream_t st)
{
    if (pr) (void)hipEventRecord(pr->b, st);
}

// Landmarks per association workgroup (EKF_OPT_SCAN_THREADS): the narrow widths exist for the
// HOT instantiations of the kernel only (symmetric fp32 / fp16 operands, kmax = 16, every flush
// arithmetic; launch_scan) and need the instance's workgroups
// within the speculative path's bound, no pipelined overlap and every instance in one launch.
// Automatic: the narrowest of 64 and 128 that fits (measured, DESIGN §4.1: N = 256 / 1024 / 2048
// +8 / +9 / +5 % updates/s at 64, N = 4096 with 8 instances +1.4 % at 128).
// Symmetric fp32 operands (sym_factor: every EKF_R_INTENDED fp32 / fp16 context; U = −2^x·V
// exactly): the association kernel stores the V rows only and every reader of U rows scales them
// (ScanParams / DowndateParams::usym). The partitioned instance stores both.
int usym_of(const ekf_ctx* c)
{
    return c->sh_world == 0 && c->cfg.precision != EKF_PREC_F64 && c->cfg.r_mode == EKF_R_INTENDED;
}

static int scan_width(const ekf_ctx* c)
{
    constexpr int W = ekf::SCAN_THREADS;
    if (c->dbg || c->sh_world > 0 || c->cfg.precision == EKF_PREC_F64 || c->cfg.r_mode != EKF_R_INTENDED ||
        c->d.kmax != 16)
        return W;
    auto fits = [&](int nt) {
        const int G = (c->d.N + nt - 1) / nt;
        return G <= ekf::SPEC_GMAX && !(G > 1 && c->cfg.pipeline) && G * c->cfg.instances <= c->resident;
    };
    if (c->nt_opt) return c->nt_opt != W && fits(c->nt_opt) ? c->nt_opt : W;
    return fits(64) ? 64 : fits(128) ? 128 : W;
}

static ekf::ScanParams scan_params(ekf_ctx* c, int phase, const double* enc,
                                   const ekf_line* lines, const int* nlines)
{
    ekf::ScanParams p;
    memset(&p, 0, sizeof(p));
    p.d = c->d;
    p.E = c->cfg.instances;
    p.phase = phase;
    p.r_mode = c->cfg.r_mode;
    p.reset_margin = c->cfg.reset_margin;
    p.gate = c->cfg.mahalanobis;
    p.enc_noise = c->cfg.encoder_noise;
    p.Rs = c->Rs;
    p.y = c->y;
    p.live = c->cur;
    p.Dd = c->D;
    p.mfrep = c->mfrep;
    p.mfrep64 = (c->cfg.precision == EKF_PREC_F64 && c->mfrep_opt) ? 1 : 0;
    p.bf = c->pmode;
    p.psig = c->psig;
    p.pvmax = c->pvmax;
    p.Etot = c->cfg.instances;
    p.spin_log2 = c->spin_log2;
    p.test_drop = c->test_drop;
    p.test_verdict = c->test_verdict;
    p.pose = c->pose;
    p.xpre = c->xpre;
    p.saved = c->saved;
    p.enc = enc;
    p.lines = lines;
    p.nlines = nlines;
    p.dbg = c->dbg;
    p.pexp = c->pexp;
    p.nt = scan_width(c);
    p.usym = usym_of(c);
    p.G = (c->d.N + p.nt - 1) / p.nt;
    c->last_G = p.G;
    p.mbw = c->mbw;
    p.spec = c->spec;
    p.mbox = c->mbox;
    p.sync = c->sync;
    p.sync_stride = c->sync_stride;
    if (c->mirror_on) {
        p.res_host = c->hd_res;
        p.pose_host = c->hd_pose;
        p.r33_host = c->hd_r33;
        p.ep_host = c->hd_ep;
    }
    return p;
}

// The association kernel in batches of co-resident instances: grid (G, batch). Its per-line
// exchange counters are zeroed on the stream first.
static hipError_t launch_scans(ekf_ctx* c, ekf::ScanParams sp)
{
    const int E = c->cfg.instances;
    sp.epoch = ++c->scan_epoch;
    hipError_t err = hipSuccess;
    // (scan_width keeps a narrow launch within one batch)
    const int batch = sp.nt == ekf::SCAN_THREADS ? c->scan_batch : E;
    for (int e0 = 0; err == hipSuccess && e0 < E; e0 += batch) {
        sp.e0 = e0;
        sp.E = (E - e0 < batch) ? E - e0 : batch;
        err = ekf::launch_scan(sp, c->cfg.precision, c->stream);
    }
    return err;
}

const ekf::Slot& slot_of(const ekf_ctx* c, long long k)
{
    return c->ring[(size_t)(k % (long long)c->ring.size())];
}

// The kernel that flushes a group of nsteps steps of this context (ekf_flush_plan.h)
static ekf::FlushPlan flush_plan_of(const ekf_ctx* c, int nsteps)
{
    return ekf::flush_plan(ekf::FlushKey{c->cfg.precision, c->pmode, c->dd_variant, nsteps, c->d.kmax, c->sh_world > 0,
                                         c->nwt > 0, c->nwt64 > 0, c->nwt24 > 0, c->nwtq > 0});
}

// One pass over the landmark block applying steps [unflushed0, nsteps) (stream D).
int enqueue_flush(ekf_ctx* c)
{
    const int nst = (int)(c->nsteps - c->unflushed0);
    if (nst <= 0) return EKF_OK;
    const ekf::FlushPlan plan = flush_plan_of(c, nst);
    // sequential schedule: the flush follows the scans on S (no cross-stream events); pipelined:
    // on D after the group's last scan
    hipStream_t fs = c->cfg.pipeline ? c->dstream : c->stream;
    if (c->cfg.pipeline) HIP_TRY(hipStreamWaitEvent(c->dstream, c->ev_scan, 0));
    ekf::DowndateParams dp;
    memset(&dp, 0, sizeof(dp));
    dp.d = c->d;
    dp.E = c->cfg.instances;
    dp.nsteps = plan.nsteps;
    dp.variant = c->dd_variant;
    dp.ncu = c->ncu;
    dp.tile_rc = c->tile_rc;
    dp.stile_rc = c->stile_rc;
    dp.stile2_rc = c->stile2_rc;
    dp.nstiles2 = c->nstiles2;
    dp.wt = c->wt;
    dp.nwt = c->nwt;
    dp.wt64 = c->wt64;
    dp.nwt64 = c->nwt64;
    dp.wt24 = c->wt24;
    dp.nwt24 = c->nwt24;
    dp.wtq = c->wtq;
    dp.nwtq = c->nwtq;
    dp.pexp = c->pexp;
    dp.usym = usym_of(c);
    dp.sink = c->sink;
    dp.ubase = c->ops_u;
    dp.vbase = c->ops_v;
    dp.slot_bytes = c->slot_bytes;
    dp.nslots = (int)c->ring.size();
    dp.slot0 = (int)(c->unflushed0 % (long long)c->ring.size());
    dp.dbg = c->dbg;
    dp.bf = c->pmode;
    dp.bbase = c->ops_b;
    dp.bslot_bytes = c->bslot_bytes;
    for (int q = 0; q < nst; q++) dp.steps[q] = slot_of(c, c->unflushed0 + q);
    for (int q = nst; q < plan.nsteps; q++) dp.steps[q] = c->sh_null;   // (the plan's padding step)
    const int in = c->last_out;
    const int out = c->cfg.pipeline ? 1 - in : in;
    dp.Pin = xview(c, in);
    dp.Pout = xview(c, out);
    // the association kernel's RES_ZMAX bound (partitioned contexts write other records). A
    // skipped wave-tile is neither loaded nor stored, so it stays valid only in place: a
    // double-buffered (pipelined) flush would leave X[out]'s copy from two flushes earlier
    dp.zskip = (c->active_flush && c->sh_world == 0 && in == out) ? 1 : 0;
    EvPair* pr = prof_begin(c, 1, fs, false);
    if (pr) c->ev_nsteps.push_back(nst);
    HIP_TRY(ekf::launch_downdate(dp, plan, c->dd_grid, fs, pr ? pr->a : nullptr,
                                 pr ? pr->b : nullptr));
    hipEvent_t ev = c->ev_flush[c->nflush & 1];
    if (c->cfg.pipeline) HIP_TRY(hipEventRecord(ev, fs));
    if (c->cfg.pipeline) {
        // next scans read X[in] (= output of the previous flush) with both groups pending
        c->base = in;
        c->ev_base = c->nflush > 0 ? c->ev_flush[(c->nflush - 1) & 1] : nullptr;
        c->pend0 = c->unflushed0;
    } else {
        c->base = in;
        c->ev_base = nullptr;   // same stream
        c->pend0 = c->nsteps;
    }
    c->last_out = out;
    c->unflushed0 = c->nsteps;
    c->nflush++;
    return EKF_OK;
}

// Enqueue one localize step (or its predict / update half).
static int enqueue(ekf_ctx* c, int phase, const double* enc, const ekf_line* lines,
                   const int* nlines)
{
    // a row-sharded context keeps only its own rows current: the whole-instance scan would read
    // stale ones (slam_ekf.h ekf_shard_abort)
    if (c->sh_world > 0) return EKF_EINVAL;
    ekf::ScanParams sp = scan_params(c, phase, enc, lines, nlines);
    if (!(phase & ekf::PHASE_UPDATE)) {
        EvPair* pr = prof_begin(c, 0, c->stream);
        HIP_TRY(launch_scans(c, sp));
        prof_end(c, pr, c->stream);
        c->predicted = 1;
        return EKF_OK;
    }
    c->predicted = 0;
    // X[base] and the ring slot this step reuses are released by the event guarding base
    if (c->ev_base) HIP_TRY(hipStreamWaitEvent(c->stream, c->ev_base, 0));
    const int np = (int)(c->nsteps - c->pend0);
    if (np > ekf::PMAX) return EKF_EINVAL;   // unreachable: T <= 24
    sp.Pread = xview(c, c->base);
    sp.npend = np;
    for (int q = 0; q < np; q++) sp.pend[q] = slot_of(c, c->pend0 + q);
    sp.cur = slot_of(c, c->nsteps);
    sp.Ust = c->Ust;
    sp.Vst = c->Vst;
    EvPair* pr = prof_begin(c, 0, c->stream);
    HIP_TRY(launch_scans(c, sp));
    prof_end(c, pr, c->stream);
    if (c->cfg.pipeline || c->mirror_on) HIP_TRY(hipEventRecord(c->ev_scan, c->stream));
    c->nsteps++;
    if (c->nsteps - c->unflushed0 >= c->T) return enqueue_flush(c);
    return EKF_OK;
}

static int stage_inputs(ekf_ctx* c, const double* enc, const ekf_line* lines, const int* nlines)
{
    const int E = c->cfg.instances;
    if (nlines)
        for (int e = 0; e < E; e++)
            if (nlines[e] < 0 || nlines[e] > c->d.max_lines) return EKF_ERANGE;
    // into the pinned staging buffer (once the previous copy out of it has been done), then one
    // stream-ordered copy of the sections given: the device buffers are rewritten after the
    // association kernels that read them
    if (c->in_pending) HIP_TRY(hipEventSynchronize(c->ev_in));
    size_t lo = c->in_bytes, hi = 0;
    if (enc) {
        memcpy(c->h_in, enc, sizeof(double) * 3 * E);
        lo = 0;
        hi = sizeof(double) * 3 * E;
    }
    if (lines) {
        memcpy(c->h_in + c->in_lines, lines, sizeof(ekf_line) * c->d.max_lines * E);
        lo = std::min(lo, c->in_lines);
        hi = c->in_nlines;
    }
    if (nlines) {
        memcpy(c->h_in + c->in_nlines, nlines, sizeof(int) * E);
        lo = std::min(lo, c->in_nlines);
        hi = c->in_bytes;
    }
    if (hi > lo) {
        HIP_TRY(hipMemcpyAsync(c->d_in + lo, c->h_in + lo, hi - lo, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipEventRecord(c->ev_in, c->stream));
        c->in_pending = 1;
    }
    return EKF_OK;
}

extern "C" int ekf_read_results(ekf_ctx* c, ekf_result* out)
{
    if (!c) return EKF_EINVAL;
    const int E = c->cfg.instances;
    if (c->nsteps == 0) {
        if (out) memset(out, 0, sizeof(ekf_result) * E);
        return EKF_OK;
    }
    HIP_TRY(hipMemcpyAsync(c->h_res, slot_of(c, c->nsteps - 1).res, sizeof(int) * ekf::RES_STRIDE * E,
                           hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(c->h_pose, c->pose, sizeof(double) * 3 * E, hipMemcpyDeviceToHost,
                           c->stream));
    std::vector<int> hs((size_t)c->sync_stride * E);
    HIP_TRY(hipMemcpyAsync(hs.data(), c->sync, sizeof(int) * hs.size(), hipMemcpyDeviceToHost,
                           c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    // every workgroup's completion word of the last association launch (commit_fold: a word of
    // another launch — a workgroup that never ran or never finished — reads as a timeout, not as
    // the status bits an earlier launch left in it). A partitioned context never launches the
    // association kernel (scan_epoch counts its shard runs, which write no completion words): its
    // status bits are already in the record SH_END wrote
    if (c->scan_epoch > 0 && c->sh_world <= 0)
        for (int e = 0; e < E; e++) {
            int st = 0;
            for (int gq = 0; gq < c->last_G; gq++)
                st = ekf::commit_fold(st, (unsigned)hs[(size_t)e * c->sync_stride + ekf::SYNC_WG0 + gq],
                                      c->scan_epoch);
            c->h_res[(size_t)e * ekf::RES_STRIDE + ekf::RES_STATUS] |= st & ekf::DONE_STATUS_MASK;
        }
    fill_results(c, out);
    return EKF_OK;
}

// ekf_result of every instance from the host copies of the last step's records and poses
void fill_results(const ekf_ctx* c, ekf_result* out)
{
    const int E = c->cfg.instances;
    if (!out) return;
    for (int e = 0; e < E; e++) {
        const int* r = c->h_res + (size_t)e * ekf::RES_STRIDE;
        ekf_result& o = out[e];
        memset(&o, 0, sizeof(o));
        o.pose[0] = c->h_pose[3 * e];
        o.pose[1] = c->h_pose[3 * e + 1];
        o.pose[2] = c->h_pose[3 * e + 2];
        o.matches = r[ekf::RES_M];
        o.new_landmarks = r[ekf::RES_NEXTRA];
        o.saved = r[ekf::RES_SAVED];
        o.reset = r[ekf::RES_RESET];
        o.status = r[ekf::RES_STATUS];
        o.nlines = r[ekf::RES_NLINES];
        for (int i = 0; i < EKF_MAX_LINES; i++)
            o.match[i] = (i < o.nlines) ? r[ekf::RES_MATCH + i] : -1;
    }
}

// A synchronous call's update: the scan's lead mirrors a committed result into pinned host memory
// (ScanParams::res_host), so the call waits for the association kernel only (not for a flush queued
// behind it) and reads the result without a copy; the robot blocks it mirrored serve
// ekf_get_pose_cov until the next launch. Any instance without this launch's epoch in its mirror
// (a rollback, a lead that never finished) takes the copies and the host fold of ekf_read_results.
static int enqueue_mirrored(ekf_ctx* c, int phase, ekf_result* out)
{
    c->mirror_on = 1;
    const int rc = enqueue(c, phase, c->d_enc, c->d_lines, c->d_nlines);
    c->mirror_on = 0;
    if (rc) return rc;
    c->mirror_epoch = 0;
    HIP_TRY(hipEventSynchronize(c->ev_scan));
    const int E = c->cfg.instances;
    bool all = true;
    for (int e = 0; e < E; e++) all = all && __atomic_load_n(c->h_ep + e, __ATOMIC_ACQUIRE) == c->scan_epoch;
    if (!all) return ekf_read_results(c, out);
    c->mirror_epoch = c->scan_epoch;
    fill_results(c, out);
    return EKF_OK;
}

extern "C" int ekf_localize(ekf_ctx* c, const double* enc, const ekf_line* lines,
                            const int32_t* nlines, ekf_result* out)
{
    if (!c || !enc || !lines || !nlines || c->sh_world > 0) return EKF_EINVAL;
    int rc = stage_inputs(c, enc, lines, nlines);
    if (rc) return rc;
    return enqueue_mirrored(c, ekf::PHASE_BOTH, out);
}

extern "C" int ekf_localize_device(ekf_ctx* c, const double* d_enc, const ekf_line* d_lines,
                                   const int32_t* d_nlines)
{
    if (!c || !d_enc || !d_lines || !d_nlines) return EKF_EINVAL;
    return enqueue(c, ekf::PHASE_BOTH, d_enc, d_lines, d_nlines);
}

extern "C" int ekf_predict(ekf_ctx* c, const double* enc)
{
    if (!c || !enc || c->sh_world > 0) return EKF_EINVAL;
    int rc = stage_inputs(c, enc, nullptr, nullptr);
    if (rc) return rc;
    return enqueue(c, ekf::PHASE_PREDICT, c->d_enc, c->d_lines, c->d_nlines);
}

extern "C" int ekf_update(ekf_ctx* c, const ekf_line* lines, const int32_t* nlines,
                          ekf_result* out)
{
    if (!c || !lines || !nlines || c->sh_world > 0) return EKF_EINVAL;
    int rc = stage_inputs(c, nullptr, lines, nlines);
    if (rc) return rc;
    return enqueue_mirrored(c, ekf::PHASE_UPDATE, out);
}

extern "C" int ekf_profile_enable(ekf_ctx* c, int enable)
{
    if (!c) return EKF_EINVAL;
    (void)hipStreamSynchronize(c->stream);
    (void)hipStreamSynchronize(c->dstream);
    for (auto& v : c->ev) {
        for (auto& pr : v) c->pool.push_back(pr);
        v.clear();
    }
    c->ev_nsteps.clear();
    c->prof = enable < 0 ? 0 : (enable > 2 ? 2 : enable);
    return EKF_OK;
}

extern "C" int ekf_profile_read(ekf_ctx* c, double* scan_ms, double* dd_ms, double* aug_ms,
                                int* launches)
{
    if (!c) return EKF_EINVAL;
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipStreamSynchronize(c->dstream));
    double avg[3] = {0, 0, 0};
    for (int k = 0; k < 3; k++) {
        double sum = 0;
        for (auto& pr : c->ev[k]) {
            float ms = 0;
            HIP_TRY(hipEventElapsedTime(&ms, pr.a, pr.b));
            sum += ms;
        }
        avg[k] = c->ev[k].empty() ? 0.0 : sum / (double)c->ev[k].size();
    }
    if (scan_ms) *scan_ms = avg[0];
    if (dd_ms) *dd_ms = avg[1];
    if (aug_ms) *aug_ms = avg[2];
    if (launches) *launches = (int)c->ev[1].size();
    return EKF_OK;
}

extern "C" int ekf_profile_flushes(ekf_ctx* c, int cap, int* nsteps, float* ms)
{
    if (!c || cap < 0 || (cap > 0 && (!nsteps || !ms))) return -EKF_EINVAL;
    if (hipStreamSynchronize(c->stream) != hipSuccess || hipStreamSynchronize(c->dstream) != hipSuccess)
        return -EKF_EDEVICE;
    const int n = (int)c->ev[1].size();
    for (int k = 0; k < n && k < cap; k++) {
        float t = 0.f;
        if (hipEventElapsedTime(&t, c->ev[1][k].a, c->ev[1][k].b) != hipSuccess) return -EKF_EDEVICE;
        ms[k] = t;
        nsteps[k] = k < (int)c->ev_nsteps.size() ? c->ev_nsteps[k] : 0;
    }
    return n;
}

extern "C" const char* ekf_flush_kernel_name(const ekf_ctx* c, int nsteps)
{
    if (!c || nsteps < 1) return "";
    // every name flush_plan_name can give, formatted once (the strings outlive the call)
    constexpr int MAXS = ekf::F16X3_MAXS;   // (the largest step count a name carries)
    struct Names {
        char n[ekf::FLUSH_FAMILIES][2][MAXS + 1][64];
        Names()
        {
            for (int f = 0; f < ekf::FLUSH_FAMILIES; f++)
                for (int h = 0; h < 2; h++)
                    for (int k = 0; k <= MAXS; k++)
                        ekf::flush_plan_name(ekf::FlushPlan{(ekf::FlushFamily)f, k, h ? EKF_PREC_F16 : EKF_PREC_F32,
                                                            ekf::GRID_STRIDED}, n[f][h][k], sizeof n[f][h][k]);
        }
    };
    static const Names names;   // (initialised once, thread-safe)
    const ekf::FlushPlan plan = flush_plan_of(c, nsteps);
    return names.n[plan.family][plan.storage == EKF_PREC_F16][std::min(plan.nsteps, MAXS)];
}

extern "C" int ekf_debug_result_words(ekf_ctx* c, int e, int out[16])
{
    // Diagnostic: the first 16 words of instance e's last result record (as copied by the last
    // ekf_read_results), including the association path code and guessed winners (RES_DBG).
    if (!c || !out || e < 0 || e >= c->cfg.instances) return EKF_EINVAL;
    memcpy(out, c->h_res + (size_t)e * ekf::RES_STRIDE, sizeof(int) * 16);
    return EKF_OK;
}

extern "C" int ekf_debug_scan_stamps(ekf_ctx* c, unsigned long long out[32])
{
    // Diagnostic: association-kernel phase times summed over instances (100 MHz ticks) since
    // context creation, when built with EKF_SCAN_STAMPS=1 in the environment; zeros otherwise.
    if (!c || !out) return EKF_EINVAL;
    memset(out, 0, sizeof(unsigned long long) * 32);
    if (!c->dbg) return EKF_OK;
    HIP_TRY(hipStreamSynchronize(c->stream));
    std::vector<unsigned long long> h((size_t)32 * c->cfg.instances);
    HIP_TRY(hipMemcpy(h.data(), c->dbg, sizeof(unsigned long long) * h.size(), hipMemcpyDeviceToHost));
    for (int e = 0; e < c->cfg.instances; e++)
        for (int k = 0; k < 32; k++) out[k] += h[(size_t)e * 32 + k];
    return EKF_OK;
}
