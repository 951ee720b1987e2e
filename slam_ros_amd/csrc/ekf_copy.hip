// ekf_copy.hip — the calls that copy instances without draining the flush (slam_ekf.h): ekf_resample and
// ekf_copy_instance (table: ekf_resample_plan.h; kernel: unit_resample.hip), ekf_resample_device (the same
// arrays as pieces; kernels: unit_resample_device.hip) with ekf_resample_plan_device, which writes its
// list (ekf_loop_plan.h; kernel: unit_loop.hip), and the instance images,
// ekf_export_instances* / ekf_import_instances* (table: ekf_image_plan.h; kernel of the device forms:
// unit_image.hip).
#include <stdint.h>

#include "ekf_ctx.h"
#include "ekf_resample_plan.h"
#include "ekf_image_plan.h"

// ---- ekf_resample ----
// Every per-instance slice the kernels read later goes from instance src[e] to instance e in one
// launch on S (the table: ekf_resample_plan.h). Nothing of the schedule changes: no flush, no step,
// no epoch, and not a byte of an instance that keeps its state.
static ekf::ResampleLayout resample_layout(const ekf_ctx* c)
{
    ekf::ResampleLayout L;
    auto addr = [](const void* p) { return (uint64_t)(uintptr_t)p; };
    L.d = c->d;
    L.E = c->cfg.instances;
    L.xinst_bytes = (uint64_t)c->xinst * c->elem;
    L.op_elem = (int)c->op_elem;
    L.usym = usym_of(c);
    L.npl = c->pmode == EKF_ARITH_F16X3 ? 2 : c->pmode == EKF_ARITH_BF16X6 ? 3 : 0;
    L.res_stride = ekf::RES_STRIDE;
    L.sync_stride = c->sync_stride;
    // pipelined: X[in] (the scans' base) and X[out] (the newest flush's output, the next one's input)
    L.nX = c->cfg.pipeline ? 2 : 1;
    L.X[0] = addr(c->X[0]);
    L.X[1] = addr(c->X[1]);
    L.Rs = addr(c->Rs);
    L.y = addr(c->y);
    L.D = addr(c->D);
    L.cur = addr(c->cur);
    L.saved = addr(c->saved);
    L.pexp = addr(c->pexp);
    L.psig = addr(c->psig);
    L.pose = addr(c->pose);
    L.xpre = addr(c->xpre);
    L.pvmax = addr(c->pvmax);
    L.sync = addr(c->sync);
    L.ops_u = addr(c->ops_u);
    L.ops_v = addr(c->ops_v);
    L.ops_b = addr(c->ops_b);
    L.slot_bytes = (uint64_t)c->slot_bytes;
    L.bslot_bytes = (uint64_t)c->bslot_bytes;
    for (const ekf::Slot& sl : c->ring) {
        L.patch.push_back(addr(sl.patch));
        L.patch_diag.push_back(addr(sl.patch_diag));
        L.res.push_back(addr(sl.res));
    }
    const long long R = (long long)c->ring.size();
    for (long long k = c->pend0; k < c->nsteps; k++) L.pending.push_back((int)(k % R));
    L.newest = c->nsteps > 0 ? (int)((c->nsteps - 1) % R) : -1;
    return L;
}

// The hazards of a copy on S that reads or writes X[base], the ring and, pipelined, X[out]: behind the
// event guarding base (as enqueue) and behind the newest flush on D, which reads X[in] and the ring
// and writes X[out]
static int rs_wait(ekf_ctx* c)
{
    if (c->ev_base) HIP_TRY(hipStreamWaitEvent(c->stream, c->ev_base, 0));
    if (c->cfg.pipeline && c->nflush > 0)
        HIP_TRY(hipStreamWaitEvent(c->stream, c->ev_flush[(c->nflush - 1) & 1], 0));
    return EKF_OK;
}

// One table-driven copy on S. The table goes into the context's pinned buffer, which is rewritten only
// after the last launch that reads it (rs_ev); launch(table, nseg) enqueues the kernel on the table's
// device address. The caller closes with end_read: the next flush on D waits for the copy too.
template <typename Seg, typename F>
static int run_table(ekf_ctx* c, const std::vector<Seg>& table, F launch)
{
    if (c->rs_pending) HIP_TRY(hipEventSynchronize(c->rs_ev));
    c->rs_pending = 0;
    if (!c->rs_ev) HIP_TRY(hipEventCreateWithFlags(&c->rs_ev, hipEventDisableTiming));
    const size_t bytes = sizeof(Seg) * table.size();
    int rc = pinned_reserve(c->rs_pin, bytes);
    if (rc) return rc;
    memcpy(c->rs_pin.host, table.data(), bytes);
    rc = rs_wait(c);
    if (rc) return rc;
    HIP_TRY(launch(reinterpret_cast<const Seg*>(c->rs_pin.dev), (int)table.size()));
    HIP_TRY(hipEventRecord(c->rs_ev, c->stream));
    c->rs_pending = 1;
    return EKF_OK;
}

extern "C" int ekf_resample(ekf_ctx* c, const int32_t* src)
{
    if (!c || !src || c->sh_world > 0) return EKF_EINVAL;
    const int E = c->cfg.instances;
    const int bad = ekf::resample_check(src, E);
    if (bad) return bad == 2 ? EKF_ERANGE : EKF_EINVAL;
    if (c->predicted) return EKF_EINVAL;   // the committed strip is the predicted one
    bool any = false;
    for (int e = 0; e < E; e++) any = any || src[e] != e;
    if (!any) return EKF_OK;
    const std::vector<ekf::CopySeg> table = ekf::resample_plan(ekf::resample_arrays(resample_layout(c)), E, src);
    int rc = run_table(c, table, [c](const ekf::CopySeg* t, int nseg) {
        return ekf::launch_resample(t, nseg, c->ncu, c->stream);
    });
    if (!rc) rc = end_read(c);
    if (rc) return rc;
    for (int e = 0; e < E; e++) c->pexp_h[e] = c->pexp_h[src[e]];   // (a source keeps its own: fixed points)
    c->mirror_epoch = 0;   // the mirrored robot blocks are stale for the overwritten instances
    return EKF_OK;
}

extern "C" int ekf_copy_instance(ekf_ctx* c, int dst, int from)
{
    if (!c || c->sh_world > 0) return EKF_EINVAL;
    const int E = c->cfg.instances;
    if (dst < 0 || dst >= E || from < 0 || from >= E) return EKF_ERANGE;
    std::vector<int32_t> src((size_t)E);
    for (int e = 0; e < E; e++) src[e] = e;
    src[dst] = from;
    return ekf_resample(c, src.data());
}

// ---- the device forms: the plan and the copy under a list in device memory ----
extern "C" int ekf_resample_plan_device(ekf_ctx* c, const double* d_weights, double u, double ess_below, int32_t* d_src,
                                        ekf_plan_info* d_info)
{
    if (!c || !d_weights || !d_src || c->sh_world > 0 || ess_below != ess_below) return EKF_EINVAL;
    if (!(u >= 0.0 && u < 1.0)) return EKF_ERANGE;
    HIP_TRY(ekf::launch_resample_plan(d_weights, c->cfg.instances, u, ess_below, d_src, d_info, c->stream));
    return EKF_OK;
}

// ekf_resample with the list on the device: the pieces of one instance's slices go into the pinned table,
// a wave checks the list and the copy applies the pieces to the pairs it found (unit_resample_device.hip).
// The hazards are ekf_resample's (rs_wait before, end_read behind). What the host mirrors of the
// overwritten instances becomes stale as a whole: it cannot know which they are.
extern "C" int ekf_resample_device(ekf_ctx* c, const int32_t* d_src, int32_t* d_status)
{
    if (!c || !d_src || c->sh_world > 0) return EKF_EINVAL;
    if (c->predicted) return EKF_EINVAL;   // the committed strip is the predicted one
    const int E = c->cfg.instances;
    if (!c->rsd_plan) {
        void* pl = nullptr;
        if (!dev_alloc(c, &pl, sizeof(int32_t) * ekf::resample_device_plan_words(E))) return EKF_ENOMEM;
        c->rsd_plan = (int32_t*)pl;
    }
    const std::vector<ekf::CopyPiece> pieces = ekf::resample_pieces(ekf::resample_arrays(resample_layout(c)));
    int rc = run_table(c, pieces, [c, d_src, d_status, E](const ekf::CopyPiece* t, int n) {
        return ekf::launch_resample_device(d_src, E, c->rsd_plan, d_status, t, n, c->ncu, c->stream);
    });
    if (!rc) rc = end_read(c);
    if (rc) return rc;
    c->pexp_stale = 1;     // (pexp_mirror)
    c->mirror_epoch = 0;   // the mirrored robot blocks are stale for the overwritten instances
    return EKF_OK;
}

// ---- instance images ----
// The arrays of ekf_resample in logical order, one instance of each as a 16-byte padded section.
// Nothing of the schedule changes in either direction; the import maps the sections onto this
// context's own ring slots and buffers and re-tags the completion words with its epoch.
static std::vector<ekf::ResampleArray> image_arrays_of(const ekf_ctx* c)
{
    return ekf::image_arrays(resample_layout(c), c->base);
}

static uint64_t image_key_of(const ekf_ctx* c)
{
    const ekf_config& g = c->cfg;
    const ekf::ImageConfig ic = {g.capacity, g.precision, g.max_lines, g.r_mode, g.reset_margin, g.pipeline ? 1 : 0,
                                 c->T, g.arith, g.mahalanobis, g.encoder_noise};
    return ekf::image_key(resample_layout(c), (int)c->elem, ic);
}

extern "C" size_t ekf_instance_image_bytes(const ekf_ctx* c)
{
    if (!c || c->sh_world > 0) return 0;
    return (size_t)ekf::image_bytes(image_arrays_of(c));
}

// The checks both directions share; 0 or the status to return
static int image_args(const ekf_ctx* c, const int32_t* inst, int K, const void* images, const void* desc)
{
    if (!c || !inst || !images || !desc || c->sh_world > 0) return EKF_EINVAL;
    const int E = c->cfg.instances;
    if (K < 0 || K > E) return EKF_ERANGE;
    for (int k = 0; k < K; k++)
        if (inst[k] < 0 || inst[k] >= E) return EKF_ERANGE;
    if (c->predicted) return EKF_EINVAL;   // the committed strip is the predicted one
    return EKF_OK;
}

static int image_describe(ekf_ctx* c, const int32_t* inst, int K, uint64_t bytes, ekf_image_desc* desc)
{
    const int rc = pexp_mirror(c);   // (storage_exp below)
    if (rc) return rc;
    const uint64_t key = image_key_of(c);
    for (int k = 0; k < K; k++) {
        ekf_image_desc& d = desc[k];
        memset(&d, 0, sizeof(d));
        d.magic = ekf::IMAGE_MAGIC;
        d.version = ekf::IMAGE_VERSION;
        d.key = key;
        d.bytes = bytes;
        d.pending = (int32_t)(c->nsteps - c->pend0);
        d.has_step = c->nsteps > 0;
        d.epoch = c->scan_epoch;
        d.groups = c->last_G;
        d.storage_exp = c->pexp_h[inst[k]];
    }
    return EKF_OK;
}

// import: the list names no slot twice and every descriptor is congruent with this context
static int image_congruent(const ekf_ctx* c, const int32_t* inst, int K, uint64_t bytes, const ekf_image_desc* desc)
{
    std::vector<char> seen((size_t)c->cfg.instances, 0);
    for (int k = 0; k < K; k++) {
        if (seen[(size_t)inst[k]]) return EKF_EINVAL;
        seen[(size_t)inst[k]] = 1;
    }
    const uint64_t key = image_key_of(c);
    for (int k = 0; k < K; k++) {
        const ekf_image_desc& d = desc[k];
        if (d.magic != ekf::IMAGE_MAGIC || d.version != ekf::IMAGE_VERSION || d.key != key || d.bytes != bytes ||
            d.pending != (int32_t)(c->nsteps - c->pend0) || d.has_step != (c->nsteps > 0 ? 1 : 0) ||
            d.groups != c->last_G)
            return EKF_EINVAL;
    }
    return EKF_OK;
}

// the host state an imported slot takes with its image
static void image_adopt(ekf_ctx* c, const int32_t* inst, int K, const ekf_image_desc* desc)
{
    for (int k = 0; k < K; k++) c->pexp_h[(size_t)inst[k]] = desc[k].storage_exp;
    c->mirror_epoch = 0;   // the mirrored robot blocks are stale for the slots
}

// the device forms' copy: the table of ekf_image_plan.h, the re-tag pieces under this context's epoch
static int run_image_table(ekf_ctx* c, const std::vector<ekf::CopySeg>& table)
{
    return run_table(c, table, [c](const ekf::CopySeg* t, int nseg) {
        return ekf::launch_image(t, nseg, c->scan_epoch, c->ncu, c->stream);
    });
}

extern "C" int ekf_export_instances(ekf_ctx* c, const int32_t* inst, int K, void* images, ekf_image_desc* desc)
{
    int rc = image_args(c, inst, K, images, desc);
    if (rc || K == 0) return rc;
    const std::vector<ekf::ResampleArray> arrays = image_arrays_of(c);
    const std::vector<ekf::ImageSection> sec = ekf::image_sections(arrays);
    const uint64_t bytes = ekf::image_bytes(arrays);
    rc = rs_wait(c);
    if (rc) return rc;
    for (int k = 0; k < K; k++)
        for (const ekf::ImageSection& s : sec) {
            char* q = (char*)images + (size_t)k * bytes + s.offset;
            HIP_TRY(hipMemcpyAsync(q, (const void*)(uintptr_t)(s.base + (uint64_t)inst[k] * s.bytes), s.bytes,
                                   hipMemcpyDeviceToHost, c->stream));
            memset(q + s.bytes, 0, (size_t)(ekf::image_pad16(s.bytes) - s.bytes));
        }
    HIP_TRY(hipStreamSynchronize(c->stream));
    return image_describe(c, inst, K, bytes, desc);
}

extern "C" int ekf_import_instances(ekf_ctx* c, const int32_t* inst, int K, const void* images,
                                    const ekf_image_desc* desc)
{
    int rc = image_args(c, inst, K, images, desc);
    if (rc || K == 0) return rc;
    const std::vector<ekf::ResampleArray> arrays = image_arrays_of(c);
    const std::vector<ekf::ImageSection> sec = ekf::image_sections(arrays);
    const uint64_t bytes = ekf::image_bytes(arrays);
    rc = image_congruent(c, inst, K, bytes, desc);
    if (rc) return rc;
    rc = rs_wait(c);
    if (rc) return rc;
    // the completion words on a private copy (the caller's buffer stays as exported), alive until the wait
    const size_t sw = (size_t)c->sync_stride;
    std::vector<uint32_t> words(sw * (size_t)K);
    for (int k = 0; k < K; k++)
        for (const ekf::ImageSection& s : sec) {
            const char* p = (const char*)images + (size_t)k * bytes + s.offset;
            const void* from = p;
            if (s.base == (uint64_t)(uintptr_t)c->sync) {
                uint32_t* w = words.data() + sw * (size_t)k;
                memcpy(w, p, sizeof(uint32_t) * sw);
                for (int g = 0; g < desc[k].groups; g++)
                    w[ekf::SYNC_WG0 + g] = ekf::image_retag(w[ekf::SYNC_WG0 + g], desc[k].epoch, c->scan_epoch);
                from = w;
            }
            HIP_TRY(hipMemcpyAsync((void*)(uintptr_t)(s.base + (uint64_t)inst[k] * s.bytes), from, s.bytes,
                                   hipMemcpyHostToDevice, c->stream));
        }
    HIP_TRY(hipStreamSynchronize(c->stream));
    image_adopt(c, inst, K, desc);
    return end_read(c);
}

extern "C" int ekf_export_instances_device(ekf_ctx* c, const int32_t* inst, int K, void* d_images, ekf_image_desc* desc)
{
    int rc = image_args(c, inst, K, d_images, desc);
    if (rc || K == 0) return rc;
    if ((uintptr_t)d_images & 3) return EKF_EINVAL;
    const std::vector<ekf::ResampleArray> arrays = image_arrays_of(c);
    const std::vector<ekf::CopySeg> table = ekf::image_export_plan(arrays, inst, K, (uint64_t)(uintptr_t)d_images);
    rc = run_image_table(c, table);
    if (rc) return rc;
    rc = image_describe(c, inst, K, ekf::image_bytes(arrays), desc);
    return rc ? rc : end_read(c);
}

extern "C" int ekf_import_instances_device(ekf_ctx* c, const int32_t* inst, int K, const void* d_images,
                                           const ekf_image_desc* desc)
{
    int rc = image_args(c, inst, K, d_images, desc);
    if (rc || K == 0) return rc;
    if ((uintptr_t)d_images & 3) return EKF_EINVAL;
    const std::vector<ekf::ResampleArray> arrays = image_arrays_of(c);
    rc = image_congruent(c, inst, K, ekf::image_bytes(arrays), desc);
    if (rc) return rc;
    std::vector<uint32_t> epochs((size_t)K);
    for (int k = 0; k < K; k++) epochs[(size_t)k] = desc[k].epoch;
    const std::vector<ekf::CopySeg> table =
        ekf::image_import_plan(arrays, (uint64_t)(uintptr_t)c->sync, ekf::SYNC_WG0, c->last_G, inst, epochs.data(), K,
                               (uint64_t)(uintptr_t)d_images);
    rc = run_image_table(c, table);
    if (rc) return rc;
    image_adopt(c, inst, K, desc);
    return end_read(c);
}
