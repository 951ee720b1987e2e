// ekf_read.hip — the calls that read the state without draining the flush (slam_ekf.h): the covariance
// queries (ekf_query_*; kernel: unit_query.hip), the gate (ekf_gate_lines*; unit_gate.hip), the joint
// gate (ekf_gate_joint*; unit_joint.hip), the joint-compatibility search (ekf_associate_joint*;
// unit_assoc.hip) and the landmark pairs (ekf_gate_landmarks*; unit_pairs.hip). Beside them the two stages of the hypothesis loop that read only what those calls wrote
// (ekf_gate_candidates_device, ekf_assoc_weights_device; unit_loop.hip): no view, no hazard handling.
//
// Each kernel takes the view the next association kernel would take in enqueue() (ReadView): X[base]
// once the event guarding it has passed, the steps [pend0, nsteps) applied on read, the committed copy
// of the strip and the mean. It runs on S after every scan enqueued so far and changes nothing: no
// flush, no step, no epoch. begin_read / end_read are the hazard handling.
#include "ekf_ctx.h"
#include "ekf_pairs.h"   // (PairParams, launch_pairs)

static int begin_read(ekf_ctx* c, ekf::ReadView& v, ekf::Slot* pend)
{
    if (c->ev_base) HIP_TRY(hipStreamWaitEvent(c->stream, c->ev_base, 0));
    const int np = (int)(c->nsteps - c->pend0);
    if (np > ekf::PMAX) return EKF_EINVAL;   // unreachable: T <= 24
    v.d = c->d;
    v.Etot = c->cfg.instances;
    v.usym = usym_of(c);
    v.bf = c->pmode;
    v.npend = np;
    v.Pread = xview(c, c->base);
    v.Rs = c->Rs;
    v.y = c->y;
    v.live = c->cur;
    v.pexp = c->pexp;
    for (int q = 0; q < np; q++) pend[q] = slot_of(c, c->pend0 + q);
    return EKF_OK;
}

// L lines per row (the host form) or nlines[row] (the device form) on the context's committed state
static ekf::TrialLines trial_lines(const ekf_ctx* c, int L, const double* enc, const ekf_line* lines, const int* nlines)
{
    ekf::TrialLines t{};
    t.L = L;
    t.enc = enc;
    t.lines = lines;
    t.nlines = nlines;
    t.pose = c->pose;
    t.xpre = c->xpre;
    t.saved = c->saved;
    t.use_xpre = c->predicted;
    t.r_mode = c->cfg.r_mode;
    t.gate = c->cfg.mahalanobis;
    t.enc_noise = c->cfg.encoder_noise;
    return t;
}

// ---- the host forms: one kernel, one copy, one wait ----
// Device scratch for `bytes` of results, and the pinned buffer [results | inputs]: the one copy lands in
// its first `bytes`, the kernel reads the request's inputs (at most `tail` bytes) from behind them.
static int host_form(ekf_ctx* c, size_t bytes, size_t tail)
{
    if (bytes > c->q_dev_bytes) {
        if (c->q_dev) (void)hipFree(c->q_dev);
        c->q_dev = nullptr;
        c->q_dev_bytes = 0;
        if (hipMalloc((void**)&c->q_dev, bytes) != hipSuccess) {
            c->q_dev = nullptr;
            return EKF_ENOMEM;
        }
        c->q_dev_bytes = bytes;
    }
    return pinned_reserve(c->q_pin, bytes + tail);
}

// n entries of src into the pinned buffer at *off, which moves past them; their device address
// (src == nullptr: the room is kept, nothing is read)
template <typename V>
static const V* stage_input(ekf_ctx* c, size_t* off, const V* src, size_t n)
{
    const size_t at = *off;
    *off += sizeof(V) * n;
    if (!src) return nullptr;
    memcpy(c->q_pin.host + at, src, sizeof(V) * n);
    return reinterpret_cast<const V*>(c->q_pin.dev + at);
}

// the results into the pinned buffer, behind the kernel; they then leave by memcpy
static int fetch_results(ekf_ctx* c, size_t bytes)
{
    HIP_TRY(hipMemcpyAsync(c->q_pin.host, c->q_dev, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return EKF_OK;
}

// ---- covariance queries ----
static int enqueue_query(ekf_ctx* c, ekf::QueryParams& qp)
{
    const int rc = begin_read(c, qp.v, qp.pend);
    if (rc) return rc;
    HIP_TRY(ekf::launch_query(qp, c->cfg.precision, c->stream));
    return end_read(c);
}

// The queries' argument checks (before any HIP call); landmarks: a host list, or nullptr
static int query_check(const ekf_ctx* c, int e, const int32_t* landmarks, int K, bool need_list)
{
    if (!c || c->sh_world > 0) return EKF_EINVAL;
    if (e < 0 || e >= c->cfg.instances || K < 0 || K > c->d.N) return EKF_ERANGE;
    if (need_list && K > 0 && !landmarks) return EKF_EINVAL;
    if (landmarks)
        for (int k = 0; k < K; k++)
            if (landmarks[k] < 0 || landmarks[k] >= c->d.N) return EKF_ERANGE;
    return EKF_OK;
}

static ekf::QueryParams query_params(int mode, int E, int e0, int K)
{
    ekf::QueryParams qp{};
    qp.mode = mode;
    qp.E = E;
    qp.e0 = e0;
    qp.K = K;
    return qp;
}

// `bytes` of results of one instance's query into the pinned buffer
static int run_host_query(ekf_ctx* c, ekf::QueryParams& qp, const int32_t* landmarks, size_t bytes)
{
    size_t off = bytes;
    qp.landmarks = stage_input(c, &off, landmarks, (size_t)qp.K);
    const int rc = enqueue_query(c, qp);
    return rc ? rc : fetch_results(c, bytes);
}

extern "C" int ekf_query_joint(ekf_ctx* c, int e, const int32_t* landmarks, int K, double* cov, double* mean)
{
    int rc = query_check(c, e, landmarks, K, true);
    if (rc) return rc;
    if (!cov && !mean) return EKF_OK;
    const size_t nq = 3 + 2 * (size_t)K;
    const size_t ncov = cov ? nq * nq : 0;
    const size_t bytes = sizeof(double) * (ncov + nq);
    rc = host_form(c, bytes, sizeof(int32_t) * (size_t)K);
    if (rc) return rc;
    ekf::QueryParams qp = query_params(ekf::QUERY_JOINT, 1, e, K);
    qp.cov = cov ? c->q_dev : nullptr;
    qp.mean = c->q_dev + ncov;
    rc = run_host_query(c, qp, landmarks, bytes);
    if (rc) return rc;
    const double* h = reinterpret_cast<const double*>(c->q_pin.host);
    if (cov) memcpy(cov, h, sizeof(double) * ncov);
    if (mean) memcpy(mean, h + ncov, sizeof(double) * nq);
    return EKF_OK;
}

extern "C" int ekf_query_marginals(ekf_ctx* c, int e, const int32_t* landmarks, int K, double* blocks,
                                   double* cross, double* mean)
{
    int rc = query_check(c, e, landmarks, K, false);
    if (rc) return rc;
    if (K == 0 || (!blocks && !cross && !mean)) return EKF_OK;
    const size_t k = (size_t)K;
    const size_t bytes = sizeof(double) * 12 * k;
    rc = host_form(c, bytes, landmarks ? sizeof(int32_t) * k : 0);
    if (rc) return rc;
    ekf::QueryParams qp = query_params(ekf::QUERY_MARGINALS, 1, e, K);
    qp.blocks = c->q_dev;
    qp.cross = c->q_dev + 4 * k;
    qp.mean = c->q_dev + 10 * k;
    rc = run_host_query(c, qp, landmarks, bytes);
    if (rc) return rc;
    const double* h = reinterpret_cast<const double*>(c->q_pin.host);
    if (blocks) memcpy(blocks, h, sizeof(double) * 4 * k);
    if (cross) memcpy(cross, h + 4 * k, sizeof(double) * 6 * k);
    if (mean) memcpy(mean, h + 10 * k, sizeof(double) * 2 * k);
    return EKF_OK;
}

extern "C" int ekf_query_joint_device(ekf_ctx* c, const int32_t* d_landmarks, int K, double* d_cov, double* d_mean)
{
    const int rc = query_check(c, 0, nullptr, K, false);
    if (rc) return rc;
    if (K > 0 && !d_landmarks) return EKF_EINVAL;
    if (!d_cov && !d_mean) return EKF_OK;
    ekf::QueryParams qp = query_params(ekf::QUERY_JOINT, c->cfg.instances, 0, K);
    qp.landmarks = K > 0 ? d_landmarks : nullptr;
    qp.cov = d_cov;
    qp.mean = d_mean;
    return enqueue_query(c, qp);
}

// ---- trial lines: the gate (two launches on S) and the joint gate (one; its only scratch is its LDS) ----
// The argument checks the four forms share (before any HIP call; each form then checks its own pointers,
// which is EKF_EINVAL too). The device forms pass e = 0 and L = 0, the gate H = 0.
static int trial_check(const ekf_ctx* c, int e, int L, int H, const double* enc)
{
    if (!c || c->sh_world > 0) return EKF_EINVAL;
    if (e < 0 || e >= c->cfg.instances || L < 0 || L > c->d.max_lines || H < 0) return EKF_ERANGE;
    if (enc && c->predicted) return EKF_EINVAL;   // the committed strip is already the predicted one
    return EKF_OK;
}

static int enqueue_gate(ekf_ctx* c, ekf::GateParams& gp)
{
    if (!c->g_flags) {
        const size_t rows = (size_t)c->cfg.instances * c->d.max_lines;
        void* fl = nullptr;
        void* pt = nullptr;
        if (!dev_alloc(c, &fl, rows * c->d.N) ||
            !dev_alloc(c, &pt, rows * ekf::gate_waves(c->d.N) * sizeof(ekf::GatePart)))
            return EKF_ENOMEM;   // (listed either way: free_all releases what was made)
        c->g_flags = (unsigned char*)fl;
        c->g_part = (ekf::GatePart*)pt;
    }
    const int rc = begin_read(c, gp.v, gp.pend);
    if (rc) return rc;
    gp.flags = c->g_flags;
    gp.part = c->g_part;
    HIP_TRY(ekf::launch_gate(gp, c->cfg.precision, c->stream));
    return end_read(c);
}

static int enqueue_joint(ekf_ctx* c, ekf::JointParams& jp)
{
    const int rc = begin_read(c, jp.v, jp.pend);
    if (rc) return rc;
    HIP_TRY(ekf::launch_joint(jp, c->cfg.precision, c->stream));
    return end_read(c);
}

extern "C" int ekf_gate_lines(ekf_ctx* c, int e, const double enc[3], const ekf_line* lines, int L,
                              ekf_gate_hit* hits, double* d2)
{
    int rc = trial_check(c, e, L, 0, enc);
    if (rc) return rc;
    if ((L > 0 && !lines) || !hits) return EKF_EINVAL;
    if (L == 0) return EKF_OK;
    // device scratch [hits | d2], the pinned buffer [hits | d2 | lines | enc]
    const size_t nh = sizeof(ekf_gate_hit) * (size_t)L;
    const size_t nd = d2 ? sizeof(double) * (size_t)L * c->d.N : 0;
    rc = host_form(c, nh + nd, sizeof(ekf_line) * (size_t)L + 3 * sizeof(double));
    if (rc) return rc;
    size_t off = nh + nd;
    const ekf_line* p_lines = stage_input(c, &off, lines, (size_t)L);
    const double* p_enc = stage_input(c, &off, enc, 3);
    ekf::GateParams gp{};
    gp.E = 1;
    gp.e0 = e;
    gp.t = trial_lines(c, L, p_enc, p_lines, nullptr);
    char* dev = reinterpret_cast<char*>(c->q_dev);
    gp.hits = reinterpret_cast<ekf_gate_hit*>(dev);
    gp.d2 = d2 ? reinterpret_cast<double*>(dev + nh) : nullptr;
    rc = enqueue_gate(c, gp);
    if (!rc) rc = fetch_results(c, nh + nd);
    if (rc) return rc;
    memcpy(hits, c->q_pin.host, nh);
    if (d2) memcpy(d2, c->q_pin.host + nh, nd);
    return EKF_OK;
}

extern "C" int ekf_gate_lines_device(ekf_ctx* c, const double* d_enc, const ekf_line* d_lines,
                                     const int32_t* d_nlines, ekf_gate_hit* d_hits, double* d_d2)
{
    const int rc = trial_check(c, 0, 0, 0, d_enc);
    if (rc) return rc;
    if (!d_lines || !d_nlines || !d_hits) return EKF_EINVAL;
    ekf::GateParams gp{};
    gp.E = c->cfg.instances;
    gp.t = trial_lines(c, 0, d_enc, d_lines, d_nlines);
    gp.hits = d_hits;
    gp.d2 = d_d2;
    return enqueue_gate(c, gp);
}

extern "C" int ekf_gate_joint(ekf_ctx* c, int e, const double enc[3], const ekf_line* lines, int L,
                              const int32_t* assign, int H, ekf_joint_hit* hits, double* d2_each)
{
    int rc = trial_check(c, e, L, H, enc);
    if (rc) return rc;
    if ((L > 0 && !lines) || (H > 0 && !hits) || (H > 0 && L > 0 && !assign)) return EKF_EINVAL;
    const size_t HL = (size_t)H * L;
    for (size_t k = 0; k < HL; k++)
        if (assign[k] < -1 || assign[k] >= c->d.N) return EKF_ERANGE;
    if (H == 0) return EKF_OK;
    if (L == 0) {   // every hypothesis is empty
        for (int h = 0; h < H; h++) hits[h] = ekf_joint_hit{0, 0, 0.0, 0.0};
        return EKF_OK;
    }
    // device scratch [hits | d2_each], the pinned buffer [hits | d2_each | lines | enc | assign]
    const size_t nh = sizeof(ekf_joint_hit) * (size_t)H;
    const size_t nd = d2_each ? sizeof(double) * HL : 0;
    rc = host_form(c, nh + nd, sizeof(ekf_line) * (size_t)L + 3 * sizeof(double) + sizeof(int32_t) * HL);
    if (rc) return rc;
    size_t off = nh + nd;
    const ekf_line* p_lines = stage_input(c, &off, lines, (size_t)L);
    const double* p_enc = stage_input(c, &off, enc, 3);
    ekf::JointParams jp{};
    jp.E = 1;
    jp.e0 = e;
    jp.t = trial_lines(c, L, p_enc, p_lines, nullptr);
    jp.H = H;
    jp.astride = L;
    jp.assign = stage_input(c, &off, assign, HL);
    char* dev = reinterpret_cast<char*>(c->q_dev);
    jp.hits = reinterpret_cast<ekf_joint_hit*>(dev);
    jp.d2_each = d2_each ? reinterpret_cast<double*>(dev + nh) : nullptr;
    rc = enqueue_joint(c, jp);
    if (!rc) rc = fetch_results(c, nh + nd);
    if (rc) return rc;
    memcpy(hits, c->q_pin.host, nh);
    if (d2_each) memcpy(d2_each, c->q_pin.host + nh, nd);
    return EKF_OK;
}

extern "C" int ekf_gate_joint_device(ekf_ctx* c, const double* d_enc, const ekf_line* d_lines, const int32_t* d_nlines,
                                     const int32_t* d_assign, int H, ekf_joint_hit* d_hits, double* d_d2_each)
{
    const int rc = trial_check(c, 0, 0, H, d_enc);
    if (rc) return rc;
    if (!d_lines || !d_nlines || (H > 0 && (!d_assign || !d_hits))) return EKF_EINVAL;
    if (H == 0) return EKF_OK;
    ekf::JointParams jp{};
    jp.E = c->cfg.instances;
    jp.t = trial_lines(c, 0, d_enc, d_lines, d_nlines);
    jp.H = H;
    jp.astride = c->d.max_lines;
    jp.assign = d_assign;
    jp.hits = d_hits;
    jp.d2_each = d_d2_each;
    return enqueue_joint(c, jp);
}

// ---- the joint-compatibility search (three launches on S; its tables are the context's scratch) ----
static int enqueue_assoc(ekf_ctx* c, ekf::AssocParams& ap)
{
    if (!c->as_plan) {
        const size_t E = (size_t)c->cfg.instances;
        void* pl = nullptr;
        void* ct = nullptr;
        void* pt = nullptr;
        void* rc = nullptr;
        if (!dev_alloc(c, &pl, E * sizeof(ekf::AssocPlan)) ||
            !dev_alloc(c, &ct, E * EKF_ASSOC_MAX_TOTAL * ekf::ASSOC_CWORDS * sizeof(double)) ||
            !dev_alloc(c, &pt, E * ekf::ASSOC_PAIRS * 4 * sizeof(double)) ||
            !dev_alloc(c, &rc, E * ekf::ASSOC_W * sizeof(ekf::AssocRec)))
            return EKF_ENOMEM;   // (listed either way: free_all releases what was made)
        c->as_ctab = (double*)ct;
        c->as_ptab = (double*)pt;
        c->as_rec = (ekf::AssocRec*)rc;
        c->as_plan = (ekf::AssocPlan*)pl;
    }
    const int rc = begin_read(c, ap.v, ap.pend);
    if (rc) return rc;
    ap.plan = c->as_plan;
    ap.ctab = c->as_ctab;
    ap.ptab = c->as_ptab;
    ap.rec = c->as_rec;
    HIP_TRY(ekf::launch_assoc(ap, c->cfg.precision, c->stream));
    return end_read(c);
}

// the checks both forms share, after trial_check
static int assoc_check(int C, int max_nodes)
{
    if (C < 1 || C > EKF_ASSOC_MAX_CAND || max_nodes < 1 || max_nodes > EKF_ASSOC_MAX_NODES) return EKF_ERANGE;
    return EKF_OK;
}

extern "C" int ekf_associate_joint(ekf_ctx* c, int e, const double enc[3], const ekf_line* lines, int L,
                                   const int32_t* cand, int C, const double* bound, int max_nodes, ekf_assoc_hit* hit)
{
    if (!c || c->sh_world > 0 || (L > 0 && (!lines || !cand)) || !bound || !hit) return EKF_EINVAL;
    int rc = trial_check(c, e, L, 0, enc);
    if (!rc) rc = assoc_check(C, max_nodes);
    if (rc) return rc;
    const size_t LC = (size_t)L * C;
    for (size_t k = 0; k < LC; k++)
        if (cand[k] < -1 || cand[k] >= c->d.N) return EKF_ERANGE;
    if (L == 0) {   // the empty hypothesis
        memset(hit, 0, sizeof(*hit));
        for (int i = 0; i < EKF_MAX_LINES; i++) hit->assign[i] = -1;
        return EKF_OK;
    }
    // device scratch [hit], the pinned buffer [hit | lines | enc | bound | cand]
    const size_t nh = sizeof(ekf_assoc_hit);
    rc = host_form(c, nh, sizeof(ekf_line) * (size_t)L + sizeof(double) * (3 + (size_t)L + 1) + sizeof(int32_t) * LC);
    if (rc) return rc;
    size_t off = nh;
    const ekf_line* p_lines = stage_input(c, &off, lines, (size_t)L);
    const double* p_enc = stage_input(c, &off, enc, 3);
    ekf::AssocParams ap{};
    ap.E = 1;
    ap.e0 = e;
    ap.t = trial_lines(c, L, p_enc, p_lines, nullptr);
    ap.C = C;
    ap.budget = max_nodes / ekf::ASSOC_W;
    ap.bound = stage_input(c, &off, bound, (size_t)L + 1);
    ap.cand = stage_input(c, &off, cand, LC);
    ap.hits = reinterpret_cast<ekf_assoc_hit*>(c->q_dev);
    rc = enqueue_assoc(c, ap);
    if (!rc) rc = fetch_results(c, nh);
    if (rc) return rc;
    memcpy(hit, c->q_pin.host, nh);
    // (every entry was in [-1, N): what is left is a cap, EKF_ASSOC_MAX_LINES or EKF_ASSOC_MAX_TOTAL, which
    // counts the usable candidates and so is known on the device only)
    return (hit->status & EKF_AS_INVALID) ? EKF_ERANGE : EKF_OK;
}

extern "C" int ekf_associate_joint_device(ekf_ctx* c, const double* d_enc, const ekf_line* d_lines,
                                          const int32_t* d_nlines, const int32_t* d_cand, int C, const double* d_bound,
                                          int max_nodes, ekf_assoc_hit* d_hits)
{
    if (!c || c->sh_world > 0 || !d_lines || !d_nlines || !d_cand || !d_bound || !d_hits) return EKF_EINVAL;
    int rc = trial_check(c, 0, 0, 0, d_enc);
    if (!rc) rc = assoc_check(C, max_nodes);
    if (rc) return rc;
    ekf::AssocParams ap{};
    ap.E = c->cfg.instances;
    ap.t = trial_lines(c, 0, d_enc, d_lines, d_nlines);
    ap.C = C;
    ap.budget = max_nodes / ekf::ASSOC_W;
    ap.bound = d_bound;
    ap.cand = d_cand;
    ap.hits = d_hits;
    return enqueue_assoc(c, ap);
}

// ---- landmark pairs (two launches on S; the partial records are the context's scratch) ----
static int pairs_check(const ekf_ctx* c, int e, double gate, const ekf_pair_hit* hits)
{
    if (!c || c->sh_world > 0 || !hits) return EKF_EINVAL;
    if (!(gate >= 0.0) || gate - gate != 0.0) return EKF_EINVAL;   // NaN, negative, +inf
    if (e < 0 || e >= c->cfg.instances) return EKF_ERANGE;
    return EKF_OK;
}

static int enqueue_pairs(ekf_ctx* c, ekf::PairParams& pp)
{
    if (!c->pr_part) {
        void* pt = nullptr;
        if (!dev_alloc(c, &pt, (size_t)c->cfg.instances * c->d.N * ekf::pair_blocks(c->d.N) * sizeof(ekf_pair_hit)))
            return EKF_ENOMEM;
        c->pr_part = (ekf_pair_hit*)pt;
    }
    const int rc = begin_read(c, pp.v, pp.pend);
    if (rc) return rc;
    pp.saved = c->saved;
    pp.part = c->pr_part;
    HIP_TRY(ekf::launch_pairs(pp, c->cfg.precision, c->stream));
    return end_read(c);
}

extern "C" int ekf_gate_landmarks(ekf_ctx* c, int e, double gate, ekf_pair_hit* hits, double* d2)
{
    int rc = pairs_check(c, e, gate, hits);
    if (rc) return rc;
    // device scratch and the pinned buffer: [hits | d2]
    const size_t N = (size_t)c->d.N;
    const size_t nh = sizeof(ekf_pair_hit) * N;
    const size_t nd = d2 ? sizeof(double) * N * N : 0;
    rc = host_form(c, nh + nd, 0);
    if (rc) return rc;
    ekf::PairParams pp{};
    pp.E = 1;
    pp.e0 = e;
    pp.gate = gate;
    char* dev = reinterpret_cast<char*>(c->q_dev);
    pp.hits = reinterpret_cast<ekf_pair_hit*>(dev);
    pp.d2 = d2 ? reinterpret_cast<double*>(dev + nh) : nullptr;
    rc = enqueue_pairs(c, pp);
    if (!rc) rc = fetch_results(c, nh + nd);
    if (rc) return rc;
    memcpy(hits, c->q_pin.host, nh);
    if (d2) memcpy(d2, c->q_pin.host + nh, nd);
    return EKF_OK;
}

extern "C" int ekf_gate_landmarks_device(ekf_ctx* c, double gate, ekf_pair_hit* d_hits, double* d_d2)
{
    const int rc = pairs_check(c, 0, gate, d_hits);
    if (rc) return rc;
    ekf::PairParams pp{};
    pp.E = c->cfg.instances;
    pp.gate = gate;
    pp.hits = d_hits;
    pp.d2 = d_d2;
    return enqueue_pairs(c, pp);
}

// ---- the loop's stages around the search: functions of the gate's matrix and of the hits, no filter state ----
extern "C" int ekf_gate_candidates_device(ekf_ctx* c, const double* d_d2, const int32_t* d_nlines, int C, double gate,
                                          int32_t* d_cand, int32_t* d_count)
{
    if (!c || c->sh_world > 0 || !d_d2 || !d_nlines || !d_cand) return EKF_EINVAL;
    if (!(gate >= 0.0) || gate - gate != 0.0) return EKF_EINVAL;   // NaN, negative, +inf
    if (C < 1 || C > EKF_ASSOC_MAX_CAND) return EKF_ERANGE;
    HIP_TRY(ekf::launch_gate_candidates(d_d2, d_nlines, c->cfg.instances, c->d.max_lines, c->d.N, C, gate, d_cand,
                                        d_count, c->stream));
    return EKF_OK;
}

extern "C" int ekf_assoc_weights_device(ekf_ctx* c, const ekf_assoc_hit* d_hits, const int32_t* d_nlines,
                                        double log_unassigned, const double* d_logprior, double* d_weights)
{
    if (!c || c->sh_world > 0 || !d_hits || !d_nlines || !d_weights) return EKF_EINVAL;
    HIP_TRY(ekf::launch_assoc_weights(d_hits, d_nlines, c->cfg.instances, log_unassigned, d_logprior, d_weights,
                                      c->stream));
    return EKF_OK;
}
