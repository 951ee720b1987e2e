// image_driver.cpp — the instance image's tables (csrc/ekf_image_plan.h) on a CPU: a stand-alone
// program, built with AddressSanitizer and UndefinedBehaviorSanitizer by tests/test_image_plan.py.
//
// Fake contexts are laid out the way ekf_create allocates one (as tests/cpp/resample_driver.cpp), then
// for every combination of shape, element size, pending steps, live buffers, operand symmetry and
// plane mode
//   * the sections start on 16-byte boundaries and the image has the closed-form number of bytes,
//   * the export table covers every byte of every image exactly once: the sections by copies out of
//     the exported instance's slices, the padding by zero pieces, in pieces of at most RS_CHUNK bytes
//     of a class their addresses allow,
//   * export of instance s followed by import into slot d of the same layout moves the same source
//     bytes to the same destination bytes as resample_plan with src[d] = s,
//   * with the destination's ring position and buffer parity shifted, the buffer the scans read goes
//     to the buffer the destination's scans read, the q-th oldest pending slot to the destination's
//     q-th oldest, the newest record to the destination's newest, and nothing leaves slot d,
//   * the completion words, and only they, travel as re-tag pieces carrying the source's epoch,
//   * the key differs when any keyed field differs and is equal for another E.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <set>
#include <utility>
#include <vector>

#include "ekf_image_plan.h"

using namespace ekf;

namespace {

constexpr int WG0 = 4;   // ekf_kernels.h SYNC_WG0

struct Alloc { uint64_t base, bytes; };
struct Fake {
    ResampleLayout L;
    int elem = 0;
    std::vector<Alloc> allocs;
    uint64_t next = 0;
    uint64_t alloc(uint64_t bytes)
    {
        const uint64_t p = next;
        allocs.push_back({p, bytes});
        next += (bytes + 255) / 256 * 256 + 256;
        return p;
    }
};

[[noreturn]] void fail(const char* what, const char* cfg)
{
    printf("FAILED: %s (%s)\n", what, cfg);
    exit(1);
}

Fake make(uint64_t origin, int N, int E, int elem, int T, int npend, int first, int nX, int usym, int npl, int max_lines = 8)
{
    Fake f;
    f.next = origin;
    f.elem = elem;
    ResampleLayout& L = f.L;
    L.d = make_dims(N, max_lines);
    const Dims& d = L.d;
    L.E = E;
    L.xinst_bytes = (uint64_t)d.ntiles * TILE_ELEMS * (uint64_t)elem;
    L.op_elem = elem == 8 ? 8 : 4;
    L.usym = usym;
    L.npl = npl;
    L.res_stride = 16 + 2 * 64 + 4;
    const int Gmax = (N + 63) / 64;
    L.sync_stride = (4 + Gmax + 15) / 16 * 16;
    L.nX = nX;
    L.X[0] = f.alloc(L.xinst_bytes * E);
    L.X[1] = nX == 2 ? f.alloc(L.xinst_bytes * E) : 0;
    L.Rs = f.alloc(8ull * 3 * d.n * E * 2);
    L.y = f.alloc(8ull * d.n * E * 2);
    L.cur = f.alloc(4ull * E);
    L.pose = f.alloc(24ull * E);
    L.xpre = f.alloc(24ull * E);
    L.saved = f.alloc(4ull * E);
    L.D = f.alloc(8ull * 4 * d.N * E * 2);
    const int R = 2 * T;
    const uint64_t op_inst = (uint64_t)d.nb * 64 * (d.kmax / 2);
    L.slot_bytes = (op_inst * L.op_elem * E + 255) / 256 * 256;
    L.ops_u = f.alloc(L.slot_bytes * R);
    L.ops_v = f.alloc(L.slot_bytes * R);
    L.bslot_bytes = npl ? (op_inst * npl * 2 * E + 255) / 256 * 256 : 0;
    L.ops_b = npl ? f.alloc(L.bslot_bytes * R) : 0;
    L.psig = f.alloc(4ull * E);
    L.pvmax = f.alloc(8ull * E);
    for (int i = 0; i < R; i++) {
        L.patch.push_back(f.alloc(8ull * d.max_lines * 2 * d.M * E));
        L.patch_diag.push_back(f.alloc(8ull * d.max_lines * 4 * E));
        L.res.push_back(f.alloc(4ull * L.res_stride * E));
    }
    L.pexp = f.alloc(4ull * E);
    L.sync = f.alloc(4ull * L.sync_stride * E);
    for (int q = 0; q < npend; q++) L.pending.push_back((first + q) % R);
    // the last step: the newest pending one, or (nothing pending) the slot before `first` (a step was run)
    L.newest = npend > 0 ? (first + npend - 1) % R : (first + R - 1) % R;
    return f;
}

// bytes of one image from the documented shapes, every item padded to 16
uint64_t closed_form(const ResampleLayout& L, int elem)
{
    auto p16 = [](uint64_t b) { return (b + 15) / 16 * 16; };
    const Dims& d = L.d;
    const uint64_t nb = (uint64_t)d.nb, M = (uint64_t)d.M, n = (uint64_t)d.n, N = (uint64_t)d.N;
    uint64_t b = (uint64_t)L.nX * p16((nb * (nb + 1) / 2) * 1024 * (uint64_t)elem);
    b += 2 * (p16(3 * n * 8) + p16(n * 8) + p16(4 * N * 8));
    b += 4 * p16(4) /*cur, saved, pexp, psig*/ + 2 * p16(24) /*pose, xpre*/ + p16(8) /*pvmax*/;
    b += p16(4ull * L.sync_stride);
    const uint64_t rows = nb * 64 * (uint64_t)(d.kmax / 2);
    const uint64_t rec = p16(4ull * (16 + 2 * 64 + 4));
    uint64_t slot = p16(rows * (elem == 8 ? 8 : 4)) * (L.usym ? 1 : 2) + (L.npl ? p16(rows * L.npl * 2) : 0);
    slot += p16(8ull * d.max_lines * 2 * M) + p16(8ull * d.max_lines * 4) + rec;
    b += slot * L.pending.size();
    if (L.pending.empty() && L.newest >= 0) b += rec;
    return b;
}

// a byte map as maximal runs (dst, src, len), sorted by dst
struct Run { uint64_t dst, src, len; };
bool operator==(const Run& a, const Run& b) { return a.dst == b.dst && a.src == b.src && a.len == b.len; }

std::vector<Run> normal(std::vector<Run> r)
{
    std::sort(r.begin(), r.end(), [](const Run& a, const Run& b) { return a.dst < b.dst; });
    std::vector<Run> out;
    for (const Run& x : r) {
        if (!out.empty() && out.back().dst + out.back().len == x.dst && out.back().src + out.back().len == x.src)
            out.back().len += x.len;
        else
            out.push_back(x);
    }
    return out;
}

void check_pieces(const std::vector<CopySeg>& t, const char* cfg)
{
    for (const CopySeg& s : t) {
        const uint32_t cls = s.cls & 0xff;
        if (s.bytes == 0 || s.bytes > RS_CHUNK || s.bytes % 4) fail("a piece's length", cfg);
        if (cls == IMAGE_CLS_ZERO) {
            if (s.dst % 4 || s.bytes >= 16) fail("a zero piece", cfg);
            continue;
        }
        if (cls == IMAGE_CLS_RETAG) {
            if ((s.src | s.dst) % 4) fail("a re-tag piece's alignment", cfg);
            continue;
        }
        if (cls != 4 && cls != 8 && cls != 16) fail("a class", cfg);
        if (s.cls != cls) fail("a copy piece with high bits", cfg);
        if ((s.src | s.dst | s.bytes) % cls) fail("a class wider than its piece's alignment", cfg);
    }
}

// export then import as one byte map from the source context to the destination context
std::vector<Run> compose(const std::vector<CopySeg>& ex, const std::vector<CopySeg>& im, const char* cfg)
{
    std::vector<CopySeg> e;
    for (const CopySeg& s : ex)
        if ((s.cls & 0xff) != IMAGE_CLS_ZERO) e.push_back(s);
    std::sort(e.begin(), e.end(), [](const CopySeg& a, const CopySeg& b) { return a.dst < b.dst; });
    std::vector<Run> out;
    for (const CopySeg& s : im) {
        uint64_t at = s.src, left = s.bytes, to = s.dst;
        while (left) {
            auto it = std::upper_bound(e.begin(), e.end(), at, [](uint64_t v, const CopySeg& a) { return v < a.dst; });
            if (it == e.begin()) fail("an import piece reads before the image", cfg);
            --it;
            if (at >= it->dst + it->bytes) fail("an import piece reads padding or past the image", cfg);
            const uint64_t take = std::min<uint64_t>(left, it->dst + it->bytes - at);
            out.push_back({to, it->src + (at - it->dst), take});
            at += take;
            to += take;
            left -= take;
        }
    }
    return normal(out);
}

void check_export(const Fake& f, int base, const std::vector<int32_t>& inst, uint64_t img, const char* cfg)
{
    const ResampleLayout& L = f.L;
    const std::vector<ResampleArray> arrays = image_arrays(L, base);
    const std::vector<ImageSection> sec = image_sections(arrays);
    const uint64_t per = image_bytes(arrays);
    if (per % 16 || per != closed_form(L, f.elem)) fail("the image's byte count", cfg);
    if (sec.size() != arrays.size()) fail("sections", cfg);
    for (const ImageSection& s : sec)
        if (s.offset % 16 || s.bytes == 0) fail("a section off a 16-byte boundary", cfg);
    const std::vector<CopySeg> t = image_export_plan(arrays, inst.data(), (int)inst.size(), img);
    check_pieces(t, cfg);
    // exact cover of [img, img + K·per): copies on the sections, zeros on the padding
    std::vector<std::pair<uint64_t, uint64_t>> got;
    for (const CopySeg& s : t) got.push_back({s.dst, s.dst + s.bytes});
    std::sort(got.begin(), got.end());
    uint64_t at = img;
    for (const auto& g : got) {
        if (g.first != at) fail("the image is not covered exactly once", cfg);
        at = g.second;
    }
    if (at != img + per * inst.size()) fail("the image is not covered to its end", cfg);
    for (const CopySeg& s : t) {
        const uint64_t k = (s.dst - img) / per, off = (s.dst - img) % per;
        const ImageSection* in = nullptr;
        for (const ImageSection& q : sec)
            if (off >= q.offset && off < q.offset + image_pad16(q.bytes)) in = &q;
        if (!in) fail("a piece outside every section", cfg);
        const uint64_t o = off - in->offset;
        if ((s.cls & 0xff) == IMAGE_CLS_ZERO) {
            if (o < in->bytes || o + s.bytes != image_pad16(in->bytes)) fail("a zero piece off the padding", cfg);
            continue;
        }
        if ((s.cls & 0xff) == IMAGE_CLS_RETAG) fail("a re-tag piece in an export", cfg);
        if (o + s.bytes > in->bytes) fail("a copy into padding", cfg);
        if (s.src != in->base + in->bytes * (uint64_t)inst[k] + o) fail("a piece reads another slice or offset", cfg);
        bool inside = false;
        for (const Alloc& al : f.allocs) inside = inside || (s.src >= al.base && s.src + s.bytes <= al.base + al.bytes);
        if (!inside) fail("a piece reads outside the buffers", cfg);
    }
    // the landmark tiles move 16 bytes per access into a 16-byte aligned image
    if (img % 16 == 0)
        for (const CopySeg& s : t)
            if ((s.dst - img) % per < L.xinst_bytes && s.cls != 16) fail("tiles not 16-byte class", cfg);
}

void check_retag(const Fake& fd, const std::vector<CopySeg>& im, int groups, const std::vector<int32_t>& slots,
                 const std::vector<uint32_t>& epochs, const char* cfg)
{
    const ResampleLayout& L = fd.L;
    std::set<uint64_t> tagged;
    for (const CopySeg& s : im) {
        if ((s.cls & 0xff) != IMAGE_CLS_RETAG) {
            // no copy piece writes a completion word
            for (size_t k = 0; k < slots.size(); k++) {
                const uint64_t lo = L.sync + 4ull * L.sync_stride * slots[k] + 4ull * WG0, hi = lo + 4ull * groups;
                if (groups > 0 && s.dst < hi && s.dst + s.bytes > lo) fail("a copy piece writes a completion word", cfg);
            }
            continue;
        }
        bool found = false;
        for (size_t k = 0; k < slots.size(); k++) {
            const uint64_t lo = L.sync + 4ull * L.sync_stride * slots[k] + 4ull * WG0, hi = lo + 4ull * groups;
            if (s.dst >= lo && s.dst + s.bytes <= hi) {
                found = true;
                if ((s.cls >> 8) != (epochs[k] & 0xffffffu)) fail("a re-tag piece's epoch", cfg);
                for (uint64_t a = s.dst; a < s.dst + s.bytes; a += 4)
                    if (!tagged.insert(a).second) fail("a completion word re-tagged twice", cfg);
            }
        }
        if (!found) fail("a re-tag piece off the completion words", cfg);
    }
    if (tagged.size() != slots.size() * (size_t)std::max(groups, 0)) fail("completion words not re-tagged", cfg);
}

// export of s then import into d of the same layout == resample_plan with src[d] = s
void check_same_layout(const Fake& f, int base, int s, int d, uint64_t img, const char* cfg)
{
    const ResampleLayout& L = f.L;
    const std::vector<ResampleArray> arrays = image_arrays(L, base);
    const int32_t from[1] = {s}, to[1] = {d};
    const uint32_t ep[1] = {0x1234567u};
    const int groups = (L.d.N + 191) / 192;
    const std::vector<CopySeg> ex = image_export_plan(arrays, from, 1, img);
    const std::vector<CopySeg> im = image_import_plan(arrays, L.sync, WG0, groups, to, ep, 1, img);
    check_pieces(im, cfg);
    check_retag(f, im, groups, {d}, {ep[0]}, cfg);
    std::vector<int32_t> src((size_t)L.E);
    for (int e = 0; e < L.E; e++) src[(size_t)e] = e;
    src[(size_t)d] = s;
    std::vector<Run> want;
    for (const CopySeg& p : resample_plan(resample_arrays(L), L.E, src.data())) want.push_back({p.dst, p.src, p.bytes});
    want = normal(want);
    const std::vector<Run> got = compose(ex, im, cfg);
    if (!(got == want)) fail("export + import differs from resample_plan", cfg);
}

// the destination at another ring position and buffer parity
void check_shifted(const Fake& fs, int bs, const Fake& fd, int bd, int s, int d, uint64_t img, const char* cfg)
{
    const ResampleLayout &A = fs.L, &B = fd.L;
    const std::vector<ResampleArray> as = image_arrays(A, bs), ad = image_arrays(B, bd);
    if (as.size() != ad.size()) fail("congruent contexts with section lists of different length", cfg);
    for (size_t i = 0; i < as.size(); i++)
        if (as[i].bytes != ad[i].bytes) fail("congruent contexts with sections of different size", cfg);
    const int32_t from[1] = {s}, to[1] = {d};
    const uint32_t ep[1] = {77u};
    const int groups = (A.d.N + 63) / 64;
    const std::vector<CopySeg> ex = image_export_plan(as, from, 1, img);
    const std::vector<CopySeg> im = image_import_plan(ad, B.sync, WG0, groups, to, ep, 1, img);
    check_pieces(im, cfg);
    check_retag(fd, im, groups, {d}, {ep[0]}, cfg);
    const std::vector<Run> got = compose(ex, im, cfg);
    // expected, from the meaning of the sections (not from image_arrays)
    std::vector<Run> want;
    auto slice = [&](uint64_t a, uint64_t b, uint64_t bytes) { want.push_back({b + bytes * d, a + bytes * s, bytes}); };
    const Dims& dm = A.d;
    const uint64_t E1 = (uint64_t)A.E, E2 = (uint64_t)B.E;
    slice(A.X[A.nX == 2 ? bs : 0], B.X[B.nX == 2 ? bd : 0], A.xinst_bytes);
    if (A.nX == 2) slice(A.X[1 - bs], B.X[1 - bd], A.xinst_bytes);
    const uint64_t strip = 24ull * dm.n, mean = 8ull * dm.n, diag = 32ull * dm.N;
    for (uint64_t cb = 0; cb < 2; cb++) {
        slice(A.Rs + cb * E1 * strip, B.Rs + cb * E2 * strip, strip);
        slice(A.y + cb * E1 * mean, B.y + cb * E2 * mean, mean);
        slice(A.D + cb * E1 * diag, B.D + cb * E2 * diag, diag);
    }
    slice(A.cur, B.cur, 4);
    slice(A.saved, B.saved, 4);
    slice(A.pexp, B.pexp, 4);
    slice(A.psig, B.psig, 4);
    slice(A.pose, B.pose, 24);
    slice(A.xpre, B.xpre, 24);
    slice(A.pvmax, B.pvmax, 8);
    slice(A.sync, B.sync, 4ull * A.sync_stride);
    const uint64_t ob = resample_op_bytes(A), pb = resample_plane_bytes(A);
    if (A.pending.size() != B.pending.size()) fail("pending counts", cfg);
    for (size_t q = 0; q < A.pending.size(); q++) {
        const uint64_t i = (uint64_t)A.pending[q], j = (uint64_t)B.pending[q];
        slice(A.ops_v + i * A.slot_bytes, B.ops_v + j * B.slot_bytes, ob);
        if (!A.usym) slice(A.ops_u + i * A.slot_bytes, B.ops_u + j * B.slot_bytes, ob);
        if (A.npl) slice(A.ops_b + i * A.bslot_bytes, B.ops_b + j * B.bslot_bytes, pb);
        slice(A.patch[i], B.patch[j], 8ull * dm.max_lines * 2 * dm.M);
        slice(A.patch_diag[i], B.patch_diag[j], 8ull * dm.max_lines * 4);
        slice(A.res[i], B.res[j], 4ull * A.res_stride);
    }
    if (A.pending.empty() && A.newest >= 0) slice(A.res[(size_t)A.newest], B.res[(size_t)B.newest], 4ull * A.res_stride);
    if (!(got == normal(want))) fail("a shifted destination takes other bytes", cfg);
    // every write stays inside slot d's slices (normal(want) above lists exactly those) and inside the buffers
    for (const CopySeg& p : im) {
        bool inside = false;
        for (const Alloc& al : fd.allocs) inside = inside || (p.dst >= al.base && p.dst + p.bytes <= al.base + al.bytes);
        if (!inside) fail("an import piece writes outside the buffers", cfg);
    }
}

void check_key()
{
    const ImageConfig c0 = {100, 1, 8, 0, 10, 0, 4, 0, 0.4, 0.024};
    const Fake f = make(0x7f0000010000ull, 80, 4, 4, 4, 3, 0, 1, 1, 0);
    const uint64_t k0 = image_key(f.L, 4, c0);
    if (k0 != image_key(make(0x7e0000010000ull, 80, 8, 4, 4, 1, 5, 1, 1, 0).L, 4, c0)) fail("the key depends on E or the ring", "key");
    std::set<uint64_t> keys{k0};
    auto differs = [&](uint64_t k, const char* what) {
        if (!keys.insert(k).second) fail(what, "key");
    };
    differs(image_key(make(0x7f0000010000ull, 81, 4, 4, 4, 3, 0, 1, 1, 0).L, 4, c0), "N");
    differs(image_key(make(0x7f0000010000ull, 80, 4, 2, 4, 3, 0, 1, 1, 0).L, 2, c0), "element size");
    differs(image_key(make(0x7f0000010000ull, 80, 4, 8, 4, 3, 0, 1, 1, 0).L, 8, c0), "operand size");
    differs(image_key(make(0x7f0000010000ull, 80, 4, 4, 4, 3, 0, 2, 1, 0).L, 4, c0), "nX");
    differs(image_key(make(0x7f0000010000ull, 80, 4, 4, 4, 3, 0, 1, 0, 0).L, 4, c0), "usym");
    differs(image_key(make(0x7f0000010000ull, 80, 4, 4, 4, 3, 0, 1, 1, 2).L, 4, c0), "plane mode 2");
    differs(image_key(make(0x7f0000010000ull, 80, 4, 4, 4, 3, 0, 1, 1, 3).L, 4, c0), "plane mode 3");
    differs(image_key(make(0x7f0000010000ull, 80, 4, 4, 4, 3, 0, 1, 1, 0, 7).L, 4, c0), "max_lines");
    {
        Fake g = make(0x7f0000010000ull, 80, 4, 4, 4, 3, 0, 1, 1, 0);
        g.L.res_stride += 4;
        differs(image_key(g.L, 4, c0), "result stride");
        g.L.res_stride -= 4;
        g.L.sync_stride += 16;
        differs(image_key(g.L, 4, c0), "completion-word stride");
    }
    ImageConfig c = c0;
    c.capacity = 101; differs(image_key(f.L, 4, c), "capacity"); c = c0;
    c.precision = 2; differs(image_key(f.L, 4, c), "precision"); c = c0;
    c.max_lines = 9; differs(image_key(f.L, 4, c), "config max_lines"); c = c0;
    c.r_mode = 1; differs(image_key(f.L, 4, c), "r_mode"); c = c0;
    c.reset_margin = 11; differs(image_key(f.L, 4, c), "reset_margin"); c = c0;
    c.pipeline = 1; differs(image_key(f.L, 4, c), "pipeline"); c = c0;
    c.flush_interval = 5; differs(image_key(f.L, 4, c), "flush_interval"); c = c0;
    c.arith = 2; differs(image_key(f.L, 4, c), "arith"); c = c0;
    c.mahalanobis = 0.5; differs(image_key(f.L, 4, c), "mahalanobis"); c = c0;
    c.encoder_noise = 0.025; differs(image_key(f.L, 4, c), "encoder_noise");
}

void check_retag_word()
{
    const uint32_t src = 77, dst = (1u << 24) + 5;   // (tags wrap mod 2^24)
    const uint32_t w = image_retag((src << 8) | 0xa5u, src, dst);
    if (w != ((5u << 8) | 0xa5u)) fail("a word of the source's epoch", "retag");
    const uint32_t stale = image_retag(((src - 1) << 8) | 0x11u, src, dst);
    if ((stale >> 8) == (dst & 0xffffffu) || (stale >> 8) == ((dst + 1) & 0xffffffu) || (stale & 0xff) != 0x11u)
        fail("a stale word", "retag");
    // a stale word that happens to carry the destination's epoch
    const uint32_t clash = image_retag((5u << 8) | 1u, src, dst);
    if ((clash >> 8) == 5u) fail("a stale word keeps the destination's epoch", "retag");
    if ((image_retag(0u, 0u, 0u) >> 8) != 0u) fail("epoch 0", "retag");
}

}  // namespace

int main()
{
    check_key();
    check_retag_word();
    long cases = 0;
    char cfg[240];
    const int T = 4;
    const uint64_t O1 = 0x7f0000010000ull, O2 = 0x7e0000010000ull, IMG = 0x7d0000000000ull;
    for (int N : {16, 37, 80, 1024})          // nb = 1, 3, 5, 64
        for (int E : {1, 4, 8})
            for (int elem : {2, 4, 8})
                for (int npend : {0, 1, T - 1, 2 * T - 1})
                    for (int nX : {1, 2})
                        for (int usym : {0, 1})
                            for (int npl : {0, 2, 3}) {
                                if (npl && elem == 8) continue;       // split arithmetics: fp32 / fp16 storage
                                if (N == 1024 && (E == 4 || (npend != 0 && npend != 2 * T - 1))) continue;
                                for (int first : {0, 2 * T - 2}) {    // (the pending slots wrap round the ring)
                                    const Fake f = make(O1, N, E, elem, T, npend, first, nX, usym, npl);
                                    if (f.L.d.nb != (N == 16 ? 1 : N == 37 ? 3 : N == 80 ? 5 : 64)) fail("nb", "dims");
                                    for (int base = 0; base < nX; base++) {
                                        snprintf(cfg, sizeof cfg, "N %d E %d elem %d pending %d from %d buffers %d base %d "
                                                 "usym %d planes %d", N, E, elem, npend, first, nX, base, usym, npl);
                                        std::vector<int32_t> all;
                                        for (int e = 0; e < E; e++) all.push_back(E - 1 - e);
                                        all.push_back(0);   // (an export list may repeat an instance)
                                        check_export(f, base, all, IMG, cfg);
                                        check_export(f, base, {E - 1}, IMG + 4, cfg);   // a 4-byte aligned buffer
                                        const int s = E - 1, d = 0;
                                        if (E > 1) {
                                            check_same_layout(f, base, s, d, IMG, cfg);
                                            check_same_layout(f, base, 0, 1, IMG + 8, cfg);
                                        }
                                        // another context: E + 1 instances, the ring 3 slots on, the other parity
                                        const Fake g = make(O2, N, E + 1, elem, T, npend, (first + 3) % (2 * T), nX, usym, npl);
                                        check_shifted(f, base, g, nX == 2 ? 1 - base : 0, s, E, IMG, cfg);
                                        check_shifted(f, base, g, base, 0, 0, IMG, cfg);
                                        cases++;
                                    }
                                }
                            }
    printf("image plan: ok (%ld cases)\n", cases);
    return 0;
}
