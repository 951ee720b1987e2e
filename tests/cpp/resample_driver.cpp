// resample_driver.cpp — ekf_resample's copy table (csrc/ekf_resample_plan.h) on a CPU: a stand-alone
// program, built with AddressSanitizer and UndefinedBehaviorSanitizer by tests/test_resample_plan.py.
//
// A fake context is laid out the way ekf_create allocates one (256-byte aligned buffers, the ring
// slots' operand rows a fixed stride apart), then for every combination of shape, element size,
// pending steps, live buffers, operand symmetry, plane mode and source list the table must
//   * cover every byte of every overwritten instance's slices exactly once,
//   * read no byte that any entry writes,
//   * read, for instance e, only instance src[e]'s slice of the same array at the same offset,
//   * stay inside the buffers, in pieces of at most RS_CHUNK bytes of the widest class that fits,
//   * move the closed-form number of bytes, and be empty for the identity list.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "ekf_resample_plan.h"

using namespace ekf;

namespace {

struct Alloc { uint64_t base, bytes; };
struct Fake {
    ResampleLayout L;
    std::vector<Alloc> allocs;
    uint64_t next = 0x7f0000010000ull;
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

Fake make(int N, int E, int elem, int T, int npend, int first, int nX, int usym, int npl)
{
    Fake f;
    ResampleLayout& L = f.L;
    L.d = make_dims(N, 8);
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
    // the last step: the newest pending one, or (nothing pending) the slot before `first`; −1 at the start
    L.newest = npend > 0 ? (first + npend - 1) % R : (first > 0 ? first - 1 : -1);
    return f;
}

// the bytes one overwritten instance receives, from the documented shapes (not from the header's sum)
uint64_t closed_form(const ResampleLayout& L, int elem)
{
    const Dims& d = L.d;
    const uint64_t nb = (uint64_t)d.nb, M = (uint64_t)d.M, n = (uint64_t)d.n, N = (uint64_t)d.N;
    uint64_t b = (uint64_t)L.nX * (nb * (nb + 1) / 2) * 1024 * (uint64_t)elem;   // the packed tiles
    b += 2 * (3 * n + n + 4 * N) * 8;                                            // strip, mean, diagonal blocks, twice
    b += 4 /*cur*/ + 4 /*saved*/ + 4 /*pexp*/ + 4 /*psig*/ + 8 /*pvmax*/ + 24 + 24 /*pose, xpre*/;
    b += 4ull * L.sync_stride;
    const uint64_t rows = nb * 64 * (uint64_t)(d.kmax / 2);
    const uint64_t rec = 4ull * (16 + 2 * 64 + 4);
    uint64_t slot = rows * (elem == 8 ? 8 : 4) * (L.usym ? 1 : 2) + rows * L.npl * 2;
    slot += 8ull * d.max_lines * 2 * M + 8ull * d.max_lines * 4 + rec;
    b += slot * L.pending.size();
    if (L.pending.empty() && L.newest >= 0) b += rec;
    return b;
}

void check(const Fake& f, int elem, const std::vector<int32_t>& src, const char* cfg)
{
    const ResampleLayout& L = f.L;
    const int E = L.E;
    if (resample_check(src.data(), E) != 0) fail("an acceptable list was refused", cfg);
    const std::vector<ResampleArray> arrays = resample_arrays(L);
    // every array lies inside one buffer, and no two arrays overlap
    std::vector<std::pair<uint64_t, uint64_t>> spans;
    for (const ResampleArray& a : arrays) {
        bool inside = false;
        for (const Alloc& al : f.allocs)
            inside = inside || (a.base >= al.base && a.base + a.bytes * E <= al.base + al.bytes);
        if (!inside || a.bytes == 0 || a.bytes % 4) fail("an array leaves its buffer", cfg);
        spans.push_back({a.base, a.base + a.bytes * E});
    }
    std::sort(spans.begin(), spans.end());
    for (size_t i = 1; i < spans.size(); i++)
        if (spans[i - 1].second > spans[i].first) fail("two arrays overlap", cfg);

    const std::vector<CopySeg> t = resample_plan(arrays, E, src.data());
    int ndst = 0;
    for (int e = 0; e < E; e++) ndst += src[e] != e;
    if (ndst == 0) {
        if (!t.empty()) fail("the identity list gives entries", cfg);
        return;
    }
    // expected destination ranges
    std::vector<std::pair<uint64_t, uint64_t>> want, got, reads;
    for (const ResampleArray& a : arrays)
        for (int e = 0; e < E; e++)
            if (src[e] != e) want.push_back({a.base + a.bytes * e, a.base + a.bytes * (e + 1)});
    uint64_t total = 0;
    for (const CopySeg& s : t) {
        if (s.bytes == 0 || s.bytes > RS_CHUNK) fail("a piece's length", cfg);
        if (s.cls != 4 && s.cls != 8 && s.cls != 16) fail("a class", cfg);
        const uint64_t m = s.src | s.dst | s.bytes;
        if (m % s.cls) fail("a class wider than its piece's alignment", cfg);
        total += s.bytes;
        // its array, instance and offset
        const ResampleArray* ar = nullptr;
        for (const ResampleArray& a : arrays)
            if (s.dst >= a.base && s.dst < a.base + a.bytes * E) ar = &a;
        if (!ar) fail("a destination outside every array", cfg);
        const uint64_t e = (s.dst - ar->base) / ar->bytes, off = (s.dst - ar->base) % ar->bytes;
        if (src[e] == (int32_t)e) fail("an entry writes an instance that keeps its state", cfg);
        if (off + s.bytes > ar->bytes) fail("a piece crosses its slice", cfg);
        if (s.src != ar->base + ar->bytes * (uint64_t)src[e] + off) fail("a piece reads another slice or offset", cfg);
        // the class is that of the whole copy (the widest that fits it), so equal for all its pieces
        const uint64_t whole = (ar->base + ar->bytes * (uint64_t)src[e]) | (ar->base + ar->bytes * e) | ar->bytes;
        const uint32_t cls = whole % 16 == 0 ? 16 : whole % 8 == 0 ? 8 : 4;
        if (s.cls != cls) fail("a narrower class than the copy allows", cfg);
        got.push_back({s.dst, s.dst + s.bytes});
        reads.push_back({s.src, s.src + s.bytes});
    }
    // known classes: the packed tiles and the records move 16 bytes per access; a strip row block of
    // 3n doubles, n odd, between instances an odd distance apart only 8; the selector 4
    for (const CopySeg& s : t) {
        if (s.dst >= L.X[0] && s.dst < L.X[0] + L.xinst_bytes * E && s.cls != 16) fail("tiles not 16-byte class", cfg);
        if (s.dst >= L.cur && s.dst < L.cur + 4ull * E && (s.cls != 4 || s.bytes != 4)) fail("selector class", cfg);
        const uint64_t strip = 8ull * 3 * L.d.n;
        if (s.dst >= L.Rs && s.dst < L.Rs + strip * E) {
            const uint64_t e = (s.dst - L.Rs) / strip;
            if (((e ^ (uint64_t)src[e]) & 1) && s.cls != 8) fail("strip class", cfg);
        }
    }
    // exact cover: sorted, the pieces tile the expected ranges
    std::sort(want.begin(), want.end());
    std::sort(got.begin(), got.end());
    size_t g = 0;
    for (const auto& w : want) {
        uint64_t at = w.first;
        while (g < got.size() && got[g].first == at && got[g].second <= w.second) at = got[g++].second;
        if (at != w.second) fail("a destination range is not covered exactly once", cfg);
    }
    if (g != got.size()) fail("pieces outside the destination ranges, or twice", cfg);
    // no read touches a written byte
    std::sort(reads.begin(), reads.end());
    size_t r = 0;
    for (const auto& w : want) {
        while (r < reads.size() && reads[r].second <= w.first) r++;
        if (r < reads.size() && reads[r].first < w.second) fail("a source range meets a destination range", cfg);
    }
    const uint64_t per = closed_form(L, elem);
    if (per != resample_bytes_per_instance(L)) fail("the header's byte count", cfg);
    if (total != per * (uint64_t)ndst) fail("the total bytes", cfg);
}

std::vector<std::vector<int32_t>> lists(int E)
{
    std::vector<int32_t> id(E);
    for (int e = 0; e < E; e++) id[e] = e;
    std::vector<std::vector<int32_t>> out{id};
    if (E == 1) return out;
    std::vector<int32_t> a = id;
    a[E - 1] = 0;                        // one copy
    out.push_back(a);
    a = id;
    a[0] = 1;                            // onto instance 0, an odd distance
    out.push_back(a);
    std::vector<int32_t> all(E, E - 2);  // one survivor, duplicated E − 1 times
    out.push_back(all);
    if (E >= 4) {
        a = id;                          // two survivors with surplus copies, one untouched instance
        a[1] = 0;
        a[3] = 2;
        if (E >= 8) { a[4] = 0; a[6] = 2; a[7] = 2; }
        out.push_back(a);
    }
    return out;
}

}  // namespace

int main()
{
    // the list check
    {
        const int32_t ok[4] = {0, 0, 2, 0}, chain[4] = {1, 2, 2, 3}, swap[2] = {1, 0}, past[4] = {0, 4, 2, 3},
                      neg[4] = {0, -1, 2, 3}, both[4] = {1, 2, 2, 7};
        if (resample_check(ok, 4) != 0 || resample_check(chain, 4) != 1 || resample_check(swap, 2) != 1 ||
            resample_check(past, 4) != 2 || resample_check(neg, 4) != 2 || resample_check(both, 4) != 2 ||
            resample_check(nullptr, 4) != 1)
            fail("resample_check", "lists");
    }
    long cases = 0;
    char cfg[200];
    const int T = 4;
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
                                    const Fake f = make(N, E, elem, T, npend, first, nX, usym, npl);
                                    if (f.L.d.nb != (N == 16 ? 1 : N == 37 ? 3 : N == 80 ? 5 : 64)) fail("nb", "dims");
                                    int li = 0;
                                    for (const auto& src : lists(E)) {
                                        snprintf(cfg, sizeof cfg, "N %d E %d elem %d pending %d from %d buffers %d usym %d "
                                                 "planes %d list %d", N, E, elem, npend, first, nX, usym, npl, li++);
                                        check(f, elem, src, cfg);
                                        cases++;
                                    }
                                }
                            }
    printf("resample plan: ok (%ld cases)\n", cases);
    return 0;
}
