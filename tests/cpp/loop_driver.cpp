// loop_driver.cpp — the host-callable parts of the hypothesis loop on a CPU (csrc/ekf_loop_plan.h,
// resample_pieces of csrc/ekf_resample_plan.h): a stand-alone program, built with AddressSanitizer and
// UndefinedBehaviorSanitizer by tests/test_loop_plan.py.
//
//   loop_driver --sizeof   sizeof(ekf_plan_info) and its field offsets
//   loop_driver --pieces   resample_pieces against resample_plan: on fake contexts laid out the way
//                          ekf_create allocates one (resample_driver.cpp's shapes: odd n, two live buffers,
//                          pending slots that wrap round the ring) and several valid lists, the pieces
//                          expanded with the list give exactly resample_plan's multiset of
//                          {src, dst, bytes, cls}
//   loop_driver --lists    resample_list_code against resample_check on every list over E = 4
//   loop_driver --plan     reads cases "E u ess_below w_0 .. w_{E-1}" (hex floats) from stdin and prints
//                          "status copies ess total src_0 .. src_{E-1}" per case (ess, total as hex floats)
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <tuple>
#include <vector>

#include "ekf_loop_plan.h"
#include "ekf_resample_plan.h"

using namespace ekf;

namespace {

[[noreturn]] void fail(const char* what, const char* cfg)
{
    printf("FAILED: %s (%s)\n", what, cfg);
    exit(1);
}

struct Fake {
    ResampleLayout L;
    uint64_t next = 0x7f0000010000ull;
    uint64_t alloc(uint64_t bytes)
    {
        const uint64_t p = next;
        next += (bytes + 255) / 256 * 256 + 256;
        return p;
    }
};

// (the layout of resample_driver.cpp's fake context)
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
    L.newest = npend > 0 ? (first + npend - 1) % R : (first > 0 ? first - 1 : -1);
    return f;
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

typedef std::tuple<uint64_t, uint64_t, uint32_t, uint32_t> Seg;

long check_pieces(const Fake& f, const std::vector<int32_t>& src, const char* cfg)
{
    const int E = f.L.E;
    const std::vector<ResampleArray> arrays = resample_arrays(f.L);
    const std::vector<CopyPiece> pieces = resample_pieces(arrays);
    uint64_t per = 0;
    for (const CopyPiece& p : pieces) {
        if (p.len == 0 || p.len > RS_CHUNK || p.off + p.len > p.slice) fail("a piece leaves its slice", cfg);
        if (p.cls != 4 && p.cls != 8 && p.cls != 16) fail("a class", cfg);
        if ((p.base | p.slice | p.off | p.len) % p.cls) fail("a class wider than its piece's alignment", cfg);
        per += p.len;
    }
    if (per != resample_bytes_per_instance(f.L)) fail("the pieces of one instance are not its bytes", cfg);
    // what the kernel does with them: every piece for every overwritten instance
    std::vector<Seg> got, want;
    for (int e = 0; e < E; e++) {
        if (src[e] == e) continue;
        for (const CopyPiece& p : pieces)
            got.push_back(Seg(p.base + (uint64_t)src[e] * p.slice + p.off, p.base + (uint64_t)e * p.slice + p.off, p.len,
                              p.cls));
    }
    for (const CopySeg& s : resample_plan(arrays, E, src.data())) want.push_back(Seg(s.src, s.dst, s.bytes, s.cls));
    std::sort(got.begin(), got.end());
    std::sort(want.begin(), want.end());
    if (got != want) fail("the expanded pieces are not resample_plan's table", cfg);
    return (long)got.size();
}

int run_pieces()
{
    long cases = 0, segs = 0;
    char cfg[200];
    const int T = 4;
    for (int N : {16, 37, 80, 1024})          // nb = 1, 3, 5, 64; N = 37: an odd n
        for (int E : {1, 4, 8})
            for (int elem : {2, 4, 8})
                for (int npend : {0, 1, T - 1, 2 * T - 1})
                    for (int nX : {1, 2})
                        for (int usym : {0, 1})
                            for (int npl : {0, 2, 3}) {
                                if (npl && elem == 8) continue;
                                if (N == 1024 && (E == 4 || (npend != 0 && npend != 2 * T - 1))) continue;
                                for (int first : {0, 2 * T - 2}) {
                                    const Fake f = make(N, E, elem, T, npend, first, nX, usym, npl);
                                    int li = 0;
                                    for (const auto& src : lists(E)) {
                                        snprintf(cfg, sizeof cfg, "N %d E %d elem %d pending %d from %d buffers %d usym %d "
                                                 "planes %d list %d", N, E, elem, npend, first, nX, usym, npl, li++);
                                        if (resample_list_code(src.data(), E) != 0) fail("a valid list refused", cfg);
                                        segs += check_pieces(f, src, cfg);
                                        cases++;
                                    }
                                }
                            }
    printf("resample pieces: ok (%ld cases, %ld entries)\n", cases, segs);
    return 0;
}

int run_lists()
{
    int32_t s[4];
    int n = 0, refused = 0;
    for (s[0] = -1; s[0] <= 4; s[0]++)      // every list over [0, 4), and entries just outside it
        for (s[1] = -1; s[1] <= 4; s[1]++)
            for (s[2] = -1; s[2] <= 4; s[2]++)
                for (s[3] = -1; s[3] <= 4; s[3]++) {
                    const int a = resample_list_code(s, 4), b = resample_check(s, 4);
                    if (a != b) {
                        printf("FAILED: list %d %d %d %d: %d, resample_check %d\n", s[0], s[1], s[2], s[3], a, b);
                        return 1;
                    }
                    const int st = resample_code_status(a);
                    if (st != (b == 2 ? EKF_ERANGE : b == 1 ? EKF_EINVAL : EKF_OK)) return 1;
                    n++;
                    refused += a != 0;
                }
    printf("resample lists: ok (%d lists, %d refused)\n", n, refused);
    return 0;
}

int run_plan()
{
    int E;
    while (scanf("%d", &E) == 1) {
        double u, below;
        if (E < 1 || E > (1 << 20) || scanf("%la %la", &u, &below) != 2) return 2;
        std::vector<double> w((size_t)E);
        std::vector<int32_t> src((size_t)E, -7);
        for (int e = 0; e < E; e++)
            if (scanf("%la", &w[(size_t)e]) != 1) return 2;
        ekf_plan_info info;
        memset(&info, 0x5a, sizeof info);
        resample_plan_sequential(w.data(), E, u, below, src.data(), &info);
        std::vector<int32_t> again((size_t)E, -7);
        resample_plan_sequential(w.data(), E, u, below, again.data(), nullptr);   // (info may be null)
        if (again != src) return 3;
        printf("%d %d %a %a", info.status, info.copies, info.ess, info.total);
        for (int e = 0; e < E; e++) printf(" %d", src[(size_t)e]);
        printf("\n");
    }
    return 0;
}

}  // namespace

int main(int argc, char** argv)
{
    const char* mode = argc > 1 ? argv[1] : "";
    if (!strcmp(mode, "--sizeof")) {
        printf("%zu %zu %zu %zu %zu\n", sizeof(ekf_plan_info), offsetof(ekf_plan_info, status),
               offsetof(ekf_plan_info, copies), offsetof(ekf_plan_info, ess), offsetof(ekf_plan_info, total));
        return 0;
    }
    if (!strcmp(mode, "--pieces")) return run_pieces();
    if (!strcmp(mode, "--lists")) return run_lists();
    if (!strcmp(mode, "--plan")) return run_plan();
    fprintf(stderr, "usage: loop_driver --sizeof | --pieces | --lists | --plan < cases\n");
    return 64;
}
