// ekf_resample_plan.h — the copy table of ekf_resample (slam_ekf.h): which bytes instance e takes
// from instance src[e]. Host only (no HIP include): ekf_copy.hip fills a ResampleLayout from the
// context and hands the table to launch_resample (unit_resample.hip); tests/cpp/resample_driver.cpp
// checks it on a CPU. ekf_resample_device, whose list is device memory, takes resample_pieces instead:
// the same arrays cut into the same pieces, without the instances (kernel: unit_resample_device.hip;
// checked by tests/cpp/loop_driver.cpp).
//
// Everything an instance owns is a slice of an array laid out [E][slice] (the two copies of the
// robot strip, the mean and the diagonal blocks are two such arrays each), so the state of an
// instance is a list of (base, slice bytes) and a resample is, per array and per overwritten
// instance, one copy of a slice onto the slice at the same offset of another instance. Sources are
// fixed points of src (src[src[e]] == src[e]): no slice is both read and written, so the copies need
// no order among themselves and one launch does them all.
#pragma once

#include <stdint.h>

#include <vector>

#include "ekf_layout.h"

namespace ekf {

// one piece of a copy: at most RS_CHUNK bytes; cls is the widest access (16, 8 or 4 bytes) that
// divides both addresses and the length
struct CopySeg {
    uint64_t src, dst;
    uint32_t bytes;
    uint32_t cls;
};
constexpr uint32_t RS_CHUNK = 16384;   // 256 lanes × 16 bytes × 4 loads in flight

// an array of E per-instance slices, `bytes` apart and long
struct ResampleArray {
    uint64_t base;
    uint64_t bytes;
};

// what of a context holds per-instance state (addresses as integers)
struct ResampleLayout {
    Dims d;
    int E;
    uint64_t xinst_bytes;     // stored landmark-block bytes per instance
    int op_elem;              // bytes per operand element
    int usym;                 // symmetric operands: the U rows are not stored
    int npl;                  // operand planes per element: 0 (EKF_ARITH_EXACT), 2 (F16X3), 3 (BF16X6)
    int res_stride;           // ints per result record
    int sync_stride;          // ints per instance of the completion words
    int nX;                   // live landmark-block buffers: 1, or 2 on the pipelined schedule
    uint64_t X[2];
    uint64_t Rs, y, D;        // [2][E][3][n], [2][E][n], [2][E][N][4] doubles
    uint64_t cur, saved, pexp, psig;   // [E] ints
    uint64_t pose, xpre;      // [E][3] doubles
    uint64_t pvmax;           // [E] doubles
    uint64_t sync;            // [E][sync_stride] ints
    uint64_t ops_u, ops_v, ops_b;      // operand rows / planes of ring slot i at base + i·slot bytes
    uint64_t slot_bytes, bslot_bytes;
    std::vector<uint64_t> patch, patch_diag, res;   // per ring slot
    std::vector<int> pending; // ring slots of the steps not yet in the block the scans read
    int newest;               // ring slot of the last step (its result record), −1: no step yet
};

// operand bytes per instance and slot: rows [nb][64][kmax/2], planes [nb][npl][64][8] of 2 bytes
inline uint64_t resample_op_bytes(const ResampleLayout& L)
{
    return (uint64_t)L.d.nb * 64 * (L.d.kmax / 2) * (uint64_t)L.op_elem;
}
inline uint64_t resample_plane_bytes(const ResampleLayout& L)
{
    return (uint64_t)L.d.nb * 64 * (L.d.kmax / 2) * (uint64_t)L.npl * 2;
}

// 0: acceptable; 1: a source that is itself overwritten (or no list); 2: an entry outside [0, E)
inline int resample_check(const int32_t* src, int E)
{
    if (!src) return 1;
    for (int e = 0; e < E; e++)
        if (src[e] < 0 || src[e] >= E) return 2;
    for (int e = 0; e < E; e++)
        if (src[src[e]] != src[e]) return 1;
    return 0;
}

// every array of per-instance slices the kernels read later
inline std::vector<ResampleArray> resample_arrays(const ResampleLayout& L)
{
    const Dims& d = L.d;
    const uint64_t E = (uint64_t)L.E, f64 = sizeof(double), i32 = sizeof(int32_t);
    std::vector<ResampleArray> a;
    for (int k = 0; k < L.nX; k++) a.push_back({L.X[k], L.xinst_bytes});
    const uint64_t strip = 3 * (uint64_t)d.n * f64, mean = (uint64_t)d.n * f64, diag = 4 * (uint64_t)d.N * f64;
    for (uint64_t cb = 0; cb < 2; cb++) {   // both copies and the selector: cur is not read back
        a.push_back({L.Rs + cb * E * strip, strip});
        a.push_back({L.y + cb * E * mean, mean});
        a.push_back({L.D + cb * E * diag, diag});
    }
    a.push_back({L.cur, i32});
    a.push_back({L.saved, i32});
    a.push_back({L.pexp, i32});
    a.push_back({L.psig, i32});
    a.push_back({L.pose, 3 * f64});
    a.push_back({L.xpre, 3 * f64});
    a.push_back({L.pvmax, f64});
    a.push_back({L.sync, (uint64_t)L.sync_stride * i32});
    const uint64_t ob = resample_op_bytes(L), pb = resample_plane_bytes(L);
    bool newest_pending = false;
    for (int s : L.pending) {
        const uint64_t i = (uint64_t)s;
        a.push_back({L.ops_v + i * L.slot_bytes, ob});
        if (!L.usym) a.push_back({L.ops_u + i * L.slot_bytes, ob});
        if (L.npl) a.push_back({L.ops_b + i * L.bslot_bytes, pb});
        a.push_back({L.patch[i], (uint64_t)d.max_lines * 2 * (uint64_t)d.M * f64});
        a.push_back({L.patch_diag[i], (uint64_t)d.max_lines * 4 * f64});
        a.push_back({L.res[i], (uint64_t)L.res_stride * i32});
        newest_pending = newest_pending || s == L.newest;
    }
    if (L.newest >= 0 && !newest_pending) a.push_back({L.res[(size_t)L.newest], (uint64_t)L.res_stride * i32});
    return a;
}

// bytes one overwritten instance receives (the closed form the driver checks the table against)
inline uint64_t resample_bytes_per_instance(const ResampleLayout& L)
{
    const Dims& d = L.d;
    const uint64_t rec = (uint64_t)L.res_stride * 4;
    uint64_t b = (uint64_t)L.nX * L.xinst_bytes + 2 * 8 * (3 * (uint64_t)d.n + (uint64_t)d.n + 4 * (uint64_t)d.N);
    b += 4 * 4 + 2 * 24 + 8 + (uint64_t)L.sync_stride * 4;
    const uint64_t slot = resample_op_bytes(L) * (L.usym ? 1 : 2) + resample_plane_bytes(L) +
                          8 * (uint64_t)d.max_lines * (2 * (uint64_t)d.M + 4) + rec;
    b += slot * L.pending.size();
    bool newest_pending = false;
    for (int s : L.pending) newest_pending = newest_pending || s == L.newest;
    if (L.newest >= 0 && !newest_pending) b += rec;
    return b;
}

inline uint32_t resample_class(uint64_t src, uint64_t dst, uint64_t bytes)
{
    const uint64_t m = src | dst | bytes;
    return (m & 15) == 0 ? 16u : (m & 7) == 0 ? 8u : 4u;
}

// The table: for every e with src[e] != e and every array, slice src[e] onto slice e, in pieces of at
// most `chunk` bytes (a multiple of 16, so a piece keeps the class of its copy). The identity list
// gives an empty table. src must pass resample_check.
inline std::vector<CopySeg> resample_plan(const std::vector<ResampleArray>& arrays, int E, const int32_t* src,
                                          uint32_t chunk = RS_CHUNK)
{
    std::vector<CopySeg> t;
    size_t pieces = 0, ndst = 0;
    for (const ResampleArray& a : arrays) pieces += (size_t)((a.bytes + chunk - 1) / chunk);
    for (int e = 0; e < E; e++) ndst += src[e] != e;
    t.reserve(pieces * ndst);
    for (int e = 0; e < E; e++) {
        if (src[e] == e) continue;
        for (const ResampleArray& a : arrays) {
            const uint64_t s = a.base + (uint64_t)src[e] * a.bytes, q = a.base + (uint64_t)e * a.bytes;
            const uint32_t cls = resample_class(s, q, a.bytes);
            for (uint64_t off = 0; off < a.bytes; off += chunk) {
                const uint64_t len = a.bytes - off < chunk ? a.bytes - off : chunk;
                t.push_back(CopySeg{s + off, q + off, (uint32_t)len, cls});
            }
        }
    }
    return t;
}

// ekf_resample_device's table: the list lives on the device, so the host lists the pieces of one
// instance's slices and the kernel applies each to every (src[e], e) it finds: bytes [off, off + len) of
// slice src[e] of the array at `base` onto the same bytes of slice e. cls comes from base | slice, which is
// resample_class for every pair of instances (the slice length enters both, and with it every distance
// between two slices).
struct CopyPiece {
    uint64_t base, slice;   // the array and its bytes per instance
    uint64_t off;           // of the piece in the slice
    uint32_t len;           // at most `chunk`
    uint32_t cls;
};

inline std::vector<CopyPiece> resample_pieces(const std::vector<ResampleArray>& arrays, uint32_t chunk = RS_CHUNK)
{
    std::vector<CopyPiece> t;
    size_t pieces = 0;
    for (const ResampleArray& a : arrays) pieces += (size_t)((a.bytes + chunk - 1) / chunk);
    t.reserve(pieces);
    for (const ResampleArray& a : arrays) {
        const uint32_t cls = resample_class(a.base, a.base, a.bytes);
        for (uint64_t off = 0; off < a.bytes; off += chunk) {
            const uint64_t len = a.bytes - off < chunk ? a.bytes - off : chunk;
            t.push_back(CopyPiece{a.base, a.bytes, off, (uint32_t)len, cls});
        }
    }
    return t;
}

}  // namespace ekf
