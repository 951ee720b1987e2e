// ekf_image_plan.h — the instance image of ekf_export_instances / ekf_import_instances (slam_ekf.h):
// everything an instance owns in a position-independent form, and the copy tables that write it
// from a context and read it into a slot of another. Host only (no HIP include): ekf_copy.hip fills a
// ResampleLayout from the context and hands the tables to launch_image (unit_image.hip);
// tests/cpp/image_driver.cpp checks them on a CPU.
//
// What an instance owns is resample_arrays (ekf_resample_plan.h) and nothing else: the image is that
// list for one instance, each slice a section padded to 16 bytes, with the list put into logical
// order first. resample_arrays already gives the pending ring slots oldest first and the newest
// result record last; only the live landmark buffers come in buffer order there, so image_arrays
// swaps them when the scans read X[1]: the buffer the scans read is section 0 and, on the pipelined
// schedule, the newest flush's output section 1. Two congruent contexts (equal key, pending count and
// has_step) then have lists of equal length and slice sizes, and the import maps section i of the
// image onto array i of the destination, whatever its ring position and buffer parity.
#pragma once

#include <stdint.h>
#include <string.h>

#include <vector>

#include "ekf_resample_plan.h"

namespace ekf {

constexpr uint32_t IMAGE_MAGIC = 0x474d4945u;   // "EIMG"
constexpr uint32_t IMAGE_VERSION = 1;
// CopySeg::cls of the image tables, low 8 bits: 16 / 8 / 4 a copy at that width (as ekf_resample), or
constexpr uint32_t IMAGE_CLS_RETAG = 1;   // completion words re-tagged on the way (bits 31..8: the source's epoch mod 2^24)
constexpr uint32_t IMAGE_CLS_ZERO = 2;    // export: a section's padding, written as zeros (src unused)

inline uint64_t image_pad16(uint64_t b) { return (b + 15) & ~(uint64_t)15; }

// resample_arrays in logical order; base: the landmark buffer the scans read (ekf_ctx::base)
inline std::vector<ResampleArray> image_arrays(const ResampleLayout& L, int base)
{
    if (L.nX == 2 && base == 1) {
        ResampleLayout V = L;
        V.X[0] = L.X[1];
        V.X[1] = L.X[0];
        return resample_arrays(V);
    }
    return resample_arrays(L);
}

// one section of the image: slice `bytes` of array `base`, at `offset` of the image
struct ImageSection {
    uint64_t base, bytes, offset;
};

inline std::vector<ImageSection> image_sections(const std::vector<ResampleArray>& arrays)
{
    std::vector<ImageSection> s;
    uint64_t off = 0;
    for (const ResampleArray& a : arrays) {
        s.push_back({a.base, a.bytes, off});
        off += image_pad16(a.bytes);
    }
    return s;
}

// bytes of one image (a multiple of 16)
inline uint64_t image_bytes(const std::vector<ResampleArray>& arrays)
{
    uint64_t b = 0;
    for (const ResampleArray& a : arrays) b += image_pad16(a.bytes);
    return b;
}

// the ekf_config fields that decide the arithmetic (all but device and instances)
struct ImageConfig {
    int32_t capacity, precision, max_lines, r_mode, reset_margin, pipeline, flush_interval, arith;
    double mahalanobis, encoder_noise;
};

// What two contexts must share for an image of one to fit the other: the layout (Dims, element and
// operand sizes, stored or symmetric U rows, plane mode, record and completion-word strides, live
// buffers) and the configuration. FNV-1a over the fields as 64-bit words; E is not among them.
inline uint64_t image_key(const ResampleLayout& L, int elem, const ImageConfig& cfg)
{
    uint64_t h = 1469598103934665603ull;
    auto mix = [&h](uint64_t v) {
        for (int i = 0; i < 8; i++) {
            h ^= (v >> (8 * i)) & 0xff;
            h *= 1099511628211ull;
        }
    };
    uint64_t mah, enc;
    memcpy(&mah, &cfg.mahalanobis, 8);
    memcpy(&enc, &cfg.encoder_noise, 8);
    const Dims& d = L.d;
    const int64_t f[] = {(int64_t)IMAGE_VERSION, d.N, d.n, d.M, d.nb, d.ntiles, d.max_lines, d.kmax, elem, L.op_elem,
                         L.usym, L.npl, L.res_stride, L.sync_stride, L.nX, (int64_t)L.xinst_bytes, cfg.capacity,
                         cfg.precision, cfg.max_lines, cfg.r_mode, cfg.reset_margin, cfg.pipeline, cfg.flush_interval,
                         cfg.arith};
    for (int64_t v : f) mix((uint64_t)v);
    mix(mah);
    mix(enc);
    return h;
}

inline void image_pieces(std::vector<CopySeg>& t, uint64_t src, uint64_t dst, uint64_t bytes, uint32_t chunk)
{
    const uint32_t cls = resample_class(src, dst, bytes);
    for (uint64_t off = 0; off < bytes; off += chunk) {
        const uint64_t len = bytes - off < chunk ? bytes - off : chunk;
        t.push_back(CopySeg{src + off, dst + off, (uint32_t)len, cls});
    }
}

// Export: image k (at img + k·image_bytes) takes instance inst[k]'s slice of every array, and zeros
// in the padding. Raw: no byte of a section is changed. inst entries in [0, E); duplicates allowed.
inline std::vector<CopySeg> image_export_plan(const std::vector<ResampleArray>& arrays, const int32_t* inst, int K,
                                              uint64_t img, uint32_t chunk = RS_CHUNK)
{
    std::vector<CopySeg> t;
    const std::vector<ImageSection> sec = image_sections(arrays);
    const uint64_t per = image_bytes(arrays);
    for (int k = 0; k < K; k++)
        for (const ImageSection& s : sec) {
            const uint64_t q = img + (uint64_t)k * per + s.offset;
            image_pieces(t, s.base + (uint64_t)inst[k] * s.bytes, q, s.bytes, chunk);
            const uint64_t pad = image_pad16(s.bytes) - s.bytes;
            if (pad) t.push_back(CopySeg{0, q + s.bytes, (uint32_t)pad, IMAGE_CLS_ZERO});
        }
    return t;
}

// Import: slot inst[k] of the destination (its arrays, in logical order) takes image k. The
// completion words — words [wg0, wg0 + groups) of the slice of the array at `sync` — are one piece
// of class IMAGE_CLS_RETAG carrying the source's epoch epoch[k]; the words around them are copies.
// inst entries distinct and in [0, E).
inline std::vector<CopySeg> image_import_plan(const std::vector<ResampleArray>& arrays, uint64_t sync, int wg0, int groups,
                                              const int32_t* inst, const uint32_t* epoch, int K, uint64_t img,
                                              uint32_t chunk = RS_CHUNK)
{
    std::vector<CopySeg> t;
    const std::vector<ImageSection> sec = image_sections(arrays);
    const uint64_t per = image_bytes(arrays);
    for (int k = 0; k < K; k++)
        for (const ImageSection& s : sec) {
            const uint64_t p = img + (uint64_t)k * per + s.offset, q = s.base + (uint64_t)inst[k] * s.bytes;
            if (s.base != sync || groups <= 0) {
                image_pieces(t, p, q, s.bytes, chunk);
                continue;
            }
            const uint64_t lo = 4 * (uint64_t)wg0, hi = 4 * (uint64_t)(wg0 + groups);
            if (lo) image_pieces(t, p, q, lo, chunk);
            for (uint64_t off = lo; off < hi; off += chunk) {
                const uint64_t len = hi - off < chunk ? hi - off : chunk;
                t.push_back(CopySeg{p + off, q + off, (uint32_t)len, IMAGE_CLS_RETAG | ((epoch[k] & 0xffffffu) << 8)});
            }
            if (hi < s.bytes) image_pieces(t, p + hi, q + hi, s.bytes - hi, chunk);
        }
    return t;
}

// A completion word of an image on its way into a context at epoch `dst` (ekf_commit.h: bits 31..8
// the launch epoch mod 2^24, 7..0 status and flags). A word of the source's last launch becomes one
// of the destination's last launch; any other (a workgroup that never finished) becomes one of the
// launch before it, which no reader takes for the last launch's and no later launch can carry.
EKF_HD uint32_t image_retag(uint32_t word, uint32_t src_epoch, uint32_t dst_epoch)
{
    const uint32_t tag = (word >> 8) == (src_epoch & 0xffffffu) ? dst_epoch : dst_epoch - 1u;
    return ((tag & 0xffffffu) << 8) | (word & 0xffu);
}

}  // namespace ekf
