// ekf_tables.h — the flush kernels' tile tables as pure host functions of nb (tile rows of the
// landmark block) and a rank's tile-row range. Host only (no HIP include): ekf_api.hip uploads
// them at context creation; tests/cpp/tables_driver.cpp checks them on a CPU. The kernels walk
// these tables in order and load / store the tiles they name, so order and content are part of the
// kernels' contract.
#pragma once

#include <algorithm>
#include <vector>

#include "ekf_layout.h"

namespace ekf {

constexpr int WT_R = 2, WT_C = 2, WT_N = WT_R * WT_C;   // f32 wave flush: tiles per wave-tile
constexpr int WT64_C = 2;                                 // f64 wave flush: 1 × 2 tiles per wave-tile
constexpr int DD_SB = 4;   // f32 flush: tiles per super-tile side (one wave per tile row)

// one wave-tile of the wave flush (host-built table, read with scalar loads): the linear indices
// of its WT_N tiles (positions below the diagonal or past the block point at a stored tile of
// the same wave-tile and are not written back), their validity, the operand row blocks of its
// WT_R tile rows and WT_C tile columns (16 bits each, clamped to the block) and (wr, wc)
struct alignas(32) WtEntry {
    int tile[WT_N];
    int valid;      // bit i: tile i is stored
    int rows[2];    // [0]: A row blocks (WT_R × 16 bits), [1]: B row blocks (WT_C × 16 bits)
    int rc;         // wr | wc << 16
};

struct TileRC { int x, y; };   // a (row, column) pair, laid out as the kernels' int2

// One packed-tile-row partition of the landmark block over `world` ranks: boundaries on even tile
// rows (whole wave-tile rows of the flush) balancing the tiles per rank; rank's rows [r0, r1)
inline void tile_partition(int nb, int world, int rank, int& r0, int& r1)
{
    const long long total = (long long)nb * (nb + 1) / 2;
    auto boundary = [&](int k) {
        if (k <= 0) return 0;
        if (k >= world) return nb;
        // the even tile row whose prefix of tiles is closest to k/world of them
        const long long want = total * k / world;
        int bi = 0;
        while (bi + 2 < nb && tile_index(bi + 2, bi + 2, nb) <= want) bi += 2;
        if (bi + 2 < nb && tile_index(bi + 2, bi + 2, nb) - want < want - tile_index(bi, bi, nb)) bi += 2;
        return bi;
    };
    r0 = boundary(rank);
    r1 = boundary(rank + 1);
}

// [ntiles] (bi, bj) of every stored tile, by its linear index
inline std::vector<TileRC> tile_rc_table(int nb)
{
    std::vector<TileRC> t((size_t)nb * (nb + 1) / 2);
    for (int bi = 0; bi < nb; bi++)
        for (int bj = bi; bj < nb; bj++) t[(size_t)tile_index(bi, bj, nb)] = TileRC{bi, bj};
    return t;
}

// (sbi, sbj), sbi <= sbj, of the super-tiles of DD_SB × DD_SB tiles
inline std::vector<TileRC> stile_rc_table(int nb)
{
    const int nsb = (nb + DD_SB - 1) / DD_SB;
    std::vector<TileRC> t;
    for (int bi = 0; bi < nsb; bi++)
        for (int bj = bi; bj < nsb; bj++) t.push_back(TileRC{bi, bj});
    return t;
}

// the super-tiles of DD_SB × 2 tiles holding at least one stored tile (bi <= bj): sbj·2 + 1 >= sbi·4
inline std::vector<TileRC> stile2_rc_table(int nb)
{
    const int nsb = (nb + DD_SB - 1) / DD_SB;
    std::vector<TileRC> t;
    for (int si = 0; si < nsb; si++)
        for (int sj = 0; sj < (nb + 1) / 2; sj++)
            if (sj * 2 + 1 >= si * 4) t.push_back(TileRC{si, sj});
    return t;
}

// The WT_R × WT_C wave-tile (wr, wc): its tile indices (fallback_tile, a stored tile, where the
// position is below the diagonal or past the block) and its operand row blocks, clamped to the block
inline WtEntry make_wt_entry(int wr, int wc, int nb, long long fallback_tile)
{
    WtEntry v = {};
    for (int r = 0; r < WT_R; r++)
        for (int cc = 0; cc < WT_C; cc++) {
            const int i = r * WT_C + cc;
            const int bi = wr * WT_R + r, bj = wc * WT_C + cc;
            const bool ok = bi < nb && bj < nb && bi <= bj;
            v.tile[i] = (int)(ok ? tile_index(bi, bj, nb) : fallback_tile);
            v.valid |= (ok ? 1 : 0) << i;
        }
    for (int r = 0; r < WT_R; r++) v.rows[0] |= std::min(wr * WT_R + r, nb - 1) << (16 * r);
    for (int cc = 0; cc < WT_C; cc++) v.rows[1] |= std::min(wc * WT_C + cc, nb - 1) << (16 * cc);
    v.rc = wr | (wc << 16);
    return v;
}

// The wave-tiles holding a stored tile (wc·WT_C + WT_C − 1 >= wr·WT_R), in panels of 16 wave-tile
// columns walked row by row (the wave-tiles an XCD has in flight share operand rows)
inline std::vector<WtEntry> wt_table(int nb)
{
    const int nwr = (nb + WT_R - 1) / WT_R, nwc = (nb + WT_C - 1) / WT_C;
    std::vector<WtEntry> t;
    for (int pc = 0; pc < nwc; pc += 16)
        for (int wr = 0; wr < nwr; wr++)
            for (int wc = pc; wc < pc + 16 && wc < nwc; wc++) {
                if (wc * WT_C + WT_C - 1 < wr * WT_R) continue;
                // the fallback: a stored tile of this wave-tile (its first row, last column in the block)
                const int fbi = wr * WT_R, fbj = std::min(wc * WT_C + WT_C - 1, nb - 1);
                t.push_back(make_wt_entry(wr, wc, nb, tile_index(fbi, fbj, nb)));
            }
    return t;
}

// The f64 wave flush: wave-tiles of 1 × WT64_C tiles (tile[0..1], rows[0] the A row block), same
// panel walk
inline std::vector<WtEntry> wt64_table(int nb)
{
    const int nwc = (nb + WT64_C - 1) / WT64_C;
    std::vector<WtEntry> t;
    for (int pc = 0; pc < nwc; pc += 16)
        for (int wr = 0; wr < nb; wr++)
            for (int wc = pc; wc < pc + 16 && wc < nwc; wc++) {
                if (wc * WT64_C + WT64_C - 1 < wr) continue;
                WtEntry v = {};
                const int fbj = std::min(wc * WT64_C + WT64_C - 1, nb - 1);   // stored
                for (int cc = 0; cc < WT64_C; cc++) {
                    const int bj = wc * WT64_C + cc;
                    const bool ok = bj < nb && wr <= bj;
                    v.tile[cc] = (int)tile_index(wr, ok ? bj : fbj, nb);
                    v.valid |= (ok ? 1 : 0) << cc;
                    v.rows[1] |= std::min(bj, nb - 1) << (16 * cc);
                }
                v.rows[0] = wr;
                v.rc = wr | (wc << 16);
                t.push_back(v);
            }
    return t;
}

// The split-bf16 flush's 2 × 4 wave-tiles holding a stored tile (4wc + 3 >= 2wr), as wr | wc << 16,
// in panels of 8 wave-tile columns walked row by row (flush_bf24_kernel)
inline std::vector<int> wt24_table(int nb)
{
    const int nwr = (nb + 1) / 2, nwc = (nb + 3) / 4;
    std::vector<int> t;
    for (int pc = 0; pc < nwc; pc += 8)
        for (int wr = 0; wr < nwr; wr++)
            for (int wc = pc; wc < pc + 8 && wc < nwc; wc++)
                if (4 * wc + 3 >= 2 * wr) t.push_back(wr | (wc << 16));
    return t;
}

// The split-fp16 quad form's groups of 2 × 2 wave-tiles holding a stored tile (group column >= group
// row), in panels of 8 group columns walked row by row; entry 2a + b of a group is its wave-tile
// (2R + a, 2C + b). Wave-tiles wholly below the diagonal or past the block stay in their group (the
// group's operand rows are loaded alike): no valid tile, indices of a stored tile of the group, rows
// clamped to the block.
inline std::vector<WtEntry> wtq_table(int nb)
{
    const int nwr = (nb + WT_R - 1) / WT_R, nwc = (nb + WT_C - 1) / WT_C;
    const int ngr = (nwr + 1) / 2, ngc = (nwc + 1) / 2;
    std::vector<WtEntry> t;
    for (int pc = 0; pc < ngc; pc += 8)
        for (int R = 0; R < ngr; R++)
            for (int C = pc; C < pc + 8 && C < ngc; C++) {
                if (C < R) continue;
                // a stored tile of the group: its first tile row, last tile column in the block
                const long long any = tile_index(4 * R, std::min(4 * C + 3, nb - 1), nb);
                for (int a = 0; a < 2; a++)
                    for (int b = 0; b < 2; b++) t.push_back(make_wt_entry(2 * R + a, 2 * C + b, nb, any));
            }
    return t;
}

// A partitioned instance flushes its tile rows only: the entries of a wave table (tile_rows tile
// rows per wave-tile row: WT_R, or 1 for the f64 table) whose first tile row is in [r0, r1)
inline std::vector<WtEntry> keep_tile_rows(const std::vector<WtEntry>& t, int tile_rows, int r0, int r1)
{
    std::vector<WtEntry> keep;
    for (const WtEntry& v : t) {
        const int r = (v.rc & 0xffff) * tile_rows;
        if (r >= r0 && r < r1) keep.push_back(v);
    }
    return keep;
}

}  // namespace ekf
