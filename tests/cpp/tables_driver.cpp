// tables_driver.cpp — the flush kernels' tile tables (ekf_tables.h) and the flush plan
// (ekf_flush_plan.h) checked on a CPU: structural properties of every table, and the two golden
// fixtures recorded from the loops, name function and launcher conditions these headers replaced.
//   tables_driver <flush_tables.txt> <flush_kernel_names.txt>
// Built with -fsanitize=address,undefined by tests/test_host_tables.py; exit status 0 = all pass.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "ekf_flush_plan.h"
#include "ekf_layout.h"
#include "ekf_tables.h"

using namespace ekf;

static int failures = 0;
#define CHECK(cond, ...)                                     \
    do {                                                     \
        if (!(cond)) {                                       \
            if (failures++ < 20) {                           \
                fprintf(stderr, "FAIL %s: ", #cond);         \
                fprintf(stderr, __VA_ARGS__);                \
                fprintf(stderr, "\n");                       \
            }                                                \
        }                                                    \
    } while (0)

static unsigned long long fnv1a64(const void* p, size_t n)
{
    unsigned long long h = 1469598103934665603ull;
    const unsigned char* b = (const unsigned char*)p;
    for (size_t i = 0; i < n; i++) {
        h ^= b[i];
        h *= 1099511628211ull;
    }
    return h;
}

template <typename V>
static void emit(std::string& out, int nb, int world, int rank, const char* name, const std::vector<V>& t)
{
    char line[128];
    snprintf(line, sizeof line, "%d %d %d %s %zu %016llx\n", nb, world, rank, name, t.size(),
             fnv1a64(t.data(), t.size() * sizeof(V)));
    out += line;
}

// every slot holds a tile of the block, every packed row block is a row of it
static void check_entry_bounds(const char* what, const WtEntry& v, int nb, long long ntiles)
{
    for (int i = 0; i < WT_N; i++)
        CHECK(v.tile[i] >= 0 && v.tile[i] < ntiles, "%s nb %d rc %#x slot %d tile %d", what, nb, v.rc, i, v.tile[i]);
    for (int h = 0; h < 2; h++)
        for (int f = 0; f < 2; f++) {
            const int rb = (v.rows[h] >> (16 * f)) & 0xffff;
            CHECK(rb < nb, "%s nb %d rc %#x rows[%d] field %d = %d", what, nb, v.rc, h, f, rb);
        }
    CHECK(v.rows[0] >= 0 && v.rows[1] >= 0, "%s nb %d rc %#x negative rows", what, nb, v.rc);
}

// a table of WT_R × WT_C wave-tiles (wt, wtq): bounds, the slots' positions, rows and rc; counts the
// entries marking each stored tile valid
static void check_wave_tiles(const char* what, const std::vector<WtEntry>& t, int nb, std::vector<int>& cnt)
{
    const long long ntiles = (long long)nb * (nb + 1) / 2;
    cnt.assign((size_t)ntiles, 0);
    for (const WtEntry& v : t) {
        check_entry_bounds(what, v, nb, ntiles);
        const int wr = v.rc & 0xffff, wc = v.rc >> 16;
        CHECK((v.valid & ~((1 << WT_N) - 1)) == 0, "%s nb %d rc %#x valid %#x", what, nb, v.rc, v.valid);
        for (int r = 0; r < WT_R; r++)
            for (int c = 0; c < WT_C; c++) {
                const int i = r * WT_C + c, bi = wr * WT_R + r, bj = wc * WT_C + c;
                const bool stored = bi < nb && bj < nb && bi <= bj;
                CHECK(((v.valid >> i) & 1) == (stored ? 1 : 0), "%s nb %d rc %#x slot %d", what, nb, v.rc, i);
                if (stored) {
                    CHECK(v.tile[i] == tile_index(bi, bj, nb), "%s nb %d rc %#x slot %d tile %d", what, nb, v.rc, i, v.tile[i]);
                    if (v.tile[i] >= 0 && v.tile[i] < ntiles) cnt[(size_t)v.tile[i]]++;
                }
            }
        for (int r = 0; r < WT_R; r++)
            CHECK(((v.rows[0] >> (16 * r)) & 0xffff) == std::min(wr * WT_R + r, nb - 1), "%s nb %d rc %#x A rows", what, nb, v.rc);
        for (int c = 0; c < WT_C; c++)
            CHECK(((v.rows[1] >> (16 * c)) & 0xffff) == std::min(wc * WT_C + c, nb - 1), "%s nb %d rc %#x B rows", what, nb, v.rc);
    }
}

static void check_once(const char* what, const std::vector<int>& cnt, int nb)
{
    for (size_t t = 0; t < cnt.size(); t++)
        CHECK(cnt[t] == 1, "%s nb %d: tile %zu valid in %d entries", what, nb, t, cnt[t]);
}

static void check_tables(int nb, std::string& out)
{
    const long long ntiles = (long long)nb * (nb + 1) / 2;
    const int nsb = (nb + DD_SB - 1) / DD_SB;
    std::vector<int> cnt;

    const std::vector<TileRC> trc = tile_rc_table(nb);
    CHECK((long long)trc.size() == ntiles, "tile_rc nb %d size %zu", nb, trc.size());
    for (size_t t = 0; t < trc.size(); t++)
        CHECK(trc[t].x >= 0 && trc[t].x <= trc[t].y && trc[t].y < nb && tile_index(trc[t].x, trc[t].y, nb) == (long long)t,
              "tile_rc nb %d entry %zu = (%d, %d)", nb, t, trc[t].x, trc[t].y);
    emit(out, nb, 0, 0, "tile_rc", trc);

    // the super-tiles: each one holding a stored tile is listed exactly once, and no other
    const std::vector<TileRC> st = stile_rc_table(nb);
    cnt.assign((size_t)nsb * nsb, 0);
    for (const TileRC& v : st) {
        CHECK(v.x >= 0 && v.x <= v.y && v.y < nsb, "stile_rc nb %d (%d, %d)", nb, v.x, v.y);
        if (v.x >= 0 && v.x < nsb && v.y >= 0 && v.y < nsb) cnt[(size_t)v.x * nsb + v.y]++;
    }
    for (int si = 0; si < nsb; si++)
        for (int sj = 0; sj < nsb; sj++)
            CHECK(cnt[(size_t)si * nsb + sj] == (si <= sj ? 1 : 0), "stile_rc nb %d (%d, %d) listed %d times", nb, si, sj,
                  cnt[(size_t)si * nsb + sj]);
    emit(out, nb, 0, 0, "stile_rc", st);

    const std::vector<TileRC> st2 = stile2_rc_table(nb);
    const int nc2 = (nb + 1) / 2;
    cnt.assign((size_t)nsb * nc2, 0);
    for (const TileRC& v : st2) {
        CHECK(v.x >= 0 && v.x < nsb && v.y >= 0 && v.y < nc2, "stile2_rc nb %d (%d, %d)", nb, v.x, v.y);
        if (v.x >= 0 && v.x < nsb && v.y >= 0 && v.y < nc2) cnt[(size_t)v.x * nc2 + v.y]++;
    }
    for (int si = 0; si < nsb; si++)
        for (int sj = 0; sj < nc2; sj++) {
            // rows 4si.., columns 2sj, 2sj + 1: a stored tile iff its first row <= its last column
            const bool holds = 4 * si <= std::min(2 * sj + 1, nb - 1);
            CHECK(cnt[(size_t)si * nc2 + sj] == (holds ? 1 : 0), "stile2_rc nb %d (%d, %d) listed %d times", nb, si, sj,
                  cnt[(size_t)si * nc2 + sj]);
        }
    emit(out, nb, 0, 0, "stile2_rc", st2);

    const std::vector<WtEntry> wt = wt_table(nb);
    check_wave_tiles("wt", wt, nb, cnt);
    check_once("wt", cnt, nb);
    emit(out, nb, 0, 0, "wt", wt);

    const std::vector<WtEntry> wt64 = wt64_table(nb);
    cnt.assign((size_t)ntiles, 0);
    for (const WtEntry& v : wt64) {
        check_entry_bounds("wt64", v, nb, ntiles);
        const int wr = v.rc & 0xffff, wc = v.rc >> 16;
        CHECK((v.valid & ~((1 << WT64_C) - 1)) == 0 && v.rows[0] == wr, "wt64 nb %d rc %#x valid %#x rows[0] %d", nb, v.rc,
              v.valid, v.rows[0]);
        for (int c = 0; c < WT64_C; c++) {
            const int bj = wc * WT64_C + c;
            const bool stored = wr < nb && bj < nb && wr <= bj;
            CHECK(((v.valid >> c) & 1) == (stored ? 1 : 0), "wt64 nb %d rc %#x slot %d", nb, v.rc, c);
            CHECK(((v.rows[1] >> (16 * c)) & 0xffff) == std::min(bj, nb - 1), "wt64 nb %d rc %#x B rows", nb, v.rc);
            if (stored) {
                CHECK(v.tile[c] == tile_index(wr, bj, nb), "wt64 nb %d rc %#x slot %d tile %d", nb, v.rc, c, v.tile[c]);
                if (v.tile[c] >= 0 && v.tile[c] < ntiles) cnt[(size_t)v.tile[c]]++;
            }
        }
    }
    check_once("wt64", cnt, nb);
    emit(out, nb, 0, 0, "wt64", wt64);

    // every stored tile in exactly one 2 × 4 wave-tile, and every code holding one
    const std::vector<int> wt24 = wt24_table(nb);
    cnt.assign((size_t)ntiles, 0);
    for (int code : wt24) {
        const int wr = code & 0xffff, wc = code >> 16;
        int held = 0;
        for (int r = 0; r < 2; r++)
            for (int c = 0; c < 4; c++) {
                const int bi = 2 * wr + r, bj = 4 * wc + c;
                if (bi < nb && bj < nb && bi <= bj) {
                    cnt[(size_t)tile_index(bi, bj, nb)]++;
                    held++;
                }
            }
        CHECK(code >= 0 && held > 0, "wt24 nb %d code %#x holds no stored tile", nb, code);
    }
    check_once("wt24", cnt, nb);
    emit(out, nb, 0, 0, "wt24", wt24);

    // the quad form: groups of four entries, entry 2a + b the wave-tile (2R + a, 2C + b)
    const std::vector<WtEntry> wtq = wtq_table(nb);
    check_wave_tiles("wtq", wtq, nb, cnt);
    check_once("wtq", cnt, nb);
    CHECK(wtq.size() % 4 == 0, "wtq nb %d size %zu", nb, wtq.size());
    for (size_t k = 0; k + 3 < wtq.size(); k += 4)
        for (int a = 0; a < 2; a++)
            for (int b = 0; b < 2; b++) {
                const int rc0 = wtq[k].rc, rc = wtq[k + 2 * a + b].rc;
                CHECK((rc0 & 1) == 0 && ((rc0 >> 16) & 1) == 0 && (rc & 0xffff) == (rc0 & 0xffff) + a && (rc >> 16) == (rc0 >> 16) + b,
                      "wtq nb %d entry %zu rc %#x in the group of %#x", nb, k + 2 * a + b, rc, rc0);
            }
    emit(out, nb, 0, 0, "wtq", wtq);

    // partitions: contiguous ranges with even boundaries that cover [0, nb); the ranks' wave tables
    // are disjoint, keep the table's order and together are the whole table
    for (int world : {1, 2, 3, 5, 8}) {
        int next = 0;
        size_t n32 = 0, n64 = 0;
        std::vector<int> seen32(wt.size(), 0), seen64(wt64.size(), 0);
        for (int rank = 0; rank < world; rank++) {
            int r0 = -1, r1 = -1;
            tile_partition(nb, world, rank, r0, r1);
            CHECK(r0 == next && r1 >= r0 && r1 <= nb, "partition nb %d world %d rank %d: [%d, %d) after %d", nb, world, rank, r0, r1, next);
            CHECK(r1 == nb || r1 % 2 == 0, "partition nb %d world %d rank %d: odd boundary %d", nb, world, rank, r1);
            next = r1;
            char line[96];
            snprintf(line, sizeof line, "%d %d %d partition %d %d\n", nb, world, rank, r0, r1);
            out += line;
            if (r0 >= r1) continue;   // (no context for this rank: more ranks than wave-tile rows)
            const std::vector<WtEntry> p32 = keep_tile_rows(wt, WT_R, r0, r1), p64 = keep_tile_rows(wt64, 1, r0, r1);
            auto account = [&](const char* what, const std::vector<WtEntry>& part, const std::vector<WtEntry>& whole,
                               std::vector<int>& seen, int tile_rows) {
                size_t k = 0;   // (a subsequence of the whole table)
                for (const WtEntry& v : part) {
                    while (k < whole.size() && memcmp(&whole[k], &v, sizeof v) != 0) k++;
                    CHECK(k < whole.size(), "%s nb %d world %d rank %d: rc %#x not in the table's order", what, nb, world, rank, v.rc);
                    if (k < whole.size()) seen[k++]++;
                    const int row = (v.rc & 0xffff) * tile_rows;
                    CHECK(row >= r0 && row < r1, "%s nb %d world %d rank %d: row %d", what, nb, world, rank, row);
                }
            };
            account("wt", p32, wt, seen32, WT_R);
            account("wt64", p64, wt64, seen64, 1);
            n32 += p32.size();
            n64 += p64.size();
            emit(out, nb, world, rank, "wt", p32);
            emit(out, nb, world, rank, "wt64", p64);
        }
        CHECK(next == nb, "partition nb %d world %d ends at %d", nb, world, next);
        CHECK(n32 == wt.size() && n64 == wt64.size(), "nb %d world %d: %zu of %zu wt, %zu of %zu wt64 entries", nb, world, n32,
              wt.size(), n64, wt64.size());
        for (size_t k = 0; k < seen32.size(); k++) CHECK(seen32[k] == 1, "wt nb %d world %d entry %zu in %d ranks", nb, world, k, seen32[k]);
        for (size_t k = 0; k < seen64.size(); k++) CHECK(seen64[k] == 1, "wt64 nb %d world %d entry %zu in %d ranks", nb, world, k, seen64[k]);
    }
}

// the kernel per precision, arithmetic, form, steps, partitioned flag and kmax that a context can have
static std::string plan_names()
{
    std::string out;
    for (int prec : {EKF_PREC_F64, EKF_PREC_F32, EKF_PREC_F16})
        for (int arith : {EKF_ARITH_EXACT, EKF_ARITH_BF16X6, EKF_ARITH_F16X3})
            for (int part = 0; part < 2; part++)
                for (int kmax : {16, 32}) {
                    // split arithmetics: fp32 / fp16 storage, kmax 16; partitioned: exact, fp32 / fp64, kmax 16
                    if (arith != EKF_ARITH_EXACT && (prec == EKF_PREC_F64 || kmax != 16)) continue;
                    if (part && (arith != EKF_ARITH_EXACT || prec == EKF_PREC_F16 || kmax != 16)) continue;
                    for (int form : {FORM_AUTO, FORM_SUPERTILE, FORM_WAVE, FORM_2X4, FORM_QUAD}) {
                        if (part && form != FORM_WAVE) continue;
                        for (int ns = 1; ns <= 24; ns++) {
                            const FlushKey key{prec, arith, form, ns, kmax, part != 0, true, true, true, !part};
                            const FlushPlan plan = flush_plan(key);
                            CHECK(plan.nsteps == ns + ((part && prec == EKF_PREC_F32) ? (ns & 1) : 0) && plan.storage == prec,
                                  "plan of %d %d %d %d %d %d: nsteps %d storage %d", prec, arith, form, ns, part, kmax, plan.nsteps, plan.storage);
                            char name[64], line[128];
                            snprintf(line, sizeof line, "%d %d %d %d %d %d | %s\n", prec, arith, form, ns, part, kmax,
                                     flush_plan_name(plan, name, sizeof name));
                            out += line;
                        }
                    }
                }
    return out;
}

static void compare(const char* path, const std::string& header_prefix, const std::string& got)
{
    std::ifstream f(path);
    std::stringstream ss;
    ss << f.rdbuf();
    std::string want = ss.str();
    CHECK(f.good() || f.eof(), "cannot read %s", path);
    if (want.compare(0, header_prefix.size(), header_prefix) == 0) want.erase(0, want.find('\n') + 1);   // the comment line
    if (want == got) return;
    std::istringstream a(want), b(got);
    std::string la, lb;
    int n = 1;
    while (true) {
        const bool ha = (bool)std::getline(a, la), hb = (bool)std::getline(b, lb);
        if (!ha && !hb) break;
        n++;
        if (ha != hb || la != lb) {
            CHECK(false, "%s line %d: fixture '%s', computed '%s'", path, n, ha ? la.c_str() : "<end>", hb ? lb.c_str() : "<end>");
            return;
        }
    }
}

int main(int argc, char** argv)
{
    if (argc != 3) {
        fprintf(stderr, "usage: %s <flush_tables.txt> <flush_kernel_names.txt>\n", argv[0]);
        return 2;
    }
    static_assert(sizeof(WtEntry) == 32 && sizeof(TileRC) == 8, "table entries as the kernels read them");
    std::string tables;
    for (int nb : {1, 2, 3, 4, 5, 6, 7, 8, 9, 16, 17, 64, 2048}) check_tables(nb, tables);
    compare(argv[1], "#", tables);
    compare(argv[2], "#", plan_names());
    CHECK(!flush_form_valid(1) && !flush_form_valid(-1) && flush_form_valid(FORM_QUAD), "flush_form_valid");
    if (failures) {
        fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    printf("tables and flush plan: ok\n");
    return 0;
}
