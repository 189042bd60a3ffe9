// levels_addr_check.cpp -- a host program for tests/test_levels_cpu.py: the uniform-lag row arithmetic of the scale-space
// search (umpa_amd/csrc/umpa_levels_geom.h over umpa_widen_geom.h) swept on the CPU.  Built with
// -fsanitize=address,undefined and run as it is; it touches no GPU and is never loaded into Python.
//
// For dense row and column counts, level lists, chunkings and both raw layouts it plays the consumer's calls on real
// buffers of exactly the sizes the library allocates.  The chunk's table is filled with a code of (row, plane, column) and
// the carry of 2 bmax rows is refilled by widen_carry_copy's runs.  Checked per call:
//   the march of levels_table_kernel: every raw row of levels_raw_rows of every segment, at every column, is read through
//     widen_src from the buffer it names, in range, and holds the code of the entry asked for;
//   every level: each entry of a fitting row (levels_fit) finds its rows r - b .. r + b inside the rows the march loaded, and
//     widen_dst stays inside that level's pooled table; over all calls every pooled row is written exactly once per level;
//   the level 0: the rows levels_plain_rows takes from the carry and from the chunk, addressed as the consumer kernels
//     address a table (grid_table_px with the ReplayArgs the host builds), are in range, hold the right code, and cover
//     every dense row exactly once over all calls;
//   levels_out_rows: the output rows of the calls partition the region's rows at every step.
#include <cassert>
#include <cstdio>
#include <vector>

#include "../umpa_amd/csrc/umpa_levels_geom.h"

using namespace umpa;

static const int SEG = 64;                                           // UMPA_WIDEN_SEG

static double code(int row, int slot, int col) { return (double)row * 4096.0 * 64.0 + (double)slot * 4096.0 + (double)col; }

static size_t raw_at(WidenGeom g, int rows, int r, int slot, int col)
{
    g.drow0 = 0; g.drows = rows; g.crows = 0;
    bool in_carry = true;
    const size_t at = widen_src(g, r, slot, col, in_carry);
    assert(!in_carry);
    return at;
}

// the consumer kernels' addressing of dense (row, col), plane `slot`, in a table that holds `rows` rows from `first`
static size_t table_px(const WidenGeom& g, int first, int rows, int row, int slot, int col)
{
    if (g.strip_w > 0) {
        const int strip = col / g.strip_w;
        return (((size_t)strip * rows + (size_t)(row - first)) * (size_t)g.U2) * g.tw + (size_t)(col - strip * g.strip_w) + (size_t)slot * g.tw;
    }
    return (size_t)(row - first) * g.N1p + (size_t)col + (size_t)slot * ((size_t)rows * g.N1p);
}

static long sweep(int N0d, int N1d, int L, const int* b, int chunk, bool strip)
{
    assert(levels_check(L, b) == 0);
    const int U2 = 4, bmax = b[0];
    WidenGeom g;
    g.b = bmax; g.U2 = U2; g.N0d = N0d; g.N1d = N1d;
    g.strip_w = strip ? 24 : 0; g.tw = strip ? 64 : 0;
    g.N1p = strip ? (N1d + 23) / 24 * 64 : (N1d + 31) / 32 * 32;
    g.N1q = (N1d + 31) / 32 * 32;
    std::vector<double> carry;
    std::vector<std::vector<int>> written(L, std::vector<int>(N0d, 0));
    int pool_rows = 0;
    long reads = 0;
    for (int drow0 = 0; drow0 < N0d; drow0 += chunk) {
        const int drows = N0d - drow0 < chunk ? N0d - drow0 : chunk;
        const bool last = drow0 + drows >= N0d;
        g.drow0 = drow0; g.drows = drows; g.crows = drow0 == 0 ? 0 : 2 * bmax;
        widen_rows(bmax, N0d, drow0, drows, g.p0, g.p1);
        assert(last || drows >= 2 * bmax);                           // what the library refuses otherwise
        if (drow0 == 0) {
            pool_rows = N0d < drows + bmax ? N0d : drows + bmax;
            carry.assign((last || bmax == 0) ? 0 : widen_table_len(g, 2 * bmax), -1.0);
        }
        assert(g.p1 - g.p0 <= pool_rows);
        std::vector<double> table(widen_table_len(g, drows), -1.0);
        for (int r = 0; r < drows; r++)
            for (int s = 0; s < U2; s++)
                for (int c = 0; c < N1d; c++) {
                    const size_t at = raw_at(g, drows, r, s, c);
                    assert(at < table.size() && table[at] == -1.0);
                    table[at] = code(drow0 + r, s, c);
                }
        const size_t pool_len = (size_t)U2 * pool_rows * g.N1q;
        // the march, segment by segment
        for (int ra = g.p0; ra < g.p1 && bmax > 0; ra += SEG) {
            const int rb = ra + SEG < g.p1 ? ra + SEG : g.p1;
            int lo, hi;
            levels_raw_rows(bmax, N0d, ra, rb, lo, hi);
            assert(lo >= g.drow0 - g.crows && hi <= g.drow0 + g.drows && lo >= 0 && hi <= N0d);
            for (int rr = lo; rr < hi; rr++)
                for (int s = 0; s < U2; s++)
                    for (int c = 0; c < N1d; c++) {
                        bool in_carry = false;
                        const size_t at = widen_src(g, rr, s, c, in_carry);
                        const std::vector<double>& buf = in_carry ? carry : table;
                        assert(at < buf.size() && buf[at] == code(rr, s, c));
                        reads++;
                    }
            for (int l = 0; l < L; l++) {
                if (b[l] == 0) continue;
                int sa, sb;
                levels_fit(b[l], N0d, ra, rb, sa, sb);
                for (int r = sa; r < sb; r++) assert(r - b[l] >= lo && r + b[l] < hi && r - b[l] >= 0 && r + b[l] < N0d);
                for (int r = ra; r < rb; r++)
                    for (int s = 0; s < U2; s++) {
                        assert(widen_dst(g, r, s, 0) + (size_t)g.N1q <= pool_len);
                    }
            }
        }
        for (int l = 0; l < L; l++) {
            if (b[l] > 0) { for (int r = g.p0; r < g.p1; r++) written[l][r]++; continue; }
            // the model's own window: raw rows of the carry, then of the chunk
            int c0, c1, t0, t1;
            levels_plain_rows(g, c0, c1, t0, t1);
            assert(c1 - c0 + t1 - t0 == g.p1 - g.p0);
            for (int r = c0; r < c1; r++) {
                written[l][r]++;
                assert(g.crows > 0 && r >= g.drow0 - g.crows && r < g.drow0);
                for (int s = 0; s < U2; s++)
                    for (int c = 0; c < N1d; c++) {
                        const size_t at = table_px(g, g.drow0 - g.crows, g.crows, r, s, c);
                        assert(at < carry.size() && carry[at] == code(r, s, c));
                        reads++;
                    }
            }
            for (int r = t0; r < t1; r++) {
                written[l][r]++;
                assert(r >= g.drow0 && r < g.drow0 + g.drows);
                for (int s = 0; s < U2; s++)
                    for (int c = 0; c < N1d; c++) {
                        const size_t at = table_px(g, g.drow0, g.drows, r, s, c);
                        assert(at < table.size() && table[at] == code(r, s, c));
                        reads++;
                    }
            }
        }
        if (!last && bmax > 0) {
            const WidenCarryCopy cc = widen_carry_copy(g);
            assert(cc.nruns * cc.run == carry.size());
            for (size_t q = 0; q < cc.nruns; q++)
                for (size_t i = 0; i < cc.run; i++) {
                    assert(cc.src_off + q * cc.pitch + i < table.size());
                    carry[q * cc.run + i] = table[cc.src_off + q * cc.pitch + i];
                }
        }
    }
    for (int l = 0; l < L; l++)
        for (int r = 0; r < N0d; r++) assert(written[l][r] == 1);
    // the output rows of the calls partition the region's rows, at every step
    for (int step = 1; step <= 3; step++) {
        if ((N0d - 1) % step) continue;
        const int N0 = (N0d - 1) / step + 1;
        int next = 0;
        for (int drow0 = 0; drow0 < N0d; drow0 += chunk) {
            const int drows = N0d - drow0 < chunk ? N0d - drow0 : chunk;
            int p0, p1, row0, rows;
            widen_rows(bmax, N0d, drow0, drows, p0, p1);
            levels_out_rows(p0, p1, step, N0, row0, rows);
            if (rows == 0) continue;
            assert(row0 == next && row0 * step >= p0 && (row0 + rows - 1) * step < p1);
            next = row0 + rows;
        }
        assert(next == N0);
    }
    return reads;
}

int main()
{
    long reads = 0, cases = 0;
    const int lists[][5] = {{1, 0}, {1, 2}, {1, 8}, {2, 1, 0}, {2, 4, 1}, {2, 8, 1}, {2, 8, 4}, {3, 8, 2, 0}, {3, 4, 2, 1}, {3, 8, 4, 2}, {4, 4, 2, 1, 0},
                            {4, 8, 4, 1, 0}, {4, 8, 4, 2, 0}, {2, 2, 1}, {2, 4, 2}, {3, 8, 2, 1}, {3, 8, 4, 1}, {2, 4, 0}, {2, 8, 2}, {1, 1}};
    const int drows_list[] = {1, 5, 16, 17, 33, 64, 97, 130};
    const int chunks[] = {32, 64, 1 << 20};                          // whole tiles of 32 rows, as tiled_table cuts them; one chunk
    for (const auto& list : lists)
        for (int N0d : drows_list)
            for (int N1d : {3, 40, 77})
                for (int chunk : chunks)
                    for (int strip = 0; strip < 2; strip++) { reads += sweep(N0d, N1d, list[0], list + 1, chunk, strip != 0); cases++; }
    printf("levels_addr_check: %ld cases, %ld reads, all in range\n", cases, reads);
    return 0;
}
