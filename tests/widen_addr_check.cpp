// widen_addr_check.cpp -- a host program for tests/test_widen_cpu.py: the addressing of window widening
// (umpa_amd/csrc/umpa_widen_geom.h) swept on the CPU.  Built with -fsanitize=address,undefined and run as it is; it touches
// no GPU and is never loaded into Python.
//
// For dense row counts, half-widths, chunkings and both raw layouts it plays the consumer's calls on real buffers of
// exactly the sizes the library allocates: the table of a chunk is filled with a code of (row, plane, column), the carry is
// refilled by widen_carry_copy's runs, and every raw entry the kernel's march reads (rows r - b .. r + b, columns c - b .. c + b
// of every pooled entry that is a number) is read through widen_src from whichever buffer it names.  Checked: every index
// is inside its buffer (by assert, and by the sanitizer's red zones), the value found is the code of the entry asked for,
// every pooled row of the region is written exactly once over all calls, and widen_dst stays inside the pooled table.
#include <cassert>
#include <cstdio>
#include <vector>

#include "../umpa_amd/csrc/umpa_widen_geom.h"

using namespace umpa;

static double code(int row, int slot, int col) { return (double)row * 4096.0 * 64.0 + (double)slot * 4096.0 + (double)col; }

// the raw index of (row in chunk, slot, col) in a chunk of `rows` rows: widen_src on a geometry without carry
static size_t raw_at(WidenGeom g, int rows, int r, int slot, int col)
{
    g.drow0 = 0; g.drows = rows; g.crows = 0;
    bool in_carry = true;
    const size_t at = widen_src(g, r, slot, col, in_carry);
    assert(!in_carry);
    return at;
}

static long sweep(int N0d, int N1d, int b, int chunk, bool strip)
{
    const int U2 = 9;
    WidenGeom g;
    g.b = b; g.U2 = U2; g.N0d = N0d; g.N1d = N1d;
    g.strip_w = strip ? 24 : 0; g.tw = strip ? 64 : 0;               // (march_plan: tw = 64 where the strip width is no multiple of 16)
    g.N1p = strip ? (N1d + 23) / 24 * 64 : (N1d + 31) / 32 * 32;
    g.N1q = (N1d + 31) / 32 * 32;
    std::vector<double> carry;
    std::vector<int> written(N0d, 0);
    int pool_rows = 0;
    long reads = 0;
    for (int drow0 = 0; drow0 < N0d; drow0 += chunk) {
        const int drows = N0d - drow0 < chunk ? N0d - drow0 : chunk;
        const bool last = drow0 + drows >= N0d;
        g.drow0 = drow0; g.drows = drows; g.crows = drow0 == 0 ? 0 : 2 * b;
        widen_rows(b, N0d, drow0, drows, g.p0, g.p1);
        assert(last || drows >= 2 * b);                              // what the library refuses otherwise
        if (drow0 == 0) {
            pool_rows = N0d < drows + b ? N0d : drows + b;
            carry.assign(last ? 0 : widen_table_len(g, 2 * b), -1.0);
        }
        assert(g.p1 - g.p0 <= pool_rows);
        std::vector<double> table(widen_table_len(g, drows), -1.0);
        for (int r = 0; r < drows; r++)
            for (int s = 0; s < U2; s++)
                for (int c = 0; c < N1d; c++) {
                    const size_t at = raw_at(g, drows, r, s, c);
                    assert(at < table.size() && table[at] == -1.0);   // in range, and no two entries share a place
                    table[at] = code(drow0 + r, s, c);
                }
        std::vector<double> pool((size_t)U2 * pool_rows * g.N1q, 0.0);
        for (int r = g.p0; r < g.p1; r++) {
            assert(r >= 0 && r < N0d);
            written[r]++;
            for (int s = 0; s < U2; s++)
                for (int c = 0; c < g.N1q; c++) {
                    const size_t to = widen_dst(g, r, s, c);
                    assert(to < pool.size());
                    pool[to] += 1.0;
                    if (!widen_inside(g, r, c)) continue;
                    for (int dr = -b; dr <= b; dr++)
                        for (int dc = -b; dc <= b; dc++) {
                            bool in_carry = false;
                            const size_t at = widen_src(g, r + dr, s, c + dc, in_carry);
                            const std::vector<double>& buf = in_carry ? carry : table;
                            assert(at < buf.size());
                            assert(buf[at] == code(r + dr, s, c + dc));
                            reads++;
                        }
                }
        }
        for (int s = 0; s < U2; s++)                                  // every pooled place of the call written once
            for (int r = g.p0; r < g.p1; r++)
                for (int c = 0; c < g.N1q; c++) assert(pool[widen_dst(g, r, s, c)] == 1.0);
        if (!last) {
            const WidenCarryCopy cc = widen_carry_copy(g);
            assert(cc.nruns * cc.run == carry.size());
            for (size_t q = 0; q < cc.nruns; q++)
                for (size_t i = 0; i < cc.run; i++) {
                    assert(cc.src_off + q * cc.pitch + i < table.size());
                    carry[q * cc.run + i] = table[cc.src_off + q * cc.pitch + i];
                }
        }
    }
    for (int r = 0; r < N0d; r++) assert(written[r] == 1);
    return reads;
}

int main()
{
    long reads = 0, cases = 0;
    const int drows_list[] = {1, 5, 16, 17, 33, 64, 97};
    const int chunks[] = {32, 64, 1 << 20};                          // whole tiles of 32 rows, as tiled_table cuts them; one chunk
    for (int N0d : drows_list)
        for (int N1d : {3, 40, 77})
            for (int b = 1; b <= 8; b++)
                for (int chunk : chunks)
                    for (int strip = 0; strip < 2; strip++) { reads += sweep(N0d, N1d, b, chunk, strip != 0); cases++; }
    printf("widen_addr_check: %ld cases, %ld reads, all in range\n", cases, reads);
    return 0;
}
