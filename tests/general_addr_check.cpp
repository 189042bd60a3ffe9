// general_addr_check.cpp -- a host program for tests/test_general_regimes_cpu.py: the footprint arithmetic of the general
// shift-table kernel (umpa_amd/csrc/umpa_general_geom.h) swept on the CPU.  Built with -fsanitize=address,undefined and run
// as it is; it touches no GPU and is never loaded into Python.
//
// For window half-widths 0..8, search ranges 1..9, steps 1..6 in each direction and one step past 273, masks on and off and
// both coordinate modes it plays general_table_kernel's staging and reads on heap buffers of exactly the sizes
// general_footprints gives (three separate allocations, so that a read past one footprint lands in a red zone and not in its
// neighbour, as it would in LDS).  The frames: one that holds the whole region, one that begins inside the first workgroup's
// box (the box origin lies at a negative frame coordinate), one smaller than a footprint that ends before the last
// workgroup's box, and one of 3 x 3 pixels that contributes to nobody.  A staged element holds the code of the frame element it
// was loaded from and whether that coordinate was clamped.  Checked, per workgroup, row chunk, pass, frame, contributing lane,
// accumulator set and window element:
//   every index lies inside its own footprint; every staged element's source lies inside the frame; no element whose source
//   was clamped is read; a set past ms - 1 reads the addresses of shift ms - 1; what is read is the code of the frame element
//   that eval_direct's addressing (umpa_direct.h) names for that window element and shift.
// Where that is cheap (S <= 3, ms <= 3) every lane plays every pass, every set and every window element.  Elsewhere the lanes
// are those on the border of the workgroup's active rectangle and every seventeenth inside it, the window elements the corners
// and the centre, and every set of every pass is played by the rectangle's four corner lanes, the passes of the first, the
// middle and the last row shift by the others: every index is affine in lane, element and shift, so its extremes lie there.
//
// Printed: one line per case of the list the Python side restates (tests/general_expect.py: LDS_CASES) -- staged or fallback
// and the LDS bytes -- and the totals.
#include <cassert>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../umpa_amd/csrc/umpa_general_geom.h"

using namespace umpa;

static const int BX = 16, BY = 16, CJ = 4, THREADS = 256;           // UMPA_STAGED_BX / BY, UMPA_GENERAL_CJ

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "general_addr_check: %s fails at line %d (Nw %d ms %d step %d,%d mask %d ref %d)\n", #cond, __LINE__, g_case[0], g_case[1], g_case[2], g_case[3], g_case[4], g_case[5]); abort(); } } while (0)
static int g_case[6];

struct Frame { int H, W, pi, pj; };
struct Cell { int row, col; bool clamped; };

static long g_reads = 0, g_staged = 0, g_fallback = 0;

static void stage(std::vector<Cell>& buf, int rows, int cols, int halo, int fi0, int fj0, const Frame& f)
{
    // the kernel's loop: q = tid, tid + THREADS, ...: every q in [0, rows * cols) exactly once
    for (int tid = 0; tid < THREADS; tid++)
        for (int q = tid; q < rows * cols; q += THREADS) {
            const int r = q / cols, c = q - r * cols;
            const int sr = general_source(fi0, halo, r, f.H), sc = general_source(fj0, halo, c, f.W);
            CHECK(sr >= 0 && sr < f.H && sc >= 0 && sc < f.W);
            CHECK((size_t)q < buf.size());
            buf[q] = Cell{sr, sc, sr != fi0 - halo + r || sc != fj0 - halo + c};
        }
}

static bool frame_misses(int H, int W, int li, int lj, int pad) { return li - pad < 0 || li + pad > H || lj - pad < 0 || lj + pad > W; }

// one read of the kernel: footprint `buf` at `idx`; it must hold frame element (row, col) unclamped
static void read_at(const std::vector<Cell>& buf, long idx, int row, int col, const Frame& f)
{
    CHECK(idx >= 0 && (size_t)idx < buf.size());
    const Cell& x = buf[(size_t)idx];
    CHECK(row >= 0 && row < f.H && col >= 0 && col < f.W);           // (eval_direct's own read lies inside the frame)
    CHECK(!x.clamped);
    CHECK(x.row == row && x.col == col);
    g_reads++;
}

static bool run_case(int Nw, int ms, int step0, int step1, bool mask, int ref_mode, size_t& lds)
{
    g_case[0] = Nw; g_case[1] = ms; g_case[2] = step0; g_case[3] = step1; g_case[4] = mask; g_case[5] = ref_mode;
    GeneralFootprints G;
    const bool staged = general_footprints(Nw, ms, ref_mode, mask, step0, step1, BY, BX, G);
    lds = G.lds_bytes;
    if (!staged) { g_fallback++; return false; }
    g_staged++;
    const int pad = Nw + ms, S = 2 * Nw + 1;
    const int N0 = 17, N1 = 18, off0 = 2, off1 = 1;                  // a ROI with an offset: two workgroups each way, ragged
    const int org0 = pad + off0, org1 = pad + off1;
    const int last_i = org0 + step0 * (N0 - 1), last_j = org1 + step1 * (N1 - 1);
    const Frame frames[4] = {
        {last_i + pad + 1, last_j + pad + 1, 0, 0},
        {last_i + pad + 1 - (org0 - pad + 2), last_j + pad + 1 - (org1 - pad + 3), org0 - pad + 2, org1 - pad + 3},
        {2 * pad + 3, 2 * pad + 2, off0 + 1, off1},
        {3, 3, org0, org1},
    };
    std::vector<Cell> fq((size_t)G.rowsQ * G.colsQ), fr((size_t)G.rowsR * G.colsR), fm((size_t)G.rowsM * G.colsM);
    const bool every = S <= 3 && ms <= 3;
    long contributing = 0;
    const int chunks[2][2] = {{0, 16}, {16, N0 - 16}};               // (row0, rows): two row chunks
    for (const auto& ch : chunks) {
        const int row0 = ch[0], rows = ch[1];
        for (int by = 0; by < (rows + BY - 1) / BY; by++)
            for (int bx = 0; bx < (N1 + BX - 1) / BX; bx++) {
                const int gi0 = general_box_origin(org0, step0, row0 + by * BY), gj0 = general_box_origin(org1, step1, bx * BX);
                const int act_r = rows - by * BY < BY ? rows - by * BY : BY, act_c = N1 - bx * BX < BX ? N1 - bx * BX : BX;
                for (const Frame& f : frames) {
                    const int fi0 = gi0 - f.pi, fj0 = gj0 - f.pj;
                    stage(fq, G.rowsQ, G.colsQ, G.hq, fi0, fj0, f);
                    stage(fr, G.rowsR, G.colsR, G.hr, fi0, fj0, f);
                    if (mask) stage(fm, G.rowsM, G.colsM, G.hm, fi0, fj0, f);
                    for (int ty = 0; ty < act_r; ty++)
                        for (int tx = 0; tx < act_c; tx++) {
                            const bool border = ty == 0 || tx == 0 || ty == act_r - 1 || tx == act_c - 1;
                            if (!every && !border && (ty * BX + tx) % 17) continue;
                            const int xi = row0 + by * BY + ty, xj = bx * BX + tx;
                            const int i = org0 + step0 * xi, j = org1 + step1 * xj;
                            if (frame_misses(f.H, f.W, i - f.pi, j - f.pj, pad)) continue;
                            contributing++;
                            const bool corner_lane = (ty == 0 || ty == act_r - 1) && (tx == 0 || tx == act_c - 1);
                            for (int si = 1 - ms; si < ms; si++) {
                                if (!every && !corner_lane && si != 1 - ms && si != 0 && si != ms - 1) continue;
                                for (int sj0 = 1 - ms; sj0 < ms; sj0 += CJ) {
                                    int ri = i, rj = j, qi = i, qj = j;
                                    if (ref_mode) { qi -= si; qj -= sj0; } else { ri += si; rj += sj0; }
                                    const int q0 = general_window_origin(qi, qj, Nw, gi0, gj0, G.hq, G.colsQ);
                                    const int r0 = general_window_origin(ri, rj, Nw, gi0, gj0, G.hr, G.colsR);
                                    const int mq0 = general_window_origin(qi, qj, Nw, gi0, gj0, G.hm, G.colsM);
                                    const int mr0 = general_window_origin(ri, rj, Nw, gi0, gj0, G.hm, G.colsM);
                                    for (int c = 0; c < CJ; c++) {
                                        const int dc = general_set_offset(c, ms, sj0);
                                        const int dq = ref_mode ? -dc : 0, dr = ref_mode ? 0 : dc;
                                        const int sj = sj0 + c < ms ? sj0 + c : ms - 1;   // a set past ms - 1 is shift ms - 1 ...
                                        CHECK(sj0 + dc == sj);
                                        if (sj0 + c >= ms) {                              // ... address for address
                                            const int dl = general_set_offset(ms - 1 - sj0, ms, sj0);
                                            CHECK(dc == dl && ms - 1 - sj0 >= 0 && ms - 1 - sj0 < CJ);
                                        }
                                        // eval_direct's window origins in frame coordinates for the shift (si, sj)
                                        int eri = i, erj = j, eqi = i, eqj = j;
                                        if (ref_mode) { eqi -= si; eqj -= sj; } else { eri += si; erj += sj; }
                                        const int rrow = eri - f.pi - Nw, rcol = erj - f.pj - Nw, qrow = eqi - f.pi - Nw, qcol = eqj - f.pj - Nw;
                                        for (int a = 0; a < S; a++)
                                            for (int b = 0; b < S; b++) {
                                                const bool corner = (a == 0 || a == S - 1) && (b == 0 || b == S - 1);
                                                if (!every && !corner && !(a == Nw && b == Nw)) continue;
                                                read_at(fr, (long)r0 + a * G.colsR + dr + b, rrow + a, rcol + b, f);
                                                read_at(fq, (long)q0 + a * G.colsQ + dq + b, qrow + a, qcol + b, f);
                                                if (mask) {
                                                    read_at(fm, (long)mr0 + a * G.colsM + dr + b, rrow + a, rcol + b, f);
                                                    read_at(fm, (long)mq0 + a * G.colsM + dq + b, qrow + a, qcol + b, f);
                                                }
                                            }
                                    }
                                }
                            }
                        }
                }
            }
    }
    CHECK(contributing > 0);
    return true;
}

int main()
{
    // the cases of tests/general_expect.py's LDS_CASES, in its order: (Nw, ms, step0, step1, mask, ref_mode)
    const int listed[][6] = {
        {1, 2, 4, 4, 0, 0}, {1, 2, 4, 3, 0, 0}, {1, 2, 3, 4, 0, 0}, {1, 1, 4, 4, 0, 0}, {1, 1, 4, 5, 0, 0}, {1, 1, 5, 4, 0, 0},
        {1, 2, 3, 3, 1, 1}, {1, 2, 3, 4, 1, 1}, {1, 2, 2, 3, 0, 0}, {1, 2, 5, 5, 0, 0}, {2, 3, 1, 1, 1, 0}, {8, 9, 1, 1, 1, 1},
        {8, 9, 2, 2, 1, 1}, {8, 9, 2, 1, 1, 1}, {0, 1, 5, 5, 0, 0}, {0, 1, 6, 5, 0, 0}, {1, 3, 273, 1, 0, 0}, {1, 3, 1, 273, 1, 1},
    };
    for (const auto& c : listed) {
        size_t lds = 0;
        const bool st = run_case(c[0], c[1], c[2], c[3], c[4] != 0, c[5], lds);
        printf("case Nw %d ms %d step %d %d mask %d ref %d: %s %zu\n", c[0], c[1], c[2], c[3], c[4], c[5], st ? "staged" : "fallback", lds);
    }
    long cases = 0;
    const int steps[][2] = {{1, 1}, {2, 2}, {3, 3}, {4, 4}, {5, 5}, {6, 6}, {1, 2}, {2, 1}, {1, 3}, {3, 1}, {1, 4}, {4, 1}, {1, 5}, {5, 1},
                            {1, 6}, {6, 1}, {2, 3}, {4, 3}, {3, 4}, {6, 2}, {273, 1}, {1, 300}};
    for (int Nw = 0; Nw <= 8; Nw++)
        for (int ms = 1; ms <= 9; ms++)
            for (const auto& s : steps)
                for (int mask = 0; mask < 2; mask++)
                    for (int ref_mode = 0; ref_mode < 2; ref_mode++) {
                        size_t lds = 0;
                        const bool st = run_case(Nw, ms, s[0], s[1], mask != 0, ref_mode, lds);
                        if (s[0] >= 273 || s[1] >= 273) CHECK(!st);                  // a box of 4096 pixels and more: never staged
                        else CHECK(st == (lds <= 65536) && lds > 0);
                        cases++;
                    }
    printf("general_addr_check: %ld cases (%ld staged, %ld fallback), %ld reads, all in range\n", cases, g_staged, g_fallback, g_reads);
    return 0;
}
