// walk_machine_check.cpp -- the walk machine of umpa_amd/csrc/umpa_walk.h on the host, against oracle/umpa_oracle.c.
//
//   g++ -O2 -ffp-contract=off -DUMPA_WALK_HOST -I umpa_amd/csrc tests/walk_machine_check.cpp oracle_object -lm
//   ./walk_machine_check [walks per configuration] [seed]
//
// For random tiny models every walk is run twice: by the oracle's blocking minimiser (umpaor_min) and by the machine
// (walk_begin / walk_feed / walk_finish, every second walk through walk_speculate the way replay_walk delivers a second
// result), with umpaor_cost as the evaluator of both.  Status, Ncalls, f, T, df, uv, the memo `d` and -- where the walk
// completes -- the 4x4 neighbourhood `a` must agree in every bit.  The sub-pixel mode is 0 (no fit): the fits are
// arithmetic of their own, not control, and the oracle sums theirs in another order.
// (`a` of a walk that does not complete: the oracle leaves what its gather had collected, walk_finish answers zeros;
//  that has always been so and is checked here as such.)
// Prints one line of counts; exit status 1 and the first mismatches on any difference.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cstdint>
#include <vector>

#include "umpa_walk.h"

extern "C" {
void* umpaor_create(int kind, int Na, const int* dims, double* const* sam, double* const* ref, double* const* mask,
                    const int* pos, int Nw, const double* win, int max_shift, int padding);
void umpaor_destroy(void* p);
void umpaor_set_subpx(void* p, int mode);
void umpaor_set_reference_shift(void* p, int v);
int umpaor_cost(void* p, int i, int j, int si, int sj, double* values);
int umpaor_min(void* p, int i, int j, double* values, double* uv, double* dbg_d, double* dbg_a, int* ncalls);
}

using namespace umpa;

struct HostMemo {
    double* p;
    double& operator[](int q) const { return p[q]; }
};

static uint64_t rng_state = 1;
static inline uint64_t rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return rng_state;
}
static inline double uni() { return (double)(rnd() >> 11) * (1.0 / 9007199254740992.0); }
static inline int below(int n) { return (int)(rnd() % (uint64_t)n); }

static bool same(const double* a, const double* b, int n) { return memcmp(a, b, n * sizeof(double)) == 0; }

struct Counts {
    long walks = 0, calls = 0, ok = 0, bound = 0, capped = 0, move_capped = 0, restarts = 0, second = 0, nan_walks = 0, ties = 0, bad = 0;
};

// one walk by the machine; returns the status
static int machine_walk(void* model, int kind, int i, int j, int cap, bool speculate, double* values, double* uv, double* d,
                        double* a, int* ncalls, Counts& C)
{
    double slots[25];
    for (int q = 0; q < 25; q++) slots[q] = 12345.0;            // never initialised on the device: the mask decides
    const HostMemo memo = {slots};
    Walk w;
    walk_begin(w, memo, uv[0], uv[1]);
    bool saw_nan = false;
    while (w.phase < PH_FIT) {
        int si = w.req_i, sj = w.req_j;
        const bool spec = speculate && walk_speculate(w, si, sj);
        double v1[5] = {0, 0, 0, 0, 0};
        Fit fit = w.live;
        const bool gather = w.phase == PH_GATHER;
        const double c_before = w.c0;
        const int st = umpaor_cost(model, i, j, w.req_i, w.req_j, v1);
        if (st & UMPA_ST_OK) { fit.t = v1[1]; fit.v = kind == 1 ? v1[2] : 0.0; }
        if ((st & UMPA_ST_OK) && gather && v1[0] < c_before) C.restarts++;
        if (v1[0] != v1[0]) saw_nan = true;
        walk_feed(w, memo, st, v1[0], fit, cap);
        if (spec && w.phase < PH_FIT && w.req_i == si && w.req_j == sj) {
            double v2[5] = {0, 0, 0, 0, 0};
            Fit fit2 = w.live;
            const bool gather2 = w.phase == PH_GATHER;
            const double c2_before = w.c0;
            const int st2 = umpaor_cost(model, i, j, si, sj, v2);
            if (st2 & UMPA_ST_OK) { fit2.t = v2[1]; fit2.v = kind == 1 ? v2[2] : 0.0; }
            if ((st2 & UMPA_ST_OK) && gather2 && v2[0] < c2_before) C.restarts++;
            if (v2[0] != v2[0]) saw_nan = true;
            walk_feed(w, memo, st2, v2[0], fit2, cap);
            C.second++;
        }
    }
    if (saw_nan) C.nan_walks++;
    walk_finish(w, memo, 0, a);
    values[0] = w.out;
    values[1] = w.live.t;
    values[2] = w.uv1;
    values[3] = w.uv0;
    values[4] = kind == 1 ? w.live.v : 0.0;
    uv[0] = w.uv0;
    uv[1] = w.uv1;
    for (int q = 0; q < 25; q++) d[q] = walk_memo_cell(w, memo, q);
    *ncalls = w.n;
    return w.status;
}

int main(int argc, char** argv)
{
    const int per_config = argc > 1 ? atoi(argv[1]) : 72;
    rng_state = argc > 2 ? strtoull(argv[2], nullptr, 10) * 2654435761u + 1 : 88172645463325252ull;
    Counts C;
    int printed = 0;
    // model space: 1-4 frames, windows 3-7 (Nw 1-3), max_shift 2-5, both models, both shift conventions;
    // image kinds: 0 speckle + noise, 1 pure noise, 2 constant image (exact ties), 3 speckle with a zeroed patch
    // (NaN costs, the move cap), 4 all zero
    for (int kind = 0; kind < 2; kind++)
    for (int ref_mode = 0; ref_mode < 2; ref_mode++)
    for (int Na = 1; Na <= 4; Na++)
    for (int Nw = 1; Nw <= 3; Nw++)
    for (int ms = 2; ms <= 5; ms++)
    for (int image = 0; image < 5; image++)
    for (int rep = 0; rep < 3; rep++) {
        const int pad = Nw + ms, side = 2 * pad + 9;             // 9 x 9 pixels with a full window at every shift
        const int H = side, W = side + 2;
        std::vector<std::vector<double>> sam(Na), ref(Na);
        std::vector<double*> ps(Na), pr(Na);
        std::vector<int> dims(2 * Na), pos(2 * Na, 0);
        const double noise = rep == 0 ? 0.02 : rep == 1 ? 0.3 : 1.5;
        const int di = below(2 * ms - 1) - (ms - 1), dj = below(2 * ms - 1) - (ms - 1);
        for (int k = 0; k < Na; k++) {
            dims[2 * k] = H; dims[2 * k + 1] = W;
            sam[k].assign((size_t)H * W, 0.0); ref[k].assign((size_t)H * W, 0.0);
            if (image == 2) {
                const double v = 1.0 + below(4);
                for (auto& x : sam[k]) x = 0.75 * v;
                for (auto& x : ref[k]) x = v;
            } else if (image != 4) {
                for (auto& x : ref[k]) x = 1.0 + uni();
                for (int y = 0; y < H; y++)
                    for (int x = 0; x < W; x++) {
                        const int yy = y + di, xx = x + dj;
                        const double r = (image == 0 || image == 3) && yy >= 0 && yy < H && xx >= 0 && xx < W ? ref[k][(size_t)yy * W + xx] : 1.0 + uni();
                        sam[k][(size_t)y * W + x] = 0.8 * r + noise * (uni() - 0.5);
                    }
                if (image == 3) {                                // a zeroed patch in both stacks, wider than a window
                    const int y0 = below(H - 2 * Nw - 3), x0 = below(W - 2 * Nw - 3), hh = 2 * Nw + 2 + below(3), ww = 2 * Nw + 2 + below(3);
                    for (int y = y0; y < y0 + hh && y < H; y++)
                        for (int x = x0; x < x0 + ww && x < W; x++) { sam[k][(size_t)y * W + x] = 0.0; ref[k][(size_t)y * W + x] = 0.0; }
                }
            }
            ps[k] = sam[k].data(); pr[k] = ref[k].data();
        }
        const int S = 2 * Nw + 1;
        std::vector<double> win((size_t)S * S);
        for (int y = 0; y < S; y++)
            for (int x = 0; x < S; x++) win[(size_t)y * S + x] = (1.0 + (y < Nw ? y : 2 * Nw - y)) * (1.0 + (x < Nw ? x : 2 * Nw - x));
        // small call caps (3 .. 40) in two of three repetitions; the oracle reads its cap when a model is created
        const int cap = rep == 2 ? 500 : 3 + below(38);
        char capstr[16];
        snprintf(capstr, sizeof(capstr), "%d", cap);
        setenv("UMPA_CALL_CAP", capstr, 1);
        void* model = umpaor_create(kind, Na, dims.data(), ps.data(), pr.data(), nullptr, pos.data(), Nw, win.data(), ms, pad);
        umpaor_set_subpx(model, 0);
        umpaor_set_reference_shift(model, ref_mode);
        for (int t = 0; t < per_config; t++) {
            const int i = pad + below(H - 2 * pad), j = pad + below(W - 2 * pad);
            double u0 = 0.0, u1 = 0.0;
            const int start = below(4);                          // 0, 1: from (0, 0); 2: inside the range; 3: anywhere near it
            if (start == 2) { u0 = (2 * uni() - 1) * (ms - 1); u1 = (2 * uni() - 1) * (ms - 1); }
            if (start == 3) { u0 = (2 * uni() - 1) * (ms + 1.5); u1 = (2 * uni() - 1) * (ms + 1.5); }
            double v_or[7] = {0, 0, 0, 0, 0, 0, 0}, uv_or[2] = {u0, u1}, d_or[25], a_or[16];
            int n_or = 0;
            const int st_or = umpaor_min(model, i, j, v_or, uv_or, d_or, a_or, &n_or);
            double v_m[5], uv_m[2] = {u0, u1}, d_m[25], a_m[16];
            int n_m = 0;
            const int st_m = machine_walk(model, kind, i, j, cap, (t & 1) != 0, v_m, uv_m, d_m, a_m, &n_m, C);
            C.walks++;
            C.calls += n_m;
            if (st_m & UMPA_ST_OK) C.ok++;
            else if (st_m & UMPA_ST_BOUND) C.bound++;
            else if (n_m < cap) C.move_capped++;                 // status 0 below the call cap: UMPA_MOVE_CAP
            else C.capped++;
            if (image == 2) C.ties++;
            bool good = st_or == st_m && n_or == n_m && same(v_or, v_m, kind == 1 ? 5 : 4) && same(uv_or, uv_m, 2) && same(d_or, d_m, 25);
            if (st_m & UMPA_ST_OK) good = good && same(a_or, a_m, 16);
            else for (int q = 0; q < 16; q++) good = good && a_m[q] == 0.0;
            if (!good) {
                C.bad++;
                if (printed++ < 10) {
                    fprintf(stderr, "MISMATCH kind %d ref_mode %d Na %d Nw %d ms %d image %d rep %d cap %d pixel (%d,%d) start (%g,%g): "
                            "status %d / %d, Ncalls %d / %d, f %g / %g, T %g / %g, uv (%g,%g) / (%g,%g)\n",
                            kind, ref_mode, Na, Nw, ms, image, rep, cap, i, j, u0, u1, st_or, st_m, n_or, n_m, v_or[0], v_m[0], v_or[1], v_m[1],
                            uv_or[0], uv_or[1], uv_m[0], uv_m[1]);
                    for (int q = 0; q < 25; q++) if (memcmp(&d_or[q], &d_m[q], 8)) fprintf(stderr, "   d[%d] %g / %g\n", q, d_or[q], d_m[q]);
                    for (int q = 0; q < 16; q++) if (memcmp(&a_or[q], &a_m[q], 8)) fprintf(stderr, "   a[%d] %g / %g\n", q, a_or[q], a_m[q]);
                }
            }
        }
        umpaor_destroy(model);
    }
    printf("walks %ld calls %ld ok %ld bound %ld call_capped %ld move_capped %ld restarts %ld second_deliveries %ld nan_walks %ld tie_walks %ld mismatches %ld\n",
           C.walks, C.calls, C.ok, C.bound, C.capped, C.move_capped, C.restarts, C.second, C.nan_walks, C.ties, C.bad);
    return C.bad ? 1 : 0;
}
