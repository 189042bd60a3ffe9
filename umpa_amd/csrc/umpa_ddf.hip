// umpa_ddf.hip -- libumpa_ddf.so: the whole-image 17 x 17 blur and the candidate fold of the directional dark-field search
// (include/umpa_ddf.h).  gfx950 only.
//
// A sixth library beside libumpa_hip.so, libumpa_grid.so, libumpa_unwarp.so, libumpa_register.so and libumpa_integrate.so,
// for the same reason those have their own: the other libraries' kernel sets stay what they are.
// Two kernel families:
//   ddf_blur_kernel<VEC>   out = g * in on the interior, in copied on the border; one launch for up to 32 frames
//   ddf_fold_kernel        one candidate's planes into the running best, one lane per pixel
// The operations are defined in the public header.  No CPU fallback.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/umpa_ddf.h"
#include "umpa_host.h"

namespace umpa {

constexpr int TAPS = UMPA_DDF_TAPS, HALF = UMPA_DDF_HALF;
constexpr int TH = 32, TW = 64;                    // the output tile of a workgroup
constexpr int RUN = 8;                             // adjacent outputs of one lane, in one row
constexpr int SH = TH + 2 * HALF, SW = TW + 2 * HALF;  // the staged tile with its halo: 48 x 80
constexpr int PITCH = SW + 2;                      // 82 doubles: see MAPPING
constexpr int LDS_DOUBLES = SH * PITCH;            // 31488 bytes
static_assert(TH * (TW / RUN) == 256, "one lane per run of the tile");
static_assert(PITCH % 2 == 0 && (PITCH / 2) % 2 == 1, "rows 16-byte aligned, an odd number of 16-byte units apart");

struct DdfCoef { double g[TAPS * TAPS]; };         // 2312 bytes of kernel argument: wave-uniform scalar operands
struct DdfFrames { const double* in[UMPA_DDF_MAX_FRAMES]; double* out[UMPA_DDF_MAX_FRAMES]; };

// MAPPING.  A workgroup of 256 threads takes one 32 x 64 tile of one frame (blockIdx: tile column, tile row, frame; the
// tiles cover the WHOLE frame, the border pixels are copied by the lanes that own them).  It stages the tile with a halo
// of 8 in LDS, 48 rows of 80 doubles at a row pitch of 82; a pixel outside the frame is replaced by the nearest one inside
// (clamped staging: nothing outside the frame is read, and such a value only ever reaches outputs that are not stored).
// Lane t owns the RUN = 8 adjacent outputs of row t / 8 that start at column 8 (t % 8).  Per kernel row it reads the 24
// staged values under them (12 ds_read_b128) for 17 * 8 fused multiply-adds whose coefficient is a scalar operand.
// BANKS.  A ds_read_b128 is served in four groups of 16 lanes, each group made of lanes of four different tile rows with
// four runs each (MI355X: {0-3, 12-15, 20-27}, ...).  The runs of one row lie 64 bytes apart, i.e. on the 16-byte bank slots
// 0, 4, 8, 12 (mod 16) -- with a row pitch that is a multiple of 64 bytes all 16 lanes of a group would share four slots, a
// four-way conflict.  The pitch of 82 doubles moves each tile row on by 41 slots = 9 (mod 16), odd, so the four rows of
// a group take the slots {0, 4, 8, 12} + {0, 1, 2, 3} (in some order): 16 different ones, no conflict.
// Nothing is added across lanes, there is no atomic: one bit pattern per output whatever the grid.
// VEC: the frames are 16-byte aligned and W is even, so global loads and stores are 16 bytes wide.
template <bool VEC>
__global__ void __launch_bounds__(256)
ddf_blur_kernel(const DdfFrames fr, const int H, const int W, const DdfCoef coef)
{
    __shared__ __attribute__((aligned(16))) double lds[LDS_DOUBLES];
    const int tid = threadIdx.x;
    const int y0 = blockIdx.y * TH, x0 = blockIdx.x * TW;
    const double* __restrict__ in = fr.in[blockIdx.z];
    double* __restrict__ out = fr.out[blockIdx.z];

    if (VEC) {
        for (int e = tid; e < SH * (SW / 2); e += 256) {
            const int yy = e / (SW / 2), xp = e - yy * (SW / 2);
            const int sy = min(max(y0 - HALF + yy, 0), H - 1);
            const int sx = min(max(x0 - HALF + 2 * xp, 0), W - 2);              // even: the pair is inside the row
            const double2 v = *reinterpret_cast<const double2*>(in + (size_t)sy * W + sx);
            *reinterpret_cast<double2*>(lds + yy * PITCH + 2 * xp) = v;
        }
    } else {
        for (int e = tid; e < SH * SW; e += 256) {
            const int yy = e / SW, xx = e - yy * SW;
            const int sy = min(max(y0 - HALF + yy, 0), H - 1);
            const int sx = min(max(x0 - HALF + xx, 0), W - 1);
            lds[yy * PITCH + xx] = in[(size_t)sy * W + sx];
        }
    }
    __syncthreads();

    const int ly = tid / (TW / RUN), cx = tid - ly * (TW / RUN);
    const int i = y0 + ly, j0 = x0 + RUN * cx;
    if (i >= H || j0 >= W) return;
    double acc[RUN];
#pragma unroll
    for (int r = 0; r < RUN; r++) acc[r] = 0.0;
#pragma unroll 1
    for (int k = 0; k < TAPS; k++) {
        const double2* row = reinterpret_cast<const double2*>(lds + (ly + k) * PITCH + RUN * cx);
        double v[RUN + 2 * HALF];
#pragma unroll
        for (int q = 0; q < (RUN + 2 * HALF) / 2; q++) {
            const double2 p = row[q];
            v[2 * q] = p.x; v[2 * q + 1] = p.y;
        }
        const double* gk = coef.g + k * TAPS;
#pragma unroll
        for (int l = 0; l < TAPS; l++) {
            const double gv = gk[l];
#pragma unroll
            for (int r = 0; r < RUN; r++) acc[r] = fma(gv, v[r + l], acc[r]);
        }
    }
    // the border keeps the input: its own staged value, bit for bit
    const bool rowin = i >= HALF && i < H - HALF;
    const double* centre = lds + (ly + HALF) * PITCH + RUN * cx + HALF;
#pragma unroll
    for (int r = 0; r < RUN; r++) {
        const int j = j0 + r;
        if (!(rowin && j >= HALF && j < W - HALF)) acc[r] = centre[r];
    }
    double* o = out + (size_t)i * W + j0;
    if (VEC) {
#pragma unroll
        for (int r = 0; r < RUN; r += 2)
            if (j0 + r < W) *reinterpret_cast<double2*>(o + r) = make_double2(acc[r], acc[r + 1]);   // W even: both or none
    } else {
#pragma unroll
        for (int r = 0; r < RUN; r++)
            if (j0 + r < W) o[r] = acc[r];
    }
}

// The fold of include/umpa_ddf.h, one lane per pixel.
__global__ void __launch_bounds__(256)
ddf_fold_kernel(const int m, const size_t N, const double* __restrict__ f, const double* __restrict__ T,
                const double* __restrict__ dx, const double* __restrict__ dy, const int* __restrict__ err,
                double* __restrict__ bf, double* __restrict__ bT, double* __restrict__ bdx, double* __restrict__ bdy,
                int* __restrict__ index, int* __restrict__ berr)
{
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= N) return;
    const bool ok = err[p] == 1;
    const double fm = f[p];
    int idx;
    bool take;
    if (m == 0) {
        idx = ok ? 0 : -1;
        take = true;
    } else {
        idx = index[p];
        take = ok && (idx < 0 || fm < bf[p]);
        if (take) idx = m;
    }
    if (take) { bf[p] = fm; bT[p] = T[p]; bdx[p] = dx[p]; bdy[p] = dy[p]; }
    index[p] = idx;
    berr[p] = idx >= 0 ? 1 : 0;
}

} // namespace umpa

using namespace umpa;

#define UMPA_DDF_API extern "C" __attribute__((visibility("default")))

namespace {

// Up to UMPA_DDF_MAX_FRAMES device frames per launch.
hipError_t launch_blur(const double* const* in, double* const* out, int K, int H, int W, const DdfCoef& coef, hipStream_t s)
{
    const dim3 block(256);
    for (int k0 = 0; k0 < K; k0 += UMPA_DDF_MAX_FRAMES) {
        const int n = K - k0 < UMPA_DDF_MAX_FRAMES ? K - k0 : UMPA_DDF_MAX_FRAMES;
        DdfFrames fr;
        memset(&fr, 0, sizeof(fr));
        bool vec = W % 2 == 0;
        for (int k = 0; k < n; k++) {
            fr.in[k] = in[k0 + k]; fr.out[k] = out[k0 + k];
            vec = vec && ((uintptr_t)fr.in[k] % 16 == 0) && ((uintptr_t)fr.out[k] % 16 == 0);
        }
        const dim3 grid((W + TW - 1) / TW, (H + TH - 1) / TH, n);
        if (vec) hipLaunchKernelGGL(ddf_blur_kernel<true>, grid, block, 0, s, fr, H, W, coef);
        else hipLaunchKernelGGL(ddf_blur_kernel<false>, grid, block, 0, s, fr, H, W, coef);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

} // namespace

UMPA_DDF_API const char* umpa_ddf_last_error(void) { return g_err.c_str(); }

UMPA_DDF_API int umpa_ddf_kernel(double a, double b, double c, double* out)
{
    if (!out) return fail(UMPA_HIP_E_ARG, "ddf: null argument");
    if (!std::isfinite(a) || !std::isfinite(b) || !std::isfinite(c))
        return fail(UMPA_HIP_E_ARG, "ddf: the candidate (%g, %g, %g) is not finite", a, b, c);
    if (!(a > 0.0) || !(c > 0.0) || !(4.0 * a * c - b * b > 0.0))
        return fail(UMPA_HIP_E_ARG, "ddf: the candidate (%g, %g, %g) is no Gaussian: a > 0, c > 0 and 4 a c - b^2 > 0 are required", a, b, c);
    double norm = 0.0;
    for (int k = 0; k < TAPS; k++)
        for (int l = 0; l < TAPS; l++) {
            const double i = (double)(k - HALF), j = (double)(l - HALF);
            const double e = std::exp(-a * i * i - b * i * j - c * j * j);
            out[k * TAPS + l] = e;
            norm += e;
        }
    for (int q = 0; q < TAPS * TAPS; q++) out[q] /= norm;
    return 0;
}

UMPA_DDF_API int umpa_ddf_blur(const double* const* in, double* const* out, int K, int H, int W, const double* kern,
                               int device, int flags, void* stream)
{
    if (!in || !out || !kern) return fail(UMPA_HIP_E_ARG, "ddf: null argument");
    if (K < 0) return fail(UMPA_HIP_E_ARG, "ddf: K = %d", K);
    if (flags & ~UMPA_HIP_F_DEVICE_IO) return fail(UMPA_HIP_E_ARG, "ddf: blur takes UMPA_HIP_F_DEVICE_IO and no other flag");
    if (H < TAPS || W < TAPS)
        return fail(UMPA_HIP_E_ARG, "ddf: frames of %d x %d pixels are smaller than the %d x %d kernel", H, W, TAPS, TAPS);
    if ((H + TH - 1) / TH > 65535) return fail(UMPA_HIP_E_UNSUPPORTED, "ddf: frames of %d rows (at most %d)", H, 65535 * TH);
    for (int q = 0; q < TAPS * TAPS; q++)
        if (!std::isfinite(kern[q])) return fail(UMPA_HIP_E_ARG, "ddf: kernel entry (%d, %d) is not finite", q / TAPS, q % TAPS);
    const size_t n = (size_t)H * W;
    for (int k = 0; k < K; k++) {
        if (!in[k] || !out[k]) return fail(UMPA_HIP_E_ARG, "ddf: frame %d is null", k);
        for (int q = 0; q < K; q++) {
            const char* a = (const char*)in[k];
            const char* b = (const char*)out[q];
            if (a < b + n * 8 && b < a + n * 8) return fail(UMPA_HIP_E_ARG, "ddf: input frame %d and output frame %d overlap (in and out may not alias)", k, q);
        }
    }
    if (int rc = pick_device("ddf", device)) return rc;
    if (K == 0) return 0;
    DdfCoef coef;
    memcpy(coef.g, kern, sizeof(coef.g));
    if (flags & UMPA_HIP_F_DEVICE_IO) {
        hipStream_t s = (hipStream_t)stream;
        HIPOK(launch_blur(in, out, K, H, W, coef, s), UMPA_HIP_E_LAUNCH, "ddf: launch of the blur");
        HIPOK(hipStreamSynchronize(s), UMPA_HIP_E_LAUNCH, "ddf: blur");
        return 0;
    }
    // host arrays: device copies of up to UMPA_DDF_MAX_FRAMES frames at a time, on the null stream
    const int chunk = K < UMPA_DDF_MAX_FRAMES ? K : UMPA_DDF_MAX_FRAMES;
    DeviceMem S;
    HIPOK(S.alloc(0, n * 8 * chunk), UMPA_HIP_E_NOMEM, "ddf: device memory for %d frames", chunk);
    HIPOK(S.alloc(1, n * 8 * chunk), UMPA_HIP_E_NOMEM, "ddf: device memory for %d frames", chunk);
    for (int k0 = 0; k0 < K; k0 += chunk) {
        const int nk = K - k0 < chunk ? K - k0 : chunk;
        const double* din[UMPA_DDF_MAX_FRAMES];
        double* dout[UMPA_DDF_MAX_FRAMES];
        for (int k = 0; k < nk; k++) {
            din[k] = (const double*)S.p[0] + (size_t)k * n;
            dout[k] = (double*)S.p[1] + (size_t)k * n;
            HIPOK(hipMemcpy((void*)din[k], in[k0 + k], n * 8, hipMemcpyHostToDevice), UMPA_HIP_E_DEVICE, "ddf: upload of frame %d", k0 + k);
        }
        HIPOK(launch_blur(din, dout, nk, H, W, coef, nullptr), UMPA_HIP_E_LAUNCH, "ddf: launch of the blur");
        for (int k = 0; k < nk; k++)
            HIPOK(hipMemcpy(out[k0 + k], dout[k], n * 8, hipMemcpyDeviceToHost), UMPA_HIP_E_LAUNCH, "ddf: blur of frame %d", k0 + k);
    }
    return 0;
}

UMPA_DDF_API int umpa_ddf_fold(int m, long long N, const double* f, const double* T, const double* dx, const double* dy, const int* err,
                               double* best_f, double* best_T, double* best_dx, double* best_dy, int* index, int* best_err,
                               int device, int flags, void* stream)
{
    if (!f || !T || !dx || !dy || !err || !best_f || !best_T || !best_dx || !best_dy || !index || !best_err)
        return fail(UMPA_HIP_E_ARG, "ddf: null argument");
    if (m < 0) return fail(UMPA_HIP_E_ARG, "ddf: candidate number %d", m);
    if (N < 0 || N >= (1LL << 31) * 256) return fail(UMPA_HIP_E_ARG, "ddf: planes of %lld pixels", N);
    if (flags & ~UMPA_HIP_F_DEVICE_IO) return fail(UMPA_HIP_E_ARG, "ddf: fold takes UMPA_HIP_F_DEVICE_IO and no other flag");
    if (int rc = pick_device("ddf", device)) return rc;
    if (N == 0) return 0;
    const size_t n = (size_t)N;
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    if (flags & UMPA_HIP_F_DEVICE_IO) {
        hipStream_t s = (hipStream_t)stream;
        hipLaunchKernelGGL(ddf_fold_kernel, grid, block, 0, s, m, n, f, T, dx, dy, err, best_f, best_T, best_dx, best_dy, index, best_err);
        LAUNCHED("ddf: launch of the fold");
        HIPOK(hipStreamSynchronize(s), UMPA_HIP_E_LAUNCH, "ddf: fold");
        return 0;
    }
    // host arrays: 0-3 the candidate's doubles, 4 its err, 5-8 the best's doubles, 9 index, 10 the best's err
    DeviceMem S;
    const void* src[11] = {f, T, dx, dy, err, best_f, best_T, best_dx, best_dy, index, best_err};
    void* dst[11] = {nullptr, nullptr, nullptr, nullptr, nullptr, best_f, best_T, best_dx, best_dy, index, best_err};
    for (int q = 0; q < 11; q++) {
        const size_t bytes = n * ((q == 4 || q >= 9) ? 4 : 8);
        HIPOK(S.alloc(q, bytes), UMPA_HIP_E_NOMEM, "ddf: device memory for the fold");
        if (q < 5 || (m > 0 && q < 10))                        // candidate 0 initialises the best planes: nothing of them is read
            HIPOK(hipMemcpy(S.p[q], src[q], bytes, hipMemcpyHostToDevice), UMPA_HIP_E_DEVICE, "ddf: upload of the fold's planes");
    }
    hipLaunchKernelGGL(ddf_fold_kernel, grid, block, 0, nullptr, m, n, (const double*)S.p[0], (const double*)S.p[1], (const double*)S.p[2],
                       (const double*)S.p[3], (const int*)S.p[4], (double*)S.p[5], (double*)S.p[6], (double*)S.p[7], (double*)S.p[8],
                       (int*)S.p[9], (int*)S.p[10]);
    LAUNCHED("ddf: launch of the fold");
    for (int q = 5; q < 11; q++)
        HIPOK(hipMemcpy(dst[q], S.p[q], n * (q >= 9 ? 4 : 8), hipMemcpyDeviceToHost), UMPA_HIP_E_LAUNCH, "ddf: fold");
    return 0;
}
