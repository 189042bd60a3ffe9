// umpa_unwarp.hip -- libumpa_unwarp.so: detector distortion correction (include/umpa_unwarp.h).  gfx950 only.
//
// A third library beside libumpa_hip.so and libumpa_grid.so, for the same reason the grid search has its own (DESIGN.md
// section 4.8): the main library's kernel set stays what it is.  It holds one kernel family, unwarp_kernel<RAW, INTERP>
// (three raw dtypes x two interpolation kinds), the stand-alone call that launches it on the caller's frames, and the
// stage filter (umpa_hipx.h) through which umpa_hip_stage_sample launches it instead of flat_correct_kernel.  The
// operation is defined in the public header, expression by expression; this file restates nothing, it evaluates them.
// No CPU fallback.
#include <hip/hip_runtime.h>
#include <atomic>
#include <cmath>
#include <cstring>

#include "../../include/umpa_unwarp.h"
#include "umpa_host.h"
#define UMPA_HIPX_STAGE_ONLY          // the stage filter alone: none of the tiled path's structs, none of its kernels
#include "umpa_hipx.h"
#include "umpa_walk.h"                // UMPA_GLOBAL, gp, gpw

#pragma clang fp contract(off)

namespace umpa {

// One output pixel per lane, pixels numbered row-major across the whole frame (no idle lanes at a row's end): a wave
// reads 256 contiguous bytes of each map plane, 512 of dark and of flat, and stores 512 contiguous bytes -- each the
// full-rate shape of a wave-instruction -- and its taps, for the smooth maps detectors have, are runs of 64 neighbouring
// samples per tap row that the next tap column and the next tap row find in L1 / L2.  Algorithmic bytes per pixel:
// 8 (map) + 2..8 (raw) + 0..16 (dark, flat) + 8 (store); the 4 or 16 tap loads per lane are cache traffic.
//
// Variants considered and not taken:
//   * two or four pixels per lane with 16-byte map loads and stores: the frames of a model sit back to back in one
//     allocation and W may be odd, so neither a row nor a frame starts 16-byte aligned in general; a variant that is
//     only legal for some shapes would be a second path to test for a kernel that is expected to be bound by its tap
//     gathers' cache traffic, not by the width of its contiguous accesses.  NOT MEASURED.
//   * staging the tap rows of a block in LDS: the footprint of a block depends on the map (it is data), so the tile
//     would have to be sized for the worst displacement gradient or fall back; the caches do this without a bound.
//     NOT MEASURED.
//   * a (64, 4) block over a 2-D tile of the output, to share tap rows between the waves of a block: 256 consecutive
//     pixels of one row already share every tap row among the block's four waves' neighbours in L2.  NOT MEASURED.
template <class RAW, int INTERP>
__global__ void __launch_bounds__(256)
unwarp_kernel(const RAW* __restrict__ raw, const float* __restrict__ d0, const float* __restrict__ d1,
              const double* __restrict__ dark, const double* __restrict__ flat, double* __restrict__ out, int H, int W)
{
    const unsigned q = blockIdx.x * 256u + threadIdx.x, n = (unsigned)H * (unsigned)W;     // H * W < 2^31 (map_create)
    if (q >= n) return;
    const int i = (int)(q / (unsigned)W), j = (int)(q - (unsigned)i * (unsigned)W);
    const double y = (double)i + (double)gp(d0)[q], x = (double)j + (double)gp(d1)[q];
    const double yf = floor(y), xf = floor(x);
    const double fy = y - yf, fx = x - xf;
    // the tap indices are clamped into the frame anyway: bring the base into int range first (a map value of 1e30 is
    // legal and reads the edge pixel), four pixels beyond the frame so that every tap's own clamp still decides
    const int i0 = (int)fmin(fmax(yf, -4.0), (double)H + 4.0), j0 = (int)fmin(fmax(xf, -4.0), (double)W + 4.0);
    const UMPA_GLOBAL RAW* __restrict__ r = gp(raw);
    double u;
    if (INTERP == UMPA_UNWARP_LINEAR) {
        const size_t ra = (size_t)min(max(i0, 0), H - 1) * W, rb = (size_t)min(max(i0 + 1, 0), H - 1) * W;
        const int ca = min(max(j0, 0), W - 1), cb = min(max(j0 + 1, 0), W - 1);
        const double v00 = (double)r[ra + ca], v01 = (double)r[ra + cb], v10 = (double)r[rb + ca], v11 = (double)r[rb + cb];
        u = (1.0 - fy) * ((1.0 - fx) * v00 + fx * v01) + fy * ((1.0 - fx) * v10 + fx * v11);
    } else {
        double wx[4], wy[4];
        wx[0] = ((-fx + 2.0) * fx - 1.0) * fx / 2.0;
        wx[1] = ((3.0 * fx - 5.0) * fx * fx + 2.0) / 2.0;
        wx[2] = ((-3.0 * fx + 4.0) * fx + 1.0) * fx / 2.0;
        wx[3] = (fx - 1.0) * fx * fx / 2.0;
        wy[0] = ((-fy + 2.0) * fy - 1.0) * fy / 2.0;
        wy[1] = ((3.0 * fy - 5.0) * fy * fy + 2.0) / 2.0;
        wy[2] = ((-3.0 * fy + 4.0) * fy + 1.0) * fy / 2.0;
        wy[3] = (fy - 1.0) * fy * fy / 2.0;
        int c[4];
#pragma unroll
        for (int b = 0; b < 4; b++) c[b] = min(max(j0 - 1 + b, 0), W - 1);
        u = 0.0;
#pragma unroll
        for (int a = 0; a < 4; a++) {
            const size_t ro = (size_t)min(max(i0 - 1 + a, 0), H - 1) * W;
            double s = wx[0] * (double)r[ro + c[0]];
            s = s + wx[1] * (double)r[ro + c[1]];
            s = s + wx[2] * (double)r[ro + c[2]];
            s = s + wx[3] * (double)r[ro + c[3]];
            u = a == 0 ? wy[0] * s : u + wy[a] * s;
        }
    }
    if (dark) u = u - gp(dark)[q];
    if (flat) u = u / gp(flat)[q];
    gpw(out)[q] = u;
}

} // namespace umpa

using namespace umpa;

#define UMPA_UNWARP_API extern "C" __attribute__((visibility("default")))

// The device planes of a map, counted: the caller's handle holds one reference, every model the map is attached to holds
// one (dropped by the stage filter's release call: detach, replacement, umpa_hip_destroy).  Freed with the last one.
struct umpa_unwarp_map {
    int H = 0, W = 0, interp = 0, device = 0;
    float* d = nullptr;                       // d0 then d1, one allocation
    std::atomic<int> refs{1};
};

namespace {

void unref(umpa_unwarp_map* map)
{
    if (map->refs.fetch_sub(1) != 1) return;
    if (map->d) {
        // frees of this runtime wait for the device's work; the device of the calling thread is put back
        int cur = -1;
        const bool have = hipGetDevice(&cur) == hipSuccess;
        if (hipSetDevice(map->device) == hipSuccess) (void)hipFree(map->d);
        if (have) (void)hipSetDevice(cur);
    }
    delete map;
}

template <class RAW>
void launch_dtype(const umpa_unwarp_map& M, const void* raw, const double* dark, const double* flat, double* out, hipStream_t s)
{
    const unsigned n = (unsigned)M.H * (unsigned)M.W, grid = (n + 255u) / 256u;
    const float* d0 = M.d;
    const float* d1 = M.d + (size_t)n;
    if (M.interp == UMPA_UNWARP_LINEAR)
        hipLaunchKernelGGL((unwarp_kernel<RAW, UMPA_UNWARP_LINEAR>), dim3(grid), dim3(256), 0, s, (const RAW*)raw, d0, d1, dark, flat, out, M.H, M.W);
    else
        hipLaunchKernelGGL((unwarp_kernel<RAW, UMPA_UNWARP_CUBIC>), dim3(grid), dim3(256), 0, s, (const RAW*)raw, d0, d1, dark, flat, out, M.H, M.W);
}

// one frame: raw, dark, flat, out are device arrays of the map's device
hipError_t launch(const umpa_unwarp_map& M, const void* raw, int raw_dtype, const double* dark, const double* flat, double* out, hipStream_t s)
{
    if (raw_dtype == 0) launch_dtype<double>(M, raw, dark, flat, out, s);
    else if (raw_dtype == 1) launch_dtype<float>(M, raw, dark, flat, out, s);
    else launch_dtype<unsigned short>(M, raw, dark, flat, out, s);
    return hipGetLastError();
}

// umpa::StageFilter (umpa_hipx.h): umpa_hip_stage_sample calls this where it would launch flat_correct_kernel
int stage_filter(void* user, int k, const void* staged_raw, int raw_dtype, const double* dark_k, const double* flat_k,
                 double* out_k, int H, int W, hipStream_t upload_stream)
{
    umpa_unwarp_map* map = (umpa_unwarp_map*)user;
    if (k < 0) { unref(map); return 0; }                                   // the model lets go of the filter
    if (H != map->H || W != map->W) return UMPA_HIP_E_UNSUPPORTED;         // (checked at attach; a model's shapes are fixed)
    return launch(*map, staged_raw, raw_dtype, dark_k, flat_k, out_k, upload_stream) == hipSuccess ? 0 : UMPA_HIP_E_LAUNCH;
}

} // namespace

UMPA_UNWARP_API const char* umpa_unwarp_last_error(void) { return g_err.c_str(); }

UMPA_UNWARP_API umpa_unwarp_map* umpa_unwarp_map_create(int H, int W, const float* d0, const float* d1, int interp, int device)
{
    if (!d0 || !d1) { fail(UMPA_HIP_E_ARG, "unwarp: null map plane"); return nullptr; }
    if (H < 1 || W < 1 || (long long)H * W >= (1LL << 31)) { fail(UMPA_HIP_E_ARG, "unwarp: a map of %d x %d pixels (H * W must be in [1, 2^31))", H, W); return nullptr; }
    if (interp != UMPA_UNWARP_LINEAR && interp != UMPA_UNWARP_CUBIC) { fail(UMPA_HIP_E_ARG, "unwarp: interpolation kind %d (0 linear, 1 cubic)", interp); return nullptr; }
    const size_t n = (size_t)H * W;
    for (size_t q = 0; q < n; q++)
        if (!std::isfinite(d0[q]) || !std::isfinite(d1[q])) {
            fail(UMPA_HIP_E_ARG, "unwarp: the map is not finite at pixel (%d, %d)", (int)(q / W), (int)(q % W));
            return nullptr;
        }
    if (pick_device("unwarp", device) < 0) return nullptr;
    umpa_unwarp_map* map = new umpa_unwarp_map;
    map->H = H; map->W = W; map->interp = interp; map->device = device;
    hipError_t e = hipMalloc((void**)&map->d, 2 * n * sizeof(float));
    if (e != hipSuccess) { map->d = nullptr; fail(UMPA_HIP_E_NOMEM, "unwarp: device memory for the map: %s", hipGetErrorString(e)); delete map; return nullptr; }
    e = hipMemcpy(map->d, d0, n * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(map->d + n, d1, n * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) { fail(UMPA_HIP_E_DEVICE, "unwarp: upload of the map: %s", hipGetErrorString(e)); unref(map); return nullptr; }
    return map;
}

UMPA_UNWARP_API void umpa_unwarp_map_destroy(umpa_unwarp_map* map)
{
    if (map) unref(map);
}

UMPA_UNWARP_API int umpa_unwarp_frames(umpa_unwarp_map* map, const void* const* raw, int raw_dtype, int K,
                                       const double* const* dark, const double* const* flat, double* const* out,
                                       int flags, void* stream)
{
    if (!map || !raw || !out) return fail(UMPA_HIP_E_ARG, "unwarp: null argument");
    if (raw_dtype < 0 || raw_dtype > 2) return fail(UMPA_HIP_E_ARG, "unwarp: raw_dtype %d: 0 float64, 1 float32, 2 uint16", raw_dtype);
    if (K < 0) return fail(UMPA_HIP_E_ARG, "unwarp: K = %d", K);
    if (flags & ~UMPA_HIP_F_DEVICE_IO) return fail(UMPA_HIP_E_ARG, "unwarp: frames takes UMPA_HIP_F_DEVICE_IO and no other flag");
    for (int k = 0; k < K; k++)
        if (!raw[k] || !out[k] || (dark && !dark[k]) || (flat && !flat[k])) return fail(UMPA_HIP_E_ARG, "unwarp: null frame %d", k);
    HIPOK(hipSetDevice(map->device), UMPA_HIP_E_DEVICE, "unwarp: hipSetDevice(%d)", map->device);    // (the map's device: it was counted at map_create)
    if (flags & UMPA_HIP_F_DEVICE_IO) {
        for (int k = 0; k < K; k++)
            HIPOK(launch(*map, raw[k], raw_dtype, dark ? dark[k] : nullptr, flat ? flat[k] : nullptr, out[k], (hipStream_t)stream),
                  UMPA_HIP_E_LAUNCH, "unwarp: launch of frame %d", k);
        return 0;
    }
    // host arrays: device copies of one frame's arrays, frame after frame on the null stream (a call made once per
    // calibration set, not the streaming path: that is umpa_unwarp_attach)
    const size_t n = (size_t)map->H * map->W, esz = dtype_size(raw_dtype);
    DeviceMem S;
    const size_t bytes[4] = {n * esz, n * 8, dark ? n * 8 : 0, flat ? n * 8 : 0};      // raw, out, dark, flat
    for (int q = 0; q < 4; q++)
        if (bytes[q]) HIPOK(S.alloc(q, bytes[q]), UMPA_HIP_E_NOMEM, "unwarp: device memory for a frame");
    for (int k = 0; k < K; k++) {
        HIPOK(hipMemcpy(S.p[0], raw[k], bytes[0], hipMemcpyHostToDevice), UMPA_HIP_E_DEVICE, "unwarp: upload of frame %d", k);
        if (dark) HIPOK(hipMemcpy(S.p[2], dark[k], bytes[2], hipMemcpyHostToDevice), UMPA_HIP_E_DEVICE, "unwarp: upload of frame %d", k);
        if (flat) HIPOK(hipMemcpy(S.p[3], flat[k], bytes[3], hipMemcpyHostToDevice), UMPA_HIP_E_DEVICE, "unwarp: upload of frame %d", k);
        HIPOK(launch(*map, S.p[0], raw_dtype, (const double*)S.p[2], (const double*)S.p[3], (double*)S.p[1], nullptr), UMPA_HIP_E_LAUNCH, "unwarp: launch of frame %d", k);
        HIPOK(hipMemcpy(out[k], S.p[1], bytes[1], hipMemcpyDeviceToHost), UMPA_HIP_E_LAUNCH, "unwarp: frame %d", k);
    }
    return 0;
}

UMPA_UNWARP_API int umpa_unwarp_attach(umpa_hip_model* m, umpa_unwarp_map* map)
{
    if (!m) return fail(UMPA_HIP_E_ARG, "unwarp: null model");
    if (!map) {
        const int rc = umpa_hipx_set_stage_filter(m, nullptr, nullptr, 0, 0, 0);
        return rc < 0 ? fail(rc, "unwarp: %s", umpa_hip_last_error()) : 0;
    }
    // the model's reference first: the setter releases an earlier filter (possibly this very map) before it installs
    map->refs.fetch_add(1);
    const int rc = umpa_hipx_set_stage_filter(m, stage_filter, map, map->H, map->W, map->device);
    if (rc < 0) { unref(map); return fail(rc, "unwarp: %s", umpa_hip_last_error()); }
    return 0;
}
