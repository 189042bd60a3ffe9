// umpa_host.h -- the host scaffold every translation unit of umpa_amd/csrc shares: the error state behind
// umpa_<lib>_last_error(), device selection, the device memory of one call, the checks of HIP calls and of weights.
// Host code only: no kernel, no __device__ function.  Everything is in an anonymous namespace, so each library has its own
// copy (its own error string, as before) and exports nothing of it.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <string>

#include "../../include/umpa_hip.h"

namespace {

thread_local std::string g_err;       // what umpa_<lib>_last_error() of this library returns

// Sets the error text (at most 511 bytes, a longer one is cut) and returns `code`.
inline int fail(int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

// `return fail(code, "<fmt>: <HIP's error string>", ...)` from the calling function unless `call` gives hipSuccess.  `fmt`
// is a literal that starts with the library's tag ("ddf: upload of frame %d"); LAUNCHED asks hipGetLastError().
#define HIPOK(call, code, fmt, ...) do { const hipError_t e_ = (call); if (e_ != hipSuccess) return fail(code, fmt ": %s", ##__VA_ARGS__, hipGetErrorString(e_)); } while (0)
#define LAUNCHED(fmt, ...) HIPOK(hipGetLastError(), UMPA_HIP_E_LAUNCH, fmt, ##__VA_ARGS__)

// Makes `device` the calling thread's device: 0, or a failure whose text names the library (`what`).
inline int pick_device(const char* what, int device)
{
    const int ndev = umpa_hip_device_count();
    if (ndev < 1) return fail(UMPA_HIP_E_DEVICE, "no HIP device available (this library has no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(UMPA_HIP_E_ARG, "device %d out of range (%d devices)", device, ndev);
    const hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) return fail(UMPA_HIP_E_DEVICE, "%s: hipSetDevice(%d): %s", what, device, hipGetErrorString(e));
    return 0;
}

// The device memory of one call, in numbered slots; freed when the call returns.  A slot whose allocation failed stays empty.
struct DeviceMem {
    void* p[12] = {};
    DeviceMem() = default;
    DeviceMem(const DeviceMem&) = delete;
    DeviceMem& operator=(const DeviceMem&) = delete;
    ~DeviceMem() { for (void* q : p) if (q) (void)hipFree(q); }
    hipError_t alloc(int slot, size_t bytes)
    {
        const hipError_t e = hipMalloc(&p[slot], bytes);
        if (e != hipSuccess) p[slot] = nullptr;
        return e;
    }
};

// The index of the first of `n` weights that is not finite and >= 0; `n` when all are.
inline size_t bad_weight(const double* w, size_t n)
{
    for (size_t i = 0; i < n; i++)
        if (!(w[i] >= 0.0) || !std::isfinite(w[i])) return i;
    return n;
}

// bytes per pixel of the frame dtype codes of the C ABI: 0 float64, 1 float32, 2 uint16
inline size_t dtype_size(int code) { return code == 0 ? 8 : code == 1 ? 4 : 2; }

} // namespace
