// Test helper (never loaded by the product): a CALLER's side of a HIP stream, for tests/test_gpu_caller_stream.py.
// Streams and events of the caller's own, a kernel that keeps a stream busy for a given time, the caller's "own work"
// behind a search (a device-side copy and a fill, plain vector code), and a host read that is NOT ordered behind a
// non-blocking stream.  Every entry point returns the hipError_t as an int (0 = success) unless it says otherwise.
#include <hip/hip_runtime.h>

#include <stdint.h>

namespace {

// The delay's hard bound, whatever the clock does: 8 iterations per microsecond asked for.  An iteration is an
// s_sleep of 8 x 64 cycles (0.2 us at the highest shader clock) and a clock read, 0.2 to 0.3 us in all, so the cap
// lies at 1.7 to 2.4 times the time asked for: it never cuts a delay short, and 20 ms asked for end within 50 ms.
constexpr unsigned long long kBusyItersPerUs = 8;
constexpr int kBusyMaxUs = 20000;

// one wave: reads the constant-rate clock until `ticks` have passed or `cap` iterations were made
__global__ void __launch_bounds__(64) busy_kernel(unsigned long long ticks, unsigned long long cap)
{
    const unsigned long long t0 = wall_clock64();
    for (unsigned long long i = 0; i < cap && wall_clock64() - t0 < ticks; i++) __builtin_amdgcn_s_sleep(8);
}

__global__ void __launch_bounds__(256) copy_kernel(int32_t *dst, const int32_t *src, size_t n)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) dst[i] = src[i];
}

__global__ void __launch_bounds__(256) fill_kernel(int32_t *dst, int32_t value, size_t n)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) dst[i] = value;
}

unsigned blocks_for(size_t n)
{
    const size_t b = (n + 255) / 256;
    return (unsigned)(b < 1 ? 1 : (b > 1024 ? 1024 : b));
}

}  // namespace

extern "C" {

// blocking != 0: hipStreamCreate (takes part in the default stream's implicit ordering); 0: hipStreamNonBlocking
int stream_create(int blocking, void **out)
{
    hipStream_t s = nullptr;
    const hipError_t e = blocking ? hipStreamCreate(&s) : hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
    *out = s;
    return (int)e;
}

int stream_destroy(void *stream) { return (int)hipStreamDestroy(static_cast<hipStream_t>(stream)); }

int stream_sync(void *stream) { return (int)hipStreamSynchronize(static_cast<hipStream_t>(stream)); }

// keep `stream` busy for `microseconds` (1..20000); -1: out of that range
int busy(void *stream, int microseconds)
{
    if (microseconds < 1 || microseconds > kBusyMaxUs) return -1;
    int dev = 0, khz = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return (int)e;
    e = hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev);
    if (e != hipSuccess) return (int)e;
    if (khz <= 0) return -2;
    const unsigned long long ticks = (unsigned long long)microseconds * (unsigned long long)khz / 1000ull;
    hipLaunchKernelGGL(busy_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), ticks,
                       (unsigned long long)microseconds * kBusyItersPerUs);
    return (int)hipGetLastError();
}

int copy_i32(void *stream, int32_t *dst, const int32_t *src, size_t n)
{
    if (!n) return 0;
    hipLaunchKernelGGL(copy_kernel, dim3(blocks_for(n)), dim3(256), 0, static_cast<hipStream_t>(stream), dst, src, n);
    return (int)hipGetLastError();
}

int fill_i32(void *stream, int32_t *dst, int32_t value, size_t n)
{
    if (!n) return 0;
    hipLaunchKernelGGL(fill_kernel, dim3(blocks_for(n)), dim3(256), 0, static_cast<hipStream_t>(stream), dst, value, n);
    return (int)hipGetLastError();
}

int event_create(void **out)
{
    hipEvent_t ev = nullptr;
    const hipError_t e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
    *out = ev;
    return (int)e;
}

int event_record(void *event, void *stream) { return (int)hipEventRecord(static_cast<hipEvent_t>(event), static_cast<hipStream_t>(stream)); }

int event_sync(void *event) { return (int)hipEventSynchronize(static_cast<hipEvent_t>(event)); }

int event_destroy(void *event) { return (int)hipEventDestroy(static_cast<hipEvent_t>(event)); }

int alloc_i32(size_t n, int32_t **out)
{
    *out = nullptr;
    return (int)hipMalloc(reinterpret_cast<void **>(out), (n ? n : 1) * sizeof(int32_t));
}

int free_i32(int32_t *p) { return (int)hipFree(p); }

// the size in bytes of the device allocation that holds `p`
int alloc_bytes(const void *p, size_t *out)
{
    hipDeviceptr_t base = nullptr;
    *out = 0;
    return (int)hipMemGetAddressRange(&base, out, const_cast<void *>(p));
}

// a plain synchronous copy to the host: ordered behind the default stream and blocking streams, NOT behind a
// non-blocking one
int read_unordered(int32_t *dst_host, const int32_t *src, size_t n)
{
    return (int)hipMemcpy(dst_host, src, n * sizeof(int32_t), hipMemcpyDeviceToHost);
}

}  // extern "C"
