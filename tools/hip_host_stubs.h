// hip_host_stubs.h -- the HIP runtime calls behind csrc/device_buf.h, csrc/ingest_fill.h, csrc/canvas_band.h and csrc/tile_table.h, defined
// over malloc / free / memcpy for the sanitizer-built host checks (device_buf_host_check.cpp, arena_layout_host_check.cpp,
// ingest_fill_host_check.cpp, canvas_band_host_check.cpp, tile_table_host_check.cpp): no GPU, no HIP runtime
// at work, and ASan / LeakSanitizer see every "device" allocation and every "copy".  Include it in exactly one translation unit of a program.
// Every call is logged (`sync(stream)`, `free(ptr)`, `malloc(n)`, `copy(dst)`, `record(event)`, `wait(event)`, `stream_wait(event)`, ...), live allocations and
// events are counted, and two injections make calls fail (a failing call is logged all the same): fail_at = N, the N-th allocation of either
// kind from now; fail_call(kind, N), the N-th call of that kind from now -- "hipMalloc", "hipHostMalloc", "copy", "sync", "record",
// "wait", "stream_wait", "event_create".  A failed call leaves the runtime's sticky error behind until hipGetLastError takes it.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

struct HipStubs {
    std::vector<std::string> log; long live = 0; long fail_at = 0;
    const char *fail_kind = nullptr; long fail_kind_at = 0;      // fail_call
    long events = 0; hipError_t sticky = hipSuccess;
    void (*probe)() = nullptr;                                    // called inside every synchronising call, behind its log line
};
static HipStubs g_hip;

static void fail_call(const char *kind, long n) { g_hip.fail_kind = kind; g_hip.fail_kind_at = n; }
static bool stub_fails(const char *kind)
{
    if (!g_hip.fail_kind || strcmp(g_hip.fail_kind, kind) || --g_hip.fail_kind_at != 0) return false;
    g_hip.fail_kind = nullptr;
    return true;
}
static std::string stub_name(const char *what, const void *p) { char line[64]; snprintf(line, sizeof(line), "%s(%p)", what, p); return line; }
static hipError_t stub_call(const char *kind, const void *p, bool synchronises = false)
{
    g_hip.log.push_back(stub_name(kind, p));
    if (synchronises && g_hip.probe) g_hip.probe();
    return stub_fails(kind) ? (g_hip.sticky = hipErrorUnknown) : hipSuccess;
}
static hipError_t stub_alloc(void **p, size_t n, const char *kind)
{
    char line[64];
    snprintf(line, sizeof(line), "malloc(%zu)", n);
    g_hip.log.push_back(line);
    *p = nullptr;
    const bool by_kind = stub_fails(kind);
    if (by_kind || (g_hip.fail_at && --g_hip.fail_at == 0)) return g_hip.sticky = hipErrorOutOfMemory;
    *p = malloc(n ? n : 1);
    g_hip.live++;
    return hipSuccess;
}
static hipError_t stub_free(void *p)
{
    if (!p) return hipSuccess;
    g_hip.log.push_back(stub_name("free", p));
    free(p);
    g_hip.live--;
    return hipSuccess;
}
extern "C" {
hipError_t hipMalloc(void **p, size_t n) { return stub_alloc(p, n, "hipMalloc"); }
hipError_t hipHostMalloc(void **p, size_t n, unsigned int) { return stub_alloc(p, n, "hipHostMalloc"); }
hipError_t hipFree(void *p) { return stub_free(p); }
hipError_t hipHostFree(void *p) { return stub_free(p); }
hipError_t hipStreamSynchronize(hipStream_t s) { return stub_call("sync", (const void *)s, true); }
hipError_t hipMemcpyAsync(void *dst, const void *src, size_t n, hipMemcpyKind, hipStream_t)
{
    const hipError_t e = stub_call("copy", dst);
    if (e == hipSuccess) memcpy(dst, src, n);
    return e;
}
hipError_t hipMemcpy2DAsync(void *dst, size_t dpitch, const void *src, size_t spitch, size_t width, size_t height, hipMemcpyKind, hipStream_t)
{
    const hipError_t e = stub_call("copy", dst);
    for (size_t y = 0; e == hipSuccess && y < height; y++) memcpy((char *)dst + y * dpitch, (const char *)src + y * spitch, width);
    return e;
}
hipError_t hipEventCreateWithFlags(hipEvent_t *ev, unsigned)
{
    *ev = nullptr;
    const hipError_t e = stub_call("event_create", nullptr);
    if (e == hipSuccess) { *ev = (hipEvent_t)malloc(1); g_hip.events++; }
    return e;
}
hipError_t hipEventDestroy(hipEvent_t ev) { g_hip.log.push_back(stub_name("event_destroy", (const void *)ev)); free((void *)ev); g_hip.events--; return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t ev, hipStream_t) { return stub_call("record", (const void *)ev); }
hipError_t hipEventSynchronize(hipEvent_t ev) { return stub_call("wait", (const void *)ev, true); }
hipError_t hipStreamWaitEvent(hipStream_t, hipEvent_t ev, unsigned) { return stub_call("stream_wait", (const void *)ev); }
hipError_t hipGetLastError(void) { g_hip.log.push_back("getlasterror"); const hipError_t e = g_hip.sticky; g_hip.sticky = hipSuccess; return e; }
const char *hipGetErrorString(hipError_t e) { return e == hipErrorOutOfMemory ? "out of memory" : e == hipErrorUnknown ? "unknown error" : "error"; }
}
