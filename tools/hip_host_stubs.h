// hip_host_stubs.h -- the HIP runtime calls behind csrc/device_buf.h, defined over malloc / free for the sanitizer-built host checks
// (device_buf_host_check.cpp, arena_layout_host_check.cpp): no GPU, no HIP runtime at work, and ASan / LeakSanitizer see every "device"
// allocation.  Include it in exactly one translation unit of a program.  Every call is logged (`sync(stream)`, `free(ptr)`, `malloc(n)`),
// live allocations are counted, and fail_at = N makes the N-th allocation from now fail (it is logged all the same).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdio.h>
#include <stdlib.h>
#include <string>
#include <vector>

struct HipStubs { std::vector<std::string> log; long live = 0; long fail_at = 0; };
static HipStubs g_hip;

static std::string stub_name(const char *what, const void *p) { char line[64]; snprintf(line, sizeof(line), "%s(%p)", what, p); return line; }
static hipError_t stub_alloc(void **p, size_t n)
{
    char line[64];
    snprintf(line, sizeof(line), "malloc(%zu)", n);
    g_hip.log.push_back(line);
    *p = nullptr;
    if (g_hip.fail_at && --g_hip.fail_at == 0) return hipErrorOutOfMemory;
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
hipError_t hipMalloc(void **p, size_t n) { return stub_alloc(p, n); }
hipError_t hipHostMalloc(void **p, size_t n, unsigned int) { return stub_alloc(p, n); }
hipError_t hipFree(void *p) { return stub_free(p); }
hipError_t hipHostFree(void *p) { return stub_free(p); }
hipError_t hipStreamSynchronize(hipStream_t s) { g_hip.log.push_back(stub_name("sync", (const void *)s)); return hipSuccess; }
const char *hipGetErrorString(hipError_t e) { return e == hipErrorOutOfMemory ? "out of memory" : "error"; }
}
