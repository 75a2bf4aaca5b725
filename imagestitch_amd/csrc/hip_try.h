// hip_try.h -- error plumbing of the libvfsms translation units: the thread's error string and the two early-return macros.
#pragma once
#include <hip/hip_runtime_api.h>
#include "../../include/vfsms.h"

void vfsms_set_error(const char *fmt, ...);
#define HIP_TRY(expr)                                                                         \
    do {                                                                                      \
        hipError_t _e = (expr);                                                               \
        if (_e != hipSuccess) {                                                               \
            vfsms_set_error("%s:%d %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(_e)); \
            return VFSMS_ERR_HIP;                                                             \
        }                                                                                     \
    } while (0)
#define TRY(expr)                  \
    do {                           \
        int _r = (expr);           \
        if (_r != VFSMS_OK) return _r; \
    } while (0)
