// device_buf.h -- the one owner of a long-lived allocation, and the one statement of the grow-only scratch rule.
// Host C++ over the HIP runtime API alone (no common.h): the library and the sanitizer-built host check (tools/device_buf_host_check.cpp,
// which supplies the runtime calls itself) compile the same lines.
//
// Buf<false> = DevBuf owns one hipMalloc allocation, Buf<true> = PinBuf one hipHostMalloc allocation.  Move-only; a moved-from buffer is empty.
// Who may still read the memory decides how it goes: reserve() and release() synchronise the stream given BEFORE they free (enqueued work may
// still read the old bytes); the destructor frees at once -- for buffers without work in flight: behind the context's synchronisation in
// vfsms_ctx_destroy, and on error paths that synchronised first.
#pragma once
#include <stddef.h>
#include "hip_try.h"

template <bool Pinned>
struct Buf {
    Buf() = default;
    Buf(const Buf &) = delete;
    Buf &operator=(const Buf &) = delete;
    Buf(Buf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    Buf &operator=(Buf &&o) noexcept
    {
        if (this != &o) { drop(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
        return *this;
    }
    ~Buf() { drop(); }

    // grow-only: nothing happens while the capacity covers `need` (no HIP call, same pointer); else the old allocation goes as release() lets it go
    // and need + headroom bytes come.  A failed allocation leaves the buffer empty.
    int reserve(size_t need, hipStream_t stream, size_t headroom = 0)
    {
        if (cap >= need) return VFSMS_OK;
        TRY(release(stream));
        void *q = nullptr;
        HIP_TRY(Pinned ? hipHostMalloc(&q, need + headroom, hipHostMallocDefault) : hipMalloc(&q, need + headroom));
        p = q; cap = need + headroom;
        return VFSMS_OK;
    }
    int release(hipStream_t stream)
    {
        if (!p) return VFSMS_OK;
        HIP_TRY(hipStreamSynchronize(stream));
        void *q = p;
        p = nullptr; cap = 0;
        HIP_TRY(Pinned ? hipHostFree(q) : hipFree(q));
        return VFSMS_OK;
    }
    template <class T> T *as() const { return (T *)p; }
    size_t bytes() const { return cap; }
    explicit operator bool() const { return p != nullptr; }

private:
    void drop()
    {
        if (p) (void)(Pinned ? hipHostFree(p) : hipFree(p));
        p = nullptr; cap = 0;
    }
    void *p = nullptr;
    size_t cap = 0;
};
using DevBuf = Buf<false>;
using PinBuf = Buf<true>;
