// arena_walk.h -- one description of a record's device arrays, walked twice: to count the bytes and to carve the pointers.
// Plain host C++ (no HIP include): the library and the sanitizer-built host check (tools/arena_layout_host_check.cpp) compile the same lines.
//
// A layout function X_layout(ArenaWalk &, XDev *, shape...) is the one place that knows which arrays a record has, in which order and how
// large.  X_bytes runs it over a counting walk (base == nullptr, limit == SIZE_MAX: every take yields nullptr, nothing is dereferenced) and
// returns `off`; X_carve runs it over a walk of the context's arena (ctx_arena_walk) and commits `off` back (ctx_arena_commit) when `ok`.
#pragma once
#include <stddef.h>
#include <stdint.h>

struct ArenaWalk {
    char *base = nullptr;
    size_t off = 0, limit = SIZE_MAX;
    bool ok = true;                   // latches the first request that does not fit: every later take yields nullptr and leaves `off` alone

    // `count` elements of T at the next multiple of `align` (a power of two); count == 0 takes one element, so that no two arrays share an address
    template <class T> T *take(size_t count, size_t align = 256)
    {
        if (!ok) return nullptr;
        if (count == 0) count = 1;
        const size_t at = (off + align - 1) & ~(align - 1);
        if (at < off || at > limit || count > (limit - at) / sizeof(T)) { ok = false; return nullptr; }      // no product that could wrap
        off = at + count * sizeof(T);
        return base ? (T *)(base + at) : nullptr;
    }
    // round `off` up, for a record that is one of an array of records `off` bytes apart
    void pad(size_t align = 256)
    {
        const size_t at = (off + align - 1) & ~(align - 1);
        if (!ok || at < off || at > limit) ok = false;
        else off = at;
    }
};
