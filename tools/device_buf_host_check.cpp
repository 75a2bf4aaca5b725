// device_buf_host_check.cpp -- csrc/device_buf.h (and the records of csrc/common.h that own memory through it) as the plain host C++ it is,
// for a sanitizer build that links neither the HIP runtime nor libvfsms: the runtime calls are tools/hip_host_stubs.h's, over malloc / free.
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan -D__HIP_PLATFORM_AMD__ \
//       -I/opt/rocm/include -I imagestitch_amd/csrc tools/device_buf_host_check.cpp -o /tmp/dbhc && /tmp/dbhc
// (the sanitizer runtimes are linked into the program, so it runs as it is, with nothing preloaded; tests/test_device_buf_host.py does this)
// Checked: the grow-only rule call by call (what is synchronised, freed and allocated, in which order), a failed allocation, moves, and
// that a CanvasRec frees each of its buffers once wherever it ends.  At exit nothing is live; LeakSanitizer agrees or fails the run.
#include "hip_host_stubs.h"
#include "device_buf.h"
#include "common.h"
#include <stdarg.h>
#include <string.h>
#include <algorithm>
#include <unordered_map>

static char g_err[512] = "";
void vfsms_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); for (auto &l : g_hip.log) fprintf(stderr, "  log: %s\n", l.c_str()); return 1; } } while (0)
static int g_checks = 0;
static std::string mal(size_t n) { char b[64]; snprintf(b, sizeof(b), "malloc(%zu)", n); return b; }
static bool log_is(std::initializer_list<std::string> want)
{
    g_checks++;
    const bool ok = g_hip.log == std::vector<std::string>(want);
    if (ok) g_hip.log.clear();
    return ok;
}
static long count(const char *prefix) { long n = 0; for (auto &l : g_hip.log) n += l.compare(0, strlen(prefix), prefix) == 0; return n; }

template <bool Pinned>
static int check_buf()
{
    const hipStream_t st = (hipStream_t)0x1000, other = (hipStream_t)0x2000;
    {
        Buf<Pinned> b;
        CHECK(!b && b.bytes() == 0 && b.template as<char>() == nullptr);
        CHECK(b.release(st) == VFSMS_OK && log_is({}));                        // nothing to let go: no call at all
        CHECK(b.reserve(0, st) == VFSMS_OK && !b && log_is({}));                // capacity 0 covers 0 bytes
        CHECK(b.reserve(100, st, 25) == VFSMS_OK && log_is({mal(125)}));        // growth from empty: the allocation alone
        CHECK(b && b.bytes() == 125);
        char *p0 = b.template as<char>();
        memset(p0, 7, 125);                                                    // (ASan: all of need + headroom is there)
        CHECK(b.reserve(125, other) == VFSMS_OK && b.reserve(1, other, 1000) == VFSMS_OK && log_is({}) && b.template as<char>() == p0 && b.bytes() == 125);
        CHECK(b.reserve(126, other, 4) == VFSMS_OK);                            // growth: the stream GIVEN is synchronised before the old bytes go
        CHECK(log_is({stub_name("sync", other), stub_name("free", p0), mal(130)}) && b.bytes() == 130);
        // a failed allocation: the old bytes went once, the buffer is empty, the error is HIP_TRY's, and the next reserve works
        char *p1 = b.template as<char>();
        g_hip.fail_at = 1;
        CHECK(b.reserve(500, st) == VFSMS_ERR_HIP && !b && b.bytes() == 0 && b.template as<char>() == nullptr);
        CHECK(strstr(g_err, "device_buf.h") && strstr(g_err, Pinned ? "hipHostMalloc" : "hipMalloc") && strstr(g_err, "-> out of memory"));
        CHECK(log_is({stub_name("sync", st), stub_name("free", p1), mal(500)}));
        CHECK(b.reserve(500, st) == VFSMS_OK && b && b.bytes() == 500 && log_is({mal(500)}));
        // moves empty their source; move assignment frees what the target held, once, without a synchronisation (as the destructor does)
        char *p2 = b.template as<char>();
        Buf<Pinned> c(std::move(b));
        CHECK(!b && b.bytes() == 0 && c.template as<char>() == p2 && c.bytes() == 500 && log_is({}));
        Buf<Pinned> d;
        CHECK(d.reserve(8, st) == VFSMS_OK && log_is({mal(8)}));
        char *p3 = d.template as<char>();
        d = std::move(c);
        CHECK(!c && c.bytes() == 0 && d.template as<char>() == p2 && d.bytes() == 500 && log_is({stub_name("free", p3)}));
        CHECK(d.release(st) == VFSMS_OK && !d && d.bytes() == 0 && log_is({stub_name("sync", st), stub_name("free", p2)}));
        CHECK(d.reserve(16, st) == VFSMS_OK && log_is({mal(16)}));
        p0 = d.template as<char>();
        b = std::move(d);                                                      // into an empty target: nothing freed
        CHECK(log_is({}) && b.template as<char>() == p0);
    }
    CHECK(g_hip.log.size() == 1 && count("free(") == 1 && g_hip.live == 0);     // the destructor: one free, no synchronisation
    g_hip.log.clear();
    return 0;
}

static int fill(CanvasRec &cv, int rows, int cols, int ch, hipStream_t st)     // the allocations of vfsms_canvas_create, in its order
{
    cv.rows = rows; cv.cols = cols; cv.ch = ch;
    TRY(cv.pix.reserve((size_t)rows * cols * ch, st));
    TRY(cv.mask.reserve((size_t)rows * cols, st));
    TRY(cv.d_err.reserve(sizeof(int), st));
    TRY(cv.scratch.reserve(4096, st));
    return VFSMS_OK;
}
static int check_canvas()
{
    const hipStream_t st = (hipStream_t)0x1000;
    {
        CanvasRec cv;
        g_hip.fail_at = 3;
        CHECK(fill(cv, 5, 7, 3, st) == VFSMS_ERR_HIP && cv.pix && cv.mask && !cv.d_err && !cv.scratch);
        CHECK(log_is({mal(105), mal(35), mal(4)}) && g_hip.live == 2);
    }
    CHECK(g_hip.log.size() == 2 && count("free(") == 2 && g_hip.live == 0);     // a half-built canvas: what it got, once each
    g_hip.log.clear();
    {
        std::unordered_map<int64_t, CanvasRec> canvases;
        CanvasRec cv;
        CHECK(fill(cv, 5, 7, 3, st) == VFSMS_OK && cv.pyr.reserve(64, st) == VFSMS_OK);
        for (DevBuf *b : {&cv.jpeg.coef, &cv.jpeg.sizes, &cv.jpeg.out, &cv.jpeg.img}) CHECK(b->reserve(32, st) == VFSMS_OK);
        CHECK(g_hip.live == 9);
        g_hip.log.clear();
        uint8_t *pix = cv.pix.as<uint8_t>();
        canvases.emplace(1, std::move(cv));
        CHECK(log_is({}) && !cv.pix && !cv.mask && !cv.d_err && !cv.scratch && !cv.pyr && !cv.jpeg.coef && !cv.jpeg.img);
        CHECK(canvases.at(1).pix.as<uint8_t>() == pix && canvases.at(1).rows == 5);
        CanvasRec spare = std::move(canvases.at(1));                              // vfsms_canvas_free: into the spare slot, then out of the map
        canvases.erase(1);
        CHECK(log_is({}) && g_hip.live == 9 && spare.pix.as<uint8_t>() == pix);
        canvases.emplace(2, std::move(spare));
        canvases.erase(2);
        std::vector<std::string> frees = g_hip.log;
        std::sort(frees.begin(), frees.end());
        CHECK(frees.size() == 9 && count("free(") == 9 && std::adjacent_find(frees.begin(), frees.end()) == frees.end() && g_hip.live == 0);
        g_hip.log.clear();
    }
    CHECK(log_is({}) && g_hip.live == 0);                                      // the emptied records had nothing left to free
    return 0;
}

int main()
{
    if (check_buf<false>() || check_buf<true>() || check_canvas()) return 1;
    if (g_hip.live != 0) { fprintf(stderr, "%ld allocations still live\n", g_hip.live); return 1; }
    printf("device_buf_host_check: %d log checks ok\n", g_checks);
    return 0;
}
