// sift_kernels.hip -- featureMethod "sift": SIFT detect-and-describe for gfx950.
//
// The algorithm is OpenCV 3.3.1's xfeatures2d::SIFT_Impl (float build, firstOctave -1, nfeatures 0); the arithmetic is this project's
// specification, restated in numpy by tests/sift_ref.py with every float expression in the order these kernels evaluate it, so the
// device output equals it bit for bit (-ffp-contract=off).  Where upstream leaves an order open the spec fixes it: blur taps in
// ascending order; exp / powf through det_exp (detmath.h); the 3 x 3 solve by Cramer's rule over the float determinant; histogram bins
// summed in raster sample order; duplicates resolved to the first keypoint in detection order; descriptor norms summed k = 0 .. 127.
//
// Launches of one group of strips (their number follows octaves x levels, not the number of strips):
//   pyramid   upsample rows + columns (exact), then per level a row blur and a column blur that also writes the DoG against the level
//             below; each octave's level 0 is the INTER_NEAREST decimation of the previous octave's level nOctaveLayers
//   extrema   per octave a counting pass (26-neighbour test + adjustLocalExtrema + contrast / edge tests), one scan per strip over its
//             (octave, layer, row) counts, the group's first host sync (the candidate counts size what follows), then the writing pass,
//             which recomputes and places the survivors of a row in column order -> candidates in detection order without atomics
//   orientation  one wave per candidate: the window's (bin, weight * magnitude) samples are staged in LDS 64 at a time and the lane that
//             owns a bin adds its samples in raster order; smoothing, peaks, parabolic interpolation
//   keypoints scan of the per-candidate peak counts, emit, duplicate flags (each keypoint against every earlier one, LDS tiles), scan,
//             compaction with the firstOctave adjustment; the group's second host sync (the keypoint counts size what is kept)
//   descriptor one wave per keypoint: samples staged in LDS; the lane that owns one of the 6 x 6 spatial cells adds the two orientation
//             bins a sample gives that cell, in sample order; wrap, clamp at 0.2 |h|, renormalise to 512, saturate to u8
// Every kernel is batched over the strips of a group (blockIdx.z, or blockIdx.x for the scans): the strips of a group have one shape,
// so one plan serves them all and strip z's planes sit z * zs floats behind strip 0's.  The single-image entry points run the group of
// one.  A group's pyramids live in ctx->sift_scratch, its candidates and keypoints in ctx->sift_kp (both grow to the largest group
// seen); what outlives the group -- keypoint positions, descriptors, their packed int8 form -- is taken from ctx->sift_pool.
#include "common.h"
#include "detmath.h"
#include <math.h>
#include <float.h>
#include <string.h>
#include <algorithm>

#define SIFT_BORDER 5
#define SIFT_MAX_STEPS 5
#define SIFT_ORI_BINS 36
#define SIFT_MAX_PEAKS 18                  // a peak is above both neighbours: at most every other bin of 36
#define SIFT_MAX_TAPS 127

struct SiftTaps { float t[SIFT_MAX_TAPS + 1]; int n; };
struct SiftOct {                            // one octave's levels
    const float *g[VFSMS_SIFT_MAX_LAYERS + 3];
    const float *d[VFSMS_SIFT_MAX_LAYERS + 2];
    int R, C;
};
struct SiftCand { float x, y, size, response; int octave, o, layer, r, c; };
struct SiftCfg { int L; float thr, contrast, edge, sigma; };
struct SiftSrc { const uint8_t *p; int stride; };                       // one strip's pixels, read in place
// one strip's share of a group's candidate / keypoint arrays (SIFT_MAX_PEAKS keypoint slots per candidate) and where its results go
struct SiftSeg { int cand0, ncand; float *desc; float *xy; };

__device__ __forceinline__ int sift_reflect101(int i, int n)
{
    if (n == 1) return 0;
    while (i < 0 || i >= n) i = i < 0 ? -i : 2 * n - 2 - i;
    return i;
}

__device__ __forceinline__ float sift_expf(float x) { return (float)det_exp((double)x); }

__device__ __forceinline__ float sift_atan2_deg(float y, float x)   // cv::fastAtan2, as fast_atan2_deg of surf_kernels.hip
{
    const float s = (float)(180 / 3.1415926535897932384626433832795);
    const float p1 = 0.9997878412794807f * s, p3 = -0.3258083974640975f * s;
    const float p5 = 0.1555786518463281f * s, p7 = -0.04432655554792128f * s;
    float ax = fabsf(x), ay = fabsf(y);
    float a, c, c2;
    if (ax >= ay) {
        c = ay / (ax + (float)DBL_EPSILON);
        c2 = c * c;
        a = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
    } else {
        c = ax / (ay + (float)DBL_EPSILON);
        c2 = c * c;
        a = 90.f - (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
    }
    if (x < 0) a = 180.f - a;
    if (y < 0) a = 360.f - a;
    return a;
}

// ---- pyramid ---------------------------------------------------------------------------------------------------------------------
// INTER_LINEAR 2x along rows: out[y][d] = a * w0 + b * w1 with a = src[x0], b = src[x0 + 1] clamped, (w0, w1) = (0.25, 0.75) for even d
__global__ void k_sift_up_rows(const SiftSrc *srcs, int h, int w, float *dst, size_t zs)
{
    const int d = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (d >= 2 * w) return;
    const uint8_t *src = srcs[blockIdx.z].p; const size_t ss = (size_t)srcs[blockIdx.z].stride;
    dst += blockIdx.z * zs;
    const int x0 = (d & 1) ? d >> 1 : (d >> 1) - 1;
    const float w0 = (d & 1) ? 0.75f : 0.25f, w1 = (d & 1) ? 0.25f : 0.75f;
    const float a = (float)src[(size_t)y * ss + min(max(x0, 0), w - 1)], b = (float)src[(size_t)y * ss + min(max(x0 + 1, 0), w - 1)];
    dst[(size_t)y * 2 * w + d] = a * w0 + b * w1;
}
__global__ void k_sift_up_cols(const float *src, int h, int W, float *dst, size_t zs)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x, d = blockIdx.y;
    if (x >= W) return;
    src += blockIdx.z * zs; dst += blockIdx.z * zs;
    const int y0 = (d & 1) ? d >> 1 : (d >> 1) - 1;
    const float w0 = (d & 1) ? 0.75f : 0.25f, w1 = (d & 1) ? 0.25f : 0.75f;
    const float a = src[(size_t)min(max(y0, 0), h - 1) * W + x], b = src[(size_t)min(max(y0 + 1, 0), h - 1) * W + x];
    dst[(size_t)d * W + x] = a * w0 + b * w1;
}

// row pass of the separable Gaussian: acc = t[0] * s[x - r], then acc + t[k] * s[x - r + k], REFLECT_101
#define SIFT_ROW_TILE 256
__global__ __launch_bounds__(256) void k_sift_blur_rows(const float *src, float *dst, int R, int C, SiftTaps T, size_t zs)
{
    __shared__ float s[SIFT_ROW_TILE + 2 * SIFT_MAX_TAPS];
    src += blockIdx.z * zs; dst += blockIdx.z * zs;
    const int y = blockIdx.y, x0 = blockIdx.x * SIFT_ROW_TILE, r = T.n >> 1;
    const float *row = src + (size_t)y * C;
    for (int q = threadIdx.x; q < SIFT_ROW_TILE + 2 * r; q += blockDim.x) {
        const int x = x0 - r + q;
        if (x0 - r + q < C + r) s[q] = row[sift_reflect101(x, C)];
    }
    __syncthreads();
    const int x = x0 + threadIdx.x;
    if (x >= C) return;
    float acc = T.t[0] * s[threadIdx.x];
    for (int k = 1; k < T.n; k++) acc = acc + T.t[k] * s[threadIdx.x + k];
    dst[(size_t)y * C + x] = acc;
}
// column pass; with prev != null also dog = out - prev (the DoG of the level below)
__global__ __launch_bounds__(256) void k_sift_blur_cols(const float *src, float *dst, const float *prev, float *dog, int R, int C, SiftTaps T, size_t zs)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y, r = T.n >> 1;
    if (x >= C) return;
    src += blockIdx.z * zs; dst += blockIdx.z * zs;
    if (prev) { prev += blockIdx.z * zs; dog += blockIdx.z * zs; }
    float acc = T.t[0] * src[(size_t)sift_reflect101(y - r, R) * C + x];
    for (int k = 1; k < T.n; k++) acc = acc + T.t[k] * src[(size_t)sift_reflect101(y - r + k, R) * C + x];
    const size_t o = (size_t)y * C + x;
    dst[o] = acc;
    if (prev) dog[o] = acc - prev[o];
}
// INTER_NEAREST to (R / 2, C / 2): source floor(d * if) in double, clamped
__global__ void k_sift_decimate(const float *src, int R, int C, float *dst, int dR, int dC, double ify, double ifx, size_t zs)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= dC) return;
    src += blockIdx.z * zs; dst += blockIdx.z * zs;
    const int sy = min((int)floor((double)y * ify), R - 1), sx = min((int)floor((double)x * ifx), C - 1);
    dst[(size_t)y * dC + x] = src[(size_t)sy * C + sx];
}

// ---- extrema ---------------------------------------------------------------------------------------------------------------------
// O names strip 0's planes; Z is the float offset of the strip at hand
__device__ __forceinline__ float sift_at(const SiftOct &O, size_t Z, int l, int r, int c) { return O.d[l][Z + (size_t)r * O.C + c]; }

// the 26-neighbour test, then adjustLocalExtrema and the contrast / edge tests; true -> *out filled
__device__ bool sift_candidate(const SiftOct &O, size_t Z, const SiftCfg &P, int o, int l, int r, int c, SiftCand *out)
{
    const float val = sift_at(O, Z, l, r, c);
    if (!(fabsf(val) > P.thr)) return false;
    bool ge = true, le = true;
    for (int dl = -1; dl <= 1; dl++)
        for (int dr = -1; dr <= 1; dr++)
            for (int dc = -1; dc <= 1; dc++) {
                if (dl == 0 && dr == 0 && dc == 0) continue;
                const float nb = sift_at(O, Z, l + dl, r + dr, c + dc);
                ge = ge && val >= nb; le = le && val <= nb;
            }
    if (!((val > 0 && ge) || (val < 0 && le))) return false;
    const float img_scale = 1.f / 255.f, deriv_scale = img_scale * 0.5f, second_scale = img_scale, cross_scale = img_scale * 0.25f;
    const int L = P.L, R = O.R, C = O.C;
    float xi = 0, xr = 0, xc = 0;
    int step = 0;
    for (; step < SIFT_MAX_STEPS; step++) {
        const float v = sift_at(O, Z, l, r, c);
        const float xp = sift_at(O, Z, l, r, c + 1), xm = sift_at(O, Z, l, r, c - 1), yp = sift_at(O, Z, l, r + 1, c), ym = sift_at(O, Z, l, r - 1, c);
        const float sp = sift_at(O, Z, l + 1, r, c), sm = sift_at(O, Z, l - 1, r, c);
        const float b0 = (xp - xm) * deriv_scale, b1 = (yp - ym) * deriv_scale, b2 = (sp - sm) * deriv_scale;
        const float v2 = v * 2.f;
        const float dxx = ((xp + xm) - v2) * second_scale, dyy = ((yp + ym) - v2) * second_scale, dss = ((sp + sm) - v2) * second_scale;
        const float dxy = (((sift_at(O, Z, l, r + 1, c + 1) - sift_at(O, Z, l, r + 1, c - 1)) - sift_at(O, Z, l, r - 1, c + 1)) + sift_at(O, Z, l, r - 1, c - 1)) * cross_scale;
        const float dxs = (((sift_at(O, Z, l + 1, r, c + 1) - sift_at(O, Z, l + 1, r, c - 1)) - sift_at(O, Z, l - 1, r, c + 1)) + sift_at(O, Z, l - 1, r, c - 1)) * cross_scale;
        const float dys = (((sift_at(O, Z, l + 1, r + 1, c) - sift_at(O, Z, l + 1, r - 1, c)) - sift_at(O, Z, l - 1, r + 1, c)) + sift_at(O, Z, l - 1, r - 1, c)) * cross_scale;
        // Matx33f H(dxx, dxy, dxs, dxy, dyy, dys, dxs, dys, dss).solve(dD, DECOMP_LU): Cramer's rule over the float determinant
        const float a00 = dxx, a01 = dxy, a02 = dxs, a10 = dxy, a11 = dyy, a12 = dys, a20 = dxs, a21 = dys, a22 = dss;
        const float det = (a00 * (a11 * a22 - a21 * a12) - a01 * (a10 * a22 - a20 * a12)) + a02 * (a10 * a21 - a20 * a11);
        float X0 = 0.f, X1 = 0.f, X2 = 0.f;
        if (det != 0) {
            const float d = 1.f / det;
            X0 = d * ((b0 * (a11 * a22 - a12 * a21) - a01 * (b1 * a22 - a12 * b2)) + a02 * (b1 * a21 - a11 * b2));
            X1 = d * ((a00 * (b1 * a22 - a12 * b2) - b0 * (a10 * a22 - a12 * a20)) + a02 * (a10 * b2 - b1 * a20));
            X2 = d * ((a00 * (a11 * b2 - b1 * a21) - a01 * (a10 * b2 - b1 * a20)) + b0 * (a10 * a21 - a11 * a20));
        }
        xi = -X2; xr = -X1; xc = -X0;
        if (fabsf(xi) < 0.5f && fabsf(xr) < 0.5f && fabsf(xc) < 0.5f) break;
        const float big = (float)(2147483647 / 3);
        if (fabsf(xi) > big || fabsf(xr) > big || fabsf(xc) > big) return false;
        c += (int)rintf(xc); r += (int)rintf(xr); l += (int)rintf(xi);
        if (l < 1 || l > L || c < SIFT_BORDER || c >= C - SIFT_BORDER || r < SIFT_BORDER || r >= R - SIFT_BORDER) return false;
    }
    if (step >= SIFT_MAX_STEPS) return false;
    const float v = sift_at(O, Z, l, r, c);
    const float xp = sift_at(O, Z, l, r, c + 1), xm = sift_at(O, Z, l, r, c - 1), yp = sift_at(O, Z, l, r + 1, c), ym = sift_at(O, Z, l, r - 1, c);
    const float sp = sift_at(O, Z, l + 1, r, c), sm = sift_at(O, Z, l - 1, r, c);
    const float b0 = (xp - xm) * deriv_scale, b1 = (yp - ym) * deriv_scale, b2 = (sp - sm) * deriv_scale;
    const float t = ((0.f + b0 * xc) + b1 * xr) + b2 * xi;
    const float contr = v * img_scale + t * 0.5f;
    if (fabsf(contr) * (float)L < P.contrast) return false;
    const float v2 = v * 2.f;
    const float dxx = ((xp + xm) - v2) * second_scale, dyy = ((yp + ym) - v2) * second_scale;
    const float dxy = (((sift_at(O, Z, l, r + 1, c + 1) - sift_at(O, Z, l, r + 1, c - 1)) - sift_at(O, Z, l, r - 1, c + 1)) + sift_at(O, Z, l, r - 1, c - 1)) * cross_scale;
    const float tr = dxx + dyy, dt = dxx * dyy - dxy * dxy, e = P.edge;
    if (dt <= 0 || tr * tr * e >= (e + 1.f) * (e + 1.f) * dt) return false;
    const float s = (float)(1 << o);
    const float y = (((float)l + xi) / (float)L) * 0.6931471805599453f;
    out->x = ((float)c + xc) * s;
    out->y = ((float)r + xr) * s;
    out->size = ((P.sigma * sift_expf(y)) * s) * 2.f;
    out->response = fabsf(contr);
    out->octave = o + (l << 8) + ((int)rint(((double)xi + 0.5) * 255) << 16);
    out->o = o; out->layer = l; out->r = r; out->c = c;
    return true;
}

// one workgroup per (row, layer) of an octave: how many candidates the row gives (pass 0), or the candidates themselves in column order
// at cand + base[row slot] (pass 1)
// strip blockIdx.z: its counts / bases zs ints behind strip 0's, its candidates at cand + segs[z].cand0
__global__ __launch_bounds__(256) void k_sift_extrema(SiftOct O, SiftCfg P, int o, int *counts, const int *base, SiftCand *cand, size_t zs,
                                                      const SiftSeg *segs)
{
    __shared__ int wsum[4];
    const size_t Z = blockIdx.z * zs;
    if (counts) counts += Z;
    if (base) base += Z;
    if (cand) cand += segs[blockIdx.z].cand0;
    const int r = blockIdx.x, l = blockIdx.y + 1, slot = (l - 1) * O.R + r;
    const bool row_ok = r >= SIFT_BORDER && r < O.R - SIFT_BORDER;
    int running = base ? base[slot] : 0, total = 0;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int c0 = SIFT_BORDER; row_ok && c0 < O.C - SIFT_BORDER; c0 += 256) {
        const int c = c0 + threadIdx.x;
        SiftCand k;
        const bool hit = c < O.C - SIFT_BORDER && sift_candidate(O, Z, P, o, l, r, c, &k);
        const unsigned long long m = __ballot(hit);
        if (lane == 0) wsum[wv] = __popcll(m);
        __syncthreads();
        int before = 0, all = 0;
        for (int q = 0; q < 4; q++) { before += q < wv ? wsum[q] : 0; all += wsum[q]; }
        if (hit && cand) cand[running + before + __popcll(m & ((1ull << lane) - 1))] = k;
        running += all; total += all;
        __syncthreads();
    }
    if (!base && threadIdx.x == 0) counts[slot] = total;
}

// exclusive scan of n ints (n_dev overrides n) by one workgroup of 1024; out[n] = total, *total_out too
// strip blockIdx.x: arrays zs ints behind strip 0's (segs == null), or at its segment (per_cand slots per candidate, + 1 per strip for
// the total); its counters are the 4 ints at tot + 4 z: n is read from tot[n_at] when n_at >= 0, the total goes to tot[tot_at]
__global__ __launch_bounds__(1024) void k_sift_scan(const int *in, int *out, int n, size_t zs, const SiftSeg *segs, int per_cand,
                                                    int *tot, int n_at, int tot_at)
{
    __shared__ int s[1024];
    const int z = blockIdx.x;
    tot += 4 * z;
    if (segs) {
        const size_t o = (size_t)segs[z].cand0 * per_cand + z;
        in += o; out += o;
        n = segs[z].ncand;
    } else { in += z * zs; out += z * zs; }
    if (n_at >= 0) n = tot[n_at];
    const int t = threadIdx.x, per = (n + 1023) / 1024, a = min(t * per, n), b = min(a + per, n);
    int sum = 0;
    for (int i = a; i < b; i++) sum += in[i];
    s[t] = sum;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const int v = t >= off ? s[t - off] : 0;
        __syncthreads();
        s[t] += v;
        __syncthreads();
    }
    int run = s[t] - sum;
    for (int i = a; i < b; i++) { const int v = in[i]; out[i] = run; run += v; }
    if (t == 1023) { out[n] = s[1023]; tot[tot_at] = s[1023]; }
}

// ---- orientation: one wave per candidate -----------------------------------------------------------------------------------------
struct SiftOcts { SiftOct o[VFSMS_SIFT_MAX_OCT]; };

__global__ __launch_bounds__(64) void k_sift_orient(const SiftOcts *Os, size_t zs, const SiftSeg *segs, const SiftCand *cand, float *angles, int *npk)
{
    __shared__ int sbin[64];
    __shared__ float sval[64];
    __shared__ float th[SIFT_ORI_BINS], hs[SIFT_ORI_BINS];
    const int k = blockIdx.x, lane = threadIdx.x, z = blockIdx.z;
    const SiftSeg S = segs[z];
    if (k >= S.ncand) return;
    cand += S.cand0; angles += (size_t)S.cand0 * SIFT_MAX_PEAKS; npk += S.cand0 + z;
    const SiftCand K = cand[k];
    const SiftOct &O = Os->o[K.o];
    const float *img = O.g[K.layer] + z * zs;
    const int R = O.R, C = O.C, px = K.c, py = K.r;
    const float scl = (K.size * 0.5f) / (float)(1 << K.o);
    const int radius = (int)rintf(4.5f * scl);
    const float sigma = 1.5f * scl;
    const float expf_scale = -1.f / ((2.f * sigma) * sigma);
    const int side = 2 * radius + 1, total = side * side;
    float acc = 0.f;
    for (int b0 = 0; b0 < total; b0 += 64) {
        const int p = b0 + lane, i = p / side - radius, j = p % side - radius, y = py + i, x = px + j;
        int bin = -1; float val = 0.f;
        if (p < total && y > 0 && y < R - 1 && x > 0 && x < C - 1) {
            const float dx = img[(size_t)y * C + x + 1] - img[(size_t)y * C + x - 1];
            const float dy = img[(size_t)(y - 1) * C + x] - img[(size_t)(y + 1) * C + x];
            const float W = sift_expf((float)(i * i + j * j) * expf_scale);
            const float ori = sift_atan2_deg(dy, dx);
            const float mag = sqrtf(dx * dx + dy * dy);
            bin = (int)rintf((36.f / 360.f) * ori);
            if (bin >= SIFT_ORI_BINS) bin -= SIFT_ORI_BINS;
            if (bin < 0) bin += SIFT_ORI_BINS;
            val = W * mag;
        }
        sbin[lane] = bin; sval[lane] = val;
        __syncthreads();
        if (lane < SIFT_ORI_BINS)
            for (int e = 0; e < 64; e++)
                if (sbin[e] == lane) acc += sval[e];
        __syncthreads();
    }
    const int n = SIFT_ORI_BINS;
    if (lane < n) th[lane] = acc;
    __syncthreads();
    if (lane < n) {
        const int i = lane;
        hs[i] = ((th[(i + n - 2) % n] + th[(i + 2) % n]) * (1.f / 16.f) + (th[(i + n - 1) % n] + th[(i + 1) % n]) * (4.f / 16.f)) + th[i] * (6.f / 16.f);
    }
    __syncthreads();
    float omax = hs[0];
    for (int i = 1; i < n; i++) omax = omax < hs[i] ? hs[i] : omax;
    const float mag_thr = omax * 0.8f;
    bool pk = false; float angle = 0.f;
    if (lane < n) {
        const int j = lane, l = j > 0 ? j - 1 : n - 1, r2 = j < n - 1 ? j + 1 : 0;
        const float hj = hs[j], hl = hs[l], hr = hs[r2];
        if (hj > hl && hj > hr && hj >= mag_thr) {
            float bin = (float)j + (0.5f * (hl - hr)) / ((hl - 2.f * hj) + hr);
            bin = bin < 0 ? (float)n + bin : bin >= (float)n ? bin - (float)n : bin;
            angle = 360.f - 10.f * bin;
            if (fabsf(angle - 360.f) < FLT_EPSILON) angle = 0.f;
            pk = true;
        }
    }
    const unsigned long long m = __ballot(pk);
    if (pk) angles[(size_t)k * SIFT_MAX_PEAKS + __popcll(m & ((1ull << lane) - 1))] = angle;
    if (lane == 0) npk[k] = __popcll(m);
}

// keypoints in detection order (before removeDuplicated and the firstOctave adjustment)
__global__ void k_sift_emit(const SiftSeg *segs, const SiftCand *cand, const float *angles, const int *npk, const int *pos, vfsms_keypoint *kp)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x, z = blockIdx.z;
    const SiftSeg S = segs[z];
    if (k >= S.ncand) return;
    cand += S.cand0; angles += (size_t)S.cand0 * SIFT_MAX_PEAKS; npk += S.cand0 + z; pos += S.cand0 + z;
    kp += (size_t)S.cand0 * SIFT_MAX_PEAKS;
    const SiftCand K = cand[k];
    for (int q = 0; q < npk[k]; q++) {
        vfsms_keypoint o;
        o.x = K.x; o.y = K.y; o.size = K.size; o.angle = angles[(size_t)k * SIFT_MAX_PEAKS + q]; o.response = K.response;
        o.octave = K.octave; o.class_id = -1;
        kp[pos[k] + q] = o;
    }
}

// keep[k] = no earlier keypoint has the same (x, y, size, angle)
__global__ __launch_bounds__(256) void k_sift_dedup(const SiftSeg *segs, const vfsms_keypoint *kp, const int *tot, int *keep)
{
    __shared__ float4 s[256];
    const int z = blockIdx.z;
    const int n = tot[4 * z + 1], start = blockIdx.x * 256, k = start + threadIdx.x;
    if (start >= n) return;
    kp += (size_t)segs[z].cand0 * SIFT_MAX_PEAKS; keep += (size_t)segs[z].cand0 * SIFT_MAX_PEAKS + z;
    float4 me = make_float4(0.f, 0.f, 0.f, 0.f);
    if (k < n) { const vfsms_keypoint q = kp[k]; me = make_float4(q.x, q.y, q.size, q.angle); }
    bool dup = false;
    const int end = min(n, start + 256);
    for (int t0 = 0; t0 < end; t0 += 256) {
        const int j = t0 + threadIdx.x;
        if (j < n) { const vfsms_keypoint q = kp[j]; s[threadIdx.x] = make_float4(q.x, q.y, q.size, q.angle); }
        __syncthreads();
        const int lim = min(256, k - t0);
        for (int e = 0; e < lim; e++) {
            const float4 v = s[e];
            dup = dup || (v.x == me.x && v.y == me.y && v.z == me.z && v.w == me.w);
        }
        __syncthreads();
    }
    if (k < n) keep[k] = dup ? 0 : 1;
}

// survivors, compacted, with the firstOctave = -1 adjustment (pt and size * 0.5, octave byte - 1)
__global__ void k_sift_compact(const SiftSeg *segs, const vfsms_keypoint *kp, const int *tot, const int *keep, const int *pos, vfsms_keypoint *out)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x, z = blockIdx.z;
    const size_t o = (size_t)segs[z].cand0 * SIFT_MAX_PEAKS;
    kp += o; out += o; keep += o + z; pos += o + z;
    if (k >= tot[4 * z + 1] || !keep[k]) return;
    vfsms_keypoint q = kp[k];
    q.x = q.x * 0.5f; q.y = q.y * 0.5f; q.size = q.size * 0.5f;
    q.octave = (q.octave & ~255) | ((q.octave - 1) & 255);
    out[pos[k]] = q;
}

// ---- descriptor: one wave per keypoint -------------------------------------------------------------------------------------------
// also writes the keypoint's position to the strip's xy array (what the vote reads)
__global__ __launch_bounds__(64) void k_sift_describe(const SiftOcts *Os, size_t zs, const SiftSeg *segs, const vfsms_keypoint *kps, const int *tot)
{
    constexpr int d = 4, n = 8, HN = (d + 2) * (d + 2) * (n + 2);
    __shared__ float hist[HN];
    __shared__ int scell[64], so0[64];
    __shared__ float sv[64][8];
    __shared__ float dst[128];
    __shared__ float s_scale;
    const int k = blockIdx.x, lane = threadIdx.x, z = blockIdx.z;
    if (k >= tot[4 * z + 2]) return;
    const SiftSeg S = segs[z];
    kps += (size_t)S.cand0 * SIFT_MAX_PEAKS;
    float *desc = S.desc;
    const vfsms_keypoint K = kps[k];
    if (lane == 0) { S.xy[2 * k] = K.x; S.xy[2 * k + 1] = K.y; }
    int octv = K.octave & 255;
    const int layer = (K.octave >> 8) & 255;
    octv = octv < 128 ? octv : (-128 | octv);
    const float scale = octv >= 0 ? 1.f / (float)(1 << octv) : (float)(1 << -octv);
    const float size = K.size * scale, ptx = K.x * scale, pty = K.y * scale;
    const SiftOct &O = Os->o[octv + 1];
    const float *img = O.g[layer] + z * zs;
    const int rows = O.R, cols = O.C;
    float ang = 360.f - K.angle;
    if (fabsf(ang - 360.f) < FLT_EPSILON) ang = 0.f;
    const float scl = size * 0.5f;
    const int px = (int)rintf(ptx), py = (int)rintf(pty);
    double sd, cd;
    det_sincos((double)(ang * (float)(3.14159265358979323846 / 180)), &sd, &cd);
    float cos_t = (float)cd, sin_t = (float)sd;
    const float bins_per_rad = (float)n / 360.f;
    const float exp_scale = -1.f / (float)(d * d * 0.5f);
    const float hist_width = 3.f * scl;
    int radius = (int)rintf(((hist_width * 1.4142135623730951f) * (float)(d + 1)) * 0.5f);
    radius = min(radius, (int)sqrt((double)cols * cols + (double)rows * rows));
    cos_t = cos_t / hist_width;
    sin_t = sin_t / hist_width;
    for (int q = lane; q < HN; q += 64) hist[q] = 0.f;
    __syncthreads();
    const int side = 2 * radius + 1, total = side * side;
    const int cr = lane / (d + 2), cc = lane % (d + 2);          // the cell a lane owns (lanes 0 .. 35)
    for (int b0 = 0; b0 < total; b0 += 64) {
        const int p = b0 + lane, i = p / side - radius, j = p % side - radius;
        const float c_rot = (float)j * cos_t - (float)i * sin_t;
        const float r_rot = (float)j * sin_t + (float)i * cos_t;
        float rbin = (r_rot + (float)(d / 2)) - 0.5f;
        float cbin = (c_rot + (float)(d / 2)) - 0.5f;
        const int r = py + i, c = px + j;
        const bool ok = p < total && rbin > -1 && rbin < d && cbin > -1 && cbin < d && r > 0 && r < rows - 1 && c > 0 && c < cols - 1;
        if (ok) {
            const float dx = img[(size_t)r * cols + c + 1] - img[(size_t)r * cols + c - 1];
            const float dy = img[(size_t)(r - 1) * cols + c] - img[(size_t)(r + 1) * cols + c];
            const float W = sift_expf((c_rot * c_rot + r_rot * r_rot) * exp_scale);
            const float ori = sift_atan2_deg(dy, dx);
            const float Mag = sqrtf(dx * dx + dy * dy);
            float obin = (ori - ang) * bins_per_rad;
            const float mag = Mag * W;
            const int r0 = (int)floorf(rbin), c0 = (int)floorf(cbin);
            int o0 = (int)floorf(obin);
            rbin = rbin - (float)r0; cbin = cbin - (float)c0; obin = obin - (float)o0;
            if (o0 < 0) o0 += n;
            if (o0 >= n) o0 -= n;
            const float v_r1 = mag * rbin, v_r0 = mag - v_r1;
            const float v_rc11 = v_r1 * cbin, v_rc10 = v_r1 - v_rc11;
            const float v_rc01 = v_r0 * cbin, v_rc00 = v_r0 - v_rc01;
            const float v111 = v_rc11 * obin, v110 = v_rc11 - v111;
            const float v101 = v_rc10 * obin, v100 = v_rc10 - v101;
            const float v011 = v_rc01 * obin, v010 = v_rc01 - v011;
            const float v001 = v_rc00 * obin, v000 = v_rc00 - v001;
            scell[lane] = (r0 + 1) * 16 + (c0 + 1); so0[lane] = o0;
            sv[lane][0] = v000; sv[lane][1] = v001; sv[lane][2] = v010; sv[lane][3] = v011;
            sv[lane][4] = v100; sv[lane][5] = v101; sv[lane][6] = v110; sv[lane][7] = v111;
        }
        unsigned long long m = __ballot(ok);
        __syncthreads();
        if (lane < (d + 2) * (d + 2)) {
            float *h = hist + lane * (n + 2);
            while (m) {
                const int e = __ffsll((long long)m) - 1;
                m &= m - 1;
                const int er = scell[e] >> 4, ec = scell[e] & 15, dr = cr - er, dc = cc - ec;
                if (dr >= 0 && dr <= 1 && dc >= 0 && dc <= 1) {
                    const int q = 2 * (2 * dr + dc), o0 = so0[e];
                    h[o0] += sv[e][q];
                    h[o0 + 1] += sv[e][q + 1];
                }
            }
        }
        __syncthreads();
    }
    if (lane < d * d) {
        const int i = lane / d, j = lane % d, idx = ((i + 1) * (d + 2) + (j + 1)) * (n + 2);
        hist[idx] += hist[idx + n];
        hist[idx + 1] += hist[idx + n + 1];
        for (int q = 0; q < n; q++) dst[(i * d + j) * n + q] = hist[idx + q];
    }
    __syncthreads();
    if (lane == 0) {
        float nrm2 = 0.f;
        for (int q = 0; q < d * d * n; q++) nrm2 += dst[q] * dst[q];
        const float thr = sqrtf(nrm2) * 0.2f;
        nrm2 = 0.f;
        for (int q = 0; q < d * d * n; q++) {
            const float v = dst[q] < thr ? dst[q] : thr;
            dst[q] = v;
            nrm2 += v * v;
        }
        const float s = sqrtf(nrm2);
        s_scale = 512.f / (s > FLT_EPSILON ? s : FLT_EPSILON);
    }
    __syncthreads();
    for (int q = lane; q < d * d * n; q += 64) {
        const float v = rintf(dst[q] * s_scale);
        desc[(size_t)k * 128 + q] = fminf(fmaxf(v, 0.f), 255.f);
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
static void sift_taps(double sig, SiftTaps *T)
{
    const int n = (int)lrint(sig * 4 * 2 + 1) | 1;
    const double scale2x = -0.5 / (sig * sig);
    double sum = 0;
    T->n = n;
    for (int i = 0; i < n; i++) {
        const double x = i - (n - 1) * 0.5;
        T->t[i] = (float)exp(scale2x * x * x);
        sum += T->t[i];
    }
    sum = 1. / sum;
    for (int i = 0; i < n; i++) T->t[i] = (float)(T->t[i] * sum);
}

struct SiftPlan {
    int L, no;
    int R[VFSMS_SIFT_MAX_OCT], C[VFSMS_SIFT_MAX_OCT];
    double sig[VFSMS_SIFT_MAX_LAYERS + 3];
    double sig0;
    size_t lvl_off[VFSMS_SIFT_MAX_OCT];       // floats before octave o's levels in the pyramid block
    size_t pyr_floats, max_plane;
    int nslots;                               // sum over octaves of L * R
};

int sift_check_params(const vfsms_sift_params *p)
{
    if (!p) { vfsms_set_error("sift: null params"); return VFSMS_ERR_BAD_ARG; }
    if (p->n_features > 0) {
        vfsms_set_error("sift: nfeatures > 0 (retainBest) is not supported; SIFT_create() uses 0");
        return VFSMS_ERR_UNSUPPORTED;
    }
    if (p->n_features < 0 || p->n_octave_layers < 1 || p->n_octave_layers > VFSMS_SIFT_MAX_LAYERS || !(p->sigma > 0) ||
        !(p->contrast_threshold >= 0) || !(p->edge_threshold > 0)) {
        vfsms_set_error("sift: bad parameters (n_octave_layers 1..%d, sigma > 0, contrast >= 0, edge > 0)", VFSMS_SIFT_MAX_LAYERS);
        return VFSMS_ERR_BAD_ARG;
    }
    return VFSMS_OK;
}

static int sift_plan(int h, int w, const vfsms_sift_params *p, SiftPlan *P)
{
    TRY(sift_check_params(p));
    const int L = p->n_octave_layers;
    P->L = L;
    const int m = std::min(2 * h, 2 * w);
    P->no = std::max((int)lrint(log((double)m) / log(2.) - 2) + 1, 0);
    if (P->no > VFSMS_SIFT_MAX_OCT) { vfsms_set_error("sift: image too large (%d octaves)", P->no); return VFSMS_ERR_BAD_ARG; }
    P->sig[0] = p->sigma;
    const double k = pow(2., 1. / L);
    for (int i = 1; i < L + 3; i++) {
        const double sig_prev = pow(k, (double)(i - 1)) * p->sigma, sig_total = sig_prev * k;
        P->sig[i] = sqrt(sig_total * sig_total - sig_prev * sig_prev);
    }
    const float s = (float)p->sigma;
    P->sig0 = (double)sqrtf(std::max(s * s - (0.5f * 0.5f) * 4.f, 0.01f));
    for (int i = 0; i < L + 3; i++)
        if ((int)lrint((i ? P->sig[i] : P->sig0) * 4 * 2 + 1) > SIFT_MAX_TAPS) { vfsms_set_error("sift: sigma too large for the blur"); return VFSMS_ERR_BAD_ARG; }
    size_t off = 0; P->nslots = 0; P->max_plane = (size_t)2 * h * 2 * w;
    int R = 2 * h, C = 2 * w;
    for (int o = 0; o < P->no; o++) {
        if (o) { R /= 2; C /= 2; }
        P->R[o] = R; P->C[o] = C;
        P->lvl_off[o] = off;
        off += (size_t)(2 * L + 5) * R * C;          // L + 3 Gaussian levels, L + 2 DoG levels
        P->nslots += L * R;
    }
    P->pyr_floats = off;
    return VFSMS_OK;
}

static void sift_octs(const SiftPlan &P, float *pyr, SiftOcts *Os)
{
    memset(Os, 0, sizeof(*Os));
    for (int o = 0; o < P.no; o++) {
        float *b = pyr + P.lvl_off[o];
        const size_t pl = (size_t)P.R[o] * P.C[o];
        for (int i = 0; i < P.L + 3; i++) Os->o[o].g[i] = b + i * pl;
        for (int i = 0; i < P.L + 2; i++) Os->o[o].d[i] = b + (P.L + 3 + i) * pl;
        Os->o[o].R = P.R[o]; Os->o[o].C = P.C[o];
    }
}

// ---- memory that outlives a group: chunks kept by the context, handed out by a bump pointer, all free again at the next call ----------
void sift_pool_reset(vfsms_ctx *ctx) { for (auto &c : ctx->sift_pool) c.off = 0; }
void *sift_pool_alloc(vfsms_ctx *ctx, size_t bytes)
{
    bytes = ((bytes ? bytes : 1) + 255) & ~(size_t)255;
    for (auto &c : ctx->sift_pool)
        if (c.off + bytes <= c.mem.bytes()) { void *r = c.mem.as<char>() + c.off; c.off += bytes; return r; }
    SiftChunk c;
    const size_t want = std::max(bytes, (size_t)256 << 20);
    c.off = bytes;
    if (c.mem.reserve(want, ctx->stream) != VFSMS_OK) { vfsms_set_error("sift: out of device memory (%zu bytes)", want); return nullptr; }
    ctx->sift_pool.push_back(std::move(c));
    return ctx->sift_pool.back().mem.as<void>();
}

// The one place that knows one strip's block in ctx->sift_scratch: [pyramid][2 planes of the largest level][row counts + their scan],
// padded to the distance between the blocks of two strips
void sift_strip_layout(ArenaWalk &a, SiftStripDev *d, size_t pyr_floats, size_t max_plane, int nslots)
{
    d->pyr = a.take<float>(pyr_floats);
    d->t0 = a.take<float>(max_plane);
    d->t1 = a.take<float>(max_plane);
    d->counts = a.take<int>(2 * ((size_t)nslots + 1));
    a.pad();
}
static size_t sift_strip_bytes(const SiftPlan &P) { ArenaWalk a; SiftStripDev d; sift_strip_layout(a, &d, P.pyr_floats, P.max_plane, P.nslots); return a.off; }

// the pyramids of g strips of one shape into ctx->sift_scratch; *zs_out: floats (= ints) between the blocks of two strips
static int sift_build_pyramid(vfsms_ctx *ctx, const SiftSrc *d_srcs, int g, int h, int w, const SiftPlan &P, float **pyr_out, int **counts_out,
                              size_t *zs_out)
{
    const size_t sb = sift_strip_bytes(P);
    TRY(ctx->sift_scratch.reserve(sb * g + 4096, ctx->stream, (sb * g + 4096) / 4));
    ArenaWalk a{ctx->sift_scratch.as<char>(), 0, ctx->sift_scratch.bytes()}; SiftStripDev d;
    sift_strip_layout(a, &d, P.pyr_floats, P.max_plane, P.nslots);           // the first strip's; strip k's lies k * sb behind
    if (!a.ok) { vfsms_set_error("sift: pyramid scratch too small"); return VFSMS_ERR_CAPACITY; }
    float *pyr = d.pyr, *t0 = d.t0, *t1 = d.t1;
    *counts_out = d.counts;
    *pyr_out = pyr;
    const size_t zs = sb / 4;
    *zs_out = zs;
    if (P.no == 0) return VFSMS_OK;
    SiftOcts Os;
    sift_octs(P, pyr, &Os);
    hipStream_t st = ctx->stream;
    const int W2 = 2 * w, H2 = 2 * h;
    const unsigned G = (unsigned)g;
    k_sift_up_rows<<<dim3((W2 + 255) / 256, h, G), 256, 0, st>>>(d_srcs, h, w, t1, zs);
    k_sift_up_cols<<<dim3((W2 + 255) / 256, H2, G), 256, 0, st>>>(t1, h, W2, t0, zs);
    SiftTaps T;
    for (int o = 0; o < P.no; o++) {
        const int R = P.R[o], C = P.C[o];
        const dim3 rg((C + SIFT_ROW_TILE - 1) / SIFT_ROW_TILE, R, G), cg((C + 255) / 256, R, G);
        float *g0 = (float *)Os.o[o].g[0];
        if (o == 0) {
            sift_taps(P.sig0, &T);
            k_sift_blur_rows<<<rg, 256, 0, st>>>(t0, t1, R, C, T, zs);
            k_sift_blur_cols<<<cg, 256, 0, st>>>(t1, g0, nullptr, nullptr, R, C, T, zs);
        } else {
            const int pr = P.R[o - 1], pc = P.C[o - 1];
            k_sift_decimate<<<cg, 256, 0, st>>>(Os.o[o - 1].g[P.L], pr, pc, g0, R, C, 1.0 / ((double)R / pr), 1.0 / ((double)C / pc), zs);
        }
        for (int i = 1; i < P.L + 3; i++) {
            sift_taps(P.sig[i], &T);
            k_sift_blur_rows<<<rg, 256, 0, st>>>(Os.o[o].g[i - 1], t1, R, C, T, zs);
            k_sift_blur_cols<<<cg, 256, 0, st>>>(t1, (float *)Os.o[o].g[i], Os.o[o].g[i - 1], (float *)Os.o[o].d[i - 1], R, C, T, zs);
        }
    }
    HIP_TRY(hipGetLastError());
    return VFSMS_OK;
}

int sift_pyramid_device(vfsms_ctx *ctx, const uint8_t *d_img, int h, int w, const vfsms_sift_params *p,
                        float *gauss, float *dog, size_t cap_floats, int32_t *shapes, int shapes_cap, int *n_oct)
{
    SiftPlan P;
    TRY(sift_plan(h, w, p, &P));
    *n_oct = P.no;
    if (shapes_cap < P.no) { vfsms_set_error("sift_pyramid: %d octaves exceed the shape capacity %d", P.no, shapes_cap); return VFSMS_ERR_CAPACITY; }
    size_t gf = 0;
    for (int o = 0; o < P.no; o++) {
        shapes[2 * o] = P.R[o]; shapes[2 * o + 1] = P.C[o];
        gf += (size_t)(P.L + 3) * P.R[o] * P.C[o];
    }
    if (!gauss && !dog) return VFSMS_OK;
    if (gf > cap_floats) { vfsms_set_error("sift_pyramid: %zu floats exceed the capacity %zu", gf, cap_floats); return VFSMS_ERR_CAPACITY; }
    float *pyr; int *counts; size_t zs;
    SiftSrc src = {d_img, w}, *d_src;
    TRY(ctx_upload_small(ctx, &src, sizeof(src), (void **)&d_src));
    TRY(sift_build_pyramid(ctx, d_src, 1, h, w, P, &pyr, &counts, &zs));
    size_t go = 0, dgo = 0;
    for (int o = 0; o < P.no; o++) {
        const size_t pl = (size_t)P.R[o] * P.C[o];
        if (gauss) HIP_TRY(hipMemcpyAsync(gauss + go, pyr + P.lvl_off[o], sizeof(float) * (P.L + 3) * pl, hipMemcpyDeviceToHost, ctx->stream));
        if (dog) HIP_TRY(hipMemcpyAsync(dog + dgo, pyr + P.lvl_off[o] + (P.L + 3) * pl, sizeof(float) * (P.L + 2) * pl, hipMemcpyDeviceToHost, ctx->stream));
        go += (P.L + 3) * pl; dgo += (P.L + 2) * pl;
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return VFSMS_OK;
}

// How many strips of (h, w) one group may hold under the context's pyramid budget (at least one)
int sift_group_strips(vfsms_ctx *ctx, int h, int w, const vfsms_sift_params *p, int *g_out)
{
    SiftPlan P;
    TRY(sift_plan(h, w, p, &P));
    static const long long env = getenv("VFSMS_SIFT_GROUP_BYTES") ? atoll(getenv("VFSMS_SIFT_GROUP_BYTES")) : 0;
    const size_t budget = env > 0 ? (size_t)env : ctx->sift_group_bytes;
    *g_out = (int)std::max<size_t>(1, std::min<size_t>(budget / std::max<size_t>(sift_strip_bytes(P), 1), 32768));
    return VFSMS_OK;
}

// Detect and describe g strips of one shape (one group: their pyramids are resident together).  The caller arena holds the launch
// records (a few hundred bytes per strip).  counts: 4 ints per strip in device memory that outlives the group -- [0] candidates,
// [1] keypoints before removeDuplicated, [2] keypoints.  Two host syncs per group, whatever g is: the candidate counts size the
// candidate and keypoint arrays, the keypoint counts size what is kept (out[k]: exact, from ctx->sift_pool).  kp_tmp (optional):
// the group's full keypoint records in ctx->sift_kp, strip k's at kp_tmp + SIFT_MAX_PEAKS * cand0[k]; valid until the next group.
int sift_group_device(vfsms_ctx *ctx, const SiftSrcHost *srcs, int g, int h, int w, const vfsms_sift_params *p, int *counts,
                      SiftStripOut *out, const vfsms_keypoint **kp_tmp)
{
    SiftPlan P;
    TRY(sift_plan(h, w, p, &P));
    hipStream_t st = ctx->stream;
    for (int k = 0; k < g; k++) { out[k].n = 0; out[k].xy = nullptr; out[k].desc = nullptr; out[k].d8 = nullptr; out[k].nrm = nullptr; out[k].cand0 = 0; }
    HIP_TRY(hipMemsetAsync(counts, 0, sizeof(int) * 4 * g, st));
    if (P.no == 0) return VFSMS_OK;
    std::vector<SiftSrc> hs(g);
    for (int k = 0; k < g; k++) { hs[k].p = srcs[k].p; hs[k].stride = srcs[k].stride; }
    SiftSrc *d_srcs;
    TRY(ctx_upload_small(ctx, hs.data(), sizeof(SiftSrc) * g, (void **)&d_srcs));
    float *pyr; int *rowc; size_t zs;
    TRY(sift_build_pyramid(ctx, d_srcs, g, h, w, P, &pyr, &rowc, &zs));
    SiftOcts Os;
    sift_octs(P, pyr, &Os);
    SiftCfg cfg;
    cfg.L = P.L;
    cfg.thr = (float)(int)floor(0.5 * p->contrast_threshold / P.L * 255);
    cfg.contrast = (float)p->contrast_threshold; cfg.edge = (float)p->edge_threshold; cfg.sigma = (float)p->sigma;
    int *pos = rowc + P.nslots + 1;
    const unsigned G = (unsigned)g;
    int slot0 = 0;
    for (int o = 0; o < P.no; o++) {
        k_sift_extrema<<<dim3(P.R[o], P.L, G), 256, 0, st>>>(Os.o[o], cfg, o, rowc + slot0, nullptr, nullptr, zs, nullptr);
        slot0 += P.L * P.R[o];
    }
    k_sift_scan<<<G, 1024, 0, st>>>(rowc, pos, P.nslots, zs, nullptr, 0, counts, -1, 0);
    HIP_TRY(hipGetLastError());
    std::vector<int> hc((size_t)4 * g);
    HIP_TRY(hipMemcpyAsync(hc.data(), counts, sizeof(int) * 4 * g, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));                               // sync 1 of the group: the candidate counts size the rest
    std::vector<SiftSeg> segs(g);
    size_t ncand = 0; int maxc = 0;
    for (int k = 0; k < g; k++) {
        segs[k].cand0 = (int)ncand; segs[k].ncand = hc[4 * k]; segs[k].desc = nullptr; segs[k].xy = nullptr;
        out[k].cand0 = (int)ncand;
        ncand += hc[4 * k]; maxc = std::max(maxc, hc[4 * k]);
        if (ncand * SIFT_MAX_PEAKS > (size_t)INT_MAX / 2) { vfsms_set_error("sift: too many candidates in one group (%zu)", ncand); return VFSMS_ERR_CAPACITY; }
    }
    if (ncand == 0) return VFSMS_OK;
    const size_t nkp_max = ncand * SIFT_MAX_PEAKS;
    // the group's candidates and keypoints in ctx->sift_kp: one description, walked to size the buffer and to carve it
    SiftCand *cand; float *angles; int *npk, *kpos, *keep, *keep_pos; vfsms_keypoint *kp0, *kp1;
    auto kp_layout = [&](ArenaWalk &a) {
        cand = a.take<SiftCand>(ncand); angles = a.take<float>(nkp_max);
        npk = a.take<int>(ncand + g); kpos = a.take<int>(ncand + g);
        kp0 = a.take<vfsms_keypoint>(nkp_max); kp1 = a.take<vfsms_keypoint>(nkp_max);
        keep = a.take<int>(nkp_max + g); keep_pos = a.take<int>(nkp_max + g);
    };
    ArenaWalk count;
    kp_layout(count);
    TRY(ctx->sift_kp.reserve(count.off + 4096, st, (count.off + 4096) / 4));
    ArenaWalk a{ctx->sift_kp.as<char>(), 0, ctx->sift_kp.bytes()};
    kp_layout(a);
    if (!a.ok) { vfsms_set_error("sift: keypoint scratch too small"); return VFSMS_ERR_CAPACITY; }
    SiftOcts *d_os; SiftSeg *d_segs;
    TRY(ctx_upload_small(ctx, &Os, sizeof(SiftOcts), (void **)&d_os));
    TRY(ctx_upload_small(ctx, segs.data(), sizeof(SiftSeg) * g, (void **)&d_segs));
    slot0 = 0;
    for (int o = 0; o < P.no; o++) {
        k_sift_extrema<<<dim3(P.R[o], P.L, G), 256, 0, st>>>(Os.o[o], cfg, o, nullptr, pos + slot0, cand, zs, d_segs);
        slot0 += P.L * P.R[o];
    }
    // grids cover the largest strip of the group; workgroups beyond a strip's own counts leave at once
    const unsigned gk = (unsigned)(((size_t)maxc * SIFT_MAX_PEAKS + 255) / 256);
    k_sift_orient<<<dim3(maxc, 1, G), 64, 0, st>>>(d_os, zs, d_segs, cand, angles, npk);
    k_sift_scan<<<G, 1024, 0, st>>>(npk, kpos, 0, 0, d_segs, 1, counts, -1, 1);
    k_sift_emit<<<dim3((maxc + 255) / 256, 1, G), 256, 0, st>>>(d_segs, cand, angles, npk, kpos, kp0);
    k_sift_dedup<<<dim3(gk, 1, G), 256, 0, st>>>(d_segs, kp0, counts, keep);
    k_sift_scan<<<G, 1024, 0, st>>>(keep, keep_pos, 0, 0, d_segs, SIFT_MAX_PEAKS, counts, 1, 2);
    k_sift_compact<<<dim3(gk, 1, G), 256, 0, st>>>(d_segs, kp0, counts, keep, keep_pos, kp1);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(hc.data(), counts, sizeof(int) * 4 * g, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));                               // sync 2 of the group: the keypoint counts size what is kept
    int maxn = 0;
    for (int k = 0; k < g; k++) {
        const int n = hc[4 * k + 2];
        out[k].n = n; maxn = std::max(maxn, n);
        if (n == 0) continue;
        const size_t npad = sift_pad_rows(n);
        out[k].xy = (float *)sift_pool_alloc(ctx, sizeof(float) * 2 * n);
        out[k].desc = (float *)sift_pool_alloc(ctx, sizeof(float) * 128 * (size_t)n);
        out[k].d8 = (int8_t *)sift_pool_alloc(ctx, 128 * npad);
        out[k].nrm = (int *)sift_pool_alloc(ctx, sizeof(int) * npad);
        if (!out[k].xy || !out[k].desc || !out[k].d8 || !out[k].nrm) return VFSMS_ERR_CAPACITY;
        segs[k].desc = out[k].desc; segs[k].xy = out[k].xy;
    }
    if (kp_tmp) *kp_tmp = kp1;
    if (maxn == 0) return VFSMS_OK;
    TRY(ctx_upload_small(ctx, segs.data(), sizeof(SiftSeg) * g, (void **)&d_segs));
    k_sift_describe<<<dim3(maxn, 1, G), 64, 0, st>>>(d_os, zs, d_segs, kp1, counts);
    HIP_TRY(hipGetLastError());
    return VFSMS_OK;
}

int sift_detect_describe_device(vfsms_ctx *ctx, const uint8_t *d_img, int h, int w, const vfsms_sift_params *p,
                                float *kps_xy, float *desc, vfsms_keypoint *kps_full, int cap, int *n_out)
{
    *n_out = 0;
    sift_pool_reset(ctx);
    int *counts = (int *)sift_pool_alloc(ctx, sizeof(int) * 4);
    if (!counts) return VFSMS_ERR_CAPACITY;
    SiftSrcHost src = {d_img, w};
    SiftStripOut o;
    const vfsms_keypoint *kp1 = nullptr;
    TRY(sift_group_device(ctx, &src, 1, h, w, p, counts, &o, &kp1));
    hipStream_t st = ctx->stream;
    const int n = o.n;
    *n_out = n;
    if (n > cap) {
        HIP_TRY(hipStreamSynchronize(st));
        vfsms_set_error("sift: %d keypoints exceed the caller's capacity %d", n, cap);
        return VFSMS_ERR_CAPACITY;
    }
    if (n > 0) {
        if (kps_xy) HIP_TRY(hipMemcpyAsync(kps_xy, o.xy, sizeof(float) * 2 * n, hipMemcpyDeviceToHost, st));
        if (desc) HIP_TRY(hipMemcpyAsync(desc, o.desc, sizeof(float) * 128 * (size_t)n, hipMemcpyDeviceToHost, st));
        if (kps_full) HIP_TRY(hipMemcpyAsync(kps_full, kp1, sizeof(vfsms_keypoint) * n, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    return VFSMS_OK;
}
