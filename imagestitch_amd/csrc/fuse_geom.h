// fuse_geom.h -- the fade blend's per-pixel weight geometry, shared by the fade kernels (fuse_kernels.hip), the multi-band
// blend's seam mask (multiband_kernels.hip) and the optimal seam's hand-over to that blend (seam_kernels.hip).
#pragma once
#include "common.h"

// the strip ramps of fuseByFadeInAndFadeOut in closed form, with the reference's float32 expression ((1. * f) * 1.0) / n:
//   col <= row: weightMatA_2[col - i - 1] = weightMatB_2[i] = f(i) / col, f(i) = i (dy >= 0) or col - i;  else  weightMatA_1[i] =
//   weightMatB_1[row - i - 1] = g(i) / row, g(i) = i (dx <= 0) or row - i  (what fuse_weights_body's strip branch stores into the arrays)
// kind 3: getWeightsMatrix's corner ramps (ImageFusion.py:43-190 as fuse_weights_body stores them) from (index, rowIndex, colIndex):
//   rows, index 2 / 1: weightMatB_1[i] = i / ri for 0 <= i <= rowIndex (ri = rowIndex, 0 patched to 1: then only [1] = 1 is written);
//         index 3 / 0: weightMatB_1[i] = (row - i - 1) / (row - ri - 1) for i >= max(rowIndex, 0);   columns alike with colIndex, index 2 / 3 | 0 / 1
//   quotients in float64, stored as float32; everything else stays 1
struct AnalyticRamps {
    int kind, r, c, dx, dy;
    int index, rowIndex, colIndex;
    __device__ __forceinline__ float corner_b(int i, int n, int at, bool counting_up) const
    {
        const int ai = at == 0 ? 1 : at;
        if (counting_up) return (at >= 1 && i <= at) ? (float)((double)i * 1 / ai) : 1.f;
        return i >= max(at, 0) ? (float)((double)(n - i - 1) * 1 / (n - ai - 1)) : 1.f;
    }
    __device__ __forceinline__ float cb_row(int i) const { return corner_b(i, r, rowIndex, index == 2 || index == 1); }
    __device__ __forceinline__ float cb_col(int j) const { return corner_b(j, c, colIndex, index == 2 || index == 3); }
    __device__ __forceinline__ float ratio(int n, int d) const { return ((1.f * (float)n) * 1.0f) / (float)d; }
    __device__ __forceinline__ float a_col(int j) const { return kind == 1 ? ratio(dy >= 0 ? c - 1 - j : j + 1, c) : 1.f; }
    __device__ __forceinline__ float b_col(int j) const { return kind == 1 ? ratio(dy >= 0 ? j : c - j, c) : 1.f; }
    __device__ __forceinline__ float a_row(int i) const { return kind == 2 ? ratio(dx <= 0 ? i : r - i, r) : 1.f; }
    __device__ __forceinline__ float b_row(int i) const { return kind == 2 ? ratio(dx <= 0 ? r - 1 - i : i + 1, r) : 1.f; }
};
// the index range [lo, lo + W) on which a corner ramp is written (corner_b above), W = 0: none.  `at` = rowIndex / colIndex, n = r / c
__host__ __device__ inline void seam_arm(int n, int at, bool up, int &lo, int &W)
{
    if (up) { lo = 0; W = at >= 1 ? (at < n - 1 ? at : n - 1) + 1 : 0; }
    else { lo = at > 0 ? at : 0; W = n - lo > 0 ? n - lo : 0; }
}
// The multi-band blend's seam: M0 = 1 where the fade gives tile A at least tile B's weight (wA >= wB), 0 elsewhere.  wA and wB are
// formed exactly as the fade kernels form them (k_fuse_apply / k_i64_apply), from one of three geometry sources:
//   kind 0: the separable ramp arrays of the statistics kernels, mode[0] = corner flag (wB = wBr wBc, wA = 1 - wB; else wAr wAc, wBr wBc)
//   kind 1 / 2: the strip ramps in closed form (AnalyticRamps, along the columns / rows)
//   kind 3: getWeightsMatrix's corner ramps from the device-side pick {., ., index, rowIndex, colIndex} in mode[0..4]
//   kind 4: an explicit mask plane, label[r][c] != 0 -> A (the optimal seam's label plane, seam_kernels.hip)
struct SeamGeom {
    int kind, r, c, dx, dy;
    const int *mode;
    const float *wAr, *wAc, *wBr, *wBc;
    const uint8_t *label;
    __device__ __forceinline__ float m0(int i, int j) const
    {
        float wA, wB;
        if (kind == 4) return label[(size_t)i * c + j] ? 1.f : 0.f;
        if (kind == 0) {
            wB = wBr[i] * wBc[j];
            wA = mode[0] ? 1 - wB : wAr[i] * wAc[j];
        } else if (kind == 3) {
            const AnalyticRamps AR = {3, r, c, dx, dy, mode[2], mode[3], mode[4]};
            wB = AR.cb_row(i) * AR.cb_col(j); wA = 1 - wB;
        } else {
            const AnalyticRamps AR = {kind, r, c, dx, dy, 0, 0, 0};
            wA = AR.a_row(i) * AR.a_col(j); wB = AR.b_row(i) * AR.b_col(j);
        }
        return wA >= wB ? 1.f : 0.f;
    }
};
