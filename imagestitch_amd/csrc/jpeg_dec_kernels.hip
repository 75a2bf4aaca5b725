// jpeg_dec_kernels.hip -- the device half of the JPEG decoder (Method.jpegDecoder = "device"; specified by tests/jpeg_dec_ref.py).
//
// The host stops behind the entropy decode (jpeg_read_coefficients, csrc/jpeg_host.cpp: jpeg_coefficients_host): what arrives are the
// quantised DCT coefficients of every component, 64 int16 per block in natural order, blocks in block-row-major order, and one uint16[64]
// quantisation table per component.  k_jpeg_idct is libjpeg's default decoder from there to the sample planes: dequantisation
// (coefficient * table entry), jidctint.c's jpeg_idct_islow (JDCT_ISLOW, CONST_BITS = 13, PASS1_BITS = 2) -- the column pass over the
// dequantised block descaled by 11 bits, then the row pass over ITS output descaled by 18 -- the level shift + 128 and the range limit to
// 0..255.  All in int32: within the two conditions tests/jpeg_dec_ref.py states (every intermediate fits int32, every column-pass output
// int16) that is the library's arithmetic, C and SIMD alike; its zero-AC shortcuts yield the values of the full butterflies.  The two
// roundings make the transform non-separable in the last bit: the order column pass -> row pass is part of the specification.
//
// Mapping: 8 lanes per block, so a wave64 covers 8 consecutive blocks and a workgroup of 256 lanes 32.  Lane r of a block loads the block's
// row r as ONE 16-byte access (a block is 128 contiguous bytes: a wave reads 1 KiB contiguous) and the table's row r likewise, multiplies,
// and the 8 x 8 goes through LDS twice: rows -> columns for the column pass (lane c holds column c in registers), columns -> rows for the row
// pass (lane r holds row r), after which the lane stores its 8 bytes -- the same pixel row of 8 horizontally adjacent blocks is 64
// contiguous bytes.  The LDS pitch of a block row is 9 dwords, a block takes 72 (= 8 mod 64): for a fixed element index the 64 lanes of a
// wave touch dwords r * 9 + block * 8 (writes of rows) or 64 consecutive dwords (reads of columns) -- 64 different banks either way.
// One launch covers all components of a file: the block index selects component, table and destination plane.
#include "common.h"

#define JD_BLOCKS_PER_WG 32
#define JD_LDS_PITCH 9
#define JD_LDS_BLOCK (8 * JD_LDS_PITCH)

// jidctint.c: FIX(x) = (int)(x * (1 << 13) + 0.5)
#define JD_FIX_0_298631336 2446
#define JD_FIX_0_390180644 3196
#define JD_FIX_0_541196100 4433
#define JD_FIX_0_765366865 6270
#define JD_FIX_0_899976223 7373
#define JD_FIX_1_175875602 9633
#define JD_FIX_1_501321110 12299
#define JD_FIX_1_847759065 15137
#define JD_FIX_1_961570560 16069
#define JD_FIX_2_053119869 16819
#define JD_FIX_2_562915447 20995
#define JD_FIX_3_072711026 25172

// one 1-D pass of jpeg_idct_islow over x[0..7], every output descaled by SHIFT bits: (v + (1 << (SHIFT - 1))) >> SHIFT, arithmetic shift
template <int SHIFT>
__device__ __forceinline__ void jd_pass(int *x)
{
    int z2 = x[2], z3 = x[6];
    int z1 = (z2 + z3) * JD_FIX_0_541196100;
    int tmp2 = z1 - z3 * JD_FIX_1_847759065;
    int tmp3 = z1 + z2 * JD_FIX_0_765366865;
    z2 = x[0]; z3 = x[4];
    int tmp0 = (z2 + z3) * 8192, tmp1 = (z2 - z3) * 8192;
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = x[7]; tmp1 = x[5]; tmp2 = x[3]; tmp3 = x[1];
    z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2;
    int z4 = tmp1 + tmp3;
    const int z5 = (z3 + z4) * JD_FIX_1_175875602;
    tmp0 *= JD_FIX_0_298631336; tmp1 *= JD_FIX_2_053119869; tmp2 *= JD_FIX_3_072711026; tmp3 *= JD_FIX_1_501321110;
    z1 *= -JD_FIX_0_899976223; z2 *= -JD_FIX_2_562915447;
    z3 = z3 * -JD_FIX_1_961570560 + z5; z4 = z4 * -JD_FIX_0_390180644 + z5;
    tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
    const int half = 1 << (SHIFT - 1);
    x[0] = (tmp10 + tmp3 + half) >> SHIFT; x[7] = (tmp10 - tmp3 + half) >> SHIFT;
    x[1] = (tmp11 + tmp2 + half) >> SHIFT; x[6] = (tmp11 - tmp2 + half) >> SHIFT;
    x[2] = (tmp12 + tmp1 + half) >> SHIFT; x[5] = (tmp12 - tmp1 + half) >> SHIFT;
    x[3] = (tmp13 + tmp0 + half) >> SHIFT; x[4] = (tmp13 - tmp0 + half) >> SHIFT;
}

__global__ void __launch_bounds__(256) k_jpeg_idct(const JpegIdctArgs A)
{
    __shared__ int lds[2][JD_BLOCKS_PER_WG * JD_LDS_BLOCK];
    const int slot = threadIdx.x >> 3, r = threadIdx.x & 7;           // the block's place in the workgroup; the lane's row, then column, then row
    const unsigned b = blockIdx.x * JD_BLOCKS_PER_WG + slot;
    const bool live = b < A.total;
    const int ci = !live ? 0 : (A.ncomp > 2 && b >= A.c[2].first) ? 2 : (A.ncomp > 1 && b >= A.c[1].first) ? 1 : 0;
    const JpegIdctComp C = A.c[ci];
    const unsigned lb = live ? b - C.first : 0;
    int v[8];
    if (live) {
        const uint4 cw = *(const uint4 *)(C.coef + (size_t)lb * 64 + r * 8);        // 8 int16, 16-byte aligned (the staging layout)
        const uint4 qw = *(const uint4 *)(C.quant + r * 8);                         // 8 uint16
        const unsigned cs[4] = { cw.x, cw.y, cw.z, cw.w }, qs[4] = { qw.x, qw.y, qw.z, qw.w };
#pragma unroll
        for (int k = 0; k < 4; k++) {
            v[2 * k] = (int)(short)(cs[k] & 0xffffu) * (int)(qs[k] & 0xffffu);
            v[2 * k + 1] = ((int)cs[k] >> 16) * (int)(qs[k] >> 16);
        }
    } else {
#pragma unroll
        for (int k = 0; k < 8; k++) v[k] = 0;
    }
    int *L0 = lds[0] + slot * JD_LDS_BLOCK, *L1 = lds[1] + slot * JD_LDS_BLOCK;
#pragma unroll
    for (int k = 0; k < 8; k++) L0[r * JD_LDS_PITCH + k] = v[k];                    // row r of the dequantised block
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 8; k++) v[k] = L0[k * JD_LDS_PITCH + r];                    // column r, top to bottom
    jd_pass<11>(v);                                                               // CONST_BITS - PASS1_BITS
#pragma unroll
    for (int k = 0; k < 8; k++) L1[k * JD_LDS_PITCH + r] = v[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 8; k++) v[k] = L1[r * JD_LDS_PITCH + k];                    // row r of the column pass's output
    jd_pass<18>(v);                                                               // CONST_BITS + PASS1_BITS + 3
    if (!live) return;
    const int br = (int)(lb / (unsigned)C.bcols), bc = (int)(lb % (unsigned)C.bcols);
    const int y = br * 8 + r, x0 = bc * 8;
    if (y >= C.rows || x0 >= C.cols) return;                                      // the crop: the grid is whole iMCUs, the plane the image
#pragma unroll
    for (int k = 0; k < 8; k++) v[k] = min(max(v[k] + 128, 0), 255);
    uint8_t *o = C.dst + (size_t)y * C.pitch + x0;
    if (x0 + 8 <= C.cols && (((size_t)o) & 7) == 0) {
        uint2 w;
        w.x = (unsigned)v[0] | ((unsigned)v[1] << 8) | ((unsigned)v[2] << 16) | ((unsigned)v[3] << 24);
        w.y = (unsigned)v[4] | ((unsigned)v[5] << 8) | ((unsigned)v[6] << 16) | ((unsigned)v[7] << 24);
        *(uint2 *)o = w;
    } else {
#pragma unroll
        for (int k = 0; k < 8; k++) if (x0 + k < C.cols) o[k] = (uint8_t)v[k];
    }
}

// stream-ordered.  The caller has checked the record: every component's blocks lie in its coefficient array, its plane holds rows x pitch bytes
int launch_jpeg_idct(hipStream_t stream, const JpegIdctArgs &A)
{
    if (A.ncomp < 1 || A.ncomp > 3 || A.total == 0) { vfsms_set_error("jpeg_idct: nothing to transform"); return VFSMS_ERR_BAD_ARG; }
    const unsigned wgs = (A.total + JD_BLOCKS_PER_WG - 1) / JD_BLOCKS_PER_WG;
    hipLaunchKernelGGL(k_jpeg_idct, dim3(wgs), dim3(256), 0, stream, A);
    HIP_TRY(hipGetLastError());
    return VFSMS_OK;
}
