// focus_kernels.hip -- Method.focusStack: a focus series of one stage position fused into one all-in-focus tile, for gfx950.
//
// The arithmetic is this project's specification (tests/focus_ref.py restates it in numpy; everything is integer, so every stage must equal
// it exactly; there is no reference counterpart):
//   luma     L = the byte (gray) or (29 B + 150 G + 77 R + 128) >> 8 (colour, B G R)
//   measure  M = |2 L - L(x-1) - L(x+1)| + |2 L - L(y-1) - L(y+1)|, indices clamped to the plane; M <= 1020
//   focus    F_i = the sum of M_i over (2R + 1)^2, indices clamped, no rounding; R <= 31, F <= 1020 * 63^2 < 2^22
//   index    D = the smallest i of the largest F_i, uint8
//   median   D replaced once by the 5th smallest of its 3 x 3 neighbourhood, indices clamped
//   compose  out = plane[D]
//   scores   S_i = the sum of M_i over the plane, int64
//
//   k_focus_select<TH>  one workgroup of 256 threads owns TH x 64 output pixels and loops over the N planes itself.  Per plane, five phases
//                       in LDS with a barrier between them:
//                         A  the rows of the block plus a halo of R + 1, as raw bytes: aligned dwords of a row go from global memory to LDS
//                            as dwords (the LDS copy keeps the row's alignment), the ragged head and tail byte by byte
//                         B  raw -> luma bytes, the clamping of columns and rows folded in
//                         C  M (uint16) of the block plus a halo of R, evaluated AT the clamped coordinates (M of a replicated border pixel
//                            is that pixel's M, not the Laplacian of a replicated image)
//                         D  row sums of 2R + 1 (uint16: <= 64 260), four adjacent outputs per thread from one sliding window; the block's
//                            own M summed for the plane's score (wave reduction, one LDS atomic per wave into the block's partial)
//                         E  column sums by a sliding window down TH / 4 consecutive rows of one column per thread -> F in a register,
//                            compared with the running (best F, best i) in registers
//                       No per-plane F or M goes to global memory: a plane is read once plus its halo, and D is written once.
//                       The block leaves its n partial scores (uint32: at most 32 x 64 x 1020) in a scratch row of its own and
//                       k_focus_score_sum adds the rows up per plane: exact, and no two blocks meet on one address (vector atomics of
//                       every wave into scores[i] made the 16 k blocks of a 2048^2 stack queue on n addresses, and set the kernel's time)
//                       LDS: raw is dead once the luma stands, M lies over it; the luma is dead once M stands, the row sums lie over it.
//   k_focus_scores      S alone, for mode "plane" and vfsms_focus_scores: tiles of any shapes, a grid row of workgroups per tile
//   k_focus_compose     the 3 x 3 median of D (a 19-exchange network over nine bytes), the chosen plane's pixel gathered (1 or 3 bytes), out and
//                       the final D written; const_d >= 0 (mode "plane") takes that plane everywhere
#include "common.h"
#include "tile_table.h"
#include <algorithm>

#define FOCUS_TW 64                    // block width in pixels = one wave64 per block row
#define FOCUS_THREADS 256

struct FocusPlane { const uint8_t *ptr; int stride, h, w, ch; };      // h, w, ch: k_focus_scores alone (a stack has one shape)

// what k_focus_select carves from its dynamic LDS (bytes); host and device size it by the same function
struct FocusLds { int raw_pitch, l_pitch, m_pitch, rows_l, rows_m, off_b, total; };
__host__ __device__ __forceinline__ FocusLds focus_lds(int TH, int R, int ch)
{
    FocusLds s;
    const int lw = FOCUS_TW + 2 * R + 2;                    // staged columns: the block plus a halo of R + 1
    s.rows_l = TH + 2 * R + 2; s.rows_m = TH + 2 * R;
    s.raw_pitch = ((lw * ch + 3 + 3) & ~3) + 4;              // up to 3 bytes of alignment shift in front, whole dwords
    s.l_pitch = (lw + 3) & ~3;
    s.m_pitch = FOCUS_TW + 2 * R;                            // uint16 entries
    const int raw = s.rows_l * s.raw_pitch, m = s.rows_m * s.m_pitch * 2, a = raw > m ? raw : m;      // raw, then M over it
    const int lum = s.rows_l * s.l_pitch, rs = s.rows_m * FOCUS_TW * 2, b = lum > rs ? lum : rs;      // luma, then the row sums over it
    s.off_b = (a + 15) & ~15;
    s.total = s.off_b + ((b + 15) & ~15);
    return s;
}

__device__ __forceinline__ int focus_clamp(int v, int hi) { return min(max(v, 0), hi); }

// the items (j, c) of a rows x width array dealt to the block's threads, FOCUS_THREADS apart, row-major: thread t starts at item t and steps
// without a division (width is a runtime value: it depends on R)
struct FocusWalk {
    int j, c, dj, dc, width;
    __device__ __forceinline__ FocusWalk(int tid, int w) : j(tid / w), c(tid - (tid / w) * w), dj(FOCUS_THREADS / w), dc(FOCUS_THREADS - (FOCUS_THREADS / w) * w), width(w) {}
    __device__ __forceinline__ void step() { j += dj; c += dc; if (c >= width) { c -= width; j++; } }
};

template <int TH>
__global__ __launch_bounds__(FOCUS_THREADS) void k_focus_select(const FocusPlane *planes, int n, int h, int w, int ch, int R, uint8_t *D,
                                                                 uint32_t *partials)
{
    extern __shared__ __align__(16) uint8_t focus_smem[];
    __shared__ uint32_t acc[VFSMS_FOCUS_MAX_PLANES];         // the block's share of every plane's score
    const FocusLds S = focus_lds(TH, R, ch);
    uint8_t *raw = focus_smem, *Lt = focus_smem + S.off_b;
    uint16_t *Mt = (uint16_t *)focus_smem, *Ht = (uint16_t *)(focus_smem + S.off_b);
    const int tid = threadIdx.x, x0 = blockIdx.x * FOCUS_TW, y0 = blockIdx.y * TH;
    const int gx_l = x0 - R - 1, gy_l = y0 - R - 1;          // the global coordinates of the luma array's entry (0, 0)
    const int lw = FOCUS_TW + 2 * R + 2;
    // the bytes of a row this block needs: the columns [cx0, cx1) of the plane
    const int cx0 = max(gx_l, 0), cx1 = min(x0 + FOCUS_TW + R + 1, w);
    const int bx0 = cx0 * ch, nb = (cx1 - cx0) * ch;
    const int ndw_max = (nb + 3 + 3) / 4;
    constexpr int RPT = TH / 4;                               // rows per thread in phase E
    const int col = tid & 63, r0 = (tid >> 6) * RPT;
    uint32_t bestF[RPT]; int bestI[RPT];
    for (int k = 0; k < RPT; k++) { bestF[k] = 0; bestI[k] = 0; }
    if (tid < VFSMS_FOCUS_MAX_PLANES) acc[tid] = 0;          // (the barriers of the first plane stand between this and the first add)

    for (int i = 0; i < n; i++) {
        const uint8_t *base = planes[i].ptr; const int stride = planes[i].stride;
        // ---- A: raw bytes.  Row j holds the plane's row clamp(gy_l + j); its byte k lies at raw[j][shift + k], shift = the row's misalignment
        for (FocusWalk k(tid, ndw_max); k.j < S.rows_l; k.step()) {
            const int j = k.j, q = k.c;
            const uint8_t *row = base + (size_t)focus_clamp(gy_l + j, h - 1) * stride + bx0;
            const int shift = (int)((uintptr_t)row & 3);
            if (4 * q >= shift + nb) continue;
            const int k0 = 4 * q - shift;                    // the row byte of the dword's first byte
            uint32_t v = 0;
            if (k0 >= 0 && k0 + 4 <= nb) v = *(const uint32_t *)(row + k0);          // wholly inside the row: one aligned dword
            else
                for (int b = 0; b < 4; b++)
                    if (k0 + b >= 0 && k0 + b < nb) v |= (uint32_t)row[k0 + b] << (8 * b);
            *(uint32_t *)(raw + j * S.raw_pitch + 4 * q) = v;
        }
        __syncthreads();
        // ---- B: luma.  Entry (j, c) is L at (clamp(gy_l + j), clamp(gx_l + c))
        for (FocusWalk k(tid, lw); k.j < S.rows_l; k.step()) {
            const int j = k.j, c = k.c;
            const uint8_t *row = base + (size_t)focus_clamp(gy_l + j, h - 1) * stride + bx0;
            const int shift = (int)((uintptr_t)row & 3);
            const uint8_t *p = raw + j * S.raw_pitch + shift + (focus_clamp(gx_l + c, w - 1) - cx0) * ch;
            Lt[j * S.l_pitch + c] = ch == 1 ? p[0] : (uint8_t)((29u * p[0] + 150u * p[1] + 77u * p[2] + 128u) >> 8);
        }
        __syncthreads();
        // ---- C: M.  Entry (j, c) is M at (cy, cx) = (clamp(y0 - R + j), clamp(x0 - R + c)); its neighbours are clamped again, and all of them
        // lie inside the luma array: cy +- 1 clamped stays within [y0 - R - 1, y0 + TH + R], the columns likewise
        for (FocusWalk k(tid, S.m_pitch); k.j < S.rows_m; k.step()) {
            const int j = k.j, c = k.c;
            const int cy = focus_clamp(y0 - R + j, h - 1), cx = focus_clamp(x0 - R + c, w - 1);
            const int ly = cy - gy_l, lx = cx - gx_l;
            const int lu = focus_clamp(cy - 1, h - 1) - gy_l, ld = focus_clamp(cy + 1, h - 1) - gy_l;
            const int ll = focus_clamp(cx - 1, w - 1) - gx_l, lr = focus_clamp(cx + 1, w - 1) - gx_l;
            const int v = 2 * Lt[ly * S.l_pitch + lx];
            const int m = abs(v - Lt[ly * S.l_pitch + ll] - Lt[ly * S.l_pitch + lr]) + abs(v - Lt[lu * S.l_pitch + lx] - Lt[ld * S.l_pitch + lx]);
            Mt[j * S.m_pitch + c] = (uint16_t)m;
        }
        __syncthreads();
        // ---- D: row sums, and the score of the pixels this block owns
        for (int it = tid; it < S.rows_m * (FOCUS_TW / 4); it += FOCUS_THREADS) {
            const int j = it / (FOCUS_TW / 4), c = (it - j * (FOCUS_TW / 4)) * 4;
            const uint16_t *m = Mt + j * S.m_pitch + c;
            uint32_t s = 0;
            for (int d = 0; d <= 2 * R; d++) s += m[d];
            uint16_t *o = Ht + j * FOCUS_TW + c;
            o[0] = (uint16_t)s;
            for (int k = 1; k < 4; k++) { s += m[2 * R + k] - m[k - 1]; o[k] = (uint16_t)s; }
        }
        {
            uint32_t part = 0;
            if (x0 + col < w)
                for (int k = 0; k < RPT; k++)
                    if (y0 + r0 + k < h) part += Mt[(R + r0 + k) * S.m_pitch + R + col];
            for (int d = 32; d > 0; d >>= 1) part += __shfl_down(part, d, 64);
            if (col == 0 && part) atomicAdd(&acc[i], part);
        }
        __syncthreads();
        // ---- E: column sums down this thread's rows, and the running maximum (strictly larger: the smallest index wins a tie)
        {
            const uint16_t *hc = Ht + r0 * FOCUS_TW + col;
            uint32_t s = 0;
            for (int d = 0; d <= 2 * R; d++) s += hc[d * FOCUS_TW];
            for (int k = 0; k < RPT; k++) {
                if (s > bestF[k]) { bestF[k] = s; bestI[k] = i; }
                if (k + 1 < RPT) s += hc[(2 * R + 1 + k) * FOCUS_TW] - hc[k * FOCUS_TW];
            }
        }
        // (the next plane's phase A writes raw = M, last read before the barrier above; its phase B writes the luma = the row sums read here,
        // behind phase A's barrier)
    }
    if (x0 + col < w)
        for (int k = 0; k < RPT; k++)
            if (y0 + r0 + k < h) D[(size_t)(y0 + r0 + k) * w + x0 + col] = (uint8_t)bestI[k];
    __syncthreads();
    if (tid < n) partials[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * n + tid] = acc[tid];
}

// scores[i] = the sum of the blocks' partials of plane i: one workgroup per plane
__global__ __launch_bounds__(FOCUS_THREADS) void k_focus_score_sum(const uint32_t *partials, unsigned nblocks, int n, unsigned long long *scores)
{
    __shared__ unsigned long long wave_sum[FOCUS_THREADS / 64];
    unsigned long long s = 0;
    for (unsigned b = threadIdx.x; b < nblocks; b += FOCUS_THREADS) s += partials[(size_t)b * n + blockIdx.x];
    for (int d = 32; d > 0; d >>= 1) s += __shfl_down(s, d, 64);
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) scores[blockIdx.x] = wave_sum[0] + wave_sum[1] + wave_sum[2] + wave_sum[3];
}

// ---- scores alone -------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int focus_luma_at(const FocusPlane &t, int y, int x)
{
    const uint8_t *p = t.ptr + (size_t)y * t.stride + x * t.ch;
    return t.ch == 1 ? p[0] : (int)((29u * p[0] + 150u * p[1] + 77u * p[2] + 128u) >> 8);
}

__global__ __launch_bounds__(FOCUS_THREADS) void k_focus_scores(const FocusPlane *tiles, unsigned long long *scores)
{
    const FocusPlane t = tiles[blockIdx.y];
    const unsigned total = (unsigned)t.h * (unsigned)t.w;
    unsigned long long part = 0;
    for (unsigned e = blockIdx.x * FOCUS_THREADS + threadIdx.x; e < total; e += gridDim.x * FOCUS_THREADS) {
        const int y = (int)(e / (unsigned)t.w), x = (int)(e - (unsigned)y * (unsigned)t.w);
        const int v = 2 * focus_luma_at(t, y, x);
        part += abs(v - focus_luma_at(t, y, max(x - 1, 0)) - focus_luma_at(t, y, min(x + 1, t.w - 1))) +
                abs(v - focus_luma_at(t, max(y - 1, 0), x) - focus_luma_at(t, min(y + 1, t.h - 1), x));
    }
    __shared__ unsigned long long wave_sum[FOCUS_THREADS / 64];
    for (int d = 32; d > 0; d >>= 1) part += __shfl_down(part, d, 64);
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = part;
    __syncthreads();
    if (threadIdx.x == 0 && wave_sum[0] + wave_sum[1] + wave_sum[2] + wave_sum[3])      // one vector atomic per workgroup, at most 1024 a tile
        atomicAdd(&scores[blockIdx.y], wave_sum[0] + wave_sum[1] + wave_sum[2] + wave_sum[3]);
}

// ---- compose --------------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void focus_cx(int &a, int &b) { const int lo = min(a, b); b = max(a, b); a = lo; }

__global__ __launch_bounds__(FOCUS_THREADS) void k_focus_compose(const FocusPlane *planes, const uint8_t *D, int h, int w, int ch, int median,
                                                                  int const_d, uint8_t *out, int out_stride, uint8_t *Dout)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    int d;
    if (const_d >= 0) d = const_d;
    else if (!median) d = D[(size_t)y * w + x];
    else {
        const uint8_t *ru = D + (size_t)max(y - 1, 0) * w, *rc = D + (size_t)y * w, *rd = D + (size_t)min(y + 1, h - 1) * w;
        const int xl = max(x - 1, 0), xr = min(x + 1, w - 1);
        int p0 = ru[xl], p1 = ru[x], p2 = ru[xr], p3 = rc[xl], p4 = rc[x], p5 = rc[xr], p6 = rd[xl], p7 = rd[x], p8 = rd[xr];
        focus_cx(p1, p2); focus_cx(p4, p5); focus_cx(p7, p8); focus_cx(p0, p1); focus_cx(p3, p4); focus_cx(p6, p7);
        focus_cx(p1, p2); focus_cx(p4, p5); focus_cx(p7, p8); focus_cx(p0, p3); focus_cx(p5, p8); focus_cx(p4, p7);
        focus_cx(p3, p6); focus_cx(p1, p4); focus_cx(p2, p5); focus_cx(p4, p7); focus_cx(p4, p2); focus_cx(p6, p4);
        focus_cx(p4, p2);
        d = p4;
    }
    const FocusPlane t = planes[d];
    const uint8_t *src = t.ptr + (size_t)y * t.stride + x * ch;
    uint8_t *dst = out + (size_t)y * out_stride + x * ch;
    for (int c = 0; c < ch; c++) dst[c] = src[c];
    Dout[(size_t)y * w + x] = (uint8_t)d;
}

// ---- launchers ----------------------------------------------------------------------------------------------------------------------------------
// the tiles' pointers, strides and shapes as the kernels read them
static_assert(sizeof(FocusPlane) <= 2 * sizeof(TileView), "api.hip reserves two TileView per tile for the table and its staging");
int focus_table_device(vfsms_ctx *ctx, const TileView *tiles, int n, FocusPlane **d_tab)
{
    std::vector<FocusPlane> T(n);
    for (int i = 0; i < n; i++) { T[i].ptr = tiles[i].ptr; T[i].stride = tiles[i].stride; T[i].h = tiles[i].h; T[i].w = tiles[i].w; T[i].ch = tiles[i].ch; }
    return ctx_upload_small(ctx, T.data(), sizeof(FocusPlane) * n, (void **)d_tab);
}

// S of n tiles of any shapes into d_scores (n x uint64, zeroed here)
int focus_scores_device(vfsms_ctx *ctx, const TileView *tiles, int n, unsigned long long *d_scores)
{
    size_t most = 0;
    for (int i = 0; i < n; i++) {
        const size_t px = (size_t)tiles[i].h * tiles[i].w;
        if (px * tiles[i].ch > 0x7fffffffu) { vfsms_set_error("focus_scores: tiles of more than 2^31 - 1 bytes are not supported"); return VFSMS_ERR_UNSUPPORTED; }
        most = std::max(most, px);
    }
    FocusPlane *d_tab;
    TRY(focus_table_device(ctx, tiles, n, &d_tab));
    HIP_TRY(hipMemsetAsync(d_scores, 0, sizeof(unsigned long long) * n, ctx->stream));
    const unsigned bx = (unsigned)std::min<size_t>((most + FOCUS_THREADS * 4 - 1) / (FOCUS_THREADS * 4), 1024);
    ProfScope ps(ctx, "focus_select");
    hipLaunchKernelGGL(k_focus_scores, dim3(std::max(bx, 1u), n), dim3(FOCUS_THREADS), 0, ctx->stream, d_tab, d_scores);
    HIP_TRY(hipGetLastError());
    return VFSMS_OK;
}

// D (h x w, before the median) and S of a stack of n planes of one shape
// the scratch of focus_select_device: a row of n partial scores per block, sized for the smaller block
size_t focus_partials_bytes(int n, int h, int w) { return sizeof(uint32_t) * (size_t)n * ((w + FOCUS_TW - 1) / FOCUS_TW) * ((h + 15) / 16); }

int focus_select_device(vfsms_ctx *ctx, const FocusPlane *d_tab, int n, int h, int w, int ch, int radius, uint8_t *d_index, unsigned long long *d_scores,
                        uint32_t *d_partials)
{
    if ((size_t)h * w * ch > 0x7fffffffu || (h + 15) / 16 > 65535) { vfsms_set_error("focus_stack: tiles of more than 2^31 - 1 bytes or 2^20 rows are not supported"); return VFSMS_ERR_UNSUPPORTED; }
    // 32 rows a block halve the halo a large radius reads and sums again; 16 rows keep more blocks on a CU at the small ones
    const int TH = radius > 8 ? 32 : 16;
    const FocusLds S = focus_lds(TH, radius, ch);
    const dim3 grid((w + FOCUS_TW - 1) / FOCUS_TW, (h + TH - 1) / TH);
    ProfScope ps(ctx, "focus_select");
    // (at most 49 920 bytes -- R = 31, colour, 32 rows -- so the default limit of 64 KiB of dynamic LDS holds)
    if (TH == 32)
        hipLaunchKernelGGL(k_focus_select<32>, grid, dim3(FOCUS_THREADS), (size_t)S.total, ctx->stream, d_tab, n, h, w, ch, radius, d_index, d_partials);
    else
        hipLaunchKernelGGL(k_focus_select<16>, grid, dim3(FOCUS_THREADS), (size_t)S.total, ctx->stream, d_tab, n, h, w, ch, radius, d_index, d_partials);
    hipLaunchKernelGGL(k_focus_score_sum, dim3(n), dim3(FOCUS_THREADS), 0, ctx->stream, d_partials, grid.x * grid.y, n, d_scores);
    HIP_TRY(hipGetLastError());
    return VFSMS_OK;
}

// out and the final D from D (const_d < 0) or from one plane (const_d >= 0: d_index is not read)
int focus_compose_device(vfsms_ctx *ctx, const FocusPlane *d_tab, const uint8_t *d_index, int h, int w, int ch, int median, int const_d,
                         uint8_t *d_out, int out_stride, uint8_t *d_index_out)
{
    ProfScope ps(ctx, "focus_compose");
    hipLaunchKernelGGL(k_focus_compose, dim3((w + 63) / 64, (h + 3) / 4), dim3(FOCUS_THREADS), 0, ctx->stream, d_tab, d_index, h, w, ch, median, const_d,
                       d_out, out_stride, d_index_out);
    HIP_TRY(hipGetLastError());
    return VFSMS_OK;
}
