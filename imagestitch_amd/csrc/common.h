// common.h -- internal declarations shared by the libvfsms translation units (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <condition_variable>
#include <list>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>
#include "../../include/vfsms.h"
#include "arena_walk.h"
#include "device_buf.h"                // with hip_try.h: vfsms_set_error, HIP_TRY, TRY

#define VFSMS_MAX_LAYERS 32      // (nOctaveLayers + 2) * nOctaves
#define VFSMS_MAX_WIN 768        // SURF descriptor window side upper bound (size <= 264 -> 739)

// ---- fast-Hessian layer description (host-built, device-resident table) ---------------------------
#define VFSMS_MAX_OCTAVES 8
// resizeHaarPattern: corner c (x1, y1, x2, y2) of box k (Dx 0-2, Dy 3-5, Dxy 6-9) of the 9 x 9 pattern scaled to `size`:
// cvRound(size / 9.f * v) == (2 size v + 9) / 18 -- 2 size v is never an odd multiple of 9, so there are no ties to break
// (ctx_prepare_surf checks the table it builds with the float expression against this one).
#ifdef __HIPCC__
__host__ __device__
#endif
constexpr int vfsms_haar_corner(int size, int k, int c)
{
    constexpr int src[10][4] = { {0, 2, 3, 7}, {3, 2, 6, 7}, {6, 2, 9, 7}, {2, 0, 7, 3}, {2, 3, 7, 6}, {2, 6, 7, 9},
                                 {1, 1, 4, 4}, {5, 1, 8, 4}, {1, 5, 4, 8}, {5, 5, 8, 8} };
    return (2 * size * src[k][c] + 9) / 18;
}
// the 9 x 9 pattern coordinate (0..9) behind corner c of box k: the integral ROW of a tap depends on it alone, which is what the
// row-staged coarse Hessian (k_hessian_rows2) indexes its LDS row slots with
#ifdef __HIPCC__
__host__ __device__
#endif
constexpr int vfsms_haar_src(int k, int c)
{
    constexpr int src[10][4] = { {0, 2, 3, 7}, {3, 2, 6, 7}, {6, 2, 9, 7}, {2, 0, 7, 3}, {2, 3, 7, 6}, {2, 6, 7, 9},
                                 {1, 1, 4, 4}, {5, 1, 8, 4}, {1, 5, 4, 8}, {5, 5, 8, 8} };
    return src[k][c];
}
struct LayerPat {
    int size, step, margin, octave;   // margin = (size/2)/step
    int box[10][4];                   // dx1, dy1, dx2, dy2 for Dx[3], Dy[3], Dxy[4]  (resizeHaarPattern)
    float w[10];
};

struct SurfTables {                   // orientation lattice + descriptor Gaussian (SURFInvoker ctor)
    int nOriSamples;
    int aptx[128], apty[128];
    float aptw[128];
    float DW[400];
    // sliding-window membership of a rounded gradient angle a (0..360): bit w of the 72-bit row a is set when the ORI_WIN = 60 degree
    // window starting at 5 w holds it, i.e. |a - 5 w| < 30 or > 330 (SURFInvoker's test, evaluated once per angle on the host)
    uint32_t oriMask[361][3];
};

struct Cand {                         // NMS survivor before sorting
    float x, y, size, response;
    int octave, class_id;
    int layer, i, j;
};

// ---- one ROI's device working set; arrays of these drive every batched kernel ---------------------
#define VFSMS_PATCH_ROW 464       // 441 patch bytes, then at VFSMS_PATCH_TRIG the (sin, cos) of the window rotation
#define VFSMS_PATCH_TRIG 448
struct RoiDev {
    const uint8_t *img;
    int stride, h, w;
    int32_t *sum;                     // (h+1) x (w+1)
    uint16_t *pair;                   // h x w: pixel (y, x) in the low byte, pixel (min(y+1, h-1), x) in the high byte (k_pair_rows)
    int32_t *icarry; int ipitch;      // integral-image band carries: ceil(h/16) x ipitch column sums (ipitch = w rounded up to 4)
    float *det[VFSMS_MAX_LAYERS];
    int cap;
    int *counters;                    // [0] n candidates, [1] n kept after deletion, [2] overflow flag
    Cand *cand;
    vfsms_keypoint *kps;              // sorted (KeypointGreater), angle filled by orientation; size=-1 -> deleted
    uint8_t *patch;                   // cap x VFSMS_PATCH_ROW: 21 x 21 resized descriptor windows, rows aligned with kps
    int *keep_pos;                    // exclusive scan of keep flags
    int *order;                       // surviving keypoints grouped by descriptor-window class (largest first); counts in counters[12..15]
    float *kps_xy;                    // compacted [n][2]
    float *desc;                      // compacted [n][D]
    vfsms_keypoint *kps_out;          // compacted
};

// ---- descriptor work list of a launch (round 5) -------------------------------------------------------------
// One 32-byte record per surviving keypoint, written by k_desc_recs in the order the descriptor kernels draw them: everything a workgroup
// needs to start on a keypoint in ONE scalar load -- before, a ticket led through counters -> order[] -> kps[] -> the trig values behind the
// patch row, four dependent trips to memory with the workgroup's four waves waiting.
struct DescRec { int roi, k, win, pad; float sin_dir, cos_dir, x, y; };      // win = (int)(21 * size * 1.2f / 9) unclamped
// The plan of a launch (k_desc_plan, one workgroup): per ticket head q (= XCD) the slice of the record arrays it serves.  Head q owns the ROIs
// q, q + 8, ...; its slice of the BIG array (windows > 64 px, k_describe) is [class 0 of its ROIs, ROI after ROI][class 1 + 2 of its first
// ROI][of its second] ..., of the SMALL array (k_describe_small) [class 3 of its first ROI][of its second] ...
#define DESC_PLAN_HEADS 8
#define VFSMS_MAX_ROIS 256        // ROIs of one fused launch
struct DescPlan {
    int big_start[DESC_PLAN_HEADS], big_n0[DESC_PLAN_HEADS], big_tickets[DESC_PLAN_HEADS];     // records before the head's slice, its class-0 records, its tickets
    int small_start[DESC_PLAN_HEADS], small_tickets[DESC_PLAN_HEADS];
    int split;                        // 21: every class-0 keypoint is 21 tickets, one per output row of its patch (small batches); else 1
    int seg_base[VFSMS_MAX_ROIS][4];  // record index of the first keypoint of (roi, class) in its array
};

// ---- ORB working set of one ROI --------------------------------------------------------------------------
#define VFSMS_ORB_MAX_LEVELS 8
struct OrbDev {
    int h, w;
    uint8_t *lv[VFSMS_ORB_MAX_LEVELS]; int ls[VFSMS_ORB_MAX_LEVELS];      // pyramid level images + row strides (level 0 = the ROI itself)
    int lw[VFSMS_ORB_MAX_LEVELS], lh[VFSMS_ORB_MAX_LEVELS]; float lscale[VFSMS_ORB_MAX_LEVELS];
    uint8_t *bl[VFSMS_ORB_MAX_LEVELS];                                    // blurred levels (descriptor sampling)
    uint8_t *score[VFSMS_ORB_MAX_LEVELS]; uint8_t *nms[VFSMS_ORB_MAX_LEVELS];
    int *hist;                        // [levels][256] FAST score histogram of NMS survivors
    int *counters;                    // [1] keypoints, [2] overflow, [4 + level] survivors of the FAST-score cut before any capacity
                                      // clamp; thr1 / n1 / n2 live in the same block
    int *thr1; int *n1; int *n2;
    int cap1, cap2, cap;
    int *k1_xy; float *k1_resp;       // per level: survivors of the FAST-score cut (+ Harris response)
    int *k2_xy; float *k2_resp; float *k2_angle;   // per level: final keypoints
    float *kps_xy; uint8_t *desc; vfsms_keypoint *kps_out;                // level-major final arrays
};
struct OrbTables { int nfeat[VFSMS_ORB_MAX_LEVELS]; int umax[34]; int half_patch; int patch_size; int kf[7]; int pattern[1024]; };

// ---- one image of an enhancement batch (equalizeHist / CLAHE before detectAndDescribe) --------------------------------------
struct EnhJob { const uint8_t *src; int stride, h, w, eh, ew; uint8_t *dst; int *hist; uint8_t *lut; };   // eh, ew: size extended to the CLAHE grid

// ---- device-resident feature set (keypoints + descriptors of one image; Stitcher.tempImageFeature's payload) ---------------
struct FeatRec { float *kps_xy; void *desc; int n, dim; int64_t block = 0; };   // kps_xy / desc point into the shared allocation `block` (feat_blocks); a set without keypoints: block 0, null pointers
struct FeatBlock { DevBuf base; int refs; };

// ---- one (query ROI, train ROI) matching job --------------------------------------------------------
struct MatchDev {
    const float *q; const float *t;   // descriptors
    const int *nq_ptr; const int *nt_ptr;   // device-side counts (RoiDev.counters+1) or host-filled
    const float *kq; const float *kt; // keypoints xy (may be null for raw matching)
    int capq;
    int dim;
    // partial 2-NN per (split, query)
    float *p_d1; float *p_d2; int *p_i1; int nsplit;
    // MFMA candidate filter (fused SURF path): per (query, split, lane half) lists of (score bits, train index) + their counts
    uint2 *c_ent; int *c_cnt;
    float2 *c_m12;                    // per (list, query): best / second-best hi-only score of the bounds pass
    unsigned short *q16, *t16;        // fp16 operands of the filter (k_bf_split16): BF16_ROW uint16 per descriptor row
    // integer 2-NN (fused SIFT path, k_bf_i8_d128): descriptors as int8 (element - 128), 128 bytes per row, and the squared norms of those
    // rows; rows padded to whole 64-row tiles (zero rows, norm BFI_PAD_NORM)
    const int8_t *q8, *t8; const int *qn2, *tn2;
    // merged
    float *d1; float *d2; int *i1;
    int *match_flag; int *match_pos;
    int32_t *pairs;                   // [capq][2] (train, query)
    int32_t *votes;                   // [capq][2] (dx, dy) after dropping (0,0)
    int *mcount;                      // [0] n matches, [1] n votes
    int32_t *result;                  // VFSMS_ATTEMPT_INTS
    int pairs_given;                  // pairs[] supplied by the caller (vfsms_mode_offset): do not rewrite
    // overlap verification (verify_kernels.hip): the job's two strips as RAW tile pixels (query strip A, train strip B; also when the
    // detector saw an enhanced copy), their common size, and the job's sums + score (8 x uint64, layout in verify_kernels.hip)
    const uint8_t *va; const uint8_t *vb; int vsa, vsb, vh, vw;
    unsigned long long *vsum;
};

// ---- context ------------------------------------------------------------------------------------------
// pending: an async upload the compute stream has not yet waited for; bytes: size of an owned allocation;
// fill: 0 filled (or being copied: `ready` is recorded), 1 reserved -- a decoder thread still owes the pixels (vfsms_tile_fill), 2 the decoder gave up
struct TileRec { uint8_t *ptr = nullptr; int h = 0, w = 0, stride = 0; bool owned = false; hipEvent_t ready = nullptr; bool pending = false; int ch = 1; size_t bytes = 0; int fill = 0; };   // made by tile_rec, entered by tile_register (tile_table.h)
struct StageBuf { uint8_t *ptr; size_t bytes; };                    // device staging of one decoded source image (vfsms_tile_fill_pair)
struct PoolEnt { size_t bytes; uint8_t *ptr; hipEvent_t idle; };   // a freed tile buffer (tile_pool_return, tile_table.h); idle: recorded on the compute stream when the tile was freed
// device scratch of the JPEG encoder (jpeg_enc_kernels.hip), grown to the largest band seen: quantised coefficients, interval sizes + offsets,
// the coded stream, and (vfsms_jpeg_encode_device only) the staged image
struct JpegScratch { DevBuf coef, sizes, out, img; };
// tile order (Method.pyramidCompression = "jpeg"): the tile rows of one level that a call encodes.  Row y of the rows x cols level lies at
// src + (y - src_row0) * pitch (src 256-byte aligned, src_bytes readable); `tile_rows` rows of tiles from row0 (a multiple of the tile side) on
struct JpegTileJob { const uint8_t *src; size_t src_bytes, pitch; int src_row0, rows, cols, row0, tile_rows; };
// what the counting half of a tile-order encode leaves for the writing half; tile_offs[0 .. n_tiles]: the tiles' offsets in the payload
struct JpegTilesRun { int n_tiles, n_int, ipt, interval, bpm, plen; uint8_t prefix[44]; uint32_t *d_sizes; unsigned long long *d_offs; int *d_err; std::vector<unsigned long long> tile_offs; };
// device scratch of the lossless tile coder (deflate_kernels.hip), grown to the largest call seen: the predicted bytes of the call's tiles, the
// records per tile and per chunk (DflArgs' arrays), the coded streams
struct DeflateScratch { DevBuf pred, meta, out, png; };     // png: the PNG coder's own records (deflate_kernels.hip): the rows' filter types, the segments' Adler sums
// the tile rows of one level as the kernels see them (JpegTileJob's fields; ntx tiles a row, first_tile: its first tile among the call's)
struct DflJobDev { const uint8_t *src; unsigned long long src_bytes, pitch; int src_row0, rows, cols, row0, ntx; long long first_tile; };
// one call of the coder: n_tiles tiles of `nbytes` = tile x tile x ch bytes in `nchunks` chunks each.  Per tile: adler (the two sums), hist
// (288 a tile), lens (288 a tile), table (288 a tile), sizes / offs (the streams' bytes and where they start, offs[n_tiles] the total), eob (the
// bit of the stream at which the end-of-block code starts).  Per chunk: bounds (its first and last run boundary), reach (the last boundary in
// front of it, the first behind it), chunk_bits (its tokens' bits, then where they start among the tile's).  out: the payload in words.
// To the passes behind predict a tile is a byte string at pred + tile * nbytes (nbytes: the stride, a multiple of 16) of which `len` bytes are
// live, `last_len` in the call's last string; a tile's are all nbytes.  head_bits: the bits in front of a string's tokens in its stream; png: the
// strings are a PNG's segments (deflate_kernels.hip), framed as IDAT chunks
struct DflArgs {
    DflJobDev job[VFSMS_PYRAMID_MAX_LEVELS + 1]; int n_jobs, tile, ch, bgr, nbytes, nchunks, n_tiles, len, last_len, head_bits, png;
    uint8_t *pred; int2 *bounds, *reach; uint32_t *adler, *hist; uint8_t *lens; uint32_t *table, *sizes; unsigned long long *offs, *eob;
    uint32_t *chunk_bits; uint32_t *out; unsigned long long out_words; int *err;
};
// what the counting half of a deflate call leaves for the writing half; tile_offs[0 .. n_tiles]: the tiles' offsets in the payload
struct DeflateTilesRun { DflArgs a; std::vector<unsigned long long> tile_offs; };
#define VFSMS_PYR_CODEC_JPEG 0
#define VFSMS_PYR_CODEC_DEFLATE 1
// the pending rows of levels 1 .. levels between the bands of vfsms_canvas_encode_pyramid_tiles: level k's rows [base[k], base[k] + have[k])
// (fewer than a tile row of them) at buf + off[k], with room for the share of a band of `band` rows behind them; next: the row0 expected;
// ch, R[k] x C[k]: the canvas's levels, and codec: the coder the walk feeds (VFSMS_PYR_CODEC_*; vfsms_canvas_encode_pyramid_tiles_deflate walks
// the same state), set when a walk starts.  The operations are canvas_band.h's: begin -> plan -> commit per band
struct PyrPlan;
struct PyrPending {
    DevBuf buf; int tile = 0, levels = -1, band = 0, next = 0; int base[VFSMS_PYRAMID_MAX_LEVELS + 1] = {}, have[VFSMS_PYRAMID_MAX_LEVELS + 1] = {}; size_t off[VFSMS_PYRAMID_MAX_LEVELS + 1] = {};
    int ch = 0, R[VFSMS_PYRAMID_MAX_LEVELS + 1] = {}, C[VFSMS_PYRAMID_MAX_LEVELS + 1] = {}, codec = VFSMS_PYR_CODEC_JPEG;
    int begin(const char *who, int rows, int cols, int ch, int row0, int nrows, int tile, int levels, hipStream_t stream, int codec);
    int plan(const char *who, const uint8_t *pix, int row0, int nrows, PyrPlan *p) const;
    int commit(const PyrPlan &p, hipStream_t stream);
};
// move-only: the record owns its buffers wherever it lies (the canvas map, the context's spare slot, a canvas under construction); an
// empty record owns nothing.  Destroying one frees without a synchronisation: api.hip's canvas_release synchronises first
struct CanvasRec { DevBuf pix, mask; int rows = 0, cols = 0, ch = 0; DevBuf d_err, scratch; std::vector<int32_t> placed; int mb_levels = 4; int seam_blend = 0; DevBuf pyr; JpegScratch jpeg; DeflateScratch deflate; PyrPending pend; };   // deflate: the lossless tile coder's scratch for the band being encoded (vfsms_canvas_encode_pyramid_tiles_deflate), allocated on first use, released with the canvas; pend: the rows of the reduced levels that do not fill a tile row yet (vfsms_canvas_encode_pyramid_tiles; canvas_band.h has its operations and the band contract of all four write-out routes), sized at the band that starts a walk, grown by a longer band, released with the canvas; jpeg: the encoder's scratch for the band being encoded (vfsms_canvas_encode_jpeg_rows), allocated on first use, released with the canvas; pyr: the reduced levels of the band being downloaded (vfsms_canvas_download_rows_pyramid), sized on first use; d_err: sticky "degenerate fuse geometry" flag for calls made without an info readback, read with every band that leaves (canvas_flag_read / canvas_flag_verdict); scratch: the fuse's statistics records + ramps; placed: (y0, x0, y1, x1) of every tile rectangle written so far = the canvas's validity (canvas_fuse_device counts the valid pixels of a ROI from it)
struct FftPlan { int M, N, nb; void *fwd, *inv, *fwd_info, *inv_info; size_t fwd_work, inv_work; };   // rocfft_plan / rocfft_execution_info
struct PhaseJobHost { const uint8_t *a, *b; int sa, sb; };
struct PhasePeak { double v; long long idx; };                      // a peak of the correlation surface: value, row-major index in the ORIGINAL (untransposed) padded surface; idx < 0: absent
// where a correlation batch leaves the K largest peaks of every job's surface (phase_resolve_kernels.hip): peaks [nb][K]; the chunks' scratch
// comes from the arena (phase_peaks_bytes)
struct PhasePeakSink { int K; PhasePeak *peaks; };
struct ProfRec { int id; hipEvent_t a, b; };
struct ShadeRec { int h, w, ch; DevBuf gain; uint16_t *q8; uint8_t *prof; bool estimated; };   // a shading field (shading_kernels.hip): one allocation behind `gain`; q8 / prof hold nothing for an uploaded gain
struct DeepRec { DevBuf pix; int h = 0, w = 0; };               // a 16-bit gray tile (deep_kernels.hip): h x w uint16 samples, dense, in an allocation of its own; a record and a handle kind of their own, so no entry that takes a TileRec can be handed one
struct DeepShadeRec { int h = 0, w = 0, pedestal = 0; DevBuf gain; uint16_t *smooth = nullptr, *prof = nullptr; bool estimated = false; };   // a shading field for deep tiles (deep_shading_kernels.hip): one allocation behind `gain`, uint16 planes; smooth / prof hold nothing for an uploaded gain; a record and a handle kind of their own, so no vfsms_shading_* entry can be handed one
struct SiftChunk { DevBuf mem; size_t off; };                   // one allocation of the SIFT batch's pool (sift_pool_alloc)

struct vfsms_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    // bump arena for per-call scratch
    DevBuf arena; size_t arena_off = 0;
    // pinned staging for small results
    PinBuf pinned; size_t pinned_off = 0;
    int kp_cap_override = 0;
    int offset_estimator = VFSMS_OFFSET_MODE, offset_tol = 3;   // the vote tail of every fused path (vfsms_ctx_set_offset_estimator)
    int offset_verifier = VFSMS_VERIFY_NONE, verify_min_pixels = 0; double verify_threshold = 0.0;   // the acceptance check behind that tail (vfsms_ctx_set_offset_verifier)
    int phase_resolver = VFSMS_PHASE_RESOLVE_NONE, phase_peaks = 2, phase_min_pixels = 4096; double phase_threshold = 0.5;   // method 2 of vfsms_pairs_offsets (vfsms_ctx_set_phase_resolver)
    // SURF tables
    vfsms_surf_params cur_params = {}; bool tables_valid = false;
    DevBuf d_layers; int n_layers = 0;   // LayerPat[VFSMS_MAX_LAYERS]
    DevBuf d_tables;                     // SurfTables
    DevBuf d_area_tab;                   // INTER_AREA tables of every descriptor-window size (ctx_prepare_area_tab)
    vfsms_orb_params cur_orb = {}; bool orb_valid = false; DevBuf d_orb_tables;   // OrbTables
    std::unordered_map<int64_t, TileRec> tiles;
    std::mutex tiles_mu; std::condition_variable tiles_cv;   // what belongs to which thread: tile_table.h
    std::mutex stage_mu; std::vector<StageBuf> stage_pool;   // device staging buffers of the decoder threads (vfsms_tile_fill_pair), the pools they share
    std::vector<StageBuf> pin_pool;                          // pinned host staging of the same threads (also under stage_mu)
    hipStream_t copy_stream = nullptr;                            // H2D uploads of tiles, overlapped with compute (vfsms_tile_upload_async)
    // second compute stream: the MFMA-bound 2-NN search of the first part of a batch runs on it beside the VALU / TA-bound detect stage of
    // the second part (attempt_surf_impl); created on first use, always joined back into `stream` before a call returns
    hipStream_t stream2 = nullptr; hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    std::vector<PoolEnt> tile_pool;      // freed tile buffers, reused by allocation size (no hipMalloc / hipFree per step)
    size_t tile_pool_bytes = 0;
    std::vector<hipEvent_t> event_pool;
    std::unordered_map<int64_t, CanvasRec> canvases;
    DevBuf mb_scratch;                                             // fp32 pyramid planes of the multi-band blend (multiband_kernels.hip): grown to the largest blend, freed with the context
    DevBuf seam_scratch;                                           // energy, predecessor, seam and label planes of the optimal-seam fuse (seam_kernels.hip): grown to the largest seam, freed with the context
    DevBuf shade_scratch;                                          // uint32 row sums + channel sums of the shading estimate (shading_kernels.hip): grown to the largest tile, freed with the context
    std::unordered_map<int64_t, ShadeRec> shade_fields;
    std::unordered_map<int64_t, DeepRec> deep_tiles;               // the 16-bit gray tiles (vfsms_deep_*): handles from next_handle like every other kind
    std::unordered_map<int64_t, DeepShadeRec> deep_fields;         // the shading fields of deep tiles (vfsms_deep_shading_*)
    DevBuf lens_scratch;                                           // the copy a tile is resampled from (lens_kernels.hip): grown to the largest tile, freed with the context
    DevBuf sift_scratch;                                           // SIFT pyramid + row counts (sift_kernels.hip): grown to the largest image, freed with the context
    DevBuf sift_kp;                                                // SIFT candidates, keypoints and descriptors, likewise
    std::vector<SiftChunk> sift_pool;                              // what a SIFT strip keeps until the match stage of its batch (positions, descriptors, their int8 form): reused from call to call, freed with the context
    size_t sift_group_bytes = (size_t)4 << 30;                     // pyramid bytes resident at once in a fused SIFT batch (VFSMS_SIFT_GROUP_BYTES overrides)
    JpegScratch jpeg_scratch;                                      // vfsms_jpeg_encode_device's scratch, freed with the context
    DeflateScratch deflate_scratch;                                // vfsms_deflate_encode_tiles_device's scratch, freed with the context
    CanvasRec spare_canvas;                                  // (or an empty record) the buffers of the last canvas freed: a session's mosaics are of one size, and hipMalloc / hipFree of a canvas (28 GB at configs[4]) cost more than the walk
    std::unordered_map<int64_t, FeatRec> feats;
    std::unordered_map<int64_t, FeatBlock> feat_blocks;      // one allocation for the sets of a call (vfsms_features_surf, one set; vfsms_features_surf_batch, a chunk's), freed with its last set
    int64_t next_handle = 1;
    std::list<FftPlan> plans;            // list: get_plan hands out stable pointers
    std::vector<std::pair<int, DevBuf>> fft_tabs;   // twiddle tables exp(-2 pi i q / L) of the LDS transforms of phase_kernels.hip, one per length
    // optional per-stage timing with HIP events on this context's stream (vfsms_profile_*)
    bool prof_on = false;
    std::vector<ProfRec> prof_recs;
    std::vector<hipEvent_t> prof_pool;
    std::vector<std::string> prof_names;
    std::vector<double> prof_ms;
    std::vector<long long> prof_calls;
};

int prof_begin(vfsms_ctx *ctx, const char *name);      // returns a record index or -1 when profiling is off
void prof_end(vfsms_ctx *ctx, int rec);
struct ProfScope {
    vfsms_ctx *c; int r;
    ProfScope(vfsms_ctx *ctx, const char *name) : c(ctx), r(prof_begin(ctx, name)) {}
    ~ProfScope() { prof_end(c, r); }
};

int ctx_arena_reserve(vfsms_ctx *ctx, size_t bytes);             // ensure capacity (may sync + realloc), reset offset
void *ctx_arena_alloc(vfsms_ctx *ctx, size_t bytes, size_t align = 256);   // one-off allocations; a record's arrays come from its layout function:
ArenaWalk ctx_arena_walk(vfsms_ctx *ctx);                        // a carving walk that starts where the arena stands
int ctx_arena_commit(vfsms_ctx *ctx, const ArenaWalk &a, const char *what);   // move the arena behind a walk that fitted; else `what` is the error, VFSMS_ERR_CAPACITY
int ctx_prepare_surf(vfsms_ctx *ctx, const vfsms_surf_params *p);

// ---- runs of consecutive records of one shape -----------------------------------------------------------------
// Kernels whose grid is cut from the image size are launched once per RUN of consecutive ROIs of one shape: a batch of the incremental search
// mixes the 409 x 2048 strips of the column pairs with the 2048 x 409 strips of the turn candidates, and a grid sized for the largest height
// AND the largest width of the batch dispatched five times the workgroups either shape needs (empty ones exit at once, but a batch of 96 ROIs
// paid 1.3 ms per launch for dispatching them).  Callers order their ROIs by shape (api.hip: shape_order).  Rec: any record with h and w.
struct ShapeRun { int first, count, h, w; };
template <typename Rec>
static std::vector<ShapeRun> shape_runs(const Rec *recs, int n)
{
    std::vector<ShapeRun> runs;
    for (int r = 0; r < n; r++) {
        if (!runs.empty() && runs.back().h == recs[r].h && runs.back().w == recs[r].w) runs.back().count++;
        else runs.push_back(ShapeRun{r, 1, recs[r].h, recs[r].w});
    }
    return runs;
}

// ---- kernel launchers (each is stream-ordered, no host sync) --------------------------------------------
struct TileView;                   // a handed-over resident tile: pointer, row stride in bytes, rows, columns, channels (tile_table.h)
// surf_kernels.hip
// every record's device arrays are described ONCE, by X_layout(ArenaWalk &, XDev *, shape): X_bytes counts with it, X_carve carves with it
void surf_roi_layout(ArenaWalk &a, RoiDev *r, const uint8_t *img, int stride, int h, int w, int cap, const vfsms_surf_params *p);
struct DescWork { int *tickets; DescPlan *plan; DescRec *rec_big, *rec_small; };     // the work list of one describe launch
void surf_describe_layout(ArenaWalk &a, DescWork *d, size_t capsum);
int launch_integral(vfsms_ctx *ctx, const RoiDev *d_rois, int nrois, int maxh, int maxw);
size_t integral_carry_bytes(int h, int w);
int launch_surf_detect(vfsms_ctx *ctx, const RoiDev *d_rois, const RoiDev *h_rois, int nrois,
                       const vfsms_surf_params *p);
int launch_surf_describe(vfsms_ctx *ctx, const RoiDev *d_rois, const RoiDev *h_rois, int nrois,
                         const vfsms_surf_params *p);
// match_kernels.hip
void match_layout(ArenaWalk &a, MatchDev *m, int capq, int dim, int nsplit);
void match_filter_layout(ArenaWalk &a, MatchDev *m, int capq, int capt, int cns);
int launch_max_norm2_d64(vfsms_ctx *ctx, const float *a, int n, unsigned *d_out);
int launch_bf_l2_filtered(vfsms_ctx *ctx, const MatchDev *d_jobs, int njobs, int capq, int capt, int cns);
int launch_bf_l2(vfsms_ctx *ctx, const MatchDev *d_jobs, int njobs, int capq, int nsplit, int dim);
#define BFI_PAD_NORM 0x3fffffff
struct PackJob { const float *src; const int *n_ptr; int8_t *dst; int *nrm; };   // one strip's descriptors -> int8 rows + norms
int launch_pack_i8_d128(vfsms_ctx *ctx, const PackJob *d_jobs, int njobs, int max_rows);
int launch_bf_i8_d128(vfsms_ctx *ctx, const MatchDev *d_jobs, int njobs, int capq, int nsplit);
int launch_bf_hamming(vfsms_ctx *ctx, const MatchDev *d_jobs, int njobs, int capq, int nsplit, int max_dist);   // 32-byte rows: search + merge
// What follows a search, or the caller's own pairs.  The fused paths VOTE: the context's estimator and verifier apply.  The operators
// behind a user's own matchDescriptors / getOffsetByMode take one of the other three, which never look at the context's settings.
enum MatchTailKind {
    TAIL_VOTE,          // ratio test, the CONTEXT's estimator + tolerance, the CONTEXT's verifier -> the job's result row
    TAIL_PAIRS,         // ratio test, order-preserving compaction (k_match_scan) -> pairs, mcount
    TAIL_KNN,           // merge only -> d1, d2, i1
    TAIL_GIVEN_PAIRS    // votes of the caller's pairs, the estimator + tolerance NAMED HERE, no verifier -> the job's result row
};
struct MatchTail {
    MatchTailKind kind;
    double ratio;                             // the ratio test of an L2 search
    int max_dist;                             // the distance bound of a Hamming search
    int offset_evaluate;                      // the vote's threshold
    bool merged = false;                      // the search has merged and flagged already (launch_bf_hamming): no k_merge_ratio
    int estimator = VFSMS_OFFSET_MODE, tol = 0;
};
int launch_match_tail(vfsms_ctx *ctx, const MatchDev *d_jobs, int njobs, int capq, const MatchTail &tail);
// consensus_kernels.hip
int launch_consensus(vfsms_ctx *ctx, const MatchDev *d_jobs, int njobs, int capq, int tol, int offset_evaluate);
// verify_kernels.hip
int launch_verify(vfsms_ctx *ctx, const MatchDev *d_jobs, int njobs, double threshold, int min_pixels);
// adjust_kernels.hip: the offset search of Method.globalAdjust = "ncc".  One job: two whole tiles of one shape (pointers, row strides in
// bytes) and the predicted offset the window is centred on (tile B's pixel (r, c) meets tile A's pixel (r + dx, c + dy))
#define VFSMS_ADJUST_MAX_RADIUS 16
struct AdjJob { const uint8_t *a, *b; int sa, sb, h, w, dx, dy; };
size_t adjust_sums_bytes(int njobs, int radius);
int launch_adjust_search(vfsms_ctx *ctx, const AdjJob *d_jobs, const AdjJob *h_jobs, int njobs, int radius, int min_pixels,
                         unsigned long long *d_sums, int32_t *d_best4, int32_t *d_surface);
// wide_kernels.hip: the two-level search of Method.failedPairRepair = "stage" (tests/ncc_wide_ref.py).  One job: the full-resolution pair
// (src), its reduced planes in arena scratch (ac, bc: hc x wc bytes, row stride sc) and the block phase (ox, oy) = (dx, dy) mod factor
struct WideJob { AdjJob src; uint8_t *ac, *bc; int sc, hc, wc, ox, oy; };
int launch_wide_reduce(vfsms_ctx *ctx, const WideJob *d_jobs, const WideJob *h_jobs, int njobs, int factor);
int launch_wide_seeds(vfsms_ctx *ctx, const WideJob *d_jobs, int njobs, int radius, int factor, int peaks, const int32_t *d_surface,
                      AdjJob *d_fine, int32_t *d_seeds, int32_t *d_out8);
int launch_wide_pick(vfsms_ctx *ctx, int njobs, int peaks, const int32_t *d_fine_best4, int32_t *d_seeds, int32_t *d_out8);
int launch_overlap_sums(vfsms_ctx *ctx, const AdjJob *d_jobs, const AdjJob *h_jobs, int njobs, unsigned long long *d_out6);
// orb_kernels.hip
int ctx_prepare_orb(vfsms_ctx *ctx, const vfsms_orb_params *p);
void orb_roi_layout(ArenaWalk &a, OrbDev *r, const uint8_t *img, int stride, int h, int w, const vfsms_orb_params *p, int cap1, int cap2, int cap);
int launch_orb(vfsms_ctx *ctx, const OrbDev *d_rois, const OrbDev *h_rois, int nrois, const vfsms_orb_params *p);
// phase_kernels.hip
int phase_correlate_device(vfsms_ctx *ctx, const uint8_t *a, int stride_a, const uint8_t *b, int stride_b,
                           int h, int w, double *d_out3);
int phase_correlate_batch_device(vfsms_ctx *ctx, const PhaseJobHost *jobs, int nb, int h, int w, double *d_out3, const PhasePeakSink *sink = nullptr);
// scratch of a batch (the spectra, partial maxima and job records are typed in phase_kernels.hip); work: rocFFT's, when its plans ask for one
struct PhaseScratch { double *RE; void *FQ, *CP; uint8_t *TB; void *partial; PhasePeak *ppart; void *jobs; void *work; size_t work_bytes; };
int phase_layout(vfsms_ctx *ctx, ArenaWalk &a, PhaseScratch *s, int h, int w, int nb, int K);
void phase_peaks_layout(ArenaWalk &a, PhaseScratch *s, int h, int w, int nb, int K);
int phase_bytes(vfsms_ctx *ctx, int h, int w, int nb, size_t *bytes);
size_t phase_peaks_bytes(int h, int w, int nb, int K);            // what a batch with a sink takes from the arena beyond phase_bytes
int phase_destroy_plans(vfsms_ctx *ctx);                          // the rocFFT plans of the context, before its streams go
void phase_surface_size(int h, int w, int *M, int *N);            // the padded size of the surface of an h x w strip, in the strip's own orientation
// phase_resolve_kernels.hip: RE holds njobs stored planes of SM x SN (tr: each the transpose of its surface); partial: njobs * phase_peaks_blocks(SM) * K records
int phase_peaks_blocks(int SM);
int launch_phase_peaks(vfsms_ctx *ctx, const double *RE, int njobs, int SM, int SN, int tr, int K, PhasePeak *partial, PhasePeak *peaks);
size_t phase_resolve_sums_bytes(int njobs, int K);
int launch_phase_resolve(vfsms_ctx *ctx, const PhaseJobHost *d_jobs, const PhasePeak *d_peaks, int njobs, int K, int oM, int oN, int h, int w,
                         double threshold, int min_pixels, unsigned long long *d_sums, int32_t *d_rows, int32_t *d_cands, int32_t *d_peaks_out);
int ctx_upload_small(vfsms_ctx *ctx, const void *src, size_t bytes, void **d);   // launch records through the pinned staging buffer
int ctx_copy_small(vfsms_ctx *ctx, const void *src, size_t bytes, void *d);      // the same into an array a layout walk took
// ingest_kernels.hip: one decoded source image (format 0: 8-bit gray, 1: Y Cb Cr interleaved, 2: Y Cb Cr X; or the raw 4:2:0 planes of
// jpeg_decode_raw420_host) -> the gray and / or the B G R tile
int ingest_source_pixel_bytes(int format);
int launch_ingest_split(hipStream_t stream, const uint8_t *src, uint8_t *gray, uint8_t *bgr, long long n, int format);
int launch_ingest_420(hipStream_t stream, const uint8_t *src, int pw, int ph, int h, int w, uint8_t *gray, uint8_t *bgr);
// enhance_kernels.hip
int enhance_check_args(const char *who, int mode, int tiles);
void enhance_layout(ArenaWalk &a, EnhJob *J, const uint8_t *src, int stride, int h, int w, int mode, int tiles);
size_t enhance_scratch_bytes(int h, int w, int mode, int tiles);
int enhance_carve(vfsms_ctx *ctx, EnhJob *J, const uint8_t *src, int stride, int h, int w, int mode, int tiles);
int launch_enhance(vfsms_ctx *ctx, const EnhJob *d_jobs, const EnhJob *h_jobs, int n, int mode, double clip_limit, int tiles);
// fuse_kernels.hip.  Placement: how one tile goes onto a canvas -- the nine ints of a geometry row of vfsms_canvas_assemble_resident plus
// the tile's shape.  The tile rectangle is h x w at canvas (y0, x0); the fuse ROI is [ry0, ry1) x [rx0, rx1) in canvas coordinates (empty: a
// plain paste); (dx, dy) is the tile's offset from its predecessor; mode is a vfsms_canvas_mode.  api.hip checks a record once (canvas_check)
// and the launchers below trust it.
struct Placement {
    int h, w, y0, x0, ry0, rx0, ry1, rx1, dx, dy, mode;
    int r() const { return ry1 > ry0 ? ry1 - ry0 : 0; }
    int c() const { return rx1 > rx0 ? rx1 - rx0 : 0; }
};
int canvas_fuse_device(vfsms_ctx *ctx, CanvasRec *cv, const uint8_t *d_tile, const Placement &p, int32_t *info);   // FADE, TRIG, MULTIBAND, SEAMLINE
int canvas_blend_device(vfsms_ctx *ctx, CanvasRec *cv, const uint8_t *d_tile, const Placement &p);                 // AVERAGE, MAXIMUM, MINIMUM
int canvas_paste_device(vfsms_ctx *ctx, CanvasRec *cv, const uint8_t *d_tile, const Placement &p);
size_t canvas_scratch_bytes(int rows, int cols);
int canvas_scratch_init(vfsms_ctx *ctx, CanvasRec *cv);
// multiband_kernels.hip (SeamGeom: fuse_geom.h)
#define VFSMS_MB_MAX_LEVELS 8
struct SeamGeom;
int mb_blend_canvas(vfsms_ctx *ctx, CanvasRec *cv, const uint8_t *d_tile, const Placement &p, const SeamGeom &G, int levels);
int mb_blend_i64(vfsms_ctx *ctx, const long long *dA, const long long *dB, int r, int c, int ch, const SeamGeom &G, int levels, uint8_t *d_out);
// seam_kernels.hip: fuseMethod "optimalSeamLine".  hostkind 1 / 2: a strip the host decided on, 0: geometry from mode[] on the device; wmax:
// an upper bound of a seam's positions; blend 0 none, 1 multiBandBlending with `levels`
int seam_fuse_canvas(vfsms_ctx *ctx, CanvasRec *cv, const uint8_t *d_tile, const Placement &p, int hostkind, const int *mode, int wmax,
                     int blend, int levels);
int seam_fuse_i64(vfsms_ctx *ctx, const long long *dA, const long long *dB, int r, int c, int ch, int dx, int dy, const int *mode,
                  int blend, int levels, uint8_t *d_out, int32_t *d_seam);
// shading_kernels.hip: Method.shadingCorrection.  Tiles as TileView (tile_table.h), all h rows of w * ch bytes
#define VFSMS_SHADE_MAX_TILES 4096
#define VFSMS_SHADE_MAX_RADIUS 127
int shade_estimate_device(vfsms_ctx *ctx, const TileView *tiles, int n, int h, int w, int ch, int percentile, int radius,
                          uint16_t *gain, uint16_t *q8, uint8_t *prof);
int shade_apply_device(vfsms_ctx *ctx, const TileView *tiles, int n, int h, int w, int ch, const uint16_t *gain);
// the ONE box / level / gain sequence, behind both profiles: q (h rows of w * ch uint16) smoothed in place, its gain; shade_plane_fits first
int shade_plane_fits(const char *who, int h, size_t row_samples);
int shade_field_device(vfsms_ctx *ctx, uint16_t *q, int h, int w, int ch, int radius, uint16_t *gain);
// exposure_kernels.hip: Method.exposureCompensation.  A pair: two whole tiles (pointers, row strides in bytes, rows, row lengths in
// BYTES = w * ch) of one channel count and the offset in pixels (tile B's pixel (r, c) meets tile A's pixel (r + dx, c + dy)).  ExpJob is
// what the kernel reads: the rectangle of B that has a partner in A, cut on the host in 64 bits, everything in bytes
struct ExpPairHost { const uint8_t *a, *b; int sa, sb, ha, wa, hb, wb, ch, dx, dy; };
struct ExpJob { const uint8_t *a, *b; int sa, sb, wa, wb, r0, nrows, c0, c1, dx, dyb; };
int overlap_stats_device(vfsms_ctx *ctx, const ExpPairHost *pairs, int n, int lo, int hi, unsigned long long *d_out3);   // d_out3: [n][3] = N, Sa, Sb
int exposure_apply_device(vfsms_ctx *ctx, const TileView *tiles, int n, const uint16_t *gain_q12);
// focus_kernels.hip: Method.focusStack.  Tiles as TileView (tile_table.h); FocusPlane: the same as the kernels
// read it, uploaded once per call (focus_table_device).  d_index: h x w bytes, D before the median; d_scores: n sums, set by the launchers
#define VFSMS_FOCUS_MIN_PLANES 2
#define VFSMS_FOCUS_MAX_PLANES 64
#define VFSMS_FOCUS_MAX_RADIUS 31
#define VFSMS_FOCUS_MAX_TILES 4096
struct FocusPlane;
int focus_table_device(vfsms_ctx *ctx, const TileView *tiles, int n, FocusPlane **d_tab);
int focus_scores_device(vfsms_ctx *ctx, const TileView *tiles, int n, unsigned long long *d_scores);
size_t focus_partials_bytes(int n, int h, int w);          // d_partials of focus_select_device: the blocks' shares of the scores
int focus_select_device(vfsms_ctx *ctx, const FocusPlane *d_tab, int n, int h, int w, int ch, int radius, uint8_t *d_index, unsigned long long *d_scores,
                        uint32_t *d_partials);
int focus_compose_device(vfsms_ctx *ctx, const FocusPlane *d_tab, const uint8_t *d_index, int h, int w, int ch, int median, int const_d,
                         uint8_t *d_out, int out_stride, uint8_t *d_index_out);
// deep_kernels.hip: 16-bit gray tiles (tests/deep_ref.py).  DeepSrc: a deep tile as the launchers take it (dense h x w samples at src;
// dst: the dense h x w bytes of its reduced view, reduce only).  The tables of a call go through the arena: deep_table_bytes /
// deep_mosaic_table_bytes say how much.  DeepRect, DeepBins: deep_bins.h
#define VFSMS_DEEP_MAX_TILES 4096
#define VFSMS_DEEP_MAX_SIDE 32768
#define VFSMS_DEEP_MAX_BIN_ENTRIES ((size_t)1 << 26)
struct DeepSrc { const uint16_t *src; uint8_t *dst; int h, w; };
struct DeepRect;
struct DeepBins;
size_t deep_table_bytes(int n);
int deep_window_device(vfsms_ctx *ctx, const DeepSrc *tiles, int n, unsigned long long k_lo, unsigned long long k_hi, int *lo, int *hi);
int deep_reduce_device(vfsms_ctx *ctx, const DeepSrc *tiles, int n, int lo, int hi);
size_t deep_mosaic_table_bytes(int n, const DeepBins &B);
int deep_mosaic_device(vfsms_ctx *ctx, const DeepSrc *tiles, const DeepRect *at, int n, const DeepBins &B, int cols, int row0, int nrows, int mode,
                       int feather, uint16_t *d_out);
// deep_shading_kernels.hip: flat-field correction of deep tiles (tests/deep_shading_ref.py).  The tiles of a call are of ONE shape; their
// pointer table goes through the arena (8 bytes a tile).  prof, field, gain: dense h x w uint16 planes, 256-byte aligned
int deep_shade_estimate_device(vfsms_ctx *ctx, const DeepSrc *tiles, int n, int h, int w, int percentile, int radius, int pedestal,
                               uint16_t *gain, uint16_t *field, uint16_t *prof);
int deep_shade_apply_device(vfsms_ctx *ctx, const DeepSrc *tiles, int n, int h, int w, int pedestal, const uint16_t *gain);
// lens_kernels.hip: Method.lensCorrection (tests/lens_ref.py).  A block job: two whole tiles of ONE shape and channel count (pointers, row
// strides in bytes) and the offset (tile B's pixel (r, c) meets tile A's pixel (r + dx, c + dy)); lens_lattice: its block lattice.  A tile
// to resample: a TileView (tile_table.h).  A centre coordinate below 0 stands for the tile's own middle
#define VFSMS_LENS_MAX_RADIUS 16
#define VFSMS_LENS_MAX_BLOCK 128
#define VFSMS_LENS_MAX_SIDE 16384
#define VFSMS_LENS_MAX_COEF (1 << 28)
struct LensBlockHost { const uint8_t *a, *b; int sa, sb, h, w, ch, dx, dy; };
void lens_lattice(int h, int w, int dx, int dy, int block, int radius, int *r0, int *c0, int *nby, int *nbx);
int lens_blocks_device(vfsms_ctx *ctx, const LensBlockHost *jobs, const long long *h_first, int njobs, int block, int radius,
                       int32_t *d_best4, int32_t *d_surface);
int lens_remap_device(vfsms_ctx *ctx, const uint8_t *d_src, uint8_t *d_dst, int dstride, int h, int w, int ch, int a1_q30, int a2_q30,
                      int cy2, int cx2, int interp);
int lens_apply_device(vfsms_ctx *ctx, const TileView *tiles, int n, int a1_q30, int a2_q30, int cy2, int cx2, int interp);
// jpeg_host.cpp / jpeg_enc_kernels.hip: the device JPEG encoder (tests/jpeg_enc_ref.py)
const uint8_t *jpeg_std_huff_bits(int ac, int chroma);
const uint8_t *jpeg_std_huff_vals(int ac, int chroma);
void jpeg_quant_tables(int quality, uint8_t q[2][64]);
int jpeg_check_geometry(const char *who, int rows, int cols, int ch, int quality, int restart_mcus, int *interval);
int jpeg_encode_band_device(vfsms_ctx *ctx, JpegScratch *s, const uint8_t *d_img, int rows, int cols, int ch, size_t pitch, int bgr,
                            int row0, int nrows, int quality, int interval, uint8_t *out, size_t cap, size_t *nbytes);
// the same encoder in tile order (tests/tiff_jpeg_ref.py): the refusals every entry shares, *interval = MCUs per restart interval; the
// prefix of every tile stream (SOI, SOF0, DRI when restart_mcus > 0, SOS: at most 41 bytes) -> its length; the two halves of a call
int jpeg_check_tile_geometry(const char *who, int tile, int ch, int quality, int restart_mcus, int *interval);
int jpeg_tile_prefix(int tile, int ch, int restart_mcus, uint8_t *out);
int jpeg_tiles_count_device(vfsms_ctx *ctx, JpegScratch *s, const JpegTileJob *jobs, int n_jobs, int ch, int bgr, int tile, int quality, int restart_mcus,
                            int interval, const int *d_flag, int *flag, JpegTilesRun *run);
int jpeg_tiles_write_device(vfsms_ctx *ctx, JpegScratch *s, const JpegTilesRun *run, uint8_t *out);
// deflate_kernels.hip: the lossless tile coder (tests/deflate_ref.py; the coder's rules are csrc/deflate_core.h's): the refusals every entry
// shares, and the two halves of a call, shaped as the JPEG tile route's
int deflate_check_tile_geometry(const char *who, int tile, int ch);
int deflate_tiles_count_device(vfsms_ctx *ctx, DeflateScratch *s, const JpegTileJob *jobs, int n_jobs, int ch, int bgr, int tile, const int *d_flag, int *flag,
                               DeflateTilesRun *run);
int deflate_tiles_write_device(vfsms_ctx *ctx, DeflateScratch *s, const DeflateTilesRun *run, uint8_t *out);
// deflate_kernels.hip: the PNG coder of Method.pngEncoder = "device" (tests/png_ref.py; the rules are csrc/png_core.h's).  Rows [row0, row0 + nrows)
// of the rows x cols x ch image at pix (rows `pitch` bytes apart; B G R when bgr) -> the IDAT chunks of their segments of `segment_rows` rows in
// `out` on the host, and the Adler-32 of their filtered bytes.  The row above row0 is read from the image.  *nbytes = the size, also on
// VFSMS_ERR_CAPACITY (nothing is written then).  d_flag (an int on the device, may be NULL) comes to *flag.  Synchronises the stream
int png_check_geometry(const char *who, int segment_rows, int rows, int cols, int ch);
int png_encode_band_device(vfsms_ctx *ctx, DeflateScratch *s, const uint8_t *pix, int rows, int cols, int ch, size_t pitch, int bgr, int row0, int nrows,
                           int segment_rows, uint8_t *out, size_t cap, size_t *nbytes, uint32_t *adler, const int *d_flag, int *flag);
// jpeg_host.cpp: the decode on the host (the system's libjpeg-turbo), into planes or into the raw 4:2:0 planes on the iMCU grid
int jpeg_decode_host(const unsigned char *jpeg, size_t nbytes, int want_planes, unsigned char *out, size_t cap, int *h_out, int *w_out, int *comp_out);
int jpeg_decode_raw420_host(const unsigned char *jpeg, size_t nbytes, unsigned char *out, size_t cap, int *h_out, int *w_out);
// jpeg_host.cpp / jpeg_dec_kernels.hip: the device half of the JPEG decoder (tests/jpeg_dec_ref.py).  A component of one launch: its blocks
// (64 int16 each, natural order, block-row-major on a grid `bcols` wide), its table (uint16[64], natural order), the plane it becomes (`rows`
// x `cols` samples kept of the grid, `pitch` bytes apart) and the index of its first block among the launch's `total`
struct JpegIdctComp { const int16_t *coef; const uint16_t *quant; uint8_t *dst; int pitch, bcols, rows, cols; unsigned first; };
struct JpegIdctArgs { JpegIdctComp c[3]; int ncomp; unsigned total; };
int launch_jpeg_idct(hipStream_t stream, const JpegIdctArgs &A);
int jpeg_coefficients_host(const unsigned char *jpeg, size_t nbytes, int luma_only, unsigned char *out, size_t cap, int *h, int *w, int *ncomp,
                           int *grid6, size_t *need);
// jpeg_host.cpp / jpeg_huff_kernels.hip: the entropy decode on the device (tests/jpeg_huff_ref.py; the records are csrc/jpeg_huff_core.h's)
struct JpegScanHeader;
int jpeg_scan_host(const unsigned char *jpeg, size_t nbytes, int sub_bits, unsigned char *out, size_t cap, size_t *need);
size_t jpeg_huff_work_bytes(const JpegScanHeader &H, int max_rounds);
int jpeg_huff_decode_device(hipStream_t stream, hipEvent_t sync, const JpegScanHeader &H, const uint8_t *d_rec, uint8_t *d_work, uint32_t *h_flags,
                            int max_rounds, int luma_only, int16_t *d_coef, int *rounds_used, vfsms_ctx *prof);
// pyramid_kernels.hip: the reduced levels of a band of the canvas (Stitcher.outputPyramid), back to back in d_levels
size_t pyramid_band_bytes(int rows, int cols, int ch, int row0, int nrows, int levels);
int pyramid_band_device(vfsms_ctx *ctx, const CanvasRec *cv, int row0, int nrows, int levels, uint8_t *d_levels);
// the same with a place of its own for every level: level k's rows of the band at lvl[k] (any alignment), k = 1 .. levels; profile stage `stage`
int pyramid_band_device_at(vfsms_ctx *ctx, const CanvasRec *cv, int row0, int nrows, int levels, uint8_t *const *lvl, const char *stage);

// sift_kernels.hip
#define VFSMS_SIFT_MAX_LAYERS 8
#define VFSMS_SIFT_MAX_OCT 16
int sift_check_params(const vfsms_sift_params *p);
struct SiftSrcHost { const uint8_t *p; int stride; };
struct SiftStripOut { int n; int cand0; float *xy; float *desc; int8_t *d8; int *nrm; };   // n keypoints: positions, float descriptors, packed rows + norms (sift_pad_rows(n) rows)
static inline size_t sift_pad_rows(int n) { return ((size_t)n + 63) & ~(size_t)63; }
void sift_pool_reset(vfsms_ctx *ctx);
void *sift_pool_alloc(vfsms_ctx *ctx, size_t bytes);
struct SiftStripDev { float *pyr, *t0, *t1; int *counts; };     // one strip's block of ctx->sift_scratch
void sift_strip_layout(ArenaWalk &a, SiftStripDev *d, size_t pyr_floats, size_t max_plane, int nslots);
int sift_group_strips(vfsms_ctx *ctx, int h, int w, const vfsms_sift_params *p, int *g_out);
int sift_group_device(vfsms_ctx *ctx, const SiftSrcHost *srcs, int g, int h, int w, const vfsms_sift_params *p, int *counts,
                      SiftStripOut *out, const vfsms_keypoint **kp_tmp);
int sift_detect_describe_device(vfsms_ctx *ctx, const uint8_t *d_img, int h, int w, const vfsms_sift_params *p,
                                float *kps_xy, float *desc, vfsms_keypoint *kps_full, int cap, int *n_out);
int sift_pyramid_device(vfsms_ctx *ctx, const uint8_t *d_img, int h, int w, const vfsms_sift_params *p,
                        float *gauss, float *dog, size_t cap_floats, int32_t *shapes, int shapes_cap, int *n_oct);

// ---- runs (api.hip): n sources or jobs in fused launches, their device arrays one block of the arena ---------------------------------
struct SurfSrc { const uint8_t *p; int stride, h, w, cap; };      // pixels on the device, keypoint capacity of the source
struct SurfEnh { int mode; double clip_limit; int tile_grid; };   // equalizeHist / CLAHE before detection (mode 0: none)
struct SurfRun {
    std::vector<RoiDev> R; RoiDev *dR = nullptr;                  // host and device copies of the ROI records
    std::vector<EnhJob> E; EnhJob *dE = nullptr;
    int *cblock = nullptr;                                        // 16 counters per source, one contiguous block: one memset, one copy back
    std::vector<int> counters;
};
struct StripTable {                                               // the distinct strips of a fused batch (api.hip: build_strip_table)
    struct Strip { const uint8_t *p; int stride, h, w; };
    std::vector<Strip> strips;               // distinct strips in launch order
    std::vector<int> a, b;                   // per slot: its A / B strip
    int u0 = 0;                              // strips of part 0 (the first u0)
};
struct MatchPlan { bool filtered; int ns, cns; };    // filtered: MFMA candidate filter (cns train splits) + exact verification; else ns splits
struct MatchJob {
    const float *q, *t, *kq, *kt;                    // descriptors and keypoint positions of the query and the train set
    const int *nq_ptr, *nt_ptr;                      // their counts, on the device
    int capq, capt;                                  // what the job's arrays are sized for
    int row;                                         // the job's row of the result block
    const int8_t *q8, *t8; const int *qn2, *tn2;     // optional: int8 rows and their norms (k_bf_i8_d128)
    const StripTable::Strip *sa, *sb;                // optional: the raw pixels of the two strips, for the verifier behind the vote
    int pairs_given;                                 // the caller has filled the job's pairs[] (TAIL_GIVEN_PAIRS): the compaction leaves them alone
};
struct MatchRun { MatchPlan P; int dim; std::vector<MatchDev> M; MatchDev *dM = nullptr; int32_t *rblock = nullptr; };
struct OrbRun {
    std::vector<OrbDev> R; OrbDev *dR = nullptr;                  // host and device copies of the ROI records
    int *cblock = nullptr;                                        // 64 ints per source, one contiguous block
    std::vector<int> counters;
};
void surf_run_layout(ArenaWalk &a, SurfRun *run, const SurfSrc *S, int n, const vfsms_surf_params *p, const SurfEnh &enh);
void match_run_layout(ArenaWalk &a, MatchRun *run, const MatchJob *J, int n, int dim, const MatchPlan &P);
struct PhaseResolveDev { double *out3; PhasePeak *peaks; unsigned long long *sums; PhaseJobHost *jobs; };   // a phase_resolve group, ahead of phase_layout's scratch
void phase_resolve_layout(ArenaWalk &a, PhaseResolveDev *d, int nb, int K);
void orb_run_layout(ArenaWalk &a, OrbRun *run, const StripTable::Strip *S, int n, const vfsms_orb_params *p, int cap1, int cap2, int cap);

#ifdef __HIPCC__
// Speed only (placement is not a contract): workgroups are observed to land on XCD (linear block id % 8), each XCD with a private
// 4 MB L2.  Gather-heavy kernels whose slowest grid index is a unit with its own working set (an ROI and its 3.4 MB integral
// image; a (match job, train chunk) and its descriptors) hand every XCD WHOLE units, so that a unit's data is pulled into one L2
// once instead of into all eight.  L = linear block id, per_unit blocks per unit; the units beyond the last multiple of 8 keep
// the plain order.
__device__ __forceinline__ void xcd_roi_map(unsigned L, unsigned per_unit, unsigned nunits, unsigned &unit, unsigned &inner)
{
    const unsigned nfull = nunits & ~7u;
    if (L < per_unit * nfull) { const unsigned x = L & 7u, slot = L >> 3; unit = x + 8u * (slot / per_unit); inner = slot % per_unit; }
    else { unit = L / per_unit; inner = L % per_unit; }
}
#endif
