/*
 * vfsms.h -- C ABI of libvfsms.so, the MI355X (gfx950) engine for the VFSMS pairwise-alignment hot path.
 *
 * Plain C: opaque context pointer, plain pointers and sizes, int status codes.  No torch / numpy / C++
 * types cross this boundary.  Every entry point names the reference interface it replaces
 * (paths relative to the reference repository Keep-Passion/ImageStitch).
 *
 * The reference's own FFI for this path is the Boost.Python module `myGpuFeatures`
 * (appendix/myGpuFeatures.cpp:203-209: detectAndDescribeBySurf, detectAndDescribeByOrb, matchDescriptors),
 * selected by Method.isGPUAvailable (ImageUtility.py:254,265,285,304); the remaining arithmetic of the path
 * is reached through cv2 (SURF_create/detectAndCompute ImageUtility.py:258,262; DescriptorMatcher
 * ImageUtility.py:288-299; cv2.phaseCorrelate Stitcher.py:230) and numpy (ImageFusion.py:43-244).
 *
 * Conventions
 *   - return value: 0 = VFSMS_OK, negative = error (vfsms_last_error gives the message, thread-local).
 *   - the caller owns every host buffer and pre-allocates outputs with a capacity; the library never
 *     returns memory it owns and never frees caller memory.
 *   - all entry points are synchronous at return (host outputs are valid) unless stated otherwise;
 *     work is issued on the context's own HIP stream.
 *   - one context per thread/GPU; contexts share no mutable state.
 *   - "zero keypoints / zero matches" is NOT an error (n_out = 0).
 */
#ifndef VFSMS_H
#define VFSMS_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VFSMS_OK 0
#define VFSMS_ERR_BAD_ARG (-1)
#define VFSMS_ERR_CAPACITY (-2)   /* an output or internal capacity was exceeded            */
#define VFSMS_ERR_HIP (-3)        /* a HIP runtime call failed (message has hipGetErrorString) */
#define VFSMS_ERR_FFT (-4)        /* rocFFT plan / execution failure                           */
#define VFSMS_ERR_NO_DEVICE (-5)
#define VFSMS_ERR_UNSUPPORTED (-6)

typedef struct vfsms_ctx vfsms_ctx;

/* cv::KeyPoint fields SURF/ORB fill (the reference keeps only pt: ImageUtility.py:264) */
typedef struct {
    float x, y, size, angle, response;
    int32_t octave, class_id;
} vfsms_keypoint;

/* SURF parameters: cv2.xfeatures2d.SURF_create() defaults at ImageUtility.py:258 are
 * {100, 4, 3, extended 0, upright 0}; the DLL path passes Method.surf* (ImageUtility.py:23-28,272). */
typedef struct {
    float hessian_threshold;
    int32_t n_octaves;
    int32_t n_octave_layers;
    int32_t extended;     /* 0 -> 64-d, 1 -> 128-d */
    int32_t upright;
} vfsms_surf_params;

/* ORB parameters: cv2.ORB_create(nfeatures, scaleFactor, nlevels, edgeThreshold, firstLevel, WTA_K, scoreType, patchSize,
 * fastThreshold) as built at ImageUtility.py:260 from Method.orb* (ImageUtility.py:30-39): {5000, 1.2, 8, 31, 0, 2, 0, 31, 20}.
 * Supported: first_level 0, wta_k 2, score_type 0 (HARRIS), n_levels <= 8, patch_size <= 31.                                */
typedef struct {
    int32_t n_features;
    float scale_factor;
    int32_t n_levels, edge_threshold, first_level, wta_k, score_type, patch_size, fast_threshold;
} vfsms_orb_params;

/* SIFT parameters: cv2.xfeatures2d.SIFT_create() defaults (ImageUtility.py:256,268) are {0, 3, 0.04, 10, 1.6}.
 * Supported: n_features 0 (retainBest is not), n_octave_layers 1..8.                                                               */
typedef struct {
    int32_t n_features;
    int32_t n_octave_layers;
    double contrast_threshold, edge_threshold, sigma;
} vfsms_sift_params;

/* One ROI attempt of the incremental search (Stitcher.py:319-351): ROI rectangles inside two
 * device-resident tiles, as Method.getROIRegionForIncreMethod (ImageUtility.py:66-101) slices them. */
typedef struct {
    int64_t tile_a, tile_b;          /* handles from vfsms_tile_upload / vfsms_tile_wrap */
    int32_t ay0, ax0, by0, bx0;      /* top-left corner of each ROI inside its tile      */
    int32_t h, w;                    /* common ROI size                                   */
} vfsms_roi_pair;

/* result of one feature attempt: out[8] = {status, dx, dy, votes, nA, nB, nMatches, reserved}
 * (status, [dx,dy]) is exactly Method.getOffsetByMode's return (ImageUtility.py:139-178)
 * BEFORE the stitch-axis correction of Stitcher.py:352-360 (that stays on the host).          */
#define VFSMS_ATTEMPT_INTS 8

/* ---- library / context -------------------------------------------------------------------------- */
int vfsms_version(void);
int vfsms_device_count(void);
int vfsms_last_error(char *buf, int buflen);           /* copies the calling thread's last message */
int vfsms_ctx_create(int device, vfsms_ctx **out);
int vfsms_ctx_destroy(vfsms_ctx *ctx);
int vfsms_ctx_sync(vfsms_ctx *ctx);
/* wait for the asynchronous tile uploads only (vfsms_tile_upload_async): their host buffers may be reused afterwards             */
int vfsms_ctx_sync_uploads(vfsms_ctx *ctx);
/* The context's hipStream_t (as void*), so a host framework can record HIP events on it.          */
void *vfsms_ctx_stream(vfsms_ctx *ctx);
/* Max SURF candidates per ROI (default: h*w/24 + 4096).  0 restores the default.                  */
int vfsms_ctx_set_keypoint_capacity(vfsms_ctx *ctx, int cap);
/* How the fused paths turn matches into an offset (Method.offsetCaculate): VFSMS_OFFSET_MODE (the default, getOffsetByMode) or
 * VFSMS_OFFSET_CONSENSUS (vfsms_consensus_offset with tolerance tol_px, 0..VFSMS_CONSENSUS_MAX_TOL).  Governs vfsms_attempt_surf_batch,
 * _enhanced, vfsms_attempt_orb_batch, vfsms_attempt_sift_batch, vfsms_pairs_offsets, _blind, vfsms_features_match_offset and _batch; rows keep their layout.
 * vfsms_mode_offset always votes by mode.  Anything else returns VFSMS_ERR_BAD_ARG and leaves the setting as it was.                */
#define VFSMS_OFFSET_MODE 0
#define VFSMS_OFFSET_CONSENSUS 1
#define VFSMS_CONSENSUS_MAX_TOL 64
int vfsms_ctx_set_offset_estimator(vfsms_ctx *ctx, int estimator, int tol_px);
/* A second, optional acceptance criterion behind that vote (Method.offsetVerify; the reference has no such step, the specification is
 * tests/verify_ref.py): VFSMS_VERIFY_NONE (the default: nothing runs, rows as before) or VFSMS_VERIFY_NCC, the normalised
 * cross-correlation of the RAW pixels (also under isEnhance) the two ROI strips share under the voted (dx, dy): strip-B pixel (r, c) meets
 * strip-A pixel (r + dx, c + dy).  A row whose vote was accepted keeps status 1 iff score >= threshold (-1..1); fewer than min_pixels
 * (>= 0) shared pixels or a flat side score 0.  Int 7 of the row = floor(score * VFSMS_VERIFY_FIXED_ONE + 0.5), 0 for rows the vote
 * did not accept; dx, dy and the counts stay.  Governs vfsms_attempt_surf_batch, _enhanced, vfsms_attempt_orb_batch,
 * vfsms_attempt_sift_batch and methods 0 / 1 of vfsms_pairs_offsets, _blind (a rejected candidate is a failed attempt: the search goes
 * on).  Method 2 (phase) ignores it: it has its own response gate, or vfsms_ctx_set_phase_resolver's score.  vfsms_mode_offset and vfsms_consensus_offset never verify.
 * vfsms_features_match_offset and _batch carry no pixels: with the verifier on they return VFSMS_ERR_UNSUPPORTED.
 * Anything else returns VFSMS_ERR_BAD_ARG and leaves the setting as it was.                                                      */
#define VFSMS_VERIFY_NONE 0
#define VFSMS_VERIFY_NCC 1
#define VFSMS_VERIFY_FIXED_ONE 1048576
int vfsms_ctx_set_offset_verifier(vfsms_ctx *ctx, int verifier, double threshold, int min_pixels);
/* How method 2 (phase) of vfsms_pairs_offsets and _blind turns a correlation surface into an attempt row (Stitcher.phaseResolve; the
 * reference has no such step, the specification is tests/phase_resolve_ref.py): VFSMS_PHASE_RESOLVE_NONE (the default: the reference's
 * one arg-max, its sign and its response gate, rows as before) or VFSMS_PHASE_RESOLVE_NCC: the `peaks` (1..VFSMS_PHASE_MAX_PEAKS) largest
 * peaks of the unshifted surface, the four circular readings of each scored like vfsms_verify_ncc scores a vote, the best one kept; the
 * row is vfsms_attempt_phase_resolve_batch's, its dx, dy a raw vote in the feature path's convention (the axis correction applies as for
 * methods 0 and 1), status = score >= threshold (-1..1); fewer than min_pixels (>= 0) shared pixels score 0.  grid_params.phase_threshold
 * plays no part then.  Anything else returns VFSMS_ERR_BAD_ARG and leaves the setting as it was.                                        */
#define VFSMS_PHASE_RESOLVE_NONE 0
#define VFSMS_PHASE_RESOLVE_NCC 1
#define VFSMS_PHASE_MAX_PEAKS 8
int vfsms_ctx_set_phase_resolver(vfsms_ctx *ctx, int resolver, int peaks, double threshold, int min_pixels);

/* Per-stage timing with HIP events recorded on the context's own stream around each kernel group
 * ("integral", "hessian", "nms", "sort", "orientation", "describe", "bf_l2", "vote", "phase", "fuse", ...).
 * read: comma-separated stage names, accumulated milliseconds and launch-group counts; reset != 0 clears. */
int vfsms_profile_enable(vfsms_ctx *ctx, int on);
int vfsms_profile_read(vfsms_ctx *ctx, char *names, int names_len, double *ms, int64_t *calls, int cap,
                       int *n_out, int reset);

/* ---- device-resident tiles (grayscale u8, row stride in bytes) ----------------------------------- */
int vfsms_tile_upload(vfsms_ctx *ctx, const uint8_t *img, int h, int w, int stride, int64_t *handle);
/* the same without waiting for the copy: it runs on the context's copy stream, overlapped with whatever the compute stream is doing,
 * and the first batch / canvas call that names the tile orders itself behind it (the decode loop of Stitcher.py:68-69 feeding the
 * GPU while earlier pairs are being registered).  img must stay valid and unchanged until vfsms_ctx_sync or the first synchronous
 * call that used the tile has returned; copies from pinned memory (vfsms_host_alloc) run at PCIe rate and truly overlap.          */
int vfsms_tile_upload_async(vfsms_ctx *ctx, const uint8_t *img, int h, int w, int stride, int64_t *handle);
/* an interleaved colour tile (ch = 3: the isColorMode = True default of Main.py, Stitcher.py:174-179) for the mosaic canvas only:
 * rows of w * ch bytes, stride_bytes between rows, synchronous or (async != 0) on the copy stream like vfsms_tile_upload_async.
 * Registration entry points reject tiles with ch != 1.                                                                          */
int vfsms_tile_upload_ch(vfsms_ctx *ctx, const uint8_t *img, int h, int w, int ch, int stride_bytes, int async, int64_t *handle);
/* Ingest pipeline (replaces the decode loop of Stitcher.py:68-69, which reads every file before the first pair is registered):
 * vfsms_tile_reserve hands out the handle of an h x w gray tile whose pixels arrive later; vfsms_tile_fill -- callable from ANY
 * thread, concurrently with a batch call on the context's thread -- copies them (it returns when the copy has landed, so the
 * decoder's staging buffer is free again; img == NULL reports a failed decode).  A batch / canvas call that names a reserved tile
 * waits for exactly that tile, so vfsms_pairs_offsets works on tiles 0, 1, ... while tile k is still being decoded.               */
int vfsms_tile_reserve(vfsms_ctx *ctx, int h, int w, int64_t *handle);
int vfsms_tile_fill(vfsms_ctx *ctx, int64_t handle, const uint8_t *img, int stride);
/* the same for an interleaved tile of ch channels (the mosaic's colour tiles); vfsms_tile_fill takes its rows of w * ch bytes, `stride` in bytes */
int vfsms_tile_reserve_ch(vfsms_ctx *ctx, int h, int w, int ch, int64_t *handle);
/* ONE decode per file for both uses the reference makes of it: cv2.imdecode(..., 0) feeds the registration loop (Stitcher.py:68-69) and,
 * with isColorMode (Main.py:14's default), cv2.imdecode(..., IMREAD_COLOR) feeds the mosaic (Stitcher.py:382-403).  Both are views of the
 * same entropy decode: IMREAD_GRAYSCALE of a JPEG is its Y plane, IMREAD_COLOR is libjpeg's fixed-point YCbCr -> RGB (jdcolor.c) of the
 * same planes, stored B G R.  `src` holds what the decoder produced once --
 *   VFSMS_SRC_GRAY8   one byte per pixel (a grayscale file; the colour tile replicates it, as IMREAD_COLOR does)
 *   VFSMS_SRC_YCC24   Y Cb Cr interleaved (libjpeg out_color_space = JCS_YCbCr: no colour conversion on the host)
 *   VFSMS_SRC_YCCX32  Y Cb Cr X, four bytes per pixel (Pillow's pixel storage, handed over without a repack)
 * -- and the device writes the reserved gray tile `gray` and the reserved 3-channel tile `color` (either may be 0).  Any thread; returns
 * when both tiles are complete; src == NULL gives both up (a failed decode).                                                              */
#define VFSMS_SRC_GRAY8 0
#define VFSMS_SRC_YCC24 1
#define VFSMS_SRC_YCCX32 2
int vfsms_tile_fill_pair(vfsms_ctx *ctx, int64_t gray, int64_t color, const uint8_t *src, int stride_bytes, int format);
/* The decode itself, for JPEG files (what cv2.imread / cv2.imdecode do on the reference's host: Stitcher.py:68-69, 382-403): the FILE'S
 * BYTES in, both tiles out.  The system's libjpeg-turbo (libjpeg.so.8, loaded at first use) decodes straight into the library's pinned
 * staging memory -- the Y plane alone when only `gray` is given (IMREAD_GRAYSCALE); when `color` is given, the DOWNSAMPLED Y Cb Cr planes of
 * a 4:2:0 file (round 6: libjpeg's h2v2 fancy upsampling and jdcolor.c's conversion both run on the device, k_ingest_420;
 * VFSMS_JPEG_RAW420=0 restores the host's upsampling), the upsampled planes of any other sampling -- and the device finishes as in
 * vfsms_tile_fill_pair.  Any thread; returns when both tiles are complete.  VFSMS_ERR_UNSUPPORTED (no
 * libjpeg.so.8 on this host; not a 1- or 3-component YCbCr / gray JPEG) and VFSMS_ERR_BAD_ARG (a damaged file; a file that is not the
 * size of the reserved tiles) leave BOTH TILES RESERVED: decode some other way and fill them, or give them up.                          */
int vfsms_tile_fill_jpeg(vfsms_ctx *ctx, int64_t gray, int64_t color, const uint8_t *jpeg, size_t nbytes);
/* the same decode into the caller's memory, no context and no GPU: rows of *w * *comp bytes, comp = 3 (Y Cb Cr interleaved) when
 * want_planes != 0 and the file has three components, else 1 (the grayscale decode).  VFSMS_ERR_CAPACITY (with *h, *w, *comp set) when
 * `cap` bytes are too few -- call with out == NULL to ask for the size.  want_planes == 2 (round 6): the DOWNSAMPLED planes of a 4:2:0
 * Y Cb Cr file as jpeg_read_raw_data hands them out (*comp = 420): Y with pitch pw = *w rounded up to 16 and ph = *h rounded up to 16 rows,
 * then Cb and Cr (pitch pw / 2, ph / 2 rows) -- pw * ph * 3 / 2 bytes; what vfsms_tile_fill_jpeg stages when the device does the chroma
 * upsampling (VFSMS_ERR_UNSUPPORTED for any other sampling).                                                                            */
int vfsms_jpeg_decode(const uint8_t *jpeg, size_t nbytes, int want_planes, uint8_t *out, size_t cap, int *h, int *w, int *comp);
/* Method.jpegDecoder = "device" (csrc/jpeg_dec_kernels.hip; specified by tests/jpeg_dec_ref.py): the host stops behind the ENTROPY decode and
 * the device does the rest of libjpeg's default decoder -- dequantisation, the integer inverse DCT of jidctint.c (JDCT_ISLOW), + 128, the clamp
 * to 0..255 -- then, for a colour tile, what vfsms_tile_fill_jpeg's device half does already (k_ingest_420 / the gray replication).  Same
 * bytes in both tiles as vfsms_tile_fill_jpeg, same contract, same return codes: any thread, returns when both tiles are complete, and
 * VFSMS_ERR_UNSUPPORTED / VFSMS_ERR_BAD_ARG leave BOTH TILES RESERVED.  Taken: 8-bit Huffman files, baseline or progressive, of one component
 * or of three (Y Cb Cr) sampled 2x2, 1x1, 1x1 with width >= 5 and height >= 2; anything else is VFSMS_ERR_UNSUPPORTED (vfsms_tile_fill_jpeg
 * takes it), a damaged file -- any decoder warning -- VFSMS_ERR_BAD_ARG.
 * The staging layout (vfsms_jpeg_coefficients writes it, host only: no context, no GPU): first one quantisation table per component,
 * uint16[64] in NATURAL (row-major) order, VFSMS_JPEG_COEF_TABLE_BYTES each; then per component its blocks in block-row-major order, each
 * block 64 int16 in natural order.  A component sampled hs x vs in a frame whose maxima are hmax x vmax has
 *     grid6[2 k]     = ceil(h * vs / (vmax * 8)) rounded up to a multiple of vs     block rows
 *     grid6[2 k + 1] = ceil(w * hs / (hmax * 8)) rounded up to a multiple of hs     block columns
 * -- whole iMCUs: the luma grid of a 4:2:0 file covers exactly the pw x ph plane of the raw 4:2:0 layout below, the chroma grids its pw / 2 x
 * ph / 2 planes.  *need = the bytes of the layout, also on VFSMS_ERR_CAPACITY (*h, *w, *ncomp, grid6 are set then too): call with out ==
 * NULL to ask for the size.
 * vfsms_jpeg_idct: the bare operator.  block_rows x block_cols blocks and ONE table in, host arrays; the plane out, block_rows * 8 rows of
 * block_cols * 8 bytes, `pitch` bytes apart.  Exact while every intermediate of both passes fits int32 and every column-pass output int16
 * (any coefficients a file holds are far inside; beyond, libjpeg's own C and SIMD transforms part ways).  Profile stage "jpeg_decode".    */
#define VFSMS_JPEG_COEF_TABLE_BYTES 128
int vfsms_tile_fill_jpeg_dct(vfsms_ctx *ctx, int64_t gray, int64_t color, const uint8_t *jpeg, size_t nbytes);
int vfsms_jpeg_coefficients(const uint8_t *jpeg, size_t nbytes, uint8_t *out, size_t cap, int *h, int *w, int *ncomp, int *grid6, size_t *need);
int vfsms_jpeg_idct(vfsms_ctx *ctx, const int16_t *coef, const uint16_t *quant, int block_rows, int block_cols, uint8_t *out, int pitch);
/* Method.jpegDecoder = "device-entropy" (csrc/jpeg_huff_kernels.hip, csrc/jpeg_huff_core.h; specified by tests/jpeg_huff_ref.py): the ENTROPY
 * decode runs on the device too.  The host reads the file once for its markers and nothing but the compressed bytes cross the link; Huffman
 * decode, DC prediction, then everything vfsms_tile_fill_jpeg_dct does on the device.  No libjpeg is involved.
 * Taken: 8-bit Huffman baseline / extended sequential files (SOF0, SOF1) with ONE scan holding every component, of one component or of three
 * (Y Cb Cr) sampled 2x2, 1x1, 1x1 with width >= 5 and height >= 2, every table defined in front of the scan.  VFSMS_ERR_UNSUPPORTED: anything
 * else -- progressive, arithmetic, 12-bit, several scans, other samplings, CMYK, a table or a scan behind SOS -- and a file whose parallel
 * decoders are not in step after the repair rounds allowed.  VFSMS_ERR_BAD_ARG: a damaged file -- broken markers, restart intervals that do
 * not add up to the frame, no EOI, and in the true sequential decode an undefined code, a coefficient beyond index 63 or bits exhausted in
 * front of the blocks.
 * vfsms_jpeg_scan (host only: no context, no GPU, no libjpeg): the scan record, in one pass over the file.  It opens with 22 int32 / uint32
 * (JpegScanHeader, csrc/jpeg_huff_core.h): h, w, ncomp, grid6[6] (as vfsms_jpeg_coefficients), restart interval, segments, subsequences, MCUs,
 * blocks per MCU, subsequence bits, stream bytes, then the byte offsets in the record of: the quantisation tables (uint16[64] natural order per
 * component), the Huffman tables (per component DC then AC, JpegHuffTable: a 9-bit look-up, maxcode / value offsets per length, the
 * symbols, the DHT counts[16]), the unstuffed stream, the segment table (uint32 x 4: byte offset in the stream -- a multiple of 4, the segment
 * padded with FF to one --, byte count, first MCU, first subsequence), the segment of every subsequence (uint32), and the record's size.
 * *need: with VFSMS_OK the bytes written; with VFSMS_ERR_CAPACITY (out == NULL asks) a bound on them.
 * The stream of a segment is cut into subsequences of VFSMS_JPEG_HUFF_SUB_BITS bits, one thread each; a thread that did not start at a code
 * boundary falls in step with the true decode after a while, and repair rounds carry the true states forward until nothing changes (at most
 * subsequences - 1 rounds; VFSMS_JPEG_HUFF_MAX_ROUNDS in the fill path: dense noise at quality 100 is practically sequential and goes back).
 * vfsms_jpeg_entropy_decode: the bare operator.  File bytes in, the layout of vfsms_jpeg_coefficients out to a host array, byte for byte
 * (*need, *h, *w, *ncomp, grid6 as there; out == NULL asks).  max_rounds: repair rounds allowed, -1 = the subsequence count.  *rounds_used:
 * the rounds that changed something.  Profile stage "jpeg_entropy" (and jpeg_entropy_sync / _rounds / _scan / _write inside it).
 * vfsms_tile_fill_jpeg_huff: vfsms_tile_fill_jpeg_dct's contract, thread rules, pools, stream ordering and return codes; on any refusal BOTH
 * TILES STAY RESERVED and nothing was written to them.                                                                                   */
#ifndef VFSMS_JPEG_HUFF_SUB_BITS      /* (a build with another size: tools/bench_jpeg_decode.py --sweep) */
#define VFSMS_JPEG_HUFF_SUB_BITS 1024
#endif
#define VFSMS_JPEG_HUFF_MAX_ROUNDS 48
int vfsms_jpeg_scan(const uint8_t *jpeg, size_t nbytes, uint8_t *out, size_t cap, size_t *need);
int vfsms_jpeg_entropy_decode(vfsms_ctx *ctx, const uint8_t *jpeg, size_t nbytes, int max_rounds, uint8_t *out, size_t cap, int *h, int *w, int *ncomp,
                              int *grid6, size_t *need, int *rounds_used);
int vfsms_tile_fill_jpeg_huff(vfsms_ctx *ctx, int64_t gray, int64_t color, const uint8_t *jpeg, size_t nbytes);
/* The way out, for the mosaic: replaces cv2.imwrite(path, result) for .jpg results (Stitcher.py:149, 175-179; Main.py:21-51 writes every
 * result as jpg).  vfsms_jpeg_encode: n_rows x cols pixels of 1 or 3 channels (R G B, or B G R -- the canvas order -- with bgr != 0), rows
 * `stride_bytes` apart -> a complete baseline JPEG stream with cv2.imwrite's settings (libjpeg defaults, `quality`: 95).  No context, no GPU,
 * any thread.  *nbytes = the stream's size, also on VFSMS_ERR_CAPACITY.  A horizontal STRIPE of an image encodes independently of the
 * others when its height is a multiple of the MCU height (16 rows for colour, 8 for gray), so a host encodes the stripes of a mosaic on all
 * its cores -- while the bands are still leaving the device -- and vfsms_jpeg_join makes ONE file of them: the headers of stripe 0 with the
 * full height, a DRI segment (restart interval = the MCUs of a stripe, <= 65535) and the stripes' entropy-coded segments separated by RSTn
 * markers.  Same DCT coefficients, hence the same decoded pixels, as the one-thread encode of the whole image.  out == NULL: size only.   */
int vfsms_jpeg_encode(const uint8_t *rows, int n_rows, int cols, int channels, int stride_bytes, int bgr, int quality,
                      uint8_t *out, size_t cap, size_t *nbytes);
int vfsms_jpeg_join(const uint8_t *const *streams, const size_t *sizes, int n_stripes, int stripe_rows, int total_rows,
                    uint8_t *out, size_t cap, size_t *nbytes);
/* The encoder on the device (Method.jpegEncoder = "device"; csrc/jpeg_enc_kernels.hip).  Its bytes are those of tests/jpeg_enc_ref.py --
 * libjpeg's baseline encoder with jpeg_set_defaults + jpeg_set_quality(quality, force_baseline), byte for byte libjpeg's file when the image
 * is one restart interval -- with a restart interval of `restart_mcus` MCUs (16 x 16 pixels for 3 channels, 4:2:0; 8 x 8 for 1).  One rule
 * for every entry: an interval holds at most 65535 MCUs, and restart_mcus = 0 means "the image is one interval", so it is refused for an
 * image of more MCUs than that.  VFSMS_ERR_BAD_ARG for that, for restart_mcus > 65535, a side beyond 65500, channels other than 1 and 3.
 * vfsms_jpeg_header (host only, no context): SOI .. the SOS header in libjpeg's layout; *nbytes = the size, also on VFSMS_ERR_CAPACITY.
 * vfsms_jpeg_encode_device: an image on the host (B G R with bgr != 0, else R G B) -> a complete file; *nbytes likewise.                  */
int vfsms_jpeg_header(int rows, int cols, int ch, int quality, int restart_mcus, uint8_t *out, size_t cap, size_t *nbytes);
int vfsms_jpeg_encode_device(vfsms_ctx *ctx, const uint8_t *img, int h, int w, int ch, int stride, int bgr, int quality, int restart_mcus,
                             uint8_t *out, size_t cap, size_t *nbytes);
/* pinned host staging memory for tiles (decoders write into it; uploads from it are asynchronous DMA)                          */
int vfsms_host_alloc(vfsms_ctx *ctx, size_t bytes, void **ptr);
int vfsms_host_free(vfsms_ctx *ctx, void *ptr);
/* adopt memory already on this device (e.g. a framework tensor); not freed by vfsms_tile_free     */
int vfsms_tile_wrap(vfsms_ctx *ctx, const void *device_ptr, int h, int w, int stride, int64_t *handle);
int vfsms_tile_free(vfsms_ctx *ctx, int64_t handle);

/* ---- per-operator entry points, host buffers in / out -------------------------------------------- */
/* cv::integral(CV_8U -> CV_32S) as SURF uses it; sum_out is (h+1) x (w+1) int32                   */
int vfsms_integral_u8_i32(vfsms_ctx *ctx, const uint8_t *img, int h, int w, int stride, int32_t *sum_out);

/* replaces myGpuFeatures.detectAndDescribeBySurf (appendix/myGpuFeatures.cpp:67-104) and
 * cv2 SURF detectAndCompute (ImageUtility.py:258,262).  kps_xy: float32[cap][2] = (x, y);
 * desc: float32[cap][64|128]; kps_full optional (may be NULL).                                    */
int vfsms_surf_detect_describe(vfsms_ctx *ctx, const uint8_t *img, int h, int w, int stride,
                               const vfsms_surf_params *params,
                               float *kps_xy, float *desc, vfsms_keypoint *kps_full,
                               int cap, int *n_out);
/* detector only (sorted keypoints before orientation/deletion); for staged parity checks          */
int vfsms_surf_detect(vfsms_ctx *ctx, const uint8_t *img, int h, int w, int stride,
                      const vfsms_surf_params *params, vfsms_keypoint *kps_full, int cap, int *n_out);

/* replaces myGpuFeatures.detectAndDescribeByOrb (appendix/myGpuFeatures.cpp:106-146) and cv2 ORB detectAndCompute
 * (ImageUtility.py:260,262).  kps_xy: float32[cap][2]; desc: uint8[cap][32]; kps_full optional.                   */
int vfsms_orb_detect_describe(vfsms_ctx *ctx, const uint8_t *img, int h, int w, int stride,
                              const vfsms_orb_params *params,
                              float *kps_xy, uint8_t *desc, vfsms_keypoint *kps_full, int cap, int *n_out);

/* cv2 SIFT detectAndCompute (ImageUtility.py:256,262) as specified by tests/sift_ref.py (OpenCV 3.3.1's SIFT_Impl arithmetic in a fixed
 * evaluation order; no byte parity with cv2 is claimed).  kps_xy: float32[cap][2]; desc: float32[cap][128] of u8 values; kps_full
 * optional (class_id -1).  Keypoints in detection order (octave, layer, row, column, peak bin), duplicates removed (first kept).       */
int vfsms_sift_detect_describe(vfsms_ctx *ctx, const uint8_t *img, int h, int w, int stride, const vfsms_sift_params *params,
                               float *kps_xy, float *desc, vfsms_keypoint *kps_full, int cap, int *n_out);
/* the Gaussian and DoG pyramids of the same call, for staged parity checks.  shapes: int32[shapes_cap][2] = (rows, cols) of each octave;
 * gauss: octave after octave, n_octave_layers + 3 levels of rows x cols floats each; dog likewise with n_octave_layers + 2 levels.
 * gauss == dog == NULL: only *n_octaves and shapes are filled.  cap_floats bounds gauss (dog needs fewer).                           */
int vfsms_sift_pyramid(vfsms_ctx *ctx, const uint8_t *img, int h, int w, int stride, const vfsms_sift_params *params,
                       float *gauss, float *dog, size_t cap_floats, int32_t *shapes, int shapes_cap, int *n_octaves);

/* replaces myGpuFeatures.matchDescriptors(featureType 1|2, param=ratio) (appendix/myGpuFeatures.cpp:160-173)
 * and BFMatcher("BruteForce").knnMatch(k=2) + ratio filter (ImageUtility.py:288-296).
 * pairs: int32[cap][2] = (trainIdx, queryIdx) in query order.
 * Results are those of the reference's float arithmetic (4-wide accumulation of (a-b)^2, sqrt-domain compares, ties to the
 * lower train index) for every input.  64-d inputs whose rows all have norm <= 1 (SURF descriptors are L2-normalised; checked
 * on the device) are searched with the fp16 MFMA candidate filter + exact verification, anything else with the exhaustive
 * kernel; VFSMS_BF_EXACT=1 in the environment forces the exhaustive kernel.                                                  */
int vfsms_bf_l2_knn2_ratio(vfsms_ctx *ctx, const float *q, int nq, const float *t, int nt, int dim,
                           double ratio, int32_t *pairs, int cap, int *m_out);
/* raw 2-NN (for parity checks): idx1/d1 best, d2 second-best distance (+inf if nt < 2)            */
int vfsms_bf_l2_knn2(vfsms_ctx *ctx, const float *q, int nq, const float *t, int nt, int dim,
                     int32_t *idx1, float *d1, float *d2);
/* the same three arrays from the integer matrix-core search of the fused SIFT batch (vfsms_attempt_sift_batch), for parity checks and
 * diagnosis: 128-d rows whose elements are integers 0..255 (checked on the host: anything else is VFSMS_ERR_BAD_ARG), packed and searched
 * exactly as the batch does.  nsplit 1..8: that many train splits; 0: the batch's own rule for one job.  VFSMS_BF_EXACT does not apply. */
int vfsms_bf_l2_knn2_u8d128(vfsms_ctx *ctx, const float *q, int nq, const float *t, int nt, int nsplit,
                            int32_t *idx1, float *d1, float *d2);
/* replaces matchDescriptors(featureType 3, param=orbMaxDistance) (appendix/myGpuFeatures.cpp:175-187)
 * and BFMatcher("BruteForce-Hamming").match (ImageUtility.py:297-302).  max_dist < 0: no threshold. */
int vfsms_bf_hamming_nn(vfsms_ctx *ctx, const uint8_t *q, int nq, const uint8_t *t, int nt, int nbytes,
                        int max_dist, int32_t *pairs, int cap, int *m_out);

/* Method.getOffsetByMode (ImageUtility.py:139-178).  kps: float32[n][2]=(x,y); out4={status,dx,dy,votes} */
int vfsms_mode_offset(vfsms_ctx *ctx, const float *kpsA, int nA, const float *kpsB, int nB,
                      const int32_t *pairs, int m, int offset_evaluate, int32_t *out4);
/* Method.getOffsetByRansac (offsetCaculate = "ransac"), specified by tests/consensus_ref.py: the votes of vfsms_mode_offset, the
 * support of each = the votes within a Chebyshev window of tol_px (0..VFSMS_CONSENSUS_MAX_TOL) around it, the first vote of largest
 * support wins, offset = the lower median of its inliers per axis.  out4={status,dx,dy,support}; tol_px = 0 is vfsms_mode_offset. */
int vfsms_consensus_offset(vfsms_ctx *ctx, const float *kpsA, int nA, const float *kpsB, int nB,
                           const int32_t *pairs, int m, int tol_px, int offset_evaluate, int32_t *out4);

/* The check of vfsms_ctx_set_offset_verifier on two host strips of h x w (u8, row strides in bytes) and a raw vote (dx, dy):
 * out8 = {N, Sa, Sb, Saa, Sbb, Sab, the bits of the double score, floor(score * VFSMS_VERIFY_FIXED_ONE + 0.5)} over the N shared pixels
 * (a = the strip-A pixel, b = its strip-B partner).  The caller compares the score with its threshold (Method.verifyOffset).       */
int vfsms_verify_ncc(vfsms_ctx *ctx, const uint8_t *a, int a_stride, const uint8_t *b, int b_stride, int h, int w,
                     int dx, int dy, int min_pixels, int64_t *out8);

/* The same statistic SEARCHED over a window of offsets, for n pairs of resident single-channel tiles (Method.globalAdjust = "ncc"; no
 * reference counterpart, the specification is tests/ncc_search_ref.py and the device equals it bit for bit).  A job names two whole tiles
 * of ONE shape and a predicted offset: tile B's pixel (r, c) meets tile A's pixel (r + dx, c + dy) -- for consecutive tiles of a path
 * exactly the entry of offsetList.  Every candidate (dx + i, dy + j), i, j in [-radius, radius], is scored as vfsms_verify_ncc scores
 * one; an empty overlap or fewer than min_pixels (>= 0) shared pixels score 0.  best4: int32[n][4] = {i, j, floor(score *
 * VFSMS_VERIFY_FIXED_ONE + 0.5), shared pixels} of the candidate with the largest double score, ties to the smallest i * i + j * j, then
 * the smallest i, then the smallest j (a flat pair gives (0, 0)); surface (may be NULL): int32[n][2 radius + 1][2 radius + 1], the
 * fixed-point score of candidate (i, j) at [i + radius][j + radius].  One launch sequence for all jobs.  VFSMS_ERR_BAD_ARG: tiles of
 * different shapes in a job, a colour tile, an unknown handle, a radius outside 1..16.                                              */
typedef struct { int64_t tile_a, tile_b; int32_t dx, dy; } vfsms_ncc_job;
int vfsms_ncc_search_batch(vfsms_ctx *ctx, const vfsms_ncc_job *jobs, int n, int radius, int min_pixels,
                           int32_t *best4, int32_t *surface);

/* The same search over a WIDE window in two levels (Method.failedPairRepair = "stage"; no reference counterpart, the specification is
 * tests/ncc_wide_ref.py and the device equals it bit for bit).  Jobs as above.  Both tiles are reduced by factor x factor block means
 * (factor 2, 4 or 8; A's blocks start at (dx mod factor, dy mod factor) so that the blocks of the two tiles meet exactly), the reduced
 * pair is searched with radius ceil(radius / factor) (<= 16) and max(1, min_pixels / factor^2); the `peaks` (1..4) best candidates of
 * that surface that are no neighbours of each other (Chebyshev distance > 1; order: score, i * i + j * j, i, j) seed one full-resolution
 * search of radius min(factor, radius) each, centred on factor x the seed, clamped so that the window stays inside [-radius, radius].
 * out8: int32[n][8] = {ti, tj, fixed-point score, shared pixels of the winner, ci, cj, coarse fixed-point score of the winning seed,
 * seeds used}: the offset found is (dx + ti, dy + tj); the winner has the largest fixed-point score, ties to the smallest ti * ti +
 * tj * tj, ti, tj.  seeds (may be NULL): int32[n][VFSMS_WIDE_MAX_PEAKS][6] = {ci, cj, coarse score, ti, tj, fine score} per seed, zeros
 * in unused rows.  reduced (may be NULL; a test hook, n == 1 only): the two reduced planes, A's then B's, hc x wc bytes each, hc =
 * (h - dx mod factor) / factor, wc = (w - dy mod factor) / factor.  One launch sequence for all jobs.  VFSMS_ERR_BAD_ARG, with the
 * outputs untouched: radius outside 1..VFSMS_WIDE_MAX_RADIUS, another factor, ceil(radius / factor) > 16, peaks outside
 * 1..VFSMS_WIDE_MAX_PEAKS, a colour tile, two shapes in one job, an unknown handle, hc or wc below 1.                               */
#define VFSMS_WIDE_MAX_RADIUS 128
#define VFSMS_WIDE_MAX_PEAKS 4
int vfsms_ncc_wide_batch(vfsms_ctx *ctx, const vfsms_ncc_job *jobs, int n, int radius, int factor, int peaks, int min_pixels,
                         int32_t *out8, int32_t *seeds, uint8_t *reduced);
/* The six integers of vfsms_verify_ncc at each job's own offset, for n pairs of resident single-channel tiles of one shape per job
 * (tests/verify_ref.py: sums): out6 = int64[n][6] = {N, Sa, Sb, Saa, Sbb, Sab}; an empty overlap gives zeros.                       */
int vfsms_overlap_sums_batch(vfsms_ctx *ctx, const vfsms_ncc_job *jobs, int n, int64_t *out6);

/* cv2.phaseCorrelate(np.float64(a), np.float64(b)) (Stitcher.py:230): out3 = {x, y, response}     */
int vfsms_phase_correlate_u8(vfsms_ctx *ctx, const uint8_t *a, const uint8_t *b, int h, int w,
                             int stride_a, int stride_b, double *out3);
/* How a strip of h x w is correlated (no reference counterpart: what bench.py / the tests report about the path that ran).
 * info8 = {1 = the transforms run in LDS (csrc/phase_kernels.hip) | 0 = rocFFT plans, 1 = correlated as its byte transpose,
 *          column length M, row length N (the padded sizes in the orientation used), columns per workgroup, rows per workgroup,
 *          threads of a row workgroup, threads of a column workgroup}; no device work                                           */
int vfsms_phase_plan(int h, int w, int32_t *info8);
/* vfsms_attempt_phase_resolve_batch (below) for two host strips: row8 = one attempt row, cands (may be NULL) int32[4 * peaks][4],
 * peaks_out (may be NULL) int32[peaks][2]                                                                                           */
int vfsms_phase_resolve_u8(vfsms_ctx *ctx, const uint8_t *a, const uint8_t *b, int h, int w, int stride_a, int stride_b,
                           int peaks, double threshold, int min_pixels, int32_t *row8, int32_t *cands, int32_t *peaks_out);

/* ImageFusion.fuseByFadeInAndFadeOut([A,B],dx,dy) (ImageFusion.py:192-244) on the reference's own
 * representation: int64 [r][c][ch] with -1 = empty (Stitcher.py:434-436).  out: uint8 [r][c][ch].
 * ch 1..4.  A pixel is empty iff every channel is -1: the sum of its channels is -ch (the reference's BGR test "sum != -3" at ch = 3);
 * every int64 operator below judges pixels by this rule, as the canvas path's validity plane does.
 * info (optional, 4 ints) = {mode 0 strip / 1 corner, corner index, rowIndex, colIndex}.           */
int vfsms_fuse_fade_i64(vfsms_ctx *ctx, const int64_t *A, const int64_t *B, int r, int c, int ch,
                        int dx, int dy, uint8_t *out, int32_t *info);
/* ImageFusion.fuseByTrigonometric([A,B],dx,dy) (ImageFusion.py:246-293), same representation and geometry decisions, weights
 * sin(w pi / 2)^2 of the float64 strip ramps / of getWeightsMatrix's float32 matrix.  The bytes hang on numpy's own sin in the
 * last ulp (where A == B the truncated result sits on an integer): equal to the reference on > 99.9 % of the bytes, |diff| <= 1.  */
int vfsms_fuse_trig_i64(vfsms_ctx *ctx, const int64_t *A, const int64_t *B, int r, int c, int ch,
                        int dx, int dy, uint8_t *out, int32_t *info);

/* multiBandBlending([A,B],dx,dy) with `levels` (1..8, the reference's default 4) pyramid levels, same representation: a hard seam
 * where the fade's weights tie (wA >= wB -> A), holes of A filled from B, then a Laplacian-pyramid blend in float32 and
 * uint8(clamp(rint(.))).  The arithmetic is this library's own specification (tests/multiband_ref.py), not a cv2 restatement.
 * info (optional, 4 ints) and the degenerate corner geometries that fail: as vfsms_fuse_fade_i64.                              */
int vfsms_fuse_multiband_i64(vfsms_ctx *ctx, const int64_t *A, const int64_t *B, int r, int c, int ch,
                             int dx, int dy, int levels, uint8_t *out, int32_t *info);

/* optimalSeamLine([A,B],dx,dy), same representation: the overlap is cut along a minimum-cost connected seam (an integer energy of the
 * difference A' - B' and its central differences, dynamic programming with lowest-index tie-breaks) inside the fade's geometry: one
 * seam across a strip, a horizontal and a vertical seam inside the corner ramps' arms in corner mode.  blend 0: every output pixel is a
 * pixel of one input; blend 1: the label plane replaces the fade-tie mask of the multi-band blend with `levels` (1..8) levels.
 * seam_out (optional, r + c ints): the vertical seam's column per row, then the horizontal seam's row per column, -1 where that seam
 * does not exist.  The arithmetic is this library's own specification (tests/seam_ref.py), not a restatement of the reference's
 * interactive ImageFusion.fuseByOptimalSeamLine.  info and the degenerate corner geometries that fail: as vfsms_fuse_fade_i64 (then
 * info[0] = -1, out is zero, seam_out is -1).                                                                                        */
int vfsms_fuse_seam_i64(vfsms_ctx *ctx, const int64_t *A, const int64_t *B, int r, int c, int ch,
                        int dx, int dy, int blend, int levels, uint8_t *out, int32_t *info, int32_t *seam_out);

/* The separable float32 ramps behind that blend, without blending: ramps = [wA_r(r) | wB_r(r) | wA_c(c) | wB_c(c)].
 * force_corner != 0 -> ImageFusion.getWeightsMatrix (ImageFusion.py:43-190): weightMatB = wB_r x wB_c,
 * weightMatA = 1 - weightMatB.  Otherwise the mode fuseByFadeInAndFadeOut itself would pick (info[0]).   */
int vfsms_fuse_ramps_i64(vfsms_ctx *ctx, const int64_t *A, int r, int c, int ch, int dx, int dy,
                         int force_corner, float *ramps, int32_t *info);

/* ---- fused, device-resident fast path ------------------------------------------------------------- */
/* n independent SURF + BF-L2 + ratio + mode-vote attempts in one batch (one launch sequence for all):
 * the body of the while-loop at Stitcher.py:322-343 for n (pair, direction, i) candidates.
 * out: int32[n][VFSMS_ATTEMPT_INTS].                                                               */
int vfsms_attempt_surf_batch(vfsms_ctx *ctx, const vfsms_roi_pair *jobs, int n,
                             const vfsms_surf_params *params, double ratio, int offset_evaluate,
                             int32_t *out);
/* the same with the reference's pre-enhancement of every ROI strip (Method.isEnhance, Stitcher.py:327-334):
 * enhance_mode 1 = cv2.equalizeHist, 2 = cv2.createCLAHE(clip_limit, (tile_grid, tile_grid)).apply, 0 = none; with mode 2 a
 * tile_grid outside 1..64 is VFSMS_ERR_BAD_ARG from every entry point that takes the three (modes 0 and 1 ignore it)            */
int vfsms_attempt_surf_batch_enhanced(vfsms_ctx *ctx, const vfsms_roi_pair *jobs, int n, const vfsms_surf_params *params,
                                      double ratio, int offset_evaluate, int enhance_mode, double clip_limit, int tile_grid,
                                      int32_t *out);
/* same with ORB + BF-Hamming 1-NN (max_dist < 0: no distance threshold, the cv2 path; else distance < max_dist, the DLL path) */
int vfsms_attempt_orb_batch(vfsms_ctx *ctx, const vfsms_roi_pair *jobs, int n,
                            const vfsms_orb_params *params, int max_dist, int offset_evaluate, int32_t *out);
/* same with SIFT (vfsms_sift_detect_describe's arithmetic, every distinct strip detected once and kept on the device) + BF-L2 2-NN +
 * ratio + vote.  Strips are processed in groups whose pyramids fit a byte budget (4 GiB; VFSMS_SIFT_GROUP_BYTES overrides); results do
 * not depend on the grouping.  params->n_features > 0 returns VFSMS_ERR_UNSUPPORTED as in vfsms_sift_detect_describe.          */
int vfsms_attempt_sift_batch(vfsms_ctx *ctx, const vfsms_roi_pair *jobs, int n,
                             const vfsms_sift_params *params, double ratio, int offset_evaluate, int32_t *out);
/* same for phase correlation (Stitcher.py:224-235): out: double[n][3] = {x, y, response}           */
int vfsms_attempt_phase_batch(vfsms_ctx *ctx, const vfsms_roi_pair *jobs, int n, double *out);
/* the same correlation resolved by overlap correlation (tests/phase_resolve_ref.py): strip-B pixel (r, c) meets strip-A pixel (r + dx,
 * c + dy).  rows: int32[n][VFSMS_ATTEMPT_INTS] = {status, dx, dy, 0, 1, 1, index of the winning candidate, floor(score *
 * VFSMS_VERIFY_FIXED_ONE + 0.5)}; a row with status 0 still names the best candidate.  cands (may be NULL): int32[n][4 * peaks][4] =
 * {dx, dy, fixed-point score, shared pixels} of candidate 4 * peak + reading, readings (uy, ux), (uy - M, ux), (uy, ux - N),
 * (uy - M, ux - N) of the peak at (uy, ux) of the M x N surface; a reading under which the strips share no pixel scores 0 over 0
 * pixels, the readings of an absent peak are zeros.  peaks_out (may be NULL): int32[n][peaks][2] = {uy, ux}, (-1, -1) when absent.
 * peaks 1..VFSMS_PHASE_MAX_PEAKS, threshold -1..1, min_pixels >= 0.  One launch sequence per strip shape, one synchronisation.     */
int vfsms_attempt_phase_resolve_batch(vfsms_ctx *ctx, const vfsms_roi_pair *jobs, int n, int peaks, double threshold, int min_pixels,
                                      int32_t *rows, int32_t *cands, int32_t *peaks_out);

/* ---- whole shooting paths behind one call (the pair loop of Stitcher.flowStitch, Stitcher.py:64-79, around the incremental search of
 * Stitcher.py:306-367 / 205-258) -------------------------------------------------------------------------------------------------
 * The candidate state machine runs inside the library: speculative fused batches (a window of consecutive pairs at the inherited
 * direction, whole candidate rings at predicted turns), results selected in the reference's order
 *     for i in 1 .. maxI-1 { d = direction; do { attempt(d, i); d = rotate(d) } while (d != direction) },  maxI = floor(0.5 / roiRatio) + 2,
 * `direction` threaded from pair to pair (Stitcher.py:252,361).  out: int32[last_pair - first_pair][6] = {status, dx, dy, accepted
 * direction, ROI growth i, votes}, offsets already carried back to full-tile coordinates (Stitcher.py:352-360); direction_out: the
 * direction the path leaves with; stats (optional, int64[8]): attempts evaluated, fused batches, keypoint-capacity retries, sum nA*nB,
 * sum nA+nB, ROI pixels processed (workload figures for roofline reports), 2 reserved.
 * midpath != 0: the chain starts inside a path (a rank of the pair-sharded form): speculation stays short until two runs were seen.
 * stop_on_fail != 0: stop behind the first pair that cannot be registered (flowStitch breaks there, Stitcher.py:74-76).              */
typedef struct { int32_t pair, direction, i; } vfsms_attempt_key;
typedef struct {
    int32_t method;                  /* 0 SURF + BF-L2 + ratio + mode, 1 ORB + BF-Hamming + mode, 2 FP64 phase correlation,
                                      * 3 SIFT; evaluator-supplied only (the *_eval entry points: the chain itself never reads `method`,
                                      * vfsms_pairs_offsets and _blind refuse it)                                                   */
    int32_t offset_evaluate;         /* Method.offsetEvaluate                                                                      */
    int32_t direct_incre;            /* Stitcher.directIncre: 1, 0 or -1                                                           */
    int32_t window;                  /* speculation window (attempts per fused batch)                                              */
    int32_t orb_max_dist;            /* < 0: no Hamming threshold (the cv2 path)                                                   */
    int32_t enhance_mode;            /* Method.isEnhance: 0 none, 1 equalizeHist, 2 CLAHE (SURF only)                              */
    int32_t tile_grid;               /* Method.tileSize                                                                            */
    int32_t reserved;
    double roi_ratio;                /* Method.roiRatio                                                                            */
    double search_ratio;             /* Method.searchRatio (ratio test)                                                            */
    double phase_threshold;          /* Stitcher.phaseResponseThreshold                                                            */
    double clip_limit;               /* Method.clipLimit                                                                           */
    vfsms_surf_params surf;
    vfsms_orb_params orb;
    /* optional PREDICTION of the accepted direction of every pair of the path (the stage's scan pattern: e.g. a column serpentine of known
     * height), path_hint[k] in 1..4 for pair k, or NULL.  It only primes the speculation predictor of a chain that starts inside the path
     * (a rank of the pair-sharded form knows nothing of the runs before its chunk) -- results never depend on it.                       */
    const int32_t *path_hint;
    int32_t path_hint_len;
    int32_t reserved2;
} vfsms_grid_params;
int vfsms_pairs_offsets(vfsms_ctx *ctx, const int64_t *tiles, const int32_t *shapes_hw, int n_tiles, int first_pair, int last_pair,
                        int direction_in, int midpath, int stop_on_fail, const vfsms_grid_params *p, int32_t *out,
                        int32_t *direction_out, int64_t *stats);
/* The same state machine over a caller-supplied evaluator of fused batches (other operators; the CPU tests): eval fills
 * rows[n][VFSMS_ATTEMPT_INTS] = {status, raw dx, raw dy, votes, nA, nB, ...} for n attempts and returns VFSMS_OK.  An attempt is
 * accepted when status != 0 && nA > 0 && nB > 0, whatever the method: a phase evaluator applies its response gate itself (status =
 * response > threshold, raw offsets truncated towards zero) and reports votes = 0, nA = nB = 1.                                     */
typedef int (*vfsms_attempt_eval)(void *user, const vfsms_attempt_key *items, int n, int32_t *rows);
int vfsms_pairs_offsets_eval(vfsms_attempt_eval eval, void *user, const int32_t *shapes_hw, int n_tiles, int first_pair, int last_pair,
                             int direction_in, int midpath, int stop_on_fail, const vfsms_grid_params *p, int32_t *out,
                             int32_t *direction_out, int64_t *stats);
/* A chunk in the MIDDLE of a path (a rank > 0 of the pair-sharded multi-GPU form): its incoming `self.direction` (Stitcher.py:252,361)
 * is the result of pairs another GPU is still registering, so the chunk [first_pair, last_pair) is registered for each of the four
 * possible incoming directions -- first candidates of the first pair in ONE batch, shared attempt cache, chains merged as soon as
 * they agree (after one pair, in practice).  out: int32[4][per][6], chain of incoming direction d at (d - 1) * per * 6 (per >= chunk
 * length: the padded row count of the all-gather payload); direction_out[4] = the direction each chain ends in.              */
int vfsms_pairs_offsets_blind(vfsms_ctx *ctx, const int64_t *tiles, const int32_t *shapes_hw, int n_tiles, int first_pair, int last_pair,
                              int per, const vfsms_grid_params *p, int32_t *out, int32_t *direction_out, int64_t *stats);
int vfsms_pairs_offsets_blind_eval(vfsms_attempt_eval eval, void *user, const int32_t *shapes_hw, int n_tiles, int first_pair, int last_pair,
                                   int per, const vfsms_grid_params *p, int32_t *out, int32_t *direction_out, int64_t *stats);

/* ---- whole-tile feature search with the reference's feature cache (Stitcher.calculateOffsetForFeatureSearch, Stitcher.py:260-304) --
 * Stitcher.tempImageFeature (Stitcher.py:14-18,278-290) keeps tile B's keypoints + descriptors so that they become tile A's of the
 * next pair; here that payload stays in HBM under a handle: SURF (+ optional enhancement, Stitcher.py:269-276) of a rectangle of a
 * resident tile -> feature handle; two handles -> BF-L2 2-NN + ratio + mode vote, only out[8] = {status, dx, dy, votes, nA, nB,
 * nMatches, 0} returns to the host.  vfsms_features_download gives the arrays Method.detectAndDescribe would have returned.      */
int vfsms_features_surf(vfsms_ctx *ctx, int64_t tile, int y0, int x0, int h, int w, const vfsms_surf_params *params,
                        int enhance_mode, double clip_limit, int tile_grid, int64_t *feat, int *n_out);
int vfsms_features_match_offset(vfsms_ctx *ctx, int64_t feat_a, int64_t feat_b, double ratio, int offset_evaluate, int32_t *out);
int vfsms_features_download(vfsms_ctx *ctx, int64_t feat, float *kps_xy, float *desc, int cap, int *n_out, int *dim_out);
/* The same for MANY tiles at once (the line scans of Main.py:29-51: 4 of the 6 demo datasets run calculateOffsetForFeatureSearch over
 * consecutive files, Stitcher.py:260-304): whole tiles, up to 16 per fused launch sequence, one host synchronisation per chunk;
 * feats[k] / counts[k] receive the set of tiles[k].  vfsms_features_match_offset_batch matches n (query set, train set) jobs --
 * the N - 1 consecutive pairs of a scan -- and votes in ONE batch: out[8 k ..] as vfsms_features_match_offset.                 */
int vfsms_features_surf_batch(vfsms_ctx *ctx, const int64_t *tiles, int n, const vfsms_surf_params *params,
                              int enhance_mode, double clip_limit, int tile_grid, int64_t *feats, int *counts);
int vfsms_features_match_offset_batch(vfsms_ctx *ctx, const int64_t *feat_a, const int64_t *feat_b, int n, double ratio,
                                      int offset_evaluate, int32_t *out);
int vfsms_features_free(vfsms_ctx *ctx, int64_t feat);
/* cv2.equalizeHist(img) (mode 1) / cv2.createCLAHE(clip_limit, (tile_grid, tile_grid)).apply(img) (mode 2), Stitcher.py:269-276;
 * out: uint8 [h][w] contiguous                                                                                                     */
int vfsms_enhance_u8(vfsms_ctx *ctx, const uint8_t *img, int h, int w, int stride, int mode, double clip_limit, int tile_grid,
                     uint8_t *out);

/* ---- device-resident mosaic canvas (Stitcher.getStitchByOffset, Stitcher.py:369-486) -------------- */
/* u8 canvas + validity plane instead of the reference's int64 / -1 sentinel                         */
int vfsms_canvas_create(vfsms_ctx *ctx, int rows, int cols, int ch, int64_t *handle);
/* the buffers of the canvas freed last stay with the context for the next canvas of the same size (released by the next free of another
 * canvas or with the context): a session's mosaics are of one size, and allocating 2 x rows x cols bytes costs more than assembling them      */
int vfsms_canvas_free(vfsms_ctx *ctx, int64_t handle);
/* plain paste of a host tile (u8 [h][w][ch]) at (y0, x0): Stitcher.py:444-451 ("notFuse" / tile 0)  */
int vfsms_canvas_paste(vfsms_ctx *ctx, int64_t canvas, const uint8_t *tile, int h, int w, int y0, int x0);
/* paste + fade-fuse of the ROI [ry0,ry1) x [rx0,rx1) (canvas coords) exactly as Stitcher.py:457-483 +
 * ImageFusion.py:192-244 do: A = canvas before paste, B = canvas after paste.  info as above.        */
int vfsms_canvas_fuse_tile(vfsms_ctx *ctx, int64_t canvas, const uint8_t *tile, int h, int w,
                           int y0, int x0, int ry0, int rx0, int ry1, int rx1,
                           int dx, int dy, int32_t *info);
/* the same with the blend chosen by `method`: 0 fadeInAndFadeOut, 1 trigonometric (Stitcher.fuseImage, Stitcher.py:488-525),
 * 2 multiBandBlending (vfsms_fuse_multiband_i64 on the canvas, levels from vfsms_canvas_set_multiband_levels),
 * 3 optimalSeamLine (vfsms_fuse_seam_i64 on the canvas, blend from vfsms_canvas_set_seam_blend)                                  */
int vfsms_canvas_fuse_tile_m(vfsms_ctx *ctx, int64_t canvas, const uint8_t *tile, int h, int w,
                             int y0, int x0, int ry0, int rx0, int ry1, int rx1,
                             int dx, int dy, int method, int32_t *info);
/* paste + element-wise blend of the ROI for fuseMethod "average" / "maximum" / "minimum" (mode 0 / 1 / 2): ImageFusion.py:12-41
 * behind the zero / empty filling of Stitcher.fuseImage (Stitcher.py:498-504).                                              */
int vfsms_canvas_blend_tile(vfsms_ctx *ctx, int64_t canvas, const uint8_t *tile, int h, int w,
                            int y0, int x0, int ry0, int rx0, int ry1, int rx1, int mode);
/* the same two operations for a tile that is already resident in HBM (a handle from vfsms_tile_upload / vfsms_tile_wrap with
 * stride == w, e.g. the tiles the registration phase uploaded, or a colour tile from vfsms_tile_upload_ch): no host copy; the
 * tile's channel count must be the canvas's.
 * With info == NULL the fuse only enqueues work (no host synchronisation per tile); a degenerate corner geometry -- where the
 * reference's getWeightsMatrix raises -- is then latched in the canvas and reported by vfsms_canvas_download.               */
int vfsms_canvas_paste_tile(vfsms_ctx *ctx, int64_t canvas, int64_t tile, int y0, int x0);
/* vfsms_canvas_blend_tile ("average" / "maximum" / "minimum", mode 0 / 1 / 2) for a resident tile; enqueue only                       */
int vfsms_canvas_blend_tile_resident(vfsms_ctx *ctx, int64_t canvas, int64_t tile,
                                     int y0, int x0, int ry0, int rx0, int ry1, int rx1, int mode);
int vfsms_canvas_fuse_tile_resident(vfsms_ctx *ctx, int64_t canvas, int64_t tile,
                                    int y0, int x0, int ry0, int rx0, int ry1, int rx1,
                                    int dx, int dy, int32_t *info);
int vfsms_canvas_fuse_tile_resident_m(vfsms_ctx *ctx, int64_t canvas, int64_t tile,
                                      int y0, int x0, int ry0, int rx0, int ry1, int rx1,
                                      int dx, int dy, int method, int32_t *info);
/* How a tile goes onto the canvas: the `mode` of a geometry row, and the one code the library speaks inside.  The numbers are ABI
 * (5 is not a mode).  The `method` 0..3 of vfsms_canvas_fuse_tile*_m is FADE, TRIG, MULTIBAND, SEAMLINE in that order, the `mode`
 * 0..2 of vfsms_canvas_blend_tile* is AVERAGE, MAXIMUM, MINIMUM.                                                              */
enum vfsms_canvas_mode {
    VFSMS_CANVAS_PASTE = -1,      /* the first tile, fuseMethod "notFuse" */
    VFSMS_CANVAS_FADE = 0,        /* fadeInAndFadeOut */
    VFSMS_CANVAS_TRIG = 1,        /* trigonometric */
    VFSMS_CANVAS_AVERAGE = 2,
    VFSMS_CANVAS_MAXIMUM = 3,
    VFSMS_CANVAS_MINIMUM = 4,
    VFSMS_CANVAS_MULTIBAND = 6,   /* multiBandBlending */
    VFSMS_CANVAS_SEAMLINE = 7     /* optimalSeamLine */
};
/* The canvas walk of Stitcher.getStitchByOffset (Stitcher.py:434-483) over n resident tiles in one call.
 * geom: n x 9 ints [y0, x0, ry0, rx0, ry1, rx1, dx, dy, mode], mode a vfsms_canvas_mode.  Every row is checked before anything is
 * enqueued.  Enqueue only: errors of a tile's geometry surface in the download. */
int vfsms_canvas_assemble_resident(vfsms_ctx *ctx, int64_t canvas, int n, const int64_t *tiles, const int32_t *geom);
/* pyramid levels (1..8) of the canvas's multiBandBlending fuses; a new canvas starts at 4                                      */
int vfsms_canvas_set_multiband_levels(vfsms_ctx *ctx, int64_t canvas, int levels);
/* how the canvas's optimalSeamLine fuses merge the two sides of the seam: 0 none, 1 multiBandBlending (with the canvas's level count);
 * a new canvas starts at 0                                                                                                          */
int vfsms_canvas_set_seam_blend(vfsms_ctx *ctx, int64_t canvas, int blend);
/* final image: empty -> 0 (Stitcher.py:485-486).  out: u8 [rows][cols][ch]                           */
int vfsms_canvas_download(vfsms_ctx *ctx, int64_t canvas, uint8_t *out);
/* rows [row0, row0 + nrows) of the same image: a multi-GB mosaic leaves the device band by band and can be handed to an
 * incremental writer (the reference holds the whole int64 canvas and the u8 copy in host memory, Stitcher.py:434-436, 485-486) */
int vfsms_canvas_download_rows(vfsms_ctx *ctx, int64_t canvas, int row0, int nrows, uint8_t *out);
/* for writers of tiled multi-resolution files (Stitcher.outputPyramid, PyramidTiffBandWriter): the same rows to out0 (NULL: levels only)
 * and reduced levels 1 .. levels of them to out_levels, back to back, level k as u8 [ceil((row0 + nrows) / 2^k) - (row0 >> k)][C_k][ch]
 * with C_k = (C_{k-1} + 1) >> 1.  A sample of level k is (a + b + c + d + 2) >> 2 of the 2 x 2 block of level k - 1, edges replicated
 * at every level against that level's own size, every level rounded once from the rounded level below.  No reference counterpart: the
 * arithmetic, all integer, is this library's own specification, tests/pyramid_ref.py, and every level equals it exactly.  The levels
 * are formed on the device in one pass over the band (pyramid_kernels.hip); one stream synchronisation ends the call.
 * VFSMS_ERR_BAD_ARG: levels outside 1..VFSMS_PYRAMID_MAX_LEVELS, row0 not a multiple of 2^levels, nrows not a multiple of 2^levels unless
 * the band ends at the last row (such a band forms complete level rows that depend on no other band), cap_levels (bytes of out_levels)
 * too small, an unknown canvas; the sticky geometry flag as vfsms_canvas_download_rows                                                */
#define VFSMS_PYRAMID_MAX_LEVELS 10
int vfsms_canvas_download_rows_pyramid(vfsms_ctx *ctx, int64_t canvas, int row0, int nrows, int levels,
                                       uint8_t *out0, uint8_t *out_levels, size_t cap_levels);
/* Rows [row0, row0 + nrows) of the mosaic as the entropy-coded bytes of a baseline JPEG (see vfsms_jpeg_header above), so a band leaves
 * the device compressed and the host only appends it to a file.  The band contract: row0 is a multiple of the MCU height; the MCUs in
 * front of the band are a multiple of the restart interval, and so are the band's own unless it ends at the last row (VFSMS_ERR_BAD_ARG
 * otherwise).  An RSTn follows every interval but the image's last: the bytes of all bands, behind vfsms_jpeg_header's and in front of
 * FF D9, are the file.  *nbytes = the size needed, also on VFSMS_ERR_CAPACITY (nothing is written then; the call may be repeated).  The
 * sticky geometry flag as vfsms_canvas_download_rows.                                                                                   */
int vfsms_canvas_encode_jpeg_rows(vfsms_ctx *ctx, int64_t canvas, int row0, int nrows, int quality, int restart_mcus,
                                  uint8_t *out, size_t cap, size_t *nbytes);
/* ---- JPEG tiles for pyramidal TIFF (Method.pyramidCompression = "jpeg": TIFF compression 7, shared tables in JPEGTables), encoded on the
 * device in tile order.  Specification: tests/tiff_jpeg_ref.py (on tests/jpeg_enc_ref.py and tests/pyramid_ref.py); bytes equal it exactly.
 * A tile is a whole tile x tile image to the coder: samples beyond the level's last row or column repeat it, DC predictors and RSTn
 * numbering start at 0, no RSTn follows the last interval.  Its stream is abbreviated: SOI, SOF0, DRI (restart_mcus > 0), SOS, scan, EOI.
 * Refused everywhere (VFSMS_ERR_BAD_ARG): a tile that is no positive multiple of 16, restart_mcus outside 0..65535 (0: one interval per
 * tile), MCUs of a tile -- (tile / 16)^2 colour, (tile / 8)^2 gray -- that are no whole number of intervals or more than 65535 in one,
 * quality outside 1..100, channels other than 1 or 3.
 * vfsms_tiff_jpeg_tables (host only, no context): the JPEGTables datastream -- SOI, the DQT and DHT segments of vfsms_jpeg_header, EOI.
 * vfsms_jpeg_encode_tiles_device: an image on the host -> all its tile streams, row-major and back to back; offsets[0 .. n_tiles] (the
 * last being the total; offsets_cap counts entries).  *nbytes = the size needed, also on VFSMS_ERR_CAPACITY.                         */
int vfsms_tiff_jpeg_tables(int ch, int quality, uint8_t *out, size_t cap, size_t *nbytes);
int vfsms_jpeg_encode_tiles_device(vfsms_ctx *ctx, const uint8_t *img, int h, int w, int ch, int stride, int bgr, int tile, int quality,
                                   int restart_mcus, uint8_t *out, size_t cap, size_t *nbytes, uint64_t *offsets, int offsets_cap);
/* Every tile row of level 0 and of reduced levels 1 .. levels (0..VFSMS_PYRAMID_MAX_LEVELS) that the band [row0, row0 + nrows) of the
 * mosaic completes, as finished tile streams back to back in `out`; index: int64 records {level, tile number in the level (row-major),
 * offset in out, bytes}, index_cap counts records, in the payload's order: level after level, a level's tiles row-major.  Band contract
 * (VFSMS_ERR_BAD_ARG otherwise): vfsms_canvas_download_rows_pyramid's; row0 a multiple of the tile; nrows a multiple of the tile unless
 * the band ends at the last row; bands in order from row 0 (row0 = 0 starts over), with one tile and level count.  Rows of a reduced level that do not fill a tile row yet stay on the device until a later band completes it; the last band
 * flushes them: nothing of the reduced levels crosses the link as pixels.  *nbytes, *n_index = the sizes needed, also on
 * VFSMS_ERR_CAPACITY (nothing is written and no row consumed: repeat the call with room).  The sticky geometry flag as
 * vfsms_canvas_download_rows.                                                                                                         */
int vfsms_canvas_encode_pyramid_tiles(vfsms_ctx *ctx, int64_t canvas, int row0, int nrows, int levels, int tile, int quality, int restart_mcus,
                                      uint8_t *out, size_t cap, size_t *nbytes, int64_t *index, int index_cap, int *n_index);

/* ---- lossless tiles for pyramidal TIFF (Method.pyramidCompression = "deflate-device": TIFF compression 8 with Predictor = 2), encoded on the
 * device in tile order.  Specification: tests/deflate_ref.py (on tests/pyramid_ref.py); bytes equal it exactly.  A tile's stream is a plain
 * zlib stream of its tile x tile x ch samples after horizontal differencing: colour R G B, samples beyond the level's last row or column 0
 * (as the "none" and "deflate" writers pad, unlike the JPEG tiles); deflate restricted to runs at distance 1 and one dynamic Huffman block.
 * Refused everywhere (VFSMS_ERR_BAD_ARG): a tile that is no positive multiple of 16 or larger than 4096, channels other than 1 or 3, more
 * tiles (2^31 - 1) or chunks of 4096 bytes (2^24 - 1) than one call takes.
 * vfsms_deflate_encode_tiles_device: an image on the host (B G R with bgr != 0, else R G B; rows `stride` bytes apart) -> all its tile
 * streams, row-major and back to back; offsets[0 .. n_tiles] (the last being the total; offsets_cap counts entries).  *nbytes = the size
 * needed, also on VFSMS_ERR_CAPACITY.                                                                                                  */
int vfsms_deflate_encode_tiles_device(vfsms_ctx *ctx, const uint8_t *img, int h, int w, int ch, int stride, int bgr, int tile,
                                      uint8_t *out, size_t cap, size_t *nbytes, uint64_t *offsets, int offsets_cap);
/* vfsms_canvas_encode_pyramid_tiles with the lossless coder: the same band contract, index records and capacity behaviour (on
 * VFSMS_ERR_CAPACITY nothing is written and no row consumed: repeat the call with room), over the same walk of a canvas.  A walk belongs
 * to the entry that started it at row0 = 0: a band of one entry that continues a walk of the other is refused with VFSMS_ERR_BAD_ARG and
 * the walk stays as it was; row0 = 0 starts over with either.                                                                          */
int vfsms_canvas_encode_pyramid_tiles_deflate(vfsms_ctx *ctx, int64_t canvas, int row0, int nrows, int levels, int tile,
                                              uint8_t *out, size_t cap, size_t *nbytes, int64_t *index, int index_cap, int *n_index);

/* ---- PNG coded on the device (Method.pngEncoder = "device").  Specification: tests/png_ref.py (on tests/deflate_ref.py); bytes equal it exactly.
 * Rows are cut into segments of segment_rows rows.  Every row gets the PNG filter (None, Sub, Up, Average, Paeth) of the smallest sum of
 * absolutes, ties to the lowest type, against the raw row above it in the whole image; a segment's filter types and filtered bytes are coded
 * by the lossless tile coder above (runs at distance 1, one dynamic Huffman block) as a block that is not final, followed by an empty stored
 * block, and framed as one IDAT chunk with its CRC-32.  Behind the signature, IHDR and IDAT(78 01), and in front of
 * IDAT(01 00 00 FF FF + the Adler-32 of all filtered bytes) and IEND, the chunks of all segments are the file; colour is stored R G B.
 * Refused everywhere (VFSMS_ERR_BAD_ARG): channels other than 1 or 3, segment_rows outside 1..4096, a segment whose bytes at 15 bits each
 * exceed 32 bits, more chunks of 4096 bytes (2^24 - 1) than one call takes.
 * vfsms_png_encode_device: an image on the host (B G R with bgr != 0, else R G B; rows `stride` bytes apart) -> the chunks of all its segments
 * and the Adler-32 of its filtered bytes.  *nbytes = the size needed, also on VFSMS_ERR_CAPACITY (nothing is written then; the call may be
 * repeated).
 * vfsms_canvas_encode_png_rows: rows [row0, row0 + nrows) of the mosaic as vfsms_canvas_download_rows hands them out, coded the same way;
 * *adler is the band's own Adler-32 (zlib's adler32_combine joins the bands').  Band contract (VFSMS_ERR_BAD_ARG otherwise): row0 a multiple
 * of segment_rows; nrows too unless the band ends at the last row.  The entry keeps no state between bands -- the row above row0 is read from
 * the canvas -- so any band may be asked for, and asked for again, and a pyramid walk in progress is not disturbed.  The sticky geometry
 * flag as vfsms_canvas_download_rows.                                                                                                  */
int vfsms_png_encode_device(vfsms_ctx *ctx, const uint8_t *img, int h, int w, int ch, int stride, int bgr, int segment_rows,
                            uint8_t *out, size_t cap, size_t *nbytes, uint32_t *adler);
int vfsms_canvas_encode_png_rows(vfsms_ctx *ctx, int64_t canvas, int row0, int nrows, int segment_rows,
                                 uint8_t *out, size_t cap, size_t *nbytes, uint32_t *adler);

/* ---- flat-field shading correction (Method.shadingCorrection).  No reference counterpart: the arithmetic, all integer, is this
 * library's own specification, tests/shading_ref.py, and every stage equals it exactly. -------------------------------------- */
/* A shading field from n (1..4096) resident tiles of one shape and channel count (any row stride): per sample the k-th smallest byte
 * over the tiles, k = (n - 1) * percentile / 100 (percentile 0..100), as Q8 smoothed by two rounded (2 radius + 1)^2 box passes with
 * replicated borders (radius 1..127), turned into a Q12 gain min(65535, (mean * 4096 + Q / 2) / Q) per channel (4096 where Q == 0)
 * (tests/shading_ref.py).  Waits for reserved / pending tiles like every batch call; the tiles are only read.                  */
int vfsms_shading_estimate(vfsms_ctx *ctx, int n, const int64_t *tiles, int percentile, int radius, int64_t *field);
/* a field measured elsewhere (a blank-slide image): gain is uint16 Q12 [h][w][ch], used as it is (tests/shading_ref.py: apply)  */
int vfsms_shading_from_gain(vfsms_ctx *ctx, const uint16_t *gain, int h, int w, int ch, int64_t *field);
/* gain: uint16 [h][w][ch]; smooth_q8 (may be NULL): the smoothed Q8 field, uint16; profile (may be NULL): the order statistic, u8;
 * both are zeros for a field from vfsms_shading_from_gain (tests/shading_ref.py: estimate returns the three planes)             */
int vfsms_shading_download(vfsms_ctx *ctx, int64_t field, uint16_t *gain, uint16_t *smooth_q8, uint8_t *profile);
/* out = min(255, (p * gain + 2048) >> 12) in place on n resident tiles of the field's shape (tests/shading_ref.py: apply).  Refused:
 * a tile from vfsms_tile_wrap (the library does not own that memory and must not rewrite it), a tile named twice in one call (it
 * would be corrected twice), a shape other than the field's.  Waits for reserved / pending tiles.                                */
int vfsms_shading_apply(vfsms_ctx *ctx, int64_t field, int n, const int64_t *tiles);
/* releases a field of vfsms_shading_estimate / vfsms_shading_from_gain (tests/shading_ref.py has no state to free)              */
int vfsms_shading_free(vfsms_ctx *ctx, int64_t field);

/* ---- focus stacking (Method.focusStack).  No reference counterpart: the arithmetic, all integer, is this library's own
 * specification, tests/focus_ref.py, and every stage equals it exactly. ----------------------------------------------------------- */
/* n (2..64) resident planes of one shape, gray or B G R (1 or 3 channels; any row stride and base), fused into one tile.  Mode 0
 * "pixel": the luma L = the byte or (29 B + 150 G + 77 R + 128) >> 8, the sum-modified Laplacian M = |2L - L(x-1) - L(x+1)| +
 * |2L - L(y-1) - L(y+1)| with clamped indices, its box sum F over (2 radius + 1)^2 with clamped indices (radius 1..31), D = the
 * smallest plane index of the largest F per pixel, with median 1 replaced once by the median of its 3 x 3 neighbourhood (clamped),
 * out = plane[D].  Mode 1 "plane": the whole plane of the largest score, the first of them; D is constant.  scores[i] = the sum of
 * M_i over the plane, in both modes (tests/focus_ref.py: fuse).  out_tile (may be NULL): a NEW resident tile, freed with
 * vfsms_tile_free; out_host (may be NULL): dense [h][w][ch]; index (may be NULL): D, [h][w]; scores (may be NULL): [n].
 * Waits for reserved / pending tiles like every batch call; the planes are only read.  VFSMS_ERR_BAD_ARG, with nothing written and
 * no tile created: n outside 2..64, an unknown handle, planes of different shape or channel count, a channel count other than 1 or
 * 3, radius outside 1..31, a median other than 0 or 1, a mode other than 0 or 1.                                                  */
int vfsms_focus_stack(vfsms_ctx *ctx, int n, const int64_t *planes, int mode, int radius, int median,
                      int64_t *out_tile, uint8_t *out_host, uint8_t *index, int64_t *scores);
/* scores[i] = the sum of M over tile i (tests/focus_ref.py: scores): n (1..4096) resident tiles of any shapes, gray or B G R     */
int vfsms_focus_scores(vfsms_ctx *ctx, int n, const int64_t *tiles, int64_t *scores);

/* ---- 16-bit gray tiles.  No reference counterpart: the arithmetic, all integer, is this library's own
 * specification, tests/deep_ref.py, and every stage equals it exactly.  A deep tile has a handle kind of its own: every vfsms_deep_*
 * entry refuses any other handle, and every other entry refuses a deep handle, so no 8-bit call can be handed 16-bit memory. -------- */
/* A deep tile from img: h x w uint16 samples (sides 1..32768), rows stride_bytes apart (at least 2 w; any alignment).  The samples are
 * on the device when the call returns: the caller's memory is free.  VFSMS_ERR_BAD_ARG, nothing created: a side outside 1..32768, a
 * stride below 2 w, a null pointer.                                                                                                 */
int vfsms_deep_upload(vfsms_ctx *ctx, const uint16_t *img, int h, int w, int stride_bytes, int64_t *deep);
/* releases a deep tile (tests/deep_ref.py has no state to free)                                                                    */
int vfsms_deep_free(vfsms_ctx *ctx, int64_t deep);
/* One intensity window for n (1..4096) deep tiles of any shapes: with s = all their samples sorted and N their number, window[0] =
 * s[(N - 1) * lo_ppm / 1000000] and window[1] = s[(N - 1) * hi_ppm / 1000000], exactly (a two-pass radix select); when the two are
 * equal, window[1] is one more (window[0] one less at 65535) (tests/deep_ref.py: window).  The tiles are only read.
 * VFSMS_ERR_BAD_ARG, nothing written: n outside 1..4096, a handle that is no deep tile, not 0 <= lo_ppm <= hi_ppm <= 1000000.       */
int vfsms_deep_window(vfsms_ctx *ctx, int n, const int64_t *deeps, int lo_ppm, int hi_ppm, int32_t *window);
/* The 8-bit registration views of n (1..4096) deep tiles: out = ((min(max(v, lo), hi) - lo) * 255 + D / 2) / D, D = hi - lo
 * (tests/deep_ref.py: reduce).  tiles_out[i]: a NEW ordinary resident gray tile of tile i's shape, freed with vfsms_tile_free, as
 * vfsms_focus_stack returns its out_tile.  VFSMS_ERR_BAD_ARG, nothing written: n outside 1..4096, a handle that is no deep tile, not
 * 0 <= lo < hi <= 65535.  On any error no tile is created.                                                                        */
int vfsms_deep_reduce(vfsms_ctx *ctx, int n, const int64_t *deeps, int lo, int hi, int64_t *tiles_out);
/* Rows [row0, row0 + nrows) of the rows x cols uint16 mosaic GATHERED from n (1..4096) deep tiles, tile i's top-left corner at
 * (yx[2 i], yx[2 i + 1]), into out, dense [nrows][cols] on the host (tests/deep_ref.py: mosaic).  A pixel no tile covers is 0.  mode 0
 * (paste): the sample of the covering tile of the largest index; mode 1 (feather): (sum w p + (sum w) / 2) / sum w over the covering
 * tiles with w = min(r + 1, h - r, c + 1, w - c) at the tile's own (r, c), cut at `feather` when that is positive.  The result does not
 * depend on the order of the tiles in mode 1.  Stateless: any band on demand, no canvas exists; the tiles are only read, may differ in
 * shape, lie inside each other, share a position, and a handle may be named more than once.  VFSMS_ERR_BAD_ARG, nothing written, the
 * first of these in this order: n outside 1..4096, a handle that is no deep tile, a tile outside the canvas, a mode other than 0 or 1,
 * feather outside 0..32767, a band outside the canvas or of more than 2^30 samples.  VFSMS_ERR_CAPACITY: the band meets more than
 * 2^26 (tile, 32 x 256 block) pairs; shorter bands do not.                                                                          */
int vfsms_deep_mosaic_rows(vfsms_ctx *ctx, int n, const int64_t *deeps, const int32_t *yx, int rows, int cols, int mode, int feather,
                           int row0, int nrows, uint16_t *out);
/* The samples of a deep tile back on the host: out holds h rows of w uint16, rows stride_bytes apart (at least 2 w; any alignment).
 * VFSMS_ERR_BAD_ARG, nothing written: a handle that is no deep tile, a null pointer, a stride below 2 w.                             */
int vfsms_deep_download(vfsms_ctx *ctx, int64_t deep, uint16_t *out, int stride_bytes);

/* ---- flat-field shading correction of deep tiles.  No reference counterpart: the arithmetic, all integer, is this library's own
 * specification, tests/deep_shading_ref.py, and every stage equals it exactly.  A deep field has a handle kind of its own: every
 * vfsms_shading_* entry refuses it, and the entries below refuse a field of vfsms_shading_estimate / vfsms_shading_from_gain and
 * any handle that is no deep tile. ------------------------------------------------------------------------------------------------- */
/* A deep shading field from n (1..4096) deep tiles of ONE shape: per position the k-th smallest sample over the tiles, k = (n - 1) *
 * percentile / 100 (percentile 0..100), less the camera's dark level `pedestal` (0..65535) and clamped at 0: F = max(P - pedestal, 0),
 * uint16 with no Q8 shift; F smoothed by two rounded (2 radius + 1)^2 box passes with replicated borders (radius 1..127); the Q12 gain
 * min(65535, (mean * 4096 + F / 2) / F), 4096 where F == 0 (tests/deep_shading_ref.py: estimate).  The tiles are only read.
 * VFSMS_ERR_BAD_ARG, nothing created and nothing written, the first of these in this order: n outside 1..4096, a handle that is no
 * deep tile of this context, tiles of more than one shape, percentile / radius / pedestal outside their ranges, a null pointer.
 * VFSMS_ERR_UNSUPPORTED: a plane of more than 2^31 - 1 samples or 65535 rows, as vfsms_shading_estimate.  On any error no field is
 * created.                                                                                                                          */
int vfsms_deep_shading_estimate(vfsms_ctx *ctx, int n, const int64_t *deeps, int percentile, int radius, int pedestal, int64_t *field);
/* a field measured elsewhere (a blank slide): gain is uint16 Q12 [h][w] (sides 1..32768), used as it is, with the pedestal the
 * corrected tiles carry (tests/deep_shading_ref.py: apply).  VFSMS_ERR_BAD_ARG, nothing created: a side or the pedestal outside its
 * range, a null pointer.                                                                                                            */
int vfsms_deep_shading_from_gain(vfsms_ctx *ctx, const uint16_t *gain, int h, int w, int pedestal, int64_t *field);
/* gain: uint16 [h][w]; smooth (may be NULL): the smoothed field F; profile (may be NULL): the order statistic P, both uint16 [h][w] and
 * zeros for a field from vfsms_deep_shading_from_gain; pedestal (may be NULL): the field's pedestal (tests/deep_shading_ref.py:
 * estimate returns the three planes).  VFSMS_ERR_BAD_ARG, nothing written: a handle that is no deep field, a null gain.           */
int vfsms_deep_shading_download(vfsms_ctx *ctx, int64_t field, uint16_t *gain, uint16_t *smooth, uint16_t *profile, int32_t *pedestal);
/* In place on n (1..4096) deep tiles of the field's shape, with d the field's pedestal: a sample p <= d is left alone, any other
 * becomes min(65535, d + (((p - d) * gain + 2048) >> 12)) (tests/deep_shading_ref.py: apply).  VFSMS_ERR_BAD_ARG, nothing written, the
 * first of these in this order: n outside 1..4096, a handle that is no deep tile of this context, a handle that is no deep field, a
 * shape other than the field's, a tile named twice in one call (it would be corrected twice).                                       */
int vfsms_deep_shading_apply(vfsms_ctx *ctx, int64_t field, int n, const int64_t *deeps);
/* releases a field of vfsms_deep_shading_estimate / vfsms_deep_shading_from_gain (tests/deep_shading_ref.py has no state to free)   */
int vfsms_deep_shading_free(vfsms_ctx *ctx, int64_t field);

/* ---- per-tile exposure compensation (Method.exposureCompensation).  No reference counterpart: the specification is
 * tests/exposure_ref.py; the sums and the corrected bytes are integers and equal it exactly. ------------------------------------ */
/* The overlap statistic of n pairs of resident tiles (gray or interleaved colour, both tiles of a job of one channel count, any
 * shapes, any row strides).  A job is a vfsms_ncc_job: tile B's pixel (r, c) meets tile A's pixel (r + dx, c + dy).  Over every sample
 * (a byte of a pixel) of the B pixels whose partner lies inside A, with lo <= a <= hi and lo <= b <= hi (0 <= lo <= hi <= 255): out3 =
 * int64[n][3] = {N, Sa, Sb}, the number of such samples and the sums of the A and of the B samples; an empty rectangle gives zeros.
 * One launch sequence for all jobs.  Waits for reserved / pending tiles like every batch call; the tiles are only read.
 * VFSMS_ERR_BAD_ARG: an unknown handle, different channel counts in a job, lo > hi or a bound outside 0..255.  n = 0 is fine.      */
int vfsms_overlap_stats_batch(vfsms_ctx *ctx, const vfsms_ncc_job *jobs, int n, int lo, int hi, int64_t *out3);
/* out = min(255, (p * gain_q12[i] + 2048) >> 12) in place on every sample of tile i, n (1..4096) resident tiles of any shapes
 * (tests/exposure_ref.py: apply); a tile whose gain is 4096 is not touched.  Refused like vfsms_shading_apply: a tile from
 * vfsms_tile_wrap, a tile named twice in one call.  Waits for reserved / pending tiles.                                            */
int vfsms_exposure_apply(vfsms_ctx *ctx, int n, const int64_t *tiles, const uint16_t *gain_q12);

/* ---- radial lens correction (Method.lensCorrection).  No reference counterpart: the specification is tests/lens_ref.py; the
 * surfaces, the best candidates and the resampled bytes are integers and equal it exactly. ---------------------------------------- */
/* The block displacement field of n pairs of resident tiles.  A job is a vfsms_ncc_job: tile B's pixel (r, c) meets tile A's pixel
 * (r + dx, c + dy); both tiles of a job have ONE shape and channel count, gray or B G R (a colour sample is its luma
 * (29 B + 150 G + 77 R + 128) >> 8), any row strides.  The overlap rectangle of B, shrunk by `radius` on all four sides, is cut into
 * nby x nbx = ((r1 - r0) / block) x ((c1 - c0) / block) whole blocks from its top-left corner (none when one does not fit).  For
 * every block and every candidate (i, j) in [-radius, radius]^2 the six sums over B's block and A's samples at (y + dx + i,
 * x + dy + j), N = block^2, are scored as vfsms_verify_ncc scores them with min_pixels 0.  first = int64[n + 1]: first[k] the index of
 * job k's first block (row-major by, bx), first[n] the total, computed by the caller and checked here.  best4 = int32[blocks][4] =
 * {i, j, fixed-point score, block^2} under the tie order of vfsms_ncc_search_batch (a flat block: 0, 0, 0); surface (or NULL) =
 * int32[blocks][2 radius + 1][2 radius + 1].  block: 8..128 in multiples of 8; radius: 1..16.  One launch for all jobs, a workgroup per
 * block.  Waits for reserved / pending tiles like every batch call; the tiles are only read.
 * VFSMS_ERR_BAD_ARG, nothing written: an unknown handle, two shapes or channel counts in a job, a channel count other than 1 or 3, a
 * `first` that does not match the lattice.                                                                                          */
int vfsms_block_ncc_batch(vfsms_ctx *ctx, const vfsms_ncc_job *jobs, int n, int block, int radius, const int64_t *first, int32_t *best4,
                          int32_t *surface);
/* n (1..4096) resident tiles of any shapes resampled in place under the radial map of tests/lens_ref.py: output pixel (y, x) takes the
 * source position s = c + (p - c) (1 + a1 rho + a2 rho^2), rho = |p - c|^2 / D^2, D the half-diagonal, in integers: a1_q30, a2_q30 in
 * Q30 (|a| <= 2^28), the centre c = (cy2 / 2, cx2 / 2) in half pixels -- a coordinate below 0 stands for every tile's own middle
 * (h - 1, w - 1) -- positions in 1/256 px, a replicated border, channels independently.  interp 0: bilinear; 1: Catmull-Rom over 4 x 4
 * taps with exact integer weights.  a1 = a2 = 0 changes no byte.  Every tile is read from a copy in the context's scratch.
 * Refused like vfsms_shading_apply, nothing written: a tile from vfsms_tile_wrap, a tile named twice, a coefficient beyond 2^28, a
 * side beyond 16384, a centre outside the middle half of an axis of any tile (2 |cy2 - (h - 1)| > h - 1), another interp.          */
int vfsms_lens_apply(vfsms_ctx *ctx, int n, const int64_t *tiles, int32_t a1_q30, int32_t a2_q30, int32_t cy2, int32_t cx2, int interp);
/* the same map for a host image of h x w x ch bytes (ch 1..4, rows src_stride bytes apart) -> dst, dense; like vfsms_enhance_u8      */
int vfsms_lens_remap_u8(vfsms_ctx *ctx, const uint8_t *src, int h, int w, int ch, int src_stride, int32_t a1_q30, int32_t a2_q30,
                        int32_t cy2, int32_t cx2, int interp, uint8_t *dst);

#ifdef __cplusplus
}
#endif
#endif /* VFSMS_H */
