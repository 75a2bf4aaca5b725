// jpeg_host.cpp -- host-side JPEG decode straight into pinned staging, for the ingest pipeline (scope row f-1: "host libjpeg-turbo + pinned
// upload").  No kernels here.
//
// The decoder pool of the Python host (Pillow) stops scaling at ~16 threads on the 256-thread host of the MI355X box: every decode maps
// and faults in 4-17 MB of fresh memory and crosses the interpreter lock a few times, and the per-tile decode time grows with the
// parallelism.  This entry decodes with the system's libjpeg-turbo (libjpeg.so.8, ABI version 80: loaded with dlopen at first use, no
// link-time dependency and no header -- the image ships the library without its headers) into a pinned buffer that is REUSED from call to
// call, from any thread, without the interpreter lock (ctypes releases it), and hands the planes to the same device path as
// vfsms_tile_fill_pair.  Grayscale wanted: out_color_space = JCS_GRAYSCALE, the Y plane (cv2.imdecode(..., 0), Stitcher.py:68-69).  Colour
// wanted: out_color_space = JCS_YCbCr, the upsampled planes interleaved, no colour conversion on the host; the device derives the gray and
// the B G R tile (csrc/ingest_kernels.hip).
//
// The other direction, for the mosaic (cv2.imwrite at Stitcher.py:149, 175-179; Main.py writes every result as .jpg): vfsms_jpeg_encode
// turns a horizontal STRIPE of an image into a complete baseline JPEG stream with cv2.imwrite's settings (libjpeg defaults: 4:2:0, standard
// Huffman tables, quality 95 unless told otherwise).  Stripes whose heights are multiples of the MCU height share no state -- the DCT
// blocks, the 2x2 chroma box filter and the quantisation are local to an MCU row -- so the host encodes them on as many threads as it
// likes and joins their entropy-coded segments into ONE file as restart intervals (vfsms_jpeg_join: DRI = the MCUs of a stripe, an RSTn
// marker between two stripes).  The coefficients, hence the decoded pixels, are those of the one-thread encode of the whole image.
//
// A third entry stops even earlier, for Method.jpegDecoder = "device": jpeg_coefficients_host hands out the quantised DCT coefficients
// (jpeg_read_coefficients: the entropy decode and nothing else) and the file's quantisation tables; csrc/jpeg_dec_kernels.hip does the rest.
//
// ABI knowledge used (libjpeg 8 / libjpeg-turbo 2.x on x86-64, `boolean` = int): the public head of jpeg_decompress_struct up to
// output_scanline and the layout of jpeg_error_mgr -- restated below field by field.  Two guards make a mismatch a clean refusal
// (VFSMS_ERR_UNSUPPORTED -> the host falls back to Pillow) instead of a wrong image: the struct SIZE is taken from the library itself
// (jpeg_CreateDecompress is first called with a wrong size; its JERR_BAD_STRUCT_SIZE error carries the size the library expects), and
// after jpeg_read_header the image size read through these offsets must equal the size this file parses from the SOF marker itself.
#include "common.h"
#include "jpeg_huff_core.h"
#include <dlfcn.h>
#include <setjmp.h>
#include <string.h>
#include <stdlib.h>
#include <atomic>

namespace {

// ---- the ABI, restated ----------------------------------------------------------------------------------------------------------------
struct jerr_abi {                       // struct jpeg_error_mgr
    void (*error_exit)(void *);
    void (*emit_message)(void *, int);
    void (*output_message)(void *);
    void (*format_message)(void *, char *);
    void (*reset_error_mgr)(void *);
    int msg_code;
    union { int i[8]; char s[80]; } msg_parm;
    int trace_level;
    long num_warnings;
    const char *const *jpeg_message_table;
    int last_jpeg_message;
    const char *const *addon_message_table;
    int first_addon_message, last_addon_message;
};
struct jdec_head_abi {                  // struct jpeg_decompress_struct, its public head (all that is touched here)
    jerr_abi *err; void *mem; void *progress; void *client_data; int is_decompressor; int global_state;      // jpeg_common_fields
    void *src;
    unsigned image_width, image_height; int num_components; int jpeg_color_space;
    int out_color_space; unsigned scale_num, scale_denom;
    double output_gamma;
    int buffered_image, raw_data_out, dct_method, do_fancy_upsampling, do_block_smoothing;
    int quantize_colors, dither_mode, two_pass_quantize, desired_number_of_colors, enable_1pass_quant, enable_external_quant, enable_2pass_quant;
    unsigned output_width, output_height; int out_color_components, output_components, rec_outbuf_height;
    int actual_number_of_colors; void *colormap;
    unsigned output_scanline;
};
static_assert(offsetof(jdec_head_abi, image_width) == 48 && offsetof(jdec_head_abi, out_color_space) == 64 && offsetof(jdec_head_abi, output_gamma) == 80 &&
              offsetof(jdec_head_abi, output_width) == 136 && offsetof(jdec_head_abi, output_components) == 148 && offsetof(jdec_head_abi, output_scanline) == 168,
              "jpeg_decompress_struct head: unexpected layout");
static_assert(offsetof(jerr_abi, msg_parm) == 44 && offsetof(jerr_abi, num_warnings) == 128 && sizeof(jerr_abi) == 168, "jpeg_error_mgr: unexpected layout");
struct jcomp_head_abi {                 // struct jpeg_compress_struct, its public head
    jerr_abi *err; void *mem; void *progress; void *client_data; int is_decompressor; int global_state;
    void *dest;
    unsigned image_width, image_height; int input_components; int in_color_space;
    double input_gamma;
};
static_assert(offsetof(jcomp_head_abi, image_width) == 48 && offsetof(jcomp_head_abi, in_color_space) == 60, "jpeg_compress_struct head: unexpected layout");
enum { JCS_GRAYSCALE_ = 1, JCS_RGB_ = 2, JCS_YCbCr_ = 3 };
#define JPEG_ABI_VERSION 80
#define JPEG_CINFO_BYTES 2048           // room for the whole struct (the library reports its size: 656 bytes in libjpeg-turbo 2.1, ABI 8)

struct JpegApi {
    jerr_abi *(*std_error)(jerr_abi *);
    void (*create)(void *, int, size_t);
    void (*mem_src)(void *, const unsigned char *, unsigned long);
    int (*read_header)(void *, int);
    int (*start)(void *);
    unsigned (*read_scanlines)(void *, unsigned char **, unsigned);
    unsigned (*read_raw)(void *, unsigned char ***, unsigned);          // jpeg_read_raw_data (may be absent: the raw 4:2:0 path is then off)
    void **(*read_coef)(void *);                                        // jpeg_read_coefficients (may be absent: the coefficient path is then off)
    int (*finish)(void *);
    void (*destroy)(void *);
    size_t cinfo_size;                  // as the library reports it
    bool ok;
    // the compressor
    void (*c_create)(void *, int, size_t);
    void (*c_mem_dest)(void *, unsigned char **, unsigned long *);
    void (*c_defaults)(void *);
    void (*c_quality)(void *, int, int);
    void (*c_start)(void *, int);
    unsigned (*c_write)(void *, unsigned char **, unsigned);
    void (*c_finish)(void *);
    void (*c_destroy)(void *);
    size_t c_size;
    bool c_ok;
};
struct Guard { jmp_buf jb; int code; int parm0, parm1; char text[200]; };

void on_error(void *cinfo)                 // (compressor or decompressor: err and client_data are jpeg_common_fields of both)
{
    jdec_head_abi *c = (jdec_head_abi *)cinfo;
    Guard *g = (Guard *)c->client_data;
    g->code = c->err->msg_code; g->parm0 = c->err->msg_parm.i[0]; g->parm1 = c->err->msg_parm.i[1];
    g->text[0] = 0;
    if (c->err->format_message) { char buf[256]; buf[0] = 0; c->err->format_message(cinfo, buf); strncpy(g->text, buf, sizeof(g->text) - 1); g->text[sizeof(g->text) - 1] = 0; }
    longjmp(g->jb, 1);
}
void on_message(void *) {}              // warnings (e.g. "extraneous bytes before marker") are not printed

const JpegApi &api()
{
    static JpegApi A = [] {
        JpegApi a; memset(&a, 0, sizeof(a));
        void *h = dlopen("libjpeg.so.8", RTLD_NOW | RTLD_LOCAL);
        if (!h) return a;
        a.std_error = (jerr_abi * (*)(jerr_abi *)) dlsym(h, "jpeg_std_error");
        a.create = (void (*)(void *, int, size_t))dlsym(h, "jpeg_CreateDecompress");
        a.mem_src = (void (*)(void *, const unsigned char *, unsigned long))dlsym(h, "jpeg_mem_src");
        a.read_header = (int (*)(void *, int))dlsym(h, "jpeg_read_header");
        a.start = (int (*)(void *))dlsym(h, "jpeg_start_decompress");
        a.read_scanlines = (unsigned (*)(void *, unsigned char **, unsigned))dlsym(h, "jpeg_read_scanlines");
        a.read_raw = (unsigned (*)(void *, unsigned char ***, unsigned))dlsym(h, "jpeg_read_raw_data");
        a.read_coef = (void **(*)(void *))dlsym(h, "jpeg_read_coefficients");
        a.finish = (int (*)(void *))dlsym(h, "jpeg_finish_decompress");
        a.destroy = (void (*)(void *))dlsym(h, "jpeg_destroy_decompress");
        if (!a.std_error || !a.create || !a.mem_src || !a.read_header || !a.start || !a.read_scanlines || !a.finish || !a.destroy) return a;
        // the struct size, from the library: a create call with a size no struct has fails with JERR_BAD_STRUCT_SIZE(library's, caller's)
        alignas(16) unsigned char cinfo[JPEG_CINFO_BYTES]; memset(cinfo, 0, sizeof(cinfo));
        jerr_abi err; memset(&err, 0, sizeof(err));
        Guard g; memset(&g.code, 0, sizeof(g) - offsetof(Guard, code));
        jdec_head_abi *c = (jdec_head_abi *)cinfo;
        c->err = a.std_error(&err);
        err.error_exit = on_error; err.output_message = on_message;
        c->client_data = &g;
        if (setjmp(g.jb) == 0) { a.create(cinfo, JPEG_ABI_VERSION, 7); return a; }       // (a size of 7 cannot be right: the error branch is the expected one)
        if (g.parm1 != 7 || g.parm0 < (int)sizeof(jdec_head_abi) || g.parm0 > JPEG_CINFO_BYTES) return a;    // not the size error, or an implausible size
        a.cinfo_size = (size_t)g.parm0;
        a.ok = true;
        a.c_create = (void (*)(void *, int, size_t))dlsym(h, "jpeg_CreateCompress");
        a.c_mem_dest = (void (*)(void *, unsigned char **, unsigned long *))dlsym(h, "jpeg_mem_dest");
        a.c_defaults = (void (*)(void *))dlsym(h, "jpeg_set_defaults");
        a.c_quality = (void (*)(void *, int, int))dlsym(h, "jpeg_set_quality");
        a.c_start = (void (*)(void *, int))dlsym(h, "jpeg_start_compress");
        a.c_write = (unsigned (*)(void *, unsigned char **, unsigned))dlsym(h, "jpeg_write_scanlines");
        a.c_finish = (void (*)(void *))dlsym(h, "jpeg_finish_compress");
        a.c_destroy = (void (*)(void *))dlsym(h, "jpeg_destroy_compress");
        if (!a.c_create || !a.c_mem_dest || !a.c_defaults || !a.c_quality || !a.c_start || !a.c_write || !a.c_finish || !a.c_destroy) return a;
        memset(cinfo, 0, sizeof(cinfo)); memset(&err, 0, sizeof(err)); memset(&g.code, 0, sizeof(g) - offsetof(Guard, code));
        c->err = a.std_error(&err);
        err.error_exit = on_error; err.output_message = on_message;
        c->client_data = &g;
        if (setjmp(g.jb) == 0) { a.c_create(cinfo, JPEG_ABI_VERSION, 7); return a; }
        if (g.parm1 != 7 || g.parm0 < (int)sizeof(jcomp_head_abi) || g.parm0 > JPEG_CINFO_BYTES) return a;
        a.c_size = (size_t)g.parm0;
        a.c_ok = true;
        return a;
    }();
    return A;
}

// zig-zag position -> natural (row-major) position of a coefficient
const uint8_t kZigzag[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                             35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// (rows, cols, components) from the first SOFn marker: the independent witness for the struct offsets
bool sof_size(const unsigned char *p, size_t n, int *h, int *w, int *nc, int *samp = nullptr)
{
    if (n < 4 || p[0] != 0xFF || p[1] != 0xD8) return false;
    size_t q = 2;
    while (q + 9 < n) {
        if (p[q] != 0xFF) return false;
        const unsigned m = p[q + 1];
        if (m == 0xFF) { q++; continue; }
        if ((m >= 0xD0 && m <= 0xD9) || m == 0x01) { q += 2; continue; }
        const size_t seg = ((size_t)p[q + 2] << 8) | p[q + 3];
        if (m >= 0xC0 && m <= 0xCF && m != 0xC4 && m != 0xC8 && m != 0xCC) {
            *h = (p[q + 5] << 8) | p[q + 6]; *w = (p[q + 7] << 8) | p[q + 8]; *nc = p[q + 9];
            if (samp) {                                       // (H << 4 | V) of up to three components
                samp[0] = samp[1] = samp[2] = 0;
                for (int k = 0; k < *nc && k < 3 && q + 10 + 3 * k + 2 < n; k++) samp[k] = p[q + 10 + 3 * k + 1];
            }
            return *h > 0 && *w > 0;
        }
        q += 2 + seg;
    }
    return false;
}

}  // namespace

// Decode `jpeg` into `out` (rows of *w_out * (*comp_out) bytes, densely packed).  want_planes != 0 and a 3-component YCbCr file: the Y Cb Cr
// planes interleaved (comp 3); otherwise the grayscale decode (comp 1).  Returns VFSMS_ERR_UNSUPPORTED when the library or the file is
// not one this path handles (the caller decodes some other way), VFSMS_ERR_CAPACITY when `cap` is too small (h, w, comp are set).
int jpeg_decode_host(const unsigned char *jpeg, size_t nbytes, int want_planes, unsigned char *out, size_t cap, int *h_out, int *w_out, int *comp_out)
{
    const JpegApi &A = api();
    if (!A.ok) { vfsms_set_error("jpeg: libjpeg.so.8 (ABI 8) is not available on this host"); return VFSMS_ERR_UNSUPPORTED; }
    int sh = 0, sw = 0, snc = 0;
    if (!jpeg || !sof_size(jpeg, nbytes, &sh, &sw, &snc) || (snc != 1 && snc != 3)) { vfsms_set_error("jpeg: not a 1- or 3-component JPEG"); return VFSMS_ERR_UNSUPPORTED; }
    alignas(16) unsigned char cinfo[JPEG_CINFO_BYTES]; memset(cinfo, 0, sizeof(cinfo));
    jerr_abi err; memset(&err, 0, sizeof(err));
    Guard g; memset(&g.code, 0, sizeof(g) - offsetof(Guard, code));
    jdec_head_abi *c = (jdec_head_abi *)cinfo;
    volatile bool created = false;
    if (setjmp(g.jb)) {
        if (created) A.destroy(cinfo);
        vfsms_set_error("jpeg: %s", g.text[0] ? g.text : "decode error");
        return VFSMS_ERR_BAD_ARG;                            // a damaged file: an error of the input, not of the path
    }
    c->err = A.std_error(&err);
    err.error_exit = on_error; err.output_message = on_message;
    c->client_data = &g;
    A.create(cinfo, JPEG_ABI_VERSION, A.cinfo_size);
    created = true;
    c->client_data = &g;                                     // (create zeroes the struct but for err and client_data; set again to be sure)
    A.mem_src(cinfo, jpeg, (unsigned long)nbytes);
    A.read_header(cinfo, 1);
    if ((int)c->image_height != sh || (int)c->image_width != sw || c->num_components != snc) {      // the offsets are not this library's
        A.destroy(cinfo);
        vfsms_set_error("jpeg: libjpeg.so.8 does not have the expected struct layout");
        return VFSMS_ERR_UNSUPPORTED;
    }
    const bool planes = want_planes && snc == 3 && c->jpeg_color_space == JCS_YCbCr_;
    if (want_planes && snc == 3 && !planes) {                // an RGB / Adobe-transform-0 file has no Y Cb Cr planes: let the caller decode it
        A.destroy(cinfo);
        vfsms_set_error("jpeg: 3-component file that is not YCbCr");
        return VFSMS_ERR_UNSUPPORTED;
    }
    c->out_color_space = planes ? JCS_YCbCr_ : JCS_GRAYSCALE_;
    const int comp = planes ? 3 : 1;
    *h_out = sh; *w_out = sw; *comp_out = comp;
    if (!out || cap < (size_t)sh * sw * comp) { A.destroy(cinfo); vfsms_set_error("jpeg: output buffer too small"); return VFSMS_ERR_CAPACITY; }
    A.start(cinfo);
    if ((int)c->output_width != sw || (int)c->output_height != sh || c->output_components != comp) {
        A.destroy(cinfo);
        vfsms_set_error("jpeg: unexpected output geometry");
        return VFSMS_ERR_UNSUPPORTED;
    }
    const size_t pitch = (size_t)sw * comp;
    while (c->output_scanline < c->output_height) {
        unsigned char *rows[16];
        const unsigned y0 = c->output_scanline;
        const unsigned nr = c->output_height - y0 < 16 ? c->output_height - y0 : 16;
        for (unsigned r = 0; r < nr; r++) rows[r] = out + (size_t)(y0 + r) * pitch;
        if (A.read_scanlines(cinfo, rows, nr) == 0) break;
    }
    const bool complete = c->output_scanline == c->output_height;
    A.finish(cinfo);
    const long warnings = err.num_warnings;                  // e.g. "premature end of data segment": libjpeg pads a truncated file with gray
    A.destroy(cinfo);
    if (!complete || warnings) { vfsms_set_error("jpeg: truncated or damaged file (%ld decoder warnings)", warnings); return VFSMS_ERR_BAD_ARG; }
    return VFSMS_OK;
}

// Round 6: the DOWNSAMPLED planes of a 4:2:0 Y Cb Cr file (jpeg_read_raw_data: entropy decode + IDCT on the host, nothing else) --
// chroma upsampling and the colour conversion run on the device (csrc/ingest_kernels.hip: k_ingest_420, libjpeg's h2v2 "fancy" triangle
// filter restated).  The host writes 1.5 bytes per pixel into pinned staging instead of 3 and skips its upsampling and interleaving passes.
// out: Y plane, pitch pw = w rounded up to 16, ph = h rounded up to 16 rows (the iMCU grid: the rows / columns beyond the image hold the
// decoder's edge padding and are never looked at), then the Cb plane (pitch pw / 2, ph / 2 rows), then Cr.  VFSMS_ERR_UNSUPPORTED: not a
// 3-component Y Cb Cr file sampled 2x2, 1x1, 1x1, or no jpeg_read_raw_data in the library -- the caller takes the full decode.
int jpeg_decode_raw420_host(const unsigned char *jpeg, size_t nbytes, unsigned char *out, size_t cap, int *h_out, int *w_out)
{
    const JpegApi &A = api();
    if (!A.ok || !A.read_raw) { vfsms_set_error("jpeg: no raw-data decode on this host"); return VFSMS_ERR_UNSUPPORTED; }
    int sh = 0, sw = 0, snc = 0, samp[3] = {0, 0, 0};
    // sw < 5: jdsample.c takes h2v2_fancy_upsample only when do_fancy_upsampling && compptr->downsampled_width > 2; a file of 3 or 4 columns
    // (2 chroma columns) gets h2v2_upsample, plain replication, which k_ingest_420 does not restate -- the full decode takes those files
    if (!jpeg || !sof_size(jpeg, nbytes, &sh, &sw, &snc, samp) || snc != 3 || samp[0] != 0x22 || samp[1] != 0x11 || samp[2] != 0x11 || sw < 5 || sh < 2) {
        vfsms_set_error("jpeg: not a 4:2:0 Y Cb Cr file"); return VFSMS_ERR_UNSUPPORTED;
    }
    const size_t pw = ((size_t)sw + 15) & ~(size_t)15, ph = ((size_t)sh + 15) & ~(size_t)15;
    *h_out = sh; *w_out = sw;
    if (!out || cap < pw * ph * 3 / 2) { vfsms_set_error("jpeg: output buffer too small"); return VFSMS_ERR_CAPACITY; }
    alignas(16) unsigned char cinfo[JPEG_CINFO_BYTES]; memset(cinfo, 0, sizeof(cinfo));
    jerr_abi err; memset(&err, 0, sizeof(err));
    Guard g; memset(&g.code, 0, sizeof(g) - offsetof(Guard, code));
    jdec_head_abi *c = (jdec_head_abi *)cinfo;
    volatile bool created = false;
    if (setjmp(g.jb)) {
        if (created) A.destroy(cinfo);
        vfsms_set_error("jpeg: %s", g.text[0] ? g.text : "decode error");
        return VFSMS_ERR_BAD_ARG;
    }
    c->err = A.std_error(&err);
    err.error_exit = on_error; err.output_message = on_message;
    c->client_data = &g;
    A.create(cinfo, JPEG_ABI_VERSION, A.cinfo_size);
    created = true;
    c->client_data = &g;
    A.mem_src(cinfo, jpeg, (unsigned long)nbytes);
    A.read_header(cinfo, 1);
    if ((int)c->image_height != sh || (int)c->image_width != sw || c->num_components != 3 || c->jpeg_color_space != JCS_YCbCr_) {
        A.destroy(cinfo);
        vfsms_set_error("jpeg: not a Y Cb Cr file (or an unexpected struct layout)");
        return VFSMS_ERR_UNSUPPORTED;
    }
    c->out_color_space = JCS_YCbCr_;
    c->raw_data_out = 1;
    A.start(cinfo);
    if ((int)c->output_width != sw || (int)c->output_height != sh) { A.destroy(cinfo); vfsms_set_error("jpeg: unexpected output geometry"); return VFSMS_ERR_UNSUPPORTED; }
    unsigned char *Y = out, *Cb = out + pw * ph, *Cr = Cb + (pw / 2) * (ph / 2);
    bool ok = true;
    while (c->output_scanline < c->output_height) {
        const unsigned y0 = c->output_scanline;                  // a multiple of 16: one iMCU row per call
        if (y0 % 16 || y0 + 16 > ph) { ok = false; break; }
        unsigned char *yr[16], *br[8], *rr[8];
        for (unsigned r = 0; r < 16; r++) yr[r] = Y + (size_t)(y0 + r) * pw;
        for (unsigned r = 0; r < 8; r++) { br[r] = Cb + (size_t)(y0 / 2 + r) * (pw / 2); rr[r] = Cr + (size_t)(y0 / 2 + r) * (pw / 2); }
        unsigned char **planes[3] = { yr, br, rr };
        if (A.read_raw(cinfo, planes, 16) == 0) { ok = false; break; }
    }
    const bool complete = ok && c->output_scanline >= c->output_height;
    if (complete) A.finish(cinfo);
    const long warnings = err.num_warnings;
    A.destroy(cinfo);
    if (!complete || warnings) { vfsms_set_error("jpeg: truncated or damaged file (%ld decoder warnings)", warnings); return VFSMS_ERR_BAD_ARG; }
    return VFSMS_OK;
}

// host-only entry (no context, no GPU): the decode of jpeg_decode_host, for tests and for callers that want the planes themselves
extern "C" int vfsms_jpeg_decode(const uint8_t *jpeg, size_t nbytes, int want_planes, uint8_t *out, size_t cap, int *h, int *w, int *comp)
{
    if (!h || !w || !comp) { vfsms_set_error("jpeg_decode: bad arguments"); return VFSMS_ERR_BAD_ARG; }
    if (want_planes == 2) {                                  // the raw 4:2:0 planes (comp = 420): Y | Cb | Cr on the iMCU grid, see jpeg_decode_raw420_host
        *comp = 420;
        return jpeg_decode_raw420_host(jpeg, nbytes, out, cap, h, w);
    }
    return jpeg_decode_host(jpeg, nbytes, want_planes, out, cap, h, w, comp);
}

// ---- the host half of Method.jpegDecoder = "device" (jpeg_dec_kernels.hip; specified by tests/jpeg_dec_ref.py) --------------------------
// More ABI knowledge: struct jpeg_memory_mgr opens with its method pointers -- alloc_small, alloc_large, alloc_sarray, alloc_barray,
// request_virt_sarray, request_virt_barray, realize_virt_arrays, access_virt_sarray, access_virt_barray -- a layout that has not changed from
// libjpeg 6b to libjpeg-turbo 3.  The ninth is the only way to the coefficient arrays of jpeg_read_coefficients:
//     JBLOCKARRAY access_virt_barray(cinfo, jvirt_barray_ptr, start_row, num_rows, writable)         num_rows <= the component's v_samp_factor
// The guard against a library laid out otherwise: the pointer read from that slot must lie in the same loaded object as
// jpeg_read_coefficients (dladdr), else the path is refused before anything is called through it.
namespace {
struct FrameInfo {
    int precision, h, w, nc, progressive;
    int hs[4], vs[4], tq[4];
    bool have[4];                       // quantisation table slot defined in front of the first scan
    uint16_t q[4][64];                  // natural order
    size_t sos;                         // where the first scan header starts
};
// SOI .. the first SOS: the frame header and every DQT segment (8- and 16-bit entries, zig-zag order in the file)
bool parse_frame(const unsigned char *p, size_t n, FrameInfo *f)
{
    memset(f, 0, sizeof(*f));
    if (n < 4 || p[0] != 0xFF || p[1] != 0xD8) return false;
    size_t q = 2; bool sof = false;
    while (q + 4 <= n) {
        if (p[q] != 0xFF) return false;
        const unsigned m = p[q + 1];
        if (m == 0xFF) { q++; continue; }
        if ((m >= 0xD0 && m <= 0xD9) || m == 0x01) { q += 2; continue; }
        const size_t seg = ((size_t)p[q + 2] << 8) | p[q + 3];
        if (seg < 2 || q + 2 + seg > n) return false;
        if (m == 0xDA) { f->sos = q; return sof; }
        if (m == 0xDB) {
            size_t s = q + 4; const size_t end = q + 2 + seg;
            while (s < end) {
                const int pq = p[s] >> 4, t = p[s] & 15; s++;
                if (t > 3 || pq > 1 || s + (pq ? 128 : 64) > end) return false;
                for (int k = 0; k < 64; k++) {
                    f->q[t][kZigzag[k]] = pq ? (uint16_t)((p[s] << 8) | p[s + 1]) : p[s];
                    s += pq ? 2 : 1;
                }
                f->have[t] = true;
            }
        } else if (m >= 0xC0 && m <= 0xCF && m != 0xC4 && m != 0xC8 && m != 0xCC) {
            if (sof || seg < 8) return false;
            f->precision = p[q + 4]; f->h = (p[q + 5] << 8) | p[q + 6]; f->w = (p[q + 7] << 8) | p[q + 8]; f->nc = p[q + 9];
            f->progressive = m == 0xC2;
            if (m > 0xC2 || f->nc < 1 || f->nc > 4 || seg < 8 + 3u * f->nc) { f->nc = 0; sof = true; q += 2 + seg; continue; }   // (a frame this path does not take: nc = 0)
            for (int k = 0; k < f->nc; k++) { f->hs[k] = p[q + 11 + 3 * k] >> 4; f->vs[k] = p[q + 11 + 3 * k] & 15; f->tq[k] = p[q + 12 + 3 * k]; }
            sof = true;
        }
        q += 2 + seg;
    }
    return false;
}
}  // namespace

// The quantised DCT coefficients of a file, for the device's inverse transform.  `out` (the staging layout, include/vfsms.h): one uint16[64]
// table per component in natural order, then per component its blocks in block-row-major order, 64 int16 each in natural order, on the grid
// grid6 = (block rows, block columns) per component: ceil(h * v / (vmax * 8)) rounded up to a multiple of v by ceil(w * hs / (hmax * 8))
// rounded up to a multiple of hs -- whole iMCUs.  luma_only: the blocks of component 0 alone (every table still).  *need: the bytes written,
// also on VFSMS_ERR_CAPACITY (h, w, ncomp, grid6 are set then too).  Taken: 8-bit baseline / extended / progressive Huffman files of one
// component, or of three (Y Cb Cr) sampled 2x2, 1x1, 1x1 with w >= 5 and h >= 2 -- the raw 4:2:0 path's condition, for its reason (k_ingest_420
// follows).  VFSMS_ERR_UNSUPPORTED for anything else, VFSMS_ERR_BAD_ARG for a damaged file (any decoder warning).
int jpeg_coefficients_host(const unsigned char *jpeg, size_t nbytes, int luma_only, unsigned char *out, size_t cap, int *h_out, int *w_out, int *ncomp,
                           int *grid6, size_t *need_out)
{
    const JpegApi &A = api();
    if (!A.ok || !A.read_coef) { vfsms_set_error("jpeg: no coefficient decode on this host"); return VFSMS_ERR_UNSUPPORTED; }
    FrameInfo F;
    if (!jpeg || !parse_frame(jpeg, nbytes, &F) || F.h <= 0 || F.w <= 0 || F.precision != 8 || (F.nc != 1 && F.nc != 3)) {
        vfsms_set_error("jpeg: not an 8-bit 1- or 3-component Huffman JPEG"); return VFSMS_ERR_UNSUPPORTED;
    }
    if (F.nc == 3 && (F.hs[0] != 2 || F.vs[0] != 2 || F.hs[1] != 1 || F.vs[1] != 1 || F.hs[2] != 1 || F.vs[2] != 1 || F.w < 5 || F.h < 2)) {
        vfsms_set_error("jpeg: not a 4:2:0 Y Cb Cr file"); return VFSMS_ERR_UNSUPPORTED;
    }
    // (a lone component's sampling factors only pad its grid: up to 2 the padded grid stays within the 16 x 16 iMCUs the callers size staging for)
    if (F.nc == 1 && (F.hs[0] < 1 || F.hs[0] > 2 || F.vs[0] < 1 || F.vs[0] > 2)) { vfsms_set_error("jpeg: sampling factors beyond 2"); return VFSMS_ERR_UNSUPPORTED; }
    for (int k = 0; k < F.nc; k++)
        if (F.tq[k] > 3 || !F.have[F.tq[k]]) { vfsms_set_error("jpeg: a quantisation table is not defined in front of the first scan"); return VFSMS_ERR_UNSUPPORTED; }
    // a table redefined between two scans would apply to the components that start later: the tables above would not be theirs.  In
    // entropy-coded data FF is followed by 00 or RSTn only, so FF DB behind the first scan header is such a segment: the full decode takes it
    for (const unsigned char *s = jpeg + F.sos, *e = jpeg + nbytes - 1; s < e && (s = (const unsigned char *)memchr(s, 0xFF, (size_t)(e - s))) != nullptr; s++)
        if (s[1] == 0xDB) { vfsms_set_error("jpeg: quantisation tables redefined between scans"); return VFSMS_ERR_UNSUPPORTED; }
    const int hmax = F.hs[0], vmax = F.vs[0];                    // (one component, or 2x2 in front of 1x1, 1x1: component 0 holds the maxima)
    size_t need = (size_t)F.nc * VFSMS_JPEG_COEF_TABLE_BYTES;
    const int ncopy = luma_only ? 1 : F.nc;
    for (int k = 0; k < F.nc; k++) {
        const long long br = ((long long)F.h * F.vs[k] + vmax * 8 - 1) / (vmax * 8), bc = ((long long)F.w * F.hs[k] + hmax * 8 - 1) / (hmax * 8);
        grid6[2 * k] = (int)((br + F.vs[k] - 1) / F.vs[k] * F.vs[k]); grid6[2 * k + 1] = (int)((bc + F.hs[k] - 1) / F.hs[k] * F.hs[k]);
        if (k < ncopy) need += (size_t)grid6[2 * k] * grid6[2 * k + 1] * 128;
    }
    *h_out = F.h; *w_out = F.w; *ncomp = F.nc; *need_out = need;
    if (!out || cap < need) { vfsms_set_error("jpeg: output buffer too small"); return VFSMS_ERR_CAPACITY; }
    alignas(16) unsigned char cinfo[JPEG_CINFO_BYTES]; memset(cinfo, 0, sizeof(cinfo));
    jerr_abi err; memset(&err, 0, sizeof(err));
    Guard g; memset(&g.code, 0, sizeof(g) - offsetof(Guard, code));
    jdec_head_abi *c = (jdec_head_abi *)cinfo;
    volatile bool created = false;
    if (setjmp(g.jb)) {
        if (created) A.destroy(cinfo);
        vfsms_set_error("jpeg: %s", g.text[0] ? g.text : "decode error");
        return VFSMS_ERR_BAD_ARG;
    }
    c->err = A.std_error(&err);
    err.error_exit = on_error; err.output_message = on_message;
    c->client_data = &g;
    A.create(cinfo, JPEG_ABI_VERSION, A.cinfo_size);
    created = true;
    c->client_data = &g;
    A.mem_src(cinfo, jpeg, (unsigned long)nbytes);
    A.read_header(cinfo, 1);
    if ((int)c->image_height != F.h || (int)c->image_width != F.w || c->num_components != F.nc || c->jpeg_color_space != (F.nc == 3 ? JCS_YCbCr_ : JCS_GRAYSCALE_)) {
        A.destroy(cinfo);
        vfsms_set_error("jpeg: not a gray / Y Cb Cr file (or an unexpected struct layout)");
        return VFSMS_ERR_UNSUPPORTED;
    }
    typedef short (**barray_rows)[64];
    typedef barray_rows (*access_fn)(void *, void *, unsigned, unsigned, int);
    const access_fn access = c->mem ? (access_fn)((void **)c->mem)[8] : nullptr;
    Dl_info da, db;
    if (!access || !dladdr((void *)access, &da) || !dladdr((void *)A.read_coef, &db) || da.dli_fbase != db.dli_fbase) {
        A.destroy(cinfo);
        vfsms_set_error("jpeg: libjpeg.so.8 does not have the expected memory manager layout");
        return VFSMS_ERR_UNSUPPORTED;
    }
    void **arrays = A.read_coef(cinfo);
    if (!arrays) { A.destroy(cinfo); vfsms_set_error("jpeg: no coefficient arrays"); return VFSMS_ERR_BAD_ARG; }      // (suspension: cannot happen with a memory source)
    for (int k = 0; k < F.nc; k++) memcpy(out + (size_t)k * VFSMS_JPEG_COEF_TABLE_BYTES, F.q[F.tq[k]], VFSMS_JPEG_COEF_TABLE_BYTES);
    unsigned char *o = out + (size_t)F.nc * VFSMS_JPEG_COEF_TABLE_BYTES;
    for (int k = 0; k < ncopy; k++) {
        const size_t row_bytes = (size_t)grid6[2 * k + 1] * 128;
        for (int r0 = 0; r0 < grid6[2 * k]; r0 += F.vs[k]) {                                   // one iMCU row of the component per access
            barray_rows rows = access(cinfo, arrays[k], (unsigned)r0, (unsigned)F.vs[k], 0);
            for (int r = 0; r < F.vs[k]; r++) { memcpy(o, rows[r], row_bytes); o += row_bytes; }
        }
    }
    A.finish(cinfo);
    const long warnings = err.num_warnings;
    A.destroy(cinfo);
    if (warnings) { vfsms_set_error("jpeg: truncated or damaged file (%ld decoder warnings)", warnings); return VFSMS_ERR_BAD_ARG; }
    return VFSMS_OK;
}

// host-only entry (no context, no GPU), beside vfsms_jpeg_decode: the staging layout into the caller's memory
extern "C" int vfsms_jpeg_coefficients(const uint8_t *jpeg, size_t nbytes, uint8_t *out, size_t cap, int *h, int *w, int *ncomp, int *grid6, size_t *need)
{
    if (!h || !w || !ncomp || !grid6 || !need) { vfsms_set_error("jpeg_coefficients: bad arguments"); return VFSMS_ERR_BAD_ARG; }
    return jpeg_coefficients_host(jpeg, nbytes, 0, out, cap, h, w, ncomp, grid6, need);
}

// ---- the host half of Method.jpegDecoder = "device-entropy" (jpeg_huff_kernels.hip; specified by tests/jpeg_huff_ref.py: parse) ------------
// No libjpeg here and no GPU: the file is read once for its markers.  SOI .. SOS give the frame, the quantisation tables, the Huffman tables
// (built into their decoding form by jh_build_table) and the restart interval; the entropy-coded data behind the scan header is copied with
// its FF 00 stuffing removed, cut at the RSTn markers into segments that each start on a dword and are padded with FF to one, up to EOI.
// UNSUPPORTED: a file the device decoder does not take.  BAD_ARG: one it would take, damaged.
namespace {
struct ScanFrame {
    int precision, h, w, nc, ri;
    int cid[3], hs[3], vs[3], tq[3], td[3], ta[3];
    bool haveq[4], haveh[2][4];
    uint16_t q[4][64];                  // natural order
    uint8_t hcounts[2][4][16], hvals[2][4][256];
    size_t data;                        // the first byte behind the scan header
};
int scan_refuse(int rc, const char *what) { vfsms_set_error("jpeg_scan: %s", what); return rc; }
#define SCAN_UNSUPPORTED(what) return scan_refuse(VFSMS_ERR_UNSUPPORTED, what)
#define SCAN_DAMAGED(what) return scan_refuse(VFSMS_ERR_BAD_ARG, what)
int scan_headers(const unsigned char *p, size_t n, ScanFrame *F)
{
    memset(F, 0, sizeof(*F));
    if (n < 4 || p[0] != 0xFF || p[1] != 0xD8) SCAN_UNSUPPORTED("no SOI");
    size_t q = 2; bool sof = false; int nc_frame = 0;
    const unsigned char *seg = nullptr; size_t len = 0;
    for (;;) {
        if (q + 4 > n) SCAN_DAMAGED("no scan");
        if (p[q] != 0xFF) SCAN_DAMAGED("marker expected");
        const unsigned m = p[q + 1];
        if (m == 0xFF) { q++; continue; }
        if ((m >= 0xD0 && m <= 0xD7) || m == 0x01) { q += 2; continue; }
        if (m == 0xD8 || m == 0xD9) SCAN_DAMAGED("SOI / EOI in front of the scan");
        const size_t sl = ((size_t)p[q + 2] << 8) | p[q + 3];
        if (sl < 2 || q + 2 + sl > n) SCAN_DAMAGED("segment beyond the file");
        seg = p + q + 4; len = sl - 2;
        if (m == 0xDB) {
            size_t s = 0;
            while (s < len) {
                const int pq = seg[s] >> 4, t = seg[s] & 15; s++;
                if (pq > 1 || t > 3 || s + (pq ? 128 : 64) > len) SCAN_DAMAGED("DQT");
                for (int k = 0; k < 64; k++) { F->q[t][kZigzag[k]] = pq ? (uint16_t)((seg[s] << 8) | seg[s + 1]) : seg[s]; s += pq ? 2 : 1; }
                F->haveq[t] = true;
            }
        } else if (m == 0xC4) {
            size_t s = 0;
            while (s < len) {
                if (s + 17 > len) SCAN_DAMAGED("DHT");
                const int tc = seg[s] >> 4, th = seg[s] & 15;
                size_t nv = 0;
                for (int k = 0; k < 16; k++) nv += seg[s + 1 + k];
                if (tc > 1 || th > 3 || nv > 256 || s + 17 + nv > len) SCAN_DAMAGED("DHT");
                JpegHuffTable T;
                bool ok = jh_build_table(seg + s + 1, seg + s + 17, &T);
                for (size_t k = 0; ok && tc == 0 && k < nv; k++) ok = seg[s + 17 + k] <= 15;
                if (!ok) SCAN_DAMAGED("DHT: no prefix code");
                memcpy(F->hcounts[tc][th], seg + s + 1, 16);
                memset(F->hvals[tc][th], 0, 256); memcpy(F->hvals[tc][th], seg + s + 17, nv);
                F->haveh[tc][th] = true;
                s += 17 + nv;
            }
        } else if (m == 0xDD) {
            if (sl != 4) SCAN_DAMAGED("DRI");
            F->ri = (seg[0] << 8) | seg[1];
        } else if (m >= 0xC0 && m <= 0xCF && m != 0xC4 && m != 0xC8 && m != 0xCC) {
            if (sof) SCAN_UNSUPPORTED("two frames");
            if (m > 0xC1) SCAN_UNSUPPORTED("not a baseline / extended sequential Huffman file");
            if (sl < 8 || sl != 8 + 3u * seg[5]) SCAN_DAMAGED("SOF");
            F->precision = seg[0]; F->h = (seg[1] << 8) | seg[2]; F->w = (seg[3] << 8) | seg[4]; nc_frame = seg[5];
            for (int k = 0; k < nc_frame && k < 3; k++) { F->cid[k] = seg[6 + 3 * k]; F->hs[k] = seg[7 + 3 * k] >> 4; F->vs[k] = seg[7 + 3 * k] & 15; F->tq[k] = seg[8 + 3 * k]; }
            sof = true;
        } else if (m == 0xDA) { q += 2 + sl; break; }
        q += 2 + sl;
    }
    if (!sof) SCAN_DAMAGED("a scan without a frame");
    if (F->precision != 8 || F->h <= 0 || F->w <= 0 || (nc_frame != 1 && nc_frame != 3)) SCAN_UNSUPPORTED("not 8 bits, 1 or 3 components");
    F->nc = nc_frame;
    if (F->nc == 3 && (F->hs[0] != 2 || F->vs[0] != 2 || F->hs[1] != 1 || F->vs[1] != 1 || F->hs[2] != 1 || F->vs[2] != 1 || F->w < 5 || F->h < 2))
        SCAN_UNSUPPORTED("not a 4:2:0 Y Cb Cr file");
    if (F->nc == 1 && (F->hs[0] < 1 || F->hs[0] > 2 || F->vs[0] < 1 || F->vs[0] > 2)) SCAN_UNSUPPORTED("sampling factors beyond 2");
    if (len < 1 || seg[0] != F->nc || len != 4 + 2u * F->nc) SCAN_UNSUPPORTED("several scans");           // (a scan that does not hold every component)
    for (int k = 0; k < F->nc; k++) {
        if (seg[1 + 2 * k] != F->cid[k]) SCAN_UNSUPPORTED("scan components out of frame order");
        F->td[k] = seg[2 + 2 * k] >> 4; F->ta[k] = seg[2 + 2 * k] & 15;
        if (F->tq[k] > 3 || !F->haveq[F->tq[k]] || F->td[k] > 3 || F->ta[k] > 3 || !F->haveh[0][F->td[k]] || !F->haveh[1][F->ta[k]])
            SCAN_UNSUPPORTED("a table is not defined in front of the scan");
    }
    if (seg[1 + 2 * F->nc] != 0 || seg[2 + 2 * F->nc] != 63 || seg[3 + 2 * F->nc] != 0) SCAN_UNSUPPORTED("not a sequential scan");
    F->data = q;
    return VFSMS_OK;
}
size_t scan_align(size_t v) { return (v + 15) & ~(size_t)15; }
}  // namespace

// The scan record of a file (csrc/jpeg_huff_core.h: JpegScanHeader and what its offsets name) into `out`.  *need: with VFSMS_OK the bytes
// written; with VFSMS_ERR_CAPACITY (out == NULL asks) a bound on them that holds for this file, from its headers and its size alone.
int jpeg_scan_host(const unsigned char *jpeg, size_t nbytes, int sub_bits, unsigned char *out, size_t cap, size_t *need)
{
    if (!jpeg || !need || sub_bits < 64 || sub_bits > (1 << 20) || (sub_bits & 31)) { vfsms_set_error("jpeg_scan: bad arguments"); return VFSMS_ERR_BAD_ARG; }
    if (nbytes > ((size_t)1 << 28)) SCAN_UNSUPPORTED("a file beyond 256 MiB");                            // (bit positions stay below 2^31)
    ScanFrame F;
    TRY(scan_headers(jpeg, nbytes, &F));
    JpegScanHeader H; memset(&H, 0, sizeof(H));
    H.h = F.h; H.w = F.w; H.ncomp = F.nc; H.restart_interval = F.ri; H.sub_bits = sub_bits;
    const int hmax = F.hs[0], vmax = F.vs[0];
    for (int k = 0; k < F.nc; k++) {
        const long long br = ((long long)F.h * F.vs[k] + vmax * 8 - 1) / (vmax * 8), bc = ((long long)F.w * F.hs[k] + hmax * 8 - 1) / (hmax * 8);
        H.grid6[2 * k] = (int)((br + F.vs[k] - 1) / F.vs[k] * F.vs[k]); H.grid6[2 * k + 1] = (int)((bc + F.hs[k] - 1) / F.hs[k] * F.hs[k]);
    }
    H.blocks_per_mcu = F.nc == 3 ? 6 : 1;
    H.mcus = F.nc == 3 ? H.grid6[2] * H.grid6[3] : ((F.h + 7) / 8) * ((F.w + 7) / 8);
    const size_t entropy = nbytes - F.data;
    const size_t want = F.ri ? ((size_t)H.mcus + F.ri - 1) / F.ri : 1;
    if (want > entropy + 1) SCAN_DAMAGED("fewer bytes than restart intervals");
    H.nseg = (int)want;
    H.off_quant = (uint32_t)scan_align(sizeof(JpegScanHeader));
    H.off_tables = (uint32_t)scan_align(H.off_quant + (size_t)F.nc * VFSMS_JPEG_COEF_TABLE_BYTES);
    H.off_seg = (uint32_t)scan_align(H.off_tables + 2 * (size_t)F.nc * sizeof(JpegHuffTable));
    H.off_stream = (uint32_t)scan_align(H.off_seg + want * sizeof(JpegHuffSeg));
    const size_t stream_cap = scan_align(entropy + 4 * want + 16);
    const size_t bound = scan_align(H.off_stream + stream_cap) + 4 * (stream_cap * 8 / (size_t)sub_bits + want + 1);
    *need = bound;
    if (!out || cap < bound) { vfsms_set_error("jpeg_scan: output buffer too small"); return VFSMS_ERR_CAPACITY; }
    memset(out, 0, H.off_stream);
    for (int k = 0; k < F.nc; k++) {
        memcpy(out + H.off_quant + (size_t)k * VFSMS_JPEG_COEF_TABLE_BYTES, F.q[F.tq[k]], VFSMS_JPEG_COEF_TABLE_BYTES);
        JpegHuffTable T;
        jh_build_table(F.hcounts[0][F.td[k]], F.hvals[0][F.td[k]], &T); memcpy(out + H.off_tables + (size_t)(2 * k) * sizeof(T), &T, sizeof(T));
        jh_build_table(F.hcounts[1][F.ta[k]], F.hvals[1][F.ta[k]], &T); memcpy(out + H.off_tables + (size_t)(2 * k + 1) * sizeof(T), &T, sizeof(T));
    }
    // the entropy-coded data: FF 00 is the data byte FF, FF RSTn ends a segment, FF FF is fill, any other marker ends the scan
    unsigned char *stream = out + H.off_stream;
    JpegHuffSeg *segs = (JpegHuffSeg *)(out + H.off_seg);
    size_t o = 0, seg_start = 0, nseg = 0, nsub = 0, s = F.data;
    int end_marker = -1;
    auto close_segment = [&]() -> bool {
        if (nseg >= want) return false;
        JpegHuffSeg &S = segs[nseg];
        S.byte_off = (uint32_t)seg_start; S.byte_count = (uint32_t)(o - seg_start); S.first_mcu = (uint32_t)(nseg * (size_t)F.ri); S.sub0 = (uint32_t)nsub;
        const size_t bits = (size_t)S.byte_count * 8;
        nsub += bits ? (bits + sub_bits - 1) / sub_bits : 1;
        while (o & 3) stream[o++] = 0xFF;
        seg_start = o; nseg++;
        return true;
    };
    while (s < nbytes) {
        const unsigned char *f = (const unsigned char *)memchr(jpeg + s, 0xFF, nbytes - s);
        const size_t run = f ? (size_t)(f - (jpeg + s)) : nbytes - s;
        if (o + run + 8 > stream_cap) SCAN_DAMAGED("stream beyond its bound");                           // (cannot happen: the bound counts every byte)
        memcpy(stream + o, jpeg + s, run); o += run; s += run;
        if (!f || s + 1 >= nbytes) break;
        const unsigned m = jpeg[s + 1];
        if (m == 0) { stream[o++] = 0xFF; s += 2; }
        else if (m == 0xFF) s += 1;
        else if (m >= 0xD0 && m <= 0xD7) {
            if (m != 0xD0 + (nseg & 7)) SCAN_DAMAGED("restart markers out of order");
            if (!close_segment()) SCAN_DAMAGED("more restart intervals than the frame holds");
            s += 2;
        } else { end_marker = (int)m; break; }
    }
    if (end_marker < 0) SCAN_DAMAGED("no EOI");
    if (end_marker != 0xD9) SCAN_UNSUPPORTED("several scans, or tables behind SOS");
    if (!close_segment() || nseg != want) SCAN_DAMAGED("the restart intervals do not add up to the frame's MCUs");
    H.stream_bytes = (uint32_t)o; H.nsub = (int)nsub;
    H.off_subseg = (uint32_t)scan_align(H.off_stream + o);
    H.total_bytes = (uint32_t)(H.off_subseg + 4 * nsub);
    if (H.total_bytes > bound) SCAN_DAMAGED("record beyond its bound");                                  // (cannot happen)
    memset(stream + o, 0xFF, H.off_subseg - H.off_stream - o);
    uint32_t *subseg = (uint32_t *)(out + H.off_subseg);
    for (size_t k = 0; k < nseg; k++) {
        const size_t last = k + 1 < nseg ? segs[k + 1].sub0 : nsub;
        for (size_t j = segs[k].sub0; j < last; j++) subseg[j] = (uint32_t)k;
    }
    memcpy(out, &H, sizeof(H));
    *need = H.total_bytes;
    return VFSMS_OK;
}

// host-only entry (no context, no GPU, no libjpeg): the scan record at VFSMS_JPEG_HUFF_SUB_BITS into the caller's memory
extern "C" int vfsms_jpeg_scan(const uint8_t *jpeg, size_t nbytes, uint8_t *out, size_t cap, size_t *need)
{
    return jpeg_scan_host(jpeg, nbytes, VFSMS_JPEG_HUFF_SUB_BITS, out, cap, need);
}

// ---- encode -----------------------------------------------------------------------------------------------------------------------------
namespace {
// the segments of a baseline stream this library wrote: [2, sos_end) = the headers up to and including the SOS header, [sos_end, n - 2) =
// the entropy-coded segment, and where the frame header keeps its size
struct StreamMap { size_t sof, sos, sos_end; int h, w, nc, vmax; };
bool map_stream(const unsigned char *p, size_t n, StreamMap *m)
{
    if (n < 6 || p[0] != 0xFF || p[1] != 0xD8 || p[n - 2] != 0xFF || p[n - 1] != 0xD9) return false;
    size_t q = 2; m->sof = 0;
    while (q + 4 <= n) {
        if (p[q] != 0xFF) return false;
        const unsigned mk = p[q + 1];
        const size_t seg = ((size_t)p[q + 2] << 8) | p[q + 3];
        if (q + 2 + seg > n) return false;
        if (mk == 0xC0) {                                        // baseline frame header
            if (seg < 8 + 3) return false;
            m->sof = q; m->h = (p[q + 5] << 8) | p[q + 6]; m->w = (p[q + 7] << 8) | p[q + 8]; m->nc = p[q + 9];
            if (seg < 8 + 3u * m->nc) return false;
            m->vmax = 1;
            for (int c = 0; c < m->nc; c++) { const int v = p[q + 11 + 3 * c] & 15; if (v > m->vmax) m->vmax = v; }
        } else if (mk == 0xDD) return false;                      // a stripe is ONE restart interval: it must not bring a DRI of its own
        else if (mk == 0xDA) { m->sos = q; m->sos_end = q + 2 + seg; return m->sof != 0 && m->sos_end <= n - 2; }
        q += 2 + seg;
    }
    return false;
}
}  // namespace

namespace {
enum { IN_RGB = 0, IN_BGR_SWAP = 1, IN_BGR_EXT = 2 };
#define JCS_EXT_BGR_ 8                  // libjpeg-turbo's extension: B G R input, converted by the same SIMD routine as R G B
// one image -> a malloc'ed stream (*mem, *memsize; the caller frees it)
int encode_impl(const uint8_t *rows, int n_rows, int cols, int channels, int stride, int input, int quality, unsigned char **mem, unsigned long *memsize)
{
    const JpegApi &A = api();
    alignas(16) unsigned char cinfo[JPEG_CINFO_BYTES]; memset(cinfo, 0, sizeof(cinfo));
    jerr_abi err; memset(&err, 0, sizeof(err));
    Guard g; memset(&g.code, 0, sizeof(g) - offsetof(Guard, code));
    jcomp_head_abi *c = (jcomp_head_abi *)cinfo;
    unsigned char *volatile swap = nullptr;
    volatile bool created = false;
    *mem = nullptr; *memsize = 0;                             // (jpeg_mem_dest allocates and grows the buffer with malloc)
    if (setjmp(g.jb)) {
        if (created) A.c_destroy(cinfo);
        free(*mem); *mem = nullptr; free(swap);
        vfsms_set_error("jpeg_encode: %s", g.text[0] ? g.text : "encoder error");
        return VFSMS_ERR_BAD_ARG;
    }
    c->err = A.std_error(&err);
    err.error_exit = on_error; err.output_message = on_message;
    c->client_data = &g;
    A.c_create(cinfo, JPEG_ABI_VERSION, A.c_size);
    created = true;
    c->client_data = &g;
    A.c_mem_dest(cinfo, mem, memsize);
    c->image_width = (unsigned)cols; c->image_height = (unsigned)n_rows; c->input_components = channels;
    c->in_color_space = channels == 1 ? JCS_GRAYSCALE_ : input == IN_BGR_EXT ? JCS_EXT_BGR_ : JCS_RGB_;
    A.c_defaults(cinfo);
    A.c_quality(cinfo, quality, 1);
    A.c_start(cinfo, 1);
    const int CH = 16;
    if (channels == 3 && input == IN_BGR_SWAP) {
        swap = (unsigned char *)malloc((size_t)CH * cols * 3);
        if (!swap) { A.c_destroy(cinfo); free(*mem); *mem = nullptr; vfsms_set_error("jpeg_encode: out of memory"); return VFSMS_ERR_CAPACITY; }
    }
    for (int y0 = 0; y0 < n_rows; y0 += CH) {
        const int nr = n_rows - y0 < CH ? n_rows - y0 : CH;
        unsigned char *ptr[CH];
        for (int r = 0; r < nr; r++) {
            const uint8_t *src = rows + (size_t)(y0 + r) * stride;
            if (swap) {
                unsigned char *d = swap + (size_t)r * cols * 3;
                for (int x = 0; x < cols; x++) { d[3 * x] = src[3 * x + 2]; d[3 * x + 1] = src[3 * x + 1]; d[3 * x + 2] = src[3 * x]; }
                ptr[r] = d;
            } else ptr[r] = (unsigned char *)src;
        }
        int done = 0;
        while (done < nr) {
            const unsigned k = A.c_write(cinfo, ptr + done, (unsigned)(nr - done));
            if (k == 0) { g.text[0] = 0; longjmp(g.jb, 1); }      // (cannot happen with a memory destination)
            done += (int)k;
        }
    }
    A.c_finish(cinfo);
    A.c_destroy(cinfo);
    created = false;
    free(swap); swap = nullptr;
    return VFSMS_OK;
}
// does this libjpeg take B G R rows directly (libjpeg-turbo does), with the very bytes of the swapped encode?  Probed once.
bool ext_bgr_ok()
{
    static std::atomic<int> state{0};
    int st = state.load();
    if (st == 0) {
        uint8_t img[16 * 16 * 3];
        for (int k = 0; k < 16 * 16 * 3; k++) img[k] = (uint8_t)((k * 37 + (k / 48) * 11) & 255);
        unsigned char *m1 = nullptr, *m2 = nullptr; unsigned long n1 = 0, n2 = 0;
        const int r1 = encode_impl(img, 16, 16, 3, 48, IN_BGR_SWAP, 90, &m1, &n1);
        const int r2 = encode_impl(img, 16, 16, 3, 48, IN_BGR_EXT, 90, &m2, &n2);
        st = (r1 == VFSMS_OK && r2 == VFSMS_OK && n1 == n2 && n1 > 0 && memcmp(m1, m2, n1) == 0) ? 1 : -1;
        free(m1); free(m2);
        state.store(st);
    }
    return st == 1;
}
}  // namespace

// `rows`: n_rows x cols pixels of `channels` (1: gray, 3: R G B, or B G R with bgr != 0 -- the canvas order), `stride` bytes apart -> a
// complete baseline JPEG in `out` (cap bytes; *nbytes = the size needed, also on VFSMS_ERR_CAPACITY).  libjpeg defaults + `quality`: what
// cv2.imwrite(path, img) writes (quality 95).
extern "C" int vfsms_jpeg_encode(const uint8_t *rows, int n_rows, int cols, int channels, int stride, int bgr, int quality, uint8_t *out, size_t cap, size_t *nbytes)
{
    const JpegApi &A = api();
    if (!A.c_ok) { vfsms_set_error("jpeg_encode: libjpeg.so.8 (ABI 8) is not available on this host"); return VFSMS_ERR_UNSUPPORTED; }
    if (!rows || !nbytes || n_rows <= 0 || cols <= 0 || n_rows > 65500 || cols > 65500 || (channels != 1 && channels != 3) || stride < cols * channels || quality < 1 || quality > 100) {
        vfsms_set_error("jpeg_encode: bad arguments (1 or 3 channels, at most 65500 pixels a side)"); return VFSMS_ERR_BAD_ARG;
    }
    const int input = (channels == 3 && bgr) ? (ext_bgr_ok() ? IN_BGR_EXT : IN_BGR_SWAP) : IN_RGB;
    unsigned char *mem = nullptr; unsigned long memsize = 0;
    int rc = encode_impl(rows, n_rows, cols, channels, stride, input, quality, &mem, &memsize);
    if (rc != VFSMS_OK) return rc;
    StreamMap m;
    const bool sane = mem && map_stream(mem, memsize, &m) && m.h == n_rows && m.w == cols && m.nc == channels;     // the witness for the struct offsets
    *nbytes = memsize;
    if (!sane) { vfsms_set_error("jpeg_encode: libjpeg.so.8 does not have the expected struct layout"); rc = VFSMS_ERR_UNSUPPORTED; }
    else if (!out || cap < memsize) { vfsms_set_error("jpeg_encode: output buffer too small"); rc = VFSMS_ERR_CAPACITY; }
    else memcpy(out, mem, memsize);
    free(mem);
    return rc;
}

// Join stripes encoded by vfsms_jpeg_encode (same width, channels and quality; every stripe but the last `stripe_rows` high, a multiple of
// the MCU height: 16 for colour, 8 for gray) into ONE JPEG of `total_rows` rows: the headers of stripe 0 with the frame height patched and a
// DRI segment (restart interval = the MCUs of one stripe, at most 65535), then the entropy-coded segments with RSTn between them.
// `streams[k]`, `sizes[k]`: stripe k.  With out == NULL only the size is computed.
extern "C" int vfsms_jpeg_join(const uint8_t *const *streams, const size_t *sizes, int n_stripes, int stripe_rows, int total_rows, uint8_t *out, size_t cap, size_t *nbytes)
{
    if (!streams || !sizes || !nbytes || n_stripes < 1 || stripe_rows < 1 || total_rows < 1 || total_rows > 65500) { vfsms_set_error("jpeg_join: bad arguments"); return VFSMS_ERR_BAD_ARG; }
    StreamMap m0;
    if (!streams[0] || !map_stream(streams[0], sizes[0], &m0)) { vfsms_set_error("jpeg_join: stripe 0 is not a stream of vfsms_jpeg_encode"); return VFSMS_ERR_BAD_ARG; }
    const int mcu_h = 8 * m0.vmax, mcu_w = m0.nc == 1 ? 8 : 16;
    const long long interval = (long long)((m0.w + mcu_w - 1) / mcu_w) * (stripe_rows / mcu_h);
    if (n_stripes > 1 && (stripe_rows % mcu_h || interval > 65535 || (m0.nc == 3 && m0.vmax != 2))) {
        vfsms_set_error("jpeg_join: stripes of %d rows cannot be restart intervals of this image (MCU %d x %d, %lld MCUs per stripe)", stripe_rows, mcu_w, mcu_h, interval);
        return VFSMS_ERR_BAD_ARG;
    }
    size_t need = m0.sos_end + (n_stripes > 1 ? 6 : 0) + 2;
    long long rows = 0;
    for (int k = 0; k < n_stripes; k++) {
        StreamMap m;
        if (!streams[k] || !map_stream(streams[k], sizes[k], &m) || m.w != m0.w || m.nc != m0.nc || (k + 1 < n_stripes && m.h != stripe_rows) ||
            m.sof != m0.sof || m.sos != m0.sos || m.sos_end != m0.sos_end || memcmp(streams[k] + 2, streams[0] + 2, m0.sof - 2) ||       // same tables in front of the frame header
            memcmp(streams[k] + m.sof + 9, streams[0] + m0.sof + 9, m0.sos_end - m0.sof - 9)) {                                        // same components, Huffman tables, scan header
            vfsms_set_error("jpeg_join: stripe %d does not continue stripe 0 (size, channels, tables or height)", k); return VFSMS_ERR_BAD_ARG;
        }
        rows += m.h;
        need += sizes[k] - 2 - m.sos_end + (k ? 2 : 0);
    }
    if (rows != total_rows) { vfsms_set_error("jpeg_join: the stripes hold %lld rows, not %d", rows, total_rows); return VFSMS_ERR_BAD_ARG; }
    *nbytes = need;
    if (!out) return VFSMS_OK;
    if (cap < need) { vfsms_set_error("jpeg_join: output buffer too small"); return VFSMS_ERR_CAPACITY; }
    uint8_t *o = out;
    memcpy(o, streams[0], m0.sos); o += m0.sos;                                         // SOI .. DHT
    out[m0.sof + 5] = (uint8_t)(total_rows >> 8); out[m0.sof + 6] = (uint8_t)total_rows;
    if (n_stripes > 1) { const uint8_t dri[6] = { 0xFF, 0xDD, 0, 4, (uint8_t)(interval >> 8), (uint8_t)interval }; memcpy(o, dri, 6); o += 6; }
    memcpy(o, streams[0] + m0.sos, m0.sos_end - m0.sos); o += m0.sos_end - m0.sos;      // the scan header
    for (int k = 0; k < n_stripes; k++) {
        if (k) { *o++ = 0xFF; *o++ = (uint8_t)(0xD0 + ((k - 1) & 7)); }
        const size_t n = sizes[k] - 2 - m0.sos_end;
        memcpy(o, streams[k] + m0.sos_end, n); o += n;
    }
    *o++ = 0xFF; *o++ = 0xD9;
    return (size_t)(o - out) == need ? VFSMS_OK : VFSMS_ERR_BAD_ARG;
}

// ---- the device encoder's host half (jpeg_enc_kernels.hip; specified by tests/jpeg_enc_ref.py) -----------------------------------------------
namespace {
const uint8_t kQuantLuma[64] = {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                                18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
const uint8_t kQuantChroma[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
                                  99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
// Annex K: codes per length, then the symbols
const uint8_t kDcBits[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
const uint8_t kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
const uint8_t kAcBits[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
const uint8_t kAcVals[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1,
     0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
     0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a,
     0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
     0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3,
     0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1,
     0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
     0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
     0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
     0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca,
     0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};
}  // namespace

const uint8_t *jpeg_std_huff_bits(int ac, int chroma) { return ac ? kAcBits[chroma] : kDcBits[chroma]; }
const uint8_t *jpeg_std_huff_vals(int ac, int chroma) { return ac ? kAcVals[chroma] : kDcVals; }

// jpeg_quality_scaling + jpeg_add_quant_table(force_baseline): q[0] luminance, q[1] chrominance, natural order, 1..255
void jpeg_quant_tables(int quality, uint8_t q[2][64])
{
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int k = 0; k < 64; k++) {
        const int l = (kQuantLuma[k] * scale + 50) / 100, c = (kQuantChroma[k] * scale + 50) / 100;
        q[0][k] = (uint8_t)(l < 1 ? 1 : l > 255 ? 255 : l);
        q[1][k] = (uint8_t)(c < 1 ? 1 : c > 255 ? 255 : c);
    }
}

// the refusals every entry of the device encoder shares (tests/jpeg_enc_ref.py: _geometry): 1 or 3 channels, at most 65500 pixels a side, at
// most 65535 MCUs in an interval -- restart_mcus = 0 is "the image is one interval".  *interval: the interval in MCUs
int jpeg_check_geometry(const char *who, int rows, int cols, int ch, int quality, int restart_mcus, int *interval)
{
    if (ch != 1 && ch != 3) { vfsms_set_error("%s: 1 or 3 channels, got %d", who, ch); return VFSMS_ERR_BAD_ARG; }
    if (rows < 1 || cols < 1 || rows > 65500 || cols > 65500) { vfsms_set_error("%s: 1..65500 pixels a side, got %d x %d", who, rows, cols); return VFSMS_ERR_BAD_ARG; }
    if (quality < 1 || quality > 100) { vfsms_set_error("%s: quality must be 1..100, got %d", who, quality); return VFSMS_ERR_BAD_ARG; }
    if (restart_mcus < 0 || restart_mcus > 65535) { vfsms_set_error("%s: restart_mcus must be 0..65535, got %d", who, restart_mcus); return VFSMS_ERR_BAD_ARG; }
    const int mcu = ch == 3 ? 16 : 8;
    const long long n = (long long)((cols + mcu - 1) / mcu) * ((rows + mcu - 1) / mcu);
    if (restart_mcus == 0 && n > 65535) { vfsms_set_error("%s: an image of %lld MCUs cannot be one restart interval (at most 65535)", who, n); return VFSMS_ERR_BAD_ARG; }
    if (interval) *interval = restart_mcus ? restart_mcus : (int)n;
    return VFSMS_OK;
}

// the refusals of the tile-order entries (tests/tiff_jpeg_ref.py: geometry): the tile a positive multiple of 16, its MCUs a whole number of
// restart intervals of at most 65535 MCUs -- restart_mcus = 0 is "the tile is one interval".  *interval: the interval in MCUs
int jpeg_check_tile_geometry(const char *who, int tile, int ch, int quality, int restart_mcus, int *interval)
{
    if (ch != 1 && ch != 3) { vfsms_set_error("%s: 1 or 3 channels, got %d", who, ch); return VFSMS_ERR_BAD_ARG; }
    if (tile <= 0 || tile % 16 || tile > 65500) { vfsms_set_error("%s: the tile must be a positive multiple of 16 (at most 65500), got %d", who, tile); return VFSMS_ERR_BAD_ARG; }
    if (quality < 1 || quality > 100) { vfsms_set_error("%s: quality must be 1..100, got %d", who, quality); return VFSMS_ERR_BAD_ARG; }
    if (restart_mcus < 0 || restart_mcus > 65535) { vfsms_set_error("%s: restart_mcus must be 0..65535, got %d", who, restart_mcus); return VFSMS_ERR_BAD_ARG; }
    const int tm = tile / (ch == 3 ? 16 : 8);
    const long long n = (long long)tm * tm, iv = restart_mcus ? restart_mcus : n;
    if (n % iv) { vfsms_set_error("%s: the %lld MCUs of a tile are not a whole number of restart intervals of %lld MCUs", who, n, iv); return VFSMS_ERR_BAD_ARG; }
    if (iv > 65535) { vfsms_set_error("%s: a tile of %lld MCUs cannot be one restart interval (at most 65535)", who, n); return VFSMS_ERR_BAD_ARG; }
    if (interval) *interval = (int)iv;
    return VFSMS_OK;
}

// the segments of vfsms_jpeg_header, so that the abbreviated streams of TIFF (tables here, frame and scan headers there) repeat its bytes
namespace {
struct SegWriter {
    uint8_t *b; size_t n = 0;
    void seg(int marker, size_t payload) { b[n++] = 0xFF; b[n++] = (uint8_t)marker; b[n++] = (uint8_t)((payload + 2) >> 8); b[n++] = (uint8_t)(payload + 2); }
    void soi() { b[n++] = 0xFF; b[n++] = 0xD8; }
    void dqt(int quality, int ch)
    {
        uint8_t q[2][64];
        jpeg_quant_tables(quality, q);
        for (int t = 0; t < (ch == 3 ? 2 : 1); t++) { seg(0xDB, 65); b[n++] = (uint8_t)t; for (int k = 0; k < 64; k++) b[n++] = q[t][kZigzag[k]]; }
    }
    void sof0(int rows, int cols, int ch)
    {
        seg(0xC0, 6 + 3 * (size_t)ch);
        b[n++] = 8; b[n++] = (uint8_t)(rows >> 8); b[n++] = (uint8_t)rows; b[n++] = (uint8_t)(cols >> 8); b[n++] = (uint8_t)cols; b[n++] = (uint8_t)ch;
        for (int c = 0; c < ch; c++) { b[n++] = (uint8_t)(c + 1); b[n++] = (ch == 3 && c == 0) ? 0x22 : 0x11; b[n++] = c ? 1 : 0; }
    }
    void dht(int ch)
    {
        for (int t = 0; t < (ch == 3 ? 2 : 1); t++) {
            seg(0xC4, 1 + 16 + 12); b[n++] = (uint8_t)t; memcpy(b + n, kDcBits[t], 16); n += 16; memcpy(b + n, kDcVals, 12); n += 12;
            seg(0xC4, 1 + 16 + 162); b[n++] = (uint8_t)(0x10 | t); memcpy(b + n, kAcBits[t], 16); n += 16; memcpy(b + n, kAcVals[t], 162); n += 162;
        }
    }
    void dri(int restart_mcus) { if (restart_mcus) { seg(0xDD, 2); b[n++] = (uint8_t)(restart_mcus >> 8); b[n++] = (uint8_t)restart_mcus; } }
    void sos(int ch)
    {
        seg(0xDA, 4 + 2 * (size_t)ch);
        b[n++] = (uint8_t)ch;
        for (int c = 0; c < ch; c++) { b[n++] = (uint8_t)(c + 1); b[n++] = c ? 0x11 : 0x00; }
        b[n++] = 0; b[n++] = 0x3F; b[n++] = 0;
    }
};
}  // namespace

// SOI, SOF0 (tile x tile), DRI (restart_mcus > 0), SOS header into out[44] -> the length (tests/tiff_jpeg_ref.py: tile_prefix)
int jpeg_tile_prefix(int tile, int ch, int restart_mcus, uint8_t *out)
{
    SegWriter w{out};
    w.soi(); w.sof0(tile, tile, ch); w.dri(restart_mcus); w.sos(ch);
    return (int)w.n;
}

// The JPEGTables datastream of a TIFF whose tiles the device encodes (tests/tiff_jpeg_ref.py: tables): SOI, the DQT and DHT segments of
// vfsms_jpeg_header in its order, EOI.  Host only.  *nbytes = the size, also on VFSMS_ERR_CAPACITY
extern "C" int vfsms_tiff_jpeg_tables(int ch, int quality, uint8_t *out, size_t cap, size_t *nbytes)
{
    if (!nbytes) { vfsms_set_error("tiff_jpeg_tables: bad arguments"); return VFSMS_ERR_BAD_ARG; }
    TRY(jpeg_check_geometry("tiff_jpeg_tables", 16, 16, ch, quality, 0, nullptr));
    uint8_t b[700];
    SegWriter w{b};
    w.soi(); w.dqt(quality, ch); w.dht(ch);
    b[w.n++] = 0xFF; b[w.n++] = 0xD9;
    *nbytes = w.n;
    if (!out || cap < w.n) { vfsms_set_error("tiff_jpeg_tables: output buffer too small"); return VFSMS_ERR_CAPACITY; }
    memcpy(out, b, w.n);
    return VFSMS_OK;
}

// SOI, JFIF APP0, DQT per table, SOF0, DHT per table, DRI (restart_mcus > 0), SOS header: libjpeg's layout byte for byte, so the entropy-coded
// bytes of the device (vfsms_canvas_encode_jpeg_rows) behind it and FF D9 behind them are a file.  Host only.  *nbytes = the size, also on
// VFSMS_ERR_CAPACITY
extern "C" int vfsms_jpeg_header(int rows, int cols, int ch, int quality, int restart_mcus, uint8_t *out, size_t cap, size_t *nbytes)
{
    if (!nbytes) { vfsms_set_error("jpeg_header: bad arguments"); return VFSMS_ERR_BAD_ARG; }
    TRY(jpeg_check_geometry("jpeg_header", rows, cols, ch, quality, restart_mcus, nullptr));
    uint8_t b[700];
    SegWriter w{b};
    w.soi();
    static const uint8_t jfif[14] = {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
    w.seg(0xE0, 14); memcpy(b + w.n, jfif, 14); w.n += 14;
    w.dqt(quality, ch); w.sof0(rows, cols, ch); w.dht(ch); w.dri(restart_mcus); w.sos(ch);
    const size_t n = w.n;
    *nbytes = n;
    if (!out || cap < n) { vfsms_set_error("jpeg_header: output buffer too small"); return VFSMS_ERR_CAPACITY; }
    memcpy(out, b, n);
    return VFSMS_OK;
}
