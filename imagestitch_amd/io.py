"""Mosaic write-out: cv2.imwrite's stand-in and the band sinks (`Stitcher.mosaicSink` / `streamOutput`) that encode a mosaic while its bands
still leave the GPU -- JPEG in stripes on all host cores (the library's encoder), PNG, TIFF / BigTIFF, NPY.  The way OUT of the path (SURVEY
section 8 row f-2); `stitcher.py` takes these names from here.

Reference: cv2.imwrite at /root/reference/Stitcher.py:150-153, 196-199 (Main.py's `.jpg` results).
"""
import os

import numpy as np

def _imwrite(path, img):
    """cv2.imwrite's stand-in for a mosaic that is whole in host memory (streamOutput = False, or a format without a band encoder).  It
    always encodes on the host, also with Method.jpegEncoder = "device": the pixels have crossed the link by then, and sending them back
    to be encoded would move them twice more."""
    if img is None:                                          # streamed to Stitcher.mosaicSink instead
        return
    from PIL import Image
    img = np.asarray(img)
    d = os.path.dirname(path)
    if d and not os.path.exists(d):
        os.makedirs(d)
    if path.lower().endswith((".jpg", ".jpeg")) and _imwrite_jpeg_stripes(path, img):
        return
    if img.ndim == 3:
        img = img[:, :, ::-1]
    kw = {"quality": 95} if path.lower().endswith((".jpg", ".jpeg")) else {}     # cv2.imwrite's JPEG default (Pillow's is 75)
    Image.fromarray(np.ascontiguousarray(img)).save(path, **kw)


def _imwrite_jpeg_stripes(path, img):
    """a .jpg result through the library's encoder (JpegBandWriter: the stripes of the image on all cores) -> True; False = not written
    (no libjpeg.so.8, VFSMS_NATIVE_JPEG=0, an image libjpeg cannot hold): Pillow writes it."""
    if os.environ.get("VFSMS_NATIVE_JPEG", "1") == "0" or img.dtype != np.uint8 or img.ndim not in (2, 3) or (img.ndim == 3 and img.shape[2] != 3):
        return False
    if max(img.shape[:2]) > 65500 or min(img.shape[:2]) < 1:
        return False
    w = JpegBandWriter(path)
    try:
        w(0, img, img.shape)
    except _NoNativeJpeg:
        return False
    return True


class NpyBandWriter:
    """A `Stitcher.mosaicSink`: writes the bands of a mosaic into one .npy file through a memory map, so a mosaic larger than host
    memory can be assembled (set `stitcher.mosaicSink = NpyBandWriter(path)`; getStitchByOffset then returns None)."""

    transient_bands = True      # done with a band when the call returns

    def __init__(self, path):
        self.path, self._mm = path, None

    def __call__(self, row0, band, full_shape):
        if self._mm is None:
            d = os.path.dirname(self.path)
            if d and not os.path.exists(d):
                os.makedirs(d)
            # the sample width is the first band's: uint8, or uint16 (the bands of Engine.deep_mosaic_bands)
            dtype = np.uint16 if np.asarray(band).dtype == np.uint16 else np.uint8
            self._mm = np.lib.format.open_memmap(self.path, mode="w+", dtype=dtype, shape=tuple(full_shape))
        self._mm[row0:row0 + band.shape[0]] = band
        if row0 + band.shape[0] >= full_shape[0]:
            self._mm.flush()
            self._mm = None


class PngBandWriter:
    """A `Stitcher.mosaicSink` that encodes the bands into ONE PNG as they leave the device (cv2.imwrite's job at Stitcher.py:174-179,
    without the whole mosaic in host memory): IHDR, then every band deflated into IDAT chunks by a streaming zlib compressor (filter 0
    on every row), IEND.  Bands are B G R like the canvas; the file is R G B."""

    transient_bands = True      # done with a band when the call returns

    def __init__(self, path, level=1):
        self.path, self.level, self._f, self._z = path, level, None, None

    @staticmethod
    def _chunk(f, tag, data):
        import struct
        import zlib
        f.write(struct.pack(">I", len(data))); f.write(tag); f.write(data)
        f.write(struct.pack(">I", zlib.crc32(data, zlib.crc32(tag)) & 0xffffffff))

    def __call__(self, row0, band, full_shape):
        import struct
        import zlib
        if self._f is None:
            d = os.path.dirname(self.path)
            if d and not os.path.exists(d):
                os.makedirs(d)
            self._f = open(self.path, "wb")
            self._f.write(b"\x89PNG\r\n\x1a\n")
            ch = full_shape[2] if len(full_shape) == 3 else 1
            self._chunk(self._f, b"IHDR", struct.pack(">IIBBBBB", full_shape[1], full_shape[0], 8, 2 if ch == 3 else 0, 0, 0, 0))
            self._z = zlib.compressobj(self.level)
        band = np.asarray(band)
        if band.ndim == 3:
            band = band[:, :, ::-1]
        rows = np.empty((band.shape[0], 1 + band.shape[1] * (band.shape[2] if band.ndim == 3 else 1)), np.uint8)
        rows[:, 0] = 0                                           # filter type None
        rows[:, 1:] = band.reshape(band.shape[0], -1)
        data = self._z.compress(rows.tobytes())
        if data:
            self._chunk(self._f, b"IDAT", data)
        if row0 + band.shape[0] >= full_shape[0]:
            data = self._z.flush()
            if data:
                self._chunk(self._f, b"IDAT", data)
            self._chunk(self._f, b"IEND", b"")
            self._f.close()
            self._f = self._z = None


class _NoNativeJpeg(Exception):
    pass


_ENCODER_POOL = {}


def _encoder_pool(nthreads):
    from concurrent.futures import ThreadPoolExecutor
    pool = _ENCODER_POOL.get(nthreads)
    if pool is None:
        pool = _ENCODER_POOL[nthreads] = ThreadPoolExecutor(max_workers=nthreads, thread_name_prefix="vfsms-encode")
    return pool


class JpegBandWriter:
    """A `Stitcher.mosaicSink` for the reference's own output format (Main.py:21-51 writes every result as .jpg; cv2.imwrite at
    Stitcher.py:149, 175-179): the bands are cut into STRIPES whose height is a multiple of the MCU height, every stripe is encoded on a pool
    of threads by the library (vfsms_jpeg_encode: the system's libjpeg-turbo with cv2.imwrite's settings, quality 95, no interpreter lock)
    while the next band is still leaving the device, and the stripes are joined into ONE baseline JPEG as restart intervals
    (vfsms_jpeg_join).  The DCT coefficients -- hence the decoded pixels -- are those of cv2.imwrite's / Pillow's one-thread encode of the
    whole mosaic; the file is a few bytes per stripe longer (RSTn markers + one DRI segment).  Only the compressed stripes are kept in
    host memory.  Bands are B G R like the canvas."""

    def __init__(self, path, quality=95, threads=None, stripe_rows=None):
        self.path, self.quality = path, int(quality)
        self.threads = int(threads or min(os.cpu_count() or 4, 32))
        self.stripe_rows = stripe_rows
        self._reset()

    transient_bands = True      # done with a band's memory once the band after the next one has been handed over (Engine.canvas_download_bands)

    def _reset(self):
        self._futures, self._carry, self._rows_in, self._stripe, self._shape, self._band_end = [], None, 0, None, None, []

    def _encode(self, rows):
        from . import _lib
        out = _lib.jpeg_encode(rows, bgr=True, quality=self.quality)
        if out is None:
            raise _NoNativeJpeg("no libjpeg.so.8 on this host")
        return out

    def _submit(self, rows):
        if len(self._futures) >= 4 * self.threads:             # encoders far behind the band stream: do not pile the bands up in host memory
            self._futures[len(self._futures) - 4 * self.threads].result()
        self._futures.append(_encoder_pool(self.threads).submit(self._encode, rows))

    def __call__(self, row0, band, full_shape):
        band = np.asarray(band)
        if self._shape is None:
            rows, cols = int(full_shape[0]), int(full_shape[1])
            ch = int(full_shape[2]) if len(full_shape) == 3 else 1
            if ch not in (1, 3) or max(rows, cols) > 65500:
                raise ValueError("JPEG holds 1- or 3-channel images of at most 65500 pixels a side (this one: %s)" % (tuple(full_shape),))
            mcu = 16 if ch == 3 else 8
            per_row = (cols + mcu - 1) // mcu
            k = max(1, min((int(self.stripe_rows) if self.stripe_rows else 256) // mcu, 65535 // per_row))    # a stripe is one restart interval: <= 65535 MCUs
            self._stripe, self._shape = k * mcu, (rows, cols, ch)
        rows, cols, ch = self._shape
        assert row0 == self._rows_in and band.shape[1] == cols, "bands arrive in order"
        self._rows_in += band.shape[0]
        last = self._rows_in >= rows
        try:
            if self._carry is not None:
                band = np.concatenate([self._carry, band], 0)
                self._carry = None
            if not band.flags.c_contiguous:
                band = np.ascontiguousarray(band)
            S, n = self._stripe, band.shape[0]
            full = n if last else (n // S) * S
            for r in range(0, full, S):
                self._submit(band[r:min(r + S, full)])
            if full < n:
                self._carry = band[full:].copy()
            self._band_end.append(len(self._futures))
            if len(self._band_end) >= 2:                       # the band before this one may be overwritten after the next call: its stripes are done
                for f in self._futures[(self._band_end[-3] if len(self._band_end) >= 3 else 0):self._band_end[-2]]:
                    f.result()
            if not last:
                return
            from . import _lib
            parts = [f.result() for f in self._futures]
            data = _lib.jpeg_join(parts, S, rows)
            d = os.path.dirname(self.path)
            if d and not os.path.exists(d):
                os.makedirs(d)
            with open(self.path, "wb") as f:
                f.write(memoryview(data))
            self._reset()
        except BaseException:
            for f in self._futures:
                f.cancel()
            for f in self._futures:
                try:
                    f.result()
                except BaseException:                          # noqa: PERF203
                    pass
            self._reset()
            raise


class DeviceJpegFile:
    """The file side of Method.jpegEncoder = "device": the header (`_lib.jpeg_header`: libjpeg's layout with a DRI segment), then the
    entropy-coded bytes of the bands as Engine.canvas_encode_jpeg_bands hands them out, appended in order, then EOI.  Creates the directory;
    refuses what JPEG cannot hold before anything is written."""

    def __init__(self, path, full_shape, quality=95, restart_mcus=8):
        rows, cols = int(full_shape[0]), int(full_shape[1])
        ch = int(full_shape[2]) if len(full_shape) == 3 else 1
        if ch not in (1, 3) or max(rows, cols) > 65500:
            raise ValueError("JPEG holds 1- or 3-channel images of at most 65500 pixels a side (this one: %s)" % (tuple(full_shape),))
        from . import _lib
        head = _lib.jpeg_header(rows, cols, ch, quality, restart_mcus)
        d = os.path.dirname(path)
        if d and not os.path.exists(d):
            os.makedirs(d)
        self.path, self.bytes_written = path, 0
        self._f = open(path, "wb")
        self._write(head)

    def _write(self, data):
        self._f.write(data)
        self.bytes_written += len(data)

    def append(self, payload):
        self._write(memoryview(payload))

    def close(self):
        self._write(b"\xFF\xD9")
        self._f.close()
        self._f = None

    def abort(self):
        if self._f is not None:
            self._f.close()
            self._f = None
        if os.path.exists(self.path):
            os.remove(self.path)


def adler_combine(adler1, adler2, len2):
    """the Adler-32 of A || B from those of A and B and B's length (zlib's adler32_combine, which Python does not export)"""
    M = 65521
    rem = int(len2) % M
    s1, s2 = adler1 & 0xFFFF, (adler1 >> 16) & 0xFFFF
    t1, t2 = adler2 & 0xFFFF, (adler2 >> 16) & 0xFFFF
    return ((s2 + t2 + rem * s1 + M * M - rem) % M) << 16 | (s1 + t1 + M - 1) % M


class DevicePngFile:
    """The file side of Method.pngEncoder = "device": the signature, IHDR and the zlib header in an IDAT of its own, then the IDAT chunks of
    the bands as Engine.canvas_encode_png_bands hands them out (filtered, coded and checksummed on the device; every chunk ends on a byte of
    the deflate stream), appended verbatim in order, then an IDAT with the final empty stored block and the Adler-32 of all filtered bytes,
    folded together from the bands' own, and IEND.  Creates the directory; refuses what PNG cannot hold before anything is written."""

    def __init__(self, path, full_shape, segment_rows=16):
        import struct
        rows, cols = int(full_shape[0]), int(full_shape[1])
        ch = int(full_shape[2]) if len(full_shape) == 3 else 1
        if ch not in (1, 3) or min(rows, cols) < 1 or max(rows, cols) >= 1 << 31:
            raise ValueError("the device's PNG holds 1- or 3-channel images of 1 .. 2^31 - 1 pixels a side (this one: %s)" % (tuple(full_shape),))
        if not 1 <= int(segment_rows) <= 4096 or int(segment_rows) * (1 + cols * ch) * 15 >= 1 << 32:
            raise ValueError("the device's PNG takes segments of 1..4096 rows whose bytes at 15 bits each fit 32 bits (segment_rows = %r, %d bytes a row)" % (segment_rows, 1 + cols * ch))
        d = os.path.dirname(path)
        if d and not os.path.exists(d):
            os.makedirs(d)
        self.path, self.bytes_written, self.segment_rows = path, 0, int(segment_rows)
        self._rowbytes, self._rows, self._rows_in, self._adler = 1 + cols * ch, rows, 0, 1
        self._f = open(path, "wb")
        self._write(b"\x89PNG\r\n\x1a\n")
        self._chunk(b"IHDR", struct.pack(">IIBBBBB", cols, rows, 8, 2 if ch == 3 else 0, 0, 0, 0))
        self._chunk(b"IDAT", b"\x78\x01")

    def _write(self, data):
        self._f.write(data)
        self.bytes_written += len(data)

    def _chunk(self, tag, data):
        import struct
        import zlib
        self._write(struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff))

    def append(self, payload, adler, nbytes_filtered):
        """the chunks of the next band, the Adler-32 of its filtered bytes and their number (the band's rows x (1 + cols x ch))"""
        self._write(memoryview(payload))
        self._adler = adler_combine(self._adler, int(adler), int(nbytes_filtered))
        self._rows_in += int(nbytes_filtered) // self._rowbytes

    def close(self):
        import struct
        if self._rows_in != self._rows:
            raise ValueError("DevicePngFile: %d of %d rows were appended" % (self._rows_in, self._rows))
        self._chunk(b"IDAT", b"\x01\x00\x00\xff\xff" + struct.pack(">I", self._adler))
        self._chunk(b"IEND", b"")
        self._f.close()
        self._f = None

    def abort(self):
        if self._f is not None:
            self._f.close()
            self._f = None
        if os.path.exists(self.path):
            os.remove(self.path)


class TiffBandWriter:
    """A `Stitcher.mosaicSink` for uncompressed baseline TIFF (BigTIFF beyond 4 GB): one strip per band, the directory written behind the
    last band.  R G B (or gray) 8-bit samples, or 16-bit little-endian ones: the sample width is the first band's dtype (uint16: a mosaic
    of Engine.deep_mosaic_bands; anything else is written as 8-bit)."""

    transient_bands = True      # done with a band when the call returns

    def __init__(self, path, force_big=False):
        self.path, self._f, self._strips, self._bits = path, None, [], 8
        self.force_big = force_big                               # BigTIFF whatever the size (tests: the > 4 GB layout on a small image)

    def __call__(self, row0, band, full_shape):
        import struct
        rows, cols = full_shape[0], full_shape[1]
        ch = full_shape[2] if len(full_shape) == 3 else 1
        if self._f is None:
            self._bits = 16 if np.asarray(band).dtype == np.uint16 else 8
        bits = self._bits
        big = self.force_big or rows * cols * ch * (bits // 8) + (1 << 20) >= (1 << 32)
        if self._f is None:
            d = os.path.dirname(self.path)
            if d and not os.path.exists(d):
                os.makedirs(d)
            self._f = open(self.path, "wb")
            self._f.write(struct.pack("<2sHHHQ", b"II", 43, 8, 0, 0) if big else struct.pack("<2sHI", b"II", 42, 0))
            self._strips, self._band_rows = [], band.shape[0]
        band = np.asarray(band)
        if band.ndim == 3:
            band = band[:, :, ::-1]
        if bits == 16:
            band = band.astype("<u2", copy=False)
        self._strips.append((self._f.tell(), band.size * (bits // 8)))       # StripByteCounts are bytes
        self._f.write(np.ascontiguousarray(band).tobytes())
        if row0 + band.shape[0] < rows:
            return
        f, n = self._f, len(self._strips)
        if f.tell() & 1:
            f.write(b"\0")
        fmt_off = "<%dQ" % n if big else "<%dI" % n
        off_pos = f.tell(); f.write(struct.pack(fmt_off, *[o for o, _c in self._strips]))
        cnt_pos = f.tell(); f.write(struct.pack(fmt_off, *[c for _o, c in self._strips]))
        # BitsPerSample 8, 8, 8: three SHORTs are 6 bytes -- more than classic TIFF's 4-byte value field (stored behind the strips, the field
        # holds the offset), but they FIT BigTIFF's 8-byte field and must then sit in it (a reader takes the field as the values)
        bps = bits | bits << 16 | bits << 32
        if ch == 3 and not big:
            bps = f.tell(); f.write(struct.pack("<3H", bits, bits, bits)); f.write(b"\0\0")
        ifd = f.tell()
        ltype = 16 if big else 4                                 # LONG8 / LONG
        tags = [(256, ltype, 1, cols), (257, ltype, 1, rows), (258, 3, ch, bps if ch == 3 else bits), (259, 3, 1, 1),
                (262, 3, 1, 2 if ch == 3 else 1), (273, ltype, n, off_pos if n > 1 else self._strips[0][0]), (277, 3, 1, ch),
                (278, ltype, 1, self._band_rows), (279, ltype, n, cnt_pos if n > 1 else self._strips[0][1])]
        if big:
            f.write(struct.pack("<Q", len(tags)))
            for t, ty, c, v in tags:
                f.write(struct.pack("<HHQQ", t, ty, c, v))
            f.write(struct.pack("<Q", 0))
            f.seek(8); f.write(struct.pack("<Q", ifd))
        else:
            f.write(struct.pack("<H", len(tags)))
            for t, ty, c, v in tags:
                f.write(struct.pack("<HHII", t, ty, c, v))
            f.write(struct.pack("<I", 0))
            f.seek(4); f.write(struct.pack("<I", ifd))
        f.close()
        self._f = None


PYRAMID_MAX_LEVELS = 10


def default_levels(rows, cols, tile):
    """reduced levels of a pyramidal file: the smallest K >= 0 whose level K fits one tile, at most PYRAMID_MAX_LEVELS (tests/pyramid_ref.py)"""
    K = 0
    while K < PYRAMID_MAX_LEVELS and max(rows, cols) > tile:
        rows, cols, K = (rows + 1) >> 1, (cols + 1) >> 1, K + 1
    return K


def _usable_cpus():
    """host CPUs this process may use: its affinity set, capped by OMP_NUM_THREADS where the host sets it (os.cpu_count() reports the
    whole machine, also to a process that was given a share of it)"""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 4)
    try:
        cap = int(os.environ.get("OMP_NUM_THREADS") or 0)
    except ValueError:
        cap = 0
    return max(1, min(n, cap) if cap > 0 else n)


class PyramidTiffBandWriter:
    """A `Stitcher.mosaicSink` for tiled pyramidal TIFF (BigTIFF beyond 4 GB), the layout OpenSlide, libvips, QuPath and GDAL read: level 0
    in tiles of `tile` x `tile`, then levels 1 .. K as reduced-resolution pages (NewSubfileType 1), every level in an IFD of its own,
    chained.  The levels are NOT computed here: they arrive with their band (`sink(row0, band, full_shape, levels=[...])`, formed on the
    device by Engine.canvas_download_pyramid_bands; arithmetic: tests/pyramid_ref.py) and `pyramid_levels(full_shape)` tells the caller how
    many to send -- `levels`, or the smallest count whose last level fits one tile.  Per level the rows that do not fill a tile row yet are
    carried (a copy), a complete tile row is written at once, the directories behind the last band.  Tiles are row-major, edge tiles
    padded with zeros; compression "none" or "deflate" (every tile a zlib stream, level 1, compressed on the encoder pool).  Bands are
    B G R like the canvas; the file is R G B.  The file is written under a hidden name beside `path` and renamed when it is complete.

    compression "jpeg" (TIFF compression 7, what slide viewers expect; tests/tiff_jpeg_ref.py): the writer takes no pixels at all.  It
    declares `device_tiles`, and `tiles(row0, nrows, payload, index, full_shape)` takes the finished tile streams of a band as
    Engine.canvas_encode_pyramid_tiles hands them out -- encoded on the device at `quality` with `restart_mcus` MCUs per restart interval
    (0: one interval per tile), edge tiles replicating the level's last row and column -- appends the payload with one write and notes
    (offset, count) per tile from the index.  The tables go into JPEGTables once per directory; colour is Y Cb Cr 4:2:0 (Photometric 6).
    There is no host encoder behind it: pixel bands are refused.

    compression "deflate-device" (TIFF compression 8 with Predictor = 2, lossless; tests/deflate_ref.py) takes finished tile streams in the
    same way -- Engine.canvas_encode_pyramid_tiles_deflate's, every tile a zlib stream of its horizontally differenced samples, coded on the
    device -- with edge tiles padded with zeros: the decoded pages equal those of "none" and "deflate", padding included.  Colour is R G B
    (Photometric 2); there are no tables to share; `quality` and `restart_mcus` play no part; pixel bands are refused."""

    transient_bands = True      # done with a band (and its levels) when the call returns

    def __init__(self, path, tile=512, levels=None, compression="none", force_big=False, quality=95, restart_mcus=8):
        if int(tile) <= 0 or int(tile) % 16:
            raise ValueError("PyramidTiffBandWriter: tile must be a positive multiple of 16 (TIFF 6.0, TileWidth), got %r" % (tile,))
        if compression not in ("none", "deflate", "jpeg", "deflate-device"):
            raise ValueError("PyramidTiffBandWriter: compression must be 'none', 'deflate', 'jpeg' or 'deflate-device', got %r" % (compression,))
        if levels is not None and not 0 <= int(levels) <= PYRAMID_MAX_LEVELS:
            raise ValueError("PyramidTiffBandWriter: levels must be None or 0..%d, got %r" % (PYRAMID_MAX_LEVELS, levels))
        self.path, self.tile, self.levels, self.compression, self.force_big = path, int(tile), levels, compression, force_big
        self.quality, self.restart_mcus = int(quality), int(restart_mcus)
        self.device_tiles = compression in ("jpeg", "deflate-device")      # the bands arrive as finished tile streams (`tiles`), not as pixels
        self.tile_codec = {"jpeg": "jpeg", "deflate-device": "deflate"}.get(compression)          # which coder of the engine makes them
        if self.tile_codec == "jpeg":
            self.check_jpeg_geometry(3)                          # (what holds for colour's (tile / 16)^2 MCUs holds for gray's (tile / 8)^2)
        self._f = None

    def check_jpeg_geometry(self, ch):
        """the refusals of tests/tiff_jpeg_ref.py's geometry for tiles of `ch` channels"""
        if ch not in (1, 3):
            raise ValueError("PyramidTiffBandWriter: JPEG tiles hold 1 or 3 channels, got %d" % ch)
        if not 1 <= self.quality <= 100:
            raise ValueError("PyramidTiffBandWriter: quality must be 1..100, got %r" % (self.quality,))
        if not 0 <= self.restart_mcus <= 65535:
            raise ValueError("PyramidTiffBandWriter: restart_mcus must be 0..65535, got %r" % (self.restart_mcus,))
        n = (self.tile // (16 if ch == 3 else 8)) ** 2
        interval = self.restart_mcus or n
        if n % interval or interval > 65535:
            raise ValueError("PyramidTiffBandWriter: the %d MCUs of a %d x %d tile are not whole restart intervals of %d MCUs (at most 65535 each)"
                             % (n, self.tile, self.tile, interval))

    def pyramid_levels(self, full_shape):
        return int(self.levels) if self.levels is not None else default_levels(int(full_shape[0]), int(full_shape[1]), self.tile)

    @property
    def _part(self):
        d, name = os.path.split(self.path)
        return os.path.join(d, "." + name + ".part")

    def _open(self, full_shape, K):
        import struct
        rows, cols = int(full_shape[0]), int(full_shape[1])
        self._ch = int(full_shape[2]) if len(full_shape) == 3 else 1
        if self._ch not in (1, 3):
            raise ValueError("PyramidTiffBandWriter holds 1- or 3-channel images (this one: %s)" % (tuple(full_shape),))
        T = self.tile
        self._sizes = [(rows, cols)]
        for _ in range(K):
            r, c = self._sizes[-1]
            self._sizes.append(((r + 1) >> 1, (c + 1) >> 1))
        padded = sum(-(-r // T) * -(-c // T) * T * T * self._ch for r, c in self._sizes)
        self._big = bool(self.force_big) or padded + (1 << 20) >= (1 << 32)
        d = os.path.dirname(self.path)
        if d and not os.path.exists(d):
            os.makedirs(d)
        self._f = open(self._part, "wb")
        self._f.write(struct.pack("<2sHHHQ", b"II", 43, 8, 0, 0) if self._big else struct.pack("<2sHI", b"II", 42, 0))
        self._carry = [None] * (K + 1)
        self._rows_in = [0] * (K + 1)
        self._tiles = [[] for _ in range(K + 1)]                 # (offset, byte count) per tile, row-major
        if self.tile_codec == "jpeg":
            from . import _lib
            self.check_jpeg_geometry(self._ch)
            self._tables = _lib.tiff_jpeg_tables(self._ch, self.quality)

    def _tile_row(self, k, strip):
        """one row of tiles of level k from `strip` (<= tile rows, the level's full width, R G B), edge tiles zero-padded"""
        import zlib
        T, ch, f = self.tile, self._ch, self._f
        ntx = -(-self._sizes[k][1] // T)
        pad = np.zeros((T, ntx * T, ch), np.uint8)
        pad[:strip.shape[0], :strip.shape[1]] = strip.reshape(strip.shape[0], strip.shape[1], ch)
        tiles = np.ascontiguousarray(pad.reshape(T, ntx, T, ch).transpose(1, 0, 2, 3))          # [ntx][T][T][ch]
        if self.compression == "none":
            pos, nb = f.tell(), T * T * ch
            f.write(tiles.data)
            self._tiles[k] += [(pos + j * nb, nb) for j in range(ntx)]
            return
        pool = _encoder_pool(min(_usable_cpus(), 32))
        for data in pool.map(lambda t: zlib.compress(t, 1), [tiles[j].data for j in range(ntx)]):
            self._tiles[k].append((f.tell(), len(data)))
            f.write(data)

    def _feed(self, k, arr):
        R, T = self._sizes[k][0], self.tile
        arr = np.asarray(arr)
        assert arr.shape[1] == self._sizes[k][1] and self._rows_in[k] + arr.shape[0] <= R, "level %d: rows beyond the level's size" % k
        if arr.ndim == 3:
            arr = arr[:, :, ::-1]
        self._rows_in[k] += arr.shape[0]
        last = self._rows_in[k] >= R
        if self._carry[k] is not None:
            arr = np.concatenate([self._carry[k], arr], 0)
            self._carry[k] = None
        full = arr.shape[0] if last else (arr.shape[0] // T) * T
        for r in range(0, full, T):
            self._tile_row(k, arr[r:min(r + T, full)])
        if full < arr.shape[0]:
            self._carry[k] = arr[full:].copy()                   # (the band's memory is the caller's again after this call)

    def _directories(self):
        import struct
        f, big, ch = self._f, self._big, self._ch
        ltype, lfmt, lsize = (16, "Q", 8) if big else (4, "I", 4)
        field = 8 if big else 4
        fmts = {3: "H", 4: "I", 7: "B", 16: "Q"}
        jpeg = self.tile_codec == "jpeg"
        ifds = []
        for k, (rows, cols) in enumerate(self._sizes):
            n = len(self._tiles[k])
            assert n == -(-rows // self.tile) * -(-cols // self.tile), "level %d: %d tiles written" % (k, n)
            tags = [(254, 4, [1 if k else 0]), (256, ltype, [cols]), (257, ltype, [rows]), (258, 3, [8] * ch),
                    (259, 3, [7 if jpeg else 8 if self.compression in ("deflate", "deflate-device") else 1]), (262, 3, [1 if ch == 1 else 6 if jpeg else 2]), (277, 3, [ch]),
                    (284, 3, [1]), (322, ltype, [self.tile]), (323, ltype, [self.tile]), (324, ltype, [o for o, _c in self._tiles[k]]),
                    (325, ltype, [c for _o, c in self._tiles[k]])]
            if jpeg:                                             # JPEGTables (UNDEFINED bytes); YCbCrSubSampling 2, 2: the coder's 4:2:0
                tags += [(347, 7, list(self._tables))] + ([(530, 3, [2, 2])] if ch == 3 else [])
            if self.tile_codec == "deflate":                     # Predictor 2: horizontal differencing, undone by the reader per tile row
                tags.insert(8, (317, 3, [2]))                  # (directory entries ascend by tag: between 284 and 322)
            entries = []
            for tag, ty, vals in tags:
                data = struct.pack("<%d%s" % (len(vals), fmts[ty]), *vals)
                # a value that fits the field sits IN it, left-justified (BitsPerSample 8, 8, 8: 6 bytes -- behind the tiles in classic TIFF, in
                # the 8-byte field of BigTIFF, as TiffBandWriter documents); anything longer is stored in front of the directories
                if len(data) > field:
                    if f.tell() & 1:
                        f.write(b"\0")
                    pos = f.tell(); f.write(data)
                    data = struct.pack("<" + lfmt, pos)
                entries.append(struct.pack("<HH" + lfmt, tag, ty, len(vals)) + data.ljust(field, b"\0"))
            ifds.append(entries)
        if f.tell() & 1:
            f.write(b"\0")
        first = pos = f.tell()
        for k, entries in enumerate(ifds):
            size = (8 if big else 2) + len(entries) * (20 if big else 12) + lsize
            nxt = pos + size if k + 1 < len(ifds) else 0
            f.write(struct.pack("<Q" if big else "<H", len(entries))); f.write(b"".join(entries)); f.write(struct.pack("<" + lfmt, nxt))
            pos += size
        if not big and f.tell() >= (1 << 32):
            raise ValueError("PyramidTiffBandWriter: the file outgrew classic TIFF's 4 GB; write it with force_big=True")
        f.seek(8 if big else 4); f.write(struct.pack("<" + lfmt, first))

    def _finish(self):
        self._directories()
        self._f.close()
        self._f = None
        os.replace(self._part, self.path)

    def _abort(self):
        if self._f is not None:
            self._f.close()
            self._f = None
        if os.path.exists(self._part):
            os.remove(self._part)

    def tiles(self, row0, nrows, payload, index, full_shape):
        """compression "jpeg" or "deflate-device": the tile streams that the band [row0, row0 + nrows) completes
        (Engine.canvas_encode_pyramid_tiles, .._deflate): `payload` holds them back to back, `index` is (n, 4) integers (level, tile number in the level, offset in payload, bytes) in file order"""
        try:
            if not self.device_tiles:
                raise ValueError("PyramidTiffBandWriter: tile streams go to compression 'jpeg' or 'deflate-device', this writer's is %r" % (self.compression,))
            if self._f is None:
                self._open(full_shape, self.pyramid_levels(full_shape))
            if row0 != self._rows_in[0] or nrows <= 0 or row0 + nrows > self._sizes[0][0]:
                raise ValueError("PyramidTiffBandWriter: bands arrive in order (row %d expected, got %d)" % (self._rows_in[0], row0))
            payload = memoryview(payload)
            pos = self._f.tell()
            for k, t, off, cnt in np.asarray(index, np.int64).reshape(-1, 4).tolist():
                if not 0 <= k < len(self._tiles) or t != len(self._tiles[k]) or off < 0 or cnt <= 0 or off + cnt > len(payload):
                    raise ValueError("PyramidTiffBandWriter: tile %d of level %d is out of order or outside the payload" % (t, k))
                self._tiles[k].append((pos + off, cnt))
            self._f.write(payload)
            self._rows_in[0] += nrows
            if self._rows_in[0] >= self._sizes[0][0]:
                self._finish()
        except BaseException:
            self._abort()
            raise

    def __call__(self, row0, band, full_shape, levels=None):
        levels = list(levels) if levels is not None else []
        try:
            if self.device_tiles:
                raise ValueError("PyramidTiffBandWriter: compression %r takes finished tile streams (tiles), there is no host encoder for pixel bands" % (self.compression,))
            if self._f is None:
                K = self.pyramid_levels(full_shape)
                if len(levels) != K:
                    raise ValueError("PyramidTiffBandWriter: %d reduced levels expected with every band (pyramid_levels), got %d" % (K, len(levels)))
                self._open(full_shape, K)
            if len(levels) != len(self._sizes) - 1 or row0 != self._rows_in[0]:
                raise ValueError("PyramidTiffBandWriter: bands arrive in order, each with its %d levels" % (len(self._sizes) - 1))
            for k, arr in enumerate([band] + levels):
                self._feed(k, arr)
            if self._rows_in[0] < self._sizes[0][0]:
                return
            self._finish()
        except BaseException:
            self._abort()
            raise


def _native_jpeg_encoder():
    """does the library encode JPEG on this host (libjpeg.so.8 present, not switched off)?"""
    if os.environ.get("VFSMS_NATIVE_JPEG", "1") == "0":
        return False
    try:
        from . import _lib
        return _lib.jpeg_encode(np.zeros((8, 8), np.uint8)) is not None
    except Exception:
        return False


def band_writer_for(path, pyramid=None):
    """the streaming encoder for an output file name, or None when its format has none here (JPEG without libjpeg.so.8 on the host: written
    whole through Pillow).  pyramid: a dict of PyramidTiffBandWriter's keyword arguments -> the pyramidal writer for .tif / .tiff"""
    ext = os.path.splitext(path)[1].lower()
    if pyramid is not None:
        return PyramidTiffBandWriter(path, **pyramid) if ext in (".tif", ".tiff") else None
    if ext in (".jpg", ".jpeg"):
        return JpegBandWriter(path) if _native_jpeg_encoder() else None
    return PngBandWriter(path) if ext == ".png" else TiffBandWriter(path) if ext in (".tif", ".tiff") else NpyBandWriter(path) if ext == ".npy" else None
