"""Sequence drivers, pair registration and mosaic assembly -- host-side mirror of the reference's
`Stitcher.Stitcher` (/root/reference/Stitcher.py; every method cites the lines it mirrors).

Drop-in for Main.py: same class attributes (direction, directIncre, fuseMethod, ...), same method names and
return conventions (`(True, [dx, dy])` / `(False, "  The two images can not match")`), same log lines.
What differs is where the work happens: registration attempts run as fused device-resident batches
(SURF + BF-L2 + ratio + mode vote, or FP64 phase correlation) and the mosaic lives in a u8 + validity canvas
in HBM; see imagestitch_amd/csrc.
"""
import copy
import os
import time

import numpy as np

from . import utility as Utility
from . import fusion as ImageFusion
from .utility import roi_rect, offset_estimator, vote_tail
from ._lib import Engine

CANNOT_MATCH = "  The two images can not match"


class ImageFeature():
    """Stitcher.py:14-18: features of the second image of the previous pair (full-image line scans)."""
    isBreak = True
    kps = None
    feature = None


class ResidentFeatures:
    """What Stitcher.tempImageFeature holds when the stock operators run: the keypoints + descriptors of a tile stay in HBM under
    an engine handle (vfsms_features_*); `kps` and `feature` of the cache point at this object, which downloads the arrays only if
    somebody actually reads them (np.asarray(obj.kps) / obj.descriptors())."""

    def __init__(self, engine, handle, n, dim):
        self.engine, self.handle, self.n, self.dim = engine, handle, n, dim
        self._host = None

    def __len__(self):
        return self.n

    def arrays(self):
        if self._host is None:
            self._host = self.engine.features_download(self.handle, self.n, self.dim)
        return self._host

    def __array__(self, dtype=None, copy=None):
        return self.arrays()[0]

    def descriptors(self):
        return self.arrays()[1]

    def release(self):
        if self.handle is not None:
            try:
                self.engine.features_free(self.handle)
            except Exception:
                pass
            self.handle = None


from .ingest import (_imread, _imread_gray_pointer, _PillowBlocks, _decoder_pool, _decode_once, _fill_from_jpeg, _ycc_to_bgr, _imshape,  # noqa: F401
                     _list_images, TileIngest)
from .io import (_imwrite, _imwrite_jpeg_stripes, NpyBandWriter, PngBandWriter, JpegBandWriter, TiffBandWriter, _NoNativeJpeg,  # noqa: F401
                 _native_jpeg_encoder, band_writer_for, PyramidTiffBandWriter, DeviceJpegFile, DevicePngFile)


def _join(base, *parts):
    return os.path.join(base.replace("\\", os.sep), *[str(p) for p in parts])


class Stitcher(Utility.Method):
    isColorMode = True
    direction = 1               # 1: A above B; 2: A left of B; 3: A below B; 4: A right of B
    directIncre = 1             # rotation step of the direction search: 1, 0 or -1
    fuseMethod = "notFuse"
    phaseResponseThreshold = 0.15
    # cv2.phaseCorrelate(a, b) reports the shift of b's content relative to a's (b - a); the feature path votes a - b, and the
    # reference adds both with the same sign (Stitcher.py:244-251), so its phase offsets come out mirrored (SURVEY 8a row G:
    # iron gives [1400, 0] where the true offset is [1699, -1]).  The default reproduces the reference as written; True negates
    # the raw shift before the axis correction (iron -> [1698, 0]).  The batched registrar follows the reference only.
    phaseSignFix = False
    # "ncc": every correlation surface is read by the resolver of tests/phase_resolve_ref.py instead -- the phasePeaks (1..8) largest peaks of
    # the unshifted surface, each of their four circular readings scored by the overlap correlation of offsetVerify, the best one kept and
    # accepted when its score reaches phaseResolveThreshold.  Neither the sign question, nor the wrap of the circular transform, nor the
    # response gate is left: phaseSignFix and phaseResponseThreshold are not consulted.  The threshold and the pixel minimum are
    # offsetVerify's defaults (the same statistic on the same kind of pixels).  Pair by pair and batched alike.
    phaseResolve = "none"       # "none" or "ncc"
    phasePeaks = 2
    phaseResolveThreshold = 0.5
    phaseResolveMinPixels = 4096
    tempImageFeature = ImageFeature()

    imageFusion = ImageFusion.ImageFusion()

    # ------------------------------------------------------------------------------------------------
    def directionIncrease(self, direction):
        """Stitcher.py:36-47: rotate within [1, 4]."""
        direction += self.directIncre
        if direction == 5:
            direction = 1
        if direction == 0:
            direction = 4
        return direction

    # ------------------------------------------------------------------------------------------------
    def flowStitch(self, fileList, caculateOffsetMethod):
        """Stitcher.py:49-94 -> ((status, endfileIndex), stitchImage)."""
        self._checkRepairOptions()
        self.printAndWrite("Stitching the directory which have " + str(fileList[0]))
        fileNum = len(fileList)
        offsetList = []
        describtion = ""
        startTime = time.time()
        status = True
        endfileIndex = 0
        imageB = None
        batched = self._registerBatched(fileList, caculateOffsetMethod)
        if batched is not None:
            (status, endfileIndex, offsetList, describtion) = batched
        # failedPairRepair = "stage" in the pair-by-pair loop: a failed pair is recorded and the loop goes on; the repair follows the loop
        repair = self.failedPairRepair == "stage" and batched is None and fileNum >= 2
        if repair and any(_imshape(f) != _imshape(fileList[0]) for f in fileList):
            self.printAndWrite("  The tiles are of different sizes: pairs that can not be registered are not repaired")
            repair = False
        rows = []
        try:
            for fileIndex in (range(0, fileNum - 1) if batched is None else ()):
                self.printAndWrite("stitching " + str(fileList[fileIndex]) + " and " + str(fileList[fileIndex + 1]))
                imageA = imageB if imageB is not None else _imread(fileList[fileIndex], False)   # decoded once per tile
                imageB = _imread(fileList[fileIndex + 1], False)
                if caculateOffsetMethod == self.calculateOffsetForPhaseCorrleate:
                    (status, offset) = self.calculateOffsetForPhaseCorrleate([fileList[fileIndex], fileList[fileIndex + 1]])
                else:
                    (status, offset) = caculateOffsetMethod([imageA, imageB])
                if status == False:
                    if repair:
                        rows.append([0, 0, 0, 0, 0, 0])
                        self.tempImageFeature.isBreak = True      # the next pair describes its own tile A
                        continue
                    describtion = "  " + str(fileList[fileIndex]) + " and " + str(fileList[fileIndex + 1]) + " can not be stitched"
                    break
                else:
                    if repair:
                        rows.append([1, int(offset[0]), int(offset[1]), int(self.direction), 0, 0])
                    offsetList.append(offset)
                    endfileIndex = fileIndex + 1
        except Exception:
            self.releaseTiles()                     # an operator that raises must not leave the pair's tiles in HBM
            raise
        self.releaseTiles()
        if repair and not all(r[0] for r in rows):
            (status, endfileIndex, offsetList, describtion) = self._repairPairLoop(fileList, rows)
        if self.globalAdjust != "none" and batched is None:
            offsetList = self._globalAdjust(fileList[:len(offsetList) + 1], offsetList)
        endTime = time.time()
        self.printAndWrite("The time of registering is " + str(endTime - startTime) + "s")
        self.printAndWrite("start stitching")
        startTime = time.time()
        stitchImage = self.getStitchByOffset(fileList, offsetList)
        endTime = time.time()
        self.printAndWrite("The time of fusing is " + str(endTime - startTime) + "s")
        if status == False:
            self.printAndWrite(describtion)
        return ((status, endfileIndex), stitchImage)

    pathHint = None              # optional PREDICTION of the accepted direction of every pair (a scan pattern the operator knows, e.g. from grid.serpentine_directions); the speculation prior of the FIRST dataset -- later ones use what the previous one taught (GridRegistrar.path_memory).  Results never depend on it.
    streamOutput = True          # imageSetStitch*: encode JPEG / PNG / TIFF / NPY results band by band as they leave the device -- the mosaic is never whole in host memory and the encoder works while later bands are still copied (default since round 5; False: download the whole mosaic, then write it)
    batchRegistration = True     # let flowStitch register a whole file list in fused device batches when the stock search is used
    decodeThreads = 0            # decoder threads of the ingest pipeline (0: one per host core, at most 32 with the library's own JPEG decoder, 16 with Pillow -- beyond that its Python-side work and the registrar's own host thread get in each other's way; _decoderThreads)

    def _streamTo(self, paths, pattern=None):
        """install a mosaicSink that opens one streaming encoder per mosaic: `paths` names the files (pattern is None) or collects the
        part files made from `pattern % n`; returns None (and installs nothing) when the format has no band encoder"""
        if "mosaicSink" in self.__dict__:                    # the user streams the mosaics somewhere else (stitcher.mosaicSink = NpyBandWriter(...)): leave it alone
            return None
        probe = pattern % 0 if pattern else paths[0]
        state = {"f": None, "w": None, "n": 0}                  # the file or writer of the mosaic at work, the mosaics begun

        def next_path():
            path = (pattern % state["n"]) if pattern else paths[state["n"]]
            if pattern:
                paths.append(path)
            state["n"] += 1
            return path
        if self._deviceJpeg(os.path.splitext(probe)[1][1:]):
            # jpegEncoder "device": the sink takes the bands' entropy-coded bytes, not their pixels (_writeOut asks the engine for them)

            def payload_sink(row0, nrows, payload, full_shape):
                try:
                    if state["f"] is None:
                        state["f"] = DeviceJpegFile(next_path(), full_shape, int(self.jpegQuality), int(self.jpegRestartMcus))
                    state["f"].append(payload)
                    if row0 + nrows >= full_shape[0]:
                        state["f"].close()
                        state["f"] = None
                except BaseException:
                    if state["f"] is not None:
                        state["f"].abort()
                        state["f"] = None
                    raise
            payload_sink.device_jpeg = True
            self.mosaicSink = payload_sink
            return payload_sink
        if self._devicePng(os.path.splitext(probe)[1][1:]):
            # pngEncoder "device": the sink takes the bands' finished IDAT chunks and Adler-32, not their pixels (_writeOut asks the engine for them)

            def png_sink(row0, nrows, payload, adler, full_shape):
                try:
                    if state["f"] is None:
                        state["f"] = DevicePngFile(next_path(), full_shape, int(self.pngSegmentRows))
                    ch = full_shape[2] if len(full_shape) > 2 else 1
                    state["f"].append(payload, adler, nrows * (1 + full_shape[1] * ch))
                    if row0 + nrows >= full_shape[0]:
                        state["f"].close()
                        state["f"] = None
                except BaseException:
                    if state["f"] is not None:
                        state["f"].abort()
                        state["f"] = None
                    raise
            png_sink.device_png = True
            self.mosaicSink = png_sink
            return png_sink
        # outputPyramid: every mosaic through the pyramidal writer, which takes the reduced levels of a band beside it
        wkw = {"pyramid": self._pyramidOptions()} if self.outputPyramid else {}
        first = band_writer_for(probe, **wkw)
        if first is None:
            return None

        def sink(row0, band, full_shape, **lkw):
            if state["w"] is None:
                state["w"] = band_writer_for(next_path(), **wkw)
            state["w"](row0, band, full_shape, **lkw)
            if row0 + band.shape[0] >= full_shape[0]:
                state["w"] = None
        def tiles(row0, nrows, payload, index, full_shape):
            # pyramidCompression "jpeg" / "deflate-device": the bands' finished tile streams, not their pixels (_writeOut asks the engine for them)
            if state["w"] is None:
                state["w"] = band_writer_for(next_path(), **wkw)
            try:
                state["w"].tiles(row0, nrows, payload, index, full_shape)
            except BaseException:
                state["w"] = None
                raise
            if row0 + nrows >= full_shape[0]:
                state["w"] = None
        sink.transient_bands = bool(getattr(first, "transient_bands", False))
        if hasattr(first, "pyramid_levels"):
            sink.pyramid_levels = first.pyramid_levels
        if getattr(first, "device_tiles", False):
            sink.device_tiles, sink.tiles, sink.tile_codec = True, tiles, getattr(first, "tile_codec", "jpeg")
        self.mosaicSink = sink
        return sink

    def _deviceJpeg(self, outputfileExtension):
        """does this output go through the device's JPEG encoder (Method.jpegEncoder = "device" with streamOutput and a .jpg / .jpeg result)?
        Judged -- with the engine's support and mosaicBandRows -- before a file is listed or a tile decoded.  Everything else (other formats,
        outputPyramid, streamOutput = False, a mosaicSink of the user's) is written as with "host"."""
        if self.jpegEncoder not in ("host", "device"):
            raise ValueError("jpegEncoder must be 'host' or 'device', got %r" % (self.jpegEncoder,))
        if self.jpegEncoder != "device" or not self.streamOutput or self.outputPyramid or str(outputfileExtension).lower() not in ("jpg", "jpeg"):
            return False
        if "mosaicSink" in self.__dict__ and not getattr(self.__dict__["mosaicSink"], "device_jpeg", False):
            return False
        self._routeNeeds("device_jpeg", "jpegEncoder = 'device'")
        if not 1 <= int(self.jpegQuality) <= 100:
            raise ValueError("jpegQuality must be 1..100, got %r" % (self.jpegQuality,))
        self._jpegBandRows()
        return True

    def _devicePng(self, outputfileExtension):
        """does this output go through the device's PNG coder (Method.pngEncoder = "device" with streamOutput and a .png result)?  Judged --
        with the engine's support, pngSegmentRows and mosaicBandRows -- before a file is listed or a tile decoded.  Everything else (other
        formats, outputPyramid, streamOutput = False, a mosaicSink of the user's) is written as with "host"."""
        if self.pngEncoder not in ("host", "device"):
            raise ValueError("pngEncoder must be 'host' or 'device', got %r" % (self.pngEncoder,))
        if self.pngEncoder != "device" or not self.streamOutput or self.outputPyramid or str(outputfileExtension).lower() != "png":
            return False
        if "mosaicSink" in self.__dict__ and not getattr(self.__dict__["mosaicSink"], "device_png", False):
            return False
        self._routeNeeds("device_png", "pngEncoder = 'device'")
        self._pngBandRows()
        return True

    def _pngBandRows(self):
        """mosaicBandRows for the device's PNG coder: every band must be whole segments, so it is a multiple of pngSegmentRows (1..4096)"""
        S = self.pngSegmentRows
        if isinstance(S, bool) or not isinstance(S, int) or not 1 <= S <= 4096:
            raise ValueError("pngSegmentRows must be an integer 1..4096, got %r" % (S,))
        return self._bandRows(S, "segments of %d rows need" % S)

    # The routes a fused canvas leaves the device by, and the engine method each needs.  A sink names its route: the flags `device_jpeg`
    # (it takes entropy-coded bands), `device_png` (the IDAT chunks of the bands' segments) and `device_tiles` (finished tile streams: JPEG's, or with `tile_codec` "deflate" the lossless coder's,
    # route "device_tiles_deflate"), the method `pyramid_levels` (pixel bands with reduced levels)
    _ROUTES = {"device_jpeg": "canvas_encode_jpeg_bands", "device_png": "canvas_encode_png_bands", "device_tiles": "canvas_encode_pyramid_tiles",
               "device_tiles_deflate": "canvas_encode_pyramid_tiles_deflate",
               "pyramid_levels": "canvas_download_pyramid_bands", "plain": "canvas_download_bands"}

    @staticmethod
    def _routeOf(sink):
        flagged = [route for route in ("device_jpeg", "device_png", "device_tiles") if getattr(sink, route, False)]
        if flagged == ["device_tiles"] and getattr(sink, "tile_codec", "jpeg") == "deflate":
            return "device_tiles_deflate"
        return flagged[0] if flagged else "pyramid_levels" if hasattr(sink, "pyramid_levels") else "plain"

    def _routeNeeds(self, route, what):
        if not hasattr(self.engine, self._ROUTES[route]):
            raise NotImplementedError("%s needs an engine with %s" % (what, self._ROUTES[route]))

    def _bandRows(self, step=0, whose=None):
        """Method.mosaicBandRows; with `step`, a positive multiple of it or ValueError: "<whose> mosaicBandRows to be a multiple of ..." """
        band_rows = int(getattr(self, "mosaicBandRows", 4096))
        if step and (band_rows <= 0 or band_rows % step):
            raise ValueError("%s mosaicBandRows to be a multiple of %d, got %d" % (whose, step, band_rows))
        return band_rows

    def _jpegBandRows(self):
        """mosaicBandRows for the device's JPEG encoder: every band must be whole restart intervals whatever the mosaic's width, so it is a
        multiple of the MCU height (16 rows in colour, 8 in gray) times jpegRestartMcus"""
        R = int(self.jpegRestartMcus)
        if not 1 <= R <= 65535:
            raise ValueError("jpegRestartMcus must be 1..65535, got %r" % (self.jpegRestartMcus,))
        return self._bandRows((16 if self.isColorMode else 8) * R, "restart intervals of %d MCUs need" % R)

    def _pyramidBandRows(self, levels):
        """mosaicBandRows for a pyramid of `levels` reduced levels: every band must form complete rows of every level"""
        return self._bandRows(1 << levels, "a pyramid of %d reduced levels needs" % levels)

    def _pyramidOptions(self):
        """Method.pyramid* as PyramidTiffBandWriter's keyword arguments"""
        return {"tile": self.pyramidTile, "levels": self.pyramidLevels, "compression": self.pyramidCompression,
                "quality": self.jpegQuality, "restart_mcus": self.jpegRestartMcus}

    def _checkPyramidOutput(self, outputfileExtension):
        """Method.outputPyramid, judged before a file is listed or a tile decoded"""
        if not self.outputPyramid:
            return
        if str(outputfileExtension).lower() not in ("tif", "tiff"):
            raise ValueError("outputPyramid needs a .tif or .tiff output, got outputfileExtension = %r" % (outputfileExtension,))
        if not self.streamOutput:
            raise ValueError("outputPyramid needs streamOutput: the levels are formed from the bands as they leave the device")
        jpeg = self.pyramidCompression == "jpeg"                 # the tiles are encoded on the device (csrc/jpeg_enc_kernels.hip in tile order)
        deflate = self.pyramidCompression == "deflate-device"    # likewise, losslessly (csrc/deflate_kernels.hip)
        self._routeNeeds("device_tiles" if jpeg else "device_tiles_deflate" if deflate else "pyramid_levels",
                         "outputPyramid" + (" with pyramidCompression = %r" % (self.pyramidCompression,) if jpeg or deflate else ""))
        writer = PyramidTiffBandWriter("", **self._pyramidOptions())       # (pyramidTile, pyramidLevels, pyramidCompression, jpegQuality, jpegRestartMcus: the writer's own refusals)
        if jpeg or deflate:
            if "mosaicSink" in self.__dict__:
                raise ValueError("pyramidCompression = %r writes the tile streams the device encodes; a mosaicSink of the user's takes pixel bands" % (self.pyramidCompression,))
            if jpeg:
                writer.check_jpeg_geometry(3 if self.isColorMode else 1)
            self._bandRows(writer.tile, "%s tiles of %d rows need" % ("JPEG" if jpeg else "deflate", writer.tile))
        if self.pyramidLevels is not None:
            self._pyramidBandRows(int(self.pyramidLevels))

    def _pyramidLevelsOf(self, full_shape):
        """how many reduced levels the installed mosaicSink wants with every band of a mosaic of `full_shape` (a sink with `pyramid_levels`:
        PyramidTiffBandWriter, or the user's own), or None: an ordinary sink, or none"""
        sink = getattr(self, "mosaicSink", None)
        if sink is None or not hasattr(sink, "pyramid_levels"):
            return None
        self._routeNeeds(self._routeOf(sink), "a mosaicSink with pyramid_levels")
        levels = int(sink.pyramid_levels(full_shape))
        self._pyramidBandRows(levels)
        return levels

    def _jpegDecoderOnDevice(self):
        """which device decoder does the ingest try first (Method.jpegDecoder)?  False for "host", else the value itself: "device" (the
        inverse DCT on the device) or "device-entropy" (the entropy decode too)"""
        if self.jpegDecoder not in ("host", "device", "device-entropy"):
            raise ValueError("jpegDecoder must be 'host', 'device' or 'device-entropy', got %r" % (self.jpegDecoder,))
        if self.jpegDecoder == "host":
            return False
        entry = "tile_fill_jpeg_dct" if self.jpegDecoder == "device" else "tile_fill_jpeg_huff"
        if not hasattr(self.engine, entry):
            raise NotImplementedError("jpegDecoder = %r needs an engine with %s" % (self.jpegDecoder, entry))
        return self.jpegDecoder

    def _decoderThreads(self, n_files):
        """size of the decoder pool: `decodeThreads`, or one per host core up to 32 when the library decodes JPEGs itself (measured on the
        256-thread host of the MI355X box, colour 2048 x 2048: 1354 tiles/s at 16 threads, 1804 at 32; Pillow: 1094 at 16 and no more beyond)"""
        native = getattr(self.engine, "tile_fill_jpeg", None) is not None and os.environ.get("VFSMS_NATIVE_JPEG", "1") != "0"
        return max(1, min(int(self.decodeThreads or min(os.cpu_count() or 4, 32 if native else 16)), n_files, 64))

    def _batchedMethod(self, caculateOffsetMethod, n_files):
        """which fused path serves `caculateOffsetMethod` ("surf" / "orb" / "phase": incremental ROI search; "surf_full" / "orb_full": whole-tile
        features, the line scans of Main.py:29-51), or None: a custom method or operators, the switch off, fewer than two files"""
        fn, owner = getattr(caculateOffsetMethod, "__func__", None), getattr(caculateOffsetMethod, "__self__", None)
        if not self.batchRegistration or owner is not self or n_files < 2:
            return None
        if fn is Stitcher.calculateOffsetForFeatureSearchIncre and self._usesStockOperators():
            return self.featureMethod
        if fn is Stitcher.calculateOffsetForPhaseCorrleateIncre and (not self.phaseSignFix or self.phaseResolve != "none"):
            return "phase"
        # (with offsetVerify the line scans stay pair by pair: whole-tile feature sets carry no pixels, calculateOffsetForFeatureSearch
        # checks the two tiles themselves after the vote)
        if fn is Stitcher.calculateOffsetForFeatureSearch and self._usesStockOperators() and self.offsetCaculate in ("mode", "ransac") \
                and self.offsetVerify == "none":
            if self.featureMethod == "surf" and hasattr(self.engine, "features_surf_batch"):
                return "surf_full"
            if self.featureMethod == "orb" and not self.isEnhance and hasattr(self.engine, "attempt_orb_batch"):
                return "orb_full"
        return None

    def _makeRegistrar(self, method, n_files):
        """the GridRegistrar of one file list, primed with what the previous dataset taught this stitcher (accepted directions, same number of
        tiles: GridRegistrar.path_memory; Main.py runs its datasets through ONE Stitcher with one setting) or with the operator's pathHint"""
        from .grid import GridRegistrar
        params = None if method in ("phase", "sift") else (self._orbParams() if method in ("orb", "orb_full") else self._surfParams())
        sift = self._siftParams() if method == "sift" else None
        reg = GridRegistrar(self.engine, method="surf" if method == "surf_full" else "orb" if method == "orb_full" else method, roiRatio=self.roiRatio,
                            searchRatio=self.searchRatio, offsetEvaluate=self.offsetEvaluate, directIncre=self.directIncre, surfParams=params,
                            phaseResponseThreshold=self.phaseResponseThreshold, window=48,
                            enhance=self._enhanceSpec() if method in ("surf", "surf_full") else (0, 0.0, 0),
                            offsetCaculate=self.offsetCaculate if method != "phase" else "mode", ransacThreshold=self.ransacThreshold, siftParams=sift,
                            offsetVerify=self.offsetVerify if method != "phase" else "none", verifyThreshold=self.verifyThreshold,
                            verifyMinPixels=self.verifyMinPixels, phaseResolve=self.phaseResolve, phasePeaks=self.phasePeaks,
                            phaseResolveThreshold=self.phaseResolveThreshold, phaseResolveMinPixels=self.phaseResolveMinPixels)
        reg.orbMaxDistance = self.orbMaxDistance if self.isGPUAvailable else -1
        reg.path_memory = self.__dict__.get("_pathMemory")
        reg.path_suspect = bool(self.__dict__.get("_pathSuspect", False))
        return reg

    def _operatorHint(self, reg, n_pairs):
        """the operator's pathHint as a CALLER'S hint of register() -- never installed as the registrar's memory, so it is not put on trial
        (GridRegistrar._learn tries memories only) -- and only while the registrar has no memory of its own for this path length; once a
        learned memory was dropped for mispredicting twice in a row, the next path runs cold as _learn promises (the hint is not slipped
        back in its place)."""
        m = reg.path_memory
        if (m is not None and len(m) == n_pairs) or self.pathHint is None or len(self.pathHint) != n_pairs:
            return None
        if self.__dict__.get("_pathMemoryDropped", False):
            return None
        return [int(d) for d in self.pathHint]

    def _registerBatched(self, fileList, caculateOffsetMethod):
        """The pair loop of flowStitch (Stitcher.py:64-79) through grid.GridRegistrar when `caculateOffsetMethod` is this
        object's own calculateOffsetForFeatureSearchIncre / calculateOffsetForPhaseCorrleateIncre with the stock operators:
        all tiles go to the GPU once (ingest.TileIngest: reserved handles filled by a pool of decoder threads while the registrar already
        works) and the pairs are registered in speculative fused batches whose selected results equal the pair-by-pair search (same
        offsets, same self.direction threading, same log lines).  Returns None when the sequential loop has to run (custom method or
        operators, tiles of different sizes, switch off) else (status, endfileIndex, offsetList, description of the break)."""
        method = self._batchedMethod(caculateOffsetMethod, len(fileList))
        if method is None:
            return None
        eng = self.engine
        shapes = [_imshape(f) for f in fileList]             # from the file headers: nothing is decoded yet
        if any(s != shapes[0] for s in shapes):
            return None
        reg = self._makeRegistrar(method, len(fileList))
        device_fuse = (self.fuseMethod in ("notFuse", "fadeInAndFadeOut", "trigonometric") and hasattr(eng, "canvas_fuse_tile_resident")) or \
                      (self.fuseMethod in ("average", "maximum", "minimum") and hasattr(eng, "canvas_blend_tile_resident")) or \
                      (self.fuseMethod == "multiBandBlending" and hasattr(eng, "canvas_fuse_tile_resident") and hasattr(eng, "canvas_set_multiband_levels")) or \
                      (self.fuseMethod == "optimalSeamLine" and hasattr(eng, "canvas_fuse_tile_resident") and hasattr(eng, "canvas_set_seam_blend"))
        # the tiles the mosaic is assembled from stay in HBM: the registration planes themselves for gray mosaics, and for colour mosaics
        # (Main.py:14's default) the B G R tiles the SAME decode produced -- every file is decoded exactly once (Stitcher.py:68-69, 382-403)
        color = bool(self.isColorMode) and device_fuse and hasattr(eng, "tile_fill_pair")
        keep = device_fuse and (color or not self.isColorMode) and len(set(fileList)) == len(fileList)
        job = TileIngest(self, fileList, shapes, color, keep)
        table = None
        try:
            handles = job.start()
            if method == "surf_full":
                table = self._fullImageTable(handles)
            elif method == "orb_full":
                table = self._fullImageTableOrb(handles, shapes)
            else:
                had_memory = reg.path_memory is not None
                # failedPairRepair = "stage": every pair is reported (a failed one leaves the direction untouched), and the repair below
                # decides where the mosaic breaks
                table, _d = reg.register(handles, shapes, self.direction, stop_on_fail=self.failedPairRepair != "stage",
                                         hint=self._operatorHint(reg, len(shapes) - 1))
                # (what this path taught, incl. "nothing": a memory that mispredicted twice in a row is dropped, GridRegistrar._learn)
                self._pathMemory, self._pathSuspect = reg.path_memory, reg.path_suspect
                self._pathMemoryDropped = had_memory and reg.path_memory is None
            repaired = {}
            if self.failedPairRepair == "stage" and method not in ("surf_full", "orb_full") and not all(row[0] for row in table):
                table, repaired = self._repairTable(handles, shapes, table, reg.repair)      # while the registration planes are resident
            adjusted = None
            if self.globalAdjust != "none":                  # while the registration planes are still resident (finish releases them)
                n_ok = 0
                while n_ok < len(table) and table[n_ok][0]:
                    n_ok += 1
                voted = [[int(table[k][1]), int(table[k][2])] for k in range(n_ok)]
                adjusted = self._globalAdjust(fileList[:n_ok + 1], voted, handles[:n_ok + 1], shapes[:n_ok + 1], log=False)
        except BaseException:
            job.failed = True
            raise
        finally:
            job.finish(table)
        offsetList, endfileIndex, status, describtion = [], 0, True, ""
        for k, row in enumerate(table):
            self.printAndWrite("stitching " + str(fileList[k]) + " and " + str(fileList[k + 1]))
            if not row[0]:
                status = False
                describtion = "  " + str(fileList[k]) + " and " + str(fileList[k + 1]) + " can not be stitched"
                break
            if k in repaired:
                self.printAndWrite(self._repairLine(fileList[k], fileList[k + 1], repaired[k]))
            if method not in ("surf_full", "orb_full"):
                self.direction = int(row[3])
            self.printAndWrite("  The offset of stitching: dx is " + str(int(row[1])) + " dy is " + str(int(row[2])))
            offsetList.append([int(row[1]), int(row[2])])
            endfileIndex = k + 1
        if adjusted is not None and adjusted[1] is not None:
            self.printAndWrite(adjusted[1])
            offsetList = adjusted[0]
        return (status, endfileIndex, offsetList, describtion)

    repairReport = None          # the report of the last failedPairRepair = "stage" run (stage.repair_table)

    def _checkRepairOptions(self):
        """Method.failedPairRepair and its parameters, judged before a file is listed or a tile decoded"""
        if self.failedPairRepair == "none":
            return
        if self.failedPairRepair != "stage":
            raise ValueError("failedPairRepair must be 'none' or 'stage', got %r" % (self.failedPairRepair,))
        R, f, K = int(self.repairRadius), int(self.repairFactor), int(self.repairPeaks)
        if not 1 <= R <= 128:
            raise ValueError("repairRadius must lie in 1..128, got %r" % (self.repairRadius,))
        if f not in (2, 4, 8):
            raise ValueError("repairFactor must be 2, 4 or 8, got %r" % (self.repairFactor,))
        if -(-R // f) > 16:
            raise ValueError("repairRadius %d at repairFactor %d leaves a coarse radius of %d (at most 16)" % (R, f, -(-R // f)))
        if not 1 <= K <= 4:
            raise ValueError("repairPeaks must lie in 1..4, got %r" % (self.repairPeaks,))
        if int(self.repairMinPixels) < 0 or not float(self.repairBlankRatio) >= 0.0:
            raise ValueError("repairMinPixels and repairBlankRatio must not be negative")
        if not hasattr(self.engine, "ncc_wide_batch") or not hasattr(self.engine, "overlap_sums_batch"):
            raise NotImplementedError("this engine has no wide correlation search (failedPairRepair = %r)" % (self.failedPairRepair,))

    def _repairTable(self, handles, shapes, table, repair=None):
        """failedPairRepair = "stage" on a result table over resident gray tiles -> (the repaired table, CUT at the first pair that stays
        unresolved -- that row is the break, the rows behind it are zero as stop_on_fail leaves them -- and {pair: its report entry} of the
        repaired pairs).  repair: GridRegistrar.repair of the registrar that made the table, default stage.repair_table on this engine."""
        if repair is None:
            from .stage import repair_table
            repair = lambda h, s, t, **kw: repair_table(self.engine, h, s, t, **kw)      # noqa: E731
        fixed, report = repair(handles, [tuple(s[:2]) for s in shapes], table, hint=self.pathHint, radius=int(self.repairRadius),
                               factor=int(self.repairFactor), peaks=int(self.repairPeaks), threshold=float(self.repairThreshold),
                               min_pixels=int(self.repairMinPixels), blank_ratio=float(self.repairBlankRatio))
        self.repairReport = report
        fixed = np.array(fixed, np.int32).reshape(-1, 6)
        bad = np.flatnonzero(fixed[:, 0] != 1)
        if len(bad):
            fixed[bad[0]:] = 0
        return fixed, {e["pair"]: e for e in report["pairs"] if e["kind"] != "unresolved"}

    @staticmethod
    def _repairLine(fileA, fileB, entry):
        how = "measured, score %.3f" % entry["score"] if entry["kind"] == "measured" else "predicted"
        return "  " + str(fileA) + " and " + str(fileB) + " can not be registered: repaired from the stage model (" + how + ")"

    def _repairPairLoop(self, fileList, rows):
        """the repair behind flowStitch's pair-by-pair loop: `rows` holds a result row per pair (failed ones zero).  The gray tiles are
        decoded and uploaded for the call the way _globalAdjust does, and freed.  -> (status, endfileIndex, offsetList, description)"""
        own = []
        try:
            shapes = []
            for f in fileList:
                img = _imread(f, False)
                shapes.append(img.shape[:2])
                own.append(self.engine.tile_upload(img))
            table, repaired = self._repairTable(own, shapes, rows)
        finally:
            for h in own:
                self.engine.tile_free(h)
        offsetList, endfileIndex, status, describtion = [], 0, True, ""
        for k, row in enumerate(table):
            if not row[0]:
                status = False
                describtion = "  " + str(fileList[k]) + " and " + str(fileList[k + 1]) + " can not be stitched"
                break
            if k in repaired:
                self.printAndWrite(self._repairLine(fileList[k], fileList[k + 1], repaired[k]))
                self.printAndWrite("  The offset of stitching: dx is " + str(int(row[1])) + " dy is " + str(int(row[2])))
            offsetList.append([int(row[1]), int(row[2])])
            endfileIndex = k + 1
        return (status, endfileIndex, offsetList, describtion)

    def _globalAdjust(self, fileList, offsetList, handles=None, shapes=None, log=True):
        """globalAdjust = "ncc" for one registered segment (adjust.adjust_offsets): the adjusted offsetList, or the list as it is for a
        segment of fewer than 3 tiles or tiles of different sizes.  handles / shapes: the segment's resident gray tiles; without them the
        files are decoded and uploaded for the call.  log=False returns (offsetList, the line to log or None) instead of logging."""
        from .adjust import adjust_offsets
        if self.globalAdjust != "ncc":
            raise ValueError("globalAdjust must be 'none' or 'ncc'")
        line, own = None, []
        if len(offsetList) >= 2:
            try:
                if handles is None:
                    shapes = []
                    for f in fileList:
                        img = _imread(f, False)
                        shapes.append(img.shape[:2])
                        own.append(self.engine.tile_upload(img))
                    handles = own
                if any(tuple(s[:2]) != tuple(shapes[0][:2]) for s in shapes):
                    line = "  The tiles are of different sizes: the offsetList is not adjusted"
                else:
                    offsetList, self.adjustReport = adjust_offsets(self.engine, handles, [tuple(s[:2]) for s in shapes], offsetList, self.adjustRadius,
                                                                   self.adjustThreshold, self.adjustMinPixels)
                    line = "  The adjusted offsetList is " + str(offsetList)
            finally:
                for h in own:
                    self.engine.tile_free(h)
        if not log:
            return offsetList, line
        if line is not None:
            self.printAndWrite(line)
        return offsetList

    def _fullImageTable(self, handles):
        """calculateOffsetForFeatureSearch (Stitcher.py:260-304) over consecutive resident tiles, batched: every tile is described once
        (vfsms_features_surf_batch: 16 tiles per fused launch sequence -- the reference's B -> A feature reuse, Stitcher.py:278-290, taken
        to its end), the N - 1 matches + mode votes are ONE batch.  Rows as the incremental registrar's: (status, dx, dy, 0, 0, votes);
        like the pair loop, nothing behind the first pair that cannot be matched is reported (flowStitch breaks there)."""
        eng = self.engine
        feats, counts = eng.features_surf_batch(handles, self._surfParams(), self._enhanceSpec())
        try:
            with self._offsetEstimator():
                rows = eng.features_match_offset_batch(feats[:-1], feats[1:], self.searchRatio, self.offsetEvaluate)
        finally:
            for f in feats:
                if f:
                    eng.features_free(f)
        table = []
        for r in rows:
            table.append([int(r[0]), int(r[1]), int(r[2]), 0, 0, int(r[3])])
            if not r[0]:
                break
        self.tempImageFeature.isBreak = True                  # the scan owns no cached set afterwards
        return table

    def _fullImageTableOrb(self, handles, shapes, chunk=16):
        """calculateOffsetForFeatureSearch (Stitcher.py:260-304) with featureMethod = "orb" over consecutive resident tiles: the N - 1
        whole-tile attempts (ORB of both tiles, BF-Hamming 1-NN, mode vote) as fused batches of `chunk` pairs.  A tile is described as B of
        one pair and again as A of the next -- the reference reuses B's features (Stitcher.py:278-290), which are the same numbers -- so the
        rows are those of the pair loop; nothing behind the first pair that cannot be matched is reported (flowStitch breaks there)."""
        eng = self.engine
        max_dist = self.orbMaxDistance if self.isGPUAvailable else -1
        table = []
        for c0 in range(0, len(handles) - 1, chunk):
            jobs = [(handles[k], handles[k + 1], 0, 0, 0, 0, shapes[k][0], shapes[k][1]) for k in range(c0, min(c0 + chunk, len(handles) - 1))]
            with self._offsetEstimator():
                rows = eng.attempt_orb_batch(jobs, self._orbParams(), max_dist, self.offsetEvaluate)
            for r in rows:
                ok = bool(r[0]) and r[4] > 0 and r[5] > 0          # an image without keypoints: featuresX is None, status stays False
                table.append([int(ok), int(r[1]), int(r[2]), 0, 0, int(r[3])])
                if not ok:
                    self.tempImageFeature.isBreak = True
                    return table
        self.tempImageFeature.isBreak = True                  # the scan owns no cached set afterwards
        return table

    def flowStitchWithMutiple(self, fileList, caculateOffsetMethod):
        """Stitcher.py:96-127: restart after every registration break; a trailing lone tile is its own result."""
        result = []
        totalNum = len(fileList)
        startNum = 0
        self._ingestCache = {}                                # tiles decoded behind a break wait here for the segment that uses them
        try:
            while 1:
                (status, stitchResult) = self.flowStitch(fileList[startNum: totalNum], caculateOffsetMethod)
                result.append(stitchResult)
                self.tempImageFeature.isBreak = True
                startNum = startNum + status[1] + 1
                if startNum == totalNum:
                    break
                if startNum == (totalNum - 1):
                    result.append(self._loneTile(fileList[startNum]))
                    break
                self.printAndWrite("stitching Break, start from " + str(fileList[startNum]) + " again")
        finally:
            for g, c, _shape in self.__dict__.pop("_ingestCache", {}).values():
                for h in (g, c):
                    if h:
                        try:
                            self.engine.tile_free(h)
                        except Exception:
                            pass
        return result

    def _loneTile(self, path):
        """the trailing tile that is a result of its own (Stitcher.py:119-121): from the device copy a broken segment left behind, else decoded"""
        ent = (self.__dict__.get("_ingestCache") or {}).get(path)
        eng = self.engine
        if ent is not None and hasattr(eng, "canvas_paste_tile") and (bool(ent[1]) or not self.isColorMode):
            h, ch = (ent[1], 3) if self.isColorMode else (ent[0], 1)
            cv = eng.canvas_create(ent[2][0], ent[2][1], ch)
            try:
                eng.canvas_paste_tile(cv, h, 0, 0)
                return eng.canvas_download(cv, ent[2][0], ent[2][1], ch)
            finally:
                eng.canvas_free(cv)
        return _imread(path, self.isColorMode)

    def imageSetStitch(self, projectAddress, outputAddress, fileNum, caculateOffsetMethod, startNum=1, fileExtension="jpg", outputfileExtension="jpg"):
        """Stitcher.py:129-151."""
        self._checkPyramidOutput(outputfileExtension)
        self._deviceJpeg(outputfileExtension)
        self._devicePng(outputfileExtension)
        self._checkRepairOptions()
        for i in range(startNum, fileNum + 1):
            fileList = _list_images(_join(projectAddress, i), fileExtension)
            outDir = outputAddress.replace("\\", os.sep)
            if not os.path.exists(outDir):
                os.makedirs(outDir)
            Stitcher.outputAddress = outDir if outDir.endswith(os.sep) else outDir + os.sep
            outPath = os.path.join(outDir, "stitching_result_" + str(i) + "." + outputfileExtension)
            # streamed results are encoded under a hidden name and renamed when the mosaic is complete: an exception in the middle of
            # an assembly must not leave a truncated file under the result's name
            partPath = os.path.join(outDir, ".stitching_part_" + str(i) + "." + outputfileExtension)
            streamed = self._streamTo([partPath]) if self.streamOutput else None
            done = False
            try:
                (status, result) = self.flowStitch(fileList, caculateOffsetMethod)
                done = True
            finally:
                if streamed is not None:
                    self.__dict__.pop("mosaicSink", None)
                    if not done and os.path.exists(partPath):
                        os.remove(partPath)
            self.tempImageFeature.isBreak = True
            if result is None and streamed is not None:
                os.replace(partPath, outPath)
            else:
                if streamed is not None and os.path.exists(partPath):
                    os.remove(partPath)
                _imwrite(outPath, result)
            if status == False:
                self.printAndWrite("stitching Failed")

    def imageSetFocusStack(self, projectAddress, stackedAddress, fileNum, startNum=1, fileExtension="jpg", outputfileExtension="png"):
        """Method.focusStack in front of the pipeline (no reference counterpart; focus.fuse_dataset, tests/focus_ref.py): the folders
        projectAddress/i of imageSetStitch, each holding focusPlanes consecutive files per stage position, go to stackedAddress/i with one
        fused tile per position, which the unchanged imageSetStitch* then reads.  -> the files written, folder by folder."""
        from .focus import check_options, fuse_dataset
        if self.focusStack == "none":
            raise ValueError("imageSetFocusStack needs focusStack = 'pixel' or 'plane' (it is 'none')")
        check_options(self.focusStack, self.focusPlanes, self.focusRadius, self.focusMedian)      # before a file is listed
        if not hasattr(self.engine, "focus_stack"):
            raise NotImplementedError("this engine has no focus stacking (focusStack = %r)" % (self.focusStack,))
        written = []
        for i in range(startNum, fileNum + 1):
            fileList = _list_images(_join(projectAddress, i), fileExtension)
            written.append(fuse_dataset(self, fileList, int(self.focusPlanes), _join(stackedAddress, i), outputfileExtension))
        return written

    def imageSetStitchWithMutiple(self, projectAddress, outputAddress, fileNum, caculateOffsetMethod, startNum=1, fileExtension="jpg", outputfileExtension="jpg"):
        """Stitcher.py:153-182 (the entry point Main.py:20-51 uses)."""
        self._checkPyramidOutput(outputfileExtension)
        self._deviceJpeg(outputfileExtension)
        self._devicePng(outputfileExtension)
        self._checkRepairOptions()
        for i in range(startNum, fileNum + 1):
            startTime = time.time()
            fileAddress = _join(projectAddress, i)
            fileList = _list_images(fileAddress, fileExtension)
            outDir = outputAddress.replace("\\", os.sep)
            if not os.path.exists(outDir):
                os.makedirs(outDir)
            Stitcher.outputAddress = outDir if outDir.endswith(os.sep) else outDir + os.sep   # printAndWrite appends the file name
            parts = []
            streamed = self._streamTo(parts, os.path.join(outDir, ".stitching_part_" + str(i) + "_%d." + outputfileExtension)) if self.streamOutput else None
            done = False
            try:
                result = self.flowStitchWithMutiple(fileList, caculateOffsetMethod)
                done = True
            finally:
                if streamed is not None:
                    self.__dict__.pop("mosaicSink", None)
                    if not done:                              # no part file outlives a failed dataset
                        for q in parts:
                            if os.path.exists(q):
                                os.remove(q)
            self.tempImageFeature.isBreak = True
            names = ([os.path.join(outDir, "stitching_result_" + str(i) + "." + outputfileExtension)] if len(result) == 1 else
                     [os.path.join(outDir, "stitching_result_" + str(i) + "_" + str(j + 1) + "." + outputfileExtension) for j in range(len(result))])
            streamedParts = iter(parts)
            for j in range(0, len(result)):
                if result[j] is None:                         # streamed while it was assembled: the part file takes the reference's name
                    os.replace(next(streamedParts), names[j])
                else:
                    _imwrite(names[j], result[j])
            endTime = time.time()
            print("Time Consuming for " + fileAddress + " is " + str(endTime - startTime))

    # ------------------------------------------------------------------------------------------------
    def calculateOffsetForPhaseCorrleate(self, dirAddress):
        """Stitcher.py:184-203 dereferences `self.phase`, which the reference never defines (dead code);
        the same AttributeError is raised here.  Use calculateOffsetForPhaseCorrleateIncre."""
        raise AttributeError("'Stitcher' object has no attribute 'phase'")

    # -- device tile cache: consecutive pairs share a tile (B of pair k is A of pair k+1) ---------------
    _TILE_CACHE = 4

    def _tileHandles(self, images):
        """Handles of the tiles of ONE job, resolved together: least-recently-used entries are evicted only after every
        tile of the job has its handle, and never a tile of the job itself.  An entry is keyed by the array object and its
        buffer address / shape / strides (a new array at a recycled id() must not hit); in-place edits of a cached array are
        not detected -- the reference's drivers decode a fresh array per tile."""
        cache = self.__dict__.setdefault("_tiles", [])
        eng = self.engine
        out = []
        for image in images:
            key = (id(image), image.__array_interface__["data"][0], image.shape, image.strides)
            for n, ent in enumerate(cache):
                if ent[0] is image and ent[1] == key:
                    cache.append(cache.pop(n))            # refresh on a hit (LRU)
                    out.append(ent[2])
                    break
            else:
                h = eng.tile_upload(image)
                cache.append((image, key, h))
                out.append(h)
        keep = set(out)
        n = 0
        while len(cache) > max(self._TILE_CACHE, len(keep)) and n < len(cache):
            if cache[n][2] in keep:
                n += 1
                continue
            eng.tile_free(cache.pop(n)[2])
        return out

    def releaseTiles(self):
        """Free the device copies the pair-by-pair methods cached (called at the end of every flowStitch)."""
        for _img, _key, h in self.__dict__.pop("_tiles", []):
            try:
                self.engine.tile_free(h)
            except Exception:
                pass
        if isinstance(self.tempImageFeature.feature, ResidentFeatures):
            # the device copy goes with the tiles; the cache keeps the (downloaded) arrays so that it still reads like the reference's
            rf = self.tempImageFeature.feature
            if rf.handle is not None:
                kps, desc = rf.arrays()
                rf.release()
                self.tempImageFeature.kps, self.tempImageFeature.feature = kps, desc

    def _usesStockOperators(self):
        c = type(self)
        stock_offset = ((self.offsetCaculate == "mode" and c.getOffsetByMode is Utility.Method.getOffsetByMode)
                        or (self.offsetCaculate == "ransac" and c.getOffsetByRansac is Utility.Method.getOffsetByRansac))
        return (c.detectAndDescribe is Utility.Method.detectAndDescribe and c.matchDescriptors is Utility.Method.matchDescriptors
                and stock_offset and (not self.isEnhance or self.featureMethod == "surf") and self.featureMethod in ("surf", "orb", "sift")
                and (self.featureMethod != "sift" or self._engineFusesSift()))

    def _engineFusesSift(self):
        """the engine offers attempt_sift_batch, and its detector is that same engine's: a wrapper that substitutes its own
        sift_detect_describe (and hands everything else through) is a user's operator like an overridden detectAndDescribe, and keeps the
        generic path"""
        batch, detect = getattr(self.engine, "attempt_sift_batch", None), getattr(self.engine, "sift_detect_describe", None)
        return batch is not None and detect is not None and getattr(batch, "__self__", None) is getattr(detect, "__self__", None)

    def _offsetEstimator(self):
        """scope of a fused engine call: with offsetCaculate = "ransac" its vote tail is the consensus of getOffsetByRansac"""
        return offset_estimator(self.engine, self.offsetCaculate, self.ransacThreshold)

    def _voteTail(self):
        """scope of a fused ATTEMPT call (its jobs name the strips' pixels): the estimator, and with offsetVerify = "ncc" the overlap check
        behind its vote"""
        return vote_tail(self.engine, self.offsetCaculate, self.ransacThreshold, self.offsetVerify, self.verifyThreshold, self.verifyMinPixels)

    def _verified(self, status, offset, rawA, rawB):
        """the host operators' vote behind Method.verifyOffset on the raw pixels; offsetVerify = "none" makes no call"""
        if status and self.offsetVerify != "none":
            status = self.verifyOffset(rawA, rawB, offset)[0]
        return status

    def _enhanceSpec(self):
        """(mode, clipLimit, tileSize) of Stitcher.py:269-276 / 327-334: 0 none, 1 cv2.equalizeHist, 2 cv2.createCLAHE(...).apply."""
        if not self.isEnhance:
            return (0, 0.0, 0)
        return (2, float(self.clipLimit), int(self.tileSize)) if self.isClahe else (1, 0.0, 0)

    def _enhance(self, image):
        mode, clip, tiles = self._enhanceSpec()
        return image if mode == 0 else self.engine.enhance(np.asarray(image), mode, clip, tiles)

    def _featureAttempt(self, imageA, imageB, direction, searchRatio):
        """One pass of the loop body at Stitcher.py:322-345 -> (status, [dx, dy]) or None when an image has no features."""
        if self._usesStockOperators():
            ra = roi_rect(imageA.shape, direction, "first", searchRatio)
            rb = roi_rect(imageB.shape, direction, "second", searchRatio)
            if ra[2:] == rb[2:] and ra[2] > 0 and ra[3] > 0:
                ha, hb = self._tileHandles([imageA, imageB])
                job = (ha, hb, ra[0], ra[1], rb[0], rb[1], ra[2], ra[3])
                with self._voteTail():
                    if self.featureMethod == "orb":
                        max_dist = self.orbMaxDistance if self.isGPUAvailable else -1
                        row = self.engine.attempt_orb_batch([job], self._orbParams(), max_dist, self.offsetEvaluate)[0]
                    elif self.featureMethod == "sift":
                        row = self.engine.attempt_sift_batch([job], self._siftParams(), self.searchRatio, self.offsetEvaluate)[0]
                    elif self.isEnhance:
                        row = self.engine.attempt_surf_batch_enhanced([job], self._surfParams(), self.searchRatio, self.offsetEvaluate, self._enhanceSpec())[0]
                    else:
                        row = self.engine.attempt_surf_batch([job], self._surfParams(), self.searchRatio, self.offsetEvaluate)[0]
                if row[4] == 0 or row[5] == 0:
                    return None                      # featuresA is None or featuresB is None: status untouched
                return (bool(row[0]), [int(row[1]), int(row[2])])
        roiImageA = self.getROIRegionForIncreMethod(imageA, direction=direction, order="first", searchRatio=searchRatio)
        roiImageB = self.getROIRegionForIncreMethod(imageB, direction=direction, order="second", searchRatio=searchRatio)
        rawA, rawB = roiImageA, roiImageB
        if self.isEnhance:                                     # Stitcher.py:327-334
            roiImageA = self._enhance(roiImageA)
            roiImageB = self._enhance(roiImageB)
        kpsA, featuresA = self.detectAndDescribe(roiImageA, featureMethod=self.featureMethod)
        kpsB, featuresB = self.detectAndDescribe(roiImageB, featureMethod=self.featureMethod)
        if featuresA is not None and featuresB is not None:
            matches = self.matchDescriptors(featuresA, featuresB)
            if self.offsetCaculate == "mode":
                (status, offset) = self.getOffsetByMode(kpsA, kpsB, matches, offsetEvaluate=self.offsetEvaluate)
            else:
                (status, offset, _adjustH) = self.getOffsetByRansac(kpsA, kpsB, matches, offsetEvaluate=self.offsetEvaluate)
            return (self._verified(status, offset, rawA, rawB), offset)
        return None

    def _phaseResolve(self, roiImageA, roiImageB):
        """phaseResolve = "ncc" on two ROI strips -> (status, [dx, dy]), a raw vote in the feature path's convention (tests/phase_resolve_ref.py)"""
        if self.phaseResolve != "ncc":
            raise ValueError("phaseResolve must be 'none' or 'ncc'")
        fn = getattr(self.engine, "phase_resolve", None)
        if fn is None:
            raise NotImplementedError("this engine has no phase resolver (phaseResolve = %r)" % (self.phaseResolve,))
        row = fn(np.asarray(roiImageA), np.asarray(roiImageB), self.phasePeaks, self.phaseResolveThreshold, self.phaseResolveMinPixels)[0]
        return (bool(row[0]), [int(row[1]), int(row[2])])

    def _phaseCorrelate(self, roiImageA, roiImageB):
        """cv2.phaseCorrelate(np.float64(a), np.float64(b)) at Stitcher.py:230 -> ((x, y), response)."""
        return self.engine.phase_correlate(roiImageA, roiImageB)

    def _axisCorrection(self, offset, localDirection, i, imageA, imageB):
        """Stitcher.py:244-251 / 353-360: put the ROI-relative vote back into full-tile coordinates."""
        if localDirection == 1:
            offset[0] = offset[0] + imageA.shape[0] - int(i * self.roiRatio * imageA.shape[0])
        elif localDirection == 2:
            offset[1] = offset[1] + imageA.shape[1] - int(i * self.roiRatio * imageA.shape[1])
        elif localDirection == 3:
            offset[0] = offset[0] - (imageB.shape[0] - int(i * self.roiRatio * imageB.shape[0]))
        elif localDirection == 4:
            offset[1] = offset[1] - (imageB.shape[1] - int(i * self.roiRatio * imageB.shape[1]))
        return offset

    def _maxI(self):
        return int(np.floor(0.5 / self.roiRatio) + 1) + 1     # Stitcher.py:217,316

    def calculateOffsetForPhaseCorrleateIncre(self, images):
        """Stitcher.py:205-258: incremental ROI x direction rotation around FP64 phase correlation.
        offset = [int(y), int(x)] (truncation), accepted when response > phaseResponseThreshold."""
        (imageA, imageB) = images
        offset = [0, 0]
        status = False
        iniDirection = self.direction
        localDirection = iniDirection
        for i in range(1, self._maxI()):
            while True:
                roiImageA = self.getROIRegionForIncreMethod(imageA, direction=localDirection, order="first", searchRatio=i * self.roiRatio)
                roiImageB = self.getROIRegionForIncreMethod(imageB, direction=localDirection, order="second", searchRatio=i * self.roiRatio)
                if self.phaseResolve != "none":        # opt-in, no reference counterpart: see the class attribute
                    (status, offset) = self._phaseResolve(roiImageA, roiImageB)
                else:
                    (offsetTemp, response) = self._phaseCorrelate(roiImageA, roiImageB)
                    offset[0] = int(offsetTemp[1])
                    offset[1] = int(offsetTemp[0])
                    if self.phaseSignFix:                  # opt-in, not the reference's behaviour: see the class attribute
                        offset[0], offset[1] = -offset[0], -offset[1]
                    if response > self.phaseResponseThreshold:
                        status = True
                if status == True:
                    break
                else:
                    localDirection = self.directionIncrease(localDirection)
                if localDirection == iniDirection:
                    break
            if status == True:
                offset = self._axisCorrection(offset, localDirection, i, imageA, imageB)
                self.direction = localDirection
                break
        if status == False:
            return (status, CANNOT_MATCH)
        self.printAndWrite("  The offset of stitching: dx is " + str(offset[0]) + " dy is " + str(offset[1]))
        return (status, offset)

    def calculateOffsetForFeatureSearch(self, images):
        """Stitcher.py:260-304: whole-tile features; tile B's features are reused as tile A's of the next pair."""
        (imageA, imageB) = images
        offset = [0, 0]
        status = False
        if self._usesStockOperators() and self.featureMethod == "surf" and hasattr(self.engine, "features_surf"):
            return self._featureSearchResident(imageA, imageB)
        rawA, rawB = imageA, imageB
        if self.isEnhance == True:                              # Stitcher.py:269-276
            imageA = self._enhance(imageA)
            imageB = self._enhance(imageB)
        if self.tempImageFeature.isBreak == True:
            (kpsA, featuresA) = self.detectAndDescribe(imageA, featureMethod=self.featureMethod)
            (kpsB, featuresB) = self.detectAndDescribe(imageB, featureMethod=self.featureMethod)
        else:
            kpsA = self.tempImageFeature.kps
            featuresA = self.tempImageFeature.feature
            (kpsB, featuresB) = self.detectAndDescribe(imageB, featureMethod=self.featureMethod)
        self.tempImageFeature.isBreak = False
        self.tempImageFeature.kps = kpsB
        self.tempImageFeature.feature = featuresB
        if featuresA is not None and featuresB is not None:
            matches = self.matchDescriptors(featuresA, featuresB)
            if self.offsetCaculate == "mode":
                (status, offset) = self.getOffsetByMode(kpsA, kpsB, matches, offsetEvaluate=self.offsetEvaluate)
            elif self.offsetCaculate == "ransac":
                (status, offset, adjustH) = self.getOffsetByRansac(kpsA, kpsB, matches, offsetEvaluate=self.offsetEvaluate)
            status = self._verified(status, offset, rawA, rawB)
        if status == False:
            self.tempImageFeature.isBreak = True
            return (status, CANNOT_MATCH)
        self.tempImageFeature.isBreak = False
        self.printAndWrite("  The offset of stitching: dx is " + str(offset[0]) + " dy is " + str(offset[1]))
        return (status, offset)

    def _featureSearchResident(self, imageA, imageB):
        """calculateOffsetForFeatureSearch with the stock SURF operators, device resident: tile B's keypoints + descriptors stay in
        HBM and become tile A's of the next pair (Stitcher.py:278-290), the optional enhancement (Stitcher.py:269-276) runs on the
        device in front of the detector, and matching + mode vote read both sets where they are -- eight ints return per pair."""
        eng = self.engine
        tf = self.tempImageFeature
        params, enh = self._surfParams(), self._enhanceSpec()
        dim = 128 if params.extended else 64

        def describe(image):
            (h,) = self._tileHandles([image])
            f, n = eng.features_surf(h, (0, 0, image.shape[0], image.shape[1]), params, enh)
            return ResidentFeatures(eng, f, n, dim)
        prev = tf.feature if isinstance(tf.feature, ResidentFeatures) and tf.feature.handle is not None else None
        if tf.isBreak == True or prev is None:
            if prev is not None:
                prev.release()
            featA = describe(imageA)
        else:
            featA = prev
        try:
            featB = describe(imageB)
        except Exception:
            featA.release()                                     # nothing cached may point at a set that is gone
            tf.isBreak, tf.kps, tf.feature = True, None, None
            raise
        tf.isBreak = False
        tf.kps = featB if featB.n else np.float32([])
        tf.feature = featB if featB.n else None            # cv2 returns (kps, None) for an image without keypoints
        status, offset = False, [0, 0]
        try:
            if featA.n and featB.n:
                with self._offsetEstimator():
                    row = eng.features_match_offset(featA.handle, featB.handle, self.searchRatio, self.offsetEvaluate)
                status, offset = bool(row[0]), [int(row[1]), int(row[2])]
                status = self._verified(status, offset, imageA, imageB)      # the sets carry no pixels: the two tiles are checked here
        finally:
            featA.release()                                     # A's set is never needed again (B's lives on in the cache)
            if not featB.n:
                featB.release()
        if status == False:
            tf.isBreak = True
            return (status, CANNOT_MATCH)
        tf.isBreak = False
        self.printAndWrite("  The offset of stitching: dx is " + str(offset[0]) + " dy is " + str(offset[1]))
        return (status, offset)

    def calculateOffsetForFeatureSearchIncre(self, images):
        """Stitcher.py:306-367: for i in 1..maxI-1 { rotate directions until one attempt votes >= offsetEvaluate }."""
        (imageA, imageB) = images
        offset = [0, 0]
        status = False
        iniDirection = self.direction
        localDirection = iniDirection
        for i in range(1, self._maxI()):
            while True:
                res = self._featureAttempt(imageA, imageB, localDirection, i * self.roiRatio)
                if res is not None:
                    (status, offset) = res
                    offset = list(offset)
                if status:
                    break
                else:
                    localDirection = self.directionIncrease(localDirection)
                if localDirection == iniDirection:
                    break
            if status:
                offset = self._axisCorrection(offset, localDirection, i, imageA, imageB)
                self.direction = localDirection
                break
        if status == False:
            return (status, CANNOT_MATCH)
        self.printAndWrite("  The offset of stitching: dx is " + str(offset[0]) + " dy is " + str(offset[1]))
        return (status, offset)

    # ------------------------------------------------------------------------------------------------
    @staticmethod
    def _layout(shapes, originOffsetList):
        """Stitcher.py:387-431: canvas-relative tile origins, running bounding boxes, canvas size.
        originOffsetList already carries the leading [0, 0]."""
        n = len(originOffsetList)
        offsetList = copy.deepcopy(originOffsetList)
        rangeX = [[0, 0] for _ in range(n)]
        rangeY = [[0, 0] for _ in range(n)]
        resultRow, resultCol = shapes[0][0], shapes[0][1]
        rangeX[0][1] = resultRow
        rangeY[0][1] = resultCol
        dxSum = dySum = 0
        for i in range(1, n):
            th, tw = shapes[i][0], shapes[i][1]
            dxSum += offsetList[i][0]
            dySum += offsetList[i][1]
            for (axis, total, ranges, tlen) in ((0, dxSum, rangeX, th), (1, dySum, rangeY, tw)):
                size = resultRow if axis == 0 else resultCol
                if total <= 0:
                    shift = abs(total)
                    for j in range(0, i):
                        offsetList[j][axis] += shift
                        ranges[j][0] += shift
                        ranges[j][1] += shift
                    size += shift
                    ranges[i][1] = size
                    ranges[i][0] = offsetList[i][axis] = 0
                    if axis == 0:
                        dxSum = 0
                    else:
                        dySum = 0
                else:
                    offsetList[i][axis] = total
                    size = max(size, total + tlen)
                    ranges[i][1] = size
                if axis == 0:
                    resultRow = size
                else:
                    resultCol = size
        return offsetList, rangeX, rangeY, resultRow, resultCol

    @staticmethod
    def _placements(shapes, originOffsetList, offsetList, rangeX, rangeY, mode):
        """The canvas walk of Stitcher.py:434-483 as data: int32 [n][9] rows y0, x0, ry0, rx0, ry1, rx1, dx, dy, mode -- the geometry rows
        of Engine.canvas_assemble_resident.  offsetList, rangeX, rangeY: from _layout; mode: a value of Engine.CANVAS_MODES.  The first
        tile, and every tile under notFuse, is a paste row; the ROI of any other is the tile rectangle cut by its predecessor's bounding box."""
        paste = Engine.CANVAS_MODES["notFuse"]
        rows = np.zeros((len(offsetList), 9), np.int32)
        for i in range(len(offsetList)):
            th, tw = shapes[i][0], shapes[i][1]
            oy, ox = offsetList[i][0], offsetList[i][1]
            if i == 0 or mode == paste:
                rows[i] = (oy, ox, 0, 0, 0, 0, 0, 0, paste)
            else:
                rows[i] = (oy, ox, max(oy, rangeX[i - 1][0]), max(ox, rangeY[i - 1][0]), min(oy + th, rangeX[i - 1][1]),
                           min(ox + tw, rangeY[i - 1][1]), originOffsetList[i][0], originOffsetList[i][1], mode)
        return rows

    @staticmethod
    def _placeTile(eng, canvas, tile, resident, row):
        """One row of _placements through the per-tile Engine call for its mode; tile: a handle (resident) or a host array."""
        y0, x0, ry0, rx0, ry1, rx1, dx, dy, mode = (int(v) for v in row)
        if mode == Engine.CANVAS_MODES["notFuse"]:
            (eng.canvas_paste_tile if resident else eng.canvas_paste)(canvas, tile, y0, x0)
        elif mode in Engine.CANVAS_BLEND_MODES:
            (eng.canvas_blend_tile_resident if resident else eng.canvas_blend_tile)(canvas, tile, y0, x0, (ry0, rx0, ry1, rx1),
                                                                                    Engine.CANVAS_BLEND_MODES[mode])
        else:
            (eng.canvas_fuse_tile_resident if resident else eng.canvas_fuse_tile)(canvas, tile, y0, x0, (ry0, rx0, ry1, rx1), dx, dy,
                                                                                  method=Engine.CANVAS_FUSE_METHODS[mode])

    def getStitchByOffset(self, fileList, originOffsetList):
        """Stitcher.py:369-486.  NB: like the reference this inserts [0, 0] at the head of the caller's list."""
        color = self.isColorMode
        originOffsetList.insert(0, [0, 0])
        n = len(originOffsetList)
        eng = self.engine
        # tiles the batched registration left in HBM (the gray planes, or the B G R tiles of the same decode): fused from where they are
        resident = self.__dict__.pop("_resident", None) or {}
        # multiBandBlending runs on the canvas with engines that can set its level count (the CPU test doubles blend through fuseImage)
        multiband = self.fuseMethod == "multiBandBlending" and hasattr(eng, "canvas_set_multiband_levels")
        # optimalSeamLine likewise with engines that can set the canvas's seam blend
        seamline = self.fuseMethod == "optimalSeamLine" and hasattr(eng, "canvas_set_seam_blend")
        device_fuse = self.fuseMethod in ("notFuse", "fadeInAndFadeOut", "trigonometric") or multiband or seamline
        mode = Engine.CANVAS_MODES.get(self.fuseMethod)        # how every tile but the first goes onto the canvas
        simple = mode in Engine.CANVAS_BLEND_MODES and hasattr(eng, "canvas_blend_tile")
        handles = imageList = None
        use_res = (device_fuse or (simple and hasattr(eng, "canvas_blend_tile_resident"))) and \
            all(fileList[i] in resident and (len(resident[fileList[i]][1]) == 3) == color for i in range(n))
        try:
            if not use_res and (device_fuse or simple) and hasattr(eng, "tile_reserve") and hasattr(eng, "tile_fill_pair") and \
                    (not simple or hasattr(eng, "canvas_blend_tile_resident")):
                # not (all) resident -- a custom registration method ran pair by pair on host arrays: the mosaic's tiles go straight from a
                # pool of decoder threads into reserved device tiles, never as a list on the host (the reference holds all of them,
                # Stitcher.py:382-403)
                for h, _shape in resident.values():
                    eng.tile_free(h)
                resident = {}
                resident = self._ingestForMosaic([fileList[i] for i in range(n)], color) or {}
                use_res = bool(resident)
            if use_res:
                shapes = [resident[fileList[i]][1] for i in range(n)]
                handles = [resident[fileList[i]][0] for i in range(n)]
            else:
                imageList = [_imread(fileList[0], color)]
                for i in range(1, n):
                    imageList.append(_imread(fileList[i], Stitcher.isColorMode))
                shapes = [im.shape for im in imageList]
                if device_fuse and hasattr(eng, "tile_upload_color") and len({im.ndim for im in imageList}) == 1:
                    # engines without the ingest entry points: all uploads are queued on the copy stream up front and the per-tile canvas
                    # calls below only enqueue work behind them -- no host synchronisation per tile (Stitcher.py:174-179, 434-483)
                    for h, _shape in resident.values():
                        eng.tile_free(h)
                    resident = {}
                    for i in range(n):
                        im = np.ascontiguousarray(imageList[i])
                        hnd = eng.tile_upload_color(im, asynchronous=True) if im.ndim == 3 else eng.tile_upload_async(im)
                        resident[(i, fileList[i])] = (hnd, im.shape)
                    handles = [resident[(i, fileList[i])][0] for i in range(n)]
                    use_res = True
            if self.shadingCorrection != "none":
                self._correctShading(handles if use_res else None, shapes)
            if self.lensCorrection != "none":                # geometry before exposure: its statistics then see aligned overlaps
                self._correctLens(handles if use_res else None, shapes, originOffsetList)
            if self.exposureCompensation != "none":
                self._compensateExposure(handles if use_res else None, shapes, originOffsetList)
            offsetList, rangeX, rangeY, resultRow, resultCol = self._layout(shapes, originOffsetList)
            self.printAndWrite("  The rectified offsetList is " + str(offsetList))
            if not device_fuse and not simple:
                return self._stitchWithHostFuse(fileList, imageList, originOffsetList, offsetList, rangeX, rangeY, resultRow, resultCol)
            ch = 3 if color else 1
            full_shape = (resultRow, resultCol, ch) if ch > 1 else (resultRow, resultCol)
            pyramid = self._pyramidLevelsOf(full_shape)         # (refuses before anything is fused)
            canvas = eng.canvas_create(resultRow, resultCol, ch)
            try:
                if multiband:
                    eng.canvas_set_multiband_levels(canvas, int(self.multiBandLevels))
                if seamline:
                    eng.canvas_set_seam_blend(canvas, str(self.seamLineBlend))
                    if hasattr(eng, "canvas_set_multiband_levels"):
                        eng.canvas_set_multiband_levels(canvas, int(self.multiBandLevels))
                rows = self._placements(shapes, originOffsetList, offsetList, rangeX, rangeY, mode)
                # every tile resident: the walk as ONE library call (the per-tile calls cost the host more than their two launches cost the device)
                one_call = use_res and hasattr(eng, "canvas_assemble_resident")
                for i in range(n):
                    self.printAndWrite("  stitching " + str(fileList[i]))
                    if not one_call:
                        self._placeTile(eng, canvas, handles[i] if use_res else imageList[i], use_res, rows[i])
                if one_call:
                    eng.canvas_assemble_resident(canvas, handles, rows)
                return self._writeOut(eng, canvas, full_shape, pyramid)
            finally:
                eng.canvas_free(canvas)
        finally:
            if hasattr(eng, "sync_uploads"):
                eng.sync_uploads()                           # the host tiles of asynchronous uploads may be released now
            for h, _shape in resident.values():
                eng.tile_free(h)

    def _writeOut(self, eng, canvas, full_shape, pyramid):
        """the fused canvas out of the device by the route of the installed mosaicSink (_routeOf), band by band -- the mosaic is never whole
        in host memory -- or whole, as the array returned, when there is no sink.  pyramid: _pyramidLevelsOf(full_shape)"""
        rows, cols, ch = full_shape[0], full_shape[1], full_shape[2] if len(full_shape) > 2 else 1
        sink = getattr(self, "mosaicSink", None)
        route = self._routeOf(sink) if sink is not None else None
        if route == "device_jpeg":                               # the sink appends the bands' entropy-coded bytes (csrc/jpeg_enc_kernels.hip)
            for r0, nr, payload in eng.canvas_encode_jpeg_bands(canvas, rows, cols, ch, int(self.jpegQuality), int(self.jpegRestartMcus), self._jpegBandRows()):
                sink(r0, nr, payload, full_shape)
        elif route == "device_png":                              # the sink appends the bands' IDAT chunks (the PNG coder of csrc/deflate_kernels.hip)
            for r0, nr, payload, adler in eng.canvas_encode_png_bands(canvas, rows, cols, ch, int(self.pngSegmentRows), self._pngBandRows()):
                sink(r0, nr, payload, adler, full_shape)
        elif route in ("device_tiles", "device_tiles_deflate"):
            # the finished tile streams of level 0 and of the reduced levels a band completes (a mosaic that fits one tile: zero reduced levels),
            # from the JPEG coder or the lossless one (csrc/deflate_kernels.hip)
            coder_args = (int(self.jpegQuality), int(self.jpegRestartMcus)) if route == "device_tiles" else ()
            for r0, nr, payload, index in getattr(eng, self._ROUTES[route])(canvas, rows, cols, ch, pyramid or 0, int(self.pyramidTile), *coder_args, self._bandRows()):
                sink.tiles(r0, nr, payload, index, full_shape)
        elif sink is not None and hasattr(eng, self._ROUTES["plain"]):
            # pixel bands.  A sink that is done with a band two bands later (`transient_bands`: JpegBandWriter) gets views of the engine's pinned
            # band ring: a DMA at link speed, no page faults of a fresh 300 MB array per band; VFSMS_PINNED_BANDS=0 turns it off
            transient = bool(getattr(sink, "transient_bands", False)) and os.environ.get("VFSMS_PINNED_BANDS", "1") == "1"
            kw = {"transient": True} if transient else {}
            if pyramid:                                          # a pyramidal sink: every band with its reduced levels, formed on the device
                for r0, band, levels in eng.canvas_download_pyramid_bands(canvas, rows, cols, ch, pyramid, self._bandRows(), **kw):
                    sink(r0, band, full_shape, levels=levels)
            else:
                lkw = {"levels": []} if pyramid is not None else {}     # (a mosaic that fits one tile: a pyramid of level 0 alone)
                for r0, band in eng.canvas_download_bands(canvas, rows, cols, ch, self._bandRows(), **kw):
                    sink(r0, band, full_shape, **lkw)
        else:
            return eng.canvas_download(canvas, rows, cols, ch)
        return None

    def _correctShading(self, handles, shapes):
        """Method.shadingCorrection on the mosaic's resident tiles, in place (tests/shading_ref.py): a field estimated over exactly these
        tiles, or Method.shadingGain uploaded, applied and freed.  Registration is over by now, and getStitchByOffset frees these handles
        itself, so nothing else sees the corrected pixels."""
        eng = self.engine
        if self.shadingCorrection != "estimate":
            raise ValueError("shadingCorrection must be 'none' or 'estimate'")
        if not hasattr(eng, "shading_estimate") or handles is None:
            raise NotImplementedError("shadingCorrection needs an engine with shading_estimate and device-resident tiles")
        if len({tuple(s_) for s_ in shapes}) != 1:
            raise ValueError("shadingCorrection needs tiles of one shape, got %s" % sorted({tuple(s_) for s_ in shapes}))
        tiles = list(dict.fromkeys(handles))                   # (a file listed twice is one resident tile: corrected once)
        if self.shadingGain is not None:
            gain = np.asarray(self.shadingGain)
            if gain.dtype != np.uint16 or gain.shape != tuple(shapes[0]):
                raise ValueError("shadingGain must be a uint16 Q12 array of the tile shape %s, got %s %s" % (tuple(shapes[0]), gain.dtype, gain.shape))
            field = eng.shading_from_gain(gain)
        elif len(tiles) < int(self.shadingMinTiles):
            self.printAndWrite("  shading correction skipped: %d tiles, shadingMinTiles is %d" % (len(tiles), int(self.shadingMinTiles)))
            return
        else:
            field = eng.shading_estimate(tiles, int(self.shadingPercentile), int(self.shadingRadius))
        try:
            eng.shading_apply(field, tiles)
        finally:
            eng.shading_free(field)

    def _correctLens(self, handles, shapes, originOffsetList):
        """Method.lensCorrection on the mosaic's resident tiles, in place (lens.correct, tests/lens_ref.py): one radial model per dataset
        from the overlaps under the offsets the mosaic is laid out by (originOffsetList carries the leading [0, 0]), the tiles resampled,
        and the path offsets measured again on the corrected tiles -- the entries of originOffsetList that moved are replaced.  Runs
        behind the shading correction and in front of the exposure compensation.  After "estimate" the fitted pair is left in
        self.lensCoefficients for a later "given" run.  The registration itself is untouched: registering on corrected planes is out of
        scope."""
        eng = self.engine
        if self.lensCorrection not in ("estimate", "given"):
            raise ValueError("lensCorrection must be 'none', 'estimate' or 'given'")
        if not hasattr(eng, "block_ncc_batch") or not hasattr(eng, "lens_apply") or handles is None:
            raise NotImplementedError("lensCorrection needs an engine with block_ncc_batch / lens_apply and device-resident tiles")
        if len({tuple(s_) for s_ in shapes}) != 1:
            raise ValueError("lensCorrection needs tiles of one shape, got %s" % sorted({tuple(s_) for s_ in shapes}))
        from .lens import correct
        offsets, pair, self.lensReport = correct(eng, handles, shapes, originOffsetList[1:], mode=self.lensCorrection,
                                                 coefficients=self.lensCoefficients, centre=self.lensCentre, block=int(self.lensBlock),
                                                 radius=int(self.lensRadius), threshold=float(self.lensThreshold),
                                                 min_blocks=int(self.lensMinBlocks), min_shift=float(self.lensMinShift),
                                                 interpolation=self.lensInterpolation)
        rep = self.lensReport
        if pair is None:
            self.printAndWrite("  lens correction skipped: %s" % rep["reason"])
            return
        if self.lensCorrection == "estimate":
            self.lensCoefficients = pair
        for k, o in enumerate(offsets):
            if list(originOffsetList[k + 1]) != o:
                originOffsetList[k + 1] = o
        self.printAndWrite("  lens correction: a1 %.6f, a2 %.6f, %.3f px at the corner, %s -> %.3f px spread over %d edges, %d offsets moved" %
                           (pair[0], pair[1], rep["corner_px"], "%.3f" % rep["spread_before"] if "spread_before" in rep else "n/a",
                            rep["spread_after"], rep["edges"], rep["moved"]))

    def _compensateExposure(self, handles, shapes, originOffsetList):
        """Method.exposureCompensation on the mosaic's resident tiles, in place (exposure.compensate, tests/exposure_ref.py): one gain per
        tile from the overlaps under the offsets the mosaic is laid out by (originOffsetList carries the leading [0, 0]; a globalAdjust
        result arrives here like any other list).  Runs behind the shading correction, on its output."""
        eng = self.engine
        if self.exposureCompensation != "gain":
            raise ValueError("exposureCompensation must be 'none' or 'gain'")
        if not hasattr(eng, "overlap_stats_batch") or not hasattr(eng, "exposure_apply") or handles is None:
            raise NotImplementedError("exposureCompensation needs an engine with overlap_stats_batch / exposure_apply and device-resident tiles")
        from .exposure import compensate
        _gains, self.exposureReport = compensate(eng, handles, shapes, originOffsetList[1:], band=tuple(self.exposureBand),
                                                 min_pixels=int(self.exposureMinPixels), max_gain=float(self.exposureMaxGain))
        self.printAndWrite("  exposure compensation: %d edges, gains %.4f .. %.4f" %
                           (self.exposureReport["edges"], self.exposureReport["gain_min"], self.exposureReport["gain_max"]))

    def _ingestForMosaic(self, files, color):
        """The mosaic's tiles from their files into reserved device tiles through a pool of decoder threads (one decode per file, the
        colour conversion on the GPU) -> {file: (handle, shape)}."""
        eng = self.engine
        if len(set(files)) != len(files):                    # (a file listed twice: the host path keys nothing by name)
            return None
        device_dct = self._jpegDecoderOnDevice()
        shapes = [_imshape(f) for f in files]
        handles = []
        try:
            for s_ in shapes:
                handles.append(eng.tile_reserve_color(s_[0], s_[1], 3) if color else eng.tile_reserve(s_[0], s_[1]))

            def ingest(k):
                try:
                    if _fill_from_jpeg(eng, files[k], 0 if color else handles[k], handles[k] if color else 0, *((device_dct,) if device_dct else ())):
                        return
                    owner, shape, parts = _decode_once(files[k], color)
                    if tuple(shape) != tuple(shapes[k]):
                        raise ValueError("decoded size %s of %s differs from its header %s" % (shape, files[k], shapes[k]))
                    if parts[0] == "src":
                        eng.tile_fill_pair(0 if color else handles[k], handles[k] if color else 0, parts[1], parts[2], parts[3])
                    else:
                        eng.tile_fill(handles[k], parts[2] if color else parts[1])
                    del owner
                except BaseException:
                    try:
                        eng.tile_fill(handles[k], None)
                    except Exception:
                        pass
                    raise
            nthreads = self._decoderThreads(len(files))
            with _PillowBlocks(color):
                futs = [_decoder_pool(nthreads).submit(ingest, k) for k in range(len(files))]
                first = None
                for fu in futs:                               # every decoder has finished with its handle before anything is given up
                    try:
                        fu.result()
                    except BaseException as e:                 # noqa: PERF203
                        first = first or e
                if first is not None:
                    raise first
        except BaseException:
            for h in handles:
                try:
                    eng.tile_fill(h, None)
                except Exception:
                    pass
                try:
                    eng.tile_free(h)
                except Exception:
                    pass
            raise
        return dict(zip(files, zip(handles, [(s_[0], s_[1], 3) if color else s_ for s_ in shapes])))

    def _stitchWithHostFuse(self, fileList, imageList, originOffsetList, offsetList, rangeX, rangeY, resultRow, resultCol):
        """Fallback for engines without the canvas blend entry points (the CPU test doubles): same int64 / -1 canvas walk as
        Stitcher.py:434-486, blend through self.fuseImage."""
        color = self.isColorMode
        shape = (resultRow, resultCol, 3) if color else (resultRow, resultCol)
        stitchResult = np.zeros(shape, np.int64) - 1
        for i in range(0, len(offsetList)):
            self.printAndWrite("  stitching " + str(fileList[i]))
            tile = imageList[i]
            oy, ox = offsetList[i][0], offsetList[i][1]
            if i == 0:
                stitchResult[oy:oy + tile.shape[0], ox:ox + tile.shape[1]] = tile
                continue
            roi_ltx = max(oy, rangeX[i - 1][0]); roi_lty = max(ox, rangeY[i - 1][0])
            roi_rbx = min(oy + tile.shape[0], rangeX[i - 1][1]); roi_rby = min(ox + tile.shape[1], rangeY[i - 1][1])
            roiImageRegionA = stitchResult[roi_ltx:roi_rbx, roi_lty:roi_rby].copy()
            stitchResult[oy:oy + tile.shape[0], ox:ox + tile.shape[1]] = tile
            roiImageRegionB = stitchResult[roi_ltx:roi_rbx, roi_lty:roi_rby].copy()
            stitchResult[roi_ltx:roi_rbx, roi_lty:roi_rby] = self.fuseImage([roiImageRegionA, roiImageRegionB],
                                                                            originOffsetList[i][0], originOffsetList[i][1])
        stitchResult[stitchResult == -1] = 0
        return stitchResult.astype(np.uint8)

    def fuseImage(self, images, dx, dy):
        """Stitcher.py:488-525: dispatch on fuseMethod (int64 regions with -1 = empty)."""
        self.imageFusion.isColorMode = self.isColorMode
        self.imageFusion.multiBandLevels = self.multiBandLevels
        self.imageFusion.seamLineBlend = self.seamLineBlend
        self.imageFusion._engine = self._engine
        (imageA, imageB) = images
        if self.fuseMethod not in ("fadeInAndFadeOut", "trigonometric", "multiBandBlending", "optimalSeamLine"):
            imageA[imageA == -1] = 0
            imageB[imageB == -1] = 0
            imageA[imageA == 0] = imageB[imageA == 0]
            imageB[imageB == 0] = imageA[imageB == 0]
        if self.fuseMethod == "notFuse":
            return imageB
        if self.fuseMethod == "average":
            return self.imageFusion.fuseByAverage([imageA, imageB])
        if self.fuseMethod == "maximum":
            return self.imageFusion.fuseByMaximum([imageA, imageB])
        if self.fuseMethod == "minimum":
            return self.imageFusion.fuseByMinimum([imageA, imageB])
        if self.fuseMethod == "fadeInAndFadeOut":
            return self.imageFusion.fuseByFadeInAndFadeOut(images, dx, dy)
        if self.fuseMethod == "trigonometric":
            return self.imageFusion.fuseByTrigonometric(images, dx, dy)
        if self.fuseMethod == "multiBandBlending":
            # the raw -1 regions, not zero-filled: the seam comes from A's -1 pattern as in the fade
            return self.imageFusion.fuseByMultiBandBlending(images, dx, dy)
        if self.fuseMethod == "optimalSeamLine":
            # the raw -1 regions: geometry and the seam's free passage through holes come from the -1 patterns (an engine without
            # fuse_seam_i64 cannot run the method: fuseByOptimalSeamLine raises NotImplementedError before anything is touched)
            return self.imageFusion.fuseByOptimalSeamLine(images, dx, dy)
        return np.zeros(imageA.shape, np.uint8)
