"""Operator layer of the VFSMS hot path -- host-side mirror of the reference's `ImageUtility.Method`.

Same class / attribute / method names, argument meaning and return conventions as
/root/reference/ImageUtility.py (cited per method), so `Stitcher` code written against the reference runs
unchanged; every operator dispatches into libvfsms.so (hand-written HIP for MI355X) through
imagestitch_amd._lib.Engine.  There is no cv2 and no CPU fallback behind these methods.
"""
import contextlib
import math

import numpy as np

from . import _lib


def roi_rect(shape, direction=1, order="first", searchRatio=0.1):
    """(y0, x0, h, w) of the strip Method.getROIRegionForIncreMethod slices (ImageUtility.py:66-101).

    direction 1: A bottom / B top; 2: A right / B left; 3: A top / B bottom; 4: A left / B right, where
    order "first" is image A and "second" image B.  The length is floor(len * searchRatio) evaluated in
    float64 exactly like np.floor(row * searchRatio).astype(int) (3*0.2 = 0.6000000000000001 matters).
    """
    row, col = int(shape[0]), int(shape[1])
    if direction in (1, 3):
        n = int(math.floor(row * searchRatio))
        at_end = (direction == 1) == (order == "first")
        if order not in ("first", "second"):
            return (0, 0, row, col)
        return (row - n, 0, n, col) if at_end else (0, 0, n, col)
    if direction in (2, 4):
        n = int(math.floor(col * searchRatio))
        at_end = (direction == 2) == (order == "first")
        if order not in ("first", "second"):
            return (0, 0, row, col)
        return (0, col - n, row, n) if at_end else (0, 0, row, n)
    return (0, 0, row, col)


@contextlib.contextmanager
def offset_estimator(engine, offsetCaculate="mode", ransacThreshold=3):
    """The engine's fused paths vote by consensus (getOffsetByRansac) inside the block when offsetCaculate is "ransac", and by mode again
    after it, also when it raises.  "mode" makes no engine call: mode is the engine's default."""
    if offsetCaculate != "ransac":
        yield
        return
    engine.set_offset_estimator("ransac", ransacThreshold)
    try:
        yield
    finally:
        engine.set_offset_estimator("mode")


@contextlib.contextmanager
def offset_verifier(engine, offsetVerify="none", verifyThreshold=0.0, verifyMinPixels=0):
    """The engine's fused paths check every voted offset by overlap correlation (Method.offsetVerify = "ncc") inside the block, and not at
    all after it, also when it raises.  "none" makes no engine call: no check is the engine's default."""
    if offsetVerify == "none":
        yield
        return
    engine.set_offset_verifier(offsetVerify, verifyThreshold, verifyMinPixels)
    try:
        yield
    finally:
        engine.set_offset_verifier("none")


@contextlib.contextmanager
def phase_resolver(engine, phaseResolve="none", phasePeaks=2, phaseResolveThreshold=0.5, phaseResolveMinPixels=4096):
    """The engine's phase chains (pairs_offsets with method "phase") resolve every correlation surface by overlap correlation
    (Stitcher.phaseResolve = "ncc") inside the block, and read it the reference's way again after it, also when it raises.  "none" makes
    no engine call: that is the engine's default.  An engine without the resolver raises NotImplementedError."""
    if phaseResolve == "none":
        yield
        return
    if phaseResolve != "ncc":
        raise ValueError("phaseResolve must be 'none' or 'ncc'")
    if not hasattr(engine, "set_phase_resolver"):
        raise NotImplementedError("this engine has no phase resolver (phaseResolve = %r)" % (phaseResolve,))
    engine.set_phase_resolver(phaseResolve, phasePeaks, phaseResolveThreshold, phaseResolveMinPixels)
    try:
        yield
    finally:
        engine.set_phase_resolver("none")


@contextlib.contextmanager
def vote_tail(engine, offsetCaculate="mode", ransacThreshold=3, offsetVerify="none", verifyThreshold=0.0, verifyMinPixels=0):
    """offset_estimator and offset_verifier around one fused engine call"""
    with offset_estimator(engine, offsetCaculate, ransacThreshold), offset_verifier(engine, offsetVerify, verifyThreshold, verifyMinPixels):
        yield


class Method():
    # ---- logging (ImageUtility.py:8-12) ----
    outputAddress = "result/"
    isEvaluate = False
    evaluateFile = "evaluate.txt"
    isPrintLog = True

    # ---- feature search (ImageUtility.py:14-17) ----
    featureMethod = "surf"      # "sift", "surf" or "orb"
    roiRatio = 0.1
    searchRatio = 0.75

    # ---- backend switch (ImageUtility.py:19-20).  Both values run on the MI355X here; the flag keeps the
    # reference's meaning of WHICH parameter set is used: False -> cv2 defaults (SURF 100/4/3, 64-d;
    # ORB without distance threshold), True -> the surf*/orb* attributes below (128-d SURF, orbMaxDistance).
    isGPUAvailable = False

    # ---- SURF parameters of the DLL path (ImageUtility.py:22-28) ----
    surfHessianThreshold = 100.0
    surfNOctaves = 4
    surfNOctaveLayers = 3
    surfIsExtended = True
    surfKeypointsRatio = 0.01
    surfIsUpright = False

    # ---- ORB parameters (ImageUtility.py:30-40) ----
    orbNfeatures = 5000
    orbScaleFactor = 1.2
    orbNlevels = 8
    orbEdgeThreshold = 31
    orbFirstLevel = 0
    orbWTA_K = 2
    orbPatchSize = 31
    orbFastThreshold = 20
    orbBlurForDescriptor = False
    orbMaxDistance = 30

    # ---- SIFT parameters: cv2.xfeatures2d.SIFT_create() defaults (ImageUtility.py:256,268; the reference passes none) ----
    siftNOctaveLayers = 3
    siftContrastThreshold = 0.04
    siftEdgeThreshold = 10
    siftSigma = 1.6

    # ---- registration (ImageUtility.py:42-44) ----
    offsetCaculate = "mode"     # "mode" or "ransac"
    offsetEvaluate = 3
    ransacThreshold = 3         # "ransac": Chebyshev tolerance in px (0..64) around a vote (getOffsetByRansac)

    # ---- acceptance check behind the vote (no reference counterpart; tests/verify_ref.py): "ncc" keeps a voted offset only when the
    # normalised cross-correlation of the RAW pixels the two strips share under it reaches verifyThreshold.  The threshold is measured
    # (tests/test_verify_host.py): on the committed real strips every true accept scores 0.844 .. 0.995 and every
    # false accept -0.105 .. 0.026; 0.5 lies between, far from both.  verifyMinPixels is a condition, not a measurement: fewer shared
    # pixels than a 64 x 64 patch cannot be judged and are rejected (the thinnest true overlap there, 39 rows of a 640-px crop, has 24921)
    offsetVerify = "none"       # "none" or "ncc"
    verifyThreshold = 0.5
    verifyMinPixels = 4096

    # ---- global placement (no reference counterpart; adjust.py, tests/ncc_search_ref.py): "ncc" also measures the offsets of side
    # neighbours ACROSS the shooting path -- the same statistic as offsetVerify, searched over a window of +-adjustRadius px around the
    # offset the path predicts -- and places all tiles of a segment by one least-squares fit before the mosaic is laid out.  An edge counts
    # when its best score reaches adjustThreshold and the peak lies inside the window.  The threshold is the verifier's (DESIGN.md section
    # 3): tests/golden holds STRIPS of the real tiles only, no whole tiles, so the ranges measured there stand -- true 0.844 .. 0.995,
    # false -0.105 .. 0.026 -- and whole tiles were measured on the three synthetic grids of tests/adjust_cases.py (36 edges): at the true
    # offset 0.9968 .. 0.9981; the BEST score of a 9 x 9 window that does not hold it (143 windows centred 29 .. 40 px off, >= 4096 shared
    # pixels) -0.108 .. 0.276 -- a maximum over 81 candidates, hence higher than a single false vote, and still far below 0.5.
    globalAdjust = "none"       # "none" or "ncc"
    adjustRadius = 4            # 1..16
    adjustThreshold = 0.5
    adjustMinPixels = 4096

    # ---- repair of pairs that cannot be registered (no reference counterpart; stage.py, tests/stage_ref.py, tests/ncc_wide_ref.py): "stage"
    # keeps ONE mosaic where a featureless tile would cut it -- the typical offset per scan direction comes from the pairs that did
    # register, a failed pair is searched by correlation within +-repairRadius px of it (two levels: tiles reduced repairFactor x
    # repairFactor, then full resolution around the repairPeaks best coarse candidates), and a pair whose overlap carries no signal takes
    # the model's offset as it is.  repairThreshold is the verifier's threshold (true accepts 0.844 and above, false accepts 0.026 and
    # below on the committed real strips).  repairBlankRatio is a design choice, not a measurement: the repository holds no real blank
    # tile; an overlap is blank when the standard deviation of one side is below that fraction of the accepted pairs' median.
    failedPairRepair = "none"   # "none" or "stage"
    repairRadius = 32           # 1..128
    repairFactor = 4            # 2, 4 or 8; ceil(repairRadius / repairFactor) <= 16
    repairPeaks = 2             # 1..4
    repairThreshold = 0.5
    repairMinPixels = 4096
    repairBlankRatio = 0.25

    # ---- enhancement (ImageUtility.py:46-50; CLAHE/equalizeHist are out of the hot-path scope) ----
    isEnhance = False
    isClahe = False
    clipLimit = 20
    tileSize = 5

    # ---- fusion (fuseMethod "multiBandBlending": pyramid levels, ImageFusion.fuseByMultiBandBlending / the device canvas) ----
    multiBandLevels = 4
    # fuseMethod "optimalSeamLine": how the two sides of the seam are merged -- "none" (every pixel from one tile) or "multiBandBlending"
    # (the seam's label plane as the mask of the pyramid blend with multiBandLevels levels)
    seamLineBlend = "none"

    # ---- flat-field shading correction before the mosaic is built (no reference counterpart; tests/shading_ref.py): "estimate" takes the
    # shadingPercentile order statistic of every sample over the mosaic's own tiles, smooths it with two box passes of shadingRadius and
    # divides the tiles by it (registration never sees corrected pixels).  shadingRadius = 32 and the two passes rest on nothing measured
    # at production size: they come from a 256 x 256 synthetic stack (tests/test_shading_host.py).  shadingMinTiles is a condition, not a
    # measurement: a median over a handful of tiles is their content, not the optics, so fewer tiles are left uncorrected.  shadingGain: a
    # uint16 Q12 array of the tile shape measured elsewhere (a blank-slide image), used instead of the estimate whatever the tile count
    shadingCorrection = "none"  # "none" or "estimate"
    shadingPercentile = 50
    shadingRadius = 32
    shadingMinTiles = 8
    shadingGain = None

    # ---- focus stacking in front of the pipeline (no reference counterpart; focus.py, tests/focus_ref.py): Stitcher.imageSetFocusStack
    # fuses the focusPlanes consecutive files of every stage position into one all-in-focus tile, which imageSetStitch* then reads like
    # any other.  "pixel": per pixel the plane whose sum-modified Laplacian, summed over (2 focusRadius + 1)^2, is largest, the index
    # map cleaned by focusMedian passes (0 or 1) of a 3 x 3 median; "plane": the whole plane of the largest score.  focusDepthMaps also
    # writes the index map of every position.  focusRadius = 4 and the one median pass rest on nothing measured on real material: they
    # come from the synthetic stacks of tests/focus_cases.py only (tests/test_focus_host.py), the repository holds no real focus series.
    # The defaults change nothing: no entry point of the pipeline reads these attributes.
    focusStack = "none"         # "none", "pixel" or "plane"
    focusPlanes = 1             # files per stage position, 2..64 when focusStack is not "none"
    focusRadius = 4             # 1..31
    focusMedian = 1             # 0 or 1
    focusDepthMaps = False

    # ---- per-tile exposure compensation after the shading correction, before the mosaic is laid out (no reference counterpart;
    # exposure.py, tests/exposure_ref.py): "gain" sums, over every overlap of two tiles of the mosaic, the samples that are unclipped in
    # both, fits one gain per tile by weighted least squares in the log domain and multiplies the resident tiles by it (registration
    # never sees corrected pixels).  The fit has no constants; the attributes below are conditions, none of them tuned:
    exposureCompensation = "none"   # "none" or "gain"
    # the samples that count, lo <= p <= hi in both tiles: everything but the two clipped codes of an 8-bit sensor -- a sample at 0 or
    # 255 has lost its value, so its ratio to the other tile says nothing about exposure
    exposureBand = (1, 254)
    # an overlap with fewer shared pixels is no edge, and an edge with fewer unclipped samples is not measured: the value of
    # adjustMinPixels, for the same reason (smaller than a 64 x 64 patch cannot be judged)
    exposureMinPixels = 4096
    # a condition, not a measurement: exposure drift within a scan is a matter of per cent; a gain beyond 2 means the overlap statistic
    # is not an exposure ratio (a wrong offset, different content), and the tile is held at the bound
    exposureMaxGain = 2.0

    # ---- radial lens correction between the shading correction and the exposure compensation (no reference counterpart; lens.py,
    # tests/lens_ref.py): "estimate" measures the displacement of every lensBlock x lensBlock square of every overlap within
    # +-lensRadius px of the registered offset, fits ONE radial model u(s) = s (1 + b1 rho^2) per dataset from how the displacement bows
    # along the shared sides, resamples the resident tiles in place (lensInterpolation "cubic" or "bilinear") and measures the path
    # offsets again; "given" skips the fit and takes lensCoefficients = (a1, a2) of s(u) = u (1 + a1 rho^2 + a2 rho^4), which an
    # "estimate" run leaves behind for the next dataset of the session.  lensCentre: (cy, cx) in pixels, None for the tile's middle.
    # Registration never sees corrected pixels.  lensThreshold = 0.5 is the verifier's threshold re-used: PROVISIONAL, nobody has tuned
    # it for blocks (tools/bench_lens.py records the block-score distribution of the committed real strips).  lensMinBlocks and
    # lensMinShift are design choices, not measurements: a fit from fewer measured blocks is not trusted, and a corner shift below a
    # quarter pixel is left alone because resampling would only blur.
    lensCorrection = "none"     # "none", "estimate" or "given"
    lensCoefficients = None
    lensCentre = None
    lensBlock = 64              # 8..128 in multiples of 8
    lensRadius = 8              # 1..16
    lensThreshold = 0.5
    lensMinBlocks = 32
    lensMinShift = 0.25
    lensInterpolation = "cubic"

    # ---- pyramidal output (no reference counterpart; tests/pyramid_ref.py): imageSetStitch* write every mosaic as ONE tiled pyramidal
    # TIFF (PyramidTiffBandWriter: level 0 in pyramidTile x pyramidTile tiles, then reduced-resolution pages, each half the size of the one
    # before) that slide and micrograph viewers open without reading all of it.  The levels are formed on the device from the band that
    # is leaving it anyway.  pyramidLevels None: as many as it takes for the last level to fit one tile (at most 10); pyramidCompression
    # "none", "deflate", or "jpeg": TIFF compression 7 with shared tables in JPEGTables, what slide viewers expect and a tenth of the
    # bytes (tests/tiff_jpeg_ref.py).  With "jpeg" the tiles of every level are encoded on the device (csrc/jpeg_enc_kernels.hip in tile
    # order) at jpegQuality with jpegRestartMcus MCUs per restart interval (0: one interval per tile; the MCUs of a tile -- (pyramidTile /
    # 16)^2 in colour, (pyramidTile / 8)^2 in gray -- must be whole intervals); edge tiles repeat the level's last row and column instead
    # of padding with zeros; mosaicBandRows must also be a multiple of pyramidTile; there is no host encoder behind it, so a mosaicSink of
    # the user's is refused.  "deflate-device": the lossless counterpart -- TIFF compression 8 with Predictor 2, every tile a zlib stream
    # coded on the device (csrc/deflate_kernels.hip, tests/deflate_ref.py: horizontal differencing, then deflate restricted to runs at
    # distance 1 and one dynamic Huffman block a tile), so nothing crosses the link as pixels; the decoded pages equal those of "none" and
    # "deflate", zero padding included; the same conditions as "jpeg" (mosaicBandRows a multiple of pyramidTile, no mosaicSink of the
    # user's); jpegQuality and jpegRestartMcus play no part.  Needs a .tif / .tiff output, streamOutput, and mosaicBandRows a multiple of 2^levels
    outputPyramid = False
    pyramidTile = 512
    pyramidLevels = None
    pyramidCompression = "none"

    # ---- JPEG results encoded on the device (no reference counterpart; tests/jpeg_enc_ref.py).  jpegEncoder "host" (the default: nothing
    # changes -- the bands cross the link as pixels and libjpeg-turbo encodes them on a host thread pool, JpegBandWriter) or "device": with
    # streamOutput, a .jpg / .jpeg result and no mosaicSink of the user's, colour conversion, DCT, quantisation and Huffman coding run where
    # the mosaic is (csrc/jpeg_enc_kernels.hip) and a band leaves as its entropy-coded bytes, which the host only appends to the file
    # (DeviceJpegFile).  The file decodes to the pixels of the host encoder's file; its bytes are tests/jpeg_enc_ref.py's.
    # jpegQuality: cv2.imwrite's default, the one the host path uses (Stitcher.py:149 passes no flags).
    # jpegRestartMcus: MCUs (16 x 16 pixels, 8 x 8 gray) per restart interval = per device lane.  Shorter intervals mean more lanes and two
    # marker bytes plus up to seven padding bits each; 8 keeps that below half a per cent of a quality-95 mosaic.  PROVISIONAL: the sweep
    # of tools/bench_jpeg_device.py over {1 .. 64} has not been run on the device yet (README).  mosaicBandRows must
    # be a multiple of the MCU height times jpegRestartMcus, so that every band is whole intervals whatever the mosaic's width.
    jpegEncoder = "host"
    jpegQuality = 95
    jpegRestartMcus = 8

    # ---- PNG results coded on the device (no reference counterpart; tests/png_ref.py).  pngEncoder "host" (the default: nothing changes --
    # the bands cross the link as pixels and ONE zlib stream at level 1 with filter 0 on every row codes them on one host thread,
    # PngBandWriter) or "device": with streamOutput, a .png result, no outputPyramid and no mosaicSink of the user's, every row gets the PNG
    # filter (None, Sub, Up, Average, Paeth) of the smallest sum of absolutes where the mosaic is, segments of pngSegmentRows rows are coded by
    # the lossless tile coder (runs at distance 1, one dynamic Huffman block a segment) and leave as finished IDAT chunks, CRC-32 included,
    # which the host only appends to the file (DevicePngFile, which folds the bands' Adler-32 together).  The file decodes to the pixels of
    # the host writer's file; its bytes are tests/png_ref.py's.
    # pngSegmentRows: rows per segment = per Huffman table and per IDAT chunk (1..4096).  Shorter segments mean more parallel strings and
    # about 170 bytes of table and frame each.  16: in the sweep of tools/bench_png_device.py over {1 .. 256} the file no longer shrinks beyond
    # it and the time grows (README).
    # mosaicBandRows must be a multiple of pngSegmentRows, so that every band is whole segments.
    pngEncoder = "host"
    pngSegmentRows = 16

    # ---- JPEG tiles decoded on the device (no reference counterpart; tests/jpeg_dec_ref.py).  jpegDecoder "host" (the default: nothing
    # changes -- libjpeg-turbo decodes a file up to its sample planes on a decoder thread, vfsms_tile_fill_jpeg) or "device": the decoder
    # thread stops behind the entropy decode (jpeg_read_coefficients) and dequantisation, the inverse DCT, the level shift and the clamp run
    # where the tile is going (csrc/jpeg_dec_kernels.hip), followed by the chroma upsampling and colour conversion that run there already.
    # The tiles hold the same bytes either way.  Taken: 8-bit gray and 4:2:0 Y Cb Cr files, baseline or progressive; any other file goes
    # the "host" way, then Pillow's, decoded once.  Twice the bytes cross the link (2 per sample instead of 1), and the host's share is not
    # gone: the library buffers the whole image's coefficients before they are copied -- README says what tools/bench_jpeg_decode.py measured.
    # "device-entropy": the entropy decode runs on the device too (csrc/jpeg_huff_kernels.hip; tests/jpeg_huff_ref.py).  The decoder thread
    # reads the file and scans it once for its markers -- no libjpeg --, the compressed bytes alone cross the link (about 0.5 B per pixel at
    # quality 90), and Huffman decode, DC prediction and everything "device" does run in device memory.  Taken: 8-bit baseline files with one
    # scan, gray or 4:2:0, with or without restart markers; any other file (progressive, several scans, damaged, or one whose bits are so
    # dense that the parallel decoders do not fall in step within VFSMS_JPEG_HUFF_MAX_ROUNDS rounds) goes the "device" way, then "host",
    # then Pillow's, decoded once.
    jpegDecoder = "host"

    # engine injection point (tests substitute fakes; production resolves the per-process GPU engine)
    _engine = None

    @property
    def engine(self):
        eng = self._engine
        if eng is None:
            eng = _lib.default_engine()
        return eng

    # ------------------------------------------------------------------------------------------------
    def printAndWrite(self, content):
        """ImageUtility.py:52-64: print if isPrintLog; append to outputAddress+evaluateFile if isEvaluate."""
        if self.isPrintLog:
            print(content)
        if self.isEvaluate:
            with open(self.outputAddress + self.evaluateFile, "a") as f:
                f.write(content)
                f.write("\n")

    def getROIRegionForIncreMethod(self, image, direction=1, order="first", searchRatio=0.1):
        """ImageUtility.py:66-101: the search strip as a numpy VIEW of `image` (no copy)."""
        if direction not in (1, 2, 3, 4) or order not in ("first", "second"):
            return np.zeros(image.shape, np.uint8)          # the reference's untouched initial value
        y0, x0, h, w = roi_rect(image.shape, direction, order, searchRatio)
        return image[y0:y0 + h, x0:x0 + w]

    def getOffsetByMode(self, kpsA, kpsB, matches, offsetEvaluate=10):
        """ImageUtility.py:139-178 -> (status, [dx, dy]).  matches: [(trainIdx, queryIdx)].
        dx/dy = int() of float32 differences (truncation), (0,0) votes dropped, mode with first-seen
        tie-break, status = count >= offsetEvaluate; empty matches -> (False, [0, 0])."""
        if len(matches) == 0:
            return (False, [0, 0])
        status, off, _votes = self.engine.mode_offset(np.asarray(kpsA, np.float32), np.asarray(kpsB, np.float32),
                                                      np.asarray(matches, np.int32), offsetEvaluate)
        return (status, off)

    def getOffsetByRansac(self, kpsA, kpsB, matches, offsetEvaluate=100):
        """offsetCaculate = "ransac" -> (status, [dx, dy], adjustH) like ImageUtility.py:180-210's tuple (adjustH = np.eye(3) when status
        is true, else 0).  The reference's version fits a homography and then breaks, so the specification is the project's own,
        tests/consensus_ref.py: a deterministic consensus over one-point translation hypotheses.  The votes are getOffsetByMode's; a vote's
        support counts the votes within `ransacThreshold` px of it on both axes; the first vote of largest support wins, and the offset is the
        lower median of its inliers per axis; status = support >= offsetEvaluate.  At ransacThreshold = 0 it equals getOffsetByMode."""
        if len(matches) == 0:
            return (False, [0, 0], 0)
        status, off, _support = self.engine.consensus_offset(np.asarray(kpsA, np.float32), np.asarray(kpsB, np.float32),
                                                             np.asarray(matches, np.int32), self.ransacThreshold, offsetEvaluate)
        return (status, off, np.eye(3) if status else 0)

    def verifyOffset(self, roiA, roiB, offset):
        """offsetVerify = "ncc" -> (ok, score): the normalised cross-correlation of the pixels roiA and roiB (uint8, one shape, the raw
        pixels) share under the RAW vote `offset` = [dx, dy] of getOffsetByMode / getOffsetByRansac on them -- roiB's pixel (r, c) meets
        roiA's pixel (r + dx, c + dy) -- and ok = score >= verifyThreshold.  Fewer than verifyMinPixels shared pixels or a flat side
        score 0.  Specified by tests/verify_ref.py."""
        _sums, score, _fixed = self.engine.verify_ncc(np.asarray(roiA), np.asarray(roiB), int(offset[0]), int(offset[1]), self.verifyMinPixels)
        return (bool(score >= self.verifyThreshold), score)

    # -- array adapters of the DLL path (ImageUtility.py:212-246): kept for API compatibility ------------
    def npToListForKeypoints(self, array):
        return [[array[i, 0], array[i, 1]] for i in range(array.shape[0])]

    def npToListForMatches(self, array):
        return [(array[i, 0], array[i, 1]) for i in range(array.shape[0])]

    def npToKpsAndDescriptors(self, array):
        """float32[N, D, 2] packing of appendix/myGpuFeatures.cpp:16-51: [i,0,0]=x, [i,1,0]=y, [i,:,1]=descriptor."""
        return ([[array[i, 0, 0], array[i, 1, 0]] for i in range(array.shape[0])], array[:, :, 1])

    # ------------------------------------------------------------------------------------------------
    def _surfParams(self):
        if self.isGPUAvailable:
            return self.engine.surf_params(self.surfHessianThreshold, self.surfNOctaves, self.surfNOctaveLayers,
                                           self.surfIsExtended, self.surfIsUpright)
        return self.engine.surf_params()      # cv2.xfeatures2d.SURF_create() defaults (ImageUtility.py:258)

    def _orbParams(self):
        """cv2.ORB_create(orbNfeatures, orbScaleFactor, orbNlevels, orbEdgeThreshold, orbFirstLevel, orbWTA_K, 0, orbPatchSize,
        orbFastThreshold) -- ImageUtility.py:260 (both backends of the reference pass the same Method.orb* attributes)."""
        return self.engine.orb_params(self.orbNfeatures, self.orbScaleFactor, self.orbNlevels, self.orbEdgeThreshold,
                                      self.orbFirstLevel, self.orbWTA_K, 0, self.orbPatchSize, self.orbFastThreshold)

    def _siftParams(self):
        """cv2.xfeatures2d.SIFT_create() -- ImageUtility.py:256,268 (both backends of the reference create SIFT without arguments)"""
        return self.engine.sift_params(self.siftNOctaveLayers, self.siftContrastThreshold, self.siftEdgeThreshold, self.siftSigma)

    def detectAndDescribe(self, image, featureMethod):
        """ImageUtility.py:248-276 -> (kps float32[N,2] of (x, y), features float32[N,D] or None).

        "sift" runs csrc/sift_kernels.hip: OpenCV 3.3.1's SIFT_Impl arithmetic with SIFT_create() defaults, in the evaluation order that
        tests/sift_ref.py specifies (the device output equals that numpy restatement bit for bit).  No byte parity with cv2 is claimed:
        OpenCV's own float blur depends on whether its IPP / SIMD paths are compiled in."""
        if featureMethod == "surf":
            kps, feats = self.engine.surf_detect_describe(np.asarray(image), self._surfParams())
            if len(kps) == 0:
                return (np.float32([]), None)      # cv2 returns ([], None) for an image without keypoints
            return (kps, feats)
        if featureMethod == "orb":
            kps, feats = self.engine.orb_detect_describe(np.asarray(image), self._orbParams())
            if len(kps) == 0:
                return (np.float32([]), None)
            return (kps, feats)
        if featureMethod == "sift":
            kps, feats = self.engine.sift_detect_describe(np.asarray(image), self._siftParams())
            if len(kps) == 0:
                return (np.float32([]), None)
            return (kps, feats)
        raise NotImplementedError("featureMethod %r is outside the VFSMS hot path" % (featureMethod,))

    def matchDescriptors(self, featuresA, featuresB):
        """ImageUtility.py:278-309 -> [(trainIdx, queryIdx)] in query order."""
        if self.featureMethod in ("surf", "sift"):
            pairs = self.engine.bf_l2_ratio_matches(featuresA, featuresB, self.searchRatio)
        elif self.featureMethod == "orb":
            max_dist = self.orbMaxDistance if self.isGPUAvailable else -1
            pairs = self.engine.bf_hamming_matches(featuresA, featuresB, max_dist)
        else:
            raise NotImplementedError("featureMethod %r" % (self.featureMethod,))
        return [(int(t), int(q)) for t, q in pairs]
