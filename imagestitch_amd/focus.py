"""Focus stacking in front of the pipeline (Method.focusStack; no reference counterpart, tests/focus_ref.py is the specification).

A sample that is never flat is shot as a short focus series at every stage position; this module fuses each series into ONE all-in-focus
tile before anything is registered.  The arithmetic runs in csrc/focus_kernels.hip behind Engine.focus_stack; here are the array-level
operator (fuse_stack) and the dataset-level walk (fuse_dataset) that Stitcher.imageSetFocusStack drives.
"""
import os

import numpy as np

from .ingest import _imread, _imshape, _decoder_pool, _PillowBlocks
from .io import _imwrite

MODES = ("pixel", "plane")
MIN_PLANES, MAX_PLANES, MAX_RADIUS = 2, 64, 31
DEPTH_DIR = "depth"            # the index maps' folder below the fused tiles
GROUPS_RESIDENT = 2            # stage positions in flight at a time: one on the device being fused, one being decoded behind it


def check_options(mode, planes, radius, median):
    """Method.focusStack / focusPlanes / focusRadius / focusMedian, judged before a file is listed or a tile decoded"""
    if mode not in MODES:
        raise ValueError("focusStack must be 'pixel' or 'plane' here, got %r" % (mode,))
    if not MIN_PLANES <= int(planes) <= MAX_PLANES:
        raise ValueError("focusPlanes must lie in %d..%d, got %r" % (MIN_PLANES, MAX_PLANES, planes))
    if not 1 <= int(radius) <= MAX_RADIUS:
        raise ValueError("focusRadius must lie in 1..%d, got %r" % (MAX_RADIUS, radius))
    if median not in (0, 1):
        raise ValueError("focusMedian must be 0 or 1, got %r" % (median,))


def _upload(engine, image):
    image = np.asarray(image)
    return engine.tile_upload_color(image) if image.ndim == 3 else engine.tile_upload(image)


def fuse_stack(engine, images_or_handles, mode="pixel", radius=4, median=1, want_tile=False):
    """The planes of one stage position -> (out, D, S) as Engine.focus_stack returns them.  A plane is a uint8 array, (h, w) or (h, w, 3)
    in B G R order, uploaded here and freed again, or the handle of a resident tile, which is only read."""
    check_options(mode, len(images_or_handles), radius, median)
    handles, mine = [], []
    try:
        for p in images_or_handles:
            if isinstance(p, (int, np.integer)):
                handles.append(int(p))
            else:
                mine.append(_upload(engine, p))
                handles.append(mine[-1])
        return engine.focus_stack(handles, mode=mode, radius=int(radius), median=int(median), want_tile=want_tile)
    finally:
        for h in mine:
            engine.tile_free(h)


def plane_histogram(D, planes):
    return [int(v) for v in np.bincount(np.asarray(D).reshape(-1), minlength=planes)[:planes]]


def fuse_dataset(stitcher, fileList, planes, outDir, extension="png"):
    """The focus series of a dataset fused position by position -> the files written, in order.

    fileList is position-major: the `planes` files of one stage position are consecutive.  A length that is no multiple of `planes`,
    planes < 2 or a position whose files differ in size (their headers, _imshape) raise ValueError before anything is decoded.  Every
    position is decoded by the decoder pool (gray, or B G R with isColorMode), uploaded, fused on the device and written losslessly to
    outDir under the stem of its first file; with focusDepthMaps the index map goes to depth/<stem>_depth.png below outDir (a folder
    of its own: imageSetStitch* takes every image of outDir for a tile).  At most GROUPS_RESIDENT
    positions are in flight at a time, and the tiles of a position are freed in a `finally`, whatever happens."""
    mode, radius, median = stitcher.focusStack, int(stitcher.focusRadius), stitcher.focusMedian
    check_options(mode, planes, radius, median)
    planes = int(planes)
    if extension.lower() not in ("png", "tif", "tiff", "bmp"):
        raise ValueError("fused tiles are written losslessly (png, tif, tiff or bmp), got %r" % (extension,))
    if len(fileList) % planes:
        raise ValueError("%d files are no whole number of positions of %d planes" % (len(fileList), planes))
    groups = [list(fileList[k:k + planes]) for k in range(0, len(fileList), planes)]
    for g in groups:
        shapes = [tuple(_imshape(f)) for f in g]
        if len(set(shapes)) != 1:
            raise ValueError("the planes of %s differ in size: %s" % (g[0], sorted(set(shapes))))
    engine, color = stitcher.engine, bool(stitcher.isColorMode)
    if not os.path.exists(outDir):
        os.makedirs(outDir)
    pool = _decoder_pool(max(1, min(16, planes * GROUPS_RESIDENT)))
    written, pending = [], []                          # pending: (group index, its decodes) of the positions ahead

    def submit(k):
        pending.append((k, [pool.submit(_imread, f, color) for f in groups[k]]))

    def settle(futs):
        """every decode of a group has ended before anything is given up; -> the images, or the first failure raised"""
        images, first = [], None
        for fu in futs:
            try:
                images.append(fu.result())
            except BaseException as e:                # noqa: PERF203
                first = first or e
        if first is not None:
            raise first
        return images

    try:
        with _PillowBlocks(color):
            for k in range(min(GROUPS_RESIDENT - 1, len(groups))):
                submit(k)
            for k in range(len(groups)):
                if k + GROUPS_RESIDENT - 1 < len(groups):
                    submit(k + GROUPS_RESIDENT - 1)
                _k, futs = pending.pop(0)
                handles = []
                try:
                    for image in settle(futs):
                        handles.append(_upload(engine, image))
                    out, D, S = engine.focus_stack(handles, mode=mode, radius=radius, median=int(median))
                finally:
                    for h in handles:
                        engine.tile_free(h)
                stem = os.path.splitext(os.path.basename(groups[k][0]))[0]
                path = os.path.join(outDir, stem + "." + extension)
                _imwrite(path, out)
                written.append(path)
                if stitcher.focusDepthMaps:
                    _imwrite(os.path.join(outDir, DEPTH_DIR, stem + "_depth.png"), D)
                if mode == "plane":
                    stitcher.printAndWrite("  focus stack %s: plane %d of %d, scores %s" % (stem, int(D.flat[0]), planes, [int(v) for v in S]))
                else:
                    stitcher.printAndWrite("  focus stack %s: pixels per plane %s" % (stem, plane_histogram(D, planes)))
    finally:
        for _k, futs in pending:                       # decodes still running read files only: wait, so none outlives the call
            for fu in futs:
                fu.cancel()
            for fu in futs:
                try:
                    fu.result()
                except BaseException:                 # noqa: PERF203
                    pass
    return written
