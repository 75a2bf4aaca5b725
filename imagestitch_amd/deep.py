"""Array-level operators over 16-bit tiles (no reference counterpart; tests/deep_shading_ref.py is the specification).

A 12- or 16-bit camera is used where intensities are measured, and a mosaic gathered from uncorrected tiles shows every tile's illumination
fall-off as a grid.  flatfield16 takes that fall-off out of a stack of tiles before they are placed: the arithmetic runs in
csrc/deep_shading_kernels.hip behind Engine.deep_shading_*; the 8-bit views are never involved, so no bit of the samples is given up.
"""
import numpy as np


def flatfield16(engine, tiles16, percentile=50, radius=32, pedestal=0, gain=None):
    """Host uint16 tiles of one shape (h, w) -> (corrected arrays, gain).  The gain (uint16 Q12) is estimated from the stack -- the
    `percentile` order statistic per position, less the camera's dark level `pedestal`, smoothed by two box passes of `radius` -- or
    taken as given (a blank-slide measurement), and applied above the pedestal.  Everything uploaded or created here is freed again,
    whatever happens."""
    tiles16 = [np.asarray(t) for t in tiles16]
    if not tiles16:
        raise ValueError("flatfield16 needs at least one tile")
    for t in tiles16:
        if t.dtype != np.uint16 or t.ndim != 2 or t.shape != tiles16[0].shape:
            raise ValueError("flatfield16 takes uint16 arrays of one shape (h, w), got %s %s" % (t.dtype, t.shape))
    handles, field = [], None
    try:
        for t in tiles16:
            handles.append(engine.deep_upload(t))
        if gain is None:
            field = engine.deep_shading_estimate(handles, percentile=percentile, radius=radius, pedestal=pedestal)
        else:
            field = engine.deep_shading_from_gain(gain, pedestal=pedestal)
        engine.deep_shading_apply(field, handles)
        return [engine.deep_download(h) for h in handles], engine.deep_shading_download(field)[0]
    finally:
        if field is not None:
            engine.deep_shading_free(field)
        for h in handles:
            engine.deep_free(h)
