"""NumPy restatement of the device resize of the training batches
(ipp_scene_feed_resize, ipp_scene_feed_index_map_sampled /
SceneRunner.feed(size=...)), straight from the rule of include/ipp.h: Pillow's
Resample.c coefficients for its five convolution filters, the two 8-bit passes
through oracle.ops.resample_h / resample_v, the table, and the NEAREST
coordinate tables of Geometry.c ImagingScaleAffine (not a test module)."""
import math

import numpy as np

from oracle import ops
from tests import feed_refs as FR

FILTERS = ("box", "bilinear", "hamming", "bicubic", "lanczos")
F32 = np.float32


def _box(x):
    return 1.0 if -0.5 < x <= 0.5 else 0.0


def _bilinear(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def _hamming(x):
    x = abs(x)
    if x == 0.0:
        return 1.0
    if x >= 1.0:
        return 0.0
    x = x * math.pi
    return math.sin(x) / x * (float(F32(0.54)) + float(F32(0.46)) * math.cos(x))   # Resample.c: 0.54f + 0.46f * cos(x)


def _bicubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


FILTER = {"box": (_box, 0.5), "bilinear": (_bilinear, 1.0), "hamming": (_hamming, 1.0), "bicubic": (_bicubic, 2.0),
          "lanczos": (ops.lanczos_filter, 3.0)}


def coeffs(name, in_size, out_size):
    """oracle.ops.precompute_coeffs (in0 = 0, in1 = in_size) with the filter and its support generalised:
    (ksize, bounds[out, 2] (xmin, count), taps[out, ksize])."""
    f, sup = FILTER[name]
    scale = in_size / out_size
    filterscale = scale if scale >= 1.0 else 1.0
    support = sup * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int64)
    kk = np.zeros((out_size, ksize), np.int64)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = 0.0 + (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        k = [f((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in k:
            ww += v
        for x in range(xmax):
            v = k[x] / ww if ww != 0.0 else k[x]
            kk[xx, x] = int(-0.5 + v * (1 << 22)) if v < 0 else int(0.5 + v * (1 << 22))
        bounds[xx] = (xmin, xmax)
    return ksize, bounds, kk


def identity(n):
    """geometry.identity_taps in the same form: the axis Pillow skips."""
    return 1, np.stack([np.arange(n), np.ones(n, np.int64)], axis=1), np.full((n, 1), 1 << 22, np.int64)


def axis(name, in_size, out_size):
    return identity(in_size) if in_size == out_size else coeffs(name, in_size, out_size)


def unpack(buf, out_size, ksize):
    """(bounds, taps) of the planner's int32[2·out + out·ksize] layout."""
    buf = np.asarray(buf).astype(np.int64)
    return buf[:2 * out_size].reshape(out_size, 2), buf[2 * out_size:].reshape(out_size, ksize)


def pack(bounds, kk):
    """The planner's layout of (bounds, taps), int32."""
    return np.concatenate([np.asarray(bounds).reshape(-1), np.asarray(kk).reshape(-1)]).astype(np.int32)


def resize(img, oh, ow, tx, ty):
    """(oh, ow, C) uint8 of the (H, W, C) image: the horizontal pass, rounded and clipped to uint8, then the
    vertical one; tx, ty = (bounds, taps) per axis."""
    return ops.resample_v(ops.resample_h(img, ow, *tx), oh, *ty)


def resize_named(img, oh, ow, name):
    H, W = img.shape[:2]
    return resize(img, oh, ow, axis(name, W, ow)[1:], axis(name, H, oh)[1:])


def images(comps, lut, bgr, oh, ow, tx, ty):
    """(S, 3, oh, ow) of the table's words: FR.images of the resized composites (the table comes last)."""
    return FR.images(np.stack([resize(c, oh, ow, tx, ty) for c in comps]), lut, bgr)


def nearest_table(in_size, out_size):
    """ImagingScaleAffine's coordinate table of a full-axis NEAREST resize: int(o), o from 0.5·(in / out) by
    repeated addition of in / out in double."""
    step = in_size / out_size
    o = 0.0 + step * 0.5
    out = []
    for _ in range(out_size):
        out.append(int(o))
        o += step
    return np.array(out, np.int64)


def nearest(img, oh, ow):
    """NEAREST resize of an (H, W) array through the two tables."""
    return img[nearest_table(img.shape[0], oh)][:, nearest_table(img.shape[1], ow)]
