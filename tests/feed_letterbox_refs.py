"""A plain restatement of the three rules of the letterboxed training batches
(include/ipp.h: ipp_scene_feed_letterbox, ipp_scene_feed_targets_letterbox,
ipp_scene_feed_index_map_letterbox), with Pillow as the judge of the pixels and
NumPy in float64 of the targets (not a test module).  ``geo`` is a
``labels_fmt.Letterbox`` (out_h, out_w, new_h, new_w, top, left)."""
import numpy as np
from PIL import Image

from tests import feed_refs as FR
from tests import feed_resize_refs as RR

PIL_FILTER = {"box": Image.Resampling.BOX, "bilinear": Image.Resampling.BILINEAR, "hamming": Image.Resampling.HAMMING,
              "bicubic": Image.Resampling.BICUBIC, "lanczos": Image.Resampling.LANCZOS}


def canvas(img, geo, name, pad):
    """(out_h, out_w, 3) uint8: Pillow's resize of the (H, W, 3) image to (new_w, new_h), pasted at (left, top) on a
    canvas filled with `pad`."""
    out = Image.new("RGB", (geo.out_w, geo.out_h), (pad, pad, pad))
    out.paste(Image.fromarray(img).resize((geo.new_w, geo.new_h), PIL_FILTER[name]), (geo.left, geo.top))
    return np.asarray(out)


def images(comps, lut, bgr, geo, name, pad):
    """(S, 3, out_h, out_w) of the table's words: the table comes last, over the pad too."""
    return FR.images(np.stack([canvas(c, geo, name, pad) for c in comps]), lut, bgr)


def targets(rows, class_ids, bg_w, bg_h, min_q, geo, present=None):
    """FR.targets with the ROW of the letterbox: int64 numerators and denominators, one float64 division, one
    rounding to float32.  Kept, order, slot and count are FR.targets' own."""
    rows = np.asarray(rows)
    out, n, slot = FR.targets(rows, class_ids, bg_w, bg_h, min_q, present)
    i64, f64 = np.int64, np.float64
    for (s, k), r in np.ndenumerate(slot):
        if r < 0:
            continue
        x0, y0, x1, y1 = (i64(v) for v in rows[s, k, :4])
        dx, dy = i64(bg_w) * i64(geo.out_w), i64(bg_h) * i64(geo.out_h)
        out[r, 2] = np.float32(f64((x0 + x1) * i64(geo.new_w) + 2 * i64(geo.left) * i64(bg_w)) / f64(2 * dx))
        out[r, 3] = np.float32(f64((y0 + y1) * i64(geo.new_h) + 2 * i64(geo.top) * i64(bg_h)) / f64(2 * dy))
        out[r, 4] = np.float32(f64((x1 - x0) * i64(geo.new_w)) / f64(dx))
        out[r, 5] = np.float32(f64((y1 - y0) * i64(geo.new_h)) / f64(dy))
    return out, n, slot


def index_map(full, geo):
    """(S, out_h, out_w) uint8 of the full-size index maps (S, H, W): the NEAREST resize to (new_h, new_w) through
    RR.nearest_table at (top, left), 0 around it."""
    full = np.asarray(full)
    out = np.zeros((full.shape[0], geo.out_h, geo.out_w), np.uint8)
    out[:, geo.top:geo.top + geo.new_h, geo.left:geo.left + geo.new_w] = \
        np.stack([RR.nearest(f, geo.new_h, geo.new_w) for f in full])
    return out
