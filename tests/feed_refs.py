"""NumPy references of the device training batches (ipp_scene_feed_images,
ipp_scene_feed_targets, ipp_scene_feed_index_map / SceneRunner.feed), straight
from the rules of include/ipp.h (not a test module)."""
import numpy as np


def images(img, lut, bgr=False):
    """(S, 3, H, W) of the table's words: out[s, c, y, x] = lut[c][img[s, y, x, ch(c)]], ch(c) = c or 2 - c."""
    img, lut = np.asarray(img), np.asarray(lut)
    assert img.dtype == np.uint8 and img.ndim == 4 and img.shape[3] == 3 and lut.shape == (3, 256)
    return np.stack([lut[c][img[..., 2 - c if bgr else c]] for c in range(3)], axis=1)


def kept(rows, min_q):
    """(S, K) bool: visible > 0 and 65536·visible >= min_q·area, in Python integers."""
    rows = np.asarray(rows)
    S, K = rows.shape[:2]
    return np.array([[int(rows[s, k, 5]) > 0 and 65536 * int(rows[s, k, 5]) >= int(min_q) * int(rows[s, k, 4])
                      for k in range(K)] for s in range(S)], bool).reshape(S, K)


def targets(rows, class_ids, bg_w, bg_h, min_q, present=None):
    """(targets (S·K, 6) float32, count, slot (S, K) int32) of the (S, K, 6)
    rows in scene, layer order.  ``class_ids``: an int or S·K of them,
    scene-major; ``present`` (S, K) bool: the overlays that have a descriptor."""
    rows = np.asarray(rows)
    S, K = rows.shape[:2]
    ids = np.full(S * K, class_ids, np.int64) if np.ndim(class_ids) == 0 else np.asarray(class_ids, np.int64)
    keep = kept(rows, min_q) & (np.ones((S, K), bool) if present is None else np.asarray(present))
    out = np.full((S * K, 6), -1, np.float32)
    slot = np.full((S, K), -1, np.int32)
    n = 0
    f = np.float32
    for s in range(S):
        for k in range(K):
            if not keep[s, k]:
                continue
            x0, y0, x1, y1 = (int(v) for v in rows[s, k, :4])
            out[n] = (f(s), f(ids[s * K + k]), f(x0 + x1) / f(2 * bg_w), f(y0 + y1) / f(2 * bg_h),
                      f(x1 - x0) / f(bg_w), f(y1 - y0) / f(bg_h))
            slot[s, k] = n
            n += 1
    return out, n, slot


def index_map(vis, slot, bg_w):
    """(S, H, pitch) uint8 of the (S, H, pitch) visibility maps and slot (S, K):
    0 where no kept layer's bit is set, else 1 + the kept layers below the
    topmost kept bit; 0 in the columns from bg_w on."""
    vis, slot = np.asarray(vis), np.asarray(slot)
    S, K = slot.shape
    out = np.zeros_like(vis)
    for s in range(S):
        mask = sum(1 << k for k in range(K) if slot[s, k] >= 0)
        table = np.zeros(256, np.uint8)
        for v in range(256):
            m = v & mask
            if m:
                table[v] = 1 + bin(mask & ((1 << (m.bit_length() - 1)) - 1)).count("1")
        out[s] = table[vis[s]]
    out[:, :, bg_w:] = 0
    return out


def random_rows(rng, S, K, bg_w, bg_h):
    """(S, K, 6) rows: a third absent (-1, -1, -1, -1, area, 0), the others a
    box inside the background with 1 <= visible <= area; fractions of exactly
    1/4, 1/2 and 1 are frequent so that every min_q of the tests has ties."""
    rows = np.empty((S, K, 6), np.int32)
    for s in range(S):
        for k in range(K):
            area = int(rng.integers(1, 5000)) * 4
            kind = int(rng.integers(0, 6))
            if kind < 2:
                rows[s, k] = (-1, -1, -1, -1, area if kind else 0, 0)
                continue
            vis = (area // 4, area // 2, area, int(rng.integers(1, area + 1)))[kind - 2]
            x0, y0 = int(rng.integers(0, bg_w)), int(rng.integers(0, bg_h))
            rows[s, k] = (x0, y0, int(rng.integers(x0 + 1, bg_w + 1)), int(rng.integers(y0 + 1, bg_h + 1)), area, vis)
    return rows
