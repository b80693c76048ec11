"""Helpers of the HSV tests (test_hsv_cpu.py, test_gpu_hsv_variants.py).

The device has four HSV implementations (csrc/ipp_hsv.h): the standalone
``hsv_keep_alpha`` and three table forms (``hsv_tab_excl``,
``hsv_tab_excl_vfirst``, ``hsv_pre``/``hsv_post``).  The helpers here build

* ``palette()`` — a colour set that is complete for the table forms: their
  result depends on the colour only through (v, d) (the saturation product
  d·sdiv[v] and the v mask), and through (sector, numerator, d) (the hue
  product numerator·hdiv[d], the index of ``hm``);
* ``sweep()`` — range sets of single-value ranges that exclude a pixel exactly
  when one channel's value is even, so that an H, S or V off by one flips it;
* ``separated()`` — the CPU predicate that says a sweep really has that
  property for the colours fed.
"""
import numpy as np

from oracle import ops

H, S, V = 0, 1, 2
CHANNELS = (H, S, V)
CHANNEL_NAMES = ("H", "S", "V")
TOP = (179, 255, 255)          # largest value of each channel (8-bit OpenCV HSV)


def hsv_of_rgb(rgb: np.ndarray) -> np.ndarray:
    """Oracle (H, S, V) of RGB colours (..., 3), as int64."""
    return ops.bgr_to_hsv(np.asarray(rgb, np.uint8)[..., ::-1]).astype(np.int64)


def hue_key(rgb: np.ndarray):
    """(sector, numerator, d) of RGB colours (N, 3), by OpenCV's sector
    priority (v == r, then v == g, else b); the numerator is the sector's own
    (g - b, b - r or r - g, without the 2d / 4d offset)."""
    c = np.asarray(rgb, np.int64)
    r, g, b = c[..., 0], c[..., 1], c[..., 2]
    v = np.maximum(np.maximum(r, g), b)
    d = v - np.minimum(np.minimum(r, g), b)
    sector = np.where(v == r, 0, np.where(v == g, 1, 2))
    num = np.where(sector == 0, g - b, np.where(sector == 1, b - r, r - g))
    return sector, num, d


def pack_hue_key(sector, num, d) -> np.ndarray:
    """One integer < 3·2^17 per (sector, numerator, d)."""
    return (sector << 17) | ((num + 255) << 8) | d


def palette() -> np.ndarray:
    """RGB colours (N, 3) uint8, N <= 2^18: every (v, d) with 0 <= d <= v <= 255,
    and for each hue sector every (numerator, d) with |numerator| <= d in both
    channel orderings (numerator >= 0: the first of the two other channels
    carries it; < 0: the second).  |numerator| = d are the ties (two channels
    at the maximum) where the sector priority decides."""
    out = []
    v, d = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    k = d <= v
    v, d = v[k], d[k]
    out.append(np.stack([v, v - d, v - d], -1))
    d, n = np.meshgrid(np.arange(256), np.arange(-255, 256), indexing="ij")
    k = np.abs(n) <= d
    d, n = d[k], n[k]
    for sector in range(3):
        v = d + (37 * n + 11 * d + 5 * sector) % (256 - d)      # any v >= d: spread over its range
        lo = v - d
        first = lo + np.maximum(n, 0)                             # numerator = first - second
        second = lo + np.maximum(-n, 0)
        chans = [None, None, None]
        chans[sector] = v
        chans[(sector + 1) % 3] = first                           # r: g - b, g: b - r, b: r - g
        chans[(sector + 2) % 3] = second
        out.append(np.stack(chans, -1))
    pal = np.unique(np.concatenate(out).astype(np.uint8), axis=0)
    assert len(pal) <= 1 << 18
    return pal


def sweep(channel: int, per_run: int):
    """Range sets of `per_run` ranges [x, x] on `channel` (full on the other
    two) that together hold every even value of the channel (H 0..178, S and V
    0..254).  Run j holds the values 2·(j·per_run + k), k < per_run; the last
    run is filled up from the start of the list, so every run has per_run
    distinct ranges and range k of a run alone decides its value."""
    vals = list(range(0, TOP[channel] + 1, 2))
    assert per_run <= len(vals)
    runs = []
    for j in range(0, len(vals), per_run):
        xs = [vals[(j + k) % len(vals)] for k in range(per_run)]
        run = []
        for x in xs:
            f = [0, 0, 0, 180, 255, 255]
            f[channel] = f[3 + channel] = x
            run.append(tuple(f))
        runs.append(run)
    return runs


def _channel_masks(ranges):
    """Per channel a table t[x] whose bit k says range k holds x (cv::inRange's
    prepared bounds)."""
    assert len(ranges) <= 64
    t = np.zeros((3, 256), np.uint64)
    x = np.arange(256)
    for k, f in enumerate(ranges):
        lo, hi = ops.inrange_bounds(f[:3], f[3:])
        for c in range(3):
            t[c] |= ((x >= lo[c]) & (x <= hi[c])).astype(np.uint64) << np.uint64(k)
    return t


def excluded(hsv: np.ndarray, ranges) -> np.ndarray:
    """True where some range holds the (h, s, v) triple (no zones)."""
    hsv = np.asarray(hsv, np.int64).reshape(-1, 3)
    t = _channel_masks(ranges)
    return (t[0][hsv[:, 0]] & t[1][hsv[:, 1]] & t[2][hsv[:, 2]]) != 0


def separated(hsv_values, runs, channel: int) -> np.ndarray:
    """Per (h, s, v) triple: for the move of `channel` by +1 and for the move
    by -1 there is a run whose exclusion mask changes.  Hue moves modulo 180;
    S and V are clipped at 0 and 255, and a move that the clipping cancels
    asks nothing."""
    hsv = np.asarray(hsv_values, np.int64).reshape(-1, 3)
    x = hsv[:, channel]
    if channel == H:
        up, dn = (x + 1) % 180, (x - 1) % 180
    else:
        up, dn = np.minimum(x + 1, 255), np.maximum(x - 1, 0)
    ok_up, ok_dn = up == x, dn == x
    others = [c for c in CHANNELS if c != channel]
    for ranges in runs:
        t = _channel_masks(ranges)
        rest = t[others[0]][hsv[:, others[0]]] & t[others[1]][hsv[:, others[1]]]
        base = (rest & t[channel][x]) != 0
        ok_up |= ((rest & t[channel][up]) != 0) != base
        ok_dn |= ((rest & t[channel][dn]) != 0) != base
    return ok_up & ok_dn


def odd_colour() -> np.ndarray:
    """An RGB colour whose oracle H, S and V are all odd: no range set of any
    sweep excludes it."""
    v = np.arange(256, dtype=np.uint8)
    g, b = np.meshgrid(v, v, indexing="ij")
    rgb = np.stack([np.full_like(g, 201), g, b], -1).reshape(-1, 3)
    hsv = hsv_of_rgb(rgb)
    k = np.flatnonzero((hsv % 2 == 1).all(axis=1))
    return rgb[k[0]]


def palette_frame(pal: np.ndarray, spine: np.ndarray, width: int) -> np.ndarray:
    """One (h, width, 3) image with the colours `pal` (N, 3) at the odd columns
    of rows 1.., in raster order, and `spine` everywhere else (row 0, every
    even column, the unused odd slots).  Every pixel is 8-connected to the
    spine, so when the spine is kept the kept pixels form one component."""
    assert width % 2 == 0
    per_row = width // 2
    rows = -(-len(pal) // per_row)
    fr = np.empty((1 + rows, width, 3), np.uint8)
    fr[:] = spine
    slots = fr[1:, 1::2].reshape(-1, 3)
    slots[:len(pal)] = pal
    fr[1:, 1::2] = slots.reshape(rows, per_row, 3)
    return fr


def bound_colours(ranges, pool_rgb: np.ndarray, pool_hsv: np.ndarray) -> np.ndarray:
    """For every range and channel, colours of the pool whose oracle value on
    that channel is lo - 1, lo, hi and hi + 1 (those that exist in 0..TOP) with
    the other two channels inside the range.  Raises when the pool has none."""
    out = []
    for f in ranges:
        lo, hi = ops.inrange_bounds(f[:3], f[3:])
        inside = [(pool_hsv[:, c] >= lo[c]) & (pool_hsv[:, c] <= hi[c]) for c in CHANNELS]
        for c in CHANNELS:
            rest = inside[(c + 1) % 3] & inside[(c + 2) % 3]
            for x in (lo[c] - 1, lo[c], hi[c], hi[c] + 1):
                if not 0 <= x <= TOP[c]:
                    continue
                k = np.flatnonzero(rest & (pool_hsv[:, c] == x))
                if k.size == 0:
                    raise LookupError(f"no pool colour with channel {c} = {x} inside {f}")
                out.append(pool_rgb[k[0]])
    return np.asarray(out, np.uint8)
