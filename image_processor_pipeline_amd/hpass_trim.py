"""Host restatement of the H pass's fill trim (ipp_pipe.hip hpass_block).

An H-pass block is one 16-row band of one item.  It derives the band's valid
M columns [xlo, xhi] (the columns whose source position can fall inside the
crop window; ±2 columns of slack, union over the band's 16 rows) and sweeps
only the output tiles from the first to the last one whose input window
[hdr.x, hdr.x + 64·hdr.y) meets that interval; the tiles before and after
see nothing but fill and get their constant T groups without a sweep.

This module computes the same bounds on the host, from the plan alone: the
count of trimmed (band, tile) pairs that DESIGN.md §3 quotes, and the
per-band bounds the tests use to check that their cases do trim.  Nothing
here runs on the device and the kernels do not read it.
"""
from __future__ import annotations

from typing import List, Tuple

import numpy as np

from .geometry import mfma_tiles

HP_ROWS = 16          # ipp_pipe.hip HR: M rows per band
TRIM_MAX_TILES = 64   # one header per lane: wider items are not trimmed


def _i32(v):
    """Wrap to int32 (the kernels' 32-bit wrap-around arithmetic)."""
    return ((np.asarray(v, np.int64) + (1 << 31)) % (1 << 32)) - (1 << 31)


TRIM_SLACK = 2        # columns the kernel widens each row's interval by, on both sides


def band_valid_columns(g, h, band: int, slack: int = TRIM_SLACK) -> Tuple[int, int]:
    """(xlo, xhi) of `band` of the item with gather desc `g` and H resample
    desc `h`, in the kernel's float32 arithmetic: per row the x interval where
    0 <= xx(x) < in_w·2^16 and 0 <= yy(x) < in_h·2^16 (both linear in x),
    widened by `slack` columns (the kernel's 2); then the union over the
    band's 16 rows, as the kernel takes it: rows past the item's last line
    included.  A band with no valid column gives xlo > xhi.  A smaller `slack`
    is what tests/test_hpass_trim_conservative.py holds the interval to."""
    f32 = np.float32
    b = [int(v) for v in g["b"]]
    y = int(h["line0"]) + HP_ROWS * band + np.arange(HP_ROWS, dtype=np.int64)
    rowx = _i32(b[2] + y * b[1]).astype(f32)
    rowy = _i32(b[5] + y * b[4]).astype(f32)
    lo = np.full(HP_ROWS, -1e9, f32)
    hi = np.full(HP_ROWS, 1e9, f32)
    for a, bb, lim in ((rowx, f32(b[0]), f32(65536.0) * f32(int(g["in_w"]))),
                       (rowy, f32(b[3]), f32(65536.0) * f32(int(g["in_h"])))):
        if bb == 0:
            bad = ~((a >= 0) & (a < lim))
            lo[bad], hi[bad] = 1e9, -1e9
        else:
            t1, t2 = -a / bb, (lim - a) / bb
            lo = np.maximum(lo, np.minimum(t1, t2))
            hi = np.minimum(hi, np.maximum(t1, t2))
    empty = lo > hi
    ilo = np.where(empty, 0x3FFFFFFF, np.trunc(np.maximum(lo - f32(slack), f32(-1e8))).astype(np.int64))
    ihi = np.where(empty, -0x3FFFFFFF, np.trunc(np.minimum(hi + f32(slack), f32(1e8))).astype(np.int64))
    return int(ilo.min()), int(ihi.max())


def tile_windows(axis) -> np.ndarray:
    """(n_tiles, 2) int array of (hdr.x, hdr.y) = (first input column, 64-column
    K steps) of every tile of a tap axis (ipp_plan_mfma_tile, the host
    restatement of the device tap planner)."""
    return mfma_tiles(axis)[0][:, :2].astype(np.int64)


def sweep_bounds(windows: np.ndarray, xlo: int, xhi: int) -> Tuple[int, int]:
    """[s_lo, s_hi): first to last tile whose window [x, x + 64·nK) meets
    [xlo, xhi]; (0, 0) when none does."""
    keep = (windows[:, 0] + 64 * windows[:, 1] > xlo) & (windows[:, 0] <= xhi)
    idx = np.flatnonzero(keep)
    return (int(idx[0]), int(idx[-1]) + 1) if len(idx) else (0, 0)


def trim_enabled(hsv) -> bool:
    """Does the H launch trim with these HSV parameters?  Only the forms
    without zones, and only where black (h = s = v = 0, the fill pixel) is
    excluded, i.e. some range holds 0 on all three channels: the fill quad in
    the window ring is then 0x80808080 and a fill tile's T bytes are all 0x80."""
    n = int(hsv["n_ranges"])
    r = hsv["r"][:n]
    if np.any(r["zone"] != 0):
        return False
    return bool(np.any(np.all((r["lo"] <= 0) & (r["hi"] >= 0), axis=-1)))


def desc_item(plan, i: int) -> int:
    """The item of descriptor `i` of a PipePlan (processing order, plan.order)
    or of a ScenePlan (layer-major, plan.desc_item)."""
    return int(plan.desc_item[i] if hasattr(plan, "desc_item") else plan.order[i])


def h_axis(plan, i: int):
    """The H tap axis of descriptor `i` of a PipePlan or a ScenePlan: the axes
    are in item order, the descriptors are not (desc_item)."""
    ax = plan.axes[2 * desc_item(plan, i)]
    assert int(ax["coef_off"]) == int(plan.descs[i]["h"]["coef_off"])
    return ax


def item_bounds(plan, i: int) -> List[Tuple[int, int, int]]:
    """(s_lo, s_hi, n_tiles) of every band of descriptor `i` of a PipePlan or a
    ScenePlan."""
    d = plan.descs[i]
    win = tile_windows(h_axis(plan, i))
    nt = len(win)
    assert nt == (int(d["h"]["out_len"]) + 15) >> 4
    out = []
    for band in range((int(d["h"]["lines"]) + HP_ROWS - 1) // HP_ROWS):
        if nt > TRIM_MAX_TILES:
            out.append((0, nt, nt))
            continue
        xlo, xhi = band_valid_columns(d["g"], d["h"], band)
        out.append(sweep_bounds(win, xlo, xhi) + (nt,))
    return out


def trim_counts(plan, items=None) -> Tuple[int, int]:
    """(trimmed, total) (band, tile) pairs over the plan's descriptors (or
    those in `items`): total = Σ bands · tiles, trimmed = those outside
    their band's [s_lo, s_hi)."""
    trimmed = total = 0
    for i in (range(len(plan.descs)) if items is None else items):
        for s_lo, s_hi, nt in item_bounds(plan, i):
            total += nt
            trimmed += nt - (s_hi - s_lo)
    return trimmed, total
