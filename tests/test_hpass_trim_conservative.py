"""The H pass's fill trim is conservative: the float32 interval [xlo, xhi] that
a band derives from the six 16.16 map coefficients (ipp_pipe.hip hpass_block,
restated in hpass_trim.band_valid_columns) holds every column the sampler
accepts, and the tile range [s_lo, s_hi) every tile that sees one.

The reference is the sampler's own arithmetic (ipp_sampler.h), exact: column x
of row y is inside the source iff

    0 <= (i32(b2 + y·b1 + x·b0) >> 16) < in_w  and
    0 <= (i32(b5 + y·b4 + x·b3) >> 16) < in_h

in int64 numpy wrapped to int32.  A band's valid columns are those some REAL
row of the band accepts (min(16, lines - 16·band) rows; the kernel's union
also takes the rows past the item's end, which can only widen it).

The restatement is numpy, the kernel device float32: the two may differ by an
ulp, which moves a truncated bound by one column at the most.  So the property
is required at slack 1 as well as at the kernel's slack 2: one whole column
lies between any such divergence and a wrong trim.

The grid crosses sources thousands of pixels wide or high (65536·in_w nears
2^29, where a float32 ulp is 32), angles a hair off an axis (b0 or b3 of a few
units), the folded flips, a margin window and three ratios, thinned to every
23rd combination (23 is coprime to every axis length, so each value of each
axis stays in); then geometries whose last band is a single row.

Nothing here touches the GPU.
"""
import itertools

import numpy as np
import pytest

from image_processor_pipeline_amd import fused
from image_processor_pipeline_amd import hpass_trim as HT

SIZES = [(5000, 300), (300, 5000), (8000, 65), (150, 190), (200, 24), (17, 400)]    # source (H, W)
ANGLES = [89.99, 0.01, 179.995, 269.9, 45.0, 30.0, 1.0, 123.4]
FLIPS = ["o", "h", "v", "hv"]
MARGINS = [(0, 0, 0, 0), (3, 5, 2, 1)]
RATIOS = [0.2, 0.5, 0.9]
STRIDE = 23
GRID = list(itertools.product(SIZES, ANGLES, FLIPS, MARGINS, RATIOS))[::STRIDE]
BG_HW = (512, 640)
REFUSED = "LANCZOS downscale needs a tap window wider than the fused H"
# (source heights, source widths, angle, flip, margins, ratio): the first size whose plan has lines % 16 == 1
TAILS = [(range(140, 200), [190], 45.0, "o", (0, 0, 0, 0), 0.5),
         (range(140, 200), [170], 30.0, "hv", (3, 5, 2, 1), 0.5),
         (range(40, 80), [4200], 0.01, "h", (0, 0, 0, 0), 0.9),
         (range(40, 80), [4200], 179.995, "v", (3, 5, 2, 1), 0.9),
         # (near a quarter turn the cut-out's height is even for every source size tried: no such case)
         (range(30, 70), [90], 123.4, "o", (0, 0, 0, 0), 0.9)]


def _plan(src_hw, angle, flip, margins, ratio):
    cfg = fused.PipeConfig(margins=margins)
    return fused.plan_pipe(src_hw, 1, BG_HW, 1, cfg, params=[fused.ItemParams(angle, flip, 0, ratio, 0, 0)])


def exact_valid_columns(g, h, band):
    """Sorted columns x in [0, in_len) that some real row of `band` maps inside
    the source window: the sampler's int32 wrap-around arithmetic."""
    b = [int(v) for v in g["b"]]
    nrows = min(HT.HP_ROWS, int(h["lines"]) - HT.HP_ROWS * band)
    assert nrows >= 1
    y = (int(h["line0"]) + HT.HP_ROWS * band + np.arange(nrows, dtype=np.int64))[:, None]
    x = np.arange(int(h["in_len"]), dtype=np.int64)[None, :]
    xin = HT._i32(b[2] + y * b[1] + x * b[0]) >> 16
    yin = HT._i32(b[5] + y * b[4] + x * b[3]) >> 16
    ok = (xin >= 0) & (xin < int(g["in_w"])) & (yin >= 0) & (yin < int(g["in_h"]))
    return np.flatnonzero(ok.any(axis=0))


def check_plan(plan, what):
    """Every band of the plan's one item.  Returns (problems, smallest margin
    at the kernel's slack, bands): a problem names the band and what escaped."""
    d = plan.descs[0]
    g, h = d["g"], d["h"]
    win = HT.tile_windows(HT.h_axis(plan, 0))
    assert len(win) == (int(h["out_len"]) + 15) >> 4
    nb = (int(h["lines"]) + HT.HP_ROWS - 1) // HT.HP_ROWS
    problems, margin = [], 1 << 30
    for band in range(nb):
        v = exact_valid_columns(g, h, band)
        if len(v) == 0:
            problems.append((what, band, "no valid column in the band"))
            continue
        first, last = int(v[0]), int(v[-1])
        # the tiles whose window [hdr.x, hdr.x + 64·hdr.y) holds a valid column
        a = np.searchsorted(v, win[:, 0], "left")
        need = np.flatnonzero(a < np.searchsorted(v, win[:, 0] + 64 * win[:, 1], "left"))
        if len(need) == 0:
            problems.append((what, band, "no tile's window holds a valid column"))
            continue
        for slack in (HT.TRIM_SLACK, 1):
            xlo, xhi = HT.band_valid_columns(g, h, band, slack=slack)
            if not (xlo <= first and last <= xhi):
                problems.append((what, band, f"slack {slack}: valid [{first}, {last}] outside [{xlo}, {xhi}]"))
            s_lo, s_hi = HT.sweep_bounds(win, xlo, xhi)
            if not s_lo < s_hi:
                problems.append((what, band, f"slack {slack}: empty sweep [{s_lo}, {s_hi})"))
            elif not (s_lo <= need[0] and need[-1] < s_hi):
                problems.append((what, band, f"slack {slack}: tiles {need[0]}..{need[-1]} outside [{s_lo}, {s_hi})"))
            if slack == HT.TRIM_SLACK:
                margin = min(margin, first - xlo, xhi - last)
    return problems, margin, nb


@pytest.fixture(scope="module")
def grid():
    """(results, refused) over the thinned grid, computed once."""
    results, refused = [], 0
    for combo in GRID:
        try:
            plan = _plan(*combo)
        except ValueError as e:
            if REFUSED not in str(e):
                raise
            refused += 1
            continue
        results.append((combo,) + check_plan(plan, combo))
    return results, refused


def test_grid_represents_every_axis_and_few_are_refused(grid):
    results, refused = grid
    for k, axis in enumerate((SIZES, ANGLES, FLIPS, MARGINS, RATIOS)):
        assert {c[k] for c in GRID} == set(axis), k
    planned = {c[k] for c, *_ in results for k in (0, 1)}
    assert set(SIZES) <= planned and set(ANGLES) <= planned      # also among those the planner took
    print("combinations", len(GRID), "refused", refused)
    assert len(GRID) >= 48 and 3 * refused <= len(GRID)


def test_interval_and_sweep_hold_every_valid_column(grid):
    results, _ = grid
    problems = [p for _, ps, _, _ in results for p in ps]
    margin = min(m for _, _, m, _ in results)
    bands = sum(nb for _, _, _, nb in results)
    print("bands", bands, "smallest margin at slack 2:", margin)
    assert not problems, problems[:10]


def _tail_plan(spec):
    hs, ws, angle, flip, margins, ratio = spec
    for src_hw in itertools.product(hs, ws):
        plan = _plan(src_hw, angle, flip, margins, ratio)
        if int(plan.descs[0]["h"]["lines"]) % 16 == 1:
            return src_hw, plan
    raise AssertionError(f"no size gives lines % 16 == 1: {spec}")


@pytest.mark.parametrize("spec", TAILS, ids=[f"{s[2]}-{s[3]}" for s in TAILS])
def test_one_row_last_band(spec):
    """lines % 16 == 1: the last band's union over rows is one row's interval,
    nothing widens it."""
    src_hw, plan = _tail_plan(spec)
    lines = int(plan.descs[0]["h"]["lines"])
    assert lines % 16 == 1 and lines > 16
    problems, margin, nb = check_plan(plan, (src_hw,) + spec[2:])
    print("source", src_hw, "lines", lines, "bands", nb, "smallest margin at slack 2:", margin)
    assert not problems, problems[:10]
