"""The host count of the H pass's fill trim (hpass_trim.py) on a case that can
be checked by hand: one square source turned by 45°.

The cut-out M of an S×S source at 45° is a diamond |x - c| + |y - c| <= R in
a D×D box, D ≈ S·√2, c = (D - 1) / 2, R ≈ D / 2: row y holds the valid
columns c ± (R - |y - c|).  A 16-row band's valid columns are those of its
row nearest the centre line.  A tile is trimmed when its input window
[x0, x0 + 64·nK) lies wholly left or right of them.  The kernel's interval is
conservative (±2 columns, plus the rounding of Pillow's 16.16 affine and of
the box), so the exact diamond gives an upper bound on the trimmed pairs and
the diamond widened by 5 columns a lower bound; the count must lie between.

By hand, for wide tiles: a window of w columns at the left edge is trimmed
while its right end is left of c - m, m the band's half width, so a band
trims about 2·(c - m - w/2)/stride tiles with stride = D / tiles; summed
over the bands of the diamond that is a share of roughly 1/2 - w / D of all
pairs (1/2 is the diamond's fill share, w / D the windows' overhang).  The
test checks that figure too, loosely (the bracket above is the sharp check).

Nothing here touches the GPU or the kernel's output.
"""
import numpy as np

from image_processor_pipeline_amd import fused
from image_processor_pipeline_amd import hpass_trim as HT


def _diamond_trimmed(win, D, R, lines, slack):
    """(band, tile) pairs whose window misses the band's diamond columns widened by `slack`."""
    c = (D - 1) / 2.0
    trimmed = 0
    for b in range((lines + 15) // 16):
        ys = np.arange(16 * b, min(16 * b + 16, D))
        m = float(np.max(R - np.abs(ys - c))) + slack
        keep = (win[:, 0] + 64 * win[:, 1] > c - m) & (win[:, 0] <= c + m)
        assert keep.any()
        trimmed += len(win) - int(keep.sum())
    return trimmed


def test_fill_trim_count_45_degrees():
    S = 724                                     # D = 1024 to a pixel or two
    cfg = fused.PipeConfig(margins=(0, 0, 0, 0))
    plan = fused.plan_pipe((S, S), 1, (1024, 1024), 1, cfg, params=[fused.ItemParams(45.0, "o", 0, 0.25, 0, 0)])
    assert HT.trim_enabled(plan.hsv)            # the reference ranges exclude black
    h = plan.descs[0]["h"]
    D, lines = int(h["in_len"]), int(h["lines"])
    assert abs(D - S * 2 ** 0.5) <= 2 and int(plan.items["cut_h"][0]) == D and lines == D
    win = HT.tile_windows(HT.h_axis(plan, 0))
    nt = len(win)
    assert nt == (int(h["out_len"]) + 15) // 16 and nt >= 10

    trimmed, total = HT.trim_counts(plan)
    assert total == nt * ((lines + 15) // 16)
    upper = _diamond_trimmed(win, D, S / 2 ** 0.5, lines, 0.0)
    lower = _diamond_trimmed(win, D, S / 2 ** 0.5, lines, 5.0)
    print("trimmed", trimmed, "of", total, "bracket", lower, upper)
    assert lower <= trimmed <= upper
    assert upper - lower <= 0.03 * total        # the bracket is sharp: the slack moves few tiles

    # every band's bounds are one interval and the trimmed tiles lead and trail it
    for s_lo, s_hi, n in HT.item_bounds(plan, 0):
        assert 0 <= s_lo < s_hi <= n == nt
    # the rough hand figure: 1/2 less the windows' overhang
    w = float(np.mean(64 * win[:, 1]))
    assert abs(trimmed / total - (0.5 - w / D)) < 0.05


def test_fill_trim_needs_black_excluded_and_no_zones():
    from image_processor_pipeline_amd import geometry as G
    ref = list(G.REFERENCE_HSV_RANGES)
    assert HT.trim_enabled(G.hsv_params(ref, None, False, bgr=False))
    assert not HT.trim_enabled(G.hsv_params(ref[1:], None, False, bgr=False))                 # black kept
    assert not HT.trim_enabled(G.hsv_params(ref, [None, (1, 0, 0, 0), None, None], False, bgr=False))
    assert not HT.trim_enabled(G.hsv_params([(0, 0, 1, 180, 255, 150)], None, False, bgr=False))   # v = 0 outside


def test_sweep_bounds_by_hand():
    # four tiles of one K step, windows [0,64) [16,80) [48,112) [80,144)
    win = np.array([[0, 1], [16, 1], [48, 1], [80, 1]])
    assert HT.sweep_bounds(win, 70, 75) == (1, 3)       # tile 0 ends at 64 <= 70, tile 3 starts at 80 > 75
    assert HT.sweep_bounds(win, 0, 200) == (0, 4)
    assert HT.sweep_bounds(win, 144, 300) == (0, 0)     # right of every window
    assert HT.sweep_bounds(win, 0x3FFFFFFF, -0x3FFFFFFF) == (0, 0)   # a band with no valid column
    # window ends need not grow with the tile index: a tile between two kept ones is swept
    win = np.array([[0, 2], [16, 1], [32, 2]])          # ends 128, 80, 160
    assert HT.sweep_bounds(win, 100, 110) == (0, 3)
