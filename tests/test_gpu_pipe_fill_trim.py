"""The H launch's fill trim (ipp_pipe.hip hpass_block): a band sweeps only the
output tiles from the first to the last one whose input window meets the
band's valid source columns, and the tiles before and after get their
constant T groups (every byte 0x80) without a sweep.

Every case runs the two launches of the pipe on one or a few small items and
compares each composite bit for bit with the CPU oracle
(oracle/pipe.pipe_item).  Before the launch the runner's T scratch and the
output are filled with 0x55, so a trimmed tile whose constant store is
missing leaves poison in T (a stale, correct T of an earlier run cannot hide
it) and the composite differs.  What a case is meant to exercise (tiles
trimmed at the front and at the back, none trimmed, K steps per tile, the
body taken) is asserted on the plan with the host restatement of the trim
(image_processor_pipeline_amd/hpass_trim.py), never on the kernel's output.

A band in which no tile is kept (s_lo >= s_hi) cannot come out of a plan: the
cut-out is the rotated canvas's exact alpha box, so every band holds a row
with a valid column and some tile's window covers it.
tests/test_hpass_trim_conservative.py asserts this for every band of its
geometries (no GPU).  The thin-source case reaches a band with a single kept
tile.  (A tile's window is 64 columns or more, so even a 24-px strip keeps two
or three tiles in most bands.)

For the same reason an item of one band (lines <= 16) never trims: the union
over all its rows holds every column of the box.  The one_band case therefore
pins the other thing such an item can get wrong, the interval itself: the
rows past the item's end join the union (nrows < 16), and the body gathers
only the columns inside [xlo, xhi].

The paths that share the H launch (4-channel sources, scenes, the label
kernels, the 64-tile limit) are in tests/test_gpu_pipe_fill_trim_paths.py.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import pipe as opipe

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
POISON = 0x55
NO_BLACK = [(15, 60, 200, 35, 255, 255), (100, 3, 9, 170, 254, 254)]   # no range holds h = s = v = 0

# name: (src (H, W), bg (h, w), margins, [(angle, sym, ratio)], PipeConfig extras)
CASES = {
    # prefix and suffix fill tiles in the top and bottom bands
    "oblique": ((150, 190), (256, 320), (0, 0, 0, 0), [(45.0, "o", 0.5), (30.0, "o", 0.5), (10.0, "o", 0.5)], {}),
    # no fill at all: nothing is trimmed
    "square_angles": ((150, 190), (256, 320), (0, 0, 0, 0), [(0.0, "o", 0.5), (90.0, "o", 0.5), (180.0, "o", 0.5)],
                      {}),
    # a thin strip: every band of the 30° items trims, one band keeps a single tile
    "thin": ((200, 24), (256, 320), (0, 0, 0, 0), [(30.0, "o", 0.45), (100.0, "o", 0.45), (30.0, "o", 0.2)], {}),
    # the sampler folds the flip: xlo / xhi move
    "flips": ((150, 190), (256, 320), (0, 0, 0, 0), [(20.0, s, 0.5) for s in ("o", "h", "v", "hv")], {}),
    # out_len and lines no multiples of 16: the last tile and the last band
    "ragged": ((150, 190), (256, 320), (0, 0, 0, 0), [(33.0, "o", 0.47)], {}),
    # upscale: nK = 1, dense tiles
    "upscale": ((100, 120), (512, 512), (0, 0, 0, 0), [(30.0, "o", 0.4)], {}),
    # strong downscale: nK >= 3
    "downscale": ((260, 260), (256, 256), (0, 0, 0, 0), [(30.0, "h", 0.2)], {}),
    # full-width crop of a dense source: the general (CLAMP) body
    "clamp_body": ((150, 170), (128, 160), (3, 5, 0, 0), [(30.0, "o", 0.5), (200.0, "v", 0.5)], {}),
    # black is kept: the fill quad is not 0x80808080 and trimming is off
    "no_black_range": ((150, 190), (256, 320), (0, 0, 0, 0), [(30.0, "o", 0.5)], {"hsv_ranges": NO_BLACK}),
    # zones: the untouched instantiation
    "zones": ((150, 190), (256, 320), (0, 0, 0, 0), [(30.0, "o", 0.5)],
              {"zones": [None, (10, 0, 0, 5), None, (0, 0, 20, 0)]}),
    # lines = 16: one band, whose union over the rows is the whole box (nothing can trim)
    "one_band": ((10, 200), (128, 320), (0, 0, 0, 0), [(2.0, "o", 0.5), (178.0, "hv", 0.5)], {}),
    # lines % 16 == 1: the last band is one real row and 15 rows past the item's end
    "one_row_tail": ((35, 60), (128, 160), (0, 0, 0, 0), [(40.0, "o", 0.6), (140.0, "h", 0.6)], {}),
    # a 4200-px source 0.01° off the axis, flipped: b3 = ±11, 65536·in_w = 2^28 (a float32 ulp of 16 or 32);
    # the planner takes the 8× downscale of ratio 0.9 on this background
    "near_axis_wide": ((33, 4200), (48, 640), (0, 0, 0, 0), [(0.01, "hv", 0.9), (179.995, "h", 0.9)], {}),
}


def make_plan(name):
    from image_processor_pipeline_amd import fused
    src_hw, bg_hw, margins, items, extra = CASES[name]
    cfg = fused.PipeConfig(margins=margins, **extra)
    params = [fused.ItemParams(a, s, k % 2, r, 1 + k, 2 + k) for k, (a, s, r) in enumerate(items)]
    return cfg, fused.plan_pipe(src_hw, len(params), bg_hw, 2, cfg, params=params)


def check_case(name, plan):
    """What the case is there for, asserted on the plan (host arithmetic)."""
    from image_processor_pipeline_amd import hpass_trim as HT
    n = len(plan.descs)
    bounds = [HT.item_bounds(plan, i) for i in range(n)]
    for i in range(n):
        assert int(plan.descs[i]["h"]["out_len"]) >= 40, (name, i)           # at least 3 H tiles
    on = HT.trim_enabled(plan.hsv)
    assert on == (name not in ("no_black_range", "zones")), name
    front = [sum(lo > 0 for lo, hi, nt in b) for b in bounds]                 # bands with trimmed leading tiles
    back = [sum(hi < nt for lo, hi, nt in b) for b in bounds]
    if name in ("oblique", "thin", "flips", "ragged", "upscale", "downscale", "clamp_body"):
        assert all(f > 0 for f in front) and all(k > 0 for k in back), (name, front, back)
    if name == "square_angles":
        assert not any(front) and not any(back), (name, front, back)
    if name == "thin":
        assert any(hi - lo == 1 for b in bounds for lo, hi, nt in b), (name, bounds)   # a band with one kept tile
        steep = [b for i, b in enumerate(bounds) if plan.order[i] == 0]            # the 30° item of 7 tiles
        assert len(steep) == 1 and all(hi - lo < nt for lo, hi, nt in steep[0]), (name, steep)
    if name == "ragged":
        h = plan.descs[0]["h"]
        assert int(h["out_len"]) % 16 and int(h["lines"]) % 16, (int(h["out_len"]), int(h["lines"]))
    if name in ("upscale", "downscale"):
        nk = HT.tile_windows(HT.h_axis(plan, 0))[:, 1]
        assert (nk.max() == 1) if name == "upscale" else (nk.max() >= 3), (name, nk)
    if name == "one_band":
        for i in range(n):
            assert int(plan.descs[i]["h"]["lines"]) <= 16 and len(bounds[i]) == 1, (name, i)
            assert bounds[i][0][2] <= HT.TRIM_MAX_TILES and bounds[i] == [(0, bounds[i][0][2], bounds[i][0][2])]
    if name == "one_row_tail":
        for i in range(n):
            assert int(plan.descs[i]["h"]["lines"]) % 16 == 1 and len(bounds[i]) >= 2, (name, i)
            lo, hi, nt = bounds[i][-1]
            assert hi - lo < nt, (name, i, bounds[i])                           # the one-row band trims
    if name == "near_axis_wide":
        for i in range(n):
            g, h = plan.descs[i]["g"], plan.descs[i]["h"]
            assert int(g["in_w"]) >= 4100 and 16 < int(h["lines"]) <= 48, (name, i)
            assert 0 < abs(int(g["b"][3])) <= 16 and abs(int(g["b"][0])) >= 65000, (name, i, g["b"])
            assert int(g["flip"]) != 0 and bounds[i][0][2] <= HT.TRIM_MAX_TILES
    if name == "clamp_body":
        for i in range(n):
            g = plan.descs[i]["g"]
            need = (int(g["in_h"]) - 1) * int(g["src_pitch"]) + int(g["in_w"]) * 3 + 1
            assert int(g["in_h"]) * int(g["src_pitch"]) < need, (name, i)      # yr_range_ok fails: general body


@pytest.mark.parametrize("name", list(CASES))
def test_pipe_fill_trim_vs_oracle(name):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from image_processor_pipeline_amd import fused
    cfg, plan = make_plan(name)
    check_case(name, plan)
    (H, W), (bh, bw) = CASES[name][0], CASES[name][1]
    n = len(plan.descs)
    rng = np.random.default_rng(len(name) + 17 * n)
    src = rng.integers(0, 256, (n, H, W, 3), np.uint8)
    src[:, H // 3: H // 2, W // 4: W // 2] = 0        # real black inside the source, beside the fill
    bgs = rng.integers(0, 256, (2, bh, bw, 3), np.uint8)
    runner = fused.PipeRunner(plan, DEV)
    runner.tmp.fill_(POISON)
    out = torch.full((n, bh, bw, 3), POISON, dtype=torch.uint8, device=DEV)
    runner.run(torch.from_numpy(src).to(DEV), torch.from_numpy(bgs).to(DEV), out)
    got = out.cpu().numpy()
    assert runner.status() == 0
    for i in range(n):
        exp = opipe.pipe_item(src[i], bgs, plan.params[i], cfg)
        assert np.array_equal(got[i], exp), (name, i, int((got[i] != exp).sum()))
