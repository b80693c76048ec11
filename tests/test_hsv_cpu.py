"""CPU checks behind the HSV parity tests: the oracle's HSV against a
real-valued conversion over all 2^24 colours, the conditions the GPU sweeps of
test_gpu_hsv_variants.py rest on (tests/hsv_refs.py), and the edges of
geometry.hsv_params."""
import numpy as np
import pytest

from oracle import ops
from tests import hsv_refs as R


# --------------------------------------------------------------------------- oracle vs real-valued HSV

def real_hsv(rgb: np.ndarray):
    """HSV from the definition, in float64, on OpenCV's 8-bit scales: V = max,
    S = 255·d / V, H = 30·(sector offset + numerator / d) wrapped into
    [0, 180); S = 0 for black, H = 0 for greys."""
    c = np.asarray(rgb, np.float64)
    r, g, b = c[..., 0], c[..., 1], c[..., 2]
    v = np.maximum(np.maximum(r, g), b)
    d = v - np.minimum(np.minimum(r, g), b)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(v > 0, 255.0 * d / v, 0.0)
        h = np.where(v == r, (g - b) / d, np.where(v == g, 2.0 + (b - r) / d, 4.0 + (r - g) / d))
    h = np.where(d > 0, 30.0 * h, 0.0)
    h = np.where(h < 0, h + 180.0, h)
    return h, s, v


@pytest.fixture(scope="module")
def all_colours():
    """One pass over all 2^24 colours (a 256×256 slab per red value): the
    maxima of |H - H_real| (circular) and |S - S_real|, whether V is equal,
    the hue values taken, and the (sector, numerator, d) keys that occur."""
    x = np.arange(256, dtype=np.uint8)
    g, b = np.meshgrid(x, x, indexing="ij")
    st = {"h_err": 0.0, "s_err": 0.0, "v_equal": True, "hues": np.zeros(256, bool),
          "keys": np.zeros(3 << 17, bool), "vd": np.zeros((256, 256), bool)}
    for r in range(256):
        rgb = np.stack([np.full_like(g, r), g, b], -1).reshape(-1, 3)
        hsv = R.hsv_of_rgb(rgb)
        h, s, v = real_hsv(rgb)
        dh = np.abs(hsv[:, 0] - h)
        st["h_err"] = max(st["h_err"], float(np.minimum(dh, 180.0 - dh).max()))
        st["s_err"] = max(st["s_err"], float(np.abs(hsv[:, 1] - s).max()))
        st["v_equal"] &= bool(np.array_equal(hsv[:, 2], v.astype(np.int64)))
        st["hues"][hsv[:, 0]] = True
        sec, num, d = R.hue_key(rgb)
        st["keys"][R.pack_hue_key(sec, num, d)] = True
        st["vd"][hsv[:, 2], d] = True
    return st


def test_oracle_hsv_within_one_of_real_hsv(all_colours):
    """ops.bgr_to_hsv restates OpenCV's fixed-point RGB2HSV_b; a fixed-point
    result that is the floor or the ceiling of the real value lies within 1 of
    it, and a wrong sector, wrap or table entry is off by 1 or more.  Measured
    maxima: 0.64 for H, 0.52 for S."""
    print(f"max |H - H_real| = {all_colours['h_err']:.4f}, max |S - S_real| = {all_colours['s_err']:.4f}")
    assert all_colours["v_equal"]
    assert all_colours["s_err"] < 1.0
    assert all_colours["h_err"] < 1.0


def test_oracle_hue_takes_0_to_179(all_colours):
    assert all_colours["hues"][:180].all() and not all_colours["hues"][180:].any()


# --------------------------------------------------------------------------- the sweeps' conditions

@pytest.fixture(scope="module")
def pal():
    p = R.palette()
    return p, R.hsv_of_rgb(p)


def test_palette_covers_every_v_d_pair(pal, all_colours):
    p, hsv = pal
    assert p.dtype == np.uint8 and p.shape[1] == 3 and len(p) <= 1 << 18
    _, _, d = R.hue_key(p)
    got = np.zeros((256, 256), bool)
    got[hsv[:, 2], d] = True
    v, dd = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    assert np.array_equal(got, dd <= v)
    assert np.array_equal(got, all_colours["vd"])


def test_palette_covers_every_sector_numerator_d(pal, all_colours):
    """Recomputed from the colours: the palette has every (sector, numerator,
    d) key that any of the 2^24 colours has; that is every |numerator| <= d of
    the red sector, and of the green and blue sectors all but the ties that
    the sector priority hands to an earlier sector (green: numerator = -d means
    r = v; blue: numerator = ±d means r = v or g = v)."""
    p, _ = pal
    got = np.zeros(3 << 17, bool)
    got[R.pack_hue_key(*R.hue_key(p))] = True
    assert np.array_equal(got, all_colours["keys"])
    d, n = np.meshgrid(np.arange(256), np.arange(-255, 256), indexing="ij")
    want = np.zeros(3 << 17, bool)
    for sector, ok in ((0, np.abs(n) <= d),
                       (1, (np.abs(n) <= d) & (n > -d)),
                       (2, np.abs(n) < d)):
        want[R.pack_hue_key(np.full_like(d[ok], sector), n[ok], d[ok])] = True
    assert np.array_equal(got, want)
    # both channel orderings of every numerator, ties included, were generated
    c = p.astype(np.int64)
    for sector in range(3):
        a, b = c[:, (sector + 1) % 3], c[:, (sector + 2) % 3]
        top = c[:, sector] == c.max(axis=1)
        dd = c[:, sector] - c.min(axis=1)
        pairs = np.zeros((511, 256), bool)
        pairs[(a - b)[top] + 255, dd[top]] = True
        assert np.array_equal(pairs, (np.abs(n) <= d).T), sector


@pytest.mark.parametrize("per_run", [16, 4])
@pytest.mark.parametrize("channel", R.CHANNELS, ids=R.CHANNEL_NAMES)
def test_sweeps_separate_the_palette(pal, channel, per_run):
    _, hsv = pal
    runs = R.sweep(channel, per_run)
    assert all(len(run) == per_run and len(set(run)) == per_run for run in runs)
    vals = sorted({f[channel] for run in runs for f in run})
    assert vals == list(range(0, R.TOP[channel] + 1, 2))
    assert R.separated(hsv, runs, channel).all()
    # the union of the runs excludes a colour exactly when its value is even
    ex = np.zeros(len(hsv), bool)
    for run in runs:
        ex |= R.excluded(hsv, run)
    assert np.array_equal(ex, hsv[:, channel] % 2 == 0)
    # and no run excludes the spine colour of the video frames
    odd = R.hsv_of_rgb(R.odd_colour()[None])
    assert not any(R.excluded(odd, run).any() for run in runs)


def test_separated_says_no_for_a_blunt_range():
    """The predicate is no tautology: under one wide range a colour in its
    middle does not feel a step of one."""
    hsv = np.array([[50, 100, 100], [40, 100, 100], [60, 100, 100]])
    runs = [[(40, 0, 0, 60, 255, 255)]]
    assert R.separated(hsv, runs, R.H).tolist() == [False, False, False]
    runs = [[(40, 0, 0, 60, 255, 255)], [(50, 0, 0, 50, 255, 255)]]
    assert R.separated(hsv, runs, R.H).tolist() == [True, False, False]


def test_excluded_equals_the_oracle_mask(pal):
    p, hsv = pal
    ranges = [(15, 60, 200, 35, 255, 255), (100, 3, 9, 170, 254, 254), (50, 0, 0, 10, 255, 255), (0, 0, 0, 180, 255, 40)]
    a = ops.hsv_alpha_mask(p[None, :, ::-1], ranges)[0]
    assert np.array_equal(R.excluded(hsv, ranges), a == 0)


def test_palette_frame_layout(pal):
    p, _ = pal
    spine = R.odd_colour()
    fr = R.palette_frame(p, spine, 1024)
    assert (fr[0] == spine).all() and (fr[:, 0::2] == spine).all()
    assert np.array_equal(fr[1:, 1::2].reshape(-1, 3)[:len(p)], p)


# --------------------------------------------------------------------------- hsv_params edges

def _distinct_ranges(n):
    return [(10 * k, k, 2 * k, 10 * k + 5, 200 + k, 220 + k) for k in range(n)]


def test_hsv_params_takes_16_ranges_and_refuses_17():
    from image_processor_pipeline_amd import _native as N
    from image_processor_pipeline_amd import geometry as G
    assert N.IPP_MAX_HSV_RANGES == 16
    p = G.hsv_params(_distinct_ranges(16))
    assert int(p["n_ranges"]) == 16
    for k, f in enumerate(_distinct_ranges(16)):
        assert p["r"][k]["lo"].tolist() == list(f[:3]) and p["r"][k]["hi"].tolist() == list(f[3:])
    with pytest.raises(NotImplementedError):
        G.hsv_params(_distinct_ranges(17))
    # 16 surviving ranges among 18: the two empty ones do not count
    many = _distinct_ranges(16)
    many.insert(3, (50, 0, 0, 10, 255, 255))
    many.insert(9, (0, 300, 0, 180, 400, 255))
    assert int(G.hsv_params(many)["n_ranges"]) == 16
    with pytest.raises(NotImplementedError):
        G.hsv_params(many + [(1, 2, 3, 4, 5, 6)])


@pytest.mark.parametrize("gimp", [False, True], ids=["opencv", "gimp"])
def test_hsv_params_zones_follow_their_ranges(gimp):
    """Empty ranges (lo > hi, lo > 255) are dropped; the zones of the ranges
    after them stay with their own ranges."""
    from image_processor_pipeline_amd import geometry as G
    if gimp:   # GIMP scale: H 0..360 (halved), S and V 0..100 (× 2.55)
        ranges = [(20, 10, 20, 60, 50, 60), (100, 0, 0, 40, 100, 100), (200, 30, 40, 300, 90, 95),
                  (0, 0, 0, 360, 100, 100), (600, 0, 0, 700, 100, 100), (340, 5, 6, 350, 7, 8)]
    else:
        ranges = [(10, 20, 30, 40, 50, 60), (50, 0, 0, 10, 255, 255), (5, 100, 110, 15, 200, 210),
                  (0, 300, 0, 180, 400, 255), (0, 0, 256, 180, 255, 300), (70, 1, 2, 80, 3, 4)]
    zones = [(1, 2, 3, 4), (5, 6, 7, 8), (9, 10, 11, 12), (13, 14, 15, 16), (17, 18, 19, 20), (-21, 22, -23, 24)]
    p = G.hsv_params(ranges, zones, gimp)
    want = []
    for f, z in zip(ranges, zones):
        lo, hi = ops.inrange_bounds(*np.split(np.asarray(ops.rescale_filter(f, gimp), float), 2))
        if lo[0] > hi[0] or lo[1] > hi[1] or lo[2] > hi[2]:
            continue                                   # cv::inRange's empty range
        want.append((lo, hi, list(z)))
    assert 0 < len(want) < len(ranges)
    assert int(p["n_ranges"]) == len(want)
    for k, (lo, hi, z) in enumerate(want):
        assert p["r"][k]["lo"].tolist() == lo, k
        assert p["r"][k]["hi"].tolist() == hi, k
        assert p["r"][k]["zone"].tolist() == z, k
