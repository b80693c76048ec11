"""Every HSV kernel variant against the oracle: H, S and V value by value
(sweeps over tests/hsv_refs.palette()), and every dispatch variant at small
shapes.  The conditions the sweeps rest on are asserted on the CPU in
tests/test_hsv_cpu.py and again here on the colours each test feeds.

Which test runs which template instantiation (V = this module, P =
test_gpu_parity.py):

k_pipe_hpass2<NR, ZONES, CN>  (ipp_pipe.hip hpass_entry; hsv_tab_excl<NR, false>)
  NR   zones  CN 3                                         CN 4
  1    no     V test_pipe_variants[1-plain], P BLACK/NEVER  V test_pipe_cn4[1-plain]
  1    yes    V test_pipe_variants[1-zones]                 V test_pipe_cn4[1-zones]
  2    no     V test_pipe_variants[2-plain]                 V test_pipe_cn4[2-plain]
  2    yes    V test_pipe_variants[2-zones]                 V test_pipe_cn4[2-zones]
  3    no     V test_pipe_variants[3-plain]                 V test_pipe_cn4[3-plain]
  3    yes    V test_pipe_variants[3-zones], P VS_RANGES    V test_pipe_cn4[3-zones]
  4    no     V test_pipe_variants[4-plain], P (reference)  V test_pipe_cn4[4-plain]
  4    yes    V test_pipe_variants[4-zones]                 V test_pipe_cn4[4-zones]
  6    no     V test_pipe_variants[5/6-plain]               V test_pipe_cn4[6-plain]
  6    yes    V test_pipe_variants[5/6-zones]               V test_pipe_cn4[6-zones]
  16   no     V test_pipe_variants[7/16-plain],
              V test_pipe_sweep[H/S/V]                      V test_pipe_cn4[16-plain]
  16   yes    V test_pipe_variants[7/16-zones]              V test_pipe_cn4[16-zones]
  Each instantiation has a fast and a CLAMP body (block-uniform choice,
  hpass_block).  CN 3: crops that reach the source's last pixel take CLAMP
  (P test_pipe_crop_reaching_source_end, V test_pipe_cn4's 3-channel runs).
  CN 4: a dword at the last pixel fits, so tight rows always take the fast
  body; CLAMP is taken once 32768 * pitch + need > 2^32 (yr_range_ok), i.e.
  rows padded to a pitch >= 131072 bytes: V test_pipe_cn4_padded_pitch
  (NR 4 plain, 6 and 16 with zones).

k_ccl_label<SRC_HSV, NR, ZONES>  (ipp_ccl.hip run_labels)
  4    no     V test_video_sweep_4_ranges (tile_words_quads: hsv_pre/hsv_post;
              edge tiles: hsv_tab_excl_vfirst), P test_video_chain_*
  4    yes    V test_video_variants[4-zones], [gimp]       (tile_words<.., ZONES>)
  16   no     V test_video_sweep_16_ranges, test_video_variants[16-plain]
  16   yes    V test_video_variants[16-zones]               (hsv_tab_excl<16, true>)

k_hsv_mask  (ipp_hsv.hip; hsv_keep_alpha)
  cn 3 / 4, bgr 1 / 0   V test_hsv_mask_sweep[H/S/V] (all four), test_hsv_mask_all_colours (cn 3, bgr 1)
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import ops
from oracle import pipe as opipe
from tests import hsv_refs as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CH = pytest.mark.parametrize("channel", R.CHANNELS, ids=R.CHANNEL_NAMES)


@pytest.fixture(scope="module")
def D():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from image_processor_pipeline_amd import device
    return device


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope="module")
def pal():
    """(palette RGB, its oracle HSV, the all-odd colour)."""
    p = R.palette()
    return p, R.hsv_of_rgb(p), R.odd_colour()


@pytest.fixture(scope="module")
def pool():
    """Colours to plant on range bounds: the palette and 2^20 random ones,
    with their oracle HSV."""
    rgb = np.concatenate([R.palette(), np.random.default_rng(3).integers(0, 256, (1 << 20, 3), np.uint8)])
    return rgb, R.hsv_of_rgb(rgb)


def _assert_separated(rgb, runs, channel):
    """The sweep's condition on the colours actually fed."""
    hsv = np.unique(R.hsv_of_rgb(np.asarray(rgb).reshape(-1, 3)), axis=0)
    assert R.separated(hsv, runs, channel).all()


# --------------------------------------------------------------------------- 3a. standalone ipp_hsv_mask

@CH
def test_hsv_mask_sweep(D, pal, channel):
    """hsv_keep_alpha, value by value: 3- and 4-channel sources (junk in the
    dropped byte), BGR and RGB order."""
    from image_processor_pipeline_amd import geometry as G
    p, _, odd = pal
    rgb = R.palette_frame(p, odd, 1024)
    runs = R.sweep(channel, 16)
    _assert_separated(rgb, runs, channel)
    junk = np.random.default_rng(1).integers(0, 256, rgb.shape[:2] + (1,), np.uint8)
    srcs = {}
    for bgr in (1, 0):
        img = rgb[..., ::-1] if bgr else rgb
        srcs[bgr, 3] = (img, _t(img))
        srcs[bgr, 4] = (img, _t(np.concatenate([img, junk], -1)))
    for j, ranges in enumerate(runs):
        alpha = ops.hsv_alpha_mask(rgb[..., ::-1], ranges)
        for (bgr, cn), (img, dev_img) in srcs.items():
            got = D.hsv_mask(dev_img, G.hsv_params(ranges, None, False, bgr=bool(bgr))).cpu().numpy()
            assert np.array_equal(got[..., :3], img), (j, bgr, cn)
            assert np.array_equal(got[..., 3], alpha), (j, bgr, cn)


def test_hsv_mask_all_colours(D):
    """All 2^24 colours as one 4096×4096 image under the three ranges of
    test_gpu_parity.test_hsv_all_pixel_values (which has 16 red values)."""
    from image_processor_pipeline_amd import geometry as G
    i = np.arange(1 << 24, dtype=np.uint32)
    img = np.stack([i & 255, (i >> 8) & 255, i >> 16], -1).astype(np.uint8).reshape(4096, 4096, 3)
    ranges = [(0, 0, 0, 180, 255, 150), (15, 60, 200, 35, 255, 255), (100, 3, 9, 170, 254, 254)]
    got = D.hsv_mask(_t(img), G.hsv_params(ranges, None, False, bgr=True))
    assert torch.equal(got[..., :3], _t(img))
    for y in range(0, 4096, 512):
        exp = ops.hsv_alpha_mask(img[y:y + 512], ranges)
        assert torch.equal(got[y:y + 512, :, 3], _t(exp)), y


# --------------------------------------------------------------------------- 3b/3c. video chain sweeps

def _video_sweep(pal, channel, per_run, width):
    """The palette at the odd columns of one BGR frame, a kept spine at row 0
    and the even columns: every kept pixel touches the spine, so the chain's
    largest component is the whole mask and its output is the oracle's mask
    cropped to the kept pixels' bounding box."""
    from scipy import ndimage
    from image_processor_pipeline_amd.video_chain import VideoChain
    p, _, odd = pal
    fr = np.ascontiguousarray(R.palette_frame(p, odd, width)[..., ::-1])
    runs = R.sweep(channel, per_run)
    _assert_separated(fr[..., ::-1], runs, channel)
    dev_fr = _t(fr[None])
    h, w = fr.shape[:2]
    for j, ranges in enumerate(runs):
        exp = ops.color_mask_bgra(fr, ranges)
        keep = exp[..., 3] != 0
        assert keep[0].all() and keep[:, 0::2].all()
        assert ndimage.label(keep, np.ones((3, 3)))[1] == 1
        ys, xs = np.flatnonzero(keep.any(axis=1)), np.flatnonzero(keep.any(axis=0))
        exp = exp[ys[0]:ys[-1] + 1, xs[0]:xs[-1] + 1]
        chain = VideoChain(1, h, w, DEV, ranges)
        assert int(chain.hsv["n_ranges"]) == per_run
        chain.run(dev_fr)
        res = chain.results()[0]
        assert res is not None and np.array_equal(res, exp), j


@pytest.mark.parametrize("width", [1024, 7404], ids=["interior", "edge"])
@CH
def test_video_sweep_4_ranges(D, pal, channel, width):
    """k_ccl_label<SRC_HSV, 4, no zones>.  1024 px wide: 16 × 7 interior tiles
    (tile_words_quads: hsv_pre / hsv_post) and a partial tile row; 7404 px
    wide: 63 rows, so every tile is an edge tile (tile_words:
    hsv_tab_excl_vfirst)."""
    _video_sweep(pal, channel, 4, width)


@CH
def test_video_sweep_16_ranges(D, pal, channel):
    """k_ccl_label<SRC_HSV, 16, no zones>: hsv_tab_excl<16, true>, uint16 masks
    and the separate vm table."""
    _video_sweep(pal, channel, 16, 1024)


# --------------------------------------------------------------------------- 3d. pipe H pass sweep

@CH
def test_pipe_sweep(D, pal, channel):
    """hsv_tab_excl<16, false> (RGB order) in k_pipe_hpass2: one item whose
    source carries the palette, unrotated and upscaled, so every pixel of the
    source is a pixel of the cut-out and every mask bit reaches the
    composite."""
    from image_processor_pipeline_amd import fused
    p, _, odd = pal
    side, m, bg_side = 480, 2, 640
    assert len(p) <= side * side
    cells = np.empty((side * side, 3), np.uint8)
    cells[:] = odd
    cells[:len(p)] = p
    src = np.empty((1, side + 2 * m, side + 2 * m, 3), np.uint8)
    src[:] = odd
    src[0, m:-m, m:-m] = cells.reshape(side, side, 3)
    bgs = np.random.default_rng(2).integers(0, 256, (1, bg_side, bg_side, 3), np.uint8)
    params = [fused.ItemParams(angle=0.0, sym="o", bg_index=0, ratio=0.8, x=37, y=53)]
    runs = R.sweep(channel, 16)
    dev_src, dev_bgs = _t(src), _t(bgs)
    out = torch.empty((1, bg_side, bg_side, 3), dtype=torch.uint8, device=DEV)
    for j, ranges in enumerate(runs):
        cfg = fused.PipeConfig(margins=(m, m, m, m), hsv_ranges=ranges)
        plan = fused.plan_pipe(src.shape[1:3], 1, (bg_side, bg_side), 1, cfg, params=params)
        if j == 0:
            ov_h, ov_w = plan.ov_dims[0]
            assert plan.cut_dims[0] == (side, side) and ov_h >= side and ov_w >= side   # not downscaled
            cut = opipe.cut_out(src[0], plan.params[0], cfg)[..., :3].reshape(-1, 3)
            packed = lambda c: (c[:, 0].astype(np.int64) << 16) | (c[:, 1].astype(np.int64) << 8) | c[:, 2]  # noqa: E731
            assert np.isin(packed(p), packed(cut)).all()           # the whole palette is in the cut-out
            _assert_separated(cut, runs, channel)
        assert int(plan.hsv["n_ranges"]) == 16
        runner = fused.PipeRunner(plan, DEV)
        runner.run(dev_src, dev_bgs, out)
        exp = opipe.pipe_item(src[0], bgs, plan.params[0], cfg)
        assert np.array_equal(out[0].cpu().numpy(), exp), j
        assert runner.status() == 0


# --------------------------------------------------------------------------- 4. dispatch variants

def variant_ranges(n):
    """n disjoint ranges (hue bands 11k .. 11k + 7), each holding about 3 % of
    uniformly random colours: a lost or shifted mask bit k changes pixels."""
    return [(11 * k, 40 + 3 * k, 60 + 2 * k, 11 * k + 7, 255 - 2 * k, 250 - k) for k in range(n)]


def variant_zones(n):
    """A different zone per range: negative margins (NumPy slice semantics)
    first, a single column (the 7th from the right) last, an empty one in the
    middle."""
    z = [((3 * k) % 17, (5 * k + 1) % 23, (7 * k + 2) % 19, (2 * k + 3) % 13) for k in range(n)]
    z[0] = (-40, 9, -25, 4)
    if n > 1:
        z[n - 1] = (0, 0, -7, 6)
    if n > 2:
        z[n // 2] = (400, 400, 0, 0)
    assert len(set(z)) == n
    return z


def _variant_sources(pool, ranges, n, H, W, seed):
    """Random colours, with the colours on every range's bounds planted as 2×2
    cells in the middle of each source (NEAREST rotation keeps such cells)."""
    rng = np.random.default_rng(seed)
    src = rng.integers(0, 256, (n, H, W, 3), np.uint8)
    cols = R.bound_colours(ranges, *pool)
    side = int(np.ceil(np.sqrt(len(cols))))
    cells = src[0, :side, :side].copy().reshape(-1, 3)
    cells[:len(cols)] = cols
    patch = np.repeat(np.repeat(cells.reshape(side, side, 3), 2, axis=0), 2, axis=1)
    assert 2 * side + 20 <= min(H, W)
    y0, x0 = (H - 2 * side) // 2, (W - 2 * side) // 2
    src[:, y0:y0 + 2 * side, x0:x0 + 2 * side] = patch
    # every range holds some of the colours fed, and no colour is in two ranges
    hsv = R.hsv_of_rgb(src.reshape(-1, 3))
    hits = np.stack([R.excluded(hsv, [f]) for f in ranges])
    assert hits.any(axis=1).all() and hits.sum(axis=0).max() == 1
    return src


def _assert_cut_out_coverage(pool, src, plan, cfg):
    """What the variant tests rely on, checked on the oracle's cut-outs: every
    planted bound colour survives the NEAREST rotation of every item, and over
    the items each range has in-range pixels outside its zone and, unless the
    zone is empty, inside it."""
    ranges, zones = cfg.hsv_ranges, cfg.zones
    cols = R.bound_colours(ranges, *pool).astype(np.int64)
    packed = lambda c: (c[..., 0] << 16) | (c[..., 1] << 8) | c[..., 2]  # noqa: E731
    held, left = np.zeros(len(ranges), bool), np.zeros(len(ranges), bool)
    empty = np.ones(len(ranges), bool)
    for i in range(len(src)):
        m = opipe.cut_out(src[i], plan.params[i], cfg)[..., :3]
        assert np.isin(packed(cols), packed(m.astype(np.int64))).all(), i
        if zones is None:
            continue
        h, w = m.shape[:2]
        hsv = R.hsv_of_rgb(m.reshape(-1, 3))
        for k, (f, z) in enumerate(zip(ranges, zones)):
            inr = R.excluded(hsv, [f]).reshape(h, w)
            r0, r1, c0, c1 = ops.zone_rows_cols(z, h, w)
            zm = np.zeros((h, w), bool)
            zm[r0:r1, c0:c1] = True
            empty[k] &= not zm.any()
            held[k] |= bool((inr & zm).any())
            left[k] |= bool((inr & ~zm).any())
    if zones is not None:
        assert left.all() and (held | empty).all()
        if len(ranges) > 2:
            assert empty.sum() == 1          # the empty zone is empty for every item, and the only one


PIPE_CASES = [(n, z) for n in (1, 2, 3, 4, 5, 6, 7, 16) for z in (False, True)]
PIPE_IDS = [f"{n}-{'zones' if z else 'plain'}" for n, z in PIPE_CASES]


@pytest.mark.parametrize("n_ranges,zoned", PIPE_CASES, ids=PIPE_IDS)
def test_pipe_variants(D, pool, n_ranges, zoned):
    """PipeRunner.run with 1-7 and 16 ranges (k_pipe_hpass2 NR = 1, 2, 3, 4, 6
    with one pad, 6, 16 padded, 16), with and without zones (the zoned forms
    run at 3 waves per SIMD; NR = 16 keeps its column bounds in LDS)."""
    from image_processor_pipeline_amd import fused
    ranges = variant_ranges(n_ranges)
    zones = variant_zones(n_ranges) if zoned else None
    n, H, W, K, bh, bw = 10, 150, 170, 3, 128, 160
    cfg = fused.PipeConfig(margins=(0.05, 9, 0.1, 3), hsv_ranges=ranges, zones=zones)
    src = _variant_sources(pool, ranges, n, H, W, seed=50 + n_ranges)
    bgs = np.random.default_rng(7).integers(0, 256, (K, bh, bw, 3), np.uint8)
    plan = fused.plan_pipe((H, W), n, (bh, bw), K, cfg, seed=60 + n_ranges)
    assert int(plan.hsv["n_ranges"]) == n_ranges
    _assert_cut_out_coverage(pool, src, plan, cfg)
    runner = fused.PipeRunner(plan, DEV)
    out = torch.empty((n, bh, bw, 3), dtype=torch.uint8, device=DEV)
    runner.run(_t(src), _t(bgs), out)
    got = out.cpu().numpy()
    for i in range(n):
        assert np.array_equal(got[i], opipe.pipe_item(src[i], bgs, plan.params[i], cfg)), i
    assert runner.status() == 0


CN4_CASES = [(n, z) for n in (1, 2, 3, 4, 6, 16) for z in (False, True)]
CN4_IDS = [f"{n}-{'zones' if z else 'plain'}" for n, z in CN4_CASES]


def _run_cn4(pool, n_ranges, zoned, pitch):
    """The 3-channel plan run with 4-channel sources through the C ABI (Python
    always passes src_cn = 3): the plan's descriptors with g.src_cn = 4, the
    row pitch `pitch` >= 4·W and the source offsets rescaled; an RGBX copy of
    the sources with random bytes in X and in the row padding.  The composites
    must equal the 3-channel run's and the oracle's.  Two crops: one that
    reaches the source's last pixel (zero bottom / right margins), one inside
    the source."""
    from image_processor_pipeline_amd import _native as N
    from image_processor_pipeline_amd import fused
    from image_processor_pipeline_amd.device import _stream, _to_dev
    ranges = variant_ranges(n_ranges)
    zones = variant_zones(n_ranges) if zoned else None
    n, H, W, K, bh, bw = 5, 70, 90, 2, 80, 96
    assert pitch >= 4 * W and pitch % 4 == 0
    lib = N.load()
    for margins in [(3, 0, 5, 0), (4, 6, 2, 7)]:
        cfg = fused.PipeConfig(margins=margins, scale_min=0.3, scale_max=0.7, hsv_ranges=ranges, zones=zones)
        src = _variant_sources(pool, ranges, n, H, W, seed=80 + n_ranges)
        bgs = np.random.default_rng(9).integers(0, 256, (K, bh, bw, 3), np.uint8)
        plan = fused.plan_pipe((H, W), n, (bh, bw), K, cfg, seed=21)
        _assert_cut_out_coverage(pool, src, plan, cfg)
        runner = fused.PipeRunner(plan, DEV)
        dev_bgs = _t(bgs)
        out3 = torch.empty((n, bh, bw, 3), dtype=torch.uint8, device=DEV)
        runner.run(_t(src), dev_bgs, out3)

        descs = plan.descs.copy()
        g = np.ascontiguousarray(descs["g"])
        assert (g["src_cn"] == 3).all() and (g["src_pitch"] == 3 * W).all() and (g["src_off"] % (3 * H * W) == 0).all()
        assert (g["src_h"] == H).all()
        g["src_off"] = g["src_off"] // (3 * H * W) * (H * pitch)
        g["src_cn"], g["src_pitch"] = 4, pitch
        N.check(lib.ipp_gather_prepare(N.np_ptr(g), n), "ipp_gather_prepare")
        descs["g"] = g
        # the last source byte a window's buffer records may cover lies inside the RGBX tensor
        assert int((g["src_off"] + g["src_h"].astype(np.int64) * g["src_pitch"]).max()) <= n * H * pitch
        r10 = np.random.default_rng(10)
        rows = r10.integers(0, 256, (n, H, pitch), np.uint8)                            # junk in the padding
        rows[:, :, :4 * W] = np.concatenate([src, r10.integers(0, 256, (n, H, W, 1), np.uint8)], -1).reshape(n, H, 4 * W)
        src4 = _t(rows)
        dev_descs = _to_dev(descs, runner.device)
        runner.tmp.fill_(0xA5)          # not the 3-channel run's (correct) intermediate
        out4 = torch.zeros((n, bh, bw, 3), dtype=torch.uint8, device=DEV)
        N.check(lib.ipp_pipe_hpass_bgcopy(src4.data_ptr(), runner.tmp.data_ptr(), runner.coefs.data_ptr(),
                                          dev_descs.data_ptr(), n, plan.max_out_w, plan.max_rows, 4,
                                          N.np_ptr(plan.hsv), plan.tap_format, dev_bgs.data_ptr(), out4.data_ptr(),
                                          _stream(runner.device)), "ipp_pipe_hpass_bgcopy")
        N.check(lib.ipp_pipe_vblend_bands(runner.tmp.data_ptr(), dev_bgs.data_ptr(), out4.data_ptr(),
                                          runner.coefs.data_ptr(), dev_descs.data_ptr(), n, plan.bg_w, plan.bg_h,
                                          plan.max_ov_w, plan.max_ov_h, plan.tap_format, _stream(runner.device)),
                "ipp_pipe_vblend_bands")
        assert runner.status() == 0
        assert torch.equal(out4, out3), margins
        got = out4.cpu().numpy()
        for i in range(n):
            assert np.array_equal(got[i], opipe.pipe_item(src[i], bgs, plan.params[i], cfg)), (margins, i)


@pytest.mark.parametrize("n_ranges,zoned", CN4_CASES, ids=CN4_IDS)
def test_pipe_cn4(D, pool, n_ranges, zoned):
    """k_pipe_hpass2<NR, ZONES, 4>, tight rows (pitch 4·W): the fast body,
    also for the crop that reaches the source's last pixel (a dword there
    fits; the 3-channel run of the same crop takes CLAMP)."""
    _run_cn4(pool, n_ranges, zoned, 4 * 90)


# hpass_block takes the fast body only if yr_range_ok: 32768 * pitch + need <= 2^32
# (no row offset may wrap into the window).  2^15 * 2^17 = 2^32 and need > 0.
CLAMP_PITCH = 1 << 17


@pytest.mark.parametrize("n_ranges,zoned", [(4, False), (6, True), (16, True)], ids=["4-plain", "6-zones", "16-zones"])
def test_pipe_cn4_padded_pitch(D, pool, n_ranges, zoned):
    """hpass2_body<NR, ZONES, 4, CLAMP>: 4-channel sources whose rows are
    padded to 131072 bytes (9 MB per 70-row item), junk in the padding.  Every
    block then takes the general body: column and row tested per pixel,
    records to the image end."""
    assert 32768 * CLAMP_PITCH + 1 > 1 << 32
    _run_cn4(pool, n_ranges, zoned, CLAMP_PITCH)


def _decisive_frame(pool, ranges, h, w):
    """A BGR frame in which range 1's zone alone decides the largest
    component.  On a background that range 0 excludes: blob A (30×30 = 900, in
    no range) and blob B (40×40 = 1600, a colour range 1 holds) across the
    tile corner (64, 64).  Range 1's zone is the columns [75, 80): it leaves of
    B a piece of 40×30 = 1200 (the largest) and one of 40×5.  A zone taken for
    the whole frame would leave A the largest, a zone taken for empty all of
    B."""
    rgb, hsv = pool
    in0, in1 = R.excluded(hsv, [ranges[0]]), R.excluded(hsv, [ranges[1]])
    free = ~R.excluded(hsv, ranges)
    fr = np.empty((h, w, 3), np.uint8)
    fr[:] = rgb[np.flatnonzero(in0)[0]][::-1]
    fr[5:35, 120:150] = rgb[np.flatnonzero(free)[0]][::-1]
    fr[50:90, 45:85] = rgb[np.flatnonzero(in1)[0]][::-1]
    return fr, (0, 0, 75, w - 80)


def _plant_bounds(pool, fr, ranges, zones, gimp, rng):
    """The BGR frame with the colours on every range's bounds (of the rescaled
    range under the GIMP scale) planted at random pixels, 8 of each: 4 inside
    and 4 outside the range's zone where the zone is a proper part of the
    frame."""
    h, w = fr.shape[:2]
    flat = fr.reshape(-1, 3)
    used = np.zeros(h * w, bool)
    for k, f in enumerate(ranges):
        cols = R.bound_colours([ops.rescale_filter(f, gimp)], *pool)
        zm = np.zeros((h, w), bool)
        r0, r1, c0, c1 = ops.zone_rows_cols(zones[k] if zones else None, h, w)
        zm[r0:r1, c0:c1] = True
        zm = zm.ravel()
        groups = [zm, ~zm] if zm.any() and not zm.all() else [np.ones(h * w, bool)]
        for g in groups:
            p = rng.choice(np.flatnonzero(g & ~used), (8 // len(groups), len(cols)), replace=False)
            flat[p] = cols[None, :, ::-1]
            used[p] = True
    return fr


VIDEO_CASES = [(4, True, False), (16, False, False), (16, True, False), (4, True, True)]
VIDEO_IDS = ["4-zones", "16-plain", "16-zones", "gimp"]


@pytest.mark.parametrize("n_ranges,zoned,gimp", VIDEO_CASES, ids=VIDEO_IDS)
def test_video_variants(D, pool, n_ranges, zoned, gimp):
    """VideoChain with its ranges, zones and use_gimp_scale arguments
    (k_ccl_label<SRC_HSV, 4 | 16, zones | none>), `run` and `run_staged`, on
    frames off the 64-pixel tile grid: random colours plus the colours on
    every range's bounds, planted inside and outside the zones; the zones cut
    through tiles and through the loader's 4-pixel quads.  The zoned 4-range
    form is the only user of hsv_tab_excl<4, true>."""
    from image_processor_pipeline_amd.video_chain import VideoChain
    if gimp:   # GIMP scale: H 0..360, S and V 0..100
        ranges = [(30, 20, 30, 90, 80, 90), (300, 10, 10, 360, 100, 60), (100, 4, 6, 200, 100, 100),
                  (0, 0, 0, 360, 100, 25)]
    else:
        ranges = variant_ranges(n_ranges)
    rng = np.random.default_rng(100 + n_ranges)
    for (h, w) in [(90, 120), (130, 200)]:
        zones = None
        if zoned:
            zones = [((5 * k + 2) % 31, (7 * k + 3) % 37, (9 * k + 1) % 43, (11 * k + 5) % 41) for k in range(len(ranges))]
            zones[0] = (0, 0, 0, 0)
            zones[-1] = (-50, 7, -70, 13)
        frames = [_plant_bounds(pool, rng.integers(0, 256, (h, w, 3), np.uint8), ranges, zones, gimp, rng)
                  for _ in range(2)]
        if zoned and not gimp and (h, w) == (130, 200):
            fr, zones[1] = _decisive_frame(pool, ranges, h, w)
            frames.append(fr)
            exp = ops.keep_largest_component(ops.color_mask_bgra(fr, ranges, zones))
            assert exp.shape[:2] == (40, 30)       # the piece of B left of the zone
        frames = np.stack(frames)
        n = len(frames)
        chain = VideoChain(n, h, w, DEV, ranges, zones, gimp)
        assert int(chain.hsv["n_ranges"]) == len(ranges)
        dev_fr = _t(frames)
        exp = [ops.keep_largest_component(ops.color_mask_bgra(frames[i], ranges, zones, gimp)) for i in range(n)]
        chain.run(dev_fr)
        fused_res = chain.results()
        chain.out.fill_(0x5A)           # not the fused run's (correct) crops and boxes
        chain.bbox.fill_(-1)
        chain.run_staged(dev_fr)
        staged_res = chain.results()
        for i in range(n):
            assert fused_res[i] is not None and np.array_equal(fused_res[i], exp[i]), ("run", h, w, i)
            assert staged_res[i] is not None and np.array_equal(staged_res[i], exp[i]), ("run_staged", h, w, i)
