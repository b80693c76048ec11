"""CPU: ``oracle/ops.py`` against live Pillow on every case of
tests/plugin_refs.py — the expectations test_gpu_plugin_kernels.py holds the
plugin-path kernels to — and the properties the case tables claim (tile edges,
row phases, corners, zone sizes), so a table edited later cannot lose them
silently.  For the rotate / flip gather it also holds plan_rotate_flip and
ipp_gather_prepare to the oracle through ``plugin_refs.gather_model``, which
asserts the bounds of every load ipp_rotate_flip_nearest would make.  For the
bilinear launches ``ops.affine_bilinear`` is held to ``Image.transform`` and,
where the arithmetic is exact, to an evaluation over the rationals.
"""
import numpy as np
import pytest
from PIL import Image, ImageEnhance, ImageFilter

from oracle import ops
from tests import plugin_refs as R

LANCZOS = Image.Resampling.LANCZOS
BILINEAR = Image.Resampling.BILINEAR


def _pil_resize(img, w, h):
    return np.asarray(Image.fromarray(img).resize((w, h), LANCZOS))


def _pil_paste(bg, ov, x, y):
    out = Image.fromarray(bg).copy()
    o = Image.fromarray(ov)
    out.paste(o, (x, y), o)
    return np.asarray(out)


# --------------------------------------------------------------------------- LANCZOS

@pytest.mark.parametrize("k", range(len(R.LANCZOS_CASES)))
def test_resize_oracle_equals_pillow(k):
    _, _, ow, oh, _ = R.LANCZOS_CASES[k]
    img = R.lanczos_image(k)
    assert np.array_equal(ops.resize_lanczos_rgba(img, ow, oh), _pil_resize(img, ow, oh)), R.LANCZOS_CASES[k]


def test_lanczos_table_visits_the_block_edges():
    cases = [c[:4] for c in R.LANCZOS_CASES]
    two_axis = [c for c in cases if c[0] != c[2] and c[1] != c[3]]
    assert {63, 64, 65} <= {c[2] for c in cases} and {63, 64, 65} <= {c[3] for c in cases}
    assert {3, 4, 5} <= {R.lanczos_lines(c[1], c[3]) for c in two_axis}
    assert any(c[0] == c[2] for c in cases) and any(c[1] == c[3] for c in cases)       # one-axis forms
    assert any(c[:2] == (1, 1) for c in cases) and any(c[2:] == (1, 1) for c in cases)
    assert any(c[2] == 8 * c[0] for c in cases) and any(c[0] == 30 * c[2] for c in cases)
    modes = {c[4] for c in R.LANCZOS_CASES}
    assert {"palette", "white", "transparent", "opaque"} <= modes
    for k, c in enumerate(R.LANCZOS_CASES):
        if c[4] in ("palette", "white"):
            img = R.lanczos_image(k)
            if img.shape[0] * img.shape[1] >= 60:
                assert set(R.ALPHA_PALETTE) <= set(np.unique(img[..., 3])), c
                assert (img[..., :3] == 255).any()


def test_lanczos_taps_stay_below_the_24_bit_multiplier_bound():
    """k_lanczos_h/v multiply with v_mul_i32_i24: |tap| < 2^23.  A 1-pixel
    input gives the largest tap there is, exactly 2^22."""
    worst = 0
    for in_w, in_h, ow, oh, _ in R.LANCZOS_CASES:
        for n_in, n_out in ((in_w, ow), (in_h, oh)):
            _, _, kk = ops.precompute_coeffs(n_in, 0.0, float(n_in), n_out)
            worst = max(worst, int(np.abs(kk).max()))
    assert 1 << 22 <= worst < 1 << 23


def test_whole_image_resize_reads_every_row():
    """Resample.c's ybox_first / ybox_last of a resize without a ``box``: the
    first output's support always reaches row 0 and the last one's the last
    row (centre ± 3·max(scale, 1) around 0.5·scale), so the H pass makes all
    in_h lines and the descriptors' ``line0`` is 0 for every size.  No call of
    ``resize_lanczos_rgba`` or ``batch_ops.overlays`` can feed the kernels
    another ``line0``."""
    sizes = sorted(set(range(1, 41)) | {63, 64, 65, 97, 330})
    for n_in in sizes:
        for n_out in sizes:
            _, b, _ = ops.precompute_coeffs(n_in, 0.0, float(n_in), n_out)
            assert b[0, 0] == 0 and b[-1, 0] + b[-1, 1] == n_in, (n_in, n_out)


# --------------------------------------------------------------------------- overlays / paste

@pytest.mark.parametrize("k", range(len(R.OVERLAY_ITEMS)))
def test_overlay_item_oracle_equals_pillow(k):
    ovs, bgs, sizes, pos = R.overlay_inputs()
    rs = ops.resize_lanczos_rgba(ovs[k], *sizes[k])
    assert np.array_equal(rs, _pil_resize(ovs[k], *sizes[k])), R.OVERLAY_ITEMS[k]
    assert np.array_equal(ops.paste_rgba_onto_rgb(bgs[k], rs, *pos[k]), _pil_paste(bgs[k], rs, *pos[k])), \
        R.OVERLAY_ITEMS[k]


def test_overlay_table_properties():
    items = R.OVERLAY_ITEMS
    assert len(items) >= 8
    assert {5, 6, 16, 21, 341, 342} == {it[4] for it in items}
    assert len({it[5] for it in items}) >= 6                                  # differing heights
    two_axis = [it for it in items if it[0] != it[2] and it[1] != it[3]]
    one_axis = [k for k, it in enumerate(items) if (it[0] != it[2]) != (it[1] != it[3])]
    assert one_axis and 0 < one_axis[0] < len(items) - 1                      # per-image branch mid-list
    assert len({3 * it[6] % 16 for it in two_axis}) >= 8                      # phases of the first blended byte
    for it in items:                                                          # inside the background
        assert 0 <= it[6] and it[6] + it[2] <= it[4] and 0 <= it[7] and it[7] + it[3] <= it[5], it
    corner = lambda it: (it[6] == 0, it[7] == 0, it[6] + it[2] == it[4], it[7] + it[3] == it[5])   # noqa: E731
    flags = [corner(it) for it in two_axis]
    assert any(l and t for l, t, r, b in flags) and any(r and t for l, t, r, b in flags)
    assert any(l and b for l, t, r, b in flags) and any(r and b for l, t, r, b in flags)
    shapes = {it[:4] for it in items}
    assert (3, 2, 1, 1) in shapes and (8, 6, 64, 48) in shapes and (330, 7, 11, 5) in shapes
    # with and without a box; every threshold leaves some item with a box and
    # 255 leaves some without
    assert R.OVERLAY_ALPHA_MINS[0] is None and set(R.OVERLAY_ALPHA_MINS[1:]) == {1, 128, 255}
    ovs, _, sizes, _ = R.overlay_inputs()
    for amin in R.OVERLAY_ALPHA_MINS[1:]:
        boxes = [R.bbox_alpha_min(ops.resize_lanczos_rgba(o, *s), amin) for o, s in zip(ovs, sizes)]
        assert any(b is not None for b in boxes) and any(b is None for b in boxes), amin
        assert len(set(boxes)) > 3


@pytest.mark.parametrize("k", range(len(R.PASTE_PITCH_CASES)))
def test_paste_oracle_equals_pillow(k):
    bw, bh, ow, oh, x, y, bp, dp = R.PASTE_PITCH_CASES[k]
    assert bp > 3 * bw and dp > 3 * bw and x + ow <= bw and y + oh <= bh
    bg, ov = R.paste_inputs(k)
    assert np.array_equal(ops.paste_rgba_onto_rgb(bg, ov, x, y), _pil_paste(bg, ov, x, y))


def test_paste_table_properties():
    c = R.PASTE_PITCH_CASES
    assert any(it[2:4] == (1, 1) and it[4] == it[0] - 1 and it[5] == it[1] - 1 for it in c)    # last pixel
    assert any(it[2:4] == it[0:2] for it in c)                                                  # whole cover
    assert any(it[6] % 16 == 0 and it[7] % 16 == 0 for it in c) and any(it[6] % 16 for it in c)


# --------------------------------------------------------------------------- windows

def test_copy_table_properties():
    imgs = R.copy_images()
    assert len(R.COPY_JOBS) >= 24
    cn = lambda i: 1 if imgs[i].ndim == 2 else imgs[i].shape[2]   # noqa: E731
    assert {1, 3, 4} == {cn(i) for i, _, _ in R.COPY_JOBS}
    assert any(im.ndim == 2 for im in imgs) and any(im.ndim == 3 for im in imgs)
    assert {0, 1, 2, 3} == {f for _, _, f in R.COPY_JOBS}
    assert {15, 16, 17, 1023, 1024, 1025} <= {w[2] * cn(i) for i, w, _ in R.COPY_JOBS}
    per_image = np.bincount([i for i, _, _ in R.COPY_JOBS])
    assert (per_image >= 2).all()                                  # several jobs read one image
    full = last_row = last_col = one = False
    for i, (x0, y0, w, h), _ in R.COPY_JOBS:
        ih, iw = imgs[i].shape[:2]
        assert 0 <= x0 and x0 + w <= iw and 0 <= y0 and y0 + h <= ih and w > 0 and h > 0
        full |= (w, h) == (iw, ih)
        one |= (w, h) == (1, 1) and (iw, ih) != (1, 1)
        last_row |= h == 1 and y0 == ih - 1 and w == iw and ih > 1
        last_col |= w == 1 and x0 == iw - 1 and h == ih and iw > 1
    assert full and one and last_row and last_col


@pytest.mark.parametrize("flip", [0, 1, 2, 3])
def test_window_ref_equals_pillow_transpose(flip):
    img = R.copy_images()[4]
    win = (3, 1, 5, 4)
    exp = Image.fromarray(img).crop((3, 1, 8, 5))
    if flip & 1:
        exp = exp.transpose(Image.Transpose.FLIP_LEFT_RIGHT)
    if flip & 2:
        exp = exp.transpose(Image.Transpose.FLIP_TOP_BOTTOM)
    assert np.array_equal(R.window_ref(img, win, flip), np.asarray(exp))


# --------------------------------------------------------------------------- HSV zones

def test_hsv_table_zones_depend_on_each_images_own_size():
    """The zones must tell an image's own size from the batch's largest: for
    every set some image's zone rectangle differs from the one the largest
    size would give, and the sets hold negative margins, a zone empty for every
    image and one larger than the smallest image."""
    dims = [(h, w) for w, h, _ in R.HSV_IMAGES]
    assert len(dims) >= 6 and (1, 1) in dims and {3, 4} == {cn for _, _, cn in R.HSV_IMAGES}
    mh, mw = max(d[0] for d in dims), max(d[1] for d in dims)
    negative = empty = oversize = False
    for ranges, zones, _ in R.HSV_SETS:
        assert len(ranges) == len(zones)
        differs = False
        for z in zones:
            if z is None:
                continue
            negative |= min(z) < 0
            rects = [ops.zone_rows_cols(z, h, w) for h, w in dims]
            areas = [(r1 - r0) * (c1 - c0) for r0, r1, c0, c1 in rects]
            empty |= max(areas) == 0
            oversize |= min(z) >= 0 and areas[dims.index((1, 1))] == 0 and max(areas) > 0
            r0, r1, c0, c1 = ops.zone_rows_cols(z, mh, mw)
            for (h, w), own in zip(dims, rects):
                shared = (min(r0, h), min(r1, h), min(c0, w), min(c1, w))
                differs |= own != shared and (own[1] - own[0]) * (own[3] - own[2]) > 0
        assert differs
    assert negative and empty and oversize


def test_hsv_table_masks_are_mixed():
    for ranges, zones, gimp in R.HSV_SETS:
        alphas = [ops.hsv_alpha_mask(im[..., :3], ranges, zones, gimp) for im in R.hsv_images()]
        assert sum(1 for a in alphas if (a == 0).any() and (a == 255).any()) >= 4


# --------------------------------------------------------------------------- alpha boxes

def _pil_bbox(img):
    im = Image.fromarray(img[..., 0] if img.shape[2] == 1 else img)
    assert im.mode == {1: "L", 2: "LA", 3: "RGB", 4: "RGBA"}[img.shape[2]]
    return im.getbbox()


def test_getbbox_oracle_equals_pillow():
    imgs = R.bbox_images()
    assert {1, 2, 3, 4} == {im.shape[2] for im in imgs}
    got = [ops.getbbox_alpha(im) for im in imgs]
    assert got == [_pil_bbox(im) for im in imgs]
    assert got[0] is None and sum(b is not None for b in got) == len(imgs) - 1
    # a box at each corner of its image, and sizes off the 64×16 tile
    assert any(b and b[:2] == (0, 0) and b[2:] == (1, 1) for b in got)
    for im, b in zip(imgs[1:6], got[1:6]):
        assert b[2] - b[0] == 1 and b[3] - b[1] == 1
        assert b[0] in (0, im.shape[1] - 1) and b[1] in (0, im.shape[0] - 1)
    assert any(im.shape[1] % 64 and im.shape[0] % 16 for im in imgs)


def test_bbox_alpha_min_helper():
    """alpha_min = 1 is Pillow's getbbox of an alpha image; a higher threshold
    is getbbox of the alpha band with the values below it cleared."""
    imgs = R.bbox_images(channels=(2, 4))
    assert {2, 4} == {im.shape[2] for im in imgs}
    for amin in R.BBOX_ALPHA_MINS:
        boxes = [R.bbox_alpha_min(im, amin) for im in imgs]
        for im, b in zip(imgs, boxes):
            a = im[..., -1]
            assert b == Image.fromarray(np.where(a >= amin, a, 0).astype(np.uint8)).getbbox()
        if amin == 1:
            assert boxes == [ops.getbbox_alpha(im) for im in imgs]
    assert [R.bbox_alpha_min(im, 1) for im in imgs] != [R.bbox_alpha_min(im, 255) for im in imgs]


# --------------------------------------------------------------------------- enhance

def _enhance_items():
    return R.enhance_ragged() + R.enhance_factor_sweep() + R.enhance_constant_images()


def test_enhance_oracle_equals_pillow_step_by_step():
    """Every item of the three enhance tables: each ops stage against the
    Pillow call it restates, fed the same input."""
    luts = R.enhance_luts()
    for n, (img, (fb, fc, fcol), radius, lut) in enumerate(_enhance_items()):
        tag = (n, img.shape, fb, fc, fcol, radius, lut)
        cur = img
        for op, enh, f in ((ops.enhance_brightness, ImageEnhance.Brightness, fb),
                           (ops.enhance_contrast, ImageEnhance.Contrast, fc),
                           (ops.enhance_color, ImageEnhance.Color, fcol)):
            nxt = op(cur, f)
            assert np.array_equal(nxt, np.asarray(enh(Image.fromarray(cur)).enhance(f))), (tag, enh.__name__)
            cur = nxt
        if radius is not None:
            nxt = ops.gaussian_blur(cur, radius)
            pil = Image.fromarray(cur).filter(ImageFilter.GaussianBlur(radius))
            assert np.array_equal(nxt, np.asarray(pil)), (tag, "GaussianBlur")
            cur = nxt
        if lut:
            bands = [b.point(list(luts[c])) for c, b in enumerate(Image.fromarray(cur).split())]
            cur = np.asarray(Image.merge("RGB", bands))
        assert np.array_equal(R.enhance_ref(img, (fb, fc, fcol), radius, luts if lut else None), cur), tag


def test_enhance_table_properties():
    from image_processor_pipeline_amd import geometry as G
    items = R.enhance_ragged()
    shapes = {(it[0].shape[1], it[0].shape[0]) for it in items}
    assert shapes == set(R.ENHANCE_SHAPES)
    assert {256, 257, 1024, 1025} <= {w * h for w, h in shapes}
    assert {(r is not None, lut) for _, _, r, lut in items} == {(a, b) for a in (True, False) for b in (True, False)}
    box_r = {r: G.gaussian_box(r)[0] for r in R.ENHANCE_RADII}
    assert set(box_r.values()) >= {1, 2} and 2 * max(box_r.values()) + 2 == R.ENHANCE_NARROW
    for w, h in R.ENHANCE_SHAPES:                       # narrow shapes meet every radius
        if min(w, h) < R.ENHANCE_NARROW:
            assert {it[2] for it in items if it[0].shape[:2] == (h, w)} >= set(R.ENHANCE_RADII)
    sweep = R.enhance_factor_sweep()
    for pos in range(3):
        assert {it[1][pos] for it in sweep} >= set(R.ENHANCE_FACTORS)
    assert np.float32(R.ENHANCE_FACTORS[2]) < np.float32(1) and np.float32(R.ENHANCE_FACTORS[2]) == R.ENHANCE_FACTORS[2]
    greys = R.enhance_constant_images()[4]
    lum = ops.rgb_to_l(greys[0])
    assert lum.sum() / lum.size == 10.5 and (ops.enhance_contrast(greys[0], 0.5) == [[[10], [11]]]).all()


@pytest.mark.parametrize("radius", R.ENHANCE_RADII + (0.5,))
def test_blur_oracle_equals_pillow_on_narrow_shapes(radius):
    for k, (w, h) in enumerate(R.ENHANCE_SHAPES + [(2, 2), (2, 9), (6, 3), (64, 65)]):
        img = R.rgb_image(R.ENHANCE_SEED + 300 + k, w, h)
        pil = Image.fromarray(img).filter(ImageFilter.GaussianBlur(radius))
        assert np.array_equal(ops.gaussian_blur(img, radius), np.asarray(pil)), (w, h, radius)


# --------------------------------------------------------------------------- bilinear rotate

@pytest.mark.parametrize("k", range(len(R.ROTATE_SHAPES)))
def test_rotate_bilinear_oracle_equals_pillow(k):
    img = R.rotate_image(k)
    assert img.size < 28 or {1, 2, 127, 128, 254} & set(np.unique(img[..., 3]))     # partial α
    for a in R.ROTATE_ANGLES:
        rot = Image.fromarray(img).rotate(a, expand=True, resample=BILINEAR)
        bb = rot.getbbox()
        exp = rot
        if bb is not None and bb[2] > bb[0] and bb[3] > bb[1]:
            exp = rot.crop(bb)
        got = ops.rotate_and_crop(img, a, "bilinear")
        assert got.shape == np.asarray(exp).shape, (R.ROTATE_SHAPES[k], a)
        assert np.array_equal(got, np.asarray(exp)), (R.ROTATE_SHAPES[k], a)
    assert {0.0, 90.0, 180.0, 270.0} <= set(R.ROTATE_ANGLES) and len(R.ROTATE_ANGLES) >= 7


# --------------------------------------------------------------------------- bilinear through the C ABI

def _pil_affine(win, m, ow, oh, flip):
    """Image.transform(AFFINE, BILINEAR) of a window (an RGB one through
    convert('RGBA')), flipped with NumPy.  A window without pixels is made
    with Image.new (no array interface for it)."""
    h, w, cn = win.shape
    im = Image.fromarray(win) if w and h else Image.new("RGB" if cn == 3 else "RGBA", (w, h))
    if win.shape[2] == 3:
        im = im.convert("RGBA")
    return R.flip_ref(np.asarray(im.transform((ow, oh), Image.Transform.AFFINE, m, BILINEAR)), flip)


def _empty(launch, j):
    oh, ow = launch.shapes[j]
    return 0 in launch.wins[j].shape[:2] or ow == 0 or oh == 0


@pytest.fixture(scope="module")
def bilinear_listed():
    launch = R.bilinear_launch()
    return launch, R.bilinear_refs(launch)


def test_affine_bilinear_oracle_equals_pillow(bilinear_listed):
    launch, refs = bilinear_listed
    assert len(refs) == len(R.BILINEAR_ITEMS) >= 30
    for j, (it, win, m, (oh, ow), ref) in enumerate(zip(launch.items, launch.wins, launch.mats, launch.shapes, refs)):
        assert ref.shape == (oh, ow, 4) and ref.dtype == np.uint8, it
        if _empty(launch, j):
            assert not ref.any(), it
        pil = _pil_affine(win, m, ow, oh, it[6])
        assert pil.shape == ref.shape and np.array_equal(ref, pil), (j, it)


@pytest.mark.parametrize("k", range(len(R.BILINEAR_ALPHA_MATRICES)))
def test_affine_bilinear_alpha_square_equals_pillow(k):
    launch = R.bilinear_alpha_launch(k)
    sq = R.alpha_colour_square()
    assert np.array_equal(launch.flat.reshape(256, 256, 4), sq) and launch.descs[0]["src_pitch"] == 1024
    ref = R.bilinear_refs(launch)[0]
    assert np.array_equal(ref, _pil_affine(sq, launch.mats[0], 256, 256, 0))
    if k == 0:
        rt = ops.unpremultiply(ops.premultiply(sq))
        assert np.array_equal(ref, rt) and (rt != sq).any()          # the round trip is lossy, and kept
    else:
        # neighbours are mixed: the canvas differs from the round trip of the
        # shifted square in partial α, and the rejected last line is zero
        assert (ref[:, -1] == 0).all() if k == 1 else (ref[-1] == 0).all()
        moved = sq[:, 1:] if k == 1 else sq[1:]
        part = ref[:, :-1] if k == 1 else ref[:-1]
        assert (part != ops.unpremultiply(ops.premultiply(moved))).any()


def _fraction_bilinear(img, m, ow, oh):
    """Geometry.c's bilinear formula over the rationals for an OPAQUE RGBA
    array (premultiply and unpremultiply are the identity at α = 255)."""
    from fractions import Fraction as F
    assert (img[..., 3] == 255).all()
    h, w = img.shape[:2]
    m = [F(v) for v in m]
    half = F(1, 2)
    out = np.zeros((oh, ow, 4), np.uint8)
    for y in range(oh):
        for x in range(ow):
            X, Y = x + half, y + half
            xin, yin = m[0] * X + m[1] * Y + m[2], m[3] * X + m[4] * Y + m[5]
            if not (0 <= xin < w and 0 <= yin < h):
                continue
            xs, ys = xin - half, yin - half
            xi, yi = xs.numerator // xs.denominator, ys.numerator // ys.denominator      # floor
            dx, dy = xs - xi, ys - yi
            x0, x1 = min(max(xi, 0), w - 1), min(max(xi + 1, 0), w - 1)
            y0 = min(max(yi, 0), h - 1)
            for c in range(4):
                a, b = int(img[y0, x0, c]), int(img[y0, x1, c])
                v1 = a + (b - a) * dx
                v2 = v1
                if 0 <= yi + 1 < h:
                    a, b = int(img[yi + 1, x0, c]), int(img[yi + 1, x1, c])
                    v2 = a + (b - a) * dx
                v = v1 + (v2 - v1) * dy
                out[y, x, c] = v.numerator // v.denominator                             # v >= 0: truncation
    return out


def test_affine_bilinear_oracle_equals_exact_rationals(bilinear_listed):
    """The `exact` items: dyadic matrices on opaque colours that are multiples
    of 4, where no double operation of the lerps rounds.  Many results are
    integers, which a last-bit error below would truncate to the byte before."""
    from fractions import Fraction as F
    launch, refs = bilinear_listed
    seen = on_integer = 0
    for it, win, m, (oh, ow), ref in zip(launch.items, launch.wins, launch.mats, launch.shapes, refs):
        if not it[9]:
            continue
        seen += 1
        assert all(F(v).denominator in (1, 2, 4) for v in m), it
        rgba = ops.to_rgba(win)
        assert (rgba[..., 3] == 255).all() and (rgba[..., :3] % 4 == 0).all(), it
        exact = _fraction_bilinear(rgba, m, ow, oh)
        assert np.array_equal(R.flip_ref(exact, it[6]), ref), it
        s = ops.affine_bilinear_samples(m, win.shape[1], win.shape[0], ow, oh)
        on_integer += int((s["ok"] & ((s["dx"] * 4) % 1 == 0) & (s["dx"] > 0) & (s["dy"] == 0)).sum())
    assert seen >= 10 and on_integer > 0
    shifts = {(m[2], m[5]) for it, m in zip(launch.items, launch.mats) if it[9] and m[:2] + m[3:5] == (1, 0, 0, 1)}
    assert {0.25, 0.5, 0.75} <= {s[0] for s in shifts} and {0.25, 0.5, 0.75} <= {s[1] for s in shifts}


def test_bilinear_table_claims(bilinear_listed):
    """What section 8b of plugin_refs.py says of its table, from the
    reference's own index arrays."""
    launch, refs = bilinear_listed
    items, n = launch.items, len(launch.items)
    sizes = [(ow, oh) for oh, ow in launch.shapes]
    assert all(max(it[0], it[1], ow, oh) <= 256 for it, (ow, oh) in zip(items, sizes))
    # the out sizes on the 64 × 4 tile's edges; widest and tallest are two items, each alone
    assert set(R.BILINEAR_WIDTHS) <= {s[0] for s in sizes} and set(R.BILINEAR_HEIGHTS) <= {s[1] for s in sizes}
    assert {0, 1, 63} <= {s[0] % R.BILINEAR_TILE_W for s in sizes}
    assert {0, 1, 3} <= {s[1] % R.BILINEAR_TILE_H for s in sizes if s[1]}
    assert [k for k, s in enumerate(sizes) if s[0] == launch.max_w] == [R.BILINEAR_WIDEST]
    assert [k for k, s in enumerate(sizes) if s[1] == launch.max_h] == [R.BILINEAR_TALLEST]
    assert -(-launch.max_w // R.BILINEAR_TILE_W) == 3 and -(-launch.max_h // R.BILINEAR_TILE_H) >= 3
    # empty items: one writes nothing, one writes zeros
    assert sum(s[1] == 0 for s in sizes) == 1
    zero_w = [j for j, it in enumerate(items) if R.bilinear_window(it)[2] == 0]
    assert len(zero_w) == 1 and sizes[zero_w[0]][0] > 0 and sizes[zero_w[0]][1] > 0 and not refs[zero_w[0]].any()
    # what the samples visit
    seen, both = set(), []
    for j, it in enumerate(items):
        if _empty(launch, j):
            continue
        s = R.bilinear_samples(launch, j)
        ok, xi, yi = s["ok"], s["xi"], s["yi"]
        _, _, ww, wh = R.bilinear_window(it)
        if (ok & (yi == -1)).any() and (ok & (yi + 1 == wh)).any():
            both.append(j)
        seen |= {name for name, hit in (
            ("xi=-1", ok & (xi == -1)), ("yi=-1", ok & (yi == -1)), ("yi+1=in_h", ok & (yi + 1 == wh)),
            ("xi+1=in_w", ok & (xi + 1 == ww)), ("xin=0.0", ok & (s["xin"] == 0.0)),
            ("xin=in_w", ~ok & (s["xin"] == ww) & (s["yin"] >= 0) & (s["yin"] < wh)),
            ("ulp inside", ok & (s["xin"] == np.nextafter(float(ww), 0.0))),
            ("all rejected", np.array(not ok.any())), ("all accepted", np.array(ok.all())),
            ("some rejected", np.array(ok.any() and not ok.all()))) if hit.any()}
        if not ok.any():
            assert j == n - 1 and not refs[j].any()          # its source ends the buffer and is never read
    assert seen == {"xi=-1", "yi=-1", "yi+1=in_h", "xi+1=in_w", "xin=0.0", "xin=in_w", "ulp inside", "all rejected",
                    "all accepted", "some rejected"}
    assert both                                             # first rows at yi = -1 and last rows at yi + 1 = in_h
    # matrices
    mats = launch.mats
    assert sum(m == R.BILINEAR_I for m in mats) >= 3
    assert any(m[0] == -1.0 for m in mats) and any(m[0] == 2.0 == m[4] for m in mats)
    assert any(m[0] == 0.25 == m[4] for m in mats) and any(m[1] != 0 and m[3] == 0 and m[0] == 1 for m in mats)
    assert any(m[0] == m[1] == m[3] == m[4] == 0.0 for m in mats)
    rots = sorted(it[4][1] for it in items if it[4][0] == "rot")
    assert rots == sorted(R.BILINEAR_ANGLES)
    for it, m, (ow, oh) in zip(items, mats, sizes):
        if it[4][0] == "rot":
            _, _, ww, wh = R.bilinear_window(it)
            g = ops.rotate_geometry(ww, wh, it[4][1])
            assert m == g["matrix"] and (ow, oh) == (g["nw"], g["nh"]), it
    # flips on odd and on even sizes, both channel counts
    for bit, axis in ((1, 0), (2, 1)):
        assert {s[axis] % 2 for it, s in zip(items, sizes) if it[6] & bit and s[0] and s[1]} == {0, 1}
    assert {it[6] for it in items} == {0, 1, 2, 3}
    assert {(it[2], it[6]) for it in items} == {(cn, f) for cn in (3, 4) for f in range(4)}
    # pitches and offsets
    assert {1, 5, 13} <= {it[7] for it in items} and {4, 60} == {it[8] for it in items if it[8]}
    d = launch.descs
    assert any(int(o) % 4 for o in d["src_off"]) and any(int(o) % 2 for o in d["src_off"])
    assert (d["dst_off"] % 4 == 0).all() and (d["dst_pitch"] % 4 == 0).all()
    assert (d["dst_off"] % 16 != 0).sum() >= n // 2 and int(d["dst_off"][0]) == 4
    assert (launch.flat == R.BILINEAR_SRC_JUNK).sum() >= sum(it[7] * it[1] for it in items)
    ends = d["dst_off"] + d["dst_pitch"].astype(np.int64) * d["out_h"]
    assert (d["dst_off"][1:] >= ends[:-1] + 4).all() and int(ends[-1]) == launch.total_bytes
    last = items[-1]
    assert int(d["src_off"][-1]) + last[0] * last[1] * last[2] == launch.flat.size
    assert last[0] * last[1] * last[2] >= int(d["src_pitch"].max())     # a row past any other source stays inside
    # the three orders
    orders = [R.bilinear_order(o) for o in R.BILINEAR_ORDERS]
    assert all(sorted(o) == list(range(n)) for o in orders) and len({tuple(o) for o in orders}) == 3
    assert orders[1] == orders[0][::-1] and orders[2][0] == R.BILINEAR_WIDEST != orders[0][0]
    for name in R.BILINEAR_ORDERS[1:]:
        other = R.bilinear_launch(name)
        assert np.array_equal(other.flat, launch.flat)
        for j, k in enumerate(other.index):
            assert np.array_equal(other.wins[j], launch.wins[k]) and other.descs[j]["src_off"] == d[k]["src_off"]


def test_bilinear_windows_tell_the_window_from_the_image(bilinear_listed):
    """Every windowed item has samples with a neighbour outside the window and
    inside the image, at a weight above zero, where the image holds another
    pixel than the one the reference clamps to; the windows strictly inside
    have them on all four sides, those on the last row and column on two."""
    launch, _ = bilinear_listed
    kinds = set()
    for j, it in enumerate(launch.items):
        if it[3] is None or _empty(launch, j):
            continue
        x0, y0, ww, wh = it[3]
        win, full = launch.wins[j], launch.fulls[j]
        H, W = full.shape[:2]
        assert x0 > 0 and y0 > 0 and x0 + ww <= W and y0 + wh <= H
        assert not (win[..., :3] == R.BILINEAR_SURROUND[0]).any()
        assert it[2] == 3 or not (win[..., 3] == R.BILINEAR_SURROUND[3]).any()
        s = R.bilinear_samples(launch, j)
        ok, xi, yi, dx, dy = s["ok"], s["xi"], s["yi"], s["dx"], s["dy"]
        sides = {"left": 0, "right": 0, "top": 0, "bottom": 0}
        for ox, oy, wgt in ((0, 0, (1 - dx) * (1 - dy)), (1, 0, dx * (1 - dy)), (0, 1, (1 - dx) * dy), (1, 1, dx * dy)):
            nx, ny = xi + ox, yi + oy
            gx, gy = x0 + nx, y0 + ny
            out = ok & (wgt > 0) & ((nx < 0) | (nx >= ww) | (ny < 0) | (ny >= wh))
            out &= (gx >= 0) & (gx < W) & (gy >= 0) & (gy < H)
            used = win[np.clip(ny, 0, wh - 1), np.clip(nx, 0, ww - 1)]
            there = full[np.clip(gy, 0, H - 1), np.clip(gx, 0, W - 1)]
            out &= (used != there).any(axis=-1)
            for name, m in (("left", nx < 0), ("right", nx >= ww), ("top", ny < 0), ("bottom", ny >= wh)):
                sides[name] += int((out & m).sum())
        inside = x0 + ww < W and y0 + wh < H
        want = ("left", "right", "top", "bottom") if inside else ("left", "top")
        assert all(sides[k] > 0 for k in want), (it, sides)
        assert inside or (x0 + ww == W and y0 + wh == H)
        kinds.add((it[2], inside))
    assert kinds == {(3, True), (4, True), (3, False), (4, False)}


# --------------------------------------------------------------------------- rotate / flip gather

@pytest.fixture(scope="module")
def D():
    from image_processor_pipeline_amd import device
    return device


def _pil_gather(item, win):
    """rotations.py:55,96-101 (the box crop with its fallback for an opaque
    source only) and symmetry.py:114-119 through live Pillow."""
    rot = Image.fromarray(win).convert("RGBA").rotate(item[3], expand=True)
    if item[2] == 3:
        bb = rot.getbbox()
        if bb is not None and bb[2] > bb[0] and bb[3] > bb[1]:
            rot = rot.crop(bb)
    if item[4] & 1:
        rot = rot.transpose(Image.Transpose.FLIP_LEFT_RIGHT)
    if item[4] & 2:
        rot = rot.transpose(Image.Transpose.FLIP_TOP_BOTTOM)
    return np.asarray(rot)


def _gather_launches():
    return [R.gather_launch()] + [R.gather_residue_launch(k) for k in range(len(R.GATHER_RESIDUE_LAUNCHES))]


def test_gather_oracle_equals_pillow():
    for launch in _gather_launches():
        for it, win, ref in zip(launch.items, launch.wins, R.gather_refs(launch)):
            pil = _pil_gather(it, win)
            assert ref.shape == pil.shape and np.array_equal(ref, pil), it


def test_gather_table_claims():
    items = R.GATHER_ITEMS
    assert 36 <= len(items) <= 44
    sizes = [R.gather_out_size(it) for it in items]
    fast = [s for it, s in zip(items, sizes) if it[3] in (0.0, 90.0, 180.0, 270.0)]
    assert set(R.GATHER_WIDTHS) <= {s[0] for s in fast} and set(R.GATHER_HEIGHTS) <= {s[1] for s in fast}
    assert {R.gather_last_nt(s[1]) for s in fast} == {1, 2, 3}
    assert [R.gather_last_nt(h) for h in (1, 16, 17, 32, 33, 48, 49, 97)] == [1, 1, 2, 2, 3, 3, 1, 1]
    assert {s[0] % 4 for s in fast} == {0, 1, 2, 3}                                # tails of 1, 2, 3 pixels
    assert {(it[2], it[4]) for it in items if it[3] in (0.0, 90.0, 180.0, 270.0)} == \
        {(cn, f) for cn in (3, 4) for f in range(4)}
    assert {0.0, 90.0, 180.0, 270.0} | set(R.GATHER_ANGLES) == {it[3] for it in items}
    for a in R.GATHER_ANGLES:                                                       # each one under both plans
        assert {it[2] for it in items if it[3] == a} == {3, 4}, a
    cns = [it[2] for it in items]
    assert sum(a != b for a, b in zip(cns, cns[1:])) >= len(items) // 2             # interleaved
    # the largest output alone sets the grid, and is split 3 × 5 (no power of two)
    mw, mh = sizes[R.GATHER_LARGEST]
    assert all(s[0] < mw and s[1] < mh for k, s in enumerate(sizes) if k != R.GATHER_LARGEST)
    assert (-(-mw // R.GATHER_TILE_W), -(-mh // (R.GATHER_TILE_H * R.GATHER_RT))) == (3, 5)
    assert mw <= 210 and mh <= 210
    # windows
    kinds = set()
    for k, it in enumerate(items):
        w, h, cn, _, _, win, pad = it
        x0, y0, ww, wh = R.gather_window(it)
        assert 0 <= x0 and x0 + ww <= w and 0 <= y0 and y0 + wh <= h and ww > 0 and wh > 0
        if win is None:
            kinds.add("full")
        elif 0 < x0 and 0 < y0 and x0 + ww < w and y0 + wh < h:
            kinds.add("margin")
        elif (ww, wh) == (1, 1) and (w, h) != (1, 1):
            kinds.add(("corner", x0 == w - 1, y0 == h - 1))
            assert x0 in (0, w - 1) and y0 in (0, h - 1)
        elif (x0, y0, ww, wh) == (0, h - 1, w, 1):
            kinds.add(("last_row", cn))
        elif (x0, y0, ww, wh) == (w - 1, 0, 1, h):
            kinds.add(("last_col", cn))
    assert kinds >= {"full", "margin", ("corner", False, False), ("corner", True, False), ("corner", False, True),
                     ("corner", True, True), ("last_row", 3), ("last_row", 4), ("last_col", 3), ("last_col", 4)}
    # padded pitches: two per channel count, one of a single byte for each
    for cn in (3, 4):
        pads = [it[6] for it in items if it[2] == cn and it[6] > 0]
        assert len(pads) >= 2 and 1 in pads, cn
    # the 3-channel bottom-right 1×1 window, tight rows: mid-buffer and as the buffer's last bytes
    tail3 = [k for k, it in enumerate(items)
             if it[2] == 3 and it[6] == 0 and R.gather_window(it) == (it[0] - 1, it[1] - 1, 1, 1)]
    assert tail3[-1] == len(items) - 1 and any(0 < k < len(items) - 1 for k in tail3)
    launch = R.gather_launch()
    assert launch.flat.size == launch.src_offsets[-1] + 3 * items[-1][0] * items[-1][1]
    assert any(o % 2 for o in launch.src_offsets) and any(o % 4 == 0 for o in launch.src_offsets[1:])
    assert (launch.flat == R.GATHER_SRC_JUNK).sum() >= sum(it[6] * it[1] for it in items)
    # the three orders
    n = len(items)
    orders = [R.gather_order(o) for o in R.GATHER_ORDERS]
    assert all(sorted(o) == list(range(n)) for o in orders) and len({tuple(o) for o in orders}) == 3
    assert orders[0] == list(range(n)) and orders[1] == orders[0][::-1]
    assert orders[2].index(R.GATHER_LARGEST) == (n - 1) // 2 and orders[0].index(R.GATHER_LARGEST) != (n - 1) // 2


def test_gather_residue_table_claims():
    """Block counts ⌈max_w / 64⌉ · ⌈max_h / 48⌉ · n of the residue launches:
    every residue mod 8, and 1 and 9 blocks."""
    counts = []
    for k, (n_small, wide) in enumerate(R.GATHER_RESIDUE_LAUNCHES):
        items = R.gather_residue_items(k)
        assert len(items) == n_small + wide
        sizes = [R.gather_out_size(it) for it in items]
        small = [s for it, s in zip(items, sizes) if it is not R.GATHER_WIDE]
        assert all(s[0] <= R.GATHER_TILE_W and s[1] <= R.GATHER_TILE_H for s in small)      # one tile
        if wide:
            assert 0 < items.index(R.GATHER_WIDE) < len(items) - 1 or len(items) <= 2
            assert R.gather_blocks(sizes) == 3 * len(items)
        else:
            assert R.gather_blocks(sizes) == len(items)
        counts.append(R.gather_blocks(sizes))
    assert {c % 8 for c in counts} == set(range(8)) and {1, 9} <= set(counts)
    assert R.gather_blocks([(183, 206)] * 5) == 3 * 5 * 5


def _wrapper_buffer(flat, plan):
    """The bytes device.rotate_flip_nearest launches from: the caller's
    buffer, made longer when it is shorter than the plan's min_src_bytes."""
    return np.concatenate([flat, np.zeros(max(0, plan.min_src_bytes - flat.size), np.uint8)])


@pytest.mark.parametrize("order", R.GATHER_ORDERS)
def test_gather_model_equals_oracle(D, order):
    """plan_rotate_flip + ipp_gather_prepare, held to the oracle without a GPU:
    the host model of the kernel, evaluated from the prepared fields and again
    from a0..a5 / off_x / off_y / flip as make_sampler does for prepared = 0."""
    launch = R.gather_launch(order)
    plan = launch.plan(D)
    assert (plan.descs["prepared"] == 1).all()
    assert (plan.max_w, plan.max_h) == R.gather_out_size(R.GATHER_ITEMS[R.GATHER_LARGEST])
    buf = _wrapper_buffer(launch.flat, plan)
    for j, ref in enumerate(R.gather_refs(launch)):
        assert plan.shapes[j] == ref.shape[:2], launch.items[j]
        for prepared in (True, False):
            got = R.gather_model(buf, plan.descs[j], prepared)
            assert np.array_equal(got, ref), (launch.items[j], prepared)


def test_gather_model_equals_oracle_on_the_residue_launches(D):
    for k in range(len(R.GATHER_RESIDUE_LAUNCHES)):
        launch = R.gather_residue_launch(k)
        plan = launch.plan(D, row_align=16)
        assert plan.min_src_bytes <= launch.flat.size
        for j, ref in enumerate(R.gather_refs(launch)):
            assert np.array_equal(R.gather_model(launch.flat, plan.descs[j]), ref), (k, launch.items[j])


def test_gather_needs_one_byte_past_a_last_pixel_window(D):
    """A 1×1 window on the last pixel of a 3-channel source that ends the
    buffer: 3 bytes are left for a 4-byte load.  ipp_gather_prepare stores
    lim = 0 (not 2³² − 1), the plan asks for one byte more than the buffer
    has, and the model's bounds assertion is what notices a launch from the
    short buffer."""
    launch = R.gather_launch()
    plan = launch.plan(D)
    last = plan.descs[-1]
    assert int(last["base_off"]) == launch.flat.size - 3 and int(last["lim"]) == 0
    assert plan.min_src_bytes == launch.flat.size + 1
    assert R.gather_sampler(last, prepared=False)[:2] == (launch.flat.size - 3, 0)
    with pytest.raises(AssertionError, match="the gather reads bytes"):
        R.gather_model(launch.flat, last)
    mid = plan.descs[17]
    assert int(mid["lim"]) == 0 and int(mid["base_off"]) + 4 <= launch.flat.size
    # what rotate_crop_single plans for a 1×1×3 tensor
    one = D.plan_rotate_flip([(1, 1, 3)], [0.0], [0])
    assert one.min_src_bytes == 4 and int(one.descs[0]["lim"]) == 0
    # 4-channel windows never need it
    assert D.plan_rotate_flip([(1, 1, 4)], [45.0], [0], crop_to_bbox=False).min_src_bytes == 0
