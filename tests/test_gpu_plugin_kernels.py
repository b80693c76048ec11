"""GPU: the kernels behind the drop-in plugins against ``oracle/ops.py``, on
the ragged batches and edge shapes of tests/plugin_refs.py.

Every comparison is ``np.array_equal`` with an array that comes from the oracle
(held to live Pillow on the same cases by test_plugin_refs_cpu.py) or from
numpy — never from another GPU call.  The ``*_batched_*`` file tests compare
two GPU paths with each other; this module is what holds the batched launches'
descriptor arrays (offsets, ``coef_off``, ``line0``, per-image sizes) and the
arithmetic both paths share (``div255``, ``blend16``, ``unpremultiply``,
``clip8``) to an independent reference.

  1. test_lanczos_single            ipp_lanczos_h / ipp_lanczos_v, one image
     test_(un)premultiply_whole_domain   every (α, c) through one H pass
     test_lanczos_h_line_window     the H pass's line0 / lines through the C ABI
  2. test_overlays_ragged           batch_ops.overlays: H, V, paste and box launches
  3. test_paste_padded_rows         ipp_paste_blend through the C ABI, pitched rows
  4. test_copy_windows_ragged       batch_ops.copy_windows: ipp_copy_window
  5. test_hsv_masks_ragged          batch_ops.hsv_masks: ipp_hsv_mask
  6. test_alpha_bbox_ragged, test_alpha_bbox_min_ragged
  7. test_enhance_*                 ipp_enhance_lsum / _color, ipp_box_pass
  8. test_rotate_bilinear_small     ipp_rotate_bilinear + box + window copy
     test_bilinear_ragged_vs_oracle, test_bilinear_alpha_square   ipp_rotate_bilinear
     through the C ABI: many items, windows, pitches, offsets, any matrix, the
     alpha round trip, into a sentinel-filled buffer
     test_rotate_bilinear_canvas_*, test_rotate_crop_bilinear_*   the wrappers on
     RGB tensors, views, angles outside [0, 360), flips, an empty box
  9. test_gather_ragged_vs_oracle, test_gather_ragged_unprepared_vs_oracle,
     test_gather_block_count_residues   ipp_rotate_flip_nearest over descriptors
     from plan_rotate_flip + ipp_gather_prepare: mixed sizes, windows, pitches
     and channel counts in one launch, into a sentinel-filled buffer
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import ops
from tests import plugin_refs as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def D():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from image_processor_pipeline_amd import device
    return device


@pytest.fixture(scope="module")
def B(D):
    from image_processor_pipeline_amd import batch_ops
    return batch_ops


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _same(got, exp, tag):
    got = np.asarray(got)
    assert got.shape == exp.shape, (tag, got.shape, exp.shape)
    assert np.array_equal(got, exp), (tag, int((got != exp).sum()), "bytes differ")


# --------------------------------------------------------------------------- 1. LANCZOS

@pytest.mark.parametrize("k", range(len(R.LANCZOS_CASES)), ids=lambda k: "{}x{}-{}x{}-{}".format(*R.LANCZOS_CASES[k]))
def test_lanczos_single(D, k):
    _, _, ow, oh, _ = R.LANCZOS_CASES[k]
    img = R.lanczos_image(k)
    got = D.resize_lanczos_rgba(_t(img), ow, oh).cpu().numpy()
    _same(got, ops.resize_lanczos_rgba(img, ow, oh), R.LANCZOS_CASES[k])


def _h_pass_identity(D, img, flags):
    """One ipp_lanczos_h launch with taps that reproduce the input, so the
    output is the flags' conversion of every pixel and nothing else."""
    from image_processor_pipeline_amd import _native as N
    from image_processor_pipeline_amd import geometry as G
    h, w = img.shape[:2]
    ksize, taps = G.identity_taps(w)
    d = np.zeros(1, N.RESAMPLE_DESC)
    d[0]["src_pitch"], d[0]["dst_pitch"] = 4 * w, 4 * w
    d[0]["in_len"], d[0]["out_len"], d[0]["lines"], d[0]["ksize"] = w, w, h, ksize
    src, dst = _t(img), torch.zeros((h, w, 4), dtype=torch.uint8, device=DEV)
    td, dd = D._to_dev(taps, src.device), D._to_dev(d, src.device)
    N.check(N.load().ipp_lanczos_h(src.data_ptr(), dst.data_ptr(), td.data_ptr(), dd.data_ptr(), 1, w, h, flags,
                                   D._stream(src.device)), "ipp_lanczos_h")
    return dst.cpu().numpy()


def test_unpremultiply_whole_domain(D):
    """rgba2rgbA over its whole domain, 254 dividing α × 256 colour bytes (and
    α 0 / 255): the float quotient's two corrections and the clamp at 255."""
    from image_processor_pipeline_amd import _native as N
    img = R.alpha_colour_square()
    _same(_h_pass_identity(D, img, N.IPP_RS_UNPREMULTIPLY), ops.unpremultiply(img), "unpremultiply")


def test_premultiply_whole_domain(D):
    """rgbA2rgba (MULDIV255) over every (α, c)."""
    from image_processor_pipeline_amd import _native as N
    img = R.alpha_colour_square()
    _same(_h_pass_identity(D, img, N.IPP_RS_PREMULTIPLY), ops.premultiply(img), "premultiply")


@pytest.mark.parametrize("line0,lines", [(0, 9), (2, 5), (8, 1), (3, 4)])
def test_lanczos_h_line_window(D, line0, lines):
    """``line0`` of the H pass through the C ABI: only rows [line0, line0 +
    lines) are resampled.  A whole-image resize always has line0 = 0
    (test_plugin_refs_cpu.py::test_whole_image_resize_reads_every_row), so no
    wrapper call reaches this field with another value."""
    from image_processor_pipeline_amd import _native as N
    from image_processor_pipeline_amd import geometry as G
    in_w, in_h, out_w = 20, 9, 65
    img = R.rgba_image(R.LANCZOS_SEED + 700, in_w, in_h)
    ksize, taps = G.lanczos_taps(in_w, out_w)
    d = np.zeros(1, N.RESAMPLE_DESC)
    d[0]["src_pitch"], d[0]["dst_pitch"] = 4 * in_w, 4 * out_w
    d[0]["in_len"], d[0]["out_len"], d[0]["lines"], d[0]["line0"], d[0]["ksize"] = in_w, out_w, lines, line0, ksize
    src, dst = _t(img), torch.zeros((lines, out_w, 4), dtype=torch.uint8, device=DEV)
    td, dd = D._to_dev(taps, src.device), D._to_dev(d, src.device)
    N.check(N.load().ipp_lanczos_h(src.data_ptr(), dst.data_ptr(), td.data_ptr(), dd.data_ptr(), 1, out_w, lines,
                                   N.IPP_RS_PREMULTIPLY, D._stream(src.device)), "ipp_lanczos_h")
    _, bh, kh = ops.precompute_coeffs(in_w, 0.0, float(in_w), out_w)
    _same(dst.cpu().numpy(), ops.resample_h(ops.premultiply(img), out_w, bh, kh, line0, lines), (line0, lines))


# --------------------------------------------------------------------------- 2. overlays, ragged

@pytest.fixture(scope="module")
def overlay_expected():
    """(inputs, oracle-resized overlays, oracle composites), computed once."""
    ovs, bgs, sizes, pos = R.overlay_inputs()
    resized = [ops.resize_lanczos_rgba(o, *s) for o, s in zip(ovs, sizes)]
    comps = [ops.paste_rgba_onto_rgb(b, r, x, y) for b, r, (x, y) in zip(bgs, resized, pos)]
    return (ovs, bgs, sizes, pos), resized, comps


@pytest.mark.parametrize("alpha_min", R.OVERLAY_ALPHA_MINS)
def test_overlays_ragged(B, overlay_expected, alpha_min):
    (ovs, bgs, sizes, pos), resized, comps = overlay_expected
    if alpha_min is None:
        got = B.overlays(ovs, bgs, sizes, pos)
    else:
        got, boxes = B.overlays(ovs, bgs, sizes, pos, bbox_alpha_min=alpha_min)
        assert boxes == [R.bbox_alpha_min(r, alpha_min) for r in resized]
    assert len(got) == len(comps)
    for k, (g, e) in enumerate(zip(got, comps)):
        _same(g, e, R.OVERLAY_ITEMS[k])


# --------------------------------------------------------------------------- 3. paste, padded rows

@pytest.mark.parametrize("k", range(len(R.PASTE_PITCH_CASES)))
def test_paste_padded_rows(D, k):
    from image_processor_pipeline_amd import _native as N
    bw, bh, ow, oh, x, y, bp, dp = R.PASTE_PITCH_CASES[k]
    bg, ov = R.paste_inputs(k)
    bg_rows = np.random.default_rng(R.PASTE_SEED + 200 + k).integers(0, 256, (bh, bp), np.uint8)   # junk padding
    bg_rows[:, :3 * bw] = bg.reshape(bh, 3 * bw)
    dst = torch.full((bh, dp), R.PASTE_SENTINEL, dtype=torch.uint8, device=DEV)
    d = np.zeros(1, N.PASTE_DESC)
    d[0]["bg_w"], d[0]["bg_h"], d[0]["bg_pitch"], d[0]["dst_pitch"] = bw, bh, bp, dp
    d[0]["ov_w"], d[0]["ov_h"], d[0]["ov_pitch"], d[0]["x"], d[0]["y"] = ow, oh, 4 * ow, x, y
    bgd, ovd = _t(bg_rows), _t(ov)
    dd = D._to_dev(d, bgd.device)
    N.check(N.load().ipp_paste_blend(bgd.data_ptr(), ovd.data_ptr(), dst.data_ptr(), dd.data_ptr(), 1, bw, bh,
                                     D._stream(bgd.device)), "ipp_paste_blend")
    got = dst.cpu().numpy()
    _same(got[:, :3 * bw].reshape(bh, bw, 3), ops.paste_rgba_onto_rgb(bg, ov, x, y), R.PASTE_PITCH_CASES[k])
    assert (got[:, 3 * bw:] == R.PASTE_SENTINEL).all(), "padding written"


# --------------------------------------------------------------------------- 4. window copies

def test_copy_windows_ragged(B):
    imgs = R.copy_images()
    got = B.copy_windows(imgs, R.COPY_JOBS)
    assert len(got) == len(R.COPY_JOBS)
    for g, (i, win, flip) in zip(got, R.COPY_JOBS):
        _same(g, R.window_ref(imgs[i], win, flip), (i, win, flip))


# --------------------------------------------------------------------------- 5. HSV masks

@pytest.mark.parametrize("s", range(len(R.HSV_SETS)))
def test_hsv_masks_ragged(B, s):
    from image_processor_pipeline_amd import geometry as G
    ranges, zones, gimp = R.HSV_SETS[s]
    imgs = R.hsv_images()
    got = B.hsv_masks(imgs, G.hsv_params(ranges, zones, gimp, bgr=True))
    assert len(got) == len(imgs)
    for g, im in zip(got, imgs):
        _same(g, ops.color_mask_bgra(im, ranges, zones, gimp), im.shape)


# --------------------------------------------------------------------------- 6. alpha boxes

def test_alpha_bbox_ragged(D):
    imgs = R.bbox_images()
    assert D.alpha_bbox([_t(im) for im in imgs]) == [ops.getbbox_alpha(im) for im in imgs]


@pytest.mark.parametrize("alpha_min", R.BBOX_ALPHA_MINS)
def test_alpha_bbox_min_ragged(D, alpha_min):
    # 2 and 4 channels only: alpha_bbox_min refuses an image without an alpha
    # band (ValueError) before anything is launched
    imgs = R.bbox_images(channels=(2, 4))
    assert D.alpha_bbox_min([_t(im) for im in imgs], alpha_min) == [R.bbox_alpha_min(im, alpha_min) for im in imgs]
    if alpha_min == 1:
        assert D.alpha_bbox_min([_t(im) for im in imgs], 1) == [ops.getbbox_alpha(im) for im in imgs]
    with pytest.raises(ValueError):
        D.alpha_bbox_min([_t(R.bbox_images(channels=(3,))[1])], alpha_min)


# --------------------------------------------------------------------------- 7. enhance

def _run_enhance(D, items):
    luts = R.enhance_luts()
    params = [D.EnhanceParams(f[0], f[1], f[2], r, luts if lut else None) for _, f, r, lut in items]
    got = D.enhance_rgb([_t(im) for im, _, _, _ in items], params)
    assert len(got) == len(items)
    for n, (g, (im, f, r, lut)) in enumerate(zip(got, items)):
        _same(g.cpu().numpy(), R.enhance_ref(im, f, r, luts if lut else None), (n, im.shape, f, r, lut))


def test_enhance_ragged_shapes(D):
    _run_enhance(D, R.enhance_ragged())


def test_enhance_factor_sweep(D):
    _run_enhance(D, R.enhance_factor_sweep())


def test_enhance_constant_images(D):
    _run_enhance(D, R.enhance_constant_images())


# --------------------------------------------------------------------------- 8. bilinear rotate

@pytest.mark.parametrize("k", range(len(R.ROTATE_SHAPES)), ids=lambda k: "{}x{}".format(*R.ROTATE_SHAPES[k]))
def test_rotate_bilinear_small(D, k):
    img = R.rotate_image(k)
    for a in R.ROTATE_ANGLES:
        got = D.rotate_crop_bilinear(_t(img), a).cpu().numpy()
        _same(got, ops.rotate_and_crop(img, a, "bilinear"), (R.ROTATE_SHAPES[k], a))


@pytest.fixture(scope="module")
def bilinear_cases():
    """{order: (launch, oracle outputs)}; the outputs are computed once, in the
    table's order, and shared by the three orders."""
    listed = R.bilinear_launch()
    refs = R.bilinear_refs(listed)
    out = {}
    for order in R.BILINEAR_ORDERS:
        launch = R.bilinear_launch(order)
        out[order] = (launch, [refs[k] for k in launch.index])
    return out


def _bilinear_vs_oracle(D, launch, refs):
    """One ipp_rotate_bilinear launch through the C ABI into total_bytes + 256
    bytes of sentinel: every item's rows equal its reference, and every byte
    outside the items' 4·out_w row bytes — row padding, the gaps between the
    items, the tail, the item without rows — still holds the sentinel."""
    from image_processor_pipeline_amd import _native as N
    assert len(launch.descs) == len(refs) == len(launch.items)
    out = torch.full((launch.total_bytes + R.BILINEAR_TAIL,), R.BILINEAR_SENTINEL, dtype=torch.uint8, device=DEV)
    src = _t(launch.flat)
    dd = D._to_dev(launch.descs, src.device)
    N.check(N.load().ipp_rotate_bilinear(src.data_ptr(), out.data_ptr(), dd.data_ptr(), len(launch.descs),
                                         launch.max_w, launch.max_h, D._stream(src.device)), "ipp_rotate_bilinear")
    got = out.cpu().numpy()
    written = np.zeros(got.size, bool)
    for j, ((oh, ow), off, pitch, ref) in enumerate(zip(launch.shapes, launch.dst_offsets, launch.dst_pitches, refs)):
        rows = got[off:off + oh * pitch].reshape(oh, pitch)
        _same(rows[:, :4 * ow].reshape(oh, ow, 4), ref, (j, launch.items[j]))
        written[off:off + oh * pitch].reshape(oh, pitch)[:, :4 * ow] = True
    stray = np.flatnonzero(~written & (got != R.BILINEAR_SENTINEL))
    assert stray.size == 0, ("bytes written outside the items' rows", stray[:8].tolist(), launch.total_bytes)


@pytest.mark.parametrize("order", R.BILINEAR_ORDERS)
def test_bilinear_ragged_vs_oracle(D, bilinear_cases, order):
    _bilinear_vs_oracle(D, *bilinear_cases[order])


@pytest.mark.parametrize("k", range(len(R.BILINEAR_ALPHA_MATRICES)), ids=["identity", "half_x", "half_y"])
def test_bilinear_alpha_square(D, k):
    """premultiply → lerp in double → truncate → unpremultiply inside the
    kernel, over every (α, c): alone, then with neighbours mixed half and half."""
    launch = R.bilinear_alpha_launch(k)
    refs = R.bilinear_refs(launch)
    if k == 0:
        sq = R.alpha_colour_square()
        assert np.array_equal(refs[0], ops.unpremultiply(ops.premultiply(sq)))
    _bilinear_vs_oracle(D, launch, refs)


BILINEAR_WRAPPER_ANGLES = (-33.3, 393.3, 450.0)


@pytest.mark.parametrize("angle", BILINEAR_WRAPPER_ANGLES + (33.3,))
def test_rotate_bilinear_canvas_rgb_tensor(D, angle):
    """A 3-channel tensor (src_cn = 3 through the wrapper), at angles below 0
    and above 360; 450 is the 90° transpose."""
    img = R.rgb_image(R.BILINEAR_SEED + 700, 21, 13)
    got = D.rotate_bilinear_canvas(_t(img), angle).cpu().numpy()
    _same(got, ops.rotate_expand_bilinear(ops.to_rgba(img), angle), angle)


@pytest.mark.parametrize("angle", BILINEAR_WRAPPER_ANGLES)
def test_rotate_bilinear_canvas_noncontiguous_view(D, angle):
    """A strided view: every second row, columns 3 .. 19 of a wider image."""
    big = R.rgba_image(R.BILINEAR_SEED + 701, 24, 31)
    view = _t(big)[::2, 3:20]
    assert not view.is_contiguous()
    img = np.ascontiguousarray(big[::2, 3:20])
    _same(D.rotate_bilinear_canvas(view, angle, 1).cpu().numpy(),
          R.flip_ref(ops.rotate_expand_bilinear(img, angle), 1), angle)
    _same(D.rotate_crop_bilinear(view, angle).cpu().numpy(), ops.rotate_and_crop(img, angle, "bilinear"), angle)


@pytest.mark.parametrize("flip", [1, 2, 3])
def test_rotate_crop_bilinear_flips(D, flip):
    """rotate_crop_bilinear(img, a, flip) on an odd-sized image is the flip of
    the oracle's crop; 450° takes the gather's transpose path."""
    img = R.rgba_image(R.BILINEAR_SEED + 702, 15, 9)
    img[:2] = 0                                   # a transparent band: the box is off-centre
    img[:, :3, 3] = 0
    for a in (33.3,) + BILINEAR_WRAPPER_ANGLES:
        crop = ops.rotate_and_crop(img, a, "bilinear")
        assert crop.shape != ops.rotate_expand_bilinear(img, a).shape
        _same(D.rotate_crop_bilinear(_t(img), a, flip).cpu().numpy(), R.flip_ref(crop, flip), (a, flip))


@pytest.mark.parametrize("angle", [33.3, 450.0])
def test_rotate_crop_bilinear_all_transparent(D, angle):
    """No α above 0: the box is None and the canvas comes back — zeros at
    33.3° (RGBa has no colour under α = 0), the transposed source at 450°."""
    img = R.rgba_image(R.BILINEAR_SEED + 703, 11, 7, "transparent")
    exp = ops.rotate_and_crop(img, angle, "bilinear")
    assert ops.getbbox_alpha(ops.rotate_expand_bilinear(img, angle)) is None
    assert exp.shape == ops.rotate_expand_bilinear(img, angle).shape
    _same(D.rotate_crop_bilinear(_t(img), angle, 2).cpu().numpy(), R.flip_ref(exp, 2), angle)


# --------------------------------------------------------------------------- 9. rotate / flip gather

@pytest.fixture(scope="module")
def gather_cases():
    """{order: (launch, oracle outputs)}; the outputs are computed once, in the
    table's order, and shared by the three orders."""
    listed = R.gather_launch()
    refs = R.gather_refs(listed)
    out = {}
    for order in R.GATHER_ORDERS:
        launch = R.gather_launch(order)
        out[order] = (launch, [refs[k] for k in launch.index])
    return out


def _gather_vs_oracle(D, launch, refs, row_align, prepared=True):
    """One ipp_rotate_flip_nearest launch into total_bytes + 256 bytes of
    sentinel: every item's rows equal its reference, and the row padding and
    the tail still hold the sentinel."""
    plan = launch.plan(D, row_align=row_align)
    assert len(plan.descs) == len(refs) and (plan.pitches % row_align == 0).all()
    if not prepared:
        plan.descs["prepared"] = 0
        plan.descs["b"] = 0x7A7A7A7A              # junk the kernel must not read
        plan.descs["base_off"] = 1 << 40
        plan.descs["lim"] = 0x7A7A7A7A
    out = torch.full((plan.total_bytes + R.GATHER_TAIL,), R.GATHER_SENTINEL, dtype=torch.uint8, device=DEV)
    buf = D.rotate_flip_nearest(_t(launch.flat), plan, out=out)
    assert buf.data_ptr() == out.data_ptr()
    got = buf.cpu().numpy()
    written = np.zeros(got.size, bool)
    for j, ((oh, ow), off, pitch, ref) in enumerate(zip(plan.shapes, plan.offsets, plan.pitches, refs)):
        rows = got[off:off + oh * pitch].reshape(oh, pitch)
        _same(rows[:, :4 * ow].reshape(oh, ow, 4), ref, (j, launch.items[j]))
        written[off:off + oh * pitch].reshape(oh, pitch)[:, :4 * ow] = True
    stray = np.flatnonzero(~written & (got != R.GATHER_SENTINEL))
    assert stray.size == 0, ("bytes written outside the items' rows", stray[:8].tolist(), plan.total_bytes)


@pytest.mark.parametrize("row_align", [128, 16])
@pytest.mark.parametrize("order", R.GATHER_ORDERS)
def test_gather_ragged_vs_oracle(D, gather_cases, order, row_align):
    _gather_vs_oracle(D, *gather_cases[order], row_align)


def test_gather_ragged_unprepared_vs_oracle(D, gather_cases):
    """prepared = 0: the kernel computes the sampler per block from a0..a5,
    off_x / off_y and flip.  Held to the oracle, not to the prepared launch."""
    _gather_vs_oracle(D, *gather_cases["listed"], 128, prepared=False)


@pytest.mark.parametrize("k", range(len(R.GATHER_RESIDUE_LAUNCHES)),
                         ids=lambda k: "{}small{}".format(R.GATHER_RESIDUE_LAUNCHES[k][0],
                                                          "+wide" if R.GATHER_RESIDUE_LAUNCHES[k][1] else ""))
def test_gather_block_count_residues(D, k):
    """Block counts of every residue mod 8, and of 1 and 9 (asserted from the
    tiling in test_plugin_refs_cpu.py): a block that xcd_remap or the FastDiv
    split loses or sends to another image leaves a tile of sentinel."""
    launch = R.gather_residue_launch(k)
    _gather_vs_oracle(D, launch, R.gather_refs(launch), 16)


@pytest.mark.parametrize("angle", [0.0, 45.0, 270.0])
def test_gather_single_pixel_rgb_tensor(D, angle):
    """rotate_crop_single on a 1×1×3 tensor: 3 bytes, so the wrapper launches
    from a copy one dword long (ipp.h's contract of the 4-byte load)."""
    img = R.rgb_image(R.GATHER_SEED + 900, 1, 1)
    got = D.rotate_crop_single(_t(img), angle, 3).cpu().numpy()
    _same(got, ops.flip(ops.rotate_and_crop(ops.to_rgba(img), angle), "hv"), angle)
