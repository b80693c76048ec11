"""The H launch's fill trim on the paths beside PipeRunner.run that share it
(tests/test_gpu_pipe_fill_trim.py holds the run path and the discipline):

  tiles_63/64/65   the 64-tile limit of the trim (one header per lane, the
                   ballot mask full at 64, everything swept at 65);
  cn4, cn4_padded  4-channel sources, tight and padded pitch, through the C
                   entry points;
  scene_k3         SceneRunner.run: ipp_pipe_hpass on the later layers, the
                   in-place blend;
  labels_poisoned  the kernels that read α out of T, the constant groups of
                   the trimmed tiles included.

Every case fills T (and the output, where there is one) with 0x55 first,
compares with the CPU oracle exactly, and asserts what it is there for on the
plan (hpass_trim), never on the kernel's output.

The V launch takes overlays up to IPP_PIPE_MAX_OV_W = 992 px, that is 62 H
tiles, and fused.plan_pipe refuses wider ones; the H launch has no such limit
(ipp_pipe_hpass is a C entry point of its own).  So 63, 64 and 65 tiles are
reached by the H launch alone, planned with the Python check lifted, and what
is compared is T itself: every byte of the item's rows with the oracle's
horizontal pass over the premultiplied cut-out
(ops.resample_h(ops.premultiply(cut_out))), in T's layout [row group][column]
[channel][row of 4], XOR 0x80.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import ops
from oracle import pipe as opipe
from tests import label_refs as R
from tests import scene_refs as SR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
POISON = 0x55


@pytest.fixture(scope="module")
def fused():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from image_processor_pipeline_amd import fused as F
    return F


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _noise(seed, n, H, W, n_bg, bh, bw):
    """Random sources with real black inside, beside the fill, and backgrounds."""
    rng = np.random.default_rng(seed)
    src = rng.integers(0, 256, (n, H, W, 3), np.uint8)
    src[:, H // 3: H // 2, W // 4: W // 2] = 0
    return src, rng.integers(0, 256, (n_bg, bh, bw, 3), np.uint8)


def _bounds(plan):
    from image_processor_pipeline_amd import hpass_trim as HT
    assert HT.trim_enabled(plan.hsv if hasattr(plan, "hsv") else plan.pipe.hsv)
    return [HT.item_bounds(plan, i) for i in range(len(plan.descs))]


def _assert_every_item_trims(plan):
    """Every descriptor has bands with trimmed leading tiles and bands with trimmed trailing ones."""
    for i, b in enumerate(_bounds(plan)):
        assert any(lo > 0 for lo, hi, nt in b) and any(hi < nt for lo, hi, nt in b), (i, b)


# --- the 64-tile limit ---------------------------------------------------------------
TILES = {63: 0.888, 64: 0.902, 65: 0.916}     # ratio of a (30, 400) source at 12° on a (320, 1120) background


def _t_rows(tmp, h):
    """The item's T rows [0, lines) as (lines, out_len, 4) bytes, XOR 0x80 undone."""
    lines, w, pitch = int(h["lines"]), int(h["out_len"]), int(h["dst_pitch"])
    assert pitch == 16 * w
    groups = (lines + 3) // 4
    t = tmp[int(h["dst_off"]): int(h["dst_off"]) + groups * pitch].reshape(groups, w, 4, 4)   # [g][x][c][r]
    return (t.transpose(0, 3, 1, 2).reshape(4 * groups, w, 4) ^ 0x80)[:lines]


@pytest.mark.parametrize("ntiles", sorted(TILES))
def test_hpass_tile_limit_vs_oracle(fused, monkeypatch, ntiles):
    from image_processor_pipeline_amd import _native as N
    from image_processor_pipeline_amd import hpass_trim as HT
    from image_processor_pipeline_amd.device import _stream
    v_limit = N.IPP_PIPE_MAX_OV_W
    monkeypatch.setattr(N, "IPP_PIPE_MAX_OV_W", 1 << 16)      # the V launch's limit; only the H launch runs here
    (H, W), bg_hw = (30, 400), (320, 1120)
    cfg = fused.PipeConfig(margins=(0, 0, 0, 0))
    prm = fused.ItemParams(12.0, "o", 0, TILES[ntiles], 0, 0)
    plan = fused.plan_pipe((H, W), 1, bg_hw, 1, cfg, params=[prm])
    h = plan.descs[0]["h"]
    out_len = int(h["out_len"])
    assert (out_len + 15) >> 4 == ntiles and out_len > v_limit
    assert out_len % 16                                       # the last tile is ragged
    b = _bounds(plan)[0]
    assert all(nt == ntiles for lo, hi, nt in b) and len(b) >= 5
    if ntiles <= HT.TRIM_MAX_TILES:
        assert any(lo > 0 for lo, hi, nt in b) and any(hi < nt for lo, hi, nt in b), b
        # both ends of the mask: a band keeps tile 0, a band keeps the last tile
        assert any(lo == 0 and hi < nt for lo, hi, nt in b) and any(hi == nt and lo > 0 for lo, hi, nt in b), b
    else:
        assert all((lo, hi) == (0, nt) for lo, hi, nt in b), b

    src, _ = _noise(ntiles, 1, H, W, 1, 8, 8)
    runner = fused.PipeRunner(plan, DEV)
    runner.tmp.fill_(POISON)
    N.check(runner.lib.ipp_pipe_hpass(_t(src).data_ptr(), runner.tmp.data_ptr(), runner.coefs.data_ptr(),
                                      runner.descs.data_ptr(), 1, plan.max_out_w, plan.max_rows, 3,
                                      N.np_ptr(plan.hsv), plan.tap_format, _stream(runner.device)), "ipp_pipe_hpass")
    assert runner.status() == 0
    got = _t_rows(runner.tmp.cpu().numpy(), h)

    m = opipe.cut_out(src[0], prm, cfg)
    assert m.shape[:2] == (int(plan.items["cut_h"][0]), int(h["in_len"]))
    _, bh_, kh = ops.precompute_coeffs(m.shape[1], 0.0, float(m.shape[1]), out_len)
    exp = ops.resample_h(ops.premultiply(m), out_len, bh_, kh, int(h["line0"]), int(h["lines"]))
    assert (exp[..., 3] == 0).mean() > 0.3                    # a good share of T is fill
    assert np.array_equal(got, exp), int((got != exp).sum())


# --- 4-channel sources -----------------------------------------------------------------
CN4_SRC, CN4_BG = (150, 190), (256, 320)
CN4_ITEMS = [(45.0, "o", 0.5), (30.0, "hv", 0.45), (200.0, "v", 0.5), (110.0, "h", 0.3)]


@pytest.mark.parametrize("pad", [0, 20], ids=["cn4", "cn4_padded"])
def test_pipe_cn4_fill_trim_vs_oracle(fused, pad):
    """k_pipe_hpass2<4, false, 4> on oblique items: the 3-channel plan's
    descriptors with g.src_cn = 4 and the row pitch 4·W + pad (780: no
    multiple of 16), RGBA sources whose alpha bytes (0 among them) the pipe
    ignores as the reference's cv2.imread does, junk in the row padding."""
    from image_processor_pipeline_amd import _native as N
    from image_processor_pipeline_amd.device import _stream, _to_dev
    (H, W), (bh, bw) = CN4_SRC, CN4_BG
    pitch = 4 * W + pad
    assert pitch % 4 == 0 and (pad == 0 or pitch % 16)
    n = len(CN4_ITEMS)
    cfg = fused.PipeConfig(margins=(0, 0, 0, 0))
    params = [fused.ItemParams(a, s, k % 2, r, 3 + k, 5 + k) for k, (a, s, r) in enumerate(CN4_ITEMS)]
    plan = fused.plan_pipe((H, W), n, (bh, bw), 2, cfg, params=params)
    _assert_every_item_trims(plan)
    src, bgs = _noise(40 + pad, n, H, W, 2, bh, bw)

    descs = plan.descs.copy()
    g = np.ascontiguousarray(descs["g"])
    assert (g["src_cn"] == 3).all() and (g["src_pitch"] == 3 * W).all() and (g["src_off"] % (3 * H * W) == 0).all()
    g["src_off"] = g["src_off"] // (3 * H * W) * (H * pitch)
    g["src_cn"], g["src_pitch"] = 4, pitch
    N.check(N.load().ipp_gather_prepare(N.np_ptr(g), n), "ipp_gather_prepare")
    descs["g"] = g
    assert int((g["src_off"] + g["src_h"].astype(np.int64) * g["src_pitch"]).max()) <= n * H * pitch
    rng = np.random.default_rng(41)
    alpha = rng.integers(0, 256, (n, H, W, 1), np.uint8)
    alpha[:, ::3] = 0                                     # transparent rows: alpha is not the pipe's mask
    rows = rng.integers(0, 256, (n, H, pitch), np.uint8)
    rows[:, :, :4 * W] = np.concatenate([src, alpha], -1).reshape(n, H, 4 * W)

    runner = fused.PipeRunner(plan, DEV)
    dev_descs, dev_bgs, src4 = _to_dev(descs, runner.device), _t(bgs), _t(rows)
    runner.tmp.fill_(POISON)
    out = torch.full((n, bh, bw, 3), POISON, dtype=torch.uint8, device=DEV)
    lib, st = runner.lib, _stream(runner.device)
    N.check(lib.ipp_pipe_hpass_bgcopy(src4.data_ptr(), runner.tmp.data_ptr(), runner.coefs.data_ptr(),
                                      dev_descs.data_ptr(), n, plan.max_out_w, plan.max_rows, 4, N.np_ptr(plan.hsv),
                                      plan.tap_format, dev_bgs.data_ptr(), out.data_ptr(), st), "ipp_pipe_hpass_bgcopy")
    N.check(lib.ipp_pipe_vblend_bands(runner.tmp.data_ptr(), dev_bgs.data_ptr(), out.data_ptr(),
                                      runner.coefs.data_ptr(), dev_descs.data_ptr(), n, plan.bg_w, plan.bg_h,
                                      plan.max_ov_w, plan.max_ov_h, plan.tap_format, st), "ipp_pipe_vblend_bands")
    assert runner.status() == 0
    got = out.cpu().numpy()
    for i in range(n):
        exp = opipe.pipe_item(src[i], bgs, plan.params[i], cfg)
        assert np.array_equal(got[i], exp), (i, int((got[i] != exp).sum()))


# --- scenes ---------------------------------------------------------------------------
SCENE_SRC, SCENE_BG = (100, 120), (160, 192)
# (angle, sym, ratio, x, y) of the K = 3 overlays of two scenes; ratio <= 0.5 keeps every overlay inside the background
SCENE_ITEMS = [(45.0, "o", 0.5, 4, 6), (30.0, "h", 0.45, 40, 20), (160.0, "v", 0.4, 20, 30),
               (70.0, "hv", 0.5, 10, 2), (250.0, "o", 0.45, 30, 25), (20.0, "h", 0.35, 60, 40)]


def _scene_plan(fused, cfg):
    params = [fused.ItemParams(a, s, i // 3, r, x, y) for i, (a, s, r, x, y) in enumerate(SCENE_ITEMS)]
    plan = fused.plan_scenes(SCENE_SRC, 2, 3, SCENE_BG, 2, cfg, params=params)
    assert plan.per_scene == 3 and len(plan.descs) == 6
    _assert_every_item_trims(plan)
    return plan


def test_scene_k3_fill_trim_vs_oracle(fused):
    """SceneRunner.run on poisoned T and output: ipp_pipe_hpass_bgcopy on layer
    0, ipp_pipe_hpass on layers 1 and 2, k_pipe_vblend_over in place."""
    cfg = fused.PipeConfig(margins=(0, 0, 0, 0))
    plan = _scene_plan(fused, cfg)
    (H, W), (bh, bw) = SCENE_SRC, SCENE_BG
    src, bgs = _noise(51, 6, H, W, 2, bh, bw)
    overlays = SR.scene_overlays(src, plan, cfg)
    exp = SR.scene_composites(bgs, plan, overlays)
    runner = fused.SceneRunner(plan, DEV)
    runner.tmp.fill_(POISON)
    out = torch.full((2, bh, bw, 3), POISON, dtype=torch.uint8, device=DEV)
    runner.run(_t(src), _t(bgs), out)
    assert runner.status() == 0
    got = out.cpu().numpy()
    for s in range(2):
        assert np.array_equal(got[s], exp[s]), (s, int((got[s] != exp[s]).sum()))


# --- the label kernels on a poisoned T -----------------------------------------------
def _structured(n, H, W, n_bg, bh, bw, seed):
    """label_refs.structured_batch's recipe: a fill colour the V-only range
    makes transparent and one bright rectangle well inside each source, so
    every tight box lies inside its overlay and the source's own transparent
    pixels reach into the first and last swept tiles."""
    rng = np.random.default_rng(seed)
    src = np.empty((n, H, W, 3), np.uint8)
    src[:] = (90, 120, 60)
    for i in range(n):
        src[i, 2 * H // 5: 3 * H // 5, 2 * W // 5: 3 * W // 5] = rng.integers(160, 256, (3 * H // 5 - 2 * H // 5,
                                                                                         3 * W // 5 - 2 * W // 5, 3))
    return src, rng.integers(0, 256, (n_bg, bh, bw, 3), np.uint8)


def _assert_boxes_inside(boxes, ov_w, ov_h):
    """Every tight box leaves a column free on both sides of its overlay: a
    stale non-zero alpha in a trimmed tile would move an edge."""
    for (x0, y0, x1, y1), w, h in zip(boxes.tolist(), ov_w, ov_h):
        assert 0 < x0 < x1 < w and 0 < y0 < y1 < h, (x0, y0, x1, y1, w, h)


def test_labels_on_poisoned_t_pipe(fused):
    """k_pipe_overlay_bbox through PipeRunner.run_labelled, alpha_min 1 and
    128: 0x55 in T is alpha 0xD5, above both."""
    (H, W), (bh, bw) = CN4_SRC, CN4_BG
    n = len(CN4_ITEMS)
    cfg = fused.PipeConfig(margins=(0, 0, 0, 0), hsv_ranges=list(R.STRUCT_RANGES))
    params = [fused.ItemParams(a, s, k % 2, r, 3 + k, 5 + k) for k, (a, s, r) in enumerate(CN4_ITEMS)]
    plan = fused.plan_pipe((H, W), n, (bh, bw), 2, cfg, params=params)
    _assert_every_item_trims(plan)
    src, bgs = _structured(n, H, W, 2, bh, bw, 61)
    alphas = R.overlay_alphas(src, plan, cfg)
    runner = fused.PipeRunner(plan, DEV)
    dsrc, dbgs = _t(src), _t(bgs)
    for alpha_min in (1, 128):
        exp = R.ref_boxes(alphas, alpha_min)
        _assert_boxes_inside(exp, plan.items["ov_w"].tolist(), plan.items["ov_h"].tolist())
        runner.tmp.fill_(POISON)
        out = torch.full((n, bh, bw, 3), POISON, dtype=torch.uint8, device=DEV)
        _, labels = runner.run_labelled(dsrc, dbgs, out, tight=True, alpha_min=alpha_min, class_id=1)
        got = runner.overlay_bboxes(alpha_min)
        assert np.array_equal(got, exp), (alpha_min, got.tolist(), exp.tolist())
        assert labels == fused.yolo_labels(plan, 1, boxes=exp)
        res = out.cpu().numpy()
        for i in range(n):
            assert np.array_equal(res[i], opipe.pipe_item(src[i], bgs, plan.params[i], cfg)), (alpha_min, i)


def test_labels_on_poisoned_t_scenes(fused):
    """k_scene_alpha and k_scene_visible through SceneRunner.run_labelled and
    scene_boxes at (alpha_min, cover_min) = (1, 128): boxes, areas and visible
    counts."""
    cfg = fused.PipeConfig(margins=(0, 0, 0, 0), hsv_ranges=list(R.STRUCT_RANGES))
    plan = _scene_plan(fused, cfg)
    (H, W), (bh, bw) = SCENE_SRC, SCENE_BG
    src, bgs = _structured(6, H, W, 2, bh, bw, 62)
    overlays = SR.scene_overlays(src, plan, cfg)
    exp = SR.scene_rows(plan, overlays, 1, 128)
    free = SR.scene_rows(plan, overlays, 1, 128, occlusion=False)
    xy = np.stack([plan.items["x"], plan.items["y"]] * 2, axis=1)
    _assert_boxes_inside(free.reshape(6, 6)[:, :4] - xy, plan.items["ov_w"].tolist(), plan.items["ov_h"].tolist())
    runner = fused.SceneRunner(plan, DEV)
    runner.tmp.fill_(POISON)
    out = torch.full((2, bh, bw, 3), POISON, dtype=torch.uint8, device=DEV)
    _, labels = runner.run_labelled(_t(src), _t(bgs), out, class_ids=2, alpha_min=1, cover_min=128)
    got = runner.scene_boxes(1, 128)
    assert np.array_equal(got, exp), (got.tolist(), exp.tolist())
    assert labels == fused.scene_labels(exp, bw, bh, 2)
    assert np.array_equal(out.cpu().numpy(), SR.scene_composites(bgs, plan, overlays))
