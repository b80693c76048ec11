"""GPU: the tight boxes of the fused pipe's overlays (ipp_pipe_overlay_bbox),
the thresholded alpha box (ipp_alpha_bbox_min), run_labelled and the plugins'
tight_bbox option.  Every box is compared exactly with numpy's box of the
oracle's (or Pillow's) resized overlay alpha >= alpha_min (tests/label_refs.py)."""
import random

import numpy as np
import pytest
from PIL import Image

torch = pytest.importorskip("torch")

from tests import gpu_scene_support as S
from tests import label_refs as R
from tests.gpu_scene_support import DEV, to_dev as _t

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fused():
    return S.require_fused()


class Batch:
    """One planned batch after its H launch, with the oracle's overlay alphas."""

    def __init__(self, fused, src, bgs, plan, cfg):
        self.src, self.bgs, self.plan, self.cfg = src, bgs, plan, cfg
        self.runner = fused.PipeRunner(plan, DEV)
        self.dsrc, self.dbgs = _t(src), _t(bgs)
        self.out = torch.empty((len(src),) + bgs.shape[1:], dtype=torch.uint8, device=DEV)
        self.runner.hpass_bgcopy(self.dsrc, self.dbgs, self.out)
        self.alphas = R.overlay_alphas(src, plan, cfg)

    def check(self, alpha_min):
        got = self.runner.overlay_bboxes(alpha_min)
        exp = R.ref_boxes(self.alphas, alpha_min)
        assert got.dtype == np.int32 and got.shape == exp.shape
        assert np.array_equal(got, exp), (alpha_min, got.tolist(), exp.tolist())
        return exp

    def v_ksteps(self):
        """K steps of every V tap tile the box kernel visits (tile headers of
        the device tap buffer: int4 (first row, K steps, block, flags))."""
        coefs = self.runner.coefs.cpu().numpy()
        ks = set()
        for d in self.plan.descs:
            off, nt = int(d["v"]["coef_off"]), (int(d["v"]["out_len"]) + (int(d["p"]["y"]) & 15) + 15) >> 4
            ks |= set(coefs[off:off + 4 * nt].reshape(nt, 4)[:, 1].tolist())
        return ks


@pytest.fixture(scope="module")
def small(fused):
    """The batch of test_pipe_small_vs_oracle."""
    cfg = fused.PipeConfig(margins=(0.05, 9, 0.1, 3))
    src, bgs, plan = R.noise_batch(fused, 10, 150, 170, 3, 128, 160, cfg, 7)
    return Batch(fused, src, bgs, plan, cfg)


@pytest.mark.parametrize("alpha_min", [1, 128, 255])
def test_noise_small(small, alpha_min):
    plan = small.plan
    assert len(set((plan.items["y"] & 15).tolist())) >= 6      # tile phases
    ks = small.v_ksteps()
    print("V tile K steps:", sorted(ks))
    assert {2, 3} <= ks
    small.check(alpha_min)


def test_structured_tight_differs_from_rectangle(fused):
    src, bgs, plan, cfg = R.structured_batch(fused)
    b = Batch(fused, src, bgs, plan, cfg)
    exp = R.ref_boxes(b.alphas, 1)
    assert np.array_equal(exp[0], [-1, -1, -1, -1])            # item 0: nothing planted
    assert R.structured_conditions(plan, exp), exp.tolist()
    for a in (1, 128):
        b.check(a)
    # the tight labels differ from the rectangle labels wherever the box does
    tight = fused.yolo_labels(plan, boxes=exp)
    rect = fused.yolo_labels(plan)
    assert tight[0] is None
    assert sum(t != r for t, r in zip(tight, rect)) >= 8


def test_upscale_one_k_step(fused):
    cfg = fused.PipeConfig(margins=(2, 2, 2, 2), scale_min=0.6, scale_max=0.8)
    src, bgs, plan = R.noise_batch(fused, 4, 40, 50, 2, 128, 160, cfg, 13)
    b = Batch(fused, src, bgs, plan, cfg)
    ks = b.v_ksteps()
    print("V tile K steps:", sorted(ks))
    assert ks == {1}
    for a in (1, 200):
        b.check(a)


def test_wide_overlays_more_than_four_column_tiles(fused):
    """The shape of test_pipe_wide_overlays_vs_oracle: each wave loops over
    more than 4 of the 16-column tiles."""
    cfg = fused.PipeConfig(margins=(4, 4, 4, 4), scale_min=0.75, scale_max=0.8)
    src, bgs, plan = R.noise_batch(fused, 2, 300, 260, 2, 760, 800, cfg, 11, plan_seed=4)
    assert plan.max_ov_w > 560 and int(plan.items["ov_w"].min()) > 16 * 4 * 4
    b = Batch(fused, src, bgs, plan, cfg)
    for a in (1, 200):
        b.check(a)


def test_odd_background_width(fused):
    cfg = fused.PipeConfig(margins=(3, 5, 2, 7), scale_min=0.2, scale_max=0.6)
    src, bgs, plan = R.noise_batch(fused, 8, 90, 110, 3, 97, 125, cfg, 125)
    b = Batch(fused, src, bgs, plan, cfg)
    for a in (1, 128):
        b.check(a)


def test_overlay_bboxes_of_a_descriptor_range(small):
    full = small.check(1)
    items = np.sort(small.plan.order[2:7])
    assert np.array_equal(small.runner.overlay_bboxes(1, items=(2, 5)), full[items])


def test_run_labelled_leaves_the_composite_alone(fused, small):
    plan = small.plan
    runner = fused.PipeRunner(plan, DEV)
    ref = torch.full_like(small.out, 7)
    runner.run(small.dsrc, small.dbgs, ref)
    out = torch.full_like(small.out, 9)
    got_out, labels = runner.run_labelled(small.dsrc, small.dbgs, out, alpha_min=128, class_id=2)
    assert got_out is out and torch.equal(out, ref)
    assert labels == fused.yolo_labels(plan, 2, boxes=runner.overlay_bboxes(128))
    assert labels == fused.yolo_labels(plan, 2, boxes=R.ref_boxes(small.alphas, 128))
    out2 = torch.full_like(small.out, 5)
    _, rect = runner.run_labelled(small.dsrc, small.dbgs, out2, tight=False)
    assert torch.equal(out2, ref)
    assert rect == fused.yolo_labels(plan)


def test_overlay_bboxes_before_any_h_launch_raises(fused, small):
    from image_processor_pipeline_amd import _native as N
    runner = fused.PipeRunner(small.plan, DEV)
    with pytest.raises(N.NativeError):
        runner.overlay_bboxes()


def test_c_entry_points_refuse_bad_arguments(fused, small):
    from image_processor_pipeline_amd import _native as N
    lib, r, p = N.load(), small.runner, small.plan
    n = len(p.descs)
    bbox = torch.zeros(4 * n, dtype=torch.int32, device=DEV)
    st = torch.cuda.current_stream().cuda_stream

    def pipe(tmp=r.tmp.data_ptr(), coefs=r.coefs.data_ptr(), descs=r.descs.data_ptr(), a=1, fmt=p.tap_format,
             bb=bbox.data_ptr()):
        return lib.ipp_pipe_overlay_bbox(tmp, coefs, descs, n, p.max_ov_w, p.max_ov_h, a, fmt, bb, st)

    assert pipe() == N.IPP_OK
    for kw in (dict(a=0), dict(a=256), dict(fmt=0), dict(fmt=2), dict(tmp=None), dict(coefs=None), dict(descs=None),
               dict(bb=None)):
        assert pipe(**kw) == N.IPP_E_ARG, kw
    img = torch.zeros(16 * 16 * 4, dtype=torch.uint8, device=DEV)
    d = np.zeros(1, N.IMAGE_DESC)
    d[0]["w"], d[0]["h"], d[0]["pitch"], d[0]["cn"] = 16, 16, 64, 4
    dd = _t(d.view(np.uint8))
    for a, rc in ((0, N.IPP_E_ARG), (256, N.IPP_E_ARG), (1, N.IPP_OK)):
        assert lib.ipp_alpha_bbox_min(img.data_ptr(), dd.data_ptr(), 1, 16, 16, a, bbox.data_ptr(), st) == rc, a
    assert lib.ipp_alpha_bbox_min(None, dd.data_ptr(), 1, 16, 16, 1, bbox.data_ptr(), st) == N.IPP_E_ARG
    torch.cuda.synchronize()


def test_alpha_bbox_min(fused):
    from image_processor_pipeline_amd import device as D
    rng = np.random.default_rng(5)
    a = rng.integers(0, 256, (67, 65, 4), np.uint8)
    a[..., 3] = np.clip(np.add.outer(np.arange(67) * 3, np.arange(65) * 2) - 40, 0, 255)     # diagonal ramp
    b = rng.integers(0, 256, (16, 16, 4), np.uint8)
    b[..., 3] = (np.arange(16) * 17)[None, :]                                                # 0 .. 255 across
    b[:3, :, 3] = 0
    imgs = [_t(a), _t(b)]
    assert D.alpha_bbox_min(imgs, 1) == D.alpha_bbox(imgs)
    for amin in (1, 128, 255):
        exp = [R.np_box(im[..., 3] >= amin) for im in (a, b)]
        got = D.alpha_bbox_min(imgs, amin)
        assert [None if e[0] < 0 else tuple(e.tolist()) for e in exp] == got, amin
    low = a.copy()
    low[..., 3] = np.minimum(low[..., 3], 99)
    la = np.dstack([b[..., 0], np.full((16, 16), 99, np.uint8)])                            # 2-channel (LA)
    assert D.alpha_bbox_min([_t(low), _t(la)], 100) == [None, None]
    assert D.alpha_bbox_min([_t(la)], 99) == [(0, 0, 16, 16)]


def _soft_overlay(rng, h, w, border):
    """RGBA overlay: transparent border, alpha rising over a few pixels to an
    opaque core."""
    yy, xx = np.mgrid[0:h, 0:w]
    d = np.minimum.reduce([yy - border[0], h - 1 - border[1] - yy, xx - border[2], w - 1 - border[3] - xx])
    ov = rng.integers(0, 256, (h, w, 4), np.uint8)
    ov[..., 3] = np.clip(d * 40, 0, 255)
    return ov


@pytest.mark.parametrize("alpha_min", [1, 128])
def test_plugin_tight_bbox(fused, tmp_path, alpha_min):
    from image_processor_pipeline_amd import geometry as G
    from image_processor_pipeline_amd.labels_math import xyxy2xywhn
    from image_processor_pipeline_amd.transforms import overlays
    rng = np.random.default_rng(17)
    ovs = [_soft_overlay(rng, 97, 83, (9, 20, 5, 14)), _soft_overlay(rng, 64, 120, (2, 3, 30, 11)),
           rng.integers(0, 256, (50, 60, 4), np.uint8)]
    ovs[2][..., 3] = 0                                       # fully transparent
    bgs = [rng.integers(0, 256, (160, 200, 3), np.uint8), rng.integers(0, 256, (220, 180, 3), np.uint8)]
    pairs = []
    for k, ov in enumerate(ovs):
        po, pb = tmp_path / f"ov{k}.png", tmp_path / f"bg{k % 2}.png"
        Image.fromarray(ov, "RGBA").save(po)
        Image.fromarray(bgs[k % 2], "RGB").save(pb)
        pairs.append((po, pb))

    def run(name, batch, **opts):
        di, dl = tmp_path / f"{name}_img", tmp_path / f"{name}_lbl"
        di.mkdir()
        dl.mkdir()
        random.seed(77)
        if batch:
            res = overlays.paste_overlay_onto_background.batch(pairs, [di, dl], **opts)
        else:
            res = [overlays.paste_overlay_onto_background(po, pb, [di, dl], **opts) for po, pb in pairs]
        assert all(r is not None and len(r) == 2 for r in res), res
        return ([np.asarray(Image.open(r[0]).convert("RGB")) for r in res], [r[1].read_text() for r in res])

    comps_f, labels_f = run("file", False, tight_bbox=True, alpha_min=alpha_min)
    comps_b, labels_b = run("batch", True, tight_bbox=True, alpha_min=alpha_min)
    comps_r, labels_r = run("rect", False)
    assert labels_f == labels_b
    for c1, c2, c3 in zip(comps_f, comps_b, comps_r):
        assert np.array_equal(c1, c3) and np.array_equal(c2, c3)
    # Pillow is the reference: replay the draws, resize, box of alpha >= alpha_min
    random.seed(77)
    for k, (ov, label) in enumerate(zip(ovs, labels_f)):
        bh, bw = bgs[k % 2].shape[:2]
        ratio = random.uniform(0.15, 0.30)
        nw, nh = G.overlay_size(ov.shape[1], ov.shape[0], bw, bh, ratio)
        x = random.randint(0, bw - nw)
        y = random.randint(0, bh - nh)
        al = np.asarray(Image.fromarray(ov, "RGBA").resize((nw, nh), Image.LANCZOS))[..., 3]
        x0, y0, x1, y1 = R.np_box(al >= alpha_min).tolist()
        if x0 < 0:
            assert label == "", k
            continue
        cx, cy, w, h = xyxy2xywhn(np.array([x + x0, y + y0, x + x1, y + y1]).reshape(1, 4), bw, bh)[0]
        assert label == f"0 {cx:.6f} {cy:.6f} {w:.6f} {h:.6f}", k
        assert label != labels_r[k], k                      # the transparent border is gone
    assert labels_f[2] == "" and labels_r[2] != ""
