"""YOLO labels of the fused pipe, host side (no GPU): the plan's descriptor
order, the rectangle and tight label strings, and the alpha_min checks of
the Python wrappers.  (The planner is host code of libipp.so.)"""
import random

import numpy as np
import pytest

from tests.conftest import unpack


@pytest.fixture(scope="module")
def fused():
    from image_processor_pipeline_amd import _native as N
    from image_processor_pipeline_amd import fused as F
    try:
        N.load()
    except N.NativeUnavailable as e:
        pytest.fail(f"libipp.so is not built: {e}")
    return F


@pytest.fixture(scope="module")
def plan21(fused):
    """21 items on 4 backgrounds (the shape of
    test_pipe_copy_groups_straddling_backgrounds): the descriptors are not in
    item order."""
    cfg = fused.PipeConfig(margins=(3, 5, 2, 7), scale_min=0.2, scale_max=0.6)
    return fused.plan_pipe((90, 110), 21, (70, 256), 4, cfg, seed=256)


def _plugin_label(cls, x, y, w, h, bw, bh):
    """The per-file plugin's label (transforms/overlays.py, reference
    overlays.py:141-149)."""
    from image_processor_pipeline_amd.labels_math import xyxy2xywhn
    bbox = np.array([x, y, x + w, y + h]).reshape(1, 4)
    cx, cy, wn, hn = xyxy2xywhn(bbox, bw, bh)[0]
    return f"{cls} {cx:.6f} {cy:.6f} {wn:.6f} {hn:.6f}"


def test_plan_order_maps_descriptors_to_items(plan21):
    plan = plan21
    order = plan.order
    assert sorted(order.tolist()) == list(range(21))
    assert order.tolist() != list(range(21))      # the sort moved something
    for f in ("x", "y", "ov_w", "ov_h"):
        assert np.array_equal(plan.descs["p"][f], plan.items[f][order]), f
    # grouped by background, stable
    bgi = plan.items["bg_index"][order]
    assert np.all(np.diff(bgi) >= 0)
    for b in np.unique(bgi):
        assert np.all(np.diff(order[bgi == b]) > 0)


def test_yolo_labels_rectangle_equals_plugin_formula(fused, plan21):
    plan = plan21
    labels = fused.yolo_labels(plan, class_id=3)
    assert len(labels) == 21
    it = plan.items
    for i, lab in enumerate(labels):
        assert lab == _plugin_label(3, int(it["x"][i]), int(it["y"][i]), int(it["ov_w"][i]), int(it["ov_h"][i]),
                                    plan.bg_w, plan.bg_h), i
    assert fused.yolo_labels(plan)[0].startswith("0 ")


def test_rectangle_label_reproduces_reference_golden(fused, golden):
    """The strings the reference wrote (tests/golden/overlays_ref.npz
    `labels`), from the replayed draws (x, y, nw, nh) and the helper
    yolo_labels formats with."""
    from image_processor_pipeline_amd import geometry as G
    g = golden("overlays_ref.npz")
    ovs = unpack(g["ov_flat"], g["ov_shapes"])
    bgs = unpack(g["bg_flat"], g["bg_shapes"])
    for ov, bg, label, seed in zip(ovs, bgs, g["labels"], g["seeds"]):
        random.seed(int(seed))
        ratio = random.uniform(0.15, 0.30)
        bh, bw = bg.shape[:2]
        nw, nh = G.overlay_size(ov.shape[1], ov.shape[0], bw, bh, ratio)
        x = random.randint(0, bw - nw)
        y = random.randint(0, bh - nh)
        assert fused.yolo_label(0, (x, y, x + nw, y + nh), bw, bh) == str(label)


def test_yolo_labels_tight_boxes(fused, plan21):
    plan = plan21
    it = plan.items
    n = len(it)
    boxes = np.zeros((n, 4), np.int32)
    boxes[:, 0] = 1
    boxes[:, 1] = 2
    boxes[:, 2] = it["ov_w"] - 1
    boxes[:, 3] = it["ov_h"]
    boxes[4] = -1
    boxes[7] = (0, 0, it["ov_w"][7], it["ov_h"][7])     # the whole rectangle
    labels = fused.yolo_labels(plan, class_id=1, boxes=boxes)
    rect = fused.yolo_labels(plan, class_id=1)
    assert labels[4] is None
    assert labels[7] == rect[7]
    for i in range(n):
        if i in (4, 7):
            continue
        x, y = int(it["x"][i]) + 1, int(it["y"][i]) + 2
        assert labels[i] == _plugin_label(1, x, y, int(it["ov_w"][i]) - 2, int(it["ov_h"][i]) - 2,
                                          plan.bg_w, plan.bg_h), i
        assert labels[i] != rect[i]
    with pytest.raises(ValueError):
        fused.yolo_labels(plan, boxes=boxes[:-1])


@pytest.mark.parametrize("bad", [0, 256, -1, 1.5, True])
def test_alpha_min_out_of_range_is_refused(fused, bad):
    """The wrappers refuse alpha_min outside 1..255 before touching the device
    (the C entry points return IPP_E_ARG: tests/test_gpu_labels.py)."""
    from image_processor_pipeline_amd import batch_ops, device
    runner = object.__new__(fused.PipeRunner)     # no device: the check comes first
    with pytest.raises(ValueError):
        runner.overlay_bboxes(alpha_min=bad)
    with pytest.raises(ValueError):
        device.alpha_bbox_min([], alpha_min=bad)
    with pytest.raises(ValueError):
        batch_ops.overlays([], [], [], [], bbox_alpha_min=bad)
    assert device.check_alpha_min(1) == 1 and device.check_alpha_min(np.int32(255)) == 255
