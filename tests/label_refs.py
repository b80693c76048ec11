"""Batches and CPU references shared by tests/test_labels_cpu.py and
tests/test_gpu_labels.py (not a test module).

The reference for every pixel comparison is the oracle's resized overlay:

    m  = opipe.cut_out(src[i], plan.params[i], cfg)
    nw, nh = ops.overlay_geometry(m.shape[1], m.shape[0], bw, bh, params.ratio)
    a  = ops.resize_lanczos_rgba(m, nw, nh)[..., 3] >= alpha_min

and numpy's box of `a` (the all -1 row when `a` has no true pixel)."""
import numpy as np

from oracle import ops
from oracle import pipe as opipe


def np_box(mask: np.ndarray) -> np.ndarray:
    """(x0, y0, x1, y1), half-open, of the true pixels; all -1 when none."""
    ys, xs = np.nonzero(mask)
    if len(ys) == 0:
        return np.full(4, -1, np.int32)
    return np.array([xs.min(), ys.min(), xs.max() + 1, ys.max() + 1], np.int32)


def overlay_alphas(src, plan, cfg):
    """The alpha band of every item's resized overlay (the paste mask of
    overlays.py:139), in item order."""
    out = []
    for i, prm in enumerate(plan.params):
        m = opipe.cut_out(src[i], prm, cfg)
        nw, nh = ops.overlay_geometry(m.shape[1], m.shape[0], plan.bg_w, plan.bg_h, prm.ratio)
        out.append(ops.resize_lanczos_rgba(m, nw, nh)[..., 3])
    return out


def ref_boxes(alphas, alpha_min: int) -> np.ndarray:
    return np.stack([np_box(a >= alpha_min) for a in alphas])


def noise_batch(fused, n, H, W, K, bh, bw, cfg, seed, plan_seed=None):
    """Random sources and backgrounds and their plan, as tests/test_gpu_parity.py
    draws them."""
    rng = np.random.default_rng(seed)
    src = rng.integers(0, 256, (n, H, W, 3), np.uint8)
    bgs = rng.integers(0, 256, (K, bh, bw, 3), np.uint8)
    plan = fused.plan_pipe((H, W), n, (bh, bw), K, cfg, seed=seed if plan_seed is None else plan_seed)
    return src, bgs, plan


# --- the structured batch: tight box != rectangle -------------------------------
# One V-only exclusion range (exact without OpenCV): every pixel with V <= 150
# is transparent, so the (90, 120, 60) fill (V = 120) and the rotation's black
# corners vanish and only the planted bytes in [160, 255] stay visible.
STRUCT_RANGES = [(0, 0, 0, 180, 255, 150)]
STRUCT_MARGINS = (4, 4, 4, 4)
STRUCT_SEED = 3        # chosen on the CPU: the reference meets structured_conditions


def structured_batch(fused, seed=STRUCT_SEED):
    cfg = fused.PipeConfig(margins=STRUCT_MARGINS, hsv_ranges=list(STRUCT_RANGES))
    n, H, W, K, bh, bw = 12, 140, 120, 2, 96, 128
    rng = np.random.default_rng(seed)
    src = np.empty((n, H, W, 3), np.uint8)
    src[:] = (90, 120, 60)
    mt, mb, ml, mr = STRUCT_MARGINS          # the crop: rows [mt, H - mb), columns [ml, W - mr)
    for i in range(n):
        rh, rw = (int(v) for v in rng.integers(8, 61, 2))
        y0 = int(rng.integers(mt, H - mb - rh + 1))
        x0 = int(rng.integers(ml, W - mr - rw + 1))
        if i == 0:
            continue                         # no rectangle: the -1 row
        if i == 1:
            rh = rw = 1                      # a single bright pixel: the reference decides
        elif i == 2:
            y0, x0 = mt, ml                  # touching the crop's top-left corner
        elif i == 3:
            y0, x0 = H - mb - rh, W - mr - rw    # touching its bottom-right corner
        src[i, y0:y0 + rh, x0:x0 + rw] = rng.integers(160, 256, (rh, rw, 3))
    bgs = rng.integers(0, 256, (K, bh, bw, 3), np.uint8)
    plan = fused.plan_pipe((H, W), n, (bh, bw), K, cfg, seed=seed)
    return src, bgs, plan, cfg


def structured_conditions(plan, boxes) -> bool:
    """At most 2 items empty, and at least 8 whose box lies strictly inside
    the overlay rectangle on at least two sides."""
    empty = int((boxes[:, 0] < 0).sum())
    inside = 0
    for (x0, y0, x1, y1), w, h in zip(boxes.tolist(), plan.items["ov_w"].tolist(), plan.items["ov_h"].tolist()):
        if x0 >= 0 and (x0 > 0) + (y0 > 0) + (x1 < w) + (y1 < h) >= 2:
            inside += 1
    return empty <= 2 and inside >= 8
