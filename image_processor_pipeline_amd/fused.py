"""Batched device mode of the 5-stage pipe (BASELINE configs 3 and 4).

The reference runs five ``ProcessingStep``s chained through files
(pipeline.py:526-541), each calling one transform per item:

  1. recadrages.crop_from_border      (margin crop,          recadrages.py:13-61)
  2. rotations.process_rotations      (RGBA, NEAREST rotate, bbox crop, rotations.py:6-133)
  3. symmetry.generate_symmetries     (flip,                 symmetry.py:11-149)
  4. filtres_liste.process_images_with_color_masks (HSV α,   filtres_liste.py:41-149)
  5. overlays.paste_overlay_onto_background ('modulo' pairing with a cycled
     background set, LANCZOS resize + alpha paste,           overlays.py:24-187)

Here one host planning pass draws every random parameter in the reference's
draw order (``draw_params``) and fills one ``ipp_pipe_desc`` per item; the
device work is two launches for the whole batch (``ipp_pipe_hpass_bgcopy``,
``ipp_pipe_vblend_bands``).  Intermediate cut-outs never touch HBM.

The reference's last step also writes one YOLO label per composite
(overlays.py:141-149): ``yolo_labels`` formats them from the plan, and
``PipeRunner.run_labelled`` / ``overlay_bboxes`` give the tight box of what
is visible of each overlay (``ipp_pipe_overlay_bbox``, a third launch between
the two, opt-in).

Scenes (an addition; the reference pastes one overlay per composite):
``plan_scenes`` / ``SceneRunner`` paste K overlays per composite in layer
order — layer 0 as above, every later layer by an H launch without the copy
(``ipp_pipe_hpass``) and an in-place V launch (``ipp_pipe_vblend_over``) — and
label each overlay by what no later layer covers (``ipp_pipe_scene_boxes``).
``SceneRunner.scene_masks`` keeps that rule's per-pixel answer: one visibility
map per composite, bit k = layer k visible (``ipp_pipe_scene_map``;
``instance_ids`` and ``scene_instance_masks`` turn it into instance masks).
``SceneRunner.scene_polygons`` traces each overlay's outer contour from that
map on the device (``ipp_scene_contours``); ``scene_seg_labels`` formats the
YOLO segmentation lines.
"""
from __future__ import annotations

import math
import os
import random
import time
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _native as N
from . import geometry as G
from .device import SYM_FLIP, _stream, _to_dev
from .device import check_alpha_min as _check_alpha_min
from .labels_math import xyxy2xywhn

ALL_SYMS = ("o", "h", "v", "hv")
H_RING_COLUMNS = 512   # ipp_pipe.hip RING


@dataclass
class PipeConfig:
    margins: Tuple[float, float, float, float] = (64, 64, 64, 64)   # crop_from_border crop_margins
    angle_min: float = 1.0                                          # process_rotations defaults
    angle_max: float = 359.0
    sym_pool: Tuple[str, ...] = ALL_SYMS                             # generate_symmetries pool
    hsv_ranges: list = field(default_factory=lambda: list(G.REFERENCE_HSV_RANGES))
    zones: Optional[list] = None
    use_gimp_scale: bool = False
    scale_min: float = 0.15                                         # paste_overlay_onto_background
    scale_max: float = 0.30


@dataclass
class ItemParams:
    angle: float
    sym: str
    bg_index: int
    ratio: float
    x: int = 0
    y: int = 0


@dataclass
class PipePlan:
    descs: np.ndarray            # PIPE_DESC[n], processing order (grouped by background)
    axes: np.ndarray             # TAP_AXIS[2n]: H then V axis of each item (device tap planner)
    coef_words: int              # int32 size of the device tap buffer
    hsv: np.ndarray              # HSV_PARAMS
    items: np.ndarray            # PIPE_ITEM[n]: drawn parameters and geometry, item order
    sym_pool: Tuple[str, ...]    # items["sym"] indexes this pool
    tmp_bytes: int
    max_out_w: int
    max_rows: int
    bg_w: int
    bg_h: int
    algo_bytes_hpass: int = 0
    algo_bytes_vblend: int = 0
    tap_format: int = 1                   # IPP_TAPS_MFMA (the only device format)
    max_ov_w: int = 1
    max_ov_h: int = 1
    # split form (ipp_pipe_hpass_bgcopy + ipp_pipe_vblend_bands): the
    # composite outside the overlay's 16-pixel groups of its bands moves with
    # the H pass.  Algorithmic bytes follow SURVEY §8(d)'s fixed blend formula
    # (the background read once per item, the composite written once);
    # copy_read_bytes is what the grouped copy actually loads (one background
    # per run of same-background items in a copy group, IPP_PT_COPY_READS).
    algo_bytes_hpass_bgcopy: int = 0
    algo_bytes_vblend_bands: int = 0
    copy_read_bytes: int = 0

    @property
    def params(self) -> List[ItemParams]:
        it = self.items
        return [ItemParams(float(a), self.sym_pool[s], int(b), float(r), int(x), int(y))
                for a, s, b, r, x, y in zip(it["angle"], it["sym"], it["bg_index"], it["ratio"], it["x"], it["y"])]

    @property
    def order(self) -> np.ndarray:
        """order[i] = item index of descriptor i: the planner groups the
        descriptors by background with a stable sort (ipp_plan.cpp)."""
        return np.argsort(self.items["bg_index"], kind="stable")

    @property
    def cut_dims(self) -> List[Tuple[int, int]]:
        """(h, w) of each item's cut-out M."""
        return list(zip(self.items["cut_h"].tolist(), self.items["cut_w"].tolist()))

    @property
    def ov_dims(self) -> List[Tuple[int, int]]:
        """(h, w) of each item's resized overlay."""
        return list(zip(self.items["ov_h"].tolist(), self.items["ov_w"].tolist()))


def draw_params(n_global: int, stop: int, src_hw: Tuple[int, int], bg_hw: Tuple[int, int], n_bg: int,
                cfg: PipeConfig, seed: int):
    """Every random draw of the 5-step pipeline, consumed from ONE stream in
    the order a chained ``ProcessingPipeline`` of the five reference steps
    consumes it (step-major: each step runs over all its files, in sorted
    order, before the next step starts; pipeline.py:555-566):

      1. crop_from_border          — no draw;
      2. process_rotations         — one ``uniform(angle_min, angle_max)`` per
                                     file (rotations.py:89; num_rotations=1,
                                     include_original=False), all n_global files;
      3. generate_symmetries       — one ``sample(pool, 1)`` per file
                                     (symmetry.py:122; choose_random=1,
                                     include_original=False), all n_global files;
      4. process_images_with_color_masks — no draw;
      5. paste_overlay_onto_background, 'modulo' pairing — ``shuffle`` of the
         background list (pipeline.py:202), then per item ``uniform`` ratio
         (overlays.py:108) and two ``randint`` (overlays.py:133-134), whose
         ranges depend on the item's geometry, for items 0 .. stop-1.

    Returns (angles, syms, order, per-item (ratio, x, y, geometry)) for
    items 0 .. stop-1; items ≥ stop only consume their steps-2/3 draws."""
    H, W = src_hw
    bh, bw = bg_hw
    rng = random.Random(seed)
    pool = list(cfg.sym_pool)
    angles = [rng.uniform(cfg.angle_min, cfg.angle_max) for _ in range(n_global)]
    syms = [rng.sample(pool, 1)[0] for _ in range(n_global)]
    order = list(range(n_bg))
    rng.shuffle(order)
    t, b, l, r = G.crop_margins(H, W, cfg.margins)
    wc, hc = W - l - r, H - t - b
    per_item = []
    for gi in range(stop):
        ratio = rng.uniform(cfg.scale_min, cfg.scale_max)
        plan, box, (nw_, nh_) = item_geometry(wc, hc, angles[gi], ratio, bw, bh, gi)
        x = rng.randint(0, bw - nw_)
        y = rng.randint(0, bh - nh_)
        per_item.append((ratio, x, y, plan, box, (nw_, nh_)))
    return angles, syms, order, per_item


def item_geometry(wc: int, hc: int, angle: float, ratio: float, bw: int, bh: int, gi: int = 0):
    """One item's host geometry: the rotation plan of the wc×hc crop
    (rotations.py:96), its bbox (x, y, w, h) (rotations.py:99-109, fallback
    to the whole canvas) and the resized overlay (w, h) (overlays.py:106-126)."""
    plan = G.rotation_plan(wc, hc, angle)
    bb = G.rotated_bbox(wc, hc, plan)
    if bb is not None and bb[2] > bb[0] and bb[3] > bb[1]:
        box = (bb[0], bb[1], bb[2] - bb[0], bb[3] - bb[1])
    else:
        box = (0, 0, plan.nw, plan.nh)
    nw_, nh_ = G.overlay_size(box[2], box[3], bw, bh, ratio)
    if nw_ <= 0 or nh_ <= 0:
        raise ValueError(f"item {gi}: degenerate overlay size {nw_}x{nh_}")
    return plan, box, (nw_, nh_)


def shard_range(n_global: int, rank: int, world: int) -> Tuple[int, int]:
    """Contiguous block of the global item list owned by `rank`:
    sizes differ by at most one, lower ranks take the remainder."""
    if world <= 0 or not 0 <= rank < world:
        raise ValueError(f"bad rank/world {rank}/{world}")
    q, rem = divmod(n_global, world)
    start = rank * q + min(rank, rem)
    return start, start + q + (1 if rank < rem else 0)


def plan_threads() -> int:
    """Host threads for the batch planner: the job's CPU share
    (OMP_NUM_THREADS when set, else the CPUs this process may run on)."""
    try:
        n = int(os.environ.get("OMP_NUM_THREADS", "0"))
    except ValueError:
        n = 0
    if n <= 0:
        n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    return max(1, min(n, 32))


_PLAN_ERRORS = {
    1: (NotImplementedError, "rotation canvas beyond Pillow's 16.16 fixed-point range (>32767 px)"),
    2: (NotImplementedError, "non-affine ScaleAffine table"),
    3: (ValueError, "degenerate overlay size"),
    4: (ValueError, "parameters do not fit the background (position, background index or symmetry)"),
    5: (ValueError, "LANCZOS downscale needs a tap window wider than the fused H pass's 512-column LDS ring; "
                    "use the plugin path"),
    6: (ValueError, "empty range for randrange() (overlay larger than the background)"),
}


def plan_pipe(src_hw: Tuple[int, int], n: int, bg_hw: Tuple[int, int], n_bg: int, cfg: PipeConfig,
              seed: int = 0, src_pitch: Optional[int] = None, item_range: Optional[Tuple[int, int]] = None,
              n_global: Optional[int] = None, params: Optional[Sequence[ItemParams]] = None,
              n_threads: int = 0) -> PipePlan:
    """Plan `n` items.  The random stream is the one a chained file-mode
    ``ProcessingPipeline`` of the five reference steps over ``n_global``
    sources would consume under ``random.seed(seed)`` (``draw_params``).
    With ``item_range=(start, stop)`` only items [start, stop) of that global
    batch are planned (stop - start must equal n): every rank of a sharded run
    sees exactly the parameters a single process would give those items, so
    outputs do not depend on the number of GPUs.  ``n_global`` defaults to
    ``stop``.  With ``params`` (one ItemParams per item) nothing is drawn:
    the caller's angles, symmetries, backgrounds, ratios and positions are
    planned as given (positions must keep the overlay inside the background).

    The whole plan is one call of the threaded C planner
    (``ipp_plan_pipe_batch``: CPython's MT19937 draws, Pillow's rotate
    geometry, the opaque getbbox, the overlay size, the descriptors); the
    LANCZOS taps are built later on the device (``PipeRunner``)."""
    H, W = src_hw
    bh, bw = bg_hw
    start, stop = item_range if item_range is not None else (0, n)
    if stop - start != n or start < 0 or n <= 0:
        raise ValueError(f"item_range {item_range} does not hold {n} items")
    n_global = stop if n_global is None else n_global
    if n_global < stop:
        raise ValueError(f"n_global {n_global} < item_range stop {stop}")
    t, b, l, r = G.crop_margins(H, W, cfg.margins)
    items = np.zeros(n, N.PIPE_ITEM)
    c = np.zeros((), N.PIPE_PLAN_CFG)
    pool = tuple(cfg.sym_pool)
    given = params
    if given is None and not (isinstance(seed, int) and abs(seed) < 1 << 64):
        # seeds the C generator does not take (floats, strings, > 64 bits):
        # draw in Python, plan the draws as given parameters
        angles, syms, order, drawn = draw_params(n_global, stop, src_hw, bg_hw, n_bg, cfg, seed)
        given = [ItemParams(angles[g], syms[g], order[g % n_bg], drawn[g][0], drawn[g][1], drawn[g][2])
                 for g in range(start, stop)]
    if given is not None:
        if len(given) != n:
            raise ValueError(f"{len(given)} ItemParams for {n} items")
        pool = ALL_SYMS
        for i, it in enumerate(given):
            if it.sym not in SYM_FLIP:
                raise ValueError(f"item {start + i}: parameters {it} do not fit a {bw}x{bh} background")
        items["angle"] = [it.angle for it in given]
        items["ratio"] = [it.ratio for it in given]
        items["sym"] = [ALL_SYMS.index(it.sym) for it in given]
        items["bg_index"] = [it.bg_index for it in given]
        items["x"] = [it.x for it in given]
        items["y"] = [it.y for it in given]
        c["given"] = 1
    else:
        if not 1 <= len(pool) <= 4 or any(p not in SYM_FLIP for p in pool):
            raise ValueError(f"symmetry pool {pool}: 1 to 4 of {ALL_SYMS}")
        c["seed"] = abs(seed)
    c["src_h"], c["src_w"], c["src_pitch"] = H, W, src_pitch or 0
    c["crop_t"], c["crop_b"], c["crop_l"], c["crop_r"] = t, b, l, r
    c["bg_h"], c["bg_w"], c["n_bg"] = bh, bw, n_bg
    c["n_sym"] = len(pool)
    c["sym_flip"][:len(pool)] = [SYM_FLIP[p] for p in pool]
    c["n_global"], c["start"], c["stop"] = n_global, start, stop
    c["angle_min"], c["angle_max"] = cfg.angle_min, cfg.angle_max
    c["scale_min"], c["scale_max"] = cfg.scale_min, cfg.scale_max
    c["n_threads"] = n_threads or plan_threads()
    c["ring_cols"] = H_RING_COLUMNS
    descs = np.zeros(n, N.PIPE_DESC)
    axes = np.zeros(2 * n, N.TAP_AXIS)
    tot = np.zeros(N.IPP_PLAN_TOTALS, np.int64)
    lib = N.load()
    rc = lib.ipp_plan_pipe_batch(N.np_ptr(c), N.np_ptr(items), N.np_ptr(descs), N.np_ptr(axes), N.np_ptr(tot))
    if rc == N.IPP_E_RANGE and int(tot[N.PT["err_code"]]) in _PLAN_ERRORS:
        exc, msg = _PLAN_ERRORS[int(tot[N.PT["err_code"]])]
        raise exc(f"item {int(tot[N.PT['err_item']])}: {msg}")
    N.check(rc, "ipp_plan_pipe_batch")
    T = {k: int(tot[v]) for k, v in N.PT.items()}
    if T["max_ov_w"] > N.IPP_PIPE_MAX_OV_W:
        # refused here, before either launch: the V launch holds an overlay's
        # 16 rows in 64 KB of LDS (ipp.h IPP_PIPE_MAX_OV_W)
        raise ValueError(f"overlay width {T['max_ov_w']} px exceeds the fused pipe's limit of "
                         f"{N.IPP_PIPE_MAX_OV_W} px (ipp_pipe_vblend_bands); use the file-mode plugins")
    hsv = G.hsv_params(cfg.hsv_ranges, cfg.zones, cfg.use_gimp_scale, bgr=False)
    return PipePlan(descs, axes, T["coef_words"], hsv, items, pool, T["tmp_bytes"], T["max_out_w"], T["max_rows"],
                    bw, bh, T["algo_h"], T["algo_v"], N.IPP_TAPS_MFMA, T["max_ov_w"], T["max_ov_h"],
                    T["algo_h"] + T["copy_bytes"], T["algo_v"] - T["copy_bytes"], T["copy_reads"])


def plan_taps(plan: PipePlan, device, stream=None) -> Tuple[torch.Tensor, int]:
    """The plan's LANCZOS taps, built on the device (ipp_pipe_plan_taps):
    returns (int32 tensor of plan.coef_words (+ slack), tiles rebuilt on the
    host).  Synchronises the stream."""
    lib = N.load()
    device = torch.device(device)
    coefs = torch.empty(plan.coef_words + 4096, dtype=torch.int32, device=device)
    nb = lib.ipp_pipe_taps_scratch_bytes(len(plan.axes))
    scratch = torch.empty(int(nb), dtype=torch.uint8, device=device)
    stats = np.zeros(2, np.int64)
    N.check(lib.ipp_pipe_plan_taps(N.np_ptr(plan.axes), len(plan.axes), coefs.data_ptr(), scratch.data_ptr(),
                                   N.np_ptr(stats), stream if stream is not None else _stream(device)),
            "ipp_pipe_plan_taps")
    if stats[1]:
        raise N.NativeError(f"ipp_pipe_plan_taps: device status {int(stats[1])} (tile beyond its K-step bound)")
    return coefs, int(stats[0])


def yolo_label(class_id: int, box: Tuple[int, int, int, int], bg_w: int, bg_h: int) -> str:
    """One YOLO label line for the pixel box (x0, y0, x1, y1) on a bg_w×bg_h
    composite, formatted as the reference does (overlays.py:143-149)."""
    cx, cy, w, h = xyxy2xywhn(np.array(box).reshape(1, 4), bg_w, bg_h)[0]
    return f"{class_id} {cx:.6f} {cy:.6f} {w:.6f} {h:.6f}"


def yolo_labels(plan: PipePlan, class_id: int = 0, boxes: Optional[np.ndarray] = None) -> List[Optional[str]]:
    """The YOLO label of every item's composite, in item order.

    ``boxes=None``: the reference's label, the resized overlay's rectangle
    (x, y, x + ov_w, y + ov_h) (overlays.py:141-149) — byte for byte what the
    per-file plugin writes.  ``boxes`` = the (n, 4) array of
    ``PipeRunner.overlay_bboxes`` (overlay coordinates): the tight label, the
    box (x + x0, y + y0, x + x1, y + y1) through the same conversion.  An
    item whose row is all -1 has no visible overlay pixel and gets ``None``:
    the caller writes an empty label file for it, the YOLO convention for an
    image without objects."""
    it = plan.items
    n = len(it)
    if boxes is not None:
        boxes = np.asarray(boxes)
        if boxes.shape != (n, 4):
            raise ValueError(f"boxes of shape {boxes.shape} for {n} items")
    out: List[Optional[str]] = []
    for i in range(n):
        x, y = int(it["x"][i]), int(it["y"][i])
        if boxes is None:
            box = (x, y, x + int(it["ov_w"][i]), y + int(it["ov_h"][i]))
        elif boxes[i][0] < 0:
            out.append(None)
            continue
        else:
            x0, y0, x1, y1 = (int(v) for v in boxes[i])
            box = (x + x0, y + y0, x + x1, y + y1)
        out.append(yolo_label(class_id, box, plan.bg_w, plan.bg_h))
    return out


def overlap_bounds(n: int, parts: int, ratio: float = 1.0, group: int = N.IPP_PIPE_COPY_GROUP) -> List[int]:
    """Item-range bounds of PipeRunner.run_overlapped: `parts` ranges of whole
    copy groups, range k holding a share proportional to ratio**k; bounds[0]
    = 0, bounds[-1] = n, non-decreasing (a range may be empty)."""
    if n < 0 or parts < 1 or ratio <= 0:
        raise ValueError(f"overlap_bounds: n={n} parts={parts} ratio={ratio}")
    groups = (n + group - 1) // group
    w = [ratio ** k for k in range(parts)]
    cum = [sum(w[:k]) / sum(w) for k in range(parts + 1)]
    b = [min(n, group * int(round(groups * c))) for c in cum]
    b[-1] = n
    return b


def _check_gpu_u8(owner: str, caller: str, src: torch.Tensor, bgs: torch.Tensor, out: torch.Tensor) -> None:
    """The entry points that take tensors hand their raw pointers to the
    launches: each must be a contiguous uint8 tensor on the GPU."""
    for t, name in ((src, "src"), (bgs, "bgs"), (out, "out")):
        if not (t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous()):
            raise N.NativeUnavailable(f"{owner}.{caller}: {name} must be a contiguous uint8 ROCm tensor")


def _launch_hpass_bgcopy(lib, plan: PipePlan, src: int, tmp: int, coefs: int, descs: int, n: int, bgs: int, out: int,
                         stream: int) -> None:
    """The H launch (ipp_pipe_hpass_bgcopy) of `n` descriptors at device
    address `descs`; the other buffers are device addresses too."""
    N.check(lib.ipp_pipe_hpass_bgcopy(src, tmp, coefs, descs, n, plan.max_out_w, plan.max_rows, 3, N.np_ptr(plan.hsv),
                                      plan.tap_format, bgs, out, stream), "ipp_pipe_hpass_bgcopy")


def _launch_vblend_bands(lib, plan: PipePlan, tmp: int, bgs: int, out: int, coefs: int, descs: int, n: int,
                         stream: int) -> None:
    """The V launch (ipp_pipe_vblend_bands) of the same descriptor range."""
    N.check(lib.ipp_pipe_vblend_bands(tmp, bgs, out, coefs, descs, n, plan.bg_w, plan.bg_h, plan.max_ov_w,
                                      plan.max_ov_h, plan.tap_format, stream), "ipp_pipe_vblend_bands")


def _pipe_status(lib, device) -> int:
    """Sticky status of the pipe kernels since the last call (ipp_pipe_status;
    bit 0: an H tile's window exceeded the LDS ring).  Synchronises."""
    st = np.zeros(1, np.int32)
    N.check(lib.ipp_pipe_status(N.np_ptr(st), _stream(device)), "ipp_pipe_status")
    return int(st[0])


class PipeRunner:
    """Device-resident plan + scratch for repeated runs of one batch."""

    def __init__(self, plan: PipePlan, device):
        self.plan = plan
        self.device = torch.device(device)
        self.descs = _to_dev(plan.descs, self.device)
        self.coefs, self.host_tiles = plan_taps(plan, self.device)
        self.tmp = torch.empty(plan.tmp_bytes, dtype=torch.uint8, device=self.device)
        self.lib = N.load()
        self._hpass_done = False   # an H launch has filled tmp (overlay_bboxes needs it)

    @staticmethod
    def _check_tensors(caller: str, src: torch.Tensor, bgs: torch.Tensor, out: torch.Tensor) -> None:
        _check_gpu_u8("PipeRunner", caller, src, bgs, out)

    def hpass_bgcopy(self, src: torch.Tensor, bgs: torch.Tensor, out: torch.Tensor, items=None) -> None:
        """H pass + the composite rows outside the overlay bands (split form);
        `items` = (first, count) of the descriptors in processing order."""
        p = self.plan
        i0, n = items if items is not None else (0, len(p.descs))
        _launch_hpass_bgcopy(self.lib, p, src.data_ptr(), self.tmp.data_ptr(), self.coefs.data_ptr(),
                             self.descs.data_ptr() + i0 * p.descs.itemsize, n, bgs.data_ptr(), out.data_ptr(),
                             _stream(self.device))
        self._hpass_done = True

    def overlay_bboxes(self, alpha_min: int = 1, items=None) -> np.ndarray:
        """Tight boxes of the resized overlays (ipp_pipe_overlay_bbox): (n, 4)
        int32 rows (x0, y0, x1, y1), half-open, in overlay coordinates, of the
        pixels whose alpha (the paste mask of overlays.py:139) is >=
        alpha_min; an invisible overlay has the row (-1, -1, -1, -1).  Rows
        are in item order.  It reads the H launch's scratch, so it runs after
        ``hpass_bgcopy`` (before the next one refills the scratch) on the
        current stream, and synchronises for the copy back.  `items` = (first,
        count) of the descriptors, as for ``hpass_bgcopy``: the rows are then
        those descriptors' items, by ascending item index."""
        alpha_min = _check_alpha_min(alpha_min)
        i0, n = items if items is not None else (0, len(self.plan.descs))
        if n <= 0:
            return np.zeros((0, 4), np.int32)
        return self._bboxes_by_item(self._launch_bboxes(alpha_min, i0, n), i0, n)

    def _launch_bboxes(self, alpha_min: int, i0: int, n: int) -> torch.Tensor:
        """Queue ipp_pipe_overlay_bbox for descriptors [i0, i0 + n): the device
        int32 boxes, in descriptor order."""
        alpha_min = _check_alpha_min(alpha_min)
        if not self._hpass_done:
            raise N.NativeError("PipeRunner.overlay_bboxes: no H launch (hpass_bgcopy) has run on this runner")
        p = self.plan
        bbox = torch.empty(4 * max(n, 0), dtype=torch.int32, device=self.device)
        N.check(self.lib.ipp_pipe_overlay_bbox(self.tmp.data_ptr(), self.coefs.data_ptr(),
                                               self.descs.data_ptr() + i0 * p.descs.itemsize, n, p.max_ov_w,
                                               p.max_ov_h, alpha_min, p.tap_format, bbox.data_ptr(),
                                               _stream(self.device)), "ipp_pipe_overlay_bbox")
        return bbox

    def _bboxes_by_item(self, bbox: torch.Tensor, i0: int, n: int) -> np.ndarray:
        """Copy the boxes back (synchronises) and order them by item index."""
        by_desc = bbox.cpu().numpy().reshape(-1, 4)
        # descriptor i0 + k holds item order[i0 + k]: row = its rank among the range's items
        rank = np.argsort(np.argsort(self.plan.order[i0:i0 + n], kind="stable"), kind="stable")
        out = np.empty_like(by_desc)
        out[rank] = by_desc
        return out

    def vblend_bands(self, bgs: torch.Tensor, out: torch.Tensor, items=None) -> None:
        """V pass + paste over the 16-row bands the overlay touches (split form)."""
        p = self.plan
        i0, n = items if items is not None else (0, len(p.descs))
        _launch_vblend_bands(self.lib, p, self.tmp.data_ptr(), bgs.data_ptr(), out.data_ptr(), self.coefs.data_ptr(),
                             self.descs.data_ptr() + i0 * p.descs.itemsize, n, _stream(self.device))

    def run_overlapped(self, src: torch.Tensor, bgs: torch.Tensor, out: torch.Tensor, parts: int,
                       ratio: float = 1.0) -> None:
        """The batch in `parts` consecutive item ranges: the H launch of range k+1
        runs on the caller's stream while the V launch of range k runs on a
        side stream (event-ordered after its own H launch), so the V pass's
        HBM streaming overlaps the texture-bound H pass.  The ranges are whole
        copy groups of the H launch; the caller's stream waits for the last V
        launch."""
        self._check_tensors("run_overlapped", src, bgs, out)
        bounds = overlap_bounds(len(self.plan.descs), parts, ratio)
        main = torch.cuda.current_stream(self.device)
        if getattr(self, "_vstream", None) is None:
            self._vstream = torch.cuda.Stream(self.device)
            self._events = []
        side = self._vstream
        while len(self._events) < parts:
            self._events.append(torch.cuda.Event())
        side.wait_stream(main)  # inputs and tmp reuse ordered after the caller's work
        for k in range(parts):
            i0, i1 = bounds[k], bounds[k + 1]
            if i1 <= i0:
                continue
            self.hpass_bgcopy(src, bgs, out, items=(i0, i1 - i0))
            ev = self._events[k]
            ev.record(main)
            side.wait_event(ev)
            with torch.cuda.stream(side):
                self.vblend_bands(bgs, out, items=(i0, i1 - i0))
        main.wait_stream(side)

    def status(self) -> int:
        """Sticky status of the pipe kernels since the last call (ipp_pipe_status;
        bit 0: an H tile's window exceeded the LDS ring).  Synchronises."""
        return _pipe_status(self.lib, self.device)

    @property
    def split(self) -> bool:
        return self.plan.tap_format == N.IPP_TAPS_MFMA

    def run(self, src: torch.Tensor, bgs: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
        self._check_tensors("run", src, bgs, out)
        if not self.split:
            raise N.NativeError(f"PipeRunner.run: tap format {self.plan.tap_format} (the pipe takes IPP_TAPS_MFMA)")
        self.hpass_bgcopy(src, bgs, out)
        self.vblend_bands(bgs, out)
        return out

    def run_labelled(self, src: torch.Tensor, bgs: torch.Tensor, out: torch.Tensor, tight: bool = True,
                     alpha_min: int = 1, class_id: int = 0) -> Tuple[torch.Tensor, List[Optional[str]]]:
        """``run`` plus the YOLO label of every composite (``yolo_labels``),
        in item order: H launch, box launch, V launch on the current stream.
        ``tight=True``: the box of the overlay pixels with alpha >= alpha_min
        (``overlay_bboxes``), None for an invisible overlay; ``tight=False``:
        the reference's rectangle labels, nothing extra is launched."""
        self._check_tensors("run_labelled", src, bgs, out)
        if not self.split:
            raise N.NativeError(f"PipeRunner.run_labelled: tap format {self.plan.tap_format} "
                                "(the pipe takes IPP_TAPS_MFMA)")
        if tight:
            alpha_min = _check_alpha_min(alpha_min)
        self.hpass_bgcopy(src, bgs, out)
        if not tight:
            self.vblend_bands(bgs, out)
            return out, yolo_labels(self.plan, class_id)
        # the V launch is queued before the boxes are copied back, so the
        # host's wait for them covers it too
        n = len(self.plan.descs)
        bbox = self._launch_bboxes(alpha_min, 0, n)
        self.vblend_bands(bgs, out)
        return out, yolo_labels(self.plan, class_id, self._bboxes_by_item(bbox, 0, n))


class PipeStream:
    """Streaming form of PipeRunner (bench.py --stream): every batch has its
    own plan, built while earlier batches run.  Worker threads run the host
    plans (ipp_plan_pipe_batch; ctypes drops the GIL) and device taps
    (ipp_pipe_plan_taps, one side stream per slot) of batches k+1 ..
    k+lookahead while batch k's two launches run on the pipe stream.  Device
    buffers live in `slots` (≥ lookahead + 1) sets used in turn; a set is
    refilled only after the batch that last used it has completed (its HIP
    event)."""

    def __init__(self, device, plan_fn, slots: int = 3, priority: bool = True, lookahead: int = 2):
        self.device = torch.device(device)
        self.plan_fn = plan_fn                  # batch index -> PipePlan
        self.lib = N.load()
        # batches k+1 .. k+lookahead are being planned while batch k runs
        # (each on its own worker thread and side stream): the tap planner of
        # one batch then has `lookahead` batch times to get its share of the
        # GPU beside the pipe
        self.lookahead = max(1, int(lookahead))
        slots = max(slots, self.lookahead + 1)
        # The pipe launches go to a high-priority stream (the hardware queue
        # dispatches its blocks first): the tap planner of the next batch, on
        # the default-priority side stream, then fills the CU slots the pipe
        # leaves free instead of displacing H-pass blocks.
        self.main = torch.cuda.Stream(self.device, priority=-1) if priority else None
        self.slots = [{"done": torch.cuda.Event(), "bufs": {}, "side": torch.cuda.Stream(self.device)}
                      for _ in range(max(2, slots))]
        self.timing: List[Tuple[float, float, int]] = []   # per batch: host plan ms, taps ms, host tiles
        self.events: List[Tuple[torch.cuda.Event, torch.cuda.Event]] = []

    def _buf(self, slot, name: str, nbytes: int) -> torch.Tensor:
        b = slot["bufs"].get(name)
        if b is None or b.numel() < nbytes:
            slot["bufs"][name] = None
            b = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=self.device)
            slot["bufs"][name] = b
        return b

    def _prepare(self, k: int, slot):
        t0 = time.perf_counter()
        plan = self.plan_fn(k)
        t1 = time.perf_counter()
        slot["done"].synchronize()              # the batch that used these buffers has finished
        bufs = {"descs": self._buf(slot, "descs", plan.descs.nbytes),
                "coefs": self._buf(slot, "coefs", 4 * (plan.coef_words + 4096)),
                "tmp": self._buf(slot, "tmp", plan.tmp_bytes),
                "scratch": self._buf(slot, "scratch", self.lib.ipp_pipe_taps_scratch_bytes(len(plan.axes)))}
        stats = np.zeros(2, np.int64)
        side = slot["side"]
        with torch.cuda.stream(side):
            bufs["descs"][:plan.descs.nbytes].copy_(torch.from_numpy(plan.descs.view(np.uint8)))
            N.check(self.lib.ipp_pipe_plan_taps(N.np_ptr(plan.axes), len(plan.axes), bufs["coefs"].data_ptr(),
                                                bufs["scratch"].data_ptr(), N.np_ptr(stats),
                                                side.cuda_stream), "ipp_pipe_plan_taps")
        if stats[1]:
            raise N.NativeError(f"ipp_pipe_plan_taps: device status {int(stats[1])}")
        t2 = time.perf_counter()
        return plan, bufs, ((t1 - t0) * 1e3, (t2 - t1) * 1e3, int(stats[0]))

    def run(self, n_batches: int, src: torch.Tensor, bgs: torch.Tensor, out: torch.Tensor, mark=None,
            record: bool = False) -> None:
        """Run batches 0 .. n_batches-1 (plan_fn(k) plans batch k).  `mark`
        (optional callable) is called right before batch `mark.at` is
        launched, with the pipeline primed (its plan ready, the following
        lookahead-1 plans in flight) — bench.py starts its clock there."""
        from concurrent.futures import ThreadPoolExecutor
        main = self.main if self.main is not None else torch.cuda.current_stream(self.device)
        if self.main is not None:
            self.main.wait_stream(torch.cuda.current_stream(self.device))  # inputs written on the caller's stream
        L, ns = self.lookahead, len(self.slots)
        with ThreadPoolExecutor(L) as ex:
            futs = {j: ex.submit(self._prepare, j, self.slots[j % ns]) for j in range(min(L, n_batches))}
            for k in range(n_batches):
                plan, b, tm = futs.pop(k).result()
                if mark is not None and k == mark.at:
                    mark()
                slot = self.slots[k % ns]
                if k + L < n_batches:
                    # its slot was last used by batch k + L - ns <= k - 1, whose
                    # completion event is already recorded
                    futs[k + L] = ex.submit(self._prepare, k + L, self.slots[(k + L) % ns])
                ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) if record else None
                if ev:
                    ev[0].record(main)
                _launch_hpass_bgcopy(self.lib, plan, src.data_ptr(), b["tmp"].data_ptr(), b["coefs"].data_ptr(),
                                     b["descs"].data_ptr(), len(plan.descs), bgs.data_ptr(), out.data_ptr(),
                                     main.cuda_stream)
                _launch_vblend_bands(self.lib, plan, b["tmp"].data_ptr(), bgs.data_ptr(), out.data_ptr(),
                                     b["coefs"].data_ptr(), b["descs"].data_ptr(), len(plan.descs), main.cuda_stream)
                if ev:
                    ev[1].record(main)
                    self.events.append(ev)
                slot["done"].record(main)
                self.timing.append(tm)
        if self.main is not None:
            torch.cuda.current_stream(self.device).wait_stream(self.main)  # outputs visible to the caller's stream


# ---------------------------------------------------------------------------
# Scenes: K overlays per composite, occlusion-aware labels (an addition: the
# reference pastes one overlay per composite).
# ---------------------------------------------------------------------------
def draw_scene_params(n_scenes_global: int, stop_scene: int, per_scene: int, src_hw: Tuple[int, int],
                      bg_hw: Tuple[int, int], n_bg: int, cfg: PipeConfig, seed) -> List[ItemParams]:
    """The seeded parameters of overlay items 0 .. stop_scene·per_scene - 1 of
    a batch of scenes: exactly ``draw_params``'s stream over n_scenes_global ·
    per_scene items (all angles, all symmetries, the background shuffle, then
    per item ratio, x, y); overlay item i = scene·per_scene + layer, and the
    background of item i is order[(i // per_scene) % n_bg], one per scene."""
    K = per_scene
    angles, syms, order, drawn = draw_params(n_scenes_global * K, stop_scene * K, src_hw, bg_hw, n_bg, cfg, seed)
    return [ItemParams(angles[i], syms[i], order[(i // K) % n_bg], drawn[i][0], drawn[i][1], drawn[i][2])
            for i in range(stop_scene * K)]


@dataclass
class ScenePlan:
    """A batch of S scenes of K overlays each.  Overlay item i = s·K + k
    (scene s, layer k; layer K-1 on top) is built from source image i.

    ``descs`` is layer-major: descriptors [k·S, (k+1)·S) are layer k's, each
    layer in the same scene order — scenes grouped by background (stable), so
    layer 0's grouped copy keeps its shared loads.  ``desc_item[d]`` is the
    overlay item of descriptor d (``pipe.order`` does not describe this
    order).  Every descriptor's ``p.dst_off`` is its scene's composite slot;
    layers >= 1 have ``p.bg_off = p.dst_off`` and ``p.bg_pitch = p.dst_pitch``
    (they blend in place).  With K = 1 the descriptors are ``plan_pipe``'s."""
    pipe: PipePlan               # the S·K overlay items (items, axes, hsv, totals)
    descs: np.ndarray            # PIPE_DESC[S·K], layer-major
    desc_item: np.ndarray        # int32[S·K]
    n_scenes: int
    per_scene: int
    copy_read_bytes: int = 0     # background bytes layer 0's grouped copy loads

    @property
    def items(self) -> np.ndarray:
        return self.pipe.items

    @property
    def axes(self) -> np.ndarray:
        return self.pipe.axes

    @property
    def params(self) -> List[ItemParams]:
        return self.pipe.params

    @property
    def bg_w(self) -> int:
        return self.pipe.bg_w

    @property
    def bg_h(self) -> int:
        return self.pipe.bg_h

    @property
    def scene_layer(self) -> np.ndarray:
        """int32 (S·K, 2): (scene, layer) of each descriptor."""
        return np.stack([self.desc_item // self.per_scene, self.desc_item % self.per_scene], axis=1).astype(np.int32)


def plan_scenes(src_hw: Tuple[int, int], n_scenes: int, per_scene: int, bg_hw: Tuple[int, int], n_bg: int,
                cfg: PipeConfig, seed: int = 0, src_pitch: Optional[int] = None,
                item_range: Optional[Tuple[int, int]] = None, n_scenes_global: Optional[int] = None,
                params: Optional[Sequence[ItemParams]] = None, n_threads: int = 0) -> ScenePlan:
    """Plan `n_scenes` scenes of `per_scene` overlays.  ``item_range`` and
    ``n_scenes_global`` count SCENES: a rank plans scenes [start, stop) of the
    global batch and sees the parameters a single process would
    (``draw_scene_params``).  ``params``: one ItemParams per overlay item
    (n_scenes·per_scene, scene-major), nothing is drawn; the items of a scene
    must name the same background.  With ``per_scene=1`` this is ``plan_pipe``
    with the same arguments."""
    K, S = per_scene, n_scenes
    if isinstance(K, bool) or not isinstance(K, (int, np.integer)) or K < 1:
        raise ValueError(f"per_scene {per_scene!r}: an integer >= 1")
    start, stop = item_range if item_range is not None else (0, S)
    if stop - start != S or start < 0 or S <= 0:
        raise ValueError(f"item_range {item_range} does not hold {S} scenes")
    sg = stop if n_scenes_global is None else n_scenes_global
    if sg < stop:
        raise ValueError(f"n_scenes_global {sg} < item_range stop {stop}")
    if params is not None:
        if len(params) != S * K:
            raise ValueError(f"{len(params)} ItemParams for {S} scenes of {K} overlays")
        for s in range(S):
            if len({int(q.bg_index) for q in params[s * K:(s + 1) * K]}) != 1:
                raise ValueError(f"scene {start + s}: its overlays name different backgrounds")
    if K == 1:
        pipe = plan_pipe(src_hw, S, bg_hw, n_bg, cfg, seed, src_pitch, (start, stop), sg, params, n_threads)
    else:
        given = params
        if given is None:
            given = draw_scene_params(sg, stop, K, src_hw, bg_hw, n_bg, cfg, seed)[start * K:]
        pipe = plan_pipe(src_hw, S * K, bg_hw, n_bg, cfg, seed, src_pitch, (start * K, stop * K), sg * K, given,
                         n_threads)
    # plan_pipe's descriptor d holds item pipe.order[d], with p.dst_off = the
    # item's own slot: re-point it at the scene's slot and reorder layer-major
    by_item = np.empty_like(pipe.descs)
    by_item[pipe.order] = pipe.descs
    slot = int(pipe.descs[0]["p"]["bg_h"]) * int(pipe.descs[0]["p"]["dst_pitch"])    # bytes of one composite
    scene_order = np.argsort(pipe.items["bg_index"][::K], kind="stable")             # scenes grouped by background
    desc_item = (scene_order[None, :] * K + np.arange(K)[:, None]).reshape(-1).astype(np.int32)
    descs = by_item[desc_item]
    descs["p"]["dst_off"] = (desc_item // K).astype(np.int64) * slot
    descs["p"]["bg_off"][S:] = descs["p"]["dst_off"][S:]
    descs["p"]["bg_pitch"][S:] = descs["p"]["dst_pitch"][S:]
    # one background load per run of same-background layer-0 descriptors in a copy group (IPP_PT_COPY_READS)
    bgi = pipe.items["bg_index"][desc_item[:S]]
    runs = sum(1 for d in range(S) if d % N.IPP_PIPE_COPY_GROUP == 0 or bgi[d] != bgi[d - 1])
    return ScenePlan(pipe, descs, desc_item, S, K, runs * 3 * pipe.bg_w * pipe.bg_h)


def _check_level(name: str, v) -> int:
    """alpha_min / cover_min: an integer in 1..255 (check_alpha_min's rule)."""
    try:
        return _check_alpha_min(v)
    except ValueError:
        raise ValueError(f"{name} {v!r}: an integer in 1..255") from None


def scene_labels(boxes: np.ndarray, bg_w: int, bg_h: int, class_ids=0, min_visible: float = 0.0) -> List[List[str]]:
    """YOLO lines of every scene from the (S, K, 6) rows (x0, y0, x1, y1, area,
    visible) of ``SceneRunner.scene_boxes``: labels[s] lists, in layer order,
    one line (``yolo_label``) per overlay with visible > 0 and visible / area
    >= min_visible; an empty list = an empty label file.  ``class_ids``: an
    int, or one int per overlay item (S·K, scene-major)."""
    boxes = np.asarray(boxes)
    if boxes.ndim != 3 or boxes.shape[2] != 6:
        raise ValueError(f"boxes of shape {boxes.shape}: (scenes, layers, 6) expected")
    S, K = boxes.shape[:2]
    if isinstance(class_ids, (int, np.integer)):
        ids = [int(class_ids)] * (S * K)
    else:
        ids = [int(c) for c in class_ids]
        if len(ids) != S * K:
            raise ValueError(f"{len(ids)} class ids for {S * K} overlays")
    out: List[List[str]] = []
    for s in range(S):
        lines = []
        for k in range(K):
            x0, y0, x1, y1, area, vis = (int(v) for v in boxes[s, k])
            if vis > 0 and vis >= min_visible * area:
                lines.append(yolo_label(ids[s * K + k], (x0, y0, x1, y1), bg_w, bg_h))
        out.append(lines)
    return out


def scene_map_pitch(bg_w: int) -> int:
    """Row pitch in bytes of a visibility map (``SceneRunner.scene_masks``): ⌈bg_w / 16⌉·16."""
    return (int(bg_w) + 15) // 16 * 16


# instance id of a visibility-map byte: 0 = nothing visible, else 1 + its topmost set bit
_INSTANCE_LUT = np.array([v.bit_length() for v in range(256)], np.uint8)


def instance_ids(vis_map):
    """Instance-id image of a visibility map (``SceneRunner.scene_masks``), a
    torch or numpy uint8 array of any shape: 0 where no overlay is visible,
    otherwise 1 + the topmost layer whose bit is set (1 + layer within the
    scene).  The result has the input's type, shape and device."""
    if isinstance(vis_map, torch.Tensor):
        if vis_map.dtype != torch.uint8:
            raise ValueError(f"instance_ids: a uint8 map expected, got {vis_map.dtype}")
        return torch.from_numpy(_INSTANCE_LUT).to(vis_map.device)[vis_map.long()]
    vis_map = np.asarray(vis_map)
    if vis_map.dtype != np.uint8:
        raise ValueError(f"instance_ids: a uint8 map expected, got {vis_map.dtype}")
    return _INSTANCE_LUT[vis_map]


def scene_instance_masks(vis_map, rows) -> List[List[Optional[np.ndarray]]]:
    """Per-overlay instance masks from a copied-back visibility map (S, bg_h,
    bg_w) and the (S, K, 6) rows of ``scene_boxes``: masks[s] lists, in layer
    order, the boolean array of bit k cropped to overlay k's box (y1 - y0, x1
    - x0), or None for an overlay without a visible pixel.  Host code; a
    device map is copied back first (synchronises)."""
    if isinstance(vis_map, torch.Tensor):
        vis_map = vis_map.cpu().numpy()
    vis_map, rows = np.asarray(vis_map), np.asarray(rows)
    if rows.ndim != 3 or rows.shape[2] != 6:
        raise ValueError(f"rows of shape {rows.shape}: (scenes, layers, 6) expected")
    S, K = rows.shape[:2]
    if vis_map.dtype != np.uint8 or vis_map.ndim != 3 or vis_map.shape[0] != S:
        raise ValueError(f"a uint8 map of {S} scenes (S, bg_h, bg_w) expected, got {vis_map.dtype} {vis_map.shape}")
    if K > N.IPP_SCENE_MAP_MAX_LAYERS:
        raise ValueError(f"{K} layers: a visibility map holds at most {N.IPP_SCENE_MAP_MAX_LAYERS}")
    out: List[List[Optional[np.ndarray]]] = []
    for s in range(S):
        masks: List[Optional[np.ndarray]] = []
        for k in range(K):
            x0, y0, x1, y1 = (int(v) for v in rows[s, k, :4])
            masks.append(None if x0 < 0 else ((vis_map[s, y0:y1, x0:x1] >> k) & 1).astype(bool))
        out.append(masks)
    return out


def scene_contour_capacity(plan) -> int:
    """Default ``max_edges`` of ``SceneRunner.scene_polygons``: 8·(max_ov_w +
    max_ov_h) rounded up to 256 — four times the 2(w + h) boundary edges of a
    monotone outline filling the largest overlay's box."""
    p = plan.pipe if hasattr(plan, "pipe") else plan
    return (8 * (int(p.max_ov_w) + int(p.max_ov_h)) + 255) // 256 * 256


SIMPLIFY_MAX_SIDE = 16384   # largest background side ipp_polygons_simplify takes (ipp.h: the overflow bounds)


def simplify_tolerance(eps) -> int:
    """``eps_q`` of ipp_polygons_simplify for a tolerance of `eps` pixels: a
    real number that is a multiple of 0.25 in 0.25..1024 (the rule works in
    exact quarter pixels).  Anything else raises ValueError."""
    if isinstance(eps, (bool, np.bool_)) or not isinstance(eps, (int, float, np.integer, np.floating)):
        raise ValueError(f"simplify tolerance {eps!r}: a real number of pixels expected")
    q = float(eps) * 4.0
    if not (q == q and 1.0 <= q <= 4096.0 and q == int(q)):
        raise ValueError(f"simplify tolerance {eps!r}: a multiple of 0.25 in 0.25..1024 pixels expected")
    return int(q)


def seg_label(class_id: int, poly, bg_w: int, bg_h: int) -> str:
    """One YOLO segmentation line for the (V, 2) lattice polygon `poly` on a
    bg_w×bg_h composite: the class, then x / bg_w and y / bg_h of every vertex,
    in the number format of ``yolo_label``."""
    poly = np.asarray(poly)
    if poly.ndim != 2 or poly.shape[1] != 2 or len(poly) < 3:
        raise ValueError(f"a polygon of shape {poly.shape}: (V >= 3, 2) expected")
    return " ".join([str(class_id)] + [f"{int(x) / bg_w:.6f} {int(y) / bg_h:.6f}" for x, y in poly])


def scene_seg_labels(polys, info, rows, bg_w: int, bg_h: int, class_ids=0, min_visible: float = 0.0) -> List[List[str]]:
    """YOLO segmentation lines of every scene from what
    ``SceneRunner.scene_polygons`` returns: labels[s] lists, in layer order,
    one line (``seg_label``) per overlay that ``scene_labels`` gives a line —
    visible > 0 and visible / area >= min_visible.  ``class_ids`` as there.
    An overlay that would get a line but overflowed ``max_edges`` (header
    flags bit 0) raises ValueError naming the ``max_edges`` it needs: a label
    is never dropped or truncated."""
    info, rows = np.asarray(info), np.asarray(rows)
    if rows.ndim != 3 or rows.shape[2] != 6:
        raise ValueError(f"rows of shape {rows.shape}: (scenes, layers, 6) expected")
    S, K = rows.shape[:2]
    if info.shape != (S, K, N.IPP_CONTOUR_HDR):
        raise ValueError(f"info of shape {info.shape}: ({S}, {K}, {N.IPP_CONTOUR_HDR}) expected")
    if len(polys) != S or any(len(p) != K for p in polys):
        raise ValueError(f"polys does not hold {S} scenes of {K} overlays")
    if isinstance(class_ids, (int, np.integer)):
        ids = [int(class_ids)] * (S * K)
    else:
        ids = [int(c) for c in class_ids]
        if len(ids) != S * K:
            raise ValueError(f"{len(ids)} class ids for {S * K} overlays")
    out: List[List[str]] = []
    for s in range(S):
        lines = []
        for k in range(K):
            area, vis = int(rows[s, k, 4]), int(rows[s, k, 5])
            if not (vis > 0 and vis >= min_visible * area):
                continue
            if int(info[s, k, 7]) & 1:
                raise ValueError(f"scene {s} layer {k}: its contour has {int(info[s, k, 0])} boundary edges, "
                                 f"scene_polygons needs max_edges >= {int(info[s, k, 0])}")
            if polys[s][k] is None:
                raise ValueError(f"scene {s} layer {k}: {vis} visible pixels but no polygon")
            lines.append(seg_label(ids[s * K + k], polys[s][k], bg_w, bg_h))
        out.append(lines)
    return out


class SceneRunner:
    """Device-resident scene plan + scratch for repeated runs of one batch:
    2 + K launches on the current stream (2 when K = 1, the pipe's own)."""

    def __init__(self, plan: ScenePlan, device):
        self.plan = plan
        self.device = torch.device(device)
        self.descs = _to_dev(plan.descs, self.device)
        self.coefs, self.host_tiles = plan_taps(plan.pipe, self.device)
        self.tmp = torch.empty(plan.pipe.tmp_bytes, dtype=torch.uint8, device=self.device)
        self.lib = N.load()
        self._hpass_done = False   # the H launches have filled tmp (scene_boxes needs it)
        self._scene_layer = None
        self._scratch = None
        self._contour_scratch = None   # (max_edges, buffer) of scene_polygons
        self._simplify_scratch = None  # buffer of scene_polygons(simplify=...), grown on demand

    def _check(self, caller: str, src: torch.Tensor, bgs: torch.Tensor, out: torch.Tensor) -> None:
        _check_gpu_u8("SceneRunner", caller, src, bgs, out)
        p, S, K = self.plan.pipe, self.plan.n_scenes, self.plan.per_scene
        if src.dim() < 1 or src.shape[0] != S * K:
            raise ValueError(f"SceneRunner.{caller}: src holds {src.shape[0] if src.dim() else 0} images, "
                             f"{S} scenes of {K} overlays take {S * K}")
        if tuple(out.shape) != (S, p.bg_h, p.bg_w, 3):
            raise ValueError(f"SceneRunner.{caller}: out of shape {tuple(out.shape)}, {S} composites "
                             f"({S}, {p.bg_h}, {p.bg_w}, 3) expected")
        if bgs.dim() != 4 or tuple(bgs.shape[1:]) != (p.bg_h, p.bg_w, 3) or \
                bgs.shape[0] <= int(p.items["bg_index"].max()):
            raise ValueError(f"SceneRunner.{caller}: bgs of shape {tuple(bgs.shape)} does not hold the plan's "
                             f"backgrounds (n, {p.bg_h}, {p.bg_w}, 3)")

    def _dptr(self, d0: int) -> int:
        return self.descs.data_ptr() + d0 * self.plan.descs.itemsize

    def run(self, src: torch.Tensor, bgs: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
        self._check("run", src, bgs, out)
        p, S, K = self.plan.pipe, self.plan.n_scenes, self.plan.per_scene
        st, lib = _stream(self.device), self.lib
        hsv = N.np_ptr(p.hsv)
        _launch_hpass_bgcopy(lib, p, src.data_ptr(), self.tmp.data_ptr(), self.coefs.data_ptr(), self._dptr(0), S,
                             bgs.data_ptr(), out.data_ptr(), st)
        if K > 1:
            N.check(lib.ipp_pipe_hpass(src.data_ptr(), self.tmp.data_ptr(), self.coefs.data_ptr(), self._dptr(S),
                                       S * (K - 1), p.max_out_w, p.max_rows, 3, hsv, p.tap_format, st),
                    "ipp_pipe_hpass")
        self._hpass_done = True
        _launch_vblend_bands(lib, p, self.tmp.data_ptr(), bgs.data_ptr(), out.data_ptr(), self.coefs.data_ptr(),
                             self._dptr(0), S, st)
        # one launch per later layer: two overlays of a scene never share a launch (ipp.h)
        for k in range(1, K):
            N.check(lib.ipp_pipe_vblend_over(self.tmp.data_ptr(), out.data_ptr(), self.coefs.data_ptr(),
                                             self._dptr(k * S), S, p.bg_w, p.bg_h, p.max_ov_w, p.max_ov_h,
                                             p.tap_format, st), "ipp_pipe_vblend_over")
        return out

    def status(self) -> int:
        """Sticky status of the pipe kernels since the last call (``PipeRunner.status``).  Synchronises."""
        return _pipe_status(self.lib, self.device)

    def _scene_scratch(self, caller: str) -> None:
        """The guard and the (once allocated) scratch shared by the label and the map launches."""
        if not self._hpass_done:
            raise N.NativeError(f"SceneRunner.{caller}: no H launch (run) has run on this runner")
        if self._scratch is None:
            p, S, K = self.plan.pipe, self.plan.n_scenes, self.plan.per_scene
            nb = self.lib.ipp_pipe_scene_scratch_bytes(S * K, S, K, p.max_ov_w, p.max_ov_h)
            if nb < 0:
                raise N.NativeError(f"ipp_pipe_scene_scratch_bytes failed with code {nb}")
            self._scratch = torch.empty(int(nb), dtype=torch.uint8, device=self.device)
            self._scene_layer = _to_dev(self.plan.scene_layer, self.device)

    def _launch_boxes(self, alpha_min: int, cover_min: int) -> torch.Tensor:
        self._scene_scratch("scene_boxes")
        p, S, K = self.plan.pipe, self.plan.n_scenes, self.plan.per_scene
        n = S * K
        rows = torch.empty(6 * n, dtype=torch.int32, device=self.device)
        N.check(self.lib.ipp_pipe_scene_boxes(self.tmp.data_ptr(), self.coefs.data_ptr(), self._dptr(0),
                                              self._scene_layer.data_ptr(), n, S, K, p.max_ov_w, p.max_ov_h,
                                              alpha_min, cover_min, p.tap_format, self._scratch.data_ptr(),
                                              rows.data_ptr(), _stream(self.device)), "ipp_pipe_scene_boxes")
        return rows

    def _check_map(self, caller: str, out: Optional[torch.Tensor]) -> None:
        """Everything ``scene_masks`` refuses with ValueError, before any launch."""
        p, S, K = self.plan.pipe, self.plan.n_scenes, self.plan.per_scene
        if K > N.IPP_SCENE_MAP_MAX_LAYERS:
            raise ValueError(f"SceneRunner.{caller}: {K} layers per scene, a visibility map holds at most "
                             f"{N.IPP_SCENE_MAP_MAX_LAYERS} (one bit per layer)")
        if out is None:
            return
        shape = (S, p.bg_h, scene_map_pitch(p.bg_w))
        same_dev = isinstance(out, torch.Tensor) and out.device.type == self.device.type and \
            self.device.index in (None, out.device.index)
        if not same_dev or out.dtype != torch.uint8 or tuple(out.shape) != shape or not out.is_contiguous() or \
                out.data_ptr() % 16:
            raise ValueError(f"SceneRunner.{caller}: out must be a contiguous uint8 tensor {shape} on {self.device}, "
                             f"16-B aligned (the row pitch is scene_map_pitch(bg_w))")

    def _launch_map(self, caller: str, alpha_min: int, cover_min: int, with_boxes: bool,
                    out: Optional[torch.Tensor]) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        """One ipp_pipe_scene_map call: the (S, bg_h, pitch) map buffer and, with
        ``with_boxes``, the device rows in descriptor order."""
        self._scene_scratch(caller)
        p, S, K = self.plan.pipe, self.plan.n_scenes, self.plan.per_scene
        n, pitch = S * K, scene_map_pitch(p.bg_w)
        buf = out if out is not None else torch.empty((S, p.bg_h, pitch), dtype=torch.uint8, device=self.device)
        rows = torch.empty(6 * n, dtype=torch.int32, device=self.device) if with_boxes else None
        N.check(self.lib.ipp_pipe_scene_map(self.tmp.data_ptr(), self.coefs.data_ptr(), self._dptr(0),
                                            self._scene_layer.data_ptr(), n, S, K, p.bg_w, p.bg_h, p.max_ov_w,
                                            p.max_ov_h, alpha_min, cover_min, p.tap_format, self._scratch.data_ptr(),
                                            rows.data_ptr() if with_boxes else None, buf.data_ptr(), pitch,
                                            _stream(self.device)), "ipp_pipe_scene_map")
        return buf, rows

    def _rows_by_scene(self, rows: torch.Tensor) -> np.ndarray:
        """Copy the rows back (synchronises): (S, K, 6) in scene, layer order."""
        by_desc = rows.cpu().numpy().reshape(-1, 6)
        out = np.empty_like(by_desc)
        out[self.plan.desc_item] = by_desc
        return out.reshape(self.plan.n_scenes, self.plan.per_scene, 6)

    def scene_boxes(self, alpha_min: int = 1, cover_min: int = 128) -> np.ndarray:
        """(S, K, 6) int32 rows (x0, y0, x1, y1, area, visible) in scene, layer
        order (ipp_pipe_scene_boxes): the half-open tight box, in composite
        coordinates, of the overlay's visible pixels — alpha >= alpha_min and
        not covered by a later layer's alpha >= cover_min — or (-1,-1,-1,-1);
        area = pixels with alpha >= alpha_min, visible = the visible ones.  It
        reads the H launches' scratch, so it runs after ``run`` on the current
        stream, and synchronises for the copy back."""
        alpha_min, cover_min = _check_level("alpha_min", alpha_min), _check_level("cover_min", cover_min)
        return self._rows_by_scene(self._launch_boxes(alpha_min, cover_min))

    def scene_masks(self, alpha_min: int = 1, cover_min: int = 128, with_boxes: bool = False,
                    out: Optional[torch.Tensor] = None):
        """The visibility maps of the batch (ipp_pipe_scene_map): a device uint8
        tensor (S, bg_h, bg_w) in scene order (slot s belongs to composite
        ``out[s]`` of ``run``), bit k of a byte set iff layer k of the scene is
        visible at that pixel — alpha >= alpha_min and no later layer with alpha
        >= cover_min there, the rule of ``scene_boxes``.  A byte may hold
        several bits (``instance_ids`` keeps the topmost).  It is a view of an
        (S, bg_h, pitch) buffer, pitch = ``scene_map_pitch(bg_w)``, whose padding
        columns are 0; ``out`` supplies that buffer (contiguous CUDA uint8, any
        contents: every byte is written).  It runs after ``run`` on the current
        stream, stays on the device and does not synchronise.  With
        ``with_boxes`` it returns (map, rows), rows = the (S, K, 6) array of
        ``scene_boxes`` from the same alpha pass; that copy back synchronises.
        Scenes of more than 8 layers are refused (ValueError)."""
        alpha_min, cover_min = _check_level("alpha_min", alpha_min), _check_level("cover_min", cover_min)
        self._check_map("scene_masks", out)
        buf, rows = self._launch_map("scene_masks", alpha_min, cover_min, with_boxes, out)
        vis = buf[:, :, :self.plan.bg_w]
        return (vis, self._rows_by_scene(rows)) if with_boxes else vis

    def _check_max_edges(self, caller: str, max_edges) -> int:
        if max_edges is None:
            return scene_contour_capacity(self.plan)
        if isinstance(max_edges, bool) or not isinstance(max_edges, (int, np.integer)) or \
                not 4 <= max_edges <= 1 << 22:
            raise ValueError(f"SceneRunner.{caller}: max_edges {max_edges!r}: an integer in 4..2^22")
        return int(max_edges)

    def _check_simplify(self, caller: str, simplify) -> Optional[int]:
        """``eps_q`` of a ``simplify`` tolerance (None: no simplification), refusing what the device would."""
        if simplify is None:
            return None
        eps_q = simplify_tolerance(simplify)
        p = self.plan.pipe
        if p.bg_w > SIMPLIFY_MAX_SIDE or p.bg_h > SIMPLIFY_MAX_SIDE:
            raise ValueError(f"SceneRunner.{caller}: simplify on a {p.bg_w}x{p.bg_h} background: bg_w and bg_h must "
                             f"not exceed {SIMPLIFY_MAX_SIDE} (ipp_polygons_simplify's exact integer bounds)")
        return eps_q

    def _polygons(self, buf: torch.Tensor, rows: torch.Tensor, max_edges: int, eps_q: Optional[int] = None):
        """The tracer, the header copy-back, the pack and the packed copy-back
        on the map and device rows of one ``_launch_map``: (polys, info), both
        in scene, layer order.  Synchronises.  With ``eps_q`` the packed
        vertices stay on the device: ipp_polygons_simplify, the counts'
        copy-back, ipp_polygons_simplify_pack, and only the kept vertices
        come back."""
        p, S, K = self.plan.pipe, self.plan.n_scenes, self.plan.per_scene
        n, lib, st = S * K, self.lib, _stream(self.device)
        if self._contour_scratch is None or self._contour_scratch[0] != max_edges:
            nb = lib.ipp_scene_contours_scratch_bytes(n, max_edges)
            if nb < 0:
                raise N.NativeError(f"ipp_scene_contours_scratch_bytes failed with code {nb}")
            self._contour_scratch = (max_edges, torch.empty(int(nb), dtype=torch.uint8, device=self.device))
        scratch = self._contour_scratch[1]
        hdr = torch.empty(N.IPP_CONTOUR_HDR * n, dtype=torch.int32, device=self.device)
        N.check(lib.ipp_scene_contours(buf.data_ptr(), buf.shape[2], p.bg_w, p.bg_h, rows.data_ptr(),
                                       self._scene_layer.data_ptr(), n, S, K, max_edges, scratch.data_ptr(),
                                       hdr.data_ptr(), st), "ipp_scene_contours")
        by_desc = hdr.cpu().numpy().reshape(n, N.IPP_CONTOUR_HDR)      # synchronises
        nv = by_desc[:, 3].astype(np.int64)
        offsets = np.concatenate([[0], np.cumsum(nv)[:-1]]).astype(np.int64)
        total = int(nv.sum())
        packed = np.empty((0, 2), np.int32)
        if total:
            verts = torch.empty(2 * total, dtype=torch.int32, device=self.device)
            N.check(lib.ipp_scene_contours_pack(scratch.data_ptr(), hdr.data_ptr(),
                                                _to_dev(offsets, self.device).data_ptr(), n, max_edges,
                                                verts.data_ptr(), st), "ipp_scene_contours_pack")
            if eps_q is None:
                packed = verts.cpu().numpy().reshape(total, 2)
            else:
                nv, offsets, packed = self._simplified(verts, offsets, hdr, total, eps_q)
        info = np.empty_like(by_desc)
        info[self.plan.desc_item] = by_desc
        polys: List[List[Optional[np.ndarray]]] = [[None] * K for _ in range(S)]
        for d, item in enumerate(self.plan.desc_item.tolist()):
            if nv[d]:
                polys[item // K][item % K] = packed[offsets[d]:offsets[d] + nv[d]].copy()
        return polys, info.reshape(S, K, N.IPP_CONTOUR_HDR)

    def _simplified(self, verts: torch.Tensor, offsets: np.ndarray, hdr: torch.Tensor, total: int, eps_q: int):
        """(counts, out_offsets, kept vertices (sum counts, 2)) of the packed device polygons."""
        p, lib, st = self.plan.pipe, self.lib, _stream(self.device)
        n = self.plan.n_scenes * self.plan.per_scene
        nb = lib.ipp_polygons_simplify_scratch_bytes(n, total)
        if nb < 0:
            raise N.NativeError(f"ipp_polygons_simplify_scratch_bytes failed with code {nb}")
        if self._simplify_scratch is None or self._simplify_scratch.numel() < nb:
            self._simplify_scratch = torch.empty(int(nb), dtype=torch.uint8, device=self.device)
        scratch = self._simplify_scratch
        d_off = _to_dev(offsets, self.device)
        counts = torch.empty(n, dtype=torch.int32, device=self.device)
        N.check(lib.ipp_polygons_simplify(verts.data_ptr(), d_off.data_ptr(), hdr.data_ptr(), n, total, p.bg_w,
                                          p.bg_h, eps_q, scratch.data_ptr(), counts.data_ptr(), st),
                "ipp_polygons_simplify")
        kept = counts.cpu().numpy().astype(np.int64)                   # synchronises
        out_offsets = np.concatenate([[0], np.cumsum(kept)[:-1]]).astype(np.int64)
        total_kept = int(kept.sum())
        out = torch.empty(2 * max(total_kept, 1), dtype=torch.int32, device=self.device)
        N.check(lib.ipp_polygons_simplify_pack(verts.data_ptr(), d_off.data_ptr(), hdr.data_ptr(), scratch.data_ptr(),
                                               counts.data_ptr(), _to_dev(out_offsets, self.device).data_ptr(), n,
                                               out.data_ptr(), st), "ipp_polygons_simplify_pack")
        return kept, out_offsets, out[:2 * total_kept].cpu().numpy().reshape(total_kept, 2)

    def scene_polygons(self, alpha_min: int = 1, cover_min: int = 128, max_edges: Optional[int] = None,
                       simplify: Optional[float] = None):
        """The outer contour of every overlay's visible pixels, traced on the
        device from the visibility map (ipp_pipe_scene_map with boxes, then
        ipp_scene_contours and ipp_scene_contours_pack; include/ipp.h states
        the contour's definition).  Returns (polys, info, rows): polys[s][k] is
        the (V, 2) int32 polygon of scene s, layer k in composite lattice
        coordinates — the largest 8-connected visible part's outline, holes
        not cut out — or None when the overlay has no visible pixel or has
        more boundary edges than ``max_edges`` (default
        ``scene_contour_capacity(plan)``); info is the (S, K, 8) headers
        {n_edges, n_outer, n_holes, n_vertices, area2, start_x, start_y,
        flags}, flags bit 0 = overflowed; rows is ``scene_boxes``' (S, K, 6)
        from the same alpha pass.  Runs after ``run`` on the current stream;
        only the headers and the packed vertices are copied back (it
        synchronises).  Scenes of more than 8 layers are refused.  With
        ``simplify`` = a tolerance in pixels (``simplify_tolerance``: a
        multiple of 0.25) the polygons are simplified on the device by the
        Douglas–Peucker rule of include/ipp.h (ipp_polygons_simplify): polys
        holds the kept vertices, at least 3 each, info and rows are unchanged
        (n_vertices stays the traced count), and the unsimplified vertices
        never leave the device — the counts and the kept vertices do.
        Backgrounds of more than 16384 pixels on a side are then refused."""
        alpha_min, cover_min = _check_level("alpha_min", alpha_min), _check_level("cover_min", cover_min)
        self._check_map("scene_polygons", None)
        max_edges = self._check_max_edges("scene_polygons", max_edges)
        eps_q = self._check_simplify("scene_polygons", simplify)
        buf, rows = self._launch_map("scene_polygons", alpha_min, cover_min, True, None)
        polys, info = self._polygons(buf, rows, max_edges, eps_q)
        return polys, info, self._rows_by_scene(rows)

    def run_labelled(self, src: torch.Tensor, bgs: torch.Tensor, out: torch.Tensor, class_ids=0,
                     alpha_min: int = 1, cover_min: int = 128, min_visible: float = 0.0, masks: bool = False,
                     polygons: bool = False, max_edges: Optional[int] = None, simplify: Optional[float] = None):
        """``run`` plus the YOLO lines of every scene (``scene_labels``):
        labels[s] lists scene s's lines in layer order, one per overlay with
        visible > 0 and visible / area >= min_visible.  Returns (out, labels);
        with ``masks`` (out, labels, map), the map of ``scene_masks`` from the
        same launch as the boxes.  With ``polygons`` the tuple gains, as its
        last element, the segmentation lines of ``scene_seg_labels`` (polygons
        of ``scene_polygons`` with ``max_edges`` and ``simplify``), traced from
        that same map launch.  ``simplify`` without ``polygons`` is refused."""
        alpha_min, cover_min = _check_level("alpha_min", alpha_min), _check_level("cover_min", cover_min)
        if simplify is not None and not polygons:
            raise ValueError("SceneRunner.run_labelled: simplify needs polygons=True")
        if masks or polygons:
            self._check_map("run_labelled", None)
        eps_q = None
        if polygons:
            max_edges = self._check_max_edges("run_labelled", max_edges)
            eps_q = self._check_simplify("run_labelled", simplify)
        self.run(src, bgs, out)
        if masks or polygons:
            buf, rows = self._launch_map("run_labelled", alpha_min, cover_min, True, None)
            boxes = self._rows_by_scene(rows)
            labels = scene_labels(boxes, self.plan.bg_w, self.plan.bg_h, class_ids, min_visible)
            res = (out, labels) + ((buf[:, :, :self.plan.bg_w],) if masks else ())
            if polygons:
                polys, info = self._polygons(buf, rows, max_edges, eps_q)
                res += (scene_seg_labels(polys, info, boxes, self.plan.bg_w, self.plan.bg_h, class_ids, min_visible),)
            return res
        boxes = self._rows_by_scene(self._launch_boxes(alpha_min, cover_min))
        return out, scene_labels(boxes, self.plan.bg_w, self.plan.bg_h, class_ids, min_visible)
