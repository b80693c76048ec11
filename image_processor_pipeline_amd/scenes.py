"""Scenes: K overlays per composite in the batched pipe, with occlusion-aware
labels (an addition: the reference pastes one overlay per composite).

``plan_scenes`` / ``SceneRunner`` paste the overlays in layer order — layer 0
as the pipe of fused.py does, every later layer by an H launch without the
copy (``ipp_pipe_hpass``) and an in-place V launch (``ipp_pipe_vblend_over``)
— and label each overlay by what no later layer covers (``scene_boxes``).
``scene_masks`` keeps that rule's per-pixel answer, one visibility map per
composite, and ``scene_polygons`` traces (and simplifies) each overlay's outer
contour from it on the device; ``scene_obbs`` reduces that contour there to its
minimum-area rectangle (YOLO-OBB), and ``scene_rles`` run-length encodes each
overlay's exact visible mask there (COCO RLE).  ``run_culled`` decides on the
device, between the H and the V launches, which overlays the later layers leave
too little of, and pastes only the others.  ``scene_amodal`` reports what the
rule hides: each overlay's full box and mask behind its occluders and the
pairwise occlusion counts (``scene_amodal_rles``, ``scene_amodal_polygons``,
``run_labelled(amodal=True)``).  ``feed`` / ``run_feed`` leave a training
batch on the device instead — normalised planar images, a targets tensor, an
instance-index map — with no copy back, at the composites' size or, with
``size``, resized on the device exactly as Pillow would.  labels_fmt.py formats the lines,
masks and annotations; every public name here is also reachable as ``fused.X``.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _native as N
from . import geometry as G
from .device import _stream, _to_dev, exclusive_offsets
from .device import check_alpha_min as _check_alpha_min
from .fused import (ItemParams, PipeConfig, PipePlan, _launch_hpass_bgcopy, _launch_vblend_bands, _Runner,
                    draw_params, plan_pipe)
from .labels_fmt import (FEED_RESAMPLE, Letterbox, feed_lut, letterbox_geometry, min_visible_q,  # noqa: F401
                         scene_amodal_annotations, scene_coco_annotations, scene_contour_capacity, scene_labels,
                         scene_map_pitch, scene_obb_labels, scene_seg_labels, simplify_tolerance)


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

    # read through to the overlay items' plan
    items = property(lambda self: self.pipe.items)
    axes = property(lambda self: self.pipe.axes)
    params = property(lambda self: self.pipe.params)
    bg_w = property(lambda self: self.pipe.bg_w)
    bg_h = property(lambda self: self.pipe.bg_h)

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


class SceneFeed(NamedTuple):
    """What ``SceneRunner.feed`` leaves on the device (include/ipp.h states the rules)."""
    images: torch.Tensor                 # (S, 3, bg_h, bg_w) of the table's dtype; (S, 3, out_h, out_w) with size (with
    #                                      letterbox the canvas of letterbox_geometry((bg_h, bg_w), size, scaleup, center))
    targets: torch.Tensor                # (S·K, 6) float32 (scene, class, cx, cy, w, h); unused rows all -1
    count: torch.Tensor                  # (1,) int32: the rows in use
    slot: torch.Tensor                   # (S, K) int32: each overlay's row of targets, or -1
    index_map: Optional[torch.Tensor]    # (S, bg_h, bg_w) uint8 ((S, out_h, out_w) with size), or None


_FEED_DTYPES = (torch.float16, torch.bfloat16, torch.float32)

SIMPLIFY_MAX_SIDE = 16384   # largest background side ipp_polygons_simplify takes (ipp.h: the overflow bounds)


class SceneRunner(_Runner):
    """Device-resident scene plan + scratch for repeated runs of one batch:
    2 + K launches on the current stream (2 when K = 1, the pipe's own)."""

    _scene_layer = _scratch = None   # of the label and map launches; these four are allocated on first use
    _contour_scratch = None          # (max_edges, buffer) of scene_polygons
    _simplify_scratch = None         # buffer of scene_polygons(simplify=...), grown on demand
    _obb_scratch = None              # buffer of scene_obbs, grown on demand
    _rle_scratch = None              # buffer of scene_rles
    _feed_cache = None               # the small device arrays of feed, by argument

    def _check(self, caller: str, src: torch.Tensor, bgs: torch.Tensor, out: torch.Tensor) -> None:
        self._check_tensors(caller, src, bgs, out)
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

    def _launch_h(self, src: torch.Tensor, bgs: torch.Tensor, out: torch.Tensor) -> None:
        """The H launches of the batch: layer 0 with the background copy, the later layers in one launch."""
        p, S, K = self.plan.pipe, self.plan.n_scenes, self.plan.per_scene
        st, lib = _stream(self.device), self.lib
        _launch_hpass_bgcopy(lib, p, src.data_ptr(), self.tmp.data_ptr(), self.coefs.data_ptr(), self._dptr(0), S,
                             bgs.data_ptr(), out.data_ptr(), st)
        if K > 1:
            N.check(lib.ipp_pipe_hpass(src.data_ptr(), self.tmp.data_ptr(), self.coefs.data_ptr(), self._dptr(S),
                                       S * (K - 1), p.max_out_w, p.max_rows, 3, N.np_ptr(p.hsv), p.tap_format, st),
                    "ipp_pipe_hpass")
        self._hpass_done = True

    def _launch_v(self, bgs: torch.Tensor, out: torch.Tensor) -> None:
        """The V launches: layer 0's, then one in-place launch per later layer."""
        p, S, K = self.plan.pipe, self.plan.n_scenes, self.plan.per_scene
        st, lib = _stream(self.device), self.lib
        _launch_vblend_bands(lib, p, self.tmp.data_ptr(), bgs.data_ptr(), out.data_ptr(), self.coefs.data_ptr(),
                             self._dptr(0), S, st)
        # one launch per later layer: two overlays of a scene never share a launch (ipp.h)
        for k in range(1, K):
            N.check(lib.ipp_pipe_vblend_over(self.tmp.data_ptr(), out.data_ptr(), self.coefs.data_ptr(),
                                             self._dptr(k * S), S, p.bg_w, p.bg_h, p.max_ov_w, p.max_ov_h,
                                             p.tap_format, st), "ipp_pipe_vblend_over")

    def run(self, src: torch.Tensor, bgs: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
        self._check("run", src, bgs, out)
        self._launch_h(src, bgs, out)
        self._launch_v(bgs, out)
        return out

    @staticmethod
    def _check_cull(caller: str, min_visible, min_pixels) -> Tuple[int, int]:
        """(min_q, min_pixels) of a cull, refusing what ipp_pipe_scene_cull would."""
        min_q = min_visible_q(min_visible)
        if isinstance(min_pixels, (bool, np.bool_)) or not isinstance(min_pixels, (int, np.integer)) or \
                not 0 <= min_pixels < 1 << 31:
            raise ValueError(f"SceneRunner.{caller}: min_pixels {min_pixels!r}: an integer >= 0 (below 2^31)")
        return min_q, int(min_pixels)

    def _launch_cull(self, caller: str, alpha_min: int, cover_min: int, min_q: int, min_pixels: int) -> torch.Tensor:
        """ipp_pipe_scene_cull between the H and the V launches: the device records, 4 int32 per descriptor."""
        self._scene_scratch(caller)
        p = self.plan.pipe
        rec = torch.empty(4 * len(self.plan.descs), dtype=torch.int32, device=self.device)
        N.check(self.lib.ipp_pipe_scene_cull(*self._scene_head(), p.max_ov_w, p.max_ov_h,
                                             alpha_min, cover_min, min_q, min_pixels, p.tap_format,
                                             self._scratch.data_ptr(), rec.data_ptr(), _stream(self.device)),
                "ipp_pipe_scene_cull")
        return rec

    def _cull_by_scene(self, rec: torch.Tensor) -> Tuple[np.ndarray, np.ndarray]:
        """Copy the cull records back (synchronises): kept (S, K) bool and stats (S, K, 2) int32, scene, layer order."""
        by_desc = rec.cpu().numpy().reshape(-1, 4)
        by_item = np.empty_like(by_desc)
        by_item[self.plan.desc_item] = by_desc
        by_item = by_item.reshape(self.plan.n_scenes, self.plan.per_scene, 4)
        return by_item[..., 0] != 0, np.ascontiguousarray(by_item[..., 1:3])

    def run_culled(self, src: torch.Tensor, bgs: torch.Tensor, out: torch.Tensor, alpha_min: int = 1,
                   cover_min: int = 128, min_visible: float = 0.0, min_pixels: int = 1):
        """``run`` without the overlays that the later layers leave too little
        of: the H launches, ipp_pipe_scene_cull, the V launches.  The layers of
        a scene are decided top down (include/ipp.h states the rule in
        integers): an overlay is kept iff, counting as ``scene_boxes`` does but
        against the KEPT later layers only, visible >= max(min_pixels, 1) and
        visible / area >= min_visible (``min_visible_q``).  A culled overlay is
        not pasted and hides nothing, so an overlay that only a culled one
        would hide is kept.  Returns (out, kept, stats): kept is an (S, K) bool
        array and stats (S, K, 2) int32 = (area, visible) at the moment of the
        decision, both in scene, layer order; that copy back synchronises.
        Every painted overlay then has a line in ``scene_labels`` at the same
        thresholds, and every line a painted overlay.

        The cull clears the culled overlays' part of the H launches' scratch:
        until the next ``run`` (or ``run_culled`` / ``run_labelled``) rewrites
        it in full, ``scene_boxes``, ``scene_masks``, ``scene_polygons``,
        ``scene_obbs`` and ``scene_rles`` on this runner report the culled
        overlays as absent — row (-1, -1, -1, -1, 0, 0), no bit in the map, no
        polygon, box or encoding — which is what the composite shows."""
        alpha_min, cover_min = _check_level("alpha_min", alpha_min), _check_level("cover_min", cover_min)
        min_q, min_pixels = self._check_cull("run_culled", min_visible, min_pixels)
        self._check("run_culled", src, bgs, out)
        self._launch_h(src, bgs, out)
        rec = self._launch_cull("run_culled", alpha_min, cover_min, min_q, min_pixels)
        self._launch_v(bgs, out)
        kept, stats = self._cull_by_scene(rec)
        return out, kept, stats

    def _scratch_bytes(self, entry: str, *args) -> int:
        """What the library's `entry` (a ``*_scratch_bytes`` function) asks for these arguments."""
        nb = getattr(self.lib, entry)(*args)
        if nb < 0:
            raise N.NativeError(f"{entry} failed with code {nb}")
        return int(nb)

    def _scene_scratch(self, caller: str) -> None:
        """The guard and the (once allocated) scratch shared by the label and the map launches."""
        if not self._hpass_done:
            raise N.NativeError(f"SceneRunner.{caller}: no H launch (run) has run on this runner")
        if self._scratch is None:
            p, S, K = self.plan.pipe, self.plan.n_scenes, self.plan.per_scene
            nb = self._scratch_bytes("ipp_pipe_scene_scratch_bytes", S * K, S, K, p.max_ov_w, p.max_ov_h)
            self._scratch = torch.empty(nb, dtype=torch.uint8, device=self.device)
            self._scene_layer = _to_dev(self.plan.scene_layer, self.device)

    def _scene_head(self) -> tuple:
        """The arguments every scene entry begins with: (tmp, coefs, descs, scene_layer, S·K, S, K)."""
        S, K = self.plan.n_scenes, self.plan.per_scene
        return (self.tmp.data_ptr(), self.coefs.data_ptr(), self._dptr(0), self._scene_layer.data_ptr(), S * K, S, K)

    def _rows(self) -> torch.Tensor:   # of one label or map launch: 6 int32 per descriptor
        return torch.empty(6 * len(self.plan.descs), dtype=torch.int32, device=self.device)

    def _launch_boxes(self, alpha_min: int, cover_min: int) -> torch.Tensor:
        self._scene_scratch("scene_boxes")
        p = self.plan.pipe
        rows = self._rows()
        N.check(self.lib.ipp_pipe_scene_boxes(*self._scene_head(), p.max_ov_w, p.max_ov_h, alpha_min, cover_min,
                                              p.tap_format, self._scratch.data_ptr(), rows.data_ptr(),
                                              _stream(self.device)), "ipp_pipe_scene_boxes")
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
        p, S = self.plan.pipe, self.plan.n_scenes
        pitch = scene_map_pitch(p.bg_w)
        buf = out if out is not None else torch.empty((S, p.bg_h, pitch), dtype=torch.uint8, device=self.device)
        rows = self._rows() if with_boxes else None
        N.check(self.lib.ipp_pipe_scene_map(*self._scene_head(), p.bg_w, p.bg_h, p.max_ov_w,
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

    def _check_obb(self, caller: str) -> None:
        """Refuse what ipp_polygons_obb would: a background side above 16384 (its exact integer bounds)."""
        p = self.plan.pipe
        if p.bg_w > SIMPLIFY_MAX_SIDE or p.bg_h > SIMPLIFY_MAX_SIDE:
            raise ValueError(f"SceneRunner.{caller}: oriented boxes on a {p.bg_w}x{p.bg_h} background: bg_w and bg_h "
                             f"must not exceed {SIMPLIFY_MAX_SIDE} (ipp_polygons_obb's exact integer bounds)")

    def _polygons(self, buf: torch.Tensor, rows: torch.Tensor, max_edges: int, eps_q: Optional[int] = None):
        """(polys, info) of ``_trace``: the polygons alone."""
        return self._trace(buf, rows, max_edges, eps_q)[:2]

    def _trace(self, buf: torch.Tensor, rows: torch.Tensor, max_edges: int, eps_q: Optional[int] = None,
               polygons: bool = True, obb: bool = False):
        """The tracer, the header copy-back, the pack and the packed copy-back
        on the map and device rows of one ``_launch_map``: (polys, info,
        obbs), all in scene, layer order.  Synchronises.  With ``eps_q`` the
        packed vertices stay on the device: ipp_polygons_simplify, the counts'
        copy-back, ipp_polygons_simplify_pack, and only the kept vertices
        come back.  With ``obb`` ipp_polygons_obb runs on the packed
        (unsimplified) vertices right after the pack and its (S, K, 8) records
        come back, else obbs is None; without ``polygons`` no vertex is copied
        back and polys is None."""
        p, S, K = self.plan.pipe, self.plan.n_scenes, self.plan.per_scene
        n, lib, st = S * K, self.lib, _stream(self.device)
        if self._contour_scratch is None or self._contour_scratch[0] != max_edges:
            nb = self._scratch_bytes("ipp_scene_contours_scratch_bytes", n, max_edges)
            self._contour_scratch = (max_edges, torch.empty(nb, dtype=torch.uint8, device=self.device))
        scratch = self._contour_scratch[1]
        hdr = torch.empty(N.IPP_CONTOUR_HDR * n, dtype=torch.int32, device=self.device)
        N.check(lib.ipp_scene_contours(buf.data_ptr(), buf.shape[2], p.bg_w, p.bg_h, rows.data_ptr(),
                                       self._scene_layer.data_ptr(), n, S, K, max_edges, scratch.data_ptr(),
                                       hdr.data_ptr(), st), "ipp_scene_contours")
        by_desc = hdr.cpu().numpy().reshape(n, N.IPP_CONTOUR_HDR)      # synchronises
        nv = by_desc[:, 3].astype(np.int64)
        offsets = exclusive_offsets(nv)
        total = int(nv.sum())
        packed = np.empty((0, 2), np.int32)
        d_obb = None
        if total:
            verts = torch.empty(2 * total, dtype=torch.int32, device=self.device)
            d_off = _to_dev(offsets, self.device)
            N.check(lib.ipp_scene_contours_pack(scratch.data_ptr(), hdr.data_ptr(), d_off.data_ptr(), n, max_edges,
                                                verts.data_ptr(), st), "ipp_scene_contours_pack")
            if obb:
                d_obb = self._launch_obb(verts, d_off, hdr, total)
            if polygons and eps_q is None:
                packed = verts.cpu().numpy().reshape(total, 2)
            elif polygons:
                nv, offsets, packed = self._simplified(verts, offsets, hdr, total, eps_q)
        info = np.empty_like(by_desc)
        info[self.plan.desc_item] = by_desc
        obbs = None
        if obb:     # no packed vertex at all: every header has n_vertices == 0, every record is the zero record
            rec = d_obb.cpu().numpy().reshape(n, N.IPP_OBB_REC) if d_obb is not None else \
                np.zeros((n, N.IPP_OBB_REC), np.int32)
            obbs = np.empty_like(rec)
            obbs[self.plan.desc_item] = rec
            obbs = obbs.reshape(S, K, N.IPP_OBB_REC)
        polys: Optional[List[List[Optional[np.ndarray]]]] = None
        if polygons:
            polys = [[None] * K for _ in range(S)]
            for d, item in enumerate(self.plan.desc_item.tolist()):
                if nv[d]:
                    polys[item // K][item % K] = packed[offsets[d]:offsets[d] + nv[d]].copy()
        return polys, info.reshape(S, K, N.IPP_CONTOUR_HDR), obbs

    def _launch_obb(self, verts: torch.Tensor, d_off: torch.Tensor, hdr: torch.Tensor, total: int) -> torch.Tensor:
        """ipp_polygons_obb on the packed device polygons: the device records, 8 int32 per descriptor."""
        p, n = self.plan.pipe, len(self.plan.descs)
        nb = max(self._scratch_bytes("ipp_polygons_obb_scratch_bytes", n, total), 16)
        if self._obb_scratch is None or self._obb_scratch.numel() < nb:
            self._obb_scratch = torch.empty(nb, dtype=torch.uint8, device=self.device)
        rec = torch.empty(N.IPP_OBB_REC * n, dtype=torch.int32, device=self.device)
        N.check(self.lib.ipp_polygons_obb(verts.data_ptr(), d_off.data_ptr(), hdr.data_ptr(), n, total, p.bg_w,
                                          p.bg_h, self._obb_scratch.data_ptr(), rec.data_ptr(),
                                          _stream(self.device)), "ipp_polygons_obb")
        return rec

    def _simplified(self, verts: torch.Tensor, offsets: np.ndarray, hdr: torch.Tensor, total: int, eps_q: int):
        """(counts, out_offsets, kept vertices (sum counts, 2)) of the packed device polygons."""
        p, lib, st = self.plan.pipe, self.lib, _stream(self.device)
        n = len(self.plan.descs)
        nb = self._scratch_bytes("ipp_polygons_simplify_scratch_bytes", n, total)
        if self._simplify_scratch is None or self._simplify_scratch.numel() < nb:
            self._simplify_scratch = torch.empty(nb, dtype=torch.uint8, device=self.device)
        scratch = self._simplify_scratch
        d_off = _to_dev(offsets, self.device)
        counts = torch.empty(n, dtype=torch.int32, device=self.device)
        N.check(lib.ipp_polygons_simplify(verts.data_ptr(), d_off.data_ptr(), hdr.data_ptr(), n, total, p.bg_w,
                                          p.bg_h, eps_q, scratch.data_ptr(), counts.data_ptr(), st),
                "ipp_polygons_simplify")
        kept = counts.cpu().numpy().astype(np.int64)                   # synchronises
        out_offsets = exclusive_offsets(kept)
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

    def scene_obbs(self, alpha_min: int = 1, cover_min: int = 128, max_edges: Optional[int] = None):
        """The oriented box (YOLO-OBB) of every overlay's visible pixels: the
        minimum-area rectangle around the outline that ``scene_polygons``
        traces (the largest 8-connected visible part, unsimplified), found on
        the device by the exact rule of include/ipp.h (ipp_polygons_obb after
        the map launch, the tracer and its pack).  Returns (obbs, info, rows):
        obbs is (S, K, 8) int32 in scene, layer order, one record {ax, ay, dx,
        dy, lo, hi, hgt, m} per overlay — ``obb_corners`` gives its corners,
        which are NOT clipped to the image: the rectangle of an overlay at the
        border may leave it slightly — and all zeros for an overlay without a
        visible pixel or one that overflowed ``max_edges``; info and rows are
        exactly ``scene_polygons``'.  Runs after ``run`` on the current stream
        and synchronises; the headers, the rows and 32 B per overlay come
        back, the packed vertices never leave the device.  Scenes of more than
        8 layers and backgrounds of more than 16384 pixels on a side are
        refused."""
        alpha_min, cover_min = _check_level("alpha_min", alpha_min), _check_level("cover_min", cover_min)
        self._check_map("scene_obbs", None)
        max_edges = self._check_max_edges("scene_obbs", max_edges)
        self._check_obb("scene_obbs")
        buf, rows = self._launch_map("scene_obbs", alpha_min, cover_min, True, None)
        _, info, obbs = self._trace(buf, rows, max_edges, None, polygons=False, obb=True)
        return obbs, info, self._rows_by_scene(rows)

    def _rles(self, buf: torch.Tensor, rows: torch.Tensor) -> List[List[Optional[np.ndarray]]]:
        """ipp_scene_rle, the header copy-back, ipp_scene_rle_pack and the
        packed copy-back on the map and device rows of one ``_launch_map``:
        rles[s][k] in scene, layer order.  Synchronises."""
        p, S, K = self.plan.pipe, self.plan.n_scenes, self.plan.per_scene
        n, lib, st = S * K, self.lib, _stream(self.device)
        if self._rle_scratch is None:
            nb = max(self._scratch_bytes("ipp_scene_rle_scratch_bytes", n, p.bg_w), 16)
            self._rle_scratch = torch.empty(nb, dtype=torch.uint8, device=self.device)
        scratch = self._rle_scratch
        hdr = torch.empty(N.IPP_RLE_HDR * n, dtype=torch.int32, device=self.device)
        args = (buf.data_ptr(), buf.shape[2], p.bg_w, p.bg_h, rows.data_ptr(), self._scene_layer.data_ptr(), n, S, K,
                scratch.data_ptr(), hdr.data_ptr())
        N.check(lib.ipp_scene_rle(*args, st), "ipp_scene_rle")
        nc = hdr.cpu().numpy().reshape(n, N.IPP_RLE_HDR)[:, 0].astype(np.int64)      # synchronises
        offsets = exclusive_offsets(nc)
        total = int(nc.sum())
        packed = np.empty(0, np.uint32)
        if total:
            counts = torch.empty(total, dtype=torch.int32, device=self.device)
            N.check(lib.ipp_scene_rle_pack(*args, _to_dev(offsets, self.device).data_ptr(), counts.data_ptr(), st),
                    "ipp_scene_rle_pack")
            packed = counts.cpu().numpy().view(np.uint32)
        rles: List[List[Optional[np.ndarray]]] = [[None] * K for _ in range(S)]
        for d, item in enumerate(self.plan.desc_item.tolist()):
            if nc[d] > 1:       # a single count is the run of N zeros: no visible pixel
                rles[item // K][item % K] = packed[offsets[d]:offsets[d] + nc[d]].copy()
        return rles

    def scene_rles(self, alpha_min: int = 1, cover_min: int = 128):
        """The exact mask of every overlay's visible pixels — every part and
        every hole, unlike ``scene_polygons`` — as the COCO API's uncompressed
        run-length encoding of the bg_h × bg_w mask, encoded on the device
        from the visibility map (ipp_pipe_scene_map with boxes, then
        ipp_scene_rle and ipp_scene_rle_pack; include/ipp.h states the
        definition).  Returns (rles, rows): rles[s][k] is the uint32 array of
        counts of scene s, layer k — runs of zeros and ones alternating, zeros
        first, over the pixels in column-major order; they sum to bg_w·bg_h and
        the ones-runs to the row's `visible` — or None for an overlay without a
        visible pixel; rows is ``scene_boxes``' (S, K, 6) from the same map
        launch.  ``rle_decode`` reads a mask back, ``scene_coco_annotations``
        writes the annotations.  Runs after ``run`` on the current stream; only
        the rows, 8 B of header per overlay and the packed counts are copied
        back (it synchronises).  Scenes of more than 8 layers are refused."""
        alpha_min, cover_min = _check_level("alpha_min", alpha_min), _check_level("cover_min", cover_min)
        self._check_map("scene_rles", None)
        buf, rows = self._launch_map("scene_rles", alpha_min, cover_min, True, None)
        return self._rles(buf, rows), self._rows_by_scene(rows)

    def _launch_amodal(self, caller: str, alpha_min: int, cover_min: int, amap: bool, visible: bool):
        """One ipp_pipe_scene_amodal call (one alpha pass): the device amodal
        rows (descriptor order), the device occ (S, 2, K, K), with ``amap`` the
        (S, bg_h, pitch) presence-map buffer, and with ``visible`` the rows and
        the map buffer of ``_launch_map`` (else None each)."""
        self._scene_scratch(caller)
        p, S, K = self.plan.pipe, self.plan.n_scenes, self.plan.per_scene
        pitch = scene_map_pitch(p.bg_w)

        def new_map():
            return torch.empty((S, p.bg_h, pitch), dtype=torch.uint8, device=self.device)

        arows, occ = self._rows(), torch.empty((S, 2, K, K), dtype=torch.int32, device=self.device)
        abuf = new_map() if amap else None
        rows, vbuf = (self._rows(), new_map()) if visible else (None, None)
        N.check(self.lib.ipp_pipe_scene_amodal(*self._scene_head(), p.bg_w, p.bg_h,
                                               p.max_ov_w, p.max_ov_h, alpha_min, cover_min, p.tap_format,
                                               self._scratch.data_ptr(), arows.data_ptr(), occ.data_ptr(),
                                               abuf.data_ptr() if amap else None,
                                               rows.data_ptr() if visible else None,
                                               vbuf.data_ptr() if visible else None, pitch,
                                               _stream(self.device)), "ipp_pipe_scene_amodal")
        return arows, occ, abuf, rows, vbuf

    def scene_amodal(self, alpha_min: int = 1, cover_min: int = 128, masks: bool = False):
        """The amodal labels of the batch (ipp_pipe_scene_amodal; include/ipp.h
        states the rule): what every overlay is behind its occluders, and who
        occludes whom.  Returns (arows, occ): arows is (S, K, 6) int32 (x0, y0,
        x1, y1, area, visible) in scene, layer order — the half-open tight box
        of the overlay's PRESENT pixels (alpha >= alpha_min), covered or not,
        or (-1, -1, -1, -1); area and visible are ``scene_boxes``' — and occ is
        (S, 2, K, K) int32: occ[s, 0, k, j] (j > k) the present pixels of layer
        k that layer j covers (alpha >= cover_min), whoever else does;
        occ[s, 1, k, j] those whose TOPMOST covering layer is j; the diagonals
        are area and visible, so each row of occ[s, 1] sums to the area.  With
        ``masks`` it returns (arows, occ, amap): the presence maps, a device
        uint8 tensor (S, bg_h, bg_w) like ``scene_masks``' (bit k of a byte =
        layer k present there; a view of a pitched buffer).  It runs after
        ``run`` on the current stream and synchronises for the copy back.
        Scenes of more than 8 layers are refused (ValueError)."""
        alpha_min, cover_min = _check_level("alpha_min", alpha_min), _check_level("cover_min", cover_min)
        if not isinstance(masks, (bool, np.bool_)):
            raise ValueError(f"SceneRunner.scene_amodal: masks {masks!r}: a bool")
        self._check_map("scene_amodal", None)
        arows, occ, abuf, _, _ = self._launch_amodal("scene_amodal", alpha_min, cover_min, bool(masks), False)
        res = (self._rows_by_scene(arows), occ.cpu().numpy())
        return res + (abuf[:, :, :self.plan.bg_w],) if masks else res

    def scene_amodal_rles(self, alpha_min: int = 1, cover_min: int = 128):
        """``scene_rles`` of the presence maps: (arles, arows, occ), arles[s][k]
        the uint32 COCO counts of overlay k's full (amodal) mask — its ones-runs
        sum to the row's `area` — or None for an overlay without a present
        pixel; arows and occ are ``scene_amodal``'s, from the same call.
        Encoded on the device (ipp_pipe_scene_amodal, then ipp_scene_rle and
        ipp_scene_rle_pack on the presence map and the amodal rows); it
        synchronises.  Scenes of more than 8 layers are refused."""
        alpha_min, cover_min = _check_level("alpha_min", alpha_min), _check_level("cover_min", cover_min)
        self._check_map("scene_amodal_rles", None)
        arows, occ, abuf, _, _ = self._launch_amodal("scene_amodal_rles", alpha_min, cover_min, True, False)
        return self._rles(abuf, arows), self._rows_by_scene(arows), occ.cpu().numpy()

    def scene_amodal_polygons(self, alpha_min: int = 1, cover_min: int = 128, max_edges: Optional[int] = None,
                              simplify: Optional[float] = None):
        """``scene_polygons`` of the presence maps: (polys, info, arows), the
        outer contour of every overlay's PRESENT pixels (its largest 8-connected
        part, as there), covered or not, traced on the device from the presence
        map and the amodal rows; ``max_edges`` and ``simplify`` as in
        ``scene_polygons``; arows is ``scene_amodal``'s.  It synchronises.
        Scenes of more than 8 layers are refused."""
        alpha_min, cover_min = _check_level("alpha_min", alpha_min), _check_level("cover_min", cover_min)
        self._check_map("scene_amodal_polygons", None)
        max_edges = self._check_max_edges("scene_amodal_polygons", max_edges)
        eps_q = self._check_simplify("scene_amodal_polygons", simplify)
        arows, _, abuf, _, _ = self._launch_amodal("scene_amodal_polygons", alpha_min, cover_min, True, False)
        polys, info = self._polygons(abuf, arows, max_edges, eps_q)
        return polys, info, self._rows_by_scene(arows)

    def run_labelled(self, src: torch.Tensor, bgs: torch.Tensor, out: torch.Tensor, class_ids=0,
                     alpha_min: int = 1, cover_min: int = 128, min_visible: float = 0.0, masks: bool = False,
                     polygons: bool = False, max_edges: Optional[int] = None, simplify: Optional[float] = None,
                     obb: bool = False, rle: bool = False, cull: bool = False, min_pixels: int = 1,
                     amodal: bool = False):
        """``run`` plus the YOLO lines of every scene (``scene_labels``):
        labels[s] lists scene s's lines in layer order, one per overlay with
        visible > 0 and visible / area >= min_visible.  Returns (out, labels);
        with ``masks`` (out, labels, map), the map of ``scene_masks`` from the
        same launch as the boxes.  With ``polygons`` the tuple gains, as its
        last element, the segmentation lines of ``scene_seg_labels`` (polygons
        of ``scene_polygons`` with ``max_edges`` and ``simplify``), traced from
        that same map launch.  ``simplify`` without ``polygons`` is refused.
        With ``obb`` the tuple gains, after the segmentation lines if any, the
        YOLO-OBB lines of ``scene_obb_labels`` (records of ``scene_obbs``):
        the map launch, the tracer and the pack run once for both, the boxes
        always come from the unsimplified outline (``simplify`` changes the
        segmentation lines only), and with ``obb`` alone no vertex is copied
        back.  Their corners are not clipped to the image.  With ``rle`` the
        tuple gains, as its last element (after the OBB lines if any), the COCO
        annotations of ``scene_coco_annotations`` (encodings of
        ``scene_rles``, compressed counts, image id = scene index), from that
        same map launch.  With ``cull`` the run is ``run_culled``'s — the H
        launches, the cull with ``min_visible`` as its threshold and
        ``min_pixels``, the V launches — everything above is produced as
        always, from the cleared scratch (a culled overlay has row (-1, -1,
        -1, -1, 0, 0), no line, no map bit, no polygon, box or annotation; a
        kept one always has its line), and the tuple gains ``kept``, the
        (S, K) bool array of ``run_culled``, as its last element.  The
        scratch stays cleared afterwards, as ``run_culled`` describes.
        ``min_visible`` must then lie in 0..1.  With ``amodal`` the tuple
        gains, after the COCO annotations if any and before ``kept``, the
        amodal annotations of ``scene_amodal_annotations`` (full and visible
        mask, occlusion rate and occluders of every overlay that has a line;
        compressed counts, image id = scene index).  The labels of the whole
        call then come from one ipp_pipe_scene_amodal call — one alpha pass —
        that takes the map launch's place; without ``amodal`` the launches are
        unchanged.  A culled overlay is absent from the amodal rows, the
        occlusion counts and the presence map as well."""
        alpha_min, cover_min = _check_level("alpha_min", alpha_min), _check_level("cover_min", cover_min)
        if not isinstance(cull, (bool, np.bool_)):
            raise ValueError(f"SceneRunner.run_labelled: cull {cull!r}: a bool")
        if not isinstance(amodal, (bool, np.bool_)):
            raise ValueError(f"SceneRunner.run_labelled: amodal {amodal!r}: a bool")
        if cull:
            min_q, min_pixels = self._check_cull("run_labelled", min_visible, min_pixels)
        if simplify is not None and not polygons:
            raise ValueError("SceneRunner.run_labelled: simplify needs polygons=True")
        if masks or polygons or obb or rle or amodal:
            self._check_map("run_labelled", None)
        eps_q = None
        if polygons or obb:
            max_edges = self._check_max_edges("run_labelled", max_edges)
        if polygons:
            eps_q = self._check_simplify("run_labelled", simplify)
        if obb:
            self._check_obb("run_labelled")
        rec = None
        if cull:
            self._check("run_labelled", src, bgs, out)
            self._launch_h(src, bgs, out)
            rec = self._launch_cull("run_labelled", alpha_min, cover_min, min_q, min_pixels)
            self._launch_v(bgs, out)
        else:
            self.run(src, bgs, out)
        if amodal:
            arows, occ, abuf, rows, buf = self._launch_amodal("run_labelled", alpha_min, cover_min, True, True)
        elif masks or polygons or obb or rle:
            buf, rows = self._launch_map("run_labelled", alpha_min, cover_min, True, None)
        else:
            rows = self._launch_boxes(alpha_min, cover_min)
        bg_w, bg_h = self.plan.bg_w, self.plan.bg_h
        boxes = self._rows_by_scene(rows)
        res = (out, scene_labels(boxes, bg_w, bg_h, class_ids, min_visible))
        if masks:
            res += (buf[:, :, :bg_w],)
        if polygons or obb:
            polys, info, obbs = self._trace(buf, rows, max_edges, eps_q, polygons=polygons, obb=obb)
            if polygons:
                res += (scene_seg_labels(polys, info, boxes, bg_w, bg_h, class_ids, min_visible),)
            if obb:
                res += (scene_obb_labels(obbs, info, boxes, bg_w, bg_h, class_ids, min_visible),)
        vrles = self._rles(buf, rows) if rle or amodal else None
        if rle:
            res += (scene_coco_annotations(vrles, boxes, bg_w, bg_h, class_ids, min_visible),)
        if amodal:
            res += (scene_amodal_annotations(self._rles(abuf, arows), vrles, self._rows_by_scene(arows), boxes,
                                             occ.cpu().numpy(), bg_w, bg_h, class_ids, min_visible),)
        if cull:
            res += (self._cull_by_scene(rec)[0],)
        return res

    def _feed_lut(self, lut, mean, std, dtype) -> torch.Tensor:
        """The device table of ``feed``: uploaded once per distinct argument."""
        if lut is None:
            try:
                key = ("lut", tuple(float(v) for v in mean), tuple(float(v) for v in std), dtype)
                hash(key)
            except (TypeError, ValueError):
                key = None
            if key is None or key not in self._feed_cache:
                table = feed_lut(mean, std, dtype).to(self.device)      # (raises on what key could not hold)
                if key is None:
                    return table
                self._feed_cache[key] = table
            return self._feed_cache[key]
        if not isinstance(lut, torch.Tensor) or lut.dtype not in _FEED_DTYPES or tuple(lut.shape) != (3, 256):
            raise ValueError("SceneRunner.feed: lut must be a (3, 256) tensor of torch.float16, torch.bfloat16 or "
                             "torch.float32 (labels_fmt.feed_lut)")
        if lut.device.type == self.device.type and self.device.index in (None, lut.device.index):
            return lut.contiguous()
        if lut.device.type != "cpu":
            raise ValueError(f"SceneRunner.feed: lut on {lut.device}: a CPU tensor or one on {self.device} expected")
        words = lut.contiguous().view(torch.int16 if lut.element_size() == 2 else torch.int32)
        key = ("table", lut.dtype, words.numpy().tobytes())
        if key not in self._feed_cache:
            self._feed_cache[key] = lut.to(self.device)
        return self._feed_cache[key]

    def _feed_classes(self, class_ids) -> Optional[torch.Tensor]:
        """Device class ids by descriptor (None = class 0 everywhere): uploaded once per distinct argument."""
        n = len(self.plan.descs)
        if isinstance(class_ids, (int, np.integer)) and not isinstance(class_ids, (bool, np.bool_)):
            ids = None if int(class_ids) == 0 else [int(class_ids)] * n
        else:
            ids = [int(c) for c in class_ids]
            if len(ids) != n:
                raise ValueError(f"SceneRunner.feed: {len(ids)} class ids for {n} overlays")
        if ids is None:
            return None
        if not all(0 <= c <= 1 << 24 for c in ids):
            raise ValueError("SceneRunner.feed: class ids must lie in 0..2^24 (float32 holds them exactly)")
        key = ("classes", tuple(ids))
        if key not in self._feed_cache:
            by_item = np.array(ids, np.int32)              # scene-major, as scene_labels takes them
            self._feed_cache[key] = _to_dev(by_item[self.plan.desc_item], self.device).view(torch.int32)
        return self._feed_cache[key]

    def feed(self, out: torch.Tensor, lut: Optional[torch.Tensor] = None, mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0),
             dtype: torch.dtype = torch.float16, bgr: bool = False, class_ids=0, alpha_min: int = 1,
             cover_min: int = 128, min_visible: float = 0.0, index_map: bool = False,
             images: Optional[torch.Tensor] = None, size=None, resample: str = "bilinear", letterbox: bool = False,
             pad_value: int = 114, scaleup: bool = True, center: bool = True) -> SceneFeed:
        """The training batch of the composites `out` of the last ``run``, left
        on the device (include/ipp.h: ipp_scene_feed_images, _targets,
        _index_map): a ``SceneFeed`` of
          images   (S, 3, bg_h, bg_w): images[s, c, y, x] = lut[c][out[s, y, x,
                   c]] (with ``bgr`` channel 2 - c).  ``lut`` is a (3, 256)
                   table of float16, bfloat16 or float32 (``feed_lut``), on the
                   CPU or on the device, and its dtype is the images'; None =
                   ``feed_lut(mean, std, dtype)``.  The table's words are
                   copied, so the images equal the table's entries bit for bit.
          targets  (S·K, 6) float32 rows (scene, class, cx, cy, w, h) of the
                   overlays ``scene_labels`` gives a line at the same
                   thresholds — visible > 0 and 65536·visible >=
                   min_visible_q(min_visible)·area, the cull's test — in scene,
                   layer order; cx = float32(x0 + x1) / float32(2·bg_w) and so
                   on, one rounded division each; the unused rows are all -1
                   (``targets[:, 0] >= 0`` masks them).  ``class_ids`` as in
                   ``scene_labels`` (0..2^24).
          count    (1,) int32, the rows in use.
          slot     (S, K) int32: each overlay's row, or -1.
          index_map  with ``index_map`` (S, bg_h, bg_w) uint8, a view of a
                   pitched buffer like ``scene_masks``': 0 where no kept
                   overlay is visible, else 1 + the row, within the scene's
                   run of targets, of the topmost kept overlay visible there;
                   else None.
        The rows come from the box launch, or with ``index_map`` from the map
        launch (at most 8 layers), so it runs after ``run`` on the current
        stream.  Everything stays on the device: nothing is copied back and
        nothing synchronises; the table and the class ids are uploaded once per
        distinct argument and kept on the runner.  ``images`` supplies the
        output (contiguous, on the device, of the table's dtype and the shape
        above; every element is written).

        ``size`` = (out_h, out_w), or one int for a square, gives the batch at
        the network's input size (include/ipp.h: ipp_scene_feed_resize,
        ipp_scene_feed_index_map_sampled): every composite is resized on the
        device exactly as Pillow's ``Image.resize((out_w, out_h), F)`` resizes
        it, F = ``resample``, one of ``FEED_RESAMPLE`` (box, bilinear, hamming,
        bicubic, lanczos) — the horizontal pass first, rounded and clipped to
        uint8, then the vertical one — and the table is applied to the result;
        ``images`` is (S, 3, out_h, out_w).  A plain stretch leaves normalised
        boxes as they are: targets, count and slot are those of ``size=None``
        bit for bit.  ``index_map`` is (S, out_h, out_w), Pillow's NEAREST
        resize of the full-size one.  The taps are built and uploaded once per
        (size, resample), the NEAREST tables once per size and only when an
        ``index_map`` is asked for; both stay on the runner for its lifetime
        (a few tens of KB per distinct size, never evicted: a loop that draws
        a new size per batch keeps one entry per size it has seen).  A
        filter window above ``IPP_FEED_RESIZE_MAX_KSIZE`` source pixels (a
        reduction beyond 21x for lanczos, 63x for bilinear) is a ValueError.

        ``letterbox=True`` (it needs ``size``) keeps the aspect instead
        (include/ipp.h: ipp_scene_feed_letterbox, _targets_letterbox,
        _index_map_letterbox).  With (out_h, out_w, new_h, new_w, top, left) =
        ``letterbox_geometry((bg_h, bg_w), size, scaleup, center)`` — the
        geometry is that call's result, ``SceneFeed`` keeps its five fields —
        every composite is resized to (new_h, new_w) as above and sits at
        (top, left) of ``images`` (S, 3, out_h, out_w); everywhere else
        ``images[s, c]`` is ``lut[c][pad_value]`` (an int in 0..255, YOLO's 114
        by default), all in one launch.  The targets follow the rectangle: cx =
        ((x0 + x1)·new_w + 2·left·bg_w) / (2·bg_w·out_w), w = (x1 - x0)·new_w /
        (bg_w·out_w), cy and h alike, exact integers divided once in float64
        and rounded once to float32 (not the one float32 division of the plain
        feed: the two can differ in the last bit even where the rectangle is the
        canvas); count and slot are unchanged.  ``index_map`` is (S, out_h,
        out_w): the NEAREST resize to (new_h, new_w) at (top, left), 0 around
        it.  The minimal rectangle of a stride is reached by passing
        ``letterbox_geometry(..., stride=s)``'s (out_h, out_w) as ``size``.  The
        taps and the NEAREST tables are those of the inner size, shared with a
        plain stretch to it."""
        if not self._hpass_done:
            raise ValueError("SceneRunner.feed: no run has filled the composites and the scratch on this runner")
        return self._feed_launch(*self._feed_args("feed", out, lut, mean, std, dtype, bgr, class_ids, alpha_min,
                                                  cover_min, min_visible, index_map, images, size, resample,
                                                  letterbox, pad_value, scaleup, center))

    def _feed_resize(self, who: str, size, resample, index_map: bool, box=None):
        """(out_h, out_w, ksize_x, ksize_y, taps_x, taps_y, xtab, ytab, box) of ``feed(size=...)``: the device taps
        of one (size, resample) and, with `index_map` only (None otherwise), the NEAREST tables of the size, each
        built and uploaded once.  With `box` = (pad_value, scaleup, center) of a letterboxed feed, the taps and
        tables are those of the rectangle and the last element is (``letterbox_geometry``'s result, pad_value),
        None otherwise.  ValueError for what the entries would refuse."""
        if isinstance(size, (int, np.integer)) and not isinstance(size, (bool, np.bool_)):
            size = (size, size)
        ok = isinstance(size, (tuple, list)) and len(size) == 2 and all(
            isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_)) and v >= 1 for v in size)
        if not ok or int(size[0]) * int(size[1]) >= 1 << 28:
            raise ValueError(f"{who}: size {size!r}: (out_h, out_w) or one int, each >= 1, out_h*out_w < 2^28")
        if not isinstance(resample, str) or resample not in FEED_RESAMPLE:
            raise ValueError(f"{who}: resample {resample!r}: one of {', '.join(FEED_RESAMPLE)}")
        p = self.plan.pipe
        oh, ow = int(size[0]), int(size[1])
        if box is not None:
            geo = letterbox_geometry((p.bg_h, p.bg_w), (oh, ow), box[1], box[2])
            oh, ow, box = geo.new_h, geo.new_w, (geo, box[0])
        key, near = ("resize", oh, ow, resample), ("nearest", oh, ow)
        if key not in self._feed_cache:
            if p.bg_w * p.bg_h >= 1 << 28:
                raise ValueError(f"{who}: a {p.bg_w}x{p.bg_h} background: bg_w*bg_h must stay below 2^28")
            axes = []
            for n_in, n_out, name in ((p.bg_w, ow, "width"), (p.bg_h, oh, "height")):
                k, taps = G.identity_taps(n_in) if n_in == n_out else G.resample_taps(resample, n_in, n_out)
                if k > N.IPP_FEED_RESIZE_MAX_KSIZE:
                    raise ValueError(f"{who}: {resample} {n_in}->{n_out} ({name}) takes windows of {k} source pixels, "
                                     f"IPP_FEED_RESIZE_MAX_KSIZE is {N.IPP_FEED_RESIZE_MAX_KSIZE}")
                axes.append((k, taps))
            dev = [_to_dev(taps, self.device).view(torch.int32) for _, taps in axes]
            self._feed_cache[key] = (oh, ow, axes[0][0], axes[1][0], *dev)
        if index_map and near not in self._feed_cache:
            self._feed_cache[near] = tuple(_to_dev(G.nearest_table(n_in, n_out), self.device).view(torch.int32)
                                           for n_in, n_out in ((p.bg_w, ow), (p.bg_h, oh)))
        return self._feed_cache[key] + (self._feed_cache[near] if index_map else (None, None)) + (box,)

    def _feed_args(self, caller: str, out, lut, mean, std, dtype, bgr, class_ids, alpha_min, cover_min, min_visible,
                   index_map, images, size=None, resample="bilinear", letterbox=False, pad_value=114, scaleup=True,
                   center=True):
        """Everything ``feed`` refuses with ValueError, before any launch, and the uploads: the arguments of
        ``_feed_launch``."""
        who = f"SceneRunner.{caller}"
        alpha_min, cover_min = _check_level("alpha_min", alpha_min), _check_level("cover_min", cover_min)
        min_q = min_visible_q(min_visible)
        for name, v in (("bgr", bgr), ("index_map", index_map), ("letterbox", letterbox), ("scaleup", scaleup),
                        ("center", center)):
            if not isinstance(v, (bool, np.bool_)):
                raise ValueError(f"{who}: {name} {v!r}: a bool")
        if isinstance(pad_value, (bool, np.bool_)) or not isinstance(pad_value, (int, np.integer)) or \
                not 0 <= pad_value <= 255:
            raise ValueError(f"{who}: pad_value {pad_value!r}: an int in 0..255")
        if letterbox and size is None:
            raise ValueError(f"{who}: letterbox=True needs size, the canvas (out_h, out_w)")
        p, S = self.plan.pipe, self.plan.n_scenes

        def on_device(t):
            return isinstance(t, torch.Tensor) and t.device.type == self.device.type and \
                self.device.index in (None, t.device.index)

        if not on_device(out) or out.dtype != torch.uint8 or tuple(out.shape) != (S, p.bg_h, p.bg_w, 3) or \
                not out.is_contiguous():
            raise ValueError(f"{who}: out must be the contiguous uint8 composites ({S}, {p.bg_h}, {p.bg_w}, 3) on "
                             f"{self.device}")
        if max(p.bg_w, p.bg_h) > N.IPP_FEED_MAX_SIDE:
            raise ValueError(f"{who}: a {p.bg_w}x{p.bg_h} background: bg_w and bg_h must not exceed "
                             f"{N.IPP_FEED_MAX_SIDE} (ipp_scene_feed_targets' exact divisions)")
        if index_map:
            self._check_map(caller, None)
        if self._feed_cache is None:
            self._feed_cache = {}
        table = self._feed_lut(lut, mean, std, dtype)
        classes = self._feed_classes(class_ids)
        resize = None if size is None else self._feed_resize(
            who, size, resample, bool(index_map), (int(pad_value), bool(scaleup), bool(center)) if letterbox else None)
        if resize is None:
            shape = (S, 3, p.bg_h, p.bg_w)
        elif resize[8] is None:
            shape = (S, 3, resize[0], resize[1])
        else:
            shape = (S, 3, resize[8][0].out_h, resize[8][0].out_w)
        if images is None:
            images = torch.empty(shape, dtype=table.dtype, device=self.device)
        elif not on_device(images) or images.dtype != table.dtype or tuple(images.shape) != shape or \
                not images.is_contiguous():
            raise ValueError(f"{who}: images must be a contiguous {table.dtype} tensor {shape} on {self.device}")
        return caller, out, table, bool(bgr), classes, alpha_min, cover_min, min_q, bool(index_map), images, resize

    def _feed_launch(self, caller: str, out, table, bgr: bool, classes, alpha_min: int, cover_min: int, min_q: int,
                     index_map: bool, images, resize=None) -> SceneFeed:
        """The launches of ``feed``: the box or the map launch, then the two or three feed entries (with `resize`,
        ``_feed_resize``'s tables, the resizing ones, or the letterboxing ones where it names a rectangle)."""
        p, S, K = self.plan.pipe, self.plan.n_scenes, self.plan.per_scene
        st, lib = _stream(self.device), self.lib
        buf = None
        if index_map:
            buf, rows = self._launch_map(caller, alpha_min, cover_min, True, None)
        else:
            rows = self._launch_boxes(alpha_min, cover_min)
        if resize is None:
            N.check(lib.ipp_scene_feed_images(out.data_ptr(), images.data_ptr(), table.data_ptr(), S, p.bg_w, p.bg_h,
                                              table.element_size(), int(bgr), st), "ipp_scene_feed_images")
        else:
            oh, ow, kx, ky, taps_x, taps_y, xtab, ytab, box = resize
        if resize is not None and box is None:
            N.check(lib.ipp_scene_feed_resize(out.data_ptr(), images.data_ptr(), table.data_ptr(), taps_x.data_ptr(),
                                              taps_y.data_ptr(), S, p.bg_w, p.bg_h, ow, oh, kx, ky,
                                              table.element_size(), int(bgr), st), "ipp_scene_feed_resize")
        elif resize is not None:
            geo, pad = box
            rect = (geo.new_w, geo.new_h, geo.left, geo.top, geo.out_w, geo.out_h)
            N.check(lib.ipp_scene_feed_letterbox(out.data_ptr(), images.data_ptr(), table.data_ptr(), taps_x.data_ptr(),
                                                 taps_y.data_ptr(), S, p.bg_w, p.bg_h, *rect, kx, ky, pad,
                                                 table.element_size(), int(bgr), st), "ipp_scene_feed_letterbox")
        targets = torch.empty((S * K, 6), dtype=torch.float32, device=self.device)
        count = torch.empty(1, dtype=torch.int32, device=self.device)
        slot = torch.empty((S, K), dtype=torch.int32, device=self.device)
        ids = classes.data_ptr() if classes is not None else None
        if resize is None or box is None:
            N.check(lib.ipp_scene_feed_targets(rows.data_ptr(), self._scene_layer.data_ptr(), ids, S * K, S, K, p.bg_w,
                                               p.bg_h, min_q, targets.data_ptr(), count.data_ptr(), slot.data_ptr(),
                                               st), "ipp_scene_feed_targets")
        else:
            N.check(lib.ipp_scene_feed_targets_letterbox(rows.data_ptr(), self._scene_layer.data_ptr(), ids, S * K, S, K,
                                                         p.bg_w, p.bg_h, min_q, *rect, targets.data_ptr(),
                                                         count.data_ptr(), slot.data_ptr(), st),
                    "ipp_scene_feed_targets_letterbox")
        idx = None
        if index_map and resize is None:
            ibuf = torch.empty_like(buf)
            N.check(lib.ipp_scene_feed_index_map(buf.data_ptr(), buf.shape[2], p.bg_w, p.bg_h, slot.data_ptr(), S, K,
                                                 ibuf.data_ptr(), st), "ipp_scene_feed_index_map")
            idx = ibuf[:, :, :p.bg_w]
        elif index_map and box is not None:
            ibuf = torch.empty((S, geo.out_h, (geo.out_w + 15) // 16 * 16), dtype=torch.uint8, device=self.device)
            N.check(lib.ipp_scene_feed_index_map_letterbox(buf.data_ptr(), buf.shape[2], p.bg_w, p.bg_h, slot.data_ptr(),
                                                           S, K, xtab.data_ptr(), ytab.data_ptr(), *rect,
                                                           ibuf.data_ptr(), ibuf.shape[2], st),
                    "ipp_scene_feed_index_map_letterbox")
            idx = ibuf[:, :, :geo.out_w]
        elif index_map:
            ibuf = torch.empty((S, oh, (ow + 15) // 16 * 16), dtype=torch.uint8, device=self.device)
            N.check(lib.ipp_scene_feed_index_map_sampled(buf.data_ptr(), buf.shape[2], p.bg_w, p.bg_h, slot.data_ptr(),
                                                         S, K, xtab.data_ptr(), ytab.data_ptr(), ow, oh,
                                                         ibuf.data_ptr(), ibuf.shape[2], st),
                    "ipp_scene_feed_index_map_sampled")
            idx = ibuf[:, :, :ow]
        return SceneFeed(images, targets, count, slot, idx)

    def run_feed(self, src: torch.Tensor, bgs: torch.Tensor, out: torch.Tensor, lut: Optional[torch.Tensor] = None,
                 mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0), dtype: torch.dtype = torch.float16, bgr: bool = False,
                 class_ids=0, alpha_min: int = 1, cover_min: int = 128, min_visible: float = 0.0,
                 index_map: bool = False, images: Optional[torch.Tensor] = None, cull: bool = False,
                 min_pixels: int = 1, size=None, resample: str = "bilinear", letterbox: bool = False,
                 pad_value: int = 114, scaleup: bool = True, center: bool = True) -> SceneFeed:
        """``run`` followed by ``feed`` (same arguments), all on the current
        stream and without a copy back.  With ``cull`` the run is
        ``run_culled``'s — the H launches, ipp_pipe_scene_cull with
        ``min_visible`` and ``min_pixels``, the V launches — and its records
        stay on the device; the feed's keep rule is the cull's fraction test,
        so every painted overlay then has a row of targets and every row a
        painted overlay (the scratch stays cleared afterwards, as
        ``run_culled`` describes)."""
        if not isinstance(cull, (bool, np.bool_)):
            raise ValueError(f"SceneRunner.run_feed: cull {cull!r}: a bool")
        if cull:
            min_q, min_pixels = self._check_cull("run_feed", min_visible, min_pixels)
        self._check("run_feed", src, bgs, out)
        args = self._feed_args("run_feed", out, lut, mean, std, dtype, bgr, class_ids, alpha_min, cover_min,
                               min_visible, index_map, images, size, resample, letterbox, pad_value, scaleup, center)
        self._launch_h(src, bgs, out)
        if cull:
            self._launch_cull("run_feed", args[5], args[6], min_q, min_pixels)
        self._launch_v(bgs, out)
        return self._feed_launch(*args)
