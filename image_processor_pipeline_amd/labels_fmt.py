"""Label and mask formatting of the batched pipe: pure host code, no library
call and no GPU.

``yolo_label(s)`` write the reference's one label per composite (overlays.py:141-149),
from its rectangle or from the tight boxes of ``PipeRunner.overlay_bboxes``.  For the
scenes of scenes.py, ``scene_labels`` formats the box lines and ``scene_seg_labels`` the
YOLO segmentation lines and ``scene_obb_labels`` the YOLO-OBB lines (``obb_corners`` states the
corner rule), all for the overlays ``_label_lines`` names; ``instance_ids`` and
``scene_instance_masks`` turn a visibility map into instance masks.  ``scene_coco_annotations``
writes the COCO annotations of ``SceneRunner.scene_rles``' run-length encodings, ``rle_counts_string``
/ ``rle_counts_from_string`` are the COCO API's compressed ``counts`` string and ``rle_decode``
reads a mask back; ``scene_amodal_annotations`` writes the amodal ones (full and visible mask, occluders)
of ``SceneRunner.scene_amodal_rles``.  ``feed_lut`` tabulates the normalisation of ``SceneRunner.feed``'s
images, ``FEED_RESAMPLE`` names the filters of its ``size`` and ``letterbox_geometry`` states where its
``letterbox`` puts a composite.  ``fused`` re-exports it all.
"""
from __future__ import annotations

import math
from typing import List, NamedTuple, Optional, Tuple

import numpy as np

from . import _native as N
from .labels_math import xyxy2xywhn


def yolo_label(class_id: int, box: Tuple[int, int, int, int], bg_w: int, bg_h: int) -> str:
    """One YOLO label line for the pixel box (x0, y0, x1, y1) on a bg_w×bg_h
    composite, formatted as the reference does (overlays.py:143-149)."""
    cx, cy, w, h = xyxy2xywhn(np.array(box).reshape(1, 4), bg_w, bg_h)[0]
    return f"{class_id} {cx:.6f} {cy:.6f} {w:.6f} {h:.6f}"


def yolo_labels(plan, class_id: int = 0, boxes: Optional[np.ndarray] = None) -> List[Optional[str]]:
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
        x0, y0, x1, y1 = (0, 0, int(it["ov_w"][i]), int(it["ov_h"][i])) if boxes is None else (int(v) for v in boxes[i])
        out.append(None if x0 < 0 else yolo_label(class_id, (x + x0, y + y0, x + x1, y + y1), plan.bg_w, plan.bg_h))
    return out


def _scene_rows(rows, name: str) -> Tuple[np.ndarray, int, int]:
    """The (S, K, 6) rows of ``SceneRunner.scene_boxes`` as an array, with S and K."""
    rows = np.asarray(rows)
    if rows.ndim != 3 or rows.shape[2] != 6:
        raise ValueError(f"{name} of shape {rows.shape}: (scenes, layers, 6) expected")
    return (rows,) + rows.shape[:2]


def _label_lines(rows: np.ndarray, class_ids, min_visible: float):
    """(s, k, class id, row) of every overlay that gets a label line, in scene, layer order: those with
    visible > 0 and visible / area >= min_visible.  ``class_ids``: an int, or one per overlay (S·K, scene-major)."""
    S, K = rows.shape[:2]
    if isinstance(class_ids, (int, np.integer)):
        ids = [int(class_ids)] * (S * K)
    else:
        ids = [int(c) for c in class_ids]
        if len(ids) != S * K:
            raise ValueError(f"{len(ids)} class ids for {S * K} overlays")
    for s in range(S):
        for k in range(K):
            area, vis = int(rows[s, k, 4]), int(rows[s, k, 5])
            if vis > 0 and vis >= min_visible * area:
                yield s, k, ids[s * K + k], rows[s, k]


def scene_labels(boxes: np.ndarray, bg_w: int, bg_h: int, class_ids=0, min_visible: float = 0.0) -> List[List[str]]:
    """YOLO lines of every scene from the (S, K, 6) rows (x0, y0, x1, y1, area,
    visible) of ``SceneRunner.scene_boxes``: labels[s] lists, in layer order,
    one line (``yolo_label``) per overlay with visible > 0 and visible / area
    >= min_visible (``_label_lines``, ``class_ids`` too); an empty list = an empty label file."""
    boxes, S, _ = _scene_rows(boxes, "boxes")
    out: List[List[str]] = [[] for _ in range(S)]
    for s, _, class_id, row in _label_lines(boxes, class_ids, min_visible):
        out[s].append(yolo_label(class_id, tuple(int(v) for v in row[:4]), bg_w, bg_h))
    return out


def min_visible_q(min_visible) -> int:
    """``min_q`` of ipp_pipe_scene_cull for a visible fraction ``min_visible``,
    a real number in [0, 1]: ⌈min_visible·65536⌉ (the product is exact, a
    scaling by a power of two).  Anything else raises ValueError.  With the
    ceiling, 65536·visible >= min_q·area implies visible >= min_visible·area in
    the reals, and rounding that product to a float cannot lift it above the
    integer `visible`: an overlay the cull keeps always passes the test of
    ``scene_labels`` with the same ``min_visible``."""
    if isinstance(min_visible, (bool, np.bool_)) or \
            not isinstance(min_visible, (int, float, np.integer, np.floating)):
        raise ValueError(f"min_visible {min_visible!r}: a real number in 0..1 expected")
    v = float(min_visible)
    if not 0.0 <= v <= 1.0:     # (NaN fails both comparisons)
        raise ValueError(f"min_visible {min_visible!r}: a real number in 0..1 expected")
    return int(math.ceil(v * 65536.0))


# The filters of ``SceneRunner.feed(size=..., resample=...)``: Pillow's five convolution filters, by the names of
# ``PIL.Image.Resampling`` in lower case, in the order of ipp_plan_resample's codes (ipp.h IPP_RESAMPLE_*).
FEED_RESAMPLE = ("box", "bilinear", "hamming", "bicubic", "lanczos")


def feed_lut(mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0), dtype=None, scale: float = 1.0 / 255.0):
    """The (3, 256) table of ``SceneRunner.feed`` (ipp_scene_feed_images) as a
    torch CPU tensor of ``dtype`` (float16, the default, bfloat16 or float32):
    entry [c][v] = ((v·scale) − mean[c]) / std[c], computed in float64 and
    rounded once to ``dtype`` (``torch.tensor(..., dtype=float64).to(dtype)``).
    Row c is output plane c's, whichever input channel feeds it (``bgr``).
    ValueError: mean or std not three finite reals, a std <= 0, a non-finite
    scale, any other dtype."""
    import torch
    dtype = torch.float16 if dtype is None else dtype
    if dtype not in (torch.float16, torch.bfloat16, torch.float32):
        raise ValueError(f"feed_lut: dtype {dtype!r}: torch.float16, torch.bfloat16 or torch.float32 expected")

    def three(name, v):
        try:
            out = [float(x) for x in v]
        except (TypeError, ValueError):
            raise ValueError(f"feed_lut: {name} {v!r}: three real numbers expected") from None
        if len(out) != 3 or not all(math.isfinite(x) for x in out):
            raise ValueError(f"feed_lut: {name} {v!r}: three finite real numbers expected")
        return out

    mean, std = three("mean", mean), three("std", std)
    if any(x <= 0.0 for x in std):
        raise ValueError(f"feed_lut: std {std!r}: every entry must be > 0")
    if isinstance(scale, (bool, np.bool_)) or not isinstance(scale, (int, float, np.integer, np.floating)) or \
            not math.isfinite(float(scale)):
        raise ValueError(f"feed_lut: scale {scale!r}: a finite real number expected")
    v = np.arange(256, dtype=np.float64) * float(scale)
    table = np.stack([(v - mean[c]) / std[c] for c in range(3)])
    return torch.tensor(table, dtype=torch.float64).to(dtype)


class Letterbox(NamedTuple):
    """The canvas and the rectangle of a letterboxed batch (``letterbox_geometry``)."""
    out_h: int
    out_w: int
    new_h: int
    new_w: int
    top: int
    left: int


def _round_half_even_div(n: int, c: int) -> int:
    """n / c rounded half to even, in integers (Python's ``round`` of the exact quotient)."""
    q, rem = divmod(n, c)
    return q + 1 if 2 * rem > c or (2 * rem == c and q & 1) else q


def letterbox_geometry(bg_hw, size, scaleup: bool = True, center: bool = True, stride=None) -> Letterbox:
    """Where ``SceneRunner.feed(size=..., letterbox=True)`` puts a bg_h x bg_w
    composite in an out_h x out_w canvas (include/ipp.h states the rule): the
    usual LetterBox, r = min(out_h / bg_h, out_w / bg_w) (min(r, 1) without
    ``scaleup``), in exact integers.  The limiting axis (the smaller ratio, by
    cross-multiplication; both on a tie) takes its canvas extent, the other
    one a·b / c rounded half to even and at least 1; ``center`` puts the
    rectangle at (dh // 2, dw // 2), else at (0, 0).  ``stride`` = s, an int
    >= 1, is the minimal rectangle: the canvas shrinks to new + (out - new) %
    s per axis before the offsets are taken; its (out_h, out_w) are what to
    pass as ``size`` to get that canvas.  ``bg_hw`` = (bg_h, bg_w); ``size`` =
    (out_h, out_w) or one int.  ValueError: sizes that are not positive ints,
    out_h·out_w >= 2^28, a side above IPP_FEED_MAX_SIDE, a stride that is not
    an int >= 1, flags that are not bools."""
    def is_int(v):
        return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))

    if is_int(size):
        size = (size, size)
    for name, v in (("bg_hw", bg_hw), ("size", size)):
        if not (isinstance(v, (tuple, list)) and len(v) == 2 and all(is_int(x) and x >= 1 for x in v)):
            raise ValueError(f"letterbox_geometry: {name} {v!r}: two ints >= 1 expected")
        if max(v) > N.IPP_FEED_MAX_SIDE:
            raise ValueError(f"letterbox_geometry: {name} {v!r}: no side may exceed {N.IPP_FEED_MAX_SIDE}")
    for name, v in (("scaleup", scaleup), ("center", center)):
        if not isinstance(v, (bool, np.bool_)):
            raise ValueError(f"letterbox_geometry: {name} {v!r}: a bool")
    if stride is not None and not (is_int(stride) and stride >= 1):
        raise ValueError(f"letterbox_geometry: stride {stride!r}: an int >= 1 or None")
    (bg_h, bg_w), (out_h, out_w) = (int(v) for v in bg_hw), (int(v) for v in size)
    if out_h * out_w >= 1 << 28:
        raise ValueError(f"letterbox_geometry: size {size!r}: out_h*out_w must stay below 2^28")
    if not scaleup and out_h >= bg_h and out_w >= bg_w:
        new_h, new_w = bg_h, bg_w
    else:
        by_h, by_w = out_h * bg_w, out_w * bg_h          # r_h < r_w  <=>  out_h·bg_w < out_w·bg_h
        new_h = out_h if by_h <= by_w else max(_round_half_even_div(bg_h * out_w, bg_w), 1)
        new_w = out_w if by_w <= by_h else max(_round_half_even_div(bg_w * out_h, bg_h), 1)
    if stride is not None:
        out_h, out_w = new_h + (out_h - new_h) % int(stride), new_w + (out_w - new_w) % int(stride)
    top, left = ((out_h - new_h) // 2, (out_w - new_w) // 2) if center else (0, 0)
    return Letterbox(out_h, out_w, new_h, new_w, top, left)


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
    import torch
    on_torch = isinstance(vis_map, torch.Tensor)
    vis_map = vis_map if on_torch else np.asarray(vis_map)
    if vis_map.dtype != (torch.uint8 if on_torch else np.uint8):
        raise ValueError(f"instance_ids: a uint8 map expected, got {vis_map.dtype}")
    return torch.from_numpy(_INSTANCE_LUT).to(vis_map.device)[vis_map.long()] if on_torch else _INSTANCE_LUT[vis_map]


def scene_instance_masks(vis_map, rows) -> List[List[Optional[np.ndarray]]]:
    """Per-overlay instance masks from a copied-back visibility map (S, bg_h,
    bg_w) and the (S, K, 6) rows of ``scene_boxes``: masks[s] lists, in layer
    order, the boolean array of bit k cropped to overlay k's box (y1 - y0, x1
    - x0), or None for an overlay without a visible pixel.  Host code; a
    device map is copied back first (synchronises)."""
    import torch
    if isinstance(vis_map, torch.Tensor):
        vis_map = vis_map.cpu().numpy()
    vis_map = np.asarray(vis_map)
    rows, S, K = _scene_rows(rows, "rows")
    if vis_map.dtype != np.uint8 or vis_map.ndim != 3 or vis_map.shape[0] != S:
        raise ValueError(f"a uint8 map of {S} scenes (S, bg_h, bg_w) expected, got {vis_map.dtype} {vis_map.shape}")
    if K > N.IPP_SCENE_MAP_MAX_LAYERS:
        raise ValueError(f"{K} layers: a visibility map holds at most {N.IPP_SCENE_MAP_MAX_LAYERS}")

    def mask(s: int, k: int) -> Optional[np.ndarray]:
        x0, y0, x1, y1 = (int(v) for v in rows[s, k, :4])
        return None if x0 < 0 else ((vis_map[s, y0:y1, x0:x1] >> k) & 1).astype(bool)

    return [[mask(s, k) for k in range(K)] for s in range(S)]


def scene_contour_capacity(plan) -> int:
    """Default ``max_edges`` of ``SceneRunner.scene_polygons``: 8·(max_ov_w +
    max_ov_h) rounded up to 256 — four times the 2(w + h) boundary edges of a
    monotone outline filling the largest overlay's box."""
    p = plan.pipe if hasattr(plan, "pipe") else plan
    return (8 * (int(p.max_ov_w) + int(p.max_ov_h)) + 255) // 256 * 256


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
    one line (``seg_label``) per overlay that ``scene_labels`` gives a line
    (``_label_lines``).  ``class_ids`` as there.  An overlay that would get a
    line but overflowed ``max_edges`` (header flags bit 0) raises ValueError
    naming the ``max_edges`` it needs: a label is never dropped or truncated."""
    info = np.asarray(info)
    rows, S, K = _scene_rows(rows, "rows")
    if info.shape != (S, K, N.IPP_CONTOUR_HDR):
        raise ValueError(f"info of shape {info.shape}: ({S}, {K}, {N.IPP_CONTOUR_HDR}) expected")
    if len(polys) != S or any(len(p) != K for p in polys):
        raise ValueError(f"polys does not hold {S} scenes of {K} overlays")
    out: List[List[str]] = [[] for _ in range(S)]
    for s, k, class_id, row in _label_lines(rows, class_ids, min_visible):
        if int(info[s, k, 7]) & 1:
            raise ValueError(f"scene {s} layer {k}: its contour has {int(info[s, k, 0])} boundary edges, "
                             f"scene_polygons needs max_edges >= {int(info[s, k, 0])}")
        if polys[s][k] is None:
            raise ValueError(f"scene {s} layer {k}: {int(row[5])} visible pixels but no polygon")
        out[s].append(seg_label(class_id, polys[s][k], bg_w, bg_h))
    return out


def obb_corners(rec) -> np.ndarray:
    """The four corners, (4, 2) float64 in lattice coordinates, of one
    ipp_polygons_obb record {ax, ay, dx, dy, lo, hi, hgt, m} with m >= 2: C(t, s)
    = (ax + (t·dx − s·dy) / nn, ay + (t·dy + s·dx) / nn) for (lo, 0), (hi, 0),
    (hi, hgt), (lo, hgt), in the rule's operation order (include/ipp.h) — clockwise
    on the screen from the chosen hull edge.  They are NOT clipped: the rectangle
    of an object at the image border may leave the image slightly."""
    rec = np.asarray(rec)
    if rec.shape != (N.IPP_OBB_REC,):
        raise ValueError(f"a record of shape {rec.shape}: ({N.IPP_OBB_REC},) expected")
    ax, ay, dx, dy, lo, hi, hgt, m = (int(v) for v in rec)
    nn = dx * dx + dy * dy
    if m < 2 or nn == 0:
        raise ValueError(f"record {rec.tolist()}: no direction (m = {m}), it has no corners")
    return np.array([(ax + (t * dx - s * dy) / nn, ay + (t * dy + s * dx) / nn)
                     for t, s in ((lo, 0), (hi, 0), (hi, hgt), (lo, hgt))], np.float64)


def obb_label(class_id: int, rec, bg_w: int, bg_h: int) -> str:
    """One YOLO-OBB line ``class x1 y1 x2 y2 x3 y3 x4 y4`` for one
    ipp_polygons_obb record on a bg_w×bg_h composite: the corners of
    ``obb_corners`` as x / bg_w and y / bg_h, in the number format of
    ``yolo_label``.  Not clipped to 0..1 (see ``obb_corners``)."""
    return " ".join([str(class_id)] + [f"{x / bg_w:.6f} {y / bg_h:.6f}" for x, y in obb_corners(rec)])


def scene_obb_labels(obbs, info, rows, bg_w: int, bg_h: int, class_ids=0, min_visible: float = 0.0) -> List[List[str]]:
    """YOLO-OBB lines of every scene from what ``SceneRunner.scene_obbs``
    returns: labels[s] lists, in layer order, one line (``obb_label``) per
    overlay that ``scene_labels`` gives a line (``_label_lines``).
    ``class_ids`` as there.  An overlay that would get a line but overflowed
    ``max_edges`` (header flags bit 0) raises ValueError naming the
    ``max_edges`` it needs, as ``scene_seg_labels`` does, and one whose record
    has m < 3 or hgt == 0 (no rectangle) raises too: a label is never dropped.
    The corners are not clipped to the image."""
    info, obbs = np.asarray(info), np.asarray(obbs)
    rows, S, K = _scene_rows(rows, "rows")
    if info.shape != (S, K, N.IPP_CONTOUR_HDR):
        raise ValueError(f"info of shape {info.shape}: ({S}, {K}, {N.IPP_CONTOUR_HDR}) expected")
    if obbs.shape != (S, K, N.IPP_OBB_REC):
        raise ValueError(f"obbs of shape {obbs.shape}: ({S}, {K}, {N.IPP_OBB_REC}) expected")
    out: List[List[str]] = [[] for _ in range(S)]
    for s, k, class_id, row in _label_lines(rows, class_ids, min_visible):
        if int(info[s, k, 7]) & 1:
            raise ValueError(f"scene {s} layer {k}: its contour has {int(info[s, k, 0])} boundary edges, "
                             f"scene_obbs needs max_edges >= {int(info[s, k, 0])}")
        if int(obbs[s, k, 7]) < 3 or int(obbs[s, k, 6]) == 0:
            raise ValueError(f"scene {s} layer {k}: {int(row[5])} visible pixels but no oriented box "
                             f"(record {obbs[s, k].tolist()})")
        out[s].append(obb_label(class_id, obbs[s, k], bg_w, bg_h))
    return out


def _rle_counts(counts) -> List[int]:
    """`counts` as a list of Python ints: a 1-D sequence of non-negative integers."""
    a = np.asarray(counts)
    if a.ndim != 1 or (a.size and a.dtype.kind not in "iu"):
        raise ValueError(f"RLE counts of shape {a.shape} and type {a.dtype}: a 1-D integer sequence expected")
    out = [int(v) for v in a]
    if any(v < 0 for v in out):
        raise ValueError("RLE counts must not be negative")
    return out


def rle_counts_string(counts) -> str:
    """The COCO API's compressed ``counts`` string of uncompressed RLE counts
    (its ``rleToString`` rule).  Count i is coded as x = counts[i] for i < 3 and
    x = counts[i] - counts[i - 2] from the fourth count on (a signed
    difference).  x is written in 5-bit groups, least significant first: c = x &
    0x1f, x >>= 5 (arithmetic); the group is the last when x has become 0 and
    bit 0x10 of c is clear, or x has become -1 and bit 0x10 is set (that bit is
    the sign); every other group gets the continuation bit 0x20; the character
    is chr(c + 48)."""
    cnts = _rle_counts(counts)
    out = []
    for i, x in enumerate(cnts):
        if i > 2:
            x -= cnts[i - 2]
        while True:
            c = x & 0x1f
            x >>= 5
            more = (x != -1) if c & 0x10 else (x != 0)
            out.append(chr((c | 0x20 if more else c) + 48))
            if not more:
                break
    return "".join(out)


def rle_counts_from_string(s: str) -> np.ndarray:
    """The uint32 counts of a COCO compressed ``counts`` string (the API's
    ``rleFrString`` rule, the inverse of ``rle_counts_string``): 5-bit groups
    c = ord(ch) - 48, least significant first, up to the first without the
    continuation bit 0x20; bit 0x10 of that last group extends the sign; from
    the fourth count on the value is a difference against the count two
    before.  A string that is not such a code raises ValueError."""
    if isinstance(s, bytes):
        s = s.decode("ascii")
    cnts: List[int] = []
    p, n = 0, len(s)
    while p < n:
        x, k = 0, 0
        while True:
            if p >= n:
                raise ValueError("RLE string ends inside a count")
            c = ord(s[p]) - 48
            if not 0 <= c < 64:
                raise ValueError(f"RLE string: character {s[p]!r} at {p}")
            x |= (c & 0x1f) << (5 * k)
            p += 1
            k += 1
            if not c & 0x20:
                if c & 0x10:
                    x |= -1 << (5 * k)
                break
        if len(cnts) > 2:
            x += cnts[-2]
        if not 0 <= x < 1 << 32:
            raise ValueError(f"RLE string: count {len(cnts)} decodes to {x}")
        cnts.append(x)
    return np.array(cnts, np.uint32)


def rle_decode(counts, bg_h: int, bg_w: int) -> np.ndarray:
    """The boolean (bg_h, bg_w) mask of uncompressed RLE counts (or of a
    compressed string): runs of zeros and ones alternate, zeros first, over the
    pixels in column-major order (include/ipp.h: ipp_scene_rle).  The counts
    must sum to bg_h·bg_w."""
    cnts = np.asarray(rle_counts_from_string(counts) if isinstance(counts, (str, bytes)) else _rle_counts(counts),
                      np.int64)
    if int(cnts.sum()) != int(bg_h) * int(bg_w):
        raise ValueError(f"RLE counts sum to {int(cnts.sum())}, a {bg_h}x{bg_w} mask has {int(bg_h) * int(bg_w)} pixels")
    flat = np.repeat(np.arange(len(cnts)) & 1, cnts).astype(bool)
    return flat.reshape(int(bg_w), int(bg_h)).T.copy()


def scene_coco_annotations(rles, rows, bg_w: int, bg_h: int, class_ids=0, min_visible: float = 0.0,
                           compressed: bool = True, image_ids=None, first_id: int = 1) -> List[List[dict]]:
    """COCO annotations of every scene from what ``SceneRunner.scene_rles``
    returns: anns[s] lists, in layer order, one dict per overlay that
    ``scene_labels`` gives a line (``_label_lines``, ``class_ids`` as there):
    {"id", "image_id", "category_id", "bbox": [x0, y0, x1 - x0, y1 - y0],
    "area": visible, "iscrowd": 0, "segmentation": {"size": [bg_h, bg_w],
    "counts": ...}} — counts is the compressed string (``rle_counts_string``),
    or with ``compressed=False`` the list of counts.  Ids run from ``first_id``
    in scene, layer order; ``image_ids`` (one per scene) defaults to the scene
    index.  Every value is a plain int, list or str: ``json.dumps`` takes the
    result.  An overlay that would get an annotation but has no encoding
    raises ValueError: an annotation is never dropped."""
    rows, S, K = _scene_rows(rows, "rows")
    if len(rles) != S or any(len(r) != K for r in rles):
        raise ValueError(f"rles does not hold {S} scenes of {K} overlays")
    img = list(range(S)) if image_ids is None else [int(v) for v in image_ids]
    if len(img) != S:
        raise ValueError(f"{len(img)} image ids for {S} scenes")
    out: List[List[dict]] = [[] for _ in range(S)]
    next_id = int(first_id)
    for s, k, class_id, row in _label_lines(rows, class_ids, min_visible):
        if rles[s][k] is None:
            raise ValueError(f"scene {s} layer {k}: {int(row[5])} visible pixels but no run-length encoding")
        cnts = _rle_counts(rles[s][k])
        x0, y0, x1, y1 = (int(v) for v in row[:4])
        out[s].append({"id": next_id, "image_id": img[s], "category_id": int(class_id),
                       "bbox": [x0, y0, x1 - x0, y1 - y0], "area": int(row[5]), "iscrowd": 0,
                       "segmentation": {"size": [int(bg_h), int(bg_w)],
                                        "counts": rle_counts_string(cnts) if compressed else cnts}})
        next_id += 1
    return out


def scene_amodal_annotations(arles, vrles, arows, rows, occ, bg_w: int, bg_h: int, class_ids=0,
                             min_visible: float = 0.0, compressed: bool = True, image_ids=None,
                             first_id: int = 1) -> List[List[dict]]:
    """Amodal annotations (KINS / COCOA style) of every scene from what
    ``SceneRunner.scene_amodal_rles`` (arles, arows, occ) and
    ``SceneRunner.scene_rles`` (vrles, rows) return at the same thresholds:
    anns[s] lists, in layer order, one dict per overlay that ``scene_labels``
    gives a line (``_label_lines`` on the VISIBLE rows, ``class_ids`` as there),
    so the lists align with every other label of the scene.  {"id", "image_id",
    "category_id", "iscrowd": 0, "bbox": the amodal box [x0, y0, w, h], "area":
    the amodal (present) area, "segmentation": the amodal mask's RLE {"size":
    [bg_h, bg_w], "counts"}, "visible_bbox", "visible_area", "visible_mask": the
    same three of the visible part, "occlude_rate": 1 - visible / area, "layer":
    k, "occluders": the layers j > k with occ[s][0][k][j] > 0, ascending}.
    counts, ids and ``image_ids`` as in ``scene_coco_annotations``; every value
    is a plain int, float, list or str (``json.dumps`` takes the result).  An
    overlay that would get an annotation but lacks one of its two encodings
    raises ValueError: an annotation is never dropped."""
    rows, S, K = _scene_rows(rows, "rows")
    arows = _scene_rows(arows, "arows")[0]
    occ = np.asarray(occ)
    if arows.shape != rows.shape:
        raise ValueError(f"arows of shape {arows.shape} beside rows of shape {rows.shape}")
    if occ.shape != (S, 2, K, K):
        raise ValueError(f"occ of shape {occ.shape}: ({S}, 2, {K}, {K}) expected")
    for name, rl in (("arles", arles), ("vrles", vrles)):
        if len(rl) != S or any(len(r) != K for r in rl):
            raise ValueError(f"{name} does not hold {S} scenes of {K} overlays")
    img = list(range(S)) if image_ids is None else [int(v) for v in image_ids]
    if len(img) != S:
        raise ValueError(f"{len(img)} image ids for {S} scenes")

    def enc(rl, s, k, what):
        if rl[s][k] is None:
            raise ValueError(f"scene {s} layer {k}: an annotation without its {what} run-length encoding")
        cnts = _rle_counts(rl[s][k])
        return {"size": [int(bg_h), int(bg_w)], "counts": rle_counts_string(cnts) if compressed else cnts}

    def xywh(row):
        x0, y0, x1, y1 = (int(v) for v in row[:4])
        return [x0, y0, x1 - x0, y1 - y0]

    out: List[List[dict]] = [[] for _ in range(S)]
    next_id = int(first_id)
    for s, k, class_id, row in _label_lines(rows, class_ids, min_visible):
        arow = arows[s, k]
        area, vis = int(arow[4]), int(row[5])
        if area < vis:
            raise ValueError(f"scene {s} layer {k}: amodal area {area} below its {vis} visible pixels "
                             f"(arows and rows of different calls?)")
        out[s].append({"id": next_id, "image_id": img[s], "category_id": int(class_id), "iscrowd": 0,
                       "bbox": xywh(arow), "area": area, "segmentation": enc(arles, s, k, "amodal"),
                       "visible_bbox": xywh(row), "visible_area": vis, "visible_mask": enc(vrles, s, k, "visible"),
                       "occlude_rate": 1.0 - vis / area, "layer": int(k),
                       "occluders": [j for j in range(k + 1, K) if int(occ[s, 0, k, j]) > 0]})
        next_id += 1
    return out
