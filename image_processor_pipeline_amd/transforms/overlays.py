"""paste_overlay_onto_background — reference transforms/overlays.py:24-187.

Diagonal-ratio sizing with one ``random.uniform(scale_min, scale_max)``
(:108) and the fit cap (:106-126), Pillow ``resize(LANCZOS)`` of the RGBA
overlay (:129), position from two ``random.randint`` (:133-134),
``background.copy().paste(ov, (x, y), ov)`` (:138-139), YOLO label (:143-149),
outputs ``{overlay_stem}{background_suffix}`` and ``{overlay_stem}.txt``
(:165-166); errors print and return None.  Resize and paste run on the GPU
(ipp_lanczos_h/v, ipp_paste_blend), bit-exact with Pillow 12.2.0.
The deprecated ``process_overlay_pair`` (:190-354) is not provided.
"""
from __future__ import annotations

import math
import random
from pathlib import Path
from typing import Any, List, Optional, Tuple

import numpy as np
from PIL import Image, UnidentifiedImageError

from ._common import batch_run, device_transform
from .. import _rt
from .. import batch_ops as BO
from .. import device as D
from .. import geometry as G
from ..jpeg import JpegDecoder, encode_grouped, parse_jpeg
from ..labels_math import xyxy2xywhn
from ..utils import utils


def _convert_to_yolo_bbox(img_width: int, img_height: int, box: Tuple[int, int, int, int]):
    """overlays.py:13-22."""
    if img_width <= 0 or img_height <= 0:
        raise ValueError(f"Les dimensions de l'image ({img_width}x{img_height}) doivent être positives.")
    dw = 1.0 / img_width
    dh = 1.0 / img_height
    return ((box[0] + box[2]) / 2.0 * dw, (box[1] + box[3]) / 2.0 * dh, (box[2] - box[0]) * dw,
            (box[3] - box[1]) * dh)


def _label_str(yolo_class_id: int, box: Optional[Tuple[int, int, int, int]], pos_x: int, pos_y: int,
               bw: int, bh: int) -> str:
    """overlays.py:143-149 for the box (x0, y0, x1, y1) of the overlay placed
    at (pos_x, pos_y): the whole rectangle (0, 0, new_w, new_h) in the
    reference; None (tight_bbox, nothing visible) gives the empty label."""
    if box is None:
        return ""
    bbox = np.array([pos_x + box[0], pos_y + box[1], pos_x + box[2], pos_y + box[3]]).reshape(1, 4)
    cx, cy, w_norm, h_norm = xyxy2xywhn(bbox, bw, bh)[0]
    return f"{yolo_class_id} {cx:.6f} {cy:.6f} {w_norm:.6f} {h_norm:.6f}"


def _is_jpeg(path: Path) -> bool:
    return path.suffix.lower() in (".jpg", ".jpeg")


_DECODER = None


def _read_jpeg(path: Path):
    """(bytes, JpegInfo) of a file the device decoder takes, None for one
    jpeg.parse_jpeg refuses (progressive, greyscale, CMYK, "4:2:2", ...):
    the file read and the marker walk, fit for a host thread.  OSError as
    ``open`` raises it."""
    data = Path(path).read_bytes()
    try:
        return data, parse_jpeg(data)
    except ValueError:
        return None


def _device_backgrounds(paths: List[Path], jobs: Optional[List] = None) -> List:
    """The files ``paths`` decoded on the device (jpeg.JpegDecoder: the pixels
    ``Image.open(p).convert("RGB")`` gives), one call for all of them: per
    path a device tensor (h, w, 3), or None — a file that cannot be read, one
    parse_jpeg refuses, or one whose stream the device finds malformed.  A
    None takes the Pillow path, messages and all.  ``jobs[i]``: what
    _read_jpeg returned for paths[i], where it has been called already."""
    global _DECODER
    if jobs is None:
        jobs = []
        for p in paths:
            try:
                jobs.append(_read_jpeg(p) if _is_jpeg(p) else None)
            except OSError:
                jobs.append(None)
    out: List = [None] * len(paths)
    idx = [i for i, j in enumerate(jobs) if j is not None]
    if idx:
        if _DECODER is None:
            _DECODER = JpegDecoder(_rt.device())
        images = _DECODER.decode_some([jobs[i][0] for i in idx], parsed=[jobs[i][1] for i in idx])[0]
        for i, im in zip(idx, images):
            out[i] = im
    return out


def _save_composite(comp, path: Path) -> None:
    """overlays.py:169 — or the bytes of the file, where the device encoded it."""
    if isinstance(comp, bytes):
        with open(path, "wb") as f:
            f.write(comp)
    elif isinstance(comp, Image.Image):
        comp.save(path)
    else:
        Image.fromarray(comp, "RGB").save(path)


@device_transform
def paste_overlay_onto_background(
    overlay_path: Path,
    background_path: Path,
    output_dirs: List[Path],
    yolo_class_id: int = 0,
    scale_min: float = 0.15,
    scale_max: float = 0.30,
    tight_bbox: bool = False,
    alpha_min: int = 1,
    device_jpeg: bool = False,
    device_decode: bool = False,
    **options: Any,
) -> Optional[List[Path]]:
    """``device_decode`` (not in the reference): a ``.jpg`` / ``.jpeg``
    background that jpeg.parse_jpeg accepts (baseline, 4:2:0 or 4:4:4) is
    decoded on the device (jpeg.JpegDecoder: the pixels ``Image.open`` gives)
    and its pixels never cross the bus; any other file, and one the device
    finds malformed, is opened by Pillow as before.  The outputs are the same
    either way.
    ``device_jpeg`` (not in the reference): where the output suffix is
    ``.jpg`` / ``.jpeg`` the composite is encoded on the device (jpeg.py: the
    same bytes ``save`` writes) and only the file's bytes are copied back; any
    other suffix is saved on the host as before.
    ``tight_bbox`` (not in the reference): the label's box is that of the
    resized overlay's pixels with alpha >= ``alpha_min`` (1..255) instead of
    its whole rectangle; an overlay without such a pixel gets an empty label
    file (the YOLO convention for an image without objects).  The draws, the
    composite, file names and messages do not depend on it."""
    image_target_dir, label_target_dir = utils._validate_dirs(output_dirs, nb_dirs=2)
    names = f"[{overlay_path.name} + {background_path.name}]"
    try:
        overlay = Image.open(overlay_path)
        if overlay.mode != "RGBA":
            overlay = overlay.convert("RGBA")
        bg_dev = _device_backgrounds([background_path])[0] if device_decode else None
        background = None if bg_dev is not None else Image.open(background_path).convert("RGB")
    except FileNotFoundError as fnf:
        print(f"Erreur {names}: Fichier non trouvé: {fnf}")
        return None
    except UnidentifiedImageError as uie:
        print(f"Erreur {names}: Impossible d'ouvrir l'image {uie}")
        return None
    except TypeError as te:
        print(f"Erreur {names}: Type d'image invalide : {te}")
        return None
    except Exception as e:
        print(f"Erreur {names}: Échec lecture fichiers: {e}")
        return None

    try:
        bw, bh = background.size if bg_dev is None else (int(bg_dev.shape[1]), int(bg_dev.shape[0]))
        target_ratio = random.uniform(scale_min, scale_max)
        if overlay.height == 0:
            raise ValueError(f"dimensions de l'overlay {overlay_path.name} invalides ({overlay.width}x{overlay.height}).")
        new_w, new_h = G.overlay_size(overlay.width, overlay.height, bw, bh, target_ratio)
        ov_dev = _rt.h2d(np.asarray(overlay))
        resized = D.resize_lanczos_rgba(ov_dev, new_w, new_h)
        pos_x = random.randint(0, bw - new_w)
        pos_y = random.randint(0, bh - new_h)
        comp = D.paste_blend(bg_dev if bg_dev is not None else _rt.h2d(np.asarray(background)), resized, pos_x, pos_y)
        if device_jpeg and _is_jpeg(background_path):
            composite_image = encode_grouped([comp])[0]
        else:
            composite_image = Image.fromarray(_rt.d2h(comp), "RGB")
        tight = D.alpha_bbox_min([resized], alpha_min)[0] if tight_bbox else (0, 0, new_w, new_h)
        yolo_label_str = _label_str(yolo_class_id, tight, pos_x, pos_y, bw, bh)
    except ValueError as ve:
        print(f"Erreur de valeur {names}: {ve}")
        return None
    except Exception as e:
        print(f"Erreur {names}: Échec pendant le processus de superposition: {e}")
        return None

    saved_paths: List[Path] = []
    img_output_path = Path(image_target_dir) / f"{overlay_path.stem}{background_path.suffix}"
    label_output_path = Path(label_target_dir) / f"{overlay_path.stem}.txt"
    try:
        _save_composite(composite_image, img_output_path)
        saved_paths.append(img_output_path)
        with open(label_output_path, "w", encoding="utf-8") as f:
            f.write(yolo_label_str)
        saved_paths.append(label_output_path)
        return saved_paths
    except Exception as e_save:
        print(f"Erreur {names}: Échec lors de la sauvegarde: {e_save}")
        for p in saved_paths:
            try:
                if p.exists():
                    p.unlink()
            except OSError:
                print(f"Avertissement: Impossible de nettoyer le fichier partiellement créé {p}")
        return None


def _overlays_batch(arg_tuples, output_dirs: List[Path], threads: int = 1, yolo_class_id: int = 0,
                    scale_min: float = 0.15, scale_max: float = 0.30, tight_bbox: bool = False,
                    alpha_min: int = 1, device_jpeg: bool = False, device_decode: bool = False, **options: Any) -> List:
    """Batched paste_overlay_onto_background ('modulo' pairs): decode on host
    threads, the per-item draws (uniform ratio, then two randint) in pair
    order, ONE batched LANCZOS H + V + paste launch set for the chunk
    (batch_ops.overlays), encode + label on host threads.  Messages and
    None results as in the per-file path.  ``tight_bbox``: the boxes come
    from one more batched launch over the chunk's resized overlays
    (ipp_alpha_bbox_min).  ``device_jpeg``: the composites whose output
    suffix is ``.jpg`` / ``.jpeg`` are encoded on the device in the same chunk
    and only their files' bytes come back.  ``device_decode``: the chunk's
    ``.jpg`` / ``.jpeg`` backgrounds that jpeg.parse_jpeg accepts are decoded
    on the device in one call (jpeg.JpegDecoder) and stay there; the host
    threads read their bytes and walk their markers.  A file parse_jpeg
    refuses is opened by Pillow on its thread as before, one the device finds
    malformed after the call."""
    image_target_dir, label_target_dir = utils._validate_dirs(output_dirs, nb_dirs=2)

    def load(args, defer: Optional[bool] = None):
        """(overlay pixels, background pixels); with ``defer`` a background
        the device decoder takes is left as (path, _read_jpeg's result), for
        compute to decode on the device."""
        overlay_path, background_path = args[0], args[1]
        if defer is None:
            defer = device_decode and _is_jpeg(background_path)
        names = f"[{overlay_path.name} + {background_path.name}]"
        try:
            overlay = Image.open(overlay_path)
            if overlay.mode != "RGBA":
                overlay = overlay.convert("RGBA")
            job = _read_jpeg(background_path) if defer else None     # a missing file fails here, as Image.open would
            if job is not None:
                return np.asarray(overlay), (background_path, job)
            background = Image.open(background_path).convert("RGB")
            return np.asarray(overlay), np.asarray(background)
        except FileNotFoundError as fnf:
            print(f"Erreur {names}: Fichier non trouvé: {fnf}")
        except UnidentifiedImageError as uie:
            print(f"Erreur {names}: Impossible d'ouvrir l'image {uie}")
        except TypeError as te:
            print(f"Erreur {names}: Type d'image invalide : {te}")
        except Exception as e:
            print(f"Erreur {names}: Échec lecture fichiers: {e}")
        return None

    def compute(items, args):
        plans, ovs, bgs, sizes, pos, jpeg = [], [], [], [], [], []
        if device_decode:
            items = list(items)
            todo = [k for k, it in enumerate(items) if it is not None and isinstance(it[1], tuple)]
            decoded = _device_backgrounds([items[k][1][0] for k in todo], [items[k][1][1] for k in todo])
            for k, im in zip(todo, decoded):
                if im is None:                         # malformed: Pillow, with its messages
                    items[k] = load(args[k], defer=False)
                else:
                    items[k] = (items[k][0], im)
        for item, a in zip(items, args):
            if item is None:
                plans.append(None)
                continue
            ov, bg = item
            names = f"[{a[0].name} + {a[1].name}]"
            try:
                bh, bw = bg.shape[:2]
                target_ratio = random.uniform(scale_min, scale_max)
                if ov.shape[0] == 0:
                    raise ValueError(f"dimensions de l'overlay {a[0].name} invalides ({ov.shape[1]}x{ov.shape[0]}).")
                new_w, new_h = G.overlay_size(ov.shape[1], ov.shape[0], bw, bh, target_ratio)
                if new_w <= 0 or new_h <= 0:
                    raise ValueError("height and width must be > 0")
                pos_x = random.randint(0, bw - new_w)
                pos_y = random.randint(0, bh - new_h)
            except ValueError as ve:
                print(f"Erreur de valeur {names}: {ve}")
                plans.append(None)
                continue
            except Exception as e:
                print(f"Erreur {names}: Échec pendant le processus de superposition: {e}")
                plans.append(None)
                continue
            plans.append((len(ovs), (new_w, new_h), (pos_x, pos_y), (bw, bh)))
            ovs.append(ov)
            bgs.append(bg)
            sizes.append((new_w, new_h))
            pos.append((pos_x, pos_y))
            jpeg.append(device_jpeg and _is_jpeg(a[1]))
        if tight_bbox:
            try:
                comps, boxes = BO.overlays(ovs, bgs, sizes, pos, bbox_alpha_min=alpha_min, jpeg=jpeg) if ovs else ([], [])
            except ValueError as ve:   # (alpha_min out of range: every pair fails as in the per-file path)
                for p, a in zip(plans, args):
                    if p is not None:
                        print(f"Erreur de valeur [{a[0].name} + {a[1].name}]: {ve}")
                return [None] * len(plans)
        else:
            comps = BO.overlays(ovs, bgs, sizes, pos, jpeg=jpeg) if ovs else []
            boxes = [(0, 0, w, h) for w, h in sizes]
        return [None if p is None else (comps[p[0]], p, boxes[p[0]]) for p in plans]

    def save(args, _item, res):
        if res is None:
            return None
        comp, (_, (new_w, new_h), (pos_x, pos_y), (bw, bh)), box = res
        overlay_path, background_path = args[0], args[1]
        names = f"[{overlay_path.name} + {background_path.name}]"
        yolo_label_str = _label_str(yolo_class_id, box, pos_x, pos_y, bw, bh)
        saved_paths: List[Path] = []
        img_output_path = Path(image_target_dir) / f"{overlay_path.stem}{background_path.suffix}"
        label_output_path = Path(label_target_dir) / f"{overlay_path.stem}.txt"
        try:
            _save_composite(comp, img_output_path)
            saved_paths.append(img_output_path)
            with open(label_output_path, "w", encoding="utf-8") as f:
                f.write(yolo_label_str)
            saved_paths.append(label_output_path)
            return saved_paths
        except Exception as e_save:
            print(f"Erreur {names}: Échec lors de la sauvegarde: {e_save}")
            for p in saved_paths:
                try:
                    if p.exists():
                        p.unlink()
                except OSError:
                    print(f"Avertissement: Impossible de nettoyer le fichier partiellement créé {p}")
            return None

    return batch_run(arg_tuples, threads, load, compute, save)


paste_overlay_onto_background.batch = _overlays_batch
