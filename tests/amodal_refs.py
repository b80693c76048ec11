"""CPU reference of the scenes' amodal labels (ipp_pipe_scene_amodal /
SceneRunner.scene_amodal) shared by tests/test_scene_amodal_cpu.py and
tests/test_gpu_scene_amodal.py (not a test module).

Three restatements of include/ipp.h that share no code path with the device's
decomposition (an overlay-centric sweep with a running `hidden` mask, and a
composite-centric map kernel), nor with each other:

  presence_map   composite-centric: per scene one byte image, every layer's
                 present pixels OR-ed in at its clipped rectangle;
  amodal_rows    overlay by overlay, in overlay coordinates, looking up at the
                 later layers (as tests/scene_refs.scene_rows does);
  occlusion      brute force over whole-background boolean images: one PRESENT
                 and one COVER image per layer, then every pair (k, j).

The overlays are ``scene_refs.scene_overlays``' and the batches and LEVELS
those of tests/scene_mask_refs.py.  ``max_ov`` = (max_ov_w, max_ov_h): a larger
overlay has no plane; ``alone``: overlay items that scene_layer does not map —
labelled as if alone in their scene, in no slot, seen by nobody."""
import numpy as np

from tests import scene_mask_refs as MR

ABSENT = [-1, -1, -1, -1, 0, 0]


def _no_plane(ov, max_ov):
    h, w = ov.shape[:2]
    return max_ov is not None and (w > max_ov[0] or h > max_ov[1])


def presence_map(plan, overlays, alpha_min, max_ov=None, alone=()):
    """(S, bg_h, pitch) uint8: bit k of byte (Y, X) set iff layer k is in its
    slot, has a plane, its clipped rectangle holds (X, Y) and A_k >= alpha_min."""
    S, K, prm = plan.n_scenes, plan.per_scene, plan.params
    bw, bh = plan.bg_w, plan.bg_h
    assert K <= MR.MAX_LAYERS
    out = np.zeros((S, bh, MR.pitch_of(bw)), np.uint8)
    for i, ov in enumerate(overlays):
        if i in alone or _no_plane(ov, max_ov):
            continue
        a = ov[..., 3]
        h, w = a.shape
        x, y = prm[i].x, prm[i].y
        X0, X1, Y0, Y1 = max(x, 0), min(x + w, bw), max(y, 0), min(y + h, bh)
        if X0 < X1 and Y0 < Y1:
            bit = (a[Y0 - y:Y1 - y, X0 - x:X1 - x] >= alpha_min).astype(np.uint8) << (i % K)
            out[i // K, Y0:Y1, X0:X1] |= bit.astype(np.uint8)
    return out


def amodal_rows(plan, overlays, alpha_min, cover_min, max_ov=None, alone=()):
    """(S, K, 6) int32 (x0, y0, x1, y1, area, visible): the box of the PRESENT
    pixels, all -1 without one; (-1, -1, -1, -1, 0, 0) without a plane."""
    S, K, prm = plan.n_scenes, plan.per_scene, plan.params
    rows = np.empty((S, K, 6), np.int32)
    for i, ov in enumerate(overlays):
        s, k = divmod(i, K)
        if _no_plane(ov, max_ov):
            rows[s, k] = ABSENT
            continue
        a = ov[..., 3]
        h, w = a.shape
        present = a >= alpha_min
        free = present.copy()                      # present and under no covering later layer
        later = () if i in alone else range(i + 1, (s + 1) * K)
        for j in later:
            if j in alone or _no_plane(overlays[j], max_ov):
                continue
            aj = overlays[j][..., 3]
            hj, wj = aj.shape
            dx, dy = prm[j].x - prm[i].x, prm[j].y - prm[i].y      # layer j's origin in this overlay's coordinates
            u0, u1 = max(dx, 0), min(dx + wj, w)
            for v in range(max(dy, 0), min(dy + hj, h)):           # row by row of the shared rows
                if u0 < u1:
                    free[v, u0:u1] &= aj[v - dy, u0 - dx:u1 - dx] < cover_min
        ys, xs = np.nonzero(present)
        box = [prm[i].x + xs.min(), prm[i].y + ys.min(), prm[i].x + xs.max() + 1, prm[i].y + ys.max() + 1] \
            if len(ys) else [-1, -1, -1, -1]
        rows[s, k] = box + [len(ys), int(free.sum())]
    return rows


def layer_images(plan, overlays, s, alpha_min, cover_min, max_ov=None, alone=()):
    """(present, cover): two (K, bg_h, bg_w) bool stacks of scene s — where layer
    k is PRESENT and where A_k >= cover_min, all False for a layer that is not in
    its slot or has no plane."""
    K, prm = plan.per_scene, plan.params
    bw, bh = plan.bg_w, plan.bg_h
    present, cover = np.zeros((K, bh, bw), bool), np.zeros((K, bh, bw), bool)
    for k in range(K):
        i = s * K + k
        if i in alone or _no_plane(overlays[i], max_ov):
            continue
        a = np.zeros((bh, bw), np.int32)
        inside = np.zeros((bh, bw), bool)
        al = overlays[i][..., 3]
        h, w = al.shape
        x, y = prm[i].x, prm[i].y
        X0, X1 = max(x, 0), min(x + w, bw)
        for v in range(h):                                         # the overlay's rows inside the background
            if 0 <= y + v < bh and X0 < X1:
                a[y + v, X0:X1] = al[v, X0 - x:X1 - x]
                inside[y + v, X0:X1] = True
        present[k], cover[k] = inside & (a >= alpha_min), inside & (a >= cover_min)
    return present, cover


def occlusion(plan, overlays, alpha_min, cover_min, max_ov=None, alone=()):
    """(S, 2, K, K) int32: plane 0 COVERS, plane 1 HIDES, the diagonals area and visible."""
    S, K = plan.n_scenes, plan.per_scene
    occ = np.zeros((S, 2, K, K), np.int32)
    for s in range(S):
        present, cover = layer_images(plan, overlays, s, alpha_min, cover_min, max_ov, alone)
        for k in range(K):
            occ[s, 0, k, k] = present[k].sum()
            occ[s, 1, k, k] = (present[k] & ~cover[k + 1:].any(axis=0)).sum()
            for j in range(k + 1, K):
                both = present[k] & cover[j]
                occ[s, 0, k, j] = both.sum()
                occ[s, 1, k, j] = (both & ~cover[j + 1:].any(axis=0)).sum()      # j is the topmost that covers
    return occ


def reference(plan, overlays, alpha_min, cover_min, max_ov=None, alone=()):
    """(amap, arows, occ) of a batch."""
    return (presence_map(plan, overlays, alpha_min, max_ov, alone),
            amodal_rows(plan, overlays, alpha_min, cover_min, max_ov, alone),
            occlusion(plan, overlays, alpha_min, cover_min, max_ov, alone))


def covered_pair(fused):
    """One scene of two hand-placed overlays on a 96×128 background: layer 1,
    a large opaque block, covers the whole rectangle of layer 0, a small one."""
    from tests import label_refs as R
    cfg = fused.PipeConfig(margins=R.STRUCT_MARGINS, hsv_ranges=list(R.STRUCT_RANGES))
    H, W = 140, 120
    rng = np.random.default_rng(9)
    src = np.empty((2, H, W, 3), np.uint8)
    src[:] = (90, 120, 60)
    src[0, 50:80, 40:70] = rng.integers(160, 256, (30, 30, 3))
    src[1, 10:130, 10:110] = rng.integers(160, 256, (120, 100, 3))
    bgs = rng.integers(0, 256, (1, 96, 128, 3), np.uint8)
    specs = [(0.0, "o", 0, 0.5), (0.0, "o", 0, 0.5)]
    return src, bgs, MR.given(fused, (H, W), (96, 128), 1, cfg, 2, specs, lambda ov: [(30, 20)] * 2), cfg
