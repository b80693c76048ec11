"""CPU reference of the scenes' cull (ipp_pipe_scene_cull /
SceneRunner.run_culled) and the cases shared by tests/test_cull_cpu.py and
tests/test_gpu_cull.py (not a test module).

``cull`` applies the rule of include/ipp.h to ``scene_refs.scene_overlays``:
per scene the layers from the last to the first, each counted against the KEPT
later layers only.  The composites are ``ops.paste_rgba_onto_rgb`` of the kept
overlays alone; the label rows are ``scene_refs.scene_rows`` on the overlays
with the culled ones made transparent — absent, as the device's readers of the
cleared scratch see them."""
import numpy as np

from oracle import ops
from tests import scene_mask_refs as MR
from tests import scene_refs as SR


def keep_rule(area: int, vis: int, min_q: int, min_pixels: int) -> bool:
    """include/ipp.h: vis >= max(min_pixels, 1) and 65536·vis >= min_q·area (Python ints: exact)."""
    return vis >= max(int(min_pixels), 1) and 65536 * int(vis) >= int(min_q) * int(area)


def _counts(plan, overlays, i, later, alpha_min, cover_min):
    """(area, visible) of overlay item i against the overlay items `later` (of its scene)."""
    prm = plan.params
    a = overlays[i][..., 3]
    h, w = a.shape
    present = a >= alpha_min
    hidden = np.zeros((h, w), bool)
    for j in later:
        aj = overlays[j][..., 3]
        hj, wj = aj.shape
        dx, dy = prm[j].x - prm[i].x, prm[j].y - prm[i].y
        u0, u1, v0, v1 = max(dx, 0), min(dx + wj, w), max(dy, 0), min(dy + hj, h)
        if u0 < u1 and v0 < v1:
            hidden[v0:v1, u0:u1] |= aj[v0 - dy:v1 - dy, u0 - dx:u1 - dx] >= cover_min
    return int(present.sum()), int((present & ~hidden).sum())


def cull(plan, overlays, alpha_min, cover_min, min_q, min_pixels, top_down=True, max_ov=None, alone=()):
    """kept (S, K) bool and stats (S, K, 2) int32 = (area, visible) at the
    decision.  ``top_down=False`` is the WRONG rule the chain case tells apart:
    every layer tested against all later layers, culled or not.  ``max_ov`` =
    (max_ov_w, max_ov_h): a larger overlay has no plane — kept, counts 0, hides
    nothing.  ``alone``: overlay items decided as if alone in their scene (and
    unseen by the others)."""
    S, K = plan.n_scenes, plan.per_scene
    kept = np.zeros((S, K), bool)
    stats = np.zeros((S, K, 2), np.int32)

    def no_plane(i):
        h, w = overlays[i].shape[:2]
        return max_ov is not None and (w > max_ov[0] or h > max_ov[1])

    for s in range(S):
        for k in range(K - 1, -1, -1):
            i = s * K + k
            if no_plane(i):
                kept[s, k] = True
                continue
            later = [] if i in alone else \
                [s * K + j for j in range(k + 1, K)
                 if (kept[s, j] or not top_down) and not no_plane(s * K + j) and s * K + j not in alone]
            area, vis = _counts(plan, overlays, i, later, alpha_min, cover_min)
            stats[s, k] = area, vis
            kept[s, k] = keep_rule(area, vis, min_q, min_pixels)
    return kept, stats


def composites(bgs, plan, overlays, kept):
    """The iterated composite of every scene from its kept overlays alone: (S, bg_h, bg_w, 3)."""
    K, prm = plan.per_scene, plan.params
    out = []
    for s in range(plan.n_scenes):
        img = bgs[prm[s * K].bg_index]
        for k in range(K):
            i = s * K + k
            if kept[s, k]:
                img = ops.paste_rgba_onto_rgb(img, overlays[i], prm[i].x, prm[i].y)
        out.append(img)
    return np.stack(out)


def absent(overlays, kept):
    """The overlays with the culled ones made fully transparent (item order)."""
    flat = np.asarray(kept).reshape(-1)
    return [ov if flat[i] else np.zeros_like(ov) for i, ov in enumerate(overlays)]


def rows(plan, overlays, kept, alpha_min, cover_min):
    """(S, K, 6) rows of ``scene_refs.scene_rows`` restricted to the kept layers: a culled one is absent."""
    return SR.scene_rows(plan, absent(overlays, kept), alpha_min, cover_min)


def t_extent(desc):
    """(offset, bytes per group row, pitch, group rows) of what the H launch writes of a descriptor's T."""
    h = desc["h"]
    return int(h["dst_off"]), 16 * int(h["out_len"]), int(h["dst_pitch"]), (int(h["lines"]) + 15) // 16 * 4


def t_mask(plan, which):
    """Bool mask over the bytes of tmp: the T of the descriptors in `which` (descriptor indices)."""
    m = np.zeros(int(plan.pipe.tmp_bytes), bool)
    for d in which:
        off, rb, pitch, G = t_extent(plan.descs[d])
        for g in range(G):
            m[off + g * pitch:off + g * pitch + rb] = True
    return m


# --- the cases ----------------------------------------------------------------------------
def chain_scene(fused):
    """One scene of 3 structured layers on a 96×128 background (the sources
    and the HSV ranges of ``scene_mask_refs.cover_scenes``): layer 2 covers
    most of layer 1, layer 1 most of layer 0, and layer 2's rectangle misses
    layer 0's object.  Top down, layer 1 is culled and layer 0 then kept; tested
    against all later layers, layer 0 would be culled too."""
    from tests import label_refs as R
    cfg = fused.PipeConfig(margins=R.STRUCT_MARGINS, hsv_ranges=list(R.STRUCT_RANGES))
    H, W, K = 140, 120, 3
    rng = np.random.default_rng(11)
    src = np.empty((K, H, W, 3), np.uint8)
    src[:] = (90, 120, 60)

    def plant(i, r0, r1, c0, c1):
        src[i, r0:r1, c0:c1] = rng.integers(160, 256, (r1 - r0, c1 - c0, 3))

    plant(0, 30, 110, 12, 36)       # layer 0: an object in the left part
    plant(1, 20, 120, 10, 110)      # layer 1: a wide object over layer 0's and further right
    plant(2, 10, 130, 10, 110)      # layer 2: a wide object, pasted over layer 1's right part only
    bgs = rng.integers(0, 256, (1, 96, 128, 3), np.uint8)
    specs = [(0.0, "o", 0, 0.5)] * K
    plan = MR.given(fused, (H, W), (96, 128), 1, cfg, K, specs, lambda ov: [(10, 10), (10, 10), (30, 10)])
    return src, bgs, plan, cfg


CHAIN_Q = (1, 128, 32768, 1)        # alpha_min, cover_min, min_q (= one half), min_pixels

# (alpha_min, cover_min, min_visible, min_pixels) per batch, at which tests/test_cull_cpu.py finds a culled and a
# kept overlay in the reference
THRESHOLDS = {
    "cover": [(1, 128, 0.4, 1), (1, 128, 0.6, 1), (1, 32, 0.5, 1)],
    "noise": [(1, 128, 0.9, 1), (128, 255, 0.97, 1), (255, 1, 0.5, 1)],
    "odd": [(1, 128, 0.8, 1), (255, 1, 0.7, 1)],
    "eight": [(1, 128, 0.3, 1)],
    "nine": [(1, 128, 0.3, 1)],
}

BATCHES = {
    "cover": MR.cover_scenes, "noise": MR.noise_scenes, "odd": MR.odd_scenes,
    "eight": lambda fused: MR.layered_scene(fused, 8), "nine": lambda fused: MR.layered_scene(fused, 9),
    "chain": chain_scene,
}
