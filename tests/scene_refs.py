"""CPU references shared by tests/test_scenes_cpu.py and tests/test_gpu_scenes.py
(not a test module).  Everything is composed from the existing oracle:

    ov_i      = oracle.pipe.overlay(src[i], bg_hw, params[i], cfg)
    composite = paste_rgba_onto_rgb(... paste_rgba_onto_rgb(bgs[b(s)], ov_{sK}, x, y) ..., ov_{sK+K-1}, x, y)

and the label rows come straight from the definition of visibility: overlay
pixel (u, v) of layer k is present iff A_k[v, u] >= alpha_min and visible iff
it is present and every later layer j > k of the scene whose rectangle holds
composite pixel (x_k + u, y_k + v) has A_j < cover_min there."""
import numpy as np

from oracle import ops
from oracle import pipe as opipe


def scene_overlays(src, plan, cfg):
    """The resized RGBA overlay of every overlay item, in item order."""
    bg_hw = (plan.bg_h, plan.bg_w)
    return [opipe.overlay(src[i], bg_hw, prm, cfg) for i, prm in enumerate(plan.params)]


def scene_composites(bgs, plan, overlays):
    """The iterated composite of every scene: (S, bg_h, bg_w, 3)."""
    K, prm = plan.per_scene, plan.params
    out = []
    for s in range(plan.n_scenes):
        img = bgs[prm[s * K].bg_index]
        for i in range(s * K, (s + 1) * K):
            img = ops.paste_rgba_onto_rgb(img, overlays[i], prm[i].x, prm[i].y)
        out.append(img)
    return np.stack(out)


def scene_rows(plan, overlays, alpha_min, cover_min, occlusion=True):
    """(S, K, 6) int32 rows (x0, y0, x1, y1, area, visible), the box half-open
    in composite coordinates and all -1 without a visible pixel.
    ``occlusion=False``: no layer hides anything (the unoccluded boxes)."""
    S, K, prm = plan.n_scenes, plan.per_scene, plan.params
    rows = np.empty((S, K, 6), np.int32)
    for s in range(S):
        for k in range(K):
            i = s * K + k
            a = overlays[i][..., 3]
            h, w = a.shape
            present = a >= alpha_min
            hidden = np.zeros((h, w), bool)
            for j in range(i + 1, (s + 1) * K if occlusion else i + 1):
                aj = overlays[j][..., 3]
                hj, wj = aj.shape
                # layer j's rectangle in layer k's overlay coordinates
                dx, dy = prm[j].x - prm[i].x, prm[j].y - prm[i].y
                u0, u1, v0, v1 = max(dx, 0), min(dx + wj, w), max(dy, 0), min(dy + hj, h)
                if u0 < u1 and v0 < v1:
                    hidden[v0:v1, u0:u1] |= aj[v0 - dy:v1 - dy, u0 - dx:u1 - dx] >= cover_min
            visible = present & ~hidden
            ys, xs = np.nonzero(visible)
            if len(ys):
                box = [prm[i].x + xs.min(), prm[i].y + ys.min(), prm[i].x + xs.max() + 1, prm[i].y + ys.max() + 1]
            else:
                box = [-1, -1, -1, -1]
            rows[s, k] = box + [int(present.sum()), int(visible.sum())]
    return rows


def scene_noise_batch(fused, S, K, H, W, n_bg, bh, bw, cfg, seed):
    """Random sources and backgrounds and their scene plan (the draws of
    tests/label_refs.noise_batch, S·K sources)."""
    rng = np.random.default_rng(seed)
    src = rng.integers(0, 256, (S * K, H, W, 3), np.uint8)
    bgs = rng.integers(0, 256, (n_bg, bh, bw, 3), np.uint8)
    return src, bgs, fused.plan_scenes((H, W), S, K, (bh, bw), n_bg, cfg, seed=seed)


def host_v_ksteps(plan):
    """K steps of every V tap tile of the plan, from the host restatement of
    the device tap tiles (ipp_plan_mfma_tile; hdr[1] = K steps)."""
    from image_processor_pipeline_amd.geometry import mfma_tiles
    return {int(nk) for ax in plan.axes[1::2] for nk in mfma_tiles(ax)[0][:, 1]}
