"""CPU reference of the scenes' visibility maps (ipp_pipe_scene_map /
SceneRunner.scene_masks) and the batches shared by tests/test_scene_masks_cpu.py
and tests/test_gpu_scene_masks.py (not a test module).

``scene_map`` restates the definition composite-centric and top-down — per
scene one `covered` image, the layers walked from the last to the first — so it
shares nothing with ``scene_refs.scene_rows``, which goes overlay by overlay
and looks up at the later layers.  Its overlays are ``scene_refs.scene_overlays``'
(the oracle's resized RGBA overlays)."""
import numpy as np

from tests import label_refs as R
from tests import scene_refs as SR

LEVELS = [(1, 128), (128, 255), (255, 1)]     # (alpha_min, cover_min), as tests/test_gpu_scenes.py
MAX_LAYERS = 8


def pitch_of(bg_w: int) -> int:
    return (bg_w + 15) // 16 * 16


def scene_map(plan, overlays, alpha_min, cover_min, max_ov=None):
    """(S, bg_h, pitch) uint8, pitch = ⌈bg_w/16⌉·16: bit k of byte (Y, X) set
    iff layer k's rectangle (clipped to the background) holds (X, Y), A_k >=
    alpha_min there and no later layer has A_j >= cover_min there.  ``max_ov``
    = (max_ov_w, max_ov_h): a larger overlay has no plane — it sets no bit and
    covers nothing."""
    S, K, prm = plan.n_scenes, plan.per_scene, plan.params
    bw, bh = plan.bg_w, plan.bg_h
    assert K <= MAX_LAYERS
    out = np.zeros((S, bh, pitch_of(bw)), np.uint8)
    for s in range(S):
        covered = np.zeros((bh, bw), bool)
        for k in range(K - 1, -1, -1):
            i = s * K + k
            a = overlays[i][..., 3]
            h, w = a.shape
            if max_ov is not None and (w > max_ov[0] or h > max_ov[1]):
                continue
            x, y = prm[i].x, prm[i].y
            X0, X1, Y0, Y1 = max(x, 0), min(x + w, bw), max(y, 0), min(y + h, bh)
            if X0 >= X1 or Y0 >= Y1:
                continue
            a = a[Y0 - y:Y1 - y, X0 - x:X1 - x]
            under = covered[Y0:Y1, X0:X1]                    # a view: what the later layers cover
            out[s, Y0:Y1, X0:X1] |= ((~under & (a >= alpha_min)).astype(np.uint8) << k).astype(np.uint8)
            under |= a >= cover_min
    return out


def map_rows(vis, K):
    """(S, K, 5) int32 (x0, y0, x1, y1, count) of bit k in each scene's map:
    what ``scene_boxes`` calls the box and `visible` of overlay k."""
    vis = np.asarray(vis)
    out = np.empty((vis.shape[0], K, 5), np.int32)
    for s in range(vis.shape[0]):
        for k in range(K):
            m = (vis[s] >> k) & 1
            out[s, k, :4] = R.np_box(m)
            out[s, k, 4] = int(m.sum())
    return out


def rects(plan, overlays):
    """Per scene the union of the overlays' rectangles, (S, bg_h, bg_w) bool."""
    K, prm = plan.per_scene, plan.params
    inside = np.zeros((plan.n_scenes, plan.bg_h, plan.bg_w), bool)
    for i, ov in enumerate(overlays):
        h, w = ov.shape[:2]
        inside[i // K, prm[i].y:prm[i].y + h, prm[i].x:prm[i].x + w] = True
    return inside


# --- the batches (sources, backgrounds, plan, cfg) ---------------------------------------
MASK_NOISE_SEED = 23   # tests/test_gpu_scenes.NOISE_SEED: tests/test_scene_masks_cpu.py asserts, on the reference
                       # alone, that this seed meets the conditions the GPU tests rely on


def noise_scenes(fused, seed=MASK_NOISE_SEED):
    """4 scenes × 3 layers of noise (the `noise` batch of tests/test_gpu_scenes.py)."""
    cfg = fused.PipeConfig(margins=(0.05, 9, 0.1, 3), scale_min=0.2, scale_max=0.7)
    src, bgs, plan = SR.scene_noise_batch(fused, 4, 3, 150, 170, 3, 128, 160, cfg, seed)
    return src, bgs, plan, cfg


def odd_scenes(fused):
    """97 rows × 125 columns: pitch 128 (three padding columns), a partial last band."""
    cfg = fused.PipeConfig(margins=(3, 5, 2, 7), scale_min=0.2, scale_max=0.6)
    src, bgs, plan = SR.scene_noise_batch(fused, 3, 2, 90, 110, 3, 97, 125, cfg, 125)
    return src, bgs, plan, cfg


def given(fused, src_hw, bg_hw, n_bg, cfg, K, specs, place):
    """Plan scenes from specs = [(angle, sym, bg_index, ratio)] per overlay item;
    `place(ov)` returns the (x, y) of every item from the overlays' (w, h)."""
    S = len(specs) // K
    sizes = fused.plan_scenes(src_hw, S, K, bg_hw, n_bg, cfg,
                              params=[fused.ItemParams(a, s, b, r, 0, 0) for a, s, b, r in specs])
    ov = list(zip(sizes.items["ov_w"].tolist(), sizes.items["ov_h"].tolist()))
    return fused.plan_scenes(src_hw, S, K, bg_hw, n_bg, cfg,
                             params=[fused.ItemParams(a, s, b, r, x, y)
                                     for (a, s, b, r), (x, y) in zip(specs, place(ov))])


def neighbour_scenes(fused):
    """The placement of tests/test_gpu_scenes.test_neighbours_share_a_group_and_a_band."""
    cfg = fused.PipeConfig(margins=(0.05, 9, 0.1, 3))
    rng = np.random.default_rng(41)
    src = rng.integers(0, 256, (4, 150, 170, 3), np.uint8)
    bgs = rng.integers(0, 256, (2, 128, 160, 3), np.uint8)
    specs = [(33.0, "o", 0, 0.22), (127.0, "h", 0, 0.25), (250.0, "v", 1, 0.2), (75.0, "hv", 1, 0.23)]

    def place(ov):
        (w0, h0), (w1, h1), (w2, h2), (w3, h3) = ov
        x0 = 21 if (21 + w0) % 16 else 22        # layer 1 starts inside layer 0's last 16-pixel group
        y2 = 9 if (9 + h2) % 16 else 10          # layer 1 starts inside layer 0's last 16-row band
        return [(x0, 37), (x0 + w0, 42), (50, y2), (53, y2 + h2)]

    return src, bgs, given(fused, (150, 170), (128, 160), 2, cfg, 2, specs, place), cfg


def cover_scenes(fused):
    """The structured sources of tests/test_gpu_scenes.test_full_partial_and_faint_cover:
    scene 0 layer 1 covers all of layer 0, scene 1 its left part, scene 2's
    layer 1 is a line that is faint once downscaled."""
    cfg = fused.PipeConfig(margins=R.STRUCT_MARGINS, hsv_ranges=list(R.STRUCT_RANGES))
    H, W, K = 140, 120, 2
    rng = np.random.default_rng(5)
    src = np.empty((6, H, W, 3), np.uint8)
    src[:] = (90, 120, 60)

    def plant(i, r0, r1, c0, c1):
        src[i, r0:r1, c0:c1] = rng.integers(160, 256, (r1 - r0, c1 - c0, 3))

    plant(0, 50, 80, 40, 70), plant(1, 10, 130, 10, 110)
    plant(2, 50, 80, 40, 70), plant(3, 10, 130, 10, 55)
    plant(4, 50, 80, 40, 70), plant(5, 10, 130, 55, 56)
    bgs = rng.integers(0, 256, (2, 96, 128, 3), np.uint8)
    specs = [(0.0, "o", s % 2, 0.5) for s in range(3) for _ in range(K)]
    return src, bgs, given(fused, (H, W), (96, 128), 2, cfg, K, specs, lambda ov: [(30, 20)] * 6), cfg


def edge_scenes(fused):
    """Overlays ending in the background's last row and column (tests/test_gpu_scenes.py, case 12)."""
    cfg = fused.PipeConfig(margins=(0.05, 9, 0.1, 3))
    rng = np.random.default_rng(43)
    src = rng.integers(0, 256, (4, 150, 170, 3), np.uint8)
    bgs = rng.integers(0, 256, (2, 128, 160, 3), np.uint8)
    specs = [(61.0, "o", 1, 0.3), (200.0, "h", 1, 0.25), (310.0, "v", 0, 0.28), (15.0, "hv", 0, 0.35)]

    def place(ov):
        (w0, h0), _, _, (w3, h3) = ov
        return [(160 - w0, 128 - h0), (70, 60), (64, 48), (160 - w3, 128 - h3)]

    return src, bgs, given(fused, (150, 170), (128, 160), 2, cfg, 2, specs, place), cfg


def layered_scene(fused, K):
    """One scene of K noise layers, 64×80 sources on a 96×128 background, every
    rectangle holding composite pixel (40, 30): all of them overlap."""
    cfg = fused.PipeConfig(margins=(2, 2, 2, 2))
    rng = np.random.default_rng(88)
    src = rng.integers(0, 256, (K, 64, 80, 3), np.uint8)
    bgs = rng.integers(0, 256, (1, 96, 128, 3), np.uint8)
    specs = [(17.0 + 37.0 * k, ("o", "h", "v", "hv")[k % 4], 0, 0.35 + 0.02 * k) for k in range(K)]
    plan = given(fused, (64, 80), (96, 128), 1, cfg, K, specs, lambda ov: [(10 + 3 * k, 5 + 2 * k) for k in range(K)])
    return src, bgs, plan, cfg
