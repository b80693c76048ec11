"""CPU: the visibility-map reference (tests/scene_mask_refs.scene_map) against
the label rows' reference (tests/scene_refs.scene_rows), the conditions the
GPU tests of tests/test_gpu_scene_masks.py rely on, and the host helpers
fused.instance_ids / fused.scene_instance_masks on hand-made maps."""
import numpy as np
import pytest

from tests import scene_mask_refs as MR
from tests import scene_refs as SR

BATCHES = {
    "noise": MR.noise_scenes, "odd": MR.odd_scenes, "neighbours": MR.neighbour_scenes, "cover": MR.cover_scenes,
    "edge": MR.edge_scenes, "eight": lambda fused: MR.layered_scene(fused, 8),
}


@pytest.fixture(scope="module")
def fused():
    from image_processor_pipeline_amd import fused as F
    return F


@pytest.fixture(scope="module")
def batches(fused):
    out = {}
    for name, make in BATCHES.items():
        src, bgs, plan, cfg = make(fused)
        out[name] = (plan, SR.scene_overlays(src, plan, cfg))
    return out


@pytest.mark.parametrize("name", sorted(BATCHES))
@pytest.mark.parametrize("alpha_min,cover_min", MR.LEVELS)
def test_reference_map_has_the_counts_and_boxes_of_the_rows(batches, name, alpha_min, cover_min):
    plan, overlays = batches[name]
    vis = MR.scene_map(plan, overlays, alpha_min, cover_min)
    assert vis.dtype == np.uint8 and vis.shape == (plan.n_scenes, plan.bg_h, MR.pitch_of(plan.bg_w))
    assert not vis[:, :, plan.bg_w:].any()
    assert not (vis >> plan.per_scene).any()                       # no bit of a layer the scene does not have
    rows = SR.scene_rows(plan, overlays, alpha_min, cover_min)
    assert np.array_equal(MR.map_rows(vis, plan.per_scene), rows[..., [0, 1, 2, 3, 5]])


def test_noise_batch_meets_the_conditions_of_the_gpu_tests(batches):
    """MASK_NOISE_SEED: checked here on the reference alone."""
    plan, overlays = batches["noise"]
    K, prm = plan.per_scene, plan.params
    vis = MR.scene_map(plan, overlays, 1, 128)
    assert (np.unpackbits(vis[..., None], axis=-1).sum(axis=-1) >= 2).any()      # a byte with two bits
    hidden = 0
    for i, ov in enumerate(overlays):                                             # present, bit clear: hidden
        h, w = ov.shape[:2]
        bit = (vis[i // K, prm[i].y:prm[i].y + h, prm[i].x:prm[i].x + w] >> (i % K)) & 1
        hidden += int(((ov[..., 3] >= 1) & (bit == 0)).sum())
    assert hidden > 0
    for k in range(3):
        assert ((vis >> k) & 1).any(), k
    inside = MR.rects(plan, overlays)
    none = MR.scene_map(plan, overlays, 255, 1)[:, :, :plan.bg_w]
    assert (inside & (none == 0)).any()                                          # in a rectangle, no bit at all
    # the layer the no-plane test drops is a later layer that covers something
    widest = max(ov.shape[1] for ov in overlays)
    dropped = MR.scene_map(plan, overlays, 1, 128, max_ov=(widest - 1, plan.pipe.max_ov_h))
    assert widest == plan.pipe.max_ov_w and not np.array_equal(dropped, vis)
    gone = [i for i, ov in enumerate(overlays) if ov.shape[1] == widest]
    for i in gone:
        assert not ((dropped[i // K] >> (i % K)) & 1).any()
    assert any(int(((dropped[i // K] >> k) & 1).sum()) > int(((vis[i // K] >> k) & 1).sum())
               for i in gone for k in range(i % K))                               # it hides nothing any more


def test_structured_and_layered_batches_meet_their_conditions(batches):
    plan, overlays = batches["cover"]
    vis = MR.scene_map(plan, overlays, 1, 128)
    assert not (vis[0] & 1).any() and (vis[0] & 2).any()             # scene 0: layer 0 wholly hidden
    faint = overlays[5][..., 3]
    assert 32 <= faint.max() < 128
    line = np.zeros(vis.shape[1:], bool)
    line[20:20 + faint.shape[0], 30:30 + faint.shape[1]] = faint >= 32
    assert line.any() and (vis[2][line & (vis[2] & 2 > 0)] == 3).any()    # both bits under the faint line
    low = MR.scene_map(plan, overlays, 1, 32)
    assert not (low[2][line] & 1).any() and (vis[2][line] & 1).any()  # at cover_min 32 the line covers layer 0
    plan, overlays = batches["neighbours"]
    assert (np.unpackbits(MR.scene_map(plan, overlays, 1, 128)[..., None], axis=-1).sum(axis=-1) <= 1).all()
    plan, overlays = batches["eight"]
    assert plan.per_scene == 8 and plan.n_scenes == 1
    for prm, ov in zip(plan.params, overlays):                       # every rectangle holds (40, 30)
        assert prm.x <= 40 < prm.x + ov.shape[1] and prm.y <= 30 < prm.y + ov.shape[0]
    assert (MR.scene_map(plan, overlays, 1, 128) & 128).any()


# --- host helpers on hand-made maps ---------------------------------------------------------
HAND = np.zeros((3, 4, 6), np.uint8)
HAND[0, 1, 1:4] = [1, 3, 2]          # a byte with two bits
HAND[0, 2, 2] = 1
HAND[2, 0, 5] = 128                  # bit 7
HAND[2, 3, 0] = 128 | 1
HAND[2, 2, 3] = 4 | 2
# scene 1 stays all zero


def test_instance_ids(fused):
    torch = pytest.importorskip("torch")
    exp = np.zeros_like(HAND)
    exp[0, 1, 1:4] = [1, 2, 2]
    exp[0, 2, 2] = 1
    exp[2, 0, 5] = 8
    exp[2, 3, 0] = 8
    exp[2, 2, 3] = 3
    got = fused.instance_ids(HAND)
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and np.array_equal(got, exp)
    t = fused.instance_ids(torch.from_numpy(HAND))
    assert isinstance(t, torch.Tensor) and t.dtype == torch.uint8 and t.shape == (3, 4, 6)
    assert np.array_equal(t.numpy(), exp)
    every = fused.instance_ids(np.arange(256, dtype=np.uint8))
    assert every.tolist() == [0] + [1 + int(np.log2(v)) for v in range(1, 256)]
    assert fused.instance_ids(HAND[:, :, ::2]).shape == (3, 4, 3)    # any shape, strided views too
    with pytest.raises(ValueError):
        fused.instance_ids(HAND.astype(np.int32))


def test_scene_instance_masks(fused):
    K = 8
    rows = np.full((3, K, 6), -1, np.int32)
    rows[..., 4:] = 0
    counts = MR.map_rows(HAND, K)
    rows[..., :4], rows[..., 5] = counts[..., :4], counts[..., 4]
    masks = fused.scene_instance_masks(HAND, rows)
    assert [len(m) for m in masks] == [K, K, K]
    assert all(m is None for m in masks[1])                          # the all-zero scene
    assert [m is None for m in masks[0]] == [False, False] + [True] * 6
    m00, m01 = masks[0][0], masks[0][1]
    assert m00.dtype == bool and m00.tolist() == [[True, True], [False, True]]     # box (1, 1, 3, 3)
    assert m01.tolist() == [[True, True]]                                          # box (2, 1, 4, 2)
    m27 = masks[2][7]
    assert m27.shape == (4, 6) and int(m27.sum()) == 2 and m27[0, 5] and m27[3, 0]
    assert masks[2][0].tolist() == [[True]] and masks[2][1].tolist() == [[True]] and masks[2][2].tolist() == [[True]]
    # every mask, put back at its box, rebuilds the map
    back = np.zeros_like(HAND)
    for s in range(3):
        for k in range(K):
            if masks[s][k] is not None:
                x0, y0, x1, y1 = rows[s, k, :4]
                back[s, y0:y1, x0:x1] |= (masks[s][k].astype(np.uint8) << k).astype(np.uint8)
    assert np.array_equal(back, HAND)
    with pytest.raises(ValueError):
        fused.scene_instance_masks(HAND, rows[0])
    with pytest.raises(ValueError):
        fused.scene_instance_masks(HAND[:2], rows)
    with pytest.raises(ValueError):
        fused.scene_instance_masks(HAND, np.concatenate([rows, rows[:, :1]], axis=1))     # nine layers
