"""CPU: the amodal reference (tests/amodal_refs.py) against its own invariants
and the visible-label references, the conditions the GPU tests of
tests/test_gpu_scene_amodal.py rely on, the host formatter
fused.scene_amodal_annotations on a hand-made case, and the argument checks of
the new SceneRunner methods that fire before any launch."""
import json
from types import SimpleNamespace as NS

import numpy as np
import pytest

from tests import amodal_refs as A
from tests import scene_mask_refs as MR
from tests import scene_refs as SR

# MR.MASK_NOISE_SEED (23) meets the conditions below: no seed of this file's own is needed.
BATCHES = {
    "noise": MR.noise_scenes, "odd": MR.odd_scenes, "neighbours": MR.neighbour_scenes, "cover": MR.cover_scenes,
    "edge": MR.edge_scenes, "eight": lambda fused: MR.layered_scene(fused, 8), "pair": A.covered_pair,
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


def check_invariants(plan, amap, arows, occ):
    """What include/ipp.h promises of any result, whatever produced it."""
    S, K = plan.n_scenes, plan.per_scene
    assert amap.dtype == np.uint8 and amap.shape == (S, plan.bg_h, MR.pitch_of(plan.bg_w))
    assert arows.shape == (S, K, 6) and occ.shape == (S, 2, K, K)
    assert not amap[:, :, plan.bg_w:].any() and not (amap >> K).any()
    covers, hides = occ[:, 0].astype(np.int64), occ[:, 1].astype(np.int64)
    low = np.tril_indices(K, -1)
    assert not covers[:, low[0], low[1]].any() and not hides[:, low[0], low[1]].any()      # j < k: 0
    assert (hides <= covers).all() and (occ >= 0).all()
    assert np.array_equal(hides.sum(axis=2), np.diagonal(covers, axis1=1, axis2=2))       # a partition of the present
    assert np.array_equal(np.diagonal(covers, axis1=1, axis2=2), arows[..., 4])
    assert np.array_equal(np.diagonal(hides, axis1=1, axis2=2), arows[..., 5])
    assert np.array_equal(MR.map_rows(amap, K), arows[..., :5])                            # the bits' boxes and counts


@pytest.mark.parametrize("name", sorted(BATCHES))
@pytest.mark.parametrize("alpha_min,cover_min", MR.LEVELS)
def test_reference_invariants(batches, name, alpha_min, cover_min):
    plan, overlays = batches[name]
    amap, arows, occ = A.reference(plan, overlays, alpha_min, cover_min)
    check_invariants(plan, amap, arows, occ)
    rows = SR.scene_rows(plan, overlays, alpha_min, cover_min)
    assert np.array_equal(arows[..., 4:6], rows[..., 4:6])                                  # area and visible
    # the visible map is the presence map minus what a later layer covers: never a bit more
    vis = MR.scene_map(plan, overlays, alpha_min, cover_min)
    assert not (vis & ~amap).any()
    # the visible box lies inside the amodal one
    has = rows[..., 0] >= 0
    assert (arows[has][:, :2] <= rows[has][:, :2]).all() and (arows[has][:, 2:4] >= rows[has][:, 2:4]).all()


def test_noise_batch_meets_the_conditions_of_the_gpu_tests(batches):
    plan, overlays = batches["noise"]
    K = plan.per_scene
    assert K >= 3
    _, arows, occ = A.reference(plan, overlays, 1, 128)
    up = np.triu_indices(K, 1)
    covers, hides = occ[:, 0][:, up[0], up[1]], occ[:, 1][:, up[0], up[1]]
    assert (covers > 0).any()
    assert ((hides > 0) & (hides < covers)).any()              # a pixel two later layers both cover
    assert ((arows[..., 5] > 0) & (arows[..., 5] < arows[..., 4])).any()
    # the amodal box differs from the visible one somewhere: the labels are not the visible ones renamed
    assert not np.array_equal(arows[..., :4], SR.scene_rows(plan, overlays, 1, 128)[..., :4])
    # the layer the no-plane test drops is a later layer that covers something
    widest = max(ov.shape[1] for ov in overlays)
    assert widest == plan.pipe.max_ov_w
    gone = [i for i, ov in enumerate(overlays) if ov.shape[1] == widest]
    assert gone and all(i % K > 0 for i in gone)
    amap2, arows2, occ2 = A.reference(plan, overlays, 1, 128, max_ov=(widest - 1, plan.pipe.max_ov_h))
    check_invariants(plan, amap2, arows2, occ2)
    for i in gone:
        s, k = divmod(i, K)
        assert occ[s, 0, :k, k].any()                          # it covered something
        assert arows2[s, k].tolist() == A.ABSENT and not occ2[s, :, k, :].any() and not occ2[s, :, :, k].any()
        assert not ((amap2[s] >> k) & 1).any()
    # the unmapped descriptors of the GPU test: items 0 (scene 0 layer 0) and 5 (scene 1 layer 2)
    amap3, arows3, occ3 = A.reference(plan, overlays, 1, 128, alone=(0, 5))
    assert arows3[0, 0, 4] == arows3[0, 0, 5] > arows[0, 0, 5]     # alone: nothing hides it
    assert arows3[1, 2, 4] > 0 and occ[1, 0, :2, 2].any()          # it covered something when mapped
    assert not occ3[0, :, 0, :].any() and not occ3[1, :, :, 2].any() and not ((amap3[1] >> 2) & 1).any()
    assert np.array_equal(arows3[2:], arows[2:])


def test_covered_pair_meets_its_conditions(batches):
    plan, overlays = batches["pair"]
    rows = SR.scene_rows(plan, overlays, 1, 128)
    _, arows, occ = A.reference(plan, overlays, 1, 128)
    assert rows[0, 0].tolist()[:4] == [-1, -1, -1, -1] and rows[0, 0, 5] == 0 and rows[0, 0, 4] > 0
    area = int(arows[0, 0, 4])
    assert arows[0, 0, 0] >= 0 and arows[0, 0, 5] == 0
    assert occ[0, 0, 0, 1] == occ[0, 1, 0, 1] == area and occ[0, 1, 0, 0] == 0
    assert arows[0, 1, 4] == arows[0, 1, 5] > 0                # the upper overlay is whole


def test_layered_and_neighbour_batches_meet_their_conditions(batches):
    plan, overlays = batches["eight"]
    for a, c in MR.LEVELS[:2]:
        amap, _, occ = A.reference(plan, overlays, a, c)
        assert (amap & 128).any() and occ[0, 0, 0, 1:].all()   # every later layer covers some of layer 0
    plan, overlays = batches["neighbours"]
    amap, arows, occ = A.reference(plan, overlays, 1, 128)
    assert not occ[:, :, 0, 1].any()                           # they touch, nobody covers
    assert np.array_equal(amap, MR.scene_map(plan, overlays, 1, 128))
    assert np.array_equal(arows, SR.scene_rows(plan, overlays, 1, 128))


# --- scene_amodal_annotations on a hand-made case ------------------------------------------------------
def _hand():
    """Two scenes of two layers on a 6-wide, 4-high background.  Scene 0: layer 0 = columns 1..3 of rows 1..2,
    layer 1 covers its columns 2..3; scene 1: only layer 1, one pixel."""
    from image_processor_pipeline_amd import fused as F
    bw, bh = 6, 4
    full = np.zeros((2, 2, bh, bw), bool)
    full[0, 0, 1:3, 1:4] = True
    full[0, 1, 0:3, 2:5] = True
    full[1, 1, 3, 5] = True
    vis = full.copy()
    vis[0, 0] &= ~full[0, 1]

    def enc(m):
        """Column-major runs, zeros first; None for an empty mask."""
        if not m.any():
            return None
        counts, cur, run = [], False, 0
        for v in m.T.reshape(-1):
            if bool(v) == cur:
                run += 1
            else:
                counts.append(run)
                cur, run = bool(v), 1
        return np.array(counts + [run], np.uint32)

    arles = [[enc(full[s, k]) for k in range(2)] for s in range(2)]
    vrles = [[enc(vis[s, k]) for k in range(2)] for s in range(2)]
    for s in range(2):
        for k in range(2):
            for rl, m in ((arles, full), (vrles, vis)):
                if m[s, k].any():
                    assert np.array_equal(F.rle_decode(rl[s][k], bh, bw), m[s, k])
    arows = np.array([[[1, 1, 4, 3, 6, 2], [2, 0, 5, 3, 9, 9]], [A.ABSENT, [5, 3, 6, 4, 1, 1]]], np.int32)
    rows = np.array([[[1, 1, 2, 3, 6, 2], [2, 0, 5, 3, 9, 9]], [A.ABSENT, [5, 3, 6, 4, 1, 1]]], np.int32)
    occ = np.array([[[[6, 4], [0, 9]], [[2, 4], [0, 9]]], [[[0, 0], [0, 1]], [[0, 0], [0, 1]]]], np.int32)
    return arles, vrles, arows, rows, occ, bw, bh


def test_annotations_key_by_key(fused):
    arles, vrles, arows, rows, occ, bw, bh = _hand()
    anns = fused.scene_amodal_annotations(arles, vrles, arows, rows, occ, bw, bh, class_ids=[7, 8, 9, 10],
                                          image_ids=[40, 41], first_id=100)
    assert [len(a) for a in anns] == [2, 1]
    a = anns[0][0]
    assert set(a) == {"id", "image_id", "category_id", "iscrowd", "bbox", "area", "segmentation", "visible_bbox",
                      "visible_area", "visible_mask", "occlude_rate", "layer", "occluders"}
    assert (a["id"], a["image_id"], a["category_id"], a["iscrowd"], a["layer"]) == (100, 40, 7, 0, 0)
    assert a["bbox"] == [1, 1, 3, 2] and a["area"] == 6
    assert a["visible_bbox"] == [1, 1, 1, 2] and a["visible_area"] == 2
    assert a["occlude_rate"] == 1 - 2 / 6 and a["occluders"] == [1]
    assert a["segmentation"]["size"] == [bh, bw] and a["visible_mask"]["size"] == [bh, bw]
    assert isinstance(a["segmentation"]["counts"], str)
    assert int(fused.rle_decode(a["segmentation"]["counts"], bh, bw).sum()) == 6
    assert int(fused.rle_decode(a["visible_mask"]["counts"], bh, bw).sum()) == 2
    b = anns[0][1]
    assert (b["id"], b["category_id"], b["layer"], b["occluders"], b["occlude_rate"]) == (101, 8, 1, [], 0.0)
    assert b["segmentation"] == b["visible_mask"] and b["bbox"] == b["visible_bbox"] == [2, 0, 3, 3]
    c = anns[1][0]
    assert (c["id"], c["image_id"], c["category_id"], c["layer"]) == (102, 41, 10, 1)
    # the lists align with every other label of the scene
    assert [len(x) for x in fused.scene_labels(rows, bw, bh)] == [2, 1]
    assert [[d["id"] for d in sc] for sc in fused.scene_coco_annotations(vrles, rows, bw, bh, first_id=100)] == \
        [[d["id"] for d in sc] for sc in anns]
    # min_visible drops the half-hidden overlay here as it does there
    half = fused.scene_amodal_annotations(arles, vrles, arows, rows, occ, bw, bh, min_visible=0.5)
    assert [[d["layer"] for d in sc] for sc in half] == [[1], [1]] and half[0][0]["id"] == 1
    # uncompressed counts are plain lists
    raw = fused.scene_amodal_annotations(arles, vrles, arows, rows, occ, bw, bh, compressed=False)
    assert raw[0][0]["segmentation"]["counts"] == [int(v) for v in arles[0][0]]
    assert raw[0][0]["visible_mask"]["counts"] == [int(v) for v in vrles[0][0]]


def test_annotations_json_round_trip(fused):
    arles, vrles, arows, rows, occ, bw, bh = _hand()
    for compressed in (True, False):
        anns = fused.scene_amodal_annotations(arles, vrles, arows, rows, occ, bw, bh, compressed=compressed)
        assert json.loads(json.dumps(anns)) == anns


def test_annotations_refuse_what_they_cannot_write(fused):
    arles, vrles, arows, rows, occ, bw, bh = _hand()
    f = fused.scene_amodal_annotations
    no_a = [[None, arles[0][1]], arles[1]]
    no_v = [[vrles[0][0], None], vrles[1]]
    with pytest.raises(ValueError, match="amodal"):
        f(no_a, vrles, arows, rows, occ, bw, bh)
    with pytest.raises(ValueError, match="visible"):
        f(arles, no_v, arows, rows, occ, bw, bh)
    assert len(f(no_a, vrles, arows, rows, occ, bw, bh, min_visible=0.5)[0]) == 1      # no annotation, nothing missing
    small = arows.copy()
    small[0, 0, 4] = 1                                                                 # below its visible pixels
    bad = [dict(arles=arles[:1]), dict(vrles=[v[:1] for v in vrles]), dict(arows=arows[:, :1]), dict(arows=arows[0]),
           dict(rows=rows[..., :5]), dict(occ=occ[:, 0]), dict(occ=occ[:1]), dict(class_ids=[1, 2, 3]),
           dict(image_ids=[1]), dict(arows=small)]
    for kw in bad:
        a = dict(arles=arles, vrles=vrles, arows=arows, rows=rows, occ=occ)
        ids = {k: kw.pop(k) for k in ("class_ids", "image_ids") if k in kw}
        a.update(kw)
        with pytest.raises(ValueError):
            f(a["arles"], a["vrles"], a["arows"], a["rows"], a["occ"], bw, bh, **ids)


# --- the runner's checks that come before any launch ------------------------------------------------------
def _runner(fused, K=3):
    r = object.__new__(fused.SceneRunner)                  # no device: every check below comes first
    r.plan = NS(pipe=NS(bg_w=160, bg_h=128, max_ov_w=64, max_ov_h=64), n_scenes=2, per_scene=K, bg_w=160, bg_h=128)
    r._hpass_done = False
    return r


def test_runner_refuses_bad_arguments_before_any_launch(fused):
    from image_processor_pipeline_amd import _native as N
    r = _runner(fused)
    calls = (r.scene_amodal, r.scene_amodal_rles, r.scene_amodal_polygons)
    for call in calls:
        for kw in (dict(alpha_min=0), dict(alpha_min=256), dict(cover_min=0), dict(cover_min=1.5),
                   dict(alpha_min=None), dict(cover_min=True)):
            with pytest.raises(ValueError):
                call(**kw)
        with pytest.raises(N.NativeError, match="no H launch"):
            call()                                          # valid arguments: the H-launch guard, as scene_masks
    for m in ("yes", 1, None):
        with pytest.raises(ValueError, match="masks"):
            r.scene_amodal(masks=m)
    for kw in (dict(max_edges=3), dict(max_edges=True), dict(simplify=0.1), dict(simplify="1")):
        with pytest.raises(ValueError):
            r.scene_amodal_polygons(**kw)
    nine = _runner(fused, 9)
    for call in (nine.scene_amodal, nine.scene_amodal_rles, nine.scene_amodal_polygons):
        with pytest.raises(ValueError, match="8"):
            call()
    for a in ("yes", 1, None):
        with pytest.raises(ValueError, match="amodal"):
            r.run_labelled(None, None, None, amodal=a)
    with pytest.raises(ValueError, match="8"):
        nine.run_labelled(None, None, None, amodal=True)
    assert r._scratch is None and nine._scratch is None    # nothing was allocated


def test_the_entry_is_declared_bound_and_exported():
    from pathlib import Path
    from image_processor_pipeline_amd import _native as N
    header = (Path(__file__).resolve().parents[1] / "include" / "ipp.h").read_text()
    assert "int ipp_pipe_scene_amodal(" in header
    assert "ipp_pipe_scene_amodal" in N.SIGNATURES and len(N.SIGNATURES["ipp_pipe_scene_amodal"][1]) == 22
    lib = N.load()
    assert lib.ipp_pipe_scene_amodal.argtypes == N.SIGNATURES["ipp_pipe_scene_amodal"][1]
