"""CPU: the run-length reference (tests/rle_refs.py) — its two encoders against
each other, the definition's sums, the handmade maps — the host helpers
fused.rle_counts_string / rle_counts_from_string / rle_decode /
scene_coco_annotations, and — on the reference alone — the conditions the GPU
tests of tests/test_gpu_rle.py lean on."""
import json

import numpy as np
import pytest

from tests import contour_refs as C
from tests import rle_refs as R
from tests import scene_mask_refs as MR
from tests import scene_refs as SR


@pytest.fixture(scope="module")
def fused():
    from image_processor_pipeline_amd import fused as F
    return F


def _random_masks():
    rng = np.random.default_rng(31)
    yield np.zeros((5, 7), bool)
    yield np.ones((5, 7), bool)
    yield np.zeros((1, 1), bool)
    yield np.ones((1, 1), bool)
    for _ in range(300):
        h, w = rng.integers(1, 15, 2)
        yield rng.random((h, w)) < rng.choice([0.05, 0.3, 0.5, 0.7, 0.95])


def test_the_two_encoders_agree_and_hold_the_definition(fused):
    n = 0
    for m in _random_masks():
        c = R.encode(m)
        assert c.dtype == np.uint32 and np.array_equal(c, R.encode_diff(m))
        assert int(c.sum()) == m.size and int(c[1::2].sum()) == int(m.sum())
        assert (c[1:] > 0).all()                                              # only the first count may be 0
        assert (c[0] == 0) == bool(m[0, 0])
        back = fused.rle_decode(c, *m.shape)
        assert back.dtype == bool and back.shape == m.shape and np.array_equal(back, m)
        assert np.array_equal(fused.rle_decode(fused.rle_counts_string(c), *m.shape), m)
        n += 1
    assert n >= 300
    assert R.encode(np.zeros((5, 7), bool)).tolist() == [35] and R.encode(np.ones((5, 7), bool)).tolist() == [0, 35]
    with pytest.raises(ValueError):
        fused.rle_decode([3, 4], 2, 4)                                        # does not sum to N


KNOWN = [([0, 6], "06"), ([5, 1], "51"), ([100000, 3, 70000, 2, 5], "PeQ33`[T2OedkM")]


def test_counts_string(fused):
    for counts, s in KNOWN:
        assert fused.rle_counts_string(counts) == s == R.to_string(counts)
        assert fused.rle_counts_from_string(s).tolist() == counts == R.from_string(s).tolist()
    rng = np.random.default_rng(32)
    seqs = [rng.integers(0, hi, int(rng.integers(1, 40))) for hi in (4, 40, 1 << 10, 1 << 15, 1 << 20, 1 << 30)
            for _ in range(40)]
    seqs += [np.array(v) for v in ([0], [1 << 15], [(1 << 15) - 1, 1, 1 << 15], [1, 2, 3, (1 << 30) - 1, 0, 1],
                                   [7, 1 << 29, 9, 1, 1 << 29, (1 << 29) + 15, 16, 31, 32],     # large negative deltas
                                   [5, 20, 5, 4, 21, 36, 5, 4, 20])]                            # deltas of -16, 16, 32
    for c in seqs:
        s = fused.rle_counts_string(c.astype(np.uint32))
        assert isinstance(s, str) and s == R.to_string(c) and all(48 <= ord(ch) < 112 for ch in s)
        got = fused.rle_counts_from_string(s)
        assert got.dtype == np.uint32 and got.tolist() == c.tolist() == R.from_string(s).tolist()
    assert fused.rle_counts_string([]) == "" and fused.rle_counts_from_string("").tolist() == []
    for bad in ("P", "0 ", "\x7f"):                                           # ends inside a count; not a code character
        with pytest.raises(ValueError):
            fused.rle_counts_from_string(bad)
    with pytest.raises(ValueError):
        fused.rle_counts_string([3, -1])
    with pytest.raises(ValueError):
        fused.rle_counts_string([[3, 1]])


def test_handmade_maps_are_what_they_are_for():
    by = {c.name: c for c in R.all_handmade()}
    ref = {n: R.case_reference(c) for n, c in by.items()}
    assert ref["first_pixel"][1][0].tolist() == [0, 1, 9 * 21 - 1]
    assert ref["last_pixel"][1][0].tolist() == [9 * 21 - 1, 1]
    assert ref["full_height_bar"][1][0].tolist() == [21, 21, 98]
    assert ref["merge_one_boundary"][1][0].tolist() == [9 * 7 + 4, 5, 9 * 7 + 5]
    assert by["full_height_ends"].rows[:, [1, 3]].tolist() == [[0, 6], [0, 6]]
    assert ref["full_height_ends"][1][0].tolist() == [30, 8, 1, 15, 66] and by["full_height_ends"].rows[1, 2] == 20
    assert ref["full_height_ends"][1][1].tolist() == [102, 6, 1, 11]
    assert by["bottom_rows"].rows[0, :4].tolist() == [3, 5, 24, 8]
    comb = by["comb_130"]
    assert comb.rows[0, :4].tolist() == [191, 1, 321, 10] and ref["comb_130"][0][0].tolist() == [130 * 10 + 1, 130 * 5]
    assert (comb.rows[0, 2] - 1) // 64 - comb.rows[0, 0] // 64 >= 2               # it meets three 64-column groups or more
    assert comb.rows[0, 0] // 256 != (comb.rows[0, 2] - 1) // 256
    # over the full height every column's last run merges with the next column's first
    assert ref["comb_full_height"][0][0].tolist() == [130 * 8 + 3, 130 * 5]
    assert by["comb_300"].rows[0, 2] - by["comb_300"].rows[0, 0] == 300
    assert len(ref["sparse_wide"][1][0]) == 9                                     # four lone pixels; (255, 3) and (256, 3) do not merge
    assert by["one_row"].bg_h == 1 and ref["one_row"][1][0].tolist() == [3, 6, 2, 1, 24, 1]
    assert by["one_column"].bg_w == 1 and ref["one_column"][1][0].tolist() == [3, 6, 2, 1, 24, 1]
    hdr, counts = ref["empty_box_and_outside"]
    assert hdr.tolist() == [[1, 0], [2 + 1, 1], [0, 0]] and counts[0].tolist() == [60] and len(counts[2]) == 0
    # the tracer's cases: a {0, 0} descriptor between live ones, and one scene_layer does not map
    assert ref["empty_and_unmapped"][0][[1, 3, 4]].tolist() == [[0, 0]] * 3
    for name, (hdr, counts) in ref.items():
        case = by[name]
        for i, c in enumerate(counts):
            assert hdr[i, 0] == len(c)
            if len(c):
                s, k = case.scene_layer[i]
                m = R.mask_of(case.vis, case.rows[i], s, k)[:, :case.bg_w]
                assert np.array_equal(c, R.encode_diff(m)) and int(c.sum()) == case.bg_w * case.bg_h
                assert int(c[1::2].sum()) == hdr[i, 1] == int(m.sum())


def _rows(entries, S, K):
    rows = np.full((S, K, 6), -1, np.int32)
    rows[..., 4:] = 0
    for (s, k), r in entries.items():
        rows[s, k] = r
    return rows


def test_scene_coco_annotations(fused):
    bg_w, bg_h = 12, 7
    rows = _rows({(0, 0): (1, 2, 4, 5, 9, 9), (0, 1): (3, 0, 6, 2, 10, 4), (1, 1): (0, 0, 12, 7, 84, 84)}, 2, 2)
    masks = {(0, 0): (slice(2, 5), slice(1, 4)), (1, 1): (slice(0, 7), slice(0, 12))}
    rles = [[None, None], [None, None]]
    for (s, k), (ys, xs) in masks.items():
        m = np.zeros((bg_h, bg_w), bool)
        m[ys, xs] = True
        rles[s][k] = R.encode(m)
    m = np.zeros((bg_h, bg_w), bool)
    m[0, 3] = m[1, 3] = m[0, 5] = m[1, 5] = True
    rles[0][1] = R.encode(m)
    ids = [5, 6, 7, 8]
    anns = fused.scene_coco_annotations(rles, rows, bg_w, bg_h, class_ids=ids, min_visible=0.5)
    lines = fused.scene_labels(rows, bg_w, bg_h, class_ids=ids, min_visible=0.5)
    assert [len(a) for a in anns] == [len(x) for x in lines] == [1, 1]            # (0, 1) is 40 % visible: filtered
    a = anns[0][0]
    assert a == {"id": 1, "image_id": 0, "category_id": 5, "bbox": [1, 2, 3, 3], "area": 9, "iscrowd": 0,
                 "segmentation": {"size": [7, 12], "counts": R.to_string(rles[0][0])}}
    assert anns[1][0]["id"] == 2 and anns[1][0]["category_id"] == 8 and anns[1][0]["segmentation"]["counts"] == "0d2"
    every = fused.scene_coco_annotations(rles, rows, bg_w, bg_h, class_ids=ids, compressed=False,
                                         image_ids=[40, 41], first_id=100)
    assert [[x["id"] for x in a] for a in every] == [[100, 101], [102]]
    assert [[x["image_id"] for x in a] for a in every] == [[40, 40], [41]]
    assert every[0][1]["segmentation"]["counts"] == rles[0][1].tolist() and every[0][1]["area"] == 4
    for res in (anns, every):
        back = json.loads(json.dumps(res))
        assert back == res
        for sc in res:
            for x in sc:
                assert all(type(v) is int for v in (x["id"], x["image_id"], x["category_id"], x["area"], x["iscrowd"]))
                assert all(type(v) is int for v in x["bbox"] + x["segmentation"]["size"])
                cnt = x["segmentation"]["counts"]
                assert type(cnt) is str or all(type(v) is int for v in cnt)
                mask = fused.rle_decode(cnt, bg_h, bg_w)
                assert int(mask.sum()) == x["area"]
                ys, xs = np.nonzero(mask)
                assert [xs.min(), ys.min(), xs.max() + 1 - xs.min(), ys.max() + 1 - ys.min()] == x["bbox"]
    # an overlay that gets a line but has no encoding is refused; so are mismatched shapes
    with pytest.raises(ValueError, match="scene 1 layer 1"):
        fused.scene_coco_annotations([rles[0], [None, None]], rows, bg_w, bg_h)
    with pytest.raises(ValueError):
        fused.scene_coco_annotations(rles[:1], rows, bg_w, bg_h)
    with pytest.raises(ValueError):
        fused.scene_coco_annotations(rles, rows, bg_w, bg_h, image_ids=[1])
    with pytest.raises(ValueError):
        fused.scene_coco_annotations(rles, rows, bg_w, bg_h, class_ids=[1, 2])


# --- on the reference alone: what the GPU tests' scene batches hold ------------------------------------------
@pytest.fixture(scope="module")
def batches(fused):
    out = {}
    for name, (src, bgs, plan, cfg) in R.scene_batches(fused).items():
        out[name] = (plan, SR.scene_overlays(src, plan, cfg))
    return out


def test_scene_batches_meet_the_conditions_of_the_gpu_tests(fused, batches):
    hidden = split_or_hole = corner = 0
    for name, (plan, overlays) in batches.items():
        rles, rows, vis = R.scene_reference(plan, overlays, 1, 128)
        _, polys, stats, c_rows, _ = C.scene_reference(plan, overlays, 1, 128)
        assert np.array_equal(rows, c_rows)
        for s in range(plan.n_scenes):
            for k in range(plan.per_scene):
                if rles[s][k] is None:
                    hidden += int(rows[s, k, 4] > 0)                            # present, but nothing of it visible
                    continue
                mask = fused.rle_decode(rles[s][k], plan.bg_h, plan.bg_w)
                assert int(mask.sum()) == rows[s, k, 5]
                cyc = stats[s][k]
                if len(cyc) > 1:                                                # a second part, or a hole
                    split_or_hole += 1
                    assert not np.array_equal(C.raster(polys[s][k], mask.shape).astype(bool), mask)
                corner += int(rows[s, k, 2] == plan.bg_w and rows[s, k, 3] == plan.bg_h)
    assert hidden > 0 and split_or_hole > 0 and corner > 0
    plan, overlays = batches["cover"]
    assert R.scene_reference(plan, overlays, 1, 128)[0][0][0] is None           # scene 0: layer 0 wholly hidden
    assert batches["single"][0].per_scene == 1 and batches["eight"][0].per_scene == 8
    assert batches["odd"][0].bg_w == 125 and MR.pitch_of(125) == 128
