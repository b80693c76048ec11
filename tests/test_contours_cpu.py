"""CPU: the contour reference (tests/contour_refs.py) held to scipy on random
and handmade masks, the host helpers fused.seg_label / scene_seg_labels /
scene_contour_capacity, and — on the reference alone — the conditions the GPU
tests of tests/test_gpu_contours.py lean on."""
import numpy as np
import pytest

from tests import contour_refs as C
from tests import scene_mask_refs as MR
from tests import scene_refs as SR

ndi = pytest.importorskip("scipy.ndimage")

EIGHT = np.ones((3, 3), int)


@pytest.fixture(scope="module")
def fused():
    from image_processor_pipeline_amd import fused as F
    return F


def _hold_to_scipy(fg):
    """The four properties of the definition, on one boolean image."""
    fg = np.asarray(fg, bool)
    cyc = C.cycles(fg)
    outer = [c for c in cyc if c["area2"] > 0]
    holes = [c for c in cyc if c["area2"] < 0]
    assert len(outer) + len(holes) == len(cyc)                         # no cycle of area 0
    assert sum(c["n_edges"] for c in cyc) == C.n_boundary_edges(fg)
    lab, n = ndi.label(fg, EIGHT)
    assert len(outer) == n
    # enclosed 4-connected background regions: those that do not reach the (padded) border
    bl, nb = ndi.label(~np.pad(fg, 1))
    assert len(holes) == nb - 1
    for c in outer:
        x, y = c["start"]
        comp = ndi.binary_fill_holes(lab == lab[y, x], structure=np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]]))
        fill = C.raster(c["verts"], fg.shape)
        assert set(np.unique(fill).tolist()) <= {0, 1}
        assert np.array_equal(fill.astype(bool), comp)
        assert c["area2"] == 2 * int(comp.sum())
        assert len(c["verts"]) % 2 == 0 and len(c["verts"]) >= 4


def test_reference_against_scipy_on_random_masks():
    rng = np.random.default_rng(2024)
    for t in range(200):
        h, w = rng.integers(1, 14, 2)
        _hold_to_scipy(rng.random((h, w)) < rng.choice([0.3, 0.5, 0.7]))


@pytest.mark.parametrize("case", C.handmade(), ids=lambda c: c.name)
def test_reference_against_scipy_on_the_handmade_maps(case):
    for i, (s, k) in enumerate(case.scene_layer):
        if case.rows[i, 0] < 0 or not (0 <= s < case.n_scenes and 0 <= k < case.per_scene):
            continue
        fg, _ = C.plane(case.vis, case.rows[i], s, k)
        _hold_to_scipy(fg)


def test_handmade_maps_are_what_they_are_for():
    by = {c.name: c for c in C.handmade()}
    h = {n: c.ref()[0] for n, c in by.items()}
    assert h["single_pixel"].tolist() == [[4, 1, 0, 4, 2, 9, 5, 0]]
    assert by["full_odd_plane"].pitch == 128 and h["full_odd_plane"][0].tolist() == [444, 1, 0, 4, 2 * 97 * 125, 0, 0, 0]
    assert by["full_odd_plane"].ref()[1][0].tolist() == [[0, 0], [125, 0], [125, 97], [0, 97]]
    hd, polys, st = by["diagonal_pair"].ref()
    assert hd[0, 1] == 1 and st[0][0]["saddles"] == 2 and polys[0].tolist().count([5, 5]) == 2     # the pinch, twice
    assert h["checkerboard"][0, 1] == 1 and h["checkerboard"][0, 2] == 18
    assert h["ring"][0, 1:3].tolist() == [1, 1]
    assert h["two_blobs"][0, 4:7].tolist() == [400, 20, 10]             # the larger blob, second in raster order
    assert h["two_blobs"][1, 4:7].tolist() == [60, 5, 3]                # equal areas: the lesser start edge
    assert h["spiral"][0, 0] >= 2000 and h["spiral"][0, 1] == 1         # one long cycle
    assert h["bits_0_and_7"][0, 4] != h["bits_0_and_7"][1, 4]
    assert h["empty_and_unmapped"][[1, 3, 4]].any() == 0 and h["empty_and_unmapped"][[0, 2], 0].all()


def test_overflow_is_refused_in_the_reference():
    c = [c for c in C.handmade() if c.name == "two_blobs"][0]
    full, _, _ = c.ref()
    hd, polys, _ = c.ref(max_edges=int(full[0, 0]) - 1)
    assert hd[0].tolist() == [int(full[0, 0]), 0, 0, 0, 0, 0, 0, 1] and polys[0] is None
    assert np.array_equal(hd[1], full[1]) and polys[1] is not None


# --- host helpers ------------------------------------------------------------------------------------------
def test_seg_label_format(fused):
    poly = np.array([[0, 0], [125, 0], [125, 97], [1, 97]], np.int32)
    assert fused.seg_label(3, poly, 125, 97) == "3 0.000000 0.000000 1.000000 0.000000 1.000000 1.000000 0.008000 1.000000"
    line = fused.seg_label(0, [[1, 2], [4, 2], [4, 7], [1, 7]], 3, 7)
    assert line == "0 0.333333 0.285714 1.333333 0.285714 1.333333 1.000000 0.333333 1.000000"
    box = fused.yolo_label(0, (1, 2, 4, 7), 3, 7).split()
    assert all(len(v.split(".")[1]) == 6 for v in line.split()[1:] + box[1:])      # yolo_label's number format
    with pytest.raises(ValueError):
        fused.seg_label(0, np.zeros((4, 3)), 8, 8)


def _seg_inputs():
    sq = np.array([[1, 1], [3, 1], [3, 3], [1, 3]], np.int32)
    polys = [[sq, None], [sq + 2, sq + 4]]
    info = np.zeros((2, 2, 8), np.int32)
    info[0, 0] = info[1, 0] = info[1, 1] = [8, 1, 0, 4, 8, 1, 1, 0]
    rows = np.array([[[1, 1, 3, 3, 8, 4], [-1, -1, -1, -1, 5, 0]],
                     [[3, 3, 5, 5, 4, 4], [5, 5, 7, 7, 16, 4]]], np.int32)
    return polys, info, rows


def test_scene_seg_labels(fused):
    polys, info, rows = _seg_inputs()
    got = fused.scene_seg_labels(polys, info, rows, 8, 8)
    assert got == [[fused.seg_label(0, polys[0][0], 8, 8)],
                   [fused.seg_label(0, polys[1][0], 8, 8), fused.seg_label(0, polys[1][1], 8, 8)]]
    # the inclusion rule and class ids of scene_labels
    ids = [5, 6, 7, 8]
    got = fused.scene_seg_labels(polys, info, rows, 8, 8, class_ids=ids, min_visible=0.5)
    assert got == [[fused.seg_label(5, polys[0][0], 8, 8)], [fused.seg_label(7, polys[1][0], 8, 8)]]
    box = fused.scene_labels(rows, 8, 8, ids, 0.5)
    assert [[ln.split()[0] for ln in sc] for sc in got] == [[ln.split()[0] for ln in sc] for sc in box]
    with pytest.raises(ValueError):
        fused.scene_seg_labels(polys, info, rows, 8, 8, class_ids=[1, 2, 3])
    with pytest.raises(ValueError):
        fused.scene_seg_labels(polys, info[:1], rows, 8, 8)


def test_scene_seg_labels_raises_on_overflow(fused):
    polys, info, rows = _seg_inputs()
    polys[1][1] = None
    info[1, 1] = [4321, 0, 0, 0, 0, 0, 0, 1]
    with pytest.raises(ValueError, match="4321"):
        fused.scene_seg_labels(polys, info, rows, 8, 8)
    # below min_visible it gets no line, so nothing is dropped: no error
    assert len(fused.scene_seg_labels(polys, info, rows, 8, 8, min_visible=0.5)[1]) == 1


def test_scene_contour_capacity(fused):
    src, bgs, plan, cfg = MR.noise_scenes(fused)
    p = plan.pipe
    cap = fused.scene_contour_capacity(plan)
    assert cap % 256 == 0 and 0 <= cap - 8 * (p.max_ov_w + p.max_ov_h) < 256
    assert fused.scene_contour_capacity(p) == cap


# --- the conditions the GPU tests lean on, on the reference alone ---------------------------------------
def test_scene_batches_meet_the_conditions_of_the_gpu_tests(fused):
    holes = multi = saddle = last_row = last_col = 0
    for name, (src, bgs, plan, cfg) in C.scene_batches(fused).items():
        assert plan.bg_w * plan.bg_h * 2 + plan.bg_w + plan.bg_h < C.SCENE_MAX_EDGES
        overlays = SR.scene_overlays(src, plan, cfg)
        for a, c in MR.LEVELS:
            hdrs, polys, stats, rows, vis = C.scene_reference(plan, overlays, a, c)
            assert hdrs[..., 0].max() <= C.SCENE_MAX_EDGES, name
            assert not hdrs[..., 7].any()
            holes += int((hdrs[..., 2] > 0).sum())
            multi += int((hdrs[..., 1] >= 2).sum())
            saddle += sum(1 for sc in stats for cyc in sc if any(cy["saddles"] for cy in cyc))
            for s in range(plan.n_scenes):
                for k in range(plan.per_scene):
                    if polys[s][k] is not None:
                        last_row += int(polys[s][k][:, 1].max() == plan.bg_h)
                        last_col += int(polys[s][k][:, 0].max() == plan.bg_w)
    assert holes and multi and saddle and last_row and last_col
