"""CPU: the scene planner (fused.plan_scenes) and the label formatting
(fused.scene_labels).  No GPU: the planner is host code of libipp.so."""
import numpy as np
import pytest

SRC_HW, BG_HW = (150, 170), (128, 160)
SLOT = 128 * 160 * 3


@pytest.fixture(scope="module")
def fused():
    from image_processor_pipeline_amd import fused as F
    return F


@pytest.fixture(scope="module")
def cfg(fused):
    return fused.PipeConfig(margins=(0.05, 9, 0.1, 3), scale_min=0.2, scale_max=0.5)


GEOMETRY = ("angle", "sym", "bg_index", "ratio", "x", "y", "rot_w", "rot_h", "cut_x", "cut_y", "cut_w", "cut_h",
            "ov_w", "ov_h")


def test_one_per_scene_is_plan_pipe(fused, cfg):
    for kw in (dict(seed=7), dict(seed=11, item_range=(3, 13), n_global=20)):
        a = fused.plan_pipe(SRC_HW, 10, BG_HW, 3, cfg, **kw)
        skw = dict(kw)
        if "n_global" in skw:
            skw["n_scenes_global"] = skw.pop("n_global")
        b = fused.plan_scenes(SRC_HW, 10, 1, BG_HW, 3, cfg, **skw)
        assert b.descs.tobytes() == a.descs.tobytes()
        assert b.axes.tobytes() == a.axes.tobytes() and b.items.tobytes() == a.items.tobytes()
        assert np.array_equal(b.desc_item, a.order)
        for f in ("coef_words", "tmp_bytes", "max_out_w", "max_rows", "max_ov_w", "max_ov_h", "algo_bytes_hpass",
                  "algo_bytes_vblend", "algo_bytes_hpass_bgcopy", "algo_bytes_vblend_bands", "copy_read_bytes"):
            assert getattr(b.pipe, f) == getattr(a, f), f
        assert b.copy_read_bytes == a.copy_read_bytes
        assert (b.n_scenes, b.per_scene) == (10, 1)
    # given parameters too
    c = fused.plan_scenes(SRC_HW, 10, 1, BG_HW, 3, cfg, params=a.params)
    d = fused.plan_pipe(SRC_HW, 10, BG_HW, 3, cfg, params=a.params)
    assert c.descs.tobytes() == d.descs.tobytes()


def test_draw_stream(fused, cfg):
    S, K, n_bg, seed = 5, 3, 2, 1234
    plan = fused.plan_scenes(SRC_HW, S, K, BG_HW, n_bg, cfg, seed=seed)
    angles, syms, order, drawn = fused.draw_params(15, 15, SRC_HW, BG_HW, n_bg, cfg, seed)
    it = plan.items
    assert it["angle"].tolist() == angles
    assert [plan.pipe.sym_pool[s] for s in it["sym"]] == syms
    assert it["ratio"].tolist() == [d[0] for d in drawn]
    assert it["x"].tolist() == [d[1] for d in drawn] and it["y"].tolist() == [d[2] for d in drawn]
    assert it["bg_index"].tolist() == [order[(i // 3) % 2] for i in range(15)]
    # the flat plan of the same 15 items draws the same stream; only the backgrounds differ
    flat = fused.plan_pipe(SRC_HW, 15, BG_HW, n_bg, cfg, seed=seed)
    for f in GEOMETRY:
        if f != "bg_index":
            assert np.array_equal(flat.items[f], it[f]), f


def test_sharding_by_scenes(fused, cfg):
    S, K = 5, 3
    whole = fused.plan_scenes(SRC_HW, S, K, BG_HW, 2, cfg, seed=9)
    parts = [fused.plan_scenes(SRC_HW, b - a, K, BG_HW, 2, cfg, seed=9, item_range=(a, b), n_scenes_global=S)
             for a, b in ((0, 2), (2, 5))]
    items = np.concatenate([p.items for p in parts])
    assert items.tobytes() == whole.items.tobytes()
    # per-item geometry of the descriptors: gather, H and V records but for the shard-local offsets
    a0 = 0
    for p in parts:
        n = len(p.descs)
        mine = np.empty_like(p.descs)
        mine[p.desc_item] = p.descs
        ref = np.empty_like(whole.descs)
        ref[whole.desc_item] = whole.descs
        ref = ref[a0:a0 + n]
        for f in ("in_w", "in_h", "a0", "a1", "a2", "a3", "a4", "a5", "out_w", "out_h", "off_x", "off_y", "flip"):
            assert np.array_equal(mine["g"][f], ref["g"][f]), f
        for ax in ("h", "v"):
            for f in ("in_len", "out_len", "lines", "line0", "ksize"):
                assert np.array_equal(mine[ax][f], ref[ax][f]), (ax, f)
        for f in ("ov_w", "ov_h", "x", "y"):
            assert np.array_equal(mine["p"][f], ref["p"][f]), f
        a0 += n
    for bad in ((0, 2), (1, 5), (-1, 2)):
        with pytest.raises(ValueError):
            fused.plan_scenes(SRC_HW, 3, K, BG_HW, 2, cfg, seed=9, item_range=bad)
    with pytest.raises(ValueError):
        fused.plan_scenes(SRC_HW, 3, K, BG_HW, 2, cfg, seed=9, item_range=(2, 5), n_scenes_global=4)


def test_descriptor_layout(fused, cfg):
    S, K = 7, 3
    plan = fused.plan_scenes(SRC_HW, S, K, BG_HW, 3, cfg, seed=5)
    d, it = plan.descs, plan.items
    assert len(d) == S * K and sorted(plan.desc_item.tolist()) == list(range(S * K))
    scene, layer = plan.desc_item // K, plan.desc_item % K
    assert np.array_equal(plan.scene_layer, np.stack([scene, layer], axis=1))
    assert layer.tolist() == [k for k in range(K) for _ in range(S)]                     # layer-major
    bg0 = it["bg_index"][plan.desc_item[:S]]
    assert len(set(bg0.tolist())) == 3 and (np.diff(bg0) >= 0).all()                     # layer 0 grouped by background
    assert np.array_equal(scene[:S], np.argsort(it["bg_index"][::K], kind="stable"))     # stable
    for k in range(1, K):
        assert np.array_equal(scene[k * S:(k + 1) * S], scene[:S])                       # every layer, same scene order
    assert np.array_equal(d["p"]["dst_off"], scene.astype(np.int64) * SLOT)              # one slot per scene
    assert np.array_equal(d["p"]["bg_off"][:S], bg0.astype(np.int64) * SLOT)
    assert np.array_equal(d["p"]["bg_off"][S:], d["p"]["dst_off"][S:])
    assert np.array_equal(d["p"]["bg_pitch"][S:], d["p"]["dst_pitch"][S:])
    # descriptor d is overlay item desc_item[d]: its source, its position
    assert np.array_equal(d["g"]["src_off"], plan.desc_item.astype(np.int64) * 150 * 170 * 3)
    assert np.array_equal(d["p"]["x"], it["x"][plan.desc_item]) and np.array_equal(d["p"]["y"], it["y"][plan.desc_item])
    assert plan.copy_read_bytes == 3 * SLOT                                              # 3 runs in one copy group


def test_refusals(fused, cfg):
    good = fused.plan_scenes(SRC_HW, 2, 2, BG_HW, 2, cfg, seed=1).params
    for K in (0, -1, 1.5, True):
        with pytest.raises(ValueError):
            fused.plan_scenes(SRC_HW, 2, K, BG_HW, 2, cfg, seed=1)
    mixed = list(good)
    mixed[1] = fused.ItemParams(good[1].angle, good[1].sym, 1 - good[1].bg_index, good[1].ratio, good[1].x, good[1].y)
    with pytest.raises(ValueError, match="scene 0"):
        fused.plan_scenes(SRC_HW, 2, 2, BG_HW, 2, cfg, params=mixed)
    with pytest.raises(ValueError):
        fused.plan_scenes(SRC_HW, 2, 2, BG_HW, 2, cfg, params=good[:3])
    with pytest.raises(ValueError):
        fused.plan_scenes(SRC_HW, 3, 2, BG_HW, 2, cfg, params=good)
    # the existing geometry refusals pass through
    far = list(good)
    far[2] = fused.ItemParams(good[2].angle, good[2].sym, good[2].bg_index, good[2].ratio, 10 ** 6, 0)
    with pytest.raises(ValueError):
        fused.plan_scenes(SRC_HW, 2, 2, BG_HW, 2, cfg, params=far)
    assert fused.plan_scenes(SRC_HW, 2, 2, BG_HW, 2, cfg, params=good).items.tobytes() == \
        fused.plan_scenes(SRC_HW, 2, 2, BG_HW, 2, cfg, seed=1).items.tobytes()


def test_scene_labels_formatting(fused):
    rows = np.array([
        [[10, 20, 50, 60, 1000, 1000], [30, 30, 40, 50, 400, 100], [-1, -1, -1, -1, 300, 0]],
        [[-1, -1, -1, -1, 50, 0], [-1, -1, -1, -1, 0, 0], [-1, -1, -1, -1, 7, 0]],
        [[0, 0, 160, 128, 9000, 4500], [5, 6, 7, 8, 4, 1], [1, 2, 3, 4, 2, 2]],
    ], np.int32)
    lab = fused.scene_labels(rows, 160, 128)
    assert lab[0] == [fused.yolo_label(0, (10, 20, 50, 60), 160, 128), fused.yolo_label(0, (30, 30, 40, 50), 160, 128)]
    assert lab[0][0] == "0 0.187500 0.312500 0.250000 0.312500"
    assert lab[1] == []                                        # nothing visible: an empty label file
    assert len(lab[2]) == 3
    half = fused.scene_labels(rows, 160, 128, min_visible=0.5)
    assert [len(x) for x in half] == [1, 0, 2]                 # 100/400 and 1/4 dropped, 4500/9000 kept
    ids = list(range(9))
    per = fused.scene_labels(rows, 160, 128, class_ids=ids, min_visible=0.25)
    assert [line.split()[0] for s in per for line in s] == ["0", "1", "6", "7", "8"]
    assert fused.scene_labels(rows, 160, 128, class_ids=4)[2][1].startswith("4 ")
    with pytest.raises(ValueError):
        fused.scene_labels(rows, 160, 128, class_ids=[0, 1])
    with pytest.raises(ValueError):
        fused.scene_labels(rows[0], 160, 128)
