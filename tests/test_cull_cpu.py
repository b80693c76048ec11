"""CPU: the cull's reference (tests/cull_refs.py) on its own — the batches and
thresholds of tests/test_gpu_cull.py have the properties those tests rely on —
and ``labels_fmt.min_visible_q``."""
import numpy as np
import pytest

from tests import cull_refs as C
from tests import scene_refs as SR


@pytest.fixture(scope="module")
def fused():
    from image_processor_pipeline_amd import fused as F
    return F


@pytest.fixture(scope="module")
def batches(fused):
    out = {}
    for name, make in C.BATCHES.items():
        src, bgs, plan, cfg = make(fused)
        out[name] = (bgs, plan, SR.scene_overlays(src, plan, cfg))
    return out


CASES = [(name, t) for name, ts in sorted(C.THRESHOLDS.items()) for t in ts]


@pytest.mark.parametrize("name,levels", CASES)
def test_each_case_culls_one_and_keeps_one(fused, batches, name, levels):
    bgs, plan, overlays = batches[name]
    a, c, mv, mp = levels
    kept, stats = C.cull(plan, overlays, a, c, fused.min_visible_q(mv), mp)
    assert kept.any() and not kept.all()
    # the top layer of a scene is hidden by nothing
    assert np.array_equal(stats[:, -1, 0], stats[:, -1, 1])
    # everything kept: the counts are the label rows' (nothing hides less than all later layers)
    all_kept, plain = C.cull(plan, overlays, a, c, 0, 0)
    rows = SR.scene_rows(plan, overlays, a, c)
    assert np.array_equal(plain, rows[..., 4:6]) and np.array_equal(all_kept, rows[..., 5] > 0)
    assert (stats[..., 1] >= plain[..., 1]).all() and np.array_equal(stats[..., 0], plain[..., 0])
    # the rows of the kept layers: a kept one has the decision's counts, a culled one is absent
    after = C.rows(plan, overlays, kept, a, c)
    assert np.array_equal(after[kept][:, 4:6], stats[kept])
    assert (after[~kept] == [-1, -1, -1, -1, 0, 0]).all()


def test_a_culled_layer_changes_a_count_below_it(fused, batches):
    """In the noise batch at (1, 128, 0.9) a layer 1 is culled and its layer 0 sees more than before."""
    _, plan, overlays = batches["noise"]
    kept, stats = C.cull(plan, overlays, 1, 128, fused.min_visible_q(0.9), 1)
    _, plain = C.cull(plan, overlays, 1, 128, 0, 0)
    assert any(not kept[s, 1] and stats[s, 0, 1] > plain[s, 0, 1] for s in range(plan.n_scenes))


def test_cover_scenes(fused, batches):
    bgs, plan, overlays = batches["cover"]
    q = fused.min_visible_q
    kept, stats = C.cull(plan, overlays, 1, 128, q(0.4), 1)
    assert stats[0, 0, 1] == 0 and stats[0, 0, 0] > 0 and not kept[0, 0]       # scene 0: fully covered
    frac = stats[1, 0, 1] / stats[1, 0, 0]
    assert 0.4 < frac < 0.6 and kept[1, 0]                                      # scene 1: partly, kept at 0.4
    k6 = C.cull(plan, overlays, 1, 128, q(0.6), 1)[0]
    assert not k6[1, 0]                                                         # and culled at 0.6
    full, c4, c6 = (C.composites(bgs, plan, overlays, k) for k in (np.ones_like(kept), kept, k6))
    assert np.array_equal(full, SR.scene_composites(bgs, plan, overlays))
    assert np.array_equal(c4, full)                                             # a fully covered overlay shows nowhere
    assert np.array_equal(c6[[0, 2]], full[[0, 2]]) and not np.array_equal(c6[1], full[1])    # the sliver is gone
    assert kept[2].all() and stats[2, 0, 1] == stats[2, 0, 0]                   # scene 2: the faint line covers nothing
    low, lstats = C.cull(plan, overlays, 1, 32, q(0.5), 1)
    assert lstats[2, 0, 1] < lstats[2, 0, 0] and low[2, 0] and not low[1, 0]    # at cover_min 32 it does


def test_chain_top_down_and_all_later_disagree_on_layer_0(batches):
    _, plan, overlays = batches["chain"]
    a, c, q, mp = C.CHAIN_Q
    kept, stats = C.cull(plan, overlays, a, c, q, mp)
    wrong, wstats = C.cull(plan, overlays, a, c, q, mp, top_down=False)
    assert kept.tolist() == [[True, False, True]] and wrong.tolist() == [[False, False, True]]
    assert stats[0, 0, 1] == stats[0, 0, 0] > 0              # layer 2 misses layer 0: all of it shows
    assert 2 * wstats[0, 0, 1] < wstats[0, 0, 0]             # under layer 1 most of it would not
    assert 2 * stats[0, 1, 1] < stats[0, 1, 0]               # layer 2 covers most of layer 1


def test_min_pixels_equal_to_visible_keeps_and_one_more_culls(batches):
    _, plan, overlays = batches["noise"]
    _, plain = C.cull(plan, overlays, 1, 128, 0, 0)
    v = int(plain[3, 0, 1])                                  # scene 3, layer 0
    assert v > 1
    assert C.cull(plan, overlays, 1, 128, 0, v)[0][3, 0]
    assert not C.cull(plan, overlays, 1, 128, 0, v + 1)[0][3, 0]
    assert C.keep_rule(10, 1, 0, 0) and C.keep_rule(10, 1, 0, 1) and not C.keep_rule(10, 0, 0, 0)


def test_min_q_equality_keeps(batches):
    """65536·vis = min_q·area keeps; one more in min_q culls (area = 2^k makes equality reachable)."""
    assert C.keep_rule(4096, 1024, 16384, 1) and not C.keep_rule(4096, 1024, 16385, 1)
    assert C.keep_rule(5, 5, 65536, 1) and not C.keep_rule(5, 4, 65536, 1)
    assert C.keep_rule(2**31 - 1, 2**31 - 1, 65536, 2**31 - 1)       # no 32-bit overflow in the reference


def test_min_visible_q(fused):
    q = fused.min_visible_q
    assert q(0) == 0 and q(0.0) == 0 and q(1) == 65536 and q(1.0) == 65536
    assert q(2.0 ** -16) == 1 and q(np.nextafter(2.0 ** -16, 1.0)) == 2 and q(np.nextafter(0.0, 1.0)) == 1
    assert q(0.5) == 32768 and q(np.float32(0.25)) == 16384 and q(np.int64(1)) == 65536
    assert q(0.4) == 26215                                   # ⌈26214.4⌉
    for bad in (-0.1, 1.0000001, float("nan"), float("inf"), True, None, "0.5", [0.5], 1 + 0j):
        with pytest.raises(ValueError):
            q(bad)


def test_a_kept_overlay_always_passes_scene_labels_test(fused):
    """Sweep: 65536·vis >= ⌈mv·65536⌉·area implies scene_labels' own vis >= mv·area in floats."""
    rng = np.random.default_rng(3)
    mvs = np.concatenate([rng.random(300), [0.0, 1.0, 0.4, 1 / 3, 2.0 ** -16, 0.1, 0.7, 0.9999999]])
    areas = np.concatenate([rng.integers(1, 1 << 22, 40), [1, 2, 3, 7, 10, 1 << 22]])
    n = 0
    for mv in mvs:
        q = fused.min_visible_q(float(mv))
        for area in areas.tolist():
            lo = -(-q * area // 65536)                       # the least vis the integer rule keeps
            for vis in {max(lo, 1), max(lo, 1) + 1, area} - {area + 1}:
                if vis <= area and C.keep_rule(area, vis, q, 1):
                    rows = np.array([[[0, 0, 1, 1, area, vis]]], np.int32)
                    assert len(fused.scene_labels(rows, 8, 8, 0, float(mv))[0]) == 1, (mv, area, vis)
                    n += 1
            if lo - 1 >= 1:
                assert not C.keep_rule(area, lo - 1, q, 1)
    assert n > 10000
