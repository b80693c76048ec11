"""``labels_fmt.feed_lut`` and the NumPy references of the device training
batches (tests/feed_refs.py) against what the project already has: the kept
set and the numbers of ``scene_labels``' lines, ``instance_ids``.  CPU only."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from image_processor_pipeline_amd import labels_fmt as L  # noqa: E402
from tests import feed_refs as FR  # noqa: E402

DTYPES = [torch.float16, torch.bfloat16, torch.float32]
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("mean,std,scale", [(MEAN, STD, 1.0 / 255.0), ((0, 0, 0), (1, 1, 1), 1.0 / 255.0),
                                            ((127.5, 100.0, 3.0), (58.0, 57.1, 0.37), 1.0)])
def test_feed_lut_is_the_float64_formula_rounded_once(dtype, mean, std, scale):
    lut = L.feed_lut(mean, std, dtype, scale)
    assert lut.dtype == dtype and tuple(lut.shape) == (3, 256) and lut.device.type == "cpu"
    for c in range(3):
        for v in range(256):
            exp = torch.tensor(((v * scale) - mean[c]) / std[c], dtype=torch.float64).to(dtype)
            assert lut[c, v].item() == exp.item(), (c, v)


def test_feed_lut_default_dtype_is_float16():
    assert L.feed_lut().dtype == torch.float16
    assert torch.equal(L.feed_lut()[1], torch.tensor(np.arange(256) * (1.0 / 255.0), dtype=torch.float64).to(torch.float16))


@pytest.mark.parametrize("kw", [dict(std=(1, 0, 1)), dict(std=(1, -2.0, 1)), dict(std=(1, float("nan"), 1)),
                                dict(mean=(0, float("inf"), 0)), dict(mean=(0, 0)), dict(std=(1, 1, 1, 1)),
                                dict(mean="abc"), dict(mean=3.0), dict(dtype=torch.float64), dict(dtype=torch.uint8),
                                dict(scale=float("nan")), dict(scale="1")])
def test_feed_lut_guards(kw):
    with pytest.raises(ValueError):
        L.feed_lut(**kw)


@pytest.mark.parametrize("min_visible", [0.0, 0.25, 0.5])
def test_targets_reference_keeps_what_scene_labels_keeps(min_visible):
    """For these multiples of 2^-16 the float test of ``_label_lines`` and the
    integer test of the rule coincide; the four numbers are those of the lines,
    which print six decimals (5e-7) — float32 adds at most 6e-8."""
    rng = np.random.default_rng(7)
    S, K, bw, bh = 40, 5, 1000, 777
    rows = FR.random_rows(rng, S, K, bw, bh)
    ids = rng.integers(0, 80, S * K)
    tg, n, slot = FR.targets(rows, ids, bw, bh, L.min_visible_q(min_visible))
    lines = list(L._label_lines(rows, ids, min_visible))
    assert 0 < n < S * K and n == len(lines)
    assert {(s, k) for s, k, _, _ in lines} == {(s, k) for s in range(S) for k in range(K) if slot[s, k] >= 0}
    assert np.array_equal(slot[slot >= 0], np.arange(n))               # compacted in scene, layer order
    assert np.all(tg[n:] == -1) and tg.dtype == np.float32
    labels = L.scene_labels(rows, bw, bh, ids, min_visible)
    flat = [(s, ln) for s in range(S) for ln in labels[s]]
    assert len(flat) == n
    for row, (s, ln) in zip(tg[:n], flat):
        f = ln.split()
        assert row[0] == s and row[1] == int(f[0])
        assert np.all(np.abs(row[2:].astype(np.float64) - np.array([float(v) for v in f[1:]])) <= 1e-6), (row, ln)


def test_targets_reference_ties_and_absent():
    rows = np.array([[[0, 0, 4, 4, 16, 4], [1, 1, 3, 3, 16, 3], [-1, -1, -1, -1, 9, 0], [2, 0, 5, 7, 8, 8]]], np.int32)
    tg, n, slot = FR.targets(rows, 3, 8, 8, 16384, present=np.array([[True, True, True, False]]))
    assert n == 1 and slot.tolist() == [[0, -1, -1, -1]]                # 4/16 ties and is kept, 3/16 is not
    assert tg[0].tolist() == [0.0, 3.0, 0.25, 0.25, 0.5, 0.5]


def test_index_map_reference():
    rng = np.random.default_rng(11)
    S, K, H, W = 5, 8, 9, 21
    pitch = L.scene_map_pitch(W)
    vis = rng.integers(0, 256, (S, H, pitch), np.uint8)
    slot = np.where(rng.random((S, K)) < 0.5, 0, -1).astype(np.int32)
    slot[0], slot[1] = -1, 0                                             # nothing kept, all kept
    ref = FR.index_map(vis, slot, W)
    assert np.all(ref[:, :, W:] == 0)
    for s in range(S):
        mask = sum(1 << k for k in range(K) if slot[s, k] >= 0)
        assert np.array_equal(ref[s, :, :W] > 0, (vis[s, :, :W] & mask) != 0)
        assert ref[s].max() <= bin(mask).count("1")
    assert np.array_equal(ref[1, :, :W], L.instance_ids(vis[1, :, :W]))  # every layer kept: 1 + the topmost layer
    # a dropped layer renumbers those above it and uncovers those below
    one = FR.index_map(np.array([[[0b101, 0b100, 0b001, 0b010, 0b110] + [0] * 11]], np.uint8),
                       np.array([[0, -1, 1]], np.int32), 5)
    assert one[0, 0, :5].tolist() == [2, 2, 1, 0, 2]
