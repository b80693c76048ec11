"""CPU: the keep-largest reference of tests/ccl_refs.py against the oracle, the
properties every designed case claims, the open-entry bound of a tile, and the
scratch layout's entry capacity on both sides of the all-open threshold.

tests/test_gpu_ccl_edges.py runs the same cases on the device; here each case
is shown, from the reference alone, to reach the branch it was built for."""
import time

import numpy as np
import pytest

from oracle import ops
from tests import ccl_refs as R


def _crop(full, bb):
    x0, y0, x1, y1 = bb
    return full[y0:y1, x0:x1]


def _masks():
    out = [(c.name, c.mask) for c in R.designed_cases()]
    out += [("stress%d" % i, m) for i, m in enumerate(R.ccl_stress_masks(np.random.default_rng(31))) if m.any()]
    out += [("fuzz%d" % i, m) for i, m in enumerate(R.fuzz_masks()[:48]) if m.any()]
    return out


def test_full_frame_reference_equals_oracle_crop():
    rng = np.random.default_rng(7)
    for name, m in _masks():
        im = R.image_from_mask(m, rng)
        full, bb = R.keep_largest_full(im)
        assert bb is not None, name
        assert np.array_equal(_crop(full, bb), ops.keep_largest_component(im)), name
        assert np.array_equal(full[..., :3], im[..., :3]), name
        kept = full[..., 3] != 0
        assert np.array_equal(full[..., 3][kept], im[..., 3][kept]) and (im[..., 3][kept] > 1).all(), name


def test_reference_without_foreground_leaves_the_frame():
    im = np.zeros((5, 7, 4), np.uint8)
    full, bb = R.keep_largest_full(im)
    assert bb is None and np.array_equal(full, im)
    im[2, 3, 3] = im[4, 6, 3] = 1                  # α = 1 is not foreground, but is not transparent either
    full, bb = R.keep_largest_full(im)
    assert bb == (3, 2, 7, 5) and np.array_equal(full, im)


@pytest.mark.parametrize("case", R.designed_cases(), ids=lambda c: c.name)
def test_designed_case_claims(case):
    R.check_claims(case)


def test_ring_tile_has_124_open_components():
    for shifted in (False, True):
        t = R.ring_tile(shifted)
        c = R.components(t)
        assert c.n == 124 and c.open[1:].all() and (c.area[1:] == 1).all()
        assert [int(t[0].sum()), int(t[1:, 63].sum()), int(t[63, :63].sum()), int(t[1:63, 0].sum())] == [32, 31, 31, 30]
        total, opened = R.tile_entries(t)
        assert total.tolist() == [124] and opened.tolist() == [124]
    assert not (R.ring_tile(False) & R.ring_tile(True)).any()
    # the even grid: 1024 components a tile, the 63 on its top row and left column open
    total, opened = R.tile_entries(R.even_grid_mask())
    assert opened.tolist() == [63] * 6 and total.max() == 1024 and total.min() >= 1021


def test_big_cases_claims_and_reference_cost():
    """The all-open images: the claimed properties (roots at the top of the
    23-bit field and past it, the tie, the kinds), the slot counts on either
    side of 2^23, and a reference that stays near a second."""
    c = R.big_closed_limit()
    assert R.slots(*c.mask.shape) == 1 << 23 and not R.all_open(*c.mask.shape)
    comps = R.check_claims(c)
    assert int(comps.root[comps.lab[c.winner]]) == (1 << 23) - 56
    assert c.mask.sum() < 1_000_000

    c = R.big_all_open()
    assert c.mask.shape == (4097, 4099) and R.slots(*c.mask.shape) == 8_400_900 and R.all_open(*c.mask.shape)
    t0 = time.perf_counter()
    comps = R.components(c.mask)
    im = np.zeros(c.mask.shape + (4,), np.uint8)
    im[..., 3] = np.where(c.mask, 200, 0)
    full, bb = R.keep_largest_full(im, comps)
    dt = time.perf_counter() - t0
    print("reference on 4097x4099: %.2f s, %d components, %d foreground pixels" % (dt, comps.n, int(c.mask.sum())))
    assert dt < 5.0                                 # per pixel in Python it would take minutes
    assert bb == (1990, 4092, 2041, 4095) and c.mask.sum() < 1_000_000
    R.check_claims(c)
    total, _ = R.tile_entries(c.mask)
    tx = (4099 + 63) // 64
    assert total[10 * tx + 20] > 1000               # the even-grid tile
    assert total[63 * tx + 31] >= 4                 # the kept bar's tile holds other components
    lb = comps.lab[1023, 990]                       # the four-tile bar is one component and loses
    assert comps.area[lb] == 140 and comps.open[lb] and lb == comps.lab[1024, 1059]
    assert total.sum() == R.expected_entries(c.mask) <= R.n_tiles(4097, 4099) * R.CMAX


def test_open_entry_bound_on_random_tiles():
    """At most 126 components of a 64×64 tile touch its ring of 252 pixels
    (two of them are never neighbours on it): the bound behind ent_cap =
    tiles·128.  2400 seeded tiles, densities 0.05..0.7, interior thinned so
    that ring pixels seldom join through it."""
    rng = np.random.default_rng(126)
    n = 2400
    dens = rng.uniform(0.05, 0.7, n)
    inner = rng.uniform(0.0, 1.0, n) * dens
    tiles = rng.random((n, R.TW, R.TW))
    ringm = np.zeros((R.TW, R.TW), bool)
    ringm[0], ringm[-1], ringm[:, 0], ringm[:, -1] = True, True, True, True
    m = np.where(ringm, tiles < dens[:, None, None], tiles < inner[:, None, None])
    # every other tile: its ring is the alternating pattern (every second pixel
    # of the ring's 252 in cyclic order, random phase) with a few bits flipped
    ry = np.concatenate([np.zeros(64, int), np.arange(1, 64), np.full(63, 63), np.arange(62, 0, -1)])
    rx = np.concatenate([np.arange(64), np.full(63, 63), np.arange(62, -1, -1), np.zeros(62, int)])
    assert ry.size == 252 and ringm[ry, rx].all() and len(set(zip(ry, rx))) == 252
    for i in range(0, n, 2):
        bits = (np.arange(252) + rng.integers(0, 2)) % 2 == 0
        bits ^= rng.random(252) < rng.uniform(0.0, 0.1)
        m[i][ry, rx] = bits
        m[i][1:-1, 1:-1] &= rng.random((62, 62)) < 0.3
    # the designed ring tiles and their seven other symmetries lead the sample
    sym = [f(np.rot90(R.ring_tile(s), k)) for s in (False, True) for k in range(4) for f in (np.asarray, np.fliplr)]
    m[:len(sym)] = sym
    # one image of 2400 tiles side by side: tile_entries labels each tile apart
    total, opened = R.tile_entries(np.concatenate(list(m), axis=1))
    print("open components per tile: designed %d, random max %d, mean %.1f"
          % (opened[0], opened[len(sym):].max(), opened[len(sym):].mean()))
    assert opened.max() <= 126 and (opened[:len(sym)] == 124).all()
    assert total.max() <= R.CMAX


def test_scratch_layout_entry_capacity():
    """ipp_ccl_scratch_layout: ent_cap = tiles·128 up to 2^23 run-start slots
    (4096×4096 is exactly 2^23), tiles·1024 past it; the entry arrays (24
    bytes an entry) lie inside [ent_off, tile_off)."""
    from image_processor_pipeline_amd import _native as N
    lib = N.load()
    one = np.zeros(1, N.CCL_WORK)
    for (h, w), per_tile in [((64, 64), 128), ((192, 192), 128), ((2160, 3840), 128), ((4096, 4096), 128),
                             ((4095, 4096), 128), ((4096, 4095), 128),
                             ((4097, 4096), 1024), ((4096, 4097), 1024), ((4097, 4099), 1024), ((70, 240000), 1024)]:
        size = lib.ipp_ccl_scratch_layout(w, h, N.np_ptr(one))
        k = one[0]
        assert R.all_open(h, w) == (per_tile == 1024), (h, w)
        assert int(k["ent_cap"]) == R.n_tiles(h, w) * per_tile, (h, w)
        assert int(k["tile_off"]) - int(k["ent_off"]) >= 24 * int(k["ent_cap"]), (h, w)
        assert int(k["a_off"]) - int(k["p_off"]) >= 4 * R.slots(h, w) <= int(k["ent_off"]) - int(k["a_off"])
        assert size >= int(k["tile_off"]) + 16 * R.n_tiles(h, w)
        assert int(k["ent_off"]) % 16 == 0 and (8 * int(k["ent_cap"])) % 16 == 0


def test_fuzz_seed_has_ties():
    """The fuzz images of the GPU test: at least 10 winners decided by the tie rule."""
    ties = sum(1 for m in R.fuzz_masks() if R.components(m).tied > 1)
    print("fuzz images decided by the tie rule:", ties)
    assert ties >= 10
