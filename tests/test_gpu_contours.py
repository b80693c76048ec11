"""GPU: polygons of scenes traced on the device (ipp_scene_contours,
ipp_scene_contours_pack, SceneRunner.scene_polygons, run_labelled(polygons=
True)) against the sequential CPU crack follower of tests/contour_refs.py.
Header and vertex buffers are pre-filled with a poison value and compared
whole, words that must stay untouched included."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import contour_refs as C
from tests import gpu_scene_support as S
from tests import scene_mask_refs as MR
from tests.gpu_scene_support import DEV, current_stream as _stream, same_polys as _same_polys, to_dev_copy as _t

pytestmark = pytest.mark.gpu

POISON = -0x5A5A5A5B            # 0xA5A5A5A5 as int32
HANDMADE = C.handmade()


@pytest.fixture(scope="module")
def fused():
    return S.require_fused()


@pytest.fixture(scope="module")
def lib(fused):
    from image_processor_pipeline_amd import _native as N
    return N.load()


def _trace(lib, case, max_edges, slack=3):
    """Both C entries on a handmade case: (hdr (n, 8), verts buffer, offsets, total).
    The vertex buffer has `slack` poisoned pairs after the polygons."""
    t = S.trace_contours(lib, case, max_edges, POISON, slack)
    return t.hdr, t.verts, t.offsets, t.total


def _expect_verts(hdrs, polys, slack=3):
    _, packed = C.pack(hdrs, polys)
    return np.concatenate([packed, np.full((slack, 2), POISON, np.int32)])


# --- 1: handmade maps through the C entries --------------------------------------------------------------
@pytest.mark.parametrize("case", HANDMADE, ids=lambda c: c.name)
def test_handmade_maps(lib, case):
    exp_h, exp_p, _ = case.ref()
    # a roomy capacity, and one that is exactly the largest descriptor's edge count (the last slot is used)
    for max_edges in (4096, max(4, int(exp_h[:, 0].max()))):
        h, verts, offsets, total = _trace(lib, case, max_edges)
        assert np.array_equal(h, exp_h), (max_edges, h.tolist(), exp_h.tolist())
        assert np.array_equal(verts, _expect_verts(exp_h, exp_p)), max_edges


# --- 2: overflow --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,victim", [("two_blobs", 0), ("bars", 2), ("bits_0_and_7", 1)])
def test_overflow_is_refused_not_truncated(fused, lib, name, victim):
    case = [c for c in HANDMADE if c.name == name][0]
    full, _, _ = case.ref()
    max_edges = int(full[victim, 0]) - 1
    assert all(int(full[i, 0]) <= max_edges for i in range(len(full)) if i != victim)
    exp_h, exp_p, _ = case.ref(max_edges)
    assert exp_h[victim].tolist() == [max_edges + 1, 0, 0, 0, 0, 0, 0, 1] and exp_p[victim] is None
    h, verts, offsets, total = _trace(lib, case, max_edges)
    assert np.array_equal(h, exp_h)                                        # flagged with its true count; others exact
    assert np.array_equal(verts, _expect_verts(exp_h, exp_p))              # pack wrote nothing for it
    n = len(case.rows)
    polys = [[p] for p in exp_p]
    rows = case.rows.reshape(n, 1, 6)
    with pytest.raises(ValueError, match=str(max_edges + 1)):
        fused.scene_seg_labels(polys, h.reshape(n, 1, 8), rows, case.bg_w, case.bg_h)


# --- 3: scene batches ------------------------------------------------------------------------------------------
class Scenes(S.SceneBatch):
    def __init__(self, fused, batch):
        super().__init__(fused, batch)
        self._refs = {}

    def ref(self, a, c):
        if (a, c) not in self._refs:
            self._refs[(a, c)] = C.scene_reference(self.plan, self.overlays, a, c, C.SCENE_MAX_EDGES)
        return self._refs[(a, c)]


@pytest.fixture(scope="module")
def batches(fused):
    return {name: Scenes(fused, b) for name, b in C.scene_batches(fused).items()}


@pytest.mark.parametrize("name", ["noise", "odd", "edge", "eight"])
@pytest.mark.parametrize("alpha_min,cover_min", MR.LEVELS)
def test_scene_batches(batches, name, alpha_min, cover_min):
    b = batches[name]
    exp_h, exp_p, _, exp_rows, _ = b.ref(alpha_min, cover_min)
    boxes = b.runner.scene_boxes(alpha_min, cover_min)
    polys, info, rows = b.runner.scene_polygons(alpha_min, cover_min, max_edges=C.SCENE_MAX_EDGES)
    assert rows.dtype == np.int32 and rows.tobytes() == boxes.tobytes()          # scene_boxes' own, byte for byte
    assert np.array_equal(rows, exp_rows)
    assert info.dtype == np.int32 and np.array_equal(info, exp_h)
    _same_polys(polys, exp_p)
    shape = (b.plan.bg_h, b.plan.bg_w)
    for s in range(b.plan.n_scenes):
        for k in range(b.plan.per_scene):
            if polys[s][k] is None:
                assert info[s, k, 3] == 0 and rows[s, k, 5] == 0
                continue
            fill = C.raster(polys[s][k], shape)
            assert int(fill.sum()) * 2 == info[s, k, 4]
            assert fill[info[s, k, 6], info[s, k, 5]] == 1                       # it covers the start pixel


# --- 4: run_labelled(polygons=True) -------------------------------------------------------------------------
def test_run_labelled_with_polygons(batches):
    b = batches["noise"]
    f, ids = b.fused, list(range(12))
    kw = dict(class_ids=ids, min_visible=0.5)
    o0, o1, o2, o3 = (torch.full_like(b.out, v) for v in (1, 2, 3, 4))
    plain = b.runner.run_labelled(b.dsrc, b.dbgs, o0, **kw)
    masked = b.runner.run_labelled(b.dsrc, b.dbgs, o1, masks=True, **kw)
    seg = b.runner.run_labelled(b.dsrc, b.dbgs, o2, polygons=True, max_edges=C.SCENE_MAX_EDGES, **kw)
    both = b.runner.run_labelled(b.dsrc, b.dbgs, o3, masks=True, polygons=True, max_edges=C.SCENE_MAX_EDGES, **kw)
    assert (len(plain), len(masked), len(seg), len(both)) == (2, 3, 3, 4)
    assert seg[0] is o2 and both[0] is o3
    for o in (o1, o2, o3):
        assert torch.equal(o, o0)                                                # the composites
    assert seg[1] == plain[1] and both[1] == plain[1] and masked[1] == plain[1]  # the box labels
    assert torch.equal(both[2], masked[2])                                       # the map
    exp_h, exp_p, _, exp_rows, vis = b.ref(1, 128)
    assert np.array_equal(both[2].cpu().numpy(), vis[:, :, :b.plan.bg_w])
    exp = f.scene_seg_labels(exp_p, exp_h, exp_rows, b.plan.bg_w, b.plan.bg_h, **kw)
    assert seg[2] == exp and both[3] == exp
    assert sum(len(x) for x in exp) > 0 and [len(x) for x in exp] == [len(x) for x in plain[1]]
    # the default capacity is too small for noise: the label is refused, never dropped
    small = f.scene_contour_capacity(b.plan)
    assert exp_h[..., 0].max() > small
    with pytest.raises(ValueError, match="max_edges"):
        b.runner.run_labelled(b.dsrc, b.dbgs, o3, polygons=True, **kw)


# --- 5: determinism ---------------------------------------------------------------------------------------------
def test_two_calls_are_byte_identical(lib, batches):
    b = batches["noise"]
    p1, i1, r1 = b.runner.scene_polygons(max_edges=C.SCENE_MAX_EDGES)
    p2, i2, r2 = b.runner.scene_polygons(max_edges=C.SCENE_MAX_EDGES)
    assert i1.tobytes() == i2.tobytes() and r1.tobytes() == r2.tobytes()
    _same_polys(p1, p2)
    case = [c for c in HANDMADE if c.name == "checkerboard"][0]
    h1, v1, _, _ = _trace(lib, case, 1024)
    h2, v2, _, _ = _trace(lib, case, 1024)
    assert h1.tobytes() == h2.tobytes() and v1.tobytes() == v2.tobytes()


# --- 6: guards -------------------------------------------------------------------------------------------------
def test_guards(fused, batches):
    from image_processor_pipeline_amd import _native as N
    b = batches["noise"]
    fresh = fused.SceneRunner(b.plan, DEV)
    with pytest.raises(N.NativeError):
        fresh.scene_polygons()                                                   # no H launch
    assert fresh._scratch is None and fresh._contour_scratch is None             # nothing allocated, nothing launched
    for kw in (dict(alpha_min=0), dict(cover_min=256), dict(cover_min=1.5), dict(alpha_min=None),
               dict(max_edges=3), dict(max_edges=(1 << 22) + 1), dict(max_edges=4.0), dict(max_edges=True)):
        before = b.runner._contour_scratch
        with pytest.raises(ValueError):
            b.runner.scene_polygons(**kw)
        with pytest.raises(ValueError):
            b.runner.run_labelled(b.dsrc, b.dbgs, torch.empty_like(b.out), polygons=True, **kw)
        assert b.runner._contour_scratch is before
    nine = Scenes(fused, MR.layered_scene(fused, 9))
    with pytest.raises(ValueError):
        nine.runner.scene_polygons()
    with pytest.raises(ValueError):
        nine.runner.run_labelled(nine.dsrc, nine.dbgs, nine.out, polygons=True)
    assert nine.runner._contour_scratch is None


def test_c_entry_points_refuse_bad_arguments(lib):
    from image_processor_pipeline_amd import _native as N
    case = [c for c in HANDMADE if c.name == "ring"][0]
    n, me = len(case.rows), 256
    nb = lib.ipp_scene_contours_scratch_bytes(n, me)
    scratch = torch.full((nb + 16,), 0xA5, dtype=torch.uint8, device=DEV)
    vis = torch.zeros((case.vis.size + 16,), dtype=torch.uint8, device=DEV)
    vis[:case.vis.size] = _t(case.vis).reshape(-1)
    rows, sl = _t(case.rows), _t(case.scene_layer)
    hdr = torch.full((n * 8,), POISON, dtype=torch.int32, device=DEV)
    assert scratch.data_ptr() % 16 == 0 and vis.data_ptr() % 16 == 0
    good = dict(map=vis.data_ptr(), pitch=case.pitch, bw=case.bg_w, bh=case.bg_h, rows=rows.data_ptr(),
                sl=sl.data_ptr(), n=n, S=case.n_scenes, K=1, me=me, scratch=scratch.data_ptr(), hdr=hdr.data_ptr())
    bad = [dict(map=None), dict(rows=None), dict(sl=None), dict(scratch=None), dict(hdr=None),
           dict(map=vis.data_ptr() + 8), dict(scratch=scratch.data_ptr() + 8),
           dict(K=0), dict(K=9), dict(pitch=16), dict(pitch=40), dict(pitch=case.bg_w - 16),
           dict(bw=1 << 15, bh=1 << 15, pitch=1 << 15),                          # bg_w·bg_h = 2^30
           dict(bw=0), dict(bh=0), dict(me=3), dict(me=(1 << 22) + 1), dict(n=-1),
           dict(n=1 << 20, me=1 << 22)]                                          # 2^20 · 2^14 blocks: the grid
    for kw in bad:
        a = dict(good)
        a.update(kw)
        rc = lib.ipp_scene_contours(a["map"], a["pitch"], a["bw"], a["bh"], a["rows"], a["sl"], a["n"], a["S"],
                                    a["K"], a["me"], a["scratch"], a["hdr"], _stream())
        assert rc == N.IPP_E_ARG, kw
    assert lib.ipp_scene_contours_scratch_bytes(n, 3) == N.IPP_E_ARG
    assert lib.ipp_scene_contours_scratch_bytes(n, (1 << 22) + 1) == N.IPP_E_ARG
    assert lib.ipp_scene_contours_scratch_bytes(-1, 256) == N.IPP_E_ARG
    torch.cuda.synchronize()
    assert bool((hdr == POISON).all()) and bool((scratch == 0xA5).all())         # nothing was launched
    # the pack entry
    offs = torch.zeros((n,), dtype=torch.int64, device=DEV)
    verts = torch.full((64,), POISON, dtype=torch.int32, device=DEV)
    pgood = dict(scratch=scratch.data_ptr(), hdr=hdr.data_ptr(), offs=offs.data_ptr(), n=n, me=me,
                 verts=verts.data_ptr())
    for kw in (dict(scratch=None), dict(hdr=None), dict(offs=None), dict(verts=None), dict(me=3),
               dict(me=(1 << 22) + 1), dict(n=-1), dict(scratch=scratch.data_ptr() + 8), dict(n=1 << 20, me=1 << 22)):
        a = dict(pgood)
        a.update(kw)
        assert lib.ipp_scene_contours_pack(a["scratch"], a["hdr"], a["offs"], a["n"], a["me"], a["verts"],
                                           _stream()) == N.IPP_E_ARG, kw
    torch.cuda.synchronize()
    assert bool((verts == POISON).all())
    # no descriptors: nothing to do, nothing written
    assert lib.ipp_scene_contours(good["map"], good["pitch"], good["bw"], good["bh"], good["rows"], good["sl"], 0,
                                  good["S"], 1, me, good["scratch"], good["hdr"], _stream()) == N.IPP_OK
    torch.cuda.synchronize()
    assert bool((hdr == POISON).all())
