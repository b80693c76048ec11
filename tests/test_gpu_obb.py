"""GPU: the oriented boxes on the device (ipp_polygons_obb,
SceneRunner.scene_obbs, run_labelled(obb=True)) against the integer reference
of tests/obb_refs.py, exactly.  The record buffer is pre-filled with a poison
value and has slack records after it, the scratch with 0xA5; everything is
compared whole, words that must stay untouched included."""
import re
from pathlib import Path

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import contour_refs as C
from tests import gpu_scene_support as S
from tests import obb_refs as O
from tests import simplify_refs as R
from tests.gpu_scene_support import DEV, current_stream as _stream, to_dev_copy as _t

pytestmark = pytest.mark.gpu

POISON = -0x5A5A5A5B            # 0xA5A5A5A5 as int32
HANDMADE = C.handmade()
SLACK = 3
# from the header: the two path thresholds of the implementation — the lattice rows of one LDS window (a ring
# spanning more sweeps its vertices once per window) and the points of a monotone chain kept in LDS (later ones
# live in the scratch) — and the workgroup's thread count, the granularity of every sweep
_HEADER = (Path(__file__).resolve().parents[1] / "include" / "ipp.h").read_text()
LDS_ROWS = int(re.search(r"#define IPP_OBB_LDS_ROWS (\d+)", _HEADER).group(1))
LDS_HULL = int(re.search(r"#define IPP_OBB_LDS_HULL (\d+)", _HEADER).group(1))
CHUNK = int(re.search(r"#define IPP_OBB_THREADS (\d+)", _HEADER).group(1))
REC = int(re.search(r"#define IPP_OBB_REC (\d+)", _HEADER).group(1))


@pytest.fixture(scope="module")
def fused():
    return S.require_fused()


@pytest.fixture(scope="module")
def lib(fused):
    from image_processor_pipeline_amd import _native as N
    return N.load()


def _obb(lib, verts, offsets, hdr, total, bg=(16384, 16384)):
    """The entry on device verts / hdr: (records (n + SLACK, 8) with the slack, the scratch (bytes))."""
    from image_processor_pipeline_amd import _native as N
    n = len(offsets)
    nb = lib.ipp_polygons_obb_scratch_bytes(n, total)
    assert nb == (8 * total + 255) // 256 * 256                                   # the documented formula
    scratch = torch.full((max(nb, 16),), 0xA5, dtype=torch.uint8, device=DEV)
    rec = torch.full(((n + SLACK) * REC,), POISON, dtype=torch.int32, device=DEV)
    N.check(lib.ipp_polygons_obb(verts.data_ptr(), _t(offsets).data_ptr(), hdr.data_ptr(), n, total, bg[0], bg[1],
                                 scratch.data_ptr(), rec.data_ptr(), _stream()), "ipp_polygons_obb")
    return rec.cpu().numpy().reshape(n + SLACK, REC), scratch.cpu().numpy()


def _check(got, rings, live, offsets, total, what):
    """Records whole (slack included), and the scratch: only a ring of more than LDS_HULL vertices may touch its
    own slots (those of its right chain, and the same + total of its left one); every other byte stays 0xA5."""
    rec, scratch = got
    exp = np.concatenate([O.records(rings, live), np.full((SLACK, REC), POISON, np.int32)])
    assert rec.shape == exp.shape
    bad = np.nonzero((rec != exp).any(axis=1))[0]
    assert len(bad) == 0, (what, bad[:5].tolist(), rec[bad[:3]].tolist(), exp[bad[:3]].tolist())
    words = scratch[:len(scratch) // 4 * 4].view(np.uint32)
    free = np.ones(len(words), bool)
    for i, r in enumerate(rings):
        n = 0 if r is None else len(r)
        if n > LDS_HULL and live[i]:
            free[offsets[i]:offsets[i] + n] = False
            free[total + offsets[i]:total + offsets[i] + n] = False
    assert (words[free] == 0xA5A5A5A5).all(), what


def _direct(lib, rings, what, bg=(16384, 16384)):
    """Rings fed directly to the entry as synthetic verts / offsets / hdr, in one launch."""
    verts, offsets, hdr = R.synthetic(rings)
    got = _obb(lib, _t(verts.reshape(-1)), offsets, _t(hdr.reshape(-1)), len(verts), bg)
    _check(got, rings, [True] * len(rings), offsets, len(verts), what)
    return got


# --- 1: handmade maps, traced, packed, then boxed ---------------------------------------------------------------
@pytest.mark.parametrize("case", HANDMADE, ids=lambda c: c.name)
def test_handmade_maps(lib, case):
    exp_h, exp_p, _ = case.ref()
    t = S.trace_contours(lib, case, 4096, POISON, 0)
    assert np.array_equal(t.hdr, exp_h)
    got = _obb(lib, t.d_verts, t.offsets, t.d_hdr, t.total, (case.bg_w, case.bg_h))
    _check(got, exp_p, [p is not None for p in exp_p], t.offsets, t.total, case.name)


# --- 2: an overflowed descriptor --------------------------------------------------------------------------------
def test_overflowed_descriptor_gets_the_zero_record(lib):
    case = [c for c in HANDMADE if c.name == "two_blobs"][0]
    full, _, _ = case.ref()
    max_edges = int(full[0, 0]) - 1
    exp_h, exp_p, _ = case.ref(max_edges)
    assert exp_h[0, 7] == 1 and exp_p[0] is None and exp_p[1] is not None
    t = S.trace_contours(lib, case, max_edges, POISON, 0)
    assert np.array_equal(t.hdr, exp_h)
    got = _obb(lib, t.d_verts, t.offsets, t.d_hdr, t.total, (case.bg_w, case.bg_h))
    _check(got, exp_p, [p is not None for p in exp_p], t.offsets, t.total, "overflow")
    assert not got[0][0].any() and got[0][1].tolist() == O.record(exp_p[1])


# --- 3: synthetic rings fed directly ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_rings():
    return R.random_small_rings() + R.degenerate_rings() + R.extreme_rings() + list(O.wide_rings()[0])


def test_small_degenerate_extreme_and_wide_rings_in_one_launch(lib, small_rings):
    assert len(small_rings) >= 2000 + 7 + 8 + 24
    rec, _ = _direct(lib, small_rings, "small")
    assert {1, 2, 3, 4} <= set(rec[:-SLACK, 7].tolist())                          # m = 1 and m = 2 records too
    # the 128-bit case: a comparison cut to 64 bits would have chosen another edge on these
    rings, wrong = O.wide_rings()
    assert wrong
    base = len(small_rings) - len(rings)
    for i in wrong:
        assert rec[base + i].tolist() == O.record(rings[i]) != O.choose(rings[i], truncate=True)[1]


# --- 4: empty and flagged descriptors --------------------------------------------------------------------------
def test_empty_and_flagged_descriptors(lib):
    """n_vertices == 0, and a header with flags set whose n_vertices is not 0: the zero record, nothing else."""
    rings = [R.pinch_ring(), None, R.random_small_rings(3, seed=1)[2], R.pinch_ring(), R.pinch_ring()[:2]]
    verts, offsets, hdr = R.synthetic([r if r is not None else np.zeros((0, 2), np.int32) for r in rings])
    hdr[3, 7] = 1
    live = [True, False, True, False, True]
    got = _obb(lib, _t(verts.reshape(-1)), offsets, _t(hdr.reshape(-1)), len(verts))
    _check(got, rings, live, offsets, len(verts), "flagged")
    assert not got[0][1].any() and not got[0][3].any() and got[0][4, 7] == 2


# --- 5: rings just below, at and just above every path threshold --------------------------------------------
def test_row_window_thresholds(lib):
    """Two columns of points spanning LDS_ROWS - 1, LDS_ROWS and LDS_ROWS + 1 rows, two windows exactly and one
    row more, and the whole lattice 0..16384; the first ring does not start at row 0."""
    rings = [O.two_columns(LDS_ROWS - 1, 3, 11, 5), O.two_columns(LDS_ROWS, 0, 9), O.two_columns(LDS_ROWS + 1, 2, 4),
             O.two_columns(2 * LDS_ROWS, 7, 8, 1), O.two_columns(2 * LDS_ROWS + 1, 0, 16384),
             O.two_columns(16385, 0, 16384), np.array([(5, 0), (9, 16384), (0, 8000)], np.int32)]
    rec, _ = _direct(lib, rings, "rows")
    assert rec[5].tolist() == [0, 0, 16384, 0, 0, 1 << 28, 1 << 28, 4]


def test_chain_thresholds(lib):
    """Strictly convex rings whose right (then left) monotone chain holds LDS_HULL - 1, LDS_HULL and LDS_HULL + 1
    points — the last one spills into the scratch — and one whose last point drops a long chain from the scratch
    back into LDS.  They span more rows than one window as well."""
    rings = [O.chain_ring(n, mirror) for mirror in (False, True) for n in (LDS_HULL - 1, LDS_HULL, LDS_HULL + 1)]
    rings.append(O.chain_ring_popped(LDS_HULL + 88))
    assert [len(O.hull(r)) for r in rings[:6]] == [LDS_HULL - 1, LDS_HULL, LDS_HULL + 1] * 2
    assert len(O.hull(rings[6])) < LDS_HULL < len(rings[6])
    _direct(lib, rings, "chains")


def test_large_synthetic_rings(lib):
    """Jittered circles around the sweep's chunk of 256 vertices, and a long one."""
    sizes = [CHUNK - 1, CHUNK, CHUNK + 1, 5001]
    _direct(lib, [R.random_large_ring(n, seed=n) for n in sizes], "large")


# --- 6: scene batches ------------------------------------------------------------------------------------------
class Scenes(S.SceneBatch):
    def __init__(self, fused, batch):
        super().__init__(fused, batch)
        self.ref = C.scene_reference(self.plan, self.overlays, 1, 128, C.SCENE_MAX_EDGES)
        self.ref_obbs = np.stack([O.records(ps) for ps in self.ref[1]])


@pytest.fixture(scope="module")
def batches(fused):
    return {name: Scenes(fused, b) for name, b in C.scene_batches(fused).items()}


@pytest.mark.parametrize("name", ["noise", "odd", "edge", "eight"])
def test_scene_obbs(batches, name):
    b = batches[name]
    exp_h, exp_p, _, exp_rows, _ = b.ref
    obbs, info, rows = b.runner.scene_obbs(max_edges=C.SCENE_MAX_EDGES)
    assert obbs.dtype == np.int32 and obbs.shape == (b.plan.n_scenes, b.plan.per_scene, REC)
    assert np.array_equal(obbs, b.ref_obbs)
    assert (obbs[..., 7] >= 3).any()
    polys, p_info, p_rows = b.runner.scene_polygons(max_edges=C.SCENE_MAX_EDGES)
    assert info.tobytes() == p_info.tobytes() and rows.tobytes() == p_rows.tobytes()
    assert np.array_equal(info, exp_h) and np.array_equal(rows, exp_rows)


@pytest.mark.parametrize("name", ["noise", "odd", "edge", "eight"])
def test_run_labelled_obb(batches, name):
    b = batches[name]
    f, ids = b.fused, list(range(b.plan.n_scenes * b.plan.per_scene))
    kw = dict(class_ids=ids, min_visible=0.5, max_edges=C.SCENE_MAX_EDGES)
    o1, o2, o3, o4, o5 = (torch.full_like(b.out, v) for v in (1, 2, 3, 4, 5))
    plain = b.runner.run_labelled(b.dsrc, b.dbgs, o1, class_ids=ids, min_visible=0.5)
    obb = b.runner.run_labelled(b.dsrc, b.dbgs, o2, obb=True, **kw)
    seg = b.runner.run_labelled(b.dsrc, b.dbgs, o3, polygons=True, simplify=1.0, **kw)
    both = b.runner.run_labelled(b.dsrc, b.dbgs, o4, polygons=True, simplify=1.0, obb=True, **kw)
    full = b.runner.run_labelled(b.dsrc, b.dbgs, o5, polygons=True, obb=True, **kw)
    assert len(plain) == 2 and len(obb) == 3 and len(seg) == 3 and len(both) == 4 and len(full) == 4
    assert obb[0] is o2 and both[0] is o4
    assert all(torch.equal(o, o1) for o in (o2, o3, o4, o5))                      # `out` is the same in all
    assert obb[1] == plain[1] and both[1] == plain[1]                             # the box labels
    exp_h, _, _, exp_rows, _ = b.ref
    exp = f.scene_obb_labels(b.ref_obbs, exp_h, exp_rows, b.plan.bg_w, b.plan.bg_h, class_ids=ids, min_visible=0.5)
    assert obb[2] == exp and sum(len(x) for x in exp) > 0
    assert both[2] == seg[2]                                                      # the seg lines: obb changes nothing
    assert both[3] == obb[2] and full[3] == obb[2]                                # the OBB lines: simplify changes nothing
    assert [len(x) for x in obb[2]] == [len(x) for x in plain[1]]                 # one OBB line per box line
    assert all(len(ln.split()) == 9 for x in obb[2] for ln in x)


# --- 7: determinism ---------------------------------------------------------------------------------------------
def test_two_calls_are_byte_identical(lib, batches, small_rings):
    b = batches["noise"]
    a1, a2 = b.runner.scene_obbs(max_edges=C.SCENE_MAX_EDGES), b.runner.scene_obbs(max_edges=C.SCENE_MAX_EDGES)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a1, a2))
    rings = small_rings + [O.chain_ring(LDS_HULL + 1), O.two_columns(LDS_ROWS + 1)]
    verts, offsets, hdr = R.synthetic(rings)
    dv, dh = _t(verts.reshape(-1)), _t(hdr.reshape(-1))
    a = _obb(lib, dv, offsets, dh, len(verts))
    c = _obb(lib, dv, offsets, dh, len(verts))
    assert a[0].tobytes() == c[0].tobytes() and a[1].tobytes() == c[1].tobytes()


# --- 8: guards ---------------------------------------------------------------------------------------------------
def test_c_entry_point_refuses_bad_arguments(lib):
    from image_processor_pipeline_amd import _native as N
    rings = [R.pinch_ring(), R.pinch_ring()]
    verts, offsets, hdr = R.synthetic(rings)
    n, total = len(rings), len(verts)
    dv = torch.full((2 * total + 4,), POISON, dtype=torch.int32, device=DEV)
    dv[:2 * total] = _t(verts.reshape(-1))
    dh, doff = _t(hdr.reshape(-1)), _t(offsets)
    nb = lib.ipp_polygons_obb_scratch_bytes(n, total)
    scratch = torch.full((nb + 16,), 0xA5, dtype=torch.uint8, device=DEV)
    rec = torch.full(((n + 1) * REC,), POISON, dtype=torch.int32, device=DEV)
    good = dict(verts=dv.data_ptr(), offs=doff.data_ptr(), hdr=dh.data_ptr(), n=n, total=total, bw=100, bh=100,
                scratch=scratch.data_ptr(), rec=rec.data_ptr())

    def call(**kw):
        a = dict(good)
        a.update(kw)
        return lib.ipp_polygons_obb(a["verts"], a["offs"], a["hdr"], a["n"], a["total"], a["bw"], a["bh"],
                                    a["scratch"], a["rec"], _stream())

    bad = [dict(verts=None), dict(offs=None), dict(hdr=None), dict(scratch=None), dict(rec=None),
           dict(scratch=scratch.data_ptr() + 8), dict(verts=dv.data_ptr() + 2), dict(offs=doff.data_ptr() + 4),
           dict(hdr=dh.data_ptr() + 1), dict(rec=rec.data_ptr() + 2),
           dict(bw=0), dict(bh=0), dict(bw=-3), dict(bw=16385), dict(bh=16385),
           dict(n=-1), dict(total=-1), dict(total=(1 << 40) + 1),
           dict(n=1 << 24)]                                                       # 2^24 rings of 256 threads: the grid
    for kw in bad:
        assert call(**kw) == N.IPP_E_ARG, kw
    for args in ((-1, 8), (2, -1), (1 << 24, 8), (2, (1 << 40) + 1)):
        assert lib.ipp_polygons_obb_scratch_bytes(*args) == N.IPP_E_ARG
    assert lib.ipp_polygons_obb_scratch_bytes(2, 1 << 40) == 8 << 40              # the largest total is taken
    # no descriptors: nothing to do, nothing written
    assert call(n=0) == N.IPP_OK
    torch.cuda.synchronize()
    assert bool((rec == POISON).all()) and bool((scratch == 0xA5).all())          # nothing was launched
    # the largest legal sides are taken
    assert call(bw=16384, bh=16384) == N.IPP_OK
    torch.cuda.synchronize()
    exp = np.concatenate([O.records(rings), np.full((1, REC), POISON, np.int32)])
    assert np.array_equal(rec.cpu().numpy().reshape(-1, REC), exp) and bool((scratch == 0xA5).all())


# --- 9: Python refusals ------------------------------------------------------------------------------------------
def test_python_refusals(fused, batches):
    b = batches["noise"]
    b.runner.scene_obbs(max_edges=C.SCENE_MAX_EDGES)                              # the scratch is cached by now
    out = torch.full_like(b.out, 9)
    for bad in (0, 3, True, "64", 4.0, (1 << 22) + 1):
        before = b.runner._obb_scratch
        with pytest.raises(ValueError, match="max_edges"):
            b.runner.scene_obbs(max_edges=bad)
        with pytest.raises(ValueError, match="max_edges"):
            b.runner.run_labelled(b.dsrc, b.dbgs, out, obb=True, max_edges=bad)
        assert b.runner._obb_scratch is before and before is not None
    assert bool((out == 9).all())                                                 # refused before `run`
    # more than 8 layers: refused as for the masks, before anything runs
    from tests import scene_mask_refs as MR
    src, bgs, plan, _ = MR.layered_scene(fused, 9)
    nine = fused.SceneRunner(plan, DEV)
    dsrc, dbgs = _t(src), _t(bgs)
    out9 = torch.full((plan.n_scenes,) + bgs.shape[1:], 9, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="8"):
        nine.run_labelled(dsrc, dbgs, out9, obb=True)
    assert bool((out9 == 9).all()) and nine._obb_scratch is None
    nine.run(dsrc, dbgs, out9)
    with pytest.raises(ValueError, match="8"):
        nine.scene_obbs()
    assert nine._obb_scratch is None
    # a background above 16384 on a side: refused by name before `run` (a stand-in plan: nothing that large is built)
    from types import SimpleNamespace as NS
    real = b.runner.plan
    before = b.runner._obb_scratch
    try:
        b.runner.plan = NS(pipe=NS(bg_w=16385, bg_h=real.bg_h), n_scenes=real.n_scenes, per_scene=real.per_scene,
                           bg_w=16385, bg_h=real.bg_h, descs=real.descs, desc_item=real.desc_item)
        with pytest.raises(ValueError, match="16384"):
            b.runner.scene_obbs(max_edges=C.SCENE_MAX_EDGES)
        with pytest.raises(ValueError, match="16384"):
            b.runner.run_labelled(b.dsrc, b.dbgs, out, obb=True, max_edges=C.SCENE_MAX_EDGES)
    finally:
        b.runner.plan = real
    assert b.runner._obb_scratch is before and bool((out == 9).all())
