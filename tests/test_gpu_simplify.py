"""GPU: the polygon simplification on the device (ipp_polygons_simplify,
ipp_polygons_simplify_pack, SceneRunner.scene_polygons(simplify=...),
run_labelled(polygons=True, simplify=...)) against the recursive reference of
tests/simplify_refs.py, exactly.  Count, mark and vertex buffers are pre-filled
with a poison value and compared whole, words that must stay untouched
included."""
import re
from pathlib import Path

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import contour_refs as C
from tests import gpu_scene_support as S
from tests import simplify_refs as R
from tests.gpu_scene_support import DEV, current_stream as _stream, same_polys as _same_polys, to_dev_copy as _t

pytestmark = pytest.mark.gpu

POISON = -0x5A5A5A5B            # 0xA5A5A5A5 as int32
HANDMADE = C.handmade()
EPS_QS = (1, 4, 6, 4096)
SLACK = 3
# from the header: the one path threshold of the implementation (a longer ring runs in the global scratch),
# and the workgroup's thread count — no path threshold, but the granularity of every sweep (thread t owns
# vertices t, t + CHUNK, ...; the scan of the keep flags goes chunk by chunk), so rings bracket it too
_HEADER = (Path(__file__).resolve().parents[1] / "include" / "ipp.h").read_text()
LDS_VERTS = int(re.search(r"#define IPP_SIMPLIFY_LDS_VERTS (\d+)", _HEADER).group(1))
CHUNK = int(re.search(r"#define IPP_SIMPLIFY_THREADS (\d+)", _HEADER).group(1))


@pytest.fixture(scope="module")
def fused():
    return S.require_fused()


@pytest.fixture(scope="module")
def lib(fused):
    from image_processor_pipeline_amd import _native as N
    return N.load()


def _trace(lib, case, max_edges):
    """The tracer and its pack on a handmade case: (hdr numpy (n, 8), offsets numpy, total, device hdr, device verts)."""
    t = S.trace_contours(lib, case, max_edges, POISON, 0)
    return t.hdr, t.offsets, t.total, t.d_hdr, t.d_verts


def _simplify(lib, verts, offsets, hdr, total, eps_q, bg=(16384, 16384)):
    """Both entries on device verts / hdr: (counts (n,), out (sum + SLACK, 2), marks (total,), the scratch's tail)."""
    from image_processor_pipeline_amd import _native as N
    n = len(offsets)
    nb = lib.ipp_polygons_simplify_scratch_bytes(n, total)
    assert nb == (4 * total + 255) // 256 * 256 + 16 * total                     # the documented formula
    scratch = torch.full((max(nb, 16),), 0xA5, dtype=torch.uint8, device=DEV)
    counts = torch.full((n + SLACK,), POISON, dtype=torch.int32, device=DEV)
    d_off = _t(offsets)
    N.check(lib.ipp_polygons_simplify(verts.data_ptr(), d_off.data_ptr(), hdr.data_ptr(), n, total, bg[0], bg[1],
                                      eps_q, scratch.data_ptr(), counts.data_ptr(), _stream()),
            "ipp_polygons_simplify")
    c = counts.cpu().numpy()
    assert (c[n:] == POISON).all()
    kept = c[:n].astype(np.int64)
    assert (kept >= 0).all()
    out_offsets = np.concatenate([[0], np.cumsum(kept)[:-1]]).astype(np.int64)
    out = torch.full((2 * (int(kept.sum()) + SLACK),), POISON, dtype=torch.int32, device=DEV)
    N.check(lib.ipp_polygons_simplify_pack(verts.data_ptr(), d_off.data_ptr(), hdr.data_ptr(), scratch.data_ptr(),
                                           counts.data_ptr(), _t(out_offsets).data_ptr(), n, out.data_ptr(),
                                           _stream()), "ipp_polygons_simplify_pack")
    s = scratch.cpu().numpy()
    marks = s[:4 * total].view(np.uint32).copy()
    pad = s[4 * total:(4 * total + 255) // 256 * 256]
    return c[:n], out.cpu().numpy().reshape(-1, 2), marks, pad


def _expect(rings, live, eps_q):
    """Reference (counts, out with SLACK poisoned pairs, marks) of the rings; live[i] False = a descriptor that
    must get count 0 and whose marks stay untouched."""
    counts, outs, marks = [], [], []
    for ring, ok in zip(rings, live):
        n = 0 if ring is None else len(ring)
        if not ok or n == 0:
            counts.append(0)
            marks.append(np.full(n, 0xA5A5A5A5, np.uint32))
            continue
        kept = R.simplify(ring, eps_q)
        m = np.zeros(n, np.uint32)
        m[kept] = np.arange(1, len(kept) + 1)
        counts.append(len(kept))
        outs.append(np.asarray(ring, np.int32)[kept])
        marks.append(m)
    outs.append(np.full((SLACK, 2), POISON, np.int32))
    return np.array(counts, np.int32), np.concatenate(outs), np.concatenate(marks) if marks else np.zeros(0, np.uint32)


def _check(got, exp, what):
    counts, out, marks, pad = got
    e_counts, e_out, e_marks = exp
    assert np.array_equal(counts, e_counts), (what, counts.tolist()[:40], e_counts.tolist()[:40])
    assert out.shape == e_out.shape and np.array_equal(out, e_out), what
    assert np.array_equal(marks, e_marks), what
    assert (pad == 0xA5).all(), what


def _direct(lib, rings, eps_q):
    """Rings fed directly to the entries as synthetic verts / offsets / hdr, in one launch."""
    verts, offsets, hdr = R.synthetic(rings)
    got = _simplify(lib, _t(verts.reshape(-1)), offsets, _t(hdr.reshape(-1)), len(verts), eps_q)
    _check(got, _expect(rings, [True] * len(rings), eps_q), eps_q)


# --- 1: handmade maps, traced, packed, then simplified ----------------------------------------------------------
@pytest.mark.parametrize("case", HANDMADE, ids=lambda c: c.name)
def test_handmade_maps(lib, case):
    exp_h, exp_p, _ = case.ref()
    h, offsets, total, hdr, verts = _trace(lib, case, 4096)
    assert np.array_equal(h, exp_h)
    live = [p is not None for p in exp_p]
    for eps_q in EPS_QS:
        got = _simplify(lib, verts, offsets, hdr, total, eps_q, (case.bg_w, case.bg_h))
        _check(got, _expect(exp_p, live, eps_q), (case.name, eps_q))
        if eps_q == 4096:
            assert all(c == 3 for c, ok in zip(got[0], live) if ok)


def test_overflowed_descriptor_gets_count_zero(lib):
    case = [c for c in HANDMADE if c.name == "two_blobs"][0]
    full, _, _ = case.ref()
    max_edges = int(full[0, 0]) - 1
    exp_h, exp_p, _ = case.ref(max_edges)
    assert exp_h[0, 7] == 1 and exp_p[0] is None and exp_p[1] is not None
    h, offsets, total, hdr, verts = _trace(lib, case, max_edges)
    assert np.array_equal(h, exp_h)
    got = _simplify(lib, verts, offsets, hdr, total, 4, (case.bg_w, case.bg_h))
    _check(got, _expect(exp_p, [p is not None for p in exp_p], 4), "overflow")
    assert got[0][0] == 0


# --- 2: synthetic rings fed directly ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_rings():
    return R.random_small_rings() + R.degenerate_rings() + R.extreme_rings()


@pytest.mark.parametrize("eps_q", (1, 4, 6, 16, 4096))
def test_random_small_rings_in_one_launch(lib, small_rings, eps_q):
    _direct(lib, small_rings, eps_q)


def test_empty_and_flagged_descriptors(lib):
    """n_vertices == 0, and a header with flags set whose n_vertices is not 0: count 0, nothing else written."""
    rings = [R.pinch_ring(), None, R.random_small_rings(3, seed=1)[2], R.pinch_ring(), R.pinch_ring()[:2]]
    verts, offsets, hdr = R.synthetic([r if r is not None else np.zeros((0, 2), np.int32) for r in rings])
    hdr[3, 7] = 1
    got = _simplify(lib, _t(verts.reshape(-1)), offsets, _t(hdr.reshape(-1)), len(verts), 4)
    _check(got, _expect(rings, [True, False, True, False, True], 4), "flagged")


# --- 3: many rounds --------------------------------------------------------------------------------------------
def test_spiral_many_rounds(lib):
    v = np.zeros((1, 64, 64), np.uint8)
    v[0] = C.spiral(64)
    case = C.Case("spiral64", v, 64, 1)
    exp_h, exp_p, _ = case.ref()
    assert R.simplify_levels(exp_p[0], 1)[1] >= 12                               # the deep case
    h, offsets, total, hdr, verts = _trace(lib, case, 8192)
    assert np.array_equal(h, exp_h)
    for eps_q in (1, 4, 6):
        _check(_simplify(lib, verts, offsets, hdr, total, eps_q, (64, 64)), _expect(exp_p, [True], eps_q), eps_q)


# --- 4: rings just below, at and just above every path threshold ---------------------------------------------
def test_comb_rings_at_the_thresholds(lib):
    """A comb's ring has 4 vertices per tooth: one scene per size, around the sweep's chunk of 256 vertices and
    around the LDS capacity (above it the ring runs in the global scratch)."""
    sizes = [CHUNK - 4, CHUNK, CHUNK + 4, LDS_VERTS - 4, LDS_VERTS, LDS_VERTS + 4]
    w = 2 * (max(sizes) // 4) - 1
    v = np.zeros((len(sizes), 2, (w + 15) // 16 * 16), np.uint8)
    for s, nv in enumerate(sizes):
        m = R.comb(nv // 4)
        v[s, :, :m.shape[1]] = m
    case = C.Case("combs", v, w, 1)
    exp_h, exp_p, _ = case.ref()
    assert [len(p) for p in exp_p] == sizes
    h, offsets, total, hdr, verts = _trace(lib, case, 8192)
    assert np.array_equal(h, exp_h)
    for eps_q in (1, 4, 4096):
        _check(_simplify(lib, verts, offsets, hdr, total, eps_q, (case.bg_w, case.bg_h)),
               _expect(exp_p, [True] * len(sizes), eps_q), eps_q)


def test_large_synthetic_rings_at_the_thresholds(lib):
    """Jittered circles (many levels, odd sizes) on both sides of the LDS capacity, and one far above it."""
    sizes = [CHUNK - 1, CHUNK, CHUNK + 1, LDS_VERTS - 1, LDS_VERTS, LDS_VERTS + 1, 2 * LDS_VERTS + 905]
    rings = [R.random_large_ring(n, seed=n) for n in sizes]
    for eps_q in (1, 6):
        _direct(lib, rings, eps_q)


# --- 5: scene batches ------------------------------------------------------------------------------------------
class Scenes(S.SceneBatch):
    def __init__(self, fused, batch):
        super().__init__(fused, batch)
        self.ref = C.scene_reference(self.plan, self.overlays, 1, 128, C.SCENE_MAX_EDGES)


@pytest.fixture(scope="module")
def batches(fused):
    return {name: Scenes(fused, b) for name, b in C.scene_batches(fused).items()}


@pytest.mark.parametrize("name", ["noise", "odd", "edge", "eight"])
def test_scene_polygons_simplified(batches, name):
    b = batches[name]
    exp_h, exp_p, _, exp_rows, _ = b.ref
    polys, info, rows = b.runner.scene_polygons(max_edges=C.SCENE_MAX_EDGES, simplify=1.0)
    assert np.array_equal(info, exp_h) and np.array_equal(rows, exp_rows)         # unchanged: the traced counts
    _same_polys(polys, [[R.apply(p, 4) for p in ps] for ps in exp_p])
    assert all(len(p) >= 3 for ps in polys for p in ps if p is not None)
    kept = sum(len(p) for ps in polys for p in ps if p is not None)
    assert kept <= int(exp_h[..., 3].sum()) and (name != "noise" or 2 * kept < int(exp_h[..., 3].sum()))
    # simplify=None is the plain call
    plain = b.runner.scene_polygons(max_edges=C.SCENE_MAX_EDGES)
    none = b.runner.scene_polygons(max_edges=C.SCENE_MAX_EDGES, simplify=None)
    _same_polys(plain[0], exp_p)
    _same_polys(none[0], plain[0])
    assert none[1].tobytes() == plain[1].tobytes() and none[2].tobytes() == plain[2].tobytes()


@pytest.mark.parametrize("name", ["noise", "odd", "edge", "eight"])
def test_run_labelled_simplified(batches, name):
    b = batches[name]
    f, ids = b.fused, list(range(b.plan.n_scenes * b.plan.per_scene))
    kw = dict(class_ids=ids, min_visible=0.5, polygons=True, max_edges=C.SCENE_MAX_EDGES)
    o1, o2, o3 = (torch.full_like(b.out, v) for v in (1, 2, 3))
    plain = b.runner.run_labelled(b.dsrc, b.dbgs, o1, **kw)
    none = b.runner.run_labelled(b.dsrc, b.dbgs, o2, simplify=None, **kw)
    seg = b.runner.run_labelled(b.dsrc, b.dbgs, o3, simplify=1.0, **kw)
    assert len(seg) == 3 and seg[0] is o3 and torch.equal(o3, o1) and torch.equal(o2, o1)
    assert none[1:] == plain[1:] and seg[1] == plain[1]                           # the box labels
    exp_h, exp_p, _, exp_rows, _ = b.ref
    simp = [[R.apply(p, 4) for p in ps] for ps in exp_p]
    exp = f.scene_seg_labels(simp, exp_h, exp_rows, b.plan.bg_w, b.plan.bg_h, class_ids=ids, min_visible=0.5)
    assert seg[2] == exp and sum(len(x) for x in exp) > 0
    assert [len(x) for x in seg[2]] == [len(x) for x in plain[1]]                 # one seg line per box line
    assert sum(len(ln) for x in seg[2] for ln in x) < sum(len(ln) for x in plain[2] for ln in x)


# --- 6: determinism ---------------------------------------------------------------------------------------------
def test_two_calls_are_byte_identical(lib, batches, small_rings):
    b = batches["noise"]
    p1, i1, r1 = b.runner.scene_polygons(max_edges=C.SCENE_MAX_EDGES, simplify=0.5)
    p2, i2, r2 = b.runner.scene_polygons(max_edges=C.SCENE_MAX_EDGES, simplify=0.5)
    assert i1.tobytes() == i2.tobytes() and r1.tobytes() == r2.tobytes()
    _same_polys(p1, p2)
    verts, offsets, hdr = R.synthetic(small_rings)
    dv, dh = _t(verts.reshape(-1)), _t(hdr.reshape(-1))
    a = _simplify(lib, dv, offsets, dh, len(verts), 4)
    c = _simplify(lib, dv, offsets, dh, len(verts), 4)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, c))


# --- 7: guards ---------------------------------------------------------------------------------------------------
def test_c_entry_points_refuse_bad_arguments(lib):
    from image_processor_pipeline_amd import _native as N
    rings = [R.pinch_ring(), R.pinch_ring()]
    verts, offsets, hdr = R.synthetic(rings)
    n, total = len(rings), len(verts)
    dv = torch.full((2 * total + 4,), POISON, dtype=torch.int32, device=DEV)
    dv[:2 * total] = _t(verts.reshape(-1))
    dh, doff = _t(hdr.reshape(-1)), _t(offsets)
    nb = lib.ipp_polygons_simplify_scratch_bytes(n, total)
    scratch = torch.full((nb + 16,), 0xA5, dtype=torch.uint8, device=DEV)
    counts = torch.full((n + 1,), POISON, dtype=torch.int32, device=DEV)
    good = dict(verts=dv.data_ptr(), offs=doff.data_ptr(), hdr=dh.data_ptr(), n=n, total=total, bw=100, bh=100,
                eps=4, scratch=scratch.data_ptr(), counts=counts.data_ptr())
    bad = [dict(verts=None), dict(offs=None), dict(hdr=None), dict(scratch=None), dict(counts=None),
           dict(scratch=scratch.data_ptr() + 8), dict(verts=dv.data_ptr() + 2), dict(offs=doff.data_ptr() + 4),
           dict(hdr=dh.data_ptr() + 1), dict(counts=counts.data_ptr() + 2),
           dict(eps=0), dict(eps=-4), dict(eps=4097), dict(bw=0), dict(bh=0), dict(bw=16385), dict(bh=16385),
           dict(n=-1), dict(total=-1), dict(total=(1 << 40) + 1),
           dict(n=1 << 24)]                                                       # 2^24 rings of 256 threads: the grid
    for kw in bad:
        a = dict(good)
        a.update(kw)
        rc = lib.ipp_polygons_simplify(a["verts"], a["offs"], a["hdr"], a["n"], a["total"], a["bw"], a["bh"],
                                       a["eps"], a["scratch"], a["counts"], _stream())
        assert rc == N.IPP_E_ARG, kw
    for args in ((-1, 8), (2, -1), (1 << 24, 8), (2, (1 << 40) + 1)):
        assert lib.ipp_polygons_simplify_scratch_bytes(*args) == N.IPP_E_ARG
    assert lib.ipp_polygons_simplify_scratch_bytes(2, 1 << 40) == 20 << 40        # the largest total is taken
    torch.cuda.synchronize()
    assert bool((counts == POISON).all()) and bool((scratch == 0xA5).all())       # nothing was launched
    # the largest legal sides and tolerance are taken
    assert lib.ipp_polygons_simplify(good["verts"], good["offs"], good["hdr"], n, total, 16384, 16384, 4096,
                                     good["scratch"], good["counts"], _stream()) == N.IPP_OK
    torch.cuda.synchronize()
    assert counts.cpu().numpy().tolist() == [3, 3, POISON]
    # the pack entry
    out_offs = _t(np.array([0, 3], np.int64))
    out = torch.full((16,), POISON, dtype=torch.int32, device=DEV)
    pgood = dict(verts=dv.data_ptr(), offs=doff.data_ptr(), hdr=dh.data_ptr(), scratch=scratch.data_ptr(),
                 counts=counts.data_ptr(), oo=out_offs.data_ptr(), n=n, out=out.data_ptr())
    for kw in (dict(verts=None), dict(offs=None), dict(hdr=None), dict(scratch=None), dict(counts=None),
               dict(oo=None), dict(out=None), dict(n=-1), dict(n=1 << 24), dict(scratch=scratch.data_ptr() + 8),
               dict(oo=out_offs.data_ptr() + 4), dict(out=out.data_ptr() + 2), dict(offs=doff.data_ptr() + 4)):
        a = dict(pgood)
        a.update(kw)
        assert lib.ipp_polygons_simplify_pack(a["verts"], a["offs"], a["hdr"], a["scratch"], a["counts"], a["oo"],
                                              a["n"], a["out"], _stream()) == N.IPP_E_ARG, kw
    torch.cuda.synchronize()
    assert bool((out == POISON).all())
    # no descriptors: nothing to do, nothing written
    assert lib.ipp_polygons_simplify_pack(pgood["verts"], pgood["offs"], pgood["hdr"], pgood["scratch"],
                                          pgood["counts"], pgood["oo"], 0, pgood["out"], _stream()) == N.IPP_OK
    torch.cuda.synchronize()
    assert bool((out == POISON).all())


def test_python_refusals(fused, batches):
    b = batches["noise"]
    out = torch.empty_like(b.out)
    with pytest.raises(ValueError, match="polygons"):
        b.runner.run_labelled(b.dsrc, b.dbgs, out, simplify=1.0)
    for bad in (0, 0.1, True, "1", 2048, float("nan")):
        before = b.runner._simplify_scratch
        with pytest.raises(ValueError):
            b.runner.scene_polygons(max_edges=C.SCENE_MAX_EDGES, simplify=bad)
        with pytest.raises(ValueError):
            b.runner.run_labelled(b.dsrc, b.dbgs, out, polygons=True, max_edges=C.SCENE_MAX_EDGES, simplify=bad)
        assert b.runner._simplify_scratch is before
