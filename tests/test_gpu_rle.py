"""GPU: the run-length encodings of scenes on the device (ipp_scene_rle,
ipp_scene_rle_pack, SceneRunner.scene_rles, run_labelled(rle=True)) against the
pixel-by-pixel reference of tests/rle_refs.py, exactly.  Header and count
buffers are pre-filled with a poison value and compared whole, words that must
stay untouched included; the scratch is pre-filled with 0xA5."""
import json

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import contour_refs as C
from tests import gpu_scene_support as S
from tests import rle_refs as R
from tests import scene_mask_refs as MR
from tests.gpu_scene_support import DEV, current_stream as _stream, to_dev_copy as _t

pytestmark = pytest.mark.gpu

POISON = -0x5A5A5A5B            # 0xA5A5A5A5 as int32
UPOISON = 0xA5A5A5A5
HANDMADE = R.all_handmade()
GAP = 2                         # poisoned slots after every descriptor's counts, those of a {0, 0} descriptor included
SLACK = 5                       # and after the last


@pytest.fixture(scope="module")
def fused():
    return S.require_fused()


@pytest.fixture(scope="module")
def lib(fused):
    from image_processor_pipeline_amd import _native as N
    return N.load()


def _encode(lib, case):
    """Both C entries on a handmade case: (hdr (n, 2), the whole count buffer as uint32, offsets)."""
    from image_processor_pipeline_amd import _native as N
    n = len(case.rows)
    nb = lib.ipp_scene_rle_scratch_bytes(n, case.bg_w)
    assert nb == (9 * n * ((case.bg_w + 3) // 4 * 4) + 255) // 256 * 256         # the documented formula
    scratch = torch.full((nb,), 0xA5, dtype=torch.uint8, device=DEV)
    vis, rows, sl = _t(case.vis), _t(case.rows), _t(case.scene_layer)
    hdr = torch.full((n * R.HDR,), POISON, dtype=torch.int32, device=DEV)
    args = (vis.data_ptr(), case.pitch, case.bg_w, case.bg_h, rows.data_ptr(), sl.data_ptr(), n, case.n_scenes,
            case.per_scene, scratch.data_ptr(), hdr.data_ptr())
    N.check(lib.ipp_scene_rle(*args, _stream()), "ipp_scene_rle")
    h = hdr.cpu().numpy().reshape(n, R.HDR)
    assert (h[:, 0] >= 0).all() and int(h[:, 0].sum()) <= 4 * case.vis.size       # before anything is sized by it
    nc = h[:, 0].astype(np.int64) + GAP
    offsets = np.concatenate([[0], np.cumsum(nc)[:-1]]).astype(np.int64)
    counts = torch.full((int(nc.sum()) + SLACK,), POISON, dtype=torch.int32, device=DEV)
    N.check(lib.ipp_scene_rle_pack(*args, _t(offsets).data_ptr(), counts.data_ptr(), _stream()),
            "ipp_scene_rle_pack")
    return h, counts.cpu().numpy().view(np.uint32), offsets


def _expect_counts(hdr, counts):
    out = []
    for c in counts:
        out += [c, np.full(GAP, UPOISON, np.uint32)]
    return np.concatenate(out + [np.full(SLACK, UPOISON, np.uint32)])


# --- 1: handmade maps through the C entries ------------------------------------------------------------------
@pytest.mark.parametrize("case", HANDMADE, ids=lambda c: c.name)
def test_handmade_maps(lib, case):
    exp_h, exp_c = R.case_reference(case)
    h, counts, offsets = _encode(lib, case)
    assert np.array_equal(h, exp_h), (h.tolist(), exp_h.tolist())
    exp = _expect_counts(exp_h, exp_c)
    assert counts.shape == exp.shape
    bad = np.nonzero(counts != exp)[0]
    assert len(bad) == 0, (bad[:8].tolist(), counts[bad[:8]].tolist(), exp[bad[:8]].tolist())


def test_two_calls_are_byte_identical(lib):
    case = [c for c in HANDMADE if c.name == "comb_300"][0]
    h1, c1, _ = _encode(lib, case)
    h2, c2, _ = _encode(lib, case)
    assert h1.tobytes() == h2.tobytes() and c1.tobytes() == c2.tobytes()


# --- 2: scene batches ----------------------------------------------------------------------------------------
class Scenes(S.SceneBatch):
    def __init__(self, fused, batch):
        super().__init__(fused, batch)
        self._refs = {}

    def ref(self, a, c):
        if (a, c) not in self._refs:
            self._refs[(a, c)] = R.scene_reference(self.plan, self.overlays, a, c)
        return self._refs[(a, c)]


@pytest.fixture(scope="module")
def batches(fused):
    return {name: Scenes(fused, b) for name, b in R.scene_batches(fused).items()}


CASES = [("noise",) + lv for lv in MR.LEVELS] + [(n, 1, 128) for n in ("odd", "edge", "cover", "eight", "single")]


@pytest.mark.parametrize("name,alpha_min,cover_min", CASES)
def test_scene_rles(batches, name, alpha_min, cover_min):
    b = batches[name]
    exp, exp_rows, _ = b.ref(alpha_min, cover_min)
    boxes = b.runner.scene_boxes(alpha_min, cover_min)
    rles, rows = b.runner.scene_rles(alpha_min, cover_min)
    assert rows.dtype == np.int32 and rows.tobytes() == boxes.tobytes()          # scene_boxes' own, byte for byte
    assert np.array_equal(rows, exp_rows)
    R.same_rles(rles, exp)
    # the device's own map, copied back and encoded on the host
    vis, m_rows = b.runner.scene_masks(alpha_min, cover_min, with_boxes=True)
    assert m_rows.tobytes() == rows.tobytes()
    R.same_rles(rles, R.scene_rles(vis.cpu().numpy(), m_rows, b.plan.bg_w))
    N = b.plan.bg_w * b.plan.bg_h
    live = 0
    for s in range(b.plan.n_scenes):
        for k in range(b.plan.per_scene):
            c = rles[s][k]
            if c is None:
                assert rows[s, k, 5] == 0 and rows[s, k, 0] == -1
                continue
            live += 1
            assert int(c.sum(dtype=np.int64)) == N and int(c[1::2].sum(dtype=np.int64)) == rows[s, k, 5]   # n_ones
    assert live > 0
    scratch = b.runner._rle_scratch
    assert b.runner.scene_rles(alpha_min, cover_min)[1].tobytes() == rows.tobytes()
    assert b.runner._rle_scratch is scratch and scratch is not None              # allocated once, reused


def test_the_edge_batch_reaches_the_last_pixel(batches):
    b = batches["edge"]
    rles, rows = b.runner.scene_rles()
    at_corner = [(s, k) for s in range(b.plan.n_scenes) for k in range(b.plan.per_scene)
                 if rows[s, k, 2] == b.plan.bg_w and rows[s, k, 3] == b.plan.bg_h]
    assert at_corner
    for s, k in at_corner:
        assert b.fused.rle_decode(rles[s][k], b.plan.bg_h, b.plan.bg_w)[:, -1].any()


# --- 3: run_labelled(rle=True) ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["noise", "cover"])
def test_run_labelled_rle(batches, name):
    b = batches[name]
    f, ids = b.fused, list(range(b.plan.n_scenes * b.plan.per_scene))
    kw = dict(class_ids=ids, min_visible=0.5)
    tr = dict(max_edges=C.SCENE_MAX_EDGES)
    o0, o1, o2, o3 = (torch.full_like(b.out, v) for v in (1, 2, 3, 4))
    plain = b.runner.run_labelled(b.dsrc, b.dbgs, o0, **kw)
    rle = b.runner.run_labelled(b.dsrc, b.dbgs, o1, rle=True, **kw)
    rest = b.runner.run_labelled(b.dsrc, b.dbgs, o2, masks=True, polygons=True, obb=True, **kw, **tr)
    every = b.runner.run_labelled(b.dsrc, b.dbgs, o3, masks=True, polygons=True, obb=True, rle=True, **kw, **tr)
    assert (len(plain), len(rle), len(rest), len(every)) == (2, 3, 5, 6)
    assert rle[0] is o1 and every[0] is o3
    for o in (o1, o2, o3):
        assert torch.equal(o, o0)                                                # the composites
    assert rle[1] == plain[1] and every[1] == plain[1]                           # the box labels
    assert torch.equal(every[2], rest[2]) and every[3] == rest[3] and every[4] == rest[4]   # map, seg and OBB lines
    exp_rles, exp_rows, _ = b.ref(1, 128)
    exp = f.scene_coco_annotations(exp_rles, exp_rows, b.plan.bg_w, b.plan.bg_h, **kw)
    assert rle[2] == exp and every[5] == exp
    assert sum(len(x) for x in exp) > 0 and [len(x) for x in exp] == [len(x) for x in plain[1]]
    assert json.loads(json.dumps(rle[2])) == exp
    for anns in exp:
        for a in anns:
            assert int(f.rle_decode(a["segmentation"]["counts"], b.plan.bg_h, b.plan.bg_w).sum()) == a["area"]


# --- 4: guards ---------------------------------------------------------------------------------------------------
def test_guards(fused, batches):
    from image_processor_pipeline_amd import _native as N
    b = batches["noise"]
    fresh = fused.SceneRunner(b.plan, DEV)
    with pytest.raises(N.NativeError):
        fresh.scene_rles()                                                       # no H launch
    assert fresh._scratch is None and fresh._rle_scratch is None                 # nothing allocated, nothing launched
    for kw in (dict(alpha_min=0), dict(cover_min=256), dict(cover_min=1.5), dict(alpha_min=None)):
        with pytest.raises(ValueError):
            b.runner.scene_rles(**kw)
        with pytest.raises(ValueError):
            b.runner.run_labelled(b.dsrc, b.dbgs, torch.empty_like(b.out), rle=True, **kw)
    src, bgs, plan, _ = MR.layered_scene(fused, 9)
    nine = fused.SceneRunner(plan, DEV)
    dsrc, dbgs = _t(src), _t(bgs)
    out9 = torch.full((plan.n_scenes,) + bgs.shape[1:], 9, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="8"):
        nine.run_labelled(dsrc, dbgs, out9, rle=True)
    assert bool((out9 == 9).all())                                               # refused before `run`
    nine.run(dsrc, dbgs, out9)
    with pytest.raises(ValueError, match="8"):
        nine.scene_rles()
    assert nine._rle_scratch is None


def test_c_entry_points_refuse_bad_arguments(lib):
    from image_processor_pipeline_amd import _native as N
    case = [c for c in HANDMADE if c.name == "ring"][0]
    n = len(case.rows)
    nb = lib.ipp_scene_rle_scratch_bytes(n, case.bg_w)
    scratch = torch.full((nb + 16,), 0xA5, dtype=torch.uint8, device=DEV)
    vis = torch.zeros((case.vis.size + 16,), dtype=torch.uint8, device=DEV)
    vis[:case.vis.size] = _t(case.vis).reshape(-1)
    rows, sl = _t(case.rows), _t(case.scene_layer)
    hdr = torch.full((n * R.HDR + 1,), POISON, dtype=torch.int32, device=DEV)
    offs = torch.zeros((n + 1,), dtype=torch.int64, device=DEV)
    counts = torch.full((64,), POISON, dtype=torch.int32, device=DEV)
    assert scratch.data_ptr() % 16 == 0 and vis.data_ptr() % 16 == 0
    good = dict(map=vis.data_ptr(), pitch=case.pitch, bw=case.bg_w, bh=case.bg_h, rows=rows.data_ptr(),
                sl=sl.data_ptr(), n=n, S=case.n_scenes, K=1, scratch=scratch.data_ptr(), hdr=hdr.data_ptr(),
                offs=offs.data_ptr(), counts=counts.data_ptr())

    def count(a):
        return lib.ipp_scene_rle(a["map"], a["pitch"], a["bw"], a["bh"], a["rows"], a["sl"], a["n"], a["S"], a["K"],
                                 a["scratch"], a["hdr"], _stream())

    def pack(a):
        return lib.ipp_scene_rle_pack(a["map"], a["pitch"], a["bw"], a["bh"], a["rows"], a["sl"], a["n"], a["S"],
                                      a["K"], a["scratch"], a["hdr"], a["offs"], a["counts"], _stream())

    bad = [dict(map=None), dict(rows=None), dict(sl=None), dict(scratch=None), dict(hdr=None),
           dict(map=vis.data_ptr() + 8), dict(scratch=scratch.data_ptr() + 8),
           dict(pitch=16), dict(pitch=40), dict(pitch=case.bg_w - 16),           # below bg_w; no multiple of 16
           dict(K=0), dict(K=9),
           dict(bw=1 << 15, bh=1 << 15, pitch=1 << 15),                          # bg_w·bg_h = 2^30
           dict(bw=0), dict(bh=0), dict(n=-1), dict(S=-1), dict(hdr=hdr.data_ptr() + 2),
           dict(n=1 << 24, bw=1 << 16, bh=1, pitch=1 << 16)]                     # 2^24 · 2^8 blocks: the grid
    for kw in bad:
        a = dict(good)
        a.update(kw)
        assert count(a) == N.IPP_E_ARG, kw
        assert pack(a) == N.IPP_E_ARG, kw
    for kw in (dict(offs=None), dict(counts=None), dict(offs=offs.data_ptr() + 4), dict(counts=counts.data_ptr() + 2)):
        a = dict(good)
        a.update(kw)
        assert pack(a) == N.IPP_E_ARG, kw
    for args in ((-1, 8), (2, 0), (2, -5)):
        assert lib.ipp_scene_rle_scratch_bytes(*args) == N.IPP_E_ARG
    assert lib.ipp_scene_rle_scratch_bytes(0, 8) == 0
    # no descriptors: nothing to do, nothing written
    a = dict(good)
    a.update(n=0)
    assert count(a) == N.IPP_OK and pack(a) == N.IPP_OK
    torch.cuda.synchronize()
    assert bool((hdr == POISON).all()) and bool((scratch == 0xA5).all()) and bool((counts == POISON).all())
    # and the good arguments are taken
    assert count(good) == N.IPP_OK
    exp_h, exp_c = R.case_reference(case)
    assert np.array_equal(hdr.cpu().numpy()[:n * R.HDR].reshape(n, R.HDR), exp_h) and int(hdr[-1]) == POISON
    assert pack(good) == N.IPP_OK
    got = counts.cpu().numpy().view(np.uint32)
    assert np.array_equal(got[:len(exp_c[0])], exp_c[0]) and (got[len(exp_c[0]):] == UPOISON).all()
