"""GPU: the scenes' cull (ipp_pipe_scene_cull / SceneRunner.run_culled,
run_labelled(cull=True)) against the CPU reference of tests/cull_refs.py, bit
for bit: the composites, the verdicts and the counts; the cleared scratch byte
by byte; the labels, maps and annotations that are read from it afterwards.
The batches and thresholds are those tests/test_cull_cpu.py checks on the
reference alone."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import cull_refs as C
from tests import gpu_scene_support as S
from tests import scene_mask_refs as MR
from tests import scene_refs as SR
from tests.gpu_scene_support import DEV, to_dev as _t

pytestmark = pytest.mark.gpu

POISON = 0x5A5A5A5A
ABSENT = [-1, -1, -1, -1, 0, 0]


@pytest.fixture(scope="module")
def fused():
    return S.require_fused()


class Batch(S.SceneBatch):
    """One scene batch after a plain ``run`` (``self.out``: the unculled composites)."""

    def ref(self, alpha_min, cover_min, min_visible, min_pixels):
        return C.cull(self.plan, self.overlays, alpha_min, cover_min, self.fused.min_visible_q(min_visible), min_pixels)

    def check(self, alpha_min, cover_min, min_visible, min_pixels):
        """run_culled into a fresh `out`: composites, kept and stats equal the reference; returns them."""
        out = torch.full_like(self.out, 99)
        got, kept, stats = self.runner.run_culled(self.dsrc, self.dbgs, out, alpha_min, cover_min, min_visible,
                                                  min_pixels)
        S_, K = self.plan.n_scenes, self.plan.per_scene
        assert got is out
        assert kept.dtype == np.bool_ and kept.shape == (S_, K)
        assert stats.dtype == np.int32 and stats.shape == (S_, K, 2)
        rkept, rstats = self.ref(alpha_min, cover_min, min_visible, min_pixels)
        assert np.array_equal(kept, rkept), (kept.tolist(), rkept.tolist())
        assert np.array_equal(stats, rstats), (stats.tolist(), rstats.tolist())
        host, exp = out.cpu().numpy(), C.composites(self.bgs, self.plan, self.overlays, rkept)
        assert np.array_equal(host, exp), int((host != exp).sum())
        return host, kept, stats

    def c_args(self, **kw):
        """Arguments of the C entry point for this batch, `kw` replacing some (``scene_layer``: the
        host array of another map); the scratch, the map and the poisoned records stay alive on the batch."""
        from image_processor_pipeline_amd import _native as N
        lib, r, p, plan = N.load(), self.runner, self.plan.pipe, self.plan
        n = len(plan.descs)
        a = dict(tmp=r.tmp.data_ptr(), coefs=r.coefs.data_ptr(), descs=r.descs.data_ptr(), n=n, S=plan.n_scenes,
                 K=plan.per_scene, mw=p.max_ov_w, mh=p.max_ov_h, a=1, c=128, q=0, mp=1, fmt=p.tap_format)
        a.update(kw)
        nb = lib.ipp_pipe_scene_scratch_bytes(n, plan.n_scenes, plan.per_scene, p.max_ov_w, p.max_ov_h)
        self.scratch = torch.empty(nb, dtype=torch.uint8, device=DEV)
        self.sl = _t(kw.get("scene_layer", plan.scene_layer))
        self.rec = torch.full((4 * n + 4,), POISON, dtype=torch.int32, device=DEV)
        a.setdefault("sl", self.sl.data_ptr())
        a.setdefault("scratch", self.scratch.data_ptr())
        a.setdefault("rec", self.rec.data_ptr())
        return lib, a

    def c_call(self, **kw):
        lib, a = self.c_args(**kw)
        return lib.ipp_pipe_scene_cull(a["tmp"], a["coefs"], a["descs"], a["sl"], a["n"], a["S"], a["K"], a["mw"],
                                       a["mh"], a["a"], a["c"], a["q"], a["mp"], a["fmt"], a["scratch"], a["rec"],
                                       S.current_stream())

    def records(self):
        """The records of the last c_call in scene, layer order: kept (S, K), stats (S, K, 2), raw (n, 4) by descriptor."""
        n = len(self.plan.descs)
        raw = self.rec.cpu().numpy()
        assert raw[4 * n:].tolist() == [POISON] * 4                 # nothing past the records
        raw = raw[:4 * n].reshape(n, 4)
        by_item = np.empty_like(raw)
        by_item[self.plan.desc_item] = raw
        by_item = by_item.reshape(self.plan.n_scenes, self.plan.per_scene, 4)
        return by_item[..., 0] != 0, by_item[..., 1:3], raw

    def culled_descs(self, kept):
        flat = np.asarray(kept).reshape(-1)
        return [d for d, item in enumerate(self.plan.desc_item.tolist()) if not flat[item]]


@pytest.fixture(scope="module")
def cover(fused):
    return Batch(fused, MR.cover_scenes(fused))


@pytest.fixture(scope="module")
def noise(fused):
    return Batch(fused, MR.noise_scenes(fused))


# --- (a) full, partial and faint cover -------------------------------------------------------
def test_full_partial_and_faint_cover(cover):
    b = cover
    full = b.out.cpu().numpy()
    assert np.array_equal(full, SR.scene_composites(b.bgs, b.plan, b.overlays))
    host4, kept4, stats4 = b.check(1, 128, 0.4, 1)
    assert kept4.tolist() == [[False, True], [True, True], [True, True]]
    assert stats4[0, 0].tolist()[1] == 0 and stats4[2, 0, 0] == stats4[2, 0, 1]        # covered; the faint line covers nothing
    host6, kept6, _ = b.check(1, 128, 0.6, 1)
    assert kept6.tolist() == [[False, True], [False, True], [True, True]]
    # a culled overlay's rectangle holds the composite without it: scene 1 is its background under layer 1 alone
    prm = b.plan.params
    alone = SR.ops.paste_rgba_onto_rgb(b.bgs[prm[3].bg_index], b.overlays[3], prm[3].x, prm[3].y)
    h, w = b.overlays[2].shape[:2]
    rect = np.s_[prm[2].y:prm[2].y + h, prm[2].x:prm[2].x + w]
    assert np.array_equal(host6[1][rect], alone[rect]) and not np.array_equal(host6[1][rect], full[1][rect])
    assert np.array_equal(host6[1], alone)
    _, low, _ = b.check(1, 32, 0.5, 1)
    assert low.tolist() == [[False, True], [False, True], [True, True]]


# --- (b) the chain: an overlay that only a culled one would hide is kept -------------------------
def test_chain_is_decided_top_down(fused):
    b = Batch(fused, C.chain_scene(fused))
    a, c, q, mp = C.CHAIN_Q
    host, kept, stats = b.check(a, c, q / 65536.0, mp)
    assert kept.tolist() == [[True, False, True]]
    assert stats[0, 0, 0] == stats[0, 0, 1] > 0
    wrong = C.cull(b.plan, b.overlays, a, c, q, mp, top_down=False)[0]
    assert wrong.tolist() == [[False, False, True]]
    assert not np.array_equal(host, C.composites(b.bgs, b.plan, b.overlays, wrong))


# --- (c) noise and the odd background ------------------------------------------------------------
@pytest.mark.parametrize("levels", C.THRESHOLDS["noise"])
def test_noise_scenes(noise, levels):
    _, kept, _ = noise.check(*levels)
    assert kept.any() and not kept.all()


def test_odd_background(fused):
    b = Batch(fused, MR.odd_scenes(fused))
    assert (b.plan.bg_h, b.plan.bg_w) == (97, 125)
    for levels in C.THRESHOLDS["odd"]:
        _, kept, _ = b.check(*levels)
        assert kept.any() and not kept.all()


# --- (d) eight and nine layers ----------------------------------------------------------------------
@pytest.mark.parametrize("K", [8, 9])
def test_many_layers(fused, K):
    b = Batch(fused, MR.layered_scene(fused, K))
    for levels in C.THRESHOLDS["eight" if K == 8 else "nine"]:
        _, kept, _ = b.check(*levels)
        assert kept.any() and not kept.all() and kept[0, K - 1]


# --- (e) T exactness --------------------------------------------------------------------------------
def test_the_cleared_scratch_byte_by_byte(fused, noise):
    from image_processor_pipeline_amd import _native as N
    b = noise
    b.runner.run(b.dsrc, b.dbgs, torch.empty_like(b.out))
    before = b.runner.tmp.cpu().numpy().copy()
    a, c, mv, mp = C.THRESHOLDS["noise"][0]
    q = fused.min_visible_q(mv)
    assert b.c_call(a=a, c=c, q=q, mp=mp) == N.IPP_OK
    after = b.runner.tmp.cpu().numpy()
    kept, stats, raw = b.records()
    rkept, rstats = C.cull(b.plan, b.overlays, a, c, q, mp)
    assert np.array_equal(kept, rkept) and np.array_equal(stats, rstats)
    assert set(raw[:, 0].tolist()) == {0, 1} and not raw[:, 3].any()           # every word written
    cleared = C.t_mask(b.plan, b.culled_descs(rkept))
    assert cleared.any() and (after[cleared] == 0x80).all()
    assert np.array_equal(after[~cleared], before[~cleared])
    assert (before[cleared] != 0x80).any()
    # the extent lies inside each descriptor's own T (ipp_pipe_layout.h t_groups: rows rounded up to 16 first)
    ends = sorted(int(d["h"]["dst_off"]) for d in b.plan.descs) + [int(b.plan.pipe.tmp_bytes)]
    for d in b.plan.descs:
        off, rb, pitch, G = C.t_extent(d)
        assert rb == pitch and off + G * pitch <= ends[ends.index(off) + 1]


def test_thresholds_that_keep_everything_change_nothing(noise):
    from image_processor_pipeline_amd import _native as N
    b = noise
    b.runner.run(b.dsrc, b.dbgs, torch.empty_like(b.out))
    before = b.runner.tmp.cpu().numpy().copy()
    assert b.c_call(q=0, mp=0) == N.IPP_OK
    kept, stats, _ = b.records()
    assert kept.all() and np.array_equal(stats, SR.scene_rows(b.plan, b.overlays, 1, 128)[..., 4:6])
    assert np.array_equal(b.runner.tmp.cpu().numpy(), before)
    out = torch.full_like(b.out, 99)
    _, kept, _ = b.runner.run_culled(b.dsrc, b.dbgs, out, min_visible=0.0, min_pixels=0)
    assert kept.all() and torch.equal(out, b.out)


# --- (f) boundary values, from the reference's own counts ----------------------------------------------
def test_equality_keeps(noise):
    b = noise
    _, plain = C.cull(b.plan, b.overlays, 1, 128, 0, 0)
    area, vis = (int(v) for v in plain[3, 0])
    assert 1 < vis < area
    _, kept, _ = b.check(1, 128, 0.0, vis)
    assert kept[3, 0]
    _, kept, _ = b.check(1, 128, 0.0, vis + 1)
    assert not kept[3, 0]
    # min_q through the C entry: the largest q with 65536·vis >= q·area keeps, q + 1 culls
    from image_processor_pipeline_amd import _native as N
    q = 65536 * vis // area
    for qq, want in ((q, True), (q + 1, False)):
        b.runner.run(b.dsrc, b.dbgs, torch.empty_like(b.out))
        assert b.c_call(q=qq, mp=0) == N.IPP_OK
        kept, stats, _ = b.records()
        rkept, rstats = C.cull(b.plan, b.overlays, 1, 128, qq, 0)
        assert np.array_equal(kept, rkept) and np.array_equal(stats, rstats)
        assert kept[3, 1:].all() and stats[3, 0].tolist() == [area, vis] and bool(kept[3, 0]) == want
    b.runner.run(b.dsrc, b.dbgs, torch.empty_like(b.out))
    assert b.c_call(q=65536, mp=0) == N.IPP_OK                                  # min_q = 65536: only the uncovered stay
    kept, stats, _ = b.records()
    assert np.array_equal(kept, (stats[..., 0] == stats[..., 1]) & (stats[..., 1] > 0)) and kept[:, 2].all()


# --- (g) run_labelled(cull=True) ---------------------------------------------------------------------------
def test_run_labelled_with_cull(cover):
    b, ids = cover, list(range(6))
    out = torch.full_like(b.out, 99)
    res = b.runner.run_labelled(b.dsrc, b.dbgs, out, class_ids=ids, min_visible=0.6, masks=True, polygons=True,
                                rle=True, cull=True)
    assert len(res) == 6
    got, labels, vis, seg, coco, kept = res
    rkept, rstats = b.ref(1, 128, 0.6, 1)
    assert got is out and np.array_equal(kept, rkept) and not rkept.all()
    assert np.array_equal(out.cpu().numpy(), C.composites(b.bgs, b.plan, b.overlays, rkept))
    rows = C.rows(b.plan, b.overlays, rkept, 1, 128)
    assert labels == b.fused.scene_labels(rows, b.plan.bg_w, b.plan.bg_h, ids, 0.6)
    # every kept overlay has a line, no culled one has: a line per kept overlay, with its class id
    assert [[int(ln.split()[0]) for ln in sc] for sc in labels] == \
        [[s * 2 + k for k in range(2) if rkept[s, k]] for s in range(3)]
    exp_map = MR.scene_map(b.plan, C.absent(b.overlays, rkept), 1, 128)[:, :, :b.plan.bg_w]
    host = vis.cpu().numpy()
    assert np.array_equal(host, exp_map)
    for s in range(3):
        for k in range(2):
            assert bool(((host[s] >> k) & 1).any()) == bool(rkept[s, k])        # no map bit of a culled overlay
    assert [[int(ln.split()[0]) for ln in sc] for sc in seg] == [[int(ln.split()[0]) for ln in sc] for sc in labels]
    assert [[an["category_id"] for an in sc] for sc in coco] == [[int(ln.split()[0]) for ln in sc] for sc in labels]
    assert [[an["area"] for an in sc] for sc in coco] == [[int(rstats[s, k, 1]) for k in range(2) if rkept[s, k]]
                                                          for s in range(3)]
    # the readers of the scratch afterwards: the culled overlays are absent, the kept have the decision's counts
    boxes = b.runner.scene_boxes(1, 128)
    assert np.array_equal(boxes, rows)
    assert (boxes[~rkept] == ABSENT).all() and np.array_equal(boxes[rkept][:, 4:6], rstats[rkept])
    polys, _, prow = b.runner.scene_polygons(1, 128)
    rles, _ = b.runner.scene_rles(1, 128)
    assert np.array_equal(prow, rows)
    for s in range(3):
        for k in range(2):
            assert (polys[s][k] is not None) == bool(rkept[s, k]) == (rles[s][k] is not None)
    # without cull the tuple is as before
    assert len(b.runner.run_labelled(b.dsrc, b.dbgs, out, min_visible=0.6, masks=True, polygons=True, rle=True)) == 5
    assert torch.equal(out, b.out)


# --- (h) a plain run afterwards rewrites T ----------------------------------------------------------------------
def test_a_plain_run_afterwards_is_unculled(noise):
    b = noise
    _, kept, _ = b.check(*C.THRESHOLDS["noise"][0])
    assert not kept.all()
    assert (b.runner.scene_boxes(1, 128)[~kept] == ABSENT).all()
    out = torch.full_like(b.out, 99)
    b.runner.run(b.dsrc, b.dbgs, out)
    assert torch.equal(out, b.out)
    assert np.array_equal(b.runner.scene_boxes(1, 128), SR.scene_rows(b.plan, b.overlays, 1, 128))


# --- (i) edge cases ------------------------------------------------------------------------------------------------
def test_a_descriptor_without_a_plane_is_kept_and_not_cleared(fused, noise):
    from image_processor_pipeline_amd import _native as N
    b, p = noise, noise.plan.pipe
    mw = p.max_ov_w - 1
    widest = [i for i, ov in enumerate(b.overlays) if ov.shape[1] > mw]
    assert widest and all(i % 3 > 0 for i in widest)                           # a later layer of its scene
    b.runner.run(b.dsrc, b.dbgs, torch.empty_like(b.out))
    before = b.runner.tmp.cpu().numpy().copy()
    q = fused.min_visible_q(0.9)
    assert b.c_call(mw=mw, q=q) == N.IPP_OK
    kept, stats, _ = b.records()
    rkept, rstats = C.cull(b.plan, b.overlays, 1, 128, q, 1, max_ov=(mw, p.max_ov_h))
    assert np.array_equal(kept, rkept) and np.array_equal(stats, rstats)
    assert not np.array_equal(rstats, C.cull(b.plan, b.overlays, 1, 128, q, 1)[1])     # it hides nothing now
    for i in widest:
        assert kept[i // 3, i % 3] and not stats[i // 3, i % 3].any()
    after = b.runner.tmp.cpu().numpy()
    cleared = C.t_mask(b.plan, b.culled_descs(rkept))
    assert (after[cleared] == 0x80).all() and np.array_equal(after[~cleared], before[~cleared])


def test_an_unmapped_descriptor_is_decided_alone(fused, noise):
    from image_processor_pipeline_amd import _native as N
    b = noise
    alone = (0, 5)                                                             # scene 0 layer 0, scene 1 layer 2
    sl = b.plan.scene_layer.copy()
    item_desc = {item: d for d, item in enumerate(b.plan.desc_item.tolist())}
    sl[item_desc[0]] = (-1, 0)
    sl[item_desc[5]] = (1, 3)
    b.runner.run(b.dsrc, b.dbgs, torch.empty_like(b.out))
    q = fused.min_visible_q(0.9)
    assert b.c_call(scene_layer=sl, q=q) == N.IPP_OK
    kept, stats, _ = b.records()
    rkept, rstats = C.cull(b.plan, b.overlays, 1, 128, q, 1, alone=alone)
    assert np.array_equal(kept, rkept) and np.array_equal(stats, rstats)
    mapped = C.cull(b.plan, b.overlays, 1, 128, q, 1)
    assert kept[0, 0] and stats[0, 0, 0] == stats[0, 0, 1] > mapped[1][0, 0, 1]         # alone: nothing hides it
    assert not np.array_equal(rstats[1], mapped[1][1])                                  # and it hides nothing


def test_no_descriptors(noise):
    from image_processor_pipeline_amd import _native as N
    b = noise
    b.runner.run(b.dsrc, b.dbgs, torch.empty_like(b.out))
    before = b.runner.tmp.clone()
    assert b.c_call(n=0) == N.IPP_OK
    torch.cuda.synchronize()
    assert bool((b.rec == POISON).all()) and torch.equal(b.runner.tmp, before)


def test_c_entry_point_refuses_bad_arguments(noise):
    from image_processor_pipeline_amd import _native as N
    b = noise
    b.runner.run(b.dsrc, b.dbgs, torch.empty_like(b.out))
    before = b.runner.tmp.clone()
    tmp = b.runner.tmp.data_ptr()
    bad = [dict(tmp=None), dict(coefs=None), dict(descs=None), dict(sl=None), dict(scratch=None), dict(rec=None),
           dict(a=0), dict(a=256), dict(c=0), dict(c=256), dict(q=-1), dict(q=65537), dict(mp=-1),
           dict(K=0), dict(K=-1), dict(fmt=0), dict(fmt=2), dict(n=-1), dict(S=-1), dict(mw=0), dict(mh=0),
           dict(tmp=tmp + 8),                                                  # T is cleared by 16-B vectors
           dict(n=1 << 28, mh=1 << 8),                                         # 17 bands × 2^28 descriptors >= 2^31 blocks
           dict(n=1 << 27)]                                                    # 16 clear blocks × 2^27 = 2^31
    for kw in bad:
        assert b.c_call(**kw) == N.IPP_E_ARG, kw
        torch.cuda.synchronize()
        assert bool((b.rec == POISON).all()), kw                               # nothing was launched
    assert torch.equal(b.runner.tmp, before)


def test_python_refuses_bad_arguments(fused, noise):
    from image_processor_pipeline_amd import _native as N
    b = noise
    b.runner.run(b.dsrc, b.dbgs, torch.empty_like(b.out))
    before = b.runner.tmp.clone()
    out = torch.full_like(b.out, 5)
    bad = [dict(min_visible=-0.1), dict(min_visible=1.5), dict(min_visible=float("nan")), dict(min_visible="0.5"),
           dict(min_visible=True), dict(min_visible=None), dict(min_pixels=-1), dict(min_pixels=1.5),
           dict(min_pixels=True), dict(min_pixels=None), dict(min_pixels=1 << 31), dict(alpha_min=0),
           dict(alpha_min=256), dict(cover_min=0), dict(cover_min=1.5)]
    for kw in bad:
        with pytest.raises(ValueError):
            b.runner.run_culled(b.dsrc, b.dbgs, out, **kw)
        with pytest.raises(ValueError):
            b.runner.run_labelled(b.dsrc, b.dbgs, out, cull=True, **kw)
    for c in ("yes", 1, None):
        with pytest.raises(ValueError):
            b.runner.run_labelled(b.dsrc, b.dbgs, out, cull=c)
    with pytest.raises(ValueError):
        b.runner.run_culled(b.dsrc, b.dbgs, out[:3])
    with pytest.raises(ValueError):
        b.runner.run_culled(b.dsrc[:5], b.dbgs, out)
    torch.cuda.synchronize()
    assert bool((out == 5).all()) and torch.equal(b.runner.tmp, before)         # refused before any launch
    # min_visible above 1 stays legal without cull (it is scene_labels' threshold alone there)
    assert b.runner.run_labelled(b.dsrc, b.dbgs, out, min_visible=2.0)[1] == [[], [], [], []]
    assert fused.SceneRunner.run_culled.__doc__ and "absent" in fused.SceneRunner.run_culled.__doc__
