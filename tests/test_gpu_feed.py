"""GPU: training batches left on the device (ipp_scene_feed_images,
ipp_scene_feed_targets, ipp_scene_feed_index_map, SceneRunner.feed / run_feed)
against the NumPy references of tests/feed_refs.py, bit for bit.  Every output
of the C entries is pre-filled with 0xA5 and has slack behind it that must stay
0xA5."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import feed_refs as FR
from tests import gpu_scene_support as S
from tests import scene_mask_refs as MR
from tests import scene_refs as SR
from tests.gpu_scene_support import DEV, current_stream as _stream, to_dev_copy as _t

pytestmark = pytest.mark.gpu

SLACK = 64                      # poisoned bytes behind every output
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


@pytest.fixture(scope="module")
def fused():
    return S.require_fused()


@pytest.fixture(scope="module")
def lib(fused):
    from image_processor_pipeline_amd import _native as N
    return N.load()


def _poisoned(nbytes):
    return torch.full((nbytes + SLACK,), 0xA5, dtype=torch.uint8, device=DEV)


def _back(buf, nbytes, dtype):
    """(the first nbytes of a poisoned buffer as dtype, True when the slack is untouched)."""
    a = buf.cpu().numpy()
    return a[:nbytes].view(dtype), bool(np.all(a[nbytes:] == 0xA5))


def _words(rng, es):
    """A (3, 256) table of distinct random words of es bytes: a wrong index cannot hide."""
    if es == 2:
        return rng.permutation(65536)[:768].astype(np.uint16).reshape(3, 256)
    w = np.unique(rng.integers(0, 1 << 32, 4096, dtype=np.uint64))[:768].astype(np.uint32)
    return rng.permutation(w).reshape(3, 256)


# --- 1: the C entries on handmade input ----------------------------------------------------------------------
# (S, H, W): all tail; all tail, three scenes' worth of odd slots; an odd slot, scenes 1 and 2 misaligned on both
# sides; fully aligned; more than one block per scene with a ragged end
SHAPES = [(1, 1, 1), (2, 3, 5), (3, 97, 125), (2, 64, 64), (1, 257, 263)]


@pytest.mark.parametrize("bgr", [0, 1])
@pytest.mark.parametrize("es", [2, 4])
@pytest.mark.parametrize("shape", SHAPES + ["in+5", "out+1"], ids=str)
def test_images(lib, shape, es, bgr):
    """'in+5': the input is a view 5 bytes into a larger buffer (not 16-B aligned); 'out+1': the output starts one
    element into its buffer."""
    in_off = 5 if shape == "in+5" else 0
    out_off = es if shape == "out+1" else 0
    n_s, H, W = (2, 33, 47) if isinstance(shape, str) else shape
    rng = np.random.default_rng(1000 * es + bgr + H)
    img = rng.integers(0, 256, (n_s, H, W, 3), np.uint8)
    lut = _words(rng, es)
    exp = FR.images(img, lut, bool(bgr))
    store = torch.full((img.size + 64,), 0x3C, dtype=torch.uint8, device=DEV)
    d_in = store[in_off:in_off + img.size]
    d_in.copy_(torch.from_numpy(img.reshape(-1)))
    assert d_in.data_ptr() % 16 == in_off
    nbytes = exp.size * es
    buf = _poisoned(out_off + nbytes)
    d_lut = _t(lut.view(np.uint8))
    rc = lib.ipp_scene_feed_images(d_in.data_ptr(), buf.data_ptr() + out_off, d_lut.data_ptr(), n_s, W, H, es, bgr,
                                   _stream())
    assert rc == 0
    a = buf.cpu().numpy()
    assert np.all(a[:out_off] == 0xA5) and np.all(a[out_off + nbytes:] == 0xA5)
    got = a[out_off:out_off + nbytes].copy().view(lut.dtype).reshape(exp.shape)
    bad = np.argwhere(got != exp)
    assert len(bad) == 0, (len(bad), bad[:6].tolist())


def _targets_case(rng, n_s, K, bw, bh):
    """Rows in scene, layer order, class ids by overlay, and the descriptor order of a scene plan: layer-major,
    the scenes grouped (stably) by a random background."""
    rows = FR.random_rows(rng, n_s, K, bw, bh)
    if n_s > 6:
        rows[3, :, 5] = 0                                       # a scene with nothing kept
        rows[5] = (1, 2, 30, 40, 96, 96)                        # and one with all kept, at every min_q
    ids = rng.integers(0, 1000, n_s * K).astype(np.int32)
    order = np.argsort(rng.integers(0, 5, n_s), kind="stable")
    desc_item = (order[None, :] * K + np.arange(K)[:, None]).reshape(-1)
    return rows, ids, desc_item


def _run_targets(lib, rows_desc, scene_layer, ids_desc, n_s, K, bw, bh, min_q):
    T = n_s * K
    tg, cnt, slot = _poisoned(24 * T), _poisoned(4), _poisoned(4 * T)
    d_rows, d_sl = _t(rows_desc.astype(np.int32)), _t(scene_layer.astype(np.int32))
    d_ids = _t(ids_desc.astype(np.int32)) if ids_desc is not None else None
    rc = lib.ipp_scene_feed_targets(d_rows.data_ptr(), d_sl.data_ptr(), d_ids.data_ptr() if d_ids is not None else None,
                                    len(rows_desc), n_s, K, bw, bh, min_q, tg.data_ptr(), cnt.data_ptr(),
                                    slot.data_ptr(), _stream())
    assert rc == 0
    (g_tg, ok1), (g_cnt, ok2), (g_slot, ok3) = _back(tg, 24 * T, np.uint32), _back(cnt, 4, np.int32), \
        _back(slot, 4 * T, np.int32)
    assert ok1 and ok2 and ok3
    return g_tg.reshape(T, 6), int(g_cnt[0]), g_slot.reshape(n_s, K)


@pytest.mark.parametrize("min_q", [0, 16384, 65536])
def test_targets_2600_overlays_in_descriptor_order(lib, min_q):
    n_s, K, bw, bh = 325, 8, 1920, 1080                         # 2600 overlays: more than two chunks of 1024
    rows, ids, desc_item = _targets_case(np.random.default_rng(5), n_s, K, bw, bh)
    exp_tg, exp_n, exp_slot = FR.targets(rows, ids, bw, bh, min_q)
    assert 0 < exp_n < n_s * K and np.all(exp_slot[3] < 0) and np.all(exp_slot[5] >= 0)
    scene_layer = np.stack([desc_item // K, desc_item % K], axis=1)
    tg, n, slot = _run_targets(lib, rows.reshape(-1, 6)[desc_item], scene_layer, ids[desc_item], n_s, K, bw, bh, min_q)
    assert n == exp_n and np.array_equal(slot, exp_slot)
    bad = np.argwhere(tg != exp_tg.view(np.uint32))
    assert len(bad) == 0, (len(bad), bad[:6].tolist())


def test_targets_one_descriptor(lib):
    rows = np.array([[3, 5, 10, 6, 20, 7]], np.int32)
    for min_q, keep in ((0, True), (22937, True), (22938, False)):           # 65536·7 = 458752 = 22937.6·20
        tg, n, slot = _run_targets(lib, rows, np.array([[0, 0]]), None, 1, 1, 13, 7, min_q)
        exp_tg, exp_n, exp_slot = FR.targets(rows[None], 0, 13, 7, min_q)
        assert exp_n == int(keep) and n == exp_n and np.array_equal(slot, exp_slot)
        assert np.array_equal(tg, exp_tg.view(np.uint32))
    # one descriptor of a 2 x 2 batch, with a class: the three other overlays are absent
    tg, n, slot = _run_targets(lib, rows, np.array([[1, 0]]), np.array([9]), 2, 2, 13, 7, 0)
    present = np.array([[False, False], [True, False]])
    exp_tg, exp_n, exp_slot = FR.targets(np.broadcast_to(rows, (2, 2, 6)), 9, 13, 7, 0, present)
    assert n == exp_n == 1 and np.array_equal(slot, exp_slot) and np.array_equal(tg, exp_tg.view(np.uint32))
    # a descriptor that scene_layer maps nowhere is ignored
    tg, n, slot = _run_targets(lib, rows, np.array([[2, 0]]), None, 2, 2, 13, 7, 0)
    assert n == 0 and np.all(slot == -1) and np.all(tg.view(np.float32) == -1)


@pytest.mark.parametrize("W,H,pitch", [(16, 7, 16), (125, 40, 128), (160, 131, 160), (16, 5, 48)])
def test_index_map(lib, W, H, pitch):
    n_s, K = 3, 8
    rng = np.random.default_rng(W + pitch)
    vis = rng.integers(0, 256, (n_s, H, pitch), np.uint8)                    # the padding columns hold noise too
    keep = rng.random((n_s, K)) < 0.6
    keep[1] = False
    slot = np.where(keep, np.cumsum(keep.reshape(-1)).reshape(n_s, K) - 1, -1).astype(np.int32)
    exp = FR.index_map(vis, slot, W)
    out = _poisoned(vis.size)
    d_vis, d_slot = _t(vis), _t(slot)
    assert lib.ipp_scene_feed_index_map(d_vis.data_ptr(), pitch, W, H, d_slot.data_ptr(), n_s, K, out.data_ptr(),
                                        _stream()) == 0
    got, ok = _back(out, vis.size, np.uint8)
    assert ok and np.all(got.reshape(vis.shape)[:, :, W:] == 0)
    assert np.array_equal(got.reshape(vis.shape), exp)


def test_c_entries_refuse_bad_arguments(lib):
    """IPP_E_ARG for every refused argument; nothing is launched, so the poisoned outputs stay poisoned."""
    E = -1
    buf, out = _poisoned(4096), _poisoned(4096)
    p, o = buf.data_ptr(), out.data_ptr()

    def img(**kw):
        a = dict(inp=p, out=o, lut=p, S=1, W=4, H=4, es=2, bgr=0)
        a.update(kw)
        return lib.ipp_scene_feed_images(a["inp"], a["out"], a["lut"], a["S"], a["W"], a["H"], a["es"], a["bgr"], _stream())

    for kw in (dict(inp=None), dict(out=None), dict(lut=None), dict(S=0), dict(S=-1), dict(W=0), dict(H=0), dict(H=-3),
               dict(es=1), dict(es=3), dict(es=8), dict(es=0), dict(bgr=2), dict(bgr=-1), dict(out=o + 1),
               dict(es=4, out=o + 2), dict(es=4, lut=p + 2), dict(W=1 << 14, H=1 << 14)):
        assert img(**kw) == E, kw

    def tg(**kw):
        a = dict(rows=p, sl=p, ids=None, n=1, S=1, K=1, W=8, H=8, q=0, t=o, c=o + 256, s=o + 512)
        a.update(kw)
        return lib.ipp_scene_feed_targets(a["rows"], a["sl"], a["ids"], a["n"], a["S"], a["K"], a["W"], a["H"], a["q"],
                                          a["t"], a["c"], a["s"], _stream())

    for kw in (dict(rows=None), dict(sl=None), dict(t=None), dict(c=None), dict(s=None), dict(n=-1), dict(S=0),
               dict(K=0), dict(W=0), dict(H=0), dict(W=(1 << 23) + 1), dict(H=(1 << 23) + 1), dict(q=-1), dict(q=65537),
               dict(n=(1 << 20) + 1), dict(S=1 << 11, K=(1 << 9) + 1), dict(rows=p + 2), dict(ids=p + 1), dict(t=o + 2),
               dict(s=o + 513)):
        assert tg(**kw) == E, kw

    def im(**kw):
        a = dict(m=p, pitch=16, W=16, H=4, s=p, S=1, K=8, out=o)
        a.update(kw)
        return lib.ipp_scene_feed_index_map(a["m"], a["pitch"], a["W"], a["H"], a["s"], a["S"], a["K"], a["out"], _stream())

    for kw in (dict(m=None), dict(s=None), dict(out=None), dict(S=0), dict(W=0), dict(H=0), dict(K=0), dict(K=9),
               dict(pitch=15), dict(pitch=24), dict(W=17), dict(pitch=1 << 31), dict(m=p + 4), dict(out=o + 8),
               dict(s=p + 2)):
        assert im(**kw) == E, kw
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all())


# --- 2: through the runner -----------------------------------------------------------------------------------
class Scenes(S.SceneBatch):
    def __init__(self, fused, batch):
        super().__init__(fused, batch)
        self.composites = SR.scene_composites(self.bgs, self.plan, self.overlays)
        self._refs = {}
        rng = np.random.default_rng(3)
        self.ids = rng.integers(0, 80, self.plan.n_scenes * self.plan.per_scene).tolist()

    def ref(self, a, c):
        """(rows (S, K, 6), map (S, bg_h, pitch)) of the references, computed once."""
        if (a, c) not in self._refs:
            self._refs[(a, c)] = (SR.scene_rows(self.plan, self.overlays, a, c),
                                  MR.scene_map(self.plan, self.overlays, a, c))
        return self._refs[(a, c)]


@pytest.fixture(scope="module")
def batches(fused):
    return {"noise": Scenes(fused, MR.noise_scenes(fused)), "odd": Scenes(fused, MR.odd_scenes(fused)),
            "eight": Scenes(fused, MR.layered_scene(fused, 8))}


def _bits(t):
    """A float tensor's words on the host."""
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32).cpu().numpy()


def _check_feed(b, fd, lut, bgr, ids, a, c, min_visible, with_map):
    from image_processor_pipeline_amd import labels_fmt as L
    plan = b.plan
    rows, vis = b.ref(a, c)
    assert np.array_equal(_bits(fd.images), FR.images(b.composites, _bits(lut), bgr))
    exp_tg, exp_n, exp_slot = FR.targets(rows, ids, plan.bg_w, plan.bg_h, L.min_visible_q(min_visible))
    assert int(fd.count.cpu()[0]) == exp_n and np.array_equal(fd.slot.cpu().numpy(), exp_slot)
    assert np.array_equal(_bits(fd.targets), exp_tg.view(np.int32))
    if with_map:
        assert tuple(fd.index_map.shape) == (plan.n_scenes, plan.bg_h, plan.bg_w)
        assert np.array_equal(fd.index_map.cpu().numpy(), FR.index_map(vis, exp_slot, plan.bg_w)[:, :, :plan.bg_w])
    else:
        assert fd.index_map is None
    return exp_n


@pytest.mark.parametrize("name,dtype,bgr,min_visible,with_map,levels", [
    ("noise", "float16", False, 0.0, True, (1, 128)), ("noise", "bfloat16", True, 0.5, True, (128, 255)),
    ("noise", "float32", True, 0.5, False, (1, 128)), ("odd", "float16", True, 0.5, True, (1, 128)),
    ("odd", "bfloat16", False, 0.0, False, (1, 128)), ("eight", "float16", False, 0.5, True, (1, 128)),
    ("eight", "bfloat16", True, 0.0, True, (255, 1))])
def test_feed_against_the_references(fused, batches, name, dtype, bgr, min_visible, with_map, levels):
    b, dtype = batches[name], getattr(torch, dtype)
    fd = b.runner.feed(b.out, mean=MEAN, std=STD, dtype=dtype, bgr=bgr, class_ids=b.ids, alpha_min=levels[0],
                       cover_min=levels[1], min_visible=min_visible, index_map=with_map)
    assert isinstance(fd, fused.SceneFeed) and fd.images.dtype == dtype and fd.images.is_cuda and fd.targets.is_cuda
    n = _check_feed(b, fd, fused.feed_lut(MEAN, STD, dtype), bgr, b.ids, levels[0], levels[1], min_visible, with_map)
    assert n > 0
    tg = fd.targets.cpu().numpy()
    assert np.array_equal(tg[:, 0] >= 0, np.arange(len(tg)) < n)             # the mask a consumer uses


def test_feed_takes_a_table_and_a_single_class(fused, batches):
    b = batches["odd"]
    lut = fused.feed_lut((10.0, 20.0, 30.0), (50.0, 60.0, 70.0), torch.float16, scale=1.0)
    for table in (lut, lut.to(DEV)):
        fd = b.runner.feed(b.out, lut=table, class_ids=7, dtype=torch.float32)          # the table's dtype decides
        assert fd.images.dtype == torch.float16
        _check_feed(b, fd, lut, False, 7, 1, 128, 0.0, False)


def test_run_feed_with_cull_matches_run_culled(fused, batches):
    b = batches["noise"]
    ref_out = torch.full_like(b.out, 9)
    _, kept, _ = fused.SceneRunner(b.plan, DEV).run_culled(b.dsrc, b.dbgs, ref_out, min_visible=0.5)
    assert kept.any() and not kept.all()
    runner, out = fused.SceneRunner(b.plan, DEV), torch.full_like(b.out, 200)
    fd = runner.run_feed(b.dsrc, b.dbgs, out, mean=MEAN, std=STD, min_visible=0.5, cull=True, index_map=True)
    assert torch.equal(out, ref_out)
    slot = fd.slot.cpu().numpy()
    assert np.array_equal(slot >= 0, kept) and int(fd.count.cpu()[0]) == int(kept.sum())
    assert np.array_equal(_bits(fd.images), FR.images(ref_out.cpu().numpy(), _bits(fused.feed_lut(MEAN, STD)), False))
    # every visible pixel of the culled composites belongs to a kept overlay: the index map hides nothing
    vis = runner.scene_masks().cpu().numpy()
    assert np.array_equal(fd.index_map.cpu().numpy() > 0, vis > 0)
    # without the cull, run_feed is run + feed
    fd2 = runner.run_feed(b.dsrc, b.dbgs, out, dtype=torch.bfloat16, class_ids=b.ids, index_map=True)
    assert torch.equal(out, b.out)
    _check_feed(b, fd2, fused.feed_lut(dtype=torch.bfloat16), False, b.ids, 1, 128, 0.0, True)


def test_images_argument(fused, batches):
    b = batches["odd"]
    shape = (b.plan.n_scenes, 3, b.plan.bg_h, b.plan.bg_w)
    mine = torch.full(shape, -7.0, dtype=torch.float16, device=DEV)
    fd = b.runner.feed(b.out, mean=MEAN, std=STD, images=mine)
    assert fd.images is mine
    assert np.array_equal(_bits(mine), FR.images(b.composites, _bits(fused.feed_lut(MEAN, STD)), False))
    for wrong in (mine.to(torch.float32), mine[:, :, :, :-1], mine[:2], mine.cpu(), mine.permute(0, 1, 3, 2),
                  mine.cpu().numpy()):
        with pytest.raises(ValueError):
            b.runner.feed(b.out, mean=MEAN, std=STD, images=wrong)


def test_python_guards(fused, batches):
    b = batches["noise"]
    with pytest.raises(ValueError, match="no run"):
        fused.SceneRunner(b.plan, DEV).feed(b.out)
    nine = MR.layered_scene(fused, 9)
    runner = fused.SceneRunner(nine[2], DEV)
    out9 = torch.empty((1,) + nine[1].shape[1:], dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="9 layers"):
        runner.run_feed(_t(nine[0]), _t(nine[1]), out9, index_map=True)
    fd = runner.run_feed(_t(nine[0]), _t(nine[1]), out9)                     # nine layers without the map are fine
    assert tuple(fd.slot.shape) == (1, 9) and fd.index_map is None
    with pytest.raises(ValueError, match="9 layers"):
        runner.feed(out9, index_map=True)
    lut = fused.feed_lut()
    for kw in (dict(dtype=torch.float64), dict(lut=lut.to(torch.float64)), dict(lut=lut[:, :255]), dict(lut=lut.numpy()),
               dict(std=(1, 0, 1)), dict(mean=(1, 2)), dict(bgr=1), dict(index_map=1), dict(alpha_min=0),
               dict(cover_min=256), dict(min_visible=1.5), dict(class_ids=[1, 2]), dict(class_ids=-1),
               dict(class_ids=[(1 << 24) + 1] * 12)):
        with pytest.raises(ValueError):
            b.runner.feed(b.out, **kw)
    for wrong in (b.out[:3], b.out.cpu(), b.out.to(torch.int8), b.out[:, :, :, :2], b.out.permute(0, 2, 1, 3)):
        with pytest.raises(ValueError):
            b.runner.feed(wrong)
    with pytest.raises(ValueError):
        b.runner.run_feed(b.dsrc, b.dbgs, b.out, cull=1)
    with pytest.raises(ValueError):
        b.runner.run_feed(b.dsrc, b.dbgs, b.out, cull=True, min_pixels=-1)


def test_feed_does_not_synchronise(fused, batches):
    """The second call, with the table and the class ids cached, under torch's sync debug mode "error": any
    synchronising call (a copy back, an upload from pageable memory, .item()) would raise."""
    b = batches["noise"]
    kw = dict(mean=MEAN, std=STD, dtype=torch.bfloat16, bgr=True, class_ids=b.ids, min_visible=0.25, index_map=True)
    first = b.runner.feed(b.out, **kw)
    torch.cuda.synchronize()
    try:
        prev = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")
    except (AttributeError, RuntimeError) as e:
        pytest.skip(f"this torch build does not offer set_sync_debug_mode on ROCm: {e}")
    try:
        second = b.runner.feed(b.out, **kw)
        flagged = False
        try:
            b.out[0, 0, 0, 0].item()                                         # the control: this one does synchronise
        except RuntimeError:
            flagged = True
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    if not flagged:
        pytest.skip("this torch build's sync debug mode does not flag a synchronising copy on ROCm")
    for x, y in zip(first, second):
        assert torch.equal(x, y)
