"""GPU: letterboxed training batches (ipp_scene_feed_letterbox,
ipp_scene_feed_targets_letterbox, ipp_scene_feed_index_map_letterbox,
SceneRunner.feed / run_feed with ``letterbox=True``) against the restatement of
tests/feed_letterbox_refs.py — live Pillow for the pixels, NumPy float64 for
the targets — bit for bit.  Every output of the C entries is pre-filled with
0xA5 and has guard bytes before and behind it that must stay 0xA5."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import feed_letterbox_refs as LR
from tests import feed_refs as FR
from tests import feed_resize_refs as RR
from tests import gpu_scene_support as S
from tests import scene_mask_refs as MR
from tests import scene_refs as SR
from tests.gpu_scene_support import DEV, current_stream as _stream, to_dev_copy as _t
from tests.test_gpu_feed import MEAN, SLACK, STD, _bits, _poisoned, _words

pytestmark = pytest.mark.gpu

GUARD = 64                      # poisoned bytes before every output (SLACK of them behind it)


@pytest.fixture(scope="module")
def fused():
    return S.require_fused()


@pytest.fixture(scope="module")
def N(fused):
    from image_processor_pipeline_amd import _native
    return _native


@pytest.fixture(scope="module")
def lib(N):
    return N.load()


@pytest.fixture(scope="module")
def G(fused):
    from image_processor_pipeline_amd import geometry
    return geometry


def _guarded(nbytes):
    """(buffer, device address of its nbytes payload): GUARD poisoned bytes before, SLACK behind."""
    buf = _poisoned(GUARD + nbytes)
    return buf, buf.data_ptr() + GUARD


def _payload(buf, nbytes, dtype):
    a = buf.cpu().numpy()
    assert np.all(a[:GUARD] == 0xA5) and np.all(a[GUARD + nbytes:] == 0xA5) and len(a) == GUARD + nbytes + SLACK
    return a[GUARD:GUARD + nbytes].copy().view(dtype)


# --- 1: ipp_scene_feed_letterbox on random input ----------------------------------------------------------------
# name: (bg_w, bg_h, out_w, out_h, letterbox_geometry's flags)
SHAPES = {
    "landscape": (37, 23, 64, 64, {}),                       # 64 x 40 at top 12: an odd pad, edges inside tiles
    "portrait": (23, 37, 64, 64, {}),
    "ragged": (100, 75, 96, 80, {}),                         # 96 x 72: not a multiple of the tile
    "reduce": (300, 200, 16, 16, {}),                        # LANCZOS ksize 115: the tile halved
    "upscale": (16, 16, 70, 33, {}),                         # 33 x 33 at left 18: a wide pad, out_w no multiple of 16
    "identity": (40, 40, 40, 64, {}),                        # new = bg: identity taps on both axes, pure pad
    "tiny": (5, 3, 64, 64, dict(scaleup=False)),             # a 5 x 3 rectangle and whole-pad tiles
    "nopad": (64, 32, 64, 32, {}),
    "corner": (37, 23, 64, 64, dict(center=False)),
    "tall": (30, 90, 100, 150, {}),                          # 50 x 150: several tile rows, whole-pad tile columns
}
# (element size, bgr, pad)
COMBOS = [(2, 0, 114), (4, 1, 0), (2, 1, 255), (4, 0, 114)]
N_SCENES = 3
_cache = {}


def _geo(fused, shape):
    bw, bh, ow, oh, flags = SHAPES[shape]
    return fused.letterbox_geometry((bh, bw), (oh, ow), **flags)


def _axis(G, name, n_in, n_out):
    return G.identity_taps(n_in) if n_in == n_out else G.resample_taps(name, n_in, n_out)


def _case(fused, G, shape, name):
    """(img, geo, taps_x, taps_y): the input and the taps of one (shape, filter), made once."""
    key = (shape, name)
    if key not in _cache:
        bw, bh = SHAPES[shape][:2]
        geo = _geo(fused, shape)
        rng = np.random.default_rng(bw * 4096 + bh)
        img = rng.integers(0, 256, (N_SCENES, bh, bw, 3), np.uint8)
        _cache[key] = (img, geo, _axis(G, name, bw, geo.new_w), _axis(G, name, bh, geo.new_h))
    return _cache[key]


def _check_images(fused, lib, G, shape, name, combo, in_off=0):
    es, bgr, pad = combo
    img, geo, tx, ty = _case(fused, G, shape, name)
    n_s, bh, bw = img.shape[:3]
    lut = _words(np.random.default_rng(1000 * es + bgr + bw), es)
    store = torch.full((img.size + 64,), 0x3C, dtype=torch.uint8, device=DEV)
    d_in = store[in_off:in_off + img.size]
    d_in.copy_(torch.from_numpy(img.reshape(-1)))
    assert d_in.data_ptr() % 16 == in_off
    d_lut, d_tx, d_ty = _t(lut.view(np.uint8)), _t(tx[1]), _t(ty[1])
    nbytes = n_s * 3 * geo.out_h * geo.out_w * es
    buf, o = _guarded(nbytes)
    assert lib.ipp_scene_feed_letterbox(d_in.data_ptr(), o, d_lut.data_ptr(), d_tx.data_ptr(), d_ty.data_ptr(), n_s, bw,
                                        bh, geo.new_w, geo.new_h, geo.left, geo.top, geo.out_w, geo.out_h, tx[0], ty[0],
                                        pad, es, bgr, _stream()) == 0
    got = _payload(buf, nbytes, lut.dtype).reshape(n_s, 3, geo.out_h, geo.out_w)
    exp = LR.images(img, lut, bool(bgr), geo, name, pad)
    bad = np.argwhere(got != exp)
    assert len(bad) == 0, (len(bad), bad[:6].tolist())
    # the plain stretch to the rectangle's size, by the entry of before, is the rectangle cut out of the canvas
    rbytes = n_s * 3 * geo.new_h * geo.new_w * es
    rbuf, ro = _guarded(rbytes)
    assert lib.ipp_scene_feed_resize(d_in.data_ptr(), ro, d_lut.data_ptr(), d_tx.data_ptr(), d_ty.data_ptr(), n_s, bw, bh,
                                     geo.new_w, geo.new_h, tx[0], ty[0], es, bgr, _stream()) == 0
    plain = _payload(rbuf, rbytes, lut.dtype).reshape(n_s, 3, geo.new_h, geo.new_w)
    assert np.array_equal(plain, got[:, :, geo.top:geo.top + geo.new_h, geo.left:geo.left + geo.new_w])


@pytest.mark.parametrize("combo", COMBOS, ids=lambda c: f"es{c[0]}-bgr{c[1]}-pad{c[2]}")
@pytest.mark.parametrize("shape", list(SHAPES))
def test_letterbox_images(fused, lib, G, shape, combo):
    name = "lanczos" if shape == "reduce" else "bilinear"
    if shape == "reduce":
        assert G.resample_taps("lanczos", 300, 16)[0] == 115
    if shape == "identity":
        geo = _geo(fused, shape)
        assert (geo.new_w, geo.new_h, geo.top) == (40, 40, 12)
    _check_images(fused, lib, G, shape, name, combo)


@pytest.mark.parametrize("name", RR.FILTERS)
@pytest.mark.parametrize("shape", ["landscape", "ragged"])
def test_letterbox_images_all_filters(fused, lib, G, shape, name):
    _check_images(fused, lib, G, shape, name, (2, 1, 114))


@pytest.mark.parametrize("es", [2, 4])
@pytest.mark.parametrize("in_off", [1, 5])
def test_letterbox_images_unaligned_input(fused, lib, G, in_off, es):
    _check_images(fused, lib, G, "portrait", "bicubic", (es, 0, 114), in_off=in_off)


def test_geometries_of_the_shapes(fused):
    """The shapes are what their comments say: the cases above cover what they name."""
    L = fused.Letterbox
    assert _geo(fused, "landscape") == L(64, 64, 40, 64, 12, 0) and _geo(fused, "portrait") == L(64, 64, 64, 40, 0, 12)
    assert _geo(fused, "ragged") == L(80, 96, 72, 96, 4, 0) and _geo(fused, "reduce") == L(16, 16, 11, 16, 2, 0)
    assert _geo(fused, "upscale") == L(33, 70, 33, 33, 0, 18) and _geo(fused, "tiny") == L(64, 64, 3, 5, 30, 29)
    assert _geo(fused, "nopad") == L(32, 64, 32, 64, 0, 0) and _geo(fused, "corner") == L(64, 64, 40, 64, 0, 0)
    assert _geo(fused, "tall") == L(150, 100, 150, 50, 0, 25)


# --- 2: ipp_scene_feed_targets_letterbox on handmade rows -------------------------------------------------------
BG_W, BG_H = 37, 23
# a box touching each edge, a 1-px box, the full background, one failing the fraction test at min_q = 16384
HAND = [(0, 5, 10, 9, 40, 40), (30, 5, 37, 9, 28, 28), (5, 0, 9, 4, 16, 16), (5, 19, 9, 23, 16, 16), (7, 7, 8, 8, 1, 1),
        (0, 0, 37, 23, 851, 851), (3, 4, 20, 21, 400, 99)]


def _run_targets(lib, entry, rows_desc, scene_layer, ids_desc, n_s, K, extra, min_q):
    T = n_s * K
    (tg, p_tg), (cnt, p_cnt), (slot, p_slot) = _guarded(24 * T), _guarded(4), _guarded(4 * T)
    d_rows, d_sl = _t(rows_desc.astype(np.int32)), _t(scene_layer.astype(np.int32))
    d_ids = _t(ids_desc.astype(np.int32)) if ids_desc is not None else None
    assert getattr(lib, entry)(d_rows.data_ptr(), d_sl.data_ptr(), d_ids.data_ptr() if d_ids is not None else None,
                               len(rows_desc), n_s, K, BG_W, BG_H, min_q, *extra, p_tg, p_cnt, p_slot, _stream()) == 0
    return _payload(tg, 24 * T, np.uint32).reshape(T, 6), int(_payload(cnt, 4, np.int32)[0]), \
        _payload(slot, 4 * T, np.int32).reshape(n_s, K)


@pytest.mark.parametrize("with_ids", [False, True], ids=["class0", "classes"])
@pytest.mark.parametrize("n_s,K", [(1, 1), (128, 8), (205, 5)], ids=["T1", "T1024", "T1025"])
@pytest.mark.parametrize("shape", ["landscape", "tiny", "tall"])
def test_letterbox_targets(fused, lib, shape, n_s, K, with_ids):
    """T = 1, 1024 and 1025 overlays: one chunk, a full one, and one more row than a chunk."""
    bw, bh, ow, oh, flags = SHAPES[shape]
    geo = fused.letterbox_geometry((BG_H, BG_W), (oh, ow), **flags)          # the shape's canvas around this background
    T, min_q = n_s * K, 16384
    rng = np.random.default_rng(T + ow)
    rows = FR.random_rows(rng, n_s, K, BG_W, BG_H).reshape(T, 6)
    rows[:min(T, len(HAND))] = HAND[:T]
    if T > len(HAND):
        rows[T - 1] = HAND[4]                                   # the row behind the chunk boundary is kept
    rows = rows.reshape(n_s, K, 6)
    present = np.ones(T, bool)
    if T > 8:
        present[8] = False                                      # an absent overlay: no descriptor maps there
    ids = rng.integers(0, 1000, T).astype(np.int32) if with_ids else None
    desc_item = rng.permutation(T)                              # the descriptors in any order
    desc_item = desc_item[present[desc_item]]
    scene_layer = np.stack([desc_item // K, desc_item % K], axis=1)
    exp_tg, exp_n, exp_slot = LR.targets(rows, ids if with_ids else 0, BG_W, BG_H, min_q, geo, present.reshape(n_s, K))
    assert exp_n > 0 and (T == 1 or exp_n < T)
    if T > len(HAND):
        assert exp_slot.reshape(-1)[6] == -1 and exp_slot.reshape(-1)[8] == -1 and exp_slot.reshape(-1)[T - 1] == exp_n - 1
    rect = (geo.new_w, geo.new_h, geo.left, geo.top, geo.out_w, geo.out_h)
    args = (rows.reshape(T, 6)[desc_item], scene_layer, ids[desc_item] if with_ids else None, n_s, K)
    tg, n, slot = _run_targets(lib, "ipp_scene_feed_targets_letterbox", *args, rect, min_q)
    assert n == exp_n and np.array_equal(slot, exp_slot)
    bad = np.argwhere(tg != exp_tg.view(np.uint32))
    assert len(bad) == 0, (len(bad), bad[:6].tolist())
    # the same slot and count as the plain entry on the same rows (its ROW is another)
    tg0, n0, slot0 = _run_targets(lib, "ipp_scene_feed_targets", *args, (), min_q)
    assert n0 == n and np.array_equal(slot0, slot) and np.array_equal(tg0[:, :2], tg[:, :2])


# --- 3: ipp_scene_feed_index_map_letterbox on random maps -------------------------------------------------------
@pytest.mark.parametrize("K", [1, 8])
@pytest.mark.parametrize("shape", ["landscape", "upscale", "tiny"])
def test_letterbox_index_map(fused, lib, G, shape, K):
    bw, bh = SHAPES[shape][:2]
    geo = _geo(fused, shape)
    n_s = N_SCENES
    pitch, opitch = (bw + 15) // 16 * 16, (geo.out_w + 15) // 16 * 16
    rng = np.random.default_rng(bw * 64 + K)
    vis = rng.integers(0, 1 << K, (n_s, bh, pitch), np.uint8)                # the padding columns hold noise too
    keep = rng.random((n_s, K)) < 0.6
    keep[1], keep[0, K - 1] = False, True
    slot = np.where(keep, np.cumsum(keep.reshape(-1)).reshape(n_s, K) - 1, -1).astype(np.int32)
    exp = LR.index_map(FR.index_map(vis, slot, bw)[:, :, :bw], geo)
    assert exp.any()
    xt, yt = G.nearest_table(bw, geo.new_w), G.nearest_table(bh, geo.new_h)
    d_vis, d_slot, d_xt, d_yt = _t(vis), _t(slot), _t(xt), _t(yt)
    nbytes = n_s * geo.out_h * opitch
    buf, o = _guarded(nbytes)
    assert lib.ipp_scene_feed_index_map_letterbox(d_vis.data_ptr(), pitch, bw, bh, d_slot.data_ptr(), n_s, K,
                                                  d_xt.data_ptr(), d_yt.data_ptr(), geo.new_w, geo.new_h, geo.left,
                                                  geo.top, geo.out_w, geo.out_h, o, opitch, _stream()) == 0
    got = _payload(buf, nbytes, np.uint8).reshape(n_s, geo.out_h, opitch)
    assert np.all(got[:, :, geo.out_w:] == 0)
    inside = np.zeros((geo.out_h, opitch), bool)
    inside[geo.top:geo.top + geo.new_h, geo.left:geo.left + geo.new_w] = True
    assert np.all(got[:, ~inside] == 0)
    assert np.array_equal(got[:, :, :geo.out_w], exp)


# --- 4: through the runner --------------------------------------------------------------------------------------
class Scenes(S.SceneBatch):
    def __init__(self, fused, batch):
        super().__init__(fused, batch)
        self.composites = self.out.cpu().numpy()
        self.ids = np.random.default_rng(3).integers(0, 80, self.plan.n_scenes * self.plan.per_scene).tolist()


@pytest.fixture(scope="module")
def batch(fused):
    return Scenes(fused, MR.odd_scenes(fused))


def _same(a, b):
    for x, y in zip(a, b):
        assert (x is None) == (y is None)
        if x is not None:
            assert x.shape == y.shape and x.dtype == y.dtype
            assert torch.equal(x.view(torch.uint8) if x.is_floating_point() else x,
                               y.view(torch.uint8) if y.is_floating_point() else y)


def test_run_feed_letterboxed_and_the_plain_calls_unchanged(fused, batch):
    b, plan = batch, batch.plan
    runner, out = fused.SceneRunner(plan, DEV), torch.full_like(b.out, 200)
    kw = dict(mean=MEAN, std=STD, class_ids=b.ids, index_map=True, min_visible=0.25)
    before = [runner.run_feed(b.dsrc, b.dbgs, out, **kw), runner.feed(out, size=(64, 48), resample="lanczos", **kw),
              runner.feed(out, size=(40, 64), **kw)]
    assert torch.equal(out, b.out)
    fd = runner.run_feed(b.dsrc, b.dbgs, out, size=(64, 48), letterbox=True, resample="lanczos", **kw)
    assert isinstance(fd, fused.SceneFeed) and len(fd) == 5 and torch.equal(out, b.out)
    geo = fused.letterbox_geometry((plan.bg_h, plan.bg_w), (64, 48))
    assert (geo.out_h, geo.out_w) == (64, 48) and (geo.new_h, geo.new_w) != (64, 48)
    assert tuple(fd.images.shape) == (plan.n_scenes, 3, 64, 48) and fd.images.dtype == torch.float16
    lut = fused.feed_lut(MEAN, STD)
    assert np.array_equal(_bits(fd.images), LR.images(b.composites, _bits(lut), False, geo, "lanczos", 114))
    rows = SR.scene_rows(plan, b.overlays, 1, 128)
    exp_tg, exp_n, exp_slot = LR.targets(rows, b.ids, plan.bg_w, plan.bg_h, 16384, geo)
    assert exp_n > 0 and int(fd.count.cpu()[0]) == exp_n and np.array_equal(fd.slot.cpu().numpy(), exp_slot)
    assert np.array_equal(_bits(fd.targets), exp_tg.view(np.int32))
    assert tuple(fd.index_map.shape) == (plan.n_scenes, 64, 48) and fd.index_map.dtype == torch.uint8
    assert np.array_equal(fd.index_map.cpu().numpy(), LR.index_map(before[0].index_map.cpu().numpy(), geo))
    _same(fd, runner.feed(out, size=(64, 48), letterbox=True, resample="lanczos", **kw))
    # flags and the pad value, against the references; an `images` of the caller's
    mine = torch.full((plan.n_scenes, 3, 90, 70), -7.0, dtype=torch.float32, device=DEV)
    fd2 = runner.feed(out, size=(90, 70), letterbox=True, pad_value=0, scaleup=False, center=False, bgr=True,
                      dtype=torch.float32, images=mine, **kw)
    geo2 = fused.letterbox_geometry((plan.bg_h, plan.bg_w), (90, 70), scaleup=False, center=False)
    assert fd2.images is mine and (geo2.top, geo2.left) == (0, 0)
    assert np.array_equal(_bits(mine), LR.images(b.composites, _bits(fused.feed_lut(MEAN, STD, torch.float32)), True,
                                                 geo2, "bilinear", 0))
    assert np.array_equal(_bits(fd2.targets), LR.targets(rows, b.ids, plan.bg_w, plan.bg_h, 16384, geo2)[0].view(np.int32))
    assert np.array_equal(fd2.index_map.cpu().numpy(), LR.index_map(before[0].index_map.cpu().numpy(), geo2))
    # the calls without letterbox return what they returned before any letterboxed call on this runner
    after = [runner.run_feed(b.dsrc, b.dbgs, out, **kw), runner.feed(out, size=(64, 48), resample="lanczos", **kw),
             runner.feed(out, size=(40, 64), letterbox=False, **kw)]
    for x, y in zip(before, after):
        _same(x, y)


def test_letterbox_arguments_are_checked(batch):
    b = batch
    for kw in (dict(letterbox=True), dict(letterbox=True, size=None), dict(letterbox=1, size=8),
               dict(letterbox=None, size=8), dict(letterbox="yes", size=8), dict(letterbox=True, size=8, pad_value=-1),
               dict(letterbox=True, size=8, pad_value=256), dict(letterbox=True, size=8, pad_value=114.0),
               dict(letterbox=True, size=8, pad_value=True), dict(size=8, pad_value=300), dict(pad_value=None),
               dict(letterbox=True, size=8, scaleup=1), dict(letterbox=True, size=8, center=0), dict(scaleup=None),
               dict(center="no"), dict(letterbox=True, size=0), dict(letterbox=True, size=(1 << 14, 1 << 14)),
               dict(letterbox=True, size=8, resample="nearest")):
        with pytest.raises(ValueError):
            b.runner.feed(b.out, **kw)
        with pytest.raises(ValueError):
            b.runner.run_feed(b.dsrc, b.dbgs, b.out, **kw)
    wrong = torch.empty((b.plan.n_scenes, 3, 8, 9), dtype=torch.float16, device=DEV)
    with pytest.raises(ValueError):
        b.runner.feed(b.out, letterbox=True, size=8, images=wrong)
