"""CPU: the rule of the device resize of the training batches against live
Pillow.  The NumPy restatement of tests/feed_resize_refs.py, driven by the
tables of ipp_plan_resample, must equal Image.resize for Pillow's five
convolution filters; the NEAREST coordinate tables must equal Pillow's; the
LANCZOS plan must be ipp_plan_lanczos'; the C entries refuse bad arguments
before any launch (no device is needed to be refused); the LDS extents fit
their budget for every admitted ksize."""
import ctypes

import numpy as np
import pytest
from PIL import Image

from tests import feed_resize_refs as RR

# (h, w) -> (oh, ow): odd sizes, up-scaling, one axis unchanged, everything into one pixel, tiny up-scaling
PAIRS = [((37, 53), (23, 31)), ((53, 37), (64, 64)), ((97, 125), (40, 125)), ((97, 125), (97, 33)),
         ((64, 64), (65, 129)), ((200, 300), (33, 47)), ((5, 7), (1, 1)), ((3, 2), (9, 11)),
         ((256, 256), (160, 160)), ((130, 70), (129, 17))]
PIL_FILTER = {"box": Image.Resampling.BOX, "bilinear": Image.Resampling.BILINEAR, "hamming": Image.Resampling.HAMMING,
              "bicubic": Image.Resampling.BICUBIC, "lanczos": Image.Resampling.LANCZOS}


@pytest.fixture(scope="module")
def native():
    from image_processor_pipeline_amd import _native as N
    try:
        return N, N.load()
    except N.NativeUnavailable as e:
        pytest.fail(f"libipp.so is not built: {e}")


@pytest.fixture(scope="module")
def G(native):
    from image_processor_pipeline_amd import geometry
    return geometry


def _contents(h, w, seed):
    rng = np.random.default_rng(seed)
    return {"random": rng.integers(0, 256, (h, w, 3), np.uint8),
            "noise": (rng.integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)}


def _axis(G, name, n_in, n_out):
    """(bounds, taps) from the C planner, or the identity taps for the axis Pillow skips."""
    k, buf = G.identity_taps(n_in) if n_in == n_out else G.resample_taps(name, n_in, n_out)
    return k, RR.unpack(buf, n_out, k)


@pytest.mark.parametrize("name", RR.FILTERS)
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0][0]}x{p[0][1]}to{p[1][0]}x{p[1][1]}")
def test_restatement_on_the_planner_tables_equals_pillow(G, pair, name):
    (h, w), (oh, ow) = pair
    kx, tx = _axis(G, name, w, ow)
    ky, ty = _axis(G, name, h, oh)
    for n_in, n_out, k, t in ((w, ow, kx, tx), (h, oh, ky, ty)):            # the Python coefficients are the C ones
        ek, eb, et = RR.axis(name, n_in, n_out)
        assert k == ek and np.array_equal(t[0], eb) and np.array_equal(t[1], et)
    for what, img in _contents(h, w, h * 1000 + w).items():
        exp = np.asarray(Image.fromarray(img).resize((ow, oh), PIL_FILTER[name]))
        got = RR.resize(img, oh, ow, tx, ty)
        assert got.shape == exp.shape and np.array_equal(got, exp), (what, int((got != exp).sum()))


def test_the_order_of_the_rule_is_observable(G):
    """On ipp_plan_resample's tables: the rule's order (H, rounded to uint8, then V) gives Pillow's bytes, and an
    intermediate kept unrounded, or the vertical pass first, gives other bytes.  That the device keeps the order is
    what the GPU tests pin on the same noise content; this shows that they can."""
    img = _contents(37, 53, 7)["noise"]
    for name in ("bilinear", "lanczos"):
        exp = np.asarray(Image.fromarray(img).resize((31, 23), PIL_FILTER[name]))
        (_, (bx, kx)), (_, (by, ky)) = _axis(G, name, 53, 31), _axis(G, name, 37, 23)
        assert np.array_equal(RR.resize(img, 23, 31, (bx, kx), (by, ky)), exp)
        wide = np.zeros((37, 31, 3), np.int64)
        for xo in range(31):
            wide[:, xo] = np.einsum("rkc,k->rc", img[:, bx[xo, 0]:bx[xo, 0] + bx[xo, 1]].astype(np.int64), kx[xo, :bx[xo, 1]])
        unrounded = np.zeros((23, 31, 3), np.int64)
        for yo in range(23):
            unrounded[yo] = np.einsum("kxc,k->xc", wide[by[yo, 0]:by[yo, 0] + by[yo, 1]], ky[yo, :by[yo, 1]])
        unrounded = np.clip((unrounded + (1 << 43)) >> 44, 0, 255)
        assert (unrounded != exp).mean() > 0.05
        v_first = RR.ops.resample_h(RR.ops.resample_v(img, 23, by, ky), 31, bx, kx)
        assert (v_first != exp).any()


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0][0]}x{p[0][1]}to{p[1][0]}x{p[1][1]}")
def test_nearest_tables_equal_pillow(G, pair):
    (h, w), (oh, ow) = pair
    rng = np.random.default_rng(h + w)
    img = rng.integers(0, 256, (h, w), np.uint8)
    exp = np.asarray(Image.fromarray(img).resize((ow, oh), Image.Resampling.NEAREST))
    xt, yt = G.nearest_table(w, ow), G.nearest_table(h, oh)
    assert xt.dtype == np.int32 and np.array_equal(xt, RR.nearest_table(w, ow)) and np.array_equal(yt, RR.nearest_table(h, oh))
    assert np.array_equal(img[yt][:, xt], exp) and np.array_equal(RR.nearest(img, oh, ow), exp)


def test_lanczos_plan_is_ipp_plan_lanczos_word_for_word(native, G):
    N, lib = native
    for n_in, n_out in [(53, 31), (37, 64), (97, 40), (300, 47), (7, 1), (2, 11), (1024, 640), (1000, 999), (5, 5)]:
        k0, a = G.lanczos_taps(n_in, n_out)
        k1, b = G.resample_taps("lanczos", n_in, n_out)
        assert k0 == k1 and a.dtype == b.dtype and np.array_equal(a, b), (n_in, n_out)
        assert lib.ipp_plan_resample(4, n_in, 0.0, float(n_in), n_out, None, 0) == \
            lib.ipp_plan_lanczos(n_in, 0.0, float(n_in), n_out, None, 0) == -len(a)
    # a sub-axis box, as the overlay path uses it
    buf0, buf1 = np.zeros(2 * 20 + 20 * 15, np.int32), np.zeros(2 * 20 + 20 * 15, np.int32)
    assert lib.ipp_plan_lanczos(90, 10.25, 50.5, 20, N.np_ptr(buf0), len(buf0)) == \
        lib.ipp_plan_resample(4, 90, 10.25, 50.5, 20, N.np_ptr(buf1), len(buf1)) == 15
    assert np.array_equal(buf0, buf1)


def test_plan_resample_refuses_and_sizes(native, G):
    N, lib = native
    buf = np.zeros(64, np.int32)
    f = lib.ipp_plan_resample
    assert f(5, 8, 0.0, 8.0, 4, None, 0) == N.IPP_E_ARG and f(-1, 8, 0.0, 8.0, 4, None, 0) == N.IPP_E_ARG
    assert f(1, 0, 0.0, 8.0, 4, None, 0) == N.IPP_E_ARG and f(1, 8, 0.0, 8.0, 0, None, 0) == N.IPP_E_ARG
    assert f(1, 8, 0.0, 8.0, 4, None, 0) == -(2 * 4 + 4 * 5)
    assert f(1, 8, 0.0, 8.0, 4, N.np_ptr(buf), 27) == N.IPP_E_ARG and f(1, 8, 0.0, 8.0, 4, N.np_ptr(buf), 28) == 5
    # ksize = 2·⌈support·max(in / out, 1)⌉ + 1
    for name, sup in (("box", 0.5), ("bilinear", 1.0), ("hamming", 1.0), ("bicubic", 2.0), ("lanczos", 3.0)):
        for n_in, n_out in ((1024, 640), (300, 47), (64, 129), (200, 33)):
            k, _ = G.resample_taps(name, n_in, n_out)
            assert k == 2 * int(np.ceil(sup * max(n_in / n_out, 1.0))) + 1
    assert G.resample_taps("lanczos", 1024, 256)[0] == 25 <= N.IPP_FEED_RESIZE_MAX_KSIZE
    assert G.resample_taps("lanczos", 300, 47)[0] == 41
    with pytest.raises(ValueError):
        G.resample_taps("nearest", 8, 4)


def test_feed_resize_entries_refuse_bad_arguments(native):
    """IPP_E_ARG before any launch: host addresses stand in for the device pointers, nothing dereferences them."""
    N, lib = native
    E = N.IPP_E_ARG
    mem = np.zeros(4096, np.uint8)
    p = (N.np_ptr(mem) + 15) & ~15
    K = N.IPP_FEED_RESIZE_MAX_KSIZE

    def rs(**kw):
        a = dict(inp=p, out=p + 256, lut=p + 512, tx=p + 1024, ty=p + 2048, S=1, W=8, H=8, ow=4, oh=4, kx=5, ky=5, es=2,
                 bgr=0)
        a.update(kw)
        return lib.ipp_scene_feed_resize(a["inp"], a["out"], a["lut"], a["tx"], a["ty"], a["S"], a["W"], a["H"], a["ow"],
                                         a["oh"], a["kx"], a["ky"], a["es"], a["bgr"], None)

    for kw in (dict(inp=None), dict(out=None), dict(lut=None), dict(tx=None), dict(ty=None), dict(S=0), dict(S=-1),
               dict(W=0), dict(H=0), dict(ow=0), dict(oh=-2), dict(es=1), dict(es=3), dict(es=8), dict(es=0), dict(bgr=2),
               dict(bgr=-1), dict(out=p + 257), dict(es=4, out=p + 258), dict(es=4, lut=p + 514), dict(tx=p + 1026),
               dict(ty=p + 2049), dict(kx=0), dict(ky=0), dict(kx=K + 1), dict(ky=K + 1), dict(W=1 << 14, H=1 << 14),
               dict(ow=1 << 14, oh=1 << 14), dict(S=(1 << 31) - 1)):
        assert rs(**kw) == E, kw

    def im(**kw):
        a = dict(m=p, mp=16, W=16, H=4, s=p + 256, S=1, K=8, xt=p + 512, yt=p + 1024, ow=8, oh=3, out=p + 2048, op=16)
        a.update(kw)
        return lib.ipp_scene_feed_index_map_sampled(a["m"], a["mp"], a["W"], a["H"], a["s"], a["S"], a["K"], a["xt"],
                                                    a["yt"], a["ow"], a["oh"], a["out"], a["op"], None)

    for kw in (dict(m=None), dict(s=None), dict(xt=None), dict(yt=None), dict(out=None), dict(S=0), dict(W=0), dict(H=0),
               dict(ow=0), dict(oh=0), dict(K=0), dict(K=9), dict(mp=15), dict(mp=1 << 31), dict(op=7), dict(op=24),
               dict(ow=17), dict(op=1 << 31), dict(out=p + 2056), dict(s=p + 258), dict(xt=p + 513), dict(yt=p + 1026),
               dict(H=1 << 17, mp=1 << 15), dict(oh=1 << 17, op=1 << 15), dict(S=(1 << 31) - 1)):
        assert im(**kw) == E, kw

    lds = lib.ipp_scene_feed_resize_lds
    for args in ((0, 8, 4, 4, 5, 5, 2), (8, 8, 4, 0, 5, 5, 2), (8, 8, 4, 4, 0, 5, 2), (8, 8, 4, 4, 5, K + 1, 2),
                 (8, 8, 4, 4, 5, 5, 3), (1 << 14, 1 << 14, 4, 4, 5, 5, 2)):
        assert lds(*args, None) == E, args


def test_lds_extents_fit_the_budget_for_every_admitted_ksize(native, G):
    """The extents come from the geometry alone; the workload's own geometry keeps the full tile, and no ksize up to
    the maximum, at the largest reduction that has it (BOX: in / out = ksize - 1), is left without a tile."""
    N, lib = native
    tile = (ctypes.c_int32 * 2)()
    budget = N.IPP_FEED_RESIZE_LDS_BYTES
    assert budget <= 80 * 1024
    for name in ("bilinear", "lanczos"):
        k, _ = G.resample_taps(name, 1024, 640)
        for es in (2, 4):
            n = lib.ipp_scene_feed_resize_lds(1024, 1024, 640, 640, k, k, es, tile)
            # three workgroups of the workload's own launch share a CU's 160 KiB
            assert 0 < 3 * n <= 160 * 1024 and tuple(tile) == (64, 32), (name, es, n, tuple(tile))
    for k in range(1, N.IPP_FEED_RESIZE_MAX_KSIZE + 1):
        red = max(k - 1, 1)
        for out in (1, 3, 70):
            n = lib.ipp_scene_feed_resize_lds(out * red, out * red, out, out, k, k, 4, tile)
            assert 0 < n <= budget and tile[0] >= 1 and tile[1] >= 1, (k, out, n)
        n = lib.ipp_scene_feed_resize_lds(16000, 16000, 70, 70, k, k, 4, tile)      # a reduction its ksize never has
        assert 0 < n <= budget, (k, n)
