"""GPU: keep-largest (csrc/ipp_ccl.hip) on the branches the mask-content tests
of test_gpu_parity.py do not reach, against tests/ccl_refs.py.

Every comparison is ``np.array_equal`` on the WHOLE image after the call: α
zeroed outside the kept component and unchanged inside it, BGR identical
everywhere, and the returned bbox equal to the reference's.  The tie rule is
the project's restatement (UNPINNED: OpenCV is absent); test_ccl_refs_cpu.py
shows, from the reference alone, that each case has the property it is here for.
(The whole image matters: the 10×12 tie image of test_gpu_parity.py crops to
the same 1×1 pixel whichever of its two components is kept, so a tie rule
turned round passes there and fails here.)

  1. test_designed_case        open/closed ties in both root orders, open/open
                               after cross-tile merges, the largest closed key
  2. test_entry_counts         counts[image] read back through the C ABI: equal to
                               the reference's open components per tile, ≤ ent_cap
  3. test_closed_limit_4096, test_all_open_4097x4099, test_all_open_fused_chain
                               exactly 2^23 slots (closed path, root at the top of
                               the 23-bit field) and the first sizes past it
  4. test_ragged_batch_one_launch, test_packed_gaps_untouched
  5. test_fuzz                 256 seeded images, 64 a launch
  6. test_pitched_rows         pitch ≠ 4·w and unaligned offsets through the C ABI
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import ops
from tests import ccl_refs as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"

_KEEP = np.array([220, 140, 40], np.uint8)        # as in test_gpu_parity.py: kept colour (blue-ish)
_DROP = np.array([24, 18, 30], np.uint8)          # excluded (dark)


@pytest.fixture(scope="module")
def C():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from image_processor_pipeline_amd import device_ccl
    return device_ccl


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _same(got, exp, tag):
    got = np.asarray(got)
    assert got.shape == exp.shape, (tag, got.shape, exp.shape)
    assert np.array_equal(got, exp), (tag, int((got != exp).sum()), "bytes differ")


def _check_batch(C, imgs, tag):
    """keep_largest_masks on the list in one launch; every whole image and bbox against the reference."""
    dev = [_t(im) for im in imgs]
    bbs = C.keep_largest_masks(dev)
    for i, (im, d, bb) in enumerate(zip(imgs, dev, bbs)):
        full, ebb = R.keep_largest_full(im)
        _same(d.cpu().numpy(), full, (tag, i, im.shape))
        assert bb == ebb, (tag, i, im.shape, bb, ebb)


def _run_abi(C, buf, descs, dims):
    """ipp_ccl_keep_largest on a device byte buffer with the caller's
    descriptors.  Returns (counts, bbox rows, the scratch layout)."""
    from image_processor_pipeline_amd import _native as N
    from image_processor_pipeline_amd.device import _stream, _to_dev
    n = len(dims)
    sc = C.CclScratch([(int(h), int(w)) for h, w in dims], buf.device)
    dd = _to_dev(descs, buf.device)
    N.check(N.load().ipp_ccl_keep_largest(buf.data_ptr(), dd.data_ptr(), n, max(w for _, w in dims),
                                          max(h for h, _ in dims), sc.works_dev.data_ptr(), sc.scratch.data_ptr(),
                                          sc.max_ent, sc.counts.data_ptr(), sc.stats.data_ptr(), sc.bbox.data_ptr(),
                                          _stream(buf.device)), "ipp_ccl_keep_largest")
    counts = sc.counts.cpu().numpy()
    return counts, sc.bbox.cpu().numpy().reshape(n, 4), sc.works


def _pack(imgs, gap, fill):
    """Images one after the other with `gap` bytes of `fill` after each."""
    from image_processor_pipeline_amd import _native as N
    offs, off = [], 0
    for im in imgs:
        offs.append(off)
        off += im.size + gap
    buf = np.full(off, fill, np.uint8)
    d = np.zeros(len(imgs), N.IMAGE_DESC)
    for i, (im, o) in enumerate(zip(imgs, offs)):
        buf[o:o + im.size] = im.reshape(-1)
        h, w = im.shape[:2]
        d[i]["off"], d[i]["w"], d[i]["h"], d[i]["pitch"], d[i]["cn"] = o, w, h, 4 * w, 4
    return buf, offs, d


# --------------------------------------------------------------------------- 1. designed cases

@pytest.mark.parametrize("case", R.designed_cases(), ids=lambda c: c.name)
def test_designed_case(C, case):
    im = R.image_from_mask(case.mask, np.random.default_rng(len(case.name)))
    _check_batch(C, [im], case.name)


# --------------------------------------------------------------------------- 2. entry counts

def test_entry_counts(C):
    """counts[image] (the entries k_ccl_label emitted) against the reference's
    open components summed per tile, and against the capacity the layout gave:
    124 per tile for the ring patterns (the bound is 126, the capacity 128),
    63 for the even grid."""
    masks = [c.mask for c in R.designed_cases() if c.name.startswith("ring")] + [R.even_grid_mask()]
    rng = np.random.default_rng(2)
    imgs = [R.image_from_mask(m, rng) for m in masks]
    buf, offs, d = _pack(imgs, 0, 0)
    dbuf = _t(buf)
    counts, bbox, works = _run_abi(C, dbuf, d, [m.shape for m in masks])
    got = dbuf.cpu().numpy()
    for i, (m, im) in enumerate(zip(masks, imgs)):
        exp = R.expected_entries(m)
        print("entries", m.shape, "counts", int(counts[i]), "reference", exp, "ent_cap", int(works[i]["ent_cap"]))
        assert int(works[i]["ent_cap"]) == R.n_tiles(*m.shape) * 128
        assert counts[i] <= works[i]["ent_cap"], i
        assert counts[i] == exp, i
        full, ebb = R.keep_largest_full(im)
        _same(got[offs[i]:offs[i] + im.size].reshape(im.shape), full, ("entries", i))
        assert tuple(int(v) for v in bbox[i]) == ebb, i
    assert int(counts[0]) == 124 * 9


# --------------------------------------------------------------------------- 3. the 2^23-slot threshold

def _big(C, case, per_tile):
    m = case.mask
    h, w = m.shape
    im = R.image_from_mask(m, np.random.default_rng(h))
    comps = R.components(m)
    full, ebb = R.keep_largest_full(im, comps)
    buf, offs, d = _pack([im], 0, 0)
    dbuf = _t(buf)
    counts, bbox, works = _run_abi(C, dbuf, d, [(h, w)])
    exp = R.expected_entries(m)
    print(case.name, "slots", R.slots(h, w), "ent_cap", int(works[0]["ent_cap"]), "counts", int(counts[0]),
          "reference entries", exp, "winner root", int(comps.root[comps.best]), "bbox", tuple(bbox[0]))
    assert int(works[0]["ent_cap"]) == R.n_tiles(h, w) * per_tile
    assert counts[0] <= works[0]["ent_cap"] and counts[0] == exp
    assert tuple(int(v) for v in bbox[0]) == ebb
    _same(dbuf.cpu().numpy().reshape(im.shape), full, case.name)


def test_closed_limit_4096(C):
    """4096×4096, exactly 2^23 run-start slots: the last image on the closed
    path.  The kept closed component's root is 2^23 - 56 (the key's 23-bit
    field ~G holds 55); the runner-up has one pixel less and a smaller root."""
    _big(C, R.big_closed_limit(), 128)


def test_all_open_4097x4099(C):
    """The first sizes past 2^23 slots (8 400 900): every component gets an
    entry, ent_cap = tiles·1024, tile_in_word looks every root up through P.
    Kept: an interior 3×51 bar with root ≥ 2^23 that wins a tie by its
    smaller root (ccl_refs.big_all_open)."""
    _big(C, R.big_all_open(), 1024)


def test_all_open_fused_chain(C):
    """The same 4097×4099 content through the fused chain (HSV mask of two
    flat colours): k_ccl_inwords and k_ccl_crop_rows in all-open mode (65
    tile columns, the crop inside the 32nd)."""
    from image_processor_pipeline_amd import geometry as G
    from image_processor_pipeline_amd.video_chain import VideoChain
    case = R.big_all_open()
    h, w = case.mask.shape
    fr = np.where(case.mask[..., None], _KEEP, _DROP).astype(np.uint8)
    bgra = ops.color_mask_bgra(fr, G.REFERENCE_HSV_RANGES)
    assert np.array_equal(bgra[..., 3] > 1, case.mask)
    exp = ops.keep_largest_component(bgra)
    chain = VideoChain(1, h, w, DEV)
    chain.out.fill_(7)
    chain.run(_t(fr[None]))
    res = chain.results()
    counts = int(chain.sc.counts.cpu()[0])
    print("fused all-open: counts", counts, "ent_cap", int(chain.sc.works[0]["ent_cap"]), "crop", exp.shape)
    assert counts == R.expected_entries(case.mask) <= int(chain.sc.works[0]["ent_cap"])
    assert tuple(int(v) for v in chain.bbox.cpu()[:4]) == (1990, 4092, 2041, 4095)
    assert res[0] is not None
    _same(res[0], exp, "fused all-open")


# --------------------------------------------------------------------------- 4. ragged batches

def _ragged_images():
    rng = np.random.default_rng(44)
    one = np.array([[[9, 8, 7, 200]]], np.uint8)
    faint = rng.integers(0, 256, (37, 70, 4), np.uint8)
    faint[..., 3] = rng.integers(0, 2, (37, 70))           # no α > 1, some α = 1
    clear = rng.integers(0, 256, (64, 65, 4), np.uint8)
    clear[..., 3] = 0
    imgs = [one, faint, clear]
    imgs += [R.image_from_mask(m, rng) for m in R.ccl_stress_masks(np.random.default_rng(31))]
    imgs += [R.image_from_mask(c.mask, rng) for c in R.designed_cases()]
    imgs.append(R.image_from_mask(rng.random((257, 389)) < 0.45, rng))
    return imgs


def test_ragged_batch_one_launch(C):
    """One launch over images of every size: the grid comes from the largest
    width and height (two different images), smaller images' waves return
    early, scratch is addressed per image.  Then the same list reversed."""
    imgs = _ragged_images()
    assert imgs[0].shape == (1, 1, 4) and imgs[-1].shape == (257, 389, 4)
    assert max(im.shape[0] for im in imgs) == 300 and max(im.shape[1] for im in imgs) == 389
    _check_batch(C, imgs, "ragged")
    _check_batch(C, imgs[::-1], "ragged reversed")


def test_packed_gaps_untouched(C):
    """keep_largest_packed on the ragged list with 256 poisoned bytes after
    every image: images equal the reference, the gaps keep their bytes."""
    imgs = _ragged_images()
    buf, offs, _ = _pack(imgs, 256, 0xC3)
    exp = buf.copy()
    ebbs = []
    for im, o in zip(imgs, offs):
        full, ebb = R.keep_largest_full(im)
        exp[o:o + im.size] = full.reshape(-1)
        ebbs.append(ebb)
    dbuf = _t(buf)
    bbs = C.keep_largest_packed(dbuf, offs, [im.shape[:2] for im in imgs])
    _same(dbuf.cpu().numpy(), exp, "packed with gaps")
    assert bbs == ebbs


# --------------------------------------------------------------------------- 5. fuzz

def test_fuzz(C):
    masks = R.fuzz_masks()
    assert len(masks) == 256
    rng = np.random.default_rng(R.FUZZ_SEED)
    ties = sum(1 for m in masks if R.components(m).tied > 1)
    print("fuzz images decided by the tie rule:", ties)
    assert ties >= 10
    for k in range(0, len(masks), 64):
        _check_batch(C, [R.image_from_mask(m, rng) for m in masks[k:k + 64]], "fuzz %d" % k)


# --------------------------------------------------------------------------- 6. pitched rows

@pytest.mark.parametrize("extra", [12, 64])
@pytest.mark.parametrize("w", [63, 64, 65, 130])
def test_pitched_rows(C, w, extra):
    """ipp_ccl_keep_largest with pitch = 4·w + extra and offsets that are no
    multiple of 16, two images a launch in a buffer of 0xA5: pixels equal the
    reference, every padding and gap byte is unchanged."""
    from image_processor_pipeline_amd import _native as N
    rng = np.random.default_rng(1000 * w + extra)
    pitch = 4 * w + extra
    dims = [(70, w), (129, w)]
    second = 20 + 70 * pitch + 36
    offs = [20, second + (4 if second % 16 == 0 else 0)]
    size = offs[1] + 129 * pitch + 64
    assert all(o % 16 for o in offs)
    buf = np.full(size, 0xA5, np.uint8)
    exp = buf.copy()
    d = np.zeros(2, N.IMAGE_DESC)
    ebbs = []
    for i, ((h, _), o) in enumerate(zip(dims, offs)):
        im = R.image_from_mask(rng.random((h, w)) < (0.35, 0.5)[i], rng)
        full, ebb = R.keep_largest_full(im)
        ebbs.append(ebb)
        for b, a in ((buf, im), (exp, full)):
            np.lib.stride_tricks.as_strided(b[o:], (h, w, 4), (pitch, 4, 1))[...] = a
        d[i]["off"], d[i]["w"], d[i]["h"], d[i]["pitch"], d[i]["cn"] = o, w, h, pitch, 4
    dbuf = _t(buf)
    counts, bbox, works = _run_abi(C, dbuf, d, dims)
    _same(dbuf.cpu().numpy(), exp, ("pitched", w, extra))
    assert [tuple(int(v) for v in r) for r in bbox] == ebbs
