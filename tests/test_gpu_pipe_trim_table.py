"""The H launch's trim table (ipp_pipe_hpass_bgcopy_trim, ipp_pipe_layout.h):
with a table the H launch records each band's swept tiles [lo, hi) and does
not store the constant T groups of the others, and the V launch and the box
launch, given the same table, do not load them.

  composites   PipeRunner.run on T and output poisoned with 0x55, then with
               0xAA: both results equal the CPU oracle bit for bit (a reader
               that loads an unstored group cannot pass both);
  elision      after the H launch alone on poisoned T: the table equals the
               host restatement (hpass_trim.item_bounds), every group it marks
               constant still holds the poison, and every byte of the items'
               T rows equals the null-table launch's;
  labels       overlay_bboxes after a table-driven H launch on poisoned T
               equal the boxes of the old entry points on a T written in full;
  null table   the three *_trim entry points with a null table write the
               bytes the old entry points write;
  sub-ranges   run_overlapped and launches over descriptor ranges equal run.

The geometries are those of tests/test_gpu_pipe_fill_trim.py (restated there
as CASES, imported here) and one 980-px overlay for the V launch's form
without the divisor table (max_ov_w in 977..992).
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import pipe as opipe
from tests.test_gpu_pipe_fill_trim import CASES as TRIM_CASES

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
POISONS = (0x55, 0xAA)

CASES = dict(TRIM_CASES)
# a 980-px overlay (62 tiles) up-scaled from a 400-px strip at 12°: k_pipe_vblend_mfma<false>
CASES["wide_no_magic"] = ((30, 400), (320, 1120), (0, 0, 0, 0), [(12.0, "o", 0.876)], {})
UNTRIMMED = ("no_black_range", "zones")


@pytest.fixture(scope="module")
def fused():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from image_processor_pipeline_amd import fused as F
    return F


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class Case:
    """Plan, inputs and (on first use) the oracle's composites of one case."""

    def __init__(self, fused, name):
        src_hw, bg_hw, margins, items, extra = CASES[name]
        self.name = name
        self.cfg = fused.PipeConfig(margins=margins, **extra)
        params = [fused.ItemParams(a, s, k % 2, r, 1 + k, 2 + k) for k, (a, s, r) in enumerate(items)]
        self.plan = fused.plan_pipe(src_hw, len(params), bg_hw, 2, self.cfg, params=params)
        self.n = len(self.plan.descs)
        (H, W), (self.bh, self.bw) = src_hw, bg_hw
        rng = np.random.default_rng(len(name) + 17 * self.n)
        self.src = rng.integers(0, 256, (self.n, H, W, 3), np.uint8)
        self.src[:, H // 3: H // 2, W // 4: W // 2] = 0        # real black inside the source, beside the fill
        self.bgs = rng.integers(0, 256, (2, self.bh, self.bw, 3), np.uint8)
        self.dsrc, self.dbgs = _t(self.src), _t(self.bgs)
        self._exp = None

    @property
    def exp(self):
        if self._exp is None:
            self._exp = [opipe.pipe_item(self.src[i], self.bgs, self.plan.params[i], self.cfg) for i in range(self.n)]
        return self._exp

    def out(self, fill):
        return torch.full((self.n, self.bh, self.bw, 3), fill, dtype=torch.uint8, device=DEV)

    def bounds(self):
        """[(lo, hi)] per band of every descriptor, as the H launch writes them."""
        from image_processor_pipeline_amd import hpass_trim as HT
        on = HT.trim_enabled(self.plan.hsv)
        assert on == (self.name not in UNTRIMMED), self.name
        return [[(lo, hi) if on else (0, nt) for lo, hi, nt in HT.item_bounds(self.plan, i)] for i in range(self.n)]


_cases = {}


@pytest.fixture
def case(fused, request):
    name = request.param
    if name not in _cases:
        _cases[name] = Case(fused, name)
    return _cases[name]


def _all(names=None):
    return pytest.mark.parametrize("case", list(names or CASES), indirect=True)


def _old_hpass(c, runner, tmp, out):
    from image_processor_pipeline_amd import _native as N
    from image_processor_pipeline_amd.device import _stream
    p = c.plan
    N.check(runner.lib.ipp_pipe_hpass_bgcopy(c.dsrc.data_ptr(), tmp.data_ptr(), runner.coefs.data_ptr(),
                                             runner.descs.data_ptr(), c.n, p.max_out_w, p.max_rows, 3,
                                             N.np_ptr(p.hsv), p.tap_format, c.dbgs.data_ptr(), out.data_ptr(),
                                             _stream(runner.device)), "ipp_pipe_hpass_bgcopy")


def _item_rows(plan, nbytes):
    """Mask over the scratch: the bytes of every item's T rows [0, lines).  (The rows a band holds past
    the item's end are the H body's to fill with whatever its window held: they differ from run to run,
    and no tap reaches them.)"""
    m = np.zeros(nbytes, bool)
    for d in plan.descs:
        h = d["h"]
        w, pitch, off, lines = int(h["out_len"]), int(h["dst_pitch"]), int(h["dst_off"]), int(h["lines"])
        item = m[off: off + (lines + 3) // 4 * pitch].reshape(-1, w, 4, 4)                   # [g][x][c][r]
        item[...] = (4 * np.arange(item.shape[0])[:, None] + np.arange(4)[None, :] < lines)[:, None, None, :]
    return m


def _old_boxes(c, runner, tmp, alpha_min):
    from image_processor_pipeline_amd import _native as N
    from image_processor_pipeline_amd.device import _stream
    p = c.plan
    bbox = torch.empty(4 * c.n, dtype=torch.int32, device=DEV)
    N.check(runner.lib.ipp_pipe_overlay_bbox(tmp.data_ptr(), runner.coefs.data_ptr(), runner.descs.data_ptr(), c.n,
                                             p.max_ov_w, p.max_ov_h, alpha_min, p.tap_format, bbox.data_ptr(),
                                             _stream(runner.device)), "ipp_pipe_overlay_bbox")
    return bbox.cpu().numpy().reshape(-1, 4)


# --- 1: composites on T poisoned two ways ---------------------------------------------------
@_all()
def test_composites_vs_oracle_on_t_poisoned_two_ways(fused, case):
    c = case
    if c.name == "wide_no_magic":
        assert 977 <= c.plan.max_ov_w <= 992
        assert any(lo > 0 or hi < 62 for lo, hi in c.bounds()[0])
    runner = fused.PipeRunner(c.plan, DEV)
    for poison in POISONS:
        runner.tmp.fill_(poison)
        out = c.out(poison)
        runner.run(c.dsrc, c.dbgs, out)
        got = out.cpu().numpy()
        assert runner.status() == 0
        for i in range(c.n):
            bad = int((got[i] != c.exp[i]).sum())
            print(c.name, hex(poison), "item", i, "differing bytes", bad)
            assert bad == 0, (c.name, hex(poison), i, bad)


# --- 2: the elision really happens ------------------------------------------------------------
@_all()
def test_h_launch_leaves_constant_groups_unstored(fused, case):
    c, poison = case, POISONS[0]
    p = c.plan
    runner = fused.PipeRunner(p, DEV)
    full = torch.full_like(runner.tmp, poison)
    _old_hpass(c, runner, full, c.out(poison))
    runner.tmp.fill_(poison)
    runner.trim.fill_(-1)
    runner.hpass_bgcopy(c.dsrc, c.dbgs, c.out(poison))
    assert runner.status() == 0
    table = runner.trim.cpu().numpy().view(np.uint16)
    sparse, full = runner.tmp.cpu().numpy(), full.cpu().numpy()
    assert table.shape == (c.n, (p.max_rows + 15) // 16)

    # compared: every byte of the items' T rows [0, lines) and every byte of the unstored groups
    exp, check = full.copy(), _item_rows(p, full.size)
    elided = 0
    for i, bands in enumerate(c.bounds()):
        h = p.descs[i]["h"]
        w, pitch, off = int(h["out_len"]), int(h["dst_pitch"]), int(h["dst_off"])
        nt = (w + 15) >> 4
        assert pitch == 16 * w and len(bands) == (int(h["lines"]) + 15) // 16
        want = [lo | hi << 8 for lo, hi in bands]
        assert table[i, :len(bands)].tolist() == want, (c.name, i, table[i].tolist(), want)
        assert (table[i, len(bands):] == 0xFFFF).all(), (c.name, i)           # bands past the item's lines: no entry
        for b, (lo, hi) in enumerate(bands):
            band = slice(off + 4 * b * pitch, off + 4 * (b + 1) * pitch)                   # the band's four group rows
            rows, crows = exp[band].reshape(4, w, 16), check[band].reshape(4, w, 16)
            for t in [*range(lo), *range(hi, nt)]:
                g = rows[:, 16 * t: 16 * t + 16]
                assert (g == 0x80).all(), (c.name, i, b, t)                    # what the old launch stored there
                g[...] = poison
                crows[:, 16 * t: 16 * t + 16] = True
                elided += g.size
    print(c.name, "bytes left unstored:", elided)
    if c.name in UNTRIMMED + ("square_angles", "one_band"):
        assert elided == 0, (c.name, elided)
    elif c.name != "near_axis_wide":
        assert elided > 0, c.name
    bad = np.flatnonzero((sparse != exp) & check)
    print(c.name, "differing bytes:", len(bad), "of", int(check.sum()), "first at", bad[:8].tolist(),
          "outside the compared bytes:", int(((sparse != exp) & ~check).sum()))
    assert len(bad) == 0, (c.name, len(bad))


# --- 3: labels ---------------------------------------------------------------------------------
@_all(["oblique", "thin", "flips", "downscale", "one_row_tail", "zones"])
def test_boxes_with_the_table_equal_boxes_on_a_full_t(fused, case):
    c, poison = case, POISONS[0]
    runner = fused.PipeRunner(c.plan, DEV)
    full = torch.full_like(runner.tmp, poison)
    _old_hpass(c, runner, full, c.out(poison))
    runner.tmp.fill_(poison)
    runner.hpass_bgcopy(c.dsrc, c.dbgs, c.out(poison))
    for alpha_min in (1, 128, 255):
        want = _old_boxes(c, runner, full, alpha_min)
        got = runner._launch_bboxes(alpha_min, 0, c.n).cpu().numpy().reshape(-1, 4)      # descriptor order
        assert np.array_equal(got, want), (c.name, alpha_min, got.tolist(), want.tolist())
        assert alpha_min > 1 or (want[:, 0] >= 0).all()      # every overlay is visible (alpha 255 need not occur)
        # and through the public call: the same rows in item order
        by_item = runner.overlay_bboxes(alpha_min)
        assert np.array_equal(by_item[c.plan.order], want), (c.name, alpha_min)


# --- 4: the null table -------------------------------------------------------------------------
@_all(["oblique", "downscale", "one_row_tail", "no_black_range", "wide_no_magic"])
def test_null_table_is_the_old_entry_points(fused, case):
    from image_processor_pipeline_amd import _native as N
    from image_processor_pipeline_amd.device import _stream
    c, poison = case, POISONS[1]
    p = c.plan
    runner = fused.PipeRunner(p, DEV)
    lib, st = runner.lib, _stream(runner.device)
    coefs, descs = runner.coefs.data_ptr(), runner.descs.data_ptr()

    t_old, o_old = torch.full_like(runner.tmp, poison), c.out(poison)
    _old_hpass(c, runner, t_old, o_old)
    b_old = _old_boxes(c, runner, t_old, 128)
    N.check(lib.ipp_pipe_vblend_bands(t_old.data_ptr(), c.dbgs.data_ptr(), o_old.data_ptr(), coefs, descs, c.n,
                                      p.bg_w, p.bg_h, p.max_ov_w, p.max_ov_h, p.tap_format, st),
            "ipp_pipe_vblend_bands")

    t_new, o_new = torch.full_like(runner.tmp, poison), c.out(poison)
    N.check(lib.ipp_pipe_hpass_bgcopy_trim(c.dsrc.data_ptr(), t_new.data_ptr(), coefs, descs, c.n, p.max_out_w,
                                           p.max_rows, 3, N.np_ptr(p.hsv), p.tap_format, c.dbgs.data_ptr(),
                                           o_new.data_ptr(), None, st), "ipp_pipe_hpass_bgcopy_trim")
    bbox = torch.empty(4 * c.n, dtype=torch.int32, device=DEV)
    N.check(lib.ipp_pipe_overlay_bbox_trim(t_new.data_ptr(), coefs, descs, c.n, p.max_ov_w, p.max_ov_h, 128,
                                           p.tap_format, bbox.data_ptr(), None, 0, st), "ipp_pipe_overlay_bbox_trim")
    N.check(lib.ipp_pipe_vblend_bands_trim(t_new.data_ptr(), c.dbgs.data_ptr(), o_new.data_ptr(), coefs, descs, c.n,
                                           p.bg_w, p.bg_h, p.max_ov_w, p.max_ov_h, p.tap_format, None, 0, st),
            "ipp_pipe_vblend_bands_trim")
    assert runner.status() == 0
    rows = _item_rows(p, t_old.numel())
    assert np.array_equal(t_new.cpu().numpy()[rows], t_old.cpu().numpy()[rows])
    assert np.array_equal(bbox.cpu().numpy().reshape(-1, 4), b_old)
    assert torch.equal(o_new, o_old)
    got = o_new.cpu().numpy()
    for i in range(c.n):
        assert np.array_equal(got[i], c.exp[i]), (c.name, i)
    # a table without its stride is refused
    assert lib.ipp_pipe_vblend_bands_trim(t_new.data_ptr(), c.dbgs.data_ptr(), o_new.data_ptr(), coefs, descs, c.n,
                                          p.bg_w, p.bg_h, p.max_ov_w, p.max_ov_h, p.tap_format,
                                          runner.trim.data_ptr(), 0, st) == N.IPP_E_ARG
    assert lib.ipp_pipe_overlay_bbox_trim(t_new.data_ptr(), coefs, descs, c.n, p.max_ov_w, p.max_ov_h, 128,
                                          p.tap_format, bbox.data_ptr(), runner.trim.data_ptr(), 0, st) == N.IPP_E_ARG
    torch.cuda.synchronize()


# --- 5: sub-ranges -------------------------------------------------------------------------------
@_all(["oblique"])
def test_run_overlapped_and_descriptor_ranges_equal_run(fused, case):
    c = case
    assert c.n == 3
    runner = fused.PipeRunner(c.plan, DEV)
    ref = c.out(7)
    runner.run(c.dsrc, c.dbgs, ref)
    assert all(np.array_equal(ref[i].cpu().numpy(), c.exp[i]) for i in range(c.n))
    runner.tmp.fill_(POISONS[0])
    out = c.out(9)
    runner.run_overlapped(c.dsrc, c.dbgs, out, 2)
    torch.cuda.synchronize()
    assert torch.equal(out, ref)
    # the table's rows advance with the descriptors: ranges (1, 2) and (0, 1), boxes of a range
    runner.tmp.fill_(POISONS[1])
    runner.trim.fill_(-1)
    out = c.out(5)
    for items in ((1, 2), (0, 1)):
        runner.hpass_bgcopy(c.dsrc, c.dbgs, out, items=items)
    full_boxes = runner.overlay_bboxes(128)
    assert np.array_equal(runner.overlay_bboxes(128, items=(1, 2)), full_boxes[np.sort(c.plan.order[1:3])])
    for items in ((0, 1), (1, 2)):
        runner.vblend_bands(c.dbgs, out, items=items)
    assert torch.equal(out, ref)


def test_run_overlapped_two_copy_groups_equals_run(fused):
    """Ten items: run_overlapped's two ranges are descriptors [0, 8) and [8, 10)."""
    items = [(10.0 + 33.0 * k, "ohv"[k % 3] if k % 3 < 2 else "hv", 0.3 + 0.02 * k) for k in range(10)]
    cfg = fused.PipeConfig(margins=(0, 0, 0, 0))
    params = [fused.ItemParams(a, s, k % 2, r, 1 + k, 2 + k) for k, (a, s, r) in enumerate(items)]
    plan = fused.plan_pipe((150, 190), 10, (256, 320), 2, cfg, params=params)
    assert fused.overlap_bounds(10, 2) == [0, 8, 10]
    rng = np.random.default_rng(3)
    src, bgs = _t(rng.integers(0, 256, (10, 150, 190, 3), np.uint8)), _t(rng.integers(0, 256, (2, 256, 320, 3), np.uint8))
    runner = fused.PipeRunner(plan, DEV)
    ref = torch.full((10, 256, 320, 3), 7, dtype=torch.uint8, device=DEV)
    runner.run(src, bgs, ref)
    runner.tmp.fill_(POISONS[0])
    out = torch.full_like(ref, 9)
    runner.run_overlapped(src, bgs, out, 2)
    torch.cuda.synchronize()
    assert runner.status() == 0
    assert torch.equal(out, ref)
