"""The V launch (csrc/ipp_pipe_vblend.hip) driven on its own: T hand-made on
the host, tap tiles from the host tile builder, descriptors written by hand,
the oracle's int64 chain as the reference (tests/vblend_refs.py, whose tables
tests/test_vblend_refs_cpu.py holds to the paths they name).  No H launch, no
planner: every comparison is bit-exact.

In every launch here dst is pre-filled with a poison byte, T past the item's
rows and T's pitch padding hold seeded garbage, the bytes the launch owns
must equal the reference and every other byte of dst — pitch padding and the
gaps between the composites included — must still hold the poison.  Each
table runs with two poisons and two garbage seeds.

  1  the ragged table in one ipp_pipe_vblend_bands launch, and three of its
     items launched alone with descs advanced;
  2  the wide rows with max_ov_w = 976 (divisor table) and 992 (reciprocal);
  3  ipp_pipe_vblend_over in place, bg_off / bg_pitch wrong (but in bounds), two layers;
  4  a hand-made trim table through ipp_pipe_vblend_bands_trim;
  5  unpremultiply and clip over the whole (c, a) domain, both forms, three axes;
  6  the blend over the whole (bg, c, a) domain, groups and chunk path;
  7  the refusals that must not launch.
"""
import time

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from image_processor_pipeline_amd import _native as N
from oracle import ops
from tests import vblend_refs as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RUNS = ((0x55, 7), (0xAA, 8))          # (poison, garbage seed)
MFMA = N.IPP_TAPS_MFMA


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return N.load()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(DEV)


class Dev:
    """A Launch's buffers on the device."""

    def __init__(self, L):
        self.L = L
        self.T, self.coefs, self.bg = _dev(L.T), _dev(L.coefs), _dev(L.bg)
        self.descs = _dev(L.descs)
        assert (self.T.data_ptr() | self.bg.data_ptr() | self.coefs.data_ptr()) % 16 == 0     # the predicates assume it

    def dst(self, poison):
        t = torch.full((self.L.dst_bytes,), poison, dtype=torch.uint8, device=DEV)
        assert t.data_ptr() % 16 == 0
        return t

    def launch(self, lib, dst, entry="bands", first=0, n=None, bg_w=None, bg_h=None, max_ov_w=None, max_ov_h=None,
               trim=None, max_rows=0, T=None, bg=True):
        L = self.L
        n = len(L.cases) - first if n is None else n
        descs = self.descs.data_ptr() + first * N.PIPE_DESC.itemsize
        st = torch.cuda.current_stream(DEV).cuda_stream
        tmp = (self.T if T is None else T).data_ptr()
        geo = (n, bg_w or L.bg_w, bg_h or L.bg_h, max_ov_w or L.max_ov_w, max_ov_h or L.max_ov_h, MFMA)
        bgp = self.bg.data_ptr() if bg else None
        if entry == "bands":
            rc = lib.ipp_pipe_vblend_bands(tmp, bgp, dst.data_ptr(), self.coefs.data_ptr(), descs, *geo, st)
        elif entry == "trim":
            rc = lib.ipp_pipe_vblend_bands_trim(tmp, bgp, dst.data_ptr(), self.coefs.data_ptr(), descs, *geo,
                                                None if trim is None else trim.data_ptr(), max_rows, st)
        else:
            rc = lib.ipp_pipe_vblend_over(tmp, dst.data_ptr(), self.coefs.data_ptr(), descs, *geo, st)
        torch.cuda.synchronize()
        return rc


def _compare(what, got, exp):
    bad = np.flatnonzero(got != exp)
    print(what, "differing bytes:", len(bad), "of", exp.size, "first at", bad[:6].tolist())
    assert len(bad) == 0, (what, len(bad), bad[:6].tolist())


_refs = {}


def _table_refs(name, table, seed=1):
    """The references of a table's rows, computed once per module (they do not depend on poison or garbage)."""
    if name not in _refs:
        L = R.Launch(table, seed=seed)
        _refs[name] = [L.reference(i) for i in range(len(L.cases))]
    return _refs[name]


def _row_errors(L, got, exp):
    """Names of the rows whose composites differ (for the message)."""
    return [c.name for i, c in enumerate(L.cases) if not np.array_equal(L.bg_rows(got, i), L.bg_rows(exp, i))]


# --- 1: the ragged table ------------------------------------------------------------------------
def test_ragged_table_one_launch(lib):
    refs = _table_refs("ragged", R.RAGGED)
    owned = []
    for poison, garbage in RUNS:
        L = R.Launch(R.RAGGED, garbage=garbage)
        assert L.blocks() % 8 != 0 and R.magic_form(L.max_ov_w)
        d = Dev(L)
        dst = d.dst(poison)
        assert d.launch(lib, dst) == N.IPP_OK
        got = dst.cpu().numpy()
        exp, own = L.expected(poison, refs)
        print("rows that differ:", _row_errors(L, got, exp))
        _compare("ragged %#x" % poison, got, exp)
        owned.append(got[own])
    assert np.array_equal(owned[0], owned[1])


@pytest.mark.parametrize("name", R.RAGGED_ALONE)
def test_ragged_item_alone_with_descs_advanced(lib, name):
    refs = _table_refs("ragged", R.RAGGED)
    owned = []
    for poison, garbage in RUNS:
        L = R.Launch(R.RAGGED, garbage=garbage)
        i = [c.name for c in L.cases].index(name)
        d = Dev(L)
        dst = d.dst(poison)
        assert d.launch(lib, dst, first=i, n=1) == N.IPP_OK
        full, own = L.expected(poison, refs)
        exp = np.full_like(full, poison)
        L.bg_rows(exp, i)[...] = L.bg_rows(full, i)
        got = dst.cpu().numpy()
        _compare("alone %s %#x" % (name, poison), got, exp)
        owned.append(L.bg_rows(got, i)[L.bg_rows(own, i)])
    assert np.array_equal(owned[0], owned[1])


# --- 2: both unpremultiply forms ---------------------------------------------------------------------
W992 = R.row("w_992", 992, 6, 6, 992, 16, 0, 10, "the widest overlay of all, identity axis: the reciprocal form only", ident=1)


def test_both_unpremultiply_forms(lib):
    table = R.ragged_wide_subset()
    refs = _table_refs("wide", table)
    for poison, garbage in RUNS:
        L = R.Launch(table, garbage=garbage)
        assert L.max_ov_w <= R.MAGIC_MAX_OV_W and max(c.bg_w for c in table) == 992
        # every K-step form runs under both unpremultiply forms
        assert {R.k_form(nk) for nks in L.nks for nk in nks} == {"db1", "db2", "hoist3", "loop"}
        d = Dev(L)
        exp, own = L.expected(poison, refs)
        out = []
        for max_ov_w in (R.MAGIC_MAX_OV_W, R.MAX_OV_W):
            dst = d.dst(poison)
            assert d.launch(lib, dst, bg_w=992, max_ov_w=max_ov_w) == N.IPP_OK
            out.append(dst.cpu().numpy())
            print("rows that differ:", _row_errors(L, out[-1], exp))
            _compare("max_ov_w %d %#x" % (max_ov_w, poison), out[-1], exp)
        assert R.magic_form(R.MAGIC_MAX_OV_W) and not R.magic_form(R.MAX_OV_W)
        assert np.array_equal(out[0], out[1])
    # and an overlay only the reciprocal form takes
    owned = []
    for poison, garbage in RUNS:
        L = R.Launch(table + [W992], garbage=garbage)
        d = Dev(L)
        dst = d.dst(poison)
        assert L.max_ov_w == 992 and d.launch(lib, dst) == N.IPP_OK
        got = dst.cpu().numpy()
        exp, own = L.expected(poison, refs + [L.reference(len(table))])
        _compare("w_992 %#x" % poison, got, exp)
        owned.append(got[own])
    assert np.array_equal(owned[0], owned[1])


# --- 3: in place -----------------------------------------------------------------------------------
def test_in_place_two_layers(lib):
    for poison, garbage in RUNS:
        L1, L2 = R.Launch(R.RAGGED, seed=1, garbage=garbage), R.Launch(R.RAGGED, seed=2, garbage=garbage + 10)
        assert np.array_equal(L1.coefs, L2.coefs) and len(L1.T) == len(L2.T)
        # bg_off and bg_pitch are nonsense the in-place form must not read.  Wrong but in bounds: a launch
        # that did read them would read the start of dst (misaligned, rows 3 bytes apart: at most
        # 1 + 3·bg_h + 3·bg_w + 48 bytes from its base) and fail the comparison, not fault
        for L in (L1, L2):
            L.descs["p"]["bg_off"] = 1
            L.descs["p"]["bg_pitch"] = 3
        assert 1 + 3 * L1.bg_h + 3 * L1.bg_w + 48 < L1.dst_bytes
        d = Dev(L1)
        host = np.full(L1.dst_bytes, poison, np.uint8)
        exp1, exp2 = host.copy(), host.copy()
        for i, c in enumerate(L1.cases):
            L1.bg_rows(host, i)[:, :3 * c.bg_w] = L1.bgs[i].reshape(c.bg_h, -1)
            one, _ = L1.reference(i, inplace=True)
            two, _ = L1.reference(i, M=L2.Ms[i], bg=one, inplace=True)
            L1.bg_rows(exp1, i)[:, :3 * c.bg_w] = one.reshape(c.bg_h, -1)
            L1.bg_rows(exp2, i)[:, :3 * c.bg_w] = two.reshape(c.bg_h, -1)
        dst = _dev(host)
        assert d.launch(lib, dst, entry="over") == N.IPP_OK
        got = dst.cpu().numpy()
        print("rows that differ:", _row_errors(L1, got, exp1))
        _compare("layer 1 %#x" % poison, got, exp1)
        assert d.launch(lib, dst, entry="over", T=_dev(L2.T)) == N.IPP_OK
        got = dst.cpu().numpy()
        print("rows that differ:", _row_errors(L1, got, exp2))
        _compare("layer 2 %#x" % poison, got, exp2)
        assert not np.array_equal(exp1, exp2)


# --- 4: a hand-made trim table ------------------------------------------------------------------------
def test_hand_made_trim_table(lib):
    base = R.Launch(R.TRIM_CASES)
    entries = [R.trim_entries(c, k) for k, c in enumerate(base.cases)]
    max_rows = max(c.in_len for c in base.cases)
    stride = (max_rows + 15) // 16
    table = np.full((len(base.cases), stride), 0xFFFF, np.uint16)        # bands past an item's lines: no entry
    for k, ent in enumerate(entries):
        table[k, :len(ent)] = [lo | hi << 8 for lo, hi in ent]
    assert (table[:, :2] & 255).max() > 0 and stride == 18
    for poison, garbage in RUNS:
        # T holds the poison in the groups the table marks constant
        held = [R.trim_M(c, M, ent, poison ^ 0x80) for c, M, ent in zip(base.cases, base.Ms, entries)]
        L = R.Launch(R.TRIM_CASES, Ms=held, garbage=garbage)
        for c, ent, (t_off, t_pitch, _) in zip(L.cases, entries, L.t_spans):
            lo, hi = ent[0]
            grp = L.T[t_off: t_off + 16]                  # band 0, column 0 lies in tile 0 < lo
            assert lo > 0 and (grp == poison).all()
        d = Dev(L)
        trimmed = [L.reference(i, M=R.trim_M(c, base.Ms[i], entries[i], 0)) for i, c in enumerate(L.cases)]
        full = [L.reference(i) for i in range(len(L.cases))]
        assert any(not np.array_equal(a[0], b[0]) for a, b in zip(trimmed, full))
        dst = d.dst(poison)
        assert d.launch(lib, dst, entry="trim", trim=_dev(table), max_rows=max_rows) == N.IPP_OK
        got, exp = dst.cpu().numpy(), L.expected(poison, trimmed)[0]
        print("rows that differ:", _row_errors(L, got, exp))
        _compare("trim table %#x" % poison, got, exp)
        # a null table on the same T: nothing is constant, the poison is read as pixels
        dst = d.dst(poison)
        assert d.launch(lib, dst, entry="trim", trim=None, max_rows=0) == N.IPP_OK
        _compare("null table %#x" % poison, dst.cpu().numpy(), L.expected(poison, full)[0])
        # a sub-range takes the table advanced with the descriptors
        dst = d.dst(poison)
        assert d.launch(lib, dst, entry="trim", first=3, n=2, trim=_dev(table[3:]), max_rows=max_rows) == N.IPP_OK
        sub = np.full_like(exp, poison)
        for i in (3, 4):
            L.bg_rows(sub, i)[...] = L.bg_rows(exp, i)
        _compare("trim table rows 3.. %#x" % poison, dst.cpu().numpy(), sub)


# --- 5: unpremultiply and clip over the whole domain -----------------------------------------------------
VALUE_AXES = {"identity": (256, 1), "one_to_one": (256, 0), "times_two": (128, 0)}


@pytest.mark.parametrize("axis", list(VALUE_AXES))
@pytest.mark.parametrize("form", ["table", "reciprocal"])
def test_values_unpremultiply_and_clip(lib, axis, form):
    rows, ident = VALUE_AXES[axis]
    bg_w, x, max_ov_w = (256, 0, 256) if form == "table" else (992, 367, 992)
    assert R.magic_form(max_ov_w) == (form == "table")
    case = R.row("vt_" + axis, 256, rows, 256, bg_w, 256, x, 0, "every (c, a)", ident=ident)
    M = R.value_table(rows)
    # the reference itself clamps: rgba2rgbA's min(255, ·) in every colour channel, and on the × 2 axis
    # clip8 below 0 and above 255 in each of the four channels
    assert all(R.unpremultiply_clamps(R.v_resample(M, rows, 256, ident)))
    if axis == "times_two":
        lo, hi = R.v_sums_range(M, 128, 256)
        assert max(lo) < 0 and min(hi) > 255, (lo, hi)
    key = ("values", axis, form)
    owned = []
    for poison, garbage in RUNS:
        L = R.Launch([case], Ms=[M], garbage=garbage)
        if key not in _refs:
            _refs[key] = [L.reference(0)]
        d = Dev(L)
        dst = d.dst(poison)
        assert d.launch(lib, dst, max_ov_w=max_ov_w) == N.IPP_OK
        got = dst.cpu().numpy()
        exp, own = L.expected(poison, _refs[key])
        _compare("values %s %s %#x" % (axis, form, poison), got, exp)
        owned.append(got[own])
    assert np.array_equal(owned[0], owned[1])


# --- 6: the blend over the whole domain ------------------------------------------------------------------
_regions = {}


def _value_ref(i, bg_w):
    """Item i's composite: the paste is computed once per item on the overlay's
    256 × 256 region, which holds the same background bytes at every bg_w."""
    c = R.value_case(i, bg_w)
    bg = R.value_bg(i, bg_w)
    if "ov" not in _regions:
        _regions["ov"] = R.v_overlay(R.value_table(), 256, 256, 1)
    if i not in _regions:
        _regions[i] = ops.paste_rgba_onto_rgb(np.ascontiguousarray(bg[:, c.x:c.x + 256]), _regions["ov"], 0, 0)
    out = bg.copy()
    out[:, c.x:c.x + 256] = _regions[i]
    return out


@pytest.mark.parametrize("bg_w", [288, 271])
def test_values_blend_every_bg_colour_alpha(lib, bg_w):
    t0 = time.time()
    M = R.value_table()
    for first in range(0, 256, 64):
        items = range(first, first + 64)
        cases = [R.value_case(i, bg_w) for i in items]
        bgs = [R.value_bg(i, bg_w) for i in items]
        refs, owned = None, []
        for poison, garbage in RUNS:
            L = R.Launch(cases, Ms=[M] * 64, bgs=bgs, garbage=garbage, shared_t=True)
            assert all(p["groups"] == (bg_w == 288) for p in L.paths) and len(L.T) == len(R.Launch(cases[:1], Ms=[M]).T)
            if refs is None:
                refs = [(_value_ref(i, bg_w), R.owned_mask(bg_w, 256, c.x, 0, 256, 256, p))
                        for i, c, p in zip(items, cases, L.paths)]
                if first == 0 and bg_w == 271:      # the shared region reference is the oracle's paste of the whole composite
                    assert np.array_equal(refs[5][0], L.reference(5)[0])
            d = Dev(L)
            dst = d.dst(poison)
            assert d.launch(lib, dst) == N.IPP_OK
            got = dst.cpu().numpy()
            exp, own = L.expected(poison, refs)
            bad = _row_errors(L, got, exp)
            print("items that differ:", bad[:8], len(bad))
            _compare("blend bg_w %d items %d.. %#x" % (bg_w, first, poison), got, exp)
            owned.append(got[own])
        assert np.array_equal(owned[0], owned[1])
    print("wall time of the whole-domain blend, bg_w %d: %.1f s" % (bg_w, time.time() - t0))


# --- 7: refusals without a launch ------------------------------------------------------------------------
def test_refusals_leave_dst_alone(lib):
    L = R.Launch(R.RAGGED[:3])
    d = Dev(L)
    for poison, _ in RUNS:
        _refusals(lib, d, d.dst(poison), poison)


def _refusals(lib, d, dst, poison):
    tab = _dev(np.zeros((3, 8), np.uint16))
    assert d.launch(lib, dst, bg_w=160, max_ov_w=161) == N.IPP_E_ARG              # max_ov_w > bg_w
    assert d.launch(lib, dst, bg_w=1000, max_ov_w=993) == N.IPP_E_ARG             # max_ov_w > IPP_PIPE_MAX_OV_W
    assert d.launch(lib, dst, bg=False) == N.IPP_E_ARG                            # a null bg on the bands entries
    assert d.launch(lib, dst, entry="trim", bg=False) == N.IPP_E_ARG
    assert d.launch(lib, dst, entry="trim", bg=False, trim=tab, max_rows=128) == N.IPP_E_ARG
    for max_rows in (0, -1):
        assert d.launch(lib, dst, entry="trim", trim=tab, max_rows=max_rows) == N.IPP_E_ARG
    assert (dst == poison).all()
    for entry in ("bands", "trim", "over"):
        assert d.launch(lib, dst, entry=entry, n=0) == N.IPP_OK                   # no items: nothing to do
    assert (dst == poison).all()
