"""The H launch (csrc/ipp_pipe.hip: k_pipe_hpass2) driven on its own: sources
and descriptors written by hand, tap tiles from the host tile builder, a plain
int64 restatement as the reference (tests/hpass_refs.py, whose tables
tests/test_hpass_refs_cpu.py holds to the oracle and to the paths they name).
No planner, no V launch: T is compared value by value, bit-exact.

In every launch here T is pre-filled with a poison byte and the source holds
seeded garbage in every byte outside the items' crop windows.  The three byte
classes of include/ipp.h: T rows [0, lines) × columns [0, out_len) must equal
the reference; the rows up to the band's 16 are written but unspecified and
ignored; every other byte of T — pitch padding, row groups past the last
band, the space between the items — must still hold the poison.  Each table
runs with two poisons and two garbage seeds, and ipp_pipe_status reads 0
after every launch.

  1  every table in one ipp_pipe_hpass launch (no background);
  2  three rows launched alone with descs advanced;
  3  the same tables through ipp_pipe_hpass_bgcopy: identical T;
  4  ipp_pipe_hpass_bgcopy_trim with a table: what it marks constant is 0x80
     in the reference and unstored in T;
  5  each of the 24 template forms (NR × zones × CN) on a two-item table;
  6  the refusals that must not launch.
"""
import time

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from image_processor_pipeline_amd import _native as N
from tests import hpass_refs as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RUNS = ((0x55, 7), (0xAA, 8))          # (poison, source garbage seed)
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
        self.src, self.coefs, self.descs = _dev(L.src), _dev(L.coefs), _dev(L.descs)
        assert self.coefs.data_ptr() % 16 == 0
        self.bg = self.dst = None

    def T(self, poison):
        t = torch.full((self.L.t_bytes,), poison, dtype=torch.uint8, device=DEV)
        assert t.data_ptr() % 16 == 0
        return t

    def background(self, poison):
        bg_bytes, dst_bytes = self.L.with_background()
        self.descs = _dev(self.L.descs)
        self.bg = _dev(np.random.default_rng(3).integers(0, 256, bg_bytes, np.uint8))
        self.dst = torch.full((dst_bytes,), poison, dtype=torch.uint8, device=DEV)
        assert (self.bg.data_ptr() | self.dst.data_ptr()) % 16 == 0

    def launch(self, lib, T, entry="hpass", first=0, n=None, max_rows=None, cn=None, params=None, tap=MFMA, trim=None):
        L = self.L
        n = len(L.cases) - first if n is None else n
        descs = self.descs.data_ptr() + first * N.PIPE_DESC.itemsize
        st = torch.cuda.current_stream(DEV).cuda_stream
        params = L.params if params is None else params
        args = (self.src.data_ptr(), T.data_ptr(), self.coefs.data_ptr(), descs, n, L.max_out_w,
                L.max_rows if max_rows is None else max_rows, L.cn if cn is None else cn, N.np_ptr(params), tap)
        if entry == "hpass":
            rc = lib.ipp_pipe_hpass(*args, st)
        elif entry == "bgcopy":
            rc = lib.ipp_pipe_hpass_bgcopy(*args, self.bg.data_ptr(), self.dst.data_ptr(), st)
        else:
            rc = lib.ipp_pipe_hpass_bgcopy_trim(*args, self.bg.data_ptr(), self.dst.data_ptr(),
                                                None if trim is None else trim.data_ptr(), st)
        torch.cuda.synchronize()
        status = np.full(1, -1, np.int32)
        assert lib.ipp_pipe_status(N.np_ptr(status), st) == N.IPP_OK
        assert status[0] == 0, "ipp_pipe_status %d" % status[0]
        return rc


_refs = {}


def _table_refs(table):
    """The references of a table's rows, computed once per module (they do not depend on poison or garbage)."""
    if table.name not in _refs:
        L = R.Launch(table)
        _refs[table.name] = [L.reference(i) for i in range(len(L.cases))]
    return _refs[table.name]


def _report(L, got, exp):
    """Names of the rows whose specified T differs, with the first differing
    (row, column, channel); and the poison-class bytes that changed."""
    lines = []
    for i, c in enumerate(L.cases):
        a, b = L.item_pixels(got, i), L.item_pixels(exp, i)
        bad = np.argwhere(a != b)
        if len(bad):
            r, x, ch = (int(v) for v in bad[0])
            lines.append("%s: %d values differ, first at (row %d, column %d, channel %d): got %d, want %d"
                         % (c.name, len(bad), r, x, ch, a[r, x, ch], b[r, x, ch]))
    return lines


def _compare(what, L, got, exp, check):
    bad = np.flatnonzero((got != exp) & check)
    rows = _report(L, got, exp)
    spec, unspec = L.classes()
    stray = np.flatnonzero((got != exp) & ~spec & ~unspec)
    print(what, "differing bytes:", len(bad), "of", int(check.sum()), "rows:", rows, "poison-class bytes changed:",
          len(stray), stray[:6].tolist())
    assert len(bad) == 0, (what, rows, "poison-class bytes changed: %d, first at %s" % (len(stray), stray[:6].tolist()))


def _run_table(lib, table, entry="hpass"):
    """One launch per (poison, garbage); returns the T buffers."""
    refs = _table_refs(table)
    out = []
    for poison, garbage in RUNS:
        L = R.Launch(table, garbage=garbage)
        d = Dev(L)
        if entry != "hpass":
            d.background(poison)
        T = d.T(poison)
        assert d.launch(lib, T, entry=entry) == N.IPP_OK
        got = T.cpu().numpy()
        spec, unspec = L.classes()
        _compare("%s %s %#x" % (table.name, entry, poison), L, got, L.expected(poison, refs), ~unspec)
        out.append((L, got, spec))
    (La, a, spec), (Lb, b, _) = out
    assert np.array_equal(a[spec], b[spec])
    return out


# --- 1: the tables, one launch each -------------------------------------------------------------------
@pytest.mark.parametrize("table", R.TABLES, ids=lambda t: t.name)
def test_table_one_launch(lib, table):
    t0 = time.time()
    out = _run_table(lib, table)
    names = [c.name for c in out[0][0].cases]
    if "prep0" in names:          # the prepared sampler and the block's own give the same T
        L, got, _ = out[0]
        assert np.array_equal(L.item_pixels(got, names.index("prep0")), L.item_pixels(got, names.index("prep1")))
    print("wall time %s: %.2f s" % (table.name, time.time() - t0))


# --- 2: items alone, descs advanced ---------------------------------------------------------------------
@pytest.mark.parametrize("name", R.ALONE)
def test_item_alone_with_descs_advanced(lib, name):
    t0 = time.time()
    refs = _table_refs(R.GEOMETRY)
    for poison, garbage in RUNS:
        L = R.Launch(R.GEOMETRY, garbage=garbage)
        i = [c.name for c in L.cases].index(name)
        d = Dev(L)
        T = d.T(poison)
        assert d.launch(lib, T, first=i, n=1) == N.IPP_OK
        _, unspec = L.classes()
        # the other items' T is untouched: their bytes are expected to hold the poison too
        own = np.zeros(L.t_bytes, bool)
        off, pitch, groups, _, _ = L.t_items[i]
        own[off: off + groups * pitch] = True
        _compare("alone %s %#x" % (name, poison), L, T.cpu().numpy(), L.expected(poison, refs, only=(i,)), ~(unspec & own))
    print("wall time alone %s: %.2f s" % (name, time.time() - t0))


# --- 3: with copy blocks -----------------------------------------------------------------------------------
@pytest.mark.parametrize("table", [R.GEOMETRY, R.GATHER, R.CN4], ids=lambda t: t.name)
def test_bgcopy_entry_writes_the_same_T(lib, table):
    t0 = time.time()
    with_bg = _run_table(lib, table, entry="bgcopy")
    plain = _run_table(lib, table)
    for (L, a, spec), (_, b, _) in zip(with_bg, plain):
        _, unspec = L.classes()
        assert np.array_equal(a[~unspec], b[~unspec])
    print("wall time bgcopy %s: %.2f s" % (table.name, time.time() - t0))


# --- 4: the trim table -------------------------------------------------------------------------------------
def _trim_launch(lib, table, poison, garbage):
    """(Launch, T bytes, table uint16 [n, bands]) after ipp_pipe_hpass_bgcopy_trim on poisoned T."""
    L = R.Launch(table, garbage=garbage)
    d = Dev(L)
    d.background(poison)
    T = d.T(poison)
    trim = torch.full((len(L.cases) * L.blocks_per_item(),), -1, dtype=torch.int16, device=DEV)
    assert d.launch(lib, T, entry="trim", trim=trim) == N.IPP_OK
    return L, T.cpu().numpy(), trim.cpu().numpy().view(np.uint16).reshape(len(L.cases), -1)


def _check_trim(what, L, got, table, refs, poison):
    """The groups the table marks constant are 0x80 in the reference and hold
    the poison in T; every other specified byte equals the reference; bands
    at or past the item's lines have no entry.  Returns the bytes left unstored."""
    exp = L.expected(poison, refs)
    spec, unspec = L.classes()
    const = np.zeros(L.t_bytes, bool)
    for i, c in enumerate(L.cases):
        lines, nt = L.t_items[i][4], (c.out_len + 15) >> 4
        nb = (lines + 15) // 16
        assert (table[i, nb:] == 0xFFFF).all(), (what, c.name, table[i].tolist())
        ev, cv = L.item_view(exp, i), L.item_view(const, i)
        for b in range(nb):
            lo, hi = int(table[i, b]) & 255, int(table[i, b]) >> 8
            assert lo <= min(hi, nt) and (hi <= nt or hi == 255), (what, c.name, b, lo, hi)
            for t in range(nt):
                if t < lo or (t >= hi and hi != 255):
                    px = refs[i][16 * b: 16 * b + 16, 16 * t: 16 * t + 16]
                    assert (px == 0).all(), "%s %s band %d tile %d is marked constant but the reference is not 0x80 there" \
                        % (what, c.name, b, t)
                    ev[4 * b: 4 * b + 4, 16 * t: 16 * t + 16] = poison
                    cv[4 * b: 4 * b + 4, 16 * t: 16 * t + 16] = True
    _compare(what, L, got, exp, ~unspec | const)
    return int(const.sum())


def test_trim_table_entry(lib):
    t0 = time.time()
    # the gather table: oblique items trim, the item beside its source sweeps nothing
    refs = _table_refs(R.GATHER)
    for poison, garbage in RUNS:
        L, got, table = _trim_launch(lib, R.GATHER, poison, garbage)
        elided = _check_trim("trim gather %#x" % poison, L, got, table, refs, poison)
        i = [c.name for c in L.cases].index("dead")
        assert (table[i, :1] == 0).all(), table[i].tolist()         # [lo, hi) = [0, 0): no tile is swept
        print("gather: bytes left unstored", elided, "table", table.tolist())
        assert elided > 0
    # rows that must not trim record (0, ntiles): black kept, and more than 64 tiles (stored as 255: no upper bound)
    for tab in (R.KEPT, R.GEOMETRY):
        refs = _table_refs(tab)
        for poison, garbage in RUNS:
            L, got, table = _trim_launch(lib, tab, poison, garbage)
            _check_trim("trim %s %#x" % (tab.name, poison), L, got, table, refs, poison)
            for i, c in enumerate(L.cases):
                nt, nb = (c.out_len + 15) >> 4, (L.t_items[i][4] + 15) // 16
                if tab is R.KEPT or nt > R.TRIM_MAX_TILES:
                    assert (table[i, :nb] == (min(nt, 255) << 8)).all(), (tab.name, c.name, table[i].tolist())
    print("wall time trim: %.2f s" % (time.time() - t0))


# --- 5: every template form ----------------------------------------------------------------------------------
@pytest.mark.parametrize("table", R.FORMS, ids=lambda t: t.name)
def test_every_template_form(lib, table):
    _run_table(lib, table)


# --- 6: refusals without a launch ----------------------------------------------------------------------------
def test_refusals_leave_T_alone(lib):
    L = R.Launch(R.CN4)
    d = Dev(L)
    d.background(0x55)
    for poison, _ in RUNS:
        T = d.T(poison)
        many = R.hsv_params(R.hsv_set(16))
        many["n_ranges"] = 17
        for entry in ("hpass", "bgcopy", "trim"):
            assert d.launch(lib, T, entry=entry, n=-1) == N.IPP_E_ARG
            assert d.launch(lib, T, entry=entry, cn=2) == N.IPP_E_ARG
            assert d.launch(lib, T, entry=entry, tap=0) == N.IPP_E_ARG
            assert d.launch(lib, T, entry=entry, tap=2) == N.IPP_E_ARG
            assert d.launch(lib, T, entry=entry, params=many) == N.IPP_E_ARG
            assert d.launch(lib, T, entry=entry, max_rows=0) == N.IPP_E_ARG
            assert (T == poison).all() and (d.dst == 0x55).all()
            assert d.launch(lib, T, entry=entry, n=0) == N.IPP_OK                 # no items: nothing to do
            assert (T == poison).all() and (d.dst == 0x55).all()
