"""CPU: the direct H-launch harness of tests/hpass_refs.py before any GPU sees
it: the reference against the oracle, the claims of every row of the tables,
and the byte classes of T.

M against the oracle's own chain (oracle.ops: to_rgba, rotate_expand_nearest,
the bbox sub-rectangle, flip, hsv_alpha_mask, premultiply), row by row:

  every row of every table whose map is a rotation and whose bbox lies inside
  the rotated canvas — all rows but the three below — is compared on ALL of its
  M rows [line0, line0 + lines) × columns [0, in_len): `line0` windows and
  bboxes are sub-rectangles of the oracle's canvas, zones are taken on the
  bbox-cropped image, as the reference's chain takes them after its crop;
  `dead`, `k_dead`   the bbox lies beside the canvas, out of the oracle's reach:
                     held to cutout_scalar (a second, straight-line scalar
                     restatement) at every pixel;
  `wrap`             a hand-made map (every source column twice), no rotation
                     of the oracle's: held to cutout_scalar at every pixel,
                     and to np.repeat of the oracle's masked source.

Besides, every row is held to cutout_scalar on a sparse sample of its pixels,
and hpass_ref followed by vblend_refs.v_resample is held to the oracle's full
RGBA LANCZOS resize of M on four rows.
"""
import numpy as np
import pytest

from oracle import ops
from tests import hpass_refs as R
from tests import vblend_refs as VR

ALL = R.TABLES + R.FORMS
SCALAR_ONLY = ("dead", "k_dead", "wrap")
SYM = {0: "o", 1: "h", 2: "v", 3: "hv"}

_launches = {}


def launch(table, garbage=7):
    if (table.name, garbage) not in _launches:
        _launches[table.name, garbage] = R.Launch(table, garbage=garbage)
    return _launches[table.name, garbage]


def oracle_M(L, i):
    """Rows [line0, line0 + lines) of the oracle's premultiplied cut-out of row i."""
    c, d = L.cases[i], L.descs[i]
    (x0, y0, w, h), _, (off_x, off_y, out_w, out_h), (nw, nh) = R.geometry(c)
    assert c.A is None and 0 <= off_x and off_x + out_w <= nw and 0 <= off_y and off_y + out_h <= nh
    g = d["g"]
    pitch = int(g["src_pitch"])
    img = np.lib.stride_tricks.as_strided(L.src[int(g["src_off"]):], (c.src[1], pitch), (pitch, 1))
    crop = img[y0:y0 + h, x0 * L.cn:(x0 + w) * L.cn].reshape(h, w, L.cn)
    rot = ops.rotate_expand_nearest(ops.to_rgba(crop), c.angle)
    assert rot.shape[:2] == (nh, nw)
    fl = ops.flip(rot[off_y:off_y + out_h, off_x:off_x + out_w], SYM[c.flip])
    alpha = ops.hsv_alpha_mask(fl[..., [2, 1, 0]], L.hsv.ranges, L.hsv.zones)
    M = ops.premultiply(np.concatenate([fl[..., :3], alpha[..., None]], -1))
    line0, lines = int(d["h"]["line0"]), int(d["h"]["lines"])
    return M[line0:line0 + lines]


@pytest.mark.parametrize("table", ALL, ids=lambda t: t.name)
def test_M_equals_the_oracle_chain(table):
    L = launch(table)
    for i, c in enumerate(L.cases):
        M = L.M(i)
        d = L.descs[i]
        lines, in_len, line0 = int(d["h"]["lines"]), int(d["h"]["in_len"]), int(d["h"]["line0"])
        assert M.shape == (lines, in_len, 4)
        # premultiplied as it stands: alpha 0 or 255, colour 0 under alpha 0
        assert set(np.unique(M[..., 3])) <= {0, 255} and (M[M[..., 3] == 0] == 0).all()
        if c.name in SCALAR_ONLY:
            want = np.array([[R.cutout_scalar(d["g"], L.hsv, L.src, x, line0 + r) for x in range(in_len)]
                             for r in range(lines)], np.uint8)
            assert np.array_equal(M, want), c.name
        else:
            assert np.array_equal(M, oracle_M(L, i)), (table.name, c.name)
            rng = np.random.default_rng(i)
            for r, x in zip(rng.integers(0, lines, 24), rng.integers(0, in_len, 24)):
                assert tuple(M[r, x]) == R.cutout_scalar(d["g"], L.hsv, L.src, int(x), line0 + int(r)), (c.name, r, x)


def test_hand_made_map_doubles_the_oracles_columns():
    L = launch(R.GEOMETRY)
    i = [c.name for c in L.cases].index("wrap")
    c = L.cases[i]
    g = L.descs[i]["g"]
    pitch = int(g["src_pitch"])
    img = np.lib.stride_tricks.as_strided(L.src[int(g["src_off"]):], (c.src[1], pitch), (pitch, 1))[:, :3 * c.src[0]]
    rgb = img.reshape(c.src[1], c.src[0], 3)
    alpha = ops.hsv_alpha_mask(rgb[..., ::-1], L.hsv.ranges, None)
    masked = ops.premultiply(np.concatenate([rgb, alpha[..., None]], -1))
    assert np.array_equal(L.M(i), np.repeat(masked, 2, axis=1))


def test_reference_does_not_depend_on_the_garbage():
    for table in (R.GATHER, R.CN4):
        A, B = launch(table, 7), launch(table, 8)
        assert not np.array_equal(A.src, B.src)
        for i in range(len(A.cases)):
            assert np.array_equal(A.M(i), B.M(i)), A.cases[i].name
        # the two sources agree in the crop windows and nowhere else (garbage: one byte in 256 agrees by chance)
        assert np.array_equal(A.window, B.window) and np.array_equal(A.src[A.window], B.src[A.window])
        out = ~A.window
        assert out.sum() > 1000 and (A.src[out] != B.src[out]).mean() > 0.98


@pytest.mark.parametrize("table,name,ov_h", [(R.GATHER, "obl_a", 20), (R.GATHER, "palette", 9), (R.GATHER, "stripes", 4),
                                             (R.GEOMETRY, "o33_l33", 12)])
def test_h_then_v_reference_equals_the_oracles_resize(table, name, ov_h):
    L = launch(table)
    i = [c.name for c in L.cases].index(name)
    h = L.descs[i]["h"]
    lines, in_len, out_len = int(h["lines"]), int(h["in_len"]), int(h["out_len"])
    assert int(h["line0"]) == 0 and lines == int(L.descs[i]["g"]["out_h"]) and in_len != out_len and lines != ov_h
    M = L.M(i)
    assert np.array_equal(ops.premultiply(M), M)
    got = ops.unpremultiply(VR.v_resample(R.hpass_ref(M, in_len, out_len), lines, ov_h, 0))
    assert np.array_equal(got, ops.resize_lanczos_rgba(M, out_len, ov_h))


def test_h_reference_equals_the_oracles_h_pass():
    """hpass_ref's taps come from geometry.resample_taps; the oracle computes its own."""
    L = launch(R.GEOMETRY)
    for name in ("nk8", "ck3", "up_in2", "o17_l17"):
        i = [c.name for c in L.cases].index(name)
        h = L.descs[i]["h"]
        in_len, out_len = int(h["in_len"]), int(h["out_len"])
        _, bounds, kk = ops.precompute_coeffs(in_len, 0.0, float(in_len), out_len)
        assert np.array_equal(L.reference(i), ops.resample_h(L.M(i), out_len, bounds, kk)), name


def problems(tables=ALL):
    bad, met = [], set()
    for table in tables:
        L = launch(table)
        for i, c in enumerate(L.cases):
            have = L.tags(i)
            mine = set(R.CLAIMS[c.name].split()) | set(R.TABLE_CLAIMS.get(table.name, "").split())
            mine |= set(R.TABLE_ROW_CLAIMS.get((table.name, c.name), "").split())
            if not mine <= have:
                bad.append(("false claim", table.name, c.name, sorted(mine - have)))
            if not c.why:
                bad.append(("no why", c.name))
            met |= mine
    return bad + [("not met", t) for t in R.REQUIRED if t not in met]


def test_every_claim_of_every_row_holds():
    assert problems() == []
    # the 24 template forms, each on the two FORM_ROWS
    forms = {(R.nr_form(len(t.hsv.ranges)), R.has_zones(t.hsv), t.cn) for t in R.FORMS}
    assert forms == {(nr, z, cn) for nr in (1, 2, 3, 4, 6, 16) for z in (False, True) for cn in (3, 4)}
    assert all(len(launch(t).cases) == 2 for t in R.FORMS)
    # sizes: sources of at most about 900 × 80, launches of at most about 20 items
    for t in ALL:
        assert len(t.rows) <= 20 and all(c.src[0] <= 900 and c.src[1] <= 80 for c in t.rows), t.name
    assert set(R.ALONE) <= {c.name for c in R.GEOMETRY.rows}


def test_claims_fail_without_their_rows():
    """Dropping a table makes the property test fail: the claims are not vacuous."""
    for drop in (R.GEOMETRY, R.GATHER, R.KEPT, R.CN4, R.Z7):
        assert problems([t for t in ALL if t is not drop]) != [], drop.name


def test_chunk_rule_by_hand():
    # (K0, nK): 4 tiles of one K step 16 apart fit; then the ring stops the prefix at 3, at 2, at 1
    hdr = np.array([[0, 1, 0, 0], [16, 1, 0, 0], [32, 1, 0, 0], [48, 1, 0, 0],
                    [64, 4, 0, 0], [160, 4, 0, 0], [256, 4, 0, 0], [352, 4, 0, 0],       # ends 320, 416, 512, 608: 3 fit
                    [448, 8, 0, 0], [480, 8, 0, 0]], np.int64)                            # 512 wide each: alone
    ck = R.chunks(hdr, 0, len(hdr))
    assert [(k["s0"], k["s1"]) for k in ck] == [(0, 4), (4, 7), (7, 8), (8, 9), (9, 10)]
    assert [k["ring_stop"] for k in ck] == [0, 608 - 64, 960 - 352, 992 - 448, 0]
    assert [k["overlap"] for k in ck] == [False, True, True, True, True]
    assert ck[2]["c0"] == 512 and ck[1]["c0"] == 112          # filled = 112 > W0 = 64
    assert R.chunks(hdr, 1, 3) == [dict(s0=1, s1=3, W0=16, W1=96, c0=16, overlap=False, ring_stop=0)]


def test_body_form_by_hand():
    g = np.zeros((), R.N.GATHER_DESC)
    g["src_pitch"], g["src_cn"], g["src_h"], g["in_w"], g["in_h"] = 36, 3, 10, 12, 10
    f = R.body_form(g)                                   # the whole dense source: the last dword crosses its end
    assert (f["need"], f["nrec"], f["clamps"], f["fast"]) == (361, 360, True, False)
    g["in_y0"], g["in_h"] = 2, 5                         # full width, rows inside: in_h·pitch = need - 1
    f = R.body_form(g)
    assert (f["need"], f["nrec"], f["yr"], f["fast"]) == (181, 288, False, False)
    g["in_x0"], g["in_w"] = 1, 10                        # narrower: row in_h starts past the records
    assert R.body_form(g)["fast"]


@pytest.mark.parametrize("table", [R.GEOMETRY, R.GATHER, R.CN4], ids=lambda t: t.name)
def test_byte_classes_partition_T(table):
    L = launch(table)
    spec, unspec = L.classes()
    assert spec.shape == (L.t_bytes,) and not (spec & unspec).any()
    lines = [int(d["h"]["lines"]) for d in L.descs]
    assert int(spec.sum()) == sum(4 * n * c.out_len for n, c in zip(lines, L.cases))
    assert int(unspec.sum()) == sum(4 * ((n + 15) // 16 * 16 - n) * c.out_len for n, c in zip(lines, L.cases))
    poison = ~(spec | unspec)
    # the poison class holds the pitch padding, the row groups past the written ones and the gaps between the items
    end = 0
    for (off, pitch, groups, alloc, n), c in zip(L.t_items, L.cases):
        assert off % 16 == 0 and off >= end + 16 and alloc > groups == 4 * ((n + 15) // 16)
        assert poison[end:off].all() and poison[off + groups * pitch: off + alloc * pitch].all()
        rows = poison[off: off + groups * pitch].reshape(groups, pitch)
        assert rows[:, 16 * c.out_len:].all() and not rows[:, :16 * c.out_len].any()
        end = off + alloc * pitch
    assert end <= L.t_bytes and poison[end:].all()
    # expected(): the references in the specified bytes, the poison in its class
    refs = [L.reference(i) for i in range(len(L.cases))]
    a, b = L.expected(0x55, refs), L.expected(0xAA, refs)
    assert (a[poison] == 0x55).all() and (b[poison] == 0xAA).all() and np.array_equal(a[spec], b[spec])
    for i in range(len(L.cases)):
        assert np.array_equal(L.item_pixels(a, i), refs[i])


def test_value_rows_reach_both_ends_of_clip8():
    L = launch(R.GATHER)
    i = [c.name for c in L.cases].index("stripes")
    lo, hi = R.sums_range(L, i)
    assert max(lo) < 0 and min(hi) > 255, (lo, hi)          # every channel, alpha included, both ways
    ref = L.reference(i)
    assert (ref == 0).any() and (ref == 255).any()
    # the clamp row: the source's last pixel is kept and its three bytes and its neighbour's last differ
    j = [c.name for c in L.cases].index("clamp")
    M = L.M(j)
    assert tuple(M[-1, -1]) == (19, 163, 251, 255) and tuple(M[-1, -2]) == (77, 130, 230, 255)
    # black kept (and a source of kept colours, or none in reach): T's alpha is 255 everywhere, the fill's included
    K = launch(R.KEPT)
    assert [c.name for c in K.cases[:2]] == ["k_obl", "k_dead"]
    for k in (0, 1):
        assert (K.reference(k)[..., 3] == 255).all()
    assert (K.reference(1) == (0, 0, 0, 255)).all()
