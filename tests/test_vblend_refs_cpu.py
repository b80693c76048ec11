"""CPU: the direct V-launch harness of tests/vblend_refs.py before any GPU
sees it — the T packing against the layout sentence of
csrc/ipp_pipe_layout.h, ``vblend_ref`` against live Pillow (a resize that
keeps the width runs Pillow's V pass alone), and the properties the case
tables claim: which K-step form, phase-2 layout, paste position and value
every row is there for.  They are asserted, not assumed, so a table edited
later cannot lose a path silently; dropping any row of the ragged table fails
``test_ragged_table_properties``.
"""
import numpy as np
import pytest
from PIL import Image

from oracle import ops
from tests import vblend_refs as R

LANCZOS = Image.Resampling.LANCZOS


# --------------------------------------------------------------------------- T

@pytest.mark.parametrize("rows,w,pad", [(1, 1, 0), (7, 5, 2), (16, 16, 0), (37, 33, 1)])
def test_pack_unpack_round_trip(rows, w, pad):
    rng = np.random.default_rng(rows)
    M = rng.integers(0, 256, (rows, w, 4), np.uint8)
    pitch, t_rows = 16 * (w + pad), 4 * R.t_groups(rows, 2)
    fill = rng.integers(0, 256, t_rows // 4 * pitch, np.uint8)
    T = R.pack_t(M, pitch, t_rows, fill)
    assert T.shape == (t_rows // 4 * pitch,)
    assert np.array_equal(R.unpack_t(T, rows, w, pitch), M)
    # nothing but M's bytes changed: rows past M and the pitch padding keep the filler
    T0 = R.pack_t(np.zeros_like(M), pitch, t_rows, fill)
    same = R.pack_t(np.full_like(M, 255), pitch, t_rows, fill) == T0
    assert int((~same).sum()) == M.size and np.array_equal(T[same], fill[same])
    assert (R.pack_t(M, pitch, t_rows, 0x33)[same] == 0x33).all()


def test_one_group_by_hand():
    """ipp_pipe_layout.h: "[row group g][column x'][4 channels][4 rows] bytes,
    values XOR 0x80 — one 16-B group per (g, x') at base + g·pitch + 16·x',
    channel c = dword c (alpha = dword 3)"."""
    rows, w, pitch = 11, 6, 16 * 9
    M = np.random.default_rng(0).integers(0, 256, (rows, w, 4), np.uint8)
    T = R.pack_t(M, pitch, 4 * R.t_groups(rows, 1), 0xEE)
    g, x = 1, 4
    grp = T[g * pitch + 16 * x: g * pitch + 16 * x + 16]
    for c in range(4):
        for r in range(4):
            assert grp[4 * c + r] == M[4 * g + r, x, c] ^ 0x80
    # rows 8..10 of group 2 are M's, row 11 is past it
    grp = T[2 * pitch + 16 * x: 2 * pitch + 16 * x + 16].reshape(4, 4)
    assert np.array_equal(grp[:, :3], (M[8:11, x, :] ^ 0x80).T) and (grp[:, 3] == 0xEE).all()
    assert R.t_groups(11, 1) == (16 + 64 + 16) // 4


# --------------------------------------------------------------------------- the reference against Pillow

# heights: downscales of about 2.5, 4, 7, 10, 14 and one upscale; y & 15 in {0, 1, 15}
@pytest.mark.parametrize("in_h,out_h,y", [(50, 20, 16), (80, 20, 1), (133, 19, 15), (200, 20, 31), (280, 20, 0),
                                          (9, 23, 17)])
def test_reference_equals_pillow(in_h, out_h, y):
    w, x, bg_w, bg_h = 37, 5, 64, 64
    rng = np.random.default_rng(in_h)
    img = rng.integers(0, 256, (in_h, w, 4), np.uint8)
    img[: in_h // 3, : w // 2, 3] = 0
    img[in_h // 2:, w // 3:, 3] = 255
    bg = rng.integers(0, 256, (bg_h, bg_w, 3), np.uint8)
    assert len(np.unique(img[..., 3])) > 100
    ov = Image.fromarray(img).resize((w, out_h), LANCZOS)
    want = Image.fromarray(bg).copy()
    want.paste(ov, (x, y), ov)
    path = R.paths(bg_w, bg_h, 3 * bg_w, 3 * bg_w, 0, 0, x, w)
    got, own = R.vblend_ref(ops.premultiply(img), in_h, out_h, 0, bg, x, y, path)
    assert np.array_equal(got, np.asarray(want))
    # the owned bytes hold every byte the paste changed
    changed = (got != bg).reshape(bg_h, -1)
    assert changed.any() and not (changed & ~own).any()


def test_identity_axis_reference_takes_the_rows_as_they_are():
    M = R.case_M(R.RAGGED[2], 3)
    c = R.RAGGED[2]
    assert c.ident and c.in_len == c.ov_h
    assert np.array_equal(R.v_overlay(M, c.in_len, c.ov_h, 1), ops.unpremultiply(M))
    # noise reaches rgba2rgbA's clamp: 255·c // a > 255 somewhere
    a = M[..., 3].astype(np.int64)
    assert ((a > 0) & (a < 255) & (M[..., 0] > a)).any()


# --------------------------------------------------------------------------- path predicates

def test_path_predicates():
    assert [R.k_form(k) for k in (1, 2, 3, 4, 5, 8)] == ["db1", "db2", "hoist3", "loop", "loop", "loop"]
    assert R.magic_form(976) and not R.magic_form(977) and not R.magic_form(992)
    assert R.paste_bands(33, 30, 96) == (32, 64) and R.paste_bands(75, 18, 93) == (64, 93)
    assert R.paste_max_bands(1) == 1 and R.paste_max_bands(2) == 2 and R.paste_max_bands(18) == 3
    p = R.paths(160, 96, 480, 480, 0, 0, 17, 65)
    assert p["groups"] and p["csplit"] and (p["gx0"], p["gx1"], p["G"]) == (1, 6, 5)
    p = R.paths(160, 96, 496, 512, 0, 0, 17, 65)
    assert p["groups"] and not p["csplit"] and p["G"] == 10
    assert not R.paths(159, 96, 477, 477, 0, 0, 17, 65)["groups"]
    assert not R.paths(160, 96, 480, 480, 8, 0, 17, 65)["groups"]
    assert not R.paths(160, 96, 480, 480, 0, 4, 17, 65)["groups"]
    # in place the background's offset and pitch do not count
    assert R.paths(160, 96, 7, 480, 3, 0, 17, 65, inplace=True)["csplit"]


# --------------------------------------------------------------------------- the tables

def ragged_table_problems(table):
    """What the ragged table `table` fails to meet (an empty list: all is met)."""
    L = R.Launch(table)
    bad = []
    claims = {}
    for c, path, nks in zip(L.cases, L.paths, L.nks):
        have = R.case_tags(c, path, nks)
        mine = set(R.RAGGED_CLAIMS[c.name].split())
        if not mine <= have:
            bad.append(("false claim", c.name, sorted(mine - have)))
        claims[c.name] = mine
    met = set().union(*claims.values())
    bad += [("not met", t) for t in R.RAGGED_REQUIRED if t not in met]
    for name, mine in claims.items():
        others = set().union(*(m for n, m in claims.items() if n != name))
        if not mine - others:
            bad.append(("dead row", name))
    nks = {nk for ks in L.nks for nk in ks}
    if not ({1, 2, 3, 4} <= nks and max(nks) >= 5):
        bad.append(("nK", sorted(nks)))
    n = len(table)
    if not 20 <= n <= 40:
        bad.append(("descriptors", n))
    if L.blocks() % 8 == 0:
        bad.append(("blocks mod 8", L.blocks()))
    return bad


def test_ragged_table_properties():
    assert ragged_table_problems(R.RAGGED) == []
    L = R.Launch(R.RAGGED)
    # most blocks leave early: max_ov_h gives every item more bands than most have
    tyb = L.blocks() // len(L.cases)
    used = [len(range(*R.paste_bands(c.y, c.ov_h, c.bg_h), 16)) for c in L.cases]
    assert tyb == 3 and all(u <= tyb for u in used) and sum(u < tyb for u in used) > len(used) // 2
    # sizes: the largest in_len about 14 × 20, no background beyond 160 × 96 but the wide ones of ≤ 48 rows
    assert max(c.in_len for c in R.RAGGED) == 280
    for c in R.RAGGED:
        assert (c.bg_w <= 160 and c.bg_h <= 96) or (c.bg_w <= 992 and c.bg_h <= 48), c.name
    # two kinds of T pitch, every T offset 16-B aligned, every image base too (but for the named misalignments)
    assert {c.t_pad > 0 for c in R.RAGGED} == {False, True}
    for c, d in zip(L.cases, L.descs):
        assert d["v"]["src_off"] % 16 == 0 and d["v"]["coef_off"] % 4 == 0
        assert d["p"]["bg_off"] % 16 == c.bg_mis and d["p"]["dst_off"] % 16 == c.dst_mis
    # a wave does 0, 1, 2 or 3 column tiles
    per_wave = {len(range(w, (c.ov_w + 15) >> 4, 4)) for c in R.RAGGED if c.bg_w <= 160 for w in range(4)}
    assert {0, 1, 2, 3} <= per_wave
    assert set(R.RAGGED_ALONE) <= {c.name for c in R.RAGGED}
    # the rows launched with both unpremultiply forms meet every K-step form and the three layouts
    wide = [c.name for c in R.ragged_wide_subset()]
    sub = [i for i, c in enumerate(L.cases) if c.name in wide]
    assert {R.k_form(nk) for i in sub for nk in L.nks[i]} == {"db1", "db2", "hoist3", "loop"}
    assert {(L.paths[i]["groups"], L.paths[i]["csplit"]) for i in sub} == {(True, True), (True, False), (False, False)}
    assert all(L.cases[i].ov_w <= R.MAGIC_MAX_OV_W and L.cases[i].bg_h <= 48 for i in sub)


@pytest.mark.parametrize("drop", ["s7_5t", "w_pow2", "one_row", "up_1t", "w_nk4"])
def test_ragged_table_needs_every_row(drop):
    """The property test fails when a row is removed (five of them tried here;
    ragged_table_problems' "dead row" check covers the rest)."""
    assert ragged_table_problems([c for c in R.RAGGED if c.name != drop]) != []


def test_trim_table_properties():
    L = R.Launch(R.TRIM_CASES)
    forms = set()
    past = False
    for k, (c, nks) in enumerate(zip(L.cases, L.nks)):
        ent = R.trim_entries(c, k)
        nt, hb = (c.ov_w + 15) >> 4, (c.in_len + 15) >> 4
        assert len(ent) == hb
        assert any(lo > 0 for lo, hi in ent) and any(hi < nt for lo, hi in ent) and sum(hi == 255 for lo, hi in ent) == 1
        assert all(0 <= lo < hi for lo, hi in ent)
        vb0, vb1 = R.paste_bands(c.y, c.ov_h, c.bg_h)
        _, words, _ = R.v_axis(c.in_len, c.ov_h, c.y & 15, c.ident)
        for y0 in range(vb0, vb1, 16):
            t = (y0 - c.y + (c.y & 15)) >> 4
            forms.add(R.k_form(nks[t]))
            k0 = int(words[4 * t])
            past |= k0 + 64 * nks[t] > 16 * hb           # a V window that runs past trim_bands(h.lines)
        # the trimmed reference differs from the untrimmed one
        M = L.Ms[k]
        assert not np.array_equal(R.trim_M(c, M, ent), M)
    assert forms == {"db1", "db2", "hoist3", "loop"} and past
    assert max(max(ks) for ks in L.nks) >= 5


def test_value_table_properties():
    M = R.value_table()
    assert M.shape == (256, 256, 4)
    for ch in range(3):
        key = M[..., ch].astype(np.int64) * 256 + M[..., 3]
        assert (np.bincount(key.ravel(), minlength=65536) == 1).all()      # every (c, a), once
    # over the 256 items every (bg, c, a) occurs in each channel, exactly once (the overlay sits on the
    # same background bytes at both widths: the hash does not know bg_w)
    ca = [(M[..., ch].astype(np.int32) << 8) | M[..., 3] for ch in range(3)]
    keys = np.empty((3, 256, 256, 256), np.int32)
    for i in range(256):
        c = R.value_case(i, 288)
        assert c.x == i & 15 and c.x + 256 <= 271 and c.y == 0 and R.value_case(i, 271).x == c.x
        bg = R.value_bg(i, 288)[:, c.x:c.x + 256]
        assert np.array_equal(bg, R.value_bg(i, 271)[:, c.x:c.x + 256])
        for ch in range(3):
            keys[ch, i] = (bg[..., ch].astype(np.int32) << 16) | ca[ch]
    for ch in range(3):
        assert (np.bincount(keys[ch].ravel(), minlength=1 << 24) == 1).all(), ch
    assert R.paths(288, 256, 864, 864, 0, 0, 3, 256)["groups"] and not R.paths(271, 256, 813, 813, 0, 0, 3, 256)["groups"]
    assert R.value_bg(7, 271)[5, 9, 2] == (7 + R.value_hash(9, 5, 2)) & 255


def test_value_references_produce_both_clamps():
    """The reference itself saturates: rgba2rgbA's min(255, ·) on the table,
    clip8 below 0 and above 255 through the 1:1 and the × 2 axes."""
    M = R.value_table()
    a = M[..., 3].astype(np.int64)
    q = 255 * M[..., 0].astype(np.int64) // np.maximum(a, 1)
    assert ((a > 0) & (a < 255) & (q > 255)).any() and ((a > 0) & (a < 255) & (q < 255)).any()
    assert all(R.unpremultiply_clamps(M)) and all(R.unpremultiply_clamps(R.v_resample(R.value_table(128), 128, 256, 0)))
    # each of the four channels leaves [0, 255] both ways: both packed clips of clip8x4_mfma saturate in both lanes
    lo, hi = R.v_sums_range(R.value_table(128), 128, 256)
    assert max(lo) < 0 and min(hi) > 255, (lo, hi)
    # the 256-row table cannot: constant or linear down every column
    lo, hi = R.v_sums_range(M[::2], 128, 256)
    assert min(lo) >= 0 and max(hi) <= 255
    # the 1:1 LANCZOS axis is not the identity in its descriptors, but its taps are: one tap of 2^22
    _, bounds, kk = ops.precompute_coeffs(256, 0.0, 256.0, 256)
    assert ((kk != 0).sum(axis=1) == 1).all() and (kk.max(axis=1) == 1 << 22).all()
