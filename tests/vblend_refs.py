"""Direct harness of the pipe's V launch (csrc/ipp_pipe_vblend.hip:
ipp_pipe_vblend_bands, ipp_pipe_vblend_bands_trim, ipp_pipe_vblend_over)
without an H launch, CPU side: no torch, no GPU.

  T            hand-made on the host (pack_t) in the layout csrc/ipp_pipe_layout.h
               states, from M = what the H pass would have produced;
  tap tiles    built tile by tile by the host builder ipp_plan_mfma_tile
               (v_axis); the device planner is not involved;
  descriptors  written by hand (desc): only the fields the V launch reads;
  reference    the oracle's plain int64 chain (vblend_ref): precompute_coeffs,
               resample_v, unpremultiply, paste_rgba_onto_rgb of oracle/ops.py,
               and the mask of the composite bytes the launch owns.

The path predicates below (paths, k_form, magic_form) RESTATE vblend_block's
and vblend_entry's: which K-step form, which phase-2 layout, which
unpremultiply form a case takes.  They must move with the kernel.  The case
tables name, row by row, the paths each row is there for;
tests/test_vblend_refs_cpu.py asserts that the tables really meet them, and
tests/test_gpu_vblend_direct.py runs them.
"""
from collections import namedtuple

import numpy as np

from image_processor_pipeline_amd import _native as N
from image_processor_pipeline_amd.geometry import mfma_tiles
from oracle import ops

BAND = 16                     # kBandRows
MAX_OV_W = N.IPP_PIPE_MAX_OV_W
MAGIC_MAX_OV_W = 976          # widest max_ov_w that keeps the divisor table (magic_form)
HOIST_MAX = 3                 # IPP_VB_HOIST_MAX
DB_MAX = 2                    # IPP_VB_DB


# --------------------------------------------------------------------------- T

def t_groups(rows, nkb):
    """ipp_pipe_layout.h t_groups: T row groups of an item."""
    return ((rows + 15) // 16 * 16 + 64 * nkb + 16) // 4


def pack_t(M, pitch, t_rows, fill=0x80):
    """M uint8 [rows, ov_w, 4] (premultiplied RGBA, the H pass's result) as T
    bytes: [row group g][column x][channel c][row r], values XOR 0x80, one
    16-B group at g·pitch + 16·x.  t_rows (a multiple of 4, e.g. 4·t_groups)
    T rows are allocated; everything past M's rows and the pitch padding is
    `fill`: one byte, or an array of (t_rows / 4)·pitch bytes."""
    rows, w, _ = M.shape
    assert t_rows % 4 == 0 and t_rows >= rows and pitch % 16 == 0 and pitch >= 16 * w
    G = t_rows // 4
    if np.ndim(fill) == 0:
        T = np.full((G, pitch), fill, np.uint8)
    else:
        T = np.array(fill, np.uint8).reshape(G, pitch).copy()
    gm = (rows + 3) // 4
    padded = np.zeros((4 * gm, w, 4), np.uint8)
    padded[:rows] = M ^ 0x80
    new = padded.reshape(gm, 4, w, 4).transpose(0, 2, 3, 1)       # [g][x][c][r]
    valid = (4 * np.arange(gm)[:, None] + np.arange(4)[None, :]) < rows      # [g][r]: rows past M keep the fill
    old = T[:gm, :16 * w].reshape(gm, w, 4, 4)
    T[:gm, :16 * w] = np.where(valid[:, None, None, :], new, old).reshape(gm, 16 * w)
    return T.reshape(-1)


def unpack_t(T, rows, ov_w, pitch):
    """Inverse of pack_t: M [rows, ov_w, 4] from T bytes."""
    G = (rows + 3) // 4
    grp = np.asarray(T, np.uint8)[:G * pitch].reshape(G, pitch)[:, :16 * ov_w].reshape(G, ov_w, 4, 4)
    return (grp.transpose(0, 3, 1, 2).reshape(4 * G, ov_w, 4)[:rows] ^ 0x80).astype(np.uint8)


# --------------------------------------------------------------------------- taps

def tap_ntiles(out_len, phase):
    return (out_len + phase + 15) >> 4


def v_axis(in_len, out_len, phase, identity=0):
    """One V axis built by the host tile builder: (TAP_AXIS record [1] with
    coef_off 0, its coefficient words int32, [nK per tile]).  V axes: compact
    0, shift 0, phase = y & 15, nkb = ipp_plan_mfma_nk_bound."""
    lib = N.load()
    a = np.zeros(1, N.TAP_AXIS)
    ks = lib.ipp_plan_lanczos_ksize(0.0, float(in_len), out_len)
    nkb = lib.ipp_plan_mfma_nk_bound(in_len, out_len, ks)
    T = tap_ntiles(out_len, phase)
    a["in_size"], a["out_size"], a["identity"], a["shift"], a["phase"] = in_len, out_len, identity, 0, phase
    a["nkb"], a["compact"], a["n_tiles"], a["coef_off"] = nkb, 0, T, 0
    hdr, bias, blocks = mfma_tiles(a)
    for t, h4 in enumerate(hdr):
        assert h4[2] == t * nkb * 192 and h4[3] == 0
    # tile t's blocks at uint4 h4[2] = t·nkb·192 of the block area: the tiles back to back
    words = np.concatenate([hdr.reshape(-1), bias.reshape(-1), blocks.reshape(-1).view(np.int32)])
    return a, words, [int(nk) for nk in hdr[:, 1]]


# --------------------------------------------------------------------------- descriptors

def desc(t_off, t_pitch, t_rows, out_len, coef_off, bg_off, dst_off, bg_w, bg_h, bg_pitch, dst_pitch,
         ov_w, ov_h, x, y):
    """One PIPE_DESC with the fields the V launch reads: v.src_off, v.src_pitch,
    v.out_len, v.coef_off; h.lines = T rows; the whole p.  Everything else 0."""
    d = np.zeros(1, N.PIPE_DESC)
    d["v"]["src_off"], d["v"]["src_pitch"], d["v"]["out_len"], d["v"]["coef_off"] = t_off, t_pitch, out_len, coef_off
    d["h"]["lines"] = t_rows
    p = d["p"]
    p["bg_off"], p["dst_off"], p["bg_w"], p["bg_h"] = bg_off, dst_off, bg_w, bg_h
    p["bg_pitch"], p["dst_pitch"], p["ov_w"], p["ov_h"], p["x"], p["y"] = bg_pitch, dst_pitch, ov_w, ov_h, x, y
    p["ov_pitch"] = 4 * ov_w
    return d


# --------------------------------------------------------------------------- path predicates

def paste_bands(y, ov_h, bg_h):
    vb0 = (y >> 4) << 4
    vb1 = min(bg_h, ((y + ov_h + 15) >> 4) << 4)
    return vb0, max(vb1, vb0)


def paste_max_bands(max_ov_h):
    return (max_ov_h + 15 + BAND - 1) // BAND


def band_cols_split(bg_w, bg_h, bg_pitch, dst_pitch, x, ov_w, aligned):
    """(split?, gx0, gx1) — ipp_pipe_layout.h band_cols_split."""
    rb = 3 * bg_w
    gx0, gx1 = max(x, 0) >> 4, min((x + ov_w + 15) >> 4, bg_w >> 4)
    lr = 3 * (bg_w >> 4)
    ok = (bg_w & 15) == 0 and bg_pitch == rb and dst_pitch == rb and gx0 < gx1 and bg_h * lr * lr < (1 << 32) and aligned
    return bool(ok), gx0, gx1


def paths(bg_w, bg_h, bg_pitch, dst_pitch, bg_off, dst_off, x, ov_w, inplace=False):
    """The phase-2 layout of an item, as vblend_block decides it (the image
    base pointers are 16-B aligned): dict(groups, csplit, gx0, gx1, G)."""
    if inplace:
        bg_off, bg_pitch = dst_off, dst_pitch
    aligned = ((bg_off | dst_off) & 15) == 0
    groups = (bg_w & 15) == 0 and ((bg_pitch | dst_pitch) & 15) == 0 and aligned   # pitches 16 | → every row pointer too
    split, gx0, gx1 = band_cols_split(bg_w, bg_h, bg_pitch, dst_pitch, x, ov_w, aligned)
    csplit = groups and split
    G = (gx1 - gx0) if csplit else (bg_w >> 4)
    return dict(groups=groups, csplit=csplit, gx0=gx0, gx1=gx1, G=G, pow2=(G & (G - 1)) == 0,
                chunks=(3 * bg_w + 15) >> 4)


def k_form(nk):
    """The K-step form of a tile: 'db1', 'db2' (double-buffered), 'hoist3',
    'loop' (nK ≥ 4, the trim entry read per step)."""
    assert nk >= 1
    if nk <= DB_MAX:
        return "db%d" % nk
    return "hoist%d" % nk if nk <= HOIST_MAX else "loop"


def orow_stride(max_ov_w):
    return (max_ov_w + 32 + 3) & ~3


def magic_form(max_ov_w):
    """Does a launch with this max_ov_w unpremultiply by the LDS divisor table?"""
    return 16 * 4 * orow_stride(max_ov_w) + 1024 <= 65536


assert magic_form(MAGIC_MAX_OV_W) and not magic_form(MAGIC_MAX_OV_W + 1)


# --------------------------------------------------------------------------- reference

def v_resample(M, in_len, out_len, identity):
    """The V pass's result, still premultiplied: resample_v of M, or M's rows
    as they are on an identity axis."""
    assert M.shape[0] == in_len
    if identity:
        assert in_len == out_len
        return M
    _, bounds, kk = ops.precompute_coeffs(in_len, 0.0, float(in_len), out_len)
    return ops.resample_v(M, out_len, bounds, kk)


def v_overlay(M, in_len, out_len, identity):
    """The overlay the V launch pastes: v_resample, then unpremultiply."""
    return ops.unpremultiply(v_resample(M, in_len, out_len, identity))


def unpremultiply_clamps(P):
    """Per colour channel: does rgba2rgbA's min(255, ·) act on the
    premultiplied image P (255·c // a > 255 at some 0 < a < 255)?"""
    a = P[..., 3].astype(np.int64)
    mid = (a > 0) & (a < 255)
    return [bool((mid & (255 * P[..., ch].astype(np.int64) // np.maximum(a, 1) > 255)).any()) for ch in range(3)]


def owned_mask(bg_w, bg_h, x, y, ov_w, ov_h, path):
    """bool [bg_h, 3·bg_w]: the composite bytes the launch writes — under the
    column split the groups [gx0, gx1) of rows [vb0, vb1), otherwise the band
    rows."""
    m = np.zeros((bg_h, 3 * bg_w), bool)
    vb0, vb1 = paste_bands(y, ov_h, bg_h)
    if path["csplit"]:
        m[vb0:vb1, 48 * path["gx0"]:48 * path["gx1"]] = True
    else:
        m[vb0:vb1] = True
    return m


def vblend_ref(M, in_len, out_len, identity, bg, x, y, path):
    """(composite [bg_h, bg_w, 3], owned mask [bg_h, 3·bg_w])."""
    ov = v_overlay(M, in_len, out_len, identity)
    out = ops.paste_rgba_onto_rgb(bg, ov, x, y)
    return out, owned_mask(bg.shape[1], bg.shape[0], x, y, ov.shape[1], ov.shape[0], path)


def v_sums_range(M, in_len, out_len):
    """(min[4], max[4]) per channel of the V sums >> 22 before clip8 (to show
    that a case saturates, and in which channels)."""
    _, bounds, kk = ops.precompute_coeffs(in_len, 0.0, float(in_len), out_len)
    src = M.astype(np.int64)
    lo, hi = np.full(4, 1 << 40), np.full(4, -(1 << 40))
    for yy in range(out_len):
        ymin, cnt = bounds[yy]
        acc = ((1 << 21) + np.einsum("kxc,k->xc", src[ymin:ymin + cnt], kk[yy, :cnt])) >> 22
        lo, hi = np.minimum(lo, acc.min(axis=0)), np.maximum(hi, acc.max(axis=0))
    return lo.tolist(), hi.tolist()


# --------------------------------------------------------------------------- the ragged table

Case = namedtuple("Case", "name ov_w in_len ov_h ident bg_w bg_h x y bg_pad dst_pad bg_mis dst_mis t_pad why")


def row(name, ov_w, in_len, ov_h, bg_w, bg_h, x, y, why, ident=0, bg_pad=0, dst_pad=0, bg_mis=0, dst_mis=0, t_pad=0):
    return Case(name, ov_w, in_len, ov_h, ident, bg_w, bg_h, x, y, bg_pad, dst_pad, bg_mis, dst_mis, t_pad, why)


# name, ov_w, in_len, ov_h (= out_len), bg_w, bg_h, x, y, why.  Pads are bytes
# added to 3·bg_w (pitch), mis bytes added to the 16-B aligned image offset,
# t_pad 16-B groups added to T's pitch.
RAGGED = [
    # --- K-step forms × column-tile counts (1, 3, 4, 5, 9 tiles; last tile of 1, 15, 16 columns) ---
    row("up_1t", 16, 7, 20, 160, 96, 16, 3, "nK 1, 1 tile of 16; x&15 = 0; two bands; groups ∧ csplit, G = 1 (pow2)"),
    row("up_3t", 33, 9, 21, 160, 96, 1, 16, "nK 1, 3 tiles, last of 1; x&15 = 1; y&15 = 0; csplit G = 3 (not pow2)"),
    row("id_4t", 63, 30, 30, 160, 96, 15, 33, "identity axis, nK 1, 4 tiles, last of 15; x&15 = 15; three bands", ident=1),
    row("up_5t", 80, 12, 19, 160, 96, 80, 77, "nK 1, 5 tiles (a wave does 2: `more` taken), last of 16; x + ov_w = bg_w; y + ov_h = bg_h",
       t_pad=3),
    row("s2_9t", 129, 40, 18, 160, 93, 0, 75, "nK 1-2, 9 tiles (wave 0 does 3), last of 1; x = 0; y + ov_h = bg_h, bg_h&15 = 13: last band 13 rows"),
    row("s4_1t", 1, 72, 18, 160, 96, 47, 1, "nK 2, ov_w = 1; y&15 = 1"),
    row("s4_3t", 47, 72, 18, 159, 96, 5, 15, "nK 2, 3 tiles, last of 15; y&15 = 15: three bands; ¬groups (odd bg_w), chunks·nrows = 480"),
    row("s4_4t", 64, 76, 19, 160, 96, 96, 0, "nK 2, 4 tiles of 16; y = 0; x + ov_w = bg_w", t_pad=1),
    row("s4_5t", 65, 80, 20, 160, 96, 17, 44, "nK 2, 5 tiles (`more` taken with two buffers), last of 1; groups ∧ ¬csplit (padded pitches, 16 |), G = 10",
       bg_pad=16, dst_pad=32),
    row("s4_9t", 144, 68, 17, 160, 96, 16, 62, "nK 2, 9 tiles of 16 (wave 0 does 3)"),
    row("s7_1t", 15, 133, 19, 160, 96, 100, 32, "nK 3, 1 tile of 15"),
    row("s7_3t", 48, 133, 19, 160, 96, 31, 60, "nK 3, 3 tiles of 16; x&15 = 15", t_pad=2),
    row("s7_4t", 49, 140, 20, 160, 96, 64, 12, "nK 3, 4 tiles, last of 1; ¬groups by dst_off (even width)", dst_mis=4),
    row("s7_5t", 79, 140, 20, 160, 96, 33, 48, "nK 3, 5 tiles (a wave's tiles run past one iteration), last of 15"),
    row("s7_9t", 143, 133, 19, 160, 96, 1, 30, "nK 3, 9 tiles, last of 15; three bands; ¬groups by bg_off (even width)", bg_mis=8),
    row("l4_1t", 16, 224, 16, 160, 96, 144, 50, "nK 4 (generic loop), 1 tile; x + ov_w = bg_w"),
    row("l4_3t", 33, 252, 18, 160, 96, 50, 12, "nK 4, 3 tiles, last of 1", t_pad=1),
    row("l4_4t", 64, 252, 18, 157, 96, 93, 64, "nK 4, 4 tiles; ¬groups (odd bg_w), x + ov_w = bg_w"),
    row("l4_5t", 80, 224, 16, 160, 96, 48, 80, "nK 4, 5 tiles; y + ov_h = bg_h"),
    row("l4_9t", 129, 252, 18, 160, 96, 20, 0, "nK 4, 9 tiles, last of 1; y = 0"),
    row("l5_3t", 47, 280, 20, 160, 96, 60, 32, "nK 5 (generic loop), the largest in_len (14 × 20 rows)"),
    row("l5_9t", 144, 280, 20, 160, 96, 0, 62, "nK 5, 9 tiles; three bands"),
    # --- small overlays ---
    row("one_row", 40, 3, 1, 160, 96, 7, 47, "ov_h = 1 (3 rows → 1), inside one band, its last row"),
    row("one_px", 1, 1, 1, 16, 16, 15, 15, "ov_w = ov_h = 1 at the last pixel of a 16 × 16 composite", ident=1),
    row("in_band", 20, 25, 10, 160, 96, 30, 34, "an overlay inside one band (rows 34..43 of band 32..47)"),
    # --- the wide composites (also the unpremultiply forms' cases) ---
    row("w_nosplit", 300, 60, 20, 992, 48, 100, 9, "groups ∧ ¬csplit, G = 62: nrows·G = 992 > 256, not pow2; 19 tiles",
       bg_pad=16, dst_pad=16),
    row("w_pow2", 250, 24, 30, 512, 48, 19, 18, "groups ∧ ¬csplit, G = 32: pow2, nrows·G = 512 > 256", bg_pad=48, dst_pad=0),
    row("w_split", 400, 30, 12, 992, 40, 333, 20, "groups ∧ csplit, G = 26: nrows·G > 256 in the full band, last band 8 rows"),
    row("w_chunks", 500, 40, 16, 991, 48, 491, 32, "¬groups (odd bg_w): chunks 186 · 16 rows = 2976 > 1024, 3·bg_w mod 16 = 13; x + ov_w = bg_w"),
    row("w_nk3", 200, 140, 20, 992, 48, 37, 16, "nK 3 on a wide composite (both unpremultiply forms); groups ∧ csplit"),
    row("w_nk4", 130, 252, 18, 991, 40, 500, 0, "nK 4 (generic loop) on a wide composite; ¬groups (odd bg_w)"),
    row("w_nk5", 90, 280, 20, 992, 48, 801, 16, "nK 5 on a wide composite; groups ∧ ¬csplit", bg_pad=32, dst_pad=16),
    row("w_976", 976, 20, 8, 992, 16, 16, 5, "the widest overlay the divisor table takes (61 tiles)", ident=0),
]
# the three items also launched alone, with descs advanced
RAGGED_ALONE = ("s7_5t", "l4_9t", "w_chunks")

# What each row is there for, as tags case_tags computes from the row itself
# (the prose above says the same).  tests/test_vblend_refs_cpu.py asserts that
# every claim is true, that the claims cover RAGGED_REQUIRED, and that every
# row claims something no other row claims: no row can be dropped or bent
# without the property test failing.
RAGGED_CLAIMS = {
    "up_1t": "nk1xct1 last16 x15_0 t_dense csplit g_pow2",
    "up_3t": "nk1xct3 last1 x15_1 y15_0 g_not2",
    "id_4t": "nk1xct4 last15 x15_15 ident",
    "up_5t": "nk1xct5 x_right t_pad",
    "s2_9t": "nk1xct9 x_0 y_bottom_ragged",
    "s4_1t": "nk2xct1 y15_1",
    "s4_3t": "nk2xct3 y15_15 chunks_odd ch_lt1024",
    "s4_4t": "nk2xct4 y_0",
    "s4_5t": "nk2xct5 groups_nosplit g_lt256",
    "s4_9t": "nk2xct9",
    "s7_1t": "nk3xct1",
    "s7_3t": "nk3xct3",
    "s7_4t": "nk3xct4 chunks_dstoff",
    "s7_5t": "nk3xct5",
    "s7_9t": "nk3xct9 chunks_bgoff",
    "l4_1t": "nk4xct1",
    "l4_3t": "nk4xct3",
    "l4_4t": "nk4xct4",
    "l4_5t": "nk4xct5 y_bottom",
    "l4_9t": "nk4xct9",
    "l5_3t": "nk5xct3",
    "l5_9t": "nk5xct9 three_bands",
    "one_row": "h1",
    "one_px": "w1",
    "in_band": "one_band",
    "w_nosplit": "nosplit_g_gt256 nosplit_g_not2",
    "w_pow2": "nosplit_g_pow2",
    "w_split": "csplit_g_gt256",
    "w_chunks": "ch_gt1024",
    "w_nk3": "wide_nk3",
    "w_nk4": "wide_nk4",
    "w_nk5": "wide_nk5",
    "w_976": "ov_w976",
}
RAGGED_REQUIRED = (
    ["nk%dxct%d" % (k, t) for k in (1, 2, 3, 4) for t in (1, 3, 4, 5, 9)] + ["nk5xct3"]
    + "last1 last15 last16 csplit groups_nosplit chunks_odd chunks_bgoff chunks_dstoff g_pow2 g_not2 g_lt256".split()
    + "nosplit_g_gt256 nosplit_g_pow2 nosplit_g_not2 ch_lt1024 ch_gt1024 x15_0 x15_1 x15_15 x_0 x_right y_0".split()
    + "y_bottom_ragged y15_0 y15_1 y15_15 w1 h1 one_band three_bands t_dense t_pad ident ov_w976 wide_nk3 wide_nk4 wide_nk5".split())


def ragged_wide_subset():
    """The ragged rows launched with both unpremultiply forms (max_ov_w = 976
    and 992): those whose composite has at most 48 rows (and at most 992
    columns: all of them), as they are."""
    return [c for c in RAGGED if c.bg_h <= 48]


def case_nks(c):
    """nK of every tile of the case's V axis, from the host-built headers."""
    return v_axis(c.in_len, c.ov_h, c.y & 15, c.ident)[2]


def case_tags(c, path, nks):
    """Every property of a row the tables speak of (path: paths(...) of the
    row as laid out, nks: its tiles' nK)."""
    ct = (c.ov_w + 15) >> 4
    vb0, vb1 = paste_bands(c.y, c.ov_h, c.bg_h)
    bands = list(range(vb0, vb1, BAND))
    tags = set()
    for y0 in bands:
        nk = nks[(y0 - c.y + (c.y & 15)) >> 4]
        tags.add("nk%dxct%d" % (min(nk, 5), ct))
        if c.bg_w > 160:
            tags.add("wide_nk%d" % min(nk, 5))
    tags.add("last%d" % ((c.ov_w - 1) % 16 + 1))
    nrows_max = max(min(BAND, c.bg_h - y0) for y0 in bands)
    if path["groups"]:
        tags.add("csplit" if path["csplit"] else "groups_nosplit")
        for t in ("g_pow2" if path["pow2"] else "g_not2", "g_gt256" if nrows_max * path["G"] > 256 else "g_lt256"):
            tags.update((t, ("csplit_" if path["csplit"] else "nosplit_") + t))
    else:
        if c.bg_w & 1:
            tags.add("chunks_odd")
        elif c.bg_mis & 15:
            tags.add("chunks_bgoff")
        elif c.dst_mis & 15:
            tags.add("chunks_dstoff")
        if (3 * c.bg_w) & 15:
            tags.add("ch_gt1024" if nrows_max * path["chunks"] > 1024 else "ch_lt1024")
    tags.add("x15_%d" % (c.x & 15))
    tags.add("y15_%d" % (c.y & 15))
    for on, tag in ((c.x == 0, "x_0"), (c.x + c.ov_w == c.bg_w, "x_right"), (c.y == 0, "y_0"),
                    (c.y + c.ov_h == c.bg_h, "y_bottom"), (c.y + c.ov_h == c.bg_h and c.bg_h & 15, "y_bottom_ragged"),
                    (c.ov_w == 1, "w1"), (c.ov_h == 1, "h1"), (len(bands) == 1 and c.ov_h > 1, "one_band"),
                    (len(bands) == 3, "three_bands"), (c.t_pad == 0, "t_dense"), (c.t_pad > 0, "t_pad"),
                    (c.ident, "ident"), (True, "ov_w%d" % c.ov_w)):
        if on:
            tags.add(tag)
    return tags


def case_M(c, seed):
    """The case's hand-made H-pass result: noise, with a fully transparent and
    a fully opaque stretch, so colour exceeds alpha (rgba2rgbA's clamp) often."""
    rng = np.random.default_rng([seed, c.in_len, c.ov_w])
    M = rng.integers(0, 256, (c.in_len, c.ov_w, 4), np.uint8)
    M[: c.in_len // 5, : max(1, c.ov_w // 3), 3] = 0
    M[c.in_len // 2:, c.ov_w // 2:, 3] = 255
    return M


def case_bg(c, seed):
    return np.random.default_rng([seed, c.bg_w, c.bg_h]).integers(0, 256, (c.bg_h, c.bg_w, 3), np.uint8)


class Launch:
    """The buffers of one launch over `cases` (any objects with Case's
    fields): descs, coefs, T, bg and dst offsets, laid out back to back.

    T past each item's rows and its pitch padding hold seeded garbage, the
    padding of bg rows too.  Ms / bgs: per-case arrays (defaults: case_M /
    case_bg with `seed`)."""

    def __init__(self, cases, seed=1, Ms=None, bgs=None, garbage=7, shared_t=False):
        self.cases = list(cases)
        n = len(self.cases)
        self.descs = np.zeros(n, N.PIPE_DESC)
        self.Ms = [case_M(c, seed) for c in self.cases] if Ms is None else list(Ms)
        self.bgs = [case_bg(c, seed) for c in self.cases] if bgs is None else list(bgs)
        rng = np.random.default_rng([garbage, n])
        coefs, ts, self.paths, self.nks, self.t_spans = [], [], [], [], []
        coef_off = t_off = bg_off = dst_off = 0
        axes = {}
        for i, c in enumerate(self.cases):
            assert self.Ms[i].shape == (c.in_len, c.ov_w, 4) and self.bgs[i].shape == (c.bg_h, c.bg_w, 3)
            assert 0 <= c.x and c.x + c.ov_w <= c.bg_w and 0 <= c.y and c.y + c.ov_h <= c.bg_h
            key = (c.in_len, c.ov_h, c.y & 15, c.ident)
            if key not in axes:
                a, words, nks = v_axis(*key)
                axes[key] = (coef_off, int(a["nkb"][0]), nks)
                coefs.append(words)
                coef_off += (len(words) + 3) // 4 * 4
                if len(words) % 4:
                    coefs.append(np.zeros(4 - len(words) % 4, np.int32))
            c_off, nkb, nks = axes[key]
            self.nks.append(nks)
            t_pitch = 16 * (c.ov_w + c.t_pad)
            t_rows = 4 * t_groups(c.in_len, nkb)
            if not (shared_t and i > 0):
                fill = rng.integers(0, 256, t_rows // 4 * t_pitch, np.uint8)
                ts.append(pack_t(self.Ms[i], t_pitch, t_rows, fill))
                this_t = t_off
                t_off += len(ts[-1])
            self.t_spans.append((this_t, t_pitch, t_rows))
            bg_pitch, dst_pitch = 3 * c.bg_w + c.bg_pad, 3 * c.bg_w + c.dst_pad
            b0, d0 = bg_off + c.bg_mis, dst_off + c.dst_mis
            self.descs[i] = desc(this_t, t_pitch, c.in_len, c.ov_h, c_off, b0, d0, c.bg_w, c.bg_h, bg_pitch, dst_pitch,
                                 c.ov_w, c.ov_h, c.x, c.y)[0]
            self.paths.append(paths(c.bg_w, c.bg_h, bg_pitch, dst_pitch, b0, d0, c.x, c.ov_w))
            bg_off = (b0 + c.bg_h * bg_pitch + 15) // 16 * 16
            dst_off = (d0 + c.bg_h * dst_pitch + 15) // 16 * 16
        self.coefs = np.concatenate(coefs)
        self.T = np.concatenate(ts)
        self.bg_bytes, self.dst_bytes = bg_off + 16, dst_off + 16
        self.bg = rng.integers(0, 256, self.bg_bytes, np.uint8)      # garbage between and beside the images
        for i, c in enumerate(self.cases):
            self.bg_rows(self.bg, i, "bg")[:, :3 * c.bg_w] = self.bgs[i].reshape(c.bg_h, -1)
        self.bg_w, self.bg_h = max(c.bg_w for c in self.cases), max(c.bg_h for c in self.cases)
        self.max_ov_w, self.max_ov_h = max(c.ov_w for c in self.cases), max(c.ov_h for c in self.cases)

    def bg_rows(self, buf, i, which="dst"):
        """View [bg_h, pitch] of item i's image rows in a flat bg / dst buffer."""
        p, c = self.descs[i]["p"], self.cases[i]
        off, pitch = int(p[which + "_off"]), int(p[which + "_pitch"])
        return np.lib.stride_tricks.as_strided(buf[off:], (c.bg_h, pitch), (pitch, 1))

    def blocks(self, max_ov_h=None, bg_h=None):
        tyb = min(paste_max_bands(max_ov_h or self.max_ov_h), ((bg_h or self.bg_h) + 15) // 16)
        return tyb * len(self.cases)

    def reference(self, i, M=None, bg=None, inplace=False):
        c = self.cases[i]
        path = self.paths[i]
        if inplace:
            p = self.descs[i]["p"]
            path = paths(c.bg_w, c.bg_h, 0, int(p["dst_pitch"]), 0, int(p["dst_off"]), c.x, c.ov_w, inplace=True)
        return vblend_ref(self.Ms[i] if M is None else M, c.in_len, c.ov_h, c.ident,
                          self.bgs[i] if bg is None else bg, c.x, c.y, path)

    def expected(self, poison, refs=None):
        """(expected dst bytes, mask of the owned bytes) for a dst pre-filled with `poison`."""
        exp = np.full(self.dst_bytes, poison, np.uint8)
        own = np.zeros(self.dst_bytes, bool)
        for i, c in enumerate(self.cases):
            comp, mask = refs[i] if refs is not None else self.reference(i)
            rows, orow = self.bg_rows(exp, i), self.bg_rows(own, i)
            rows[:, :3 * c.bg_w] = np.where(mask, comp.reshape(c.bg_h, -1), poison)
            orow[:, :3 * c.bg_w] = mask
        return exp, own


# --------------------------------------------------------------------------- the trim table's cases

# name, ov_w, in_len, ov_h, bg_w, bg_h, x, y; trim entries per H band are made by trim_entries
TRIM_CASES = [
    row("t_nk1", 80, 20, 24, 160, 64, 33, 7, "nK 1 (upscale): lo > 0, hi below the 5 tiles"),
    row("t_nk2", 100, 80, 20, 160, 64, 16, 17, "nK 2: 7 tiles"),
    row("t_nk3", 64, 140, 20, 160, 64, 40, 16, "nK 3: 4 tiles"),
    row("t_nk4", 144, 252, 18, 160, 64, 9, 34, "nK 4 (entry read per K step): 9 tiles"),
    row("t_nk5", 47, 280, 20, 160, 64, 100, 44, "nK 5; the last tile's window runs past trim_bands(h.lines)"),
]


def trim_entries(c, k):
    """Hand-made (lo, hi) of case c's H bands [0, trim_bands(in_len)): lo > 0
    and hi below the tile count where there are ≥ 3 tiles, rotating with the
    band; one band per item has hi = 255 (no upper bound)."""
    nt, nb = (c.ov_w + 15) >> 4, (c.in_len + 15) >> 4
    out = []
    for b in range(nb):
        lo = 1 + (b + k) % 2 if nt >= 3 else 0
        hi = max(lo + 1, nt - 1 - (b % 2))
        if b == (k + 1) % nb:
            hi = 255
        out.append((min(lo, nt - 1), hi))
    return out


def trim_const(lo, hi, ct):
    return ct < lo or (ct >= hi and hi != 255)


def trim_M(c, M, entries, value=0):
    """M with the column tiles the entries mark constant set to `value` in
    those 16-row bands."""
    out = M.copy()
    nt = (c.ov_w + 15) >> 4
    for b, (lo, hi) in enumerate(entries):
        for ct in range(nt):
            if trim_const(lo, hi, ct):
                out[16 * b:16 * b + 16, 16 * ct:16 * ct + 16] = value
    return out


# --------------------------------------------------------------------------- the value tables

def value_table(rows=256):
    """[256, 256, 4]: pixel (x = c, y = a) = (c, (c + 85) & 255, (c + 170) & 255, a).

    rows = 128: the table for the × 2 upscale.  The 256-row table is constant
    (colour) or linear (alpha) down every column, which no LANCZOS axis
    overshoots; this one steps every two rows — rows 4k, 4k + 1 have alpha k
    and the table's colours, rows 4k + 2, 4k + 3 alpha 255 - k and the colours
    shifted by 128 — so the V sums leave [0, 255] both ways in each of the four
    channels (asserted per channel by the tests)."""
    c = np.arange(256)
    M = np.empty((rows, 256, 4), np.uint8)
    if rows == 256:
        a, sh = np.arange(256), np.zeros(256, np.int64)
    else:
        assert rows == 128
        r = np.arange(128)
        hi = (r >> 1) & 1
        a, sh = np.where(hi, 255 - r // 4, r // 4), 128 * hi
    for ch in range(3):
        M[..., ch] = (c[None, :] + 85 * ch + sh[:, None]) & 255
    M[..., 3] = a[:, None]
    return M


def value_hash(X, Y, ch):
    """Background byte of item i at composite (X, Y), channel ch =
    (i + value_hash) & 255.  Its low nibble does not depend on X, so that with
    x = i & 15 the 256 items put every byte value under every overlay pixel."""
    return 16 * ((5 * X + 3 * Y + 7 * ch) & 15) + ((11 * Y + 3 * ch) & 15)


_hash_grids = {}


def value_bg(i, bg_w, bg_h=256):
    if (bg_w, bg_h) not in _hash_grids:
        Y, X, ch = np.meshgrid(np.arange(bg_h), np.arange(bg_w), np.arange(3), indexing="ij")
        _hash_grids[bg_w, bg_h] = value_hash(X, Y, ch).astype(np.uint8)
    return _hash_grids[bg_w, bg_h] + np.uint8(i)          # uint8 wrap-around = & 255


def value_case(i, bg_w, rows=256, ident=1, bg_h=256):
    return row("v%d" % i, 256, rows, 256, bg_w, bg_h, i & 15, 0, "value table", ident=ident)
