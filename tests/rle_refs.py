"""CPU reference of the scenes' run-length encodings (ipp_scene_rle /
SceneRunner.scene_rles) and the extra handmade maps shared by
tests/test_rle_cpu.py and tests/test_gpu_rle.py (not a test module).

``encode`` restates the definition of include/ipp.h one pixel at a time: walk
the pixels in column-major order and push a count at every change.
``encode_diff`` is an independent second form: ``np.diff`` of the transition
positions.  ``to_string`` / ``from_string`` are the COCO API's string rule in
scalar form.  None of them shares anything with the device's route (four
columns per lane, a scan over the columns' counts) or with labels_fmt."""
import numpy as np

from tests import contour_refs as C

HDR = 2


def encode(mask):
    """uint32 counts of the boolean (bg_h, bg_w) mask: zeros-run first."""
    mask = np.asarray(mask, bool)
    H, W = mask.shape
    counts, run, cur = [], 0, False
    for x in range(W):
        for y in range(H):
            v = bool(mask[y, x])
            if v != cur:
                counts.append(run)
                run, cur = 0, v
            run += 1
    counts.append(run)
    return np.array(counts, np.uint32)


def encode_diff(mask):
    """The same counts from the positions where the column-major mask changes."""
    flat = np.asarray(mask, bool).T.reshape(-1).astype(np.int8)
    t = np.flatnonzero(np.diff(flat, prepend=np.int8(0)))
    return np.diff(t, prepend=0, append=flat.size).astype(np.uint32)


def to_string(counts):
    """rleToString, one count and one 5-bit group at a time."""
    s = ""
    cnts = [int(v) for v in counts]
    for i in range(len(cnts)):
        x = cnts[i] - (cnts[i - 2] if i > 2 else 0)
        more = True
        while more:
            c = x % 32                   # the low five bits, of a negative x too
            x = (x - c) // 32            # the arithmetic shift
            more = x != (-1 if c >= 16 else 0)
            s += chr(48 + c + (32 if more else 0))
    return s


def from_string(s):
    """rleFrString."""
    cnts, p = [], 0
    while p < len(s):
        x, k, more = 0, 0, True
        while more:
            c = ord(s[p]) - 48
            x += (c % 32) * 32 ** k
            more = c >= 32
            p, k = p + 1, k + 1
            if not more and c % 32 >= 16:
                x -= 32 ** k
        if len(cnts) > 2:
            x += cnts[-2]
        cnts.append(x)
    return np.array(cnts, np.uint32)


def mask_of(vis, rows_i, scene, layer):
    """The full (bg_h, pitch) boolean mask of one descriptor: bit `layer` of scene `scene`'s map inside its box."""
    m = np.zeros(vis.shape[1:], bool)
    x0, y0, x1, y1 = (int(v) for v in rows_i[:4])
    m[y0:y1, x0:x1] = (vis[scene, y0:y1, x0:x1] >> layer) & 1
    return m


def reference(vis, rows, scene_layer, n_scenes, per_scene, bg_w):
    """(hdr (n, 2) int32, list of uint32 counts — empty for a {0, 0} descriptor)
    of every descriptor; vis (S, bg_h, >= bg_w) uint8, rows (n, 6), scene_layer (n, 2).
    A row that is no box of the map ((-1,-1,-1,-1) or any other) and a
    descriptor scene_layer does not map get {0, 0}."""
    rows, scene_layer = np.asarray(rows).reshape(-1, 6), np.asarray(scene_layer).reshape(-1, 2)
    hdr, out = np.zeros((len(rows), HDR), np.int32), []
    bg_h = vis.shape[1]
    for i in range(len(rows)):
        s, k = (int(v) for v in scene_layer[i])
        x0, y0, x1, y1 = (int(v) for v in rows[i][:4])
        if not (0 <= x0 < x1 <= bg_w and 0 <= y0 < y1 <= bg_h) or not (0 <= s < n_scenes and 0 <= k < per_scene):
            out.append(np.zeros(0, np.uint32))
            continue
        m = mask_of(vis, rows[i], s, k)[:, :bg_w]
        c = encode(m)
        hdr[i] = len(c), int(m.sum())
        out.append(c)
    return hdr, out


def case_reference(case):
    return reference(case.vis, case.rows, case.scene_layer, case.n_scenes, case.per_scene, case.bg_w)


def pack(hdr, counts):
    """(offsets int64[n], packed uint32): the host's running sum and what the pack launch writes."""
    nc = hdr[:, 0].astype(np.int64)
    offsets = np.concatenate([[0], np.cumsum(nc)[:-1]]).astype(np.int64)
    return offsets, np.concatenate(counts + [np.zeros(0, np.uint32)]).astype(np.uint32)


def scene_rles(vis, rows, bg_w):
    """rles[s][k] of a scene batch from a map (S, bg_h, >= bg_w) and (S, K, 6) rows: ``encode`` of every plane that
    has a box, None for the others."""
    S, K = rows.shape[:2]
    return [[None if rows[s, k, 0] < 0 else encode(mask_of(vis, rows[s, k], s, k)[:, :bg_w]) for k in range(K)]
            for s in range(S)]


def same_rles(got, exp):
    assert len(got) == len(exp)
    for gs, es in zip(got, exp):
        assert len(gs) == len(es)
        for g, e in zip(gs, es):
            assert (g is None) == (e is None)
            if g is not None:
                assert g.dtype == np.uint32 and g.shape == e.shape and np.array_equal(g, e)


# --- handmade maps -------------------------------------------------------------------------------------------
def _canvas(h, w, scenes=1):
    return np.zeros((scenes, h, (w + 15) // 16 * 16), np.uint8)


def handmade():
    """The extra handmade cases of the encoder, each named for the trap of the definition it sets."""
    cases = []
    # only pixel (0, 0): M(0) = 1, a leading 0
    v = _canvas(9, 21)
    v[0, 0, 0] = 1
    cases.append(C.Case("first_pixel", v, 21, 1))
    # only the last pixel: its closing position is N, no transition
    v = _canvas(9, 21)
    v[0, 8, 20] = 1
    cases.append(C.Case("last_pixel", v, 21, 1))
    # a full-height bar in the middle columns of 7 rows × 20 columns: its runs merge across the columns
    v = _canvas(7, 20)
    v[0, :, 3:6] = 1
    cases.append(C.Case("full_height_bar", v, 20, 1))
    # two adjacent columns, the left ending in the bottom row, the right starting in the top row: one merge
    v = _canvas(7, 20)
    v[0, 4:7, 9] = 1
    v[0, 0:2, 10] = 1
    cases.append(C.Case("merge_one_boundary", v, 20, 1))
    # a full-height box whose last column ends set, short of the last column: the closing transition of a box's
    # last column; and one ending in the last column: none
    v = _canvas(6, 20, scenes=2)
    v[0, :, 5:9] = 1
    v[0, 2, 6] = 0
    v[1, :, 17:20] = 1
    v[1, 0, 18] = 0
    cases.append(C.Case("full_height_ends", v, 20, 1))
    # a box touching the last row but not the first: every column closes at the next column's row 0
    v = _canvas(8, 24)
    v[0, 5:8, 3:24] = 1
    v[0, 6, 10] = 0
    cases.append(C.Case("bottom_rows", v, 24, 1))
    # a 130-column comb, every other row set: many counts per column, the carry crosses the lanes' dwords, two
    # 64-column groups and a 256-column block (it starts at column 191)
    v = _canvas(11, 330)
    v[0, 1:10:2, 191:321] = 1
    cases.append(C.Case("comb_130", v, 330, 1))
    # the same comb over the full height with the last row set: runs merge at every column boundary
    v = _canvas(9, 330)
    v[0, 0:9:2, 63:193] = 1
    cases.append(C.Case("comb_full_height", v, 330, 1))
    # a comb 300 columns wide: more columns than one round of the column scan takes
    v = _canvas(5, 320)
    v[0, 1:5:2, 7:307] = 1
    v[0, 2, 7:307:3] = 1
    cases.append(C.Case("comb_300", v, 320, 1))
    # a sparse box 300 columns wide: most columns have no transition, the carry runs across them and across two blocks
    v = _canvas(5, 560)
    v[0, 2, 250] = v[0, 1, 549] = v[0, 3, 255] = v[0, 3, 256] = 1
    cases.append(C.Case("sparse_wide", v, 560, 1))
    # one-row and one-column backgrounds
    v = _canvas(1, 37)
    v[0, 0, 3:9] = v[0, 0, 11] = v[0, 0, 36] = 1
    cases.append(C.Case("one_row", v, 37, 1))
    v = _canvas(37, 1)
    v[0, 3:9, 0] = v[0, 11, 0] = v[0, 36, 0] = 1
    cases.append(C.Case("one_column", v, 1, 1))
    # a box without a set bit (rows given by hand): the single count N; and a box outside the map: {0, 0}
    v = _canvas(6, 10)
    v[0, 1, 1] = 2
    cases.append(C.Case("empty_box_and_outside", v, 10, 2, scene_layer=[(0, 0), (0, 1), (0, 1)],
                        rows=[(2, 2, 5, 4, 0, 0), (1, 1, 2, 2, 1, 1), (8, 0, 11, 3, 0, 0)]))
    return cases


def all_handmade():
    return C.handmade() + handmade()


# --- scene batches (tests/scene_mask_refs.py) -----------------------------------------------------------------
def single_layer_scenes(fused):
    """Three scenes of one overlay each: the plan is ``plan_pipe``'s own."""
    from tests import scene_refs as SR
    cfg = fused.PipeConfig(margins=(4, 6, 3, 5), scale_min=0.3, scale_max=0.7)
    src, bgs, plan = SR.scene_noise_batch(fused, 3, 1, 90, 110, 2, 97, 125, cfg, 7)
    return src, bgs, plan, cfg


def scene_batches(fused):
    from tests import scene_mask_refs as MR
    return {"noise": MR.noise_scenes(fused), "odd": MR.odd_scenes(fused), "edge": MR.edge_scenes(fused),
            "cover": MR.cover_scenes(fused), "eight": MR.layered_scene(fused, 8), "single": single_layer_scenes(fused)}


def scene_reference(plan, overlays, alpha_min, cover_min):
    """(rles[s][k], rows (S, K, 6), vis) of a scene batch from the CPU map and rows."""
    from tests import scene_mask_refs as MR
    from tests import scene_refs as SR
    vis = MR.scene_map(plan, overlays, alpha_min, cover_min)
    rows = SR.scene_rows(plan, overlays, alpha_min, cover_min)
    return scene_rles(vis, rows, plan.bg_w), rows, vis
