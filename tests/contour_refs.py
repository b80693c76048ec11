"""CPU reference of the scene polygons (ipp_scene_contours /
SceneRunner.scene_polygons) and the handmade visibility maps shared by
tests/test_contours_cpu.py and tests/test_gpu_contours.py (not a test module).

``trace`` is a SEQUENTIAL crack follower: it walks from every unvisited top
edge, one edge at a time, by the left / straight / right rule of include/ipp.h,
and collects corners and the doubled signed area as it goes.  It shares nothing
with the device's route (edge slots, pointer jumping, atomic selection)."""
import numpy as np

HDR = 8
# direction of edge kind d (0 top +x, 1 right +y, 2 bottom -x, 3 left -y) and the side its outer pixel lies on
FWD = ((1, 0), (0, 1), (-1, 0), (0, -1))
OUT = ((0, -1), (1, 0), (0, 1), (-1, 0))
TAIL = ((0, 0), (1, 0), (1, 1), (0, 1))     # tail vertex of pixel (X, Y)'s edge of kind d, minus (X, Y)


def cycles(fg):
    """Every boundary cycle of the boolean image `fg` (background outside):
    a list of dicts {start: (x, y) of the start edge's tail, area2, verts:
    (V, 2) corners from the start edge's tail, n_edges, saddles}, in (y, x)
    order of their start edges."""
    fg = np.asarray(fg, bool)
    H, W = fg.shape
    pad = np.zeros((H + 2, W + 2), bool)
    pad[1:-1, 1:-1] = fg

    def F(x, y):
        return bool(pad[y + 1, x + 1])

    seen = set()
    out = []
    for Y in range(H):
        for X in range(W):
            if not (F(X, Y) and not F(X, Y - 1)) or (X, Y, 0) in seen:
                continue
            # (X, Y, top) is the least top edge of a cycle not walked yet: the raster scan meets it first
            x, y, d = X, Y, 0
            verts, area2, n, prev_d, saddles = [], 0, 0, None, 0
            edges = []
            while True:
                seen.add((x, y, d))
                edges.append((x, y, d))
                tx, ty = x + TAIL[d][0], y + TAIL[d][1]
                hx, hy = tx + FWD[d][0], ty + FWD[d][1]
                area2 += tx * hy - hx * ty
                n += 1
                (fx, fy), (ox, oy) = FWD[d], OUT[d]
                a = F(x + fx + ox, y + fy + oy)      # ahead on the outer side
                b = F(x + fx, y + fy)                # ahead
                if a:
                    if not b:
                        saddles += 1                 # the contour crosses to the diagonal pixel
                    x, y, d = x + fx + ox, y + fy + oy, (d + 3) % 4
                elif b:
                    x, y = x + fx, y + fy
                else:
                    d = (d + 1) % 4
                if (x, y, d) == (X, Y, 0):
                    break
            # corners: tails of edges whose direction differs from the predecessor's
            dirs = [e[2] for e in edges]
            for j, (ex, ey, ed) in enumerate(edges):
                if dirs[j - 1] != ed:
                    verts.append((ex + TAIL[ed][0], ey + TAIL[ed][1]))
            assert dirs[-1] != 0, "a start edge's tail is a corner"
            out.append(dict(start=(X, Y), area2=area2, verts=np.array(verts, np.int32).reshape(-1, 2), n_edges=n,
                            saddles=saddles))
    return out


def n_boundary_edges(fg):
    fg = np.asarray(fg, bool)
    pad = np.pad(fg, 1)
    c = pad[1:-1, 1:-1]
    return int((c & ~pad[:-2, 1:-1]).sum() + (c & ~pad[2:, 1:-1]).sum() + (c & ~pad[1:-1, :-2]).sum() +
               (c & ~pad[1:-1, 2:]).sum())


def trace(fg, origin=(0, 0), max_edges=None):
    """(hdr int32[8], polygon (V, 2) int32 or None, cycles) of one foreground
    image whose pixel (0, 0) is composite pixel `origin`."""
    cyc = cycles(fg)
    n_edges = sum(c["n_edges"] for c in cyc)
    assert n_edges == n_boundary_edges(fg)
    hdr = np.zeros(HDR, np.int32)
    hdr[0] = n_edges
    if max_edges is not None and n_edges > max_edges:
        hdr[7] = 1
        return hdr, None, cyc
    outer = [c for c in cyc if c["area2"] > 0]
    if not outer:
        return hdr, None, cyc
    best = outer[0]
    for c in outer[1:]:              # (y, x) order: a later cycle wins only with a strictly larger area
        if c["area2"] > best["area2"]:
            best = c
    ox, oy = origin
    poly = best["verts"] + np.array([ox, oy], np.int32)
    hdr[1], hdr[2] = len(outer), sum(1 for c in cyc if c["area2"] < 0)
    hdr[3], hdr[4], hdr[5], hdr[6] = len(poly), best["area2"], best["start"][0] + ox, best["start"][1] + oy
    return hdr, poly, cyc


def plane(vis, rows_i, scene, layer):
    """Foreground of one descriptor: bit `layer` of scene `scene`'s map inside its box, and the box origin."""
    x0, y0, x1, y1 = (int(v) for v in rows_i[:4])
    return ((vis[scene, y0:y1, x0:x1] >> layer) & 1).astype(bool), (x0, y0)


def reference(vis, rows, scene_layer, n_scenes, per_scene, max_edges=None):
    """Headers (n, 8) and polygons (list of (V, 2) or None) of every descriptor;
    vis (S, bg_h, >= bg_w) uint8, rows (n, 6), scene_layer (n, 2)."""
    rows, scene_layer = np.asarray(rows).reshape(-1, 6), np.asarray(scene_layer).reshape(-1, 2)
    hdrs, polys, stats = np.zeros((len(rows), HDR), np.int32), [], []
    for i in range(len(rows)):
        s, k = (int(v) for v in scene_layer[i])
        if rows[i][0] < 0 or not (0 <= s < n_scenes and 0 <= k < per_scene):
            polys.append(None)
            stats.append([])
            continue
        fg, origin = plane(vis, rows[i], s, k)
        hdrs[i], poly, cyc = trace(fg, origin, max_edges)
        polys.append(poly)
        stats.append(cyc)
    return hdrs, polys, stats


def pack(hdrs, polys):
    """(offsets int64[n], packed (sum V, 2) int32): the host's running sum and what the pack launch writes."""
    nv = hdrs[:, 3].astype(np.int64)
    offsets = np.concatenate([[0], np.cumsum(nv)[:-1]]).astype(np.int64)
    packed = np.zeros((int(nv.sum()), 2), np.int32)
    for i, p in enumerate(polys):
        if p is not None:
            packed[offsets[i]:offsets[i] + len(p)] = p
    return offsets, packed


def raster(poly, shape):
    """Fill a lattice polygon: +1 / -1 at every unit step of its vertical edges
    (down / up), then a cumulative sum along x.  With the foreground on the
    right of the contour, interior pixels come out as 1."""
    H, W = shape
    acc = np.zeros((H, W + 1), np.int32)
    poly = np.asarray(poly)
    for (xa, ya), (xb, yb) in zip(poly, np.roll(poly, -1, axis=0)):
        if xa == xb and ya != yb:
            lo, hi = min(ya, yb), max(ya, yb)
            acc[lo:hi, xa] += -1 if yb > ya else 1      # a +y edge has the foreground on its left in x: it closes a span
    return np.cumsum(acc, axis=1)[:, :W]


def rows_of(vis, scene_layer):
    """int32 (n, 6) rows in the shape ipp_pipe_scene_map writes: the tight box
    of each descriptor's bit, (-1,-1,-1,-1) without one; area = visible = count."""
    out = np.zeros((len(scene_layer), 6), np.int32)
    for i, (s, k) in enumerate(scene_layer):
        m = (vis[s] >> k) & 1
        ys, xs = np.nonzero(m)
        if len(ys) == 0:
            out[i, :4] = -1
        else:
            out[i] = (xs.min(), ys.min(), xs.max() + 1, ys.max() + 1, len(ys), len(ys))
    return out


# --- handmade maps ---------------------------------------------------------------------------------------
class Case:
    """One handmade batch: vis (S, bg_h, pitch) uint8, its rows and scene_layer."""

    def __init__(self, name, vis, bg_w, per_scene, scene_layer=None, rows=None):
        self.name, self.vis, self.bg_w, self.per_scene = name, np.ascontiguousarray(vis, np.uint8), bg_w, per_scene
        self.n_scenes, self.bg_h, self.pitch = self.vis.shape
        assert self.pitch % 16 == 0 and self.pitch >= bg_w and not self.vis[:, :, bg_w:].any()
        if scene_layer is None:
            scene_layer = [(s, k) for s in range(self.n_scenes) for k in range(per_scene)]
        self.scene_layer = np.array(scene_layer, np.int32).reshape(-1, 2)
        self.rows = rows_of(self.vis, self.scene_layer) if rows is None else np.array(rows, np.int32)
        self.vis.setflags(write=False)

    def ref(self, max_edges=None):
        return reference(self.vis, self.rows, self.scene_layer, self.n_scenes, self.per_scene, max_edges)


def _canvas(h, w, scenes=1):
    return np.zeros((scenes, h, (w + 15) // 16 * 16), np.uint8)


def spiral(n):
    """A one-pixel-wide square spiral in n×n: arms two pixels apart."""
    m = np.zeros((n, n), bool)
    x, y, dx, dy = 0, 0, 1, 0
    m[0, 0] = True
    while True:
        moved = 0
        while True:
            nx, ny = x + dx, y + dy
            ax, ay = nx + dx, ny + dy                  # stop one short of a pixel already set two ahead
            if not (0 <= nx < n and 0 <= ny < n) or m[ny, nx]:
                break
            if 0 <= ax < n and 0 <= ay < n and m[ay, ax]:
                break
            x, y = nx, ny
            m[y, x] = True
            moved += 1
        if moved < 2:
            break
        dx, dy = -dy, dx
    return m


def handmade():
    """The handmade cases, each named for why it exists."""
    cases = []
    # a single pixel: the smallest polygon, 4 edges, 4 vertices
    v = _canvas(16, 16)
    v[0, 5, 9] = 1
    cases.append(Case("single_pixel", v, 16, 1))
    # a plane filling an odd 97×125 background: all four borders, pitch 128
    v = _canvas(97, 125)
    v[0, :, :125] = 1
    cases.append(Case("full_odd_plane", v, 125, 1))
    # a diagonal pair: one saddle vertex, one 8-connected component, a pinch vertex listed twice
    v = _canvas(16, 16)
    v[0, 4, 4] = v[0, 5, 5] = 1
    cases.append(Case("diagonal_pair", v, 16, 1))
    # an 8×8 checkerboard: every interior vertex a saddle, the enclosed background pixels are holes
    v = _canvas(16, 16)
    yy, xx = np.mgrid[0:8, 0:8]
    v[0, 3:11, 2:10] = ((yy + xx) % 2 == 0)
    cases.append(Case("checkerboard", v, 16, 1))
    # a ring: one hole
    v = _canvas(32, 32)
    v[0, 5:20, 7:25] = 1
    v[0, 9:15, 12:20] = 0
    cases.append(Case("ring", v, 32, 1))
    # two blobs of different area (the larger is second in raster order), and two of equal area (the tie rule)
    v = _canvas(32, 48, scenes=2)
    v[0, 2:5, 3:7] = 1
    v[0, 10:20, 20:40] = 1
    v[1, 3:8, 30:36] = 1
    v[1, 3:9, 5:10] = 1           # 6×5 = 5×6 pixels, same start row: the lesser x wins
    cases.append(Case("two_blobs", v, 48, 1))
    # a one-pixel-wide spiral in 48×48: one cycle of a few thousand edges in a small box (the ranking depth)
    v = _canvas(48, 48)
    v[0, :, :48] = spiral(48)
    cases.append(Case("spiral", v, 48, 1))
    # bars crossing a 64-column word boundary, and exactly 64 and 128 wide (word carries)
    v = _canvas(24, 160, scenes=3)
    v[0, 4:7, 60:71] = 1
    v[0, 5, 3] = 1                # the box starts at column 3: the bar straddles the 62-pixel strips
    v[1, 2:5, 7:71] = 1           # 64 wide
    v[1, 9, 7:71:2] = 1           # teeth under it
    v[2, 2:6, 16:144] = 1         # 128 wide
    v[2, 6, 16:144:3] = 1
    cases.append(Case("bars", v, 160, 1))
    # bits 0 and 7 set in the same bytes with different shapes (plane selection)
    v = _canvas(32, 32)
    v[0, 4:12, 4:20] |= 1
    v[0, 8:28, 10:14] |= 128
    v[0, 20:24, 2:30] |= 128
    cases.append(Case("bits_0_and_7", v, 32, 8, scene_layer=[(0, 0), (0, 7)]))
    # a descriptor with a (-1) row between two live ones, and one that scene_layer does not map
    v = _canvas(16, 32, scenes=2)
    v[0, 2:6, 2:9] = 1
    v[1, 3:9, 20:31] = 2
    v[1, 1, 1] = 1
    sl = [(0, 0), (0, 1), (1, 1), (2, 0), (1, 5)]
    rows = rows_of(v, [(0, 0), (0, 1), (1, 1), (1, 0), (1, 0)])
    assert rows[1, 0] == -1
    cases.append(Case("empty_and_unmapped", v, 32, 2, scene_layer=sl, rows=rows))
    return cases


# --- scene batches (tests/scene_mask_refs.py) --------------------------------------------------------------
# Any mask on a W×H background has at most 2·W·H + W + H boundary edges (every
# lattice edge once); the largest background of the batches is 128×160: 41,248.
SCENE_MAX_EDGES = 1 << 16


def scene_batches(fused):
    from tests import scene_mask_refs as MR
    return {"noise": MR.noise_scenes(fused), "odd": MR.odd_scenes(fused), "edge": MR.edge_scenes(fused),
            "eight": MR.layered_scene(fused, 8)}


def scene_reference(plan, overlays, alpha_min, cover_min, max_edges=None):
    """(hdrs (S, K, 8), polys[s][k], stats[s][k], rows (S, K, 6), vis) of a scene batch from the CPU map and rows."""
    from tests import scene_mask_refs as MR
    from tests import scene_refs as SR
    S, K = plan.n_scenes, plan.per_scene
    vis = MR.scene_map(plan, overlays, alpha_min, cover_min)
    rows = SR.scene_rows(plan, overlays, alpha_min, cover_min)
    sl = [(s, k) for s in range(S) for k in range(K)]
    hdrs, polys, stats = reference(vis, rows.reshape(-1, 6), sl, S, K, max_edges)
    return (hdrs.reshape(S, K, HDR), [polys[s * K:(s + 1) * K] for s in range(S)],
            [stats[s * K:(s + 1) * K] for s in range(S)], rows, vis)
