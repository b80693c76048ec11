"""CPU reference and designed cases for keep-largest (csrc/ipp_ccl.hip),
shared by tests/test_ccl_refs_cpu.py and tests/test_gpu_ccl_edges.py.

The reference restates ``oracle/ops.py keep_largest_component`` on the whole
frame: fg = α > 1, ``scipy.ndimage.label`` with the 3×3 structure, the largest
area, and on equal areas the component whose first 2×2 block in raster order
comes first.  That tie rule is the project's restatement of OpenCV's block-based
labelling order; kernel and oracle both mark it UNPINNED (OpenCV is absent), and
nothing here claims OpenCV parity.  All work is per foreground pixel and per
component inside NumPy/SciPy; there is no Python loop over pixels.

Kernel vocabulary (header of ipp_ccl.hip):
  * run-start index  G = (((y >> 1) * wb + (x >> 1)) << 1) + (y & 1), wb = ⌈w/2⌉;
    a component's root is the smallest G of its run starts;
  * a component is OPEN when it has a pixel on row or column 0 or 63 of a 64×64
    tile, else CLOSED; images of more than 2^23 run-start slots (2·wb·hb)
    treat every component as open ("all-open mode");
  * k_ccl_label emits one entry per open component OF A TILE (the pieces a
    tile cuts a component into count one each), counted in ``counts[image]``.

Each designed-case builder returns a ``Case``: the mask and the properties the
case claims.  ``check_claims`` asserts them from the reference alone, so a case
cannot silently stop covering its branch.
"""
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import numpy as np
from scipy import ndimage

TW = 64
CMAX = 1024                      # components per tile at the most (one per 2×2 block)
CLOSED_SLOTS = 1 << 23
_S8 = np.ones((3, 3), int)
_BIG = np.iinfo(np.int64).max


def slots(h: int, w: int) -> int:
    return 2 * ((w + 1) // 2) * ((h + 1) // 2)


def all_open(h: int, w: int) -> bool:
    return slots(h, w) > CLOSED_SLOTS


def n_tiles(h: int, w: int) -> int:
    return ((h + TW - 1) // TW) * ((w + TW - 1) // TW)


@dataclass
class Components:
    """Per-component facts of a mask; arrays are indexed by label (0 unused)."""
    lab: np.ndarray
    n: int
    area: np.ndarray
    root: np.ndarray             # smallest run-start index G
    first: np.ndarray            # first 2×2 block in raster order (the oracle's tie key)
    open: np.ndarray             # touches row/column 0 or 63 of a tile
    best: int                    # the kept label, 0 when there is none
    tied: int                    # components sharing the largest area


def components(mask: np.ndarray) -> Components:
    mask = np.asarray(mask, bool)
    h, w = mask.shape
    wb = (w + 1) // 2
    lab, n = ndimage.label(mask, structure=_S8)
    ys, xs = np.nonzero(mask)
    L = lab[ys, xs]
    area = np.bincount(L, minlength=n + 1).astype(np.int64)
    first = np.full(n + 1, _BIG, np.int64)
    np.minimum.at(first, L, (ys >> 1) * wb + (xs >> 1))
    start = mask.copy()
    start[:, 1:] &= ~mask[:, :-1]
    sy, sx = np.nonzero(start)
    root = np.full(n + 1, _BIG, np.int64)
    np.minimum.at(root, lab[sy, sx], (((sy >> 1) * wb + (sx >> 1)) << 1) + (sy & 1))
    ring = ((ys & 63) == 0) | ((ys & 63) == 63) | ((xs & 63) == 0) | ((xs & 63) == 63)
    op = np.zeros(n + 1, bool)
    op[L[ring]] = True
    best, tied = 0, 0
    if n:
        top = np.flatnonzero(area[1:] == area[1:].max()) + 1
        best, tied = int(top[np.argmin(first[top])]), int(top.size)
    return Components(lab, n, area, root, first, op, best, tied)


def keep_largest_full(img: np.ndarray, comps: Optional[Components] = None):
    """(H, W, 4) BGRA → (the whole frame with α zeroed outside the kept
    component, the α ≠ 0 bbox (x0, y0, x1, y1) or None).  Without any α > 1
    the frame is unchanged (label 0, the background, is "kept")."""
    alpha = img[..., 3]
    c = comps if comps is not None else components(alpha > 1)
    out = img.copy()
    if c.n:
        out[..., 3] = np.where(c.lab == c.best, alpha, 0)
    a = out[..., 3] != 0
    rows = np.flatnonzero(a.any(axis=1))
    if rows.size == 0:
        return out, None
    cols = np.flatnonzero(a.any(axis=0))
    return out, (int(cols[0]), int(rows[0]), int(cols[-1]) + 1, int(rows[-1]) + 1)


def run_start_root(mask: np.ndarray, label: int, comps: Optional[Components] = None) -> int:
    """Root G (smallest run-start index) of component `label` of ndimage.label(mask, 3×3)."""
    c = comps if comps is not None else components(mask)
    return int(c.root[label])


def is_open(mask: np.ndarray, label: int, comps: Optional[Components] = None) -> bool:
    c = comps if comps is not None else components(mask)
    return bool(c.open[label])


def tile_entries(mask: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """Per 64×64 tile (row-major): (components of the tile's own sub-mask,
    those of them on the tile's ring).  Tiles are labelled apart by spreading
    them onto a 65-pixel grid, so one ndimage.label call does all of them."""
    mask = np.asarray(mask, bool)
    h, w = mask.shape
    ty, tx = (h + TW - 1) // TW, (w + TW - 1) // TW
    ex = np.zeros((ty, TW + 1, tx, TW + 1), bool)
    pad = np.zeros((ty * TW, tx * TW), bool)
    pad[:h, :w] = mask
    ex[:, :TW, :, :TW] = pad.reshape(ty, TW, tx, TW)
    ex = ex.reshape(ty * (TW + 1), tx * (TW + 1))
    lab, n = ndimage.label(ex, structure=_S8)
    ys, xs = np.nonzero(ex)
    L = lab[ys, xs]
    tile_of = np.zeros(n + 1, np.int64)
    tile_of[L] = (ys // (TW + 1)) * tx + xs // (TW + 1)
    ry, rx = ys % (TW + 1), xs % (TW + 1)
    ring = (ry == 0) | (ry == TW - 1) | (rx == 0) | (rx == TW - 1)
    op = np.zeros(n + 1, bool)
    op[L[ring]] = True
    total = np.bincount(tile_of[1:], minlength=ty * tx)
    opened = np.bincount(tile_of[1:][op[1:]], minlength=ty * tx)
    return total, opened


def expected_entries(mask: np.ndarray) -> int:
    """What k_ccl_label leaves in counts[image]."""
    total, opened = tile_entries(mask)
    return int(total.sum() if all_open(*mask.shape) else opened.sum())


def image_from_mask(mask: np.ndarray, rng) -> np.ndarray:
    """Random BGR; α in 2..255 on the mask and 0..1 off it."""
    h, w = mask.shape
    im = rng.integers(0, 256, (h, w, 4), np.uint8)
    im[..., 3] = np.where(mask, rng.integers(2, 256, (h, w), np.uint8), rng.integers(0, 2, (h, w), np.uint8))
    return im


# --------------------------------------------------------------------------- stress masks

def ccl_stress_masks(rng):
    """Foreground patterns for the bit-plane run labelling (64×64 tiles, lane =
    row): densities around the 8-connected percolation threshold, the maximum
    component count per tile (isolated pixels on the even grid: 1024 per
    tile, many LDS stats passes, mixed tiles in the emit), a serpentine that
    crosses every tile border many times (deep union-find chains), full rows
    (runs reaching column 63), equal-area components in different tiles (tie
    rule across tiles), and sizes off the tile grid."""
    out = []
    for (h, w), dens in [((130, 200), 0.3), ((129, 193), 0.42), ((200, 131), 0.6), ((64, 64), 0.5),
                         ((65, 127), 0.45)]:
        out.append(rng.random((h, w)) < dens)
    grid = np.zeros((128, 192), bool)
    grid[::2, ::2] = True
    grid[100, 101] = grid[101, 102] = True          # one 3-pixel component wins
    out.append(grid)
    snake = np.zeros((300, 260), bool)
    for c in range(0, 260, 3):
        snake[:, c] = True
        snake[0 if (c // 3) % 2 else 299, c:c + 3] = True
    snake[150, 1] = False                            # notch: still one component
    out.append(snake)
    full = np.zeros((70, 190), bool)
    full[3:9, :] = True
    full[40, 5:70] = True
    out.append(full)
    tie = np.zeros((140, 150), bool)
    tie[70:72, 100:103] = True                       # area 6, later block
    tie[5:7, 130:133] = True                         # area 6, first block: wins
    out.append(tie)
    for (h, w) in [(1, 1), (1, 77), (77, 1), (2, 65)]:
        out.append(rng.random((h, w)) < 0.6)
    return out


def even_grid_mask() -> np.ndarray:
    """The even grid of ccl_stress_masks: 1024 components per tile, 63 of them open."""
    grid = np.zeros((128, 192), bool)
    grid[::2, ::2] = True
    grid[100, 101] = grid[101, 102] = True
    return grid


# --------------------------------------------------------------------------- designed cases

@dataclass
class Case:
    name: str
    mask: np.ndarray
    winner: Tuple[int, int]                       # a pixel (y, x) of the kept component
    rivals: List[Tuple[int, int]] = field(default_factory=list)   # pixels of the runners-up
    tie: bool = False                             # the rivals have the winner's area (else a smaller one)
    kinds: Dict[Tuple[int, int], str] = field(default_factory=dict)  # pixel → "open" | "closed"
    winner_root_smaller: Optional[bool] = None    # against every rival
    area: Optional[int] = None                    # the winner's
    rival_area: Optional[int] = None
    root_far_from_area: bool = False              # winner and rivals: root's tile ≠ the tile with most area
    min_tiles: int = 0                            # winner and rivals each meet at least this many tiles
    open_per_tile: Optional[int] = None           # every tile has exactly this many open components
    min_root: Optional[int] = None                # the winner's root is at least this
    max_root: Optional[int] = None
    entries: Optional[int] = None                 # expected counts[image]


def _tile_id(y, x, w):
    return (y // TW) * ((w + TW - 1) // TW) + x // TW


def check_claims(case: Case) -> Components:
    """Asserts every property the case claims, from the reference alone."""
    m = case.mask
    h, w = m.shape
    c = components(m)
    lw = int(c.lab[case.winner])
    assert lw and lw == c.best, (case.name, "the claimed winner is not kept")
    rl = [int(c.lab[p]) for p in case.rivals]
    assert all(rl) and len(set(rl + [lw])) == len(rl) + 1, (case.name, "rivals are not distinct components")
    if case.tie:
        assert c.tied == len(rl) + 1 and all(c.area[r] == c.area[lw] for r in rl), (case.name, "no tie")
    else:
        assert c.tied == 1, (case.name, "unexpected tie")
        others = np.delete(c.area, [0, lw])
        assert others.size == 0 or others.max() < c.area[lw]
        if rl:
            assert all(c.area[r] == others.max() for r in rl), (case.name, "rivals are not the runners-up")
    if case.area is not None:
        assert c.area[lw] == case.area, (case.name, int(c.area[lw]))
    if case.rival_area is not None:
        assert all(c.area[r] == case.rival_area for r in rl), case.name
    for p, kind in case.kinds.items():
        assert is_open(m, int(c.lab[p]), c) == (kind == "open"), (case.name, p, kind)
    if case.winner_root_smaller is not None:
        for r in rl:
            assert (c.root[lw] < c.root[r]) == case.winner_root_smaller, (case.name, "root order")
    for lb in [lw] + rl if (case.root_far_from_area or case.min_tiles) else []:
        ys, xs = np.nonzero(c.lab == lb)
        per_tile = np.bincount(_tile_id(ys, xs, w))
        assert np.count_nonzero(per_tile) >= case.min_tiles, (case.name, "tiles met")
        if case.root_far_from_area:
            G = int(c.root[lb])
            yb, xb = divmod(G >> 1, (w + 1) // 2)
            root_tile = _tile_id(2 * yb + (G & 1), 2 * xb, w)
            assert root_tile != int(np.argmax(per_tile)) and 2 * per_tile[root_tile] < per_tile.sum(), case.name
    if case.open_per_tile is not None:
        _, opened = tile_entries(m)
        assert (opened == case.open_per_tile).all(), (case.name, opened)
    if case.min_root is not None:
        assert c.root[lw] >= case.min_root, (case.name, int(c.root[lw]))
    if case.max_root is not None:
        assert c.root[lw] <= case.max_root, (case.name, int(c.root[lw]))
    if case.entries is not None:
        assert expected_entries(m) == case.entries, (case.name, expected_entries(m))
    # the two statements of the tie key agree: the root's block is the first block
    assert np.array_equal(c.root[1:] >> 1, c.first[1:]), case.name
    return c


def _tie_open_closed(open_first: bool) -> Case:
    """A 3×4 closed rectangle and a 3×4 open one (over the border between tile
    columns 0 and 1, so its two entries meet in K2-K4), areas 12 and 12; the
    earlier rows hold the one with the smaller root.  Two smaller specks."""
    m = np.zeros((70, 140), bool)
    yo, yc = (2, 10) if open_first else (10, 2)
    m[yo:yo + 3, 62:66] = True
    m[yc:yc + 3, 10:14] = True
    m[40:42, 100:103] = True
    m[66:69, 63:65] = True                       # open, over a border of the second tile row
    po, pc = (yo, 62), (yc, 10)
    return Case("tie_open_first" if open_first else "tie_closed_first", m,
                winner=po if open_first else pc, rivals=[pc if open_first else po], tie=True,
                kinds={po: "open", pc: "closed"}, winner_root_smaller=True, area=12)


def tie_open_first() -> Case:
    return _tie_open_closed(True)


def tie_closed_first() -> Case:
    return _tie_open_closed(False)


def tie_open_open_merged() -> Case:
    """Two components of area 1141 each over three tiles.  A: a two-pixel lead
    ending on the last pixel (63, 63) of tile (0, 0), touching the body in
    tile (1, 1) through the corner only; the body runs on into tile (1, 2).
    B: a lead ending on (63, 192), the first column of tile (0, 3), touching
    through the other kind of corner its body at (64, 191) in tile (1, 2),
    which runs down into tile (2, 2).  Each root is the lead's first pixel."""
    m = np.zeros((200, 300), bool)
    m[62, 62] = m[63, 63] = True
    m[64:81, 64:131] = True                      # 17 × 67
    m[62, 193] = m[63, 192] = True
    m[64:131, 175:192] = True                    # 67 × 17
    m[150:160, 20:40] = True                     # smaller, closed
    return Case("tie_open_open_merged", m, winner=(62, 62), rivals=[(62, 193)], tie=True,
                kinds={(62, 62): "open", (62, 193): "open"}, winner_root_smaller=True, area=1141,
                root_far_from_area=True, min_tiles=3)


def max_closed(open_area: int = 3844) -> Case:
    """The largest closed component, 62×62 at offset (1, 1) of tile (0, 1)
    (in-tile bbox 1..62 in x and y, the widest the closed key holds), against
    an open 31×124 bar over three tiles of the second tile row (the larger
    root).  open_area 3844: a tie, the closed one wins; 3845: the open one."""
    assert open_area in (3844, 3845)
    m = np.zeros((128, 192), bool)
    m[1:63, 65:127] = True
    m[70:101, 10:134] = True
    pc, po = (1, 65), (70, 10)
    if open_area == 3845:
        m[101, 10] = True
        return Case("max_closed_open_wins", m, winner=po, rivals=[pc], kinds={po: "open", pc: "closed"},
                    winner_root_smaller=False, area=3845, rival_area=3844)
    return Case("max_closed", m, winner=pc, rivals=[po], tie=True, kinds={po: "open", pc: "closed"},
                winner_root_smaller=True, area=3844)


def ring_tile(shifted: bool = False) -> np.ndarray:
    """64×64: the alternating pattern on the tile's ring, 32 pixels on the top
    row, 31 on the right column, 31 on the bottom row and 30 on the left
    column, no two of them 8-adjacent: 124 open components.  `shifted` moves
    the pattern one pixel along every edge (it then holds three corners)."""
    t = np.zeros((TW, TW), bool)
    if not shifted:
        t[0, 0:63:2] = True                      # columns 0 .. 62
        t[2:63:2, 63] = True                     # rows 2 .. 62
        t[63, 1:62:2] = True                     # columns 1 .. 61
        t[2:61:2, 0] = True                      # rows 2 .. 60
    else:
        t[0, 1:64:2] = True                      # columns 1 .. 63
        t[3:64:2, 63] = True                     # rows 3 .. 63
        t[63, 0:61:2] = True                     # columns 0 .. 60
        t[3:62:2, 0] = True                      # rows 3 .. 61
    return t


def ring(tiles: int = 3, shifted: bool = False) -> Case:
    """The ring pattern in every tile of a tiles×tiles-tile image: 124 open
    components per tile taken alone.  Neighbouring rings touch across every
    border (k_ccl_border's skipped-pair rule sees alternating roots) and merge
    into zigzag chains of up to 64 pixels along the horizontal borders; a
    closed 9×9 blob inside the middle tile is larger than any of them, so the
    winner is unique."""
    m = np.tile(ring_tile(shifted), (tiles, tiles))
    c0 = (tiles // 2) * TW
    m[c0 + 20:c0 + 29, c0 + 20:c0 + 29] = True
    name = "ring%d%s" % (tiles, "_shifted" if shifted else "")
    return Case(name, m, winner=(c0 + 20, c0 + 20), kinds={(c0 + 20, c0 + 20): "closed"}, area=81, open_per_tile=124,
                entries=124 * tiles * tiles)


def designed_cases() -> List[Case]:
    return [tie_open_first(), tie_closed_first(), tie_open_open_merged(), max_closed(3844), max_closed(3845),
            ring(3), ring(3, shifted=True), ring(1), ring(1, shifted=True)]


# --------------------------------------------------------------------------- all-open mode

def _specks(m: np.ndarray, rng, n: int, keep_out: List[Tuple[int, int, int, int]]) -> None:
    """n random rectangles of 1..3 × 1..3 pixels, none within 4 pixels of the
    (y0, x0, y1, x1) windows of keep_out."""
    h, w = m.shape
    ys, xs = rng.integers(0, h - 3, n), rng.integers(0, w - 3, n)
    hh, ww = rng.integers(1, 4, n), rng.integers(1, 4, n)
    ok = np.ones(n, bool)
    for (y0, x0, y1, x1) in keep_out:
        ok &= ~((ys + 3 >= y0 - 4) & (ys <= y1 + 4) & (xs + 3 >= x0 - 4) & (xs <= x1 + 4))
    for k in range(3):
        for j in range(3):
            sel = ok & (hh > k) & (ww > j)
            m[ys[sel] + k, xs[sel] + j] = True


def big_closed_limit() -> Case:
    """4096×4096: 2·wb·hb = 2^23 slots exactly, the last image on the closed
    path.  The kept component is a 1×51 bar on row 4094 of the last tile (a
    component with a pixel on rows 4092-4093 has its root in block row 2046,
    at least 4097 below the top of the field), closed, with its root 56
    below 2^23: the key's 23-bit field ~G holds 55.  The runner-up (area 50)
    covers rows 4092-4094 of the tile before; a decoy of area 49 sits in the
    first tile with root 3 (field value near its maximum), and sparse specks
    fill the frame."""
    h = w = 4096
    m = np.zeros((h, w), bool)
    win, second, decoy = (4094, 4040, 4095, 4091), (4092, 3980, 4095, 4000), (1, 2, 8, 9)
    _specks(m, np.random.default_rng(4096), 6000, [win, second, decoy])
    m[4094, 4040:4091] = True                    # 51
    m[4092:4094, 3980:4000] = True               # 40 + 10
    m[4094, 3980:3990] = True
    m[1:8, 2:9] = True                           # 49
    return Case("big_closed_limit", m, winner=(4094, 4040), rivals=[(4092, 3980)],
                kinds={(4094, 4040): "closed", (4092, 3980): "closed", (1, 2): "closed"},
                winner_root_smaller=False, area=51, rival_area=50,
                min_root=CLOSED_SLOTS - 300, max_root=CLOSED_SLOTS - 1)


ALL_OPEN_SHAPE = (4097, 4099)                    # h, w: 8 400 900 slots, the first sizes past 2^23


def big_all_open() -> Case:
    """4097×4099, all-open mode.  Kept: a 3×51 bar on rows 4092-4094 (tile row
    63, lanes 60-62) inside tile column 31, on no tile edge, root ≥ 2^23; an
    equal bar in tile column 47 loses the tie by its larger root.  The kept
    bar's tile holds other components.  Tile (10, 20) holds the even grid
    (more than 1000 components from one tile) with its 3-pixel component; a
    2×70 bar over the corner of four tiles (area 140) must lose; sparse
    specks elsewhere."""
    h, w = ALL_OPEN_SHAPE
    m = np.zeros((h, w), bool)
    win, tied = (4092, 1990, 4095, 2041), (4092, 3010, 4095, 3061)
    gy, gx = 10 * TW, 20 * TW
    _specks(m, np.random.default_rng(4097), 6000, [win, tied, (gy, gx, gy + TW, gx + TW), (1023, 990, 1025, 1060)])
    m[4092:4095, 1990:2041] = True               # 153, kept
    m[4092:4095, 3010:3061] = True               # 153, the larger root
    m[4040:4043, 1990:1993] = True               # the kept bar's tile: other components
    m[4050, 2000:2030] = True
    m[4060:4070:2, 2010:2040:2] = True
    m[gy:gy + TW:2, gx:gx + TW:2] = True
    m[gy + 36, gx + 37] = m[gy + 37, gx + 38] = True
    m[1023:1025, 990:1060] = True                # 140 over four tiles
    return Case("big_all_open", m, winner=(4092, 1990), rivals=[(4092, 3010)], tie=True,
                kinds={(4092, 1990): "closed", (4092, 3010): "closed", (1023, 990): "open"},
                winner_root_smaller=True, area=153, min_root=CLOSED_SLOTS)


# --------------------------------------------------------------------------- fuzz

FUZZ_SEED = 20
FUZZ_N = 256
_FUZZ_SIZES = np.concatenate([np.arange(1, 201), np.repeat([63, 64, 65, 127, 128, 129], 12)])


def fuzz_masks(seed: int = FUZZ_SEED, n: int = FUZZ_N) -> List[np.ndarray]:
    """n masks, h and w from 1..200 weighted towards the tile sizes ± 1,
    densities 0.02..0.7; every fourth is a few rectangles of few distinct
    sizes, so exact area ties between the largest components are common."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        h, w = (int(v) for v in rng.choice(_FUZZ_SIZES, 2))
        if i % 4 == 3:
            m = np.zeros((h, w), bool)
            rh, rw = int(rng.integers(1, 6)), int(rng.integers(1, 9))
            for _ in range(int(rng.integers(2, 9))):
                y, x = int(rng.integers(0, h)), int(rng.integers(0, w))
                if rng.random() < 0.7:
                    m[y:y + rh, x:x + rw] = True
                else:
                    m[y:y + rw, x:x + rh] = True
        else:
            m = rng.random((h, w)) < rng.uniform(0.02, 0.7)
        out.append(m)
    return out
