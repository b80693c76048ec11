"""CPU references of the polygon simplification (ipp_polygons_simplify; the
rule is stated in include/ipp.h) and the rings shared by
tests/test_simplify_cpu.py and tests/test_gpu_simplify.py (not a test module).

``simplify`` is the RECURSIVE form (an explicit stack) in Python integers.
``simplify_levels`` restates it level by level in numpy int64: every open
segment is split once per round, as the device does."""
import numpy as np

EPS_QS = (1, 4, 6, 16, 4096)


def _cross(pa, pb, pj):
    return (pb[0] - pa[0]) * (pj[1] - pa[1]) - (pb[1] - pa[1]) * (pj[0] - pa[0])


def _d2(p, q):
    return (p[0] - q[0]) ** 2 + (p[1] - q[1]) ** 2


def anchor_b(P):
    """Index in 1..n-1 farthest from P[0], ties to the least index."""
    best, B = -1, 0
    for j in range(1, len(P)):
        d = _d2(P[j], P[0])
        if d > best:
            best, B = d, j
    return B


def simplify(ring, eps_q, triangle=True):
    """Kept indices (ascending, from 0) of the ring (n, 2) at tolerance eps_q
    quarter pixels; ``triangle=False`` leaves out the rule's last step (the
    third vertex of a ring that kept its anchors alone)."""
    P = [(int(x), int(y)) for x, y in np.asarray(ring).reshape(-1, 2)]
    n = len(P)
    assert 1 <= eps_q <= 4096
    if n < 3:
        return list(range(n))
    Q = P + [P[0]]
    B = anchor_b(P)
    keep = {0, B}
    stack = [(0, B), (B, n)]
    e2 = eps_q * eps_q
    while stack:
        a, b = stack.pop()
        if b <= a + 1:
            continue
        len2 = _d2(Q[b], Q[a])
        best, c = -1, a
        for j in range(a + 1, b):
            m = abs(_cross(Q[a], Q[b], Q[j])) if len2 > 0 else _d2(Q[j], Q[a])
            if m > best:
                best, c = m, j
        split = 16 * best * best > e2 * len2 if len2 > 0 else 16 * best > e2
        if split:
            keep.add(c)
            stack.append((a, c))
            stack.append((c, b))
    if len(keep) == 2 and triangle:
        best, c = 0, None
        for j in range(n):
            m = abs(_cross(P[0], P[B], P[j]))
            if m > best:
                best, c = m, j
        if c is not None:
            keep.add(c)
    return sorted(keep)


def simplify_levels(ring, eps_q):
    """The same kept indices, level by level: per round one vectorised pass over
    the open vertices, a per-segment arg-max of (measure, least index), and a
    move of every vertex to its half.  Also returns the number of rounds."""
    P = np.asarray(ring, np.int64).reshape(-1, 2)
    n = len(P)
    if n < 3:
        return list(range(n)), 0
    Q = np.concatenate([P, P[:1]])
    d2 = ((P - P[0]) ** 2).sum(1)
    d2[0] = -1
    B = int(np.argmax(d2))                       # the first maximum
    idx = np.arange(n)
    a = np.where(idx < B, 0, B)
    b = np.where(idx < B, B, n)
    kept = np.zeros(n, bool)
    kept[[0, B]] = True
    opened = ~kept
    e2 = eps_q * eps_q
    rounds = 0
    while opened.any():
        rounds += 1
        j = idx[opened]
        aj, bj = a[j], b[j]
        va, vj = Q[bj] - Q[aj], Q[j] - Q[aj]
        len2 = (va ** 2).sum(1)
        m = np.where(len2 > 0, np.abs(va[:, 0] * vj[:, 1] - va[:, 1] * vj[:, 0]), (vj ** 2).sum(1))
        # per segment (its left end names it): the largest measure, then the least index
        order = np.lexsort((j, -m, aj))
        first = np.ones(len(j), bool)
        first[1:] = aj[order][1:] != aj[order][:-1]
        win_m, win_j = np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64)
        win_m[aj[order][first]] = m[order][first]
        win_j[aj[order][first]] = j[order][first]
        wm, wj = win_m[aj], win_j[aj]
        split = np.where(len2 > 0, 16 * wm * wm > e2 * len2, 16 * wm > e2)
        opened[j[~split]] = False
        won = split & (j == wj)
        kept[j[won]] = True
        opened[j[won]] = False
        left, right = split & (j < wj), split & (j > wj)
        b[j[left]] = wj[left]
        a[j[right]] = wj[right]
    if kept.sum() == 2:
        cr = np.abs((P[B, 0] - P[0, 0]) * (P[:, 1] - P[0, 1]) - (P[B, 1] - P[0, 1]) * (P[:, 0] - P[0, 0]))
        if cr.max() > 0:
            kept[int(np.argmax(cr))] = True
    return idx[kept].tolist(), rounds


def apply(poly, eps_q):
    """The simplified polygon (V', 2) int32 of a traced polygon, or None."""
    if poly is None:
        return None
    poly = np.asarray(poly, np.int32).reshape(-1, 2)
    return poly[simplify(poly, eps_q)]


def spanning_error_ok(ring, kept, eps_q):
    """Every dropped vertex lies within eps of the kept segment that spans it:
    16·cross² <= eps_q²·len2 in exact integers (with len2 = 0, 16·d² <= eps_q²)."""
    P = [(int(x), int(y)) for x, y in np.asarray(ring).reshape(-1, 2)]
    n = len(P)
    Q = P + [P[0]]
    ends = list(kept) + [n]
    for a, b in zip(ends[:-1], ends[1:]):
        len2 = _d2(Q[b], Q[a])
        for j in range(a + 1, b):
            if len2 > 0:
                c = _cross(Q[a], Q[b], Q[j])
                if 16 * c * c > eps_q * eps_q * len2:
                    return False
            elif 16 * _d2(Q[j], Q[a]) > eps_q * eps_q:
                return False
    return True


# --- rings ------------------------------------------------------------------------------------------------
def random_small_rings(count=2000, seed=20251):
    """Seeded rings of 3..40 points on the 0..4 lattice: ties, repeated points and collinear runs abound."""
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 5, size=(int(rng.integers(3, 41)), 2)).astype(np.int32) for _ in range(count)]


def pinch_ring():
    """Two diamonds sharing the corner (4, 4), which the ring visits twice and
    starts at: P[4] = P[0] = P[n].  (A segment's winner never coincides with
    one of its ends unless every measure is 0, so len2 = 0 itself is reached
    only by a ring whose points all coincide: ``degenerate_rings``.)"""
    return np.array([(4, 4), (6, 2), (8, 4), (6, 6), (4, 4), (2, 6), (0, 4), (2, 2)], np.int32)


def degenerate_rings():
    """Rings that exercise repeated points, len2 = 0 (all points coincide), zero area and n < 3."""
    return [pinch_ring(),
            np.array([(4, 4), (2, 6), (0, 4), (2, 2), (4, 4), (6, 2), (8, 4), (6, 6)], np.int32),
            np.array([(1, 1), (1, 1), (1, 1), (1, 1)], np.int32),                    # one point: B = 1, no triangle
            np.array([(0, 0), (2, 2), (4, 4), (3, 3), (1, 1)], np.int32),            # collinear: zero area, 2 kept
            np.array([(0, 0), (3, 0), (0, 0), (0, 3), (0, 0), (3, 3)], np.int32),    # P[0] revisited twice
            np.array([(5, 7)], np.int32).reshape(1, 2),
            np.array([(5, 7), (9, 1)], np.int32)]


def extreme_rings(seed=7):
    """Rings whose points sit on and near the corners of the 0..16384 lattice (the overflow bounds)."""
    rng = np.random.default_rng(seed)
    out = [np.array([(0, 0), (16384, 0), (16384, 16384), (0, 16384)], np.int32),
           np.array([(0, 0), (16384, 16384), (16384, 0), (0, 16384), (8192, 8191)], np.int32)]
    for _ in range(6):
        n = int(rng.integers(5, 60))
        p = rng.choice(np.array([0, 1, 2, 8191, 8192, 16382, 16383, 16384]), size=(n, 2))
        out.append(p.astype(np.int32))
    return out


def random_large_ring(n, seed, span=300):
    """A jittered circle-like ring of n points: many levels, many ties."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) * (2 * np.pi / n)
    r = span + rng.integers(-12, 13, size=n)
    return np.stack([np.rint(2 * span + r * np.cos(t)), np.rint(2 * span + r * np.sin(t))], 1).astype(np.int32)


def comb(teeth):
    """A bar of 2·teeth − 1 pixels with a 1-px tooth over every other pixel: its outline has 4·teeth vertices."""
    m = np.zeros((2, 2 * teeth - 1), bool)
    m[1, :] = True
    m[0, ::2] = True
    return m


def synthetic(rings):
    """(verts (sum n, 2) int32, offsets int64, hdr (len, 8) int32) of rings fed directly to the entries."""
    nv = np.array([len(r) for r in rings], np.int64)
    offsets = np.concatenate([[0], np.cumsum(nv)[:-1]]).astype(np.int64)
    hdr = np.zeros((len(rings), 8), np.int32)
    hdr[:, 3] = nv
    verts = np.concatenate([np.asarray(r, np.int32).reshape(-1, 2) for r in rings]) if len(rings) else \
        np.zeros((0, 2), np.int32)
    return verts, offsets, hdr
