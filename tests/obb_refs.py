"""CPU references of the oriented boxes (ipp_polygons_obb; the rule is stated
in include/ipp.h) and the rings shared by tests/test_obb_cpu.py and
tests/test_gpu_obb.py (not a test module).

``record`` is the rule in Python integers: a monotone-chain hull put into the
canonical order, the rectangle on every hull edge over every point, and the
cross-multiplied choice.  ``brute`` does not build a hull: every ordered pair
of distinct points is a candidate direction, admissible iff no point lies on
its left, and the least area is found with ``Fraction``.  ``wide_rings`` are
the rings on which the comparison needs its 128 bits."""
import functools
from fractions import Fraction
from math import gcd

import numpy as np

REC = 8
M64 = (1 << 64) - 1


def _cross(ux, uy, vx, vy):
    return ux * vy - uy * vx


def _points(ring):
    return [(int(x), int(y)) for x, y in np.asarray(ring).reshape(-1, 2)]


def hull(ring):
    """The strictly convex hull of the ring's point set in the canonical order:
    H[0] least in (y, x), then cross(H[e+1]-H[e], H[e+2]-H[e+1]) > 0."""
    pts = sorted(set(_points(ring)))
    if len(pts) <= 2:
        H = pts
    else:
        def chain(seq):
            out = []
            for p in seq:
                while len(out) >= 2 and _cross(out[-1][0] - out[-2][0], out[-1][1] - out[-2][1],
                                               p[0] - out[-1][0], p[1] - out[-1][1]) <= 0:
                    out.pop()
                out.append(p)
            return out
        lower, upper = chain(pts), chain(pts[::-1])
        H = lower[:-1] + upper[:-1]
        if len(H) == 2 and H[0] == H[1]:
            H = H[:1]
    k = min(range(len(H)), key=lambda i: (H[i][1], H[i][0]))
    H = H[k:] + H[:k]
    if len(H) >= 3:
        assert all(_cross(H[(e + 1) % len(H)][0] - H[e][0], H[(e + 1) % len(H)][1] - H[e][1],
                          H[(e + 2) % len(H)][0] - H[(e + 1) % len(H)][0],
                          H[(e + 2) % len(H)][1] - H[(e + 1) % len(H)][1]) > 0 for e in range(len(H)))
    return H


def edge_rect(a, b, pts):
    """(nn, lo, hi, hgt, least s) of the rectangle on the direction a -> b over pts."""
    dx, dy = b[0] - a[0], b[1] - a[1]
    ts = [dx * (x - a[0]) + dy * (y - a[1]) for x, y in pts]
    ss = [-dy * (x - a[0]) + dx * (y - a[1]) for x, y in pts]
    return dx * dx + dy * dy, min(ts), max(ts), max(ss), min(ss)


def choose(ring, truncate=False):
    """(e, record) of the ring by the rule; ``truncate``: the same choice with
    both compared products cut to their low 64 bits, what a 64-bit device
    comparison would compute (for ``wide_rings``)."""
    pts = _points(ring)
    H = hull(pts)
    m = len(H)
    if m == 1:
        return 0, [H[0][0], H[0][1], 0, 0, 0, 0, 0, 1]
    if m == 2:
        dx, dy = H[1][0] - H[0][0], H[1][1] - H[0][1]
        return 0, [H[0][0], H[0][1], dx, dy, 0, dx * dx + dy * dy, 0, 2]
    best = None
    for e in range(m):
        a, b = H[e], H[(e + 1) % m]
        nn, lo, hi, hgt, smin = edge_rect(a, b, pts)
        assert smin == 0 and lo <= 0 and hi >= nn and hgt > 0
        assert nn <= 1 << 29 and hi - lo <= 1 << 30 and hgt <= 1 << 29 and max(abs(lo), abs(hi)) <= 1 << 29
        if best is not None:
            l, r = (hi - lo) * hgt * best[1], (best[3] - best[2]) * best[4] * nn
            if truncate:
                l, r = l & M64, r & M64
        if best is None or l < r:
            best = (e, nn, lo, hi, hgt)
    e, nn, lo, hi, hgt = best
    a, b = H[e], H[(e + 1) % m]
    return e, [a[0], a[1], b[0] - a[0], b[1] - a[1], lo, hi, hgt, m]


def record(ring):
    """The 8 words {ax, ay, dx, dy, lo, hi, hgt, m} of the ring."""
    return choose(ring)[1]


def records(rings, live=None):
    """int32 (len, 8): ``record`` of every ring; the zero record where the ring is empty, None or not live."""
    out = np.zeros((len(rings), REC), np.int32)
    for i, r in enumerate(rings):
        if r is not None and len(r) and (live is None or live[i]):
            out[i] = record(r)
    return out


def area(rec):
    """The rectangle's area, exactly."""
    ax, ay, dx, dy, lo, hi, hgt, m = (int(v) for v in rec)
    return Fraction((hi - lo) * hgt, dx * dx + dy * dy) if m >= 2 else Fraction(0)


def corners(rec):
    """The four corners as exact Fractions, in the rule's order."""
    ax, ay, dx, dy, lo, hi, hgt, m = (int(v) for v in rec)
    nn = dx * dx + dy * dy
    return [(ax + Fraction(t * dx - s * dy, nn), ay + Fraction(t * dy + s * dx, nn))
            for t, s in ((lo, 0), (hi, 0), (hi, hgt), (lo, hgt))]


def _angle_key(d):
    """Sorts directions by their angle from +x towards +y (clockwise on the screen), exactly."""
    half = 0 if (d[1] > 0 or (d[1] == 0 and d[0] > 0)) else 1
    return half, functools.cmp_to_key(lambda u, v: -1 if _cross(u[0], u[1], v[0], v[1]) > 0 else
                                      1 if _cross(u[0], u[1], v[0], v[1]) < 0 else 0)(d)


def brute(ring):
    """(least area as a Fraction, record) without a hull: every ordered pair
    of distinct points as a direction (numpy int64: small rings only).  An
    admissible pair lies on a supporting line; it is moved to that line's
    extreme points (the hull edge it lies on), the edges are ordered by their
    direction's angle from the one that leaves the least (y, x) point, and ties
    in area go to the first."""
    pts = sorted(set(_points(ring)), key=lambda p: (p[1], p[0]))
    if len(pts) == 1:
        return Fraction(0), [pts[0][0], pts[0][1], 0, 0, 0, 0, 0, 1]
    P = np.array(pts, np.int64)
    D = P[None, :, :] - P[:, None, :]                                   # D[a, b] = P[b] - P[a]
    Q = P[None, None, :, :] - P[:, None, None, :]                       # Q[a, ., p] = P[p] - P[a]
    S = -D[:, :, None, 1] * Q[..., 0] + D[:, :, None, 0] * Q[..., 1]    # s of p for the direction a -> b
    ok = (S >= 0).all(axis=2)
    np.fill_diagonal(ok, False)
    if not (S[ok] > 0).any():                                           # collinear: both directions admissible
        a, b = pts[0], pts[-1]
        dx, dy = b[0] - a[0], b[1] - a[1]
        return Fraction(0), [a[0], a[1], dx, dy, 0, dx * dx + dy * dy, 0, 2]
    edges = {}
    for ia, ib in zip(*np.nonzero(ok)):
        a, b = pts[ia], pts[ib]
        on_line = [p for p, s in zip(pts, S[ia, ib]) if s == 0]
        dx, dy = b[0] - a[0], b[1] - a[1]
        on_line.sort(key=lambda p: dx * p[0] + dy * p[1])
        a, b = on_line[0], on_line[-1]
        nn, lo, hi, hgt, _ = edge_rect(a, b, pts)
        edges[(a, b)] = (Fraction((hi - lo) * hgt, nn), [a[0], a[1], b[0] - a[0], b[1] - a[1], lo, hi, hgt])
    order = sorted(edges, key=lambda ab: _angle_key((ab[1][0] - ab[0][0], ab[1][1] - ab[0][1])))
    assert order[0][0] == pts[0]                                        # the first edge leaves the least (y, x) point
    least = min(edges[k][0] for k in order)
    first = [k for k in order if edges[k][0] == least][0]
    return least, edges[first][1] + [len(order)]


# --- rings ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def wide_rings(count=24, seed=1729):
    """Seeded rings of 3..7 points within 40 of the corners of the 0..16384
    lattice: edges of nn near 2^28..2^29 and rectangles near 2^58, so the
    compared products pass 2^64 by far.  Demonstrated here, on the CPU: cut to
    64 bits, the comparison picks a different edge on at least one of them
    (in fact on many)."""
    rng = np.random.default_rng(seed)
    rings = []
    while len(rings) < count:
        n = int(rng.integers(3, 8))
        near = rng.integers(0, 41, size=(n, 2))
        far = rng.integers(0, 2, size=(n, 2)).astype(bool)
        p = np.where(far, 16384 - near, near).astype(np.int32)
        if len(hull(p)) >= 3:
            rings.append(p)
    wrong = [i for i, r in enumerate(rings) if choose(r, truncate=True)[0] != choose(r)[0]]
    assert wrong, "no wide ring tells the 128-bit comparison from a 64-bit one: the set is wrong"
    assert any((area_products(r) >> 64) > 0 for r in rings)
    return tuple(rings), tuple(wrong)


def area_products(ring):
    """The largest product (hi-lo)·hgt·nn' the choice compares on this ring."""
    pts = _points(ring)
    H = hull(pts)
    rects = [edge_rect(H[e], H[(e + 1) % len(H)], pts) for e in range(len(H))]
    return max((r[2] - r[1]) * r[3] for r in rects) * max(r[0] for r in rects)


def two_columns(rows, x0=3, x1=11, y0=0):
    """2·rows points: columns x0 and x1 over lattice rows y0 .. y0 + rows - 1, the left column going down and
    the right one coming back up."""
    ys = np.arange(y0, y0 + rows)
    return np.concatenate([np.stack([np.full(rows, x0), ys], 1), np.stack([np.full(rows, x1), ys[::-1]], 1)]).astype(
        np.int32)


def chain_ring(length, mirror=False):
    """A strictly convex ring of `length` vertices whose right monotone chain
    (mirror: its left one) holds all of them: from the top vertex, the length - 1
    shortest primitive vectors with dy > 0 in the order of their angle, closed
    by one straight edge back to the top."""
    vecs = sorted(((dx, dy) for dy in range(1, 41) for dx in range(-40, 41) if gcd(abs(dx), dy) == 1),
                  key=lambda v: (v[0] * v[0] + v[1] * v[1], v))[:length - 1]
    assert len(vecs) == length - 1
    vecs.sort(key=lambda v: -Fraction(v[0], v[1]))                     # +x first, turning towards -x
    p = np.concatenate([[(0, 0)], np.cumsum(np.array(vecs, np.int64), axis=0)])
    p[:, 0] -= p[:, 0].min()
    if mirror:
        p[:, 0] = p[:, 0].max() - p[:, 0]
    assert p.min() >= 0 and p.max() <= 16384
    return p.astype(np.int32)


def chain_ring_popped(length):
    """``chain_ring(length)`` and one far point on its last row: pushed last, it drops most of the right chain."""
    p = chain_ring(length)
    return np.concatenate([p, [(16384, int(p[:, 1].max()))]]).astype(np.int32)
