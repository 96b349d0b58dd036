"""Truths for polygon locations (PCV_SHAPE_POLYGON).

Two restatements of the two rules:
  * numpy, in the stated operation order. numpy's f64 arithmetic rounds every operation on its own (no contraction), so these
    are what the library's host twins and kernels must give BIT FOR BIT;
  * exact rational arithmetic (fractions), which says what the polygon really contains and how far a point is from the nearest
    crossing, so the f64 rule can be held to it away from the edges.
"""
from fractions import Fraction

import numpy as np


def as_rings(rings):
    if isinstance(rings, np.ndarray) and rings.ndim == 2:
        rings = [rings]
    return [np.asarray(r, dtype=np.float64).reshape(-1, 2) for r in rings]


def segments(rings):
    """Every edge a -> b as given: (n, 4) of ax, ay, bx, by."""
    out = []
    for r in as_rings(rings):
        out.append(np.concatenate([r, np.roll(r, -1, axis=0)], axis=1))
    return np.concatenate(out)


def edge_table(rings):
    """The point rule's table: horizontal edges dropped, each other edge from its lower endpoint: lx, ly, uy, slope."""
    s = segments(rings)
    s = s[s[:, 1] != s[:, 3]]
    up = s[:, 1] < s[:, 3]
    lx, ly = np.where(up, s[:, 0], s[:, 2]), np.where(up, s[:, 1], s[:, 3])
    ux, uy = np.where(up, s[:, 2], s[:, 0]), np.where(up, s[:, 3], s[:, 1])
    with np.errstate(all="ignore"):
        slope = (ux - lx) / (uy - ly)
    return lx, ly, uy, slope


def inside(rings, px, py):
    """Parity of the edges with ly <= py && py < uy && px < lx + (py - ly) * slope."""
    px, py = np.asarray(px, dtype=np.float64), np.asarray(py, dtype=np.float64)
    parity = np.zeros(px.shape, dtype=bool)
    with np.errstate(all="ignore"):
        for lx, ly, uy, slope in zip(*edge_table(rings)):
            t = (py - ly) * slope
            parity ^= (ly <= py) & (py < uy) & (px < lx + t)
    return parity


def contains(rings, x, y, z, z_min=-np.inf, z_max=np.inf):
    """The xy frame's point rule."""
    z = np.asarray(z, dtype=np.float64)
    return inside(rings, x, y) & (z_min <= z) & (z <= z_max)


def contains_web_mercator(rings, u, v):
    """The web-mercator frame's point rule on the projected points (pcv.wmr_project)."""
    return inside(rings, u, v)


def _side(ax, ay, bx, by, cx, cy):
    return (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)


def intersects_cubes(rings, cubes, z_min=-np.inf, z_max=np.inf):
    """The xy frame's node rule for (m, 4) cubes: min xyz, edge."""
    cubes = np.asarray(cubes, dtype=np.float64).reshape(-1, 4)
    x0, y0, zl, e = cubes[:, 0], cubes[:, 1], cubes[:, 2], cubes[:, 3]
    x1, y1, zh = x0 + e, y0 + e, zl + e
    hit = inside(rings, x0, y0)
    for ax, ay, bx, by in segments(rings):
        overlap = (min(ax, bx) <= x1) & (max(ax, bx) >= x0) & (min(ay, by) <= y1) & (max(ay, by) >= y0)
        s = [_side(ax, ay, bx, by, cx, cy) for cx, cy in ((x0, y0), (x1, y0), (x0, y1), (x1, y1))]
        all_pos = (s[0] > 0) & (s[1] > 0) & (s[2] > 0) & (s[3] > 0)
        all_neg = (s[0] < 0) & (s[1] < 0) & (s[2] < 0) & (s[3] < 0)
        hit |= overlap & ~(all_pos | all_neg)
    return hit & (z_min <= zh) & (z_max >= zl)


def bounding_rect(rings):
    """("web_mercator_rect", (min x, min y), (max x, max y)) over the vertices: a web-mercator polygon's nodes and cells."""
    v = np.concatenate(as_rings(rings))
    return ("web_mercator_rect", v.min(axis=0), v.max(axis=0))


# ---- exact --------------------------------------------------------------------------------------------------------------
def exact_inside(rings, px, py):
    """(inside, distance): the even-odd verdict of the half-open rule in rational arithmetic, and the smallest horizontal distance
    from the point to a crossing of its scanline with an edge (None when the scanline meets no edge)."""
    px, py = Fraction(float(px)), Fraction(float(py))
    parity, dist = False, None
    for ax, ay, bx, by in segments(rings):
        if ay == by:
            continue
        (lx, ly), (ux, uy) = ((ax, ay), (bx, by)) if ay < by else ((bx, by), (ax, ay))
        lx, ly, ux, uy = Fraction(float(lx)), Fraction(float(ly)), Fraction(float(ux)), Fraction(float(uy))
        if not (ly <= py < uy):
            continue
        xc = lx + (py - ly) * (ux - lx) / (uy - ly)
        parity ^= px < xc
        d = abs(px - xc)
        dist = d if dist is None or d < dist else dist
    return parity, dist


def extent(rings):
    v = np.concatenate(as_rings(rings))
    return float(max(v[:, 0].max() - v[:, 0].min(), v[:, 1].max() - v[:, 1].min()))


# ---- shapes -------------------------------------------------------------------------------------------------------------
def regular(n, cx, cy, r, phase=0.0):
    a = phase + 2.0 * np.pi * np.arange(n) / n
    return np.stack([cx + r * np.cos(a), cy + r * np.sin(a)], axis=1)


def star(n, cx, cy, r_out, r_in, phase=0.1):
    """n vertices alternating between two radii (n odd: the last two are both outer)."""
    a = phase + 2.0 * np.pi * np.arange(n) / n
    r = np.where(np.arange(n) % 2 == 0, r_out, r_in)
    return np.stack([cx + r * np.cos(a), cy + r * np.sin(a)], axis=1)


def cpu_shapes():
    """name -> rings: the shapes of tests/test_polygon_cpu.py."""
    tri = np.array([[1.0, 1.0], [9.0, 2.0], [4.0, 8.0]])
    ell = np.array([[0.0, 0.0], [8.0, 0.0], [8.0, 3.0], [3.0, 3.0], [3.0, 9.0], [0.0, 9.0]])
    sq = np.array([[0.0, 0.0], [10.0, 0.0], [10.0, 10.0], [0.0, 10.0]])
    hole = np.array([[3.0, 3.0], [7.0, 3.0], [7.0, 7.0], [3.0, 7.0]])
    quad = np.array([[0.5, 0.25], [7.75, 1.5], [9.25, 8.5], [1.5, 6.75]])
    return {
        "triangle": [tri],
        "concave_l": [ell],
        "square_with_hole": [sq, hole],
        "two_rings": [np.array([[0.0, 0.0], [4.0, 0.5], [3.0, 4.0]]), np.array([[6.0, 5.0], [9.5, 5.5], [8.0, 9.0], [5.5, 8.0]])],
        "ccw": [quad],
        "cw": [quad[::-1].copy()],
        "horizontal_edges": [np.array([[1.0, 2.0], [4.0, 2.0], [4.0, 5.0], [7.0, 5.0], [7.0, 2.0], [9.0, 2.0], [9.0, 8.0], [1.0, 8.0]])],
        "star_257": [star(257, 5.0, 5.0, 4.9, 2.1)],
    }


def fan_tiling():
    """The square [0, 8]^2 cut into a triangle fan around (3, 5): (outline rings, list of pieces)."""
    c = [3.0, 5.0]
    rim = [[0.0, 0.0], [4.0, 0.0], [8.0, 0.0], [8.0, 4.0], [8.0, 8.0], [2.0, 8.0], [0.0, 8.0], [0.0, 3.0]]
    pieces = []
    for k in range(len(rim)):
        a, b = rim[k], rim[(k + 1) % len(rim)]
        tri = np.array([c, a, b])
        pieces.append([tri if k % 2 == 0 else tri[::-1].copy()])  # mixed orientations
    return [np.array([[0.0, 0.0], [8.0, 0.0], [8.0, 8.0], [0.0, 8.0]])], pieces


def l_tiling():
    """An L and its complement in the square [0, 8]^2: (outline rings, [L, complement])."""
    ell = np.array([[0.0, 0.0], [8.0, 0.0], [8.0, 3.0], [3.0, 3.0], [3.0, 8.0], [0.0, 8.0]])
    rest = np.array([[8.0, 8.0], [3.0, 8.0], [3.0, 3.0], [8.0, 3.0]])
    return [np.array([[0.0, 0.0], [8.0, 0.0], [8.0, 8.0], [0.0, 8.0]])], [[ell], [rest]]


def planted_points(rings, rng=None):
    """Points on every vertex, at every vertex's y level (at the other vertices' x and between), and the midpoints of the edges."""
    v = np.concatenate(as_rings(rings))
    xs, ys = [v[:, 0]], [v[:, 1]]
    ux = np.unique(np.concatenate([v[:, 0], (v[:-1, 0] + v[1:, 0]) / 2, [v[:, 0].min() - 1.0, v[:, 0].max() + 1.0]]))
    for y in np.unique(v[:, 1]):
        xs.append(ux)
        ys.append(np.full(ux.size, y))
    s = segments(rings)
    xs.append((s[:, 0] + s[:, 2]) / 2)
    ys.append((s[:, 1] + s[:, 3]) / 2)
    return np.concatenate(xs), np.concatenate(ys)
