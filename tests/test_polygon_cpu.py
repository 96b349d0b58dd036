"""Polygon locations on the host (PCV_SHAPE_POLYGON): the library's host twins against the numpy restatement of the
two rules bit for bit, the f64 rule against exact rational arithmetic away from the edges, the tiling property, the superset
property of the node rule, the web-mercator frame and every message of the validation. No device."""
from fractions import Fraction

import numpy as np
import pytest

import point_cloud_viewer_amd as pcv
import polygon_truth as P

SHAPES = P.cpu_shapes()
# the uniform points' seed: with it the share of points within 1e-9 of the extent of a crossing is far below the 1 % cap for
# every shape (a margin of 1e-9 x 10 around some hundreds of edges covers ~1e-7 of the square; the cap guards the test, not the code)
SEED = 20240607


def uniform_points(n=20000, lo=-1.0, hi=11.0):
    rng = np.random.Generator(np.random.PCG64(SEED))
    return rng.uniform(lo, hi, n), rng.uniform(lo, hi, n), rng.uniform(-5.0, 5.0, n)


def all_points(rings):
    ux, uy, uz = uniform_points()
    px, py = P.planted_points(rings)
    return np.concatenate([ux, px]), np.concatenate([uy, py]), np.concatenate([uz, np.zeros(px.size)])


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_contains_twin_equals_the_numpy_restatement(name):
    rings = SHAPES[name]
    x, y, z = all_points(rings)
    for z_min, z_max in ((-np.inf, np.inf), (-1.5, 2.25), (2.0, -2.0), (np.nan, 1.0)):
        got = pcv.polygon_contains(rings, x, y, z, z_min=z_min, z_max=z_max).astype(bool)
        want = P.contains(rings, x, y, z, z_min, z_max)
        assert np.array_equal(got, want), (name, z_min, np.nonzero(got != want)[0][:5])
        if z_min != z_min or z_min > z_max:
            assert not got.any()
    inside = pcv.polygon_contains(rings, x, y, z).astype(bool)
    assert 0.05 < inside[:20000].mean() < 0.95, name


def test_both_orientations_give_the_same_flags():
    x, y, z = all_points(SHAPES["ccw"])
    assert np.array_equal(pcv.polygon_contains(SHAPES["ccw"], x, y, z), pcv.polygon_contains(SHAPES["cw"], x, y, z))


def test_integer_points_on_horizontal_and_shared_edges():
    """Exact by construction: integer coordinates, so the rule's arithmetic does not round. The half-open rule keeps a point on a
    left or bottom edge and drops one on a right or top edge."""
    sq = [np.array([[0.0, 0.0], [10.0, 0.0], [10.0, 10.0], [0.0, 10.0]])]
    xs, ys = np.meshgrid(np.arange(-1.0, 12.0), np.arange(-1.0, 12.0))
    x, y = xs.ravel(), ys.ravel()
    got = pcv.polygon_contains(sq, x, y, np.zeros(x.size)).astype(bool)
    assert np.array_equal(got, (0 <= x) & (x < 10) & (0 <= y) & (y < 10))
    rings = SHAPES["horizontal_edges"]
    got = pcv.polygon_contains(rings, x, y, np.zeros(x.size)).astype(bool)
    assert np.array_equal(got, P.contains(rings, x, y, np.zeros(x.size)))
    want = [P.exact_inside(rings, a, b)[0] for a, b in zip(x, y)]
    assert got.tolist() == want


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_contains_against_the_rationals(name):
    """The same verdict as exact arithmetic for every point whose exact horizontal distance to every crossing of its scanline is
    more than 1e-9 of the polygon's extent; at most 1 % of the uniform points are left out by that margin."""
    rings = SHAPES[name]
    x, y, z = uniform_points()
    want_np = P.inside(rings, x, y)
    assert np.array_equal(pcv.polygon_contains(rings, x, y, z).astype(bool), want_np)
    margin = Fraction(1e-9) * Fraction(P.extent(rings))
    seg = P.segments(rings)
    seg = seg[seg[:, 1] != seg[:, 3]]
    up = seg[:, 1] < seg[:, 3]
    lx, ly = np.where(up, seg[:, 0], seg[:, 2]), np.where(up, seg[:, 1], seg[:, 3])
    ux, uy = np.where(up, seg[:, 2], seg[:, 0]), np.where(up, seg[:, 3], seg[:, 1])
    # every f64 is an integer over a power of two: over the largest of them all, the rule is integer arithmetic
    den = max(float(v).as_integer_ratio()[1] for col in (lx, ly, ux, uy, x, y) for v in col)
    I = [[int(Fraction(float(v)) * den) for v in col] for col in (lx, ly, ux, uy)]
    left_out = 0
    for i in range(x.size):
        px, py = int(Fraction(float(x[i])) * den), int(Fraction(float(y[i])) * den)
        parity, near = False, False
        for e in np.nonzero((ly <= y[i]) & (y[i] < uy))[0]:  # (exact: comparisons of f64)
            dy = I[3][e] - I[1][e]
            diff = (px - I[0][e]) * dy - (py - I[1][e]) * (I[2][e] - I[0][e])  # (px - xc) * dy, times den^2
            parity ^= diff < 0
            near = near or abs(diff) * margin.denominator <= margin.numerator * dy * den
        if near:
            left_out += 1
        else:
            assert bool(want_np[i]) == parity, (name, i, x[i], y[i])
    print(f"{name}: {left_out} of {x.size} uniform points within the margin")
    assert left_out <= x.size // 100


@pytest.mark.parametrize("tiling", ["fan", "l"])
def test_a_tiling_keeps_every_point_in_exactly_one_piece(tiling):
    outline, pieces = P.fan_tiling() if tiling == "fan" else P.l_tiling()
    rng = np.random.Generator(np.random.PCG64(99))
    xs, ys = [rng.uniform(-1.0, 9.0, 20000)], [rng.uniform(-1.0, 9.0, 20000)]
    gx, gy = np.meshgrid(np.arange(-1.0, 10.0, 0.5), np.arange(-1.0, 10.0, 0.5))  # lattice points: on the shared edges too
    xs.append(gx.ravel())
    ys.append(gy.ravel())
    for piece in pieces:
        px, py = P.planted_points(piece)
        xs.append(px)
        ys.append(py)
    x, y = np.concatenate(xs), np.concatenate(ys)
    z = np.zeros(x.size)
    in_outline = pcv.polygon_contains(outline, x, y, z).astype(np.int64)
    count = np.zeros(x.size, dtype=np.int64)
    for piece in pieces:
        count += pcv.polygon_contains(piece, x, y, z)
    assert np.array_equal(count, in_outline), np.nonzero(count != in_outline)[0][:8]
    assert in_outline.sum() > 10000 and (in_outline == 0).sum() > 1000


def node_rule_cubes():
    """Cubes for the square with a square hole ([0, 10]^2 without [3, 7]^2), z slab [-1, 2]: min xyz, edge."""
    cubes = {
        "inside": [0.5, 0.5, 0.0, 1.0], "outside": [12.0, 12.0, 0.0, 1.0], "across_an_edge": [9.5, 4.0, 0.0, 1.0],
        "around_a_vertex": [9.5, 9.5, 0.0, 1.0], "inside_the_hole": [4.0, 4.0, 0.0, 1.0], "across_the_hole_edge": [2.5, 4.0, 0.0, 1.0],
        "touches_at_a_corner": [10.0, 10.0, 0.0, 1.0], "touches_at_a_corner_from_below": [-1.0, -1.0, 0.0, 1.0],
        "touches_an_edge": [10.0, 4.0, 0.0, 1.0], "above_the_slab": [0.5, 0.5, 2.5, 1.0], "below_the_slab": [0.5, 0.5, -3.0, 1.0],
        "touches_the_slab_from_above": [0.5, 0.5, 2.0, 1.0], "touches_the_slab_from_below": [0.5, 0.5, -2.0, 1.0],
        "holds_the_polygon": [-5.0, -5.0, -10.0, 20.0], "holds_the_hole": [2.5, 2.5, 0.0, 5.0], "near_miss": [10.0 + 1e-9, 4.0, 0.0, 1.0],
    }
    return cubes


def test_the_node_rule_twin_equals_the_numpy_restatement():
    rings = SHAPES["square_with_hole"]
    named = node_rule_cubes()
    want_named = dict(inside=1, outside=0, across_an_edge=1, around_a_vertex=1, inside_the_hole=0, across_the_hole_edge=1,
                      touches_at_a_corner=1, touches_at_a_corner_from_below=1, touches_an_edge=1, above_the_slab=0, below_the_slab=0,
                      touches_the_slab_from_above=1, touches_the_slab_from_below=1, holds_the_polygon=1, holds_the_hole=1, near_miss=0)
    cubes = np.array([named[k] for k in want_named])
    got = pcv.polygon_intersects_cubes(rings, cubes, z_min=-1.0, z_max=2.0)
    assert got.tolist() == list(want_named.values()), dict(zip(want_named, got))
    assert np.array_equal(got.astype(bool), P.intersects_cubes(rings, cubes, -1.0, 2.0))
    rng = np.random.Generator(np.random.PCG64(5))
    for name, rings in SHAPES.items():
        n = 4000
        cubes = np.stack([rng.uniform(-2, 11, n), rng.uniform(-2, 11, n), rng.uniform(-4, 4, n), rng.choice([0.01, 0.3, 1.0, 4.0, 20.0], n)], axis=1)
        v = np.concatenate(P.as_rings(rings))[:64]  # cubes around vertices, and with a corner on one
        around = np.concatenate([np.stack([v[:, 0] - 0.25, v[:, 1] - 0.25, np.zeros(len(v)), np.full(len(v), 0.5)], axis=1),
                                 np.stack([v[:, 0], v[:, 1], np.zeros(len(v)), np.full(len(v), 0.5)], axis=1),
                                 np.stack([v[:, 0] - 0.5, v[:, 1] - 0.5, np.zeros(len(v)), np.full(len(v), 0.5)], axis=1)])
        cubes = np.concatenate([cubes, around])
        for z_min, z_max in ((-np.inf, np.inf), (-1.0, 0.5), (np.nan, 0.0)):
            got = pcv.polygon_intersects_cubes(rings, cubes, z_min=z_min, z_max=z_max).astype(bool)
            want = P.intersects_cubes(rings, cubes, z_min, z_max)
            assert np.array_equal(got, want), (name, z_min, np.nonzero(got != want)[0][:5])
        assert 0 < got.sum() or z_min != z_min


def host_walk(rings, z_min, z_max, bmin, edge, depth):
    """Breadth-first walk of a full octree over the cube (bmin, edge) to `depth` with the host twin as predicate: the leaf cubes
    (depth `depth`) it lists."""
    level = np.array([[bmin[0], bmin[1], bmin[2], edge]])
    for _ in range(depth + 1):
        hit = pcv.polygon_intersects_cubes(rings, level, z_min=z_min, z_max=z_max).astype(bool)
        listed = level[hit]
        half = listed[:, 3:4] / 2
        offs = np.array([[i, j, k] for i in (0, 1) for j in (0, 1) for k in (0, 1)], dtype=np.float64)
        level = np.concatenate([np.concatenate([listed[:, :3] + half * o, half], axis=1) for o in offs]) if len(listed) else np.zeros((0, 4))
    return listed


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_kept_points_lie_in_listed_nodes(seed):
    """Superset: every point that contains keeps lies in a leaf that the walk over the host twin lists."""
    rng = np.random.Generator(np.random.PCG64(seed))
    n = 6000
    x, y, z = rng.uniform(-1, 11, n), rng.uniform(-1, 11, n), rng.uniform(-3, 3, n)
    bmin, edge, depth = np.array([-1.0, -1.0, -6.5]), 12.0 + seed * 0.37, 4
    for name in ("concave_l", "square_with_hole", "star_257", "two_rings"):
        rings = SHAPES[name]
        z_min, z_max = (-1.25, 1.5) if seed != 2 else (-np.inf, np.inf)
        keep = pcv.polygon_contains(rings, x, y, z, z_min=z_min, z_max=z_max).astype(bool)
        leaves = host_walk(rings, z_min, z_max, bmin, edge, depth)
        size = edge / 2 ** depth
        # a point's leaf, as the recurrence places it: compare against every listed leaf's half-open box
        idx = {(round((c[0] - bmin[0]) / size), round((c[1] - bmin[1]) / size), round((c[2] - bmin[2]) / size)) for c in leaves}
        cell = np.floor((np.stack([x, y, z], axis=1)[keep] - bmin) / size).astype(np.int64)
        assert keep.sum() > 100 and all(tuple(c) in idx for c in cell), name
        assert len(leaves) < 8 ** depth  # and it does cull


def test_the_web_mercator_frame_is_the_projection_and_the_rule():
    from point_cloud_viewer_amd import synthetic
    x, y, z, _, _, _ = synthetic.uniform_ecef(5000)
    u, v = pcv.wmr_project(x, y, z)
    cu, cv = float(np.median(u)), float(np.median(v))
    ru, rv = float(u.max() - u.min()), float(v.max() - v.min())
    rings = [np.stack([cu + 0.3 * ru * np.cos(np.arange(7) * 0.9), cv + 0.3 * rv * np.sin(np.arange(7) * 0.9)], axis=1),
             np.array([[cu - 0.05 * ru, cv - 0.05 * rv], [cu + 0.05 * ru, cv - 0.05 * rv], [cu, cv + 0.08 * rv]])]
    got = pcv.polygon_contains(rings, x, y, z, frame=1).astype(bool)
    assert np.array_equal(got, P.contains_web_mercator(rings, u, v)) and 0.05 < got.mean() < 0.95
    deg = pcv.polygon_from_lat_lng([np.array([[37.40, -122.15], [37.41, -122.15], [37.41, -122.14]])])
    uu, vv = pcv.wmr_from_lat_lng(np.radians([37.40, 37.41, 37.41]), np.radians([-122.15, -122.15, -122.14]))
    assert len(deg) == 1 and np.array_equal(deg[0], np.stack([uu, vv], axis=1))
    pcv.polygon_check(deg, frame=1)


def test_polygon_check_says_what_is_wrong():
    sq = np.array([[0.0, 0.0], [0.5, 0.0], [0.5, 0.5]])

    def message(rings, **kw):
        with pytest.raises(pcv.PcvError) as e:
            pcv.polygon_check(rings, **kw)
        assert e.value.code == pcv.PCV_E_INVALID
        return str(e.value)

    pcv.polygon_check([sq])
    pcv.polygon_check([sq], frame=1)
    pcv.polygon_check([sq], z_min=3.0, z_max=1.0)  # valid: contains nothing
    assert "ring 1 has fewer than 3 vertices" in message([sq, sq[:2]])
    assert "has no ring" in message([])
    assert "vertex 1 is not finite" in message([np.array([[0.0, 0.0], [np.inf, 0.0], [0.5, 0.5]])])
    assert "vertex 2 is not finite" in message([np.array([[0.0, 0.0], [0.1, 0.0], [0.5, np.nan]])])
    many = P.regular(40000, 0.5, 0.5, 0.4)
    assert "more than 65535 vertices" in message([many, many[:25536]])
    pcv.polygon_check([many, many[:25535]])
    assert "the frame is 0 (xy) or 1 (web-mercator)" in message([sq], frame=2)
    assert "the frame is 0 (xy) or 1 (web-mercator)" in message([sq], frame=-1)
    assert "vertex 1 is outside [0, 1)" in message([np.array([[0.0, 0.0], [1.0, 0.0], [0.5, 0.5]])], frame=1)
    assert "vertex 0 is outside [0, 1)" in message([np.array([[-0.1, 0.0], [0.9, 0.0], [0.5, 0.5]])], frame=1)
    assert "has no height range" in message([sq], frame=1, z_min=0.0)
    assert "has no height range" in message([sq], frame=1, z_max=100.0)
