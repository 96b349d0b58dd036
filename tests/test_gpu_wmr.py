"""PCV_SHAPE_WEB_MERCATOR_RECT on the device: shape setup (corners, up to 45 separating axes), node culling through every
entry point, and the point test — device keep flag == pcv_wmr_contains on the host, bit for bit, alone and mixed with the other
kinds in one batch."""
import ctypes as C
import os
import subprocess
import types

import numpy as np
import pytest

import oracle_lib as O
import point_cloud_viewer_amd as pcv
from point_cloud_viewer_amd import synthetic
from test_gpu_query import ctx, random_frusta  # noqa: F401  (module fixture + the config-4 frustum generator)
from test_gpu_query_batch import assert_points_equal, oracle_segment, scene_of

import wmr_oracle as W

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def shape_of(r):
    return ("web_mercator_rect", r[0:2], r[2:4])


def center_uv(p):
    u, v = pcv.wmr_project([p[0]], [p[1]], [p[2]])
    return float(u[0]), float(v[0])


def rectangles_for(cu, cv):
    """The grids of test_wmr_cpu.py around (cu, cv), then a rectangle that misses the cloud, one that contains it whole and one
    that wraps in x."""
    rects = W.grid(cu, cv, 7, 1e-6) + W.grid(cu, cv, 26, 2.5e-7)
    rects.append((cu + 0.01, cv + 0.01, cu + 0.012, cv + 0.012))
    rects.append((cu - 0.0019, cv - 0.0019, cu + 0.0019, cv + 0.0019))
    rects.append((255.5 / 256.0, cv - 0.001, 0.5 / 256.0, cv + 0.001))
    # millimetre rectangles over the cloud's centre, the first 12 of them: 6 with more than 26 axes and 6 with fewer. Which ones
    # are wide depends on the rounding of the corners, i.e. on the host's libm — so they are chosen by counting the axes of the
    # host's own corners (the device starts from the same corners), not by a seed
    rng = np.random.default_rng(34)
    wide, narrow = [], []
    for k in range(4000):
        side = (0.1, 0.01, 0.001)[k % 3] / float(256 << 23)
        du, dv = rng.uniform(0.2, 0.8, 2)
        r = (cu - du * side, cv - dv * side, cu + (1.0 - du) * side, cv + (1.0 - dv) * side)
        (wide if len(W.axes_for_aabb(pcv.wmr_corners(r))) > 26 else narrow).append(r)
        if len(wide) >= 6 and len(narrow) >= 6:
            break
    assert len(wide) >= 6, "no millimetre rectangle with more than 26 axes among 4 000"
    return wide[:6] + narrow[:6] + rects



@pytest.fixture(scope="module")
def four(ctx):  # noqa: F811
    """A city-scale ECEF cloud built like test_all_four_encodings': u8, u16, f32 and f64 nodes in one octree."""
    # (that cloud lies 28 km below the ellipsoid, where no rectangle's polyhedron — 500 m below to 10 km above — reaches: this
    # one is centred on the ground, and its dense blob sits on the point nearest to 1 km above it)
    rot, ground = synthetic.ecef_from_local(37.407204, -122.147604)
    x, y, z, rgb, bmin, bmax = synthetic.gaussian_clusters(340_000, seed=12, num_clusters=6, extent=30000.0,
                                                           sigma_range=(5.0, 400.0), offset=tuple(ground - 15000.0))
    rng = np.random.default_rng(13)
    near = int(np.argmin((x - (ground + 1000.0 * rot[:, 2])[0]) ** 2 + (y - (ground + 1000.0 * rot[:, 2])[1]) ** 2 +
                         (z - (ground + 1000.0 * rot[:, 2])[2]) ** 2))
    c = np.array([x[near], y[near], z[near]])
    x = np.concatenate([x, c[0] + rng.normal(0.0, 0.03, 60_000)])
    y = np.concatenate([y, c[1] + rng.normal(0.0, 0.03, 60_000)])
    z = np.concatenate([z, c[2] + rng.normal(0.0, 0.03, 60_000)])
    rgb = synthetic.index_colors(x.size)
    bmin, bmax = np.array([x.min(), y.min(), z.min()]), np.array([x.max(), y.max(), z.max()])
    inten = (np.arange(x.size) % 251).astype(np.float32)
    s = scene_of(ctx, x, y, z, rgb, inten, bmin, bmax, 1500)
    tree = s["tree"]
    assert {tree.node(i).encoding for i in range(tree.num_nodes) if tree.node(i).num_points > 0} == {1, 2, 3, 4}
    s["center"] = c
    s["cubes"] = np.array([list(tree.node(i).cube_min) + [tree.node(i).cube_edge] for i in range(tree.num_nodes)])
    yield s
    tree.free()


# ---- 5. shape setup -------------------------------------------------------------------------------------------------------
def test_shape_setup_corners_and_axes(ctx):  # noqa: F811
    rng = np.random.default_rng(3)
    rects = []
    for _ in range(220):
        z = int(rng.integers(0, 24))
        zoom = float(256 << z)
        mn = rng.uniform(0.0, zoom - 1.5, 2)
        r = pcv.web_mercator_rect_from_zoomed(mn, mn + rng.uniform(0.05, 1.0, 2), z)
        assert r is not None
        rects.append(tuple(r[1]) + tuple(r[2]))
    rects.append((0.25, 0.5 - 1e-3, 0.25 + 2e-3, 0.5 + 1e-3))  # straddles the equator at lng = -90 degrees: axes coincide
    # The four east-west edges of a rectangle are parallel chords, so rounding aside a rectangle has at most 26 distinct axes;
    # the wide ones are the small ones, whose edges (millimetres) are short enough for the corners' rounding (1e-9 m) to turn
    # parallel edges by more than the deduplication's 1.5e-8: measured on the host, 27-28 axes at zoom 23 below 0.1 px.
    zoom = float(256 << 23)
    for k in range(300):
        mn = rng.uniform(0.2 * zoom, 0.8 * zoom, 2)
        r = pcv.web_mercator_rect_from_zoomed(mn, mn + (0.1, 0.01, 0.001)[k % 3], 23)
        rects.append(tuple(r[1]) + tuple(r[2]))
    shapes = ctx.shapes([shape_of(r) for r in rects])
    most = 0
    for i, r in enumerate(rects):
        corners, axes, valid = shapes.get(i)
        assert valid
        assert corners.tobytes() == pcv.wmr_corners(r).tobytes(), i
        want = W.axes_for_aabb(corners)
        assert axes.shape == want.shape and axes.tobytes() == want.tobytes(), (i, axes.shape, want.shape)
        most = max(most, len(axes))
    assert most > 26, most  # the wide path is exercised
    assert most <= 45
    # the narrow getter refuses a shape with more than 26 axes
    wide = next(i for i in range(len(rects)) if len(shapes.get(i)[1]) > 26)
    n, valid = C.c_uint32(), C.c_int()
    rc = ctx.lib.pcv_shapes_get(shapes.handle, wide, (C.c_double * 24)(), (C.c_double * 78)(), C.byref(n), C.byref(valid))
    assert rc == pcv.PCV_E_INVALID
    shapes.free()


# ---- 6. node lists --------------------------------------------------------------------------------------------------------
def bfs(names, index_of, rel):
    out, queue = [], [0]
    while queue:
        cur = queue.pop(0)
        if rel[cur] == W.REL_OUT:
            continue
        for d in range(8):
            child = index_of.get(names[cur] + str(d))
            if child is not None:
                queue.append(child)
        out.append(cur)
    return out


def test_node_lists_equal_the_numpy_sat(ctx, four):  # noqa: F811
    tree, names, index_of = four["tree"], four["names"], four["index_of"]
    rects = rectangles_for(*center_uv(four["center"]))
    shapes = ctx.shapes([shape_of(r) for r in rects])
    dense = tree.cull_nodes(shapes)
    counts, idx, rel, _ = tree.cull_nodes_sparse(shapes, tree.num_nodes, with_sizes=False)
    lists = tree.nodes_in_location(shapes)
    batch = tree.query_batch(shapes)
    first, seg_nodes, _ = batch.segments()
    kept_any = 0
    for s, r in enumerate(rects):
        want = W.relations_for_cubes(shapes.get(s)[0], four["cubes"])
        assert np.array_equal(dense[s], want), (s, np.nonzero(dense[s] != want)[0][:5])
        keep = np.nonzero(want != W.REL_OUT)[0]
        assert counts[s] == keep.size and np.array_equal(idx[s, :keep.size], keep) and np.array_equal(rel[s, :keep.size], want[keep]), s
        walk = bfs(names, index_of, want)
        assert list(lists[s]) == walk, s
        assert list(seg_nodes[first[s]:first[s + 1]]) == walk, s
        kept_any += bool(walk)
    assert max(len(shapes.get(s)[1]) for s in range(12)) > 26  # the SAT over more axes than the narrow table holds
    assert len(bfs(names, index_of, W.relations_for_cubes(shapes.get(len(rects) - 3)[0], four["cubes"]))) == 0   # the one that misses
    assert dense[len(rects) - 2][0] != W.REL_OUT                                                                  # the one that holds the cloud
    assert kept_any > 100
    batch.free()
    shapes.free()


# ---- 7. points ------------------------------------------------------------------------------------------------------------
def wmr_segment(sc, rect, name, interval):
    """Oracle decode of the node + pcv_wmr_contains + interval + retain."""
    nd = sc["oracle"].nodes[name]
    if nd["num_points"] == 0:
        return np.zeros(0), np.zeros(0), np.zeros(0), np.zeros((0, 3), np.uint8), np.zeros(0, np.float32)
    info = sc["tree"].node(sc["index_of"][name])
    px, py, pz = O.decode_positions(nd["encoding"], info.cube_min, info.cube_edge, nd["xyz"])
    inten = np.frombuffer(nd["intensity"], dtype=np.float32)
    keep = pcv.wmr_contains(rect, px, py, pz).astype(bool)
    if interval is not None:
        keep &= (interval[0] <= inten.astype(np.float64)) & (inten.astype(np.float64) <= interval[1])
    return px[keep], py[keep], pz[keep], np.frombuffer(nd["rgb"], dtype=np.uint8).reshape(-1, 3)[keep], inten[keep]


def mixed_batch(sc, seed):
    """The rectangles interleaved with AABB, OBB, frustum and AllPoints shapes, every third shape with an interval."""
    rng = np.random.default_rng(seed)
    bmin, bmax, c = sc["bmin"], sc["bmax"], sc["center"]
    rects = rectangles_for(*center_uv(c))
    fr = random_frusta(rng, bmin, bmax, 3)
    obb = (c, O.quat_from_axis_angle([1.0, 0.0, 0.0], 0.5), [300.0, 200.0, 150.0])
    lo, hi = bmin + (bmax - bmin) * 0.1, bmin + (bmax - bmin) * 0.8
    others = [(("aabb", lo, hi), (O.SHAPE_AABB, list(lo) + list(hi))), (("all",), (O.SHAPE_ALL, None)),
              (("obb", *obb), (O.SHAPE_OBB, list(obb[0]) + list(obb[1]) + list(obb[2]))),
              (("frustum", fr[0][0]), (O.SHAPE_FRUSTUM, fr[0][0])), (("frustum2", *fr[1]), (O.SHAPE_FRUSTUM2, np.concatenate(fr[1]))),
              (("aabb", c - 0.05, c + 0.04), (O.SHAPE_AABB, list(c - 0.05) + list(c + 0.04)))]
    shapes, kinds = [], []
    step = max(1, len(rects) // len(others))
    for i, r in enumerate(rects):
        if i % step == 0 and i // step < len(others):
            shapes.append(others[i // step][0])
            kinds.append(others[i // step][1])
        shapes.append(shape_of(r))
        kinds.append(("wmr", r))
    ivs = [(20.0, 180.0) if k % 3 == 0 else None for k in range(len(shapes))]
    return shapes, kinds, ivs


def check_batch(sc, batch, kinds, ivs):
    first, nodes, off = batch.segments()
    names = sc["names"]
    full = batch.points()
    assert full["count"] == batch.num_points == int(off[-1])
    kept = {"wmr": 0, "other": 0}
    for s, (kind, params) in enumerate(kinds):
        for k in range(int(first[s]), int(first[s + 1])):
            a, b = int(off[k]), int(off[k + 1])
            seg = dict(count=b - a, x=full["x"][a:b], y=full["y"][a:b], z=full["z"][a:b], rgb=full["rgb"][a:b],
                       intensity=None if full["intensity"] is None else full["intensity"][a:b])
            name = names[nodes[k]]
            want = wmr_segment(sc, params, name, ivs[s]) if kind == "wmr" else oracle_segment(sc, kind, params, name, ivs[s])
            assert_points_equal(seg, want, (s, k))
            kept["wmr" if kind == "wmr" else "other"] += b - a
        if kind != "wmr":
            want_names = O.nodes_in_location(sc["bmin"], sc["bmax"], sc["oracle"].nodes, kind, params)
            assert [names[i] for i in nodes[first[s]:first[s + 1]]] == want_names, s
    return kept


def test_mixed_batch_points_equal_the_host_chain(ctx, four):  # noqa: F811
    shapes, kinds, ivs = mixed_batch(four, 5)
    prepared = ctx.shapes(shapes)
    batch = four["tree"].query_batch(prepared, intervals=ivs)
    kept = check_batch(four, batch, kinds, ivs)
    assert kept["wmr"] > 50_000 and kept["other"] > 50_000, kept
    # the same through the single-location entry points, for a few rectangles
    tree, names = four["tree"], four["names"]
    first, nodes, off = batch.segments()
    full = batch.points()
    picks = [s for s, (k, _) in enumerate(kinds) if k == "wmr"]
    picks = picks[:2] + picks[12 + 22:12 + 26] + picks[-3:]
    for s in picks:
        a, b = int(off[first[s]]), int(off[first[s + 1]])
        got = tree.query_points(prepared, s, interval=ivs[s])
        assert got["count"] == b - a, s
        for key in ("x", "y", "z"):
            assert got[key].tobytes() == full[key][a:b].tobytes(), (s, key)
        for k in range(int(first[s]), int(first[s + 1]))[:4]:
            node = int(nodes[k])
            one = tree.query_points(prepared, s, interval=ivs[s], node=node)
            assert_points_equal(one, wmr_segment(four, kinds[s][1], names[node], ivs[s]), (s, k))
            info = tree.node(node)
            if info.num_points:
                keep, n_kept = tree.cull_node_points(prepared, s, node, interval=ivs[s])
                assert n_kept == one["count"] == int(keep.sum()), (s, k)
    batch.free()
    prepared.free()


def test_cull_points_on_raw_arrays_and_an_opened_directory(ctx, four, tmp_path):  # noqa: F811
    x, y, z = synthetic.uniform_ecef(200_000)[:3]
    c = synthetic._ecef_from_lat_lng(37.407204, -122.147604)
    rects = W.grid(*center_uv(c), 7, 1e-6)[::5]
    shapes = ctx.shapes([shape_of(r) for r in rects])
    inten = (np.arange(x.size) % 97).astype(np.float32)
    total = 0
    for s, r in enumerate(rects):
        keep, kept = ctx.cull_points(shapes, s, x, y, z)
        want = pcv.wmr_contains(r, x, y, z)
        assert keep.tobytes() == want.tobytes() and kept == int(want.sum()), s
        keep, kept = ctx.cull_points(shapes, s, x, y, z, intensity=inten, interval=(10.0, 40.0))
        want2 = want & (inten >= 10.0) & (inten <= 40.0)
        assert keep.tobytes() == want2.astype(np.uint8).tobytes() and kept == int(want2.sum()), s
        total += int(want.sum())
    assert total > 10_000
    shapes.free()
    # an octree opened from a directory gives the segments the built one gives
    four["tree"].write_dir(tmp_path)
    opened = ctx.open_dir(tmp_path)
    rects = rectangles_for(*center_uv(four["center"]))[::9]
    prepared = ctx.shapes([shape_of(r) for r in rects])
    b1, b2 = four["tree"].query_batch(prepared), opened.query_batch(prepared)
    p1, p2 = b1.points(), b2.points()
    assert p1["count"] == p2["count"] > 1000
    for key in ("x", "y", "z", "rgb"):
        assert np.asarray(p1[key]).tobytes() == np.asarray(p2[key]).tobytes(), key
    assert all(np.array_equal(a, b) for a, b in zip(b1.segments(), b2.segments()))
    b1.free()
    b2.free()
    prepared.free()
    opened.free()


# ---- 8. points planted around the four edges ------------------------------------------------------------------------------
def planted_points(r, per_edge, rng):
    """Per edge of `r`: positions whose truth lies within 1e-12 of the bound, and their f64 neighbours 1-3 nextafter steps away
    in each ECEF coordinate. Returns x, y, z."""
    out = []
    for edge in range(4):
        t = rng.uniform(0.0, 1.0, per_edge)
        u = np.full(per_edge, r[0] if edge == 0 else r[2]) if edge < 2 else r[0] + t * (r[2] - r[0])
        v = r[1] + t * (r[3] - r[1]) if edge < 2 else np.full(per_edge, r[1] if edge == 2 else r[3])
        lat, lng = pcv.wmr_to_lat_lng(u, v)
        h = rng.uniform(-400.0, 9000.0, per_edge)
        n = W.A / np.sqrt(1.0 - W.E2 * np.sin(lat) ** 2)
        p = np.stack([(n + h) * np.cos(lat) * np.cos(lng), (n + h) * np.cos(lat) * np.sin(lng), (n * (1.0 - W.E2) + h) * np.sin(lat)])
        tu, tv = W.truth_uv_ld(p[0], p[1], p[2])
        d = np.abs(tu - np.longdouble(u)) if edge < 2 else np.abs(tv - np.longdouble(v))
        assert float(d.max()) < 1e-12, (edge, float(d.max()))
        pts = [p]
        for axis in range(3):
            for direction in (-np.inf, np.inf):
                q = p.copy()
                for _ in range(3):
                    q[axis] = np.nextafter(q[axis], direction)
                    pts.append(q.copy())
        out.append(np.concatenate(pts, axis=1))
        assert out[-1].shape[1] >= 5000
    return out


def test_points_planted_around_the_edges(ctx):  # noqa: F811
    """Several thousand points per edge on and 1-3 ulps beside the rectangle's four edges, in an octree whose nodes are all
    f64-encoded (resolution 1e-6 m: every cube wider than 17 m), through the batch and pcv_query_points (the staged decode:
    query_flags_wmr_kernel, query_flags_kernel<5>) and through pcv_cull_points on the raw arrays: device == host for all."""
    rng = np.random.default_rng(17)
    r = (0.16, 0.38, 0.16 + 3e-3, 0.38 + 3e-3)
    edges = planted_points(r, 800, rng)
    shapes = ctx.shapes([shape_of(r), ("all",)])
    for edge, p in enumerate(edges):  # raw arrays
        x, y, z = (np.ascontiguousarray(p[k]) for k in range(3))
        keep, kept = ctx.cull_points(shapes, 0, x, y, z)
        want = pcv.wmr_contains(r, x, y, z)
        assert keep.tobytes() == want.tobytes(), (edge, int((keep != want).sum()))
        assert 0 < int(want.sum()) < x.size, (edge, int(want.sum()))  # both sides of the edge are there
    x, y, z = (np.ascontiguousarray(np.concatenate([p[k] for p in edges])) for k in range(3))
    order = rng.permutation(x.size)
    x, y, z = x[order], y[order], z[order]
    rgb = synthetic.index_colors(x.size)
    inten = (np.arange(x.size) % 251).astype(np.float32)
    bmin, bmax = np.array([x.min(), y.min(), z.min()]) - 1.0, np.array([x.max(), y.max(), z.max()]) + 1.0
    tree = ctx.build(1e-6, pcv.Aabb(bmin, bmax), x, y, z, rgb, inten, max_points_per_node=1500)
    assert {tree.node(i).encoding for i in range(tree.num_nodes) if tree.node(i).num_points > 0} == {4}
    names = tree.node_names()
    sc = dict(tree=tree, names=names, index_of={n: i for i, n in enumerate(names)}, oracle=types.SimpleNamespace(nodes=tree.to_dict()))
    batch = tree.query_batch(shapes)
    first, nodes, off = batch.segments()
    full = batch.points()
    candidates = kept = 0
    for k in range(int(first[0]), int(first[1])):
        a, b = int(off[k]), int(off[k + 1])
        seg = dict(count=b - a, x=full["x"][a:b], y=full["y"][a:b], z=full["z"][a:b], rgb=full["rgb"][a:b], intensity=full["intensity"][a:b])
        assert_points_equal(seg, wmr_segment(sc, r, names[nodes[k]], None), k)
        candidates += tree.node(int(nodes[k])).num_points
        kept += b - a
    # the node walk reaches the planted points (they lie on the polyhedron's faces, up to its sagitta), and both sides are there
    assert candidates >= 0.9 * x.size, (candidates, x.size)
    assert 0.2 * x.size < kept < 0.8 * x.size, (kept, x.size)
    one = tree.query_points(shapes, 0)
    assert one["count"] == kept
    a, b = int(off[first[0]]), int(off[first[1]])
    for key in ("x", "y", "z"):
        assert one[key].tobytes() == np.asarray(full[key][a:b]).tobytes(), key
    batch.free()
    shapes.free()
    tree.free()


# ---- 9. groupings and repeats ---------------------------------------------------------------------------------------------
def test_flags_do_not_depend_on_the_batch(ctx, four):  # noqa: F811
    tree = four["tree"]
    rects = rectangles_for(*center_uv(four["center"]))
    pick = 12 + 7 * 3 + 3  # the rectangle of the 7 x 7 grid over the dense cluster (after the 12 millimetre ones)
    alone = ctx.shapes([shape_of(rects[pick])])
    one = tree.query_batch(alone)
    want = one.points()
    assert want["count"] > 1000
    many = [shape_of(rects[i % len(rects)]) for i in range(2000)]
    many[1234] = shape_of(rects[pick])
    big = ctx.shapes(many)
    for _ in range(2):
        batch = tree.query_batch(big)
        got = batch.shape_points(1234)
        assert got["count"] == want["count"]
        for key in ("x", "y", "z", "rgb"):
            assert np.asarray(got[key]).tobytes() == np.asarray(want[key]).tobytes(), key
        batch.free()
    again = tree.query_points(alone, 0)
    assert again["count"] == want["count"] and again["x"].tobytes() == np.asarray(want["x"]).tobytes()
    one.free()
    alone.free()
    big.free()


# ---- 10. the C example ----------------------------------------------------------------------------------------------------
def test_c_example_prints_the_map_tile_counts(ctx, four, tmp_path):  # noqa: F811
    """examples/query_batch.c --map-tiles <zoom>: plain C over pcv_wmr_project, pcv_wmr_from_zoomed and the batch prints the
    counts the Python mirror gets for the same tiles."""
    four["tree"].write_dir(tmp_path / "oct")
    zoom = 14
    p = subprocess.run([os.path.join(ROOT, "examples", "bin", "query_batch"), str(tmp_path / "oct"), "--map-tiles", str(zoom)],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    got = [tuple(int(v) for v in line.split()) for line in p.stdout.splitlines()]
    assert len(got) >= 4
    opened = ctx.open_dir(tmp_path / "oct")
    shapes = []
    for tx, ty, _ in got:
        rect = pcv.web_mercator_rect_from_zoomed((256.0 * tx, 256.0 * ty), (256.0 * (tx + 1), 256.0 * (ty + 1)), zoom)
        assert rect is not None
        shapes.append(rect)
    batch = opened.query_batch(ctx.shapes(shapes))
    first, _, off = batch.segments()
    want = [(tx, ty, int(off[first[k + 1]] - off[first[k]])) for k, (tx, ty, _) in enumerate(got)]
    assert got == want
    assert sum(c for _, _, c in want) > 50_000  # (not every point: nodes above 10 km or below -500 m meet no tile's polyhedron)
    batch.free()
    opened.free()
