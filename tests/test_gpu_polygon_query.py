"""Polygons as query locations (PCV_SHAPE_POLYGON) on the device: node lists against the breadth-first walk over
the host twin and over the numpy restatement of the node rule, every segment against decode + the numpy restatement of the
point rule + interval (byte for byte), the tiling property, web-mercator polygons over an ECEF octree and an S2 cell cloud, PLY
output, the C example and the refusals."""
import math
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import point_cloud_viewer_amd as pcv
from point_cloud_viewer_amd import synthetic
import polygon_truth as P
import union_octree_cases as U

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
FIELDS = ("x", "y", "z", "rgb", "intensity")


@pytest.fixture(scope="module")
def ctx():
    c = pcv.Context(0)
    yield c
    c.close()


def _intensity(n):
    return (((np.arange(n, dtype=np.int64) * 2654435761) % 100003).astype(np.float32) * 0.25 - 7.0)


def _index_of(rgb):
    rgb = np.asarray(rgb).reshape(-1, 3).astype(np.int64)
    return (rgb[:, 0] << 16) | (rgb[:, 1] << 8) | rgb[:, 2]


def local_cloud(n=20000):
    rng = np.random.Generator(np.random.PCG64(41))
    x, y, z = rng.uniform(0.0, 100.0, n), rng.uniform(0.0, 100.0, n), rng.uniform(0.0, 20.0, n)
    return x, y, z, synthetic.index_colors(n), np.array([0.0, 0.0, 0.0]), np.array([100.0, 100.0, 20.0])


def polygon_specs(s):
    """name -> ("polygon", rings, z_min, z_max) over the local cloud [0, 100]^2 x [0, 20]."""
    cubes, tree = s["cubes"], s["tree"]
    deepest = max(range(tree.num_nodes), key=lambda i: (int(tree.node(i).level), tree.node(i).num_points))
    c = cubes[deepest]
    leaf_tri = np.array([[c[0] + 0.2 * c[3], c[1] + 0.2 * c[3]], [c[0] + 0.8 * c[3], c[1] + 0.3 * c[3]], [c[0] + 0.4 * c[3], c[1] + 0.8 * c[3]]])
    sq = np.array([[10.0, 10.0], [90.0, 10.0], [90.0, 90.0], [10.0, 90.0]])
    hole = np.array([[30.0, 30.0], [70.0, 30.0], [70.0, 70.0], [30.0, 70.0]])
    specs = {f"gon{n}": ("polygon", [P.regular(n, 50.0, 50.0, 38.0, 0.05 * n)], -INF, INF) for n in (3, 63, 64, 65, 129)}
    specs.update({
        "hole": ("polygon", [sq, hole], -INF, INF),
        "two_rings": ("polygon", [P.regular(5, 25.0, 30.0, 18.0), P.regular(7, 70.0, 65.0, 22.0)[::-1].copy()], -INF, INF),
        "in_one_leaf": ("polygon", [leaf_tri], -INF, INF),
        "holds_the_cloud": ("polygon", [np.array([[-50.0, -50.0], [150.0, -50.0], [150.0, 150.0], [-50.0, 150.0]])], -INF, INF),
        "disjoint": ("polygon", [np.array([[500.0, 500.0], [520.0, 500.0], [510.0, 530.0]])], -INF, INF),
        "slab": ("polygon", [P.regular(65, 50.0, 50.0, 38.0, 0.3)], 5.0, 12.25),
        "slab_below": ("polygon", [sq], -INF, 7.5),
        "slab_above": ("polygon", [sq], 14.0, INF),
        "slab_inverted": ("polygon", [sq], 9.0, 3.0),
        "slab_nan": ("polygon", [sq], float("nan"), 3.0),
    })
    return specs


def make_scene(ctx):
    """About 20 000 uniform points in [0, 100]^2 x [0, 20] with an intensity, max_points_per_node = 300: four levels."""
    x, y, z, rgb, bmin, bmax = local_cloud()
    inten = _intensity(x.size)
    tree = ctx.build(0.001, pcv.Aabb(bmin, bmax), x, y, z, rgb, inten, max_points_per_node=300)
    assert max(int(tree.node(i).level) for i in range(tree.num_nodes)) >= 3
    cubes, first_child, child_mask = U.tree_tables(tree)
    s = dict(tree=tree, cubes=cubes, first_child=first_child, child_mask=child_mask, x=x, y=y, z=z, rgb=rgb, inten=inten, bmin=bmin, bmax=bmax)
    s["specs"] = polygon_specs(s)
    s["names"] = list(s["specs"])
    s["shapes"] = ctx.shapes([s["specs"][k] for k in s["names"]])
    return s


@pytest.fixture(scope="module")
def scene(ctx):
    s = make_scene(ctx)
    yield s
    s["shapes"].free()
    s["tree"].free()


def want_list(s, spec):
    _, rings, z_min, z_max = spec
    twin = U.bfs(pcv.polygon_intersects_cubes(rings, s["cubes"], z_min=z_min, z_max=z_max), s["first_child"], s["child_mask"])
    restated = U.bfs(P.intersects_cubes(rings, s["cubes"], z_min, z_max), s["first_child"], s["child_mask"])
    assert np.array_equal(twin, restated)
    return twin


def test_node_lists_equal_the_walk_over_the_host_twin(ctx, scene):
    tree, shapes, names, specs = scene["tree"], scene["shapes"], scene["names"], scene["specs"]
    got = np.array([list(tree.node(i).cube_min) + [tree.node(i).cube_edge] for i in range(tree.num_nodes)])
    assert np.array_equal(got, scene["cubes"])
    lists = dict(zip(names, tree.nodes_in_location(shapes)))
    batch = tree.query_batch(shapes)
    first, node, _ = batch.segments()
    for l, name in enumerate(names):
        want = want_list(scene, specs[name])
        assert lists[name].dtype == np.uint32 and np.array_equal(lists[name], want), (name, lists[name][:8], want[:8])
        assert np.all(np.diff(lists[name].astype(np.int64)) > 0)
        assert np.array_equal(node[int(first[l]):int(first[l + 1])], want), name
        one = ctx.shapes([specs[name]])  # the single-location form
        assert np.array_equal(tree.nodes_in_location(one)[0], want), name
        rings = shapes.polygon(l)
        assert len(rings) == len(specs[name][1]) and all(np.array_equal(a, b) for a, b in zip(rings, specs[name][1]))
        one.free()
    batch.free()
    print(f"{tree.num_nodes} nodes; listed: { {k: len(v) for k, v in lists.items()} }")
    assert len(lists["holds_the_cloud"]) == tree.num_nodes  # no edge hits an inner node: the corner rule carries the walk
    assert len(lists["disjoint"]) == 0 and len(lists["slab_nan"]) == 0
    assert 1 <= len(lists["in_one_leaf"]) <= 5 and 0 < len(lists["hole"]) < tree.num_nodes
    assert 0 < len(lists["slab"]) < len(lists["gon65"]) and 0 < len(lists["slab_above"]) < len(lists["hole"])
    # a capacity below the count: the full count, the first entries
    capacity = 5
    counts, out = np.zeros(len(names), dtype=np.uint32), np.full((len(names), capacity), 0xFFFFFFFF, dtype=np.uint32)
    ctx._check(ctx.lib.pcv_nodes_in_location(ctx.handle, shapes.handle, tree.handle, capacity, counts.ctypes.data, out.ctypes.data))
    for l, name in enumerate(names):
        assert counts[l] == len(lists[name]) and np.array_equal(out[l, :min(capacity, counts[l])], lists[name][:capacity]), name


def mixed_table(s):
    """Polygons interleaved with the six other kinds, and per-shape intervals: none, lo > hi, NaN, plain."""
    specs, bmin, bmax = s["specs"], s["bmin"], s["bmax"]
    lo, hi = (float(v) for v in np.quantile(s["inten"], [0.2, 0.7]))
    c, q = O.frustum_new([50.0, -20.0, 10.0], O.quat_from_axis_angle([1.0, 0.0, 0.0], -math.pi / 2), O.perspective3_new(1.0, 1.2, 0.1, 90.0))
    tile = ("web_mercator_rect", [0.1, 0.1], [0.9, 0.9])  # (over a local cloud: projected as if ECEF; taken as given)
    table = [("aabb", bmin + 10.0, bmax - 5.0), specs["gon3"], ("all",), specs["hole"], ("obb", [50.0, 50.0, 10.0], O.quat_from_axis_angle([0.0, 0.0, 1.0], 0.4), [30.0, 20.0, 6.0]),
             specs["gon129"], ("frustum2", c, q), specs["slab"], ("frustum", c), tile, specs["two_rings"], ("s2_cells", [U.centre_leaf()]),
             specs["in_one_leaf"], specs["gon64"], specs["holds_the_cloud"], specs["disjoint"], specs["gon63"]]
    ivs = [None] * len(table)
    ivs[1] = (lo, hi)
    ivs[3] = (hi, lo)             # inverted: nothing
    ivs[5] = (float("nan"), hi)   # NaN: nothing
    ivs[7] = (lo, hi)
    ivs[0] = (lo, hi)
    ivs[14] = (lo, INF)
    return table, ivs


def check_polygon_segments(tree, table, shapes, ivs, all_l):
    """Every (polygon, listed node) segment == the node's AllPoints segment filtered by the numpy restatement and the interval."""
    batch = tree.query_batch(shapes, ivs)
    first, node, off = batch.segments()
    all_first = int(first[all_l])
    assert np.array_equal(node[all_first:int(first[all_l + 1])], np.arange(tree.num_nodes))
    counts = []
    for l, spec in enumerate(table):
        whole = batch.shape_points(l)
        counts.append(whole["count"])
        if spec[0] != "polygon":
            continue
        parts = []
        for k in range(int(first[l]), int(first[l + 1])):
            p = batch.points(all_first + int(node[k]), 1)
            keep = P.contains(spec[1], p["x"], p["y"], p["z"], spec[2], spec[3])
            if ivs[l] is not None:
                a = p["intensity"].astype(np.float64)
                keep &= (ivs[l][0] <= a) & (a <= ivs[l][1])
            got = batch.points(k, 1)
            for f in FIELDS:
                assert np.array_equal(got[f], p[f][keep]), (l, int(node[k]), f)
            parts.append(got)
        for f in FIELDS:
            cat = np.concatenate([p[f] for p in parts]) if parts else whole[f][:0]
            assert np.array_equal(whole[f], cat), (l, f)
    return batch, counts


def test_mixed_batch_segments_equal_decode_rule_interval(ctx, scene):
    tree = scene["tree"]
    table, ivs = mixed_table(scene)
    shapes = ctx.shapes(table)
    batch, counts = check_polygon_segments(tree, table, shapes, ivs, 2)
    print(f"points per shape: {counts}")
    assert counts[3] == 0 and counts[5] == 0 and counts[15] == 0 and 0 < counts[1] and 0 < counts[7] and 0 < counts[12] < 300
    assert 0 < counts[14] < tree.num_points and counts[13] > 0 and counts[16] > 0 and counts[10] > 0
    # the other kinds are what they are in a table without polygons
    others = [l for l, spec in enumerate(table) if spec[0] != "polygon"]
    plain = ctx.shapes([table[l] for l in others])
    pb = tree.query_batch(plain, [ivs[l] for l in others])
    for k, l in enumerate(others):
        a, b = batch.shape_points(l), pb.shape_points(k)
        assert a["count"] == b["count"] and all(np.array_equal(a[f], b[f]) for f in FIELDS), l
    # one polygon alone == the same polygon inside the mixed batch == pcv_query_points (and its single-node forms)
    for l in (1, 7, 10, 13):
        one = ctx.shapes([table[l]])
        ob = tree.query_batch(one, [ivs[l]])
        alone, inside = ob.shape_points(0), batch.shape_points(l)
        single = tree.query_points(shapes, l, interval=ivs[l])
        assert alone["count"] == inside["count"] == single["count"]
        for f in FIELDS:
            assert np.array_equal(alone[f], inside[f]) and np.array_equal(single[f], inside[f]), (l, f)
        first, node, _ = batch.segments()
        for k in range(int(first[l]), min(int(first[l]) + 3, int(first[l + 1]))):
            n = int(node[k])
            got = batch.points(k, 1)
            in_node = tree.query_points(shapes, l, interval=ivs[l], node=n)
            flags, kept = tree.cull_node_points(shapes, l, n, interval=ivs[l])
            assert kept == int(flags.sum()) == in_node["count"] == got["count"], (l, n)
            assert all(np.array_equal(in_node[f], got[f]) for f in FIELDS), (l, n)
        ob.free()
        one.free()
    for o in (pb, plain, batch, shapes):
        o.free()


def test_cull_points_on_raw_arrays_with_planted_points(ctx, scene):
    import torch
    specs = scene["specs"]
    rng = np.random.Generator(np.random.PCG64(8))
    for name in ("gon65", "hole", "two_rings", "slab"):
        _, rings, z_min, z_max = specs[name]
        px, py = P.planted_points(rings)
        x = np.concatenate([rng.uniform(-5.0, 105.0, 3000), px])
        y = np.concatenate([rng.uniform(-5.0, 105.0, 3000), py])
        z = np.concatenate([rng.uniform(0.0, 20.0, 3000), np.array([5.0, 12.25, 8.0, 4.9])[np.arange(px.size) % 4]])
        inten = _intensity(x.size)
        shapes = ctx.shapes([("all",), specs[name]])
        want = P.contains(rings, x, y, z, z_min, z_max)
        assert np.array_equal(pcv.polygon_contains(rings, x, y, z, z_min=z_min, z_max=z_max).astype(bool), want)
        keep, kept = ctx.cull_points(shapes, 1, x, y, z)
        assert np.array_equal(keep.astype(bool), want) and kept == int(want.sum()) and 0 < kept < x.size, name
        lo, hi = (float(v) for v in np.quantile(inten, [0.3, 0.6]))
        a = inten.astype(np.float64)
        keep, kept = ctx.cull_points(shapes, 1, x, y, z, intensity=inten, interval=(lo, hi))
        assert np.array_equal(keep.astype(bool), want & (lo <= a) & (a <= hi)) and kept == int(keep.sum()) > 0
        dev = [torch.from_numpy(v).cuda() for v in (x, y, z)]
        torch.cuda.synchronize()
        keep_d, kept_d = ctx.cull_points(shapes, 1, *dev)
        assert keep_d.is_cuda and np.array_equal(keep_d.cpu().numpy().astype(bool), want) and kept_d == int(want.sum())
        shapes.free()


def test_a_tiling_keeps_every_point_once_on_the_device(ctx, scene):
    tree = scene["tree"]
    for outline, pieces in (P.fan_tiling(), P.l_tiling()):
        place = lambda rings: [r * 10.0 + 10.0 for r in rings]  # noqa: E731  [0, 8]^2 -> [10, 90]^2, exact in f64
        table = [("polygon", place(outline), -INF, INF)] + [("polygon", place(p), -INF, INF) for p in pieces]
        shapes = ctx.shapes(table)
        batch = tree.query_batch(shapes)
        whole = batch.shape_points(0)
        got = [batch.shape_points(1 + k) for k in range(len(pieces))]
        assert sum(g["count"] for g in got) == whole["count"] > 5000
        index = np.concatenate([_index_of(g["rgb"]) for g in got])
        assert np.array_equal(np.sort(index), np.sort(_index_of(whole["rgb"]))) and np.unique(index).size == index.size
        batch.free()
        shapes.free()


def test_a_reopened_octree_answers_the_same(ctx, scene, tmp_path):
    tree, shapes = scene["tree"], scene["shapes"]
    tree.write_dir(tmp_path)
    opened = ctx.open_dir(tmp_path)
    for got, want in zip(opened.nodes_in_location(shapes), tree.nodes_in_location(shapes)):
        assert np.array_equal(got, want)
    a, b = opened.query_batch(shapes), tree.query_batch(shapes)
    for l in range(shapes.count):
        pa, pb = a.shape_points(l), b.shape_points(l)
        assert pa["count"] == pb["count"] and all(np.array_equal(pa[f], pb[f]) for f in FIELDS), l
    for o in (a, b, opened):
        o.free()


def test_a_directory_with_all_four_encodings(ctx, tmp_path):
    """A directory written by the oracle: a city-scale cloud with a dense blob, so that u8, u16, f32 and f64 nodes occur."""
    x, y, z, rgb, bmin, bmax = synthetic.gaussian_clusters(12000, seed=12, num_clusters=6, extent=30000.0, sigma_range=(5.0, 400.0))
    rng = np.random.default_rng(13)
    c = np.array([x[0], y[0], z[0]])
    x, y, z = (np.concatenate([v, c[a] + rng.normal(0.0, 0.03, 4000)]) for a, v in enumerate((x, y, z)))
    rgb = synthetic.index_colors(x.size)
    bmin, bmax = np.array([x.min(), y.min(), z.min()]), np.array([x.max(), y.max(), z.max()])
    inten = (np.arange(x.size) % 251).astype(np.float32)
    with O.max_points_per_node(300):
        assert O.build_literal_dir(tmp_path, 0.001, bmin, bmax, x, y, z, rgb, inten, threads=4) == 0
    tree = ctx.open_dir(tmp_path)
    assert {tree.node(i).encoding for i in range(tree.num_nodes) if tree.node(i).num_points > 0} == {1, 2, 3, 4}
    mid = (bmin + bmax) / 2
    blob = [np.array([[c[0] - 0.05, c[1] - 0.04], [c[0] + 0.06, c[1] - 0.02], [c[0] + 0.01, c[1] + 0.05]])]
    table = [("all",), ("polygon", [P.regular(65, mid[0], mid[1], 9000.0)], -INF, INF), ("polygon", blob, -INF, INF),
             ("polygon", blob, c[2] - 0.02, c[2] + 0.03), ("polygon", [P.star(129, mid[0], mid[1], 14000.0, 5000.0)], mid[2], INF)]
    ivs = [None, (20.0, 180.0), None, (20.0, 180.0), None]
    shapes = ctx.shapes(table)
    cubes, first_child, child_mask = U.tree_tables(tree)
    lists = tree.nodes_in_location(shapes)
    for l in range(1, len(table)):
        want = U.bfs(pcv.polygon_intersects_cubes(table[l][1], cubes, z_min=table[l][2], z_max=table[l][3]), first_child, child_mask)
        assert np.array_equal(lists[l], want), l
    batch, counts = check_polygon_segments(tree, table, shapes, ivs, 0)
    encodings = {tree.node(int(n)).encoding for n in lists[1]} | {tree.node(int(n)).encoding for n in lists[2]}
    assert encodings == {1, 2, 3, 4} and all(cnt > 0 for cnt in counts), (encodings, counts)
    assert counts[3] < counts[2]
    for o in (batch, shapes, tree):
        o.free()


def test_node_lists_across_the_batch_seam(ctx):
    """As test_gpu_union_query's seam test: the polygon walk is launched again past `batch` locations, the queues indexed inside
    the batch, counts, lists and rows by the shape."""
    x, y, z, rgb, bmin, bmax = local_cloud()
    tree = ctx.build(0.001, pcv.Aabb(bmin, bmax), x, y, z, rgb, max_points_per_node=2)
    m = tree.num_nodes
    batch = max(64, (256 << 20) // (4 * m))
    assert batch < 6000, (m, batch)
    kinds = {"far": ("polygon", [np.array([[500.0, 500.0], [520.0, 500.0], [510.0, 530.0]])], -INF, INF),
             "gon": ("polygon", [P.regular(65, 50.0, 50.0, 8.0)], 5.0, 9.0),
             "fine": ("polygon", [np.array([[20.0, 20.0], [21.0, 20.5], [20.5, 21.5]])], -INF, INF),
             "box": ("aabb", bmin, bmin + 0.1 * (bmax - bmin))}
    alone = {}
    for name, spec in kinds.items():
        one = ctx.shapes([spec])
        alone[name] = tree.nodes_in_location(one)[0]
        one.free()
    assert len(alone["gon"]) > 64 and len(alone["fine"]) > 0 and len(alone["far"]) == 0
    pick = ["far"] * (batch + 7)
    pick[0], pick[1], pick[2] = "gon", "box", "fine"
    pick[batch - 2:batch + 3] = ["gon", "fine", "box", "gon", "fine"]
    pick[-2:] = ["far", "gon"]
    shapes = ctx.shapes([kinds[p] for p in pick])
    capacity = max(len(v) for v in alone.values()) + 1
    counts, out = np.zeros(len(pick), dtype=np.uint32), np.zeros((len(pick), capacity), dtype=np.uint32)
    ctx._check(ctx.lib.pcv_nodes_in_location(ctx.handle, shapes.handle, tree.handle, capacity, counts.ctypes.data, out.ctypes.data))
    b = tree.query_batch(shapes)
    first, node, _ = b.segments()
    for l, p in enumerate(pick):
        assert np.array_equal(out[l, :counts[l]], alone[p]), (l, p)
        assert np.array_equal(node[int(first[l]):int(first[l + 1])], alone[p]), (l, p)
    for o in (b, shapes, tree):
        o.free()


# ---- the web-mercator frame -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ecef(ctx):
    """An ECEF cloud of 4 000 points as an octree and as an S2 cell cloud at level 20, and web-mercator polygons over it."""
    x, y, z, rgb, bmin, bmax = synthetic.uniform_ecef(4000)
    inten = _intensity(x.size)
    tree = ctx.build(0.001, pcv.Aabb(bmin, bmax), x, y, z, rgb, inten, max_points_per_node=200)
    cloud = ctx.s2_split(dict(x=x, y=y, z=z, color=rgb, intensity=inten), 20)
    u, v = pcv.wmr_project(x, y, z)
    cu, cv, ru, rv = float(np.median(u)), float(np.median(v)), float(u.max() - u.min()), float(v.max() - v.min())

    def gon(n, scale, du=0.0, dv=0.0):
        a = 0.1 + 2.0 * np.pi * np.arange(n) / n
        return np.stack([cu + du * ru + scale * ru * np.cos(a), cv + dv * rv + scale * rv * np.sin(a)], axis=1)

    polys = [[gon(8, 0.3)], [gon(65, 0.35), gon(5, 0.1)], [gon(3, 0.05, 0.3, 0.3), gon(4, 0.08, -0.25, -0.2)], [gon(6, 2.0)],
             [gon(4, 0.1, 30.0, 30.0)]]
    s = dict(tree=tree, cloud=cloud, x=x, y=y, z=z, rgb=rgb, inten=inten, polys=polys)
    yield s
    cloud.free()
    tree.free()


def test_web_mercator_polygons_over_the_octree_and_the_s2_cloud(ctx, ecef):
    tree, cloud, polys = ecef["tree"], ecef["cloud"], ecef["polys"]
    table = [("all",)]
    for rings in polys:
        table += [("polygon_web_mercator", rings), P.bounding_rect(rings)]
    lo, hi = (float(v) for v in np.quantile(ecef["inten"], [0.25, 0.8]))
    ivs = [None] * len(table)
    ivs[3] = (lo, hi)
    shapes = ctx.shapes(table)
    node_lists, cell_lists = tree.nodes_in_location(shapes), cloud.cells_in_location_indices(shapes)
    tb, cb = tree.query_batch(shapes, ivs), cloud.query_batch(shapes, intervals=ivs)
    tfirst, tnode, _ = tb.segments()
    cfirst, ccell, _ = cb.segments()
    x, y, z = ecef["x"], ecef["y"], ecef["z"]
    r = 2.0 * math.sqrt(3.0) * 0.001  # the octree's decoded positions lie within this of the input
    for k, rings in enumerate(polys):
        l = 1 + 2 * k
        # the lists are the bounding rectangle's
        assert np.array_equal(node_lists[l], node_lists[l + 1]) and np.array_equal(cell_lists[l], cell_lists[l + 1]), k
        assert np.array_equal(tnode[int(tfirst[l]):int(tfirst[l + 1])], node_lists[l]) and np.array_equal(ccell[int(cfirst[l]):int(cfirst[l + 1])], cell_lists[l])
        assert all(np.array_equal(a, b) for a, b in zip(shapes.polygon(l), rings))
        # the segments are the host chain's: projection, then the rule (and the interval)
        for batch, first, every_first, every in ((tb, tfirst, int(tfirst[0]), tnode), (cb, cfirst, int(cfirst[0]), ccell)):
            _, ids, _ = batch.segments()
            where = {int(n): every_first + j for j, n in enumerate(ids[every_first:int(first[1])])}
            for seg in range(int(first[l]), int(first[l + 1])):
                p = batch.points(where[int(ids[seg])], 1)
                pu, pv = pcv.wmr_project(p["x"], p["y"], p["z"])
                keep = P.contains_web_mercator(rings, pu, pv)
                assert np.array_equal(keep, pcv.polygon_contains(rings, p["x"], p["y"], p["z"], frame=1).astype(bool))
                if ivs[l] is not None:
                    a = p["intensity"].astype(np.float64)
                    keep &= (ivs[l][0] <= a) & (a <= ivs[l][1])
                got = batch.points(seg, 1)
                for f in FIELDS:
                    assert np.array_equal(got[f], p[f][keep]), (k, seg, f)
        # the two clouds keep the same points (told apart by their index colours), among those whose verdict does not depend on
        # the octree's quantization: the cube of half-edge r around the input point has all its corners on one side (the polygons'
        # edges are metres long and meet at wide angles, so no edge cuts such a cube without parting its corners)
        own = pcv.polygon_contains(rings, x, y, z, frame=1)
        safe = np.ones(x.size, dtype=bool)
        for sx in (-r, r):
            for sy in (-r, r):
                for sz in (-r, r):
                    safe &= pcv.polygon_contains(rings, x + sx, y + sy, z + sz, frame=1) == own
        assert int((~safe).sum()) < 0.01 * x.size
        a = ecef["inten"].astype(np.float64)
        want = own.astype(bool) & ((ivs[l][0] <= a) & (a <= ivs[l][1]) if ivs[l] is not None else True)
        from_tree, from_cloud = _index_of(tb.shape_points(l)["rgb"]), _index_of(cb.shape_points(l)["rgb"])
        assert np.array_equal(np.sort(from_cloud), np.nonzero(want)[0])  # the S2 cloud holds the input's f64 as they are
        safe_set = set(np.nonzero(safe)[0].tolist())
        assert set(from_tree.tolist()) & safe_set == set(from_cloud.tolist()) & safe_set, k
    counts = [cb.shape_points(1 + 2 * k)["count"] for k in range(len(polys))]
    print(f"web-mercator polygons keep {counts} of {x.size} points")
    assert counts[3] == x.size and counts[4] == 0 and all(0 < c < x.size for c in counts[:3])
    # single-location forms over the octree
    single = tree.query_points(shapes, 3, interval=ivs[3])
    whole = tb.shape_points(3)
    assert single["count"] == whole["count"] and all(np.array_equal(single[f], whole[f]) for f in FIELDS)
    keep, kept = ctx.cull_points(shapes, 1, x, y, z)
    assert np.array_equal(keep, pcv.polygon_contains(polys[0], x, y, z, frame=1)) and kept == int(keep.sum())
    for o in (tb, cb, shapes):
        o.free()


def test_write_ply_over_a_polygon_batch(ctx, scene, tmp_path):
    tree, specs = scene["tree"], scene["specs"]
    shapes = ctx.shapes([specs["hole"], specs["slab"]])
    batch = tree.query_batch(shapes)
    for l in range(2):
        want = batch.shape_points(l)
        path = tmp_path / f"polygon_{l}.ply"
        assert batch.write_ply(path, shape=l) == want["count"] > 0
        got = pcv.read_ply(path)
        assert np.array_equal(got["x"], want["x"]) and np.array_equal(got["y"], want["y"]) and np.array_equal(got["z"], want["z"])
        assert np.array_equal(got["color"].reshape(-1, 3), want["rgb"].reshape(-1, 3)) and np.array_equal(got["intensity"], want["intensity"])
        rows, layout = batch.ply_rows(shape=l)
        assert layout["stride"] == pcv.ply_layout(dict(color="u8vec3", intensity="f32"))["stride"] == rows.shape[1]
        rec = rows.view(layout["dtype"]).ravel()
        assert np.array_equal(rec["x"], want["x"]) and np.array_equal(rec["intensity"], want["intensity"])
    batch.free()
    shapes.free()


def test_refusals(ctx, scene, ecef):
    tree, specs = scene["tree"], scene["specs"]
    L = pcv._lib
    tri = np.array([[0.1, 0.1], [0.6, 0.2], [0.3, 0.7]])

    def message(fn):
        with pytest.raises(pcv.PcvError) as e:
            fn()
        assert e.value.code == pcv.PCV_E_INVALID
        return str(e.value)

    assert "fewer than 3 vertices" in message(lambda: ctx.shapes([("polygon", [tri[:2]], -INF, INF)]))
    assert "is not finite" in message(lambda: ctx.shapes([("polygon", [np.array([[0.0, 0.0], [1.0, np.nan], [1.0, 1.0]])], -INF, INF)]))
    many = P.regular(40000, 50.0, 50.0, 40.0)
    assert "more than 65535 vertices" in message(lambda: ctx.shapes([("polygon", [many, many[:25536]], -INF, INF)]))
    assert "outside [0, 1)" in message(lambda: ctx.shapes([("polygon_web_mercator", [tri * 2.0])]))
    arr = (L.Shape * 1)()
    arr[0].kind = L.SHAPE_POLYGON
    h = pcv.octree.C.c_void_p()
    C = pcv.octree.C
    pf, rf, verts = np.array([0, 1], dtype=np.uint32), np.array([0, 3], dtype=np.uint32), np.ascontiguousarray(tri)

    def create(reserved, params, fn="ex2"):
        arr[0].reserved = reserved
        for j in range(3):
            arr[0].params[j] = params[j]
        if fn == "ex2":
            return ctx.lib.pcv_shapes_create_ex2(ctx.handle, arr, 1, 0, None, None, 1, pf.ctypes.data, rf.ctypes.data, verts.ctypes.data, C.byref(h))
        if fn == "ex":
            return ctx.lib.pcv_shapes_create_ex(ctx.handle, arr, 1, 0, None, None, C.byref(h))
        return ctx.lib.pcv_shapes_create(ctx.handle, arr, 1, C.byref(h))

    assert "polygon index out of range" in message(lambda: ctx._check(create(1, (-INF, INF, 0.0))))
    assert "polygon index out of range" in message(lambda: ctx._check(create(-1, (-INF, INF, 0.0))))
    assert "the frame is 0 (xy) or 1 (web-mercator)" in message(lambda: ctx._check(create(0, (-INF, INF, 2.0))))
    assert "the frame is 0 (xy) or 1 (web-mercator)" in message(lambda: ctx._check(create(0, (-INF, INF, float("nan")))))
    assert "has no height range" in message(lambda: ctx._check(create(0, (0.0, INF, 1.0))))
    assert "needs its rings" in message(lambda: ctx._check(create(0, (-INF, INF, 0.0), "ex")))
    assert "needs its rings" in message(lambda: ctx._check(create(0, (-INF, INF, 0.0), "plain")))
    # a table that holds a polygon
    shapes = ctx.shapes([("aabb", scene["bmin"], scene["bmax"]), specs["hole"], ("polygon_web_mercator", [tri])])
    assert "pcv_shapes_polygon gives its rings" in message(lambda: shapes.get(1))
    assert "pcv_shapes_polygon gives its rings" in message(lambda: shapes.get(2))
    assert "is not a polygon" in message(lambda: shapes.polygon(0))
    for what, fn in (("pcv_cull_nodes", lambda: tree.cull_nodes(shapes)), ("pcv_cull_nodes_sparse", lambda: tree.cull_nodes_sparse(shapes, 4, with_sizes=False)),
                     ("pcv_visible_nodes", lambda: tree.visible_nodes(shapes))):
        text = message(fn)
        assert what in text and "shape 1 is a polygon" in text, text
    assert "every shape must be a frustum" in message(lambda: tree.render(shapes, 64, 64))
    # an S2 cloud takes the web-mercator frame only
    text = message(lambda: ecef["cloud"].cells_in_location_indices(shapes))
    assert "shape 1" in text and "a polygon in the xy frame has no meaning over an ECEF cell cloud" in text
    assert "a polygon in the xy frame has no meaning over an ECEF cell cloud" in message(lambda: ecef["cloud"].query_batch(shapes))
    shapes.free()


def test_the_c_example_prints_the_counts(ctx, scene, tmp_path):
    tree, specs = scene["tree"], scene["specs"]
    tree.write_dir(tmp_path / "oct")
    _, rings, _, _ = specs["hole"]
    with open(tmp_path / "hole.txt", "w") as f:
        f.write("\n\n".join("\n".join(f"{float(a)!r} {float(b)!r}" for a, b in r) for r in rings) + "\n")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "examples"), "bin/query_to_ply"])
    out = subprocess.run([os.path.join(ROOT, "examples", "bin", "query_to_ply"), str(tmp_path / "oct"), "--polygon", str(tmp_path / "hole.txt"),
                          "--z", "5,12.25", "--output", str(tmp_path / "hole.ply")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    shapes = ctx.shapes([("polygon", rings, 5.0, 12.25)])
    batch = tree.query_batch(shapes)
    first, node, off = batch.segments()
    want = [f"  node {int(node[k])}: {int(off[k + 1] - off[k])} points" for k in range(int(first[1]))]
    lines = out.stdout.splitlines()
    assert [l for l in lines if l.startswith("  node ")] == want and len(want) > 3, out.stdout
    whole = batch.shape_points(0)
    assert f"{whole['count']} points written to" in lines[0]
    got = pcv.read_ply(tmp_path / "hole.ply")
    assert np.array_equal(got["x"], whole["x"]) and np.array_equal(got["z"], whole["z"])
    batch.free()
    shapes.free()
