"""The products that tests/test_gpu_pool_guard.py runs under the pool's guard: each case is a function of a fresh context (and
a scratch directory) that runs one product at a small shape and asserts it against the truth its own GPU test uses, through
that test's helpers. A case returns the objects that still hold device memory, for the test to scan their fences before it
frees them. Truths that cost more than a moment are computed once and kept for the three fills."""
import functools

import numpy as np

import oracle_lib as O
import point_cloud_viewer_amd as pcv
from point_cloud_viewer_amd import synthetic

CASES = {}


def case(fn):
    CASES[fn.__name__] = fn
    return fn


# ---- octree builds (test_gpu_build) ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _capacity_cloud():
    x, y, z, rgb, bmin, bmax = synthetic.gaussian_clusters(60_000, seed=9, num_clusters=5, extent=20.0, sigma_range=(0.001, 0.5))
    x[:3000], y[:3000], z[:3000] = x[0], y[0], z[0]  # duplicates: resolution-limited nodes above capacity
    inten = (np.arange(x.size) % 1000).astype(np.float32) * 0.25
    with O.max_points_per_node(500):
        plain = O.build_closed(0.01, bmin, bmax, x, y, z, rgb, threads=4)
        with_int = O.build_closed(0.01, bmin, bmax, x, y, z, rgb, inten, threads=4)
    return x, y, z, rgb, inten, bmin, bmax, plain, with_int


def _build(ctx, single_chain, intensity):
    from test_gpu_build import assert_same
    x, y, z, rgb, inten, bmin, bmax, plain, with_int = _capacity_cloud()
    t = ctx.build(0.01, pcv.Aabb(bmin, bmax), x, y, z, rgb, inten if intensity else None, max_points_per_node=500, single_chain=single_chain)
    assert t.build_info()["single_chain"] == bool(single_chain)
    assert_same(t.to_dict(), with_int if intensity else plain, check_intensity=intensity)
    return [t]


@case
def build_staged_tables(ctx, tmp):
    return _build(ctx, False, False)


@case
def build_single_chain_8_byte_records(ctx, tmp):
    return _build(ctx, True, False)


@case
def build_single_chain_12_byte_records(ctx, tmp):
    return _build(ctx, True, True)


@functools.lru_cache(maxsize=None)
def _special_cloud():
    from test_gpu_build import special_coordinates_cloud
    x, y, z, rgb, boxes = special_coordinates_cloud()
    lo, hi, _ = boxes[1]
    with O.max_points_per_node(900):
        want = O.build_closed(1e-7, lo, hi, x, y, z, rgb, threads=4)
    assert max(nd["level"] for nd in want.nodes.values()) > 21  # deeper than one key word holds
    return x, y, z, rgb, lo, hi, want


@case
def build_two_word_keys(ctx, tmp):
    from test_gpu_build import assert_same
    x, y, z, rgb, lo, hi, want = _special_cloud()
    held = []
    for single_chain in (None, True):
        t = ctx.build(1e-7, pcv.Aabb(lo, hi), x, y, z, rgb, max_points_per_node=900, single_chain=single_chain)
        assert_same(t.to_dict(), want)
        held.append(t)
    return held


# ---- streamed and out-of-core builds (test_gpu_ingest, test_gpu_out_of_core) ------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ragged_stream():
    sizes = [1, 1, 1, 7, 64, 1023, 1024, 1025]
    n = sum(sizes)
    x, y, z, rgb, _, _ = synthetic.gaussian_clusters(n, seed=62 + len(sizes), num_clusters=3, extent=120.0, sigma_range=(0.1, 4.0),
                                                     offset=(-2.7e6, -4.3e6, 3.8e6))
    inten = (np.arange(n, dtype=np.int64) * 7919 % 10_007).astype(np.float32) * 0.125 - 3.0
    lo, hi = np.array([x.min(), y.min(), z.min()]), np.array([x.max(), y.max(), z.max()])
    with O.max_points_per_node(3_000):
        want = O.build_closed(0.001, lo, hi, x, y, z, rgb, inten, threads=8).nodes
    return sizes, x, y, z, rgb, inten, lo, hi, want


@case
def streamed_build_of_ragged_batches(ctx, tmp):
    from test_gpu_ingest import batches, same_tree
    sizes, x, y, z, rgb, inten, lo, hi, want = _ragged_stream()
    ing = ctx.ingest(x.size, has_intensity=True)
    for b in batches(x, y, z, rgb, inten, sizes):
        ing.append(b["position"], b["color"], b["intensity"])
    tree = ing.finish(0.001, None, max_points_per_node=3_000)
    meta = tree.meta()
    assert np.array_equal(meta["bbox_min"], lo) and np.array_equal(meta["bbox_max"], hi)
    same_tree(tree.to_dict(), want, check_intensity=True)
    return [tree]


@functools.lru_cache(maxsize=None)
def _deep_duplicates():
    """The cloud of test_duplicates_deep_tree_empty_buckets_unsplit_octant_and_small_partition."""
    rng = np.random.default_rng(3)
    lone = rng.uniform(1.0, 9.0, (3_000, 3))
    dup = np.full((200_000, 3), 60.123456789)
    dup[::3] += rng.normal(0, 1e-7, (dup[::3].shape[0], 3))
    spread = rng.uniform(50.0, 100.0, (200_000, 3))
    pos = np.concatenate([lone, dup, spread])[rng.permutation(403_000)]
    x, y, z = (np.ascontiguousarray(pos[:, k]) for k in range(3))
    rgb = rng.integers(0, 256, (x.size, 3), dtype=np.uint8)
    first = dup.shape[0] + int(np.all(spread < 75.0, axis=1).sum())
    return x, y, z, rgb, first


@case
def out_of_core_build_in_three_passes(ctx, tmp):
    from test_gpu_out_of_core import in_core, out_of_core, same_dir
    x, y, z, rgb, first = _deep_duplicates()
    bmin, bmax = np.zeros(3), np.full(3, 100.0)
    in_core(ctx, tmp / "in", 1e-9, bmin, bmax, x, y, z, rgb, None, 4_000)
    st = out_of_core(ctx, tmp / "ooc", 1e-9, bmin, bmax, x, y, z, rgb, None, 4_000, first + 1_500)
    assert st["partitions"] == 3 and st["split_mask"] == 0x80 and st["routed"] == 0, st
    same_dir(tmp / "ooc", tmp / "in")
    return []


# ---- terrain (test_gpu_terrain) -----------------------------------------------------------------------------------------------------
@case
def terrain_three_statistics_and_a_seam(ctx, tmp):
    import terrain_truth as TT
    from test_gpu_terrain import STATS, assert_property, assert_same, colours, run
    n, T = 257, 4  # test_point_counts_round_the_wave_and_the_block
    rng = np.random.default_rng(n + T)
    x, y = rng.uniform(-37.0, 41.0, n), rng.uniform(-29.0, 23.0, n)
    z = rng.normal(5.0, 20.0, n)
    rgb = colours(n, n)
    lo, hi = [-37.0, -29.0, -100.0], [41.0, 23.0, 100.0]
    for stat in STATS:
        p = TT.params(tile_size=T, resolution_m=0.75, origin=(0.3, -0.2, 1.0), statistic=stat)
        got = run(ctx, p, lo, hi, x, y, z, rgb, device=(stat == "max"))
        assert_same(got, TT.reduce(p, lo, hi, x, y, z, rgb), n)
        assert_property(got, T)
    # test_seams_of_a_two_by_two_block_of_tiles at corner (-5, -1)
    corner = (-5, -1)
    cx, cy = corner[0] * T, corner[1] * T
    rng = np.random.default_rng(T * 100 + corner[0] * 10 + corner[1])
    ii, jj = np.meshgrid(np.arange(cx - T, cx + T), np.arange(cy - T, cy + T))
    on = rng.random(ii.shape) < 0.85
    for di, dj in ((-1, -1), (0, -1), (-1, 0), (0, 0)):
        on[T + dj, T + di] = True
    on[T, T + 1] = False
    i, j = ii[on].astype(np.float64), jj[on].astype(np.float64)
    reps = rng.integers(1, 4, i.size)
    i, j = np.repeat(i, reps), np.repeat(j, reps)
    x, y = i + rng.uniform(-0.49, 0.49, i.size), j + rng.uniform(-0.49, 0.49, i.size)
    z = rng.normal(0.0, 30.0, i.size)
    rgb = colours(i.size, 1)
    lo, hi = [cx - T, cy - T, -200.0], [cx + T - 1, cy + T - 1, 200.0]
    for stat in STATS:
        p = TT.params(tile_size=T, resolution_m=1.0, statistic=stat)
        want = TT.reduce(p, lo, hi, x, y, z, rgb)
        assert len(want["tiles"]) == 4 and want["rendered_quads"] > 4
        got = run(ctx, p, lo, hi, x, y, z, rgb)
        assert_same(got, want, len(x))
        assert_property(got, T)
    return []


# ---- map tiles (test_gpu_maptiles) ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _map_cloud():
    import maptiles_truth as MT
    cloud = MT.main_cloud()
    want = MT.reduce(19, *cloud)
    return cloud, want, MT.parents(19, 17, want["tiles"], want["images"])


@case
def map_tiles_in_seven_calls_parents_and_files(ctx, tmp):
    import maptiles_truth as MT
    from test_gpu_maptiles import ZOOM, assert_same, results, run
    cloud, want, truth = _map_cloud()
    x, y, z, rgb = cloud
    n = len(x)
    res = run(ctx, ZOOM, x, y, z, rgb, device=True, cuts=np.array([0, 1, 64, 65, 321, 7000, 7001, n]), staging_points=1000)
    assert_same(res, want, n)
    m = ctx.map_tiles_begin(ZOOM).add_points(*cloud).finish().build_parents(17)
    assert_same(results(m), want, n)
    for zoom in range(17, ZOOM + 1):
        tiles, images = truth[zoom]
        assert np.array_equal(m.tiles(zoom), tiles)
        assert np.array_equal(m.images(zoom), images), zoom
    m.write(tmp / "tiles", png="deflate")
    for zoom in (17, 18, 19):
        images, files = m.images(zoom), m.tile_pngs(zoom, png="deflate")
        for k, (a, b) in enumerate(m.tiles(zoom).tolist()):
            data = open(tmp / "tiles" / str(zoom) / str(a) / f"{b}.png", "rb").read()
            assert data == files[k]
            assert np.array_equal(pcv.png_decode(data), images[k])
    # the edge set
    ex, ey, ez = MT.edge_points(ZOOM)
    ergb = np.random.default_rng(4).integers(0, 256, (len(ex), 3), dtype=np.uint8)
    assert_same(run(ctx, ZOOM, ex, ey, ez, ergb, device=True), MT.reduce(ZOOM, ex, ey, ez, ergb), len(ex))
    return [m]


# ---- LAS (test_gpu_las) ----------------------------------------------------------------------------------------------------------------
@case
def las_filter_extras_and_parked_colours(ctx, tmp):
    import las_truth as T
    from test_gpu_las import check, fields
    n = 700
    raw = T.pack_records(7, fields(7, n), 1)  # stride 37
    check(ctx, 7, raw, n, extra=1, pieces=(100,), extras=T.extras_of(7), keep_intensity=True)
    check(ctx, 7, raw, n, extra=1, pieces=(100,), classes=[1, 2, 3, 5, 8, 13, 21, 200], drop_withheld=True, extras=["gps_time"])
    # colour AUTO on both sides of 255 / 256: every piece parks its 16-bit colours until the last record decides
    n = 500
    f = fields(3, n)
    for top, rule in ((255, "rgb8"), (256, "rgb16")):
        f["r"][:], f["g"][:], f["b"][:] = f["r"] % 256, f["g"] % 255, f["b"] % 200
        f["classification"][:] = 2
        f["classification"][-1], f["b"][-1] = 7, top
        want = check(ctx, 3, T.pack_records(3, f), n, pieces=(100,), classes=[2])
        assert want["info"]["color_rule"] == rule and want["info"]["max_color"] == top and want["info"]["num_kept"] == n - 1
    return []


# ---- batched queries (test_gpu_query_batch, test_gpu_wmr, test_gpu_polygon_query, test_gpu_union_query) ---------------------------
@functools.lru_cache(maxsize=None)
def _query_cloud():
    x, y, z, rgb, bmin, bmax = synthetic.gaussian_clusters(60_000, seed=2, num_clusters=6, extent=100.0, sigma_range=(0.5, 6.0))
    inten = (np.arange(x.size) % 251).astype(np.float32)
    with O.max_points_per_node(2000):
        want = O.build_closed(0.001, bmin, bmax, x, y, z, rgb, inten, threads=4)
    return x, y, z, rgb, inten, bmin, bmax, want


@case
def query_batch_of_72_frusta_boxes_and_all(ctx, tmp):
    """The scene of test_gpu_query at 60 000 points; eight tables of mixed_shapes in one batch: past a wave of 64 shapes."""
    from test_gpu_query_batch import check_against_oracle, mixed_shapes
    x, y, z, rgb, inten, bmin, bmax, want = _query_cloud()
    tree = ctx.build(0.001, pcv.Aabb(bmin, bmax), x, y, z, rgb, inten, max_points_per_node=2000)
    names = tree.node_names()
    sc = dict(bmin=bmin, bmax=bmax, tree=tree, oracle=want, names=names, index_of={n: i for i, n in enumerate(names)})
    shapes, kinds, ivs = [], [], []
    for seed in range(30, 38):
        s, k = mixed_shapes(sc, seed)
        shapes += s
        kinds += k
        ivs += [None, (20.0, 180.0), (180.0, 20.0), (float("nan"), 100.0), None, (20.0, 180.0), (5.0, float("nan")), None, (20.0, 180.0)]
    assert len(shapes) == 72
    prepared = ctx.shapes(shapes)
    batch = tree.query_batch(prepared, intervals=ivs)
    assert check_against_oracle(sc, batch, kinds, ivs) >= 20
    return [batch, prepared, tree]


@case
def query_batch_of_68_shapes_of_every_kind(ctx, tmp):
    """test_gpu_polygon_query's mixed table (polygon, AABB, OBB, both frusta, AllPoints, map tile, cell union) four times over."""
    from test_gpu_polygon_query import check_polygon_segments, make_scene, mixed_table
    s = make_scene(ctx)
    table, ivs = mixed_table(s)
    table, ivs = table * 4, ivs * 4
    assert len(table) == 68
    shapes = ctx.shapes(table)
    batch, counts = check_polygon_segments(s["tree"], table, shapes, ivs, 2)
    n = len(counts) // 4
    assert all(counts[k] == counts[k % n] for k in range(len(counts))) and counts[1] > 0 and counts[3] == 0
    # the other kinds are what they are in a table without polygons
    others = [l for l, spec in enumerate(table) if spec[0] != "polygon"]
    plain = ctx.shapes([table[l] for l in others])
    pb = s["tree"].query_batch(plain, [ivs[l] for l in others])
    for k, l in enumerate(others):
        a, b = batch.shape_points(l), pb.shape_points(k)
        assert a["count"] == b["count"] and all(np.array_equal(a[f], b[f]) for f in ("x", "y", "z", "rgb", "intensity")), l
    return [pb, plain, batch, shapes, s["shapes"], s["tree"]]


@case
def query_cell_unions_over_the_octree(ctx, tmp):
    from test_gpu_union_query import _check_points, make_scene
    s = make_scene(ctx)
    lo, hi = np.quantile(s["inten"], [0.2, 0.7])
    intervals = [None] * len(s["table"])
    for l in (1, 3, 9, 10):
        intervals[l] = (float(lo), float(hi))
    counts = _check_points(ctx, s, s["tree"], intervals)
    assert 0 < counts[1] and 0 < counts[10] < s["x"].size
    return [s["shapes"], s["tree"]]


@functools.lru_cache(maxsize=None)
def _ground_cloud():
    """test_gpu_wmr's city-scale ECEF cloud at a seventh of its points: u8, u16, f32 and f64 nodes in one octree."""
    rot, ground = synthetic.ecef_from_local(37.407204, -122.147604)
    x, y, z, rgb, bmin, bmax = synthetic.gaussian_clusters(48_000, seed=12, num_clusters=6, extent=30000.0, sigma_range=(5.0, 400.0),
                                                           offset=tuple(ground - 15000.0))
    rng = np.random.default_rng(13)
    up = ground + 1000.0 * rot[:, 2]
    near = int(np.argmin((x - up[0]) ** 2 + (y - up[1]) ** 2 + (z - up[2]) ** 2))
    c = np.array([x[near], y[near], z[near]])
    x = np.concatenate([x, c[0] + rng.normal(0.0, 0.03, 10_000)])
    y = np.concatenate([y, c[1] + rng.normal(0.0, 0.03, 10_000)])
    z = np.concatenate([z, c[2] + rng.normal(0.0, 0.03, 10_000)])
    rgb = synthetic.index_colors(x.size)
    bmin, bmax = np.array([x.min(), y.min(), z.min()]), np.array([x.max(), y.max(), z.max()])
    inten = (np.arange(x.size) % 251).astype(np.float32)
    with O.max_points_per_node(1500):
        want = O.build_closed(0.001, bmin, bmax, x, y, z, rgb, inten, threads=8)
    return x, y, z, rgb, inten, bmin, bmax, c, want


@case
def query_batch_of_map_tile_rectangles(ctx, tmp):
    import wmr_oracle as W
    from test_gpu_query import random_frusta
    from test_gpu_wmr import center_uv, check_batch, shape_of
    x, y, z, rgb, inten, bmin, bmax, c, want = _ground_cloud()
    tree = ctx.build(0.001, pcv.Aabb(bmin, bmax), x, y, z, rgb, inten, max_points_per_node=1500)
    names = tree.node_names()
    sc = dict(bmin=bmin, bmax=bmax, tree=tree, oracle=want, names=names, index_of={n: i for i, n in enumerate(names)}, center=c)
    assert len({tree.node(i).encoding for i in range(tree.num_nodes) if tree.node(i).num_points > 0}) >= 3
    cu, cv = center_uv(c)
    # the grids of test_wmr_cpu.py around the centre, a rectangle that misses the cloud, one that holds it and one that wraps in x
    rects = W.grid(cu, cv, 7, 1e-6) + W.grid(cu, cv, 4, 2.5e-7) + [(cu + 0.01, cv + 0.01, cu + 0.012, cv + 0.012),
                                                                  (cu - 0.0019, cv - 0.0019, cu + 0.0019, cv + 0.0019),
                                                                  (255.5 / 256.0, cv - 0.001, 0.5 / 256.0, cv + 0.001)]
    fr = random_frusta(np.random.default_rng(5), bmin, bmax, 1)
    shapes = [("all",), ("frustum", fr[0][0])] + [shape_of(r) for r in rects]
    kinds = [(O.SHAPE_ALL, None), (O.SHAPE_FRUSTUM, fr[0][0])] + [("wmr", r) for r in rects]
    assert len(shapes) >= 65
    ivs = [(20.0, 180.0) if k % 3 == 0 else None for k in range(len(shapes))]
    prepared = ctx.shapes(shapes)
    batch = tree.query_batch(prepared, intervals=ivs)
    kept = check_batch(sc, batch, kinds, ivs)
    assert kept["wmr"] > 5_000 and kept["other"] > 5_000, kept
    return [batch, prepared, tree]


# ---- visible nodes and a rendered frame (visible_cases, test_gpu_render_outline, test_gpu_render_terrain) --------------------------
@functools.lru_cache(maxsize=None)
def _visible_truth():
    import visible_cases as VC
    import visible_mirror as VM
    tree, cases = VC.oracle_tree("A"), VC.fixed_cases("A")
    mats = [m for _, m in cases]
    return tree, cases, VC.oracle_lists(tree.nodes, mats), [VM.traverse(VC.BMIN, VC.BMAX, tree.nodes, m) for m in mats]


@case
def visible_nodes_of_the_fixed_views(ctx, tmp):
    import visible_cases as VC
    _, cases, wants, mirrors = _visible_truth()
    x, y, z, rgb = VC.cloud("A")
    tree = ctx.build(VC.RESOLUTION, pcv.Aabb(VC.BMIN, VC.BMAX), x, y, z, rgb, max_points_per_node=VC.MAX_POINTS_PER_NODE)
    names = tree.node_names()
    shapes = ctx.shapes([("frustum", m) for _, m in cases])
    vis, status = tree.visible_nodes(shapes)
    for f, ((tag, _), want, mirror) in enumerate(zip(cases, wants, mirrors)):
        assert status[f] == mirror.status, (tag, status[f], mirror)
        if want is not None:
            assert [names[i] for i in vis[f]] == want, tag
        elif mirror.status == 1:
            assert len(vis[f]) == 0, tag
        else:
            assert len(vis[f]) == mirror.listed <= mirror.panic_after, (tag, len(vis[f]), mirror)
    assert (status == 0).sum() >= 8 and (status == 1).sum() >= 3 and (status == 2).sum() >= 3
    return [shapes, tree]


_frame = {}


@case
def rendered_frame_with_terrain_and_outlines(ctx, tmp):
    import test_gpu_render_terrain as RT
    from test_gpu_render_outline import build_scene, cloud, frusta
    s = build_scene(ctx, *cloud())
    # the oracle's frames are cached by the identity of the tree nodes and the layer: keep the first fill's for the others
    if "tn" not in _frame:
        _frame["tn"] = s["tn"]
    ground, gd = RT.build_layer(ctx, RT.GROUND, (-8, 6), (-5, 10), lambda i, j: 28.0 + 6.0 * np.sin(0.7 * i) * np.cos(0.5 * j),
                                skip=lambda i, j: 0 <= i < 8 and 0 <= j < 8, single=lambda i, j: (i * 5 + j * 3) % 11 == 0)
    if "gd" in _frame:  # the layer is the same bytes under every fill
        for k in ("tiles", "heights", "colors"):
            assert np.array_equal(np.ascontiguousarray(gd[k]).view(np.uint8), np.ascontiguousarray(_frame["gd"][k]).view(np.uint8)), k
    else:
        _frame["gd"] = gd
    mats, cams = RT.views()
    mats, cams = mats[:3], cams[:3]
    rv = s["tree"].render(frusta(ctx, mats), RT.W, RT.H, point_size=2.0, gamma=2.2, depth=True, show_octree_nodes=True, terrain=[ground],
                          camera_positions=cams, terrain_window=16)
    wants = RT.check_views(rv, _frame["tn"], mats, cams, RT.W, RT.H, [_frame["gd"]], 16, 2.0, 2.2, outlines=True)
    assert wants[0]["outline_pixels"] > 0 and wants[0]["terrain"][0]["pixels_won"] > 0 and wants[0]["nodes_visible"] > 3
    rv.close()
    return [ground, s["tree"]]


# ---- xray (test_gpu_xray, test_gpu_xray_merge, test_gpu_xray_pyramid, test_gpu_xray_png, test_gpu_xray_inpaint) -------------------
_xray_tiles = {}


@case
def xray_tiles_parents_pngs_and_a_merge(ctx, tmp):
    import xray_many_oracle as M
    import xray_oracle as X
    from test_gpu_xray import check_colored_exact, check_exact, run
    from test_gpu_xray_merge import PX, W, assert_same_quadtree, build, make_cloud, shards
    from test_gpu_xray_png import host_pngs
    from test_gpu_xray_pyramid import check_nodes, check_pyramid, pyramid_of
    cloud = make_cloud(ctx)
    tree = cloud["tree"]
    if "tp" not in _xray_tiles:
        from test_gpu_xray import tree_points
        x, y, z, rgb, bmin, bmax = cloud["points"]
        with O.max_points_per_node(2000):
            oracle = O.build_closed(0.001, bmin, bmax, x, y, z, rgb, threads=4)
        tp = tree_points(dict(tree=tree, oracle=oracle, names=tree.node_names(), bmin=bmin, bmax=bmax))
        # (the oracle reads node cubes through the first fill's tree object: read them all now, the tree goes at the case's end)
        _xray_tiles["colored"] = M.tile_points([tp], W, PX)
        _xray_tiles["xray7"] = X.xray_tiles(tp, 7, 1.0, "xray", background="white")
        _xray_tiles["tp"] = True
    # leaf tiles: colored at 16 px against the exact-integer truth, xray at 7 px (ragged tiles) against the oracle
    xt, got = run(tree, "colored", tile_size_px=W, pixel_size_m=PX, background="transparent")
    check_colored_exact(got, *_xray_tiles["colored"], tile_px=W, background="transparent")
    x7, got7 = run(tree, "xray", tile_size_px=7, pixel_size_m=1.0, background="white")
    want7, g7 = _xray_tiles["xray7"]
    assert x7.deepest_level == g7["deepest_level"] and x7.leaf_ids == g7["leaf_ids"]
    check_exact(got7, want7)
    # parents from the leaves, the compressed files against the host encoder
    held = [xt, x7]
    for strategy, bg, tile, px in (("colored", "transparent", W, PX), ("xray", "white", 7, 1.0)):
        q = build(cloud, strategy, bg, tile=tile, px=px)
        nodes = check_nodes(q)
        want, _ = pyramid_of(q, bg)
        check_pyramid(q, want, nodes)
        pngs = q.node_pngs(png="deflate")
        assert len(pngs) == len(q.node_ids) > len(q.created_ids) > 4 and pngs == host_pngs(q)
        held.append(q)
    # a merge of the four level-1 shards is the whole quadtree
    parts = shards(cloud, 1, "colored", "transparent")
    merged = ctx.xray_merge(parts, "transparent")
    assert_same_quadtree(merged, held[2])
    return [merged] + parts + held + [tree]


@case
def xray_inpaint_of_an_opened_quadtree(ctx, tmp):
    from test_gpu_xray_inpaint import CASES as INPAINT, assert_equals_oracle, case as inpaint_case, write_quadtree
    name = "w8_d2_4x4_missing"
    W, d, G, deepest, missing, alpha, blank, bg = INPAINT[name]
    leaves, images, counters, _, _ = inpaint_case(name)
    write_quadtree(tmp / "in", "r", leaves, deepest, W)
    (x,) = ctx.xray_open(tmp / "in")
    out = x.inpaint(d, background=bg)
    assert_equals_oracle(out, images, counters, sorted(leaves))
    total = {k: int(v.sum()) for k, v in out.inpaint_info().items()}
    assert total["target_pixels"] > 0 and total["filled_pixels"] > 0 and total["blended_pixels"] > 0
    return [out, x]


# ---- S2 (test_gpu_s2, test_gpu_s2_stream, test_gpu_s2_attr, test_gpu_s2_query, test_gpu_xray_s2) ------------------------------------
@case
def s2_split_stream_and_a_typed_attribute(ctx, tmp):
    import s2_truth as T
    from test_gpu_s2 import check_split, intensity_of
    from test_gpu_s2_attr import LEVEL, check_columns, columns_for
    from test_gpu_s2_stream import same_cloud, slices, stream_of
    x, y, z, rgb = T.uniform_cloud()
    points = dict(x=x, y=y, z=z, color=rgb, intensity=intensity_of(x.size))
    whole = ctx.s2_split(points)
    ids, counts, _ = check_split(whole, x, y, z, rgb, points["intensity"], 20, T.set_leaf_ids("uniform"))
    assert (ids.size, int(counts.max()), int(counts.min())) == (675, 49, 1)
    stream = stream_of(ctx, points, slices([1, 7, 0, 4999, 1024, None], x.size))
    cloud = stream.finish()
    same_cloud(cloud, whole)
    check_split(cloud, x, y, z, rgb, points["intensity"], 20, T.set_leaf_ids("uniform"))
    # twelve typed columns through the split (test_split_regroups_every_column at n = 4 099)
    n = 4099
    batch = dict(x=x[:n], y=y[:n], z=z[:n], color=rgb[:n], intensity=intensity_of(n), attributes=columns_for(n, 7))
    cells = T.parents(T.set_leaf_ids("uniform")[:n], LEVEL)
    order = np.argsort(cells, kind="stable")
    typed = ctx.s2_split(batch, LEVEL)
    assert np.array_equal(typed.order, order.astype(np.uint32))
    check_columns(typed, batch, order)
    return [typed, cloud, whole]


@case
def s2_query_batch_over_65_cells(ctx, tmp):
    import s2_region_truth as R
    import s2_truth as T
    from test_gpu_s2_query import _expected, _intensity
    specs = R.scene()[6]
    shapes = ctx.shapes(list(specs))
    x, y, z, rgb = R.scene()[:4]
    ids = T.parents(T.set_leaf_ids("uniform"), 20)
    keep_points = np.isin(ids, np.unique(ids)[:65])
    x, y, z, rgb = (np.ascontiguousarray(a[keep_points]) for a in (x, y, z, rgb))
    cloud = ctx.s2_split(dict(x=x, y=y, z=z, color=rgb, intensity=_intensity(x.size)), 20)
    assert cloud.num_cells == 65
    xyz, c, inten = cloud.cell_points()
    px, py, pz = (np.ascontiguousarray(xyz[:, k]) for k in range(3))
    unions = R.scene_unions(20)
    keep = []
    for l, spec in enumerate(specs):
        if spec[0] == "all":
            keep.append(np.ones(x.size, dtype=bool))
        elif spec[0] == "web_mercator_rect":
            keep.append(pcv.wmr_contains(spec, px, py, pz).astype(bool))
        elif spec[0] == "frustum":
            keep.append(np.zeros(x.size, dtype=bool))
        else:
            keep.append(np.asarray(ctx.cull_points(shapes, l, px, py, pz)[0]).astype(bool))
    for cells in unions:
        keep.append(pcv.s2_union_contains(cells, px, py, pz).astype(bool))
    locations = len(specs) + len(unions)
    intervals = [(-3.0, 900.0) if l % 3 == 0 else ((1e9, 2e9) if l % 7 == 1 else None) for l in range(locations)]
    lists = cloud.cells_in_location_indices(shapes, unions)
    want_lists = pcv.s2_cells_in_location(cloud.cells[0], shapes.kinds, [int(shapes.get(i)[2]) for i in range(shapes.count)],
                                          np.array([shapes.get(i)[0] for i in range(shapes.count)]), unions)
    assert all(np.array_equal(g, w) for g, w in zip(lists, want_lists)) and len(lists) == len(want_lists)
    batch = cloud.query_batch(shapes, unions, intervals)
    first, cell, off = batch.segments()
    assert np.array_equal(cell, np.concatenate(lists)) and batch.num_segments == len(cell)
    want = _expected(cloud, lists, keep, intervals, inten)
    sizes = np.concatenate([np.asarray(w[1], dtype=np.uint64) for w in want])
    assert np.array_equal(off, np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64))
    assert batch.num_points == int(sizes.sum()) > 0
    for l, (slots, _) in enumerate(want):
        got = batch.shape_points(l)
        assert got["count"] == slots.size
        assert np.stack([got["x"], got["y"], got["z"]], axis=1).tobytes() == xyz[slots].tobytes(), l
        assert got["rgb"].tobytes() == c[slots].tobytes() and got["intensity"].tobytes() == inten[slots].tobytes(), l
    return [batch, cloud, shapes]


_s2_xray = {}


@case
def xray_over_an_s2_cloud(ctx, tmp):
    import test_gpu_xray_s2 as XS
    import xray_many_oracle as M
    import xray_truth as T
    from test_gpu_xray import check_exact
    cloud, sp = XS.make(ctx, 20)
    _, sh = XS.prepare(ctx, [sp])  # the device's corners of the tile shapes: what the oracle's lists are made from
    if "pts" not in _s2_xray:
        _s2_xray["pts"] = M.tile_points([sp], XS.W, XS.PX, XS.ISO)
        _s2_xray["xray"] = M.xray_tiles([sp], XS.W, "xray", "white", points=_s2_xray["pts"])[0]
    pts = _s2_xray["pts"]
    xt, got = XS.run(ctx, [cloud], "xray", background="white")
    XS.check_tiles(xt, got, _s2_xray["xray"], pts[0])
    xc, gotc = XS.run(ctx, [cloud], "colored", background="transparent")
    check_exact(gotc, T.colored_tiles(pts[0], pts[1], XS.W, "transparent"))
    return [xt, xc, sh, cloud]


# ---- PLY rows (test_gpu_ply_write) -----------------------------------------------------------------------------------------------------
def _check_rows(sc, names, want_stride, tmp, kind):
    import ply_write_truth as PT
    from test_gpu_ply_write import check_scene_is_what_the_tests_need, pick, truth_rows
    batch = sc["batch"]
    first, off = check_scene_is_what_the_tests_need(sc)
    want = truth_rows(sc, names)
    got, layout = batch.ply_rows(attributes=names)
    assert layout["stride"] == want_stride and got.shape == want.shape and got.tobytes() == want.tobytes()
    for s in range(4):  # the four shapes, into device memory
        got, _ = batch.ply_rows(shape=s, attributes=names, device=True)
        a, b = int(off[first[s]]), int(off[first[s + 1]])
        assert tuple(got.shape) == (b - a, want_stride) and got.cpu().numpy().tobytes() == want[a:b].tobytes(), s
    for shape in (0, 1):  # files written in pieces of 63 and of 1 000 points
        a, b = int(off[first[shape]]), int(off[first[shape + 1]])
        for chunk in (63, 1000):
            path = tmp / f"{kind}_{shape}_{chunk}.ply"
            assert batch.write_ply(path, shape=shape, attributes=names, chunk_points=chunk) == b - a
            assert path.read_bytes() == PT.file_bytes(pick(sc, names), [want[a:b]]), (shape, chunk)


@case
def ply_rows_of_an_octree_and_an_s2_batch(ctx, tmp):
    from test_gpu_ply_write import OCTREE_SETS, S2_SETS, make_s2_scene, octree_scene
    sc = octree_scene(ctx, True, 120)
    _check_rows(sc, OCTREE_SETS[0], 31, tmp, "octree")
    s2 = make_s2_scene(ctx)
    _check_rows(s2, S2_SETS[0], 78, tmp, "s2")
    return [sc["batch"], sc["tree"], s2["batch"], s2["cloud"]]
