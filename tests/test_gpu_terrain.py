"""Terrain layers on the device (csrc/pcv_terrain.hip) against tests/terrain_truth.py, byte for byte: tile list,
heights (height and quad mask), colours, counts and the counters. Shapes are the smallest that cross every boundary: tile
sizes 4 and 16, point counts 1, 63, 64, 65, 257 and 100 003, tiles at negative positions, seams, ties, contention."""
import json
import os

import numpy as np
import pytest

import point_cloud_viewer_amd as pcv
from point_cloud_viewer_amd import _lib as L
from point_cloud_viewer_amd import synthetic

import terrain_truth as TT
from test_terrain_cpu import EXACT, GENERAL, lib_params

pytestmark = pytest.mark.gpu
STATS = ["max", "min", "mean"]


@pytest.fixture(scope="module")
def ctx():
    c = pcv.Context(0)
    yield c
    c.close()


def colours(n, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, 3), dtype=np.uint8)


def results(t):
    info = t.info()
    return dict(tiles=t.tiles(), heights=t.heights(), colors=t.colors(), counts=t.counts(), info=info)


def run(ctx, p, lo, hi, x, y, z, rgb, calls=1, device=False, **more):
    t = ctx.terrain_begin(lo, hi, params=lib_params(p, **more))
    try:
        cuts = np.linspace(0, len(x), calls + 1).astype(int)
        for a, b in zip(cuts[:-1], cuts[1:]):
            part = [np.ascontiguousarray(v[a:b]) for v in (x, y, z, rgb)]
            if device:
                import torch
                part = [torch.from_numpy(v).to(f"cuda:{ctx.device}") for v in part]
            t.add_points(*part)
        t.finish()
        return results(t)
    finally:
        t.free()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_same(got, want, n=None):
    assert np.array_equal(got["tiles"], want["tiles"]), (got["tiles"], want["tiles"])
    assert np.array_equal(got["counts"], want["counts"])
    assert np.array_equal(got["colors"], want["colors"])
    assert np.array_equal(bits(got["heights"]), bits(want["heights"]))
    if "info" in got and "outside" in want:
        inf = got["info"]
        assert inf["outside"] == want["outside"] and inf["set_vertices"] == want["set_vertices"], (inf, want["outside"], want["set_vertices"])
        assert inf["rendered_quads"] == want["rendered_quads"] and inf["tiles"] == len(want["tiles"]) and inf["finished"]
        assert inf["pool_bytes"] == 0  # the accumulators go at finish
        if n is not None:
            assert inf["points_added"] == n


def assert_property(res, T):
    """The geometry shader's requirement over the assembled tiles."""
    if len(res["tiles"]) == 0:
        return
    _, _, masks = TT.assemble(res["tiles"], res["heights"][..., 1], T)
    _, _, alpha = TT.assemble(res["tiles"], res["colors"][..., 3], T)
    assert np.array_equal(masks, np.floor(masks)) and masks.max() <= 511
    assert TT.check_property(masks.astype(np.uint32), alpha == 255) == []


# ---- seams ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [4, 16])
@pytest.mark.parametrize("corner", [(0, 0), (3, 2), (-5, -1)])
@pytest.mark.parametrize("stat", STATS)
def test_seams_of_a_two_by_two_block_of_tiles(ctx, T, corner, stat):
    """Vertices set across the four tiles that meet at vertex (cx T, cy T): the quad on the shared corner is whole, a hole
    lies one vertex from it, and the rest is a random pattern dense enough to have rendered quads on both seams."""
    cx, cy = corner[0] * T, corner[1] * T
    rng = np.random.default_rng(T * 100 + corner[0] * 10 + corner[1])
    ii, jj = np.meshgrid(np.arange(cx - T, cx + T), np.arange(cy - T, cy + T))
    on = rng.random(ii.shape) < 0.85
    for di, dj in ((-1, -1), (0, -1), (-1, 0), (0, 0)):
        on[T + dj, T + di] = True  # the quad whose corners lie in four tiles
    on[T, T + 1] = False           # a hole one vertex from it
    i, j = ii[on].astype(np.float64), jj[on].astype(np.float64)
    reps = rng.integers(1, 4, i.size)
    i, j = np.repeat(i, reps), np.repeat(j, reps)
    x, y = i + rng.uniform(-0.49, 0.49, i.size), j + rng.uniform(-0.49, 0.49, i.size)
    z = rng.normal(0.0, 30.0, i.size)
    rgb = colours(i.size, 1)
    p = TT.params(tile_size=T, resolution_m=1.0, statistic=stat)
    lo, hi = [cx - T, cy - T, -200.0], [cx + T - 1, cy + T - 1, 200.0]
    want = TT.reduce(p, lo, hi, x, y, z, rgb)
    got = run(ctx, p, lo, hi, x, y, z, rgb)
    assert len(want["tiles"]) == 4 and want["tiles"].min() == min(corner) - 1 and want["rendered_quads"] > 4
    assert_same(got, want, len(x))
    assert_property(got, T)
    # the corner quad is rendered: its four vertices, one in each tile, share a bit; the hole's quads are not
    i0, j0, masks = TT.assemble(got["tiles"], got["heights"][..., 1], T)
    m = lambda a, b: int(masks[b - j0, a - i0])
    assert m(cx - 1, cy - 1) & m(cx, cy - 1) & m(cx - 1, cy) & m(cx, cy)
    assert m(cx + 1, cy) == 0 and (m(cx, cy) & m(cx, cy + 1) & m(cx + 1, cy + 1)) == 0


# ---- sizes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 100_003])
@pytest.mark.parametrize("T", [4, 16])
def test_point_counts_round_the_wave_and_the_block(ctx, n, T):
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


# ---- ties and order --------------------------------------------------------------------------------------------------
def tie_points():
    """Distinct f64 heights that round to one f32, +-0 heights, exact duplicates — with different colours."""
    pts = []
    for k in range(40):  # vertex (0, 0): 1 + k 1e-12 all round to 1.0f
        pts.append((0.1, -0.1, 1.0 + k * 1e-12, (k * 5 % 256, 255 - k, k)))
    for k, zz in enumerate([0.0, -0.0, 1e-60, -1e-60, 0.0, -0.0]):  # vertex (1, 0): +0 and -0, also from roundings
        pts.append((1.0, 0.2, zz, (10 * k, 7, 200 - k)))
    for k in range(9):  # vertex (5, 3), in the next tile: one point nine times, and one twin with another colour
        pts.append((5.2, 2.9, -3.25, (1, 2, 3)))
    pts.append((5.2, 2.9, -3.25, (1, 2, 4)))
    for k in range(30):  # vertex (-2, -3): heights both sides of a tie at the top and at the bottom
        pts.append((-2.0, -3.0, [7.5, 7.5, -7.5, -7.5, 0.5][k % 5], (k, k * 3 % 256, 77)))
    x, y, z = (np.array([q[a] for q in pts], dtype=np.float64) for a in range(3))
    return x, y, z, np.array([q[3] for q in pts], dtype=np.uint8)


@pytest.mark.parametrize("stat", STATS)
def test_ties_and_order_do_not_reach_the_bytes(ctx, stat):
    x, y, z, rgb = tie_points()
    p = TT.params(tile_size=4, resolution_m=1.0, statistic=stat)
    lo, hi = [-4.0, -4.0, -10.0], [7.0, 7.0, 10.0]
    want = TT.reduce(p, lo, hi, x, y, z, rgb)
    # what the rules say, read off the truth: the largest colour among the points at 1.0f; -0 < +0
    ti, tj, hh = TT.assemble(want["tiles"], want["heights"][..., 0], 4)
    _, _, cc = TT.assemble(want["tiles"], want["colors"], 4)
    if stat == "max":
        assert hh[0 - tj, 0 - ti] == np.float32(1.0) and tuple(cc[0 - tj, 0 - ti]) == tuple(max(map(tuple, rgb[:40].tolist()))) + (255,)
        assert bits(hh[0 - tj, 1 - ti]) == 0 and tuple(cc[3 - tj, 5 - ti]) == (1, 2, 4, 255)
    if stat == "min":
        assert bits(hh[0 - tj, 1 - ti]) == 0x80000000
    for seed in range(3):
        order = np.random.default_rng(seed).permutation(len(x))
        for calls in (1, 3, 17):
            got = run(ctx, p, lo, hi, x[order], y[order], z[order], rgb[order], calls=calls)
            assert_same(got, want, len(x))


# ---- contention -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["one vertex", "four vertices round a tile corner"])
def test_contention(ctx, where):
    n = 200_000
    rng = np.random.default_rng(9)
    if where == "one vertex":
        x, y = rng.uniform(2.6, 3.4, n), rng.uniform(-1.4, -0.6, n)
    else:
        x, y = rng.uniform(-1.4, 0.4, n), rng.uniform(14.6, 16.4, n)  # i in {-1, 0}, j in {15, 16}: one vertex in each of four tiles
    z = np.round(rng.normal(100.0, 900.0, n), 2)  # many repeated heights among distinct ones
    z[:50] = z.max()  # and a fifty-fold tie at the top, colours apart
    rgb = colours(n, 10)
    lo, hi = [-20.0, -20.0, -1e4], [20.0, 20.0, 1e4]
    for stat in STATS:
        p = TT.params(tile_size=16, resolution_m=1.0, statistic=stat)
        want = TT.reduce(p, lo, hi, x, y, z, rgb)
        assert want["set_vertices"] == len(want["tiles"]) == (1 if where == "one vertex" else 4) and want["outside"] == 0
        assert_same(run(ctx, p, lo, hi, x, y, z, rgb), want, n)


# ---- thresholds and drops ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stat", STATS)
def test_thresholds_and_drops_leave_no_trace(ctx, stat):
    rng = np.random.default_rng(21)
    n = 5000
    x, y, z = rng.uniform(-12.0, 12.0, n), rng.uniform(-12.0, 12.0, n), rng.normal(0.0, 3.0, n)
    x[:300] = rng.uniform(14.0, 400.0, 300)       # outside the declared box (beyond its one-vertex margin)
    y[300:500] = rng.uniform(-1e9, -14.0, 200)
    x[500:520], y[520:540], z[540:560] = np.nan, np.inf, -np.inf
    z[560:580] = np.nan
    x[580:590] = 1e300                             # u overflows nothing but is far out; 1e308 / res would
    y[590:600] = -1.7e308
    z[600:640] = [1e39, -1e39, 3.5e38, -3.5e38] * 10  # finite in f64, not in f32
    z[640:700] = rng.choice([2.0 ** 21, -2.0 ** 21, 2.0 ** 21 + 1, 2.0 ** 30, 2.0 ** 21 - 0.001], 60)  # MEAN's bound; finite f32 otherwise
    fmax, mid = float(np.finfo(np.float32).max), 2.0 ** 128 - 2.0 ** 103
    z[700:706] = [np.nextafter(fmax, np.inf), -np.nextafter(mid, 0.0), mid, -mid, fmax, -fmax]  # FLT_MAX after rounding, or none
    x[700:706], y[700:706] = [1.0, 1.0, 1.0, 1.0, 1.0, 1.0], 2.0  # four of them stay, on one vertex (MAX, MIN): it is set
    rgb = colours(n, 22)
    p = TT.params(tile_size=4, resolution_m=0.5, statistic=stat, min_points=3)
    lo, hi = [-12.0, -12.0, -50.0], [12.0, 12.0, 50.0]
    want = TT.reduce(p, lo, hi, x, y, z, rgb)
    assert want["outside"] >= 640 and (stat != "mean" or want["outside"] > 660) and 0 < want["set_vertices"]
    assert ((want["counts"] > 0) & (want["counts"] < 3)).any()  # vertices below the threshold are there, unset
    got = run(ctx, p, lo, hi, x, y, z, rgb, calls=2)
    assert_same(got, want, n)
    assert_property(got, 4)
    unset = got["counts"] < 3
    assert not bits(got["heights"])[unset].any() and not got["colors"][unset].any()
    # the same points without the dropped ones: the same bytes
    keep = np.ones(n, bool)
    keep[:640] = False
    kept = TT.reduce(p, lo, hi, x[keep], y[keep], z[keep], rgb[keep])
    again = run(ctx, p, lo, hi, x[keep], y[keep], z[keep], rgb[keep])
    assert again["info"]["outside"] == kept["outside"]
    if stat != "mean":  # MEAN drops most of the 60 tall points besides, so its count differs; its bytes are checked above
        for k in ("tiles", "counts", "colors"):
            assert np.array_equal(again[k], got[k])
        assert np.array_equal(bits(again["heights"]), bits(got["heights"]))


# ---- frames ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(EXACT))
def test_exact_frames(ctx, name):
    iso = [3_900_000.25, -12.5, 5_000_000.0] + EXACT[name]
    n = 20_011
    rng = np.random.default_rng(31)
    x, y, z = (rng.normal(c, 15.0, n) for c in iso[:3])
    rgb = colours(n, 32)
    lo, hi = [v - 70.0 for v in iso[:3]], [v + 70.0 for v in iso[:3]]
    for stat in ("max", "mean"):
        p = TT.params(tile_size=16, resolution_m=0.4, origin=(0.1, 0.2, -0.3), world_from_terrain=iso, statistic=stat)
        got = run(ctx, p, lo, hi, x, y, z, rgb)
        assert_same(got, TT.reduce(p, lo, hi, x, y, z, rgb), n)
    assert got["info"]["set_vertices"] > 1000


def test_a_general_frame_lands_every_point_on_the_host_twins_vertex(ctx):
    """The device's chain is the host twin's, bit for bit, for a rounded matrix too: the reduction over the twin's (i, j, h)
    of every point equals the device's — counts, winners and all."""
    iso = [6_378_137.0 * 0.6, -6_378_137.0 * 0.5, 6_378_137.0 * 0.62] + GENERAL
    n = 100_003
    rng = np.random.default_rng(41)
    x, y, z = (rng.uniform(c - 20.0, c + 20.0, n) for c in iso[:3])
    rgb = colours(n, 42)
    lo, hi = [v - 21.0 for v in iso[:3]], [v + 21.0 for v in iso[:3]]
    for stat in ("max", "min"):
        p = TT.params(tile_size=16, resolution_m=0.05, world_from_terrain=iso, statistic=stat)
        i, j, h, ok = pcv.terrain_vertex(lib_params(p), x, y, z)
        twin = dict(i=i, j=j, h=h, ok=ok, dz=h.astype(np.float64))
        cx = np.array([[hi[a] if c >> a & 1 else lo[a] for a in range(3)] for c in range(8)])
        ci, cj, _, cok = pcv.terrain_vertex(lib_params(p, ), cx[:, 0], cx[:, 1], cx[:, 2])
        assert cok.all()
        want = TT.reduce(p, lo, hi, x, y, z, rgb, vertices=twin)
        got = run(ctx, p, lo, hi, x, y, z, rgb)
        assert got["info"]["vertex_min"] == (ci.min() - 1, cj.min() - 1) and got["info"]["vertex_max"] == (ci.max() + 1, cj.max() + 1)
        assert_same(got, want, n)
        assert want["outside"] == 0 and want["set_vertices"] > 50_000  # most points alone on their vertex


# ---- clouds ---------------------------------------------------------------------------------------------------------
CENTRE = [4_000_000.0, 3_000_000.0, 3_950_000.0]  # an ECEF place: the same points serve the octree and the S2 cloud
CLOUD_N = 200_000


@pytest.fixture(scope="module")
def cloud_points():
    x, y, z, rgb, bmin, bmax = synthetic.gaussian_clusters(CLOUD_N, seed=5, num_clusters=7, extent=90.0, sigma_range=(1.0, 9.0), offset=CENTRE)
    return x, y, z, rgb, bmin, bmax


def cloud_params(stat, **more):
    return TT.params(tile_size=16, resolution_m=0.5, origin=(0.0, 0.0, 0.0), world_from_terrain=CENTRE + EXACT["halves"], statistic=stat, **more)


def check_cloud(ctx, cloud, bmin, bmax):
    mid = (np.asarray(bmin) + np.asarray(bmax)) / 2
    shapes = ctx.shapes([("all",), ("aabb", np.asarray(bmin) - 1.0, [mid[0], bmax[1] + 1.0, bmax[2] + 1.0])])
    batch = cloud.query_batch(shapes)
    first, _, off = batch.segments()
    sizes = np.diff(off.astype(np.int64))
    assert batch.num_segments > 4 and sizes.max() > 100
    for shape in (0, 1, None):
        pts = batch.shape_points(shape) if shape is not None else batch.points()
        assert pts["count"] > 10_000
        for stat in (STATS if shape == 0 else ["max"]):
            p = cloud_params(stat)
            want = TT.reduce(p, bmin, bmax, pts["x"], pts["y"], pts["z"], pts["rgb"])
            kw = dict(tile_size=16, resolution_m=0.5, world_from_terrain=p["world_from_terrain"], statistic=stat)
            # the default piece; a piece smaller than the large segments (they are cut inside, pieces straddle the small ones); one
            # that ends in the middle of a segment
            assert sizes.max() > 1009
            for staging in (0, 1009, int(sizes[sizes > 0][0]) + int(sizes.max()) // 2):
                t = batch.terrain(shape=shape, bbox_min=bmin, bbox_max=bmax, staging_points=staging, **kw)
                assert_same(results(t), want, pts["count"])
                t.free()
    # the clouds' own method: all points, the cloud's box
    t = cloud.terrain(tile_size=16, resolution_m=0.5, world_from_terrain=CENTRE + EXACT["halves"])
    pts = batch.shape_points(0)
    box = (cloud.bbox_min, cloud.bbox_max) if isinstance(cloud, pcv.S2Cloud) else (cloud.meta()["bbox_min"], cloud.meta()["bbox_max"])
    assert_same(results(t), TT.reduce(cloud_params("max"), box[0], box[1], pts["x"], pts["y"], pts["z"], pts["rgb"]), pts["count"])
    assert_property(results(t), 16)
    t.free()
    batch.free()
    shapes.free()


def test_an_octree_through_the_query_adder(ctx, cloud_points):
    x, y, z, rgb, bmin, bmax = cloud_points
    tree = ctx.build(0.001, pcv.Aabb(bmin, bmax), x, y, z, rgb, max_points_per_node=4000)
    try:
        check_cloud(ctx, tree, bmin, bmax)
    finally:
        tree.free()


def test_an_s2_cloud_through_the_query_adder(ctx, cloud_points):
    x, y, z, rgb, bmin, bmax = cloud_points
    cloud = ctx.s2_split(dict(x=x, y=y, z=z, color=rgb), 19)
    try:
        assert cloud.num_cells > 4
        check_cloud(ctx, cloud, bmin, bmax)
    finally:
        cloud.free()


# ---- directory ----------------------------------------------------------------------------------------------------------
def test_the_directory_round_trips(ctx, tmp_path):
    n = 3000
    rng = np.random.default_rng(51)
    x, y, z = rng.uniform(-30.0, 25.0, n), rng.uniform(-8.0, 40.0, n), rng.normal(0.0, 2.0, n)
    rgb = colours(n, 52)
    iso = [0.5, -0.25, 100.0] + EXACT["z +90"]
    p = TT.params(tile_size=16, resolution_m=1.25, origin=(0.1, 1e-7, -0.0), world_from_terrain=iso, statistic="mean", min_points=2)
    lo, hi = [-30.0, -8.0, -10.0], [25.0, 40.0, 10.0]
    t = ctx.terrain_begin(lo, hi, params=lib_params(p))
    t.add_points(x, y, z, rgb).finish()
    res = results(t)
    out = tmp_path / "layer"
    t.write(out)
    t.free()
    assert_same(res, TT.reduce(p, lo, hi, x, y, z, rgb), n)
    tiles = res["tiles"]
    assert len(tiles) > 4 and tiles.min() < 0
    want_files = {"meta.json"} | {f"{pcv.terrain_tile_name(a, b)}.{ext}" for a, b in tiles for ext in ("height", "color")}
    assert set(os.listdir(out)) == want_files
    for a, b in tiles:
        assert os.path.getsize(out / f"{pcv.terrain_tile_name(a, b)}.height") == 16 * 16 * 8
        assert os.path.getsize(out / f"{pcv.terrain_tile_name(a, b)}.color") == 16 * 16 * 4
    meta = json.load(open(out / "meta.json"))
    assert meta["tile_positions"] == tiles.tolist() == sorted(tiles.tolist()) and meta["tile_size"] == 16
    assert open(out / "meta.json").read() == pcv.terrain_meta_json(lib_params(p), tiles)
    back = pcv.read_terrain(out)
    assert np.array_equal(back["tiles"], tiles) and np.array_equal(bits(back["heights"]), bits(res["heights"]))
    assert np.array_equal(back["colors"], res["colors"]) and back["tile_size"] == 16 and back["resolution_m"] == 1.25
    assert np.array_equal(back["world_from_terrain"], iso) and np.array_equal(back["origin"].view(np.uint64), np.float64([0.1, 1e-7, -0.0]).view(np.uint64))


def test_a_terrain_without_a_set_vertex_writes_meta_only(ctx, tmp_path):
    p = TT.params(tile_size=4, resolution_m=1.0, min_points=2)
    t = ctx.terrain_begin([0, 0, 0], [10, 10, 10], params=lib_params(p))
    t.add_points(np.array([1.0, 5.0, 500.0]), np.array([1.0, 5.0, 5.0]), np.array([1.0, 2.0, 3.0]), np.zeros((3, 3), np.uint8)).finish()
    inf = t.info()
    assert (inf["points_added"], inf["outside"], inf["set_vertices"], inf["tiles"], inf["rendered_quads"]) == (3, 1, 0, 0, 0)
    assert t.tiles().shape == (0, 2) and t.heights().shape == (0, 4, 4, 2) and t.counts().shape == (0, 4, 4)
    t.write(tmp_path / "empty")
    t.free()
    assert os.listdir(tmp_path / "empty") == ["meta.json"]
    assert json.load(open(tmp_path / "empty" / "meta.json"))["tile_positions"] == []
    assert len(pcv.read_terrain(tmp_path / "empty")["tiles"]) == 0


def test_build_terrain_from_directories(ctx, tmp_path, cloud_points):
    x, y, z, rgb, bmin, bmax = (a[:30_000] if np.ndim(a) and len(a) == CLOUD_N else a for a in cloud_points)
    tree = ctx.build(0.001, pcv.Aabb(bmin, bmax), x, y, z, rgb, max_points_per_node=3000)
    every = tree.query_batch(ctx.shapes([("all",)]))
    pts = every.points()
    every.free()
    tree.write_dir(str(tmp_path / "octree"))
    tree.free()
    kw = dict(tile_size=16, resolution_m=0.5, world_from_terrain=CENTRE + EXACT["halves"], statistic="min")
    t = pcv.build_terrain(ctx, [str(tmp_path / "octree")], str(tmp_path / "layer"), **kw)
    res = results(t)
    t.free()
    opened = ctx.open_dir(str(tmp_path / "octree"))
    box = opened.meta()
    opened.free()
    assert_same(res, TT.reduce(cloud_params("min"), box["bbox_min"], box["bbox_max"], pts["x"], pts["y"], pts["z"], pts["rgb"]), len(x))
    back = pcv.read_terrain(tmp_path / "layer")
    assert np.array_equal(back["tiles"], res["tiles"]) and np.array_equal(bits(back["heights"]), bits(res["heights"]))


# ---- limits -------------------------------------------------------------------------------------------------------------
def test_limits(ctx):
    # vertices 1 .. 8191 widen to 0 .. 8192: 2049 x 2049 tiles of 4; one vertex less is 2048 x 2048 = 2^22, which is allowed
    with pytest.raises(pcv.PcvError, match="2\\^22") as e:
        ctx.terrain_begin([1, 1, 0], [8191, 8191, 1], tile_size=4, resolution_m=1.0)
    assert e.value.code == L.PCV_E_INVALID
    ctx.terrain_begin([1, 1, 0], [8190, 8190, 1], tile_size=4, resolution_m=1.0).free()
    with pytest.raises(pcv.PcvError) as e:
        ctx.terrain_begin([0, 0, 0], [np.inf, 1, 1], tile_size=4, resolution_m=1.0)
    assert e.value.code == L.PCV_E_INVALID
    # a pool cap of one tile: 16 vertices x (8 + 4) bytes for MAX
    before = ctx.pool_stats()[0]
    t = ctx.terrain_begin([0, 0, 0], [20, 20, 1], tile_size=4, resolution_m=1.0, max_pool_bytes=16 * 12)
    t.add_points(np.array([1.0, 2.0]), np.array([1.0, 2.0]), np.zeros(2), np.zeros((2, 3), np.uint8))  # one tile: fits
    assert t.info()["pool_bytes"] == 16 * 12 and t.info()["tiles"] == 1
    with pytest.raises(pcv.PcvError, match="max_pool_bytes") as e:
        t.add_points(np.array([1.0, 9.0]), np.array([1.0, 9.0]), np.zeros(2), np.zeros((2, 3), np.uint8))
    assert e.value.code == L.PCV_E_OOM
    assert ctx.pool_stats()[0] == before and t.info()["pool_bytes"] == 0
    with pytest.raises(pcv.PcvError, match="only be freed"):
        t.finish()
    t.free()
    assert ctx.pool_stats()[0] == before
    # finished terrains take no points; unfinished ones give no tiles
    t = ctx.terrain_begin([0, 0, 0], [20, 20, 1], tile_size=4, resolution_m=1.0)
    with pytest.raises(pcv.PcvError, match="not finished"):
        t.tiles()
    t.finish()
    with pytest.raises(pcv.PcvError, match="no more points"):
        t.add_points(np.zeros(1), np.zeros(1), np.zeros(1), np.zeros((1, 3), np.uint8))
    t.free()
    assert ctx.pool_stats()[0] == before
