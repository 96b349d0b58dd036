"""pcv_xray_run_many (xray leaf tiles over several octrees, as build_xray_quadtree with several point_cloud_locations)
against xray_many_oracle, and against pcv_xray_run: the union box, the created set, kept / drawn sums, every tile's RGBA,
the parents and the quadtree directory, one raster launch per pass whatever the number of octrees, and the errors."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import point_cloud_viewer_amd as pcv
import xray_many_oracle as M
from point_cloud_viewer_amd import synthetic
from test_gpu_query import ctx  # noqa: F401  (module fixture)
import xray_truth as T
from test_gpu_xray import ISO, check_close, check_colored_exact, tree_points

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, PX = 64, 1.0  # the union below spans 256 ..= 512 m: 3 levels, 64 leaf tiles of 64 m


def make_scene(ctx, n, seed, res, offset, extent, with_intensity, cap, pad=None):  # noqa: F811
    x, y, z, rgb, inten, bmin, bmax = T.many_cloud(n, seed, res, offset, extent, with_intensity, cap, pad)
    tree = ctx.build(res, pcv.Aabb(bmin, bmax), x, y, z, rgb, inten, max_points_per_node=cap)
    with O.max_points_per_node(cap):
        want = O.build_closed(res, bmin, bmax, x, y, z, rgb, inten, threads=4)
    names = tree.node_names()
    return dict(bmin=bmin, bmax=bmax, tree=tree, oracle=want, names=names, index_of={m: i for i, m in enumerate(names)})


@pytest.fixture(scope="module")
def scenes(ctx):  # noqa: F811
    """a: 0.001 m, intensity; b: 0.05 m (other node encodings), no intensity, overlapping a, its meta box padded by 100 m
    in +y (the union's max y, with no point near it); c: 0.002 m, intensity, disjoint from both"""
    return [make_scene(ctx, *args) for args in T.MANY]


@pytest.fixture(scope="module")
def tps(scenes):
    return [tree_points(s) for s in scenes]


@pytest.fixture(scope="module")
def points(tps):
    """the oracle's kept points per tile, once per query setting"""
    cache = {}

    def get(key, iso=None):
        if key not in cache:
            cache[key] = M.tile_points(tps, W, PX, iso)
        return cache[key]
    return get


def run(ctx, trees, strategy="xray", **kw):  # noqa: F811
    xt = ctx.xray_tiles(trees, kw.pop("tile_size_px", W), kw.pop("pixel_size_m", PX), strategy, **kw)
    imgs = xt.images() if xt.num_created else np.zeros((0, W, W, 4), np.uint8)
    return xt, {n: (imgs[i], int(xt.drawn[i])) for i, n in enumerate(xt.created_ids)}


def run_one(tree, strategy="xray", **kw):
    xt = tree.xray_tiles(kw.pop("tile_size_px", W), kw.pop("pixel_size_m", PX), strategy, **kw)
    imgs = xt.images() if xt.num_created else np.zeros((0, W, W, 4), np.uint8)
    return xt, {n: (imgs[i], int(xt.drawn[i])) for i, n in enumerate(xt.created_ids)}


def check_against_oracle(xt, got, want, g):
    assert xt.deepest_level == g["deepest_level"] and xt.leaf_ids == g["leaf_ids"]
    assert tuple(xt.bounding_rect) == g["rect"]
    assert xt.created_ids == [n for n in g["leaf_ids"] if n in want]  # leaf order
    assert [int(k) for k in xt.kept] == [want[n][2] for n in xt.created_ids]
    for n, (img, drawn, _) in want.items():
        assert got[n][1] == drawn, n
        assert np.array_equal(got[n][0], img), (n, int((got[n][0] != img).any(-1).sum()))


def test_scenes_differ(scenes, tps):
    encs = [{s["tree"].node(i).encoding for i in range(s["tree"].num_nodes) if s["tree"].node(i).num_points} for s in scenes]
    assert encs[0] != encs[1], encs  # different resolutions: different node encodings
    lo, hi = M.union_box(tps)
    assert lo == tuple(float(min(s["bmin"][a] for s in scenes)) for a in range(3))
    assert hi == tuple(float(max(s["bmax"][a] for s in scenes)) for a in range(3))
    assert hi[1] == float(scenes[1]["bmax"][1]) and lo[1] == float(scenes[2]["bmin"][1]) and hi[0] == float(scenes[2]["bmax"][0])


@pytest.mark.parametrize("background", ["white", "transparent"])
def test_xray_over_three_octrees_matches_oracle(ctx, scenes, tps, points, background):  # noqa: F811
    trees = [s["tree"] for s in scenes]
    xt, got = run(ctx, trees, "xray", background=background)
    want, g = M.xray_tiles(tps, W, "xray", background, points=points("plain"))
    assert g["deepest_level"] == 3 and 4 < len(want) < 64
    # tiles that only one of the octrees reaches, and tiles that two share
    single = [n for n in want if sum(k > 0 for k in g["kept_per_octree"][n]) == 1]
    assert 0 < len(single) < len(want)
    check_against_oracle(xt, got, want, g)


def test_xray_over_three_octrees_with_query_from_global(ctx, scenes, tps, points):  # noqa: F811
    xt, got = run(ctx, [s["tree"] for s in scenes], "xray", query_from_global=ISO)
    want, g = M.xray_tiles(tps, W, "xray", points=points("iso", ISO))
    assert len(want) > 4
    check_against_oracle(xt, got, want, g)


def test_colored_and_height_stddev_over_three_octrees(ctx, scenes, tps, points):  # noqa: F811
    trees = [s["tree"] for s in scenes]
    xt, got = run(ctx, trees, "colored")
    want, _ = M.xray_tiles(tps, W, "colored", points=points("plain"))
    assert [int(k) for k in xt.kept] == [want[n][2] for n in xt.created_ids]
    check_colored_exact(got, *points("plain"))
    check_close(got, {n: v[:2] for n, v in want.items()}, 0.98)
    intervals = T.stddev_intervals(*points("plain"), W)
    for cmap in ("jet", "purplish"):
        strat = ("height_stddev", 1.5, cmap)
        _, got = run(ctx, trees, strat, background="transparent")
        T.stddev_check(got, *points("plain"), W, 1.5, cmap, "transparent", intervals)
        want, _ = M.xray_tiles(tps, W, strat, "transparent", points=points("plain"))
        check_close(got, {n: v[:2] for n, v in want.items()}, 0.0)


def same_quadtree(a, b, exact=True):
    """a, b: XrayTiles; the leaf lists, kept / drawn, every node and its image (exact, or equal alpha and RGB within 2:
    a leaf pixel within 1 can move a 2:1 Lanczos3 parent pixel by a little more)"""
    assert a.leaf_ids == b.leaf_ids and a.created_ids == b.created_ids and a.deepest_level == b.deepest_level
    assert tuple(a.bounding_rect) == tuple(b.bounding_rect)
    assert np.array_equal(a.kept, b.kept) and np.array_equal(a.drawn, b.drawn)
    a.build_parents()
    b.build_parents()
    assert a.node_ids == b.node_ids
    ia, ib = a.node_images(), b.node_images()
    if exact:
        assert np.array_equal(ia, ib)
    else:
        assert np.array_equal(ia[..., 3], ib[..., 3]) and np.abs(ia.astype(int) - ib.astype(int)).max() <= 2


@pytest.mark.parametrize("kw", [dict(), dict(query_from_global=ISO), dict(intensity_interval=(10.0, 120.5)),
                                dict(query_from_global=ISO, intensity_interval=(30.0, 200.0), background="transparent")])
def test_one_octree_list_equals_xray_run(ctx, scenes, kw):  # noqa: F811
    """xray and colored byte for byte, parents included. height_stddev sums f64 in the order records reach their
    bucket, which two runs of pcv_xray_run do not share either: its node images close, alpha exact."""
    tree = scenes[0]["tree"]
    for strat in ("xray", "colored", ("height_stddev", 1.5, "purplish")):
        a, _ = run(ctx, [tree], strat, pixel_size_m=0.25, **kw)  # 16 m tiles over tree a's ~110 m
        b, _ = run_one(tree, strat, pixel_size_m=0.25, **kw)
        assert a.num_created > 8
        # height_stddev keeps the slack: its leaves are pinned to an interval of the true deviation, not to bytes, and two
        # runs may round an ambiguous pixel differently (f64 LDS atomics in scheduling order)
        same_quadtree(a, b, exact=isinstance(strat, str))
        a.free()
        b.free()


def test_same_octree_twice(ctx, scenes):  # noqa: F811
    tree = scenes[0]["tree"]
    for strat in ("xray", "colored"):
        a, _ = run(ctx, [tree, tree], strat)
        b, _ = run(ctx, [tree], strat)
        assert a.created_ids == b.created_ids
        assert np.array_equal(a.kept, 2 * b.kept) and np.array_equal(a.drawn, 2 * b.drawn)
        a.build_parents()
        b.build_parents()
        assert a.node_ids == b.node_ids and np.array_equal(a.node_images(), b.node_images()), strat


def test_one_launch_per_raster_pass(ctx, scenes):  # noqa: F811
    tree = scenes[0]["tree"]
    counts = []
    ctx.set_profiling(True)
    try:
        for trees in ([tree], [tree] * 4):
            ctx.reset_kernel_stats()
            xt, _ = run(ctx, trees, "xray")
            st = ctx.kernel_stats()
            counts.append({k: st[k][0] for k in ("xray_bin_kernel", "xray_scatter_kernel", "xray_accum_kernel")})
            xt.free()
    finally:
        ctx.set_profiling(False)
    assert counts[0] == counts[1] == {"xray_bin_kernel": 1, "xray_scatter_kernel": 1, "xray_accum_kernel": 1}, counts


def test_groups_across_octrees(ctx, scenes):  # noqa: F811
    trees = [s["tree"] for s in scenes] + [scenes[0]["tree"]]
    for strat in ("xray", "colored"):
        xa, a = run(ctx, trees, strat)
        xb, b = run(ctx, trees, strat, max_workspace_bytes=3_000_000)  # a few tiles per group
        assert list(a) == list(b) and np.array_equal(xa.kept, xb.kept) and np.array_equal(xa.drawn, xb.drawn)
        assert int(xa.kept.sum()) * 8 > 3_000_000  # more than one group
        for n in a:
            assert np.array_equal(a[n][0], b[n][0]), (strat, n)


def test_errors(ctx, scenes):  # noqa: F811
    a, b = scenes[0]["tree"], scenes[1]["tree"]
    with pytest.raises(ValueError):
        ctx.xray_tiles([], W, PX)
    p = pcv._lib.XrayParams(tile_size_px=W, pixel_size_m=PX)
    h = C.c_void_p(1)
    arr = (C.c_void_p * 2)(a.handle, None)
    assert ctx.lib.pcv_xray_run_many(ctx.handle, arr, 0, C.byref(p), C.byref(h)) == pcv.PCV_E_INVALID
    assert "No locations specified" in ctx.lib.pcv_last_error(ctx.handle).decode() and not h.value
    assert ctx.lib.pcv_xray_run_many(ctx.handle, arr, 2, C.byref(p), C.byref(h)) == pcv.PCV_E_INVALID
    assert "octree 1 is null" in ctx.lib.pcv_last_error(ctx.handle).decode() and not h.value
    many = (C.c_void_p * (pcv._lib.XRAY_MAX_TREES + 1))(*([a.handle] * (pcv._lib.XRAY_MAX_TREES + 1)))
    assert ctx.lib.pcv_xray_run_many(ctx.handle, many, pcv._lib.XRAY_MAX_TREES + 1, C.byref(p), C.byref(h)) == pcv.PCV_E_INVALID
    assert "PCV_XRAY_MAX_TREES" in ctx.lib.pcv_last_error(ctx.handle).decode()
    with pytest.raises(pcv.PcvError, match="has no intensity"):
        ctx.xray_tiles([a, b], W, PX, intensity_interval=(0.0, 100.0))
    with pytest.raises(pcv.PcvError, match="only intensity"):
        p2 = pcv._lib.XrayParams(tile_size_px=W, pixel_size_m=PX, interval_attribute=b"color")
        ctx._check(ctx.lib.pcv_xray_run_many(ctx.handle, arr, 1, C.byref(p2), C.byref(h)))
    other = pcv.Context(0)
    try:
        x, y, z, rgb, bmin, bmax = synthetic.gaussian_clusters(5_000, seed=3, num_clusters=2, extent=20.0)
        t2 = other.build(0.001, pcv.Aabb(bmin, bmax), x, y, z, rgb)
        with pytest.raises(pcv.PcvError, match="another context"):
            ctx.xray_tiles([a, t2], W, PX)
        t2.free()
    finally:
        other.close()
    xt, _ = run(ctx, [a, b], "xray")  # the context still works
    assert xt.num_created > 0


def test_quadtree_directory_and_example(ctx, scenes, tmp_path):  # noqa: F811
    a, b = scenes[0]["tree"], scenes[2]["tree"]
    a.write_dir(str(tmp_path / "a"))
    b.write_dir(str(tmp_path / "b"))
    xt = ctx.xray_quadtree([a, b], W, PX, "colored", background="transparent", intensity_interval=(10.0, 200.0))
    xt.write(tmp_path / "py")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "examples")])
    exe = os.path.join(ROOT, "examples", "bin", "build_xray_quadtree")
    p = subprocess.run([exe, str(tmp_path / "a"), str(tmp_path / "b"), "--output-directory", str(tmp_path / "c"), "--resolution",
                        str(PX), "--tile-size", str(W), "--coloring-strategy", "colored", "--tile-background-color", "transparent",
                        "--filter-interval", "intensity=10,200"], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr
    names = sorted(os.listdir(tmp_path / "py"))
    assert names == sorted(os.listdir(tmp_path / "c")) and "meta.pb" in names and len(names) > 10
    for n in names:
        assert (tmp_path / "py" / n).read_bytes() == (tmp_path / "c" / n).read_bytes(), n
    xt.free()
