"""pcv_xray_run_s2 (xray leaf tiles over S2 cell clouds, as build_xray_quadtree runs over S2 directories) against
xray_s2_oracle: every strategy, the created set, kept / drawn / negative, every tile's RGBA; against the brute-force filter of
all points; several clouds, tile groups, the downstream quadtree calls, and the refusals. The oracle lists a tile's cells
with the host twin over the corners the DEVICE computed (Shapes.get), as the existing S2 tests take them, so every created
tile of every case is compared."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import point_cloud_viewer_amd as pcv
import s2_region_truth as R
import xray_inpaint_oracle as IO
import xray_many_oracle as M
import xray_oracle as X
import xray_s2_oracle as S
import xray_truth as T
from point_cloud_viewer_amd import synthetic
from test_gpu_xray import check_exact
from test_gpu_xray_inpaint import assert_equals_oracle
from test_gpu_xray_merge import assert_same_quadtree

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, PX = 64, 0.5  # with the transform: a 512 m rect, 256 leaf tiles of 32 m, 64 of them over the 200 m x 200 m cloud
ISO = S.local_from_ecef()
CORNERS = {}  # (kind, params) -> the (8, 3) corners the device computed for that tile shape


def corners_of(kind, params):
    return CORNERS[(int(kind), tuple(float(v) for v in params))]


def intensity_of(n):
    """the test's own intensity: -20 ..= 232 in steps of 0.25, so about 8 % negative, and one NaN"""
    inten = ((np.arange(n, dtype=np.int64) * 2654435761) % 1009).astype(np.float32) * np.float32(0.25) - np.float32(20.0)
    inten[n // 3] = np.nan
    return inten


def cloud_points(shift_east=0.0):
    x, y, z, rgb = R.scene()[:4]
    if shift_east:
        rot, _ = synthetic.ecef_from_local(S.LAT, S.LNG)
        x, y, z = x + shift_east * rot[0, 0], y + shift_east * rot[1, 0], z + shift_east * rot[2, 0]
    return tuple(np.ascontiguousarray(a) for a in (x, y, z, rgb))


@pytest.fixture(scope="module")
def ctx():
    c = pcv.Context(0)
    yield c
    c.close()


def make(ctx, level, with_intensity=True, shift_east=0.0):
    x, y, z, rgb = cloud_points(shift_east)
    inten = intensity_of(x.size) if with_intensity else None
    pts = dict(x=x, y=y, z=z, color=rgb)
    if with_intensity:
        pts["intensity"] = inten
    return ctx.s2_split(pts, level), S.S2Points(x, y, z, rgb, inten, level, corners_of)


@pytest.fixture(scope="module")
def a20(ctx):
    return make(ctx, 20)


@pytest.fixture(scope="module")
def a16(ctx):
    return make(ctx, 16)


def prepare(ctx, sps, tile=W, px=PX, iso=ISO, root="r"):
    """the leaf tiles' shapes on the device: their corners into CORNERS (what the oracle's lists are made from); returns
    (geometry, Shapes)"""
    g = S.geometry(sps, tile, px, iso, root)
    shapes = S.tile_shapes(g, iso)
    sh = ctx.shapes([S.shape_spec(k, p) for k, p in shapes])
    for i, (k, p) in enumerate(shapes):
        CORNERS[(int(k), tuple(float(v) for v in p))] = sh.get(i)[0]
    return g, sh


def run(ctx, clouds, strategy="xray", tile=W, px=PX, iso=ISO, **kw):
    xt = ctx.xray_tiles(clouds, tile, px, strategy, query_from_global=iso, **kw)
    imgs = xt.images() if xt.num_created else np.zeros((0, tile, tile, 4), np.uint8)
    return xt, {n: (imgs[i], int(xt.drawn[i])) for i, n in enumerate(xt.created_ids)}


def check_tiles(xt, got, want, g):
    """want: {leaf id: (image, drawn, kept)}"""
    assert xt.deepest_level == g["deepest_level"] and xt.leaf_ids == g["leaf_ids"]
    assert tuple(xt.bounding_rect) == g["rect"]
    assert xt.created_ids == [n for n in g["leaf_ids"] if n in want]  # the created set, in leaf order
    assert [int(k) for k in xt.kept] == [want[n][2] for n in xt.created_ids]
    for n, (img, drawn, _) in want.items():
        assert got[n][1] == drawn, n
        assert np.array_equal(got[n][0], img), (n, int((got[n][0] != img).any(-1).sum()))


@pytest.fixture(scope="module")
def scene_points(ctx, a20, a16):
    """per split level: (cloud, S2Points, oracle (geometry, points), Shapes) of the 64 px set-up with the transform"""
    out = {}
    for level, (cloud, sp) in ((20, a20), (16, a16)):
        _, sh = prepare(ctx, [sp])
        out[level] = (cloud, sp, M.tile_points([sp], W, PX, ISO), sh)
    return out


# ---- 1. every strategy on the scene ------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [20, 16])
def test_every_strategy(ctx, scene_points, level):
    cloud, sp, pts, sh = scene_points[level]
    g = pts[0]
    assert cloud.num_cells == sp.cell_ids.size == (675 if level == 20 else 5) and np.array_equal(cloud.cells[0], sp.cell_ids)
    assert np.array_equal(cloud.bbox_min, sp.bmin) and np.array_equal(cloud.bbox_max, sp.bmax)
    assert len(g["leaf_ids"]) == 256 and len(pts[1]) == 64
    first, _, off = cloud.query_batch(sh).segments()
    first = first.astype(np.int64)
    per_location = (off[first[1:]] - off[first[:-1]]).astype(np.int64)
    for bg in ("white", "transparent"):
        xt, got = run(ctx, [cloud], "xray", background=bg)
        want, _ = M.xray_tiles([sp], W, "xray", bg, points=pts)
        check_tiles(xt, got, want, g)
        assert np.array_equal(xt.kept.astype(np.int64), per_location[xt.created.astype(np.int64)])
        assert np.count_nonzero(per_location) == xt.num_created
        xc, gotc = run(ctx, [cloud], "colored", background=bg)
        check_exact(gotc, T.colored_tiles(g, pts[1], W, bg))
        assert np.array_equal(xc.kept, xt.kept) and xc.created_ids == xt.created_ids
    for cmap in ("jet", "purplish"):
        xs, gots = run(ctx, [cloud], ("height_stddev", 1.5, cmap), background="transparent")
        T.stddev_check(gots, *pts, W, 1.5, cmap, "transparent")
        assert np.array_equal(xs.kept, xt.kept)
    # S2Cloud's own methods are the one-cloud list
    own = cloud.xray_tiles(W, PX, "colored", query_from_global=ISO, background="transparent")
    assert own.created_ids == xc.created_ids and np.array_equal(own.images(), xc.images())


# ---- 2. brute force: independent of the listing code -------------------------------------------------------------------------
@pytest.mark.parametrize("level", [20, 16])
def test_images_equal_the_brute_force_layer(ctx, scene_points, level):
    cloud, sp, _, _ = scene_points[level]
    brute, failures = S.brute_tile_points([sp], W, PX, ISO)
    assert failures == []  # the precondition, on the device's corners: no tile is left out
    g = brute[0]
    xt, got = run(ctx, [cloud], "xray")
    want, _ = M.xray_tiles([sp], W, "xray", "white", points=brute)
    check_tiles(xt, got, want, g)
    _, gotc = run(ctx, [cloud], "colored", background="transparent")
    check_exact(gotc, T.colored_tiles(g, brute[1], W, "transparent"))


# ---- 3. many small tiles, and AABB tiles in the ECEF frame -------------------------------------------------------------------
@pytest.mark.parametrize("tile,px,iso,leaves,created", [(32, 0.25, ISO, 4096, 675), (64, 0.5, None, 64, 39)])
def test_other_tilings(ctx, a20, tile, px, iso, leaves, created):
    cloud, sp = a20
    prepare(ctx, [sp], tile, px, iso)
    xt, got = run(ctx, [cloud], "xray", tile, px, iso)
    want, g = M.xray_tiles([sp], tile, "xray", pixel_size_m=px, iso=iso)
    assert (len(g["leaf_ids"]), len(want)) == (leaves, created)
    check_tiles(xt, got, want, g)


# ---- 4. intensity: the filter, colored_with_intensity, binning -----------------------------------------------------------
def test_intensity(ctx, a20):
    cloud, sp = a20
    assert np.isnan(sp.intensity).sum() == 1 and (sp.intensity < 0).sum() > 1000
    g, _ = prepare(ctx, [sp])
    interval = (-5.0, 100.0)
    xt, got = run(ctx, [cloud], "xray", intensity_interval=interval)
    want, _ = M.xray_tiles([sp], W, "xray", pixel_size_m=PX, iso=ISO, interval=interval)
    check_tiles(xt, got, want, g)
    assert 0 < int(xt.kept.sum()) < sp.x.size // 2 and not xt.negative.any()
    for strategy, kw, okw in (("colored_with_intensity", dict(min_intensity=1.0, max_intensity=200.0), dict(lo=1.0, hi=200.0)),
                              ("colored_with_intensity", dict(min_intensity=1.0, max_intensity=200.0, binning=("intensity", 16.0)),
                               dict(lo=1.0, hi=200.0, bin_size=16.0)),
                              ("colored", dict(binning=("intensity", 16.0)), dict(bin_size=16.0)),
                              ("colored_with_intensity", dict(min_intensity=0.5, max_intensity=150.0, intensity_interval=interval),
                               dict(lo=0.5, hi=150.0, interval=interval))):
        xi, goti = run(ctx, [cloud], strategy, background="transparent", **kw)
        wanti, _ = S.intensity_tiles([sp], W, PX, strategy, background="transparent", iso=ISO, **okw)
        assert xi.created_ids == [n for n in g["leaf_ids"] if n in wanti]
        assert [int(k) for k in xi.kept] == [wanti[n][3] for n in xi.created_ids]
        assert [int(k) for k in xi.negative] == [wanti[n][2] for n in xi.created_ids]
        assert (int(xi.negative.sum()) > 0) == (strategy == "colored_with_intensity")
        check_exact(goti, {n: (img, drawn) for n, (img, drawn, _, _) in wanti.items()})
    bare, _ = make(ctx, 20, with_intensity=False)
    for kw in (dict(strategy="xray", intensity_interval=interval), dict(strategy="colored_with_intensity"),
               dict(strategy="colored", binning=("intensity", 16.0))):
        for clouds in ([bare], [cloud, bare]):
            with pytest.raises(pcv.PcvError, match="has no intensity") as e:
                ctx.xray_tiles(clouds, W, PX, query_from_global=ISO, **kw)
            assert e.value.code == pcv.PCV_E_INVALID
    xb, gotb = run(ctx, [bare], "colored")  # without intensity the other strategies run
    assert xb.num_created == 64 and len(gotb) == 64
    bare.free()


# ---- 5. several clouds ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def several(ctx, a20, tmp_path_factory):
    """[A, B, A]: B the same points 150 m to the local east, split at level 18, written and reopened"""
    d = tmp_path_factory.mktemp("s2") / "b"
    split_b, sb = make(ctx, 18, shift_east=150.0)
    split_b.write(str(d))
    opened = ctx.s2_open(d)
    return dict(a=a20[0], b=opened, b_split=split_b, clouds=[a20[0], opened, a20[0]], sps=[a20[1], sb, a20[1]], dir=d)


def test_several_clouds(ctx, several):
    clouds, sps = several["clouds"], several["sps"]
    g, _ = prepare(ctx, sps)
    lo, hi = M.union_box(sps)
    assert np.array_equal(lo, np.minimum(sps[0].bmin, sps[1].bmin)) and np.array_equal(hi, np.maximum(sps[0].bmax, sps[1].bmax))
    assert g["rect"] == X.leaf_geometry(W, PX, lo, hi, ISO)["rect"]
    pts = M.tile_points(sps, W, PX, ISO)
    xt, got = run(ctx, clouds, "xray")
    want, _ = M.xray_tiles(sps, W, "xray", points=pts)
    check_tiles(xt, got, want, g)  # kept and drawn are sums over the three
    per = pts[0]["kept_per_octree"]
    assert any(k[1] == 0 for k in per.values()) and any(k[0] == 0 and k[1] > 0 for k in per.values()) and any(min(k) > 0 for k in per.values())
    _, gotc = run(ctx, clouds, "colored", background="transparent")
    check_exact(gotc, T.colored_tiles(g, pts[1], W, "transparent"))
    # an opened cloud (blobs made resident by the run) equals the split one it was written from
    fresh = ctx.s2_open(several["dir"])
    for strategy in ("xray", "colored"):
        xo, goto = run(ctx, [fresh], strategy)
        xs, gots = run(ctx, [several["b_split"]], strategy)
        assert xo.created_ids == xs.created_ids and np.array_equal(xo.kept, xs.kept) and np.array_equal(xo.drawn, xs.drawn)
        assert np.array_equal(xo.images(), xs.images())
    # the result does not hold its clouds
    fresh.free()
    assert np.array_equal(xo.images(), xs.images())
    with pytest.raises(ValueError):
        ctx.xray_tiles([clouds[0], object()], W, PX)


# ---- 6. tile groups ---------------------------------------------------------------------------------------------------------
def num_groups(kept, strategy_id, workspace):
    p = pcv._lib.XrayParams(tile_size_px=W, pixel_size_m=PX, strategy=strategy_id, max_workspace_bytes=workspace)
    k = np.ascontiguousarray(kept, dtype=np.uint64)
    n = C.c_uint64()
    err = C.create_string_buffer(256)
    assert pcv.load_library().pcv_xray_plan_groups(k.ctypes.data, k.size, C.byref(p), None, 0, C.byref(n), None, err, 256) == 0, err.value
    return n.value


def test_groups(ctx, several):
    a, clouds, sps = several["a"], several["clouds"], several["sps"]
    prepare(ctx, sps)
    prepare(ctx, sps[:1])
    workspace = 60_000  # 64 px tiles: 4 buckets of 16 B each, 8 B per kept point
    launches = {}
    for name, cl in (("one", [a]), ("three", clouds)):
        xa, ga = run(ctx, cl, "xray")
        groups = num_groups(xa.kept, 0, workspace)
        assert groups >= 3
        ctx.set_profiling(True)
        try:
            ctx.reset_kernel_stats()
            xb, gb = run(ctx, cl, "xray", max_workspace_bytes=workspace)
            st = ctx.kernel_stats()
        finally:
            ctx.set_profiling(False)
        launches[name] = ({k: st[k][0] for k in ("xray_bin_kernel", "xray_scatter_kernel", "xray_accum_kernel")}, groups)
        assert list(ga) == list(gb) and np.array_equal(xa.kept, xb.kept) and np.array_equal(xa.drawn, xb.drawn)
        for n in ga:
            assert np.array_equal(ga[n][0], gb[n][0]), (name, n)
        _, gc = run(ctx, cl, "colored")
        _, gd = run(ctx, cl, "colored", max_workspace_bytes=workspace)
        assert all(np.array_equal(gc[n][0], gd[n][0]) for n in gc)
    for name, (st, groups) in launches.items():  # one launch per raster pass and group, whatever the number of clouds
        assert st == {"xray_bin_kernel": groups, "xray_scatter_kernel": groups, "xray_accum_kernel": groups}, (name, st, groups)
    # the far cloud keeps nothing in some of the groups' tiles: those groups run with fewer clouds in their chunk list
    per = M.tile_points(sps, W, PX, ISO)[0]["kept_per_octree"]
    assert sum(k[1] == 0 for k in per.values()) >= 8


# ---- 7. downstream ---------------------------------------------------------------------------------------------------------
def test_quadtree_directory_merge_and_example(ctx, several, tmp_path):
    a = several["a"]
    whole = a.xray_quadtree(W, PX, "colored", query_from_global=ISO, background="transparent", output_directory=tmp_path / "whole")
    back = ctx.xray_open(tmp_path / "whole")
    assert len(back) == 1 and sorted(back[0].node_ids) == sorted(whole.node_ids) and whole.node_ids[-1] == "r"
    by_name = dict(zip(back[0].node_ids, back[0].node_images()))
    for n, img in zip(whole.node_ids, whole.node_images()):
        assert np.array_equal(by_name[n], img), n
    parts = [ctx.xray_quadtree([a], W, PX, "colored", query_from_global=ISO, background="transparent", root_node_id=f"r{k}") for k in range(4)]
    assert sum(p.num_created for p in parts) == whole.num_created == 64
    assert_same_quadtree(ctx.xray_merge(parts, "transparent"), whole)
    # the Python helper and the example binary over the written S2 directory
    a.write(str(tmp_path / "a"))
    assert pcv.cloud_kind(tmp_path / "a") == "s2"
    xt = pcv.build_xray_quadtree(ctx, [tmp_path / "a", several["dir"]], tmp_path / "py", W, PX, "colored",
                                 intensity_interval=(0.0, 150.0), background="transparent")
    direct = ctx.xray_quadtree([a, several["b"]], W, PX, "colored", intensity_interval=(0.0, 150.0), background="transparent")
    assert xt.node_ids == direct.node_ids and np.array_equal(xt.node_images(), direct.node_images())
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "examples")])
    exe = os.path.join(ROOT, "examples", "bin", "build_xray_quadtree")
    p = subprocess.run([exe, str(tmp_path / "a"), str(several["dir"]), "--output-directory", str(tmp_path / "c"), "--resolution", str(PX),
                        "--tile-size", str(W), "--coloring-strategy", "colored", "--tile-background-color", "transparent",
                        "--filter-interval", "intensity=0,150"], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr
    names = sorted(os.listdir(tmp_path / "py"))
    assert names == sorted(os.listdir(tmp_path / "c")) and "meta.pb" in names and len(names) > 10
    for n in names:
        assert (tmp_path / "py" / n).read_bytes() == (tmp_path / "c" / n).read_bytes(), n
    # a directory of the other kind fails with the opener's own message
    rng = np.random.default_rng(5)
    tree = ctx.build(0.001, pcv.Aabb(np.zeros(3), np.ones(3)), rng.random(100), rng.random(100), rng.random(100), np.zeros((100, 3), np.uint8))
    tree.write_dir(str(tmp_path / "octree"))
    assert pcv.cloud_kind(tmp_path / "octree") == "octree"
    with pytest.raises(pcv.PcvError, match="does not describe S2"):
        pcv.build_xray_quadtree(ctx, [tmp_path / "a", tmp_path / "octree"], tmp_path / "bad", W, PX)
    with pytest.raises(pcv.PcvError, match="No octree meta"):
        pcv.build_xray_quadtree(ctx, [tmp_path / "octree", tmp_path / "a"], tmp_path / "bad", W, PX)


def test_inpaint(ctx, a20):
    cloud = a20[0]
    tile, d = 16, 2
    xt = cloud.xray_tiles(tile, 1.0, "colored", query_from_global=ISO, background="transparent")  # about half a point per pixel
    deepest = xt.deepest_level
    assert xt.num_created > 100
    leaves = {int(xt.leaf_index[int(c)]): img for c, img in zip(xt.created, xt.images())}
    images, counters, _, _ = IO.inpaint(leaves, deepest, (0, 0), tile, d, "white")
    out = xt.inpaint(d)
    assert_equals_oracle(out, images, counters, [int(xt.leaf_index[int(c)]) for c in xt.created])
    assert out.inpaint_info()["filled_pixels"].sum() > 0


# ---- 8. errors -----------------------------------------------------------------------------------------------------------
def test_errors(ctx, a20, several, tmp_path):
    a = a20[0]
    lib = ctx.lib
    p = pcv._lib.XrayParams(tile_size_px=W, pixel_size_m=PX)
    h = C.c_void_p(1)

    def refused(arr, n, params=p, col=None):
        h.value = 1
        rc = lib.pcv_xray_run_s2(ctx.handle, arr, n, C.byref(params), C.byref(col) if col is not None else None, C.byref(h))
        assert rc == pcv.PCV_E_INVALID and not h.value
        return lib.pcv_last_error(ctx.handle).decode()

    arr = (C.c_void_p * 2)(a.handle, None)
    assert "No locations specified for point cloud client." in refused(arr, 0)
    assert "S2 cloud 1 is null" in refused(arr, 2)
    many = (C.c_void_p * (pcv._lib.XRAY_MAX_TREES + 1))(*([a.handle] * (pcv._lib.XRAY_MAX_TREES + 1)))
    assert "PCV_XRAY_MAX_TREES" in refused(many, pcv._lib.XRAY_MAX_TREES + 1)
    with pytest.raises(ValueError):
        ctx.xray_tiles([], W, PX)
    # pcv_xray_check_params_ex's own refusals
    assert "only intensity" in refused(arr, 1, pcv._lib.XrayParams(tile_size_px=W, pixel_size_m=PX, interval_attribute=b"color"))
    assert "colored_with_intensity" in refused(arr, 1, pcv._lib.XrayParams(tile_size_px=W, pixel_size_m=PX, strategy=3))
    assert "unknown strategy" in refused(arr, 1, pcv._lib.XrayParams(tile_size_px=W, pixel_size_m=PX, strategy=9))
    col = pcv._lib.XrayColoring(min_intensity=0.0, max_intensity=1.0, binning_attribute=b"color", bin_size=1.0)
    assert "only intensity can be binned on" in refused(arr, 1, p, col)
    assert "tile_size_px" in refused(arr, 1, pcv._lib.XrayParams(tile_size_px=0, pixel_size_m=PX))
    # a host-only cloud, a cloud of another context
    a.write(str(tmp_path / "a"))
    host = pcv.s2_open_host(tmp_path / "a")
    assert "without a context" in refused((C.c_void_p * 2)(a.handle, host.handle), 2)
    with pytest.raises(ValueError):
        host.xray_tiles(W, PX)
    host.free()
    other = pcv.Context(0)
    try:
        foreign = other.s2_open(tmp_path / "a")
        with pytest.raises(pcv.PcvError, match="another context"):
            ctx.xray_tiles([a, foreign], W, PX)
        foreign.free()
    finally:
        other.close()
    # a cloud with a level-0 cell: the refusal of geometric locations is passed on
    x, y, z, rgb = cloud_points()
    face = ctx.s2_split(dict(x=x[:100], y=y[:100], z=z[:100], color=rgb[:100]), 0)
    with pytest.raises(pcv.PcvError, match="level 0") as e:
        ctx.xray_tiles([face], W, PX)
    assert e.value.code == pcv.PCV_E_INVALID
    face.free()
    # a tile over the workspace: out of memory, nothing left behind
    with pytest.raises(pcv.PcvError) as e:
        ctx.xray_tiles([a], W, PX, query_from_global=ISO, max_workspace_bytes=64)
    assert e.value.code == pcv.PCV_E_OOM
    xt, got = run(ctx, [a], "xray")  # the context still works
    assert xt.num_created == 64
