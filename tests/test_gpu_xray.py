"""pcv_xray_* (xray leaf tiles rasterised on the device) against xray_oracle, the numpy restatement of
xray/src/generation.rs over the CPU oracle's octree: the created set, every tile's RGBA, the drawn-point counts, and their
agreement with the batched point query. `colored` is held byte for byte to xray_truth's exact-integer oracle and
`height_stddev` to its interval truth; the arrival-order restatement stays beside them as the tie to the reference."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import point_cloud_viewer_amd as pcv
import xray_many_oracle as M
import xray_oracle as X
import xray_truth as T
from point_cloud_viewer_amd import synthetic
from test_gpu_query import ctx, scene  # noqa: F401  (module fixtures)
from test_gpu_query_batch import scene_of

pytestmark = pytest.mark.gpu
W, PX = 64, 0.25  # the 300 000-point scene of test_gpu_query: 3 levels, 64 leaf tiles of 16 m
ISO = T.ISO  # config 5 scale


def tree_points(s):
    tree, idx = s["tree"], s.get("index_of") or {n: i for i, n in enumerate(s["names"])}

    def cube(name):
        nd = tree.node(idx[name])
        return nd.cube_min, nd.cube_edge
    return X.TreePoints(s["oracle"].nodes, cube, s["bmin"], s["bmax"])


@pytest.fixture(scope="module")
def tp(scene):  # noqa: F811
    return tree_points(scene)


def run(tree, strategy="xray", **kw):
    xt = tree.xray_tiles(W if "tile_size_px" not in kw else kw.pop("tile_size_px"), kw.pop("pixel_size_m", PX), strategy, **kw)
    imgs = xt.images() if xt.num_created else np.zeros((0, W, W, 4), np.uint8)
    return xt, {n: (imgs[i], int(xt.drawn[i])) for i, n in enumerate(xt.created_ids)}


def check_exact(got, want):
    assert list(got) == list(want) or set(got) == set(want), (set(got) ^ set(want))
    for name, (img, drawn) in want.items():
        assert got[name][1] == drawn, name
        assert np.array_equal(got[name][0], img), (name, int((got[name][0] != img).any(-1).sum()))


@pytest.mark.parametrize("background", ["white", "transparent"])
def test_xray_matches_oracle(scene, tp, background):  # noqa: F811
    xt, got = run(scene["tree"], "xray", background=background)
    want, g = X.xray_tiles(tp, W, PX, "xray", background=background)
    assert xt.deepest_level == g["deepest_level"] == 3 and xt.leaf_ids == g["leaf_ids"]
    assert tuple(xt.bounding_rect) == g["rect"]
    assert xt.created_ids == [n for n in g["leaf_ids"] if n in want]  # leaf order
    assert 8 < len(want) < 64
    check_exact(got, want)


def check_close(got, want, exact_share):
    """against the arrival-order oracle (one order the reference may take): within 1, and `exact_share` of the pixels equal.
    Every caller also holds the same run to xray_truth, which leaves no such slack."""
    assert set(got) == set(want)
    exact = total = 0
    for name, (img, drawn) in want.items():
        g = got[name][0]
        assert got[name][1] == drawn, name
        assert np.array_equal(g[..., 3], img[..., 3]), name  # coverage and alpha
        d = np.abs(g.astype(int) - img.astype(int))
        assert d.max() <= 1, name
        drawn_px = img[..., 3] == 255
        exact += int((d[drawn_px] == 0).all(-1).sum())
        total += int(drawn_px.sum())
    assert total > 0 and exact >= exact_share * total, (exact, total)


def check_colored_exact(got, g, pts, tile_px=W, background="white"):
    """every byte of every created tile against the exact-integer oracle"""
    want = T.colored_tiles(g, pts, tile_px, background)
    check_exact(got, want)
    px = sum(int((img[..., 3] == 255).sum()) for img, _ in want.values()) if background == "transparent" else len(want) * tile_px ** 2
    print(f"colored: {len(want)} tiles, {px} pixels compared, all equal")


@pytest.fixture(scope="module")
def pts(tp):
    return M.tile_points([tp], W, PX)


def test_colored_matches_oracle(scene, tp, pts):  # noqa: F811
    _, got = run(scene["tree"], "colored")
    check_colored_exact(got, *pts)
    _, got_t = run(scene["tree"], "colored", background="transparent")
    check_colored_exact(got_t, *pts, background="transparent")
    want, _ = X.xray_tiles(tp, W, PX, "colored")
    check_close(got, want, 0.99)


@pytest.mark.parametrize("cmap", ["jet", "purplish"])
def test_height_stddev_matches_oracle(scene, tp, pts, cmap):  # noqa: F811
    strat = ("height_stddev", 1.5, cmap)
    _, got = run(scene["tree"], strat, background="transparent")
    T.stddev_check(got, *pts, W, 1.5, cmap, "transparent")
    want, _ = X.xray_tiles(tp, W, PX, strat, background="transparent")
    check_close(got, want, 0.0)


def test_query_from_global_and_interval(scene, tp):  # noqa: F811
    _, got = run(scene["tree"], "xray", query_from_global=ISO)
    want, g = X.xray_tiles(tp, W, PX, "xray", iso=ISO)
    assert len(want) > 8
    check_exact(got, want)
    _, got = run(scene["tree"], "xray", query_from_global=ISO, intensity_interval=(10.0, 120.5))
    want, _ = X.xray_tiles(tp, W, PX, "xray", iso=ISO, interval=(10.0, 120.5))
    check_exact(got, want)
    xt, got = run(scene["tree"], "colored", intensity_interval=(5.0, 4.0))  # lo > hi: nothing passes, no tile is created
    assert xt.num_created == 0 and got == {} and len(xt.leaf_ids) == 64


def test_invalid_parameters(ctx, scene):  # noqa: F811
    tree = scene["tree"]
    for kw in (dict(strategy="binned"), dict(strategy=("height_stddev", 0.0, "jet")), dict(strategy=("height_stddev", -1.0, "jet"))):
        with pytest.raises((ValueError, pcv.PcvError)):
            tree.xray_tiles(W, PX, **kw)
    p = pcv._lib.XrayParams(tile_size_px=W, pixel_size_m=PX, strategy=7)
    h = C.c_void_p()
    assert ctx.lib.pcv_xray_run(ctx.handle, tree.handle, C.byref(p), C.byref(h)) == pcv.PCV_E_INVALID
    p = pcv._lib.XrayParams(tile_size_px=W, pixel_size_m=PX, interval_attribute=b"color")
    assert ctx.lib.pcv_xray_run(ctx.handle, tree.handle, C.byref(p), C.byref(h)) == pcv.PCV_E_INVALID
    assert "only intensity" in ctx.lib.pcv_last_error(ctx.handle).decode()
    p = pcv._lib.XrayParams(tile_size_px=1, pixel_size_m=0.001)  # 100 m / 1 mm pixels: far more than 2^24 leaves
    assert ctx.lib.pcv_xray_run(ctx.handle, tree.handle, C.byref(p), C.byref(h)) == pcv.PCV_E_INVALID
    assert "root_node_id" in ctx.lib.pcv_last_error(ctx.handle).decode()


def test_workspace_groups_and_determinism(scene):  # noqa: F811
    tree = scene["tree"]
    for strat in ("xray", "colored"):
        xt1, a = run(tree, strat)
        xt2, b = run(tree, strat, max_workspace_bytes=1_000_000)  # a few tiles per group
        _, c = run(tree, strat)
        assert list(a) == list(b) == list(c)
        for n in a:
            assert np.array_equal(a[n][0], b[n][0]) and np.array_equal(a[n][0], c[n][0]), (strat, n)
    with pytest.raises(pcv.PcvError, match="max_workspace_bytes"):
        run(tree, "xray", max_workspace_bytes=4096)


def test_batch_agreement(ctx, scene, tp):  # noqa: F811
    """kept == the tile's points in query_batch, drawn == kept minus the points outside the image (the oracle's count)."""
    tree = scene["tree"]
    xt, got = run(tree, "xray")
    geo = pcv.xray_leaf_tiles(W, PX, scene["bmin"], scene["bmax"])
    shapes = ctx.shapes([("aabb", b[:3], b[3:]) for b in geo["tile_bbox"]])
    batch = tree.query_batch(shapes)
    first, _, off = batch.segments()
    per_shape = off[first[1:]] - off[first[:-1]]
    assert [geo["leaf_ids"][int(s)] for s in np.flatnonzero(per_shape)] == xt.created_ids
    assert np.array_equal(per_shape[per_shape > 0], xt.kept)
    want, _ = X.xray_tiles(tp, W, PX, "xray")
    for i, n in enumerate(xt.created_ids):
        pts = batch.shape_points(geo["leaf_ids"].index(n))
        mn, mx = geo["tile_bbox"][geo["leaf_ids"].index(n)][:3], geo["tile_bbox"][geo["leaf_ids"].index(n)][3:]
        px, py, _ = X.discretise(pts["x"], pts["y"], pts["z"], mn, mx, W)
        assert xt.drawn[i] == int(((px < W) & (py < W)).sum()) == want[n][1], n


def test_edge_cloud(ctx):  # noqa: F811
    """Points on tile faces and on the min.y face (y == H: never drawn), a pixel with all 1 024 z buckets of a half-open
    box, 10^6 points in one pixel, pixels of one point and pixels whose points share one z (deviation 0), and a sorted copy
    of the same cloud (same bytes). colored byte for byte against the exact-integer oracle, height_stddev against the
    interval truth."""
    p, rgb, bmin, bmax, orders = T.edge_cloud()
    results = []
    for order in orders:
        x, y, z = (np.ascontiguousarray(p[order, a]) for a in range(3))
        s = scene_of(ctx, x, y, z, np.ascontiguousarray(rgb[order]), None, bmin, bmax, 20_000)
        tpp = tree_points(s)
        xt, got = run(s["tree"], "xray")
        want, geo = X.xray_tiles(tpp, W, PX, "xray")
        assert geo["deepest_level"] == 1
        check_exact(got, want)
        # +x, min y: only points on its min.y face, which is the root cube's min face (Cube::bounding, aabb.rs:149-157),
        # so they decode onto it exactly: kept (the box is closed at min), all at y == H, never drawn
        r2 = xt.created_ids.index("r2")
        assert xt.kept[r2] == 300 and xt.drawn[r2] == 0 and np.all(got["r2"][0] == 255)
        col = got["r0"][0]
        assert tuple(col[W - 1 - int(5.1 / PX), int(3.1 / PX)]) == (0, 0, 0, 255)  # n = 1 024: ln(n) / ln(1024) = 1
        _, cgot = run(s["tree"], "colored")
        tile_pts = M.tile_points([tpp], W, PX)
        check_colored_exact(cgot, *tile_pts)
        for cmap in ("jet", "purplish"):
            _, sgot = run(s["tree"], ("height_stddev", 1.5, cmap))
            T.stddev_check(sgot, *tile_pts, W, 1.5, cmap)
        # equal z, n = 2 and 3: deviation 0 (an interval from 0 up, where only the colour of 0 passes), purplish(0) = (204, 204, 255)
        for i in range(2):
            assert tuple(sgot["r0"][0][W - 1 - int(9.1 / PX), int((7.1 + 0.5 * i) / PX)]) == (204, 204, 255, 255), i
        results.append((got, cgot))
        s["tree"].free()
    (a, ca), (b, cb) = results
    for n in a:
        assert np.array_equal(a[n][0], b[n][0]) and np.array_equal(ca[n][0], cb[n][0]), n


@pytest.fixture(scope="module")
def ecef(ctx):  # noqa: F811
    x, y, z, rgb, inten, bmin, bmax, cap = T.ecef_cloud()
    s = scene_of(ctx, x, y, z, rgb, inten, bmin, bmax, cap)
    s.update(x=x, y=y, z=z, rgb=rgb, inten=inten, tp=tree_points(s))
    yield s
    s["tree"].free()


def test_four_encodings_and_opened_directory(ctx, ecef, tmp_path):  # noqa: F811
    s, tree, tpp = ecef, ecef["tree"], ecef["tp"]
    x, y, z, rgb, inten, bmin, bmax = (s[k] for k in ("x", "y", "z", "rgb", "inten", "bmin", "bmax"))
    assert {tree.node(i).encoding for i in range(tree.num_nodes) if tree.node(i).num_points > 0} == {1, 2, 3, 4}
    _, got = run(tree, "xray", tile_size_px=128, pixel_size_m=32.0)
    want, _ = X.xray_tiles(tpp, 128, 32.0, "xray")
    check_exact(got, want)
    O.build_literal_dir(tmp_path / "oracle", 0.001, bmin, bmax, x, y, z, rgb, inten, threads=4)
    opened = ctx.open_dir(tmp_path / "oracle")
    _, got2 = run(opened, "xray", tile_size_px=128, pixel_size_m=32.0)
    assert list(got2) == list(got)
    for n in got:
        assert np.array_equal(got2[n][0], got[n][0]), n
    _, got3 = run(opened, "xray", tile_size_px=128, pixel_size_m=32.0, root_node_id="r1")
    assert got3 and all(n.startswith("r1") for n in got3)
    for n in got3:
        assert np.array_equal(got3[n][0], got[n][0]), n
    xt = opened.xray_tiles(128, 32.0, "xray")
    dev = xt.images(0, 2, device=True)
    assert np.array_equal(dev.cpu().numpy(), xt.images(0, 2))
    opened.free()


@pytest.mark.parametrize("iso", [None, ISO], ids=["plain", "query_from_global"])
def test_colored_and_height_stddev_at_ecef_scale(ecef, iso):
    """The four-encodings cloud, z of order 10^6 in both frames: colored byte for byte, height_stddev (two passes; one
    pass would lose the deviation here) against the interval truth."""
    kw = dict(tile_size_px=T.ECEF_W, pixel_size_m=T.ECEF_PX, **({} if iso is None else dict(query_from_global=iso)))
    tile_pts = M.tile_points([ecef["tp"]], T.ECEF_W, T.ECEF_PX, iso)
    _, got = run(ecef["tree"], "colored", **kw)
    check_colored_exact(got, *tile_pts, tile_px=T.ECEF_W)
    intervals = T.stddev_intervals(*tile_pts, T.ECEF_W)
    for cmap in ("jet", "purplish"):
        _, got = run(ecef["tree"], ("height_stddev", T.ECEF_MAX_STDDEV, cmap), background="transparent", **kw)
        T.stddev_check(got, *tile_pts, T.ECEF_W, T.ECEF_MAX_STDDEV, cmap, "transparent", intervals)


def test_closed_query_faces_with_identity_transform(ctx):  # noqa: F811
    """With query_from_global the tile's query is a closed Obb (obb.rs:83-90): points on the box's max faces are kept.
    On the max z face they land in z bucket 1 024, so a pixel holds 1 025 distinct buckets; on the max x face they land at
    x == W and are never drawn. Float64 nodes under a root cube of edge 64 decode these binary coordinates exactly."""
    iso = [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0]
    pts = [np.stack([np.full(1025, 3.1), np.full(1025, 5.1), np.arange(1025) / 16.0], 1),  # z = 0 .. 64: buckets 0 ..= 1024
           [[9.1, 5.1, 0.0], [9.1, 5.1, 64.0]],                                          # buckets 0 and 1 024: n = 2
           np.stack([np.full(200, 32.0), np.linspace(1.0, 15.0, 200), np.full(200, 30.0)], 1),  # x == max x, tile r2 only
           [[0.0, 0.0, 0.0]]]
    p = np.concatenate([np.asarray(a, dtype=np.float64) for a in pts])
    rgb = np.full((p.shape[0], 3), 7, dtype=np.uint8)
    bmin, bmax = p.min(0), p.max(0)
    assert tuple(bmin) == (0.0, 0.0, 0.0) and tuple(bmax) == (32.0, 15.0, 64.0)
    x, y, z = (np.ascontiguousarray(p[:, a]) for a in range(3))
    tree = ctx.build(1e-9, pcv.Aabb(bmin, bmax), x, y, z, rgb, max_points_per_node=100_000)
    with O.max_points_per_node(100_000):
        want_tree = O.build_closed(1e-9, bmin, bmax, x, y, z, rgb, threads=4)
    names = tree.node_names()
    assert {tree.node(i).encoding for i in range(tree.num_nodes) if tree.node(i).num_points} == {4}
    tpp = tree_points(dict(tree=tree, oracle=want_tree, names=names, bmin=bmin, bmax=bmax))
    xt, got = run(tree, "xray", query_from_global=iso)
    want, geo = X.xray_tiles(tpp, W, PX, "xray", iso=iso)
    assert geo["deepest_level"] == 1
    check_exact(got, want)
    # the column's pixel: 1 025 distinct buckets (value 0); the two-point pixel: buckets 0 and 1 024 (n = 2, not 1)
    mn, mx = geo["tile_bbox"][geo["leaf_ids"].index("r0")]
    qx, qy, qz, _ = tpp.query(O.SHAPE_OBB, X.tile_obb(iso, mn, mx))
    px, py, pz = X.discretise(qx, qy, qz, mn, mx, W)
    col = (px == int(3.1 / PX)) & (py == W - 1 - int(5.1 / PX))
    assert np.unique(pz[col]).size == 1025 and pz.max() == 1024
    img = got["r0"][0]
    assert tuple(img[W - 1 - int(5.1 / PX), int(3.1 / PX)]) == (0, 0, 0, 255)
    assert tuple(img[W - 1 - int(5.1 / PX), int(9.1 / PX)]) == (X.xray_value(2),) * 3 + (255,)
    # +x tile: only points on its max x face: created, nothing drawn, all background
    r2 = xt.created_ids.index("r2")
    assert xt.kept[r2] == 200 and xt.drawn[r2] == 0 and np.all(got["r2"][0] == 255)
    tree.free()


def test_accumulation_strides_over_buckets(scene, tp):  # noqa: F811
    """256 px tiles: 64 blocks per tile, thousands of buckets against the few hundred accumulation workgroups that are
    resident at once, so every workgroup strides over many buckets; equal to the oracle byte for byte."""
    _, got = run(scene["tree"], "xray", tile_size_px=256, pixel_size_m=PX / 4)
    want, _ = X.xray_tiles(tp, 256, PX / 4, "xray")
    assert len(want) * 64 > 4 * 256
    check_exact(got, want)


def test_group_and_grid_caps_in_the_experiment_build(scene):  # noqa: F811
    """The experiment build lowers the bucket cap of a tile group (here 2 tiles of 4 blocks) and the accumulation grid
    (3 workgroups): the same bytes as the shipped library's one group."""
    import hashlib
    import os
    import subprocess
    import sys
    _, got = run(scene["tree"], "colored")
    digest = hashlib.sha256(b"".join(n.encode() + got[n][0].tobytes() for n in got)).hexdigest()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys, hashlib; sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + '/tests')\n"
            "import numpy as np, point_cloud_viewer_amd as pcv\nfrom point_cloud_viewer_amd import synthetic\n"
            "x, y, z, rgb, bmin, bmax = synthetic.gaussian_clusters(300_000, seed=2, num_clusters=6, extent=100.0, sigma_range=(0.5, 6.0))\n"
            "inten = (np.arange(x.size) % 251).astype(np.float32)\n"
            "t = pcv.Context(0).build(0.001, pcv.Aabb(bmin, bmax), x, y, z, rgb, inten, max_points_per_node=2000)\n"
            f"xt = t.xray_tiles({W}, {PX}, 'colored')\nim = xt.images()\n"
            "print('DIGEST', hashlib.sha256(b''.join(n.encode() + im[i].tobytes() for i, n in enumerate(xt.created_ids))).hexdigest())\n")
    env = dict(os.environ, PCV_HIP_LIBRARY="exp", PCV_XRAY_MAX_GROUP_BUCKETS="8", PCV_XRAY_ACCUM_GRID="3")
    out = subprocess.run([sys.executable, "-c", code, root], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and f"DIGEST {digest}" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]
