"""Terrain layers in the headless frame (pcv_render_views_terrain) against the numpy oracle of
tests/render_terrain_oracle.py over the CPU oracle's node bytes and visible lists: images, depth planes, every pcv_render_info
field and the per-layer terrain info, byte for byte; no tolerance anywhere. An octree of 3 000 points, images of 64 x 48 and
161 x 97, terrains of 8 x 8 tiles (4 and 5 of them), windows of 16, 64 and once 1024 vertices."""
import ctypes as C
import filecmp
import os

import numpy as np
import pytest

import oracle_lib as O
import point_cloud_viewer_amd as pcv
import render_oracle as R
import render_terrain_oracle as RT
from point_cloud_viewer_amd import _lib as L
from test_gpu_query import ctx  # noqa: F401  (module fixture)
from test_gpu_render_outline import build_scene, cloud, frusta

pytestmark = pytest.mark.gpu
W, H = 64, 48
BMIN, BMAX = np.zeros(3), np.full(3, 64.0)
IDENTITY = [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0]
GROUND = dict(tile_size=8, resolution_m=4.0, origin=(40.0, 24.0, 0.0), world_from_terrain=IDENTITY, min_points=2)
TILTED = dict(tile_size=8, resolution_m=3.0, origin=(-20.0, -14.0, 0.0), min_points=1,
              world_from_terrain=[30.0, 34.0, 40.0] + O.quat_from_axis_angle([0.2 / np.sqrt(1.05), 0.1 / np.sqrt(1.05), 1.0 / np.sqrt(1.05)], 0.4))


def rotation(q):
    i, j, k, w = q
    return np.array([[1 - 2 * (j * j + k * k), 2 * (i * j - k * w), 2 * (i * k + j * w)],
                     [2 * (i * j + k * w), 1 - 2 * (i * i + k * k), 2 * (j * k - i * w)],
                     [2 * (i * k - j * w), 2 * (j * k + i * w), 1 - 2 * (i * i + j * j)]])


def build_layer(ctx, params, i_range, j_range, height, skip=lambda i, j: False, single=lambda i, j: False, seed=3):  # noqa: F811
    """A finished Terrain with `min_points` points on every vertex of the ranges (one only where `single` says: such a vertex
    stays unset at min_points 2; none where `skip` says), and the dict the oracle reads."""
    rng = np.random.default_rng(seed)
    o, res = np.asarray(params["origin"]), params["resolution_m"]
    iso = np.asarray(params["world_from_terrain"])
    pts = []
    for j in range(*j_range):
        for i in range(*i_range):
            if skip(i, j):
                continue
            for n in range(1 if single(i, j) else params["min_points"]):
                pts.append([o[0] + res * i, o[1] + res * j, o[2] + height(i, j) - 0.25 * n])
    world = np.asarray(pts) @ rotation(iso[3:]).T + iso[:3]
    rgb = rng.integers(0, 256, (world.shape[0], 3), dtype=np.uint8)
    t = ctx.terrain_begin(world.min(axis=0) - 1.0, world.max(axis=0) + 1.0, **params)
    t.add_points(world[:, 0].copy(), world[:, 1].copy(), world[:, 2].copy(), rgb).finish()
    return t, layer_dict(t, params)


def layer_dict(t, params):
    return dict(tile_size=params["tile_size"], resolution_m=params["resolution_m"], origin=np.asarray(params["origin"], np.float64),
                world_from_terrain=np.asarray(params["world_from_terrain"], np.float64), tiles=t.tiles(), heights=t.heights(), colors=t.colors())


@pytest.fixture(scope="module")
def scene(ctx):  # noqa: F811
    s = build_scene(ctx, *cloud())
    # the ground cuts through the cloud (heights 22 .. 34): vertices i -8 .. 5, j -5 .. 9 around the origin at (40, 24), the
    # tile (0, 0) left out whole, a few vertices unset at min_points 2
    ground, gd = build_layer(ctx, GROUND, (-8, 6), (-5, 10), lambda i, j: 28.0 + 6.0 * np.sin(0.7 * i) * np.cos(0.5 * j),
                             skip=lambda i, j: 0 <= i < 8 and 0 <= j < 8, single=lambda i, j: (i * 5 + j * 3) % 11 == 0)
    assert sorted(map(tuple, gd["tiles"].tolist())) == [(-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1)]
    info = ground.info()
    assert 0 < info["set_vertices"] < 14 * 15 - 36 and info["rendered_quads"] > 20
    tilted, td = build_layer(ctx, TILTED, (0, 13), (0, 10), lambda i, j: 3.0 * np.sin(0.9 * i + 0.4 * j), seed=4)
    assert len(td["tiles"]) == 4
    s.update(ground=ground, ground_dict=gd, tilted=tilted, tilted_dict=td)
    yield s
    for k in ("tree", "ground", "tilted"):
        s[k].free()


PERSPECTIVE = dict(aspect=4.0 / 3.0, fovy=1.2, near=0.1, far=200.0)


def camera(eye, axis=(1.0, 0.0, 0.0), angle=0.0, **kw):
    p = dict(PERSPECTIVE, **kw)
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    m, _ = O.frustum_new(list(eye), O.quat_from_axis_angle(list(axis), angle), O.perspective3_new(p["aspect"], p["fovy"], p["near"], p["far"]))
    return m, list(eye)


def views():
    """Looking down on the ground from inside the cube; just above the ground and nearly level, so that edges pass under and
    behind the eye (w = 0); oblique from a corner; from below the ground's height looking along -x."""
    cams = [camera((31.3, 33.7, 50.1)), camera((33.1, 29.7, 36.3), angle=1.3), camera((9.7, 10.9, 45.3), axis=(1.0, -1.0, 0.0), angle=0.9),
            camera((70.3, 31.9, 20.7), axis=(0.0, 1.0, 0.0), angle=np.pi / 2)]
    return [m for m, _ in cams], np.array([e for _, e in cams])


_oracle_cache = {}


def oracle_view(tn, m, cam, w, h, layers, window, point_size, gamma, max_nodes, outlines):
    """One oracle frame, computed once per (tree, layers, arguments) and never changed afterwards."""
    key = (id(tn), tuple(id(l) for l in layers), np.asarray(m, np.float64).tobytes(), tuple(cam), w, h, window, point_size, gamma, max_nodes, outlines)
    if key not in _oracle_cache:
        _oracle_cache[key] = RT.render_view(tn, m, w, h, layers, cam, window, point_size, gamma, max_nodes, outlines)
    return _oracle_cache[key]


def check_views(rv, tn, mats, cams, w, h, layers, window, point_size=1.0, gamma=1.0, max_nodes=0, outlines=False):
    imgs, dep = rv.images().cpu().numpy(), rv.depth().cpu().numpy()
    assert imgs.shape == (len(mats), h, w, 4) and dep.shape == (len(mats), h, w) and dep.dtype == np.float32
    wants = []
    for v, m in enumerate(mats):
        want = oracle_view(tn, m, cams[v], w, h, layers, window, point_size, gamma, max_nodes, outlines)
        info = rv.info(v)
        if want["status"] is None:  # the reference panics: a cleared image, no terrain
            assert info["status"] in (1, 2) and info["nodes_drawn"] == 0 and info["points_submitted"] == 0, (v, info)
        else:
            assert info["status"] == 0 and info["nodes_visible"] == want["nodes_visible"] and info["nodes_drawn"] == len(want["drawn"]), (v, info)
        for k in ("points_submitted", "points_drawn", "pixels_covered"):
            assert info[k] == want[k], (v, k, info[k], want[k])
        if outlines:
            oinfo = rv.outline_info(v)
            for k in ("segments_submitted", "segments_drawn", "outline_pixels"):
                assert oinfo[k] == want[k], (v, k, oinfo[k], want[k])
        for k in range(len(layers)):
            assert rv.terrain_info(v, k) == want["terrain"][k], (v, k, rv.terrain_info(v, k), want["terrain"][k])
        assert np.array_equal(imgs[v], want["image"]), (v, int((imgs[v] != want["image"]).any(axis=-1).sum()))
        assert np.array_equal(dep[v].view(np.uint32), want["depth"].view(np.uint32)), v
        wants.append(want)
    return wants


def both_ways(tn, mats, wants, w, h, point_size, gamma):
    """(pixels a point held that terrain took, pixels with a terrain fragment that a point kept) over the views."""
    took = kept = 0
    for m, want in zip(mats, wants):
        if want["status"] is None:
            continue
        points = R.render_view(tn, m, w, h, point_size, gamma)
        ground = want["winner"].reshape(-1) >= want["terrain_rank0"]
        took += int((ground & (points["winner"].reshape(-1) >= 0)).sum())
        frag = np.zeros(w * h, bool)
        for f in want["terrain_fragments"]:
            frag[f["pix"]] = True
        kept += int((frag & ~ground).sum())
    return took, kept


@pytest.mark.parametrize("size,window", [((W, H), 16), ((161, 97), 64)])
def test_views_equal_the_oracle(ctx, scene, size, window):  # noqa: F811
    mats, cams = views()
    w, h = size
    rv = scene["tree"].render(frusta(ctx, mats), w, h, point_size=2.0, gamma=2.2, depth=True, terrain=[scene["ground"]], camera_positions=cams,
                              terrain_window=window)
    assert rv.num_terrain_layers == 1
    wants = check_views(rv, scene["tn"], mats, cams, w, h, [scene["ground_dict"]], window, 2.0, 2.2)
    infos = [wt["terrain"][0] for wt in wants]
    assert sum(t["pixels_won"] for t in infos) > 200 and sum(t["pixels_won"] > 0 for t in infos) >= 3
    assert sum(t["edges_drawn"] for t in infos) < sum(t["edges_submitted"] for t in infos)  # some edges are clipped away whole
    assert all(0 < t["edges_submitted"] < 3 * window * window for t in infos)  # holes, the missing tile, the window's rim
    took, kept = both_ways(scene["tn"], mats, wants, w, h, 2.0, 2.2)
    assert took > 0 and kept > 0, (took, kept)  # the depth test decides both ways
    # the second camera sits inside the ground's extent: some of its edges cross w = 0
    f = wants[1]["terrain_fragments"][0]
    clip = RT.clip_points(scene["ground_dict"], f["pos"], window, RT.load_window(scene["ground_dict"], f["pos"], window)[0], mats[1])
    crossing = sum((clip[a[1], a[0], 3] > 0) != (clip[b[1], b[0], 3] > 0) for a, b in map(RT.edge_ends, f["edges"]))
    assert crossing > 0
    with pytest.raises(pcv.PcvError):
        rv.terrain_info(0, 1)
    with pytest.raises(pcv.PcvError):
        rv.terrain_info(len(mats), 0)
    rv.close()


def test_window_over_seams_a_missing_tile_and_negative_tiles(ctx, scene):  # noqa: F811
    """Cameras whose windows of 16 hang over the tile seams at i = 0 and j = 0, 8, over the tile that is missing, and half off
    the terrain: the frustum stays put, only the window moves."""
    m, _ = camera((31.3, 33.7, 50.1))
    cams = np.array([[40.0, 24.0, 0.0], [39.9, 56.1, 5.0], [71.9, 40.0, -3.0], [8.1, 4.3, 90.0], [500.0, 500.0, 0.0]])
    mats = [m] * len(cams)
    rv = scene["tree"].render(frusta(ctx, mats), W, H, terrain=[scene["ground"]], camera_positions=cams, terrain_window=16)
    wants = check_views(rv, scene["tn"], mats, cams, W, H, [scene["ground_dict"]], 16)
    assert [wt["terrain"][0]["pos"] for wt in wants[:2]] == [(-8, -8), (-9, 0)]
    submitted = [wt["terrain"][0]["edges_submitted"] for wt in wants]
    assert submitted[-1] == 0 and min(submitted[:-1]) > 0 and len(set(submitted)) > 2
    assert np.array_equal(rv.images(4, 1).cpu().numpy()[0], R.render_view(scene["tn"], m, W, H)["image"])  # a window off the terrain
    rv.close()


def test_rotated_frame_and_two_layers(ctx, scene):  # noqa: F811
    mats, cams = views()
    shapes = frusta(ctx, mats)
    images = {}
    for name in ("tilted", "ground+tilted", "tilted+ground", "ground+ground", "ground"):
        names = name.split("+")
        rv = scene["tree"].render(shapes, W, H, point_size=1.0, terrain=[scene[n] for n in names], camera_positions=cams, terrain_window=16)
        wants = check_views(rv, scene["tn"], mats, cams, W, H, [scene[n + "_dict"] for n in names], 16)
        assert sum(wt["terrain"][0]["pixels_won"] for wt in wants) > 100
        images[name] = rv.images().cpu().numpy(), rv.depth().cpu().numpy()
        if name == "ground+ground":  # the second copy ties with the first everywhere and loses on the rank
            assert all(rv.terrain_info(v, 1)["pixels_won"] == 0 for v in range(len(mats)))
            assert all(rv.terrain_info(v, 1)["edges_drawn"] == rv.terrain_info(v, 0)["edges_drawn"] > 0 for v in range(len(mats)))
        if name == "ground+tilted":
            assert all(sum(wt["terrain"][k]["pixels_won"] for wt in wants) > 0 for k in (0, 1))
        rv.close()
    assert np.array_equal(images["ground+ground"][0], images["ground"][0]) and np.array_equal(images["ground+ground"][1], images["ground"][1])
    assert not np.array_equal(images["tilted"][0], images["ground"][0])
    assert np.array_equal(images["ground+tilted"][1], images["tilted+ground"][1])  # the depth plane does not depend on the order


def test_outlines_max_nodes_and_a_cleared_view(ctx, scene):  # noqa: F811
    mats, cams = views()
    mats, cams = [mats[0], np.zeros(16), mats[2]], cams[[0, 1, 2]]
    shapes = frusta(ctx, mats)
    for max_nodes in (3, 0):
        rv = scene["tree"].render(shapes, W, H, point_size=2.0, max_nodes=max_nodes, show_octree_nodes=True, terrain=[scene["ground"], scene["tilted"]],
                                  camera_positions=cams, terrain_window=16)
        wants = check_views(rv, scene["tn"], mats, cams, W, H, [scene["ground_dict"], scene["tilted_dict"]], 16, 2.0, max_nodes=max_nodes, outlines=True)
        assert wants[0]["outline_pixels"] > 0 and wants[0]["terrain"][0]["pixels_won"] > 0 and wants[0]["nodes_visible"] > 3
        assert rv.info(1)["status"] == 1 and wants[1]["status"] is None
        assert rv.terrain_info(1, 0) == dict(pos=RT.window_pos(scene["ground_dict"], cams[1], 16), edges_submitted=0, edges_drawn=0, pixels_won=0)
        assert (rv.images(1, 1).cpu().numpy()[0] == [0, 0, 0, 255]).all() and (rv.depth(1, 1).cpu().numpy() == 1.0).all()
        rv.close()


def test_groups_and_repeated_runs(ctx, scene):  # noqa: F811
    mats, cams = views()
    shapes, layers = frusta(ctx, mats), [scene["ground"], scene["tilted"]]
    kw = dict(point_size=2.0, show_octree_nodes=True, terrain=layers, camera_positions=cams, terrain_window=16)
    first = scene["tree"].render(shapes, W, H, **kw)
    check_views(first, scene["tn"], mats, cams, W, H, [scene["ground_dict"], scene["tilted_dict"]], 16, 2.0, outlines=True)
    ref = first.images().cpu().numpy(), first.depth().cpu().numpy(), [(first.info(v), first.terrain_info(v, 0), first.terrain_info(v, 1)) for v in range(4)]
    first.close()
    per_view = 8 * W * H + 2 * 16 * 16 * 24  # the key plane and two windows of 24-byte vertices
    for ws in (None, per_view, 3 * per_view + 5):  # the same again; one view per group; groups of three and one
        rv = scene["tree"].render(shapes, W, H, max_workspace_bytes=ws, **kw)
        assert np.array_equal(rv.images().cpu().numpy(), ref[0]) and np.array_equal(rv.depth().cpu().numpy(), ref[1]), ws
        assert [(rv.info(v), rv.terrain_info(v, 0), rv.terrain_info(v, 1)) for v in range(4)] == ref[2], ws
        rv.close()
    live = ctx.pool_stats()[0]
    with pytest.raises(pcv.PcvError) as e:  # one view's windows no longer fit: refused before anything is allocated
        scene["tree"].render(shapes, W, H, max_workspace_bytes=per_view - 1, **kw)
    assert e.value.code == pcv.PCV_E_OOM and "terrain windows" in str(e.value) and ctx.pool_stats()[0] == live
    with pytest.raises(pcv.PcvError) as e:  # 1 400 layers of 3 * 2^20 ranks
        scene["tree"].render(shapes, W, H, terrain=[scene["ground"]] * 1400, camera_positions=cams, max_workspace_bytes=1 << 50)
    assert e.value.code == pcv.PCV_E_INVALID and "draw ranks" in str(e.value) and ctx.pool_stats()[0] == live
    with pytest.raises(pcv.PcvError) as e:
        scene["tree"].render(shapes, W, H, terrain=[scene["ground"]], camera_positions=cams + [[1e300, 0.0, 0.0]], terrain_window=16)
    assert e.value.code == pcv.PCV_E_INVALID and "Terrain location not representable." in str(e.value) and ctx.pool_stats()[0] == live
    with pytest.raises(pcv.PcvError) as e:
        scene["tree"].render(shapes, W, H, terrain=[scene["ground"]], camera_positions=cams, terrain_window=15)
    assert e.value.code == pcv.PCV_E_INVALID and "window" in str(e.value)
    unfinished = ctx.terrain_begin(BMIN, BMAX, **GROUND)
    with pytest.raises(pcv.PcvError) as e:
        scene["tree"].render(shapes, W, H, terrain=[unfinished], camera_positions=cams, terrain_window=16)
    assert e.value.code == pcv.PCV_E_INVALID and "not finished" in str(e.value)
    unfinished.free()


def raw_terrain(ctx, tree, shapes, overlay, terrain, **kw):  # noqa: F811
    """pcv_render_views_terrain called as C would, with `terrain` a RenderTerrainLayers or None."""
    p, h = pcv.render_params(**kw), C.c_void_p()
    ctx._check(ctx.lib.pcv_render_views_terrain(ctx.handle, shapes.handle, tree.handle, C.byref(p), C.byref(overlay) if overlay is not None else None,
                                                C.byref(terrain) if terrain is not None else None, C.byref(h)))
    return pcv.RenderedViews(ctx, h, shapes.count, kw["width"], kw["height"], False)


def test_no_layers_is_render_views_ex(ctx, scene):  # noqa: F811
    mats, cams = views()
    tree, shapes = scene["tree"], frusta(ctx, mats)
    kw = dict(width=W, height=H, point_size=2.0, gamma=2.2, max_nodes=5)
    ctx.set_profiling(True)
    try:
        for outlines in (False, True):
            ctx.reset_kernel_stats()
            base = tree.render(shapes, W, H, point_size=2.0, gamma=2.2, max_nodes=5, show_octree_nodes=outlines)
            plain = {k: v[0] for k, v in ctx.kernel_stats().items() if v[0]}
            ref = base.images().cpu().numpy(), base.depth().cpu().numpy(), [base.info(v) for v in range(len(mats))]
            assert not any("terrain" in k for k in plain)
            overlay = pcv.render_overlay(outlines)
            for terrain in (None, L.RenderTerrainLayers(0, 0, None, None), L.RenderTerrainLayers(0, 15, None, cams.ctypes.data)):
                ctx.reset_kernel_stats()
                rv = raw_terrain(ctx, tree, shapes, overlay, terrain, **kw)
                assert {k: v[0] for k, v in ctx.kernel_stats().items() if v[0]} == plain
                assert np.array_equal(rv.images().cpu().numpy(), ref[0]) and np.array_equal(rv.depth().cpu().numpy(), ref[1])
                assert [rv.info(v) for v in range(len(mats))] == ref[2]
                with pytest.raises(pcv.PcvError):
                    rv.terrain_info(0, 0)  # no layers
                rv.close()
            ctx.reset_kernel_stats()
            on = tree.render(shapes, W, H, point_size=2.0, gamma=2.2, max_nodes=5, show_octree_nodes=outlines, terrain=[scene["ground"]],
                             camera_positions=cams, terrain_window=16)
            st = ctx.kernel_stats()
            assert st["render_terrain_gather_kernel"][0] == 1 and st["render_terrain_edges_kernel"][0] == 1 and st["render_resolve_kernel"][0] == 1
            assert st["render_outline_kernel"][0] == (1 if outlines else 0) and st["render_splat_kernel"][0] == 1
            assert not np.array_equal(on.images().cpu().numpy(), ref[0])
            on.close()
            base.close()
    finally:
        ctx.set_profiling(False)


def listing(directory):
    return sorted(os.listdir(directory))


def test_written_opened_and_made_from_tiles(ctx, scene, tmp_path):  # noqa: F811
    mats, cams = views()
    shapes = frusta(ctx, mats)
    kw = dict(point_size=2.0, camera_positions=cams, terrain_window=16)
    built = scene["tree"].render(shapes, W, H, terrain=[scene["tilted"]], **kw)
    ref = built.images().cpu().numpy(), built.depth().cpu().numpy(), [built.terrain_info(v, 0) for v in range(4)]
    assert sum(t["pixels_won"] for t in ref[2]) > 100
    built.close()
    d1, d2, d3 = tmp_path / "a", tmp_path / "b", tmp_path / "c"
    scene["tilted"].write(d1)
    opened = ctx.terrain_open(d1)
    assert np.array_equal(opened.tiles(), scene["tilted"].tiles()) and opened.info()["finished"] and opened.info()["tiles"] == 4
    assert np.array_equal(opened.heights().view(np.uint32), scene["tilted"].heights().view(np.uint32))
    assert np.array_equal(opened.colors(device=True).cpu().numpy(), scene["tilted"].colors())
    opened.write(d2)
    assert listing(d1) == listing(d2) and len(listing(d1)) == 9
    assert filecmp.cmpfiles(d1, d2, listing(d1), shallow=False) == (listing(d1), [], [])
    # the tiles again in another order, from host arrays and from device tensors; and the directory by its name
    import torch
    rd = pcv.read_terrain(d1)
    order = np.array([2, 0, 3, 1])
    shuffled = dict(rd, tiles=rd["tiles"][order], heights=rd["heights"][order], colors=rd["colors"][order])
    on_device = dict(shuffled, heights=torch.from_numpy(shuffled["heights"]).to(f"cuda:{ctx.device}"),
                     colors=torch.from_numpy(shuffled["colors"]).to(f"cuda:{ctx.device}"))
    for layer in (opened, ctx.terrain_from_tiles(**shuffled), ctx.terrain_from_tiles(**on_device), str(d1)):
        rv = scene["tree"].render(shapes, W, H, terrain=[layer], **kw)
        assert np.array_equal(rv.images().cpu().numpy(), ref[0]) and np.array_equal(rv.depth().cpu().numpy(), ref[1])
        assert [rv.terrain_info(v, 0) for v in range(4)] == ref[2]
        rv.close()
        if isinstance(layer, pcv.Terrain) and layer is not opened:
            assert np.array_equal(layer.tiles(), rd["tiles"])  # stored ascending by (x, y)
            layer.write(d3)
            assert filecmp.cmpfiles(d1, d3, listing(d1), shallow=False) == (listing(d1), [], [])
            layer.free()
    # what an imported terrain refuses
    for call, word in [(lambda: opened.counts(), "no point counts"), (lambda: opened.add_points([0.0], [0.0], [0.0], np.zeros((1, 3), np.uint8)), "no points"),
                       (lambda: opened.finish(), "no points")]:
        with pytest.raises(pcv.PcvError) as e:
            call()
        assert e.value.code == pcv.PCV_E_INVALID and word in str(e.value)
    opened.free()
    for bad, word in [(dict(rd, tiles=rd["tiles"][[0, 1, 2, 1]]), "twice"), (dict(rd, heights=rd["heights"][:3]), "heights"),
                      (dict(rd, tile_size=0), "tile_size"), (dict(rd, tile_size=4097), "tile_size")]:
        with pytest.raises(pcv.PcvError) as e:
            ctx.terrain_from_tiles(**bad)
        assert e.value.code == pcv.PCV_E_INVALID and word in str(e.value), str(e.value)
    empty = ctx.terrain_from_tiles(**dict(rd, tiles=rd["tiles"][:0], heights=rd["heights"][:0], colors=rd["colors"][:0]))
    rv = scene["tree"].render(shapes, W, H, terrain=[empty], **kw)
    assert all(rv.terrain_info(v, 0)["edges_submitted"] == 0 for v in range(4))
    rv.close()
    empty.free()
    # a directory that is not whole
    name = str(d2 / pcv.terrain_tile_name(*rd["tiles"][1]))
    with open(name + ".height", "ab") as f:
        f.write(b"\0")
    with pytest.raises(pcv.PcvError) as e:
        ctx.terrain_open(d2)
    assert e.value.code == pcv.PCV_E_INVALID and name + ".height" in str(e.value)
    os.remove(name + ".height")
    with pytest.raises(pcv.PcvError) as e:
        ctx.terrain_open(d2)
    assert e.value.code == pcv.PCV_E_IO and name + ".height" in str(e.value)
    with open(d2 / "meta.json", "r+") as f:
        f.truncate(60)
    with pytest.raises(pcv.PcvError) as e:
        ctx.terrain_open(d2)
    assert e.value.code == pcv.PCV_E_INVALID and "meta.json" in str(e.value)


def test_the_viewers_window_of_1024(ctx, scene):  # noqa: F811
    mats, cams = views()
    mats, cams = mats[:2], cams[:2]
    rv = scene["tree"].render(frusta(ctx, mats), W, H, point_size=2.0, terrain=[scene["ground"]], camera_positions=cams)  # terrain_window: 1024
    wants = check_views(rv, scene["tn"], mats, cams, W, H, [scene["ground_dict"]], 1024, 2.0)
    assert wants[0]["terrain"][0]["pos"][0] < -500 and wants[0]["terrain"][0]["pixels_won"] > 50
    # the whole terrain lies inside the window: the image is that of a window of 64 around the same camera
    small = scene["tree"].render(frusta(ctx, mats), W, H, point_size=2.0, terrain=[scene["ground"]], camera_positions=cams, terrain_window=64)
    assert np.array_equal(small.images().cpu().numpy(), rv.images().cpu().numpy())
    assert small.terrain_info(0, 0)["edges_submitted"] == rv.terrain_info(0, 0)["edges_submitted"]
    small.close()
    rv.close()
