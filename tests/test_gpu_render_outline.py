"""show_octree_nodes on the device (pcv_render_views_ex) against the numpy oracle of
tests/render_outline_oracle.py over the CPU oracle's node bytes and visible lists: images, depth planes, every pcv_render_info
field and the outline info, byte for byte; no tolerance anywhere. Trees of a few thousand points, images of 64 x 48 and 33 x 17."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import point_cloud_viewer_amd as pcv
import render_oracle as R
import render_outline_oracle as RO
import xray_pyramid_oracle as P
from test_gpu_query import ctx, random_frusta  # noqa: F401  (module fixture + the config-4 frustum generator)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 64, 48
BMIN, BMAX = np.zeros(3), np.full(3, 64.0)  # a power-of-two cube: every node cube plane is an exactly representable number
CAP = 600


def cloud(n=3000, seed=21, lattice=False):
    """Three Gaussian clusters clipped to the cube; `lattice`: plus points on the corners and edge midpoints of the node cubes
    of the first three levels that lie on the cube's 12 edges — with a Float32-coded level they decode to those positions."""
    rng = np.random.default_rng(seed)
    centres = rng.uniform(12.0, 52.0, (3, 3))
    p = np.clip(np.concatenate([c + rng.normal(0.0, s, (n // 3, 3)) for c, s in zip(centres, (2.0, 5.0, 9.0))]), 0.0, 64.0)
    if lattice:
        t = np.arange(0.0, 64.1, 8.0)
        ends = [(a, b) for a in (0.0, 64.0) for b in (0.0, 64.0)]
        on = [np.stack([t, np.full_like(t, a), np.full_like(t, b)], axis=1)[:, order] for a, b in ends for order in ([0, 1, 2], [1, 0, 2], [1, 2, 0])]
        p = np.concatenate([p, np.concatenate(on)])
        p = p[rng.permutation(p.shape[0])]
    rgb = rng.integers(1, 255, (p.shape[0], 3), dtype=np.uint8)  # never the outline's colours of these tests
    return p, rgb


def build_scene(ctx, p, rgb, resolution=0.001, cap=CAP):  # noqa: F811
    x, y, z = (p[:, a].copy() for a in range(3))
    tree = ctx.build(resolution, pcv.Aabb(BMIN, BMAX), x, y, z, rgb, None, max_points_per_node=cap)
    with O.max_points_per_node(cap):
        want = O.build_closed(resolution, BMIN, BMAX, x, y, z, rgb, None, threads=4)
    return dict(tree=tree, oracle=want, tn=R.TreeNodes(want, BMIN, BMAX), x=x, y=y, z=z, rgb=rgb)


@pytest.fixture(scope="module")
def scene(ctx):  # noqa: F811
    s = build_scene(ctx, *cloud())
    assert 8 < s["tree"].num_nodes <= 60
    yield s
    s["tree"].free()


@pytest.fixture(scope="module")
def mats():
    """8 config-4-style frusta; the first looks at the cloud from inside the cube (not from a cube plane: with a corner at
    w == 0 the reference's traversal panics)."""
    rng = np.random.default_rng(77)
    fr = [c for c, _ in random_frusta(rng, BMIN, BMAX, 7)]
    inside, _ = O.frustum_new([31.3, 33.7, 50.1], [0.0, 0.0, 0.0, 1.0], O.perspective3_new(1.0, 1.2, 0.1, 100.0))
    return [inside] + fr


_oracle_cache = {}


def oracle_view(tn, m, w, h, point_size, gamma, max_nodes, color):
    """One oracle frame, computed once per (tree, arguments) and never changed afterwards."""
    key = (id(tn), np.asarray(m, np.float64).tobytes(), w, h, point_size, gamma, max_nodes, tuple(color))
    if key not in _oracle_cache:
        _oracle_cache[key] = RO.render_view(tn, m, w, h, point_size, gamma, max_nodes, None, color)
    return _oracle_cache[key]


def check_views(rv, tn, mats, w, h, point_size=1.0, gamma=1.0, max_nodes=0, color=RO.YELLOW):  # noqa: F811
    """Every view of `rv` against the oracle with outlines; returns the oracle's results."""
    imgs, dep = rv.images().cpu().numpy(), rv.depth().cpu().numpy()
    assert imgs.shape == (len(mats), h, w, 4) and dep.shape == (len(mats), h, w) and dep.dtype == np.float32
    wants = []
    for v, m in enumerate(mats):
        want = oracle_view(tn, m, w, h, point_size, gamma, max_nodes, color)
        info, oinfo = rv.info(v), rv.outline_info(v)
        if want["status"] is None:  # the reference panics: a cleared image, no outlines
            assert info["status"] in (1, 2) and info["nodes_drawn"] == 0 and info["points_submitted"] == 0, (v, info)
            assert oinfo == dict(segments_submitted=0, segments_drawn=0, outline_pixels=0), (v, oinfo)
        else:
            assert info["status"] == 0 and info["nodes_visible"] == want["nodes_visible"] and info["nodes_drawn"] == len(want["drawn"]), (v, info)
        for k in ("points_submitted", "points_drawn", "pixels_covered"):
            assert info[k] == want[k], (v, k, info[k], want[k])
        for k in ("segments_submitted", "segments_drawn", "outline_pixels"):
            assert oinfo[k] == want[k], (v, k, oinfo[k], want[k])
        assert np.array_equal(imgs[v], want["image"]), (v, int((imgs[v] != want["image"]).any(axis=-1).sum()))
        assert np.array_equal(dep[v].view(np.uint32), want["depth"].view(np.uint32)), v
        wants.append(want)
    return wants


def frusta(ctx, mats):  # noqa: F811
    return ctx.shapes([("frustum", m) for m in mats])


def raw_ex(ctx, tree, shapes, overlay, **kw):  # noqa: F811
    """pcv_render_views_ex called as C would, with `overlay` a RenderOverlay or None."""
    p, h = pcv.render_params(**kw), C.c_void_p()
    ctx._check(ctx.lib.pcv_render_views_ex(ctx.handle, shapes.handle, tree.handle, C.byref(p), C.byref(overlay) if overlay is not None else None,
                                           C.byref(h)))
    return pcv.RenderedViews(ctx, h, shapes.count, kw["width"], kw["height"], False)


def test_no_overlay_is_render_views(ctx, scene, mats):  # noqa: F811
    tree, shapes = scene["tree"], frusta(ctx, mats)
    kw = dict(width=W, height=H, point_size=2.0, gamma=2.2, max_nodes=5)
    ctx.set_profiling(True)
    try:
        ctx.reset_kernel_stats()
        base = tree.render(shapes, W, H, point_size=2.0, gamma=2.2, max_nodes=5)
        plain = {k: v[0] for k, v in ctx.kernel_stats().items() if v[0]}
        ref = base.images().cpu().numpy(), base.depth().cpu().numpy(), [base.info(v) for v in range(len(mats))]
        assert (ref[0][..., :3] != 0).any()
        for overlay in (None, pcv.render_overlay(False, (1, 2, 3, 4))):
            ctx.reset_kernel_stats()
            rv = raw_ex(ctx, tree, shapes, overlay, **kw)
            assert {k: v[0] for k, v in ctx.kernel_stats().items() if v[0]} == plain and "render_outline_kernel" not in plain
            assert np.array_equal(rv.images().cpu().numpy(), ref[0]) and np.array_equal(rv.depth().cpu().numpy(), ref[1])
            assert [rv.info(v) for v in range(len(mats))] == ref[2]
            assert all(rv.outline_info(v) == dict(segments_submitted=0, segments_drawn=0, outline_pixels=0) for v in range(len(mats)))
            rv.close()
        ctx.reset_kernel_stats()
        on = tree.render(shapes, W, H, point_size=2.0, gamma=2.2, max_nodes=5, show_octree_nodes=True)
        st = ctx.kernel_stats()
        assert st["render_outline_kernel"][0] == 1 and st["render_splat_kernel"][0] == 1 and st["render_resolve_kernel"][0] == 1
        assert not np.array_equal(on.images().cpu().numpy(), ref[0])
        on.close()
        base.close()
    finally:
        ctx.set_profiling(False)
    with pytest.raises(pcv.PcvError) as e:
        raw_ex(ctx, tree, shapes, pcv.render_overlay(flags=5), **kw)
    assert e.value.code == pcv.PCV_E_INVALID and "unknown overlay flag" in str(e.value)
    with pytest.raises(pcv.PcvError):
        base.outline_info(0)  # closed


@pytest.mark.parametrize("point_size,color", [(1.0, RO.YELLOW), (7.0, (0, 128, 255, 200))])
def test_views_equal_the_oracle(ctx, scene, mats, point_size, color):  # noqa: F811
    rv = scene["tree"].render(frusta(ctx, mats), W, H, point_size=point_size, gamma=2.2, depth=True, show_octree_nodes=True, outline_color=color)
    wants = check_views(rv, scene["tn"], mats, W, H, point_size, 2.2, color=color)
    assert sum(w["outline_pixels"] for w in wants) > 300 and sum(w["outline_pixels"] > 0 for w in wants) >= 3
    assert max(w["nodes_visible"] for w in wants) > 8 and sum(w["segments_drawn"] for w in wants) < sum(w["segments_submitted"] for w in wants)
    with pytest.raises(pcv.PcvError):
        rv.outline_info(len(mats))
    rv.close()


def test_max_nodes_and_a_singular_matrix(ctx, scene, mats):  # noqa: F811
    views = [mats[0], np.zeros(16), mats[1]]
    shapes, images = frusta(ctx, views), {}
    for max_nodes in (1, 3, 0):
        rv = scene["tree"].render(shapes, W, H, point_size=2.0, max_nodes=max_nodes, show_octree_nodes=True)
        wants = check_views(rv, scene["tn"], views, W, H, 2.0, max_nodes=max_nodes)
        assert wants[0]["nodes_visible"] > 3 and wants[0]["segments_submitted"] == 12 * (max_nodes or wants[0]["nodes_visible"])
        assert rv.info(1)["status"] == 1 and rv.outline_info(1) == dict(segments_submitted=0, segments_drawn=0, outline_pixels=0)
        assert (rv.images(1, 1).cpu().numpy()[0] == [0, 0, 0, 255]).all() and (rv.depth(1, 1).cpu().numpy() == 1.0).all()
        images[max_nodes] = rv.images().cpu().numpy()
        rv.close()
    assert not np.array_equal(images[1][0], images[3][0]) and not np.array_equal(images[3][0], images[0][0])


def edge_kinds(tn, names, m):
    """What the clip does to the edges of the drawn cubes of one view, from their clip coordinates alone."""
    kinds = set()
    for name in names:
        nd = tn.node(name)
        for a, b in RO.box_segments(nd["cube_min"], nd["cube_edge"], m):
            (x0, y0, z0, w0), (x1, y1, z1, w1) = (float(v) for v in a), (float(v) for v in b)
            if (w0 <= 0) != (w1 <= 0):
                kinds.add("behind the eye")
            if min(w0, w1) > 0:
                if (w0 + z0 < 0) != (w1 + z1 < 0):
                    kinds.add("near")
                if (w0 - z0 < 0) != (w1 - z1 < 0):
                    kinds.add("far")
                if (w0 - x0 < 0) != (w1 - x1 < 0) or (w0 + x0 < 0) != (w1 + x1 < 0) or (w0 - y0 < 0) != (w1 - y1 < 0) or (w0 + y0 < 0) != (w1 + y1 < 0):
                    kinds.add("side")
            if RO.clip_segment(a, b) is None:
                kinds.add("outside")
            elif max(abs(x0), abs(y0), abs(z0)) <= w0 and max(abs(x1), abs(y1), abs(z1)) <= w1:
                kinds.add("inside")
    return kinds


def clip_views(tn):
    """Cameras for every way an edge can meet the clip volume: inside a leaf's cube (twice, the second turned), just inside
    the root's cube with a far plane in the middle of the cloud, outside with near and far planes that cut the cloud, and one
    that looks away from everything."""
    leaf = max(tn.nodes, key=len)
    nd = tn.node(leaf)
    centre = np.asarray(nd["cube_min"]) + nd["cube_edge"] / 2
    short = O.perspective3_new(1.5, 1.0, 0.5, 25.0)
    views = [O.frustum_new(centre, [0.0, 0.0, 0.0, 1.0], O.perspective3_new(1.0, 1.5, nd["cube_edge"] / 64, 200.0))[0],
             O.frustum_new(centre, O.quat_from_axis_angle([0.0, 1.0, 0.0], 1.9), short)[0],
             O.frustum_new([31.0, 33.0, 63.5], [0.0, 0.0, 0.0, 1.0], short)[0],
             O.frustum_new([32.0, 32.0, 70.0], O.quat_from_axis_angle([1.0, 0.0, 0.0], 0.4), O.perspective3_new(1.0, 0.8, 10.0, 40.0))[0],
             O.frustum_new([32.0, 32.0, 200.0], O.quat_from_axis_angle([1.0, 0.0, 0.0], 3.0), short)[0]]
    return leaf, views


@pytest.mark.parametrize("size", [(W, H), (33, 17)])
def test_edges_across_every_clip_plane(ctx, scene, size):  # noqa: F811
    tn = scene["tn"]
    leaf, views = clip_views(tn)
    w, h = size
    rv = scene["tree"].render(frusta(ctx, views), w, h, point_size=1.0, show_octree_nodes=True)
    wants = check_views(rv, tn, views, w, h, 1.0)
    kinds = [edge_kinds(tn, wt["drawn"], m) for wt, m in zip(wants, views)]
    assert set().union(*kinds) == {"behind the eye", "near", "far", "side", "outside", "inside"}, kinds
    assert leaf in wants[0]["drawn"] and "behind the eye" in kinds[0]  # the camera inside a node's cube
    assert wants[0]["outline_pixels"] > 0 and sum(wt["outline_pixels"] > 0 for wt in wants) >= 3
    assert wants[-1]["outline_pixels"] == 0  # nothing in front of the last camera
    rv.close()


def tie_classes(want):
    """Pixels of one oracle frame where a node's outline fragment and the winner among the points share zw, by who is first:
    (the node's own point, a point of an earlier node, a point of a later node); and the pixels where an outline is hidden
    behind a nearer point / hides a farther point. The points' winner is read from the frame without outlines."""
    pts = want["points_only"]
    h, w = pts["depth"].shape
    pdepth, pwin = pts["depth"].reshape(-1), pts["winner"].reshape(-1)
    counts = np.diff(np.concatenate([want["first_rank"] - np.arange(len(want["first_rank"])), [pts["points_submitted"]]]))
    node_of_point = np.repeat(np.arange(len(counts)), counts)
    own = earlier = later = hidden = front = 0
    final_rank, final_depth = want["winner"].reshape(-1), want["depth"].reshape(-1)
    for k, (pix, zw) in enumerate(want["fragments"]):
        for p, z in zip(pix, zw):
            if pwin[p] < 0:
                continue
            if pdepth[p] == z:
                pk = node_of_point[pwin[p]]
                own, earlier, later = own + (pk == k), earlier + (pk < k), later + (pk > k)
                if pk <= k:  # (the outline may still win the pixel with a nearer fragment of another edge)
                    assert final_rank[p] != want["outline_rank"][k] or final_depth[p] < z
            elif pdepth[p] < z:
                hidden += 1
                assert final_rank[p] != want["outline_rank"][k] or final_depth[p] < z
            elif final_rank[p] == want["outline_rank"][k] and final_depth[p] == z:
                front += 1
    return own, earlier, later, hidden, front


def ortho(depth_scale=1.0):
    """Column-major matrix that maps the cube into 0.9 of the clip cube, w = 1, looking along z."""
    m = np.zeros((4, 4))
    for a in range(3):
        s = 0.9 / 32.0 * (depth_scale if a == 2 else 1.0)
        m[a, a], m[a, 3] = s, -s * 32.0
    m[3, 3] = 1.0
    return m.ravel(order="F")


def test_order_at_equal_depth(ctx):  # noqa: F811
    """Float32-coded nodes (resolution 1e-5 over a 64 m cube: 23 bits) with points planted on cube corners and edge midpoints:
    under an axis-aligned orthographic view a point on an edge has exactly the zw of that edge's fragments."""
    s = build_scene(ctx, *cloud(3000, seed=5, lattice=True), resolution=1e-5)
    tn, tree = s["tn"], s["tree"]
    assert {nd["encoding"] for nd in s["oracle"].nodes.values()} == {3} and 4 < tree.num_nodes <= 60
    views = [ortho(), ortho(depth_scale=1e-30)]  # real depths; then a depth so flat that only the draw order decides
    rv = tree.render(frusta(ctx, views), W, H, point_size=3.0, show_octree_nodes=True)
    wants = check_views(rv, tn, views, W, H, 3.0)
    total = np.zeros(5, np.int64)
    for m, want in zip(views, wants):
        want = dict(want, points_only=R.render_view(tn, m, W, H, 3.0, 1.0))
        total += tie_classes(want)
    assert (total > 0).all(), total  # own, earlier, later, hidden, in front
    rv.close()
    tree.free()


def test_groups_and_repeated_runs(ctx, scene, mats):  # noqa: F811
    shapes = frusta(ctx, mats)
    first = scene["tree"].render(shapes, W, H, point_size=2.0, show_octree_nodes=True)
    check_views(first, scene["tn"], mats, W, H, 2.0)
    ref = first.images().cpu().numpy(), first.depth().cpu().numpy(), [(first.info(v), first.outline_info(v)) for v in range(len(mats))]
    first.close()
    for ws in (None, 8 * W * H, 3 * 8 * W * H):  # the same again; one view per group; groups of three, three and two
        rv = scene["tree"].render(shapes, W, H, point_size=2.0, show_octree_nodes=True, max_workspace_bytes=ws)
        assert np.array_equal(rv.images().cpu().numpy(), ref[0]) and np.array_equal(rv.depth().cpu().numpy(), ref[1]), ws
        assert [(rv.info(v), rv.outline_info(v)) for v in range(len(mats))] == ref[2], ws
        rv.close()


@pytest.mark.parametrize("resolution,encoding", [(1.0, 1), (0.01, 2), (1e-5, 3), (1e-9, 4)])
def test_opened_directory_in_every_encoding(ctx, mats, tmp_path, resolution, encoding):  # noqa: F811
    p, rgb = cloud(2500, seed=9)
    x, y, z = (p[:, a].copy() for a in range(3))
    with O.max_points_per_node(CAP):
        want = O.build_closed(resolution, BMIN, BMAX, x, y, z, rgb, None, threads=4)
        O.build_literal_dir(tmp_path / "oracle", resolution, BMIN, BMAX, x, y, z, rgb, None, threads=4)
    tn = R.TreeNodes(want, BMIN, BMAX)
    assert want.nodes["r"]["encoding"] == encoding and 1 < len(want.nodes) <= 60
    opened = ctx.open_dir(tmp_path / "oracle")
    assert sorted(opened.node_names()) == sorted(want.nodes)
    views = [mats[0], ortho(), mats[1]]
    rv = opened.render(frusta(ctx, views), W, H, point_size=2.0, show_octree_nodes=True)
    wants = check_views(rv, tn, views, W, H, 2.0)
    assert wants[1]["outline_pixels"] > 50 and "r" in wants[1]["drawn"]
    rv.close()
    opened.free()


def test_c_example_draws_the_same_frame(ctx, scene, mats, tmp_path):  # noqa: F811
    scene["tree"].write_dir(tmp_path / "oct")
    out = tmp_path / "view.png"
    m = ortho()
    cmd = [os.path.join(ROOT, "examples", "bin", "render_view"), str(tmp_path / "oct"), "--matrix", *[repr(float(v)) for v in m],
           "--size", f"{W}x{H}", "--point-size", "2.5", "--gamma", "2.2", "--max-nodes", "6", "--show-octree-nodes", "-o", str(out)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    rv = scene["tree"].render(frusta(ctx, [m]), W, H, point_size=2.5, gamma=2.2, max_nodes=6, show_octree_nodes=True)
    want = rv.images().cpu().numpy()[0]
    info, oinfo = rv.info(0), rv.outline_info(0)
    assert (want == [255, 255, 0, 255]).all(axis=-1).sum() == oinfo["outline_pixels"] > 50
    assert np.array_equal(P.read_png(open(out, "rb").read()), want)
    assert [int(v) for v in p.stdout.split()] == [info["nodes_visible"], info["nodes_drawn"], info["points_submitted"], info["points_drawn"],
                                                  info["pixels_covered"], oinfo["segments_submitted"], oinfo["segments_drawn"], oinfo["outline_pixels"]]
    rv.close()
