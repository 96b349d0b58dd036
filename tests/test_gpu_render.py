"""The viewer's frame on the device (pcv_render_views) against the numpy oracle of tests/render_oracle.py: images,
depth planes and every info field, byte for byte; no tolerance anywhere."""
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import point_cloud_viewer_amd as pcv
import render_oracle as R
import xray_pyramid_oracle as P
from test_gpu_query import ctx, random_frusta, scene  # noqa: F401  (module fixtures + the config-4 frustum generator)
from test_gpu_query_batch import scene_of
from test_gpu_xray import ecef  # noqa: F401

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 96, 64


def tree_nodes(s):
    return R.TreeNodes(s["oracle"], s["bmin"], s["bmax"])


@pytest.fixture(scope="module")
def tn(scene):  # noqa: F811
    return tree_nodes(scene)


@pytest.fixture(scope="module")
def mats(scene):  # noqa: F811
    """8 config-4-style frusta; the first looks at the cloud from inside it, so that its points reach every border."""
    rng = np.random.default_rng(77)
    fr = [c for c, _ in random_frusta(rng, scene["bmin"], scene["bmax"], 7)]
    mid = (scene["bmin"] + scene["bmax"]) / 2
    inside, _ = O.frustum_new(mid, [0.0, 0.0, 0.0, 1.0], O.perspective3_new(1.0, 1.2, 0.1, 100.0))
    return [inside] + fr


def check_views(rv, tree, tn, mats, w, h, point_size=1.0, gamma=1.0, max_nodes=0, shapes=None):  # noqa: F811
    """Every view of `rv` against the oracle; returns the oracle's results."""
    imgs, dep = rv.images().cpu().numpy(), rv.depth().cpu().numpy()
    assert imgs.shape == (len(mats), h, w, 4) and imgs.dtype == np.uint8 and dep.shape == (len(mats), h, w) and dep.dtype == np.float32
    lut = R.gamma_lut(gamma)
    lists = tree.visible_nodes(shapes)[0] if shapes is not None else None
    names = tree.node_names() if shapes is not None else None
    wants = []
    for v, m in enumerate(mats):
        want = R.render_view(tn, m, w, h, point_size, gamma, max_nodes, lut)
        info = rv.info(v)
        if want["status"] is None:  # the reference panics: a cleared image and the traversal's status
            assert info["status"] in (1, 2) and info["nodes_drawn"] == 0 and info["points_submitted"] == 0, (v, info)
        else:
            assert info["status"] == 0 and info["nodes_visible"] == want["nodes_visible"] and info["nodes_drawn"] == len(want["drawn"]), (v, info)
            if lists is not None:  # nodes_visible and the drawn nodes are pcv_visible_nodes' own
                assert info["nodes_visible"] == len(lists[v])
                assert [names[i] for i in lists[v][:info["nodes_drawn"]]] == want["drawn"], v
        for k in ("points_submitted", "points_drawn", "pixels_covered"):
            assert info[k] == want[k], (v, k, info[k], want[k])
        assert np.array_equal(imgs[v], want["image"]), (v, int((imgs[v] != want["image"]).any(axis=-1).sum()))
        assert np.array_equal(dep[v].view(np.uint32), want["depth"].view(np.uint32)), v
        wants.append(want)
    return wants


def test_views_equal_the_oracle(ctx, scene, tn, mats):  # noqa: F811
    tree = scene["tree"]
    shapes = ctx.shapes([("frustum", m) for m in mats])
    rv = tree.render(shapes, W, H, depth=True)
    wants = check_views(rv, tree, tn, mats, W, H, shapes=shapes)
    assert sum(w["pixels_covered"] for w in wants) > 2000 and sum(w["pixels_covered"] > 0 for w in wants) >= 3
    assert max(w["nodes_visible"] for w in wants) > 10
    with pytest.raises(pcv.PcvError):
        rv.info(len(mats))
    rv.close()
    with pytest.raises(pcv.PcvError):
        rv.images()


@pytest.mark.parametrize("point_size", [1.0, 2.5, 7.0])
@pytest.mark.parametrize("gamma", [1.0, 2.2])
def test_point_size_and_gamma(ctx, scene, tn, mats, point_size, gamma):  # noqa: F811
    use = mats[:3]
    rv = scene["tree"].render(ctx.shapes([("frustum", m) for m in use]), W, H, point_size=point_size, gamma=gamma)
    wants = check_views(rv, scene["tree"], tn, use, W, H, point_size, gamma)
    inside = wants[0]["depth"] < 1.0  # the view from inside the cloud: drawn pixels on all four borders
    assert inside[0].any() and inside[-1].any() and inside[:, 0].any() and inside[:, -1].any()
    rv.close()


def ortho(bmin, bmax, depth_scale=1.0):
    """Column-major matrix that maps the box into 0.9 of the clip cube, w = 1; depth_scale 0 would flatten the depth."""
    c, e = (bmin + bmax) / 2, (bmax - bmin) / 2
    m = np.zeros((4, 4))
    for a in range(3):
        s = 0.9 / e[a] * (depth_scale if a == 2 else 1.0)
        m[a, a], m[a, 3] = s, -s * c[a]
    m[3, 3] = 1.0
    return m.ravel(order="F")


def small_scene(ctx, pts, rgb, cap=100_000):  # noqa: F811
    pts, rgb = np.asarray(pts, np.float64), np.asarray(rgb, np.uint8)
    bmin, bmax = pts.min(axis=0), pts.max(axis=0)
    s = scene_of(ctx, pts[:, 0].copy(), pts[:, 1].copy(), pts[:, 2].copy(), rgb, None, bmin, bmax, cap)
    return s, tree_nodes(s)


def test_depth_order_and_ties(ctx, scene, tn, mats):  # noqa: F811
    # two points on one pixel at different depths, two exact duplicates (one leaf) with different colours, two corners
    pts = [[0, 0, 0], [8, 8, 8], [3, 3, 2], [3, 3, 6], [5, 2, 4], [5, 2, 4]]
    rgb = [[9, 9, 9], [99, 99, 99], [250, 0, 0], [0, 250, 0], [0, 0, 250], [250, 250, 0]]
    s, stn = small_scene(ctx, pts, rgb)
    m = ortho(s["bmin"], s["bmax"])
    rv = s["tree"].render(ctx.shapes([("frustum", m)]), 8, 8)
    want = check_views(rv, s["tree"], stn, [m], 8, 8)[0]
    assert want["points_drawn"] == 6 and want["pixels_covered"] == 4
    colours = {tuple(px[:3]) for px in want["image"].reshape(-1, 4) if tuple(px[:3]) != (0, 0, 0)}
    assert len(colours) == 4 and ((250, 0, 0) in colours) != ((0, 250, 0) in colours) and ((0, 0, 250) in colours) != ((250, 250, 0) in colours)
    rv.close()
    s["tree"].free()
    # several nodes: real depths, then a depth row so flat that every point has the same zw — the winner of every pixel is
    # decided by the draw rank alone, inside a node and across nodes
    rng = np.random.default_rng(5)
    pts = rng.uniform(0.0, 50.0, (6000, 3))
    rgb = rng.integers(1, 256, (6000, 3), dtype=np.uint8)
    s, stn = small_scene(ctx, pts, rgb, cap=500)
    views = [ortho(s["bmin"], s["bmax"]), ortho(s["bmin"], s["bmax"], depth_scale=1e-30)]
    rv = s["tree"].render(ctx.shapes([("frustum", m) for m in views]), 16, 12, point_size=2.0)
    wants = check_views(rv, s["tree"], stn, views, 16, 12, point_size=2.0)
    assert len(wants[0]["drawn"]) > 8 and wants[0]["pixels_covered"] == 16 * 12
    assert len(np.unique(wants[0]["depth"])) > 20 and len(np.unique(wants[1]["depth"])) == 1
    assert not np.array_equal(wants[0]["image"], wants[1]["image"])
    rv.close()
    s["tree"].free()
    # the same bytes over 5 runs, and with one view per group
    shapes = ctx.shapes([("frustum", m) for m in mats])
    first = scene["tree"].render(shapes, W, H, point_size=2.5)
    ref_img, ref_dep = first.images().cpu().numpy(), first.depth().cpu().numpy()
    first.close()
    for k in range(5):
        rv = scene["tree"].render(shapes, W, H, point_size=2.5, max_workspace_bytes=8 * W * H if k == 4 else None)
        assert np.array_equal(rv.images().cpu().numpy(), ref_img) and np.array_equal(rv.depth().cpu().numpy(), ref_dep), k
        rv.close()


def test_clip_planes(ctx):  # noqa: F811
    pts = [[0, 0, 0], [4, 4, 4], [1, 2, 3], [3, 1, 2], [2, 3, 1]]
    rgb = [[10, 20, 30], [40, 50, 60], [250, 0, 0], [0, 250, 0], [0, 0, 250]]
    s, stn = small_scene(ctx, pts, rgb)
    root = stn.node("r")
    p = R.attribute(root["encoding"], root["xyz"]) * root["cube_edge"] + root["cube_min"][None, :]  # the shader's positions
    k = int(np.argmin(np.abs(p - np.array([1.0, 2.0, 3.0])).sum(axis=1)))
    one_up = float(np.nextafter(np.float32(1.0), np.float32(2.0)))

    def translate(tx, ty, tz, w_row=(0.0, 0.0, 0.0, 1.0)):
        m = np.eye(4)
        m[:3, 3] = [tx, ty, tz]
        m[:3, :3] *= 0.2
        m[3] = w_row
        return m.ravel(order="F")
    q = 0.2 * p[k]
    views = [translate(1.0 - q[0], -q[1], -q[2]),            # x == w: drawn, on the last column's right edge
             translate(one_up - q[0], -q[1], -q[2]),         # one f32 step outside
             translate(-q[0], -q[1], -1.0 - q[2]),           # z == -w: drawn at depth 0
             translate(-q[0], -q[1], -one_up - q[2]),        # one f32 step in front of the near plane
             translate(-q[0], -q[1], -q[2], (0.0, 0.0, 1.0, -p[k][2])),         # w == 0 for the point, < 0 and > 0 for others
             translate(-q[0], -q[1], -q[2], (0.0, 0.0, -1.0, p[k][2] - 0.5))]   # w < 0 for most
    on = []
    for m in views:
        x, y, z, w = R.clip_f32(m, p[k:k + 1])
        on.append((float(x[0]), float(z[0]), float(w[0])))
    assert on[0][0] == 1.0 and on[1][0] == one_up and on[2][1] == -1.0 and on[3][1] == -one_up and on[4][2] == 0.0 and on[5][2] < 0
    rv = s["tree"].render(ctx.shapes([("frustum", m) for m in views]), 16, 16, point_size=3.0)
    wants = check_views(rv, s["tree"], stn, views, 16, 16, point_size=3.0)
    assert all(w["status"] == 0 for w in wants)
    assert wants[0]["points_drawn"] == wants[1]["points_drawn"] + 1 and wants[2]["points_drawn"] == wants[3]["points_drawn"] + 1
    assert (wants[2]["depth"] == 0.0).any() and not (wants[3]["depth"] == 0.0).any()
    assert 0 < wants[4]["points_drawn"] < 5
    rv.close()
    s["tree"].free()


def test_max_nodes_and_a_singular_matrix(ctx, scene, tn, mats):  # noqa: F811
    tree = scene["tree"]
    views = [mats[0], np.zeros(16), mats[1]]
    shapes = ctx.shapes([("frustum", m) for m in views])
    images = {}
    for max_nodes in (1, 3, 0):
        rv = tree.render(shapes, W, H, point_size=2.0, max_nodes=max_nodes)
        wants = check_views(rv, tree, tn, views, W, H, point_size=2.0, max_nodes=max_nodes, shapes=shapes)
        assert wants[0]["nodes_visible"] > 3 and len(wants[0]["drawn"]) == (max_nodes or wants[0]["nodes_visible"])
        info = rv.info(1)
        assert info["status"] == 1 and info["nodes_visible"] == 0 and info["pixels_covered"] == 0
        img = rv.images(1, 1).cpu().numpy()[0]
        assert (img == [0, 0, 0, 255]).all() and (rv.depth(1, 1).cpu().numpy() == 1.0).all()
        images[max_nodes] = rv.images().cpu().numpy()
        rv.close()
    assert not np.array_equal(images[1][0], images[3][0]) and not np.array_equal(images[3][0], images[0][0])
    # the other views do not depend on their neighbour
    alone = tree.render(ctx.shapes([("frustum", mats[1])]), W, H, point_size=2.0)
    assert np.array_equal(alone.images().cpu().numpy()[0], images[0][2])
    alone.close()


def test_four_encodings_and_opened_directory(ctx, ecef, tmp_path):  # noqa: F811
    s = ecef
    x, y, z, rgb, inten, bmin, bmax = (s[k] for k in ("x", "y", "z", "rgb", "inten", "bmin", "bmax"))
    etn = tree_nodes(s)
    c = np.array([x[0], y[0], z[0]])  # the dense centimetre-scale cluster: Uint8 .. Float64 nodes on the way down to it
    persp = O.perspective3_new(1.5, 1.0, 1.0, 80_000.0)
    views = [O.frustum_new(c + np.array([0.0, 0.0, 30_000.0]), [0.0, 0.0, 0.0, 1.0], persp)[0],
             O.frustum_new(c + np.array([0.0, 0.0, 2.0]), [0.0, 0.0, 0.0, 1.0], O.perspective3_new(1.5, 1.0, 0.01, 100.0))[0],
             ortho(bmin, bmax)]
    with O.max_points_per_node(1500):  # the fixture's own cap: the directory holds the tree the oracle nodes describe
        O.build_literal_dir(tmp_path / "oracle", 0.001, bmin, bmax, x, y, z, rgb, inten, threads=4)
    opened = ctx.open_dir(tmp_path / "oracle")
    assert sorted(opened.node_names()) == sorted(s["names"])
    shapes = ctx.shapes([("frustum", m) for m in views])
    rv = opened.render(shapes, W, H, point_size=2.0, gamma=2.2)
    wants = check_views(rv, opened, etn, views, W, H, point_size=2.0, gamma=2.2)
    drawn = {n for w in wants for n in w["drawn"]}
    assert {s["oracle"].nodes[n]["encoding"] for n in drawn} == {1, 2, 3, 4}
    assert all(w["pixels_covered"] > 0 for w in wants)
    built = s["tree"].render(shapes, W, H, point_size=2.0, gamma=2.2)
    assert np.array_equal(built.images().cpu().numpy(), rv.images().cpu().numpy())
    built.close()
    rv.close()
    opened.free()


def test_invalid_input(ctx, scene, mats):  # noqa: F811
    tree = scene["tree"]
    frusta = ctx.shapes([("frustum", mats[0])])
    with pytest.raises(pcv.PcvError) as e:
        tree.render(ctx.shapes([("frustum", mats[0]), ("aabb", scene["bmin"], scene["bmax"])]), W, H)
    assert e.value.code == pcv.PCV_E_INVALID
    for kw in (dict(point_size=64.5), dict(point_size=0.5), dict(gamma=0.0)):
        with pytest.raises(pcv.PcvError) as e:
            tree.render(frusta, W, H, **kw)
        assert e.value.code == pcv.PCV_E_INVALID
    with pytest.raises(pcv.PcvError) as e:
        tree.render(frusta, W, 16385)
    assert e.value.code == pcv.PCV_E_INVALID
    import torch
    torch.cuda.synchronize()
    before = torch.cuda.mem_get_info()[0]
    with pytest.raises(pcv.PcvError) as e:
        tree.render(frusta, 16384, 16384, max_workspace_bytes=1 << 20)
    assert e.value.code == pcv.PCV_E_OOM
    # nothing is held: the smallest thing the call could leak is the view's 1 GiB image (its key plane is 2 GiB); the margin
    # is for what the runtime itself moves
    assert torch.cuda.mem_get_info()[0] >= before - (256 << 20)
    rv = tree.render(frusta, W, H)  # the next call succeeds
    assert rv.info(0)["status"] == 0
    rv.close()


def test_write_png(ctx, scene, mats, tmp_path):  # noqa: F811
    rv = scene["tree"].render(ctx.shapes([("frustum", m) for m in mats[:2]]), W, H, point_size=3.0, gamma=2.2)
    paths = rv.write_png(tmp_path / "frames")
    imgs = rv.images().cpu().numpy()
    assert len(paths) == 2
    for v, path in enumerate(paths):
        assert np.array_equal(P.read_png(open(path, "rb").read()), imgs[v]), v
    rv.close()


def test_c_example_draws_the_same_frame(ctx, scene, mats, tmp_path):  # noqa: F811
    scene["tree"].write_dir(tmp_path / "oct")
    out = tmp_path / "view.png"
    cmd = [os.path.join(ROOT, "examples", "bin", "render_view"), str(tmp_path / "oct"), "--matrix", *[repr(float(v)) for v in mats[0]],
           "--size", f"{W}x{H}", "--point-size", "2.5", "--gamma", "2.2", "--max-nodes", "40", "-o", str(out)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    rv = scene["tree"].render(ctx.shapes([("frustum", mats[0])]), W, H, point_size=2.5, gamma=2.2, max_nodes=40)
    want = rv.images().cpu().numpy()[0]
    assert (want[..., :3] != 0).any()
    assert np.array_equal(P.read_png(open(out, "rb").read()), want)
    rv.close()
