"""pcv_xray_build_parents / _nodes / _node_images / _write_dir (xray's parent levels and quadtree directory on the
device) against tests/xray_pyramid_oracle.py: every parent byte for byte from the GPU's own leaves, the whole pyramid from
the leaf oracle, the node list of create_non_leaf_nodes, awkward tile sizes, sparse sets under non-root roots, edge cases,
errors, and the directory (PNG pixels, meta.pb) from Python and from the C example."""
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import point_cloud_viewer_amd as pcv
import xray_oracle as X
import xray_pyramid_oracle as P
from point_cloud_viewer_amd import synthetic
from test_gpu_query import ctx, scene  # noqa: F401  (module fixtures)
from test_gpu_xray import tree_points

pytestmark = pytest.mark.gpu
W, PX = 64, 0.25  # the 300 000-point scene: deepest level 3, 64 leaves of 16 m
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRATEGIES = ["xray", "colored", ("height_stddev", 1.5, "jet")]


@pytest.fixture(scope="module")
def tp(scene):  # noqa: F811
    return tree_points(scene)


def pyramid_of(xt, background, root="r"):
    """The restatement over the GPU's own leaves: {(level, index): image}, children counts."""
    leaves = xt.node_images(0, xt.num_created)
    idx = [int(xt.leaf_index[int(c)]) for c in xt.created]
    return P.pyramid(dict(zip(idx, leaves)), xt.deepest_level, X.node_id(root)[0], xt.tile_size_px, background)


def check_nodes(xt, root="r"):
    level, index = xt.nodes()
    idx = [int(xt.leaf_index[int(c)]) for c in xt.created]
    want = P.node_list(idx, xt.deepest_level, X.node_id(root)[0])
    assert list(zip(level.tolist(), index.tolist())) == want
    return want


def check_pyramid(xt, want_imgs, nodes):
    got = xt.node_images()
    assert got.shape[0] == len(nodes)
    for k, n in enumerate(nodes):
        assert np.array_equal(got[k], want_imgs[n]), (X.node_name(*n), int((got[k] != want_imgs[n]).any(-1).sum()))


@pytest.mark.parametrize("background", ["white", "transparent"])
@pytest.mark.parametrize("strategy", STRATEGIES, ids=["xray", "colored", "height_stddev"])
def test_parents_from_the_gpus_leaves(scene, strategy, background):  # noqa: F811
    xt = scene["tree"].xray_quadtree(W, PX, strategy, background=background)
    nodes = check_nodes(xt)
    assert xt.deepest_level == 3 and len(nodes) > xt.num_created > 8
    want, _ = pyramid_of(xt, background)
    check_pyramid(xt, want, nodes)
    assert nodes[-1] == (0, 0)


def test_whole_pyramid_against_the_oracle(scene, tp):  # noqa: F811
    xt = scene["tree"].xray_quadtree(W, PX, "xray")
    leaves, g = X.xray_tiles(tp, W, PX, "xray")
    idx = {n: i for n, i in zip(g["leaf_ids"], g["leaf_index"])}
    want, _ = P.pyramid({idx[n]: im for n, (im, _) in leaves.items()}, g["deepest_level"], 0, W, "white")
    nodes = check_nodes(xt)
    assert set(nodes) == set(want)
    check_pyramid(xt, want, nodes)


@pytest.mark.parametrize("tile", [1, 7, 33])
def test_awkward_tile_sizes(scene, tile):  # noqa: F811
    xt = scene["tree"].xray_quadtree(tile, 16.0 / tile, "colored", background="transparent")
    assert xt.deepest_level >= 2
    nodes = check_nodes(xt)
    want, _ = pyramid_of(xt, "transparent")
    check_pyramid(xt, want, nodes)


def test_sparse_sets_and_non_root_roots(scene, tmp_path):  # noqa: F811
    counts = set()
    for root, px in (("r", PX / 4), ("r1", PX / 4), ("r03", PX / 8)):
        xt = scene["tree"].xray_quadtree(W, px, "xray", intensity_interval=(20.0, 140.0), root_node_id=root)
        nodes = check_nodes(xt, root)
        assert xt.num_created > 4, root
        assert all(X.node_name(*n).startswith(root) for n in nodes) and nodes[-1] == X.node_id(root)
        want, nch = pyramid_of(xt, "white", root)
        check_pyramid(xt, want, nodes)
        counts |= {1 if c == 1 else (4 if c == 4 else 2) for c in nch.values()}
        xt.write(tmp_path / root)
        files = set(os.listdir(tmp_path / root))
        assert files == {X.node_name(*n) + ".png" for n in nodes} | {P.meta_file_name(root)}
        meta = P.decode_meta((tmp_path / root / P.meta_file_name(root)).read_bytes())
        assert meta["rect"] == P.root_rect(xt.bounding_rect, root) and meta["nodes"] == nodes
        xt.free()
    assert counts == {1, 2, 4}, counts


def test_edge_cases(ctx, scene, tmp_path):  # noqa: F811
    tree = scene["tree"]
    xt = tree.xray_quadtree(W, PX, "xray", intensity_interval=(5.0, 4.0))  # nothing passes: no leaf, no parent
    assert xt.num_created == 0 and xt.node_ids == [] and xt.node_images().shape == (0, W, W, 4)
    xt.write(tmp_path / "empty")
    assert os.listdir(tmp_path / "empty") == ["meta.pb"]
    meta = P.decode_meta((tmp_path / "empty" / "meta.pb").read_bytes())
    assert meta["nodes"] == [] and meta["version"] == 3 and meta["deepest_level"] == 3 and meta["tile_size"] == W
    # root_node_id at the deepest level: the root is the one leaf, there are no parents
    full = tree.xray_tiles(W, PX, "xray")
    leaf = full.created_ids[0]
    xt = tree.xray_tiles(W, PX, "xray", root_node_id=leaf)
    assert ctx.lib.pcv_xray_write_dir(xt.handle, os.fsencode(str(tmp_path / "leaf"))) == pcv.PCV_OK  # nothing to build first
    xt.build_parents()
    assert xt.node_ids == [leaf] and np.array_equal(xt.node_images()[0], full.images(0, 1)[0])
    assert sorted(os.listdir(tmp_path / "leaf")) == sorted([leaf + ".png", P.meta_file_name(leaf)])


def test_repeat_and_errors(ctx, scene, tmp_path):  # noqa: F811
    tree = scene["tree"]
    a = tree.xray_quadtree(W, PX, "colored")
    b = tree.xray_quadtree(W, PX, "colored")
    assert a.node_ids == b.node_ids and np.array_equal(a.node_images(), b.node_images())
    before = a.node_images()
    a.build_parents()  # a second call is a no-op
    assert np.array_equal(a.node_images(), before)
    n = len(a.node_ids)
    buf = np.zeros((2, W, W, 4), np.uint8)
    assert ctx.lib.pcv_xray_node_images(a.handle, n - 1, 2, buf.nbytes, pcv._lib.MEM_HOST, buf.ctypes.data) == pcv.PCV_E_INVALID
    assert ctx.lib.pcv_xray_node_images(a.handle, n + 1, 0, buf.nbytes, pcv._lib.MEM_HOST, buf.ctypes.data) == pcv.PCV_E_INVALID
    assert not buf.any()
    leaves_only = tree.xray_tiles(W, PX, "colored")
    assert len(leaves_only.node_ids) == leaves_only.num_created  # before build_parents: the leaves
    assert ctx.lib.pcv_xray_write_dir(leaves_only.handle, os.fsencode(str(tmp_path / "early"))) == pcv.PCV_E_INVALID
    assert not (tmp_path / "early").exists()
    with pytest.raises(pcv.PcvError):
        leaves_only.write(tmp_path / "early")
    dev = a.node_images(a.num_created, 3, device=True)
    assert np.array_equal(dev.cpu().numpy(), before[a.num_created:a.num_created + 3])


def test_directory(scene, tmp_path):  # noqa: F811
    xt = scene["tree"].xray_quadtree(W, PX, ("height_stddev", 1.5, "purplish"), background="transparent")
    out = tmp_path / "q"
    out.mkdir()
    (out / "r.png").write_bytes(b"stale")  # overwritten
    xt.write(out)
    ids = xt.node_ids
    assert set(os.listdir(out)) == {n + ".png" for n in ids} | {"meta.pb"}
    imgs = xt.node_images()
    for k, n in enumerate(ids):
        assert np.array_equal(P.read_png((out / (n + ".png")).read_bytes()), imgs[k]), n
    meta = P.decode_meta((out / "meta.pb").read_bytes())
    level, index = xt.nodes()
    assert meta == dict(version=3, rect=tuple(xt.bounding_rect), deepest_level=3, tile_size=W,
                        nodes=list(zip(level.tolist(), index.tolist())))


def test_example_writes_the_same_directory(ctx, scene, tmp_path):  # noqa: F811
    s = scene
    inten = (np.arange(s["x"].size) % 251).astype(np.float32)
    rgb = synthetic.index_colors(s["x"].size)
    O.build_literal_dir(tmp_path / "octree", 0.001, s["bmin"], s["bmax"], s["x"], s["y"], s["z"], rgb, inten, threads=4)
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "examples")])
    exe = os.path.join(ROOT, "examples", "bin", "build_xray_quadtree")
    p = subprocess.run([exe, str(tmp_path / "octree"), "--output-directory", str(tmp_path / "c"), "--resolution", str(PX), "--tile-size",
                        str(W), "--coloring-strategy", "colored", "--tile-background-color", "transparent", "--filter-interval",
                        "intensity=10,200", "--root-node-id", "r2"], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr
    opened = ctx.open_dir(tmp_path / "octree")
    xt = opened.xray_quadtree(W, PX, "colored", background="transparent", intensity_interval=(10.0, 200.0), root_node_id="r2")
    xt.write(tmp_path / "py")
    names = sorted(os.listdir(tmp_path / "py"))
    assert names == sorted(os.listdir(tmp_path / "c")) and "meta2.pb" in names and len(names) > 3
    for n in names:
        assert (tmp_path / "py" / n).read_bytes() == (tmp_path / "c" / n).read_bytes(), n
    xt.free()
    opened.free()
