"""pcv_xray_merge / pcv_xray_open_dir on the device: partial quadtrees built with root_node_id and merged must be the
quadtree of one whole build, node for node and byte for byte, with device-built parts, parts reopened from directories,
re-encoded PNGs, mixed parts, in place, with another background, and through the C example."""
import os
import struct
import subprocess

import numpy as np
import pytest

import point_cloud_viewer_amd as pcv
import xray_merge_oracle as MO
import xray_oracle as X
import xray_pyramid_oracle as P
from test_gpu_query import ctx  # noqa: F401  (module fixture)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, PX = 16, 0.5  # 8 m tiles over a 64 m square: deepest level 3
# patches of points as (x0, x1, y0, y1), strictly inside level-2 cells of 16 m; the level-2 cell (1, 1) = r03 and many
# others stay empty, while its level-1 parent r0 holds the first patch
PATCHES = [(1.0, 30.0, 1.0, 14.0), (41.0, 63.0, 35.0, 63.0), (2.0, 10.0, 50.0, 60.0), (50.0, 60.0, 3.0, 12.0)]


def cell_name(cx, cy, level):
    """NodeId of the cell (cx, cy) of the 2^level x 2^level grid: child index bit 1 = upper half in x, bit 0 in y."""
    return "r" + "".join(str((((cx >> l) & 1) << 1) | ((cy >> l) & 1)) for l in range(level - 1, -1, -1))


def make_cloud(ctx):  # noqa: F811
    rng = np.random.default_rng(42)
    n = 20_000
    which = rng.integers(0, len(PATCHES), n)
    lo = np.array([[p[0], p[2]] for p in PATCHES])[which]
    hi = np.array([[p[1], p[3]] for p in PATCHES])[which]
    xy = lo + rng.random((n, 2)) * (hi - lo)
    x, y, z = xy[:, 0].copy(), xy[:, 1].copy(), rng.random(n) * 8.0
    x[:2], y[:2], z[:2] = (0.0, 64.0), (0.0, 64.0), (0.0, 8.0)  # the planted corners: the bounding box is theirs
    rgb = rng.integers(0, 256, (n, 3), dtype=np.uint8)
    bmin, bmax = np.array([0.0, 0.0, 0.0]), np.array([64.0, 64.0, 8.0])
    tree = ctx.build(0.001, pcv.Aabb(bmin, bmax), x, y, z, rgb, max_points_per_node=2000)
    # occupancy on the CPU: level-2 cells that hold a point strictly inside (the corners sit on cell borders)
    inner = (x > 0) & (x < 64)
    occupied = {cell_name(int(cx), int(cy), 2) for cx, cy in zip(x[inner] // 16, y[inner] // 16)}
    return dict(tree=tree, occupied=occupied, points=(x, y, z, rgb, bmin, bmax))


@pytest.fixture(scope="module")
def cloud(ctx):  # noqa: F811
    return make_cloud(ctx)


def build(cloud, strategy, background, root="r", tile=W, px=PX):
    return cloud["tree"].xray_quadtree(tile, px, strategy, background=background, root_node_id=root)


def shards(cloud, level, strategy, background, tile=W, px=PX):
    return [build(cloud, strategy, background, cell_name(cx, cy, level), tile, px) for cx in range(2 ** level) for cy in range(2 ** level)]


def images_by_name(xt):
    return dict(zip(xt.node_ids, xt.node_images()))


def assert_same_quadtree(got, whole):
    gi, wi = images_by_name(got), images_by_name(whole)
    assert set(gi) == set(wi) and len(got.node_ids) == len(gi), set(gi) ^ set(wi)
    for name, img in wi.items():
        assert np.array_equal(gi[name], img), (name, int((gi[name] != img).any(-1).sum()))
    assert struct.pack("<3d", *got.bounding_rect) == struct.pack("<3d", *whole.bounding_rect)
    assert got.deepest_level == whole.deepest_level and sorted(got.leaf_ids) == sorted(whole.created_ids)


@pytest.fixture(scope="module")
def whole(cloud):
    return {bg: build(cloud, s, bg) for s, bg in (("xray", "white"), ("colored", "transparent"))}


@pytest.mark.parametrize("level", [1, 2])
@pytest.mark.parametrize("strategy,background", [("xray", "white"), ("colored", "transparent")])
def test_merged_equals_whole(ctx, cloud, whole, strategy, background, level):  # noqa: F811
    w = whole[background]
    assert w.bounding_rect == (0.0, 0.0, 64.0) and w.deepest_level == 3
    parts = shards(cloud, level, strategy, background)
    merged = ctx.xray_merge(parts, background)
    assert_same_quadtree(merged, w)
    # pcv_xray_nodes: every part's nodes in part order, then the new levels in ascending index
    own = [n for p in parts for n in p.node_ids]
    upper = [X.node_name(lv, i) for lv, idx in P.parent_levels([X.node_id(p.node_ids[-1])[1] for p in parts if p.node_ids], level, 0)
             for i in idx]
    assert merged.node_ids == own + upper and merged.node_ids[-1] == "r"
    if level == 2:
        # the whole build itself, against the occupancy counted on the CPU: empty shards, a level-1 parent with a missing child
        empty = [cell_name(cx, cy, 2) for cx in range(4) for cy in range(4) if cell_name(cx, cy, 2) not in cloud["occupied"]]
        assert "r03" in empty and "r0" in w.node_ids and len(empty) >= 8
        assert all(e not in w.node_ids for e in empty)
        names = [cell_name(cx, cy, 2) for cx in range(4) for cy in range(4)]
        assert [n for n, p in zip(names, parts) if not p.node_ids] == empty
        nchildren = {n: sum(c in w.node_ids for c in (n + "0", n + "1", n + "2", n + "3")) for n in w.node_ids if len(n) == 2}
        assert 0 < min(nchildren.values()) < 4


def test_tile_size_7(ctx, cloud):  # noqa: F811
    w = build(cloud, "xray", "white", tile=7, px=1.0)
    assert w.deepest_level == 4 and w.bounding_rect == (0.0, 0.0, 112.0)
    merged = ctx.xray_merge(shards(cloud, 2, "xray", "white", tile=7, px=1.0), "white")
    assert_same_quadtree(merged, w)


def write_parts(parts, base):
    dirs = []
    os.makedirs(base, exist_ok=True)
    for k, p in enumerate(parts):
        p.write(base / f"part{k}")
        dirs.append(base / f"part{k}")
    return dirs


def test_through_directories(ctx, cloud, whole, tmp_path):  # noqa: F811
    w = whole["white"]
    dirs = write_parts(shards(cloud, 1, "xray", "white"), tmp_path)
    # one shard as another encoder would have written it: zlib level 9, Paeth rows, split IDAT
    for f in sorted(os.listdir(dirs[0])):
        if f.endswith(".png"):
            img = P.read_png((dirs[0] / f).read_bytes())
            (dirs[0] / f).write_bytes(MO.make_png(img, 9, filters=(4,), idat_pieces=3, ancillary=True))
    opened = [x for d in dirs for x in ctx.xray_open(d)]
    assert len(opened) == 4 and all(o.tile_size_px == W for o in opened)
    merged = ctx.xray_merge(opened, "white")
    assert_same_quadtree(merged, w)
    dev = merged.node_images(device=True)  # opened nodes decode into device memory too
    assert np.array_equal(dev.cpu().numpy(), merged.node_images())
    out = tmp_path / "out"
    merged.write(out)
    assert set(os.listdir(out)) == {n + ".png" for n in w.node_ids} | {"meta.pb"}
    for d in dirs:  # part nodes: byte copies of the sources
        for f in os.listdir(d):
            if f.endswith(".png"):
                assert (out / f).read_bytes() == (d / f).read_bytes(), f
    meta = P.decode_meta((out / "meta.pb").read_bytes())
    assert sorted(meta["nodes"]) == sorted(X.node_id(n) for n in w.node_ids) and len(meta["nodes"]) == len(w.node_ids)
    assert meta["rect"] == w.bounding_rect and meta["deepest_level"] == 3 and meta["tile_size"] == W and meta["version"] == 3
    assert np.array_equal(P.read_png((out / "r.png").read_bytes()), images_by_name(w)["r"])
    (back,) = ctx.xray_open(out)
    assert_same_quadtree(back, w)
    with pytest.raises(pcv.PcvError, match="PCV_E_INVALID"):
        back.write(tmp_path / "again")


def test_mixed_parts_and_in_place(ctx, cloud, whole, tmp_path):  # noqa: F811
    w = whole["transparent"]
    parts = shards(cloud, 1, "colored", "transparent")
    dirs = write_parts(parts[:2], tmp_path)
    mixed = [parts[3], ctx.xray_open(dirs[1])[0], parts[2], ctx.xray_open(dirs[0])[0]]
    assert_same_quadtree(ctx.xray_merge(mixed, "transparent"), w)
    # in place: the output is the first input
    dirs = write_parts(parts, tmp_path / "inplace")
    before = {f: (dirs[0] / f).read_bytes() for f in os.listdir(dirs[0])}
    merged = pcv.merge_xray_quadtrees(ctx, dirs, dirs[0], "transparent")
    assert_same_quadtree(merged, w)
    assert set(os.listdir(dirs[0])) == {n + ".png" for n in w.node_ids} | {"meta.pb", P.meta_file_name(parts[0].node_ids[-1])}
    assert all((dirs[0] / f).read_bytes() == b for f, b in before.items())
    metas = ctx.xray_open(dirs[0])  # meta.pb sorts before meta0.pb
    assert_same_quadtree(metas[0], w)


def test_root_level_zero_and_errors(ctx, cloud, whole):  # noqa: F811
    w = whole["white"]
    merged = ctx.xray_merge([w], "transparent")  # L == 0: nothing is built
    assert merged.node_ids == w.node_ids and np.array_equal(merged.node_images(), w.node_images())
    part = build(cloud, "xray", "white", "r0")
    with pytest.raises(pcv.PcvError, match="Not all roots have the same level"):
        ctx.xray_merge([w, part], "white")
    with pytest.raises(pcv.PcvError, match="No subquadtrees meta files found"):
        ctx.xray_merge([], "white")
    leaves_only = cloud["tree"].xray_tiles(W, PX, "xray", root_node_id="r0")
    with pytest.raises(pcv.PcvError, match="parent levels"):
        ctx.xray_merge([leaves_only], "white")
    for call in (merged.images, merged.build_parents):
        with pytest.raises(pcv.PcvError, match="PCV_E_INVALID"):
            call()
    # a part freed before the merged quadtree: an error, not a stale read
    m = ctx.xray_merge([part], "white")
    assert m.node_ids[-1] == "r" and m.node_images().shape[0] == len(part.node_ids) + 1
    part.free()
    with pytest.raises(pcv.PcvError, match="PCV_E_INVALID.*freed"):
        m.node_images()
    assert m.node_ids[-1] == "r"


def test_another_background_only_fills_missing_children(ctx, cloud, whole):  # noqa: F811
    w = whole["white"]
    parts = shards(cloud, 2, "xray", "white")
    merged = ctx.xray_merge(parts, "transparent")
    gi, wi = images_by_name(merged), images_by_name(w)
    roots = {X.node_id(p.node_ids[-1])[1]: p.node_images(len(p.node_ids) - 1, 1)[0] for p in parts if p.node_ids}
    want, nchildren = P.pyramid(roots, 2, 0, W, "transparent")
    for name, img in gi.items():
        if len(name) > 2:
            assert np.array_equal(img, wi[name]), name  # the parts' own images are never re-backgrounded
        else:
            assert np.array_equal(img, want[X.node_id(name)]), name
    changed = [n for n in ("r", "r0", "r1", "r2", "r3") if n in gi and not np.array_equal(gi[n], wi[n])]
    assert changed and min(nchildren.values()) < 4
    full = [X.node_name(*k) for k, c in nchildren.items() if c == 4 and k[0] == 1]
    assert all(np.array_equal(gi[n], wi[n]) for n in full)  # a parent whose four children exist does not see the background


def test_c_example_matches_the_python_helper(ctx, cloud, tmp_path):  # noqa: F811
    dirs = write_parts(shards(cloud, 1, "xray", "white"), tmp_path)
    pcv.merge_xray_quadtrees(ctx, dirs, tmp_path / "py", "transparent")
    exe = os.path.join(ROOT, "examples", "bin", "merge_xray_quadtrees")
    subprocess.check_call([exe, "--output-directory", str(tmp_path / "c"), "--tile-background-color", "transparent"] + [str(d) for d in dirs])
    files = sorted(os.listdir(tmp_path / "py"))
    assert files == sorted(os.listdir(tmp_path / "c")) and "meta.pb" in files and "r.png" in files
    for f in files:
        assert (tmp_path / "py" / f).read_bytes() == (tmp_path / "c" / f).read_bytes(), f
