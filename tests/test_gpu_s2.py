"""S2 cell clouds on the device (pcv_s2.hip): cell ids against the host twin bit for bit, the split against s2_truth.py (the
independent restatement of DESIGN §9c), the written directory, invalid points, and cell-union containment — alone and against
the octree of the same cloud, as the reference's check_cell_union_query_equality (point_cloud_test) does."""
import math
import os

import numpy as np
import pytest

import point_cloud_viewer_amd as pcv
from point_cloud_viewer_amd import synthetic

import s2_truth as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = pcv.Context(0)
    yield c
    c.close()


def intensity_of(n):
    return (((np.arange(n, dtype=np.int64) * 2654435761) % 100003).astype(np.float32) * 0.25 - 7.0)


def index_of(rgb):
    rgb = np.asarray(rgb).reshape(-1, 3).astype(np.int64)
    return (rgb[:, 0] << 16) | (rgb[:, 1] << 8) | rgb[:, 2]


def check_split(cloud, x, y, z, rgb, inten, level, truth_leaves):
    """Every property of a split against the truth's leaf ids of the same points."""
    want_ids, want_counts = np.unique(T.parents(truth_leaves, level), return_counts=True)
    want_order = np.argsort(T.parents(truth_leaves, level), kind="stable")
    ids, counts, offsets = cloud.cells
    assert cloud.num_points == x.size and cloud.split_level == level
    assert np.all(ids[1:] > ids[:-1]) and np.array_equal(ids, want_ids)
    assert np.array_equal(counts, want_counts.astype(np.uint64))
    assert np.array_equal(offsets, np.concatenate([[0], np.cumsum(want_counts)[:-1]]).astype(np.uint64))
    order = cloud.order
    assert np.array_equal(order, want_order.astype(np.uint32))
    xyz, c, i = cloud.cell_points()
    assert xyz.tobytes() == np.stack([x, y, z], axis=1)[want_order].tobytes()
    assert c.tobytes() == np.ascontiguousarray(rgb[:, :3])[want_order].tobytes()
    if inten is None:
        assert i is None and not cloud.has_intensity
    else:
        assert i.tobytes() == inten[want_order].tobytes()
    assert np.array_equal(cloud.bbox_min, [x.min(), y.min(), z.min()]) and np.array_equal(cloud.bbox_max, [x.max(), y.max(), z.max()])
    return want_ids, want_counts, want_order


# ---- ids ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(T.POINT_SETS))
def test_ids_equal_the_host_twin(ctx, name):
    x, y, z = T.POINT_SETS[name]()[:3]
    for level in (0, 13, 20, 30):
        got = ctx.s2_cell_ids(x, y, z, level)
        want = pcv.s2_cell_ids(x, y, z, level)
        assert got.dtype == np.uint64 and np.array_equal(got, want), (level, int((got != want).sum()))
    assert np.array_equal(ctx.s2_cell_ids(x, y, z), T.set_leaf_ids(name))


def test_ids_of_device_tensors(ctx):
    import torch
    x, y, z = T.edge_points()
    dev = [torch.from_numpy(a).cuda() for a in (x, y, z)]
    torch.cuda.synchronize()
    got = ctx.s2_cell_ids(*dev, level=20)
    assert got.is_cuda and np.array_equal(got.cpu().numpy().view(np.uint64), pcv.s2_cell_ids(x, y, z, 20))
    with pytest.raises(pcv.PcvError) as e:
        ctx.s2_cell_ids(x, y, z, 31)
    assert e.value.code == pcv.PCV_E_INVALID


# ---- the split ----------------------------------------------------------------------------------------------------------
def test_split_against_the_truth(ctx):
    x, y, z, rgb = T.uniform_cloud()
    inten = intensity_of(x.size)
    cloud = ctx.s2_split(dict(x=x, y=y, z=z, color=rgb, intensity=inten))
    ids, counts, _ = check_split(cloud, x, y, z, rgb, inten, 20, T.set_leaf_ids("uniform"))
    assert (ids.size, int(counts.max()), int(counts.min())) == (675, 49, 1)
    assert cloud.tokens()[0].startswith("808e4d142b")
    # a range of cells in the middle, and the refusals
    ids, counts, offsets = cloud.cells
    xyz, c, i = cloud.cell_points(100, 7)
    lo, hi = int(offsets[100]), int(offsets[107])
    assert xyz.shape == (hi - lo, 3) and np.array_equal(index_of(c), cloud.order[lo:hi])
    with pytest.raises(ValueError):
        cloud.cell_points(670, 6)
    cloud.free()


def test_split_level_30_and_level_0(ctx):
    x, y, z = T.edge_points()
    x, y, z = x[::5].copy(), y[::5].copy(), z[::5].copy()
    # the edge set sits at a radius of 6.37e6: valid ECEF
    rgb = synthetic.index_colors(x.size)
    leaves = T.set_leaf_ids("edges")[::5]
    cloud = ctx.s2_split(dict(x=x, y=y, z=z, color=rgb), split_level=30)
    ids, _, _ = check_split(cloud, x, y, z, rgb, None, 30, leaves)
    assert ids.size == np.unique(leaves).size and ids.size < x.size  # duplicates of a leaf share its cell
    cloud.free()
    x, y, z = T.shell_points()
    rgb = synthetic.index_colors(x.size)
    cloud = ctx.s2_split(dict(x=x, y=y, z=z, color=rgb), split_level=0)
    ids, _, _ = check_split(cloud, x, y, z, rgb, None, 0, T.set_leaf_ids("shell"))
    assert [pcv.s2_cell_token(int(i)) for i in ids] == ["1", "3", "5", "7", "9", "b"] == cloud.tokens()
    cloud.free()


def test_split_one_cell_and_a_tile_seam(ctx):
    # 100 points inside one level-20 cell: a point of the config-1 cloud and its neighbours a tenth of a millimetre around
    x0, y0, z0, _ = T.uniform_cloud()
    rng = np.random.Generator(np.random.PCG64(3))
    d = rng.uniform(-1e-4, 1e-4, (100, 3))
    x, y, z = x0[0] + d[:, 0], y0[0] + d[:, 1], z0[0] + d[:, 2]
    leaves = T.leaf_ids(x, y, z)
    rgba = np.concatenate([synthetic.index_colors(100), np.full((100, 1), 255, np.uint8)], axis=1)  # stride 4
    cloud = ctx.s2_split(dict(x=x, y=y, z=z, color=rgba, intensity=intensity_of(100)))
    ids, counts, order = check_split(cloud, x, y, z, rgba, intensity_of(100), 20, leaves)
    assert ids.size == 1 and counts[0] == 100 and np.array_equal(order, np.arange(100))
    cloud.free()
    # 65 537 points: more than one workgroup of every kernel and more than one tile of the sorts; 16-bit cell ranks would wrap
    n = 65537
    x, y, z, rgb, _, _ = synthetic.uniform_ecef(n, seed=77, width=1500.0)
    leaves = T.leaf_ids(x, y, z)
    for level in (20, 24):
        cloud = ctx.s2_split(dict(x=x, y=y, z=z, color=rgb, intensity=intensity_of(n)), split_level=level)
        ids, _, _ = check_split(cloud, x, y, z, rgb, intensity_of(n), level, leaves)
        assert ids.size > (2048 if level == 20 else 40000)
        cloud.free()


def test_device_tensors_and_host_arrays_agree(ctx):
    import torch
    x, y, z, rgb = T.uniform_cloud()
    inten = intensity_of(x.size)
    host = ctx.s2_split(dict(x=x, y=y, z=z, color=rgb, intensity=inten))
    dev_in = dict(x=torch.from_numpy(x).cuda(), y=torch.from_numpy(y).cuda(), z=torch.from_numpy(z).cuda(),
                  color=torch.from_numpy(rgb).cuda(), intensity=torch.from_numpy(inten).cuda())
    torch.cuda.synchronize()
    dev = ctx.s2_split(dev_in)
    for a, b in zip(host.cells, dev.cells):
        assert np.array_equal(a, b)
    assert np.array_equal(host.order, dev.order)
    for a, b in zip(host.cell_points(), dev.cell_points()):
        assert a.tobytes() == b.tobytes()
    assert np.array_equal(host.bbox_min, dev.bbox_min) and np.array_equal(host.bbox_max, dev.bbox_max)
    host.free()
    dev.free()


# ---- the directory ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_intensity", [True, False])
def test_written_directory(ctx, tmp_path, with_intensity):
    x, y, z, rgb = T.uniform_cloud()
    inten = intensity_of(x.size) if with_intensity else None
    out = tmp_path / "s2"
    points = dict(x=x, y=y, z=z, color=rgb)
    if with_intensity:
        points["intensity"] = inten
    cloud = pcv.build_s2_cells(str(out), points, ctx=ctx)
    ids, counts, offsets = cloud.cells
    exts = (".xyz", ".rgb", ".intensity") if with_intensity else (".xyz", ".rgb")
    assert set(os.listdir(out)) == {T.token(int(i)) + e for i in ids for e in exts} | {"meta.pb"}
    xyz, c, i = cloud.cell_points()
    for k, cell in enumerate(ids.tolist()):
        lo, hi = int(offsets[k]), int(offsets[k] + counts[k])
        stem = out / T.token(cell)
        assert stem.with_suffix(".xyz").read_bytes() == xyz[lo:hi].tobytes()
        assert stem.with_suffix(".rgb").read_bytes() == c[lo:hi].tobytes()
        if with_intensity:
            assert stem.with_suffix(".intensity").read_bytes() == i[lo:hi].tobytes()
    meta = T.parse_s2_meta((out / "meta.pb").read_bytes())
    want_ids, want_counts = np.unique(T.parents(T.set_leaf_ids("uniform"), 20), return_counts=True)
    assert meta["version"] == 13 and meta["has_s2"]
    assert meta["bbox_min"] == [x.min(), y.min(), z.min()] and meta["bbox_max"] == [x.max(), y.max(), z.max()]
    assert meta["cells"] == list(zip(want_ids.tolist(), want_counts.tolist()))
    assert meta["attributes"] == [("color", T.U8VEC3)] + ([("intensity", T.F32)] if with_intensity else [])
    cloud.free()


# ---- invalid points -----------------------------------------------------------------------------------------------------
def at_radius(p, radius):
    p = np.asarray(p, dtype=np.float64)
    return p * (radius / math.sqrt(float(p[0] * p[0] + p[1] * p[1] + p[2] * p[2])))


@pytest.mark.parametrize("case", ["low", "high", "nan"])
def test_invalid_points(ctx, tmp_path, case):
    x, y, z, rgb = (a.copy() for a in T.uniform_cloud())
    first, later = 12345, 17000
    p = np.array([x[first], y[first], z[first]])
    bad = {"low": at_radius(p, 6352799.0), "high": at_radius(p, 6384401.0), "nan": np.array([p[0], float("nan"), p[2]])}[case]
    assert not T.valid_ecef(*bad.tolist()) and all(T.valid_ecef(*q) for q in zip(x[:first].tolist(), y[:first].tolist(), z[:first].tolist()))
    # the boundary itself is valid on both sides, as in s2.rs:65 (> and <, not >= and <=)
    assert T.valid_ecef(6384400.0, 0.0, 0.0) and T.valid_ecef(0.0, -6352800.0, 0.0)
    for at in (first, later):  # a second invalid point further on: the FIRST is reported
        x[at], y[at], z[at] = bad
    out = tmp_path / "s2"
    with pytest.raises(pcv.PcvError) as e:
        pcv.build_s2_cells(str(out), dict(x=x, y=y, z=z, color=rgb), ctx=ctx)
    assert e.value.code == pcv.PCV_E_INVALID
    assert f"index {first} " in str(e.value) and "not a valid ECEF point" in str(e.value), str(e.value)
    assert repr(float(bad[0])) in str(e.value) or f"{bad[0]:.17g}" in str(e.value)
    assert not out.exists()
    # the same cloud without them splits
    x0, y0, z0, _ = T.uniform_cloud()
    x[[first, later]], y[[first, later]], z[[first, later]] = x0[[first, later]], y0[[first, later]], z0[[first, later]]
    cloud = ctx.s2_split(dict(x=x, y=y, z=z, color=rgb))
    assert cloud.num_cells == 675
    cloud.free()


def test_boundary_radii_are_valid(ctx):
    x = np.array([6384400.0, 0.0, 6352800.0])
    y = np.array([0.0, -6352800.0, 0.0])
    z = np.zeros(3)
    cloud = ctx.s2_split(dict(x=x, y=y, z=z, color=synthetic.index_colors(3)), split_level=0)
    assert cloud.tokens() == ["1", "9"] and cloud.cells[1].tolist() == [2, 1] and cloud.order.tolist() == [0, 2, 1]
    cloud.free()


# ---- cell unions --------------------------------------------------------------------------------------------------------
def test_union_contains_equals_the_host_twin(ctx):
    import torch
    x, y, z = T.edge_points()
    leaves = T.set_leaf_ids("edges")
    rng = np.random.Generator(np.random.PCG64(6))
    picked = sorted({T.parent(int(leaf), int(rng.integers(14, 31))) for leaf in rng.choice(leaves, 60, replace=False)})
    cells = [c for k, c in enumerate(picked) if k == 0 or T.range_min(c) > T.range_max(picked[k - 1])]
    assert len({T.lsb_for_level(0) // (c & -c) for c in cells}) > 5  # mixed levels
    want = pcv.s2_union_contains(cells, x, y, z)
    got = ctx.s2_union_contains(cells, x, y, z)
    assert np.array_equal(got, want) and 0 < int(want.sum()) < want.size
    dev = [torch.from_numpy(a).cuda() for a in (x, y, z)]
    torch.cuda.synchronize()
    assert np.array_equal(ctx.s2_union_contains(cells, *dev).cpu().numpy(), want)
    assert not ctx.s2_union_contains([], x, y, z).any()
    with pytest.raises(pcv.PcvError) as e:
        ctx.s2_union_contains(cells[::-1], x, y, z)
    assert e.value.code == pcv.PCV_E_INVALID and "ascend" in str(e.value)


def test_cell_union_query_equals_the_octree(ctx):
    """point_cloud_test's check_cell_union_query_equality: the points a cell union selects from the S2 cell cloud, from the raw
    input and from the octree of the same cloud are the same points (told apart by their index colours). The octree's decoded
    positions lie within 2 sqrt(3) resolution of the input, so its side is compared on the points whose cube of that half-edge
    stays inside one level-20 cell (cells are convex: the cube's corners decide)."""
    resolution = 0.001
    x, y, z, rgb, bmin, bmax = synthetic.uniform_ecef(20000)
    cloud = ctx.s2_split(dict(x=x, y=y, z=z, color=rgb))
    ids, counts, offsets = cloud.cells
    top = np.sort(np.argsort(-counts.astype(np.int64), kind="stable")[:3])
    union = ids[top]
    from_split = set()
    for k in top.tolist():
        from_split |= set(index_of(cloud.cell_points(k, 1)[1]).tolist())
    assert len(from_split) == int(counts[top].sum())
    keep = ctx.s2_union_contains(union, x, y, z)
    from_input = set(np.nonzero(keep)[0].tolist())
    assert from_split == from_input
    assert from_split == {i for i, leaf in enumerate(T.set_leaf_ids("uniform").tolist()) if T.union_contains(union.tolist(), leaf)}

    tree = ctx.build(resolution, pcv.Aabb(bmin, bmax), x, y, z, rgb)
    everything = ctx.shapes([("aabb", bmin - 1.0, bmax + 1.0)])
    pts = tree.query_points(everything, 0)
    assert pts["count"] == x.size
    tree_index = index_of(pts["rgb"])
    assert np.array_equal(np.sort(tree_index), np.arange(x.size))
    tree_keep = ctx.s2_union_contains(union, pts["x"], pts["y"], pts["z"])
    r = 2.0 * math.sqrt(3.0) * resolution
    assert float(np.max(np.abs(np.stack([pts["x"] - x[tree_index], pts["y"] - y[tree_index], pts["z"] - z[tree_index]])))) <= r
    own = pcv.s2_cell_ids(x, y, z, 20)
    safe = np.ones(x.size, dtype=bool)
    for sx in (-r, r):
        for sy in (-r, r):
            for sz in (-r, r):
                safe &= pcv.s2_cell_ids(x + sx, y + sy, z + sz, 20) == own
    skipped = int((~safe).sum())
    # measured: 54 of 20 000 points (0.27 %) lie that close to a cell edge; the reference's test allows 1 %
    assert skipped < 0.01 * x.size, skipped
    from_tree = set(tree_index[tree_keep.astype(bool)].tolist())
    safe_set = set(np.nonzero(safe)[0].tolist())
    assert from_tree & safe_set == from_split & safe_set
    assert len(from_split & safe_set) > 100
    everything.free()
    tree.free()
    cloud.free()
