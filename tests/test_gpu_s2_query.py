"""S2 cell clouds on the device, the region side (pcv_s2_query.hip): the cell lists of S2Cloud.cells_in_location
against the host twin pcv_s2_cells_in_location_host, bit for bit and list for list. The host twin is held against the
independent truth on the CPU (test_s2_query_cpu.py); here the device has to reproduce it: every location kind mixed in one
call, 1 / 65 / 130 locations (one wave each: the grid's edges), clouds of 1, 63, 64, 65 and several hundred cells (the 64-cell
steps of a wave's walk), a frustum with a singular matrix, and a capacity below the list lengths."""


import numpy as np
import pytest

import point_cloud_viewer_amd as pcv

import s2_region_truth as R
import s2_truth as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = pcv.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def prepared(ctx):
    """The scene's shapes, prepared once: (specs, Shapes, kinds, valid, corners as the device computed them)."""
    specs = R.scene()[6]
    shapes = ctx.shapes(list(specs))
    got = [shapes.get(i) for i in range(shapes.count)]
    return specs, shapes, shapes.kinds, [int(g[2]) for g in got], np.array([g[0] for g in got])


def _split(ctx, level, cells=None):
    """The scene's cloud split at `level`; with `cells`, only the points of its first `cells` cells."""
    x, y, z, rgb = R.scene()[:4]
    if cells is not None:
        ids = T.parents(T.set_leaf_ids("uniform"), level)
        keep = np.isin(ids, np.unique(ids)[:cells])
        x, y, z, rgb = x[keep], y[keep], z[keep], rgb[keep]
    return ctx.s2_split(dict(x=np.ascontiguousarray(x), y=np.ascontiguousarray(y), z=np.ascontiguousarray(z), color=np.ascontiguousarray(rgb)), level)


def _same_lists(got, want):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == np.uint32 and np.array_equal(g, w), (k, g[:8], w[:8])


def test_the_scene_is_the_uniform_cloud():
    x, y, z = R.scene()[:3]
    ux, uy, uz, _ = T.uniform_cloud()
    assert np.array_equal(x, ux) and np.array_equal(y, uy) and np.array_equal(z, uz)


@pytest.mark.parametrize("cells", [1, 63, 64, 65, None])
def test_lists_equal_the_host_twin(ctx, prepared, cells):
    specs, shapes, kinds, valid, corners = prepared
    assert {s[0] for s in specs} == {"all", "aabb", "obb", "frustum2", "frustum", "web_mercator_rect"}
    assert [v for s, v in zip(specs, valid) if s[0] == "frustum"] == [0]  # the singular matrix
    cloud = _split(ctx, 20, cells)
    ids = cloud.cells[0]
    assert ids.size == (cells if cells is not None else 675)
    unions = R.scene_unions(20)
    got = cloud.cells_in_location_indices(shapes, unions)
    want = pcv.s2_cells_in_location(ids, kinds, valid, corners, unions)
    _same_lists(got, want)
    assert [len(g) for g, s in zip(got, specs) if s[0] == "all"] == [ids.size]
    assert [len(g) for g, s in zip(got, specs) if s[0] == "frustum"] == [0]
    if cells is None:
        assert sum(len(g) > 0 for g in got) > 30 and len(got[len(specs)]) >= 1  # [cell, cell.next()] at the centre
    by_id = cloud.cells_in_location(shapes, unions)
    assert all(np.array_equal(a, ids[b]) for a, b in zip(by_id, got))
    # the second call reads the cached cell table; shapes alone and unions alone give the same lists
    _same_lists(cloud.cells_in_location_indices(shapes), want[:len(specs)])
    _same_lists(cloud.cells_in_location_indices(None, unions), want[len(specs):])
    assert cloud.cells_in_location_indices() == []
    cloud.free()


@pytest.mark.parametrize("count", [1, 65, 130])
def test_location_counts_at_the_wave_edges(ctx, count):
    specs = R.scene()[6]
    picked = [specs[(7 * k + 3) % len(specs)] for k in range(count)]
    shapes = ctx.shapes(picked)
    got_shapes = [shapes.get(i) for i in range(count)]
    cloud = _split(ctx, 20)
    got = cloud.cells_in_location_indices(shapes, [])
    want = pcv.s2_cells_in_location(cloud.cells[0], shapes.kinds, [int(g[2]) for g in got_shapes], np.array([g[0] for g in got_shapes]))
    _same_lists(got, want)
    assert len(got) == count and any(len(g) for g in got)
    cloud.free()
    shapes.free()


def test_finer_and_coarser_clouds(ctx, prepared):
    specs, shapes, kinds, valid, corners = prepared
    for level in (16, 24):
        cloud = _split(ctx, level)
        unions = R.scene_unions(level)
        _same_lists(cloud.cells_in_location_indices(shapes, unions), pcv.s2_cells_in_location(cloud.cells[0], kinds, valid, corners, unions))
        cloud.free()


def test_capacity_and_errors(ctx, prepared):
    specs, shapes, kinds, valid, corners = prepared
    cloud = _split(ctx, 20)
    ids = cloud.cells[0]
    want = pcv.s2_cells_in_location(ids, kinds, valid, corners)
    capacity = 7
    counts, out = np.zeros(len(specs), dtype=np.uint32), np.zeros((len(specs), capacity), dtype=np.uint32)
    ctx._check(ctx.lib.pcv_s2_cells_in_location(cloud.handle, shapes.handle, 0, None, None, capacity, counts.ctypes.data, out.ctypes.data))
    assert counts.tolist() == [len(w) for w in want] and max(counts) > capacity
    for k, w in enumerate(want):
        assert np.array_equal(out[k, :min(len(w), capacity)], w[:capacity])
    with pytest.raises(pcv.PcvError) as e:
        cloud.cells_in_location(None, [[ids[3], ids[1]]])
    assert e.value.code == pcv.PCV_E_INVALID and "ascend" in str(e.value)
    coarse = _split(ctx, 0)  # one face cell: AllPoints and unions only
    assert [g.tolist() for g in coarse.cells_in_location_indices(ctx.shapes([("all",)]), [[int(ids[0])]])] == [[0], [0]]
    with pytest.raises(pcv.PcvError) as e:
        coarse.cells_in_location_indices(shapes)
    assert e.value.code == pcv.PCV_E_INVALID and "level 0" in str(e.value)
    coarse.free()
    cloud.free()


def test_round_trip_through_a_directory(ctx, prepared, tmp_path):
    specs, shapes, kinds, valid, corners = prepared
    x, y, z, rgb = R.scene()[:4]
    inten = (((np.arange(x.size, dtype=np.int64) * 2654435761) % 100003).astype(np.float32) * 0.25 - 7.0)
    cloud = ctx.s2_split(dict(x=x, y=y, z=z, color=rgb, intensity=inten), 20)
    cloud.write(tmp_path)
    opened = ctx.s2_open(tmp_path)
    assert (opened.num_cells, opened.num_points, opened.has_intensity, opened.split_level) == (cloud.num_cells, cloud.num_points, True, 20)
    assert np.array_equal(opened.bbox_min, cloud.bbox_min) and np.array_equal(opened.bbox_max, cloud.bbox_max)
    assert all(np.array_equal(a, b) for a, b in zip(opened.cells, cloud.cells))
    unions = R.scene_unions(20)
    _same_lists(opened.cells_in_location_indices(shapes, unions), cloud.cells_in_location_indices(shapes, unions))  # before any file is read
    for first, count in ((0, None), (3, 2), (cloud.num_cells - 1, 1)):
        got, want = opened.cell_points(first, count), cloud.cell_points(first, count)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want))
    again = tmp_path / "again"
    opened.write(again)
    names = sorted(p.name for p in tmp_path.iterdir() if p.is_file())
    assert names == sorted(p.name for p in again.iterdir()) and len(names) == 3 * cloud.num_cells + 1
    assert all((again / n).read_bytes() == (tmp_path / n).read_bytes() for n in names)
    host = pcv.s2_open_host(tmp_path)  # the same directory without a device
    assert all(a.tobytes() == b.tobytes() for a, b in zip(host.cell_points(), cloud.cell_points()))
    with pytest.raises(pcv.PcvError):
        opened.order
    for c in (host, opened, cloud):
        c.free()


# ---- the batched point query over an S2 cloud (pcv_s2_points.hip) ----------------------------------------------------------
def _intensity(n):
    return (((np.arange(n, dtype=np.int64) * 2654435761) % 100003).astype(np.float32) * 0.25 - 7.0)


def _index_of(rgb):
    rgb = np.asarray(rgb).reshape(-1, 3).astype(np.int64)
    return (rgb[:, 0] << 16) | (rgb[:, 1] << 8) | rgb[:, 2]


@pytest.fixture(scope="module")
def queried(ctx, prepared):
    """The scene's cloud with intensity, split at level 20, its file contents, and the host keep flags of every location (the
    scene's shapes, then its unions) over those contents — computed once, read-only."""
    specs, shapes = prepared[0], prepared[1]
    x, y, z, rgb = R.scene()[:4]
    cloud = ctx.s2_split(dict(x=x, y=y, z=z, color=rgb, intensity=_intensity(x.size)), 20)
    xyz, c, inten = cloud.cell_points()
    px, py, pz = (np.ascontiguousarray(xyz[:, k]) for k in range(3))
    unions = R.scene_unions(20)
    keep = []
    for l, spec in enumerate(specs):
        if spec[0] == "all":
            keep.append(np.ones(x.size, dtype=bool))
        elif spec[0] == "web_mercator_rect":
            keep.append(pcv.wmr_contains(spec, px, py, pz).astype(bool))
        elif spec[0] == "frustum":  # the singular matrix: no cells, so no flag is ever asked for
            keep.append(np.zeros(x.size, dtype=bool))
        else:
            keep.append(np.asarray(ctx.cull_points(shapes, l, px, py, pz)[0]).astype(bool))
    for cells in unions:
        keep.append(pcv.s2_union_contains(cells, px, py, pz).astype(bool))
    for k in keep:
        k.setflags(write=False)
    yield cloud, xyz, c, inten, unions, keep
    cloud.free()


def _expected(cloud, lists, keep, intervals, inten):
    """Per location: (kept slot indices in segment order, kept count per segment)."""
    _, counts, offsets = cloud.cells
    out = []
    for l, cells in enumerate(lists):
        ok = keep[l]
        if intervals is not None and intervals[l] is not None:
            ok = ok & (inten.astype(np.float64) >= intervals[l][0]) & (inten.astype(np.float64) <= intervals[l][1])
        slots, sizes = [], []
        for cidx in cells:
            at = np.arange(int(offsets[cidx]), int(offsets[cidx] + counts[cidx]))
            hit = at[ok[at]]
            slots.append(hit)
            sizes.append(hit.size)
        out.append((np.concatenate(slots) if slots else np.zeros(0, dtype=np.int64), sizes))
    return out


@pytest.mark.parametrize("with_intervals", [False, True])
def test_segments_equal_the_filtered_cell_files(ctx, prepared, queried, with_intervals):
    specs, shapes = prepared[0], prepared[1]
    cloud, xyz, rgb, inten, unions, keep = queried
    locations = len(specs) + len(unions)
    intervals = [(-3.0, 900.0) if l % 3 == 0 else ((1e9, 2e9) if l % 7 == 1 else None) for l in range(locations)] if with_intervals else None
    lists = cloud.cells_in_location_indices(shapes, unions)
    batch = cloud.query_batch(shapes, unions, intervals)
    first, cell, off = batch.segments()
    assert first.tolist() == np.concatenate([[0], np.cumsum([len(v) for v in lists])]).tolist()
    assert np.array_equal(cell, np.concatenate(lists)) and batch.num_segments == len(cell)
    want = _expected(cloud, lists, keep, intervals, inten)
    sizes = np.concatenate([np.asarray(w[1], dtype=np.uint64) for w in want])
    assert np.array_equal(off, np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64))  # the u64 scan
    assert batch.num_points == int(sizes.sum()) and np.any(sizes == 0) and np.any(sizes > 0)  # empty segments are present
    for l, (slots, _) in enumerate(want):
        got = batch.shape_points(l)
        assert got["count"] == slots.size
        assert np.stack([got["x"], got["y"], got["z"]], axis=1).tobytes() == xyz[slots].tobytes(), l  # the stored f64, untouched
        assert got["rgb"].tobytes() == rgb[slots].tobytes() and got["intensity"].tobytes() == inten[slots].tobytes(), l
    # single segments: an empty one, a full one, the last
    for k in (int(np.flatnonzero(sizes == 0)[0]), int(np.argmax(sizes)), len(sizes) - 1):
        got = batch.points(k, 1)
        l = int(np.searchsorted(first, k, side="right") - 1)
        lo = int(off[k] - off[first[l]])
        assert got["count"] == int(sizes[k]) and np.array_equal(got["x"], xyz[want[l][0][lo:lo + int(sizes[k])], 0])
    batch.free()


def test_ranges_into_device_buffers_and_past_the_end(ctx, prepared, queried):
    import torch
    specs, shapes = prepared[0], prepared[1]
    cloud, xyz, rgb, inten, unions, keep = queried
    batch = cloud.query_batch(shapes, unions)
    first, cell, off = batch.segments()
    a, n = int(first[3]), int(first[9] - first[3])  # the segments of locations 3 .. 8
    host = batch.points(a, n)
    count = host["count"]
    assert count > 0
    out = dict(x=torch.full((count + 5,), -1.0, dtype=torch.float64, device="cuda"), y=torch.zeros(count + 5, dtype=torch.float64, device="cuda"),
               z=torch.zeros(count + 5, dtype=torch.float64, device="cuda"), rgb=torch.zeros((count + 5, 3), dtype=torch.uint8, device="cuda"),
               intensity=torch.zeros(count + 5, dtype=torch.float32, device="cuda"))
    dev = batch.points(a, n, out=out)
    for key in ("x", "y", "z", "rgb", "intensity"):
        assert np.array_equal(dev[key].cpu().numpy(), host[key]), key
    assert bool((out["x"][count:] == -1.0).all())
    # a range past the end: PCV_E_INVALID, nothing written
    x = np.full(4, 7.0)
    rc = ctx.lib.pcv_s2_query_points(batch.handle, batch.num_segments - 1, 2, 1 << 40, 0, x.ctypes.data, None, None, None, None)
    assert rc == pcv.PCV_E_INVALID and np.all(x == 7.0)
    with pytest.raises(pcv.PcvError):
        batch.points(batch.num_segments, 1)
    rc = ctx.lib.pcv_s2_query_points(batch.handle, a, n, count - 1, 0, x.ctypes.data, None, None, None, None)  # capacity too small
    assert rc == pcv.PCV_E_INVALID and np.all(x == 7.0)
    batch.free()
    plain = ctx.s2_split(dict(x=R.scene()[0], y=R.scene()[1], z=R.scene()[2], color=R.scene()[3]), 20)
    with pytest.raises(pcv.PcvError) as e:
        plain.query_batch(shapes, None, [(0.0, 1.0)] * shapes.count)
    assert e.value.code == pcv.PCV_E_INVALID and "intensity" in str(e.value)
    assert plain.query_batch().num_segments == 0
    plain.free()


def test_batch_of_a_reopened_directory(ctx, prepared, queried, tmp_path):
    specs, shapes = prepared[0], prepared[1]
    cloud, xyz, rgb, inten, unions, keep = queried
    cloud.write(tmp_path)
    opened = ctx.s2_open(tmp_path)
    intervals = [(-3.0, 900.0) if l % 2 else None for l in range(len(specs) + len(unions))]
    a, b = cloud.query_batch(shapes, unions, intervals), opened.query_batch(shapes, unions, intervals)  # reads the files on first use
    assert all(np.array_equal(u, v) for u, v in zip(a.segments(), b.segments())) and a.num_points == b.num_points > 0
    pa, pb = a.points(), b.points()
    assert all(pa[k].tobytes() == pb[k].tobytes() for k in ("x", "y", "z", "rgb", "intensity"))
    for o in (a, b, opened):
        o.free()


def _quat_of(m):
    """Unit quaternion (i, j, k, w) of a rotation matrix (Shepperd's method)."""
    t = np.trace(m)
    if t > 0:
        s = np.sqrt(t + 1.0) * 2
        q = [(m[2, 1] - m[1, 2]) / s, (m[0, 2] - m[2, 0]) / s, (m[1, 0] - m[0, 1]) / s, 0.25 * s]
    else:
        i = int(np.argmax(np.diag(m)))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = np.sqrt(1.0 + m[i, i] - m[j, j] - m[k, k]) * 2
        q = [0.0, 0.0, 0.0, (m[k, j] - m[j, k]) / s]
        q[i], q[j], q[k] = 0.25 * s, (m[j, i] + m[i, j]) / s, (m[k, i] + m[i, k]) / s
    return list(np.asarray(q) / np.linalg.norm(q))


def test_the_reference_integration_test_restated(ctx):
    """point_cloud_test/tests/main.rs:85-99, :162-203: the same query over the octree and over the S2 cloud of one data set
    returns the same indexed points — the index sets differ in at most ceil(min(len) / 100) indices and matching indices lie
    within 2 * sqrt(3) * resolution (both numbers are the reference's). Where the truth's cell list covers every cell that
    holds a passing point, the S2 result is the brute-force filter of the input, exactly."""
    import math
    import oracle_lib as O
    from point_cloud_viewer_amd import synthetic
    x, y, z, rgb, bmin, bmax = R.scene()[:6]
    rot, centre = synthetic.ecef_from_local(37.407204, -122.147604)
    quat = _quat_of(rot)
    assert np.allclose(R.quat_rotate(quat, [1.0, 2.0, 3.0]), rot @ np.array([1.0, 2.0, 3.0]), atol=1e-12)
    diag = bmax - bmin
    wmr = [s for s in R.scene()[6] if s[0] == "web_mercator_rect"][0]  # queries.rs:59-68
    specs = [("all",), ("aabb", bmin + 0.2 * diag, bmin + 0.8 * diag), ("obb", centre, quat, [50.0, 50.0, 5.0]),
             ("frustum2", *O.frustum_new(list(centre), quat, O.perspective3_new(1.0, 1.2, 0.1, 10.0))), wmr]
    shapes = ctx.shapes(specs)
    resolution = 0.001
    tree = ctx.build(resolution, pcv.Aabb(bmin, bmax), x, y, z, rgb)
    cloud = ctx.s2_split(dict(x=x, y=y, z=z, color=rgb), 20)
    ids, counts, offsets = cloud.cells
    cell_of_point = np.searchsorted(ids, T.parents(T.set_leaf_ids("uniform"), 20))
    octree, s2 = tree.query_batch(shapes), cloud.query_batch(shapes)
    bounds = R.cell_bounds(ids)
    for l, spec in enumerate(specs):
        a, b = octree.shape_points(l), s2.shape_points(l)
        ia, ib = _index_of(a["rgb"]), _index_of(b["rgb"])
        assert len(set(ia.tolist())) == ia.size and len(set(ib.tolist())) == ib.size and ib.size > 0, spec[0]
        allowed = math.ceil(min(ia.size, ib.size) / 100)
        assert len(set(ia.tolist()) ^ set(ib.tolist())) <= allowed, (spec[0], ia.size, ib.size)
        common, at_a, at_b = np.intersect1d(ia, ib, return_indices=True)
        d = np.sqrt((a["x"][at_a] - b["x"][at_b]) ** 2 + (a["y"][at_a] - b["y"][at_b]) ** 2 + (a["z"][at_a] - b["z"][at_b]) ** 2)
        assert d.max() <= 2.0 * math.sqrt(3.0) * resolution, (spec[0], d.max())
        # the S2 side returns the stored f64: exactly the input's
        assert np.array_equal(b["x"], x[ib]) and np.array_equal(b["y"], y[ib]) and np.array_equal(b["z"], z[ib])
        if spec[0] == "all":
            passing = np.arange(x.size)
        elif spec[0] == "web_mercator_rect":
            passing = np.flatnonzero(pcv.wmr_contains(spec, x, y, z))
        else:
            passing = np.flatnonzero(np.asarray(ctx.cull_points(shapes, l, x, y, z)[0]))
        if spec[0] != "all":
            yes, _, _ = R.decided_lists(ids, R.corners_rect(shapes.get(l)[0]), bounds=bounds)
            assert set(np.unique(cell_of_point[passing]).tolist()) <= set(yes), spec[0]  # the precondition, on the truth
        assert sorted(ib.tolist()) == passing.tolist(), spec[0]
    for o in (octree, s2, cloud, tree, shapes):
        o.free()


def test_a_batch_that_outlives_its_cloud_goes_with_it(ctx):
    """pcv_s2_query_free reads the batch's cloud. A cloud freed before its batches — by hand, or by a garbage collection that
    finalizes a cloud and its batch in the order it likes (an exception's traceback holds both) — releases them itself; the
    batch is dead from then on, freeing it again does nothing, and the pool gets every byte back."""
    shapes = ctx.shapes([("all",)])
    live = ctx.pool_stats()[0]
    cloud = _split(ctx, 20)
    a, b = cloud.query_batch(shapes), cloud.query_batch(shapes)
    assert a.num_points == b.num_points == cloud.num_points > 0
    a.free()
    cloud.free()
    with pytest.raises(pcv.PcvError):
        b.points()
    b.free()
    b.free()
    assert ctx.pool_stats()[0] == live
    cloud = _split(ctx, 20)
    b = cloud.query_batch(shapes)
    cloud.__del__()  # the collector's other order
    b.__del__()
    assert ctx.pool_stats()[0] == live and b.handle is None and cloud.handle is None
    shapes.free()
