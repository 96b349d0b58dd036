"""S2 cell clouds from a stream of batches (pcv_s2_stream.hip): the in-memory stream against pcv_s2_split of the concatenated
batches and, independently, against s2_truth.py's leaf ids with a stable argsort; the directory stream, byte for byte, against
the directory of the one-shot build, for every batching and flush size; OpenMode::Append; the refusals; build_s2_cells over an
iterator of batches, and the read side over what it wrote."""
import itertools
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


def check_split(cloud, x, y, z, rgb, inten, level, truth_leaves):
    """Every property of a split against the truth's leaf ids of the same points (as in test_gpu_s2.py)."""
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


def same_cloud(got, want):
    """ids, counts, offsets, bbox, level, the three blobs and the order: equal."""
    assert (got.num_points, got.num_cells, got.split_level, got.has_intensity) == (want.num_points, want.num_cells, want.split_level,
                                                                                 want.has_intensity)
    for a, b in zip(got.cells, want.cells):
        assert np.array_equal(a, b)
    assert got.bbox_min.tobytes() == want.bbox_min.tobytes() and got.bbox_max.tobytes() == want.bbox_max.tobytes()
    for a, b in zip(got.cell_points(), want.cell_points()):
        assert (a is None and b is None) or a.tobytes() == b.tobytes()
    assert np.array_equal(got.order, want.order)


def slices(sizes, n):
    """[begin, end) of consecutive batches of the given sizes; None = the rest."""
    at, out = 0, []
    for s in sizes:
        s = n - at if s is None else s
        out.append((at, at + s))
        at += s
    assert at == n
    return out


def take(points, lo, hi):
    return {k: v[lo:hi] for k, v in points.items()}


def stream_of(ctx, points, cuts, level=20, **kw):
    stream = ctx.s2_stream(level, **kw)
    for lo, hi in cuts:
        stream.append(take(points, lo, hi))
    return stream


@pytest.fixture(scope="module")
def uniform(ctx):
    """The uniform cloud with intensity, its one-shot split (truth 1, checked here against truth 2) — shared, read-only."""
    x, y, z, rgb = T.uniform_cloud()
    points = dict(x=x, y=y, z=z, color=rgb, intensity=intensity_of(x.size))
    whole = ctx.s2_split(points)
    check_split(whole, x, y, z, rgb, points["intensity"], 20, T.set_leaf_ids("uniform"))
    yield points, whole
    whole.free()


@pytest.fixture(scope="module")
def whole_dir(ctx, uniform, tmp_path_factory):
    """The directory of the one-shot build of the uniform cloud."""
    out = tmp_path_factory.mktemp("s2_whole")
    pcv.build_s2_cells(str(out), uniform[0], ctx=ctx).free()
    return out


def same_directory(got, want):
    """The file set, then every file's bytes, meta.pb included."""
    assert sorted(os.listdir(got)) == sorted(os.listdir(want))
    for name in sorted(os.listdir(want)):
        assert (got / name).read_bytes() == (want / name).read_bytes(), name


def expected_flushes(sizes, flush_points):
    pending = flushes = 0
    for s in sizes:
        pending += s
        if s and pending >= flush_points:
            flushes, pending = flushes + 1, 0
    return flushes + (1 if pending else 0)


# ---- the in-memory stream -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes", [[1, 7, 0, 4999, 1024, None], "sevens", [None]], ids=["ragged", "sevens", "one"])
def test_in_memory_stream_equals_the_split(ctx, uniform, sizes):
    """ragged: batches of 1, 7, 0, 4 999, 1 024 and the rest. sevens: 2 858 parts, every output chunk a run of about two thousand
    1-point segments — past the 1 024 segment offsets staged in LDS, and source runs at every rgb byte alignment. one: the merge
    is the identity."""
    points, whole = uniform
    n = points["x"].size
    cuts = [(lo, min(lo + 7, n)) for lo in range(0, n, 7)] if sizes == "sevens" else slices(sizes, n)
    stream = stream_of(ctx, points, cuts)
    info = stream.info
    assert info == dict(batches=len(cuts), points=n, cells=whole.num_cells, pending_points=n, flushes=0)
    if sizes == "sevens":  # the plan of this stream really is what the docstring says
        first = T.parents(T.set_leaf_ids("uniform"), 20)
        plan = pcv.s2_merge_plan([np.unique(first[lo:hi], return_counts=True) for lo, hi in cuts])
        assert int(np.diff(plan["chunk_first_segment"].astype(np.int64)).max()) > 1024
    cloud = stream.finish()
    same_cloud(cloud, whole)
    check_split(cloud, points["x"], points["y"], points["z"], points["color"], points["intensity"], 20, T.set_leaf_ids("uniform"))
    cloud.free()


def test_one_cell_over_many_chunks(ctx):
    """A 5 000-point patch at level 0: one cell, three segments, the middle one across three output chunks."""
    x, y, z, rgb, _, _ = synthetic.uniform_ecef(5000, seed=4242, width=60.0)
    points = dict(x=x, y=y, z=z, color=rgb)
    whole = ctx.s2_split(points, split_level=0)
    stream = stream_of(ctx, points, slices([100, 4500, 400], 5000), level=0)
    cloud = stream.finish()
    assert cloud.num_cells == 1
    same_cloud(cloud, whole)
    check_split(cloud, x, y, z, rgb, None, 0, T.leaf_ids(x, y, z))
    whole.free()
    cloud.free()


def test_edge_points_at_level_30(ctx):
    x, y, z = (a[::5].copy() for a in T.edge_points())
    rgb = synthetic.index_colors(x.size)
    points = dict(x=x, y=y, z=z, color=rgb)
    whole = ctx.s2_split(points, split_level=30)
    cloud = stream_of(ctx, points, slices([3001, 17, 4096, None], x.size), level=30).finish()
    same_cloud(cloud, whole)
    check_split(cloud, x, y, z, rgb, None, 30, T.set_leaf_ids("edges")[::5])
    whole.free()
    cloud.free()


def test_device_and_host_batches_in_one_stream(ctx, uniform):
    import torch
    points, whole = uniform
    n, cut = points["x"].size, 8191
    rgba = np.concatenate([points["color"], np.full((n, 1), 255, np.uint8)], axis=1)  # stride 4, in the device batch
    dev = {k: torch.from_numpy(np.ascontiguousarray(v[:cut])).cuda() for k, v in dict(points, color=rgba).items()}
    torch.cuda.synchronize()
    stream = ctx.s2_stream()
    stream.append(dev)
    stream.append(take(points, cut, n))
    cloud = stream.finish()
    same_cloud(cloud, whole)
    cloud.free()
    # and a PointsBatch dict (position (n, 3)) on the host, stride 4 in the host batch this time
    stream = ctx.s2_stream()
    stream.append(dict(position=np.stack([points["x"], points["y"], points["z"]], axis=1)[:cut], color=rgba[:cut], intensity=points["intensity"][:cut]))
    stream.append(take(points, cut, n))
    cloud = stream.finish()
    same_cloud(cloud, whole)
    cloud.free()


def test_no_points_at_all(ctx):
    empty = dict(x=np.zeros(0), y=np.zeros(0), z=np.zeros(0), color=np.zeros((0, 3), np.uint8))
    want = ctx.s2_split(empty)
    stream = ctx.s2_stream()
    stream.append(empty)
    assert stream.info == dict(batches=1, points=0, cells=0, pending_points=0, flushes=0)
    got = stream.finish()
    same_cloud(got, want)
    got.free()
    want.free()


# ---- the directory stream -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flush_points", [1, 3000, 10 ** 9])
def test_directory_stream_equals_the_one_shot_directory(ctx, uniform, whole_dir, tmp_path, flush_points):
    points, whole = uniform
    n = points["x"].size
    sizes = [1, 7, 0, 4999, 1024, n - 6031]
    out = tmp_path / "streamed"
    stream = stream_of(ctx, points, slices(sizes, n), directory=out, flush_points=flush_points)
    info = stream.info
    assert (info["batches"], info["points"], info["cells"]) == (6, n, whole.num_cells)
    cloud = stream.finish()
    same_directory(out, whole_dir)
    assert (cloud.num_points, cloud.num_cells, cloud.split_level, cloud.has_intensity) == (n, whole.num_cells, 20, True)
    for a, b in zip(cloud.cell_points(), whole.cell_points()):
        assert a.tobytes() == b.tobytes()
    with pytest.raises(pcv.PcvError):  # no input order is kept in this mode
        cloud.order
    cloud.free()
    # the number of flushes, on a second stream that is looked at before it finishes (finish adds the last one)
    stream = stream_of(ctx, points, slices(sizes, n), directory=tmp_path / "again", flush_points=flush_points)
    want = expected_flushes(sizes, flush_points)
    assert want == {1: 5, 3000: 2, 10 ** 9: 1}[flush_points]
    info = stream.info
    assert info["flushes"] == want - (1 if info["pending_points"] else 0)
    assert info["pending_points"] == {1: 0, 3000: 0, 10 ** 9: n}[flush_points]
    stream.finish().free()
    same_directory(tmp_path / "again", whole_dir)


def test_stale_files_and_first_write_truncates(ctx, uniform, whole_dir, tmp_path):
    """A file of a cell the stream writes is truncated the first time, a file of a cell it never sees is left alone."""
    points, whole = uniform
    out = tmp_path / "reused"
    out.mkdir()
    token = whole.tokens()[3]
    (out / (token + ".xyz")).write_bytes(b"stale" * 100)
    (out / "0123.rgb").write_bytes(b"other")
    n = points["x"].size
    stream_of(ctx, points, slices([5000, 5000, None], n), directory=out, flush_points=4000).finish().free()
    assert (out / "0123.rgb").read_bytes() == b"other"
    (out / "0123.rgb").unlink()
    same_directory(out, whole_dir)


def test_append_mode(ctx, uniform, whole_dir, tmp_path):
    points, whole = uniform
    n, cut = points["x"].size, 9000
    out = tmp_path / "two_streams"
    first = stream_of(ctx, points, slices([4000, 5000], cut), directory=out, flush_points=4500).finish()
    assert first.num_points == cut
    first.free()
    second = ctx.s2_stream(directory=out, open_mode="append", flush_points=6000)
    assert second.info == dict(batches=0, points=cut, cells=first.num_cells, pending_points=0, flushes=0)
    for lo, hi in [(cut, cut + 3), (cut + 3, 16000), (16000, n)]:
        second.append(take(points, lo, hi))
    cloud = second.finish()
    assert cloud.num_points == n
    same_directory(out, whole_dir)
    cloud.free()
    # through build_s2_cells
    out2 = tmp_path / "two_builds"
    pcv.build_s2_cells(str(out2), take(points, 0, cut), ctx=ctx).free()
    pcv.build_s2_cells(str(out2), take(points, cut, n), ctx=ctx, open_mode="append").free()
    same_directory(out2, whole_dir)
    # onto a level-19 directory: refused, and nothing is touched
    out19 = tmp_path / "level19"
    pcv.build_s2_cells(str(out19), take(points, 0, cut), split_level=19, ctx=ctx).free()
    before = {name: (out19 / name).read_bytes() for name in os.listdir(out19)}
    with pytest.raises(pcv.PcvError) as e:
        ctx.s2_stream(20, out19, "append")
    assert e.value.code == pcv.PCV_E_INVALID and "split level 20" in str(e.value)
    assert {name: (out19 / name).read_bytes() for name in os.listdir(out19)} == before
    # intensity mismatch with the directory: the cloud there has intensity, the batch has none
    stream = ctx.s2_stream(20, out, "append")
    bare = {k: v for k, v in take(points, 0, 10).items() if k != "intensity"}
    with pytest.raises(pcv.PcvError) as e:
        stream.append(bare)
    assert e.value.code == pcv.PCV_E_INVALID and "S2Splitter received incompatible data types for attribute intensity" in str(e.value)
    stream.abort()
    same_directory(out, whole_dir)
    with pytest.raises(pcv.PcvError) as e:  # no meta.pb there
        ctx.s2_stream(20, tmp_path / "nothing", "append")
    assert "meta.pb" in str(e.value)


# ---- refusals -----------------------------------------------------------------------------------------------------------
def test_an_invalid_point_refuses_its_batch_only(ctx, uniform):
    points, _ = uniform
    stream = stream_of(ctx, points, [(0, 500), (500, 1200)])
    bad = {k: v.copy() for k, v in take(points, 1200, 2000).items()}
    bad["x"][5], bad["y"][5], bad["z"][5] = 1.0, 2.0, 3.0
    bad["x"][9] = float("nan")
    with pytest.raises(pcv.PcvError) as e:
        stream.append(bad)
    assert e.value.code == pcv.PCV_E_INVALID
    assert "Point (1, 2, 3) at index 5 is not a valid ECEF point" in str(e.value) and "(batch 2 of the stream)" in str(e.value)
    assert stream.info["batches"] == 2 and stream.info["points"] == 1200 and stream.info["pending_points"] == 1200
    stream.append(take(points, 3000, 3100))
    cloud = stream.finish()
    keep = np.r_[0:1200, 3000:3100]
    want = ctx.s2_split({k: v[keep] for k, v in points.items()})
    same_cloud(cloud, want)
    cloud.free()
    want.free()


def test_intensity_mismatch(ctx, uniform):
    points, _ = uniform
    bare = {k: v for k, v in points.items() if k != "intensity"}
    empty_bare = take(bare, 0, 0)
    for first, second in ((points, bare), (bare, points)):
        stream = ctx.s2_stream()
        stream.append(empty_bare)  # an empty batch decides nothing
        stream.append(take(first, 0, 100))
        with pytest.raises(pcv.PcvError) as e:
            stream.append(take(second, 100, 200))
        assert e.value.code == pcv.PCV_E_INVALID
        assert "S2Splitter received incompatible data types for attribute intensity" in str(e.value) and "(batch 2 of the stream)" in str(e.value)
        stream.append(take(first, 100, 200))
        cloud = stream.finish()
        want = ctx.s2_split(take(first, 0, 200))
        same_cloud(cloud, want)
        cloud.free()
        want.free()


def test_in_memory_overflow_is_decided_on_the_host(ctx, uniform):
    """The limit of 2^32 - 1 points, lowered to 1 000 through the test hook: the append that reaches it is refused."""
    points, _ = uniform
    stream = ctx.s2_stream()
    stream._set_memory_cap(1000)
    stream.append(take(points, 0, 600))
    with pytest.raises(pcv.PcvError) as e:
        stream.append(take(points, 600, 1000))
    assert e.value.code == pcv.PCV_E_INVALID and "fewer than 1000 points" in str(e.value)
    stream.append(take(points, 600, 999))
    assert stream.info["points"] == 999
    cloud = stream.finish()
    want = ctx.s2_split(take(points, 0, 999))
    same_cloud(cloud, want)
    cloud.free()
    want.free()
    with pytest.raises(pcv.PcvError):
        ctx.s2_stream()._set_memory_cap(0)


def test_finish_twice_append_after_finish_abort(ctx, uniform, tmp_path):
    points, _ = uniform
    stream = ctx.s2_stream()
    stream.append(take(points, 0, 50))
    stream.finish().free()
    with pytest.raises(ValueError):
        stream.finish()
    with pytest.raises(ValueError):
        stream.append(take(points, 0, 50))
    with pytest.raises(ValueError):
        stream.info
    stream = ctx.s2_stream()
    stream.append(take(points, 0, 50))
    stream.abort()
    stream.abort()
    with pytest.raises(ValueError):
        stream.append(take(points, 0, 50))
    # the context manager aborts on an exception; what was flushed stays, no meta.pb is written
    out = tmp_path / "aborted"
    with pytest.raises(RuntimeError):
        with ctx.s2_stream(directory=out, flush_points=10) as stream:
            stream.append(take(points, 0, 50))
            raise RuntimeError("the reader failed")
    assert stream.handle is None and not (out / "meta.pb").exists() and any(name.endswith(".xyz") for name in os.listdir(out))
    with pytest.raises(pcv.PcvError):
        ctx.s2_stream(split_level=31)
    with pytest.raises(ValueError):
        ctx.s2_stream(open_mode="update")


# ---- build_s2_cells over an iterator, and the read side over it ------------------------------------------------------------
def test_build_s2_cells_of_an_iterator_of_batches(ctx, uniform, whole_dir, tmp_path):
    points, whole = uniform
    n = points["x"].size
    position = np.stack([points["x"], points["y"], points["z"]], axis=1)

    def batches():
        for lo in range(0, n, 3333):
            yield dict(position=position[lo:lo + 3333], color=points["color"][lo:lo + 3333], intensity=points["intensity"][lo:lo + 3333])

    out = tmp_path / "iterated"
    cloud = pcv.build_s2_cells(str(out), batches(), ctx=ctx, flush_points=7000)
    same_directory(out, whole_dir)
    lo = np.array([np.quantile(points[a], 0.3) for a in "xyz"])
    hi = np.array([np.quantile(points[a], 0.8) for a in "xyz"])
    shapes = ctx.shapes([("aabb", lo, hi)])
    got, want = cloud.query_batch(shapes), whole.query_batch(shapes)
    assert got.num_points == want.num_points > 100 and got.num_segments == want.num_segments
    for a, b in zip(got.segments(), want.segments()):
        assert np.array_equal(a, b)
    a, b = got.points(), want.points()
    for key in ("x", "y", "z", "rgb", "intensity"):
        assert a[key].tobytes() == b[key].tobytes(), key
    for q in (got, want, shapes, cloud):
        q.free()
    assert len(list(itertools.islice(batches(), 10))) == 7
