"""Typed extra attributes of S2 cell clouds on the device (pcv_s2_attr.hip): the split's gather, the stream's merge,
the query's filter and gather — columns compared as bytes (float columns hold random bit patterns, NaN payloads among them)
against numpy: a stable argsort of s2_truth.py's cell ids for the regroup, astype(float64) for the conversion, a brute-force
filter of all points for the query."""
import ctypes as C
import math

import numpy as np
import pytest

import point_cloud_viewer_amd as pcv
from point_cloud_viewer_amd import _lib as L

import s2_truth as T
from test_s2_attr_cpu import ALL_TYPES, SCALARS, brute_keep, dir_files, random_column

pytestmark = pytest.mark.gpu

LEVEL = 18  # the uniform cloud (a 200 m box) falls into 58 cells of ~38 m: 39 of them among its first 63 points
INF = math.inf


@pytest.fixture(scope="module")
def ctx():
    c = pcv.Context(0)
    yield c
    c.close()


def intensity_of(n):
    return (((np.arange(n, dtype=np.int64) * 2654435761) % 100003).astype(np.float32) * 0.25 - 7.0)


def columns_for(n, seed):
    """One column of every data type: name -> array; the names sort in another order than ALL_TYPES."""
    rng = np.random.Generator(np.random.PCG64(seed))
    return {f"{'lkjihgfedcba'[k]}_{t}": random_column(t, n, rng) for k, t in enumerate(ALL_TYPES)}


def type_of(name):
    return name.split("_", 1)[1]


@pytest.fixture(scope="module")
def cloud_points():
    """The uniform cloud's first 4 099 points with intensity and twelve extras, and the truth's cells — shared, read-only."""
    x, y, z, rgb = (a[:4099] for a in T.uniform_cloud())
    cells = T.parents(T.set_leaf_ids("uniform")[:4099], LEVEL)
    points = dict(x=x, y=y, z=z, color=rgb, intensity=intensity_of(4099), attributes=columns_for(4099, 7))
    return points, cells


def take(points, lo, hi):
    out = {k: v[lo:hi] for k, v in points.items() if k != "attributes"}
    out["attributes"] = {k: v[lo:hi] for k, v in points["attributes"].items()}
    return out


def to_device(points):
    """The batch as device tensors; u16 / u32 / u64 columns as same-sized signed tensors with their type stated."""
    import torch
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in points.items() if k != "attributes"}
    dev["attributes"] = {}
    for name, col in points["attributes"].items():
        t = type_of(name)
        signed = {"u16": np.int16, "u32": np.int32, "u64": np.int64}.get(t)
        dev["attributes"][name] = (torch.from_numpy(np.ascontiguousarray(col).view(signed)).cuda(), t) if signed else torch.from_numpy(np.ascontiguousarray(col)).cuda()
    torch.cuda.synchronize()
    return dev


def check_columns(cloud, points, order):
    assert list(cloud.attributes) == sorted(points["attributes"]) and cloud.attributes == {k: type_of(k) for k in points["attributes"]}
    for name, col in points["attributes"].items():
        got = cloud.cell_attribute(name)
        assert got.dtype == col.dtype and got.shape == col.shape
        assert got.tobytes() == col[order].tobytes(), name
    xyz, rgb, inten = cloud.cell_points()
    assert xyz.tobytes() == np.stack([points["x"], points["y"], points["z"]], axis=1)[order].tobytes()
    assert rgb.tobytes() == np.ascontiguousarray(points["color"][:, :3])[order].tobytes()
    if order.size:  # (an empty device tensor has no address: a batch without points says nothing about intensity)
        assert inten.tobytes() == points["intensity"][order].tobytes()


# ---- split ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 4099])
def test_split_regroups_every_column(ctx, cloud_points, n, device):
    points, cells = cloud_points
    batch = take(points, 0, n)
    order = np.argsort(cells[:n], kind="stable")
    ids, counts = np.unique(cells[:n], return_counts=True)
    assert n < 3 or ids.size >= 3
    cloud = ctx.s2_split(to_device(batch) if device else batch, LEVEL)
    assert cloud.num_points == n and np.array_equal(cloud.cells[0], ids) and np.array_equal(cloud.cells[1], counts.astype(np.uint64))
    if n:
        assert np.array_equal(cloud.order, order.astype(np.uint32))
    check_columns(cloud, batch, order)
    if n == 257:  # a cell range in the middle, and a capacity too small
        first, count = 3, 4
        lo, hi = int(cloud.cells[2][first]), int(cloud.cells[2][first + count])
        for name, col in batch["attributes"].items():
            assert cloud.cell_attribute(name, first, count).tobytes() == col[order][lo:hi].tobytes()
        out = np.zeros(1, dtype=np.uint8)
        assert ctx.lib.pcv_s2_cell_attribute(cloud.handle, b"l_u8", 0, cloud.num_cells, 256, L.MEM_HOST, out.ctypes.data) == pcv.PCV_E_INVALID
    cloud.free()


def test_split_ex_without_extras_is_split(ctx, cloud_points):
    points, _ = cloud_points
    plain = {k: v for k, v in points.items() if k != "attributes"}
    want = ctx.s2_split(plain, LEVEL)
    p, keep_alive = ctx._points(plain["x"], plain["y"], plain["z"], plain["color"], plain["intensity"])
    h = C.c_void_p()
    ctx._check(ctx.lib.pcv_s2_split_ex(ctx.handle, C.byref(p), None, 0, LEVEL, C.byref(h)))
    got = pcv.S2Cloud(ctx, h)
    assert got.attributes == {} and (got.num_points, got.num_cells, got.split_level, got.has_intensity) == (want.num_points, want.num_cells, LEVEL, True)
    for a, b in zip(got.cells, want.cells):
        assert np.array_equal(a, b)
    for a, b in zip(got.cell_points(), want.cell_points()):
        assert a.tobytes() == b.tobytes()
    assert np.array_equal(got.order, want.order) and got.bbox_min.tobytes() == want.bbox_min.tobytes() and got.bbox_max.tobytes() == want.bbox_max.tobytes()
    got.free(), want.free()


def test_split_refuses_bad_attributes(ctx, cloud_points):
    points, _ = cloud_points
    batch = take(points, 0, 65)
    for attrs, says in (({"color": np.zeros(65, dtype=np.uint8)}, "'color'"), ({"a.b": np.zeros(65, dtype=np.uint8)}, "'a.b'"),
                        ({f"a{k:02d}": np.zeros(65, dtype=np.uint8) for k in range(17)}, "16 extra attributes at most")):
        with pytest.raises(pcv.PcvError) as e:
            ctx.s2_split(dict(batch, attributes=attrs), LEVEL)
        assert e.value.code == pcv.PCV_E_INVALID and says in str(e.value)
    with pytest.raises(ValueError):
        ctx.s2_split(dict(batch, attributes={"short": np.zeros(64, dtype=np.uint8)}), LEVEL)


# ---- stream -----------------------------------------------------------------------------------------------------------------
SIZES = (0, 1, 300, 2049, 64)  # the fourth batch alone crosses the merge's 2 048-point chunk


def cuts_of(sizes):
    at = np.concatenate([[0], np.cumsum(sizes)])
    return [(int(at[k]), int(at[k + 1])) for k in range(len(sizes))]


@pytest.fixture(scope="module")
def streamed(ctx, cloud_points, tmp_path_factory):
    """The first 2 414 points, their one-shot split and its directory — shared, read-only."""
    points, cells = cloud_points
    n = sum(SIZES)
    whole = take(points, 0, n)
    order = np.argsort(cells[:n], kind="stable")
    cloud = ctx.s2_split(whole, LEVEL)
    check_columns(cloud, whole, order)
    directory = tmp_path_factory.mktemp("one_shot")
    cloud.write(directory)
    yield whole, order, cloud, directory
    cloud.free()


def test_stream_in_memory_equals_the_one_shot_split(ctx, streamed):
    whole, order, want, _ = streamed
    stream = ctx.s2_stream(LEVEL)
    for k, (lo, hi) in enumerate(cuts_of(SIZES)):
        batch = take(whole, lo, hi)
        stream.append(to_device(batch) if k == 2 else batch)
    got = stream.finish()
    assert np.array_equal(got.order, want.order) and all(np.array_equal(a, b) for a, b in zip(got.cells, want.cells))
    check_columns(got, whole, order)
    got.free()


def test_stream_directory_and_append(ctx, streamed, tmp_path):
    whole, order, want, one_shot = streamed
    d = tmp_path / "stream"
    stream = ctx.s2_stream(LEVEL, d, flush_points=512)
    for lo, hi in cuts_of(SIZES):
        stream.append(take(whole, lo, hi))
    assert stream.info["flushes"] == 1 and stream.info["pending_points"] == 64  # three parts merged and written; the last waits for finish
    opened = stream.finish()
    old = dir_files(d)
    assert old == dir_files(one_shot) and len(old) == 1 + 15 * want.num_cells  # byte for byte: xyz, rgb, intensity and 12 extras per cell
    meta = T.parse_s2_meta(old["meta.pb"])
    assert meta["attributes"] == [("color", T.U8VEC3), ("intensity", T.F32)] + [(k, L.ATTR_TYPES[type_of(k)][0]) for k in sorted(whole["attributes"])]
    check_columns(opened, whole, order)  # read back (and uploaded) extra by extra, on first use
    opened.free()
    # append: every file is the old one followed by the one-shot split of what was appended
    more = take(whole, 100, 1400)
    with ctx.s2_stream(LEVEL, d, open_mode="append", flush_points=512) as stream:
        for lo, hi in ((0, 700), (700, 1300)):
            stream.append(take(more, lo, hi))
        both = stream.finish()
    assert both.num_points == sum(SIZES) + 1300 and both.attributes == want.attributes
    added = ctx.s2_split(more, LEVEL)
    added.write(tmp_path / "added")
    new, extra = dir_files(d), dir_files(tmp_path / "added")
    assert set(new) == set(old) and set(extra) <= set(old)
    for name in old:
        if name != "meta.pb":
            assert new[name] == old[name] + extra.get(name, b""), name
    both.free(), added.free()


def test_stream_refusals_leave_the_stream_usable(ctx, streamed, tmp_path):
    whole, order, want, one_shot = streamed
    first, second = take(whole, 0, 1000), take(whole, 1000, sum(SIZES))

    def refused(stream, batch, name, k):
        with pytest.raises(pcv.PcvError) as e:
            stream.append(batch)
        assert e.value.code == pcv.PCV_E_INVALID
        assert f"S2Splitter received incompatible data types for attribute {name} (batch {k} of the stream)" in str(e.value)

    def variants(batch):
        a = batch["attributes"]
        yield dict(batch, attributes=dict(a, l_u8=a["l_u8"].view(np.int8))), "l_u8"  # another type
        yield dict(batch, attributes=dict(a, unknown=a["l_u8"])), "unknown"  # a name the stream does not know
        yield dict(batch, attributes={k: v for k, v in a.items() if k != "f_i32"}), "f_i32"  # one is missing
        yield {k: v for k, v in batch.items() if k != "attributes"}, "a_f64vec3"  # all are missing: the first by name

    stream = ctx.s2_stream(LEVEL)
    stream.append(first)
    for bad, name in variants(second):
        refused(stream, bad, name, 1)
    stream.append(second)
    got = stream.finish()
    check_columns(got, whole, order)
    got.free()
    # append mode: the directory's attribute set holds from the first batch on
    d = tmp_path / "d"
    want.write(d)
    stream = ctx.s2_stream(LEVEL, d, open_mode="append")
    for bad, name in variants(first):
        refused(stream, bad, name, 0)
    stream.append(first)
    both = stream.finish()
    assert both.num_points == sum(SIZES) + 1000 and both.attributes == want.attributes
    both.free()


# ---- query ------------------------------------------------------------------------------------------------------------------
QLEVEL = 16  # the uniform cloud's five cells of ~150 m: 6 908, 5 149, 4 470, 2 856 and 617 points
TIES = (2**53 + 1, 2**53 + 3, 2**64 - 1, 2**53, 2**53 + 2)


@pytest.fixture(scope="module")
def scene(ctx):
    """A cloud with cells of 1, 1 024, 1 025 and 2 500 points (the query's 1 024-candidate chunk and its neighbours), intensity and
    twelve extras; its columns in file order; three locations — an Aabb, AllPoints, a cell union — and their `contains` flags."""
    x, y, z, rgb = T.uniform_cloud()
    cells = T.parents(T.set_leaf_ids("uniform"), QLEVEL)
    ids, counts = np.unique(cells, return_counts=True)
    by_size = ids[np.argsort(-counts, kind="stable")]
    pick = np.concatenate([np.flatnonzero(cells == by_size[k])[:m] for k, m in enumerate((2500, 1025, 1024, 1))])
    pick = np.random.Generator(np.random.PCG64(12)).permutation(pick)
    n = pick.size
    assert n == 4550
    cols = columns_for(n, 21)
    cols["i_u64"] = cols["i_u64"].copy()
    cols["i_u64"][:len(TIES) * 40:40] = np.array(TIES, dtype=np.uint64)  # the ties, spread over the cloud
    points = dict(x=x[pick], y=y[pick], z=z[pick], color=rgb[pick], intensity=intensity_of(n), attributes=cols)
    order = np.argsort(cells[pick], kind="stable")
    cloud = ctx.s2_split(points, QLEVEL)
    assert sorted(cloud.cells[1].tolist()) == [1, 1024, 1025, 2500]
    check_columns(cloud, points, order)
    filed = {k: v[order] for k, v in cols.items()}
    filed["intensity"] = points["intensity"][order]
    xyz = np.stack([points["x"], points["y"], points["z"]], axis=1)[order]
    px, py, pz = (np.ascontiguousarray(xyz[:, k]) for k in range(3))
    big = int(np.argmax(cloud.cells[1]))
    mid = xyz[int(cloud.cells[2][big]):int(cloud.cells[2][big]) + 2500].mean(axis=0)
    shapes = ctx.shapes([("aabb", mid - 45.0, mid + 30.0), ("all",)])
    by_count = {int(c): int(i) for i, c in zip(cloud.cells[0], cloud.cells[1])}
    unions = [sorted([by_count[1024], by_count[1]])]
    keep = [np.asarray(ctx.cull_points(shapes, 0, px, py, pz)[0]).astype(bool), np.ones(n, dtype=bool),
            pcv.s2_union_contains(unions[0], px, py, pz).astype(bool)]
    assert 50 < keep[0].sum() < 4000 and keep[2].sum() == 1025
    lists = cloud.cells_in_location_indices(shapes, unions)
    assert [len(v) for v in lists][1:] == [4, 2] and len(lists[0]) >= 1
    yield cloud, shapes, unions, lists, keep, filed, xyz, points
    cloud.free()


def quartiles(col):
    with np.errstate(invalid="ignore"):
        a = col.astype(np.float64)
    a = np.sort(a[np.isfinite(a)])
    return float(a[a.size // 4]), float(a[(3 * a.size) // 4])


def expect(cloud, lists, keep, filed, filters):
    """Brute force: per location the kept slots in segment order and the segments' sizes."""
    _, counts, offsets = cloud.cells
    out = []
    for l, cells in enumerate(lists):
        ok = keep[l].copy()
        for name, (lo, hi) in ((filters[l] or {}) if filters else {}).items():
            ok &= brute_keep(filed[name], lo, hi).astype(bool)
        slots = [np.arange(int(offsets[c]), int(offsets[c] + counts[c])) for c in cells]
        slots = [s[ok[s]] for s in slots]
        out.append((np.concatenate(slots), [s.size for s in slots]))
    return out


def check_query(scene, filters, columns=None):
    cloud, shapes, unions, lists, keep, filed, xyz, points = scene
    batch = cloud.query_batch(shapes, unions, filters=filters)
    want = expect(cloud, lists, keep, filed, filters)
    first, cell, off = batch.segments()
    sizes = np.concatenate([np.asarray(w[1], dtype=np.uint64) for w in want])
    assert np.array_equal(cell, np.concatenate(lists)) and np.array_equal(off, np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64))
    for l, (slots, _) in enumerate(want):
        got = batch.shape_points(l)
        assert got["count"] == slots.size and np.stack([got["x"], got["y"], got["z"]], axis=1).tobytes() == xyz[slots].tobytes(), l
        assert got["intensity"].tobytes() == filed["intensity"][slots].tobytes()
        for name in (columns if columns is not None else (filters[l] or {}) if filters else ()):
            if name != "intensity":  # (first_segment > 0 for every location but the first)
                assert batch.attribute(name, int(first[l]), int(first[l + 1] - first[l])).tobytes() == filed[name][slots].tobytes(), (l, name)
    batch.free()
    return want


def test_query_without_filters_and_every_column(ctx, scene):
    cloud, shapes, unions, lists, keep, filed, xyz, points = scene
    names = list(points["attributes"])
    want = check_query(scene, [None, None, None], columns=names)
    assert [w[0].size for w in want] == [int(keep[0].sum()), 4550, 1025]
    # single segments past the first, the whole batch, an empty range; and the refusals of a range
    batch = cloud.query_batch(shapes, unions, filters=[None] * 3)
    every = np.concatenate([w[0] for w in want])
    _, _, off = batch.segments()
    for name in names:
        assert batch.attribute(name).tobytes() == filed[name][every].tobytes()
        for k in (1, batch.num_segments - 1):
            assert batch.attribute(name, k, 1).tobytes() == filed[name][every[int(off[k]):int(off[k + 1])]].tobytes()
        assert batch.attribute(name, 2, 0).size == 0
    with pytest.raises(pcv.PcvError) as e:
        batch.attribute(names[0], batch.num_segments, 1)
    assert e.value.code == pcv.PCV_E_INVALID
    with pytest.raises(pcv.PcvError) as e:
        batch.attribute("nothing")
    assert e.value.code == pcv.PCV_E_INVALID and "Data type for attribute 'nothing' not found." in str(e.value)
    out = np.zeros(8, dtype=np.uint64)
    assert ctx.lib.pcv_s2_query_attribute(batch.handle, b"i_u64", 0, batch.num_segments, 8, L.MEM_HOST, out.ctypes.data) == pcv.PCV_E_INVALID
    batch.free()
    # points() does not see the extras: the same points without them give the same batch
    bare = ctx.s2_split({k: v for k, v in points.items() if k != "attributes"}, QLEVEL)
    a, b = bare.query_batch(shapes, unions), cloud.query_batch(shapes, unions)
    for l in range(3):
        pa, pb = a.shape_points(l), b.shape_points(l)
        assert pa["count"] == pb["count"] and all(pa[k].tobytes() == pb[k].tobytes() for k in ("x", "y", "z", "rgb", "intensity"))
    a.free(), b.free(), bare.free()


@pytest.mark.parametrize("typ", SCALARS)
def test_one_filter_per_scalar_type(ctx, scene, typ):
    cloud, shapes, unions, lists, keep, filed, xyz, points = scene
    name = next(k for k in points["attributes"] if type_of(k) == typ)
    q1, q3 = quartiles(filed[name])
    want = check_query(scene, [{name: (q1, q3)}, {name: (-INF, q1)}, {name: (q3, INF)}])
    assert all(0 < w[0].size for w in want[1:])
    # the device's flags are the host twin's, bit for bit: AllPoints keeps exactly what s2_filter_keep keeps
    assert np.array_equal(want[1][0], np.flatnonzero(pcv.s2_filter_keep(typ, filed[name], -INF, q1)))
    for lo, hi in ((q3, q1), (math.nan, INF), (-INF, INF)):
        host = np.flatnonzero(pcv.s2_filter_keep(typ, filed[name], lo, hi))
        assert np.array_equal(check_query(scene, [None, {name: (lo, hi)}, None])[1][0], host)
        assert host.size == (0 if lo != -INF else int((brute_keep(filed[name], -INF, INF)).sum()))  # every value but NaN


def test_filters_are_anded_and_the_u64_ties(ctx, scene):
    cloud, shapes, unions, lists, keep, filed, xyz, points = scene
    u8, i64, f32 = quartiles(filed["l_u8"]), quartiles(filed["e_i64"]), quartiles(filed["d_f32"])
    check_query(scene, [{"l_u8": u8, "e_i64": i64}, {"d_f32": f32, "l_u8": (u8[0], INF), "j_u32": (0.0, 3e9)}, {"e_i64": (-INF, i64[1])}])
    check_query(scene, [{"l_u8": u8, "intensity": (0.0, 9000.0)}, {"intensity": (-3.0, 900.0)}, {"intensity": (1e9, 2e9), "e_i64": i64}])
    # "intensity" alone is pcv_s2_query_run's interval
    a = cloud.query_batch(shapes, unions, intervals=[None, (-3.0, 900.0), None])
    b = cloud.query_batch(shapes, unions, filters=[None, {"intensity": (-3.0, 900.0)}, None])
    assert all(np.array_equal(s, t) for s, t in zip(a.segments(), b.segments())) and a.shape_points(1)["x"].tobytes() == b.shape_points(1)["x"].tobytes()
    a.free(), b.free()
    # 2^53 + 1 -> 2^53 and 2^53 + 3 -> 2^53 + 4 (ties to even), 2^64 - 1 -> 2^64: decided on the device as astype(float64) decides
    col = filed["i_u64"]
    for lo, hi, values in ((2.0**53, 2.0**53, {2**53, 2**53 + 1}), (2.0**53 + 2, 2.0**53 + 2, {2**53 + 2}), (2.0**53 + 4, 2.0**53 + 4, {2**53 + 3}),
                           (2.0**64, 2.0**64, {2**64 - 1}), (math.nextafter(2.0**53, INF), math.nextafter(2.0**53 + 4, 0.0), {2**53 + 2})):
        kept = check_query(scene, [None, {"i_u64": (lo, hi)}, None])[1][0]
        planted = {int(v) for v in col[kept] if int(v) in TIES}
        assert planted == values, (lo, hi)


def test_query_refusals(ctx, scene):
    cloud, shapes, unions, lists, keep, filed, xyz, points = scene
    for filters, says in (([{"nothing": (0, 1)}, None, None], "Data type for attribute 'nothing' not found."),
                          ([None, {"a_f64vec3": (0, 1)}, None], "vector"), ([None, None, {"b_u8vec3": (0, 1)}], "vector"),
                          ([{"color": (0, 1)}, None, None], "vector")):
        with pytest.raises(pcv.PcvError) as e:
            cloud.query_batch(shapes, unions, filters=filters)
        assert e.value.code == pcv.PCV_E_INVALID and says in str(e.value)
    first, flat = np.array([0, len(unions[0])], dtype=np.uint32), np.array(unions[0], dtype=np.uint64)

    def run(entries):
        arr = (L.S2Filter * len(entries))()
        for k, (l, name) in enumerate(entries):
            arr[k].location, arr[k].attribute, arr[k].lo, arr[k].hi = l, name, 0.0, 1.0
        h = C.c_void_p()
        rc = ctx.lib.pcv_s2_query_run_ex(cloud.handle, shapes.handle, 1, first.ctypes.data, flat.ctypes.data, arr, len(entries), C.byref(h))
        assert not h.value
        return rc, ctx.lib.pcv_last_error(ctx.handle).decode()

    rc, msg = run([(1, b"l_u8"), (0, b"l_u8"), (1, b"l_u8")])
    assert rc == pcv.PCV_E_INVALID and "two filters on attribute 'l_u8' for location 1" in msg
    rc, msg = run([(2, b"intensity"), (2, b"intensity")])
    assert rc == pcv.PCV_E_INVALID and "two filters on attribute 'intensity' for location 2" in msg
    rc, msg = run([(3, b"l_u8")])
    assert rc == pcv.PCV_E_INVALID and "location 3" in msg
    bare = ctx.s2_split(dict(x=points["x"], y=points["y"], z=points["z"], color=points["color"]), QLEVEL)
    with pytest.raises(pcv.PcvError) as e:
        bare.query_batch(shapes, unions, filters=[{"intensity": (0, 1)}, None, None])
    assert e.value.code == pcv.PCV_E_INVALID and "no intensity" in str(e.value)
    bare.free()
