"""Query results as PLY files (pcv_ply_rows.hip, pcv_ply_write.cpp): the rows packed on the device and the files
written from them against tests/ply_write_truth.py — a header built from the format's rules and a packed numpy dtype filled
from points() / attribute() of the same batch — byte for byte; append, the pieces of the pipeline, its memory, the round
trips through read_ply, and the refusals. Small clouds: 6 000 points in an octree of at least 40 nodes, 4 001 ECEF points in at
least 30 S2 cells."""
import ctypes as C
import os

import numpy as np
import pytest

import point_cloud_viewer_amd as pcv
from point_cloud_viewer_amd import _lib as L
from point_cloud_viewer_amd import synthetic

import ply_write_truth as PT
import s2_truth as T
from test_s2_attr_cpu import random_column

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "xyz_f32_rgb_u8_intensity_f32.ply")
N_OCTREE, N_S2, LEVEL = 6000, 4001, 18
# (no name ends in a digit: the reader takes such a property for a component of a vector and skips it)
EXTRAS = {"a_byte": "u8", "ring": "u16", "timestamp": "i64", "gps": "u64", "reflect": "f32", "normal": "f64vec3"}


@pytest.fixture(scope="module")
def ctx():
    c = pcv.Context(0)
    yield c
    c.close()


def odd_intensity(n, seed):
    """float32 with NaNs of distinct payloads and a -0.0 among ordinary values."""
    rng = np.random.Generator(np.random.PCG64(seed))
    v = (rng.random(n) * 200.0 - 50.0).astype(np.float32)
    bits = v.view(np.uint32)
    bits[5:5 + 40] = 0x7FC00001 + np.arange(40, dtype=np.uint32) * 0x101  # quiet NaNs, every payload another
    bits[60:70] = 0xFFC00000 | (np.arange(10, dtype=np.uint32) + 7)        # negative ones
    bits[100] = 0x80000000                                                  # -0.0
    return v


def isolated_point(px, py, pz, eps):
    """A point with no other within 2 eps of it (Chebyshev): the box of half-width eps around it keeps exactly one point."""
    p = np.stack([px, py, pz], axis=1)
    for i in range(len(p)):
        if np.sum(np.abs(p - p[i]).max(axis=1) <= 2 * eps) == 1:
            return p[i]
    raise AssertionError("no isolated point")


def octree_scene(ctx, with_intensity, cap):
    x, y, z, rgb, bmin, bmax = synthetic.gaussian_clusters(N_OCTREE, seed=17, num_clusters=5, extent=120.0, sigma_range=(0.5, 6.0))
    inten = odd_intensity(N_OCTREE, 3) if with_intensity else None
    tree = ctx.build(0.001, pcv.Aabb(bmin, bmax), x, y, z, rgb, inten, max_points_per_node=cap)
    every = tree.query_batch(ctx.shapes([("all",)]))
    decoded = every.points()
    every.free()
    one = isolated_point(decoded["x"], decoded["y"], decoded["z"], 0.01)
    # AllPoints; a box that keeps about half; a box that meets the root and holds no point; a box around one point
    shapes = ctx.shapes([("all",), ("aabb", bmin - 1.0, [np.median(x), bmax[1] + 1.0, bmax[2] + 1.0]), ("aabb", bmin - 1.0, bmin + 1e-7),
                         ("aabb", one - 0.01, one + 0.01)])
    batch = tree.query_batch(shapes)
    have = {"color": "u8vec3", **({"intensity": "f32"} if with_intensity else {})}
    return dict(tree=tree, batch=batch, have=have, points=batch.points(), columns={}, bmin=bmin, bmax=bmax, cap=cap)


@pytest.fixture(scope="module")
def octree_i(ctx):
    sc = octree_scene(ctx, True, 120)
    assert sc["tree"].num_nodes >= 40
    return sc


@pytest.fixture(scope="module")
def octree_c(ctx):
    return octree_scene(ctx, False, 120)


@pytest.fixture(scope="module")
def octree_big(ctx):
    """The same points in a few large nodes: segments of many chunks, chunks of several 64-lane groups."""
    return octree_scene(ctx, True, 5000)


def make_s2_scene(ctx):
    x, y, z, rgb = (a[:N_S2] for a in T.uniform_cloud())
    rng = np.random.Generator(np.random.PCG64(11))
    attrs = {name: random_column(typ, N_S2, rng) for name, typ in EXTRAS.items()}
    points = dict(x=x, y=y, z=z, color=rgb, intensity=odd_intensity(N_S2, 4), attributes=attrs)
    cloud = ctx.s2_split(points, LEVEL)
    assert cloud.num_cells >= 30
    lo, hi = np.array([x.min(), y.min(), z.min()]), np.array([x.max(), y.max(), z.max()])
    one = isolated_point(x, y, z, 0.001)
    shapes = ctx.shapes([("all",), ("aabb", lo - 1.0, [np.median(x), hi[1] + 1.0, hi[2] + 1.0]), ("aabb", hi + 10.0, hi + 20.0),
                         ("aabb", one - 0.001, one + 0.001)])
    batch = cloud.query_batch(shapes)
    columns = {name: batch.attribute(name) for name in EXTRAS}
    have = {"color": "u8vec3", "intensity": "f32", **EXTRAS}
    return dict(cloud=cloud, batch=batch, have=have, points=batch.points(), columns=columns, input=points)


@pytest.fixture(scope="module")
def s2_scene(ctx):
    sc = make_s2_scene(ctx)
    yield sc
    sc["batch"].free()  # before its cloud: pcv_s2_query_free reads the cloud
    sc["cloud"].free()


def pick(sc, names):
    """names (None: all) as the dict name -> type the truth takes."""
    return dict(sc["have"]) if names is None else {n: sc["have"][n] for n in names}


def truth_rows(sc, names):
    return PT.rows(sc["points"], sc["columns"], pick(sc, names))


def check_scene_is_what_the_tests_need(sc):
    first, _, off = sc["batch"].segments()
    kept = [int(off[first[s + 1]] - off[first[s]]) for s in range(4)]
    total = kept[0]
    assert total in (N_OCTREE, N_S2) and 0.3 * total < kept[1] < 0.7 * total and kept[2] == 0 and kept[3] == 1, kept
    return first, off


OCTREE_SETS = [None, [], ["color"], ["intensity"]]  # strides 31, 24, 27, 28
S2_SETS = [None, ["color"] + list(EXTRAS), ["a_byte"], ["ring"], ["intensity"]]  # strides 78, 74, 25, 26, 28


def check_every_range(sc, names, want_stride):
    batch = sc["batch"]
    first, off = check_scene_is_what_the_tests_need(sc)
    want = truth_rows(sc, names)
    assert want.shape[1] == want_stride
    nseg = batch.num_segments
    got, layout = batch.ply_rows(attributes=names)  # the whole batch, host
    assert layout["stride"] == want_stride and got.shape == want.shape and got.tobytes() == want.tobytes()
    assert layout["dtype"] == PT.row_dtype(pick(sc, names))
    sizes = set()
    for k in range(nseg):  # each single segment
        got, _ = batch.ply_rows(first_segment=k, num_segments=1, attributes=names)
        a, b = int(off[k]), int(off[k + 1])
        sizes.add(b - a)
        assert got.tobytes() == want[a:b].tobytes(), k
    assert {0, 1} <= sizes and max(sizes) > 64, sorted(sizes)  # segments with no kept point, with one, and with more than a wave's lanes
    for start in range(min(17, nseg + 1)):  # every range that starts at segments 0 .. 16, the empty one first
        for num in range(0, nseg - start + 1):
            got, _ = batch.ply_rows(first_segment=start, num_segments=num, attributes=names)
            a, b = int(off[start]), int(off[start + num])
            assert got.shape == (b - a, want_stride) and got.tobytes() == want[a:b].tobytes(), (start, num)
    for s in range(4):  # the four shapes; device memory
        got, _ = batch.ply_rows(shape=s, attributes=names, device=True)
        a, b = int(off[first[s]]), int(off[first[s + 1]])
        assert tuple(got.shape) == (b - a, want_stride) and got.cpu().numpy().tobytes() == want[a:b].tobytes(), s
    for k in range(0, nseg, 3):
        got, _ = batch.ply_rows(first_segment=k, num_segments=min(2, nseg - k), attributes=names, device=True)
        a, b = int(off[k]), int(off[k + min(2, nseg - k)])
        assert got.cpu().numpy().tobytes() == want[a:b].tobytes(), k


@pytest.mark.parametrize("which", range(len(OCTREE_SETS)))
def test_octree_rows_equal_the_truth(octree_i, which):
    check_every_range(octree_i, OCTREE_SETS[which], [31, 24, 27, 28][which])


@pytest.mark.parametrize("which", [0, 1])
def test_octree_rows_without_intensity(octree_c, which):
    check_every_range(octree_c, [None, []][which], [27, 24][which])


def test_octree_rows_of_large_nodes(octree_big):
    check_every_range(octree_big, None, 31)
    check_every_range(octree_big, ["color"], 27)


@pytest.mark.parametrize("which", range(len(S2_SETS)))
def test_s2_rows_equal_the_truth(s2_scene, which):
    check_every_range(s2_scene, S2_SETS[which], [78, 74, 25, 26, 28][which])


def names_array(names):
    if names is None:
        return None, 0
    enc = [n.encode() for n in names]
    return (C.c_char_p * max(1, len(enc)))(*enc), len(enc)


@pytest.mark.parametrize("kind", ["octree", "s2"])
def test_rows_at_every_alignment_and_nothing_beside_them(ctx, octree_i, s2_scene, kind):
    """The output at every residue mod 16, for odd and even strides: the head, interior and tail of every tile; the bytes before
    and after the rows stay what they were."""
    import torch
    sc, sets = (octree_i, OCTREE_SETS) if kind == "octree" else (s2_scene, S2_SETS)
    fn = ctx.lib.pcv_query_batch_ply_rows if kind == "octree" else ctx.lib.pcv_s2_query_ply_rows
    batch = sc["batch"]
    for names in sets:
        want = truth_rows(sc, names)
        nbytes = want.size
        arr, count = names_array(names)
        for k in range(16):
            buf = torch.full((nbytes + 64,), 0xA5, dtype=torch.uint8, device=f"cuda:{ctx.device}")
            torch.cuda.synchronize()
            stride, rows = C.c_uint32(), C.c_uint64()
            ctx._check(fn(batch.handle, 0, batch.num_segments, arr, count, nbytes, L.MEM_DEVICE, buf.data_ptr() + 16 + k, C.byref(stride), C.byref(rows)))
            host = buf.cpu().numpy()
            assert (stride.value, rows.value) == (want.shape[1], want.shape[0])
            assert host[16 + k:16 + k + nbytes].tobytes() == want.tobytes(), (names, k)
            assert np.all(host[:16 + k] == 0xA5) and np.all(host[16 + k + nbytes:] == 0xA5), (names, k)


@pytest.mark.parametrize("kind", ["octree", "s2"])
def test_files_equal_header_rows_newline_whatever_the_pieces(ctx, octree_i, s2_scene, tmp_path, kind):
    sc, sets = (octree_i, OCTREE_SETS[:3]) if kind == "octree" else (s2_scene, S2_SETS[:3])
    batch = sc["batch"]
    first, off = check_scene_is_what_the_tests_need(sc)
    for names in sets:
        attrs = pick(sc, names)
        rows = truth_rows(sc, names)
        for shape in (0, 1):
            a, b = int(off[first[shape]]), int(off[first[shape + 1]])
            want = PT.file_bytes(attrs, [rows[a:b]])
            for chunk in (1, 63, 64, 1000, 0) if (shape == 1 or names is None) else (63, 0):
                path = tmp_path / f"{kind}_{shape}_{chunk}.ply"
                written = batch.write_ply(path, shape=shape, attributes=names, chunk_points=chunk)
                assert written == b - a and path.read_bytes() == want, (names, shape, chunk)
    # a segment range in the middle, through the default arguments' path
    k0, kn = 3, min(9, batch.num_segments - 3)
    written = batch.write_ply(tmp_path / "mid.ply", first_segment=k0, num_segments=kn)
    rows = truth_rows(sc, None)[int(off[k0]):int(off[k0 + kn])]
    assert written == len(rows) and (tmp_path / "mid.ply").read_bytes() == PT.file_bytes(sc["have"], [rows])


def test_pipeline_memory_does_not_grow_with_the_result(ctx, octree_i, s2_scene, tmp_path):
    """chunk_points = 64: two row buffers of 64 rows from the pool, whatever the result holds (6 000, about 3 000, 4 001 rows)."""
    for sc in (octree_i, s2_scene):
        stride = PT.stride(sc["have"])
        per_buffer = (64 * stride + 255) // 256 * 256
        for shape in (0, 1):
            ctx.trim()  # no cached block may stand in for a fresh one of another size
            live, _ = ctx.pool_stats(reset_peak=True)
            sc["batch"].write_ply(tmp_path / "m.ply", shape=shape, chunk_points=64)
            live_after, peak = ctx.pool_stats()
            assert live_after == live and peak - live == 2 * per_buffer, (stride, shape, peak - live)


@pytest.mark.parametrize("kind", ["octree", "s2"])
def test_append(ctx, octree_i, s2_scene, tmp_path, kind):
    sc = octree_i if kind == "octree" else s2_scene
    batch = sc["batch"]
    first, off = check_scene_is_what_the_tests_need(sc)
    a, b = int(off[first[1]]), int(off[first[2]])
    rows = truth_rows(sc, None)[a:b]
    path = tmp_path / "twice.ply"
    assert batch.write_ply(path, shape=1) == b - a
    assert batch.write_ply(path, shape=1, open_mode="append", chunk_points=777) == b - a
    want = PT.file_bytes(sc["have"], [rows, rows])
    assert path.read_bytes() == want and want[51:71] == b"%020d" % (2 * (b - a))
    assert pcv.ply_append_check(path, sc["have"]) == 2 * (b - a)
    # another column set: refused, the file stays byte-identical
    with pytest.raises(pcv.PcvError) as e:
        batch.write_ply(path, shape=1, attributes=["color"], open_mode="append")
    assert e.value.code == pcv.PCV_E_INVALID and "property" in str(e.value) and path.read_bytes() == want
    # an empty range appends nothing
    assert batch.write_ply(path, shape=2, open_mode="append") == 0 and path.read_bytes() == want
    assert batch.write_ply(path, first_segment=4, num_segments=0, open_mode="append") == 0 and path.read_bytes() == want
    # append to no file, and to a file shorter than the fixed prefix: written anew
    fresh = tmp_path / "fresh.ply"
    assert batch.write_ply(fresh, shape=1, open_mode="append") == b - a and fresh.read_bytes() == PT.file_bytes(sc["have"], [rows])
    short = tmp_path / "short.ply"
    short.write_bytes(b"ply\nformat")
    assert batch.write_ply(short, shape=1, open_mode="append") == b - a and short.read_bytes() == PT.file_bytes(sc["have"], [rows])
    # an empty range in truncate mode leaves no file and removes nothing else
    before = sorted(os.listdir(tmp_path))
    assert batch.write_ply(tmp_path / "none.ply", shape=2) == 0
    assert sorted(os.listdir(tmp_path)) == before
    assert batch.write_ply(path, shape=2) == 0 and path.read_bytes() == want  # (not even the file it names)


def test_the_references_own_round_trip(ctx, tmp_path):
    """test_ply_read_write (ply.rs:796-836) restated: the golden file -> cloud -> AllPoints -> write, then append -> read. The
    file's points lie 3 to 40 m from the origin, which S2Splitter refuses (s2.rs:64-71) in the reference as here, so they are
    moved to the earth's surface by one constant first; everything else is the reference's test."""
    src = pcv.read_ply(GOLDEN)
    n = len(src["x"])
    assert n == 8 and np.all(np.isnan(src["intensity"]))
    x = src["x"] + 6_370_000.0
    cloud = ctx.s2_split(dict(x=x, y=src["y"], z=src["z"], color=src["color"], intensity=src["intensity"]), 20)
    order = cloud.order
    batch = cloud.query_batch(ctx.shapes([("all",)]))
    path = tmp_path / "out.ply"
    assert batch.write_ply(path) == n
    assert batch.write_ply(path, open_mode="append") == n
    batch.free()
    cloud.free()
    got = pcv.read_ply(path)
    twice = np.concatenate([order, order])
    assert got["x"].tobytes() == x[twice].tobytes() and got["y"].tobytes() == src["y"][twice].tobytes() and got["z"].tobytes() == src["z"][twice].tobytes()
    assert got["color"].tobytes() == src["color"][twice].tobytes()
    assert got["intensity"].shape == (2 * n,) and np.all(np.isnan(got["intensity"]))


def test_s2_cloud_round_trip_with_extras(ctx, s2_scene, tmp_path):
    """cloud -> AllPoints -> PLY -> read_ply(extras=True) -> s2_split: the same cells, points and scalar extras (the F64Vec3
    column becomes normal0 .. normal2 in the file, which the reader skips: it is lost, as documented)."""
    cloud, batch = s2_scene["cloud"], s2_scene["batch"]
    path = tmp_path / "cloud.ply"
    assert batch.write_ply(path, shape=0, chunk_points=500) == N_S2
    back = pcv.read_ply(path, extras=True)
    scalars = {k: v for k, v in EXTRAS.items() if k != "normal"}
    assert sorted(back["attributes"]) == sorted(scalars)
    again = ctx.s2_split(back, LEVEL)
    assert again.attributes == scalars and again.has_intensity
    for a, b in zip(again.cells, cloud.cells):
        assert np.array_equal(a, b)
    for a, b in zip(again.cell_points(), cloud.cell_points()):
        assert a.tobytes() == b.tobytes()
    for name in scalars:
        assert again.cell_attribute(name).tobytes() == cloud.cell_attribute(name).tobytes(), name
    again.free()


def test_octree_round_trip(ctx, octree_i, tmp_path):
    """The PLY of AllPoints -> build_octree_from_file's device path gives the octree that the decoded points give directly."""
    sc = octree_i
    path = tmp_path / "tree.ply"
    assert sc["batch"].write_ply(path, shape=0) == N_OCTREE
    first, off = check_scene_is_what_the_tests_need(sc)
    pts = sc["batch"].points(int(first[0]), int(first[1] - first[0]))
    direct = ctx.build(0.001, None, pts["x"], pts["y"], pts["z"], pts["rgb"], pts["intensity"], max_points_per_node=120)
    from_file = ctx.build_from_ply(0.001, path, with_intensity=True, max_points_per_node=120)
    a, b = direct.to_dict(), from_file.to_dict()
    assert direct.node_names() == from_file.node_names() and len(a) >= 40
    for name in a:
        assert a[name]["num_points"] == b[name]["num_points"] and a[name]["xyz"] == b[name]["xyz"] and a[name]["rgb"] == b[name]["rgb"], name
        assert a[name]["intensity"] == b[name]["intensity"], name
    direct.free()
    from_file.free()


def test_one_file_per_location(ctx, octree_i, tmp_path):
    """9 slabs along x with about as many points each, two of them moved off the cloud: 7 files, each the single-range call's."""
    sc = octree_i
    bmin, bmax = sc["bmin"], sc["bmax"]
    cuts = np.quantile(sc["points"]["x"][:N_OCTREE], np.linspace(0, 1, 10))
    cuts[0], cuts[-1] = bmin[0] - 1.0, bmax[0] + 1.0
    tiles = []
    for k in range(9):
        lo = np.array([cuts[k], bmin[1] - 1.0, bmin[2] - 1.0])
        hi = np.array([cuts[k + 1], bmax[1] + 1.0, bmax[2] + 1.0])
        if k in (2, 6):
            lo, hi = lo + 10_000.0, hi + 10_000.0
        tiles.append(("aabb", lo, hi))
    batch = sc["tree"].query_batch(ctx.shapes(tiles))
    first, _, off = batch.segments()
    kept = [int(off[first[s + 1]] - off[first[s]]) for s in range(9)]
    assert [k for k in range(9) if kept[k] == 0] == [2, 6], kept  # (a tile of the cloud without points would be a third)
    written = batch.write_ply_per_location(str(tmp_path / "tile_{}.ply"))
    assert written == {k: kept[k] for k in range(9) if k not in (2, 6)}
    assert sorted(os.listdir(tmp_path)) == sorted(f"tile_{k}.ply" for k in range(9) if k not in (2, 6))
    rows = PT.rows(batch.points(), {}, sc["have"])
    for k in written:
        single = tmp_path / "single.ply"
        batch.write_ply(single, first_segment=int(first[k]), num_segments=int(first[k + 1] - first[k]))
        want = PT.file_bytes(sc["have"], [rows[int(off[first[k]]):int(off[first[k + 1]])]])
        assert (tmp_path / f"tile_{k}.ply").read_bytes() == want == single.read_bytes(), k
        single.unlink()
    batch.free()


@pytest.mark.parametrize("kind", ["octree", "s2"])
def test_errors_write_nothing(ctx, octree_i, s2_scene, tmp_path, kind):
    sc = octree_i if kind == "octree" else s2_scene
    batch = sc["batch"]
    fn = ctx.lib.pcv_query_batch_ply_rows if kind == "octree" else ctx.lib.pcv_s2_query_ply_rows
    nseg, stride = batch.num_segments, PT.stride(sc["have"])
    out = np.full(batch.num_points * stride, 0x5A, dtype=np.uint8)
    s, r = C.c_uint32(), C.c_uint64()

    def rows_call(first, num, names, cap):
        arr, count = names_array(names)
        return fn(batch.handle, first, num, arr, count, cap, L.MEM_HOST, out.ctypes.data, C.byref(s), C.byref(r))

    assert rows_call(0, nseg + 1, None, out.size) == pcv.PCV_E_INVALID and "past the end" in ctx.lib.pcv_last_error(ctx.handle).decode()
    assert rows_call(nseg + 1, 0, None, out.size) == pcv.PCV_E_INVALID
    assert rows_call(0, nseg, None, out.size - 1) == pcv.PCV_E_INVALID and (s.value, r.value) == (stride, batch.num_points)
    assert rows_call(0, nseg, ["color", "nope"], out.size) == pcv.PCV_E_INVALID
    assert ctx.lib.pcv_last_error(ctx.handle).decode() == "Data type for attribute 'nope' not found."
    assert rows_call(0, nseg, ["color", "color"], out.size) == pcv.PCV_E_INVALID
    assert rows_call(0, nseg, None, out.size) == pcv.PCV_OK and np.any(out != 0x5A)  # (the buffer was large enough all along)
    out[:] = 0x5A
    assert rows_call(0, nseg, None, 0) == pcv.PCV_E_INVALID and np.all(out == 0x5A)
    for kwargs, word in ((dict(first_segment=0, num_segments=nseg + 1), "past the end"), (dict(attributes=["nope"]), "'nope' not found."),
                         (dict(attributes=["color", "color"]), "twice")):
        with pytest.raises(pcv.PcvError) as e:
            batch.write_ply(tmp_path / "bad.ply", **kwargs)
        assert e.value.code == pcv.PCV_E_INVALID and word in str(e.value), str(e.value)
    with pytest.raises(pcv.PcvError) as e:
        batch.ply_rows(attributes=["nope"])
    assert "'nope' not found." in str(e.value)
    with pytest.raises(ValueError):
        batch.write_ply(tmp_path / "bad.ply", open_mode="overwrite")
    missing = tmp_path / "no_such_directory" / "out.ply"
    with pytest.raises(pcv.PcvError) as e:
        batch.write_ply(missing)
    assert e.value.code == pcv.PCV_E_IO and str(missing) in str(e.value)
    pr = L.PlyWriteParams()
    pr.struct_size = 8
    wfn = ctx.lib.pcv_query_batch_write_ply if kind == "octree" else ctx.lib.pcv_s2_query_write_ply
    assert wfn(batch.handle, 0, nseg, str(tmp_path / "bad.ply").encode(), C.byref(pr), None) == pcv.PCV_E_INVALID
    assert os.listdir(tmp_path) == []


def run_example(args):
    import subprocess
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "examples"), "bin/query_to_ply"])
    return subprocess.run([os.path.join(ROOT, "examples", "bin", "query_to_ply")] + [str(a) for a in args], capture_output=True, text=True)


def test_example_over_an_octree_directory(ctx, octree_i, tmp_path):
    """examples/query_to_ply.c over the written octree: one box, an intensity filter, a column list, then the same appended."""
    sc = octree_i
    sc["tree"].write_dir(tmp_path / "tree")
    lo, hi = sc["bmin"] - 1.0, np.array([np.median(sc["points"]["x"][:N_OCTREE]), sc["bmax"][1] + 1.0, sc["bmax"][2] + 1.0])
    batch = sc["tree"].query_batch(ctx.shapes([("aabb", lo, hi)]), intervals=[(-10.0, 90.0)])
    assert 0 < batch.num_points < N_OCTREE // 2
    want = tmp_path / "want.ply"
    batch.write_ply(want, attributes=["intensity"])
    box = ",".join(repr(float(v)) for v in list(lo) + list(hi))
    args = [tmp_path / "tree", "--aabb", box, "--filter", "intensity:-10:90", "--attributes", "intensity", "--output", tmp_path / "got.ply"]
    p = run_example(args)
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "got.ply").read_bytes() == want.read_bytes()
    p = run_example(args + ["--append", "--per-location", tmp_path / "loc_%u.ply"])
    assert p.returncode == 0, p.stderr
    batch.write_ply(want, attributes=["intensity"], open_mode="append")
    assert (tmp_path / "got.ply").read_bytes() == want.read_bytes()
    batch.write_ply(want, attributes=["intensity"])
    assert (tmp_path / "loc_0.ply").read_bytes() == want.read_bytes()  # (append to no file writes it anew)
    p = run_example([tmp_path / "tree", "--all", "--filter", "ring:0:1", "--output", tmp_path / "no.ply"])
    assert p.returncode == 1 and "intensity" in p.stderr and not (tmp_path / "no.ply").exists()
    batch.free()


def test_example_over_an_s2_directory(ctx, s2_scene, tmp_path):
    """The same over the written S2 cloud: a filter on an extra with chosen columns; then the map tiles of zoom 19, whose files
    together hold every point once."""
    cloud = s2_scene["cloud"]
    cloud.write(tmp_path / "cloud")
    batch = cloud.query_batch(ctx.shapes([("all",)]), filters=[{"ring": (1000.0, 40000.0)}])
    assert 0 < batch.num_points < N_S2
    want = tmp_path / "want.ply"
    batch.write_ply(want, attributes=["timestamp", "color", "ring"])
    p = run_example([tmp_path / "cloud", "--all", "--filter", "ring:1000:40000", "--attributes", "timestamp,color,ring", "--output", tmp_path / "got.ply"])
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "got.ply").read_bytes() == want.read_bytes()
    batch.free()
    p = run_example([tmp_path / "cloud", "--map-tiles", "19", "--output", tmp_path / "tiles.ply", "--per-location", tmp_path / "tile_%u.ply"])
    assert p.returncode == 0, p.stderr
    # the same tiles here: the zoom-19 tiles that the corners of the bounding box span, row by row
    lo, hi = cloud.bbox_min, cloud.bbox_max
    corners = np.array([[(hi if k & 1 else lo)[0], (hi if k & 2 else lo)[1], (hi if k & 4 else lo)[2]] for k in range(8)])
    u, v = pcv.wmr_project(corners[:, 0], corners[:, 1], corners[:, 2])
    tx, ty = np.floor(u * 2 ** 19).astype(np.int64), np.floor(v * 2 ** 19).astype(np.int64)
    tiles = [pcv.web_mercator_rect_from_zoomed((256 * x, 256 * y), (256 * (x + 1), 256 * (y + 1)), 19)
             for y in range(ty.min(), ty.max() + 1) for x in range(tx.min(), tx.max() + 1)]
    assert len(tiles) >= 2 and all(tiles)
    batch = cloud.query_batch(ctx.shapes(tiles))
    first, _, off = batch.segments()
    assert batch.num_points > N_S2 // 2
    want = tmp_path / "want_tiles.ply"
    batch.write_ply(want)
    assert (tmp_path / "tiles.ply").read_bytes() == want.read_bytes()
    nonempty = [k for k in range(len(tiles)) if off[first[k + 1]] > off[first[k]]]
    assert sorted(f for f in os.listdir(tmp_path) if f.startswith("tile_")) == sorted(f"tile_{k}.ply" for k in nonempty)
    for k in nonempty[:3]:
        batch.write_ply(want, shape=k)
        assert (tmp_path / f"tile_{k}.ply").read_bytes() == want.read_bytes(), k
    batch.free()
