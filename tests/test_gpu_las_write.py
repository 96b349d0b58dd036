"""Query results as LAS files (pcv_las_write.hip, pcv_las_write.cpp): the records packed on the device against the
host twin fed from points() / attribute() of the same batch, byte for byte (tests/test_las_write_cpu.py pins the twin to the
numpy truth); info and the files against tests/las_write_truth.py; the pieces of the pipeline and its memory, auto offset,
out-of-range refusals, append, the round trip through the project's own LAS reader, and the pool guard. Small clouds: the 6 000
points of test_gpu_ply_write.py's octrees, 4 001 ECEF points in at least 30 S2 cells with all twelve LAS-named extras."""
import ctypes as C
import os

import numpy as np
import pytest

import point_cloud_viewer_amd as pcv
from point_cloud_viewer_amd import _lib as L

import las_truth as LT
import las_write_truth as WT
import s2_truth as T
from test_gpu_ply_write import N_OCTREE, N_S2, LEVEL, check_scene_is_what_the_tests_need, isolated_point, octree_scene, odd_intensity

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMATS = [0, 1, 2, 3, 6, 7, 8]
OCTREE_KW = dict(scale=0.001, offset=(-100.0, -100.0, -100.0))


@pytest.fixture(scope="module")
def ctx():
    c = pcv.Context(0)
    yield c
    c.close()


def as_points(sc):
    """points() / attribute() of the scene's batch as the dict the host twin and the truth take."""
    p = sc["points"]
    return dict(x=p["x"], y=p["y"], z=p["z"], color=p["rgb"].reshape(-1, 3), intensity=p["intensity"], attributes=sc["columns"])


def rows_of(points, a, b):
    return dict(x=points["x"][a:b], y=points["y"][a:b], z=points["z"][a:b], color=points["color"][a:b],
                intensity=None if points["intensity"] is None else points["intensity"][a:b],
                attributes={k: v[a:b] for k, v in points["attributes"].items()})


@pytest.fixture(scope="module")
def octree_i(ctx):
    sc = octree_scene(ctx, True, 120)
    assert sc["tree"].num_nodes >= 40
    sc["las"], sc["kw"] = as_points(sc), OCTREE_KW
    return sc


@pytest.fixture(scope="module")
def octree_big(ctx):
    """The same points in a few large nodes: chunks of several 64-lane groups."""
    sc = octree_scene(ctx, True, 5000)
    sc["las"], sc["kw"] = as_points(sc), OCTREE_KW
    return sc


def las_extras(n, rng):
    """All twelve LAS-named extras in their table types; return numbers with 0 and values above both fields; one foreign extra."""
    ret = rng.integers(0, 20, n).astype(np.uint8)
    ret[:4] = [0, 7, 8, 255]
    gps = rng.random(n) * 4e8
    gps.view(np.uint64)[2:6] = [0x7ff8000000000001, 0xfff0dead0000beef, 0x8000000000000000, 0x7ff0000000000000]
    angle = (rng.random(n) * 420.0 - 210.0).astype(np.float32)
    angle[:3] = [np.nan, np.inf, -0.0]
    return dict(classification=rng.integers(0, 256, n).astype(np.uint8), classification_flags=rng.integers(0, 32, n).astype(np.uint8),
                return_number=ret, number_of_returns=rng.integers(0, 20, n).astype(np.uint8),
                scan_direction_flag=rng.integers(0, 2, n).astype(np.uint8), edge_of_flight_line=rng.integers(0, 3, n).astype(np.uint8),
                scanner_channel=rng.integers(0, 6, n).astype(np.uint8), scan_angle=angle, user_data=rng.integers(0, 256, n).astype(np.uint8),
                point_source_id=rng.integers(0, 65536, n).astype(np.uint16), gps_time=gps, nir=rng.integers(0, 65536, n).astype(np.uint16),
                beam_id=rng.integers(0, 1000, n).astype(np.int32))


@pytest.fixture(scope="module")
def s2_scene(ctx):
    x, y, z, rgb = (a[:N_S2] for a in T.uniform_cloud())
    rng = np.random.Generator(np.random.PCG64(12))
    attrs = las_extras(N_S2, rng)
    inten = (rng.random(N_S2) * 70000.0 - 2000.0).astype(np.float32)
    inten[:3] = [np.nan, np.inf, 0.5]
    cloud = ctx.s2_split(dict(x=x, y=y, z=z, color=rgb, intensity=inten, attributes=attrs), LEVEL)
    assert cloud.num_cells >= 30
    lo, hi = np.array([x.min(), y.min(), z.min()]), np.array([x.max(), y.max(), z.max()])
    one = isolated_point(x, y, z, 0.001)
    shapes = ctx.shapes([("all",), ("aabb", lo - 1.0, [np.median(x), hi[1] + 1.0, hi[2] + 1.0]), ("aabb", hi + 10.0, hi + 20.0),
                         ("aabb", one - 0.001, one + 0.001)])
    batch = cloud.query_batch(shapes)
    sc = dict(cloud=cloud, batch=batch, points=batch.points(), columns={name: batch.attribute(name) for name in attrs})
    sc["las"], sc["kw"] = as_points(sc), dict(scale=0.001, offset=tuple(float(np.floor(v)) for v in lo))
    yield sc
    batch.free()  # before its cloud: pcv_s2_query_free reads the cloud
    cloud.free()


def check_every_range(sc, fmt, sweep):
    batch, pts, kw = sc["batch"], sc["las"], dict(sc["kw"], point_format=fmt)
    first, off = check_scene_is_what_the_tests_need(sc)
    want, winfo = pcv.las_encode_host(pts, **kw)
    truth_bytes, tinfo = WT.records(pts, fmt=fmt, scale=kw["scale"], offset=kw["offset"])
    assert want.tobytes() == truth_bytes  # (the twin is the truth here as well)
    nseg, length = batch.num_segments, LT.MIN_LEN[fmt]
    got, info = batch.las_records(**kw)  # the whole batch, host
    assert got.shape == want.shape == (batch.num_points, length) and got.tobytes() == want.tobytes()
    WT.assert_info(info, tinfo, "whole batch")
    sizes = set()
    for k in range(nseg):  # each single segment
        a, b = int(off[k]), int(off[k + 1])
        got, info = batch.las_records(first_segment=k, num_segments=1, **kw)
        sizes.add(b - a)
        assert got.tobytes() == want[a:b].tobytes(), k
        if k % 7 == 0 or b - a <= 1:
            WT.assert_info(info, pcv.las_encode_host(rows_of(pts, a, b), **kw)[1], f"segment {k}")
    assert {0, 1} <= sizes and max(sizes) > 64, sorted(sizes)  # segments with no kept point, with one, with more than a wave's lanes
    for start in range(min(17, nseg + 1) if sweep else 0):  # every range that starts at segments 0 .. 16, the empty one first
        for num in range(0, nseg - start + 1):
            got, info = batch.las_records(first_segment=start, num_segments=num, **kw)
            a, b = int(off[start]), int(off[start + num])
            assert got.shape == (b - a, length) and got.tobytes() == want[a:b].tobytes() and info["num_records"] == b - a, (start, num)
    for s in range(4):  # the four shapes; device memory
        got, info = batch.las_records(shape=s, device=True, **kw)
        a, b = int(off[first[s]]), int(off[first[s + 1]])
        assert tuple(got.shape) == (b - a, length) and got.cpu().numpy().tobytes() == want[a:b].tobytes(), s
        WT.assert_info(info, WT.records(rows_of(pts, a, b), fmt=fmt, scale=kw["scale"], offset=kw["offset"])[1], f"shape {s}")


@pytest.mark.parametrize("fmt", FORMATS)
def test_octree_records_equal_the_twin(octree_i, fmt):
    check_every_range(octree_i, fmt, sweep=True)


@pytest.mark.parametrize("fmt", [2, 7])
def test_octree_records_of_large_nodes(octree_big, fmt):
    check_every_range(octree_big, fmt, sweep=True)


@pytest.mark.parametrize("fmt", FORMATS)
def test_s2_records_equal_the_twin(s2_scene, fmt):
    check_every_range(s2_scene, fmt, sweep=True)


def test_format_auto_and_field_subsets(octree_i, s2_scene):
    _, info = octree_i["batch"].las_records(shape=3, **OCTREE_KW)
    assert (info["point_format"], info["version_minor"], info["skipped_extras"]) == (2, 2, 0)
    kw = s2_scene["kw"]
    got, info = s2_scene["batch"].las_records(shape=1, **kw)
    want, winfo = pcv.las_encode_host(s2_scene["las"], **kw)
    first, off = check_scene_is_what_the_tests_need(s2_scene)
    a, b = int(off[first[1]]), int(off[first[2]])
    assert (info["point_format"], info["version_minor"], info["skipped_extras"]) == (8, 4, 1) and got.tobytes() == want[a:b].tobytes()
    assert info["masked_values"] > 0 and info["clamped_intensity"] > 0
    fields = ["gps_time", "classification", "color"]
    got, info = s2_scene["batch"].las_records(shape=1, point_format=3, fields=fields, **kw)
    want, _ = pcv.las_encode_host(s2_scene["las"], point_format=3, fields=fields, **kw)
    truth, _ = WT.records(rows_of(s2_scene["las"], a, b), fmt=3, fields=fields, **kw)
    assert got.tobytes() == want[a:b].tobytes() == truth
    for bad, word in ((dict(fields=["nope"]), "Data type for attribute 'nope' not found."), (dict(fields=["nir"], point_format=3), "'nir'"),
                      (dict(fields=["beam_id"]), "'beam_id'"), (dict(point_format=4), "format 4"), (dict(version_minor=3), "1.3"),
                      (dict(point_format=6, version_minor=2), "1.4"), (dict(scale=0.0), "scale"), (dict(scale=float("nan")), "scale")):
        with pytest.raises(pcv.PcvError) as e:
            s2_scene["batch"].las_records(shape=1, **{**kw, **bad})
        assert e.value.code == pcv.PCV_E_INVALID and word in str(e.value), str(e.value)
    with pytest.raises(pcv.PcvError) as e:
        octree_i["batch"].las_records(fields=["gps_time"], point_format=3, **OCTREE_KW)
    assert str(e.value).endswith("Data type for attribute 'gps_time' not found.")
    with pytest.raises(pcv.PcvError) as e:
        octree_i["batch"].las_records(first_segment=0, num_segments=octree_i["batch"].num_segments + 1, **OCTREE_KW)
    assert "past the end" in str(e.value)


@pytest.mark.parametrize("kind", ["octree", "s2"])
def test_records_at_every_alignment_and_nothing_beside_them(ctx, octree_i, s2_scene, kind):
    """The output at every residue mod 16, record lengths 34 and 38 (octree: 26 and 30): head, interior and tail of every tile;
    the bytes before and after the records stay what they were."""
    import torch
    sc, fmts = (octree_i, (2, 6)) if kind == "octree" else (s2_scene, (3, 8))
    fn = ctx.lib.pcv_query_batch_las_records if kind == "octree" else ctx.lib.pcv_s2_query_las_records
    batch = sc["batch"]
    for fmt in fmts:
        kw = dict(sc["kw"], point_format=fmt)
        want, _ = pcv.las_encode_host(sc["las"], **kw)
        pr, _keep = pcv.las_write_params(**kw)
        nbytes = want.size
        for k in range(16):
            buf = torch.full((nbytes + 64,), 0xA5, dtype=torch.uint8, device=f"cuda:{ctx.device}")
            torch.cuda.synchronize()
            length, count, info = C.c_uint32(), C.c_uint64(), L.LasWriteInfo()
            ctx._check(fn(batch.handle, 0, batch.num_segments, C.byref(pr), nbytes, L.MEM_DEVICE, buf.data_ptr() + 16 + k, C.byref(length),
                          C.byref(count), C.byref(info)))
            host = buf.cpu().numpy()
            assert (length.value, count.value) == (want.shape[1], want.shape[0])
            assert host[16 + k:16 + k + nbytes].tobytes() == want.tobytes(), (fmt, k)
            assert np.all(host[:16 + k] == 0xA5) and np.all(host[16 + k + nbytes:] == 0xA5), (fmt, k)


def truth_file(points, header_kw=None, **kw):
    data, info = WT.records(points, fmt=kw.pop("point_format", WT.AUTO), **kw)
    return WT.header(info, **(header_kw or {})) + data, info


@pytest.mark.parametrize("kind", ["octree", "s2"])
def test_files_equal_header_and_records_whatever_the_pieces(ctx, octree_i, s2_scene, tmp_path, kind):
    sc, fmts = (octree_i, (3, 7)) if kind == "octree" else (s2_scene, (1, 8))
    batch, pts, kw = sc["batch"], sc["las"], sc["kw"]
    first, off = check_scene_is_what_the_tests_need(sc)
    for fmt in fmts:
        for shape in (0, 1):
            a, b = int(off[first[shape]]), int(off[first[shape + 1]])
            want, winfo = truth_file(rows_of(pts, a, b), point_format=fmt, **kw)
            infos = []
            for chunk in (1, 7, 64, 1000, 0) if (shape == 1 and fmt == fmts[0]) else (7, 1000, 0):
                path = tmp_path / f"{kind}_{shape}_{chunk}.las"
                info = batch.write_las(path, shape=shape, point_format=fmt, chunk_points=chunk, **kw)
                assert path.read_bytes() == want, (fmt, shape, chunk)
                WT.assert_info(info, winfo, f"{fmt} {shape} {chunk}")
                infos.append(info)
    # the header's own fields, and a file the project's reader accepts
    hk = dict(file_source_id=7, global_encoding=1, day=42, year=2031, system_identifier=b"scanner", generating_software=b"a test")
    path = tmp_path / "named.las"
    batch.write_las(path, shape=1, point_format=fmts[1], file_source_id=7, global_encoding=1, day=42, year=2031, system_identifier="scanner",
                    generating_software="a test", **kw)
    a, b = int(off[first[1]]), int(off[first[2]])
    assert path.read_bytes() == truth_file(rows_of(pts, a, b), header_kw=hk, point_format=fmts[1], **kw)[0]
    hdr = pcv.read_las_header(path, as_dict=True)
    assert hdr["num_points"] == b - a and hdr["point_format"] == fmts[1] and hdr["offset_to_points"] == hdr["header_size"]


def test_pipeline_memory_does_not_grow_with_the_result(ctx, octree_i, s2_scene, tmp_path):
    """chunk_points = 64: two record buffers of 64 records and the block of the header's sums, whatever the result holds."""
    for sc in (octree_i, s2_scene):
        peaks = []
        for shape in (1, 0):  # about half, then all: the larger result takes no more
            ctx.trim()
            live, _ = ctx.pool_stats(reset_peak=True)
            sc["batch"].write_las(tmp_path / "m.las", shape=shape, chunk_points=64, point_format=3, **sc["kw"])
            live_after, peak = ctx.pool_stats()
            assert live_after == live
            peaks.append(peak - live)
        assert peaks[0] == peaks[1] and 2 * (64 * 34 + 255) // 256 * 256 <= peaks[0] <= 2 * 2304 + 4096, peaks
    # a 4 x larger result at one chunk_points
    first, off = check_scene_is_what_the_tests_need(octree_i)
    small = next(k for k in range(octree_i["batch"].num_segments) if 64 < off[k + 1] - off[k] < N_OCTREE // 4)
    ctx.trim()
    live, _ = ctx.pool_stats(reset_peak=True)
    octree_i["batch"].write_las(tmp_path / "s.las", first_segment=small, num_segments=1, chunk_points=64, point_format=3, **OCTREE_KW)
    assert ctx.pool_stats()[1] - live == peaks[0]


@pytest.mark.parametrize("kind", ["octree", "s2"])
def test_auto_offset_and_out_of_range(ctx, octree_i, s2_scene, tmp_path, kind):
    sc = octree_i if kind == "octree" else s2_scene
    batch, pts = sc["batch"], sc["las"]
    first, off = check_scene_is_what_the_tests_need(sc)
    for shape in (0, 1, 3):
        a, b = int(off[first[shape]]), int(off[first[shape + 1]])
        part = rows_of(pts, a, b)
        want, winfo = truth_file(part, point_format=3, scale=0.001, offset=None)
        assert winfo["offset"] == tuple(float(np.floor(part[k].min())) for k in "xyz")
        got, info = batch.las_records(shape=shape, point_format=3)
        WT.assert_info(info, winfo, f"auto offset, shape {shape}")
        assert got.tobytes() == want[227:]
        path = tmp_path / f"auto_{shape}.las"
        WT.assert_info(batch.write_las(path, shape=shape, point_format=3, chunk_points=500), winfo, "file")
        assert path.read_bytes() == want
    _, info = batch.las_records(shape=2, point_format=3)  # a range without rows takes 0
    assert info["offset"] == (0.0, 0.0, 0.0) and info["num_records"] == 0 and info["bounds"] == (0.0,) * 6
    # an offset 3 000 km away at 1 mm: every point is out of range
    far = tuple(v + 3.0e6 for v in sc["kw"]["offset"])
    got, info = batch.las_records(shape=1, point_format=3, offset=far)
    a, b = int(off[first[1]]), int(off[first[2]])
    assert info["out_of_range"] == b - a and info["min_xyz"] == info["max_xyz"] == (0, 0, 0)
    assert got.tobytes() == WT.records(rows_of(pts, a, b), fmt=3, offset=far)[0]
    path = tmp_path / "far.las"
    with pytest.raises(pcv.PcvError) as e:
        batch.write_las(path, shape=1, point_format=3, offset=far, chunk_points=300)
    assert e.value.code == pcv.PCV_E_INVALID and f"{b - a} of {b - a} points are out of range" in str(e.value) and "2147483647" in str(e.value)
    assert not path.exists()
    # in append mode the old file (five records around that far offset, from the truth writer) stays byte for byte
    LT.write_las(path, 2, 3, LT.random_fields(3, 5, seed=2), scale=(0.001,) * 3, offset=far)
    before = path.read_bytes()
    assert pcv.las_append_check(path, dict(point_format=3, version_minor=2, scale=(0.001,) * 3, offset=far), offset=far) == 5
    with pytest.raises(pcv.PcvError) as e:
        batch.write_las(path, shape=1, point_format=3, offset=far, open_mode="append", chunk_points=300)
    assert e.value.code == pcv.PCV_E_INVALID and "out of range" in str(e.value) and path.read_bytes() == before


@pytest.mark.parametrize("kind", ["octree", "s2"])
def test_append(ctx, octree_i, s2_scene, tmp_path, kind):
    sc, fmt = (octree_i, 3) if kind == "octree" else (s2_scene, 8)
    batch, pts, kw = sc["batch"], sc["las"], dict(sc["kw"], point_format=fmt)
    nseg = batch.num_segments
    first, off = check_scene_is_what_the_tests_need(sc)
    s0, s1 = int(first[0]), int(first[1])
    mid = s0 + (s1 - s0) // 2
    whole, halves = tmp_path / "whole.las", tmp_path / "halves.las"
    winfo = batch.write_las(whole, shape=0, **kw)
    a = batch.write_las(halves, first_segment=s0, num_segments=mid - s0, open_mode="append", **kw)  # a missing file is written anew
    b = batch.write_las(halves, first_segment=mid, num_segments=s1 - mid, open_mode="append", chunk_points=333, **kw)
    assert a["num_records"] > 0 and b["num_records"] > 0 and a["num_records"] + b["num_records"] == winfo["num_records"]
    assert halves.read_bytes() == whole.read_bytes() == truth_file(rows_of(pts, int(off[s0]), int(off[s1])), **kw)[0]
    assert pcv.las_append_check(halves, winfo, **sc["kw"]) == winfo["num_records"]
    # auto offset is satisfied by the file's
    c = batch.write_las(halves, shape=3, open_mode="append", point_format=fmt)
    assert c["offset"] == winfo["offset"] and os.path.getsize(halves) == os.path.getsize(whole) + c["record_length"]
    before = halves.read_bytes()
    other = 2 if fmt == 3 else 7
    for bad, word in ((dict(kw, point_format=other), "format"), (dict(kw, scale=0.01), "scale"),
                      (dict(kw, offset=tuple(v + 1.0 for v in kw["offset"])), "offset")):
        with pytest.raises(pcv.PcvError) as e:
            batch.write_las(halves, shape=1, open_mode="append", **bad)
        assert e.value.code == pcv.PCV_E_INVALID and word in str(e.value) and halves.read_bytes() == before, str(e.value)
    if fmt == 3:
        with pytest.raises(pcv.PcvError) as e:
            batch.write_las(halves, shape=1, open_mode="append", **dict(kw, version_minor=4))
        assert "version" in str(e.value) and halves.read_bytes() == before
    # a file with a VLR, from the truth writer
    f = LT.random_fields(fmt, 5, seed=1)
    vlr = tmp_path / "vlr.las"
    LT.write_las(vlr, 2 if fmt <= 3 else 4, fmt, f, scale=(0.001,) * 3, offset=kw["offset"], offset_to_points=LT.HEADER_SIZE[2 if fmt <= 3 else 4] + 54)
    before = vlr.read_bytes()
    with pytest.raises(pcv.PcvError) as e:
        batch.write_las(vlr, shape=1, open_mode="append", **kw)
    assert "offset to point data" in str(e.value) and vlr.read_bytes() == before
    # an empty range appends nothing and writes no file
    assert batch.write_las(halves, shape=2, open_mode="append", **kw)["num_records"] == 0
    assert batch.write_las(tmp_path / "none.las", shape=2, **kw)["num_records"] == 0 and not (tmp_path / "none.las").exists()
    assert batch.write_las(whole, first_segment=nseg, num_segments=0, **kw)["num_records"] == 0 and whole.read_bytes() == truth_file(
        rows_of(pts, int(off[s0]), int(off[s1])), **kw)[0]


def survey_fields(fmt, n, seed):
    """Every field random, ECEF-sized at 1 mm around the offset, colours multiples of 257, gps specials with NaN payloads."""
    f = LT.random_fields(fmt, n, seed=seed)
    rng = np.random.default_rng(seed + 100)
    for k, span in (("X", 400_000), ("Y", 400_000), ("Z", 300_000)):
        f[k] = rng.integers(-span, span, n).astype(np.int32)
    for k in "rgb":
        f[k] = (rng.integers(0, 256, n) * 257).astype(np.uint16)
    return f


@pytest.mark.parametrize("fmt,minor", [(3, 2), (7, 4)])
def test_round_trip_through_the_reader(ctx, tmp_path, fmt, minor):
    """A file of the truth writer -> las_load with every extra -> s2_split -> query -> write_las with the file's format, scale
    and offset: the same multiset of records, the same counts, by-return counts and bounds; then a polygon that keeps about half."""
    n, scale, offset = 3001, (0.001,) * 3, (4_200_000.0, 170_000.0, 4_780_000.0)
    f = survey_fields(fmt, n, fmt)
    src = tmp_path / "src.las"
    data = LT.write_las(src, minor, fmt, f, scale=scale, offset=offset)
    stride = LT.MIN_LEN[fmt]
    records = np.frombuffer(data[LT.HEADER_SIZE[minor]:], np.uint8).reshape(n, stride)
    cloud = ctx.las_load(src, extras="all", keep_intensity=True, color="rgb16")
    s2 = ctx.s2_split(cloud.points, 16)
    kw = dict(point_format=fmt, version_minor=minor, scale=scale, offset=offset)

    def sorted_rows(rows):
        return sorted(bytes(r) for r in rows)

    batch = s2.query_batch(ctx.shapes([("all",)]))
    out = tmp_path / "out.las"
    info = batch.write_las(out, **kw)
    got = out.read_bytes()
    assert info["num_records"] == n and info["out_of_range"] == 0 and info["masked_values"] == 0 and info["clamped_intensity"] == 0
    assert sorted_rows(np.frombuffer(got[LT.HEADER_SIZE[minor]:], np.uint8).reshape(n, stride)) == sorted_rows(records)

    def expected_header(keep):
        by_return = np.zeros(15, np.uint64)
        for r in range(1, 16):
            by_return[r - 1] = int((f["return_number"][keep] == r).sum())
        ext = [(int(f[k][keep].min()), int(f[k][keep].max())) for k in "XYZ"]
        bounds = []
        for a in range(3):
            bounds += [np.float64(ext[a][1]) * scale[a] + offset[a], np.float64(ext[a][0]) * scale[a] + offset[a]]
        return WT.header(dict(version_minor=minor, point_format=fmt, num_records=int(keep.sum()), by_return=by_return, scale=scale, offset=offset,
                              bounds=tuple(float(b) for b in bounds)))

    assert got[:LT.HEADER_SIZE[minor]] == expected_header(np.ones(n, bool))
    batch.free()
    # a web-mercator polygon over about half of the points: a rectangle in (u, v) whose right edge lies in the widest gap between
    # neighbouring u near the median, so that no point is within rounding of the edge (positions by the reader's formula)
    x, y, z = (f[k].astype(np.float64) * scale[a] + offset[a] for a, k in enumerate("XYZ"))
    u, v = pcv.wmr_project(x, y, z)
    su = np.sort(u)
    mid = n // 2 - 100 + int(np.argmax(np.diff(su[n // 2 - 100:n // 2 + 100])))
    cut, pad = float((su[mid] + su[mid + 1]) / 2), 1e-6
    assert su[mid + 1] - su[mid] > 1e-12
    ring = np.array([[u.min() - pad, v.min() - pad], [cut, v.min() - pad], [cut, v.max() + pad], [u.min() - pad, v.max() + pad]])
    batch = s2.query_batch(ctx.shapes([("polygon_web_mercator", [ring])]))
    keep = u < cut
    info = batch.write_las(out, chunk_points=700, **kw)
    got = out.read_bytes()
    assert 0.3 * n < info["num_records"] == int(keep.sum()) < 0.7 * n
    assert sorted_rows(np.frombuffer(got[LT.HEADER_SIZE[minor]:], np.uint8).reshape(-1, stride)) == sorted_rows(records[keep])
    assert got[:LT.HEADER_SIZE[minor]] == expected_header(keep)
    batch.free()
    s2.free()
    cloud.free()


def test_read_las_of_an_octree_file(ctx, octree_i, tmp_path):
    sc = octree_i
    path = tmp_path / "tree.las"
    info = sc["batch"].write_las(path, shape=0, point_format=2, intensity_scale=100.0, **OCTREE_KW)
    pts = rows_of(sc["las"], 0, N_OCTREE)
    back = pcv.read_las(path, keep_intensity=True, color="rgb16")
    assert info["num_records"] == N_OCTREE == len(back["x"]) and back["info"]["num_records"] == N_OCTREE
    s = 0.001
    for k, o in zip("xyz", OCTREE_KW["offset"]):
        bound = s / 2 + 4 * np.spacing(np.maximum(np.abs(pts[k]), abs(o)))  # four operations, each rounded once
        assert np.all(np.abs(back[k] - pts[k]) <= bound), k
    assert back["color"].tobytes() == pts["color"].tobytes()
    codes, clamped = WT.intensity_u16(pts["intensity"], 100.0)
    assert back["intensity"].tobytes() == codes.astype(np.float32).tobytes() and info["clamped_intensity"] == int(clamped.sum()) > 0


def test_bytes_do_not_depend_on_what_the_pool_hands_out(tmp_path):
    """Under the pool guard with two fills: identical records and files, no fence damaged."""
    results = []
    for fill in (0x00, 0x4B):
        ctx = pcv.Context(0)
        try:
            ctx.set_pool_guard(2, fill)
            sc = octree_scene(ctx, True, 120)
            rec, info = sc["batch"].las_records(shape=1, point_format=3)  # with the min pass
            path = tmp_path / f"guard_{fill}.las"
            sc["batch"].write_las(path, shape=0, point_format=7, chunk_points=777, **OCTREE_KW)
            results.append((rec.tobytes(), path.read_bytes(), info["offset"]))
            sc["batch"].free()
            sc["tree"].free()
            rep = ctx.pool_guard_report()
            assert rep["damaged"] == 0 and rep["checked"] > 0, rep
        finally:
            ctx.close()
    assert results[0] == results[1]


def test_one_file_per_location(ctx, octree_i, tmp_path):
    sc = octree_i
    batch = sc["batch"]
    first, off = check_scene_is_what_the_tests_need(sc)
    written = batch.write_las_per_location(str(tmp_path / "loc_{}.las"), point_format=2, **OCTREE_KW)
    assert sorted(written) == [0, 1, 3] and sorted(os.listdir(tmp_path)) == ["loc_0.las", "loc_1.las", "loc_3.las"]
    for s in written:
        a, b = int(off[first[s]]), int(off[first[s + 1]])
        assert (tmp_path / f"loc_{s}.las").read_bytes() == truth_file(rows_of(sc["las"], a, b), point_format=2, **OCTREE_KW)[0], s


def run_example(args):
    import subprocess
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "examples"), "bin/query_to_las"])
    return subprocess.run([os.path.join(ROOT, "examples", "bin", "query_to_las")] + [str(a) for a in args], capture_output=True, text=True)


def test_example_over_an_octree_directory(ctx, octree_i, tmp_path):
    """examples/query_to_las.c over the written octree: one box with auto offset, then the same appended, against the Python call."""
    sc = octree_i
    sc["tree"].write_dir(tmp_path / "tree")
    lo, hi = sc["bmin"] - 1.0, np.array([np.median(sc["points"]["x"][:N_OCTREE]), sc["bmax"][1] + 1.0, sc["bmax"][2] + 1.0])
    batch = sc["tree"].query_batch(ctx.shapes([("aabb", lo, hi)]))
    assert 0.3 * N_OCTREE < batch.num_points < 0.7 * N_OCTREE
    want = tmp_path / "want.las"
    info = batch.write_las(want, point_format=3, scale=0.01)
    box = ",".join(repr(float(v)) for v in list(lo) + list(hi))
    args = [tmp_path / "tree", "--aabb", box, "--format", "3", "--scale", "0.01", "--output", tmp_path / "got.las", "--info"]
    p = run_example(args)
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "got.las").read_bytes() == want.read_bytes()
    assert f"{info['num_records']} records" in p.stdout and "format 3" in p.stdout
    p = run_example(args + ["--append", "--per-location", tmp_path / "loc_%u.las"])
    assert p.returncode == 0, p.stderr
    batch.write_las(want, point_format=3, scale=0.01, open_mode="append")
    assert (tmp_path / "got.las").read_bytes() == want.read_bytes() and os.path.getsize(want) == 227 + 2 * 34 * info["num_records"]
    batch.write_las(want, point_format=3, scale=0.01)
    assert (tmp_path / "loc_0.las").read_bytes() == want.read_bytes()  # (append to no file writes it anew)
    p = run_example([tmp_path / "tree", "--all", "--fields", "gps_time", "--output", tmp_path / "no.las"])
    assert p.returncode == 1 and "'gps_time' not found" in p.stderr and not (tmp_path / "no.las").exists()
    batch.free()


def test_example_over_an_s2_directory(ctx, s2_scene, tmp_path):
    """The same over the written S2 cloud: every point with a given offset and chosen fields, then the map tiles of zoom 19."""
    cloud, kw = s2_scene["cloud"], s2_scene["kw"]
    cloud.write(tmp_path / "cloud")
    batch = cloud.query_batch(ctx.shapes([("all",)]))
    want = tmp_path / "want.las"
    fields = ["color", "gps_time", "classification", "return_number"]
    batch.write_las(want, point_format=7, fields=fields, **kw)
    offset = ",".join(repr(float(v)) for v in kw["offset"])
    p = run_example([tmp_path / "cloud", "--all", "--format", "7", "--offset", offset, "--fields", ",".join(fields), "--output", tmp_path / "got.las"])
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "got.las").read_bytes() == want.read_bytes()
    batch.free()
    p = run_example([tmp_path / "cloud", "--map-tiles", "19", "--output", tmp_path / "tiles.las", "--per-location", tmp_path / "tile_%u.las"])
    assert p.returncode == 0, p.stderr
    lo, hi = cloud.bbox_min, cloud.bbox_max
    corners = np.array([[(hi if k & 1 else lo)[0], (hi if k & 2 else lo)[1], (hi if k & 4 else lo)[2]] for k in range(8)])
    u, v = pcv.wmr_project(corners[:, 0], corners[:, 1], corners[:, 2])
    tx, ty = np.floor(u * 2 ** 19).astype(np.int64), np.floor(v * 2 ** 19).astype(np.int64)
    tiles = [pcv.web_mercator_rect_from_zoomed((256 * x, 256 * y), (256 * (x + 1), 256 * (y + 1)), 19)
             for y in range(ty.min(), ty.max() + 1) for x in range(tx.min(), tx.max() + 1)]
    batch = cloud.query_batch(ctx.shapes(tiles))
    first, _, off = batch.segments()
    assert len(tiles) >= 2 and batch.num_points > N_S2 // 2
    batch.write_las(want)  # format 8 by AUTO, auto offset
    assert (tmp_path / "tiles.las").read_bytes() == want.read_bytes()
    nonempty = [k for k in range(len(tiles)) if off[first[k + 1]] > off[first[k]]]
    assert sorted(f for f in os.listdir(tmp_path) if f.startswith("tile_")) == sorted(f"tile_{k}.las" for k in nonempty)
    for k in nonempty[:3]:
        batch.write_las(want, shape=k)
        assert (tmp_path / f"tile_{k}.las").read_bytes() == want.read_bytes(), k
    batch.free()
