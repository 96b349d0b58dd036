"""LAS input on the device (csrc/pcv_las.hip). The truth is the host twin (pcv_las_decode_host, read_las), which
tests/test_las_cpu.py pins against a numpy truth and hand-typed files; the device's outputs equal it byte for byte in every
case: sizes around the wave and the tile, pieces that cut inside them, every format at strides that move a tile's first byte
through the residues modulo 16, the filter's corner cases, the colour rules, the transform, the file path and what is built
downstream from a LasCloud."""
import filecmp
import os

import numpy as np
import pytest

import las_truth as T
import point_cloud_viewer_amd as pcv
from point_cloud_viewer_amd import _lib as L

pytestmark = pytest.mark.gpu
SCALE, OFFSET = (0.001, 0.01, 1e-7), (4.5e6, -4.5e6, 12.5)


@pytest.fixture(scope="module")
def ctx():
    c = pcv.Context(0)
    yield c
    c.close()


def header(fmt, stride, n):
    minor = 4 if fmt >= 6 else 2
    return dict(version=(1, minor), point_format=fmt, header_size=T.HEADER_SIZE[minor], record_length=stride,
                offset_to_points=T.HEADER_SIZE[minor], num_points=n, scale=SCALE, offset=OFFSET)


_fields = {}


def fields(fmt, n, seed=0):
    key = (fmt, n, seed)
    if key not in _fields:
        _fields[key] = T.random_fields(fmt, n, seed=seed + 100 * fmt + n)
    return {k: v.copy() for k, v in _fields[key].items()}


def check(ctx, fmt, raw, n, extra=0, pieces=(0,), device=False, skew=0, want=None, **kw):
    """las_decode of the records against the host twin, for every piece size; returns the twin's result."""
    hdr = header(fmt, T.MIN_LEN[fmt] + extra, n)
    want = pcv.las_decode_host(hdr, raw, **kw) if want is None else want
    src = np.frombuffer(raw, dtype=np.uint8)
    if device:
        import torch
        buf = torch.zeros(src.size + 32, dtype=torch.uint8, device=f"cuda:{ctx.device}")
        buf[skew:skew + src.size] = torch.from_numpy(src.copy())
        src = buf[skew:skew + src.size]
    for pp in pieces:
        got = ctx.las_decode(hdr, src, n=n, piece_points=pp, **kw)
        T.assert_same(got, want, f"format {fmt} +{extra} n={n} piece_points={pp} device={device} skew={skew}")
        most = (32 << 20) // hdr["record_length"] // 256 * 256
        assert got["info"]["num_pieces"] == (0 if n == 0 else -(-n // (pp if 0 < pp <= most else most)))
    return want


# ---- stage entry: sizes and cuts ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 1000])
def test_sizes_and_piece_cuts(ctx, n):
    for fmt in (3, 7):
        f = fields(fmt, n)
        raw = T.pack_records(fmt, f, 1)
        check(ctx, fmt, raw, n, extra=1, pieces=(1, 64, 100, 0), extras=T.extras_of(fmt), keep_intensity=True)
        check(ctx, fmt, raw, n, extra=1, pieces=(1, 64, 100, 0), classes=[1, 2, 3, 5, 8, 13, 21, 200], drop_withheld=True, extras=["gps_time"])


@pytest.mark.parametrize("fmt", range(11))
def test_formats_strides_and_memories(ctx, fmt):
    n = 700  # three tiles, the last one ragged
    f = fields(fmt, n)
    for extra in (0, 1, 3, 7):
        raw = T.pack_records(fmt, f, extra)
        kw = dict(extras=T.extras_of(fmt), keep_intensity=True, classes=list(range(0, 256, 2)) if extra == 3 else None)
        want = check(ctx, fmt, raw, n, extra=extra, pieces=(100, 0), **kw)
        # device memory at an odd address: pieces of 77 records start at every residue the stride allows
        check(ctx, fmt, raw, n, extra=extra, pieces=(77, 0), device=True, skew=1 + 2 * extra, want=want, **kw)


def test_every_residue_modulo_16(ctx):
    n, fmt = 300, 7
    raw = T.pack_records(fmt, fields(fmt, n), 1)  # stride 37
    want = None
    for skew in range(16):
        want = check(ctx, fmt, raw, n, extra=1, pieces=(0,), device=True, skew=skew, want=want, extras=["gps_time", "scan_angle"])


def test_records_too_long_for_the_tile_in_lds(ctx):
    n = 600
    for fmt, extra in ((1, 224 - 28), (1, 225 - 28), (6, 1000)):  # the last staged stride, the first direct one, a long one
        raw = T.pack_records(fmt, fields(fmt, n), extra)
        want = check(ctx, fmt, raw, n, extra=extra, pieces=(100, 0), extras=T.extras_of(fmt), classes=[0, 1, 2, 3, 4, 5, 6, 7])
        check(ctx, fmt, raw, n, extra=extra, pieces=(0,), device=True, skew=5, want=want, extras=T.extras_of(fmt), classes=[0, 1, 2, 3, 4, 5, 6, 7])


# ---- filter -----------------------------------------------------------------------------------------------------------------------
def test_filter_corner_cases_and_counts(ctx):
    n, fmt, pieces = 1000, 6, (64, 100, 256, 0)
    f = fields(fmt, n)
    cases = {"nothing": np.full(n, 9), "all": np.full(n, 2), "alternating": np.where(np.arange(n) % 2, 2, 9),
             "last of a piece": np.where(np.arange(n) % 100 == 99, 2, 9), "first of a piece": np.where(np.arange(n) % 100 == 0, 2, 9)}
    for name, cls in cases.items():
        f["classification"][:] = cls
        raw = T.pack_records(fmt, f)
        want = check(ctx, fmt, raw, n, pieces=pieces, classes=[2], extras=["classification", "return_number"], keep_intensity=True)
        assert want["info"]["num_kept"] == int((cls == 2).sum()), name
        check(ctx, fmt, raw, n, pieces=pieces, classes=[2], drop_withheld=True, extras=["classification_flags"])
        check(ctx, fmt, raw, n, pieces=pieces, drop_withheld=True)
    # every record of one class: the hot bin of the histogram
    f["classification"][:] = 2
    f["return_number"][:] = 1
    want = check(ctx, fmt, T.pack_records(fmt, f), n, pieces=pieces)
    assert want["info"]["class_hist"][2] == n and want["info"]["return_hist"][1] == n and want["info"]["class_hist"].sum() == n


# ---- colour -----------------------------------------------------------------------------------------------------------------------
def test_colour_modes(ctx):
    n = 500
    f = fields(3, n)
    raw = T.pack_records(3, f)
    for color in ("auto", "rgb16", "rgb8", "intensity", (1, 2, 3)):
        want = check(ctx, 3, raw, n, pieces=(100, 0), color=color, classes=list(range(16)))
        assert want["info"]["color_rule"] == (color if isinstance(color, str) and color != "auto" else "rgb16" if color == "auto" else "constant")
    # AUTO on both sides of 255 / 256: the deciding record is the last one, in the last piece, and dropped
    for top, rule in ((255, "rgb8"), (256, "rgb16")):
        f["r"][:], f["g"][:], f["b"][:] = f["r"] % 256, f["g"] % 255, f["b"] % 200
        f["classification"][:] = 2
        f["classification"][-1], f["b"][-1] = 7, top
        want = check(ctx, 3, T.pack_records(3, f), n, pieces=(100, 0), classes=[2])
        assert want["info"]["color_rule"] == rule and want["info"]["max_color"] == top and want["info"]["num_kept"] == n - 1
    f0 = fields(0, n)
    spread = f0["intensity"].astype(np.uint32)
    for imax in (0, 1, 65535):
        f0["intensity"][:] = spread % (imax + 1)
        f0["intensity"][-1] = imax
        want = check(ctx, 0, T.pack_records(0, f0), n, pieces=(100, 0))
        assert want["info"]["color_rule"] == "intensity" and want["info"]["max_intensity"] == imax
    with pytest.raises(pcv.PcvError) as e:
        ctx.las_decode(header(1, 28, 1), np.zeros(28, np.uint8), color="rgb16")
    assert e.value.code == L.PCV_E_INVALID and "RGB16" in str(e.value)


# ---- the file path ------------------------------------------------------------------------------------------------------------------
def test_transform_equals_transform_points(ctx, tmp_path):
    n = 5000
    T.write_las(tmp_path / "t.las", 2, 3, fields(3, n), scale=SCALE, offset=OFFSET)
    iso = (6.3e6, -1.2e5, 4.4e6, 0.1, -0.2, 0.3, float(np.sqrt(1 - 0.14)))
    plain, moved = ctx.las_load(tmp_path / "t.las"), ctx.las_load(tmp_path / "t.las", global_from_local=iso, piece_points=999)
    want = ctx.transform_points(iso, plain.read("x"), plain.read("y"), plain.read("z"))
    for k, w in zip("xyz", want):
        assert T.same_bits(moved.read(k), w), k
    T.assert_same(moved.to_host(), pcv.read_las(tmp_path / "t.las", global_from_local=iso), "transform against the host reader")
    plain.free(), moved.free()


def test_load_odd_headers_and_offsets(ctx, tmp_path):
    for minor, fmt, hs, gap, extra in ((0, 0, 227, 0, 0), (2, 2, 229, 1, 1), (3, 5, 241, 54 + 13, 3), (4, 8, 375, 0, 0), (4, 10, 381, 777, 7)):
        n = 3000
        p = tmp_path / f"o{minor}{fmt}.las"
        T.write_las(p, minor, fmt, fields(fmt, n), extra_bytes=extra, header_size=hs, offset_to_points=hs + gap, tail=b"\xee" * 61,
                    scale=SCALE, offset=OFFSET)
        for kw in (dict(extras="all", keep_intensity=True), dict(classes=[2, 3, 4, 5, 6], drop_withheld=True, piece_points=1000)):
            cloud = ctx.las_load(p, **kw)
            T.assert_same(cloud.to_host(), pcv.read_las(p, **kw), f"{p.name} {kw}")
            cloud.free()


def test_large_file_against_the_host_reader(ctx, tmp_path):
    n = 1_200_001  # 44 MB of format 7 at stride 37: more than one staging chunk, cut at an odd byte
    f = T.random_fields(7, n, seed=5)
    p = tmp_path / "big.las"
    T.write_las(p, 4, 7, f, extra_bytes=1, scale=SCALE, offset=OFFSET)
    kw = dict(extras=["gps_time", "classification", "return_number"], keep_intensity=True, classes=list(range(0, 256, 3)), drop_withheld=True)
    cloud = ctx.las_load(p, **kw)
    assert cloud.info["num_pieces"] == 2
    T.assert_same(cloud.to_host(), pcv.read_las(p, **kw), "1 200 001 records")
    cloud.free()


def test_raw_bytes_on_the_device_are_bounded_by_pieces(ctx, tmp_path):
    """Peak pool bytes of a piece_points = 4 096 load: the outputs (sized for every record), the parked 16-bit colours of the
    AUTO rule, PCV_LAS_RAW_PIECES raw pieces, and less than 64 KiB of statistics and tile tables; the part on top of the outputs
    is the same for twice the records."""
    stride, pp, over = 34, 4096, []

    def r256(nbytes):  # the pool hands out multiples of 256 bytes
        return (nbytes + 255) // 256 * 256

    for n in (100_000, 200_000):
        p = tmp_path / f"pool{n}.las"
        T.write_las(p, 2, 3, T.random_fields(3, n, seed=6), scale=SCALE, offset=OFFSET)
        ctx.trim()
        live0, _ = ctx.pool_stats(reset_peak=True)
        cloud = ctx.las_load(p, piece_points=pp, keep_intensity=True, extras=["gps_time"])
        live1, peak = ctx.pool_stats()
        outputs = 4 * r256(8 * n) + r256(3 * n) + r256(4 * n)  # x, y, z, gps_time; colour; intensity
        assert cloud.info["num_pieces"] == -(-n // pp) and live1 - live0 == outputs
        over.append(peak - live0 - outputs - r256(6 * n))  # 6 n: the parked r g b
        assert L.LAS_RAW_PIECES * pp * stride <= over[-1] <= L.LAS_RAW_PIECES * pp * stride + (64 << 10), over
        cloud.free()
    assert over[0] == over[1]


def test_truncated_file_is_io_and_the_context_lives_on(ctx, tmp_path):
    n = 50_000
    f = fields(1, n)
    data = T.write_las(tmp_path / "whole.las", 2, 1, f, scale=SCALE, offset=OFFSET)
    (tmp_path / "cut.las").write_bytes(data[:-1000])
    with pytest.raises(pcv.PcvError) as e:
        ctx.las_load(tmp_path / "cut.las")
    assert e.value.code == L.PCV_E_IO
    cloud = ctx.las_load(tmp_path / "whole.las", piece_points=7000)
    T.assert_same(cloud.to_host(), pcv.read_las(tmp_path / "whole.las"), "after a refused load")
    cloud.free()


# ---- downstream, 20 000 points -----------------------------------------------------------------------------------------------------
ECEF = (6.37e6, 1.0e4, -2.0e4, 0.0, 0.0, 0.0, 1.0)  # inside the radii S2 clouds accept


@pytest.fixture(scope="module")
def survey(tmp_path_factory):
    n = 20_000
    rng = np.random.default_rng(77)
    f = T.random_fields(7, n, seed=8)
    f["X"], f["Y"], f["Z"] = (rng.integers(-40_000, 40_000, n).astype(np.int32) for _ in range(3))  # an 80 m cube at millimetres
    p = tmp_path_factory.mktemp("las") / "survey.las"
    T.write_las(p, 4, 7, f, scale=(0.001,) * 3, offset=(100.0, 200.0, 50.0))
    return p


def _same_dirs(a, b):
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b)) and len(names) > 3
    _, mismatch, errors = filecmp.cmpfiles(a, b, names, shallow=False)
    assert not mismatch and not errors, (mismatch, errors)


def test_octree_from_a_las_file(ctx, survey, tmp_path):
    tree = pcv.build_octree_from_file(str(tmp_path / "dev"), 0.001, str(survey), ctx=ctx, classes=list(range(0, 256, 2)))
    host = pcv.read_las(survey, keep_intensity=True, classes=list(range(0, 256, 2)))
    assert tree.num_points == host["info"]["num_kept"] < 20_000
    pcv.build_octree(str(tmp_path / "host"), 0.001, None, {k: host[k] for k in ("x", "y", "z", "color", "intensity")}, ("color", "intensity"), ctx)
    _same_dirs(tmp_path / "dev", tmp_path / "host")
    tree.free()
    with pytest.raises(TypeError):
        pcv.build_octree_from_file(str(tmp_path / "no"), 0.001, os.path.join(os.path.dirname(__file__), "golden", "missing.ply"), classes=[2])


def test_s2_split_of_a_las_cloud(ctx, survey):
    kw = dict(extras=["gps_time", "classification", "return_number"], global_from_local=ECEF, keep_intensity=True)
    cloud, host = ctx.las_load(survey, **kw), pcv.read_las(survey, **kw)
    a, b = ctx.s2_split(cloud.points, 20), ctx.s2_split(host, 20)
    assert all(np.array_equal(u, v) for u, v in zip(a.cells, b.cells)) and a.num_cells > 1
    for u, v in zip(a.cell_points(), b.cell_points()):
        assert T.same_bits(u, v)
    for name in kw["extras"]:
        assert T.same_bits(a.cell_attribute(name), b.cell_attribute(name)), name
    a.free(), b.free(), cloud.free()


def test_terrain_and_map_tiles_from_a_las_cloud(ctx, survey):
    cloud, host = ctx.las_load(survey, drop_withheld=True), pcv.read_las(survey, drop_withheld=True)
    p = cloud.points
    lo, hi = [host[k].min() - 1 for k in "xyz"], [host[k].max() + 1 for k in "xyz"]
    a = ctx.terrain_begin(lo, hi, tile_size=64, resolution_m=0.5).add_points(p["x"], p["y"], p["z"], p["color"])
    b = ctx.terrain_begin(lo, hi, tile_size=64, resolution_m=0.5).add_points(host["x"], host["y"], host["z"], host["color"])
    a.finish(), b.finish()
    assert np.array_equal(a.tiles(), b.tiles()) and len(a.tiles()) > 1
    assert T.same_bits(a.heights(), b.heights()) and T.same_bits(a.colors(), b.colors())
    a.free(), b.free(), cloud.free()
    cloud, host = ctx.las_load(survey, global_from_local=ECEF), pcv.read_las(survey, global_from_local=ECEF)
    p = cloud.points
    a = ctx.map_tiles_begin(21).add_points(p["x"], p["y"], p["z"], p["color"])
    b = ctx.map_tiles_begin(21).add_points(host["x"], host["y"], host["z"], host["color"])
    a.finish(), b.finish()
    assert np.array_equal(a.tiles(), b.tiles()) and len(a.tiles()) >= 1
    assert np.array_equal(a.images(), b.images()) and np.array_equal(a.counts(), b.counts())
    a.free(), b.free(), cloud.free()
