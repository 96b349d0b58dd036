"""pcv_xray_run_s2_ex — xray over S2 cell clouds with filters and binning on any scalar attribute — against
xray_attr_oracle: the created set, kept / drawn / negative and every tile's RGBA, byte for byte, for every created tile.
The scene is test_gpu_xray_s2's (20 000 ECEF points, 64 px tiles at 0.5 m with the local transform, split at level 20 and at
level 16) with extras: `timestamp` (I64; U64 in the second cloud), `ring` (U8, from the local east), `weight` (F64 with a
NaN and an inf), columns of the other widths, and `normal` (F64Vec3)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import oracle_lib as O
import point_cloud_viewer_amd as pcv
import xray_attr_oracle as A
import xray_s2_oracle as S
from test_gpu_xray_merge import assert_same_quadtree
from test_gpu_xray_s2 import CORNERS, ISO, PX, W, cloud_points, corners_of, intensity_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = 30000000000.0  # the reference's own example: timestamp=30000000000
I64_MIN, I64_MAX = np.iinfo(np.int64).min, np.iinfo(np.int64).max
RING = (10, 17)  # local east -48 m ..< 16 m: whole columns of 32 m tiles lose every point


def columns(x, y, z, unsigned_timestamp=False):
    n = x.size
    i = np.arange(n, dtype=np.int64)
    east = O.iso_transform_points(ISO, x, y, z)[0]
    h = (i * 2654435761) % 1000003
    ts = ((h % 7) - 3) * 30000000000 + (i % 1000) * 1000000  # seven slices of 30 s, three of them negative
    ts[[5, 6, 7, 8, 9, 10]] = [2 ** 53 + 1, 2 ** 53 - 1, 2 ** 53 + 3, 2 ** 63 - 1, I64_MIN, -(2 ** 53) - 1]
    if unsigned_timestamp:  # the U64 twin: the same slices from 0, and the edges only a U64 has
        ts = (ts - ts[11:].min()).astype(np.uint64)
        ts[[5, 6, 7, 8, 9, 10]] = np.array([2 ** 53 + 1, 2 ** 63 - 1, 2 ** 63, 2 ** 64 - 1, 2 ** 63 - 513, 2 ** 53 + 3], dtype=np.uint64)
    weight = (h % 997).astype(np.float64) * 0.01 - 2.0
    weight[[3, 4, 12]] = [np.nan, np.inf, -np.inf]
    normal = np.stack([np.cos(i * 0.1), np.sin(i * 0.1), (i % 5) * 0.25], axis=1)
    return {"timestamp": ts, "ring": np.clip(np.floor((east + 128.0) / 8.0), 0, 255).astype(np.uint8), "weight": weight,
            "w_u8": (h % 251).astype(np.uint8), "w_u16": (h % 50000).astype(np.uint16), "w_i32": ((h % 2001) - 1000).astype(np.int32) * 1000,
            "w_f32": ((h % 613).astype(np.float32) - np.float32(300.0)) * np.float32(0.37), "normal": normal}


def make(ctx, level, shift_east=0.0, unsigned_timestamp=False):
    x, y, z, rgb = cloud_points(shift_east)
    inten = intensity_of(x.size)
    cols = columns(x, y, z, unsigned_timestamp)
    cloud = ctx.s2_split(dict(x=x, y=y, z=z, color=rgb, intensity=inten, attributes=cols), level)
    return cloud, A.AttrPoints(x, y, z, rgb, inten, level, cols, corners_of)


def prepare(ctx, sps):
    """the leaf tiles' shapes on the device, their corners into CORNERS: the oracle lists cells from the device's corners"""
    g = S.geometry(sps, W, PX, ISO)
    shapes = S.tile_shapes(g, ISO)
    sh = ctx.shapes([S.shape_spec(k, p) for k, p in shapes])
    for i, (k, p) in enumerate(shapes):
        CORNERS[(int(k), tuple(float(v) for v in p))] = sh.get(i)[0]
    return g, sh


@pytest.fixture(scope="module")
def ctx():
    c = pcv.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def scene(ctx):
    out = {}
    for level in (20, 16):
        cloud, sp = make(ctx, level)
        assert cloud.num_cells == (675 if level == 20 else 5)
        assert cloud.attributes == {"timestamp": "i64", "ring": "u8", "weight": "f64", "w_u8": "u8", "w_u16": "u16", "w_i32": "i32", "w_f32": "f32",
                                    "normal": "f64vec3"}
        out[level] = (cloud, sp, prepare(ctx, [sp]))
    return out


def run(ctx, clouds, strategy, **kw):
    xt = ctx.xray_tiles(clouds, W, PX, strategy, query_from_global=ISO, **kw)
    imgs = xt.images() if xt.num_created else np.zeros((0, W, W, 4), np.uint8)
    return xt, {n: imgs[i] for i, n in enumerate(xt.created_ids)}


def check(xt, got, want, g):
    """want: {leaf id: (image, drawn, negative, kept)}: every created tile, every pixel"""
    assert xt.leaf_ids == g["leaf_ids"] and xt.deepest_level == g["deepest_level"] and tuple(xt.bounding_rect) == g["rect"]
    assert xt.created_ids == [n for n in g["leaf_ids"] if n in want]
    assert [int(k) for k in xt.kept] == [want[n][3] for n in xt.created_ids]
    assert [int(k) for k in xt.drawn] == [want[n][1] for n in xt.created_ids]
    assert [int(k) for k in xt.negative] == [want[n][2] for n in xt.created_ids]
    for n in xt.created_ids:
        assert np.array_equal(got[n], want[n][0]), (n, int((got[n] != want[n][0]).any(-1).sum()))


def differ(a, b):
    return any(not np.array_equal(a[n], b[n]) for n in a)


# ---- 1. binning on an extra ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [20, 16])
def test_binning_on_timestamp(ctx, scene, level):
    cloud, sp, (g, _) = scene[level]
    for strategy, kw, okw in (("colored", {}, {}), ("colored_with_intensity", dict(min_intensity=1.0, max_intensity=200.0), dict(lo=1.0, hi=200.0))):
        xt, got = run(ctx, [cloud], strategy, background="transparent", binning=("timestamp", BIN), **kw)
        want, _, _ = A.tiles([sp], W, PX, strategy, ("timestamp", BIN), background="transparent", iso=ISO, **okw)
        assert len(want) == 64
        check(xt, got, want, g)
        assert (int(xt.negative.sum()) > 0) == (strategy == "colored_with_intensity")
        # a run that ignored the column, or read the intensity in its place, would not pass
        _, plain = run(ctx, [cloud], strategy, background="transparent", **kw)
        _, by_intensity = run(ctx, [cloud], strategy, background="transparent", binning=("intensity", 16.0), **kw)
        assert differ(got, plain) and differ(got, by_intensity)
    # the S2Cloud's own method, and bins of one nanosecond: (2^53 + 1 and 2^53 - 1 and 2^53 + 3 are bins of their own or not
    # as the conversion rounds)
    own = cloud.xray_tiles(W, PX, "colored", query_from_global=ISO, background="transparent", binning=("timestamp", 1.0))
    want, _, _ = A.tiles([sp], W, PX, "colored", ("timestamp", 1.0), background="transparent", iso=ISO)
    check(own, {n: img for n, img in zip(own.created_ids, own.images())}, want, g)
    # xray and height_stddev never read the binning
    for strategy in ("xray", ("height_stddev", 1.5, "jet")):
        xa, ga = run(ctx, [cloud], strategy, binning=("timestamp", BIN))
        xb, gb = run(ctx, [cloud], strategy)
        assert xa.created_ids == xb.created_ids and np.array_equal(xa.kept, xb.kept) and np.array_equal(xa.drawn, xb.drawn)
        assert np.array_equal(xa.images(), xb.images())


# ---- 2. every element width --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,size", [("w_u8", 30.0), ("w_u16", 1000.0), ("w_i32", 250000.0), ("w_f32", 7.5), ("weight", 0.75)])
def test_every_element_width(ctx, scene, name, size):
    cloud, sp, (g, _) = scene[16]
    xt, got = run(ctx, [cloud], "colored", binning=(name, size))
    want, _, kept = A.tiles([sp], W, PX, "colored", (name, size), iso=ISO)
    check(xt, got, want, g)
    _, plain = run(ctx, [cloud], "colored")
    assert differ(got, plain)
    if name == "weight":  # the NaN is in bin 0, the infinities in the i64::MAX and i64::MIN bins; all three points are drawn
        assert pcv.xray_bins(sp.extras["weight"][[3, 4, 12]], size).tolist() == [0, I64_MAX, I64_MIN]
        assert all(any(k in parts[0] for parts in kept.values()) for k in (3, 4, 12))


# ---- 3. filters ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [20, 16])
def test_filters(ctx, scene, level):
    cloud, sp, (g, sh) = scene[level]
    cases = [({"ring": RING}, None), ({"ring": RING, "weight": (-1.0, 4.5)}, None), ({"ring": RING}, (-5.0, 100.0)),
             ({"timestamp": (-30000000000, 2.0 ** 53)}, None)]
    created = []
    for filters, interval in cases:
        xt, got = run(ctx, [cloud], "colored", background="transparent", filter_intervals=filters, intensity_interval=interval)
        want, _, _ = A.tiles([sp], W, PX, "colored", filters=filters, interval=interval, background="transparent", iso=ISO)
        check(xt, got, want, g)
        created.append(xt.num_created)
        xx, gotx = run(ctx, [cloud], "xray", filter_intervals=filters, intensity_interval=interval)
        wantx, _, _ = A.tiles([sp], W, PX, "xray", filters=filters, interval=interval, iso=ISO)
        check(xx, gotx, wantx, g)
        # the batched point query with the same filters on the same tile shapes keeps the same points per tile
        per = dict(filters)
        if interval is not None:
            per["intensity"] = interval
        first, _, off = cloud.query_batch(sh, filters=[per] * len(g["leaf_ids"])).segments()
        first = first.astype(np.int64)
        per_location = (off[first[1:]] - off[first[:-1]]).astype(np.int64)
        assert np.array_equal(xt.kept.astype(np.int64), per_location[xt.created.astype(np.int64)])
        assert np.count_nonzero(per_location) == xt.num_created
    assert 0 < created[1] <= created[0] < 64 and 0 < created[2] <= created[0] < created[3]  # the ring empties whole tiles
    # a list entry on intensity is the interval; a NaN bound keeps nothing and creates no tile
    xa, ga = run(ctx, [cloud], "colored", filter_intervals={"intensity": (-5.0, 100.0), "ring": RING})
    xb, gb = run(ctx, [cloud], "colored", filter_intervals={"ring": RING}, intensity_interval=(-5.0, 100.0))
    assert xa.created_ids == xb.created_ids and np.array_equal(xa.kept, xb.kept) and np.array_equal(xa.images(), xb.images())
    for bad in ({"ring": (np.nan, 200)}, {"weight": (0.0, np.nan)}):
        xn, _ = run(ctx, [cloud], "colored", filter_intervals=bad)
        assert xn.num_created == 0 and xn.created_ids == [] and xn.kept.size == 0


# ---- 4. filter and binning together, two clouds ------------------------------------------------------------------------------
def test_two_clouds_filter_and_binning(ctx, scene):
    a, sa, _ = scene[20]
    b, sb = make(ctx, 18, shift_east=150.0, unsigned_timestamp=True)
    assert a.attributes["timestamp"] == "i64" and b.attributes["timestamp"] == "u64"
    sps = [sa, sb]
    g, _ = prepare(ctx, sps)
    filters = {"ring": (12, 30), "weight": (-1.5, 6.0)}
    kw = dict(background="transparent", binning=("timestamp", BIN), filter_intervals=filters)
    for strategy, skw, okw in (("colored", {}, {}), ("colored_with_intensity", dict(min_intensity=1.0, max_intensity=200.0), dict(lo=1.0, hi=200.0))):
        xt, got = run(ctx, [a, b], strategy, **kw, **skw)
        want, _, kept = A.tiles(sps, W, PX, strategy, ("timestamp", BIN), filters, background="transparent", iso=ISO, **okw)
        check(xt, got, want, g)
        assert any(p[0].size and p[1].size for p in kept.values()) and any(p[1].size == 0 for p in kept.values())
        # several tile groups give the same bytes
        xs, gots = run(ctx, [a, b], strategy, max_workspace_bytes=40_000, **kw, **skw)
        assert xs.created_ids == xt.created_ids and np.array_equal(xs.kept, xt.kept) and not differ(got, gots)
    p = pcv._lib.XrayParams(tile_size_px=W, pixel_size_m=PX, strategy=1, max_workspace_bytes=40_000)
    col = pcv.xray_coloring("colored", binning=("timestamp", BIN))
    k = np.ascontiguousarray(xs.kept, dtype=np.uint64)
    n, err = C.c_uint64(), C.create_string_buffer(256)
    assert pcv.load_library().pcv_xray_plan_groups(k.ctypes.data, k.size, C.byref(p), C.byref(col), 0, C.byref(n), None, err, 256) == 0
    assert n.value >= 3
    # colored does not depend on the order of the clouds (the bounding box is the same union)
    xt, got = run(ctx, [a, b], "colored", **kw)
    xr, gotr = run(ctx, [b, a], "colored", **kw)
    assert xr.created_ids == xt.created_ids and np.array_equal(xr.kept, xt.kept) and np.array_equal(xr.drawn, xt.drawn) and not differ(got, gotr)
    # the U64 cloud alone: its own edges (2^63, 2^64 - 1: the i64::MAX bin at size 1)
    gb, _ = prepare(ctx, [sb])
    xu, gotu = run(ctx, [b], "colored", binning=("timestamp", 1.0))
    wantu, _, _ = A.tiles([sb], W, PX, "colored", ("timestamp", 1.0), iso=ISO)
    check(xu, gotu, wantu, gb)
    b.free()


# ---- 5. directory round trip ---------------------------------------------------------------------------------------------------
def test_directory_round_trip(ctx, scene, tmp_path):
    cloud, sp, _ = scene[20]
    d = tmp_path / "cloud"
    cloud.write(str(d))
    filters = {"ring": RING}
    kw = dict(background="transparent", binning=("timestamp", BIN), filter_intervals=filters)
    direct = cloud.xray_quadtree(W, PX, "colored", query_from_global=ISO, **kw)
    assert 0 < direct.num_created < 64
    built = pcv.build_xray_quadtree(ctx, [d], tmp_path / "py", W, PX, "colored", query_from_global=ISO, **kw)
    assert built.node_ids == direct.node_ids and np.array_equal(built.node_images(), direct.node_images())
    back = ctx.xray_open(tmp_path / "py")  # the written quadtree, read back
    assert len(back) == 1
    assert_same_quadtree(back[0], direct)
    opened = ctx.s2_open(d)
    opened.xray_quadtree(W, PX, "colored", query_from_global=ISO, output_directory=tmp_path / "opened", **kw)
    assert_same_quadtree(ctx.xray_open(tmp_path / "opened")[0], direct)
    # the compiled example writes the same directory (no transform flag there: both sides without one)
    pcv.build_xray_quadtree(ctx, [d], tmp_path / "py_ecef", W, PX, "colored", **kw)
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "examples")])
    exe = os.path.join(ROOT, "examples", "bin", "build_xray_quadtree")
    p = subprocess.run([exe, str(d), "--output-directory", str(tmp_path / "c"), "--resolution", str(PX), "--tile-size", str(W),
                        "--coloring-strategy", "colored", "--tile-background-color", "transparent", "--filter-interval",
                        f"ring={RING[0]},{RING[1]}", "--binning", "timestamp=30000000000"], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr
    names = sorted(os.listdir(tmp_path / "py_ecef"))
    assert names == sorted(os.listdir(tmp_path / "c")) and "meta.pb" in names and len(names) > 5
    for n in names:
        assert (tmp_path / "py_ecef" / n).read_bytes() == (tmp_path / "c" / n).read_bytes(), n
    # a damaged file of the binned column: PCV_E_IO naming it, and the cloud stays usable for what does not read it
    victim = sorted(f for f in os.listdir(d) if f.endswith(".timestamp") and os.path.getsize(d / f) >= 16)[3]
    with open(d / victim, "r+b") as f:
        f.truncate(os.path.getsize(d / victim) - 8)
    broken = ctx.s2_open(d)
    with pytest.raises(pcv.PcvError, match=victim.replace(".", r"\.")) as e:
        broken.xray_tiles(W, PX, "colored", query_from_global=ISO, **kw)
    assert e.value.code == pcv.PCV_E_IO
    plain = broken.xray_tiles(W, PX, "xray", query_from_global=ISO)
    whole = cloud.xray_tiles(W, PX, "xray", query_from_global=ISO)
    assert plain.created_ids == whole.created_ids and np.array_equal(plain.images(), whole.images())
    # the filter's column is intact: a run that reads only that one works too
    ringed = broken.xray_tiles(W, PX, "colored", query_from_global=ISO, filter_intervals=filters)
    assert ringed.num_created == direct.num_created
    opened.free()
    broken.free()


# ---- 6. the old entry equals the new one -------------------------------------------------------------------------------------
def test_old_entry_equals_new(ctx, scene):
    cloud = scene[16][0]
    lib = ctx.lib
    arr = (C.c_void_p * 1)(cloud.handle)
    for strategy, binning in (("xray", None), ("colored", None), ("colored", ("intensity", 16.0)), (("height_stddev", 1.5, "jet"), None),
                              ("colored_with_intensity", None), ("colored_with_intensity", ("intensity", 16.0)), ("xray", ("intensity", 16.0))):
        p = pcv.xray_params(W, PX, strategy, ISO, (-5.0, 150.0), "transparent")
        col = pcv.xray_coloring(strategy if isinstance(strategy, str) else strategy[0], 1.0, 200.0, binning)
        colp = C.byref(col) if col is not None else None
        tiles = []
        for new in (False, True):
            h = C.c_void_p()
            if new:
                ctx._check(lib.pcv_xray_run_s2_ex(ctx.handle, arr, 1, C.byref(p), colp, None, 0, C.byref(h)))
            else:
                ctx._check(lib.pcv_xray_run_s2(ctx.handle, arr, 1, C.byref(p), colp, C.byref(h)))
            tiles.append(pcv.XrayTiles(ctx, h, W))
        old, new = tiles
        assert old.num_created > 0 and old.created_ids == new.created_ids
        for f in ("kept", "drawn", "negative"):
            assert np.array_equal(getattr(old, f), getattr(new, f)), (strategy, binning, f)
        assert np.array_equal(old.images(), new.images()), (strategy, binning)


# ---- 7. refusals on the device path ------------------------------------------------------------------------------------------
def test_refusals(ctx, scene):
    cloud, sp, _ = scene[16]
    x, y, z, rgb = cloud_points()
    bare = ctx.s2_split(dict(x=x, y=y, z=z, color=rgb, attributes={"ring": np.zeros(x.size, np.uint8)}), 16)  # no intensity, no timestamp
    run(ctx, [cloud], "colored", binning=("timestamp", BIN), filter_intervals={"ring": RING})  # (the columns are resident now)
    torch.cuda.synchronize()
    before = torch.cuda.mem_get_info()[0]

    def refused(match, clouds, strategy="colored", **kw):
        with pytest.raises(pcv.PcvError, match=match) as e:
            ctx.xray_tiles(clouds, W, PX, strategy, query_from_global=ISO, **kw)
        assert e.value.code == pcv.PCV_E_INVALID
        return str(e.value)

    assert "S2 cloud 1" in refused("Data type for attribute 'weight' not found", [cloud, bare], filter_intervals={"weight": (0, 1)})
    assert "S2 cloud 1" in refused("Binning attribute needs to be available in points batch", [cloud, bare], binning=("timestamp", BIN))
    refused("Binning attribute needs to be available", [cloud], "xray", binning=("nope", 1.0))
    refused("'normal' of S2 cloud 0 is a vector attribute", [cloud], filter_intervals={"normal": (0, 1)})
    refused("'color' of S2 cloud 0 is a vector attribute", [cloud], filter_intervals={"color": (0, 1)})
    refused("binning takes a scalar attribute; 'normal'", [cloud], binning=("normal", 1.0))
    refused("binning takes a scalar attribute; 'color'", [cloud], binning=("color", 1.0))
    refused("two filters on attribute 'intensity'", [cloud], intensity_interval=(0.0, 1.0), filter_intervals={"intensity": (0.0, 1.0)})
    refused("has no intensity attribute to filter on", [cloud, bare], filter_intervals={"intensity": (0.0, 1.0)})
    refused("has no intensity attribute to color or bin by", [bare], "colored_with_intensity", binning=("ring", 1.0))
    # what a dict cannot say, through the C entry: a repeated name, a NULL name, a NULL list
    lib, h = ctx.lib, C.c_void_p(1)
    arr = (C.c_void_p * 2)(cloud.handle, None)
    p = pcv.xray_params(W, PX, "colored", ISO)

    def raw(filters, n, clouds=1, params=p):
        h.value = 1
        rc = lib.pcv_xray_run_s2_ex(ctx.handle, arr, clouds, C.byref(params), None, filters, n, C.byref(h))
        assert rc == pcv.PCV_E_INVALID and not h.value
        return lib.pcv_last_error(ctx.handle).decode()

    fl = (pcv._lib.XrayFilter * 3)()
    fl[0].attribute, fl[1].attribute, fl[2].attribute = b"ring", b"weight", b"ring"
    assert "two filters on attribute 'ring'" in raw(fl, 3)
    fl[2].attribute = None
    assert "filter 2 has no attribute name" in raw(fl, 3)
    assert "null argument" in raw(None, 2)
    # every refusal of pcv_xray_run_s2
    assert "No locations specified for point cloud client." in raw(fl, 2, clouds=0)
    assert "S2 cloud 1 is null" in raw(fl, 2, clouds=2)
    assert "unknown strategy" in raw(fl, 2, params=pcv._lib.XrayParams(tile_size_px=W, pixel_size_m=PX, strategy=9))
    assert "only intensity is supported" in raw(fl, 2, params=pcv._lib.XrayParams(tile_size_px=W, pixel_size_m=PX, interval_attribute=b"ring"))
    assert "tile_size_px" in raw(fl, 2, params=pcv._lib.XrayParams(tile_size_px=0, pixel_size_m=PX))
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] >= before - (1 << 20)  # nothing is left allocated (the margin is the runtime's own)
    xt, _ = run(ctx, [cloud], "colored", binning=("timestamp", BIN), filter_intervals={"ring": RING})  # a good run follows
    assert xt.num_created > 0
    # the octree forms keep today's message
    rng = np.random.default_rng(5)
    tree = ctx.build(0.001, pcv.Aabb(np.zeros(3), np.ones(3)), rng.random(100), rng.random(100), rng.random(100), np.zeros((100, 3), np.uint8),
                     rng.random(100).astype(np.float32))
    for form in (lambda **kw: tree.xray_tiles(16, 0.1, "colored", **kw), lambda **kw: ctx.xray_tiles([tree, tree], 16, 0.1, "colored", **kw)):
        with pytest.raises(pcv.PcvError, match="xray: binning on attribute 'timestamp': only intensity can be binned on"):
            form(binning=("timestamp", 1))
    with pytest.raises(ValueError, match="filter_intervals take S2 cell clouds"):
        ctx.xray_tiles([tree], 16, 0.1, "colored", filter_intervals={"ring": RING})
    tree.free()
    bare.free()
