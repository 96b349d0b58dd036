"""The host side of xray's filters and binning on any scalar attribute of S2 cell clouds (pcv_xray_run_s2_ex): the bin of a
value, pcv_xray_bins_host — the function the raster kernel compiles — against a numpy restatement of
BinnedColoringStrategy::bins (xray/src/generation.rs:138-157) written here, and the refusals of pcv_xray_check_attrs_host
with their messages. No device."""
import numpy as np
import pytest

import point_cloud_viewer_amd as pcv

I64_MIN, I64_MAX = np.iinfo(np.int64).min, np.iinfo(np.int64).max
SIZES = [1.0, 3.0, 30000000000.0, 0.25, 0.0, -7.0, np.inf, np.nan]


def restated_bins(values, size):
    """`(e as f64 / size) as i64`: numpy's conversion to f64 (exact, or nearest-even for the 64-bit integers), one f64
    division, then the truncation of xray_intensity_oracle.bins_of: saturating, NaN -> 0."""
    with np.errstate(all="ignore"):
        v = values.astype(np.float64) / np.float64(size)
    out = np.zeros(v.shape, dtype=np.int64)
    fin = np.isfinite(v) & (v < 9223372036854775808.0) & (v >= -9223372036854775808.0)
    out[fin] = np.trunc(v[fin]).astype(np.int64)
    out[~np.isnan(v) & (v >= 9223372036854775808.0)] = I64_MAX
    out[~np.isnan(v) & (v < -9223372036854775808.0)] = I64_MIN
    return out


def values_of(dtype):
    dt = np.dtype(dtype)
    rng = np.random.default_rng(dt.num)
    if dt.kind == "f":
        tiny = np.finfo(dt).smallest_subnormal
        edge = [0.0, -0.0, np.inf, -np.inf, np.nan, tiny, -tiny, 3 * tiny, np.finfo(dt).max, np.finfo(dt).min, 0.25, -0.25, 6.999, -6.999,
                7.0, -7.0, 2.0 ** 53, 2.0 ** 63, -(2.0 ** 63), 2.0 ** 64, 9.3e18, -9.3e18, 89999999999.0, 90000000000.0]
        rand = (rng.standard_normal(500) * 1e11).tolist()
        return np.array(edge + rand, dtype=dt)
    info = np.iinfo(dt)
    edge = [0, 1, 2, 3, 6, 7, 8, info.max, info.max - 1, info.min, info.min + 1]
    if info.min < 0:
        edge += [-1, -2, -3, -6, -7, -8]
    if dt.itemsize == 8:
        edge += [2 ** 53 - 1, 2 ** 53, 2 ** 53 + 1, 2 ** 53 + 2, 2 ** 53 + 3, 2 ** 63 - 1, 2 ** 63 - 512, 2 ** 63 - 513,
                 29999999999, 30000000000, 89999999999, 90000000000]
        if info.min < 0:
            edge += [-(2 ** 53) - 1, -(2 ** 53) + 1, -(2 ** 53) - 3, I64_MIN, I64_MIN + 1, -29999999999, -30000000000]
        else:
            edge += [2 ** 63, 2 ** 63 + 1, 2 ** 63 + 1024, 2 ** 63 + 1025, 2 ** 64 - 1, 2 ** 64 - 1024, 2 ** 64 - 1025]
    rand = rng.integers(info.min, info.max, 500, dtype=dt, endpoint=True)
    return np.concatenate([np.array(edge, dtype=dt), rand])


@pytest.mark.parametrize("dtype", ["u1", "<u2", "<u4", "<u8", "i1", "<i2", "<i4", "<i8", "<f4", "<f8"])
def test_bins_equal_the_restatement(dtype):
    v = values_of(dtype)
    if np.dtype(dtype).kind == "i":
        assert (v < 0).sum() > 100
    for size in SIZES:
        got = pcv.xray_bins(v, size)
        want = restated_bins(v, size)
        assert got.dtype == np.int64 and np.array_equal(got, want), (dtype, size, v[got != want][:5], got[got != want][:5], want[got != want][:5])
    # an unaligned buffer, and an empty one
    raw = np.zeros(v.nbytes + 1, dtype=np.uint8)
    raw[1:] = v.view(np.uint8)
    assert np.array_equal(pcv.xray_bins(raw[1:].view(dtype), 3.0), restated_bins(v, 3.0))
    assert pcv.xray_bins(np.zeros(0, dtype=dtype), 1.0).size == 0


def test_bins_at_the_edges_of_f64():
    """the values the conversion and the saturation decide, written out"""
    i64 = np.array([2 ** 53 - 1, 2 ** 53, 2 ** 53 + 1, 2 ** 53 + 2, 2 ** 53 + 3, 2 ** 63 - 1, I64_MIN, -(2 ** 53) - 1, -7, 7], dtype=np.int64)
    # ties to even: 2^53 + 1 -> 2^53, 2^53 + 3 -> 2^53 + 4; 2^63 - 1 -> 2^63, which saturates; i64::MIN is exact
    assert pcv.xray_bins(i64, 1.0).tolist() == [2 ** 53 - 1, 2 ** 53, 2 ** 53, 2 ** 53 + 2, 2 ** 53 + 4, I64_MAX, I64_MIN, -(2 ** 53), -7, 7]
    u64 = np.array([2 ** 53 + 1, 2 ** 53 + 3, 2 ** 63 - 1, 2 ** 63, 2 ** 64 - 1, 2 ** 63 - 513, 2 ** 63 - 512], dtype=np.uint64)
    assert pcv.xray_bins(u64, 1.0).tolist() == [2 ** 53, 2 ** 53 + 4, I64_MAX, I64_MAX, I64_MAX, 2 ** 63 - 1024, I64_MAX]
    assert pcv.xray_bins(u64, 2.0).tolist() == [2 ** 52, 2 ** 52 + 2, 2 ** 62, 2 ** 62, 2 ** 63 - 1, 2 ** 62 - 512, 2 ** 62]
    # a pair that differs only below f64 precision lands in one bin; a pair that straddles a rounded boundary in two
    assert pcv.xray_bins(np.array([2 ** 53, 2 ** 53 + 1], dtype=np.int64), 1.0).tolist() == [2 ** 53, 2 ** 53]
    assert pcv.xray_bins(np.array([2 ** 60, 2 ** 60 + 64], dtype=np.uint64), 128.0).tolist() == [2 ** 53, 2 ** 53]
    assert pcv.xray_bins(np.array([2 ** 53 + 1, 2 ** 53 + 3], dtype=np.int64), 1.0).tolist() == [2 ** 53, 2 ** 53 + 4]
    assert pcv.xray_bins(np.array([89999999999, 90000000000], dtype=np.int64), 30000000000.0).tolist() == [2, 3]
    # truncation toward zero, size 0, NaN, infinities
    assert pcv.xray_bins(np.array([-1, 1, -29999999999, 29999999999], dtype=np.int64), 30000000000.0).tolist() == [0, 0, 0, 0]
    assert pcv.xray_bins(np.array([-5, 0, 5], dtype=np.int8), 0.0).tolist() == [I64_MIN, 0, I64_MAX]  # -inf, NaN, +inf
    assert pcv.xray_bins(np.array([-5, 0, 5], dtype=np.int8), -0.0).tolist() == [I64_MAX, 0, I64_MIN]
    f = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 5e-324, -5e-324, 1e300], dtype=np.float64)
    assert pcv.xray_bins(f, 1.0).tolist() == [0, I64_MAX, I64_MIN, 0, 0, 0, 0, I64_MAX]
    assert pcv.xray_bins(f, np.inf).tolist() == [0, 0, 0, 0, 0, 0, 0, 0]  # inf / inf is NaN
    assert pcv.xray_bins(f, 5e-324).tolist() == [0, I64_MAX, I64_MIN, 0, 0, 1, -1, I64_MAX]
    f32 = np.array([1e-45, -1e-45, 3e-45], dtype=np.float32)  # denormals: exact in f64
    assert pcv.xray_bins(f32, float(np.float32(1e-45))).tolist() == [1, -1, 2]


def test_bins_refuse_what_has_no_bins():
    lib = pcv.load_library()
    out = np.zeros(4, dtype=np.int64)
    data = np.zeros(96, dtype=np.uint8)
    for code in (27, 38):  # U8Vec3, F64Vec3
        assert lib.pcv_xray_bins_host(code, 4, data.ctypes.data, 1.0, out.ctypes.data) == pcv.PCV_E_INVALID
        assert b"scalar" in lib.pcv_host_last_error()
    assert lib.pcv_xray_bins_host(5, 4, data.ctypes.data, 1.0, out.ctypes.data) == pcv.PCV_E_INVALID
    assert lib.pcv_xray_bins_host(9, 4, None, 1.0, out.ctypes.data) == pcv.PCV_E_INVALID
    assert lib.pcv_xray_bins_host(9, 0, None, 1.0, None) == pcv.PCV_OK
    with pytest.raises(pcv.PcvError):
        pcv.xray_bins(np.zeros(3, dtype=np.complex64), 1.0)


# ---- pcv_xray_check_attrs_host ---------------------------------------------------------------------------------------------
A = ({"timestamp": "i64", "ring": "u8", "weight": "f64", "normal": "f64vec3", "tint": "u8vec3"}, True)
B = ({"timestamp": "u64", "ring": "u8", "weight": "f64", "normal": "f64vec3"}, True)
BARE = ({"timestamp": "i64"}, False)


def check(clouds, strategy="colored", binning=None, filters=None, intensity_interval=None, **kw):
    p = pcv.xray_params(64, 0.5, strategy, intensity_interval=intensity_interval)
    col = pcv.xray_coloring(strategy, binning=binning, **kw)
    pcv.xray_check_attrs(p, clouds, col, filters)


def refused(match, *args, **kw):
    with pytest.raises(pcv.PcvError, match=match) as e:
        check(*args, **kw)
    assert e.value.code == pcv.PCV_E_INVALID
    return str(e.value)


def test_check_attrs_accepts():
    check([A])
    check([A], binning=("timestamp", 30000000000.0))
    check([A, B], binning=("timestamp", 30000000000.0))  # one name, I64 in one cloud and U64 in the other
    check([A, B, A], "colored_with_intensity", binning=("weight", 0.5), filters={"ring": (3, 9), "weight": (0.0, 1.0)})
    check([A], binning=("intensity", 16.0), filters={"ring": (0, 255)})
    check([A], filters={"intensity": (0.0, 1.0), "timestamp": (-1e18, 1e18)})
    check([A], filters={"ring": (np.nan, 1.0)})  # a NaN bound keeps nothing; it is no error
    check([A], intensity_interval=(0.0, 5.0), filters={"ring": (1, 2)})  # interval_attribute is ANDed with the list
    check([A], binning=("timestamp", 0.0))  # the size is not validated (generation.rs:149)
    check([BARE], binning=("timestamp", 5.0))  # colored binned on an extra reads no intensity
    check([BARE], "xray", binning=("intensity", 5.0))  # xray and height_stddev never read the binning
    check([A], "xray", binning=("timestamp", 5.0))
    check([A], ("height_stddev", 1.5, "jet"), binning=("ring", 5.0), filters={"weight": (0, 1)})
    check([({}, True)], filters={"intensity": (0.0, 1.0)})


def test_check_attrs_refuses():
    # an attribute some cloud does not have, with the cloud's index
    m = refused("Data type for attribute 'ring' not found", [A, BARE], filters={"ring": (1, 2)})
    assert "S2 cloud 1" in m
    m = refused("Binning attribute needs to be available in points batch", [A, B, BARE], binning=("weight", 1.0))
    assert "S2 cloud 2" in m and "'weight'" in m
    refused("Binning attribute needs to be available", [A], "xray", binning=("nope", 1.0))  # the name is checked whatever reads it
    refused("Data type for attribute '' not found", [A], filters={"": (1, 2)})
    # vector attributes, color included
    for name in ("normal", "tint", "color"):
        assert "S2 cloud 0" in refused(f"'{name}' of S2 cloud 0 is a vector attribute", [A], filters={name: (0, 1)})
        refused(f"binning takes a scalar attribute; '{name}'", [A], binning=(name, 1.0))
    assert "S2 cloud 1" not in refused("vector", [A, B], filters={"normal": (0, 1)})
    # two filters on one attribute; intensity beside interval_attribute
    refused("two filters on attribute 'ring'", [A], filters=[("ring", 0, 1), ("weight", 0, 1), ("ring", 2, 3)])
    refused("two filters on attribute 'intensity'", [A], intensity_interval=(0.0, 1.0), filters={"intensity": (0.0, 1.0)})
    # a NULL name
    refused("filter 1 has no attribute name", [A], filters=[("ring", 0, 1), (None, 0, 1)])
    # intensity that a cloud lacks: filter, interval, strategy, binning
    assert "S2 cloud 1" in refused("has no intensity attribute to filter on", [A, BARE], filters={"intensity": (0.0, 1.0)})
    refused("has no intensity attribute to filter on", [BARE], intensity_interval=(0.0, 1.0), filters={"timestamp": (0, 1)})
    refused("has no intensity attribute to color or bin by", [BARE], "colored_with_intensity", binning=("timestamp", 1.0))
    refused("has no intensity attribute to color or bin by", [BARE], binning=("intensity", 1.0), filters={"timestamp": (0, 1)})
    # the refusals of pcv_xray_check_params_ex come through unchanged
    lib, L = pcv.load_library(), pcv._lib
    import ctypes as C
    err = C.create_string_buffer(256)
    first = np.zeros(2, dtype=np.uint32)
    has = np.ones(1, dtype=np.uint8)

    def raw(p, col=None, clouds=1):
        rc = lib.pcv_xray_check_attrs_host(C.byref(p) if p is not None else None, C.byref(col) if col is not None else None, None, 0, clouds,
                                           first.ctypes.data, None, None, has.ctypes.data, err, 256)
        return rc, err.value.decode()

    assert raw(L.XrayParams(tile_size_px=64, pixel_size_m=0.5, strategy=9)) == (pcv.PCV_E_INVALID, "xray: unknown strategy")
    rc, m = raw(L.XrayParams(tile_size_px=64, pixel_size_m=0.5, strategy=3))
    assert rc == pcv.PCV_E_INVALID and "colored_with_intensity needs a pcv_xray_coloring" in m
    rc, m = raw(L.XrayParams(tile_size_px=64, pixel_size_m=0.5, interval_attribute=b"ring"))
    assert rc == pcv.PCV_E_INVALID and "only intensity is supported" in m  # interval_attribute stays "intensity" or NULL
    rc, m = raw(L.XrayParams(tile_size_px=64, pixel_size_m=0.5), clouds=0)
    assert rc == pcv.PCV_E_INVALID and "No locations specified for point cloud client." in m
    assert raw(None)[0] == pcv.PCV_E_INVALID
    assert raw(L.XrayParams(tile_size_px=64, pixel_size_m=0.5))[0] == pcv.PCV_OK


def test_old_checks_keep_their_messages():
    """pcv_xray_check_params_ex, the octree path's check, still knows intensity alone"""
    p = pcv.xray_params(64, 0.5, "colored")
    with pytest.raises(pcv.PcvError, match="xray: binning on attribute 'timestamp': only intensity can be binned on"):
        pcv.xray_check_params(p, True, pcv.xray_coloring("colored", binning=("timestamp", 1.0)))
    p = pcv._lib.XrayParams(tile_size_px=64, pixel_size_m=0.5, interval_attribute=b"ring")
    with pytest.raises(pcv.PcvError, match="xray: filter on attribute 'ring': only intensity is supported"):
        pcv.xray_check_params(p, True)


def test_filters_argument():
    arr, names = pcv.xray_filters({"ring": (1, 2), "weight": (0.5, np.inf)})
    assert [(arr[k].attribute, arr[k].lo, arr[k].hi) for k in range(2)] == [(b"ring", 1.0, 2.0), (b"weight", 0.5, np.inf)] and len(names) == 2
    assert pcv.xray_filters(None) == (None, []) and pcv.xray_filters({}) == (None, [])
    with pytest.raises(ValueError):
        pcv.xray_filters({"ring": (1, 2, 3)})
    with pytest.raises(ValueError):
        pcv.xray_filters({3: (1, 2)})
