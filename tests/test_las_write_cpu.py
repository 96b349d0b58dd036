"""LAS output on the host (no GPU): the numpy truth of tests/las_write_truth.py against two files typed byte by byte
from the specification's offsets, the host twin (pcv_las_encode_host) and the header builder against the truth for every format,
pick after put through the project's reader, the edges of the quantiser, the intensity and the scan angle, the masking counts,
every refusal with the field it names, the append check, and a sanitizer build of the host code."""
import os
import struct
import subprocess

import numpy as np
import pytest

import las_truth as LT
import las_write_truth as WT
import point_cloud_viewer_amd as pcv
from point_cloud_viewer_amd import _lib as L
from sort_plan_helper import SANITIZE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "point_cloud_viewer_amd", "csrc")
FORMATS = [0, 1, 2, 3, 6, 7, 8]


def points_of(n, seed, **attributes):
    rng = np.random.default_rng(seed)
    return dict(x=rng.random(n) * 2000 + 4.2e6, y=rng.random(n) * 2000 - 3.3e6, z=rng.random(n) * 300 - 50,
                color=rng.integers(0, 256, (n, 3)).astype(np.uint8), intensity=(rng.random(n) * 70000 - 2000).astype(np.float32),
                attributes=attributes)


def corner_attributes(fmt, n, seed):
    """All twelve extras with the corners of every field's range and beyond, and a foreign one."""
    f = LT.random_fields(fmt, n, seed=seed)
    rng = np.random.default_rng(seed + 50)
    wide = lambda: np.concatenate([[0, 1, 7, 8, 15, 16, 31, 32, 255], rng.integers(0, 256, n - 9)]).astype(np.uint8)
    angle = (rng.random(n) * 500 - 250).astype(np.float32)
    angle[:8] = [np.nan, np.inf, -np.inf, -0.0, 0.5, 1.5, 2.5, -128.5]
    return dict(classification=wide(), classification_flags=wide(), return_number=wide(), number_of_returns=wide()[::-1].copy(),
                scan_direction_flag=rng.integers(0, 3, n).astype(np.uint8), edge_of_flight_line=rng.integers(0, 2, n).astype(np.uint8),
                scanner_channel=wide(), scan_angle=angle, user_data=f["user_data"], point_source_id=f["point_source_id"],
                gps_time=f["gps_bits"].view(np.float64), nir=f["nir"], foreign=np.arange(n, dtype=np.int64))


# ---- the two files typed by hand ----------------------------------------------------------------------------------------------
def _hand_format3_v12():
    """LAS 1.2, format 3, three records; every byte placed by struct at the offsets of the specification."""
    h = bytearray(227)
    struct.pack_into("<4sHH", h, 0, b"LASF", 9, 1)
    struct.pack_into("<BB", h, 24, 1, 2)
    struct.pack_into("<32s32s", h, 26, b"OTHER", b"point_cloud_viewer_amd")
    struct.pack_into("<HHH", h, 90, 200, 2030, 227)
    struct.pack_into("<II", h, 96, 227, 0)
    struct.pack_into("<BH", h, 104, 3, 34)
    struct.pack_into("<I5I", h, 107, 3, 1, 1, 0, 0, 0)  # count; returns 1 and 2 once each, the third record's return 0 nowhere
    struct.pack_into("<3d", h, 131, 0.01, 0.01, 0.001)
    struct.pack_into("<3d", h, 155, 4.5e6, 5.0e5, -10.0)
    # max x, min x, max y, min y, max z, min z: X * scale + offset over the integers below
    struct.pack_into("<6d", h, 179, 12345 * 0.01 + 4.5e6, -1 * 0.01 + 4.5e6, 0 * 0.01 + 5.0e5, -678 * 0.01 + 5.0e5, 1000 * 0.001 + -10.0,
                     2 * 0.001 + -10.0)
    recs = b""
    # X, Y, Z, intensity, return byte, class byte, scan angle rank, user data, point source id, gps time, R, G, B
    recs += struct.pack("<iiiHBBbBHdHHH", 12345, -678, 1000, 500, 2 | (3 << 3) | (1 << 6), 2 | (1 << 7), -15, 7, 4711, 1.5, 255 * 257, 257, 0)
    recs += struct.pack("<iiiHBBbBHdHHH", -1, 0, 2, 65535, 1 | (1 << 3) | (1 << 7), 31 | (1 << 5) | (1 << 6), 90, 255, 1, -0.0, 0, 257, 2 * 257)
    recs += struct.pack("<iiiHBBbBHdHHH", 0, -1, 500, 0, 0 | (7 << 3), 0, -128, 0, 65535, 2.0, 3 * 257, 4 * 257, 5 * 257)
    points = dict(x=np.array([12345 * 0.01 + 4.5e6, -1 * 0.01 + 4.5e6, 4.5e6]), y=np.array([-678 * 0.01 + 5.0e5, 5.0e5, -0.01 + 5.0e5]),
                  z=np.array([-9.0, -9.998, -9.5]), color=np.array([[255, 1, 0], [0, 1, 2], [3, 4, 5]], np.uint8),
                  intensity=np.array([500.0, 70000.0, -3.0], np.float32),
                  attributes=dict(return_number=np.array([2, 1, 8], np.uint8), number_of_returns=np.array([3, 1, 7], np.uint8),
                                  scan_direction_flag=np.array([1, 0, 0], np.uint8), edge_of_flight_line=np.array([0, 1, 0], np.uint8),
                                  classification=np.array([2, 31, 32], np.uint8), classification_flags=np.array([4, 3, 8], np.uint8),
                                  scan_angle=np.array([-15.2, 90.4, -200.0], np.float32), user_data=np.array([7, 255, 0], np.uint8),
                                  point_source_id=np.array([4711, 1, 65535], np.uint16), gps_time=np.array([1.5, -0.0, 2.0])))
    kw = dict(point_format=3, scale=(0.01, 0.01, 0.001), offset=(4.5e6, 5.0e5, -10.0))
    hk = dict(file_source_id=9, global_encoding=1, day=200, year=2030)
    return bytes(h), recs, points, kw, hk, dict(masked_values=3, clamped_intensity=2)  # return 8, class 32, flags 8; 70000 and -3


def _hand_format8_v14():
    """LAS 1.4, format 8, two records."""
    h = bytearray(375)
    struct.pack_into("<4s", h, 0, b"LASF")
    struct.pack_into("<BB", h, 24, 1, 4)
    struct.pack_into("<32s32s", h, 26, b"a scanner", b"some software")
    struct.pack_into("<H", h, 94, 375)
    struct.pack_into("<I", h, 96, 375)
    struct.pack_into("<BH", h, 104, 8, 38)
    struct.pack_into("<3d", h, 131, 0.001, 0.001, 0.001)
    struct.pack_into("<3d", h, 155, 0.0, 0.0, 0.0)
    struct.pack_into("<6d", h, 179, 1000 * 0.001, -2147483648 * 0.001, 2147483647 * 0.001, 2000 * 0.001, 0.0, -3000 * 0.001)
    struct.pack_into("<Q", h, 247, 2)
    struct.pack_into("<Q", h, 255 + 8 * 4, 1)   # return 5
    struct.pack_into("<Q", h, 255 + 8 * 14, 1)  # return 15
    recs = b""
    # X, Y, Z, intensity, return byte, flag byte, class, user data, scan angle, point source id, gps time, R, G, B, NIR
    recs += struct.pack("<iiiHBBBBhHdHHHH", 1000, 2000, -3000, 10, 5 | (9 << 4), 8 | (2 << 4) | (1 << 6), 255, 1, 5000, 2, 3.25, 256, 512, 768, 40000)
    recs += struct.pack("<iiiHBBBBhHdHHHH", -2147483648, 2147483647, 0, 0, 15 | (15 << 4), 4 | (3 << 4) | (1 << 7), 32, 0, -30000, 65535, 1e9,
                        200 << 8, 100 << 8, 0, 0)
    points = dict(x=np.array([1.0, -2147483.648]), y=np.array([2.0, 2147483.647]), z=np.array([-3.0, 0.0]),
                  color=np.array([[1, 2, 3], [200, 100, 0]], np.uint8), intensity=np.array([10.4, 0.0], np.float32),
                  attributes=dict(return_number=np.array([5, 15], np.uint8), number_of_returns=np.array([9, 15], np.uint8),
                                  classification_flags=np.array([8, 4], np.uint8), scanner_channel=np.array([2, 3], np.uint8),
                                  scan_direction_flag=np.array([1, 0], np.uint8), edge_of_flight_line=np.array([0, 1], np.uint8),
                                  classification=np.array([255, 32], np.uint8), user_data=np.array([1, 0], np.uint8),
                                  scan_angle=np.array([30.0, -180.0], np.float32), point_source_id=np.array([2, 65535], np.uint16),
                                  gps_time=np.array([3.25, 1e9]), nir=np.array([40000, 0], np.uint16)))
    kw = dict(scale=0.001, offset=0.0, color="shift8")
    hk = dict(system_identifier=b"a scanner", generating_software=b"some software")
    return bytes(h), recs, points, kw, hk, dict(masked_values=0, clamped_intensity=0)


@pytest.mark.parametrize("make", [_hand_format3_v12, _hand_format8_v14])
def test_truth_and_twin_equal_the_hand_typed_files(make):
    header, recs, points, kw, hk, counts = make()
    tkw = dict(kw)
    data, tinfo = WT.records(points, fmt=tkw.pop("point_format", WT.AUTO), **tkw)
    assert data == recs and WT.header(tinfo, **hk) == header
    got, info = pcv.las_encode_host(points, **kw)
    assert got.tobytes() == recs
    WT.assert_info(info, tinfo)
    assert {k: info[k] for k in counts} == counts and info["out_of_range"] == 0
    names = {k: (v.decode() if isinstance(v, bytes) else v) for k, v in hk.items()}
    assert pcv.las_write_header(info, **kw, **names) == header


@pytest.mark.parametrize("fmt", FORMATS)
def test_host_twin_equals_the_truth_and_the_reader_gives_the_fields_back(tmp_path, fmt):
    n = 257
    pts = points_of(n, fmt, **corner_attributes(fmt, n, fmt))
    for offset in (None, (4.2e6, -3.3e6, -50.0)):
        want, winfo = WT.records(pts, fmt=fmt, offset=offset)
        got, info = pcv.las_encode_host(pts, point_format=fmt, offset=offset)
        assert got.shape == (n, LT.MIN_LEN[fmt]) and got.tobytes() == want
        WT.assert_info(info, winfo, f"format {fmt}")
        assert info["skipped_extras"] == 1 and info["masked_values"] > 0 and info["clamped_intensity"] > 0 and info["out_of_range"] == 0
        assert pcv.las_write_header(info, day=1, year=2) == WT.header(winfo, day=1, year=2)
    # pick after put: the project's own decode of these records returns the logical fields, masked and clamped by the rules
    hdr = dict(version=(1, info["version_minor"]), point_format=fmt, header_size=info["header_size"], record_length=info["record_length"],
               offset_to_points=info["header_size"], num_points=n, scale=info["scale"], offset=info["offset"])
    back = pcv.las_decode_host(hdr, got, extras="all", keep_intensity=True, color="rgb16" if fmt in LT.HAS_RGB else "auto")
    a = pts["attributes"]
    rmask, cmask, fmask = (15, 255, 15) if fmt >= 6 else (7, 31, 7)
    expect = dict(classification=a["classification"] & cmask, classification_flags=a["classification_flags"] & fmask,
                  return_number=a["return_number"] & rmask, number_of_returns=a["number_of_returns"] & rmask,
                  scan_direction_flag=a["scan_direction_flag"] & 1, edge_of_flight_line=a["edge_of_flight_line"] & 1,
                  user_data=a["user_data"], point_source_id=a["point_source_id"])
    if fmt >= 6:
        expect["scanner_channel"] = a["scanner_channel"] & 3
        expect["scan_angle"] = WT.angle_code(a["scan_angle"], True).astype(np.float32) * np.float32(0.006)
    else:
        expect["scan_angle"] = WT.angle_code(a["scan_angle"], False).astype(np.float32)
    if fmt in LT.HAS_GPS:
        expect["gps_time"] = a["gps_time"]
    if fmt in LT.HAS_NIR:
        expect["nir"] = a["nir"]
    assert sorted(back["attributes"]) == sorted(expect)
    for k, v in expect.items():
        assert LT.same_bits(back["attributes"][k], np.asarray(v).astype(LT.EXTRA_DTYPES[k])), k
    assert back["intensity"].tobytes() == WT.intensity_u16(pts["intensity"])[0].astype(np.float32).tobytes()
    if fmt in LT.HAS_RGB:
        assert back["color"].tobytes() == pts["color"].tobytes()  # c * 257 >> 8 == c
    for k, s, o in zip("xyz", info["scale"], info["offset"]):
        assert np.all(np.abs(back[k] - pts[k]) <= s / 2 + 4 * np.spacing(np.maximum(np.abs(pts[k]), abs(o)))), k


def test_position_edges():
    s, o = 0.5, 0.0  # the quotients are exact: a power of two as scale
    q = np.array([0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 2147483647.49, 2147483647.5, -2147483648.49, -2147483648.5, np.inf, -np.inf, np.nan, 0.0])
    x = q * s + o
    assert np.array_equal(((x - o) / s)[:10], q[:10])
    x[-1] = -0.0
    pts = dict(x=x, y=np.full(len(x), o), z=np.full(len(x), o), color=None, intensity=None, attributes={})
    got, info = pcv.las_encode_host(pts, point_format=0, scale=s, offset=o)
    X = got.view("<i4")[:, 0]
    # ties go to the even integer; 2147483647.49 rounds to 2147483647 and is in
    assert X.tolist() == [0, 2, 2, 0, -2, -2, 2147483647, 0, -2147483648, 0, 0, 0, 0, 0]
    assert info["out_of_range"] == 5 and got.tobytes() == WT.records(pts, fmt=0, scale=s, offset=o)[0]
    # one axis out of range: the whole record's position is 0, and it counts once
    pts2 = dict(x=np.array([11.0, 11.0]), y=np.array([12.0, np.nan]), z=np.array([13.0, 13.0]), color=None, intensity=None, attributes={})
    got, info = pcv.las_encode_host(pts2, point_format=0, scale=s, offset=10.0)
    assert got.view("<i4")[:, :3].tolist() == [[2, 4, 6], [0, 0, 0]] and info["out_of_range"] == 1
    assert info["min_xyz"] == (0, 0, 0) and info["max_xyz"] == (2, 4, 6)
    # floor(min) for negative minima, -0.0 and a range without rows
    for v, want in (([-0.25, 3.0], -1.0), ([-7.0, -6.5], -7.0), ([-0.0, 0.0], -0.0), ([2.75], 2.0), ([], 0.0)):
        p = dict(x=np.array(v), y=np.array(v), z=np.array(v), color=None, intensity=None, attributes={})
        _, info = pcv.las_encode_host(p, point_format=0, scale=0.001)
        assert info["offset"] == (want,) * 3 and WT.floor_min(v) == want, v


def test_intensity_edges():
    v = np.array([np.nan, -1.0, 0.5, 1.5, 2.5, 65535.4, 65535.5, np.inf, -np.inf, 65535.0, 65534.5, -0.0], np.float32)
    pts = dict(x=np.zeros(len(v)), y=np.zeros(len(v)), z=np.zeros(len(v)), color=None, intensity=v, attributes={})
    got, info = pcv.las_encode_host(pts, point_format=0, scale=1.0, offset=0.0)
    codes = got[:, 12:14].copy().view("<u2")[:, 0]
    assert codes.tolist() == [0, 0, 0, 2, 2, 65535, 65535, 65535, 0, 65535, 65534, 0]
    assert info["clamped_intensity"] == 6  # NaN, -1, 65535.4, 65535.5, inf, -inf
    assert np.array_equal(codes, WT.intensity_u16(v)[0]) and int(WT.intensity_u16(v)[1].sum()) == 6
    unit = np.linspace(0.0, 1.0, 4097).astype(np.float32)
    pts = dict(x=np.zeros(4097), y=np.zeros(4097), z=np.zeros(4097), color=None, intensity=unit, attributes={})
    got, info = pcv.las_encode_host(pts, point_format=0, scale=1.0, offset=0.0, intensity_scale=65535.0)
    codes = got[:, 12:14].copy().view("<u2")[:, 0]
    assert np.array_equal(codes, np.rint(unit * np.float32(65535.0)).astype(np.uint16)) and codes[0] == 0 and codes[-1] == 65535
    assert info["clamped_intensity"] == 0


def test_every_angle_code_round_trips():
    for modern, codes, fmt in ((True, np.arange(-32768, 32768), 6), (False, np.arange(-128, 128), 0)):
        n = len(codes)
        degrees = codes.astype(np.float32) * np.float32(0.006) if modern else codes.astype(np.float32)  # the reader's value
        assert np.array_equal(WT.angle_code(degrees, modern), codes)
        pts = dict(x=np.zeros(n), y=np.zeros(n), z=np.zeros(n), color=None, intensity=None, attributes=dict(scan_angle=degrees))
        got, _ = pcv.las_encode_host(pts, point_format=fmt, scale=1.0, offset=0.0)
        back = got[:, 18:20].copy().view("<i2")[:, 0] if modern else got[:, 16].view(np.int8)
        assert np.array_equal(back, codes)


def test_masking_counts():
    n = 256
    every = np.arange(n, dtype=np.uint8)
    for fmt, widths in ((1, dict(return_number=7, number_of_returns=7, classification=31, classification_flags=7)),
                        (6, dict(return_number=15, number_of_returns=15, classification=255, classification_flags=15, scanner_channel=3))):
        for name, top in widths.items():
            pts = dict(x=np.zeros(n), y=np.zeros(n), z=np.zeros(n), color=None, intensity=None, attributes={name: every})
            _, info = pcv.las_encode_host(pts, point_format=fmt, scale=1.0, offset=0.0)
            assert info["masked_values"] == 255 - top, (fmt, name)
            if name == "return_number":
                assert info["by_return"].tolist() == [n // (top + 1)] * top + [0] * (15 - top)  # return 0 counts nowhere


def test_headers_of_both_versions():
    info = dict(point_format=1, version_minor=2, scale=(0.001, 0.002, 0.003), offset=(1.0, 2.0, 3.0), num_records=77,
                by_return=np.arange(1, 16, dtype=np.uint64), bounds=(6.0, 5.0, 4.0, 3.0, 2.0, 1.0))
    for fmt, minor in ((1, 2), (1, 4), (6, 4)):
        info.update(point_format=fmt, version_minor=minor)
        h = pcv.las_write_header(info, file_source_id=3, year=1999)
        assert h == WT.header(info, file_source_id=3, year=1999) and len(h) == (227 if minor == 2 else 375)
        legacy_count, legacy_returns = struct.unpack_from("<I5I", h, 107)[0], struct.unpack_from("<I5I", h, 107)[1:]
        assert (legacy_count, legacy_returns) == ((77, (1, 2, 3, 4, 5)) if fmt <= 3 else (0, (0,) * 5))
        if minor == 4:
            assert struct.unpack_from("<Q15Q", h, 247) == (77,) + tuple(range(1, 16))
        assert h[8:24] == bytes(16) and struct.unpack_from("<HI", h, 94) == (len(h), len(h)) and struct.unpack_from("<I", h, 100) == (0,)
    info.update(num_records=2 ** 32 - 1)
    with pytest.raises(pcv.PcvError) as e:
        pcv.las_write_header(info)
    assert e.value.code == L.PCV_E_INVALID and "2^32 - 1" in str(e.value)


def test_params_refused_with_the_field_they_name():
    extras = dict(gps_time="f64", classification="u8", ring="u16")
    ok = pcv.las_write_check_params(True, extras)
    assert (ok["point_format"], ok["version_minor"], ok["record_length"], ok["header_size"], ok["skipped_extras"]) == (3, 2, 34, 227, 1)
    assert pcv.las_write_check_params(False, dict(nir="u16"))["point_format"] == 8
    assert pcv.las_write_check_params(False, dict(scanner_channel="u8", gps_time="f64"))["point_format"] == 7
    assert pcv.las_write_check_params(False, {})["point_format"] == 2
    assert pcv.las_write_check_params(False, {}, point_format=1, version_minor=4)["header_size"] == 375
    for kw, attrs, word in ((dict(point_format=4), extras, "format 4"), (dict(point_format=5), extras, "format 5"),
                            (dict(point_format=9), extras, "format 9"), (dict(point_format=10), extras, "format 10"),
                            (dict(version_minor=1), extras, "1.1"), (dict(version_minor=3), extras, "1.3"),
                            (dict(point_format=7, version_minor=2), extras, "1.4"), (dict(scale=0.0), extras, "x scale"),
                            (dict(scale=(1.0, -1.0, 1.0)), extras, "y scale"), (dict(scale=(1.0, 1.0, float("inf"))), extras, "z scale"),
                            (dict(offset=(0.0, float("nan"), 0.0)), extras, "y offset"), (dict(), dict(gps_time="f32"), "'gps_time'"),
                            (dict(), dict(nir="u8"), "'nir'"), (dict(fields=["color"], point_format=1), extras, "'color'"),
                            (dict(fields=["gps_time"], point_format=2), extras, "'gps_time'"), (dict(fields=["ring"]), extras, "'ring'"),
                            (dict(fields=["user_data"]), extras, "Data type for attribute 'user_data' not found."),
                            (dict(intensity_scale=float("inf")), extras, "intensity_scale")):
        with pytest.raises(pcv.PcvError) as e:
            pcv.las_write_check_params(True, attrs, **kw)
        assert e.value.code == L.PCV_E_INVALID and word in str(e.value), str(e.value)
    with pytest.raises(pcv.PcvError) as e:
        pcv.las_write_check_params(False, extras, fields=["intensity"])
    assert str(e.value).endswith("Data type for attribute 'intensity' not found.")
    pr, _ = pcv.las_write_params()
    pr.struct_size = 8
    assert L.load_library().pcv_las_write_check_params_host(pr, 0, None, None, 0, None) == L.PCV_E_INVALID


def test_append_check(tmp_path):
    pts = points_of(9, 1, gps_time=np.arange(9.0))
    kw = dict(scale=0.001, offset=(4.2e6, -3.3e6, -50.0))
    recs, info = pcv.las_encode_host(pts, **kw)
    good = pcv.las_write_header(info) + recs.tobytes()
    path = tmp_path / "f.las"
    path.write_bytes(good)
    assert pcv.las_append_check(path, info, **kw) == 9 and pcv.las_append_check(path, info, scale=0.001) == 9  # (auto offset: the file's)
    assert pcv.las_append_check(tmp_path / "missing.las", info, **kw) == 0

    def refused(data, word, **other):
        path.write_bytes(data)
        with pytest.raises(pcv.PcvError) as e:
            pcv.las_append_check(path, dict(info, **other.pop("info", {})), **dict(kw, **other))
        assert e.value.code == L.PCV_E_INVALID and word in str(e.value), str(e.value)

    refused(b"LASX" + good[4:], "signature")
    refused(good, "version", info=dict(version_minor=4))
    refused(good, "format", info=dict(point_format=1))
    refused(good, "x scale", scale=0.01)
    refused(good, "z offset", offset=(4.2e6, -3.3e6, -51.0))
    refused(good[:-1], "length")
    refused(good + b"\0", "length")
    refused(good[:100], "length")
    refused(b"", "signature")
    foreign = LT.las_bytes(2, 3, LT.pack_records(3, LT.random_fields(3, 4, seed=3)), 4, scale=(0.001,) * 3, offset=kw["offset"])
    path.write_bytes(foreign)
    assert pcv.las_append_check(path, info, **kw) == 4  # a file of another writer with this writer's geometry
    refused(LT.las_bytes(2, 3, LT.pack_records(3, LT.random_fields(3, 4, seed=3)), 4, scale=(0.001,) * 3, offset=kw["offset"],
                         offset_to_points=227 + 54), "offset to point data")
    refused(LT.las_bytes(2, 3, LT.pack_records(3, LT.random_fields(3, 4, seed=3), 2), 4, scale=(0.001,) * 3, offset=kw["offset"], extra_bytes=2),
            "record length")
    refused(LT.las_bytes(2, 3, LT.pack_records(3, LT.random_fields(3, 4, seed=3)), 4, scale=(0.001,) * 3, offset=kw["offset"], header_size=230,
                         offset_to_points=230), "header size")
    vlrs = bytearray(good)
    struct.pack_into("<I", vlrs, 100, 1)
    refused(bytes(vlrs), "variable length records")


def test_sanitizer_build_of_the_host_code_runs_clean(tmp_path):
    """csrc/pcv_las_write.cpp, csrc/pcv_las.cpp and tests/las_write_host_driver.cpp as one stand-alone program with ASan and UBSan:
    the encode of every format into buffers of exactly the records' size, the header, and the append check over every truncation
    and every single-byte flip of a small file's header."""
    exe = tmp_path / "las_write_host_driver"
    subprocess.check_call(SANITIZE + ["-I", CSRC, os.path.join(ROOT, "tests", "las_write_host_driver.cpp"), os.path.join(CSRC, "pcv_las_write.cpp"),
                                      os.path.join(CSRC, "pcv_las.cpp"), "-o", str(exe)])
    p = subprocess.run([str(exe), str(tmp_path / "scratch.las")], capture_output=True, text=True)
    assert p.returncode == 0, (p.stdout[-1000:] + p.stderr)[-3000:]
    assert "runtime error" not in p.stderr and "Sanitizer" not in p.stderr, p.stderr[-3000:]
    cases, accepted = (int(t) for t in p.stdout.split() if t.isdigit())
    # The check reads 23 bytes of a 1.2 header (signature 4, version 2, header size 2, offset to point data 4, number of VLRs 4, format
    # 1, record length 2, count 4; scale and offset are the file's to state here): a flip in any other byte leaves an appendable file.
    assert cases == 1 + (227 + 5 * 34) + 227 + 1 and accepted == 1 + (227 - 23)
