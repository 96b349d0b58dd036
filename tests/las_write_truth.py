"""An independent truth for LAS output: the contract's rules restated in numpy — quantise, clamp, mask — into the
field dict that las_truth.pack_records packs from the ASPRS field order, and the header from las_truth.header_dtype with every
field the contract states. No offsets are typed here; tests/test_las_write_cpu.py pins this against two files typed byte by
byte from the specification's offsets."""
import numpy as np

import las_truth as LT

LAS_FIELDS = list(LT.EXTRA_DTYPES)  # the twelve names, in the table's order
AUTO = "auto"


def choose_format(attributes):
    names = set(attributes or {})
    return 8 if "nir" in names else 7 if "scanner_channel" in names else 3 if "gps_time" in names else 2


def choose_minor(fmt, minor=0):
    return minor if minor else (2 if fmt <= 3 else 4)


def floor_min(v):
    """floor of the least value by IEEE total order (a range without rows: 0)."""
    v = np.asarray(v, np.float64)
    if v.size == 0:
        return 0.0
    bits = v.view(np.uint64)
    key = np.where(bits >> np.uint64(63), ~bits, bits | np.uint64(1 << 63))
    return float(np.floor(v[int(np.argmin(key))]))


def quantize(v, offset, scale):
    """-> (X int32 with 0 where out of range, in-range mask)"""
    with np.errstate(all="ignore"):
        q = (np.asarray(v, np.float64) - np.float64(offset)) / np.float64(scale)
        ok = (q > -2147483648.5) & (q < 2147483647.5)
        X = np.where(ok, np.rint(np.where(ok, q, 0.0)), 0.0).astype(np.int64).astype(np.int32)
    return X, ok


def intensity_u16(intensity, scale=1.0):
    with np.errstate(all="ignore"):
        v = np.asarray(intensity, np.float32) * np.float32(scale)
        nan = np.isnan(v)
        clamped = nan | (v < 0) | (v > 65535)
        code = np.rint(np.clip(np.where(nan, np.float32(0), v), np.float32(0), np.float32(65535))).astype(np.uint16)
    return code, clamped


def angle_code(a, modern):
    with np.errstate(all="ignore"):
        a = np.asarray(a, np.float32)
        nan = np.isnan(a)
        r = np.rint(a / np.float32(0.006)) if modern else np.rint(a)
        lo, hi = (-32768, 32767) if modern else (-128, 127)
        return np.where(nan, 0, np.clip(np.where(nan, np.float32(0), r), lo, hi)).astype(np.int16)


def color_u16(c, rule):
    c = np.asarray(c, np.uint16)
    return {"x257": c * np.uint16(257), "shift8": c << np.uint16(8), "rgb8": c}[rule]


def records(points, fmt=AUTO, scale=(0.001,) * 3, offset=None, color="x257", intensity_scale=1.0, fields=None, minor=0):
    """points: dict(x, y, z, color (n, 3) or None, intensity or None, attributes {name: array}) -> (record bytes, info dict)."""
    attrs = dict(points.get("attributes") or {})
    named = {k: v for k, v in attrs.items() if k in LT.EXTRA_DTYPES}
    for k, v in named.items():
        assert np.asarray(v).dtype == np.dtype(LT.EXTRA_DTYPES[k]), k
    if fmt == AUTO:
        fmt = choose_format(named)
    minor = choose_minor(fmt, minor)
    x, y, z = (np.asarray(points[k], np.float64) for k in "xyz")
    n = len(x)
    scale = [float(scale)] * 3 if np.isscalar(scale) else [float(s) for s in scale]
    if offset is None:
        offset = [floor_min(x), floor_min(y), floor_min(z)]
    offset = [float(offset)] * 3 if np.isscalar(offset) else [float(o) for o in offset]
    holds = set(LT.extras_of(fmt))
    want = None if fields is None else set(fields)
    use = lambda name: (want is None or name in want)
    X, okx = quantize(x, offset[0], scale[0])
    Y, oky = quantize(y, offset[1], scale[1])
    Z, okz = quantize(z, offset[2], scale[2])
    ok = okx & oky & okz
    X, Y, Z = (np.where(ok, v, 0).astype(np.int32) for v in (X, Y, Z))
    f = dict(X=X, Y=Y, Z=Z)
    clamped = np.zeros(n, bool)
    f["intensity"] = np.zeros(n, np.uint16)
    if points.get("intensity") is not None and use("intensity"):
        f["intensity"], clamped = intensity_u16(points["intensity"], intensity_scale)
    rgb = np.zeros((n, 3), np.uint16)
    if points.get("color") is not None and fmt in LT.HAS_RGB and use("color"):
        rgb = color_u16(np.asarray(points["color"]).reshape(n, 3), color)
    f["r"], f["g"], f["b"] = rgb[:, 0], rgb[:, 1], rgb[:, 2]

    def col(name, default, dtype):
        if name in named and name in holds and use(name):
            return np.asarray(named[name]).astype(dtype)
        return np.full(n, default, dtype)

    rmask, cmask, fmask = (15, 255, 15) if fmt >= 6 else (7, 31, 7)
    raw = dict(return_number=col("return_number", 1, np.uint8), number_of_returns=col("number_of_returns", 1, np.uint8),
               classification=col("classification", 0, np.uint8), flags=col("classification_flags", 0, np.uint8),
               channel=col("scanner_channel", 0, np.uint8), scan_direction=col("scan_direction_flag", 0, np.uint8),
               edge=col("edge_of_flight_line", 0, np.uint8))
    masks = dict(return_number=rmask, number_of_returns=rmask, classification=cmask, flags=fmask, channel=3 if fmt >= 6 else 0,
                 scan_direction=1, edge=1)
    masked = 0
    for k, v in raw.items():
        masked += int((v > masks[k]).sum())
        f[k] = (v & np.uint8(masks[k])).astype(np.uint8)
    f["user_data"] = col("user_data", 0, np.uint8)
    f["point_source_id"] = col("point_source_id", 0, np.uint16)
    f["scan_angle"] = angle_code(col("scan_angle", 0, np.float32), fmt >= 6)
    f["gps_bits"] = col("gps_time", 0, np.float64).view(np.uint64)
    f["nir"] = col("nir", 0, np.uint16)
    by_return = np.zeros(15, np.uint64)
    for r in range(1, 16):
        by_return[r - 1] = int((f["return_number"] == r).sum())
    mins = [int(v.min()) if n else 0 for v in (X, Y, Z)]
    maxs = [int(v.max()) if n else 0 for v in (X, Y, Z)]
    bounds = []
    for a in range(3):
        bounds += [np.float64(maxs[a]) * np.float64(scale[a]) + np.float64(offset[a]) if n else 0.0,
                   np.float64(mins[a]) * np.float64(scale[a]) + np.float64(offset[a]) if n else 0.0]
    info = dict(point_format=fmt, version_minor=minor, record_length=LT.MIN_LEN[fmt], header_size=LT.HEADER_SIZE[minor], scale=tuple(scale),
                offset=tuple(offset), min_xyz=tuple(mins), max_xyz=tuple(maxs), bounds=tuple(float(b) for b in bounds), num_records=n,
                by_return=by_return, out_of_range=int((~ok).sum()), clamped_intensity=int(clamped.sum()), masked_values=masked,
                skipped_extras=len(attrs) - len(named))
    return LT.pack_records(fmt, f), info


def header(info, file_source_id=0, global_encoding=0, day=0, year=0, system_identifier=b"OTHER", generating_software=b"point_cloud_viewer_amd"):
    minor, fmt, n = info["version_minor"], info["point_format"], info["num_records"]
    h = np.zeros(1, dtype=LT.header_dtype(minor))
    h["signature"], h["file_source_id"], h["global_encoding"] = b"LASF", file_source_id, global_encoding
    h["version_major"], h["version_minor"] = 1, minor
    h["system_identifier"], h["generating_software"], h["day_of_year"], h["year"] = system_identifier, generating_software, day, year
    h["header_size"] = h["offset_to_point_data"] = LT.HEADER_SIZE[minor]
    h["number_of_vlrs"], h["point_format"], h["record_length"] = 0, fmt, LT.MIN_LEN[fmt]
    if fmt <= 5:
        h["legacy_count"] = n
        h["legacy_by_return"] = np.asarray(info["by_return"][:5], np.uint32)
    h["scale"], h["offset"] = info["scale"], info["offset"]
    h["bounds"] = info["bounds"] if n else (0.0,) * 6
    if minor >= 4:
        h["count"] = n
        h["by_return"] = np.asarray(info["by_return"], np.uint64)
    return h.tobytes()


def merge_info(a, b):
    """The header's totals of two record sets under one scale and offset."""
    if a["num_records"] == 0 or b["num_records"] == 0:
        return dict(b if a["num_records"] == 0 else a)
    m = dict(a)
    m["num_records"] = a["num_records"] + b["num_records"]
    m["by_return"] = a["by_return"] + b["by_return"]
    m["bounds"] = tuple(min(u, v) if k & 1 else max(u, v) for k, (u, v) in enumerate(zip(a["bounds"], b["bounds"])))
    return m


def assert_info(got, want, what=""):
    for k in ("point_format", "version_minor", "record_length", "header_size", "min_xyz", "max_xyz", "num_records", "out_of_range",
              "clamped_intensity", "masked_values", "skipped_extras"):
        assert got[k] == want[k], f"{what}: info {k}: {got[k]} != {want[k]}"
    for k in ("scale", "offset", "bounds"):
        assert np.asarray(got[k], np.float64).tobytes() == np.asarray(want[k], np.float64).tobytes(), f"{what}: info {k}: {got[k]} != {want[k]}"
    assert np.array_equal(got["by_return"], want["by_return"]), f"{what}: by_return"
