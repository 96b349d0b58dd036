"""An independent truth for LAS input: a numpy writer of LAS 1.0 - 1.4 files in point data record formats 0 - 10 from
structured dtypes that list every field of the ASPRS layouts in order (no offsets are typed here: they follow from the field
sizes), and a numpy restatement of the decode: position, colour rules, extras, filter and info. tests/test_las_cpu.py pins both
against two files built byte by byte from the offsets of the specification."""
import numpy as np

MIN_LEN = [20, 28, 26, 34, 57, 63, 30, 36, 38, 59, 67]
HEADER_SIZE = [227, 227, 227, 235, 375]
HAS_GPS, HAS_RGB, HAS_NIR, HAS_WAVE = {1, 3, 4, 5, 6, 7, 8, 9, 10}, {2, 3, 5, 7, 8, 10}, {8, 10}, {4, 5, 9, 10}
EXTRA_DTYPES = {"classification": "u1", "classification_flags": "u1", "return_number": "u1", "number_of_returns": "u1",
                "scan_direction_flag": "u1", "edge_of_flight_line": "u1", "scanner_channel": "u1", "scan_angle": "<f4",
                "user_data": "u1", "point_source_id": "<u2", "gps_time": "<f8", "nir": "<u2"}
COLOR_RULES = ["auto", "rgb16", "rgb8", "intensity", "constant"]


def extras_of(fmt):
    names = ["classification", "classification_flags", "return_number", "number_of_returns", "scan_direction_flag", "edge_of_flight_line"]
    names += ["scanner_channel"] if fmt >= 6 else []
    names += ["scan_angle", "user_data", "point_source_id"]
    names += ["gps_time"] if fmt in HAS_GPS else []
    return names + (["nir"] if fmt in HAS_NIR else [])


def header_dtype(minor):
    f = [("signature", "S4"), ("file_source_id", "<u2"), ("global_encoding", "<u2"), ("guid", "V16"), ("version_major", "u1"),
         ("version_minor", "u1"), ("system_identifier", "S32"), ("generating_software", "S32"), ("day_of_year", "<u2"), ("year", "<u2"),
         ("header_size", "<u2"), ("offset_to_point_data", "<u4"), ("number_of_vlrs", "<u4"), ("point_format", "u1"),
         ("record_length", "<u2"), ("legacy_count", "<u4"), ("legacy_by_return", "<u4", (5,)), ("scale", "<f8", (3,)),
         ("offset", "<f8", (3,)), ("bounds", "<f8", (6,))]
    if minor >= 3:
        f += [("waveform_start", "<u8")]
    if minor >= 4:
        f += [("first_evlr", "<u8"), ("number_of_evlrs", "<u4"), ("count", "<u8"), ("by_return", "<u8", (15,))]
    dt = np.dtype(f)
    assert dt.itemsize == HEADER_SIZE[minor]
    return dt


def record_dtype(fmt, extra_bytes=0):
    f = [("X", "<i4"), ("Y", "<i4"), ("Z", "<i4"), ("intensity", "<u2")]
    if fmt <= 5:
        f += [("return_byte", "u1"), ("class_byte", "u1"), ("scan_angle", "i1"), ("user_data", "u1"), ("point_source_id", "<u2")]
    else:
        f += [("return_byte", "u1"), ("flag_byte", "u1"), ("classification", "u1"), ("user_data", "u1"), ("scan_angle", "<i2"),
              ("point_source_id", "<u2")]
    if fmt in HAS_GPS:
        f += [("gps_bits", "<u8")]  # the eight bytes of the double, so that NaN payloads survive the trip
    if fmt in HAS_RGB:
        f += [("r", "<u2"), ("g", "<u2"), ("b", "<u2")]
    if fmt in HAS_NIR:
        f += [("nir", "<u2")]
    if fmt in HAS_WAVE:
        f += [("wave", "V29")]
    if extra_bytes:
        f += [("extra", f"V{extra_bytes}")]
    dt = np.dtype(f)
    assert dt.itemsize == MIN_LEN[fmt] + extra_bytes
    return dt


def random_fields(fmt, n, seed=0, gps_specials=True):
    """Logical fields of n records; the corners of every field's range occur."""
    rng = np.random.default_rng(seed)
    f = dict(X=rng.integers(-2**31, 2**31, n, dtype=np.int64).astype(np.int32), Y=rng.integers(-10**7, 10**7, n).astype(np.int32),
             Z=rng.integers(-10**5, 10**5, n).astype(np.int32), intensity=rng.integers(0, 65536, n).astype(np.uint16),
             return_number=rng.integers(0, 8 if fmt <= 5 else 16, n).astype(np.uint8),
             number_of_returns=rng.integers(0, 8 if fmt <= 5 else 16, n).astype(np.uint8),
             scan_direction=rng.integers(0, 2, n).astype(np.uint8), edge=rng.integers(0, 2, n).astype(np.uint8),
             classification=rng.integers(0, 32 if fmt <= 5 else 256, n).astype(np.uint8),
             flags=rng.integers(0, 8 if fmt <= 5 else 16, n).astype(np.uint8), channel=rng.integers(0, 4 if fmt >= 6 else 1, n).astype(np.uint8),
             user_data=rng.integers(0, 256, n).astype(np.uint8),
             scan_angle=rng.integers(-128, 128, n).astype(np.int16) if fmt <= 5 else rng.integers(-32768, 32768, n).astype(np.int16),
             point_source_id=rng.integers(0, 65536, n).astype(np.uint16),
             gps_bits=(rng.random(n) * 4e8).view(np.uint64), r=rng.integers(0, 65536, n).astype(np.uint16),
             g=rng.integers(0, 65536, n).astype(np.uint16), b=rng.integers(0, 65536, n).astype(np.uint16),
             nir=rng.integers(0, 65536, n).astype(np.uint16))
    if n >= 2:
        f["X"][0], f["X"][1] = -2**31, 2**31 - 1
    if gps_specials and n >= 6:
        f["gps_bits"][2:6] = [0x7ff8000000000001, 0xfff0dead0000beef, 0x8000000000000000, 0x7ff0000000000000]  # NaN payloads, -0.0, inf
    return f


def pack_records(fmt, f, extra_bytes=0, filler=0xA5):
    n = len(f["X"])
    rec = np.zeros(n, dtype=record_dtype(fmt, extra_bytes))
    for k in ("X", "Y", "Z", "intensity", "user_data", "point_source_id"):
        rec[k] = f[k]
    if fmt <= 5:
        rec["return_byte"] = f["return_number"] | (f["number_of_returns"] << 3) | (f["scan_direction"] << 6) | (f["edge"] << 7)
        rec["class_byte"] = f["classification"] | (f["flags"] << 5)
        rec["scan_angle"] = f["scan_angle"].astype(np.int8)
    else:
        rec["return_byte"] = f["return_number"] | (f["number_of_returns"] << 4)
        rec["flag_byte"] = f["flags"] | (f["channel"] << 4) | (f["scan_direction"] << 6) | (f["edge"] << 7)
        rec["classification"] = f["classification"]
        rec["scan_angle"] = f["scan_angle"]
    for k in ("gps_bits", "r", "g", "b", "nir"):
        if k in rec.dtype.names:
            rec[k] = f[k]
    for k in ("wave", "extra"):
        if k in rec.dtype.names:
            rec[k] = np.full(rec.dtype[k].itemsize, filler, np.uint8).tobytes()
    return rec.tobytes()


def las_bytes(minor, fmt, records, n, scale=(0.01, 0.01, 0.01), offset=(0.0, 0.0, 0.0), extra_bytes=0, header_size=None,
              offset_to_points=None, tail=b"", legacy_count=None, count64=None, format_byte=None, major=1):
    """A whole file: header (padded to header_size with 0x5A), VLR bytes (0xC3) up to offset_to_points, records, trailing bytes."""
    hs = HEADER_SIZE[minor] if header_size is None else header_size
    otp = hs if offset_to_points is None else offset_to_points
    h = np.zeros(1, dtype=header_dtype(minor))
    h["signature"], h["version_major"], h["version_minor"] = b"LASF", major, minor
    h["header_size"], h["offset_to_point_data"] = hs, otp
    h["point_format"] = fmt if format_byte is None else format_byte
    h["record_length"] = MIN_LEN[fmt] + extra_bytes
    h["legacy_count"] = (n if (minor < 4 or fmt <= 5) else 0) if legacy_count is None else legacy_count
    if minor >= 4:
        h["count"] = n if count64 is None else count64
    h["scale"], h["offset"] = scale, offset
    head = h.tobytes()
    head += b"\x5a" * (hs - len(head))
    return head[:hs] + b"\xc3" * (otp - hs) + records + tail


def write_las(path, minor, fmt, fields, extra_bytes=0, **kw):
    data = las_bytes(minor, fmt, pack_records(fmt, fields, extra_bytes), len(fields["X"]), extra_bytes=extra_bytes, **kw)
    with open(path, "wb") as fh:
        fh.write(data)
    return data


def decode(raw, fmt, stride, scale, offset, color="auto", classes=None, drop_withheld=False, keep_intensity=False, extras=(),
           global_from_local=None):
    """The contract restated in numpy over raw record bytes -> the dict read_las returns."""
    rec = np.frombuffer(raw, dtype=record_dtype(fmt, stride - MIN_LEN[fmt]))
    n = len(rec)
    if fmt <= 5:
        rb, cb = rec["return_byte"], rec["class_byte"]
        col = dict(classification=cb & 31, classification_flags=cb >> 5, return_number=rb & 7, number_of_returns=(rb >> 3) & 7,
                   scan_direction_flag=(rb >> 6) & 1, edge_of_flight_line=rb >> 7, scan_angle=rec["scan_angle"].astype(np.float32))
    else:
        rb, fb = rec["return_byte"], rec["flag_byte"]
        col = dict(classification=rec["classification"], classification_flags=fb & 15, return_number=rb & 15, number_of_returns=rb >> 4,
                   scanner_channel=(fb >> 4) & 3, scan_direction_flag=(fb >> 6) & 1, edge_of_flight_line=fb >> 7,
                   scan_angle=rec["scan_angle"].astype(np.float32) * np.float32(0.006))
    col["user_data"], col["point_source_id"] = rec["user_data"], rec["point_source_id"]
    if fmt in HAS_GPS:
        col["gps_time"] = rec["gps_bits"].view(np.float64)
    if fmt in HAS_NIR:
        col["nir"] = rec["nir"]
    inten = rec["intensity"]
    has_rgb = fmt in HAS_RGB
    rgb = np.stack([rec["r"], rec["g"], rec["b"]], axis=1).astype(np.uint32) if has_rgb else np.zeros((n, 3), np.uint32)
    max_color = int(rgb.max()) if n and has_rgb else 0
    max_intensity = int(inten.max()) if n else 0
    withheld = (col["classification_flags"] >> 2) & 1
    by_class = np.ones(n, bool) if classes is None else np.isin(col["classification"], np.asarray(list(classes), np.uint8))
    keep = by_class & ~(withheld.astype(bool) & bool(drop_withheld))
    rule = color if isinstance(color, str) else "constant"
    if rule == "auto":
        rule = "intensity" if not has_rgb else ("rgb16" if max_color > 255 else "rgb8")
    if rule in ("rgb16", "rgb8") and not has_rgb:
        raise ValueError("no colour in this format")
    if rule == "rgb16":
        c = rgb >> 8
    elif rule == "rgb8":
        c = np.minimum(rgb, 255)
    elif rule == "intensity":
        v = (inten.astype(np.uint32) * 255 // max_intensity) if max_intensity else np.zeros(n, np.uint32)
        c = np.stack([v, v, v], axis=1)
    else:
        c = np.tile(np.asarray(color, np.uint32), (n, 1))
    x = rec["X"].astype(np.float64) * scale[0] + offset[0]
    y = rec["Y"].astype(np.float64) * scale[1] + offset[1]
    z = rec["Z"].astype(np.float64) * scale[2] + offset[2]
    if global_from_local is not None:  # Isometry3 * Point3 as pcv_transform_points computes it: v + w t + q x t, t = 2 (q x v)
        t0, t1, t2, qx, qy, qz, qw = (np.float64(v) for v in global_from_local)
        tx, ty, tz = (qy * z - qz * y) * 2.0, (qz * x - qx * z) * 2.0, (qx * y - qy * x) * 2.0
        cx, cy, cz = qy * tz - qz * ty, qz * tx - qx * tz, qx * ty - qy * tx
        x, y, z = ((tx * qw + cx) + x) + t0, ((ty * qw + cy) + y) + t1, ((tz * qw + cz) + z) + t2
    info = dict(num_records=n, num_kept=int(keep.sum()), dropped_class=int((~by_class).sum()), dropped_withheld=int((by_class & ~keep).sum()),
                max_color=max_color, max_intensity=max_intensity, color_rule=rule,
                class_hist=np.bincount(col["classification"], minlength=256).astype(np.uint64),
                return_hist=np.bincount(col["return_number"], minlength=16).astype(np.uint64),
                flag_counts=dict(zip(("synthetic", "key_point", "withheld", "overlap"),
                                     (int(((col["classification_flags"] >> b) & 1).sum()) for b in range(4)))))
    for name in extras:
        if name not in col:
            raise KeyError(name)
    return dict(x=x[keep], y=y[keep], z=z[keep], color=c[keep].astype(np.uint8), intensity=inten[keep].astype(np.float32) if keep_intensity else None,
                attributes={name: np.ascontiguousarray(col[name][keep]).astype(EXTRA_DTYPES[name]) for name in extras}, info=info)


def same_bits(a, b):
    """Equal as bytes: NaN payloads and -0.0 count."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype.itemsize == b.dtype.itemsize and a.shape == b.shape and a.tobytes() == b.tobytes()


def assert_same(got, want, what=""):
    """read_las's dict against the truth's, bit for bit; info without the piece count."""
    for k in ("x", "y", "z", "color"):
        assert same_bits(got[k], want[k]), f"{what}: column {k}"
    assert (got["intensity"] is None) == (want["intensity"] is None), f"{what}: intensity presence"
    if want["intensity"] is not None:
        assert same_bits(got["intensity"], want["intensity"]), f"{what}: intensity"
    assert list(got["attributes"]) == list(want["attributes"]), f"{what}: attribute names"
    for k in want["attributes"]:
        assert same_bits(got["attributes"][k], want["attributes"][k]), f"{what}: attribute {k}"
    gi, wi = got["info"], want["info"]
    for k in ("num_records", "num_kept", "dropped_class", "dropped_withheld", "max_color", "max_intensity", "color_rule", "flag_counts"):
        assert gi[k] == wi[k], f"{what}: info {k}: {gi[k]} != {wi[k]}"
    assert np.array_equal(gi["class_hist"], wi["class_hist"]) and np.array_equal(gi["return_hist"], wi["return_hist"]), f"{what}: histograms"
