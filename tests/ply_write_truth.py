"""An independent restatement of the PLY that write_ply writes (PlyNodeWriter with Encoding::Plain, reference
src/read_write/ply.rs:559-732), for the tests to compare bytes with: the header is a string built from the rules of the format,
a row is a numpy structured dtype with align=False, and the rows come from points() / attribute() of the same batch. Nothing
here calls the library's layout, header or row functions."""
import numpy as np

# type string -> (PLY type word (ply.rs:582-593), numpy dtype, components)
TYPES = {"u8": ("uchar", "u1", 1), "u16": ("ushort", "<u2", 1), "u32": ("uint", "<u4", 1), "u64": ("ulonglong", "<u8", 1),
         "i8": ("char", "i1", 1), "i16": ("short", "<i2", 1), "i32": ("int", "<i4", 1), "i64": ("longlong", "<i8", 1),
         "f32": ("float", "<f4", 1), "f64": ("double", "<f8", 1), "u8vec3": ("uchar", "u1", 3), "f64vec3": ("double", "<f8", 3)}
START = b"ply\nformat binary_little_endian 1.0\nelement vertex "  # HEADER_START_TO_NUM_VERTICES (ply.rs:32-33)
DIGITS = 20  # HEADER_NUM_VERTICES (ply.rs:34)


def in_row_order(attrs):
    """attrs: dict name -> type string. BTreeMap<String, _> iterates in ascending byte order of the keys."""
    return sorted(attrs.items(), key=lambda kv: kv[0].encode())


def property_names(name, comps):
    if name == "color":
        return ["red", "green", "blue"][:comps]
    return [f"{name}{i}" for i in range(comps)] if comps > 1 else [name]


def header(attrs, count):
    lines = ["property double x", "property double y", "property double z"]
    for name, typ in in_row_order(attrs):
        word, _, comps = TYPES[typ]
        lines += [f"property {word} {p}" for p in property_names(name, comps)]
    return START + b"%0*d\n" % (DIGITS, count) + "".join(l + "\n" for l in lines).encode() + b"end_header\n"


def row_dtype(attrs):
    fields = [("x", "<f8"), ("y", "<f8"), ("z", "<f8")]
    for name, typ in in_row_order(attrs):
        _, dt, comps = TYPES[typ]
        fields += [(p, dt) for p in property_names(name, comps)]
    return np.dtype(fields, align=False)


def stride(attrs):
    return 24 + sum(np.dtype(TYPES[t][1]).itemsize * TYPES[t][2] for t in attrs.values())


def rows(points, columns, attrs):
    """points: what QueryBatch.points returns; columns: name -> array for every extra named in attrs. The packed rows, (n, stride) u8."""
    n = int(points["count"])
    out = np.zeros(n, dtype=row_dtype(attrs))
    for axis in "xyz":
        out[axis] = points[axis]
    for name, typ in attrs.items():
        comps = TYPES[typ][2]
        col = points["rgb"].reshape(-1, 3) if name == "color" else points["intensity"] if name == "intensity" else columns[name]
        for i, p in enumerate(property_names(name, comps)):
            # a view of the same bits: NaN payloads and -0.0 must not pass through a float conversion
            out[p] = col[:, i] if comps > 1 else col
    assert out.dtype.itemsize == stride(attrs)
    return out.view(np.uint8).reshape(n, stride(attrs))


def file_bytes(attrs, row_blocks):
    """The file after one write per block of rows (truncate, then appends): one header with the total, the rows, one newline."""
    body = b"".join(np.ascontiguousarray(r).tobytes() for r in row_blocks)
    return header(attrs, sum(len(r) for r in row_blocks)) + body + b"\n"
