"""The reference's `Meta` schema (point_viewer_proto_rust/src/proto.proto:27-149) as a protobuf descriptor built at
run time with the REAL protobuf runtime — an independent reader/writer for meta.pb (the library's own writer and
reader are hand-rolled). Field numbers are restated here; `check_against_reference()` re-derives them from the
reference's proto.proto, and tests/golden/reference_proto_schema.json holds the digest of what that file declares
(refresh: python tests/meta_proto.py <reference checkout>/point_viewer_proto_rust/src/proto.proto)."""
import hashlib
import json
import os
import re
import sys

from google.protobuf import descriptor_pb2, descriptor_pool, message_factory

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_proto_schema.json")
_T = descriptor_pb2.FieldDescriptorProto
_SCALAR = {"double": _T.TYPE_DOUBLE, "float": _T.TYPE_FLOAT, "int32": _T.TYPE_INT32, "int64": _T.TYPE_INT64,
           "uint64": _T.TYPE_UINT64, "uint32": _T.TYPE_UINT32, "string": _T.TYPE_STRING}

# message -> [(name, number, type, repeated)]; types: scalar name, or message / enum name
SCHEMA = {
    "Vector3f": [("x", 1, "float", False), ("y", 2, "float", False), ("z", 3, "float", False)],
    "Vector3d": [("x", 1, "double", False), ("y", 2, "double", False), ("z", 3, "double", False)],
    "AxisAlignedCuboid": [("min", 3, "Vector3d", False), ("max", 4, "Vector3d", False),
                          ("deprecated_min", 1, "Vector3f", False), ("deprecated_max", 2, "Vector3f", False)],
    "NodeId": [("high", 3, "uint64", False), ("low", 4, "uint64", False), ("deprecated_level", 1, "int32", False),
               ("deprecated_index", 2, "int64", False)],
    "OctreeNode": [("position_encoding", 2, "PositionEncoding", False), ("num_points", 3, "int64", False),
                   ("id", 4, "NodeId", False)],
    "OctreeMeta": [("resolution", 2, "double", False), ("nodes", 3, "OctreeNode", True),
                   ("deprecated_bounding_box", 1, "AxisAlignedCuboid", False)],
    "S2Cell": [("id", 1, "uint64", False), ("num_points", 2, "uint64", False)],
    "S2Meta": [("cells", 1, "S2Cell", True)],
    "Meta": [("version", 1, "int32", False), ("bounding_box", 4, "AxisAlignedCuboid", False),
             ("octree", 6, "OctreeMeta", False), ("s2", 7, "S2Meta", False),
             ("deprecated_resolution", 3, "double", False), ("deprecated_nodes", 5, "OctreeNode", True)],
}
ENUMS = {"PositionEncoding": [("INVALID", 0), ("Uint8", 1), ("Uint16", 2), ("Float32", 3), ("Float64", 4)]}
ONEOF = {"Meta": ("data", ("octree", "s2"))}

# the xray quadtree's Meta (xray_proto_rust/src/proto.proto:21-54), package xray.proto
XRAY_SCHEMA = {
    "Vector2f": [("x", 1, "float", False), ("y", 2, "float", False)],
    "Vector2d": [("x", 1, "double", False), ("y", 2, "double", False)],
    "Rect": [("min", 3, "Vector2d", False), ("edge_length", 4, "double", False), ("deprecated_min", 1, "Vector2f", False),
             ("deprecated_edge_length", 2, "float", False)],
    "NodeId": [("level", 1, "uint32", False), ("index", 2, "uint64", False)],
    "Meta": [("version", 1, "int32", False), ("bounding_rect", 2, "Rect", False), ("deepest_level", 3, "uint32", False),
             ("tile_size", 4, "uint32", False), ("nodes", 5, "NodeId", True)],
}

_classes = {}


def classes():
    """{message name: generated class} for package point_viewer.proto."""
    return _build("point_viewer.proto", SCHEMA, ENUMS, ONEOF)


def xray_classes():
    """{message name: generated class} for package xray.proto."""
    return _build("xray.proto", XRAY_SCHEMA, {}, {})


def _build(package, SCHEMA, ENUMS, ONEOF):
    if package in _classes:
        return _classes[package]
    fd = descriptor_pb2.FileDescriptorProto()
    fd.name = "pcv_test_%s.proto" % package.replace(".", "_")
    fd.package = package
    fd.syntax = "proto3"
    for ename, values in ENUMS.items():
        e = fd.enum_type.add()
        e.name = ename
        for vname, num in values:
            v = e.value.add()
            v.name, v.number = vname, num
    for mname, fields in SCHEMA.items():
        m = fd.message_type.add()
        m.name = mname
        if mname in ONEOF:
            m.oneof_decl.add().name = ONEOF[mname][0]
        for fname, num, typ, rep in fields:
            f = m.field.add()
            f.name, f.number = fname, num
            f.label = _T.LABEL_REPEATED if rep else _T.LABEL_OPTIONAL
            if typ in _SCALAR:
                f.type = _SCALAR[typ]
            elif typ in ENUMS:
                f.type, f.type_name = _T.TYPE_ENUM, "." + package + "." + typ
            else:
                f.type, f.type_name = _T.TYPE_MESSAGE, "." + package + "." + typ
            if mname in ONEOF and fname in ONEOF[mname][1]:
                f.oneof_index = 0
    pool = descriptor_pool.DescriptorPool()
    pool.Add(fd)
    _classes[package] = {m: message_factory.GetMessageClass(pool.FindMessageTypeByName(package + "." + m)) for m in SCHEMA}
    return _classes[package]


def read_proto(path):
    """The messages of SCHEMA and the enums of ENUMS as a .proto file declares them, in the shape of SCHEMA / ENUMS.
    Of S2Meta only the fields SCHEMA names are kept (its attributes are not part of the octree path)."""
    text = re.sub(r"//[^\n]*", "", open(path).read())
    schema, enums = {}, {}
    for mname, fields in SCHEMA.items():
        body = re.search(r"message\s+%s\s*\{(.*?)\n\}" % mname, text, re.S).group(1)
        found = [(name, int(num), typ, bool(rep))
                 for rep, typ, name, num in re.findall(r"(repeated\s+)?([\w.]+)\s+(\w+)\s*=\s*(\d+)\s*;", body)]
        if mname == "S2Meta":
            found = [f for f in found if f[0] in {g[0] for g in fields}]
        schema[mname] = found
    for ename in ENUMS:
        body = re.search(r"enum\s+%s\s*\{(.*?)\}" % ename, text, re.S).group(1)
        enums[ename] = [(n, int(v)) for n, v in re.findall(r"(\w+)\s*=\s*(\d+)\s*;", body)]
    return schema, enums


def schema_digest(schema, enums):
    """SHA-256 of a (schema, enums) pair shaped like SCHEMA / ENUMS; the order fields are listed in does not count, the
    order of enum values does."""
    canon = ({m: sorted(list(f) for f in fields) for m, fields in schema.items()},
             {e: [list(v) for v in values] for e, values in enums.items()})
    return hashlib.sha256(json.dumps(canon, sort_keys=True).encode()).hexdigest()


def check_against_reference(path):
    """Field numbers / types / labels of SCHEMA and ENUMS against the reference's own proto file
    (point_viewer_proto_rust/src/proto.proto). Returns the number of fields compared."""
    schema, enums = read_proto(path)
    compared = 0
    for mname, fields in SCHEMA.items():
        found = {f[0]: f[1:] for f in schema[mname]}
        for fname, num, typ, rep in fields:
            assert found.get(fname) == (num, typ, rep), (mname, fname, found.get(fname), (num, typ, rep))
            compared += 1
        assert set(found) == {f[0] for f in fields}, (mname, sorted(found))
    for ename, values in ENUMS.items():
        assert enums[ename] == values, (ename, enums[ename])
    return compared


def freeze_reference(path, out=GOLDEN):
    """Check SCHEMA / ENUMS against the reference's proto file and store the digest of what the file declares, so that
    the test can check the schema where the reference is not at hand."""
    compared = check_against_reference(path)
    with open(out, "w") as f:
        json.dump({"source": "point_viewer_proto_rust/src/proto.proto of the reference", "fields": compared,
                   "enum_values": sum(len(v) for v in ENUMS.values()), "sha256": schema_digest(*read_proto(path))}, f, indent=1)
        f.write("\n")
    return compared


def node_id(level, index):
    """(high, low) of NodeId u128 = level << 120 | index (src/octree/node.rs:101-111)."""
    v = (level << 120) | index
    return v >> 64, v & ((1 << 64) - 1)


if __name__ == "__main__":
    print(freeze_reference(sys.argv[1]), "fields checked; digest written to", os.path.relpath(GOLDEN))
