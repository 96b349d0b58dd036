"""An independent restatement of the 3D Tiles export in numpy, struct.pack and exact rational arithmetic: every
.pnts file and the tileset from node tables and node bytes. Nothing here calls the library. A node is a dict with id (high,
low), level, num_points, encoding, cube_min, cube_edge (and xyz / rgb / intensity bytes where a file is made)."""
import json
import struct
from fractions import Fraction

import numpy as np

U8, U16, F32, F64 = 1, 2, 3, 4
SRC_DTYPE = {U8: "u1", U16: "<u2", F32: "<f4", F64: "<f8"}
BATCH_JSON = '{"INTENSITY":{"byteOffset":0,"componentType":"FLOAT","type":"SCALAR"}}'
DEFAULT_ERROR_FACTOR = 0.0625


def f64(v):
    """The shortest of %.15g .. %.17g that reads back as v, ".0" after an integral value."""
    v = float(v)
    for digits in (15, 16, 17):
        s = "%.*g" % (digits, v)
        if float(s) == v:
            break
    return s if any(c in s for c in ".en") else s + ".0"


def vec(a):
    return "[" + ",".join(f64(v) for v in a) + "]"


def rtc(node):
    """(double)(float)(min + edge / 2) per axis."""
    c = np.asarray(node["cube_min"], dtype=np.float64) + np.float64(node["cube_edge"]) / 2.0
    return c.astype(np.float32).astype(np.float64)


def mode_of(position_mode, encoding):
    if position_mode != "auto":
        return position_mode
    return "quantized" if encoding in (U8, U16) else "float"


def fma(u, edge, mn):
    """round(u * edge + mn) with one rounding, per element: exact in rationals, rounded once by float()."""
    e, m = Fraction(float(edge)), Fraction(float(mn))
    return np.array([float(Fraction(float(v)) * e + m) for v in u], dtype=np.float64)


def positions(node, mode):
    """The feature binary's positions: uint16 [n, 3] or float32 [n, 3]."""
    enc = node["encoding"]
    raw = np.frombuffer(node["xyz"], dtype=SRC_DTYPE[enc]).reshape(-1, 3)
    if mode == "quantized":
        if enc == U8:
            return (raw.astype(np.uint32) * 257).astype("<u2")
        if enc == U16:
            return raw.astype("<u2")
        return np.trunc(np.float64(65535.0) * raw.astype(np.float64)).astype(np.int64).astype("<u2")
    unit = raw.astype(np.float64) / 255.0 if enc == U8 else raw.astype(np.float64) / 65535.0 if enc == U16 else raw.astype(np.float64)
    rc = rtc(node)
    out = np.zeros(raw.shape, dtype="<f4")
    for a in range(3):
        out[:, a] = (fma(unit[:, a], node["cube_edge"], node["cube_min"][a]) - rc[a]).astype(np.float32)
    return out


def feature_json(node, mode):
    """Without its padding."""
    n, rc = node["num_points"], rtc(node)
    s = '{"POINTS_LENGTH":%d,"RTC_CENTER":%s' % (n, vec(rc))
    if mode == "quantized":
        off = np.asarray(node["cube_min"], dtype=np.float64) - rc
        s += ',"QUANTIZED_VOLUME_OFFSET":%s,"QUANTIZED_VOLUME_SCALE":%s,"POSITION_QUANTIZED":{"byteOffset":0}' % (vec(off), vec([node["cube_edge"]] * 3))
        return s + ',"RGB":{"byteOffset":%d}}' % (6 * n)
    return s + ',"POSITION":{"byteOffset":0},"RGB":{"byteOffset":%d}}' % (12 * n)


def pad(b, fill, start=0):
    return b + fill * (-(start + len(b)) % 8)


def tile_file(node, position_mode="auto", intensity=False):
    """The complete .pnts file and dict(mode, feature_json_len: the unpadded length, offsets of the four sections)."""
    mode = mode_of(position_mode, node["encoding"])
    fj = pad(feature_json(node, mode).encode(), b" ", 28)
    fb = pad(positions(node, mode).tobytes() + bytes(node["rgb"]), b"\0")
    bj = pad(BATCH_JSON.encode(), b" ") if intensity else b""
    bb = pad(bytes(node["intensity"]), b"\0") if intensity else b""
    total = 28 + len(fj) + len(fb) + len(bj) + len(bb)
    head = b"pnts" + struct.pack("<6I", 1, total, len(fj), len(fb), len(bj), len(bb))
    plan = dict(mode=mode, feature_json_len=len(feature_json(node, mode)), file_bytes=total, feature_json_offset=28,
                feature_binary_offset=28 + len(fj), batch_json_offset=28 + len(fj) + len(fb), batch_binary_offset=28 + len(fj) + len(fb) + len(bj))
    return head + fj + fb + bj + bb, plan


def node_index(node):
    hi, lo = node["id"]
    return ((hi & ((1 << 56) - 1)) << 64) | lo


def node_name(node):
    idx = node_index(node)
    return "r" + "".join(str((idx >> (3 * j)) & 7) for j in range(node["level"] - 1, -1, -1))


def tileset(nodes, error_factor=DEFAULT_ERROR_FACTOR, transform=None):
    """tileset.json of a node table (any order): the text, and the names of the content tiles in (level, index) order."""
    by_key = {(n["level"], node_index(n)): n for n in nodes}
    kids = {k: [] for k in by_key}
    for (level, idx) in sorted(by_key):
        if level:
            kids[(level - 1, idx >> 3)].append((level, idx))

    def subtree(k):
        return by_key[k]["num_points"] + sum(subtree(c) for c in kids[k])

    def tile(k, root):
        n = by_key[k]
        h = np.float64(n["cube_edge"]) / 2.0
        c = np.asarray(n["cube_min"], dtype=np.float64) + h
        ch = [c2 for c2 in sorted(kids[k]) if subtree(c2) > 0]
        g = np.float64(n["cube_edge"]) * np.float64(error_factor) if ch else 0.0
        s = '{"boundingVolume":{"box":[%s,%s,%s,%s,0.0,0.0,0.0,%s,0.0,0.0,0.0,%s]},"geometricError":%s' % (f64(c[0]), f64(c[1]), f64(c[2]), f64(h), f64(h), f64(h), f64(g))
        if root:
            s += ',"refine":"ADD"'
            if transform is not None and any(float(v) != 0.0 for v in transform):
                s += ',"transform":' + vec(transform)
        if n["num_points"] > 0:
            s += ',"content":{"uri":"%s.pnts"}' % node_name(n)
        if ch:
            s += ',"children":[' + ",".join(tile(c2, False) for c2 in ch) + "]"
        return s + "}"

    root = by_key[(0, 0)]
    text = '{"asset":{"version":"1.0"},"geometricError":%s,"root":%s}' % (f64(root["cube_edge"]), tile((0, 0), True))
    return text, [node_name(by_key[k]) for k in sorted(by_key) if by_key[k]["num_points"] > 0]


def check_structure(text):
    """json.loads of a tileset has the stated structure, and every child's box lies inside its parent's. Returns the number of
    tiles and of content tiles."""
    doc = json.loads(text)
    assert list(doc) == ["asset", "geometricError", "root"] and doc["asset"] == {"version": "1.0"}
    count = [0, 0]

    def walk(t, parent_box, root):
        keys = list(t)
        want = ["boundingVolume", "geometricError"] + (["refine"] if root else [])
        assert keys[:len(want)] == want and all(k in ("transform", "content", "children") for k in keys[len(want):]), keys
        assert ("transform" not in t or root) and (not root or t["refine"] == "ADD")
        box = t["boundingVolume"]["box"]
        assert len(box) == 12 and box[3] == box[7] == box[11] > 0 and [box[i] for i in (4, 5, 6, 8, 9, 10)] == [0.0] * 6
        if parent_box is not None:
            for a in range(3):
                assert parent_box[a] - parent_box[3] <= box[a] - box[3] and box[a] + box[3] <= parent_box[a] + parent_box[3], (parent_box, box)
        count[0] += 1
        count[1] += "content" in t
        assert "children" in t or t["geometricError"] == 0.0
        assert "content" in t or "children" in t  # a tile without content has non-empty descendants
        for c in t.get("children", []):
            walk(c, box, False)

    walk(doc["root"], None, True)
    return tuple(count)


# ---- scenes ------------------------------------------------------------------------------------------------------------------
def scene_a():
    """20 003 points in the unit cube, denser towards the origin by powers of two: 164 nodes down to level 21 with all four
    encodings. Returns dict(x, y, z, rgb, intensity, bmin, bmax, resolution, cap)."""
    rng = np.random.default_rng(7)
    n = 20000
    k = np.arange(n) % 24
    p = rng.random((n, 3)) * 2.0 ** -k[:, None]
    p[k == 0] *= 0.5
    p = np.concatenate([p, np.array([[0.9, 0.9, 0.9], [0.9, 0.1, 0.1], [0.8, 0.2, 0.2]])])
    rgb = rng.integers(0, 256, (len(p), 3), dtype=np.uint8)
    inten = (rng.random(len(p)) * 1000.0 - 300.0).astype(np.float32)
    return dict(x=p[:, 0].copy(), y=p[:, 1].copy(), z=p[:, 2].copy(), rgb=rgb, intensity=inten, bmin=np.zeros(3), bmax=np.ones(3),
                resolution=2.0 ** -24.5, cap=3000)


ECEF_OFFSET = np.array([4_000_000.0, 500_000.0, 4_930_000.0])  # |.| = 6.37e6


def scene_e():
    """Scene A times 1 000 at an Earth-fixed offset; the box is exactly the moved cube."""
    s = scene_a()
    for a, key in enumerate("xyz"):
        s[key] = s[key] * 1000.0 + ECEF_OFFSET[a]
    s.update(bmin=ECEF_OFFSET.copy(), bmax=ECEF_OFFSET + 1000.0, resolution=1000.0 * 2.0 ** -24.5)
    return s


def scene_k():
    """The shape of the reference's own unit-test cloud at 100 points a node: r, r0 (0 points) and r4."""
    n = 101
    x, y, z = np.zeros(n), np.zeros(n), np.zeros(n)
    x[-1], y[-1], z[-1] = -200.0, -40.0, 30.0
    rng = np.random.default_rng(3)
    return dict(x=x, y=y, z=z, rgb=rng.integers(0, 256, (n, 3), dtype=np.uint8), intensity=rng.random(n).astype(np.float32),
                bmin=np.array([-200.0, -40.0, 0.0]), bmax=np.array([0.0, 0.0, 30.0]), resolution=1.0, cap=100)


SCENES = {"A": scene_a, "E": scene_e, "K": scene_k}


def oracle_nodes(scene, O):
    """The scene's octree by the CPU oracle (O: tests/oracle_lib) as a list of node dicts in (level, index) order."""
    with O.max_points_per_node(scene["cap"]):
        t = O.build_closed(scene["resolution"], scene["bmin"], scene["bmax"], scene["x"], scene["y"], scene["z"], scene["rgb"], scene["intensity"], threads=4)
    root_edge = float(np.max(scene["bmax"] - scene["bmin"]))
    nodes = []
    for name in t.order:
        nd = t.nodes[name]
        mn, edge = O.find_bounding_cube(nd["id"][0], nd["id"][1], scene["bmin"], root_edge)
        nodes.append(dict(name=name, id=nd["id"], level=nd["level"], num_points=nd["num_points"], encoding=nd["encoding"],
                          cube_min=tuple(float(v) for v in mn), cube_edge=float(edge), xyz=nd["xyz"], rgb=nd["rgb"], intensity=nd["intensity"]))
    nodes.sort(key=lambda n: (n["level"], node_index(n)))
    return nodes
