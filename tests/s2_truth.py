"""An independent restatement of the S2 cell chain of DESIGN §9c in plain Python: ints and math.sqrt, one correctly rounded
f64 operation per step. It never calls the library; test_s2_cpu.py and test_gpu_s2.py compare the library against it.

The Hilbert curve here walks the 1 024-entry lookup table of the public S2 definition in eight 4-bit steps (the library
takes thirty 2-bit steps without a table), and the inverse (`face_ij`) walks the curve one level at a time."""
import functools
import math
import struct

import numpy as np

MAX_LEVEL = 30
MAX_SIZE = 1 << MAX_LEVEL
RADIUS_MAX_M = 6384400.0  # EARTH_RADIUS_MAX_M (src/math/mod.rs)
RADIUS_MIN_M = 6352800.0  # EARTH_RADIUS_MIN_M
POS_TO_IJ = ((0, 1, 3, 2), (0, 2, 3, 1), (3, 2, 0, 1), (3, 1, 0, 2))
POS_TO_ORIENTATION = (1, 0, 0, 3)
U8VEC3, F32 = 27, 11  # proto AttributeDataType


def _build_lookup():
    lookup = [0] * 1024

    def cell(level, i, j, orig, pos, orientation):
        if level == 4:
            lookup[(((i << 4) + j) << 2) + orig] = (pos << 2) + orientation
            return
        r = POS_TO_IJ[orientation]
        for k in range(4):
            cell(level + 1, (i << 1) + (r[k] >> 1), (j << 1) + (r[k] & 1), orig, (pos << 2) + k,
                 orientation ^ POS_TO_ORIENTATION[k])

    for orig in range(4):
        cell(0, 0, 0, orig, 0, orig)
    return lookup


LOOKUP_POS = _build_lookup()


def face_uv(x, y, z):
    """Steps 1-3: normalise, face (ties to the later axis), (u, v)."""
    n2 = x * x + y * y + z * z
    r = 1.0 / math.sqrt(n2) if n2 > 0.0 else math.inf
    x, y, z = x * r, y * r, z * r
    ax, ay, az = abs(x), abs(y), abs(z)
    if ax > ay:
        axis = 0 if ax > az else 2
    else:
        axis = 1 if ay > az else 2
    face = axis + (3 if (x, y, z)[axis] < 0.0 else 0)
    if axis == 0:
        u, v = (y / x, z / x) if face == 0 else (z / x, y / x)
    elif axis == 1:
        u, v = (-x / y, z / y) if face == 1 else (z / y, -x / y)
    else:
        u, v = (-x / z, -y / z) if face == 2 else (-y / z, -x / z)
    return face, u, v


def uv_to_st(u):
    return 0.5 * math.sqrt(1.0 + 3.0 * u) if u >= 0.0 else 1.0 - 0.5 * math.sqrt(1.0 - 3.0 * u)


def st_to_ij(s):
    if not s > 0.0:  # zero, negative or NaN
        return 0
    return min(MAX_SIZE - 1, math.floor(MAX_SIZE * s))


def leaf_from_face_ij(face, i, j):
    n = face << 60
    bits = face & 1
    for k in range(7, -1, -1):
        bits += ((i >> (k * 4)) & 15) << 6
        bits += ((j >> (k * 4)) & 15) << 2
        bits = LOOKUP_POS[bits]
        n |= (bits >> 2) << (k * 8)
        bits &= 3
    return ((n << 1) | 1) & 0xFFFFFFFFFFFFFFFF


def leaf_id(x, y, z):
    face, u, v = face_uv(x, y, z)
    return leaf_from_face_ij(face, st_to_ij(uv_to_st(u)), st_to_ij(uv_to_st(v)))


def lsb_for_level(level):
    return 1 << (2 * (MAX_LEVEL - level))


def parent(cell, level):
    lsb = lsb_for_level(level)
    return (cell & -lsb & 0xFFFFFFFFFFFFFFFF) | lsb


def range_min(cell):
    return cell - ((cell & -cell) - 1)


def range_max(cell):
    return cell + ((cell & -cell) - 1)


def token(cell):
    if cell == 0:
        return "X"
    return f"{cell:016x}".rstrip("0")


def face_ij(leaf):
    """Inverse of leaf_from_face_ij, one level at a time."""
    face = leaf >> 61
    pos = (leaf >> 1) & ((1 << 60) - 1)
    orientation = face & 1
    i = j = 0
    for level in range(MAX_LEVEL):
        p = (pos >> (2 * (MAX_LEVEL - 1 - level))) & 3
        ij = POS_TO_IJ[orientation][p]
        i = (i << 1) | (ij >> 1)
        j = (j << 1) | (ij & 1)
        orientation ^= POS_TO_ORIENTATION[p]
    return face, i, j


def valid_ecef(x, y, z):
    if x != x or y != y or z != z:
        return False
    radius = math.sqrt(x * x + y * y + z * z)
    return not (radius > RADIUS_MAX_M or radius < RADIUS_MIN_M)


def union_contains(cells, leaf):
    """CellUnion::contains_cellid over an ascending list of cell ids."""
    lo, hi = 0, len(cells)
    while lo < hi:  # first cell with id >= leaf
        mid = (lo + hi) // 2
        if cells[mid] < leaf:
            lo = mid + 1
        else:
            hi = mid
    if lo < len(cells) and range_min(cells[lo]) <= leaf:
        return True
    return lo > 0 and range_max(cells[lo - 1]) >= leaf


def leaf_ids(x, y, z):
    return np.array([leaf_id(a, b, c) for a, b, c in zip(np.asarray(x).tolist(), np.asarray(y).tolist(), np.asarray(z).tolist())],
                    dtype=np.uint64)


def parents(ids, level):
    lsb = np.uint64(lsb_for_level(level))
    return (np.asarray(ids, dtype=np.uint64) & (~lsb + np.uint64(1))) | lsb


def from_lat_lng_deg(lat, lng):
    """S2 LatLng -> unit vector (the known answers of the S2 test suites are given this way)."""
    phi, theta = math.radians(lat), math.radians(lng)
    return math.cos(phi) * math.cos(theta), math.cos(phi) * math.sin(theta), math.sin(phi)


def split(x, y, z, level):
    """What S2Splitter::write leaves behind, as arrays: ascending cell ids, their counts, and the stable order."""
    cells = parents(leaf_ids(x, y, z), level)
    order = np.argsort(cells, kind="stable")
    ids, counts = np.unique(cells, return_counts=True)
    return ids, counts.astype(np.uint64), order.astype(np.uint32)


# ---- point sets shared by the CPU and the GPU tests (built once) --------------------------------------------------------
def _ulp_step(v, k):
    bits = struct.unpack("<q", struct.pack("<d", v))[0]
    bits += k if v >= 0.0 else -k
    return struct.unpack("<d", struct.pack("<q", bits))[0]


def _st_to_uv(s):
    return (4.0 * s * s - 1.0) / 3.0 if s >= 0.5 else (1.0 - 4.0 * (1.0 - s) * (1.0 - s)) / 3.0


def _face_uv_to_xyz(face, u, v):
    return ((1.0, u, v), (-u, 1.0, v), (-u, -v, 1.0), (-1.0, -v, -u), (v, -1.0, -u), (v, u, -1.0))[face]


@functools.lru_cache(maxsize=None)
def shell_points(n=3000, seed=5):
    """Points all over the sphere at Earth radius: every face gets a share."""
    rng = np.random.Generator(np.random.PCG64(seed))
    p = rng.standard_normal((n, 3))
    p *= (6.371e6 + rng.uniform(-5000.0, 5000.0, n))[:, None] / np.linalg.norm(p, axis=1)[:, None]
    return np.ascontiguousarray(p[:, 0]), np.ascontiguousarray(p[:, 1]), np.ascontiguousarray(p[:, 2])


@functools.lru_cache(maxsize=None)
def tie_points():
    """|x| == |y|, |y| == |z|, |x| == |z|, all three equal, every sign pattern, a third component above and below."""
    r = 6.371e6
    pts = []
    for sx in (-1.0, 1.0):
        for sy in (-1.0, 1.0):
            for sz in (-1.0, 1.0):
                pts.append((sx * r, sy * r, sz * r))
                for small in (0.25, 0.999999, 1.0, 1.000001, 1.75):
                    pts.append((sx * r, sy * r, sz * r * small))
                    pts.append((sx * r * small, sy * r, sz * r))
                    pts.append((sx * r, sy * r * small, sz * r))
    p = np.array(pts)
    return np.ascontiguousarray(p[:, 0]), np.ascontiguousarray(p[:, 1]), np.ascontiguousarray(p[:, 2])


@functools.lru_cache(maxsize=None)
def edge_points(seed=9, random_k=20, level20_k=20):
    """Points within two ulps of a cell edge: s = k / 2^30 for random k and for k a multiple of 2^10 (a level-20 edge), inverted
    to u, placed on every face at a radius of about 6.37e6 (v random), each coordinate moved by 0, +-1, +-2 ulp."""
    rng = np.random.Generator(np.random.PCG64(seed))
    ks = [int(k) for k in rng.integers(1, MAX_SIZE, random_k)] + [int(k) << 10 for k in rng.integers(1, 1 << 20, level20_k)]
    steps = (-2, -1, 0, 1, 2)
    pts = []
    for k in ks:
        u = _st_to_uv(k / MAX_SIZE)
        v = _st_to_uv(float(rng.uniform(0.05, 0.95)))
        for face in range(6):
            for swap in (False, True):  # the edge in u, then in v
                p = _face_uv_to_xyz(face, v, u) if swap else _face_uv_to_xyz(face, u, v)
                scale = 6.37e6 / math.sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2])
                q = (p[0] * scale, p[1] * scale, p[2] * scale)
                for a in steps:
                    for b in steps:
                        for c in steps:
                            pts.append((_ulp_step(q[0], a), _ulp_step(q[1], b), _ulp_step(q[2], c)))
    p = np.array(pts)
    return np.ascontiguousarray(p[:, 0]), np.ascontiguousarray(p[:, 1]), np.ascontiguousarray(p[:, 2])


@functools.lru_cache(maxsize=None)
def uniform_cloud(n=20000):
    from point_cloud_viewer_amd import synthetic
    x, y, z, rgb, _, _ = synthetic.uniform_ecef(n)
    return x, y, z, rgb


POINT_SETS = {"uniform": uniform_cloud, "shell": shell_points, "ties": tie_points, "edges": edge_points}


@functools.lru_cache(maxsize=None)
def set_leaf_ids(name):
    """Leaf ids of one of POINT_SETS by this restatement, computed once per process; read-only."""
    ids = leaf_ids(*POINT_SETS[name]()[:3])
    ids.setflags(write=False)
    return ids


# ---- meta.pb of an S2 directory (tests/meta_proto.py drops the s2 attributes) --------------------------------------------
def _varint(buf, at):
    v = shift = 0
    while True:
        b = buf[at]
        at += 1
        v |= (b & 0x7F) << shift
        shift += 7
        if not b & 0x80:
            return v, at


def _fields(buf):
    at = 0
    while at < len(buf):
        key, at = _varint(buf, at)
        field, wire = key >> 3, key & 7
        if wire == 0:
            val, at = _varint(buf, at)
        elif wire == 1:
            val = struct.unpack_from("<d", buf, at)[0]
            at += 8
        elif wire == 2:
            ln, at = _varint(buf, at)
            val = bytes(buf[at:at + ln])
            at += ln
        else:
            raise ValueError(f"wire type {wire}")
        yield field, val


def _vec3(buf):
    v = [0.0, 0.0, 0.0]
    for field, val in _fields(buf):
        v[field - 1] = val
    return v


def parse_s2_meta(buf):
    """proto.proto Meta with the s2 arm: {version, bbox_min, bbox_max, cells: [(id, num_points)], attributes: [(name, type)]}"""
    out = {"version": 0, "bbox_min": None, "bbox_max": None, "cells": [], "attributes": [], "has_s2": False}
    for field, val in _fields(buf):
        if field == 1:
            out["version"] = val
        elif field == 4:
            for f2, v2 in _fields(val):
                out["bbox_min" if f2 == 3 else "bbox_max"] = _vec3(v2)
        elif field == 7:
            out["has_s2"] = True
            for f2, v2 in _fields(val):
                sub = dict(_fields(v2))
                if f2 == 1:
                    out["cells"].append((sub.get(1, 0), sub.get(2, 0)))
                elif f2 == 2:
                    out["attributes"].append((sub.get(1, b"").decode(), sub.get(2, 0)))
        else:
            raise ValueError(f"unexpected Meta field {field}")
    return out
