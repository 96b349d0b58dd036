"""S2 cell ids on the host: the library's host twin (pcv_s2_cell_ids_host, pcv_s2_cell_token, pcv_s2_union_contains_host)
against s2_truth.py, the independent restatement of DESIGN §9c, and against the known answers of the S2 test suites. No GPU."""
import numpy as np
import pytest

import point_cloud_viewer_amd as pcv

import s2_truth as T

# the S2 test suites' own leaf ids for lat / lng in degrees
KNOWN = [((49.703498679, 11.770681595), 0x47a1cbd595522b39),
         ((55.685376759, 12.588490937), 0x46525318b63be0f9),
         ((45.486546517, -93.449700022), 0x52b30b71698e729d)]
AXES = [((1.0, 0.0, 0.0), 0x1), ((0.0, 1.0, 0.0), 0x3), ((0.0, 0.0, 1.0), 0x5),
        ((-1.0, 0.0, 0.0), 0x7), ((0.0, -1.0, 0.0), 0x9), ((0.0, 0.0, -1.0), 0xb)]


def ids_of(points, level=30):
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    return pcv.s2_cell_ids(p[:, 0], p[:, 1], p[:, 2], level)


def test_known_answers():
    for (lat, lng), want in KNOWN:
        p = T.from_lat_lng_deg(lat, lng)
        assert T.leaf_id(*p) == want, (lat, lng)
        assert int(ids_of([p])[0]) == want, (lat, lng)
        # any radius: the chain normalises first
        assert int(ids_of([[c * 6371000.0 for c in p]])[0]) == want, (lat, lng)


def test_axis_points():
    for p, nibble in AXES:
        leaf = (nibble << 60) | 1
        assert T.leaf_id(*p) == leaf and int(ids_of([p])[0]) == leaf, p
        assert pcv.s2_cell_token(int(ids_of([p], 0)[0])) == f"{nibble:x}" == T.token(T.parent(leaf, 0))
        assert pcv.s2_cell_token(int(ids_of([p], 20)[0])) == f"{nibble:x}0000000001" == T.token(T.parent(leaf, 20))


@pytest.mark.parametrize("name", sorted(T.POINT_SETS))
def test_host_twin_equals_the_truth(name):
    x, y, z = T.POINT_SETS[name]()[:3]
    want = T.set_leaf_ids(name)
    got = pcv.s2_cell_ids(x, y, z)
    assert got.dtype == np.uint64 and np.array_equal(got, want), f"{int((got != want).sum())} of {want.size} leaf ids differ"
    for level in (0, 13, 20, 29):
        assert np.array_equal(pcv.s2_cell_ids(x, y, z, level), T.parents(want, level)), level


def test_uniform_cloud_cells():
    """The config-1 cloud: 675 level-20 cells around the generator's default location, 1 to 49 points each."""
    cells, counts = np.unique(T.parents(T.set_leaf_ids("uniform"), 20), return_counts=True)
    assert (cells.size, int(counts.max()), int(counts.min())) == (675, 49, 1)
    assert T.token(int(cells[0])).startswith("808e4d142b") and len(T.token(int(cells[0]))) == 11


def test_point_sets_cover_what_they_claim():
    faces = np.bincount((T.set_leaf_ids("shell") >> np.uint64(61)).astype(np.int64), minlength=6)
    assert faces.min() > 300, faces
    x, y, z = T.tie_points()
    assert ((np.abs(x) == np.abs(y)) & (np.abs(y) == np.abs(z))).sum() >= 8 and (np.abs(x) == np.abs(y)).sum() > 40
    # the edge set straddles its edges: more cells than (k, face, direction) groups
    edges20 = np.unique(T.parents(T.set_leaf_ids("edges"), 20)).size
    assert edges20 > T.edge_points()[0].size // 125, edges20


def test_parent_contains_the_leaf():
    leaves = np.concatenate([T.set_leaf_ids("shell"), T.set_leaf_ids("edges")[::7]])
    x, y, z = (np.concatenate([a, b[::7]]) for a, b in zip(T.shell_points(), T.edge_points()))
    for level in range(0, 31, 3):
        got = pcv.s2_cell_ids(x, y, z, level)
        lsb = got & (~got + np.uint64(1))
        assert np.all(lsb == np.uint64(T.lsb_for_level(level)))
        lo, hi = got - (lsb - np.uint64(1)), got + (lsb - np.uint64(1))
        assert np.all((lo <= leaves) & (leaves <= hi)), level
    for leaf in leaves[:50].tolist():
        for level in (0, 1, 17, 30):
            c = T.parent(leaf, level)
            assert T.range_min(c) <= leaf <= T.range_max(c)


def test_hilbert_continuity():
    """Consecutive leaf positions on a face are 4-neighbours in (i, j), and the curve decodes back to what encoded it."""
    rng = np.random.Generator(np.random.PCG64(2))
    for face in range(6):
        for start in [0, (1 << 60) - 300] + [int(s) for s in rng.integers(0, (1 << 60) - 300, 4)]:
            prev = None
            for pos in range(start, start + 300):
                f, i, j = T.face_ij((((face << 60) | pos) << 1) | 1)
                assert f == face and T.leaf_from_face_ij(f, i, j) == (((face << 60) | pos) << 1) | 1
                if prev is not None:
                    assert abs(i - prev[0]) + abs(j - prev[1]) == 1, (face, pos)
                prev = (i, j)


def mixed_union(leaves, rng):
    """Cells of mixed levels around some of the leaves, disjoint and ascending."""
    picked = []
    for leaf in rng.choice(leaves, 40, replace=False).tolist():
        picked.append(T.parent(int(leaf), int(rng.integers(17, 31))))
    picked.sort()
    cells = []
    for c in picked:  # drop what overlaps its predecessor: a normalised union is disjoint
        if not cells or T.range_min(c) > T.range_max(cells[-1]):
            cells.append(c)
    return cells


def test_union_contains_equals_the_truth():
    rng = np.random.Generator(np.random.PCG64(4))
    for name in ("uniform", "edges"):
        step = 3 if name == "edges" else 1
        x, y, z = (a[::step] for a in T.POINT_SETS[name]()[:3])
        leaves = T.set_leaf_ids(name)[::step]
        for cells in (mixed_union(leaves, rng), [T.parent(int(leaves[0]), 20)], [int(leaves[5])], []):
            got = pcv.s2_union_contains(cells, x, y, z)
            want = np.array([T.union_contains(cells, leaf) for leaf in leaves.tolist()], dtype=np.uint8)
            assert np.array_equal(got, want), (name, len(cells))
            if cells:
                assert got.any() and not got.all()


def test_union_range_ends():
    """Leaves exactly at range_min and range_max of a cell are inside, their outer neighbours are not. The points are found by
    inverting the chain: the centre of the leaf in (s, t), through the truth's own uv and face maps."""
    rng = np.random.Generator(np.random.PCG64(8))
    leaves = T.set_leaf_ids("shell")
    pts, want, cells = [], [], set()
    for leaf in rng.choice(leaves, 12, replace=False).tolist():
        cell = T.parent(int(leaf), int(rng.integers(3, 25)))
        cells.add(cell)
    cells = sorted(cells)
    kept = [c for k, c in enumerate(cells) if k == 0 or T.range_min(c) > T.range_max(cells[k - 1]) + 2]
    for cell in kept:
        for leaf, inside in ((T.range_min(cell), True), (T.range_max(cell), True), (T.range_min(cell) - 2, False),
                             (T.range_max(cell) + 2, False)):
            if leaf < 1 or (leaf >> 61) > 5 or any(T.range_min(c) <= leaf <= T.range_max(c) for c in kept) != inside:
                continue
            face, i, j = T.face_ij(leaf)
            p = T._face_uv_to_xyz(face, T._st_to_uv((i + 0.5) / T.MAX_SIZE), T._st_to_uv((j + 0.5) / T.MAX_SIZE))
            if T.leaf_id(*p) != leaf:  # (never seen: the centre of a leaf is 2^-31 away from its edges)
                continue
            pts.append(p)
            want.append(inside)
    assert len(pts) >= 3 * len(kept) and any(want) and not all(want)
    p = np.array(pts)
    got = pcv.s2_union_contains(kept, p[:, 0], p[:, 1], p[:, 2])
    assert np.array_equal(got.astype(bool), np.array(want))
    assert [T.union_contains(kept, T.leaf_id(*q)) for q in pts] == want


def test_errors():
    one = ([6.371e6], [0.0], [0.0])
    with pytest.raises(pcv.PcvError) as e:
        pcv.s2_cell_ids(*one, level=31)
    assert e.value.code == pcv.PCV_E_INVALID and "30" in str(e.value)
    leaf = int(pcv.s2_cell_ids(*one)[0])
    with pytest.raises(pcv.PcvError) as e:
        pcv.s2_union_contains([T.parent(leaf, 10) + (1 << 45), T.parent(leaf, 10)], *one)
    assert e.value.code == pcv.PCV_E_INVALID and "ascend" in str(e.value)
    with pytest.raises(pcv.PcvError):
        pcv.s2_union_contains([0], *one)
    assert pcv.s2_cell_ids([], [], []).size == 0


def test_tokens():
    assert pcv.s2_cell_token(0) == "X" == T.token(0)
    ids = np.concatenate([T.set_leaf_ids("shell")[:200], T.parents(T.set_leaf_ids("shell")[:200], 20),
                          T.parents(T.set_leaf_ids("shell")[:200], 0)])
    for cell in ids.tolist():
        tok = pcv.s2_cell_token(cell)
        assert tok == T.token(cell) and tok == tok.lower() and not tok.endswith("0") and 1 <= len(tok) <= 16
        assert int(tok.ljust(16, "0"), 16) == cell  # CellID::from_token


def test_meta_parser_round_trip():
    """The small parser the GPU test reads meta.pb with, against bytes built here field by field."""
    def varint(v):
        out = bytearray()
        while v >= 0x80:
            out.append((v & 0x7F) | 0x80)
            v >>= 7
        out.append(v)
        return bytes(out)

    def field(number, wire, payload):
        return varint((number << 3) | wire) + (varint(len(payload)) + payload if wire == 2 else payload)

    import struct
    vec = lambda v: b"".join(field(k + 1, 1, struct.pack("<d", c)) for k, c in enumerate(v) if c != 0.0)  # noqa: E731
    cells = [(0x808e4d142b100000, 49), (0x808e4d142b300000, 1)]
    s2 = b"".join(field(1, 2, field(1, 0, varint(i)) + field(2, 0, varint(c))) for i, c in cells)
    s2 += field(2, 2, field(1, 2, b"color") + field(2, 0, varint(27))) + field(2, 2, field(1, 2, b"intensity") + field(2, 0, varint(11)))
    box = field(3, 2, vec((-2.5, 0.0, 3.0))) + field(4, 2, vec((1.0, 2.0, 4.5)))
    meta = T.parse_s2_meta(field(1, 0, varint(13)) + field(4, 2, box) + field(7, 2, s2))
    assert meta == {"version": 13, "bbox_min": [-2.5, 0.0, 3.0], "bbox_max": [1.0, 2.0, 4.5], "cells": cells,
                    "attributes": [("color", T.U8VEC3), ("intensity", T.F32)], "has_s2": True}
