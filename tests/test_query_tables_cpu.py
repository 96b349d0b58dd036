"""The octree's query tables (point_cloud_viewer_amd/csrc/pcv_query_tables.h) on the CPU, through the test hook
pcv_query_tables_selftest: children and masks against (level, id) arithmetic in Python, the two cube tables against
oracle_lib.find_bounding_cube and the get_child recurrence as visible_mirror.child_cube states it, the host walk against
oracle_lib.nodes_in_location, and the layout of the device block."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle_lib as O
import point_cloud_viewer_amd as pcv
import visible_cases as VC
import visible_mirror as VM
from point_cloud_viewer_amd import _lib

BATCH_NODE = np.dtype([("xyz_off", "<u8"), ("point_off", "<u8"), ("cube_min", "<f8", 3), ("cube_edge", "<f8"), ("n", "<u4"),
                       ("enc", "<u4")])  # struct BatchNode
SECTIONS = ("cubes", "fb_cubes", "nodes", "first_child", "child_mask", "empty")
ALIGN = dict(cubes=32, fb_cubes=32, nodes=8, first_child=4, child_mask=1, empty=1)  # a cube is read as one double4
ENTRY = dict(cubes=32, fb_cubes=32, nodes=56, first_child=4, child_mask=1, empty=1)
INDEX_MASK = (1 << 120) - 1


def key_of(level, index):
    """(id_high, id_low) of NodeId { level, index } (node.rs:101-111): 8 bits of level over 120 bits of index."""
    v = (level << 120) | index
    return v >> 64, v & 0xFFFFFFFFFFFFFFFF


def node_table(ids, num_points, bmin, root_edge):
    """[(level, index)] in any order -> (pcv_node_info array in (level, index) order, that order's [(level, index)]): cubes from
    the oracle's find_bounding_cube, running offsets, an encoding that changes with the level."""
    order = sorted(range(len(ids)), key=lambda k: ids[k])
    infos = (_lib.NodeInfo * max(len(ids), 1))()
    xyz = pts = 0
    for at, k in enumerate(order):
        level, index = ids[k]
        hi, lo = key_of(level, index)
        mn, edge = O.find_bounding_cube(hi, lo, bmin, root_edge)
        nd = infos[at]
        nd.id_high, nd.id_low, nd.num_points, nd.level, nd.encoding = hi, lo, num_points[k], level, 1 + level % 4
        nd.cube_min[:] = list(mn)
        nd.cube_edge = edge
        nd.xyz_offset, nd.point_offset = xyz, pts
        xyz += (num_points[k] * 3 * (1 << (level % 4)) + 15) // 16 * 16
        pts += num_points[k]
    return infos, [ids[k] for k in order]


def run(infos, m, bmin, bmax, relation=None):
    f = pcv.load_library().pcv_query_tables_selftest
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_uint32] + [C.c_void_p] * 12
    lo, hi = np.ascontiguousarray(bmin, dtype=np.float64), np.ascontiguousarray(bmax, dtype=np.float64)
    out = dict(cubes=np.full((m, 4), np.nan), fb_cubes=np.full((m, 4), np.nan), first_child=np.full(m, 0xdead, dtype=np.uint32),
               child_mask=np.full(m, 0xee, dtype=np.uint8), empty=np.full(m, 0xee, dtype=np.uint8), nodes=np.zeros(m, dtype=BATCH_NODE))
    layout, walk, count = np.zeros(7, dtype=np.uint64), np.zeros(max(m, 1), dtype=np.uint32), C.c_uint32(0)
    rel = None if relation is None else np.ascontiguousarray(relation, dtype=np.uint8)
    rc = f(C.addressof(infos), m, lo.ctypes.data, hi.ctypes.data, out["cubes"].ctypes.data, out["fb_cubes"].ctypes.data,
           out["first_child"].ctypes.data, out["child_mask"].ctypes.data, out["empty"].ctypes.data, out["nodes"].ctypes.data,
           layout.ctypes.data, None if rel is None else rel.ctypes.data, walk.ctypes.data, C.addressof(count))
    assert rc == 0
    out["layout"] = dict(zip(SECTIONS + ("bytes",), (int(v) for v in layout)))
    out["walk"] = walk[:count.value].copy()
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def check_tables(got, infos, ids, bmin, bmax, orphans=()):
    """Children and masks from (level, index); fb_cubes = the oracle's find_bounding_cube; cubes = the get_child recurrence
    from Cube::bounding of the box — zeros, today's values, for the nodes of `orphans` (no parent in the table) and below."""
    m = len(ids)
    at = {key: i for i, key in enumerate(ids)}
    root_edge = max(float(bmax[a]) - float(bmin[a]) for a in range(3))
    cube = {(0, 0): (float(bmin[0]), float(bmin[1]), float(bmin[2]), root_edge)}
    for i, (level, index) in enumerate(ids):
        kids = [(d, at[(level + 1, index * 8 + d)]) for d in range(8) if (level + 1, index * 8 + d) in at]
        assert got["child_mask"][i] == sum(1 << d for d, _ in kids), (level, index)
        if kids:
            assert got["first_child"][i] == kids[0][1] and [c for _, c in kids] == list(range(kids[0][1], kids[0][1] + len(kids)))
        else:  # where the children would be inserted: after every node of the next level with a smaller index
            assert got["first_child"][i] == sum(1 for l, x in ids if l < level + 1 or (l == level + 1 and x < index * 8))
        nd = infos[i]
        mn, edge = O.find_bounding_cube(nd.id_high, nd.id_low, bmin, root_edge)
        assert np.array_equal(bits(got["fb_cubes"][i]), bits(list(mn) + [edge])), (level, index)
        assert got["empty"][i] == (nd.num_points == 0)
        row = got["nodes"][i]
        assert (row["xyz_off"], row["point_off"], row["n"], row["enc"]) == (nd.xyz_offset, nd.point_offset, nd.num_points, nd.encoding)
        assert np.array_equal(bits(row["cube_min"]), bits(nd.cube_min[:])) and bits(row["cube_edge"]) == bits(nd.cube_edge)
        if (level, index) in cube:
            for d, _ in kids:
                cube[(level + 1, index * 8 + d)] = VM.child_cube(cube[(level, index)], d)
        want = cube.get((level, index), (0.0, 0.0, 0.0, 0.0))
        assert np.array_equal(bits(got["cubes"][i]), bits(want)), (level, index)
    missing = {key for key in ids if key not in cube}
    assert missing == {key for key in ids if any(key[0] >= l and key[1] >> (3 * (key[0] - l)) == x for l, x in orphans)}
    return m


def ids_of(tree):
    ids, npts = [], []
    for nd in tree.nodes.values():
        hi, lo = nd["id"]
        ids.append((nd["level"], ((hi << 64) | lo) & INDEX_MASK))
        npts.append(nd["num_points"])
    return ids, npts


@functools.lru_cache(maxsize=None)
def clipped(key):
    """One of the clipped trees of visible_cases.py (empty inner nodes, missing octants) as a node table; computed once."""
    tree = VC.oracle_tree(key)
    ids, npts = ids_of(tree)
    infos, order = node_table(ids, npts, VC.BMIN, 64.0)
    return tree, infos, order


def test_empty_table():
    got = run((_lib.NodeInfo * 1)(), 0, VC.BMIN, VC.BMAX, relation=np.zeros(1, dtype=np.uint8))
    assert got["walk"].size == 0 and got["layout"]["bytes"] == 126


def test_lone_root():
    bmin, bmax = np.array([-3.0, 1.0, 2.0]), np.array([5.0, 4.0, 3.5])  # Cube::bounding: the longest side
    infos, ids = node_table([(0, 0)], [17], bmin, 8.0)
    got = run(infos, 1, bmin, bmax, relation=[1])
    check_tables(got, infos, ids, bmin, bmax)
    assert got["child_mask"][0] == 0 and got["first_child"][0] == 1 and list(got["cubes"][0]) == [-3.0, 1.0, 2.0, 8.0]
    assert list(got["walk"]) == [0]
    assert run(infos, 1, bmin, bmax, relation=[2])["walk"].size == 0


@pytest.mark.parametrize("key", ["A", "B"])
def test_clipped_trees(key):
    tree, infos, ids = clipped(key)
    m = len(ids)
    assert m == VC.NODES[key]
    got = run(infos, m, VC.BMIN, VC.BMAX)
    check_tables(got, infos, ids, VC.BMIN, VC.BMAX)
    inner = got["child_mask"] != 0
    assert got["empty"].sum() > 0  # nodes without points
    assert inner.sum() > 100 and (got["child_mask"][inner] != 0xff).sum() > 50  # missing octants


@pytest.mark.parametrize("key", ["A", "B"])
def test_walk_is_nodes_in_location(key):
    """The host walk over a relation row == the oracle's NodeIdsIterator, for boxes that prune, keep everything, keep nothing."""
    tree, infos, ids = clipped(key)
    m = len(ids)
    names = [O.node_id_str(infos[i].id_high, infos[i].id_low) for i in range(m)]
    fb = run(infos, m, VC.BMIN, VC.BMAX)["fb_cubes"]
    boxes = [[5.0, 5.0, 5.0, 30.0, 22.0, 41.0], [-1.0, -1.0, -1.0, 65.0, 65.0, 65.0], [70.0, 70.0, 70.0, 80.0, 80.0, 80.0],
             [31.5, 0.0, 0.0, 32.5, 64.0, 64.0], [16.0, 16.0, 16.0, 32.0, 32.0, 32.0]]
    sizes = []
    for box in boxes:
        rel = O.cull_cubes(O.SHAPE_AABB, box, fb)
        walk = run(infos, m, VC.BMIN, VC.BMAX, relation=rel)["walk"]
        assert [names[i] for i in walk] == O.nodes_in_location(VC.BMIN, VC.BMAX, tree.nodes, O.SHAPE_AABB, box), box
        sizes.append(walk.size)
    assert sizes[1] == m and sizes[2] == 0 and 0 < sizes[0] < m


def test_level_gap_pins_todays_values():
    """A table whose largest level-1 node was removed: its children keep their rows, their masks and their find_bounding_cube cubes, and
    what the get_child table holds for them and everything below them is what it holds today — zeros. The walk never reaches
    them: the root's mask has no bit for it."""
    tree, _, _ = clipped("A")
    ids, npts = ids_of(tree)
    under = lambda d: [k for k in ids if k[0] > 1 and k[1] >> (3 * (k[0] - 1)) == d]
    octant = max(range(8), key=lambda d: len(under(d)))
    gone, below = (1, octant), under(octant)
    assert gone in ids and len(below) > 50
    keep = [k for k in range(len(ids)) if ids[k] != gone]
    infos, order = node_table([ids[k] for k in keep], [npts[k] for k in keep], VC.BMIN, 64.0)
    m = len(order)
    rel = np.ones(m, dtype=np.uint8)
    got = run(infos, m, VC.BMIN, VC.BMAX, relation=rel)
    orphans = [k for k in order if k[0] == 2 and k[1] >> 3 == octant]
    check_tables(got, infos, order, VC.BMIN, VC.BMAX, orphans=orphans)
    assert not (got["child_mask"][0] >> octant) & 1
    zero = [i for i, k in enumerate(order) if k in set(below)]
    assert len(zero) == len(below) and not got["cubes"][zero].any() and got["fb_cubes"][zero][:, 3].all()
    assert any(got["child_mask"][i] for i in zero)  # an orphan still finds its own children
    assert set(got["walk"]) == set(range(m)) - set(zero) and list(got["walk"]) == sorted(got["walk"])


def test_deep_path_searches_128_bit_indices():
    """One path from the root to level 24 with two leaves: from level 22 on the index needs more than 64 bits."""
    bmin, bmax = np.zeros(3), np.full(3, 1.0e4)
    digits = [(5 * l + 1) % 8 for l in range(1, 24)]
    ids, index = [(0, 0)], 0
    for l, d in enumerate(digits, 1):
        index = index * 8 + d
        ids.append((l, index))
    ids += [(24, index * 8 + 1), (24, index * 8 + 6)]
    assert ids[22][1] >= 1 << 64
    infos, order = node_table(ids, [0] * 24 + [3, 4], bmin, 1.0e4)
    got = run(infos, len(order), bmin, bmax, relation=np.ones(len(order), dtype=np.uint8))
    check_tables(got, infos, order, bmin, bmax)
    assert list(got["child_mask"][:23]) == [1 << d for d in digits] and got["child_mask"][23] == 0b1000010
    assert list(got["first_child"][:24]) == list(range(1, 25)) and list(got["walk"]) == list(range(26))


def layout_only(m):
    """The layout of a table of m nodes: m copies of an empty root give the arithmetic its m without a tree."""
    infos = (_lib.NodeInfo * max(m, 1))()
    return run(infos, m, np.zeros(3), np.zeros(3))["layout"]


@pytest.mark.parametrize("m", [0, 1, 7, 2191, 5766, 100_003])
def test_layout_of_the_device_block(m):
    """Sections in today's order, each of m + 1 entries, disjoint, aligned for what reads them, and summing to today's byte
    count, (m + 1) * (64 + sizeof(BatchNode) + 4 + 2)."""
    lay = layout_only(m)
    at = 0
    for name in SECTIONS:
        assert lay[name] == at and lay[name] % ALIGN[name] == 0, name
        at += ENTRY[name] * (m + 1)
    assert lay["bytes"] == at == (m + 1) * (64 + BATCH_NODE.itemsize + 4 + 2)
