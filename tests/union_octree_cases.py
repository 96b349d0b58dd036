"""Inputs shared by the cell-union-over-the-octree tests (test_union_octree_cpu.py, test_gpu_union_query.py): the cubes of
NodeId::find_bounding_cube, the scene's unions, the independent truth of cells_intersecting_polyhedron
(s2_region_truth.py) and the breadth-first walk a node list has to equal."""
import functools

import numpy as np

import s2_region_truth as R
import s2_truth as T


def cubes_to_depth(bmin, bmax, depth):
    """(n, 4) cubes (min xyz, edge) of every node id down to `depth`, level by level: Cube::bounding of the box (aabb.rs:149-157:
    the longest side), then NodeId::find_bounding_cube's recurrence (node.rs:160-170: edge /= 2; min += bit * edge)."""
    level = np.array([[float(bmin[0]), float(bmin[1]), float(bmin[2]), float(np.max(np.asarray(bmax) - np.asarray(bmin)))]])
    out = [level]
    for _ in range(depth):
        half = level[:, 3] / 2.0
        kids = []
        for digit in range(8):
            k = level.copy()
            k[:, 3] = half
            for axis, bit in ((0, 4), (1, 2), (2, 1)):
                if digit & bit:
                    k[:, axis] = level[:, axis] + half
            kids.append(k)
        level = np.stack(kids, axis=1).reshape(-1, 4)
        out.append(level)
    return np.concatenate(out)


@functools.lru_cache(maxsize=None)
def scene_cubes():
    """The 4 681 cubes to depth 4 over the bounding cube of the scene's cloud."""
    from point_cloud_viewer_amd import synthetic
    _, _, _, _, bmin, bmax = synthetic.uniform_ecef(20000)
    return cubes_to_depth(bmin, bmax, 4)


def centre_leaf():
    from point_cloud_viewer_amd import synthetic
    _, centre = synthetic.ecef_from_local(37.407204, -122.147604)
    return T.leaf_id(*[float(v) for v in centre])


@functools.lru_cache(maxsize=None)
def unions():
    """R.scene_unions(20) and one level-8 cell over the whole cloud; each ascending."""
    return [list(u) for u in R.scene_unions(20)] + [[T.parent(centre_leaf(), 8)]]


def truth_of_cube(union, cube, bounds=None):
    """1 / 0 / None (undecided) for cells_intersecting_polyhedron(union, cube), by the independent truth."""
    lo = np.asarray(cube[:3], dtype=np.float64)
    rect = R.corners_rect(R.aabb_corners(lo, lo + cube[3]))
    yes, undecided, _ = R.decided_lists(union, rect, bounds=bounds)
    if yes:
        return 1
    return None if undecided else 0


def bfs(intersects, first_child, child_mask):
    """NodeIdsIterator over flags per node: a node is listed and descended into iff it intersects."""
    out, queue = [], [0] if len(intersects) else []
    at = 0
    while at < len(queue):
        n = queue[at]
        at += 1
        if not intersects[n]:
            continue
        out.append(n)
        c = int(first_child[n])
        for digit in range(8):
            if (int(child_mask[n]) >> digit) & 1:
                queue.append(c)
                c += 1
    return np.array(out, dtype=np.uint32)


def tree_tables(tree):
    """(cubes (m, 4) by find_bounding_cube, first_child, child_mask) of an OctreeResult from its node ids: nodes are stored in
    (level, index) order, a node's children are consecutive, in digit order."""
    m = tree.num_nodes
    infos = [tree.node(i) for i in range(m)]
    meta = tree.meta()
    root = np.array([*meta["bbox_min"], float(np.max(meta["bbox_max"] - meta["bbox_min"]))])
    key = {(int(nd.level), int(nd.id_low)): i for i, nd in enumerate(infos)}
    assert all(int(nd.id_high) & ((1 << 56) - 1) == 0 for nd in infos), "node ids deeper than 21 levels"
    cubes = np.zeros((m, 4))
    first_child, child_mask = np.zeros(m, dtype=np.uint32), np.zeros(m, dtype=np.uint8)
    for i, nd in enumerate(infos):
        level, index = int(nd.level), int(nd.id_low)
        c = root.copy()
        for k in range(level - 1, -1, -1):
            digit = (index >> (3 * k)) & 7
            c[3] = c[3] / 2.0
            for axis, bit in ((0, 4), (1, 2), (2, 1)):
                if digit & bit:
                    c[axis] = c[axis] + c[3]
        cubes[i] = c
        kids = [key.get((level + 1, index * 8 + d)) for d in range(8)]
        present = [k for k in kids if k is not None]
        if present:
            first_child[i] = present[0]
            assert present == list(range(present[0], present[0] + len(present)))
        child_mask[i] = sum(1 << d for d in range(8) if kids[d] is not None)
    return cubes, first_child, child_mask
