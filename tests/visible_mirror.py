"""Octree::get_visible_nodes (octree/mod.rs:228-283, 360-404) in plain Python: a third statement of the traversal, beside
the kernel's and the C++ oracle's, written from the reference's lines and from the algorithm of std's BinaryHeap alone.

The heap is a Python list of (size, name, relation). `heap_push` / `heap_pop` are std's BinaryHeap::push / pop:
  push: append, sift_up(0, old_len);
  sift_up(start, pos): the element at pos climbs while it is strictly GREATER than its parent (`hole.element() <= parent`
      breaks), so an equal key stays below;
  pop: take the last element off; if the heap is not empty, swap it with the top and sift_down_to_bottom(0);
  sift_down_to_bottom(pos): the hole goes all the way to a leaf, always to the GREATER child and to the RIGHT one on a tie
      (`child += (left <= right) as usize`), a lone left child at the end is taken too; then sift_up(start, pos).
Only the Relation and relative_size_on_screen of a cube come from elsewhere: oracle_lib.cull_cubes, which the Relation
tests pin on its own."""
from collections import namedtuple

import numpy as np

import oracle_lib as O

Result = namedtuple("Result", "names max_heap_len tie_pops panic_after status listed")


def _sift_up(h, start, pos):
    elt = h[pos]
    while pos > start:
        parent = (pos - 1) // 2
        if elt[0] <= h[parent][0]:
            break
        h[pos] = h[parent]
        pos = parent
    h[pos] = elt


def heap_push(h, item):
    h.append(item)
    _sift_up(h, 0, len(h) - 1)


def heap_pop(h):
    item = h.pop()
    if h:
        item, h[0] = h[0], item
        end, pos = len(h), 0
        elt = h[0]
        child = 1
        while child <= max(end, 2) - 2:
            child += h[child][0] <= h[child + 1][0]
            h[pos] = h[child]
            pos = child
            child = 2 * pos + 1
        if child == end - 1:
            h[pos] = h[child]
            pos = child
        h[pos] = elt
        _sift_up(h, 0, pos)
    return item


def pop_order(keys):
    """The item numbers 0 .. len(keys) - 1, pushed in that order with these keys, in the order they pop."""
    h = []
    for i, k in enumerate(keys):
        heap_push(h, (k, i, None))
    return [heap_pop(h)[1] for _ in range(len(keys))]


def child_cube(cube, digit):
    """Node::get_child (node.rs:190-211): half = edge / 2; min += half where the digit's bit is set (4: x, 2: y, 1: z)."""
    half = cube[3] / 2.0
    return (cube[0] + half if digit & 4 else cube[0], cube[1] + half if digit & 2 else cube[1],
            cube[2] + half if digit & 1 else cube[2], half)


def traverse(bmin, bmax, nodes, matrix):
    """nodes: {name: {"num_points": ..}} ('r', 'r3', 'r35' ..). Returns Result(names in pop order or None where the reference
    panics, the longest heap, the pops whose key equals the key of the top they leave behind, the pops before the panic,
    the status the library documents: 0, 1 (Frustum::from_matrix4 fails: mod.rs:229-230), 2 (a projection with w == 0:
    project()'s unwrap, mod.rs:103-106, reported by the oracle as a NaN size), and the number of nodes that hold points among
    the popped ones — the length of the list, or of what the library leaves behind where it reports status 2)."""
    matrix = np.asarray(matrix, dtype=np.float64).ravel()
    if O.cached_axes(O.SHAPE_FRUSTUM, matrix) is None:
        return Result(None, 0, 0, 0, 1, 0)
    bmin, bmax = np.asarray(bmin, np.float64), np.asarray(bmax, np.float64)
    heap, cubes = [], {}
    stats = dict(longest=0)

    def maybe_push(children, relations_known):
        """maybe_push_node over (name, cube) in child order; False where the reference panics."""
        children = [(n, c) for n, c in children if n in nodes]
        if not children:
            return True
        rel, size = O.cull_cubes(O.SHAPE_FRUSTUM, matrix, np.array([c for _, c in children]), with_sizes=True)
        for k, (name, cube) in enumerate(children):
            relation = relations_known if relations_known is not None else int(rel[k])
            if relation == O.REL_OUT:
                continue
            if size[k] != size[k]:
                return False
            cubes[name] = cube
            heap_push(heap, (float(size[k]), name, relation))
            stats["longest"] = max(stats["longest"], len(heap))
        return True

    root = (float(bmin[0]), float(bmin[1]), float(bmin[2]), float(np.max(bmax - bmin)))  # Cube::bounding, aabb.rs:149-157
    visible, ties, pops = [], 0, 0
    # the root is pushed as Cross without a test (mod.rs:233-239)
    if "r" in nodes:
        size = O.cull_cubes(O.SHAPE_FRUSTUM, matrix, np.array([root]), with_sizes=True)[1][0]
        if size != size:
            return Result(None, 0, 0, 0, 2, 0)
        cubes["r"] = root
        heap_push(heap, (float(size), "r", O.REL_CROSS))
        stats["longest"] = 1
    while heap:
        size, name, relation = heap_pop(heap)
        pops += 1
        ties += bool(heap) and heap[0][0] == size
        cube = cubes.pop(name)
        children = [(name + str(d), child_cube(cube, d)) for d in range(8)]
        good = maybe_push(children, None if relation == O.REL_CROSS else O.REL_IN)
        if nodes[name]["num_points"] != 0:
            visible.append(name)
        if not good:
            return Result(None, stats["longest"], ties, pops, 2, len(visible))
    return Result(visible, stats["longest"], ties, pops, 0, len(visible))
