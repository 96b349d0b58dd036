"""get_visible_nodes' pop order without a GPU: std's BinaryHeap mechanics on cases that can be checked on paper, the plain
Python traversal of tests/visible_mirror.py against the C++ oracle on every view of tests/visible_cases.py, and what those
views reach: heaps past the kernel's 256 LDS slots, heaps that end at that boundary, runs of equal keys, panics in the
middle of a traversal. test_gpu_visible_fuzz.py submits the same views to the device; the conditions here keep it from
passing on views that never leave the easy path. No tolerance anywhere: every comparison is list equality."""
import numpy as np
import pytest

import oracle_lib as O
import visible_cases as VC
import visible_mirror as VM

HEAP_LDS_SLOTS = 256  # kHeapLds of visible_nodes_kernel


def test_equal_keys_pop_in_the_order_of_the_sift_mechanics():
    # Five equal keys, items 0..4. No push moves anything (sift_up stops at `element <= parent`): the heap is [0 1 2 3 4].
    # pop 1: the last, 4, is swapped with the top: 0 is returned, [4 1 2 3]. sift_down_to_bottom(0): children 1 and 2 are
    #        equal, `left <= right` takes the RIGHT one: 2 moves up, the hole is at slot 2, which has no child (5 > end - 2 and
    #        5 != end - 1 = 3): 4 lands there, [2 1 4 3]; sift_up: 4 <= 2's key, stays.
    # pop 2: last 3, top 2 is returned, [3 1 4]: the right child 4 moves up, 3 lands in slot 2: [4 1 3].
    # pop 3: last 3, top 4 is returned, [3 1]: no pair of children (1 > end - 2 = 0), but child == end - 1: the lone left
    #        child 1 moves up, 3 lands in slot 1, [1 3]; sift_up: 3 <= 1's key, stays.
    # pop 4: last 3, top 1 is returned, [3].  pop 5: 3.
    assert VM.pop_order([1.0] * 5) == [0, 2, 4, 1, 3]
    assert VM.pop_order([4.0] * 8) == [0, 2, 6, 5, 7, 4, 1, 3]
    assert VM.pop_order([2.0, 4.0, 4.0, 1.0, 4.0, 2.0]) == [1, 2, 4, 5, 0, 3]
    # a max-heap whatever the ties: the keys come out sorted, every item once
    rng = np.random.default_rng(3)
    keys = rng.integers(0, 6, 400).astype(np.float64).tolist()
    order = VM.pop_order(keys)
    assert sorted(order) == list(range(400)) and [keys[i] for i in order] == sorted(keys, reverse=True)


def test_child_cubes_are_the_get_child_recurrence():
    assert VM.child_cube((0.0, 8.0, 16.0, 64.0), 0) == (0.0, 8.0, 16.0, 32.0)
    assert VM.child_cube((0.0, 8.0, 16.0, 64.0), 4) == (32.0, 8.0, 16.0, 32.0)   # bit 4 is x
    assert VM.child_cube((0.0, 8.0, 16.0, 64.0), 2) == (0.0, 40.0, 16.0, 32.0)   # bit 2 is y
    assert VM.child_cube((0.0, 8.0, 16.0, 64.0), 1) == (0.0, 8.0, 48.0, 32.0)    # bit 1 is z
    # and equal NodeId::find_bounding_cube where the cube is a power of two
    cube = (0.0, 0.0, 0.0, 64.0)
    for d in "0172":
        cube = VM.child_cube(cube, int(d))
    hi, lo = O.node_id_from_str("r0172")
    mn, edge = O.find_bounding_cube(hi, lo, VC.BMIN, 64.0)
    assert cube == (mn[0], mn[1], mn[2], edge)


@pytest.fixture(scope="module", params=["A", "B"])
def exp(request):
    return request.param, VC.expected(request.param)


def test_mirror_equals_the_oracle_on_every_view(exp):
    key, e = exp
    assert len(e["cases"]) >= 200
    for (tag, _), want, got in zip(e["cases"], e["want"], e["mirror"]):
        assert got.names == want, (key, tag)  # None where the reference panics
        assert (got.status == 0) == (want is not None), (key, tag)
    assert sum(bool(w) for w in e["want"]) > 150


def test_the_views_reach_the_gaps():
    a, b = VC.expected("A")["mirror"], VC.expected("B")["mirror"]
    heaps = [r.max_heap_len for r in a + b]
    assert any(HEAP_LDS_SLOTS < h <= 512 for h in heaps) and any(512 < h <= 1024 for h in heaps) and any(h > 1024 for h in heaps)
    # sifts that straddle the boundary with a nearly empty global part, and the heap that just fits
    assert {r.max_heap_len for r in a[9:14]} == {252, 255, 256, 257, 259}
    assert sum(250 <= h <= 262 for h in heaps) >= 5
    assert max(r.tie_pops for r in a) > 1000 and max(r.tie_pops for r in b) > 1000
    panics = [r for r in a + b if r.status == 2]
    assert sum(r.panic_after >= 5 for r in panics) >= 2 and sum(r.panic_after == 1 for r in panics) >= 1
    assert sum(r.panic_after == 0 for r in panics) >= 1  # at the root's own push
    assert sum(r.status == 1 for r in a) >= 3 and all(r.names is None and r.panic_after == 0 for r in a if r.status == 1)
    # the figures the pull request states
    assert max(heaps) == 2459 and sum(r.tie_pops for r in a + b) == 78241 and len(panics) == 15


def test_reference_points():
    a, b = VC.expected("A"), VC.expected("B")
    by_tag = lambda e: {tag: r for (tag, _), r in zip(e["cases"], e["mirror"])}
    ra, rb = by_tag(a), by_tag(b)
    r = ra["ortho 0.9: every node In, every level one size"]
    assert (r.max_heap_len, r.tie_pops, r.panic_after) == (803, 2147, 2191)
    r = rb["ortho 0.9: every node In, every level one size"]
    assert (r.max_heap_len, r.tie_pops, r.panic_after) == (2051, 5719, 5766)
    assert ra["from above, z = 72"].max_heap_len == 664 and ra["heap at the LDS boundary, z = 40.0"].max_heap_len == 252
    r = ra["w == 0 on every child of the root"]
    assert r.names is None and r.status == 2 and r.panic_after == 1
    # the mid-traversal panics: the eyes are the top centres of nodes that exist, at level >= 3
    for name, eye in VC.PANIC_NODES.items():
        assert name in a["oracle"].nodes and len(name) - 1 >= 3
        cube = (0.0, 0.0, 0.0, 64.0)
        for d in name[1:]:
            cube = VM.child_cube(cube, int(d))
        assert eye == (cube[0] + cube[3] / 2, cube[1] + cube[3] / 2, cube[2] + cube[3])
        r = ra[f"w == 0 at the top of {name}"]
        assert r.status == 2 and r.panic_after >= 5, (name, r)


def empty_nodes(nodes):
    """Two inner nodes of the tree, one of them at level 1, to be declared empty (num_points = 0)."""
    inner = [n for n in nodes if any(n + str(d) in nodes for d in range(8)) and nodes[n]["num_points"] > 0]
    level1 = [n for n in inner if len(n) == 2]
    deeper = [n for n in inner if len(n) == 4 and not n.startswith(level1[0])]
    return level1[0], deeper[0]


def test_empty_nodes_are_expanded_but_not_listed():
    a = VC.expected("A")
    nodes = {k: dict(v) for k, v in a["oracle"].nodes.items()}
    holes = empty_nodes(nodes)
    for n in holes:
        nodes[n]["num_points"] = 0
    for tag, m in VC.fixed_cases("A"):
        got, want = VM.traverse(VC.BMIN, VC.BMAX, nodes, m), O.get_visible_nodes(VC.BMIN, VC.BMAX, nodes, m)
        assert got.names == want, tag
    full = VM.traverse(VC.BMIN, VC.BMAX, a["oracle"].nodes, VC.ortho())
    got = VM.traverse(VC.BMIN, VC.BMAX, nodes, VC.ortho())
    assert got.names == [n for n in full.names if n not in holes] and got.max_heap_len == full.max_heap_len
    assert all(any(n.startswith(h) and n != h for n in got.names) for h in holes)
