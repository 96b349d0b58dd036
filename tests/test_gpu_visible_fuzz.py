"""pcv_visible_nodes (K7b, visible_nodes_kernel) against Octree::get_visible_nodes' pop order where the kernel's heap leaves
LDS, where keys tie, where the reference panics in the middle of a traversal, across traverse()'s batches, under a
truncating capacity and with empty nodes. The views are those of tests/visible_cases.py; test_visible_cpu.py asserts on the CPU
that they reach those paths. Lists are compared with the C++ oracle's name for name, statuses with the plain Python mirror's
(tests/visible_mirror.py). No tolerance anywhere."""
import glob
import os

import numpy as np
import pytest

import meta_proto
import oracle_lib as O
import point_cloud_viewer_amd as pcv
import render_oracle as R
import visible_cases as VC
import visible_mirror as VM
from test_gpu_render import check_views
from test_visible_cpu import empty_nodes

pytestmark = pytest.mark.gpu
HEAP_ENTRY_BYTES = 24  # sizeof(HeapEntry): f64 size, u32 node, first child, bits, pad


@pytest.fixture(scope="module")
def ctx():
    c = pcv.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def scenes(ctx):
    out = {}
    for key in "AB":
        x, y, z, rgb = VC.cloud(key)
        tree = ctx.build(VC.RESOLUTION, pcv.Aabb(VC.BMIN, VC.BMAX), x, y, z, rgb, max_points_per_node=VC.MAX_POINTS_PER_NODE)
        e = VC.expected(key)
        names = tree.node_names()
        assert sorted(names) == sorted(e["oracle"].nodes)
        out[key] = dict(e, tree=tree, names=names, mats=[m for _, m in e["cases"]], bmin=VC.BMIN, bmax=VC.BMAX)
    return out


def frusta(ctx, mats):
    return ctx.shapes([("frustum", m) for m in mats])


@pytest.mark.parametrize("key", ["A", "B"])
def test_pop_order_and_status_equal_the_reference(ctx, scenes, key):
    s = scenes[key]
    vis, status = s["tree"].visible_nodes(frusta(ctx, s["mats"]))
    for f, ((tag, _), want, mirror) in enumerate(zip(s["cases"], s["want"], s["mirror"])):
        assert status[f] == mirror.status, (tag, status[f], mirror)  # 0 ok, 1 no frustum, 2 a push with w == 0
        if want is not None:
            assert [s["names"][i] for i in vis[f]] == want, tag  # the same nodes in the same BinaryHeap pop order
        elif mirror.status == 1:
            assert len(vis[f]) == 0, tag
        else:  # what include/pcv_hip.h says of status 2: the nodes with points popped until the push that panics
            assert len(vis[f]) == mirror.listed <= mirror.panic_after, (tag, len(vis[f]), mirror)
    assert (status == 0).sum() > 150 and (status == 1).sum() >= 3 and (status == 2).sum() >= 7


def test_lists_do_not_depend_on_neighbours_or_runs(ctx, scenes):
    """Four waves share a workgroup's LDS heap array, every wave has its own global part: a frustum's list is the same alone,
    inside the batch, with the batch reversed, and in every repetition."""
    s = scenes["A"]
    tree, mats, n = s["tree"], s["mats"], len(s["mats"])
    heavy = sorted(range(n), key=lambda f: -s["mirror"][f].max_heap_len)[:16]
    assert all(s["mirror"][f].max_heap_len > 256 and s["want"][f] is not None for f in heavy)
    batch, batch_status = tree.visible_nodes(frusta(ctx, mats))
    for f in heavy:
        assert [s["names"][i] for i in batch[f]] == s["want"][f]
        alone, st = tree.visible_nodes(frusta(ctx, [mats[f]]))
        assert st[0] == 0 and np.array_equal(alone[0], batch[f]), s["cases"][f][0]
    rev, rev_status = tree.visible_nodes(frusta(ctx, mats[::-1]))
    assert np.array_equal(rev_status[::-1], batch_status)
    assert all(np.array_equal(rev[n - 1 - f], batch[f]) for f in range(n))
    shapes = frusta(ctx, mats)
    for k in range(5):
        again, st = tree.visible_nodes(shapes)
        assert np.array_equal(st, batch_status), k
        assert all(a.tobytes() == b.tobytes() for a, b in zip(again, batch)), k


def test_second_batch_of_traverse(ctx, scenes):
    """traverse() bounds its heap scratch to 256 MiB: past `batch` frusta it launches again, with the heaps indexed by the
    index inside the batch and the outputs by the global one. The spilling all-In view sits on both sides of the seam."""
    s = scenes["B"]
    tree, m = s["tree"], s["tree"].num_nodes
    batch = max(64, (256 << 20) // (HEAP_ENTRY_BYTES * m))
    n = batch + 70
    fill = [mat for _, mat in VC.random_cases(731, 70)]
    spill = VC.ortho()
    mats = fill + [spill]
    pick = np.arange(n) % 70
    pick[[batch - 1, batch, batch + 1, n - 1]] = 70
    want = VC.oracle_lists(s["oracle"].nodes, mats)
    assert len(want[70]) > 5000 and sum(bool(w) for w in want[:70]) > 40
    shapes = frusta(ctx, [mats[k] for k in pick])
    ctx.set_profiling(True)
    try:
        ctx.reset_kernel_stats()
        vis, status = tree.visible_nodes(shapes)
        launches = ctx.kernel_stats()["visible_nodes_kernel"][0]
    finally:
        ctx.set_profiling(False)
    assert launches >= 2
    index_of = {name: i for i, name in enumerate(s["names"])}
    want_idx = [None if w is None else np.array([index_of[name] for name in w], dtype=np.uint32) for w in want]
    for f in range(n):
        w = want_idx[pick[f]]
        assert (status[f] == 0) == (w is not None), f
        if w is not None:
            assert np.array_equal(vis[f], w), (f, pick[f])


def test_capacity_truncates_the_lists_and_keeps_the_counts(ctx, scenes):
    s = scenes["A"]
    tree, lib = s["tree"], s["tree"].lib
    mats = [m for _, m in VC.fixed_cases("A")]
    shapes = frusta(ctx, mats)
    f = len(mats)
    full, full_status = tree.visible_nodes(shapes)
    want_counts = np.array([len(v) for v in full], dtype=np.uint32)
    assert want_counts.max() > 2000
    guard, sentinel = 4096, 0xDEADBEEF
    for cap in (0, 1, int(want_counts.max()) // 2):
        counts = np.full(f, sentinel, dtype=np.uint32)
        status = np.full(f, -7, dtype=np.int32)
        idx = np.full(f * cap + guard, sentinel, dtype=np.uint32)
        ctx._check(lib.pcv_visible_nodes(ctx.handle, shapes.handle, tree.handle, cap, counts.ctypes.data,
                                         idx.ctypes.data if cap else None, status.ctypes.data))
        assert np.array_equal(counts, want_counts) and np.array_equal(status, full_status), cap
        assert (idx[f * cap:] == sentinel).all(), cap  # nothing past f * capacity
        for k in range(f):
            keep = min(cap, int(want_counts[k]))
            assert np.array_equal(idx[k * cap:k * cap + keep], full[k][:keep]), (cap, k)


def write_opened(ctx, tree, directory):
    tree.write_dir(directory)
    return ctx.open_dir(directory)


def test_empty_nodes_are_expanded_but_not_listed(ctx, scenes, tmp_path):
    s = scenes["A"]
    s["tree"].write_dir(tmp_path / "oct")
    nodes = {k: dict(v) for k, v in s["oracle"].nodes.items()}
    holes = empty_nodes(nodes)
    assert len(holes[0]) == 2 and len(holes[1]) > 2
    ids = {nodes[h]["id"] for h in holes}
    meta = meta_proto.classes()["Meta"]()
    meta.ParseFromString((tmp_path / "oct" / "meta.pb").read_bytes())
    changed = 0
    for nd in meta.octree.nodes:
        if (nd.id.high, nd.id.low) in ids:
            assert nd.num_points > 0
            nd.num_points = 0
            changed += 1
    assert changed == 2
    (tmp_path / "oct" / "meta.pb").write_bytes(meta.SerializeToString())
    for h in holes:
        files = glob.glob(str(tmp_path / "oct" / (h + ".*")))
        assert files
        for path in files:
            os.remove(path)
        nodes[h]["num_points"] = 0
    opened = ctx.open_dir(tmp_path / "oct")
    names = opened.node_names()
    assert sorted(names) == sorted(nodes)
    mats = [m for _, m in VC.fixed_cases("A")]
    vis, status = opened.visible_nodes(frusta(ctx, mats))
    for f, (tag, m) in enumerate(VC.fixed_cases("A")):
        want = O.get_visible_nodes(VC.BMIN, VC.BMAX, nodes, m)
        assert status[f] == VM.traverse(VC.BMIN, VC.BMAX, nodes, m).status, tag
        if want is not None:
            assert [names[i] for i in vis[f]] == want, tag
    everything = [names[i] for i in vis[0]]  # the all-In orthographic view
    assert not set(holes) & set(everything)
    assert all(any(n.startswith(h) and n != h for n in everything) for h in holes)
    opened.free()


def test_opened_directory_gives_the_built_tree_s_lists(ctx, scenes, tmp_path):
    s = scenes["B"]
    opened = write_opened(ctx, s["tree"], tmp_path / "oct")
    assert opened.node_names() == s["names"]
    shapes = frusta(ctx, [m for _, m in VC.fixed_cases("B")])
    built, built_status = s["tree"].visible_nodes(shapes)
    got, status = opened.visible_nodes(shapes)
    assert np.array_equal(status, built_status) and max(len(v) for v in built) > 5000
    assert all(np.array_equal(a, b) for a, b in zip(got, built))
    opened.free()


def test_render_draws_a_spilled_list_and_cuts_it_inside_a_run_of_ties(ctx, scenes):
    s = scenes["A"]
    tn = R.TreeNodes(s["oracle"], VC.BMIN, VC.BMAX)
    m = VC.ortho()
    want = s["want"][0]
    assert np.array_equal(s["mats"][0], m) and s["mirror"][0].max_heap_len > 256
    sizes = O.cull_cubes(O.SHAPE_FRUSTUM, m, np.array([[*tn.node(n)["cube_min"], tn.node(n)["cube_edge"]] for n in want[298:302]]),
                         with_sizes=True)[1]
    assert len(set(sizes.tolist())) == 1  # the cut at 300 falls between equal keys
    shapes = frusta(ctx, [m])
    for max_nodes in (0, 300):
        rv = s["tree"].render(shapes, 32, 32, max_nodes=max_nodes)
        got = check_views(rv, s["tree"], tn, [m], 32, 32, max_nodes=max_nodes, shapes=shapes)[0]
        assert len(got["drawn"]) == (max_nodes or len(want)) and got["pixels_covered"] > 100
        rv.close()


def test_sparse_cull_sizes_mark_the_corners_at_w_zero(ctx, scenes):
    """pcv_cull_nodes_sparse computes its sizes with the traversal's eight-lanes-per-cube arithmetic: NaN wherever ANY corner of a
    listed cube projects to w == 0 (the reference's project() panics there), as the oracle and the dense matrix have it."""
    s = scenes["A"]
    tree, m = s["tree"], s["tree"].num_nodes
    cases = [(tag, mat) for tag, mat in VC.fixed_cases("A") if O.cached_axes(O.SHAPE_FRUSTUM, mat) is not None]
    counts, idx, rel, sizes = tree.cull_nodes_sparse(frusta(ctx, [mat for _, mat in cases]), m)
    cubes = np.array([[*tree.node(i).cube_min, tree.node(i).cube_edge] for i in range(m)])
    nans = 0
    for f, (tag, mat) in enumerate(cases):
        want_rel, want_sz = O.cull_cubes(O.SHAPE_FRUSTUM, mat, cubes, with_sizes=True)
        keep = np.nonzero(want_rel != 2)[0]
        assert counts[f] == keep.size and np.array_equal(idx[f, :keep.size], keep), tag
        assert np.array_equal(sizes[f, :keep.size], want_sz[keep], equal_nan=True), tag
        nans += int(np.isnan(want_sz[keep]).sum())
    assert nans >= 8
