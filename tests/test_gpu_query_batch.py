"""pcv_query_batch_* (one point query over many locations) against the CPU oracle and the single-location entry points:
segment nodes == nodes_in_location per shape, segment points == decode + FilteredIterator keep mask + retain per node (the
oracle's nodes_in_location / decode_positions / cull_points), byte for byte; u64 offsets past 2^32; ranges, device outputs,
opened directories, lifetimes, and the C example."""
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import point_cloud_viewer_amd as pcv
from point_cloud_viewer_amd import synthetic
from test_gpu_query import ctx, random_frusta, scene  # noqa: F401  (module fixtures + the config-4 frustum generator)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def oracle_segment(sc, kind, params, name, interval):
    """Shape (kind, params)'s points in node `name`: x, y, z, rgb (n x 3), intensity."""
    nd = sc["oracle"].nodes[name]
    if nd["num_points"] == 0:
        return np.zeros(0), np.zeros(0), np.zeros(0), np.zeros((0, 3), np.uint8), np.zeros(0, np.float32)
    info = sc["tree"].node(sc["index_of"][name])
    px, py, pz = O.decode_positions(nd["encoding"], info.cube_min, info.cube_edge, nd["xyz"])
    inten = np.frombuffer(nd["intensity"], dtype=np.float32)
    keep = O.cull_points(kind, params, px, py, pz, inten if interval is not None else None, interval).astype(bool)
    return px[keep], py[keep], pz[keep], np.frombuffer(nd["rgb"], dtype=np.uint8).reshape(-1, 3)[keep], inten[keep]


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def assert_points_equal(got, want, what):
    gx, gy, gz, grgb, gint = got["x"], got["y"], got["z"], got["rgb"].reshape(-1, 3), got["intensity"]
    wx, wy, wz, wrgb, wint = want
    assert got["count"] == wx.size, what
    assert same_bytes(gx, wx) and same_bytes(gy, wy) and same_bytes(gz, wz), what
    assert same_bytes(grgb, wrgb), what
    if gint is not None:
        assert same_bytes(gint, wint), what


def check_against_oracle(sc, batch, kinds, intervals):
    """Every segment of every shape against the oracle; returns the number of non-empty segments."""
    first, nodes, off = batch.segments()
    names = sc["names"]
    full = batch.points()
    assert full["count"] == batch.num_points == int(off[-1])
    nonempty = 0
    for s, (kind, params) in enumerate(kinds):
        want_names = O.nodes_in_location(sc["bmin"], sc["bmax"], sc["oracle"].nodes, kind, params) if kind is not None else []
        got_names = [names[i] for i in nodes[first[s]:first[s + 1]]]
        assert got_names == want_names, s
        for k in range(int(first[s]), int(first[s + 1])):
            a, b = int(off[k]), int(off[k + 1])
            seg = dict(count=b - a, x=full["x"][a:b], y=full["y"][a:b], z=full["z"][a:b], rgb=full["rgb"][a:b],
                       intensity=None if full["intensity"] is None else full["intensity"][a:b])
            assert_points_equal(seg, oracle_segment(sc, kind, params, names[nodes[k]], intervals[s]), (s, k))
            nonempty += b > a
    return nonempty


def scene_of(ctx, x, y, z, rgb, inten, bmin, bmax, cap):  # noqa: F811
    tree = ctx.build(0.001, pcv.Aabb(bmin, bmax), x, y, z, rgb, inten, max_points_per_node=cap)
    with O.max_points_per_node(cap):
        want = O.build_closed(0.001, bmin, bmax, x, y, z, rgb, inten, threads=8)
    names = tree.node_names()
    return dict(bmin=bmin, bmax=bmax, tree=tree, oracle=want, names=names, index_of={n: i for i, n in enumerate(names)})


@pytest.fixture(scope="module")
def sc(scene):  # noqa: F811
    return dict(scene, index_of={n: i for i, n in enumerate(scene["names"])})


def mixed_shapes(sc, seed):
    """All five kinds interleaved, plus a non-invertible frustum: (shapes for ctx.shapes, oracle kinds)."""
    rng = np.random.default_rng(seed)
    bmin, bmax = sc["bmin"], sc["bmax"]
    fr = random_frusta(rng, bmin, bmax, 4)
    obb = (bmin + 45, O.quat_from_axis_angle([1.0, 0.0, 0.0], 0.5), [30.0, 20.0, 15.0])
    lo, hi = bmin + 10, bmin + 60
    shapes = [("frustum2", *fr[0]), ("aabb", lo, hi), ("all",), ("frustum", fr[1][0]), ("frustum", np.zeros(16)), ("obb", *obb),
              ("frustum2", *fr[2]), ("aabb", bmin + 30, bmax - 5), ("frustum", fr[3][0])]
    obbp = list(obb[0]) + list(obb[1]) + list(obb[2])
    kinds = [(O.SHAPE_FRUSTUM2, np.concatenate(fr[0])), (O.SHAPE_AABB, list(lo) + list(hi)), (O.SHAPE_ALL, None),
             (O.SHAPE_FRUSTUM, fr[1][0]), (None, None), (O.SHAPE_OBB, obbp),
             (O.SHAPE_FRUSTUM2, np.concatenate(fr[2])), (O.SHAPE_AABB, list(bmin + 30) + list(bmax - 5)),
             (O.SHAPE_FRUSTUM, fr[3][0])]
    return shapes, kinds


def test_segments_are_the_node_lists(ctx, sc):  # noqa: F811
    shapes, kinds = mixed_shapes(sc, 21)
    prepared = ctx.shapes(shapes)
    batch = sc["tree"].query_batch(prepared)
    first, nodes, off = batch.segments()
    lists = sc["tree"].nodes_in_location(prepared)
    assert first[0] == 0 and first[-1] == batch.num_segments == sum(len(l) for l in lists)
    for s, l in enumerate(lists):
        assert np.array_equal(nodes[first[s]:first[s + 1]], l), s
        kind, params = kinds[s]
        if kind is not None:
            assert [sc["names"][i] for i in l] == O.nodes_in_location(sc["bmin"], sc["bmax"], sc["oracle"].nodes, kind, params)
    assert first[5] == first[4]  # the non-invertible frustum: no segments
    assert np.all(np.diff(off.astype(np.int64)) >= 0)
    assert first[3] - first[2] == sc["tree"].num_nodes  # AllPoints lists every node, empty ones included
    batch.free()


def test_points_per_segment_equal_the_oracle_with_per_shape_intervals(ctx, sc):  # noqa: F811
    shapes, kinds = mixed_shapes(sc, 22)
    ivs = [None, (20.0, 180.0), (180.0, 20.0), (float("nan"), 100.0), None, (20.0, 180.0), (5.0, float("nan")), None, (20.0, 180.0)]
    prepared = ctx.shapes(shapes)
    batch = sc["tree"].query_batch(prepared, intervals=ivs)
    del prepared  # the batch does not need the shapes any more
    assert check_against_oracle(sc, batch, kinds, ivs) >= 20
    first, _, off = batch.segments()
    assert off[first[2]] == off[first[3]]  # lo > hi: nothing passes
    assert off[first[3]] == off[first[4]]  # NaN bound: nothing passes


def test_batch_equals_query_points_and_query_node_points(ctx, sc):  # noqa: F811
    """~2 000 random config-4 frusta over the 300 k scene: every shape's concatenation == query_points; every segment of 40
    of them == query_points(node=...)."""
    rng = np.random.default_rng(23)
    fr = random_frusta(rng, sc["bmin"], sc["bmax"], 2000)
    prepared = ctx.shapes([("frustum2", c, q) for c, q in fr])
    tree = sc["tree"]
    batch = tree.query_batch(prepared)
    first, nodes, off = batch.segments()
    full = batch.points()
    total = 0
    for s in range(len(fr)):
        a, b = int(off[first[s]]), int(off[first[s + 1]])
        want = tree.query_points(prepared, s)
        assert want["count"] == b - a, s
        assert same_bytes(full["x"][a:b], want["x"]) and same_bytes(full["y"][a:b], want["y"]) and same_bytes(full["z"][a:b], want["z"])
        assert same_bytes(full["rgb"][a:b], want["rgb"]) and same_bytes(full["intensity"][a:b], want["intensity"])
        total += want["count"]
    assert total == batch.num_points > 0
    for s in rng.choice(len(fr), 40, replace=False):
        for k in range(int(first[s]), int(first[s + 1])):
            want = tree.query_points(prepared, int(s), node=int(nodes[k]))
            got = batch.node_points(int(s), int(nodes[k]))
            assert got["count"] == want["count"] == int(off[k + 1] - off[k])
            assert same_bytes(got["x"], want["x"]) and same_bytes(got["rgb"], want["rgb"]) and same_bytes(got["intensity"], want["intensity"])


def test_all_four_encodings(ctx):  # noqa: F811
    """test_query_points_all_four_encodings' city-scale cloud: every chunk size of the staged decode in one batch."""
    x, y, z, rgb, bmin, bmax = synthetic.gaussian_clusters(340_000, seed=12, num_clusters=6, extent=30000.0,
                                                           sigma_range=(5.0, 400.0), offset=(-2.7e6, -4.3e6, 3.8e6))
    rng = np.random.default_rng(13)
    c = np.array([x[0], y[0], z[0]])
    x = np.concatenate([x, c[0] + rng.normal(0.0, 0.03, 60_000)])
    y = np.concatenate([y, c[1] + rng.normal(0.0, 0.03, 60_000)])
    z = np.concatenate([z, c[2] + rng.normal(0.0, 0.03, 60_000)])
    rgb = synthetic.index_colors(x.size)
    bmin, bmax = np.array([x.min(), y.min(), z.min()]), np.array([x.max(), y.max(), z.max()])
    inten = (np.arange(x.size) % 251).astype(np.float32)
    s = scene_of(ctx, x, y, z, rgb, inten, bmin, bmax, 1500)
    tree = s["tree"]
    assert {tree.node(i).encoding for i in range(tree.num_nodes) if tree.node(i).num_points > 0} == {1, 2, 3, 4}
    lo, hi = bmin + (bmax - bmin) * 0.1, bmin + (bmax - bmin) * 0.8
    clo, chi = c - 0.05, c + 0.04
    shapes = [("all",), ("aabb", lo, hi), ("aabb", clo, chi), ("all",), ("aabb", lo, hi)]
    kinds = [(O.SHAPE_ALL, None), (O.SHAPE_AABB, list(lo) + list(hi)), (O.SHAPE_AABB, list(clo) + list(chi)), (O.SHAPE_ALL, None),
             (O.SHAPE_AABB, list(lo) + list(hi))]
    ivs = [None, None, None, (20.0, 180.0), (20.0, 180.0)]
    batch = tree.query_batch(ctx.shapes(shapes), intervals=ivs)
    assert check_against_oracle(s, batch, kinds, ivs) >= 10
    assert batch.shape_points(0)["count"] == tree.num_points
    batch.free()
    tree.free()


def test_box_faces_on_decoded_positions_in_one_batch(ctx):  # noqa: F811
    """Boxes whose faces are decoded point positions, one ulp beside them, missing, inverted and NaN boxes, with and without the
    interval — all in one batch (cf. test_box_faces_on_decoded_positions_keep_the_reference_ties)."""
    x, y, z, rgb, bmin, bmax = synthetic.gaussian_clusters(3_000_000, seed=6, num_clusters=4, extent=300.0, sigma_range=(0.5, 20.0))
    inten = (np.arange(x.size) % 251).astype(np.float32)
    s = scene_of(ctx, x, y, z, rgb, inten, bmin, bmax, 20000)
    tree, want = s["tree"], s["oracle"]
    rng = np.random.default_rng(12)
    faces = []
    for name, nd in want.nodes.items():
        if nd["num_points"] > 100 and len(faces) < 6 and rng.random() < 0.02:
            info = tree.node(s["index_of"][name])
            px, py, pz = O.decode_positions(nd["encoding"], info.cube_min, info.cube_edge, nd["xyz"])
            k = int(rng.integers(0, px.size))
            faces.append(np.array([px[k], py[k], pz[k]]))
    assert len(faces) >= 4
    boxes = []
    for a, b in zip(faces[0::2], faces[1::2]):
        lo, hi = np.minimum(a, b), np.maximum(a, b)
        boxes += [(lo, hi), (np.nextafter(lo, np.inf), np.nextafter(hi, np.inf)), (np.nextafter(lo, -np.inf), np.nextafter(hi, -np.inf)),
                  (lo - 7.5, hi + 3.25)]
    boxes += [(bmax + 1.0, bmax + 2.0), (bmin + 50.0, bmin + 20.0), (np.array([np.nan, bmin[1], bmin[2]]), bmax),
              (bmin, np.array([bmax[0], np.nan, bmax[2]])), (bmin - 1.0, bmax + 1.0)]
    shapes = [("aabb", lo, hi) for lo, hi in boxes] * 2
    kinds = [(O.SHAPE_AABB, list(lo) + list(hi)) for lo, hi in boxes] * 2
    ivs = [None] * len(boxes) + [(20.0, 180.0)] * len(boxes)
    batch = tree.query_batch(ctx.shapes(shapes), intervals=ivs)
    assert check_against_oracle(s, batch, kinds, ivs) >= 8
    assert batch.shape_points(len(boxes) - 1)["count"] == tree.num_points
    batch.free()
    tree.free()


def test_ranges_and_outputs(ctx, sc):  # noqa: F811
    import torch
    shapes, _ = mixed_shapes(sc, 24)
    batch = sc["tree"].query_batch(ctx.shapes(shapes))
    full = batch.points()
    _, _, off = batch.segments()
    ns = batch.num_segments
    rng = np.random.default_rng(25)
    for _ in range(25):
        a = int(rng.integers(0, ns + 1))
        n = int(rng.integers(0, ns - a + 1))
        got = batch.points(a, n)
        p0, p1 = int(off[a]), int(off[a + n])
        assert got["count"] == p1 - p0
        for key in ("x", "y", "z", "rgb", "intensity"):
            assert same_bytes(got[key], full[key][p0:p1]), (a, n, key)
    # device outputs, and host outputs the caller owns
    a, n = 3, ns - 7
    p0, p1 = int(off[a]), int(off[a + n])
    cnt = p1 - p0
    dev = dict(x=torch.zeros(cnt, dtype=torch.float64, device="cuda"), y=torch.zeros(cnt, dtype=torch.float64, device="cuda"),
               z=torch.zeros(cnt, dtype=torch.float64, device="cuda"), rgb=torch.zeros((cnt, 3), dtype=torch.uint8, device="cuda"),
               intensity=torch.zeros(cnt, dtype=torch.float32, device="cuda"))
    got = batch.points(a, n, out=dev)
    torch.cuda.synchronize()
    for key in ("x", "y", "z", "rgb", "intensity"):
        assert same_bytes(got[key].cpu().numpy(), full[key][p0:p1]), key
    # a capacity one too small, a range past the end: PcvError, nothing written
    small = {k: torch.full_like(v[:-1] if v.ndim == 1 else v[:-1], 7) for k, v in dev.items()}
    with pytest.raises(pcv.PcvError):
        batch.points(a, n, out=small)
    host = dict(x=np.full(cnt - 1, 7.0), y=np.full(cnt - 1, 7.0), z=np.full(cnt - 1, 7.0), rgb=np.full((cnt - 1, 3), 7, np.uint8),
                intensity=np.full(cnt - 1, 7.0, np.float32))
    with pytest.raises(pcv.PcvError):
        batch.points(a, n, out=host)
    with pytest.raises(pcv.PcvError):
        batch.points(ns - 2, 3)
    with pytest.raises(pcv.PcvError):
        batch.points(ns + 1, 0)
    torch.cuda.synchronize()
    assert all(bool((v == 7).all()) for v in small.values())
    assert all(bool((v == 7).all()) for v in host.values())
    batch.free()


def test_opened_directory_gives_the_same_batch(ctx, sc, tmp_path):  # noqa: F811
    x, y, z, rgb, bmin, bmax = synthetic.gaussian_clusters(300_000, seed=2, num_clusters=6, extent=100.0, sigma_range=(0.5, 6.0))
    inten = (np.arange(x.size) % 251).astype(np.float32)
    with O.max_points_per_node(2000):
        O.build_literal_dir(tmp_path / "oracle", 0.001, bmin, bmax, x, y, z, rgb, inten, threads=4)
    opened = ctx.open_dir(tmp_path / "oracle")
    assert opened.node_names() == sc["names"]
    shapes, _ = mixed_shapes(sc, 26)
    prepared = ctx.shapes(shapes)
    ivs = [None, (20.0, 180.0)] * 4 + [None]
    a, b = sc["tree"].query_batch(prepared, ivs), opened.query_batch(prepared, ivs)
    for p, q in zip(a.segments(), b.segments()):
        assert np.array_equal(p, q)
    pa, pb = a.points(), b.points()
    for key in ("x", "y", "z", "rgb", "intensity"):
        assert same_bytes(pa[key], pb[key]), key
    b.free()
    opened.free()


def test_offsets_beyond_2_to_the_32(ctx):  # noqa: F811
    x, y, z, rgb, bmin, bmax = synthetic.gaussian_clusters(4_000_000, seed=27, num_clusters=5, extent=200.0, sigma_range=(1.0, 20.0))
    tree = ctx.build(0.001, pcv.Aabb(bmin, bmax), x, y, z, rgb, max_points_per_node=20000)
    n, m, S = tree.num_points, tree.num_nodes, 1100
    batch = tree.query_batch(ctx.shapes([("all",)] * S))
    assert batch.num_points == S * n > 1 << 32
    first, nodes, off = batch.segments()
    assert np.array_equal(first, np.arange(S + 1, dtype=np.uint64) * m)
    assert np.array_equal(nodes[:m], np.arange(m)) and np.array_equal(nodes[-m:], np.arange(m))
    assert np.array_equal(off[first], np.arange(S + 1, dtype=np.uint64) * n)
    last = batch.shape_points(S - 1)
    want = tree.query_points(ctx.shapes([("all",)]), 0)
    assert last["count"] == want["count"] == n
    for key in ("x", "y", "z", "rgb"):
        assert same_bytes(last[key], want[key]), key
    batch.free()
    tree.free()


def test_edges_and_lifetimes(ctx, sc, tmp_path):  # noqa: F811
    tree = sc["tree"]
    none = tree.query_batch(ctx.shapes([]))
    assert (none.num_segments, none.num_points) == (0, 0)
    assert none.points()["count"] == 0 and none.segments()[0].tolist() == [0]
    bmin, bmax = np.array([-1.0, 2.0, 3.0]), np.array([4.0, 5.0, 9.0])
    pcv.build_octree(str(tmp_path / "empty"), 0.01, pcv.Aabb(bmin, bmax), iter([]), attributes=("color",), ctx=ctx).free()
    empty = ctx.open_dir(tmp_path / "empty")
    assert empty.num_nodes == 0
    eb = empty.query_batch(ctx.shapes([("all",), ("aabb", bmin, bmax)]))
    assert (eb.num_segments, eb.num_points) == (0, 0) and eb.segments()[0].tolist() == [0, 0, 0]
    # an interval on an octree without intensity: PcvError, and the context goes on working
    x, y, z, rgb, lo, hi = synthetic.gaussian_clusters(20_000, seed=28, num_clusters=2, extent=10.0, sigma_range=(0.5, 2.0))
    plain = ctx.build(0.001, pcv.Aabb(lo, hi), x, y, z, rgb, max_points_per_node=500)
    sh = ctx.shapes([("all",), ("aabb", lo, (lo + hi) / 2)])
    with pytest.raises(pcv.PcvError):
        plain.query_batch(sh, intervals=[None, (0.0, 1.0)])
    ok = plain.query_batch(sh)
    assert ok.num_points == plain.query_points(sh, 0)["count"] + plain.query_points(sh, 1)["count"]
    assert ok.shape_points(0)["intensity"] is None
    # the batch holds its tree; a freed tree is an error, not a read of freed memory
    plain.free()
    with pytest.raises(pcv.PcvError):
        ok.points()
    # Context.close() with a live batch and tree frees the children in any order
    c2 = pcv.Context(0)
    t2 = c2.build(0.001, pcv.Aabb(lo, hi), x, y, z, rgb, max_points_per_node=500)
    b2 = t2.query_batch(c2.shapes([("all",)]))
    assert b2.num_points == t2.num_points
    c2.close()
    with pytest.raises(pcv.PcvError):
        b2.points()


def test_c_example_prints_the_batch_counts(ctx, sc, tmp_path):  # noqa: F811
    sc["tree"].write_dir(tmp_path / "oct")
    tiles = 8
    p = subprocess.run([os.path.join(ROOT, "examples", "bin", "query_batch"), str(tmp_path / "oct"), str(tiles)], capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    got = [tuple(int(v) for v in line.split()) for line in p.stdout.splitlines()]
    opened = ctx.open_dir(tmp_path / "oct")
    m = opened.meta()
    bmin, bmax = m["bbox_min"], m["bbox_max"]
    shapes = []
    for i in range(tiles):
        for j in range(tiles):
            lo = [bmin[0] + (bmax[0] - bmin[0]) * i / tiles, bmin[1] + (bmax[1] - bmin[1]) * j / tiles, bmin[2]]
            hi = [bmin[0] + (bmax[0] - bmin[0]) * (i + 1) / tiles, bmin[1] + (bmax[1] - bmin[1]) * (j + 1) / tiles, bmax[2]]
            shapes.append(("aabb", lo, hi))
    batch = opened.query_batch(ctx.shapes(shapes))
    first, _, off = batch.segments()
    want = [(k // tiles, k % tiles, int(off[first[k + 1]] - off[first[k]])) for k in range(tiles * tiles)]
    assert got == want
    assert sum(c for _, _, c in want) > 0
    opened.free()
