"""Oriented boxes and frusta AT their faces, on the device: the two location kinds whose f64 chains are the longest of the
query path and which the other files compare with the oracle on random points and random shapes only — inputs that never come
within an ulp of a face, so that a fused multiply-add, a reordered sum or `<=` turned into `<` would pass them all
(tests/test_contain_truth_cpu.py shows it on a contracted build of the oracle). Inputs and truths come from
tests/contain_truth.py: exact scenes (the chain rounds nowhere; truth = the exact rule in rationals, no exception), points planted
on faces and 1-3 `nextafter` steps beside them, shapes planted through node cube corners and stored points (truth = the oracle).
Every comparison is flag for flag or Relation for Relation; there is no tolerance anywhere."""
import numpy as np
import pytest

import contain_truth as T
import oracle_lib as O
import point_cloud_viewer_amd as pcv
from point_cloud_viewer_amd import synthetic
from test_contain_truth_cpu import KIND, MAKE_FRUSTUM, params_of

pytestmark = pytest.mark.gpu

SLICES = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025)
INTERVAL = (10.0, 99.5)


@pytest.fixture(scope="module")
def ctx():
    c = pcv.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def planted():
    return {scale: T.planted_points_scene(scale, MAKE_FRUSTUM) for scale in T.SCALES}


def _intensity(n):
    return (np.arange(n) % 251).astype(np.float32)


def _in_interval(inten):
    v = inten.astype(np.float64)
    return (INTERVAL[0] <= v) & (v <= INTERVAL[1])


def _cull_all_ways(ctx, prepared, i, x, y, z, want, ways=(0, 1, 2, 3)):
    """cull_points of shape i from host arrays / device tensors, without / with the intensity interval: flags and kept count."""
    import torch
    inten = _intensity(x.size)
    for way in ways:
        device, interval = way & 1, way & 2
        args = [x, y, z] + ([inten] if interval else [])
        if device:
            args = [torch.tensor(a, device="cuda") for a in args]
        keep, kept = ctx.cull_points(prepared, i, *args, interval=INTERVAL if interval else None)
        keep = keep.cpu().numpy() if device else keep
        expect = want & _in_interval(inten) if interval else want
        assert np.array_equal(keep.astype(bool), expect) and kept == int(expect.sum()), (i, way, x.size)


# ---- raw arrays: cull_points_kernel<OBB | FRUSTUM>, positions as given -----------------------------------------------------
def test_exact_scenes_equal_the_exact_rule(ctx):
    s = T.obb_exact_scene()
    prepared = ctx.shapes([("obb", *sh) for sh in s["shapes"]])
    assert sum(s["on_face"][:20]) == 6120
    for i, want in enumerate(s["want"]):
        _cull_all_ways(ctx, prepared, i, s["x"], s["y"], s["z"], want)
    f = T.frustum_exact_scene()
    prepared = ctx.shapes([("frustum", m) for m in f["shapes"]])
    assert f["on_plane"][0] == 578 and f["kept"][0] == 851
    for i, want in enumerate(f["want"]):
        _cull_all_ways(ctx, prepared, i, f["x"], f["y"], f["z"], want)


@pytest.mark.parametrize("scale", list(T.SCALES))
def test_planted_points_equal_the_oracle(ctx, planted, scale):
    sc = planted[scale]
    prepared = ctx.shapes(sc["shapes"])
    both = 0
    for i, sh in enumerate(sc["shapes"]):
        want = O.cull_points(KIND[sh[0]], params_of(sh), sc["x"], sc["y"], sc["z"]).astype(bool)
        _cull_all_ways(ctx, prepared, i, sc["x"], sc["y"], sc["z"], want)
        mine = want[sc["owner"] == i]
        both += bool(mine.any() and not mine.all())
    assert both == len(sc["shapes"])


@pytest.mark.parametrize("scale", list(T.SCALES))
def test_planted_points_through_every_lane_group_and_the_ragged_tail(ctx, planted, scale):
    """The first n points, n around the 64-lane group, the 256-thread block and the 1 024-point chunk of four groups: a shape's
    own planted points come first, so every slice is made of them."""
    sc = planted[scale]
    prepared = ctx.shapes(sc["shapes"])
    for i in (0, 7, 10, 17):  # two boxes, two frusta
        sh = sc["shapes"][i]
        order = np.concatenate([np.flatnonzero(sc["owner"] == i), np.flatnonzero(sc["owner"] != i)])
        x, y, z = (np.ascontiguousarray(sc[k][order]) for k in "xyz")
        want = O.cull_points(KIND[sh[0]], params_of(sh), x, y, z).astype(bool)
        assert want[:1025].any() and not want[:1025].all()
        for k, n in enumerate(SLICES):
            _cull_all_ways(ctx, prepared, i, x[:n], y[:n], z[:n], want[:n], ways=(k % 4, (k + 3) % 4))


def test_degenerate_shapes_and_non_finite_points(ctx):
    """Zero, negative and NaN half extents, a singular clip matrix, a zero bottom row, NaN / inf coordinates: the flags of
    cull_points are the rule's (exact scene inputs: the exact rule), and in one table with sound shapes nobody disturbs anybody."""
    s, f = T.obb_exact_scene(), T.frustum_exact_scene()
    singular = f["shapes"][0].copy()
    singular[4:8] = singular[0:4]  # two equal columns
    assert O.mat4_try_inverse(singular) is None and O.mat4_try_inverse(f["shapes"][-1]) is None
    specs = [("obb", *s["shapes"][k]) for k in (20, 21, 22, 7)] + [("frustum", singular), ("frustum", f["shapes"][-1]), ("frustum", f["shapes"][0])]
    prepared = ctx.shapes(specs)
    assert [prepared.get(k)[2] for k in range(7)] == [True, True, True, True, False, False, True]
    for i, spec in enumerate(specs):
        for scene in (s, f):
            x, y, z = scene["x"], scene["y"], scene["z"]
            if spec[0] == "obb":
                tail = [T.obb_contains_exact(*spec[1:], (x[k], y[k], z[k])) for k in range(scene["finite"], x.size)]
                want = np.concatenate([T.obb_exact(*spec[1:], x[:scene["finite"]], y[:scene["finite"]], z[:scene["finite"]])[0], tail])
            else:
                tail = [T.frustum_contains_exact(spec[1], (x[k], y[k], z[k])) for k in range(scene["finite"], x.size)]
                want = np.concatenate([T.frustum_exact(spec[1], x[:scene["finite"]], y[:scene["finite"]], z[:scene["finite"]])[0], tail])
            assert np.array_equal(want, O.cull_points(KIND[spec[0]], params_of(spec), x, y, z).astype(bool)), i
            assert not want[scene["finite"]:].any()
            _cull_all_ways(ctx, prepared, i, x, y, z, want.astype(bool), ways=(0, 3))


# ---- an octree: query_flags_kernel, staged_keep_enc<KIND, ENC>, cull_points_kernel on encoded nodes -------------------------
class _Oracle:
    """nodes_in_location + decode + keep of the oracle over one built tree, the tree's arrays and decodes made once."""

    def __init__(self, tree, want, bmin, bmax):
        self.tree, self.nodes, self.bmin, self.bmax = tree, want.nodes, np.asarray(bmin, dtype=np.float64), np.asarray(bmax, dtype=np.float64)
        self.names = tree.node_names()
        self.index_of = {name: i for i, name in enumerate(self.names)}
        self.arrays = O._tree_arrays(self.nodes)
        self.decoded = {}

    def nodes_in(self, shape):
        hi, lo, npnts = self.arrays
        ohi, olo = np.zeros(hi.size, dtype=np.uint64), np.zeros(hi.size, dtype=np.uint64)
        p = np.ascontiguousarray(params_of(shape))
        n = O.lib().pcvo_nodes_in_location(O._d(self.bmin), O._d(self.bmax), hi.size, hi.ctypes.data_as(O._u64p), lo.ctypes.data_as(O._u64p),
                                           npnts.ctypes.data_as(O._i64p), KIND[shape[0]], O._d(p), ohi.ctypes.data_as(O._u64p),
                                           olo.ctypes.data_as(O._u64p))
        return None if n < 0 else [O.node_id_str(int(ohi[i]), int(olo[i])) for i in range(n)]

    def positions(self, name):
        if name not in self.decoded:
            nd, info = self.nodes[name], self.tree.node(self.index_of[name])
            self.decoded[name] = O.decode_positions(nd["encoding"], info.cube_min, info.cube_edge, nd["xyz"])
        return self.decoded[name]

    def keep(self, shape, name, interval=None):
        px, py, pz = self.positions(name)
        inten = np.frombuffer(self.nodes[name]["intensity"], dtype=np.float32)
        return O.cull_points(KIND[shape[0]], params_of(shape), px, py, pz, inten if interval else None, interval).astype(bool)

    def check_batch(self, ctx, shapes, intervals=None):
        """One query_batch of all shapes: per shape the oracle's node list, per node the oracle's kept points, in order."""
        prepared = ctx.shapes(shapes)
        batch = self.tree.query_batch(prepared, intervals)
        first, node, off = batch.segments()
        kept = 0
        try:
            for s, shape in enumerate(shapes):
                names = self.nodes_in(shape) or []  # None: no frustum (the reference panics); the device lists nothing
                got_nodes = [self.names[k] for k in node[int(first[s]):int(first[s + 1])]]
                assert got_nodes == names, (s, shape[0])
                want = [self.keep(shape, n, intervals[s] if intervals else None) for n in names]
                sizes = np.diff(off[int(first[s]):int(first[s + 1]) + 1].astype(np.int64))
                assert sizes.tolist() == [int(w.sum()) for w in want], (s, shape[0])
                if sizes.sum():
                    got = batch.shape_points(s)
                    for axis, key in enumerate("xyz"):
                        assert np.array_equal(got[key], np.concatenate([self.positions(n)[axis][w] for n, w in zip(names, want)])), (s, key)
                kept += int(sizes.sum())
        finally:
            batch.free()
        return prepared, kept


@pytest.fixture(scope="module")
def city(ctx):
    """The city-scale tree of test_query_points_all_four_encodings: Float64, Float32, UInt16 and UInt8 nodes."""
    x, y, z, rgb, bmin, bmax = synthetic.gaussian_clusters(340_000, seed=12, num_clusters=6, extent=30000.0, sigma_range=(5.0, 400.0),
                                                           offset=(-2.7e6, -4.3e6, 3.8e6))
    rng = np.random.default_rng(13)
    c = np.array([x[0], y[0], z[0]])
    x, y, z = (np.concatenate([v, c[a] + rng.normal(0.0, 0.03, 60_000)]) for a, v in enumerate((x, y, z)))
    rgb = synthetic.index_colors(x.size)
    bmin, bmax = np.array([x.min(), y.min(), z.min()]), np.array([x.max(), y.max(), z.max()])
    inten = _intensity(x.size)
    tree = ctx.build(0.001, pcv.Aabb(bmin, bmax), x, y, z, rgb, inten, max_points_per_node=1500)
    with O.max_points_per_node(1500):
        want = O.build_closed(0.001, bmin, bmax, x, y, z, rgb, inten, threads=8)
    oracle = _Oracle(tree, want, bmin, bmax)
    # two stored points per encoding: (node name, index in the node)
    # two stored points per encoding (of two nodes where there are two: the root alone is Float64)
    by_encoding = {1: [], 2: [], 3: [], 4: []}
    for name, nd in want.nodes.items():
        if nd["num_points"] >= 4 and len(by_encoding[nd["encoding"]]) < 2:
            by_encoding[nd["encoding"]].append(name)
    assert all(by_encoding.values()), by_encoding
    picks = [(names[k % len(names)], (want.nodes[names[k % len(names)]]["num_points"] // 2 + 3 * k) % want.nodes[names[k % len(names)]]["num_points"])
             for names in by_encoding.values() for k in range(2)]
    targets = [np.array([oracle.positions(name)[a][k] for a in range(3)]) for name, k in picks]
    families, shapes = T.planted_stored_shapes(MAKE_FRUSTUM, targets)
    yield dict(oracle=oracle, picks=picks, targets=targets, families=families, shapes=shapes)
    tree.free()


def test_stored_points_of_all_four_encodings_in_one_batch(ctx, city):
    """Boxes and frusta with a face through a stored point, general rotations and the exact closed / open pairs, every encoding:
    the batch's segments against the oracle's decode + rule, with and without the intensity interval."""
    oracle, shapes = city["oracle"], city["shapes"]
    assert len(shapes) == 8 * (13 + 13 + 24)
    _, kept = oracle.check_batch(ctx, shapes)
    assert kept > 1000
    intervals = [INTERVAL if s % 2 else None for s in range(len(shapes))]
    oracle.check_batch(ctx, shapes, intervals)


def test_stored_points_flip_on_the_device(ctx, city):
    """cull_node_points of the stored point's node under every shape of its families: the oracle's flags, the stored point kept
    by some shapes of a family and dropped by others, kept at the closed face and dropped one step inside it."""
    oracle, shapes = city["oracle"], city["shapes"]
    prepared = ctx.shapes(shapes)
    for fam in city["families"]:
        name, k = city["picks"][fam["target"]]
        flags = []
        for s in range(fam["first"], fam["first"] + fam["count"]):
            keep, kept = oracle.tree.cull_node_points(prepared, s, oracle.index_of[name])
            want = oracle.keep(shapes[s], name)
            assert np.array_equal(keep.astype(bool), want) and kept == int(want.sum()), (fam, s)
            flags.append(bool(keep[k]))
        assert set(flags) == {False, True}, fam
        if fam["kind"] == "pair":
            p = city["targets"][fam["target"]]
            assert fam["exact"] and flags == [True, False]
            assert flags == [T.obb_contains_exact(*shapes[fam["first"] + j][1:], p) for j in range(2)]  # the exact rule on the decoded values
    s = city["families"][0]["first"]
    name = city["picks"][0][0]
    keep, _ = oracle.tree.cull_node_points(prepared, s, oracle.index_of[name], interval=INTERVAL)
    assert np.array_equal(keep.astype(bool), oracle.keep(shapes[s], name, INTERVAL))


# ---- S2 clouds: s2_flags_kernel<OBB | FRUSTUM> on the stored f64 -----------------------------------------------------------
def test_s2_segments_of_the_planted_ecef_set(ctx, planted):
    sc = planted["ecef"]
    n = sc["x"].size
    cloud = ctx.s2_split(dict(x=sc["x"], y=sc["y"], z=sc["z"], color=np.zeros((n, 3), dtype=np.uint8), intensity=_intensity(n)), 20)
    xyz, _, inten = cloud.cell_points()
    px, py, pz = (np.ascontiguousarray(xyz[:, a]) for a in range(3))
    owner = sc["owner"][cloud.order]
    assert np.array_equal(px, sc["x"][cloud.order])  # the stored f64, untouched
    _, counts, offsets = cloud.cells
    prepared = ctx.shapes(sc["shapes"])
    lists = cloud.cells_in_location_indices(prepared)
    try:
        for intervals in (None, [INTERVAL if s % 2 else None for s in range(len(sc["shapes"]))]):
            batch = cloud.query_batch(prepared, None, intervals)
            first, cell, off = batch.segments()
            assert np.array_equal(cell, np.concatenate(lists))
            for s, shape in enumerate(sc["shapes"]):
                flags = O.cull_points(KIND[shape[0]], params_of(shape), px, py, pz).astype(bool)
                want = flags & _in_interval(inten) if intervals and intervals[s] else flags
                slots = np.concatenate([np.arange(int(offsets[c]), int(offsets[c] + counts[c])) for c in lists[s]])
                mine = flags[slots][owner[slots] == s]
                assert mine.size > 500 and mine.any() and not mine.all(), s  # the listed cells hold the planted points, both flags
                sizes = np.diff(off[int(first[s]):int(first[s + 1]) + 1].astype(np.int64))
                assert sizes.tolist() == [int(want[int(offsets[c]):int(offsets[c] + counts[c])].sum()) for c in lists[s]], s
                got = batch.shape_points(s)
                assert np.stack([got["x"], got["y"], got["z"]], axis=1).tobytes() == xyz[slots[want[slots]]].tobytes(), s
            batch.free()
    finally:
        cloud.free()  # its batches with it


# ---- node level: the dense kernel, the sparse kernel, the tree walk and the one-lane walk ----------------------------------
@pytest.fixture(scope="module")
def cube_scene(ctx):
    """The power-of-two scene of test_gpu_query_fuzz.py: cube [0, 64]^3, every node plane a representable number."""
    x, y, z, rgb, _, _ = synthetic.gaussian_clusters(200_000, seed=12, num_clusters=5, extent=64.0, sigma_range=(0.3, 5.0))
    bmin, bmax = np.zeros(3), np.full(3, 64.0)
    x, y, z = (np.clip(v, 0.0, 64.0) for v in (x, y, z))
    inten = _intensity(x.size)
    tree = ctx.build(0.001, pcv.Aabb(bmin, bmax), x, y, z, rgb, inten, max_points_per_node=1500)
    with O.max_points_per_node(1500):
        want = O.build_closed(0.001, bmin, bmax, x, y, z, rgb, inten, threads=4)
    cubes = np.array([[*tree.node(i).cube_min, tree.node(i).cube_edge] for i in range(tree.num_nodes)])
    levels = np.array([tree.node(i).level for i in range(tree.num_nodes)])
    yield dict(tree=tree, cubes=cubes, levels=levels, oracle=_Oracle(tree, want, bmin, bmax))
    tree.free()


def test_faces_through_node_cube_corners(ctx, cube_scene):
    """About 600 boxes and frusta with a face through (and 1-2 steps beside) a corner of a node cube of levels 1-5, one table:
    pcv_cull_nodes rows, pcv_cull_nodes_sparse lists and nodes_in_location against the oracle's sat() and its BFS."""
    tree, cubes, levels, oracle = (cube_scene[k] for k in ("tree", "cubes", "levels", "oracle"))
    rng = np.random.default_rng(31)
    targets = []
    for k in range(24):
        of_level = cubes[levels == 1 + k % 5]
        of_level = of_level[np.lexsort(of_level.T)]  # whatever order the tree lists its nodes in
        c = of_level[int(rng.integers(0, len(of_level)))]
        targets.append((c[:3].copy(), float(c[3])))
    families, shapes = T.planted_node_shapes(MAKE_FRUSTUM, targets)
    assert len(shapes) == 624
    prepared = ctx.shapes(shapes)
    rel = tree.cull_nodes(prepared)
    counts, idx, srel, _ = tree.cull_nodes_sparse(prepared, tree.num_nodes, with_sizes=False)
    got = tree.nodes_in_location(prepared)
    seen, flips = set(), 0
    for (kind, corner, start), (cube_min, edge) in zip(families, [t for t in targets for _ in range(2)]):
        touching = int(np.flatnonzero(np.all(cubes[:, :3] == cube_min, axis=1) & (cubes[:, 3] == edge))[0])
        rows = []
        for i in range(start, start + 13):
            want = O.cull_cubes(KIND[shapes[i][0]], params_of(shapes[i]), cubes)
            assert np.array_equal(rel[i], want), (i, kind)
            keep = np.flatnonzero(want != 2)
            assert counts[i] == keep.size and np.array_equal(idx[i, :keep.size], keep) and np.array_equal(srel[i, :keep.size], want[keep]), (i, kind, "sparse")
            assert [oracle.names[k] for k in got[i]] == oracle.nodes_in(shapes[i]), (i, kind, "walk")
            seen |= set(np.unique(want).tolist())
            rows.append(int(rel[i][touching]))
        flips += len(set(rows)) > 1
    assert seen == {0, 1, 2}
    # the families do decide Relations: the node that touches the face in the corner changes its own within a family — in every
    # third one at least (the SAT's tie lies a few steps from the point rule's, which the families are centred on; on nodes of
    # the full cube grid the oracle counts 23 of 48)
    assert flips >= len(families) // 3, flips


def test_degenerate_shapes_in_one_batch(ctx, cube_scene):
    """Zero, negative and NaN half extents, a singular matrix and a zero bottom row among sound shapes, one table, one batch:
    the segments are the oracle's for every shape; the matrices without an inverse are no frustum and list nothing."""
    s, f = T.obb_exact_scene(), T.frustum_exact_scene()
    singular = f["shapes"][0].copy()
    singular[4:8] = singular[0:4]
    oracle = cube_scene["oracle"]
    crowd = np.array([np.median(v) for v in oracle.positions("r")])  # where the points are
    centre, quat = tuple(np.round(crowd * 4.0) / 4.0), T.EXACT_QUATS[6]
    sound = MAKE_FRUSTUM(crowd + np.array([0.0, 0.0, 40.0]), T.EXACT_ROTATIONS[0][0], (1.0, 1.0, 0.5, 80.0))
    shapes = [("obb", centre, quat, (8.0, 4.0, 10.0)), ("obb", centre, quat, (8.0, 0.0, 10.0)), ("obb", centre, quat, (8.0, -4.0, 10.0)),
              ("obb", centre, quat, (8.0, 4.0, np.nan)), ("frustum", singular), ("frustum", f["shapes"][-1]), ("frustum2", *sound),
              ("frustum", sound[0])]
    assert oracle.nodes_in(shapes[4]) is None and oracle.nodes_in(shapes[5]) is None
    prepared, kept = oracle.check_batch(ctx, shapes)
    assert kept > 0
    batch = oracle.tree.query_batch(prepared)
    try:
        first, _, _ = batch.segments()
        assert first[5] == first[4] == first[6] and first[1] > 0 and first[7] > first[6] and batch.shape_points(0)["count"] > 0
    finally:
        batch.free()
