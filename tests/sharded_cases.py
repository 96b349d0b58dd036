"""Cases of the sharded-build fuzz (tests/test_sharded_fuzz_cpu.py on the host backend, tests/test_gpu_sharded_fuzz.py on the
HIP backend): the clouds of the streamed-ingest fuzz (test_gpu_stream_fuzz._draw: octant-plane ties and their 1-2 ulp neighbours,
duplicates, planes, lines, far origins, every level-1 coding regime) cut into rank slices the way no even split does, and named
cases the draw cannot guarantee. Importable without a GPU; `facts` needs the oracle only.

A case is a dict: name, x, y, z, rgb, intensity or None, bmin, bmax, res, cap, world, shard_mode, compress, cuts (world + 1
offsets into the cloud: rank r holds [cuts[r], cuts[r + 1])), views (every rank passes views of ONE tensor of the whole cloud, so
that addresses fall where the cuts fall; otherwise fresh contiguous copies), regime, kind, cut_kind."""
import functools

import numpy as np

from test_gpu_build import special_coordinates_cloud
from test_gpu_stream_fuzz import REGIMES, _draw

SEEDS = list(range(120))
SIZES = [1, 2, 9, 257, 4_097, 20_000, 70_000]
_SIZE_P = [0.04, 0.04, 0.06, 0.12, 0.2, 0.3, 0.24]
CAPS = [12, 100, 1_000]
WORLDS = [1, 2, 3, 5, 6, 7, 8]
SHARD_MODES = ["buckets", "octants"]
CUT_KINDS = ["even", "random", "one_rank", "empty_middle", "tile_edges"]
TILE = 4_096  # points per routing tile (pcv_route_plan)
TILE_EDGE_LENGTHS = [0, 1, 3, 4, 5, TILE - 1, TILE, TILE + 1, 2 * TILE + 1]
ENC_F32 = 3


def _random_cuts(rng, n, ranks):
    """ranks slice lengths summing to n, drawn as sorted random offsets (empty slices happen)."""
    inner = np.sort(rng.integers(0, n + 1, ranks - 1)) if ranks > 1 else np.zeros(0, dtype=np.int64)
    return np.diff(np.concatenate([[0], inner, [n]])).astype(np.int64)


def make_cuts(rng, cut_kind, n, world):
    if cut_kind == "even":
        return np.array([r * n // world for r in range(world + 1)], dtype=np.int64)
    if cut_kind == "random":
        sizes = _random_cuts(rng, n, world)
    elif cut_kind == "one_rank":
        sizes = np.zeros(world, dtype=np.int64)
        sizes[int(rng.integers(0, world))] = n
    elif cut_kind == "empty_middle":  # an empty rank strictly between two that hold points
        assert world >= 3 and n >= 2
        m = int(rng.integers(1, world - 1))
        before = int(rng.integers(1, n))
        sizes = np.concatenate([_random_cuts(rng, before, m), [0], _random_cuts(rng, n - before, world - 1 - m)])
    elif cut_kind == "tile_edges":  # slices that end on, one before and one after a routing tile and a group of four
        sizes, left = [], n
        for _ in range(world - 1):
            s = min(int(rng.choice(TILE_EDGE_LENGTHS)), left)
            sizes.append(s)
            left -= s
        sizes.append(left)
        sizes = np.array(sizes, dtype=np.int64)
    else:
        raise AssertionError(cut_kind)
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def _case(name, x, y, z, rgb, intensity, bmin, bmax, res, cap, world, shard_mode="buckets", compress=True, cuts=None, views=False,
          regime="", kind="", cut_kind="even"):
    n = int(x.size)
    if cuts is None:
        cuts = make_cuts(None, "even", n, world)
    cuts = np.asarray(cuts, dtype=np.int64)
    assert cuts.size == world + 1 and cuts[0] == 0 and cuts[-1] == n and np.all(np.diff(cuts) >= 0)
    return dict(name=name, x=np.ascontiguousarray(x, dtype=np.float64), y=np.ascontiguousarray(y, dtype=np.float64),
                z=np.ascontiguousarray(z, dtype=np.float64), rgb=np.ascontiguousarray(rgb, dtype=np.uint8),
                intensity=None if intensity is None else np.ascontiguousarray(intensity, dtype=np.float32),
                bmin=np.asarray(bmin, dtype=np.float64), bmax=np.asarray(bmax, dtype=np.float64), res=float(res), cap=int(cap),
                world=int(world), shard_mode=shard_mode, compress=bool(compress), cuts=cuts, views=bool(views), regime=regime,
                kind=kind, cut_kind=cut_kind)


@functools.lru_cache(maxsize=None)
def case(seed):
    rng = np.random.default_rng(13_000 + seed)
    regime = REGIMES[seed % len(REGIMES)]
    cut_kind = CUT_KINDS[(seed // len(REGIMES)) % len(CUT_KINDS)]  # every regime meets every kind of cut
    world = int(rng.choice([w for w in WORLDS if w >= 3] if cut_kind == "empty_middle" else WORLDS))
    n = int(rng.choice(SIZES, p=_SIZE_P))
    if cut_kind == "empty_middle":
        n = max(n, 2)
    kind, x, y, z, bmin, bmax, res = _draw(rng, regime, n)
    # every kind's oracle build is fast at every size here (the slowest, 23 000 nodes, takes 0.3 s); the largest size only keeps off
    # the smallest capacity, which would write tens of thousands of node files in the directory check
    cap = max(int(rng.choice(CAPS)), n // 700)
    shard_mode = SHARD_MODES[int(rng.integers(0, 2))]
    compress = bool(rng.random() < 0.7)
    rgb = rng.integers(0, 256, (n, 3), dtype=np.uint8)
    inten = rng.random(n).astype(np.float32) * 100.0 - 20.0 if rng.random() < 0.4 else None
    views = bool(rng.random() < 0.5)
    cuts = make_cuts(rng, cut_kind, n, world)
    return _case(f"seed{seed}", x, y, z, rgb, inten, bmin, bmax, res, cap, world, shard_mode, compress, cuts, views, regime, kind,
                 cut_kind)


# ---- named cases the draw cannot guarantee ---------------------------------------------------------------------------------------
def _colors(n, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, 3), dtype=np.uint8)


def _special(box, res, world):
    """NaN, infinities, denormals, huge values and points outside the box through route and (routed) build."""
    x, y, z, rgb, boxes = special_coordinates_cloud()
    lo, hi, _ = boxes[box]
    rng = np.random.default_rng(100 * box + world)
    return _case("", x, y, z, rgb, None, lo, hi, res, 900, world, SHARD_MODES[(box + world) % 2], True,
                 make_cuts(rng, "tile_edges" if world == 8 else "random", x.size, world), world == 3, kind="special",
                 cut_kind="tile_edges" if world == 8 else "random")


def _empty(world):
    e = np.zeros(0)
    return _case("", e, e, e, np.zeros((0, 3), np.uint8), None, [-1.0, 2.0, 3.0], [4.0, 5.0, 9.0], 0.01, 100, world, kind="empty")


def _few(n):
    rng = np.random.default_rng(n)
    pos = rng.choice([0.0, 2.0, 4.0, 6.0, 8.0, 3.9999999999999996, 4.000000000000001, 1.3], (n, 3))
    inten = rng.random(n).astype(np.float32)
    return _case("", pos[:, 0], pos[:, 1], pos[:, 2], _colors(n, n), inten, np.zeros(3), np.full(3, 8.0), 0.001, 2, 8, kind="few")


def _duplicates():
    """5 000 copies of one position + 2 000 uniform points at capacity 100: one bucket holds a resolution-limited node far above the
    capacity, which no plan can balance."""
    rng = np.random.default_rng(71)
    p = np.concatenate([np.tile([[13.25, 2.125, 7.0625]], (5_000, 1)), rng.random((2_000, 3)) * 16.0])
    p = p[rng.permutation(p.shape[0])]
    return _case("", p[:, 0], p[:, 1], p[:, 2], _colors(p.shape[0], 72), None, np.zeros(3), np.full(3, 16.0), 0.001, 100, 5,
                 cuts=make_cuts(rng, "random", p.shape[0], 5), views=True, kind="duplicates", cut_kind="random")


def _one_bucket():
    """Every point in level-2 bucket 0 of the box: at world 5 four ranks own nothing."""
    rng = np.random.default_rng(73)
    p = rng.random((3_000, 3)) * 0.999
    return _case("", p[:, 0], p[:, 1], p[:, 2], _colors(3_000, 74), rng.random(3_000).astype(np.float32), np.zeros(3), np.full(3, 8.0),
                 0.0001, 100, 5, kind="one_bucket")


def _centre_planes():
    """300 points on each of the three centre planes of the root and of the level-1 node of octant 0: `p > centre` is strict
    (node.rs:34-42), a point on the plane belongs to the lower octant."""
    rng = np.random.default_rng(75)
    parts = [rng.random((4_000, 3)) * 8.0]
    for axis in range(3):
        q = rng.random((300, 3)) * 8.0
        q[:, axis] = 4.0  # a centre plane of the root
        parts.append(q)
        q = rng.random((300, 3)) * 4.0
        q[:, axis] = 2.0  # a centre plane of r0
        parts.append(q)
    p = np.concatenate(parts)
    p = p[rng.permutation(p.shape[0])]
    return _case("", p[:, 0], p[:, 1], p[:, 2], _colors(p.shape[0], 76), None, np.zeros(3), np.full(3, 8.0), 0.001, 100, 6,
                 cuts=make_cuts(rng, "tile_edges", p.shape[0], 6), views=True, kind="centre_planes", cut_kind="tile_edges")


def _coarse(res):
    """A resolution of at least the root edge, or between half the edge and the edge, with octants far above the capacity. The root
    always has its level-1 children (the level table never reports a max_level below 1: generation.rs:137 stops a node whose own edge
    is within the resolution from splitting, and the root is split before that is asked); in both cubes level 1 exists and cannot
    split."""
    rng = np.random.default_rng(77)
    p = rng.random((3_000, 3)) * 8.0
    return _case("", p[:, 0], p[:, 1], p[:, 2], _colors(3_000, 78), rng.random(3_000).astype(np.float32), np.zeros(3), np.full(3, 8.0),
                 res, 100, 3, regime="octants", kind="coarse")


def _deep_tree():
    """test_virtual_ranks_deep_tree's cloud at 8 000 points: two piles of duplicates 4 mm apart in an 8 km cube at 1 mm, more than
    21 levels, i.e. keys of two words."""
    rng = np.random.default_rng(23)
    x = np.concatenate([rng.uniform(0, 8192, 5_000), np.full(1_600, 5000.5), np.full(1_400, 5000.5 + 0.004)])
    y = np.concatenate([rng.uniform(0, 8192, 5_000), np.full(1_600, 123.0), np.full(1_400, 123.0)])
    z = np.concatenate([rng.uniform(0, 8192, 5_000), np.full(1_600, 8000.25), np.full(1_400, 8000.25)])
    perm = rng.permutation(x.size)
    return _case("", x[perm], y[perm], z[perm], _colors(x.size, 79), None, np.zeros(3), np.full(3, 8192.0), 0.001, 1_000, 3,
                 kind="deep_tree")


def _tiles_on_8_ranks():
    """70 000 points, more than two routing tiles on every one of 8 ranks, none of the slices ending on a tile or a group of four:
    the two-pass compressed route (Float32-coded level 1) with intensity, from views of one tensor."""
    rng = np.random.default_rng(81)
    n = 70_000
    p = 1.0e3 + rng.random((n, 3)) * 256.0
    sizes = np.array([8_193, 8_195, 8_197, 8_201, 8_999, 9_001, 9_003, 0])
    sizes[-1] = n - sizes.sum()
    return _case("", p[:, 0], p[:, 1], p[:, 2], _colors(n, 82), rng.random(n).astype(np.float32), np.full(3, 1.0e3),
                 np.full(3, 1.0e3 + 256.0), 256.0 / 2.0 ** 21, 1_000, 8, cuts=np.concatenate([[0], np.cumsum(sizes)]), views=True,
                 regime="f32", kind="uniform", cut_kind="tile_edges")


_BUILDERS = {}
for _box in (1, 2):
    for _res in (1e-3, 1e-5, 1e-7):
        for _world in (3, 8):
            _BUILDERS[f"special_box{_box}_res{_res:g}_world{_world}"] = functools.partial(_special, _box, _res, _world)
_BUILDERS.update({
    "empty_world1": functools.partial(_empty, 1), "empty_world3": functools.partial(_empty, 3),
    "one_point_world8": functools.partial(_few, 1), "nine_points_world8": functools.partial(_few, 9),
    "duplicates_over_capacity": _duplicates, "one_bucket_world5": _one_bucket, "centre_planes": _centre_planes,
    "resolution_root_edge": functools.partial(_coarse, 8.0), "resolution_half_edge": functools.partial(_coarse, 5.0),
    "deep_tree": _deep_tree, "tiles_on_8_ranks": _tiles_on_8_ranks,
})
CONSTRUCTED = list(_BUILDERS)


@functools.lru_cache(maxsize=None)
def constructed(name):
    c = _BUILDERS[name]()
    c["name"] = name
    return c


def all_cases():
    """Every case id, in the order the fuzz runs them (seed order, then the named ones)."""
    return list(SEEDS) + list(CONSTRUCTED)


def get(case_id):
    return case(case_id) if isinstance(case_id, int) else constructed(case_id)


# ---- what the oracle says about a case (no sharded code but the pure plan) ---------------------------------------------------------
@functools.lru_cache(maxsize=None)
def facts(case_id):
    """max_level, level-1 encoding (0 when there is no level 1), can_split, the 64 bucket counts, the plan of those counts, whether
    the exchange is compressed, the ranks with and without input, and the points on the centre planes of levels 1 and 2."""
    import oracle_lib as O
    import point_cloud_viewer_amd as pcv
    from point_cloud_viewer_amd.distributed import plan_buckets
    c = get(case_id)
    ml, edges, enc = pcv.level_table(c["bmin"], c["bmax"], c["res"])
    can_split = bool(ml >= 2 and edges[1] > c["res"])
    n = c["x"].size
    keys = O.chain_keys64(c["bmin"], c["bmax"], c["res"], 2, c["x"], c["y"], c["z"]) if n else np.zeros(0, dtype=np.uint64)
    d1 = (keys >> np.uint64(60)).astype(np.int64) & 7
    bucket = ((keys >> np.uint64(57)).astype(np.int64) & 63) if ml >= 2 else d1 << 3
    counts = np.bincount(bucket, minlength=64)
    rank_of, split_mask = plan_buckets(counts, c["world"], c["cap"], can_split, c["shard_mode"])
    owned = np.bincount(rank_of, weights=counts, minlength=c["world"]).astype(np.int64)
    # points exactly on a plane that decides a level-1 digit (the root's centre) or a level-2 digit (a level-1 node's centre)
    on_plane = np.zeros(n, dtype=bool)
    if n and ml >= 1:
        coords = (c["x"], c["y"], c["z"])
        edge = float(edges[0])
        for axis in range(3):
            on_plane |= coords[axis] == c["bmin"][axis] + edge / 2.0
        if ml >= 2:
            for digit in np.unique(d1):
                lo, e1 = O.find_bounding_cube(1 << 56, int(digit), c["bmin"], edge)
                inside = d1 == digit
                for axis in range(3):
                    on_plane |= inside & (coords[axis] == lo[axis] + e1 / 2.0)
    lengths = np.diff(c["cuts"])
    return dict(max_level=int(ml), enc1=int(enc[1]) if ml >= 1 else 0, can_split=can_split, counts=counts, rank_of=rank_of,
                split_mask=int(split_mask), owned=owned, octant_max=int(counts.reshape(8, 8).sum(axis=1).max()),
                compressed=bool(c["compress"] and ml >= 1 and int(enc[1]) == ENC_F32),
                ranks_with_input=int(np.count_nonzero(lengths)), ranks_without_input=int(np.count_nonzero(lengths == 0)),
                on_planes=int(np.count_nonzero(on_plane)))


# Lower bounds of the branch tally of the device fuzz (tests/test_gpu_sharded_fuzz.py), proven from the oracle by
# tests/test_sharded_cases_cpu.py: cases whose exchange is compressed and ranks of those cases with / without input, cases that ship
# raw coordinates, cases whose global plan splits a level-1 node. Conditions, not measurements.
MIN_COMPRESSED_CASES, MIN_TWO_PASS_RANKS, MIN_ONE_PASS_RANKS, MIN_RAW_CASES, MIN_SPLIT_CASES = 10, 30, 5, 40, 30


def tally_expected(case_ids):
    """The branch tally the oracle predicts for the cases: what the device fuzz must have counted at its end."""
    t = dict(cases=0, two_pass_ranks=0, one_pass_ranks=0, compressed_cases=0, raw_cases=0, split_cases=0)
    for cid in case_ids:
        f = facts(cid)
        t["cases"] += 1
        t["compressed_cases"] += f["compressed"]
        t["raw_cases"] += not f["compressed"]
        t["two_pass_ranks"] += f["ranks_with_input"] if f["compressed"] else 0
        t["one_pass_ranks"] += f["ranks_without_input"] if f["compressed"] else 0
        t["split_cases"] += f["split_mask"] != 0
    return t


# ---- what both legs of the fuzz do with a case -----------------------------------------------------------------------------------
def oracle_tree(case_id):
    """The truth of a case: ONE oracle build of the whole cloud (generation.rs:289-403 has one answer per input)."""
    import oracle_lib as O
    c = get(case_id)
    with O.max_points_per_node(c["cap"]):
        return O.build_closed(c["res"], c["bmin"], c["bmax"], c["x"], c["y"], c["z"], c["rgb"], c["intensity"], threads=4)


def whole_tensors(c, device):
    """The whole cloud as one tensor per plane on `device`."""
    import torch
    names = ("x", "y", "z", "rgb") + (("intensity",) if c["intensity"] is not None else ())
    return {k: torch.from_numpy(c[k]).to(device) for k in names}


def rank_input(c, whole, rank):
    """(x, y, z, rgb, intensity or None) of a rank: views of the whole cloud's tensors, or contiguous copies of its slice."""
    a, b = int(c["cuts"][rank]), int(c["cuts"][rank + 1])
    cut = (lambda t: t[a:b]) if c["views"] else (lambda t: t[a:b].clone())
    return tuple(cut(whole[k]) for k in ("x", "y", "z", "rgb")) + ((cut(whole["intensity"]),) if "intensity" in whole else (None,))


def assert_same_tree(merged, want, c):
    """Same node set; num_points, encoding, xyz, rgb and intensity byte for byte."""
    assert set(merged) == set(want.nodes), (c["name"], sorted(set(merged) ^ set(want.nodes))[:10])
    for name, nd in want.nodes.items():
        for f in ("num_points", "encoding", "xyz", "rgb", "intensity"):
            assert merged[name][f] == nd[f], (c["name"], name, f)


def assert_exchange(c, f, results):
    """exchange_info() of every rank: the points owned sum to n, row i of the send matrix sums to rank i's slice length, and a row
    of the exchange takes 16 (+ 4 with intensity) bytes exactly when compression is on and level 1 is Float32 coded, 27 (+ 4)
    otherwise."""
    n, lengths = int(c["x"].size), np.diff(c["cuts"])
    extra = 4 if c["intensity"] is not None else 0
    for rank, (ex, matrix) in enumerate(results):
        assert ex["ranks"] == c["world"] and ex["shard_mode"] == c["shard_mode"], (c["name"], rank, ex)
        assert sum(ex["points_owned_per_rank"]) == n, (c["name"], rank, ex)
        assert np.array_equal(np.asarray(matrix).sum(axis=1), lengths), (c["name"], rank, matrix)
        assert ex["bytes_per_row"] == (16 if f["compressed"] else 27) + extra, (c["name"], rank, ex)
        assert ex["points_owned_per_rank"] == [int(v) for v in f["owned"]], (c["name"], rank, ex)


def assert_same_directory(got_dir, c):
    """A directory written by all ranks against the oracle's literal build of the whole cloud, written next to it: the same octree
    (meta.pb and every node file, byte for byte) and the same set of files."""
    import os
    import oracle_lib as O
    want_dir = str(got_dir) + "_oracle"
    with O.max_points_per_node(c["cap"]):
        O.build_literal_dir(want_dir, c["res"], c["bmin"], c["bmax"], c["x"], c["y"], c["z"], c["rgb"], c["intensity"], threads=4)
    diffs = O.compare_octrees(O.load_dir(got_dir), O.load_dir(want_dir))
    assert not diffs, (c["name"], diffs[:10])
    assert sorted(os.listdir(got_dir)) == sorted(os.listdir(want_dir)), c["name"]
