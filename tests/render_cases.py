"""Inputs of the rendered-frame fuzz (test_render_fuzz_cpu.py states on the CPU what they reach, test_gpu_render_fuzz.py
submits them to the device): views of visible_cases' trees A and B at plane sizes that are no multiple of a wave, leaves of an
exact point count per encoding whose colours carry the point's index, small trees with ragged multi-chunk inner nodes, and
points planted on the f32 edges of DESIGN §9b's coverage and clip rules.

The reference always splits the root (generation.rs:312-323) and hands every 8th point of a child to its parent, in input
order. A cloud whose points all lie in octant 0 of its bounding cube therefore builds two nodes: 'r' with the points
0, 8, 16, .. and the leaf 'r0' with the others. That leaf is the "single leaf" of the chunk-seam cases."""

import numpy as np

import oracle_lib as O
import render_oracle as R
import visible_cases as VC

F32 = np.float32
FLT_MAX = float(np.finfo(np.float32).max)
RESOLUTION = 0.001
PER = {1: 2048, 2: 1024, 3: 512, 4: 256}  # points per chunk: 6 KiB at 3 / 6 / 12 / 24 bytes per point
# edge of the leaf cube at 1 mm: floor(log2(edge / resolution)) + 1 bits = 7, 15, 22 and 26 (codec.rs:31-40), the cube
# sizes at which test_query_points_all_four_encodings' city-scale tree changes its encoding on the way down; the root
# cube (twice the edge) has the same encoding
LEAF_EDGE = {1: 0.125, 2: 32.0, 3: 4096.0, 4: 65536.0}
ODD_SIZES = [(1, 1), (3, 5), (7, 9), (33, 17), (65, 63), (1, 130), (130, 1)]
WG_THREADS, WG_WAVES, CU_WAVE_SLOTS = 256, 4, 32


def resident_workgroups(cus):
    """No resident grid of 256-thread workgroups exceeds this: 4 waves each, 32 wave slots per CU."""
    return (CU_WAVE_SLOTS // WG_WAVES) * cus


def pixel_threshold(cus):
    """More pixels than this in one group send render_resolve round its loop again."""
    return resident_workgroups(cus) * WG_THREADS


def chunk_threshold(cus):
    """More chunks than this in one group send render_splat round its loop again."""
    return resident_workgroups(cus) * WG_WAVES


_trees = {}


def tree(key):
    """dict(oracle, tn) of visible_cases' tree `key`, built once per process."""
    if key not in _trees:
        oracle = VC.oracle_tree(key)
        _trees[key] = dict(oracle=oracle, tn=R.TreeNodes(oracle, VC.BMIN, VC.BMAX), bmin=VC.BMIN, bmax=VC.BMAX)
    return _trees[key]


def gpu_tree(ctx, key):
    import point_cloud_viewer_amd as pcv
    x, y, z, rgb = VC.cloud(key)
    return ctx.build(VC.RESOLUTION, pcv.Aabb(VC.BMIN, VC.BMAX), x, y, z, rgb, max_points_per_node=VC.MAX_POINTS_PER_NODE)


def oracle_scene(cloud):
    """dict(cloud, oracle, tn): the oracle's tree of a cloud dict(x, y, z, rgb, bmin, bmax, cap)."""
    with O.max_points_per_node(cloud["cap"]):
        oracle = O.build_closed(RESOLUTION, cloud["bmin"], cloud["bmax"], cloud["x"], cloud["y"], cloud["z"], cloud["rgb"], threads=4)
    return dict(cloud, oracle=oracle, tn=R.TreeNodes(oracle, cloud["bmin"], cloud["bmax"]))


def gpu_scene(ctx, cloud):
    """oracle_scene plus the device's tree of the same cloud."""
    import point_cloud_viewer_amd as pcv
    s = oracle_scene(cloud)
    s["tree"] = ctx.build(RESOLUTION, pcv.Aabb(cloud["bmin"], cloud["bmax"]), cloud["x"], cloud["y"], cloud["z"], cloud["rgb"],
                          max_points_per_node=cloud["cap"])
    assert sorted(s["tree"].node_names()) == sorted(s["oracle"].nodes)
    return s


def positions(tn, name):
    """The shader's f64 positions of a node, from the node's own bytes (never from the input)."""
    nd = tn.node(name)
    return R.attribute(nd["encoding"], nd["xyz"]) * float(nd["cube_edge"]) + np.asarray(nd["cube_min"], np.float64)[None, :]


def drawn_chunks(tn, names):
    """Chunks of a draw list: the sum over its nodes of ceil(n / per)."""
    return sum(-(-tn.node(k)["num_points"] // PER[tn.node(k)["encoding"]]) for k in names)


# ---- (a) odd planes and view seams -------------------------------------------------------------------------------------------

def seam_views():
    """5 views of tree A: two ortho scales, two cameras, and a singular matrix in the middle of the batch."""
    return [VC.ortho(0.9), VC.look((20.0, 20.0, 72.0)), np.zeros(16), VC.look((44.0, 36.0, 81.0), aspect=1.7777), VC.ortho(0.5)]


# ---- (b) second trip of the stride loops -------------------------------------------------------------------------------------

RESOLVE_SIZE = (523, 401)


def resolve_stride_views(cus):
    """V views of tree A whose 523 x 401 planes together exceed what one resident grid of render_resolve takes in one trip."""
    w, h = RESOLVE_SIZE
    v = -(-pixel_threshold(cus) // (w * h)) + 1
    pool = [VC.ortho(0.9), VC.look((20.0, 20.0, 72.0)), VC.ortho(0.5), VC.look((44.0, 36.0, 81.0), aspect=1.7777)]
    return [pool[k % 4] if k < 4 else VC.ortho(0.9 - 0.01 * k) for k in range(v)]


def splat_stride_views(cus, chunks_per_view):
    """Orthographic views of tree B, a slightly different scale each, whose chunks exceed twice one trip of render_splat."""
    v = -(-2 * chunk_threshold(cus) // chunks_per_view)
    return [VC.ortho(0.9 - 0.01 * k) for k in range(v)]


# ---- (c) chunk seams ---------------------------------------------------------------------------------------------------------

LEAF_W = LEAF_H = 16
LEAF_LAYERS = 32


def leaf_counts(enc):
    per = PER[enc]
    return [per - 1, per, per + 1, 2 * per + 63, 2 * per + 64, 2 * per + 65]


def rank_colours(k):
    k = np.asarray(k, np.int64)
    return np.stack([k & 255, (k >> 8) & 255, (k >> 16) | 1], axis=1).astype(np.uint8)


def colour_rank(rgb):
    """The index a rank colour carries; (..., 3) u8 -> int64."""
    c = np.asarray(rgb).astype(np.int64)
    return c[..., 0] | (c[..., 1] << 8) | ((c[..., 2] >> 1) << 16)


def leaf_cloud(enc, n):
    """A cloud whose leaf 'r0' holds exactly n points of encoding `enc`: N points with N - ceil(N / 8) == n in octant 0 of a
    cube of twice the leaf's edge. Point k has the colour of k, sits on the centre of pixel k % 256 of a 16 x 16 image under
    leaf_views (image rows top to bottom), and lies deeper the smaller k is."""
    total = n
    while total - -(-total // 8) < n:
        total += 1
    assert total - -(-total // 8) == n and -(-total // (LEAF_W * LEAF_H)) <= LEAF_LAYERS
    edge = LEAF_EDGE[enc]
    lo = np.array([3.0, -2.0, 1.0]) * (2 * edge)  # exact in every encoding's arithmetic
    k = np.arange(total)
    pix, layer = k % (LEAF_W * LEAF_H), k // (LEAF_W * LEAF_H)
    col, row = pix % LEAF_W, pix // LEAF_W
    x = lo[0] + edge * ((col + 0.5) / LEAF_W)
    y = lo[1] + edge * ((LEAF_H - 1 - row + 0.5) / LEAF_H)
    z = lo[2] + edge * (1.0 - (layer + 0.5) / LEAF_LAYERS)
    return dict(x=x, y=y, z=z, rgb=rank_colours(k), bmin=lo, bmax=lo + 2 * edge, cap=total + 1, leaf_lo=lo, leaf_hi=lo + edge,
                total=total)


def leaf_views(cloud):
    """Real depth (it decreases with k: the highest ranks win) and depth flattened (rank alone decides: the lowest win)."""
    return [VC.ortho(1.0, 1.0, cloud["leaf_lo"], cloud["leaf_hi"]), VC.ortho(1.0, 1e-30, cloud["leaf_lo"], cloud["leaf_hi"])]


def drawn_ranks(tn, drawn):
    """The index carried by every drawn point's colour, in draw order."""
    return np.concatenate([colour_rank(np.frombuffer(tn.node(k)["rgb"], np.uint8).reshape(-1, 3)) for k in drawn])


def multi_cloud(enc):
    """A uniform cloud of 18 chunks under a cap of 3 in a cube of the encoding's leaf edge: the root keeps an eighth of it
    (about 2.25 chunks), each of the eight leaves below about 1.97 chunks."""
    per = PER[enc]
    cap = 3 * per
    rng = np.random.default_rng(50 + enc)
    edge = LEAF_EDGE[enc]
    lo = np.array([3.0, -2.0, 1.0]) * edge
    p = lo + rng.uniform(0.0, edge, (18 * per, 3))
    rgb = rng.integers(1, 256, (18 * per, 3), dtype=np.uint8)
    return dict(x=p[:, 0].copy(), y=p[:, 1].copy(), z=p[:, 2].copy(), rgb=rgb, bmin=lo, bmax=lo + edge, cap=cap)


def multi_view(cloud):
    return VC.ortho(0.9, 1.0, cloud["bmin"], cloud["bmax"])


def multi_cut(tn, enc, matrix):
    """(i, max_nodes): the first node of the visible list that is neither its first nor, under max_nodes, its last entry, has
    encoding `enc`, several chunks and a ragged last one; max_nodes cuts the list two entries after it."""
    names = tn.visible(matrix)
    per = PER[enc]
    for i, name in enumerate(names):
        nd = tn.node(name)
        if i > 0 and nd["encoding"] == enc and nd["num_points"] > per and nd["num_points"] % per != 0:
            return i, i + 3
    raise AssertionError(f"no ragged multi-chunk node of encoding {enc}")


# ---- (d) f32 edges of the splat ----------------------------------------------------------------------------------------------

PLANT_EDGE = 65536.0  # Float64 nodes 'r' (edge 131072) and 'r0': positions decode to the input exactly
PLANT_BOX = 64.0      # the views look at [0, 64]^3
# places along the tested axis, in units of the box: window coordinate t * extent / 64
PLANT_T = [0.0, 1.0 / 512, 1.0 / 256, 0.5, 1.0, 5.0, 5.5, 31.5, 32.0, 63.0, 63.5, 64.0 - 1.0 / 256, 64.0 - 1.0 / 512, 64.0]


def planted_cloud():
    """Point k = axis * 14 + j varies along `axis` (0: x, 1: y) over PLANT_T, sits at 32 on the other axis and alone in the
    slab z = 2 k + 1."""
    pts = []
    for axis in range(2):
        for j, t in enumerate(PLANT_T):
            k = axis * len(PLANT_T) + j
            pts.append([t, 32.0, 2.0 * k + 1.0] if axis == 0 else [32.0, t, 2.0 * k + 1.0])
    pts = np.array(pts)
    return dict(x=pts[:, 0].copy(), y=pts[:, 1].copy(), z=pts[:, 2].copy(), rgb=rank_colours(np.arange(len(pts)) + 1000),
                bmin=np.zeros(3), bmax=np.full(3, 2 * PLANT_EDGE), cap=1000, pts=pts)


def slab_view(zk):
    """Orthographic, w = 1: x and y of [0, 64] onto the whole clip square (a power of two: exact), z - zk as clip z, so that of
    points 2 apart in z only the one at zk passes the depth planes."""
    m = np.zeros((4, 4))
    m[0, 0] = m[1, 1] = 2.0 / PLANT_BOX
    m[0, 3] = m[1, 3] = -1.0
    m[2, 2], m[2, 3] = 1.0, -float(zk)
    m[3, 3] = 1.0
    return m.ravel(order="F")


def planted_views(axis):
    n = len(PLANT_T)
    return [slab_view(2.0 * (axis * n + j) + 1.0) for j in range(n)]


# (W, H, point_size) per axis: the 64-wide image at the sizes whose half is whole and half-whole, and the extent limit
PLANT_CASES = {0: [(64, 3, 1.0), (64, 3, 2.0), (64, 3, 3.0), (64, 3, 64.0), (16384, 1, 64.0)],
               1: [(3, 64, 1.0), (3, 64, 2.0), (3, 64, 3.0), (3, 64, 64.0), (1, 16384, 64.0)]}


def exact_run(t, extent, point_size):
    """Pixels i of [0, extent) with xw - h <= i + 0.5 < xw + h for xw = t * extent / 64, in exact arithmetic (every value is a
    small dyadic rational: Python floats do not round here)."""
    xw, h = t * extent / PLANT_BOX, point_size / 2.0
    return [i for i in range(extent) if xw - h <= i + 0.5 < xw + h]


def brute_force_coverage(xw, yw, point_size, W, H):
    """The predicate of step 5 on every pixel of the image, f32, one numpy operation per step: (H, W) bool, row 0 the top."""
    h = F32(0.5) * F32(point_size)
    ci = np.arange(W).astype(F32) + F32(0.5)
    cj = np.arange(H).astype(F32) + F32(0.5)
    cov = np.zeros((H, W), bool)
    for a, b in zip(np.asarray(xw, F32), np.asarray(yw, F32)):
        okx = ((a - h) <= ci) & (ci < (a + h))
        oky = ((b - h) <= cj) & (cj < (b + h))
        cov |= oky[::-1, None] & okx[None, :]
    return cov


def window(matrix, p, W, H):
    """Steps 3 and 4 for the drawn points of p: (draw mask, xw, yw, zw), f32."""
    x, y, z, w = R.clip_f32(matrix, p)
    with np.errstate(invalid="ignore"):
        draw = (w > F32(0)) & (w < F32(np.inf)) & (-w <= x) & (x <= w) & (-w <= y) & (y <= w) & (-w <= z) & (z <= w)
    x, y, z, w = x[draw], y[draw], z[draw], w[draw]
    xw = (x / w + F32(1.0)) * (F32(0.5) * F32(W))
    yw = (y / w + F32(1.0)) * (F32(0.5) * F32(H))
    zw = (z / w) * F32(0.5) + F32(0.5)
    return draw, xw, yw, zw


W_LIMIT = 2.0 ** 128 - 2.0 ** 103  # the smallest f64 that rounds to +inf in f32 (a tie, to even); one f64 step is 2^75
W_STEP = 2.0 ** 75


def fltmax_cloud():
    pts = np.array([[10.0, 20.0, 0.0], [30.0, 40.0, 1.0], [50.0, 10.0, 2.0], [20.0, 50.0, 3.0]])
    return dict(x=pts[:, 0].copy(), y=pts[:, 1].copy(), z=pts[:, 2].copy(), rgb=rank_colours(np.arange(4) + 7),
                bmin=np.zeros(3), bmax=np.full(3, 2 * PLANT_EDGE), cap=1000, pts=pts)


def fltmax_views():
    """w = 2^75 z + b: the first view has w one f64 step below W_LIMIT at z == 1 (FLT_MAX after rounding) and W_LIMIT itself at
    z == 2 (+inf); the second is the first moved one step, which takes the point at z == 1 to +inf too."""
    out = []
    for b in (W_LIMIT - 2 * W_STEP, W_LIMIT - W_STEP):
        m = np.zeros((4, 4))
        m[0, 0] = m[1, 1] = 1.0
        m[2, 2] = W_STEP
        m[3, 2], m[3, 3] = W_STEP, b
        out.append(m.ravel(order="F"))
    return out


# ---- (e) seeded random views -------------------------------------------------------------------------------------------------

# About 45 % of random_cases' views put a point of tree A on the screen; 1753 is the first seed of a CPU scan of 761 .. 2400
# with at least 44 such views of 64 (test_render_fuzz_cpu.py counts them: 45, and one view on which the reference panics)
RANDOM_SEED = 1753
RANDOM_POINT_SIZES = (1.0, 1.5, 2.5, 4.0)


def random_plan(seed=RANDOM_SEED):
    """[(matrices, (W, H), point_size)]: the 64 views of VC.random_cases(seed) in four calls of 16, a size of ODD_SIZES and a
    point size drawn per call, and a fifth call that draws four of them again at point_size 64 (on 3 x 5, 7 x 9 or 33 x 17)."""
    mats = [m for _, m in VC.random_cases(seed)]
    rng = np.random.default_rng(seed)
    plan = []
    for b in range(4):
        size = ODD_SIZES[int(rng.integers(1, len(ODD_SIZES)))]
        plan.append((mats[16 * b:16 * b + 16], size, float(rng.choice(RANDOM_POINT_SIZES))))
    # at point size 64 the oracle's cost is 20 000 points times the pixels they cover: one of the three smallest planes
    plan.append(([mats[k] for k in (3, 18, 33, 48)], ODD_SIZES[int(rng.integers(1, 4))], 64.0))
    return plan
