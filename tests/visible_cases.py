"""The trees and frusta of the get_visible_nodes pop-order tests (test_visible_cpu.py states what they reach,
test_gpu_visible_fuzz.py submits them to the device): two clipped cluster clouds in the cube [0, 64]^3, whose node cubes are
powers of two, fixed views found on the CPU with tests/visible_mirror.py, and a seeded generator of random ones."""
import math

import numpy as np

import oracle_lib as O
from point_cloud_viewer_amd import synthetic

BMIN, BMAX = np.zeros(3), np.full(3, 64.0)
MAX_POINTS_PER_NODE = 40
RESOLUTION = 0.001
POINTS = {"A": 20_000, "B": 60_000}   # 2 191 and 5 766 nodes
NODES = {"A": 2191, "B": 5766}
IDENTITY = [0.0, 0.0, 0.0, 1.0]


def cloud(key):
    x, y, z, rgb, _, _ = synthetic.gaussian_clusters(POINTS[key], seed=12, num_clusters=5, extent=64, sigma_range=(0.3, 5.0))
    return np.clip(x, 0.0, 64.0), np.clip(y, 0.0, 64.0), np.clip(z, 0.0, 64.0), rgb


def oracle_tree(key):
    x, y, z, rgb = cloud(key)
    with O.max_points_per_node(MAX_POINTS_PER_NODE):
        tree = O.build_closed(RESOLUTION, BMIN, BMAX, x, y, z, rgb, threads=4)
    assert len(tree.nodes) == NODES[key]
    return tree


def ortho(scale=0.9, depth_scale=1.0, lo=BMIN, hi=BMAX):
    """test_gpu_render.ortho with the scale as a parameter: the box onto `scale` of the clip cube, w = 1, column-major."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    c, e = (lo + hi) / 2, (hi - lo) / 2
    m = np.zeros((4, 4))
    for a in range(3):
        s = scale / e[a] * (depth_scale if a == 2 else 1.0)
        m[a, a], m[a, 3] = s, -s * c[a]
    m[3, 3] = 1.0
    return m.ravel(order="F")


def look(eye, quat=IDENTITY, aspect=1.0, fovy=1.2, near=0.1, far=1000.0):
    """clip_from_query of a camera at `eye`; the identity rotation looks along -z. Defaults: BASELINE config 4 with far = 1000."""
    return O.frustum_new([float(v) for v in eye], [float(v) for v in quat], O.perspective3_new(aspect, fovy, near, far))[0]


def rank3():
    m = np.eye(4)
    m[2] = 0.0
    return m.ravel(order="F")


# Nodes of tree A at level 3 and 4. An eye over such a node's centre AT its cube's max z, looking along -z, puts the top
# corners of that cube (and of its neighbours at that height) at w == 0 exactly: the reference panics when the traversal
# reaches them, after some pops. Eyes = (min + edge / 2, min + edge / 2, min + edge) of the get_child recurrence.
PANIC_NODES = {"r024": (12.0, 20.0, 8.0), "r072": (20.0, 28.0, 24.0), "r0172": (10.0, 14.0, 28.0)}

# eye heights over (20, 20) found by a scan of z = 33 .. 80 in steps of 0.5 with the mirror: the longest heap of the
# traversal is 256, 255, 257, 252 and 259 entries: all in LDS, one slot short of full, one / three entries in global memory
BOUNDARY_Z = (33.0, 33.5, 34.0, 40.0, 41.5)


def fixed_cases(key):
    """[(tag, matrix)]: the views whose reach test_visible_cpu.py asserts."""
    cases = [("ortho 0.9: every node In, every level one size", ortho()),
             ("ortho 4: every node fills the screen, size 4", ortho(4.0)),
             ("ortho 0.25", ortho(0.25)),
             ("ortho, depth flattened", ortho(0.9, 1e-30)),
             ("ortho, depth scale 0: singular", ortho(0.9, 0.0)),
             ("zeros: singular", np.zeros(16)),
             ("rank 3: singular", rank3()),
             ("from above, z = 72", look((20.0, 20.0, 72.0))),
             ("w == 0 on every child of the root", look((20.0, 20.0, 32.0)))]
    if key == "A":
        cases += [(f"heap at the LDS boundary, z = {z}", look((20.0, 20.0, z))) for z in BOUNDARY_Z]
        cases += [(f"w == 0 at the top of {name}", look(eye)) for name, eye in PANIC_NODES.items()]
    return cases


def _plane(rng):
    """A coordinate on a node cube plane of a random level, sometimes an ulp beside it (as in test_gpu_query_fuzz.py)."""
    level = int(rng.integers(0, 9))
    v = float(rng.integers(0, 2 ** level + 1)) * (64.0 / 2 ** level)
    step = int(rng.integers(-1, 2))
    return float(np.nextafter(v, math.inf if step > 0 else -math.inf)) if step else v


def random_cases(seed, n=64):
    """[(tag, matrix)]: perspectives of every fovy / aspect / depth range from eyes inside the cloud, outside it, on node cube
    planes and one ulp beside them, with the identity and with random rotations; orthographic views of random sub-boxes."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        if i % 8 == 7:
            lo = rng.uniform(-8.0, 40.0, 3)
            hi = lo + rng.uniform(4.0, 64.0, 3)
            scale, depth = float(rng.choice([0.25, 0.9, 4.0])), float(rng.choice([1.0, 1.0, 1e-30]))
            out.append((f"seed {seed} #{i}: ortho {scale} depth {depth}", ortho(scale, depth, lo, hi)))
            continue
        where = i % 4
        if where == 0:
            eye = rng.uniform(0.0, 64.0, 3)
        elif where == 1:
            eye = rng.uniform(-40.0, 104.0, 3)
        else:
            eye = np.array([_plane(rng) for _ in range(3)])
        if rng.random() < 0.4:
            q = np.array(IDENTITY)
        else:
            q = rng.normal(size=4)
            q = q / math.sqrt(float(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]))
        fovy, aspect = float(rng.uniform(0.05, 2.8)), float(rng.choice([0.5, 1.0, 1.7777]))
        near, far = float(10.0 ** rng.uniform(-3.0, 1.0)), float(10.0 ** rng.uniform(1.0, 4.0))
        out.append((f"seed {seed} #{i}: eye {eye.tolist()} quat {q.tolist()} fovy {fovy} aspect {aspect} near {near} far {far}",
                    look(eye, q, aspect, fovy, near, far)))
    return out


SEEDS = (701, 702, 703)


def all_cases(key):
    """About 200 views of tree `key`: the fixed ones, then three seeds of random ones."""
    cases = list(fixed_cases(key))
    for seed in SEEDS:
        cases += random_cases(seed + (0 if key == "A" else 10))
    return cases


def oracle_lists(nodes, matrices):
    """O.get_visible_nodes per matrix, eight calls at a time (ctypes releases the GIL)."""
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(8) as pool:
        return list(pool.map(lambda m: O.get_visible_nodes(BMIN, BMAX, nodes, m), matrices))


_expected = {}


def expected(key):
    """Computed once per process: dict(oracle=the oracle's tree, cases=all_cases(key), want=the oracle's list per case (None
    where the reference panics), mirror=visible_mirror.traverse's Result per case)."""
    import visible_mirror as VM
    if key not in _expected:
        tree, cases = oracle_tree(key), all_cases(key)
        _expected[key] = dict(oracle=tree, cases=cases, want=oracle_lists(tree.nodes, [m for _, m in cases]),
                              mirror=[VM.traverse(BMIN, BMAX, tree.nodes, m) for _, m in cases])
    return _expected[key]
