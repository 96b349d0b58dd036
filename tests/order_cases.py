"""Input ORDERS and constructed clouds for the octree builds (tests/test_order_cases_cpu.py, tests/test_gpu_order_fuzz.py).

The reference's inputs come from scanners and SLAM pipelines: spatially coherent, not shuffled. The single-chain build reads
the input order in several places — the sample (8 consecutive points every 8 x stride positions, csrc/pcv_single_chain.hip
plan_sample / sample_round), the chain pass's deal of a 1 024-point tile over its depth classes, one pool reservation per wave
on the region of the tile's slice, the rank-count rows and the record sort's passes, the every-8th promotion inside a leaf —
and the oracle is stable, so it gives the truth for every order. No GPU in here: plain numpy plus the library's host hooks."""
import ctypes as C

import numpy as np

import oracle_lib as O
import point_cloud_viewer_amd as pcv
from point_cloud_viewer_amd import synthetic


# ---- the library's host hooks ----------------------------------------------------------------------------------------
def sample_plan(n, cap):
    """(stride, delta) of a forced single-chain build of n points at capacity cap: pcv_spec_sample_plan, the rule
    plan_sample (csrc/pcv_single_chain.hip) itself calls. The device reads input positions i with i % (8 * stride) < 8."""
    f = pcv.load_library().pcv_spec_sample_plan
    f.restype = None
    f.argtypes = [C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p]
    stride, delta = C.c_uint32(0), C.c_double(0.0)
    f(n, cap, C.byref(stride), C.byref(delta))
    return stride.value, delta.value


def sampled_positions(n, stride):
    """Input positions of the device's sample, in sample order (chain_keys_kernel, csrc/pcv_chain.hip: sample i reads
    ((i >> 3) * stride << 3) + (i & 7); n // stride of them)."""
    i = np.arange(n // stride, dtype=np.int64)
    return i if stride == 1 else (((i >> 3) * stride) << 3) + (i & 7)


def lower_threshold(cap, delta):
    """A sample node is opened iff count * stride > cap * (1 - delta) (pcv_spec_sample_threshold, csrc/pcv_spec.cpp)."""
    return cap * (1.0 - delta)


PCV_SPEC_OK, PCV_SPEC_TOO_SHALLOW = 0, 1


def _selftest(name, keys, stride, cap, delta, resolution, edges, nlevels):
    f = getattr(pcv.load_library(), name)
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_double, C.c_double, C.c_void_p, C.c_int, C.c_uint32,
                  C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    capn = 1 << 18
    prefix, level = np.zeros(capn, dtype=np.uint64), np.zeros(capn, dtype=np.uint8)
    count, opn = np.zeros(capn, dtype=np.uint64), np.zeros(capn, dtype=np.uint8)
    num, stats = C.c_uint64(0), np.zeros(4, dtype=np.uint64)
    e = np.ascontiguousarray(edges, dtype=np.float64)
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    rc = f(keys.ctypes.data, keys.size, stride, cap, delta, resolution, e.ctypes.data, nlevels, 0, capn, prefix.ctypes.data,
           level.ctypes.data, count.ctypes.data, opn.ctypes.data, C.byref(num), stats.ctypes.data)
    return rc, stats


def path_keys(x, y, z, bmin, bmax, res):
    ml, edges, enc = O.level_table(bmin, bmax, res)
    nlevels = min(ml, 21)
    return O.chain_keys64(bmin, bmax, res, nlevels, x, y, z, threads=8), edges, enc, nlevels


def host_verdict(x, y, z, bmin, bmax, res, cap):
    """What the host logic of the single-chain build (csrc/pcv_spec.cpp: sample tree -> T'' -> exact counts -> pcv_spec_resolve)
    says about this cloud IN THIS ORDER, with the sample the device takes (pcv_spec_selftest_clumps): (status, stats) with
    stats = [T'' nodes, predicted leaves, points that passed a candidate, replayed points]. PCV_SPEC_OK: the prediction
    holds; PCV_SPEC_TOO_SHALLOW: PcvBuild::drop_single_chain and the exact pipeline."""
    keys, edges, _, nlevels = path_keys(x, y, z, bmin, bmax, res)
    stride, delta = sample_plan(x.size, cap)
    return _selftest("pcv_spec_selftest_clumps", keys, stride, cap, delta, res, edges, nlevels)


def selftest_with_device_sample(keys, stride, cap, delta, res, edges, nlevels):
    """pcv_spec_selftest samples every stride-th key: reorder the keys so that those are the device's sample (n must be a
    multiple of the stride, or the hook would take one sample more than the device)."""
    n = keys.size
    assert n % stride == 0
    src = sampled_positions(n, stride)
    rest = np.ones(n, dtype=bool)
    rest[src] = False
    out = np.empty(n, dtype=np.uint64)
    at = np.arange(n // stride, dtype=np.int64) * stride
    out[at] = keys[src]
    other = np.ones(n, dtype=bool)
    other[at] = False
    out[other] = keys[rest]
    return _selftest("pcv_spec_selftest", out, stride, cap, delta, res, edges, nlevels)


# ---- orders: (x, y, z, bmin, bmax) -> permutation (new position -> old index) ------------------------------------------
def _spread(v):  # 10 bits -> every third bit
    v = v.astype(np.uint32)
    v = (v | (v << 16)) & np.uint32(0x030000FF)
    v = (v | (v << 8)) & np.uint32(0x0300F00F)
    v = (v | (v << 4)) & np.uint32(0x030C30C3)
    v = (v | (v << 2)) & np.uint32(0x09249249)
    return v


def morton_key(x, y, z, bmin, bmax):
    """30-bit Morton key: 10 bits per axis over the cube of the longest box edge (x in the top bit of each triple, like the
    octree's child index)."""
    edge = float(np.max(np.asarray(bmax) - np.asarray(bmin))) or 1.0
    q = [np.clip(np.floor((a - lo) / edge * 1024.0), 0, 1023).astype(np.uint32) for a, lo in zip((x, y, z), bmin)]
    return (_spread(q[0]) << 2) | (_spread(q[1]) << 1) | _spread(q[2])


def shuffled(x, y, z, bmin, bmax):
    """The order the generators emit: every point's place drawn independently."""
    return np.arange(x.size, dtype=np.int64)


def morton(x, y, z, bmin, bmax):
    return np.argsort(morton_key(x, y, z, bmin, bmax), kind="stable").astype(np.int64)


def morton_reversed(x, y, z, bmin, bmax):
    return morton(x, y, z, bmin, bmax)[::-1].copy()


def scanline(x, y, z, bmin, bmax):
    """Slabs of 1/40 of the z extent, inside a slab row by row: coherent along one axis only."""
    slab = max(float(bmax[2] - bmin[2]) / 40.0, 1e-300)
    return np.lexsort((x, y, np.floor((z - bmin[2]) / slab))).astype(np.int64)


def cluster_major(centres):
    """Submaps: points grouped by nearest centre, one group after another, stable inside a group."""
    centres = np.asarray(centres, dtype=np.float64)

    def order(x, y, z, bmin, bmax):
        best = np.full(x.size, np.inf)
        which = np.zeros(x.size, dtype=np.int64)
        for k, c in enumerate(centres):
            d = (x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2
            closer = d < best
            which[closer], best[closer] = k, d[closer]
        return np.argsort(which, kind="stable").astype(np.int64)
    return order


def blocks(B, seed=5):
    """Morton order cut into blocks of B points, the blocks shuffled (a ragged last block stays last, so every seam sits on a
    multiple of B): B = 64 / 1 024 / 4 096 puts the seams between two unrelated places on the wave, tile and slice boundaries
    of the chain pass; B + 1 (`blocks_off`) lets them drift through every lane and slot position."""
    def order(x, y, z, bmin, bmax):
        m = morton(x, y, z, bmin, bmax)
        full = m.size // B
        which = np.random.default_rng(seed).permutation(full)
        return np.concatenate([m[:full * B].reshape(full, B)[which].reshape(-1), m[full * B:]])
    return order


def blocks_off(B, seed=5):
    return blocks(B + 1, seed)


BLOCK_SIZES = (64, 1024, 4096)


def orders(centres):
    out = {"shuffled": shuffled, "morton": morton, "morton_reversed": morton_reversed, "scanline": scanline,
           "cluster_major": cluster_major(centres)}
    for B in BLOCK_SIZES:
        out[f"blocks{B}"] = blocks(B)
        out[f"blocks_off{B}"] = blocks_off(B)
    return out


ORDER_NAMES = list(orders(np.zeros((1, 3))))
ORDERED = [k for k in ORDER_NAMES if k != "shuffled"]


class Cloud:
    """A cloud with its build parameters. `reorder(perm)` permutes the payloads WITH the points, so the colours (hash or
    index of the original position) still say which point is which."""

    def __init__(self, x, y, z, rgb, inten, bmin, bmax, cap, res, centres=None):
        self.x, self.y, self.z, self.rgb, self.inten = x, y, z, rgb, inten
        self.bmin, self.bmax, self.cap, self.res, self.centres = np.asarray(bmin, float), np.asarray(bmax, float), cap, res, centres
        self.n = x.size

    def reorder(self, perm):
        return Cloud(self.x[perm], self.y[perm], self.z[perm], np.ascontiguousarray(self.rgb[perm]),
                     None if self.inten is None else self.inten[perm], self.bmin, self.bmax, self.cap, self.res, self.centres)

    def ordered(self, name):
        return self.reorder(orders(self.centres)[name](self.x, self.y, self.z, self.bmin, self.bmax))

    def oracle(self):
        with O.max_points_per_node(self.cap):
            return O.build_closed(self.res, self.bmin, self.bmax, self.x, self.y, self.z, self.rgb, self.inten, threads=8)

    def verdict(self):
        return host_verdict(self.x, self.y, self.z, self.bmin, self.bmax, self.res, self.cap)


def _centres(seed, num_clusters, extent):  # the first draw of synthetic.gaussian_clusters
    return np.random.Generator(np.random.PCG64(seed)).uniform(0.0, extent, (num_clusters, 3))


# ---- the base clouds: the smallest shapes at which the paths named beside them are taken ---------------------------------
BASE = {  # n, cap, res, intensity, (seed, clusters, extent, sigma range)
    "a": (600_000, 20_000, 0.001, False, (1, 6, 200.0, (0.2, 8.0))),     # few leaves, one sort pass
    "b": (300_000, 400, 0.001, True, (4, 5, 60.0, (0.01, 2.0))),         # settling second pass, plane, climber records
    "c": (1_300_000, 30_000, 0.0002, False, (7, 7, 220.0, (0.1, 7.0))),  # depth-binned pass, wide records, last tile of 544
}
_cache = {}


def base_cloud(name):
    if name not in _cache:
        n, cap, res, with_int, (seed, k, extent, sigma) = BASE[name]
        x, y, z, rgb, bmin, bmax = synthetic.gaussian_clusters(n, seed=seed, num_clusters=k, extent=extent, sigma_range=sigma)
        inten = ((np.arange(n, dtype=np.int64) * 2654435761) % 100_003).astype(np.float32) * 0.25 - 7.0 if with_int else None
        _cache[name] = Cloud(x, y, z, rgb, inten, bmin, bmax, cap, res, _centres(seed, k, extent))
    return _cache[name]


# ---- constructed clouds ----------------------------------------------------------------------------------------------------
STARVED_CENTRE = (30.0, 30.0, 30.0)
STARVED_DENSE = 30_000


def _starved(n, cap, seed):
    """A prediction that must be too shallow: n points uniform in [0, 200)^3, 30 000 of them moved tightly (sigma 0.05)
    around (30, 30, 30) — only at input positions the sample never reads (i % (8 * stride) >= 8, stride from the hook). The
    cell around (30, 30, 30) at the level where the uniform background's leaves are then holds 30 000 points more than the
    sample can know of: a predicted LEAF that must split, so pcv_spec_resolve returns PCV_SPEC_TOO_SHALLOW and
    PcvBuild::drop_single_chain hands the build to the exact pipeline after the record sort was queued."""
    rng = np.random.default_rng(seed)
    stride, _ = sample_plan(n, cap)
    x, y, z = rng.uniform(0.0, 200.0, n), rng.uniform(0.0, 200.0, n), rng.uniform(0.0, 200.0, n)
    unread = np.flatnonzero(np.arange(n) % (8 * stride) >= 8)
    at = rng.permutation(unread)[:STARVED_DENSE]
    x[at], y[at], z[at] = (STARVED_CENTRE[a] + rng.normal(0.0, 0.05, STARVED_DENSE) for a in range(3))
    return Cloud(x, y, z, synthetic.index_colors(n), None, np.zeros(3), np.full(3, 200.0), cap, 0.001)


def starved():
    """600 000 points, capacity 20 000: stride 64, delta 0.283, the band's lower end 14 343. The target is the level-2 cell
    r00 = [0, 50)^3: (600 000 - 30 000) / 64 = 8 906 background points + 30 000 = ~38 900 > 20 000 (counted: 39 023), of
    which the scaled sample sees ~8 906 (counted: 9 152) < 14 343. ~70 predicted leaves: ONE sort pass, queued ahead of the
    verdict."""
    return _starved(600_000, 20_000, 101)


def starved_settling():
    """300 000 points, capacity 1 500: stride 16, delta 0.516, lower end 725. The level-2 cells hold 4 200 background points
    and split for everyone; the target is the level-3 cell r007 = [25, 50)^3: 270 000 / 512 = 527 background points + 30 000
    (counted: 30 527) > 1 500, of which the scaled sample sees ~527 (counted: 320) < 725. ~790 predicted leaves = 10 rank
    bits: the record sort has two passes, the second held back (sort_second.pending), so drop_single_chain runs with its
    join_side branch."""
    return _starved(300_000, 1_500, 102)


STARVED_TARGET_LEVEL = {"starved": 2, "starved_settling": 3}  # level of the cell around STARVED_CENTRE that must split

OVERSAMPLED_CENTRES = [(30.0, 30.0, 30.0), (170.0, 40.0, 35.0), (45.0, 160.0, 30.0), (160.0, 165.0, 40.0),
                       (35.0, 40.0, 170.0), (165.0, 160.0, 165.0)]


def pool_tops(res=0.0001):
    """The oversampled clusters of test_oversampled_clusters_replay_the_chain_from_their_coordinates (six clusters of 700
    points exactly AT the sampled positions: their level-2 nodes look like ~54 k points (64 x 700 + 9 k) and are split without kept codes, the
    exact ~10 k make them leaves whose points replay the chain) at resolution 0.0001: edge / resolution >= 2^16 down to level
    4 (200 / 16 / 0.0001 = 125 000), so every level a leaf or candidate can have here is Float32-coded and EVERY point takes
    an entry of the Float32 pool. pcv_pool_region_entries(600 000) = 1 024 = one full 1 024-point slice: the regions of the
    585 full slices are full to pool_cap, and the first replayed point makes most + 1 > pool_cap in settle_verdict
    (csrc/pcv_single_chain.hip): the second give-up."""
    rng = np.random.default_rng(77)
    n, cap, k = 600_000, 20_000, 700
    stride, _ = sample_plan(n, cap)
    x, y, z = rng.uniform(0.0, 200.0, n), rng.uniform(0.0, 200.0, n), rng.uniform(0.0, 200.0, n)
    sampled = np.flatnonzero(np.arange(n) % (8 * stride) < 8)
    slots = rng.permutation(sampled)[: 6 * k].reshape(6, k)
    for c, centre in enumerate(OVERSAMPLED_CENTRES):
        x[slots[c]], y[slots[c]], z[slots[c]] = (centre[a] + rng.normal(0.0, 0.05, k) for a in range(3))
    return Cloud(x, y, z, synthetic.index_colors(n), None, np.zeros(3), np.full(3, 200.0), cap, res)


def one_class_tiles():
    """Whole 1 024-point tiles of ONE predicted depth: a third of 1 300 000 points (>= 2^20: the depth-binned chain pass;
    a last tile of 544) in one very tight cluster (sigma 0.02 around (77.7, 131.3, 52.1)), the rest uniform in [0, 200)^3,
    in Morton order. At capacity 30 000 the background's leaves are the 64 level-2 cells (~13 500 points each) and the
    cluster goes several levels deeper; Morton order lays the cluster's 433 333 points down as ~420 consecutive tiles of a
    single depth class each, and the background as runs of ~13 tiles per level-2 cell. The chain pass's deal (one LDS counter
    per depth class) then hands all 1 024 slots of a tile to one class."""
    rng = np.random.default_rng(103)
    n = 1_300_000
    m = n // 3
    x, y, z = rng.uniform(0.0, 200.0, n), rng.uniform(0.0, 200.0, n), rng.uniform(0.0, 200.0, n)
    at = rng.permutation(n)[:m]
    for a, c in zip((x, y, z), (77.7, 131.3, 52.1)):
        a[at] = c + rng.normal(0.0, 0.02, m)
    cl = Cloud(x, y, z, synthetic.hash_colors(n), None, np.zeros(3), np.full(3, 200.0), 30_000, 0.001)
    return cl.reorder(morton(x, y, z, cl.bmin, cl.bmax))


CONSTRUCTED = {"starved": starved, "starved_settling": starved_settling, "pool_tops": pool_tops, "one_class_tiles": one_class_tiles}


# ---- what the host logic (host_verdict / Cloud.verdict) predicts for every case of tests/test_gpu_order_fuzz.py. Recorded here,
# recomputed entry by entry in tests/test_order_cases_cpu.py: the GPU test knows what to expect without asking the code under
# test. (pool_tops HOLDS as far as pcv_spec_resolve goes; its give-up is the pool arithmetic of settle_verdict.)
HELD, SHALLOW = "held", "too_shallow"
PREDICTED = {(c, o): HELD for c in BASE for o in ORDER_NAMES}
PREDICTED.update({("starved", None): SHALLOW, ("starved_settling", None): SHALLOW, ("pool_tops", None): HELD,
                  ("one_class_tiles", None): HELD})
