"""The orders and constructed clouds of tests/order_cases.py, checked on the CPU: every order is a permutation that really
reorders, the oracle's tree is the same for every order while its bytes are not, and the arithmetic that makes each
constructed cloud do what it claims is counted here — with the stride and band of the library's own sample plan
(pcv_spec_sample_plan, which plan_sample in csrc/pcv_single_chain.hip calls) — not asserted from memory."""
import numpy as np
import pytest

import oracle_lib as O
import order_cases as OC


@pytest.fixture(scope="module")
def small():
    rng = np.random.default_rng(9)
    n = 50_001
    centres = rng.uniform(0.0, 100.0, (4, 3))
    p = centres[rng.integers(0, 4, n)] + rng.normal(0.0, 3.0, (n, 3))
    x, y, z = (np.ascontiguousarray(p[:, a]) for a in range(3))
    return x, y, z, p.min(axis=0), p.max(axis=0), centres


def test_the_sample_plan_hook_gives_the_strides_the_cases_were_built_for():
    """pcv_spec_sample_plan (csrc/pcv_spec.cpp): stride 64 from 4 096 x 64 points on, halved until a node at the capacity holds
    64 sample points; delta = 5 sqrt(stride / cap) within [0.02, 0.9]; stride 1 samples everything and has no band."""
    assert OC.sample_plan(600_000, 20_000) == (64, pytest.approx(5.0 * np.sqrt(64 / 20_000)))
    assert OC.sample_plan(300_000, 1_500) == (16, pytest.approx(5.0 * np.sqrt(16 / 1_500)))
    assert OC.sample_plan(300_000, 400) == (4, pytest.approx(0.5))
    assert OC.sample_plan(1_300_000, 30_000)[0] == 64 and OC.sample_plan(100_000_000, 100_000)[0] == 64
    assert OC.sample_plan(100_000, 100_000)[0] == 16 and OC.sample_plan(5_000, 12) == (1, 0.0)
    assert OC.sample_plan(10_000_000, 64 * 64)[1] == pytest.approx(5.0 / 8.0) and OC.sample_plan(1 << 30, 1 << 30)[1] == 0.02
    # the sample the device reads (chain_keys_kernel, csrc/pcv_chain.hip): 8 consecutive positions every 8 x stride
    src = OC.sampled_positions(600_000, 64)
    assert src.size == 9_375 and np.all(src % 512 < 8) and np.array_equal(src[:10], [0, 1, 2, 3, 4, 5, 6, 7, 512, 513])
    assert src[-1] < 600_000


@pytest.mark.parametrize("name", OC.ORDER_NAMES)
def test_every_order_is_a_permutation(small, name):
    x, y, z, bmin, bmax, centres = small
    perm = OC.orders(centres)[name](x, y, z, bmin, bmax)
    assert perm.shape == (x.size,) and np.array_equal(np.sort(perm), np.arange(x.size))
    if name != "shuffled":
        assert np.count_nonzero(perm != np.arange(x.size)) > 0.99 * x.size  # and not the identity


def test_coherent_orders_are_coherent(small):
    x, y, z, bmin, bmax, centres = small
    key = OC.morton_key(x, y, z, bmin, bmax)
    m = OC.morton(x, y, z, bmin, bmax)
    assert np.all(np.diff(key[m].astype(np.int64)) >= 0) and np.all(np.diff(key[OC.morton_reversed(x, y, z, bmin, bmax)].astype(np.int64)) <= 0)
    # stable: equal keys keep their input order
    same = np.flatnonzero(np.diff(key[m].astype(np.int64)) == 0)
    assert same.size and np.all(m[same] < m[same + 1])
    s = OC.scanline(x, y, z, bmin, bmax)
    slab = np.floor((z[s] - bmin[2]) / ((bmax[2] - bmin[2]) / 40.0))
    assert np.all(np.diff(slab) >= 0) and 30 <= np.unique(slab).size <= 41
    c = OC.cluster_major(centres)(x, y, z, bmin, bmax)
    d = np.stack([(x[c] - k[0]) ** 2 + (y[c] - k[1]) ** 2 + (z[c] - k[2]) ** 2 for k in centres])
    which = np.argmin(d, axis=0)
    assert np.all(np.diff(which) >= 0) and np.unique(which).size == 4
    for k in range(4):
        assert np.all(np.diff(c[which == k]) > 0)  # stable inside a group


@pytest.mark.parametrize("B", [b + off for b in OC.BLOCK_SIZES for off in (0, 1)])
def test_blocks_put_their_seams_where_they_say(small, B):
    """Inside a block the Morton rank goes up by one; it jumps only at multiples of B (B + 1 for blocks_off), and at nearly all
    of them."""
    x, y, z, bmin, bmax, centres = small
    perm = OC.blocks(B)(x, y, z, bmin, bmax)
    rank = np.empty(x.size, dtype=np.int64)
    rank[OC.morton(x, y, z, bmin, bmax)] = np.arange(x.size)
    step = np.diff(rank[perm])
    seams = np.flatnonzero(step != 1) + 1
    assert np.all(seams % B == 0)
    possible = (x.size - 1) // B
    # a shuffled block keeps its Morton successor with probability 1 / blocks: one such non-seam expected, whatever B
    assert seams.size >= possible - 5 and seams.size >= 10
    off = OC.blocks_off(B - 1)(x, y, z, bmin, bmax) if B - 1 in OC.BLOCK_SIZES else None
    if off is not None:
        assert np.array_equal(off, perm)
        assert np.unique(seams % 64).size >= min(10, seams.size // 2)  # the seams drift through the lane positions


@pytest.mark.parametrize("cloud", list(OC.BASE))
def test_the_oracle_tree_is_the_same_for_every_order_and_its_bytes_are_not(cloud):
    """The oracle is stable: node names and num_points do not depend on the input order, the bytes do (which points a node
    keeps is decided by the order inside each leaf: every 8th point climbs, generation.rs:222-238). At least half the nodes
    differ between `shuffled` and `morton`: an order helper that quietly did nothing would show here. Also records what the
    host logic says of every ordered case (OC.PREDICTED): held or too shallow."""
    base = OC.base_cloud(cloud)
    want = base.oracle()
    shape = {k: v["num_points"] for k, v in want.nodes.items()}
    assert sum(shape.values()) == base.n
    for name in OC.ORDERED:
        cl = base.ordered(name)
        got = cl.oracle()
        assert {k: v["num_points"] for k, v in got.nodes.items()} == shape, name
        differ = sum(1 for k in shape if got.nodes[k]["xyz"] != want.nodes[k]["xyz"] or got.nodes[k]["rgb"] != want.nodes[k]["rgb"])
        # (cluster_major is stable inside a group and a node's points nearly all come from one cluster: it moves every point
        # and leaves most nodes' bytes alone, in (b) all of them — what it changes is WHERE in the input a node's points lie)
        assert name == "cluster_major" or differ >= len(shape) // 2, (name, differ, len(shape))
        status, stats = cl.verdict()
        assert {OC.PCV_SPEC_OK: OC.HELD, OC.PCV_SPEC_TOO_SHALLOW: OC.SHALLOW}[status] == OC.PREDICTED[(cloud, name)], (name, status, stats)
    status, _ = base.verdict()
    assert status == OC.PCV_SPEC_OK and OC.PREDICTED[(cloud, "shuffled")] == OC.HELD


@pytest.mark.parametrize("name,n,cap", [("starved", 600_000, 20_000), ("starved_settling", 300_000, 1_500)])
def test_starved_clouds_hide_a_full_node_from_the_sample(name, n, cap):
    """The arithmetic of OC.starved / OC.starved_settling, counted: with the hook's stride, the cell around (30, 30, 30) at the
    level of the background's leaves holds more points than the capacity while its scaled clump-sample count is below the
    band's lower end cap * (1 - delta) — so it is a predicted LEAF that must split. pcv_spec_selftest, fed a key array whose
    every stride-th entry is the device's sample, says PCV_SPEC_TOO_SHALLOW; so does the hook that takes the clumps itself."""
    cl = OC.CONSTRUCTED[name]()
    assert cl.n == n and cl.cap == cap
    stride, delta = OC.sample_plan(n, cap)
    level = OC.STARVED_TARGET_LEVEL[name]
    edge = 200.0 / 2 ** level
    inside = np.ones(n, dtype=bool)
    for a, c in zip((cl.x, cl.y, cl.z), OC.STARVED_CENTRE):
        inside &= np.floor(a / edge) == np.floor(c / edge)
    true_count = int(inside.sum())
    seen = int(inside[OC.sampled_positions(n, stride)].sum()) * stride
    print(f"{name}: stride {stride}, delta {delta:.4f}, level-{level} cell holds {true_count}, the scaled sample sees {seen}, "
          f"lower end {OC.lower_threshold(cap, delta):.0f}")
    assert true_count > cap and seen < OC.lower_threshold(cap, delta)
    # the parent of the target IS opened by the sample (or the target would not be a node of the predicted tree at all)
    parent = np.ones(n, dtype=bool)
    for a, c in zip((cl.x, cl.y, cl.z), OC.STARVED_CENTRE):
        parent &= np.floor(a / (2 * edge)) == np.floor(c / (2 * edge))
    assert int(parent[OC.sampled_positions(n, stride)].sum()) * stride > cap * (1.0 + delta)
    want = cl.oracle()
    target = "r" + "0" * (level - 1) + ("0" if level == 2 else "7")
    assert any(k.startswith(target) and len(k) > len(target) for k in want.nodes), target  # the truth splits it
    keys, edges, _, nlevels = OC.path_keys(cl.x, cl.y, cl.z, cl.bmin, cl.bmax, cl.res)
    status, _ = OC.selftest_with_device_sample(keys, stride, cap, delta, cl.res, edges, nlevels)
    assert status == OC.PCV_SPEC_TOO_SHALLOW
    assert cl.verdict()[0] == OC.PCV_SPEC_TOO_SHALLOW and OC.PREDICTED[(name, None)] == OC.SHALLOW
    # the same cloud with the tight points where the sample CAN see them is predicted fine: it is the order that starves
    rng = np.random.default_rng(1)
    assert cl.reorder(rng.permutation(n)).verdict()[0] == OC.PCV_SPEC_OK


def test_pool_tops_fills_whole_pool_regions_and_replays():
    """OC.pool_tops: pcv_spec_resolve holds with replayed points (the oversampled clusters), every leaf of the tree is
    Float32-coded (every point takes a pool entry in the chain pass), and a region of the pool has exactly the 1 024 entries of
    one full input slice (pcv_pool_region_entries, csrc/pcv_internal.h): settle_verdict's most + ceil(replay / 1 024) >
    pool_cap must be true."""
    cl = OC.pool_tops()
    status, stats = cl.verdict()
    assert status == OC.PCV_SPEC_OK and stats[3] >= 6 * 700 and OC.PREDICTED[("pool_tops", None)] == OC.HELD, (status, stats)
    _, _, enc = O.level_table(cl.bmin, cl.bmax, cl.res)
    want = cl.oracle()
    leaves = [k for k in want.nodes if not any(c.startswith(k) and len(c) == len(k) + 1 for c in want.nodes)]
    float32 = want.nodes["r"]["encoding"]  # the root of a 200 m cube at 0.1 mm
    assert all(int(e) == float32 for e in enc[:5]) and int(enc[5]) != float32
    assert all(1 <= len(k) - 1 <= 4 and want.nodes[k]["encoding"] == float32 for k in leaves)
    slices, regions = (cl.n + 1023) // 1024, 1024
    pool_cap = (slices + regions - 1) // regions * 1024
    assert pool_cap == 1024 and slices <= regions and cl.n // 1024 >= 1  # one slice per region, full slices fill theirs
    # the same cloud at 1 mm keeps the integer-coded levels out of the pool: the existing replay test's geometry
    _, _, enc3 = O.level_table(cl.bmin, cl.bmax, 0.001)
    assert int(enc3[2]) != float32


def test_one_class_tiles_has_whole_tiles_of_one_depth_class():
    """OC.one_class_tiles: the chain pass (chain_pass_kernel, csrc/pcv_encode.hip) deals the points of a 1 024-point tile by
    predicted leaf depth, read from a 128^3 grid over the root cube: classes 1..7, and 8 for "deeper than the grid". With the
    TRUE leaf depth in place of the predicted one (the predicted tree is at least as deep, and equal almost everywhere): in
    the cloud's Morton order hundreds of whole tiles are of class 2 (the background's level-2 leaves) and hundreds of class 8
    (the tight cluster; counted: 831 and 280 of 1 269) — one LDS counter takes all 1 024 points. 1 300 000 points: >= 2^20, a last tile of 544."""
    cl = OC.one_class_tiles()
    assert cl.n >= 1 << 20 and cl.n % 1024 == 544
    status, _ = cl.verdict()
    assert status == OC.PCV_SPEC_OK and OC.PREDICTED[("one_class_tiles", None)] == OC.HELD
    want = cl.oracle()
    keys, _, _, _ = OC.path_keys(cl.x, cl.y, cl.z, cl.bmin, cl.bmax, cl.res)
    depth = np.zeros(cl.n, dtype=np.int64)
    for name in want.nodes:
        if any(c.startswith(name) and len(c) == len(name) + 1 for c in want.nodes):
            continue  # not a leaf
        lvl = len(name) - 1
        pfx = sum(int(d) << (3 * (21 - k)) for k, d in enumerate(name[1:], start=1))
        sh = 3 * (21 - lvl)
        depth[(keys >> np.uint64(sh)) == np.uint64(pfx >> sh)] = lvl
    assert np.all(depth >= 1)
    full = cl.n // 1024
    t = np.minimum(depth, 8)[:full * 1024].reshape(full, 1024)
    single = t[np.all(t == t[:, :1], axis=1), 0]
    print(f"one_class_tiles: {single.size} of {full} full tiles have one depth class; tiles per class {np.bincount(single)}")
    assert np.count_nonzero(single == 2) >= 200 and np.count_nonzero(single == 8) >= 200
