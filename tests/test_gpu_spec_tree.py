"""The predicted tree T'' of the single-chain build, made from the sorted sample keys in two launches
(spec_sample_open_kernel + spec_tree_build_kernel, csrc/pcv_topology.hip), against the node-table split it replaces
(libpcv_hip_exp.so, PCV_SAMPLE_TREE_SPLIT=1): the same build statistics and the same bytes in every node, and both equal to the
oracle. The cases put sample nodes exactly at the split threshold and at the candidate band's upper end (the two probes of
the open-run pass), force level-1 splits, need sample keys deeper than the first ones (the re-key) and sample every point."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O
import point_cloud_viewer_amd as pcv
from point_cloud_viewer_amd import synthetic
from test_gpu_build import assert_same

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INFO_KEYS = ("single_chain", "predicted_nodes", "predicted_leaves", "kept_code_points", "continued_points", "replayed_points")


def _sample_bounds(n, cap):
    """stride, split threshold and floor(upper) of the sample as plan_sample derives them (pcv_single_chain.hip)."""
    stride = 64
    while stride > 1 and n // stride < 4096:
        stride >>= 1
    while stride > 1 and cap // stride < 64:
        stride >>= 1
    delta = 0.0 if stride == 1 else min(0.9, max(0.02, 5.0 * math.sqrt(stride / cap)))
    thr = math.floor(cap * (1.0 - delta) / stride)
    upper = math.floor(cap * (1.0 + delta) / stride)
    return stride, thr, upper


def _octant_cloud(n, cap, sample_counts, seed):
    """n points in the cube [0, 8)^3 whose SAMPLE points (the clumps of 8 single_chain_topology takes) fall into the eight
    level-1 octants exactly `sample_counts` times; every other point takes the octant of a sample point of its clump, so an
    octant holds stride x its sample count (the prediction is right about it)."""
    stride, _, _ = _sample_bounds(n, cap)
    ns = n // stride
    assert sum(sample_counts) == ns and ns * stride == n
    rng = np.random.default_rng(seed)
    sample_octant = rng.permutation(np.repeat(np.arange(8), sample_counts))
    p = np.arange(n, dtype=np.int64)
    # clump j of the sample (samples 8 j .. 8 j + 7) sits at the first eight points of the block [8 j stride, 8 (j + 1) stride)
    octant = sample_octant[(p // (8 * stride)) * 8 + (p % 8)] if stride > 1 else sample_octant
    pos = rng.uniform(0.05, 3.95, (n, 3))
    for axis in range(3):
        pos[:, axis] += 4.0 * ((octant >> axis) & 1)
    return pos[:, 0].copy(), pos[:, 1].copy(), pos[:, 2].copy(), synthetic.hash_colors(n), np.zeros(3), np.full(3, 8.0)


def _boundary_counts(n, cap):
    _, thr, upper = _sample_bounds(n, cap)
    ns = n // _sample_bounds(n, cap)[0]
    counts = [thr, thr + 1, upper, upper + 1, thr - 1, upper - 1]
    rest = ns - sum(counts)
    return counts + [rest // 2, rest - rest // 2]


def cloud(name):
    """(x, y, z, rgb, bmin, bmax, resolution, capacity, force_mask) of one case"""
    if name == "clustered":
        x, y, z, rgb, bmin, bmax = synthetic.gaussian_clusters(600_000, seed=1, num_clusters=6, extent=200.0, sigma_range=(0.2, 8.0))
        return x, y, z, rgb, bmin, bmax, 0.001, 20_000, 0
    if name == "uniform":
        rng = np.random.default_rng(7)
        p = rng.uniform(-50.0, 50.0, (700_000, 3))
        return p[:, 0].copy(), p[:, 1].copy(), p[:, 2].copy(), synthetic.hash_colors(700_000), np.full(3, -50.0), np.full(3, 50.0), 0.001, 5_000, 0
    if name == "duplicates":  # 400 000 points on 300 positions: nodes stop at the resolution with more than the capacity
        rng = np.random.default_rng(8)
        at = rng.uniform(-5.0, 5.0, (300, 3))
        p = at[rng.integers(0, 300, 400_000)]
        return p[:, 0].copy(), p[:, 1].copy(), p[:, 2].copy(), synthetic.hash_colors(400_000), np.full(3, -5.0), np.full(3, 5.0), 0.01, 2_000, 0
    if name == "at_threshold_and_band":  # stride 64: level-1 sample counts thr, thr + 1, floor(upper), floor(upper) + 1, ...
        n, cap = 524_288, 20_000
        return _octant_cloud(n, cap, _boundary_counts(n, cap), seed=9) + (0.001, cap, 0)
    if name == "stride1_tiny":  # every point is a sample point: threshold == band == capacity
        n, cap = 6_000, 500
        assert _sample_bounds(n, cap) == (1, cap, cap)
        return _octant_cloud(n, cap, [cap, cap + 1, cap - 1, 1200, 1300, 1000, cap, cap], seed=10) + (0.001, cap, 0)
    if name == "forced_level1":  # three clusters: most level-1 nodes hold few points and are split because the mask says so
        x, y, z, rgb, bmin, bmax = synthetic.gaussian_clusters(600_000, seed=12, num_clusters=3, extent=300.0, sigma_range=(0.3, 6.0))
        return x, y, z, rgb, bmin, bmax, 0.001, 20_000, 0b10110111
    if name == "rekey_deep":  # a cluster that needs ~17 levels, more than the sample keys' first 11: keyed again at full depth
        rng = np.random.default_rng(13)
        wide = rng.uniform(-1000.0, 1000.0, (400_000, 3))
        tight = 123.456 + rng.normal(0.0, 0.002, (200_000, 3))
        p = np.concatenate([wide, tight])[rng.permutation(600_000)]
        return p[:, 0].copy(), p[:, 1].copy(), p[:, 2].copy(), synthetic.hash_colors(600_000), np.full(3, -1000.0), np.full(3, 1000.0), 0.001, 2_000, 0
    raise KeyError(name)


CASES = ["clustered", "uniform", "duplicates", "at_threshold_and_band", "stride1_tiny", "forced_level1", "rekey_deep"]
HELD = ("clustered", "uniform", "at_threshold_and_band", "forced_level1")


def build(ctx, name):
    """the single-chain build of one case (forced onto that path whatever its size); returns the tree"""
    import point_cloud_viewer_amd._lib as L
    x, y, z, rgb, bmin, bmax, res, cap, mask = cloud(name)
    if not mask:
        return ctx.build(res, pcv.Aabb(bmin, bmax), x, y, z, rgb, max_points_per_node=cap, single_chain=True, check_resolve=True)
    import ctypes as C
    p, keep = ctx._points(x, y, z, rgb, None)
    pr = ctx._params(res, bmin, bmax, cap, ((mask & 0xFF) << 8) | L.BUILD_FORCE_SINGLE_CHAIN)
    h = C.c_void_p()
    ctx._check(ctx.lib.pcv_build_begin(ctx.handle, C.byref(pr), C.byref(p), C.byref(h)))
    from point_cloud_viewer_amd.octree import PendingBuild
    return PendingBuild(ctx, h, keep).finish(None)


def summary(tree):
    import bench
    info = tree.build_info()
    return {"info": {k: int(info[k]) for k in INFO_KEYS}, "nodes": bench.digest_of_digests(bench.tree_digests(tree))}


_CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import point_cloud_viewer_amd as pcv
import test_gpu_spec_tree as T
ctx = pcv.Context(0)
out = {}
for name in T.CASES:
    t = T.build(ctx, name)
    out[name] = T.summary(t)
    t.free()
print("SUMMARY " + json.dumps(out))
"""


def _exp_summaries(env):
    out = subprocess.run([sys.executable, "-c", _CHILD, ROOT], env=dict(os.environ, PCV_HIP_LIBRARY="exp", **env),
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    line = [s for s in out.stdout.splitlines() if s.startswith("SUMMARY ")][-1]
    return json.loads(line[len("SUMMARY "):])


@pytest.fixture(scope="module")
def ctx():
    c = pcv.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def shipped():
    return {}


@pytest.mark.parametrize("name", CASES)
def test_sample_tree_from_sorted_keys_equals_oracle(ctx, shipped, name):
    x, y, z, rgb, bmin, bmax, res, cap, mask = cloud(name)
    with O.max_points_per_node(cap):
        if mask:
            want, _ = O.build_closed_shard(res, bmin, bmax, x, y, z, rgb, threads=8, force_mask=mask)
        else:
            want = O.build_closed(res, bmin, bmax, x, y, z, rgb, threads=8)
    t = build(ctx, name)
    assert_same(t.to_dict(), want)
    shipped[name] = summary(t)
    if name in HELD:  # the prediction, not the exact pipeline, made the tree
        assert shipped[name]["info"]["single_chain"] and shipped[name]["info"]["predicted_nodes"] > 0, shipped[name]
    t.free()


def test_two_launch_tree_equals_the_node_table_split(shipped):
    """the experiment library with the old path (node table by split kernels + spec_tree_scan / emit) and with the new one
    against each other and against the shipped library: same statistics, same node bytes"""
    if not os.path.exists(os.path.join(os.path.dirname(pcv._lib.LIB_PATH), "libpcv_hip_exp.so")):
        pytest.skip("libpcv_hip_exp.so (make -C point_cloud_viewer_amd/csrc) is not built")
    new = _exp_summaries({})
    old = _exp_summaries({"PCV_SAMPLE_TREE_SPLIT": "1"})
    for name in CASES:
        assert new[name] == old[name], (name, new[name], old[name])
        if name in shipped:
            assert shipped[name] == new[name], (name, shipped[name], new[name])
