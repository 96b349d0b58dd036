"""The single-chain build (csrc/pcv_spec.h: topology predicted from a strided sample, ONE chain pass, exact per-leaf
counts decide the tree) against the CPU oracle: byte-exact like every other build test, whatever the prediction did —
held, kept a candidate's codes as leaf codes, continued the chain from a split candidate's codes, replayed the chain
from the coordinates for a few points, or gave up and let the exact pipeline redo the build. The reference has one answer per input (src/octree/generation.rs:289-403); so do all of these paths."""
import numpy as np
import pytest

import oracle_lib as O
import point_cloud_viewer_amd as pcv
from point_cloud_viewer_amd import synthetic
from test_gpu_build import assert_same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = pcv.Context(0)
    yield c
    c.close()


SEEN = {"held": 0, "fell_back": 0, "kept": 0, "continued": 0, "replayed": 0}

CASES = [  # n, capacity, resolution, clusters, extent, sigma range, intensity, seed
    (600_000, 20_000, 0.001, 6, 200.0, (0.2, 8.0), False, 1),
    (600_000, 20_000, 0.001, 6, 200.0, (0.2, 8.0), True, 2),
    (800_000, 5_000, 0.001, 12, 300.0, (0.05, 5.0), False, 3),
    (300_000, 2_000, 0.01, 5, 60.0, (0.01, 2.0), True, 4),
    (200_000, 300, 0.001, 4, 40.0, (0.005, 1.0), False, 5),
    (1_500_000, 100_000, 0.001, 3, 150.0, (0.5, 6.0), False, 6),
    (1_300_000, 30_000, 0.001, 7, 220.0, (0.1, 7.0), True, 7),   # >= 2^20 points: depth-binned pass, with intensity
    # finer resolutions: levels 1..5 are Float32-coded, so most leaves (and the candidates whose kept codes are taken,
    # and the replayed leaves) are "wide" for the packed 12-byte records — their codes travel through the side array
    (600_000, 20_000, 0.0001, 6, 200.0, (0.2, 8.0), True, 21),
    (800_000, 5_000, 0.0002, 12, 300.0, (0.05, 5.0), False, 22),
    (1_200_000, 60_000, 0.0001, 5, 180.0, (0.3, 9.0), False, 23),
]


@pytest.mark.parametrize("n,cap,res,clusters,extent,sigma,with_int,seed", CASES)
def test_forced_single_chain_equals_oracle(ctx, n, cap, res, clusters, extent, sigma, with_int, seed):
    x, y, z, rgb, bmin, bmax = synthetic.gaussian_clusters(n, seed=seed, num_clusters=clusters, extent=extent, sigma_range=sigma)
    inten = (np.arange(n) % 509).astype(np.float32) * 0.5 if with_int else None
    with O.max_points_per_node(cap):
        want = O.build_closed(res, bmin, bmax, x, y, z, rgb, inten, threads=8)
    t = ctx.build(res, pcv.Aabb(bmin, bmax), x, y, z, rgb, inten, max_points_per_node=cap, single_chain=True, check_resolve=True)
    info = t.build_info()
    assert_same(t.to_dict(), want, check_intensity=with_int)
    assert info["attempts"] in (0, 2, 3), info  # held, or redone by the exact pipeline (with or without its own retry)
    SEEN["held" if info["single_chain"] else "fell_back"] += 1
    SEEN["kept"] += info["kept_code_points"] > 0
    SEEN["replayed"] += info["replayed_points"] > 0
    SEEN["continued"] += info["continued_points"] > 0
    if info["single_chain"]:
        assert info["record_bytes"] == 12, info  # packed records are what ships on this path
        leaves = sum(1 for k in want.nodes if not any(c.startswith(k) and len(c) == len(k) + 1 for c in want.nodes))
        assert info["predicted_leaves"] >= leaves
    t.free()
    # same input through the exact pipeline: the two must agree with each other, too
    t2 = ctx.build(res, pcv.Aabb(bmin, bmax), x, y, z, rgb, inten, max_points_per_node=cap, single_chain=False)
    assert t2.build_info()["attempts"] >= 1
    assert_same(t2.to_dict(), want, check_intensity=with_int)


def test_the_cases_above_covered_every_branch_of_the_prediction():
    """held / a candidate's codes were the leaf codes / the chain was continued from a split candidate's codes must all
    have happened above (the replay from coordinates needs a sample that OVER-counts a node: next test)."""
    assert SEEN["held"] >= 3 and SEEN["kept"] >= 2 and SEEN["continued"] >= 2, SEEN


def test_oversampled_clusters_replay_the_chain_from_their_coordinates(ctx):
    """A sample that over-counts: six tight clusters of 700 points sit at input positions i % 256 < 8. The build samples 8
    consecutive points every 512 (stride 64 at 600 000 points and capacity 20 000: pcv_spec_sample_plan, csrc/pcv_spec.cpp), so
    half of every cluster is in the sample — 64 x 350 on top of 9 k background points —
    and their level-2 nodes look like 30 k points to the prediction — above the candidate
    band, split without kept codes — while the exact counts (~10 k < capacity 20 k) make those nodes LEAVES. Their points
    went down to candidates below the leaf, so their records hold codes of a deeper level: the one case that still needs
    the coordinates (PCV_SPEC_MAP_REPLAY). (The clusters take a fifth of the sampled slots; more would starve the sample
    of background points and send the whole build to the exact pipeline.) Byte-exact like everything else."""
    rng = np.random.default_rng(77)
    n, cap, k = 600_000, 20_000, 700
    x, y, z = rng.uniform(0.0, 200.0, n), rng.uniform(0.0, 200.0, n), rng.uniform(0.0, 200.0, n)
    sampled = np.flatnonzero(np.arange(n) % 256 < 8)
    slots = rng.permutation(sampled)[: 6 * k].reshape(6, k)
    for c, centre in enumerate([(30.0, 30.0, 30.0), (170.0, 40.0, 35.0), (45.0, 160.0, 30.0), (160.0, 165.0, 40.0),
                                (35.0, 40.0, 170.0), (165.0, 160.0, 165.0)]):
        x[slots[c]], y[slots[c]], z[slots[c]] = (centre[a] + rng.normal(0.0, 0.05, k) for a in range(3))
    rgb = synthetic.index_colors(n)
    bmin, bmax = np.array([0.0, 0.0, 0.0]), np.array([200.0, 200.0, 200.0])
    with O.max_points_per_node(cap):
        want = O.build_closed(0.001, bmin, bmax, x, y, z, rgb, threads=8)
    t = ctx.build(0.001, pcv.Aabb(bmin, bmax), x, y, z, rgb, max_points_per_node=cap, single_chain=True, check_resolve=True)
    info = t.build_info()
    assert_same(t.to_dict(), want)
    assert info["single_chain"] and info["replayed_points"] >= 6 * k, info


def test_many_small_leaves_take_8_bit_digits_and_the_global_rank_map(ctx):
    """28 000 leaves: the record sort runs two 8-bit passes (256 digit values: the wide digit state of the 12-byte
    downsweep), the predicted tree has more nodes than the rank map's LDS copy holds (the first upsweep then reads the
    map from memory) and more than the device-side resolve keeps in LDS — the geometry a 1 B-point build has, at test
    size. (A capacity of 150 would push the predicted tree's bound past the 24 rank bits of the packed key: that build
    takes the 20-byte records and is byte-exact as well.)"""
    n, cap = 2_000_000, 250
    x, y, z, rgb, bmin, bmax = synthetic.gaussian_clusters(n, seed=31, num_clusters=9, extent=250.0, sigma_range=(0.3, 7.0))
    with O.max_points_per_node(cap):
        want = O.build_closed(0.001, bmin, bmax, x, y, z, rgb, threads=8)
    leaves = len(want.nodes) - len({k[:-1] for k in want.nodes if len(k) > 1})  # nodes that are nobody's parent
    assert 16_384 < leaves <= 65_536, leaves  # 15 or 16 rank bits -> two passes of 8
    t = ctx.build(0.001, pcv.Aabb(bmin, bmax), x, y, z, rgb, max_points_per_node=cap, single_chain=True, check_resolve=True)
    info = t.build_info()
    assert_same(t.to_dict(), want)
    assert info["single_chain"] and info["record_bytes"] == 12 and info["predicted_nodes"] > 15_360, info
    t.free()
    t = ctx.build(0.001, pcv.Aabb(bmin, bmax), x[:1_200_000], y[:1_200_000], z[:1_200_000], rgb[:1_200_000], max_points_per_node=90,
                  single_chain=True, check_resolve=True)
    with O.max_points_per_node(90):
        want = O.build_closed(0.001, bmin, bmax, x[:1_200_000], y[:1_200_000], z[:1_200_000], rgb[:1_200_000], threads=8)
    assert_same(t.to_dict(), want)
    assert t.build_info()["record_bytes"] == 20, t.build_info()  # the predicted tree could outgrow 24 rank bits


@pytest.mark.parametrize("n,cap,lo,hi", [(2_000_000, 250, 16_384, 65_536),   # 8-bit digits, the rank map gathered from global memory
                                         (1_500_000, 1_500, 1_024, 8_192),   # <= 7-bit digits, the map's half-word copy in LDS beside the plane
                                         (1_500_000, 420, 5_000, 16_384)])   # two passes from the rows, map bigger than the LDS left beside the plane
def test_intensity_plane_rides_the_12_byte_record_sort(ctx, n, cap, lo, hi):
    """The reference binary always builds ["color", "intensity"] (src/bin/build_octree.rs:47-52): the f32 plane travels with
    the 12-byte records through the SAME two downsweeps (downsweep_rec12_kernel<..., PL = true>, histograms from the rank
    counts) — in every map placement the kernel has. `.intensity` bytes checked like `.xyz` / `.rgb` (raw.rs:374-392)."""
    x, y, z, rgb, bmin, bmax = synthetic.gaussian_clusters(n, seed=33, num_clusters=9, extent=250.0, sigma_range=(0.3, 7.0))
    inten = ((np.arange(n, dtype=np.int64) * 2654435761) % 100_003).astype(np.float32) * 0.25 - 7.0
    with O.max_points_per_node(cap):
        want = O.build_closed(0.001, bmin, bmax, x, y, z, rgb, inten, threads=8)
    leaves = len(want.nodes) - len({k[:-1] for k in want.nodes if len(k) > 1})
    assert lo < leaves <= hi, leaves
    t = ctx.build(0.001, pcv.Aabb(bmin, bmax), x, y, z, rgb, inten, max_points_per_node=cap, single_chain=True, check_resolve=True)
    info = t.build_info()
    assert info["single_chain"] and info["record_bytes"] == 12, info
    assert_same(t.to_dict(), want, check_intensity=True)
    t.free()


@pytest.mark.parametrize("n,cap,lo,hi", [(1_500_000, 1_500, 1_024, 8_192),    # two passes of <= 7 bits: 128 digit values in the settling pass
                                         (1_500_000, 800, 4_000, 16_384),     # 14 rank bits
                                         (300_000_000, 55_000, 16_384, 32_768),   # 15 rank bits (8 + 7): clouds of >= 200 M points only
                                         (520_000_000, 55_000, 32_768, 65_536)])  # 16 rank bits (8 + 8, 256 digit values): >= 500 M points
def test_second_sort_pass_settles_the_leaves(ctx, n, cap, lo, hi):
    """Colour-only single-chain builds: the record sort's second pass writes the final bytes of the integer-coded leaves itself
    (downsweep_settle_kernel: the rewrite of generation.rs:222-238 and the node-contiguous layout of raw.rs:361-450) and the
    climber records of their every-8th points; the settle kernel only sees the leaves left over (Float32-coded ones, chains
    to continue). Same bytes as the oracle; build_info says how many points went that way."""
    if n > 10_000_000:  # the 15-bit geometry needs a cloud whose sort scratch holds 2^15 counters per workgroup: device-side cloud
        import torch
        import bench
        import os
        # tens of GB of device memory and the experiment library (the reference build runs with the pass switched off): skipped,
        # not failed, on a smaller or shared GPU. The geometries themselves are checked against the ORACLE at a size
        # it can handle by test_wide_rank_geometries_against_the_oracle below.
        free_b, _ = torch.cuda.mem_get_info(0)
        if free_b < 110 * n + (8 << 30):
            pytest.skip(f"needs ~{(110 * n) >> 30} GiB of free device memory, {free_b >> 30} GiB there")
        if not os.path.exists(os.path.join(os.path.dirname(pcv._lib.LIB_PATH), "libpcv_hip_exp.so")):
            pytest.skip("libpcv_hip_exp.so (make -C point_cloud_viewer_amd/csrc) is not built")
        dev = torch.device("cuda", 0)
        x, y, z, rgb = bench.make_cloud(torch, n, seed=5, device=dev, clusters=40, extent=300.0, sigma=(0.5, 9.0))
        t = ctx.build(0.001, None, x, y, z, rgb, max_points_per_node=cap, single_chain=True, check_resolve=True)
        info = t.build_info()
        leaves = info["predicted_leaves"]
        assert lo < leaves <= hi, info
        assert info["settled_in_sort"] > 0.5 * n, info
        # no oracle at this size inside a unit test: the same build with the pass switched off is the reference (digest of every byte)
        d1 = bench.digest_of_digests(bench.tree_digests(t))
        t.free()
        import os, subprocess, sys
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        code = ("import sys; sys.path.insert(0, sys.argv[1]); import torch, bench, point_cloud_viewer_amd as pcv\n"
                "dev = torch.device('cuda', 0); ctx = pcv.Context(0)\n"
                f"x, y, z, rgb = bench.make_cloud(torch, {n}, seed=5, device=dev, clusters=40, extent=300.0, sigma=(0.5, 9.0))\n"
                f"t = ctx.build(0.001, None, x, y, z, rgb, max_points_per_node={cap}, single_chain=True, check_resolve=True)\n"
                "assert t.build_info()['settled_in_sort'] == 0\nprint('digest', bench.digest_of_digests(bench.tree_digests(t)))\n")
        del x, y, z, rgb
        torch.cuda.empty_cache()
        out = subprocess.run([sys.executable, "-c", code, root], env=dict(os.environ, PCV_HIP_LIBRARY="exp", PCV_SETTLE_IN_SORT="0"),
                             capture_output=True, text=True, timeout=900)
        assert out.returncode == 0 and f"digest {d1}" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]
        return
    x, y, z, rgb, bmin, bmax = synthetic.gaussian_clusters(n, seed=33, num_clusters=9, extent=250.0, sigma_range=(0.3, 7.0))
    with O.max_points_per_node(cap):
        want = O.build_closed(0.001, bmin, bmax, x, y, z, rgb, threads=8)
    leaves = len(want.nodes) - len({k[:-1] for k in want.nodes if len(k) > 1})
    assert lo < leaves <= hi, leaves
    for bbox in (pcv.Aabb(bmin, bmax), None):
        t = ctx.build(0.001, bbox, x, y, z, rgb, max_points_per_node=cap, single_chain=True, check_resolve=True)
        info = t.build_info()
        assert info["single_chain"] and info["record_bytes"] == 12 and info["settled_in_sort"] > 0.5 * n, info
        if bbox is not None:
            assert_same(t.to_dict(), want)
        t.free()
    # the reference binary's payload (src/bin/build_octree.rs:47-52): the intensity plane goes through the settling pass too
    # (downsweep_settle_kernel<true>: 4 bytes per point into .intensity, 32-byte climber records)
    inten = ((np.arange(n, dtype=np.int64) * 2654435761) % 100_003).astype(np.float32) * 0.25 - 7.0
    with O.max_points_per_node(cap):
        want = O.build_closed(0.001, bmin, bmax, x, y, z, rgb, inten, threads=8)
    t = ctx.build(0.001, pcv.Aabb(bmin, bmax), x, y, z, rgb, inten, max_points_per_node=cap, single_chain=True, check_resolve=True)
    info = t.build_info()
    assert info["single_chain"] and info["record_bytes"] == 12 and info["settled_in_sort"] > 0.5 * n, info
    assert_same(t.to_dict(), want, check_intensity=True)
    t.free()


@pytest.mark.parametrize("n,cap,bins,lo,hi", [(8_000_000, 2_500, 32768, 16_384, 32_768),   # ranks of 15 bits: 8 + 7, 128 digit values in the settling pass
                                             (8_000_000, 1_300, 65536, 32_768, 65_536)])    # ranks of 16 bits: 8 + 8, downsweep_settle_kernel<false, 1024, 256>
def test_wide_rank_geometries_against_the_oracle(n, cap, bins, lo, hi):
    """The 15- and 16-bit rank geometries of the settling pass are taken from 200 M / 500 M points on (their counters need 128 /
    256 MB of sort scratch), where a unit test has no oracle. The experiment library can be told to take them on a small cloud
    (PCV_ROWS_TRUE_BINS): the same kernels, checked here against the CPU oracle byte for byte. (n / cap <= 13 107
    keeps the predicted-tree capacity inside the 24 rank bits of a 12-byte record.)"""
    import json
    import os
    import subprocess
    import sys
    import bench
    if not os.path.exists(os.path.join(os.path.dirname(pcv._lib.LIB_PATH), "libpcv_hip_exp.so")):
        pytest.skip("libpcv_hip_exp.so (make -C point_cloud_viewer_amd/csrc) is not built")
    x, y, z, rgb, bmin, bmax = synthetic.gaussian_clusters(n, seed=91, num_clusters=12, extent=300.0, sigma_range=(0.3, 8.0))
    with O.max_points_per_node(cap):
        want, _ = O.build_closed_digests(0.001, bmin, bmax, x, y, z, rgb, threads=8)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys, json; sys.path.insert(0, sys.argv[1]); import bench, point_cloud_viewer_amd as pcv\n"
            "from point_cloud_viewer_amd import synthetic\n"
            f"x, y, z, rgb, bmin, bmax = synthetic.gaussian_clusters({n}, seed=91, num_clusters=12, extent=300.0, sigma_range=(0.3, 8.0))\n"
            f"t = pcv.Context(0).build(0.001, pcv.Aabb(bmin, bmax), x, y, z, rgb, max_points_per_node={cap}, single_chain=True, check_resolve=True)\n"
            "print('RESULT ' + json.dumps({'info': t.build_info(), 'digests': bench.tree_digests(t)}))\n")
    out = subprocess.run([sys.executable, "-c", code, root], env=dict(os.environ, PCV_HIP_LIBRARY="exp", PCV_ROWS_TRUE_BINS=str(bins)),
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    res = json.loads(next(line for line in out.stdout.splitlines() if line.startswith("RESULT "))[7:])
    info = res["info"]
    # the width of the rank follows the PREDICTED leaves (an upper bound of the true ones)
    assert lo < info["predicted_leaves"] <= hi, info
    assert info["single_chain"] and info["record_bytes"] == 12 and info["settled_in_sort"] > 0.5 * n, info
    got = {k: tuple(v) for k, v in res["digests"].items()}
    cmp_ = bench.compare_digests({k: tuple(v) for k, v in want.items()}, got)
    assert cmp_["ok"], cmp_


def test_single_chain_is_the_default_from_4M_points_and_keeps_candidate_codes(ctx):
    n = 6_000_000
    x, y, z, rgb, bmin, bmax = synthetic.gaussian_clusters(n, seed=8, num_clusters=24, extent=500.0, sigma_range=(0.3, 9.0))
    t = ctx.build(0.001, pcv.Aabb(bmin, bmax), x, y, z, rgb, stage_times=True)
    info = t.build_info()
    assert info["single_chain"] and info["attempts"] == 0, info
    assert info["kept_code_points"] > 0, info  # some node sat in the band and turned out to be a leaf
    assert info["continued_points"] > 0, info  # and some node in the band was split: its points continued their chain
    assert_same(t.to_dict(), O.build_closed(0.001, bmin, bmax, x, y, z, rgb, threads=8))
    st = t.stage_ms()
    assert st["sort_keys"] == 0.0 and st["leaf_encode"] > 0.0  # no key sort of the full input on this path


def test_single_chain_with_computed_bbox_device_inputs_and_rgba(ctx):
    import torch
    n = 5_000_000
    x, y, z, rgb, bmin, bmax = synthetic.gaussian_clusters(n, seed=9, num_clusters=10, extent=250.0, sigma_range=(0.2, 7.0))
    rgba = np.concatenate([rgb, np.full((n, 1), 9, np.uint8)], axis=1)
    dev = torch.device("cuda", 0)
    dx, dy, dz = (torch.from_numpy(a).to(dev) for a in (x, y, z))
    dc = torch.from_numpy(rgba).to(dev)
    torch.cuda.synchronize()
    t = ctx.build(0.001, None, dx, dy, dz, dc)
    assert t.build_info()["single_chain"]
    m = t.meta()
    assert np.array_equal(m["bbox_min"], bmin) and np.array_equal(m["bbox_max"], bmax)
    assert_same(t.to_dict(), O.build_closed(0.001, bmin, bmax, x, y, z, rgb, threads=8))


def test_duplicates_and_resolution_limited_nodes(ctx):
    rng = np.random.default_rng(11)
    n = 700_000
    x, y, z = rng.uniform(-30, 30, n), rng.uniform(-30, 30, n), rng.uniform(-3, 3, n)
    x[: n // 3], y[: n // 3], z[: n // 3] = 1.25, -7.5, 0.5  # a third of the cloud is ONE point
    perm = rng.permutation(n)
    x, y, z = x[perm], y[perm], z[perm]
    rgb = synthetic.index_colors(n)
    bmin, bmax = np.array([-30.0, -30, -3]), np.array([30.0, 30, 3])
    with O.max_points_per_node(10_000):
        want = O.build_closed(0.01, bmin, bmax, x, y, z, rgb, threads=8)
    t = ctx.build(0.01, pcv.Aabb(bmin, bmax), x, y, z, rgb, max_points_per_node=10_000, single_chain=True, check_resolve=True)
    assert_same(t.to_dict(), want)


def test_two_step_build_with_forced_level1_split(ctx):
    """pcv_build_begin / pcv_build_finish (the multi-GPU halves) through the single-chain path, incl. a forced split of
    level-1 nodes that hold few points."""
    import torch
    n = 5_000_000
    x, y, z, rgb, bmin, bmax = synthetic.gaussian_clusters(n, seed=12, num_clusters=8, extent=400.0, sigma_range=(0.3, 8.0))
    dev = torch.device("cuda", 0)
    dx, dy, dz = (torch.from_numpy(a).to(dev) for a in (x, y, z))
    dc = torch.from_numpy(rgb).to(dev)
    torch.cuda.synchronize()
    pend = ctx.build_begin(0.001, pcv.Aabb(bmin, bmax), dx, dy, dz, dc, force_split_level1=0xff)
    l1, l2, mask = pend.top_streams()
    tree = pend.finish(None)
    assert tree.build_info()["single_chain"]
    want, streams = O.build_closed_shard(0.001, bmin, bmax, x, y, z, rgb, threads=8, force_mask=0xff)
    assert np.array_equal(l1, streams[:8].astype(np.int64)) and np.array_equal(l2, streams[8:72].astype(np.int64))
    assert mask == int(streams[72])
    assert_same(tree.to_dict(), want)


def test_back_to_back_builds_are_identical_and_survive_interleaved_queries(ctx):
    """The single-chain build forks small copies onto a side stream, queues its record sort before the host has built
    the node tables and keeps those tables in a context-owned block: repeated builds of alternating sizes on ONE context,
    with queries on the trees that are still alive in between, must give the same bytes every time."""
    import hashlib

    def digest(t):
        h = hashlib.blake2b(digest_size=16)
        for name, nd in sorted(t.to_dict().items()):
            h.update(name.encode())
            h.update(nd["xyz"])
            h.update(nd["rgb"])
        return h.hexdigest()

    clouds = []
    for n, seed in ((700_000, 21), (2_300_000, 22)):
        x, y, z, rgb, bmin, bmax = synthetic.gaussian_clusters(n, seed=seed, num_clusters=7, extent=250.0, sigma_range=(0.1, 9.0))
        clouds.append((x, y, z, rgb, bmin, bmax))
    first, alive = {}, []
    for it in range(8):
        k = it % 2
        x, y, z, rgb, bmin, bmax = clouds[k]
        t = ctx.build(0.001, None if it % 3 == 0 else pcv.Aabb(bmin, bmax), x, y, z, rgb, max_points_per_node=25_000,
                      single_chain=True, check_resolve=True)
        d = digest(t)
        assert first.setdefault(k, d) == d, it
        alive.append((t, bmin, bmax))
        if len(alive) > 2:
            alive.pop(0)[0].free()
        for tr, lo, hi in alive:  # a point query on every tree that is still alive: a box around everything, half of it
            shapes = ctx.shapes([("aabb", lo - 1.0, hi + 1.0), ("aabb", lo - 1.0, (lo + hi) / 2)])
            assert tr.query_points(shapes, 0, capacity=1)["count"] == tr.num_points
            assert tr.query_points(shapes, 1, capacity=1)["count"] < tr.num_points
    for t, _, _ in alive:
        t.free()


_ALT_PATH_SCRIPT = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import numpy as np
import oracle_lib as O
import point_cloud_viewer_amd as pcv
from point_cloud_viewer_amd import synthetic
from test_gpu_build import assert_same
want_bytes = int(sys.argv[2])
ctx = pcv.Context(0)
for n, cap, res, clusters, extent, sigma, with_int, seed in ((600_000, 20_000, 0.001, 6, 200.0, (0.2, 8.0), True, 2),
                                                              (600_000, 20_000, 0.0001, 6, 200.0, (0.2, 8.0), False, 21),
                                                              # >= 2^20 points: the depth-binned chain pass (a last tile of 544)
                                                              (1_300_000, 30_000, 0.0002, 7, 220.0, (0.1, 7.0), True, 7)):
    x, y, z, rgb, bmin, bmax = synthetic.gaussian_clusters(n, seed=seed, num_clusters=clusters, extent=extent, sigma_range=sigma)
    inten = (np.arange(n) % 509).astype(np.float32) * 0.5 if with_int else None
    with O.max_points_per_node(cap):
        want = O.build_closed(res, bmin, bmax, x, y, z, rgb, inten, threads=8)
    t = ctx.build(res, pcv.Aabb(bmin, bmax), x, y, z, rgb, inten, max_points_per_node=cap, single_chain=True, check_resolve=True)
    info = t.build_info()
    assert info["single_chain"] and info["record_bytes"] == want_bytes, info
    assert_same(t.to_dict(), want, check_intensity=with_int)
print("alt-path ok")
"""


@pytest.mark.parametrize("env,record_bytes", [({"PCV_COMPACT_RECORDS": "0"}, 20), ({"PCV_SETTLE_BY_LEAF": "0"}, 12),
                                              ({"PCV_COMPACT_RECORDS": "0", "PCV_SETTLE_BY_LEAF": "0"}, 20),
                                              # the first sort pass counting and mapping the keys in a pass of its own (what
                                              # trees of more than 16 384 predicted nodes took before round 4)
                                              ({"PCV_SORT_ROWS": "0"}, 12),
                                              # the second pass counting its keys itself (equal chunks instead of pieces of
                                              # whole first-pass runs)
                                              ({"PCV_SORT_ROWS2": "0"}, 12),
                                              # the shipped chain kernel with every Float32-coded level step taken in full; with
                                              # the colour joined by the record sort's first pass instead (round 6, measured, dropped)
                                              ({"PCV_CODE_STEPS": "0"}, 12), ({"PCV_COLOR_LATE": "1"}, 12),
                                              # the write-combining form of the record downsweep, both passes (experiment)
                                              ({"PCV_REC_WC": "3"}, 12),
                                              # the record sort's upper digit first, the second pass inside every bucket (experiment)
                                              ({"PCV_SORT_MSD": "1"}, 12),
                                              # the record sort running to its end on its own, every leaf finished by the settle kernel
                                              ({"PCV_SETTLE_IN_SORT": "0"}, 12),
                                              # the sample tree by counting the keys instead of from sorted keys (experiment, slower)
                                              ({"PCV_SAMPLE_COUNTS": "1"}, 12),
                                              # the sample tree split one level per launch pair (what u32 keys and levels
                                              # beyond the first key word still take)
                                              ({"PCV_SPLIT2": "0"}, 12)])
def test_alternative_kernels_behind_the_switches_are_byte_exact_too(env, record_bytes):
    """The 20-byte record format (what a predicted tree of more than 2^24 nodes falls back to) and the slot-wise settle
    kernel are selected by switches that are read once per process: run them in a child process against the oracle."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    # the switches only exist in the experiment build of the library (libpcv_hip_exp.so, -DPCV_EXPERIMENTS)
    out = subprocess.run([sys.executable, "-c", _ALT_PATH_SCRIPT, root, str(record_bytes)],
                         env=dict(os.environ, PCV_HIP_LIBRARY="exp", **env),
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "alt-path ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
