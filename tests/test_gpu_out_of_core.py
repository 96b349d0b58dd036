"""Out-of-core build (pcv_ooc_*): a stream of PointsBatches goes through the device into host spills and is built partition by
partition into the reference's directory. Every directory must equal the in-core build of the same cloud byte for byte — every
node file and meta.pb — whatever the partitioning, the spill form (level-1 chain state or raw planes) and the batch sizes."""
import os

import numpy as np
import pytest

import oracle_lib as O
import point_cloud_viewer_amd as pcv
from point_cloud_viewer_amd import synthetic

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    c = pcv.Context(0)
    yield c
    c.close()


def batches(x, y, z, rgb, inten, batch=500_000):
    pos = np.stack([x, y, z], axis=1)
    for at in range(0, x.size, batch):  # the last batch is ragged
        yield dict(position=pos[at:at + batch], color=rgb[at:at + batch], intensity=None if inten is None else inten[at:at + batch])


def read_dir(path):
    return {name: open(os.path.join(path, name), "rb").read() for name in sorted(os.listdir(path))}


def same_dir(a, b, skip_meta=False):
    da, db = read_dir(a), read_dir(b)
    assert sorted(da) == sorted(db), sorted(set(da) ^ set(db))[:10]
    for name in da:
        if skip_meta and name == "meta.pb":
            continue
        assert da[name] == db[name], name
    return len(da)


def in_core(ctx, path, res, bmin, bmax, x, y, z, rgb, inten, cap):
    attrs = ("color", "intensity") if inten is not None else ("color",)
    tree = pcv.build_octree(str(path), res, pcv.Aabb(bmin, bmax), batches(x, y, z, rgb, inten), attributes=attrs, ctx=ctx,
                            max_points_per_node=cap)
    tree.free()


def out_of_core(ctx, path, res, bmin, bmax, x, y, z, rgb, inten, cap, per_pass, batch=500_000):
    attrs = ("color", "intensity") if inten is not None else ("color",)
    return pcv.build_octree(str(path), res, pcv.Aabb(bmin, bmax), batches(x, y, z, rgb, inten, batch), attributes=attrs, ctx=ctx,
                            max_points_per_node=cap, max_points_per_pass=per_pass)


@pytest.fixture(scope="module")
def cloud():
    n = 2_300_017
    x, y, z, rgb, bmin, bmax = synthetic.gaussian_clusters(n, seed=5, num_clusters=12, extent=300.0, sigma_range=(0.2, 9.0))
    inten = ((np.arange(n, dtype=np.int64) * 2654435761) % 100_003).astype(np.float32) * 0.25 - 7.0
    return x, y, z, rgb, inten, bmin, bmax


@pytest.mark.parametrize("with_intensity", [False, True])
def test_many_partitions_equal_the_in_core_build(ctx, cloud, tmp_path, with_intensity):
    x, y, z, rgb, inten, bmin, bmax = cloud
    inten = inten if with_intensity else None
    in_core(ctx, tmp_path / "in", 0.001, bmin, bmax, x, y, z, rgb, inten, 20_000)
    st = out_of_core(ctx, tmp_path / "ooc", 0.001, bmin, bmax, x, y, z, rgb, inten, 20_000, 500_000)
    assert st["partitions"] >= 4 and st["points"] == x.size and st["routed"] == 1, st
    files = same_dir(tmp_path / "ooc", tmp_path / "in")
    assert files > 20 and os.path.exists(tmp_path / "ooc" / "meta.pb")


def test_partition_count_does_not_change_the_directory(ctx, cloud, tmp_path):
    x, y, z, rgb, inten, bmin, bmax = cloud
    seen = []
    for per_pass in (0, 1_200_000, 400_000):
        st = out_of_core(ctx, tmp_path / f"p{per_pass}", 0.001, bmin, bmax, x, y, z, rgb, None, 20_000, per_pass)
        seen.append(st["partitions"])
        if per_pass:
            same_dir(tmp_path / f"p{per_pass}", tmp_path / "p0")
    assert seen[0] == 1 and seen[1] >= 2 and seen[2] > seen[1], seen


def test_equals_the_oracle_literal_directory(ctx, tmp_path):
    n = 700_003
    x, y, z, rgb, bmin, bmax = synthetic.gaussian_clusters(n, seed=71, num_clusters=5, extent=200.0, sigma_range=(0.1, 5.0))
    inten = np.linspace(-1.0, 250.0, n).astype(np.float32)
    st = out_of_core(ctx, tmp_path / "ooc", 0.001, bmin, bmax, x, y, z, rgb, inten, 0, 250_000, batch=100_000)
    assert st["partitions"] >= 3, st
    O.build_literal_dir(str(tmp_path / "want"), 0.001, bmin, bmax, x, y, z, rgb, inten, threads=8)
    # the reference writes the node list of meta.pb in a nondeterministic order
    assert same_dir(tmp_path / "ooc", tmp_path / "want", skip_meta=True) > 20


def test_raw_plane_spill_when_level1_is_not_float32(ctx, tmp_path):
    # a small cube at a coarse resolution: level 1 is integer-coded, the spill holds the raw planes
    n = 600_000
    x, y, z, rgb, bmin, bmax = synthetic.gaussian_clusters(n, seed=9, num_clusters=6, extent=20.0, sigma_range=(0.1, 2.0))
    res = 0.01
    _, _, enc = pcv.level_table(bmin, bmax, res)
    assert int(enc[1]) != 3
    in_core(ctx, tmp_path / "in", res, bmin, bmax, x, y, z, rgb, None, 5_000)
    st = out_of_core(ctx, tmp_path / "ooc", res, bmin, bmax, x, y, z, rgb, None, 5_000, 150_000)
    assert st["routed"] == 0 and st["partitions"] >= 4, st
    same_dir(tmp_path / "ooc", tmp_path / "in")


def test_duplicates_deep_tree_empty_buckets_unsplit_octant_and_small_partition(ctx, tmp_path):
    rng = np.random.default_rng(3)
    # octant 0: 3 000 points, fewer than max_points_per_node — its level-1 node is a leaf, kept whole, alone in the first partition;
    # octant 7: a heavy duplicate stack (its bucket goes below level 21, the second key word) over a uniform spread; the other
    # 48 buckets stay empty
    lone = rng.uniform(1.0, 9.0, (3_000, 3))
    dup = np.full((200_000, 3), 60.123456789)
    dup[::3] += rng.normal(0, 1e-7, (dup[::3].shape[0], 3))
    spread = rng.uniform(50.0, 100.0, (200_000, 3))
    pos = np.concatenate([lone, dup, spread])[rng.permutation(403_000)]
    x, y, z = (np.ascontiguousarray(pos[:, k]) for k in range(3))
    rgb = rng.integers(0, 256, (x.size, 3), dtype=np.uint8)
    bmin, bmax = np.zeros(3), np.full(3, 100.0)
    first = dup.shape[0] + int(np.all(spread < 75.0, axis=1).sum())  # bucket 56: the stack + its share of the spread
    in_core(ctx, tmp_path / "in", 1e-9, bmin, bmax, x, y, z, rgb, None, 4_000)
    st = out_of_core(ctx, tmp_path / "ooc", 1e-9, bmin, bmax, x, y, z, rgb, None, 4_000, first + 1_500)
    assert st["partitions"] == 3 and st["split_mask"] == 0x80 and st["routed"] == 0, st
    same_dir(tmp_path / "ooc", tmp_path / "in")
    names = read_dir(tmp_path / "ooc")
    assert any(len(k.split(".")[0]) > 23 for k in names), "the tree should reach below level 21"


@pytest.mark.parametrize("order", ["shuffled", "morton", "single"])
@pytest.mark.parametrize("routed", [True, False])
def test_bucket_runs_equal_route_buckets_and_are_stable(ctx, order, routed):
    import torch
    n = 300_001
    x, y, z, rgb, bmin, bmax = synthetic.gaussian_clusters(n, seed=17, num_clusters=8, extent=100.0, sigma_range=(0.5, 9.0))
    if order == "single":
        x, y, z = 80.0 + (x - bmin[0]) * 1e-3, 80.0 + (y - bmin[1]) * 1e-3, 80.0 + (z - bmin[2]) * 1e-3
    bbox = pcv.Aabb(bmin, bmax)
    dev = torch.device("cuda", 0)
    tx, ty, tz = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (x, y, z))
    bucket, counts, state = ctx.route_buckets(0.001, bbox, tx, ty, tz, torch.from_numpy(rgb).to(dev), with_state=True)
    b = bucket.cpu().numpy()
    if order == "morton":
        perm = np.argsort(b, kind="stable")
        x, y, z, rgb, b = x[perm], y[perm], z[perm], rgb[perm], b[perm]
        state = {k: v[torch.from_numpy(perm).to(dev)] for k, v in state.items()}
    if order == "single":
        assert np.unique(b).size == 1
    inten = np.arange(x.size, dtype=np.float32)
    xyz = torch.from_numpy(np.ascontiguousarray(np.stack([x, y, z], axis=1))).to(dev)
    planes, digits, got_counts = ctx.ooc_bucket_runs(0.001, bbox, xyz, torch.from_numpy(np.ascontiguousarray(rgb)).to(dev),
                                                     torch.from_numpy(inten).to(dev), routed=routed)
    assert np.array_equal(got_counts, np.bincount(b, minlength=64))
    order_idx = np.argsort(b, kind="stable")  # the stable 64-way partition
    assert np.array_equal(planes[4].cpu().numpy(), inten[order_idx])
    if routed:
        for k, name in enumerate(("cx", "cy", "cz", "oct_rgb")):
            assert np.array_equal(planes[k].cpu().numpy(), state[name].cpu().numpy()[order_idx]), name
    else:
        for k, a in enumerate((x, y, z)):
            assert np.array_equal(planes[k].cpu().numpy(), a[order_idx])
        assert np.array_equal(planes[3].cpu().numpy(), rgb[order_idx])
    # the level-2 digits of every octant's points, in input order, over the octant's range
    d = digits.cpu().numpy()
    oct_order = np.argsort(b >> 3, kind="stable")
    assert np.array_equal(d, (b & 7)[oct_order].astype(np.uint8))


def test_over_budget_bucket_and_abort_leave_the_context_usable(ctx, cloud, tmp_path):
    x, y, z, rgb, inten, bmin, bmax = cloud
    ooc = ctx.out_of_core(0.001, pcv.Aabb(bmin, bmax), False, 50_000, 20_000)
    for bt in batches(x, y, z, rgb, None):
        ooc.append(bt["position"], bt["color"])
    with pytest.raises(pcv.PcvError) as e:
        ooc.finish(str(tmp_path / "fail"))
    assert e.value.code == pcv.PCV_E_OOM and "bucket" in str(e.value) and "max_points_per_pass" in str(e.value)
    assert not os.path.exists(tmp_path / "fail" / "meta.pb")
    ooc = ctx.out_of_core(0.001, pcv.Aabb(bmin, bmax), True, 500_000, 20_000)
    bt = next(batches(x, y, z, rgb, inten))
    ooc.append(bt["position"], bt["color"], bt["intensity"])
    ooc.abort()
    # the context builds correctly afterwards, through an ingest (the ring) and out of core
    in_core(ctx, tmp_path / "in", 0.001, bmin, bmax, x, y, z, rgb, None, 20_000)
    st = out_of_core(ctx, tmp_path / "ooc", 0.001, bmin, bmax, x, y, z, rgb, None, 20_000, 700_000)
    same_dir(tmp_path / "ooc", tmp_path / "in")
    assert st["partitions"] >= 2


def test_compute_bbox_is_rejected(ctx):
    with pytest.raises(ValueError):
        ctx.out_of_core(0.001, None)


def test_c_example_writes_the_same_directory(ctx, tmp_path):
    import subprocess
    exe = os.path.join(ROOT, "examples", "bin", "ooc_batches")
    n = 900_001
    x, y, z, rgb, bmin, bmax = synthetic.gaussian_clusters(n, seed=29, num_clusters=4, extent=150.0, sigma_range=(0.1, 4.0))
    inten = np.linspace(0.0, 1.0, n).astype(np.float32)
    raw = tmp_path / "cloud.bin"
    with open(raw, "wb") as f:
        f.write(np.stack([x, y, z], axis=1).tobytes())
        f.write(rgb.tobytes())
        f.write(inten.tobytes())
    args = [exe, str(raw), str(n), str(tmp_path / "c_out"), "0.001", "20000", "300000"] + [repr(float(v)) for v in (*bmin, *bmax)]
    subprocess.check_call(args)
    in_core(ctx, tmp_path / "in", 0.001, bmin, bmax, x, y, z, rgb, inten, 20_000)
    same_dir(tmp_path / "c_out", tmp_path / "in")
