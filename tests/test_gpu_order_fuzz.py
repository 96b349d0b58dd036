"""The octree builds over input ORDER (tests/order_cases.py), byte for byte against the CPU oracle: coherent orders (Morton, its
reverse, scan lines, submaps), periodic ones (Morton blocks of one wave / one chain-pass tile / a few tiles, shuffled, and the
same one point off) and clouds constructed around the sample so that the prediction MUST fail. The reference's inputs are
spatially coherent and the oracle is stable, so it is the truth for every order (src/octree/generation.rs:289-403 has one
answer per input AND order: which points climb is decided by the order inside each leaf, generation.rs:222-238). What each
case expects of the prediction comes from the host logic on the CPU (order_cases.PREDICTED, tests/test_order_cases_cpu.py),
not from the build under test."""
import numpy as np
import pytest

import oracle_lib as O
import order_cases as OC
import point_cloud_viewer_amd as pcv
from test_gpu_build import assert_same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = pcv.Context(0)
    yield c
    c.close()


SEEN = {"held": 0, "fell_back": 0, "kept": 0, "continued": 0, "replayed": 0, "settled_b": 0, "gave_up_pool": 0}
_oracle = {}


def _want(key, cloud):
    if key not in _oracle:
        _oracle[key] = cloud.oracle()
    return _oracle[key]


def _build(ctx, cl, single_chain, bbox=True):
    return ctx.build(cl.res, pcv.Aabb(cl.bmin, cl.bmax) if bbox else None, cl.x, cl.y, cl.z, cl.rgb, cl.inten,
                     max_points_per_node=cl.cap, single_chain=single_chain, check_resolve=bool(single_chain))


def _count(info):
    SEEN["held" if info["single_chain"] else "fell_back"] += 1
    SEEN["kept"] += info["kept_code_points"] > 0
    SEEN["replayed"] += info["replayed_points"] > 0
    SEEN["continued"] += info["continued_points"] > 0


@pytest.mark.parametrize("order", OC.ORDERED)
@pytest.mark.parametrize("cloud", list(OC.BASE))
def test_ordered_build_equals_oracle(ctx, cloud, order):
    """Base clouds (a) few leaves, one sort pass, (b) the settling second pass with the intensity plane and the climber records
    (downsweep_settle_kernel, csrc/pcv_sort_rec12.hip), (c) the depth-binned chain pass with wide records through the Float32
    pool and a last tile of 544 (chain_pass_kernel, csrc/pcv_encode.hip) — in every order: the sample's clumps see eight
    copies of one place (sample_round, csrc/pcv_single_chain.hip), a tile's deal has one or two depth classes, one wave's pool
    reservation takes 64 entries at once, a sort chunk falls into one or two leaves (rank_hist_rows and both record-sort
    passes, csrc/pcv_sort_rec12.hip), and the every-8th promotion follows the order inside each leaf. Through the exact
    pipeline and the forced single-chain build; the prediction holds where the host logic says it does."""
    cl = OC.base_cloud(cloud).ordered(order)
    want = cl.oracle()
    t = _build(ctx, cl, True)
    info = t.build_info()
    print(cloud, order, info)
    assert_same(t.to_dict(), want, check_intensity=cl.inten is not None)
    t.free()
    _count(info)
    if cloud == "b":
        SEEN["settled_b"] += info["settled_in_sort"] > 0
    # a case the CPU predicted to hold that falls back on the device (or the reverse) is a finding, not a number to relax
    assert info["single_chain"] == (OC.PREDICTED[(cloud, order)] == OC.HELD), info
    assert info["attempts"] in (0, 2, 3), info
    t = _build(ctx, cl, False)
    assert t.build_info()["attempts"] >= 1
    assert_same(t.to_dict(), want, check_intensity=cl.inten is not None)
    t.free()


def _context_is_clean(ctx):
    """After a dropped attempt (PcvBuild::drop_single_chain, csrc/pcv_build_state.h: buffers freed behind queued work, keys_a /
    keys_b reused by the exact pipeline) the SAME context builds base cloud (a) through the single-chain path and answers a
    query over everything."""
    cl = OC.base_cloud("a")
    t = _build(ctx, cl, True)
    info = t.build_info()
    assert_same(t.to_dict(), _want("a", cl))
    assert info["single_chain"], info
    shapes = ctx.shapes([("aabb", cl.bmin - 1.0, cl.bmax + 1.0)])
    assert t.query_points(shapes, 0, capacity=1)["count"] == t.num_points == cl.n
    t.free()


@pytest.mark.parametrize("name", ["starved", "starved_settling"])
def test_a_starved_sample_sends_the_build_to_the_exact_pipeline(ctx, name):
    """OC.starved / OC.starved_settling: 30 000 tight points only where the sample never reads, so a predicted leaf holds more
    than the capacity: pcv_spec_resolve says PCV_SPEC_TOO_SHALLOW in settle_verdict (csrc/pcv_single_chain.hip) AFTER
    count_and_queue_sort has queued the record sort, and PcvBuild::drop_single_chain (csrc/pcv_build_state.h) frees the
    attempt's buffers behind that work before the exact pipeline reuses keys_a / keys_b. `starved`: one sort pass.
    `starved_settling`: two passes, the second held back (sort_second.pending -> the join_side branch). Byte-exact, fallen back
    (attempts 2, or 3 with the exact pipeline's own retry), and the context is clean afterwards."""
    cl = OC.CONSTRUCTED[name]()
    want = cl.oracle()
    t = _build(ctx, cl, True)
    info = t.build_info()
    print(name, info)
    assert_same(t.to_dict(), want)
    t.free()
    _count(info)
    assert OC.PREDICTED[(name, None)] == OC.SHALLOW
    assert not info["single_chain"] and info["attempts"] in (2, 3), info
    _context_is_clean(ctx)
    t = _build(ctx, cl, False)
    assert_same(t.to_dict(), want)
    t.free()


def test_a_full_pool_region_leaves_no_room_for_the_replay(ctx):
    """OC.pool_tops: the oversampled clusters replay their chain, and at resolution 0.0001 every leaf level is Float32-coded, so
    every point of a full 1 024-point input slice took an entry of its pool region in the chain pass: the region is full to
    pool_cap = 1 024 (pcv_pool_region_entries, csrc/pcv_internal.h) and `most + ceil(replay_slots / 1 024) > pool_cap` in
    settle_verdict (csrc/pcv_single_chain.hip) gives the build to the exact pipeline — the second give-up, also through
    PcvBuild::drop_single_chain. The host logic itself holds (OC.PREDICTED), so attempts >= 2 here can only be that line.
    Confirmed on the device: attempts == 2 at 0.1 mm, while the same cloud at 1 mm holds and replays 60 286 points."""
    cl = OC.pool_tops()
    want = cl.oracle()
    t = _build(ctx, cl, True)
    info = t.build_info()
    print("pool_tops", info)
    assert_same(t.to_dict(), want)
    t.free()
    _count(info)
    assert OC.PREDICTED[("pool_tops", None)] == OC.HELD
    assert not info["single_chain"] and info["attempts"] in (2, 3), info
    SEEN["gave_up_pool"] += 1
    _context_is_clean(ctx)
    # the same cloud at 1 mm (level 2 is u16-coded: few pool entries) holds and replays: the give-up above is the pool's
    cl3 = OC.pool_tops(0.001)
    t = _build(ctx, cl3, True)
    info = t.build_info()
    assert_same(t.to_dict(), cl3.oracle())
    assert info["single_chain"] and info["replayed_points"] >= 6 * 700, info
    t.free()
    _count(info)


def test_tiles_of_one_depth_class(ctx):
    """OC.one_class_tiles in Morton order: hundreds of whole 1 024-point tiles whose points all have ONE predicted depth (the
    tight cluster: "deeper than the grid"; the background: level 2), so the deal of chain_pass_kernel (csrc/pcv_encode.hip:
    kcnt[], one returning LDS atomic per point) hands every slot of the tile to one class and the scan over the classes has
    a single non-zero entry; >= 2^20 points so that the depth grid is used at all, a last tile of 544."""
    cl = OC.one_class_tiles()
    want = cl.oracle()
    t = _build(ctx, cl, True)
    info = t.build_info()
    print("one_class_tiles", info)
    assert_same(t.to_dict(), want)
    t.free()
    _count(info)
    assert info["single_chain"], info
    t = _build(ctx, cl, False)
    assert_same(t.to_dict(), want)
    t.free()


def test_computed_bbox_over_monotone_coordinates(ctx):
    """bbox=None: the box pass (aabb_partial_kernel / aabb_final_kernel, csrc/pcv_chain.hip) reduces coordinates that arrive in Morton order —
    the extremes sit in the first and last workgroups — and the build on that box is the oracle's on the exact min / max."""
    base = OC.base_cloud("a")
    cl = base.ordered("morton")
    assert np.array_equal(cl.bmin, [cl.x.min(), cl.y.min(), cl.z.min()]) and np.array_equal(cl.bmax, [cl.x.max(), cl.y.max(), cl.z.max()])
    want = cl.oracle()
    for single_chain in (True, False):
        t = _build(ctx, cl, single_chain, bbox=False)
        m = t.meta()
        assert np.array_equal(m["bbox_min"], cl.bmin) and np.array_equal(m["bbox_max"], cl.bmax)
        assert_same(t.to_dict(), want)
        t.free()


def test_sharded_build_of_a_morton_ordered_cloud(tmp_path):
    """The cloud of test_virtual_ranks_on_one_gpu (tests/test_gpu_sharded.py) at world 4, capacity 20 000, in Morton order: every
    4 096-point routing tile goes to one or two buckets (route_octants_kernel / route_scatter_kernel, csrc/pcv_chain.hip: a
    tile histogram with one or two non-zero rows) and every rank holds one contiguous slice of space, so ranks
    send nearly all they have to one owner."""
    import torch
    from point_cloud_viewer_amd import distributed as pdist, synthetic
    from test_gpu_sharded import _same
    from thread_dist import run_ranks
    world, cap, n = 4, 20_000, 400_000
    x, y, z, rgb, bmin, bmax = synthetic.gaussian_clusters(n, seed=29, num_clusters=7, extent=300.0, sigma_range=(0.02, 5.0))
    perm = OC.morton(x, y, z, bmin, bmax)
    x, y, z, rgb = x[perm], y[perm], z[perm], np.ascontiguousarray(rgb[perm])
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream

    def rank_main(rank, dist):
        torch.cuda.set_device(0)
        ctx = pcv.Context(0, stream=stream)
        sl = slice(rank * n // world, (rank + 1) * n // world)
        tx, ty, tz = (torch.from_numpy(np.ascontiguousarray(a[sl])).cuda() for a in (x, y, z))
        trgb = torch.from_numpy(np.ascontiguousarray(rgb[sl])).cuda()
        b = pdist.ShardedOctreeBuilder(ctx, dist, dev)
        bbox = b.global_bbox(tx, ty, tz)
        assert np.array_equal(bbox.min, bmin) and np.array_equal(bbox.max, bmax)
        res = b.build(0.001, bbox, tx, ty, tz, trgb, max_points_per_node=cap)
        return res.gather(0), res.plan

    out = run_ranks(world, rank_main)
    merged, (rank_of, split_mask) = out[0]
    with O.max_points_per_node(cap):
        want = O.build_closed(0.001, bmin, bmax, x, y, z, rgb, threads=4)
    _same(merged, want)
    assert split_mask != 0 and len(set(rank_of.tolist())) == world


def test_the_cases_above_covered_every_branch():
    """Across this file: the prediction held, fell back for BOTH reasons (too shallow: the starved clouds; the pool's tops:
    pool_tops), kept a candidate's codes, continued chains, replayed chains, and the record sort's second pass settled leaves in an ordered
    case of base cloud (b)."""
    assert SEEN["held"] >= 3 and SEEN["fell_back"] >= 2 and SEEN["kept"] > 0 and SEEN["continued"] > 0, SEEN
    assert SEEN["settled_b"] > 0 and SEEN["gave_up_pool"] == 1 and SEEN["replayed"] > 0, SEEN
