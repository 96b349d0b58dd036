"""The sharded build's kernels over the cases of tests/sharded_cases.py: the real ShardedOctreeBuilder + HipBackend, the ranks as
threads on one device (tests/thread_dist.py, as test_virtual_ranks_on_one_gpu sets them up), against ONE oracle build of the whole
cloud — pcv_route_plan / pcv_route_scatter / pcv_route_buckets / pcv_partition_by_owner on ragged, empty and unaligned rank slices,
pcv_build_begin and pcv_build_begin_routed with a forced level-1 split, pcv_build_finish under a global layout, the top-node merge,
for a level 1 that is u8, u16, Float32 or Float64 coded or cannot split. Contexts and builders live for the whole module, so every
case but the first of a (world, rank) runs on the device buffers an earlier, differently sized case left behind. No tolerance
anywhere: every comparison is byte equality."""
import os

import numpy as np
import pytest

import oracle_lib as O
import point_cloud_viewer_amd as pcv
import sharded_cases as SC
from point_cloud_viewer_amd import distributed as pdist

pytestmark = pytest.mark.gpu

TALLY = dict(cases=0, two_pass_ranks=0, one_pass_ranks=0, compressed_cases=0, raw_cases=0, split_cases=0, single_chain_true=0,
             single_chain_false=0, directories=0)


class CountingBackend(pdist.HipBackend):
    """HipBackend that notes which entry points a build went through."""

    def __init__(self, ctx, device):
        super().__init__(ctx, device)
        self.calls = []

    def buckets(self, resolution, bbox, x, y, z, rgb=None, with_state=False):
        self.calls.append("buckets_state" if with_state else "buckets")
        return super().buckets(resolution, bbox, x, y, z, rgb, with_state)

    def route_plan(self, resolution, bbox, x, y, z, octants_only=False):
        self.calls.append("route_plan")
        return super().route_plan(resolution, bbox, x, y, z, octants_only)

    def route_scatter(self, *args):
        self.calls.append("route_scatter")
        return super().route_scatter(*args)

    def partition(self, *args):
        self.calls.append("partition")
        return super().partition(*args)

    def build_begin(self, *args):
        self.calls.append("build_begin")
        return super().build_begin(*args)

    def build_begin_routed(self, *args):
        self.calls.append("build_begin_routed")
        return super().build_begin_routed(*args)


class Ranks:
    """One context per (world, rank) and one builder per (world, rank, compress, shard_mode), made on first use by the rank's thread
    and kept until the module ends."""

    def __init__(self):
        self.ctx, self.builders = {}, {}

    def builder(self, c, rank, dist, device, stream):
        ctx = self.ctx.get((c["world"], rank))
        if ctx is None:
            ctx = self.ctx[(c["world"], rank)] = pcv.Context(0, stream=stream)
        key = (c["world"], rank, c["compress"], c["shard_mode"])
        b = self.builders.get(key)
        if b is None:
            b = self.builders[key] = pdist.ShardedOctreeBuilder(ctx, dist, device, backend=CountingBackend(ctx, device),
                                                                compress_exchange=c["compress"], shard_mode=c["shard_mode"])
        b.dist = dist  # the rendezvous of this case's threads
        b.backend.calls = []
        return ctx, b

    def close(self):
        self.builders.clear()
        for ctx in self.ctx.values():
            ctx.close()
        self.ctx.clear()


@pytest.fixture(scope="module")
def ranks():
    r = Ranks()
    yield r
    r.close()


def run_case(ranks, c, directory=None):
    """Per rank: (merged on rank 0, exchange_info, send matrix, plan, backend calls, single_chain or None, pool bytes before and
    after)."""
    import torch
    from thread_dist import run_ranks
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    whole = SC.whole_tensors(c, dev)

    def rank_main(rank, dist):
        torch.cuda.set_device(0)
        ctx, b = ranks.builder(c, rank, dist, dev, stream)
        live_before = ctx.pool_stats()[0]
        x, y, z, rgb, inten = SC.rank_input(c, whole, rank)
        res = b.build(c["res"], pcv.Aabb(c["bmin"], c["bmax"]), x, y, z, rgb, inten, max_points_per_node=c["cap"])
        merged = res.gather(0)
        if directory is not None:
            res.write_dir(str(directory))
        single = res.local.build_info()["single_chain"] if res.num_nodes_local else None
        out = (merged, res.exchange_info(), res.counts, res.plan, list(b.backend.calls), single)
        res.free()
        del res
        return out + (live_before, ctx.pool_stats()[0])

    return run_ranks(c["world"], rank_main)


@pytest.mark.parametrize("case_id", SC.all_cases(), ids=str)
def test_sharded_build_on_the_device_equals_one_oracle_build(ranks, case_id, tmp_path):
    c, f = SC.get(case_id), SC.facts(case_id)
    with_dir = not isinstance(case_id, int) or case_id % 5 == 0
    out = run_case(ranks, c, tmp_path / "sharded" if with_dir else None)
    SC.assert_same_tree(out[0][0], SC.oracle_tree(case_id), c)
    SC.assert_exchange(c, f, [(o[1], o[2]) for o in out])
    lengths = np.diff(c["cuts"])
    for rank, (_, _, _, (rank_of, split_mask), calls, single, live_before, live_after) in enumerate(out):
        assert split_mask == f["split_mask"] and np.array_equal(rank_of, f["rank_of"]), (c["name"], rank)
        assert live_after == live_before, (c["name"], rank, live_before, live_after)  # the pool is back where it was
        # the route the rank took is the one the level table and its slice call for
        if f["compressed"] and lengths[rank] > 0:
            assert calls == ["route_plan", "route_scatter", "build_begin_routed"], (c["name"], rank, calls)
            TALLY["two_pass_ranks"] += 1
        elif f["compressed"]:
            assert calls == ["buckets_state", "partition", "build_begin_routed"], (c["name"], rank, calls)
            TALLY["one_pass_ranks"] += 1
        else:
            assert calls == ["buckets", "partition", "build_begin"], (c["name"], rank, calls)
        if single is not None:
            TALLY["single_chain_true" if single else "single_chain_false"] += 1
    if with_dir:
        SC.assert_same_directory(tmp_path / "sharded", c)
        TALLY["directories"] += 1
    TALLY["cases"] += 1
    TALLY["compressed_cases"] += f["compressed"]
    TALLY["raw_cases"] += not f["compressed"]
    TALLY["split_cases"] += out[0][3][1] != 0


@pytest.mark.parametrize("world", [1, 3])
def test_empty_cloud_writes_what_the_one_gpu_build_writes(ranks, world, tmp_path):
    """No point on any rank: no node, the root included, and the directory of ctx.build(empty cloud).write_dir — meta.pb alone, the
    same bytes."""
    c = SC.constructed(f"empty_world{world}")
    out = run_case(ranks, c, tmp_path / "sharded")
    assert out[0][0] == {}
    ctx = pcv.Context(0)
    try:
        e = np.zeros(0)
        t = ctx.build(c["res"], pcv.Aabb(c["bmin"], c["bmax"]), e, e, e, np.zeros((0, 3), np.uint8), max_points_per_node=c["cap"])
        assert t.num_nodes == 0
        t.write_dir(str(tmp_path / "plain"))
        t.free()
    finally:
        ctx.close()
    assert os.listdir(tmp_path / "sharded") == os.listdir(tmp_path / "plain") == ["meta.pb"]
    assert (tmp_path / "sharded" / "meta.pb").read_bytes() == (tmp_path / "plain" / "meta.pb").read_bytes()


def test_the_cases_above_took_every_branch():
    """The two-pass compressed route (a rank with input while the exchange is compressed), the one-pass compressed route (a rank
    without input in such a case), the raw exchange and plans that split a level-1 node: as often as the oracle predicts, which
    tests/test_sharded_cases_cpu.py holds above the lower bounds. Which of the local builds took the single-chain build is
    reported, not required."""
    print("sharded fuzz tally:", TALLY)
    want = SC.tally_expected(SC.all_cases())
    assert {k: TALLY[k] for k in want} == want, (TALLY, want)
    assert TALLY["compressed_cases"] >= SC.MIN_COMPRESSED_CASES and TALLY["two_pass_ranks"] >= SC.MIN_TWO_PASS_RANKS, TALLY
    assert TALLY["one_pass_ranks"] >= SC.MIN_ONE_PASS_RANKS and TALLY["raw_cases"] >= SC.MIN_RAW_CASES, TALLY
    assert TALLY["split_cases"] >= SC.MIN_SPLIT_CASES, TALLY
    assert TALLY["directories"] >= len(SC.CONSTRUCTED) + len(SC.SEEDS) // 5, TALLY
