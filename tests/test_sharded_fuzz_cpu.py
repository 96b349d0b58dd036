"""point_cloud_viewer_amd.distributed alone, over the cases of tests/sharded_cases.py: ShardedOctreeBuilder with the host backend
(the oracle stands in for the device) on CPU tensors, the ranks as threads (tests/thread_dist.py). What is under test is the plan,
the send matrix, the stable partition, the exchange in source-rank order, the global layout of the top of the tree and its merge,
for every level-1 coding, worlds of 1 to 8, ragged and empty rank slices and builders that are reused from case to case. Truth: ONE
oracle build of the whole cloud; every comparison is byte equality."""
import numpy as np
import pytest
import torch

import oracle_lib as O
import point_cloud_viewer_amd as pcv
import sharded_cases as SC
from host_backend import ORACLE_LOCK, HostBackend
from point_cloud_viewer_amd import distributed as pdist
from thread_dist import run_ranks

# one builder per (world, rank, compress, shard_mode) for the whole module: the cases run in seed order, so sizes, regimes and
# intensity change between consecutive builds on the same _exchange_buffers
BUILDERS = {}


def _builder(c, rank, dist):
    key = (c["world"], rank, c["compress"], c["shard_mode"])
    b = BUILDERS.get(key)
    if b is None:
        b = BUILDERS[key] = pdist.ShardedOctreeBuilder(None, dist, torch.device("cpu"), backend=HostBackend(O, c["cap"]),
                                                       compress_exchange=c["compress"], shard_mode=c["shard_mode"])
    b.dist = dist  # the rendezvous of this case's threads
    b.backend.cap = c["cap"]
    return b


def run_case(c, directory=None):
    """[(merged on rank 0 or None, exchange_info, send matrix, plan)] of the ranks."""
    whole = SC.whole_tensors(c, torch.device("cpu"))

    def rank_main(rank, dist):
        b = _builder(c, rank, dist)
        x, y, z, rgb, inten = SC.rank_input(c, whole, rank)
        res = b.build(c["res"], pcv.Aabb(c["bmin"], c["bmax"]), x, y, z, rgb, inten, max_points_per_node=c["cap"])
        merged = res.gather(0)
        if directory is not None:
            res.write_dir(str(directory))
        return merged, res.exchange_info(), res.counts, res.plan

    return run_ranks(c["world"], rank_main)


@pytest.mark.parametrize("case_id", SC.all_cases(), ids=str)
def test_sharded_build_on_the_host_backend_equals_one_oracle_build(case_id, tmp_path):
    c, f = SC.get(case_id), SC.facts(case_id)
    with_dir = not isinstance(case_id, int) or case_id % 5 == 0
    out = run_case(c, tmp_path / "sharded" if with_dir else None)
    with ORACLE_LOCK:
        want = SC.oracle_tree(case_id)
    SC.assert_same_tree(out[0][0], want, c)
    assert all(o[0] is None for o in out[1:])
    SC.assert_exchange(c, f, [(o[1], o[2]) for o in out])
    for _, _, _, (rank_of, split_mask) in out:  # every rank derives the plan the oracle's counts give
        assert split_mask == f["split_mask"] and np.array_equal(rank_of, f["rank_of"]), c["name"]
    if with_dir:
        SC.assert_same_directory(tmp_path / "sharded", c)


@pytest.mark.parametrize("world", [1, 3])
def test_empty_cloud_has_no_node(world, tmp_path):
    """No point on any rank: the oracle and the one-GPU build report no node at all (test_degenerate_inputs), so the sharded build has
    no top node either, gather() is empty, and the directory holds meta.pb alone — the bytes write_meta gives for no nodes, which
    is what pcv_octree_write_dir writes for an empty tree (test_empty_stream_writes_meta_without_nodes)."""
    import os
    c = SC.constructed(f"empty_world{world}")
    out = run_case(c, tmp_path / "sharded")
    assert out[0][0] == {} and all(o[0] is None for o in out[1:])
    assert os.listdir(tmp_path / "sharded") == ["meta.pb"]
    os.makedirs(tmp_path / "plain")
    pcv.octree.write_meta(str(tmp_path / "plain"), c["res"], c["bmin"], c["bmax"], [])
    assert (tmp_path / "sharded" / "meta.pb").read_bytes() == (tmp_path / "plain" / "meta.pb").read_bytes()
    from point_cloud_viewer_amd.distributed import top_layout, top_nodes
    layout = top_layout([0] * 8, [0] * 64, 0)
    assert layout["root_points"] == 0 and top_nodes(layout, [2, 2], False) == ([], 0)


def test_builders_were_reused():
    """The cases above ran on builders kept from case to case: a second, smaller build views the blocks of a larger one."""
    assert BUILDERS and len(BUILDERS) < len(SC.all_cases())
    assert any(int(t.shape[0]) >= 4_096 for b in BUILDERS.values() for t in b._exchange_buffers.values())
