"""The host side of the out-of-core build (pcv_ooc_plan, pcv_ooc_top_layout): pure, deterministic, no GPU needed."""
import ctypes as C

import numpy as np
import pytest

import point_cloud_viewer_amd as pcv
from point_cloud_viewer_amd import _lib as L
from point_cloud_viewer_amd import distributed as pdist
from point_cloud_viewer_amd.octree import ooc_plan, ooc_top_layout


def random_counts(rng, empty=0.3, scale=200_000):
    c = rng.integers(0, scale, 64).astype(np.int64)
    c[rng.random(64) < empty] = 0
    return c


@pytest.mark.parametrize("seed", range(20))
def test_plan_covers_every_bucket_once_keeps_unsplit_octants_whole_and_respects_the_budget(seed):
    rng = np.random.default_rng(seed)
    counts = random_counts(rng)
    counts[rng.integers(0, 8) * 8:][:8] //= 1000  # an octant small enough to stay a leaf
    cap = int(rng.integers(1_000, 300_000))
    budget = int(counts.max() + rng.integers(0, 500_000))
    can_split = bool(seed % 5)
    try:
        part, nparts, mask = ooc_plan(counts, cap, can_split, budget)
    except pcv.PcvError as e:  # an unsplit octant larger than the budget
        assert e.code == pcv.PCV_E_OOM and "octant" in str(e)
        return
    _, want_mask = pdist.plan_buckets(counts, 1, cap, can_split)
    assert mask == want_mask
    assert ((part >= 0) == (counts > 0)).all() and (part < nparts).all()
    loads = np.bincount(part[part >= 0], weights=counts[part >= 0], minlength=nparts)
    assert nparts == 0 or (loads <= budget).all() and (loads > 0).all()
    for c in range(8):
        if not (mask >> c) & 1:
            owners = set(part[c * 8:c * 8 + 8][counts[c * 8:c * 8 + 8] > 0])
            assert len(owners) <= 1, (c, owners)
    again = ooc_plan(counts, cap, can_split, budget)
    assert np.array_equal(again[0], part) and again[1:] == (nparts, mask)


def test_plan_is_deterministic_and_one_partition_when_everything_fits():
    counts = random_counts(np.random.default_rng(1))
    a = ooc_plan(counts, 100_000, True, 0)
    b = ooc_plan(counts, 100_000, True, 0)
    assert np.array_equal(a[0], b[0]) and a[1:] == b[1:] and a[1] == 1


def test_over_budget_units_are_reported():
    counts = np.zeros(64, dtype=np.int64)
    counts[19] = 5_000_000
    counts[20] = 10
    with pytest.raises(pcv.PcvError) as e:
        ooc_plan(counts, 100_000, True, 1_000_000)
    assert e.value.code == pcv.PCV_E_OOM and "bucket 19" in str(e.value) and "5000000" in str(e.value)
    counts[:] = 0
    counts[40:48] = 70_000  # 560 000 points in octant 5; no level-1 node can be split
    with pytest.raises(pcv.PcvError) as e:
        ooc_plan(counts, 100_000, False, 500_000)
    assert "octant 5" in str(e.value) and "560000" in str(e.value)
    # the same octant splits when it may: every bucket fits
    part, nparts, mask = ooc_plan(counts, 100_000, True, 500_000)
    assert mask == 1 << 5 and nparts == 2


def test_totals_beyond_2_to_the_32_are_counted_in_64_bits():
    counts = np.full(64, 100_000_000, dtype=np.int64)  # 6.4 x 10^9 points
    part, nparts, mask = ooc_plan(counts, 100_000, True, 1_000_000_000)
    assert mask == 0xFF and nparts == 7
    loads = np.bincount(part, weights=counts, minlength=nparts)
    assert loads.sum() == 6_400_000_000 and (loads <= 1_000_000_000).all()


@pytest.mark.parametrize("seed", range(20))
def test_top_layout_equals_distributed_top_layout(seed):
    rng = np.random.default_rng(100 + seed)
    l1 = rng.integers(0, 5_000_000, 8)
    l2 = rng.integers(0, 700_000, 64)
    l2[rng.random(64) < 0.3] = 0
    mask = int(rng.integers(0, 256))
    want = pdist.top_layout(l1, l2, mask)
    got = ooc_top_layout(l1, l2, mask)
    for k in ("root_points", "l1_stream", "l1_offset", "l2_offset"):
        assert np.array_equal(np.asarray(got[k], dtype=np.int64), np.asarray(want[k], dtype=np.int64)), k


def test_stats_struct_layout():
    assert C.sizeof(L.OocStats) == 120
    assert L.OocStats.spill_bytes.offset == 32 and L.OocStats.h2d_ms.offset == 56 and L.OocStats.write_ms.offset == 104
    assert L.OocStats.split_mask.offset == 112 and L.OocStats.routed.offset == 116
