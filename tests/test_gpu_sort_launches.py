"""The launch sequence of the stage sorts, pinned: which kernels pcv_sort_keys64 / pcv_sort_keys32 / pcv_sort_pairs32 launch
and how often, on inputs of two tiles and a ragged tail and of a single key — the keys-only sort and the generic record sort
of csrc/pcv_sort.hip through the C ABI; every result against np.sort / a stable argsort. (The sorts of the octree build — the
rows form, the held-back pass — are pinned by test_gpu_build_launches.py.)
tests/golden/sort_launches.json was recorded on an MI355X at the commit named inside it, before the sort's host code was
split into a plan and two files; it is a record of that commit and is not regenerated from later code. (Recording: run this
file with PCV_RECORD_SORT_LAUNCHES=<commit hash> at that commit.)"""
import json
import os

import numpy as np
import pytest

import point_cloud_viewer_amd as pcv

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sort_launches.json")
RECORD = os.environ.get("PCV_RECORD_SORT_LAUNCHES", "")

N = 8209  # two tiles of 4 096 and a ragged tail of 17
SORTS = {  # name: (sort, n, begin_bit, end_bit)
    "keys64_0_63": ("keys64", N, 0, 63),
    "keys64_12_33": ("keys64", N, 12, 33),
    "keys64_one_key": ("keys64", 1, 0, 63),
    "keys32_6_30": ("keys32", N, 6, 30),
    "pairs32_13_bits": ("pairs32", N, 0, 13),
    "pairs32_32_bits": ("pairs32", N, 0, 32),
}


@pytest.fixture(scope="module")
def ctx():
    c = pcv.Context(0)
    c.set_profiling(1)
    yield c
    c.close()


@pytest.fixture(scope="module")
def golden():
    if RECORD:
        return {"commit": RECORD, "sorts": {}}
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("name", list(SORTS))
def test_sort_launches_the_recorded_kernels(ctx, golden, name):
    kind, n, begin, end = SORTS[name]
    rng = np.random.default_rng(17)
    bits = 64 if kind == "keys64" else 32
    keys = rng.integers(0, 2 ** (bits - 1), n, dtype=np.uint64).astype(np.uint64 if bits == 64 else np.uint32)
    if kind == "pairs32":
        keys &= np.uint32((1 << end) - 1) if end < 32 else np.uint32(0xFFFFFFFF)  # pairs sort on whole keys
    if n > 10:
        keys[::7] = keys[3]  # heavy duplicates: the order among them shows whether the sort is stable
    masked = (keys >> keys.dtype.type(begin)) & keys.dtype.type((1 << (end - begin)) - 1)
    order = np.argsort(masked, kind="stable")
    ctx.reset_kernel_stats()
    if kind == "keys64":
        got = ctx.sort_keys64(keys.copy(), begin, end)
    elif kind == "keys32":
        got = ctx.sort_keys32(keys.copy(), begin, end)
    else:
        vals = np.arange(n, dtype=np.uint32)
        got, got_vals = ctx.sort_pairs32(keys.copy(), vals.copy(), begin, end)
        assert np.array_equal(got_vals, vals[order])
    ctx.synchronize()
    launches = {k: int(v[0]) for k, v in sorted(ctx.kernel_stats().items()) if v[0] > 0}
    print(name, "launches:", launches)
    assert np.array_equal(got, keys[order])
    if begin == 0 and end >= bits - 1:
        assert np.array_equal(got, np.sort(keys))
    if RECORD:
        golden["sorts"][name] = launches
        if len(golden["sorts"]) == len(SORTS):
            with open(GOLDEN, "w") as f:
                json.dump(golden, f, indent=1, sort_keys=True)
                f.write("\n")
        return
    assert launches == golden["sorts"][name]
