"""The merge plan of an S2 stream (pcv_s2_merge_plan.h through pcv_s2_merge_plan_host) against a numpy restatement: the parts
concatenated and sorted stably by cell id. No device."""
import numpy as np
import pytest

import point_cloud_viewer_amd as pcv

CHUNK = 2048  # kMergeChunkPoints


def starts(counts):
    """Exclusive prefix sums, uint64."""
    counts = np.asarray(counts, dtype=np.uint64)
    return (np.cumsum(counts, dtype=np.uint64) - counts).astype(np.uint64)


def restate(parts):
    """(ids, counts, offsets, segments as rows (dst_offset, src_offset, part, count)) of the merge by a stable argsort."""
    cell, part, src, count = [], [], [], []
    for p, (ids, counts) in enumerate(parts):
        ids, counts = np.asarray(ids, dtype=np.uint64), np.asarray(counts, dtype=np.uint64)
        cell.append(ids)
        part.append(np.full(ids.size, p, dtype=np.uint64))
        src.append(starts(counts))
        count.append(counts)
    cell, part, src, count = (np.concatenate(a) if a else np.zeros(0, dtype=np.uint64) for a in (cell, part, src, count))
    order = np.argsort(cell, kind="stable")  # parts were concatenated in order: stable = by part inside a cell
    cell, part, src, count = cell[order], part[order], src[order], count[order]
    dst = starts(count)
    ids, first = np.unique(cell, return_index=True)
    counts = np.add.reduceat(count, first).astype(np.uint64) if cell.size else np.zeros(0, dtype=np.uint64)
    offsets = dst[first] if cell.size else np.zeros(0, dtype=np.uint64)
    return ids, counts, offsets, np.stack([dst, src, part, count], axis=1) if cell.size else np.zeros((0, 4), dtype=np.uint64)


def check(parts, chunk_points=0):
    plan = pcv.s2_merge_plan(parts, chunk_points)
    again = pcv.s2_merge_plan(parts, chunk_points)
    for key in plan:  # deterministic
        assert plan[key].tobytes() == again[key].tobytes(), key
    ids, counts, offsets, rows = restate(parts)
    n = int(sum(int(np.asarray(c, dtype=np.uint64).sum()) for _, c in parts))
    assert np.all(plan["ids"][1:] > plan["ids"][:-1])
    assert np.array_equal(plan["ids"], ids) and np.array_equal(plan["counts"], counts) and np.array_equal(plan["offsets"], offsets)
    assert int(plan["counts"].sum()) == n
    seg = plan["segments"]
    got = np.stack([seg["dst_offset"], seg["src_offset"], seg["part"].astype(np.uint64), seg["count"].astype(np.uint64)], axis=1) \
        if seg.size else np.zeros((0, 4), dtype=np.uint64)
    assert np.array_equal(got, rows)
    # the segments tile [0, n) exactly once, in (cell, part) order
    if seg.size:
        assert seg["dst_offset"][0] == 0 and np.all(seg["count"] > 0)
        assert np.array_equal(seg["dst_offset"][1:], (seg["dst_offset"] + seg["count"])[:-1])
        assert int(seg["dst_offset"][-1] + seg["count"][-1]) == n
        seg_cell = plan["ids"][np.searchsorted(plan["offsets"], seg["dst_offset"], side="right") - 1]
        key = list(zip(seg_cell.tolist(), seg["part"].tolist()))
        assert key == sorted(key) and len(set(key)) == len(key)
        # every source point once: per part, the segments' source ranges tile the part
        for p, (_, c) in enumerate(parts):
            mine = seg[seg["part"] == p]
            mine = mine[np.argsort(mine["src_offset"], kind="stable")]
            assert np.array_equal(mine["count"], np.asarray(c, dtype=np.uint64))
            assert np.array_equal(mine["src_offset"], starts(mine["count"]))
    # every chunk's first segment
    step = chunk_points or CHUNK
    first = plan["chunk_first_segment"]
    assert first.size == (n + step - 1) // step
    want = np.searchsorted(seg["dst_offset"], np.arange(first.size, dtype=np.uint64) * np.uint64(step), side="right") - 1
    assert np.array_equal(first, want.astype(np.uint64))
    return plan


def random_parts(seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    universe = np.unique(rng.integers(1, 1 << 62, int(rng.integers(1, 400)), dtype=np.uint64))
    parts = []
    for _ in range(int(rng.integers(1, 40))):
        take = rng.random(universe.size) < rng.uniform(0.0, 1.0)
        ids = universe[take]
        big = rng.random(ids.size) < 0.02
        counts = np.where(big, rng.integers(1, 20000, ids.size), rng.integers(1, 12, ids.size)).astype(np.uint64)
        parts.append((ids, counts))
    return parts


@pytest.mark.parametrize("seed", range(20))
def test_seeded_plans(seed):
    parts = random_parts(seed)
    check(parts)
    check(parts, chunk_points=(1, 7, 64, 100000)[seed % 4])


NAMED = {
    "one part": [([3, 5, 9], [4, 1, 7000])],
    "a part with no cells": [([3, 5], [2, 2]), ([], []), ([5, 7], [1, 1])],
    "a cell in every part": [([4, 8], [3, 1]), ([8], [2]), ([2, 8, 10], [1, 5000, 1])],
    "a cell in one part only": [([4, 8], [3, 1]), ([6], [2]), ([4, 8], [1, 1])],
    "every segment of 1 point": [(np.arange(1, 3001, dtype=np.uint64) * 2 + (p % 2), np.ones(3000, dtype=np.uint64)) for p in range(5)],
    "one cell only": [([42], [c]) for c in (1, 4097, 2048, 1)],
    "no parts": [],
    "no points": [([], []), ([], [])],
}


@pytest.mark.parametrize("name", sorted(NAMED))
def test_named_plans(name):
    plan = check(NAMED[name])
    check(NAMED[name], chunk_points=3)
    if name == "one part":  # the merge is the identity
        assert np.array_equal(plan["segments"]["dst_offset"], plan["segments"]["src_offset"])
    if name == "every segment of 1 point":
        assert plan["segments"].size == 15000 and np.all(plan["segments"]["count"] == 1)
        assert np.array_equal(plan["chunk_first_segment"], np.arange(8, dtype=np.uint64) * CHUNK)
    if name == "one cell only":
        assert plan["ids"].tolist() == [42] and plan["counts"].tolist() == [6147]
        assert plan["chunk_first_segment"].tolist() == [0, 1, 1, 2]  # runs at 0, 1, 4098, 6146: points 2048 and 4096 lie in part 1's, 6144 in part 2's
    if name in ("no parts", "no points"):
        assert all(plan[k].size == 0 for k in plan)


def test_refusals():
    for parts, word in (([([5, 3], [1, 1])], "ascend"), ([([3, 3], [1, 1])], "ascend"), ([([0, 3], [1, 1])], "no cell id"),
                        ([([3, 5], [1, 1]), ([7, 2], [1, 1])], "part 1"), ([([3], [0])], "no points"),
                        ([([3, 5], [1 << 31, 1 << 31])], "2^32 - 1")):
        with pytest.raises(pcv.PcvError) as e:
            pcv.s2_merge_plan(parts)
        assert e.value.code == pcv.PCV_E_INVALID and word in str(e.value), str(e.value)
    with pytest.raises(ValueError):
        pcv.s2_merge_plan([([3, 5], [1])])


def test_named_cases_under_the_sanitizers(tmp_path):
    """csrc/pcv_s2_merge_plan.cpp stand-alone (tests/s2_merge_plan_driver.cpp, ASan + UBSan, no HIP, no library) over the named
    cases, a few seeded ones and the refusals: silent sanitizers, and the plans the library gives."""
    import os
    import subprocess

    from sort_plan_helper import CSRC, ROOT, SANITIZE, sanitizers_silent
    exe = tmp_path / "s2_merge_plan_driver"
    subprocess.check_call(SANITIZE + [os.path.join(ROOT, "tests", "s2_merge_plan_driver.cpp"), os.path.join(CSRC, "pcv_s2_merge_plan.cpp"),
                                      "-o", str(exe)])
    cases = [(name, NAMED[name], chunk) for name in sorted(NAMED) for chunk in (CHUNK, 3)]
    cases += [(f"seed {seed}", random_parts(seed), CHUNK) for seed in range(4)]
    refused = [[([5, 3], [1, 1])], [([0, 3], [1, 1])], [([3], [0])], [([3, 5], [1 << 31, 1 << 31])]]
    cases += [("refused", parts, CHUNK) for parts in refused]
    lines = []
    for _, parts, chunk in cases:
        words = [chunk, len(parts)]
        for ids, counts in parts:
            words.append(len(ids))
            for i, c in zip(np.asarray(ids, dtype=np.uint64).tolist(), np.asarray(counts, dtype=np.uint64).tolist()):
                words += [i, c]
        lines.append(" ".join(str(w) for w in words))
    (tmp_path / "cases.txt").write_text("\n".join(lines) + "\n")
    p = subprocess.run([str(exe), str(tmp_path / "cases.txt")], capture_output=True, text=True)
    sanitizers_silent(p)
    out = p.stdout.splitlines()
    assert out[-1] == f"cases {len(cases)}"
    at = 0
    for name, parts, chunk in cases:
        _, rc, n = out[at].split()
        if name == "refused":
            assert int(rc) == pcv.PCV_E_INVALID and out[at + 1]
            at += 2
            continue
        plan = pcv.s2_merge_plan(parts, chunk)
        assert int(rc) == pcv.PCV_OK and int(n) == int(plan["counts"].sum()), name
        rows = {line.split()[0]: [int(w) for w in line.split()[1:]] for line in out[at + 1:at + 6]}
        seg = plan["segments"]
        assert rows["ids"] == plan["ids"].tolist() and rows["counts"] == plan["counts"].tolist() and rows["offsets"] == plan["offsets"].tolist(), name
        assert rows["segments"] == np.stack([seg["dst_offset"], seg["src_offset"], seg["part"], seg["count"]], axis=1).ravel().tolist(), name
        assert rows["chunks"] == plan["chunk_first_segment"].tolist(), name
        at += 6
    assert at == len(out) - 1
