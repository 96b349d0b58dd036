#!/usr/bin/env python
"""The extra attributes of S2 cell clouds measured (GPU box): the cloud of tools/s2_split_bench.py (Gaussian clusters in a
1 000 m cube 1.5 km above 37.4 N 122.1 W, device-resident, colour) with intensity and one U8, one U64 and one F64Vec3 extra
(1 + 8 + 24 bytes per point beside the 31 of xyz, rgb and intensity).
  split    wall time of s2_split without and with the extras, and s2_attr_gather_kernel alone (ctx.kernel_stats) against the
           bytes it moves: per point 3 x 4 (the permutation, once per extra) + 33 read and 33 written
  merge    an in-memory stream in device batches of --batch-points: wall time without and with the extras, s2_attr_merge_kernel
           alone against 33 bytes read and 33 written per point
  query    AllPoints over the whole cloud with one filter (the U8 column) and with three (U8, U64 and intensity, the last of
           which stays inside s2_flags_kernel): wall time and s2_attr_filter_kernel alone; the kept count is checked against torch
Medians over --runs after one warm-up. Element-granular gathers are uncoalesced by nature: no rate is promised anywhere; this
tool only reports.

usage: python tools/s2_attr_bench.py [--points N] [--batch-points B] [--level L] [--runs R] [--out FILE]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import point_cloud_viewer_amd as pcv  # noqa: E402
from bench import build_hash, make_cloud  # noqa: E402
from point_cloud_viewer_amd import synthetic  # noqa: E402

GATHER, MERGE, FILTER = "s2_attr_gather_kernel", "s2_attr_merge_kernel", "s2_attr_filter_kernel"
EXTRA_BYTES = 1 + 8 + 24


def median_ms(fn, runs):
    fn()  # warm-up
    out = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(out)), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100_000_000)
    ap.add_argument("--batch-points", type=int, default=10_000_000)
    ap.add_argument("--level", type=int, default=20)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "s2_attr_bench.json"))
    args = ap.parse_args()
    n, step = args.points, args.batch_points

    dev = torch.device("cuda", 0)
    rot, ground = synthetic.ecef_from_local(37.407204, -122.147604)
    origin = ground + 1500.0 * rot[:, 2] - 500.0
    x, y, z, rgb = make_cloud(torch, n, seed=1, device=dev, offset=tuple(float(c) for c in origin))
    gen = torch.Generator(device=dev).manual_seed(7)
    label = torch.randint(0, 256, (n,), dtype=torch.uint8, device=dev, generator=gen)
    inten = torch.rand((n,), dtype=torch.float32, device=dev, generator=gen)
    stamp = torch.randint(0, 1 << 62, (n,), dtype=torch.int64, device=dev, generator=gen)  # the bits of a u64 timestamp
    normal = torch.randn((n, 3), dtype=torch.float64, device=dev, generator=gen)
    torch.cuda.synchronize()
    ctx = pcv.Context(0)
    bare = dict(x=x, y=y, z=z, color=rgb, intensity=inten)
    extras = dict(label=label, timestamp=(stamp, "u64"), normal=normal)
    full = dict(bare, attributes=extras)

    def take(points, lo, hi):
        out = {k: v[lo:hi] for k, v in points.items() if k != "attributes"}
        if "attributes" in points:
            out["attributes"] = {k: ((v[0][lo:hi], v[1]) if isinstance(v, tuple) else v[lo:hi]) for k, v in points["attributes"].items()}
        return out

    # ---- split ----
    split_bare = median_ms(lambda: ctx.s2_split(bare, args.level).free(), args.runs)
    split_full = median_ms(lambda: ctx.s2_split(full, args.level).free(), args.runs)
    ctx.set_profiling(True)
    ctx.reset_kernel_stats()
    cloud = ctx.s2_split(full, args.level)
    gather = ctx.kernel_stats()[GATHER]

    # ---- merge ----
    def stream_of(points):
        stream = ctx.s2_stream(args.level)
        for lo in range(0, n, step):
            stream.append(take(points, lo, min(n, lo + step)))
        return stream.finish()

    ctx.set_profiling(False)
    stream_bare = median_ms(lambda: stream_of(bare).free(), args.runs)
    stream_full = median_ms(lambda: stream_of(full).free(), args.runs)
    ctx.set_profiling(True)
    ctx.reset_kernel_stats()
    merged = stream_of(full)
    merge = ctx.kernel_stats()[MERGE]
    same = all(np.array_equal(a, b) for a, b in zip(merged.cells, cloud.cells))
    k = cloud.num_cells // 2
    same = same and all(merged.cell_attribute(a, k, 1).tobytes() == cloud.cell_attribute(a, k, 1).tobytes() for a in cloud.attributes)
    merged.free()

    # ---- query ----
    shapes = ctx.shapes([("all",)])
    one = [{"label": (16.0, 200.0)}]
    three = [{"label": (16.0, 200.0), "timestamp": (0.0, float(1 << 61)), "intensity": (0.125, 0.875)}]
    ctx.set_profiling(False)
    query = {"no_filter_ms": median_ms(lambda: cloud.query_batch(shapes).free(), args.runs),
             "one_filter_ms": median_ms(lambda: cloud.query_batch(shapes, filters=one).free(), args.runs),
             "three_filters_ms": median_ms(lambda: cloud.query_batch(shapes, filters=three).free(), args.runs)}
    ctx.set_profiling(True)
    ctx.reset_kernel_stats()
    batch = cloud.query_batch(shapes, filters=three)
    flt = ctx.kernel_stats()[FILTER]
    want = int(((label >= 16) & (label <= 200) & (stamp <= (1 << 61)) & (inten >= 0.125) & (inten <= 0.875)).sum().item())
    same = same and batch.num_points == want
    query.update(filter_kernel_launches=int(flt[0]), filter_kernel_ms=round(float(flt[1]), 4), kept=int(batch.num_points), kept_by_torch=want)
    batch.free()
    ctx.set_profiling(False)

    out = {"tool": "tools/s2_attr_bench.py", "build_hash": build_hash(), "device": torch.cuda.get_device_name(0),
           "cloud": f"{n} Gaussian-cluster points (bench.make_cloud, seed 1) in a 1 000 m cube 1.5 km above 37.4 N 122.1 W, ECEF, "
                    "device-resident, colour, intensity; extras label U8, timestamp U64, normal F64Vec3",
           "split_level": args.level, "cells": int(cloud.num_cells), "runs": args.runs,
           "split": {"without_extras_wall_ms": split_bare, "with_extras_wall_ms": split_full, "gather_launches": int(gather[0]),
                     "gather_ms": round(float(gather[1]), 4), "bytes_per_point": f"3 x 4 + {EXTRA_BYTES} read, {EXTRA_BYTES} written",
                     "GB_per_s": round((3 * 4 + 2 * EXTRA_BYTES) * n / (float(gather[1]) * 1e-3) / 1e9, 1) if gather[1] else None},
           "stream": {"batch_points": step, "without_extras_wall_ms": stream_bare, "with_extras_wall_ms": stream_full,
                      "merge_launches": int(merge[0]), "merge_ms": round(float(merge[1]), 4),
                      "GB_per_s": round(2 * EXTRA_BYTES * n / (float(merge[1]) * 1e-3) / 1e9, 1) if merge[1] else None},
           "query_all_points": query, "checks_passed": bool(same)}
    cloud.free()
    print(json.dumps(out))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    ctx.close()
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
