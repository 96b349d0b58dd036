#!/usr/bin/env python
"""The S2 split measured (GPU box): Gaussian clusters (bench.py's generator and seed, as BASELINE config 5 uses it) in a 1 000 m
cube 1.5 km above 37.4 N 122.1 W — config 5's own offset (-2.7e6, -4.3e6, 3.8e6) has a radius of 6.342e6 m, which S2Splitter
rejects as no valid ECEF point —, device-resident, split at --level `--runs` times after one warm-up. Per run: wall time of
Context.s2_split (ends in a stream synchronise) and kernel time per stage from ctx.kernel_stats():
  ids      s2_ids_kernel (validity + cell id), bbox = aabb_partial_kernel
  regroup  the two radix sorts (64-bit ids on the bits that vary, then (rank, index) pairs), s2_unique_kernel, s2_rank_kernel
  gather   s2_gather_kernel
Medians over the runs. The host twin (pcv_s2_cell_ids_host, one thread) runs over --host-points of the same cloud for scale, and
the device's ids of those points are checked against it.

usage: python tools/s2_split_bench.py [--points N] [--level L] [--runs R] [--host-points H] [--out FILE]"""
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

IDS, BBOX, GATHER = "s2_ids_kernel", "aabb_partial_kernel", "s2_gather_kernel"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100_000_000)
    ap.add_argument("--level", type=int, default=20)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--host-points", type=int, default=4_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "s2_split_bench.json"))
    args = ap.parse_args()

    dev = torch.device("cuda", 0)
    rot, ground = synthetic.ecef_from_local(37.407204, -122.147604)
    origin = ground + 1500.0 * rot[:, 2] - 500.0  # make_cloud's centres fill a 1 000 m cube from its offset
    x, y, z, rgb = make_cloud(torch, args.points, seed=1, device=dev, offset=tuple(float(c) for c in origin))
    torch.cuda.synchronize()
    ctx = pcv.Context(0)
    points = dict(x=x, y=y, z=z, color=rgb)
    ctx.s2_split(points, args.level).free()  # warm-up: the pool's blocks exist from here on
    ctx.set_profiling(True)
    rows, cells = [], None
    for _ in range(args.runs):
        ctx.reset_kernel_stats()
        t0 = time.perf_counter()
        cloud = ctx.s2_split(points, args.level)
        wall = (time.perf_counter() - t0) * 1e3
        st = {k: v[1] for k, v in ctx.kernel_stats().items() if v[0]}
        cells, counts = cloud.num_cells, cloud.cells[1]
        cloud.free()
        total = sum(st.values())
        rows.append(dict(wall=wall, kernels=total, ids=st[IDS], bbox=st.get(BBOX, 0.0), gather=st[GATHER],
                         regroup=total - st[IDS] - st.get(BBOX, 0.0) - st[GATHER], per_kernel=st))
    med = {k: round(float(np.median([r[k] for r in rows])), 4) for k in ("wall", "kernels", "ids", "bbox", "regroup", "gather")}
    per_kernel = {k: round(float(np.median([r["per_kernel"].get(k, 0.0) for r in rows])), 4) for k in rows[0]["per_kernel"]}
    ctx.set_profiling(False)

    h = min(args.host_points, args.points)
    hx, hy, hz = (a[:h].cpu().numpy() for a in (x, y, z))
    t0 = time.perf_counter()
    host_ids = pcv.s2_cell_ids(hx, hy, hz, args.level)
    host_s = time.perf_counter() - t0
    dev_ids = ctx.s2_cell_ids(x[:h], y[:h], z[:h], args.level).cpu().numpy().view(np.uint64)
    same = bool(np.array_equal(host_ids, dev_ids))
    n = args.points
    out = {"tool": "tools/s2_split_bench.py", "build_hash": build_hash(), "device": torch.cuda.get_device_name(0),
           "cloud": f"{n} Gaussian-cluster points (bench.make_cloud, seed 1) in a 1 000 m cube 1.5 km above 37.4 N 122.1 W, ECEF, "
                    "device-resident, colour, no intensity",
           "split_level": args.level, "cells": int(cells), "largest_cell_points": int(counts.max()), "runs": args.runs,
           "median_ms": med, "median_ms_per_kernel": per_kernel,
           "min_max_wall_ms": [round(min(r["wall"] for r in rows), 3), round(max(r["wall"] for r in rows), 3)],
           "split_Mpoints_per_s_wall": round(n / med["wall"] / 1e3, 1),
           "ids_ns_per_point": round(med["ids"] * 1e6 / n, 5),
           "ids_input_GB_per_s": round(24.0 * n / (med["ids"] * 1e-3) / 1e9, 1),
           "host_twin": {"points": h, "seconds": round(host_s, 3), "Mpoints_per_s_one_thread": round(h / host_s / 1e6, 2),
                         "device_ids_equal": same}}
    print(json.dumps(out))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    ctx.close()
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
