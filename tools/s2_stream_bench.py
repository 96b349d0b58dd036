#!/usr/bin/env python
"""The S2 stream measured (GPU box): the cloud of tools/s2_split_bench.py (Gaussian clusters in a 1 000 m cube 1.5 km above
37.4 N 122.1 W, device-resident, colour, no intensity) fed to Context.s2_stream in device batches of --batch-points.
  in_memory   wall time from the first append to the end of finish, `--runs` times after one warm-up, against the one-shot
              s2_split of the same points (what there was before the stream); the result is checked against it once
  merge       s2_merge_kernel alone (ctx.kernel_stats) against the bytes it moves: per point 24 + 3 + 4 (xyz, rgb, order) read
              and the same written
  directory   a directory stream onto tmpfs (/dev/shm when there is one) at each of --flush-points: wall time, flushes, and the
              directory's bytes; the first one is checked against the one-shot cloud's cells
Medians over the runs. No time is promised anywhere; this tool only reports.

usage: python tools/s2_stream_bench.py [--points N] [--batch-points B] [--level L] [--runs R] [--flush-points F ...] [--out FILE]"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import point_cloud_viewer_amd as pcv  # noqa: E402
from bench import build_hash, make_cloud  # noqa: E402
from point_cloud_viewer_amd import synthetic  # noqa: E402

MERGE = "s2_merge_kernel"


def feed(stream, points, n, step):
    for lo in range(0, n, step):
        stream.append({k: v[lo:lo + step] for k, v in points.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100_000_000)
    ap.add_argument("--batch-points", type=int, default=500_000)
    ap.add_argument("--level", type=int, default=20)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--flush-points", type=int, nargs="*", default=[1 << 24, 1 << 26])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "s2_stream_bench.json"))
    args = ap.parse_args()
    n, step = args.points, args.batch_points

    dev = torch.device("cuda", 0)
    rot, ground = synthetic.ecef_from_local(37.407204, -122.147604)
    origin = ground + 1500.0 * rot[:, 2] - 500.0
    x, y, z, rgb = make_cloud(torch, n, seed=1, device=dev, offset=tuple(float(c) for c in origin))
    torch.cuda.synchronize()
    ctx = pcv.Context(0)
    points = dict(x=x, y=y, z=z, color=rgb)

    # ---- the one-shot split: the truth of the checks and the time to compare with ----
    whole = ctx.s2_split(points, args.level)
    one_shot = []
    for _ in range(args.runs):
        t0 = time.perf_counter()
        ctx.s2_split(points, args.level).free()
        one_shot.append((time.perf_counter() - t0) * 1e3)

    # ---- in memory ----
    stream = ctx.s2_stream(args.level)
    feed(stream, points, n, step)
    cloud = stream.finish()  # warm-up, and the check
    same = all(np.array_equal(a, b) for a, b in zip(cloud.cells, whole.cells)) and np.array_equal(cloud.order, whole.order)
    for k in range(0, whole.num_cells, max(1, whole.num_cells // 16)):  # the blobs of a sample of cells
        same = same and all(a.tobytes() == b.tobytes() for a, b in zip(cloud.cell_points(k, 1)[:2], whole.cell_points(k, 1)[:2]))
    cloud.free()
    ctx.set_profiling(True)
    rows = []
    for _ in range(args.runs):
        ctx.reset_kernel_stats()
        t0 = time.perf_counter()
        stream = ctx.s2_stream(args.level)
        feed(stream, points, n, step)
        t1 = time.perf_counter()
        cloud = stream.finish()
        t2 = time.perf_counter()
        st = ctx.kernel_stats()
        cloud.free()
        rows.append(dict(wall=(t2 - t0) * 1e3, appends=(t1 - t0) * 1e3, finish=(t2 - t1) * 1e3, merge=st[MERGE][1], launches=st[MERGE][0]))
    ctx.set_profiling(False)
    med = {k: round(float(np.median([r[k] for r in rows])), 4) for k in ("wall", "appends", "finish", "merge")}
    merge_bytes = 2 * 31 * n
    batches = (n + step - 1) // step

    # ---- directory streams on tmpfs ----
    base = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else None
    directory = []
    for flush_points in args.flush_points:
        out = tempfile.mkdtemp(prefix="s2_stream_bench_", dir=base)
        try:
            t0 = time.perf_counter()
            stream = ctx.s2_stream(args.level, out, flush_points=flush_points)
            feed(stream, points, n, step)
            info = stream.info
            flushes = info["flushes"] + (1 if info["pending_points"] else 0)  # finish flushes what is pending
            cloud = stream.finish()
            wall = (time.perf_counter() - t0) * 1e3
            ok = all(np.array_equal(a, b) for a, b in zip(cloud.cells, whole.cells))
            if not directory:
                k = whole.num_cells // 2
                ok = ok and all(a.tobytes() == b.tobytes() for a, b in zip(cloud.cell_points(k, 1)[:2], whole.cell_points(k, 1)[:2]))
            cloud.free()
            size = sum(os.path.getsize(os.path.join(out, f)) for f in os.listdir(out))
            directory.append(dict(flush_points=flush_points, wall_ms=round(wall, 1), flushes=flushes,
                                  directory_bytes=size, files=len(os.listdir(out)), Mpoints_per_s=round(n / wall / 1e3, 1),
                                  equals_one_shot=bool(ok), tmpfs=base is not None))
            same = same and ok
        finally:
            shutil.rmtree(out, ignore_errors=True)

    out = {"tool": "tools/s2_stream_bench.py", "build_hash": build_hash(), "device": torch.cuda.get_device_name(0),
           "cloud": f"{n} Gaussian-cluster points (bench.make_cloud, seed 1) in a 1 000 m cube 1.5 km above 37.4 N 122.1 W, ECEF, "
                    "device-resident, colour, no intensity",
           "split_level": args.level, "cells": int(whole.num_cells), "batch_points": step, "batches": batches, "runs": args.runs,
           "one_shot_split_wall_ms": round(float(np.median(one_shot)), 4),
           "in_memory_stream_median_ms": med,
           "in_memory_stream_Mpoints_per_s_wall": round(n / med["wall"] / 1e3, 1),
           "stream_over_one_shot": round(med["wall"] / float(np.median(one_shot)), 3),
           "merge": {"launches_per_stream": int(rows[0]["launches"]), "ms": med["merge"], "bytes_moved": merge_bytes,
                     "GB_per_s": round(merge_bytes / (med["merge"] * 1e-3) / 1e9, 1), "bytes_per_point": "31 read + 31 written"},
           "directory_streams": directory, "equals_one_shot": bool(same)}
    whole.free()
    print(json.dumps(out))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    ctx.close()
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
