#!/usr/bin/env python
"""Terrain layers, measured (GPU box; there is no CPU fallback). The cloud is config 2: 100 M Gaussian-cluster points
(bench.py's generator, seed 1, colour) in an octree of resolution 0.001; the terrain takes AllPoints of it at tile size 256.
resolution_m is the first of --resolutions at which between 1 000 and 5 000 tiles are touched; the value is recorded.
One process, a warm-up round and then --runs rounds in which the three statistics and their legs alternate; medians and spreads:
  accumulate   add_points over device planes (the batch's points, copied out once): wall, and terrain_mark_kernel /
               terrain_accum_kernel alone (ctx.kernel_stats); the atomics' achieved rate over the accumulate kernel's time, in
               operations and bytes per second (MAX / MIN: one 8-byte max and one 4-byte add per kept point; MEAN: four 8-byte
               adds and one 4-byte add)
  query        the same points through add_query_batch: staging (the row packer and the unpack pass per piece) included
  resolve      terrain_count_kernel + terrain_resolve_kernel of finish
  mask         terrain_mask_kernel of finish
  write        write_dir onto tmpfs
Yardstick, for the README and no pass criterion: the `colored` xray leaf build of the same tree at a pixel size equal to the
resolution and 256-pixel tiles (the leg tools/xray_bench.py times), in the same process and rounds.
Prints one JSON line and writes it to --out.

usage: python tools/terrain_bench.py [--points N] [--runs R] [--resolutions a,b,..] [--tmp DIR] [--out FILE]"""
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

TILE = 256
STATS = ("max", "min", "mean")
ATOMICS = {"max": (2, 12), "min": (2, 12), "mean": (5, 36)}  # operations and bytes per kept point
POOL_CAP = 64 << 30


def spread(values):
    v = np.asarray(values, dtype=np.float64)
    return dict(median=round(float(np.median(v)), 3), min=round(float(v.min()), 3), max=round(float(v.max()), 3), runs=[round(float(t), 3) for t in v])


def kernel_ms(ctx, *names):
    st = ctx.kernel_stats()
    return sum(st[k][1] for k in names if k in st)


def timed(ctx, fn):
    ctx.reset_kernel_stats()
    t0 = time.perf_counter()
    fn()
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100_000_000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--resolutions", default="0.2,0.15,0.12,0.1,0.08,0.06,0.05,0.04,0.03")
    ap.add_argument("--tmp", default="/dev/shm" if os.path.isdir("/dev/shm") else tempfile.gettempdir())
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "terrain_bench.json"))
    args = ap.parse_args()
    n = args.points
    dev = torch.device("cuda", 0)
    ctx = pcv.Context(0)
    x, y, z, rgb = make_cloud(torch, n, seed=1, device=dev)
    tree = ctx.build(0.001, None, x, y, z, rgb)
    del x, y, z, rgb
    torch.cuda.empty_cache()
    meta = tree.meta()
    lo, hi = meta["bbox_min"], meta["bbox_max"]
    shapes = ctx.shapes([("all",)])
    batch = tree.query_batch(shapes)
    m = batch.num_points
    planes = dict(x=torch.empty(m, dtype=torch.float64, device=dev), y=torch.empty(m, dtype=torch.float64, device=dev),
                  z=torch.empty(m, dtype=torch.float64, device=dev), rgb=torch.empty((m, 3), dtype=torch.uint8, device=dev))
    batch.points(out=planes)
    torch.cuda.synchronize()

    def begin(stat, res):
        return ctx.terrain_begin(lo, hi, tile_size=TILE, resolution_m=res, statistic=stat, max_pool_bytes=POOL_CAP)

    # the resolution: between 1 000 and 5 000 touched tiles
    tried, res = {}, None
    for r in (float(v) for v in args.resolutions.split(",")):
        t = begin("max", r)
        t.add_points(planes["x"], planes["y"], planes["z"], planes["rgb"])
        tried[str(r)] = t.info()["tiles"]
        t.free()
        if 1000 <= tried[str(r)] <= 5000:
            res = r
            break
    if res is None:
        print(json.dumps({"error": "no resolution of --resolutions touches 1 000 to 5 000 tiles", "tiles_touched": tried}))
        return 1
    st = os.statvfs(args.tmp)
    if st.f_bavail * st.f_frsize < 2 * tried[str(res)] * TILE * TILE * 12:  # a small tmpfs: the system's temporary directory instead
        args.tmp = tempfile.gettempdir()
    tmp = tempfile.mkdtemp(prefix="terrain_bench_", dir=args.tmp)
    ctx.set_profiling(True)
    legs = ("accumulate_wall", "mark_kernel", "accum_kernel", "query_wall", "query_accum_kernel", "resolve_kernels", "mask_kernel", "finish_wall", "write_wall")
    ms = {s: {k: [] for k in legs} for s in STATS}
    xray = dict(wall=[], kernels=[])
    infos = {}
    for rnd in range(args.runs + 1):  # round 0 warms every leg up
        for stat in STATS:
            rec = {}
            t = begin(stat, res)
            rec["accumulate_wall"] = timed(ctx, lambda: t.add_points(planes["x"], planes["y"], planes["z"], planes["rgb"]))
            rec["mark_kernel"], rec["accum_kernel"] = kernel_ms(ctx, "terrain_mark_kernel"), kernel_ms(ctx, "terrain_accum_kernel")
            rec["finish_wall"] = timed(ctx, t.finish)
            rec["resolve_kernels"], rec["mask_kernel"] = kernel_ms(ctx, "terrain_count_kernel", "terrain_resolve_kernel"), kernel_ms(ctx, "terrain_mask_kernel")
            out_dir = os.path.join(tmp, stat)
            rec["write_wall"] = timed(ctx, lambda: t.write(out_dir))
            infos[stat] = t.info()
            written = sum(os.path.getsize(os.path.join(out_dir, f)) for f in os.listdir(out_dir))
            infos[stat]["directory_bytes"] = written
            shutil.rmtree(out_dir)
            t.free()
            t = begin(stat, res)
            rec["query_wall"] = timed(ctx, lambda: t.add(batch))
            rec["query_accum_kernel"] = kernel_ms(ctx, "terrain_accum_kernel")
            t.free()
            if rnd:
                for k, v in rec.items():
                    ms[stat][k].append(v)
        ctx.reset_kernel_stats()
        t0 = time.perf_counter()
        xt = tree.xray_tiles(TILE, res, "colored")
        wall = (time.perf_counter() - t0) * 1e3
        if rnd:
            xray["wall"].append(wall)
            xray["kernels"].append(sum(v[1] for v in ctx.kernel_stats().values()))
        xray_tiles = xt.num_created
        xt.free()
    os.rmdir(tmp)
    out = {"tool": "tools/terrain_bench.py", "build_hash": build_hash(), "device": torch.cuda.get_device_name(0),
           "cloud": f"config 2: {n} Gaussian-cluster points (bench.make_cloud, seed 1), octree resolution 0.001, AllPoints = {m} points",
           "tile_size": TILE, "resolution_m": res, "tiles_touched_by_resolution": tried, "runs": args.runs, "tmp": args.tmp, "statistics": {}}
    for stat in STATS:
        inf = infos[stat]
        kept = inf["points_added"] - inf["outside"]
        ops, nbytes = ATOMICS[stat]
        accum = float(np.median(ms[stat]["accum_kernel"]))
        rec = {k: spread(v) for k, v in ms[stat].items()}
        rec.update(points_added=inf["points_added"], outside=inf["outside"], set_vertices=inf["set_vertices"], rendered_quads=inf["rendered_quads"],
                   tiles=inf["tiles"], directory_bytes=inf["directory_bytes"],
                   atomic_ops_per_s=round(kept * ops / (accum * 1e-3), 1), atomic_bytes_per_s=round(kept * nbytes / (accum * 1e-3), 1),
                   points_per_s_accum_kernel=round(kept / (accum * 1e-3), 1),
                   accum_kernel_input_bytes_per_s=round(inf["points_added"] * 27 / (accum * 1e-3), 1),
                   write_bytes_per_s=round(inf["directory_bytes"] / (float(np.median(ms[stat]["write_wall"])) * 1e-3), 1))
        out["statistics"][stat] = rec
    out["xray_colored_yardstick"] = dict(tile_size_px=TILE, pixel_size_m=res, created_tiles=xray_tiles, wall_ms=spread(xray["wall"]),
                                         kernel_ms_total=spread(xray["kernels"]))
    for stat in STATS:
        whole = float(np.median(ms[stat]["query_wall"])) + float(np.median(ms[stat]["finish_wall"]))
        out["statistics"][stat]["query_plus_finish_over_xray_colored_wall"] = round(whole / float(np.median(xray["wall"])), 3)
    batch.free()
    shapes.free()
    tree.free()
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
