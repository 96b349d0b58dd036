#!/usr/bin/env python
"""Map tiles, measured (GPU box; there is no CPU fallback). The cloud is the config-5 distribution: --points (100 M)
Gaussian-cluster points (bench.py's generator, seed 1, colour) offset to ECEF magnitudes, in an octree of resolution 0.001; the
S2 leg reads the same generator in an S2 cell cloud of level 20, moved out along the offset to a radius of 6 371 km (config 5's
offset lies below what the S2 split takes as ECEF). The layer takes AllPoints at --zoom (20).
One process, a warm-up round and then --runs rounds in which the sources and their legs alternate; medians and spreads:
  planes       add_points over device planes (the batch's points, copied out once): wall, and maptiles_project_kernel,
               maptiles_mark_kernel, maptiles_accum_kernel alone (ctx.kernel_stats)
  octree, s2   the same points through add_query_batch: staging (the row packer and the unpack pass per piece) included
  resolve      finish: wall and maptiles_resolve_kernel
  parents      build_parents down to zoom - 8: wall and the parent kernel
  write        write onto tmpfs, stored and deflate
Derived: f64 instructions per second of the project pass (358 per point, the chain's count) against the 39.3 T/s roof; atomic
operations per second of the accumulate pass (two 8-byte adds per drawn point); the colliding share of lanes: of the first
--collide-points points in stream order, taken 64 at a time as the accumulate kernel's waves take them, the lanes whose pixel an
earlier lane of the same wave already holds (what combining lanes before the atomic could save).
Yardsticks in the same process and rounds, for the README and no pass criterion: the terrain MEAN accumulate of the same planes
(identity frame with the origin at the cloud's height, resolution = the zoom's ground pixel at the cloud's latitude, tile size
256) and the `colored` xray leaf build of the same tree at that pixel size.
Prints one JSON line and writes it to --out.

usage: python tools/maptiles_bench.py [--points N] [--zoom Z] [--runs R] [--no-s2] [--tmp DIR] [--out FILE]"""
import argparse
import json
import math
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

OFFSET = (-2.7e6, -4.3e6, 3.8e6)  # bench.py's config 5
CHAIN_F64 = 358                   # f64 instructions per point of the chain (README, the web-mercator point test)
F64_ROOF = 39.3e12
POOL_CAP = 64 << 30
PROJECT, MARK, ACCUM, RESOLVE, PARENT = ("maptiles_project_kernel", "maptiles_mark_kernel", "maptiles_accum_kernel", "maptiles_resolve_kernel",
                                         "maptiles_parent_kernel")


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


def colliding_share(zoom, x, y, z):
    """Of the points taken 64 at a time: the share of drawn lanes whose pixel an earlier lane of the same wave holds."""
    gx, gy, ok = pcv.map_tile_pixels(zoom, x, y, z)
    n = (len(gx) // 64) * 64
    key = np.where(ok[:n], gx[:n].astype(np.uint64) | (gy[:n].astype(np.uint64) << np.uint64(32)), np.uint64(0xffffffffffffffff)).reshape(-1, 64)
    key = np.sort(key, axis=1)
    drawn = key != np.uint64(0xffffffffffffffff)
    repeat = (key[:, 1:] == key[:, :-1]) & drawn[:, 1:]
    return float(repeat.sum()) / max(1, int(drawn.sum()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100_000_000)
    ap.add_argument("--zoom", type=int, default=20)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--collide-points", type=int, default=1 << 22)
    ap.add_argument("--no-s2", action="store_true")
    ap.add_argument("--tmp", default="/dev/shm" if os.path.isdir("/dev/shm") else tempfile.gettempdir())
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "maptiles_bench.json"))
    args = ap.parse_args()
    n, zoom = args.points, args.zoom
    min_zoom = max(0, zoom - 8)
    dev = torch.device("cuda", 0)
    ctx = pcv.Context(0)
    x, y, z, rgb = make_cloud(torch, n, seed=1, device=dev, offset=OFFSET)
    s2, s2_error = None, None
    if not args.no_s2:
        try:
            # config 5's offset lies 31 km below the ellipsoid, outside what S2Splitter takes as ECEF: the S2 leg reads the same
            # generator moved out along the offset to a radius of 6 371 km
            scale = 6.371e6 / math.sqrt(sum(v * v for v in OFFSET))
            sx, sy, sz, srgb = make_cloud(torch, n, seed=1, device=dev, offset=tuple(v * scale for v in OFFSET))
            s2 = ctx.s2_split(dict(x=sx, y=sy, z=sz, color=srgb), 20)
            del sx, sy, sz, srgb
        except Exception as e:  # the cloud is the subject, not the split: the octree legs still run
            s2_error = f"{type(e).__name__}: {e}"
    tree = ctx.build(0.001, None, x, y, z, rgb)
    del x, y, z, rgb
    torch.cuda.empty_cache()
    meta = tree.meta()
    lo, hi = meta["bbox_min"], meta["bbox_max"]
    shapes = ctx.shapes([("all",)])
    batch = tree.query_batch(shapes)
    s2_batch = s2.query_batch(shapes) if s2 is not None else None
    m = batch.num_points
    planes = dict(x=torch.empty(m, dtype=torch.float64, device=dev), y=torch.empty(m, dtype=torch.float64, device=dev),
                  z=torch.empty(m, dtype=torch.float64, device=dev), rgb=torch.empty((m, 3), dtype=torch.uint8, device=dev))
    batch.points(out=planes)
    torch.cuda.synchronize()
    k = min(m, args.collide_points)
    collide = colliding_share(zoom, *(planes[a][:k].cpu().numpy() for a in "xyz"))
    lat = math.asin(OFFSET[2] / math.sqrt(sum(v * v for v in OFFSET)))
    pixel_m = 2.0 * math.pi * 6378137.0 * math.cos(lat) / (256 << zoom)

    def begin():
        return ctx.map_tiles_begin(zoom, max_pool_bytes=POOL_CAP)

    st = os.statvfs(args.tmp)
    if st.f_bavail * st.f_frsize < (8 << 30):  # a small tmpfs: the system's temporary directory instead
        args.tmp = tempfile.gettempdir()
    tmp = tempfile.mkdtemp(prefix="maptiles_bench_", dir=args.tmp)
    ctx.set_profiling(True)
    legs = ("planes_wall", "project_kernel", "mark_kernel", "accum_kernel", "octree_wall", "octree_kernels", "s2_wall", "s2_kernels", "finish_wall",
            "resolve_kernel", "parents_wall", "parent_kernel", "write_stored_wall", "write_deflate_wall", "terrain_mean_wall", "terrain_mean_accum_kernel",
            "xray_colored_wall", "xray_colored_kernels")
    ms = {leg: [] for leg in legs}
    info, sizes, xray_tiles, terrain_info = None, {}, 0, None
    for rnd in range(args.runs + 1):  # round 0 warms every leg up
        rec = {}
        t = begin()
        rec["planes_wall"] = timed(ctx, lambda: t.add_points(planes["x"], planes["y"], planes["z"], planes["rgb"]))
        rec["project_kernel"], rec["mark_kernel"], rec["accum_kernel"] = kernel_ms(ctx, PROJECT), kernel_ms(ctx, MARK), kernel_ms(ctx, ACCUM)
        rec["finish_wall"] = timed(ctx, t.finish)
        rec["resolve_kernel"] = kernel_ms(ctx, RESOLVE)
        rec["parents_wall"] = timed(ctx, lambda: t.build_parents(min_zoom))
        rec["parent_kernel"] = kernel_ms(ctx, PARENT)
        info = t.info()
        for png in ("stored", "deflate"):
            out_dir = os.path.join(tmp, png)
            rec[f"write_{png}_wall"] = timed(ctx, lambda: t.write(out_dir, png=png))
            sizes[png] = sum(os.path.getsize(os.path.join(d, f)) for d, _, fs in os.walk(out_dir) for f in fs)
            shutil.rmtree(out_dir)
        t.free()
        for name, b in (("octree", batch), ("s2", s2_batch)):
            if b is None:
                continue
            t = begin()
            rec[f"{name}_wall"] = timed(ctx, lambda: t.add_query_batch(b))
            rec[f"{name}_kernels"] = kernel_ms(ctx, PROJECT, MARK, ACCUM, "maptiles_unpack_kernel", "ply_rows_kernel")
            t.free()
        tr = ctx.terrain_begin(lo, hi, tile_size=256, resolution_m=pixel_m, origin=(0.0, 0.0, OFFSET[2]), statistic="mean", max_pool_bytes=POOL_CAP)  # MEAN keeps |z - origin| < 2^21
        rec["terrain_mean_wall"] = timed(ctx, lambda: tr.add_points(planes["x"], planes["y"], planes["z"], planes["rgb"]))
        rec["terrain_mean_accum_kernel"] = kernel_ms(ctx, "terrain_accum_kernel")
        terrain_info = tr.info()
        tr.free()
        ctx.reset_kernel_stats()
        t0 = time.perf_counter()
        xt = tree.xray_tiles(256, pixel_m, "colored")
        rec["xray_colored_wall"] = (time.perf_counter() - t0) * 1e3
        rec["xray_colored_kernels"] = sum(v[1] for v in ctx.kernel_stats().values())
        xray_tiles = xt.num_created
        xt.free()
        if rnd:
            for leg, v in rec.items():
                ms[leg].append(v)
    os.rmdir(tmp)
    med = lambda leg: float(np.median(ms[leg]))
    out = {"tool": "tools/maptiles_bench.py", "build_hash": build_hash(), "device": torch.cuda.get_device_name(0),
           "cloud": f"config-5 distribution: {n} Gaussian-cluster points (bench.make_cloud, seed 1) offset by {OFFSET}, octree resolution 0.001, "
                    f"AllPoints = {m} points",
           "zoom": zoom, "min_zoom": min_zoom, "ground_pixel_m": round(pixel_m, 6), "runs": args.runs, "tmp": args.tmp, "s2_error": s2_error,
           "points_added": info["points_added"], "dropped": info["dropped"], "drawn": info["drawn"], "tiles": info["tiles"],
           "directory_bytes": sizes, "legs_ms": {leg: spread(v) for leg, v in ms.items() if v},
           "colliding_lane_share": round(collide, 5), "colliding_lane_sample_points": k}
    out["derived"] = dict(
        project_f64_instructions_per_s=round(m * CHAIN_F64 / (med("project_kernel") * 1e-3), 1),
        project_share_of_f64_roof=round(m * CHAIN_F64 / (med("project_kernel") * 1e-3) / F64_ROOF, 4),
        accum_atomics_per_s=round(info["drawn"] * 2 / (med("accum_kernel") * 1e-3), 1),
        accum_points_per_s=round(info["drawn"] / (med("accum_kernel") * 1e-3), 1),
        planes_points_per_s_wall=round(m / (med("planes_wall") * 1e-3), 1))
    kept = terrain_info["points_added"] - terrain_info["outside"]
    out["terrain_mean_yardstick"] = dict(resolution_m=round(pixel_m, 6), tiles=terrain_info["tiles"], kept_points=kept,
                                         atomics_per_s=round(kept * 5 / (med("terrain_mean_accum_kernel") * 1e-3), 1))
    out["xray_colored_yardstick"] = dict(tile_size_px=256, pixel_size_m=round(pixel_m, 6), created_tiles=xray_tiles)
    batch.free()
    if s2_batch is not None:
        s2_batch.free()
        s2.free()
    shapes.free()
    tree.free()
    print(json.dumps(out))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
